"""GPU suite (run with -m gpu on an MI355X): Matcher.adjust / Matcher.adjust_points (vsm_adjust_run, vsm_points_adjust) - poses and
points adjusted jointly by the kernels of csrc/vsm_ba.hip.  Every result is compared with tests/ba_ref.py (the definition
restated in plain Python floats) and with vsm_host_adjust: every int equal, every double equal by its bytes.  The cases are
those of tests/ba_cases.py, proven on the CPU by test_ba_cpu.py; their sizes are the smallest at which the kernels can go
wrong (row counts on either side of the 256 lanes and of their second round, track counts on either side of a workgroup of
lanes, frame counts of 1, 2, 3 and 9, every status in one grid, every exit of the solve and of the call; frame counts on
either side of 256 / 6, 512 / 6 and 256, and 513, for the scalar products' partial sums and the lane-per-frame loops and grids).
test_long_run runs two scenes to the minimum, against the host view and the dense reference of tests/ba_dense.py."""
import numpy as np
import pytest

import ba_cases as BC
import ba_ref as B
import motions_cases as MO
import points_cases as PC
import points_ref as PR
import resect_cases as RC
import resect_ref as R
import tracks_ref as TR
import vet_ref as VR
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def vm():
    m = pkg("visomatch")
    L = m.lib()  # raises if the HIP library is missing: no silent fallback
    assert hasattr(L, "vsm_adjust_run") and hasattr(L, "vsm_points_adjust")
    return m


@pytest.fixture(scope="module")
def matcher(vm):
    m = vm.Matcher()
    yield m
    m.close()


def last_adjustment(m):
    return m._adjust_result(0, "the last result")


# ---- 1: every case against the restatement and the host view ---------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(BC.cases()))
def test_cases(vm, matcher, name):
    a, kw = BC.cases()[name].args()
    want = BC.reference(name)
    got = matcher.adjust(*a, **kw)
    B.assert_same(got, want, (name, "device against the restatement"))
    B.assert_same(vm.host_adjust(*a, **kw), got, (name, "host view against the device"))
    assert got.timings["kernels_us"] > 0 and got.timings["group_us"] > 0


@pytest.mark.parametrize("name", ["band_257_held", "converges", "dense_257", "first_step_rejected", "grid", "lambda_max"])
def test_the_schedule_does_not_show(vm, name):
    """every launch of max_rounds rounds enqueued at once, the control block turning the launches behind the call's stop into
    no-ops, against the default, a wait per round: the same bytes"""
    a, kw = BC.cases()[name].args()
    m = vm.Matcher()
    m.set_option("adjust_fixed", 1)
    B.assert_same(m.adjust(*a, **kw), BC.reference(name), (name, "fixed schedule against the restatement"))
    m.close()


def test_pool_chunks_against_one_chunk(vm, matcher):
    """the rows grouped in four chunks on the pool against the host view's one chunk: the same rows in the same places"""
    a, kw = RC.pool_chunks_case().args()
    kw["params"] = dict(BC.QUICK, max_rounds=2, cg_iters=5)
    got = matcher.adjust(*a, **kw)
    assert got.rows.tolist() == [416] * 4 and len(got.history) >= 1
    B.assert_same(got, vm.host_adjust(*a, **kw), "four chunks on the device path against the host view")


@pytest.mark.parametrize("seed", sorted(BC.LONG_SCENES))
def test_long_run(vm, matcher, seed):
    """to the minimum: some twenty rounds, rejected ones between accepted ones, lambda up and down, thirty and more iterations
    of the solve in a round - too long for the restatement.  The device equals the host view, byte for byte, and meets
    tests/ba_dense.py, the dense reference with its own derivatives, within the limits the host view is held to."""
    c, _, _ = BC.long_case(seed)
    a, kw = c.args()
    want = vm.host_adjust(*a, **kw)
    got = matcher.adjust(*a, **kw)
    B.assert_same(got, want, (seed, "device against the host view"))
    accepted, iters = got.history["accepted"].tolist(), got.history["cg_iters"].tolist()
    print("long run:", seed, "accepted", accepted, "cg_iters", iters, "lambda", got.history["lambda"].tolist())
    assert got.stats["stop"] == 1 and any(a == 0 and 1 in accepted[k:] for k, a in enumerate(accepted)), accepted
    assert max(iters) > 20
    BC.against_the_dense_reference(got, seed, "device")


def test_long_run_on_the_fixed_schedule(vm):
    """every launch of twelve rounds of up to 64 iterations enqueued at once; the run needs eight rounds and 42 iterations"""
    c, _, _ = BC.long_case(72)
    a, kw = c.args()
    kw["params"] = dict(BC.LONG, max_rounds=12, cg_iters=64)
    want = vm.host_adjust(*a, **kw)
    assert want.stats["stop"] == 1 and len(want.history) < 12 and 20 < max(want.history["cg_iters"]) < 64
    m = vm.Matcher()
    m.set_option("adjust_fixed", 1)
    got = m.adjust(*a, **kw)
    m.close()
    B.assert_same(got, want, "fixed schedule against the host view")
    BC.against_the_dense_reference(got, 72, "device, fixed schedule")


# ---- 2: on the handle's own track and point results ----------------------------------------------------------------------------

SCENES = ["scene_type-1", "noise_half_px", "merged_tracks"]
ADJUST = dict(min_observations=6, max_rounds=4, cg_iters=20, max_residual=10.0)  # (the gate: scene_type-1 keeps points a few centimetres from a camera)
RESECT = dict(min_observations=6)


@pytest.mark.parametrize("name", SCENES)
def test_adjust_points(vm, matcher, name):
    c = PC.cases()[name]
    tr = matcher.tracks(len(c.poses), c.pairs, c.lists, 0, 2)
    pts = matcher.track_points(c.poses, c.f, c.cu, c.cv, lists=c.lists, params=c.params)
    poses = RC.perturb(c.poses, np.random.default_rng(5), 2e-3, 0.01)
    refine = BC.root_fixed(len(poses))
    res = matcher.resect_points(poses, c.f, c.cu, c.cv, lists=c.lists, refine=refine, params=RESECT)
    vet = matcher.vet_points(poses, c.f, c.cu, c.cv, lists=c.lists)
    got = matcher.adjust_points(poses, c.f, c.cu, c.cv, lists=c.lists, refine=refine, params=ADJUST)
    assert len(got) == len(c.poses) and got.stats["rounds_accepted"] >= 1 and got.stats["frames_free"] >= 1 and got.cost < got.history["cost_before"][0]
    uv = PC.gather(tr.obs, c.lists, 0)
    want = matcher.adjust(poses, c.f, c.cu, c.cv, tr.offsets, tr.obs[:, 0], uv, pts.xyz, use=pts.kept, refine=refine, params=ADJUST)
    B.assert_same(got, want, (name, "adjust_points against adjust on the same arrays"))
    B.assert_same(vm.host_adjust(poses, c.f, c.cu, c.cv, tr.offsets, tr.obs[:, 0], uv, pts.xyz, use=pts.kept, refine=refine, params=ADJUST), got, (name, "host view"))
    assert got.xyz[~pts.kept].tobytes() == pts.xyz[~pts.kept].tobytes() and got.poses[0].tobytes() == np.ascontiguousarray(poses[0]).tobytes()
    TR.assert_same(matcher._tracks_result(0, "the last result", len(c.pairs)), tr, "the track result is untouched")
    PR.assert_same(matcher._points_result(0, "the last result"), pts, "the point result is untouched")
    R.assert_same(matcher._resect_result(0, "the last result"), res, "the resect result is untouched")
    VR.assert_same(matcher._vet_result(0, "the last result"), vet, "the vet result is untouched")


def test_not_ready_and_errors_keep_the_last_result(vm):
    m = vm.Matcher()
    c = PC.cases()["merged_tracks"]
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):  # neither result
        m.adjust_points(c.poses, c.f, c.cu, c.cv, lists=c.lists)
    tr = m.tracks(len(c.poses), c.pairs, c.lists, 0, 2)
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):  # no point result
        m.adjust_points(c.poses, c.f, c.cu, c.cv, lists=c.lists)
    assert len(last_adjustment(m)) == 0 and len(last_adjustment(m).history) == 0
    pts = m.track_points(c.poses, c.f, c.cu, c.cv, lists=c.lists, params=c.params)
    good = m.adjust_points(c.poses, c.f, c.cu, c.cv, lists=c.lists, params=ADJUST)
    # argument errors: nothing enqueued, the last result kept
    for prm in (dict(min_observations=5), dict(max_rounds=0), dict(cg_iters=0), dict(lambda0=0.0), dict(cg_tol=float("nan")), dict(ftol=float("inf"))):
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            m.adjust_points(c.poses, c.f, c.cu, c.cv, lists=c.lists, params=prm)
        B.assert_same(last_adjustment(m), good, "the last good result")
    s = BC.cases()["frames_2"]
    (poses, f, cu, cv, off, fr, uv, xyz), kw = s.args()
    bad_fr = fr.copy()
    bad_fr[3] = len(poses)
    for args, over in (((poses, f, cu, cv, off, bad_fr, uv, xyz), {}), ((poses, f, cu, cv, off, fr, uv, None), {}), ((poses, f, cu, cv, off, fr, uv, xyz), {"n_tracks": -2}),
                       ((poses, f, cu, cv, off, fr, uv, xyz), {"params": dict(min_observations=5)})):
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            m.adjust(*args, **{**kw, **over})
        B.assert_same(last_adjustment(m), good, "the last good result")
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):  # lists == NULL: these tracks did not come from a pairs run
        m.adjust_points(c.poses, c.f, c.cu, c.cv, params=ADJUST)
    other = PC.cases()["noise_half_px"]
    tr2 = m.tracks(len(other.poses), other.pairs, other.lists, 0, 2)
    assert len(tr2) != len(tr)
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):  # a track call with another T: the point result is not these tracks'
        m.adjust_points(other.poses, other.f, other.cu, other.cv, lists=other.lists, params=ADJUST)
    B.assert_same(last_adjustment(m), good, "the last good result")
    PR.assert_same(m._points_result(0, "the last result"), pts, "the point result is untouched")
    m.close()


# ---- 3: from images ----------------------------------------------------------------------------------------------------------------

def test_from_images(vm, synth):
    """match_pairs -> pair_tracks -> pair_motions -> chain_poses -> track_points -> adjust_points on the small street clip of the
    motions tests, against host_adjust on the same inputs.  Equality, not accuracy, is the subject."""
    frames = MO.road_frames(synth)
    par = MO.road_params()
    m = vm.Matcher()
    lists = m.match_pairs(frames, None, MO.ROAD_PAIRS, 0)
    tr = m.pair_tracks()
    mot = m.pair_motions(par, bucket=True)
    poses, valid, _ = vm.chain_poses(MO.ROAD_N, MO.ROAD_PAIRS, mot.T, mot.rc)
    pts = m.track_points(poses, par.f, par.cu, par.cv, pose_valid=valid, params=MO.ROAD_POINT_PARAMS)
    refine = BC.root_fixed(MO.ROAD_N)
    prm = dict(min_observations=6, max_rounds=5, cg_iters=30, max_residual=4.0)
    got = m.adjust_points(poses, par.f, par.cu, par.cv, refine=refine, pose_valid=valid, params=prm)
    print("street clip:", got.stats, "rows", got.rows.tolist(), "active", got.active.tolist(), got.history, got.timings)
    assert len(got) == MO.ROAD_N and len(got.xyz) == len(tr) and got.frame_status[0] in (1, 2) and len(got.history) >= 1
    want = vm.host_adjust(poses, par.f, par.cu, par.cv, tr.offsets, tr.obs[:, 0], PC.gather(tr.obs, lists, 0), pts.xyz, use=pts.kept, refine=refine, pose_valid=valid,
                          params=prm)
    B.assert_same(got, want, "adjust_points against host_adjust on the same inputs")
    B.assert_same(m.adjust_points(poses, par.f, par.cu, par.cv, lists=lists, refine=refine, pose_valid=valid, params=prm), got, "the lists given explicitly")
    TR.assert_same(m._tracks_result(0, "the last result", len(MO.ROAD_PAIRS)), tr, "the track result is untouched")
    PR.assert_same(m._points_result(0, "the last result"), pts, "the point result is untouched")
    assert all(m.pair_matches(k).tobytes() == lists[k].tobytes() for k in range(len(MO.ROAD_PAIRS)))
    m.close()
