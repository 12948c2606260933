"""GPU suite (run with -m gpu on an MI355X): Matcher.resect / Matcher.resect_points / Matcher.alternate (vsm_resect_run,
vsm_points_resect) - every frame's pose refined against the points it sees, a 256-thread workgroup per frame.  Every result is
compared with tests/resect_ref.py (the definition restated in plain Python floats) and with vsm_host_resect: every int equal,
every double equal by its bytes.  The cases are those of tests/resect_cases.py, proven on the CPU by test_resect_cpu.py; their
sizes are the smallest at which the kernel can go wrong: row counts on either side of a wave, of the 256 lanes and of their
second round, frame counts of 1, 2 and 9 (each workgroup is one frame, so nothing larger is needed), every status in one grid."""
import numpy as np
import pytest

import motions_cases as MO
import points_cases as PC
import points_ref as PR
import resect_cases as RC
import resect_ref as R
import tracks_ref as TR
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def vm():
    m = pkg("visomatch")
    L = m.lib()  # raises if the HIP library is missing: no silent fallback
    assert hasattr(L, "vsm_resect_run") and hasattr(L, "vsm_points_resect")
    return m


@pytest.fixture(scope="module")
def matcher(vm):
    m = vm.Matcher()
    yield m
    m.close()


def last_resection(m):
    return m._resect_result(0, "the last result")


# ---- 1: every case against the restatement and the host view ---------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(RC.cases()))
def test_cases(vm, matcher, name):
    a, kw = RC.cases()[name].args()
    want = RC.reference(name)
    got = matcher.resect(*a, **kw)
    R.assert_same(got, want, (name, "device against the restatement"))
    R.assert_same(vm.host_resect(*a, **kw), got, (name, "host view against the device"))
    assert [got.stats[k] for k in vm.RESECT_STATUS] == np.bincount(want.status, minlength=7).tolist(), (name, got.stats)
    assert (got.refined == (want.status == 0)).all()
    if len(want.status):
        assert got.timings["kernels_us"] > 0 and got.timings["group_us"] > 0


def test_pool_chunks_against_one_chunk(vm, matcher):
    """the rows grouped in four chunks on the pool against the host view's one chunk: the same rows in the same places"""
    a, kw = RC.pool_chunks_case().args()
    got = matcher.resect(*a, **kw)
    assert got.rows.tolist() == [416] * 4 and got.status[0] == 2 and got.stats["refined"] >= 1
    R.assert_same(got, vm.host_resect(*a, **kw), "four chunks on the device path against the host view")


# ---- 2: on the handle's own track and point results ----------------------------------------------------------------------------

SCENES = ["scene_type-1", "noise_half_px", "merged_tracks"]
RESECT = dict(min_observations=6)


@pytest.mark.parametrize("name", SCENES)
def test_resect_points(vm, matcher, name):
    c = PC.cases()[name]
    tr = matcher.tracks(len(c.poses), c.pairs, c.lists, 0, 2)
    pts = matcher.track_points(c.poses, c.f, c.cu, c.cv, lists=c.lists, params=c.params)
    poses = RC.perturb(c.poses, np.random.default_rng(5), 2e-3, 0.01)
    got = matcher.resect_points(poses, c.f, c.cu, c.cv, lists=c.lists, params=RESECT)
    assert len(got) == len(c.poses) and got.stats["refined"] >= 1
    want = matcher.resect(poses, c.f, c.cu, c.cv, tr.offsets, tr.obs[:, 0], PC.gather(tr.obs, c.lists, 0), pts.xyz, use=pts.kept, params=RESECT)
    R.assert_same(got, want, (name, "resect_points against resect on the same arrays"))
    R.assert_same(vm.host_resect(poses, c.f, c.cu, c.cv, tr.offsets, tr.obs[:, 0], PC.gather(tr.obs, c.lists, 0), pts.xyz, use=pts.kept, params=RESECT), got,
                  (name, "host view"))
    TR.assert_same(matcher._tracks_result(0, "the last result", len(c.pairs)), tr, "the track result is untouched")
    PR.assert_same(matcher._points_result(0, "the last result"), pts, "the point result is untouched")


def test_not_ready_and_errors_keep_the_last_result(vm):
    m = vm.Matcher()
    c = PC.cases()["merged_tracks"]
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):  # neither result
        m.resect_points(c.poses, c.f, c.cu, c.cv, lists=c.lists)
    tr = m.tracks(len(c.poses), c.pairs, c.lists, 0, 2)
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):  # no point result
        m.resect_points(c.poses, c.f, c.cu, c.cv, lists=c.lists)
    assert len(last_resection(m)) == 0
    pts = m.track_points(c.poses, c.f, c.cu, c.cv, lists=c.lists, params=c.params)
    good = m.resect_points(c.poses, c.f, c.cu, c.cv, lists=c.lists, params=RESECT)
    # argument errors: nothing enqueued, the last result kept
    for kw in (dict(params=dict(min_observations=5)), dict(params=dict(max_updates=0)), dict(params=dict(eps=0.0)), dict(params=dict(eps=float("nan")))):
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            m.resect_points(c.poses, c.f, c.cu, c.cv, lists=c.lists, **kw)
        R.assert_same(last_resection(m), good, "the last good result")
    s = RC.cases()["frames_2"]
    (poses, f, cu, cv, off, fr, uv, xyz), kw = s.args()
    bad_fr = fr.copy()
    bad_fr[3] = len(poses)
    for args, over in (((poses, f, cu, cv, off, bad_fr, uv, xyz), {}), ((poses, f, cu, cv, off, fr, uv, None), {}), ((poses, f, cu, cv, off, fr, uv, xyz), {"n_tracks": -2}),
                       ((poses, f, cu, cv, off, fr, uv, xyz), {"params": dict(min_observations=5)})):
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            m.resect(*args, **{**kw, **over})
        R.assert_same(last_resection(m), good, "the last good result")
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):  # lists == NULL: these tracks did not come from a pairs run
        m.resect_points(c.poses, c.f, c.cu, c.cv, params=RESECT)
    # a track call with another T: the point result is not these tracks'
    other = PC.cases()["noise_half_px"]
    tr2 = m.tracks(len(other.poses), other.pairs, other.lists, 0, 2)
    assert len(tr2) != len(tr)
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):
        m.resect_points(other.poses, other.f, other.cu, other.cv, lists=other.lists, params=RESECT)
    R.assert_same(last_resection(m), good, "the last good result")
    PR.assert_same(m._points_result(0, "the last result"), pts, "the point result is untouched")
    m.close()


# ---- 3: the alternation is the four calls ---------------------------------------------------------------------------------------

def test_alternate(vm, matcher):
    c = PC.cases()["noise_half_px"]
    start = RC.perturb(c.poses, np.random.default_rng(6), 2e-3, 0.01)
    refine = np.ones(len(start), np.uint8)
    refine[0] = 0  # the root is pinned
    matcher.tracks(len(c.poses), c.pairs, c.lists, 0, 2)
    poses, pts, history = matcher.alternate(start, c.f, c.cu, c.cv, 2, refine=refine, point_params=c.params, resect_params=RESECT, lists=c.lists)
    p1 = matcher.track_points(start, c.f, c.cu, c.cv, lists=c.lists, params=c.params)
    r1 = matcher.resect_points(start, c.f, c.cu, c.cv, lists=c.lists, refine=refine, params=RESECT)
    p2 = matcher.track_points(r1.poses, c.f, c.cu, c.cv, lists=c.lists, params=c.params)
    r2 = matcher.resect_points(r1.poses, c.f, c.cu, c.cv, lists=c.lists, refine=refine, params=RESECT)
    assert poses.tobytes() == r2.poses.tobytes() and r2.poses[0].tobytes() == np.ascontiguousarray(start[0]).tobytes()
    PR.assert_same(pts, p2, "the last points")
    assert history == [(float(r.ss_before.sum()), float(r.ss_after.sum())) for r in (r1, r2)]
    assert r1.status[0] == 2 and (r1.status[1:] == 0).any() and len(p1) == len(p2)
    print("alternate:", history, r2.stats)


# ---- 4: from images ----------------------------------------------------------------------------------------------------------------

def test_from_images(vm, synth):
    """match_pairs -> pair_tracks -> pair_motions -> chain_poses -> track_points -> resect_points on the small street clip of the
    motions tests, against host_resect on the same inputs.  Equality, not accuracy, is the subject."""
    frames = MO.road_frames(synth)
    par = MO.road_params()
    m = vm.Matcher()
    lists = m.match_pairs(frames, None, MO.ROAD_PAIRS, 0)
    tr = m.pair_tracks()
    mot = m.pair_motions(par, bucket=True)
    poses, valid, _ = vm.chain_poses(MO.ROAD_N, MO.ROAD_PAIRS, mot.T, mot.rc)
    pts = m.track_points(poses, par.f, par.cu, par.cv, pose_valid=valid, params=MO.ROAD_POINT_PARAMS)
    refine = np.ones(MO.ROAD_N, np.uint8)
    refine[0] = 0
    got = m.resect_points(poses, par.f, par.cu, par.cv, refine=refine, pose_valid=valid, params=RESECT)
    print("street clip: frames by status", got.stats, "rows", got.rows.tolist(), "used", got.used.tolist(), got.timings)
    assert len(got) == MO.ROAD_N and sum(got.stats.values()) == MO.ROAD_N and got.status[0] in (1, 2)
    want = vm.host_resect(poses, par.f, par.cu, par.cv, tr.offsets, tr.obs[:, 0], PC.gather(tr.obs, lists, 0), pts.xyz, use=pts.kept, refine=refine, pose_valid=valid,
                          params=RESECT)
    R.assert_same(got, want, "resect_points against host_resect on the same inputs")
    R.assert_same(m.resect_points(poses, par.f, par.cu, par.cv, lists=lists, refine=refine, pose_valid=valid, params=RESECT), got, "the lists given explicitly")
    TR.assert_same(m._tracks_result(0, "the last result", len(MO.ROAD_PAIRS)), tr, "the track result is untouched")
    PR.assert_same(m._points_result(0, "the last result"), pts, "the point result is untouched")
    assert all(m.pair_matches(k).tobytes() == lists[k].tobytes() for k in range(len(MO.ROAD_PAIRS)))
    m.close()
