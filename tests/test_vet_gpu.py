"""GPU suite (run with -m gpu on an MI355X): Matcher.vet / Matcher.vet_points / Matcher.track_pixels (vsm_vet_run,
vsm_points_vet, vsm_tracks_pixels) - every observation's reprojection residual, the verdicts per observation, track and frame,
and the pruned track set, a 16-lane group per track.  Every result is compared with tests/vet_ref.py (the definition restated in
plain Python floats) and with vsm_host_vet, every array by its bytes.  The cases are those of tests/vet_cases.py, proven on the
CPU by test_vet_cpu.py; their sizes are the smallest at which the kernels can go wrong: track lengths on either side of the
group's 16 lanes, of its second chunk and of many chunks, track counts on either side of a wave's four and a workgroup's sixteen
groups and of a second level of nothing (the scan has one level below 256 tracks; test_regrow's scene has two)."""
import numpy as np
import pytest

import motions_cases as MO
import points_cases as PC
import points_ref as PR
import resect_ref as RR
import tracks_ref as TR
import vet_cases as VC
import vet_ref as V
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def vm():
    m = pkg("visomatch")
    L = m.lib()  # raises if the HIP library is missing: no silent fallback
    assert hasattr(L, "vsm_vet_run") and hasattr(L, "vsm_points_vet")
    return m


@pytest.fixture(scope="module")
def matcher(vm):
    m = vm.Matcher()
    yield m
    m.close()


def last_vetting(m):
    return m._vet_result(0, "the last result")


def check_stats(vm, got, want):
    assert [got.stats[k] for k in vm.VET_STATS] == np.bincount(want.code, minlength=5).tolist() + np.bincount(want.status, minlength=4).tolist(), got.stats


# ---- 1: every case against the restatement and the host view ---------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(VC.cases()))
def test_cases(vm, matcher, name):
    a, kw = VC.cases()[name].args()
    want = VC.reference(name)
    got = matcher.vet(*a, **kw)
    V.assert_same(got, want, (name, "device against the restatement"))
    V.assert_same(vm.host_vet(*a, **kw), got, (name, "host view against the device"))
    check_stats(vm, got, want)
    if len(want.status):
        assert got.timings["kernels_us"] > 0 and got.timings["gather_us"] > 0


def test_the_planted_scene_prunes_to_the_clean_one(vm, matcher):
    planted, clean = VC.planted_case()
    off, fr, uv = matcher.vet(*planted.args()[0]).prune(planted.obs_frames, planted.uv)
    assert off.tobytes() == clean.offsets.tobytes() and fr.tobytes() == clean.obs_frames.tobytes() and uv.tobytes() == clean.uv.tobytes()


# ---- 2: on the handle's own track and point results ------------------------------------------------------------------------

SCENES = ["scene_type-1", "noise_half_px", "merged_tracks"]
RESECT = dict(min_observations=6)


@pytest.mark.parametrize("name", SCENES)
def test_vet_points(vm, matcher, name):
    c = PC.cases()[name]
    tr = matcher.tracks(len(c.poses), c.pairs, c.lists, 0, 2)
    pts = matcher.track_points(c.poses, c.f, c.cu, c.cv, lists=c.lists, params=c.params)
    rs = matcher.resect_points(c.poses, c.f, c.cu, c.cv, lists=c.lists, params=RESECT)
    fr, uv = matcher.track_pixels(lists=c.lists)
    assert fr.tobytes() == np.ascontiguousarray(tr.obs[:, 0]).tobytes() and uv.tobytes() == PC.gather(tr.obs, c.lists, 0).tobytes()
    got = matcher.vet_points(c.poses, c.f, c.cu, c.cv, lists=c.lists)
    assert len(got) == len(tr) and len(got.code) == len(fr) and got.stats["obs_inlier"] > 0 and got.stats["tracks_unused"] == int((pts.status != 0).sum())
    want = matcher.vet(c.poses, c.f, c.cu, c.cv, tr.offsets, fr, uv, pts.xyz, use=pts.kept)
    V.assert_same(got, want, (name, "vet_points against vet on the arrays of track_pixels"))
    V.assert_same(vm.host_vet(c.poses, c.f, c.cu, c.cv, tr.offsets, fr, uv, pts.xyz, use=pts.kept), got, (name, "host view"))
    TR.assert_same(matcher._tracks_result(0, "the last result", len(c.pairs)), tr, "the track result is untouched")
    PR.assert_same(matcher._points_result(0, "the last result"), pts, "the point result is untouched")
    RR.assert_same(matcher._resect_result(0, "the last result"), rs, "the resection result is untouched")


def test_not_ready_and_errors_keep_the_last_result(vm):
    m = vm.Matcher()
    c = PC.cases()["merged_tracks"]
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):  # neither result
        m.vet_points(c.poses, c.f, c.cu, c.cv, lists=c.lists)
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):
        m.track_pixels(lists=c.lists)
    tr = m.tracks(len(c.poses), c.pairs, c.lists, 0, 2)
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):  # no point result
        m.vet_points(c.poses, c.f, c.cu, c.cv, lists=c.lists)
    assert len(last_vetting(m)) == 0 and len(last_vetting(m).code) == 0
    pts = m.track_points(c.poses, c.f, c.cu, c.cv, lists=c.lists, params=c.params)
    good = m.vet_points(c.poses, c.f, c.cu, c.cv, lists=c.lists)
    nan = float("nan")
    # argument errors: nothing enqueued, the last result kept
    for kw in (dict(params=dict(min_observations=0)), dict(params=dict(max_residual=-1.0)), dict(params=dict(max_residual=nan)), dict(params=dict(min_depth=nan)),
               dict(params=vm._NO_PARAMS), dict(counts=[len(l) + 1 for l in c.lists])):
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            m.vet_points(c.poses, c.f, c.cu, c.cv, lists=c.lists, **kw)
        V.assert_same(last_vetting(m), good, "the last good result")
    s = VC.cases()["counts_5"]
    (poses, f, cu, cv, off, fr, uv, xyz), kw = s.args()
    bad_fr = fr.copy()
    bad_fr[3] = len(poses)
    for args, over in (((poses, f, cu, cv, off, bad_fr, uv, xyz), {}), ((poses, f, cu, cv, off, fr, uv, None), {}), ((poses, f, cu, cv, off, fr, uv, xyz), {"n_tracks": -2}),
                       ((poses, f, cu, cv, off, fr, uv, xyz), {"params": dict(min_observations=0)}), ((poses, f, cu, cv, off, fr, uv, xyz), {"params": vm._NO_PARAMS})):
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            m.vet(*args, **{**kw, **over})
        V.assert_same(last_vetting(m), good, "the last good result")
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):  # lists == NULL: these tracks did not come from a pairs run
        m.vet_points(c.poses, c.f, c.cu, c.cv)
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):
        m.track_pixels()
    # a track call with another T: the point result is not these tracks'
    other = PC.cases()["noise_half_px"]
    tr2 = m.tracks(len(other.poses), other.pairs, other.lists, 0, 2)
    assert len(tr2) != len(tr)
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):
        m.vet_points(other.poses, other.f, other.cu, other.cv, lists=other.lists)
    V.assert_same(last_vetting(m), good, "the last good result")
    PR.assert_same(m._points_result(0, "the last result"), pts, "the point result is untouched")
    m.close()


# ---- 3: a larger scene after a small one ----------------------------------------------------------------------------------------

def test_regrow(vm):
    """a handle's first call sizes the stage for five tracks; the second brings 600 (a second level of the scan) and longer ones"""
    m = vm.Matcher()
    a, kw = VC.cases()["counts_5"].args()
    V.assert_same(m.vet(*a, **kw), VC.reference("counts_5"), "the small scene")
    rng = np.random.default_rng(50)
    true = PC.camera_path(6)
    pts = VC.RC.visible_points(600, rng)
    big = VC.Case(true, [VC.noisy_track(true, X, [j % 6 for j in range(int(rng.integers(0, 40)))], rng, every=5) for X in pts], pts)
    a, kw = big.args()
    got = m.vet(*a, **kw)
    want = vm.host_vet(*a, **kw)
    V.assert_same(got, want, "the large scene against the host view")
    assert got.stats["tracks_kept"] > 256 and got.stats["obs_gated"] > 1000 and len(got.kept_index) == got.stats["obs_inlier"] - int(got.n_in[got.status != 0].sum())
    a, kw = VC.cases()["counts_5"].args()
    V.assert_same(m.vet(*a, **kw), VC.reference("counts_5"), "the small scene again")
    m.close()


# ---- 4: from images -----------------------------------------------------------------------------------------------------------------

def test_from_images(vm, synth):
    """match_pairs -> pair_tracks -> pair_motions -> chain_poses -> track_points -> vet_points -> prune -> triangulate on the small
    street clip of the motions tests.  The vetting equals host_vet on the same inputs; on the pruned arrays every track of length 0
    is too short for a point and no other is, nor has one an observation without a pose; and the kept tracks' summed squares at the
    new points are no larger than they were at the old ones: the new points minimise exactly that sum."""
    frames = MO.road_frames(synth)
    par = MO.road_params()
    m = vm.Matcher()
    lists = m.match_pairs(frames, None, MO.ROAD_PAIRS, 0)
    tr = m.pair_tracks()
    mot = m.pair_motions(par, bucket=True)
    poses, valid, _ = vm.chain_poses(MO.ROAD_N, MO.ROAD_PAIRS, mot.T, mot.rc)
    pts = m.track_points(poses, par.f, par.cu, par.cv, pose_valid=valid, params=MO.ROAD_POINT_PARAMS)
    got = m.vet_points(poses, par.f, par.cu, par.cv, pose_valid=valid)
    print("street clip:", got.stats, got.timings, "frames", got.frame_counts.tolist())
    fr, uv = m.track_pixels()
    assert fr.tobytes() == np.ascontiguousarray(tr.obs[:, 0]).tobytes() and uv.tobytes() == PC.gather(tr.obs, lists, 0).tobytes()
    V.assert_same(got, vm.host_vet(poses, par.f, par.cu, par.cv, tr.offsets, fr, uv, pts.xyz, use=pts.kept, pose_valid=valid), "vet_points against host_vet")
    V.assert_same(m.vet_points(poses, par.f, par.cu, par.cv, lists=lists, pose_valid=valid), got, "the lists given explicitly")
    TR.assert_same(m._tracks_result(0, "the last result", len(MO.ROAD_PAIRS)), tr, "the track result is untouched")
    PR.assert_same(m._points_result(0, "the last result"), pts, "the point result is untouched")
    assert got.stats["tracks_kept"] > 0
    off, pfr, puv = got.prune(fr, uv)
    assert off[-1] == len(got.kept_index) == len(pfr)
    again = m.triangulate(poses, par.f, par.cu, par.cv, off, pfr, puv, pose_valid=valid, params=MO.ROAD_POINT_PARAMS)
    length = np.diff(off)
    assert ((again.status == 3) == (length == 0)).all() and (again.status != 2).all() and (again.status != 1).all()
    both = got.kept & again.kept
    after = m.vet(poses, par.f, par.cu, par.cv, off, pfr, puv, again.xyz, use=both, pose_valid=valid, params=dict(max_residual=0.0))
    both &= after.n_in == length  # (the two sums run over the same observations: none has gone behind its camera)
    print("kept tracks with a point before and after:", int(both.sum()), "ss", float(got.ss[both].sum()), "->", float(after.ss[both].sum()))
    assert both.any() and after.ss[both].sum() <= got.ss[both].sum()
    m.close()
