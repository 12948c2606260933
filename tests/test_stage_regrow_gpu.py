"""GPU suite (run with -m gpu on an MI355X): the staging of the tracks, points, resection and motions calls (csrc/vsm_stage.h)
when it grows and is then reused (the vetting's is in test_vet_gpu.test_regrow).  On one fresh handle every stage runs a tiny
input, then one more than 1.25 times larger in every block (pinned input, pinned output, device), then the tiny one again; the
stages then run interleaved, an argument error after the growth leaves the last result readable, and the calls that share one
round trip (points, resection, vetting) take their empty call on the grown blocks.  Every result is compared with the stage's
host view by the comparison of the stage's own suite (tracks_ref, points_ref, resect_ref, vet_ref, motions_cases); the
generators are theirs too."""
import functools

import numpy as np
import pytest

import motions_cases as MO
import points_cases as PC
import points_ref as PR
import resect_cases as RC
import resect_ref as RR
import tracks_ref as TR
import vet_cases as VC
import vet_ref as V
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vm():
    m = pkg("visomatch")
    m.lib()  # raises if the HIP library is missing: no silent fallback
    return m


@pytest.fixture(scope="module")
def matcher(vm):
    """the one handle of this file: its staging keeps what the tests before have grown"""
    m = vm.Matcher()
    yield m
    m.close()


# ---- the inputs: (small, large) per stage ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def track_inputs():
    """2 frames, 1 pair, 3 matches; 6 frames, 5 pairs, about 2000 matches per pair"""
    small = (2, [(0, 1)], [TR.make_list([0, 1, 2], [2, 1, 0])], 0, 2)
    rng = np.random.default_rng(41)
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
    lists = [TR.make_list(rng.integers(0, 2500, n), rng.integers(0, 2500, n)) for n in (1990, 2000, 2011, 1999, 2003)]
    return small, (6, pairs, lists, 0, 2)


@functools.lru_cache(maxsize=None)
def point_inputs():
    """2 tracks of 2 observations (points_cases' exact pixels); a scene of 3000 points over 6 frames: tracks of 2 to 6"""
    poses, uv = PC.exact_case()
    small = PC.Case(poses, [0, 2, 4], [0, 1, 0, 1], uv + uv, f=512.0, cu=320.0, cv=240.0)
    return small, PC.build_scene(6, 3000, seed=6)


@functools.lru_cache(maxsize=None)
def motion_inputs():
    """1 pair of 12 flow matches, 50 hypotheses; 3 pairs of about 300 matches, 200 hypotheses"""
    return ([MO.one("scene12")], MO.params(50)), ([MO.one("scene299"), MO.one("scene300"), MO.one("scene301")], MO.params(200))


@functools.lru_cache(maxsize=None)
def large_scene():
    """the scene of test_vet_gpu.test_regrow: six frames, 600 points, tracks of 0 to 39 observations, every fifth 50 px off ->
    (true poses, tracks, points)"""
    rng = np.random.default_rng(50)
    true = PC.camera_path(6)
    pts = VC.RC.visible_points(600, rng)
    return true, [VC.noisy_track(true, X, [j % 6 for j in range(int(rng.integers(0, 40)))], rng, every=5) for X in pts], pts


@functools.lru_cache(maxsize=None)
def resect_inputs():
    """resect_cases' one refined frame of 30 rows; the large scene from poses a little off, behind a gate of 8 px"""
    true, tracks, pts = large_scene()
    return RC.cases()["frames_1"], RC.Case(RC.perturb(true, np.random.default_rng(51)), tracks, pts, params=dict(max_residual=8.0), true_poses=true)


@functools.lru_cache(maxsize=None)
def vet_inputs():
    """vet_cases' five tracks; the large scene at its true poses"""
    true, tracks, pts = large_scene()
    return VC.cases()["counts_5"], VC.Case(true, tracks, pts)


def run_tracks(vm, m, args, what):
    got = m.tracks(*args)
    TR.assert_same(vm.host_tracks(*args), got, (what, "host view against the device"))
    return got


def run_points(vm, m, case, what):
    a, kw = case.args()
    got = m.triangulate(*a, **kw)
    PR.assert_same(vm.host_triangulate(*a, **kw), got, (what, "host view against the device"))
    return got


def run_resect(vm, m, case, what):
    a, kw = case.args()
    got = m.resect(*a, **kw)
    RR.assert_same(vm.host_resect(*a, **kw), got, (what, "host view against the device"))
    return got


def run_vet(vm, m, case, what):
    a, kw = case.args()
    got = m.vet(*a, **kw)
    V.assert_same(vm.host_vet(*a, **kw), got, (what, "host view against the device"))
    return got


def run_motions(vm, m, args, what):
    lists, par = args
    got = m.motions(lists, par)
    MO.assert_same(got, vm.host_pairs_motions(lists, par, threads=8), (what, "device against the host view"))
    assert got.stats["device_svd"] == 1, got.stats  # (no silent fallback to the host view)
    return got


def motions_bytes_equal(a, b, what):
    MO.assert_same(a, b, what)
    assert a.rc.tobytes() == b.rc.tobytes() and a.stage.tobytes() == b.stage.tobytes(), what


# ---- small, large, small again --------------------------------------------------------------------------------------------------------

def test_tracks_regrow(vm, matcher):
    small, large = track_inputs()
    first = run_tracks(vm, matcher, small, "small")
    assert len(first) == 3
    big = run_tracks(vm, matcher, large, "large")
    assert len(big) > 100 and big.stats["edges"] == sum(len(x) for x in large[2]) > 9000
    TR.assert_same(run_tracks(vm, matcher, small, "small again"), first, "the third result equals the first")


def test_points_regrow(vm, matcher):
    small, large = point_inputs()
    first = run_points(vm, matcher, small, "small")
    assert len(first) == 2 and first.kept.all()
    big = run_points(vm, matcher, large, "large")
    seg = np.diff(large.offsets)
    assert len(big) > 2500 and seg.min() >= 2 and seg.max() <= 6 and big.kept.any() and not big.kept.all()
    PR.assert_same(run_points(vm, matcher, small, "small again"), first, "the third result equals the first")


def test_resect_regrow(vm, matcher):
    small, large = resect_inputs()
    first = run_resect(vm, matcher, small, "small")
    assert len(first) == 1 and first.refined.all() and first.rows[0] == 30
    big = run_resect(vm, matcher, large, "large")
    assert len(big) == 6 and big.rows.min() > 1000 and big.refined.all() and (big.used < big.rows).all() and len(large.xyz) == 600
    RR.assert_same(run_resect(vm, matcher, small, "small again"), first, "the third result equals the first")


def test_motions_regrow(vm, matcher):
    small, large = motion_inputs()
    first = run_motions(vm, matcher, small, "small")
    assert len(first) == 1
    big = run_motions(vm, matcher, large, "large")
    assert (big.rc == 1).all()
    motions_bytes_equal(run_motions(vm, matcher, small, "small again"), first, "the third result equals the first")


# ---- no stage reads another's staging; an argument error after the growth ------------------------------------------------------------

def test_interleaved_and_errors(vm, matcher):
    (t_small, t_large), (p_small, p_large), (m_small, m_large) = track_inputs(), point_inputs(), motion_inputs()
    tr = run_tracks(vm, matcher, t_large, "tracks")
    mo = run_motions(vm, matcher, m_large, "motions")
    pt = run_points(vm, matcher, p_large, "points")
    tr2 = run_tracks(vm, matcher, t_small, "tracks again")
    # every stage's last result is still what its call returned
    motions_bytes_equal(matcher.last_motions(), mo, "the motions result after the other stages")
    PR.assert_same(matcher._points_result(0, "the last result"), pt, "the point result after the other stages")
    TR.assert_same(run_tracks(vm, matcher, t_large, "tracks, large again"), tr, "the large tracks again")
    # an argument error after the growth leaves the last result readable (test_bad_arguments_keep_the_last_result)
    good = run_tracks(vm, matcher, t_small, "tracks, small")
    TR.assert_same(good, tr2, "the small tracks again")
    L = TR.make_list
    for bad in ((2, [(0, 2)], [L([0], [0])], 0, 2), (2, [(0, 1)], [L([0], [-1])], 0, 2), (2, [(0, 1)], [L([0], [0])], 0, 0)):
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            matcher.tracks(*bad)
        TR.assert_same(matcher._tracks_result(0, "the last result", len(t_small[1])), good, "the last good result")
    a, kw = p_small.args()
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        matcher.triangulate(*a, **{**kw, "params": dict(min_track_length=0)})
    PR.assert_same(matcher._points_result(0, "the last result"), pt, "the last good points")
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        matcher.motions(m_small[0], None)
    motions_bytes_equal(matcher.last_motions(), mo, "the last good motions")


# ---- the calls that share one round trip: interleaved, and their empty call on grown blocks -------------------------------------------

def last_three(m):
    return m._points_result(0, "the last result"), m._resect_result(0, "the last result"), m._vet_result(0, "the last result")


def test_points_resect_vet_interleaved(vm, matcher):
    (p_small, p_large), (r_small, r_large), (v_small, v_large) = point_inputs(), resect_inputs(), vet_inputs()
    pt = run_points(vm, matcher, p_large, "points")
    rs = run_resect(vm, matcher, r_large, "resection")
    PR.assert_same(last_three(matcher)[0], pt, "the point result after the resection")
    ve = run_vet(vm, matcher, v_large, "vetting")
    assert ve.stats["tracks_kept"] > 256 and ve.stats["obs_gated"] > 1000
    PR.assert_same(last_three(matcher)[0], pt, "the point result after the vetting")
    RR.assert_same(last_three(matcher)[1], rs, "the resection result after the vetting")
    pt2 = run_points(vm, matcher, p_small, "points again")
    RR.assert_same(last_three(matcher)[1], rs, "the resection result after the second points call")
    V.assert_same(last_three(matcher)[2], ve, "the vetting result after the second points call")
    PR.assert_same(last_three(matcher)[0], pt2, "the second point result")


def test_empty_calls_on_grown_blocks(vm, matcher):
    """T = 0 for the points and the vetting, F = 0 for the resection: no round trip, empty arrays, zero stats"""
    (p_small, p_large), (r_small, r_large), (v_small, v_large) = point_inputs(), resect_inputs(), vet_inputs()
    poses = PC.camera_path(3)
    run_points(vm, matcher, p_large, "points, large")
    got = run_points(vm, matcher, PC.Case(poses, [0], [], np.zeros((0, 2), np.float32)), "points, no track")
    assert len(got) == 0 and got.xyz.shape == (0, 3) and len(got.angle) == 0 and set(got.stats.values()) == {0}
    assert got.timings["upload_us"] == 0 and got.timings["kernels_us"] == 0
    run_resect(vm, matcher, r_large, "resection, large")
    got = run_resect(vm, matcher, RC.cases()["no_frames"], "resection, no frame")
    assert len(got) == 0 and got.poses.shape == (0, 12) and len(got.rms_after) == 0 and set(got.stats.values()) == {0}
    assert got.timings["upload_us"] == 0 and got.timings["kernels_us"] == 0
    run_vet(vm, matcher, v_large, "vetting, large")
    got = run_vet(vm, matcher, VC.Case(poses, [], np.zeros((0, 3))), "vetting, no track")
    assert len(got) == 0 and len(got.code) == 0 and len(got.kept_index) == 0 and got.kept_offsets.tolist() == [0] and set(got.stats.values()) == {0}
    assert got.frame_counts.shape == (3, 3) and not got.frame_counts.any() and got.timings["upload_us"] == 0 and got.timings["kernels_us"] == 0
    # and a call with something in it again
    assert run_points(vm, matcher, p_small, "points, small").kept.all()
    assert run_resect(vm, matcher, r_small, "resection, small").refined.all()
    V.assert_same(run_vet(vm, matcher, v_small, "vetting, small"), VC.reference("counts_5"), "vetting after the empty call")
