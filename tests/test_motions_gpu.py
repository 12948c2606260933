"""GPU suite (run with -m gpu on an MI355X): Matcher.motions / Matcher.pair_motions (vsm_motions_run, vsm_pairs_motions) - the
monocular motion of every pair of a pair set in one batched call.  Every result is compared with host_pairs_motions, which
tests/test_motions_cpu.py pins to the per-pair estimate: every int equal, every double equal by its bytes.  The batches are
those of tests/motions_cases.py; their sizes sit on either side of a wave, of a 256-thread block of the count, winner and vote
kernels and of the fit kernel's 16 hypotheses per block, and K = 17 puts a pair boundary inside a fit block."""
import numpy as np
import pytest

import motions_cases as MO
import points_cases as PC
import points_ref as R
import tracks_ref as TR
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def vm():
    m = pkg("visomatch")
    L = m.lib()  # raises if the HIP library is missing: no silent fallback
    assert hasattr(L, "vsm_motions_run") and hasattr(L, "vsm_pairs_motions")
    return m


@pytest.fixture(scope="module")
def matcher(vm):
    m = vm.Matcher()
    yield m
    m.close()


_host = {}


def host(vm, name):
    if name not in _host:
        lists, par, bucket = MO.batch(name)
        _host[name] = vm.host_pairs_motions(lists, par, bucket=bucket, threads=8)
    return _host[name]


def assert_from_device(got, K):
    """no silent fallback: the self-test passed, and every pair that reached a stage took it from the device"""
    st = got.stats
    assert st["device_svd"] == 1, st
    reached = lambda s: int((got.stage >= s).sum())   # noqa: E731
    assert [st[n] for n in MO.pkg("visomatch").MOTION_STAGES] == np.bincount(got.stage, minlength=7).tolist(), st
    assert st["device_fit"] == st["device_count"] == (reached(2) if K > 0 else 0), st
    assert st["device_triangulate"] == reached(3), st
    assert st["device_vote"] == reached(6), st
    assert st["waits"] <= 3 * st["chunks"], st


# ---- 1: every batch against the host view ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(MO.BATCHES))
def test_batches(vm, matcher, name):
    lists, par, bucket = MO.batch(name)
    got = matcher.motions(lists, par, bucket=bucket)
    MO.assert_same(got, host(vm, name), name)
    assert_from_device(got, par.ransac_iters)
    if name == "stages":
        assert sorted(set(got.stage.tolist())) == [0, 1, 2, 4, 5, 6] and got.stats["chunks"] == 1
    if name == "twice":
        assert got.T[0].tobytes() == got.T[2].tobytes() and np.array_equal(got.inliers(0), got.inliers(2))
    if name == "bucket":
        assert sum(len(m) for m in lists) - sum(len(got.matches(k)) for k in range(len(lists))) > 500
    if (got.rc == 1).any():
        assert got.timings["fit_count_winner_us"] > 0 and got.timings["total_us"] > 0


# ---- 2: chunking and repetition do not change a result ------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 2, 7])
def test_chunks(vm, P):
    lists, par, _ = MO.batch("seven")
    want = vm.host_pairs_motions(lists[:P], par, threads=8)
    for chunk in (0, 1, 3):
        m = vm.Matcher(options={"motions_chunk": chunk})
        got = m.motions(lists[:P], par)
        MO.assert_same(got, want, (P, chunk))
        assert got.stats["chunks"] == (1 if chunk == 0 else -(-P // chunk)), got.stats
        assert_from_device(got, 200)
        MO.assert_same(m.motions(lists[:P], par), got, (P, chunk, "called twice"))
        m.close()


# ---- 3: nothing else of the handle moves; error codes keep the last result ------------------------------------------------------

def test_handle_untouched_and_errors(vm, synth):
    frames = MO.road_frames(synth)
    m = vm.Matcher()
    par = MO.road_params()
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):
        m.pair_motions(par)
    assert m.push_back(frames[1]) == 0 and m.push_back(frames[2]) == 0 and m.match(0)
    ring = m.get_matches()
    pairs = MO.ROAD_PAIRS[:3]
    lists = m.match_pairs(frames, None, pairs, 0)
    tr = m.pair_tracks()
    poses = PC.camera_path(MO.ROAD_N, step=(0.0, 0.0, 0.6), yaw=0.0)
    pts = m.track_points(poses, par.f, par.cu, par.cv, params=MO.ROAD_POINT_PARAMS)
    good = m.pair_motions(par, bucket=True)
    MO.assert_same(good, vm.host_pairs_motions(lists, par, bucket=True, threads=4), "pair_motions")
    assert m.get_matches().tobytes() == ring.tobytes()
    assert all(m.pair_matches(k).tobytes() == lists[k].tobytes() for k in range(len(pairs)))
    TR.assert_same(m._tracks_result(0, "the last result", len(pairs)), tr, "the track result is untouched")
    R.assert_same(m._points_result(0, "the last result"), pts, "the point result is untouched")
    # argument errors: nothing enqueued, the last result kept
    bad = lists[1].copy()
    bad["u1p"][0] = np.inf
    for args, kw in (((lists, None), {}), (([], par), {}), (([lists[0], None], par), {"counts": [len(lists[0]), 4]}),
                     ((lists, par), {"counts": [len(lists[0]), -1, len(lists[2])]}), ((lists, MO.road_params(-1)), {}), (([lists[0], bad], par), {})):
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            m.motions(*args, **kw)
        MO.assert_same(m.last_motions(), good, "the last good result")
    # a stereo pairs run has no flow lists
    both = np.stack([frames, frames])
    m.match_pairs(both[0], both[1], pairs, 1, fetch=False)
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        m.pair_motions(par)
    MO.assert_same(m.last_motions(), good, "the last good result")
    m.close()


# ---- 4: from images ----------------------------------------------------------------------------------------------------------------

def test_from_images(vm, synth):
    """match_pairs -> pair_motions(bucket=True) against a fresh VisualOdometryMono per pair; then chain_poses -> pair_tracks ->
    track_points against the same chain assembled from the host views.  Equality, not accuracy, is the subject."""
    frames = MO.road_frames(synth)
    par = MO.road_params()
    m = vm.Matcher()
    lists = m.match_pairs(frames, None, MO.ROAD_PAIRS, 0)
    assert all(len(l) > 10 for l in lists)
    got = m.pair_motions(par, bucket=True)
    assert_from_device(got, 200)
    print("road clip:", got.rc.tolist(), got.stats, got.timings)
    for k, (a, b) in enumerate(MO.ROAD_PAIRS):
        vm.vo_sampler_seed(71)
        vo = vm.VisualOdometryMono(par.f, par.cu, par.cv, bucket=MO.BUCKET, height=1.65, pitch=0.0, ransac_iters=200)
        assert vo.process(frames[a])[0] is False
        ok, T = vo.process(frames[b])
        assert vo.device_svd()
        assert vo.bucketed().tobytes() == got.matches(k).tobytes(), k
        assert ok == bool(got.rc[k] == 1), k
        assert np.array_equal(vo.inliers(), got.inliers(k)), k
        assert T.tobytes() == got.T[k].tobytes(), k   # (a failed estimate leaves the identity in both)
        vo.close()
    assert int((got.rc == 1).sum()) >= 1
    MO.assert_same(got, vm.host_pairs_motions(lists, par, bucket=True, threads=8), "host view")
    # the chain: device results against the host views' on the same lists
    poses, valid, posed = vm.chain_poses(MO.ROAD_N, MO.ROAD_PAIRS, got.T, got.rc)
    assert posed >= 2
    tr = m.pair_tracks()
    pts = m.track_points(poses, par.f, par.cu, par.cv, pose_valid=valid, params=MO.ROAD_POINT_PARAMS)
    h_mot = vm.host_pairs_motions(lists, par, bucket=True, threads=8)
    h_poses, h_valid, _ = vm.chain_poses(MO.ROAD_N, MO.ROAD_PAIRS, h_mot.T, h_mot.rc)
    assert h_poses.tobytes() == poses.tobytes() and h_valid.tobytes() == valid.tobytes()
    h_tr = vm.host_tracks(MO.ROAD_N, MO.ROAD_PAIRS, lists)
    TR.assert_same(tr, h_tr, "tracks")
    uv = PC.gather(h_tr.obs, lists, 0)
    h_pts = vm.host_triangulate(h_poses, par.f, par.cu, par.cv, h_tr.offsets, h_tr.obs[:, 0], uv, flags=h_tr.flags, pose_valid=h_valid, params=MO.ROAD_POINT_PARAMS)
    R.assert_same(pts, h_pts, "points of the chain")
    assert int(pts.kept.sum()) >= 1
    m.close()
