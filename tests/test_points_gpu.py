"""GPU suite (run with -m gpu on an MI355X): Matcher.triangulate / Matcher.track_points (vsm_triangulate_run,
vsm_tracks_triangulate) - multi-view feature tracks into 3-D points on the device.  Every result is compared with
tests/points_ref.py (the definition restated in plain Python floats) and with vsm_host_triangulate: every int equal, every double
equal by its bytes.  The cases are those of tests/points_cases.py, proven on the CPU by test_points_cpu.py; their sizes are the
smallest at which the kernel can go wrong: track lengths on either side of a 16-lane group and of a wave, track counts on either
side of a wave and a workgroup, lengths and statuses mixed inside one wave."""
import numpy as np
import pytest

import content as CT
import points_cases as PC
import points_ref as R
import tracks_ref as TR
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def vm():
    m = pkg("visomatch")
    L = m.lib()  # raises if the HIP library is missing: no silent fallback
    assert hasattr(L, "vsm_triangulate_run") and hasattr(L, "vsm_tracks_triangulate")
    return m


@pytest.fixture(scope="module")
def matcher(vm):
    m = vm.Matcher()
    yield m
    m.close()


def last_points(vm, m):
    return m._points_result(0, "the last result")


# ---- 1: every case against the restatement and the host view ---------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(PC.cases()))
def test_cases(vm, matcher, name):
    a, kw = PC.cases()[name].args()
    want = PC.reference(name)
    got = matcher.triangulate(*a, **kw)
    R.assert_same(got, want, (name, "device against the restatement"))
    R.assert_same(vm.host_triangulate(*a, **kw), got, (name, "host view against the device"))
    assert [got.stats[k] for k in vm.POINT_STATUS] == np.bincount(want.status, minlength=10).tolist(), (name, got.stats)
    if len(want.status):
        assert got.timings["kernels_us"] > 0 and got.timings["gather_us"] > 0


# ---- 2: the tracks of the scenes on the device, their pixels gathered by the library --------------------------------------

@pytest.mark.parametrize("name", ["scene_type1", "noise_half_px", "world_frame", "merged_tracks", "min_length_4"])
def test_track_points_with_lists(vm, matcher, name):
    c = PC.cases()[name]
    tr = matcher.tracks(len(c.poses), c.pairs, c.lists, 0, 2)
    assert tr.offsets.tobytes() == c.offsets.tobytes() and tr.flags.tobytes() == c.flags.tobytes()
    got = matcher.track_points(c.poses, c.f, c.cu, c.cv, lists=c.lists, params=c.params)
    R.assert_same(got, PC.reference(name), (name, "track_points against the restatement"))
    a, kw = c.args()
    R.assert_same(matcher.triangulate(*a, **kw), got, (name, "triangulate on the same tracks"))
    TR.assert_same(matcher._tracks_result(0, "the last result", len(c.pairs)), tr, "the track result is untouched")
    # the lists of a pairs run are not these tracks' lists
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):
        matcher.track_points(c.poses, c.f, c.cu, c.cv, params=c.params)
    R.assert_same(last_points(vm, matcher), got, "the last good result")


# ---- 3: from images: match_pairs + pair_tracks + track_points ---------------------------------------------------------------

W, H, N = 417, 163, 7
IMAGE_PAIRS = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (0, 2), (6, 0), (2, 2)]


@pytest.fixture(scope="module")
def frames(synth):
    """test_tracks_gpu.py's image case: ([N,H,W] left, [N,H,W] right)"""
    return CT.stack(synth.stereo_sequence(31, W, H, N, disparity=10, ramp=(1, 12)))


def made_up_poses():
    """a sideways path with a little yaw; nothing about the images says so - equality is the subject here, not geometry"""
    return PC.camera_path(N, step=(0.3, 0.0, 0.02), yaw=0.004)


@pytest.mark.parametrize("method,side", [(0, 0), (2, 0), (2, 1)])
def test_from_images(vm, frames, method, side):
    left, right = frames
    m = vm.Matcher()
    assert m.push_back(left[1], right[1]) == 0 and m.push_back(left[4], right[4]) == 0 and m.match(method)
    ring = m.get_matches()
    assert m.match_pairs(left, right, IMAGE_PAIRS, method, fetch=False) is None
    tr = m.pair_tracks(side=side)
    lists = [m.pair_matches(k) for k in range(len(IMAGE_PAIRS))]
    poses, valid = made_up_poses(), [1, 1, 1, 0, 1, 1, 1]
    prm = dict(point_type=-1, max_dist=1e6, min_angle=0.01)
    got = m.track_points(poses, 400.0, W / 2, H / 2, pose_valid=valid, params=prm)
    assert len(got) == len(tr) >= 750
    print("points by status", got.stats, got.timings)
    uv = PC.gather(tr.obs, lists, side)  # the test's own gather from the fetched lists
    want = m.triangulate(poses, 400.0, W / 2, H / 2, tr.offsets, tr.obs[:, 0], uv, flags=tr.flags, pose_valid=valid, params=prm)
    R.assert_same(got, want, "track_points against triangulate on the gathered pixels")
    R.assert_same(m.track_points(poses, 400.0, W / 2, H / 2, lists=lists, pose_valid=valid, params=prm), got, "the lists given explicitly")
    assert got.stats["flagged"] == int(tr.flags.sum()) >= 1 and got.stats["no_pose"] >= 50 and sum(got.stats.values()) == len(tr)
    assert sum(1 for v in got.stats.values() if v) >= 3
    # the statuses are the definition's (ints: a NaN in a degenerate made-up point would not compare by bytes)
    host = vm.host_triangulate(poses, 400.0, W / 2, H / 2, tr.offsets, tr.obs[:, 0], uv, flags=tr.flags, pose_valid=valid, params=prm)
    assert (host.status == got.status).all() and (host.type == got.type).all() and (host.updates == got.updates).all()
    # nothing else of the handle has moved
    assert all(a.tobytes() == b.tobytes() for a, b in zip([m.pair_matches(k) for k in range(len(IMAGE_PAIRS))], lists))
    assert m.get_matches().tobytes() == ring.tobytes()
    TR.assert_same(m._tracks_result(0, "the last result", len(IMAGE_PAIRS)), tr, "the track result is untouched")
    m.close()


# ---- 4: determinism -----------------------------------------------------------------------------------------------------------------

def test_determinism(vm, matcher):
    a, kw = PC.cases()["lengths"].args()
    first = matcher.triangulate(*a, **kw)
    b, kwb = PC.cases()["scene_type-1"].args()
    matcher.triangulate(*b, **kwb)
    R.assert_same(matcher.triangulate(*a, **kw), first, "the same call again, after another")
    other = vm.Matcher()
    R.assert_same(other.triangulate(*a, **kw), first, "a second handle")
    other.close()


# ---- 5: error codes, the previous result intact ----------------------------------------------------------------------------------

def test_errors_keep_the_last_result(vm, frames):
    left, right = frames
    m = vm.Matcher()
    c = PC.cases()["special"]
    (poses, f, cu, cv, off, fr, uv), kw = c.args()
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):  # no track result at all
        m.track_points(poses, f, cu, cv)
    assert len(last_points(vm, m)) == 0
    good = m.triangulate(poses, f, cu, cv, off, fr, uv, **kw)
    R.assert_same(good, PC.reference("special"), "special")
    bad_fr = fr.copy()
    bad_fr[2] = len(poses)
    dec = off.copy()
    dec[3] = dec[2] - 1
    for args, over in (((poses, f, cu, cv, off, bad_fr, uv), {}), ((poses, f, cu, cv, dec, fr, uv), {}), ((poses, f, cu, cv, off, fr, uv), {"n_tracks": -2}),
                       ((poses, f, cu, cv, off, fr, uv), {"params": dict(min_track_length=0)})):
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            m.triangulate(*args, **{**kw, **over})
        R.assert_same(last_points(vm, m), good, "the last good result")
    # tracks from lists of the caller's: lists == NULL is not ready, wrong counts are an argument error
    s = PC.cases()["merged_tracks"]
    tr = m.tracks(len(s.poses), s.pairs, s.lists, 0, 2)
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):
        m.track_points(s.poses, s.f, s.cu, s.cv)
    counts = np.array([len(x) for x in s.lists], np.int32)
    counts[1] += 1
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        m.track_points(s.poses, s.f, s.cu, s.cv, lists=s.lists, counts=counts)
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        m.track_points(s.poses, s.f, s.cu, s.cv, lists=s.lists, params=dict(min_track_length=0))
    R.assert_same(last_points(vm, m), good, "the last good result")
    TR.assert_same(m._tracks_result(0, "the last result", len(s.pairs)), tr, "the track result is untouched")
    # a pairs run alone does not make lists == NULL ready: the tracks did not come from it
    m.match_pairs(left[:3], right[:3], [(0, 1), (1, 2)], 0, fetch=False)
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):
        m.track_points(s.poses, s.f, s.cu, s.cv)
    R.assert_same(last_points(vm, m), good, "the last good result")
    m.close()
