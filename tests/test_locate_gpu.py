"""GPU suite (run with -m gpu on an MI355X): Matcher.locate / Matcher.locate_points (vsm_locate_run, vsm_points_locate) - every
asked-for frame's pose from its observations of the points alone: a 16-lane group per (frame, hypothesis) for the linear fit,
tiles of 256 rows by runs of 16 hypotheses for the counts, a workgroup per frame for the winner, the resection's kernel for the
refinement.  Every result is compared with vsm_host_locate: every int equal, every double equal by its bytes.  The cases are those
of tests/locate_cases.py, proven on the CPU by test_locate_cpu.py; their sizes are the smallest at which the kernels can go
wrong: row counts on either side of a group, of a tile of 256 and of its second and third, hypothesis counts on either side of a
run of 16 and of a fit block (which two frames then share), frame counts of 1, 2, 9 and 257, every status in one grid.  A call
returns each frame's winner alone, and in the clean scenes that is hypothesis 0: what the other hypotheses hold and count is
checked in test_locate_kernels_gpu.py, kernel by kernel and on these calls' own tables."""
import numpy as np
import pytest

import ba_ref as B
import locate_cases as LC
import motions_cases as MO
import points_cases as PC
import points_ref as PR
import resect_ref as R
import tracks_ref as TR
import vet_ref as VR
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def vm():
    m = pkg("visomatch")
    L = m.lib()  # raises if the HIP library is missing: no silent fallback
    assert hasattr(L, "vsm_locate_run") and hasattr(L, "vsm_points_locate")
    return m


@pytest.fixture(scope="module")
def matcher(vm):
    m = vm.Matcher()
    yield m
    m.close()


def last_location(m):
    return m._locate_result(0, "the last result")


# ---- 1: every case against the host view ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(LC.cases()))
def test_cases(vm, matcher, name):
    a, kw = LC.cases()[name].args()
    want = LC.host(name)
    got = matcher.locate(*a, **kw)
    LC.assert_same(got, want, (name, "device against the host view"))
    assert [got.stats[k] for k in vm.LOCATE_STATUS] == np.bincount(want.status, minlength=7).tolist(), (name, got.stats)
    assert (got.located() == np.isin(want.status, (0, 6))).all()
    if len(want.status):
        assert got.timings["kernels_us"] > 0 and got.timings["group_sample_us"] > 0


def test_pool_chunks_against_one_chunk(vm, matcher):
    """the rows grouped in four chunks on the pool, the samples drawn a frame per pool task, against the host view's one thread"""
    c = LC.scene(4, 520, seed=60, locate=[1, 0, 1, 1], params=dict(ransac_iters=33))
    assert len(c.obs_frames) == 2080
    a, kw = c.args()
    got = matcher.locate(*a, **kw)
    assert got.rows.tolist() == [520] * 4 and got.status.tolist() == [0, 1, 0, 0]
    LC.assert_same(got, vm.host_locate(*a, **kw), "four chunks on the device path against the host view")
    LC.assert_same(matcher.locate(*a, **kw), got, "the same call again")


def test_errors_keep_the_last_result(vm):
    m = vm.Matcher()
    assert len(last_location(m)) == 0
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):  # neither a track nor a point result
        m.locate_points(PC.F, PC.CU, PC.CV)
    c = LC.cases()["frames_2"]
    (n, f, cu, cv, off, fr, uv, xyz), kw = c.args()
    good = m.locate(n, f, cu, cv, off, fr, uv, xyz, **kw)
    bad_fr = fr.copy()
    bad_fr[3] = n
    nan = float("nan")
    for args, over in (((n, f, cu, cv, off, bad_fr, uv, xyz), {}), ((n, f, cu, cv, off, fr, uv, None), {}), ((n, f, cu, cv, off, fr, uv, xyz), {"n_tracks": -2}),
                       ((-1, f, cu, cv, off, fr, uv, xyz), {"locate": None})) + tuple(
                           ((n, f, cu, cv, off, fr, uv, xyz), {"params": p}) for p in (dict(ransac_iters=0), dict(inlier_threshold=0.0), dict(inlier_threshold=nan),
                                                                                      dict(min_inliers=5), dict(max_updates=0), dict(eps=0.0), dict(eps=nan), vm._NO_PARAMS)):
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            m.locate(*args, **{**kw, **over})
        LC.assert_same(last_location(m), good, "the last good result")
    m.close()


# ---- 2: on the handle's own results, from images -------------------------------------------------------------------------------

WITHDRAWN = (2, 4)
LOCATE = dict(min_inliers=10)


@pytest.fixture(scope="module")
def clip(vm, synth):
    """match_pairs -> pair_tracks -> pair_motions -> chain_poses -> track_points on the small street clip of the motions tests,
    then a resection, a vetting and an adjustment so that the handle holds a result of every stage"""
    frames = MO.road_frames(synth)
    par = MO.road_params()
    m = vm.Matcher()
    lists = m.match_pairs(frames, None, MO.ROAD_PAIRS, 0)
    tr = m.pair_tracks()
    mot = m.pair_motions(par, bucket=True)
    poses, valid, _ = vm.chain_poses(MO.ROAD_N, MO.ROAD_PAIRS, mot.T, mot.rc)
    pts = m.track_points(poses, par.f, par.cu, par.cv, pose_valid=valid, params=MO.ROAD_POINT_PARAMS)
    res = m.resect_points(poses, par.f, par.cu, par.cv, pose_valid=valid, params=dict(min_observations=6))
    vet = m.vet_points(poses, par.f, par.cu, par.cv, pose_valid=valid)
    adj = m.adjust_points(poses, par.f, par.cu, par.cv, pose_valid=valid, params=dict(min_observations=6, max_rounds=2, cg_iters=10, max_residual=4.0))
    yield dict(m=m, par=par, lists=lists, tr=tr, mot=mot, poses=poses, valid=valid, pts=pts, res=res, vet=vet, adj=adj)
    m.close()


def test_handle_untouched(vm, clip):
    """locate_points = host_locate on track_pixels' arrays, and no other result of the handle moves"""
    m, par, tr, pts = clip["m"], clip["par"], clip["tr"], clip["pts"]
    assert clip["valid"][list(WITHDRAWN)].all()
    ask = np.zeros(MO.ROAD_N, np.uint8)
    ask[list(WITHDRAWN)] = 1
    got = m.locate_points(par.f, par.cu, par.cv, locate=ask, params=LOCATE)
    fr, uv = m.track_pixels()
    want = vm.host_locate(MO.ROAD_N, par.f, par.cu, par.cv, tr.offsets, fr, uv, pts.xyz, use=pts.kept, locate=ask, params=LOCATE)
    print("street clip: frames by status", got.stats, "rows", got.rows.tolist(), "eligible", got.eligible.tolist(), "inliers", got.inliers.tolist(), "best",
          got.best.tolist(), "used", got.used.tolist(), got.timings)
    LC.assert_same(got, want, "locate_points against host_locate on the same inputs")
    assert np.array_equal(fr, tr.obs[:, 0]) and uv.tobytes() == PC.gather(tr.obs, clip["lists"], 0).tobytes()
    LC.assert_same(m.locate_points(par.f, par.cu, par.cv, locate=ask, lists=clip["lists"], params=LOCATE), got, "the lists given explicitly")
    LC.assert_same(m.locate(MO.ROAD_N, par.f, par.cu, par.cv, tr.offsets, fr, uv, pts.xyz, use=pts.kept, locate=ask, params=LOCATE), got, "the general form")
    assert len(got) == MO.ROAD_N and sum(got.stats.values()) == MO.ROAD_N and (np.delete(got.status, list(WITHDRAWN)) == 1).all()
    TR.assert_same(m._tracks_result(0, "the last result", len(MO.ROAD_PAIRS)), tr, "the track result is untouched")
    PR.assert_same(m._points_result(0, "the last result"), pts, "the point result is untouched")
    MO.assert_same(m._motions_result(0, "the last result"), clip["mot"], "the motions result is untouched")
    R.assert_same(m._resect_result(0, "the last result"), clip["res"], "the resect result is untouched")
    VR.assert_same(m._vet_result(0, "the last result"), clip["vet"], "the vet result is untouched")
    B.assert_same(m._adjust_result(0, "the last result"), clip["adj"], "the adjust result is untouched")
    assert all(m.pair_matches(k).tobytes() == clip["lists"][k].tobytes() for k in range(len(MO.ROAD_PAIRS)))
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        m.locate_points(par.f, par.cu, par.cv, locate=ask, params=dict(min_inliers=5))
    LC.assert_same(last_location(m), got, "the last good result")


def test_images_to_poses(vm, clip):
    """the withdrawn frames come back located, and their located poses explain at least as many observations as the chained
    poses they had"""
    m, par, poses, valid = clip["m"], clip["par"], clip["poses"], clip["valid"]
    ask = np.zeros(MO.ROAD_N, np.uint8)
    ask[list(WITHDRAWN)] = 1
    got = m.locate_points(par.f, par.cu, par.cv, locate=ask, params=LOCATE)
    before = m.vet_points(poses, par.f, par.cu, par.cv, pose_valid=valid)
    moved = poses.copy()
    moved[list(WITHDRAWN)] = got.poses[list(WITHDRAWN)]
    after = m.vet_points(moved, par.f, par.cu, par.cv, pose_valid=valid)
    print("street clip: status", got.status.tolist(), "inliers at the chained poses", before.frame_counts[:, 0].tolist(), "at the located poses",
          after.frame_counts[:, 0].tolist(), "located - chained", np.abs(moved - poses).max(axis=1).tolist())
    assert got.status[list(WITHDRAWN)].tolist() == [0] * len(WITHDRAWN)
    assert (after.frame_counts[list(WITHDRAWN), 0] >= before.frame_counts[list(WITHDRAWN), 0]).all()
    m.vet_points(poses, par.f, par.cu, par.cv, pose_valid=valid)  # (the handle's vet result as the fixture left it)
