"""GPU suite (run with -m gpu on an MI355X): Matcher.fuse / Matcher.fuse_points (vsm_fuse_run, vsm_points_fuse) - the owners by
atomic minimum, the counting sort of the owned features by (frame, class, bin), a 16-lane group per track that projects and
searches and counts, the list by compaction of the counting pass's proposals or by a second pass, the conflict test, the 64-bit bids, the verdicts, the scan over the new lengths and
the merge per survivor.  Every result is compared with vsm_host_fuse: every int equal, every double equal by its bytes.  The
cases are those of tests/fuse_cases.py, proven against the plain-Python restatement by test_fuse_cpu.py; their sizes are the
smallest at which the kernels can go wrong: track counts on either side of a workgroup's sixteen groups and of the scan's 256
items, frame counts on either side of a group's sixteen lanes, windows of 0 to 33 features, proposal counts around 256,
fragments of 1 to 257 observations."""
import numpy as np
import pytest

import ba_ref as B
import fuse_cases as FC
import fuse_ref as FR
import motions_cases as MO
import points_ref as PR
import reobserve_cases as RC
import reobserve_ref as RR
import resect_ref as R
import tracks_ref as TR
import vet_ref as VR
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def vm():
    m = pkg("visomatch")
    L = m.lib()  # raises if the HIP library is missing: no silent fallback
    assert hasattr(L, "vsm_fuse_run") and hasattr(L, "vsm_points_fuse")
    return m


@pytest.fixture(scope="module")
def matcher(vm):
    m = vm.Matcher()
    yield m
    m.close()


def last_result(m):
    return m._fuse_result(0, "the last result")


def same(vm, got, want, what):
    FR.assert_same(got, want, what)
    assert [got.stats[k] for k in vm.FUSE_STATS] == [want.stats[k] for k in vm.FUSE_STATS], (what, got.stats, want.stats)


# ---- 1: every case against the host view, on one handle that runs all the sizes --------------------------------------------------

@pytest.mark.parametrize("name", sorted(FC.cases()))
def test_cases(vm, matcher, name):
    c = FC.cases()[name]
    a, kw = c.args()
    want = FC.host(name)
    got = matcher.fuse(*a, **kw)
    same(vm, got, want, (name, "device against the host view"))
    if kw["ref_obs"] is None:
        same(vm, matcher.fuse(*a, **{**kw, "ref_obs": c.middle_refs()}), want, (name, "ref_obs spelled out"))
    if len(want.prop):
        assert got.timings["kernels_us"] > 0 and got.timings["gather_us"] > 0


def test_another_reference_observation(vm, matcher):
    c = FC.cases()["frames_17"]
    a, kw = c.args()
    last = np.maximum(np.diff(c.offsets) - 1, 0).astype(np.int32)
    same(vm, matcher.fuse(*a, **{**kw, "ref_obs": last}), vm.host_fuse(*a, **{**kw, "ref_obs": last}), "the last observation as reference")


def test_blocks_regrow_and_shrink(vm):
    """a small scene, a larger one, the small one again on one handle: the staging and the proposals' block grow and are reused"""
    m = vm.Matcher()
    for name in ("tracks_1", "tracks_257", "fragments", "tracks_15", "no_frames", "carpet_sweep_4", "frames_1", "proposals_257", "tracks_16"):
        a, kw = FC.cases()[name].args()
        same(vm, m.fuse(*a, **kw), FC.host(name), (name, "on a handle that ran other sizes"))
    m.close()


def test_the_compacting_form_gives_the_same_bytes(vm):
    """option fuse_compact: 1, the search once, the proposals kept in places per track and moved behind the scan, and 0, the
    search twice - the same result either way, on sizes on either side of a workgroup and of the scan's block, each form
    before and after the other (the default takes the first where the places fit)"""
    m = vm.Matcher()
    for form, names in ((1, ("tracks_257", "tracks_1", "proposals_257", "everything", "no_frames", "fragments", "masks", "tracks_16")),
                        (0, ("frames_33", "tracks_17", "tracks_257", "proposals_256", "everything", "fragments", "no_frames", "tracks_1")), (1, ("frames_33", "three_ways", "carpet_sweep_4", "windows"))):
        m.set_option("fuse_compact", form)
        for name in names:
            a, kw = FC.cases()[name].args()
            same(vm, m.fuse(*a, **kw), FC.host(name), (name, "fuse_compact", form))
    m.close()


def test_a_second_call_on_the_merged_set(vm, matcher):
    """three fragments: the first call joins two, the second - on the merged set of the first - the third"""
    for name in ("three_ways", "three_ways_interleaved", "split_8"):
        c = FC.cases()[name]
        a, kw = c.args()
        first = matcher.fuse(*a, **kw)
        off, fr, uv, ft = first.merge(c.obs_frames, FC.pixels(c), c.obs_feat)
        second = matcher.fuse(*a[:6], off, fr, ft, *a[9:], **kw)
        same(vm, second, vm.host_fuse(*a[:6], off, fr, ft, *a[9:], **kw), (name, "the second call"))
        assert len(first.fused()) > 8 and (len(second.fused()) > 8) == (c.ways == 3)
        off2, fr2, uv2, ft2 = second.merge(fr, uv, ft)
        u, T = c.unsplit, c.n_points
        assert off2[:T + 1].tobytes() == u.offsets.tobytes() and fr2.tobytes() == u.obs_frames.tobytes() and ft2.tobytes() == u.obs_feat.tobytes()


def test_errors_keep_the_last_result(vm):
    import test_fuse_cpu as cpu
    m = vm.Matcher()
    assert len(last_result(m)) == 0 and len(last_result(m).partner) == 0 and len(last_result(m).obs_src) == 0
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):  # no pairs run, no track result, no point result
        m.fuse_points(np.zeros((0, 12)), 1.0, 0.0, 0.0)
    c = FC.cases()["frames_9"]
    good_kw, bad = cpu._bad_calls(vm, c)
    good = cpu._call(m.fuse, good_kw)
    same(vm, good, FC.host("frames_9"), "frames_9")
    for over in bad:
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            cpu._call(m.fuse, {**good_kw, **over})
        same(vm, last_result(m), good, ("the last good result after", sorted(over)))
    m.close()


# ---- 2: on the handle's own results, from images -------------------------------------------------------------------------------

PAIRS = [(f - 1, f) for f in range(1, MO.ROAD_N)]  # consecutive pairs only: a point's track ends where one match is missed


@pytest.fixture(scope="module")
def clip(vm, synth):
    """the synthetic street clip of the re-observation's tests with a result of every stage on the handle"""
    frames = MO.road_frames(synth)
    par = MO.road_params()
    m = vm.Matcher()
    lists = m.match_pairs(frames, None, PAIRS, 0)
    tr = m.pair_tracks()
    mot = m.pair_motions(par, bucket=True)
    poses, valid, _ = vm.chain_poses(MO.ROAD_N, PAIRS, mot.T, mot.rc)
    pts = m.track_points(poses, par.f, par.cu, par.cv, pose_valid=valid, params=MO.ROAD_POINT_PARAMS)
    res = m.resect_points(poses, par.f, par.cu, par.cv, pose_valid=valid, params=dict(min_observations=6))
    vet = m.vet_points(poses, par.f, par.cu, par.cv, pose_valid=valid)
    adj = m.adjust_points(poses, par.f, par.cu, par.cv, pose_valid=valid, params=dict(min_observations=6, max_rounds=2, cg_iters=10, max_residual=4.0))
    ro = m.reobserve_points(poses, par.f, par.cu, par.cv, pose_valid=valid)
    feats = [m.pair_features(g) for g in range(MO.ROAD_N)]
    yield dict(m=m, par=par, lists=lists, tr=tr, mot=mot, poses=poses, valid=valid, pts=pts, res=res, vet=vet, adj=adj, ro=ro, feats=feats)
    m.close()


def host_on_the_clip(vm, clip, **kw):
    par, tr, pts, feats = clip["par"], clip["tr"], clip["pts"], clip["feats"]
    fo = np.cumsum([0] + [len(x) for x in feats]).astype(np.int32)
    return vm.host_fuse(clip["poses"], par.f, par.cu, par.cv, MO.ROAD_W, MO.ROAD_H, tr.offsets, tr.obs[:, 0], tr.obs[:, 1], pts.xyz, fo, np.vstack(feats),
                        use=pts.kept, pose_valid=clip["valid"], **kw)


def test_handle_form_against_the_host_view(vm, clip):
    """fuse_points = host_fuse on pair_features and the same tracks and points, and no other result of the handle moves"""
    m, par, tr, pts = clip["m"], clip["par"], clip["tr"], clip["pts"]
    got = m.fuse_points(clip["poses"], par.f, par.cu, par.cv, pose_valid=clip["valid"])
    want = host_on_the_clip(vm, clip)
    print("street clip:", got.stats, "proposals per frame", got.frame_counts[:, 1].tolist(), got.timings)
    same(vm, got, want, "fuse_points against host_fuse on the same inputs")
    assert len(got.prop) > 0 and sorted(got.obs_src.tolist()) == list(range(len(tr.obs)))
    ask = np.zeros(MO.ROAD_N, np.uint8)
    ask[[1, 4]] = 1
    prm = dict(radius=2.5, max_cost=600, ratio_num=4, ratio_den=5)
    some = m.fuse_points(clip["poses"], par.f, par.cu, par.cv, pose_valid=clip["valid"], search=ask, params=prm)
    same(vm, some, host_on_the_clip(vm, clip, search=ask, params=prm), "two frames searched, with a cap and a ratio")
    assert np.isin(some.prop[:, 1], (1, 4)).all()
    fo = np.cumsum([0] + [len(x) for x in clip["feats"]]).astype(np.int32)
    general = (clip["poses"], par.f, par.cu, par.cv, MO.ROAD_W, MO.ROAD_H)
    same(vm, m.fuse(*general, tr.offsets, tr.obs[:, 0], tr.obs[:, 1], pts.xyz, fo, np.vstack(clip["feats"]), use=pts.kept, pose_valid=clip["valid"]), want,
         "the general form")
    # the merged set feeds the next stages on the device, and a second call
    fr, uv = m.track_pixels()
    off2, fr2, uv2, ft2 = got.merge(fr, uv, tr.obs[:, 1])
    assert len(fr2) == len(fr) and off2[-1] == len(fr)
    pts2 = m.triangulate(clip["poses"], par.f, par.cu, par.cv, off2, fr2, uv2, pose_valid=clip["valid"], params=MO.ROAD_POINT_PARAMS)
    again = m.fuse(*general, off2, fr2, ft2, pts2.xyz, fo, np.vstack(clip["feats"]), use=pts2.kept, pose_valid=clip["valid"])
    same(vm, again, vm.host_fuse(*general, off2, fr2, ft2, pts2.xyz, fo, np.vstack(clip["feats"]), use=pts2.kept, pose_valid=clip["valid"]), "the second call")
    m.track_points(clip["poses"], par.f, par.cu, par.cv, pose_valid=clip["valid"], params=MO.ROAD_POINT_PARAMS)  # (the point result as the fixture left it)
    TR.assert_same(m._tracks_result(0, "the last result", len(PAIRS)), tr, "the track result is untouched")
    PR.assert_same(m._points_result(0, "the last result"), pts, "the point result is untouched")
    MO.assert_same(m._motions_result(0, "the last result"), clip["mot"], "the motions result is untouched")
    R.assert_same(m._resect_result(0, "the last result"), clip["res"], "the resect result is untouched")
    VR.assert_same(m._vet_result(0, "the last result"), clip["vet"], "the vet result is untouched")
    B.assert_same(m._adjust_result(0, "the last result"), clip["adj"], "the adjust result is untouched")
    RR.assert_same(m._reobserve_result(0, "the last result"), clip["ro"], "the re-observation result is untouched")
    assert all(m.pair_matches(k).tobytes() == clip["lists"][k].tobytes() for k in range(len(PAIRS)))
    assert all(m.pair_features(g).tobytes() == clip["feats"][g].tobytes() for g in range(MO.ROAD_N))
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        m.fuse_points(clip["poses"], par.f, par.cu, par.cv, params=dict(radius=-1.0))
    same(vm, last_result(m), again, "the last good result")


def test_not_ready_states(vm, synth):
    frames = MO.road_frames(synth)[:3]
    par = MO.road_params()
    pairs = [(0, 1), (1, 2)]
    poses = np.tile(np.array(RC.IDENTITY, np.float64), (3, 1))
    m = vm.Matcher()

    def not_ready():
        with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):
            m.fuse_points(poses, par.f, par.cu, par.cv)

    not_ready()  # nothing at all
    lists = m.match_pairs(frames, None, pairs, 0)
    not_ready()  # no track result
    m.pair_tracks()
    not_ready()  # no point result
    m.track_points(poses, par.f, par.cu, par.cv, params=MO.ROAD_POINT_PARAMS)
    assert len(m.fuse_points(poses, par.f, par.cu, par.cv).partner) == len(m._tracks_result(0, "the last result", 2))
    m.tracks(3, pairs, lists)  # tracks that are not from the pairs run
    m.track_points(poses, par.f, par.cu, par.cv, lists=lists, params=MO.ROAD_POINT_PARAMS)
    not_ready()
    m.pair_tracks()
    m.track_points(poses, par.f, par.cu, par.cv, params=MO.ROAD_POINT_PARAMS)
    m.fuse_points(poses, par.f, par.cu, par.cv)
    m.match_pairs(frames, None, [(0, 2), (0, 1)], 0)  # the lists have been replaced since
    not_ready()
    m.close()
    m = vm.Matcher(match_binsize=5)  # more than 1024 statistics bins: the whole call goes frame by frame, no features stay
    m.match_pairs(frames[:2], None, [(0, 1)], 0)
    m.pair_tracks()
    m.track_points(poses[:2], par.f, par.cu, par.cv, params=MO.ROAD_POINT_PARAMS)
    assert len(m.pair_features(0)) == 0
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):
        m.fuse_points(poses[:2], par.f, par.cu, par.cv)
    m.close()
