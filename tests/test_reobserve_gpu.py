"""GPU suite (run with -m gpu on an MI355X): Matcher.reobserve / Matcher.reobserve_points (vsm_reobserve_run,
vsm_points_reobserve) - the occupied features, the counting sort of the free ones by (frame, class, bin), a 16-lane group per
track for the projections, the tracks' scan over the counts, the list in (track, frame) order, a 16-lane group per candidate
for the search, the 64-bit claims and the verdicts.  Every result is compared with vsm_host_reobserve: every int equal, every
double equal by its bytes.  The cases are those of tests/reobserve_cases.py, proven against the plain-Python restatement by
test_reobserve_cpu.py; their sizes are the smallest at which the kernels can go wrong: track counts on either side of a
workgroup's sixteen groups and of the scan's 256 items, frame counts on either side of a group's sixteen lanes, windows of 0 to
33 features, a projection swept over every bin edge, contested features with equal and unequal costs."""
import numpy as np
import pytest

import ba_ref as B
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
    assert hasattr(L, "vsm_reobserve_run") and hasattr(L, "vsm_points_reobserve")
    return m


@pytest.fixture(scope="module")
def matcher(vm):
    m = vm.Matcher()
    yield m
    m.close()


def last_result(m):
    return m._reobserve_result(0, "the last result", lambda g: np.zeros((1 << 16, 12), np.int32))


def same(vm, got, want, what):
    RR.assert_same(got, want, what)
    assert [got.stats[k] for k in vm.REOBSERVE_STATS] == [want.stats[k] for k in vm.REOBSERVE_STATS], (what, got.stats, want.stats)


# ---- 1: every case against the host view ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(RC.cases()))
def test_cases(vm, matcher, name):
    c = RC.cases()[name]
    a, kw = c.args()
    want = RC.host(name)
    got = matcher.reobserve(*a, **kw)
    same(vm, got, want, (name, "device against the host view"))
    assert got.pixels.tobytes() == want.pixels.tobytes()
    same(vm, matcher.reobserve(*a, **{**kw, "ref_obs": c.middle_refs()}), want, (name, "ref_obs spelled out"))
    if len(want.cand):
        assert got.timings["kernels_us"] > 0 and got.timings["gather_us"] > 0


def test_another_reference_observation(vm, matcher):
    c = RC.cases()["frames_17"]
    a, kw = c.args()
    last = (np.diff(c.offsets) - 1).astype(np.int32)
    same(vm, matcher.reobserve(*a, **{**kw, "ref_obs": last}), vm.host_reobserve(*a, **{**kw, "ref_obs": last}), "the last observation as reference")


def test_scan_block_is_between_the_track_counts(vm, matcher):
    """the tracks' scan takes `scan_block` items per workgroup: the planted family has track counts on both sides of it"""
    lists = [np.zeros(1, vm.P_MATCH)]
    block = matcher.tracks(2, [(0, 1)], lists).stats["scan_block"]
    assert min(RC.TRACK_COUNTS) < block and block - 1 in RC.TRACK_COUNTS and block in RC.TRACK_COUNTS and block + 1 in RC.TRACK_COUNTS


def test_blocks_regrow_and_shrink(vm):
    """a small scene, a larger one, the small one again on one handle: the staging and the candidates' block grow and are reused"""
    m = vm.Matcher()
    for name in ("tracks_1", "tracks_257", "frames_33", "tracks_15", "no_frames", "sweep_4", "all_observed", "tracks_16"):
        a, kw = RC.cases()[name].args()
        same(vm, m.reobserve(*a, **kw), RC.host(name), (name, "on a handle that ran other sizes"))
    m.close()


def test_errors_keep_the_last_result(vm):
    import test_reobserve_cpu as cpu
    m = vm.Matcher()
    assert len(last_result(m)) == 0 and len(last_result(m).track_accepted) == 0
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):  # no pairs run, no track result, no point result
        m.reobserve_points(np.zeros((0, 12)), 1.0, 0.0, 0.0)
    c = RC.cases()["frames_9"]
    good_kw, bad = cpu._bad_calls(vm, c)
    good = cpu._call(m.reobserve, good_kw)
    same(vm, good, RC.host("frames_9"), "frames_9")
    for over in bad:
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            cpu._call(m.reobserve, {**good_kw, **over})
        same(vm, last_result(m), good, ("the last good result after", sorted(over)))
    m.close()


# ---- 2: on the handle's own results, from images -------------------------------------------------------------------------------

PAIRS = [(f - 1, f) for f in range(1, MO.ROAD_N)]  # consecutive pairs only: a point is not matched across a gap


@pytest.fixture(scope="module")
def clip(vm, synth):
    """match_pairs -> pair_tracks -> pair_motions -> chain_poses -> track_points on the small street clip of the motions tests,
    then a resection, a vetting, an adjustment and a location so that the handle holds a result of every stage"""
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
    feats = [m.pair_features(g) for g in range(MO.ROAD_N)]
    yield dict(m=m, frames=frames, par=par, lists=lists, tr=tr, mot=mot, poses=poses, valid=valid, pts=pts, res=res, vet=vet, adj=adj, feats=feats)
    m.close()


def host_on_the_clip(vm, clip, **kw):
    par, tr, pts, feats = clip["par"], clip["tr"], clip["pts"], clip["feats"]
    fo = np.cumsum([0] + [len(x) for x in feats]).astype(np.int32)
    return vm.host_reobserve(clip["poses"], par.f, par.cu, par.cv, MO.ROAD_W, MO.ROAD_H, tr.offsets, tr.obs[:, 0], tr.obs[:, 1], pts.xyz, fo, np.vstack(feats),
                             use=pts.kept, pose_valid=clip["valid"], **kw)


def test_pair_features_are_the_per_frame_features(vm, clip):
    """per frame: set 1 of the left image of a fresh matcher after push_back of that frame"""
    for g in range(MO.ROAD_N):
        fresh = vm.Matcher()
        fresh.push_back(clip["frames"][g])
        want = fresh.features(vm.FEATURE_SETS["1c2"])
        fresh.close()
        got = clip["feats"][g]
        assert len(got) > 100 and got.tobytes() == np.ascontiguousarray(want, dtype=np.int32).reshape(-1, 12).tobytes(), g
    m = clip["m"]
    assert len(m.pair_features(MO.ROAD_N)) == 0 and len(m.pair_features(-1)) == 0 and len(m.pair_features(0, side=1)) == 0 and len(m.pair_features(0, set=2)) == 0
    assert len(m.pair_features(0, set=0)) > 0


def test_match_lists_index_set_1(vm, synth):
    """refinement = 0: a match's pixels are its features' own, so the lists' i1p / i1c count in set 1 of their frames"""
    frames = MO.road_frames(synth)[:3]
    m = vm.Matcher(refinement=0)
    lists = m.match_pairs(frames, None, [(0, 1), (1, 2)], 0)
    feats = [m.pair_features(g) for g in range(3)]
    for (a, b), l in zip([(0, 1), (1, 2)], lists):
        assert len(l) > 50
        assert (np.abs(feats[b][l["i1c"], 0] - l["u1c"]) <= 1).all() and (np.abs(feats[b][l["i1c"], 1] - l["v1c"]) <= 1).all()
        assert (np.abs(feats[a][l["i1p"], 0] - l["u1p"]) <= 1).all() and (np.abs(feats[a][l["i1p"], 1] - l["v1p"]) <= 1).all()
    m.close()


def test_handle_form_against_the_host_view(vm, clip):
    """reobserve_points = host_reobserve on pair_features and the same tracks and points, and no other result of the handle moves"""
    m, par, tr, pts = clip["m"], clip["par"], clip["tr"], clip["pts"]
    assert (np.diff(tr.offsets) < MO.ROAD_N).any()  # tracks that end early: there is something to find
    got = m.reobserve_points(clip["poses"], par.f, par.cu, par.cv, pose_valid=clip["valid"])
    want = host_on_the_clip(vm, clip)
    print("street clip:", got.stats, "accepted per frame", got.frame_counts[:, 1].tolist(), got.timings)
    same(vm, got, want, "reobserve_points against host_reobserve on the same inputs")
    assert got.pixels.tobytes() == want.pixels.tobytes() and len(got.accepted()) > 0
    ask = np.zeros(MO.ROAD_N, np.uint8)
    ask[[1, 4]] = 1
    prm = dict(radius=2.5, max_cost=600, ratio_num=4, ratio_den=5)
    some = m.reobserve_points(clip["poses"], par.f, par.cu, par.cv, pose_valid=clip["valid"], search=ask, params=prm)
    same(vm, some, host_on_the_clip(vm, clip, search=ask, params=prm), "two frames searched, with a cap and a ratio")
    assert np.isin(some.cand[:, 1], (1, 4)).all()
    fo = np.cumsum([0] + [len(x) for x in clip["feats"]]).astype(np.int32)
    same(vm, m.reobserve(clip["poses"], par.f, par.cu, par.cv, MO.ROAD_W, MO.ROAD_H, tr.offsets, tr.obs[:, 0], tr.obs[:, 1], pts.xyz, fo, np.vstack(clip["feats"]),
                         use=pts.kept, pose_valid=clip["valid"]), want, "the general form")
    # the extended set feeds the next stages on the device
    fr, uv = m.track_pixels()
    off2, fr2, uv2, ft2 = got.extend(tr.offsets, fr, uv, tr.obs[:, 1])
    assert len(fr2) == len(fr) + len(got.accepted())
    vet2 = m.vet(clip["poses"], par.f, par.cu, par.cv, off2, fr2, uv2, pts.xyz, use=pts.kept, pose_valid=clip["valid"])
    assert len(vet2.code) == len(fr2)
    m.vet_points(clip["poses"], par.f, par.cu, par.cv, pose_valid=clip["valid"])  # (the handle's vet result as the fixture left it)
    TR.assert_same(m._tracks_result(0, "the last result", len(PAIRS)), tr, "the track result is untouched")
    PR.assert_same(m._points_result(0, "the last result"), pts, "the point result is untouched")
    MO.assert_same(m._motions_result(0, "the last result"), clip["mot"], "the motions result is untouched")
    R.assert_same(m._resect_result(0, "the last result"), clip["res"], "the resect result is untouched")
    VR.assert_same(m._vet_result(0, "the last result"), clip["vet"], "the vet result is untouched")
    B.assert_same(m._adjust_result(0, "the last result"), clip["adj"], "the adjust result is untouched")
    assert all(m.pair_matches(k).tobytes() == clip["lists"][k].tobytes() for k in range(len(PAIRS)))
    assert all(m.pair_features(g).tobytes() == clip["feats"][g].tobytes() for g in range(MO.ROAD_N))
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        m.reobserve_points(clip["poses"], par.f, par.cu, par.cv, params=dict(radius=-1.0))
    same(vm, last_result(m), want, "the last good result")


def test_not_ready_states(vm, synth):
    frames = MO.road_frames(synth)[:3]
    par = MO.road_params()
    pairs = [(0, 1), (1, 2)]
    poses = np.tile(np.array(RC.IDENTITY, np.float64), (3, 1))
    m = vm.Matcher()

    def not_ready():
        with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):
            m.reobserve_points(poses, par.f, par.cu, par.cv)

    not_ready()  # nothing at all
    lists = m.match_pairs(frames, None, pairs, 0)
    not_ready()  # no track result
    m.pair_tracks()
    not_ready()  # no point result
    m.track_points(poses, par.f, par.cu, par.cv, params=MO.ROAD_POINT_PARAMS)
    assert len(m.reobserve_points(poses, par.f, par.cu, par.cv).track_accepted) == len(m._tracks_result(0, "the last result", 2))
    m.tracks(3, pairs, lists)  # tracks that are not from the pairs run
    m.track_points(poses, par.f, par.cu, par.cv, lists=lists, params=MO.ROAD_POINT_PARAMS)
    not_ready()
    m.pair_tracks()
    m.track_points(poses, par.f, par.cu, par.cv, params=MO.ROAD_POINT_PARAMS)
    m.reobserve_points(poses, par.f, par.cu, par.cv)
    m.match_pairs(frames, None, [(0, 2), (0, 1)], 0)  # the lists have been replaced since
    not_ready()
    m.close()
    m = vm.Matcher(match_binsize=5)  # more than 1024 statistics bins: the whole call goes frame by frame, no features stay
    m.match_pairs(frames[:2], None, [(0, 1)], 0)
    m.pair_tracks()
    m.track_points(poses[:2], par.f, par.cu, par.cv, params=MO.ROAD_POINT_PARAMS)
    assert len(m.pair_features(0)) == 0
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):
        m.reobserve_points(poses[:2], par.f, par.cu, par.cv)
    m.close()
