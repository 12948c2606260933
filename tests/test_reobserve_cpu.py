"""CPU suite: vsm_host_reobserve - the re-observation's host view, one thread walking csrc/vsm_reobserve.h - against
tests/reobserve_ref.py, the definition restated in plain Python ints and floats without any index: every array equal by its
bytes, on all cases of tests/reobserve_cases.py.  Then what the cases are for is checked on the restatement's own result, so that
a case that no longer reaches its window size, its edge, its tie or its code fails here and not silently; the planted scenes are
recovered exactly; a frame's feature order and the other frames of a call do not matter; every argument error is returned with
the outputs untouched; and the extended track set feeds the vetting, the resection and the adjustment."""
import ctypes as C
import math

import numpy as np
import pytest

import reobserve_cases as RC
import reobserve_ref as RR
from conftest import pkg


@pytest.fixture(scope="module")
def vm():
    m = pkg("visomatch")
    m.lib()
    return m


@pytest.mark.parametrize("name", sorted(RC.cases()))
def test_host_view_equals_the_restatement(vm, name):
    got, want = RC.host(name), RC.reference(name)
    RR.assert_same(got, want, name)
    assert [got.stats[k] for k in vm.REOBSERVE_STATS] == want.stats
    c = RC.cases()[name]
    assert sum(want.stats[5:]) == len(want.cand) and want.frame_counts[:, 0].sum() == len(want.cand)
    in_use = int(((np.ones(len(c.offsets) - 1) if c.use is None else c.use[:len(c.offsets) - 1]) * (np.diff(c.offsets) > 0)).sum()) if len(c.offsets) else 0
    assert sum(want.stats) == in_use * len(c.poses)
    assert want.track_accepted.sum() == want.frame_counts[:, 1].sum() == want.stats[5] == len(got.accepted())
    order = want.cand[:, 0].astype(np.int64) * (len(c.poses) + 1) + want.cand[:, 1]
    assert (np.diff(order) > 0).all()  # ascending (track, frame)


@pytest.mark.parametrize("name", sorted(n for n, c in RC.cases().items() if c.expected is not None))
def test_the_planted_scene_is_recovered_exactly(vm, name):
    c, got = RC.cases()[name], RC.host(name)
    found = {(int(r[0]), int(r[1])): int(r[2]) for r in got.cand[got.accepted()]}
    assert found == c.expected, (name, sorted(set(found.items()) ^ set(c.expected.items()))[:10])
    # the margins: a planted feature costs at most 64, the best of the rest is far off
    acc = got.cand[got.accepted()]
    assert (acc[:, 3] <= 64).all() and (acc[:, 4][acc[:, 4] >= 0] > 1000).all()
    if name != "empty_frame":
        assert (got.code == 0).all()  # every candidate has its planted feature
    else:
        assert ((got.code == 1) == (got.cand[:, 1] == 2)).all() and (got.code == 1).sum() > 5


def test_families():
    for n in RC.TRACK_COUNTS:
        assert len(RC.cases()["tracks_%d" % n].offsets) - 1 == n or n == 0
    for n in RC.FRAME_COUNTS:
        assert len(RC.cases()["frames_%d" % n].poses) == n
    assert len(RC.reference("tracks_257").cand) > 200 and len(RC.reference("frames_33").cand) > 100
    assert len(RC.reference("all_observed").cand) == 0 and RC.reference("all_observed").stats[RR.OBSERVED] > 0
    one = RC.reference("one_all_observed")
    assert not (one.cand[:, 0] == 3).any() and len(set(one.cand[:, 0].tolist())) > 5
    assert RC.cases()["empty_frame"].feat_offsets[2] == RC.cases()["empty_frame"].feat_offsets[3]


def test_window_sizes_and_classes():
    want = RC.reference("windows")
    assert want.cand[:, 5].tolist() == list(RC.WINDOW_SIZES)  # the features of the other classes, cost 0, are not counted
    assert want.cand[:, 6].tolist() == [1] + [0] * 6 and (want.cand[1:, 3] > 0).all()
    assert want.cand[1, 4] == -1 and (want.cand[2:, 4] >= want.cand[2:, 3]).all()


@pytest.mark.parametrize("name,radius,shift", [("sweep_4", 4.0, 0.0), ("sweep_2_5", 2.5, 0.0), ("sweep_2_5_half", 2.5, 0.5), ("sweep_0", 0.0, 0.0)])
def test_sweep_window_edges(name, radius, shift):
    """the window's size in closed form: columns u with |u - pu| <= radius inside the frame, times the rows within radius"""
    want, r = RC.reference(name), int(math.floor(radius))
    rows = sum(1 for dv in (-(r + 1), -r, 0, r, r + 1) if abs(dv) <= radius)
    width = RC.cases()[name].width
    for row, (pu, pv) in zip(want.cand, want.uv):
        cols = sum(1 for u in range(width) if abs(u - pu) <= radius)
        assert row[5] == cols * rows, (name, row.tolist(), pu)
    assert len(want.cand) == (width if shift == 0 else width - 1) and want.uv[0][0] == shift


def test_edges_depth_and_non_finite_inputs():
    c, want = RC.cases()["edges"], RC.reference("edges")
    tracks = want.cand[:, 0].tolist()
    depth0 = c.n_inside + c.n_outside
    assert tracks == [0, 1, 2, 3, depth0 + 3, depth0 + 4 + 6, depth0 + 4 + 8] and (want.cand[:, 1] == 1).all()
    assert want.uv[:4].tolist() == [[0.0, 0.0], [c.width - 1.0, c.height - 1.0], [0.0, c.height - 1.0], [c.width - 1.0, 0.0]] and (want.cand[:4, 6] == 0).all()
    assert want.uv[4].tolist() == [30.0, 20.0] and want.uv[5].tolist() == [30.0, 20.0]
    # the next doubles outside, the depths up to min_depth itself, the NaN and infinite points and the frames with a NaN or an
    # infinity in their pose: each fails one comparison or the other, none is a candidate
    assert want.stats[RR.OUTSIDE] >= c.n_outside + 2 and want.stats[RR.BEHIND] >= 3 + len(c.xyz)
    assert want.stats[RR.OUTSIDE] + want.stats[RR.BEHIND] + len(want.cand) == 3 * len(c.xyz)
    assert sorted(want.cand[4:, 6].tolist()) == [0, 4, 4] and (want.cand[4:, 2] == 4).all()


def test_ties_and_the_occupied_feature():
    c, want = RC.cases()["ties"], RC.reference("ties")
    assert want.cand[0].tolist() == [0, 1, 1, 7, 7, 4, 0]  # three features at cost 7: the lowest index; second = best
    assert want.cand[1].tolist() == [1, 1, c.taken + 1, 5, 5, 2, 0]  # the occupied feature (cost 0) is not in the window
    assert want.stats[RR.OBSERVED] == 2 and len(want.cand) == 2  # the unused track's observations occupy, its pairs do not count


def test_contested_features():
    c, want = RC.cases()["claims"], RC.reference("claims")
    code = {int(r[0]): int(r[6]) for r in want.cand}
    cost = {int(r[0]): int(r[3]) for r in want.cand}
    for n, un, eq in zip(RC.CLAIMANTS, c.unequal, c.equal):
        assert [cost[t] for t in un] == list(range(n, 0, -1)) and [code[t] for t in un] == [4] * (n - 1) + [0]
        assert [cost[t] for t in eq] == [2] * n and [code[t] for t in eq] == [0] + [4] * (n - 1)
    assert (want.cand[:, 4] > 0).all() and want.stats[5:] == [6, 0, 0, 0, 38]  # a loser keeps its record, and takes nothing else


def test_cap_and_ratio_on_their_limits():
    want = RC.reference("limits")
    assert want.cand[:, 6].tolist() == RC.LIMITS_CODES
    assert want.cand[:, 3].tolist() == [40, 41, 10, 10, 0, 0, 40, 40] and want.cand[:, 4].tolist() == [255, 255, 21, 20, -1, 0, 80, 81]


def test_every_reason_and_code_in_one_call():
    c, want = RC.cases()["everything"], RC.reference("everything")
    assert all(x > 0 for x in want.stats), want.stats
    assert sorted(set(want.cand[:, 6].tolist())) == [0, 1, 2, 3, 4]
    assert not np.isin(want.cand[:, 0], (9, 10)).any() and sum(want.stats) == 9 * 5
    masks = RC.reference("masks")
    m = RC.cases()["masks"]
    assert masks.stats[RR.NOT_SEARCHED] > 0 and masks.stats[RR.NO_POSE] > 0 and np.isin(masks.cand[:, 1], (0, 3, 5)).all() and m.use[masks.cand[:, 0]].all()


@pytest.mark.parametrize("name", ["tracks_17", "frames_9", "windows", "radius_1", "no_distractors"])
def test_a_frames_feature_order_does_not_matter(vm, name):
    """permuting every frame's records maps the result through the permutation (tie-free scenes)"""
    c = RC.cases()[name]
    assert c.tie_free
    rng = np.random.default_rng(5)
    feat, obs_feat = c.feat.copy(), c.obs_feat.copy()
    new_of = np.zeros(len(c.feat), np.int32)
    for g in range(len(c.poses)):
        a, b = int(c.feat_offsets[g]), int(c.feat_offsets[g + 1])
        perm = rng.permutation(b - a)  # perm[new] = old
        feat[a:b] = c.feat[a:b][perm]
        new_of[a:b] = np.argsort(perm)
    obs_feat = new_of[c.feat_offsets[c.obs_frames] + c.obs_feat]
    (poses, f, cu, cv, w, h, off, fr, _, xyz, fo, _), kw = c.args()
    got, want = vm.host_reobserve(poses, f, cu, cv, w, h, off, fr, obs_feat, xyz, fo, feat, **kw), RC.host(name)
    mapped = want.cand.copy()
    has = mapped[:, 2] >= 0
    mapped[has, 2] = new_of[c.feat_offsets[mapped[has, 1]] + mapped[has, 2]]
    assert got.cand.tobytes() == mapped.tobytes() and got.uv.tobytes() == want.uv.tobytes()
    assert got.track_accepted.tobytes() == want.track_accepted.tobytes() and got.frame_counts.tobytes() == want.frame_counts.tobytes()


@pytest.mark.parametrize("name", ["frames_9", "sweep_4", "everything", "claims"])
def test_a_frames_result_does_not_depend_on_the_other_frames(vm, name):
    c, full = RC.cases()[name], RC.host(name)
    a, kw = c.args()
    for g in range(len(c.poses)):
        only = np.zeros(len(c.poses), np.uint8)
        only[g] = 1
        if c.search is not None:
            only &= c.search
        got = vm.host_reobserve(*a, **{**kw, "search": only})
        rows = full.cand[:, 1] == g
        assert got.cand[:, :6].tobytes() == full.cand[rows, :6].tobytes() and got.uv.tobytes() == full.uv[rows].tobytes()
        assert got.cand[:, 6].tolist() == full.cand[rows, 6].tolist() and got.frame_counts[g].tolist() == full.frame_counts[g].tolist()


def _bad_calls(vm, c):
    (poses, f, cu, cv, w, h, off, fr, ft, xyz, fo, feat), kw = c.args()
    nan, inf = float("nan"), float("inf")
    T = len(off) - 1

    def changed(arr, i, v):
        out = arr.copy()
        out.reshape(-1)[i] = v
        return out

    good = dict(poses=poses, f=f, cu=cu, cv=cv, width=w, height=h, offsets=off, obs_frames=fr, obs_feat=ft, xyz=xyz, feat_offsets=fo, feat=feat, **kw)
    bad = [dict(obs_frames=changed(fr, 3, len(poses))), dict(obs_frames=changed(fr, 3, -1)), dict(offsets=changed(off, 3, off[2] - 1)), dict(offsets=changed(off, 0, 1)),
           dict(n_tracks=-2), dict(xyz=None), dict(params=vm._NO_PARAMS)]
    bad += [dict(params=p) for p in (dict(radius=-1.0), dict(radius=nan), dict(radius=inf), dict(min_depth=nan), dict(max_cost=-1), dict(ratio_num=-1, ratio_den=2),
                                     dict(ratio_num=1, ratio_den=-2), dict(ratio_num=0, ratio_den=2))]
    bad += [dict(width=0), dict(width=16384), dict(height=0), dict(height=16384), dict(feat_offsets=changed(fo, 0, 1)), dict(feat_offsets=changed(fo, 1, fo[2] + 1)),
            dict(obs_feat=changed(ft, 2, -1)), dict(obs_feat=changed(ft, 2, fo[fr[2] + 1] - fo[fr[2]])), dict(ref_obs=changed(c.middle_refs(), 1, off[2] - off[1])),
            dict(ref_obs=changed(c.middle_refs(), 1, -1)), dict(feat=changed(feat, 12 * 5 + 3, 4)), dict(feat=changed(feat, 12 * 5 + 3, -1)),
            dict(feat=changed(feat, 12 * 5, w)), dict(feat=changed(feat, 12 * 5, -1)), dict(feat=changed(feat, 12 * 5 + 1, h)), dict(feat=changed(feat, 12 * 5 + 1, -1))]
    assert T > 4
    return good, bad


def _call(fn, kw):
    kw = dict(kw)
    return fn(*[kw.pop(k) for k in ("poses", "f", "cu", "cv", "width", "height", "offsets", "obs_frames", "obs_feat", "xyz", "feat_offsets", "feat")], **kw)


def test_argument_errors_leave_the_outputs_untouched(vm):
    c = RC.cases()["frames_9"]
    good, bad = _bad_calls(vm, c)
    assert len(_call(vm.host_reobserve, good)) == len(RC.host("frames_9"))
    for over in bad:
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            _call(vm.host_reobserve, {**good, **over})
    # through the library itself: every output holds a pattern before the call and after it
    L = vm.lib()
    (poses, f, cu, cv, w, h, off, fr, ft, xyz, fo, feat), _ = c.args()
    T, n = len(off) - 1, len(RC.host("frames_9"))
    outs = [np.full((n, 7), -77, np.int32), np.full((n, 2), 7.5), np.full(T, -77, np.int32), np.full((len(poses), 2), -77, np.int32), np.full(10, -77, np.int64)]
    before = [o.copy() for o in outs]
    head = (len(poses), vm._ptr(poses), None, None, f, cu, cv, w, h, T, vm._ptr(off), vm._ptr(fr), vm._ptr(ft), vm._ptr(xyz), None, None, vm._ptr(fo))
    for ft_ptr, p, cap in ((vm._ptr(feat), vm.reobserve_params(radius=-1.0), n), (vm._ptr(feat), None, n), (None, vm.reobserve_params(), n),
                           (vm._ptr(feat), vm.reobserve_params(), -1)):
        assert L.vsm_host_reobserve(*head, ft_ptr, None if p is None else C.byref(p), cap, *[vm._ptr(o) for o in outs]) == -4
    assert all(a.tobytes() == b.tobytes() for a, b in zip(outs, before))
    # the smallest legal values pass; every output may be NULL; a short cap takes the first candidates
    p = vm.reobserve_params(radius=0.0, min_depth=-1e300, max_cost=0, ratio_num=1, ratio_den=1)
    assert L.vsm_host_reobserve(*head, vm._ptr(feat), C.byref(p), 0, None, None, None, None, None) == n
    assert L.vsm_host_reobserve(*head, vm._ptr(feat), C.byref(vm.reobserve_params()), 3, *[vm._ptr(o) for o in outs]) == n
    assert outs[0][:3].tobytes() == RC.host("frames_9").cand[:3].tobytes() and (outs[0][3:] == -77).all()


def test_both_forms_of_ref_obs(vm):
    for name in ("frames_9", "everything", "windows"):
        c = RC.cases()[name]
        a, kw = c.args()
        RR.assert_same(vm.host_reobserve(*a, **{**kw, "ref_obs": c.middle_refs()}), RC.host(name), name)
    # another reference observation: the track's last
    c = RC.cases()["frames_9"]
    a, kw = c.args()
    last = (np.diff(c.offsets) - 1).astype(np.int32)
    RR.assert_same(vm.host_reobserve(*a, **{**kw, "ref_obs": last}), RR.reobserve(*a, **{**kw, "ref_obs": last}), "the last observation as reference")


def _pixels(c):
    """the float pixel of every existing observation: its feature's"""
    return c.feat[c.feat_offsets[c.obs_frames] + c.obs_feat, :2].astype(np.float32)


@pytest.mark.parametrize("name", ["frames_9", "tracks_257", "radius_1", "masks"])
def test_extend_feeds_the_vetting(vm, name):
    """the window is a square of integer pixels around the projection: at the same poses and points a new observation's
    residual is at most radius * sqrt(2), so host_vet with max_residual just above that calls every one an inlier"""
    c, got = RC.cases()[name], RC.host(name)
    radius = dict(RR.DEFAULTS, **c.params)["radius"]
    off, fr, uv, ft = got.extend(c.offsets, c.obs_frames, _pixels(c), c.obs_feat)
    n_new = len(got.accepted())
    assert n_new > 0 and len(fr) == len(c.obs_frames) + n_new and off.dtype == np.int32 and fr.dtype == np.int32 and uv.dtype == np.float32 and ft.dtype == np.int32
    assert np.diff(off).tolist() == (np.diff(c.offsets) + got.track_accepted).tolist()
    for t in range(len(off) - 1):
        assert (np.diff(fr[off[t]:off[t + 1]]) > 0).all()  # ascending frames, none twice
    assert uv.tobytes() == c.feat[c.feat_offsets[fr] + ft, :2].astype(np.float32).tobytes()
    old = set(zip(np.repeat(np.arange(len(c.offsets) - 1), np.diff(c.offsets)).tolist(), c.obs_frames.tolist()))
    per_obs = np.repeat(np.arange(len(off) - 1), np.diff(off))
    is_new = np.array([(int(t), int(g)) not in old for t, g in zip(per_obs, fr)])
    assert is_new.sum() == n_new
    vet = vm.host_vet(c.poses, c.f, c.cu, c.cv, off, fr, uv, c.xyz, use=c.use, pose_valid=c.pose_valid,
                      params=dict(max_residual=radius * math.sqrt(2.0) * (1 + 1e-9) + 1e-9))
    assert (vet.code[is_new] == 0).all(), (name, vet.code[is_new].tolist())
    # and the next call finds nothing more in the frames it searched: every planted feature is taken
    again = vm.host_reobserve(c.poses, c.f, c.cu, c.cv, c.width, c.height, off, fr, ft, c.xyz, c.feat_offsets, c.feat, use=c.use, search=c.search,
                              pose_valid=c.pose_valid, params=c.params)
    assert len(again.accepted()) == 0 or name == "masks"


def test_extend_feeds_the_resection_and_the_adjustment(vm):
    c, got = RC.cases()["frames_9"], RC.host("frames_9")
    off, fr, uv, ft = got.extend(c.offsets, c.obs_frames, _pixels(c), c.obs_feat)
    before = vm.host_resect(c.poses, c.f, c.cu, c.cv, c.offsets, c.obs_frames, _pixels(c), c.xyz, params=dict(min_observations=6))
    after = vm.host_resect(c.poses, c.f, c.cu, c.cv, off, fr, uv, c.xyz, params=dict(min_observations=6))
    assert (after.rows >= before.rows).all() and after.rows.sum() == before.rows.sum() + len(got.accepted()) and (after.status == 0).sum() >= (before.status == 0).sum() > 0
    adj = vm.host_adjust(c.poses, c.f, c.cu, c.cv, off, fr, uv, c.xyz, params=dict(min_observations=6, max_rounds=2, cg_iters=10))
    assert adj.rows.sum() == after.rows.sum() and np.isfinite(adj.poses).all() and (adj.frame_status == 0).any()


def test_interface(vm):
    L = vm.lib()
    p = vm.reobserve_params()
    assert C.sizeof(vm.VsmReobserveParams) == 32
    assert (p.radius, p.min_depth, p.max_cost, p.ratio_num, p.ratio_den) == (4.0, 1e-10, 0, 0, 0) == tuple(RR.DEFAULTS[k] for k in ("radius", "min_depth", "max_cost",
                                                                                                                                      "ratio_num", "ratio_den"))
    names = [L.vsm_kernel_name(i).decode() for i in range(L.vsm_num_kernels())]
    assert all(names) and all(names.count(k) == 1 for k in ("k_ro_occupy", "k_ro_bin_count", "k_ro_scatter", "k_ro_project<count>", "k_ro_project<list>", "k_ro_search",
                                                             "k_ro_verdict"))
    assert len(vm.REOBSERVE_REASONS) == 5 and len(vm.REOBSERVE_CODES) == 5 and len(vm.REOBSERVE_STATS) == 10 and len(vm.REOBSERVE_TIMINGS) == 4
    for s in ("vsm_reobserve_default_params", "vsm_reobserve_run", "vsm_points_reobserve", "vsm_reobserve_count", "vsm_reobserve_get", "vsm_reobserve_get_tracks",
              "vsm_reobserve_get_frames", "vsm_reobserve_get_stats", "vsm_reobserve_get_timings", "vsm_host_reobserve", "vsm_pairs_num_features", "vsm_pairs_get_features"):
        assert s in vm.EXPORTS and hasattr(L, s), s
    assert all(hasattr(vm.Matcher, m) for m in ("reobserve", "reobserve_points", "pair_features")) and hasattr(vm.Reobservation, "extend")
