"""CPU suite: vsm_host_fuse - the fusion's host view, one thread walking csrc/vsm_fuse.h - against tests/fuse_ref.py, the
definition restated in plain Python ints and floats without any index: every array equal by its bytes, on all cases of
tests/fuse_cases.py.  Then what the cases are for is checked on the restatement's own result, so that a case that no longer
reaches its size, its tie, its conflict or its code fails here and not silently; the split scenes come back byte for byte, the
three-way splits in two calls and not in one; a frame's feature order and frames that are not searched do not matter; every
argument error is returned with the outputs untouched; and the merged track set feeds the triangulation, the adjustment and the
vetting, where the merged tracks' points are no further from the truth than the fragments'."""
import ctypes as C
import math

import numpy as np
import pytest

import fuse_cases as FC
import fuse_ref as FR
import reobserve_cases as RC
import reobserve_ref as RR
from conftest import pkg


@pytest.fixture(scope="module")
def vm():
    m = pkg("visomatch")
    m.lib()
    return m


def _in_use(c):
    T = len(c.offsets) - 1 if len(c.offsets) else 0
    return (np.ones(T, bool) if c.use is None else c.use[:T].astype(bool)) & (np.diff(c.offsets) > 0) if T else np.zeros(0, bool)


@pytest.mark.parametrize("name", sorted(FC.cases()))
def test_host_view_equals_the_restatement(vm, name):
    got, want = FC.host(name), FC.reference(name)
    FR.assert_same(got, want, name)
    assert [got.stats[k] for k in vm.FUSE_STATS] == want.stats
    c = FC.cases()[name]
    s = want.stats
    # the stats add up: pairs, candidates, proposals, fusions
    assert sum(s[:12]) == int(_in_use(c).sum()) * len(c.poses)
    assert sum(s[5:12]) == want.frame_counts[:, 0].sum() and sum(s[5:12]) - s[6] == len(want.prop) == want.frame_counts[:, 1].sum()
    assert s[5] == 2 * s[12] == 2 * (want.fused_into >= 0).sum() == 2 * len(got.fused())
    order = want.prop[:, 0].astype(np.int64) * (len(c.poses) + 1) + want.prop[:, 1]
    assert (np.diff(order) > 0).all()  # ascending (a, g)
    # obs_src is a permutation; the merged lengths are the fragments' sums
    assert sorted(want.obs_src.tolist()) == list(range(len(c.obs_frames)))
    n = np.diff(c.offsets) if len(c.offsets) else np.zeros(0, int)
    after = n.copy()
    for s_, a in got.fused():
        assert want.partner[s_] == a and want.partner[a] == s_ and s_ < a and _in_use(c)[[s_, a]].all()
        after[s_] += n[a]
        after[a] = 0
        fr = c.obs_frames[want.obs_src[want.offsets_after[s_]:want.offsets_after[s_ + 1]]]
        assert (np.diff(fr) > 0).all() or name == "twice"
    assert np.diff(want.offsets_after).tolist() == after.tolist()


def _check_recovered(vm, c, fusion, final=True):
    """Fusion.merge on a split scene against the unsplit one"""
    u, T = c.unsplit, c.n_points
    off, fr, uv, ft = fusion.merge(c.obs_frames, FC.pixels(c), c.obs_feat)
    assert off.dtype == np.int32 and fr.dtype == np.int32 and uv.dtype == np.float32 and ft.dtype == np.int32
    same = off[:T + 1].tobytes() == u.offsets.tobytes() and (off[T:] == off[T]).all()
    if final:
        assert same and fr.tobytes() == u.obs_frames.tobytes() and ft.tobytes() == u.obs_feat.tobytes() and uv.tobytes() == FC.pixels(u).tobytes()
    return same, (off, fr, uv, ft)


SPLITS = sorted(n for n, c in FC.cases().items() if hasattr(c, "unsplit") and c.ways == 2 and len(c.offsets) - 1 == 2 * c.n_points and n != "masks")


@pytest.mark.parametrize("name", SPLITS)
def test_the_split_scene_comes_back(vm, name):
    c, got = FC.cases()[name], FC.host(name)
    _check_recovered(vm, c, got)
    T = c.n_points
    two = np.diff(c.offsets)[T:] > 0  # the tracks that were cut
    assert got.fused().tolist() == [[t, T + t] for t in np.nonzero(two)[0]]
    fused = got.prop[got.code == 0]
    assert (fused[:, 3] <= 64).all() and len(fused) == 2 * two.sum()
    assert two.sum() > 5 or name.startswith(("tracks_", "frames_1"))


def test_families():
    for n in FC.TRACK_COUNTS:
        assert len(FC.cases()["tracks_%d" % n].offsets) - 1 == n
        assert len(FC.reference("tracks_%d" % n).fused_into) == n
    for n in FC.FRAME_COUNTS:
        assert len(FC.cases()["frames_%d" % n].poses) == n
    assert len(FC.host("tracks_257").fused()) > 100 and len(FC.host("tracks_1").prop) == 0 and len(FC.host("frames_33").fused()) > 8
    assert len(FC.host("frames_1").prop) == 0 and FC.reference("frames_1").stats[RR.OBSERVED] > 0
    for n in FC.PROPOSAL_COUNTS:
        want = FC.reference("proposals_%d" % n)
        assert len(want.prop) == n and (want.prop[:, 6] == FR.ONE_SIDED).all() and (want.prop[:, 7] == n).all() and (want.prop[:, 5] == 1).all()
    # the masked scene: only searched frames with a pose, only tracks in use, on either side of a proposal
    m, want = FC.cases()["masks"], FC.reference("masks")
    use = np.tile(m.unsplit.use, 2)
    assert want.stats[RR.NOT_SEARCHED] > 0 and want.stats[RR.NO_POSE] > 0 and np.isin(want.prop[:, 1], (0, 3, 5)).all()
    assert use[want.prop[:, 0]].all() and use[want.prop[:, 7]].all() and len(FC.host("masks").fused()) > 3


def test_three_way_splits_need_two_calls(vm):
    for name in ("three_ways", "three_ways_interleaved"):
        c, first = FC.cases()[name], FC.host(name)
        T = c.n_points
        three = np.nonzero(np.diff(c.offsets)[2 * T:] > 0)[0]
        assert len(three) > 8
        same, (off, fr, uv, ft) = _check_recovered(vm, c, first, final=False)
        assert not same
        assert first.fused().tolist() == [[t, T + t] for t in np.nonzero(np.diff(c.offsets)[T:2 * T] > 0)[0]]  # the first two fragments; the third is one-sided
        assert (first.prop[np.isin(first.prop[:, 0], 2 * T + three), 6] >= FR.OUTBID).all()
        assert sorted(first.obs_src.tolist()) == list(range(len(c.obs_frames)))
        a, kw = c.args()
        second = vm.host_fuse(*a[:6], off, fr, ft, *a[9:], **kw)
        assert second.fused().tolist() == [[t, 2 * T + t] for t in three]
        off2, fr2, uv2, ft2 = second.merge(fr, uv, ft)
        u = c.unsplit
        assert off2[:T + 1].tobytes() == u.offsets.tobytes() and (off2[T:] == off2[T]).all()
        assert fr2.tobytes() == u.obs_frames.tobytes() and ft2.tobytes() == u.obs_feat.tobytes() and uv2.tobytes() == FC.pixels(u).tobytes()
        # and a third call finds nothing to fuse
        assert len(vm.host_fuse(*a[:6], off2, fr2, ft2, *a[9:], **kw).fused()) == 0


def test_window_sizes_classes_and_free_features():
    want = FC.reference("windows")
    assert want.prop[:, 5].tolist() == list(FC.WINDOW_SIZES[1:])  # the free feature and those of the other classes, cost 0, are not counted
    assert want.stats[5 + FR.EMPTY] >= 1 and (want.prop[:, 3] > 0).all() and want.prop[0, 4] == -1 and (want.prop[1:, 4] >= want.prop[1:, 3]).all()
    assert (want.prop[:, 7] == len(FC.WINDOW_SIZES)).all() and (want.prop[:, 6] == FR.ONE_SIDED).all()


@pytest.mark.parametrize("name", sorted(n for n in FC.cases() if n.startswith("carpet_")))
def test_the_windows_are_the_complement_of_the_reobservations(vm, name):
    """with every free feature handed to one more track, the fusion sees what the re-observation saw"""
    c, want = FC.cases()[name], FC.reference(name)
    a, kw = c.plain.args()
    ro = RR.reobserve(*a, **kw)
    if name == "carpet_half_windows":
        # half of the free features owned: what the fusion sees and what the re-observation still sees add up to the whole
        a, kw = c.args()
        left = {(int(r[0]), int(r[1])): int(r[5]) for r in RR.reobserve(*a, **kw).cand}
        mine = {(int(r[0]), int(r[1])): int(r[5]) for r in want.prop}
        assert all(mine.get(k, 0) + left[k] == int(r[5]) for r in ro.cand for k in [(int(r[0]), int(r[1]))])
        assert sum(mine.values()) > 20 and sum(left.values()) > 20 and (want.prop[:, 5] < ro.cand[ro.cand[:, 5] > 0][-len(want.prop):, 5]).any()
        return
    full = ro.cand[:, 5] > 0
    assert want.prop[:, :6].tobytes() == ro.cand[full, :6].tobytes() and want.uv.tobytes() == ro.uv[full].tobytes()
    assert want.stats[:5] == [x + y for x, y in zip(ro.stats[:5], [0, 0, len(c.poses) - 1, 1, 0])] and (want.prop[:, 7] == c.carpet).all()


@pytest.mark.parametrize("name,radius", [("carpet_sweep_4", 4.0), ("carpet_sweep_2_5", 2.5), ("carpet_sweep_2_5_half", 2.5), ("carpet_sweep_0", 0.0)])
def test_sweep_window_edges(name, radius):
    """the window's size in closed form: columns u with |u - pu| <= radius inside the frame, times the rows within radius"""
    want, r = FC.reference(name), int(math.floor(radius))
    rows = sum(1 for dv in (-(r + 1), -r, 0, r, r + 1) if abs(dv) <= radius)
    width = FC.cases()[name].width
    assert len(want.prop) >= width - 1
    for row, (pu, pv) in zip(want.prop, want.uv):
        assert row[5] == rows * sum(1 for u in range(width) if abs(u - pu) <= radius), (name, row.tolist(), pu)


def test_non_finite_inputs():
    c, want = FC.cases()["carpet_edges"], FC.reference("carpet_edges")
    assert (want.prop[:, 1] == 1).all() and len(want.prop) == 7 and np.isfinite(want.uv).all()  # the frames with a NaN or an infinity in their pose give none
    assert want.stats[RR.BEHIND] + want.stats[RR.OUTSIDE] + len(want.prop) + want.stats[5 + FR.EMPTY] == 3 * (len(c.xyz) - 1) + 1  # (the carpet track: behind frame 0's camera, observed in the others)


def test_fragments_of_every_length_and_interleaved_lists():
    c, want = FC.cases()["fragments"], FC.reference("fragments")
    assert want.fused().tolist() if hasattr(want, "fused") else True
    pairs = {int(b): int(a) for a, b in c.pairs}
    assert {int(t): int(s) for t, s in enumerate(want.fused_into) if s >= 0} == pairs
    n = np.diff(c.offsets)
    assert sorted(set(n.tolist())) == [1, 2, 8, 9, 16, 17, 33, 257]
    for a, b in c.pairs:
        src = want.obs_src[want.offsets_after[a]:want.offsets_after[a + 1]]
        assert len(src) == n[a] + n[b] and (np.diff(c.obs_frames[src]) > 0).all()
    a, b = c.pairs[-1]  # the smaller index holds the odd frames: the merged list starts with the absorbed track's
    assert want.obs_src[want.offsets_after[a]] == c.offsets[b] and want.obs_src[want.offsets_after[a] + 1] == c.offsets[a]


def test_conflicts_and_frames_seen_twice():
    c, want = FC.cases()["conflicts"], FC.reference("conflicts")
    assert len(want.prop) == 2 * 7 * 4 and (want.prop[:, 6] == FR.CONFLICT).all() and (want.partner == -1).all() and want.stats[12] == 0
    assert want.obs_src.tolist() == list(range(len(c.obs_frames))) and want.offsets_after.tobytes() == c.offsets.tobytes()
    c, want = FC.cases()["twice"], FC.reference("twice")
    assert want.fused_into.tolist() == [-1, 0, -1, 2, -1, -1]
    assert c.obs_frames[want.obs_src].tolist() == [1, 1, 2, 3] + [1, 3, 3, 4] + [2, 2, 0, 2, 5]
    assert want.obs_src[:8].tolist() == [0, 1, 2, 3, 5, 6, 7, 4]  # stable: equal frames keep their order
    assert (want.prop[np.isin(want.prop[:, 0], (4, 5)), 6] == FR.CONFLICT).all() and np.isin(want.prop[:, 0], (4, 5)).sum() == 2


def test_owners():
    want = FC.reference("owners")
    assert want.prop[:, [0, 1, 7]].tolist() == [[0, 1, 3], [1, 1, 6]] and (want.prop[:, 6] == FR.ONE_SIDED).all()
    assert want.partner.tolist() == [3, 6, -1, -1, -1, -1, -1, -1] and want.stats[5 + FR.EMPTY] == 1 + 3 + 3


def test_ties_and_the_chain():
    want = FC.reference("ties")
    assert want.prop[0].tolist() == [0, 1, 1, 7, 7, 4, FR.ONE_SIDED, 1]  # three features at cost 7: the lowest index, its owner; second = best
    t3 = want.prop[want.prop[:, 0] == 3]
    assert t3[:, [1, 3, 6, 7]].tolist() == [[1, 5, FR.ONE_SIDED, 4], [2, 5, FR.OUTBID, 5]]  # equal costs: the lower proposal is the choice
    assert want.partner.tolist() == [1, -1, -1, 4, 5, 4] and want.fused_into.tolist() == [-1, -1, -1, -1, -1, 4]
    want = FC.reference("chain")
    assert want.prop[:, [0, 1, 3, 6, 7]].tolist() == [[0, 1, 10, 6, 1], [0, 2, 14, 5, 2], [1, 0, 10, 5, 0], [1, 2, 4, 0, 2], [2, 0, 14, 5, 0], [2, 1, 4, 0, 1]]
    assert want.partner.tolist() == [1, 2, 1] and want.fused_into.tolist() == [-1, -1, 1]


def test_cap_and_ratio_on_their_limits():
    want = FC.reference("limits")
    assert want.prop[:, 6].tolist() == FC.LIMITS_CODES
    assert want.prop[:, 3].tolist() == [40, 41, 10, 10, 0, 0, 40, 40] and want.prop[:, 4].tolist() == [255, 255, 21, 20, -1, 0, 80, 81]


def test_every_reason_and_code_in_one_call():
    want = FC.reference("everything")
    assert all(x > 0 for x in want.stats), want.stats
    assert sorted(set(want.prop[:, 6].tolist())) == [0, 2, 3, 4, 5, 6] and want.stats[12] == 2
    assert not np.isin(want.prop[:, [0, 7]], (14, 15)).any() and sum(want.stats[:12]) == 14 * 6
    assert want.fused_into.tolist() == [-1, 0] + [-1] * 9 + [10] + [-1] * 4


@pytest.mark.parametrize("name", ["tracks_17", "frames_9", "split_8", "split_radius_1", "three_ways"])
def test_a_frames_feature_order_does_not_matter(vm, name):
    """permuting every frame's records maps the result through the permutation"""
    c = FC.cases()[name]
    rng = np.random.default_rng(5)
    feat = c.feat.copy()
    new_of = np.zeros(len(c.feat), np.int32)
    for g in range(len(c.poses)):
        a, b = int(c.feat_offsets[g]), int(c.feat_offsets[g + 1])
        perm = rng.permutation(b - a)  # perm[new] = old
        feat[a:b] = c.feat[a:b][perm]
        new_of[a:b] = np.argsort(perm)
    obs_feat = new_of[c.feat_offsets[c.obs_frames] + c.obs_feat]
    (poses, f, cu, cv, w, h, off, fr, _, xyz, fo, _), kw = c.args()
    got, want = vm.host_fuse(poses, f, cu, cv, w, h, off, fr, obs_feat, xyz, fo, feat, **kw), FC.host(name)
    mapped = want.prop.copy()
    mapped[:, 2] = new_of[c.feat_offsets[mapped[:, 1]] + mapped[:, 2]]
    want_ = vm.Fusion(mapped, want.uv, want.partner, want.fused_into, want.offsets_after, want.obs_src, want.frame_counts)
    FR.assert_same(got, want_, name)
    assert got.stats == want.stats


@pytest.mark.parametrize("name", ["frames_9", "split_8", "everything", "chain"])
def test_frames_that_are_not_searched_do_not_matter(vm, name):
    """three more frames in front, with features and valid poses but not searched and observed by nobody: the same result
    with every frame index moved by three"""
    c, want = FC.cases()[name], FC.host(name)
    (poses, f, cu, cv, w, h, off, fr, ft, xyz, fo, feat), kw = c.args()
    extra = np.array([[5, 6, 0, 1] + [7] * 8] * 4, np.int32)
    F = len(poses)
    poses2 = np.vstack([poses[:1].repeat(3, axis=0), poses])
    fo2 = np.concatenate([[0, 4, 8, 12], fo[1:] + 12]).astype(np.int32)
    feat2 = np.vstack([extra] * 3 + [feat])
    search = np.concatenate([[0, 0, 0], np.ones(F, np.uint8) if c.search is None else c.search]).astype(np.uint8)
    valid = np.concatenate([[1, 1, 1], np.ones(F, np.uint8) if c.pose_valid is None else c.pose_valid]).astype(np.uint8)
    got = vm.host_fuse(poses2, f, cu, cv, w, h, off, fr + 3, ft, xyz, fo2, feat2, **{**kw, "search": search, "pose_valid": valid})
    moved = want.prop.copy()
    moved[:, 1] += 3
    FR.assert_same(got, vm.Fusion(moved, want.uv, want.partner, want.fused_into, want.offsets_after, want.obs_src, np.vstack([np.zeros((3, 2), np.int32), want.frame_counts])), name)
    assert got.stats["pairs_not_searched"] == want.stats["pairs_not_searched"] + 3 * int(_in_use(c).sum())


def _bad_calls(vm, c):
    (poses, f, cu, cv, w, h, off, fr, ft, xyz, fo, feat), kw = c.args()
    nan, inf = float("nan"), float("inf")

    def changed(arr, i, v):
        out = arr.copy()
        out.reshape(-1)[i] = v
        return out

    middle = np.maximum((np.diff(off) - 1) // 2, 0).astype(np.int32)
    good = dict(poses=poses, f=f, cu=cu, cv=cv, width=w, height=h, offsets=off, obs_frames=fr, obs_feat=ft, xyz=xyz, feat_offsets=fo, feat=feat, **kw)
    bad = [dict(obs_frames=changed(fr, 3, len(poses))), dict(obs_frames=changed(fr, 3, -1)), dict(offsets=changed(off, 3, off[2] - 1)), dict(offsets=changed(off, 0, 1)),
           dict(n_tracks=-2), dict(xyz=None), dict(params=vm._NO_PARAMS)]
    bad += [dict(params=p) for p in (dict(radius=-1.0), dict(radius=nan), dict(radius=inf), dict(min_depth=nan), dict(max_cost=-1), dict(ratio_num=-1, ratio_den=2),
                                     dict(ratio_num=1, ratio_den=-2), dict(ratio_num=0, ratio_den=2))]
    bad += [dict(width=0), dict(width=16384), dict(height=0), dict(height=16384), dict(feat_offsets=changed(fo, 0, 1)), dict(feat_offsets=changed(fo, 1, fo[2] + 1)),
            dict(obs_feat=changed(ft, 2, -1)), dict(obs_feat=changed(ft, 2, fo[fr[2] + 1] - fo[fr[2]])), dict(ref_obs=changed(middle, 1, off[2] - off[1])),
            dict(ref_obs=changed(middle, 1, -1)), dict(feat=changed(feat, 12 * 5 + 3, 4)), dict(feat=changed(feat, 12 * 5 + 3, -1)),
            dict(feat=changed(feat, 12 * 5, w)), dict(feat=changed(feat, 12 * 5, -1)), dict(feat=changed(feat, 12 * 5 + 1, h)), dict(feat=changed(feat, 12 * 5 + 1, -1))]
    return good, bad


def _call(fn, kw):
    kw = dict(kw)
    return fn(*[kw.pop(k) for k in ("poses", "f", "cu", "cv", "width", "height", "offsets", "obs_frames", "obs_feat", "xyz", "feat_offsets", "feat")], **kw)


def test_argument_errors_leave_the_outputs_untouched(vm):
    c = FC.cases()["frames_9"]
    good, bad = _bad_calls(vm, c)
    assert len(_call(vm.host_fuse, good)) == len(FC.host("frames_9"))
    for over in bad:
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            _call(vm.host_fuse, {**good, **over})
    # through the library itself: every output holds a pattern before the call and after it
    L = vm.lib()
    (poses, f, cu, cv, w, h, off, fr, ft, xyz, fo, feat), _ = c.args()
    T, n = len(off) - 1, len(FC.host("frames_9"))
    outs = [np.full((n, 8), -77, np.int32), np.full((n, 2), 7.5), np.full(T, -77, np.int32), np.full(T, -77, np.int32), np.full(T + 1, -77, np.int32),
            np.full(len(fr), -77, np.int32), np.full((len(poses), 2), -77, np.int32), np.full(13, -77, np.int64)]
    before = [o.copy() for o in outs]
    head = (len(poses), vm._ptr(poses), None, None, f, cu, cv, w, h, T, vm._ptr(off), vm._ptr(fr), vm._ptr(ft), vm._ptr(xyz), None, None, vm._ptr(fo))
    for ft_ptr, p, cap in ((vm._ptr(feat), vm.fuse_params(radius=-1.0), n), (vm._ptr(feat), None, n), (None, vm.fuse_params(), n), (vm._ptr(feat), vm.fuse_params(), -1)):
        assert L.vsm_host_fuse(*head, ft_ptr, None if p is None else C.byref(p), cap, *[vm._ptr(o) for o in outs]) == -4
    assert all(a.tobytes() == b.tobytes() for a, b in zip(outs, before))
    # the smallest legal values pass; every output may be NULL; a short cap takes the first proposals
    p = vm.fuse_params(radius=0.0, min_depth=-1e300, max_cost=0, ratio_num=1, ratio_den=1)
    assert L.vsm_host_fuse(*head, vm._ptr(feat), C.byref(p), 0, *[None] * 8) >= 0
    assert L.vsm_host_fuse(*head, vm._ptr(feat), C.byref(vm.fuse_params()), 3, *[vm._ptr(o) for o in outs]) == n
    assert outs[0][:3].tobytes() == FC.host("frames_9").prop[:3].tobytes() and (outs[0][3:] == -77).all() and outs[4].tobytes() == FC.host("frames_9").offsets_after.tobytes()


def test_both_forms_of_ref_obs(vm):
    for name in ("frames_9", "everything", "fragments"):
        c = FC.cases()[name]
        a, kw = c.args()
        FR.assert_same(vm.host_fuse(*a, **{**kw, "ref_obs": c.middle_refs()}), FC.host(name), name)
    c = FC.cases()["split_8"]
    a, kw = c.args()
    last = np.maximum(np.diff(c.offsets) - 1, 0).astype(np.int32)
    FR.assert_same(vm.host_fuse(*a, **{**kw, "ref_obs": last}), FR.fuse(*a, **{**kw, "ref_obs": last}), "the last observation as reference")


def test_the_merged_set_feeds_triangulation_adjustment_and_vetting(vm):
    """pixel noise on a split scene: the fragments and the merged tracks are triangulated, adjusted and vetted alike; a merged
    track sees its point from more frames than either fragment, so over the fused tracks the merged points lie no further
    from the truth than the fragments' points - one set against the other, no threshold"""
    c, got = FC.cases()["split_8"], FC.host("split_8")
    T = c.n_points
    rng = np.random.default_rng(11)
    px = (FC.pixels(c) + rng.normal(0.0, 0.4, (len(c.obs_frames), 2))).astype(np.float32)
    off, fr, uv, ft = got.merge(c.obs_frames, px, c.obs_feat)
    truth = c.unsplit.xyz

    def points(offsets, frames, pixels):
        tri = vm.host_triangulate(c.poses, c.f, c.cu, c.cv, offsets, frames, pixels, params=dict(point_type=-1, max_dist=1000.0, min_angle=0.0))
        ok = tri.status == 0
        adj = vm.host_adjust(c.poses, c.f, c.cu, c.cv, offsets, frames, pixels, tri.xyz, use=ok, refine=np.zeros(len(c.poses), np.uint8),
                             params=dict(min_track_observations=2, max_rounds=5))
        vet = vm.host_vet(c.poses, c.f, c.cu, c.cv, offsets, frames, pixels, adj.xyz, use=ok, params=dict(max_residual=3.0))
        return adj.xyz, ok & (adj.track_status == 0), vet

    xyz_f, ok_f, vet_f = points(c.offsets, c.obs_frames, px)
    xyz_m, ok_m, vet_m = points(off, fr, uv)
    fused = got.fused()
    both = [(s, a) for s, a in fused if ok_m[s] and ok_f[s] and ok_f[a]]
    assert len(both) > 10 and ok_m[fused[:, 0]].sum() >= max(ok_f[fused[:, 0]].sum(), ok_f[fused[:, 1]].sum())
    err_m = np.array([np.linalg.norm(xyz_m[s] - truth[s]) for s, a in both])
    err_f = np.array([[np.linalg.norm(xyz_f[s] - truth[s]), np.linalg.norm(xyz_f[a] - truth[s])] for s, a in both])
    assert np.median(err_m) <= np.median(err_f.min(axis=1)) and err_m.sum() <= err_f.mean(axis=1).sum()
    assert (vet_m.code[np.repeat(ok_m, np.diff(off))] == 0).sum() >= (vet_f.code[np.repeat(ok_f, np.diff(c.offsets))] == 0).sum() * 0.9


def test_interface(vm):
    L = vm.lib()
    p = vm.fuse_params()
    assert C.sizeof(vm.VsmFuseParams) == 32
    assert (p.radius, p.min_depth, p.max_cost, p.ratio_num, p.ratio_den) == (4.0, 1e-10, 0, 0, 0) == tuple(FR.DEFAULTS[k] for k in ("radius", "min_depth", "max_cost",
                                                                                                                                      "ratio_num", "ratio_den"))
    names = [L.vsm_kernel_name(i).decode() for i in range(L.vsm_num_kernels())]
    assert all(names) and all(names.count(k) == 1 for k in ("k_fu_owner", "k_fu_bin_count", "k_fu_scatter", "k_fu_search<count>", "k_fu_search<list>", "k_fu_conflict",
                                                             "k_fu_verdict", "k_fu_lengths", "k_fu_merge"))
    assert len(vm.FUSE_CODES) == 7 and len(vm.FUSE_STATS) == 13 == FR.N_STATS and len(vm.FUSE_TIMINGS) == 4
    for s in ("vsm_fuse_default_params", "vsm_fuse_run", "vsm_points_fuse", "vsm_fuse_count", "vsm_fuse_get", "vsm_fuse_get_tracks", "vsm_fuse_get_merged",
              "vsm_fuse_get_frames", "vsm_fuse_get_stats", "vsm_fuse_get_timings", "vsm_host_fuse"):
        assert s in vm.EXPORTS and hasattr(L, s), s
