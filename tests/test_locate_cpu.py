"""CPU suite: vsm_host_locate - the location's host view, one thread walking csrc/vsm_locate.h - on the cases of
tests/locate_cases.py.  The call as a whole has no counterpart to compare with (its stages have one: tests/locate_ref.py,
test_locate_kernels_cpu.py), so it is pinned from four sides: against the two stages whose
arithmetic it shares (the located poses are host_resect's from the linear poses, byte for byte; the winner's count is host_vet's
inlier count at the linear pose), against the truth the scenes were made from, against itself under a change of frame order and
of the frames in the call, and by what the cases are for - every status in one call, the row and hypothesis counts, the hard
inputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import locate_cases as LC
from conftest import ROOT, pkg

# The largest absolute difference, over every located frame of every case with a truth, between the located pose and
# host_resect started at the TRUE pose on the same rows with the same gate: both end within eps of the same minimum, and what
# is left is convergence noise.  Measured on the CPU (test_pose_against_truth prints it): 1.22e-14.  The bound is ten times that.
MEASURED_POSE_DIFFERENCE = 1.22e-14


@pytest.fixture(scope="module")
def vm():
    m = pkg("visomatch")
    m.lib()
    return m


def resect_params(vm, c):
    """the resection as the location asks for it"""
    p = vm.locate_params(**c.params)
    return dict(min_observations=p.min_inliers, max_updates=p.max_updates, eps=p.eps, max_residual=p.inlier_threshold, min_depth=p.min_depth)


def vet_params(vm, c):
    p = vm.locate_params(**c.params)
    return dict(max_residual=p.inlier_threshold, min_depth=p.min_depth)


WITH_TRUTH = sorted(n for n, c in LC.cases().items() if c.true_poses is not None)


def test_interface(vm):
    L = vm.lib()
    p = vm.locate_params()
    assert C.sizeof(vm.VsmLocateParams) == 48
    assert (p.ransac_iters, p.inlier_threshold, p.min_inliers, p.min_depth, p.seed, p.max_updates, p.eps) == (200, 2.0, 10, 1e-10, 71, 20, 1e-8)
    names = [L.vsm_kernel_name(i).decode() for i in range(L.vsm_num_kernels())]
    assert all(names) and all(names.count(k) == 1 for k in ("k_locate_fit", "k_locate_count", "k_locate_winner", "k_rs_resect"))
    assert len(vm.LOCATE_STATUS) == 7 and len(vm.LOCATE_TIMINGS) == 4
    for s in ("vsm_locate_default_params", "vsm_locate_run", "vsm_points_locate", "vsm_locate_count", "vsm_locate_get", "vsm_locate_get_stats",
              "vsm_locate_get_timings", "vsm_host_locate"):
        assert s in vm.EXPORTS and hasattr(L, s), s
    assert all(hasattr(vm.Matcher, m) for m in ("locate", "locate_points"))
    r = LC.host("mask")
    assert r.located().tolist() == [False, True, True, False, True, False] and len(r) == 6


def test_the_definition_is_rational():
    """no trigonometric function, and none of libm's but fabs, in the shared header (sqrt is inside the decompositions)"""
    txt = open(os.path.join(ROOT, "opencl-structure-from-motion_amd", "csrc", "vsm_locate.h")).read()
    code = re.sub(r"//.*", "", txt)
    assert not re.search(r"\b(sin|cos|tan|asin|acos|atan|atan2|sincos|sqrt|exp|pow|isfinite|isnan)\s*\(", code)


def test_argument_checks_leave_the_outputs_untouched(vm):
    c = LC.cases()["frames_2"]
    (n, f, cu, cv, off, fr, uv, xyz), kw = c.args()
    L = vm.lib()
    bad_fr = fr.copy()
    bad_fr[3] = n
    dec = off.copy()
    dec[3] = dec[2] - 1
    shifted = off.copy()
    shifted[0] = 1
    nan, inf = float("nan"), float("inf")
    calls = [dict(fr=bad_fr), dict(off=dec), dict(off=shifted), dict(T=-2), dict(n=-1), dict(xyz=None), dict(params=None)]
    calls += [dict(params=vm.locate_params(**p)) for p in (dict(ransac_iters=0), dict(ransac_iters=-5), dict(inlier_threshold=0.0), dict(inlier_threshold=-2.0),
                                                           dict(inlier_threshold=inf), dict(inlier_threshold=nan), dict(min_inliers=5), dict(max_updates=0),
                                                           dict(eps=0.0), dict(eps=-1e-8), dict(eps=inf), dict(eps=nan))]
    for over in calls:
        a = dict(n=n, off=off, fr=fr, uv=uv, xyz=xyz, T=len(off) - 1, params=vm.locate_params())
        a.update(over)
        out = vm._locate_arrays(2)
        for o in out:
            o.fill(77)
        before = [o.copy() for o in out]
        prm = None if a["params"] is None else C.byref(a["params"])
        rc = L.vsm_host_locate(a["n"], None, f, cu, cv, a["T"], vm._ptr(a["off"]), vm._ptr(a["fr"]), vm._ptr(a["uv"]), vm._ptr(a["xyz"]), None, prm,
                               *[vm._ptr(o) for o in out])
        assert rc == -4, (over, rc)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(out, before)), over
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        vm.host_locate(n, f, cu, cv, off, bad_fr, uv, xyz)
    # what is accepted: the smallest parameters, no outputs at all, frames without tracks
    assert L.vsm_host_locate(n, None, f, cu, cv, len(off) - 1, vm._ptr(off), vm._ptr(fr), vm._ptr(uv), vm._ptr(xyz), None, C.byref(vm.locate_params()), *[None] * 11) == n
    assert L.vsm_host_locate(3, None, f, cu, cv, 0, None, None, None, None, None, C.byref(vm.locate_params()), *[None] * 11) == 3
    r = vm.host_locate(n, f, cu, cv, off, fr, uv, xyz, params=dict(ransac_iters=1, min_inliers=6, max_updates=1))
    assert r.status.tolist() in ([0, 0], [6, 6], [0, 6], [6, 0])


def test_every_status_in_one_call():
    r = LC.host("statuses")
    assert r.status.tolist() == [1, 2, 3, 4, 5, 0, 6]
    assert r.eligible.tolist() == [0, 7, 12, 12, 14, 40, 40] and r.rows.tolist() == [40, 7, 12, 12, 14, 40, 40]
    assert r.best[:3].tolist() == [-1, -1, -1] and r.inliers[:3].tolist() == [0, 0, 0] and r.inliers[3] < 10
    assert (r.poses[:4] == 0).all() and (r.linear_poses[:3] == 0).all()
    assert r.poses[4].tobytes() == r.linear_poses[4].tobytes() and r.inliers[4] == 14 and r.used[4] == 14  # no pivot: the pose is the linear one
    assert r.updates.tolist() == [0, 0, 0, 0, 0, 1, 1] and r.inliers[5] == 40 and r.inliers[6] >= 10
    assert (r.poses[5:] != r.linear_poses[5:]).any(axis=1).all()
    assert r.rms_after[:5].tolist() == [0] * 5 and (r.rms_after[5:] > 0).all()
    census = set()
    for name in LC.cases():
        census |= set(LC.host(name).status.tolist())
    assert census == set(range(7))


def test_row_counts():
    r, r6 = LC.host("rows_family"), LC.host("rows_family_6")
    assert r.rows.tolist() == r.eligible.tolist() == list(LC.ROW_COUNTS) == r6.eligible.tolist()
    assert r.status.tolist() == [2 if n < 10 else 0 for n in LC.ROW_COUNTS]
    assert r6.status.tolist() == [2 if n < 6 else 0 for n in LC.ROW_COUNTS]
    assert r.inliers[5:].tolist() == list(LC.ROW_COUNTS[5:]) == r.used[5:].tolist()  # clean pixels: every row an inlier
    assert r6.poses[5:].tobytes() == r.poses[5:].tobytes()  # min_inliers does not enter a frame's estimate


def test_hypothesis_counts():
    """clean pixels: the first hypothesis already has every row, so every K gives the same frames"""
    first = LC.host("iters_1")
    assert (first.status == 0).all() and (first.best == 0).all()
    for k in LC.ITERS[1:]:
        LC.assert_same(LC.host("iters_%d" % k), first, k)
    # with outliers the winner comes later, and fewer hypotheses find a worse or no winner
    c = LC.cases()["outliers"]
    a, kw = c.args()
    few = pkg("visomatch").host_locate(*a, **{**kw, "params": dict(ransac_iters=2)})
    full = LC.host("outliers")
    assert (full.best > 1).any() and (few.best <= 1).all() and (few.inliers <= full.inliers).all() and (few.inliers < full.inliers).any()


def test_shapes():
    for n in (1, 2, 9):
        r = LC.host("frames_%d" % n)
        assert len(r) == n and (r.status == 0).all() and (r.inliers == 30).all()
    r = LC.host("frames_257")
    assert len(r) == 257 and (r.status == 0).all() and r.rows.tolist() == [10 + g % 3 for g in range(257)]
    r = LC.host("no_tracks")
    assert r.status.tolist() == [2, 2, 2] and (r.poses == 0).all()
    assert len(LC.host("no_frames")) == 0


def test_hard_inputs(vm):
    r = LC.host("nan")
    assert r.rows.tolist() == [50] * 3 and r.eligible.tolist() == [46, 46, 44] == r.inliers.tolist() and (r.status == 0).all()
    assert np.isfinite(r.poses).all() and np.isfinite(r.ss_after).all()
    r = LC.host("unused")
    assert r.rows.tolist() == [48] * 3 == r.eligible.tolist() and (r.status == 0).all() and np.isfinite(r.poses).all()
    r = LC.host("behind")
    assert r.eligible.tolist() == [90] * 3 and r.inliers.tolist() == [60] * 3 == r.used.tolist() and (r.status == 0).all()
    assert (r.best > 0).all()  # the first hypotheses sample a point behind the camera and are invalid
    r = LC.host("duplicates")
    assert (r.status == 0).all() and r.inliers.tolist() == [30, 30]
    r = LC.host("identical")
    assert r.status.tolist() == [0, 4, 3] and r.eligible.tolist() == [30, 10, 12] and r.best[2] == -1 and r.inliers[1] < 10
    r = LC.host("huge")
    assert (r.status == 0).all() and r.eligible.tolist() == [40] * 3 and r.inliers.tolist() == [39] * 3 and np.isfinite(r.poses).all()
    r = LC.host("planar")  # the known limit
    assert set(r.status.tolist()) <= {3, 4} and (r.poses == 0).all()
    a, kw = LC.cases()["seed_0"].args()
    LC.assert_same(LC.host("seed_0"), vm.host_locate(*a, **{**kw, "params": dict(seed=1)}), "seed 0 is the engine's seed 1")
    LC.assert_same(LC.host("seed_0"), vm.host_locate(*a, **{**kw, "params": dict(seed=2147483647)}), "and so is 2^31 - 1")


@pytest.mark.parametrize("name", sorted(LC.cases()))
def test_refinement_bytes(vm, name):
    """poses = host_resect from linear_poses with the location's gate, byte for byte; zeros where there is no pose"""
    c, r = LC.cases()[name], LC.host(name)
    go = np.isin(r.status, (0, 5, 6))
    want = vm.host_resect(r.linear_poses, *c.tracks_args(), use=c.use, refine=go, pose_valid=go, params=resect_params(vm, c))
    assert r.poses[go].tobytes() == want.poses[go].tobytes() and (r.poses[~go] == 0).all()
    assert r.updates[go].tolist() == want.updates[go].tolist() and r.used[go].tolist() == want.used[go].tolist() and (r.updates[~go] == 0).all()
    assert r.ss_after[go].tobytes() == want.ss_after[go].tobytes() and r.rms_after[go].tobytes() == want.rms_after[go].tobytes()
    assert [{0: 0, 6: 6}.get(s, 5) for s in want.status[go].tolist()] == r.status[go].tolist()
    assert r.rows.tolist() == want.rows.tolist()


@pytest.mark.parametrize("name", sorted(LC.cases()))
def test_hypothesis_bytes(vm, name):
    """the winner's count = host_vet's inliers of the frame at the linear pose with the same gate"""
    c, r = LC.cases()[name], LC.host(name)
    won = r.best >= 0
    assert ((r.inliers > 0) == won).all() and (r.linear_poses[~won] == 0).all()
    if c.n_frames == 0:
        return
    v = vm.host_vet(r.linear_poses, *c.tracks_args(), use=c.use, pose_valid=won, params=vet_params(vm, c))
    assert v.frame_counts[won, 0].tolist() == r.inliers[won].tolist(), (name, v.frame_counts[:, 0].tolist(), r.inliers.tolist())
    p = vm.locate_params(**c.params)
    assert ((r.inliers >= p.min_inliers) == np.isin(r.status, (0, 5, 6))).all()


def relabelled(c, order):
    """the case with frame g called order[g]"""
    order = np.asarray(order)
    d = LC.Case(c.n_frames, [], c.xyz, use=c.use, params=c.params, f=c.f, cu=c.cu, cv=c.cv)
    d.offsets, d.uv, d.obs_frames = c.offsets, c.uv, order[c.obs_frames].astype(np.int32)
    if c.locate is not None:
        d.locate = np.zeros(c.n_frames, np.uint8)
        d.locate[order] = c.locate
    return d


@pytest.mark.parametrize("name", ["outliers", "statuses", "rows_family", "mask"])
def test_determinism(vm, name):
    """a frame's result depends on its own rows alone: not on what the frame is called, not on the other frames in the call"""
    c, r = LC.cases()[name], LC.host(name)
    order = np.random.default_rng(7).permutation(c.n_frames)
    a, kw = relabelled(c, order).args()
    moved = vm.host_locate(*a, **kw)
    for n in LC.FIELDS:
        assert np.ascontiguousarray(getattr(moved, n)[order]).tobytes() == np.ascontiguousarray(getattr(r, n)).tobytes(), (name, n)
    asked = np.ones(c.n_frames, bool) if c.locate is None else c.locate.astype(bool)
    a, kw = c.args()
    for g in np.nonzero(asked)[0][:4]:
        # alone in the call: by the mask, and with the other frames' observations taken out of the tracks
        only = np.zeros(c.n_frames, np.uint8)
        only[g] = 1
        one = vm.host_locate(*a, **{**kw, "locate": only})
        keep = c.obs_frames == g
        off = np.cumsum([0] + [int(keep[a0:a1].sum()) for a0, a1 in zip(c.offsets[:-1], c.offsets[1:])]).astype(np.int32)
        cut = vm.host_locate(c.n_frames, c.f, c.cu, c.cv, off, c.obs_frames[keep], c.uv[keep], c.xyz, use=c.use, locate=only, params=c.params)
        for n in LC.FIELDS:
            assert getattr(one, n)[g].tobytes() == getattr(r, n)[g].tobytes() == getattr(cut, n)[g].tobytes(), (name, g, n)
        assert (np.delete(one.status, g) == 1).all()


def planted_outliers(vm, name):
    c, r = LC.cases()[name], LC.host(name)
    assert 0.25 < 1 - c.clean.mean() < 0.35
    assert (r.status == 0).all()
    v = vm.host_vet(r.poses, *c.tracks_args(), params=vet_params(vm, c))
    assert (v.code == 0).tolist() == c.clean.tolist()
    assert r.used.tolist() == np.bincount(c.obs_frames[c.clean], minlength=c.n_frames).tolist() == r.inliers.tolist()
    return r


def test_planted_outliers(vm):
    """30 % of the pixels displaced by 50 px and more: every frame is located, and the inliers at the located poses are exactly
    the clean observations"""
    planted_outliers(vm, "outliers")


def test_planted_outliers_across_tiles(vm):
    """the same on frames of 255, 257 and 513 rows with 33 hypotheses: the winner is not the first hypothesis, so what the
    hypotheses behind it hold and count decides the result, on either side of the count kernel's tile and in its third"""
    r = planted_outliers(vm, "outliers_tiles")
    assert r.rows.tolist() == list(LC.TILE_ROWS) and (r.best > 0).any()
    print("outliers_tiles: best", r.best.tolist(), "inliers", r.inliers.tolist())


def test_pose_against_truth(vm):
    """the located pose against host_resect started at the true pose on the same rows with the same gate"""
    worst = 0.0
    for name in WITH_TRUTH:
        c, r = LC.cases()[name], LC.host(name)
        if name in ("statuses", "planar"):  # (statuses stops after one update at eps = 1e-3; planar locates nothing)
            continue
        ok = r.status == 0
        assert ok.any(), name
        ref = vm.host_resect(c.true_poses, *c.tracks_args(), use=c.use, refine=ok, params=resect_params(vm, c))
        assert (ref.status[ok] == 0).all() and ref.used[ok].tolist() == r.used[ok].tolist(), name
        d = float(np.abs(r.poses[ok] - ref.poses[ok]).max())
        print("%-14s %d frames, largest |located - resected from the truth| = %.3g" % (name, int(ok.sum()), d))
        worst = max(worst, d)
    print("largest over the suite: %.3g (bound %.3g)" % (worst, 10 * MEASURED_POSE_DIFFERENCE))
    assert worst <= 10 * MEASURED_POSE_DIFFERENCE
