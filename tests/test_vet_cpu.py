"""CPU suite: vsm_host_vet - the vetting's host view, one thread walking csrc/vsm_vet.h - against tests/vet_ref.py, the
definition restated in plain Python floats: every array equal by its bytes (NaN positions equal), on all cases of
tests/vet_cases.py.  Then what the cases are for is checked on the restatement's own result, so that a case that no longer
reaches its code, its status or its length fails here and not silently; the planted scene prunes to the clean one; the inliers of
a frame are the rows the resection uses at the same poses; counts, stats and the pruned set are consistent with the codes."""
import ctypes as C

import numpy as np
import pytest

import vet_cases as VC
import vet_ref as V
from conftest import pkg


@pytest.fixture(scope="module")
def vm():
    m = pkg("visomatch")
    m.lib()
    return m


@pytest.mark.parametrize("name", sorted(VC.cases()))
def test_host_view_equals_the_restatement(vm, name):
    a, kw = VC.cases()[name].args()
    got = vm.host_vet(*a, **kw)
    V.assert_same(got, VC.reference(name), name)
    want = VC.reference(name)
    assert [got.stats[k] for k in vm.VET_STATS] == np.bincount(want.code, minlength=5).tolist() + np.bincount(want.status, minlength=4).tolist()


def test_lengths_family():
    c, want = VC.cases()["lengths"], VC.reference("lengths")
    assert np.diff(c.offsets).tolist() == list(VC.LENGTHS)
    # every seventh observation is planted 50 px off, the others are within 0.7 px of the truth
    assert want.n_in.tolist() == [n - n // 7 for n in VC.LENGTHS]
    assert want.status.tolist() == [2, 2] + [0] * 10 and set(np.unique(want.code).tolist()) == {0, 4}
    assert (want.ss[2:] > 0).all() and (want.worst[2:] < 2 * 0.75 ** 2).all()
    assert want.frame_lo.tolist() == [-1] + [0] * 11 and want.frame_hi.tolist() == [-1, 0, 1] + [5] * 9


def test_count_family():
    for n in VC.COUNTS:
        want = VC.reference("counts_%d" % n)
        assert len(want.status) == n and (want.n_in > 0).all()


def test_every_code_and_status_in_one_call():
    c, want = VC.cases()["codes"], VC.reference("codes")
    assert set(want.code.tolist()) == {0, 1, 2, 3, 4}
    assert want.status.tolist() == [0, 0, 0, 0, 1, 2, 2, 3, 0]
    # the observation on the gate: ru^2 + rv^2 == max_residual^2 exactly, and that is not below it
    i = int(c.offsets[VC.ON_THE_GATE])
    assert want.code[i] == 4 and want.r2[i] == np.float32(4.0) and V.DEFAULTS["max_residual"] ** 2 == 4.0
    assert want.n_in[VC.ON_THE_GATE] == 3 and want.status[VC.ON_THE_GATE] == 0
    assert want.n_in[5] == c.params["min_observations"] - 1 and want.code[c.offsets[5]:c.offsets[6]].tolist() == [0, 0, 2]
    assert want.code[c.offsets[6]:c.offsets[7]].tolist() == [3, 3, 3] and (want.r2[c.offsets[6]:c.offsets[7]] == 0).all()
    assert want.n_in[7] == 3 and want.frame_lo[7] == want.frame_hi[7] == 1  # a triple row: three inliers, one view
    assert want.n_in[8] == 5 and (want.frame_lo[8], want.frame_hi[8]) == (0, 4)
    assert (want.code[c.offsets[4]:c.offsets[5]] == 1).all() and want.n_in[4] == 0 and want.ss[4] == 0 and want.worst[4] == 0


def test_nan_and_infinite_inputs():
    c, want = VC.cases()["nan"], VC.reference("nan")
    for i in (5, 17, 40):
        assert want.code[i] == 4 and np.isnan(want.r2[i])
    for i in (77, 90):
        assert want.code[i] == 4 and np.isinf(want.r2[i])
    assert (want.code[c.offsets[7]:c.offsets[8]] == 3).all()  # the NaN point: its depth is NaN
    assert np.isfinite(want.ss).all() and np.isfinite(want.worst).all()
    assert np.isnan(want.r2).sum() == 3 and np.isinf(want.r2).sum() == 2


def test_masks_gate_and_depth():
    c, want = VC.cases()["masks"], VC.reference("masks")
    per_obs = np.repeat(np.arange(len(c.xyz)), np.diff(c.offsets))
    assert (want.code[c.use[per_obs] == 0] == 1).all() and (want.status[::5] == 1).all()
    rest = c.use[per_obs] == 1
    assert (want.code[rest & np.isin(c.obs_frames, (2, 3))] == 2).all() and (want.frame_counts[2:4] == 0).all()
    assert set(want.code[rest & ~np.isin(c.obs_frames, (2, 3))].tolist()) == {0, 4}
    gated, open_ = VC.reference("min_depth_9"), VC.reference("no_gate")
    assert (open_.code == 0).all() and (open_.worst.max() > 50 * 50)  # no gate: the planted pixels are inliers
    assert set(gated.code.tolist()) == {0, 3, 4} and (gated.frame_counts[:, 1] > 0).all()


def test_empty_inputs(vm):
    for name in ("no_tracks", "no_frames"):
        a, kw = VC.cases()[name].args()
        got = vm.host_vet(*a, **kw)
        assert len(got) == 0 and got.kept_offsets.tolist() == [0] and len(got.kept_index) == 0 and len(got.code) == 0
    assert vm.host_vet(*VC.cases()["no_tracks"].args()[0]).frame_counts.tolist() == [[0, 0, 0]] * 3


def test_the_planted_scene_prunes_to_the_clean_one(vm):
    planted, clean = VC.planted_case()
    want = VC.reference("planted")
    # the margins, from the restatement's r2: clean pixels below (1e-3 px)^2, planted ones beyond (20 px)^2, the gate at 2^2
    assert want.r2[want.code == 0].max() < 1e-6 and want.r2[want.code == 4].min() > 400.0 and set(want.code.tolist()) == {0, 4}
    assert (want.code == 4).sum() == len(planted.uv) - len(clean.uv) > 30
    assert (want.status[planted.is_planted] == 2).all() and (want.status[~planted.is_planted] == 0).all() and planted.is_planted.sum() == 12
    for res in (want, vm.host_vet(*planted.args()[0])):
        v = vm.Vetting(*[getattr(res, k) for k in V.FIELDS])
        off, fr, uv = v.prune(planted.obs_frames, planted.uv)
        assert off.dtype == np.int32 and fr.dtype == np.int32 and uv.dtype == np.float32
        assert off.tobytes() == clean.offsets.tobytes() and fr.tobytes() == clean.obs_frames.tobytes() and uv.tobytes() == clean.uv.tobytes()


@pytest.mark.parametrize("name", ["lengths", "codes", "masks", "min_depth_9", "no_gate", "planted", "nan"])
def test_inliers_are_the_rows_the_resection_uses(vm, name):
    """with the same max_residual, min_depth and poses: where vsm_host_resect reaches an evaluation (status 0, 4, 5, 6), the
    frame's inlier count is the count of rows used at the input pose.  host_resect returns that count through rms_before =
    sqrt(ss_before / count) (and, where it stops before the first update, as `used` itself)."""
    c = VC.cases()[name]
    prm = dict(V.DEFAULTS, **c.params)
    got = vm.host_vet(*c.args()[0], **c.args()[1])
    rs = vm.host_resect(c.poses, c.f, c.cu, c.cv, c.offsets, c.obs_frames, c.uv, c.xyz, use=c.use, pose_valid=c.pose_valid,
                        params=dict(max_residual=prm["max_residual"], min_depth=prm["min_depth"], min_observations=6))
    checked = 0
    for g in range(len(c.poses)):
        if rs.status[g] not in (0, 4, 5, 6):
            continue
        if rs.updates[g] == 0:
            count = int(rs.used[g])
        else:
            assert rs.rms_before[g] > 0
            ratio = rs.ss_before[g] / rs.rms_before[g] ** 2
            count = int(round(ratio))
            assert abs(ratio - count) < 1e-6 * count
        assert got.frame_counts[g, 0] == count, (name, g, got.frame_counts[g].tolist(), count, int(rs.status[g]))
        checked += 1
    assert checked >= 2, (name, rs.status.tolist())


@pytest.mark.parametrize("name", sorted(VC.cases()))
def test_counts_and_the_pruned_set_are_consistent(vm, name):
    c = VC.cases()[name]
    a, kw = c.args()
    got = vm.host_vet(*a, **kw)
    assert got.frame_counts.sum(axis=0).tolist() == [got.stats["obs_inlier"], got.stats["obs_behind"], got.stats["obs_gated"]]
    assert sum(got.stats[k] for k in vm.VET_STATS[:5]) == len(c.uv) and sum(got.stats[k] for k in vm.VET_STATS[5:]) == len(c.xyz)
    for g in range(len(c.poses)):
        assert got.frame_counts[g].tolist() == [int(((c.obs_frames == g) & (got.code == k)).sum()) for k in (0, 3, 4)]
    per_obs = np.repeat(np.arange(len(c.xyz)), np.diff(c.offsets))
    keep = (got.code == 0) & (got.status[per_obs] == 0) if len(per_obs) else np.zeros(0, bool)
    assert got.kept_index.tolist() == np.nonzero(keep)[0].tolist()
    assert np.diff(got.kept_offsets).tolist() == np.where(got.status == 0, got.n_in, 0).tolist() and got.kept_offsets[0] == 0
    assert got.n_in.tolist() == np.bincount(per_obs[got.code == 0], minlength=len(c.xyz)).tolist()
    assert (got.kept == (got.status == 0)).all() and (got.inlier == (got.code == 0)).all()


def test_argument_errors_leave_the_outputs_untouched(vm):
    c = VC.cases()["counts_5"]
    (poses, f, cu, cv, off, fr, uv, xyz), kw = c.args()
    bad_fr = fr.copy()
    bad_fr[3] = len(poses)
    dec = off.copy()
    dec[3] = dec[2] - 1
    shifted = off.copy()
    shifted[0] = 1
    nan = float("nan")
    for args, over in (((poses, f, cu, cv, off, bad_fr, uv, xyz), {}), ((poses, f, cu, cv, dec, fr, uv, xyz), {}), ((poses, f, cu, cv, shifted, fr, uv, xyz), {}),
                       ((poses, f, cu, cv, off, fr, uv, xyz), {"n_tracks": -2}), ((poses, f, cu, cv, off, fr, uv, None), {}),
                       ((poses, f, cu, cv, off, fr, uv, xyz), {"params": vm._NO_PARAMS}), ((poses, f, cu, cv, off, fr, uv, xyz), {"params": dict(min_observations=0)}),
                       ((poses, f, cu, cv, off, fr, uv, xyz), {"params": dict(max_residual=-1.0)}), ((poses, f, cu, cv, off, fr, uv, xyz), {"params": dict(max_residual=nan)}),
                       ((poses, f, cu, cv, off, fr, uv, xyz), {"params": dict(min_depth=nan)})):
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            vm.host_vet(*args, **{**kw, **over})
    # through the library itself: every output holds a pattern before the call and after it
    L = vm.lib()
    T, n = len(off) - 1, len(fr)
    outs = [np.full(n, 0xA5, np.uint8), np.full(n, 7.5, np.float32)] + [np.full(T, -77, np.int32) for _ in range(4)] + [np.full(T, 7.5), np.full(T, 7.5)] + \
           [np.full((len(poses), 3), -77, np.int32), np.full(T + 1, -77, np.int32), np.full(n, -77, np.int32)]
    before = [o.copy() for o in outs]
    n_kept = C.c_int32(-77)
    for p in (vm.vet_params(min_observations=0), vm.vet_params(max_residual=-0.5), vm.vet_params(max_residual=nan), vm.vet_params(min_depth=nan), None):
        rc = L.vsm_host_vet(len(poses), vm._ptr(poses), None, f, cu, cv, T, vm._ptr(off), vm._ptr(fr), vm._ptr(uv), vm._ptr(xyz), None, None if p is None else C.byref(p),
                            *[vm._ptr(o) for o in outs], C.byref(n_kept))
        assert rc == -4
    rc = L.vsm_host_vet(len(poses), vm._ptr(poses), None, f, cu, cv, T, vm._ptr(off), vm._ptr(bad_fr), vm._ptr(uv), vm._ptr(xyz), None, C.byref(vm.vet_params()),
                        *[vm._ptr(o) for o in outs], C.byref(n_kept))
    assert rc == -4 and n_kept.value == -77 and all(a.tobytes() == b.tobytes() for a, b in zip(outs, before))
    # the smallest legal values pass; every output may be NULL
    assert L.vsm_host_vet(len(poses), vm._ptr(poses), None, f, cu, cv, T, vm._ptr(off), vm._ptr(fr), vm._ptr(uv), vm._ptr(xyz), None,
                          C.byref(vm.vet_params(min_observations=1, max_residual=0.0, min_depth=-1e300)), *[None] * 12) == T


def test_interface(vm):
    L = vm.lib()
    p = vm.vet_params()
    assert C.sizeof(vm.VsmVetParams) == 24
    assert (p.max_residual, p.min_depth, p.min_observations) == (2.0, 1e-10, 2) == tuple(V.DEFAULTS[k] for k in ("max_residual", "min_depth", "min_observations"))
    names = [L.vsm_kernel_name(i).decode() for i in range(L.vsm_num_kernels())]
    assert all(names) and names.count("k_vet_obs") == 1 and names.count("k_vet_emit") == 1
    assert len(vm.VET_CODES) == 5 and len(vm.VET_STATUS) == 4 and len(vm.VET_STATS) == 9 and len(vm.VET_TIMINGS) == 4
    for s in ("vsm_vet_default_params", "vsm_vet_run", "vsm_points_vet", "vsm_vet_count", "vsm_vet_get_obs", "vsm_vet_get_tracks", "vsm_vet_get_frames",
              "vsm_vet_get_kept", "vsm_vet_get_stats", "vsm_vet_get_timings", "vsm_host_vet", "vsm_tracks_pixels"):
        assert s in vm.EXPORTS and hasattr(L, s), s
    assert all(hasattr(vm.Matcher, m) for m in ("vet", "vet_points", "track_pixels")) and hasattr(vm.Vetting, "prune")
