"""CPU suite: the refinement's host pieces and the inputs of tests/test_refine_gpu.py (tests/refine_cases.py).

  * vsm_host_parabolic_update (the per-frame path's fit under stage capture) against the oracle's vo_parabolic_update on every
    cost record, outputs and verdicts byte for byte;
  * the oracle's vo_refine against the reference's own Matcher::refinement on every injected list (where oracle/_ref is built),
    and against the refinement inside the oracle's matchFeatures;
  * the entry points' argument checks (host arithmetic: the same function guards the GPU entry);
  * censuses - conditions on the INPUTS, not on the code under test: every class of cost record has at least 100 members, and
    the injected lists reach every exit of relocateMinimum and parabolicFitting under both half_resolution values.

Census of the injected lists (seven families, both sizes, methods 0, 1, 2, every list of refine_cases.lists_of), as the oracle
counts it - the same for half_resolution = 1 and 0, which only decides whether the tiled or the row-major planes are read:
  relocation  114030 calls: 29519 margin exits, 84511 relocations, 24522 of them with a tied minimum
  fit         76426 calls: 28632 margin exits, 26329 minima on the window's border, 386 |divisor| < 1e-8, 69 |b2| < 1e-8,
              907 |ddu| or |ddv| >= 1, 20103 successes (7084 of them with a non-zero minimum cost), 16246 windows with a
              tied minimum; the singular-system exit of Matrix::solve cannot be taken (At A is a constant)
Per family and method-2 pass the 3258 matches of the lists put 7216 targets inside the 5 x 5 window's margin, 762 to 1208 on
each of the eight residues of (iu - 4) & 7 (2196 of them at x.5), and 776 to 902 reference points on each residue of
(ru - 2) & 3.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import refine_cases as RC
from conftest import ROOT, pkg


@pytest.fixture(scope="module")
def vm():
    m = pkg("visomatch")
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "opencl-structure-from-motion_amd", "csrc")])
    m.lib()
    return m


@pytest.fixture(scope="module")
def record_sets():
    return RC.record_sets()


# ---- cost records ---------------------------------------------------------------------------------------------------------

def test_record_classes(B, record_sets):
    """every class of the exhaustive set has at least 100 members, and the oracle's own exits count the same records"""
    r = record_sets["exhaustive"]
    assert len(r) == 19683
    cls = RC.classify(r)
    counts = np.bincount(cls, minlength=len(RC.CLASSES))
    print(dict(zip(RC.CLASSES, counts.tolist())))
    assert counts.min() >= 100, counts
    B.oracle_refine_census()
    uv, ok = B.oracle_parabolic_fits(r, RC.start_points(len(r)))
    cen = B.oracle_refine_census()
    assert np.array_equal(ok == 1, cls == 0)
    assert (cen["fit_ok"], cen["fit_divisor"], cen["fit_b2"], cen["fit_range"], cen["fit_singular"]) == \
        (counts[0], counts[1], counts[2], counts[3] + counts[4], 0), (cen, counts)


@pytest.mark.parametrize("name", ["exhaustive", "uniform", "scaled255", "scaled510"])
def test_host_fit_vs_oracle(vm, B, record_sets, name):
    r = record_sets[name]
    start = RC.start_points(len(r))
    want_uv, want_ok = B.oracle_parabolic_fits(r, start)
    got_uv, got_ok = vm.host_parabolic_fits(r, start)
    assert np.array_equal(got_ok, want_ok), np.flatnonzero(got_ok != want_ok)[:8]
    assert got_uv.tobytes() == want_uv.tobytes(), np.flatnonzero((got_uv != want_uv).any(axis=1))[:8]
    assert np.array_equal(got_uv[want_ok == 0], start[want_ok == 0])        # a failed fit leaves the target alone
    assert 0 < want_ok.sum() < len(r)
    if name != "exhaustive":
        assert r[:, 3:].max() > 255       # costs beyond one byte


def test_scaled_records_keep_their_ties(record_sets):
    base = RC.exhaustive_records()
    for k in (255, 510):
        r = record_sets[f"scaled{k}"]
        assert len(r) == 2000 and np.array_equal(r[:, 3:] // k, base[np.arange(2000) * 9 + np.arange(2000) % 9][:, 3:])
    assert record_sets["uniform"][:, 3:].max() == 4080 and record_sets["uniform"][:, 3:].min() == 0


# ---- lists for k_parabolic_apply ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pools(B, record_sets):
    r = np.concatenate([record_sets["exhaustive"], record_sets["uniform"][:4000], record_sets["scaled510"]])
    _, ok = B.oracle_parabolic_fits(r, RC.start_points(len(r)))
    return r[ok == 1], r[ok == 0]


@pytest.mark.parametrize("n", RC.APPLY_NS)
def test_apply_cases_keep_what_they_say(B, pools, n):
    """a condition on the inputs: the oracle's fits keep exactly the pattern's matches, in order; dropped matches fail in
    every step, by status word and by fit, with steps behind the failed one that would succeed"""
    good, bad = pools
    run = max((n + 1023) // 1024, 1)
    pats = RC.keep_patterns(n)
    assert set(pats) >= {"all", "none", "alternating", "only_first", "only_last", "runs", "runs+1"} and ("runs-1" in pats) == (run > 1)
    for name, keep in pats.items():
        m, rec = RC.apply_case(n, keep, good, bad, seed=len(name))
        want = RC.apply_expected(m, rec, B.oracle_parabolic_fits)
        assert np.array_equal(want["i1c"], m["i1c"][keep]), (n, name)
        if n >= 1023 and name in ("alternating", "runs+1"):
            drop = ~keep
            for st in range(3):
                assert np.count_nonzero(drop & (rec[:, st, 0] == 0)) and np.count_nonzero(drop & (rec[:, st, 0] == 1))
            assert np.count_nonzero(drop & (rec[:, 0, 0] == 0) & (rec[:, 1, 0] == 1) & (rec[:, 2, 0] == 1))
            assert np.count_nonzero(keep & (rec[:, :, 0] == 2).all(axis=1)) and np.count_nonzero(keep & (rec[:, :, 0] == 1).all(axis=1))
            changed = want[["u1p", "v1p", "u2c", "v2c", "u2p", "v2p"]] != m[keep][["u1p", "v1p", "u2c", "v2c", "u2p", "v2p"]]
            assert np.count_nonzero(changed) > len(want) // 2
    if run > 1:   # the runs' ends fall on every place of a thread's ownership range
        ends = np.flatnonzero(np.diff(pats["runs"].astype(np.int8)) != 0) + 1
        assert set((ends % run).tolist()) == set(range(run)) or n < 4 * run * run


# ---- argument checks --------------------------------------------------------------------------------------------------------

def _one(w, h, **kw):
    m = RC.master_list(0)[8:9].copy()
    for k, v in kw.items():
        m[k] = v
    return m


def test_refine_check(vm):
    w, h = RC.SIZES[0]
    EARG = vm.Matcher.EARG
    assert vm.refine_check(w, h, [RC.master_list(0)]) == 0
    assert vm.refine_check(w, h, [RC.master_list(0)[:7], RC.master_list(0)[:0]]) == 0
    for f in ("u1p", "v1p", "u2p", "v2p", "u1c", "v1c", "u2c", "v2c"):
        for bad in (np.nan, np.inf, -np.inf):
            assert vm.refine_check(w, h, [_one(w, h, **{f: bad})]) == EARG, (f, bad)
    for f, hi in (("u1c", w - 1 - RC.MARGIN), ("v1c", h - 1 - RC.MARGIN)):
        assert vm.refine_check(w, h, [_one(w, h, **{f: RC.MARGIN})]) == 0 and vm.refine_check(w, h, [_one(w, h, **{f: hi})]) == 0
        for bad in (RC.MARGIN - 1, hi + 1, -3, 1e9, 20.5, np.nextafter(np.float32(20), np.float32(21)), np.nextafter(np.float32(RC.MARGIN), np.float32(0))):
            assert vm.refine_check(w, h, [_one(w, h, **{f: bad})]) == EARG, (f, bad)
    for f in ("u1p", "v1p", "u2p", "v2p", "u2c", "v2c"):      # targets: any finite float
        for fine in (-1e30, 3e38, 20.5, -0.0):
            assert vm.refine_check(w, h, [_one(w, h, **{f: fine})]) == 0, (f, fine)
    big = np.zeros(RC.PARA_MAX_LIST + 1, dtype=RC.MATCH)
    big["u1c"] = big["v1c"] = 20
    assert vm.refine_check(w, h, [big[:-1]]) == 0 and vm.refine_check(w, h, [big]) == EARG
    assert vm.refine_check(w, h, [big[:3]], counts=[-1]) == EARG
    assert vm.refine_check(w, h, [big[:1]] * 64) == 0 and vm.refine_check(w, h, [big[:1]] * 65) == EARG
    assert vm.refine_check(w, h, []) == EARG
    assert vm.refine_check(12, 12, [big[:0]]) == EARG      # no pixel inside the margin
    last = RC.master_list(0)[:100].copy()                   # the check reads every match of every list
    last["u1c"][99] = 5
    assert vm.refine_check(w, h, [RC.master_list(0)[:5], last]) == EARG


def test_entries_reject_before_touching_the_gpu(vm):
    """VSM_EARG without a HIP call: these run where there is no GPU"""
    L, EARG = vm.lib(), vm.Matcher.EARG
    big = np.zeros(RC.PARA_MAX_LIST + 1, dtype=RC.MATCH)
    rec = np.zeros((RC.PARA_MAX_LIST + 1, 3, 12), dtype=np.int32)
    one = (C.c_void_p * 1)
    out, oc = np.zeros(len(big), dtype=RC.MATCH), np.zeros(1, dtype=np.int32)
    args = lambda n: (one(big.ctypes.data), one(rec.ctypes.data), np.array([n], dtype=np.int32).ctypes.data_as(C.c_void_p), 1, one(out.ctypes.data),
                      oc.ctypes.data_as(C.c_void_p))
    assert L.vsm_debug_parabolic_apply(*args(RC.PARA_MAX_LIST + 1)) == EARG
    assert L.vsm_debug_parabolic_apply(*args(-1)) == EARG
    a = args(5)
    assert L.vsm_debug_parabolic_apply(a[0], a[1], a[2], 0, a[4], a[5]) == EARG and L.vsm_debug_parabolic_apply(a[0], a[1], a[2], 65, a[4], a[5]) == EARG
    assert L.vsm_debug_parabolic_apply(a[0], None, a[2], 1, a[4], a[5]) == EARG
    assert L.vsm_debug_refine(None, 2, a[0], a[2], 1, a[4], a[5]) == EARG
    assert L.vsm_host_parabolic_fits(None, 3, None, None) == EARG and L.vsm_host_parabolic_fits(None, 0, None, None) == 0


# ---- injected match lists over images ---------------------------------------------------------------------------------------

CASES = [(fam, size, half) for fam in RC.FAMILIES for size in range(len(RC.SIZES)) for half in (1, 0)]
_REFINED = {}


def oracle_refined(B, fam, size, half):
    """{(refinement, method, list name): [refined list per pair]} from vo_refine, and the census of each refinement"""
    key = (fam, size, half)
    if key not in _REFINED:
        out, cen = {}, {}
        for refinement in (1, 2):
            c = B.CpuMatcher("oracle", half_resolution=half, refinement=refinement)
            RC.push_all(c, fam, size)
            B.oracle_refine_census()
            for method in (0, 1, 2):
                for name, lists in RC.lists_of(size):
                    out[refinement, method, name] = [c.refine(m, method) for m in lists]
            cen[refinement] = B.oracle_refine_census()
            c.close()
        _REFINED[key] = (out, cen)
    return _REFINED[key]


def test_master_list_covers_the_residues():
    for size, (w, h) in enumerate(RC.SIZES):
        m = RC.master_list(size)
        assert vm_check_ok(m, w, h)
        assert set(m["u1c"].astype(int).tolist()) == set(range(RC.MARGIN, w - RC.MARGIN)) and set(m["v1c"].astype(int).tolist()) == set(range(RC.MARGIN, h - RC.MARGIN))
        for fu, fv in RC.STEP_FIELDS:
            ok = (m[fu] - 2 >= RC.MARGIN) & (m[fu] + 2 <= w - 1 - RC.MARGIN) & (m[fv] - 2 >= RC.MARGIN) & (m[fv] + 2 <= h - 1 - RC.MARGIN)
            iu, ru = m[fu][ok].astype(int), m["u1c"][ok].astype(int)
            assert set(((iu - 4) & 7).tolist()) == set(range(8)) and set(((ru - 2) & 3).tolist()) == set(range(4))
            assert set(((iu - 4) & 7)[m[fu][ok] != iu].tolist()) == set(range(8))      # ... at x.5 too
            for x, length in ((m[fu], w), (m[fv], h)):
                for r in (2, 3):
                    for edge in (RC.MARGIN + r, length - 1 - RC.MARGIN - r):
                        for v in RC._neighbours(edge):
                            assert np.count_nonzero(x == np.float32(v)), (fu, length, v)
                assert np.count_nonzero(x < 0) and np.count_nonzero(x > 1e6) and np.count_nonzero(x != np.floor(x))
        assert sum(len(l) for _, ls in RC.lists_of(size) for l in ls) == sum(RC.COUNTS) + sum(RC.BATCH)
        assert [len(l) for l in RC.lists_of(size)[-1][1]] == list(RC.BATCH)


def vm_check_ok(m, w, h):
    return bool(np.all((m["u1c"] >= RC.MARGIN) & (m["u1c"] <= w - 1 - RC.MARGIN) & (m["v1c"] >= RC.MARGIN) & (m["v1c"] <= h - 1 - RC.MARGIN) &
                       (m["u1c"] == np.floor(m["u1c"])) & (m["v1c"] == np.floor(m["v1c"]))))


@pytest.mark.parametrize("half", [1, 0])
def test_census_of_the_injected_lists(B, half):
    """every exit of relocateMinimum and parabolicFitting occurs, minima are tied, and fits with a non-zero minimum succeed"""
    total = {}
    for fam in RC.FAMILIES:
        for size in range(len(RC.SIZES)):
            _, cen = oracle_refined(B, fam, size, half)
            for refinement, c in cen.items():
                for k, v in c.items():
                    total[k] = total.get(k, 0) + v
    print(half, total)
    for k in ("reloc_margin", "reloc_moved", "reloc_tied", "fit_margin", "fit_border", "fit_divisor", "fit_b2", "fit_range", "fit_ok", "fit_tied",
              "fit_ok_nonzero"):
        assert total[k] > 0, (k, total)
    assert total["fit_singular"] == 0       # (At A is a constant: that exit of Matrix::solve cannot be taken)


def test_flat_frames_relocate_by_minus_two_and_drop_every_fit(B):
    """flat77: every cost is equal, the first of them wins: relocation moves by (-2, -2), the fit's minimum is on the border"""
    out, cen = oracle_refined(B, "flat77", 0, 1)
    (m,) = RC.lists_of(0)[6][1]
    (got,) = out[1, 2, "n256"]
    for fu, fv in RC.STEP_FIELDS:
        feasible = (m[fu] - 2 >= RC.MARGIN) & (m[fu] + 2 <= RC.SIZES[0][0] - 1 - RC.MARGIN) & (m[fv] - 2 >= RC.MARGIN) & (m[fv] + 2 <= RC.SIZES[0][1] - 1 - RC.MARGIN)
        assert 0 < feasible.sum() < len(m)
        assert np.array_equal(got[fu], np.where(feasible, m[fu] - 2, m[fu])) and np.array_equal(got[fv], np.where(feasible, m[fv] - 2, m[fv]))
    assert all(len(l) == 0 for l in out[2, 2, "n256"]) and cen[2]["fit_ok"] == 0 and cen[2]["fit_border"] > 0


def test_step_zero_infeasible_drops_the_match(B):
    out, _ = oracle_refined(B, "bytes", 0, 1)
    m = RC.lists_of(0)[-1][1][2]
    assert len(m) == 1 and m["u1p"][0] < 0
    assert len(out[2, 2, "batch"][2]) == 0 and len(out[2, 1, "batch"][2]) == 1       # quad: gone; stereo: step 0 is not run
    kept = out[1, 2, "batch"][2]                            # relocation: step 0 leaves its target alone, the others move theirs
    assert len(kept) == 1 and kept["u1p"][0] == m["u1p"][0] and kept["v1p"][0] == m["v1p"][0]
    assert (kept["u2c"][0], kept["v2c"][0], kept["u2p"][0], kept["v2p"][0]) == (60 - RC.DISPARITY, 40, 63 - RC.DISPARITY, 40)


@pytest.mark.parametrize("fam,size,half", CASES)
def test_oracle_refine_vs_reference(B, have_ref, fam, size, half):
    if not have_ref:
        pytest.skip("oracle/_ref/libvisoref.so not built")
    if not B.have_ref_refine():
        pytest.skip("oracle/_ref/libvisoref.so was built before ref_matcher_refine and not rebuilt since")
    out, _ = oracle_refined(B, fam, size, half)
    for refinement in (1, 2):
        r = B.CpuMatcher("ref", half_resolution=half, refinement=refinement)
        RC.push_all(r, fam, size)
        for method in (0, 1, 2):
            for name, lists in RC.lists_of(size):
                for k, m in enumerate(lists):
                    got, want = out[refinement, method, name][k], r.refine(m, method)
                    assert got.shape == want.shape and got.tobytes() == want.tobytes(), (refinement, method, name, k, len(got), len(want))
        r.close()


@pytest.mark.parametrize("refinement", [1, 2])
def test_vo_refine_is_the_refinement_of_match_features(B, refinement):
    """vo_refine on the pass-2 list gives the list matchFeatures hands to the final removeOutliers"""
    c = B.CpuMatcher("oracle", refinement=refinement)
    RC.push_all(c, "synth", 1)
    for method in (0, 1, 2):
        assert c.match(method)
        s2, s3 = c.stage(2), c.stage(3)
        assert len(s2) > 100 and c.refine(s2, method).tobytes() == s3.tobytes(), method
    c.close()
