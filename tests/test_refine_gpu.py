"""GPU suite (run with -m gpu on an MI355X): the refinement kernels of csrc/vsm_match.hip alone, on the inputs of
tests/refine_cases.py (what they reach is counted in tests/test_refine_cpu.py).

  * k_parabolic_apply through vsm_debug_parabolic_apply, on caller-given lists and cost records, against the oracle's fit
    (vo_parabolic_update) and plain compaction: every cost record of the four sets, and the list lengths and keep patterns
    around the kernel's ownership ranges;
  * k_refine<true> / k_refine<false> / k_parabolic_costs + k_parabolic_apply through vsm_debug_refine, on match lists built
    over seven image families, against the oracle's vo_refine.

Every comparison is of bytes: the survivors' 48-byte records, their order, their number."""
import numpy as np
import pytest

import refine_cases as RC
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vm():
    m = pkg("visomatch")
    m.lib()  # raises if the HIP library is missing: no silent fallback
    return m


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- k_parabolic_apply ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def record_sets():
    return RC.record_sets()


@pytest.fixture(scope="module")
def pools(B, record_sets):
    r = np.concatenate([record_sets["exhaustive"], record_sets["uniform"][:4000], record_sets["scaled510"]])
    _, ok = B.oracle_parabolic_fits(r, RC.start_points(len(r)))
    return r[ok == 1], r[ok == 0]


@pytest.mark.parametrize("name", ["exhaustive", "uniform", "scaled255", "scaled510"])
def test_apply_fits_every_record(vm, B, record_sets, name):
    """one record per match, in each of the three step slots in turn (the other two: status 2), lists of up to 16384"""
    r = record_sets[name]
    start = RC.start_points(len(r))
    want_uv, want_ok = B.oracle_parabolic_fits(r, start)
    for st, (fu, fv) in enumerate(RC.STEP_FIELDS):
        lists, recs, wants = [], [], []
        for a in range(0, len(r), RC.PARA_MAX_LIST):
            b = min(a + RC.PARA_MAX_LIST, len(r))
            m = np.zeros(b - a, dtype=RC.MATCH)
            for k, f in enumerate(("u1p", "v1p", "u2p", "v2p", "u1c", "v1c", "u2c", "v2c")):
                m[f] = 1000 + k
            m[fu], m[fv] = start[a:b, 0], start[a:b, 1]
            m["i1c"] = np.arange(a, b)
            rec = np.zeros((b - a, 3, 12), dtype=np.int32)
            rec[:, :, 0] = 2
            rec[:, st] = r[a:b]
            w = m.copy()
            w[fu], w[fv] = want_uv[a:b, 0], want_uv[a:b, 1]
            lists.append(m), recs.append(rec), wants.append(w[want_ok[a:b] == 1])
        got = vm.device_parabolic_apply(lists, recs)
        for k, (g, w) in enumerate(zip(got, wants)):
            assert len(g) == len(w), (name, st, k, len(g), len(w))
            assert same(g, w), (name, st, k, np.flatnonzero(g != w)[:8])


@pytest.mark.parametrize("n", RC.APPLY_NS)
def test_apply_lengths_and_keep_patterns(vm, B, pools, n):
    """every keep pattern of a length as the pairs of one launch"""
    good, bad = pools
    pats = RC.keep_patterns(n)
    cases = [RC.apply_case(n, keep, good, bad, seed=len(name)) for name, keep in pats.items()]
    got = vm.device_parabolic_apply([m for m, _ in cases], [rec for _, rec in cases])
    for name, (m, rec), g in zip(pats, cases, got):
        want = RC.apply_expected(m, rec, B.oracle_parabolic_fits)
        assert len(want) == int(pats[name].sum())
        assert len(g) == len(want), (n, name, len(g), len(want))
        assert same(g, want), (n, name, np.flatnonzero(g != want)[:8])


def test_apply_pairs_of_different_lengths(vm, B, pools):
    good, bad = pools
    cases = [RC.apply_case(n, RC.keep_patterns(n)["alternating" if n else "all"], good, bad, seed=n) for n in (1025, 0, 7)]
    got = vm.device_parabolic_apply([m for m, _ in cases], [rec for _, rec in cases])
    assert [len(g) for g in got] == [513, 0, 4]
    for (m, rec), g in zip(cases, got):
        assert same(g, RC.apply_expected(m, rec, B.oracle_parabolic_fits))


def test_apply_rejects_a_list_the_kernel_would_truncate(vm, B, pools):
    good, bad = pools
    n = RC.PARA_MAX_LIST + 1
    m, rec = RC.apply_case(n, np.ones(n, bool), good, bad)
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        vm.device_parabolic_apply([m], [rec])
    (g,) = vm.device_parabolic_apply([m[:-1]], [rec[:-1]])       # ... and works on afterwards
    assert same(g, RC.apply_expected(m[:-1], rec[:-1], B.oracle_parabolic_fits))


# ---- the refinement over images -----------------------------------------------------------------------------------------------

CASES = [(fam, size, half) for fam in RC.FAMILIES for size in range(len(RC.SIZES)) for half in (1, 0)]


def _expect_kernels(stats, refinement, launches):
    """the refinement's launch (k_refine<TILED> or k_parabolic_costs) and, for refinement = 2, the tail's - nothing else"""
    ran = {k: v[1] for k, v in stats.items() if v[1]}
    assert ran == ({"k_refine": launches, "k_parabolic_apply": launches} if refinement == 2 else {"k_refine": launches}), ran


@pytest.mark.parametrize("fam,size,half", CASES)
def test_refine_vs_oracle(vm, B, fam, size, half):
    """both refinements, the three methods on stereo frames and method 0 on mono frames, every list of lists_of(size)"""
    named = RC.lists_of(size)
    for refinement in (1, 2):
        for mono in (False, True):
            g = vm.Matcher(half_resolution=half, refinement=refinement)
            c = B.CpuMatcher("oracle", half_resolution=half, refinement=refinement)
            try:
                RC.push_all(g, fam, size, mono)
                RC.push_all(c, fam, size, mono)
                g.set_profiling(True)
                methods = (0,) if mono else (0, 1, 2)
                for method in methods:
                    for name, lists in named:
                        got = g.refine_lists(method, lists)
                        assert len(got) == len(lists)
                        for k, (m, gk) in enumerate(zip(lists, got)):
                            want = c.refine(m, method)
                            assert len(gk) == len(want), (refinement, mono, method, name, k, len(gk), len(want))
                            assert same(gk, want), (refinement, mono, method, name, k, np.flatnonzero(gk != want)[:8])
                _expect_kernels(g.kernel_stats(), refinement, len(methods) * len(named))
                if mono:
                    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):
                        g.refine_lists(2, named[0][1])
            finally:
                g.close()
                c.close()


def test_refine_needs_no_match_and_invalidates_the_last_one(vm, B):
    g = vm.Matcher(refinement=1)
    c = B.CpuMatcher("oracle", refinement=1)
    try:
        m = RC.lists_of(1)[3][1]
        with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):
            g.refine_lists(2, m)                        # nothing pushed yet
        RC.push_all(g, "synth", 1)
        RC.push_all(c, "synth", 1)
        assert g.match(2) and c.match(2) and len(g.matches()) > 100
        (got,) = g.refine_lists(2, m)
        assert same(got, c.refine(m[0], 2))
        assert len(g.matches()) == 0 and all(len(g.stage(s)) == 0 for s in range(5))
        assert g.match(2) and same(g.matches(), c.matches())
    finally:
        g.close()
        c.close()


@pytest.mark.parametrize("half,refinement", [(1, 1), (0, 2)])
def test_refine_rejections_leave_the_handle_usable(vm, B, half, refinement):
    """every rejected argument returns VSM_EARG before a launch; an ordinary match() afterwards equals the oracle's"""
    w, h = RC.SIZES[0]
    g = vm.Matcher(half_resolution=half, refinement=refinement)
    c = B.CpuMatcher("oracle", half_resolution=half, refinement=refinement)
    try:
        RC.push_all(g, "synth", 0)
        RC.push_all(c, "synth", 0)
        g.set_profiling(True)
        ok = RC.master_list(0)[:40]
        bad = []
        for f, v in (("u1c", np.nan), ("v2p", np.inf), ("u1c", 20.5), ("u1c", RC.MARGIN - 1), ("u1c", w - RC.MARGIN), ("v1c", h - RC.MARGIN), ("v1c", -7),
                     ("u1c", 1e9)):
            m = ok.copy()
            m[f][39] = v
            bad.append(dict(lists=[ok, m]))
        big = np.zeros(RC.PARA_MAX_LIST + 1, dtype=RC.MATCH)
        big["u1c"] = big["v1c"] = 20
        bad += [dict(lists=[big]), dict(lists=[ok], counts=[-1]), dict(lists=[]), dict(lists=[ok[:1]] * 65), dict(lists=[ok], method=3), dict(lists=[ok], method=-1)]
        for kw in bad:
            with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
                g.refine_lists(kw.pop("method", 2), **kw)
        assert not any(v[1] for v in g.kernel_stats().values())          # nothing was launched
        (got,) = g.refine_lists(2, [ok])
        assert same(got, c.refine(ok, 2))
        for method in (2, 0, 1):
            assert g.match(method) and c.match(method)
            assert same(g.matches(), c.matches()) and len(g.matches()) > 50, method
    finally:
        g.close()
        c.close()


def test_refinement_zero_is_rejected(vm):
    g = vm.Matcher(refinement=0)
    try:
        RC.push_all(g, "synth", 0)
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            g.refine_lists(2, [RC.master_list(0)[:5]])
    finally:
        g.close()
