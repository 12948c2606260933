"""GPU suite (run with -m gpu on an MI355X): the four HIP kernels of the monocular egomotion (csrc/vsm_mono.hip), each
alone through its vsm_debug_mono_* entry against the CPU oracle's piece of the same name, on the inputs of
tests/mono_content.py that send the SVD through its rank-deficient paths; then every match family through
VisualOdometryMono.process_matches against the oracle and tests/golden/mono_content.npz, with the stages the GPU took.

Doubles are compared byte for byte, except that where the oracle's double is NaN the device's only has to be NaN too
(x86 and gfx950 may differ in the sign bit of a generated NaN)."""
import os

import numpy as np
import pytest

import mono_content as MC
from conftest import pkg

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def vm():
    m = pkg("visomatch")
    m.lib()  # raises if the HIP library is missing: no silent fallback
    return m


def same_doubles(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.all(np.isnan(got[nan]))) and got[~nan].tobytes() == want[~nan].tobytes()


def _device_svd(vm):
    v = vm.VisualOdometryMono(MC.F, MC.CU, MC.CV)
    try:
        return v.device_svd()
    finally:
        v.close()


# ---- k_mono_fit -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_fits(B):
    """the oracle's fits of fit_inputs(200); fit_inputs(K) is its prefix for every smaller K"""
    pts, picks, _ = MC.fit_inputs(200)
    m = MC.as_matches(pts)
    return np.stack([B.oracle_fundamental(m, picks[k]) for k in range(len(picks))])


@pytest.mark.parametrize("K", [1, 15, 16, 17, 33, 200])
def test_fit_vs_oracle(vm, oracle_fits, K):
    """all nine doubles of every hypothesis; the hypotheses of a wave take different branches of the cooperative SVD"""
    assert _device_svd(vm) == 1      # a device SVD that fails the context's self-test is a failure here, not a fallback
    pts, picks, props = MC.fit_inputs(K)
    assert np.array_equal(picks, MC.fit_inputs(200)[1][:K])
    got = vm.device_mono_fit(pts, picks)
    bad = [(k, props[k]) for k in range(K) if not same_doubles(got[k], oracle_fits[k])]
    assert not bad, bad[:8]


# ---- k_mono_inlier_count ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def count_cases(B):
    """{K: (F [K, 3, 3], the oracle's counts [len(COUNT_NS), K])} on the first n of count_points()"""
    pts = MC.count_points()
    thr = 1e-5
    out = {}
    for K in MC.COUNT_KS:
        Fs = MC.count_matrices(B, K)
        want = np.array([[B.oracle_mono_inlier_count(MC.as_matches(pts[:n]), Fs[k], thr) for k in range(K)] for n in MC.COUNT_NS])
        out[K] = (Fs, want)
    return pts, thr, out


@pytest.mark.parametrize("K", MC.COUNT_KS)
@pytest.mark.parametrize("n", MC.COUNT_NS)
def test_count_vs_oracle(vm, count_cases, n, K):
    pts, thr, cases = count_cases
    Fs, want = cases[K]
    got = vm.device_mono_count(pts[:n], Fs, thr)
    assert np.array_equal(got, want[MC.COUNT_NS.index(n)]), (n, K)


def test_count_threshold_on_the_edge(vm, B):
    """thr is exactly one match's distance: the strict `<` leaves it out, the next double takes it in"""
    pts, Fm, thr = MC.edge_threshold(B)
    m = MC.as_matches(pts)
    for t in (np.nextafter(thr, 0), thr, np.nextafter(thr, 1)):
        assert vm.device_mono_count(pts, Fm, t)[0] == B.oracle_mono_inlier_count(m, Fm, t), t
    assert vm.device_mono_count(pts, Fm, np.nextafter(thr, 1))[0] > vm.device_mono_count(pts, Fm, thr)[0]


def test_count_in_slices(vm, count_cases):
    """20 hypotheses in launches of at most 7 (the path more hypotheses than the grid's y extent take)"""
    pts, thr, cases = count_cases
    Fs, want = cases[200]
    w = want[MC.COUNT_NS.index(257)][:20]
    assert len(set(w[14:])) > 1 and w[14:].max() > 0        # the last slice has something to lose
    for sl in (7, 1, 20, 0):
        assert np.array_equal(vm.device_mono_count(pts[:257], Fs[:20], thr, slice=sl), w), sl


# ---- k_mono_triangulate -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("zero_t", [False, True])
@pytest.mark.parametrize("n", MC.TRI_NS)
def test_triangulate_vs_oracle(vm, B, n, zero_t):
    """all of X[4][4][n] and the four chirality counts; a match that does not move, one on the principal point in both
    frames and a repeated one are in every list; t = 0 makes both cameras coincide"""
    m = MC.triangulation_matches(n)
    R4, t4 = MC.rt_candidates(zero_t=zero_t)
    X, chir = vm.device_mono_triangulate(m, MC.F, MC.CU, MC.CV, R4, t4)
    for c in range(4):
        Xo, co = B.oracle_mono_triangulate(m, MC.F, MC.CU, MC.CV, R4[c], t4[c])
        assert same_doubles(X[c], Xo), (c, np.argwhere(X[c] != Xo)[:5].tolist())
        assert chir[c] == co, (c, chir.tolist(), co)


# ---- k_mono_plane_vote ------------------------------------------------------------------------------------------------------

VOTE_EPS = 5e-10     # best_plane keeps proposals down to top * (1 - 1e-9): the true first maximum is among them if every
                     # proposal is within eps of its exact sum and 2 eps <= 1e-9


@pytest.mark.parametrize("np_", MC.VOTE_NPS)
@pytest.mark.parametrize("kind", MC.VOTE_KINDS)
def test_vote_vs_oracle(vm, B, kind, np_):
    d, threshold, weight = MC.vote_inputs(kind, np_)
    want_sums, want_idx = B.oracle_mono_plane_vote(d, threshold, weight)
    sums, idx, on_device = vm.device_mono_vote(d, threshold, weight)
    assert on_device
    above = d > threshold
    assert np.all(sums[~above] == 0)
    dev = float(np.max(np.abs(sums[above] - want_sums[above]) / want_sums[above])) if above.any() else 0.0
    print(f"vote {kind} np={np_}: largest relative deviation of a proposal {dev:.3e}")
    assert idx == want_idx, (idx, want_idx)
    if above.any():
        assert want_sums[above].min() >= 1.0     # the candidate's own term is exp(0)
    assert dev <= VOTE_EPS, dev


def test_vote_below_512_points_runs_on_the_host(vm, B):
    d, threshold, weight = MC.vote_inputs("scene", 512)
    sums, idx, on_device = vm.device_mono_vote(d[:511], threshold, weight)
    want_sums, want_idx = B.oracle_mono_plane_vote(d[:511], threshold, weight)
    assert not on_device and idx == want_idx and sums.tobytes() == want_sums.tobytes()


# ---- every family end to end ------------------------------------------------------------------------------------------------

def test_families_end_to_end(vm, B):
    want = MC.replay(B.OracleMonoVO, B.oracle_sampler_seed, after=lambda vo: B.oracle_mono_last_in_front())
    got = MC.replay(vm.VisualOdometryMono, vm.vo_sampler_seed, after=lambda vo: (vo.device_svd(), vo.device_stages()))
    g = np.load(os.path.join(HERE, "golden", "mono_content.npz"))
    MC.assert_equals_golden(got, g, same_doubles)
    for name in MC.FAMILIES:
        ok, T, inl, (svd, stages) = got[name]
        ok_o, T_o, inl_o, front = want[name]
        assert svd == 1, name
        assert ok == ok_o and np.array_equal(inl, inl_o) and same_doubles(T, T_o), name
        expect = vm.MONO_STAGE_FIT | vm.MONO_STAGE_COUNT      # every family has n >= 10 and normalises
        if len(inl_o) >= 10:
            expect |= vm.MONO_STAGE_TRIANGULATE
        if ok_o and front >= MC.VOTE_MIN_POINTS:
            expect |= vm.MONO_STAGE_VOTE
        assert stages == expect, (name, stages, expect, front)
    assert got["front512"][3][1] & vm.MONO_STAGE_VOTE and not got["front511"][3][1] & vm.MONO_STAGE_VOTE
