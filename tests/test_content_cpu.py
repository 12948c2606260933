"""The content families of tests/content.py (ties, saturation, repeats) on the CPU: that each family reaches the condition it
was written for (measured with the oracle), the oracle against the compiled reference on every family (where that build
is present), the CPU emulation of the fused feature tiles against the oracle, and the oracle against the hashes the
reference left in tests/golden/content_hashes.npz (tests/golden/make_golden.py content_hashes).
tests/test_content_gpu.py runs the HIP path over the same cases.
"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import content as CT
import golden_util as G
import test_feat_emu as FE

TAU, N_DENSE = 50, 3


def planes(B, kind, l, half):
    h, w = l.shape
    img = B.pad_image(l)
    mimg = np.ascontiguousarray(B.half_image(kind, img, w) if half else img)
    return mimg, (w // 2 if half else w), B.sobel5x5(kind, mimg), B.blob5x5(kind, mimg), B.checkerboard5x5(kind, mimg)


# ---- the families reach their conditions ----------------------------------------------------------------------------------

def _measure(B, fam, w=640, h=200, seed=5):
    """default parameters, quad matching, third frame: (f1 tie share, f2 tie share, duplicate share of the dense features,
    SADs per query, dense features, match()'s value)"""
    seq = CT.stereo_sequence(fam, w, h, 3, seed=seed, scale=2)
    c = B.CpuMatcher("oracle")
    for l, r in seq:
        c.push_back(l, r)
        ran = c.match(2)
    _, mw, _, f1, f2 = planes(B, "oracle", seq[2][0], True)
    t1, t2 = CT.tie_cells(f1, mw, N_DENSE, TAU), CT.tie_cells(f2, mw, N_DENSE, TAU)
    feats = c.features("1c2")
    out = (t1[0] / max(t1[1], 1), t2[0] / max(t2[1], 1), CT.dup_share(feats), CT.sads_per_query(c.counters()), len(feats), ran)
    c.close()
    return out


def test_families_reach_their_conditions(B, synth):
    """conditions on the inputs, from the oracle at 640 x 200 with default parameters (the suite's other images, synth.py's:
    0.2 % of the dense suppression cells tie, 2 % of the descriptors repeat, a query judges 2.4 candidates)"""
    base = synth.stereo_sequence(5, 640, 200, 3)
    c = B.CpuMatcher("oracle")
    for l, r in base:
        c.push_back(l, r)
        c.match(2)
    assert CT.dup_share(c.features("1c2")) < 0.1 and CT.sads_per_query(c.counters()) < 5   # what the families are measured against
    c.close()
    for fam in ("blocks4", "blocks8"):
        assert _measure(B, fam)[0] >= 0.25, fam
    assert _measure(B, "checker4")[0] == 1.0
    assert _measure(B, "dots8")[1] == 1.0              # the lattice ties the checkerboard response instead
    for fam in CT.PERIODIC:
        _, _, dup, sq, nfeat, ran = _measure(B, fam)
        assert dup >= 0.95 and nfeat > 1000, (fam, dup, nfeat)
        if fam == "checker2":   # 1 px squares at half resolution: no sparse features, match() returns false
            assert not ran and nfeat > 1000
        else:
            assert ran and sq >= 30, (fam, sq)
    assert _measure(B, "tile150")[2] >= 0.95           # repeats beyond most windows: no condition on its S/Q
    # saturation: the ends of the ranges that the header of csrc/vsm_feat.h argues for
    l = CT.stereo_sequence("blocks3", 333, 141, 1, seed=3)[0][0]
    _, _, (du, dv), f1, f2 = planes(B, "oracle", l, False)
    assert (f1.min(), f1.max(), f2.min(), f2.max()) == (-4080, 4080, -2040, 2040)
    assert (du.min(), du.max(), dv.min(), dv.max()) == (32, 223, 32, 223)


@pytest.mark.parametrize("tau,half", [(50, True), (50, False), (20, False), (90, True)])
def test_threshold_family_has_extrema_at_the_threshold(B, tau, half):
    """cell extrema of exactly tau - 1, tau and tau + 1 in both planes and both signs; the suppression keeps tau and tau + 1"""
    w, h = (640, 200) if half else (333, 141)
    l = CT.stereo_sequence("threshold", w, h, 1, tau=tau, scale=2 if half else 1)[0][0]
    _, mw, _, f1, f2 = planes(B, "oracle", l, half)
    for f in (f1, f2):
        mx, mn = set(), set()
        for i in range(N_DENSE + CT.MARGIN, mw - N_DENSE - CT.MARGIN, N_DENSE + 1):
            for j in range(N_DENSE + CT.MARGIN, f.shape[0] - N_DENSE - CT.MARGIN, N_DENSE + 1):
                cell = f[j:j + N_DENSE + 1, i:i + N_DENSE + 1]
                mx.add(int(cell.max()))
                mn.add(int(cell.min()))
        assert {tau - 1, tau, tau + 1} <= mx and {-tau + 1, -tau, -tau - 1} <= mn, (tau, half, sorted(mx), sorted(mn))
    kept = B.nms("oracle", f1, f2, mw, N_DENSE, tau)
    for cls, want in ((0, {-tau, -tau - 1}), (1, {tau, tau + 1}), (2, {-tau, -tau - 1}), (3, {tau, tau + 1})):
        vals = set(kept[kept[:, 3] == cls][:, 2].tolist())
        assert want <= vals and all(abs(v) >= tau for v in vals), (tau, half, cls, sorted(vals))


def test_cases_reach_short_lists(B):
    """across the per-frame cases: final lists of 1, 2 and 3 matches, a non-empty stage 2 with an empty stage 4, lists of
    thousands, and a match() that returns false on more than 1000 features"""
    finals, emptied, refused = set(), 0, 0
    for fam in CT.FAMILIES:
        for pi in range(len(CT.PARAM_SETS)):
            for method in CT.METHODS:
                for rec in CT.oracle_case(B, fam, pi, method)[1:]:
                    finals.add(len(rec["final"]))
                    if rec["ran"]:
                        emptied += len(rec["stages"][2]) > 0 and len(rec["stages"][4]) == 0
                    else:
                        refused += len(rec["feats"]["1c2"]) > 1000
    assert {0, 1, 2, 3} <= finals and max(finals) > 2000, sorted(finals)[:8]
    assert emptied > 0 and refused > 0


# ---- the oracle against the compiled reference ------------------------------------------------------------------------------

needs_ref = pytest.mark.skipif(not __import__("oracle.bindings", fromlist=["x"]).have_ref(),
                               reason="oracle/_ref/libvisoref.so not built")


@needs_ref
@pytest.mark.parametrize("fam", CT.FAMILIES)
def test_oracle_vs_reference_planes(B, fam):
    """Sobel, blob, checkerboard, half image and the suppression at six scales and three thresholds, with
    tests/test_oracle_vs_ref.py's masks for the bytes the reference never writes"""
    w, h = 333, 141
    l = CT.stereo_sequence(fam, w, h, 1, seed=CT.SEED)[0][0]
    img = B.pad_image(l)
    n = img.size
    (duo, dvo), (dur, dvr) = B.sobel5x5("oracle", img), B.sobel5x5("ref", img)
    assert np.array_equal(duo.ravel()[2:n - 2], dur.ravel()[2:n - 2])
    assert np.array_equal(dvo.ravel()[2:n - 2], dvr.ravel()[2:n - 2])
    f1o, f1r = B.blob5x5("oracle", img), B.blob5x5("ref", img)
    f2o, f2r = B.checkerboard5x5("oracle", img), B.checkerboard5x5("ref", img)
    assert np.array_equal(f1o[3:h - 3, 3:w - 3], f1r[3:h - 3, 3:w - 3])
    assert np.array_equal(f2o[3:h - 3, 3:w - 3], f2r[3:h - 3, 3:w - 3])
    assert np.array_equal(B.half_image("oracle", img, w), B.half_image("ref", img, w))
    for n_ in (1, 2, 3, 5, 9, 10):
        for tau in (20, 50, 200):
            assert np.array_equal(B.nms("oracle", f1r, f2r, w, n_, tau), B.nms("ref", f1r, f2r, w, n_, tau)), (n_, tau)


@needs_ref
@pytest.mark.parametrize("fam", CT.FAMILIES)
def test_oracle_vs_reference_matcher(B, fam):
    """feature sets, match()'s value, the five stages, the prior ranges and the final list, frame by frame"""
    for pi, p in enumerate(CT.PARAM_SETS):
        for method in CT.METHODS:
            r = B.CpuMatcher("ref", **p)
            got = CT.record(r, CT.case_sequence(fam, pi), method, B.make_params(**p)["multi_stage"])
            r.close()
            CT.assert_same_records(CT.oracle_case(B, fam, pi, method), got, (fam, pi, method))


@needs_ref
@pytest.mark.parametrize("method", CT.METHODS)
def test_oracle_vs_reference_scene_changes(B, method):
    """twelve frames whose content changes every second frame: on a frame where matchFeatures returns early (a flat image has
    no features) getMatches() still shows the list of the frame before - in the reference and in the oracle alike; the
    look-ahead call of the HIP path has to return that list for such a frame (tests/test_content_gpu.py)"""
    seq = CT.scene_changes(12, 640, 200, seed=1)
    for p in (dict(), dict(refinement=2)):
        o, r = B.CpuMatcher("oracle", **p), B.CpuMatcher("ref", **p)
        kept = 0
        for f, (l, rt) in enumerate(seq):
            for m in (o, r):
                m.push_back(l, rt if method else None)
            ran = o.match(method)
            assert ran == r.match(method), (method, p, f)
            assert CT.same(o.matches(), r.matches()), (method, p, f, len(o.matches()), len(r.matches()))
            kept += (not ran) and len(o.matches()) > 1000
        assert kept >= 2, (method, p, kept)
        o.close()
        r.close()


# ---- the fused tiles' emulation against the oracle ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(FE.CLANG):
        pytest.skip("no clang++ with vector extensions here")
    L = C.CDLL(FE.build_emu())
    vp = C.c_void_p
    L.emu_feat_dense.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.emu_feat_sparse.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    return L


EMU_GEOMETRIES = [(1242, 375, True, 50), (333, 141, False, 20), (640, 480, False, 50), (417, 163, True, 1)]


@pytest.mark.parametrize("w,h,half,tau", EMU_GEOMETRIES)
@pytest.mark.parametrize("fam", CT.FAMILIES)
def test_fused_tiles_vs_oracle_on_content(emu, B, fam, w, h, half, tau):
    """the per-thread code of k_feat_dense / k_feat_sparse (csrc/vsm_feat.h), tile by tile on the CPU: whole planes and the
    survivors of both suppression scales in the reference's emission order"""
    l = CT.stereo_sequence(fam, w, h, 1, seed=CT.SEED, tau=max(tau, 20), scale=2 if half else 1)[0][0]
    mimg, mw, (du_o, dv_o), f1_o, f2_o = planes(B, "oracle", l, half)
    mh, mbpl = mimg.shape
    du, dv = np.full((mh, mbpl), 77, np.uint8), np.full((mh, mbpl), 77, np.uint8)
    f1, f2 = np.full((mh, mbpl), 777, np.int16), np.full((mh, mbpl), 777, np.int16)
    ncu, ncv = FE.cells(mw, 3), FE.cells(mh, 3)
    cand = np.full(max(ncu * ncv, 1) * 4, 12345, np.int32)
    emu.emu_feat_dense(FE.ptr(mimg), mw, mh, mbpl, tau, ncu, ncv, FE.ptr(du), FE.ptr(dv), FE.ptr(f1), FE.ptr(f2), FE.ptr(cand))
    assert np.array_equal(du, du_o) and np.array_equal(dv, dv_o)
    assert np.array_equal(f1, f1_o) and np.array_equal(f2, f2_o)
    want = [tuple(int(x) for x in (r[0], r[1], r[3])) for r in B.nms("oracle", f1_o, f2_o, mw, 3, tau)]
    assert FE.cand_list(cand, ncu, ncv) == want
    ncu9, ncv9 = FE.cells(mw, 9), FE.cells(mh, 9)
    cand9 = np.full(ncu9 * ncv9 * 4, 12345, np.int32)
    emu.emu_feat_sparse(FE.ptr(mimg), mw, mh, mbpl, tau, ncu9, ncv9, FE.ptr(cand9))
    want9 = [tuple(int(x) for x in (r[0], r[1], r[3])) for r in B.nms("oracle", f1_o, f2_o, mw, 9, tau)]
    assert FE.cand_list(cand9, ncu9, ncv9) == want9
    if not fam.startswith("flat"):
        assert len(want) > 20 and ncu9 * ncv9 > 0, (fam, len(want))
    if tau == 1 and fam not in ("flat0", "flat77", "flat255", "step", "threshold", "border_marks"):
        assert len(want) > ncu * ncv // 2, (fam, len(want), ncu * ncv)   # textured all over: most cells keep an extremum


# ---- the oracle against the reference's recorded hashes ----------------------------------------------------------------------

@pytest.mark.parametrize("fam", CT.FAMILIES)
def test_golden_content_oracle(B, fam):
    g = G.load("content_hashes")
    CT.check_golden_inputs(g, B)
    fi = list(g["families"]).index(fam)
    for pi in range(len(CT.PARAM_SETS)):
        for f, (l, r) in enumerate(CT.case_sequence(fam, pi)):
            assert hashlib.sha256(l.tobytes() + r.tobytes()).digest() == g["input_digests"][fi, pi, f].tobytes(), "tests/content.py drifted from the fixture's inputs"
        for method in CT.METHODS:
            CT.check_against_golden(g, fam, pi, method, CT.oracle_case(B, fam, pi, method))
