"""GPU suite (run with -m gpu on an MI355X): the HIP path on the content families of tests/content.py - ties in the
suppression cells, saturated filters, descriptors that repeat inside every search window, lists of 0, 1, 2 and 3 matches
next to lists of thousands.  Everything is tobytes() equality with the CPU oracle run side by side, and with the hashes
the reference left in tests/golden/content_hashes.npz; no tolerance anywhere.  Every test asserts from the oracle's side
(list lengths, feature counts) that it is not vacuous.  tests/test_content_cpu.py pins the oracle on the same cases."""
import numpy as np
import pytest

import content as CT
import golden_util as G
from conftest import pkg

pytestmark = pytest.mark.gpu

VSM_PARA_MAX_LIST = 16384       # look-ahead, refinement = 2: longer dense query lists decline the GPU-resident form
VSM_DC_KD_MAX_POINTS = 65536    # look-ahead: longer dense query lists decline the GPU-resident form
VSM_DC_TIE_POINTS = 10240       # look-ahead: longer sparse query lists decline
VSM_DC2_PRIOR_MAX_BINS = 1024   # look-ahead: frames with more prior bins decline

FLAT = ("flat0", "flat77", "flat255")


@pytest.fixture(scope="module")
def vm():
    m = pkg("visomatch")
    m.lib()  # raises if the HIP library is missing: no silent fallback
    return m


# ---- planes --------------------------------------------------------------------------------------------------------------

PLANE_GEOMETRIES = ((333, 141, 0), (417, 163, 1), (1242, 375, 1), (640, 200, 1), (333, 141, 1), (417, 163, 0))


@pytest.mark.parametrize("fam", CT.FAMILIES)
def test_planes_vs_oracle(vm, B, fam):
    """whole du / dv / f1 / f2 planes of both images, matching and full resolution, from the fused tiles (k_feat_dense's side
    output) and from k_filters; widths that are not multiples of 16 and one multiple of 64"""
    peak = 0
    for w, h, half in PLANE_GEOMETRIES:
        l, r = CT.stereo_sequence(fam, w, h, 1, seed=CT.SEED, scale=2 if half else 1)[0]
        img, rimg = B.pad_image(l), B.pad_image(r)
        mimg, rm = (B.half_image("oracle", img, w), B.half_image("oracle", rimg, w)) if half else (img, rimg)
        (du, dv), (du2, dv2) = B.sobel5x5("oracle", mimg), B.sobel5x5("oracle", rm)
        f1, f2 = B.blob5x5("oracle", mimg), B.checkerboard5x5("oracle", mimg)
        peak = max(peak, int(np.abs(f1).max()), int(np.abs(f2).max()))
        for fused in (1, 0):
            m = vm.Matcher(half_resolution=half, options={"fused_features": fused, "filter_planes": 1})
            assert m.push_back(l, r) == 0
            what = (fam, w, h, half, fused)
            gdu, gdv = m.gradients(2, False)
            assert gdu.tobytes() == du.tobytes() and gdv.tobytes() == dv.tobytes(), what
            gdu2, gdv2 = m.gradients(3, False)
            assert gdu2.tobytes() == du2.tobytes() and gdv2.tobytes() == dv2.tobytes(), what
            if half:
                duf, dvf = B.sobel5x5("oracle", img)
                gduf, gdvf = m.gradients(2, True)
                assert gduf.tobytes() == duf.tobytes() and gdvf.tobytes() == dvf.tobytes(), what
            g1, g2 = m.filter_responses()
            assert g1.tobytes() == f1.tobytes() and g2.tobytes() == f2.tobytes(), what
            m.close()
    assert fam in FLAT or peak >= 100, (fam, peak)   # (a flat image responds at the row padding only)


def test_planes_at_the_ends_of_the_filter_ranges(vm, B):
    """f1 = +-4080, f2 = +-2040 and Sobel bytes 32 and 223 (the ranges csrc/vsm_feat.h's packed arithmetic relies on) on the
    device, full resolution and half"""
    l, r = CT.stereo_sequence("blocks3", 333, 141, 1, seed=3)[0]
    l2, r2 = (np.ascontiguousarray(np.kron(x, np.ones((2, 2), np.uint8))) for x in (l, r))   # its half image is l again
    for li, ri, half in ((l, r, 0), (l2, r2, 1)):
        img = B.pad_image(li)
        mimg = B.half_image("oracle", img, li.shape[1]) if half else img
        (du, dv), f1, f2 = B.sobel5x5("oracle", mimg), B.blob5x5("oracle", mimg), B.checkerboard5x5("oracle", mimg)
        assert (f1.min(), f1.max(), f2.min(), f2.max()) == (-4080, 4080, -2040, 2040)
        assert (du.min(), du.max(), dv.min(), dv.max()) == (32, 223, 32, 223)
        for fused in (1, 0):
            m = vm.Matcher(half_resolution=half, options={"fused_features": fused, "filter_planes": 1})
            assert m.push_back(li, ri) == 0
            gdu, gdv = m.gradients(2, False)
            g1, g2 = m.filter_responses()
            assert gdu.tobytes() == du.tobytes() and gdv.tobytes() == dv.tobytes(), (half, fused)
            assert g1.tobytes() == f1.tobytes() and g2.tobytes() == f2.tobytes(), (half, fused)
            m.close()


# ---- per-frame API -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", CT.FAMILIES)
def test_per_frame_vs_oracle_and_golden(vm, B, fam):
    """every family x four parameter sets x quad, flow and stereo matching, three frames: all feature sets, match()'s value,
    stages 0-4, the prior ranges, the final list - against the oracle and against the reference's recorded hashes"""
    g = G.load("content_hashes")
    CT.check_golden_inputs(g, B)
    nfeat = longest = 0
    for pi, p in enumerate(CT.PARAM_SETS):
        for method in CT.METHODS:
            want = CT.oracle_case(B, fam, pi, method)
            m = vm.Matcher(stage_capture=True, **p)
            got = CT.record(m, CT.case_sequence(fam, pi), method, B.make_params(**p)["multi_stage"])
            m.close()
            CT.assert_same_records(got, want, (fam, pi, method))
            CT.check_against_golden(g, fam, pi, method, got)
            nfeat += sum(len(x["feats"]["1c2"]) for x in want)
            longest = max(longest, max(len(x["final"]) for x in want))
    if fam in FLAT:
        assert nfeat == 0
    else:
        assert nfeat > 1000, (fam, nfeat)
    if fam in ("binary", "bytes", "blocks2", "blocks3", "blocks4", "blocks8", "tile150", "btile100"):
        assert longest > 1000, (fam, longest)


def _side_by_side(vm, B, seq, method, params, options=None, replace_last=False, tr=None, intr=None, device=False):
    """pushes the sequence through the HIP path and the oracle, compares everything after every frame; returns the oracle's
    (dense feature count, final list length, SADs per query) of the last frame"""
    g, c = vm.Matcher(stage_capture=True, options=options, **params), B.CpuMatcher("oracle", **params)
    if intr:
        g.set_intrinsics(*intr)
        c.set_intrinsics(*intr)
    what = (params, options, method)
    for f, (l, r) in enumerate(seq):
        rep = replace_last and f == len(seq) - 1
        if device:
            import torch
            gl, gr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
        else:
            gl, gr = l, r
        assert g.push_back(gl, gr if method else None, replace=rep) == 0
        c.push_back(l, r if method else None, replace=rep)
        for s in CT.SETS + ("1p1", "1p2"):
            assert CT.same(g.features(s), c.features(s)), (what, f, s)
        t = tr if (tr is not None and f >= 1) else None
        ran = c.match(method, t)
        assert g.match(method, t) == ran, (what, f)
        if ran:
            for s in range(5):
                assert CT.same(g.stage(s), c.stage(s)), (what, f, "stage", s, len(g.stage(s)), len(c.stage(s)))
            if c.p["multi_stage"]:
                ns = 4 if method == 2 else 2
                assert np.array_equal(g.ranges()[:, :, :ns], c.ranges()[:, :, :ns]), (what, f)
        assert CT.same(g.get_matches(), c.matches()), (what, f, len(g.get_matches()), len(c.matches()))
    out = (len(c.features("1c2")), len(c.matches()), CT.sads_per_query(c.counters()))
    g.close()
    c.close()
    return out


TIED = ("blocks4", "checker4", "btile32")


@pytest.mark.parametrize("fam", TIED)
def test_suppression_scales_on_tied_content(vm, B, fam):
    """nms_n 1, 2, 3, 4, 7 and 11 through the unfused suppression (dense / sparse scale n / 3n: k_nms_tile / k_nms_fixed,
    k_nms_tile / k_nms_tile8, k_nms_fixed both, k_nms_tile / k_nms, k_nms_tile8 / k_nms, k_nms both) and through the
    default path, on plateaus and lattices"""
    seq = CT.stereo_sequence(fam, 417, 163, 3, seed=CT.SEED, scale=2)
    for n in (1, 2, 3, 4, 7, 11):
        for fused in (0, 1):
            nfeat, _, _ = _side_by_side(vm, B, seq, 2, dict(nms_n=n), options={"fused_features": fused})
            assert nfeat > 30, (fam, n, nfeat)


@pytest.mark.parametrize("fam", TIED)
def test_matcher_variants_on_tied_content(vm, B, fam):
    """bins of 7, 23 and 301 px, the second pass on per-bin head records, a replaced third frame, and quad matching with a
    Tr_delta (double costs: ties in SAD that the distance term must break as the reference does) where descriptors repeat"""
    w, h = 417, 163
    seq = CT.stereo_sequence(fam, w, h, 3, seed=CT.SEED, scale=2)
    seen = []
    for bs in (7, 23, 301):
        seen.append(_side_by_side(vm, B, seq, 2, dict(match_binsize=bs)))
    for method in CT.METHODS:
        seen.append(_side_by_side(vm, B, seq, method, {}, options={"match_heads": 1}))
        seen.append(_side_by_side(vm, B, seq, method, {}, replace_last=True))
    Tr = np.eye(4)
    Tr[0, 3], Tr[2, 3], Tr[0, 2], Tr[2, 0] = 0.011, -0.35, 0.004, -0.004
    intr = (400.0, w / 2.0 + 0.5, h / 2.0 - 0.25, 0.54)
    for p in (dict(), dict(multi_stage=0), dict(half_resolution=0), dict(refinement=2)):
        sq = CT.stereo_sequence(fam, w, h, 3, seed=CT.SEED, scale=2 if p.get("half_resolution", 1) else 1)
        seen.append(_side_by_side(vm, B, sq, 2, p, tr=Tr, intr=intr))
        seen.append(_side_by_side(vm, B, sq, 2, p, options={"match_heads": 1}, tr=Tr, intr=intr))
    assert min(x[0] for x in seen) > 500, seen
    if fam != "blocks4":   # descriptors repeat: a query judges tens of candidates
        assert max(x[2] for x in seen) >= 30, seen


@pytest.mark.parametrize("half", [1, 0])
@pytest.mark.parametrize("w,h", [(333, 141), (418, 163), (419, 120), (1242, 375)])
def test_border_marks_from_device_memory(vm, B, w, h, half):
    """marks at every distance 0 .. 13 from the frame's edges, widths 1, 2 and 3 mod 4, through k_ingest (device-resident
    inputs) and from host memory"""
    seq = CT.stereo_sequence("border_marks", w, h, 3, scale=2 if half else 1)
    for device in (True, False):
        for method in (2, 0):
            nfeat, _, _ = _side_by_side(vm, B, seq, method, dict(half_resolution=half), device=device)
            assert nfeat > 20, (w, h, half, nfeat)
    if (w, h) == (333, 141):
        _side_by_side(vm, B, seq, 2, dict(half_resolution=half, nms_n=1, nms_tau=20, multi_stage=0), device=True)


@pytest.mark.parametrize("method", CT.METHODS)
def test_scene_changes_frame_by_frame(vm, B, method):
    """content that changes every second frame through pushBack + matchFeatures: lists of thousands, of a handful and of
    nothing follow each other, and where matching does not run (a flat frame) the list of the frame before stays"""
    seq = CT.scene_changes(12, 640, 200, seed=1)
    for p in (dict(), dict(refinement=2), dict(multi_stage=0, refinement=0)):
        _, n_last, _ = _side_by_side(vm, B, seq, method, p)
        assert n_last > 1000, (method, p, n_last)
    c = B.CpuMatcher("oracle")
    kept = 0
    for l, r in seq:
        c.push_back(l, r if method else None)
        kept += (not c.match(method)) and len(c.matches()) > 1000
    c.close()
    assert kept >= 2, kept


# ---- look-ahead ----------------------------------------------------------------------------------------------------------

LOOKAHEAD = {"scene_changes": (640, 200), "blocks2": (640, 200), "checker4": (417, 163), "btile100": (417, 163)}
_LOOKAHEAD_ORACLE = {}


def _lookahead_frames(name):
    w, h = LOOKAHEAD[name]
    return CT.scene_changes(12, w, h, seed=1) if name == "scene_changes" else CT.stereo_sequence(name, w, h, 12, seed=CT.SEED, scale=2)


def _expected_path(vm, w, h, params, v2, nq0, nq1):
    """the rule of vsm_sequence_run / vsm_seq2.inc: the GPU-resident form unless it is switched off or declines"""
    p = vm.default_params()
    for k, v in params.items():
        setattr(p, k, v)
    bins = -(-w // p.match_binsize) * -(-h // p.match_binsize)
    declines = (bins > VSM_DC2_PRIOR_MAX_BINS or nq0 > VSM_DC_TIE_POINTS or nq1 > VSM_DC_KD_MAX_POINTS or
                (p.refinement == 2 and nq1 > VSM_PARA_MAX_LIST))
    return 2 if v2 and not declines else 1


@pytest.mark.parametrize("refinement", [1, 2])
@pytest.mark.parametrize("method", [2, 0])
@pytest.mark.parametrize("name", list(LOOKAHEAD))
def test_lookahead_on_content(vm, B, monkeypatch, name, method, refinement):
    """run_sequence over 12 frames against the oracle frame by frame: both forms, chunks of 1, 3 and 5 (with scene_changes
    the pass-1 slabs grow in the middle of a call), host and device inputs, quad and mono flow matching, refinement 1 and 2;
    the form taken against the rule worked out from the oracle's feature counts"""
    w, h = LOOKAHEAD[name]
    seq = _lookahead_frames(name)
    params = dict(refinement=refinement)
    c = B.CpuMatcher("oracle", **params)
    want, ran, nq0, nq1 = [], [], 0, 0
    for l, r in seq:
        c.push_back(l, r if method else None)
        nq0, nq1 = max(nq0, len(c.features("1c1"))), max(nq1, len(c.features("1c2")))
        ran.append(bool(c.match(method)))
        want.append(c.matches())
    c.close()
    lens = [len(x) for x in want]
    if name == "scene_changes":   # thousands, a handful and nothing, in both orders
        steps = list(zip(lens[:-1], lens[1:]))
        assert max(lens) > 1000 and any(0 < n < 20 for n in lens) and lens[:3] == [0, 0, 0], lens
        assert any(a > 1000 and b < 20 for a, b in steps) and any(a < 20 and b > 1000 for a, b in steps), lens
        assert ran.count(False) >= 4 and any(not k and n > 1000 for k, n in zip(ran, lens)), (ran, lens)   # an early return keeps the list
    elif name == "blocks2":
        assert min(lens[1:]) > 1000, lens
    elif name == "checker4":
        assert max(lens) <= 3 and max(lens) > 0 and nq1 > 2000, (lens, nq1)
    else:
        assert min(lens[1:]) > 200, lens
    left, right = CT.stack(seq)
    if method == 0:
        right = None
    for v2, chunk, device in [(v, ch, False) for v in (1, 0) for ch in (1, 3, 5)] + [(1, 3, True), (0, 3, True), (1, 5, True)]:
        monkeypatch.setenv("VSM_SEQ_V2", str(v2))
        monkeypatch.setenv("VSM_SEQ_CHUNK", str(chunk))
        gl, gr = left, right
        if device:
            import torch
            gl, gr = torch.from_numpy(left).cuda(), (torch.from_numpy(right).cuda() if right is not None else None)
        g = vm.Matcher(**params)
        got = g.run_sequence(gl, gr, method)
        path = g.sequence_path()
        g.close()
        what = (name, method, refinement, v2, chunk, device)
        for f in range(len(seq)):
            assert CT.same(got[f], want[f]), (what, f, len(got[f]), len(want[f]))
        assert path == _expected_path(vm, w, h, params, v2, nq0, nq1), (what, path)
        if v2:
            assert path == 2, what   # sizes chosen so that every sequence here takes the GPU-resident form
