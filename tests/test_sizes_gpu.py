"""GPU suite (run with -m gpu on an MI355X): the image side of the HIP path over the frame sizes of tests/sizes.py - every
residue of the row padding, the first cell of either suppression scale, the second tile column and row of k_feat_dense and
k_feat_sparse, the clipped suppression at every pixel of width and height, the tiles of k_feat_order with 1, bu - 1 and bu
search bins, grids that are no multiple of 8.  Everything is equality of bytes with the CPU oracle run side by side on the
same frames, and with the hashes in tests/golden/size_hashes.npz; no tolerance anywhere.  The bin-sorted copy that
k_feat_order (or k_emit + k_bin_*) writes is read by k_match alone, so every size goes through matching with stage capture.
tests/test_sizes_cpu.py pins the oracle (against the reference) and the CPU emulation of the fused tiles on the same sizes."""
import numpy as np
import pytest

import sizes as S
from conftest import pkg

pytestmark = pytest.mark.gpu

RES = {"full": 0, "half": 1}


@pytest.fixture(scope="module")
def vm():
    m = pkg("visomatch")
    m.lib()  # raises if the HIP library is missing: no silent fallback
    return m


def _gpu_record(vm, seq, method, half, options=None, profile=False, **params):
    """-> (record, kernel statistics or None)"""
    m = vm.Matcher(stage_capture=True, options=options, half_resolution=half, nms_tau=S.TAU, **params)
    if profile:
        m.set_profiling(True)
    rec = S.record(m, seq, method)
    st = m.kernel_stats() if profile else None
    m.close()
    return rec, st


def _check_path(st, plan, what):
    """the fused order (k_feat_scan, k_feat_order) or the separate kernels (k_emit, k_bin_rank), as vsm_order_plan's rule gives
    it for the size; neither where no set has a cell"""
    fused = st["k_feat_scan"][1] > 0 and st["k_feat_order"][1] > 0
    fallback = st["k_emit"][1] > 0 and st["k_bin_rank"][1] > 0
    if plan is None:
        assert st["k_feat_order"][1] == 0 and st["k_emit"][1] == 0, (what, "path")
    else:
        assert (fused, fallback) == ((True, False) if plan["fused"] else (False, True)), (what, "path", (fused, fallback), plan)


def _check_tiles(st, mw, mh, half, what, multi_stage=1, nms_n=3, fused_features=1, front=1):
    """the fused tiles or the separate filter and suppression kernels, as vsm_launch_features' rule gives them for the size;
    the fused front end at half resolution unless it is switched off"""
    fuse = bool(fused_features) and S.fused_tiles(mw, mh, multi_stage, nms_n)
    assert (st["k_feat_dense"][1] > 0) == fuse and (st["k_feat_sparse"][1] > 0) == (fuse and bool(multi_stage)), (what, "tiles", fuse)
    assert (st["k_filters<false>"][1] > 0) == (not fuse), (what, "k_filters")
    if S.cells(mw, nms_n) * S.cells(mh, nms_n) > 0:
        assert (st["k_nms:dense"][1] > 0) == (not fuse), (what, "k_nms")
    if half:
        assert (st["k_front"][1] > 0, st["k_halve"][1] > 0) == ((True, False) if front else (False, True)), (what, "front end")


# ---- planes --------------------------------------------------------------------------------------------------------------

def _first_plane_difference(got, want):
    if got is None:
        return "none"
    got = got.reshape(want.shape)
    if got.tobytes() == want.tobytes():
        return None
    y, x = np.argwhere(got != want)[0]
    return (int(x), int(y)), int(got[y, x]), int(want[y, x])


@pytest.mark.parametrize("res", list(RES))
@pytest.mark.parametrize("family", list(S.FAMILIES))
def test_planes(vm, B, synth, family, res):
    """du / dv of both images at the matching resolution and, with half resolution, at full resolution, and f1 / f2 (the side output
    of the fused tiles, or k_filters' planes where the frame has no dense cell): whole planes, pad columns included"""
    half = RES[res]
    for mw, mh in S.FAMILIES[family]:
        w, h = S.frame(mw, mh, half)
        l, r = S.frames(synth, w, h, 1)[0]
        img, rimg = B.pad_image(l), B.pad_image(r)
        mimg, rm = (B.half_image("oracle", img, w), B.half_image("oracle", rimg, w)) if half else (img, rimg)
        m = vm.Matcher(half_resolution=half, nms_tau=S.TAU, options={"filter_planes": 1})
        assert m.push_back(l, r) == 0
        want = dict(zip(("du", "dv"), B.sobel5x5("oracle", mimg)))
        want.update(zip(("du right", "dv right"), B.sobel5x5("oracle", rm)))
        got = dict(zip(("du", "dv"), m.gradients(2, False)))
        got.update(zip(("du right", "dv right"), m.gradients(3, False)))
        if half:
            want.update(zip(("du full", "dv full"), B.sobel5x5("oracle", img)))
            got.update(zip(("du full", "dv full"), m.gradients(2, True)))
            want.update(zip(("du full right", "dv full right"), B.sobel5x5("oracle", rimg)))
            got.update(zip(("du full right", "dv full right"), m.gradients(3, True)))
        want.update(f1=B.blob5x5("oracle", mimg), f2=B.checkerboard5x5("oracle", mimg))
        got.update(zip(("f1", "f2"), m.filter_responses()))
        m.close()
        for k in want:
            d = _first_plane_difference(got[k], want[k])
            assert d is None, ((mw, mh), res, k, d)


# ---- features and matches ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("res", list(RES))
@pytest.mark.parametrize("family", list(S.FAMILIES))
def test_features_and_matches(vm, B, synth, family, res):
    """default options, two frames, quad and flow matching with stage capture: the four feature sets, stages 0..4, the final
    list, the order kernels taken; frames with fewer than 4 sparse cells with multi_stage = 0 too"""
    half = RES[res]
    g = S.golden()
    for mw, mh in S.FAMILIES[family]:
        w, h = S.frame(mw, mh, half)
        seq = S.frames(synth, w, h)
        for params in ({}, {"multi_stage": 0}) if S.small(mw, mh) else ({},):
            for method in (2, 0):
                what = ((mw, mh), res, params, method)
                got, st = _gpu_record(vm, seq, method, half, profile=True, **params)
                S.assert_same_record(got, S.oracle_record(B, synth, w, h, half, method, **params), what)
                _check_path(st, S.order_plan(w, h, half, 50, params.get("multi_stage", 1)), what)
                _check_tiles(st, mw, mh, half, what, params.get("multi_stage", 1))
                if not params and method == 2:
                    for s in S.SETS:
                        S.check_slot(g, mw, mh, half, s, got["feats"][s])
                S.check_slot(g, mw, mh, half, f"final m{method}" + (" ms0" if params else ""), got["final"])


@pytest.mark.parametrize("res", list(RES))
@pytest.mark.parametrize("k", range(6))
def test_bin_families(vm, B, synth, k, res):
    """search bins that give tiles of 8, 4, 2 and 1 bins and both sides of the fall-back at bw = 72; widths at which the last
    tile of a tile row holds 1, bu - 1 and bu bins; all three methods, and quad and flow matching with multi_stage = 0 on the
    frames of one or two small bins, which have fewer than 4 sparse cells"""
    half = RES[res]
    g = S.golden()
    bs = S.BIN_SIZES[half][k]
    cases = [c for c in S.BIN_FAMILY[half] if c[0] == bs]
    assert len(cases) >= 3
    longest = 0
    for case in cases:
        _, w, h = case
        seq = S.frames(synth, w, h)
        for slot, method, params in S.bin_legs(case, half):
            what = (case, res, slot)
            plan = S.order_plan(w, h, half, bs, params.get("multi_stage", 1))
            assert plan is None or plan["fused"] == (k < 5), (case, plan)
            got, st = _gpu_record(vm, seq, method, half, profile=True, **params)
            want = S.oracle_record(B, synth, w, h, half, method, **params)
            S.assert_same_record(got, want, what)
            _check_path(st, plan, what)
            S.check_bin_slot(g, case, half, slot, got["final"])
            longest = max(longest, len(want["final"]))
    assert longest >= 300, (bs, longest)   # (tests/test_sizes_cpu.py::test_census has every case's count)


# ---- kernel variants at the edges -----------------------------------------------------------------------------------------

VARIANTS = {"fused_features=0": ({"fused_features": 0}, {}), "feat_order=0": ({"feat_order": 0}, {}), "front=0": ({"front": 0}, {}),
            "match_heads=1": ({"match_heads": 1}, {}), "nms_n=2": (None, {"nms_n": 2}), "nms_n=5": (None, {"nms_n": 5})}


@pytest.mark.parametrize("res", list(RES))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_variants_at_the_edges(vm, B, synth, variant, res):
    """every size within 1 px of an edge named in tests/sizes.py - the fused tiles' and the separate kernels' own - through
    the unfused filters and suppression (k_filters, k_nms_fixed), the separate order kernels (k_emit, k_bin_*), the separate
    front end (k_ingest, k_halve), the per-bin head records, and k_nms_tile / k_nms_tile8 (nms_n 2: scales 2 and 6; nms_n 5:
    scales 5 and 10)"""
    half = RES[res]
    options, params = VARIANTS[variant]
    assert len(S.EDGE_SIZES) > 100
    for mw, mh in S.EDGE_SIZES:
        w, h = S.frame(mw, mh, half)
        what = ((mw, mh), res, variant)
        got, st = _gpu_record(vm, S.frames(synth, w, h), 2, half, options=options, profile=True, **params)
        S.assert_same_record(got, S.oracle_record(B, synth, w, h, half, 2, **params), what)
        plan = S.order_plan(w, h, half, 50, 1, params.get("nms_n", 3))
        if variant == "feat_order=0" and plan is not None:
            plan = dict(plan, fused=False)
        _check_path(st, plan, what)
        _check_tiles(st, mw, mh, half, what, nms_n=params.get("nms_n", 3), fused_features=(options or {}).get("fused_features", 1),
                     front=(options or {}).get("front", 1))


# ---- device inputs ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("res", list(RES))
def test_device_inputs_at_every_row_residue(vm, B, synth, res):
    """k_ingest / k_front from a strided view in device memory (row stride w + 7, offset 3): frame widths of every residue
    modulo 16, across a step of the row stride of the matching-resolution image"""
    import torch
    half = RES[res]
    w0, h = (250, 95) if half else (118, 47)
    assert {w % 16 for w in range(w0, w0 + 16)} == set(range(16))
    assert len({S.bpl16(S.matching(w, h, half)[0]) for w in range(w0, w0 + 16)}) == 2
    for w in range(w0, w0 + 16):
        seq = S.frames(synth, w, h)
        views = []
        for l, r in seq:
            big = torch.zeros((2, h, w + 7), dtype=torch.uint8, device="cuda")
            big[0, :, 3:3 + w] = torch.from_numpy(l).cuda()
            big[1, :, 3:3 + w] = torch.from_numpy(r).cuda()
            views.append((big[0, :, 3:3 + w], big[1, :, 3:3 + w]))
        for method in (2, 0):
            got, _ = _gpu_record(vm, views, method, half)
            want = S.oracle_record(B, synth, w, h, half, method)
            S.assert_same_record(got, want, ((w, h), res, "device", method))
            assert len(want["final"]) >= 50


# ---- batched forms ---------------------------------------------------------------------------------------------------------

PAIRS = ((0, 1), (1, 2), (2, 0))


@pytest.mark.parametrize("res", list(RES))
def test_batched_forms(vm, B, synth, res):
    """run_sequence on 3 frames and match_pairs on 3 frames with pairs (0,1), (1,2), (2,0), stereo (6 images) and mono (3),
    at sizes with 1, 2, 3, 4 and 6 dense tiles per image - grids of tiles x images that are no multiple of 8 - against the
    oracle frame by frame / pair by pair"""
    half = RES[res]
    longest = 0
    for mw, mh in S.BATCH_SIZES:
        w, h = S.frame(mw, mh, half)
        seq = S.frames(synth, w, h, 3)
        left, right = np.stack([l for l, _ in seq]), np.stack([r for _, r in seq])
        for method in (2, 0):
            c = B.CpuMatcher("oracle", half_resolution=half, nms_tau=S.TAU)
            want = []
            for l, r in seq:
                c.push_back(l, r if method else None)
                c.match(method)
                want.append(c.matches())
            c.close()
            m = vm.Matcher(half_resolution=half, nms_tau=S.TAU)
            got = m.run_sequence(left, right if method else None, method)
            m.close()
            for f in range(3):
                d = S.first_difference(got[f], want[f])
                assert d is None, ((mw, mh), res, "run_sequence", method, f, d)
            longest = max(longest, len(want[-1]))
            want = []
            for a, b in PAIRS:
                c = B.CpuMatcher("oracle", half_resolution=half, nms_tau=S.TAU)
                for f in (a, b):
                    c.push_back(seq[f][0], seq[f][1] if method else None)
                c.match(method)
                want.append(c.matches())
                c.close()
            m = vm.Matcher(half_resolution=half, nms_tau=S.TAU)
            got = m.match_pairs(left, right if method else None, PAIRS, method)
            m.close()
            for k in range(3):
                d = S.first_difference(got[k], want[k])
                assert d is None, ((mw, mh), res, "match_pairs", method, PAIRS[k], d)
    assert longest >= 300, longest
