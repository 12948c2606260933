"""The frame sizes of tests/sizes.py (every tile and padding edge of the image side) on the CPU: the emulation of the fused
feature tiles (tests/emu/feat_emu.cpp walks csrc/vsm_feat.h's per-thread functions) against the oracle - whole du / dv / f1 / f2
planes and both survivor lists in emission order -, the oracle against the compiled reference (where that build is present)
on features and on the match lists of all three methods, the census of what the frames give, and the oracle against
tests/golden/size_hashes.npz (tests/golden/make_size_hashes.py).  Everything is equality of bytes.
tests/test_sizes_gpu.py runs the HIP path over the same sizes.

The compiled reference takes frames below 19 px (no dense cell; tried once in a child process down to 13 x 13, both
resolutions, all three methods: no feature, matchFeatures returns before it matches), so its leg covers every size."""
import os
import re

import numpy as np
import pytest

import sizes as S
import test_feat_emu as FE
from test_feat_emu import emu  # noqa: F401  (the fixture that builds and loads tests/emu/libfeatemu.so)

CSRC = FE.CSRC
RES = (0, 1)


def _constants(text, struct):
    body = re.search(r"struct %s \{(.*?)\n\};" % struct, text, re.S).group(1)
    return {k: int(v) for k, v in re.findall(r"\b([A-Z][A-Z0-9_]*) = (-?\d+)", body)}


def test_constants_are_the_sources():
    """the constants tests/sizes.py derives its edges from are those of csrc/vsm_feat.h, vsm_internal.h and vsm_order_plan"""
    feat = open(os.path.join(CSRC, "vsm_feat.h")).read()
    for name, mine in (("VfDense", S.DENSE), ("VfSparse", S.SPARSE)):
        theirs = _constants(feat, name)
        assert {k: theirs[k] for k in mine} == mine, name
    internal = open(os.path.join(CSRC, "vsm_internal.h")).read()
    assert int(re.search(r"#define VSM_MARGIN (\d+)", internal).group(1)) == S.MARGIN
    assert int(re.search(r"#define VSM_VSUB (\d+)", internal).group(1)) == S.VSUB
    image = open(os.path.join(CSRC, "vsm_image.hip")).read()
    plan = image[image.index("static bool vsm_order_plan"):image.index("void vsm_launch_ingest")]
    assert int(re.search(r"if\s*\(\s*bw\s*>\s*(\d+)\s*\)\s*return false", plan).group(1)) == S.ORDER_BW_MAX
    assert int(re.search(r"maxcells\s*>\s*(\d+)\s*\)\s*return false", plan).group(1)) == S.ORDER_CELLS_MAX
    assert [int(x) for x in re.search(r"std::min\(\s*(\d+)\s*,\s*(\d+)\s*/\s*bw\s*\)", plan).groups()] == [8, 128]
    lds = re.search(r"return\s+pl\.lds_bytes\s*<=\s*(\d+)\s*\*\s*(\d+)\s*;", plan).groups()
    hist = re.search(r">\s*(\d+)\s*\*\s*(\d+)\s*\)\s*return false", plan).groups()
    assert (int(lds[0]) * int(lds[1]), int(hist[0]) * int(hist[1])) == (S.ORDER_LDS_MAX, S.ORDER_HIST_MAX)
    for k, v in S.UNFUSED.items():
        assert int(re.search(r"#define\s+%s\s+(\d+)" % k, image).group(1)) == v, k
    # cells per tile of the two k_nms_fixed launches: the divisors of the grid and the template arguments agree with UNFUSED
    for n, tcu, tcv in ((3, S.UNFUSED["NMS_TCU"], S.UNFUSED["NMS_TCV"]), (9, S.UNFUSED["NMS8_TC"], S.UNFUSED["NMS8_TC"])):
        m = re.search(r"cdiv\(st\.ncu,\s*(\d+)\)\s*\*\s*cdiv\(st\.ncv,\s*(\d+)\);\s*hipLaunchKernelGGL\(\(k_nms_fixed<%d,\s*(\d+),\s*(\d+)," % n, image)
        assert [int(x) for x in m.groups()] == [tcu, tcv, tcu, tcv], n
    tiles = re.search(r"static void vsm_feat_tiles\(.*?\n\}", image, re.S).group(0)
    nums = [int(x) for x in re.findall(r"-?\d+", re.sub(r"[a-z_]+\.", "", tiles.split("{", 1)[1]))]
    D = S.DENSE
    tw, th = 8 * D["PC_OWN"], D["ROWS"] * D["PR_OWN"]
    assert nums == [-D["FX"], tw - 1, tw, -D["CELL_U0"], D["CU"] - 1, D["CU"], -D["FY"], th - 1, th, -D["CELL_V0"], D["CV"] - 1, D["CV"]], nums
    assert S.cells is not FE.cells and all(S.cells(x, n) == FE.cells(x, n) for x in range(0, 400) for n in (2, 3, 5, 6, 9, 10))


def test_frames_are_the_generator_s(synth):
    for w, h in ((13, 13), (333, 101), (653, 201)):
        want = synth.stereo_sequence(S.SEED, w, h, S.N_FRAMES, **S.FRAME_KW)
        for (l, r), (wl, wr) in zip(S.frames(synth, w, h), want):
            assert l.tobytes() == wl.tobytes() and r.tobytes() == wr.tobytes(), (w, h)


def _planes(B, l, half):
    h, w = l.shape
    img = B.pad_image(l)
    return np.ascontiguousarray(B.half_image("oracle", img, w) if half else img)


@pytest.mark.parametrize("half", RES)
@pytest.mark.parametrize("family", list(S.FAMILIES))
def test_emulation_vs_oracle(emu, B, synth, family, half):  # noqa: F811
    """whole planes (pad columns included) and the survivors of both scales in the reference's emission order"""
    for mw, mh in S.FAMILIES[family]:
        w, h = S.frame(mw, mh, half)
        mimg = _planes(B, S.frames(synth, w, h, 1)[0][0], half)
        mbpl = mimg.shape[1]
        assert mimg.shape == (mh, S.bpl16(mw))
        what = ((mw, mh), "half" if half else "full")
        want = dict(zip(("du", "dv"), B.sobel5x5("oracle", mimg)), f1=B.blob5x5("oracle", mimg), f2=B.checkerboard5x5("oracle", mimg))
        got = dict(du=np.full((mh, mbpl), 77, np.uint8), dv=np.full((mh, mbpl), 77, np.uint8),
                   f1=np.full((mh, mbpl), 777, np.int16), f2=np.full((mh, mbpl), 777, np.int16))
        ncu, ncv = S.cells(mw, 3), S.cells(mh, 3)
        cand = np.full(max(ncu * ncv, 1) * 4, 12345, np.int32)
        emu.emu_feat_dense(FE.ptr(mimg), mw, mh, mbpl, S.TAU, ncu, ncv, *[FE.ptr(got[k]) for k in ("du", "dv", "f1", "f2")], FE.ptr(cand))
        for k in got:
            if got[k].tobytes() != want[k].tobytes():
                y, x = np.argwhere(got[k] != want[k])[0]
                raise AssertionError((what, k, (int(x), int(y)), int(got[k][y, x]), int(want[k][y, x])))
        for n, fn in ((3, None), (9, emu.emu_feat_sparse)):
            nu, nv = S.cells(mw, n), S.cells(mh, n)
            lst = [tuple(int(x) for x in (r[0], r[1], r[3])) for r in B.nms("oracle", want["f1"], want["f2"], mw, n, S.TAU)]
            if n == 9:
                cand = np.full(max(nu * nv, 1) * 4, 12345, np.int32)
                if nu * nv > 0:
                    fn(FE.ptr(mimg), mw, mh, mbpl, S.TAU, nu, nv, FE.ptr(cand))
            mine = FE.cand_list(cand, nu, nv) if nu * nv > 0 else []
            if mine != lst:
                i = next((i for i, (a, b) in enumerate(zip(mine, lst)) if a != b), min(len(mine), len(lst)))
                raise AssertionError((what, "survivors", n, i, mine[i:i + 1], lst[i:i + 1], len(mine), len(lst)))


def _records(B, synth, mw, mh, half, kind):
    """[(slot of tests/sizes.py, array)] of one size from the oracle or the reference"""
    w, h = S.frame(mw, mh, half)

    def run(method, **params):
        if kind == "oracle":
            return S.oracle_record(B, synth, w, h, half, method, **params)
        c = B.CpuMatcher("ref", half_resolution=half, nms_tau=S.TAU, **params)
        rec = S.record(c, S.frames(synth, w, h), method)
        c.close()
        return rec
    rec = {m: run(m) for m in (2, 0, 1)}
    if S.small(mw, mh):
        rec.update({(m, 0): run(m, multi_stage=0) for m in (2, 0)})
    return rec


@pytest.mark.parametrize("half", RES)
@pytest.mark.parametrize("family", list(S.FAMILIES))
def test_oracle_vs_reference(B, synth, have_ref, family, half):
    """features of all four sets, match()'s value, the five stages and the final lists of quad, flow and stereo matching;
    the small frames with multi_stage = 0 too"""
    if not have_ref:
        pytest.skip("the compiled reference is not here")
    for mw, mh in S.FAMILIES[family]:
        want, got = _records(B, synth, mw, mh, half, "ref"), _records(B, synth, mw, mh, half, "oracle")
        for k in want:
            S.assert_same_record(got[k], want[k], ((mw, mh), "half" if half else "full", k))


@pytest.mark.parametrize("half", RES)
def test_oracle_vs_reference_bin_families(B, synth, have_ref, half):
    if not have_ref:
        pytest.skip("the compiled reference is not here")
    for case in S.BIN_FAMILY[half]:
        _, w, h = case
        for slot, m, params in S.bin_legs(case, half):
            c = B.CpuMatcher("ref", half_resolution=half, nms_tau=S.TAU, **params)
            want = S.record(c, S.frames(synth, w, h), m)
            c.close()
            S.assert_same_record(S.oracle_record(B, synth, w, h, half, m, **params), want, (case, "half" if half else "full", slot))


@pytest.mark.parametrize("half", RES)
def test_oracle_vs_size_hashes(B, synth, half):
    g = S.golden()
    for mw, mh in S.ALL_SIZES:
        rec = _records(B, synth, mw, mh, half, "oracle")
        for s in S.SETS:
            S.check_slot(g, mw, mh, half, s, rec[2]["feats"][s])
        for m in (2, 0, 1):
            S.check_slot(g, mw, mh, half, f"final m{m}", rec[m]["final"])
        for m in (2, 0):
            if (m, 0) in rec:
                S.check_slot(g, mw, mh, half, f"final m{m} ms0", rec[(m, 0)]["final"])
            else:
                assert int(g["counts"][S.INDEX[(mw, mh)], half, S.SLOTS.index(f"final m{m} ms0")]) == 0
    for case in S.BIN_FAMILY[half]:
        legs = S.bin_legs(case, half)
        for slot, m, params in legs:
            S.check_bin_slot(g, case, half, slot, S.oracle_record(B, synth, case[1], case[2], half, m, **params)["final"])
        for slot in set(S.BIN_SLOTS) - {x[0] for x in legs}:
            assert int(g[f"bin_counts{half}"][S.BIN_INDEX[half][case], S.BIN_SLOTS.index(slot)]) == 0


# Sizes with at least 8 sparse features in the current left image whose final list is shorter than 50: narrow frames, 31 - 54 px
# wide, where the disparity (6 px + 1 px per 6 rows) takes up to a third of the width away from the overlap of the two images
# and the sparse grid has 5 - 10 cells, so that few features close the circle of quad matching.
# (size, resolution): (sparse features, quad matches, flow matches).
SHORT_LISTS = {((31, 71), 0): (9, 11, 49), ((31, 71), 1): (9, 3, 63), ((32, 71), 1): (8, 2, 59), ((33, 71), 1): (8, 2, 59),
               ((41, 71), 0): (10, 30, 76), ((41, 71), 1): (13, 35, 90), ((42, 71), 0): (10, 30, 76), ((42, 71), 1): (12, 34, 87),
               ((43, 71), 0): (10, 42, 92), ((44, 71), 0): (10, 41, 91), ((45, 71), 0): (10, 41, 91), ((46, 71), 0): (10, 41, 91),
               ((46, 71), 1): (10, 40, 107), ((47, 71), 1): (10, 47, 127), ((48, 71), 1): (10, 45, 124), ((49, 71), 1): (10, 45, 122),
               ((50, 71), 1): (10, 45, 122), ((51, 47), 0): (9, 47, 72), ((52, 47), 0): (8, 45, 70), ((53, 47), 0): (8, 45, 70),
               ((54, 47), 0): (8, 45, 70)}


# The cases of the bin families whose quad, flow or stereo list is shorter than 40: the frames one below, at and one above one
# and two search bins of 15 - 50 px, which have no sparse cell (matching-resolution width below 31: nothing matches with
# multi_stage = 1) or a single column of them.  (resolution, binsize, frame width): (quad, flow, stereo, quad and flow with
# multi_stage = 0 - run where the frame has fewer than 4 sparse cells, 0 elsewhere).
BIN_SHORT_LISTS = {(0, 15, 14): (0, 0, 0, 0, 0), (0, 15, 15): (0, 0, 0, 0, 0), (0, 15, 16): (0, 0, 0, 0, 0), (0, 15, 29): (0, 0, 0, 9, 33),
                   (0, 15, 30): (0, 0, 0, 9, 33), (0, 15, 31): (12, 47, 19, 0, 0), (0, 31, 30): (0, 0, 0, 9, 33),
                   (0, 31, 31): (12, 52, 20, 0, 0), (0, 31, 32): (13, 49, 21, 0, 0),
                   (1, 30, 29): (0, 0, 0, 0, 0), (1, 30, 30): (0, 0, 0, 0, 0), (1, 30, 31): (0, 0, 0, 0, 0), (1, 30, 59): (0, 0, 0, 4, 51),
                   (1, 30, 60): (0, 0, 0, 4, 51), (1, 30, 61): (0, 0, 0, 4, 51), (1, 50, 49): (0, 0, 0, 1, 32), (1, 50, 50): (0, 0, 0, 1, 33),
                   (1, 50, 51): (0, 0, 0, 1, 33)}


def test_census(B, synth):
    """what the frames give, from the oracle (seed 33, nms_tau 20):
      - every size whose grid has at least 4 cells at a scale gives at least one feature at that scale;
      - every size with at least 8 sparse features gives at least 50 matches in quad and in flow matching - but for the 21
        narrow frames of SHORT_LISTS (of 1728 size-resolutions), whose counts are pinned here (the shortest lists: 2 quad
        matches, 49 flow matches); every such size gives a list that is not empty;
      - the bin families give at least 40 matches with every method and bin size (measured: 47 .. 873) - but for the 18
        cases of BIN_SHORT_LISTS (of 135), frames of one or two small search bins, whose counts are pinned here;
      - of the small frames (fewer than 4 sparse cells) at least four fifths reach a match list with multi_stage = 0
        (measured: 586 of 666), so the dense bin order of frames without sparse features is seen"""
    short, ms0 = {}, []
    for mw, mh in S.ALL_SIZES:
        for half in RES:
            rec = _records(B, synth, mw, mh, half, "oracle")
            f = rec[2]["feats"]
            for n, s in ((9, "1c1"), (3, "1c2")):
                if S.cells(mw, n) * S.cells(mh, n) >= 4:
                    assert len(f[s]) >= 1 and len(f["2" + s[1:]]) >= 1, ((mw, mh), half, s)
            if len(f["1c1"]) >= 8:
                n2, n0 = len(rec[2]["final"]), len(rec[0]["final"])
                assert n2 >= 1 and n0 >= 1
                if min(n2, n0) < 50:
                    short[((mw, mh), half)] = (len(f["1c1"]), n2, n0)
            if (2, 0) in rec:
                ms0.append(len(rec[(2, 0)]["final"]) > 0)
    assert short == SHORT_LISTS, short
    assert len(ms0) > 600 and sum(ms0) >= 0.8 * len(ms0), (sum(ms0), len(ms0))
    short = {}
    for half in RES:
        for case in S.BIN_FAMILY[half]:
            n = dict.fromkeys(S.BIN_SLOTS, 0)
            for slot, m, params in S.bin_legs(case, half):
                n[slot] = len(S.oracle_record(B, synth, case[1], case[2], half, m, **params)["final"])
            if min(n[slot] for slot in S.BIN_SLOTS[:3]) < 40:
                short[(half, case[0], case[1])] = tuple(n[slot] for slot in S.BIN_SLOTS)
    assert short == BIN_SHORT_LISTS, short
