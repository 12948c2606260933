"""Frame sizes at every tile and padding edge of the image side (csrc/vsm_image.hip, csrc/vsm_feat.h), shared by
tests/test_sizes_cpu.py and tests/test_sizes_gpu.py.

A size is (mw, mh) in MATCHING-resolution pixels; frame(mw, mh, half) is the frame that gives it: (mw, mh) itself at full
resolution, (2 mw + (mw & 1), 2 mh + (mh & 1)) at half resolution, so that odd and even frames both occur.

Every number below is derived from the constants of the code under test (copied here; tests/test_sizes_cpu.py reads them
back out of the sources) and asserted at import:

  row padding     bpl = w rounded up to 16 (bpl16); the filters run over the image as one byte stream, so at w % 16 == 0 a tap
                  that leaves a row reads the neighbouring row's pixels and at every other residue zeros.  The width family
                  runs from 13 to 172 without a gap: all residues occur many times (asserted).
  cell counts     cells(len, n) = ceil((len - 2 n - 2 MARGIN) / (n + 1)): the k-th cell appears at len = 2 n + 2 MARGIN + 1 +
                  (k - 1)(n + 1): 19 (dense, n = 3) and 31 (sparse, n = 9).
  dense tile      VfDense owns image cells (CU tx + CELL_U0 + c, CV ty + CELL_V0 + r): tile column 0 holds CU + CELL_U0 = 29
                  cell columns, the 30th needs width 135; tile row 0 holds CV + CELL_V0 = 10 cell rows, the 11th needs height
                  59.  The tile also owns du / dv of PC_OWN x PR_OWN patches from (FX, FY) on: a second tile column is
                  LAUNCHED (for the planes alone) once mbpl - FX > 8 PC_OWN, i.e. mbpl = 128, width 113, and a second tile row
                  once mh - FY > ROWS PR_OWN, height 45.
  sparse tile     VfSparse owns CU x CV = 16 x 4 cells: the 17th cell column needs width 191, the 5th cell row height 71.
  clipped form    vf_nms_item<.., fast> is the clipped one in every tile whose windows meet (w - 1 - MARGIN, h - 1 - MARGIN):
                  which tiles those are changes with every pixel, hence whole ranges and not single values.
  separate        the kernels behind the options fused_features / feat_order / front = 0 and behind other radii have tiles
  kernels         of their own (UNFUSED): the first cell or pixel beyond one is derived the same way - widths 47, 53, 65, 71,
                  77, 83 and 147, heights 33, 41, 47, 51, 53 and 77 - and lies inside the families too.
  record order    order_plan() restates vsm_order_plan (vsm_image.hip): tiles of bu = min(8, 128 / bw) whole search bins,
                  bw = ceil(binsize / scale) + 1; the separate kernels at bw > 72 or more than 512 cells per tile.
"""
import numpy as np

# ---- constants of the code under test (test_sizes_cpu.py::test_constants_are_the_sources checks them against the sources) ----
MARGIN = 6      # VSM_MARGIN, csrc/vsm_internal.h
VSUB = 5        # VSM_VSUB
DENSE = dict(N=3, ROWS=4, TW=128, TH=48, PC_OWN=16, PR_OWN=12, FX=-8, FY=-4, CU=32, CV=12, CELL_U0=-3, CELL_V0=-2)   # VfDense
SPARSE = dict(N=9, ROWS=6, TW=160, TH=40, FX=4, FY=6, CU=16, CV=4, CELL_U0=0, CELL_V0=0)                            # VfSparse
ORDER_BW_MAX, ORDER_CELLS_MAX, ORDER_LDS_MAX, ORDER_HIST_MAX = 72, 512, 64 * 1024, 150 * 1024   # vsm_order_plan
# tiles of the separate kernels (vsm_image.hip), which the options fused_features / feat_order / front = 0 and other radii select:
# cells per tile of k_nms_fixed<3> and k_nms_tile (16 x 8), k_nms_fixed<9> and k_nms_tile8 (4 x 4), pixels per tile of k_emit and k_front
UNFUSED = dict(NMS_TCU=16, NMS_TCV=8, NMS8_TC=4, EMIT_TW=128, EMIT_TH=32, FRONT_TW=128, FRONT_TH=64)

SEED, TAU, N_FRAMES = 33, 20, 2
FRAME_KW = dict(disparity=6, ramp=(1, 6))
SETS = ("1c1", "1c2", "2c1", "2c2")


def cdiv(a, b):
    return -(-a // b)


def bpl16(w):
    return (w + 15) & ~15


def cells(length, n, margin=MARGIN):
    """loop count of `for (i = n + margin; i < length - n - margin; i += n + 1)`"""
    span = length - 2 * n - 2 * margin
    return cdiv(span, n + 1) if span > 0 else 0


def first_length_with_cells(k, n):
    return 2 * n + 2 * MARGIN + 1 + (k - 1) * (n + 1)


def sparse_n(nms_n):
    """viso/matcher.cpp:685-687"""
    ns = 3 * nms_n
    return ns if ns <= 10 else (nms_n if nms_n > 10 else 10)


def frame(mw, mh, half):
    return (2 * mw + (mw & 1), 2 * mh + (mh & 1)) if half else (mw, mh)


def matching(w, h, half):
    return (w // 2, h // 2) if half else (w, h)


def dense_tiles(mw, mh):
    """vsm_feat_tiles: tiles of k_feat_dense per image"""
    D = DENSE
    return (max(cdiv(bpl16(mw) - D["FX"], 8 * D["PC_OWN"]), cdiv(cells(mw, 3) - D["CELL_U0"], D["CU"])),
            max(cdiv(mh - D["FY"], D["ROWS"] * D["PR_OWN"]), cdiv(cells(mh, 3) - D["CELL_V0"], D["CV"])))


def sparse_tiles(mw, mh):
    return cdiv(cells(mw, 9), SPARSE["CU"]), cdiv(cells(mh, 9), SPARSE["CV"])


def fused_tiles(mw, mh, multi_stage=1, nms_n=3):
    """vsm_launch_features' rule: k_feat_dense (and, with multi_stage, k_feat_sparse) serve the default radii where the dense
    grid has a cell and - with multi_stage - the sparse one too; every other frame takes k_filters + k_nms*"""
    return nms_n == 3 and cells(mw, 3) * cells(mh, 3) > 0 and (not multi_stage or cells(mw, 9) * cells(mh, 9) > 0)


def order_plan(w, h, half, binsize, multi_stage=1, nms_n=3):
    """vsm_order_plan's rule for a frame: None where no set has a cell (neither form runs), else a dict with `fused`
    (k_feat_scan + k_feat_order; False: k_scan_cells + k_emit + k_bin_*), bu, bw, tiles_u, tiles_v, last (search bins in the
    last tile of a tile row), cells (the largest number of suppression cells meeting a tile)"""
    scale = 2 if half else 1
    mw, mh = matching(w, h, half)
    ub, vb = cdiv(w, binsize), cdiv(h, binsize)
    nn = (sparse_n(nms_n), nms_n)
    ncu, ncv = [cells(mw, n) for n in nn], [cells(mh, n) for n in nn]
    if max(ncu[k] * ncv[k] for k in range(2)) <= 0:
        return None
    bw = cdiv(binsize, scale) + 1
    bu = max(1, min(8, 128 // bw))
    out = dict(fused=False, bu=bu, bw=bw, tiles_u=cdiv(ub, bu), tiles_v=vb, last=ub - (cdiv(ub, bu) - 1) * bu, cells=0)
    if 4 * ub * vb * VSUB * 4 > ORDER_HIST_MAX or bw > ORDER_BW_MAX:
        return out
    maxcells = maxl = 0
    for k in range(0 if multi_stage else 1, 2):
        if ncu[k] * ncv[k] <= 0:
            continue
        n1 = nn[k] + 1
        cwt, cht, cwb = min(ncu[k], (bu * bw - 1) // n1 + 2), min(ncv[k], (bw - 1) // n1 + 2), min(ncu[k], (bw - 1) // n1 + 2)
        maxcells, maxl = max(maxcells, cwt * cht), max(maxl, (cwb * cht + 3) & ~3)
        if max(4 * ncu[k] * ncv[k], 4) >= 1 << 21:
            return out
    out["cells"] = maxcells
    if maxcells <= 0 or maxcells > ORDER_CELLS_MAX:
        return out
    o = ((bu * bw + 13 + 3) & ~3) * (bw + 10) * 2
    for nbytes in (maxcells * 16, 2 * bu * 4 * (VSUB + 1) * 4, (bu * 4 + 1) * 4, bu * 4 * maxl * 4, maxcells * 4 * 4):
        o = ((o + 15) & ~15) + nbytes
    out["fused"] = ((o + 15) & ~15) <= ORDER_LDS_MAX
    return out


# ---- the edges, derived ----------------------------------------------------------------------------------------------------
DENSE_CELL = first_length_with_cells(1, DENSE["N"])                                        # 19: the first dense cell
SPARSE_CELL = first_length_with_cells(1, SPARSE["N"])                                      # 31: the first sparse cell
DENSE_TILE_U = first_length_with_cells(DENSE["CU"] + DENSE["CELL_U0"] + 1, DENSE["N"])     # 135: a cell in dense tile column 1
DENSE_TILE_V = first_length_with_cells(DENSE["CV"] + DENSE["CELL_V0"] + 1, DENSE["N"])     # 59: a cell in dense tile row 1
SPARSE_TILE_U = first_length_with_cells(SPARSE["CU"] + 1, SPARSE["N"])                     # 191
SPARSE_TILE_V = first_length_with_cells(SPARSE["CV"] + 1, SPARSE["N"])                     # 71
DENSE_PLANES_U = bpl16(8 * DENSE["PC_OWN"] + DENSE["FX"] + 1) - 15   # 113: the first width whose bpl (128) exceeds tile column 0's 120 columns
DENSE_PLANES_V = DENSE["ROWS"] * DENSE["PR_OWN"] + DENSE["FY"] + 1                         # 45: the first row of tile row 1
assert (DENSE_CELL, SPARSE_CELL, DENSE_TILE_U, DENSE_TILE_V, SPARSE_TILE_U, SPARSE_TILE_V) == (19, 31, 135, 59, 191, 71)
assert (DENSE_PLANES_U, DENSE_PLANES_V) == (113, 45)
# the two facts behind them: the width at which a tile column appears, and the cell counts
assert [cells(x, 3) for x in (18, 19, 22, 23, 134, 135)] == [0, 1, 1, 2, 29, 30]
assert [cells(x, 9) for x in (30, 31, 40, 41, 190, 191)] == [0, 1, 1, 2, 16, 17]
assert [dense_tiles(x, 47)[0] for x in (112, 113, 134, 135)] == [1, 2, 2, 2] and dense_tiles(135, 47)[0] == cdiv(30 + 3, 32)
assert cdiv(cells(134, 3) - DENSE["CELL_U0"], DENSE["CU"]) == 1 and cdiv(cells(135, 3) - DENSE["CELL_U0"], DENSE["CU"]) == 2
assert [dense_tiles(37, y)[1] for y in (44, 45, 58, 59)] == [1, 2, 2, 2] and cdiv(cells(58, 3) + 2, 12) == 1 and cdiv(cells(59, 3) + 2, 12) == 2
assert [sparse_tiles(x, 47)[0] for x in (30, 31, 190, 191)] == [0, 1, 1, 2] and [sparse_tiles(37, y)[1] for y in (70, 71)] == [1, 2]
assert [bpl16(x) for x in (1, 16, 17, 112, 113, 128, 129)] == [16, 16, 32, 112, 128, 128, 144]

WIDTH_EDGES = {"first dense cell column": DENSE_CELL, "first sparse cell column": SPARSE_CELL,
               "dense tile column 1, planes": DENSE_PLANES_U, "dense tile column 1, cells": DENSE_TILE_U,
               "sparse tile column 1": SPARSE_TILE_U}
HEIGHT_EDGES = {"first dense cell row": DENSE_CELL, "first sparse cell row": SPARSE_CELL, "dense tile row 1, planes": DENSE_PLANES_V,
                "dense tile row 1, cells": DENSE_TILE_V, "sparse tile row 1": SPARSE_TILE_V}
# the same for the separate kernels: the first cell beyond a tile of NMS_TCU x NMS_TCV cells (k_nms_fixed<3>; k_nms_tile at
# nms_n = 2), of NMS8_TC x NMS8_TC cells (k_nms_fixed<9>; k_nms_tile8 at the scales 5, 6 and 10 that nms_n = 2 and 5 give), of
# EMIT_TW / 4 x EMIT_TH / 4 dense cells (k_emit), and the first half-resolution frame beyond one k_front tile
_U = UNFUSED
UNFUSED_WIDTH_EDGES = {"k_nms_fixed<3> tile column 1": first_length_with_cells(_U["NMS_TCU"] + 1, 3),
                       "k_nms_fixed<9> tile column 1": first_length_with_cells(_U["NMS8_TC"] + 1, 9),
                       "k_nms_tile tile column 1, n = 2": first_length_with_cells(_U["NMS_TCU"] + 1, 2),
                       "k_emit tile column 1": first_length_with_cells(_U["EMIT_TW"] // 4 + 1, 3),
                       "k_front tile column 1, half resolution": _U["FRONT_TW"] // 2 + 1}
UNFUSED_WIDTH_EDGES.update({f"k_nms_tile8 tile column 1, n = {n}": first_length_with_cells(_U["NMS8_TC"] + 1, n) for n in (5, 6, 10)})
UNFUSED_HEIGHT_EDGES = {"k_nms_fixed<3> tile row 1": first_length_with_cells(_U["NMS_TCV"] + 1, 3),
                        "k_nms_tile tile row 1, n = 2": first_length_with_cells(_U["NMS_TCV"] + 1, 2),
                        "k_emit tile row 1": first_length_with_cells(_U["EMIT_TH"] // 4 + 1, 3),
                        "k_front tile row 1, half resolution": _U["FRONT_TH"] // 2 + 1}
UNFUSED_HEIGHT_EDGES.update({f"k_nms_tile8 tile row 1, n = {n}": first_length_with_cells(_U["NMS8_TC"] + 1, n) for n in (5, 6, 10)})
assert sorted(UNFUSED_WIDTH_EDGES.values()) == [47, 53, 65, 65, 71, 77, 83, 147], UNFUSED_WIDTH_EDGES
assert sorted(UNFUSED_HEIGHT_EDGES.values()) == [33, 41, 47, 51, 51, 53, 77], UNFUSED_HEIGHT_EDGES
assert bpl16(frame(64, 1, 1)[0]) == 128 and bpl16(frame(65, 1, 1)[0]) > 128 and frame(32, 32, 1)[1] == 64 and frame(33, 33, 1)[1] > 64
ALL_WIDTH_EDGES = sorted(set(WIDTH_EDGES.values()) | set(UNFUSED_WIDTH_EDGES.values()))
ALL_HEIGHT_EDGES = sorted(set(HEIGHT_EDGES.values()) | set(UNFUSED_HEIGHT_EDGES.values()))
NO_PAD_WIDTHS = (32, 128, 160, 192, 256, 320)   # w % 16 == 0: no pad byte; below, at and above one / two tile widths of both tiles

# ---- width and height families ---------------------------------------------------------------------------------------------
WIDTH_RANGES = ((13, 44), (45, 74), (75, 104), (105, 117), (118, 140), (141, 149), (150, 172), (184, 196), (250, 268), (312, 326))
WIDTH_CROSS = (21, 47, 71)
HEIGHT_RANGES = ((13, 44), (45, 62), (66, 74), (76, 100))
HEIGHT_CROSS = (37, 131, 191)
assert {x % 16 for lo, hi in WIDTH_RANGES for x in range(lo, hi + 1)} == set(range(16))
for _e in ALL_WIDTH_EDGES + list(NO_PAD_WIDTHS):
    assert all(any(lo <= _e + d <= hi for lo, hi in WIDTH_RANGES) for d in (-1, 0, 1)), _e
for _e in ALL_HEIGHT_EDGES:
    assert all(any(lo <= _e + d <= hi for lo, hi in HEIGHT_RANGES) for d in (-1, 0, 1)), _e


def _name(lo, hi):
    return f"{lo}-{hi}"


FAMILIES = {}
for _lo, _hi in WIDTH_RANGES:
    FAMILIES["w" + _name(_lo, _hi)] = [(x, y) for x in range(_lo, _hi + 1) for y in WIDTH_CROSS]
for _lo, _hi in HEIGHT_RANGES:
    FAMILIES["h" + _name(_lo, _hi)] = [(x, y) for y in range(_lo, _hi + 1) for x in HEIGHT_CROSS]
ALL_SIZES = sorted({s for f in FAMILIES.values() for s in f})
INDEX = {s: i for i, s in enumerate(ALL_SIZES)}


def _near(x, edges):
    return any(abs(x - e) <= 1 for e in edges)


# the fixed subset for the kernel variants: every size of a family whose SWEPT coordinate is within 1 px of an edge named above
# (the crossed coordinates 71 and 191 are edges themselves: counting them would take in whole families)
EDGE_SIZES = sorted({(x, y) for name, f in FAMILIES.items() for x, y in f
                     if (_near(x, ALL_WIDTH_EDGES + list(NO_PAD_WIDTHS)) if name[0] == "w" else _near(y, ALL_HEIGHT_EDGES))})


def small(mw, mh):
    """fewer than 4 sparse cells: with multi_stage = 1 such a frame matches little or nothing, so its dense bin order reaches a
    match list only through a second leg with multi_stage = 0"""
    return cells(mw, 9) * cells(mh, 9) < 4


# about a dozen sizes with 1, 2 and 3 dense tiles per image (and 0, 1 or 2 sparse ones): with 3 (mono) or 6 (stereo) images per
# call tiles * n_img is no multiple of 8, so the grids' rounding to 8 and the remapping over the XCDs leave idle blocks
BATCH_SIZES = [(37, 21), (44, 44), (111, 40), (112, 44), (113, 21), (131, 44), (135, 47), (37, 45), (37, 59), (37, 100), (191, 21),
               (131, 100), (196, 71)]
assert {dense_tiles(*s)[0] * dense_tiles(*s)[1] for s in BATCH_SIZES} >= {1, 2, 3}
assert all((dense_tiles(*s)[0] * dense_tiles(*s)[1] * 3) % 8 for s in BATCH_SIZES if dense_tiles(*s)[0] * dense_tiles(*s)[1] < 8)

# ---- bin families: (match_binsize, frame width, frame height) per resolution ------------------------------------------------
# bw = ceil(binsize / scale) + 1, bu = min(8, 128 / bw): binsizes with bu = 8, 4, 2 and 1, and one on each side of bw = 72
BIN_SIZES = {0: (15, 31, 50, 66, 71, 72), 1: (30, 50, 100, 130, 142, 144)}
BIN_HEIGHT = {0: 75, 1: 151}
BIN_MAX_W = 420     # a group of three widths stays whole: it is dropped if its widest frame is wider than this


def bin_widths(binsize, half):
    """one below, at and one above k, k bu and k bu - 1 bins (k = 1, 2): the last tile of a tile row holds 1, bu - 1 and bu bins"""
    p = order_plan(400, BIN_HEIGHT[half], half, binsize)
    bu = p["bu"]
    base = {k * m * binsize for k in (1, 2) for m in (1, bu, max(bu - 1, 1))} | {(k * bu - 1) * binsize for k in (1, 2) if k * bu > 1}
    return sorted({b + d for b in base if b + 1 <= BIN_MAX_W for d in (-1, 0, 1)})


BIN_FAMILY = {half: [(bs, w, BIN_HEIGHT[half]) for bs in BIN_SIZES[half] for w in bin_widths(bs, half)] for half in (0, 1)}
BIN_INDEX = {half: {c: i for i, c in enumerate(BIN_FAMILY[half])} for half in (0, 1)}
for _half in (0, 1):
    _plans = {bs: order_plan(300, BIN_HEIGHT[_half], _half, bs) for bs in BIN_SIZES[_half]}
    assert [p["bu"] for p in _plans.values()] == [8, 4, 2, 1, 1, 1], _plans
    assert [p["bw"] for p in _plans.values()][-2:] == [72, 73] and [p["fused"] for p in _plans.values()] == [True] * 5 + [False]
    for _bs in BIN_SIZES[_half]:
        _last = {p["last"] for p in (order_plan(w, h, _half, b) for b, w, h in BIN_FAMILY[_half] if b == _bs) if p is not None}
        _bu = _plans[_bs]["bu"]
        assert {1, _bu, max(_bu - 1, 1)} <= _last, (_half, _bs, _last)


# ---- frames ---------------------------------------------------------------------------------------------------------------
_CANVAS = {}


def frames(synth, w, h, n=N_FRAMES):
    """synth.stereo_sequence(SEED, w, h, n, disparity=6, ramp=(1, 6)): the canvas is a function of absolute pixel positions
    alone, so one canvas serves every size (test_sizes_cpu.py::test_frames_are_the_generator_s compares)"""
    if "cv" not in _CANVAS:
        _CANVAS["cv"] = synth.canvas(SEED, 704, 256)
    cv = _CANVAS["cv"]
    assert w <= 704 and h <= 256
    return [synth.stereo_frame(cv, f, w, h, FRAME_KW["disparity"], FRAME_KW["ramp"]) for f in range(n)]


# ---- records ---------------------------------------------------------------------------------------------------------------
def record(m, seq, method):
    """what a matcher with the CpuMatcher face gives after the last frame of seq: the four feature sets, match()'s value, the
    five stages (when matching ran) and the final list"""
    for l, r in seq:
        assert m.push_back(l, r if method else None) in (0, None)
        ran = bool(m.match(method))
    return dict(feats={s: m.features(s) for s in SETS}, ran=ran, stages=[m.stage(s) for s in range(5)] if ran else None,
                final=m.matches())


_ORACLE = {}


def oracle_record(B, synth, w, h, half, method, **params):
    """the oracle's record of one frame size, computed once per session and left unchanged"""
    key = (w, h, half, method, tuple(sorted(params.items())))
    if key not in _ORACLE:
        c = B.CpuMatcher("oracle", half_resolution=half, nms_tau=TAU, **params)
        _ORACLE[key] = record(c, frames(synth, w, h), method)
        c.close()
    return _ORACLE[key]


def first_difference(a, b):
    """None if the arrays hold the same bytes, else (index of the first differing record, got, want) - lengths if only they differ"""
    if a.shape == b.shape and a.tobytes() == b.tobytes():
        return None
    n = min(len(a), len(b))
    ra, rb = a.reshape(len(a), -1) if a.dtype.names is None else a, b.reshape(len(b), -1) if b.dtype.names is None else b
    for i in range(n):
        if ra[i].tobytes() != rb[i].tobytes():
            return (i, ra[i].tolist() if a.dtype.names is None else ra[i].item(), rb[i].tolist() if b.dtype.names is None else rb[i].item())
    return ("length", len(a), len(b))


def assert_same_record(got, want, what, stages=True):
    for s in SETS:
        d = first_difference(got["feats"][s], want["feats"][s])
        assert d is None, (what, s, d)
    assert got["ran"] == want["ran"], (what, "match()", got["ran"], want["ran"])
    if want["ran"] and stages and got["stages"] is not None:
        for s in range(5):
            d = first_difference(got["stages"][s], want["stages"][s])
            assert d is None, (what, "stage", s, d)
    d = first_difference(got["final"], want["final"])
    assert d is None, (what, "final", d)


# ---- tests/golden/size_hashes.npz -------------------------------------------------------------------------------------------
# per (size, resolution): the four feature sets after the second frame (quad matching), the final lists of methods 2, 0 and 1,
# and the final lists of methods 2 and 0 with multi_stage = 0 (small() sizes only; zeros elsewhere)
SLOTS = ("1c1", "1c2", "2c1", "2c2", "final m2", "final m0", "final m1", "final m2 ms0", "final m0 ms0")
BIN_SLOTS = ("final m2", "final m0", "final m1", "final m2 ms0", "final m0 ms0")   # (the last two: small() frames only)


def bin_legs(case, half):
    """[(slot, method, parameters)] of one case of the bin families: the three methods, and for frames with fewer than 4 sparse
    cells quad and flow matching with multi_stage = 0 (their dense bin order reaches no match list otherwise)"""
    bs, w, h = case
    legs = [(f"final m{m}", m, dict(match_binsize=bs)) for m in (2, 0, 1)]
    if small(*matching(w, h, half)):
        legs += [(f"final m{m} ms0", m, dict(match_binsize=bs, multi_stage=0)) for m in (2, 0)]
    return legs


def digest(a):
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


_GOLDEN = {}


def golden():
    """tests/golden/size_hashes.npz as a dict of arrays, read once and checked against the families above"""
    if not _GOLDEN:
        import os
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "size_hashes.npz"), allow_pickle=False) as z:
            _GOLDEN.update({k: z[k] for k in z.files})
        check_golden_inputs(_GOLDEN)
    return _GOLDEN


def check_golden_inputs(g):
    """tests/golden/size_hashes.npz was written for these families, this seed and these parameters"""
    assert np.array_equal(g["sizes"], np.array(ALL_SIZES)) and (int(g["seed"]), int(g["tau"])) == (SEED, TAU)
    assert tuple(str(s) for s in g["slots"]) == SLOTS and tuple(str(s) for s in g["bin_slots"]) == BIN_SLOTS
    for half in (0, 1):
        assert np.array_equal(g[f"bins{half}"], np.array(BIN_FAMILY[half]))


def check_slot(g, mw, mh, half, slot, a):
    i, k = INDEX[(mw, mh)], SLOTS.index(slot)
    assert len(a) == int(g["counts"][i, half, k]), ((mw, mh), half, slot, len(a), int(g["counts"][i, half, k]))
    assert np.array_equal(digest(a), g["digests"][i, half, k]), ((mw, mh), half, slot)


def check_bin_slot(g, case, half, slot, a):
    i, k = BIN_INDEX[half][case], BIN_SLOTS.index(slot)
    assert len(a) == int(g[f"bin_counts{half}"][i, k]), (case, half, slot, len(a), int(g[f"bin_counts{half}"][i, k]))
    assert np.array_equal(digest(a), g[f"bin_digests{half}"][i, k]), (case, half, slot)
