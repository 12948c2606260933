"""GPU suite (run with -m gpu on an MI355X): the matcher and the exact Delaunay at frame sizes up to the 14-bit
coordinate limit (w, h < 16384).  Point sets and match lists of tests/fullrange.py through the device chain of the
look-ahead path, the device sub-trees and the device vertex sort; frames at the geometry boundaries of the feature
records' bin order, each asserting which kernels it took; the look-ahead call on UHD and 16383-wide frames; the frame
size limit; the device's in-circle and orientation predicates against exact integer arithmetic.  Everything against
the CPU oracle byte for byte (and the reference's removeOutliers where its build is present)."""
import functools

import numpy as np
import pytest

import fullrange as FR
from conftest import pkg

pytestmark = pytest.mark.gpu

VSM_PARA_MAX_LIST = 16384       # per-frame refinement = 2: longer query lists take the fits' tail on the host
VSM_DC_KD_MAX_POINTS = 65536    # look-ahead call: longer dense query lists decline the GPU-resident form
VSM_DC_TIE_POINTS = 10240       # the device's vertex sort takes lists up to this length (look-ahead: longer sparse query lists decline)
VSM_DC2_PRIOR_MAX_BINS = 1024   # the device's prior statistics keep this many bins (look-ahead: frames with more decline)


@pytest.fixture(scope="module")
def vm():
    m = pkg("visomatch")
    m.lib()  # raises if the HIP library is missing: no silent fallback
    return m


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _oracle_survivors(B, lst, method):
    want = B.remove_outliers("oracle", lst, method)
    if B.have_ref() and not FR.one_pixel_only(lst):
        assert _same(want, B.remove_outliers("ref", lst, method))
    return want


# ---- point sets and match lists over the whole coordinate range ------------------------------------------------------

@pytest.mark.parametrize("w,h", FR.EXTENTS)
def test_device_chain_remove_outliers_full_range(vm, B, w, h):
    """the GPU-resident removeOutliers + prior statistics (keys x << 34 | y << 20 | index, mesh points x | y << 16, reach
    words) on lists whose pixels reach 16382: survivors against the oracle's, prior boxes against the host code's"""
    bs = 50   # (the device's prior statistics keep at most 1024 bins in LDS, as a handle's frame must: vsm_seq2.inc declines more)
    while -(-w // bs) * -(-h // bs) > VSM_DC2_PRIOR_MAX_BINS:
        bs *= 2
    lists = FR.match_lists(vm, w, h, seed=w ^ h)
    rs = np.random.RandomState(w + h)
    lists.append(("uniform12289", FR.to_matches(vm, rs, FR.uniform(rs, 12289, w, h), w, h)))   # the long-list preparation kernel
    for name, lst in lists:
        for method in ((0, 1, 2) if name in ("uniform481", "rows6", "grid", "circle+interior") else (2,)):
            want = _oracle_survivors(B, lst, method)
            hs, hr, _ = vm.remove_outliers(lst, method, w, h, match_binsize=bs)
            assert _same(want, hs), (w, h, name, method, len(want), len(hs))
            for gt in (False, True):
                if gt and len(lst) > VSM_DC_TIE_POINTS:
                    continue
                gs, gr, _ = vm.remove_outliers(lst, method, w, h, gpu=True, gpu_ties=gt, copies=3, match_binsize=bs)
                assert _same(want, gs) and np.array_equal(hr, gr), (w, h, name, method, gt, len(want), len(gs))


def test_device_chain_band_overflow_full_range(vm, B):
    """large-extent lists with the merge levels' band turned down (every large node redone in global memory)"""
    try:
        vm.lib().vsm_debug_dc2_band_factor(0)
        for w, h in ((16383, 16383), (16383, 64)):
            for name, lst in FR.match_lists(vm, w, h, seed=7):
                if len(lst) < 400:
                    continue
                want = _oracle_survivors(B, lst, 2)
                gs, _, _ = vm.remove_outliers(lst, 2, w, h, gpu=True, copies=2, match_binsize=800 if h > 64 else 50)
                assert _same(want, gs), (w, h, name, len(want), len(gs))
    finally:
        vm.lib().vsm_debug_dc2_band_factor(-1)


@pytest.mark.parametrize("w,h", FR.EXTENTS)
def test_delaunay_subtrees_on_gpu_full_range(vm, B, w, h):
    """the shared form of the exact Delaunay (device sub-trees and merge nodes, device kd order both ways) against the
    oracle's triangles, over the leaf / top grid of test_gpu_parity.test_delaunay_subtrees_on_gpu"""
    for name, p in FR.point_sets(w, h, seed=w ^ h):
        whole = FR.canon(B.delaunay("oracle", p.astype(np.float32)))
        for leaf, top in ((3, 0), (14, 0), (56, 0), (500, 0), (3, 12), (14, 120), (16, 240), (56, 480), (30, 900),
                          (480, -1), (100, -1), (14, -1), (5000, -1)):
            for kd in (False, True):
                assert np.array_equal(whole, FR.canon(vm.delaunay_gpu_split(p, leaf, top, kd))), (w, h, name, leaf, top, kd)


def test_device_vertex_sort_at_large_coordinates(vm):
    """k_dc_ties names the same match for every shared pixel as the host emulation, pixels near the 14-bit limit"""
    rs = np.random.RandomState(5)
    checked = pairs = 0
    for w, h in FR.EXTENTS:
        sets = [p for name, p in FR.point_sets(w, h, seed=w ^ h) if name.startswith("dup")]
        for n in (40, 300, 2000):
            base = np.stack([rs.randint(w // 2, w, 24), rs.randint(h // 2, h, 24)], 1)   # few pixels, many matches each
            sets.append(np.concatenate([base[rs.randint(0, 24, n)], FR.uniform(rs, n, w, h)]))
        for p in sets:
            host, _ = vm.ties(p, gpu=False)
            dev, _ = vm.ties(p, gpu=True)
            if dev is None:
                assert len(host) > 255, len(p)
                continue
            assert np.array_equal(host, dev), (w, h, len(p))
            checked += 1
            pairs += len(host)
    assert checked >= 15 and pairs > 100


# ---- the device predicates -------------------------------------------------------------------------------------------

def _exact(q):
    """orientation of a, b, c and the in-circle determinant of a, b, c, d in Python integers"""
    out = []
    for (ax, ay), (bx, by), (cx, cy), (dx, dy) in q.tolist():
        ccw = (ax - cx) * (by - cy) - (ay - cy) * (bx - cx)
        adx, ady, bdx, bdy, cdx, cdy = ax - dx, ay - dy, bx - dx, by - dy, cx - dx, cy - dy
        det = ((adx * adx + ady * ady) * (bdx * cdy - cdx * bdy) + (bdx * bdx + bdy * bdy) * (cdx * ady - adx * cdy) +
               (cdx * cdx + cdy * cdy) * (adx * bdy - bdx * ady))
        out.append((ccw, (det > 0) - (det < 0), int(det > 0)))
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def test_device_predicates_exact_over_the_full_range(vm):
    """ccw_p, incircle_s and incircle_in of the device chain's mesh (vsm_dc_lds.h) evaluated on the GPU against Python
    integers: quadruples of the 7735-circle's lattice points (all exactly cocircular: a double-precision sum gets some
    of them wrong), the frame's four corners, +-1 perturbations of cocircular quadruples, random ones at the full range"""
    rs = np.random.RandomState(17)
    c = FR.circle_7735()
    qs = [c[np.argsort(rs.rand(60000, 108), axis=1)[:, :4]]]                       # 60 k cocircular quadruples
    corners = np.array([(0, 0), (16383, 0), (0, 16383), (16383, 16383)])
    import itertools
    qs.append(np.array([corners[list(p)] for p in itertools.permutations(range(4))]))
    pert = c[np.argsort(rs.rand(40000, 108), axis=1)[:, :4]].copy()
    k = rs.randint(0, 4, len(pert))
    pert[np.arange(len(pert)), k, rs.randint(0, 2, len(pert))] += rs.choice([-1, 1], len(pert))
    qs.append(pert)
    qs.append(rs.randint(0, 1 << 14, (100000, 4, 2)))
    q = np.concatenate(qs).astype(np.int64)
    assert q.min() >= 0 and q.max() < 1 << 14
    want = _exact(q)
    got = vm.device_predicates(q).astype(np.int64)
    assert np.count_nonzero(want[:60000, 1]) == 0
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    assert len(bad) == 0, (len(bad), q[bad[:3]].tolist(), got[bad[:3]].tolist(), want[bad[:3]].tolist())


# ---- frames at the geometry boundaries ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _frames(w, h, n):
    synth = pkg("synth")
    # (the disparity ramp grows down the frame; the synthetic canvas is 1024 px wider than the frame)
    return tuple(synth.stereo_sequence(5, w, h, n, disparity=20, ramp=(1, 16) if h < 8192 else (1, 32)))


_ORACLE = {}


def _oracle_run(B, w, h, n, params, method):
    """the oracle's features, match result, stages and final list after every frame; computed once per geometry"""
    key = (w, h, n, tuple(sorted(params.items())), method)
    if key not in _ORACLE:
        c = B.CpuMatcher("oracle", **params)
        out = []
        for l, r in _frames(w, h, n):
            c.push_back(l, r if method else None)
            sets = ("1c1", "1c2", "2c1", "2c2") if method else ("1c1", "1c2")
            feats = {s: c.features(s) for s in sets}
            ok = c.match(method)
            out.append(dict(feats=feats, ok=ok, stages=[c.stage(s) for s in range(5)], matches=c.matches()))
        c.close()
        _ORACLE[key] = out
    return _ORACLE[key]


FUSED, FALLBACK = "k_feat_scan + k_feat_order", "k_scan_cells + k_emit + k_bin_*"
# (frame, parameters, frames pushed, record / bin order the geometry takes - vsm_order_plan, vsm_image.hip)
GEOMETRIES = {
    "3000x1500 half, histogram 141 KB": (3000, 1500, {}, 2, FUSED),
    "3072x1536 half, histogram 150.2 KB": (3072, 1536, {}, 2, FALLBACK),
    "8192x560 half, histogram 153.8 KB": (8192, 560, {}, 2, FALLBACK),
    "3840x2160 half, refinement 0": (3840, 2160, {"refinement": 0}, 2, FALLBACK),
    "3840x2160 half": (3840, 2160, {}, 3, FALLBACK),
    "3840x2160 half, refinement 2": (3840, 2160, {"refinement": 2}, 2, FALLBACK),
    "3840x2160 full, bins 71, capacity < 2^21": (3840, 2160, {"half_resolution": 0, "match_binsize": 71}, 2, FUSED),
    "4096x2160 full, bins 71, capacity >= 2^21": (4096, 2160, {"half_resolution": 0, "match_binsize": 71}, 2, FALLBACK),
    "16383x96 half": (16383, 96, {}, 2, FUSED),
    "96x16383 half": (96, 16383, {}, 2, FUSED),
}
CASES = [(g, 2) for g in GEOMETRIES] + [(g, m) for g in ("3000x1500 half, histogram 141 KB", "3840x2160 half") for m in (0, 1)]


@pytest.mark.parametrize("geometry,method", CASES)
def test_frames_at_the_geometry_boundaries(vm, B, geometry, method):
    w, h, params, n, path = GEOMETRIES[geometry]
    want = _oracle_run(B, w, h, n, params, method)
    g = vm.Matcher(stage_capture=True, **params)
    g.set_profiling(True)
    for f, (l, r) in enumerate(_frames(w, h, n)):
        assert g.push_back(l, r if method else None) == 0
        for s, fs in want[f]["feats"].items():
            assert _same(g.features(s), fs), (geometry, method, f, s)
        assert g.match(method) == want[f]["ok"], (geometry, method, f)
        for s in range(5):
            assert _same(g.stage(s), want[f]["stages"][s]), (geometry, method, f, s)
        assert _same(g.get_matches(), want[f]["matches"]), (geometry, method, f)
    st = g.kernel_stats()
    g.close()
    fused = st["k_feat_scan"][1] > 0 and st["k_feat_order"][1] > 0
    fallback = st["k_emit"][1] > 0 and st["k_bin_rank"][1] > 0
    assert (fused, fallback) == ((True, False) if path == FUSED else (False, True)), (geometry, st)
    assert len(want[-1]["matches"]) > 1000
    if w >= 16383 or h >= 16383:   # pixels with bit 13 set reach the final list
        assert max(want[-1]["matches"]["u1c"].max(), want[-1]["matches"]["v1c"].max()) > 16000
    if w == 8192:   # x fills 13 bits
        assert want[-1]["matches"]["u1c"].max() > 8100
    if params.get("refinement") == 2:
        # longer than the device's fits take (the query list is at least as long as the matches): the per-frame path's
        # tail runs on the host - without stage capture, which keeps the fits on the host anyway.  k_parabolic_apply (the
        # device's tail) must not launch here, and must on a short list with the same parameters
        assert len(want[-1]["stages"][2]) > VSM_PARA_MAX_LIST
        for fw, fh in ((w, h), (640, 480)):
            ref = want if fw == w else _oracle_run(B, fw, fh, n, params, method)
            g = vm.Matcher(**params)
            g.set_profiling(True)
            for f, (l, r) in enumerate(_frames(fw, fh, n)):
                assert g.push_back(l, r if method else None) == 0
                assert g.match(method) == ref[f]["ok"]
                assert _same(g.get_matches(), ref[f]["matches"]), (geometry, fw, f)
            launches = g.kernel_stats()["k_parabolic_apply"][1]
            g.close()
            if fw == w:
                assert launches == 0, launches
            else:
                assert launches > 0 and len(ref[-1]["stages"][2]) <= VSM_PARA_MAX_LIST


# (frame, parameters, device inputs, why the look-ahead call declines its GPU-resident form - vsm_seq2.inc - or None)
LOOKAHEAD = {
    "3840x2160, 77 x 44 bins": (3840, 2160, {}, False, "bins"),
    "3840x2160, 77 x 44 bins, device inputs": (3840, 2160, {}, True, "bins"),
    "3840x2160, bins 128": (3840, 2160, {"match_binsize": 128}, False, "sparse and dense lists"),
    "3840x2160, bins 128, one stage": (3840, 2160, {"match_binsize": 128, "multi_stage": 0}, False, "dense list"),
    "3840x2160, bins 128, one stage, nms_n 5": (3840, 2160, {"match_binsize": 128, "multi_stage": 0, "nms_n": 5}, False, None),
    "16383x96": (16383, 96, {}, False, None),
}


@pytest.mark.parametrize("case", list(LOOKAHEAD))
def test_lookahead_at_large_frames(vm, B, case):
    """run_sequence against the oracle frame by frame, and the form it took against the rule of vsm_seq2.inc, worked out
    from the oracle's feature counts (a job's queries are the previous left image's features): the GPU-resident form
    declines a frame with more prior bins than the device's statistics keep, a sparse query list beyond the device's
    vertex sort (VSM_DC_TIE_POINTS) and a dense one beyond its kd order (VSM_DC_KD_MAX_POINTS).  At UHD the 128-pixel bins
    keep the frame within the bin limit, so the list lengths alone decide: both lists too long; the dense list alone
    (one stage: no sparse queries); both within the limits (one stage, nms_n 5: 63 k dense features) - the GPU-resident
    form with lists of 30 k matches.  16383 x 96: every list fits, pixels near 16383 go through the device chain"""
    w, h, params, device_inputs, reason = LOOKAHEAD[case]
    n = 3
    want = _oracle_run(B, w, h, n, params, 2)
    p = vm.default_params()
    for k, v in params.items():
        setattr(p, k, v)
    bins = -(-w // p.match_binsize) * -(-h // p.match_binsize)
    nq0 = max(len(x["feats"]["1c1"]) for x in want[:-1]) if p.multi_stage else 0
    nq1 = max(len(x["feats"]["1c2"]) for x in want[:-1])
    why = ("bins" if bins > VSM_DC2_PRIOR_MAX_BINS else
           "sparse and dense lists" if nq0 > VSM_DC_TIE_POINTS and nq1 > VSM_DC_KD_MAX_POINTS else
           "sparse list" if nq0 > VSM_DC_TIE_POINTS else "dense list" if nq1 > VSM_DC_KD_MAX_POINTS else None)
    assert why == reason, (case, bins, nq0, nq1)
    if reason in ("sparse and dense lists", "dense list"):   # the matches alone are more than the kd order takes
        assert max(len(x["stages"][2]) for x in want) > VSM_DC_KD_MAX_POINTS
    fr = _frames(w, h, n)
    left, right = np.stack([l for l, _ in fr]), np.stack([r for _, r in fr])
    if device_inputs:
        import torch
        left, right = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    g = vm.Matcher(**params)
    got = g.run_sequence(left, right, 2)
    path = g.sequence_path()
    g.close()
    for f in range(n):
        assert _same(got[f], want[f]["matches"]), (case, f, len(got[f]), len(want[f]["matches"]))
    assert path == (1 if reason else 2), (case, path)
    assert len(want[-1]["matches"]) > 1000
    if w == 16383:
        assert want[-1]["matches"]["u1c"].max() > 16000


def test_frame_size_limit(vm, B):
    """w or h of 16384 is rejected (14-bit coordinates), and the handle then matches valid frames like a fresh one"""
    synth = pkg("synth")
    g = vm.Matcher()
    assert g.push_back(np.zeros((64, 16384), np.uint8), np.zeros((64, 16384), np.uint8)) == vm.Matcher.EDIMS
    assert g.push_back(np.zeros((16384, 64), np.uint8), np.zeros((16384, 64), np.uint8)) == vm.Matcher.EDIMS
    c = B.CpuMatcher("oracle")
    for l, r in synth.stereo_sequence(9, 320, 128, 2, disparity=12, ramp=(1, 16)):
        assert g.push_back(l, r) == 0
        c.push_back(l, r)
        assert g.match(2) == c.match(2)
        assert _same(g.get_matches(), c.matches())
    assert len(c.matches()) > 50
    g.close()
    c.close()
