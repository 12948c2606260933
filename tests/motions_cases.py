"""Batches of flow-match lists for the batched monocular motions (Matcher.motions / host_pairs_motions).  Shared by
tests/test_motions_cpu.py and tests/test_motions_gpu.py.

The lists are mostly those of tests/mono_content.py (FAMILIES: expected results pinned to the oracle in
golden/mono_content.npz), plus lists that end where no family does:

  nine            9 matches                                          stage 0 (rc -1)
  same_prev       20 matches whose previous points are one pixel     stage 1 (rc -1): the normalisation's scale is 0 / 0
  noise50         50 matches between uniformly random pixels         stage 2 (rc 0): no hypothesis finds 10 inliers
  dup10           (family)                                           stage 4
  stationary      (family)                                           stage 5
  control         (family)                                           stage 6

Stage 3 - no R|t candidate with a point in front of both cameras - has no list here: for a match that satisfies the
epipolar constraint one of the four candidates always puts the point in front of both cameras unless it lies at infinity,
and the rounding of the 4 x 4 SVD then still gives the homogeneous coordinate some sign.  None of the families, and nothing
tried while these cases were written (zero flow, coordinates of 1e19, mirrored and swapped lists), ends there.

A batch = (lists, K hypotheses, bucket).  Sizes: 9 / 10 matches (the estimator's minimum), 63 / 64 / 65 (a wave), 255 / 256 /
257 (a block of the count, winner and vote kernels), 511 / 512 / 513 points in front (two vote tiles and one more), K = 1, 16,
17 (the fit kernel takes 16 hypotheses per block: with 17 a pair boundary falls inside a block) and 200."""
import numpy as np

import mono_content as MC
from conftest import pkg

MG = MC.MG
STAGES = {"nine": 0, "same_prev": 1, "noise50": 2, "dup10": 4, "stationary": 5, "control": 6}
BUCKET = (2, 50.0, 50.0)


def params(K=200, **kw):
    vm = pkg("visomatch")
    return vm.vo_mono_params(MC.F, MC.CU, MC.CV, bucket=BUCKET, **{**MC.PARAMS, "ransac_iters": K, **kw})


def _as_pmatch(m):
    vm = pkg("visomatch")
    out = np.zeros(len(m), vm.P_MATCH)
    for k in vm.P_MATCH.names:
        out[k] = m[k]
    return out


_cache = {}


def one(name):
    """a list by name: a family of mono_content, one of the extra lists above, or scene<n> / front<n>"""
    if name in _cache:
        return _cache[name]
    if name in MC.FAMILIES:
        m = MC.matches(name)
    elif name == "nine":
        m = MC.matches("control")[:9]
    elif name == "ten":
        m = MC.matches("control")[:10]
    elif name == "same_prev":
        m = MC.matches("control")[:20].copy()
        m["u1p"], m["v1p"] = 100.0, 50.0
    elif name == "noise50":
        rs = np.random.RandomState(5)
        m = MC.matches("control")[:50].copy()
        for k in ("u1p", "v1p", "u1c", "v1c"):
            m[k] = rs.uniform(0, 1000, 50).astype(np.float32)
    elif name == "empty":
        m = MC.matches("control")[:0]
    elif name.startswith("scene"):      # a regular noisy scene of that many matches
        n = int(name[5:])
        m = MG.mono_scene(np.random.RandomState(2000 + n), n, MC.MOTION)
    elif name.startswith("front"):      # a clean scene, all of whose matches end in front of the chosen camera pair
        n = int(name[5:])
        m = MG.mono_scene(np.random.RandomState(1511), n, MC.MOTION, noise=0.05, out_frac=0.0)
    else:
        raise KeyError(name)
    _cache[name] = _as_pmatch(m)
    return _cache[name]


SEVEN = ("control", "nine", "integer", "same_prev", "dup10", "noise50", "front512")   # P = 1, 2, 7 x motions_chunk 0, 1, 3

BATCHES = {
    # name: (list names, K, bucket)
    "families": (MC.FAMILIES, 200, False),
    "stages": (tuple(STAGES), 200, False),
    "sizes_small": (("nine", "ten", "scene63", "scene64", "scene65"), 200, False),
    "sizes_block": (("scene255", "scene256", "scene257"), 200, False),
    "front": (("front511", "front512", "front513"), 200, False),
    "k1": (("control", "integer", "dup12"), 1, False),
    "k16": (("control", "integer", "dup12"), 16, False),
    "k17": (("control", "integer", "dup12"), 17, False),
    "k0": (("control", "integer"), 0, False),
    "empty_between": (("control", "empty", "half_pixel"), 200, False),
    "twice": (("control", "integer", "control"), 200, False),
    "seven": (SEVEN, 200, False),
    "bucket": (("integer", "half_pixel", "repeated", "nine", "control"), 200, True),
}


def batch(name):
    names, K, bucket = BATCHES[name]
    lists = [one(n) for n in names]
    if bucket:   # bucketFeatures has no bucket left of or above the image: the scenes' few matches out there go
        lists = [m[(m["u1c"] >= 0) & (m["v1c"] >= 0)] for m in lists]
    return lists, params(K), bucket


def assert_same(a, b, what=""):
    """two Motions results: every int equal, every double by its bytes, inliers and lists equal"""
    assert len(a) == len(b), what
    assert np.array_equal(a.rc, b.rc), (what, a.rc, b.rc)
    assert np.array_equal(a.stage, b.stage), (what, a.stage, b.stage)
    assert a.tr.tobytes() == b.tr.tobytes(), (what, "tr6")
    assert a.T.tobytes() == b.T.tobytes(), (what, "T16")
    for k in range(len(a)):
        assert np.array_equal(a.inliers(k), b.inliers(k)), (what, k, "inliers")
        assert a.matches(k).tobytes() == b.matches(k).tobytes(), (what, k, "matches")


def chain_poses_ref(n_frames, pairs, T, rc, root=0):
    """vsm_chain_poses restated in plain Python floats -> (poses [F, 12], valid [F])"""
    poses = [[0.0] * 12 for _ in range(n_frames)]
    valid = [0] * n_frames
    for i in range(3):
        poses[root][5 * i] = 1.0
    valid[root] = 1

    def mul(A, Bm):
        out = [0.0] * 12
        for i in range(3):
            for j in range(4):
                s = A[i * 4 + 0] * Bm[0 * 4 + j]
                for k in (1, 2):
                    s += A[i * 4 + k] * Bm[k * 4 + j]
                if j == 3:
                    s += A[i * 4 + 3]
                out[i * 4 + j] = s
        return out

    changed = True
    while changed:
        changed = False
        for k, (a, b) in enumerate(pairs):
            if rc[k] != 1 or a == b or valid[a] == valid[b]:
                continue
            t = [float(x) for x in np.asarray(T[k], dtype=np.float64).reshape(16)]
            if valid[a]:
                M = [0.0] * 12
                for i in range(3):
                    for j in range(3):
                        M[i * 4 + j] = t[j * 4 + i]
                    s = t[0 * 4 + i] * t[0 * 4 + 3]
                    for q in (1, 2):
                        s += t[q * 4 + i] * t[q * 4 + 3]
                    M[i * 4 + 3] = -s
                poses[b] = mul(poses[a], M)
                valid[b] = 1
            else:
                poses[a] = mul(poses[b], t[:12])
                valid[a] = 1
            changed = True
    return np.array(poses, dtype=np.float64), np.array(valid, dtype=np.uint8)


# ---- the image case: a short street clip (synth.road_*), consecutive and skip-one pairs -------------------------------------

ROAD_W, ROAD_H, ROAD_N = 417, 163, 6
ROAD_PAIRS = [(f - 1, f) for f in range(1, ROAD_N)] + [(f - 2, f) for f in range(2, ROAD_N)]


def road_frames(synth):
    pyr = synth.road_pyramid(1234, levels=8, size=1024)
    return np.stack([synth.road_mono_frame(pyr, f, ROAD_W, ROAD_H) for f in range(ROAD_N)])


def road_params(K=200):
    vm = pkg("visomatch")
    return vm.vo_mono_params(float(pkg("synth").ROAD_F), ROAD_W // 2, (ROAD_H * 2) // 5, bucket=BUCKET, height=1.65, pitch=0.0, ransac_iters=K)


ROAD_POINT_PARAMS = dict(point_type=-1, max_dist=1e6, min_angle=0.001)
