"""Match lists and kernel inputs on which the monocular egomotion's linear algebra degenerates.  Shared by
tests/test_mono_content_cpu.py, tests/test_mono_kernels_gpu.py and the `mono_content` target of golden/make_golden.py.

Match families (FAMILIES, built by matches(name) from make_golden.mono_scene; every one has its own seed):

  control               a regular noisy scene
  stationary            u1c == u1p, v1c == v1p exactly: every 8-point sample has rank <= 6
  stationary_outliers   the same with 10 % of the current points moved
  integer, half_pixel   all coordinates rounded to whole / half pixels (the matcher without sub-pixel refinement)
  repeated              600 matches drawn from 40 distinct ones
  pure_rotation         no translation, no noise: the epipolar constraint has a three-dimensional null space
  one_row               v1p == v1c == one image row
  one_column            u1p == u1c == the column through the principal point
  dup10, dup12          10 / 12 matches, 6 distinct: no sample of 8 is free of repeats
  front511, front512    one clean scene cut to 511 / 512 matches, all of them in front of the chosen camera pair: the
                        plane vote runs on the host for the first and on the GPU for the second

Kernel-level inputs: fit_inputs(K) (samples of declared rank properties, interleaved so that the four hypotheses of a
64-lane wave differ), count_points() / count_matrices() / edge_threshold(), triangulation_matches(n) / rt_candidates(),
vote_inputs(kind, np_).  replay() runs every family through one estimator class in order, from one fresh sampler."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as MG  # noqa: E402

F, CU, CV = MG.KITTI["f"], MG.KITTI["cu"], MG.KITTI["cv"]
PARAMS = dict(height=1.65, pitch=-0.08, ransac_iters=200)
MOTION = (0.002, 0.01, -0.001, 0.02, -0.01, -0.9)
VOTE_MIN_POINTS = 512    # best_plane: fewer points in front of the camera are voted on the host

FAMILIES = ("control", "stationary", "stationary_outliers", "integer", "half_pixel", "repeated", "pure_rotation", "one_row",
            "one_column", "dup10", "dup12", "front511", "front512")
RANK_DEFICIENT = ("stationary", "one_row", "one_column", "dup10", "dup12")   # all rows together have rank < 8, so has every sample
VOTE_ON_DEVICE = ("integer", "half_pixel", "repeated", "front512")    # at least 512 points in front of the camera (checked with the oracle)


def _rs(name):
    return np.random.RandomState(1000 + FAMILIES.index(name))


def matches(name):
    rs = _rs(name)
    if name == "control":
        return MG.mono_scene(rs, 300, MOTION)
    if name in ("stationary", "stationary_outliers"):
        m = MG.mono_scene(rs, 300, (0, 0, 0, 0, 0, 0), noise=0.0, out_frac=0.0)
        m["u1c"], m["v1c"] = m["u1p"], m["v1p"]
        if name == "stationary_outliers":
            bad = rs.permutation(300)[:30]
            m["u1c"][bad] += rs.uniform(5, 30, 30).astype(np.float32)
            m["v1c"][bad] -= rs.uniform(5, 30, 30).astype(np.float32)
        return m
    if name in ("integer", "half_pixel"):
        n, q = (600, 1.0) if name == "integer" else (700, 2.0)
        m = MG.mono_scene(rs, n, MOTION, out_frac=0.02 if name == "half_pixel" else 0.2)
        for k in ("u1p", "v1p", "u1c", "v1c"):
            m[k] = np.rint(m[k] * q) / q
        return m
    if name == "repeated":
        base = MG.mono_scene(rs, 40, MOTION, out_frac=0.1)
        m = base[rs.randint(0, 40, 600)]
        m["i1p"] = m["i1c"] = np.arange(600)
        return m
    if name == "pure_rotation":
        return MG.mono_scene(rs, 400, (0.0, 0.03, 0.0, 0.0, 0.0, 0.0), noise=0.0, out_frac=0.0)
    if name == "one_row":
        m = MG.mono_scene(rs, 300, MOTION)
        m["v1p"] = m["v1c"] = 200.0
        return m
    if name == "one_column":
        m = MG.mono_scene(rs, 300, MOTION)
        m["u1p"] = m["u1c"] = np.float32(CU)
        return m
    if name in ("dup10", "dup12"):
        n = int(name[3:])
        base = MG.mono_scene(rs, 6, MOTION, noise=0.0, out_frac=0.0)
        m = base[np.arange(n) % 6]
        m["i1p"] = m["i1c"] = np.arange(n)
        return m
    if name in ("front511", "front512"):
        return MG.mono_scene(np.random.RandomState(1511), 512, MOTION, noise=0.05, out_frac=0.0)[: int(name[5:])]
    raise KeyError(name)


def replay(make_vo, reset_sampler, after=None):
    """every family in order from one fresh sampler -> {family: (ok, T, inliers, after())}"""
    reset_sampler()
    out = {}
    for name in FAMILIES:
        vo = make_vo(F, CU, CV, **PARAMS)
        ok, T = vo.process_matches(matches(name))
        out[name] = (bool(ok), T.copy(), vo.inliers().copy(), after(vo) if after else None)
        vo.close()
    return out


def assert_equals_golden(got, g, same_doubles=lambda a, b: a.tobytes() == b.tobytes()):
    assert list(g["families"]) == list(FAMILIES)
    for name in FAMILIES:
        sha = hashlib.sha256(np.ascontiguousarray(matches(name)).tobytes()).hexdigest()
        assert sha == str(g[name + "_input_sha"]), f"{name}: the generated match list is not the recorded one"
        ok, T, inl, _ = got[name]
        assert ok == bool(g[name + "_ok"]), name
        assert np.array_equal(inl, g[name + "_inliers"]), name
        assert same_doubles(T, np.frombuffer(g[name + "_T"].tobytes(), np.float64).reshape(4, 4)), name


def constraint_matrix(pts, picks=None):
    """the 8-point constraint rows (float products, as fundamentalMatrix forms them) of pts [n, 4] = u1p, v1p, u1c, v1c"""
    p = np.asarray(pts, dtype=np.float32).reshape(-1, 4)
    if picks is not None:
        p = p[np.asarray(picks)]
    u1p, v1p, u1c, v1c = p.T
    one = np.ones(len(p), np.float32)
    return np.stack([u1c * u1p, u1c * v1p, u1c, v1c * u1p, v1c * v1p, v1c, u1p, v1p, one], axis=1).astype(np.float64)


def rank(A, tol=1e-12):
    s = np.linalg.svd(A, compute_uv=False)
    return int(np.sum(s > tol * s[0])) if s[0] > 0 else 0


def points_of(m):
    return np.stack([m["u1p"], m["v1p"], m["u1c"], m["v1c"]], axis=1).astype(np.float32)


def as_matches(pts):
    """pts [n, 4] as a match list (what the oracle's per-piece functions take)"""
    p = np.asarray(pts, dtype=np.float32).reshape(-1, 4)
    m = np.zeros(len(p), dtype=MG.B.MATCH_DTYPE)
    m["u1p"], m["v1p"], m["u1c"], m["v1c"] = p.T
    m["i1p"] = m["i1c"] = np.arange(len(p))
    return m


def normalised(m):
    """normalizeFeaturePoints in numpy (centred, mean radius sqrt 2, float fields); close to the estimator's, not bit-equal"""
    p = points_of(m).astype(np.float64)
    p -= p.mean(axis=0)
    sp = np.sqrt(2.0) / np.mean(np.hypot(p[:, 0], p[:, 1]))
    sc = np.sqrt(2.0) / np.mean(np.hypot(p[:, 2], p[:, 3]))
    return (p * np.array([sp, sp, sc, sc])).astype(np.float32)


# ---- k_mono_fit: samples with a declared property ---------------------------------------------------------------------

FIT_PROPERTIES = ("full", "rank_lt8", "zero_column", "two_equal_rows")
FIT_SCALES = tuple(10.0 ** e for e in range(-3, 4))
_GROUP = 48   # points per scale: 24 generic, 12 stationary, 12 with u1c == 0


def fit_points():
    """7 groups of 48 normalised-like points, group g scaled by 10^(g - 3)"""
    rs = np.random.RandomState(77)
    out = []
    for s in FIT_SCALES:
        g = rs.normal(0, 1, (_GROUP, 4))
        g[:, 2:] = g[:, :2] + rs.normal(0, 0.05, (_GROUP, 2))   # a small flow
        g[24:36, 2:] = g[24:36, :2]                              # stationary
        g[36:, 2] = 0.0                                          # u1c == 0: the first three columns vanish
        out.append(g * s)
    return np.concatenate(out).astype(np.float32)


def fit_inputs(K):
    """(pts [336, 4], picks [K, 8], property of each hypothesis): hypothesis k has property (k + k // 4) % 4 and scale
    group (k // 4) % 7, so the four hypotheses of a wave hold four different properties"""
    pts = fit_points()
    rs = np.random.RandomState(78)
    picks = np.zeros((K, 8), np.int32)
    props = []
    for k in range(K):
        prop = FIT_PROPERTIES[(k + k // 4) % 4]
        base = ((k // 4) % len(FIT_SCALES)) * _GROUP
        if prop == "full":
            p = rs.permutation(24)[:8]
        elif prop == "rank_lt8":
            p = 24 + rs.permutation(12)[:8]
        elif prop == "zero_column":
            p = 36 + rs.permutation(12)[:8]
        else:
            p = rs.permutation(24)[:8]
            p[rs.randint(1, 8)] = p[0]
        picks[k] = base + p
        props.append(prop)
    return pts, picks, props


def has_property(A, prop):
    if prop == "full":
        return rank(A) == 8
    if prop == "rank_lt8":
        return rank(A) < 8
    if prop == "zero_column":
        return bool(np.any(np.all(A == 0, axis=0)))
    return any(np.array_equal(A[i], A[j]) for i in range(8) for j in range(i))


# ---- k_mono_inlier_count ------------------------------------------------------------------------------------------------

COUNT_NS = (10, 63, 64, 65, 255, 256, 257, 700)
COUNT_KS = (1, 17, 200)
HUGE_F = np.full((3, 3), 1e160)   # squares overflow: the Sampson denominator is inf, the distance NaN or 0


def count_points():
    """700 normalised points: a regular scene, every seventh match stationary, every eleventh a repeat of its neighbour"""
    m = MG.mono_scene(np.random.RandomState(79), 700, MOTION)
    p = normalised(m)
    p[::7, 2:] = p[::7, :2]
    p[11::11] = p[10::11][: len(p[11::11])]
    return p


def count_matrices(B, K):
    """K matrices: the oracle's fits of fit_inputs(K), with an all-zero matrix at 1 and HUGE_F at 2 where K allows"""
    pts, picks, _ = fit_inputs(K)
    m = as_matches(pts)
    Fs = np.stack([B.oracle_fundamental(m, picks[k]) for k in range(K)])
    if K > 2:
        Fs[1] = 0.0
        Fs[2] = HUGE_F
    return Fs


def sampson(p, Fm):
    """getInlier's distance of one point (u1p, v1p, u1c, v1c) in the reference's operation order; Python floats are IEEE
    doubles and nothing here is contracted, so the value is the oracle's"""
    u1, v1, u2, v2 = (float(x) for x in p)
    f = [float(x) for x in np.asarray(Fm).reshape(9)]
    Fx1u = f[0] * u1 + f[1] * v1 + f[2]
    Fx1v = f[3] * u1 + f[4] * v1 + f[5]
    Fx1w = f[6] * u1 + f[7] * v1 + f[8]
    Ftx2u = f[0] * u2 + f[3] * v2 + f[6]
    Ftx2v = f[1] * u2 + f[4] * v2 + f[7]
    x2tFx1 = u2 * Fx1u + v2 * Fx1v + Fx1w
    return abs(x2tFx1 * x2tFx1 / (Fx1u * Fx1u + Fx1v * Fx1v + Ftx2u * Ftx2u + Ftx2v * Ftx2v))


def edge_threshold(B):
    """(points, F, thr): thr is exactly the distance of point 5 to F (a fit on a regular sample), so the strict `<` decides"""
    pts = count_points()
    Fm = B.oracle_fundamental(as_matches(pts), [1, 2, 3, 4, 6, 8, 9, 12])
    return pts, Fm, sampson(pts[5], Fm)


# ---- k_mono_triangulate ---------------------------------------------------------------------------------------------------

TRI_NS = (10, 63, 64, 65, 700)


def rt_candidates(motion=MOTION, zero_t=False):
    """the four (R, t) of EtoRt for the essential matrix of `motion`: (Ra, t), (Ra, -t), (Rb, t), (Rb, -t)"""
    rx, ry, rz, tx, ty, tz = motion
    sx, cx, sy, cy, sz, cz = np.sin(rx), np.cos(rx), np.sin(ry), np.cos(ry), np.sin(rz), np.cos(rz)
    R = np.array([[cy * cz, -cy * sz, sy], [sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy],
                  [-cx * sy * cz + sx * sz, cx * sy * sz + sx * cz, cx * cy]])
    t = np.array([tx, ty, tz]) / np.linalg.norm([tx, ty, tz])
    E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
    U, _, Vt = np.linalg.svd(E)
    W = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    Ra, Rb = U @ W @ Vt, U @ W.T @ Vt
    Ra, Rb = Ra * np.sign(np.linalg.det(Ra)), Rb * np.sign(np.linalg.det(Rb))
    tt = np.zeros(3) if zero_t else U[:, 2].copy()
    return np.stack([Ra, Ra, Rb, Rb]), np.stack([tt, -tt, tt, -tt])


def triangulation_matches(n):
    """a regular scene; match 0 does not move, match 1 sits on the principal point in both frames, match 2 repeats 3"""
    m = MG.mono_scene(np.random.RandomState(80), n, MOTION)
    m["u1c"][0], m["v1c"][0] = m["u1p"][0], m["v1p"][0]
    m["u1p"][1] = m["u1c"][1] = np.float32(CU)
    m["v1p"][1] = m["v1c"][1] = np.float32(CV)
    for k in ("u1p", "v1p", "u1c", "v1c"):
        m[k][2] = m[k][3]
    return m


# ---- k_mono_plane_vote ----------------------------------------------------------------------------------------------------

VOTE_NPS = (512, 513, 4097)
VOTE_KINDS = ("scene", "all_equal", "grid_ties", "none_above", "huge_weight")


def vote_inputs(kind, np_):
    """(d [np_], threshold, weight) as estimateMotion would pass them for a median L1 norm of 20 (sigma = median / 50)"""
    rs = np.random.RandomState(81 + np_)
    threshold, weight = 0.2, 1.0 / (2.0 * 0.4 * 0.4)
    d = np.concatenate([rs.normal(1.65, 0.05, np_ // 2), rs.uniform(-3.0, 40.0, np_ - np_ // 2)])[rs.permutation(np_)]
    if kind == "scene":
        return d, threshold, weight
    if kind == "all_equal":
        return np.full(np_, 1.65), threshold, weight
    if kind == "grid_ties":
        # multiples of 1/32 mirrored about 1.625, the values recurring with period 41: all candidates of one value see the
        # same terms in the same order, so their exact sums are equal and the first of the central value must win
        k = np.arange(np_) % 41 - 20
        return 1.625 + k / 32.0, threshold, weight
    if kind == "none_above":
        return -np.abs(d), threshold, weight
    if kind == "huge_weight":
        d[7::9] = d[6::9][: len(d[7::9])]        # repeats: sums 2 beside sums 1
        d[8::27] = d[6::27][: len(d[8::27])]     # and 3
        return d, threshold, 1e300
    raise KeyError(kind)
