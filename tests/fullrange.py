"""Point sets and match lists over frames up to the 14-bit coordinate limit (w, h < 16384), shared by
tests/test_fullrange_cpu.py and tests/test_fullrange_gpu.py.  Everything is generated from a seed at run time.

Families: uniform over the whole frame (odd and even coordinates, the frame's first and last row and column included),
the 108 lattice points of x^2 + y^2 = 7735^2 around (8191, 8191) (every quadruple exactly cocircular), a coarse grid of
about 1000 px pitch, points on the four frame edges, long nearly collinear rows (circumcircles far beyond +-32767 px)
and duplicates at the extreme pixels."""
import math

import numpy as np

EXTENTS = ((4096, 2160), (8192, 4320), (16383, 16383), (16383, 64), (64, 16383))
LENGTHS = (4, 5, 17, 100, 481, 2000, 9000)


def circle_7735():
    """the 108 integer points of x^2 + y^2 = 7735^2, centred at (8191, 8191)"""
    r2 = 7735 * 7735
    pts = set()
    for x in range(-7735, 7736):
        y = math.isqrt(r2 - x * x)
        if y * y == r2 - x * x:
            pts.add((x, y))
            pts.add((x, -y))
    out = np.array(sorted(pts), dtype=np.int64) + 8191
    assert len(out) == 108
    return out


def uniform(rs, n, w, h):
    p = np.stack([rs.randint(0, w, n), rs.randint(0, h, n)], 1).astype(np.int64)
    ext = np.array([(0, 0), (w - 1, h - 1), (0, h - 1), (w - 1, 0), (w - 1, h // 2), (w // 2, 0)], dtype=np.int64)
    k = min(n // 3, len(ext))
    p[rs.permutation(n)[:k]] = ext[:k]
    return p


def edges(rs, n, w, h):
    side = rs.randint(0, 4, n)
    t = rs.rand(n)
    x = np.where(side < 2, np.round(t * (w - 1)), np.where(side == 2, 0, w - 1))
    y = np.where(side >= 2, np.round(t * (h - 1)), np.where(side == 0, 0, h - 1))
    return np.stack([x, y], 1).astype(np.int64)


def grid(w, h, pitch=1000):
    xs = np.unique(np.append(np.arange(0, w, pitch), w - 1))
    ys = np.unique(np.append(np.arange(0, h, pitch), h - 1))
    return np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2).astype(np.int64)


def rows(w, h, k):
    """k rows of three points across the frame's long side (first, middle and last pixel) and a fourth one 1 px off the row
    at a quarter of its length: the circles through it and two of the row's points have radii of millions of pixels"""
    long_x = w >= h
    L, S = (w, h) if long_x else (h, w)
    out = []
    for i in range(k):
        s = (i * (S - 2)) // max(k - 1, 1)
        out += [(0, s), (L // 2, s), (L - 1, s), (L // 4 + (i & 1), s + 1)]
    p = np.array(out, dtype=np.int64)
    return p if long_x else p[:, ::-1].copy()


def extreme_duplicates(rs, n, w, h):
    p = uniform(rs, n, w, h)
    ext = np.array([(0, 0), (w - 1, h - 1), (0, h - 1), (w - 1, 0)], dtype=np.int64)
    k = max(n // 4, 4)
    p[rs.randint(0, n, k)] = ext[rs.randint(0, 4, k)]
    return p


def point_sets(w, h, seed):
    """[(name, [n, 2] int64 points)] for one extent"""
    rs = np.random.RandomState(seed)
    out = [(f"uniform{n}", uniform(rs, n, w, h)) for n in LENGTHS]
    out += [(f"edges{n}", edges(rs, n, w, h)) for n in (5, 100, 2000)]
    out += [("grid", grid(w, h)), ("rows1", rows(w, h, 1)), ("rows6", rows(w, h, 6))]
    out += [(f"dup{n}", extreme_duplicates(rs, n, w, h)) for n in (17, 481)]
    if w >= 16383 and h >= 16383:
        c = circle_7735()
        out.append(("circle", c))
        inner = np.stack([rs.randint(8191 - 5000, 8191 + 5000, 12), rs.randint(8191 - 5000, 8191 + 5000, 12)], 1)
        out.append(("circle+interior", np.concatenate([c, inner])[rs.permutation(len(c) + len(inner))]))
    for name, p in out:
        assert p.min() >= 0 and p[:, 0].max() < w and p[:, 1].max() < h, name
    return out


def to_matches(vm, rs, pts, w, h):
    """a P_MATCH list whose current left pixels are pts: small flows and disparities around a common motion, a tenth of
    the flows and a twentieth of the disparities off (outliers for removeOutliers' support test)"""
    n = len(pts)
    m = np.zeros(n, dtype=vm.P_MATCH)
    u, v = pts[:, 0].astype(np.int64), pts[:, 1].astype(np.int64)
    m["u1c"], m["v1c"] = u, v
    fl = rs.randint(-3, 4, (n, 2))
    bad = rs.rand(n) < 0.1
    fl[bad] += rs.randint(-30, 30, (int(bad.sum()), 2))
    m["u1p"], m["v1p"] = u + 6 + fl[:, 0], v + fl[:, 1]
    d = 20 + rs.randint(-2, 3, n)
    d[rs.rand(n) < 0.05] += 17
    m["u2c"], m["v2c"] = u - d, v
    m["u2p"], m["v2p"] = m["u1p"] - d - rs.randint(-1, 2, n), m["v1p"]
    for k in ("i1p", "i2p", "i1c", "i2c"):
        m[k] = rs.randint(0, 9000, n)
    return m


def match_lists(vm, w, h, seed):
    """[(name, P_MATCH list)] for one extent: every point set as the current left pixels of a list"""
    rs = np.random.RandomState(seed + 1000)
    return [(name, to_matches(vm, rs, p, w, h)) for name, p in point_sets(w, h, seed)]


def one_pixel_only(lst):
    """more than three matches that all share one pixel: a list the reference's Triangle cannot take (it recurses without
    end on a single distinct vertex); the oracle and the product define the case"""
    return len(lst) > 3 and len(set(zip(np.asarray(lst["u1c"]).tolist(), np.asarray(lst["v1c"]).tolist()))) < 2


def canon(t):
    t = np.sort(np.asarray(t).reshape(-1, 3), axis=1)
    return t[np.lexsort(t.T[::-1])]
