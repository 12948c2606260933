"""The definition of the location's stages (include/visomatch.h, vsm_locate_run), restated for the tests.
Nothing comes from csrc/vsm_locate.h or from the library.

fit      the linear six-point resection at 60 significant digits (mpmath): conditioning by the mean and the largest absolute
         deviation exactly as the definition has it - the algebraic minimiser depends on the column scaling, so a restatement
         that skips it answers another question -, the 12 x 12 matrix, its singular value decomposition, the last right vector,
         the decomposition of its left 3 x 3 block, R = sigma U V^T, lambda = sigma 3 / (w0 + w1 + w2), t = lambda p4 s - R m.
         The null vector's sign cancels through sigma.  Whether step 2 refuses the sample is a property of double arithmetic (an
         overflowed mean) and is decided in plain floats, in the definition's order.
count    the eligible rows that vote for a state: tests/resect_ref.py's row_terms, which restates the resection's row test bit
         for bit, so the counts are exact integers.
winner   the largest count at the smallest k; -1 where the largest count is 0; verdict 3 / 4 / 0.
sample   the draw in plain Python integers: the minstd engine, std::uniform_int_distribution's rejection with the divisions of
         a range done once, a partial Fisher-Yates on the identity deck that is undone after each hypothesis."""
import math

import mpmath as mp
import numpy as np

import resect_ref as R

DPS = 60
SAMPLE = 6
MINSTD_A, MINSTD_M = 16807, 2147483647
ENGINE_SPAN = MINSTD_M - 1 - 1  # max() - min() of the engine, whose values are 1 .. 2^31 - 2


# ---- sample ---------------------------------------------------------------------------------------------------------------------

def seed_state(seed):
    s = int(seed) % MINSTD_M
    return s if s else 1


def sample(seed, E, K):
    """picks [K][6]: positions in [0, E)"""
    assert E >= SAMPLE and E - 1 < ENGINE_SPAN
    state = seed_state(seed)
    deck = list(range(E))
    out = []
    for _ in range(K):
        swapped = []
        for i in range(SAMPLE):
            cells = (E - 1 - i) + 1  # draw i is uniform in [i, E - 1]
            per_cell = ENGINE_SPAN // cells
            reject_from = cells * per_cell
            while True:
                state = state * MINSTD_A % MINSTD_M
                v = state - 1
                if v < reject_from:
                    break
            j = v // per_cell + i
            swapped.append(j)
            deck[i], deck[j] = deck[j], deck[i]
        out.append(deck[:SAMPLE])
        for i in reversed(range(SAMPLE)):
            deck[i], deck[swapped[i]] = deck[swapped[i]], deck[i]
    assert deck == list(range(E))
    return out


# ---- fit ------------------------------------------------------------------------------------------------------------------------

def conditioned(X6):
    """step 2 in doubles, in the definition's order: (mean, scale), or None where the sample is refused"""
    m = []
    for c in range(3):
        s = X6[0][c]
        for i in range(1, SAMPLE):
            s = s + X6[i][c]
        m.append(s / 6.0)
    big = 0.0
    for i in range(SAMPLE):
        for c in range(3):
            d = abs(X6[i][c] - m[c])
            if d > big:
                big = d
    if not (big > 0.0 and big < math.inf):
        return None
    return m, big


def fit(uv6, X6, f, cu, cv):
    """-> (state [12] as doubles, sigma11 / sigma1, sigma12 / sigma1), or None where step 2 refuses the sample.  The state's
    entries are Python floats and may be inf or nan where the decomposition has nothing to say (a scale of zero in M)."""
    X6 = [[float(x) for x in X] for X in X6]
    if conditioned(X6) is None:
        return None
    with mp.workdps(DPS):
        P = [[mp.mpf(x) for x in X] for X in X6]
        m = [sum(P[i][c] for i in range(SAMPLE)) / 6 for c in range(3)]
        s = max(abs(P[i][c] - m[c]) for i in range(SAMPLE) for c in range(3))
        if s == 0:  # (six equal points whose mean in doubles is an ulp off: the definition goes on, there is nothing to restate)
            return [math.nan] * 12, 0.0, 0.0
        A = mp.zeros(12, 12)
        for i in range(SAMPLE):
            x = (mp.mpf(float(uv6[i][0])) - mp.mpf(cu)) / mp.mpf(f)
            y = (mp.mpf(float(uv6[i][1])) - mp.mpf(cv)) / mp.mpf(f)
            q = [(P[i][c] - m[c]) / s for c in range(3)] + [mp.mpf(1)]
            for j in range(4):
                A[2 * i, j] = q[j]
                A[2 * i, 8 + j] = -x * q[j]
                A[2 * i + 1, 4 + j] = q[j]
                A[2 * i + 1, 8 + j] = -y * q[j]
        _, S, V = mp.svd_r(A)  # A = U diag(S) V, S decreasing: the rows of V are the right vectors
        p = [V[11, j] for j in range(12)]
        M = mp.matrix(3, 3)
        for i in range(3):
            for j in range(3):
                M[i, j] = p[4 * i + j]
        U3, w, V3 = mp.svd_r(M)
        R0 = U3 * V3
        sigma = 1 if mp.det(R0) > 0 else -1
        wsum = w[0] + w[1] + w[2]
        state = [math.nan] * 12
        if wsum > 0:
            lam = sigma * 3 / wsum
            for i in range(3):
                for j in range(3):
                    state[4 * i + j] = float(sigma * R0[i, j])
                state[4 * i + 3] = float(lam * p[4 * i + 3] * s - sigma * (R0[i, 0] * m[0] + R0[i, 1] * m[1] + R0[i, 2] * m[2]))
        return state, float(S[10] / S[0]), float(S[11] / S[0])


def in_front(S, X, min_depth):
    """a sampled point's depth at the state, as the row test forms it"""
    zc = X[0] * S[8] + X[1] * S[9] + X[2] * S[10] + S[11]
    return zc > min_depth


def valid(S, X6, min_depth):
    """the hypothesis' validity: twelve finite numbers, six points in front"""
    return all(math.isfinite(x) for x in S) and all(in_front(S, [float(x) for x in X], min_depth) for X in X6)


# ---- count and winner -----------------------------------------------------------------------------------------------------------

def eligible(uv, xyz):
    return np.isfinite(np.asarray(uv, dtype=np.float64)).all(axis=1) & np.isfinite(np.asarray(xyz, dtype=np.float64)).all(axis=1)


def residual(S, X, u, v, f, cu, cv, min_depth=1e-10):
    """a row's ru^2 + rv^2 at the state as the row test forms it, or None behind min_depth"""
    t = R.row_terms([float(x) for x in S], [float(x) for x in X], float(np.float32(u)), float(np.float32(v)), float(f), float(cu), float(cv), min_depth, math.inf, False)
    return None if t is None else t[27][0]


def count(S, uv, xyz, f, cu, cv, inlier_threshold=2.0, min_depth=1e-10):
    """the eligible rows with zc > min_depth and ru^2 + rv^2 < inlier_threshold^2"""
    limit = inlier_threshold * inlier_threshold
    S = [float(x) for x in S]
    n = 0
    for (u, v), X, ok in zip(uv, xyz, eligible(uv, xyz)):
        if ok and R.row_terms(S, [float(x) for x in X], float(np.float32(u)), float(np.float32(v)), float(f), float(cu), float(cv), min_depth, limit, False) is not None:
            n += 1
    return n


def winner(counts, hvalid, min_inliers):
    """-> (verdict, best, inliers): the first hypothesis with strictly more inliers than all before it"""
    best, top, any_valid = -1, 0, False
    for k, (c, ok) in enumerate(zip(counts, hvalid)):
        if not ok:
            continue
        any_valid = True
        if int(c) > top:
            best, top = k, int(c)
    verdict = 3 if not any_valid else (4 if top < min_inliers else 0)
    return verdict, best, top
