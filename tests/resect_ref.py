"""The definition of the pose refinement (include/visomatch.h, vsm_resect_run; csrc/vsm_resect.h), restated for the tests in
plain Python floats: one operation per expression step, nothing vectorised, so the order of every sum - the 256 partial sums
and their tree included - can be read off the page.  Nothing comes from the library; the 6x6 Matrix::solve is restated below
the way tests/points_ref.py restates the 3x3 one."""
import math

import numpy as np

DEFAULTS = dict(min_observations=10, max_updates=20, eps=1e-8, max_residual=0.0, min_depth=1e-10)
LANES, SUMS = 256, 28


def solve6(A, B, eps=1e-20):
    """Matrix::solve for a 6x6 A (list of rows) and a 6-vector B, both overwritten: Gauss-Jordan with full pivoting"""
    m = 6
    ipiv = [0] * m
    for _ in range(m):
        big = 0.0
        irow = icol = 0
        for j in range(m):
            if ipiv[j] != 1:
                for k in range(m):
                    if ipiv[k] == 0:
                        if abs(A[j][k]) >= big:
                            big = abs(A[j][k])
                            irow = j
                            icol = k
        ipiv[icol] += 1
        if irow != icol:
            A[irow], A[icol] = A[icol], A[irow]
            B[irow], B[icol] = B[icol], B[irow]
        if abs(A[icol][icol]) < eps:
            return False
        pivinv = 1.0 / A[icol][icol]
        A[icol][icol] = 1.0
        for l in range(m):
            A[icol][l] = A[icol][l] * pivinv
        B[icol] = B[icol] * pivinv
        for ll in range(m):
            if ll != icol:
                dum = A[ll][icol]
                A[ll][icol] = 0.0
                for l in range(m):
                    A[ll][l] = A[ll][l] - A[icol][l] * dum
                B[ll] = B[ll] - B[icol] * dum
    return True


def rigid_inverse(p):
    """12 floats, rows 0..2 of [R | c] -> [R^T | -R^T c], the last column summed over k ascending from the k = 0 product"""
    out = [0.0] * 12
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = p[4 * j + i]
        s = p[0 + i] * p[3]
        s = s + p[4 + i] * p[7]
        s = s + p[8 + i] * p[11]
        out[4 * i + 3] = -s
    return out


def row_terms(S, X, u, v, f, cu, cv, min_depth, limit, jacobian):
    """None for a skipped row, else the row's 28 pairs of terms as a list of tuples (sum 27: one term)"""
    xc = X[0] * S[0] + X[1] * S[1] + X[2] * S[2] + S[3]
    yc = X[0] * S[4] + X[1] * S[5] + X[2] * S[6] + S[7]
    zc = X[0] * S[8] + X[1] * S[9] + X[2] * S[10] + S[11]
    if not zc > min_depth:
        return None
    ru = u - (f * xc / zc + cu)
    rv = v - (f * yc / zc + cv)
    t = ru * ru + rv * rv
    if not t < limit:
        return None
    if not jacobian:
        return [()] * 27 + [(t,)]
    zz = zc * zc
    dx = (0.0, zc, -yc, 1.0, 0.0, 0.0)
    dy = (-zc, 0.0, xc, 0.0, 1.0, 0.0)
    dz = (yc, -xc, 0.0, 0.0, 0.0, 1.0)
    ju = [f * (dx[j] * zc - xc * dz[j]) / zz for j in range(6)]
    jv = [f * (dy[j] * zc - yc * dz[j]) / zz for j in range(6)]
    terms = []
    for m in range(6):
        for c in range(m, 6):
            terms.append((ju[m] * ju[c], jv[m] * jv[c]))
    for m in range(6):
        terms.append((ju[m] * ru, jv[m] * rv))
    terms.append((t,))
    return terms


def evaluate(S, rows, xyz, f, cu, cv, prm, jacobian):
    """-> (the 28 sums, the count of used rows): 256 partial sums, then the tree"""
    limit = prm["max_residual"] * prm["max_residual"] if prm["max_residual"] > 0 else math.inf
    partial = [[0.0] * SUMS for _ in range(LANES)]
    used = 0
    for i, (t, u, v) in enumerate(rows):
        terms = row_terms(S, xyz[t], u, v, f, cu, cv, prm["min_depth"], limit, jacobian)
        if terms is None:
            continue
        used += 1
        acc = partial[i % LANES]
        for k in range(SUMS):
            for x in terms[k]:
                acc[k] = acc[k] + x
    s = LANES // 2
    while s >= 1:
        for l in range(s):
            for k in range(SUMS):
                partial[l][k] = partial[l][k] + partial[l + s][k]
        s //= 2
    return partial[0], used


def step(sums, S, eps):
    """'no_pivot' (S untouched) | 'updated' | 'converged' (S moved)"""
    A = [[0.0] * 6 for _ in range(6)]
    k = 0
    for m in range(6):
        for c in range(m, 6):
            A[m][c] = sums[k]
            A[c][m] = sums[k]
            k += 1
    d = [sums[21 + m] for m in range(6)]
    if not solve6(A, d):
        return "no_pivot"
    a = [0.5 * d[0], 0.5 * d[1], 0.5 * d[2]]
    aa = a[0] * a[0] + a[1] * a[1] + a[2] * a[2]
    den = 1.0 + aa
    one = 1.0 - aa
    Rd = [[(one + 2.0 * (a[0] * a[0])) / den, (2.0 * (a[0] * a[1]) - 2.0 * a[2]) / den, (2.0 * (a[0] * a[2]) + 2.0 * a[1]) / den],
          [(2.0 * (a[1] * a[0]) + 2.0 * a[2]) / den, (one + 2.0 * (a[1] * a[1])) / den, (2.0 * (a[1] * a[2]) - 2.0 * a[0]) / den],
          [(2.0 * (a[2] * a[0]) - 2.0 * a[1]) / den, (2.0 * (a[2] * a[1]) + 2.0 * a[0]) / den, (one + 2.0 * (a[2] * a[2])) / den]]
    N = [0.0] * 12
    for i in range(3):
        for j in range(4):
            x = Rd[i][0] * S[0 + j]
            x = x + Rd[i][1] * S[4 + j]
            x = x + Rd[i][2] * S[8 + j]
            N[4 * i + j] = x
        N[4 * i + 3] = N[4 * i + 3] + d[3 + i]
    S[:] = N
    for m in range(6):
        if not abs(d[m]) <= eps:
            return "updated"
    return "converged"


def frame(pose, valid, refine, rows, xyz, f, cu, cv, prm):
    """-> (status, pose, updates, rows, used, ss_before, ss_after, rms_before, rms_after)"""
    n = len(rows)
    if not valid:
        return 1, pose, 0, n, 0, 0.0, 0.0, 0.0, 0.0
    if not refine:
        return 2, pose, 0, n, 0, 0.0, 0.0, 0.0, 0.0
    if n < prm["min_observations"]:
        return 3, pose, 0, n, 0, 0.0, 0.0, 0.0, 0.0
    S = rigid_inverse(pose)
    updates, status = 0, 6
    ss_before, used_before = 0.0, 0
    while updates < prm["max_updates"]:
        sums, used = evaluate(S, rows, xyz, f, cu, cv, prm, True)
        if updates == 0:
            ss_before, used_before = sums[27], used
        rms_before = math.sqrt(ss_before / used_before) if used_before > 0 else 0.0
        if used < prm["min_observations"]:
            return 4, pose, updates, n, used, ss_before, 0.0, rms_before, 0.0
        r = step(sums, S, prm["eps"])
        if r == "no_pivot":
            return 5, pose, updates, n, used, ss_before, 0.0, rms_before, 0.0
        updates += 1
        if r == "converged":
            status = 0
            break
    sums, used = evaluate(S, rows, xyz, f, cu, cv, prm, False)
    ss_after = sums[27]
    rms_after = math.sqrt(ss_after / used) if used > 0 else 0.0
    return status, rigid_inverse(S), updates, n, used, ss_before, ss_after, rms_before, rms_after


class Ref:
    pass


FIELDS = ("status", "updates", "rows", "used", "poses", "ss_before", "ss_after", "rms_before", "rms_after")


def group(n_frames, offsets, obs_frames, uv, use):
    """the rows {track, u, v} of every frame, in ascending (track, observation)"""
    rows = [[] for _ in range(n_frames)]
    for t in range(len(offsets) - 1):
        if use is not None and not use[t]:
            continue
        for i in range(int(offsets[t]), int(offsets[t + 1])):
            rows[int(obs_frames[i])].append((t, float(np.float32(uv[i][0])), float(np.float32(uv[i][1]))))
    return rows


def resect(poses, f, cu, cv, offsets, obs_frames, uv, xyz, use=None, refine=None, pose_valid=None, params=None):
    prm = dict(DEFAULTS)
    prm.update(params or {})
    poses = np.asarray(poses, dtype=np.float64).reshape(len(poses), -1)[:, :12] if len(poses) else np.zeros((0, 12))
    pts = [[float(x) for x in p] for p in np.asarray(xyz, dtype=np.float64).reshape(-1, 3)]
    uv = np.asarray(uv, dtype=np.float32).reshape(-1, 2)
    rows = group(len(poses), offsets, obs_frames, uv, use)
    out = []
    for g, po in enumerate(poses):
        out.append(frame([float(x) for x in po], pose_valid is None or bool(pose_valid[g]), refine is None or bool(refine[g]), rows[g], pts, float(f), float(cu),
                         float(cv), prm))
    r = Ref()
    F = len(out)
    r.status = np.array([x[0] for x in out], dtype=np.int32)
    r.poses = np.array([x[1] for x in out], dtype=np.float64).reshape(F, 12)
    r.updates = np.array([x[2] for x in out], dtype=np.int32)
    r.rows = np.array([x[3] for x in out], dtype=np.int32)
    r.used = np.array([x[4] for x in out], dtype=np.int32)
    for i, name in enumerate(("ss_before", "ss_after", "rms_before", "rms_after")):
        setattr(r, name, np.array([x[5 + i] for x in out], dtype=np.float64))
    return r


def assert_same(got, want, what=""):
    """every int, and every double by its bytes"""
    for name in FIELDS:
        a, b = np.ascontiguousarray(getattr(got, name)), np.ascontiguousarray(getattr(want, name))
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.nonzero((a.reshape(len(a), -1).view(np.uint8) != b.reshape(len(b), -1).view(np.uint8)).any(axis=1))[0]
            g = int(bad[0])
            raise AssertionError((what, name, "frames", bad[:10].tolist(), "first", g, a[g].tolist(), b[g].tolist(), "status", int(got.status[g]), int(want.status[g])))
