"""The definition of track triangulation (include/visomatch.h, vsm_triangulate_run), restated for the tests in plain Python
floats: one operation per expression step, nothing vectorised, so the order of every sum can be read off the page.  Nothing
comes from the library.  The 4x4 SVD is the oracle's (oracle.bindings.oracle_svd, pinned to the reference's Matrix::svd by
test_mono_oracle.py); the 3x3 Matrix::solve (viso/matrix.cpp:424-519) is restated below."""
import math

import numpy as np

DEFAULTS = dict(point_type=1, min_track_length=2, max_dist=30.0, min_angle=2.0, cam_pitch=-0.08, cam_height=1.6)


def f32(x):
    """a float32 pixel as the Python float it widens to"""
    return float(np.float32(x))


def solve3(A, B, eps=1e-20):
    """Matrix::solve for a 3x3 A (list of rows) and a 3-vector B, both overwritten: Gauss-Jordan elimination with full pivoting.
    Returns False where the reference does (pivot below eps)."""
    m = 3
    ipiv = [0] * m
    irow = icol = 0
    for i in range(m):
        big = 0.0
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
            for l in range(m):
                A[irow][l], A[icol][l] = A[icol][l], A[irow][l]
            B[irow], B[icol] = B[icol], B[irow]
        if abs(A[icol][icol]) < eps:
            return False
        pivinv = 1.0 / A[icol][icol]
        A[icol][icol] = 1.0
        for l in range(m):
            A[icol][l] *= pivinv
        B[icol] *= pivinv
        for ll in range(m):
            if ll != icol:
                dum = A[ll][icol]
                A[ll][icol] = 0.0
                for l in range(m):
                    A[ll][l] -= A[icol][l] * dum
                B[ll] -= B[icol] * dum
    return True


def frame_matrices(pose, f, cu, cv):
    """pose: 12 floats, rows 0..2 of [R | c].  -> (inv 3x4, proj 3x4, c): inv = [R^T | -R^T c], proj = K * inv, every entry
    summed over k ascending from the k = 0 product"""
    R = [[pose[4 * i + j] for j in range(3)] for i in range(3)]
    c = [pose[3], pose[7], pose[11]]
    inv = []
    for i in range(3):
        s = R[0][i] * c[0]
        s = s + R[1][i] * c[1]
        s = s + R[2][i] * c[2]
        inv.append([R[0][i], R[1][i], R[2][i], -s])
    K = [[f, 0.0, cu], [0.0, f, cv], [0.0, 0.0, 1.0]]
    proj = []
    for i in range(3):
        row = []
        for j in range(4):
            s = K[i][0] * inv[0][j]
            s = s + K[i][1] * inv[1][j]
            s = s + K[i][2] * inv[2][j]
            row.append(s)
        proj.append(row)
    return inv, proj, c


def road_matrix(cam_pitch, cam_height):
    """rows 0..2 of Tr_cam_road (Reconstruction::setCalibration)"""
    return [[1.0, 0.0, 0.0, 0.0], [0.0, +math.cos(cam_pitch), -math.sin(cam_pitch), -cam_height], [0.0, +math.sin(cam_pitch), +math.cos(cam_pitch), 0.0]]


def affine(M, p):
    return [p[0] * M[r][0] + p[1] * M[r][1] + p[2] * M[r][2] + M[r][3] for r in range(3)]


def init_point(P1, P2, p1, p2, svd):
    J = [[0.0] * 4 for _ in range(4)]
    for j in range(4):
        J[0][j] = P1[2][j] * p1[0] - P1[0][j]
        J[1][j] = P1[2][j] * p1[1] - P1[1][j]
        J[2][j] = P2[2][j] * p2[0] - P2[0][j]
        J[3][j] = P2[2][j] * p2[1] - P2[1][j]
    _, _, V = svd(np.array(J, dtype=np.float64))
    w = float(V[3][3])
    if abs(w) < 1e-10:
        return None
    return [float(V[0][3]) / w, float(V[1][3]) / w, float(V[2][3]) / w]


def point_type(inv1, inv2, road, p):
    x1c = affine(inv1, p)
    x2c = affine(inv2, p)
    x2r = affine(road, x2c)
    if x1c[2] <= 1 or x2c[2] <= 1:
        return -1
    if x2r[1] > 0.5:
        return 0
    if x2r[1] > -1:
        return 1
    return 2


def update_point(projs, pixels, p):
    """updatePoint(step 1, eps 1e-5) over all observations: 'failed' | 'updated' | 'converged'; p is changed in place"""
    J, res = [], []  # J: 2n rows of 3, res: 2n residuals
    for P, (u, v) in zip(projs, pixels):
        a = P[0][0] * p[0] + P[0][1] * p[1] + P[0][2] * p[2] + P[0][3]
        b = P[1][0] * p[0] + P[1][1] * p[1] + P[1][2] * p[2] + P[1][3]
        c = P[2][0] * p[0] + P[2][1] * p[1] + P[2][2] * p[2] + P[2][3]
        cc = c * c
        if cc < 1e-10:
            return "failed"
        J.append([(P[0][0] * c - P[2][0] * a) / cc, (P[0][1] * c - P[2][1] * a) / cc, (P[0][2] * c - P[2][2] * a) / cc])
        J.append([(P[1][0] * c - P[2][0] * b) / cc, (P[1][1] * c - P[2][1] * b) / cc, (P[1][2] * c - P[2][2] * b) / cc])
        res.append(u - a / c)
        res.append(v - b / c)
    A = [[0.0] * 3 for _ in range(3)]
    B = [0.0] * 3
    for m in range(3):
        for n in range(3):
            s = 0.0
            for i in range(len(J)):
                s += J[i][m] * J[i][n]
            A[m][n] = s
        s = 0.0
        for i in range(len(J)):
            s += J[i][m] * res[i]
        B[m] = s
    if not solve3(A, B):
        return "failed"
    step, eps = 1.0, 1e-5
    p[0] += step * B[0]
    p[1] += step * B[1]
    p[2] += step * B[2]
    if abs(B[0]) < eps and abs(B[1]) < eps and abs(B[2]) < eps:
        return "converged"
    return "updated"


def track_point(frames, valid, road, fr, pixels, flagged, prm, svd):
    """-> (status, xyz, type, updates, dist, angle) of one track; frames[k] = (inv, proj, c)"""
    zero = [0.0, 0.0, 0.0]
    n = len(fr)
    if flagged:
        return 1, zero, -2, 0, 0.0, 0.0
    for k in fr:
        if not valid[k]:
            return 2, zero, -2, 0, 0.0, 0.0
    if n < prm["min_track_length"]:
        return 3, zero, -2, 0, 0.0, 0.0
    inv1, P1, c1 = frames[fr[0]]
    inv2, P2, c2 = frames[fr[-1]]
    p = init_point(P1, P2, pixels[0], pixels[-1], svd)
    if p is None:
        return 4, zero, -2, 0, 0.0, 0.0
    ty = point_type(inv1, inv2, road, p)
    if ty < prm["point_type"]:
        return 5, p, ty, 0, 0.0, 0.0
    projs = [frames[k][1] for k in fr]
    updates, it, result = 0, 0, "updated"
    while result == "updated":
        result = update_point(projs, pixels, p)
        updates += 1
        it += 1
        if it - 1 > 20 or result == "converged":
            break
    if result == "failed":
        return 6, p, ty, updates, 0.0, 0.0
    if result != "converged":
        return 7, p, ty, updates, 0.0, 0.0
    mid = (fr[0] + fr[-1]) // 2
    while not valid[mid]:
        mid -= 1
    cm = frames[mid][2]
    dx, dy, dz = cm[0] - p[0], cm[1] - p[1], cm[2] - p[2]
    dist = math.sqrt(dx * dx + dy * dy + dz * dz)
    if not dist < prm["max_dist"]:
        return 8, p, ty, updates, dist, 0.0
    v1 = [c1[i] - p[i] for i in range(3)]
    v2 = [c2[i] - p[i] for i in range(3)]
    n1 = 0.0
    for x in v1:
        n1 += x * x
    n2 = 0.0
    for x in v2:
        n2 += x * x
    n1, n2 = math.sqrt(n1), math.sqrt(n2)
    if n1 < 1e-10 or n2 < 1e-10:
        angle = 1000.0
    else:
        dot = 0.0
        for i in range(3):
            dot += (v1[i] / n1) * (v2[i] / n2)
        a = abs(dot)
        angle = math.acos(a) * 180.0 / math.pi if a <= 1.0 else float("nan")
    if not angle > prm["min_angle"]:
        return 9, p, ty, updates, dist, angle
    return 0, p, ty, updates, dist, angle


class Ref:
    pass


def triangulate(poses, f, cu, cv, offsets, obs_frames, uv, flags=None, pose_valid=None, params=None, svd=None):
    """-> object with status, type, updates (int32 [T]), xyz (float64 [T, 3]), dist, angle (float64 [T])"""
    if svd is None:
        from oracle.bindings import oracle_svd as svd
    prm = dict(DEFAULTS)
    prm.update(params or {})
    poses = np.asarray(poses, dtype=np.float64).reshape(len(poses), -1)[:, :12] if len(poses) else np.zeros((0, 12))
    frames = [frame_matrices([float(x) for x in po], float(f), float(cu), float(cv)) for po in poses]
    valid = [True] * len(frames) if pose_valid is None else [bool(x) for x in pose_valid]
    road = road_matrix(float(prm["cam_pitch"]), float(prm["cam_height"]))
    offsets = [int(x) for x in offsets]
    fr_all = [int(x) for x in obs_frames]
    px_all = [(f32(u), f32(v)) for u, v in np.asarray(uv, dtype=np.float32).reshape(-1, 2)]
    rows = []
    for t in range(len(offsets) - 1):
        a, b = offsets[t], offsets[t + 1]
        rows.append(track_point(frames, valid, road, fr_all[a:b], px_all[a:b], bool(flags[t] & 1) if flags is not None else False, prm, svd))
    r = Ref()
    r.status = np.array([x[0] for x in rows], dtype=np.int32)
    r.xyz = np.array([x[1] for x in rows], dtype=np.float64).reshape(-1, 3)
    r.type = np.array([x[2] for x in rows], dtype=np.int32)
    r.updates = np.array([x[3] for x in rows], dtype=np.int32)
    r.dist = np.array([x[4] for x in rows], dtype=np.float64)
    r.angle = np.array([x[5] for x in rows], dtype=np.float64)
    return r


FIELDS = ("status", "type", "updates", "xyz", "dist", "angle")


def assert_same(got, want, what=""):
    """every int, and every double by its bytes"""
    for name in FIELDS:
        a, b = np.ascontiguousarray(getattr(got, name)), np.ascontiguousarray(getattr(want, name))
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.nonzero((a.reshape(len(a), -1).view(np.uint8) != b.reshape(len(b), -1).view(np.uint8)).any(axis=1))[0]
            t = int(bad[0])
            raise AssertionError((what, name, "tracks", bad[:10].tolist(), "first", t, a[t].tolist(), b[t].tolist(), "status", int(got.status[t]), int(want.status[t])))
