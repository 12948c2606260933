"""The definition of the vetting of observations (include/visomatch.h, vsm_vet_run; csrc/vsm_vet.h), restated for the tests in
plain Python floats: one operation per expression step, nothing vectorised, so the order of a track's sum - the 16 partial sums
and their tree - can be read off the page.  numpy.float32 serves the r2 conversion alone.  Nothing comes from the library.  The
row is the resection's: the state and the row evaluation are those of tests/resect_ref.py, and obs_code() below, which has to
tell "behind" from "gated" and needs the gated row's number too, is checked against resect_ref.row_terms on every row it sees."""
import math

import numpy as np

import resect_ref as R

DEFAULTS = dict(max_residual=2.0, min_depth=1e-10, min_observations=2)
LANES = 16
NO_FRAME = 0x7fffffff
FIELDS = ("code", "r2", "status", "n_in", "frame_lo", "frame_hi", "ss", "worst", "frame_counts", "kept_offsets", "kept_index")


def obs_code(S, X, u, v, in_use, valid, f, cu, cv, min_depth, limit):
    """-> (code, t): t is the double ru^2 + rv^2 for codes 0 and 4, None otherwise"""
    if not in_use:
        return 1, None
    if not valid:
        return 2, None
    terms = R.row_terms(S, X, u, v, f, cu, cv, min_depth, limit, False)
    zc = X[0] * S[8] + X[1] * S[9] + X[2] * S[10] + S[11]
    if not zc > min_depth:
        assert terms is None
        return 3, None
    xc = X[0] * S[0] + X[1] * S[1] + X[2] * S[2] + S[3]
    yc = X[0] * S[4] + X[1] * S[5] + X[2] * S[6] + S[7]
    ru = u - (f * xc / zc + cu)
    rv = v - (f * yc / zc + cv)
    t = ru * ru + rv * rv
    if not t < limit:
        assert terms is None
        return 4, t
    assert terms is not None and terms[27] == (t,)
    return 0, t


def to_float32(t):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(t)


class Ref:
    pass


def vet(poses, f, cu, cv, offsets, obs_frames, uv, xyz, use=None, pose_valid=None, params=None):
    prm = dict(DEFAULTS)
    prm.update(params or {})
    limit = prm["max_residual"] * prm["max_residual"] if prm["max_residual"] > 0 else math.inf
    poses = np.asarray(poses, dtype=np.float64).reshape(len(poses), -1)[:, :12] if len(poses) else np.zeros((0, 12))
    states = [R.rigid_inverse([float(x) for x in p]) for p in poses]
    pts = [[float(x) for x in p] for p in np.asarray(xyz, dtype=np.float64).reshape(-1, 3)]
    uv = np.asarray(uv, dtype=np.float32).reshape(-1, 2)
    f, cu, cv = float(f), float(cu), float(cv)
    T, n_obs, n_frames = len(offsets) - 1 if len(offsets) else 0, len(obs_frames), len(poses)
    code = np.zeros(n_obs, np.uint8)
    r2 = np.zeros(n_obs, np.float32)
    status, n_in, frame_lo, frame_hi = (np.zeros(T, np.int32) for _ in range(4))
    ss, worst = np.zeros(T, np.float64), np.zeros(T, np.float64)
    frame_counts = np.zeros((n_frames, 3), np.int32)
    kept_offsets, kept_index = [0], []
    for t in range(T):
        o, end = int(offsets[t]), int(offsets[t + 1])
        in_use = use is None or bool(use[t])
        partial = [0.0] * LANES
        count, lo, hi, big = 0, NO_FRAME, -1, 0.0
        inliers = []
        for i in range(o, end):
            g = int(obs_frames[i])
            c, tt = obs_code(states[g], pts[t], float(uv[i][0]), float(uv[i][1]), in_use, pose_valid is None or bool(pose_valid[g]), f, cu, cv, prm["min_depth"], limit)
            code[i] = c
            r2[i] = to_float32(tt) if c in (0, 4) else np.float32(0.0)
            if c == 0:
                partial[(i - o) % LANES] = partial[(i - o) % LANES] + tt
                count += 1
                lo, hi = min(lo, g), max(hi, g)
                big = tt if tt > big else big
                frame_counts[g][0] += 1
                inliers.append(i)
            elif c == 3:
                frame_counts[g][1] += 1
            elif c == 4:
                frame_counts[g][2] += 1
        s = LANES // 2
        while s >= 1:
            for l in range(s):
                partial[l] = partial[l] + partial[l + s]
            s //= 2
        if not in_use:
            st = 1
        elif count < prm["min_observations"]:
            st = 2
        elif lo == hi:
            st = 3
        else:
            st = 0
        status[t], n_in[t], frame_lo[t], frame_hi[t], ss[t], worst[t] = st, count, (lo if count else -1), hi, partial[0], big
        if st == 0:
            kept_index.extend(inliers)
        kept_offsets.append(len(kept_index))
    r = Ref()
    r.code, r.r2, r.status, r.n_in, r.frame_lo, r.frame_hi, r.ss, r.worst, r.frame_counts = code, r2, status, n_in, frame_lo, frame_hi, ss, worst, frame_counts
    r.kept_offsets, r.kept_index = np.array(kept_offsets, np.int32), np.array(kept_index, np.int32)
    return r


def assert_same(got, want, what=""):
    """every array by its bytes; where both hold a NaN (r2 alone can) the position counts, not the NaN's sign or payload"""
    for name in FIELDS:
        a, b = np.ascontiguousarray(getattr(got, name)), np.ascontiguousarray(getattr(want, name))
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        if a.dtype.kind == "f":
            na, nb = np.isnan(a), np.isnan(b)
            assert (na == nb).all(), (what, name, "NaN positions", np.nonzero(na != nb)[0][:10].tolist())
            a, b = np.where(na, 0, a), np.where(nb, 0, b)
        if a.tobytes() != b.tobytes():
            bad = np.nonzero((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(axis=1) | (np.signbit(a.reshape(len(a), -1)) != np.signbit(b.reshape(len(b), -1))).any(axis=1)
                             if a.dtype.kind == "f" else (a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(axis=1))[0]
            g = int(bad[0])
            raise AssertionError((what, name, "entries", bad[:10].tolist(), "first", g, a[g].tolist(), b[g].tolist()))
