"""The definition of the joint adjustment of poses and points (include/visomatch.h, vsm_adjust_run; csrc/vsm_ba.h), restated for
the tests in plain Python floats on the row of tests/resect_ref.py: one operation per expression step, nothing vectorised, so
the order of every sum - the 256 partial sums and their tree included - can be read off the page.  Nothing comes from the
library; the 6x6 solve and the rigid inverse are resect_ref's, the 3x3 inverse is restated below."""
import math

import numpy as np

import resect_ref as R

DEFAULTS = dict(min_observations=10, min_track_observations=2, max_rounds=10, cg_iters=40, lambda0=1e-3, lambda_min=1e-9, lambda_max=1e6, cg_tol=1e-2,
                ftol=1e-6, max_residual=0.0, min_depth=1e-10)
LANES = 256
HELD = 7


def tree(partial):
    """partial: LANES lists of K running sums -> the K sums"""
    s = LANES // 2
    while s >= 1:
        for l in range(s):
            for k in range(len(partial[l])):
                partial[l][k] = partial[l][k] + partial[l + s][k]
        s //= 2
    return partial[0]


def invert3(ab, eps=1e-20):
    """Gauss-Jordan with full pivoting on the 3x6 [V | I] (list of rows), overwritten: True, and columns 3..5 are the inverse"""
    ipiv = [0, 0, 0]
    for _ in range(3):
        big = 0.0
        irow = icol = 0
        for j in range(3):
            if ipiv[j] != 1:
                for k in range(3):
                    if ipiv[k] == 0:
                        if abs(ab[j][k]) >= big:
                            big = abs(ab[j][k])
                            irow, icol = j, k
        ipiv[icol] += 1
        if irow != icol:
            ab[irow], ab[icol] = ab[icol], ab[irow]
        if abs(ab[icol][icol]) < eps:
            return False
        pivinv = 1.0 / ab[icol][icol]
        ab[icol][icol] = 1.0
        for l in range(6):
            ab[icol][l] = ab[icol][l] * pivinv
        for ll in range(3):
            if ll != icol:
                dum = ab[ll][icol]
                ab[ll][icol] = 0.0
                for l in range(6):
                    ab[ll][l] = ab[ll][l] - ab[icol][l] * dum
    return True


def divide(a, b):
    """a / b as IEEE 754 has it, where Python raises"""
    if b != 0.0:
        return a / b
    return math.nan if (a == 0.0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)


def mul3(A, y):
    out = []
    for i in range(3):
        s = A[3 * i] * y[0]
        s = s + A[3 * i + 1] * y[1]
        s = s + A[3 * i + 2] * y[2]
        out.append(s)
    return out


def camera_point(S, X):
    return (X[0] * S[0] + X[1] * S[1] + X[2] * S[2] + S[3], X[0] * S[4] + X[1] * S[5] + X[2] * S[6] + S[7], X[0] * S[8] + X[1] * S[9] + X[2] * S[10] + S[11])


def move(S, d):
    """the Cayley step of delta d = (w, tau) on the state S (12 floats) -> the new state"""
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
    return N


def linearise_row(S, X, u, v, f, cu, cv, min_depth, limit):
    """None for an inactive row, else (the 28 tuples of terms of resect_ref.row_terms, W[18], pu[3], pv[3], (ru, rv))"""
    xc, yc, zc = camera_point(S, X)
    if not zc > min_depth:
        return None
    ru = u - (f * xc / zc + cu)
    rv = v - (f * yc / zc + cv)
    t = ru * ru + rv * rv
    if not t < limit:
        return None
    zz = zc * zc
    dx = (0.0, zc, -yc, 1.0, 0.0, 0.0)
    dy = (-zc, 0.0, xc, 0.0, 1.0, 0.0)
    dz = (yc, -xc, 0.0, 0.0, 0.0, 1.0)
    ju = [f * (dx[j] * zc - xc * dz[j]) / zz for j in range(6)]
    jv = [f * (dy[j] * zc - yc * dz[j]) / zz for j in range(6)]
    pu = [f * (S[0 + j] * zc - xc * S[8 + j]) / zz for j in range(3)]
    pv = [f * (S[4 + j] * zc - yc * S[8 + j]) / zz for j in range(3)]
    terms = []
    for m in range(6):
        for c in range(m, 6):
            terms.append((ju[m] * ju[c], jv[m] * jv[c]))
    for m in range(6):
        terms.append((ju[m] * ru, jv[m] * rv))
    terms.append((t,))
    W = []
    for m in range(6):
        for j in range(3):
            s = ju[m] * pu[j]
            s = s + jv[m] * pv[j]
            W.append(s)
    return terms, W, pu, pv, (ru, rv)


class State:
    pass


def group(n_frames, offsets, obs_frames, uv, use):
    """the rows (track, observation, u, v) of every frame, in ascending (track, observation)"""
    rows = [[] for _ in range(n_frames)]
    for t in range(len(offsets) - 1):
        if use is not None and not use[t]:
            continue
        for i in range(int(offsets[t]), int(offsets[t + 1])):
            rows[int(obs_frames[i])].append((t, i, float(np.float32(uv[i][0])), float(np.float32(uv[i][1]))))
    return rows


def dot(a, b, ffree):
    partial = [[0.0] for _ in range(LANES)]
    for i in range(len(a)):
        if ffree[i // 6]:
            partial[i % LANES][0] = partial[i % LANES][0] + a[i] * b[i]
    return tree(partial)[0]


def wz_sums(rows, active, tfree, lin, zt):
    partial = [[0.0] * 6 for _ in range(LANES)]
    for i, (t, o, _, _) in enumerate(rows):
        if not active[o] or not tfree[t]:
            continue
        W, acc = lin[o][0], partial[i % LANES]
        for m in range(6):
            for j in range(3):
                acc[m] = acc[m] + W[3 * m + j] * zt[t][j]
    return tree(partial)


def wt_sum(t, vec, offsets, obs_frames, active, ffree, lin):
    y = [0.0, 0.0, 0.0]
    for i in range(int(offsets[t]), int(offsets[t + 1])):
        g = int(obs_frames[i])
        if not active[i] or not ffree[g]:
            continue
        W = lin[i][0]
        for j in range(3):
            for m in range(6):
                y[j] = y[j] + W[3 * m + j] * vec[6 * g + m]
    return y


def inverse6(U):
    """U^-1 (36 floats, row-major) column after column: the 6x6 solve on a copy with the unit vector as right-hand side"""
    inv = [0.0] * 36
    for c in range(6):
        e = [1.0 if m == c else 0.0 for m in range(6)]
        R.solve6([list(U[6 * m:6 * m + 6]) for m in range(6)], e)
        for m in range(6):
            inv[6 * m + c] = e[m]
    return inv


def precond(Ui, r6):
    z = []
    for m in range(6):
        s = Ui[6 * m] * r6[0]
        for c in range(1, 6):
            s = s + Ui[6 * m + c] * r6[c]
        z.append(s)
    return z


def adjust(poses, f, cu, cv, offsets, obs_frames, uv, xyz, use=None, refine=None, pose_valid=None, params=None):
    prm = dict(DEFAULTS)
    prm.update(params or {})
    poses = np.asarray(poses, dtype=np.float64).reshape(len(poses), -1)[:, :12] if len(poses) else np.zeros((0, 12))
    xyz_in = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    F, T = len(poses), len(offsets) - 1
    f, cu, cv = float(f), float(cu), float(cv)
    uv = np.asarray(uv, dtype=np.float32).reshape(-1, 2)
    n_obs = int(offsets[T]) if T > 0 else 0
    rows = group(F, offsets, obs_frames, uv, use)
    valid = [pose_valid is None or bool(pose_valid[g]) for g in range(F)]
    asked = [refine is None or bool(refine[g]) for g in range(F)]
    in_use = [use is None or bool(use[t]) for t in range(T)]
    limit = prm["max_residual"] * prm["max_residual"] if prm["max_residual"] > 0 else math.inf
    tol2 = prm["cg_tol"] * prm["cg_tol"]
    # the state
    S = [R.rigid_inverse([float(x) for x in p]) for p in poses]
    X = [[float(x) for x in p] for p in xyz_in[:T]]
    moved, tmoved = [False] * F, [False] * T
    lam = prm["lambda0"]
    history = []
    fstatus, factive, tstatus = [0] * F, [0] * F, [0] * T
    stop = n_accepted = total_cg = 0
    while not stop:
        # ---- linearise ----
        active = [False] * n_obs
        lin = [None] * n_obs
        usum, cnt = [], []
        for g in range(F):
            partial = [[0.0] * 28 for _ in range(LANES)]
            count = 0
            if valid[g]:
                for i, (t, o, u, v) in enumerate(rows[g]):
                    got = linearise_row(S[g], X[t], u, v, f, cu, cv, prm["min_depth"], limit)
                    if got is None:
                        continue
                    active[o] = True
                    count += 1
                    lin[o] = got[1:]
                    acc = partial[i % LANES]
                    for k in range(28):
                        for x in got[0][k]:
                            acc[k] = acc[k] + x
            usum.append(tree(partial))
            cnt.append(count)
        # ---- the tracks' systems ----
        damp = 1.0 + lam
        tfree, vinv, gp, zt = [False] * T, [None] * T, [None] * T, [None] * T
        for t in range(T):
            if not in_use[t]:
                tstatus[t] = 1
                continue
            acc, n = [0.0] * 9, 0
            for i in range(int(offsets[t]), int(offsets[t + 1])):
                if not active[i]:
                    continue
                n += 1
                _, pu, pv, r = lin[i]
                k = 0
                for a in range(3):
                    for c in range(a, 3):
                        acc[k] = acc[k] + pu[a] * pu[c]
                        acc[k] = acc[k] + pv[a] * pv[c]
                        k += 1
                for a in range(3):
                    acc[6 + a] = acc[6 + a] + pu[a] * r[0]
                    acc[6 + a] = acc[6 + a] + pv[a] * r[1]
            gp[t] = acc[6:9]
            if n < prm["min_track_observations"]:
                tstatus[t] = 2
                continue
            ab = [[0.0] * 6 for _ in range(3)]
            k = 0
            for a in range(3):
                for c in range(a, 3):
                    ab[a][c] = acc[k]
                    ab[c][a] = acc[k]
                    k += 1
            for a in range(3):
                ab[a][a] = ab[a][a] * damp
                ab[a][3 + a] = 1.0
            if not invert3(ab):
                tstatus[t] = 3
                continue
            vinv[t] = [ab[a][3 + c] for a in range(3) for c in range(3)]
            tstatus[t] = 0
            tfree[t] = True
            zt[t] = mul3(vinv[t], gp[t])
        # ---- the frames' damped systems, who is free, the right-hand side ----
        ffree, Ud, Ui, b = [False] * F, [None] * F, [None] * F, [0.0] * (6 * F)
        for g in range(F):
            acc = wz_sums(rows[g], active, tfree, lin, zt)
            sums = usum[g]
            U = [0.0] * 36
            k = 0
            for m in range(6):
                for c in range(m, 6):
                    U[6 * m + c] = sums[k]
                    U[6 * c + m] = sums[k]
                    k += 1
            for m in range(6):
                U[6 * m + m] = U[6 * m + m] * damp
            Ud[g] = U
            st = 1 if not valid[g] else 2 if not asked[g] else 3 if len(rows[g]) < prm["min_observations"] else 0
            if st == 0:
                if cnt[g] >= prm["min_observations"]:
                    ffree[g] = R.solve6([list(U[6 * m:6 * m + 6]) for m in range(6)], [sums[21 + m] for m in range(6)])
                if ffree[g]:
                    Ui[g] = inverse6(U)
                else:
                    st = HELD
            fstatus[g], factive[g] = st, cnt[g]
            if ffree[g]:
                for m in range(6):
                    b[6 * g + m] = sums[21 + m] - acc[m]
        # ---- conjugate gradients ----
        x, r, z, q = [0.0] * (6 * F), list(b), [0.0] * (6 * F), [0.0] * (6 * F)
        for g in range(F):
            if ffree[g]:
                z[6 * g:6 * g + 6] = precond(Ui[g], r[6 * g:6 * g + 6])
        p = list(z)
        rz = rz0 = dot(r, z, ffree)
        iters, end = 0, 0
        if rz <= tol2 * rz0:
            end = 1
        while not end:
            for t in range(T):
                if tfree[t]:
                    zt[t] = mul3(vinv[t], wt_sum(t, p, offsets, obs_frames, active, ffree, lin))
            for g in range(F):
                if not ffree[g]:
                    continue
                acc = wz_sums(rows[g], active, tfree, lin, zt)
                for m in range(6):
                    s = Ud[g][6 * m] * p[6 * g]
                    for c in range(1, 6):
                        s = s + Ud[g][6 * m + c] * p[6 * g + c]
                    q[6 * g + m] = s - acc[m]
            pq = dot(p, q, ffree)
            if not (pq > 0.0 and pq < math.inf):
                end = 2
                break
            alpha = rz / pq
            for g in range(F):
                if not ffree[g]:
                    continue
                for i in range(6 * g, 6 * g + 6):
                    x[i] = x[i] + alpha * p[i]
                    r[i] = r[i] - alpha * q[i]
                z[6 * g:6 * g + 6] = precond(Ui[g], r[6 * g:6 * g + 6])
            rz_new = dot(r, z, ffree)
            iters += 1
            if rz_new <= tol2 * rz0:
                end = 1
            elif iters >= prm["cg_iters"]:
                end = 3
            beta = divide(rz_new, rz)
            rz = rz_new
            if end:
                break
            for g in range(F):
                if ffree[g]:
                    for i in range(6 * g, 6 * g + 6):
                        p[i] = z[i] + beta * p[i]
        # ---- back-substitution, the trial state ----
        Xt, St = [], []
        for t in range(T):
            if not tfree[t]:
                Xt.append(X[t])
                continue
            s = wt_sum(t, x, offsets, obs_frames, active, ffree, lin)
            dX = mul3(vinv[t], [gp[t][a] - s[a] for a in range(3)])
            Xt.append([X[t][a] + dX[a] for a in range(3)])
        for g in range(F):
            St.append(move(S[g], x[6 * g:6 * g + 6]) if ffree[g] else S[g])
        # ---- the trial cost over the same active rows ----
        cost = trial = 0.0
        behind, n_active = False, 0
        for g in range(F):
            if not valid[g]:
                continue
            partial = [[0.0] for _ in range(LANES)]
            for i, (t, o, u, v) in enumerate(rows[g]):
                if not active[o]:
                    continue
                xc, yc, zc = camera_point(St[g], Xt[t])
                if not zc > prm["min_depth"]:
                    behind = True
                    continue
                ru = u - (f * xc / zc + cu)
                rv = v - (f * yc / zc + cv)
                partial[i % LANES][0] = partial[i % LANES][0] + (ru * ru + rv * rv)
            cost = cost + usum[g][27]
            trial = trial + tree(partial)[0]
            n_active += cnt[g]
        # ---- the decision ----
        accept = (not behind) and trial < math.inf and trial < cost
        history.append((cost, trial if accept else cost, lam, iters, end, int(accept), n_active))
        total_cg += iters
        if accept:
            n_accepted += 1
            if cost - trial <= prm["ftol"] * cost:
                stop = 1
            lam = lam / 10.0
            if lam < prm["lambda_min"]:
                lam = prm["lambda_min"]
            for g in range(F):
                if ffree[g]:
                    S[g], moved[g] = St[g], True
            for t in range(T):
                if tfree[t]:
                    X[t], tmoved[t] = Xt[t], True
        else:
            lam = lam * 10.0
        if not stop and lam > prm["lambda_max"]:
            stop = 2
        if not stop and len(history) >= prm["max_rounds"]:
            stop = 3
    out = State()
    out.frame_status = np.array(fstatus, dtype=np.int32)
    out.poses = np.array([R.rigid_inverse(S[g]) if moved[g] else [float(x) for x in poses[g]] for g in range(F)], dtype=np.float64).reshape(F, 12)
    for g in range(F):  # (an unmoved frame keeps the input's bytes, a NaN's payload included)
        if not moved[g]:
            out.poses[g] = poses[g]
    out.rows = np.array([len(r) for r in rows], dtype=np.int32)
    out.active = np.array(factive, dtype=np.int32)
    out.track_status = np.array(tstatus, dtype=np.int32)
    out.xyz = np.array(X, dtype=np.float64).reshape(T, 3)
    for t in range(T):  # (likewise a point that was never moved)
        if not tmoved[t]:
            out.xyz[t] = xyz_in[t]
    out.history = history
    out.stats = dict(frames=np.bincount(out.frame_status, minlength=8).tolist(), tracks=np.bincount(out.track_status, minlength=4).tolist(), rounds=len(history),
                     rounds_accepted=n_accepted, stop=stop, cg_iterations=total_cg)
    return out


INT_FIELDS = ("frame_status", "rows", "active", "track_status")
DOUBLE_FIELDS = ("poses", "xyz")
HISTORY = ("cost_before", "cost_after", "lambda", "cg_iters", "cg_end", "accepted", "active")


def history_of(res):
    """a result's history as a list of tuples, whichever side it comes from"""
    h = res.history
    if isinstance(h, np.ndarray):
        return [tuple(rec[n].item() for n in HISTORY) for rec in h]
    return [tuple(rec) for rec in h]


def stats_of(res):
    s = res.stats
    if "frames" in s:
        return s["frames"] + s["tracks"] + [s["rounds"], s["rounds_accepted"], s["stop"], s["cg_iterations"]]
    return list(s.values())


def assert_same(got, want, what=""):
    """every int, and every double by its bytes"""
    hg, hw = history_of(got), history_of(want)
    assert len(hg) == len(hw), (what, "rounds", len(hg), len(hw), hg, hw)
    for k, (a, b) in enumerate(zip(hg, hw)):
        assert np.array(a[:3], dtype=np.float64).tobytes() == np.array(b[:3], dtype=np.float64).tobytes() and a[3:] == b[3:], (what, "round", k, a, b)
    for name in INT_FIELDS + DOUBLE_FIELDS:
        a, b = np.ascontiguousarray(getattr(got, name)), np.ascontiguousarray(getattr(want, name))
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.nonzero((a.reshape(len(a), -1).view(np.uint8) != b.reshape(len(b), -1).view(np.uint8)).any(axis=1))[0]
            g = int(bad[0])
            raise AssertionError((what, name, "items", bad[:10].tolist(), "first", g, a[g].tolist(), b[g].tolist()))
    assert stats_of(got) == stats_of(want), (what, stats_of(got), stats_of(want))
