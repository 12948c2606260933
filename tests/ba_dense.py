"""A second definition of the joint adjustment, for the tests: dense, in numpy alone, and sharing nothing with the library's - not
its header, not its restatement (tests/ba_ref.py), not its parameterisation.  What is minimised is stated from scratch: over
the observations (frame g, track t, pixel (u, v)) the sum of |(u, v) - (f x / z + cu, f y / z + cv)|^2 with (x, y, z) = R_g X_t
+ t_g, where the pose [Rc | c] of frame g (camera to world) gives R = Rc^T and t = -Rc^T c.

A frame's step is (w, tau): R <- exp(w) R by Rodrigues' formula, exactly, and t <- t + tau (the library turns the whole camera
frame, t included, by a Cayley rotation: another chart of the same poses).  A point's step is added.  The Jacobian below is
written for this chart; the damped normal equations (J^T J + lambda diag(J^T J)) d = -J^T r are formed and solved densely, a
step is kept if it lowers the cost, lambda goes down by ten after a kept step and up by ten after one that is not.  Frames that
are not asked for or have no valid pose are held, and so are points with fewer than two rows.

The gauge.  The root of the tests' scenes is held; that takes six of a monocular problem's seven free directions.  The seventh
is left: every centre and every point scaled about the root's centre projects to the same pixels, so the minimum is a line of
states, one per scale, and where on it a method ends depends on its path (this reference ends at scales 1e-3 apart from two
starts, with costs 3e-15 apart).  Cost and gradient do not see the scale.  States are compared at one scale: to_scale brings a
state's centres to the other's root-mean-square distance from the root.

The state is carried in np.longdouble, so that a step far below one ulp of a double state is not lost; a round's residuals,
Jacobian, solve and cost comparison are double arithmetic (`work`), which makes minimise a double-precision route to the
minimum as the library is one, by other formulae.  cost and gradient, as the tests call them, evaluate in np.longdouble.

LIMITS: what the tests allow between the library's result and this reference is 100 times what this reference differs from
itself by (see the table at the end), measured by `python tests/ba_dense.py`."""
import numpy as np

LD = np.longdouble
ROUNDS = 40


class Behind(ValueError):
    pass


class Problem:
    """the observations and who is free, from a case of tests/resect_cases.Case's fields"""

    def __init__(self, case):
        F, T = len(case.poses), len(case.offsets) - 1
        off = np.asarray(case.offsets, dtype=np.int64)
        track = np.repeat(np.arange(T), np.diff(off))
        frame = np.asarray(case.obs_frames, dtype=np.int64)[:off[T]]
        valid = np.ones(F, bool) if case.pose_valid is None else np.asarray(case.pose_valid, dtype=bool)
        asked = np.ones(F, bool) if case.refine is None else np.asarray(case.refine, dtype=bool)
        used = np.ones(T, bool) if case.use is None else np.asarray(case.use, dtype=bool)
        keep = used[track] & valid[frame]
        self.track, self.frame = track[keep], frame[keep]
        self.uv = np.asarray(case.uv, dtype=np.float32).reshape(-1, 2)[:off[T]][keep]
        self.f, self.cu, self.cv = case.f, case.cu, case.cv
        self.free_frames = np.nonzero(valid & asked & (np.bincount(self.frame, minlength=F) > 0))[0]
        self.free_tracks = np.nonzero(used & (np.bincount(self.track, minlength=T) >= 2))[0]
        self.n_frames, self.n_tracks = F, T


def split(poses, dtype=LD):
    """poses [Rc | c] -> world to camera (R, t)"""
    P = np.asarray(poses, dtype=dtype).reshape(-1, 3, 4)
    R = np.transpose(P[:, :, :3], (0, 2, 1)).copy()
    return R, -np.einsum("gij,gj->gi", R, P[:, :, 3])


def join(R, t):
    Rc = np.transpose(R, (0, 2, 1))
    return np.concatenate([Rc, -np.einsum("gij,gj->gi", Rc, t)[:, :, None]], axis=2).reshape(-1, 12)


def skew(a):
    S = np.zeros(a.shape[:-1] + (3, 3), dtype=a.dtype)
    S[..., 0, 1], S[..., 0, 2], S[..., 1, 0] = -a[..., 2], a[..., 1], a[..., 2]
    S[..., 1, 2], S[..., 2, 0], S[..., 2, 1] = -a[..., 0], -a[..., 1], a[..., 0]
    return S


def rodrigues(w):
    """exp of the skew matrices of w (n x 3)"""
    th2 = (w * w).sum(axis=1)
    th = np.sqrt(th2)
    small = th < 1e-6
    safe = np.where(small, 1, th)
    a = np.where(small, 1 - th2 / 6, np.sin(safe) / safe)
    b = np.where(small, 0.5 - th2 / 24, (1 - np.cos(safe)) / (safe * safe))
    K = skew(w)
    return np.eye(3, dtype=w.dtype) + a[:, None, None] * K + b[:, None, None] * (K @ K)


def residuals(pb, R, t, X, jacobian=False):
    """r (n x 2) in the dtype of R; with jacobian=True also J, 2 n x (6 free frames + 3 free tracks), of r in (w, tau) and dX"""
    dt = R.dtype
    Rg = R[pb.frame]
    RX = np.einsum("nij,nj->ni", Rg, X[pb.track])
    xc = RX + t[pb.frame]
    z = xc[:, 2]
    if not (z > 0).all():
        raise Behind("a point behind its camera: not a state for this reference")
    f = dt.type(pb.f)
    r = pb.uv.astype(dt) - (f * xc[:, :2] / z[:, None] + np.array([pb.cu, pb.cv], dtype=dt))
    if not jacobian:
        return r
    n = len(z)
    D = np.zeros((n, 2, 3), dtype=dt)  # d(projection) / d(x, y, z)
    D[:, 0, 0] = D[:, 1, 1] = f / z
    D[:, 0, 2], D[:, 1, 2] = -f * xc[:, 0] / (z * z), -f * xc[:, 1] / (z * z)
    Jw = D @ -skew(RX)                 # exp(w) R X + t = R X + w x R X + ..: d / dw = -[R X]x
    JX = D @ Rg
    col_f = np.full(pb.n_frames, -1)
    col_f[pb.free_frames] = 6 * np.arange(len(pb.free_frames))
    col_t = np.full(pb.n_tracks, -1)
    col_t[pb.free_tracks] = 6 * len(pb.free_frames) + 3 * np.arange(len(pb.free_tracks))
    J = np.zeros((2 * n, 6 * len(pb.free_frames) + 3 * len(pb.free_tracks)), dtype=dt)
    rows = np.arange(n)
    for e in range(2):
        on = col_f[pb.frame] >= 0
        for k in range(3):
            J[2 * rows[on] + e, col_f[pb.frame[on]] + k] = -Jw[on, e, k]
            J[2 * rows[on] + e, col_f[pb.frame[on]] + 3 + k] = -D[on, e, k]
        on = col_t[pb.track] >= 0
        for k in range(3):
            J[2 * rows[on] + e, col_t[pb.track[on]] + k] = -JX[on, e, k]
    return r, J


def moved(pb, R, t, X, d):
    """the state after the step d"""
    nf = len(pb.free_frames)
    d = d.astype(R.dtype)
    R, t, X = R.copy(), t.copy(), X.copy()
    df = d[:6 * nf].reshape(nf, 6)
    R[pb.free_frames] = rodrigues(df[:, :3]) @ R[pb.free_frames]
    t[pb.free_frames] += df[:, 3:]
    X[pb.free_tracks] += d[6 * nf:].reshape(-1, 3)
    return R, t, X


def state_of(case):
    return np.asarray(case.poses, dtype=LD), np.asarray(case.xyz, dtype=LD)


def cost(state, case, dtype=LD):
    """the sum of the squared residuals of a state (poses [Rc | c], points)"""
    R, t = split(state[0], dtype)
    r = residuals(Problem(case), R, t, np.asarray(state[1], dtype=dtype).reshape(-1, 3))
    return (r * r).sum()


def gradient(state, case, dtype=LD):
    """the cost's derivative in the free frames' (w, tau) and the free tracks' dX at a state"""
    R, t = split(state[0], dtype)
    r, J = residuals(Problem(case), R, t, np.asarray(state[1], dtype=dtype).reshape(-1, 3), jacobian=True)
    return 2 * (J.T @ r.reshape(-1))


def minimise(case, start=None, rounds=ROUNDS, work=np.float64):
    """Levenberg-Marquardt from `start` (default: the case's poses and points) -> ((poses, points) in np.longdouble, cost)"""
    pb = Problem(case)
    poses, xyz = state_of(case) if start is None else start
    R, t = split(poses)
    X = np.asarray(xyz, dtype=LD).reshape(-1, 3).copy()
    lam = 1e-3

    def down(*a):
        return [x.astype(work) for x in a]

    for _ in range(rounds):
        r, J = residuals(pb, *down(R, t, X), jacobian=True)
        now = (r * r).sum()
        A, g = J.T @ J, J.T @ r.reshape(-1)
        A[np.diag_indices_from(A)] *= 1 + lam
        d = np.linalg.solve(A, -g)
        trial = moved(pb, R, t, X, d)
        try:
            r = residuals(pb, *down(*trial))
            after = (r * r).sum()
        except Behind:
            after = np.inf
        if after < now:
            R, t, X = trial
            lam = max(lam / 10, 1e-12)
        else:
            lam *= 10
            if lam > 1e12:
                break
    state = (join(R, t), X)
    return state, cost(state, case)


def to_scale(state, like):
    """the state with every centre and point scaled about the root's centre, so that the centres lie at the root-mean-square
    distance from it that they have in `like`; the factor"""
    P = np.array(state[0], dtype=LD).reshape(-1, 3, 4)
    Q = np.asarray(like[0], dtype=LD).reshape(-1, 3, 4)
    root = P[0, :, 3].copy()
    k = np.sqrt(((Q[:, :, 3] - Q[0, :, 3]) ** 2).sum() / ((P[:, :, 3] - root) ** 2).sum())
    P[:, :, 3] = root + k * (P[:, :, 3] - root)
    return (P.reshape(-1, 12), root + k * (np.asarray(state[1], dtype=LD).reshape(-1, 3) - root)), k


def compare(state, case, ref_state, ref_cost, reported=None):
    """the figures of a state against the reference's minimum: the reported cost against the cost of that state and the cost
    against the minimum (both relative), max |gradient| over that at the case's start, and the poses' and the free points'
    largest difference, taken at the reference's scale"""
    c = cost(state, case)
    g0 = np.abs(gradient(state_of(case), case)).max()
    free = Problem(case).free_tracks
    (poses, xyz), k = to_scale(state, ref_state)
    return dict(reported=0.0 if reported is None else float(abs(LD(reported) - c) / c),
                cost=float(abs(c - ref_cost) / ref_cost),
                gradient=float(np.abs(gradient(state, case)).max() / g0),
                poses=float(np.abs(poses - ref_state[0]).max()),
                points=float(np.abs(xyz[free] - ref_state[1][free]).max()),
                scale=float(k - 1))


def rounded(state):
    """a state as any double-precision result holds it"""
    return np.asarray(state[0], dtype=np.float64), np.asarray(state[1], dtype=np.float64)


def spreads(case):
    """this reference against itself: its minimum from the planted truth against its minimum from the case's start, each state
    rounded to doubles; the cost as a round computes it, in doubles, against the long-double cost of the same state; the larger
    of the gradient ratios at its two minima"""
    a, ca = minimise(case)
    b, _ = minimise(case, start=(np.asarray(case.true_poses, dtype=LD), np.asarray(case.true_xyz, dtype=LD)))
    own = compare(rounded(a), case, a, ca, reported=cost(rounded(a), case, dtype=np.float64))
    out = compare(rounded(b), case, a, ca, reported=cost(rounded(b), case, dtype=np.float64))
    out["reported"], out["gradient"] = max(out["reported"], own["reported"]), max(out["gradient"], own["gradient"])
    return out


def check(figures, what=""):
    for name, limit in LIMITS.items():
        assert figures[name] <= limit, (what, name, figures[name], limit, figures)


# The spreads of the two scenes of the tests (ba_cases.noisy_scene(6, 60, seed=71) and (9, 120, seed=72), 40 rounds), as
# `python tests/ba_dense.py` prints them; SPREADS holds the larger of the two, rounded up:
#               seed 71    seed 72
#   reported    2.7e-14    1.6e-14   (a cost summed in doubles: each residual of some 0.2 px is the difference of two numbers
#   cost        2.7e-15    4.5e-15    of some 600 px and carries 1e-13 of itself)
#   gradient    1.7e-12    1.3e-12   (one of the two routes stalls: its last steps are turned down by costs that differ in the noise)
#   poses       1.1e-10    1.2e-11
#   points      1.1e-7     7.0e-9    (points 40 .. 60 m away, seen along a path of 2 m: their depth is the flattest direction)
SPREADS = dict(reported=2.7e-14, cost=4.6e-15, gradient=1.8e-12, poses=1.2e-10, points=1.2e-7)
# Two double-precision routes to one minimum differ by small factors of this, not by orders of magnitude: 100 times each.
LIMITS = {name: 100 * spread for name, spread in SPREADS.items()}
assert LIMITS["cost"] <= 1e-9 and LIMITS["gradient"] <= 1e-9  # beyond that the scenes or this reference are not fit for the tests


if __name__ == "__main__":
    import time
    import ba_cases as BC
    for seed, frames, points in ((71, 6, 60), (72, 9, 120)):
        t0 = time.time()
        print(seed, spreads(BC.noisy_scene(frames, points, seed=seed)), "%.1f s" % (time.time() - t0))
