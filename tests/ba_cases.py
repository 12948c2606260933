"""Inputs for the joint-adjustment tests, from the synthetic geometry of tests/points_cases.py and tests/resect_cases.py (camera
path, points, float32 pixels), no images.  cases() returns {name: Case} - resect_cases.Case with vsm_adjust_params fields as
params -; reference(name) the restatement's result (tests/ba_ref.py), computed once per process and shared by the CPU and the
GPU suite.  The scenes are the smallest at which the kernels can go wrong: frame counts 1, 2, 3, 9 (a workgroup per frame);
rows per frame 0, 5, 6, 255 .. 257, 513 (either side of min_observations, of the 256 lanes and of their second round); track
lengths 1, 2, 15 .. 17, 33 and track counts 1, 15 .. 17, 65, 257 (a lane per track, 256 lanes per workgroup); every status of
a frame and of a track in one call; and one case per exit of the solve and of the call.  Then the wide ones, for what is
dealt out over 256 lanes by the frame: frame counts 42 | 43 and 85 | 86 (6 F entries of the solve's vectors on either side of
the 256 partial sums of a scalar product, and of their second wrap), 256 | 257 and 513 (a lane per frame: a second and a third
trip of one workgroup's loops, a second and a third block of the flat grids), with fewer tracks than frames, and with held
frames all along.  Rounds and iterations are kept few: the restatement walks 256 partial sums and their tree in plain Python
for every sum.  long_case: two scenes run to the minimum, for the comparison with the dense reference of tests/ba_dense.py."""
import numpy as np

import points_cases as PC
import resect_cases as RC
import ba_ref as B
import ba_dense as D

QUICK = dict(min_observations=6, max_rounds=3, cg_iters=8)
ROW_COUNTS = (0, 5, 6, 255, 256, 257, 513)
TRACK_LENGTHS = (1, 2, 15, 16, 17, 33)
TRACK_COUNTS = (1, 15, 16, 17, 65, 257)


def root_fixed(n):
    r = np.ones(n, np.uint8)
    if n:
        r[0] = 0
    return r


def noisy_scene(n_frames, n_points, seed, noise=0.3, seen=0.8, angle=1e-2, shift=0.03, point_shift=0.05, params=None, fix_root=True, path=None):
    """a forward-moving camera, `noise` px of pixel noise, poses and points moved off the truth; the root frame (pinned) keeps
    its true pose.  .true_poses / .true_xyz: the planted state."""
    rng = np.random.default_rng(seed)
    true = PC.camera_path(n_frames, **(path or {}))
    pts = RC.visible_points(n_points, rng)
    tracks = [[(g,) + RC.pixel(true[g], X, (noise * rng.uniform(-1, 1), noise * rng.uniform(-1, 1))) for g in range(n_frames) if rng.uniform() < seen] for X in pts]
    poses = RC.perturb(true, rng, angle, shift)
    if fix_root and n_frames:
        poses[0] = true[0]
    c = RC.Case(poses, tracks, pts + rng.uniform(-1, 1, pts.shape) * point_shift, refine=root_fixed(n_frames) if fix_root else None,
                params=dict(QUICK, **(params or {})), true_poses=true)
    c.true_xyz = np.ascontiguousarray(pts, dtype=np.float64)
    return c


def rows_family():
    """frame g has exactly ROW_COUNTS[g] rows: point i is seen by the frames with more than i rows"""
    rng = np.random.default_rng(31)
    true = PC.camera_path(len(ROW_COUNTS), step=(0.06, 0.0, 0.01), yaw=0.002)
    pts = RC.visible_points(max(ROW_COUNTS), rng)
    tracks = [[(g,) + RC.pixel(true[g], X, (0.2 * rng.uniform(-1, 1), 0.2 * rng.uniform(-1, 1))) for g, n in enumerate(ROW_COUNTS) if i < n] for i, X in enumerate(pts)]
    return RC.Case(RC.perturb(true, rng), tracks, pts + rng.uniform(-1, 1, pts.shape) * 0.02, params=dict(QUICK, max_rounds=2, cg_iters=5), true_poses=true)


def lengths_family():
    """eight tracks of every length in TRACK_LENGTHS over 33 frames: a track of length n is seen by the frames 0 .. n - 1"""
    rng = np.random.default_rng(32)
    n_frames = max(TRACK_LENGTHS)
    true = PC.camera_path(n_frames, step=(0.05, 0.0, 0.02), yaw=0.002)
    pts = RC.visible_points(8 * len(TRACK_LENGTHS), rng)
    tracks = [[(g,) + RC.pixel(true[g], X, (0.2 * rng.uniform(-1, 1), 0.2 * rng.uniform(-1, 1))) for g in range(TRACK_LENGTHS[i % len(TRACK_LENGTHS)])] for i, X in enumerate(pts)]
    return RC.Case(RC.perturb(true, rng, 3e-3, 0.01), tracks, pts + rng.uniform(-1, 1, pts.shape) * 0.02, refine=root_fixed(n_frames),
                   params=dict(QUICK, max_rounds=2, cg_iters=6), true_poses=true)


def grid_case():
    """every status of a frame and of a track in one call.  The frames are resect_cases.statuses_case's: [0] no valid pose (its
    pose NaN), [1] not asked for, [2] five rows, [3] twelve rows, eight of them behind the camera: held, [4] twelve points on
    the optical axis, no pivot: held, [5], [6] free.  Tracks: the first 40 free but [7] (not in use, its point NaN); the eight
    seen by camera 3 alone, from behind, and the twelve seen by camera 4 alone, once each: too few active rows; the last one
    at a distance of 1e200: its Jp is f * 1e200 / inf = 0, its V has no pivot, and its rows put NaNs into the sums of the
    frames 5 and 6 (Jc has z * z / zz = inf / inf), so the solve of every round ends on the p.q test with x = 0: the points alone move."""
    s = RC.statuses_case()
    c5, c6 = s.true_poses[5].reshape(3, 4), s.true_poses[6].reshape(3, 4)
    far = c5[:, 3] + c5[:, :3] @ np.array([0.0, 0.0, 1e200])
    tracks = [[(int(g), float(u), float(v)) for g, (u, v) in zip(s.obs_frames[a:b], s.uv[a:b])] for a, b in zip(s.offsets[:-1], s.offsets[1:])]
    tracks.append([(5, RC.CU + 2.0, RC.CV + 1.0), (6, RC.CU + 2.5, RC.CV + 1.0)])
    xyz = np.vstack([s.xyz, far[None, :]])
    xyz[7] = np.nan
    use = np.ones(len(xyz), np.uint8)
    use[7] = 0
    poses = s.poses.copy()
    poses[0] = np.nan
    del c6
    return RC.Case(poses, tracks, xyz, use=use, refine=s.refine, pose_valid=s.pose_valid, params=dict(QUICK, max_rounds=3))


def held_frame_only_case():
    """frame 1 is not asked for; five tracks are seen by it alone, twice each at the same pixel - parallel rays, a V of rank 2
    that only the damping gives its third pivot -, so they are free tracks whose every row lies in a held frame"""
    c = noisy_scene(4, 40, seed=33)
    rng = np.random.default_rng(34)
    extra = RC.visible_points(5, rng)
    tracks = [[(int(g), float(u), float(v)) for g, (u, v) in zip(c.obs_frames[a:b], c.uv[a:b])] for a, b in zip(c.offsets[:-1], c.offsets[1:])]
    for X in extra:
        px = RC.pixel(c.true_poses[1], X)
        tracks.append([(1,) + px, (1,) + px])
    refine = np.array([0, 0, 1, 1], np.uint8)
    poses = c.poses.copy()
    poses[1] = c.true_poses[1]
    return RC.Case(poses, tracks, np.vstack([c.xyz, extra + 0.03]), refine=refine, params=c.params, true_poses=c.true_poses)


def gate_case():
    """max_residual = 5 with exact intrinsics (f = 512, cu = 640, cv = 192) and the pinned root at the identity: the point (0, 0,
    5) projects to (cu, cv) exactly, so the pixel (cu + 3, cv + 4) has ru^2 + rv^2 = 25 = the limit, exactly: inactive in
    every round; its neighbour with (cu + 3, cv + 3.5) is active.  Every sixth of the other pixels is 3 px off (inside), every
    seventh 40 px (outside)."""
    f, cu, cv = 512.0, 640.0, 192.0
    rng = np.random.default_rng(35)
    true = PC.camera_path(4)
    pts = RC.visible_points(60, rng)
    tracks = []
    for i, X in enumerate(pts):
        noise = (3.0, 0.0) if i % 6 == 0 else (0.0, 40.0) if i % 7 == 0 else (0.0, 0.0)
        tracks.append([(g,) + tuple(float(np.float32(a + b)) for a, b in zip(PC.project(true[g], X, f, cu, cv), noise)) for g in range(4)])
    pts = list(pts) + [np.array([0.0, 0.0, 5.0]), np.array([0.0, 0.0, 5.0])]
    tracks.append([(0, cu + 3.0, cv + 4.0), (0, cu + 3.0, cv + 4.0)])
    tracks.append([(0, cu + 3.0, cv + 3.5), (0, cu + 3.0, cv + 3.5)])
    poses = RC.perturb(true, rng, 2e-3, 0.01)
    poses[0] = true[0]
    # (min_track_observations beyond every track: the points stay where they are, and so does the row on the gate)
    return RC.Case(poses, tracks, pts, refine=root_fixed(4), params=dict(QUICK, max_residual=5.0, min_track_observations=100), true_poses=true, f=f, cu=cu, cv=cv)


def nan_case():
    """resect_cases.nan_case (NaN and infinite pixels, a NaN point) with two more frames that see the first ten tracks: [3] a NaN
    pose behind pose_valid = 0, [4] a valid pose with an infinite entry - each of its rows is behind the camera or not a number"""
    c = RC.nan_case()
    tracks = [[(int(g), float(u), float(v)) for g, (u, v) in zip(c.obs_frames[a:b], c.uv[a:b])] for a, b in zip(c.offsets[:-1], c.offsets[1:])]
    for t in tracks[:10]:
        t.extend([(3,) + t[-1][1:], (4,) + t[-1][1:]])
    poses = np.vstack([c.poses, c.poses[2:3], c.poses[2:3]])
    poses[3] = np.nan
    poses[4, 3] = np.inf
    return RC.Case(poses, tracks, c.xyz, refine=root_fixed(5), pose_valid=[1, 1, 1, 0, 1], params=dict(QUICK))


SLOW_PATH = dict(step=(0.01, 0.0, 0.002), yaw=0.0005)  # every point stays in front of every camera over hundreds of frames
DENSE_FRAMES = (42, 43, 85, 86, 256, 257)              # 6 F = 252, 258 | 510, 516 | 1536, 1542: either side of the 256 partials' first and second wrap, and of a block of lanes
DENSE_POINTS = 12
BANDS = {"band_257": (257, 520, 8), "band_513": (513, 700, 10), "band_257_held": (257, 520, 8)}  # name: frames, tracks, track length
BAND_PARAMS = dict(QUICK, max_rounds=2, cg_iters=4, cg_tol=1e-9)


def dense_wide(n_frames):
    """DENSE_POINTS points, each seen by every frame of a slow path: fewer tracks than frames, so the grids over both are sized
    by the frames; all frames but the pinned root are free"""
    return noisy_scene(n_frames, DENSE_POINTS, seed=80 + n_frames, seen=1.0, angle=2e-3, shift=0.01, point_shift=0.02, params=dict(max_rounds=2, cg_iters=3), path=SLOW_PATH)


def band_wide(n_frames, n_points, length, seed, held=False):
    """point i is seen by `length` consecutive frames from (i * (n_frames - length)) // (n_points - 1) on: a band along the slow
    path, a few rows in the frames at its two ends.  held: every fifth frame is not asked for and the frames 100 and
    n_frames - 1 have no valid pose, so held entries are passed over all along the scalar products and the last frame of the
    last block of lanes is one of them."""
    rng = np.random.default_rng(seed)
    true = PC.camera_path(n_frames, **SLOW_PATH)
    pts = RC.visible_points(n_points, rng)
    tracks = []
    for i, X in enumerate(pts):
        first = (i * (n_frames - length)) // (n_points - 1)
        tracks.append([(g,) + RC.pixel(true[g], X, (0.3 * rng.uniform(-1, 1), 0.3 * rng.uniform(-1, 1))) for g in range(first, first + length)])
    poses = RC.perturb(true, rng, 2e-3, 0.01)
    poses[0] = true[0]
    refine, valid = root_fixed(n_frames), None
    if held:
        refine[::5] = 0
        valid = np.ones(n_frames, np.uint8)
        valid[[100, n_frames - 1]] = 0
    c = RC.Case(poses, tracks, pts + rng.uniform(-1, 1, pts.shape) * 0.02, refine=refine, pose_valid=valid, params=dict(BAND_PARAMS), true_poses=true)
    c.true_xyz = np.ascontiguousarray(pts, dtype=np.float64)
    return c


def with_params(c, **params):
    d = RC.Case(c.poses, [], c.xyz, use=c.use, refine=c.refine, pose_valid=c.pose_valid, params=dict(c.params, **params), true_poses=c.true_poses, f=c.f, cu=c.cu, cv=c.cv)
    d.offsets, d.obs_frames, d.uv = c.offsets, c.obs_frames, c.uv
    return d


_cases = None
_refs = {}


def cases():
    global _cases
    if _cases is not None:
        return _cases
    c = {}
    c["rows_family"] = rows_family()
    c["lengths_family"] = lengths_family()
    c["grid"] = grid_case()
    c["held_frame_only"] = held_frame_only_case()
    c["gate"] = gate_case()
    c["nan"] = nan_case()
    c["behind"] = with_params(RC.behind_case(), **QUICK)
    c["masks"] = with_params(RC.masks_case(), **QUICK)
    for n in (1, 2, 3, 9):  # the grid's edge: every workgroup is one frame
        c["frames_%d" % n] = noisy_scene(n, 24, seed=40 + n, seen=1.0)
    for n in TRACK_COUNTS:  # (one track: every frame has one row, nothing but the point moves)
        c["tracks_%d" % n] = noisy_scene(3, n, seed=50 + n, seen=1.0, params=dict(max_rounds=2, cg_iters=5))
    small = noisy_scene(5, 40, seed=60)
    c["points_only"] = with_params(small, max_rounds=3)
    c["points_only"].refine = np.zeros(5, np.uint8)
    c["poses_only"] = with_params(small, min_track_observations=1000)
    c["no_tracks"] = RC.Case(PC.camera_path(3), [], np.zeros((0, 3)), params=dict(QUICK))
    c["no_frames"] = RC.Case(np.zeros((0, 12)), [], np.zeros((0, 3)), params=dict(QUICK))
    # the exits (found with the host view, pinned by test_ba_cpu.py's census)
    c["first_step_rejected"] = noisy_scene(4, 40, seed=63, angle=0.25, shift=0.5, point_shift=0.5, params=dict(max_rounds=4))
    c["hits_cg_iters"] = with_params(small, cg_iters=2, cg_tol=1e-8)
    c["converges"] = with_params(small, max_rounds=8, cg_iters=30, ftol=1e-3)
    c["lambda_max"] = with_params(c["no_tracks"], lambda_max=1e-1, max_rounds=5)  # (no rows: the cost is 0 and no step can lower it)
    # the wide ones: more than 256 entries of the frames' vectors, more than 256 frames, more frames than tracks
    for n in DENSE_FRAMES:
        c["dense_%d" % n] = dense_wide(n)
    for k, (name, (n_frames, n_points, length)) in enumerate(sorted(BANDS.items())):
        c[name] = band_wide(n_frames, n_points, length, seed=90 + k, held=name.endswith("_held"))
    _cases = c
    return c


def reference(name):
    if name not in _refs:
        a, kw = cases()[name].args()
        _refs[name] = B.adjust(*a, **kw)
    return _refs[name]


# ---- the long run: to the minimum, against the dense reference (tests/ba_dense.py) ---------------------------------------------------

LONG_SCENES = {71: (6, 60), 72: (9, 120)}  # seed: frames, points - the scenes of test_ba_cpu.py's test_minimiser
LONG = dict(min_observations=10, max_rounds=40, cg_iters=200, cg_tol=1e-12, ftol=1e-14)
_long = {}


def long_case(seed):
    """-> (the case, the dense reference's minimum (poses, points) and its cost), computed once per process"""
    if seed not in _long:
        c = noisy_scene(*LONG_SCENES[seed], seed=seed, params=LONG)
        _long[seed] = (c,) + D.minimise(c)
    return _long[seed]


def against_the_dense_reference(got, seed, what):
    """the four comparisons of a result of long_case(seed) with ba_dense, within ba_dense.LIMITS"""
    c, state, cost = long_case(seed)
    assert got.frame_status.tolist() == [2] + [0] * (len(c.poses) - 1) and (got.track_status == 0).all()  # what ba_dense takes for free
    assert got.history["active"][-1] == len(c.uv)
    figures = D.compare((got.poses, got.xyz), c, state, cost, reported=got.cost)
    print(what, seed, "rounds", len(got.history), "against the dense reference:", figures, "limits:", D.LIMITS)
    D.check(figures, (what, seed))
