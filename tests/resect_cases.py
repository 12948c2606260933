"""Inputs for the pose-refinement tests, all from the synthetic geometry of tests/points_cases.py (camera_path, scene_points,
project to float32 pixels), no images: a camera path, 3-D points, the pixels of the points in the frames that see them, and the
poses the call is given - the true ones moved by about 1e-2 rad and a few centimetres.  cases() returns {name: Case};
reference(name) the restatement's result (tests/resect_ref.py), computed once per process and shared by the CPU and the GPU
suite.  The scenes are small (the restatement walks 256 partial sums and their tree in plain Python for every evaluation): the
row counts that matter are in one case, rows_family, whose frames have 0, 1, 9, 10, 63 .. 65, 255 .. 257 and 511 .. 513 rows."""
import math

import numpy as np

import points_cases as PC
import resect_ref as R

F, CU, CV = PC.F, PC.CU, PC.CV
ROW_COUNTS = (0, 1, 9, 10, 63, 64, 65, 255, 256, 257, 511, 512, 513)


class Case:
    def __init__(self, poses, tracks, xyz, use=None, refine=None, pose_valid=None, params=None, true_poses=None, f=F, cu=CU, cv=CV):
        """tracks: per track a list of (frame, u, v)"""
        self.poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(len(poses), 12)
        self.offsets = np.cumsum([0] + [len(t) for t in tracks]).astype(np.int32)
        obs = [o for t in tracks for o in t]
        self.obs_frames = np.array([o[0] for o in obs], dtype=np.int32)
        self.uv = np.array([(o[1], o[2]) for o in obs], dtype=np.float32).reshape(-1, 2)
        self.xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.use = None if use is None else np.ascontiguousarray(use, dtype=np.uint8)
        self.refine = None if refine is None else np.ascontiguousarray(refine, dtype=np.uint8)
        self.pose_valid = None if pose_valid is None else np.ascontiguousarray(pose_valid, dtype=np.uint8)
        self.params = dict(params or {})
        self.true_poses = None if true_poses is None else np.ascontiguousarray(true_poses, dtype=np.float64).reshape(len(poses), 12)
        self.f, self.cu, self.cv = f, cu, cv

    def args(self):
        """positional and keyword arguments of host_resect / Matcher.resect / resect_ref.resect"""
        return ((self.poses, self.f, self.cu, self.cv, self.offsets, self.obs_frames, self.uv, self.xyz),
                dict(use=self.use, refine=self.refine, pose_valid=self.pose_valid, params=self.params))


def rot_z(a):
    return np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])


def perturb(poses, rng, angle=1e-2, shift=0.03):
    """every pose turned by up to `angle` rad about each axis and moved by up to `shift` m along each"""
    out = []
    for p in np.asarray(poses).reshape(-1, 3, 4):
        a = rng.uniform(-1, 1, 3) * angle
        Rn = p[:, :3] @ PC.rot_x(a[0]) @ PC.rot_y(a[1]) @ rot_z(a[2])
        out.append(np.hstack([Rn, (p[:, 3] + rng.uniform(-1, 1, 3) * shift)[:, None]]).reshape(12))
    return np.array(out)


def visible_points(n, rng):
    """n points of PC.scene_points in front of every camera of a short path (its classes 6 and 8 are behind / too near)"""
    pts = PC.scene_points(3 * n, rng)
    keep = [i for i in range(len(pts)) if i % 9 not in (6, 8)]
    return pts[keep][:n]


def pixel(pose, X, noise=(0.0, 0.0)):
    u, v = PC.project(pose, X)
    return float(np.float32(u + noise[0])), float(np.float32(v + noise[1]))


def scene(n_frames, n_points, seed, seen=0.8, angle=1e-2, shift=0.03, **kw):
    """every point is seen by a frame with probability `seen`; noise-free float32 pixels; perturbed poses"""
    rng = np.random.default_rng(seed)
    true = PC.camera_path(n_frames)
    pts = visible_points(n_points, rng)
    tracks = [[(g,) + pixel(true[g], X) for g in range(n_frames) if rng.uniform() < seen] for X in pts]
    return Case(perturb(true, rng, angle, shift), tracks, pts, true_poses=true, **kw)


def rows_family():
    """frame g has exactly ROW_COUNTS[g] rows: point i is seen by the frames with more than i rows"""
    rng = np.random.default_rng(11)
    true = PC.camera_path(len(ROW_COUNTS), step=(0.06, 0.0, 0.01), yaw=0.002)
    pts = visible_points(max(ROW_COUNTS), rng)
    tracks = [[(g,) + pixel(true[g], X) for g, n in enumerate(ROW_COUNTS) if i < n] for i, X in enumerate(pts)]
    return Case(perturb(true, rng), tracks, pts, true_poses=true)


def statuses_case():
    """seven frames, one per status, in the order 1, 2, 3, 4, 5, 0, 6 (max_updates = 1, eps = 1e-3): [0] no valid pose; [1] not
    asked for; [2] five rows; [3] twelve rows, eight of them of points behind the camera; [4] twelve points on the optical axis
    of a camera without rotation: columns 2 and 5 of J are zero, no pivot; [5] moved by 1e-5: the first delta is within eps; [6]
    moved by 1e-2: it is not"""
    rng = np.random.default_rng(12)
    true = PC.camera_path(7, step=(0.06, 0.0, 0.01), yaw=0.0)
    pts = list(visible_points(40, rng))
    tracks = [[(g,) + pixel(true[g], X) for g in (0, 1, 5, 6)] for X in pts]
    for i in range(5):
        tracks[i].append((2,) + pixel(true[2], pts[i]))
    for i in range(4):
        tracks[i].append((3,) + pixel(true[3], pts[i]))
    c3 = true[3].reshape(3, 4)[:, 3]
    for k in range(8):  # behind camera 3, seen by it alone
        pts.append(c3 + np.array([0.1 * k - 0.4, 0.2, -3.0 - k]))
        tracks.append([(3, 600.0 + k, 200.0)])
    c4 = true[4].reshape(3, 4)[:, 3]
    for k in range(12):  # on camera 4's optical axis, seen by it alone
        pts.append(c4 + np.array([0.0, 0.0, 4.0 + k]))
        tracks.append([(4, CU + 1.0, CV - 1.0)])
    poses = true.copy()
    poses[5] = perturb(true[5:6], rng, 1e-5, 1e-5)[0]
    poses[6] = perturb(true[6:7], rng, 1e-2, 0.03)[0]
    return Case(poses, tracks, pts, refine=[1, 0, 1, 1, 1, 1, 1], pose_valid=[0, 1, 1, 1, 1, 1, 1], params=dict(max_updates=1, eps=1e-3), true_poses=true)


def gate_case():
    """max_residual = 8 px on poses that start some 6 px off: every sixth pixel is 4 px off (inside the gate at the optimum, on
    either side of it at the start: the used set changes between updates), every seventh 50 px (outside throughout)"""
    rng = np.random.default_rng(13)
    true = PC.camera_path(4)
    pts = visible_points(80, rng)
    tracks = []
    for i, X in enumerate(pts):
        noise = (4.0, 0.0) if i % 6 == 0 else (0.0, 50.0) if i % 7 == 0 else (0.0, 0.0)
        tracks.append([(g,) + pixel(true[g], X, noise) for g in range(4)])
    return Case(perturb(true, rng), tracks, pts, params=dict(max_residual=8.0), true_poses=true)


def behind_case():
    """a third of the points lie behind the cameras: rows that are never used"""
    rng = np.random.default_rng(14)
    true = PC.camera_path(3)
    front = iter(visible_points(60, rng))
    pts = [np.array([rng.uniform(-2, 2), rng.uniform(-1, 1), -rng.uniform(2, 9)]) if k % 3 == 2 else next(front) for k in range(90)]
    tracks = [[(g,) + pixel(true[g], X) for g in range(3)] for X in pts]
    return Case(perturb(true, rng), tracks, pts, true_poses=true)


def nan_case():
    """NaN and infinite pixels, one NaN point: rows that are never used, whichever test they fail"""
    c = scene(3, 50, seed=15, seen=1.0)
    uv = c.uv.copy()
    uv[5, 0] = np.nan
    uv[17, 1] = np.nan
    uv[40] = (np.nan, np.nan)
    uv[77, 0] = np.inf
    uv[90, 1] = -np.inf
    c.uv = uv
    xyz = c.xyz.copy()
    xyz[7, 2] = np.nan
    c.xyz = xyz
    return c


def masks_case():
    """refine and pose_valid masks over six frames; every fifth track unused, its point NaN (a track the triangulation dropped)"""
    c = scene(6, 60, seed=16)
    use = np.ones(len(c.xyz), np.uint8)
    use[::5] = 0
    xyz = c.xyz.copy()
    xyz[::5] = np.nan
    c.xyz, c.use = xyz, use
    c.refine = np.array([0, 1, 1, 0, 1, 1], np.uint8)
    c.pose_valid = np.array([1, 1, 0, 0, 1, 1], np.uint8)
    return c


def double_row_case():
    """tracks with two rows in one frame (what a flagged track looks like), the second pixel a little off"""
    rng = np.random.default_rng(17)
    true = PC.camera_path(3)
    pts = visible_points(40, rng)
    tracks = []
    for i, X in enumerate(pts):
        t = [(g,) + pixel(true[g], X) for g in range(3)]
        if i % 8 == 0:
            t.insert(2, (1,) + pixel(true[1], X, (0.5, -0.25)))
        tracks.append(t)
    return Case(perturb(true, rng), tracks, pts, true_poses=true)


def pool_chunks_case():
    """4 frames, 520 points, every point seen by every frame: 2080 observations, which the device paths group in 4 chunks of 130
    tracks on the handle's pool (rs_group_chunks, csrc/vsm_resect.h) where the host views take one; every fifth track unused;
    the root frame fixed.  Not one of cases(): the restatement walks every partial sum in Python and takes too long at this
    size, so the device is compared with the host view alone (test_resect_gpu.py, test_ba_gpu.py)."""
    c = scene(4, 520, seed=25, seen=1.0, refine=[0, 1, 1, 1])
    c.use = np.ones(520, np.uint8)
    c.use[::5] = 0
    assert len(c.obs_frames) == 2080 and len(c.offsets) == 521
    return c


_cases = None
_refs = {}


def cases():
    global _cases
    if _cases is not None:
        return _cases
    c = {}
    c["rows_family"] = rows_family()
    c["statuses"] = statuses_case()
    c["gate"] = gate_case()
    c["behind"] = behind_case()
    c["nan"] = nan_case()
    c["masks"] = masks_case()
    c["double_row"] = double_row_case()
    c["minimiser"] = scene(8, 60, seed=18)
    for n in (1, 2, 9):  # the grid's edge: every workgroup is one frame
        c["frames_%d" % n] = scene(n, 30, seed=20 + n, seen=1.0)
    c["no_tracks"] = Case(PC.camera_path(3), [], np.zeros((0, 3)))
    c["no_frames"] = Case(np.zeros((0, 12)), [], np.zeros((0, 3)))
    c["at_the_truth"] = scene(3, 40, seed=19, angle=0.0, shift=0.0)
    c["min_depth_9"] = scene(3, 60, seed=24, params=dict(min_depth=9.0, min_observations=6))
    _cases = c
    return c


def reference(name):
    if name not in _refs:
        a, kw = cases()[name].args()
        _refs[name] = R.resect(*a, **kw)
    return _refs[name]
