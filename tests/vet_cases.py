"""Inputs for the vetting tests, from the synthetic geometry of tests/points_cases.py and tests/resect_cases.py (camera_path,
visible_points, pixel), no images.  cases() returns {name: Case}; reference(name) the restatement's result (tests/vet_ref.py),
computed once per process and shared by the CPU and the GPU suite.  The scenes are small, the restatement is plain Python; the
sizes that matter to a 16-lane group per track, sixteen tracks per workgroup, are in two families: track lengths around the
lane count, the chunk and many chunks (LENGTHS, one scene) and track counts around a wave's four and a workgroup's sixteen
tracks (COUNTS, a scene each)."""
import numpy as np

import points_cases as PC
import resect_cases as RC
import vet_ref as V

F, CU, CV = PC.F, PC.CU, PC.CV
LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257)
COUNTS = (1, 3, 4, 5, 15, 16, 17, 65)


class Case:
    def __init__(self, poses, tracks, xyz, use=None, pose_valid=None, params=None, f=F, cu=CU, cv=CV):
        """tracks: per track a list of (frame, u, v)"""
        self.poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(len(poses), 12)
        self.offsets = np.cumsum([0] + [len(t) for t in tracks]).astype(np.int32)
        obs = [o for t in tracks for o in t]
        self.obs_frames = np.array([o[0] for o in obs], dtype=np.int32)
        self.uv = np.array([(o[1], o[2]) for o in obs], dtype=np.float32).reshape(-1, 2)
        self.xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.use = None if use is None else np.ascontiguousarray(use, dtype=np.uint8)
        self.pose_valid = None if pose_valid is None else np.ascontiguousarray(pose_valid, dtype=np.uint8)
        self.params = dict(params or {})
        self.f, self.cu, self.cv = f, cu, cv

    def args(self):
        """positional and keyword arguments of host_vet / Matcher.vet / vet_ref.vet"""
        return ((self.poses, self.f, self.cu, self.cv, self.offsets, self.obs_frames, self.uv, self.xyz), dict(use=self.use, pose_valid=self.pose_valid, params=self.params))


def noisy_track(true, X, frames, rng, every=7):
    """one observation per entry of `frames`: up to 0.7 px off, every `every`-th 50 px off"""
    out = []
    for k, g in enumerate(frames):
        noise = (50.0, -30.0) if k % every == every - 1 else tuple(rng.uniform(-0.7, 0.7, 2))
        out.append((g,) + RC.pixel(true[g], X, noise))
    return out


def lengths_case():
    """track k has LENGTHS[k] observations, observation j in frame j mod 6: every lane and chunk edge of a 16-lane group"""
    rng = np.random.default_rng(31)
    true = PC.camera_path(6)
    pts = RC.visible_points(len(LENGTHS), rng)
    return Case(true, [noisy_track(true, X, [j % 6 for j in range(n)], rng) for n, X in zip(LENGTHS, pts)], pts)


def count_case(n):
    rng = np.random.default_rng(40 + n)
    true = PC.camera_path(5)
    pts = RC.visible_points(n, rng)
    tracks = [noisy_track(true, X, sorted(rng.choice(5, size=int(rng.integers(2, 6)), replace=False).tolist()), rng, every=4) for X in pts]
    return Case(true, tracks, pts)


ON_THE_GATE = 3  # codes_case: the track whose first observation sits on the gate exactly


def codes_case():
    """every code and every track status in one scene of five frames (frame 0 is the identity, frame 3 has no valid pose; f =
    512, cu = 600, cv = 180, min_observations = 3):
    tracks 0 .. 2: clean, five observations - status 0;
    track 3: the point (0.5, 0.25, 2) predicts (728, 244) in frame 0 exactly; its first pixel is (730, 244): ru = 2, rv = 0, so
             ru^2 + rv^2 equals max_residual^2 and the observation is gated (code 4); the others are clean - status 0;
    track 4: not in use - code 1, status 1;
    track 5: clean in frames 0, 1, 3: the frame-3 observation has code 2, two inliers remain = min_observations - 1 - status 2;
    track 6: a point behind the cameras - code 3, status 2;
    track 7: three inliers, all in frame 1 (a triple row), and one observation 50 px off in frame 2 - status 3;
    track 8: clean in frames 0, 1, 2, 4, a double row in frame 2 - status 0 with five inliers."""
    rng = np.random.default_rng(33)
    f, cu, cv = 512.0, 600.0, 180.0
    true = PC.camera_path(5)
    pts = list(RC.visible_points(9, rng))
    pts[3] = np.array([0.5, 0.25, 2.0])
    pts[6] = np.array([0.3, 0.2, -6.0])

    def px(g, X, noise=(0.0, 0.0)):
        u, v = PC.project(true[g], X, f, cu, cv)
        return (g, float(np.float32(u + noise[0])), float(np.float32(v + noise[1])))

    tracks = [[px(g, pts[t]) for g in (0, 1, 2, 4)] + [px(4, pts[t], (0.25, 0.5))] for t in range(3)]
    tracks.append([(0, 730.0, 244.0)] + [px(g, pts[3]) for g in (1, 2, 4)])
    tracks.append([px(g, pts[4]) for g in (0, 1, 2)])
    tracks.append([px(g, pts[5]) for g in (0, 1, 3)])
    tracks.append([(g, 500.0 + g, 100.0) for g in (0, 1, 2)])
    tracks.append([px(1, pts[7]), px(1, pts[7], (0.5, 0.0)), px(1, pts[7], (0.0, -0.5)), px(2, pts[7], (50.0, 0.0))])
    tracks.append([px(0, pts[8]), px(1, pts[8]), px(2, pts[8]), px(2, pts[8], (0.5, -0.25)), px(4, pts[8])])
    return Case(true, tracks, pts, use=[1, 1, 1, 1, 0, 1, 1, 1, 1], pose_valid=[1, 1, 1, 0, 1], params=dict(min_observations=3), f=f, cu=cu, cv=cv)


def nan_case():
    """NaN and +-inf pixels and a NaN point, as resect_cases.nan_case has them: the pixels are gated (code 4) by the comparison
    alone; the NaN point's depth is NaN, which fails rs_row's first test (code 3)"""
    c = RC.nan_case()
    return Case(c.true_poses, [[(int(c.obs_frames[i]), float(c.uv[i][0]), float(c.uv[i][1])) for i in range(c.offsets[t], c.offsets[t + 1])] for t in range(len(c.xyz))],
                c.xyz)


def masks_cases():
    """use and pose_valid masks (every fifth track unused with a NaN point); the same scene without a gate; min_depth = 9"""
    rng = np.random.default_rng(36)
    true = PC.camera_path(6)
    pts = RC.visible_points(40, rng)
    tracks = [noisy_track(true, X, [g for g in range(6) if rng.uniform() < 0.8], rng, every=5) for X in pts]
    use = np.ones(len(pts), np.uint8)
    use[::5] = 0
    xyz = pts.copy()
    xyz[::5] = np.nan
    return {"masks": Case(true, tracks, xyz, use=use, pose_valid=[1, 1, 0, 0, 1, 1]),
            "no_gate": Case(true, tracks, pts, params=dict(max_residual=0.0)),
            "min_depth_9": Case(true, tracks, pts, params=dict(min_depth=9.0))}


def planted_case():
    """-> (the planted Case, the clean Case).  The clean scene: true poses, true points, noise-free float32 pixels, every track in
    at least two frames.  Planted into it: in every third track one further observation 50 px off, at the front, in the middle
    or at the end; and after every fourth track a whole track of wrong observations (pixels of another point, 80 px off) with a
    point of its own.  Pruning the planted scene has to give the clean scene's arrays, with the planted tracks at length 0."""
    rng = np.random.default_rng(37)
    true = PC.camera_path(6)
    pts = RC.visible_points(48, rng)
    clean, planted, xyz, is_planted = [], [], [], []
    for t, X in enumerate(pts):
        frames = sorted(rng.choice(6, size=int(rng.integers(2, 7)), replace=False).tolist())
        tr = [(g,) + RC.pixel(true[g], X) for g in frames]
        bad = list(tr)
        if t % 3 == 0:
            g = int(rng.integers(0, 6))
            bad.insert((0, len(tr) // 2, len(tr))[(t // 3) % 3], (g,) + RC.pixel(true[g], X, (50.0, 0.0) if t % 2 else (-30.0, 40.0)))
        clean.append(tr)
        planted.append(bad)
        xyz.append(X)
        is_planted.append(False)
        if t % 4 == 3:
            clean.append([])
            planted.append([(g,) + RC.pixel(true[g], pts[(t + 5) % len(pts)], (80.0, -80.0)) for g in frames])
            xyz.append(X)
            is_planted.append(True)
    c = Case(true, planted, xyz)
    c.is_planted = np.array(is_planted)
    return c, Case(true, clean, xyz)


_cases = None
_refs = {}


def cases():
    global _cases
    if _cases is not None:
        return _cases
    c = {"lengths": lengths_case(), "codes": codes_case(), "nan": nan_case(), "planted": planted_case()[0]}
    for n in COUNTS:
        c["counts_%d" % n] = count_case(n)
    c.update(masks_cases())
    c["no_tracks"] = Case(PC.camera_path(3), [], np.zeros((0, 3)))
    c["no_frames"] = Case(np.zeros((0, 12)), [], np.zeros((0, 3)))
    _cases = c
    return c


def reference(name):
    if name not in _refs:
        a, kw = cases()[name].args()
        _refs[name] = V.vet(*a, **kw)
    return _refs[name]
