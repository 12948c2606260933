"""Inputs for the track-triangulation tests, all from synthetic geometry, no images: a camera path, 3-D points projected to
float32 pixels, match lists whose feature index is the point id, tracks from vsm_host_tracks, and a few tracks given as raw
arrays where a status needs inputs that no scene produces.  cases() returns {name: Case}; reference(name) the restatement's
result (tests/points_ref.py), computed once per process and shared by the CPU and the GPU suite.

Cameras look along +z with y down (the reference's road transform expects that): a point 1.6 m below the camera is on the road.
The scenes have 6 to 12 frames and at most 288 points; the family of track lengths alone needs 66 frames (a consistent track
has one observation per frame, and the lengths go up to 65)."""
import math

import numpy as np

import points_ref as R
from conftest import pkg

F, CU, CV = 645.24, 635.96, 194.13


class Case:
    def __init__(self, poses, offsets, obs_frames, uv, flags=None, pose_valid=None, params=None, f=F, cu=CU, cv=CV, lists=None, pairs=None, ids=None):
        self.poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(len(poses), 12)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        self.obs_frames = np.ascontiguousarray(obs_frames, dtype=np.int32)
        self.uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
        self.flags = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        self.pose_valid = None if pose_valid is None else np.ascontiguousarray(pose_valid, dtype=np.uint8)
        self.params = dict(params or {})
        self.f, self.cu, self.cv = f, cu, cv
        self.lists, self.pairs, self.ids = lists, pairs, ids  # (scenes only: the match lists, their pairs, the point id per track)

    def args(self):
        """positional and keyword arguments of host_triangulate / Matcher.triangulate / points_ref.triangulate"""
        return (self.poses, self.f, self.cu, self.cv, self.offsets, self.obs_frames, self.uv), dict(flags=self.flags, pose_valid=self.pose_valid, params=self.params)

    def with_(self, **kw):
        c = Case(self.poses, self.offsets, self.obs_frames, self.uv, self.flags, self.pose_valid, self.params, self.f, self.cu, self.cv, self.lists, self.pairs, self.ids)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def first_tracks(self, n):
        """the first n tracks as a case of their own"""
        off = self.offsets[:n + 1]
        last = int(off[-1]) if len(off) else 0
        return Case(self.poses, off, self.obs_frames[:last], self.uv[:last], None if self.flags is None else self.flags[:n], self.pose_valid, self.params, self.f,
                    self.cu, self.cv)


# ---- geometry --------------------------------------------------------------------------------------------------------------------

def rot_y(a):
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])


def rot_x(a):
    return np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])


def camera_path(n, step=(0.40, -0.01, 0.30), yaw=0.012, world=None):
    """n poses [R | c], camera to world; world = (Rw, tw) moves the whole scene into another world frame"""
    poses = []
    for k in range(n):
        Rk, c = rot_y(yaw * k), np.array(step) * k
        if world is not None:
            Rk, c = world[0] @ Rk, world[0] @ c + world[1]
        poses.append(np.hstack([Rk, c[:, None]]).reshape(12))
    return np.array(poses)


def project(pose, X, f=F, cu=CU, cv=CV):
    P = pose.reshape(3, 4)
    xc = P[:, :3].T @ (np.asarray(X, dtype=np.float64) - P[:, 3])
    return f * xc[0] / xc[2] + cu, f * xc[1] / xc[2] + cv


def scene_points(n, rng):
    """n points in the frame of camera 0, nine classes by id % 9 (see the module text of test_points_cpu.py)"""
    pts = []
    for i in range(n):
        k = i % 9
        z = rng.uniform(5, 20)
        x = rng.uniform(-0.3, 0.3) * z
        y = {0: 1.6 - 0.08 * z + 0.85, 1: 1.6 - 0.08 * z + 0.15, 2: -1.5, 3: -3.0, 7: 3.5}.get(k, 1.0)
        if k == 4:    # far
            z = rng.uniform(40, 60)
        elif k == 5:  # far enough for a small angle over two frames
            z, x = rng.uniform(25, 28), rng.uniform(-1, 1)
        elif k == 6:  # behind the cameras
            z = -rng.uniform(6, 12)
        elif k == 8:  # in front of camera 0, but not by more than a metre
            z, x, y = rng.uniform(0.5, 0.95), rng.uniform(-0.2, 0.2), 0.1
        pts.append((x, y, z))
    return np.array(pts)


def build_scene(n_frames, n_points, seed, noise=0.0, world=None, extra_matches=(), gaps=True):
    """poses, and tracks through vsm_host_tracks from match lists over the pairs of frames in which a point is seen one after the
    other.  extra_matches: (frame a, point p, frame b, point q) mismatches that merge two points' tracks."""
    vm = pkg("visomatch")
    rng = np.random.default_rng(seed)
    poses = camera_path(n_frames, world=world)
    pts = scene_points(n_points, rng)
    if world is not None:
        pts = pts @ world[0].T + world[1]
    seen, pix = [], {}
    for i in range(n_points):
        if i % 9 == 5:
            a = int(rng.integers(0, n_frames - 1))
            frames = [a, a + 1]
        else:
            length = int(rng.integers(2, n_frames + 1))
            a = int(rng.integers(0, n_frames - length + 1))
            frames = list(range(a, a + length))
            if gaps and length >= 4 and i % 4 == 0:
                del frames[1 + int(rng.integers(0, length - 2))]  # a gap: the pair skips a frame
        seen.append(frames)
        for k in frames:
            u, v = project(poses[k], pts[i])
            pix[i, k] = (np.float32(u + noise * rng.uniform(-1, 1)), np.float32(v + noise * rng.uniform(-1, 1)))
    by_pair = {}
    for i, frames in enumerate(seen):
        for a, b in zip(frames[:-1], frames[1:]):
            by_pair.setdefault((a, b), []).append((i, i))
    for a, p, b, q in extra_matches:
        by_pair.setdefault((a, b), []).append((p, q))
        for k, i in ((a, p), (b, q)):
            if (i, k) not in pix:
                pix[i, k] = tuple(np.float32(x) for x in project(poses[k], pts[i]))
    pairs = sorted(by_pair)
    lists = []
    for a, b in pairs:
        m = np.zeros(len(by_pair[a, b]), dtype=vm.P_MATCH)
        for j, (p, q) in enumerate(by_pair[a, b]):
            m[j]["i1p"], m[j]["i1c"], m[j]["i2p"], m[j]["i2c"] = p, q, -1, -1
            m[j]["u1p"], m[j]["v1p"] = pix[p, a]
            m[j]["u1c"], m[j]["v1c"] = pix[q, b]
        lists.append(m)
    tr = vm.host_tracks(n_frames, pairs, lists, 0, 2)
    uv = gather(tr.obs, lists, 0)
    ids = tr.obs[tr.offsets[:-1], 1] if len(tr) else np.zeros(0, np.int32)
    return Case(poses, tr.offsets, tr.obs[:, 0], uv, tr.flags, lists=lists, pairs=pairs, ids=ids)


def gather(obs, lists, side):
    """the pixel of every observation {frame, feature, pair, 2 * match + end}, read from the match it names"""
    uv = np.zeros((len(obs), 2), np.float32)
    s = "2" if side else "1"
    for i, (_, _, pair, code) in enumerate(np.asarray(obs).tolist()):
        m, e = lists[pair][code >> 1], "c" if code & 1 else "p"
        uv[i] = (m["u" + s + e], m["v" + s + e])
    return uv


# ---- tracks given as raw arrays --------------------------------------------------------------------------------------------------

def exact_case():
    """pixels that are exact in float32 (f = 512): point (0.5, 1, 8) seen from (0, 0, 0) and (1, 0, 0), so that initPoint lands on
    the point to a few ulps.  Returns the two poses and pixels."""
    poses = [[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], [1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0]]
    uv = [project(np.array(p, dtype=np.float64), (0.5, 1, 8), 512, 320, 240) for p in poses]
    assert uv == [(352.0, 304.0), (288.0, 304.0)]
    return poses, uv


def special_case():
    """seven tracks over five frames, f = 512, all of the point (0.5, 1, 8): [0] a regular one; [1] the same pixel from two
    cameras that differ by a translation: parallel rays (status 4); [2] with a middle camera whose principal plane holds the
    point: cc < 1e-10 (status 6); [3] seen through a frame without a pose (status 2); [4] over frames 0 and 3; [5] the
    regular one, flagged (status 1); [6] one observation (status 3)"""
    (p0, p1), (a0, a1) = exact_case()
    # frame 2: centre (1.5, 1, 8), so z_cam of the point is 0 there.  frame 3: further along the baseline.  frame 4: no pose.
    poses = [p0, p1, [1, 0, 0, 1.5, 0, 1, 0, 1, 0, 0, 1, 8], [1, 0, 0, 2, 0, 1, 0, 0, 0, 0, 1, 0], [1, 0, 0, 0.5, 0, 1, 0, 0, 0, 0, 1, 0]]
    a3 = project(np.array(poses[3], dtype=np.float64), (0.5, 1, 8), 512, 320, 240)
    a4 = project(np.array(poses[4], dtype=np.float64), (0.5, 1, 8), 512, 320, 240)
    tracks = [([0, 1], [a0, a1]), ([0, 1], [a0, a0]), ([0, 2, 1], [a0, (300.0, 200.0), a1]), ([0, 4, 1], [a0, a4, a1]), ([0, 3], [a0, a3]), ([0, 1], [a0, a1]),
              ([1], [a1])]
    offsets, fr, uv = [0], [], []
    for frames, px in tracks:
        fr += frames
        uv += px
        offsets.append(len(fr))
    return Case(poses, offsets, fr, uv, flags=[0, 0, 0, 0, 0, 1, 0], pose_valid=[1, 1, 1, 1, 0], f=512.0, cu=320.0, cv=240.0)


def outlier_case():
    """a gross outlier pixel: the point (-0.49, 0.39, 8.17) seen in frames 0, 1 and 3 of a path that also moves forward, its last
    pixel some 2400 px off.  The initial point falls behind the cameras, so point_type is -1 to let it
    through; Gauss-Newton then neither converges nor fails within the 22 updates (status 7), and stays finite.  The second track
    is the same without the outlier."""
    poses = [[1, 0, 0, 0.5 * k, 0, 1, 0, 0, 0, 0, 1, 0.1 * k] for k in range(4)]
    good = [project(np.array(poses[k], dtype=np.float64), (-0.49, 0.39, 8.17), 512, 320, 240) for k in (0, 1, 3)]
    return Case(poses, [0, 3, 6], [0, 1, 3, 0, 1, 3], [good[0], good[1], (1103.5, 2554.0)] + good, params=dict(point_type=-1), f=512.0, cu=320.0,
                cv=240.0)


def mid_invalid_case():
    """five frames 0.5 m apart on a baseline, frame 2 without a pose; the point (0.5, 1, 8).  Tracks over frames (1, 3): mid
    frame 2 has no pose -> frame 1; (0, 1): mid frame 0, not 1; (0, 4): mid frame 2 -> 1, not observed; (3, 4): mid frame 3.
    The four distances differ from each other and from what the neighbouring frame would give."""
    pts = (0.5, 1, 8)
    poses = [[1, 0, 0, 0.5 * k, 0, 1, 0, 0, 0, 0, 1, 0] for k in range(5)]
    px = [project(np.array(p, dtype=np.float64), pts, 512, 320, 240) for p in poses]
    fr = [1, 3, 0, 1, 0, 4, 3, 4]
    return Case(poses, [0, 2, 4, 6, 8], fr, [px[k] for k in fr], pose_valid=[1, 1, 0, 1, 1], f=512.0, cu=320.0, cv=240.0)


def tiny_focal_case():
    """f = 1e-11 with cu = cv = 0: initPoint and pointType are scale-free and succeed, but every entry of A = J^T J is about
    (f / z)^2 = 1e-24 - below Matrix::solve's eps of 1e-20, so the first pivot search ends the update (status 6, singular A)"""
    (p0, p1), _ = exact_case()
    f = 1e-11
    uv = [project(np.array(p, dtype=np.float64), (0.5, 1, 8), f, 0, 0) for p in (p0, p1)]
    return Case([p0, p1], [0, 2], [0, 1], uv, f=f, cu=0.0, cv=0.0)


def lengths_case():
    """66 frames on a slow path; tracks of 2, 3, 15, 16, 17, 33 and 65 observations, with and without pixel noise, and between them
    tracks that stop early (type -1, a flagged one, a one-observation one): mixed lengths and statuses inside one wave"""
    rng = np.random.default_rng(5)
    poses = camera_path(66, step=(0.06, 0.0, 0.01), yaw=0.002)
    offsets, fr, uv, flags = [0], [], [], []

    def add(frames, px, flag=0):
        fr.extend(frames)
        uv.extend(px)
        offsets.append(len(fr))
        flags.append(flag)

    for noise in (0.0, 0.5):
        for n in (2, 3, 15, 16, 17, 33, 65):
            X = (rng.uniform(-2, 2), rng.uniform(-1.4, 1.2), rng.uniform(6, 14))
            a = int(rng.integers(0, 66 - n + 1)) if n > 3 else 0
            frames = list(range(a, a + n)) if n > 3 else [0, 65][:n] if n == 2 else [0, 30, 65]
            px = [tuple(np.float32(c + noise * rng.uniform(-1, 1)) for c in project(poses[k], X)) for k in frames]
            add(frames, px)
            if n in (3, 17):
                add([0, 1], [px[0], px[0]])                      # one pixel in two frames: a point behind the cameras (type -1)
            if n == 16:
                add(frames, px, flag=1)                          # flagged
                add([frames[0]], [px[0]])                        # too short
    return Case(poses, offsets, fr, uv, flags=flags)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------

_cases = None
_refs = {}


def cases():
    global _cases
    if _cases is not None:
        return _cases
    c = {}
    big = build_scene(8, 288, seed=1)
    for pt in (-1, 0, 1, 2):
        c["scene_type%d" % pt] = big.with_(params=dict(point_type=pt))
    for n in (0, 1, 3, 4, 5, 63, 64, 65, 257):
        c["count_%d" % n] = big.first_tracks(n)
    c["noise_half_px"] = build_scene(12, 120, seed=2, noise=0.5)
    c["noise_half_px_type0"] = c["noise_half_px"].with_(params=dict(point_type=0))
    Rw = rot_y(0.7) @ rot_x(-0.4)
    c["world_frame"] = build_scene(6, 90, seed=3, world=(Rw, np.array([120.0, -35.0, 60.0])))
    c["world_frame_identity"] = build_scene(6, 90, seed=3)
    c["merged_tracks"] = build_scene(7, 45, seed=4, extra_matches=[(0, 0, 1, 9), (2, 10, 3, 11)], gaps=False)
    c["min_length_4"] = c["merged_tracks"].with_(params=dict(min_track_length=4))
    c["special"] = special_case()
    c["special_type_any"] = c["special"].with_(params=dict(point_type=-1))
    c["outlier"] = outlier_case()
    c["mid_invalid"] = mid_invalid_case()
    c["tiny_focal"] = tiny_focal_case()
    c["lengths"] = lengths_case()
    # distance and angle just inside and just outside their limits: the limits are set to the restatement's own values
    ex = c["special"].first_tracks(1)
    ref = R.triangulate(*ex.args()[0], **ex.args()[1])
    d, a = float(ref.dist[0]), float(ref.angle[0])
    assert ref.status[0] == 0 and 8 < d < 9 and 5 < a < 10
    c["dist_at_limit"] = ex.with_(params=dict(max_dist=d))                                  # dist < max_dist fails
    c["dist_inside"] = ex.with_(params=dict(max_dist=float(np.nextafter(d, np.inf))))
    c["angle_at_limit"] = ex.with_(params=dict(min_angle=a))                                # angle > min_angle fails
    c["angle_inside"] = ex.with_(params=dict(min_angle=float(np.nextafter(a, -np.inf))))
    _cases = c
    return c


def reference(name):
    if name not in _refs:
        a, kw = cases()[name].args()
        _refs[name] = R.triangulate(*a, **kw)
    return _refs[name]
