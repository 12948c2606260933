"""Inputs for the re-observation tests, without images.  cases() returns {name: Case}; reference(name) the restatement's result
(tests/reobserve_ref.py) and host(name) the host view's, each computed once per process and shared by the CPU and the GPU
suite.

Two families.  PLANTED scenes: random points in front of F posed cameras (the path of tests/points_cases.py); per point and
frame in which the restatement's own projection falls inside the image, a feature at the rounded projection with the point's
class and the point's random 32-byte descriptor, every byte moved by at most 1 per view (so two views of a point differ by at
most 2 per byte, 64 in all, where two random descriptors differ by some 2700); distractor features with fresh descriptors;
the features of a frame shuffled; each track observed in a random non-empty subset of its frames.  With radius >= 1 a planted
feature is in its window (rounding moves it by at most 0.5), so the expected result is exact: every planted, unobserved,
searched (point, frame) is accepted with the planted feature and nothing else is (Case.expected).
BUILT scenes: a camera with f = 1, cu = cv = 0 and identity poses, where the point (pu, pv, 1) projects to (pu, pv) exactly;
frame 0 holds every track's reference observation, the later frames are searched.  They put features on a window's edges, equal
costs, contested features, the cap and the ratio on their limits, and every reason and code into one call.  The sizes are the
smallest at which a 16-lane group per track or candidate, sixteen groups per workgroup and a scan of 256 items per workgroup can
go wrong."""
import numpy as np

import points_cases as PC
import reobserve_ref as RR
import resect_cases as RC
import resect_ref as R

TRACK_COUNTS = (0, 1, 15, 16, 17, 255, 256, 257)
FRAME_COUNTS = (1, 2, 9, 15, 16, 17, 33)
WINDOW_SIZES = (0, 1, 2, 15, 16, 17, 33)
CLAIMANTS = (2, 3, 17)
W, H = 1280, 400


def words(desc):
    """32 bytes -> the record's eight int32 words, lowest byte first"""
    return np.frombuffer(np.asarray(desc, dtype=np.uint8).tobytes(), dtype="<i4").tolist()


def byte_desc(first, fill=0):
    """a descriptor whose distance to byte_desc(0) is `first` (<= 255) when fill is 0"""
    return [first] + [fill] * 31


class Case:
    def __init__(self, poses, width, height, feats, tracks, xyz, use=None, ref_obs=None, search=None, pose_valid=None, params=None, f=1.0, cu=0.0, cv=0.0):
        """feats: per frame a list of (u, v, class, 32 bytes); tracks: per track a list of (frame, feature)"""
        self.poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(len(poses), 12)
        self.width, self.height = width, height
        self.feat_offsets = np.cumsum([0] + [len(x) for x in feats]).astype(np.int32)
        self.feat = np.array([[u, v, 0, c] + words(d) for fr in feats for (u, v, c, d) in fr], dtype=np.int32).reshape(-1, 12)
        self.offsets = np.cumsum([0] + [len(t) for t in tracks]).astype(np.int32)
        self.obs_frames = np.array([o[0] for t in tracks for o in t], dtype=np.int32)
        self.obs_feat = np.array([o[1] for t in tracks for o in t], dtype=np.int32)
        self.xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        as_bytes = lambda m: None if m is None else np.ascontiguousarray(m, dtype=np.uint8)
        self.use, self.search, self.pose_valid = as_bytes(use), as_bytes(search), as_bytes(pose_valid)
        self.ref_obs = None if ref_obs is None else np.ascontiguousarray(ref_obs, dtype=np.int32)
        self.params = dict(params or {})
        self.f, self.cu, self.cv = f, cu, cv
        self.expected = None  # planted scenes: {(track, frame): feature}
        self.tie_free = False

    def args(self):
        """positional and keyword arguments of host_reobserve / Matcher.reobserve / reobserve_ref.reobserve"""
        return ((self.poses, self.f, self.cu, self.cv, self.width, self.height, self.offsets, self.obs_frames, self.obs_feat, self.xyz, self.feat_offsets, self.feat),
                dict(use=self.use, ref_obs=self.ref_obs, search=self.search, pose_valid=self.pose_valid, params=self.params))

    def middle_refs(self):
        """ref_obs spelled out as the default: (length - 1) // 2"""
        return np.maximum((np.diff(self.offsets) - 1) // 2, 0).astype(np.int32)


# ---- planted scenes ---------------------------------------------------------------------------------------------------------

def planted(n_frames, n_points, seed, distractors=40, empty_frame=None, observe_all=(), params=None, search=None, use=None, pose_valid=None):
    rng = np.random.default_rng(seed)
    poses = PC.camera_path(n_frames, step=(0.06, -0.002, 0.03), yaw=0.002)
    prm = dict(RR.DEFAULTS, **(params or {}))
    states = [R.rigid_inverse([float(x) for x in np.asarray(p).reshape(12)]) for p in poses]
    # n_points points that some frame other than the empty one sees, out of a larger draw
    pool = RC.visible_points(2 * n_points + 8, rng)
    in_view = [any(isinstance(RR.project(states[g], [float(x) for x in X], PC.F, PC.CU, PC.CV, prm["min_depth"], W, H), tuple) for g in range(n_frames) if g != empty_frame)
               for X in pool]
    pts = pool[np.nonzero(in_view)[0][:n_points]].reshape(-1, 3)
    assert len(pts) == n_points
    cls = rng.integers(0, 4, n_points)
    desc = rng.integers(1, 255, (n_points, 32))
    feats = [[] for _ in range(n_frames)]
    where = {}  # (point, frame) -> position in feats[frame] before the shuffle
    for t in range(n_points):
        for g in range(n_frames):
            p = RR.project(states[g], [float(x) for x in pts[t]], PC.F, PC.CU, PC.CV, prm["min_depth"], W, H)
            if isinstance(p, tuple) and g != empty_frame:
                where[(t, g)] = len(feats[g])
                feats[g].append((int(np.rint(p[0])), int(np.rint(p[1])), int(cls[t]), (desc[t] + rng.integers(-1, 2, 32)).tolist()))
    for g in range(n_frames):
        if g != empty_frame:
            for _ in range(distractors):
                feats[g].append((int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(0, 4)), rng.integers(0, 256, 32).tolist()))
    new_index = []
    for g in range(n_frames):
        perm = rng.permutation(len(feats[g]))  # perm[new] = old
        feats[g] = [feats[g][i] for i in perm]
        new_index.append(np.argsort(perm))
    tracks, keep = [], []
    for t in range(n_points):
        seen = [g for g in range(n_frames) if (t, g) in where]
        if not seen:
            continue
        sub = seen if t in observe_all else sorted(rng.choice(seen, size=int(rng.integers(1, len(seen) + 1)), replace=False).tolist())
        tracks.append([(g, int(new_index[g][where[(t, g)]])) for g in sub])
        keep.append(t)
    c = Case(poses, W, H, feats, tracks, pts[keep], params=params, search=search, pose_valid=pose_valid, f=PC.F, cu=PC.CU, cv=PC.CV,
             use=None if use is None else np.asarray(use)[:len(keep)])
    c.expected = {}
    for i, t in enumerate(keep):
        if c.use is not None and not c.use[i]:
            continue
        mine = set(g for g, _ in tracks[i])
        for g in range(n_frames):
            if (t, g) in where and g not in mine and (c.search is None or c.search[g]) and (c.pose_valid is None or c.pose_valid[g]):
                c.expected[(i, g)] = int(new_index[g][where[(t, g)]])
    c.tie_free = True
    return c


# ---- built scenes: f = 1, cu = cv = 0, identity poses --------------------------------------------------------------------------

IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]


class Builder:
    def __init__(self, n_frames, width, height, seed=0):
        self.n, self.width, self.height = n_frames, width, height
        self.feats = [[] for _ in range(n_frames)]
        self.tracks, self.xyz, self.use = [], [], []
        self.rng = np.random.default_rng(seed)
        self.next_ref = 0

    def feature(self, g, u, v, cls=0, desc=None):
        self.feats[g].append((u, v, cls, self.rng.integers(0, 256, 32).tolist() if desc is None else desc))
        return len(self.feats[g]) - 1

    def track(self, pu, pv, cls=0, desc=None, z=1.0, use=1, more=(), X=None):
        """a track whose reference observation is a new feature of frame 0 and whose point projects to (pu, pv) in every frame;
        more: further observations (frame, feature)"""
        k = self.feature(0, self.next_ref % self.width, (self.next_ref // self.width) % self.height, cls, desc)
        self.next_ref += 1
        self.tracks.append([(0, k)] + list(more))
        self.xyz.append([pu * z, pv * z, z] if X is None else X)
        self.use.append(use)
        return len(self.tracks) - 1

    def case(self, **kw):
        poses = kw.pop("poses", [IDENTITY] * self.n)
        return Case(poses, self.width, self.height, self.feats, self.tracks, self.xyz, use=self.use, **kw)


def windows_case():
    """track i's window in frame 1 holds WINDOW_SIZES[i] features of its class 1 and, from the second on, one feature of each
    other class beside them; the windows are 40 pixels apart"""
    b = Builder(2, 400, 60, seed=1)
    for i, n in enumerate(WINDOW_SIZES):
        pu, pv = 20.0 + 40 * i, 30.0
        b.track(pu, pv, cls=1)
        for j in range(n):
            b.feature(1, int(pu) - 3 + j % 7, int(pv) - 3 + j // 7, 1)
        if i:
            for c in (0, 2, 3):
                b.feature(1, int(pu) + c - 1, int(pv) + 4, c, desc=b.feats[0][i][3])  # (the reference's own bytes: cost 0, wrong class)
    c = b.case()
    c.tie_free = True
    return c


def sweep_case(radius, shift=0.0, width=130):
    """the projection swept pixel by pixel across a frame 130 wide (at u + shift), over a grid of features at every u in the rows
    v0 - (r + 1), v0 - r, v0, v0 + r, v0 + r + 1 with r = floor(radius): whatever the bins, a feature stands exactly at +-r and
    +-(r + 1) of every projection, in u and in v.  Neighbouring tracks contest the same features."""
    r = int(np.floor(radius))
    v0 = r + 3
    b = Builder(2, width, 2 * v0 + 1, seed=2)
    for dv in (-(r + 1), -r, 0, r, r + 1):
        for u in range(width):
            b.feature(1, u, v0 + dv, 2)
    for u in range(width):
        if u + shift <= width - 1:
            b.track(u + shift, float(v0), cls=2)
    return b.case(params=dict(radius=radius))


def edges_case():
    """projections exactly at 0 and width - 1 / height - 1 (candidates), and the next doubles outside; depths behind, at and just
    above min_depth; NaN and infinite points, points at 1e200 (one in view: 2^665 is 1.5e200, and 30 * 2^665 / 2^665 is 30 exactly); a frame whose pose holds a NaN and one that holds an infinity"""
    width, height = 64, 48
    b = Builder(4, width, height, seed=3)
    for g in (1, 2, 3):
        for u, v in ((0, 0), (width - 1, height - 1), (0, height - 1), (width - 1, 0), (30, 20)):
            b.feature(g, u, v, 0)
    inside = [(0.0, 0.0), (width - 1.0, height - 1.0), (0.0, height - 1.0), (width - 1.0, 0.0)]
    outside = [(-5e-324, 5.0), (np.nextafter(width - 1.0, np.inf), 5.0), (5.0, -1e-300), (5.0, np.nextafter(height - 1.0, np.inf))]
    for pu, pv in inside + outside:
        b.track(pu, pv)
    md = 0.25
    for z in (-1.0, 0.0, md, np.nextafter(md, 1.0)):
        b.track(0, 0, X=[30.0 * z, 20.0 * z, z])
    for X in ([np.nan, 1, 1], [1, np.nan, 1], [1, 1, np.nan], [np.inf, 1, 1], [1, 1, np.inf], [-np.inf, np.inf, 1], [30 * 2.0 ** 665, 20 * 2.0 ** 665, 2.0 ** 665], [1e200, 1e200, 1.0]):
        b.track(0, 0, X=X)
    b.track(30.0, 20.0)
    poses = [list(IDENTITY) for _ in range(4)]
    poses[2][3] = np.nan
    poses[3][5] = np.inf
    c = b.case(poses=poses, params=dict(min_depth=md))
    c.n_inside, c.n_outside = len(inside), len(outside)
    return c


def ties_case():
    """equal costs inside a window: the lowest feature index wins and second equals best; then a window whose only features
    are two equal ones behind an occupied feature that would win (cost 0) - occupied by a track that is not in use"""
    b = Builder(2, 100, 40, seed=4)
    ref = byte_desc(0)
    b.track(20.0, 20.0, desc=ref)
    b.feature(1, 22, 20, 0, byte_desc(9))
    b.feature(1, 18, 21, 0, byte_desc(7))
    b.feature(1, 21, 19, 0, byte_desc(7))
    b.feature(1, 20, 20, 0, byte_desc(7))
    b.track(60.0, 20.0, desc=ref)
    taken = b.feature(1, 60, 20, 0, byte_desc(0))
    b.feature(1, 61, 20, 0, byte_desc(5))
    b.feature(1, 59, 20, 0, byte_desc(5))
    b.track(90.0, 5.0, use=0, more=[(1, taken)])
    c = b.case()
    c.taken = taken
    return c


def claims_case():
    """CLAIMANTS[i] tracks project onto one feature of frame 1, twice: with unequal costs (the last track of the group is nearest
    and keeps it) and with equal costs (the first candidate keeps it); a loser does not fall back to its second"""
    b = Builder(2, 200, 40, seed=5)
    unequal, equal = [], []
    for i, n in enumerate(CLAIMANTS):
        u = 30 + 60 * i
        b.feature(1, u, 10, 0, byte_desc(100))
        b.feature(1, u + 1, 10, 0, byte_desc(200, 3))  # everybody's second
        unequal.append([b.track(float(u), 10.0, desc=byte_desc(100 - n + j)) for j in range(n)])
        b.feature(1, u, 30, 0, byte_desc(9))
        b.feature(1, u - 1, 30, 0, byte_desc(90, 1))
        equal.append([b.track(float(u), 30.0, desc=byte_desc(7)) for j in range(n)])
    c = b.case()
    c.unequal, c.equal = unequal, equal
    return c


def limits_case():
    """max_cost = 40 and ratio 1 / 2: best 40 passes the cap, best 41 does not; best 10 against second 21 passes the ratio, against
    second 20 it does not (10 * 2 < 20 * 1 is false); a single feature has no second and passes"""
    b = Builder(2, 300, 40, seed=6)
    for i, (best, second) in enumerate(((40, 255), (41, 255), (10, 21), (10, 20), (0, None), (0, 0), (40, 80), (40, 81))):
        u = 20 + 30 * i
        b.track(float(u), 20.0, desc=byte_desc(0))
        b.feature(1, u, 20, 0, byte_desc(best))
        if second is not None:
            b.feature(1, u + 2, 21, 0, byte_desc(second))
    return b.case(params=dict(max_cost=40, ratio_num=1, ratio_den=2))


LIMITS_CODES = [0, 2, 0, 3, 0, 3, 3, 0]


def everything_case():
    """every reason and every code in one call of five frames: frame 1 is not searched, frame 2 has no valid pose, frames 3 and
    4 are searched.  Tracks: 0 accepted in 3 and 4; 1 also observed in 3; 2 behind; 3 outside; 4 with an empty window; 5 over
    the cap; 6 ambiguous; 7 and 8 contest one feature; 9 not in use; 10 without an observation."""
    b = Builder(5, 200, 40, seed=7)
    z = byte_desc(0)
    b.track(10.0, 10.0, desc=z)
    for g in (3, 4):
        b.feature(g, 10, 10, 0, byte_desc(3))
    k = b.feature(3, 30, 10, 0, byte_desc(1))
    b.track(30.0, 10.0, desc=z, more=[(3, k)])
    b.feature(4, 30, 10, 0, byte_desc(2))
    b.track(0, 0, X=[1.0, 1.0, -2.0])
    b.track(500.0, 10.0)
    b.track(50.0, 30.0, cls=3)
    b.track(70.0, 10.0, desc=z)
    b.track(90.0, 10.0, desc=z)
    b.track(110.0, 10.0, desc=z)
    b.track(111.0, 10.0, desc=byte_desc(1))
    for g in (3, 4):
        b.feature(g, 70, 10, 0, byte_desc(200))
        b.feature(g, 90, 10, 0, byte_desc(10))
        b.feature(g, 91, 10, 0, byte_desc(12))
        b.feature(g, 110, 10, 0, byte_desc(5))
    b.track(10.0, 10.0, desc=z, use=0)
    c = b.case(search=[1, 0, 1, 1, 1], pose_valid=[1, 1, 0, 1, 1], params=dict(max_cost=100, ratio_num=1, ratio_den=2))
    # a track without an observation, in use: it has no reference and counts as not in use
    c.offsets = np.append(c.offsets, c.offsets[-1]).astype(np.int32)
    c.xyz = np.vstack([c.xyz, [[10.0, 10.0, 1.0]]])
    c.use = np.append(c.use, 1).astype(np.uint8)
    return c


def masks_case():
    """search, use and pose_valid masks over a planted scene of six frames"""
    return planted(6, 30, seed=70, search=[1, 0, 1, 1, 0, 1], pose_valid=[1, 1, 0, 1, 1, 1], use=[i % 4 != 1 for i in range(30)])


_cases = None
_refs, _hosts = {}, {}


def cases():
    global _cases
    if _cases is not None:
        return _cases
    c = {}
    for n in TRACK_COUNTS:
        c["tracks_%d" % n] = planted(3, n, seed=100 + n, distractors=30)
    for n in FRAME_COUNTS:
        c["frames_%d" % n] = planted(n, 12, seed=200 + n, distractors=20)
    c["empty_frame"] = planted(4, 20, seed=300, empty_frame=2)
    c["all_observed"] = planted(3, 10, seed=301, observe_all=range(10))  # every track in every frame that sees it: n_cand = 0
    c["one_all_observed"] = planted(5, 18, seed=302, observe_all=(3,))
    c["no_distractors"] = planted(4, 17, seed=303, distractors=0)
    c["radius_1"] = planted(4, 40, seed=304, params=dict(radius=1.0))
    c["masks"] = masks_case()
    c["windows"] = windows_case()
    c["sweep_4"] = sweep_case(4.0)
    c["sweep_2_5"] = sweep_case(2.5)
    c["sweep_2_5_half"] = sweep_case(2.5, shift=0.5)
    c["sweep_0"] = sweep_case(0.0)
    c["edges"] = edges_case()
    c["ties"] = ties_case()
    c["claims"] = claims_case()
    c["limits"] = limits_case()
    c["everything"] = everything_case()
    c["no_frames"] = Case(np.zeros((0, 12)), 10, 10, [], [], np.zeros((0, 3)))
    _cases = c
    return c


def reference(name):
    if name not in _refs:
        a, kw = cases()[name].args()
        _refs[name] = RR.reobserve(*a, **kw)
    return _refs[name]


def host(name):
    from conftest import pkg
    if name not in _hosts:
        a, kw = cases()[name].args()
        _hosts[name] = pkg("visomatch").host_reobserve(*a, **kw)
    return _hosts[name]
