"""Inputs for the location tests (vsm_host_locate, Matcher.locate), no images: a camera path (tests/points_cases.py), random 3-D
points in a volume in front of the cameras - not planar -, and the pixels of the points in the frames that see them, projected
exactly and rounded to float32.  The call is given no pose; true_poses is what it should find.  cases() returns {name: Case};
host(name) the host view's result, computed once per process and shared by the tests that need it.

Row counts: rows_family (and rows_family_6 with min_inliers = 6) has frames with E = 0, 5, 6, 7, 9, 10, 11, 15, 16, 17, 255, 256,
257 and 513 eligible rows - either side of min_inliers, of a 16-lane group, of the count kernel's tile of 256 rows and of its
second and third tile.  Hypothesis counts: iters_1, 15, 16, 17, 33, 200 on three frames - either side of a group run of 16 and
of a fit block of 16 groups, so that with K = 15, 17 and 33 a fit block is shared by two frames.  Shapes: 1, 2 and 9 frames, and
257 frames of 10 to 12 rows.  outliers_tiles: a late winner on frames of 255, 257 and 513 rows."""
import numpy as np

import points_cases as PC
import resect_cases as RC

F, CU, CV = PC.F, PC.CU, PC.CV
ROW_COUNTS = (0, 5, 6, 7, 9, 10, 11, 15, 16, 17, 255, 256, 257, 513)
ITERS = (1, 15, 16, 17, 33, 200)
FIELDS = ("status", "poses", "linear_poses", "best", "inliers", "rows", "eligible", "updates", "used", "ss_after", "rms_after")


class Case:
    def __init__(self, n_frames, tracks, xyz, use=None, locate=None, params=None, true_poses=None, clean=None, f=F, cu=CU, cv=CV):
        """tracks: per track a list of (frame, u, v); clean: per observation, whether its pixel is the point's projection"""
        self.n_frames = int(n_frames)
        self.offsets = np.cumsum([0] + [len(t) for t in tracks]).astype(np.int32)
        obs = [o for t in tracks for o in t]
        self.obs_frames = np.array([o[0] for o in obs], dtype=np.int32)
        self.uv = np.array([(o[1], o[2]) for o in obs], dtype=np.float32).reshape(-1, 2)
        self.xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.use = None if use is None else np.ascontiguousarray(use, dtype=np.uint8)
        self.locate = None if locate is None else np.ascontiguousarray(locate, dtype=np.uint8)
        self.params = dict(params or {})
        self.true_poses = None if true_poses is None else np.ascontiguousarray(true_poses, dtype=np.float64).reshape(self.n_frames, 12)
        self.clean = None if clean is None else np.ascontiguousarray(clean, dtype=bool)
        self.f, self.cu, self.cv = f, cu, cv

    def args(self):
        """positional and keyword arguments of host_locate / Matcher.locate"""
        return ((self.n_frames, self.f, self.cu, self.cv, self.offsets, self.obs_frames, self.uv, self.xyz), dict(use=self.use, locate=self.locate, params=self.params))

    def tracks_args(self):
        """the arguments host_resect and host_vet share behind the poses"""
        return (self.f, self.cu, self.cv, self.offsets, self.obs_frames, self.uv, self.xyz)


def volume(n, rng):
    """n points in the frame of camera 0, 5 to 20 m ahead, within the field of view of every camera of a short path"""
    z = rng.uniform(5, 20, n)
    return np.stack([rng.uniform(-0.25, 0.25, n) * z, rng.uniform(-0.12, 0.12, n) * z, z], axis=1)


def scene(n_frames, n_points, seed, seen=1.0, **kw):
    rng = np.random.default_rng(seed)
    true = PC.camera_path(n_frames)
    pts = volume(n_points, rng)
    tracks = [[(g,) + RC.pixel(true[g], X) for g in range(n_frames) if rng.uniform() < seen] for X in pts]
    return Case(n_frames, tracks, pts, true_poses=true, **kw)


def rows_family(**params):
    """frame g has exactly ROW_COUNTS[g] rows, all eligible: point i is seen by the frames with more than i rows"""
    rng = np.random.default_rng(31)
    true = PC.camera_path(len(ROW_COUNTS), step=(0.06, 0.0, 0.01), yaw=0.002)
    pts = volume(max(ROW_COUNTS), rng)
    tracks = [[(g,) + RC.pixel(true[g], X) for g, n in enumerate(ROW_COUNTS) if i < n] for i, X in enumerate(pts)]
    return Case(len(ROW_COUNTS), tracks, pts, true_poses=true, params=params)


def many_frames():
    """257 frames of 10, 11 or 12 rows on twelve points: more frames than a block has threads; 17 hypotheses each"""
    rng = np.random.default_rng(32)
    n = 257
    true = PC.camera_path(n, step=(0.01, 0.0, 0.004), yaw=0.0005)
    pts = volume(12, rng)
    tracks = [[(g,) + RC.pixel(true[g], X) for g in range(n) if i < 10 + g % 3] for i, X in enumerate(pts)]
    return Case(n, tracks, pts, true_poses=true, params=dict(ransac_iters=17))


def statuses_case():
    """seven frames, one per status, in the order 1, 2, 3, 4, 5, 0, 6 (max_updates = 1, eps = 1e-3, inlier_threshold = 8): [0] not
    asked for; [1] seven rows; [2] twelve rows of twelve tracks with one and the same point: the scale is zero, no hypothesis is
    valid; [3] twelve rows, eight of them with pixels from nowhere: no hypothesis finds ten; [4] fourteen points 1e14 m away: the
    linear fit stands, but the translation's entries of the normal equations are about (f / z)^2 = 1e-22, below the solver's 1e-20:
    no pivot; [5] clean pixels: the linear pose is within eps of the optimum; [6] pixels with up to 1.5 px of noise: it is not"""
    rng = np.random.default_rng(33)
    true = PC.camera_path(7, step=(0.06, 0.0, 0.01), yaw=0.0)
    pts = list(volume(40, rng))
    tracks = [[(g,) + RC.pixel(true[g], X) for g in (0, 5)] + [(6,) + RC.pixel(true[6], X, tuple(rng.uniform(-1.5, 1.5, 2)))] for X in pts]
    for i in range(7):
        tracks[i].append((1,) + RC.pixel(true[1], pts[i]))
    for i in range(4):
        tracks[i].append((3,) + RC.pixel(true[3], pts[i]))
    for k in range(12):  # frame 2: one point twelve times
        pts.append(np.array([0.5, -0.25, 9.0]))
        tracks.append([(2,) + RC.pixel(true[2], pts[-1])])
    for k in range(8):  # frame 3: pixels from nowhere
        pts.append(volume(1, rng)[0])
        tracks.append([(3, float(np.float32(rng.uniform(50, 1190))), float(np.float32(rng.uniform(20, 350))))])
    for X in volume(14, rng) * 1e13:  # frame 4: very far away
        pts.append(X)
        tracks.append([(4,) + RC.pixel(true[4], X)])
    return Case(7, tracks, pts, locate=[0, 1, 1, 1, 1, 1, 1], params=dict(max_updates=1, eps=1e-3, inlier_threshold=8.0), true_poses=true)


def mask_case():
    c = scene(6, 40, seed=34, seen=0.9)
    c.locate = np.array([0, 1, 1, 0, 1, 0], np.uint8)
    return c


def nan_case():
    """NaN and infinite pixels, NaN and infinite points among the rows: never sampled, never counted"""
    c = scene(3, 50, seed=35)
    uv, xyz = c.uv.copy(), c.xyz.copy()
    uv[5, 0] = np.nan
    uv[17, 1] = np.nan
    uv[40] = (np.nan, np.nan)
    uv[77, 0] = np.inf
    uv[90, 1] = -np.inf
    xyz[7, 2] = np.nan
    xyz[11, 0] = np.inf
    xyz[12, 1] = -np.inf
    c.uv, c.xyz = uv, xyz
    return c


def unused_case():
    """every fifth track unused, its point NaN (a track the triangulation dropped)"""
    c = scene(3, 60, seed=36)
    c.use = np.ones(60, np.uint8)
    c.use[::5] = 0
    c.xyz[::5] = np.nan
    return c


def behind_case():
    """a third of the points lie behind the cameras: eligible rows that no valid hypothesis samples and none counts"""
    rng = np.random.default_rng(37)
    true = PC.camera_path(3)
    front = iter(volume(60, rng))
    pts = [np.array([rng.uniform(-2, 2), rng.uniform(-1, 1), -rng.uniform(2, 9)]) if k % 3 == 2 else next(front) for k in range(90)]
    tracks = [[(g,) + RC.pixel(true[g], X) for g in range(3)] for X in pts]
    return Case(3, tracks, pts, true_poses=true)


def duplicates_case():
    """every third track is a copy of the track in front of it, point and pixels: samples with repeated rows"""
    rng = np.random.default_rng(38)
    true = PC.camera_path(2)
    base = volume(30, rng)
    pts = [base[i - 1] if i % 3 == 2 else base[i] for i in range(30)]
    tracks = [[(g,) + RC.pixel(true[g], X) for g in range(2)] for X in pts]
    return Case(2, tracks, pts, true_poses=true)


def identical_case():
    """frame 0 sees six copies of one point beside 24 others, frame 1 the six copies and four others (E = 10), frame 2 twelve
    copies alone"""
    rng = np.random.default_rng(39)
    true = PC.camera_path(3)
    one = np.array([-0.75, 0.5, 11.0])
    others = volume(24, rng)
    pts = [one] * 12 + list(others)
    tracks = [[(0,) + RC.pixel(true[0], one), (1,) + RC.pixel(true[1], one), (2,) + RC.pixel(true[2], one)] for _ in range(6)]
    tracks += [[(2,) + RC.pixel(true[2], one)] for _ in range(6)]
    tracks += [[(0,) + RC.pixel(true[0], X)] + ([(1,) + RC.pixel(true[1], X)] if i < 4 else []) for i, X in enumerate(others)]
    return Case(3, tracks, pts, true_poses=true)


def planar_case():
    """every point on one tilted plane: the linear fit's known limit"""
    rng = np.random.default_rng(40)
    true = PC.camera_path(3)
    pts = volume(60, rng)
    pts[:, 2] = 12.0 + 0.3 * pts[:, 0] - 0.2 * pts[:, 1]
    tracks = [[(g,) + RC.pixel(true[g], X) for g in range(3)] for X in pts]
    return Case(3, tracks, pts, true_poses=true)


def huge_case():
    """one point at 1e200 among the rows of every frame: its samples' mean and scale are 1e199, everything stays finite"""
    c = scene(3, 40, seed=41)
    c.xyz[13] = (1e200, -1e200, 1e200)
    return c


def outliers_case():
    """30 % planted outliers: the pixel displaced by 50 to 120 px in a random direction; 9 frames, 60 points each"""
    rng = np.random.default_rng(42)
    n = 9
    true = PC.camera_path(n)
    pts = volume(60, rng)
    tracks, clean = [], []
    for X in pts:
        t = []
        for g in range(n):
            bad = rng.uniform() < 0.3
            a, r = rng.uniform(0, 2 * np.pi), rng.uniform(50, 120)
            t.append((g,) + RC.pixel(true[g], X, (r * np.cos(a), r * np.sin(a)) if bad else (0.0, 0.0)))
            clean.append(not bad)
        tracks.append(t)
    return Case(n, tracks, pts, true_poses=true, clean=clean)


TILE_ROWS = (255, 257, 513)


def outliers_tiles_case():
    """30 % planted outliers as in outliers_case on frames of 255, 257 and 513 rows, 33 hypotheses: the winner comes late, and the
    counts of every hypothesis differ from tile to tile and from wave to wave of the count kernel"""
    rng = np.random.default_rng(45)
    true = PC.camera_path(len(TILE_ROWS))
    pts = volume(max(TILE_ROWS), rng)
    tracks, clean = [], []
    for i, X in enumerate(pts):
        t = []
        for g, n in enumerate(TILE_ROWS):
            if i >= n:
                continue
            bad = rng.uniform() < 0.3
            a, r = rng.uniform(0, 2 * np.pi), rng.uniform(50, 120)
            t.append((g,) + RC.pixel(true[g], X, (r * np.cos(a), r * np.sin(a)) if bad else (0.0, 0.0)))
            clean.append(not bad)
        tracks.append(t)
    return Case(len(TILE_ROWS), tracks, pts, true_poses=true, clean=clean, params=dict(ransac_iters=33))


def frame_rows(c, g):
    """frame g's rows in the call's order - ascending (track, observation) - as (uv [n, 2] float32, xyz [n, 3]), a point per row"""
    use = np.ones(len(c.offsets) - 1, bool) if c.use is None else c.use.astype(bool)
    track = np.repeat(np.arange(len(c.offsets) - 1), np.diff(c.offsets))
    at = np.nonzero((c.obs_frames == g) & use[track])[0]
    return np.ascontiguousarray(c.uv[at]), np.ascontiguousarray(c.xyz[track[at]])


def degenerate_rows():
    """a frame of rows for the degenerate samples and the picks that make them: (uv, xyz, {name: pick})"""
    c = cases()["rows_family"]
    g = ROW_COUNTS.index(17)
    uv, xyz = frame_rows(c, g)
    uv, xyz = [tuple(x) for x in uv.tolist()], [tuple(x) for x in xyz.tolist()]
    pose = c.true_poses[g]
    def add(X):
        xyz.append(tuple(float(x) for x in X))
        uv.append(RC.pixel(pose, np.asarray(X, dtype=np.float64)))
        return len(xyz) - 1

    picks = {"ordinary": [0, 1, 2, 3, 4, 5], "one_row_six_times": [3] * 6, "two_rows_three_times": [2, 9, 2, 9, 2, 9]}
    picks["one_point_six_rows"] = [add((0.5, -0.25, 9.0)) for _ in range(6)]
    picks["coplanar"] = [add((x, y, 12.0 + 0.3 * x - 0.2 * y)) for x, y in ((-2, -1), (1.5, -0.8), (0.3, 0.9), (-1.1, 0.4), (2.2, 0.1), (-0.4, -0.6))]
    picks["collinear"] = [add((0.2 * t - 1.0, 0.1 * t, 8.0 + 0.5 * t)) for t in range(6)]
    far = len(xyz)
    xyz.append((1e200, -1e200, 1e200))
    uv.append((600.0, 200.0))
    picks["huge"] = [0, 1, 2, 3, 4, far]
    big = len(xyz)
    xyz.extend([(1.7e308, 1.7e308, 1.7e308), (1.7e308, -1.7e308, 1.7e308), (-1.7e308, 1.7e308, -1.7e308)])
    uv.extend([(600.0, 200.0)] * 3)
    picks["overflow"] = [big, big, big + 1, big + 2, 0, 1]
    behind = add((0.3, -0.2, -6.0))
    picks["one_behind"] = [0, 1, 2, 3, 4, behind]
    return np.array(uv, np.float32), np.array(xyz, np.float64), picks


def host_hypotheses(vm, c, g, p, fill=0.0):
    """frame g's rows and every hypothesis of it through the host entries: (uv, xyz, picks as row indices, states, valid, counts)"""
    uv, xyz = frame_rows(c, g)
    elig = np.nonzero(np.isfinite(uv).all(axis=1) & np.isfinite(xyz).all(axis=1))[0]
    picks = elig[vm.host_locate_sample(p.seed, len(elig), p.ransac_iters)].astype(np.int32)
    states, valid = vm.host_locate_fit(c.f, c.cu, c.cv, uv, xyz, picks, p.min_depth, fill=fill)
    counts = vm.host_locate_count(c.f, c.cu, c.cv, uv, xyz, states, valid, p.inlier_threshold, p.min_depth)
    return uv, xyz, picks, states, valid, counts


_cases = None
_host = {}


def cases():
    global _cases
    if _cases is not None:
        return _cases
    c = {}
    c["rows_family"] = rows_family()
    c["rows_family_6"] = rows_family(min_inliers=6)
    for k in ITERS:
        c["iters_%d" % k] = scene(3, 40, seed=43, params=dict(ransac_iters=k))
    for n in (1, 2, 9):
        c["frames_%d" % n] = scene(n, 30, seed=50 + n)
    c["frames_257"] = many_frames()
    c["statuses"] = statuses_case()
    c["mask"] = mask_case()
    c["nan"] = nan_case()
    c["unused"] = unused_case()
    c["behind"] = behind_case()
    c["duplicates"] = duplicates_case()
    c["identical"] = identical_case()
    c["planar"] = planar_case()
    c["huge"] = huge_case()
    c["outliers"] = outliers_case()
    c["outliers_tiles"] = outliers_tiles_case()
    c["seed_0"] = scene(2, 30, seed=44, params=dict(seed=0))
    c["no_tracks"] = Case(3, [], np.zeros((0, 3)))
    c["no_frames"] = Case(0, [], np.zeros((0, 3)))
    _cases = c
    return c


def host(name):
    """vsm_host_locate on the case, once per process"""
    from conftest import pkg
    if name not in _host:
        a, kw = cases()[name].args()
        _host[name] = pkg("visomatch").host_locate(*a, **kw)
    return _host[name]


def assert_same(got, want, what=""):
    """two Location results: every int equal, every double equal by its bytes"""
    for n in FIELDS:
        a, b = np.ascontiguousarray(getattr(got, n)), np.ascontiguousarray(getattr(want, n))
        assert a.shape == b.shape and a.dtype == b.dtype, (what, n, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (what, n, a.tolist(), b.tolist())
