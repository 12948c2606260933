"""Inputs that pin the track triangulation and the track linking to the reference's Reconstruction class
(viso/reconstruction.{h,cpp}), and the comparison both suites use (test_points_vs_ref.py on the CPU, test_points_ref_gpu.py
on the device).  The reference's side is oracle.bindings.ref_recon_tracks / ref_recon_sequence; its recorded outputs are in
tests/golden/reconstruction_ref.npz, so that the device suite runs without the compiled reference.

THE CONVENTION is the reference's.  A sequence has at most 6 images, so a track has at most 6 pixels and the class's
max_track_length of 6 never binds (update() only adds a pixel while a track has fewer than 6; with 6 images the sixth is the
last there can be).  update() number k (1, 2, ..) pushes frame state k and links the matches between images k - 1 and k; the class
pairs pixel i of a track that starts in image a with state a + 1 + i, the state of the update AFTER the image (the one-frame shift
that include/visomatch.h documents).  So here pixel i of a track is the projection of its point into state first image + 1 + i,
rounded to float32, and the library's call gets obs_frames = image + 1 with pose k = rows 0..2 of state k's fwd: both sides then
use the same matrices for the same pixel.  State 0 is a dummy (the identity) that no track names.

How the four deviations the header lists are neutralised: the 6-pixel cap and the frame pairing as just said; the rigid inverse
differs from Matrix::inv on a rotation-and-translation by a few double ulps, far inside float32 rounding; and the float point
is what the agreement bound BOUND below measures.

Cameras look along +z with y down; a point 1.6 m below the camera is on the road (Tr_cam_road: pitch -0.08, height 1.6)."""
import math
import os

import numpy as np

import points_cases as PC
import points_ref as R

F, CU, CV = PC.F, PC.CU, PC.CV
N_IMAGES = 6
N_TRACKS = 260     # per family: prefixes of 1 .. 257 tracks are what the device suite runs
COUNTS = (1, 15, 17, 63, 65, 255, 257)

# The largest |ours - reference| / max(1, |reference|) over xyz, dist and angle of all kept tracks of all families, measured with
# vsm_host_triangulate on the CPU (test_points_vs_ref.py prints it): the reference keeps the point as three floats through
# initPoint and the Gauss-Newton loop, so this is float32 rounding.  The tests assert 4 times that - room for the rounding that
# moves with another machine's libm and compiler - and that the bound stays under 1e-4.
MEASURED = 7.6e-7  # (7.594e-7, in the family "stray", whose kept tracks carry a gross outlier; 5.4e-8 to 8.0e-8 in the others)
BOUND = 4 * MEASURED


class Family:
    """one set of tracks over one sequence of states, with the parameters it is run with"""

    def __init__(self, fwd, offsets, uv, first_image, params=None, inputs=None):
        self.fwd = np.ascontiguousarray(fwd, dtype=np.float64).reshape(-1, 4, 4)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        self.uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
        self.first_image = np.ascontiguousarray(first_image, dtype=np.int32)
        self.params = dict(params or {})
        self.inputs = inputs  # the family whose arrays these are (a variant differs in its parameters only)

    def __len__(self):
        return len(self.first_image)

    def variant(self, inputs, **params):
        return Family(self.fwd, self.offsets, self.uv, self.first_image, params, inputs)

    def prefix(self, n):
        off = self.offsets[:n + 1]
        return Family(self.fwd, off, self.uv[:int(off[-1])], self.first_image[:n], self.params, self.inputs)

    @property
    def poses(self):
        return np.ascontiguousarray(self.fwd[:, :3, :]).reshape(-1, 12)

    @property
    def obs_frames(self):
        """image + 1: the state the reference pairs every pixel with"""
        n = np.diff(self.offsets)
        return (np.repeat(self.first_image + 1 - self.offsets[:-1], n) + np.arange(int(self.offsets[-1]))).astype(np.int32)

    def ours(self):
        """positional and keyword arguments of host_triangulate / Matcher.triangulate / points_ref.triangulate"""
        return (self.poses, F, CU, CV, self.offsets, self.obs_frames, self.uv), dict(params=self.params)

    def reference(self, B):
        """the class itself on these tracks (oracle.bindings)"""
        return B.ref_recon_tracks(F, CU, CV, self.fwd, self.offsets, self.uv, self.first_image + 1, **self.params)


# ---- geometry -------------------------------------------------------------------------------------------------------------------

def states(centres, yaws):
    """fwd of states 1 .. n (camera to world, [R | c]) behind the dummy state 0"""
    out = [np.eye(4)]
    for c, a in zip(centres, yaws):
        G = np.eye(4)
        G[:3, :3] = PC.rot_y(a)
        G[:3, 3] = c
        out.append(G)
    return np.array(out)


def path(step=(0.6, -0.01, 0.3), yaw=0.012, n=N_IMAGES):
    return states([np.array(step) * k for k in range(n)], [yaw * k for k in range(n)])


def pixel(G, X, rng, noise):
    xc = G[:3, :3].T @ (np.asarray(X, dtype=np.float64) - G[:3, 3])
    u, v = F * xc[0] / xc[2] + CU, F * xc[1] / xc[2] + CV
    if noise:
        u, v = u + noise * rng.uniform(-1, 1), v + noise * rng.uniform(-1, 1)
    return np.float32(u), np.float32(v)


def in_camera(G, x):
    """a point given in a state's camera frame -> world"""
    return G[:3, :3] @ np.asarray(x, dtype=np.float64) + G[:3, 3]


class Builder:
    def __init__(self, fwd, seed, noise=0.0):
        self.fwd, self.rng, self.noise = fwd, np.random.default_rng(seed), noise
        self.offsets, self.uv, self.first = [0], [], []

    def span(self, length):
        a = int(self.rng.integers(0, N_IMAGES - length + 1))
        return a, length

    def add_point(self, X, a, length):
        """the track of world point X over images a .. a + length - 1"""
        self.add_pixels(a, [pixel(self.fwd[a + 1 + i], X, self.rng, self.noise) for i in range(length)])

    def add_pixels(self, a, px):
        assert 0 <= a and a + len(px) <= N_IMAGES
        self.uv += px
        self.first.append(a)
        self.offsets.append(len(self.uv))

    def family(self, **params):
        assert len(self.first) == N_TRACKS
        return Family(self.fwd, self.offsets, self.uv, self.first, params)


def road_point(rng, last, kind):
    """a point in the frame of the track's last camera: kind 0 on the road, 1 below it, 2 above it (an obstacle).  The height over
    the road, x2r.y, is about the third summand of y; the classes keep 0.2 m off the lines at 0.5 and -1."""
    z = rng.uniform(5, 18)
    x = rng.uniform(-0.3, 0.3) * z
    y = 1.6 - 0.08 * z + (rng.uniform(-0.8, 0.3), rng.uniform(0.7, 2.0), rng.uniform(-3.0, -1.2))[kind]
    return in_camera(last, (x, y, z))


def road_family(seed, noise):
    """track lengths 2 to 6 by points on the road, below and above it, in turn.  The path climbs 0.15 m per image, so the height
    over the road that pointType takes from the track's last camera is not the one its first camera would give."""
    b = Builder(path(step=(0.6, -0.15, 0.3)), seed, noise)
    for t in range(N_TRACKS):
        a, n = b.span(2 + t % 5)
        b.add_point(road_point(b.rng, b.fwd[a + n], (t // 5) % 3), a, n)
    return b.family()


def visibility_family(seed):
    """behind the cameras; less than a metre in front of the last camera; a little more than a metre in front of it; and regular
    points between them.  The path moves 0.3 m forward per image over the first three states and 0.3 m back per image after them,
    so the first camera of a track is further from the point than the last on some tracks and nearer on others: both halves of
    pointType's visibility test decide."""
    z = (0.0, 0.3, 0.6, 0.3, 0.0, -0.3)
    b = Builder(states([np.array((0.6 * k, -0.01 * k, z[k])) for k in range(N_IMAGES)], [0.012 * k for k in range(N_IMAGES)]), seed)
    for t in range(N_TRACKS):
        a, n = b.span(2 + t % 3)
        last, k = b.fwd[a + n], t % 4
        if k == 0:
            X = in_camera(last, (b.rng.uniform(-2, 2), b.rng.uniform(-1, 1), -b.rng.uniform(6, 12)))
        elif k == 1:
            X = in_camera(last, (b.rng.uniform(-0.2, 0.2), 0.1, b.rng.uniform(0.5, 0.97)))
        elif k == 2:
            X = in_camera(last, (b.rng.uniform(-0.2, 0.2), 0.1, b.rng.uniform(1.03, 1.5)))
        else:
            X = road_point(b.rng, last, 2)
        b.add_point(X, a, n)
    return b.family()


def far_family(seed):
    """points past max_dist; points at 18 to 29 m seen in two images, whose rays are nearly parallel; points at 6 to 14 m seen in
    two images, on both sides of min_angle; regular ones"""
    b = Builder(path(), seed)
    for t in range(N_TRACKS):
        k = t % 4
        a, n = b.span(2 + t % 5) if k in (0, 3) else b.span(2)
        last = b.fwd[a + n]
        if k == 0:
            z = b.rng.uniform(34, 60)
            X = in_camera(last, (b.rng.uniform(-0.3, 0.3) * z, 1.0 - 0.08 * z, z))
        elif k == 1:
            X = in_camera(last, (b.rng.uniform(-1, 1), -0.5, b.rng.uniform(18, 29)))
        elif k == 2:
            z = b.rng.uniform(6, 14)
            X = in_camera(last, (b.rng.uniform(-0.3, 0.3) * z, -0.5, z))
        else:
            X = road_point(b.rng, last, 0)
        b.add_point(X, a, n)
    return b.family()


def degenerate_states():
    """states 1 and 2 differ by a translation alone, states 2 and 3 by a rotation alone; then the regular path"""
    step = np.array((0.6, -0.01, 0.3))
    return states([step * 0, step * 1, step * 1, step * 2, step * 3, step * 4], [0.0, 0.0, 0.05, 0.06, 0.07, 0.08])


def degenerate_family(seed):
    """one pixel in images 0 and 1, whose states differ by a pure translation: parallel rays, a point at infinity; one pixel in
    images 1 and 2, whose states differ by a pure rotation: the rays meet in the camera centre, which is where initPoint puts the
    point (not visible); regular points over the whole sequence"""
    b = Builder(degenerate_states(), seed)
    for t in range(N_TRACKS):
        k = t % 3
        px = (np.float32(b.rng.uniform(100, 1100)), np.float32(b.rng.uniform(20, 360)))
        if k == 0:
            b.add_pixels(0, [px, px])
        elif k == 1:
            b.add_pixels(1, [px, px])
        else:
            a, n = b.span(2 + t % 5)
            b.add_point(road_point(b.rng, b.fwd[a + n], t % 3), a, n)
    return b.family()


def stray_family(seed):
    """tracks of 3 to 6 pixels with a gross outlier among the inner ones, 1500 to 5000 pixels off: the first estimate, from the
    first and the last pixel, is good and passes pointType, but Gauss-Newton with full steps then runs into a singular update,
    or goes on for all 22 updates without converging, or converges late.  Every fourth track has no outlier.  Where such an
    iteration ends can hang on the last bit of an iterate, and the reference's iterate is a float: the seed is one at which the
    reference's own stage does not move when the pixels move by one float32 ulp, in the eight patterns of nudged()
    (test_points_vs_ref.py asserts that)."""
    b = Builder(path(step=(0.5, 0.0, 0.1), yaw=0.0), seed)
    for t in range(N_TRACKS):
        a, n = b.span(3 + t % 4)
        X = in_camera(b.fwd[a + n], (b.rng.uniform(-1, 1), b.rng.uniform(-0.5, 0.5), b.rng.uniform(6, 10)))
        px = [pixel(b.fwd[a + 1 + i], X, b.rng, 0.0) for i in range(n)]
        if t % 4 != 3:
            k, m, ang = int(b.rng.integers(1, n - 1)), b.rng.uniform(1500, 5000), b.rng.uniform(0, 2 * math.pi)
            px[k] = (np.float32(px[k][0] + m * math.cos(ang)), np.float32(px[k][1] + m * math.sin(ang)))
        b.add_pixels(a, px)
    return b.family()


def nudged(fam, k):
    """the family with every pixel moved to the next float32 above it (k = 0), below it (k = 1), or above or below by a coin
    thrown per coordinate (k >= 2, which seeds the coin)"""
    if k < 2:
        to = np.float32(np.inf if k == 0 else -np.inf)
    else:
        to = np.where(np.random.default_rng(k).integers(0, 2, fam.uv.shape) == 1, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    return Family(fam.fwd, fam.offsets, np.nextafter(fam.uv, to), fam.first_image, fam.params, fam.inputs)


_families = None


def families():
    """{name: Family}.  The seeds are chosen so that the reference's own values keep clear of every threshold on all but at most
    1 % of a family's tracks (test_points_vs_ref.py asserts the share)."""
    global _families
    if _families is None:
        f = {}
        f["road"] = road_family(101, 0.0)
        f["noise_half_px"] = road_family(102, 0.5)
        f["visibility"] = visibility_family(103)
        f["far"] = far_family(104)
        f["degenerate"] = degenerate_family(105)
        # the first seed from 106 on that is stable in the sense of stray_family's text and has a track that converges with the
        # last of the 22 updates (track 220; test_points_vs_ref.py asserts both), so that a loop one update short would show
        f["stray"] = stray_family(112)
        f["road_type0"] = f["road"].variant("road", point_type=0)
        f["road_type2"] = f["road"].variant("road", point_type=2)
        f["noise_min_length3"] = f["noise_half_px"].variant("noise_half_px", min_track_length=3)
        f["far_min_angle3"] = f["far"].variant("far", min_angle=3.0)
        _families = f
    return _families


# ---- the comparison -----------------------------------------------------------------------------------------------------------

DEFAULTS = dict(point_type=1, min_track_length=2, max_dist=30.0, min_angle=2.0)


def _near(v, thr, bound):
    return np.abs(v - thr) <= bound * np.maximum(1.0, np.abs(v))


def near_threshold(ref, params, bound):
    """[T] bool: a value of the REFERENCE's lies within `bound` (relative to max(1, |value|), as the bound is measured) of the
    threshold it is compared with - the only tracks whose status and type may differ.  dist against max_dist and angle against
    min_angle where the reference got there; x1c.z and x2c.z against 1 and x2r.y against 0.5 and -1 where it reached pointType.
    |w| against 1e-10: the class does not keep w, but V's last column is a unit vector, so |w| = 1 / sqrt(1 + |xyz0|^2) of the
    point initPoint returned; it is compared relative to 1e-10.  Where initPoint returned false there is no value and the track
    is never left out."""
    p = dict(DEFAULTS)
    p.update(params)
    stage = ref.stage
    typed = (stage != 3) & (stage != 4)
    probe = ref.probe.astype(np.float64)
    near = typed & (_near(probe[:, 0], 1.0, bound) | _near(probe[:, 1], 1.0, bound) | _near(probe[:, 2], 0.5, bound) | _near(probe[:, 2], -1.0, bound))
    w = 1.0 / np.sqrt(1.0 + (ref.xyz0.astype(np.float64) ** 2).sum(axis=1))
    near |= typed & (np.abs(w - 1e-10) <= bound * 1e-10)
    near |= np.isin(stage, (0, 8, 9)) & _near(ref.dist, p["max_dist"], bound)
    near |= np.isin(stage, (0, 9)) & _near(ref.angle, p["min_angle"], bound)
    return near


def differences(got, ref):
    """[T, 5] |ours - reference| / max(1, |reference|) of xyz, dist and angle"""
    a = np.column_stack([got.xyz, got.dist, got.angle])
    b = np.column_stack([ref.xyz.astype(np.float64), ref.dist, ref.angle])
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def measure(got, ref, params):
    """the largest difference over the tracks both sides keep, 0 without any"""
    kept = (ref.stage == 0) & (got.status == 0)
    return float(differences(got, ref)[kept].max()) if kept.any() else 0.0


def stages_of(got, fam):
    """Our statuses in the driver's numbering.  The class has one outcome for a refinement that did not converge, refinePoint
    returning false; the driver tells the two apart by one more updatePoint at the point refinePoint left: it fails (6) where the
    loop stopped on a failed update, which leaves the point alone - but also where the loop used its 22 updates and the 23rd would
    have failed.  So a status 7 of ours becomes 6 where one more update (points_ref.update_point) at our point fails; then both
    sides say the same thing with the same number."""
    st = got.status.copy()
    idx = np.nonzero(st == 7)[0]
    if len(idx):
        frames = [R.frame_matrices([float(x) for x in po], F, CU, CV) for po in fam.poses]
        fr = fam.obs_frames
        for t in idx:
            a, b = int(fam.offsets[t]), int(fam.offsets[t + 1])
            if R.update_point([frames[k][1] for k in fr[a:b]], [(R.f32(u), R.f32(v)) for u, v in fam.uv[a:b]], [float(x) for x in got.xyz[t]]) == "failed":
                st[t] = 6
    return st


def compare(got, ref, fam, what, bound=None):
    """ours (a Points object or points_ref's) on the family fam against the reference's record of the same tracks: status (see
    stages_of) and type equal on every track that is not near a threshold; xyz, dist and angle of the kept ones within the bound;
    `updates` only as far as both converged, which the status says (0, 8 and 9 are the converged ones): a float iterate may take
    an update more or fewer.  Returns the share of tracks left out."""
    bound = BOUND if bound is None else bound
    params = fam.params
    near = near_threshold(ref, params, bound)
    firm = ~near
    status = stages_of(got, fam)
    bad = np.nonzero(firm & ((status != ref.stage) | (got.type != ref.type)))[0]
    assert len(bad) == 0, (what, "status / type", bad[:10].tolist(), got.status[bad[:10]].tolist(), ref.stage[bad[:10]].tolist(), got.type[bad[:10]].tolist(),
                           ref.type[bad[:10]].tolist())
    conv = firm & np.isin(ref.stage, (0, 8, 9))
    assert ((got.updates[conv] >= 1) & (got.updates[conv] <= 22)).all(), (what, "updates")
    kept = firm & (ref.stage == 0)
    d = differences(got, ref)[kept]
    assert np.isfinite(d).all() and (len(d) == 0 or d.max() <= bound), (what, "xyz / dist / angle", float(d.max()), bound)
    return float(near.mean()) if len(near) else 0.0


# ---- sequences for update() and for the linking --------------------------------------------------------------------------------

class Sequence:
    """match lists of the consecutive image pairs (k - 1, k), the Tr of every update, and what the generator knows: tracks[i] =
    (first image, [feature index in every image it is seen in])"""

    def __init__(self, lists, Tr, tracks, params):
        self.lists, self.Tr, self.tracks, self.params = lists, Tr, tracks, dict(params)


def sequence(seed, n_points, noise=0.0, params=None, shared_i1p=False):
    """points on a path, each seen over a span of 2 to 6 images, so that tracks end at every update from the second on.  Feature
    indices are a random permutation per image and a list is in random order, so that every i1p and every i1c occurs once per
    list.  The pixels follow the convention of the module text; Tr of update k is state k's inverse times state k - 1.
    shared_i1p: one more match in the list of images (2, 3) whose i1p another match of that list has."""
    vm = PC.pkg("visomatch")
    rng = np.random.default_rng(seed)
    G = path()
    spans, feats = [], []
    perm = [rng.permutation(n_points + 1) for _ in range(N_IMAGES)]
    for i in range(n_points):
        n = 2 + i % 5
        a = int(rng.integers(0, N_IMAGES - n + 1))
        spans.append((a, n))
        feats.append([int(perm[a + j][i]) for j in range(n)])
    X = []
    for i, (a, n) in enumerate(spans):  # road, below, above; every fourth point 18 to 60 m away: too far, or under a small angle
        if i % 4 == 3:
            z = rng.uniform(18, 60)
            X.append(in_camera(G[a + n], (rng.uniform(-1, 1), 1.0 - 0.08 * z, z)))
        else:
            X.append(road_point(rng, G[a + n], i % 3))
    lists = []
    for k in range(1, N_IMAGES):
        rows = [i for i, (a, n) in enumerate(spans) if a < k < a + n]
        rows = [rows[j] for j in rng.permutation(len(rows))]
        m = np.zeros(len(rows), dtype=vm.P_MATCH)
        for j, i in enumerate(rows):
            a = spans[i][0]
            m[j]["i1p"], m[j]["i1c"], m[j]["i2p"], m[j]["i2c"] = feats[i][k - 1 - a], feats[i][k - a], -1, -1
            m[j]["u1p"], m[j]["v1p"] = pixel(G[k], X[i], rng, 0.0)
            m[j]["u1c"], m[j]["v1c"] = pixel(G[k + 1], X[i], rng, 0.0)
        lists.append(m)
    if noise:
        # a feature has one pixel per image: the end of one match is the start of the next
        jitter = {}
        for k, m in enumerate(lists):
            for r in m:
                for img, e in ((k, "p"), (k + 1, "c")):
                    key = (img, int(r["i1" + e]))
                    if key not in jitter:
                        jitter[key] = (np.float32(r["u1" + e] + noise * rng.uniform(-1, 1)), np.float32(r["v1" + e] + noise * rng.uniform(-1, 1)))
                    r["u1" + e], r["v1" + e] = jitter[key]
    if shared_i1p:
        m = lists[2]
        extra = m[:1].copy()
        extra["i1c"] = int(perm[3][n_points])  # an index no other match has
        extra["u1c"] += 3.0
        lists[2] = np.concatenate([m, extra])
    Tr = [np.eye(4)] + [np.linalg.inv(G[k]) @ G[k - 1] for k in range(2, N_IMAGES + 1)]  # the last one is the flush update's
    return Sequence(lists, Tr, [(a, f) for (a, n), f in zip(spans, feats)], params or {})


def sequences():
    return {"plain": sequence(201, 60), "noise_min_length3": sequence(202, 45, noise=0.5, params=dict(min_track_length=3)),
            "type0_angle3": sequence(203, 50, params=dict(point_type=0, min_angle=3.0))}


def finished(seq, records):
    """From the reference's live tracks after every update (records: what ref_recon_sequence returned) and the lists: per update
    k = 1 .. the tracks it finished, [(pixels, last_idx)] in the order of the class's list.  A live track is finished by the next
    update unless a match of that update's list starts at its last_idx (every i1p occurs once there)."""
    out = [[]]
    for k in range(1, len(records)):
        starts = set(seq.lists[k]["i1p"].tolist()) if k < len(seq.lists) else set()
        out.append([(int(n), int(last)) for n, last in records[k - 1]["live"] if int(last) not in starts])
    return out


def chain(seq, r, last_idx, n):
    """the n pixels of the track that ends in feature last_idx of image r, as update() collected them: u1p / v1p of its first
    match, then u1c / v1c of every match (every i1c occurs once per list)"""
    px, idx = [], last_idx
    for k in range(r - 1, r - n, -1):
        m = seq.lists[k]
        j = int(np.nonzero(m["i1c"] == idx)[0][0])
        px.append((m[j]["u1c"], m[j]["v1c"]))
        idx = int(m[j]["i1p"])
        if k == r - n + 1:
            px.append((m[j]["u1p"], m[j]["v1p"]))
    return px[::-1]


# ---- the fixture: the inputs above and what the reference made of them ----------------------------------------------------------

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reconstruction_ref.npz")
PARAM_KEYS = ("point_type", "min_track_length", "max_dist", "min_angle")
INPUT_FIELDS = ("fwd", "offsets", "uv", "first_image")
REF_FIELDS = (("stage", np.int8), ("type", np.int8), ("xyz", np.float32), ("xyz0", np.float32), ("probe", np.float32), ("dist", np.float64),
              ("angle", np.float64))
SHARED = "shared_i1p"


class Recorded:
    """the reference's outputs for a family, as oracle.bindings.ReconTracks has them"""


def all_sequences():
    s = sequences()
    s[SHARED] = sequence(204, 40, shared_i1p=True)
    return s


def record(B):
    """{key: array}: everything the fixture holds, from a fresh run of the compiled reference (B: oracle.bindings)"""
    out = {"families": np.array(list(families()))}
    for name, fam in families().items():
        if fam.inputs is None:
            for k in INPUT_FIELDS:
                out[name + "_" + k] = getattr(fam, k)
        out[name + "_inputs"] = np.array(fam.inputs or name)
        p = dict(DEFAULTS)
        p.update(fam.params)
        out[name + "_params"] = np.array([p[k] for k in PARAM_KEYS], dtype=np.float64)
        ref = fam.reference(B)
        for k, dt in REF_FIELDS:
            out[name + "_" + k] = getattr(ref, k).astype(dt)
    seqs = all_sequences()
    out["sequences"] = np.array(list(seqs))
    for name, seq in seqs.items():
        out[name + "_matches"] = np.concatenate(seq.lists)
        out[name + "_counts"] = np.array([len(m) for m in seq.lists], dtype=np.int32)
        recs = B.ref_recon_sequence(F, CU, CV, seq.lists, seq.Tr, **seq.params)
        out[name + "_finished"] = np.array([(r, n, last) for r, fin in enumerate(finished(seq, recs)) for n, last in fin], dtype=np.int32).reshape(-1, 3)
    a, feats = next((a, f) for a, f in seqs[SHARED].tracks if a <= 2 < a + len(f) - 1 and f[2 - a] == int(seqs[SHARED].lists[2][-1]["i1p"]))
    out[SHARED + "_track"] = np.array([a] + feats, dtype=np.int32)  # the track whose i1p the added match shares: first image, features
    return out


class Fixture:
    """families: {name: Family}; refs: {name: Recorded}; lists: {sequence: [P_MATCH arrays]}; finished: {sequence: int32 [n, 3]
    rows (update - 1 = the image the track ends in, pixels, last_idx)}; shared_track: see record()"""


def load():
    z = np.load(FIXTURE)
    fx = Fixture()
    fx.families, fx.refs, fx.lists, fx.finished = {}, {}, {}, {}
    for name in z["families"].tolist():
        src = str(z[name + "_inputs"])
        p = dict(zip(PARAM_KEYS, z[name + "_params"].tolist()))
        p["point_type"], p["min_track_length"] = int(p["point_type"]), int(p["min_track_length"])
        fx.families[name] = Family(*[z[src + "_" + k] for k in INPUT_FIELDS], params=p, inputs=None if src == name else src)
        r = Recorded()
        for k, _ in REF_FIELDS:
            setattr(r, k, z[name + "_" + k])
        r.stage, r.type = r.stage.astype(np.int32), r.type.astype(np.int32)
        fx.refs[name] = r
    for name in z["sequences"].tolist():
        fx.lists[name] = np.split(z[name + "_matches"], np.cumsum(z[name + "_counts"])[:-1])
        fx.finished[name] = z[name + "_finished"]
    fx.shared_track = z[SHARED + "_track"]
    return fx


def prefix_ref(ref, n):
    r = Recorded()
    for k, _ in REF_FIELDS:
        setattr(r, k, getattr(ref, k)[:n])
    return r


def linking(tr, skip=()):
    """a Tracks object as sorted rows (last frame, pixels, last feature) - what `finished` says of the reference's tracks;
    skip: tracks to leave out"""
    rows = []
    for t in range(len(tr)):
        if t not in skip:
            o = tr.track(t)
            rows.append((int(o[-1, 0]), len(o), int(o[-1, 1])))
    return sorted(rows)


PAIRS = [(k, k + 1) for k in range(N_IMAGES - 1)]
