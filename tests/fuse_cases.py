"""Inputs for the fusion tests, without images.  cases() returns {name: Case}; reference(name) the restatement's result
(tests/fuse_ref.py) and host(name) the host view's, each computed once per process and shared by the CPU and the GPU suite.

Three families.  SPLIT scenes: a planted scene of tests/reobserve_cases.py in which every track observes every frame that sees
its point - a feature with the point's descriptor at the rounded projection, distractors, shuffled records -, and then every
track of two or more observations cut at a frame into fragments, each a track of its own with the true point.  The first
fragments keep the indices 0..T-1, the second follow as T..2T-1 (the third as 2T..3T-1): a call that fuses every pair leaves
the unsplit scene in the first T tracks and empties the rest (Case.unsplit).  Two views of a point differ by at most 64, two
random descriptors by some 2700, so which fragments choose each other is certain.
CARPETED scenes: a built scene of the re-observation's tests, and one more track, behind every camera, that observes every
free feature of the frames behind frame 0.  The fusion's windows are then the re-observation's, feature for feature.
BUILT scenes: identity poses with f = 1, cu = cv = 0, where the point (pu, pv, 1) projects to (pu, pv) in every frame, and
tracks whose observations are set one by one: owners, ties, chains of choices, conflicts, long and interleaved fragments,
every reason and code in one call.  The sizes are the smallest at which a 16-lane group per track or proposal, sixteen groups
per workgroup and a scan of 256 items per workgroup can go wrong."""
import numpy as np

import fuse_ref as FR
import reobserve_cases as RC

TRACK_COUNTS = (0, 1, 15, 16, 17, 255, 256, 257)
FRAME_COUNTS = (1, 2, 9, 15, 16, 17, 33)
WINDOW_SIZES = (0, 1, 2, 15, 16, 17, 33)
PROPOSAL_COUNTS = (255, 256, 257)
FRAGMENTS = ((1, 1), (2, 2), (16, 17), (17, 16), (33, 1), (1, 33), (257, 257))
Case, byte_desc = RC.Case, RC.byte_desc


# ---- split scenes -----------------------------------------------------------------------------------------------------------

def split(n_frames, n_points, seed, ways=2, n_tracks=None, interleave=False, exact=False, **kw):
    """the planted scene (every track in every frame that sees it), cut into `ways` fragments per track; n_tracks: only the
    first n_tracks fragments are kept.  exact: the views of the first two fragments carry one descriptor and those of the
    third differ from it by 1 in one byte, so that the first two choose each other whatever the third does."""
    base = RC.planted(n_frames, n_points, seed, observe_all=range(2 * n_points + 8), **kw)
    rng = np.random.default_rng(seed + 1)
    T = len(base.offsets) - 1
    frag = [[] for _ in range(ways)]
    feat = base.feat.copy()
    for t in range(T):
        obs = [(int(g), int(k)) for g, k in zip(base.obs_frames[base.offsets[t]:base.offsets[t + 1]], base.obs_feat[base.offsets[t]:base.offsets[t + 1]])]
        n = len(obs)
        if interleave:
            parts = [obs[w::ways] for w in range(ways)]
        else:
            cuts = sorted(rng.choice(np.arange(1, n), size=min(ways - 1, n - 1), replace=False).tolist()) if n > 1 else []
            parts = [obs[a:b] for a, b in zip([0] + cuts, cuts + [n])] + [[]] * (ways - 1 - len(cuts))
        for w in range(ways):
            frag[w].append(parts[w])
            if exact and parts[w]:
                first = feat[base.feat_offsets[obs[0][0]] + obs[0][1], 4:].copy()
                first[0] ^= 1 if w == 2 else 0
                for g, k in parts[w]:
                    feat[base.feat_offsets[g] + k, 4:] = first
    tracks = [p for w in range(ways) for p in frag[w]]
    keep = len(tracks) if n_tracks is None else n_tracks
    assert keep <= len(tracks)
    use = None if base.use is None else np.tile(base.use[:T], ways)[:keep]
    feats = [[(int(r[0]), int(r[1]), int(r[3]), np.asarray(r[4:], dtype="<i4").view(np.uint8).tolist()) for r in feat[base.feat_offsets[g]:base.feat_offsets[g + 1]]]
             for g in range(n_frames)]
    c = Case(base.poses, base.width, base.height, feats, tracks[:keep], np.tile(base.xyz, (ways, 1))[:keep], use=use, search=base.search, pose_valid=base.pose_valid,
             params=base.params, f=base.f, cu=base.cu, cv=base.cv)
    c.unsplit, c.ways, c.n_points = base, ways, T
    return c


# ---- carpeted scenes ----------------------------------------------------------------------------------------------------------

def carpeted(c, keep=lambda g, k: True):
    """one more track, behind every camera, that observes every free feature (g, k) of the frames g >= 1 with keep(g, k)"""
    taken = set(zip(c.obs_frames.tolist(), c.obs_feat.tolist()))
    more = [(g, k) for g in range(1, len(c.poses)) for k in range(int(c.feat_offsets[g + 1] - c.feat_offsets[g])) if (g, k) not in taken and keep(g, k)]
    assert more
    out = Case.__new__(Case)
    out.__dict__.update(c.__dict__)
    T = len(c.offsets) - 1
    out.offsets = np.append(c.offsets, c.offsets[-1] + len(more)).astype(np.int32)
    out.obs_frames = np.append(c.obs_frames, [g for g, _ in more]).astype(np.int32)
    out.obs_feat = np.append(c.obs_feat, [k for _, k in more]).astype(np.int32)
    out.xyz = np.vstack([c.xyz[:T], [[0.0, 0.0, -1.0]]])
    out.use = None if c.use is None else np.append(c.use[:T], 1).astype(np.uint8)
    out.ref_obs = None
    out.plain, out.carpet = c, T
    return out


# ---- built scenes: f = 1, cu = cv = 0, identity poses ------------------------------------------------------------------------

class Scene:
    def __init__(self, n_frames, width, height, seed=0):
        self.n, self.width, self.height = n_frames, width, height
        self.feats = [[] for _ in range(n_frames)]
        self.tracks, self.xyz, self.use = [], [], []
        self.rng = np.random.default_rng(seed)

    def feature(self, g, u, v, cls=0, desc=None):
        self.feats[g].append((u, v, cls, self.rng.integers(0, 256, 32).tolist() if desc is None else desc))
        return len(self.feats[g]) - 1

    def track(self, obs, pu, pv, use=1, X=None):
        """a track with the observations obs [(frame, feature)] whose point projects to (pu, pv) in every frame"""
        self.tracks.append(list(obs))
        self.xyz.append([pu, pv, 1.0] if X is None else X)
        self.use.append(use)
        return len(self.tracks) - 1

    def seen(self, frames, pu, pv, cls=0, desc=None, use=1, X=None):
        """a track that observes, in each of `frames`, a new feature at (pu, pv) with one descriptor"""
        desc = self.rng.integers(0, 256, 32).tolist() if desc is None else desc
        return self.track([(g, self.feature(g, int(pu), int(pv), cls, desc)) for g in frames], float(pu), float(pv), use=use, X=X)

    def case(self, **kw):
        return Case([RC.IDENTITY] * self.n, self.width, self.height, self.feats, self.tracks, self.xyz, use=self.use, **kw)


def windows_case():
    """track i's window in frame 1 holds WINDOW_SIZES[i] owned features of its class 1; beside them a free feature with the
    track's own bytes (cost 0, would win) and, from the second on, an owned feature of each other class with the track's bytes"""
    s = Scene(2, 400, 60, seed=1)
    owned = []
    for i, n in enumerate(WINDOW_SIZES):
        pu, pv = 20 + 40 * i, 30
        d = s.rng.integers(0, 256, 32).tolist()
        s.seen([0], pu, pv, cls=1, desc=d)
        for j in range(n):
            owned.append((1, s.feature(1, pu - 3 + j % 7, pv - 3 + j // 7, 1)))
        s.feature(1, pu + 1, pv + 4, 1, desc=d)  # free
        if i:
            for c in (0, 2, 3):
                owned.append((1, s.feature(1, pu + c - 1, pv + 4, c, desc=d)))
    s.track(owned, 0, 0, X=[0.0, 0.0, -1.0])
    return s.case()


def proposals_case(n):
    """n tracks with one proposal each: points on a grid 10 pixels apart seen in frame 0, and in frame 1 a feature at each that
    one track behind the camera owns"""
    s = Scene(2, 310, 100, seed=2)
    owned = []
    for i in range(n):
        pu, pv = 5 + 10 * (i % 30), 5 + 10 * (i // 30)
        s.seen([0], pu, pv)
        owned.append((1, s.feature(1, pu, pv)))
    s.track(owned, 0, 0, X=[0.0, 0.0, -1.0])
    return s.case()


def fragments_case():
    """pairs of fragments of FRAGMENTS observations in 514 frames, the first from frame 0 on, the second from frame 257 on;
    then interleaved pairs: even against odd frames, the smaller index holding the odd ones in the second"""
    s = Scene(514, 200, 40, seed=3)
    pairs = []
    for i, (na, nb) in enumerate(FRAGMENTS):
        d = s.rng.integers(0, 256, 32).tolist()
        pairs.append((s.seen(range(na), 10 + 20 * i, 10, desc=d), s.seen(range(257, 257 + nb), 10 + 20 * i, 10, desc=d)))
    d = s.rng.integers(0, 256, 32).tolist()
    pairs.append((s.seen(range(0, 17, 2), 10, 30, desc=d), s.seen(range(1, 17, 2), 10, 30, desc=d)))
    pairs.append((s.seen(range(1, 33, 2), 40, 30, desc=d), s.seen(range(0, 33, 2), 40, 30, desc=d)))
    c = s.case()
    c.pairs = pairs
    return c


def conflicts_case():
    """pairs of tracks at one pixel with one descriptor that share exactly one frame: the first, a middle or the last of the
    first track's list, and of the second's; the lists are not sorted"""
    s = Scene(12, 300, 20, seed=4)
    pairs = []
    for i, (pa, pb) in enumerate(((0, 1), (2, 0), (4, 2), (1, 4), (3, 3), (0, 0), (4, 4))):
        d = s.rng.integers(0, 256, 32).tolist()
        fa, fb = [3, 1, 4, 0, 2], [8, 6, 9, 5, 7]
        fb[pb] = fa[pa]
        pairs.append((s.seen(fa, 10 + 20 * i, 10, desc=d), s.seen(fb, 10 + 20 * i, 10, desc=d)))
    c = s.case()
    c.pairs = pairs
    return c


def twice_case():
    """tracks that see a frame twice: a survivor with frames [1, 1, 2] takes [3]; a survivor with [4, 1] takes [3, 3]; and a
    pair whose only common frame is one that the first sees twice"""
    s = Scene(6, 100, 20, seed=5)
    d = [s.rng.integers(0, 256, 32).tolist() for _ in range(3)]
    k = [s.feature(1, 10, 10, 0, d[0]), s.feature(1, 11, 10, 0, d[0]), s.feature(2, 10, 10, 0, d[0])]
    s.track([(1, k[0]), (1, k[1]), (2, k[2])], 10.0, 10.0)
    s.seen([3], 10, 10, desc=d[0])
    s.seen([4, 1], 40, 10, desc=d[1])
    k = [s.feature(3, 40, 10, 0, d[1]), s.feature(3, 41, 10, 0, d[1])]
    s.track([(3, k[0]), (3, k[1])], 40.0, 10.0)
    k = [s.feature(2, 70, 10, 0, d[2]), s.feature(2, 71, 10, 0, d[2]), s.feature(0, 70, 10, 0, d[2])]
    s.track([(2, k[0]), (2, k[1]), (0, k[2])], 70.0, 10.0)
    s.seen([2, 5], 70, 10, desc=d[2])
    return s.case()


def owners_case():
    """a feature named by two tracks in use belongs to the smaller index; one named by a track not in use and by one in use
    belongs to the latter; one named only by a track not in use belongs to nobody: the window there is empty"""
    s = Scene(3, 200, 20, seed=6)
    z = byte_desc(0)
    s.seen([0], 10, 10, desc=z)                    # 0: searches frame 1 at (10, 10)
    s.seen([0], 50, 10, desc=z)                    # 1: at (50, 10)
    s.seen([0], 90, 10, desc=z)                    # 2: at (90, 10): only an unused track's feature there
    x = s.feature(1, 10, 10, 0, byte_desc(3))
    y = s.feature(1, 50, 10, 0, byte_desc(4))
    w = s.feature(1, 90, 10, 0, byte_desc(5))
    s.track([(1, x)], 150.0, 5.0)                  # 3
    s.track([(1, y)], 150.0, 5.0, use=0)           # 4
    s.track([(1, x)], 150.0, 5.0)                  # 5: names x too
    s.track([(1, y)], 150.0, 5.0)                  # 6: names y beside the unused track
    s.track([(1, w)], 150.0, 5.0, use=0)           # 7
    return s.case(search=[0, 1, 1])


def ties_case():
    """equal costs inside a window: the lowest feature index wins and second equals best; equal costs of a track's two
    proposals: the lower proposal index is its choice, the other is outbid"""
    s = Scene(3, 100, 40, seed=7)
    z = byte_desc(0)
    s.seen([0], 20, 20, desc=z)
    k = [s.feature(1, 22, 20, 0, byte_desc(9)), s.feature(1, 18, 21, 0, byte_desc(7)), s.feature(1, 21, 19, 0, byte_desc(7)), s.feature(1, 20, 20, 0, byte_desc(7))]
    s.track([(1, k[0]), (1, k[1])], 0, 0, X=[0.0, 0.0, -1.0])
    s.track([(1, k[2]), (1, k[3])], 0, 0, X=[0.0, 0.0, -1.0])
    s.seen([0], 60, 20, desc=z)
    s.seen([1], 60, 20, desc=byte_desc(5))
    s.seen([2], 60, 20, desc=byte_desc(5))
    return s.case()


def chain_case():
    """three tracks at one pixel in three frames with descriptors 0, 10 and 14 apart: 0 chooses 1, 1 chooses 2, 2 chooses 1"""
    s = Scene(3, 40, 40, seed=8)
    for g, first in enumerate((0, 10, 14)):
        s.seen([g], 20, 20, desc=byte_desc(first))
    return s.case()


def limits_case():
    """max_cost = 40 and ratio 1 / 2 on owned features: best 40 passes the cap, 41 does not; best 10 against second 21 passes the
    ratio, against 20 it does not; a single feature has no second and passes"""
    s = Scene(2, 300, 40, seed=9)
    owned = []
    for i, (best, second) in enumerate(((40, 255), (41, 255), (10, 21), (10, 20), (0, None), (0, 0), (40, 80), (40, 81))):
        u = 20 + 30 * i
        s.seen([0], u, 20, desc=byte_desc(0))
        owned.append((1, s.feature(1, u, 20, 0, byte_desc(best))))
        if second is not None:
            owned.append((1, s.feature(1, u + 2, 21, 0, byte_desc(second))))
    s.track(owned, 0, 0, X=[0.0, 0.0, -1.0])
    return s.case(params=dict(max_cost=40, ratio_num=1, ratio_den=2))


LIMITS_CODES = [6, 2, 6, 3, 6, 3, 3, 6]


def everything_case():
    """every reason and every code in one call of six frames: frame 4 is not searched, frame 5 has no valid pose.  Tracks: 0 and
    1 fuse; 2 finds empty windows; 3 and 4 are over the cap; 5 is ambiguous between the two features of 6; 7 and 8 share frame
    2; 9, 10, 11 are the chain; 12 behind; 13 outside; 14 not in use; 15 without an observation"""
    s = Scene(6, 200, 40, seed=10)
    z = byte_desc(0)
    s.seen([0], 10, 10, desc=z)
    s.seen([1], 10, 10, desc=byte_desc(1))
    s.seen([0], 30, 30, cls=3)
    s.seen([0], 50, 10, desc=z)
    s.seen([1], 50, 10, desc=byte_desc(200))
    s.seen([0], 70, 10, desc=z)
    k = [s.feature(1, 70, 10, 0, byte_desc(10)), s.feature(1, 71, 10, 0, byte_desc(12))]
    s.track([(1, k[0]), (1, k[1])], 70.0, 10.0)
    s.seen([0, 2], 90, 10, desc=z)
    s.seen([1, 2], 90, 10, desc=z)
    for g, first in enumerate((20, 30, 34)):
        s.seen([g], 110, 10, desc=byte_desc(first))
    s.seen([0], 130, 10, X=[1.0, 1.0, -2.0])
    s.seen([0], 150, 10, X=[500.0, 10.0, 1.0])
    s.seen([1], 10, 10, desc=z, use=0)
    c = s.case(search=[1, 1, 1, 1, 0, 1], pose_valid=[1, 1, 1, 1, 1, 0], params=dict(max_cost=100, ratio_num=1, ratio_den=2))
    c.offsets = np.append(c.offsets, c.offsets[-1]).astype(np.int32)
    c.xyz = np.vstack([c.xyz, [[10.0, 10.0, 1.0]]])
    c.use = np.append(c.use, 1).astype(np.uint8)
    return c


def masks_case():
    """search, use and pose_valid masks over a split scene of six frames"""
    return split(6, 30, seed=70, search=[1, 0, 1, 1, 0, 1], pose_valid=[1, 1, 0, 1, 1, 1], use=[i % 4 != 1 for i in range(30)])


_cases = None
_refs, _hosts = {}, {}


def cases():
    global _cases
    if _cases is not None:
        return _cases
    c = {}
    for n in TRACK_COUNTS:
        c["tracks_%d" % n] = split(4, (n + 1) // 2, seed=100 + n, n_tracks=n, distractors=30)
    for n in FRAME_COUNTS:
        c["frames_%d" % n] = split(n, 12, seed=200 + n, distractors=20)
    c["split_8"] = split(8, 40, seed=300)
    c["split_interleaved"] = split(9, 25, seed=301, interleave=True)
    c["split_radius_1"] = split(5, 40, seed=302, params=dict(radius=1.0))
    c["three_ways"] = split(9, 24, seed=303, ways=3, exact=True)
    c["three_ways_interleaved"] = split(9, 24, seed=304, ways=3, exact=True, interleave=True)
    c["masks"] = masks_case()
    c["windows"] = windows_case()
    for n in PROPOSAL_COUNTS:
        c["proposals_%d" % n] = proposals_case(n)
    c["fragments"] = fragments_case()
    c["conflicts"] = conflicts_case()
    c["twice"] = twice_case()
    c["owners"] = owners_case()
    c["ties"] = ties_case()
    c["chain"] = chain_case()
    c["limits"] = limits_case()
    c["everything"] = everything_case()
    c["carpet_sweep_4"] = carpeted(RC.sweep_case(4.0))
    c["carpet_sweep_2_5"] = carpeted(RC.sweep_case(2.5))
    c["carpet_sweep_2_5_half"] = carpeted(RC.sweep_case(2.5, shift=0.5))
    c["carpet_sweep_0"] = carpeted(RC.sweep_case(0.0))
    c["carpet_edges"] = carpeted(RC.edges_case())
    c["carpet_half_windows"] = carpeted(RC.windows_case(), keep=lambda g, k: k % 2 == 0)
    c["no_frames"] = Case(np.zeros((0, 12)), 10, 10, [], [], np.zeros((0, 3)))
    _cases = c
    return c


def reference(name):
    if name not in _refs:
        a, kw = cases()[name].args()
        _refs[name] = FR.fuse(*a, **kw)
    return _refs[name]


def host(name):
    from conftest import pkg
    if name not in _hosts:
        a, kw = cases()[name].args()
        _hosts[name] = pkg("visomatch").host_fuse(*a, **kw)
    return _hosts[name]


def pixels(c):
    """the float pixel of every observation: its feature's"""
    return c.feat[c.feat_offsets[c.obs_frames] + c.obs_feat, :2].astype(np.float32) if len(c.obs_frames) else np.zeros((0, 2), np.float32)
