"""The definition of the re-observation (include/visomatch.h, vsm_reobserve_run; csrc/vsm_reobserve.h), restated for the tests
in plain Python ints and floats: one operation per expression step, nothing vectorised, no index - every candidate looks at
every feature of its frame.  Nothing comes from the library.  The state is the resection's (tests/resect_ref.py)."""
import numpy as np

import resect_ref as R

DEFAULTS = dict(radius=4.0, min_depth=1e-10, max_cost=0, ratio_num=0, ratio_den=0)
FIELDS = ("cand", "uv", "track_accepted", "frame_counts")
NOT_SEARCHED, NO_POSE, OBSERVED, BEHIND, OUTSIDE = range(5)
ACCEPTED, EMPTY, COSTLY, AMBIGUOUS, LOST = range(5)


def project(S, X, f, cu, cv, min_depth, width, height):
    """-> BEHIND, OUTSIDE or the pair (pu, pv)"""
    xc = X[0] * S[0] + X[1] * S[1] + X[2] * S[2] + S[3]
    yc = X[0] * S[4] + X[1] * S[5] + X[2] * S[6] + S[7]
    zc = X[0] * S[8] + X[1] * S[9] + X[2] * S[10] + S[11]
    if not zc > min_depth:
        return BEHIND
    pu = f * xc / zc + cu
    pv = f * yc / zc + cv
    if not (pu >= 0.0 and pu <= float(width - 1) and pv >= 0.0 and pv <= float(height - 1)):
        return OUTSIDE
    return pu, pv


def descriptor(rec):
    """the 32 bytes of a record's words 4..11, lowest byte of a word first"""
    return [((int(w) & 0xffffffff) >> s) & 255 for w in rec[4:12] for s in (0, 8, 16, 24)]


def sad(a, b):
    return sum(abs(x - y) for x, y in zip(a, b))


class Ref:
    pass


def reobserve(poses, f, cu, cv, width, height, offsets, obs_frames, obs_feat, xyz, feat_offsets, feat, use=None, ref_obs=None, search=None, pose_valid=None,
              params=None):
    prm = dict(DEFAULTS)
    prm.update(params or {})
    radius = float(prm["radius"])
    poses = np.asarray(poses, dtype=np.float64).reshape(len(poses), -1)[:, :12] if len(poses) else np.zeros((0, 12))
    states = [R.rigid_inverse([float(x) for x in p]) for p in poses]
    pts = [[float(x) for x in p] for p in np.asarray(xyz, dtype=np.float64).reshape(-1, 3)]
    f, cu, cv = float(f), float(cu), float(cv)
    F, T = len(poses), len(offsets) - 1 if len(offsets) else 0
    offsets, obs_frames, obs_feat = [int(x) for x in offsets], [int(x) for x in obs_frames], [int(x) for x in obs_feat]
    fo = [int(x) for x in feat_offsets] if F else [0]
    rec = [[int(x) for x in r] for r in np.asarray(feat, dtype=np.int32).reshape(-1, 12)]
    occupied = set((g, k) for g, k in zip(obs_frames, obs_feat))
    # per frame and class the free features (k, u, v), in index order; descriptors as they are needed
    free = [[[] for _ in range(4)] for _ in range(F)]
    for g in range(F):
        for k in range(fo[g + 1] - fo[g]):
            r = rec[fo[g] + k]
            if (g, k) not in occupied:
                free[g][r[3]].append((k, r[0], r[1]))
    desc = {}

    def desc_of(g, k):
        if (g, k) not in desc:
            desc[(g, k)] = descriptor(rec[fo[g] + k])
        return desc[(g, k)]

    stats = [0] * 10
    cand, uv = [], []
    claim = {}
    for t in range(T):
        o, n = offsets[t], offsets[t + 1] - offsets[t]
        if not ((use is None or bool(use[t])) and n > 0):
            continue
        ref = o + (int(ref_obs[t]) if ref_obs is not None else (n - 1) // 2)
        ref_rec = rec[fo[obs_frames[ref]] + obs_feat[ref]]
        cls, a = ref_rec[3], descriptor(ref_rec)
        frames = set(obs_frames[o:o + n])
        for g in range(F):
            if not (search is None or bool(search[g])):
                stats[NOT_SEARCHED] += 1
                continue
            if not (pose_valid is None or bool(pose_valid[g])):
                stats[NO_POSE] += 1
                continue
            if g in frames:
                stats[OBSERVED] += 1
                continue
            p = project(states[g], pts[t], f, cu, cv, prm["min_depth"], width, height)
            if p in (BEHIND, OUTSIDE):
                stats[p] += 1
                continue
            pu, pv = p
            costs = []  # (cost, k) of the window
            for k, u, v in free[g][cls]:
                if float(u) - pu <= radius and pu - float(u) <= radius and float(v) - pv <= radius and pv - float(v) <= radius:
                    costs.append((sad(a, desc_of(g, k)), k))
            costs.sort()
            if not costs:
                row = [t, g, -1, -1, -1, 0, EMPTY]
            else:
                best, k = costs[0]
                second = costs[1][0] if len(costs) > 1 else -1
                if prm["max_cost"] > 0 and best > prm["max_cost"]:
                    code = COSTLY
                elif prm["ratio_den"] > 0 and second >= 0 and not best * prm["ratio_den"] < second * prm["ratio_num"]:
                    code = AMBIGUOUS
                else:
                    code = ACCEPTED
                    claim[(g, k)] = min(claim.get((g, k), (1 << 62, 0)), (best, len(cand)))
                row = [t, g, k, best, second, len(costs), code]
            cand.append(row)
            uv.append((pu, pv))
    track_accepted = np.zeros(T, np.int32)
    frame_counts = np.zeros((F, 2), np.int32)
    for i, row in enumerate(cand):
        if row[6] == ACCEPTED and claim[(row[1], row[2])][1] != i:
            row[6] = LOST
        if row[6] == ACCEPTED:
            track_accepted[row[0]] += 1
            frame_counts[row[1]][1] += 1
        frame_counts[row[1]][0] += 1
        stats[5 + row[6]] += 1
    r = Ref()
    r.cand = np.array(cand, np.int32).reshape(-1, 7)
    r.uv = np.array(uv, np.float64).reshape(-1, 2)
    r.track_accepted, r.frame_counts, r.stats = track_accepted, frame_counts, stats
    return r


def assert_same(got, want, what=""):
    """every int, and every double by its bytes"""
    for name in FIELDS:
        a, b = np.ascontiguousarray(getattr(got, name)), np.ascontiguousarray(getattr(want, name))
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.nonzero((a.reshape(len(a), -1).view(np.uint8) != b.reshape(len(b), -1).view(np.uint8)).any(axis=1))[0]
            g = int(bad[0])
            raise AssertionError((what, name, "entries", bad[:10].tolist(), "first", g, a[g].tolist(), b[g].tolist()))
