"""The definition of the fusion (include/visomatch.h, vsm_fuse_run; csrc/vsm_fuse.h), restated for the tests in plain Python
ints and floats: nothing vectorised, no index - every track against every frame against every feature.  Nothing comes from the
library.  The state is the resection's (tests/resect_ref.py), the projection the re-observation restatement's."""
import numpy as np

import reobserve_ref as RR
import resect_ref as R

DEFAULTS = dict(radius=4.0, min_depth=1e-10, max_cost=0, ratio_num=0, ratio_den=0)
FIELDS = ("prop", "uv", "partner", "fused_into", "offsets_after", "obs_src", "frame_counts")
FUSED, EMPTY, COSTLY, AMBIGUOUS, CONFLICT, OUTBID, ONE_SIDED = range(7)
N_STATS = 13


class Ref:
    pass


def fuse(poses, f, cu, cv, width, height, offsets, obs_frames, obs_feat, xyz, feat_offsets, feat, use=None, ref_obs=None, search=None, pose_valid=None, params=None):
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
    in_use = [(use is None or bool(use[t])) and offsets[t + 1] > offsets[t] for t in range(T)]
    frames_of = [obs_frames[offsets[t]:offsets[t + 1]] for t in range(T)]
    owner = {}
    for t in range(T):
        if in_use[t]:
            for i in range(offsets[t], offsets[t + 1]):
                key = (obs_frames[i], obs_feat[i])
                owner[key] = min(owner.get(key, t), t)
    desc = {}

    def desc_of(g, k):
        if (g, k) not in desc:
            desc[(g, k)] = RR.descriptor(rec[fo[g] + k])
        return desc[(g, k)]

    stats = [0] * N_STATS
    frame_counts = np.zeros((F, 2), np.int32)
    prop, uv = [], []
    for a in range(T):
        if not in_use[a]:
            continue
        o, n = offsets[a], offsets[a + 1] - offsets[a]
        ref = o + (int(ref_obs[a]) if ref_obs is not None else (n - 1) // 2)
        ref_rec = rec[fo[obs_frames[ref]] + obs_feat[ref]]
        cls, da = ref_rec[3], RR.descriptor(ref_rec)
        for g in range(F):
            if not (search is None or bool(search[g])):
                stats[RR.NOT_SEARCHED] += 1
                continue
            if not (pose_valid is None or bool(pose_valid[g])):
                stats[RR.NO_POSE] += 1
                continue
            if g in frames_of[a]:
                stats[RR.OBSERVED] += 1
                continue
            p = RR.project(states[g], pts[a], f, cu, cv, prm["min_depth"], width, height)
            if p in (RR.BEHIND, RR.OUTSIDE):
                stats[p] += 1
                continue
            pu, pv = p
            frame_counts[g][0] += 1
            costs = []
            for k in range(fo[g + 1] - fo[g]):
                u, v, _, c = rec[fo[g] + k][:4]
                if (g, k) in owner and c == cls and float(u) - pu <= radius and pu - float(u) <= radius and float(v) - pv <= radius and pv - float(v) <= radius:
                    costs.append((RR.sad(da, desc_of(g, k)), k))
            costs.sort()
            if not costs:
                stats[5 + EMPTY] += 1
                continue
            best, k = costs[0]
            second = costs[1][0] if len(costs) > 1 else -1
            b = owner[(g, k)]
            if prm["max_cost"] > 0 and best > prm["max_cost"]:
                code = COSTLY
            elif prm["ratio_den"] > 0 and second >= 0 and not best * prm["ratio_den"] < second * prm["ratio_num"]:
                code = AMBIGUOUS
            elif set(frames_of[a]) & set(frames_of[b]):
                code = CONFLICT
            else:
                code = FUSED
            frame_counts[g][1] += 1
            prop.append([a, g, k, best, second, len(costs), code, b])
            uv.append((pu, pv))
    # every track's choice among its proposals that came this far: the smallest (cost, proposal index)
    choice = {}
    for i, row in enumerate(prop):
        if row[6] == FUSED:
            choice[row[0]] = min(choice.get(row[0], (1 << 62, 0)), (row[3], i))
    partner = np.full(T, -1, np.int32)
    for a, (_, i) in choice.items():
        partner[a] = prop[i][7]
    for i, row in enumerate(prop):
        if row[6] == FUSED:
            if choice[row[0]][1] != i:
                row[6] = OUTBID
            elif partner[row[7]] != row[0]:
                row[6] = ONE_SIDED
        stats[5 + row[6]] += 1
    fused_into = np.full(T, -1, np.int32)
    for a in range(T):
        b = int(partner[a])
        if b >= 0 and partner[b] == a and a < b:
            fused_into[b] = a
            stats[12] += 1
    # the merged set
    absorbed_by = {int(s): t for t, s in enumerate(fused_into) if s >= 0}
    offsets_after, obs_src = [0], []
    for t in range(T):
        mine = []
        if fused_into[t] < 0:
            mine = list(range(offsets[t], offsets[t + 1]))
            if t in absorbed_by:
                b = absorbed_by[t]
                mine += list(range(offsets[b], offsets[b + 1]))
                mine = [i for _, _, i in sorted((obs_frames[i], pos, i) for pos, i in enumerate(mine))]
        obs_src += mine
        offsets_after.append(len(obs_src))
    r = Ref()
    r.prop = np.array(prop, np.int32).reshape(-1, 8)
    r.uv = np.array(uv, np.float64).reshape(-1, 2)
    r.partner, r.fused_into, r.frame_counts, r.stats = partner, fused_into, frame_counts, stats
    r.offsets_after, r.obs_src = np.array(offsets_after if T else [0], np.int32), np.array(obs_src, np.int32)
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


def assert_stats(got, want, what=""):
    import importlib
    names = importlib.import_module("conftest").pkg("visomatch").FUSE_STATS
    assert [got.stats[k] for k in names] == list(want.stats), (what, got.stats, want.stats)
