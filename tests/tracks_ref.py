"""The definition of multi-view feature tracks (include/visomatch.h, vsm_tracks_run), restated for the tests: dictionaries,
Python sorts, nothing from the library.  Nodes are (frame, feature index) named by at least one match; match m of pair
k = (a, b) joins (a, ip) and (b, ic); a track is a connected component."""
import numpy as np

P_MATCH = np.dtype(
    [("u1p", "<f4"), ("v1p", "<f4"), ("i1p", "<i4"), ("u2p", "<f4"), ("v2p", "<f4"), ("i2p", "<i4"),
     ("u1c", "<f4"), ("v1c", "<f4"), ("i1c", "<i4"), ("u2c", "<f4"), ("v2c", "<f4"), ("i2c", "<i4")])


def make_list(ip, ic, side=0):
    """a match list whose chosen side links ip[m] -> ic[m]; the other side's indices are -7 (never to be read), the
    coordinates tell the match's number"""
    ip, ic = np.asarray(ip, dtype=np.int32).reshape(-1), np.asarray(ic, dtype=np.int32).reshape(-1)
    a = np.zeros(len(ip), dtype=P_MATCH)
    for n in ("i1p", "i2p", "i1c", "i2c"):
        a[n] = -7
    a["i2p" if side else "i1p"] = ip
    a["i2c" if side else "i1c"] = ic
    a["u1p"] = np.arange(len(ip))
    return a


class Ref:
    pass


def tracks(n_frames, pairs, lists, side=0, min_length=2):
    """-> object with offsets [T+1] int32, obs [n_obs,4] int32, flags [T] uint8, of_pairs: list of int32 arrays, sets: the
    tracks as a set of frozensets of nodes (for order-independence checks)"""
    fp, fc = ("i2p", "i2c") if side else ("i1p", "i1c")
    parent, first = {}, {}

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for k, ((a, b), lst) in enumerate(zip(pairs, lists)):
        ips, ics = lst[fp].tolist(), lst[fc].tolist()
        for m, (ip, ic) in enumerate(zip(ips, ics)):
            for end, node in enumerate(((int(a), ip), (int(b), ic))):
                if node not in parent:
                    parent[node] = node
                    first[node] = (k, m, end)  # pairs and matches are visited in ascending order: the first one stays
            ra, rb = find((int(a), ip)), find((int(b), ic))
            if ra != rb:
                parent[ra] = rb
    groups = {}
    for node in parent:
        groups.setdefault(find(node), []).append(node)
    kept = sorted((sorted(g) for g in groups.values() if len(g) >= min_length), key=lambda g: g[0])
    number = {}
    offsets, obs, flags = [0], [], []
    for t, g in enumerate(kept):
        frames = [f for f, _ in g]
        flags.append(1 if len(set(frames)) < len(frames) else 0)
        for node in g:
            number[node] = t
            k, m, end = first[node]
            obs.append((node[0], node[1], k, 2 * m + end))
        offsets.append(len(obs))
    r = Ref()
    r.offsets = np.array(offsets, dtype=np.int32)
    r.obs = np.array(obs, dtype=np.int32).reshape(-1, 4)
    r.flags = np.array(flags, dtype=np.uint8)
    r.of_pairs = [np.array([number.get((int(a), ip), -1) for ip in lst[fp].tolist()], dtype=np.int32) for (a, b), lst in zip(pairs, lists)]
    r.sets = {frozenset(g) for g in kept}
    return r


def assert_same(got, want, what=""):
    """a library result (offsets, obs, flags, of_pair) against a reference or another library result: bytes equal"""
    assert got.offsets.dtype == np.int32 and got.obs.dtype == np.int32 and got.flags.dtype == np.uint8, what
    assert got.offsets.tobytes() == np.ascontiguousarray(want.offsets).tobytes(), (what, "offsets", got.offsets[:8], want.offsets[:8])
    assert got.obs.shape == want.obs.shape and got.obs.tobytes() == np.ascontiguousarray(want.obs).tobytes(), (what, "obs")
    assert got.flags.tobytes() == want.flags.tobytes(), (what, "flags")
    wp = want.of_pairs if hasattr(want, "of_pairs") else want._of_pairs
    gp = got.of_pairs if hasattr(got, "of_pairs") else got._of_pairs
    assert len(gp) == len(wp), what
    for k, (g, w) in enumerate(zip(gp, wp)):
        assert g.dtype == np.int32 and g.tobytes() == w.tobytes(), (what, "track_of_match", k)


# ---- the hand-built families both suites run: name -> (n_frames, pairs, lists, side, min_length) ----
def families():
    L = make_list
    out = {}
    out["chain3"] = (3, [(0, 1), (1, 2)], [L([0, 1, 2], [5, 6, 7]), L([5, 6, 9], [1, 0, 3])], 0, 2)
    # two chains (frames 0-1-2 and 4-5) merged by the loop-closure pair (5, 0)
    out["loop_closure"] = (6, [(0, 1), (1, 2), (4, 5), (5, 0)], [L([3, 4], [3, 4]), L([3, 4], [8, 9]), L([1, 2], [6, 7]), L([6], [3])], 0, 2)
    out["both_directions"] = (2, [(0, 1), (1, 0)], [L([0, 1, 2], [2, 1, 0]), L([2, 1, 5], [0, 1, 4])], 0, 2)
    out["repeated_pair"] = (2, [(0, 1), (0, 1), (0, 1)], [L([0, 1], [0, 1]), L([0, 1], [0, 1]), L([1, 2], [1, 3])], 0, 2)
    out["duplicate_edges"] = (2, [(0, 1)], [L([4, 4, 4, 2], [1, 1, 1, 0])], 0, 2)
    # a self pair: (2, 0)-(2, 1) share frame 2; the self-edge 5 -> 5 is a track of one observation
    out["self_pair_min2"] = (3, [(2, 2), (1, 2)], [L([0, 5], [1, 5]), L([0], [0])], 0, 2)
    out["self_pair_min1"] = (3, [(2, 2), (1, 2)], [L([0, 5], [1, 5]), L([0], [0])], 0, 1)
    out["empty_among_full"] = (4, [(0, 1), (1, 2), (2, 3), (3, 0)], [L([], []), L([1, 2], [2, 1]), L([], []), L([0], [7])], 0, 2)
    out["all_empty"] = (3, [(0, 1), (1, 2)], [L([], []), L([], [])], 0, 2)
    out["no_pairs"] = (3, np.zeros((0, 2), np.int32), [], 0, 2)
    out["side1"] = (3, [(0, 1), (1, 2)], [L([0, 1, 2], [5, 6, 7], side=1), L([5, 6, 9], [1, 0, 3], side=1)], 1, 2)
    out["min_length3"] = (3, [(0, 1), (1, 2)], [L([0, 1, 2], [5, 6, 7]), L([5, 6, 9], [1, 0, 3])], 0, 3)
    # mismatches merge two points: frame 1 is seen twice
    out["merged_points"] = (3, [(0, 1), (1, 2), (0, 2)], [L([0, 1], [0, 1]), L([0, 1], [0, 1]), L([0], [1])], 0, 2)
    return out
