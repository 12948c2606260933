"""GPU suite (run with -m gpu on an MI355X): Matcher.tracks / Matcher.pair_tracks (vsm_tracks_run, vsm_pairs_tracks) - multi-view
feature tracks as the connected components of the match graph, on the device.  Every result is compared, tobytes() equal,
with tests/tracks_ref.py (the definition restated in Python) and with vsm_host_tracks (the sequential host view).  Sizes are
the smallest at which each piece of the device path can go wrong."""
import numpy as np
import pytest

import content as CT
import tracks_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vm():
    m = pkg("visomatch")
    m.lib()  # raises if the HIP library is missing: no silent fallback
    return m


@pytest.fixture(scope="module")
def matcher(vm):
    m = vm.Matcher()
    yield m
    m.close()


def check(vm, m, n_frames, pairs, lists, side=0, min_length=2, what=""):
    """the device result against the reference and the host view; returns (device result, reference)"""
    got = m.tracks(n_frames, pairs, lists, side, min_length)
    want = R.tracks(n_frames, pairs, lists, side, min_length)
    R.assert_same(got, want, (what, "device against the reference"))
    R.assert_same(vm.host_tracks(n_frames, pairs, lists, side, min_length), got, (what, "host view against the device"))
    s = got.stats
    assert s["tracks"] == len(want.flags) and s["inconsistent"] == int(want.flags.sum()) and s["edges"] == sum(len(x) for x in lists), (what, s)
    assert s["by_wave"] + s["by_workgroup"] + s["by_host"] == s["tracks"], (what, s)
    return got, want


# ---- 1: the hand-built families of the CPU suite -------------------------------------------------------------------------

FAMILIES = R.families()


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_hand_built(vm, matcher, name):
    n_frames, pairs, lists, side, min_length = FAMILIES[name]
    got, want = check(vm, matcher, n_frames, pairs, lists, side, min_length, name)
    if name in ("all_empty", "no_pairs"):
        assert len(got) == 0 and got.offsets.tolist() == [0]
    else:
        assert len(got) >= 1


# ---- 2: segment-length classes: a wave, a workgroup, the host ------------------------------------------------------------------

def test_segment_length_classes(vm, matcher):
    WM, BM = vm.TRACKS_WAVE_MAX, vm.TRACKS_BLOCK_MAX
    lengths = [1, 2, WM - 1, WM, WM + 1, BM - 1, BM, BM + 1]
    n_frames = BM + 1
    # paths: class j is feature j of frames 0 .. length - 1; pair (f - 1, f) carries a match j -> j of every class that reaches f
    pairs = [(f - 1, f) for f in range(1, n_frames)]
    lists = []
    for f in range(1, n_frames):
        js = [j for j, n in enumerate(lengths) if n > f]
        lists.append(R.make_list(js, js))
    # ... the class of length 1 is a self-edge of a self pair; so is the star of length 1
    pairs.append((0, 0))
    lists.append(R.make_list([0, 200], [0, 200]))
    # stars inside frames 0 and 1: the centre in frame 0, length - 1 leaves in frame 1 (two observations in frame 1 from length 3 on)
    ip, ic = [], []
    for j, n in enumerate(lengths):
        ip += [100 + j] * (n - 1)
        ic += [1000 + 3000 * j + i for i in range(n - 1)]
    pairs.append((0, 1))
    lists.append(R.make_list(ip, ic))
    order = np.random.default_rng(2).permutation(len(pairs))  # (pairs in no particular order)
    pairs, lists = [pairs[i] for i in order], [lists[i] for i in order]
    got, want = check(vm, matcher, n_frames, pairs, lists, 0, 1, "length classes")
    seg = np.diff(got.offsets)
    assert sorted(seg.tolist()) == sorted(lengths * 2)
    assert sorted(seg[got.flags == 1].tolist()) == [n for n in lengths if n >= 3]  # the stars; every path is consistent
    s = got.stats
    print("segments by path", s)
    assert (s["by_wave"], s["by_workgroup"], s["by_host"]) == (8, 6, 2), s
    # min_length drops the short ones and renumbers the rest
    got3, _ = check(vm, matcher, n_frames, pairs, lists, 0, 3, "length classes, min_length 3")
    assert sorted(np.diff(got3.offsets).tolist()) == sorted([n for n in lengths if n >= 3] * 2)
    assert sum((t == -1).sum() for t in got3._of_pairs) == 2 + 2  # the self-edges and the edges of the two tracks of length 2


# ---- 3: the scan's workgroup boundaries ------------------------------------------------------------------------------------------

def test_scan_boundaries(vm, matcher):
    first, _ = check(vm, matcher, *FAMILIES["chain3"][:3])
    B = first.stats["scan_block"]
    assert B == 256
    for N in (B - 1, B, B + 1, B * B - 1, B * B, B * B + 1):
        # one frame of N features, a self pair: v -> v + 1 for every third v, so every third node is a kept root
        v = np.arange(0, N - 1, 3)
        ip, ic = v.tolist(), (v + 1).tolist()
        if (N - 1) % 3 != 1:  # no edge names the last node: a self-edge makes the node space N (its track of one is dropped)
            ip.append(N - 1)
            ic.append(N - 1)
        got, want = check(vm, matcher, 1, [(0, 0)], [R.make_list(ip, ic)], 0, 2, ("scan", N))
        assert got.stats["nodes"] == N and len(got) == len(v) and got.offsets.tolist() == list(range(0, 2 * len(v) + 1, 2))
        assert got.obs[:, 1].tolist() == np.stack([v, v + 1], 1).reshape(-1).tolist()


# ---- 4: the order of the unions -----------------------------------------------------------------------------------------------------

def three_orders(n):
    return [np.arange(n), np.arange(n)[::-1], np.random.default_rng(17).permutation(n)]


def same_partition(results, what):
    base = results[0]
    for r in results[1:]:
        assert r.offsets.tobytes() == base.offsets.tobytes() and r.flags.tobytes() == base.flags.tobytes(), what
        assert np.ascontiguousarray(r.obs[:, :2]).tobytes() == np.ascontiguousarray(base.obs[:, :2]).tobytes(), what


def test_union_order_path_across_frames(vm, matcher):
    """one path of 20 000 nodes, a node per frame: 19 999 pairs of one match each (more pairs than a workgroup keeps in LDS),
    the pairs in ascending, descending and random order: a deep tree whatever the order"""
    n = 20000
    results = []
    for order in three_orders(n - 1):
        pairs = [(int(f), int(f) + 1) for f in order]
        lists = [R.make_list([0], [0])] * (n - 1)
        got, _ = check(vm, matcher, n, pairs, lists, 0, 2, "path")
        assert len(got) == 1 and got.offsets.tolist() == [0, n] and got.flags.tolist() == [0] and got.stats["by_host"] == 1
        assert got.obs[:, 0].tolist() == list(range(n))
        results.append(got)
    same_partition(results, "path")


def graph_in_one_list(vm, matcher, ip, ic, what):
    """a graph over the features of one frame (a self pair), its edges in three orders: identical tracks"""
    ip, ic = np.asarray(ip), np.asarray(ic)
    results = []
    for order in three_orders(len(ip)):
        got, _ = check(vm, matcher, 1, [(0, 0)], [R.make_list(ip[order], ic[order])], 0, 2, what)
        results.append(got)
    same_partition(results, what)
    return results[0]


def test_union_order_comb(vm, matcher):
    """a spine of every eighth node and a tooth of seven nodes below each: one component, every root contended"""
    n = 20000
    spine = np.arange(0, n - 8, 8)
    ip, ic = [spine], [spine + 8]
    for k in range(1, 8):
        ip.append(spine + k)
        ic.append(spine + k - 1)
    got = graph_in_one_list(vm, matcher, np.concatenate(ip), np.concatenate(ic), "comb")
    assert len(got) == 1 and got.offsets[1] == len(spine) * 8 + 1


def random_graph():
    rng = np.random.default_rng(23)
    return rng.integers(0, 20000, 30000), rng.integers(0, 20000, 30000)


def test_union_order_random_graph(vm, matcher):
    ip, ic = random_graph()
    got = graph_in_one_list(vm, matcher, ip, ic, "random graph")
    assert len(got) > 20 and np.diff(got.offsets).max() > vm.TRACKS_BLOCK_MAX  # the giant component and many small ones


# ---- 5: determinism ------------------------------------------------------------------------------------------------------------------

def test_determinism(vm, matcher):
    ip, ic = random_graph()
    args = (3, [(0, 1), (1, 2), (2, 0)], [R.make_list(ip[:10000], ic[:10000]), R.make_list(ip[10000:20000], ic[10000:20000]), R.make_list(ip[20000:], ic[20000:])])
    a, _ = check(vm, matcher, *args, what="first call")
    b = matcher.tracks(*args)
    other = vm.Matcher()
    c = other.tracks(*args)
    other.close()
    R.assert_same(b, a, "the same call again")
    R.assert_same(c, a, "a second handle")
    assert len(a) > 100


# ---- 6: from images -------------------------------------------------------------------------------------------------------------------

W, H, N = 417, 163, 7
IMAGE_PAIRS = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (0, 2), (6, 0), (2, 2)]


@pytest.fixture(scope="module")
def frames(synth):
    """test_pairs_gpu.py's case-1 frames, stacked: ([N,H,W] left, [N,H,W] right)"""
    return CT.stack(synth.stereo_sequence(31, W, H, N, disparity=10, ramp=(1, 12)))


@pytest.mark.parametrize("method,side", [(0, 0), (2, 0), (2, 1)])
def test_from_images(vm, frames, method, side):
    """match_pairs(fetch=False) then pair_tracks().  With the oracle's lists of these pairs (computed on the CPU) the reference
    gives 1079 / 910 / 911 tracks for the three cases, 879 / 774 / 774 of them with four observations or more, the longest with
    8 / 8 / 7, and 1 / 2 / 1 inconsistent ones (the self pair's matches are all i -> i; mismatches merge points)."""
    left, right = frames
    m = vm.Matcher()
    assert m.push_back(left[1], right[1]) == 0 and m.push_back(left[4], right[4]) == 0 and m.match(method)
    ring = m.get_matches()
    assert len(ring) >= 700
    assert m.match_pairs(left, right, IMAGE_PAIRS, method, fetch=False) is None
    got = m.pair_tracks(side=side)
    lists = [m.pair_matches(k) for k in range(len(IMAGE_PAIRS))]
    assert min(len(x) for x in lists) >= 745  # (the oracle's shortest of these lists: quad matching, pair (5, 6))
    want = R.tracks(N, IMAGE_PAIRS, lists, side, 2)
    print("tracks", len(want.flags), "longest", int(np.diff(want.offsets).max()), "inconsistent", int(want.flags.sum()), got.stats, got.timings)
    assert len(want.flags) >= 750 and np.diff(want.offsets).max() >= 4
    R.assert_same(got, want, "pair_tracks against the reference")
    R.assert_same(vm.host_tracks(N, IMAGE_PAIRS, lists, side, 2), got, "host view")
    R.assert_same(m.tracks(N, IMAGE_PAIRS, lists, side, 2), got, "vsm_tracks_run on the fetched lists")
    assert got.flags.any()  # (the oracle's lists give at least one inconsistent track in each case)
    # an observation leads to its pixel: the match it names has that feature index at that end
    for frame, feature, pair, code in got.obs[:: max(1, len(got.obs) // 50)].tolist():
        mt = lists[pair][code >> 1]
        assert IMAGE_PAIRS[pair][code & 1] == frame and mt[("i2" if side else "i1") + "pc"[code & 1]] == feature
    # nothing else of the handle has moved
    again = [m.pair_matches(k) for k in range(len(IMAGE_PAIRS))]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, lists))
    assert m.get_matches().tobytes() == ring.tobytes()
    t = got.timings
    assert t["pack_us"] > 0 and t["kernels_us"] > 0
    m.close()


# ---- 7: error codes ---------------------------------------------------------------------------------------------------------------------

def test_error_codes(vm, frames):
    left, right = frames
    m = vm.Matcher()
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):
        m.pair_tracks()
    m.match_pairs(left[:3], right[:3], [(-1, 1), (0, 2)], 1, fetch=False)
    assert len(m.pair_matches(0)) >= 750
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        m.pair_tracks()
    m.match_pairs(left[:3], right[:3], [(0, 1), (1, 2)], 0, fetch=False)
    good = m.pair_tracks()
    assert len(good) >= 500
    for kw in ({"side": 2}, {"min_length": 0}, {"side": 1}):  # (flow lists carry no right-image indices: -1, negative)
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            m.pair_tracks(**kw)
        R.assert_same(m._tracks_result(0, "the last result", 2), good, ("the last good result", kw))
    m.close()


def test_bad_arguments_keep_the_last_result(vm, matcher):
    n_frames, pairs, lists, side, min_length = FAMILIES["loop_closure"]
    good, _ = check(vm, matcher, n_frames, pairs, lists, side, min_length)
    L = R.make_list
    for bad in ((2, [(0, 2)], [L([0], [0])], 0, 2), (2, [(-1, 1)], [L([0], [0])], 0, 2), (2, [(0, 1)], [L([0], [-1])], 0, 2),
                (2, [(0, 1)], [L([0], [0])], 1, 2), (2, [(0, 1)], [L([0], [0])], 0, 0), (3, [(0, 1), (1, 2)], [L([0], [2 ** 30]), L([1], [2 ** 30])], 0, 2)):
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            matcher.tracks(*bad)
        R.assert_same(matcher._tracks_result(0, "the last result", len(pairs)), good, "the last good result")
