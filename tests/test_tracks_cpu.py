"""CPU suite: vsm_host_tracks (the sequential host view of multi-view feature tracks) against tests/tracks_ref.py, the
definition restated with dictionaries and Python sorts.  Every comparison is tobytes() equality."""
import os
import subprocess

import numpy as np
import pytest

import tracks_ref as R
from conftest import ROOT, pkg


@pytest.fixture(scope="module")
def vm():
    m = pkg("visomatch")
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "opencl-structure-from-motion_amd", "csrc")])
    m.lib()
    return m


FAMILIES = R.families()


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_hand_built(vm, name):
    n_frames, pairs, lists, side, min_length = FAMILIES[name]
    want = R.tracks(n_frames, pairs, lists, side, min_length)
    got = vm.host_tracks(n_frames, pairs, lists, side, min_length)
    R.assert_same(got, want, name)
    assert [got.track(t).tolist() for t in range(len(got))] == [want.obs[want.offsets[t]:want.offsets[t + 1]].tolist() for t in range(len(want.flags))]


def test_hand_built_expectations():
    """the reference itself, against results written down by hand: the families test what they say they test"""
    r = R.tracks(*FAMILIES["chain3"])
    assert r.offsets.tolist() == [0, 3, 6, 8, 10]
    assert r.obs.tolist() == [[0, 0, 0, 0], [1, 5, 0, 1], [2, 1, 1, 1], [0, 1, 0, 2], [1, 6, 0, 3], [2, 0, 1, 3], [0, 2, 0, 4], [1, 7, 0, 5], [1, 9, 1, 4], [2, 3, 1, 5]]
    assert r.flags.tolist() == [0, 0, 0, 0] and [x.tolist() for x in r.of_pairs] == [[0, 1, 2], [0, 1, 3]]
    assert R.tracks(*FAMILIES["min_length3"]).of_pairs[1].tolist() == [0, 1, -1]
    r = R.tracks(*FAMILIES["loop_closure"])
    assert [len(s) for s in sorted(r.sets, key=min)] == [5, 3, 2] and r.flags.tolist() == [0, 0, 0]
    assert sorted(r.sets, key=min)[0] == {(0, 3), (1, 3), (2, 8), (4, 1), (5, 6)}
    r2, r1 = R.tracks(*FAMILIES["self_pair_min2"]), R.tracks(*FAMILIES["self_pair_min1"])
    assert r2.flags.tolist() == [1] and r2.obs.tolist() == [[1, 0, 1, 0], [2, 0, 0, 0], [2, 1, 0, 1]] and r2.of_pairs[0].tolist() == [0, -1]
    assert r1.flags.tolist() == [1, 0] and r1.obs[3].tolist() == [2, 5, 0, 2] and r1.of_pairs[0].tolist() == [0, 1]
    assert len(R.tracks(*FAMILIES["all_empty"]).flags) == 0 and R.tracks(*FAMILIES["all_empty"]).offsets.tolist() == [0]
    assert R.tracks(*FAMILIES["merged_points"]).flags.tolist() == [1]
    assert R.tracks(*FAMILIES["duplicate_edges"]).obs.tolist() == [[0, 2, 0, 6], [1, 0, 0, 7], [0, 4, 0, 0], [1, 1, 0, 1]]


def test_sizes_only_call(vm):
    """null outputs: the sizes"""
    import ctypes as C
    n_frames, pairs, lists, side, min_length = FAMILIES["chain3"]
    pa, ls, ptrs, cnt = vm._track_inputs(pairs, lists)
    n_obs = C.c_int32(-1)
    T = vm.lib().vsm_host_tracks(n_frames, pa.ctypes.data_as(C.c_void_p), len(pa), ptrs, cnt.ctypes.data_as(C.c_void_p), side, min_length,
                                 None, None, None, None, C.byref(n_obs))
    assert (T, n_obs.value) == (4, 10)


def bad_inputs():
    """every VSM_EARG case of the contract: name -> (n_frames, pairs, lists, side, min_length, counts or None)"""
    L = R.make_list
    ok = [L([0, 1], [1, 0])]
    return {
        "side 2": (2, [(0, 1)], ok, 2, 2, None),
        "side -1": (2, [(0, 1)], ok, -1, 2, None),
        "min_length 0": (2, [(0, 1)], ok, 0, 0, None),
        "current frame outside": (2, [(0, 2)], ok, 0, 2, None),
        "previous frame outside": (2, [(2, 0)], ok, 0, 2, None),
        "previous frame -1 (a stereo-only list)": (2, [(-1, 1)], ok, 0, 2, None),
        "negative previous index": (2, [(0, 1)], [L([0, -1], [1, 0])], 0, 2, None),
        "negative current index": (2, [(0, 1)], [L([0, 1], [-3, 0])], 0, 2, None),
        "the other side's indices (-7) chosen": (2, [(0, 1)], ok, 1, 2, None),
        "null list, positive count": (2, [(0, 1), (1, 0)], [ok[0], None], 0, 2, [2, 5]),
        "negative count": (2, [(0, 1)], ok, 0, 2, [-1]),
        "node ids beyond 31 bits": (3, [(0, 1), (1, 2)], [L([0], [2 ** 30]), L([1], [2 ** 30])], 0, 2, None),
        "an index of 2^31 - 1": (2, [(0, 1)], [L([2 ** 31 - 1], [0])], 0, 2, None),
    }


BAD = bad_inputs()


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_arguments_leave_the_outputs_untouched(vm, name):
    import ctypes as C
    n_frames, pairs, lists, side, min_length, counts = BAD[name]
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        vm.host_tracks(n_frames, pairs, lists, side, min_length, counts=counts)
    # ... and with output arrays: they keep what they held
    pa, ls, ptrs, cnt = vm._track_inputs(pairs, lists)
    if counts is not None:
        cnt = np.ascontiguousarray(counts, dtype=np.int32)
    outs = [np.full(64, 0x5A5A5A5A, np.int32) for _ in range(3)] + [np.full(64, 0x5A, np.uint8)]
    n_obs = C.c_int32(-77)
    rc = vm.lib().vsm_host_tracks(n_frames, pa.ctypes.data_as(C.c_void_p), len(pa), ptrs, cnt.ctypes.data_as(C.c_void_p), side, min_length,
                                  outs[0].ctypes.data_as(C.c_void_p), outs[1].ctypes.data_as(C.c_void_p), outs[3].ctypes.data_as(C.c_void_p),
                                  outs[2].ctypes.data_as(C.c_void_p), C.byref(n_obs))
    assert rc == vm.Matcher.EARG and n_obs.value == -77
    assert all((o == 0x5A5A5A5A).all() for o in outs[:3]) and (outs[3] == 0x5A).all()


def consecutive_lists(seed, n_frames, n_feat, keep):
    """match lists of pairs (f-1, f): a random injective partial map from frame f-1's features to frame f's, so that tracks
    are paths (consistent)"""
    rng = np.random.default_rng(seed)
    pairs, lists = [], []
    for f in range(1, n_frames):
        n = int(n_feat * keep)
        ip = rng.permutation(n_feat)[:n]
        ic = rng.permutation(n_feat)[:n]
        pairs.append((f - 1, f))
        lists.append(R.make_list(ip, ic))
    return pairs, lists


def test_plot_track_rule(vm):
    """matlab/plotTrack.m: for consecutive pairs with consistent tracks, walking i1p back from a match of the last list visits
    exactly the observations of that match's track from that frame backwards"""
    n_frames = 9
    pairs, lists = consecutive_lists(5, n_frames, 60, 0.7)
    got = vm.host_tracks(n_frames, pairs, lists)
    R.assert_same(got, R.tracks(n_frames, pairs, lists))
    assert not got.flags.any() and len(got) > 40
    longest = 0
    for m in range(len(lists[-1])):
        walk, f, idx = [(n_frames - 1, int(lists[-1]["i1c"][m]))], n_frames - 1, int(lists[-1]["i1p"][m])
        while True:  # frame f's match has previous index idx in frame f - 1: look for the match of list f - 2 whose i1c is idx
            walk.append((f - 1, idx))
            f -= 1
            if f == 0:
                break
            hit = np.nonzero(lists[f - 1]["i1c"] == idx)[0]
            if len(hit) == 0:
                break
            idx = int(lists[f - 1]["i1p"][hit[0]])
        t = got.of_pair(len(pairs) - 1)[m]
        assert t >= 0
        rows = got.track(t)
        assert rows[-1, 0] == n_frames - 1  # the track ends in the last frame: from there backwards is all of it
        assert [tuple(r) for r in rows[:, :2].tolist()] == sorted(walk)
        longest = max(longest, len(walk))
    assert longest >= 4


def test_pair_order_independence(vm):
    rng = np.random.default_rng(11)
    n_frames = 7
    pairs, lists = consecutive_lists(3, n_frames, 40, 0.8)
    pairs += [(0, 3), (6, 1), (2, 2)]
    lists += [R.make_list(rng.integers(0, 40, 15), rng.integers(0, 40, 15)) for _ in range(3)]
    base = vm.host_tracks(n_frames, pairs, lists)
    R.assert_same(base, R.tracks(n_frames, pairs, lists))
    assert base.flags.any() and not base.flags.all()

    def node_sets(t):
        return {frozenset((int(a), int(b)) for a, b in t.track(i)[:, :2]) for i in range(len(t))}

    want = node_sets(base)
    assert want == R.tracks(n_frames, pairs, lists).sets
    for seed in range(4):
        order = np.random.default_rng(seed).permutation(len(pairs))
        sh = vm.host_tracks(n_frames, [pairs[i] for i in order], [lists[i] for i in order])
        R.assert_same(sh, R.tracks(n_frames, [pairs[i] for i in order], [lists[i] for i in order]))
        assert node_sets(sh) == want
        assert sh.offsets.tobytes() == base.offsets.tobytes() and sh.flags.tobytes() == base.flags.tobytes()
        assert sh.obs[:, :2].tobytes() == base.obs[:, :2].tobytes()  # (only the first naming match depends on the order)
