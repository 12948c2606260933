"""GPU suite (run with -m gpu on an MI355X): Matcher.match_pairs / vsm_pairs_run - arbitrary (previous, current) frame pairs
of an image set in one batched call.  The expected list of pair (a, b) is getMatches() of a FRESH CPU oracle matcher after
pushBack(a), pushBack(b), matchFeatures(method, Tr of the pair); everything is tobytes() equality, no tolerance anywhere.
Every test asserts list sizes from the oracle's side (the figures were computed with the oracle on the CPU), so that no
case can pass on empty lists."""
import numpy as np
import pytest

import content as CT
from conftest import pkg

pytestmark = pytest.mark.gpu

W, H, N = 417, 163, 7
PAIRS = [(0, 1), (0, 2), (3, 1), (2, 2), (0, 6), (6, 0), (5, 4), (0, 1)]  # a keyframe, a self pair, both directions, a repeat
SCENE_PAIRS = [(0, 1), (2, 3), (3, 2), (1, 2), (4, 5), (5, 4), (2, 5), (4, 4), (6, 7), (1, 6)]
SCENE_QUAD_SIZES = [0, 246, 245, 0, 215, 214, 0, 246, 0, 0]
METHODS = (2, 0, 1)


@pytest.fixture(scope="module")
def vm():
    m = pkg("visomatch")
    m.lib()  # raises if the HIP library is missing: no silent fallback
    return m


@pytest.fixture(scope="module")
def frames(synth):
    """case 1's frames, stacked: ([N,H,W] left, [N,H,W] right)"""
    return CT.stack(synth.stereo_sequence(31, W, H, N, disparity=10, ramp=(1, 12)))


_ORACLE = {}


def oracle_pairs(B, key, left, right, pairs, method, Tr=None, Tr_valid=None, intr=None, **params):
    """the contract, pair by pair: a fresh oracle matcher per pair.  Computed once per key, shared and left unchanged."""
    key = (key, tuple(pairs), method, None if Tr is None else np.asarray(Tr).tobytes(), None if Tr_valid is None else tuple(Tr_valid), intr,
           tuple(sorted(params.items())))
    if key not in _ORACLE:
        out = []
        for k, (a, b) in enumerate(pairs):
            c = B.CpuMatcher("oracle", **params)
            if intr:
                c.set_intrinsics(*intr)
            for f in (a, b):
                if f >= 0:
                    c.push_back(left[f], None if right is None else right[f])
            c.match(method, Tr[k] if Tr is not None and (Tr_valid is None or Tr_valid[k]) else None)
            out.append(c.matches())
            c.close()
        _ORACLE[key] = out
    return _ORACLE[key]


def assert_same_lists(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), (what, k, g.shape, w.shape)


# ---- 1: three methods across chunk boundaries ---------------------------------------------------------------------------

@pytest.mark.parametrize("method", METHODS)
def test_methods_across_chunk_boundaries(vm, B, frames, method):
    left, right = frames
    want = oracle_pairs(B, "case1", left, right, PAIRS, method)
    sizes = [len(x) for x in want]
    print("oracle list sizes, method", method, sizes)
    assert min(sizes) >= 750, sizes
    assert want[0].tobytes() == want[7].tobytes() and want[4].tobytes() != want[5].tobytes()
    for chunk in (1, 3, 50):
        m = vm.Matcher(options={"pairs_chunk": chunk})
        got = m.match_pairs(left, right, PAIRS, method)
        assert_same_lists(got, want, (method, chunk))
        assert got[0].tobytes() == got[7].tobytes() and got[4].tobytes() != got[5].tobytes()
        t = m.pair_timings()
        assert t["total_us"] > 0 and t["image_side_us"] > 0
        m.close()


@pytest.mark.parametrize("method", METHODS)
def test_first_pass_chain_on_the_device(vm, B, frames, method):
    """the first-pass lists' outlier removal and prior boxes by the device chain (what chunks of more pairs than host threads
    take by themselves) instead of the host pool"""
    left, right = frames
    want = oracle_pairs(B, "case1", left, right, PAIRS, method)
    for chunk in (3, 50):
        m = vm.Matcher(options={"pairs_chunk": chunk, "multi_host_pass1": 0})
        assert_same_lists(m.match_pairs(left, right, PAIRS, method), want, (method, chunk))
        m.close()


# ---- 2: scene changes ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", METHODS)
def test_scene_changes(vm, B, method):
    left, right = CT.stack(CT.scene_changes(8, 256, 96))
    want = oracle_pairs(B, "scenes", left, right, SCENE_PAIRS, method)
    sizes = [len(x) for x in want]
    print("oracle list sizes, method", method, sizes)
    if method == 2:
        assert sizes == SCENE_QUAD_SIZES
        assert sum(s == 0 for s in sizes) >= 4 and sum(s > 200 for s in sizes) >= 4
    else:
        assert min(sizes) == 0 and max(sizes) > 200, sizes
    for options in ({}, {"pairs_chunk": 4}, {"pairs_chunk": 4, "multi_host_pass1": 0}):
        m = vm.Matcher(options=options)
        assert_same_lists(m.match_pairs(left, right, SCENE_PAIRS, method), want, (method, options))
        m.close()


# ---- 3: a motion prior per pair ----------------------------------------------------------------------------------------------

def test_motion_prior_per_pair(vm, B):
    left, right = CT.stack(CT.stereo_sequence("tile64", 256, 96, 5))
    intr = (400.0, 128.0, 48.0, 0.5)
    pairs = [(0, 2), (3, 1), (0, 1)]
    tr = np.eye(4)
    tr[0, 3] = 0.15
    Tr = np.stack([tr] * 3)
    plain = oracle_pairs(B, "prior", left, right, pairs, 2, intr=intr)
    prior = oracle_pairs(B, "prior", left, right, pairs, 2, Tr=Tr, intr=intr)
    mixed = oracle_pairs(B, "prior", left, right, pairs, 2, Tr=Tr, Tr_valid=(1, 0, 1), intr=intr)
    print("oracle list sizes without / with the prior", [len(x) for x in plain], [len(x) for x in prior])
    assert all(len(x) >= n for x, n in zip(plain, (124, 130, 57))) and all(len(x) >= n for x, n in zip(prior, (42, 33, 12)))
    assert all(a.tobytes() != b.tobytes() for a, b in zip(plain, prior))  # the prior is really exercised
    assert mixed[1].tobytes() == plain[1].tobytes() and mixed[0].tobytes() == prior[0].tobytes()
    m = vm.Matcher()
    m.set_intrinsics(*intr)
    assert_same_lists(m.match_pairs(left, right, pairs, 2), plain, "no prior")
    assert_same_lists(m.match_pairs(left, right, pairs, 2, Tr_delta=Tr), prior, "prior")
    assert_same_lists(m.match_pairs(left, right, pairs, 2, Tr_delta=Tr, Tr_valid=[1, 0, 1]), mixed, "prior, flags 1 0 1")
    m.close()


# ---- 4: parameter sets ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params,least", [({"refinement": 2}, 740), ({"multi_stage": 0}, 710), ({"half_resolution": 0}, 3000)],
                         ids=["refinement2", "single_stage", "full_resolution"])
def test_parameter_sets(vm, B, frames, params, least):
    left, right = frames
    pairs = PAIRS[:5]
    want = oracle_pairs(B, "case1", left, right, pairs, 2, **params)
    sizes = [len(x) for x in want]
    print("oracle list sizes", params, sizes)
    assert min(sizes) >= least, sizes
    for options in ({"pairs_chunk": 2}, {"pairs_chunk": 50, "multi_host_pass1": 0}):
        m = vm.Matcher(options=options, **params)
        assert_same_lists(m.match_pairs(left, right, pairs, 2), want, (params, options))
        m.close()


# ---- 5: mono input ---------------------------------------------------------------------------------------------------------------

def test_mono_input(vm, B, frames):
    left, right = frames
    want = oracle_pairs(B, "case1", left, right, PAIRS, 0)  # (flow matching reads the left images only)
    # (879 is the oracle's size of the first list, pair (0, 1); its shortest flow list of these pairs is (5, 4) with 870)
    assert len(want[0]) >= 879 and min(len(x) for x in want) >= 870
    assert_same_lists(oracle_pairs(B, "case1-mono", left, None, PAIRS, 0), want, "the oracle on mono input")
    for chunk in (3, 50):
        m = vm.Matcher(options={"pairs_chunk": chunk})
        assert_same_lists(m.match_pairs(left, None, PAIRS, 0), want, ("mono", chunk))
        for method in (2, 1):  # matchFeatures returns early: empty lists, and the call succeeds
            got = m.match_pairs(left, None, PAIRS, method)
            assert [len(x) for x in got] == [0] * len(PAIRS), method
        m.close()
    # an odd and an even number of mono frames, each through the front end once
    m = vm.Matcher()
    assert_same_lists(m.match_pairs(left[:6], None, [(0, 5), (5, 4)], 0), oracle_pairs(B, "case1", left, right, [(0, 5), (5, 4)], 0), "six frames")
    m.close()


# ---- 6: device-resident inputs ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", (2, 0))
def test_device_inputs(vm, B, frames, method):
    import torch
    left, right = frames
    want = oracle_pairs(B, "case1", left, right, PAIRS, method)
    m = vm.Matcher(options={"pairs_chunk": 3})
    host = m.match_pairs(left, right, PAIRS, method)
    assert_same_lists(host, want, "host input")
    dl, dr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    assert_same_lists(m.match_pairs(dl, dr, PAIRS, method), host, "contiguous tensors")
    wide = [torch.full((N, H, 448), 255, dtype=torch.uint8, device="cuda") for _ in range(2)]
    wide[0][:, :, :W] = dl
    wide[1][:, :, :W] = dr
    vl, vr = wide[0][:, :, :W], wide[1][:, :, :W]
    assert vl.stride() == (H * 448, 448, 1)
    assert_same_lists(m.match_pairs(vl, vr, PAIRS, method), host, "views with a row stride of 448 bytes")
    assert_same_lists(m.match_pairs(vl, None, PAIRS, 0), oracle_pairs(B, "case1", left, right, PAIRS, 0), "a mono view")
    m.close()


# ---- 7: ties to the existing forms -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", (2, 0))
def test_ties_to_sequence_and_ring(vm, B, frames, method):
    left, right = frames
    m = vm.Matcher()
    # the ring, filled by the caller's own pushes
    assert m.push_back(left[2], right[2]) == 0 and m.push_back(left[5], right[5]) == 0
    assert m.match(method)
    ring = m.get_matches()
    assert ring.tobytes() == oracle_pairs(B, "case1", left, right, [(2, 5)], method)[0].tobytes()
    before = m.run_sequence(left, right, method)
    consecutive = [(f - 1, f) for f in range(1, N)]
    want = oracle_pairs(B, "case1", left, right, consecutive, method)
    assert len(ring) >= 700 and min(len(x) for x in want) >= 700, [len(x) for x in want]  # (the oracle's shortest: 745, quad, pair (5, 6))
    got = m.match_pairs(left, right, consecutive, method)
    assert_same_lists(got, want, "pairs (f-1, f) against the oracle")
    assert_same_lists(got, before[1:], "pairs (f-1, f) against run_sequence")
    assert_same_lists(m.run_sequence(left, right, method), before, "run_sequence after match_pairs")
    assert m.get_matches().tobytes() == ring.tobytes()
    # ... and the ring goes on from where it was: frame 5 is still its current frame
    assert m.push_back(left[6], right[6]) == 0 and m.match(method)
    assert m.get_matches().tobytes() == oracle_pairs(B, "case1", left, right, [(5, 6)], method)[0].tobytes()
    m.close()


# ---- 8: what the device chain cannot take ----------------------------------------------------------------------------------------

def test_fallback_beyond_1024_statistics_bins(vm, B, frames):
    """match_binsize = 8 at 417 x 163: 53 x 21 = 1113 statistics bins, more than k_dc2_prior keeps in LDS (the oracle accepts
    this bin size and gives the list sizes asserted below: checked on the CPU)"""
    left, right = frames
    assert -(-W // 8) * -(-H // 8) > 1024
    pairs = [(0, 2), (6, 0), (3, 3)]
    want = oracle_pairs(B, "case1", left, right, pairs, 2, match_binsize=8)
    sizes = [len(x) for x in want]
    print("oracle list sizes, match_binsize 8", sizes)
    assert min(sizes) >= 700, sizes
    m = vm.Matcher(match_binsize=8)
    assert m.push_back(left[1], right[1]) == 0 and m.push_back(left[4], right[4]) == 0 and m.match(2)
    ring = m.get_matches()
    assert len(ring) >= 700
    assert_same_lists(m.match_pairs(left, right, pairs, 2), want, "fallback")
    assert m.get_matches().tobytes() == ring.tobytes()  # the caller's ring was set aside and put back
    assert m.push_back(left[5], right[5]) == 0 and m.match(2)
    assert m.get_matches().tobytes() == oracle_pairs(B, "case1", left, right, [(4, 5)], 2, match_binsize=8)[0].tobytes()
    m.close()


BIG_W, BIG_H = 1344, 720
BIG_PAIRS = [(2, 1), (0, 1), (2, 0)]
BIG_SIZES = {2: (7418, 14984, 8637), 0: (7668, 15224, 8911)}  # the oracle's list sizes, per method and pair


@pytest.fixture(scope="module")
def big_frames(synth):
    """three stereo frames of 1344 x 720; the right half of frame 2 is blank, which halves its features"""
    cv = synth.canvas(5, BIG_W, BIG_H)
    seq = [synth.stereo_frame(cv, f, BIG_W, BIG_H) for f in range(3)]
    for img in seq[2]:
        img[:, BIG_W // 2:] = 96
    return CT.stack(seq)


@pytest.mark.parametrize("chunk", (1, 3))
@pytest.mark.parametrize("method", (2, 0))
def test_fallback_of_a_chunk_beyond_the_refinement_limit(vm, B, big_frames, method, chunk):
    """refinement = 2 batches lists of up to 16384 entries (VSM_PARA_MAX_LIST); the second-pass list of a pair is as long as
    the dense set of its previous frame.  Frames 0 and 1 have 18051 and 18040 dense features, the half-blanked frame 2 has
    9077 (the oracle's counts): a chunk that holds pair (0, 1) goes pair by pair, the others through the device chain.
    pairs_chunk = 1: chain, fall-back, chain - a chain chunk after the ring was set aside; 3: one long list sends the
    whole chunk through the fall-back."""
    left, right = big_frames
    want = oracle_pairs(B, "big", left, right, BIG_PAIRS, method, refinement=2)
    sizes = tuple(len(x) for x in want)
    print("oracle list sizes, method", method, sizes)
    assert sizes == BIG_SIZES[method] and min(sizes) > 1000
    m = vm.Matcher(options={"pairs_chunk": chunk}, refinement=2)
    # the caller's own pushes: they also show the precondition that forces the path
    assert m.push_back(left[0], right[0]) == 0
    dense0 = len(m.features("1c2"))
    assert m.push_back(left[2], right[2]) == 0
    dense2 = len(m.features("1c2"))
    print("dense features of frames 0 and 2", dense0, dense2)
    assert dense0 > 16384 > dense2
    assert m.match(method)
    ring = m.get_matches()
    assert len(ring) > 1000
    got = m.match_pairs(left, right, BIG_PAIRS, method)
    assert_same_lists(got, want, (method, chunk))
    assert min(len(x) for x in got) > 1000
    assert m.get_matches().tobytes() == ring.tobytes()  # the caller's ring was set aside and put back
    m.close()


# ---- 9: bad arguments ------------------------------------------------------------------------------------------------------------

def test_bad_arguments(vm, B, frames):
    left, right = frames
    m = vm.Matcher()
    good = m.match_pairs(left, right, PAIRS[:3], 2)
    assert min(len(x) for x in good) >= 750
    for pairs, method in (([(0, 1), (0, N)], 2), ([(N, 0)], 0), ([(-1, 0)], 2), ([(-1, 0)], 0), ([(-2, 0)], 1), (np.zeros((0, 2), np.int32), 2)):
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            m.match_pairs(left, right, pairs, method)
        assert_same_lists([m.pair_matches(k) for k in range(3)], good, "the last good call's lists")
    stereo = m.match_pairs(left, right, [(-1, 3), (0, 3)], 1)  # (stereo matching does not read the previous frame)
    assert len(stereo[0]) >= 750 and stereo[0].tobytes() == stereo[1].tobytes()
    assert stereo[0].tobytes() == oracle_pairs(B, "case1", left, right, [(-1, 3)], 1)[0].tobytes()
    m.close()
