"""GPU suite (run with -m gpu on an MI355X): option fused_keys - the batched forms' compactions write the Delaunay chains'
keys and the chains' job tables go up in front of the matching launches (1, the default) or every chain starts with
k_upload + k_dc2_keys behind the compaction (0).  Both settings must give the same bytes, and the oracle's, in all three
batched forms: vsm_sequence_run (frames resident in HBM, so that the call takes its run-ahead order - the first pass of chunk
k in front of the second pass of chunk k - 2 - and host frames for the in-order loop; three and four chunks, so that the
pass-1 slabs, their job tables and the pair banks come round), vsm_multi_process (lists and the Tr_delta trail against the
reference's fixture) and vsm_pairs_run.  refinement = 2 shortens the lists behind the compaction and keeps the old hand-over
whatever the option says."""
import numpy as np
import pytest

import golden_util as G
from conftest import pkg

pytestmark = pytest.mark.gpu

W, H = 417, 163  # the suite's small synthetic frames
SETTINGS = [0, 1]


@pytest.fixture(scope="module")
def vm():
    m = pkg("visomatch")
    m.lib()  # raises if the HIP library is missing: no silent fallback
    return m


@pytest.fixture(scope="module")
def seq12(synth):
    return synth.stereo_sequence(31, W, H, 12, disparity=10, ramp=(1, 12))


_ORACLE = {}


def oracle_sequence(B, seq, method, mono, **params):
    """pushBack + matchFeatures per frame; computed once per case, shared and left unchanged"""
    key = (method, mono, tuple(sorted(params.items())))
    if key not in _ORACLE:
        c = B.CpuMatcher("oracle", **params)
        out = []
        for l, r in seq:
            c.push_back(l, None if mono else r)
            c.match(method)
            out.append(c.matches())
        c.close()
        _ORACLE[key] = out
    return _ORACLE[key]


def same_lists(got, want, what):
    assert len(got) == len(want), what
    for f, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), (what, f, g.shape, w.shape)


def inputs(seq, mono, resident):
    """the frames stacked: torch tensors in HBM (the run-ahead order) or numpy arrays (host-fed: the in-order loop)"""
    import torch
    left = np.stack([l for l, _ in seq])
    right = None if mono else np.stack([r for _, r in seq])
    if resident:
        left = torch.from_numpy(left).cuda()
        right = None if mono else torch.from_numpy(right).cuda()
    return left, right


@pytest.mark.parametrize("resident,chunk,ties1_host,keys_dma", [(True, "5", 1, 2), (True, "5", 0, 1), (True, "3", 1, 0), (False, "5", 1, 1)])
@pytest.mark.parametrize("method,mono", [(2, False), (0, True)])
def test_sequence_run_chunks(vm, B, seq12, monkeypatch, method, mono, resident, chunk, ties1_host, keys_dma):
    """12 frames in chunks of 5 + 5 + 2 (the slabs bank1[k & 1] come round) and of 3 (four chunks: the pair banks too), stereo
    quad (k_compact_quad) and mono flow (k_compact_write).  Resident frames: the pass-1 keys' copy on the fifth stream, the
    final keys' copy out of the pair bank on either stream (seq_keys_dma 2 / 1; 0 asks for stores of the key kernel, which
    only the old hand-over has), the pass-1 vertex sorts on the pool and on the device (which reads the keys where the
    compaction put them).  Host frames: the in-order loop, the pass-1 keys' copy on the chain's stream."""
    monkeypatch.setenv("VSM_SEQ_CHUNK", chunk)
    left, right = inputs(seq12, mono, resident)
    want = oracle_sequence(B, seq12, method, mono)
    assert min(len(x) for x in want[1:]) > 100
    for fused in SETTINGS:
        m = vm.Matcher(options={"fused_keys": fused, "seq_ties1_host": ties1_host, "seq_keys_dma": keys_dma})
        got = m.run_sequence(left, right, method)
        assert m.sequence_path() == 2, fused
        same_lists(got, want, (method, fused, resident, chunk, ties1_host, keys_dma))
        m.close()


@pytest.mark.parametrize("resident", [True, False])
@pytest.mark.parametrize("method,mono", [(2, False), (0, True)])
def test_sequence_run_with_subpixel_refinement_keeps_the_key_kernel(vm, B, seq12, monkeypatch, method, mono, resident):
    """refinement = 2: k_parabolic_apply shortens the lists after the compaction, so the keys are made behind it as before
    whatever fused_keys says - the oracle's lists under both settings, in both orders of the call"""
    monkeypatch.setenv("VSM_SEQ_CHUNK", "5")
    left, right = inputs(seq12, mono, resident)
    want = oracle_sequence(B, seq12, method, mono, refinement=2)
    assert min(len(x) for x in want[1:]) > 100
    for fused in SETTINGS:
        m = vm.Matcher(refinement=2, options={"fused_keys": fused})
        got = m.run_sequence(left, right, method)
        assert m.sequence_path() == 2
        same_lists(got, want, ("refinement 2", method, fused, resident))
        m.close()


@pytest.mark.parametrize("host_pass1", [None, "0"])
def test_multi_process_two_sequences(vm, synth, monkeypatch, host_pass1):
    """K = 2 sequences, 6 steps with live Tr_delta feedback, the first-pass lists on the pool (two sequences' default) and
    through the device chain: per setting the reference's lists and Tr_delta trail - so the settings agree byte for byte"""
    g = G.load("cfg4_multi_8procs_32f")
    w, h, nf, K = int(g["w"]), int(g["h"]), 6, 2
    seeds = [int(s) for s in g["seeds"]][:K]
    canv = {sd: synth.canvas(sd, w, h) for sd in seeds}
    frames = [{sd: synth.stereo_frame(canv[sd], f, w, h) for sd in seeds} for f in range(nf)]
    if host_pass1 is not None:
        monkeypatch.setenv("VSM_MULTI_HOST_PASS1", host_pass1)
    trails = []
    for fused in SETTINGS:
        monkeypatch.setenv("VSM_FUSED_KEYS", str(fused))  # (vsm_multi_create takes no options: read when the handle is made)
        vo = vm.MultiVisualOdometryStereo(K, *[float(x) for x in g["intr"]])
        trail = []
        for f in range(nf):
            left = np.stack([frames[f][sd][0] for sd in seeds])
            right = np.stack([frames[f][sd][1] for sd in seeds])
            ok = vo.process(left, right)
            for k, sd in enumerate(seeds):
                key = f"s{sd}_"
                fin = vo.get_matches(k, bucketed=False)
                assert len(fin) == int(g[key + "counts"][f]) and G.sha(fin) == str(g[key + "hashes"][f]), (fused, f, k, len(fin))
                assert bool(ok[k]) == bool(g[key + "ok"][f]), (fused, f, k)
                assert vo.get_motion(k).tobytes() == g[key + "tr_out"][f].tobytes(), (fused, f, k)
                trail.append(fin.tobytes() + vo.get_motion(k).tobytes())
        vo.close()
        trails.append(trail)
    assert trails[0] == trails[1]


@pytest.mark.parametrize("host_pass1", [-1, 0])
@pytest.mark.parametrize("method", [2, 0])
def test_pairs_run_four_frames_five_pairs(vm, B, seq12, method, host_pass1):
    """five (previous, current) pairs of four frames - a repeat and both directions among them - in chunks of three"""
    left = np.stack([l for l, _ in seq12[:4]])
    right = np.stack([r for _, r in seq12[:4]])
    pairs = [(0, 1), (1, 0), (0, 3), (2, 3), (0, 1)]
    if ("pairs", method) not in _ORACLE:
        want = []
        for a, b in pairs:  # the contract: a fresh oracle matcher per pair
            c = B.CpuMatcher("oracle")
            c.push_back(left[a], right[a])
            c.push_back(left[b], right[b])
            c.match(method)
            want.append(c.matches())
            c.close()
        _ORACLE[("pairs", method)] = want
    want = _ORACLE[("pairs", method)]
    assert min(len(x) for x in want) > 100
    for fused in SETTINGS:
        m = vm.Matcher(options={"fused_keys": fused, "pairs_chunk": 3, "multi_host_pass1": host_pass1})
        same_lists(m.match_pairs(left, right, pairs, method), want, (method, fused, host_pass1))
        m.close()
