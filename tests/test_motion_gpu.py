"""GPU suite (run with -m gpu on an MI355X): the HIP path on the motion families of tests/motion.py - every true match on a
limit of findMatch's search window (match radius, stereo tolerance, sign tests, pass-2 prior boxes, bin and fine-row
edges, the motion prior's clamp) or one step beyond it.  Everything is tobytes() equality with the CPU oracle run side by
side, and with the counts and hashes the reference left in tests/golden/motion_hashes.npz; no tolerance anywhere.  Every
test asserts from the oracle's side that its lists are long inside the limit and short outside (motion.check_sizes).
tests/test_motion_cpu.py pins the oracle on the same cases."""
import numpy as np
import pytest

import content as CT
import golden_util as G
import motion as MO
import test_content_gpu as TCG
from conftest import pkg

pytestmark = pytest.mark.gpu

IDS = [f"{fam}-{grp}" for fam, grp in MO.GROUPS]


@pytest.fixture(scope="module")
def vm():
    m = pkg("visomatch")
    m.lib()  # raises if the HIP library is missing: no silent fallback
    return m


@pytest.mark.parametrize("fam,grp", MO.GROUPS, ids=IDS)
def test_per_frame_vs_oracle_and_golden(vm, B, fam, grp):
    """pushBack + matchFeatures on both frames of every case: all feature sets, match()'s value, stages 0-4, the prior ranges
    and the final list - a wrong limit is reported at the stage where it acts"""
    MO.check_sizes(B, fam, grp)
    g = G.load("motion_hashes")
    for c in MO.cases(fam, grp):
        m = vm.Matcher(stage_capture=True, **dict(c.params))
        got = MO.record(m, c)
        m.close()
        CT.assert_same_records(got, MO.oracle_case(B, c), c.name)
        MO.check_against_golden(g, c, got)


@pytest.mark.parametrize("fam,grp", MO.GROUPS, ids=IDS)
def test_pairs_in_one_batched_call(vm, B, fam, grp):
    """the group's frames as one set through match_pairs with the pairs (previous, current) and (current, previous) - the
    reverse pair has every displacement with the opposite sign and oracle lists of its own; chunks of 3 and 50 pairs, the
    first pass's prior boxes from the host pool and from k_dc2_prior"""
    MO.check_sizes(B, fam, grp)
    left, right, pairs, Tr, valid, cs = MO.pair_set(fam, grp)
    want = MO.oracle_pairs(B, fam, grp)
    sizes = [len(x) for x in want]
    print("oracle list sizes", fam, grp, sizes)
    assert max(sizes[1::2]) >= 400, sizes   # the reverse pairs are not vacuous either
    c0 = cs[0]
    for chunk in (3, 50):
        for options in ({"pairs_chunk": chunk}, {"pairs_chunk": chunk, "multi_host_pass1": 0}):
            m = vm.Matcher(options=options, **dict(c0.params))
            if c0.intr:
                m.set_intrinsics(*c0.intr)
            got = m.match_pairs(left, right if c0.method else None, pairs, c0.method, Tr_delta=Tr, Tr_valid=valid if Tr is not None else None)
            m.close()
            assert len(got) == len(want)
            for k, (a, b) in enumerate(zip(got, want)):
                assert CT.same(a, b), (fam, grp, options, cs[k // 2].name, "reverse" if k % 2 else "forward", len(a), len(b))


@pytest.mark.parametrize("fam,method", MO.SEQUENCES, ids=[f"{f}-m{m}" for f, m in MO.SEQUENCES])
def test_jerky_sequence(vm, B, monkeypatch, fam, method):
    """one sequence whose consecutive steps are the family's displacements, inside and outside alternating, through
    run_sequence in the GPU-resident and the host-shared form, against the oracle run frame by frame"""
    seq, params, tr, intr = MO.sequence(fam, method)
    h, w = seq[0][0].shape
    c = B.CpuMatcher("oracle", **params)
    if intr:
        c.set_intrinsics(*intr)
    want, nq0, nq1 = [], 0, 0
    for f, (l, r) in enumerate(seq):
        c.push_back(l, r if method else None)
        nq0, nq1 = max(nq0, len(c.features("1c1"))), max(nq1, len(c.features("1c2")))
        c.match(method, tr if f else None)
        want.append(c.matches())
    c.close()
    lens = [len(x) for x in want]
    print("oracle list sizes", fam, method, lens)
    first = 0 if method == 1 else 1   # (stereo matching has a list on the first frame too)
    assert max(lens) >= 400, lens
    if fam != "tr_prior":   # long and short lists follow each other (tr_prior: every step is inside, the prior decides)
        assert min(lens[first:]) * 2 <= max(lens), lens
    left = np.stack([l for l, _ in seq])
    right = np.stack([r for _, r in seq]) if method else None
    Tr = np.stack([tr] * len(seq)) if tr is not None else None
    valid = [0] + [1] * (len(seq) - 1) if tr is not None else None
    for v2 in (1, 0):
        monkeypatch.setenv("VSM_SEQ_V2", str(v2))
        g = vm.Matcher(**params)
        if intr:
            g.set_intrinsics(*intr)
        got = g.run_sequence(left, right, method, Tr_delta=Tr, Tr_valid=valid)
        path = g.sequence_path()
        g.close()
        for f in range(len(seq)):
            assert CT.same(got[f], want[f]), (fam, method, v2, f, len(got[f]), len(want[f]))
        assert path == TCG._expected_path(vm, w, h, params, v2, nq0, nq1), (fam, method, v2, path)
