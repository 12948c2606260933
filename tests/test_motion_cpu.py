"""The motion families of tests/motion.py (matches on the limits of the search window: radius, tolerance, sign, prior boxes)
on the CPU: that every boundary pair reaches its conditions (measured with the oracle), the oracle against the compiled
reference on every case (where that build is present), and the oracle against the counts and hashes the reference left
in tests/golden/motion_hashes.npz (tests/golden/make_golden.py motion).  tests/test_motion_gpu.py runs the HIP path over
the same cases.
"""
import hashlib

import numpy as np
import pytest

import content as CT
import golden_util as G
import motion as MO

needs_ref = pytest.mark.skipif(not __import__("oracle.bindings", fromlist=["x"]).have_ref(),
                               reason="oracle/_ref/libvisoref.so not built")
IDS = [f"{fam}-{grp}" for fam, grp in MO.GROUPS]


@pytest.mark.parametrize("fam,grp", MO.GROUPS, ids=IDS)
def test_boundary_pairs_reach_their_conditions(B, fam, grp):
    """at least 400 matches inside, at least twice the outside's (tr_prior: the Tr_delta changes the list), and the sizes
    recorded in motion.ORACLE_SIZES"""
    MO.check_sizes(B, fam, grp)


def test_case_names_are_unique_and_recorded():
    names = [c.name for c in MO.all_cases()]
    assert len(names) == len(set(names))
    assert sorted(MO.ORACLE_SIZES) == sorted(n[:-3] for n in names if n.endswith("|in"))


def test_the_steps_are_the_smallest_that_cross_a_limit():
    """inside and outside differ by one band's displacement in one coordinate (split_motion's and quad_window's outside cases:
    one per band or image pair), by 1 px at full and 2 px at half resolution; half-resolution displacements are even"""
    for c in MO.all_cases():
        half = dict(c.params).get("half_resolution", 1)
        if half:
            for spec in (c.prev, c.curr):
                for side in spec:
                    assert side is None or all(b[4] % 2 == 0 and b[5] % 2 == 0 for b in side), c.name
    for fam, grp in MO.GROUPS:
        if fam == "tr_prior":
            continue
        for p in MO.groups(fam)[grp]:
            step = 2 if dict(p.inside.params).get("half_resolution", 1) else 1
            diffs = set()
            for si, so in zip(p.inside.prev + p.inside.curr, p.outside.prev + p.outside.curr):
                if si is not None:
                    diffs |= {(abs(a[4] - b[4]), abs(a[5] - b[5])) for a, b in zip(si, so)}
            if fam == "stereo_window" and "/sign/d" in p.inside.name and not p.inside.name.endswith("d0|in"):
                continue   # (d = 1 and 2 against -2: further inside, not a smallest step)
            assert diffs - {(0, 0)} and diffs <= {(0, 0), (step, 0), (0, step)}, (p.inside.name, diffs)


@needs_ref
@pytest.mark.parametrize("fam,grp", MO.GROUPS, ids=IDS)
def test_oracle_vs_reference(B, fam, grp):
    """feature sets, match()'s value, the five stages, the prior ranges and the final list of both frames of every case"""
    for c in MO.cases(fam, grp):
        r = B.CpuMatcher("ref", **dict(c.params))
        got = MO.record(r, c)
        r.close()
        CT.assert_same_records(MO.oracle_case(B, c), got, c.name)


@pytest.mark.parametrize("fam,grp", MO.GROUPS, ids=IDS)
def test_golden_motion_oracle(B, fam, grp):
    g = G.load("motion_hashes")
    MO.check_golden_inputs(g, B)
    for c in MO.cases(fam, grp):
        MO.check_against_golden(g, c, MO.oracle_case(B, c))
