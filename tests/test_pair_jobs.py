"""CPU suite: the job table of Matcher.match_pairs / vsm_pairs_run (csrc/vsm_jobs.h: pair_jobs, through the debug entry
vsm_debug_pair_jobs - pure arithmetic, no GPU).

The expected values do not come from the function: they restate the call's contract - for pair (a, b) a fresh matcher after
pushBack(a), pushBack(b), matchFeatures(method, Tr of the pair) - pair by pair in Python (`expected` below), with
Matcher::matchFeatures' sanity checks written out again (`match_ready`)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg


def _ensure_built():
    vm = pkg("visomatch")
    if not os.path.exists(vm.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "opencl-structure-from-motion_amd", "csrc")])
    return vm


SPARSE, DENSE = 0, 1
LEFT, RIGHT = 0, 1
N_FRAMES = 6
# a keyframe against later frames, both directions, a self pair, a repeated pair, a loop closure
PAIRS = [(0, 1), (0, 2), (3, 1), (2, 2), (0, 5), (5, 0), (4, 3), (0, 1), (1, 4), (5, 5)]
CHUNKS = [1, 3, len(PAIRS), len(PAIRS) + 7]
FORMS = [(sides, method) for sides in (1, 2) for method in (0, 1, 2)]


def match_ready(method, multi_stage, prev, curr):
    """the sanity checks of Matcher::matchFeatures (viso/matcher.cpp:190-212) on the counts [side][set] of the previous and
    the current frame: flow needs both left images' sets, stereo the current pair's, quad matching all four"""
    used = {0: [prev[LEFT], curr[LEFT]], 1: [curr[LEFT], curr[RIGHT]], 2: [prev[LEFT], prev[RIGHT], curr[LEFT], curr[RIGHT]]}[method]
    if any(img[DENSE] == 0 for img in used):
        return False
    return not (multi_stage and any(img[SPARSE] == 0 for img in used))


def expected(method, multi_stage, sides, counts, pairs, chunk, tr_valid):
    """per pair (img_prev, img_curr, nq[0], nq[1], use_tr, valid, pair number of the Tr taken) and per chunk max_nq"""

    def of(f):  # counts [side][set] of frame f as a matcher holds them: no right image of mono input
        return [[int(counts[f][side][s]) if side < sides else 0 for s in (SPARSE, DENSE)] for side in (LEFT, RIGHT)]

    rows = []
    max_nq = [[0, 0] for _ in range(0, len(pairs), chunk)]
    for k, (a, b) in enumerate(pairs):
        curr = of(b)
        prev = [[0, 0], [0, 0]] if method == 1 else of(a)  # stereo matching does not read the previous frame
        valid = match_ready(method, multi_stage, prev, curr)
        query = prev[LEFT] if method == 2 else curr[LEFT]  # quad matching walks the previous left image's features
        nq = [query[SPARSE] if multi_stage else 0, query[DENSE]] if valid else [0, 0]
        use_tr = int(valid and (tr_valid is None or bool(tr_valid[k])))
        rows.append((sides * (b if method == 1 else a), sides * b, nq[0], nq[1], use_tr, int(valid), k + 1 if use_tr else 0))
        max_nq[k // chunk] = [max(x, y) for x, y in zip(max_nq[k // chunk], nq)]
    return rows, max_nq


def base_counts(n=N_FRAMES):
    """every set present, every count different (so that a query count names its frame, side and set)"""
    c = np.zeros((n, 2, 2), dtype=np.int32)
    for f in range(n):
        for side in (LEFT, RIGHT):
            for s in (SPARSE, DENSE):
                c[f, side, s] = 100 + 8 * f + 2 * side + s
    return c


# name -> the (frame, side, set) entries that are zero: each of the sets the checks read, in a frame that is mostly a previous
# frame (frame 0: of five pairs, the current one of (5, 0)) and in one that is mostly a current frame (frame 1: of three pairs,
# the previous one of (1, 4))
ZEROS = {
    "none": [],
    "frame0_left_dense": [(0, LEFT, DENSE)],
    "frame0_left_sparse": [(0, LEFT, SPARSE)],
    "frame0_right_dense": [(0, RIGHT, DENSE)],
    "frame0_right_sparse": [(0, RIGHT, SPARSE)],
    "frame1_left_dense": [(1, LEFT, DENSE)],
    "frame1_left_sparse": [(1, LEFT, SPARSE)],
    "frame1_right_dense": [(1, RIGHT, DENSE)],
    "frame1_right_sparse": [(1, RIGHT, SPARSE)],
    "self_pair_frame": [(2, LEFT, DENSE)],
}
TR_VALID = [None, np.ones(len(PAIRS), np.uint8), (np.arange(len(PAIRS)) % 3 != 1).astype(np.uint8)]


def zeroed(name):
    counts = base_counts()
    for f, side, s in ZEROS[name]:
        counts[f, side, s] = 0
    return counts


def pairs_for(method):
    """stereo matching also takes pairs without a previous frame"""
    return PAIRS + [(-1, 3), (-1, 1)] if method == 1 else PAIRS


@pytest.mark.parametrize("multi_stage", (0, 1))
@pytest.mark.parametrize("sides,method", FORMS, ids=[f"sides{s}-method{m}" for s, m in FORMS])
def test_jobs_follow_the_contract(sides, method, multi_stage):
    vm = _ensure_built()
    pairs = pairs_for(method)
    for name in ZEROS:
        counts = zeroed(name)
        for tv in TR_VALID:
            tv = None if tv is None else np.resize(tv, len(pairs))
            for chunk in CHUNKS:
                got, max_nq = vm.pair_jobs(method, multi_stage, sides, counts, pairs, chunk, tv)
                rows, exp_max = expected(method, multi_stage, sides, counts, pairs, chunk, tv)
                what = f"{name} chunk={chunk} tr_valid={None if tv is None else tv.tolist()}"
                assert got.tolist() == [list(r) for r in rows], what
                assert max_nq.tolist() == exp_max, what


def test_cases_do_what_they_are_for():
    """the conditions on the case list, from the contract alone (`expected`)"""
    clean = {}
    for sides, method in FORMS:
        for multi_stage in (0, 1):
            pairs = pairs_for(method)
            rows0, _ = expected(method, multi_stage, sides, base_counts(), pairs, 3, None)
            clean[sides, method, multi_stage] = [r[5] for r in rows0]
            if sides == 1 and method != 0:  # mono input is flow-matched only: stereo and quad matching return early everywhere
                assert not any(clean[sides, method, multi_stage])
                continue
            assert all(clean[sides, method, multi_stage])
            for name in ZEROS:
                rows, max_nq = expected(method, multi_stage, sides, zeroed(name), pairs, 3, None)
                valid = [r[5] for r in rows]
                side_read = "right" not in name or (sides == 2 and method != 0)
                set_read = "sparse" not in name or multi_stage
                reads = name != "none" and side_read and set_read  # (every zeroed frame is some pair's current frame)
                assert (valid != clean[sides, method, multi_stage]) == reads, (sides, method, multi_stage, name)
                assert any(valid), name  # never a table of invalid pairs only
                # the chunks' maxima differ from each other: a table that reported one maximum for all would not pass
                assert len({tuple(m) for m in max_nq}) > 1
    # quad matching takes its queries from the previous frame, the others from the current one: (0, 5) and (5, 0) tell
    rows, _ = expected(2, 1, 2, base_counts(), PAIRS, 3, None)
    assert rows[4][2:4] != rows[5][2:4] and rows[0] == rows[7][:6] + (1,)
    # the mixed flags switch Tr off for some pairs and leave it on for others
    rows, _ = expected(2, 1, 2, base_counts(), PAIRS, 3, TR_VALID[2])
    assert {r[4] for r in rows} == {0, 1}


def test_bad_arguments_are_rejected():
    vm = _ensure_built()
    counts = base_counts()
    bad = [
        (2, 1, 2, counts, [(0, N_FRAMES)], 3),      # a current frame past the set
        (2, 1, 2, counts, [(N_FRAMES, 0)], 3),      # a previous frame past the set
        (2, 1, 2, counts, [(-1, 0)], 3),            # no previous frame, quad matching
        (0, 1, 2, counts, [(-1, 0)], 3),            # ... flow matching
        (1, 1, 2, counts, [(-2, 0)], 3),            # stereo matching takes -1, nothing below
        (1, 1, 2, counts, [(0, -1)], 3),            # the current frame is always read
        (2, 1, 2, counts, np.zeros((0, 2)), 3),     # no pairs
        (3, 1, 2, counts, [(0, 1)], 3),             # no such method
        (2, 1, 3, counts, [(0, 1)], 3),             # no such input
        (2, 1, 2, counts, [(0, 1)], 0),             # no such chunk
    ]
    for args in bad:
        with pytest.raises(vm.VisoMatchError):
            vm.pair_jobs(*args)
    vm.pair_jobs(1, 1, 2, counts, [(-1, 0)], 3)  # (the one pair without a previous frame that is accepted)
