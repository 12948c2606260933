"""CPU suite: the chunk plan of the look-ahead call's GPU-resident form (csrc/vsm_jobs.h: seq2_plan, through the debug
entry vsm_debug_seq_plan - pure arithmetic, no GPU).  The expected plans were worked out from the arithmetic of the commit
before the planner was lifted out of sequence_run_v2 (110 + 90, 40 + 80 + 60 + 20, ten chunks of
100 for 1000 frames): they pin what that commit did, not what the function returns today."""
import os
import subprocess

import pytest

from conftest import ROOT, pkg


def _ensure_built():
    vm = pkg("visomatch")
    if not os.path.exists(vm.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "opencl-structure-from-motion_amd", "csrc")])
    return vm


RESIDENT, HOST_FED = False, True

# (host_in, pool threads, frames, seq_chunk, seq_first_chunk, plan string) -> (chunk size, starts)
PLANS = [
    ((RESIDENT, 14, 200, 0, 0, None), (110, [0, 110, 200])),
    ((RESIDENT, 14, 1000, 0, 0, None), (100, list(range(0, 1001, 100)))),  # not nine of 110 and one of 10
    ((RESIDENT, 14, 230, 0, 0, None), (77, [0, 77, 154, 230])),
    ((RESIDENT, 8, 200, 0, 0, None), (80, [0, 80, 160, 200])),
    ((RESIDENT, 4, 200, 0, 0, None), (100, [0, 100, 200])),
    ((RESIDENT, 5, 200, 0, 0, None), (50, [0, 50, 100, 150, 200])),
    ((HOST_FED, 14, 200, 0, 0, None), (80, [0, 40, 120, 180, 200])),  # half a chunk first, a short one last
    ((HOST_FED, 8, 200, 0, 0, None), (80, [0, 40, 120, 180, 200])),
    ((HOST_FED, 4, 200, 0, 0, None), (50, [0, 25, 75, 125, 175, 200])),
    ((RESIDENT, 14, 200, 0, 4, None), (110, [0, 4, 114, 200])),
    ((HOST_FED, 14, 200, 0, 4, None), (80, [0, 40, 120, 180, 200])),  # seq_first_chunk is for resident frames
    ((RESIDENT, 14, 7, 3, 0, None), (3, [0, 3, 6, 7])),
    ((HOST_FED, 14, 7, 3, 0, None), (3, [0, 1, 4, 7])),
    ((RESIDENT, 14, 5, 0, 0, None), (5, [0, 5])),
    ((HOST_FED, 14, 5, 0, 0, None), (5, [0, 5])),
    ((RESIDENT, 1, 1, 0, 0, None), (1, [0, 1])),
    # the plan string: host-fed calls only, every entry clamped to [2, chunk size], the rest in whole chunks
    ((HOST_FED, 14, 200, 0, 0, "40,80,60,20"), (80, [0, 40, 120, 180, 200])),
    ((HOST_FED, 4, 200, 0, 0, "40,80,60,20"), (50, [0, 40, 90, 140, 160, 200])),
    ((HOST_FED, 14, 200, 0, 0, "40,1"), (80, [0, 40, 42, 122, 200])),
    ((RESIDENT, 14, 200, 0, 0, "40,80,60,20"), (110, [0, 110, 200])),
]


@pytest.mark.parametrize("args,expected", PLANS, ids=["-".join("host" if x is True else "hbm" if x is False else str(x) for x in a) for a, _ in PLANS])
def test_plan_is_pinned(args, expected):
    vm = _ensure_built()
    host_in, threads, frames, seq_chunk, first, plan = args
    chunk, starts = vm.seq_plan(frames, threads, host_in, seq_chunk, first, plan)
    assert (chunk, starts) == expected
    # what every plan has to be, whatever its sizes: the banks are laid out for chunks of at most `chunk` frames
    assert starts[0] == 0 and starts[-1] == frames
    assert all(0 < b - a <= chunk for a, b in zip(starts, starts[1:]))


def test_plan_rejects_bad_arguments():
    vm = _ensure_built()
    with pytest.raises(vm.VisoMatchError):
        vm.seq_plan(0, 14)
    with pytest.raises(vm.VisoMatchError):
        vm.seq_plan(200, 0)
