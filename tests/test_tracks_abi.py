"""CPU suite: the feature-track entry points are exported and their constants agree between include/visomatch.h and the
Python binding."""
import os
import re
import subprocess

from conftest import ROOT, pkg

SYMBOLS = ["vsm_tracks_run", "vsm_pairs_tracks", "vsm_tracks_count", "vsm_tracks_num_obs", "vsm_tracks_get", "vsm_tracks_of_matches",
           "vsm_tracks_get_stats", "vsm_tracks_get_timings", "vsm_host_tracks"]


def _vm():
    vm = pkg("visomatch")
    if not os.path.exists(vm.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "opencl-structure-from-motion_amd", "csrc")])
    return vm


def test_symbols_exported():
    vm = _vm()
    L = vm.lib()
    hdr = open(os.path.join(ROOT, "include", "visomatch.h")).read()
    for s in SYMBOLS:
        assert s in vm.EXPORTS and hasattr(L, s), s
        assert re.search(r"\b" + s + r"\s*\(", hdr), s


def test_constants_agree():
    vm = _vm()
    hdr = open(os.path.join(ROOT, "include", "visomatch.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (VSM_TRACKS_[A-Z_]+) (\d+)", hdr)}
    assert consts == {"VSM_TRACKS_WAVE_MAX": vm.TRACKS_WAVE_MAX, "VSM_TRACKS_BLOCK_MAX": vm.TRACKS_BLOCK_MAX}
    assert vm.TRACKS_WAVE_MAX == 64 and vm.TRACKS_BLOCK_MAX > vm.TRACKS_WAVE_MAX
    assert len(vm.TRACK_STATS) == 8 and len(vm.TRACK_TIMINGS) == 4


def test_kernels_in_the_profiling_table():
    vm = _vm()
    L = vm.lib()
    names = [L.vsm_kernel_name(i).decode() for i in range(L.vsm_num_kernels())]
    assert all(n for n in names)
    for k in ("k_trk_init", "k_trk_hook", "k_trk_flatten", "k_trk_keep", "k_trk_scan_reduce", "k_trk_scan_top", "k_trk_scan_apply",
              "k_trk_match_tracks", "k_trk_fill", "k_trk_order_wave", "k_trk_order_block"):
        assert names.count(k) == 1, k
