#!/usr/bin/env python3
"""Feature tracks from the lists of a match_pairs call (vsm_pairs_tracks), on tools/pairs_bench.py's workload:
200 stereo frames 1242 x 375 resident in HBM (the flagship sequence, seed 1234), pairs (f-1, f) and (f-2, f) of every frame,
quad matching, default parameters.  Medians of --reps calls after a warm-up of
  pairs        Matcher.match_pairs(fetch=False), what produces the lists
  tracks       Matcher's vsm_pairs_tracks on them (side 0, min_length 2) - packing, upload, kernels, download, host part - and
               its split by vsm_tracks_get_timings
  host         vsm_host_tracks, one thread, on the same lists (fetched once, not timed)
and the device time per kernel from the profiling table (a separate set of calls: the event records slow the call).
Device and host results are compared byte for byte before anything is timed.  Prints one JSON line.
  python tools/tracks_bench.py [--frames 200] [--reps 20] [--chunk 110]"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

vm = importlib.import_module("opencl-structure-from-motion_amd.visomatch")
synth = importlib.import_module("opencl-structure-from-motion_amd.synth")
W, H, METHOD = 1242, 375, 2


def pair_list(n):
    return [(f - k, f) for f in range(1, n) for k in (1, 2) if f - k >= 0]


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=110, help="option pairs_chunk of the match_pairs call")
    a = ap.parse_args()
    F = a.frames
    seq = synth.stereo_sequence(1234, W, H, F)
    left, right = np.stack([l for l, _ in seq]), np.stack([r for _, r in seq])
    dev = torch.device("cuda:0")
    dl, dr = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    pairs = pair_list(F)
    P = len(pairs)
    L = vm.lib()

    m = vm.Matcher(options={"pairs_chunk": a.chunk})
    t_pairs, _ = timed(lambda: m.match_pairs(dl, dr, pairs, METHOD, fetch=False), max(5, a.reps // 4), warmup=1)
    lists = [m.pair_matches(k) for k in range(P)]

    # ---- equal before anything is timed ----
    device = m.pair_tracks()
    host = vm.host_tracks(F, pairs, lists)
    equal = (device.offsets.tobytes() == host.offsets.tobytes() and device.obs.tobytes() == host.obs.tobytes() and
             device.flags.tobytes() == host.flags.tobytes() and all(device.of_pair(k).tobytes() == host.of_pair(k).tobytes() for k in range(P)))
    if not equal:
        print(json.dumps({"error": "device and host tracks differ", "device_tracks": len(device), "host_tracks": len(host)}))
        sys.exit(1)

    # ---- the calls alone: no result marshalling into numpy ----
    splits = []

    def device_call():
        rc = L.vsm_pairs_tracks(m.h, 0, 2)
        assert rc == 0, rc
        t = np.zeros(4)
        L.vsm_tracks_get_timings(m.h, t.ctypes.data_as(C.c_void_p))
        splits.append(t)
    t_dev, all_dev = timed(device_call, a.reps)
    split = np.median(np.stack(splits[-a.reps:]), axis=0)

    pa, ls, ptrs, cnt = vm._track_inputs(pairs, lists)
    n_obs = C.c_int32(0)
    offsets, obs, flags = np.zeros(len(host) + 1, np.int32), np.zeros((len(host.obs), 4), np.int32), np.zeros(len(host), np.uint8)
    tom = np.zeros(int(cnt.sum()), np.int32)

    def host_call():
        T = L.vsm_host_tracks(F, pa.ctypes.data_as(C.c_void_p), P, ptrs, cnt.ctypes.data_as(C.c_void_p), 0, 2, offsets.ctypes.data_as(C.c_void_p),
                              obs.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p), tom.ctypes.data_as(C.c_void_p), C.byref(n_obs))
        assert T == len(host)
    t_host, all_host = timed(host_call, a.reps)

    # ---- device time per kernel ----
    m.set_profiling(True)
    for _ in range(5):
        device_call()
    kernels = {k: {"us_per_call": round(ms * 1e3 / 5, 1), "launches_per_call": n / 5} for k, (ms, n) in m.kernel_stats().items() if k.startswith("k_trk_") and n}
    m.set_profiling(False)
    m.close()
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = None
    seg = np.diff(device.offsets)
    print(json.dumps({
        "frames": F, "pairs": P, "method": METHOD, "commit": commit, "reps": a.reps, "results_equal": bool(equal),
        "stats": device.stats, "observations": int(len(device.obs)), "longest_track": int(seg.max()) if len(seg) else 0,
        "ms": {"pairs_run": round(t_pairs * 1e3, 3), "pairs_tracks": round(t_dev * 1e3, 3), "host_tracks_one_thread": round(t_host * 1e3, 3)},
        "pairs_tracks_split_us": dict(zip(vm.TRACK_TIMINGS, [round(float(x), 1) for x in split])),
        "pairs_tracks_ms_all": [round(t * 1e3, 3) for t in all_dev], "host_tracks_ms_all": [round(t * 1e3, 3) for t in all_host],
        "host_over_device": round(t_host / t_dev, 2), "tracks_over_pairs_run": round(t_dev / t_pairs, 3),
        "kernels": kernels, "kernels_us_sum": round(sum(k["us_per_call"] for k in kernels.values()), 1),
    }))


if __name__ == "__main__":
    main()
