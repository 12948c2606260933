#!/usr/bin/env python3
"""Joint adjustment of poses and points (vsm_points_adjust) on tools/resect_bench.py's workload, the street scene
(synth.road_*, seed 1234): 200 mono frames 1242 x 375 resident in HBM, pairs (f-1, f) and (f-2, f) of every frame (397 pairs),
flow matching, default parameters.  The chain in front of the call: match_pairs, pair_tracks (side 0, min_length 2),
pair_motions (bucketed, 2000 hypotheses), chain_poses, track_points, resect_points, vet_points; the first frame is pinned
(refine = 0); the adjustment and the alternation both start from the chained poses.  Medians of --reps calls after a warm-up of
  adjust       vsm_points_adjust with lists == NULL - gather, grouping, upload, the rounds' kernels with a wait per round,
               download, host part - and its split by vsm_adjust_get_timings; the same with every launch enqueued at once
               (option adjust_fixed)
  host         vsm_host_adjust, one thread, on the same tracks, pixels and points (gathered once, not timed)
  alternate    Matcher.alternate at the same round count (track_points + resect_points per round), and its final cost
and the kernels' device time from the profiling table (a separate set of calls).  Device and host results are compared first:
every int, and every double by its bytes.  Prints one JSON line.
  python tools/ba_bench.py [--frames 200] [--reps 10] [--rounds 5] [--cg-iters 40] [--max-residual 4] [--ftol 1e-6]"""
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
W, H = 1242, 375
F_PX, CU, CV = float(synth.ROAD_F), W // 2, (H * 2) // 5
FIELDS = ("frame_status", "poses", "rows", "active", "track_status", "xyz", "history")


def pair_list(n):
    return [(f - k, f) for f in range(1, n) for k in (1, 2) if f - k >= 0]


def timed(fn, reps, warmup=2):
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cg-iters", type=int, default=40)
    ap.add_argument("--max-residual", type=float, default=4.0)
    ap.add_argument("--min-observations", type=int, default=10)
    ap.add_argument("--ftol", type=float, default=1e-6, help="a larger value stops the call early: what the wait per round is for")
    a = ap.parse_args()
    F = a.frames
    pyr = synth.road_pyramid(1234)
    frames = np.stack([synth.road_mono_frame(pyr, f, W, H) for f in range(F)])
    dl = torch.from_numpy(frames).to(torch.device("cuda:0"))
    pairs = pair_list(F)
    P = len(pairs)
    L = vm.lib()
    par = vm.vo_mono_params(F_PX, CU, CV, height=1.65, pitch=0.0, ransac_iters=a.iters)
    prm = vm.adjust_params(min_observations=a.min_observations, max_rounds=a.rounds, cg_iters=a.cg_iters, max_residual=a.max_residual, ftol=a.ftol)
    rs_prm = dict(min_observations=a.min_observations, max_residual=a.max_residual)

    m = vm.Matcher()
    m.match_pairs(dl, None, pairs, 0, fetch=False)
    tracks = m.pair_tracks()
    lists = [m.pair_matches(k) for k in range(P)]
    mot = m.pair_motions(par, bucket=True)
    poses, valid, posed = vm.chain_poses(F, pairs, mot.T, mot.rc)
    points = m.track_points(poses, F_PX, CU, CV, pose_valid=valid)
    refine = np.ones(F, np.uint8)
    refine[0] = 0
    m.resect_points(poses, F_PX, CU, CV, refine=refine, pose_valid=valid, params=rs_prm)
    m.vet_points(poses, F_PX, CU, CV, pose_valid=valid)

    # ---- equal before anything is timed ----
    device = m.adjust_points(poses, F_PX, CU, CV, refine=refine, pose_valid=valid, params=prm)
    fr, uv = m.track_pixels()
    use = np.ascontiguousarray(points.kept.astype(np.uint8))
    host = vm.host_adjust(poses, F_PX, CU, CV, tracks.offsets, fr, uv, points.xyz, use=use, refine=refine, pose_valid=valid, params=prm)
    equal = all(np.ascontiguousarray(getattr(device, n)).tobytes() == np.ascontiguousarray(getattr(host, n)).tobytes() for n in FIELDS)
    if not equal:
        print(json.dumps({"error": "device and host results differ", "device": device.stats, "host": host.stats}))
        sys.exit(1)

    # ---- the calls alone: no result marshalling into numpy ----
    splits = []
    pp, pv, pr = (x.ctypes.data_as(C.c_void_p) for x in (poses, valid, refine))

    def device_call():
        rc = L.vsm_points_adjust(m.h, None, None, pp, pv, pr, F_PX, float(CU), float(CV), C.byref(prm))
        assert rc == 0, rc
        t = np.zeros(4)
        L.vsm_adjust_get_timings(m.h, t.ctypes.data_as(C.c_void_p))
        splits.append(t)
    t_dev, all_dev = timed(device_call, a.reps)
    split = np.median(np.stack(splits[-a.reps:]), axis=0)
    m.set_option("adjust_fixed", 1)
    fixed = m.adjust_points(poses, F_PX, CU, CV, refine=refine, pose_valid=valid, params=prm)
    fixed_equal = all(np.ascontiguousarray(getattr(device, n)).tobytes() == np.ascontiguousarray(getattr(fixed, n)).tobytes() for n in FIELDS)
    t_fixed, _ = timed(device_call, a.reps)
    split_fixed = np.median(np.stack(splits[-a.reps:]), axis=0)
    m.set_option("adjust_fixed", 0)

    T = len(tracks)
    fa, ta, ha = vm._adjust_arrays(F, T, a.rounds)
    n_rounds, stats = C.c_int32(0), np.zeros(16, np.int64)

    def host_call():
        got = L.vsm_host_adjust(F, pp, pv, pr, F_PX, float(CU), float(CV), T, tracks.offsets.ctypes.data_as(C.c_void_p), fr.ctypes.data_as(C.c_void_p),
                                uv.ctypes.data_as(C.c_void_p), points.xyz.ctypes.data_as(C.c_void_p), use.ctypes.data_as(C.c_void_p), C.byref(prm),
                                *[x.ctypes.data_as(C.c_void_p) for x in fa + ta + ha], C.byref(n_rounds), stats.ctypes.data_as(C.c_void_p))
        assert got == F
    t_host, all_host = timed(host_call, max(3, a.reps // 3), warmup=1)

    # ---- the alternation at the same round count (it replaces the point result: last) ----
    # ---- device time of the kernels first ----
    m.set_profiling(True)
    for _ in range(3):
        device_call()
    kernels = {k: {"us_per_call": round(ms * 1e3 / 3, 1), "launches_per_call": n / 3} for k, (ms, n) in m.kernel_stats().items() if k.startswith("k_ba_") and n}
    m.set_profiling(False)
    alt = {}

    def alternate_call():
        alt["poses"], alt["points"], alt["history"] = m.alternate(poses, F_PX, CU, CV, len(device.history), refine=refine, resect_params=rs_prm, pose_valid=valid)
    t_alt, all_alt = timed(alternate_call, max(3, a.reps // 3), warmup=1)
    # the alternation's final state under the adjustment's own cost: one round's linearisation there
    at_alt = vm.host_adjust(alt["poses"], F_PX, CU, CV, tracks.offsets, fr, uv, alt["points"].xyz, use=np.ascontiguousarray(alt["points"].kept.astype(np.uint8)),
                            refine=refine, pose_valid=valid, params=dict(max_rounds=1, max_residual=a.max_residual, min_observations=a.min_observations))
    m.close()
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = None
    kernel_us = sum(k["us_per_call"] for k in kernels.values())
    h = device.history
    print(json.dumps({
        "frames": F, "pairs": P, "commit": commit, "reps": a.reps, "results_equal": bool(equal), "fixed_schedule_equal": bool(fixed_equal), "frames_with_a_pose": int(posed),
        "tracks": T, "observations": int(len(tracks.obs)), "points_kept": int(points.kept.sum()), "rows": int(device.rows.sum()),
        "params": {n: getattr(prm, n) for n, _ in vm.VsmAdjustParams._fields_}, "stats": device.stats,
        "history": {n: h[n].tolist() for n in h.dtype.names},
        "ms": {"points_adjust": round(t_dev * 1e3, 3), "points_adjust_fixed_schedule": round(t_fixed * 1e3, 3), "host_adjust_one_thread": round(t_host * 1e3, 3),
               "alternate_same_rounds": round(t_alt * 1e3, 3)},
        "points_adjust_split_us": dict(zip(vm.ADJUST_TIMINGS, [round(float(x), 1) for x in split])),
        "points_adjust_fixed_split_us": dict(zip(vm.ADJUST_TIMINGS, [round(float(x), 1) for x in split_fixed])),
        "kernels_device_us": round(kernel_us, 1), "launches_per_call": sum(k["launches_per_call"] for k in kernels.values()),
        "kernel_share_of_kernels_span": round(kernel_us / max(float(split[2]), 1e-9), 3),
        "copy_share_of_call": round(float(split[1] + split[3]) / max(t_dev * 1e6, 1e-9), 3),
        "cost": {"start": float(h["cost_before"][0]), "adjust": device.cost, "active_rows": int(h["active"][-1]),
                 "alternate_resect_ss_after": alt["history"][-1][1], "alternate_under_the_adjustment_cost": float(at_alt.history["cost_before"][0]),
                 "alternate_active_rows": int(at_alt.history["active"][0])},
        "points_adjust_ms_all": [round(t * 1e3, 3) for t in all_dev], "host_adjust_ms_all": [round(t * 1e3, 3) for t in all_host],
        "alternate_ms_all": [round(t * 1e3, 3) for t in all_alt], "host_over_device": round(t_host / t_dev, 2), "kernels": kernels,
    }))


if __name__ == "__main__":
    main()
