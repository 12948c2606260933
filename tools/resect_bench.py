#!/usr/bin/env python3
"""Pose refinement (vsm_points_resect) on tools/motions_bench.py's workload, the street scene (synth.road_*, seed
1234), whose images do carry a geometry: 200 mono frames 1242 x 375 resident in HBM, pairs (f-1, f) and (f-2, f) of every frame
(397 pairs), flow matching, default parameters.  The chain in front of the call: match_pairs, pair_tracks (side 0, min_length
2), pair_motions (bucketed, 2000 hypotheses), chain_poses, track_points; the first frame is pinned (refine = 0).  Medians of
--reps calls after a warm-up of
  resect       vsm_points_resect with lists == NULL - gather, grouping, upload, kernel, download, host part - and its split
               by vsm_resect_get_timings
  host         vsm_host_resect, one thread, on the same tracks, pixels and points (gathered once, not timed)
and the kernel's device time from the profiling table (a separate set of calls).  Device and host results are compared first:
every int, and every double by its bytes.  Prints one JSON line.
  python tools/resect_bench.py [--frames 200] [--reps 20] [--min-observations 10] [--points default|loose]"""
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
FIELDS = ("status", "updates", "rows", "used", "poses", "ss_before", "ss_after", "rms_before", "rms_after")


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
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--min-observations", type=int, default=10)
    ap.add_argument("--points", choices=("default", "loose"), default="default",
                    help="the triangulation's parameters: the library's defaults, or every point that converges (point_type -1, max_dist 1e6, min_angle 0.001)")
    a = ap.parse_args()
    F = a.frames
    pyr = synth.road_pyramid(1234)
    frames = np.stack([synth.road_mono_frame(pyr, f, W, H) for f in range(F)])
    dl = torch.from_numpy(frames).to(torch.device("cuda:0"))
    pairs = pair_list(F)
    P = len(pairs)
    L = vm.lib()
    par = vm.vo_mono_params(F_PX, CU, CV, height=1.65, pitch=0.0, ransac_iters=a.iters)
    prm = vm.resect_params(min_observations=a.min_observations)
    tri = vm.triangulate_params(**(dict(point_type=-1, max_dist=1e6, min_angle=0.001) if a.points == "loose" else {}))

    m = vm.Matcher()
    t_pairs, _ = timed(lambda: m.match_pairs(dl, None, pairs, 0, fetch=False), 3, warmup=1)
    tracks = m.pair_tracks()
    lists = [m.pair_matches(k) for k in range(P)]
    mot = m.pair_motions(par, bucket=True)
    poses, valid, posed = vm.chain_poses(F, pairs, mot.T, mot.rc)
    t_points, _ = timed(lambda: m.track_points(poses, F_PX, CU, CV, pose_valid=valid, params=tri), max(5, a.reps // 4), warmup=1)
    points = m.track_points(poses, F_PX, CU, CV, pose_valid=valid, params=tri)
    refine = np.ones(F, np.uint8)
    refine[0] = 0

    # ---- equal before anything is timed ----
    device = m.resect_points(poses, F_PX, CU, CV, refine=refine, pose_valid=valid, params=prm)
    uv = np.zeros((len(tracks.obs), 2), np.float32)
    for k in range(P):  # the pixels, gathered here: observation rows of pair k, end 0 / 1
        rows = np.nonzero(tracks.obs[:, 2] == k)[0]
        code = tracks.obs[rows, 3]
        mt = lists[k][code >> 1]
        uv[rows, 0] = np.where(code & 1, mt["u1c"], mt["u1p"])
        uv[rows, 1] = np.where(code & 1, mt["v1c"], mt["v1p"])
    fr = np.ascontiguousarray(tracks.obs[:, 0])
    use = np.ascontiguousarray(points.kept.astype(np.uint8))
    host = vm.host_resect(poses, F_PX, CU, CV, tracks.offsets, fr, uv, points.xyz, use=use, refine=refine, pose_valid=valid, params=prm)
    equal = all(np.ascontiguousarray(getattr(device, n)).tobytes() == np.ascontiguousarray(getattr(host, n)).tobytes() for n in FIELDS)
    if not equal:
        print(json.dumps({"error": "device and host poses differ", "device": device.stats, "host": np.bincount(host.status, minlength=7).tolist()}))
        sys.exit(1)

    # ---- the calls alone: no result marshalling into numpy ----
    splits = []
    pp, pv, pr = (x.ctypes.data_as(C.c_void_p) for x in (poses, valid, refine))

    def device_call():
        rc = L.vsm_points_resect(m.h, None, None, pp, pv, pr, F_PX, float(CU), float(CV), C.byref(prm))
        assert rc == 0, rc
        t = np.zeros(4)
        L.vsm_resect_get_timings(m.h, t.ctypes.data_as(C.c_void_p))
        splits.append(t)
    t_dev, all_dev = timed(device_call, a.reps)
    split = np.median(np.stack(splits[-a.reps:]), axis=0)

    T = len(tracks)
    out = vm._resect_arrays(F)

    def host_call():
        got = L.vsm_host_resect(F, pp, pv, pr, F_PX, float(CU), float(CV), T, tracks.offsets.ctypes.data_as(C.c_void_p), fr.ctypes.data_as(C.c_void_p),
                                uv.ctypes.data_as(C.c_void_p), points.xyz.ctypes.data_as(C.c_void_p), use.ctypes.data_as(C.c_void_p), C.byref(prm),
                                *[x.ctypes.data_as(C.c_void_p) for x in out])
        assert got == F
    t_host, all_host = timed(host_call, max(3, a.reps // 5), warmup=1)

    # ---- device time of the kernel ----
    m.set_profiling(True)
    for _ in range(5):
        device_call()
    kernels = {k: {"us_per_call": round(ms * 1e3 / 5, 1), "launches_per_call": n / 5} for k, (ms, n) in m.kernel_stats().items() if k.startswith("k_rs_") and n}
    m.set_profiling(False)
    m.close()
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = None
    work = device.updates > 0
    print(json.dumps({
        "frames": F, "pairs": P, "points": a.points, "commit": commit, "reps": a.reps, "results_equal": bool(equal), "frames_with_a_pose": int(posed),
        "tracks": T, "observations": int(len(tracks.obs)), "points_kept": int(points.kept.sum()), "rows": int(device.rows.sum()),
        "rows_per_frame_max": int(device.rows.max()), "rows_per_frame_median": float(np.median(device.rows)), "frames_by_status": device.stats,
        "updates_mean": round(float(device.updates[work].mean()), 2) if work.any() else 0, "updates_max": int(device.updates.max()),
        "ss_before": float(device.ss_before.sum()), "ss_after": float(device.ss_after.sum()),
        "ms": {"pairs_run": round(t_pairs * 1e3, 3), "tracks_triangulate": round(t_points * 1e3, 3), "points_resect": round(t_dev * 1e3, 3),
               "host_resect_one_thread": round(t_host * 1e3, 3)},
        "points_resect_split_us": dict(zip(vm.RESECT_TIMINGS, [round(float(x), 1) for x in split])),
        "points_resect_ms_all": [round(t * 1e3, 3) for t in all_dev], "host_resect_ms_all": [round(t * 1e3, 3) for t in all_host],
        "host_over_device": round(t_host / t_dev, 2), "kernels": kernels,
    }))


if __name__ == "__main__":
    main()
