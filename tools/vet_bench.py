#!/usr/bin/env python3
"""Vetting of observations (vsm_points_vet) on tools/resect_bench.py's workload, the street scene (synth.road_*,
seed 1234): 200 mono frames 1242 x 375 resident in HBM, pairs (f-1, f) and (f-2, f) of every frame (397 pairs), flow matching,
default parameters.  The chain in front of the call: match_pairs, pair_tracks (side 0, min_length 2), pair_motions (bucketed,
2000 hypotheses), chain_poses, track_points.  Device and host results are compared first, every array by its bytes.  Then medians
and ranges of --reps calls after 3 warm-up calls of
  vet          vsm_points_vet with lists == NULL - gather, packing, upload, kernels, download, host part - and its split by
               vsm_vet_get_timings
  host         vsm_host_vet, one thread, on the same tracks, pixels (vsm_tracks_pixels, not timed) and points
  points       vsm_tracks_triangulate, the call in front
  resect       vsm_points_resect, the call behind
and the kernels' device time from the profiling table (a separate set of calls) with the bytes they read and write.  Prints one
JSON line.
  python tools/vet_bench.py [--frames 200] [--reps 20] [--points default|loose] [--max-residual 2.0]"""
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
FIELDS = ("code", "r2", "status", "n_in", "frame_lo", "frame_hi", "ss", "worst", "frame_counts", "kept_offsets", "kept_index")


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


def ms(ts):
    return {"median": round(statistics.median(ts) * 1e3, 3), "min": round(min(ts) * 1e3, 3), "max": round(max(ts) * 1e3, 3)}


def same(a, b):
    """bytes, with NaNs (r2 alone can hold them) compared by position"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind == "f":
        na, nb = np.isnan(a), np.isnan(b)
        return bool((na == nb).all()) and np.where(na, 0, a).tobytes() == np.where(nb, 0, b).tobytes()
    return a.tobytes() == b.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--max-residual", type=float, default=2.0)
    ap.add_argument("--points", choices=("default", "loose"), default="default",
                    help="the triangulation's parameters: the library's defaults, or every point that converges (point_type -1, max_dist 1e6, min_angle 0.001)")
    a = ap.parse_args()
    F = a.frames
    pyr = synth.road_pyramid(1234)
    frames = np.stack([synth.road_mono_frame(pyr, f, W, H) for f in range(F)])
    dl = torch.from_numpy(frames).to(torch.device("cuda:0"))
    pairs = pair_list(F)
    L = vm.lib()
    par = vm.vo_mono_params(F_PX, CU, CV, height=1.65, pitch=0.0, ransac_iters=a.iters)
    prm = vm.vet_params(max_residual=a.max_residual)
    rsp = vm.resect_params()
    tri = vm.triangulate_params(**(dict(point_type=-1, max_dist=1e6, min_angle=0.001) if a.points == "loose" else {}))

    m = vm.Matcher()
    m.match_pairs(dl, None, pairs, 0, fetch=False)
    tracks = m.pair_tracks()
    mot = m.pair_motions(par, bucket=True)
    poses, valid, posed = vm.chain_poses(F, pairs, mot.T, mot.rc)
    points = m.track_points(poses, F_PX, CU, CV, pose_valid=valid, params=tri)
    refine = np.ones(F, np.uint8)
    refine[0] = 0

    # ---- equal before anything is timed ----
    device = m.vet_points(poses, F_PX, CU, CV, pose_valid=valid, params=prm)
    fr, uv = m.track_pixels()
    use = np.ascontiguousarray(points.kept.astype(np.uint8))
    host = vm.host_vet(poses, F_PX, CU, CV, tracks.offsets, fr, uv, points.xyz, use=use, pose_valid=valid, params=prm)
    differ = [n for n in FIELDS if not same(getattr(device, n), getattr(host, n))]
    if differ:
        print(json.dumps({"error": "device and host results differ", "arrays": differ, "device": device.stats, "host": host.stats}))
        sys.exit(1)

    # ---- the calls alone: no result marshalling into numpy ----
    splits = []
    pp, pv, pr = (x.ctypes.data_as(C.c_void_p) for x in (poses, valid, refine))

    def device_call():
        rc = L.vsm_points_vet(m.h, None, None, pp, pv, F_PX, float(CU), float(CV), C.byref(prm))
        assert rc == 0, rc
        t = np.zeros(4)
        L.vsm_vet_get_timings(m.h, t.ctypes.data_as(C.c_void_p))
        splits.append(t)
    _, all_dev = timed(device_call, a.reps)
    split = np.stack(splits[-a.reps:])

    T, n_obs = len(tracks), len(fr)
    out = vm._vet_arrays(T, n_obs, F, n_obs)
    n_kept = C.c_int32(0)

    def host_call():
        got = L.vsm_host_vet(F, pp, pv, F_PX, float(CU), float(CV), T, vm._ptr(tracks.offsets), vm._ptr(fr), vm._ptr(uv), vm._ptr(points.xyz), vm._ptr(use), C.byref(prm),
                             *[vm._ptr(x) for x in out], C.byref(n_kept))
        assert got == T
    _, all_host = timed(host_call, a.reps)

    def points_call():
        assert L.vsm_tracks_triangulate(m.h, None, None, pp, pv, F_PX, float(CU), float(CV), C.byref(tri)) == 0
    _, all_points = timed(points_call, a.reps)

    def resect_call():
        assert L.vsm_points_resect(m.h, None, None, pp, pv, pr, F_PX, float(CU), float(CV), C.byref(rsp)) == 0
    _, all_resect = timed(resect_call, a.reps)

    # ---- device time of the kernels ----
    m.set_profiling(True)
    for _ in range(5):
        device_call()
    stats = m.kernel_stats()
    m.set_profiling(False)
    kernels = {k: {"us_per_call": round(t * 1e3 / 5, 1), "launches_per_call": n / 5} for k, (t, n) in stats.items() if (k.startswith("k_vet_") or k.startswith("k_trk_scan")) and n}
    m.close()
    n_in = int(device.stats["obs_inlier"])
    # k_vet_obs reads 12 bytes per observation, 36 per track (offsets, point, use, the next offset) and a frame's 97 where it is not
    # cached, writes 5 per observation and 44 per track (six results and the scan's item), and one atomic per counted observation;
    # k_vet_emit reads 1 byte per observation of a kept track, 12 per track, writes 4 per kept observation and 4 per track
    bytes_obs = 17 * n_obs + 80 * T + 4 * (n_in + int(device.stats["obs_behind"]) + int(device.stats["obs_gated"]))
    bytes_emit = n_obs + 16 * T + 4 * len(device.kept_index)
    for k, b in (("k_vet_obs", bytes_obs), ("k_vet_emit", bytes_emit)):
        if k in kernels:
            kernels[k]["bytes"] = b
            kernels[k]["gb_per_s"] = round(b / (kernels[k]["us_per_call"] * 1e-6) / 1e9, 1) if kernels[k]["us_per_call"] else None
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = None
    med = statistics.median
    print(json.dumps({
        "frames": F, "pairs": len(pairs), "points": a.points, "max_residual": a.max_residual, "commit": commit, "reps": a.reps, "results_equal": True,
        "frames_with_a_pose": int(posed), "tracks": T, "observations": n_obs, "points_kept": int(points.kept.sum()), "stats": device.stats,
        "kept_observations": int(len(device.kept_index)), "ss_inliers": float(device.ss.sum()), "ss_kept_tracks": float(device.ss[device.kept].sum()),
        "rms_inliers_px": round(float(np.sqrt(device.ss.sum() / max(n_in, 1))), 4),
        "ms": {"points_vet": ms(all_dev), "host_vet_one_thread": ms(all_host), "tracks_triangulate": ms(all_points), "points_resect": ms(all_resect)},
        "points_vet_split_us": {k: {"median": round(float(np.median(split[:, i])), 1), "min": round(float(split[:, i].min()), 1), "max": round(float(split[:, i].max()), 1)}
                                for i, k in enumerate(vm.VET_TIMINGS)},
        "host_over_device": round(med(all_host) / med(all_dev), 2), "vet_over_points": round(med(all_dev) / med(all_points), 2),
        "vet_over_resect": round(med(all_dev) / med(all_resect), 2), "kernels": kernels,
    }))


if __name__ == "__main__":
    main()
