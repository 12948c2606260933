#!/usr/bin/env python3
"""Re-observation of the points by projection (vsm_points_reobserve) on the street scene (synth.road_*, seed
1234): 200 mono frames 1242 x 375 resident in HBM, CONSECUTIVE pairs (f-1, f) only, flow matching, default parameters - so a
track ends where a match is missed, and the frames behind it are there to be found again.  The chain in front of the call:
match_pairs, pair_tracks (side 0, min_length 2), pair_motions (bucketed, 2000 hypotheses), chain_poses, track_points.  Device
and host results are compared first: every int, and every double by its bytes.  Medians and ranges of --reps calls after 3
warm-up calls of
  reobserve    vsm_points_reobserve - packing, upload, kernels with the wait for the number of candidates, download, host part -
               and its split by vsm_reobserve_get_timings
  host         vsm_host_reobserve, one thread, on the same tracks, points and the frames' feature records (fetched once, not timed)
and the kernels' device times from the profiling table (a separate set of calls).  Then what the new observations are worth:
the joint adjustment's rows and cost on the tracks as they were and on the extended ones, and - at the poses adjusted on the
extended set - the vetting's verdict on every new observation, with the histograms of best cost and of best / second for the
accepted candidates split by that verdict: the data from which a cap and a ratio can be chosen.  Prints one JSON line.
  python tools/reobserve_bench.py [--frames 200] [--reps 20] [--radius 4]"""
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
COST_EDGES = [0, 100, 200, 300, 400, 600, 800, 1200, 1600, 2400, 8161]
RATIO_EDGES = [0.0, 0.2, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0000001]


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
    ap.add_argument("--iters", type=int, default=2000, help="hypotheses of the pair motions in front of the call")
    ap.add_argument("--radius", type=float, default=4.0)
    a = ap.parse_args()
    F = a.frames
    pyr = synth.road_pyramid(1234)
    frames = np.stack([synth.road_mono_frame(pyr, f, W, H) for f in range(F)])
    dl = torch.from_numpy(frames).to(torch.device("cuda:0"))
    pairs = [(f - 1, f) for f in range(1, F)]
    L = vm.lib()
    par = vm.vo_mono_params(F_PX, CU, CV, height=1.65, pitch=0.0, ransac_iters=a.iters)
    prm = vm.reobserve_params(radius=a.radius)

    m = vm.Matcher()
    m.match_pairs(dl, None, pairs, 0, fetch=False)
    tracks = m.pair_tracks()
    mot = m.pair_motions(par, bucket=True)
    poses, valid, posed = vm.chain_poses(F, pairs, mot.T, mot.rc)
    points = m.track_points(poses, F_PX, CU, CV, pose_valid=valid)
    use = np.ascontiguousarray(points.kept.astype(np.uint8))
    feats = [m.pair_features(g) for g in range(F)]
    fo = np.cumsum([0] + [len(x) for x in feats]).astype(np.int32)
    feat = np.ascontiguousarray(np.vstack(feats))
    obs_frames, obs_feat = np.ascontiguousarray(tracks.obs[:, 0]), np.ascontiguousarray(tracks.obs[:, 1])

    # ---- equal before anything is timed ----
    device = m.reobserve_points(poses, F_PX, CU, CV, pose_valid=valid, params=prm)
    host = vm.host_reobserve(poses, F_PX, CU, CV, W, H, tracks.offsets, obs_frames, obs_feat, points.xyz, fo, feat, use=use, pose_valid=valid, params=prm)
    equal = all(np.ascontiguousarray(getattr(device, n)).tobytes() == np.ascontiguousarray(getattr(host, n)).tobytes() for n in vm.REOBSERVE_ARRAYS)
    if not equal or device.stats != host.stats:
        print(json.dumps({"error": "device and host results differ", "device": device.stats, "host": host.stats}))
        sys.exit(1)

    # ---- the calls alone: no result marshalling into numpy ----
    splits = []
    po, pv = np.ascontiguousarray(poses.reshape(F, -1)[:, :12]), np.ascontiguousarray(valid.astype(np.uint8))

    def device_call():
        rc = L.vsm_points_reobserve(m.h, vm._ptr(po), vm._ptr(pv), None, F_PX, float(CU), float(CV), C.byref(prm))
        assert rc == 0, rc
        t = np.zeros(4)
        L.vsm_reobserve_get_timings(m.h, vm._ptr(t))
        splits.append(t)
    t_dev, all_dev = timed(device_call, a.reps)
    split = np.median(np.stack(splits[-a.reps:]), axis=0)

    T, n = len(tracks), len(device)
    out = (np.zeros((n, 7), np.int32), np.zeros((n, 2)), np.zeros(T, np.int32), np.zeros((F, 2), np.int32), np.zeros(10, np.int64))

    def host_call():
        got = L.vsm_host_reobserve(F, vm._ptr(po), vm._ptr(pv), None, F_PX, float(CU), float(CV), W, H, T, vm._ptr(tracks.offsets), vm._ptr(obs_frames),
                                   vm._ptr(obs_feat), vm._ptr(points.xyz), vm._ptr(use), None, vm._ptr(fo), vm._ptr(feat), C.byref(prm), n, *[vm._ptr(x) for x in out])
        assert got == n
    t_host, all_host = timed(host_call, max(3, a.reps // 4), warmup=1)

    # ---- device time of the kernels ----
    m.set_profiling(True)
    for _ in range(5):
        device_call()
    kernels = {k: {"us_per_call": round(ms * 1e3 / 5, 1), "launches_per_call": n_ / 5} for k, (ms, n_) in m.kernel_stats().items()
               if (k.startswith("k_ro_") or k.startswith("k_trk_scan")) and n_}
    m.set_profiling(False)

    # ---- what the new observations are worth ----
    fr, uv = m.track_pixels()
    adj_prm = dict(max_residual=4.0)
    before = m.adjust(poses, F_PX, CU, CV, tracks.offsets, fr, uv, points.xyz, use=use, pose_valid=valid, params=adj_prm)
    off2, fr2, uv2, ft2 = device.extend(tracks.offsets, fr, uv, obs_feat)
    after = m.adjust(poses, F_PX, CU, CV, off2, fr2, uv2, points.xyz, use=use, pose_valid=valid, params=adj_prm)
    vet = m.vet(after.poses, F_PX, CU, CV, off2, fr2, uv2, after.xyz, use=use, pose_valid=valid)
    old = set(zip(np.repeat(np.arange(T), np.diff(tracks.offsets)).tolist(), fr.tolist()))
    per_obs = np.repeat(np.arange(T), np.diff(off2))
    code_of = {(int(t), int(g)): int(c) for t, g, c in zip(per_obs, fr2, vet.code) if (int(t), int(g)) not in old}
    acc = device.cand[device.accepted()]
    inlier = np.array([code_of[(int(r[0]), int(r[1]))] == 0 for r in acc], bool)
    ratio = np.where(acc[:, 4] > 0, acc[:, 3] / np.maximum(acc[:, 4], 1), np.where(acc[:, 4] == 0, 1.0, -1.0))  # (-1: no second)

    def hist(x, edges, mask):
        return np.histogram(x[mask], bins=edges)[0].tolist()

    m.close()
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = None
    cost = lambda r: None if not len(r.history) else round(float(r.history["cost_after"][-1]), 3)
    print(json.dumps({
        "frames": F, "pairs": len(pairs), "commit": commit, "reps": a.reps, "radius": a.radius, "results_equal": bool(equal), "frames_with_a_chained_pose": int(posed),
        "tracks": T, "observations": int(len(tracks.obs)), "points_kept": int(points.kept.sum()), "features": int(len(feat)), "candidates": n, "stats": device.stats,
        "candidate_block_mb": round(n * 44 / 1e6, 2),
        "ms": {"points_reobserve": round(t_dev * 1e3, 3), "points_reobserve_range": [round(min(all_dev) * 1e3, 3), round(max(all_dev) * 1e3, 3)],
               "host_reobserve_one_thread": round(t_host * 1e3, 3), "host_reobserve_range": [round(min(all_host) * 1e3, 3), round(max(all_host) * 1e3, 3)]},
        "points_reobserve_split_us": dict(zip(vm.REOBSERVE_TIMINGS, [round(float(x), 1) for x in split])),
        "points_reobserve_ms_all": [round(t * 1e3, 3) for t in all_dev], "host_over_device": round(t_host / t_dev, 2), "kernels": kernels,
        "new_observations": {"accepted": int(len(acc)), "inliers_at_adjusted_poses": int(inlier.sum()), "vet_codes": np.bincount(list(code_of.values()), minlength=5).tolist(),
                             "no_second": {"inlier": int(((acc[:, 4] < 0) & inlier).sum()), "outlier": int(((acc[:, 4] < 0) & ~inlier).sum())}},
        "best_cost_hist": {"edges": COST_EDGES, "inlier": hist(acc[:, 3], COST_EDGES, inlier), "outlier": hist(acc[:, 3], COST_EDGES, ~inlier)},
        "best_over_second_hist": {"edges": RATIO_EDGES, "inlier": hist(ratio, RATIO_EDGES, inlier & (ratio >= 0)), "outlier": hist(ratio, RATIO_EDGES, ~inlier & (ratio >= 0))},
        "adjust": {"rows_before": int(before.rows.sum()), "rows_after": int(after.rows.sum()), "first_cost": [round(float(r.history["cost_before"][0]), 3) if len(r.history) else None for r in (before, after)], "last_cost": [cost(before), cost(after)],
                   "rounds": [len(before.history), len(after.history)], "ms": [round(sum(before.timings.values()) / 1e3, 2), round(sum(after.timings.values()) / 1e3, 2)]},
    }))


if __name__ == "__main__":
    main()
