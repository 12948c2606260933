"""ctypes binding of libvisomatch.so (include/visomatch.h) -- the Python mirror of the
reference's `class Matcher` (viso/matcher.h:37-136): pushBack / matchFeatures / getMatches /
bucketFeatures / getGain / setIntrinsics, plus the stage-level views the parity tests use.

The library is the HIP build for gfx950; there is no CPU path.  Importing works anywhere (the
CPU test-suite checks the exported symbols), creating a Matcher needs a GPU and raises otherwise.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# The look-ahead path uses four streams (the handle's and three side streams the Delaunay chains rotate over).  The HIP
# runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4: two of ours would share one and serialise), and
# with SIX or more hardware queues in a process every kernel's workgroup dispatch runs at a half or a quarter of its rate
# (DESIGN_HISTORY.md 6c), so: five - ours and the null stream's.  Read when the runtime initialises, so it only helps if nothing in
# this process has touched the GPU yet.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "5")
LIB_PATH = os.environ.get("VSM_LIB_PATH") or os.path.join(HERE, "libvisomatch.so")  # override: kernel experiments

P_MATCH = np.dtype(
    [("u1p", "<f4"), ("v1p", "<f4"), ("i1p", "<i4"), ("u2p", "<f4"), ("v2p", "<f4"), ("i2p", "<i4"),
     ("u1c", "<f4"), ("v1c", "<f4"), ("i1c", "<i4"), ("u2c", "<f4"), ("v2c", "<f4"), ("i2c", "<i4")])
assert P_MATCH.itemsize == 48

INT_PARAMS = ["nms_n", "nms_tau", "match_binsize", "match_radius", "match_disp_tolerance",
              "outlier_disp_tolerance", "outlier_flow_tolerance", "multi_stage", "half_resolution", "refinement"]
# include/visomatch.h: the longest track segment a wave / a workgroup puts into order (longer ones: the host)
TRACKS_WAVE_MAX = 64
TRACKS_BLOCK_MAX = 2048
FEATURE_SETS = {"1p1": 0, "2p1": 1, "1c1": 2, "2c1": 3, "1p2": 4, "2p2": 5, "1c2": 6, "2c2": 7}

# every symbol include/visomatch.h declares
EXPORTS = ["vsm_default_params", "vsm_create", "vsm_destroy", "vsm_set_intrinsics", "vsm_push_back",
           "vsm_push_back_device", "vsm_wait_for_stream", "vsm_match", "vsm_num_matches", "vsm_get_matches", "vsm_bucket", "vsm_gain",
           "vsm_num_features", "vsm_get_features", "vsm_set_stage_capture", "vsm_stage_size", "vsm_stage_get",
           "vsm_num_ranges", "vsm_get_ranges", "vsm_get_gradients", "vsm_get_filter_responses", "vsm_get_counters",
           "vsm_get_timings", "vsm_set_profiling", "vsm_num_kernels", "vsm_kernel_name", "vsm_get_kernel_stats",
           "vsm_host_delaunay", "vsm_host_delaunay_split", "vsm_debug_delaunay_gpu", "vsm_debug_dc_bench", "vsm_host_ties", "vsm_debug_ties_gpu", "vsm_host_outliers_and_prior", "vsm_host_outliers_and_prior_threads", "vsm_debug_dc2", "vsm_debug_dc2_band_factor", "vsm_debug_predicates", "vsm_debug_ctx_layout", "vsm_debug_dc2_layout", "vsm_debug_seq_plan", "vsm_debug_chunk_jobs", "vsm_debug_pair_jobs", "vsm_debug_refine", "vsm_debug_refine_check", "vsm_debug_parabolic_apply", "vsm_host_parabolic_fits", "vsm_debug_compact_keys", "vsm_local_cpus", "vsm_forkjoin_cpus", "vsm_device_pool_stats", "vsm_device_pool_trim", "vsm_sequence_run", "vsm_sequence_num_matches", "vsm_sequence_get_matches",
           "vsm_sequence_get_timings", "vsm_sequence_path", "vsm_pairs_run", "vsm_pairs_num_matches", "vsm_pairs_get_matches", "vsm_pairs_get_timings",
           "vsm_tracks_run", "vsm_pairs_tracks", "vsm_tracks_count", "vsm_tracks_num_obs", "vsm_tracks_get", "vsm_tracks_of_matches",
           "vsm_tracks_get_stats", "vsm_tracks_get_timings", "vsm_host_tracks",
           "vsm_triangulate_default_params", "vsm_triangulate_run", "vsm_tracks_triangulate", "vsm_points_count", "vsm_points_get",
           "vsm_points_get_stats", "vsm_points_get_timings", "vsm_host_triangulate",
           "vsm_resect_default_params", "vsm_resect_run", "vsm_points_resect", "vsm_resect_count", "vsm_resect_get", "vsm_resect_get_stats",
           "vsm_resect_get_timings", "vsm_host_resect",
           "vsm_vet_default_params", "vsm_vet_run", "vsm_points_vet", "vsm_vet_count", "vsm_vet_get_obs", "vsm_vet_get_tracks", "vsm_vet_get_frames",
           "vsm_vet_get_kept", "vsm_vet_get_stats", "vsm_vet_get_timings", "vsm_host_vet", "vsm_tracks_pixels",
           "vsm_adjust_default_params", "vsm_adjust_run", "vsm_points_adjust", "vsm_adjust_count", "vsm_adjust_get_frames", "vsm_adjust_get_tracks",
           "vsm_adjust_get_history", "vsm_adjust_get_stats", "vsm_adjust_get_timings", "vsm_host_adjust",
           "vsm_locate_default_params", "vsm_locate_run", "vsm_points_locate", "vsm_locate_count", "vsm_locate_get", "vsm_locate_get_stats",
           "vsm_locate_get_timings", "vsm_host_locate", "vsm_host_locate_sample", "vsm_host_locate_fit", "vsm_host_locate_count",
           "vsm_debug_locate_fit", "vsm_debug_locate_count", "vsm_debug_locate_winner", "vsm_debug_locate_hypotheses",
           "vsm_reobserve_default_params", "vsm_reobserve_run", "vsm_points_reobserve", "vsm_reobserve_count", "vsm_reobserve_get", "vsm_reobserve_get_tracks",
           "vsm_reobserve_get_frames", "vsm_reobserve_get_stats", "vsm_reobserve_get_timings", "vsm_host_reobserve", "vsm_pairs_num_features",
           "vsm_pairs_get_features",
           "vsm_fuse_default_params", "vsm_fuse_run", "vsm_points_fuse", "vsm_fuse_count", "vsm_fuse_get", "vsm_fuse_get_tracks", "vsm_fuse_get_merged",
           "vsm_fuse_get_frames", "vsm_fuse_get_stats", "vsm_fuse_get_timings", "vsm_host_fuse", "vsm_set_option", "vsm_version", "vsm_host_register", "vsm_host_unregister",
           "vsm_multi_create", "vsm_multi_destroy", "vsm_multi_process", "vsm_multi_num_sequences", "vsm_multi_get_motion",
           "vsm_multi_motion_valid", "vsm_multi_num_matches", "vsm_multi_get_matches", "vsm_multi_num_inliers", "vsm_multi_get_inliers",
           "vsm_multi_get_timings",
           "vsm_vo_stereo_default_params", "vsm_vo_stereo_create", "vsm_vo_stereo_destroy", "vsm_vo_stereo_process",
           "vsm_vo_stereo_process_device", "vsm_vo_stereo_process_matches", "vsm_vo_stereo_get_motion",
           "vsm_vo_stereo_motion_valid", "vsm_vo_stereo_num_matches", "vsm_vo_stereo_get_matches",
           "vsm_vo_stereo_num_inliers", "vsm_vo_stereo_get_inliers", "vsm_vo_stereo_gain", "vsm_vo_stereo_matcher",
           "vsm_vo_stereo_get_timings", "vsm_vo_sampler_seed", "vsm_host_estimate_motion_stereo",
           "vsm_vo_mono_default_params", "vsm_vo_mono_create", "vsm_vo_mono_destroy", "vsm_vo_mono_process",
           "vsm_vo_mono_process_device", "vsm_vo_mono_process_matches", "vsm_vo_mono_get_motion",
           "vsm_vo_mono_motion_valid", "vsm_vo_mono_num_matches", "vsm_vo_mono_get_matches", "vsm_vo_mono_num_inliers",
           "vsm_vo_mono_get_inliers", "vsm_vo_mono_gain", "vsm_vo_mono_matcher", "vsm_vo_mono_get_timings",
           "vsm_vo_mono_device_svd", "vsm_vo_mono_device_stages",
           "vsm_debug_mono_fit", "vsm_debug_mono_count", "vsm_debug_mono_triangulate", "vsm_debug_mono_vote",
           "vsm_host_estimate_motion_mono",
           "vsm_motions_run", "vsm_pairs_motions", "vsm_motions_count", "vsm_motions_get", "vsm_motions_inliers", "vsm_motions_matches",
           "vsm_motions_get_stats", "vsm_motions_get_timings", "vsm_motions_device_svd", "vsm_host_pairs_motions", "vsm_chain_poses"]


class VsmParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in INT_PARAMS] + [(n, C.c_double) for n in ("f", "cu", "cv", "base")]


class VsmVoStereoParams(C.Structure):
    _fields_ = [("match", VsmParams), ("bucket_max_features", C.c_int32), ("bucket_width", C.c_double),
                ("bucket_height", C.c_double), ("f", C.c_double), ("cu", C.c_double), ("cv", C.c_double),
                ("base", C.c_double), ("ransac_iters", C.c_int32), ("inlier_threshold", C.c_double),
                ("reweighting", C.c_int32)]


class VsmVoMonoParams(C.Structure):
    _fields_ = [("match", VsmParams), ("bucket_max_features", C.c_int32), ("bucket_width", C.c_double),
                ("bucket_height", C.c_double), ("f", C.c_double), ("cu", C.c_double), ("cv", C.c_double),
                ("height", C.c_double), ("pitch", C.c_double), ("ransac_iters", C.c_int32),
                ("inlier_threshold", C.c_double), ("motion_threshold", C.c_double)]


class VsmTriangulateParams(C.Structure):
    _fields_ = [("point_type", C.c_int32), ("min_track_length", C.c_int32), ("max_dist", C.c_double), ("min_angle", C.c_double),
                ("cam_pitch", C.c_double), ("cam_height", C.c_double)]


class VsmResectParams(C.Structure):
    _fields_ = [("min_observations", C.c_int32), ("max_updates", C.c_int32), ("eps", C.c_double), ("max_residual", C.c_double), ("min_depth", C.c_double)]


class VsmVetParams(C.Structure):
    _fields_ = [("max_residual", C.c_double), ("min_depth", C.c_double), ("min_observations", C.c_int32)]


class VsmAdjustParams(C.Structure):
    _fields_ = [("min_observations", C.c_int32), ("min_track_observations", C.c_int32), ("max_rounds", C.c_int32), ("cg_iters", C.c_int32),
                ("lambda0", C.c_double), ("lambda_min", C.c_double), ("lambda_max", C.c_double), ("cg_tol", C.c_double), ("ftol", C.c_double),
                ("max_residual", C.c_double), ("min_depth", C.c_double)]


class VsmLocateParams(C.Structure):
    _fields_ = [("ransac_iters", C.c_int32), ("inlier_threshold", C.c_double), ("min_inliers", C.c_int32), ("min_depth", C.c_double), ("seed", C.c_uint32),
                ("max_updates", C.c_int32), ("eps", C.c_double)]


class VsmReobserveParams(C.Structure):
    _fields_ = [("radius", C.c_double), ("min_depth", C.c_double), ("max_cost", C.c_int32), ("ratio_num", C.c_int32), ("ratio_den", C.c_int32)]


class VsmFuseParams(C.Structure):
    _fields_ = [("radius", C.c_double), ("min_depth", C.c_double), ("max_cost", C.c_int32), ("ratio_num", C.c_int32), ("ratio_den", C.c_int32)]


def host_register(arr):
    """page-lock a (contiguous) numpy array for DMA (vsm_host_register = hipHostRegister); True on success.  Pair with
    Matcher.set_option("seq_host_pinned", 1) and host_unregister(arr) before the array is freed."""
    assert arr.flags["C_CONTIGUOUS"]
    return lib().vsm_host_register(arr.ctypes.data_as(C.c_void_p), arr.nbytes) == 0


def host_unregister(arr):
    return lib().vsm_host_unregister(arr.ctypes.data_as(C.c_void_p)) == 0


def device_pool_stats():
    """(blocks in the cache, their bytes, large blocks in use): the device memory closed handles left for the next one"""
    out = (C.c_int64 * 3)()
    lib().vsm_device_pool_stats(out)
    return int(out[0]), int(out[1]), int(out[2])


def device_pool_trim():
    lib().vsm_device_pool_trim()


class VisoMatchError(RuntimeError):
    pass


_RC_NAMES = {-2: " (VSM_ENOTREADY)", -4: " (VSM_EARG)"}  # include/visomatch.h


def _check(rc, what):
    """a library call's return value: an error code (negative) raises VisoMatchError, anything else is handed on"""
    if rc < 0:
        raise VisoMatchError(f"{what} failed with {rc}" + _RC_NAMES.get(rc, ""))
    return rc


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VisoMatchError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        # PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME as /opt/rocm's).  Two HIP
        # runtimes in one process cannot both own the GPU, so when torch is installed let it load
        # its runtime first; libvisomatch.so then binds to that copy.
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch-less environments use /opt/rocm's runtime
            pass
        L = C.CDLL(LIB_PATH)
        vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
        L.vsm_version.restype = C.c_char_p
        L.vsm_default_params.argtypes = [C.POINTER(VsmParams)]
        L.vsm_create.restype = vp
        L.vsm_create.argtypes = [C.POINTER(VsmParams)]
        L.vsm_destroy.argtypes = [vp]
        L.vsm_set_intrinsics.argtypes = [vp] + [C.c_double] * 4
        L.vsm_push_back.argtypes = [vp, vp, vp, i32, i32, i32, C.c_int]
        L.vsm_push_back_device.argtypes = [vp, vp, vp, i32, i32, i32, C.c_int]
        L.vsm_wait_for_stream.argtypes = [vp, vp]
        L.vsm_match.argtypes = [vp, i32, vp]
        L.vsm_num_matches.argtypes = [vp]
        L.vsm_get_matches.argtypes = [vp, vp, i32]
        L.vsm_bucket.argtypes = [vp, i32, f32, f32]
        L.vsm_gain.argtypes = [vp, vp, i32]
        L.vsm_gain.restype = f32
        L.vsm_num_features.argtypes = [vp, i32]
        L.vsm_get_features.argtypes = [vp, i32, vp, i32]
        L.vsm_set_stage_capture.argtypes = [vp, C.c_int]
        L.vsm_stage_size.argtypes = [vp, i32]
        L.vsm_stage_get.argtypes = [vp, i32, vp, i32]
        L.vsm_num_ranges.argtypes = [vp]
        L.vsm_get_ranges.argtypes = [vp, vp, i32]
        L.vsm_get_gradients.argtypes = [vp, i32, i32, vp, vp]
        L.vsm_get_filter_responses.argtypes = [vp, vp, vp]
        L.vsm_get_counters.argtypes = [vp, vp]
        L.vsm_get_timings.argtypes = [vp, vp]
        L.vsm_set_profiling.argtypes = [vp, C.c_int]
        L.vsm_kernel_name.restype = C.c_char_p
        L.vsm_kernel_name.argtypes = [i32]
        L.vsm_get_kernel_stats.argtypes = [vp, vp, vp]
        L.vsm_host_delaunay.argtypes = [vp, vp, i32, vp, i32, i32]
        L.vsm_host_delaunay_split.argtypes = [vp, vp, i32, vp, i32, i32, i32]
        L.vsm_debug_delaunay_gpu.argtypes = [vp, vp, i32, vp, i32, i32, i32, i32]
        L.vsm_debug_dc_bench.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32]
        L.vsm_debug_dc_bench.restype = C.c_double
        L.vsm_host_ties.argtypes = [vp, vp, i32, vp, i32]
        L.vsm_debug_ties_gpu.argtypes = [vp, vp, i32, vp, i32, vp]
        L.vsm_host_outliers_and_prior.argtypes = [C.POINTER(VsmParams), vp, i32, i32, vp, i32, vp, i32, i32]
        L.vsm_host_outliers_and_prior_threads.argtypes = [C.POINTER(VsmParams), vp, i32, i32, vp, i32, vp, i32, i32, i32]
        L.vsm_debug_dc2.argtypes = [C.POINTER(VsmParams), vp, i32, i32, i32, i32, vp, i32, vp, i32, i32, vp]
        L.vsm_debug_dc2_band_factor.argtypes = [i32]
        L.vsm_debug_predicates.argtypes = [vp, i32, vp]
        L.vsm_debug_ctx_layout.argtypes = [C.POINTER(VsmParams), i32, i32, i32, i32, i32, vp, vp, vp, i32, vp]
        L.vsm_debug_dc2_layout.argtypes = [i32, i32, i32, vp, vp, vp, i32, vp]
        L.vsm_debug_seq_plan.argtypes = [i32, i32, i32, i32, i32, C.c_char_p, vp, vp, i32]
        L.vsm_debug_chunk_jobs.restype = i32
        L.vsm_debug_chunk_jobs.argtypes = [i32, i32, i32, i32, i32, vp, i32, vp, vp, vp, vp]
        L.vsm_debug_pair_jobs.restype = i32
        L.vsm_debug_pair_jobs.argtypes = [i32, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp]
        L.vsm_debug_refine.argtypes = [vp, i32, vp, vp, i32, vp, vp]
        L.vsm_debug_refine_check.argtypes = [i32, i32, vp, vp, i32]
        L.vsm_debug_parabolic_apply.argtypes = [vp, vp, vp, i32, vp, vp]
        L.vsm_host_parabolic_fits.argtypes = [vp, i32, vp, vp]
        L.vsm_debug_compact_keys.argtypes = [i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp]
        L.vsm_pairs_run.argtypes = [vp, vp, vp, C.c_int64, C.c_int, i32, i32, i32, i32, i32, vp, i32, vp, vp]
        L.vsm_pairs_num_matches.argtypes = [vp, i32]
        L.vsm_pairs_get_matches.argtypes = [vp, i32, vp, i32]
        L.vsm_pairs_get_timings.argtypes = [vp, vp]
        L.vsm_pairs_get_timings.restype = None
        L.vsm_tracks_run.argtypes = [vp, i32, vp, i32, vp, vp, i32, i32]
        L.vsm_pairs_tracks.argtypes = [vp, i32, i32]
        L.vsm_tracks_count.argtypes = [vp]
        L.vsm_tracks_num_obs.argtypes = [vp]
        L.vsm_tracks_get.argtypes = [vp, vp, vp, vp]
        L.vsm_tracks_of_matches.argtypes = [vp, i32, vp, i32]
        L.vsm_tracks_get_stats.argtypes = [vp, vp]
        L.vsm_tracks_get_stats.restype = None
        L.vsm_tracks_get_timings.argtypes = [vp, vp]
        L.vsm_tracks_get_timings.restype = None
        L.vsm_host_tracks.restype = i32
        L.vsm_host_tracks.argtypes = [i32, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp]
        f64 = C.c_double
        L.vsm_triangulate_default_params.argtypes = [C.POINTER(VsmTriangulateParams)]
        L.vsm_triangulate_default_params.restype = None
        L.vsm_triangulate_run.argtypes = [vp, i32, vp, vp, f64, f64, f64, i32, vp, vp, vp, vp, C.POINTER(VsmTriangulateParams)]
        L.vsm_tracks_triangulate.argtypes = [vp, vp, vp, vp, vp, f64, f64, f64, C.POINTER(VsmTriangulateParams)]
        L.vsm_points_count.argtypes = [vp]
        L.vsm_points_get.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.vsm_points_get_stats.argtypes = [vp, vp]
        L.vsm_points_get_stats.restype = None
        L.vsm_points_get_timings.argtypes = [vp, vp]
        L.vsm_points_get_timings.restype = None
        L.vsm_host_triangulate.restype = i32
        L.vsm_host_triangulate.argtypes = [i32, vp, vp, f64, f64, f64, i32, vp, vp, vp, vp, C.POINTER(VsmTriangulateParams)] + [vp] * 6
        L.vsm_resect_default_params.argtypes = [C.POINTER(VsmResectParams)]
        L.vsm_resect_default_params.restype = None
        L.vsm_resect_run.argtypes = [vp, i32, vp, vp, vp, f64, f64, f64, i32, vp, vp, vp, vp, vp, C.POINTER(VsmResectParams)]
        L.vsm_points_resect.argtypes = [vp, vp, vp, vp, vp, vp, f64, f64, f64, C.POINTER(VsmResectParams)]
        L.vsm_resect_count.argtypes = [vp]
        L.vsm_resect_get.argtypes = [vp] + [vp] * 9
        L.vsm_resect_get_stats.argtypes = [vp, vp]
        L.vsm_resect_get_stats.restype = None
        L.vsm_resect_get_timings.argtypes = [vp, vp]
        L.vsm_resect_get_timings.restype = None
        L.vsm_adjust_default_params.argtypes = [C.POINTER(VsmAdjustParams)]
        L.vsm_adjust_default_params.restype = None
        L.vsm_adjust_run.argtypes = [vp, i32, vp, vp, vp, f64, f64, f64, i32, vp, vp, vp, vp, vp, C.POINTER(VsmAdjustParams)]
        L.vsm_points_adjust.argtypes = [vp, vp, vp, vp, vp, vp, f64, f64, f64, C.POINTER(VsmAdjustParams)]
        L.vsm_adjust_count.argtypes = [vp, vp, vp, vp]
        L.vsm_adjust_count.restype = None
        L.vsm_adjust_get_frames.argtypes = [vp] + [vp] * 4
        L.vsm_adjust_get_tracks.argtypes = [vp] + [vp] * 2
        L.vsm_adjust_get_history.argtypes = [vp] + [vp] * 7
        L.vsm_adjust_get_stats.argtypes = [vp, vp]
        L.vsm_adjust_get_stats.restype = None
        L.vsm_adjust_get_timings.argtypes = [vp, vp]
        L.vsm_adjust_get_timings.restype = None
        L.vsm_host_adjust.restype = i32
        L.vsm_host_adjust.argtypes = [i32, vp, vp, vp, f64, f64, f64, i32, vp, vp, vp, vp, vp, C.POINTER(VsmAdjustParams)] + [vp] * 15
        L.vsm_host_resect.restype = i32
        L.vsm_host_resect.argtypes = [i32, vp, vp, vp, f64, f64, f64, i32, vp, vp, vp, vp, vp, C.POINTER(VsmResectParams)] + [vp] * 9
        L.vsm_locate_default_params.argtypes = [C.POINTER(VsmLocateParams)]
        L.vsm_locate_default_params.restype = None
        L.vsm_locate_run.argtypes = [vp, i32, vp, f64, f64, f64, i32, vp, vp, vp, vp, vp, C.POINTER(VsmLocateParams)]
        L.vsm_points_locate.argtypes = [vp, vp, vp, vp, f64, f64, f64, C.POINTER(VsmLocateParams)]
        L.vsm_locate_count.argtypes = [vp]
        L.vsm_locate_get.argtypes = [vp] + [vp] * 11
        L.vsm_locate_get_stats.argtypes = [vp, vp]
        L.vsm_locate_get_stats.restype = None
        L.vsm_locate_get_timings.argtypes = [vp, vp]
        L.vsm_locate_get_timings.restype = None
        L.vsm_host_locate.restype = i32
        L.vsm_host_locate.argtypes = [i32, vp, f64, f64, f64, i32, vp, vp, vp, vp, vp, C.POINTER(VsmLocateParams)] + [vp] * 11
        L.vsm_host_locate_sample.argtypes = [C.c_uint32, i32, i32, vp]
        L.vsm_host_locate_fit.argtypes = [f64, f64, f64, f64, i32, vp, vp, vp, i32, vp, vp]
        L.vsm_host_locate_count.argtypes = [f64, f64, f64, i32, vp, vp, vp, vp, i32, f64, f64, vp]
        L.vsm_debug_locate_fit.argtypes = [f64, f64, f64, f64, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp]
        L.vsm_debug_locate_count.argtypes = [f64, f64, f64, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, f64, f64, i32, vp]
        L.vsm_debug_locate_winner.argtypes = [i32, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.vsm_debug_locate_hypotheses.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        for fn in (L.vsm_host_locate_sample, L.vsm_host_locate_fit, L.vsm_host_locate_count, L.vsm_debug_locate_fit, L.vsm_debug_locate_count,
                   L.vsm_debug_locate_winner, L.vsm_debug_locate_hypotheses):
            fn.restype = i32
        rop = C.POINTER(VsmReobserveParams)
        L.vsm_reobserve_default_params.argtypes = [rop]
        L.vsm_reobserve_default_params.restype = None
        L.vsm_reobserve_run.argtypes = [vp, i32, vp, vp, vp, f64, f64, f64, i32, i32, i32] + [vp] * 8 + [rop]
        L.vsm_points_reobserve.argtypes = [vp, vp, vp, vp, f64, f64, f64, rop]
        L.vsm_reobserve_count.argtypes = [vp, vp, vp]
        L.vsm_reobserve_count.restype = None
        L.vsm_reobserve_get.argtypes = [vp, vp, vp]
        L.vsm_reobserve_get_tracks.argtypes = [vp, vp]
        L.vsm_reobserve_get_frames.argtypes = [vp, vp]
        L.vsm_reobserve_get_stats.argtypes = [vp, vp]
        L.vsm_reobserve_get_stats.restype = None
        L.vsm_reobserve_get_timings.argtypes = [vp, vp]
        L.vsm_reobserve_get_timings.restype = None
        L.vsm_host_reobserve.argtypes = [i32, vp, vp, vp, f64, f64, f64, i32, i32, i32] + [vp] * 8 + [rop, i32] + [vp] * 5
        L.vsm_pairs_num_features.argtypes = [vp, i32, i32, i32]
        L.vsm_pairs_get_features.argtypes = [vp, i32, i32, i32, vp, i32]
        for fn in (L.vsm_reobserve_get, L.vsm_reobserve_get_tracks, L.vsm_reobserve_get_frames, L.vsm_host_reobserve, L.vsm_pairs_num_features,
                   L.vsm_pairs_get_features):
            fn.restype = i32
        fup = C.POINTER(VsmFuseParams)
        L.vsm_fuse_default_params.argtypes = [fup]
        L.vsm_fuse_default_params.restype = None
        L.vsm_fuse_run.argtypes = [vp, i32, vp, vp, vp, f64, f64, f64, i32, i32, i32] + [vp] * 8 + [fup]
        L.vsm_points_fuse.argtypes = [vp, vp, vp, vp, f64, f64, f64, fup]
        L.vsm_fuse_count.argtypes = [vp, vp, vp]
        L.vsm_fuse_count.restype = None
        L.vsm_fuse_get.argtypes = [vp, vp, vp]
        L.vsm_fuse_get_tracks.argtypes = [vp, vp, vp]
        L.vsm_fuse_get_merged.argtypes = [vp, vp, vp]
        L.vsm_fuse_get_frames.argtypes = [vp, vp]
        L.vsm_fuse_get_stats.argtypes = [vp, vp]
        L.vsm_fuse_get_stats.restype = None
        L.vsm_fuse_get_timings.argtypes = [vp, vp]
        L.vsm_fuse_get_timings.restype = None
        L.vsm_host_fuse.argtypes = [i32, vp, vp, vp, f64, f64, f64, i32, i32, i32] + [vp] * 8 + [fup, i32] + [vp] * 8
        for fn in (L.vsm_fuse_get, L.vsm_fuse_get_tracks, L.vsm_fuse_get_merged, L.vsm_fuse_get_frames, L.vsm_host_fuse):
            fn.restype = i32
        L.vsm_vet_default_params.argtypes = [C.POINTER(VsmVetParams)]
        L.vsm_vet_default_params.restype = None
        L.vsm_vet_run.argtypes = [vp, i32, vp, vp, f64, f64, f64, i32, vp, vp, vp, vp, vp, C.POINTER(VsmVetParams)]
        L.vsm_points_vet.argtypes = [vp, vp, vp, vp, vp, f64, f64, f64, C.POINTER(VsmVetParams)]
        L.vsm_vet_count.argtypes = [vp, vp, vp, vp]
        L.vsm_vet_count.restype = None
        L.vsm_vet_get_obs.argtypes = [vp] + [vp] * 2
        L.vsm_vet_get_tracks.argtypes = [vp] + [vp] * 6
        L.vsm_vet_get_frames.argtypes = [vp, vp]
        L.vsm_vet_get_kept.argtypes = [vp, vp, vp]
        for fn in (L.vsm_vet_get_obs, L.vsm_vet_get_tracks, L.vsm_vet_get_frames, L.vsm_vet_get_kept):
            fn.restype = i32
        L.vsm_vet_get_stats.argtypes = [vp, vp]
        L.vsm_vet_get_stats.restype = None
        L.vsm_vet_get_timings.argtypes = [vp, vp]
        L.vsm_vet_get_timings.restype = None
        L.vsm_host_vet.restype = i32
        L.vsm_host_vet.argtypes = [i32, vp, vp, f64, f64, f64, i32, vp, vp, vp, vp, vp, C.POINTER(VsmVetParams)] + [vp] * 12
        L.vsm_tracks_pixels.restype = i32
        L.vsm_tracks_pixels.argtypes = [vp, vp, vp, vp, vp]
        L.vsm_local_cpus.argtypes = [vp, i32]
        L.vsm_forkjoin_cpus.argtypes = [vp, i32]
        L.vsm_debug_dc2_band_factor.restype = None
        L.vsm_sequence_run.argtypes = [vp, vp, vp, C.c_int64, C.c_int, i32, i32, i32, i32, i32, vp, vp]
        L.vsm_sequence_num_matches.argtypes = [vp, i32]
        L.vsm_sequence_get_matches.argtypes = [vp, i32, vp, i32]
        L.vsm_sequence_get_timings.argtypes = [vp, vp]
        L.vsm_sequence_path.argtypes = [vp]
        L.vsm_set_option.argtypes = [vp, C.c_char_p, i32]
        L.vsm_host_register.argtypes = [vp, C.c_uint64]
        L.vsm_host_unregister.argtypes = [vp]
        L.vsm_device_pool_stats.argtypes = [vp]
        L.vsm_device_pool_stats.restype = None
        L.vsm_device_pool_trim.argtypes = []
        L.vsm_device_pool_trim.restype = None
        L.vsm_multi_create.restype = vp
        L.vsm_multi_create.argtypes = [C.POINTER(VsmVoStereoParams), i32]
        L.vsm_multi_destroy.argtypes = [vp]
        L.vsm_multi_process.argtypes = [vp, vp, vp, C.c_int64, C.c_int, i32, i32, i32, vp]
        L.vsm_multi_num_sequences.argtypes = [vp]
        L.vsm_multi_get_motion.argtypes = [vp, i32, vp]
        L.vsm_multi_motion_valid.argtypes = [vp, i32]
        L.vsm_multi_num_matches.argtypes = [vp, i32, C.c_int]
        L.vsm_multi_get_matches.argtypes = [vp, i32, C.c_int, vp, i32]
        L.vsm_multi_num_inliers.argtypes = [vp, i32]
        L.vsm_multi_get_inliers.argtypes = [vp, i32, vp, i32]
        L.vsm_multi_get_timings.argtypes = [vp, vp]
        vop = C.POINTER(VsmVoStereoParams)
        L.vsm_vo_stereo_default_params.argtypes = [vop]
        L.vsm_vo_stereo_create.restype = vp
        L.vsm_vo_stereo_create.argtypes = [vop]
        L.vsm_vo_stereo_destroy.argtypes = [vp]
        L.vsm_vo_stereo_process.argtypes = [vp, vp, vp, i32, i32, i32, C.c_int]
        L.vsm_vo_stereo_process_device.argtypes = [vp, vp, vp, i32, i32, i32, C.c_int]
        L.vsm_vo_stereo_process_matches.argtypes = [vp, vp, i32]
        L.vsm_vo_stereo_get_motion.argtypes = [vp, vp]
        L.vsm_vo_stereo_motion_valid.argtypes = [vp]
        L.vsm_vo_stereo_num_matches.argtypes = [vp]
        L.vsm_vo_stereo_get_matches.argtypes = [vp, vp, i32]
        L.vsm_vo_stereo_num_inliers.argtypes = [vp]
        L.vsm_vo_stereo_get_inliers.argtypes = [vp, vp, i32]
        L.vsm_vo_stereo_gain.argtypes = [vp, vp, i32]
        L.vsm_vo_stereo_gain.restype = f32
        L.vsm_vo_stereo_matcher.restype = vp
        L.vsm_vo_stereo_matcher.argtypes = [vp]
        L.vsm_vo_stereo_get_timings.argtypes = [vp, vp]
        L.vsm_vo_sampler_seed.argtypes = [C.c_uint32]
        L.vsm_host_estimate_motion_stereo.argtypes = [vop, vp, i32, i32, vp, vp, vp, vp]
        mop = C.POINTER(VsmVoMonoParams)
        L.vsm_vo_mono_default_params.argtypes = [mop]
        L.vsm_vo_mono_create.restype = vp
        L.vsm_vo_mono_create.argtypes = [mop]
        L.vsm_vo_mono_destroy.argtypes = [vp]
        L.vsm_vo_mono_process.argtypes = [vp, vp, i32, i32, i32, C.c_int]
        L.vsm_vo_mono_process_device.argtypes = [vp, vp, i32, i32, i32, C.c_int]
        L.vsm_vo_mono_process_matches.argtypes = [vp, vp, i32]
        L.vsm_vo_mono_get_motion.argtypes = [vp, vp]
        L.vsm_vo_mono_motion_valid.argtypes = [vp]
        L.vsm_vo_mono_num_matches.argtypes = [vp]
        L.vsm_vo_mono_get_matches.argtypes = [vp, vp, i32]
        L.vsm_vo_mono_num_inliers.argtypes = [vp]
        L.vsm_vo_mono_get_inliers.argtypes = [vp, vp, i32]
        L.vsm_vo_mono_gain.argtypes = [vp, vp, i32]
        L.vsm_vo_mono_gain.restype = f32
        L.vsm_vo_mono_matcher.restype = vp
        L.vsm_vo_mono_matcher.argtypes = [vp]
        L.vsm_vo_mono_get_timings.argtypes = [vp, vp]
        L.vsm_vo_mono_device_svd.argtypes = [vp]
        L.vsm_vo_mono_device_stages.argtypes = [vp]
        L.vsm_debug_mono_fit.argtypes = [vp, i32, vp, i32, vp]
        L.vsm_debug_mono_count.argtypes = [vp, i32, vp, i32, C.c_double, i32, vp]
        L.vsm_debug_mono_triangulate.argtypes = [vp, i32, C.c_double, C.c_double, C.c_double, vp, vp, vp, vp]
        L.vsm_debug_mono_vote.argtypes = [vp, i32, C.c_double, C.c_double, vp, vp]
        L.vsm_host_estimate_motion_mono.argtypes = [mop, vp, i32, i32, vp, vp, vp, vp]
        L.vsm_motions_run.argtypes = [vp, mop, i32, vp, vp, i32]
        L.vsm_pairs_motions.argtypes = [vp, mop, i32]
        L.vsm_motions_count.argtypes = [vp]
        L.vsm_motions_get.argtypes = [vp, vp, vp, vp, vp, vp]
        L.vsm_motions_inliers.argtypes = [vp, i32, vp, i32]
        L.vsm_motions_matches.argtypes = [vp, i32, vp, i32]
        L.vsm_motions_get_stats.argtypes = [vp, vp]
        L.vsm_motions_get_stats.restype = None
        L.vsm_motions_get_timings.argtypes = [vp, vp]
        L.vsm_motions_get_timings.restype = None
        L.vsm_motions_device_svd.argtypes = [vp]
        L.vsm_host_pairs_motions.restype = i32
        L.vsm_host_pairs_motions.argtypes = [mop, i32, vp, vp, i32, i32] + [vp] * 8
        L.vsm_chain_poses.restype = i32
        L.vsm_chain_poses.argtypes = [i32, vp, i32, vp, vp, i32, vp, vp]
        _lib = L
    return _lib


MONO_DEFAULTS = dict(height=1.0, pitch=0.0, ransac_iters=2000, inlier_threshold=0.00001, motion_threshold=100.0)


def vo_mono_params(f=1.0, cu=0.0, cv=0.0, bucket=(2, 50.0, 50.0), **kw):
    """VisualOdometryMono::parameters (viso/viso_mono.h:33-46, viso/viso.h:33-60) as the C struct"""
    p = VsmVoMonoParams()
    lib().vsm_vo_mono_default_params(C.byref(p))
    for k in list(kw):
        if k in MONO_DEFAULTS:
            v = kw.pop(k)
            setattr(p, k, int(v) if k == "ransac_iters" else float(v))
    for k, v in kw.items():
        if not hasattr(p.match, k):
            raise TypeError(f"unknown matcher parameter {k}")
        setattr(p.match, k, v)
    p.bucket_max_features, p.bucket_width, p.bucket_height = int(bucket[0]), float(bucket[1]), float(bucket[2])
    p.f, p.cu, p.cv = float(f), float(cu), float(cv)
    return p


def host_estimate_motion_mono(matches, params, threads=1):
    """mono egomotion of the product on a given flow-match list, host code only (no GPU)
    -> (rc, tr6, T 4x4, inliers or None)"""
    m = np.ascontiguousarray(matches, dtype=P_MATCH)
    tr = np.zeros(6)
    T = np.zeros(16)
    inl = np.zeros(max(len(m), 1), dtype=np.int32)
    n = C.c_int32(0)
    rc = lib().vsm_host_estimate_motion_mono(C.byref(params), m.ctypes.data_as(C.c_void_p), len(m), threads,
                                             tr.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p),
                                             inl.ctypes.data_as(C.c_void_p), C.cast(C.byref(n), C.c_void_p))
    return rc, tr, T.reshape(4, 4), (inl[: n.value].copy() if rc >= 0 else None)


MONO_STAGE_FIT, MONO_STAGE_COUNT, MONO_STAGE_TRIANGULATE, MONO_STAGE_VOTE = 1, 2, 4, 8


def _mono_check(rc, name):
    if rc == -1:
        raise ValueError(name + ": bad argument")
    if rc < 0:
        raise VisoMatchError(name + ": HIP error")
    return rc


def _mono_pts(pts):
    p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 4)   # u1p, v1p, u1c, v1c per row
    return p


def device_mono_fit(pts, picks):
    """test hook: k_mono_fit alone.  pts [n, 4] normalised (u1p, v1p, u1c, v1c), picks [K, 8] -> F [K, 3, 3]"""
    p = _mono_pts(pts)
    k = np.ascontiguousarray(picks, dtype=np.int32).reshape(-1, 8)
    F = np.zeros((len(k), 3, 3))
    _mono_check(lib().vsm_debug_mono_fit(p.ctypes.data_as(C.c_void_p), len(p), k.ctypes.data_as(C.c_void_p), len(k),
                                         F.ctypes.data_as(C.c_void_p)), "vsm_debug_mono_fit")
    return F


def device_mono_count(pts, F, thr, slice=0):
    """test hook: k_mono_inlier_count alone, at most `slice` hypotheses per launch (0: the device's limit) -> counts [K]"""
    p = _mono_pts(pts)
    F = np.ascontiguousarray(F, dtype=np.float64).reshape(-1, 9)
    out = np.zeros(len(F), dtype=np.int32)
    _mono_check(lib().vsm_debug_mono_count(p.ctypes.data_as(C.c_void_p), len(p), F.ctypes.data_as(C.c_void_p), len(F),
                                           float(thr), int(slice), out.ctypes.data_as(C.c_void_p)), "vsm_debug_mono_count")
    return out


def device_mono_triangulate(matches, f, cu, cv, R4, t4):
    """test hook: k_mono_triangulate alone for four candidates R4 [4, 3, 3], t4 [4, 3] -> (X [4, 4, n], chir [4])"""
    m = np.ascontiguousarray(matches, dtype=P_MATCH)
    R = np.ascontiguousarray(R4, dtype=np.float64).reshape(4, 9)
    t = np.ascontiguousarray(t4, dtype=np.float64).reshape(4, 3)
    X = np.zeros((4, 4, len(m)))
    chir = np.zeros(4, dtype=np.int32)
    _mono_check(lib().vsm_debug_mono_triangulate(m.ctypes.data_as(C.c_void_p), len(m), float(f), float(cu), float(cv),
                                                 R.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p),
                                                 X.ctypes.data_as(C.c_void_p), chir.ctypes.data_as(C.c_void_p)),
                "vsm_debug_mono_triangulate")
    return X, chir


def device_mono_vote(d, threshold, weight):
    """test hook: the estimator's plane vote on d [np] -> (sums [np], chosen index, True if the GPU proposed the sums)"""
    d = np.ascontiguousarray(d, dtype=np.float64).ravel()
    sums = np.zeros(len(d))
    best = C.c_int32(-1)
    rc = _mono_check(lib().vsm_debug_mono_vote(d.ctypes.data_as(C.c_void_p), len(d), float(threshold), float(weight),
                                               sums.ctypes.data_as(C.c_void_p), C.cast(C.byref(best), C.c_void_p)),
                     "vsm_debug_mono_vote")
    return sums, int(best.value), rc == 0


def vo_stereo_params(f=1.0, cu=0.0, cv=0.0, base=1.0, bucket=(2, 50.0, 50.0), ransac_iters=200, inlier_threshold=2.0,
                     reweighting=True, **match):
    """VisualOdometryStereo::parameters (viso/viso_stereo.h:33-44, viso/viso.h:33-60) as the C struct"""
    p = VsmVoStereoParams()
    lib().vsm_vo_stereo_default_params(C.byref(p))
    for k, v in match.items():
        if not hasattr(p.match, k):
            raise TypeError(f"unknown matcher parameter {k}")
        setattr(p.match, k, v)
    p.bucket_max_features, p.bucket_width, p.bucket_height = int(bucket[0]), float(bucket[1]), float(bucket[2])
    p.f, p.cu, p.cv, p.base = float(f), float(cu), float(cv), float(base)
    p.ransac_iters, p.inlier_threshold, p.reweighting = int(ransac_iters), float(inlier_threshold), int(reweighting)
    return p


def vo_sampler_seed(seed=71):
    """re-seed the process-wide RANSAC sampler (viso/viso.cpp:93 seeds it with 71 once per process)"""
    lib().vsm_vo_sampler_seed(seed)


def host_estimate_motion_stereo(matches, params, threads=1):
    """egomotion solver of the product on a given match list (host code; no GPU needed)
    -> (rc, tr6, T 4x4, inliers or None); rc 1 ok, 0 failed, -1 fewer than 6 matches (inliers None)"""
    m = np.ascontiguousarray(matches, dtype=P_MATCH)
    tr = np.zeros(6)
    T = np.zeros(16)
    inl = np.zeros(max(len(m), 1), dtype=np.int32)
    n = C.c_int32(0)
    rc = lib().vsm_host_estimate_motion_stereo(C.byref(params), m.ctypes.data_as(C.c_void_p), len(m), threads,
                                               tr.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p),
                                               inl.ctypes.data_as(C.c_void_p), C.cast(C.byref(n), C.c_void_p))
    return rc, tr, T.reshape(4, 4), (inl[: n.value].copy() if rc >= 0 else None)


def host_delaunay(pts, threads=1):
    """exact Delaunay of integer points (host code of the product; no GPU needed)"""
    pts = np.asarray(pts).reshape(-1, 2)
    x = np.ascontiguousarray(pts[:, 0], dtype=np.int32)
    y = np.ascontiguousarray(pts[:, 1], dtype=np.int32)
    cap = 2 * len(x) + 16
    tris = np.zeros((cap, 3), dtype=np.int32)
    k = lib().vsm_host_delaunay(x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), len(x),
                                tris.ctypes.data_as(C.c_void_p), cap, threads)
    return tris[:k]


def host_delaunay_split(pts, max_task_points, device_top_points=0):
    """the same triangulation through prepare / independent sub-trees / the merge nodes listed for the
    sub-tree solver's side (at most device_top_points points) / remaining merges (host code only)"""
    pts = np.asarray(pts).reshape(-1, 2)
    x = np.ascontiguousarray(pts[:, 0], dtype=np.int32)
    y = np.ascontiguousarray(pts[:, 1], dtype=np.int32)
    cap = 2 * len(x) + 16
    tris = np.zeros((cap, 3), dtype=np.int32)
    k = lib().vsm_host_delaunay_split(x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), len(x),
                                      tris.ctypes.data_as(C.c_void_p), cap, max_task_points, device_top_points)
    return tris[:k]


def delaunay_gpu_split(pts, max_task_points, device_top_points=0, device_kd=False):
    """test hook: sub-trees of the exact Delaunay and the merge nodes of at most device_top_points points on
    the GPU (device_kd: the kd order of the keys too), preparation and the remaining merges on the host"""
    pts = np.asarray(pts).reshape(-1, 2)
    x = np.ascontiguousarray(pts[:, 0], dtype=np.int32)
    y = np.ascontiguousarray(pts[:, 1], dtype=np.int32)
    cap = 2 * len(x) + 16
    tris = np.zeros((cap, 3), dtype=np.int32)
    k = lib().vsm_debug_delaunay_gpu(x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), len(x),
                                     tris.ctypes.data_as(C.c_void_p), cap, max_task_points, device_top_points, int(device_kd))
    if k < 0:
        raise VisoMatchError("vsm_debug_delaunay_gpu: HIP error")
    return tris[:k]


def ties(pts, gpu=False):
    """which matches at shared pixels stand for their points: sorted (carried index, right index) pairs where they
    differ, from the host emulation of Triangle's vertex sort or from the GPU's; (pairs, kernel microseconds).  pairs is
    None where the GPU's sort declines the list (too long, or more shared pixels than it reports)"""
    pts = np.asarray(pts).reshape(-1, 2)
    x = np.ascontiguousarray(pts[:, 0], dtype=np.int32)
    y = np.ascontiguousarray(pts[:, 1], dtype=np.int32)
    cap = 4096
    out = np.zeros((cap, 2), dtype=np.int32)
    us = C.c_double(0)
    if gpu:
        k = lib().vsm_debug_ties_gpu(x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), len(x), out.ctypes.data_as(C.c_void_p), cap,
                                     C.byref(us))
    else:
        k = lib().vsm_host_ties(x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), len(x), out.ctypes.data_as(C.c_void_p), cap)
    if k == -2:
        raise VisoMatchError("vsm_debug_ties_gpu: HIP error")
    if k < 0:
        return None, us.value
    o = out[:k]
    return o[np.lexsort(o.T[::-1])], us.value


def device_predicates(quads):
    """test hook: the exact Delaunay's predicates as the GPU evaluates them on [n, 4, 2] integer points (coordinates < 2^14):
    an [n, 3] array of (orientation determinant of a, b, c; sign of the in-circle determinant of a, b, c, d; 1 if d lies
    strictly inside the circle through a, b, c)"""
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4, 2)
    assert q.min(initial=0) >= 0 and q.max(initial=0) < 1 << 14
    packed = np.ascontiguousarray(q[:, :, 0] | (q[:, :, 1] << 16), dtype=np.uint32)
    out = np.zeros((len(q), 3), dtype=np.int32)
    if lib().vsm_debug_predicates(packed.ctypes.data_as(C.c_void_p), len(q), out.ctypes.data_as(C.c_void_p)) != 0:
        raise VisoMatchError("vsm_debug_predicates: HIP error")
    return out


def _layout(call, n_scalars):
    """a layout hook's answer: (return code, scalars, [(name, block, index, set, offset, bytes) per array, as placed])"""
    scalars, n = np.zeros(n_scalars, dtype=np.int64), C.c_int32(0)
    rc = call(scalars.ctypes.data_as(C.c_void_p), None, None, 0, C.addressof(n))
    rows, names = np.zeros((n.value, 5), dtype=np.int64), np.zeros(n.value, dtype="S16")
    if rc == 0:
        rc = call(scalars.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p), names.ctypes.data_as(C.c_void_p), n.value, C.addressof(n))
    return rc, scalars.tolist(), [(nm.decode(),) + tuple(r) for nm, r in zip(names.tolist(), rows.tolist())]


def ctx_layout(params, w, h, nframes, npairs, heads=False):
    """test hook (no GPU): the device arena (block 0) and the host-mapped result block (block 1) of a working set of nframes
    frame slots and npairs pairs - (return code, [arena bytes, host-mapped bytes, pair_stride, f_stride, ranges_stride,
    cap_set[0], cap_set[1], qcap], rows); with a code other than 0 the rest is empty"""
    return _layout(lambda *a: lib().vsm_debug_ctx_layout(C.byref(params), w, h, nframes, npairs, int(bool(heads)), *a), 8)


def dc2_layout(npairs, cap, host_ties):
    """test hook (no GPU): the device block (0) and the host-mapped block (1) of a Delaunay chain's bank - (return code,
    [device bytes, host-mapped bytes, pair_stride, ties_stride, host keys' pitch, tie patches' pitch], rows)"""
    return _layout(lambda *a: lib().vsm_debug_dc2_layout(npairs, cap, int(bool(host_ties)), *a), 6)


def seq_plan(n_frames, pool_threads, host_in=False, seq_chunk=0, seq_first_chunk=0, plan=None):
    """test hook (no GPU): the chunk plan of the look-ahead call's GPU-resident form - (chunk size the banks are laid out
    for, [first frame of each chunk ..., n_frames]); plan: what VSM_SEQ_PLAN would hold"""
    chunk = C.c_int32(0)
    starts = np.zeros(n_frames + 2, dtype=np.int32)
    n = lib().vsm_debug_seq_plan(n_frames, pool_threads, int(bool(host_in)), seq_chunk, seq_first_chunk,
                                 None if plan is None else plan.encode(), C.addressof(chunk), starts.ctypes.data_as(C.c_void_p), len(starts))
    if n < 0:
        raise VisoMatchError("vsm_debug_seq_plan: bad arguments")
    return chunk.value, starts[:n + 1].tolist()


def chunk_jobs(method, multi_stage, sides, banks, chunk, starts, counts, tr_valid=None):
    """test hook (no GPU): the job tables of a look-ahead call's chunks - starts: [first frame of each chunk ..., n_frames];
    counts[frame][side][set]: the feature counts; tr_valid: a flag per frame or None.  Returns (int32 [frames][7]: img_prev,
    img_curr, nq[0], nq[1], use_tr, valid, seq_src; int32 [chunks][2]: max_nq)"""
    starts = np.ascontiguousarray(starts, dtype=np.int32)
    n_chunks, n_frames = len(starts) - 1, int(starts[-1])
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    assert counts.shape == (n_frames, 2, 2)
    tv = None if tr_valid is None else np.ascontiguousarray(tr_valid, dtype=np.uint8)
    assert tv is None or tv.shape == (n_frames,)
    frames = np.zeros((n_frames, 7), dtype=np.int32)
    max_nq = np.zeros((n_chunks, 2), dtype=np.int32)
    rc = lib().vsm_debug_chunk_jobs(method, int(bool(multi_stage)), sides, banks, chunk, starts.ctypes.data_as(C.c_void_p), n_chunks,
                                    counts.ctypes.data_as(C.c_void_p), None if tv is None else tv.ctypes.data_as(C.c_void_p),
                                    frames.ctypes.data_as(C.c_void_p), max_nq.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise VisoMatchError("vsm_debug_chunk_jobs: bad arguments")
    return frames, max_nq


def pair_jobs(method, multi_stage, sides, counts, pairs, chunk, tr_valid=None):
    """test hook (no GPU): the job table of match_pairs - counts[frame][side][set]: the feature counts of the frame set;
    pairs: [(previous frame, current frame), ...]; chunk: pairs per step; tr_valid: a flag per pair or None.  Returns (int32
    [pairs][7]: img_prev, img_curr, nq[0], nq[1], use_tr, valid, number (from 1) of the pair whose Tr the job took;
    int32 [chunks][2]: max_nq)"""
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    assert counts.ndim == 3 and counts.shape[1:] == (2, 2)
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    tv = None if tr_valid is None else np.ascontiguousarray(tr_valid, dtype=np.uint8)
    assert tv is None or tv.shape == (len(pr),)
    chunk = int(chunk)
    out = np.zeros((len(pr), 7), dtype=np.int32)
    max_nq = np.zeros((max(-(-len(pr) // max(chunk, 1)), 1), 2), dtype=np.int32)
    n = lib().vsm_debug_pair_jobs(method, int(bool(multi_stage)), sides, len(counts), counts.ctypes.data_as(C.c_void_p),
                                  pr.ctypes.data_as(C.c_void_p), len(pr), chunk, None if tv is None else tv.ctypes.data_as(C.c_void_p),
                                  out.ctypes.data_as(C.c_void_p), max_nq.ctypes.data_as(C.c_void_p))
    if n < 0:
        raise VisoMatchError("vsm_debug_pair_jobs: bad arguments")
    return out, max_nq[:n]


TRACK_STATS = ("nodes", "edges", "tracks", "inconsistent", "by_wave", "by_workgroup", "by_host", "scan_block")
TRACK_TIMINGS = ("pack_us", "upload_us", "kernels_us", "download_host_us")


class Tracks:
    """multi-view feature tracks (include/visomatch.h, vsm_tracks_run): offsets [T+1], obs [n_obs, 4] = {frame, feature,
    pair, 2 * match + end}, flags [T] (bit 0: two observations in one frame); of_pair(k): the track of every match of pair k
    (-1: dropped); stats / timings: dicts (empty for the host view)."""

    def __init__(self, offsets, obs, flags, of_pairs, stats=None, timings=None):
        self.offsets, self.obs, self.flags, self._of_pairs = offsets, obs, flags, of_pairs
        self.stats, self.timings = stats or {}, timings or {}

    def __len__(self):
        return len(self.flags)

    def of_pair(self, k):
        return self._of_pairs[k]

    def track(self, t):
        return self.obs[self.offsets[t]:self.offsets[t + 1]]


def _list_inputs(lists, counts=None):
    """(the lists as contiguous P_MATCH arrays, their addresses, their counts); counts: override the lists' lengths"""
    ls = [None if l is None else np.ascontiguousarray(l, dtype=P_MATCH) for l in lists]
    ptrs = (C.c_void_p * max(len(ls), 1))(*[None if l is None or len(l) == 0 else l.ctypes.data for l in ls])
    if counts is None:
        counts = [0 if l is None else len(l) for l in ls]
    return ls, ptrs, np.ascontiguousarray(counts, dtype=np.int32)


def _optional_lists(lists, counts=None):
    """_list_inputs for a handle form's lists, or - None: the lists of the last match_pairs call - three times None"""
    return (None, None, None) if lists is None else _list_inputs(lists, counts)


def _track_inputs(pairs, lists, counts=None):
    """(pairs [P,2] int32, then what _list_inputs gives for the pairs' lists)"""
    pa = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    assert len(lists) == len(pa)
    return (pa,) + _list_inputs(lists, counts)


def _stage_dicts(handle, get_stats, stat_names, get_timings, timing_names):
    """(stats, timings) of a stage's last result on a handle, as dicts under the given names"""
    st, tm = np.zeros(len(stat_names), np.int64), np.zeros(len(timing_names), np.float64)
    get_stats(handle, _ptr(st))
    get_timings(handle, _ptr(tm))
    return dict(zip(stat_names, st.tolist())), dict(zip(timing_names, tm.tolist()))


def host_tracks(n_frames, pairs, lists, side=0, min_length=2, counts=None):
    """vsm_host_tracks: the tracks of the match lists `lists` (one P_MATCH array per pair of `pairs`) by a sequential
    union-find on the host - no GPU.  counts: override the lists' lengths (argument tests).  Returns a Tracks object;
    raises VisoMatchError on VSM_EARG."""
    L = lib()
    pa, ls, ptrs, cnt = _track_inputs(pairs, lists, counts)
    args = (int(n_frames), pa.ctypes.data_as(C.c_void_p), len(pa), ptrs, cnt.ctypes.data_as(C.c_void_p), int(side), int(min_length))
    n_obs = C.c_int32(0)
    T = _check(L.vsm_host_tracks(*args, None, None, None, None, C.byref(n_obs)), "vsm_host_tracks")
    offsets, obs, flags = np.zeros(T + 1, np.int32), np.zeros((n_obs.value, 4), np.int32), np.zeros(T, np.uint8)
    tom = np.zeros(int(cnt.sum()), np.int32)
    got = L.vsm_host_tracks(*args, offsets.ctypes.data_as(C.c_void_p), obs.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p),
                            tom.ctypes.data_as(C.c_void_p), C.byref(n_obs))
    assert got == T
    return Tracks(offsets, obs, flags, np.split(tom, np.cumsum(cnt)[:-1]) if len(cnt) else [])


POINT_STATUS = ("kept", "flagged", "no_pose", "too_short", "at_infinity", "type", "update_failed", "not_converged", "too_far", "small_angle")
POINT_TIMINGS = ("gather_us", "upload_us", "kernels_us", "download_host_us")


class Points:
    """triangulated tracks (include/visomatch.h, vsm_triangulate_run): per track status [T] int32 (0 = kept, POINT_STATUS names
    the values), xyz [T, 3] float64, type [T] int32, updates [T] int32, dist [T] and angle [T] float64; stats: tracks per
    status name, timings: dict (both empty for the host view)."""

    def __init__(self, status, xyz, type, updates, dist, angle, stats=None, timings=None):
        self.status, self.xyz, self.type, self.updates, self.dist, self.angle = status, xyz, type, updates, dist, angle
        self.stats, self.timings = stats or {}, timings or {}

    def __len__(self):
        return len(self.status)

    @property
    def kept(self):
        return self.status == 0


MOTION_STAGES = ("few_matches", "degenerate", "few_inliers", "none_in_front", "few_in_front", "median", "ok")
MOTION_STATS = MOTION_STAGES + ("device_fit", "device_count", "device_triangulate", "device_vote", "chunks", "waits")
MOTION_TIMINGS = ("sample_pack_upload_us", "fit_count_winner_us", "host_fits_us", "triangulate_us", "median_vote_us", "total_us")


class Motions:
    """monocular motions of a pair set (include/visomatch.h, vsm_motions_run): per pair rc [P] int32 (1, 0, -1), stage [P] int32
    (MOTION_STAGES names the values), tr [P, 6] and T [P, 4, 4] float64 (zero / the identity where rc != 1); inliers(k): pair k's
    inlier indices into matches(k), the list its estimate saw (bucketed where bucketing was on); stats / timings: dicts (the
    host view's stats hold the stage counts only)."""

    def __init__(self, rc, stage, tr, T, inliers, matches, stats=None, timings=None):
        self.rc, self.stage, self.tr, self.T, self._inliers, self._matches = rc, stage, tr, T, inliers, matches
        self.stats, self.timings = stats or {}, timings or {}

    def __len__(self):
        return len(self.rc)

    def inliers(self, k):
        return self._inliers[k]

    def matches(self, k):
        return self._matches[k]


def host_pairs_motions(lists, params, bucket=False, threads=1, counts=None):
    """vsm_host_pairs_motions: every list's mono motion on `threads` host threads - no GPU.  counts: override the lists'
    lengths (argument tests).  Returns a Motions object; raises VisoMatchError on VSM_EARG."""
    ls, ptrs, cnt = _list_inputs(lists, counts)
    P, tot = len(ls), int(np.clip(cnt, 0, None).sum())
    rc, stage, n_inl, n_m = (np.zeros(P, np.int32) for _ in range(4))
    tr, T = np.zeros((P, 6)), np.zeros((P, 4, 4))
    inl, mm = np.zeros(max(tot, 1), np.int32), np.zeros(max(tot, 1), P_MATCH)
    _check(lib().vsm_host_pairs_motions(None if params is None else C.byref(params), P, ptrs, _ptr(cnt), int(bool(bucket)), int(threads), _ptr(rc), _ptr(stage),
                                        _ptr(tr), _ptr(T), _ptr(n_inl), _ptr(inl), _ptr(n_m), _ptr(mm)), "vsm_host_pairs_motions")
    off = np.concatenate([[0], np.cumsum(cnt)])
    st = np.bincount(stage, minlength=len(MOTION_STAGES))
    return Motions(rc, stage, tr, T, [inl[off[k]:off[k] + n_inl[k]].copy() for k in range(P)], [mm[off[k]:off[k] + n_m[k]].copy() for k in range(P)],
                   dict(zip(MOTION_STAGES, st.tolist())))


def chain_poses(n_frames, pairs, T, rc, root=0):
    """vsm_chain_poses: pair motions T [P, 4, 4] (or [P, 16]) with their rc into camera-to-world poses -> (poses [F, 12],
    valid [F] uint8, frames with a pose); raises VisoMatchError on VSM_EARG."""
    pa = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    t = np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(len(pa), 16)) if len(pa) else np.zeros((0, 16))
    r = np.ascontiguousarray(rc, dtype=np.int32)
    assert r.shape == (len(pa),)
    n = max(int(n_frames), 0)
    poses, valid = np.zeros((n, 12)), np.zeros(n, np.uint8)
    got = _check(lib().vsm_chain_poses(int(n_frames), _ptr(pa), len(pa), _ptr(t), _ptr(r), int(root), _ptr(poses), _ptr(valid)), "vsm_chain_poses")
    return poses, valid, got


def _default_params(struct, defaults, kw):
    """a parameter struct filled by the library's function `defaults`, with fields overridden by keyword"""
    p = struct()
    getattr(lib(), defaults)(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def _params_ref(struct, make, params):
    """a call's params argument by reference: a `struct` itself, or make(**params) for a dict of its fields (None: the
    defaults); _NO_PARAMS: a NULL pointer"""
    if params is _NO_PARAMS:
        return None
    return C.byref(params if isinstance(params, struct) else make(**(params or {})))


def triangulate_params(**kw):
    """vsm_triangulate_default_params with fields overridden by keyword"""
    return _default_params(VsmTriangulateParams, "vsm_triangulate_default_params", kw)


def _n_tracks(offsets, n_tracks=None):
    """T = len(offsets) - 1, unless overridden (argument tests)"""
    return max(len(offsets) - 1, 0) if n_tracks is None else int(n_tracks)


def _mask(mask, n):
    """a per-frame mask as n bytes, or None"""
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
    assert m is None or m.shape == (n,)
    return m


def _pose_inputs(poses, pose_valid, n_frames=None):
    """(poses [F, 12] float64 - from [F, 12], [F, 3, 4] or [F, 4, 4] -, validity bytes or None)"""
    po = np.asarray(poses, dtype=np.float64)
    po = np.ascontiguousarray(po.reshape(len(po), -1)[:, :12]) if po.size else np.zeros((0, 12))
    if n_frames is not None:
        assert len(po) == n_frames, (len(po), n_frames)
    return po, _mask(pose_valid, len(po))


def _triangulate_inputs(poses, pose_valid, offsets, obs_frames, uv, flags):
    po, pv = _pose_inputs(poses, pose_valid)
    off = np.ascontiguousarray(offsets, dtype=np.int32)
    fr = np.ascontiguousarray(obs_frames, dtype=np.int32)
    px = np.ascontiguousarray(np.asarray(uv, dtype=np.float32).reshape(-1, 2))
    fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
    return po, pv, off, fr, px, fl


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _points_arrays(T):
    return (np.zeros(T, np.int32), np.zeros((T, 3), np.float64), np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T, np.float64),
            np.zeros(T, np.float64))


def host_triangulate(poses, f, cu, cv, offsets, obs_frames, uv, flags=None, pose_valid=None, params=None, n_tracks=None):
    """vsm_host_triangulate: the tracks' 3-D points on one host thread - no GPU.  n_tracks: override len(offsets) - 1 (argument
    tests).  Returns a Points object; raises VisoMatchError on VSM_EARG."""
    po, pv, off, fr, px, fl = _triangulate_inputs(poses, pose_valid, offsets, obs_frames, uv, flags)
    T = _n_tracks(off, n_tracks)
    out = _points_arrays(max(T, 0))
    got = _check(lib().vsm_host_triangulate(len(po), _ptr(po), _ptr(pv), float(f), float(cu), float(cv), T, _ptr(off), _ptr(fr), _ptr(px), _ptr(fl),
                                            _params_ref(VsmTriangulateParams, triangulate_params, params), *[_ptr(a) for a in out]), "vsm_host_triangulate")
    assert got == T
    return Points(*out)


RESECT_STATUS = ("refined", "no_pose", "not_asked", "too_few_rows", "too_few_used", "no_pivot", "not_converged")
RESECT_TIMINGS = ("group_us", "upload_us", "kernels_us", "download_host_us")


class Resection:
    """refined poses (include/visomatch.h, vsm_resect_run): per frame status [F] int32 (0 = refined, RESECT_STATUS names the
    values), poses [F, 12] float64 camera to world, updates, rows, used [F] int32, ss_before, ss_after, rms_before, rms_after [F]
    float64; stats: frames per status name, timings: dict (both empty for the host view)."""

    def __init__(self, status, poses, updates, rows, used, ss_before, ss_after, rms_before, rms_after, stats=None, timings=None):
        self.status, self.poses, self.updates, self.rows, self.used = status, poses, updates, rows, used
        self.ss_before, self.ss_after, self.rms_before, self.rms_after = ss_before, ss_after, rms_before, rms_after
        self.stats, self.timings = stats or {}, timings or {}

    def __len__(self):
        return len(self.status)

    @property
    def refined(self):
        return self.status == 0


def resect_params(**kw):
    """vsm_resect_default_params with fields overridden by keyword"""
    return _default_params(VsmResectParams, "vsm_resect_default_params", kw)


def _resect_arrays(F):
    return (np.zeros(F, np.int32), np.zeros((F, 12), np.float64), np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros(F, np.int32),
            np.zeros(F, np.float64), np.zeros(F, np.float64), np.zeros(F, np.float64), np.zeros(F, np.float64))


def _resect_inputs(poses, pose_valid, refine, offsets, obs_frames, uv, xyz, use):
    po, pv, off, fr, px, us = _triangulate_inputs(poses, pose_valid, offsets, obs_frames, uv, use)
    rf = _mask(refine, len(po))
    pt = None if xyz is None else np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
    assert pt is None or len(pt) >= len(off) - 1
    assert us is None or len(us) >= len(off) - 1
    return po, pv, rf, off, fr, px, pt, us


def host_resect(poses, f, cu, cv, offsets, obs_frames, uv, xyz, use=None, refine=None, pose_valid=None, params=None, n_tracks=None):
    """vsm_host_resect: every frame's pose refined against the points on one host thread - no GPU.  n_tracks: override
    len(offsets) - 1 (argument tests).  Returns a Resection object; raises VisoMatchError on VSM_EARG."""
    po, pv, rf, off, fr, px, pt, us = _resect_inputs(poses, pose_valid, refine, offsets, obs_frames, uv, xyz, use)
    T = _n_tracks(off, n_tracks)
    out = _resect_arrays(len(po))
    got = _check(lib().vsm_host_resect(len(po), _ptr(po), _ptr(pv), _ptr(rf), float(f), float(cu), float(cv), T, _ptr(off), _ptr(fr), _ptr(px), _ptr(pt),
                                       _ptr(us), _params_ref(VsmResectParams, resect_params, params), *[_ptr(a) for a in out]), "vsm_host_resect")
    assert got == len(po)
    return Resection(*out)


VET_CODES = ("inlier", "unused", "no_pose", "behind", "gated")
VET_STATUS = ("kept", "unused", "too_few_inliers", "one_frame")
VET_STATS = tuple("obs_" + c for c in VET_CODES) + tuple("tracks_" + s for s in VET_STATUS)
VET_TIMINGS = ("gather_us", "upload_us", "kernels_us", "download_host_us")


class Vetting:
    """vetted observations (include/visomatch.h, vsm_vet_run): per observation code [n_obs] uint8 (0 = inlier, VET_CODES names the
    values) and r2 [n_obs] float32; per track status [T] int32 (0 = kept, VET_STATUS names the values), n_in, frame_lo, frame_hi
    [T] int32, ss, worst [T] float64; per frame frame_counts [F, 3] int32 (inliers, behind, gated); the pruned set kept_offsets
    [T + 1], kept_index [n_kept] int32; stats: observations per code and tracks per status by name, timings: dict (empty for the
    host view)."""

    def __init__(self, code, r2, status, n_in, frame_lo, frame_hi, ss, worst, frame_counts, kept_offsets, kept_index, stats=None, timings=None):
        self.code, self.r2 = code, r2
        self.status, self.n_in, self.frame_lo, self.frame_hi, self.ss, self.worst = status, n_in, frame_lo, frame_hi, ss, worst
        self.frame_counts, self.kept_offsets, self.kept_index = frame_counts, kept_offsets, kept_index
        if stats is None:
            stats = dict(zip(VET_STATS, np.bincount(code, minlength=5).tolist() + np.bincount(status, minlength=4).tolist()))
        self.stats, self.timings = stats, timings or {}

    def __len__(self):
        return len(self.status)

    @property
    def kept(self):
        return self.status == 0

    @property
    def inlier(self):
        return self.code == 0

    def prune(self, obs_frames, uv):
        """the track set without the outliers, over the same T tracks: (kept_offsets, obs_frames[kept_index], uv[kept_index])"""
        fr = np.asarray(obs_frames, dtype=np.int32)
        px = np.asarray(uv, dtype=np.float32).reshape(-1, 2)
        assert len(fr) == len(self.code) and len(px) == len(self.code)
        return self.kept_offsets.copy(), np.ascontiguousarray(fr[self.kept_index]), np.ascontiguousarray(px[self.kept_index])


def vet_params(**kw):
    """vsm_vet_default_params with fields overridden by keyword"""
    return _default_params(VsmVetParams, "vsm_vet_default_params", kw)


def _vet_arrays(T, n_obs, F, n_kept):
    return (np.zeros(n_obs, np.uint8), np.zeros(n_obs, np.float32), np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T, np.int32),
            np.zeros(T, np.float64), np.zeros(T, np.float64), np.zeros((F, 3), np.int32), np.zeros(T + 1, np.int32), np.zeros(n_kept, np.int32))


def _vet_inputs(poses, pose_valid, offsets, obs_frames, uv, xyz, use):
    po, pv, _, off, fr, px, pt, us = _resect_inputs(poses, pose_valid, None, offsets, obs_frames, uv, xyz, use)
    return po, pv, off, fr, px, pt, us


def host_vet(poses, f, cu, cv, offsets, obs_frames, uv, xyz, use=None, pose_valid=None, params=None, n_tracks=None):
    """vsm_host_vet: every observation vetted on one host thread - no GPU.  n_tracks: override len(offsets) - 1 (argument
    tests).  Returns a Vetting object; raises VisoMatchError on VSM_EARG."""
    po, pv, off, fr, px, pt, us = _vet_inputs(poses, pose_valid, offsets, obs_frames, uv, xyz, use)
    T = _n_tracks(off, n_tracks)
    out = _vet_arrays(max(T, 0), len(fr), len(po), len(fr))
    n_kept = C.c_int32(0)
    got = _check(lib().vsm_host_vet(len(po), _ptr(po), _ptr(pv), float(f), float(cu), float(cv), T, _ptr(off), _ptr(fr), _ptr(px), _ptr(pt), _ptr(us),
                                    _params_ref(VsmVetParams, vet_params, params), *[_ptr(a) for a in out], C.byref(n_kept)), "vsm_host_vet")
    assert got == T
    return Vetting(*out[:-1], out[-1][:n_kept.value].copy())


ADJUST_FRAME_STATUS = ("free", "no_pose", "not_asked", "too_few_rows", "unused_4", "unused_5", "unused_6", "held")
ADJUST_TRACK_STATUS = ("free", "unused", "too_few_active", "no_pivot")
ADJUST_STATS = (tuple("frames_" + s for s in ADJUST_FRAME_STATUS) + tuple("tracks_" + s for s in ADJUST_TRACK_STATUS)
                + ("rounds", "rounds_accepted", "stop", "cg_iterations"))
ADJUST_STOP = ("", "ftol", "lambda_max", "max_rounds")
ADJUST_CG_END = ("", "converged", "breakdown", "cg_iters")
ADJUST_TIMINGS = ("group_us", "upload_us", "kernels_us", "download_host_us")
ADJUST_HISTORY = np.dtype([("cost_before", "<f8"), ("cost_after", "<f8"), ("lambda", "<f8"), ("cg_iters", "<i4"), ("cg_end", "<i4"), ("accepted", "<i4"),
                           ("active", "<i4")])


class Adjustment:
    """jointly adjusted poses and points (include/visomatch.h, vsm_adjust_run): per frame frame_status [F] int32 (0 = free in the
    last round, ADJUST_FRAME_STATUS names the values), poses [F, 12] float64 camera to world, rows, active [F] int32; per track
    track_status [T] int32 (ADJUST_TRACK_STATUS) and xyz [T, 3] float64; history: one ADJUST_HISTORY record per round run;
    stats: dict by ADJUST_STATS; timings: dict (empty for the host view)."""

    def __init__(self, frame_status, poses, rows, active, track_status, xyz, history, stats, timings=None):
        self.frame_status, self.poses, self.rows, self.active = frame_status, poses, rows, active
        self.track_status, self.xyz, self.history = track_status, xyz, history
        self.stats, self.timings = stats, timings or {}

    def __len__(self):
        return len(self.frame_status)

    @property
    def cost(self):
        """the cost after the last round (0.0 without a round)"""
        return float(self.history["cost_after"][-1]) if len(self.history) else 0.0


def adjust_params(**kw):
    """vsm_adjust_default_params with fields overridden by keyword"""
    return _default_params(VsmAdjustParams, "vsm_adjust_default_params", kw)


def _adjust_arrays(F, T, rounds):
    return ([np.zeros(F, np.int32), np.zeros((F, 12), np.float64), np.zeros(F, np.int32), np.zeros(F, np.int32)],
            [np.zeros(T, np.int32), np.zeros((T, 3), np.float64)],
            [np.zeros(rounds, np.float64) for _ in range(3)] + [np.zeros(rounds, np.int32) for _ in range(4)])


def _adjust_history(cols, n):
    h = np.zeros(n, ADJUST_HISTORY)
    for name, c in zip(ADJUST_HISTORY.names, cols):
        h[name] = c[:n]
    return h


def host_adjust(poses, f, cu, cv, offsets, obs_frames, uv, xyz, use=None, refine=None, pose_valid=None, params=None, n_tracks=None):
    """vsm_host_adjust: poses and points adjusted jointly on one host thread - no GPU.  Arguments as for host_resect; params: a
    dict of vsm_adjust_params fields or the struct.  Returns an Adjustment object; raises VisoMatchError on VSM_EARG."""
    po, pv, rf, off, fr, px, pt, us = _resect_inputs(poses, pose_valid, refine, offsets, obs_frames, uv, xyz, use)
    T = _n_tracks(off, n_tracks)
    ref = _params_ref(VsmAdjustParams, adjust_params, params)
    rounds = max(int(ref._obj.max_rounds), 0) if ref is not None else 0
    fa, ta, ha = _adjust_arrays(len(po), max(T, 0), rounds)
    n, stats = C.c_int32(0), np.zeros(16, np.int64)
    got = _check(lib().vsm_host_adjust(len(po), _ptr(po), _ptr(pv), _ptr(rf), float(f), float(cu), float(cv), T, _ptr(off), _ptr(fr), _ptr(px), _ptr(pt),
                                       _ptr(us), ref, *[_ptr(a) for a in fa + ta + ha], C.byref(n), _ptr(stats)), "vsm_host_adjust")
    assert got == len(po)
    return Adjustment(*fa, *ta, _adjust_history(ha, n.value), dict(zip(ADJUST_STATS, stats.tolist())))


LOCATE_STATUS = ("located", "not_asked", "too_few_eligible", "no_valid_hypothesis", "too_few_inliers", "linear_only", "not_converged")
LOCATE_TIMINGS = ("group_sample_us", "upload_us", "kernels_us", "download_host_us")
LOCATE_ARRAYS = ("status", "poses", "linear_poses", "best", "inliers", "rows", "eligible", "updates", "used", "ss_after", "rms_after")


class Location:
    """located frames (include/visomatch.h, vsm_locate_run): per frame status [F] int32 (0 = located, LOCATE_STATUS names the
    values), poses and linear_poses [F, 12] float64 camera to world (zeros where there is none), best (the winning hypothesis or
    -1), inliers (its count), rows, eligible, updates, used [F] int32, ss_after, rms_after [F] float64; stats: frames per status
    name, timings: dict (both empty for the host view)."""

    def __init__(self, status, poses, linear_poses, best, inliers, rows, eligible, updates, used, ss_after, rms_after, stats=None, timings=None):
        self.status, self.poses, self.linear_poses, self.best, self.inliers = status, poses, linear_poses, best, inliers
        self.rows, self.eligible, self.updates, self.used, self.ss_after, self.rms_after = rows, eligible, updates, used, ss_after, rms_after
        self.stats, self.timings = stats or {}, timings or {}

    def __len__(self):
        return len(self.status)

    def located(self):
        """the frames that have a refined pose: status 0, or 6 (the estimate as it stands after max_updates)"""
        return (self.status == 0) | (self.status == 6)


def locate_params(**kw):
    """vsm_locate_default_params with fields overridden by keyword"""
    return _default_params(VsmLocateParams, "vsm_locate_default_params", kw)


def _locate_arrays(F):
    return (np.zeros(F, np.int32), np.zeros((F, 12), np.float64), np.zeros((F, 12), np.float64), np.zeros(F, np.int32), np.zeros(F, np.int32),
            np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros(F, np.float64), np.zeros(F, np.float64))


def _locate_inputs(n_frames, locate, offsets, obs_frames, uv, xyz, use):
    F = int(n_frames)
    lo = _mask(locate, max(F, 0))
    off = np.ascontiguousarray(offsets, dtype=np.int32)
    fr = np.ascontiguousarray(obs_frames, dtype=np.int32)
    px = np.ascontiguousarray(np.asarray(uv, dtype=np.float32).reshape(-1, 2))
    pt = None if xyz is None else np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
    us = None if use is None else np.ascontiguousarray(use, dtype=np.uint8)
    assert pt is None or len(pt) >= len(off) - 1
    assert us is None or len(us) >= len(off) - 1
    return F, lo, off, fr, px, pt, us


def host_locate(n_frames, f, cu, cv, offsets, obs_frames, uv, xyz, use=None, locate=None, params=None, n_tracks=None):
    """vsm_host_locate: every asked-for frame located against the points on one host thread - no GPU.  The tracks and xyz as for
    host_resect; locate [F]: a mask (None: all frames); params: a dict of vsm_locate_params fields or the struct; n_tracks:
    override len(offsets) - 1 (argument tests).  Returns a Location object; raises VisoMatchError on VSM_EARG."""
    F, lo, off, fr, px, pt, us = _locate_inputs(n_frames, locate, offsets, obs_frames, uv, xyz, use)
    out = _locate_arrays(max(F, 0))
    got = _check(lib().vsm_host_locate(F, _ptr(lo), float(f), float(cu), float(cv), _n_tracks(off, n_tracks), _ptr(off), _ptr(fr), _ptr(px), _ptr(pt), _ptr(us),
                                       _params_ref(VsmLocateParams, locate_params, params), *[_ptr(a) for a in out]), "vsm_host_locate")
    assert got == F
    return Location(*out)


# ---- test hooks of the location's stages (include/visomatch.h, the debug section): rows without tracks, row r of a frame has
# the pixel uv[r] and the point xyz[r] ----

def _locate_rows(uv, xyz):
    px = np.ascontiguousarray(np.asarray(uv, dtype=np.float32).reshape(-1, 2))
    pt = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
    assert len(px) == len(pt)
    return px, pt


def _locate_tables(states, valid, K):
    st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, K, 12)
    va = np.ascontiguousarray(valid, dtype=np.uint8).reshape(-1, K)
    assert len(st) == len(va)
    return st, va


def host_locate_sample(seed, E, K):
    """vsm_host_locate_sample: picks [K, 6], the positions in [0, E) the K hypotheses of a frame with E eligible rows draw"""
    picks = np.zeros((max(int(K), 0), 6), np.int32)
    _check(lib().vsm_host_locate_sample(int(seed), int(E), int(K), _ptr(picks)), "vsm_host_locate_sample")
    return picks


def host_locate_fit(f, cu, cv, uv, xyz, picks, min_depth=1e-10, fill=0.0):
    """vsm_host_locate_fit on one frame of rows: picks [K, 6] -> (states [K, 12], valid [K]); a state the fit leaves unwritten
    stays `fill`"""
    px, pt = _locate_rows(uv, xyz)
    pk = np.ascontiguousarray(picks, dtype=np.int32).reshape(-1, 6)
    states, valid = np.full((len(pk), 12), fill, np.float64), np.zeros(len(pk), np.uint8)
    _check(lib().vsm_host_locate_fit(float(f), float(cu), float(cv), float(min_depth), len(px), _ptr(px), _ptr(pt), _ptr(pk), len(pk), _ptr(states), _ptr(valid)),
           "vsm_host_locate_fit")
    return states, valid


def host_locate_count(f, cu, cv, uv, xyz, states, valid, inlier_threshold=2.0, min_depth=1e-10):
    """vsm_host_locate_count on one frame of rows: states [K, 12], valid [K] -> counts [K]"""
    px, pt = _locate_rows(uv, xyz)
    va = np.ascontiguousarray(valid, dtype=np.uint8).ravel()
    st, va = _locate_tables(states, va, len(va))
    counts = np.zeros(len(va[0]), np.int32)
    _check(lib().vsm_host_locate_count(float(f), float(cu), float(cv), len(px), _ptr(px), _ptr(pt), _ptr(st), _ptr(va), len(counts), float(inlier_threshold),
                                       float(min_depth), _ptr(counts)), "vsm_host_locate_count")
    return counts


def _locate_frames(row_off, uv, xyz, job_frame, job_E):
    off = np.ascontiguousarray(row_off, dtype=np.int32)
    px, pt = _locate_rows(uv, xyz)
    jf, je = np.ascontiguousarray(job_frame, dtype=np.int32), np.ascontiguousarray(job_E, dtype=np.int32)
    assert len(jf) == len(je) and (len(off) == 0 or len(px) >= off[-1])
    return off, px, pt, jf, je


def device_locate_fit(f, cu, cv, row_off, uv, xyz, job_frame, job_E, picks, states, hvalid, min_depth=1e-10):
    """test hook: k_locate_fit alone, one launch.  Frames of rows (row_off [F + 1], uv [R, 2], xyz [R, 3]), jobs (job_frame,
    job_E [J]), picks [J, K, 6]; states [J, K, 12] and hvalid [J, K] go up as given and come back as new arrays"""
    off, px, pt, jf, je = _locate_frames(row_off, uv, xyz, job_frame, job_E)
    pk = np.ascontiguousarray(picks, dtype=np.int32)
    K = pk.shape[1] if pk.ndim == 3 else 0
    st, va = _locate_tables(np.array(states, dtype=np.float64), np.array(hvalid, dtype=np.uint8), max(K, 1))
    _check(lib().vsm_debug_locate_fit(float(f), float(cu), float(cv), float(min_depth), len(off) - 1, _ptr(off), _ptr(px), _ptr(pt), len(jf), _ptr(jf), _ptr(je),
                                      _ptr(pk), K, _ptr(st), _ptr(va)), "vsm_debug_locate_fit")
    return st, va


def device_locate_count(f, cu, cv, row_off, uv, xyz, job_frame, job_E, states, hvalid, inlier_threshold=2.0, min_depth=1e-10, launches=1):
    """test hook: k_locate_count alone on states [J, K, 12] and hvalid [J, K]; the counts are cleared once, then the kernel is
    launched `launches` times -> counts [J, K]"""
    off, px, pt, jf, je = _locate_frames(row_off, uv, xyz, job_frame, job_E)
    va = np.ascontiguousarray(hvalid, dtype=np.uint8)
    K = va.shape[1] if va.ndim == 2 else 0
    st, va = _locate_tables(states, va, max(K, 1))
    counts = np.zeros(va.shape, np.int32)
    _check(lib().vsm_debug_locate_count(float(f), float(cu), float(cv), len(off) - 1, _ptr(off), _ptr(px), _ptr(pt), len(jf), _ptr(jf), _ptr(je), K, _ptr(st),
                                        _ptr(va), float(inlier_threshold), float(min_depth), int(launches), _ptr(counts)), "vsm_debug_locate_count")
    return counts


def device_locate_winner(frame_job, job_E, counts, hvalid, states, min_inliers, fill=77):
    """test hook: k_locate_winner alone on counts, hvalid [J, K] and states [J, K, 12] -> (verdict, best, inliers [F], lin_poses
    [F, 12], lin_valid [F]); the outputs go up filled with `fill`"""
    fj, je = np.ascontiguousarray(frame_job, dtype=np.int32), np.ascontiguousarray(job_E, dtype=np.int32)
    cn = np.ascontiguousarray(counts, dtype=np.int32)
    K = cn.shape[1] if cn.ndim == 2 else 0
    st, va = _locate_tables(states, hvalid, max(K, 1))
    assert cn.shape == va.shape and len(cn) == len(je)
    F = len(fj)
    verdict, best, inliers = (np.full(F, fill, np.int32) for _ in range(3))
    lin, lin_valid = np.full((F, 12), float(fill), np.float64), np.full(F, fill, np.uint8)
    _check(lib().vsm_debug_locate_winner(F, _ptr(fj), len(je), _ptr(je), K, int(min_inliers), _ptr(cn), _ptr(va), _ptr(st), _ptr(verdict), _ptr(best),
                                         _ptr(inliers), _ptr(lin), _ptr(lin_valid)), "vsm_debug_locate_winner")
    return verdict, best, inliers, lin, lin_valid


REOBSERVE_REASONS = ("not_searched", "no_pose", "observed", "behind", "outside")
REOBSERVE_CODES = ("accepted", "empty_window", "over_max_cost", "ambiguous", "lost")
REOBSERVE_STATS = tuple("pairs_" + r for r in REOBSERVE_REASONS) + tuple("cand_" + c for c in REOBSERVE_CODES)
REOBSERVE_TIMINGS = ("gather_us", "upload_us", "kernels_us", "download_host_us")
REOBSERVE_ARRAYS = ("cand", "uv", "track_accepted", "frame_counts")


class Reobservation:
    """new observations found by projection (include/visomatch.h, vsm_reobserve_run): per candidate cand [n_cand, 7] int32
    {track, frame, feature, cost, second, n_window, code} (code 0 = accepted, REOBSERVE_CODES names the values) and uv [n_cand, 2]
    float64, the projection; track_accepted [T] int32; frame_counts [F, 2] int32 (candidates, accepted); stats: pairs per reason
    and candidates per code by name, timings: dict (empty for the host view).  pixels [n_cand, 2] float32, filled in by the
    binding from the records the call searched: the integer pixel of an accepted candidate's feature (zeros elsewhere)."""

    def __init__(self, cand, uv, track_accepted, frame_counts, stats=None, timings=None, pixels=None):
        self.cand, self.uv, self.track_accepted, self.frame_counts = cand, uv, track_accepted, frame_counts
        self.stats, self.timings = stats or {}, timings or {}
        self.pixels = np.zeros((len(cand), 2), np.float32) if pixels is None else pixels

    def _take_pixels(self, records_of):
        """records_of(g): frame g's feature records [n, 12]"""
        acc = self.accepted()
        for g in np.unique(self.cand[acc, 1]).tolist():
            i = acc[self.cand[acc, 1] == g]
            self.pixels[i] = np.asarray(records_of(g)).reshape(-1, 12)[self.cand[i, 2], :2].astype(np.float32)
        return self

    def __len__(self):
        return len(self.cand)

    @property
    def code(self):
        return self.cand[:, 6]

    def accepted(self):
        """the indices of the accepted candidates, ascending"""
        return np.nonzero(self.cand[:, 6] == 0)[0]

    def extend(self, offsets, obs_frames, uv, obs_feat):
        """the track set with the accepted observations merged in by ascending frame (a new one behind the old ones of its
        frame: there are none), over the same T tracks: (offsets, obs_frames, uv, obs_feat).  A new observation's pixel is its
        feature's integer pixel as float32.  The counterpart of Vetting.prune: the arrays feed triangulate, resect, vet,
        adjust and the next reobserve as they are."""
        off = np.asarray(offsets, dtype=np.int32)
        fr, ft = np.asarray(obs_frames, dtype=np.int32), np.asarray(obs_feat, dtype=np.int32)
        px = np.asarray(uv, dtype=np.float32).reshape(-1, 2)
        T = max(len(off) - 1, 0)
        assert len(fr) == len(ft) == len(px) == (off[-1] if T else 0) and len(self.track_accepted) == T
        acc = self.accepted()
        new = self.cand[acc]
        track = np.concatenate([np.repeat(np.arange(T, dtype=np.int64), np.diff(off)), new[:, 0].astype(np.int64)])
        frames = np.concatenate([fr, new[:, 1]]).astype(np.int32)
        feats = np.concatenate([ft, new[:, 2]]).astype(np.int32)
        pixels = np.concatenate([px, self.pixels[acc]])
        order = np.lexsort((np.arange(len(track)), frames, track))  # by (track, frame), the old observations first
        out_off = np.zeros(T + 1, np.int32)
        out_off[1:] = np.cumsum(np.diff(off) + self.track_accepted)
        return out_off, np.ascontiguousarray(frames[order]), np.ascontiguousarray(pixels[order]), np.ascontiguousarray(feats[order])


def reobserve_params(**kw):
    """vsm_reobserve_default_params with fields overridden by keyword"""
    return _default_params(VsmReobserveParams, "vsm_reobserve_default_params", kw)


def _reobserve_inputs(poses, pose_valid, search, offsets, obs_frames, obs_feat, xyz, use, ref_obs, feat_offsets, feat):
    po, pv = _pose_inputs(poses, pose_valid)
    se = _mask(search, len(po))
    off = np.ascontiguousarray(offsets, dtype=np.int32)
    fr, ft = np.ascontiguousarray(obs_frames, dtype=np.int32), np.ascontiguousarray(obs_feat, dtype=np.int32)
    assert len(fr) == len(ft)
    pt = None if xyz is None else np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
    us = None if use is None else np.ascontiguousarray(use, dtype=np.uint8)
    ro = None if ref_obs is None else np.ascontiguousarray(ref_obs, dtype=np.int32)
    assert all(a is None or len(a) >= len(off) - 1 for a in (pt, us, ro))
    fo = None if feat_offsets is None else np.ascontiguousarray(feat_offsets, dtype=np.int32)
    fe = None if feat is None else np.ascontiguousarray(np.asarray(feat, dtype=np.int32).reshape(-1, 12))
    assert fo is None or len(fo) == len(po) + 1
    return po, pv, se, off, fr, ft, pt, us, ro, fo, fe


def host_reobserve(poses, f, cu, cv, width, height, offsets, obs_frames, obs_feat, xyz, feat_offsets, feat, use=None, ref_obs=None, search=None, pose_valid=None,
                   params=None, n_tracks=None):
    """vsm_host_reobserve: the re-observation on one host thread - no GPU.  n_tracks: override len(offsets) - 1 (argument
    tests).  Returns a Reobservation object; raises VisoMatchError on VSM_EARG."""
    po, pv, se, off, fr, ft, pt, us, ro, fo, fe = _reobserve_inputs(poses, pose_valid, search, offsets, obs_frames, obs_feat, xyz, use, ref_obs, feat_offsets, feat)
    T = _n_tracks(off, n_tracks)
    prm = _params_ref(VsmReobserveParams, reobserve_params, params)
    head = (len(po), _ptr(po), _ptr(pv), _ptr(se), float(f), float(cu), float(cv), int(width), int(height), T, _ptr(off), _ptr(fr), _ptr(ft), _ptr(pt), _ptr(us),
            _ptr(ro), _ptr(fo), _ptr(fe), prm)
    n = _check(lib().vsm_host_reobserve(*head, 0, None, None, None, None, None), "vsm_host_reobserve")
    cand, uv = np.zeros((n, 7), np.int32), np.zeros((n, 2), np.float64)
    acc, fc, stats = np.zeros(max(T, 0), np.int32), np.zeros((len(po), 2), np.int32), np.zeros(10, np.int64)
    got = _check(lib().vsm_host_reobserve(*head, n, _ptr(cand), _ptr(uv), _ptr(acc), _ptr(fc), _ptr(stats)), "vsm_host_reobserve")
    assert got == n
    return Reobservation(cand, uv, acc, fc, dict(zip(REOBSERVE_STATS, stats.tolist())))._take_pixels(lambda g: fe[fo[g]:fo[g + 1]])


FUSE_CODES = ("fused", "empty_window", "over_max_cost", "ambiguous", "conflict", "outbid", "one_sided")
FUSE_STATS = tuple("pairs_" + r for r in REOBSERVE_REASONS) + tuple("cand_" + c for c in FUSE_CODES) + ("fusions",)
FUSE_TIMINGS = REOBSERVE_TIMINGS
FUSE_ARRAYS = ("prop", "uv", "partner", "fused_into", "offsets_after", "obs_src", "frame_counts")


class Fusion:
    """duplicate tracks joined (include/visomatch.h, vsm_fuse_run): per proposal prop [n_prop, 8] int32 {a, frame, feature, cost,
    second, n_window, code, b} (code 0 = fused, FUSE_CODES names the values) and uv [n_prop, 2] float64, the projection;
    partner [T] and fused_into [T] int32 (-1: none); the merged track set offsets_after [T + 1] and obs_src [n_obs] int32;
    frame_counts [F, 2] int32 (candidates, proposals); stats by name, timings: dict (empty for the host view)."""

    def __init__(self, prop, uv, partner, fused_into, offsets_after, obs_src, frame_counts, stats=None, timings=None):
        self.prop, self.uv, self.partner, self.fused_into = prop, uv, partner, fused_into
        self.offsets_after, self.obs_src, self.frame_counts = offsets_after, obs_src, frame_counts
        self.stats, self.timings = stats or {}, timings or {}

    def __len__(self):
        return len(self.prop)

    @property
    def code(self):
        return self.prop[:, 6]

    def fused(self):
        """the fusions [n, 2] int32: (survivor, absorbed), by ascending absorbed track"""
        gone = np.nonzero(self.fused_into >= 0)[0].astype(np.int32)
        return np.stack([self.fused_into[gone], gone], axis=1).astype(np.int32).reshape(-1, 2)

    def merge(self, obs_frames, uv, obs_feat):
        """the merged track set over the same T tracks: (offsets_after, obs_frames, uv, obs_feat), the observations gathered
        through obs_src - a survivor's own and the absorbed track's by ascending frame, an absorbed track empty.  The
        counterpart of Vetting.prune and Reobservation.extend: the arrays feed triangulate, adjust, vet, reobserve and the
        next fuse as they are (the points of the survivors want a new triangulation)."""
        fr, ft = np.asarray(obs_frames, dtype=np.int32), np.asarray(obs_feat, dtype=np.int32)
        px = np.asarray(uv, dtype=np.float32).reshape(-1, 2)
        assert len(fr) == len(ft) == len(px) == len(self.obs_src)
        src = self.obs_src
        return self.offsets_after.copy(), np.ascontiguousarray(fr[src]), np.ascontiguousarray(px[src]), np.ascontiguousarray(ft[src])


def fuse_params(**kw):
    """vsm_fuse_default_params with fields overridden by keyword"""
    return _default_params(VsmFuseParams, "vsm_fuse_default_params", kw)


def host_fuse(poses, f, cu, cv, width, height, offsets, obs_frames, obs_feat, xyz, feat_offsets, feat, use=None, ref_obs=None, search=None, pose_valid=None,
              params=None, n_tracks=None):
    """vsm_host_fuse: the fusion on one host thread - no GPU.  Arguments as host_reobserve.  Returns a Fusion object; raises
    VisoMatchError on VSM_EARG."""
    po, pv, se, off, fr, ft, pt, us, ro, fo, fe = _reobserve_inputs(poses, pose_valid, search, offsets, obs_frames, obs_feat, xyz, use, ref_obs, feat_offsets, feat)
    T = _n_tracks(off, n_tracks)
    prm = _params_ref(VsmFuseParams, fuse_params, params)
    head = (len(po), _ptr(po), _ptr(pv), _ptr(se), float(f), float(cu), float(cv), int(width), int(height), T, _ptr(off), _ptr(fr), _ptr(ft), _ptr(pt), _ptr(us),
            _ptr(ro), _ptr(fo), _ptr(fe), prm)
    n = _check(lib().vsm_host_fuse(*head, 0, None, None, None, None, None, None, None, None), "vsm_host_fuse")
    T = max(T, 0)
    out = (np.zeros((n, 8), np.int32), np.zeros((n, 2), np.float64), np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T + 1, np.int32),
           np.zeros(len(fr), np.int32), np.zeros((len(po), 2), np.int32))
    stats = np.zeros(len(FUSE_STATS), np.int64)
    got = _check(lib().vsm_host_fuse(*head, n, *[_ptr(o) for o in out], _ptr(stats)), "vsm_host_fuse")
    assert got == n
    return Fusion(*out, dict(zip(FUSE_STATS, stats.tolist())))


_NO_PARAMS = object()  # params=_NO_PARAMS: a NULL params pointer (argument tests)


def remove_outliers(matches, method, w, h, gpu=False, gpu_ties=False, copies=1, threads=1, **params):
    """Matcher::removeOutliers + computePriorStatistics on a match list: host code of the per-frame path (gpu=False; threads > 1:
    split over fork-join threads the way vsm_match runs a frame's final list) or the GPU-resident chain of the look-ahead path;
    returns (survivors, ranges in device layout, kernel microseconds)"""
    p = default_params()
    for k, v in params.items():
        setattr(p, k, v)
    m = np.ascontiguousarray(matches, dtype=P_MATCH)
    n = len(m)
    out = np.zeros(max(n, 1), dtype=P_MATCH)
    ub, vb = -(-w // p.match_binsize), -(-h // p.match_binsize)
    rg = np.zeros((ub * vb, 16), dtype=np.float32)
    us = C.c_double(0)
    if gpu:
        k = lib().vsm_debug_dc2(C.byref(p), m.ctypes.data_as(C.c_void_p), n, method, int(gpu_ties), copies, out.ctypes.data_as(C.c_void_p),
                                len(out), rg.ctypes.data_as(C.c_void_p), w, h, C.cast(C.byref(us), C.c_void_p))
    elif threads > 1:
        k = lib().vsm_host_outliers_and_prior_threads(C.byref(p), m.ctypes.data_as(C.c_void_p), n, method, out.ctypes.data_as(C.c_void_p), len(out),
                                                      rg.ctypes.data_as(C.c_void_p), w, h, threads)
    else:
        k = lib().vsm_host_outliers_and_prior(C.byref(p), m.ctypes.data_as(C.c_void_p), n, method, out.ctypes.data_as(C.c_void_p), len(out),
                                              rg.ctypes.data_as(C.c_void_p), w, h)
    if k < 0:
        raise VisoMatchError(f"remove_outliers: code {k}")
    return out[:k].copy(), rg, us.value


def _refine_inputs(lists):
    """P match lists -> (the arrays, their lengths, the pointer table the library takes)"""
    ms = [np.ascontiguousarray(m, dtype=P_MATCH) for m in lists]
    cnt = np.array([len(m) for m in ms], dtype=np.int32)
    return ms, cnt, (C.c_void_p * max(len(ms), 1))(*[m.ctypes.data if len(m) else None for m in ms])


def _refine_outputs(counts):
    outs = [np.zeros(max(int(n), 0), dtype=P_MATCH) for n in counts]
    return outs, np.full(len(outs), -1, dtype=np.int32), (C.c_void_p * max(len(outs), 1))(*[o.ctypes.data if len(o) else None for o in outs])


def refine_check(w, h, lists, counts=None):
    """test hook: the list checks of Matcher.refine_lists for frames of w x h pixels, host arithmetic only -> the return code
    (0, or Matcher.EARG); counts: the lengths handed to the library instead of the lists' own"""
    ms, cnt, ptrs = _refine_inputs(lists)
    if counts is not None:
        cnt = np.ascontiguousarray(counts, dtype=np.int32)
    return lib().vsm_debug_refine_check(int(w), int(h), ptrs, _ptr(cnt), len(ms))


def device_parabolic_apply(lists, records, counts=None):
    """test hook: k_parabolic_apply alone over len(lists) pairs in one launch.  lists[k]: n_k matches, records[k]:
    [n_k, 3, 12] int32 {status, du, dv, c0..c8} per relocation step -> the lists after the fits, failed matches removed.
    counts: the lengths handed to the library instead of the lists' own (argument checks)."""
    ms, cnt, ptrs = _refine_inputs(lists)
    rs = [np.ascontiguousarray(r, dtype=np.int32).reshape(-1, 3, 12) for r in records]
    assert len(rs) == len(ms) and all(len(r) == len(m) for r, m in zip(rs, ms))
    rptrs = (C.c_void_p * max(len(rs), 1))(*[r.ctypes.data if len(r) else None for r in rs])
    if counts is not None:
        cnt = np.ascontiguousarray(counts, dtype=np.int32)
    outs, oc, optrs = _refine_outputs([len(m) for m in ms])
    _check(lib().vsm_debug_parabolic_apply(ptrs, rptrs, _ptr(cnt), len(ms), optrs, _ptr(oc)), "vsm_debug_parabolic_apply")
    return [o[:n].copy() for o, n in zip(outs, oc)]


def host_parabolic_fits(records, uv):
    """the host's least-squares tail of the sub-pixel fit (vsm_host_parabolic_update, no GPU) on records [n, 12] int32
    {-, du, dv, c0..c8} and targets uv [n, 2] float32 -> (uv after the fits, ok [n])"""
    r = np.ascontiguousarray(records, dtype=np.int32).reshape(-1, 12)
    out = np.array(uv, dtype=np.float32).reshape(-1, 2).copy()
    assert len(out) == len(r)
    ok = np.zeros(len(r), dtype=np.int32)
    _check(lib().vsm_host_parabolic_fits(_ptr(r), len(r), _ptr(out), _ptr(ok)), "vsm_host_parabolic_fits")
    return out, ok


COMPACT_KEY_GUARD = 8


def device_compact_keys(flags, raws, key_caps, method=2, pass_=1, old_keys=False):
    """test hook: the matching passes' compaction over len(flags) pairs in one launch.  flags[k]: int32 [n_k] acceptance flags,
    raws[k]: [n_k] per-query records, key_caps[k]: capacity of pair k's key array -> per pair (list with one guard record,
    count, keys with COMPACT_KEY_GUARD guard words); what the kernels did not write holds 0xA5 bytes.  old_keys 1: the keys by
    k_dc2_keys behind the plain compaction; 2: the keys as the fused store leaves them in its host-mapped second target."""
    fs = [np.ascontiguousarray(f, dtype=np.int32) for f in flags]
    rs = [np.ascontiguousarray(r, dtype=P_MATCH) for r in raws]
    assert len(fs) == len(rs) == len(key_caps) and all(len(f) == len(r) for f, r in zip(fs, rs))
    nq = np.array([len(f) for f in fs], dtype=np.int32)
    caps = np.ascontiguousarray(key_caps, dtype=np.int32)
    lists = [np.zeros(len(f) + 1, dtype=P_MATCH) for f in fs]
    keys = [np.zeros(int(c) + COMPACT_KEY_GUARD, dtype=np.uint64) for c in caps]
    counts = np.full(len(fs), -1, dtype=np.int32)
    tab = lambda arrs: (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    _check(lib().vsm_debug_compact_keys(int(method), int(pass_), len(fs), _ptr(nq), tab(fs), tab(rs), _ptr(caps), int(old_keys), tab(lists),
                                        _ptr(counts), tab(keys)), "vsm_debug_compact_keys")
    return [(l, int(n), k) for l, n, k in zip(lists, counts, keys)]


def local_cpus():
    """the CPUs of the GPU's NUMA node the library keeps its own host threads on (after the first Matcher exists); [] = no
    restriction.  os.sched_setaffinity(0, local_cpus()) puts the calling thread there too."""
    buf = (C.c_int32 * 1024)()
    n = lib().vsm_local_cpus(C.cast(buf, C.c_void_p), 1024)
    return [int(buf[i]) for i in range(min(n, 1024))]


def forkjoin_cpus():
    """the CPUs of the L3 domain the per-frame path's fork-join threads share (after the first Matcher exists); [] = none.
    os.sched_setaffinity(0, forkjoin_cpus()) puts the thread that calls match_features / process beside them."""
    buf = (C.c_int32 * 1024)()
    n = lib().vsm_forkjoin_cpus(C.cast(buf, C.c_void_p), 1024)
    return [int(buf[i]) for i in range(min(n, 1024))]


def default_params():
    p = VsmParams()
    lib().vsm_default_params(C.byref(p))
    return p


def _order_behind_torch(handle, *tensors):
    """device-resident inputs: the library reads them asynchronously on its own stream, so its stream is made to wait for
    whatever torch's current stream holds (the kernels or copies that produce the tensors) - vsm_wait_for_stream"""
    import torch
    dev = tensors[0].device
    _check(lib().vsm_wait_for_stream(handle, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "vsm_wait_for_stream")


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class Matcher:
    """Drop-in mirror of the reference Matcher.  Images: (H,W) uint8 numpy arrays (host path,
    vsm_push_back) or CUDA/HIP torch tensors (device-resident path, vsm_push_back_device)."""

    OK, EDIMS, ENOTREADY, EHIP, EARG = 0, -1, -2, -3, -4

    _inputs = None
    _n_pairs = 0  # pairs of the last successful match_pairs call
    _pairs_frames = _track_frames = None  # frames of the last successful match_pairs / tracks or pair_tracks call

    def __init__(self, stage_capture=False, options=None, **params):
        """params: fields of the reference's Matcher::parameters; options: measurement / test switches of the handle
        (vsm_set_option: "seq_chunk", "dc_gpu", ...), applied right after creation"""
        L = lib()
        p = default_params()
        for k, v in params.items():
            if not hasattr(p, k):
                raise TypeError(f"unknown matcher parameter {k}")
            setattr(p, k, v)
        self.params = p
        self.h = L.vsm_create(C.byref(p))
        if not self.h:
            raise VisoMatchError("vsm_create failed: no usable HIP device (the matcher has no CPU path)")
        self.h = C.c_void_p(self.h)
        if stage_capture:
            L.vsm_set_stage_capture(self.h, 1)
        # (tools: VSM_PY_OPTIONS="seq_fstreams=2,seq_chunk=50" reaches handles created by scripts that pass no options)
        env_opts = dict(kv.split("=") for kv in os.environ.get("VSM_PY_OPTIONS", "").split(",") if "=" in kv)
        for k, v in {**env_opts, **(options or {})}.items():
            self.set_option(k, int(v))

    # --- reference API -------------------------------------------------------------------
    def set_intrinsics(self, f, cu, cv, base):
        lib().vsm_set_intrinsics(self.h, f, cu, cv, base)

    def push_back(self, I1, I2=None, replace=False):
        L = lib()
        if _is_torch(I1):
            assert I1.is_cuda and I1.dtype.__str__() == "torch.uint8" and I1.dim() == 2
            h, w = I1.shape
            bpl = I1.stride(0)
            assert I1.stride(1) == 1
            p2 = None
            if I2 is not None:
                assert I2.is_cuda and I2.shape == I1.shape and I2.stride() == I1.stride()
                p2 = C.c_void_p(I2.data_ptr())
            _order_behind_torch(self.h, I1)
            self._inputs = (I1, I2)      # the push reads them asynchronously: kept alive until the next push
            return L.vsm_push_back_device(self.h, C.c_void_p(I1.data_ptr()), p2, w, h, bpl, int(replace))
        I1 = np.ascontiguousarray(I1, dtype=np.uint8)
        h, w = I1.shape
        p2 = None
        if I2 is not None:
            I2 = np.ascontiguousarray(I2, dtype=np.uint8)
            assert I2.shape == I1.shape
            p2 = I2.ctypes.data_as(C.c_void_p)
        return L.vsm_push_back(self.h, I1.ctypes.data_as(C.c_void_p), p2, w, h, w, int(replace))

    def match_features(self, method, Tr_delta=None):
        tp = None
        if Tr_delta is not None:
            t = np.ascontiguousarray(np.asarray(Tr_delta, dtype=np.float64).reshape(-1)[:12])
            tp = t.ctypes.data_as(C.c_void_p)
        rc = lib().vsm_match(self.h, method, tp)
        return rc if rc == self.ENOTREADY else _check(rc, "vsm_match")

    def get_matches(self):
        n = lib().vsm_num_matches(self.h)
        out = np.zeros(n, dtype=P_MATCH)
        if n:
            lib().vsm_get_matches(self.h, out.ctypes.data_as(C.c_void_p), n)
        return out

    def bucket_features(self, max_features, bucket_width, bucket_height):
        lib().vsm_bucket(self.h, max_features, bucket_width, bucket_height)

    def get_gain(self, inliers):
        a = np.ascontiguousarray(inliers, dtype=np.int32)
        return float(lib().vsm_gain(self.h, a.ctypes.data_as(C.c_void_p), len(a)))

    # --- the face the golden drivers use (same names as oracle.bindings.CpuMatcher) ---------
    def match(self, method, Tr=None):
        return self.match_features(method, Tr) == self.OK

    matches = get_matches
    bucket = bucket_features
    gain = get_gain

    def stage(self, s):
        n = lib().vsm_stage_size(self.h, s)
        out = np.zeros(n, dtype=P_MATCH)
        if n:
            lib().vsm_stage_get(self.h, s, out.ctypes.data_as(C.c_void_p), n)
        return out

    def ranges(self):
        n = lib().vsm_num_ranges(self.h)
        out = np.zeros((n, 4, 4), dtype=np.float32)
        if n:
            lib().vsm_get_ranges(self.h, out.ctypes.data_as(C.c_void_p), n)
        return out

    def features(self, which):
        w = FEATURE_SETS[which] if isinstance(which, str) else which
        n = lib().vsm_num_features(self.h, w)
        out = np.zeros((n, 12), dtype=np.int32)
        if n:
            got = lib().vsm_get_features(self.h, w, out.ctypes.data_as(C.c_void_p), n)
            assert got == n
        return out

    def gradients(self, which, full):
        n = lib().vsm_get_gradients(self.h, which, int(full), None, None)
        if n == 0:
            return None, None
        du = np.zeros(n, dtype=np.uint8)
        dv = np.zeros(n, dtype=np.uint8)
        lib().vsm_get_gradients(self.h, which, int(full), du.ctypes.data_as(C.c_void_p), dv.ctypes.data_as(C.c_void_p))
        return du, dv

    def filter_responses(self):
        n = lib().vsm_get_filter_responses(self.h, None, None)
        if n == 0:
            return None, None
        f1 = np.zeros(n, dtype=np.int16)
        f2 = np.zeros(n, dtype=np.int16)
        lib().vsm_get_filter_responses(self.h, f1.ctypes.data_as(C.c_void_p), f2.ctypes.data_as(C.c_void_p))
        return f1, f2

    def refine_lists(self, method, lists, counts=None):
        """test hook: the refinement kernels alone on len(lists) caller-given pass-2 lists as the pairs of one launch, over the
        frames pushed last (vsm_debug_refine; the last match result is gone afterwards) -> the refined lists.  counts: the
        lengths handed to the library instead of the lists' own (argument checks).  A rejected argument raises."""
        ms, cnt, ptrs = _refine_inputs(lists)
        if counts is not None:
            cnt = np.ascontiguousarray(counts, dtype=np.int32)
        outs, oc, optrs = _refine_outputs([len(m) for m in ms])
        _check(lib().vsm_debug_refine(self.h, int(method), ptrs, _ptr(cnt), len(ms), optrs, _ptr(oc)), "vsm_debug_refine")
        return [o[:n].copy() for o, n in zip(outs, oc)]

    def counters(self):
        c = np.zeros(5, dtype=np.int64)
        lib().vsm_get_counters(self.h, c.ctypes.data_as(C.c_void_p))
        return c

    def timings(self):
        t = np.zeros(5, dtype=np.float64)
        lib().vsm_get_timings(self.h, t.ctypes.data_as(C.c_void_p))
        return dict(zip(("pass1_gpu_us", "pass1_host_us", "pass2_gpu_us", "final_host_us", "total_us"), t.tolist()))

    # --- look-ahead API -------------------------------------------------------------------
    def run_sequence(self, left, right, method, Tr_delta=None, Tr_valid=None, fetch=True):
        """left/right: [F,H,W] uint8 numpy arrays (host) or CUDA torch tensors (resident in HBM);
        returns the list of per-frame match arrays (getMatches() after each frame), or, with
        fetch=False, nothing (the lists stay in the handle: sequence_matches(f))."""
        L = lib()
        if _is_torch(left):
            assert left.is_cuda and left.dim() == 3 and left.stride(2) == 1
            F, h, w = left.shape
            bpl, fs = left.stride(1), left.stride(0)
            _order_behind_torch(self.h, left)
            pl = C.c_void_p(left.data_ptr())
            pr = None
            if right is not None:
                assert right.is_cuda and right.shape == left.shape and right.stride() == left.stride()
                pr = C.c_void_p(right.data_ptr())
            dev = 1
        else:
            left = np.ascontiguousarray(left, dtype=np.uint8)
            F, h, w = left.shape
            bpl, fs = w, w * h
            pl = left.ctypes.data_as(C.c_void_p)
            pr = None
            if right is not None:
                right = np.ascontiguousarray(right, dtype=np.uint8)
                assert right.shape == left.shape
                pr = right.ctypes.data_as(C.c_void_p)
            dev = 0
        tp = vp_ = None
        if Tr_delta is not None:
            t = np.ascontiguousarray(np.asarray(Tr_delta, dtype=np.float64).reshape(F, -1)[:, :12])
            tp = t.ctypes.data_as(C.c_void_p)
            if Tr_valid is not None:
                v = np.ascontiguousarray(np.asarray(Tr_valid).astype(np.uint8))
                vp_ = v.ctypes.data_as(C.c_void_p)
        _check(L.vsm_sequence_run(self.h, pl, pr, fs, dev, F, w, h, bpl, method, tp, vp_), "vsm_sequence_run")
        return [self.sequence_matches(f) for f in range(F)] if fetch else None

    def sequence_matches(self, f):
        L = lib()
        n = L.vsm_sequence_num_matches(self.h, f)
        a = np.zeros(n, dtype=P_MATCH)
        if n:
            L.vsm_sequence_get_matches(self.h, f, a.ctypes.data_as(C.c_void_p), n)
        return a

    # --- arbitrary frame pairs of an image set ---------------------------------------------
    def match_pairs(self, left, right, pairs, method, Tr_delta=None, Tr_valid=None, fetch=True):
        """left/right: [F,H,W] uint8 numpy arrays (host) or CUDA torch tensors (resident in HBM; a view with row and frame
        strides is read in place), right=None: mono input.  pairs: [(previous frame, current frame), ...].  Tr_delta: None
        or one matrix per pair ([P,4,4], [P,3,4] or [P,12]), Tr_valid: None or a flag per pair.  Returns the list of per-pair
        match arrays - for (a, b): getMatches() of a fresh matcher after pushBack(a), pushBack(b), matchFeatures(method, Tr) -
        or, with fetch=False, nothing (the lists stay in the handle: pair_matches(k)).  Every frame goes through the image
        side once, however many pairs name it."""
        L = lib()
        if _is_torch(left):
            assert left.is_cuda and left.dtype.__str__() == "torch.uint8" and left.dim() == 3 and left.stride(2) == 1
            F, h, w = left.shape
            bpl, fs = left.stride(1), left.stride(0)
            _order_behind_torch(self.h, left)
            pl = C.c_void_p(left.data_ptr())
            pr = None
            if right is not None:
                assert right.is_cuda and right.dtype == left.dtype and right.shape == left.shape and right.stride() == left.stride()
                pr = C.c_void_p(right.data_ptr())
            dev = 1
        else:
            left = np.ascontiguousarray(left, dtype=np.uint8)
            F, h, w = left.shape
            bpl, fs = w, w * h
            pl = left.ctypes.data_as(C.c_void_p)
            pr = None
            if right is not None:
                right = np.ascontiguousarray(right, dtype=np.uint8)
                assert right.shape == left.shape
                pr = right.ctypes.data_as(C.c_void_p)
            dev = 0
        pa = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        P = len(pa)
        tp = vp_ = None
        if Tr_delta is not None:
            t = np.ascontiguousarray(np.asarray(Tr_delta, dtype=np.float64).reshape(P, -1)[:, :12])
            tp = t.ctypes.data_as(C.c_void_p)
            if Tr_valid is not None:
                v = np.ascontiguousarray(np.asarray(Tr_valid).astype(np.uint8))
                assert v.shape == (P,)
                vp_ = v.ctypes.data_as(C.c_void_p)
        _check(L.vsm_pairs_run(self.h, pl, pr, fs, dev, F, w, h, bpl, method, pa.ctypes.data_as(C.c_void_p), P, tp, vp_), "vsm_pairs_run")
        self._n_pairs, self._pairs_frames = P, F
        return [self.pair_matches(k) for k in range(P)] if fetch else None

    def pair_matches(self, k):
        L = lib()
        n = L.vsm_pairs_num_matches(self.h, k)
        a = np.zeros(n, dtype=P_MATCH)
        if n:
            L.vsm_pairs_get_matches(self.h, k, a.ctypes.data_as(C.c_void_p), n)
        return a

    # --- feature tracks from pair match lists --------------------------------------------------
    def _tracks_result(self, rc, what, n_pairs):
        L = lib()
        _check(rc, what)
        T, n_obs = L.vsm_tracks_count(self.h), L.vsm_tracks_num_obs(self.h)
        offsets, obs, flags = np.zeros(T + 1, np.int32), np.zeros((n_obs, 4), np.int32), np.zeros(T, np.uint8)
        L.vsm_tracks_get(self.h, offsets.ctypes.data_as(C.c_void_p), obs.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p))
        of_pairs = []
        for k in range(n_pairs):
            n = L.vsm_tracks_of_matches(self.h, k, None, 0)
            a = np.zeros(n, np.int32)
            if n:
                L.vsm_tracks_of_matches(self.h, k, a.ctypes.data_as(C.c_void_p), n)
            of_pairs.append(a)
        return Tracks(offsets, obs, flags, of_pairs, *_stage_dicts(self.h, L.vsm_tracks_get_stats, TRACK_STATS, L.vsm_tracks_get_timings, TRACK_TIMINGS))

    def tracks(self, n_frames, pairs, lists, side=0, min_length=2):
        """vsm_tracks_run: the connected components of the match lists `lists` (one P_MATCH array per (previous, current)
        pair of `pairs`), on the device.  Returns a Tracks object."""
        pa, ls, ptrs, cnt = _track_inputs(pairs, lists)
        rc = lib().vsm_tracks_run(self.h, int(n_frames), pa.ctypes.data_as(C.c_void_p), len(pa), ptrs, cnt.ctypes.data_as(C.c_void_p),
                                  int(side), int(min_length))
        res = self._tracks_result(rc, "vsm_tracks_run", len(pa))
        self._track_frames = int(n_frames)
        return res

    def pair_tracks(self, side=0, min_length=2):
        """vsm_pairs_tracks: the tracks of the last match_pairs call's lists (fetched or not), which stay as they are"""
        rc = lib().vsm_pairs_tracks(self.h, int(side), int(min_length))
        res = self._tracks_result(rc, "vsm_pairs_tracks", self._n_pairs)
        self._track_frames = self._pairs_frames
        return res

    # --- tracks into 3-D points -------------------------------------------------------------------
    def _points_result(self, rc, what):
        L = lib()
        _check(rc, what)
        out = _points_arrays(L.vsm_points_count(self.h))
        L.vsm_points_get(self.h, *[_ptr(a) for a in out])
        return Points(*out, *_stage_dicts(self.h, L.vsm_points_get_stats, POINT_STATUS, L.vsm_points_get_timings, POINT_TIMINGS))

    def triangulate(self, poses, f, cu, cv, offsets, obs_frames, uv, flags=None, pose_valid=None, params=None, n_tracks=None):
        """vsm_triangulate_run: the 3-D point of every track, on the device.  poses [F, 12] (or [F, 3, 4] / [F, 4, 4]) camera to
        world; offsets [T + 1], obs_frames [n_obs], uv [n_obs, 2]; params: a dict of vsm_triangulate_params fields or the
        struct.  Returns a Points object."""
        po, pv, off, fr, px, fl = _triangulate_inputs(poses, pose_valid, offsets, obs_frames, uv, flags)
        T = _n_tracks(off, n_tracks)
        rc = lib().vsm_triangulate_run(self.h, len(po), _ptr(po), _ptr(pv), float(f), float(cu), float(cv), T, _ptr(off), _ptr(fr), _ptr(px), _ptr(fl),
                                       _params_ref(VsmTriangulateParams, triangulate_params, params))
        return self._points_result(rc, "vsm_triangulate_run")

    def track_points(self, poses, f, cu, cv, lists=None, pose_valid=None, params=None, counts=None):
        """vsm_tracks_triangulate: the 3-D points of the handle's last track result.  lists: the match lists the tracks were
        built from (None: those of the last match_pairs call, for tracks from pair_tracks).  counts: override the lists' lengths
        (argument tests)."""
        po, pv = _pose_inputs(poses, pose_valid, self._track_frames)  # (the library reads one pose per frame of the track call)
        ls, ptrs, cnt = _optional_lists(lists, counts)
        rc = lib().vsm_tracks_triangulate(self.h, ptrs, _ptr(cnt), _ptr(po), _ptr(pv), float(f), float(cu), float(cv),
                                          _params_ref(VsmTriangulateParams, triangulate_params, params))
        return self._points_result(rc, "vsm_tracks_triangulate")

    # --- poses refined against the points ---------------------------------------------------------
    def _resect_result(self, rc, what):
        L = lib()
        _check(rc, what)
        out = _resect_arrays(L.vsm_resect_count(self.h))
        L.vsm_resect_get(self.h, *[_ptr(a) for a in out])
        return Resection(*out, *_stage_dicts(self.h, L.vsm_resect_get_stats, RESECT_STATUS, L.vsm_resect_get_timings, RESECT_TIMINGS))

    def resect(self, poses, f, cu, cv, offsets, obs_frames, uv, xyz, use=None, refine=None, pose_valid=None, params=None, n_tracks=None):
        """vsm_resect_run: every frame's pose refined against the points it sees, on the device.  poses [F, 12] (or [F, 3, 4] /
        [F, 4, 4]) camera to world; the tracks as for triangulate; xyz [T, 3]; use [T] and refine [F]: masks (None: all);
        params: a dict of vsm_resect_params fields or the struct.  Returns a Resection object."""
        po, pv, rf, off, fr, px, pt, us = _resect_inputs(poses, pose_valid, refine, offsets, obs_frames, uv, xyz, use)
        T = _n_tracks(off, n_tracks)
        rc = lib().vsm_resect_run(self.h, len(po), _ptr(po), _ptr(pv), _ptr(rf), float(f), float(cu), float(cv), T, _ptr(off), _ptr(fr), _ptr(px), _ptr(pt),
                                  _ptr(us), _params_ref(VsmResectParams, resect_params, params))
        return self._resect_result(rc, "vsm_resect_run")

    def resect_points(self, poses, f, cu, cv, lists=None, refine=None, pose_valid=None, params=None, counts=None):
        """vsm_points_resect: the same on the handle's last track and point results (the kept points; lists as for
        track_points)."""
        po, pv = _pose_inputs(poses, pose_valid, self._track_frames)
        rf = _mask(refine, len(po))
        ls, ptrs, cnt = _optional_lists(lists, counts)
        rc = lib().vsm_points_resect(self.h, ptrs, _ptr(cnt), _ptr(po), _ptr(pv), _ptr(rf), float(f), float(cu), float(cv),
                                     _params_ref(VsmResectParams, resect_params, params))
        return self._resect_result(rc, "vsm_points_resect")

    # --- observations vetted by reprojection error -----------------------------------------------
    def _vet_result(self, rc, what):
        L = lib()
        _check(rc, what)
        T, n_obs, n_kept = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        L.vsm_vet_count(self.h, C.byref(T), C.byref(n_obs), C.byref(n_kept))
        out = _vet_arrays(T.value, n_obs.value, L.vsm_vet_get_frames(self.h, None), n_kept.value)
        L.vsm_vet_get_obs(self.h, _ptr(out[0]), _ptr(out[1]))
        L.vsm_vet_get_tracks(self.h, *[_ptr(a) for a in out[2:8]])
        L.vsm_vet_get_frames(self.h, _ptr(out[8]))
        L.vsm_vet_get_kept(self.h, _ptr(out[9]), _ptr(out[10]))
        return Vetting(*out, *_stage_dicts(self.h, L.vsm_vet_get_stats, VET_STATS, L.vsm_vet_get_timings, VET_TIMINGS))

    def vet(self, poses, f, cu, cv, offsets, obs_frames, uv, xyz, use=None, pose_valid=None, params=None, n_tracks=None):
        """vsm_vet_run: every observation's reprojection residual at the poses and points, the verdicts per observation, track
        and frame, and the pruned track set, on the device.  Arguments as for resect, without refine; params: a dict of
        vsm_vet_params fields or the struct.  Returns a Vetting object."""
        po, pv, off, fr, px, pt, us = _vet_inputs(poses, pose_valid, offsets, obs_frames, uv, xyz, use)
        T = _n_tracks(off, n_tracks)
        rc = lib().vsm_vet_run(self.h, len(po), _ptr(po), _ptr(pv), float(f), float(cu), float(cv), T, _ptr(off), _ptr(fr), _ptr(px), _ptr(pt), _ptr(us),
                               _params_ref(VsmVetParams, vet_params, params))
        return self._vet_result(rc, "vsm_vet_run")

    def vet_points(self, poses, f, cu, cv, lists=None, pose_valid=None, params=None, counts=None):
        """vsm_points_vet: the same on the handle's last track and point results (the kept points; lists as for track_points)"""
        po, pv = _pose_inputs(poses, pose_valid, self._track_frames)
        ls, ptrs, cnt = _optional_lists(lists, counts)
        rc = lib().vsm_points_vet(self.h, ptrs, _ptr(cnt), _ptr(po), _ptr(pv), float(f), float(cu), float(cv),
                                  _params_ref(VsmVetParams, vet_params, params))
        return self._vet_result(rc, "vsm_points_vet")

    # --- poses and points adjusted jointly ----------------------------------------------------------
    def _adjust_result(self, rc, what):
        L = lib()
        _check(rc, what)
        F, T, n = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        L.vsm_adjust_count(self.h, C.byref(F), C.byref(T), C.byref(n))
        fa, ta, ha = _adjust_arrays(F.value, T.value, n.value)
        L.vsm_adjust_get_frames(self.h, *[_ptr(a) for a in fa])
        L.vsm_adjust_get_tracks(self.h, *[_ptr(a) for a in ta])
        L.vsm_adjust_get_history(self.h, *[_ptr(a) for a in ha])
        return Adjustment(*fa, *ta, _adjust_history(ha, n.value), *_stage_dicts(self.h, L.vsm_adjust_get_stats, ADJUST_STATS, L.vsm_adjust_get_timings, ADJUST_TIMINGS))

    def adjust(self, poses, f, cu, cv, offsets, obs_frames, uv, xyz, use=None, refine=None, pose_valid=None, params=None, n_tracks=None):
        """vsm_adjust_run: poses and points adjusted jointly, on the device.  Arguments as for resect; params: a dict of
        vsm_adjust_params fields or the struct.  Returns an Adjustment object."""
        po, pv, rf, off, fr, px, pt, us = _resect_inputs(poses, pose_valid, refine, offsets, obs_frames, uv, xyz, use)
        T = _n_tracks(off, n_tracks)
        rc = lib().vsm_adjust_run(self.h, len(po), _ptr(po), _ptr(pv), _ptr(rf), float(f), float(cu), float(cv), T, _ptr(off), _ptr(fr), _ptr(px), _ptr(pt),
                                  _ptr(us), _params_ref(VsmAdjustParams, adjust_params, params))
        return self._adjust_result(rc, "vsm_adjust_run")

    def adjust_points(self, poses, f, cu, cv, lists=None, refine=None, pose_valid=None, params=None, counts=None):
        """vsm_points_adjust: the same on the handle's last track and point results (the kept points; lists as for
        track_points)."""
        po, pv = _pose_inputs(poses, pose_valid, self._track_frames)
        rf = _mask(refine, len(po))
        ls, ptrs, cnt = _optional_lists(lists, counts)
        rc = lib().vsm_points_adjust(self.h, ptrs, _ptr(cnt), _ptr(po), _ptr(pv), _ptr(rf), float(f), float(cu), float(cv),
                                     _params_ref(VsmAdjustParams, adjust_params, params))
        return self._adjust_result(rc, "vsm_points_adjust")

    # --- frames without a pose located against the points ------------------------------------------
    def _locate_result(self, rc, what):
        L = lib()
        _check(rc, what)
        out = _locate_arrays(L.vsm_locate_count(self.h))
        L.vsm_locate_get(self.h, *[_ptr(a) for a in out])
        return Location(*out, *_stage_dicts(self.h, L.vsm_locate_get_stats, LOCATE_STATUS, L.vsm_locate_get_timings, LOCATE_TIMINGS))

    def locate_hypotheses(self):
        """test hook (vsm_debug_locate_hypotheses): every hypothesis of the last location as the call left it ->
        (picks [J, K, 6], states [J, K, 12], hvalid [J, K], counts [J, K])"""
        J, K = C.c_int32(0), C.c_int32(0)
        sizes = (C.cast(C.byref(J), C.c_void_p), C.cast(C.byref(K), C.c_void_p))
        _check(lib().vsm_debug_locate_hypotheses(self.h, None, None, None, None, *sizes), "vsm_debug_locate_hypotheses")
        j, k = J.value, K.value
        picks, states, hvalid, counts = np.zeros((j, k, 6), np.int32), np.zeros((j, k, 12), np.float64), np.zeros((j, k), np.uint8), np.zeros((j, k), np.int32)
        _check(lib().vsm_debug_locate_hypotheses(self.h, _ptr(picks), _ptr(states), _ptr(hvalid), _ptr(counts), *sizes), "vsm_debug_locate_hypotheses")
        return picks, states, hvalid, counts

    def locate(self, n_frames, f, cu, cv, offsets, obs_frames, uv, xyz, use=None, locate=None, params=None, n_tracks=None):
        """vsm_locate_run: every asked-for frame's pose from its observations of the points alone, on the device - RANSAC over a
        linear six-point resection, the winner refined by the resection.  The tracks and xyz as for resect; locate [F]: a mask
        (None: all frames); params: a dict of vsm_locate_params fields or the struct.  Returns a Location object."""
        F, lo, off, fr, px, pt, us = _locate_inputs(n_frames, locate, offsets, obs_frames, uv, xyz, use)
        rc = lib().vsm_locate_run(self.h, F, _ptr(lo), float(f), float(cu), float(cv), _n_tracks(off, n_tracks), _ptr(off), _ptr(fr), _ptr(px), _ptr(pt), _ptr(us),
                                  _params_ref(VsmLocateParams, locate_params, params))
        return self._locate_result(rc, "vsm_locate_run")

    def locate_points(self, f, cu, cv, locate=None, lists=None, params=None, counts=None):
        """vsm_points_locate: the same on the handle's last track and point results (the kept points; lists as for
        track_points)."""
        lo = None if locate is None else _mask(locate, len(locate) if self._track_frames is None else self._track_frames)
        ls, ptrs, cnt = _optional_lists(lists, counts)
        rc = lib().vsm_points_locate(self.h, ptrs, _ptr(cnt), _ptr(lo), float(f), float(cu), float(cv), _params_ref(VsmLocateParams, locate_params, params))
        return self._locate_result(rc, "vsm_points_locate")

    # --- new observations of the points, found by projection ---------------------------------------
    def _reobserve_result(self, rc, what, records_of=None):
        L = lib()
        _check(rc, what)
        n, acc = C.c_int32(0), C.c_int32(0)
        L.vsm_reobserve_count(self.h, C.byref(n), C.byref(acc))
        out = (np.zeros((n.value, 7), np.int32), np.zeros((n.value, 2), np.float64), np.zeros(L.vsm_reobserve_get_tracks(self.h, None), np.int32),
               np.zeros((L.vsm_reobserve_get_frames(self.h, None), 2), np.int32))
        L.vsm_reobserve_get(self.h, _ptr(out[0]), _ptr(out[1]))
        L.vsm_reobserve_get_tracks(self.h, _ptr(out[2]))
        L.vsm_reobserve_get_frames(self.h, _ptr(out[3]))
        res = Reobservation(*out, *_stage_dicts(self.h, L.vsm_reobserve_get_stats, REOBSERVE_STATS, L.vsm_reobserve_get_timings, REOBSERVE_TIMINGS))
        assert acc.value == res.stats.get("cand_accepted", 0)
        return res._take_pixels(records_of or self.pair_features)

    def reobserve(self, poses, f, cu, cv, width, height, offsets, obs_frames, obs_feat, xyz, feat_offsets, feat, use=None, ref_obs=None, search=None,
                  pose_valid=None, params=None, n_tracks=None):
        """vsm_reobserve_run: every point in use projected into every searched frame with a pose that does not observe it yet,
        and the frame's free features near the projection searched for the track's descriptor, on the device.  poses, the
        tracks, xyz, use as for vet; obs_feat [n_obs]: each observation's feature index in its frame; feat_offsets [F + 1], feat
        [n_feat, 12]: the frames' feature records; search [F], ref_obs [T]: None for all / the middle observation; params: a dict
        of vsm_reobserve_params fields or the struct.  Returns a Reobservation object."""
        po, pv, se, off, fr, ft, pt, us, ro, fo, fe = _reobserve_inputs(poses, pose_valid, search, offsets, obs_frames, obs_feat, xyz, use, ref_obs, feat_offsets, feat)
        T = _n_tracks(off, n_tracks)
        rc = lib().vsm_reobserve_run(self.h, len(po), _ptr(po), _ptr(pv), _ptr(se), float(f), float(cu), float(cv), int(width), int(height), T, _ptr(off), _ptr(fr),
                                     _ptr(ft), _ptr(pt), _ptr(us), _ptr(ro), _ptr(fo), _ptr(fe), _params_ref(VsmReobserveParams, reobserve_params, params))
        return self._reobserve_result(rc, "vsm_reobserve_run", lambda g: fe[fo[g]:fo[g + 1]])

    def reobserve_points(self, poses, f, cu, cv, search=None, pose_valid=None, params=None):
        """vsm_points_reobserve: the same on the handle's last track and point results (pair_tracks with side 0; the kept points)
        and the features the last match_pairs call left resident in HBM"""
        po, pv = _pose_inputs(poses, pose_valid, self._track_frames)
        se = _mask(search, len(po))
        rc = lib().vsm_points_reobserve(self.h, _ptr(po), _ptr(pv), _ptr(se), float(f), float(cu), float(cv),
                                        _params_ref(VsmReobserveParams, reobserve_params, params))
        return self._reobserve_result(rc, "vsm_points_reobserve")

    # --- duplicate tracks of one point, joined ---------------------------------------------------------
    def _fuse_result(self, rc, what):
        L = lib()
        _check(rc, what)
        n, nf = C.c_int32(0), C.c_int32(0)
        L.vsm_fuse_count(self.h, C.byref(n), C.byref(nf))
        T = L.vsm_fuse_get_tracks(self.h, None, None)
        out = (np.zeros((n.value, 8), np.int32), np.zeros((n.value, 2), np.float64), np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T + 1, np.int32),
               np.zeros(L.vsm_fuse_get_merged(self.h, None, None), np.int32), np.zeros((L.vsm_fuse_get_frames(self.h, None), 2), np.int32))
        L.vsm_fuse_get(self.h, _ptr(out[0]), _ptr(out[1]))
        L.vsm_fuse_get_tracks(self.h, _ptr(out[2]), _ptr(out[3]))
        L.vsm_fuse_get_merged(self.h, _ptr(out[4]), _ptr(out[5]))
        L.vsm_fuse_get_frames(self.h, _ptr(out[6]))
        res = Fusion(*out, *_stage_dicts(self.h, L.vsm_fuse_get_stats, FUSE_STATS, L.vsm_fuse_get_timings, FUSE_TIMINGS))
        assert nf.value == res.stats.get("fusions", 0) == len(res.fused())
        return res

    def fuse(self, poses, f, cu, cv, width, height, offsets, obs_frames, obs_feat, xyz, feat_offsets, feat, use=None, ref_obs=None, search=None, pose_valid=None,
             params=None, n_tracks=None):
        """vsm_fuse_run: every point in use projected into every searched frame with a pose that does not observe it yet, the
        features that tracks in use own near the projection searched for the track's descriptor, and the tracks that choose
        each other fused, on the device.  Arguments as reobserve; params: a dict of vsm_fuse_params fields or the struct.
        Returns a Fusion object."""
        po, pv, se, off, fr, ft, pt, us, ro, fo, fe = _reobserve_inputs(poses, pose_valid, search, offsets, obs_frames, obs_feat, xyz, use, ref_obs, feat_offsets, feat)
        T = _n_tracks(off, n_tracks)
        rc = lib().vsm_fuse_run(self.h, len(po), _ptr(po), _ptr(pv), _ptr(se), float(f), float(cu), float(cv), int(width), int(height), T, _ptr(off), _ptr(fr),
                                _ptr(ft), _ptr(pt), _ptr(us), _ptr(ro), _ptr(fo), _ptr(fe), _params_ref(VsmFuseParams, fuse_params, params))
        return self._fuse_result(rc, "vsm_fuse_run")

    def fuse_points(self, poses, f, cu, cv, search=None, pose_valid=None, params=None):
        """vsm_points_fuse: the same on the handle's last track and point results (pair_tracks with side 0; the kept points)
        and the features the last match_pairs call left resident in HBM"""
        po, pv = _pose_inputs(poses, pose_valid, self._track_frames)
        se = _mask(search, len(po))
        rc = lib().vsm_points_fuse(self.h, _ptr(po), _ptr(pv), _ptr(se), float(f), float(cu), float(cv), _params_ref(VsmFuseParams, fuse_params, params))
        return self._fuse_result(rc, "vsm_points_fuse")

    def pair_features(self, frame, side=0, set=1):
        """vsm_pairs_get_features: the feature records [n, 12] int32 of a frame of the last match_pairs call (set 1: the set the
        match lists' indices count in)"""
        L = lib()
        n = L.vsm_pairs_num_features(self.h, int(frame), int(side), int(set))
        a = np.zeros((n, 12), np.int32)
        if n:
            assert L.vsm_pairs_get_features(self.h, int(frame), int(side), int(set), _ptr(a), n) == n
        return a

    def track_pixels(self, lists=None, counts=None):
        """vsm_tracks_pixels: (obs_frames [n_obs] int32, uv [n_obs, 2] float32) of the handle's last track result, the pixels
        read from the match lists as track_points reads them (lists: as there)"""
        ls, ptrs, cnt = _optional_lists(lists, counts)
        n = _check(lib().vsm_tracks_pixels(self.h, ptrs, _ptr(cnt), None, None), "vsm_tracks_pixels")
        fr, px = np.zeros(n, np.int32), np.zeros((n, 2), np.float32)
        _check(lib().vsm_tracks_pixels(self.h, ptrs, _ptr(cnt), _ptr(fr), _ptr(px)), "vsm_tracks_pixels")
        return fr, px

    def alternate(self, poses, f, cu, cv, rounds, refine=None, point_params=None, resect_params=None, pose_valid=None, lists=None):
        """block-coordinate bundle adjustment from the two batched calls: `rounds` times track_points, then resect_points on its
        poses.  Returns (the last poses, the last Points, [(sum of ss_before, sum of ss_after) per round])."""
        points, history = None, []
        for _ in range(int(rounds)):
            points = self.track_points(poses, f, cu, cv, lists=lists, pose_valid=pose_valid, params=point_params)
            res = self.resect_points(poses, f, cu, cv, lists=lists, refine=refine, pose_valid=pose_valid, params=resect_params)
            poses = res.poses
            history.append((float(res.ss_before.sum()), float(res.ss_after.sum())))
        return poses, points, history

    # --- monocular motions of a pair set ---------------------------------------------------------
    def _motions_result(self, rc, what):
        L = lib()
        _check(rc, what)
        P = L.vsm_motions_count(self.h)
        r, stage, n_inl = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32)
        tr, T = np.zeros((P, 6)), np.zeros((P, 4, 4))
        L.vsm_motions_get(self.h, _ptr(r), _ptr(stage), _ptr(tr), _ptr(T), _ptr(n_inl))
        inl, mm = [], []
        for k in range(P):
            a = np.zeros(int(n_inl[k]), np.int32)
            if len(a):
                L.vsm_motions_inliers(self.h, k, _ptr(a), len(a))
            inl.append(a)
            m = np.zeros(L.vsm_motions_matches(self.h, k, None, 0), P_MATCH)
            if len(m):
                L.vsm_motions_matches(self.h, k, _ptr(m), len(m))
            mm.append(m)
        stats, timings = _stage_dicts(self.h, L.vsm_motions_get_stats, MOTION_STATS, L.vsm_motions_get_timings, MOTION_TIMINGS)
        stats["device_svd"] = L.vsm_motions_device_svd(self.h)
        return Motions(r, stage, tr, T, inl, mm, stats, timings)

    def motions(self, lists, params, bucket=False, counts=None):
        """vsm_motions_run: the mono motion of every list (one P_MATCH array of flow matches per pair) in one batched call on
        the device.  params: vo_mono_params(...).  Returns a Motions object."""
        ls, ptrs, cnt = _list_inputs(lists, counts)
        rc = lib().vsm_motions_run(self.h, None if params is None else C.byref(params), len(ls), ptrs, _ptr(cnt), int(bool(bucket)))
        return self._motions_result(rc, "vsm_motions_run")

    def pair_motions(self, params, bucket=False):
        """vsm_pairs_motions: the same on the lists of the last match_pairs call (fetched or not), which stay as they are"""
        rc = lib().vsm_pairs_motions(self.h, None if params is None else C.byref(params), int(bool(bucket)))
        return self._motions_result(rc, "vsm_pairs_motions")

    def last_motions(self):
        """the handle's last motions result as it stands (None: there is none)"""
        return self._motions_result(self.OK, "") if lib().vsm_motions_count(self.h) else None

    def pair_timings(self):
        t = np.zeros(4, dtype=np.float64)
        lib().vsm_pairs_get_timings(self.h, t.ctypes.data_as(C.c_void_p))
        return dict(zip(("image_side_us", "pass1_us", "pass2_us", "total_us"), t.tolist()))

    def sequence_path(self):
        """2: the last run_sequence went through the GPU-resident form, 1: through the host-shared form"""
        return lib().vsm_sequence_path(self.h)

    def set_option(self, name, value):
        """measurement / test switch of this handle (vsm_set_option): "seq_serial", "seq_chunk", "seq_v2", ..."""
        if lib().vsm_set_option(self.h, name.encode(), int(value)) != self.OK:
            raise VisoMatchError(f"unknown option {name}")

    def sequence_timings(self):
        t = np.zeros(4, dtype=np.float64)
        lib().vsm_sequence_get_timings(self.h, t.ctypes.data_as(C.c_void_p))
        return dict(zip(("gpu_us", "host_us", "total_us", "chunk"), t.tolist()))

    def set_profiling(self, on, only=None, print_spans=False):
        """HIP-event spans around the library's kernels: all of them, or (only="k_match<16>:pass2") one kernel's launches
        alone - the spans' own event records are packets on every stream and slow the pipeline they measure"""
        L = lib()
        if on and only is not None:
            ids = [i for i in range(L.vsm_num_kernels()) if L.vsm_kernel_name(i).decode() == only]
            if not ids:
                raise VisoMatchError(f"unknown kernel {only}")
            L.vsm_set_profiling(self.h, (1100 if print_spans else 100) + ids[0])
        else:
            L.vsm_set_profiling(self.h, int(bool(on)))

    def kernel_stats(self):
        """{kernel name: (total device ms, launches)} since set_profiling(True)"""
        L = lib()
        n = L.vsm_num_kernels()
        ms = np.zeros(n, dtype=np.float64)
        cnt = np.zeros(n, dtype=np.int64)
        L.vsm_get_kernel_stats(self.h, ms.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p))
        return {L.vsm_kernel_name(i).decode(): (float(ms[i]), int(cnt[i])) for i in range(n)}

    def close(self):
        if getattr(self, "h", None):
            lib().vsm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiVisualOdometryStereo:
    """K independent stereo sequences in lock-step (vsm_multi_*): process(left, right) is VisualOdometryStereo::process
    for the next pair of every sequence, one launch per kernel over all of them; per sequence the results equal the
    reference's for that sequence alone."""

    def __init__(self, n_sequences, f, cu, cv, base, bucket=(2, 50.0, 50.0), ransac_iters=200, inlier_threshold=2.0,
                 reweighting=True, **match):
        self.params = vo_stereo_params(f, cu, cv, base, bucket, ransac_iters, inlier_threshold, reweighting, **match)
        self.K = int(n_sequences)
        h = lib().vsm_multi_create(C.byref(self.params), self.K)
        if not h:
            raise VisoMatchError("vsm_multi_create failed: no usable HIP device (there is no CPU path)")
        self.h = C.c_void_p(h)

    def close(self):
        if getattr(self, "h", None):
            lib().vsm_multi_destroy(self.h)
            self.h = None

    __del__ = close

    def process(self, left, right):
        """left / right: [K,H,W] uint8, numpy (host) or CUDA torch tensors -> K success flags"""
        L = lib()
        ok = np.zeros(self.K, dtype=np.int32)
        # (checked BEFORE the call: the library reads K images per side from these pointers)
        if _is_torch(left):
            import torch
            if not (_is_torch(right) and left.is_cuda and right.is_cuda and left.dtype == torch.uint8 and right.dtype == torch.uint8 and left.dim() == 3
                    and left.shape == right.shape and left.shape[0] == self.K and left.stride() == right.stride() and left.stride(2) == 1):
                raise VisoMatchError(f"process: left / right must be uint8 CUDA tensors [K={self.K},H,W] of equal shape and strides, unit stride along W")
            K, h, w = left.shape
            torch.cuda.current_stream(left.device).synchronize()   # (the library reads the images on its own stream)
            rc = L.vsm_multi_process(self.h, C.c_void_p(left.data_ptr()), C.c_void_p(right.data_ptr()), left.stride(0), 1, w, h, left.stride(1),
                                     ok.ctypes.data_as(C.c_void_p))
        else:
            left = np.ascontiguousarray(left, dtype=np.uint8)
            right = np.ascontiguousarray(right, dtype=np.uint8)
            if left.ndim != 3 or left.shape != right.shape or left.shape[0] != self.K:
                raise VisoMatchError(f"process: left / right must be uint8 arrays [K={self.K},H,W] of equal shape, got {left.shape} / {right.shape}")
            K, h, w = left.shape
            rc = L.vsm_multi_process(self.h, left.ctypes.data_as(C.c_void_p), right.ctypes.data_as(C.c_void_p), w * h, 0, w, h, w,
                                     ok.ctypes.data_as(C.c_void_p))
        _check(rc, "vsm_multi_process")
        return ok.astype(bool)

    def get_motion(self, k):
        t = np.zeros(16)
        lib().vsm_multi_get_motion(self.h, k, t.ctypes.data_as(C.c_void_p))
        return t.reshape(4, 4)

    def motion_valid(self, k):
        return bool(lib().vsm_multi_motion_valid(self.h, k))

    def get_matches(self, k, bucketed=True):
        n = lib().vsm_multi_num_matches(self.h, k, int(bucketed))
        out = np.zeros(n, dtype=P_MATCH)
        if n:
            lib().vsm_multi_get_matches(self.h, k, int(bucketed), out.ctypes.data_as(C.c_void_p), n)
        return out

    def get_inlier_indices(self, k):
        n = lib().vsm_multi_num_inliers(self.h, k)
        out = np.zeros(n, dtype=np.int32)
        if n:
            lib().vsm_multi_get_inliers(self.h, k, out.ctypes.data_as(C.c_void_p), n)
        return out

    def timings(self):
        t = np.zeros(4, dtype=np.float64)
        lib().vsm_multi_get_timings(self.h, t.ctypes.data_as(C.c_void_p))
        return dict(zip(("features_us", "pass1_us", "pass2_us", "egomotion_us"), t.tolist()))


class VisualOdometryStereo:
    """Mirror of the reference's VisualOdometryStereo (viso/viso_stereo.h:28-88): process() runs
    pushBack + matchFeatures(2, Tr_delta) + bucketFeatures + egomotion and keeps Tr_delta."""

    def __init__(self, f, cu, cv, base, bucket=(2, 50.0, 50.0), ransac_iters=200, inlier_threshold=2.0,
                 reweighting=True, **match):
        self.params = vo_stereo_params(f, cu, cv, base, bucket, ransac_iters, inlier_threshold, reweighting, **match)
        h = lib().vsm_vo_stereo_create(C.byref(self.params))
        if not h:
            raise VisoMatchError("vsm_vo_stereo_create failed: no usable HIP device (there is no CPU path)")
        self.h = C.c_void_p(h)

    def close(self):
        if getattr(self, "h", None):
            lib().vsm_vo_stereo_destroy(self.h)
            self.h = None

    __del__ = close

    def get_motion(self):
        t = np.zeros(16)
        lib().vsm_vo_stereo_get_motion(self.h, t.ctypes.data_as(C.c_void_p))
        return t.reshape(4, 4)

    def process(self, I1, I2, replace=False):
        """-> (success, Tr_valid before the call, Tr_delta before, Tr_delta after)"""
        L = lib()
        valid = bool(L.vsm_vo_stereo_motion_valid(self.h))
        tin = self.get_motion()
        if _is_torch(I1):
            assert I1.is_cuda and I2.is_cuda and I1.shape == I2.shape and I1.stride() == I2.stride()
            h, w = I1.shape
            _order_behind_torch(L.vsm_vo_stereo_matcher(self.h), I1)
            ok = L.vsm_vo_stereo_process_device(self.h, C.c_void_p(I1.data_ptr()), C.c_void_p(I2.data_ptr()), w, h,
                                                I1.stride(0), int(replace))
        else:
            I1 = np.ascontiguousarray(I1, dtype=np.uint8)
            I2 = np.ascontiguousarray(I2, dtype=np.uint8)
            h, w = I1.shape
            ok = L.vsm_vo_stereo_process(self.h, I1.ctypes.data_as(C.c_void_p), I2.ctypes.data_as(C.c_void_p), w, h, w,
                                         int(replace))
        return bool(ok), valid, tin, self.get_motion()

    def process_matches(self, m):
        m = np.ascontiguousarray(m, dtype=P_MATCH)
        ok = lib().vsm_vo_stereo_process_matches(self.h, m.ctypes.data_as(C.c_void_p), len(m))
        return bool(ok), self.get_motion()

    def get_matches(self):
        n = lib().vsm_vo_stereo_num_matches(self.h)
        out = np.zeros(n, dtype=P_MATCH)
        if n:
            lib().vsm_vo_stereo_get_matches(self.h, out.ctypes.data_as(C.c_void_p), n)
        return out

    def get_inlier_indices(self):
        n = lib().vsm_vo_stereo_num_inliers(self.h)
        out = np.zeros(n, dtype=np.int32)
        if n:
            lib().vsm_vo_stereo_get_inliers(self.h, out.ctypes.data_as(C.c_void_p), n)
        return out

    def get_number_of_matches(self):
        return lib().vsm_vo_stereo_num_matches(self.h)

    def get_number_of_inliers(self):
        return lib().vsm_vo_stereo_num_inliers(self.h)

    def get_gain(self, inliers):
        a = np.ascontiguousarray(inliers, dtype=np.int32)
        return float(lib().vsm_vo_stereo_gain(self.h, a.ctypes.data_as(C.c_void_p), len(a)))

    def timings(self):
        t = np.zeros(4)
        lib().vsm_vo_stereo_get_timings(self.h, t.ctypes.data_as(C.c_void_p))
        return t

    # the face the golden drivers use (same names as oracle.bindings.OracleStereoVO)
    bucketed = get_matches
    inliers = get_inlier_indices


class VisualOdometryMono:
    """Mirror of the reference's VisualOdometryMono (viso/viso_mono.h:28-90): process() runs
    pushBack + matchFeatures(0) + bucketFeatures + the monocular egomotion."""

    def __init__(self, f, cu, cv, bucket=(2, 50.0, 50.0), **kw):
        self.params = vo_mono_params(f, cu, cv, bucket, **kw)
        h = lib().vsm_vo_mono_create(C.byref(self.params))
        if not h:
            raise VisoMatchError("vsm_vo_mono_create failed: no usable HIP device (there is no CPU path)")
        self.h = C.c_void_p(h)

    def close(self):
        if getattr(self, "h", None):
            lib().vsm_vo_mono_destroy(self.h)
            self.h = None

    __del__ = close

    def get_motion(self):
        t = np.zeros(16)
        lib().vsm_vo_mono_get_motion(self.h, t.ctypes.data_as(C.c_void_p))
        return t.reshape(4, 4)

    def process(self, I, replace=False):
        """-> (success, Tr_delta after the call)"""
        L = lib()
        if _is_torch(I):
            assert I.is_cuda and I.dim() == 2 and I.stride(1) == 1
            h, w = I.shape
            _order_behind_torch(L.vsm_vo_mono_matcher(self.h), I)
            ok = L.vsm_vo_mono_process_device(self.h, C.c_void_p(I.data_ptr()), w, h, I.stride(0), int(replace))
        else:
            I = np.ascontiguousarray(I, dtype=np.uint8)
            h, w = I.shape
            ok = L.vsm_vo_mono_process(self.h, I.ctypes.data_as(C.c_void_p), w, h, w, int(replace))
        return bool(ok), self.get_motion()

    def process_matches(self, m):
        m = np.ascontiguousarray(m, dtype=P_MATCH)
        ok = lib().vsm_vo_mono_process_matches(self.h, m.ctypes.data_as(C.c_void_p), len(m))
        return bool(ok), self.get_motion()

    def get_matches(self):
        n = lib().vsm_vo_mono_num_matches(self.h)
        out = np.zeros(n, dtype=P_MATCH)
        if n:
            lib().vsm_vo_mono_get_matches(self.h, out.ctypes.data_as(C.c_void_p), n)
        return out

    def get_inlier_indices(self):
        n = lib().vsm_vo_mono_num_inliers(self.h)
        out = np.zeros(n, dtype=np.int32)
        if n:
            lib().vsm_vo_mono_get_inliers(self.h, out.ctypes.data_as(C.c_void_p), n)
        return out

    def get_number_of_matches(self):
        return lib().vsm_vo_mono_num_matches(self.h)

    def get_number_of_inliers(self):
        return lib().vsm_vo_mono_num_inliers(self.h)

    def get_gain(self, inliers):
        a = np.ascontiguousarray(inliers, dtype=np.int32)
        return float(lib().vsm_vo_mono_gain(self.h, a.ctypes.data_as(C.c_void_p), len(a)))

    def timings(self):
        t = np.zeros(10)
        lib().vsm_vo_mono_get_timings(self.h, t.ctypes.data_as(C.c_void_p))
        return t

    def device_svd(self):
        return bool(lib().vsm_vo_mono_device_svd(self.h))

    def device_stages(self):
        """MONO_STAGE_* bits of the stages the last estimate took from the GPU"""
        return int(lib().vsm_vo_mono_device_stages(self.h))

    bucketed = get_matches
    inliers = get_inlier_indices
