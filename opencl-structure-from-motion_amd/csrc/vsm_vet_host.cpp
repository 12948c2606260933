// Vetting of observations, the host side without HIP: the default parameters and vsm_host_vet - one host thread walking the
// functions of vsm_vet.h, a track's 16 partial sums and their tree in a loop.  The host view is the CPU suite's subject and
// the device path's second opinion, never its fallback.
#include "vsm_vet.h"

#include <string.h>

#include <vector>

extern "C" {

void vsm_vet_default_params(vsm_vet_params *p) {
  if (!p) return;
  p->max_residual = 2.0;
  p->min_depth = 1e-10;
  p->min_observations = 2;
}

int32_t vsm_host_vet(int32_t n_frames, const double *poses, const uint8_t *pose_valid, double f, double cu, double cv, int32_t n_tracks,
                     const int32_t *offsets, const int32_t *obs_frames, const float *uv, const double *xyz, const uint8_t *use, const vsm_vet_params *params,
                     uint8_t *code, float *r2, int32_t *status, int32_t *n_in, int32_t *frame_lo, int32_t *frame_hi, double *ss, double *worst,
                     int32_t *frame_counts, int32_t *kept_offsets, int32_t *kept_index, int32_t *n_kept) {
  const int64_t n_obs = pts_check_points(vet_params_ok(params), n_frames, poses, n_tracks, offsets, obs_frames, uv, xyz);
  if (n_obs < 0) return VSM_EARG;
  const double limit = rs_limit(params->max_residual);
  std::vector<double> states((size_t)n_frames * 12 + 1);
  for (int32_t g = 0; g < n_frames; g++) pts_rigid_inverse(poses + 12 * (size_t)g, states.data() + 12 * (size_t)g);
  std::vector<uint8_t> codes((size_t)n_obs + 1);
  std::vector<int32_t> fc((size_t)n_frames * 3 + 1, 0);
  if (kept_offsets) kept_offsets[0] = 0;
  int32_t kept = 0;
  for (int32_t t = 0; t < n_tracks; t++) {
    const int32_t o = offsets[t], n = offsets[t + 1] - o;
    const int in_use = !use || use[t];
    VetAcc partial[VET_LANES];
    for (int l = 0; l < VET_LANES; l++) vet_acc_init(&partial[l]);
    for (int32_t k = 0; k < n; k++) {
      const int32_t i = o + k, g = obs_frames[i];
      double tt = 0.0;
      const int32_t c = vet_obs(states.data() + 12 * (size_t)g, xyz + 3 * (size_t)t, uv[2 * (size_t)i], uv[2 * (size_t)i + 1], in_use, !pose_valid || pose_valid[g], f,
                                cu, cv, params->min_depth, limit, &tt);
      codes[i] = (uint8_t)c;
      if (r2) r2[i] = vet_r2(c, tt);
      if (c == VET_INLIER) {
        vet_acc_add(&partial[k % VET_LANES], g, tt);
        fc[3 * (size_t)g]++;
      } else if (c == VET_BEHIND) {
        fc[3 * (size_t)g + 1]++;
      } else if (c == VET_GATED) {
        fc[3 * (size_t)g + 2]++;
      }
    }
    for (int s = VET_LANES / 2; s >= 1; s >>= 1)
      for (int l = 0; l < s; l++) {
        const VetAcc &b = partial[l + s];
        vet_acc_merge(&partial[l], b.ss, b.worst, b.n_in, b.lo, b.hi);
      }
    const VetAcc &a = partial[0];
    const int32_t st = vet_track_status(in_use, a, params->min_observations);
    if (status) status[t] = st;
    if (n_in) n_in[t] = a.n_in;
    if (frame_lo) frame_lo[t] = vet_frame_lo(a);
    if (frame_hi) frame_hi[t] = a.hi;
    if (ss) ss[t] = a.ss;
    if (worst) worst[t] = a.worst;
    if (vet_kept_length(st, a.n_in) > 0)
      for (int32_t k = 0; k < n; k++)
        if (codes[o + k] == VET_INLIER) {
          if (kept_index) kept_index[kept] = o + k;
          kept++;
        }
    if (kept_offsets) kept_offsets[t + 1] = kept;
  }
  if (code && n_obs > 0) memcpy(code, codes.data(), (size_t)n_obs);
  if (frame_counts && n_frames > 0) memcpy(frame_counts, fc.data(), (size_t)n_frames * 12);
  if (n_kept) *n_kept = kept;
  return n_tracks;
}

}  // extern "C"
