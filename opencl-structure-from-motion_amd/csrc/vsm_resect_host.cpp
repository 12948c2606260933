// Pose refinement, the host side without HIP: the argument checks, libm's sqrt and
// vsm_host_resect - one host thread walking the functions of vsm_resect.h, the 256 partial sums and their tree in a loop.
// The host view is the CPU suite's subject and the device path's second opinion, never its fallback.
#include "vsm_resect.h"

#include <math.h>
#include <string.h>

#include <vector>

int64_t rs_check_args(int32_t n_frames, const double *poses, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv,
                      const double *xyz, const vsm_resect_params *params) {
  if (!rs_params_ok(params) || (n_tracks > 0 && !xyz)) return -1;
  return pts_check_obs(n_frames, poses, n_tracks, offsets, obs_frames, uv);
}

bool rs_params_ok(const vsm_resect_params *p) { return p && p->min_observations >= 6 && p->max_updates >= 1 && p->eps > 0 && p->eps < HUGE_VAL; }

double rs_rms(double ss, int32_t used) { return used > 0 ? sqrt(ss / (double)used) : 0.0; }

namespace {

// one evaluation of a frame's rows at the state S, in the definition's order
void host_evaluate(const RsRow *rows, int32_t n, const double *xyz, double f, double cu, double cv, const vsm_resect_params &prm, const double *S, double *sums,
                   int32_t *count, bool jacobian, std::vector<double> &partial) {
  const double limit = rs_limit(prm.max_residual);
  partial.assign((size_t)RS_LANES * RS_SUMS, 0.0);
  int32_t used = 0;
  for (int32_t i = 0; i < n; i++) {
    double xc[3], r[2], t, ju[6], jv[6];
    if (!rs_row(S, xyz + 3 * (size_t)rows[i].track, rows[i].u, rows[i].v, f, cu, cv, prm.min_depth, limit, xc, r, &t)) continue;
    used++;
    double *acc = &partial[(size_t)(i % RS_LANES) * RS_SUMS];
    if (jacobian) {
      rs_jacobian(xc, f, ju, jv);
      rs_add_row(acc, ju, jv, r, t);
    } else {
      acc[27] += t;
    }
  }
  for (int s = RS_LANES / 2; s >= 1; s >>= 1)
    for (int l = 0; l < s; l++)
      for (int k = 0; k < RS_SUMS; k++) partial[(size_t)l * RS_SUMS + k] += partial[(size_t)(l + s) * RS_SUMS + k];
  for (int k = 0; k < RS_SUMS; k++) sums[k] = partial[k];
  *count = used;
}

}  // namespace

extern "C" {

void vsm_resect_default_params(vsm_resect_params *p) {
  if (!p) return;
  p->min_observations = 10;
  p->max_updates = 20;
  p->eps = 1e-8;
  p->max_residual = 0.0;
  p->min_depth = 1e-10;
}

int32_t vsm_host_resect(int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *refine, double f, double cu, double cv,
                        int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv, const double *xyz, const uint8_t *use,
                        const vsm_resect_params *params, int32_t *status, double *out_poses, int32_t *updates, int32_t *rows, int32_t *used,
                        double *ss_before, double *ss_after, double *rms_before, double *rms_after) {
  if (rs_check_args(n_frames, poses, n_tracks, offsets, obs_frames, uv, xyz, params) < 0) return VSM_EARG;
  // the rows by frame, one chunk
  const auto frame_of = [&](int32_t i) { return obs_frames[i]; };
  const auto pixel_of = [&](int32_t i, float *u, float *v) {
    *u = uv[2 * (size_t)i];
    *v = uv[2 * (size_t)i + 1];
  };
  std::vector<int32_t> row_off((size_t)n_frames + 1, 0);
  rs_group_count(0, n_tracks, offsets, use, frame_of, row_off.data() + 1);
  for (int32_t g = 0; g < n_frames; g++) row_off[g + 1] += row_off[g];
  std::vector<RsRow> table((size_t)row_off[n_frames] + 1);
  std::vector<int32_t> at(row_off.begin(), row_off.end() - 1);
  rs_group_fill(0, n_tracks, offsets, use, frame_of, pixel_of, at.data(), table.data());
  std::vector<double> partial;
  for (int32_t g = 0; g < n_frames; g++) {
    const RsRow *fr = table.data() + row_off[g];
    const int32_t n = row_off[g + 1] - row_off[g];
    const double *pose = poses + 12 * (size_t)g;
    RsResult res = {0, 0, 0, 0, 0.0, 0.0};
    double S[12], ab[42], out[12];
    memcpy(out, pose, sizeof(out));
    res.status = rs_early_status(!pose_valid || pose_valid[g], !refine || refine[g], n, params->min_observations);
    if (res.status == 0) {
      pts_rigid_inverse(pose, S);
      rs_frame(
          [&](const double *state, double *sums, int32_t *count, bool jacobian) {
            host_evaluate(fr, n, xyz, f, cu, cv, *params, state, sums, count, jacobian, partial);
          },
          ab, S, *params, &res);
      if (res.status == 0 || res.status == 6) pts_rigid_inverse(S, out);
    }
    if (status) status[g] = res.status;
    if (out_poses) memcpy(out_poses + 12 * (size_t)g, out, sizeof(out));
    if (updates) updates[g] = res.updates;
    if (rows) rows[g] = n;
    if (used) used[g] = res.used;
    if (ss_before) ss_before[g] = res.ss_before;
    if (ss_after) ss_after[g] = res.ss_after;
    if (rms_before) rms_before[g] = rs_rms(res.ss_before, res.used_before);
    if (rms_after) rms_after[g] = rs_rms(res.ss_after, res.status == 0 || res.status == 6 ? res.used : 0);
  }
  return n_frames;
}

}  // extern "C"
