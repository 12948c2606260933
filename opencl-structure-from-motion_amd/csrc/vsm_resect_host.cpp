// Pose refinement, the host side without HIP: the parameters' test, libm's sqrt and
// vsm_host_resect - one host thread walking the functions of vsm_resect.h, the 256 partial sums and their tree in a loop.
// The host view is the CPU suite's subject and the device path's second opinion, never its fallback.
#include "vsm_resect.h"

#include <math.h>
#include <string.h>

#include <vector>

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
  rs_host_tree(partial.data(), RS_SUMS);
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
  if (pts_check_points(rs_params_ok(params), n_frames, poses, n_tracks, offsets, obs_frames, uv, xyz) < 0) return VSM_EARG;
  // the rows by frame, one chunk
  std::vector<int32_t> at;
  RsGroup G(n_frames, n_tracks, offsets, use, RsObsArrays{obs_frames, uv}, 1, RsLoop(), at);
  const std::vector<int32_t> &row_off = G.row_off;
  std::vector<RsRow> table((size_t)row_off[n_frames] + 1);
  G.fill(table.data());
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
