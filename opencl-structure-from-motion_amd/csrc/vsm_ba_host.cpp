// Joint adjustment of poses and points, the host side without HIP: the parameters' test, the stats, the history's columns
// and vsm_host_adjust - one host thread walking the functions and the schedule of vsm_ba.h, the 256 partial sums and their
// tree in a loop.  The host
// view works on the device path's block (BaBlocks, vsm_layouts.h: the same placing, packing and binding) in one zeroed buffer
// of host memory and makes no HIP call.  It is the CPU suite's subject, the device path's second opinion and the benchmark's
// baseline, never a fallback.
#include "vsm_layouts.h"

#include <math.h>
#include <string.h>

#include <vector>

static bool ba_positive_finite(double x) { return x > 0 && x < HUGE_VAL; }

bool ba_params_ok(const vsm_adjust_params *p) {
  return p && p->min_observations >= 6 && p->max_rounds >= 1 && p->cg_iters >= 1 && ba_positive_finite(p->lambda0) && ba_positive_finite(p->cg_tol) &&
         ba_positive_finite(p->ftol);
}

void ba_stats(int32_t n_frames, const int32_t *fstatus, int32_t n_tracks, const int32_t *tstatus, const BaCtl &ctl, int64_t *out16) {
  memset(out16, 0, 16 * sizeof(int64_t));
  for (int32_t g = 0; g < n_frames; g++)
    if (fstatus[g] >= 0 && fstatus[g] < 8) out16[fstatus[g]]++;
  for (int32_t t = 0; t < n_tracks; t++)
    if (tstatus[t] >= 0 && tstatus[t] < 4) out16[8 + tstatus[t]]++;
  out16[12] = ctl.round;
  out16[13] = ctl.n_accepted;
  out16[14] = ctl.stop;
  out16[15] = ctl.total_cg;
}

void ba_history(int32_t rounds, const double *hist_d, const int32_t *hist_i, double *cost_before, double *cost_after, double *lambda, int32_t *cg_iters,
                int32_t *cg_end, int32_t *accepted, int32_t *active) {
  for (int32_t k = 0; k < rounds; k++) {
    if (cost_before) cost_before[k] = hist_d[3 * (size_t)k];
    if (cost_after) cost_after[k] = hist_d[3 * (size_t)k + 1];
    if (lambda) lambda[k] = hist_d[3 * (size_t)k + 2];
    if (cg_iters) cg_iters[k] = hist_i[4 * (size_t)k];
    if (cg_end) cg_end[k] = hist_i[4 * (size_t)k + 1];
    if (accepted) accepted[k] = hist_i[4 * (size_t)k + 2];
    if (active) active[k] = hist_i[4 * (size_t)k + 3];
  }
}

namespace {

// the steps of ba_schedule as loops
struct HostOps {
  BaData D;
  std::vector<double> partial;  // [RS_LANES][RS_SUMS]

  void tree(int n) { rs_host_tree(partial.data(), n); }
  double dot(const double *a, const double *b) {
    for (int l = 0; l < RS_LANES; l++) partial[(size_t)l * RS_SUMS] = ba_dot_partial(D, a, b, l);
    tree(1);
    return partial[0];
  }
  bool idle() const { return D.ctl->done != 0; }
  bool solve_idle() const { return D.ctl->done || D.ctl->cg_done; }

  void init() {
    partial.assign((size_t)RS_LANES * RS_SUMS, 0.0);
    ba_ctl_init(D);
    for (int32_t g = 0; g < D.n_frames; g++) ba_init_frame(D, g);
    for (int32_t t = 0; t < D.n_tracks; t++)
      for (int a = 0; a < 3; a++) D.out_xyz[3 * (size_t)t + a] = D.xyz_in[3 * (size_t)t + a];
  }
  void linearise() {
    if (idle()) return;
    const double limit = rs_limit(D.prm.max_residual);
    for (int32_t g = 0; g < D.n_frames; g++) {
      const int32_t o = D.row_off[g], n = D.row_off[g + 1] - o;
      partial.assign((size_t)RS_LANES * RS_SUMS, 0.0);
      int32_t count = 0;
      for (int32_t i = 0; i < n; i++) {
        if (D.valid[g])
          ba_lin_row(D, D.state + 12 * (size_t)g, D.rows[o + i], limit, &partial[(size_t)(i % RS_LANES) * RS_SUMS], count);
        else
          D.active[D.rows[o + i].obs] = 0;
      }
      tree(RS_SUMS);
      ba_lin_frame_end(D, g, partial.data(), count);
    }
  }
  void tracks() {
    if (idle()) return;
    for (int32_t t = 0; t < D.n_tracks; t++) ba_track_system(D, t);
  }
  // the six sums of W zt over a frame's rows
  void wz(int32_t g) {
    const int32_t o = D.row_off[g], n = D.row_off[g + 1] - o;
    partial.assign((size_t)RS_LANES * RS_SUMS, 0.0);
    for (int32_t i = 0; i < n; i++) ba_wz_row(D, D.rows[o + i], &partial[(size_t)(i % RS_LANES) * RS_SUMS]);
    tree(6);
  }
  void rhs() {
    if (idle()) return;
    double ab[42];
    for (int32_t g = 0; g < D.n_frames; g++) {
      wz(g);
      ba_rhs_frame_end(D, g, partial.data(), ab);
    }
  }
  void cg_init() {
    if (idle()) return;
    for (int32_t g = 0; g < D.n_frames; g++) ba_cg_frame_init(D, g);
    ba_cg_begin(D, dot(D.r, D.z));
  }
  void op_tracks() {
    if (solve_idle()) return;
    for (int32_t t = 0; t < D.n_tracks; t++) ba_op_track(D, t);
  }
  void op_frames() {
    if (solve_idle()) return;
    for (int32_t g = 0; g < D.n_frames; g++)
      if (D.ffree[g]) {
        wz(g);
        ba_op_frame_end(D, g, partial.data());
      }
  }
  void cg_step() {
    if (solve_idle()) return;
    if (!ba_cg_alpha(D, dot(D.p, D.q))) return;
    for (int32_t g = 0; g < D.n_frames; g++) ba_cg_frame_move(D, g, D.ctl->alpha);
    if (!ba_cg_beta(D, dot(D.r, D.z))) return;
    for (int32_t g = 0; g < D.n_frames; g++) ba_cg_frame_direction(D, g, D.ctl->beta);
  }
  void back() {
    if (idle()) return;
    for (int32_t t = 0; t < D.n_tracks; t++) ba_back_track(D, t);
    for (int32_t g = 0; g < D.n_frames; g++) ba_trial_frame(D, g);
  }
  void trial_cost() {
    if (idle()) return;
    for (int32_t g = 0; g < D.n_frames; g++) {
      const int32_t o = D.row_off[g], n = D.row_off[g + 1] - o;
      partial.assign((size_t)RS_LANES * RS_SUMS, 0.0);
      int32_t behind = 0;
      if (D.valid[g])
        for (int32_t i = 0; i < n; i++) ba_trial_row(D, D.trial_state + 12 * (size_t)g, D.rows[o + i], partial[(size_t)(i % RS_LANES) * RS_SUMS], behind);
      tree(1);
      D.tcost[g] = partial[0];
      D.tbehind[g] = behind;
    }
  }
  void decide() {
    if (idle()) return;
    ba_decide(D);
  }
  void commit(int32_t k) {
    if (!ba_commits(D, k)) return;
    for (int32_t g = 0; g < D.n_frames; g++) ba_commit_frame(D, g);
    for (int32_t t = 0; t < D.n_tracks; t++) ba_commit_track(D, t);
  }
  bool solve_over() const { return solve_idle(); }
  bool round_over(int32_t) const { return idle(); }
  void finish() {
    for (int32_t g = 0; g < D.n_frames; g++) ba_finish_frame(D, g);
  }
};

}  // namespace

extern "C" {

void vsm_adjust_default_params(vsm_adjust_params *p) {
  if (!p) return;
  p->min_observations = 10;
  p->min_track_observations = 2;
  p->max_rounds = 10;
  p->cg_iters = 40;
  p->lambda0 = 1e-3;
  p->lambda_min = 1e-9;
  p->lambda_max = 1e6;
  p->cg_tol = 1e-2;
  p->ftol = 1e-6;
  p->max_residual = 0.0;
  p->min_depth = 1e-10;
}

int32_t vsm_host_adjust(int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *refine, double f, double cu, double cv,
                        int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv, const double *xyz, const uint8_t *use,
                        const vsm_adjust_params *params, int32_t *frame_status, double *out_poses, int32_t *rows, int32_t *active, int32_t *track_status,
                        double *out_xyz, double *cost_before, double *cost_after, double *lambda, int32_t *cg_iters, int32_t *cg_end, int32_t *accepted,
                        int32_t *round_active, int32_t *n_rounds, int64_t *stats16) {
  if (pts_check_points(ba_params_ok(params), n_frames, poses, n_tracks, offsets, obs_frames, uv, xyz) < 0) return VSM_EARG;
  const size_t F = (size_t)n_frames, T = (size_t)n_tracks;
  // the rows by frame, one chunk; then the device path's block in one zeroed buffer, packed and bound as there
  std::vector<int32_t> at;
  RsGroup G(n_frames, n_tracks, offsets, use, RsObsArrays{obs_frames, uv}, 1, RsLoop(), at);
  const BaBlocks L(F, T, (size_t)G.row_off[F], n_tracks > 0 ? (size_t)offsets[T] : 0, (size_t)params->max_rounds);
  std::vector<uint8_t> block(L.dev_bytes, 0);
  L.pack(block.data(), poses, pose_valid, refine, G, xyz);
  HostOps o;
  const BaData &D = o.D = L.bind(block.data(), block.data() + L.out_at, f, cu, cv, *params);
  ba_schedule(o, *params);
  const BaCtl &ctl = *D.ctl;
  if (frame_status && F) memcpy(frame_status, D.fstatus, F * 4);
  if (out_poses && F) memcpy(out_poses, D.out_poses, F * 96);
  if (rows)
    for (size_t g = 0; g < F; g++) rows[g] = G.rows_of(g);
  if (active && F) memcpy(active, D.factive, F * 4);
  if (track_status && T) memcpy(track_status, D.tstatus, T * 4);
  if (out_xyz && T) memcpy(out_xyz, D.out_xyz, T * 24);
  ba_history(ctl.round, D.hist_d, D.hist_i, cost_before, cost_after, lambda, cg_iters, cg_end, accepted, round_active);
  if (n_rounds) *n_rounds = ctl.round;
  if (stats16) ba_stats(n_frames, D.fstatus, n_tracks, D.tstatus, ctl, stats16);
  return n_frames;
}

}  // extern "C"
