// Joint adjustment of poses and points, the host side without HIP: the argument checks, the stats and vsm_host_adjust - one
// host thread walking the functions and the schedule of vsm_ba.h, the 256 partial sums and their tree in a loop.  The host
// view is the CPU suite's subject, the device path's second opinion and the benchmark's baseline, never a fallback.
#include "vsm_ba.h"

#include <math.h>
#include <string.h>

#include <vector>

static bool ba_positive_finite(double x) { return x > 0 && x < HUGE_VAL; }

bool ba_params_ok(const vsm_adjust_params *p) {
  return p && p->min_observations >= 6 && p->max_rounds >= 1 && p->cg_iters >= 1 && ba_positive_finite(p->lambda0) && ba_positive_finite(p->cg_tol) &&
         ba_positive_finite(p->ftol);
}

int64_t ba_check_args(int32_t n_frames, const double *poses, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv,
                      const double *xyz, const vsm_adjust_params *params) {
  if (!ba_params_ok(params) || (n_tracks > 0 && !xyz)) return -1;
  return pts_check_obs(n_frames, poses, n_tracks, offsets, obs_frames, uv);
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

namespace {

// the steps of ba_schedule as loops
struct HostOps {
  BaData D;
  std::vector<double> partial;  // [RS_LANES][RS_SUMS]

  // the tree over the first n sums of the 256 partials; the sums are partial[0 .. n - 1] afterwards
  void tree(int n) {
    for (int s = RS_LANES / 2; s >= 1; s >>= 1)
      for (int l = 0; l < s; l++)
        for (int k = 0; k < n; k++) partial[(size_t)l * RS_SUMS + k] += partial[(size_t)(l + s) * RS_SUMS + k];
  }
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
  if (ba_check_args(n_frames, poses, n_tracks, offsets, obs_frames, uv, xyz, params) < 0) return VSM_EARG;
  const size_t F = (size_t)n_frames, T = (size_t)n_tracks;
  const int32_t zero = 0;
  if (n_tracks <= 0) offsets = &zero;
  const size_t N = (size_t)offsets[T];
  // the rows by frame, one chunk
  const auto frame_of = [&](int32_t i) { return obs_frames[i]; };
  const auto pixel_of = [&](int32_t i, float *u, float *v) {
    *u = uv[2 * (size_t)i];
    *v = uv[2 * (size_t)i + 1];
  };
  std::vector<int32_t> row_off(F + 1, 0);
  rs_group_count(0, n_tracks, offsets, use, frame_of, row_off.data() + 1);
  for (size_t g = 0; g < F; g++) row_off[g + 1] += row_off[g];
  std::vector<BaRow> table((size_t)row_off[F] + 1);
  std::vector<int32_t> at(row_off.begin(), row_off.end() - 1);
  ba_group_fill(0, n_tracks, offsets, use, frame_of, pixel_of, at.data(), table.data());
  // the masks as bytes, the working set
  std::vector<uint8_t> b_valid(F + 1), b_refine(F + 1), b_use(T + 1), b_active(N + 1, 0), b_ffree(F + 1, 0), b_tfree(T + 1, 0), b_moved(F + 1, 0);
  for (size_t g = 0; g < F; g++) {
    b_valid[g] = (!pose_valid || pose_valid[g]) ? 1 : 0;
    b_refine[g] = (!refine || refine[g]) ? 1 : 0;
  }
  for (size_t t = 0; t < T; t++) b_use[t] = (!use || use[t]) ? 1 : 0;
  std::vector<double> state(12 * F + 1), trial_state(12 * F + 1), trial_X(3 * T + 1), lin((size_t)BA_LIN * N + 1), usum(RS_SUMS * F + 1), ud(36 * F + 1), uinv(36 * F + 1),
      vinv(9 * T + 1), gp(3 * T + 1), zt(3 * T + 1, 0.0), cg(6 * 6 * F + 1), tcost(F + 1), o_poses(12 * F + 1), o_xyz(3 * T + 1),
      hist_d(3 * (size_t)params->max_rounds);
  std::vector<int32_t> cnt(F + 1), tbehind(F + 1), fstatus(F + 1), factive(F + 1), tstatus(T + 1), hist_i(4 * (size_t)params->max_rounds);
  BaCtl ctl;
  HostOps o;
  BaData &D = o.D;
  memset(&D, 0, sizeof(D));
  D.poses = poses;
  D.valid = b_valid.data();
  D.refine = b_refine.data();
  D.use = b_use.data();
  D.row_off = row_off.data();
  D.rows = table.data();
  D.offsets = offsets;
  D.obs_frames = obs_frames;
  D.xyz_in = xyz;
  D.state = state.data();
  D.trial_state = trial_state.data();
  D.trial_X = trial_X.data();
  D.active = b_active.data();
  D.lin = lin.data();
  D.usum = usum.data();
  D.cnt = cnt.data();
  D.ud = ud.data();
  D.uinv = uinv.data();
  D.vinv = vinv.data();
  D.gp = gp.data();
  D.zt = zt.data();
  D.ffree = b_ffree.data();
  D.tfree = b_tfree.data();
  D.moved = b_moved.data();
  D.b = cg.data();
  D.x = D.b + 6 * F;
  D.r = D.x + 6 * F;
  D.z = D.r + 6 * F;
  D.p = D.z + 6 * F;
  D.q = D.p + 6 * F;
  D.tcost = tcost.data();
  D.tbehind = tbehind.data();
  D.ctl = &ctl;
  D.fstatus = fstatus.data();
  D.factive = factive.data();
  D.tstatus = tstatus.data();
  D.out_poses = o_poses.data();
  D.out_xyz = o_xyz.data();
  D.hist_d = hist_d.data();
  D.hist_i = hist_i.data();
  D.f = f;
  D.cu = cu;
  D.cv = cv;
  D.prm = *params;
  D.n_frames = n_frames;
  D.n_tracks = n_tracks;
  ba_schedule(o, *params);
  if (frame_status && F) memcpy(frame_status, fstatus.data(), F * 4);
  if (out_poses && F) memcpy(out_poses, o_poses.data(), F * 96);
  if (rows)
    for (size_t g = 0; g < F; g++) rows[g] = row_off[g + 1] - row_off[g];
  if (active && F) memcpy(active, factive.data(), F * 4);
  if (track_status && T) memcpy(track_status, tstatus.data(), T * 4);
  if (out_xyz && T) memcpy(out_xyz, o_xyz.data(), T * 24);
  for (int32_t k = 0; k < ctl.round; k++) {
    if (cost_before) cost_before[k] = hist_d[3 * (size_t)k];
    if (cost_after) cost_after[k] = hist_d[3 * (size_t)k + 1];
    if (lambda) lambda[k] = hist_d[3 * (size_t)k + 2];
    if (cg_iters) cg_iters[k] = hist_i[4 * (size_t)k];
    if (cg_end) cg_end[k] = hist_i[4 * (size_t)k + 1];
    if (accepted) accepted[k] = hist_i[4 * (size_t)k + 2];
    if (round_active) round_active[k] = hist_i[4 * (size_t)k + 3];
  }
  if (n_rounds) *n_rounds = ctl.round;
  if (stats16) ba_stats(n_frames, fstatus.data(), n_tracks, tstatus.data(), ctl, stats16);
  return n_frames;
}

}  // extern "C"
