// Joint adjustment of poses and points (vsm_ba.hip, vsm_ba_host.cpp, vsm_ba.inc): damped Gauss-Newton
// rounds, the points eliminated, the reduced camera system solved by preconditioned conjugate gradients without forming its
// matrix.  include/visomatch.h has the contract; this header is the one statement of the arithmetic: every product, every
// sum and its order.  The kernels and the host view (one thread) both call the functions below on the same BaData - a
// block of pointers, into device memory there, into vectors here - and differ only in who calls them: a by-frame step deals
// a frame's rows to 256 lanes and adds the lanes' partial sums in a tree (the host walks the same 256 partial sums and the
// same tree in a loop), a by-track step is one lane per track walking the track's observations in ascending order, and the
// vector work of the conjugate gradient is one workgroup.  ba_schedule is the sequence of steps, the same on both sides: no
// step's launch depends on a value, a control block (BaCtl) turns the steps behind a finished solve or a finished call into
// no-ops.  Everything is double, every operation one of + - * /; build with -ffp-contract=off.
//
// The sums and their orders:
//  - per frame, the resection's 28 sums by rs_add_row, rows in rs_group_* order, row i of the frame to partial[i mod 256],
//    then the tree (vsm_resect.h); the same partials and tree for the 6 sums of W z (ba_wz_row) and the trial cost;
//  - per track, observations ascending from +0.0: the 6 upper entries of V and the 3 of gp (ba_add_obs: the u row's product,
//    then the v row's), and W^T p (ba_wt_sum: per observation, for j = 0..2, for m = 0..5);
//  - the scalar products over the 6 F entries (ba_dot_*): entry i = 6 g + m to partial[i mod 256], ascending, the entries of
//    held frames passed over, then the tree;
//  - the cost and the trial cost of the call: the frames' sums added in ascending frame order from +0.0 (ba_decide).
// An inactive row, a held track's row, a held frame's entry adds nothing - it is passed over, not added as zero.
#pragma once
#include <math.h>
#include <stdint.h>

#include "visomatch.h"
#include "vsm_linalg.h"
#include "vsm_points.h"
#include "vsm_resect.h"

enum { BA_LIN = 26 };  // doubles kept per active observation: W[18] (6x3, row-major), the u row of Jp [3], its v row [3], r[2]
enum { BA_FRAME_HELD = 7 };

// a row of a frame: 16 bytes - the resection's row and the observation's index, under which the row is found by track
struct BaRow {
  int32_t track, obs;
  float u, v;
};

// the control block: one per call, on the device in the device path
struct BaCtl {
  double lambda;           // of the round that is linearised next
  double rz, rz0;          // the conjugate gradient's r.z and its first value
  double alpha, beta;
  int32_t round;           // rounds decided
  int32_t done;            // the call has stopped: every later step is a no-op
  int32_t cg_done;         // the round's solve has ended: its later steps are no-ops
  int32_t cg_iters, cg_end;
  int32_t accepted;        // the last decision
  int32_t stop;            // why the call stopped: 1 ftol, 2 lambda_max, 3 max_rounds
  int32_t n_accepted, total_cg, pad_;
};

struct BaData {
  // input
  const double *poses;        // [F][12]
  const uint8_t *valid, *refine, *use;  // per frame, per frame, per track: bytes, never null here
  const int32_t *row_off;     // [F + 1]
  const BaRow *rows;          // by frame
  const int32_t *offsets;     // [T + 1]
  const int32_t *obs_frames;  // per observation
  const double *xyz_in;       // [T][3]
  // the state and the trial state
  double *state, *trial_state;  // [F][12], world to camera
  double *trial_X;              // [T][3] (the points themselves live in out_xyz)
  // a round's linearisation
  uint8_t *active;  // per observation
  double *lin;      // [n_obs][BA_LIN]
  double *usum;     // [F][28]
  int32_t *cnt;     // [F] active rows
  double *ud;       // [F][36] damped U
  double *uinv;     // [F][36] its inverse, for a free frame
  double *vinv;     // [T][9]
  double *gp, *zt;  // [T][3]
  uint8_t *ffree, *tfree, *moved;
  // the conjugate gradient's vectors, [6 F] each
  double *b, *x, *r, *z, *p, *q;
  double *tcost;     // [F]
  int32_t *tbehind;  // [F]
  BaCtl *ctl;
  // results
  int32_t *fstatus, *factive, *tstatus;
  double *out_poses, *out_xyz;
  double *hist_d;   // [max_rounds][3]: cost before, cost after, lambda
  int32_t *hist_i;  // [max_rounds][4]: CG iterations, CG end, accepted, active rows
  double f, cu, cv;
  vsm_adjust_params prm;
  int32_t n_frames, n_tracks;
};

// ---- per row ----
// the derivative of the prediction with respect to X, in rs_jacobian's form: R is the rotation part of the state S
template <class M>
VSM_HD inline void ba_jacobian_point(M S, const double *xc, double f, double *pu, double *pv) {
  const double x = xc[0], y = xc[1], z = xc[2], zz = z * z;
  for (int j = 0; j < 3; j++) {
    pu[j] = f * (S[0 * 4 + j] * z - x * S[2 * 4 + j]) / zz;
    pv[j] = f * (S[1 * 4 + j] * z - y * S[2 * 4 + j]) / zz;
  }
}
// W = Jc^T Jp, entry (m, j): the u rows' product, then the v rows'
VSM_HD inline void ba_w(const double *ju, const double *jv, const double *pu, const double *pv, double *W) {
  for (int m = 0; m < 6; m++)
    for (int j = 0; j < 3; j++) {
      double s = ju[m] * pu[j];
      s += jv[m] * pv[j];
      W[m * 3 + j] = s;
    }
}
// The linearisation of one row at the frame's state S: the row's activity byte; if active, its terms onto the frame's running
// sums (rs_add_row) and its record for the by-track steps.
template <class M, class Acc>
VSM_HD inline void ba_lin_row(const BaData &D, M S, const BaRow &row, double limit, Acc acc, int32_t &count) {
  const double *Xp = D.out_xyz + 3 * (size_t)row.track;
  const double P[3] = {Xp[0], Xp[1], Xp[2]};
  double xc[3], r[2], t;
  if (!rs_row(S, P, row.u, row.v, D.f, D.cu, D.cv, D.prm.min_depth, limit, xc, r, &t)) {
    D.active[row.obs] = 0;
    return;
  }
  D.active[row.obs] = 1;
  count++;
  double ju[6], jv[6], pu[3], pv[3];
  rs_jacobian(xc, D.f, ju, jv);
  ba_jacobian_point(S, xc, D.f, pu, pv);
  rs_add_row(acc, ju, jv, r, t);
  double *L = D.lin + (size_t)BA_LIN * row.obs;
  ba_w(ju, jv, pu, pv, L);
  for (int j = 0; j < 3; j++) {
    L[18 + j] = pu[j];
    L[21 + j] = pv[j];
  }
  L[24] = r[0];
  L[25] = r[1];
}
// an active row of a free track onto the frame's six sums of W z
template <class Acc>
VSM_HD inline void ba_wz_row(const BaData &D, const BaRow &row, Acc acc) {
  if (!D.active[row.obs] || !D.tfree[row.track]) return;
  const double *W = D.lin + (size_t)BA_LIN * row.obs, *z = D.zt + 3 * (size_t)row.track;
  for (int m = 0; m < 6; m++)
    for (int j = 0; j < 3; j++) acc[m] += W[m * 3 + j] * z[j];
}
// an active row at the trial state: its squared residual onto the frame's trial cost, or the verdict "behind the camera"
template <class M>
VSM_HD inline void ba_trial_row(const BaData &D, M S, const BaRow &row, double &acc, int32_t &behind) {
  if (!D.active[row.obs]) return;
  const double *X = D.trial_X + 3 * (size_t)row.track;
  const double x = pts_affine_row(S, 0, X[0], X[1], X[2]), y = pts_affine_row(S, 1, X[0], X[1], X[2]), z = pts_affine_row(S, 2, X[0], X[1], X[2]);
  if (!(z > D.prm.min_depth)) {
    behind = 1;
    return;
  }
  const double ru = (double)row.u - (D.f * x / z + D.cu), rv = (double)row.v - (D.f * y / z + D.cv);
  acc += ru * ru + rv * rv;
}

// ---- 3x3 ----
// Gauss-Jordan with full pivoting in pts_solve3's pattern (eps 1e-20), widened to three right-hand sides: ab is the
// row-major 3x6 [V | I], on success columns 3..5 hold the inverse of V
template <class M>
VSM_HD inline bool ba_invert3(M ab) {
  uint32_t ipiv = 0;
  int icol = 0, irow = 0;
  for (int i = 0; i < 3; i++) {
    double big = 0.0;
    for (int j = 0; j < 3; j++)
      if (((ipiv >> (4 * j)) & 15u) != 1u)
        for (int k = 0; k < 3; k++)
          if (((ipiv >> (4 * k)) & 15u) == 0u)
            if (fabs(ab[j * 6 + k]) >= big) {
              big = fabs(ab[j * 6 + k]);
              irow = j;
              icol = k;
            }
    ipiv += 1u << (4 * icol);
    if (irow != icol)
      for (int l = 0; l < 6; l++) {
        const double t = ab[irow * 6 + l];
        ab[irow * 6 + l] = ab[icol * 6 + l];
        ab[icol * 6 + l] = t;
      }
    if (fabs(ab[icol * 6 + icol]) < 1e-20) return false;
    const double pivinv = 1.0 / ab[icol * 6 + icol];
    ab[icol * 6 + icol] = 1.0;
    for (int l = 0; l < 6; l++) ab[icol * 6 + l] = ab[icol * 6 + l] * pivinv;
    for (int ll = 0; ll < 3; ll++)
      if (ll != icol) {
        const double dum = ab[ll * 6 + icol];
        ab[ll * 6 + icol] = 0.0;
        for (int l = 0; l < 6; l++) ab[ll * 6 + l] = ab[ll * 6 + l] - ab[icol * 6 + l] * dum;
      }
  }
  return true;
}
// out = A y for a row-major 3x3: every entry summed over k ascending from the k = 0 product
VSM_HD inline void ba_mul3(const double *A, const double *y, double *out) {
  for (int i = 0; i < 3; i++) {
    double s = A[i * 3 + 0] * y[0];
    s += A[i * 3 + 1] * y[1];
    s += A[i * 3 + 2] * y[2];
    out[i] = s;
  }
}

// ---- per track ----
// an active observation's terms onto acc[9]: the upper entries (a, b >= a) of V row after row, then gp
VSM_HD inline void ba_add_obs(double *acc, const double *L) {
  const double *pu = L + 18, *pv = L + 21;
  int k = 0;
  for (int a = 0; a < 3; a++)
    for (int c = a; c < 3; c++, k++) {
      acc[k] += pu[a] * pu[c];
      acc[k] += pv[a] * pv[c];
    }
  for (int a = 0; a < 3; a++) {
    acc[6 + a] += pu[a] * L[24];
    acc[6 + a] += pv[a] * L[25];
  }
}
// V, gp, the damped V's inverse, whether the track is free in the round, and zt = V^-1 gp for the right-hand side
VSM_HD inline void ba_track_system(const BaData &D, int32_t t) {
  D.tfree[t] = 0;
  if (!D.use[t]) {
    D.tstatus[t] = 1;
    return;
  }
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int32_t n = 0;
  for (int32_t i = D.offsets[t]; i < D.offsets[t + 1]; i++)
    if (D.active[i]) {
      n++;
      ba_add_obs(acc, D.lin + (size_t)BA_LIN * i);
    }
  double *gp = D.gp + 3 * (size_t)t;
  for (int a = 0; a < 3; a++) gp[a] = acc[6 + a];
  if (n < D.prm.min_track_observations) {
    D.tstatus[t] = 2;
    return;
  }
  const double damp = 1.0 + D.ctl->lambda;
  double ab[18];
  int k = 0;
  for (int a = 0; a < 3; a++)
    for (int c = a; c < 3; c++, k++) {
      ab[a * 6 + c] = acc[k];
      ab[c * 6 + a] = acc[k];
    }
  for (int a = 0; a < 3; a++) {
    ab[a * 6 + a] = ab[a * 6 + a] * damp;
    for (int c = 0; c < 3; c++) ab[a * 6 + 3 + c] = a == c ? 1.0 : 0.0;
  }
  if (!ba_invert3(ab)) {
    D.tstatus[t] = 3;
    return;
  }
  double *vi = D.vinv + 9 * (size_t)t;
  for (int a = 0; a < 3; a++)
    for (int c = 0; c < 3; c++) vi[a * 3 + c] = ab[a * 6 + 3 + c];
  D.tstatus[t] = 0;
  D.tfree[t] = 1;
  ba_mul3(vi, gp, D.zt + 3 * (size_t)t);
}
// y = sum of W^T vec_frame over the track's active observations in free frames
VSM_HD inline void ba_wt_sum(const BaData &D, int32_t t, const double *vec, double *y) {
  y[0] = y[1] = y[2] = 0.0;
  for (int32_t i = D.offsets[t]; i < D.offsets[t + 1]; i++) {
    const int32_t g = D.obs_frames[i];
    if (!D.active[i] || !D.ffree[g]) continue;
    const double *W = D.lin + (size_t)BA_LIN * i, *v = vec + 6 * (size_t)g;
    for (int j = 0; j < 3; j++)
      for (int m = 0; m < 6; m++) y[j] += W[m * 3 + j] * v[m];
  }
}
// the operator's first half: zt = V^-1 W^T p
VSM_HD inline void ba_op_track(const BaData &D, int32_t t) {
  if (!D.tfree[t]) return;
  double y[3];
  ba_wt_sum(D, t, D.p, y);
  ba_mul3(D.vinv + 9 * (size_t)t, y, D.zt + 3 * (size_t)t);
}
// back-substitution and the trial point
VSM_HD inline void ba_back_track(const BaData &D, int32_t t) {
  const double *X = D.out_xyz + 3 * (size_t)t;
  double *Xt = D.trial_X + 3 * (size_t)t;
  if (!D.tfree[t]) {
    for (int a = 0; a < 3; a++) Xt[a] = X[a];
    return;
  }
  double s[3], d[3], dX[3];
  ba_wt_sum(D, t, D.x, s);
  for (int a = 0; a < 3; a++) d[a] = D.gp[3 * (size_t)t + a] - s[a];
  ba_mul3(D.vinv + 9 * (size_t)t, d, dX);
  for (int a = 0; a < 3; a++) Xt[a] = X[a] + dX[a];
}

// ---- per frame ----
VSM_HD inline void ba_init_frame(const BaData &D, int32_t g) {
  pts_rigid_inverse(D.poses + 12 * (size_t)g, D.state + 12 * (size_t)g);
  D.moved[g] = 0;
}
// the linearisation's end: the frame's sums (zeros and no rows for a frame without a valid pose)
template <class Acc>
VSM_HD inline void ba_lin_frame_end(const BaData &D, int32_t g, Acc sums, int32_t count) {
  for (int k = 0; k < RS_SUMS; k++) D.usum[RS_SUMS * (size_t)g + k] = sums[k];
  D.cnt[g] = count;
}
// The damped U and - for a free frame - its inverse, whether the frame is free in the round, its status, and its part of the right-hand side gc - sum of W V^-1 gp
// (acc: the six sums of ba_wz_row); ab: 42 doubles of work space.
template <class Acc, class Wk>
VSM_HD inline void ba_rhs_frame_end(const BaData &D, int32_t g, Acc acc, Wk ab) {
  const double *sums = D.usum + RS_SUMS * (size_t)g;
  const double damp = 1.0 + D.ctl->lambda;
  double *Ud = D.ud + 36 * (size_t)g;
  int k = 0;
  for (int m = 0; m < 6; m++)
    for (int c = m; c < 6; c++, k++) {
      Ud[m * 6 + c] = sums[k];
      Ud[c * 6 + m] = sums[k];
    }
  for (int m = 0; m < 6; m++) Ud[m * 6 + m] = Ud[m * 6 + m] * damp;
  int32_t st = rs_early_status(D.valid[g], D.refine[g], D.row_off[g + 1] - D.row_off[g], D.prm.min_observations);
  bool free = false;
  if (st == 0) {
    if (D.cnt[g] >= D.prm.min_observations) {
      for (int i = 0; i < 36; i++) ab[i] = Ud[i];
      for (int m = 0; m < 6; m++) ab[36 + m] = sums[21 + m];
      free = vsm_la::solve6(ab, ab + 36);
      // U^-1 for the preconditioner, column after column: vsm_la::solve6 on a copy with the unit vector as right-hand side
      // (the pivots are the matrix's alone: every column succeeds where the first solve did)
      for (int c = 0; free && c < 6; c++) {
        for (int i = 0; i < 36; i++) ab[i] = Ud[i];
        for (int m = 0; m < 6; m++) ab[36 + m] = m == c ? 1.0 : 0.0;
        (void)vsm_la::solve6(ab, ab + 36);
        for (int m = 0; m < 6; m++) D.uinv[36 * (size_t)g + m * 6 + c] = ab[36 + m];
      }
    }
    if (!free) st = BA_FRAME_HELD;
  }
  D.fstatus[g] = st;
  D.factive[g] = D.cnt[g];
  D.ffree[g] = free ? 1 : 0;
  for (int m = 0; m < 6; m++) D.b[6 * (size_t)g + m] = free ? sums[21 + m] - acc[m] : 0.0;
}
// the operator's second half for a free frame: q = U p - sum of W zt, every entry of U p summed over c ascending from c = 0
template <class Acc>
VSM_HD inline void ba_op_frame_end(const BaData &D, int32_t g, Acc acc) {
  const double *Ud = D.ud + 36 * (size_t)g, *p = D.p + 6 * (size_t)g;
  for (int m = 0; m < 6; m++) {
    double s = Ud[m * 6 + 0] * p[0];
    for (int c = 1; c < 6; c++) s += Ud[m * 6 + c] * p[c];
    D.q[6 * (size_t)g + m] = s - acc[m];
  }
}
// the preconditioner: z = U^-1 r, every entry summed over c ascending from the c = 0 product (the frame is free: U^-1 stands)
VSM_HD inline void ba_precond(const BaData &D, int32_t g) {
  const double *Ui = D.uinv + 36 * (size_t)g, *r = D.r + 6 * (size_t)g;
  for (int m = 0; m < 6; m++) {
    double s = Ui[m * 6 + 0] * r[0];
    for (int c = 1; c < 6; c++) s += Ui[m * 6 + c] * r[c];
    D.z[6 * (size_t)g + m] = s;
  }
}
// the conjugate gradient's start for a frame: x = 0, r = b, z = U^-1 r, p = z (zeros for a held frame)
VSM_HD inline void ba_cg_frame_init(const BaData &D, int32_t g) {
  for (int m = 0; m < 6; m++) {
    const size_t i = 6 * (size_t)g + m;
    D.x[i] = 0.0;
    D.r[i] = D.b[i];
    D.z[i] = 0.0;
    D.q[i] = 0.0;
  }
  if (D.ffree[g]) ba_precond(D, g);
  for (int m = 0; m < 6; m++) D.p[6 * (size_t)g + m] = D.z[6 * (size_t)g + m];
}
VSM_HD inline void ba_cg_frame_move(const BaData &D, int32_t g, double alpha) {
  if (!D.ffree[g]) return;
  for (int m = 0; m < 6; m++) {
    const size_t i = 6 * (size_t)g + m;
    D.x[i] = D.x[i] + alpha * D.p[i];
    D.r[i] = D.r[i] - alpha * D.q[i];
  }
  ba_precond(D, g);
}
VSM_HD inline void ba_cg_frame_direction(const BaData &D, int32_t g, double beta) {
  if (!D.ffree[g]) return;
  for (int m = 0; m < 6; m++) {
    const size_t i = 6 * (size_t)g + m;
    D.p[i] = D.z[i] + beta * D.p[i];
  }
}
// the trial pose
VSM_HD inline void ba_trial_frame(const BaData &D, int32_t g) {
  double S[12];
  for (int i = 0; i < 12; i++) S[i] = D.state[12 * (size_t)g + i];
  if (D.ffree[g]) rs_move(S, D.x + 6 * (size_t)g);
  for (int i = 0; i < 12; i++) D.trial_state[12 * (size_t)g + i] = S[i];
}
VSM_HD inline void ba_finish_frame(const BaData &D, int32_t g) {
  if (D.moved[g])
    pts_rigid_inverse(D.state + 12 * (size_t)g, D.out_poses + 12 * (size_t)g);
  else
    for (int i = 0; i < 12; i++) D.out_poses[12 * (size_t)g + i] = D.poses[12 * (size_t)g + i];
}

// ---- the scalar products: lane l's partial sum of a . b ----
VSM_HD inline double ba_dot_partial(const BaData &D, const double *a, const double *b, int l) {
  double s = 0.0;
  for (int32_t i = l; i < 6 * D.n_frames; i += RS_LANES)
    if (D.ffree[i / 6]) s += a[i] * b[i];
  return s;
}

// ---- the control block's steps: one lane ----
VSM_HD inline void ba_ctl_init(const BaData &D) {
  BaCtl *c = D.ctl;
  c->lambda = D.prm.lambda0;
  c->rz = c->rz0 = c->alpha = c->beta = 0.0;
  c->round = c->done = c->cg_done = c->cg_iters = c->cg_end = c->accepted = c->stop = c->n_accepted = c->total_cg = c->pad_ = 0;
}
VSM_HD inline bool ba_cg_converged(const BaData &D, double rz) { return rz <= (D.prm.cg_tol * D.prm.cg_tol) * D.ctl->rz0; }
// with the first r.z
VSM_HD inline void ba_cg_begin(const BaData &D, double rz) {
  BaCtl *c = D.ctl;
  c->rz = c->rz0 = rz;
  c->cg_iters = c->cg_end = c->cg_done = 0;
  if (ba_cg_converged(D, rz)) {
    c->cg_done = 1;
    c->cg_end = 1;
  }
}
// with p.q: false ends the solve with x as it stands
VSM_HD inline bool ba_cg_alpha(const BaData &D, double pq) {
  BaCtl *c = D.ctl;
  if (!(pq > 0.0 && pq < HUGE_VAL)) {
    c->cg_done = 1;
    c->cg_end = 2;
    return false;
  }
  c->alpha = c->rz / pq;
  return true;
}
// with the new r.z: false ends the solve
VSM_HD inline bool ba_cg_beta(const BaData &D, double rz) {
  BaCtl *c = D.ctl;
  c->cg_iters++;
  if (ba_cg_converged(D, rz)) {
    c->cg_done = 1;
    c->cg_end = 1;
  } else if (c->cg_iters >= D.prm.cg_iters) {
    c->cg_done = 1;
    c->cg_end = 3;
  }
  c->beta = rz / c->rz;
  c->rz = rz;
  return !c->cg_done;
}
// the decision of a round, its history record and what it means for lambda and for the call
VSM_HD inline void ba_decide(const BaData &D) {
  BaCtl *c = D.ctl;
  double cost = 0.0, trial = 0.0;
  int32_t behind = 0, active = 0;
  for (int32_t g = 0; g < D.n_frames; g++)
    if (D.valid[g]) {
      cost += D.usum[RS_SUMS * (size_t)g + 27];
      trial += D.tcost[g];
      behind |= D.tbehind[g];
      active += D.cnt[g];
    }
  const bool accept = !behind && trial < HUGE_VAL && trial < cost;
  const int32_t k = c->round;
  D.hist_d[3 * k + 0] = cost;
  D.hist_d[3 * k + 1] = accept ? trial : cost;
  D.hist_d[3 * k + 2] = c->lambda;
  D.hist_i[4 * k + 0] = c->cg_iters;
  D.hist_i[4 * k + 1] = c->cg_end;
  D.hist_i[4 * k + 2] = accept ? 1 : 0;
  D.hist_i[4 * k + 3] = active;
  c->accepted = accept ? 1 : 0;
  c->total_cg += c->cg_iters;
  c->round = k + 1;
  int32_t stop = 0;
  if (accept) {
    c->n_accepted++;
    if (cost - trial <= D.prm.ftol * cost) stop = 1;
    double l = c->lambda / 10.0;
    if (l < D.prm.lambda_min) l = D.prm.lambda_min;
    c->lambda = l;
  } else {
    c->lambda = c->lambda * 10.0;
  }
  if (!stop && c->lambda > D.prm.lambda_max) stop = 2;
  if (!stop && c->round >= D.prm.max_rounds) stop = 3;
  if (stop) {
    c->stop = stop;
    c->done = 1;
  }
}
// round k's accepted step becomes the state
VSM_HD inline bool ba_commits(const BaData &D, int32_t k) { return D.ctl->accepted && D.ctl->round == k + 1; }
VSM_HD inline void ba_commit_frame(const BaData &D, int32_t g) {
  if (!D.ffree[g]) return;
  for (int i = 0; i < 12; i++) D.state[12 * (size_t)g + i] = D.trial_state[12 * (size_t)g + i];
  D.moved[g] = 1;
}
VSM_HD inline void ba_commit_track(const BaData &D, int32_t t) {
  if (!D.tfree[t]) return;
  for (int a = 0; a < 3; a++) D.out_xyz[3 * (size_t)t + a] = D.trial_X[3 * (size_t)t + a];
}

// ---- the sequence of steps, the same for the kernels' launches and the host view's loops ----
// Every step looks at the control block itself; round_over(k) is where a side that can look at it (the host view at once,
// the device path after a wait) stops enqueuing, and solve_over() likewise for the solve.  Neither changes a result.
template <class Ops>
inline void ba_schedule(Ops &o, const vsm_adjust_params &prm) {
  o.init();
  for (int32_t k = 0; k < prm.max_rounds; k++) {
    o.linearise();
    o.tracks();
    o.rhs();
    o.cg_init();
    for (int32_t i = 0; i < prm.cg_iters && !o.solve_over(); i++) {
      o.op_tracks();
      o.op_frames();
      o.cg_step();
    }
    o.back();
    o.trial_cost();
    o.decide();
    o.commit(k);
    if (o.round_over(k)) break;
  }
  o.finish();
}

// ---- host side (vsm_ba_host.cpp; no HIP) ----
bool ba_params_ok(const vsm_adjust_params *params);  // the test of the parameters (the arguments: pts_check_points)
// the rows by frame are the resection's (RsGroup, vsm_resect.h), with the observation's index in the row
inline void row_set(BaRow &r, int32_t t, int32_t i) { r.track = t, r.obs = i; }
// the 16 stats from the results (include/visomatch.h)
void ba_stats(int32_t n_frames, const int32_t *fstatus, int32_t n_tracks, const int32_t *tstatus, const BaCtl &ctl, int64_t *out16);
// the rounds' history from hist_d [rounds][3] and hist_i [rounds][4] into the seven columns a caller wants
void ba_history(int32_t rounds, const double *hist_d, const int32_t *hist_i, double *cost_before, double *cost_after, double *lambda, int32_t *cg_iters,
                int32_t *cg_end, int32_t *accepted, int32_t *active);

// ---- device path (vsm_ba.hip) ----
#ifdef __HIP__
struct VsmProf;
// Enqueues the call's steps on s.  ctl_host: pinned room for the control block, which the wait per round copies back;
// fixed_schedule: no waits, every launch of max_rounds rounds enqueued.  hipSuccess, or the first error of a wait.
hipError_t vsm_ba_launch(hipStream_t s, VsmProf &pf, const BaData &d, BaCtl *ctl_host, bool fixed_schedule);
#endif
