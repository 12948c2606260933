// Refinement of camera poses against triangulated points (vsm_resect.hip, vsm_resect_host.cpp,
// vsm_resect.inc): motion-only bundle adjustment, one Gauss-Newton resection per frame.  include/visomatch.h has the
// contract; this header is the one statement of the arithmetic: every product, every sum and its order.  The kernel (a
// 256-thread workgroup per frame) and the host view (one thread) both call the functions below and differ only in who
// calls them: the workgroup deals a frame's rows to its lanes and adds the lanes' partial sums in a tree, the host walks
// the same 256 partial sums and the same tree in a loop.  Everything is double, every operation one of + - * /: the
// rotation moves by a Cayley step, so no trigonometric function is in here, and not one of libm's (the host applies
// sqrt to the two sums of squares afterwards).  Build with -ffp-contract=off.
//
// The sums of one evaluation: RS_SUMS = 28 doubles - sums 0..20 the upper entries (m, c >= m) of J^T J row after row,
// 21..26 the entries of J^T r, 27 the sum of ru^2 + rv^2 - and the count of used rows, an int32 (integer addition has no
// order, a frame has fewer than 2^31 rows).
// A used row adds, to sum (m, c): first Ju[m] * Ju[c], then Jv[m] * Jv[c]; to sum 21 + m: first Ju[m] * ru, then Jv[m] *
// rv; to sum 27: the one number ru * ru + rv * rv.  A skipped row adds nothing - it is passed over, not added as zero -
// and keeps its place: row i of the frame belongs to partial[i mod RS_LANES] whether it is used or not.  (A partial sum
// starts at +0.0 and can therefore never be -0.0, so adding a zero would not show; passing over is what keeps a NaN out.)
// The tests of a row let no NaN and no infinity into a sum; a sum can still overflow (a min_depth near zero), and what
// follows from an infinite sum is the same sequence of operations on both sides, but a NaN's sign and payload are not
// part of the definition.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "visomatch.h"
#include "vsm_linalg.h"
#include "vsm_points.h"

enum { RS_SUMS = 28, RS_LANES = 256 };
enum { RS_UPDATED = -1, RS_CONVERGED = 0, RS_NO_PIVOT = 5 };  // rs_step: the update's result (the two statuses by their values)

// a row of a frame: 12 bytes
struct RsRow {
  int32_t track;
  float u, v;
};

// the statuses that need no arithmetic: 1, 2, 3, or 0 = there is work
VSM_HD inline int32_t rs_early_status(int valid, int refine, int32_t rows, int32_t min_observations) {
  if (!valid) return 1;
  if (!refine) return 2;
  if (rows < min_observations) return 3;
  return 0;
}

// the gate as the number t = ru^2 + rv^2 has to stay below: NaNs and infinities never do
VSM_HD inline double rs_limit(double max_residual) { return max_residual > 0 ? max_residual * max_residual : HUGE_VAL; }

// One row at the state S = [Rw | tw] (3x4, row-major): the point in the camera frame xc[3], the residuals r[2] (observed -
// predicted) and t = ru^2 + rv^2.  false: the row is skipped (what has been written is not to be used).
template <class M>
VSM_HD inline bool rs_row(M S, const double *X, float u, float v, double f, double cu, double cv, double min_depth, double limit, double *xc, double *r,
                          double *t) {
  xc[0] = pts_affine_row(S, 0, X[0], X[1], X[2]);
  xc[1] = pts_affine_row(S, 1, X[0], X[1], X[2]);
  xc[2] = pts_affine_row(S, 2, X[0], X[1], X[2]);
  if (!(xc[2] > min_depth)) return false;
  r[0] = (double)u - (f * xc[0] / xc[2] + cu);
  r[1] = (double)v - (f * xc[1] / xc[2] + cv);
  *t = r[0] * r[0] + r[1] * r[1];
  return *t < limit;
}

// The derivative of the prediction for Xc' = Xc + w x Xc + tau with respect to (w, tau): the rows ju[6], jv[6], in the form
// of the stereo egomotion's update (vsm_ego.cpp) - the zeros and ones of dXc take part as numbers.
VSM_HD inline void rs_jacobian(const double *xc, double f, double *ju, double *jv) {
  const double x = xc[0], y = xc[1], z = xc[2], zz = z * z;
  const double dx[6] = {0, z, -y, 1, 0, 0}, dy[6] = {-z, 0, x, 0, 1, 0}, dz[6] = {y, -x, 0, 0, 0, 1};
  for (int j = 0; j < 6; j++) {
    ju[j] = f * (dx[j] * z - x * dz[j]) / zz;
    jv[j] = f * (dy[j] * z - y * dz[j]) / zz;
  }
}

// a used row's terms onto running sums (the order: the head of this file)
template <class Acc>
VSM_HD inline void rs_add_row(Acc acc, const double *ju, const double *jv, const double *r, double t) {
  int k = 0;
  for (int m = 0; m < 6; m++)
    for (int c = m; c < 6; c++, k++) {
      acc[k] += ju[m] * ju[c];
      acc[k] += jv[m] * jv[c];
    }
  for (int m = 0; m < 6; m++) {
    acc[21 + m] += ju[m] * r[0];
    acc[21 + m] += jv[m] * r[1];
  }
  acc[27] += t;
}

// The update half of rs_step, which the joint adjustment (vsm_ba.h) takes its trial poses from: with delta d = (w, tau), a =
// w / 2: Rd = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a), Rw <- Rd Rw, tw <- Rd tw + tau, every product summed over k
// ascending from the k = 0 product.
template <class M>
VSM_HD inline void rs_move(M S, const double *d) {
  const double a0 = 0.5 * d[0], a1 = 0.5 * d[1], a2 = 0.5 * d[2];
  const double aa = a0 * a0 + a1 * a1 + a2 * a2, den = 1.0 + aa, one = 1.0 - aa;
  double Rd[9];
  Rd[0] = (one + 2.0 * (a0 * a0)) / den;
  Rd[1] = (2.0 * (a0 * a1) - 2.0 * a2) / den;
  Rd[2] = (2.0 * (a0 * a2) + 2.0 * a1) / den;
  Rd[3] = (2.0 * (a1 * a0) + 2.0 * a2) / den;
  Rd[4] = (one + 2.0 * (a1 * a1)) / den;
  Rd[5] = (2.0 * (a1 * a2) - 2.0 * a0) / den;
  Rd[6] = (2.0 * (a2 * a0) - 2.0 * a1) / den;
  Rd[7] = (2.0 * (a2 * a1) + 2.0 * a0) / den;
  Rd[8] = (one + 2.0 * (a2 * a2)) / den;
  double N[12];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 4; j++) {
      double s = Rd[i * 3 + 0] * S[0 * 4 + j];
      s += Rd[i * 3 + 1] * S[1 * 4 + j];
      s += Rd[i * 3 + 2] * S[2 * 4 + j];
      N[i * 4 + j] = s;
    }
    N[i * 4 + 3] = N[i * 4 + 3] + d[3 + i];
  }
  for (int i = 0; i < 12; i++) S[i] = N[i];
}

// From an evaluation's sums to the next state: the 6x6 system into ab (36 + 6 doubles of work space), vsm_la::solve6,
// and rs_move by the solution delta.  RS_NO_PIVOT: S is untouched.  RS_CONVERGED: all six |delta| <= eps (the state has
// moved by that last delta).
template <class Sums, class W, class M>
VSM_HD inline int rs_step(Sums sums, W ab, M S, double eps) {
  int k = 0;
  for (int m = 0; m < 6; m++)
    for (int c = m; c < 6; c++, k++) {
      ab[m * 6 + c] = sums[k];
      ab[c * 6 + m] = sums[k];
    }
  for (int m = 0; m < 6; m++) ab[36 + m] = sums[21 + m];
  if (!vsm_la::solve6(ab, ab + 36)) return RS_NO_PIVOT;
  double d[6];
  for (int m = 0; m < 6; m++) d[m] = ab[36 + m];
  rs_move(S, d);
  for (int m = 0; m < 6; m++)
    if (!(fabs(d[m]) <= eps)) return RS_UPDATED;
  return RS_CONVERGED;
}

// The frame's loop, given `evaluate(S, sums, &count, jacobian)`: sums[RS_SUMS] and the count of the used rows at the state
// S (without the Jacobian only sums[27] and the count are wanted).  The kernel's lane 0 and the host view both follow
// exactly this sequence; the kernel spells it out around its barriers (k_rs_resect), the host view calls it.
struct RsResult {
  int32_t status, updates, used_before, used;
  double ss_before, ss_after;
};
template <class Eval, class W, class M>
inline void rs_frame(Eval evaluate, W ab, M S, const vsm_resect_params &prm, RsResult *out) {
  double sums[RS_SUMS];
  int32_t count = 0;
  out->status = 6;
  out->updates = 0;
  out->used_before = out->used = 0;
  out->ss_before = out->ss_after = 0;
  while (out->updates < prm.max_updates) {
    evaluate(S, sums, &count, true);
    if (out->updates == 0) {
      out->ss_before = sums[27];
      out->used_before = count;
    }
    out->used = count;
    if (count < prm.min_observations) {
      out->status = 4;
      return;
    }
    const int r = rs_step(sums, ab, S, prm.eps);
    if (r == RS_NO_PIVOT) {
      out->status = 5;
      return;
    }
    out->updates++;
    if (r == RS_CONVERGED) {
      out->status = 0;
      break;
    }
  }
  evaluate(S, sums, &count, false);
  out->ss_after = sums[27];
  out->used = count;
}

// ---- host side (vsm_resect_host.cpp; no HIP) ----
bool rs_params_ok(const vsm_resect_params *params);  // the test of the parameters (the arguments: pts_check_points)
// An observation source gives frame_of(i), observation i's frame, and pixel_of(i, &u, &v), its pixel.  This one is the
// caller's arrays; the handle's track result and match lists are the other (TracksObs, vsm_points.inc).
struct RsObsArrays {
  const int32_t *obs_frames;
  const float *uv;
  int32_t frame_of(int32_t i) const { return obs_frames[i]; }
  void pixel_of(int32_t i, float *u, float *v) const {
    *u = uv[2 * (size_t)i];
    *v = uv[2 * (size_t)i + 1];
  }
};
// what a row keeps of its track and observation beside the pixel (vsm_ba.h has BaRow's)
inline void row_set(RsRow &r, int32_t t, int32_t) { r.track = t; }
// the two passes over the tracks t0 .. t1 - 1 of one chunk: its rows per frame, added to cnt[n_frames]; then, with at[g]
// where the chunk's first row of frame g belongs, the rows themselves (obs by value: a copy no store of the loop can alias)
template <class Obs>
inline void rs_group_count(int32_t t0, int32_t t1, const int32_t *offsets, const uint8_t *use, Obs obs, int32_t *cnt) {
  for (int32_t t = t0; t < t1; t++)
    if (!use || use[t])
      for (int32_t i = offsets[t]; i < offsets[t + 1]; i++) cnt[obs.frame_of(i)]++;
}
template <class Obs, class Row>
inline void rs_group_fill(int32_t t0, int32_t t1, const int32_t *offsets, const uint8_t *use, Obs obs, int32_t *at, Row *rows) {
  for (int32_t t = t0; t < t1; t++)
    if (!use || use[t])
      for (int32_t i = offsets[t]; i < offsets[t + 1]; i++) {
        Row &r = rows[at[obs.frame_of(i)]++];
        row_set(r, t, i);
        obs.pixel_of(i, &r.u, &r.v);
      }
}
// the chunks of tracks the device paths group n_obs observations in, and the host views' runner: a loop
inline int rs_group_chunks(int64_t n_obs) { return (int)std::max<int64_t>(1, std::min<int64_t>(32, n_obs / 512)); }
struct RsLoop {
  template <class Fn>
  void operator()(int n, Fn fn) const {
    for (int c = 0; c < n; c++) fn(c);
  }
};
// The rows by frame: a stable counting sort of the observations of the tracks in use (use null: all), a chunk of tracks per
// task of run(chunks, fn).  Every chunk counts its rows per frame, the counts of the chunks in front give a chunk its place
// in every frame - so the order is that of one chunk, ascending (track, observation) within a frame, whatever the chunk
// count: the sort is stable -, and the chunks write their rows side by side.  Two phases, because the row count sizes the
// block the rows go to: the constructor fills row_off[n_frames + 1] and turns `at` ([chunks][n_frames], the caller's, so
// that a stage keeps its allocation) into the chunks' places; fill(rows) - once - writes the rows.  offsets may be null
// without tracks.
template <class Obs, class Run>
struct RsGroup {
  const size_t F;
  const int32_t n_tracks;
  const int32_t *const offsets;
  const uint8_t *const use;
  const Obs obs;
  const int chunks;
  Run run;
  std::vector<int32_t> &at;
  std::vector<int32_t> row_off;
  RsGroup(int32_t n_frames, int32_t n_tracks_, const int32_t *offsets_, const uint8_t *use_, const Obs &obs_, int chunks_, Run run_, std::vector<int32_t> &at_)
      : F((size_t)n_frames), n_tracks(n_tracks_), offsets(offsets_), use(use_), obs(obs_), chunks(chunks_), run(run_), at(at_), row_off(F + 1, 0) {
    at.assign((size_t)chunks * F, 0);
    if (n_tracks > 0 && F > 0) run(chunks, [&](int c) { rs_group_count(first_track(c), first_track(c + 1), offsets, use, obs, at.data() + (size_t)c * F); });
    for (size_t g = 0; g < F; g++) {
      int32_t place = row_off[g];
      for (int c = 0; c < chunks; c++) {
        const int32_t n = at[(size_t)c * F + g];
        at[(size_t)c * F + g] = place;
        place += n;
      }
      row_off[g + 1] = place;
    }
  }
  int32_t first_track(int c) const { return (int32_t)((int64_t)n_tracks * c / chunks); }
  int32_t rows_of(size_t g) const { return row_off[g + 1] - row_off[g]; }
  template <class Row>
  void fill(Row *rows) {
    if (row_off[F] > 0) run(chunks, [&](int c) { rs_group_fill(first_track(c), first_track(c + 1), offsets, use, obs, at.data() + (size_t)c * F, rows); });
  }
};
// the tree over the first n sums of the partials [RS_LANES][RS_SUMS], as a loop; the sums are partial[0 .. n - 1] afterwards
inline void rs_host_tree(double *partial, int n) {
  for (int s = RS_LANES / 2; s >= 1; s >>= 1)
    for (int l = 0; l < s; l++)
      for (int k = 0; k < n; k++) partial[(size_t)l * RS_SUMS + k] += partial[(size_t)(l + s) * RS_SUMS + k];
}
// libm's part: sqrt(ss / used), 0 where nothing was used
double rs_rms(double ss, int32_t used);

// ---- device path (vsm_resect.hip) ----
#ifdef __HIP__
struct VsmProf;
struct RsDevice {
  // uploaded
  const double *poses;      // [n_frames][12]
  const uint8_t *valid;     // per frame
  const uint8_t *refine;    // per frame
  const int32_t *row_off;   // [n_frames + 1]
  const RsRow *rows;        // by frame
  const double *xyz;        // [n_tracks][3]
  // results, per frame
  int32_t *status, *updates, *used_before, *used;
  double *out_poses, *ss_before, *ss_after;
  double f, cu, cv;
  vsm_resect_params prm;
  int32_t n_frames;
};
void vsm_resect_launch(hipStream_t s, VsmProf &pf, const RsDevice &d);
#endif
