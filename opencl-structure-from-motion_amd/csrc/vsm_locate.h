// Location of frames without a pose against the points (vsm_locate.hip, vsm_locate_host.cpp,
// vsm_locate.inc): RANSAC over a linear six-point resection, the winner refined by the resection's own update loop.
// include/visomatch.h has the contract; this header is the one statement of the fit's arithmetic: every product, every sum
// and its order.  The kernel (a 16-lane group per (frame, hypothesis)) and the host view (one thread) both call the
// functions below and differ only in who runs the two decompositions between them: the group runs vsm_la::svd_group on
// matrices in LDS, the host vsm_la::svd_nr on arrays - the same sums in the same order (vsm_svd_coop.h).  Everything is
// double, every operation one of + - * /, sqrt (inside the decompositions) or a comparison, as in the mono fit.  Build with
// -ffp-contract=off.  The inlier test and the refinement are the resection's (rs_row, the resection itself; vsm_resect.h).
//
// What the decomposition guarantees about the order (vsm_la::svd_nr, Matrix::svd): on return the singular values are in
// decreasing order - a shell sort on w with the strict test w[j - inc] < w[j], so equal values keep the order the sort's
// increments leave them in - and the columns of U and V have moved with them.  Column N - 1 of V therefore belongs to the
// smallest singular value; where several are equal (a rank-deficient sample) it is whichever the sort left last, the same
// on both sides.  The fundamental-matrix fit takes its ninth column the same way (vsm_mono.hip, mono_fit_group).
//
// No NaN and no infinity enters a decomposition: the rows a sample is drawn from are eligible (finite pixel, finite
// point), lc_condition refuses a sample whose mean overflows, and then every entry of the matrix is a finite number of
// modest size.  (Matrix::svd is not safe against NaNs: vsm_points.h, PTS_SVD_PAD.)
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "visomatch.h"
#include "vsm_linalg.h"
#include "vsm_points.h"
#include "vsm_resect.h"

enum { LC_SAMPLE = 6, LC_N = 12 };
// a group's LDS (the host view's arrays): U 144 + V 144 + W 12 + RV 12 doubles
enum { LC_U = 0, LC_V = 144, LC_W = 288, LC_RV = 300, LC_GROUP_DOUBLES = 312 };
// where the group keeps the second decomposition and p once the first is done (all inside U's 144 doubles)
enum { LC_U3 = 0, LC_V3 = 16, LC_W3 = 32, LC_RV3 = 40, LC_P = 48 };

VSM_HD inline bool lc_finite(double x) { return x > -HUGE_VAL && x < HUGE_VAL; }
// a row one may sample and count: finite pixel, finite point
VSM_HD inline bool lc_eligible(float u, float v, const double *X) {
  return lc_finite((double)u) && lc_finite((double)v) && lc_finite(X[0]) && lc_finite(X[1]) && lc_finite(X[2]);
}
// the engine's first state
VSM_HD inline uint32_t lc_seed_state(uint32_t seed) {
  const uint32_t s = seed % 2147483647u;
  return s ? s : 1u;
}

// step 2: mean and scale of the six points P[6][3]; false: the hypothesis is invalid
VSM_HD inline bool lc_condition(const double *P, double *m, double *s) {
  for (int c = 0; c < 3; c++) {
    double sum = P[c];
    for (int i = 1; i < LC_SAMPLE; i++) sum += P[3 * i + c];
    m[c] = sum / 6.0;
  }
  double big = 0.0;
  for (int i = 0; i < LC_SAMPLE; i++)
    for (int c = 0; c < 3; c++) {
      const double d = fabs(P[3 * i + c] - m[c]);
      if (d > big) big = d;
    }
  *s = big;
  return big > 0.0 && big < HUGE_VAL;
}

// steps 1 and 3: rows 2 i and 2 i + 1 of A (row-major 12 x 12) from sample i's pixel and point
template <class A>
VSM_HD inline void lc_rows(A a, int i, float u, float v, const double *X, const double *m, double s, double f, double cu, double cv) {
  const double x = ((double)u - cu) / f, y = ((double)v - cv) / f;
  const double q[4] = {(X[0] - m[0]) / s, (X[1] - m[1]) / s, (X[2] - m[2]) / s, 1.0};
  for (int j = 0; j < 4; j++) {
    a[(2 * i) * LC_N + j] = q[j];
    a[(2 * i) * LC_N + 4 + j] = 0.0;
    a[(2 * i) * LC_N + 8 + j] = -x * q[j];
    a[(2 * i + 1) * LC_N + j] = 0.0;
    a[(2 * i + 1) * LC_N + 4 + j] = q[j];
    a[(2 * i + 1) * LC_N + 8 + j] = -y * q[j];
  }
}

// steps 5 (behind the second decomposition) and 6: the state S[12] = [R | tw] from p[12], U3, w3, V3 (3 x 3, row-major),
// the mean and the scale.  false: one of the twelve is not finite.
template <class Pv, class Mv, class Wv>
VSM_HD inline bool lc_state(Pv p, Mv U3, Wv w3, Mv V3, const double *m, double s, double *S) {
  double R0[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double t = U3[i * 3 + 0] * V3[j * 3 + 0];
      t += U3[i * 3 + 1] * V3[j * 3 + 1];
      t += U3[i * 3 + 2] * V3[j * 3 + 2];
      R0[i * 3 + j] = t;
    }
  const double d = R0[0] * (R0[4] * R0[8] - R0[5] * R0[7]) - R0[1] * (R0[3] * R0[8] - R0[5] * R0[6]) + R0[2] * (R0[3] * R0[7] - R0[4] * R0[6]);
  const double sigma = d > 0.0 ? 1.0 : -1.0;
  const double lambda = sigma * (3.0 / ((w3[0] + w3[1]) + w3[2]));
  bool ok = true;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) S[i * 4 + j] = sigma * R0[i * 3 + j];
    S[i * 4 + 3] = (lambda * p[4 * i + 3]) * s - ((S[i * 4 + 0] * m[0] + S[i * 4 + 1] * m[1]) + S[i * 4 + 2] * m[2]);
    for (int j = 0; j < 4; j++) ok = ok && lc_finite(S[i * 4 + j]);
  }
  return ok;
}
// the other half of validity: a sampled point in front of the camera
VSM_HD inline bool lc_in_front(const double *S, const double *X, double min_depth) { return pts_affine_row(S, 2, X[0], X[1], X[2]) > min_depth; }

// an eligible row's vote at the state S: the resection's test
template <class M>
VSM_HD inline bool lc_inlier(M S, const double *X, float u, float v, double f, double cu, double cv, double min_depth, double limit) {
  double xc[3], r[2], t;
  return rs_row(S, X, u, v, f, cu, cv, min_depth, limit, xc, r, &t);
}

// What the winner means for the frame, before the refinement: 3 no valid hypothesis, 4 too few inliers, 0 go on.
VSM_HD inline int32_t lc_verdict(bool any_valid, int32_t best_count, int32_t min_inliers) {
  if (!any_valid) return 3;
  if (best_count < min_inliers) return 4;
  return 0;
}
// ... and the frame's status from everything: asked, E, the verdict, the resection's status
VSM_HD inline int32_t lc_status(bool asked, int32_t eligible, int32_t min_inliers, int32_t verdict, int32_t resect_status) {
  if (!asked) return 1;
  if (eligible < min_inliers) return 2;
  if (verdict != 0) return verdict;
  if (resect_status == 0 || resect_status == 6) return resect_status;
  return 5;
}

// ---- host side (vsm_locate_host.cpp; no HIP) ----
bool lc_params_ok(const vsm_locate_params *params);
// the argument checks of vsm_locate_run / vsm_host_locate: the number of observations, or -1
int64_t lc_check_args(int32_t n_frames, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv, const double *xyz,
                      const vsm_locate_params *params);
// the refinement's parameters: the resection as a caller would ask for it
vsm_resect_params lc_resect_params(const vsm_locate_params &p);
// the eligible rows of a frame: their indices in the frame, ascending
void lc_eligible_rows(const RsRow *rows, int32_t n, const double *xyz, std::vector<int32_t> &elig);
// K hypotheses' samples from a fresh engine: picks[K][6], indices of rows in the frame (deck: work space)
void lc_sample(uint32_t seed, const int32_t *elig, int32_t E, int32_t K, int32_t *picks, std::vector<int32_t> &deck);

// ---- device path (vsm_locate.hip) ----
struct LcTile {
  int32_t job, off;
};
#ifdef __HIP__
struct VsmProf;
struct LcDevice {
  // uploaded
  const int32_t *row_off;    // [n_frames + 1]
  const RsRow *rows;         // by frame
  const double *xyz;         // [n_tracks][3]
  const int32_t *frame_job;  // [n_frames]: the frame's job, or -1
  const int32_t *job_frame;  // [n_jobs]
  const int32_t *job_E;      // [n_jobs]: the frame's eligible rows, 0 where it has fewer than min_inliers (no hypotheses then)
  const LcTile *tiles;       // [n_tiles]: 256 rows of a job with hypotheses
  const int32_t *picks;      // [n_jobs][K][6]
  // working set
  double *states;            // [n_jobs][K][12]
  uint8_t *hvalid;           // [n_jobs][K]
  int32_t *counts;           // [n_jobs][K], zeroed before the launches
  uint8_t *lin_valid;        // [n_frames]: the frame goes to the refinement
  // results, per frame
  int32_t *verdict, *best, *inliers;
  double *lin_poses;
  double f, cu, cv;
  vsm_locate_params prm;
  int32_t n_frames, n_jobs, n_tiles;
};
// fit, count and winner; the refinement is the resection's launch on lin_poses (vsm_locate.inc)
void vsm_locate_launch(hipStream_t s, VsmProf &pf, const LcDevice &d);
#endif
