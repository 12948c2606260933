// Vetting of observations by reprojection error (vsm_vet.hip, vsm_vet_host.cpp, vsm_vet.inc): the
// step between rounds of adjustment - every observation's residual at the given poses and points, a verdict per
// observation, per track and per frame, and the track set with the outliers taken out.  include/visomatch.h has the
// contract; this header is the one statement of the arithmetic.  The row test is the resection's own (rs_row, rs_limit of
// vsm_resect.h) at the state the resection starts from (pts_rigid_inverse of vsm_points.h), so an inlier here is exactly a
// row the resection uses at the input pose.  The kernel (a 16-lane group per track) and the host view (one thread) both
// call the functions below and differ only in who calls them.  Everything is double, every operation one of + - * /;
// build with -ffp-contract=off.
//
// The one ordered sum is a track's ss, the sum of t = ru^2 + rv^2 over its inliers: partial[l], l = 0 .. 15, adds the
// inliers whose position in the track is l mod 16, ascending, from +0.0 (a non-inlier is passed over, not added as zero);
// then partial[l] += partial[l + s] for l < s, s = 8, 4, 2, 1.  The count, the two frame bounds and the largest t are
// order-free (an inlier's t is finite: it passed t < limit), so a VetAcc merges with another in any order but for ss.
#pragma once
#include <math.h>
#include <stdint.h>

#include "visomatch.h"
#include "vsm_points.h"
#include "vsm_resect.h"

enum { VET_LANES = 16 };
enum { VET_INLIER = 0, VET_UNUSED = 1, VET_NO_POSE = 2, VET_BEHIND = 3, VET_GATED = 4, VET_CODES = 5, VET_STATUSES = 4 };
#define VET_NO_FRAME 0x7fffffff  // frame_lo of an accumulator without an inlier

VSM_HD inline bool vet_params_ok(const vsm_vet_params *p) {
  return p && p->min_observations >= 1 && p->max_residual >= 0 && p->min_depth == p->min_depth;
}

// One observation: its code, and in *t the double ru^2 + rv^2 (codes 0 and 4; untouched otherwise).  S: the frame's state
// [Rw | tw]; X: the track's point.
template <class M>
VSM_HD inline int32_t vet_obs(M S, const double *X, float u, float v, int in_use, int valid, double f, double cu, double cv, double min_depth, double limit,
                              double *t) {
  if (!in_use) return VET_UNUSED;
  if (!valid) return VET_NO_POSE;
  double xc[3], r[2], tt;
  if (rs_row(S, X, u, v, f, cu, cv, min_depth, limit, xc, r, &tt)) {
    *t = tt;
    return VET_INLIER;
  }
  if (!(xc[2] > min_depth)) return VET_BEHIND;  // (rs_row's first test: nothing behind it has been computed)
  *t = tt;
  return VET_GATED;
}
// r2 of an observation: the float of t where there is one
VSM_HD inline float vet_r2(int32_t code, double t) { return (code == VET_INLIER || code == VET_GATED) ? (float)t : 0.0f; }

// what a lane (a partial sum) knows of its track's inliers
struct VetAcc {
  double ss, worst;
  int32_t n_in, lo, hi;
};
VSM_HD inline void vet_acc_init(VetAcc *a) {
  a->ss = 0.0;
  a->worst = 0.0;
  a->n_in = 0;
  a->lo = VET_NO_FRAME;
  a->hi = -1;
}
VSM_HD inline void vet_acc_add(VetAcc *a, int32_t frame, double t) {
  a->ss += t;
  a->worst = t > a->worst ? t : a->worst;
  a->n_in++;
  a->lo = frame < a->lo ? frame : a->lo;
  a->hi = frame > a->hi ? frame : a->hi;
}
// a step of the tree: a = partial[l], the other five numbers partial[l + s]
VSM_HD inline void vet_acc_merge(VetAcc *a, double ss, double worst, int32_t n_in, int32_t lo, int32_t hi) {
  a->ss += ss;
  a->worst = worst > a->worst ? worst : a->worst;
  a->n_in += n_in;
  a->lo = lo < a->lo ? lo : a->lo;
  a->hi = hi > a->hi ? hi : a->hi;
}
VSM_HD inline int32_t vet_frame_lo(const VetAcc &a) { return a.n_in > 0 ? a.lo : -1; }
VSM_HD inline int32_t vet_track_status(int in_use, const VetAcc &a, int32_t min_observations) {
  if (!in_use) return 1;
  if (a.n_in < min_observations) return 2;
  if (a.lo == a.hi) return 3;
  return 0;
}
// the track's length in the pruned set
VSM_HD inline int32_t vet_kept_length(int32_t status, int32_t n_in) { return status == 0 ? n_in : 0; }

// ---- device path (vsm_vet.hip) ----
#ifdef __HIP__
struct VsmProf;
struct VetDevice {
  // uploaded
  const double *states;       // [n_frames][12]: [Rw | tw]
  const uint8_t *valid;       // per frame
  const int32_t *offsets;     // [n_tracks + 1]
  const int32_t *obs_frames;  // per observation
  const float *uv;            // per observation, (u, v)
  const double *xyz;          // [n_tracks][3]
  const uint8_t *use;         // per track
  // results per observation
  uint8_t *code;
  float *r2;
  // results per track
  int32_t *status, *n_in, *frame_lo, *frame_hi;
  double *ss, *worst;
  // results per frame: {inliers, behind, gated}, zero before the launch
  int32_t *frame_counts;
  // the pruned set
  int32_t *kept_offsets;  // [n_tracks + 1]
  int32_t *kept_index;    // [n_obs] at most
  // working set: the scan of vsm_tracks.hip over (kept track, kept length) per track
  int32_t *scan, *scan_part, *totals;
  double f, cu, cv;
  vsm_vet_params prm;
  int32_t n_tracks;
};
void vsm_vet_launch(hipStream_t s, VsmProf &pf, const VetDevice &d);
#endif
