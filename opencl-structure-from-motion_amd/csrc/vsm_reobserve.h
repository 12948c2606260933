// Re-observation: new observations of the points, found by projection (vsm_reobserve.hip,
// vsm_reobserve_host.cpp, vsm_reobserve.inc).  Every point in use is projected into every searched frame with a pose that
// does not observe it yet; among that frame's free features of the track's class near the projection, the one whose
// descriptor is nearest the track's reference feature becomes a new observation, unless a cap, a ratio test or another
// track's better claim speaks against it.  include/visomatch.h has the contract; this header is the one statement of the
// arithmetic.  The geometry is the resection's row (pts_rigid_inverse and pts_affine_row of vsm_points.h, the prediction
// f x / z + c of rs_row) in double, every operation one of + - * /; build with -ffp-contract=off.  The cost is the
// matcher's: the sum of absolute differences of the 32 descriptor bytes, an integer.  Nothing here is summed in an order
// that matters: a window's best, second and size merge in any order (RoBest), a contested feature goes to the smallest
// (cost, candidate) - so the device's groups and atomics and the host view's one thread give the same bytes.
//
// The index (bins of 2^shift pixels per class and frame, a counting sort of the free features) only narrows the features a
// window looks at; ro_in_window is the test, and ro_bin_span takes a pixel more on every side than the window needs, so
// no rounding of pu - radius can lose a feature.
#pragma once
#include <math.h>
#include <stdint.h>

#include "visomatch.h"
#include "vsm_points.h"

enum { RO_LANES = 16, RO_FEAT_INTS = 12, RO_CAND_INTS = 7 };
enum { RO_ACCEPTED = 0, RO_EMPTY = 1, RO_COSTLY = 2, RO_AMBIGUOUS = 3, RO_LOST = 4, RO_CODES = 5 };
// why a pair (track in use, frame) is no candidate, in the order of the tests; RO_CANDIDATE: it is one
enum { RO_NOT_SEARCHED = 0, RO_NO_POSE = 1, RO_OBSERVED = 2, RO_BEHIND = 3, RO_OUTSIDE = 4, RO_REASONS = 5, RO_CANDIDATE = 5 };
enum { RO_STATS = RO_REASONS + RO_CODES };
enum { RO_MAX_DIM = 16383, RO_MAX_BINS = 16384, RO_MIN_SHIFT = 3 };
#define RO_NONE 0x7fffffff             // second of a window with fewer than two features
#define RO_NO_KEY 0xffffffffffffffffull  // best of an empty window; a feature nobody claims

VSM_HD inline bool ro_finite(double x) { return x > -HUGE_VAL && x < HUGE_VAL; }
VSM_HD inline bool ro_params_ok(const vsm_reobserve_params *p) {
  return p && ro_finite(p->radius) && p->radius >= 0 && p->min_depth == p->min_depth && p->max_cost >= 0 && p->ratio_num >= 0 && p->ratio_den >= 0 &&
         !(p->ratio_den > 0 && p->ratio_num <= 0);
}
VSM_HD inline bool ro_dims_ok(int32_t width, int32_t height) { return width >= 1 && width <= RO_MAX_DIM && height >= 1 && height <= RO_MAX_DIM; }

// the reference observation of a track of n > 0 observations where the caller names none
VSM_HD inline int32_t ro_middle(int32_t n) { return (n - 1) / 2; }

// The projection of X by the state S = [Rw | tw]: RO_BEHIND, RO_OUTSIDE or RO_CANDIDATE with (pu, pv).  NaN fails the
// comparison it reaches.
template <class M>
VSM_HD inline int32_t ro_project(M S, const double *X, double f, double cu, double cv, double min_depth, int32_t width, int32_t height, double *pu, double *pv) {
  const double xc = pts_affine_row(S, 0, X[0], X[1], X[2]);
  const double yc = pts_affine_row(S, 1, X[0], X[1], X[2]);
  const double zc = pts_affine_row(S, 2, X[0], X[1], X[2]);
  if (!(zc > min_depth)) return RO_BEHIND;
  const double u = f * xc / zc + cu, v = f * yc / zc + cv;
  if (!(u >= 0.0 && u <= (double)(width - 1) && v >= 0.0 && v <= (double)(height - 1))) return RO_OUTSIDE;
  *pu = u;
  *pv = v;
  return RO_CANDIDATE;
}
// is frame g one of the n frames at fr
VSM_HD inline bool ro_observed(const int32_t *fr, int32_t n, int32_t g) {
  for (int32_t i = 0; i < n; i++)
    if (fr[i] == g) return true;
  return false;
}
// A pair (track in use, frame g): the first reason that applies, or RO_CANDIDATE.
template <class M>
VSM_HD inline int32_t ro_pair(int searched, int valid, const int32_t *fr, int32_t n, int32_t g, M S, const double *X, double f, double cu, double cv,
                              double min_depth, int32_t width, int32_t height, double *pu, double *pv) {
  if (!searched) return RO_NOT_SEARCHED;
  if (!valid) return RO_NO_POSE;
  if (ro_observed(fr, n, g)) return RO_OBSERVED;
  return ro_project(S, X, f, cu, cv, min_depth, width, height, pu, pv);
}

VSM_HD inline bool ro_in_window(int32_t u, int32_t v, double pu, double pv, double radius) {
  const double du = (double)u, dv = (double)v;
  return du - pu <= radius && pu - du <= radius && dv - pv <= radius && pv - dv <= radius;
}

// the cost: a, b are the records' eight descriptor words
VSM_HD inline int32_t ro_sad(const uint32_t *a, const uint32_t *b) {
#ifdef __HIP_DEVICE_COMPILE__
  uint32_t s = 0;
  for (int i = 0; i < 8; i++) s = __builtin_amdgcn_sad_u8(a[i], b[i], s);
  return (int32_t)s;
#else
  int32_t s = 0;
  for (int i = 0; i < 8; i++)
    for (int k = 0; k < 32; k += 8) {
      const int32_t x = (int32_t)((a[i] >> k) & 255u), y = (int32_t)((b[i] >> k) & 255u);
      s += x > y ? x - y : y - x;
    }
  return s;
#endif
}

// What a lane (or the host's loop) knows of a window: key = cost << 32 | feature of the best, the smallest cost among the
// others, the size.  ro_best_merge is commutative and associative.
struct RoBest {
  uint64_t key;
  int32_t second, n;
};
VSM_HD inline void ro_best_init(RoBest *a) {
  a->key = RO_NO_KEY;
  a->second = RO_NONE;
  a->n = 0;
}
VSM_HD inline uint64_t ro_key(int32_t cost, int32_t k) { return ((uint64_t)(uint32_t)cost << 32) | (uint32_t)k; }
VSM_HD inline void ro_best_merge(RoBest *a, uint64_t key, int32_t second, int32_t n) {
  uint64_t loser = key;
  if (key < a->key) {
    loser = a->key;
    a->key = key;
  }
  const int32_t lc = loser == RO_NO_KEY ? RO_NONE : (int32_t)(loser >> 32);
  const int32_t s = second < a->second ? second : a->second;
  a->second = lc < s ? lc : s;
  a->n += n;
}
VSM_HD inline void ro_best_add(RoBest *a, int32_t cost, int32_t k) { ro_best_merge(a, ro_key(cost, k), RO_NONE, 1); }
// The code a window earns by itself: RO_EMPTY, RO_COSTLY, RO_AMBIGUOUS, or RO_ACCEPTED for one that goes on to claim its best.
VSM_HD inline int32_t ro_window_code(const RoBest &b, const vsm_reobserve_params &p) {
  if (b.n == 0) return RO_EMPTY;
  const int32_t best = (int32_t)(b.key >> 32);
  if (p.max_cost > 0 && best > p.max_cost) return RO_COSTLY;
  if (p.ratio_den > 0 && b.second != RO_NONE && !((int64_t)best * p.ratio_den < (int64_t)b.second * p.ratio_num)) return RO_AMBIGUOUS;
  return RO_ACCEPTED;
}
// a candidate's record before the verdict: {track, frame, feature, cost, second, n_window, code}
VSM_HD inline void ro_record(int32_t *r, const RoBest &b, int32_t code) {
  r[2] = b.n > 0 ? (int32_t)(uint32_t)b.key : -1;
  r[3] = b.n > 0 ? (int32_t)(b.key >> 32) : -1;
  r[4] = b.second == RO_NONE ? -1 : b.second;
  r[5] = b.n;
  r[6] = code;
}

// ---- the index: bins of 2^shift pixels, per frame 4 classes of nbv rows of nbu bins ----
struct RoGrid {
  int32_t shift, nbu, nbv;
};
VSM_HD inline int32_t ro_frame_bins(const RoGrid &g) { return 4 * g.nbu * g.nbv; }
// the smallest shift from RO_MIN_SHIFT up that keeps a frame within RO_MAX_BINS bins
inline RoGrid ro_grid(int32_t width, int32_t height) {
  RoGrid g;
  for (g.shift = RO_MIN_SHIFT;; g.shift++) {
    g.nbu = ((width - 1) >> g.shift) + 1;
    g.nbv = ((height - 1) >> g.shift) + 1;
    if (ro_frame_bins(g) <= RO_MAX_BINS) return g;
  }
}
VSM_HD inline int32_t ro_clamp(int32_t x, int32_t hi) { return x < 0 ? 0 : (x > hi ? hi : x); }
// the bin of a feature within its frame's bins (a record out of range lands in an edge bin: no index leaves the table)
VSM_HD inline int32_t ro_bin(const RoGrid &g, int32_t cls, int32_t u, int32_t v) {
  return ((cls & 3) * g.nbv + ro_clamp(v >> g.shift, g.nbv - 1)) * g.nbu + ro_clamp(u >> g.shift, g.nbu - 1);
}
// the bins [lo, hi] along one axis that hold every pixel within radius of p, and a pixel more on either side (0 <= p <= last)
VSM_HD inline void ro_bin_span(double p, double radius, int32_t last, int32_t shift, int32_t *lo, int32_t *hi) {
  const double a = p - radius - 1.0, b = p + radius + 1.0;
  *lo = (a > 0.0 ? (int32_t)a : 0) >> shift;
  *hi = (b < (double)last ? (int32_t)b : last) >> shift;
}

// ---- host side (vsm_reobserve_host.cpp; no HIP) ----
// The argument checks of both forms but for the feature records: the number of observations, or -1.  feat_count(g): the
// features of frame g.
int64_t ro_check_tracks(const vsm_reobserve_params *params, int32_t n_frames, const double *poses, int32_t width, int32_t height, int32_t n_tracks,
                        const int32_t *offsets, const int32_t *obs_frames, const int32_t *obs_feat, const double *xyz, const int32_t *ref_obs,
                        const int32_t *feat_offsets);
// feat_offsets[F + 1] and the records: the number of features, or -1
int64_t ro_check_features(int32_t n_frames, int32_t width, int32_t height, const int32_t *feat_offsets, const int32_t *feat);
// the candidates a call can have at the most: tracks in use with an observation times frames searched with a pose
int64_t ro_candidate_bound(int32_t n_frames, const uint8_t *pose_valid, const uint8_t *search, int32_t n_tracks, const int32_t *offsets, const uint8_t *use);

// ---- device path (vsm_reobserve.hip) ----
#ifdef __HIP__
struct VsmProf;
struct RoDevice {
  // uploaded
  const double *states;       // [n_frames][12]: [Rw | tw]
  const uint8_t *valid, *search;  // per frame
  const int32_t *offsets;     // [n_tracks + 1]
  const int32_t *obs_frames, *obs_feat;  // per observation
  const double *xyz;          // [n_tracks][3]
  const uint8_t *use;         // per track: in use and with an observation
  const int32_t *ref_obs;     // per track, resolved
  const int32_t *feat_offsets;           // [n_frames + 1]
  const int32_t *const *frame_feat;      // per frame: its records, in the uploaded block or resident in a pairs context
  // working set
  uint8_t *occupied;              // per feature
  unsigned long long *claim;      // per feature: the smallest cost << 32 | candidate
  int32_t *bins;                  // int2 per bin: (start, count) once the index stands
  int32_t *bins_part, *bins_total;
  int32_t *sorted;                // [n_feat][12]: the free features' records in bin order, the feature's index in word 2
  int32_t *scan, *scan_part;      // int2 per track: (candidates, 0) -> exclusive prefix
  // results
  int32_t *totals;                // int2 (candidates, 0)
  int32_t *track_accepted;        // per track
  int32_t *frame_counts;          // per frame {candidates, accepted}
  unsigned long long *stats;      // [RO_STATS]
  int32_t *cand;                  // [n_cand][7]
  double *cand_uv;                // [n_cand][2]
  double f, cu, cv;
  vsm_reobserve_params prm;
  RoGrid grid;
  int32_t n_frames, n_tracks, n_obs, n_feat, width, height;
};
// occupied features, the index, the candidates' counts per track and their scan: everything up to the totals
void vsm_reobserve_launch_count(hipStream_t s, VsmProf &pf, const RoDevice &d);
// the candidate list, the search, the verdicts, for the n_cand the host has read back
void vsm_reobserve_launch_search(hipStream_t s, VsmProf &pf, const RoDevice &d, int32_t n_cand);
#endif
