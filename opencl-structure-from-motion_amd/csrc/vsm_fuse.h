// Fusion: duplicate tracks of one 3-D point joined (vsm_fuse.hip, vsm_fuse_host.cpp, vsm_fuse.inc).
// Every point in use is projected into every searched frame with a pose that does not observe it yet - the re-observation's
// candidates - and there the features that tracks in use own are searched for the track's descriptor: the complement of the
// re-observation's window.  The best feature's owner b is proposed as a duplicate of a; a cap, a ratio test, a frame that both
// tracks see, a's better proposal or b's other choice speak against it.  Two tracks that choose each other are fused: the
// smaller index survives and takes the other's observations.  include/visomatch.h has the contract; this header is the one
// statement of what is new in the arithmetic.  Projection, window test, cost, a window's best and second, the window's code
// and the index are the re-observation's (vsm_reobserve.h), included and not restated.  Every decision is a comparison of
// integers - costs, indices, frames - so the device's groups and atomics and the host view's one thread give the same bytes.
#pragma once
#include "vsm_reobserve.h"

enum { FU_PROP_INTS = 8 };
// a proposal's code, the first that applies; FU_EMPTY is counted only: a candidate with an empty window is no proposal
enum { FU_FUSED = 0, FU_EMPTY = 1, FU_COSTLY = 2, FU_AMBIGUOUS = 3, FU_CONFLICT = 4, FU_OUTBID = 5, FU_ONE_SIDED = 6, FU_CODES = 7 };
enum { FU_STAT_FUSIONS = RO_REASONS + FU_CODES, FU_STATS = FU_STAT_FUSIONS + 1 };
#define FU_NO_OWNER 0xffffffffu  // a feature no track in use observes
// The compacting form keeps 48 bytes per pair of a track in use and a searched frame with a pose on the device; a call that
// would need more than this searches twice instead (handle option fuse_compact; profiles/README.md).
#define FU_PLACES_MAX ((size_t)2 << 30)

VSM_HD inline vsm_reobserve_params fu_as_reobserve(const vsm_fuse_params &p) {
  vsm_reobserve_params r;
  r.radius = p.radius;
  r.min_depth = p.min_depth;
  r.max_cost = p.max_cost;
  r.ratio_num = p.ratio_num;
  r.ratio_den = p.ratio_den;
  return r;
}
VSM_HD inline bool fu_params_ok(const vsm_fuse_params *p) {
  if (!p) return false;
  const vsm_reobserve_params r = fu_as_reobserve(*p);
  return ro_params_ok(&r);
}

// Does a frame of fa[start], fa[start + step], ... occur among the nb frames at fb?  The host asks with (0, 1), a lane of a
// group with (lane, RO_LANES); the group's answer is the OR of its lanes'.
VSM_HD inline bool fu_conflict(const int32_t *fa, int32_t na, const int32_t *fb, int32_t nb, int32_t start, int32_t step) {
  for (int32_t i = start; i < na; i += step)
    if (ro_observed(fb, nb, fa[i])) return true;
  return false;
}

// a track's bid for its partner: the smallest wins.  cost < 2^31 and the proposal's index < 2^31, so no key is FU_NO_CHOICE
#define FU_NO_CHOICE 0xffffffffffffffffull
VSM_HD inline uint64_t fu_bid(int32_t cost, int32_t proposal) { return ro_key(cost, proposal); }

// The verdict of a proposal p = {a, ., ., ., ., ., code, b} that came through the window's tests and the conflict test, given
// every track's smallest bid (choice) and the proposals' records: FU_OUTBID, FU_ONE_SIDED or FU_FUSED.  It reads word 7
// of another proposal and the bids, which no verdict changes.
VSM_HD inline int32_t fu_verdict(const int32_t *prop, const unsigned long long *choice, int32_t p) {
  const int32_t a = prop[FU_PROP_INTS * (size_t)p], b = prop[FU_PROP_INTS * (size_t)p + 7];
  if ((uint32_t)choice[a] != (uint32_t)p) return FU_OUTBID;
  const unsigned long long cb = choice[b];
  if (cb == FU_NO_CHOICE || prop[FU_PROP_INTS * (size_t)(uint32_t)cb + 7] != a) return FU_ONE_SIDED;
  return FU_FUSED;
}

// ---- the merged track set ----
// Track t after the fusions: absorbed (fused_into[t] >= 0), survivor (its partner is absorbed into it) or as it was.
VSM_HD inline bool fu_survivor(const int32_t *partner, const int32_t *fused_into, int32_t t) { return partner[t] > t && fused_into[partner[t]] == t; }
VSM_HD inline int32_t fu_length_after(const int32_t *offsets, const int32_t *partner, const int32_t *fused_into, int32_t t) {
  if (fused_into[t] >= 0) return 0;
  const int32_t n = offsets[t + 1] - offsets[t];
  return fu_survivor(partner, fused_into, t) ? n + offsets[partner[t] + 1] - offsets[partner[t]] : n;
}
// A survivor's observations are its own na, then the absorbed track's nb, stably sorted by frame: the place of element i of
// that list of na + nb is the number of elements with a smaller frame plus the number of earlier elements with its frame.
VSM_HD inline int32_t fu_list_frame(const int32_t *fa, int32_t na, const int32_t *fb, int32_t i) { return i < na ? fa[i] : fb[i - na]; }
VSM_HD inline int32_t fu_rank(const int32_t *fa, int32_t na, const int32_t *fb, int32_t nb, int32_t i) {
  const int32_t fi = fu_list_frame(fa, na, fb, i);
  int32_t r = 0;
  for (int32_t j = 0; j < na + nb; j++) {
    const int32_t fj = fu_list_frame(fa, na, fb, j);
    r += (fj < fi || (fj == fi && j < i)) ? 1 : 0;
  }
  return r;
}

// ---- device path (vsm_fuse.hip) ----
#ifdef __HIP__
struct VsmProf;
struct FuDevice {
  // uploaded: as RoDevice
  const double *states;
  const uint8_t *valid, *search;
  const int32_t *offsets, *obs_frames, *obs_feat;
  const double *xyz;
  const uint8_t *use;
  const int32_t *ref_obs;
  const int32_t *feat_offsets;
  const int32_t *const *frame_feat;
  const int32_t *use_rank;        // per track: the tracks in use in front of it
  // the compacting form (null: the search runs twice): per track in use slot_stride places for its proposals
  int32_t *slots;                 // [tracks in use][slot_stride][8]
  double *slots_uv;               // [tracks in use][slot_stride][2]
  int32_t slot_stride;            // the frames searched with a pose: no track has more candidates
  // working set
  uint32_t *owner;                // per feature: the smallest track in use that observes it, or FU_NO_OWNER
  int32_t *bins;                  // int2 per bin: (start, count) once the index stands
  int32_t *bins_part, *bins_total;
  int32_t *sorted;                // [n_feat][12]: the owned features' records in bin order, the feature's index in word 2
  int32_t *scan, *scan_part;      // int2 per track: (proposals, 0) -> exclusive prefix; later (length after, 0) -> offsets_after
  unsigned long long *choice;     // per track: its smallest bid
  // results
  int32_t *totals;                // int2 (proposals, 0); later (observations, 0)
  int32_t *partner, *fused_into;  // per track
  int32_t *offsets_after;         // [n_tracks + 1]
  int32_t *obs_src;               // [n_obs]
  int32_t *frame_counts;          // per frame {candidates, proposals}
  unsigned long long *stats;      // [FU_STATS]
  int32_t *prop;                  // [n_prop][8]
  double *prop_uv;                // [n_prop][2]
  double f, cu, cv;
  vsm_reobserve_params prm;
  RoGrid grid;
  int32_t n_frames, n_tracks, n_obs, n_feat, width, height;
};
// owners, the index of the owned features, the proposals' counts per track and their scan: everything up to the total
void vsm_fuse_launch_count(hipStream_t s, VsmProf &pf, const FuDevice &d);
// the proposals' list for the n_prop the host has read back, conflicts, bids, verdicts, the merged set
void vsm_fuse_launch_fuse(hipStream_t s, VsmProf &pf, const FuDevice &d, int32_t n_prop);
#endif
