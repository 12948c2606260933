// Multi-view feature tracks from pair match lists (vsm_tracks.hip, vsm_tracks_host.cpp, vsm_tracks.inc).
//
// Nodes are (frame, feature index), numbered feat_base[frame] + feature; match m of pair k = (a, b) is edge
// pair_base[k] + m between (a, ip) and (b, ic).  A track is a connected component.  This header holds what the device
// kernels, the host view and a stand-alone host program share: the union-find steps, written once for both sides, the
// packing of a match list, and the launch interface of the device path.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "visomatch.h"

#ifdef __HIP__
#define TRK_HD __host__ __device__
#else
#define TRK_HD
#endif

#define TRK_UNUSED 0x7fffffff             // first[] of a node no match names
#define TRK_MAX_NODES 0x7ffffffe          // node ids and 2 * edge + end are 31-bit
#define TRK_MAX_EDGES 0x3fffffff
#define TRK_SCAN_BLOCK 256                // items one workgroup scans: the scan has ceil(log256(nodes)) levels

// ---- the union-find steps.  Invariant: parent[x] <= x, and parent[x] only ever decreases.  So every loop below ends, a
// stale value of parent[x] is still an ancestor of x, and the root a component ends with is its smallest node whatever the
// order of the unions.  On the device the accesses are relaxed agent-scope atomics (they go to L2: the vector L1 of a CU is
// not refreshed by other CUs' stores); on the host the same builtins, so that threads can drive the functions too. ----
TRK_HD inline int32_t trk_load(int32_t *p) {
#ifdef __HIP_DEVICE_COMPILE__
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}
TRK_HD inline void trk_lower(int32_t *p, int32_t v) {  // *p = min(*p, v)
#ifdef __HIP_DEVICE_COMPILE__
  (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  int32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v < old && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }
#endif
}
TRK_HD inline int32_t trk_cas(int32_t *p, int32_t expected, int32_t v) {  // returns what *p held
#ifdef __HIP_DEVICE_COMPILE__
  (void)__hip_atomic_compare_exchange_strong(p, &expected, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  (void)__atomic_compare_exchange_n(p, &expected, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
#endif
  return expected;
}
// the root above x, with path halving: x strictly decreases from hop to hop
TRK_HD inline int32_t trk_find(int32_t *parent, int32_t x) {
  for (;;) {
    const int32_t p = trk_load(parent + x);
    if (p == x) return x;
    const int32_t g = trk_load(parent + p);
    if (g != p) trk_lower(parent + x, g);
    x = g;
  }
}
// lock-free union: the larger root is hooked below the smaller node; a lost race goes on from what the winner wrote
TRK_HD inline void trk_unite(int32_t *parent, int32_t u, int32_t v) {
  for (;;) {
    u = trk_find(parent, u);
    v = trk_find(parent, v);
    if (u == v) return;
    if (u < v) {
      const int32_t t = u;
      u = v;
      v = t;
    }
    const int32_t old = trk_cas(parent + u, u, v);
    if (old == u) return;
    u = old;  // (smaller than before: u + v decreases with every turn)
  }
}

// largest k in [0, n) with base[k] <= e, for a non-decreasing base[0 .. n] with base[0] <= e < base[n]
TRK_HD inline int32_t trk_owner(const int32_t *base, int32_t n, int32_t e) {
  int32_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const int32_t mid = (lo + hi + 1) >> 1;
    if (base[mid] <= e)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// the int2 items the levels above level 0 of a scan over n items need
inline size_t trk_scan_part_items(int64_t n) {
  size_t items = 0;
  while (n > TRK_SCAN_BLOCK) {
    n = (n + TRK_SCAN_BLOCK - 1) / TRK_SCAN_BLOCK;
    items += (size_t)n;
  }
  return items;
}

// ---- host side (vsm_tracks_host.cpp; no HIP) ----
// the argument checks that need no list: returns the number of edges, or -1
int64_t trk_check_args(int32_t n_frames, const int32_t *pairs, int32_t n_pairs, const vsm_p_match *const *lists, const int32_t *counts, int32_t side,
                       int32_t min_length);
// one list's (ip, ic) of the chosen side into edges[2 * n]; the largest of each; false at a negative index
bool trk_pack_list(const vsm_p_match *list, int32_t n, int32_t side, int32_t *edges, int32_t *max_p, int32_t *max_c);
// feat_base[n_frames + 1] and pair_base[n_pairs + 1] from the lists' maxima; false if the nodes do not fit 31 bits
bool trk_bases(int32_t n_frames, const int32_t *pairs, int32_t n_pairs, const int32_t *counts, const int32_t *max_p, const int32_t *max_c, int32_t *feat_base,
               int32_t *pair_base);
// rows [4] of one segment into ascending (frame, feature) order; returns 1 if two rows share a frame
int trk_sort_segment(int32_t *rows, int32_t n);

// ---- device path (vsm_tracks.hip) ----
#ifdef __HIP__
struct VsmProf;
struct TrkDevice {
  // uploaded
  const int32_t *pair_base, *pairs, *feat_base, *edges;
  // working set, per node
  int32_t *parent, *first, *size, *cursor;
  int32_t *scan;       // int2 per node: (kept root, its size) -> exclusive prefix (track number, offset)
  int32_t *scan_part;  // the partial sums of every level above, one after the other
  int32_t *totals;     // int2 (tracks, observations)
  int32_t *mid_list;   // tracks a workgroup orders
  // results
  int32_t *counters;   // [4]: {segments a workgroup ordered, 0, 0, 0}
  int32_t *offsets, *obs, *track_of_match;
  uint8_t *flags;
  int32_t n_nodes, n_edges, n_pairs, n_frames, min_length;
};
// init, hook, flatten + sizes, kept roots, the scan: everything up to the totals (2 words, device memory)
void vsm_tracks_launch_link(hipStream_t s, VsmProf &pf, const TrkDevice &d);
// The scan alone, for a further stage (vsm_vet.hip): the exclusive prefix of n_items int2 items in place, their sum into
// totals (2 words); scan_part holds the partial sums of every level above (trk_scan_part_items int2 items).
void vsm_tracks_launch_scan(hipStream_t s, VsmProf &pf, int32_t *scan, int32_t n_items, int32_t *scan_part, int32_t *totals);
// track of every match, observations, their order and the flags, for the totals the host has read back
void vsm_tracks_launch_emit(hipStream_t s, VsmProf &pf, const TrkDevice &d, int32_t n_tracks, int32_t n_obs);
#endif
