// Re-observation on the device (vsm_reobserve.h has the arithmetic, vsm_reobserve.inc the host side).
//
// k_ro_occupy: a lane per observation marks the feature it names.  k_ro_bin_count / k_ro_scatter: a lane per feature; the
// free features are counted per (frame, class, bin), the tracks' multi-level scan turns the counts into starts, and each
// feature's record goes to its bin's next place with its index in word 2 - the order inside a bin is whatever the atomics
// give, and nothing below depends on it.
// k_ro_project<false>: a 16-lane group per track, sixteen groups per 256-thread workgroup, the workgroups striding the
// tracks; the group walks the frames 16 at a time, counts the candidates and the reasons, and hands the track's count to the scan.
// k_ro_project<true>, behind the host's wait for the total: the same walk, a candidate's place being the track's prefix
// plus its rank among the group's lanes (a ballot), so the list is in (track, frame) order.
// k_ro_search, the hot kernel: a 16-lane group per candidate.  The bins a window touches are, row by row, one contiguous
// run of sorted records; the lanes stride the run, a lane reads a record as three 16-byte loads (head, two descriptor halves)
// and costs it with v_sad_u8 as k_match does.  Best, second and size are merged across the group by cross-lane moves of
// width 16 (no LDS, no barrier); lane 0 writes the record and claims the feature with a 64-bit atomicMin of cost << 32 |
// candidate.  k_ro_verdict: a lane per candidate reads the claim back: its own key keeps the feature, another's means lost.
// All control flow is uniform inside a group; the groups of a wave differ in their trip counts only.
#include "vsm_internal.h"
#include "vsm_reobserve.h"
#include "vsm_tracks.h"

namespace {

__device__ inline uint32_t ro_group_ballot(bool pred) {
  const unsigned long long all = __ballot(pred);
  return (uint32_t)(all >> (threadIdx.x & 48)) & 0xffffu;
}
__device__ inline int64_t ro_gid() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ inline int64_t ro_gsize() { return (int64_t)gridDim.x * blockDim.x; }

__global__ __launch_bounds__(256) void k_ro_occupy(RoDevice d) {
  for (int64_t i = ro_gid(); i < d.n_obs; i += ro_gsize()) d.occupied[(size_t)d.feat_offsets[d.obs_frames[i]] + d.obs_feat[i]] = 1;
}

// a feature's frame, index and bin; false for an occupied one
__device__ inline bool ro_free_feature(const RoDevice &d, int32_t j, const int32_t **rec, int32_t *k, size_t *bin) {
  if (d.occupied[j]) return false;
  const int32_t g = trk_owner(d.feat_offsets, d.n_frames, j);
  *k = j - d.feat_offsets[g];
  *rec = d.frame_feat[g] + RO_FEAT_INTS * (size_t)*k;
  const int4 head = *(const int4 *)*rec;  // {u, v, 0, class}
  *bin = (size_t)g * ro_frame_bins(d.grid) + ro_bin(d.grid, head.w, head.x, head.y);
  return true;
}
__global__ __launch_bounds__(256) void k_ro_bin_count(RoDevice d) {
  for (int64_t j = ro_gid(); j < d.n_feat; j += ro_gsize()) {
    const int32_t *rec;
    int32_t k;
    size_t bin;
    if (ro_free_feature(d, (int32_t)j, &rec, &k, &bin)) atomicAdd(d.bins + 2 * bin, 1);
  }
}
// (the scan has left every bin's second word at zero: the sum of zeros - it is the bin's cursor, and its count at the end)
__global__ __launch_bounds__(256) void k_ro_scatter(RoDevice d) {
  for (int64_t j = ro_gid(); j < d.n_feat; j += ro_gsize()) {
    const int32_t *rec;
    int32_t k;
    size_t bin;
    if (!ro_free_feature(d, (int32_t)j, &rec, &k, &bin)) continue;
    const int32_t at = d.bins[2 * bin] + atomicAdd(d.bins + 2 * bin + 1, 1);
    int4 head = ((const int4 *)rec)[0];
    head.z = k;
    int4 *out = (int4 *)d.sorted + 3 * (size_t)at;
    out[0] = head;
    out[1] = ((const int4 *)rec)[1];
    out[2] = ((const int4 *)rec)[2];
  }
}

// Workgroups stride the tracks.  The counting pass keeps its frames' candidate counts (up to RO_LDS_FRAMES frames) and the
// reasons in LDS and hands them on with one atomic per workgroup and non-zero entry: a global atomic per candidate onto a
// few hundred addresses was the slowest part of the call.
enum { RO_LDS_FRAMES = 4096 };
template <bool WRITE>
__global__ __launch_bounds__(256) void k_ro_project(RoDevice d) {
  __shared__ int32_t s_frames[WRITE ? 1 : RO_LDS_FRAMES];
  __shared__ unsigned long long s_why[RO_REASONS];
  const int grp = threadIdx.x >> 4, ln = threadIdx.x & 15;
  const bool in_lds = !WRITE && d.n_frames <= RO_LDS_FRAMES;
  if (!WRITE) {
    if (in_lds)
      for (int32_t g = threadIdx.x; g < d.n_frames; g += 256) s_frames[g] = 0;
    if (threadIdx.x < RO_REASONS) s_why[threadIdx.x] = 0;
    __syncthreads();
  }
  for (int64_t t = (int64_t)blockIdx.x * 16 + grp; t < d.n_tracks; t += (int64_t)gridDim.x * 16) {  // (a group's lanes share t)
    if (!d.use[t]) {
      if (!WRITE && ln == 0) ((int2 *)d.scan)[t] = make_int2(0, 0);
      continue;
    }
    const int32_t o = d.offsets[t], n = d.offsets[t + 1] - o;
    const double X[3] = {d.xyz[3 * t + 0], d.xyz[3 * t + 1], d.xyz[3 * t + 2]};
    int32_t at = WRITE ? d.scan[2 * t] : 0;  // the candidates in front of this track; then those of the frames walked
    int32_t why[RO_REASONS] = {0, 0, 0, 0, 0};
    for (int32_t g0 = 0; g0 < d.n_frames; g0 += RO_LANES) {
      const int32_t g = g0 + ln;
      double pu = 0.0, pv = 0.0;
      int32_t kind = -1;
      if (g < d.n_frames)
        kind = ro_pair(d.search[g], d.valid[g], d.obs_frames + o, n, g, d.states + 12 * (size_t)g, X, d.f, d.cu, d.cv, d.prm.min_depth, d.width, d.height, &pu, &pv);
      const bool is_cand = kind == RO_CANDIDATE;
      const uint32_t m = ro_group_ballot(is_cand);
      if (WRITE) {
        if (is_cand) {
          const size_t c = (size_t)at + __popc(m & ((1u << ln) - 1u));
          int32_t *r = d.cand + RO_CAND_INTS * c;
          r[0] = (int32_t)t;
          r[1] = g;
          d.cand_uv[2 * c] = pu;
          d.cand_uv[2 * c + 1] = pv;
        }
      } else {
        if (is_cand) atomicAdd(in_lds ? s_frames + g : d.frame_counts + 2 * (size_t)g, 1);
        for (int q = 0; q < RO_REASONS; q++) why[q] += kind == q ? 1 : 0;
      }
      at += __popc(m);
    }
    if (!WRITE) {
      for (int s = RO_LANES / 2; s >= 1; s >>= 1)
        for (int q = 0; q < RO_REASONS; q++) why[q] += __shfl_down(why[q], s, RO_LANES);
      if (ln == 0) {
        ((int2 *)d.scan)[t] = make_int2(at, 0);
        for (int q = 0; q < RO_REASONS; q++)
          if (why[q]) atomicAdd(s_why + q, (unsigned long long)why[q]);
      }
    }
  }
  if (!WRITE) {
    __syncthreads();
    if (in_lds)
      for (int32_t g = threadIdx.x; g < d.n_frames; g += 256)
        if (s_frames[g]) atomicAdd(d.frame_counts + 2 * (size_t)g, s_frames[g]);
    if (threadIdx.x < RO_REASONS && s_why[threadIdx.x]) atomicAdd(d.stats + threadIdx.x, s_why[threadIdx.x]);
  }
}

__global__ __launch_bounds__(256) void k_ro_search(RoDevice d, int32_t n_cand) {
  const int ln = threadIdx.x & 15;
  const int64_t c = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (c >= n_cand) return;  // whole groups leave together
  int32_t *r = d.cand + RO_CAND_INTS * (size_t)c;
  const int32_t t = r[0], g = r[1];
  const double pu = d.cand_uv[2 * c], pv = d.cand_uv[2 * c + 1];
  // the track's reference feature: its class and descriptor
  const size_t ref = (size_t)d.offsets[t] + d.ref_obs[t];
  const int4 *ref_rec = (const int4 *)(d.frame_feat[d.obs_frames[ref]] + RO_FEAT_INTS * (size_t)d.obs_feat[ref]);
  const int32_t cls = ref_rec[0].w & 3;
  const int4 a0 = ref_rec[1], a1 = ref_rec[2];
  const uint32_t a[8] = {(uint32_t)a0.x, (uint32_t)a0.y, (uint32_t)a0.z, (uint32_t)a0.w, (uint32_t)a1.x, (uint32_t)a1.y, (uint32_t)a1.z, (uint32_t)a1.w};
  int32_t bu0, bu1, bv0, bv1;
  ro_bin_span(pu, d.prm.radius, d.width - 1, d.grid.shift, &bu0, &bu1);
  ro_bin_span(pv, d.prm.radius, d.height - 1, d.grid.shift, &bv0, &bv1);
  const int2 *bins = (const int2 *)d.bins + (size_t)g * ro_frame_bins(d.grid) + (size_t)cls * d.grid.nbv * d.grid.nbu;
  const int4 *sorted = (const int4 *)d.sorted;
  RoBest best;
  ro_best_init(&best);
  for (int32_t bv = bv0; bv <= bv1; bv++) {
    // a row's bins lie one after the other, and so do their records
    const int2 first = bins[(size_t)bv * d.grid.nbu + bu0], last = bins[(size_t)bv * d.grid.nbu + bu1];
    const int32_t end = last.x + last.y;
    for (int32_t i = first.x + ln; i < end; i += RO_LANES) {
      const int4 head = sorted[3 * (size_t)i], b0 = sorted[3 * (size_t)i + 1], b1 = sorted[3 * (size_t)i + 2];
      if (!ro_in_window(head.x, head.y, pu, pv, d.prm.radius)) continue;
      const uint32_t b[8] = {(uint32_t)b0.x, (uint32_t)b0.y, (uint32_t)b0.z, (uint32_t)b0.w, (uint32_t)b1.x, (uint32_t)b1.y, (uint32_t)b1.z, (uint32_t)b1.w};
      ro_best_add(&best, ro_sad(a, b), head.z);
    }
  }
  for (int s = RO_LANES / 2; s >= 1; s >>= 1) {
    const unsigned long long key = __shfl_down((unsigned long long)best.key, s, RO_LANES);
    const int32_t second = __shfl_down(best.second, s, RO_LANES), n = __shfl_down(best.n, s, RO_LANES);
    ro_best_merge(&best, key, second, n);  // (what the lanes l >= s compute is never read)
  }
  if (ln == 0) {
    const int32_t code = ro_window_code(best, d.prm);
    ro_record(r, best, code);
    if (code == RO_ACCEPTED) {
      const size_t j = (size_t)d.feat_offsets[g] + (uint32_t)best.key;
      atomicMin(d.claim + j, (unsigned long long)((best.key & 0xffffffff00000000ull) | (uint32_t)c));
    }
  }
}

__global__ __launch_bounds__(256) void k_ro_verdict(RoDevice d, int32_t n_cand) {
  int32_t count[RO_CODES] = {0, 0, 0, 0, 0};
  for (int64_t c = ro_gid(); c < n_cand; c += ro_gsize()) {
    int32_t *r = d.cand + RO_CAND_INTS * (size_t)c;
    int32_t code = r[6];
    if (code == RO_ACCEPTED) {
      const unsigned long long key = d.claim[(size_t)d.feat_offsets[r[1]] + r[2]];
      if ((uint32_t)key != (uint32_t)c) {
        code = RO_LOST;
        r[6] = code;
      } else {
        atomicAdd(d.track_accepted + r[0], 1);
        atomicAdd(d.frame_counts + 2 * (size_t)r[1] + 1, 1);
      }
    }
    for (int q = 0; q < RO_CODES; q++) count[q] += code == q ? 1 : 0;
  }
  // the wave's lanes are together again: one atomic per wave and code
  for (int q = 0; q < RO_CODES; q++) {
    int32_t v = count[q];
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_down(v, s);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(d.stats + RO_REASONS + q, (unsigned long long)v);
  }
}

inline int ro_grid_for(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 2048)); }

}  // namespace

#define RO_LAUNCH(id, kernel, grid, ...)                                  \
  do {                                                                    \
    pf.begin(id, s);                                                      \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, __VA_ARGS__); \
    pf.end(s);                                                            \
  } while (0)

void vsm_reobserve_launch_count(hipStream_t s, VsmProf &pf, const RoDevice &d) {
  if (d.n_tracks <= 0 || d.n_frames <= 0) return;
  if (d.n_obs > 0) RO_LAUNCH(VSM_K_RO_OCCUPY, k_ro_occupy, ro_grid_for(d.n_obs), d);
  if (d.n_feat > 0) RO_LAUNCH(VSM_K_RO_BIN_COUNT, k_ro_bin_count, ro_grid_for(d.n_feat), d);
  vsm_tracks_launch_scan(s, pf, d.bins, d.n_frames * ro_frame_bins(d.grid), d.bins_part, d.bins_total);
  if (d.n_feat > 0) RO_LAUNCH(VSM_K_RO_SCATTER, k_ro_scatter, ro_grid_for(d.n_feat), d);
  RO_LAUNCH(VSM_K_RO_COUNT, k_ro_project<false>, ro_grid_for((int64_t)d.n_tracks * 16), d);
  vsm_tracks_launch_scan(s, pf, d.scan, d.n_tracks, d.scan_part, d.totals);
}

void vsm_reobserve_launch_search(hipStream_t s, VsmProf &pf, const RoDevice &d, int32_t n_cand) {
  if (n_cand <= 0) return;
  RO_LAUNCH(VSM_K_RO_LIST, k_ro_project<true>, ro_grid_for((int64_t)d.n_tracks * 16), d);
  RO_LAUNCH(VSM_K_RO_SEARCH, k_ro_search, (uint32_t)(((int64_t)n_cand + 15) / 16), d, n_cand);
  RO_LAUNCH(VSM_K_RO_VERDICT, k_ro_verdict, ro_grid_for(n_cand), d, n_cand);
}
