// Feature tracks on the device: connected components of the match graph (vsm_tracks.h has the definitions and the
// union-find steps; vsm_tracks.inc the host side).  All kernels are grid-stride with 256-thread workgroups, and none of
// them waits for another workgroup: what one level of the scan needs from the one above comes from a separate launch.
#include "vsm_internal.h"
#include "vsm_tracks.h"

namespace {

constexpr int kB = TRK_SCAN_BLOCK;
constexpr int kLdsBase = 4096;  // pair_base entries a workgroup keeps in LDS; longer tables are searched in global memory
static_assert(kB == 256, "one scan item per thread");

__device__ inline int64_t trk_gid() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ inline int64_t trk_gsize() { return (int64_t)gridDim.x * blockDim.x; }

// pair_base into LDS where it fits; returns the table to search
template <bool LDS>
__device__ inline const int32_t *trk_stage_base(const int32_t *pair_base, int32_t n_pairs, int32_t *s_base) {
  if (!LDS) return pair_base;
  for (int i = threadIdx.x; i <= n_pairs; i += blockDim.x) s_base[i] = pair_base[i];
  __syncthreads();
  return s_base;
}

// ---- 1: parent[v] = v, first[v] = unused ----
__global__ __launch_bounds__(256) void k_trk_init(TrkDevice d) {
  if (trk_gid() < 4) d.counters[trk_gid()] = 0;
  for (int64_t v = trk_gid(); v < d.n_nodes; v += trk_gsize()) {
    d.parent[v] = (int32_t)v;
    d.first[v] = TRK_UNUSED;
    d.size[v] = 0;
    d.cursor[v] = 0;
  }
}

// ---- 2: one thread per edge: the first match that names each end, then the union ----
template <bool LDS>
__global__ __launch_bounds__(256) void k_trk_hook(TrkDevice d) {
  __shared__ int32_t s_base[LDS ? kLdsBase + 1 : 1];
  const int32_t *base = trk_stage_base<LDS>(d.pair_base, d.n_pairs, s_base);
  for (int64_t e = trk_gid(); e < d.n_edges; e += trk_gsize()) {
    const int32_t k = trk_owner(base, d.n_pairs, (int32_t)e);
    const int32_t u = d.feat_base[d.pairs[2 * k]] + d.edges[2 * e], v = d.feat_base[d.pairs[2 * k + 1]] + d.edges[2 * e + 1];
    atomicMin(d.first + u, (int32_t)(2 * e));
    atomicMin(d.first + v, (int32_t)(2 * e + 1));
    trk_unite(d.parent, u, v);
  }
}

// ---- 3, 4: parent[v] = root for the nodes in use, and the number of them per root ----
__global__ __launch_bounds__(256) void k_trk_flatten(TrkDevice d) {
  for (int64_t v = trk_gid(); v < d.n_nodes; v += trk_gsize()) {
    if (d.first[v] == TRK_UNUSED) continue;
    const int32_t r = trk_find(d.parent, (int32_t)v);
    trk_lower(d.parent + v, r);  // (lowering, not storing: a halving step of another thread cannot put an ancestor back)
    atomicAdd(d.size + r, 1);
  }
}

// ---- 5: the scan's input: (1, size) at a kept root, (0, 0) elsewhere ----
__global__ __launch_bounds__(256) void k_trk_keep(TrkDevice d) {
  int2 *x = (int2 *)d.scan;
  for (int64_t v = trk_gid(); v < d.n_nodes; v += trk_gsize()) {
    const int32_t n = d.size[v];
    const bool keep = d.parent[v] == v && d.first[v] != TRK_UNUSED && n >= d.min_length;
    x[v] = keep ? make_int2(1, n) : make_int2(0, 0);
  }
}

// ---- 6: exclusive scan of int2 items, kB per workgroup: reduce, scan of the partials (the same kernels, one level up), apply ----
__device__ inline int2 trk_wave_inclusive(int2 v, int lane) {
  for (int dlt = 1; dlt < 64; dlt <<= 1) {
    const int ax = __shfl_up(v.x, dlt), ay = __shfl_up(v.y, dlt);
    if (lane >= dlt) {
      v.x += ax;
      v.y += ay;
    }
  }
  return v;
}
// exclusive prefix of v over the workgroup's 256 threads; *total = the workgroup's sum (same value in every thread)
__device__ inline int2 trk_block_exclusive(int2 v, int2 *total) {
  __shared__ int2 s_wave[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int2 inc = trk_wave_inclusive(v, lane);
  __syncthreads();  // (s_wave of the call before has been read)
  if (lane == 63) s_wave[w] = inc;
  __syncthreads();
  int2 pre = make_int2(inc.x - v.x, inc.y - v.y), sum = make_int2(0, 0);
  for (int i = 0; i < 4; i++) {
    if (i < w) {
      pre.x += s_wave[i].x;
      pre.y += s_wave[i].y;
    }
    sum.x += s_wave[i].x;
    sum.y += s_wave[i].y;
  }
  *total = sum;
  return pre;
}
__global__ __launch_bounds__(256) void k_trk_scan_reduce(const int2 *x, int32_t n, int2 *part, int32_t n_part) {
  for (int32_t b = blockIdx.x; b < n_part; b += gridDim.x) {
    const int64_t i = (int64_t)b * kB + threadIdx.x;
    int2 sum;
    (void)trk_block_exclusive(i < n ? x[i] : make_int2(0, 0), &sum);
    if (threadIdx.x == 0) part[b] = sum;
  }
}
__global__ __launch_bounds__(256) void k_trk_scan_top(int2 *x, int32_t n, int2 *total) {  // one workgroup, n <= kB
  int2 sum;
  const int2 pre = trk_block_exclusive((int)threadIdx.x < n ? x[threadIdx.x] : make_int2(0, 0), &sum);
  if ((int)threadIdx.x < n) x[threadIdx.x] = pre;
  if (threadIdx.x == 0) *total = sum;
}
__global__ __launch_bounds__(256) void k_trk_scan_apply(int2 *x, int32_t n, const int2 *part, int32_t n_part) {
  for (int32_t b = blockIdx.x; b < n_part; b += gridDim.x) {
    const int64_t i = (int64_t)b * kB + threadIdx.x;
    int2 sum;
    const int2 pre = trk_block_exclusive(i < n ? x[i] : make_int2(0, 0), &sum);
    const int2 off = part[b];
    if (i < n) x[i] = make_int2(pre.x + off.x, pre.y + off.y);
  }
}

__device__ inline bool trk_kept(const TrkDevice &d, int32_t root) { return d.size[root] >= d.min_length; }

// ---- 9: the track of every match ----
template <bool LDS>
__global__ __launch_bounds__(256) void k_trk_match_tracks(TrkDevice d) {
  __shared__ int32_t s_base[LDS ? kLdsBase + 1 : 1];
  const int32_t *base = trk_stage_base<LDS>(d.pair_base, d.n_pairs, s_base);
  for (int64_t e = trk_gid(); e < d.n_edges; e += trk_gsize()) {
    const int32_t k = trk_owner(base, d.n_pairs, (int32_t)e);
    const int32_t r = d.parent[d.feat_base[d.pairs[2 * k]] + d.edges[2 * e]];
    d.track_of_match[e] = trk_kept(d, r) ? d.scan[2 * (int64_t)r] : -1;
  }
}

// ---- 7: every kept node takes a slot of its track's segment; the kept roots write the offsets ----
template <bool LDS>
__global__ __launch_bounds__(256) void k_trk_fill(TrkDevice d, int32_t n_tracks, int32_t n_obs) {
  __shared__ int32_t s_base[LDS ? kLdsBase + 1 : 1];
  const int32_t *base = trk_stage_base<LDS>(d.pair_base, d.n_pairs, s_base);
  const int2 *x = (const int2 *)d.scan;
  if (trk_gid() == 0) d.offsets[n_tracks] = n_obs;
  for (int64_t v = trk_gid(); v < d.n_nodes; v += trk_gsize()) {
    const int32_t fv = d.first[v];
    if (fv == TRK_UNUSED) continue;
    const int32_t r = d.parent[v];
    if (!trk_kept(d, r)) continue;
    const int2 to = x[r];  // (track number, offset of its segment)
    if (r == v) d.offsets[to.x] = to.y;
    const int32_t e = fv >> 1, end = fv & 1, k = trk_owner(base, d.n_pairs, e);
    const int32_t frame = d.pairs[2 * k + end];
    const int32_t slot = to.y + atomicAdd(d.cursor + r, 1);
    ((int4 *)d.obs)[slot] = make_int4(frame, (int32_t)v - d.feat_base[frame], k, 2 * (e - base[k]) + end);
  }
}

// ---- 8: every segment into ascending (frame, feature) order; inconsistent = two observations in one frame ----
// a wave per segment of at most VSM_TRACKS_WAVE_MAX rows: a row per lane, its rank by counting over shuffles
__global__ __launch_bounds__(256) void k_trk_order_wave(TrkDevice d, int32_t n_tracks) {
  int4 *obs = (int4 *)d.obs;
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = trk_gsize() >> 6;
  for (int64_t t = trk_gid() >> 6; t < n_tracks; t += n_waves) {  // (t, o and len are the same in every lane of a wave)
    const int32_t o = d.offsets[t], len = d.offsets[t + 1] - o;
    if (len > VSM_TRACKS_WAVE_MAX) {
      if (lane == 0 && len <= VSM_TRACKS_BLOCK_MAX) d.mid_list[atomicAdd(d.counters, 1)] = (int32_t)t;
      continue;  // (longer still: the host orders it)
    }
    const int4 row = lane < len ? obs[o + lane] : make_int4(TRK_UNUSED, TRK_UNUSED, 0, 0);
    int rank = 0;
    bool dup = false;
    for (int j = 0; j < len; j++) {
      const int fj = __shfl(row.x, j), gj = __shfl(row.y, j);
      rank += (fj < row.x || (fj == row.x && gj < row.y)) ? 1 : 0;
      dup = dup || (fj == row.x && j != lane);
    }
    const unsigned long long any = __ballot(dup && lane < len);
    if (lane < len) obs[o + rank] = row;  // (every lane has loaded its row: one instruction stream)
    if (lane == 0) d.flags[t] = any ? 1 : 0;
  }
}
// a workgroup per segment of at most VSM_TRACKS_BLOCK_MAX rows, in LDS
__global__ __launch_bounds__(256) void k_trk_order_block(TrkDevice d) {
  __shared__ int4 s_rows[VSM_TRACKS_BLOCK_MAX];
  int4 *obs = (int4 *)d.obs;
  const int32_t n_mid = d.counters[0];
  for (int32_t i = blockIdx.x; i < n_mid; i += gridDim.x) {
    const int32_t t = d.mid_list[i], o = d.offsets[t], len = d.offsets[t + 1] - o;
    for (int j = threadIdx.x; j < len; j += blockDim.x) s_rows[j] = obs[o + j];
    __syncthreads();
    int dup = 0;
    for (int j = threadIdx.x; j < len; j += blockDim.x) {
      const int4 row = s_rows[j];
      int rank = 0;
      for (int q = 0; q < len; q++) {
        const int fq = s_rows[q].x, gq = s_rows[q].y;
        rank += (fq < row.x || (fq == row.x && gq < row.y)) ? 1 : 0;
        dup |= (fq == row.x && q != j) ? 1 : 0;
      }
      obs[o + rank] = row;
    }
    dup = __syncthreads_or(dup);  // (also: s_rows has been read before the next segment overwrites it)
    if (threadIdx.x == 0) d.flags[t] = dup ? 1 : 0;
  }
}

inline int trk_grid(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 2048)); }

}  // namespace

#define TRK_LAUNCH(id, kernel, grid, ...)                                  \
  do {                                                                     \
    pf.begin(id, s);                                                       \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, __VA_ARGS__); \
    pf.end(s);                                                             \
  } while (0)

void vsm_tracks_launch_scan(hipStream_t s, VsmProf &pf, int32_t *scan, int32_t n_items, int32_t *scan_part, int32_t *totals) {
  // the levels of the scan: level 0 is the items, level l + 1 the workgroup sums of level l
  int2 *lev[8];
  int32_t n[8];
  int top = 0;
  lev[0] = (int2 *)scan;
  n[0] = n_items;
  int2 *next = (int2 *)scan_part;
  while (n[top] > kB) {
    n[top + 1] = (int32_t)(((int64_t)n[top] + kB - 1) / kB);
    lev[top + 1] = next;
    next += n[top + 1];
    TRK_LAUNCH(VSM_K_TRK_SCAN_REDUCE, k_trk_scan_reduce, std::min(n[top + 1], 2048), (const int2 *)lev[top], n[top], lev[top + 1], n[top + 1]);
    top++;
  }
  TRK_LAUNCH(VSM_K_TRK_SCAN_TOP, k_trk_scan_top, 1, lev[top], n[top], (int2 *)totals);
  for (int l = top - 1; l >= 0; l--)
    TRK_LAUNCH(VSM_K_TRK_SCAN_APPLY, k_trk_scan_apply, std::min(n[l + 1], 2048), lev[l], n[l], (const int2 *)lev[l + 1], n[l + 1]);
}

void vsm_tracks_launch_link(hipStream_t s, VsmProf &pf, const TrkDevice &d) {
  const bool lds = d.n_pairs <= kLdsBase;
  const int gn = trk_grid(d.n_nodes), ge = trk_grid(d.n_edges);
  TRK_LAUNCH(VSM_K_TRK_INIT, k_trk_init, gn, d);
  if (lds)
    TRK_LAUNCH(VSM_K_TRK_HOOK, k_trk_hook<true>, ge, d);
  else
    TRK_LAUNCH(VSM_K_TRK_HOOK, k_trk_hook<false>, ge, d);
  TRK_LAUNCH(VSM_K_TRK_FLATTEN, k_trk_flatten, gn, d);
  TRK_LAUNCH(VSM_K_TRK_KEEP, k_trk_keep, gn, d);
  vsm_tracks_launch_scan(s, pf, d.scan, d.n_nodes, d.scan_part, d.totals);
}

void vsm_tracks_launch_emit(hipStream_t s, VsmProf &pf, const TrkDevice &d, int32_t n_tracks, int32_t n_obs) {
  const bool lds = d.n_pairs <= kLdsBase;
  const int gn = trk_grid(d.n_nodes), ge = trk_grid(d.n_edges);
  if (lds) {
    TRK_LAUNCH(VSM_K_TRK_MATCH_TRACKS, k_trk_match_tracks<true>, ge, d);
    TRK_LAUNCH(VSM_K_TRK_FILL, k_trk_fill<true>, gn, d, n_tracks, n_obs);
  } else {
    TRK_LAUNCH(VSM_K_TRK_MATCH_TRACKS, k_trk_match_tracks<false>, ge, d);
    TRK_LAUNCH(VSM_K_TRK_FILL, k_trk_fill<false>, gn, d, n_tracks, n_obs);
  }
  if (n_tracks <= 0) return;
  TRK_LAUNCH(VSM_K_TRK_ORDER_WAVE, k_trk_order_wave, trk_grid((int64_t)n_tracks * 64), d, n_tracks);
  // (the number of segments for a workgroup is on the device only: at most one per VSM_TRACKS_WAVE_MAX + 1 observations)
  TRK_LAUNCH(VSM_K_TRK_ORDER_BLOCK, k_trk_order_block, std::max(1, std::min(n_obs / (VSM_TRACKS_WAVE_MAX + 1), 1024)), d);
}
