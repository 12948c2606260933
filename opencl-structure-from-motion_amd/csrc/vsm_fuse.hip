// Fusion on the device (vsm_fuse.h has the arithmetic, vsm_fuse.inc the host side).
//
// k_fu_owner: a lane per observation of a track in use lowers its feature's owner to its track (32-bit atomicMin).
// k_fu_bin_count / k_fu_scatter: a lane per feature; the owned features are counted per (frame, class, bin) of ro_grid, the
// tracks' multi-level scan turns the counts into starts, and each record goes to its bin's next place with its index in
// word 2 - the order inside a bin is whatever the atomics give, and nothing below depends on it.
// k_fu_search<false>, the hot kernel: a 16-lane group per track, sixteen groups per 256-thread workgroup, the workgroups
// striding the tracks.  The group walks the frames 16 at a time, a lane projecting into its frame (reasons, candidates); then
// the group takes the sixteen's candidates one after the other, all lanes on one window: the bins a window touches are, row
// by row, one contiguous run of sorted records, the lanes stride the run, a lane reads a record as three 16-byte loads and
// costs it with v_sad_u8 (ro_sad).  Best, second and size are merged across the group by cross-lane moves of width 16 (no
// LDS, no barrier).  The pass counts: proposals per track for the scan, candidates and proposals per frame, the reasons and
// the empty windows.  No candidate is written anywhere.  In the compacting form (d.slots) lane 0 also writes each proposal's
// record - the window's code, the best feature's owner - into the track's own places, and k_fu_compact, behind the host's wait
// for the proposals' number, moves them to the track's prefix: the list is in (track, frame) order.
// k_fu_search<true>, where the places would be too large: the same walk a second time, a proposal's place being the track's
// prefix plus the proposals the group has written.
// k_fu_conflict: a 16-lane group per proposal that came through its window's tests; the lanes stride a's frames, each against
// b's; without a common frame lane 0 bids for a's partner (64-bit atomicMin of cost << 32 | proposal).
// k_fu_verdict: a lane per proposal - outbid, one-sided or fused; the track's partner, the absorbed track's survivor, the codes'
// counts.  k_fu_lengths: a lane per track, its length after the fusions, for the scan.  k_fu_merge: a 16-lane group per
// track writes offsets_after and obs_src; a survivor's lanes stride the two tracks' observations, each finds its place by
// fu_rank - whatever the lengths, 2 or 257.
// All control flow is uniform inside a group; the groups of a wave differ in their trip counts only.
#include "vsm_internal.h"
#include "vsm_fuse.h"
#include "vsm_tracks.h"

namespace {

__device__ inline uint32_t fu_group_ballot(bool pred) {
  const unsigned long long all = __ballot(pred);
  return (uint32_t)(all >> (threadIdx.x & 48)) & 0xffffu;
}
__device__ inline int64_t fu_gid() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ inline int64_t fu_gsize() { return (int64_t)gridDim.x * blockDim.x; }

__global__ __launch_bounds__(256) void k_fu_owner(FuDevice d) {
  for (int64_t i = fu_gid(); i < d.n_obs; i += fu_gsize()) {
    const int32_t t = trk_owner(d.offsets, d.n_tracks, (int32_t)i);
    if (d.use[t]) atomicMin(d.owner + (size_t)d.feat_offsets[d.obs_frames[i]] + d.obs_feat[i], (uint32_t)t);
  }
}

// a feature's frame, index and bin; false for one nobody owns
__device__ inline bool fu_owned_feature(const FuDevice &d, int32_t j, const int32_t **rec, int32_t *k, size_t *bin) {
  if (d.owner[j] == FU_NO_OWNER) return false;
  const int32_t g = trk_owner(d.feat_offsets, d.n_frames, j);
  *k = j - d.feat_offsets[g];
  *rec = d.frame_feat[g] + RO_FEAT_INTS * (size_t)*k;
  const int4 head = *(const int4 *)*rec;  // {u, v, 0, class}
  *bin = (size_t)g * ro_frame_bins(d.grid) + ro_bin(d.grid, head.w, head.x, head.y);
  return true;
}
__global__ __launch_bounds__(256) void k_fu_bin_count(FuDevice d) {
  for (int64_t j = fu_gid(); j < d.n_feat; j += fu_gsize()) {
    const int32_t *rec;
    int32_t k;
    size_t bin;
    if (fu_owned_feature(d, (int32_t)j, &rec, &k, &bin)) atomicAdd(d.bins + 2 * bin, 1);
  }
}
// (the scan has left every bin's second word at zero: it is the bin's cursor, and its count at the end)
__global__ __launch_bounds__(256) void k_fu_scatter(FuDevice d) {
  for (int64_t j = fu_gid(); j < d.n_feat; j += fu_gsize()) {
    const int32_t *rec;
    int32_t k;
    size_t bin;
    if (!fu_owned_feature(d, (int32_t)j, &rec, &k, &bin)) continue;
    const int32_t at = d.bins[2 * bin] + atomicAdd(d.bins + 2 * bin + 1, 1);
    int4 head = ((const int4 *)rec)[0];
    head.z = k;
    int4 *out = (int4 *)d.sorted + 3 * (size_t)at;
    out[0] = head;
    out[1] = ((const int4 *)rec)[1];
    out[2] = ((const int4 *)rec)[2];
  }
}

// The window of a projection (pu, pv) into frame g among the owned features of class cls, by the whole group; the result
// stands in the group's lane 0.
__device__ inline RoBest fu_window(const FuDevice &d, int32_t g, int32_t cls, const uint32_t *a, double pu, double pv, int ln) {
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
  return best;
}

// The counting pass keeps its frames' counts (up to FU_LDS_FRAMES frames) and the reasons in LDS and hands them on with one
// atomic per workgroup and non-zero entry, as the re-observation's does.
enum { FU_LDS_FRAMES = 2048 };
template <bool WRITE>
__global__ __launch_bounds__(256) void k_fu_search(FuDevice d) {
  __shared__ int32_t s_frames[WRITE ? 2 : 2 * FU_LDS_FRAMES];
  __shared__ unsigned long long s_why[RO_REASONS + 1];  // the reasons, then the empty windows
  const int grp = threadIdx.x >> 4, ln = threadIdx.x & 15;
  const bool in_lds = !WRITE && d.n_frames <= FU_LDS_FRAMES;
  if (!WRITE) {
    if (in_lds)
      for (int32_t g = threadIdx.x; g < 2 * d.n_frames; g += 256) s_frames[g] = 0;
    if (threadIdx.x <= RO_REASONS) s_why[threadIdx.x] = 0;
    __syncthreads();
  }
  int32_t *const per_frame = in_lds ? s_frames : d.frame_counts;
  for (int64_t t = (int64_t)blockIdx.x * 16 + grp; t < d.n_tracks; t += (int64_t)gridDim.x * 16) {  // (a group's lanes share t)
    if (!d.use[t]) {
      if (!WRITE && ln == 0) ((int2 *)d.scan)[t] = make_int2(0, 0);
      continue;
    }
    const int32_t o = d.offsets[t], n = d.offsets[t + 1] - o;
    const double X[3] = {d.xyz[3 * t + 0], d.xyz[3 * t + 1], d.xyz[3 * t + 2]};
    // the track's reference feature: its class and descriptor
    const size_t ref = (size_t)o + d.ref_obs[t];
    const int4 *ref_rec = (const int4 *)(d.frame_feat[d.obs_frames[ref]] + RO_FEAT_INTS * (size_t)d.obs_feat[ref]);
    const int32_t cls = ref_rec[0].w & 3;
    const int4 a0 = ref_rec[1], a1 = ref_rec[2];
    const uint32_t a[8] = {(uint32_t)a0.x, (uint32_t)a0.y, (uint32_t)a0.z, (uint32_t)a0.w, (uint32_t)a1.x, (uint32_t)a1.y, (uint32_t)a1.z, (uint32_t)a1.w};
    int32_t at = WRITE ? d.scan[2 * t] : 0;  // the proposals in front of this track; then those of the frames walked
    int32_t why[RO_REASONS] = {0, 0, 0, 0, 0}, empty = 0;
    for (int32_t g0 = 0; g0 < d.n_frames; g0 += RO_LANES) {
      const int32_t g = g0 + ln;
      double pu = 0.0, pv = 0.0;
      int32_t kind = -1;
      if (g < d.n_frames)
        kind = ro_pair(d.search[g], d.valid[g], d.obs_frames + o, n, g, d.states + 12 * (size_t)g, X, d.f, d.cu, d.cv, d.prm.min_depth, d.width, d.height, &pu, &pv);
      const bool is_cand = kind == RO_CANDIDATE;
      if (!WRITE) {
        if (is_cand) atomicAdd(per_frame + 2 * (size_t)g, 1);
        for (int q = 0; q < RO_REASONS; q++) why[q] += kind == q ? 1 : 0;
      }
      for (uint32_t m = fu_group_ballot(is_cand); m; m &= m - 1) {
        const int src = __ffs(m) - 1;
        const double cpu = __shfl(pu, src, RO_LANES), cpv = __shfl(pv, src, RO_LANES);
        const int32_t cg = g0 + src;
        const RoBest best = fu_window(d, cg, cls, a, cpu, cpv, ln);
        const bool some = __shfl(best.n, 0, RO_LANES) > 0;
        if (ln == 0) {
          if (!WRITE) {
            if (some)
              atomicAdd(per_frame + 2 * (size_t)cg + 1, 1);
            else
              empty++;
          }
          if (some && (WRITE || d.slots)) {  // (the compacting form keeps the counting pass's proposals in the track's places)
            const size_t to = WRITE ? (size_t)at : (size_t)d.use_rank[t] * d.slot_stride + at;
            int32_t *r = (WRITE ? d.prop : d.slots) + FU_PROP_INTS * to;
            double *ruv = (WRITE ? d.prop_uv : d.slots_uv) + 2 * to;
            r[0] = (int32_t)t;
            r[1] = cg;
            ro_record(r, best, ro_window_code(best, d.prm));
            r[7] = (int32_t)d.owner[(size_t)d.feat_offsets[cg] + (uint32_t)best.key];
            ruv[0] = cpu;
            ruv[1] = cpv;
          }
        }
        at += some ? 1 : 0;
      }
    }
    if (!WRITE) {
      for (int s = RO_LANES / 2; s >= 1; s >>= 1)
        for (int q = 0; q < RO_REASONS; q++) why[q] += __shfl_down(why[q], s, RO_LANES);
      if (ln == 0) {
        ((int2 *)d.scan)[t] = make_int2(at, 0);
        for (int q = 0; q < RO_REASONS; q++)
          if (why[q]) atomicAdd(s_why + q, (unsigned long long)why[q]);
        if (empty) atomicAdd(s_why + RO_REASONS, (unsigned long long)empty);
      }
    }
  }
  if (!WRITE) {
    __syncthreads();
    if (in_lds)
      for (int32_t g = threadIdx.x; g < 2 * d.n_frames; g += 256)
        if (s_frames[g]) atomicAdd(d.frame_counts + g, s_frames[g]);
    if (threadIdx.x < RO_REASONS && s_why[threadIdx.x]) atomicAdd(d.stats + threadIdx.x, s_why[threadIdx.x]);
    if (threadIdx.x == RO_REASONS && s_why[RO_REASONS]) atomicAdd(d.stats + RO_REASONS + FU_EMPTY, s_why[RO_REASONS]);
  }
}

// the compacting form: a 16-lane group per track moves the proposals from the track's places to the list, a lane a proposal
__global__ __launch_bounds__(256) void k_fu_compact(FuDevice d, int32_t n_prop) {
  const int grp = threadIdx.x >> 4, ln = threadIdx.x & 15;
  for (int64_t t = (int64_t)blockIdx.x * 16 + grp; t < d.n_tracks; t += (int64_t)gridDim.x * 16) {
    if (!d.use[t]) continue;
    const int32_t at = d.scan[2 * t], n = (t + 1 < d.n_tracks ? d.scan[2 * (t + 1)] : n_prop) - at;
    const size_t from = (size_t)d.use_rank[t] * d.slot_stride;
    for (int32_t i = ln; i < n; i += RO_LANES) {
      const int4 *src = (const int4 *)(d.slots + FU_PROP_INTS * (from + i));
      int4 *dst = (int4 *)(d.prop + FU_PROP_INTS * ((size_t)at + i));
      dst[0] = src[0];
      dst[1] = src[1];
      ((double2 *)d.prop_uv)[(size_t)at + i] = ((const double2 *)d.slots_uv)[from + i];
    }
  }
}

__global__ __launch_bounds__(256) void k_fu_conflict(FuDevice d, int32_t n_prop) {
  const int ln = threadIdx.x & 15;
  const int64_t p = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (p >= n_prop) return;  // whole groups leave together
  int32_t *r = d.prop + FU_PROP_INTS * (size_t)p;
  if (r[6] != FU_FUSED) return;  // (the window's own code: the group's lanes read the same word)
  const int32_t a = r[0], b = r[7];
  const int32_t oa = d.offsets[a], ob = d.offsets[b];
  const bool hit = fu_conflict(d.obs_frames + oa, d.offsets[a + 1] - oa, d.obs_frames + ob, d.offsets[b + 1] - ob, ln, RO_LANES);
  const bool any = fu_group_ballot(hit) != 0;
  if (ln != 0) return;
  if (any)
    r[6] = FU_CONFLICT;
  else
    atomicMin(d.choice + a, (unsigned long long)fu_bid(r[3], (int32_t)p));
}

__global__ __launch_bounds__(256) void k_fu_verdict(FuDevice d, int32_t n_prop) {
  int32_t count[FU_CODES + 1] = {0, 0, 0, 0, 0, 0, 0, 0};  // the codes, then the fusions
  for (int64_t p = fu_gid(); p < n_prop; p += fu_gsize()) {
    int32_t *r = d.prop + FU_PROP_INTS * (size_t)p;
    int32_t code = r[6];
    if (code == FU_FUSED) {
      code = fu_verdict(d.prop, d.choice, (int32_t)p);
      r[6] = code;
      if (code != FU_OUTBID) d.partner[r[0]] = r[7];
      if (code == FU_FUSED) {
        if (r[0] > r[7])
          d.fused_into[r[0]] = r[7];
        else
          count[FU_CODES]++;
      }
    }
    for (int q = 0; q < FU_CODES; q++) count[q] += code == q ? 1 : 0;
  }
  // the wave's lanes are together again: one atomic per wave and counter
  for (int q = 0; q <= FU_CODES; q++) {
    int32_t v = count[q];
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_down(v, s);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(d.stats + RO_REASONS + q, (unsigned long long)v);
  }
}

__global__ __launch_bounds__(256) void k_fu_lengths(FuDevice d) {
  for (int64_t t = fu_gid(); t < d.n_tracks; t += fu_gsize()) ((int2 *)d.scan)[t] = make_int2(fu_length_after(d.offsets, d.partner, d.fused_into, (int32_t)t), 0);
}

__global__ __launch_bounds__(256) void k_fu_merge(FuDevice d) {
  const int grp = threadIdx.x >> 4, ln = threadIdx.x & 15;
  if (blockIdx.x == 0 && threadIdx.x == 0) d.offsets_after[d.n_tracks] = d.totals[0];
  for (int64_t t = (int64_t)blockIdx.x * 16 + grp; t < d.n_tracks; t += (int64_t)gridDim.x * 16) {
    const int32_t at = d.scan[2 * t];
    if (ln == 0) d.offsets_after[t] = at;
    if (d.fused_into[t] >= 0) continue;
    const int32_t o = d.offsets[t], n = d.offsets[t + 1] - o;
    if (!fu_survivor(d.partner, d.fused_into, (int32_t)t)) {
      for (int32_t i = ln; i < n; i += RO_LANES) d.obs_src[(size_t)at + i] = o + i;
      continue;
    }
    const int32_t b = d.partner[t], ob = d.offsets[b], nb = d.offsets[b + 1] - ob;
    for (int32_t i = ln; i < n + nb; i += RO_LANES)
      d.obs_src[(size_t)at + fu_rank(d.obs_frames + o, n, d.obs_frames + ob, nb, i)] = i < n ? o + i : ob + (i - n);
  }
}

inline int fu_grid_for(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 2048)); }

}  // namespace

#define FU_LAUNCH(id, kernel, grid, ...)                                  \
  do {                                                                    \
    pf.begin(id, s);                                                      \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, __VA_ARGS__); \
    pf.end(s);                                                            \
  } while (0)

void vsm_fuse_launch_count(hipStream_t s, VsmProf &pf, const FuDevice &d) {
  if (d.n_tracks <= 0 || d.n_frames <= 0) return;
  if (d.n_obs > 0) FU_LAUNCH(VSM_K_FU_OWNER, k_fu_owner, fu_grid_for(d.n_obs), d);
  if (d.n_feat > 0) FU_LAUNCH(VSM_K_FU_BIN_COUNT, k_fu_bin_count, fu_grid_for(d.n_feat), d);
  vsm_tracks_launch_scan(s, pf, d.bins, d.n_frames * ro_frame_bins(d.grid), d.bins_part, d.bins_total);
  if (d.n_feat > 0) FU_LAUNCH(VSM_K_FU_SCATTER, k_fu_scatter, fu_grid_for(d.n_feat), d);
  FU_LAUNCH(VSM_K_FU_COUNT, k_fu_search<false>, fu_grid_for((int64_t)d.n_tracks * 16), d);
  vsm_tracks_launch_scan(s, pf, d.scan, d.n_tracks, d.scan_part, d.totals);
}

void vsm_fuse_launch_fuse(hipStream_t s, VsmProf &pf, const FuDevice &d, int32_t n_prop) {
  if (d.n_tracks <= 0 || d.n_frames <= 0) return;
  if (n_prop > 0) {
    if (d.slots)
      FU_LAUNCH(VSM_K_FU_COMPACT, k_fu_compact, fu_grid_for((int64_t)d.n_tracks * 16), d, n_prop);
    else
      FU_LAUNCH(VSM_K_FU_LIST, k_fu_search<true>, fu_grid_for((int64_t)d.n_tracks * 16), d);
    FU_LAUNCH(VSM_K_FU_CONFLICT, k_fu_conflict, (uint32_t)(((int64_t)n_prop + 15) / 16), d, n_prop);
    FU_LAUNCH(VSM_K_FU_VERDICT, k_fu_verdict, fu_grid_for(n_prop), d, n_prop);
  }
  FU_LAUNCH(VSM_K_FU_LENGTHS, k_fu_lengths, fu_grid_for(d.n_tracks), d);
  vsm_tracks_launch_scan(s, pf, d.scan, d.n_tracks, d.scan_part, d.totals);
  FU_LAUNCH(VSM_K_FU_MERGE, k_fu_merge, fu_grid_for((int64_t)d.n_tracks * 16), d);
}
