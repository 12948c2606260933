// Vetting of observations on the device (vsm_vet.h has the arithmetic, vsm_vet.inc the host side).
//
// The mapping of k_pts_triangulate: a 16-lane group per track, four tracks per wave, sixteen per 256-thread workgroup.
// k_vet_obs: lane l of the group takes observation 16 c + l for chunk after chunk c, writes its code and r2, counts it
// for its frame with an integer atomic and keeps partial[l] of the track - the definition's 16 partial sums are the
// group's lanes.  The tree runs through cross-lane moves of width 16 (s = 8 .. 1: lane l adds what lane l + s holds; x + y
// and y + x have the same bits, and what the lanes l >= s compute is never read).  Lane 0 writes the track's results and
// the scan's input, (1, n_in) for a kept track and (0, 0) otherwise.  The scan is the multi-level one of vsm_tracks.hip.
// k_vet_emit: the same groups once more; a kept inlier's place is the track's offset plus its rank among the track's
// inliers, a ballot over the group's sixteen lanes and a count of the bits below the lane's own.
// All control flow is uniform inside a group, nothing goes through LDS and there is no barrier: a group that is done
// leaves.  The groups of a wave differ in their trip counts only.
#include "vsm_internal.h"
#include "vsm_tracks.h"
#include "vsm_vet.h"

namespace {

// the ballot's bits of the lane's own group
__device__ inline uint32_t vet_group_ballot(bool pred) {
  const unsigned long long all = __ballot(pred);
  return (uint32_t)(all >> (threadIdx.x & 48)) & 0xffffu;
}

__global__ __launch_bounds__(256) void k_vet_obs(VetDevice d) {
  const int grp = threadIdx.x >> 4, ln = threadIdx.x & 15;
  const int64_t t = (int64_t)blockIdx.x * 16 + grp;
  if (t >= d.n_tracks) return;  // whole groups leave together
  const int32_t o = d.offsets[t], n = d.offsets[t + 1] - o;
  const int in_use = d.use[t];
  const double X[3] = {d.xyz[3 * t + 0], d.xyz[3 * t + 1], d.xyz[3 * t + 2]};
  const double limit = rs_limit(d.prm.max_residual);
  VetAcc acc;
  vet_acc_init(&acc);
  for (int32_t c0 = 0; c0 < n; c0 += VET_LANES) {
    const int32_t k = c0 + ln;
    if (k < n) {
      const size_t i = (size_t)o + k;
      const int32_t g = d.obs_frames[i];
      double tt = 0.0;
      const int32_t c = vet_obs(d.states + 12 * (size_t)g, X, d.uv[2 * i], d.uv[2 * i + 1], in_use, d.valid[g], d.f, d.cu, d.cv, d.prm.min_depth, limit, &tt);
      d.code[i] = (uint8_t)c;
      d.r2[i] = vet_r2(c, tt);
      if (c == VET_INLIER) {
        vet_acc_add(&acc, g, tt);
        atomicAdd(d.frame_counts + 3 * (size_t)g, 1);
      } else if (c == VET_BEHIND) {
        atomicAdd(d.frame_counts + 3 * (size_t)g + 1, 1);
      } else if (c == VET_GATED) {
        atomicAdd(d.frame_counts + 3 * (size_t)g + 2, 1);
      }
    }
  }
  for (int s = VET_LANES / 2; s >= 1; s >>= 1) {
    const double ss = __shfl_down(acc.ss, s, VET_LANES), worst = __shfl_down(acc.worst, s, VET_LANES);
    const int32_t n_in = __shfl_down(acc.n_in, s, VET_LANES), lo = __shfl_down(acc.lo, s, VET_LANES), hi = __shfl_down(acc.hi, s, VET_LANES);
    vet_acc_merge(&acc, ss, worst, n_in, lo, hi);
  }
  if (ln == 0) {
    const int32_t st = vet_track_status(in_use, acc, d.prm.min_observations);
    d.status[t] = st;
    d.n_in[t] = acc.n_in;
    d.frame_lo[t] = vet_frame_lo(acc);
    d.frame_hi[t] = acc.hi;
    d.ss[t] = acc.ss;
    d.worst[t] = acc.worst;
    const int32_t len = vet_kept_length(st, acc.n_in);
    ((int2 *)d.scan)[t] = make_int2(len > 0 ? 1 : 0, len);
  }
}

__global__ __launch_bounds__(256) void k_vet_emit(VetDevice d) {
  const int grp = threadIdx.x >> 4, ln = threadIdx.x & 15;
  const int64_t t = (int64_t)blockIdx.x * 16 + grp;
  if (t >= d.n_tracks) return;
  const int32_t at = d.scan[2 * t + 1];  // the kept observations in front of this track
  if (ln == 0) {
    d.kept_offsets[t] = at;
    if (t == 0) d.kept_offsets[d.n_tracks] = d.totals[1];
  }
  if (d.status[t] != 0) return;
  const int32_t o = d.offsets[t], n = d.offsets[t + 1] - o;
  int32_t rank = at;
  for (int32_t c0 = 0; c0 < n; c0 += VET_LANES) {
    const int32_t k = c0 + ln;
    const bool inl = k < n && d.code[(size_t)o + k] == VET_INLIER;
    const uint32_t m = vet_group_ballot(inl);
    if (inl) d.kept_index[rank + __popc(m & ((1u << ln) - 1u))] = o + k;
    rank += __popc(m);
  }
}

}  // namespace

void vsm_vet_launch(hipStream_t s, VsmProf &pf, const VetDevice &d) {
  if (d.n_tracks <= 0) return;
  const int grid = (d.n_tracks + 15) / 16;
  pf.begin(VSM_K_VET_OBS, s);
  hipLaunchKernelGGL(k_vet_obs, dim3(grid), dim3(256), 0, s, d);
  pf.end(s);
  vsm_tracks_launch_scan(s, pf, d.scan, d.n_tracks, d.scan_part, d.totals);
  pf.begin(VSM_K_VET_EMIT, s);
  hipLaunchKernelGGL(k_vet_emit, dim3(grid), dim3(256), 0, s, d);
  pf.end(s);
}
