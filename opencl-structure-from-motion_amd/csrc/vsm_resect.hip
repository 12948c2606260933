// Pose refinement on the device (vsm_resect.h has the arithmetic, vsm_resect.inc the host side).
//
// One 256-thread workgroup per frame, the whole update loop inside the kernel.  Lane l walks the frame's rows l, l + 256, ..
// and keeps partial[l] of all 28 sums in registers; a row's point is gathered from the xyz table by its track index.  The
// tree of the definition runs through LDS across the four waves (s = 128: waves 2, 3 hand their partials to waves 0, 1;
// s = 64: wave 1 to wave 0) and by cross-lane moves inside wave 0 (s = 32 .. 1: lane l adds what lane l + s holds - the
// operand pair of the definition; x + y and y + x have the same bits, and what the lanes l >= s compute is never read).
// Lane 0 then holds the sums, solves the 6x6 system in LDS and moves the state, which all lanes read back from LDS.  The
// sequence of evaluations, updates and statuses is rs_frame's (vsm_resect.h), spelled out around the barriers.
// All control flow is uniform in the workgroup: every branch around a barrier depends on the frame, on LDS words written
// before the last barrier, or on the lane range alone, and the barriers stand outside the lane-range branches.  A frame
// without work (status 1..3) leaves before the first barrier.
#include "vsm_internal.h"
#include "vsm_resect.h"

namespace {

struct RsShared {
  double part[RS_SUMS * 128];  // the tree's hand-over: sum k of lane l at part[k * 128 + l]
  int32_t cnt[128];
  double state[12];            // [Rw | tw]
  double ab[42];               // the 6x6 system and its right-hand side
  int32_t result;              // lane 0's verdict after an evaluation: RS_UPDATED, or the status that ends the loop
};

// a double that is the same in every lane of the wave, as the compiler may keep it: in a pair of scalar registers
__device__ inline double rs_uniform(double x) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(x)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(x));
  return __hiloint2double(hi, lo);
}

// One evaluation: lane 0 returns with the sums and the count, the other lanes with partial results of no meaning.
// Without the Jacobian only sum 27 and the count are formed (N = 1: acc[0] is sum 27).
template <bool kJacobian>
__device__ inline void rs_evaluate(const RsDevice &d, const RsRow *rows, int32_t n, RsShared &sh, double *acc, int32_t &count) {
  constexpr int N = kJacobian ? RS_SUMS : 1;
  const int lane = threadIdx.x;
  const double limit = rs_limit(d.prm.max_residual);
  double S[12];  // the same twelve numbers in every lane: kept in scalar registers, the accumulators need the vector ones
  for (int i = 0; i < 12; i++) S[i] = rs_uniform(sh.state[i]);
  for (int k = 0; k < N; k++) acc[k] = 0.0;
  count = 0;
  for (int32_t i = lane; i < n; i += RS_LANES) {
    const RsRow row = rows[i];
    const double *X = d.xyz + 3 * (size_t)row.track;
    const double P[3] = {X[0], X[1], X[2]};
    double xc[3], r[2], t;
    if (rs_row(S, P, row.u, row.v, d.f, d.cu, d.cv, d.prm.min_depth, limit, xc, r, &t)) {
      count++;
      if (kJacobian) {
        double ju[6], jv[6];
        rs_jacobian(xc, d.f, ju, jv);
        rs_add_row(acc, ju, jv, r, t);
      } else {
        acc[0] += t;
      }
    }
  }
  // s = 128
  if (lane >= 128) {
    for (int k = 0; k < N; k++) sh.part[k * 128 + lane - 128] = acc[k];
    sh.cnt[lane - 128] = count;
  }
  __syncthreads();
  if (lane < 128) {
    for (int k = 0; k < N; k++) acc[k] += sh.part[k * 128 + lane];
    count += sh.cnt[lane];
  }
  __syncthreads();
  // s = 64
  if (lane >= 64 && lane < 128) {
    for (int k = 0; k < N; k++) sh.part[k * 128 + lane - 64] = acc[k];
    sh.cnt[lane - 64] = count;
  }
  __syncthreads();
  // s = 32 .. 1, inside wave 0
  if (lane < 64) {
    for (int k = 0; k < N; k++) acc[k] += sh.part[k * 128 + lane];
    count += sh.cnt[lane];
    for (int s = 32; s >= 1; s >>= 1) {
      for (int k = 0; k < N; k++) acc[k] += __shfl_down(acc[k], s, 64);
      count += __shfl_down(count, s, 64);
    }
  }
}

__global__ __launch_bounds__(RS_LANES) void k_rs_resect(RsDevice d) {
  __shared__ RsShared sh;
  const int32_t g = blockIdx.x;
  const int lane = threadIdx.x;
  const int32_t o = d.row_off[g], n = d.row_off[g + 1] - o;
  const RsRow *rows = d.rows + o;
  const double *pose = d.poses + 12 * (size_t)g;
  double *out = d.out_poses + 12 * (size_t)g;
  const int32_t early = rs_early_status(d.valid[g], d.refine[g], n, d.prm.min_observations);
  if (early != 0) {  // the whole workgroup
    if (lane < 12) out[lane] = pose[lane];
    if (lane == 0) {
      d.status[g] = early;
      d.updates[g] = 0;
      d.used_before[g] = 0;
      d.used[g] = 0;
      d.ss_before[g] = 0.0;
      d.ss_after[g] = 0.0;
    }
    return;
  }
  if (lane == 0) pts_rigid_inverse(pose, sh.state);
  __syncthreads();
  RsResult res = {6, 0, 0, 0, 0.0, 0.0};  // (lane 0's copy is the one that counts)
  double acc[RS_SUMS];
  int32_t count;
  for (int32_t it = 0; it < d.prm.max_updates; it++) {
    rs_evaluate<true>(d, rows, n, sh, acc, count);
    if (lane == 0) {
      if (res.updates == 0) {
        res.ss_before = acc[27];
        res.used_before = count;
      }
      res.used = count;
      int result = RS_UPDATED;
      if (count < d.prm.min_observations) {
        result = 4;
      } else {
        const int r = rs_step(acc, sh.ab, sh.state, d.prm.eps);
        if (r != RS_NO_PIVOT) res.updates++;
        result = r;
      }
      if (result != RS_UPDATED) res.status = result;
      sh.result = result;
    }
    __syncthreads();  // the state and the verdict are in place; the tree's hand-over block is free again
    if (sh.result != RS_UPDATED) break;
  }
  // (no barrier between the last read of sh.result and its next write: a status ends the loop, so there is none)
  const bool moved = sh.result == RS_UPDATED || sh.result == RS_CONVERGED;  // status 6 or 0: the final evaluation
  if (moved) {
    rs_evaluate<false>(d, rows, n, sh, acc, count);
    if (lane == 0) {
      res.ss_after = acc[0];
      res.used = count;
    }
  }
  if (lane == 0) {
    if (moved)
      pts_rigid_inverse(sh.state, out);
    else
      for (int i = 0; i < 12; i++) out[i] = pose[i];
    d.status[g] = res.status;
    d.updates[g] = res.updates;
    d.used_before[g] = res.used_before;
    d.used[g] = res.used;
    d.ss_before[g] = res.ss_before;
    d.ss_after[g] = res.ss_after;
  }
}

}  // namespace

void vsm_resect_launch(hipStream_t s, VsmProf &pf, const RsDevice &d) {
  if (d.n_frames <= 0) return;
  pf.begin(VSM_K_RS_RESECT, s);
  hipLaunchKernelGGL(k_rs_resect, dim3(d.n_frames), dim3(RS_LANES), 0, s, d);
  pf.end(s);
}
