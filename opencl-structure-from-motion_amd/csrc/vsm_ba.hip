// Joint adjustment of poses and points on the device (vsm_ba.h has the arithmetic and the schedule, vsm_ba.inc the host side).
//
// Three shapes of kernel, each a step of ba_schedule:
//  - by frame, a 256-thread workgroup per frame with k_rs_resect's layout: lane l walks the frame's rows l, l + 256, .. and
//    keeps partial[l] of the step's sums in registers; the tree of the definition runs through LDS (s = 128: the upper half
//    hands its partials over; s = 64 .. 1 in place), lane 0 finishes the frame (k_ba_linearise, k_ba_frames<>, k_ba_trial_cost);
//  - by track, one lane per track walking the track's observations in ascending order (k_ba_tracks, k_ba_op_tracks, k_ba_back);
//  - one workgroup for the conjugate gradient's vectors and scalars and for the decision (k_ba_cg_init, k_ba_cg_step,
//    k_ba_decide): a lane per frame for the vectors, the scalar products by the 256 partial sums and the tree.
// No atomics on doubles, no cooperative launch, no graph: the stream's order is the only synchronisation between kernels.
// Every kernel reads the control block first and returns when the call, or the round's solve, is over; the flags are
// uniform in the grid, so all barriers stay in uniform control flow.  All indices are bounded by the counts the host packed:
// a row's track < n_tracks and obs < n_obs by construction (rs_group_fill), an observation's frame < n_frames by the argument
// checks.
#include "vsm_internal.h"
#include "vsm_ba.h"

namespace {

// The tree over K sums: every lane comes with its partial sums in acc, lane 0 leaves with the sums.  part: K * 128 doubles.
template <int K>
__device__ inline void ba_tree(double *acc, double *part) {
  const int lane = threadIdx.x;
  if (lane >= 128)
    for (int k = 0; k < K; k++) part[k * 128 + lane - 128] = acc[k];
  __syncthreads();
  if (lane < 128)
    for (int k = 0; k < K; k++) {
      acc[k] += part[k * 128 + lane];
      part[k * 128 + lane] = acc[k];
    }
  __syncthreads();
  for (int s = 64; s >= 1; s >>= 1) {
    if (lane < s)
      for (int k = 0; k < K; k++) part[k * 128 + lane] += part[k * 128 + lane + s];
    __syncthreads();
  }
  if (lane == 0)
    for (int k = 0; k < K; k++) acc[k] = part[k * 128];
  __syncthreads();  // (the block is free again)
}

__global__ __launch_bounds__(RS_LANES) void k_ba_init(BaData d) {
  const int32_t i = blockIdx.x * RS_LANES + threadIdx.x;
  if (i == 0) ba_ctl_init(d);
  if (i < d.n_frames) ba_init_frame(d, i);
  if (i < d.n_tracks)
    for (int a = 0; a < 3; a++) d.out_xyz[3 * (size_t)i + a] = d.xyz_in[3 * (size_t)i + a];
}

__global__ __launch_bounds__(RS_LANES) void k_ba_linearise(BaData d) {
  __shared__ double part[RS_SUMS * 128];
  __shared__ int32_t cnt;
  if (d.ctl->done) return;
  const int32_t g = blockIdx.x;
  const int lane = threadIdx.x;
  const int32_t o = d.row_off[g], n = d.row_off[g + 1] - o;
  const BaRow *rows = d.rows + o;
  double acc[RS_SUMS];
  for (int k = 0; k < RS_SUMS; k++) acc[k] = 0.0;
  int32_t count = 0;
  if (lane == 0) cnt = 0;
  __syncthreads();
  if (d.valid[g]) {  // the whole workgroup
    const double limit = rs_limit(d.prm.max_residual);
    double S[12];
    for (int i = 0; i < 12; i++) S[i] = d.state[12 * (size_t)g + i];
    for (int32_t i = lane; i < n; i += RS_LANES) ba_lin_row(d, S, rows[i], limit, acc, count);
  } else {
    for (int32_t i = lane; i < n; i += RS_LANES) d.active[rows[i].obs] = 0;
  }
  if (count) atomicAdd(&cnt, count);
  ba_tree<RS_SUMS>(acc, part);
  if (lane == 0) ba_lin_frame_end(d, g, acc, cnt);
}

__global__ __launch_bounds__(RS_LANES) void k_ba_tracks(BaData d) {
  if (d.ctl->done) return;
  const int32_t t = blockIdx.x * RS_LANES + threadIdx.x;
  if (t < d.n_tracks) ba_track_system(d, t);
}

// the by-frame gather of W zt: the right-hand side (kRhs, every frame) or the operator's second half (free frames)
template <bool kRhs>
__global__ __launch_bounds__(RS_LANES) void k_ba_frames(BaData d) {
  __shared__ double part[6 * 128];
  if (d.ctl->done || (!kRhs && d.ctl->cg_done)) return;
  const int32_t g = blockIdx.x;
  if (!kRhs && !d.ffree[g]) return;  // the whole workgroup
  const int lane = threadIdx.x;
  const int32_t o = d.row_off[g], n = d.row_off[g + 1] - o;
  const BaRow *rows = d.rows + o;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int32_t i = lane; i < n; i += RS_LANES) ba_wz_row(d, rows[i], acc);
  ba_tree<6>(acc, part);
  if (lane == 0) {
    if (kRhs) {
      double ab[42];
      ba_rhs_frame_end(d, g, acc, ab);
    } else {
      ba_op_frame_end(d, g, acc);
    }
  }
}

// a . b over the 6 F entries: every lane calls, lane 0 returns with the sum
__device__ inline double ba_dot(const BaData &d, const double *a, const double *b, double *part) {
  double s = ba_dot_partial(d, a, b, threadIdx.x);
  ba_tree<1>(&s, part);
  return s;
}

__global__ __launch_bounds__(RS_LANES) void k_ba_cg_init(BaData d) {
  __shared__ double part[128];
  if (d.ctl->done) return;
  for (int32_t g = threadIdx.x; g < d.n_frames; g += RS_LANES) ba_cg_frame_init(d, g);
  __syncthreads();
  const double rz = ba_dot(d, d.r, d.z, part);
  if (threadIdx.x == 0) ba_cg_begin(d, rz);
}

__global__ __launch_bounds__(RS_LANES) void k_ba_op_tracks(BaData d) {
  if (d.ctl->done || d.ctl->cg_done) return;
  const int32_t t = blockIdx.x * RS_LANES + threadIdx.x;
  if (t < d.n_tracks) ba_op_track(d, t);
}

__global__ __launch_bounds__(RS_LANES) void k_ba_cg_step(BaData d) {
  __shared__ double part[128];
  __shared__ int go;
  if (d.ctl->done || d.ctl->cg_done) return;
  const double pq = ba_dot(d, d.p, d.q, part);
  if (threadIdx.x == 0) go = ba_cg_alpha(d, pq) ? 1 : 0;
  __syncthreads();  // (the control block's alpha is lane 0's write: in place for the workgroup behind the barrier)
  if (!go) return;
  const double alpha = d.ctl->alpha;
  for (int32_t g = threadIdx.x; g < d.n_frames; g += RS_LANES) ba_cg_frame_move(d, g, alpha);
  __syncthreads();
  const double rz = ba_dot(d, d.r, d.z, part);
  if (threadIdx.x == 0) go = ba_cg_beta(d, rz) ? 1 : 0;
  __syncthreads();
  if (!go) return;
  const double beta = d.ctl->beta;
  for (int32_t g = threadIdx.x; g < d.n_frames; g += RS_LANES) ba_cg_frame_direction(d, g, beta);
}

__global__ __launch_bounds__(RS_LANES) void k_ba_back(BaData d) {
  if (d.ctl->done) return;
  const int32_t i = blockIdx.x * RS_LANES + threadIdx.x;
  if (i < d.n_tracks) ba_back_track(d, i);
  if (i < d.n_frames) ba_trial_frame(d, i);
}

__global__ __launch_bounds__(RS_LANES) void k_ba_trial_cost(BaData d) {
  __shared__ double part[128];
  __shared__ int32_t any_behind;
  if (d.ctl->done) return;
  const int32_t g = blockIdx.x;
  const int lane = threadIdx.x;
  const int32_t o = d.row_off[g], n = d.row_off[g + 1] - o;
  const BaRow *rows = d.rows + o;
  double acc = 0.0;
  int32_t behind = 0;
  if (lane == 0) any_behind = 0;
  __syncthreads();
  if (d.valid[g]) {  // the whole workgroup
    double S[12];
    for (int i = 0; i < 12; i++) S[i] = d.trial_state[12 * (size_t)g + i];
    for (int32_t i = lane; i < n; i += RS_LANES) ba_trial_row(d, S, rows[i], acc, behind);
  }
  if (behind) atomicOr(&any_behind, 1);
  ba_tree<1>(&acc, part);
  if (lane == 0) {
    d.tcost[g] = acc;
    d.tbehind[g] = any_behind;
  }
}

__global__ void k_ba_decide(BaData d) {
  if (d.ctl->done) return;
  ba_decide(d);
}

__global__ __launch_bounds__(RS_LANES) void k_ba_commit(BaData d, int32_t round) {
  if (!ba_commits(d, round)) return;
  const int32_t i = blockIdx.x * RS_LANES + threadIdx.x;
  if (i < d.n_frames) ba_commit_frame(d, i);
  if (i < d.n_tracks) ba_commit_track(d, i);
}

__global__ __launch_bounds__(RS_LANES) void k_ba_finish(BaData d) {
  const int32_t g = blockIdx.x * RS_LANES + threadIdx.x;
  if (g < d.n_frames) ba_finish_frame(d, g);
}

// ba_schedule's steps as launches on one stream
struct DeviceOps {
  hipStream_t s;
  VsmProf &pf;
  const BaData &d;
  BaCtl *ctl_host;
  bool fixed;
  hipError_t err = hipSuccess;
  dim3 by_frame, by_track, by_both, by_frames_flat;

  DeviceOps(hipStream_t stream, VsmProf &prof, const BaData &data, BaCtl *ctl_h, bool fixed_schedule) : s(stream), pf(prof), d(data), ctl_host(ctl_h), fixed(fixed_schedule) {
    const auto blocks = [](int32_t n) { return dim3((unsigned)((n + RS_LANES - 1) / RS_LANES)); };
    by_frame = dim3((unsigned)d.n_frames);
    by_track = blocks(d.n_tracks);
    by_both = blocks(d.n_tracks > d.n_frames ? d.n_tracks : d.n_frames);
    by_frames_flat = blocks(d.n_frames);
  }
  template <class K, class... A>
  void launch(int id, K kernel, dim3 grid, dim3 block, A... args) {
    if (grid.x == 0 || err != hipSuccess) return;
    pf.begin(id, s);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
    pf.end(s);
  }
  void init() { launch(VSM_K_BA_INIT, k_ba_init, dim3(by_both.x ? by_both.x : 1), dim3(RS_LANES), d); }
  void linearise() { launch(VSM_K_BA_LINEARISE, k_ba_linearise, by_frame, dim3(RS_LANES), d); }
  void tracks() { launch(VSM_K_BA_TRACKS, k_ba_tracks, by_track, dim3(RS_LANES), d); }
  void rhs() { launch(VSM_K_BA_RHS, k_ba_frames<true>, by_frame, dim3(RS_LANES), d); }
  void cg_init() { launch(VSM_K_BA_CG_INIT, k_ba_cg_init, dim3(1), dim3(RS_LANES), d); }
  void op_tracks() { launch(VSM_K_BA_OP_TRACKS, k_ba_op_tracks, by_track, dim3(RS_LANES), d); }
  void op_frames() { launch(VSM_K_BA_OP_FRAMES, k_ba_frames<false>, by_frame, dim3(RS_LANES), d); }
  void cg_step() { launch(VSM_K_BA_CG_STEP, k_ba_cg_step, dim3(1), dim3(RS_LANES), d); }
  void back() { launch(VSM_K_BA_BACK, k_ba_back, by_both, dim3(RS_LANES), d); }
  void trial_cost() { launch(VSM_K_BA_TRIAL_COST, k_ba_trial_cost, by_frame, dim3(RS_LANES), d); }
  void decide() { launch(VSM_K_BA_DECIDE, k_ba_decide, dim3(1), dim3(1), d); }
  void commit(int32_t k) { launch(VSM_K_BA_COMMIT, k_ba_commit, by_both, dim3(RS_LANES), d, k); }
  void finish() { launch(VSM_K_BA_FINISH, k_ba_finish, by_frames_flat, dim3(RS_LANES), d); }
  bool solve_over() const { return false; }  // (the solve's launches are enqueued without looking)
  // the wait per round: the control block comes back, and a call that has stopped enqueues no further round
  bool round_over(int32_t k) {
    if (fixed || err != hipSuccess || k + 1 >= d.prm.max_rounds) return err != hipSuccess;
    err = hipMemcpyAsync(ctl_host, d.ctl, sizeof(BaCtl), hipMemcpyDeviceToHost, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    return err != hipSuccess || ctl_host->done != 0;
  }
};

}  // namespace

hipError_t vsm_ba_launch(hipStream_t s, VsmProf &pf, const BaData &d, BaCtl *ctl_host, bool fixed_schedule) {
  DeviceOps o(s, pf, d, ctl_host, fixed_schedule);
  ba_schedule(o, d.prm);
  return o.err;
}
