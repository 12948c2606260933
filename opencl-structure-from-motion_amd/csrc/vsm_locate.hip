// Location of frames against the points on the device (vsm_locate.h has the arithmetic, vsm_locate.inc the host side).
//
// A job is a frame that is asked for and has at least min_inliers eligible rows; K = ransac_iters hypotheses per job.
//   k_locate_fit     one 16-lane group per (job, hypothesis), 16 groups per 256-thread block - a block may span two jobs.
//                    The group's matrices live in LDS (LC_GROUP_DOUBLES doubles): lanes 0..5 fetch the six sampled rows and
//                    their points, every lane forms the mean and the scale (the same operands in the same order, hence the
//                    same bits), lanes 0..5 write two rows of the 12 x 12 matrix each, the group runs svd_group<12, 12>, then
//                    svd_group<3, 3> on the left block of the last column of V, and lane 0 forms the state and its validity.
//   k_locate_count   blockIdx.x = a tile of 256 rows of one job (the host's table: unequal frames cost no empty blocks),
//                    blockIdx.y = a run of `hyps` hypotheses.  A lane keeps its row and point in registers, the state is
//                    the same for the whole block; ballot and popcount, one integer atomic per wave and hypothesis.
//   k_locate_winner  one block per frame: the maximum of (count << 32 | ~k) - the largest count at the smallest k -, whether
//                    any hypothesis was valid, the verdict, and the winner's state inverted to a pose where the resection's
//                    kernel reads it.
// No floating-point atomic; the counts are integer sums, which have no order.
#include "vsm_internal.h"
#include "vsm_locate.h"
#include "vsm_svd_coop.h"

namespace {

__global__ void __launch_bounds__(256) k_locate_fit(LcDevice d) {
  __shared__ double s_m[16 * LC_GROUP_DOUBLES];
  const int grp = threadIdx.x >> 4, ln = threadIdx.x & 15;
  const int K = d.prm.ransac_iters;
  const size_t g = (size_t)blockIdx.x * 16 + grp;
  if (g >= (size_t)d.n_jobs * K) return;  // whole groups leave together
  const int32_t j = (int32_t)(g / K);
  if (d.job_E[j] == 0) return;  // a frame with too few eligible rows: no hypotheses
  const RsRow *rows = d.rows + d.row_off[d.job_frame[j]];
  const int32_t *pick = d.picks + g * LC_SAMPLE;
  volatile double *A = s_m + grp * LC_GROUP_DOUBLES;
  volatile double *U = A + LC_U, *V = A + LC_V, *W = A + LC_W, *RV = A + LC_RV;
  // the six rows: lane i fetches sample i and shows its point to the group (V is free until the decomposition clears it)
  RsRow row = {0, 0.f, 0.f};
  double Xl[3] = {0.0, 0.0, 0.0};
  if (ln < LC_SAMPLE) {
    row = rows[pick[ln]];
    const double *X = d.xyz + 3 * (size_t)row.track;
    for (int c = 0; c < 3; c++) V[3 * ln + c] = Xl[c] = X[c];
  }
  VSM_GROUP_SYNC();
  double P[3 * LC_SAMPLE], m[3], s;
  for (int i = 0; i < 3 * LC_SAMPLE; i++) P[i] = V[i];
  const bool conditioned = lc_condition(P, m, &s);  // (the same in all sixteen lanes)
  if (!conditioned) {
    if (ln == 0) d.hvalid[g] = 0;
    return;
  }
  if (ln < LC_SAMPLE) lc_rows(U, ln, row.u, row.v, Xl, m, s, d.f, d.cu, d.cv);  // all 144 entries, the zeros too
  VSM_GROUP_SYNC();
  vsm_la::svd_group<LC_N, LC_N>(U, V, W, RV, ln);
  // p = the last column of V; its left block goes through the same group decomposition
  double pl = 0;
  if (ln < LC_N) pl = V[ln * LC_N + (LC_N - 1)];
  VSM_GROUP_SYNC();
  volatile double *U3 = A + LC_U3, *V3 = A + LC_V3, *W3 = A + LC_W3, *R3 = A + LC_RV3, *p = A + LC_P;
  if (ln < LC_N) {
    p[ln] = pl;
    if ((ln & 3) != 3) U3[3 * (ln >> 2) + (ln & 3)] = pl;
  }
  VSM_GROUP_SYNC();
  vsm_la::svd_group<3, 3>(U3, V3, W3, R3, ln);
  if (ln == 0) {
    double S[12];
    bool ok = lc_state(p, U3, W3, V3, m, s, S);
    for (int i = 0; i < LC_SAMPLE; i++) ok = ok && lc_in_front(S, P + 3 * i, d.prm.min_depth);
    double *out = d.states + g * 12;
    for (int i = 0; i < 12; i++) out[i] = S[i];
    d.hvalid[g] = ok ? 1 : 0;
  }
}

__global__ void __launch_bounds__(256) k_locate_count(LcDevice d, int hyps) {
  const LcTile t = d.tiles[blockIdx.x];
  const int32_t o = d.row_off[d.job_frame[t.job]], n = d.row_off[d.job_frame[t.job] + 1] - o;
  if (t.off + (int)(threadIdx.x & ~63u) >= n) return;  // a whole wave past the frame's end
  const int i = t.off + threadIdx.x;
  const bool live = i < n;
  const RsRow row = d.rows[o + (live ? i : 0)];
  const double *Xp = d.xyz + 3 * (size_t)row.track;
  const double X[3] = {Xp[0], Xp[1], Xp[2]};
  const bool eligible = live && lc_eligible(row.u, row.v, X);
  const double limit = rs_limit(d.prm.inlier_threshold);
  const int K = d.prm.ransac_iters;
  const int k0 = blockIdx.y * hyps, k1 = min(K, k0 + hyps);
  for (int k = k0; k < k1; k++) {
    const size_t g = (size_t)t.job * K + k;
    if (!d.hvalid[g]) continue;  // (uniform: an invalid hypothesis counts 0)
    const double *S = d.states + g * 12;
    const bool in = eligible && lc_inlier(S, X, row.u, row.v, d.f, d.cu, d.cv, d.prm.min_depth, limit);
    const unsigned long long b = __ballot(in);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&d.counts[g], (int32_t)__popcll(b));
  }
}

__global__ void __launch_bounds__(256) k_locate_winner(LcDevice d) {
  __shared__ unsigned long long s_key[4];
  __shared__ int32_t s_any[4];
  const int32_t fr = blockIdx.x, j = d.frame_job[fr];
  double *lin = d.lin_poses + 12 * (size_t)fr;
  if (j < 0 || d.job_E[j] == 0) {  // the whole block: status 1 or 2, the host knows which
    if (threadIdx.x < 12) lin[threadIdx.x] = 0.0;
    if (threadIdx.x == 0) {
      d.verdict[fr] = -1;
      d.best[fr] = -1;
      d.inliers[fr] = 0;
      d.lin_valid[fr] = 0;
    }
    return;
  }
  const int K = d.prm.ransac_iters;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long key = 0;  // count << 32 | ~k: the maximum is the largest count at the smallest k
  int32_t any = 0;
  for (int k = threadIdx.x; k < K; k += 256) {
    const size_t g = (size_t)j * K + k;
    if (!d.hvalid[g]) continue;
    any = 1;
    const unsigned long long c = (unsigned long long)(uint32_t)d.counts[g];
    const unsigned long long v = (c << 32) | (uint32_t)(0xffffffffu - (uint32_t)k);
    key = v > key ? v : key;
  }
  for (int s = 32; s > 0; s >>= 1) {
    const unsigned long long o = __shfl_xor(key, s);
    key = o > key ? o : key;
  }
  const unsigned long long anyb = __ballot(any != 0);
  if (lane == 0) {
    s_key[wave] = key;
    s_any[wave] = anyb ? 1 : 0;
  }
  __syncthreads();
  key = s_key[0];
  for (int w = 1; w < 4; w++) key = s_key[w] > key ? s_key[w] : key;
  const bool any_valid = (s_any[0] | s_any[1] | s_any[2] | s_any[3]) != 0;
  const int32_t count = (int32_t)(key >> 32);
  const int32_t bestk = count ? (int32_t)(0xffffffffu - (uint32_t)key) : -1;
  if (threadIdx.x == 0) {
    const int32_t verdict = lc_verdict(any_valid, count, d.prm.min_inliers);
    if (bestk >= 0) {
      pts_rigid_inverse(d.states + ((size_t)j * K + bestk) * 12, lin);
    } else {
      for (int i = 0; i < 12; i++) lin[i] = 0.0;
    }
    d.verdict[fr] = verdict;
    d.best[fr] = bestk;
    d.inliers[fr] = count;
    d.lin_valid[fr] = verdict == 0 ? 1 : 0;
  }
}

}  // namespace

void vsm_locate_launch(hipStream_t s, VsmProf &pf, const LcDevice &d) {
  if (d.n_frames <= 0) return;
  const int K = d.prm.ransac_iters;
  const size_t total = (size_t)d.n_jobs * K;
  if (total > 0) {
    pf.begin(VSM_K_LC_FIT, s);
    hipLaunchKernelGGL(k_locate_fit, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, s, d);
    pf.end(s);
  }
  if (d.n_tiles > 0) {
    const int hyps = std::max(16, (K + 65534) / 65535);
    pf.begin(VSM_K_LC_COUNT, s);
    hipLaunchKernelGGL(k_locate_count, dim3((unsigned)d.n_tiles, (unsigned)((K + hyps - 1) / hyps)), dim3(256), 0, s, d, hyps);
    pf.end(s);
  }
  pf.begin(VSM_K_LC_WINNER, s);
  hipLaunchKernelGGL(k_locate_winner, dim3((unsigned)d.n_frames), dim3(256), 0, s, d);
  pf.end(s);
}
