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
// No floating-point atomic; the counts are integer sums, which have no order.  k_locate_count only adds: whoever launches it
// clears the counts first (vsm_locate.inc before the call's launches, vsm_debug_locate_count before its own).
// Behind the kernels: the three launches, stated once, and the test hooks that run one of them alone (include/visomatch.h).
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

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

// the three launches: their geometry is stated here once, for the call and for the test hooks below
static void launch_fit(hipStream_t s, const LcDevice &d) {
  const size_t total = (size_t)d.n_jobs * d.prm.ransac_iters;
  hipLaunchKernelGGL(k_locate_fit, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, s, d);
}
static void launch_count(hipStream_t s, const LcDevice &d) {
  const int K = d.prm.ransac_iters;
  const int hyps = std::max(16, (K + 65534) / 65535);
  hipLaunchKernelGGL(k_locate_count, dim3((unsigned)d.n_tiles, (unsigned)((K + hyps - 1) / hyps)), dim3(256), 0, s, d, hyps);
}
static void launch_winner(hipStream_t s, const LcDevice &d) { hipLaunchKernelGGL(k_locate_winner, dim3((unsigned)d.n_frames), dim3(256), 0, s, d); }

void vsm_locate_launch(hipStream_t s, VsmProf &pf, const LcDevice &d) {
  if (d.n_frames <= 0) return;
  if ((size_t)d.n_jobs * d.prm.ransac_iters > 0) {
    pf.begin(VSM_K_LC_FIT, s);
    launch_fit(s, d);
    pf.end(s);
  }
  if (d.n_tiles > 0) {
    pf.begin(VSM_K_LC_COUNT, s);
    launch_count(s, d);
    pf.end(s);
  }
  pf.begin(VSM_K_LC_WINNER, s);
  launch_winner(s, d);
  pf.end(s);
}

// ---- test hooks (include/visomatch.h, the debug section): ONE kernel each on plain device allocations, through the launch
// functions above and an LcDevice filled by hand.  Every argument is checked before the device is touched: a pick, a job's
// frame or a frame's job outside its table would be a read out of bounds on the device.
#define HIPCHK(expr)                                                                                                           \
  do {                                                                                                                         \
    const hipError_t e_ = (expr);                                                                                              \
    if (e_ != hipSuccess) {                                                                                                    \
      fprintf(stderr, "visomatch: HIP error %s at %s:%d (%s)\n", hipGetErrorString(e_), __FILE__, __LINE__, #expr);            \
      (void)hipGetLastError();                                                                                                 \
      return VSM_EHIP;                                                                                                         \
    }                                                                                                                          \
  } while (0)

namespace {

enum { LC_DEBUG_MAX_HYPOTHESES = 1 << 22 };  // jobs x hypotheses of one hook call

// a device array of n elements that goes when the hook returns, whichever way
template <typename T>
struct LcDebugDev {
  T *p = nullptr;
  size_t n = 0;
  LcDebugDev() = default;
  LcDebugDev(const LcDebugDev &) = delete;
  LcDebugDev &operator=(const LcDebugDev &) = delete;
  ~LcDebugDev() {
    if (p) (void)hipFree(p);
  }
  // the allocation, and the caller's content where there is some
  hipError_t put(const T *src, size_t count) {
    n = count;
    const hipError_t e = hipMalloc((void **)&p, std::max<size_t>(n, 1) * sizeof(T));
    if (e != hipSuccess || !src || n == 0) return e;
    return hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
  }
  hipError_t get(T *dst) const { return n ? hipMemcpy(dst, p, n * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess; }
};

// frames of rows as the hooks take them: row_off[F + 1], pixels [R][2] and a point per row [R][3]
bool debug_frames_ok(int32_t n_frames, const int32_t *row_off, const float *rows_uv, const double *rows_xyz) {
  if (n_frames < 1 || !row_off || row_off[0] != 0) return false;
  for (int32_t g = 0; g < n_frames; g++)
    if (row_off[g + 1] < row_off[g]) return false;
  return row_off[n_frames] == 0 || (rows_uv && rows_xyz);
}
// the job tables: every job a frame of the call, job_E between 0 and the frame's rows
bool debug_jobs_ok(int32_t n_frames, const int32_t *row_off, int32_t n_jobs, const int32_t *job_frame, const int32_t *job_E, int32_t K) {
  if (n_jobs < 1 || K < 1 || !job_frame || !job_E || (int64_t)n_jobs * K > LC_DEBUG_MAX_HYPOTHESES) return false;
  for (int32_t j = 0; j < n_jobs; j++) {
    if (job_frame[j] < 0 || job_frame[j] >= n_frames) return false;
    if (job_E[j] < 0 || job_E[j] > row_off[job_frame[j] + 1] - row_off[job_frame[j]]) return false;
  }
  return true;
}

// the frames on the device: row r is {track r, u, v}, its point xyz[r]
struct LcDebugFrames {
  LcDebugDev<int32_t> row_off, job_frame, job_E;
  LcDebugDev<RsRow> rows;
  LcDebugDev<double> xyz;
  hipError_t put(int32_t n_frames, const int32_t *off, const float *uv, const double *pts, int32_t n_jobs, const int32_t *jf, const int32_t *je, LcDevice &d) {
    const size_t R = (size_t)off[n_frames];
    std::vector<RsRow> table(R + 1);
    for (size_t r = 0; r < R; r++) table[r] = {(int32_t)r, uv[2 * r], uv[2 * r + 1]};
    hipError_t e = row_off.put(off, (size_t)n_frames + 1);
    if (e == hipSuccess) e = rows.put(table.data(), R);
    if (e == hipSuccess) e = xyz.put(pts, 3 * R);
    if (e == hipSuccess) e = job_frame.put(jf, (size_t)n_jobs);
    if (e == hipSuccess) e = job_E.put(je, (size_t)n_jobs);
    d.row_off = row_off.p, d.rows = rows.p, d.xyz = xyz.p, d.job_frame = job_frame.p, d.job_E = job_E.p;
    d.n_frames = n_frames, d.n_jobs = n_jobs;
    return e;
  }
};

}  // namespace

extern "C" {

int32_t vsm_debug_locate_fit(double f, double cu, double cv, double min_depth, int32_t n_frames, const int32_t *row_off, const float *rows_uv,
                             const double *rows_xyz, int32_t n_jobs, const int32_t *job_frame, const int32_t *job_E, const int32_t *picks, int32_t K,
                             double *states, uint8_t *hvalid) {
  if (!debug_frames_ok(n_frames, row_off, rows_uv, rows_xyz) || !debug_jobs_ok(n_frames, row_off, n_jobs, job_frame, job_E, K) || !picks || !states || !hvalid)
    return VSM_EARG;
  for (int32_t j = 0; j < n_jobs; j++) {
    const int32_t n = row_off[job_frame[j] + 1] - row_off[job_frame[j]];
    for (size_t i = (size_t)j * K * LC_SAMPLE; job_E[j] && i < ((size_t)j + 1) * K * LC_SAMPLE; i++)
      if (picks[i] < 0 || picks[i] >= n) return VSM_EARG;
  }
  const size_t JK = (size_t)n_jobs * K;
  LcDevice d;
  memset(&d, 0, sizeof(d));
  LcDebugFrames frames;
  LcDebugDev<int32_t> d_picks;
  LcDebugDev<double> d_states;
  LcDebugDev<uint8_t> d_hvalid;
  HIPCHK(frames.put(n_frames, row_off, rows_uv, rows_xyz, n_jobs, job_frame, job_E, d));
  HIPCHK(d_picks.put(picks, JK * LC_SAMPLE));
  HIPCHK(d_states.put(states, JK * 12));  // (the caller's content: what the kernel leaves alone comes back as it was)
  HIPCHK(d_hvalid.put(hvalid, JK));
  d.picks = d_picks.p, d.states = d_states.p, d.hvalid = d_hvalid.p;
  d.f = f, d.cu = cu, d.cv = cv;
  d.prm.ransac_iters = K;
  d.prm.min_depth = min_depth;
  launch_fit(nullptr, d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(d_states.get(states));
  HIPCHK(d_hvalid.get(hvalid));
  return VSM_OK;
}

int32_t vsm_debug_locate_count(double f, double cu, double cv, int32_t n_frames, const int32_t *row_off, const float *rows_uv, const double *rows_xyz,
                               int32_t n_jobs, const int32_t *job_frame, const int32_t *job_E, int32_t K, const double *states, const uint8_t *hvalid,
                               double inlier_threshold, double min_depth, int32_t launches, int32_t *counts) {
  if (!debug_frames_ok(n_frames, row_off, rows_uv, rows_xyz) || !debug_jobs_ok(n_frames, row_off, n_jobs, job_frame, job_E, K) || !states || !hvalid ||
      !counts || !(inlier_threshold > 0) || launches < 1 || launches > 2)
    return VSM_EARG;
  const size_t JK = (size_t)n_jobs * K;
  std::vector<LcTile> tiles;  // as the call builds them: every 256 rows of every job with hypotheses
  for (int32_t j = 0; j < n_jobs; j++)
    if (job_E[j])
      for (int32_t off = 0; off < row_off[job_frame[j] + 1] - row_off[job_frame[j]]; off += 256) tiles.push_back({j, off});
  LcDevice d;
  memset(&d, 0, sizeof(d));
  LcDebugFrames frames;
  LcDebugDev<LcTile> d_tiles;
  LcDebugDev<double> d_states;
  LcDebugDev<uint8_t> d_hvalid;
  LcDebugDev<int32_t> d_counts;
  HIPCHK(frames.put(n_frames, row_off, rows_uv, rows_xyz, n_jobs, job_frame, job_E, d));
  HIPCHK(d_tiles.put(tiles.data(), tiles.size()));
  HIPCHK(d_states.put(states, JK * 12));
  HIPCHK(d_hvalid.put(hvalid, JK));
  HIPCHK(d_counts.put(nullptr, JK));
  HIPCHK(hipMemset(d_counts.p, 0, JK * 4));  // the caller of the kernel clears, once: the kernel only adds
  d.tiles = d_tiles.p, d.states = d_states.p, d.hvalid = d_hvalid.p, d.counts = d_counts.p;
  d.n_tiles = (int32_t)tiles.size();
  d.f = f, d.cu = cu, d.cv = cv;
  d.prm.ransac_iters = K;
  d.prm.inlier_threshold = inlier_threshold;
  d.prm.min_depth = min_depth;
  for (int32_t l = 0; l < launches && d.n_tiles > 0; l++) launch_count(nullptr, d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(d_counts.get(counts));
  return VSM_OK;
}

int32_t vsm_debug_locate_winner(int32_t n_frames, const int32_t *frame_job, int32_t n_jobs, const int32_t *job_E, int32_t K, int32_t min_inliers,
                                const int32_t *counts, const uint8_t *hvalid, const double *states, int32_t *verdict, int32_t *best, int32_t *inliers,
                                double *lin_poses, uint8_t *lin_valid) {
  if (n_frames < 1 || n_jobs < 1 || K < 1 || (int64_t)n_jobs * K > LC_DEBUG_MAX_HYPOTHESES || !frame_job || !job_E || !counts || !hvalid || !states ||
      !verdict || !best || !inliers || !lin_poses || !lin_valid)
    return VSM_EARG;
  for (int32_t g = 0; g < n_frames; g++)
    if (frame_job[g] < -1 || frame_job[g] >= n_jobs) return VSM_EARG;
  const size_t JK = (size_t)n_jobs * K, F = (size_t)n_frames;
  LcDevice d;
  memset(&d, 0, sizeof(d));
  LcDebugDev<int32_t> d_frame_job, d_job_E, d_counts, d_verdict, d_best, d_inliers;
  LcDebugDev<uint8_t> d_hvalid, d_lin_valid;
  LcDebugDev<double> d_states, d_lin;
  HIPCHK(d_frame_job.put(frame_job, F));
  HIPCHK(d_job_E.put(job_E, (size_t)n_jobs));
  HIPCHK(d_counts.put(counts, JK));
  HIPCHK(d_hvalid.put(hvalid, JK));
  HIPCHK(d_states.put(states, JK * 12));
  HIPCHK(d_verdict.put(verdict, F));  // (the caller's content: the kernel writes every frame's entry)
  HIPCHK(d_best.put(best, F));
  HIPCHK(d_inliers.put(inliers, F));
  HIPCHK(d_lin.put(lin_poses, 12 * F));
  HIPCHK(d_lin_valid.put(lin_valid, F));
  d.frame_job = d_frame_job.p, d.job_E = d_job_E.p, d.counts = d_counts.p, d.hvalid = d_hvalid.p, d.states = d_states.p;
  d.verdict = d_verdict.p, d.best = d_best.p, d.inliers = d_inliers.p, d.lin_poses = d_lin.p, d.lin_valid = d_lin_valid.p;
  d.n_frames = n_frames, d.n_jobs = n_jobs;
  d.prm.ransac_iters = K;
  d.prm.min_inliers = min_inliers;
  launch_winner(nullptr, d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(d_verdict.get(verdict));
  HIPCHK(d_best.get(best));
  HIPCHK(d_inliers.get(inliers));
  HIPCHK(d_lin.get(lin_poses));
  HIPCHK(d_lin_valid.get(lin_valid));
  return VSM_OK;
}

}  // extern "C"
