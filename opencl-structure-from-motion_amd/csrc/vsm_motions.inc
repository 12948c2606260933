// Monocular motion of every pair of a pair set (included by vsm_mono.hip behind MonoEgo; DESIGN.md section 5).
//
// MonoEgo::estimate's steps, each for all pairs of a chunk at once: the host pool buckets, normalises and samples (every
// pair from a sampler and a rand() stream of its own), one launch fits all (pair, hypothesis), one counts all (pair,
// hypothesis, match), one picks every pair's winner and compacts its inlier list; the host pool then runs the sequential
// pieces of the pairs side by side (F from all inliers, E -> R|t); one launch triangulates all (pair, candidate, match), one
// gathers every pair's chosen candidate; the pool filters and takes medians; one launch votes for all surviving pairs and
// the pool settles the proposals exactly.  Three waits per chunk.  The points of a chunk's pairs lie one behind the other,
// pt_base[pair] = where a pair's begin (a pair that ended before the RANSAC has none).
//
// Block -> (pair, offset) goes through tile tables the host builds from the pairs' sizes: a launch has exactly the blocks
// its pairs need, whatever the spread of their sizes, and in a pair's last tile the waves past its end leave at once.

struct MotTile {
  int32_t pair, off;
};
struct MotVote {  // one pair's plane vote: its d values at d[base .. base + np)
  int32_t base, np;
  double threshold, weight;
};

// k_mono_fit's group per (pair, hypothesis): g = pair * K + hypothesis, 16 per block - a block may span two pairs
__global__ void __launch_bounds__(256)
    k_motions_fit(const MonoPt *__restrict__ pts, const int32_t *__restrict__ pt_base, const int32_t *__restrict__ picks, int K, int total,
                  double *__restrict__ Fs) {
  __shared__ double s_m[16 * FIT_GROUP_DOUBLES];
  const int grp = threadIdx.x >> 4, ln = threadIdx.x & 15;
  const int g = blockIdx.x * 16 + grp;
  if (g >= total) return;  // whole groups leave together
  const int p = g / K, base = pt_base[p];
  if (pt_base[p + 1] == base) return;  // a pair that ended before the RANSAC
  mono_fit_group(pts + base, picks + (size_t)g * 8, s_m + grp * FIT_GROUP_DOUBLES, ln, Fs + (size_t)g * 9);
}

// Sampson counts: blockIdx.x = a tile of 256 matches of one pair, blockIdx.y = a run of `hyps` hypotheses; a lane keeps its
// match in registers, F is wave-uniform.  counts[pair * K + k] += inliers (integer atomics: the sum has no order).
__global__ void __launch_bounds__(256)
    k_motions_count(const MonoPt *__restrict__ pts, const int32_t *__restrict__ pt_base, const MotTile *__restrict__ tiles, const double *__restrict__ Fs,
                    int K, int hyps, double thr, int32_t *__restrict__ counts) {
  const MotTile t = tiles[blockIdx.x];
  const int base = pt_base[t.pair], n = pt_base[t.pair + 1] - base;
  if (t.off + (int)(threadIdx.x & ~63u) >= n) return;  // a whole wave past the pair's end
  const int i = t.off + threadIdx.x;
  const bool live = i < n;
  const MonoPt q = pts[base + (live ? i : 0)];
  const int k0 = blockIdx.y * hyps, k1 = min(K, k0 + hyps);
  for (int k = k0; k < k1; k++) {
    const size_t g = (size_t)t.pair * K + k;
    const bool in = live && sampson_in(q, Fs + g * 9, thr);
    const unsigned long long b = __ballot(in);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&counts[g], (int32_t)__popcll(b));
  }
}

// One block per pair: the winner = the smallest k among the largest counts (none if every count is 0), a reduction on
// (count, -k); then the matches passing sampson_in for its F, indices ascending: per tile of 256 a ballot per wave, popcount
// prefixes inside the wave and over the block's four waves - the order does not depend on timing.
__global__ void __launch_bounds__(256)
    k_motions_winner(const MonoPt *__restrict__ pts, const int32_t *__restrict__ pt_base, const double *__restrict__ Fs,
                     const int32_t *__restrict__ counts, int K, double thr, int32_t *__restrict__ best, double *__restrict__ Fwin,
                     int32_t *__restrict__ inl, int32_t *__restrict__ n_inl) {
  __shared__ unsigned long long s_key[4];
  __shared__ int32_t s_cnt[4];
  const int p = blockIdx.x, base = pt_base[p], n = pt_base[p + 1] - base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long key = 0;  // count << 32 | ~k: the maximum is the largest count at the smallest k
  if (n > 0)
    for (int k = threadIdx.x; k < K; k += 256) {
      const unsigned long long c = (unsigned long long)(uint32_t)counts[(size_t)p * K + k];
      const unsigned long long v = (c << 32) | (uint32_t)(0xffffffffu - (uint32_t)k);
      key = v > key ? v : key;
    }
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o = __shfl_xor(key, d);
    key = o > key ? o : key;
  }
  if (lane == 0) s_key[wave] = key;
  __syncthreads();
  key = s_key[0];
  for (int w = 1; w < 4; w++) key = s_key[w] > key ? s_key[w] : key;
  const int bestk = (key >> 32) ? (int)(0xffffffffu - (uint32_t)key) : -1;
  if (threadIdx.x == 0) best[p] = bestk;
  if (bestk < 0) {  // (uniform for the block)
    if (threadIdx.x == 0) n_inl[p] = 0;
    return;
  }
  const double *F = Fs + ((size_t)p * K + bestk) * 9;
  if (threadIdx.x < 9) Fwin[(size_t)p * 9 + threadIdx.x] = F[threadIdx.x];
  int running = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + threadIdx.x;
    const bool in = i < n && sampson_in(pts[base + i], F, thr);
    const unsigned long long b = __ballot(in);
    __syncthreads();  // (the last tile's s_cnt has been read)
    if (lane == 0) s_cnt[wave] = (int32_t)__popcll(b);
    __syncthreads();
    int before = running;
    for (int w = 0; w < wave; w++) before += s_cnt[w];
    if (in) inl[base + before + (int)__popcll(b & ((1ull << lane) - 1ull))] = i;
    running += s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
  }
  if (threadIdx.x == 0) n_inl[p] = running;
}

// k_mono_triangulate's thread per (pair, candidate blockIdx.y, match): tiles of 64 matches of the pairs that came this far,
// the cameras from a table.  X of a pair: [candidate][row][match] at X + 16 * pt_base[pair]; chir[pair * 4 + candidate].
__global__ void __launch_bounds__(64)
    k_motions_triangulate(const MonoPt *__restrict__ raw, const int32_t *__restrict__ pt_base, const MotTile *__restrict__ tiles,
                          const MonoCams *__restrict__ cams, double *__restrict__ X, int32_t *__restrict__ chir) {
  __shared__ double s_m[TRI_LDS_DOUBLES];
  const MotTile t = tiles[blockIdx.x];
  const int base = pt_base[t.pair], n = pt_base[t.pair + 1] - base;
  const int i = t.off + threadIdx.x, c = blockIdx.y;
  bool front = false;
  if (i < n) {
    const MonoCams *cm = cams + t.pair;
    front = mono_triangulate_one(raw[base + i], cm->P1, cm->P2[c], s_m + threadIdx.x, X + (size_t)16 * base + (size_t)c * 4 * n + i, (size_t)n);
  }
  const unsigned long long b = __ballot(front);
  if (threadIdx.x == 0 && b) atomicAdd(&chir[t.pair * 4 + c], (int32_t)__popcll(b));
}

// the chosen candidate's points of every pair, [row][match] at Xsel + 4 * pt_base[pair]: the host picks the same candidate
// from the same four counts (MonoEgo::pick_candidate)
__global__ void __launch_bounds__(64)
    k_motions_gather(const int32_t *__restrict__ pt_base, const MotTile *__restrict__ tiles, const int32_t *__restrict__ chir,
                     const double *__restrict__ X, double *__restrict__ Xsel) {
  const MotTile t = tiles[blockIdx.x];
  const int base = pt_base[t.pair], n = pt_base[t.pair + 1] - base;
  const int i = t.off + threadIdx.x;
  if (i >= n) return;
  int pick = -1, max_in = 0;
  for (int c = 0; c < 4; c++) {
    const int v = chir[t.pair * 4 + c];
    if (v > max_in) {
      max_in = v;
      pick = c;
    }
  }
  if (pick < 0) return;
  for (int r = 0; r < 4; r++) Xsel[(size_t)4 * base + (size_t)r * n + i] = X[(size_t)16 * base + ((size_t)pick * 4 + r) * n + i];
}

// k_mono_plane_vote per pair: blockIdx.x = a tile of 256 candidates of one pair, which walks all of the pair's points
// through LDS (no slices of the j range: the pairs fill the device).  Proposals only, like the per-pair kernel's.
__global__ void __launch_bounds__(256)
    k_motions_vote(const double *__restrict__ d, const MotVote *__restrict__ votes, const MotTile *__restrict__ tiles, double *__restrict__ sums) {
  __shared__ double s_d[256];
  const MotTile t = tiles[blockIdx.x];
  const MotVote v = votes[t.pair];
  const double *dp = d + v.base;
  const int i = t.off + threadIdx.x;
  const double di = i < v.np ? dp[i] : 0.0;
  const bool active = i < v.np && di > v.threshold;
  double sum = 0;
  for (int j0 = 0; j0 < v.np; j0 += 256) {
    __syncthreads();
    s_d[threadIdx.x] = j0 + (int)threadIdx.x < v.np ? dp[j0 + threadIdx.x] : 0.0;
    __syncthreads();
    const int lim = min(256, v.np - j0);
    if (active)
      for (int j = 0; j < lim; j++) {
        const double dist = s_d[j] - di;
        sum += exp(-dist * dist * v.weight);
      }
  }
  if (i < v.np) sums[v.base + i] = active ? sum : 0.0;
}

namespace {

// one pair of a batch: its list (bucketed where asked), its sampler and its estimator
struct MotPair {
  MonoEgo ego;
  uint32_t sampler = 71;  // a fresh process of the reference (viso/viso.cpp:93)
  int n = 0, np = 0, pick = -1;
  bool running = false;
};

// the list the estimate sees: the caller's, or what a fresh VisualOdometryMono's second process() would keep of it
void mot_take_list(const vsm_vo_mono_params &par, const vsm_p_match *list, int32_t n, int bucket, std::vector<vsm_p_match> &out) {
  out.assign(list, list + (n > 0 ? n : 0));
  if (bucket) {
    VsmRandStream rnd;  // srand(0), viso/viso.cpp:35
    rnd.seed(0);
    vsm_host_bucket_with(out, par.bucket_max_features, (float)par.bucket_width, (float)par.bucket_height, rnd);
  }
}

void mot_store(VsmMotionsResult &out, int32_t k, int rc, int stage, const double *tr6) {
  out.rc[k] = rc;
  out.stage[k] = stage;
  if (rc == 1) {
    memcpy(&out.tr6[(size_t)6 * k], tr6, 6 * sizeof(double));
    vsm_pose_matrix(tr6, &out.T16[(size_t)16 * k]);
  }
  if (rc < 0) out.inliers[k].clear();  // (the reference leaves a stale list; a batch has none to leave)
}

void mot_count_stages(VsmMotionsResult &out) {
  for (int32_t s : out.stage)
    if (s >= 0 && s <= VSM_MOT_OK) out.stats[s]++;
}

}  // namespace

void vsm_motions_dev_release(VsmMotionsDev &D) {
  D.st.release();
  D = VsmMotionsDev();
}

void vsm_motions_host(const vsm_vo_mono_params &par, int32_t n_pairs, const vsm_p_match *const *lists, const int32_t *counts, int bucket, int threads,
                      VsmPool *pool, VsmMotionsResult &out) {
  const double t0 = vsm_now_us();
  out.reset(n_pairs);
  auto one = [&](int k) {
    mot_take_list(par, lists[k], counts[k], bucket, out.matches[k]);
    MotPair P;
    P.ego.par = par;
    P.ego.own_sampler = &P.sampler;
    double tr6[6];
    const int rc = P.ego.estimate(out.matches[k].data(), (int)out.matches[k].size(), (VsmPool *)nullptr, (MonoGpu *)nullptr, tr6, out.inliers[k]);
    mot_store(out, k, rc, P.ego.stage, tr6);
  };
  if (pool) {
    pool->run(n_pairs, one);
  } else if (threads > 1 && n_pairs > 1) {
    VsmPool own(std::min(threads, (int)n_pairs));
    own.run(n_pairs, one);
  } else {
    for (int32_t k = 0; k < n_pairs; k++) one(k);
  }
  mot_count_stages(out);
  out.timings[5] = vsm_now_us() - t0;
  out.have = true;
}

// Device bytes of a chunk: per (pair, hypothesis) 32 (picks) + 72 (F) + 4 (count) = 108, per match 16 + 16 (normalised and
// raw points) + 128 (X of four candidates) + 32 (the chosen one) + 4 (inlier index) + 8 + 8 (d, vote sum) = 212, per pair
// about 700 (cameras, bases, tiles, winner).  chunk = 0 keeps a chunk's block below MOT_CHUNK_BYTES.
#define MOT_CHUNK_BYTES ((size_t)256 << 20)

int vsm_motions_device(VsmMotionsDev &D, hipStream_t stream, VsmPool *pool, const vsm_vo_mono_params &par, int32_t n_pairs, const vsm_p_match *const *lists,
                       const int32_t *counts, int bucket, int chunk, VsmMotionsResult &out) {
  const double t_begin = vsm_now_us();
  if (!D.tested) {  // the self-test every estimator runs when it is created: does the device reproduce the host's SVD bit for bit?
    MonoGpu g;
    D.svd_on_device = g.init() && g.svd_on_device;
    D.tested = true;
  }
  if (!D.svd_on_device) {  // (not silently: the stats then show no pair from the device)
    vsm_motions_host(par, n_pairs, lists, counts, bucket, 0, pool, out);
    return VSM_OK;
  }
  out.reset(n_pairs);
  const int K = std::max(par.ransac_iters, 0);
  if (chunk <= 0) {
    int32_t max_n = 0;
    for (int32_t k = 0; k < n_pairs; k++) max_n = std::max(max_n, counts[k]);
    const size_t per_pair = (size_t)K * 108 + (size_t)max_n * 212 + 700;
    chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_pairs, MOT_CHUNK_BYTES / per_pair));
  }
  chunk = std::min(chunk, (int)n_pairs);
  std::vector<MotPair> pairs((size_t)chunk);
  std::vector<int32_t> running;  // chunk-local indices of the pairs still in the estimate
  const VsmDrain fail{stream};  // (vsm_stage.h)
  auto run_pairs = [&](const std::vector<int32_t> &which, const std::function<void(int)> &fn) {
    if (which.empty()) return;
    pool->run((int)which.size(), [&](int t) { fn(which[t]); });
  };
  for (int32_t p0 = 0; p0 < n_pairs; p0 += chunk) {
    const int Pc = std::min(chunk, (int)(n_pairs - p0));
    const double t0 = vsm_now_us();
    out.stats[VSM_MOT_STAT_CHUNKS]++;
    // ---- host pool: lists, normalisation, samples ----
    pool->run(Pc, [&](int j) {
      MotPair &P = pairs[j];
      const int32_t k = p0 + j;
      mot_take_list(par, lists[k], counts[k], bucket, out.matches[k]);
      P.ego.par = par;
      P.sampler = 71;
      P.ego.own_sampler = &P.sampler;
      P.n = (int)out.matches[k].size();
      P.np = 0;
      P.pick = -1;
      P.running = P.ego.begin(out.matches[k].data(), P.n);
      if (!P.running) mot_store(out, k, -1, P.ego.stage, nullptr);
    });
    std::vector<int32_t> base((size_t)Pc + 1, 0);
    std::vector<MotTile> tiles256;
    running.clear();
    for (int j = 0; j < Pc; j++) {
      const int n = pairs[j].running ? pairs[j].n : 0;
      base[j + 1] = base[j] + n;
      for (int off = 0; off < n; off += 256) tiles256.push_back({j, off});
      if (pairs[j].running) running.push_back(j);
    }
    if (running.empty()) continue;
    const size_t N = (size_t)base[Pc], PK = (size_t)Pc * K, T256 = tiles256.size(), T64 = (N + 63) / 64 + running.size();
    // ---- layout: the pinned input block and its device twin share offsets; device-only arrays and the results behind ----
    VsmLayout in;
    const size_t o_base = in.take(((size_t)Pc + 1) * 4), o_t256 = in.take(T256 * sizeof(MotTile)), o_pts = in.take(N * sizeof(MonoPt)),
                 o_raw = in.take(N * sizeof(MonoPt)), o_picks = in.take(PK * 32 + 4);
    const size_t up1 = in.at;
    const size_t o_cams = in.take((size_t)Pc * sizeof(MonoCams)), o_t64 = in.take(T64 * sizeof(MotTile));
    const size_t up2 = in.at;
    const size_t o_votes = in.take((size_t)Pc * sizeof(MotVote)), o_vt = in.take(T256 * sizeof(MotTile)), o_d = in.take(N * 8);
    VsmLayout res;
    const size_t r_best = res.take((size_t)Pc * 4), r_ninl = res.take((size_t)Pc * 4), r_fwin = res.take((size_t)Pc * 72), r_inl = res.take(N * 4);
    const size_t dn1 = res.at;
    const size_t r_chir = res.take((size_t)Pc * 16), r_xsel = res.take(N * 32);
    const size_t dn2 = res.at;
    const size_t r_sums = res.take(N * 8);
    VsmLayout dv;
    dv.at = in.at;
    const size_t d_res = dv.take(res.at), d_F = dv.take(PK * 72 + 8), d_counts = dv.take(PK * 4 + 4), d_X = dv.take(N * 128);
    VSM_CHK(D.st.grow_in(in.at, stream));
    VSM_CHK(D.st.grow_out(res.at, stream));
    VSM_CHK(D.st.grow_dev(dv.at, stream));
    uint8_t *hin = D.st.pin_in, *hout = D.st.pin_out, *dev = D.st.dev, *dres = D.st.dev + d_res;
    // ---- pack ----
    memcpy(hin + o_base, base.data(), ((size_t)Pc + 1) * 4);
    memcpy(hin + o_t256, tiles256.data(), T256 * sizeof(MotTile));
    run_pairs(running, [&](int j) {
      MotPair &P = pairs[j];
      const vsm_p_match *m = out.matches[p0 + j].data();
      memcpy((MonoPt *)(hin + o_pts) + base[j], P.ego.pts.data(), (size_t)P.n * sizeof(MonoPt));
      MonoPt *raw = (MonoPt *)(hin + o_raw) + base[j];
      for (int i = 0; i < P.n; i++) raw[i] = {m[i].u1p, m[i].v1p, m[i].u1c, m[i].v1c};
      if (K > 0) memcpy(hin + o_picks + (size_t)j * K * 32, P.ego.picks.data(), (size_t)K * 32);
    });
    const int32_t *d_base = (const int32_t *)(dev + o_base);
    const MonoPt *d_pts = (const MonoPt *)(dev + o_pts), *d_raw = (const MonoPt *)(dev + o_raw);
    double *dF = (double *)(dev + d_F);
    int32_t *dcounts = (int32_t *)(dev + d_counts);
    // ---- fit, count, winner ----
    VSM_CHK(hipMemcpyAsync(dev, hin, up1, hipMemcpyHostToDevice, stream));
    const double t1 = vsm_now_us();
    if (K > 0) {
      VSM_CHK(hipMemsetAsync(dcounts, 0, PK * 4, stream));
      hipLaunchKernelGGL(k_motions_fit, dim3((unsigned)((PK + 15) / 16)), dim3(256), 0, stream, d_pts, d_base, (const int32_t *)(dev + o_picks), K, (int)PK, dF);
      VSM_CHK(hipGetLastError());
      const int hyps = std::max(16, (K + 65534) / 65535);
      hipLaunchKernelGGL(k_motions_count, dim3((unsigned)T256, (unsigned)((K + hyps - 1) / hyps)), dim3(256), 0, stream, d_pts, d_base,
                         (const MotTile *)(dev + o_t256), dF, K, hyps, par.inlier_threshold, dcounts);
      VSM_CHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_motions_winner, dim3((unsigned)Pc), dim3(256), 0, stream, d_pts, d_base, dF, dcounts, K, par.inlier_threshold,
                       (int32_t *)(dres + r_best), (double *)(dres + r_fwin), (int32_t *)(dres + r_inl), (int32_t *)(dres + r_ninl));
    VSM_CHK(hipGetLastError());
    VSM_CHK(hipMemcpyAsync(hout, dres, dn1, hipMemcpyDeviceToHost, stream));
    VSM_CHK(hipStreamSynchronize(stream));
    out.stats[VSM_MOT_STAT_WAITS]++;
    if (K > 0) {
      out.stats[VSM_MOT_STAT_FIT] += (int64_t)running.size();
      out.stats[VSM_MOT_STAT_COUNT] += (int64_t)running.size();
    }
    const double t2 = vsm_now_us();
    // ---- host pool: F from all inliers, E, the four candidates and their cameras ----
    const int32_t *h_ninl = (const int32_t *)(hout + r_ninl), *h_inl = (const int32_t *)(hout + r_inl);
    run_pairs(running, [&](int j) {
      MotPair &P = pairs[j];
      const int32_t k = p0 + j;
      out.inliers[k].assign(h_inl + base[j], h_inl + base[j] + h_ninl[j]);
      if (h_ninl[j] < 10) {
        P.running = false;
        mot_store(out, k, 0, VSM_MOT_FEW_INLIERS, nullptr);
        return;
      }
      P.ego.motion_candidates(out.inliers[k]);
      memcpy((MonoCams *)(hin + o_cams) + j, &P.ego.cams, sizeof(MonoCams));
    });
    std::vector<MotTile> tiles;
    {
      std::vector<int32_t> still;
      for (int32_t j : running)
        if (pairs[j].running) {
          still.push_back(j);
          for (int off = 0; off < pairs[j].n; off += 64) tiles.push_back({j, off});
        }
      running.swap(still);
    }
    const double t3 = vsm_now_us();
    out.timings[0] += t1 - t0;
    out.timings[1] += t2 - t1;
    out.timings[2] += t3 - t2;
    if (running.empty()) continue;
    // ---- triangulation of all (pair, candidate, match), the chosen candidates gathered ----
    memcpy(hin + o_t64, tiles.data(), tiles.size() * sizeof(MotTile));
    VSM_CHK(hipMemcpyAsync(dev + o_cams, hin + o_cams, up2 - up1, hipMemcpyHostToDevice, stream));
    VSM_CHK(hipMemsetAsync(dres + r_chir, 0, (size_t)Pc * 16, stream));
    hipLaunchKernelGGL(k_motions_triangulate, dim3((unsigned)tiles.size(), 4), dim3(64), 0, stream, d_raw, d_base, (const MotTile *)(dev + o_t64),
                       (const MonoCams *)(dev + o_cams), (double *)(dev + d_X), (int32_t *)(dres + r_chir));
    VSM_CHK(hipGetLastError());
    hipLaunchKernelGGL(k_motions_gather, dim3((unsigned)tiles.size()), dim3(64), 0, stream, d_base, (const MotTile *)(dev + o_t64),
                       (const int32_t *)(dres + r_chir), (const double *)(dev + d_X), (double *)(dres + r_xsel));
    VSM_CHK(hipGetLastError());
    VSM_CHK(hipMemcpyAsync(hout + dn1, dres + dn1, dn2 - dn1, hipMemcpyDeviceToHost, stream));
    VSM_CHK(hipStreamSynchronize(stream));
    out.stats[VSM_MOT_STAT_WAITS]++;
    out.stats[VSM_MOT_STAT_TRI] += (int64_t)running.size();
    const double t4 = vsm_now_us();
    // ---- host pool: the candidate, the points in front, their median, the d values ----
    const int32_t *h_chir = (const int32_t *)(hout + r_chir);
    const double *h_xsel = (const double *)(hout + r_xsel);
    run_pairs(running, [&](int j) {
      MotPair &P = pairs[j];
      const int32_t k = p0 + j;
      P.pick = MonoEgo::pick_candidate(h_chir + 4 * j);
      if (P.pick < 0) {
        P.running = false;
        mot_store(out, k, 0, VSM_MOT_NONE_IN_FRONT, nullptr);
        return;
      }
      P.np = P.ego.front_points(h_xsel + (size_t)4 * base[j], P.n);
      if (P.np < 0) {
        P.running = false;
        mot_store(out, k, 0, P.ego.stage, nullptr);
      }
    });
    tiles.clear();
    {
      std::vector<int32_t> still;
      MotVote *votes = (MotVote *)(hin + o_votes);
      memset(votes, 0, (size_t)Pc * sizeof(MotVote));
      int32_t at = 0;
      for (int32_t j : running)
        if (pairs[j].running) {
          still.push_back(j);
          votes[j].base = at;
          votes[j].np = pairs[j].np;
          votes[j].threshold = pairs[j].ego.vote_threshold;
          votes[j].weight = pairs[j].ego.vote_weight;
          memcpy((double *)(hin + o_d) + at, pairs[j].ego.dvals.data(), (size_t)pairs[j].np * 8);
          for (int off = 0; off < pairs[j].np; off += 256) tiles.push_back({j, off});
          at += pairs[j].np;
        }
      running.swap(still);
    }
    if (running.empty()) {
      out.timings[3] += t4 - t3;
      out.timings[4] += vsm_now_us() - t4;
      continue;
    }
    // ---- the plane vote of all surviving pairs (on the device whatever their size), settled exactly on the host ----
    memcpy(hin + o_vt, tiles.data(), tiles.size() * sizeof(MotTile));
    VSM_CHK(hipMemcpyAsync(dev + o_votes, hin + o_votes, in.at - up2, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_motions_vote, dim3((unsigned)tiles.size()), dim3(256), 0, stream, (const double *)(dev + o_d), (const MotVote *)(dev + o_votes),
                       (const MotTile *)(dev + o_vt), (double *)(dres + r_sums));
    VSM_CHK(hipGetLastError());
    VSM_CHK(hipMemcpyAsync(hout + r_sums, dres + r_sums, N * 8, hipMemcpyDeviceToHost, stream));
    VSM_CHK(hipStreamSynchronize(stream));
    out.stats[VSM_MOT_STAT_WAITS]++;
    out.stats[VSM_MOT_STAT_VOTE] += (int64_t)running.size();
    const MotVote *votes = (const MotVote *)(hin + o_votes);
    const double *h_sums = (const double *)(hout + r_sums);
    run_pairs(running, [&](int j) {
      MotPair &P = pairs[j];
      const int best_idx = P.ego.resolve_vote(h_sums + votes[j].base, P.np, P.ego.vote_threshold, P.ego.vote_weight);
      double tr6[6];
      P.ego.finish(P.pick, best_idx, tr6);
      mot_store(out, p0 + j, 1, VSM_MOT_OK, tr6);
    });
    out.timings[3] += t4 - t3;
    out.timings[4] += vsm_now_us() - t4;
  }
  mot_count_stages(out);
  out.timings[5] = vsm_now_us() - t_begin;
  out.have = true;
  return VSM_OK;
}

extern "C" {

int32_t vsm_host_pairs_motions(const vsm_vo_mono_params *p, int32_t n_pairs, const vsm_p_match *const *lists, const int32_t *counts, int32_t bucket,
                               int32_t threads, int32_t *rc, int32_t *stage, double *tr6, double *T16, int32_t *n_inliers, int32_t *inliers,
                               int32_t *n_matches, vsm_p_match *matches) {
  if (!vsm_motions_args_ok(p, n_pairs, lists, counts, bucket)) return VSM_EARG;
  VsmMotionsResult R;
  vsm_motions_host(*p, n_pairs, lists, counts, bucket, threads, nullptr, R);
  size_t at = 0;  // pair k's inliers and matches start where the lists in front of it would (the sum of their counts)
  for (int32_t k = 0; k < n_pairs; k++) {
    if (rc) rc[k] = R.rc[k];
    if (stage) stage[k] = R.stage[k];
    if (n_inliers) n_inliers[k] = (int32_t)R.inliers[k].size();
    if (n_matches) n_matches[k] = (int32_t)R.matches[k].size();
    if (inliers && !R.inliers[k].empty()) memcpy(inliers + at, R.inliers[k].data(), R.inliers[k].size() * 4);
    if (matches && !R.matches[k].empty()) memcpy(matches + at, R.matches[k].data(), R.matches[k].size() * sizeof(vsm_p_match));
    at += (size_t)counts[k];
  }
  if (tr6) memcpy(tr6, R.tr6.data(), (size_t)n_pairs * 6 * 8);
  if (T16) memcpy(T16, R.T16.data(), (size_t)n_pairs * 16 * 8);
  return n_pairs;
}

// pair motions into camera-to-world poses (viso/sfm.hh:57-58: Tr_total = Tr_total * inv(motion))
int32_t vsm_chain_poses(int32_t n_frames, const int32_t *pairs, int32_t n_pairs, const double *T16, const int32_t *rc, int32_t root, double *poses12,
                        uint8_t *pose_valid) {
  if (n_frames <= 0 || root < 0 || root >= n_frames || n_pairs < 0 || !poses12 || !pose_valid || (n_pairs > 0 && (!pairs || !T16 || !rc))) return VSM_EARG;
  for (int32_t k = 0; k < n_pairs; k++)
    if (pairs[2 * k] < 0 || pairs[2 * k] >= n_frames || pairs[2 * k + 1] < 0 || pairs[2 * k + 1] >= n_frames) return VSM_EARG;
  memset(poses12, 0, (size_t)n_frames * 12 * sizeof(double));
  memset(pose_valid, 0, (size_t)n_frames);
  for (int i = 0; i < 3; i++) poses12[(size_t)12 * root + 5 * i] = 1.0;
  pose_valid[root] = 1;
  // out (3x4) = A (3x4, as [A | 0 0 0 1]) * B (3x4 likewise): every entry a sum over k ascending from the k = 0 product
  auto mul = [](const double *A, const double *B, double *out) {
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 4; j++) {
        double s = A[i * 4 + 0] * B[0 * 4 + j];
        for (int k = 1; k < 3; k++) s += A[i * 4 + k] * B[k * 4 + j];
        if (j == 3) s += A[i * 4 + 3];
        out[i * 4 + j] = s;
      }
  };
  int32_t posed = 1;
  for (bool set = true; set;) {
    set = false;
    for (int32_t k = 0; k < n_pairs; k++) {
      const int32_t a = pairs[2 * k], b = pairs[2 * k + 1];
      if (rc[k] != 1 || a == b || pose_valid[a] == pose_valid[b]) continue;
      const double *T = T16 + (size_t)16 * k;
      double M[12], R[12];
      if (pose_valid[a]) {  // pose[b] = pose[a] * inv(T), inv = [R' | -R' t]
        for (int i = 0; i < 3; i++) {
          for (int j = 0; j < 3; j++) M[i * 4 + j] = T[j * 4 + i];
          double s = T[0 * 4 + i] * T[0 * 4 + 3];
          for (int q = 1; q < 3; q++) s += T[q * 4 + i] * T[q * 4 + 3];
          M[i * 4 + 3] = -s;
        }
        mul(poses12 + (size_t)12 * a, M, R);
        memcpy(poses12 + (size_t)12 * b, R, sizeof(R));
        pose_valid[b] = 1;
      } else {  // pose[a] = pose[b] * T
        memcpy(M, T, sizeof(M));
        mul(poses12 + (size_t)12 * b, M, R);
        memcpy(poses12 + (size_t)12 * a, R, sizeof(R));
        pose_valid[a] = 1;
      }
      posed++;
      set = true;
    }
  }
  return posed;
}

}  // extern "C"
