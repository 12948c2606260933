// The library's test hooks (included last by vsm_api.cpp; DESIGN.md section 5): the debug entries of the batched forms'
// arithmetic (vsm_jobs.h), the host stages alone, and single kernels or chains on inputs of the caller.  None of this is
// part of a call's path.  The hooks that launch something share two pieces: DebugDev, a device allocation that goes when
// the hook returns whichever way, and DebugPairs, caller-given pairs as the pairs of one launch.

// a device allocation of n elements, freed by the destructor
template <typename T>
struct DebugDev {
  T *p = nullptr;
  DebugDev() = default;
  DebugDev(const DebugDev &) = delete;
  DebugDev &operator=(const DebugDev &) = delete;
  ~DebugDev() {
    if (p) (void)hipFree(p);
  }
  bool alloc(size_t n) { return hipMalloc((void **)&p, std::max<size_t>(n, 1) * sizeof(T)) == hipSuccess; }
  operator T *() const { return p; }
};

// P caller-given pairs as the P pairs of one launch: per pair the arrays asked for and the counts in one device block
// (VsmLayout), the pair table and the job table
struct DebugPairs {
  // what a pair gets: elements per array (0: none) and content for the front of some
  struct Pair {
    size_t raw = 0, flag = 0, blockcnt = 0, list1 = 0, list2 = 0, pf = 0;  // (pf: ints, 36 per match)
    bool one_list = false;  // list2 is list1 (a launch that runs one pass)
    size_t keys = 0;        // one array for keys[0] and keys[1], key_cap of them the kernels' to write
    int32_t key_cap = 0;
    int32_t count[2] = {0, 0};  // the lists' lengths before the launch
    size_t n_in = 0;            // records of content: raw_in, flag_in (an int each), list2_in, pf_in (36 ints each), where given
    const vsm_p_match *raw_in = nullptr, *list2_in = nullptr;
    const int32_t *flag_in = nullptr, *pf_in = nullptr;
  };
  DebugDev<uint8_t> block;
  VsmPair *d_pairs = nullptr;
  VsmJob *d_jobs = nullptr;
  uint8_t *extra = nullptr;  // extra_bytes of the block for a table of the hook's own
  std::vector<VsmPair> pairs;
  std::vector<VsmJob> jobs;
  // fill >= 0: the list and key arrays start as that byte (what the kernels leave unwritten comes back as it); everything
  // else of the block starts as zeros.  The sources may be pageable memory: the stream is idle when this returns.
  hipError_t create(hipStream_t s, const std::vector<Pair> &want, const std::vector<VsmJob> &job_table, int fill = -1, size_t extra_bytes = 0) {
    const size_t P = want.size();
    pairs.assign(P, VsmPair());
    jobs = job_table;
    // the block's layout and the tables' pointers into it: once for the size (on no block), once more on the block
    auto lay = [&](uint8_t *b) {
      VsmLayout L;
      auto arr = [&](size_t bytes) { return bytes ? (uint8_t *)((uintptr_t)b + L.take(bytes)) : nullptr; };
      for (size_t k = 0; k < P; k++) {
        const Pair &q = want[k];
        VsmPair &pr = pairs[k];
        pr.raw = (vsm_p_match *)arr(q.raw * sizeof(vsm_p_match));
        pr.flag = (int32_t *)arr(q.flag * 4);
        pr.blockcnt = (int32_t *)arr(q.blockcnt * 4);
        pr.list1 = (vsm_p_match *)arr(q.list1 * sizeof(vsm_p_match));
        pr.list2 = q.one_list ? pr.list1 : (vsm_p_match *)arr(q.list2 * sizeof(vsm_p_match));
        pr.pf = (int32_t *)arr(q.pf * 4);
        pr.keys[0] = pr.keys[1] = (uint64_t *)arr(q.keys * 8);
        pr.key_cap[0] = pr.key_cap[1] = q.key_cap;
        pr.count = (int32_t *)arr(4 * sizeof(int32_t));
      }
      d_pairs = (VsmPair *)arr(P * sizeof(VsmPair));
      d_jobs = (VsmJob *)arr(P * sizeof(VsmJob));
      extra = arr(extra_bytes);
      return L.at;
    };
    if (!block.alloc(lay(nullptr))) return hipErrorOutOfMemory;
    hipError_t e = hipMemsetAsync(block, 0, lay(block), s);
    for (size_t k = 0; k < P && e == hipSuccess; k++) {
      const Pair &q = want[k];
      VsmPair &pr = pairs[k];
      pr.hcount = pr.count + 2;  // (no host-mapped twin here: a kernel's second count goes beside the first)
      if (fill >= 0) {
        if (pr.list1) e = hipMemsetAsync(pr.list1, fill, q.list1 * sizeof(vsm_p_match), s);
        if (e == hipSuccess && pr.list2 && !q.one_list) e = hipMemsetAsync(pr.list2, fill, q.list2 * sizeof(vsm_p_match), s);
        if (e == hipSuccess && pr.keys[0]) e = hipMemsetAsync(pr.keys[0], fill, q.keys * 8, s);
      }
      if (e == hipSuccess) e = hipMemcpyAsync(pr.count, q.count, sizeof(q.count), hipMemcpyHostToDevice, s);
      auto content = [&](void *dst, const void *src, size_t bytes) {
        if (e == hipSuccess && q.n_in > 0 && src) e = hipMemcpyAsync(dst, src, q.n_in * bytes, hipMemcpyHostToDevice, s);
      };
      content(pr.raw, q.raw_in, sizeof(vsm_p_match)), content(pr.flag, q.flag_in, 4);
      content(pr.list2, q.list2_in, sizeof(vsm_p_match)), content(pr.pf, q.pf_in, 36 * 4);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(d_pairs, pairs.data(), P * sizeof(VsmPair), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_jobs, jobs.data(), P * sizeof(VsmJob), hipMemcpyHostToDevice, s);
    const hipError_t es = hipStreamSynchronize(s);
    return e != hipSuccess ? e : es;
  }
  // pair k's count of a pass as the kernels left it; its second copy must agree
  hipError_t fetch_count(size_t k, int pass, int32_t *n) const {
    int32_t cnt[4] = {0, 0, 0, 0};
    const hipError_t e = hipMemcpy(cnt, pairs[k].count, sizeof(cnt), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    *n = cnt[pass];
    return cnt[2 + pass] == cnt[pass] ? hipSuccess : hipErrorUnknown;
  }
  // the first n records of pair k's list of a pass; the first n words of its key array
  hipError_t fetch_list(size_t k, int pass, size_t n, vsm_p_match *out) const {
    return n ? hipMemcpy(out, pass ? pairs[k].list2 : pairs[k].list1, n * sizeof(vsm_p_match), hipMemcpyDeviceToHost) : hipSuccess;
  }
  hipError_t fetch_keys(size_t k, size_t n, uint64_t *out) const { return n ? hipMemcpy(out, pairs[k].keys[0], n * 8, hipMemcpyDeviceToHost) : hipSuccess; }
};

// One prepared triangulation on the device, `copies` times (vsm_debug_delaunay_gpu and vsm_debug_dc_bench), in one block
struct DcDeviceCopy {
  std::vector<VsmDcJob> jobs;
  DebugDev<uint8_t> block;
  VsmDcJob *d_jobs = nullptr;
  int nt = 0, nn = 0, m = 0, nlev = 0, lev_nodes[VSM_DC_MAX_LEVELS] = {0};
  size_t tri_bytes = 0;
  bool device_kd = false;  // the keys arrive in (x,y) order and k_dc_kd_order runs first
  bool blocks = false;     // k_dc_block instead of k_dc_subtrees + k_dc_merge_level
  bool create(ExactDelaunay &d, int copies) {
    static_assert(sizeof(VsmDcTask) == sizeof(ExactDelaunay::Task), "task layout");
    static_assert(sizeof(VsmDcMerge) == sizeof(ExactDelaunay::Merge), "merge layout");
    m = d.points();
    nt = (int)d.tasks().size();
    nn = d.num_nodes();
    const int ng = (int)d.device_merges().size();
    nlev = (int)d.device_levels().size();
    if (nlev > VSM_DC_MAX_LEVELS) return false;
    tri_bytes = (size_t)m * 2 * 8 * sizeof(int32_t);
    jobs.assign(copies, VsmDcJob());
    VsmDcTask *d_tasks = nullptr;
    VsmDcMerge *d_merges = nullptr;
    // the block's layout and the jobs' pointers into it: once for the size (on no block), once more on the block
    auto lay = [&](uint8_t *b) {
      VsmLayout L;
      auto arr = [&](size_t bytes) { return (uint8_t *)((uintptr_t)b + L.take(bytes)); };
      d_tasks = (VsmDcTask *)arr(sizeof(VsmDcTask) * nt);
      d_merges = (VsmDcMerge *)arr(sizeof(VsmDcMerge) * ng);
      d_jobs = (VsmDcJob *)arr(sizeof(VsmDcJob) * copies);
      for (VsmDcJob &job : jobs) {
        job.key = (uint64_t *)arr((size_t)m * 8);
        job.pt = (uint32_t *)arr((size_t)m * 4);
        job.id = (int32_t *)arr((size_t)m * 4);
        job.tri = (int32_t *)arr(tri_bytes);
        job.hulls = (VsmDcHull *)arr(sizeof(VsmDcHull) * nn);
        if (device_kd) {
          job.key_sorted = (const uint64_t *)arr((size_t)m * 8);
          job.kd_scratch = (uint32_t *)arr((size_t)m * 4 * VSM_DC_KD_SCRATCH);
        }
        job.tasks = d_tasks;
        job.merges = d_merges;
      }
      return L.at;
    };
    if (!block.alloc(lay(nullptr))) return false;
    lay(block);
    (void)hipMemcpy(d_tasks, d.tasks().data(), sizeof(VsmDcTask) * nt, hipMemcpyHostToDevice);
    (void)hipMemcpy(d_merges, d.device_merges().data(), sizeof(VsmDcMerge) * ng, hipMemcpyHostToDevice);
    for (VsmDcJob &job : jobs) {
      job.kd_stride = m;
      job.ntasks = nt;
      job.m = m;
      job.nlevels = nlev;
      job.level_off[0] = 0;
      for (int l = 0; l < nlev; l++) {
        job.level_off[l + 1] = job.level_off[l] + d.device_levels()[l];
        lev_nodes[l] = d.device_levels()[l];
      }
    }
    return hipMemcpy(d_jobs, jobs.data(), sizeof(VsmDcJob) * copies, hipMemcpyHostToDevice) == hipSuccess;
  }
  void load(const DcMesh &mesh, hipStream_t s) {
    for (VsmDcJob &job : jobs) {
      (void)hipMemcpyAsync(device_kd ? (void *)job.key_sorted : (void *)job.key, mesh.key, (size_t)m * 8, hipMemcpyHostToDevice, s);
      (void)hipMemsetAsync(job.tri, 0xff, tri_bytes, s);
    }
  }
  void launch(hipStream_t s) {
    if (device_kd) vsm_dc_launch_kd_order(s, d_jobs, (int)jobs.size());
    if (blocks) {
      vsm_dc_launch_blocks(s, d_jobs, (int)jobs.size(), nt);
      return;
    }
    vsm_dc_launch_subtrees(s, d_jobs, (int)jobs.size(), nt);
    for (int l = 0; l < nlev; l++) vsm_dc_launch_merge_level(s, d_jobs, (int)jobs.size(), l, lev_nodes[l]);
  }
};

// The refinement reads 5 x 5 bytes around (u1c, v1c) unguarded and converts the point to int: every reference point must be a
// pixel inside the margin.  The targets only have to be finite (the kernels' own margin tests guard them; the conversion of
// a float they let through is defined).  Pure arithmetic: the CPU suite calls it (vsm_debug_refine_check).
#define VSM_DEBUG_REFINE_MAX_PAIRS 64
static int refine_lists_check(int32_t w, int32_t hh, const vsm_p_match *const *lists, const int32_t *counts, int32_t P) {
  if (P < 1 || P > VSM_DEBUG_REFINE_MAX_PAIRS || !lists || !counts) return VSM_EARG;
  if (w < 2 * VSM_MARGIN + 1 || hh < 2 * VSM_MARGIN + 1) return VSM_EARG;
  const float u_lo = (float)VSM_MARGIN, u_hi = (float)(w - 1 - VSM_MARGIN), v_hi = (float)(hh - 1 - VSM_MARGIN);
  for (int32_t k = 0; k < P; k++) {
    if (counts[k] < 0 || counts[k] > VSM_PARA_MAX_LIST || (counts[k] > 0 && !lists[k])) return VSM_EARG;
    for (int32_t i = 0; i < counts[k]; i++) {
      const vsm_p_match &m = lists[k][i];
      const float xy[8] = {m.u1p, m.v1p, m.u2p, m.v2p, m.u1c, m.v1c, m.u2c, m.v2c};
      for (float x : xy)
        if (!std::isfinite(x)) return VSM_EARG;
      if (!(m.u1c >= u_lo && m.u1c <= u_hi && m.v1c >= u_lo && m.v1c <= v_hi)) return VSM_EARG;
      if (m.u1c != floorf(m.u1c) || m.v1c != floorf(m.v1c)) return VSM_EARG;
    }
  }
  return VSM_OK;
}

// P caller-given pass-2 lists as the pairs of a refinement launch: per pair list2, raw, (the fits' records) and the count;
// every job is `job`
static hipError_t debug_lists_create(DebugPairs &D, hipStream_t s, const vsm_p_match *const *lists, const int32_t *const *records, const int32_t *counts,
                                     int32_t P, bool with_pf, const VsmJob &job) {
  std::vector<DebugPairs::Pair> want(P);
  for (int32_t k = 0; k < P; k++) {
    DebugPairs::Pair &q = want[k];
    q.list2 = q.raw = (size_t)std::max(counts[k], 1);
    q.pf = with_pf ? q.list2 * 36 : 0;
    q.count[1] = counts[k];
    q.n_in = (size_t)counts[k];
    q.list2_in = lists[k];
    q.pf_in = records ? records[k] : nullptr;
  }
  return D.create(s, want, std::vector<VsmJob>(P, job));
}
// the lists as the kernels left them; shorter: the tail of refinement == 2 has rewritten the counts
static hipError_t debug_lists_fetch(const DebugPairs &D, const int32_t *counts, int32_t P, bool shorter, vsm_p_match *const *out, int32_t *out_counts) {
  for (int32_t k = 0; k < P; k++) {
    int32_t n = counts[k];
    if (shorter) {
      const hipError_t e = D.fetch_count(k, 1, &n);
      if (e != hipSuccess) return e;
      if (n < 0 || n > counts[k]) return hipErrorUnknown;
    }
    out_counts[k] = n;
    const hipError_t e = D.fetch_list(k, 1, (size_t)n, out[k]);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// what the triangulation hooks return: the triangles (cap of them at most) and their number
static int32_t debug_triangles_out(ExactDelaunay &d, int32_t *tris, int32_t cap) {
  const int32_t nt = d.num_triangles();
  for (int32_t i = 0; i < nt && i < cap; i++)
    for (int k = 0; k < 3; k++) tris[i * 3 + k] = d.triangles()[i * 3 + k];
  return nt;
}
// ... and the outlier hooks: the survivors, their number and (ranges given) their prior boxes in the device's layout
static int32_t debug_survivors_out(const vsm_params &p, const std::vector<vsm_p_match> &m, int32_t method, vsm_p_match *out, int32_t cap, float *ranges,
                                   int32_t w, int32_t hh) {
  if (ranges) {
    const int32_t dims[3] = {w, hh, w};
    std::vector<float> rg;
    vsm_host_prior_statistics(p, dims, m, method, rg);
    ranges_to_device_layout(ranges, rg.data(), rg.size());
  }
  for (size_t i = 0; i < m.size() && (int32_t)i < cap; i++) out[i] = m[i];
  return (int32_t)m.size();
}
// HIP-event time of what a hook puts on the null stream between start() and stop(); us(): behind a synchronisation
struct DebugTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  DebugTimer() { (void)hipEventCreate(&e0), (void)hipEventCreate(&e1); }
  ~DebugTimer() { (void)hipEventDestroy(e0), (void)hipEventDestroy(e1); }
  void start() { (void)hipEventRecord(e0, nullptr); }
  void stop() { (void)hipEventRecord(e1, nullptr); }
  double us() const { float ms = 0; return hipEventElapsedTime(&ms, e0, e1) == hipSuccess ? ms * 1e3 : 0; }
};

// a row of vsm_debug_chunk_jobs / vsm_debug_pair_jobs
static void debug_job_row(int32_t *o, const VsmJob &jb, int valid, int32_t last) {
  o[0] = jb.img_prev;
  o[1] = jb.img_curr;
  o[2] = jb.nq[0];
  o[3] = jb.nq[1];
  o[4] = jb.use_tr;
  o[5] = valid;
  o[6] = last;
}

// the rows of vsm_debug_ctx_layout / vsm_debug_dc2_layout: block 0's arrays, then block 1's
static int32_t debug_layout_rows(const VsmPlacer *const blocks[2], int64_t *rows, char *names, int32_t cap) {
  const size_t n = blocks[0]->rows.size() + blocks[1]->rows.size();
  if (n > (size_t)cap || !rows || !names) return (int32_t)n;
  for (int b = 0; b < 2; b++)
    for (const VsmPlacer::Row &r : blocks[b]->rows) {
      const int64_t row[5] = {b, r.index, r.set, (int64_t)r.at, (int64_t)r.bytes};
      memcpy(rows, row, sizeof(row));
      strncpy(names, r.name, 16);
      rows += 5, names += 16;
    }
  return (int32_t)n;
}

extern "C" {

// ---- debug entries of the device blocks' layouts (vsm_ctx.h, vsm_layouts.h; include/visomatch.h) ----
int32_t vsm_debug_ctx_layout(const vsm_params *p, int32_t w, int32_t hh, int32_t nframes, int32_t npairs, int32_t heads, int64_t *scalars,
                             int64_t *rows, char *names, int32_t cap, int32_t *n_rows) {
  if (!p || nframes < 0 || npairs < 0 || !scalars || !n_rows) return VSM_EARG;
  VsmGeom g;
  const int rc = vsm_ctx_geometry(*p, w, hh, g);
  if (rc != VSM_OK) return rc;
  const VsmCtxLayout L(g, *p, nframes, npairs, heads != 0);
  const int64_t s[8] = {(int64_t)L.arena.at, (int64_t)L.hm.at, (int64_t)L.pair_stride, (int64_t)g.f_stride, (int64_t)g.ranges_stride, g.cap_set[0], g.cap_set[1], (int64_t)g.qcap};
  memcpy(scalars, s, sizeof(s));
  const VsmPlacer *const blocks[2] = {&L.arena, &L.hm};
  *n_rows = debug_layout_rows(blocks, rows, names, cap);
  return VSM_OK;
}

int32_t vsm_debug_dc2_layout(int32_t npairs, int32_t list_cap, int32_t host_ties, int64_t *scalars, int64_t *rows, char *names, int32_t cap,
                             int32_t *n_rows) {
  if (npairs < 0 || list_cap < 0 || !scalars || !n_rows) return VSM_EARG;
  const Dc2Layout L(npairs, list_cap, host_ties != 0);
  const int64_t s[6] = {(int64_t)L.dev.at, (int64_t)L.host.at, (int64_t)L.pair_stride, L.ties_stride, (int64_t)L.keys_pitch, (int64_t)L.ties_pitch};
  memcpy(scalars, s, sizeof(s));
  const VsmPlacer *const blocks[2] = {&L.dev, &L.host};
  *n_rows = debug_layout_rows(blocks, rows, names, cap);
  return VSM_OK;
}

// ---- debug entries of the batched forms' arithmetic (vsm_jobs.h; include/visomatch.h) ----
int32_t vsm_debug_seq_plan(int32_t n_frames, int32_t pool_threads, int32_t host_in, int32_t seq_chunk, int32_t seq_first_chunk, const char *plan,
                           int32_t *chunk, int32_t *starts, int32_t cap) {
  if (n_frames <= 0 || pool_threads <= 0 || !chunk || !starts) return -1;
  const Seq2Plan P = seq2_plan(n_frames, pool_threads, host_in != 0, seq_chunk, seq_first_chunk, plan);
  if ((int32_t)P.start.size() > cap) return -1;
  *chunk = P.C;
  std::copy(P.start.begin(), P.start.end(), starts);
  return (int32_t)P.start.size() - 1;
}

int32_t vsm_debug_chunk_jobs(int32_t method, int32_t multi_stage, int32_t sides, int32_t banks, int32_t chunk, const int32_t *starts,
                             int32_t n_chunks, const int32_t *counts, const uint8_t *tr_valid, int32_t *frames_out, int32_t *max_nq_out) {
  if (method < 0 || method > 2 || sides < 1 || sides > 2 || banks < 2 || chunk < 1 || n_chunks < 1 || !starts || !counts || !frames_out ||
      !max_nq_out || starts[0] != 0)
    return -1;
  for (int k = 0; k < n_chunks; k++)
    if (starts[k + 1] <= starts[k] || starts[k + 1] - starts[k] > chunk) return -1;
  const std::vector<int32_t> chunk_start(starts, starts + n_chunks + 1);
  const int32_t n_frames = chunk_start[n_chunks];
  vsm_params p;
  vsm_default_params(&p);
  p.multi_stage = multi_stage;
  std::vector<int32_t> hm_counts((size_t)banks * chunk * sides * 2, 0), seq_src(n_frames, 0);
  const std::vector<double> Tr((size_t)n_frames * 12, 0.0);
  std::vector<VsmJob> jobs(chunk);
  std::vector<char> valid(chunk);
  int32_t nprev[2][2] = {{0, 0}, {0, 0}};
  for (int k = 0; k < n_chunks; k++) {
    const int32_t f0 = chunk_start[k];
    const int n = chunk_start[k + 1] - f0, first_img = sides * (k % banks) * chunk;
    for (int i = 0; i < n; i++)  // what the feature kernels of the chunk leave in its bank (an older chunk's counts are gone)
      for (int side = 0; side < sides; side++)
        for (int s = 0; s < 2; s++) hm_counts[(size_t)(first_img + sides * i + side) * 2 + s] = counts[((size_t)(f0 + i) * 2 + side) * 2 + s];
    seq_chunk_jobs(p, method, sides, f0, n, first_img, seq_slot_before(chunk_start, k, sides, banks, chunk), hm_counts.data(), nprev, Tr.data(), tr_valid,
                   jobs.data(), valid.data(), max_nq_out + 2 * k, seq_src.data());
    for (int i = 0; i < n; i++) debug_job_row(frames_out + (size_t)(f0 + i) * 7, jobs[i], valid[i], seq_src[f0 + i]);
  }
  return 0;
}

int32_t vsm_debug_pair_jobs(int32_t method, int32_t multi_stage, int32_t sides, int32_t n_frames, const int32_t *counts, const int32_t *pairs,
                            int32_t n_pairs, int32_t chunk, const uint8_t *tr_valid, int32_t *pairs_out, int32_t *max_nq_out) {
  if (sides < 1 || sides > 2 || chunk < 1 || !counts || !pairs_out || !max_nq_out || !pair_list_ok(method, n_frames, pairs, n_pairs)) return -1;
  vsm_params p;
  vsm_default_params(&p);
  p.multi_stage = multi_stage;
  std::vector<int32_t> img_counts((size_t)n_frames * sides * 2, 0);  // [frame][2 sides][set] -> [image][set]
  for (int32_t f = 0; f < n_frames; f++)
    for (int side = 0; side < sides; side++)
      for (int s = 0; s < 2; s++) img_counts[((size_t)f * sides + side) * 2 + s] = counts[((size_t)f * 2 + side) * 2 + s];
  std::vector<double> Tr((size_t)n_pairs * 12, 0.0);
  for (int32_t k = 0; k < n_pairs; k++) Tr[(size_t)k * 12] = (double)(k + 1);  // (says which pair's Tr a job took)
  std::vector<VsmJob> jobs(chunk);
  std::vector<char> valid(chunk);
  int32_t nchunks = 0;
  for (int32_t k0 = 0; k0 < n_pairs; k0 += chunk, nchunks++) {
    const int n = std::min(chunk, n_pairs - k0);
    pair_jobs(p, method, sides, img_counts.data(), pairs + 2 * (size_t)k0, n, Tr.data() + (size_t)k0 * 12, tr_valid ? tr_valid + k0 : nullptr, jobs.data(),
              valid.data(), max_nq_out + 2 * nchunks);
    for (int i = 0; i < n; i++) debug_job_row(pairs_out + (size_t)(k0 + i) * 7, jobs[i], valid[i], (int32_t)jobs[i].t[0]);
  }
  return nchunks;
}

// ---- the host stages alone ----
int32_t vsm_host_delaunay(const int32_t *x, const int32_t *y, int32_t n, int32_t *tris, int32_t cap, int32_t threads) {
  ExactDelaunay d;
  VsmForkJoin pool(threads);
  VsmPool side(2);  // with more than one thread the emulated vertex sort runs next to the triangulation (as in a handle)
  d.run(x, y, n, threads > 1 ? &pool : nullptr, threads > 1 ? &side : nullptr);
  return debug_triangles_out(d, tris, cap);
}

int32_t vsm_host_delaunay_split(const int32_t *x, const int32_t *y, int32_t n, int32_t *tris, int32_t cap,
                                int32_t max_task_points, int32_t device_top_points) {
  ExactDelaunay d;
  // (device_top_points < 0: additionally with the emulated vertex sort set apart, see ExactDelaunay::prepare)
  if (d.prepare(x, y, n, max_task_points, nullptr, std::max(device_top_points, 0), false, device_top_points < 0)) {
    d.solve_tasks();
    d.solve_merges();
    d.finish();
    d.resolve_ties();
    d.apply_ties();
  }
  return debug_triangles_out(d, tris, cap);
}

// test hook: prepare on the host; sub-trees and the merge nodes of at most device_top_points points on
// the GPU (vsm_dc.hip); the merges above them on the host
int32_t vsm_debug_delaunay_gpu(const int32_t *x, const int32_t *y, int32_t n, int32_t *tris, int32_t cap,
                               int32_t max_task_points, int32_t device_top_points, int32_t device_kd) {
  ExactDelaunay d;
  if (d.prepare(x, y, n, max_task_points, nullptr, std::max(device_top_points, 0), device_kd != 0)) {
    if (d.points() > VSM_DC_KD_MAX_POINTS) return -1;
    const DcMesh mesh = d.mesh();
    DcDeviceCopy dev;
    dev.device_kd = device_kd != 0;
    dev.blocks = device_top_points < 0;
    if (!dev.create(d, 1)) return -1;
    dev.load(mesh, nullptr);
    dev.launch(nullptr);
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    std::vector<VsmDcHull> hulls(dev.nn);
    (void)hipMemcpy(mesh.tri, dev.jobs[0].tri, dev.tri_bytes, hipMemcpyDeviceToHost);
    (void)hipMemcpy(mesh.pt, dev.jobs[0].pt, (size_t)dev.m * 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(mesh.id, dev.jobs[0].id, (size_t)dev.m * 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(hulls.data(), dev.jobs[0].hulls, sizeof(VsmDcHull) * dev.nn, hipMemcpyDeviceToHost);
    auto take = [&](int32_t q) {
      d.set_node_hull(q, ExactDelaunay::OTri{hulls[q].fl_t, hulls[q].fl_o}, ExactDelaunay::OTri{hulls[q].fr_t, hulls[q].fr_o});
    };
    for (const ExactDelaunay::Task &tk : d.tasks()) take(tk.node);
    for (const ExactDelaunay::Merge &mg : d.device_merges()) take(mg.node);
    d.finish();
  }
  return debug_triangles_out(d, tris, cap);
}

// micro-benchmark of the GPU side of the Delaunay stage: `njobs` copies of one prepared triangulation per
// launch sequence (sub-trees, then the merge levels up to device_top_points); returns microseconds per
// sequence (kernels only, HIP events), -1 on error
double vsm_debug_dc_bench(const int32_t *x, const int32_t *y, int32_t n, int32_t max_task_points, int32_t device_top_points,
                          int32_t device_kd, int32_t njobs, int32_t reps) {
  ExactDelaunay d;
  if (!d.prepare(x, y, n, max_task_points, nullptr, std::max(device_top_points, 0), device_kd != 0)) return -1;
  const DcMesh mesh = d.mesh();
  DcDeviceCopy dev;
  dev.device_kd = device_kd != 0;
  dev.blocks = device_top_points < 0;
  if (!dev.create(d, njobs)) return -1;
  DebugTimer timer;
  double total = 0;
  for (int r = 0; r < reps + 1; r++) {
    dev.load(mesh, nullptr);
    timer.start();
    dev.launch(nullptr);
    timer.stop();
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (r > 0) total += timer.us();
  }
  return total / reps;
}

// test hooks: which matches at shared pixels stand for their points, (index the radix-sorted keys carry, index
// Triangle's randomised vertex sort puts first) pairs - from the host emulation and from k_dc_ties; -1: not done
int32_t vsm_host_ties(const int32_t *x, const int32_t *y, int32_t n, int32_t *pairs, int32_t cap) {
  ExactDelaunay d;
  d.prepare(x, y, n, n, nullptr, 0, true, true);
  d.resolve_ties();
  const auto &t = d.ties();
  for (size_t k = 0; k < t.size() && (int32_t)k < cap; k++) {
    pairs[2 * k] = t[k].first;
    pairs[2 * k + 1] = t[k].second;
  }
  return (int32_t)t.size();
}

int32_t vsm_debug_ties_gpu(const int32_t *x, const int32_t *y, int32_t n, int32_t *pairs, int32_t cap, double *kernel_us) {
  ExactDelaunay d;
  d.prepare(x, y, n, n, nullptr, 0, true, true);
  VsmDcJob job;
  memset(&job, 0, sizeof(job));
  DebugDev<VsmDcJob> d_job;
  DebugDev<uint64_t> d_keys;
  DebugDev<int32_t> d_out;
  std::vector<int32_t> out(1 + 2 * VSM_DC_TIE_PATCHES, 0);
  if (!d_keys.alloc((size_t)std::max(n, 1)) || !d_out.alloc(out.size()) || !d_job.alloc(1)) return -2;
  (void)hipMemcpy(d_keys, d.tie_keys(), (size_t)n * 8, hipMemcpyHostToDevice);
  (void)hipMemset(d_out, 0, out.size() * 4);
  job.tie_keys = d_keys;
  job.tie_out = d_out;
  job.n_in = n;
  (void)hipMemcpy(d_job, &job, sizeof(job), hipMemcpyHostToDevice);
  DebugTimer timer;
  timer.start();
  vsm_dc_launch_ties(nullptr, d_job, 1);
  timer.stop();
  const bool ok = hipDeviceSynchronize() == hipSuccess;
  if (kernel_us) *kernel_us = timer.us();
  (void)hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost);
  if (!ok) return -2;
  for (int32_t k = 0; k < out[0] && k < cap; k++) {
    pairs[2 * k] = out[1 + 2 * k];
    pairs[2 * k + 1] = out[2 + 2 * k];
  }
  return out[0];
}

int32_t vsm_host_outliers_and_prior(const vsm_params *p, const vsm_p_match *list, int32_t n, int32_t method, vsm_p_match *out,
                                    int32_t cap, float *ranges, int32_t w, int32_t hh) {
  VsmHostWork wk;
  std::vector<vsm_p_match> m(list, list + std::max(n, 0));
  vsm_host_remove_outliers(wk, *p, m, method);
  return debug_survivors_out(*p, m, method, out, cap, ranges, w, hh);
}

int32_t vsm_host_outliers_and_prior_threads(const vsm_params *p, const vsm_p_match *list, int32_t n, int32_t method, vsm_p_match *out,
                                            int32_t cap, float *ranges, int32_t w, int32_t hh, int32_t threads) {
  if (threads <= 1) return vsm_host_outliers_and_prior(p, list, n, method, out, cap, ranges, w, hh);
  VsmForkJoin fj(std::min(threads, 64));
  VsmPool apart(2);  // (as in a handle: Triangle's emulated vertex sort runs beside the triangulation of lists from 1024 matches)
  VsmHostWork wk;
  wk.pool = &fj;
  wk.async = &apart;
  std::vector<vsm_p_match> m;
  if (n > 3) {  // vsm_match's final stage (early_xy): pixels first, then flows, votes, survivors
    std::vector<uint32_t> xy((size_t)n);
    for (int32_t i = 0; i < n; i++) xy[i] = (uint32_t)(int32_t)list[i].u1c | ((uint32_t)(int32_t)list[i].v1c << 16);
    vsm_host_outliers_begin_xy(wk, xy.data(), n);
    wk.del.run(wk.x.data(), wk.y.data(), n, wk.pool, wk.async);
    vsm_host_outliers_begin_flows(wk, list, n, method);
    vsm_host_outliers_end(wk, *p, list, n, method, m);
  } else {
    m.assign(list, list + std::max(n, 0));  // the reference leaves short lists alone (viso/matcher.cpp:1210)
  }
  return debug_survivors_out(*p, m, method, out, cap, ranges, w, hh);
}

int32_t vsm_debug_dc2(const vsm_params *p, const vsm_p_match *list, int32_t n, int32_t method, int32_t gpu_ties, int32_t copies,
                      vsm_p_match *out, int32_t cap, float *ranges, int32_t w, int32_t hh, double *kernel_us) {
  if (copies < 1) copies = 1;
  const int ub = (int)vsm_bins_along(w, p->match_binsize), vb = (int)vsm_bins_along(hh, p->match_binsize);
  if (ranges && ub * vb > 1024) return -2;
  Dc2Bank B;
  if (!B.reserve(copies, std::max(n, 64), true)) return -1;
  DebugDev<vsm_p_match> d_list, d_out;
  DebugDev<int32_t> d_cnt;
  DebugDev<float> d_ranges;
  const size_t ln = (size_t)std::max(n, 1), rn = (size_t)ub * vb * 16;  // records per list, floats per copy's boxes
  bool ok = d_list.alloc(ln) && d_out.alloc(ln * copies) && d_cnt.alloc(1) && d_ranges.alloc(rn * copies);
  int32_t result = -1;
  if (ok) {
    (void)hipMemcpy(d_list, list, (size_t)n * sizeof(vsm_p_match), hipMemcpyHostToDevice);
    (void)hipMemcpy(d_cnt, &n, 4, hipMemcpyHostToDevice);
    for (int i = 0; i < copies; i++) B.fill_job(i, d_list, d_cnt, gpu_ties != 0, d_out + (size_t)i * ln, nullptr, d_ranges + (size_t)i * rn);
    (void)hipMemcpy(B.d_jobs, B.h_jobs, sizeof(VsmDc2Job) * copies, hipMemcpyHostToDevice);
    DebugTimer timer;
    timer.start();
    dc2_enqueue_triangulation(nullptr, B, copies, n, gpu_ties != 0);
    if (!gpu_ties) {  // the host's verdicts (the look-ahead path computes them while the device triangulates)
      ok = hipDeviceSynchronize() == hipSuccess;
      for (int i = 0; i < copies && ok; i++) B.sort_ties_of(i);
    }
    // (VSM_DC2_EXPECT_LONG=0, tests: a list of 8193..16384 matches through the narrow form inside the LDS kernel, as in a handle
    // that has not met a long list yet)
    const char *xl = getenv("VSM_DC2_EXPECT_LONG");
    dc2_enqueue_mesh(nullptr, B, copies, n, g_no_prof, false, nullptr, xl ? atoi(xl) != 0 : true);
    dc2_enqueue_votes(nullptr, B, copies, n, method, (float)p->outlier_flow_tolerance, (float)p->outlier_disp_tolerance);
    if (ranges) vsm_dc2_launch_prior(nullptr, B.d_jobs, copies, method, p->match_binsize, p->match_radius, w, hh, ub, vb);
    timer.stop();
    ok = ok && hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
    if (kernel_us) *kernel_us = timer.us();
#ifdef VSM_DC2_DUMP_FILE  // debugging aid (tools/dc2_dump.py on a -DVSM_DC2_DUMP_FILE=\"path\" build): the first job's triangulation as the device left it
    {
      const char *dump = VSM_DC2_DUMP_FILE;  // debugging aid: the first job's triangulation as the device left it
      int32_t mn[2] = {0, 0};
      (void)hipMemcpy(mn, B.pp[0].mn, 8, hipMemcpyDeviceToHost);
      const int32_t mm = std::max(mn[0], 0);
      std::vector<int32_t> tri((size_t)mm * 16), idv(mm);
      std::vector<uint32_t> ptv(mm);
      (void)hipMemcpy(tri.data(), B.pp[0].tri, tri.size() * 4, hipMemcpyDeviceToHost);
      (void)hipMemcpy(ptv.data(), B.pp[0].pt, ptv.size() * 4, hipMemcpyDeviceToHost);
      (void)hipMemcpy(idv.data(), B.pp[0].id, idv.size() * 4, hipMemcpyDeviceToHost);
      if (FILE *f = fopen(dump, "wb")) {
        fwrite(mn, 4, 2, f);
        fwrite(tri.data(), 4, tri.size(), f);
        fwrite(ptv.data(), 4, ptv.size(), f);
        fwrite(idv.data(), 4, idv.size(), f);
        fclose(f);
      }
    }
#endif
    if (ok && *B.h_error) {
      result = -2;
    } else if (ok) {
      // every copy must have produced the same survivors
      std::vector<int32_t> cnt(copies);
      std::vector<vsm_p_match> first, other;
      bool same = true;
      for (int i = 0; i < copies && same; i++) {
        (void)hipMemcpy(&cnt[i], B.pp[i].out_count, 4, hipMemcpyDeviceToHost);
        same = cnt[i] == cnt[0] && cnt[i] >= 0 && cnt[i] <= n;
        if (!same) break;
        std::vector<vsm_p_match> &dst = i == 0 ? first : other;
        dst.resize(cnt[i]);
        if (cnt[i]) (void)hipMemcpy(dst.data(), d_out + (size_t)i * ln, (size_t)cnt[i] * sizeof(vsm_p_match), hipMemcpyDeviceToHost);
        if (i > 0) same = memcmp(first.data(), other.data(), (size_t)cnt[0] * sizeof(vsm_p_match)) == 0;
      }
      if (same) {
        result = cnt[0];
        for (int32_t i = 0; i < result && i < cap; i++) out[i] = first[i];
        if (ranges) (void)hipMemcpy(ranges, d_ranges + (size_t)(copies - 1) * rn, rn * 4, hipMemcpyDeviceToHost);
      } else {
        result = -3;
      }
    }
  }
  B.release();
  return result;
}

// ---- test hook of the compaction and its key store (k_compact_quad, k_compact_count / k_compact_write) ----
// P pairs in one launch, pair k with n_query[k] queries whose acceptance flags and raw records the caller gives.  Out per pair:
// the list (n_query[k] + 1 records), its count, the keys (key_cap[k] + VSM_DEBUG_KEY_GUARD words).  List and key arrays are
// filled with 0xA5 bytes before the launch, so whatever the kernels do not write - the guard entries behind each array, keys
// at and beyond the count or the capacity - comes back as that pattern.  old_keys = 1: the compaction without its key
// store, then k_dc2_keys over the lists (cap = key_cap[k]) - the hand-over the fused store replaces; 2: the fused store
// with its host-mapped second target, whose content comes back.
#define VSM_DEBUG_KEY_GUARD 8
int32_t vsm_debug_compact_keys(int32_t method, int32_t pass, int32_t P, const int32_t *n_query, const int32_t *const *flag, const vsm_p_match *const *raw,
                               const int32_t *key_cap, int32_t old_keys, vsm_p_match *const *list_out, int32_t *count_out, uint64_t *const *keys_out) {
  if (P < 1 || P > 64 || method < 0 || method > 2 || pass < 0 || pass > 1 || !n_query || !flag || !raw || !key_cap || !list_out || !count_out || !keys_out)
    return VSM_EARG;
  int max_nq = 0;
  int32_t max_cap = 0;
  for (int32_t k = 0; k < P; k++) {
    if (n_query[k] < 0 || n_query[k] > (1 << 20) || key_cap[k] < 0 || key_cap[k] > (1 << 20)) return VSM_EARG;
    max_nq = std::max(max_nq, n_query[k]);
    max_cap = std::max(max_cap, key_cap[k]);
  }
  std::vector<DebugPairs::Pair> want(P);
  std::vector<VsmJob> jobs(P, VsmJob());
  for (int32_t k = 0; k < P; k++) {
    DebugPairs::Pair &q = want[k];
    const size_t nq = (size_t)n_query[k];
    q.raw = q.list1 = nq + 1;
    q.one_list = true;
    q.flag = nq + 4;
    q.blockcnt = nq / 256 + 2;
    q.keys = (size_t)key_cap[k] + VSM_DEBUG_KEY_GUARD;
    q.key_cap = key_cap[k];
    q.n_in = nq;
    q.raw_in = raw[k];
    q.flag_in = flag[k];
    jobs[k].nq[pass] = n_query[k];
  }
  DebugPairs D;
  bool ok = D.create(nullptr, want, jobs, 0xA5, (size_t)P * sizeof(VsmDc2Job)) == hipSuccess;
  VsmDc2Job *d_dc = (VsmDc2Job *)D.extra;  // (old_keys = 1: k_dc2_keys' jobs over the lists)
  if (ok) {
    std::vector<VsmDc2Job> dc(P);
    for (int32_t k = 0; k < P; k++) {
      memset(&dc[k], 0, sizeof(VsmDc2Job));
      dc[k].list = D.pairs[k].list1;
      dc[k].count = D.pairs[k].count + pass;
      dc[k].cap = key_cap[k];
      dc[k].keys_in = D.pairs[k].keys[0];
    }
    ok = hipMemcpy(d_dc, dc.data(), (size_t)P * sizeof(VsmDc2Job), hipMemcpyHostToDevice) == hipSuccess;
  }
  // (old_keys = 2: the key store's second target, a host-mapped array per pair, is what comes back)
  uint8_t *hk = nullptr;
  uint64_t *hk_dev = nullptr;
  const size_t hk_stride = al256(((size_t)max_cap + VSM_DEBUG_KEY_GUARD) * 8);
  if (ok && old_keys == 2) {
    ok = hipHostMalloc((void **)&hk, hk_stride * P, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer((void **)&hk_dev, hk, 0) == hipSuccess;
    if (ok) memset(hk, 0xA5, hk_stride * P);
  }
  if (ok) {
    VsmJob dummy;
    memset(&dummy, 0, sizeof(dummy));
    const VsmKeyOut ko = {hk_dev, hk_stride, max_cap};
    vsm_launch_compact(nullptr, D.d_pairs, D.d_jobs, dummy, P, method, pass, max_nq, old_keys == 1 ? nullptr : &ko);
    if (old_keys == 1) vsm_dc2_launch_keys(nullptr, d_dc, P, max_nq);
    ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  }
  for (int32_t k = 0; k < P && ok; k++) {
    const size_t nk = (size_t)key_cap[k] + VSM_DEBUG_KEY_GUARD;
    ok = D.fetch_count(k, pass, &count_out[k]) == hipSuccess && D.fetch_list(k, 0, (size_t)n_query[k] + 1, list_out[k]) == hipSuccess &&
         D.fetch_keys(k, nk, keys_out[k]) == hipSuccess;
    if (ok && old_keys == 2) memcpy(keys_out[k], hk + hk_stride * k, nk * 8);
  }
  if (hk) (void)hipHostFree(hk);
  return ok ? VSM_OK : VSM_EHIP;
}

// ---- test hooks of the refinement kernels (k_refine<TILED>, k_parabolic_costs, k_parabolic_apply) on lists of the caller ----
int32_t vsm_debug_refine_check(int32_t w, int32_t hh, const vsm_p_match *const *lists, const int32_t *counts, int32_t P) {
  return refine_lists_check(w, hh, lists, counts, P);
}

int32_t vsm_debug_refine(vsm_handle *h, int32_t method, const vsm_p_match *const *lists, const int32_t *counts, int32_t P,
                         vsm_p_match *const *out, int32_t *out_counts) {
  if (!h || method < 0 || method > 2 || !out || !out_counts) return VSM_EARG;
  VsmCtx &c = h->ring;
  if (!c.ready) return VSM_ENOTREADY;
  const vsm_params &p = h->param;
  if (p.refinement != 1 && p.refinement != 2) return VSM_EARG;
  {
    const int rc = refine_lists_check(c.dims.w, c.dims.h, lists, counts, P);
    if (rc != VSM_OK) return rc;
  }
  HIPCHK(hipSetDevice(h->device));
  {
    const int rc = settle(h);
    if (rc != VSM_OK) return rc;
  }
  const int sc = h->cur, sp = h->cur ^ 1;
  if (!h->have[sc] || (method != 1 && !h->have[sp]) || (method != 0 && !h->right[sc]) || (method == 2 && !h->right[sp])) return VSM_ENOTREADY;
  for (int s = 0; s < 5; s++) h->stage[s].clear();
  h->stage3_in_hm = false;
  h->matched.clear();
  const VsmJob job = ring_job(h, method);
  int32_t n_upper = 0;
  for (int32_t k = 0; k < P; k++) n_upper = std::max(n_upper, counts[k]);
  DebugPairs D;
  HIPCHK(debug_lists_create(D, h->stream, lists, nullptr, counts, P, p.refinement == 2, job));
  vsm_launch_refine(h->stream, h->prof, c.d_imgs, D.d_pairs, D.d_jobs, job, P, c.dims, c.dims, method, p.refinement, n_upper);
  if (p.refinement == 2) vsm_launch_parabolic_apply(h->stream, h->prof, D.d_pairs, P);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  h->prof.resolve();
  HIPCHK(debug_lists_fetch(D, counts, P, p.refinement == 2, out, out_counts));
  return VSM_OK;
}

int32_t vsm_debug_parabolic_apply(const vsm_p_match *const *lists, const int32_t *const *records, const int32_t *counts, int32_t P,
                                  vsm_p_match *const *out, int32_t *out_counts) {
  if (P < 1 || P > VSM_DEBUG_REFINE_MAX_PAIRS || !lists || !records || !counts || !out || !out_counts) return VSM_EARG;
  for (int32_t k = 0; k < P; k++)
    if (counts[k] < 0 || counts[k] > VSM_PARA_MAX_LIST || (counts[k] > 0 && (!lists[k] || !records[k]))) return VSM_EARG;
  DebugPairs D;
  HIPCHK(debug_lists_create(D, nullptr, lists, records, counts, P, true, VsmJob()));
  vsm_launch_parabolic_apply(nullptr, g_no_prof, D.d_pairs, P);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(debug_lists_fetch(D, counts, P, true, out, out_counts));
  return VSM_OK;
}

int32_t vsm_host_parabolic_fits(const int32_t *records, int32_t n, float *uv, int32_t *ok) {
  if (n < 0 || (n > 0 && (!records || !uv || !ok))) return VSM_EARG;
  for (int32_t i = 0; i < n; i++) {
    const int32_t *r = records + (size_t)i * 12;
    ok[i] = vsm_host_parabolic_update(r + 3, r[1], r[2], uv[2 * i], uv[2 * i + 1]) ? 1 : 0;
  }
  return n;
}

}  // extern "C"
