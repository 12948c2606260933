// The first (host-shared) look-ahead form of vsm_sequence_run; part of vsm_api.cpp's translation unit (included there).
// The exact-Delaunay support test of a chunk's final lists is shared between the host pool and the GPU (DcChunk below);
// outlier removal and prior boxes of the pass-1 lists run on the pool.  vsm_sequence_run takes this form with option
// seq_v2 = 0 (VSM_SEQ_V2=0) and when the GPU-resident form (vsm_seq2.inc) declines a run.

// Look-ahead final stage, shared between host and GPU (vsm_dc.hip): per pair bank the pinned / device
// slabs that carry the prepared keys and task lists to the GPU and the triangle records back.
struct DcBank {
  int npairs = 0, stride_pts = 0, stride_tasks = 0;
  uint64_t *d_key = nullptr, *h_key = nullptr, *d_key_sorted = nullptr;  // h_key: (x,y) order, the GPU orders them (k_dc_kd_order)
  uint32_t *d_kd = nullptr;  // scratch of k_dc_kd_order
  float *d_flow = nullptr, *h_flow = nullptr;          // per pair [3][stride_pts]: flow u, flow v, disparity of every match
  int32_t *d_support = nullptr, *h_support = nullptr;  // per pair [stride_pts]: support count of every match
  uint32_t *d_pt = nullptr, *h_pt = nullptr;
  int32_t *d_id = nullptr, *h_id = nullptr, *d_tri = nullptr, *h_tri = nullptr;
  uint32_t *d_trip = nullptr, *h_trip = nullptr;  // packed triangle records, [2 * stride_pts][3] per pair (VsmDcJob::tri_packed)
  VsmDcTask *d_tasks = nullptr, *h_tasks = nullptr;
  VsmDcMerge *d_merges = nullptr, *h_merges = nullptr;  // stride_tasks per pair (a binary tree has fewer internal nodes than leaves)
  VsmDcHull *d_hulls = nullptr, *h_hulls = nullptr;    // by node number: 2 * stride_tasks per pair
  VsmDcJob *d_jobs = nullptr, *h_jobs = nullptr;
  std::vector<int32_t> m, nt, nn;  // per pair: distinct points, tasks (nt < 0: the host solves the sub-trees), tree nodes
  void release() {
    vsm_dev_free(d_key);
    vsm_dev_free(d_key_sorted);
    vsm_dev_free(d_kd);
    vsm_dev_free(d_flow);
    vsm_dev_free(d_support);
    (void)hipHostFree(h_flow);
    (void)hipHostFree(h_support);
    vsm_dev_free(d_pt);
    vsm_dev_free(d_id);
    vsm_dev_free(d_tri);
    vsm_dev_free(d_trip);
    (void)hipHostFree(h_trip);
    vsm_dev_free(d_tasks);
    vsm_dev_free(d_merges);
    vsm_dev_free(d_hulls);
    vsm_dev_free(d_jobs);
    (void)hipHostFree(h_key);
    (void)hipHostFree(h_pt);
    (void)hipHostFree(h_id);
    (void)hipHostFree(h_tri);
    (void)hipHostFree(h_tasks);
    (void)hipHostFree(h_merges);
    (void)hipHostFree(h_hulls);
    (void)hipHostFree(h_jobs);
    *this = DcBank();
  }
  bool reserve(int pairs, int pts, int tasks) {
    pts = (pts + 1) & ~1;  // (the long-list y order views two adjacent scratch arrays as 64-bit items)
    if (pairs <= npairs && pts <= stride_pts && tasks <= stride_tasks) return true;
    release();
    npairs = pairs;
    stride_pts = pts;
    stride_tasks = tasks;
    const size_t P = (size_t)pairs * pts, T = (size_t)pairs * tasks;
    bool ok = vsm_dev_alloc((void **)&d_key, P * 8) == hipSuccess && vsm_dev_alloc((void **)&d_key_sorted, P * 8) == hipSuccess &&
              vsm_dev_alloc((void **)&d_kd, P * 4 * VSM_DC_KD_SCRATCH) == hipSuccess && vsm_dev_alloc((void **)&d_pt, P * 4) == hipSuccess &&
              vsm_dev_alloc((void **)&d_flow, P * 12) == hipSuccess && vsm_dev_alloc((void **)&d_support, P * 4) == hipSuccess &&
              hipHostMalloc((void **)&h_flow, P * 12, hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void **)&h_support, P * 4, hipHostMallocDefault) == hipSuccess &&
              vsm_dev_alloc((void **)&d_id, P * 4) == hipSuccess && vsm_dev_alloc((void **)&d_tri, P * 64) == hipSuccess &&
              vsm_dev_alloc((void **)&d_trip, P * 24) == hipSuccess && hipHostMalloc((void **)&h_trip, P * 24, hipHostMallocDefault) == hipSuccess &&
              vsm_dev_alloc((void **)&d_tasks, T * sizeof(VsmDcTask)) == hipSuccess &&
              vsm_dev_alloc((void **)&d_merges, T * sizeof(VsmDcMerge)) == hipSuccess &&
              vsm_dev_alloc((void **)&d_hulls, 2 * T * sizeof(VsmDcHull)) == hipSuccess &&
              vsm_dev_alloc((void **)&d_jobs, pairs * sizeof(VsmDcJob)) == hipSuccess &&
              hipHostMalloc((void **)&h_key, P * 8, hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void **)&h_pt, P * 4, hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void **)&h_id, P * 4, hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void **)&h_tri, P * 64, hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void **)&h_tasks, T * sizeof(VsmDcTask), hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void **)&h_merges, T * sizeof(VsmDcMerge), hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void **)&h_hulls, 2 * T * sizeof(VsmDcHull), hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void **)&h_jobs, pairs * sizeof(VsmDcJob), hipHostMallocDefault) == hipSuccess;
    m.assign(pairs, 0);
    nt.assign(pairs, 0);
    nn.assign(pairs, 0);
    if (!ok) release();
    return ok;
  }
};

// ---------------------------------------------------------------------------------------
// Final stage of a look-ahead chunk (exact Delaunay support test), shared between host and GPU:
//   A  host pool, per pair: copy the exported list, per-match arrays, ExactDelaunay::prepare (emulated
//      sort, kd order, tree); keys and sub-tree tasks go to the bank's pinned slab
//   G  GPU, second stream: kd order of the keys, then all sub-trees of all pairs in one launch (k_dc_block: sub-trees of at
//      most VSM_DC_BLOCK_POINTS points, one wave each inside LDS), records back
//   B  host pool, per pair: adopt the records, the merges above the sub-trees, support, survivors
// The stages hand over to each other without the caller's thread: the last A task to finish enqueues
// G, a host function at the end of G submits B.  VSM_DC_GPU=0 keeps everything on the host.
// ---------------------------------------------------------------------------------------
struct DcChunk {
  vsm_handle *h = nullptr;
  VsmCtx *ctx = nullptr;
  vsm_params p;
  int method = 0;
  bool full = true;       // all merge levels and the support test on the GPU too: only the counts come back
  bool packed = false;    // (not full) the triangle records come back as 12-byte packed words (set when G is enqueued)
  int bank = 0, n = 0, f0 = 0, first_pair = 0, work0 = 0;
  std::shared_ptr<std::vector<char>> valid;
  std::atomic<int> a_left{0};
  DcBank *B = nullptr;         // its slabs
  VsmHostWork *work = nullptr; // its per-pair host state [n]
  int pass = 1;            // 1: the final stage (pass-2 lists -> seq_matches); 0: pass-1 lists, survivors stay in work[i].tmp_list
  hipStream_t stream = nullptr;
  int chunk = 0;           // the look-ahead chunk it belongs to
  bool submitted = false;  // dc_submit_a() has run (caller's thread only)
  bool a_waited = false;   // (caller's thread only)
  std::atomic<int> stage{0};  // 0: A running, 1: G enqueued, 2: B submitted
  std::atomic<bool> b_once{false};  // B is submitted by whoever comes first: the end of G, or dc_wait() giving up on it
  VsmPool::Ticket a, b;
  // VSM_DEBUG_TIMING: when the stages changed hands, and the task time summed over the pool
  double t_a0 = 0, t_g0 = 0, t_g1 = 0, t_b0 = 0, t_b1 = 0;
  std::atomic<long long> a_ns{0}, b_ns{0}, part_ns[8] = {};  // A: copy, arrays, prepare, slab; B: records, merges, support
  std::atomic<int> b_left{0};
};

// B for pair i of the chunk: the GPU's records adopted, the merges above them, support test, survivors
static void dc_task_b(DcChunk *ch, int i) {
  {
    const double t0 = vsm_now_us();
    if (!(*ch->valid)[i]) return;
    vsm_handle *h = ch->h;
    VsmHostWork &wk = ch->work[i];
    std::vector<vsm_p_match> dummy_out;
    std::vector<vsm_p_match> &out = ch->pass == 1 ? h->seq_matches[ch->f0 + i] : dummy_out;
    const int32_t nl = (int32_t)wk.tmp_list.size();
    if (nl <= 3) {  // the reference leaves short lists alone (:1210)
      if (ch->pass == 1) out.assign(wk.tmp_list.begin(), wk.tmp_list.end());
      return;
    }
    const DcBank &B = *ch->B;
    const int32_t m = B.m[i], nt = B.nt[i];
    if (ch->full && nt > 0) {  // the GPU went all the way: keep the matches with support >= 4 (:1369)
      const double t1 = vsm_now_us();
      const int32_t *support = B.h_support + (size_t)i * B.stride_pts;
      vsm_host_keep_supported(wk.tmp_list, support);  // in place, then the buffers change hands
      if (ch->pass == 1) out.swap(wk.tmp_list);
      ch->part_ns[6].fetch_add((long long)((vsm_now_us() - t1) * 1e3), std::memory_order_relaxed);
      return;
    }
    if (m >= 2) {
      if (nt > 0) {  // adopt what the GPU built
        // (copied, not used in place: the merges and the support test chase pointers through these arrays, and
        // on the pinned slab - small pages, no prefetch-friendly order - that cost 25 % of the whole run)
        const DcMesh mesh = wk.del.mesh();
        if (ch->packed) {
          const uint32_t *src = B.h_trip + (size_t)i * B.stride_pts * 6;
          int32_t *dst = mesh.tri;
          for (int32_t t = 0; t < 2 * m; t++, src += 3, dst += 8) {
            for (int o = 0; o < 3; o++) {
              const uint32_t wv = src[o], nb = wv & 0x1ffffu, vx = wv >> 17;
              dst[o] = nb == 0x1ffffu ? -1 : (int32_t)nb;
              dst[4 + o] = vx == 0x7fffu ? -1 : (int32_t)vx;
            }
          }
        } else {
          memcpy(mesh.tri, B.h_tri + (size_t)i * B.stride_pts * 16, (size_t)m * 16 * sizeof(int32_t));
        }
        memcpy(mesh.pt, B.h_pt + (size_t)i * B.stride_pts, (size_t)m * 4);
        memcpy(mesh.id, B.h_id + (size_t)i * B.stride_pts, (size_t)m * 4);
        const VsmDcHull *hu = B.h_hulls + (size_t)i * 2 * B.stride_tasks;
        auto take = [&](int32_t q) { wk.del.set_node_hull(q, ExactDelaunay::OTri{hu[q].fl_t, hu[q].fl_o}, ExactDelaunay::OTri{hu[q].fr_t, hu[q].fr_o}); };
        for (const ExactDelaunay::Task &tk : wk.del.tasks()) take(tk.node);
        for (const ExactDelaunay::Merge &mg : wk.del.device_merges()) take(mg.node);
      } else {
        wk.del.order_keys();
        wk.del.solve_tasks();
        wk.del.solve_merges();
      }
      const double t1 = vsm_now_us();
      ch->part_ns[4].fetch_add((long long)((t1 - t0) * 1e3), std::memory_order_relaxed);
      wk.del.finish();
      ch->part_ns[5].fetch_add((long long)((vsm_now_us() - t1) * 1e3), std::memory_order_relaxed);
    }
    const double t2 = vsm_now_us();
    vsm_host_count_support(wk, ch->p, nl, ch->method);
    vsm_host_keep_supported(wk.tmp_list, wk.support.data());  // in place, then the buffers change hands
    if (ch->pass == 1) out.swap(wk.tmp_list);
    ch->part_ns[6].fetch_add((long long)((vsm_now_us() - t2) * 1e3), std::memory_order_relaxed);
  }
}

static void dc_submit_b(DcChunk *ch) {
  vsm_handle *h = ch->h;
  ch->t_b0 = vsm_now_us();
  ch->b_left.store(ch->n, std::memory_order_relaxed);
  ch->b = h->pool->submit(ch->n, [ch](int i) {
    const double t0 = vsm_now_us();
    dc_task_b(ch, i);
    ch->b_ns.fetch_add((long long)((vsm_now_us() - t0) * 1e3), std::memory_order_relaxed);
    if (ch->b_left.fetch_sub(1, std::memory_order_acq_rel) == 1) ch->t_b1 = vsm_now_us();
  });
  ch->stage.store(2, std::memory_order_release);
}

static void dc_after_gpu(void *arg) {  // runs on a HIP runtime thread: no HIP calls
  DcChunk *ch = (DcChunk *)arg;
  ch->t_g1 = vsm_now_us();
  if (!ch->b_once.exchange(true)) dc_submit_b(ch);
}

// from the pool thread that finished the chunk's last A task; wait_here: from the caller's thread, which waits for the
// GPU's part itself and submits nothing (pass 0)
static void dc_enqueue_gpu(DcChunk *ch, bool wait_here = false) {
  vsm_handle *h = ch->h;
  (void)hipSetDevice(h->device);
  ch->t_g0 = vsm_now_us();
  DcBank &B = *ch->B;
  int maxt = 0, maxm = 0, maxin = 0, maxn = 0, maxlev = 0, maxg = 0, lev_nodes[VSM_DC_MAX_LEVELS] = {0};
  for (int i = 0; i < ch->n; i++) {
    VsmDcJob &jb = B.h_jobs[i];  // (the A task left the level table in it)
    jb.key = B.d_key + (size_t)i * B.stride_pts;
    jb.key_sorted = B.nt[i] > 0 ? B.d_key_sorted + (size_t)i * B.stride_pts : nullptr;
    jb.kd_scratch = B.d_kd + (size_t)i * B.stride_pts * VSM_DC_KD_SCRATCH;
    jb.kd_stride = B.stride_pts;
    jb.pt = B.d_pt + (size_t)i * B.stride_pts;
    jb.id = B.d_id + (size_t)i * B.stride_pts;
    jb.tri = B.d_tri + (size_t)i * B.stride_pts * 16;
    jb.tasks = B.d_tasks + (size_t)i * B.stride_tasks;
    jb.merges = B.d_merges + (size_t)i * B.stride_tasks;
    jb.hulls = B.d_hulls + (size_t)i * 2 * B.stride_tasks;
    jb.flow_u = B.d_flow + (size_t)i * 3 * B.stride_pts;
    jb.flow_v = jb.flow_u + B.stride_pts;
    jb.disp = jb.flow_v + B.stride_pts;
    jb.support = ch->full ? B.d_support + (size_t)i * B.stride_pts : nullptr;
    jb.ntasks = std::max(B.nt[i], 0);
    jb.m = B.m[i];
    maxt = std::max(maxt, jb.ntasks);
    if (B.nt[i] > 0) {
      maxm = std::max(maxm, B.m[i]);
      maxin = std::max(maxin, jb.n_in);
      maxn = std::max(maxn, B.nn[i]);
      maxlev = std::max(maxlev, jb.nlevels);
      maxg = std::max(maxg, jb.level_off[jb.nlevels]);
      for (int l = 0; l < jb.nlevels; l++) lev_nodes[l] = std::max(lev_nodes[l], jb.level_off[l + 1] - jb.level_off[l]);
    } else {
      jb.nlevels = 0;
    }
  }
  ch->packed = !ch->full && maxm > 0 && maxm <= VSM_DC_PACKED_MAX_POINTS;
  for (int i = 0; i < ch->n; i++) B.h_jobs[i].tri_packed = ch->packed ? B.d_trip + (size_t)i * B.stride_pts * 6 : nullptr;
  // only the used part of every pair's slab row travels: rows of maxm points / maxt tasks
  const size_t sp = (size_t)B.stride_pts, st = (size_t)B.stride_tasks, rows = (size_t)ch->n;
  hipStream_t s2 = ch->stream;
  bool ok = true;
  if (maxt > 0) {
    ok = hipMemcpy2DAsync(B.d_key_sorted, sp * 8, B.h_key, sp * 8, (size_t)maxm * 8, rows, hipMemcpyHostToDevice,
                          s2) == hipSuccess &&
         hipMemcpy2DAsync(B.d_tasks, st * sizeof(VsmDcTask), B.h_tasks, st * sizeof(VsmDcTask), (size_t)maxt * sizeof(VsmDcTask), rows,
                          hipMemcpyHostToDevice, s2) == hipSuccess &&
         (maxg == 0 || hipMemcpy2DAsync(B.d_merges, st * sizeof(VsmDcMerge), B.h_merges, st * sizeof(VsmDcMerge),
                                        (size_t)maxg * sizeof(VsmDcMerge), rows, hipMemcpyHostToDevice, s2) == hipSuccess) &&
         hipMemcpyAsync(B.d_jobs, B.h_jobs, ch->n * sizeof(VsmDcJob), hipMemcpyHostToDevice, s2) == hipSuccess;
    if (ok) {
      VsmProf &pf = h->prof;
      pf.begin(VSM_K_DC_KD, s2);
      vsm_dc_launch_kd_order(s2, B.d_jobs, ch->n);
      pf.end(s2);
      pf.begin(VSM_K_DC_BLOCK, s2);
      vsm_dc_launch_blocks(s2, B.d_jobs, ch->n, maxt);  // (writes every slot of every sub-tree: no fill of d_tri in front)
      pf.end(s2);
      if (maxlev > 0) {
        pf.begin(VSM_K_DC_MERGE, s2);
        for (int l = 0; l < maxlev; l++) vsm_dc_launch_merge_level(s2, B.d_jobs, ch->n, l, lev_nodes[l]);
        pf.end(s2);
      }
      if (ch->full) {
        // the triangulations are complete on the device: count the support there, only the counts travel
        ok = hipMemcpy2DAsync(B.d_flow, sp * 12, B.h_flow, sp * 12, sp * 12, rows, hipMemcpyHostToDevice, s2) == hipSuccess &&
             hipMemset2DAsync(B.d_support, sp * 4, 0, (size_t)maxin * 4, rows, s2) == hipSuccess;
        if (ok) {
          pf.begin(VSM_K_DC_SUPPORT, s2);
          vsm_dc_launch_support(s2, B.d_jobs, ch->n, maxm, ch->method, (float)ch->p.outlier_flow_tolerance, (float)ch->p.outlier_disp_tolerance);
          pf.end(s2);
          ok = hipMemcpy2DAsync(B.h_support, sp * 4, B.d_support, sp * 4, (size_t)maxin * 4, rows, hipMemcpyDeviceToHost, s2) == hipSuccess;
        }
      } else {
        ok = (ch->packed ? hipMemcpy2DAsync(B.h_trip, sp * 24, B.d_trip, sp * 24, (size_t)maxm * 24, rows, hipMemcpyDeviceToHost, s2)
                         : hipMemcpy2DAsync(B.h_tri, sp * 64, B.d_tri, sp * 64, (size_t)maxm * 64, rows, hipMemcpyDeviceToHost, s2)) == hipSuccess &&
             hipMemcpy2DAsync(B.h_pt, sp * 4, B.d_pt, sp * 4, (size_t)maxm * 4, rows, hipMemcpyDeviceToHost, s2) == hipSuccess &&
             hipMemcpy2DAsync(B.h_id, sp * 4, B.d_id, sp * 4, (size_t)maxm * 4, rows, hipMemcpyDeviceToHost, s2) == hipSuccess &&
             hipMemcpy2DAsync(B.h_hulls, 2 * st * sizeof(VsmDcHull), B.d_hulls, 2 * st * sizeof(VsmDcHull), (size_t)maxn * sizeof(VsmDcHull),
                              rows, hipMemcpyDeviceToHost, s2) == hipSuccess;
      }
    }
  }
  ch->stage.store(1, std::memory_order_release);
  if (wait_here) {
    if (maxt > 0 && !(ok && hipStreamSynchronize(s2) == hipSuccess)) {
      (void)hipStreamSynchronize(s2);
      for (int i = 0; i < ch->n; i++)
        if (B.nt[i] > 0) B.nt[i] = -1;
    }
    return;
  }
  // (option dc_fault_inject = 1, tests only: the completion callback is "lost" - dc_wait()'s watchdog has to notice)
  const bool lose_callback = ch->h->sw.dc_fault_inject == 1;
  if (ok && maxt > 0 && lose_callback) return;
  if (ok && maxt > 0 && hipLaunchHostFunc(s2, dc_after_gpu, ch) == hipSuccess) return;
  // nothing for the GPU, or it could not be used: the host solves the sub-trees too
  if (maxt > 0) {
    (void)hipStreamSynchronize(s2);
    for (int i = 0; i < ch->n; i++)
      if (B.nt[i] > 0) B.nt[i] = -1;
  }
  if (!ch->b_once.exchange(true)) dc_submit_b(ch);
}

// A for pair i of the chunk: the list out of host-mapped memory, the per-match arrays, the host's part of the triangulation
static void dc_task_a(DcChunk *ch, int i) {
  {
    const double t0 = vsm_now_us();
    VsmHostWork &wk = ch->work[i];
    DcBank &B = *ch->B;
    B.m[i] = 0;
    B.nt[i] = 0;
    wk.tmp_list.clear();
    if ((*ch->valid)[i]) {
      const int pj = ch->first_pair + i;
      // one wide copy out of the host-mapped export, then cache-resident work
      if (ch->pass == 1)
        wk.tmp_list.assign(ch->ctx->hm_list2[pj], ch->ctx->hm_list2[pj] + ch->ctx->hm_lcount[2 * pj + 1]);
      else
        wk.tmp_list.assign(ch->ctx->hm_list1[pj], ch->ctx->hm_list1[pj] + ch->ctx->hm_lcount[2 * pj]);
      const int32_t nl = (int32_t)wk.tmp_list.size();
      const double t1 = vsm_now_us();
      ch->part_ns[0].fetch_add((long long)((t1 - t0) * 1e3), std::memory_order_relaxed);
      if (nl > 3) {
        vsm_host_outliers_begin(wk, wk.tmp_list.data(), nl, ch->method);
        const double t2 = vsm_now_us();
        ch->part_ns[1].fetch_add((long long)((t2 - t1) * 1e3), std::memory_order_relaxed);
        // (the kd order of the keys is left to the GPU: defer_order)
        const bool prepared = wk.del.prepare(wk.x.data(), wk.y.data(), nl, VSM_DC_BLOCK_POINTS, nullptr, ch->full ? INT32_MAX : 0, true);
        ch->part_ns[2].fetch_add((long long)((vsm_now_us() - t2) * 1e3), std::memory_order_relaxed);
        if (prepared) {
          const int32_t m = wk.del.points(), nt = (int32_t)wk.del.tasks().size(), ng = (int32_t)wk.del.device_merges().size();
          const std::vector<int32_t> &lv = wk.del.device_levels();
          B.m[i] = m;
          B.nn[i] = wk.del.num_nodes();
          if (m < nl) ch->part_ns[7].fetch_add(1, std::memory_order_relaxed);  // pairs with duplicate points
          if (m > B.stride_pts || nl > B.stride_pts || nt > B.stride_tasks || ng > B.stride_tasks || B.nn[i] > 2 * B.stride_tasks ||
              (int)lv.size() > VSM_DC_MAX_LEVELS || m > VSM_DC_KD_MAX_POINTS) {
            B.nt[i] = -1;  // does not fit the slab: this pair stays on the host
          } else {
            memcpy(B.h_key + (size_t)i * B.stride_pts, wk.del.mesh().key, (size_t)m * 8);
            memcpy(B.h_tasks + (size_t)i * B.stride_tasks, wk.del.tasks().data(), (size_t)nt * sizeof(VsmDcTask));
            memcpy(B.h_merges + (size_t)i * B.stride_tasks, wk.del.device_merges().data(), (size_t)ng * sizeof(VsmDcMerge));
            if (ch->full) {
              float *fl = B.h_flow + (size_t)i * 3 * B.stride_pts;
              memcpy(fl, wk.fu.data(), (size_t)nl * 4);
              memcpy(fl + B.stride_pts, wk.fv.data(), (size_t)nl * 4);
              memcpy(fl + 2 * (size_t)B.stride_pts, wk.dp.data(), (size_t)nl * 4);
            }
            VsmDcJob &jb = B.h_jobs[i];
            jb.n_in = nl;
            jb.nlevels = (int32_t)lv.size();
            jb.level_off[0] = 0;
            for (int l = 0; l < jb.nlevels; l++) jb.level_off[l + 1] = jb.level_off[l] + lv[l];
            B.nt[i] = nt;
          }
        }
      }
    }
    ch->a_ns.fetch_add((long long)((vsm_now_us() - t0) * 1e3), std::memory_order_relaxed);
  }
}

static void dc_submit_a(DcChunk *ch) {
  ch->submitted = true;
  ch->a_left.store(ch->n, std::memory_order_relaxed);
  ch->t_a0 = vsm_now_us();
  ch->a = ch->h->pool->submit(ch->n, [ch](int i) {
    dc_task_a(ch, i);
    if (ch->a_left.fetch_sub(1, std::memory_order_acq_rel) == 1) dc_enqueue_gpu(ch);  // the last one hands over
  });
}

// Until the chunk's final lists are in seq_matches.  The GPU's part normally takes a millisecond or two and reports back
// through a host function on its stream.  If nothing has been heard after the watchdog time (option dc_watchdog_ms, default
// 20 s) the stream itself is asked: hipStreamSynchronize() either returns an error - the device faulted; that is logged
// with HIP's own message, remembered in the handle (no GPU share from then on) and reported by vsm_sequence_run as
// VSM_EHIP - or it returns success, in which case the device's results are complete and only the callback went missing.
// Either way nothing on the device can touch the chunk's slabs any more when the host takes over, and the chunk and
// its bank stay alive until then (they are owned by vsm_sequence_run, which calls this for every chunk before it returns).
static void dc_wait(DcChunk *ch) {
  vsm_handle *h = ch->h;
  const double watchdog_us = (double)h->sw.dc_watchdog_ms * 1e3;
  if (!ch->submitted) return;  // (left early, between setting it up and submitting it: nothing of it is in flight)
  const double t0 = vsm_now_us();
  while (ch->stage.load(std::memory_order_acquire) < 2) {
    std::this_thread::sleep_for(std::chrono::microseconds(50));
    if (ch->stage.load(std::memory_order_acquire) == 1 && vsm_now_us() - t0 > watchdog_us && !ch->b_once.exchange(true)) {
      const hipError_t e = hipStreamSynchronize(ch->stream);  // (blocks until the stream has drained or failed)
      if (e != hipSuccess) {
        fprintf(stderr, "visomatch: the GPU share of the Delaunay stage failed (%s); finishing the chunk on the host, no GPU share from now on\n",
                hipGetErrorString(e));
        h->dc_gpu_broken = true;
        h->seq_hip_error.store(1);
        DcBank &B = *ch->B;
        for (int i = 0; i < ch->n; i++)
          if (B.nt[i] > 0) B.nt[i] = -1;
        ch->full = false;
      } else {
        fprintf(stderr, "visomatch: the GPU share of the Delaunay stage finished without reporting back; continuing with its results\n");
      }
      dc_submit_b(ch);
    }
  }
  h->pool->wait(ch->b);
}

// The first form's call, on the caller's thread (the result vectors are reset by vsm_sequence_run).
static int sequence_run_v1(vsm_handle *h, const uint8_t *left, const uint8_t *right, int64_t frame_stride, int on_device, int32_t n_frames,
                           int32_t w, int32_t hh, int32_t bpl, int32_t method, const double *Tr, const uint8_t *Tr_valid) {
  const double t_entry = now_us();
  const vsm_params &p = h->param;
  int C = h->sw.seq_chunk > 0 ? h->sw.seq_chunk : 50;
  if (C > n_frames) C = n_frames;
  VsmCtx &c = h->seq;
  if (!c.holds(w, hh, 3 * C, 2 * C) || h->seq_chunk != C) {
    (void)hipStreamSynchronize(h->stream);
    int rc = ctx_create(c, p, w, hh, 3 * C, 2 * C, h->stream, h->sw.match_heads != 0);  // three banks of frames, two of pairs
    if (rc != VSM_OK) return rc;
    h->seq_chunk = C;
  }
  // Software pipeline over chunks.  GPU order: pass 1 of chunk k, features of chunk k+1, pass 2 of
  // chunk k - so the GPU has the next chunk's features to compute while the pool does chunk k's
  // prior statistics, and the caller's thread never waits for features.  Frames live in three banks
  // (chunk k+1's features must not overwrite the last frame of chunk k-1, which chunk k's first pair
  // reads); pairs in two (the final host stage of chunk k reads pair bank k&1 in host-mapped memory
  // while the GPU runs chunk k+1 on the other).
  std::vector<VsmPool::Ticket> tickets;  // final stages that stay on the host ...
  std::vector<int> ticket_chunk;         // ... and the chunk each belongs to
  // final stage: see DcChunk above
  // (options dc_gpu / dc_full, vsm_set_option)
  const VsmSwitches &sw = h->sw;
  const bool dc_env = sw.dc_gpu != 0;
  const bool dc_forced = sw.dc_gpu > 0;
  // the merges above the sub-trees and the support test on the GPU too: a third less host work per
  // pair, but the large merges are slow there (a dependent L2 round trip per step), so it pays when the host has
  // few cores for this rank (200 frames 1242x375, ms: 16 threads 9.1 shared / 14.2 full, 8: 12.9 / 14.9, 4: 21.5 / 18.6,
  // 2: 33.1 / 25.8; host only: 14.0, 25.3, 43.4, 70.8); option dc_full = 0 / 1 decides otherwise
  const bool dc_full = sw.dc_full >= 0 ? sw.dc_full != 0 : h->pool->size() <= 6;
  bool dc_gpu = dc_env && !h->dc_gpu_broken;
  h->seq_hip_error.store(0);
  for (hipStream_t &st : h->dc_stream)
    if (dc_gpu && !st) dc_gpu = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;  // (stream priorities make no measurable difference)
  if (dc_gpu) {
    for (int b = 0; b < vsm_handle::kDcBanks; b++)
      if (!h->dc_bank[b]) h->dc_bank[b] = new DcBank();
    if ((int)h->seq_work.size() < vsm_handle::kDcBanks * C) h->seq_work.resize((size_t)vsm_handle::kDcBanks * C);
  }
  std::vector<std::unique_ptr<DcChunk>> chunks;
  struct Drain {  // whatever way this function is left, nothing of it may still be running
    std::vector<std::unique_ptr<DcChunk>> &c;
    ~Drain() {
      for (auto &ch : c) dc_wait(ch.get());
    }
  } drain{chunks};
  const int32_t dims_c[3] = {w, hh, c.dims.bpl};
  int32_t nprev[2][2] = {{0, 0}, {0, 0}};  // feature counts [side][set] of the previous chunk's last frame
  double tg = 0, thost = 0;
  std::atomic<long long> mid_ns[2] = {};  // VSM_DEBUG_TIMING: pass-1 outlier removal, prior statistics (task time)
  const double tstart = now_us();
  const std::vector<int32_t> chunk_start = seq1_plan(n_frames, C);  // (vsm_jobs.h)
  const int nchunks = (int)chunk_start.size() - 1;
  auto launch_features_of = [&](int k) -> hipError_t {  // ingest + all feature kernels of chunk k, then the marker
    const int32_t f0 = chunk_start[k];
    const int n = chunk_start[k + 1] - f0;
    const int first_img = 2 * (k % 3) * C;
    if (on_device) {
      enqueue_front_frames(h, c, first_img, 2, left + (size_t)f0 * frame_stride, (size_t)frame_stride, right + (size_t)f0 * frame_stride,
                           (size_t)frame_stride, bpl, n);
    } else {
      if (seq_ingest_host_frames(h, c, first_img, left, right, frame_stride, bpl, w, hh, f0, n) != VSM_OK) return hipErrorUnknown;
    }
    enqueue_features(h, c, first_img, 2 * n);
    return hipEventRecord(h->seq_ev[0], h->stream);
  };
  // what a chunk needs from one step to the next
  struct SeqChunk {
    int32_t f0 = 0;
    int n = 0, bank = 0, first_img = 0, first_pair = 0;
    int max_nq[2] = {0, 0};
    std::shared_ptr<std::vector<char>> validp;
    DcChunk *dc = nullptr;  // its final stage, if that is shared with the GPU
    double t_pass2 = 0;
  };
  std::vector<SeqChunk> sc(nchunks);
  // First step of chunk k: wait for its features, one job per frame, pass 1 (if there is one) and its export.
  // Order on the stream: ... pass 2 of k-1, features of k+1, pass 1 of k+1, pass 2 of k, features of k+2 ...: while the
  // pool computes chunk k's prior statistics the GPU has pass 2 of chunk k-1 and the features of chunk k+1 to do, and
  // pass 1 of chunk k+1 is over before its prior statistics are wanted.
  auto start_chunk = [&](int k, bool then_features) -> int {
    SeqChunk &q = sc[k];
    q.f0 = chunk_start[k];
    q.n = chunk_start[k + 1] - q.f0;
    q.bank = k & 1;
    q.first_img = 2 * (k % 3) * C;
    q.first_pair = q.bank * C;
    const int32_t f0 = q.f0;
    const int n = q.n, first_img = q.first_img, first_pair = q.first_pair;
    const VsmPair *d_pairs = c.d_pairs + first_pair;
    VsmJob *h_jobs = c.h_jobs + first_pair, *d_jobs = c.d_jobs + first_pair;
    int *max_nq = q.max_nq;
    const double tl0 = now_us();
    HIPCHK(hipEventSynchronize(h->seq_ev[0]));  // the chunk's feature counts are in host-mapped memory
    HIPCHK(hipGetLastError());
    if (vsm_debug_timing()) fprintf(stderr, "  chunk %d: feature wait %.0f us\n", k, now_us() - tl0);
    // ---- one job per frame of the chunk ----
    q.validp = std::make_shared<std::vector<char>>(n, 0);
    seq_chunk_jobs(p, method, 2, f0, n, first_img, seq_slot_before(chunk_start, k, 2, 3, C), c.hm_counts, nprev, Tr, Tr_valid, h_jobs,
                   q.validp->data(), max_nq, h->seq_src.data());
    HIPCHK(vsm_upload(h->stream, d_jobs, h_jobs, sizeof(VsmJob) * n));
    if (p.multi_stage) {
      VsmMatchCfg cfg = make_cfg(p, method, h->sw.match_heads && c.has_heads);
      VsmJob dummy;
      memset(&dummy, 0, sizeof(dummy));
      cfg.sparse = 1;
      cfg.use_prior = 0;
      vsm_launch_match(h->stream, h->prof, c.d_imgs, d_pairs, d_jobs, dummy, n, c.dims, cfg, max_nq[0]);
      vsm_launch_export(h->stream, h->prof, d_pairs, n, 0, max_nq[0]);
      HIPCHK(hipEventRecord(h->seq_ev[1], h->stream));
    }
    if (then_features && k + 1 < nchunks) HIPCHK(launch_features_of(k + 1));
    return VSM_OK;
  };
  // Last step of chunk j: its pass 2 is over, the final stage goes to the pool (and from there to the GPU and back)
  VsmCtx *cp = &c;
  auto finalize = [&](int j) -> int {
    const SeqChunk &q = sc[j];
    const double t0 = now_us();
    HIPCHK(hipEventSynchronize(h->idle_wait));
    HIPCHK(hipGetLastError());
    // (kernel timing: the spans are read once, after the last chunk - the event pool grows over the sequence instead of
    // the pipeline being drained per chunk, so the profiled pass overlaps its kernels like any other)
    // (kernel timing is resolved at the end of the run, when the Delaunay streams have drained too)
    if (vsm_debug_timing()) fprintf(stderr, "  chunk %d: pass2 launched %.0f us ago, waited %.0f us for it\n", j, t0 - q.t_pass2, now_us() - t0);
    tg += now_us() - t0;
    if (q.dc) {
      dc_submit_a(q.dc);
    } else {
      const vsm_params pcopy = p;
      const std::shared_ptr<std::vector<char>> validp = q.validp;
      const int32_t f0 = q.f0;
      const int first_pair = q.first_pair;
      ticket_chunk.push_back(j);
      tickets.push_back(h->pool->submit(q.n, [h, cp, pcopy, validp, f0, first_pair, method](int i) {
        if (!(*validp)[i]) return;
        static thread_local VsmHostWork tw;
        const int pj = first_pair + i;
        std::vector<vsm_p_match> &out = h->seq_matches[f0 + i];
        // one wide copy out of the host-mapped export, then cache-resident work
        tw.tmp_list.assign(cp->hm_list2[pj], cp->hm_list2[pj] + cp->hm_lcount[2 * pj + 1]);
        vsm_host_remove_outliers_from(tw, pcopy, tw.tmp_list.data(), (int32_t)tw.tmp_list.size(), method, out);
      }));
    }
    return VSM_OK;
  };
  HIPCHK(launch_features_of(0));
  {
    const int rc = start_chunk(0, true);
    if (rc != VSM_OK) return rc;
  }
  for (int32_t k = 0; k < nchunks; k++) {
    const SeqChunk &q = sc[k];
    const int32_t f0 = q.f0;
    const int n = q.n, first_pair = q.first_pair;
    const VsmPair *d_pairs = c.d_pairs + first_pair;
    const VsmJob *d_jobs = c.d_jobs + first_pair;
    const int *max_nq = q.max_nq;
    const std::shared_ptr<std::vector<char>> validp = q.validp;
    const std::vector<char> &valid = *validp;
    VsmMatchCfg cfg = make_cfg(p, method, h->sw.match_heads && c.has_heads);
    VsmJob dummy;
    memset(&dummy, 0, sizeof(dummy));
    double ta = now_us();
    if (p.multi_stage) {
      const double tl1 = now_us();
      HIPCHK(hipEventSynchronize(h->seq_ev[1]));
      double tb = now_us();
      if (vsm_debug_timing()) fprintf(stderr, "  chunk %d: pass1 sync %.0f us\n", k, tb - tl1);
      tg += tb - ta;
      // (the pool's tasks queue behind the previous chunk's final stage: FIFO)
      HIPCHK(host_pass1_boxes(h, c, first_pair, n, valid.data(), method, dims_c, mid_ns));
      ta = now_us();
      thost += ta - tb;
    }
    if (k > 0) {  // pass 2 of the previous chunk ran meanwhile
      const int rc = finalize(k - 1);
      if (rc != VSM_OK) return rc;
    }
    if (k + 1 < nchunks) {  // pass 1 of the next chunk goes in front of this chunk's pass 2
      const int rc = start_chunk(k + 1, false);
      if (rc != VSM_OK) return rc;
    }
    ta = now_us();
    // the export below overwrites this pair bank's host lists: chunk k-2 must be done with them
    const double tw0 = now_us();
    for (auto &ch : chunks)  // (they copied the lists out first thing)
      if (ch->chunk <= k - 2 && !ch->a_waited) {
        h->pool->wait(ch->a);
        ch->a_waited = true;
      }
    for (size_t q = 0; q < tickets.size(); q++)
      if (ticket_chunk[q] <= k - 2 && tickets[q]) {
        h->pool->wait(tickets[q]);
        tickets[q].reset();
      }
    if (vsm_debug_timing() && now_us() - tw0 > 2000) fprintf(stderr, "  chunk %d: waited %.0f us for chunk %d's final stage\n", k, now_us() - tw0, k - 2);
    // The GPU share pays when the pool has other pairs to work on while the GPU has this chunk's (its part is
    // latency-bound): a chunk with fewer pairs than pool threads stays on the host, unless VSM_DC_GPU=1 insists
    bool use_dc = dc_gpu && (dc_forced || n >= h->pool->size());
    const int dc_q = (int)chunks.size(), dc_b = dc_q % vsm_handle::kDcBanks;
    if (use_dc) {
      if (dc_q >= vsm_handle::kDcBanks) dc_wait(chunks[dc_q - vsm_handle::kDcBanks].get());  // its slabs are reused now
      // slab sizes from this chunk's longest possible list (every pair's list is at most max_nq[1] long); a task row per
      // kSlabPointsPerTask points (the sub-trees of k_dc_block are larger: room to spare)
      constexpr int kSlabPointsPerTask = 16;
      const int pts = ((max_nq[1] + 63) / 64) * 64 + 64, tsk = 2 * pts / kSlabPointsPerTask + 16;
      if (!h->dc_bank[dc_b]->reserve(C, pts, tsk)) {
        fprintf(stderr, "visomatch: no memory for the GPU share of the Delaunay stage, staying on the host\n");
        dc_gpu = use_dc = false;
      }
    }
    if (use_dc) {
      chunks.emplace_back(new DcChunk());
      DcChunk *ch = chunks.back().get();
      ch->h = h;
      ch->ctx = cp;
      ch->p = p;
      ch->method = method;
      ch->full = dc_full;
      ch->chunk = k;
      ch->bank = dc_b;
      ch->n = n;
      ch->f0 = f0;
      ch->first_pair = first_pair;
      ch->work0 = ch->bank * C;
      ch->B = h->dc_bank[dc_b];
      ch->work = h->seq_work.data() + ch->work0;
      ch->stream = h->dc_stream[dc_b & 1];
      ch->valid = validp;
      sc[k].dc = ch;
    }
    cfg.sparse = 0;
    cfg.use_prior = p.multi_stage ? 1 : 0;
    vsm_launch_match(h->stream, h->prof, c.d_imgs, d_pairs, d_jobs, dummy, n, c.dims, cfg, max_nq[1]);
    if (p.refinement > 0)
      vsm_launch_refine(h->stream, h->prof, c.d_imgs, d_pairs, d_jobs, dummy, n, c.dims, c.dims, method, p.refinement,
                        max_nq[1]);
    vsm_launch_export(h->stream, h->prof, d_pairs, n, 1, max_nq[1]);
    sc[k].t_pass2 = now_us();
    HIPCHK(hipEventRecord(h->idle_wait, h->stream));
    if (k + 2 < nchunks) HIPCHK(launch_features_of(k + 2));
    tg += now_us() - ta;
  }
  if (nchunks > 0) {
    const int rc = finalize(nchunks - 1);
    if (rc != VSM_OK) return rc;
  }
  {
    const double tb = now_us();
    for (auto &ch : chunks) dc_wait(ch.get());
    if (vsm_debug_timing())
      for (auto &ch : chunks)
        fprintf(stderr, "  final stage of %d pairs: A %.0f..%.0f us (tasks %.0f us), G ..%.0f, B %.0f..%.0f (tasks %.0f us)\n", ch->n,
                ch->t_a0 - tstart, ch->t_g0 - tstart, ch->a_ns.load() * 1e-3, ch->t_g1 - tstart, ch->t_b0 - tstart, ch->t_b1 - tstart,
                ch->b_ns.load() * 1e-3);
    if (vsm_debug_timing() && !chunks.empty()) {
      double part[8] = {0};
      for (auto &ch : chunks)
        for (int q = 0; q < 8; q++) part[q] += ch->part_ns[q].load() * 1e-3 / n_frames;
      fprintf(stderr, "  per pair, us: pass-1 outliers %.0f prior statistics %.0f | A copy %.0f arrays %.0f prepare %.0f | B records %.0f merges %.0f support+survivors %.0f; pairs with duplicate points: %.0f\n",
              mid_ns[0].load() * 1e-3 / n_frames, mid_ns[1].load() * 1e-3 / n_frames, part[0], part[1], part[2], part[4], part[5], part[6], part[7] * n_frames * 1e3);
    }
    for (auto &t : tickets)
      if (t) h->pool->wait(t);
    thost += now_us() - tb;
    if (h->prof.on) {
      HIPCHK(hipStreamSynchronize(h->stream));
      for (hipStream_t st : h->dc_stream)
        if (st) HIPCHK(hipStreamSynchronize(st));
      h->prof.resolve();
    }
  }
  h->seq_timings[0] = tg;
  h->seq_timings[1] = thost;
  h->seq_timings[2] = now_us() - tstart;
  h->seq_timings[3] = (double)C;
  if (vsm_debug_timing())
    fprintf(stderr, "seq: entry->start %.0f us, gpu %.0f, host %.0f, total %.0f\n", tstart - t_entry, tg, thost,
            h->seq_timings[2]);
  // (a Delaunay stream that failed: the lists are complete - the host finished those chunks - but the caller must know)
  return h->seq_hip_error.load() ? VSM_EHIP : VSM_OK;
}

static void seq1_destroy(vsm_handle *h) {
  for (int b = 0; b < vsm_handle::kDcBanks; b++)
    if (h->dc_bank[b]) {
      h->dc_bank[b]->release();
      delete h->dc_bank[b];
      h->dc_bank[b] = nullptr;
    }
}
