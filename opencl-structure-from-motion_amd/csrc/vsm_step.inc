// One chunk step on the handle's one stream (included by vsm_api.cpp in front of vsm_multi.inc and vsm_pairs.inc; DESIGN.md
// section 5): the K sequences of a vsm_multi_process step, or up to C pairs of a vsm_pairs_run call, from a job table the
// caller has filled - first pass, its outlier removal and prior boxes (on the host pool or by the device chain), second
// pass, refinement, the final exact-Delaunay chain with the pool's vertex sorts beside the mesh, survivors into a
// host-mapped arena.  What a list beyond the chain's limits or a list the chain declined means is the caller's business.
struct VsmStep {
  Dc2Bank bank1, bank2;  // the chains of the first-pass and of the second-pass lists
  VsmResArena arena;     // host-mapped survivors, one slot per job
  hipEvent_t ev_feat = nullptr, ev_a = nullptr, ev_keys = nullptr;  // the caller's feature counts; first-pass lists or keys; final keys
  bool create_events() {  // (those that are not there yet)
    for (hipEvent_t *e : {&ev_feat, &ev_a, &ev_keys})
      if (!*e && hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) return false;
    return true;
  }
  void release() {  // (the stream is idle)
    for (hipEvent_t *e : {&ev_feat, &ev_a, &ev_keys}) {
      if (*e) (void)hipEventDestroy(*e);
      *e = nullptr;
    }
    bank1.release();
    bank2.release();
    arena.free();
  }
  // the banks' host flag words: [0] a list the chain declined, [1] long_seen (not read here: dc2_enqueue_mesh's expect_long stays true)
  void clear_flags() {
    for (Dc2Bank *B : {&bank1, &bank2})
      if (B->h_error) B->h_error[0] = B->h_error[1] = 0;
  }
  // a call that fails after something was enqueued: drain the device, clear the sticky error and the flag words, report
  int fail(hipStream_t stream, int rc) {
    (void)hipStreamSynchronize(stream);
    (void)hipGetLastError();
    clear_flags();
    return rc;
  }
};

// every size limit of the device chain, asked before anything of the step is enqueued (max_nq: the longest first-pass and
// second-pass list the jobs can give; the first-pass lists are sorted on the pool here: only the triangulation's own
// limits apply to them - vsm_chain_fits, vsm_jobs.h)
static bool vsm_step_fits(const vsm_params &p, const int max_nq[2]) { return vsm_chain_fits(p, max_nq, VSM_DC_KD_MAX_POINTS); }

// Jobs 0 .. n - 1 of c.h_jobs (filled by the caller, uploaded here; valid[i]: job i has lists at all; their lists fit:
// vsm_step_fits) from the reservation of the banks, for `reserve` jobs, to the drained stream.  t_keys: when the final
// keys reached the host.  declined: the banks' flag word - a list the chain would not take; the survivors in S.arena mean
// nothing then, and the flag words are still set.  Returns VSM_OK or, the stream drained and the flag words cleared, an error.
static int vsm_step_run(vsm_handle *h, VsmCtx &c, VsmStep &S, int reserve, int n, const char *valid, int method, const int max_nq[2], int32_t w,
                        int32_t hh, double *t_keys, int *declined) {
  const vsm_params &p = h->param;
  auto fail = [&](int rc) { return S.fail(h->stream, rc); };
  if ((p.multi_stage && !S.bank1.reserve(reserve, std::max(max_nq[0], 64), true)) || !S.bank2.reserve(reserve, std::max(max_nq[1], 64), true)) return fail(VSM_EHIP);
  const VsmPair *d_pairs = c.d_pairs;
  VsmJob *d_jobs = c.d_jobs;
  VSM_CHK(vsm_upload(h->stream, d_jobs, c.h_jobs, sizeof(VsmJob) * n));
  VsmMatchCfg cfg = make_cfg(p, method, h->sw.match_heads && c.has_heads);
  // option fused_keys: the chains' job tables go up in front of the matching launches and the compactions write the chains'
  // keys - into the pair bank and, the single stream having nothing beside it that a store across PCIe could hold up, into
  // the host-mapped arrays the pool sorts from; no k_upload + k_dc2_keys between a compaction and its chain's sort kernel.
  // (refinement = 2 shortens the lists behind the compaction: keys by k_dc2_keys behind it, as before)
  const bool fused_keys = h->sw.fused_keys && p.refinement != 2;
  VsmJob dummy;
  memset(&dummy, 0, sizeof(dummy));
  // Few jobs: the first-pass lists (0.7 k matches) go to the host pool, a list per thread - the device chain is a row
  // of latencies whatever the number of lists (0.4 ms for 8: keys, sort, sub-trees, two merge levels, votes, boxes),
  // one thread triangulates such a list in 50-60 us.  (Option multi_host_pass1: -1 = up to as many jobs as pool threads.)
  const bool host_p1 = p.multi_stage && (h->sw.multi_host_pass1 >= 0 ? h->sw.multi_host_pass1 != 0 : n <= h->pool->size());
  if (host_p1) {
    // ---- pass 1; removeOutliers + computePriorStatistics on the pool (viso/matcher.cpp:222-226) ----
    cfg.sparse = 1;
    cfg.use_prior = 0;
    if (!vsm_launch_match(h->stream, h->prof, c.d_imgs, d_pairs, d_jobs, dummy, n, c.dims, cfg, max_nq[0], 1))
      vsm_launch_export(h->stream, h->prof, d_pairs, n, 0, max_nq[0]);
    VSM_CHK(hipEventRecord(S.ev_a, h->stream));
    VSM_CHK(hipEventSynchronize(S.ev_a));  // the lists are in host-mapped memory
    VSM_CHK(hipGetLastError());
    const int32_t dims_c[3] = {w, hh, c.dims.bpl};
    VSM_CHK(host_pass1_boxes(h, c, 0, n, valid, method, dims_c));
  } else if (p.multi_stage) {
    // ---- pass 1 and its chain: removeOutliers + computePriorStatistics on the device (viso/matcher.cpp:222-226) ----
    cfg.sparse = 1;
    cfg.use_prior = 0;
    Dc2Bank &B = S.bank1;
    for (int i = 0; i < n; i++)
      B.fill_job(i, c.h_pairs[i].list1, c.h_pairs[i].count, false, nullptr, nullptr, c.h_pairs[i].ranges, nullptr, false, fused_keys ? c.h_pairs[i].keys[0] : nullptr, c.hm_lcount + 2 * i);
    if (fused_keys) {  // the chain's job table first, the keys from the compaction - also into host-mapped memory (see above)
      VSM_CHK(vsm_upload(h->stream, B.d_jobs, B.h_jobs, sizeof(VsmDc2Job) * n));
      const VsmKeyOut ko = {B.dev_of(B.host_keys(0)), B.keys_pitch, B.cap};
      vsm_launch_match(h->stream, h->prof, c.d_imgs, d_pairs, d_jobs, dummy, n, c.dims, cfg, max_nq[0], 0, nullptr, &ko);
    } else {
      vsm_launch_match(h->stream, h->prof, c.d_imgs, d_pairs, d_jobs, dummy, n, c.dims, cfg, max_nq[0]);
      VSM_CHK(vsm_upload(h->stream, B.d_jobs, B.h_jobs, sizeof(VsmDc2Job) * n));
      vsm_dc2_launch_keys(h->stream, B.d_jobs, n, max_nq[0]);  // (also into host-mapped memory)
    }
    VSM_CHK(hipEventRecord(S.ev_a, h->stream));
    dc2_enqueue_mesh(h->stream, B, n, max_nq[0]);
    // Triangle's vertex sort of the short lists on the pool (a few microseconds each) while the device triangulates: the
    // device's own sort of such a list is one wave for 0.36 ms, longer than the triangulation beside it
    VSM_CHK(hipEventSynchronize(S.ev_a));
    h->pool->run(n, [&](int i) { B.sort_ties_of(i); });
    dc2_enqueue_votes(h->stream, B, n, max_nq[0], method, (float)p.outlier_flow_tolerance, (float)p.outlier_disp_tolerance);
    vsm_dc2_launch_prior(h->stream, B.d_jobs, n, method, p.match_binsize, p.match_radius, w, hh, c.dims.ub, c.dims.vb);
  }
  // ---- pass 2, refinement, final removeOutliers (viso/matcher.cpp:229-232) ----
  cfg.sparse = 0;
  cfg.use_prior = p.multi_stage ? 1 : 0;
  Dc2Bank &B = S.bank2;
  for (int i = 0; i < n; i++)
    B.fill_job(i, c.h_pairs[i].list2, c.h_pairs[i].count + 1, false, (vsm_p_match *)(S.arena.res_dev + S.arena.slot * i), S.arena.res_cnt_dev + i, nullptr, nullptr, false,
               fused_keys ? c.h_pairs[i].keys[1] : nullptr, c.hm_lcount + 2 * i + 1);
  if (fused_keys) {
    VSM_CHK(vsm_upload(h->stream, B.d_jobs, B.h_jobs, sizeof(VsmDc2Job) * n));
    const VsmKeyOut ko = {B.dev_of(B.host_keys(0)), B.keys_pitch, B.cap};
    vsm_launch_match(h->stream, h->prof, c.d_imgs, d_pairs, d_jobs, dummy, n, c.dims, cfg, max_nq[1], 0, nullptr, &ko);
  } else {
    vsm_launch_match(h->stream, h->prof, c.d_imgs, d_pairs, d_jobs, dummy, n, c.dims, cfg, max_nq[1]);
    VSM_CHK(vsm_upload(h->stream, B.d_jobs, B.h_jobs, sizeof(VsmDc2Job) * n));
  }
  if (p.refinement == 2) {  // sub-pixel fits drop matches: they come before the keys of what is left (section 6b of DESIGN.md)
    vsm_launch_refine(h->stream, h->prof, c.d_imgs, d_pairs, d_jobs, dummy, n, c.dims, c.dims, method, p.refinement, max_nq[1]);
    vsm_launch_parabolic_apply(h->stream, h->prof, d_pairs, n);
  }
  if (!fused_keys) vsm_dc2_launch_keys(h->stream, B.d_jobs, n, max_nq[1]);  // (also into host-mapped memory: the pool sorts them)
  VSM_CHK(hipEventRecord(S.ev_keys, h->stream));
  dc2_enqueue_mesh(h->stream, B, n, max_nq[1]);
  if (p.refinement == 1) vsm_launch_refine(h->stream, h->prof, c.d_imgs, d_pairs, d_jobs, dummy, n, c.dims, c.dims, method, p.refinement, max_nq[1]);
  VSM_CHK(hipGetLastError());
  VSM_CHK(hipEventSynchronize(S.ev_keys));
  *t_keys = now_us();
  // Triangle's vertex sort of every list on the pool while the device triangulates (which match stands for a shared pixel)
  h->pool->run(n, [&](int i) { B.sort_ties_of(i); });
  dc2_enqueue_votes(h->stream, B, n, max_nq[1], method, (float)p.outlier_flow_tolerance, (float)p.outlier_disp_tolerance);
  VSM_CHK(hipGetLastError());
  VSM_CHK(hipStreamSynchronize(h->stream));
  *declined = S.bank2.h_error ? S.bank2.h_error[0] : 0;
  if (S.bank1.h_error) *declined |= S.bank1.h_error[0];
  return VSM_OK;
}
