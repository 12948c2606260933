// Lock-step multi-sequence stereo visual odometry (included by vsm_api.cpp; SURVEY.md section 8 row f-3, DESIGN.md).
//
// VisualOdometryStereo::process (viso/viso_stereo.cpp:33-40) is serial inside one sequence: frame t's matching takes the
// Tr_delta that frame t-1's egomotion produced.  K independent sequences (the eight of BASELINE's config 4, the cameras of
// a rig, the clips of a batch job) have no such tie between them: vsm_multi_process takes frame t of ALL of them through
// every kernel in one launch - features of 2 K images, both matching passes and the refinement of K pairs, the exact
// Delaunay chains of K lists (the device chain of the look-ahead path, vsm_dc.hip) - and then runs bucketing and
// egomotion of the K sequences side by side on the host pool, each with the rand() stream and the RANSAC sampler a
// process of its own would have.  Per sequence the result is bit for bit what K separate processes of the reference give.
struct vsm_multi {
  vsm_handle *h = nullptr;  // the matcher context: stream, pool, switches, the frame / pair buffers (h->seq)
  vsm_vo_stereo_params par;
  int K = 0;
  int64_t step = 0;
  int32_t w = 0, hh = 0;
  VsmStep st;  // the step's banks, events and survivors (vsm_step.inc): one arena slot per sequence
  struct Seq {
    VsmEgoSeq *ego = nullptr;
    double T[16];
    bool valid = false;
    std::vector<vsm_p_match> final_list, matched;  // getMatches() before / after bucketFeatures
    std::vector<int32_t> inliers;
    int ok = 0;
    int32_t nfeat[2][2] = {{0, 0}, {0, 0}};  // previous frame's feature counts [side][set]
    bool have_prev = false;
  };
  std::vector<Seq> seq;
  double timings[4] = {0, 0, 0, 0};  // last step, microseconds: features, first pass + chain, second pass + chain, bucketing + egomotion
};

static void multi_release(vsm_multi *m) {
  if (!m) return;
  if (m->h) {
    (void)hipSetDevice(m->h->device);
    (void)hipStreamSynchronize(m->h->stream);
  }
  m->st.release();
  for (auto &s : m->seq) vsm_ego_seq_destroy(s.ego);
  if (m->h) vsm_destroy(m->h);
  delete m;
}

extern "C" {

vsm_multi *vsm_multi_create(const vsm_vo_stereo_params *p, int32_t n_sequences) {
  if (!p || n_sequences < 1 || n_sequences > 4096) return nullptr;
  vsm_handle *h = vsm_create(&p->match);
  if (!h) return nullptr;
  vsm_multi *m = new vsm_multi();
  m->h = h;
  m->par = *p;
  m->K = n_sequences;
  vsm_set_intrinsics(h, p->f, p->cu, p->cv, p->base);  // viso/viso_stereo.cpp:28
  m->seq.resize((size_t)n_sequences);
  for (auto &s : m->seq) {
    s.ego = vsm_ego_seq_create(p);
    for (int i = 0; i < 16; i++) s.T[i] = (i % 5 == 0) ? 1.0 : 0.0;
  }
  if (!m->st.create_events()) {
    multi_release(m);
    return nullptr;
  }
  return m;
}

void vsm_multi_destroy(vsm_multi *m) { multi_release(m); }

// One lock-step: the next stereo pair of every sequence.  left / right: K images seq_stride bytes apart (sequence k at
// k * seq_stride), in host memory or (on_device != 0) in HBM.  ok_out (K flags, may be NULL): process()'s return value
// per sequence.  Returns VSM_OK or an error - then NO sequence has advanced: the frame's features went into the bank that
// the next call overwrites again, the previous frame's features, the feature counts, Tr_delta, the match lists and both
// random streams of every sequence are what they were before the call (everything that moves a sequence on is committed
// at the end, in one place), and nothing of the failed step is still running on the device.
int vsm_multi_process(vsm_multi *m, const uint8_t *left, const uint8_t *right, int64_t seq_stride, int on_device, int32_t w, int32_t hh,
                      int32_t bpl, int32_t *ok_out) {
  if (!m || w <= 0 || hh <= 0 || bpl < w || !left || !right) {
    fprintf(stderr, "ERROR: Image dimension mismatch!\n");
    return VSM_EDIMS;
  }
  vsm_handle *h = m->h;
  HIPCHK(hipSetDevice(h->device));
  const vsm_params &p = h->param;
  const int K = m->K, method = 2;
  VsmCtx &c = h->seq;
  if (!c.holds(w, hh, 2 * K, K)) {
    (void)hipStreamSynchronize(h->stream);
    const int rc = ctx_create(c, p, w, hh, 2 * K, K, h->stream, h->sw.match_heads != 0);
    if (rc != VSM_OK) return rc;
    h->seq_chunk = K;
    m->step = 0;
    for (auto &s : m->seq) s.have_prev = false;
    if (!m->st.arena.alloc(c.list_slot_bytes(), (size_t)K)) {
      c.ready = false;  // (the next call sets the context up again instead of running with half of it)
      return VSM_EHIP;
    }
    m->w = w;
    m->hh = hh;
  }
  if ((size_t)c.dims.ub * c.dims.vb > 1024) return VSM_EARG;  // (k_dc2_prior keeps the bins' minima and maxima in LDS)
  // a step that fails after something was enqueued: drain the device, report, commit nothing
  auto fail = [&](int rc) { return m->st.fail(h->stream, rc); };
  const double t0 = now_us();
  const int bank = (int)(m->step & 1), first_img = 2 * bank * K, prev_img = 2 * (bank ^ 1) * K;
  // ---- pushBack of K frames: one launch per kernel over 2 K images ----
  if (on_device) {
    enqueue_front_frames(h, c, first_img, 2, left, (size_t)seq_stride, right, (size_t)seq_stride, bpl, K);
  } else {
    const int rc = seq_ingest_host_frames(h, c, first_img, left, right, seq_stride, bpl, w, hh, 0, K);
    if (rc != VSM_OK) return fail(rc);
  }
  enqueue_features(h, c, first_img, 2 * K);
  VSM_CHK(hipEventRecord(m->st.ev_feat, h->stream));
  VSM_CHK(hipEventSynchronize(m->st.ev_feat));  // the feature counts are in host-mapped memory
  VSM_CHK(hipGetLastError());
  const double t1 = now_us();
  // ---- one job per sequence ----
  VsmJob *h_jobs = c.h_jobs;
  std::vector<char> valid((size_t)K, 0);
  std::vector<int32_t> nfeat_new((size_t)K * 4, 0);
  int max_nq[2] = {0, 0};
  for (int i = 0; i < K; i++) {
    vsm_multi::Seq &s = m->seq[i];
    const int img_c = first_img + 2 * i, img_p = prev_img + 2 * i;
    int32_t cnt[4][2];
    for (int q = 0; q < 2; q++) {
      cnt[0][q] = s.have_prev ? s.nfeat[0][q] : 0;
      cnt[1][q] = s.have_prev ? s.nfeat[1][q] : 0;
      cnt[2][q] = c.hm_counts[img_c * 2 + q];
      cnt[3][q] = c.hm_counts[(img_c + 1) * 2 + q];
    }
    if (s.have_prev)  // matchFeatures(2, Tr_valid ? &Tr_delta : 0), viso/viso_stereo.cpp:35
      valid[i] = vsm_job_fill(p, method, cnt, img_p, img_c, s.valid ? s.T : nullptr, h_jobs[i], max_nq) ? 1 : 0;
    else  // (a sequence's first frame: nothing to match it with)
      vsm_job_slots(h_jobs[i], img_p, img_c);
    for (int q = 0; q < 2; q++) {  // (this frame is the next step's previous one - once the step has succeeded)
      nfeat_new[(size_t)i * 4 + q] = cnt[2][q];
      nfeat_new[(size_t)i * 4 + 2 + q] = cnt[3][q];
    }
  }
  double t2 = t1, t3 = t1;
  bool any = false;
  for (int i = 0; i < K; i++) any = any || valid[i];
  if (any) {
    if (!vsm_step_fits(p, max_nq)) {
      fprintf(stderr, "visomatch: vsm_multi_process: a match list of %d / %d entries is beyond the device chain\n", max_nq[0], max_nq[1]);
      return fail(VSM_EARG);
    }
    int declined = 0;
    const int rc = vsm_step_run(h, c, m->st, K, K, valid.data(), method, max_nq, w, hh, &t2, &declined);
    if (rc != VSM_OK) return rc;
    if (declined) {
      fprintf(stderr, "visomatch: vsm_multi_process: the device chain declined a list (code %d)\n", declined);
      return fail(VSM_EARG);
    }
    t3 = now_us();
  }
  // ---- bucketFeatures + updateMotion of every sequence, side by side (viso/viso_stereo.cpp:37-39) ----
  // (option multi_shared_ego = 1: idle pool threads take hypotheses of the sequences' RANSAC loops as nested batches - measured
  // at K = 8 on 15 threads: no difference, 4.46-4.61 against 4.65-4.67 k frames/s; off)
  const bool shared_ego = h->sw.multi_shared_ego > 0;
  h->pool->run(K, [&](int i) {
    vsm_multi::Seq &s = m->seq[i];
    for (int q = 0; q < 2; q++) {  // the step is through: this frame becomes the previous one
      s.nfeat[0][q] = nfeat_new[(size_t)i * 4 + q];
      s.nfeat[1][q] = nfeat_new[(size_t)i * 4 + 2 + q];
    }
    s.have_prev = true;
    if (valid[i]) {
      const int32_t n = m->st.arena.res_cnt[i];
      const vsm_p_match *src = (const vsm_p_match *)(m->st.arena.res + m->st.arena.slot * i);
      s.final_list.assign(src, src + std::max(n, 0));
      s.matched = s.final_list;
    } else {
      // matchFeatures returned early (viso/matcher.cpp:190-216): p_matched_2 still holds what the previous step's
      // bucketFeatures left in it (viso/matcher.cpp:266-280 rewrites the list in place), and process() buckets THAT list
      // again - consuming rand() - and hands it to updateMotion (viso/viso_stereo.cpp:36-39)
      s.final_list = s.matched;
    }
    s.ok = vsm_ego_seq_step(s.ego, s.matched, s.T, &s.valid, s.inliers, shared_ego ? h->pool : nullptr);
  });
  if (ok_out)
    for (int i = 0; i < K; i++) ok_out[i] = m->seq[i].ok;
  m->step++;
  const double t4 = now_us();
  m->timings[0] = t1 - t0;
  m->timings[1] = t2 - t1;
  m->timings[2] = t3 - t2;
  m->timings[3] = t4 - t3;
  return VSM_OK;
}

int32_t vsm_multi_num_sequences(vsm_multi *m) { return m ? m->K : 0; }
void vsm_multi_get_motion(vsm_multi *m, int32_t k, double *T16) {
  if (m && k >= 0 && k < m->K) memcpy(T16, m->seq[k].T, sizeof(m->seq[k].T));
}
int vsm_multi_motion_valid(vsm_multi *m, int32_t k) { return (m && k >= 0 && k < m->K && m->seq[k].valid) ? 1 : 0; }
// bucketed = 0: getMatches() as matchFeatures left it; 1: after bucketFeatures (what the egomotion saw)
int32_t vsm_multi_num_matches(vsm_multi *m, int32_t k, int bucketed) {
  if (!m || k < 0 || k >= m->K) return 0;
  return (int32_t)(bucketed ? m->seq[k].matched.size() : m->seq[k].final_list.size());
}
int32_t vsm_multi_get_matches(vsm_multi *m, int32_t k, int bucketed, vsm_p_match *out, int32_t cap) {
  if (!m || k < 0 || k >= m->K) return 0;
  const std::vector<vsm_p_match> &v = bucketed ? m->seq[k].matched : m->seq[k].final_list;
  const int32_t n = std::min<int32_t>((int32_t)v.size(), cap);
  if (n > 0) memcpy(out, v.data(), (size_t)n * sizeof(vsm_p_match));
  return n;
}
int32_t vsm_multi_num_inliers(vsm_multi *m, int32_t k) { return (m && k >= 0 && k < m->K) ? (int32_t)m->seq[k].inliers.size() : 0; }
int32_t vsm_multi_get_inliers(vsm_multi *m, int32_t k, int32_t *out, int32_t cap) {
  if (!m || k < 0 || k >= m->K) return 0;
  const int32_t n = std::min<int32_t>((int32_t)m->seq[k].inliers.size(), cap);
  if (n > 0) memcpy(out, m->seq[k].inliers.data(), (size_t)n * sizeof(int32_t));
  return n;
}
void vsm_multi_get_timings(vsm_multi *m, double *out4) {
  if (m) memcpy(out4, m->timings, sizeof(m->timings));
}

}  // extern "C"
