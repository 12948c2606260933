// Arbitrary frame pairs of an image set in one batched call (included by vsm_api.cpp; DESIGN.md section 5).
//
// vsm_sequence_run and vsm_multi_process pair every frame with the one just before it.  A structure-from-motion driver
// wants other pairs of the same frames: the keyframe kept by pushBack(replace = true) against later frames, (a, b) and
// (b, a), loop-closure candidates, the frames of several short clips.  vsm_pairs_run takes the frames and a list of
// (previous, current) pairs: every frame goes through the image side ONCE, whatever number of pairs names it, and stays
// in HBM; the pairs then go, C at a time, through the step a vsm_multi_process call runs for its K sequences (vsm_step_run,
// vsm_step.inc) - first pass, its outlier removal and prior boxes, second pass, refinement, the final exact-Delaunay chain -
// from a job table that names the images by slot (pair_jobs, vsm_jobs.h).  No kernel is this form's own.  Per pair the list is, byte for byte,
// getMatches() of a fresh Matcher after pushBack(a), pushBack(b), matchFeatures(method, Tr of the pair).
struct VsmPairs {
  VsmCtx ctx;  // every image of the set (frame f: slots sides * f, + 1) and one bank of C pairs
  int chunk = 0;
  VsmStep st;  // a chunk's banks, events and survivors (vsm_step.inc): one arena slot per pair of the bank
  std::vector<std::vector<vsm_p_match>> lists;  // per pair of the last call
  std::vector<int32_t> pair_list;  // ... its pairs, frame count and method, for vsm_pairs_tracks; done: it ran to its end
  int32_t n_frames = 0, method = -1;
  bool done = false;
  int32_t sides = 1;      // images per frame of the last call
  bool resident = false;  // ... and whether its frames' feature records stand in ctx (not after the whole-call fallback)
  double timings[4] = {0, 0, 0, 0};  // image side, first passes + chains, second passes + chains, total; us
};

static void pairs_destroy(vsm_handle *h) {
  VsmPairs *P = h->pairs;
  if (!P) return;
  P->st.release();
  ctx_destroy(P->ctx);
  delete P;
  h->pairs = nullptr;
}

// The lists of the last vsm_pairs_run that ran to its end, as the later stages take lists: a pointer and a count per pair,
// into the caller's vectors.  Null: there is no such run (the vectors are then left alone).
static const VsmPairs *pairs_last_lists(const vsm_handle *h, std::vector<const vsm_p_match *> &lists, std::vector<int32_t> &counts) {
  const VsmPairs *P = h->pairs;
  if (!P || !P->done) return nullptr;
  lists.resize(P->lists.size());
  counts.resize(P->lists.size());
  for (size_t k = 0; k < P->lists.size(); k++) {
    lists[k] = P->lists[k].data();
    counts[k] = (int32_t)P->lists[k].size();
  }
  return P;
}

// The streaming ring of a handle, set aside while vsm_pairs_run's fallback matches pairs frame by frame on a ring of its
// own, and put back afterwards: images, counts, stage views and getMatches() of the caller's own pushes stay what they were.
struct PairsRingSave {
  vsm_handle *h = nullptr;
  VsmCtx ring;
  int cur = 0;
  bool have[2], right[2], f_valid = false, stage3_in_hm = false;
  int32_t n_feat[2][2][2], dims_p[3], dims_c[3];
  std::vector<vsm_p_match> stage[5], matched;
  std::vector<float> ranges;
  std::vector<uint8_t> gainI[2];
  int64_t counters[5];
  double timings[5];
  int take(vsm_handle *hh) {
    const int rc = settle(hh);  // (a push of the caller's that is still in flight)
    if (rc != VSM_OK) return rc;
    h = hh;
    std::swap(ring, h->ring);
    cur = h->cur;
    f_valid = h->f_valid;
    stage3_in_hm = h->stage3_in_hm;
    memcpy(have, h->have, sizeof(have));
    memcpy(right, h->right, sizeof(right));
    memcpy(n_feat, h->n_feat, sizeof(n_feat));
    memcpy(dims_p, h->dims_p, sizeof(dims_p));
    memcpy(dims_c, h->dims_c, sizeof(dims_c));
    memcpy(counters, h->counters, sizeof(counters));
    memcpy(timings, h->timings, sizeof(timings));
    for (int s = 0; s < 5; s++) stage[s].swap(h->stage[s]);
    matched.swap(h->matched);
    ranges.swap(h->ranges);
    for (int k = 0; k < 2; k++) gainI[k].swap(h->gainI[k]);
    h->stage3_in_hm = false;
    reset_ring_state(h);
    return VSM_OK;
  }
  ~PairsRingSave() {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    (void)hipGetLastError();
    ctx_destroy(h->ring);
    reset_ring_state(h);
    std::swap(ring, h->ring);
    h->cur = cur;
    h->f_valid = f_valid;
    h->stage3_in_hm = stage3_in_hm;
    memcpy(h->have, have, sizeof(have));
    memcpy(h->right, right, sizeof(right));
    memcpy(h->n_feat, n_feat, sizeof(n_feat));
    memcpy(h->dims_p, dims_p, sizeof(dims_p));
    memcpy(h->dims_c, dims_c, sizeof(dims_c));
    memcpy(h->counters, counters, sizeof(counters));
    memcpy(h->timings, timings, sizeof(timings));
    for (int s = 0; s < 5; s++) stage[s].swap(h->stage[s]);
    matched.swap(h->matched);
    ranges.swap(h->ranges);
    for (int k = 0; k < 2; k++) gainI[k].swap(h->gainI[k]);
  }
};

// Pairs k0 .. k0 + n - 1 the way the per-frame API does them: pushBack(a), pushBack(b), matchFeatures on a fresh ring (what
// the device chain cannot take: more than 1024 statistics bins, a list beyond its limits, a list it declined).
static int pairs_fallback(vsm_handle *h, VsmPairs &P, PairsRingSave &save, const uint8_t *left, const uint8_t *right, int64_t frame_stride,
                          int on_device, int32_t w, int32_t hh, int32_t bpl, int32_t method, const int32_t *pairs, int32_t k0, int32_t n,
                          const double *Tr, const uint8_t *Tr_valid) {
  if (!save.h) {
    const int rc = save.take(h);
    if (rc != VSM_OK) return rc;
  }
  for (int32_t k = k0; k < k0 + n; k++) {
    (void)hipStreamSynchronize(h->stream);
    reset_ring_state(h);
    h->matched.clear();
    const int32_t fr[2] = {method == 1 ? -1 : pairs[2 * k], pairs[2 * k + 1]};  // (stereo matching reads the current frame only)
    for (int q = 0; q < 2; q++) {
      if (fr[q] < 0) continue;
      const uint8_t *l = left + (size_t)fr[q] * frame_stride, *r = right ? right + (size_t)fr[q] * frame_stride : nullptr;
      const int rc = push_common(h, l, r, w, hh, bpl, 0, on_device != 0);
      if (rc != VSM_OK) return rc;
    }
    const double *t = (Tr && (!Tr_valid || Tr_valid[k])) ? Tr + (size_t)k * 12 : nullptr;
    const int rc = vsm_match(h, method, t);
    if (rc != VSM_OK && rc != VSM_ENOTREADY) return rc;
    P.lists[k] = h->matched;  // (ENOTREADY: matchFeatures returns early, the fresh matcher's list is empty)
  }
  return VSM_OK;
}

extern "C" {

int vsm_pairs_run(vsm_handle *h, const uint8_t *left, const uint8_t *right, int64_t frame_stride, int on_device, int32_t n_frames, int32_t w,
                  int32_t hh, int32_t bpl, int32_t method, const int32_t *pairs, int32_t n_pairs, const double *Tr, const uint8_t *Tr_valid) {
  if (!h || w <= 0 || hh <= 0 || bpl < w || left == nullptr || n_frames <= 0) {
    fprintf(stderr, "ERROR: Image dimension mismatch!\n");
    return VSM_EDIMS;
  }
  if (!pair_list_ok(method, n_frames, pairs, n_pairs)) return VSM_EARG;  // (nothing enqueued, the last call's lists stay)
  HIPCHK(hipSetDevice(h->device));
  const vsm_params &p = h->param;
  if (!h->pairs) h->pairs = new VsmPairs();
  VsmPairs &P = *h->pairs;
  const double t0 = now_us();
  P.lists.resize((size_t)n_pairs);  // (keeps the capacity of earlier calls)
  for (auto &v : P.lists) v.clear();
  P.pair_list.assign(pairs, pairs + 2 * (size_t)n_pairs);
  P.n_frames = n_frames;
  P.method = method;
  P.done = false;
  P.resident = false;
  memset(P.timings, 0, sizeof(P.timings));
  const int sides = right ? 2 : 1;
  P.sides = sides;
  PairsRingSave save;  // (armed by the first fallback; puts the caller's ring back however the call is left)
  // the statistics bins of k_dc2_prior live in LDS: a binning beyond 1024 bins goes pair by pair
  if (vsm_match_bins(p, w, hh) > 1024) {
    const int rc = pairs_fallback(h, P, save, left, right, frame_stride, on_device, w, hh, bpl, method, pairs, 0, n_pairs, Tr, Tr_valid);
    P.timings[3] = now_us() - t0;
    P.done = rc == VSM_OK;
    return rc;
  }
  const int C = seq2_plan(n_pairs, h->pool->size(), false, h->sw.pairs_chunk, 0, nullptr).C;
  const int slots = (sides * n_frames + 1) / 2;  // (a context holds two images per frame slot)
  VsmCtx &c = P.ctx;
  if (!c.holds(w, hh, slots, C) || c.has_heads != (h->sw.match_heads != 0)) {
    (void)hipStreamSynchronize(h->stream);
    const int rc = ctx_create(c, p, w, hh, slots, C, h->stream, h->sw.match_heads != 0);
    if (rc != VSM_OK) return rc;
    P.chunk = C;
    if (!P.st.arena.alloc(c.list_slot_bytes(), (size_t)C)) {
      c.ready = false;  // (the next call sets the context up again instead of running with half of it)
      return VSM_EHIP;
    }
  }
  if (!P.st.create_events()) return VSM_EHIP;
  // a call that fails after something was enqueued: drain the device, report
  auto fail = [&](int rc) { return P.st.fail(h->stream, rc); };
  // ---- pushBack of every frame, once: chunks of frames through the front end and the feature kernels ----
  {
    const int Cf = std::min<int>(n_frames, 64);
    const int seq_chunk_before = h->seq_chunk;  // (seq_ingest_host_frames sizes its pinned slots by it; they only grow)
    h->seq_chunk = std::max(seq_chunk_before, Cf);
    int rc = VSM_OK;
    for (int32_t f0 = 0; f0 < n_frames && rc == VSM_OK; f0 += Cf) {
      const int n = std::min<int>(Cf, n_frames - f0);
      if (on_device)
        enqueue_front_frames(h, c, sides * f0, sides, left + (size_t)f0 * frame_stride, (size_t)frame_stride,
                             right ? right + (size_t)f0 * frame_stride : nullptr, (size_t)frame_stride, bpl, n);
      else
        rc = seq_ingest_host_frames(h, c, sides * f0, left, right, frame_stride, bpl, w, hh, f0, n);
      if (rc == VSM_OK) enqueue_features(h, c, sides * f0, sides * n);
    }
    h->seq_chunk = seq_chunk_before;
    if (rc != VSM_OK) return fail(rc);
  }
  VSM_CHK(hipEventRecord(P.st.ev_feat, h->stream));
  VSM_CHK(hipEventSynchronize(P.st.ev_feat));  // every image's feature counts are in host-mapped memory
  VSM_CHK(hipGetLastError());
  P.resident = true;
  P.timings[0] = now_us() - t0;
  // ---- the pairs, C at a time: the step a vsm_multi_process call runs for its K sequences (vsm_step.inc) ----
  std::vector<char> valid((size_t)C, 0);
  for (int32_t k0 = 0; k0 < n_pairs; k0 += C) {
    const int n = std::min<int>(C, n_pairs - k0);
    const double t1 = now_us();
    int max_nq[2];
    pair_jobs(p, method, sides, c.hm_counts, pairs + 2 * (size_t)k0, n, Tr ? Tr + (size_t)k0 * 12 : nullptr, Tr_valid ? Tr_valid + k0 : nullptr, c.h_jobs,
              valid.data(), max_nq);
    bool any = false;
    for (int i = 0; i < n; i++) any = any || valid[i];
    if (!any) continue;  // (matchFeatures returns early on every pair of the chunk: empty lists)
    // a chunk with a list beyond the device chain's limits, or with a list the chain declined, goes pair by pair
    bool chain = vsm_step_fits(p, max_nq);
    double t2 = t1;
    if (chain) {
      int declined = 0;
      const int rc = vsm_step_run(h, c, P.st, C, n, valid.data(), method, max_nq, w, hh, &t2, &declined);
      if (rc != VSM_OK) return rc;
      if (declined) {
        P.st.clear_flags();
        chain = false;
      }
    }
    if (chain) {
      // the survivors out of the chunk's arena into the pairs' own lists: host memory grows with the matches found
      h->pool->run(n, [&](int i) {
        if (!valid[i]) return;
        const vsm_p_match *src = (const vsm_p_match *)(P.st.arena.res + P.st.arena.slot * i);
        P.lists[(size_t)k0 + i].assign(src, src + std::max(P.st.arena.res_cnt[i], 0));
      });
    } else {
      const int rc = pairs_fallback(h, P, save, left, right, frame_stride, on_device, w, hh, bpl, method, pairs, k0, n, Tr, Tr_valid);
      if (rc != VSM_OK) return fail(rc);
    }
    const double t3 = now_us();
    P.timings[1] += t2 - t1;
    P.timings[2] += t3 - t2;
  }
  if (h->prof.on) h->prof.resolve();
  P.timings[3] = now_us() - t0;
  P.done = true;
  return VSM_OK;
}

int32_t vsm_pairs_num_matches(vsm_handle *h, int32_t pair) {
  if (!h || !h->pairs || pair < 0 || pair >= (int32_t)h->pairs->lists.size()) return 0;
  return (int32_t)h->pairs->lists[pair].size();
}
int32_t vsm_pairs_get_matches(vsm_handle *h, int32_t pair, vsm_p_match *out, int32_t cap) {
  if (!h || !h->pairs || pair < 0 || pair >= (int32_t)h->pairs->lists.size()) return 0;
  const std::vector<vsm_p_match> &v = h->pairs->lists[pair];
  const int32_t n = std::min<int32_t>((int32_t)v.size(), cap);
  if (n > 0) memcpy(out, v.data(), (size_t)n * sizeof(vsm_p_match));
  return n;
}
void vsm_pairs_get_timings(vsm_handle *h, double *out4) {
  if (h && h->pairs)
    memcpy(out4, h->pairs->timings, sizeof(h->pairs->timings));
  else
    memset(out4, 0, 4 * sizeof(double));
}

}  // extern "C"
