// Re-observation of the points by projection (included by vsm_api.cpp; DESIGN.md section 5, INTEGRATION.md).
//
// The stage that adds observations: every point in use is projected into every searched frame with a pose that does not
// observe it yet, and the frame's free features near the projection are searched for the track's descriptor (vsm_reobserve.h
// has the definition, vsm_reobserve.hip the kernels).  The host's part: the frames' states, one pinned block with them, the
// masks, the tracks (8 bytes per observation, 33 per track), the features' offsets and a pointer per frame to its records -
// into the uploaded block for the general form, which carries the records (48 bytes per feature), into the last
// vsm_pairs_run's context for vsm_points_reobserve, which uploads none.  One copy up, the kernels up to the candidates'
// number, the call's one wait in the middle - the number sizes the candidates' block, 44 bytes each, which only then is
// made -, the list, the search and the verdicts, one copy back.  Blocks: RoBlocks, RoCandBlocks (vsm_layouts.h); the call
// waits twice, as the tracks call does, so it keeps its own sequence of copies and launches and takes the drain, the keep
// and the timings' close of vsm_stage.h.
struct VsmReobserve : VsmResult<RO_STATS> {  // the staging and the last result's stats and timings (vsm_stage.h)
  VsmStage cs;                               // the candidates' device block and pinned copy
  std::vector<int32_t> cand, track_accepted, frame_counts;
  std::vector<double> cand_uv;
  int32_t n_accepted = 0;
};

static void reobserve_destroy(vsm_handle *h) {
  if (h->reobserve) h->reobserve->cs.release();
  vsm_result_destroy(h->reobserve);
}

// what a form gives the run beside the shared arguments: where the tracks' arrays and the features are
struct RoSource {
  const int32_t *obs;         // the handle form: rows {frame, feature, ., .} of the track result; else null
  const int32_t *obs_frames, *obs_feat;
  const int32_t *feat;        // the general form's records; null: resident, frame g's at resident[g]
  const int32_t *const *resident;
};

// The arguments have been checked.  use_of(t) is track t's use byte, feat_offsets[F + 1] the features' offsets.
template <class UseOf>
static int reobserve_run(vsm_handle *h, double t0, int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *search, double f, double cu,
                         double cv, int32_t width, int32_t height, int32_t n_tracks, int64_t n_obs, const int32_t *offsets, const double *xyz, const int32_t *ref_obs,
                         const int32_t *feat_offsets, const RoSource &src, const vsm_reobserve_params &prm, UseOf use_of) {
  HIPCHK(hipSetDevice(h->device));
  if (!h->reobserve) h->reobserve = new VsmReobserve();
  VsmReobserve &V = *h->reobserve;
  VsmStage &S = V.st;
  const size_t F = (size_t)n_frames, T = (size_t)n_tracks, N = (size_t)n_obs, NF = F > 0 ? (size_t)feat_offsets[n_frames] : 0;
  const RoGrid grid = ro_grid(width, height);
  const size_t B = (size_t)ro_frame_bins(grid);
  if (F * B > 0x7fffffff || NF > 0x7fffffff) return VSM_EHIP;  // (an index the device cannot hold)
  const RoBlocks L(F, T, N, NF, src.feat ? NF : 0, B);
  HIPCHK(S.grow_in(L.in.at, h->stream));
  HIPCHK(S.grow_out(L.out.at, h->stream));
  // ---- pack ----
  for (size_t g = 0; g < F; g++) pts_rigid_inverse(poses + 12 * g, L.states.host(S) + 12 * g);
  vsm_mask_bytes(pose_valid, F, L.valid.host(S));
  vsm_mask_bytes(search, F, L.search.host(S));
  memcpy(L.offsets.host(S), offsets, (T + 1) * 4);
  if (T > 0) memcpy(L.xyz.host(S), xyz, T * 24);
  int64_t tracks_in_use = 0;
  for (size_t t = 0; t < T; t++) {
    const int32_t n = offsets[t + 1] - offsets[t];
    const bool in_use = use_of((int32_t)t) && n > 0;
    L.use.host(S)[t] = in_use ? 1 : 0;
    L.ref_obs.host(S)[t] = n > 0 ? (ref_obs ? ref_obs[t] : ro_middle(n)) : 0;
    tracks_in_use += in_use ? 1 : 0;
  }
  if (src.obs) {
    int32_t *fr = L.obs_frames.host(S), *ft = L.obs_feat.host(S);
    for (size_t i = 0; i < N; i++) fr[i] = src.obs[4 * i], ft[i] = src.obs[4 * i + 1];
  } else if (N > 0) {
    memcpy(L.obs_frames.host(S), src.obs_frames, N * 4);
    memcpy(L.obs_feat.host(S), src.obs_feat, N * 4);
  }
  if (F > 0) memcpy(L.feat_offsets.host(S), feat_offsets, (F + 1) * 4);
  else L.feat_offsets.host(S)[0] = 0;
  if (src.feat && NF > 0) memcpy(L.feat.host(S), src.feat, NF * RO_FEAT_INTS * 4);
  {
    int64_t frames = 0;
    for (size_t g = 0; g < F; g++) frames += (L.valid.host(S)[g] && L.search.host(S)[g]) ? 1 : 0;
    if (frames * tracks_in_use > 0x7fffffff) return VSM_EARG;  // (more candidates than an index counts: search fewer frames)
  }
  // ---- from here on the call replaces the last result ----
  HIPCHK(V.replace(L, h->stream, t0));
  HIPCHK(V.cs.events());
  for (size_t g = 0; g < F; g++) L.frame_feat.host(S)[g] = src.feat ? L.feat.dev(S) + RO_FEAT_INTS * (size_t)feat_offsets[g] : src.resident[g];
  V.n_accepted = 0;
  RoDevice d;
  memset(&d, 0, sizeof(d));
  d.states = L.states.dev(S);
  d.valid = L.valid.dev(S);
  d.search = L.search.dev(S);
  d.offsets = L.offsets.dev(S);
  d.obs_frames = L.obs_frames.dev(S);
  d.obs_feat = L.obs_feat.dev(S);
  d.xyz = L.xyz.dev(S);
  d.use = L.use.dev(S);
  d.ref_obs = L.ref_obs.dev(S);
  d.feat_offsets = L.feat_offsets.dev(S);
  d.frame_feat = L.frame_feat.dev(S);
  d.occupied = L.occupied.dev(S, L.out_at);
  d.claim = L.claim.dev(S, L.out_at);
  d.bins = L.bins.dev(S, L.out_at);
  d.bins_part = L.bins_part.dev(S, L.out_at);
  d.bins_total = L.bins_total.dev(S, L.out_at);
  d.sorted = L.sorted.dev(S, L.out_at);
  d.scan = L.scan.dev(S, L.out_at);
  d.scan_part = L.scan_part.dev(S, L.out_at);
  d.totals = L.totals.dev(S, L.out_at);
  d.track_accepted = L.track_accepted.dev(S, L.out_at);
  d.frame_counts = L.frame_counts.dev(S, L.out_at);
  d.stats = L.stats.dev(S, L.out_at);
  d.f = f;
  d.cu = cu;
  d.cv = cv;
  d.prm = prm;
  d.grid = grid;
  d.n_frames = n_frames;
  d.n_tracks = n_tracks;
  d.n_obs = (int32_t)n_obs;
  d.n_feat = (int32_t)NF;
  d.width = width;
  d.height = height;
  int32_t n_cand = 0;
  RoCandBlocks C(0);
  memset(S.pin_out, 0, L.out.at);  // (what a call without a launch returns: no candidates)
  if (n_tracks > 0 && n_frames > 0) {
    const VsmDrain fail{h->stream};  // a call that fails after something was enqueued: drain the device, report
    VSM_CHK(hipEventRecord(S.ev[0], h->stream));
    VSM_CHK(hipMemcpyAsync(S.dev, S.pin_in, L.in.at, hipMemcpyHostToDevice, h->stream));
    // the counts the kernels add to, the occupied bytes and the bins start at zero; a feature nobody claims holds RO_NO_KEY
    VSM_CHK(hipMemsetAsync(S.dev + L.out_at, 0, L.out.at, h->stream));
    VSM_CHK(hipMemsetAsync(d.occupied, 0, L.zero_bytes, h->stream));
    if (NF > 0) VSM_CHK(hipMemsetAsync(d.claim, 0xff, NF * 8, h->stream));
    VSM_CHK(hipEventRecord(S.ev[1], h->stream));
    vsm_reobserve_launch_count(h->stream, h->prof, d);
    VSM_CHK(hipGetLastError());
    // the candidates' number sizes their block: the one place where the host waits in the middle of the call
    VSM_CHK(hipMemcpyAsync(L.totals.host(S), d.totals, 8, hipMemcpyDeviceToHost, h->stream));
    VSM_CHK(hipStreamSynchronize(h->stream));
    n_cand = L.totals.host(S)[0];
    if (n_cand < 0) return fail(VSM_EHIP);  // (cannot be: the bound was checked)
    C = RoCandBlocks((size_t)n_cand);
    VSM_CHK(V.cs.grow_dev(C.dev_bytes, h->stream));
    VSM_CHK(V.cs.grow_out(C.out.at, h->stream));
    d.cand = C.cand.dev(V.cs, C.out_at);
    d.cand_uv = C.uv.dev(V.cs, C.out_at);
    vsm_reobserve_launch_search(h->stream, h->prof, d, n_cand);
    VSM_CHK(hipGetLastError());
    VSM_CHK(hipEventRecord(S.ev[2], h->stream));
    VSM_CHK(hipMemcpyAsync(S.pin_out, S.dev + L.out_at, L.out.at, hipMemcpyDeviceToHost, h->stream));
    if (n_cand > 0) VSM_CHK(hipMemcpyAsync(V.cs.pin_out, V.cs.dev + C.out_at, C.out.at, hipMemcpyDeviceToHost, h->stream));
    VSM_CHK(hipStreamSynchronize(h->stream));
    VSM_CHK(hipGetLastError());
    if (h->prof.on) h->prof.resolve();
    S.elapsed();
  }
  // ---- into the handle's vectors ----
  VsmKeep K(true);
  L.track_accepted.keep(K, S, V.track_accepted);
  L.frame_counts.keep(K, S, V.frame_counts);
  K.add(V.cand, n_cand > 0 ? C.cand.host(V.cs) : nullptr, (size_t)n_cand * RO_CAND_INTS);
  K.add(V.cand_uv, n_cand > 0 ? C.uv.host(V.cs) : nullptr, (size_t)n_cand * 2);
  K.run(h->pool);
  for (int q = 0; q < RO_STATS; q++) V.stats[q] = (int64_t)L.stats.host(S)[q];
  V.n_accepted = (int32_t)V.stats[RO_REASONS + RO_ACCEPTED];
  V.close();
  return VSM_OK;
}

static const VsmReobserve *reobserve_result(vsm_handle *h) { return (h && h->reobserve && h->reobserve->have) ? h->reobserve : nullptr; }

// frame g of the last vsm_pairs_run that left its features resident: the image, or -1
static int pairs_image(const vsm_handle *h, int32_t frame, int32_t side) {
  const VsmPairs *P = h ? h->pairs : nullptr;
  if (!P || !P->done || !P->resident || !P->ctx.ready || frame < 0 || frame >= P->n_frames || side < 0 || side >= P->sides) return -1;
  return P->sides * frame + side;
}

extern "C" {

int vsm_reobserve_run(vsm_handle *h, int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *search, double f, double cu, double cv,
                      int32_t width, int32_t height, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const int32_t *obs_feat, const double *xyz,
                      const uint8_t *use, const int32_t *ref_obs, const int32_t *feat_offsets, const int32_t *feat, const vsm_reobserve_params *params) {
  if (!h) return VSM_EARG;
  const double t0 = now_us();
  if (ro_check_features(n_frames, width, height, feat_offsets, feat) < 0) return VSM_EARG;
  const int64_t n_obs = ro_check_tracks(params, n_frames, poses, width, height, n_tracks, offsets, obs_frames, obs_feat, xyz, ref_obs, feat_offsets);
  if (n_obs < 0) return VSM_EARG;
  const int32_t zero = 0;
  const RoSource src{nullptr, obs_frames, obs_feat, feat ? feat : &zero, nullptr};
  return reobserve_run(h, t0, n_frames, poses, pose_valid, search, f, cu, cv, width, height, n_tracks, n_obs, n_tracks > 0 ? offsets : &zero, xyz, ref_obs,
                       feat_offsets, src, *params, [=](int32_t t) { return !use || use[t]; });
}

int vsm_points_reobserve(vsm_handle *h, const double *poses, const uint8_t *pose_valid, const uint8_t *search, double f, double cu, double cv,
                         const vsm_reobserve_params *params) {
  if (!h) return VSM_EARG;
  const double t0 = now_us();
  TracksInput in;
  const int rc = in.take(h, true, nullptr, nullptr);
  if (rc != VSM_OK) return rc;
  const VsmPairs *P = h->pairs;
  if (in.T->side != 0 || pairs_image(h, 0, 0) < 0 || P->n_frames != in.n_frames) return VSM_ENOTREADY;
  const int32_t width = P->ctx.dims.w, height = P->ctx.dims.h;
  if (!ro_params_ok(params) || !ro_dims_ok(width, height) || !poses) return VSM_EARG;
  // the features: set 1 of every frame's left image, where the pairs run left them
  std::vector<int32_t> feat_offsets((size_t)in.n_frames + 1, 0);
  std::vector<const int32_t *> resident((size_t)in.n_frames);
  for (int32_t g = 0; g < in.n_frames; g++) {
    const int img = P->sides * g;
    feat_offsets[g + 1] = feat_offsets[g] + std::min(std::max(P->ctx.hm_counts[img * 2 + 1], 0), P->ctx.cap_set[1]);
    resident[g] = P->ctx.h_imgs[img].set[1].feat;
  }
  const int32_t *obs = in.T->obs.data();
  for (int64_t i = 0; i < in.n_obs; i++) {  // (the tracks' features are those of the lists, which index set 1)
    const int32_t g = obs[4 * i], k = obs[4 * i + 1];
    if (k < 0 || k >= feat_offsets[g + 1] - feat_offsets[g]) return VSM_ENOTREADY;
  }
  const int32_t *status = in.P->status.data();
  const RoSource src{obs, nullptr, nullptr, nullptr, resident.data()};
  return reobserve_run(h, t0, in.n_frames, poses, pose_valid, search, f, cu, cv, width, height, in.n_tracks, in.n_obs, in.T->offsets.data(), in.P->xyz.data(),
                       nullptr, feat_offsets.data(), src, *params, [=](int32_t t) { return status[t] == 0; });
}

void vsm_reobserve_count(vsm_handle *h, int32_t *n_cand, int32_t *n_accepted) {
  const VsmReobserve *V = reobserve_result(h);
  if (n_cand) *n_cand = V ? (int32_t)(V->cand.size() / RO_CAND_INTS) : 0;
  if (n_accepted) *n_accepted = V ? V->n_accepted : 0;
}
int32_t vsm_reobserve_get(vsm_handle *h, int32_t *cand7, double *uv) {
  const VsmReobserve *V = reobserve_result(h);
  if (!V) return 0;
  vsm_copy_wanted(V->cand, cand7);
  vsm_copy_wanted(V->cand_uv, uv);
  return (int32_t)(V->cand.size() / RO_CAND_INTS);
}
int32_t vsm_reobserve_get_tracks(vsm_handle *h, int32_t *accepted) {
  const VsmReobserve *V = reobserve_result(h);
  if (!V) return 0;
  vsm_copy_wanted(V->track_accepted, accepted);
  return (int32_t)V->track_accepted.size();
}
int32_t vsm_reobserve_get_frames(vsm_handle *h, int32_t *counts2) {
  const VsmReobserve *V = reobserve_result(h);
  if (!V) return 0;
  vsm_copy_wanted(V->frame_counts, counts2);
  return (int32_t)(V->frame_counts.size() / 2);
}
void vsm_reobserve_get_stats(vsm_handle *h, int64_t *out10) { vsm_result_get(reobserve_result(h), &VsmReobserve::stats, out10); }
void vsm_reobserve_get_timings(vsm_handle *h, double *out4) { vsm_result_get(reobserve_result(h), &VsmReobserve::timings, out4); }

int32_t vsm_pairs_num_features(vsm_handle *h, int32_t frame, int32_t side, int32_t set) {
  const int img = pairs_image(h, frame, side);
  if (img < 0 || set < 0 || set > 1) return 0;
  return std::min(std::max(h->pairs->ctx.hm_counts[img * 2 + set], 0), h->pairs->ctx.cap_set[set]);
}
int32_t vsm_pairs_get_features(vsm_handle *h, int32_t frame, int32_t side, int32_t set, int32_t *out, int32_t cap) {
  int32_t n = vsm_pairs_num_features(h, frame, side, set);
  if (n > cap) n = cap;
  if (n <= 0 || !out) return 0;
  const VsmPairs *P = h->pairs;
  if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess ||
      hipMemcpy(out, P->ctx.h_imgs[P->sides * frame + side].set[set].feat, (size_t)n * RO_FEAT_INTS * 4, hipMemcpyDeviceToHost) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

}  // extern "C"
