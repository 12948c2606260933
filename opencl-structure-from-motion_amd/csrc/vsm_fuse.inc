// Fusion of duplicate tracks (included by vsm_api.cpp behind vsm_reobserve.inc; DESIGN.md section 5, INTEGRATION.md).
//
// The stage that joins tracks: every point in use is projected into every searched frame with a pose that does not observe
// it yet, and the features that tracks in use own near the projection are searched for the track's descriptor; two tracks
// that choose each other are fused (vsm_fuse.h has the definition, vsm_fuse.hip the kernels).  The host's part is the
// re-observation's: the frames' states, one pinned block with them, the masks, the tracks, the features' offsets and a pointer
// per frame to its records - uploaded for the general form, resident in the last vsm_pairs_run's context for vsm_points_fuse.
// The call waits twice.  The first wait, in the middle, is for the number of proposals: it sizes their block, 48 bytes each,
// which only then is made - the candidates, thirty times as many on the street scene, are never listed and never copied.
// The search runs once where its proposals' places fit the device block (FU_PLACES_MAX; FuSlotBlocks) - the counting pass
// keeps each track's proposals in the track's places and k_fu_compact moves them into the list behind the scan - and twice,
// counting and then listing, where they do not (option fuse_compact: 1 / 0 force either; profiles/README.md has both times).  The second is the call's end,
// behind the one copy back: the tracks' partners, the merged set, the counts, and the proposals.  Blocks: FuBlocks,
// FuPropBlocks (vsm_layouts.h); the sequence of copies and launches is the re-observation's, with the drain, the keep and the
// timings' close of vsm_stage.h.
struct VsmFuse : VsmResult<FU_STATS> {  // the staging and the last result's stats and timings (vsm_stage.h)
  VsmStage ps;                         // the proposals' device block and pinned copy
  VsmStage ss;                         // the compacting form's places (device only)
  std::vector<int32_t> prop, partner, fused_into, offsets_after, obs_src, frame_counts;
  std::vector<double> prop_uv;
};

static void fuse_destroy(vsm_handle *h) {
  if (h->fuse) h->fuse->ps.release(), h->fuse->ss.release();
  vsm_result_destroy(h->fuse);
}

// The arguments have been checked.  use_of(t) is track t's use byte, feat_offsets[F + 1] the features' offsets; src as for
// the re-observation (RoSource).
template <class UseOf>
static int fuse_run(vsm_handle *h, double t0, int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *search, double f, double cu, double cv,
                    int32_t width, int32_t height, int32_t n_tracks, int64_t n_obs, const int32_t *offsets, const double *xyz, const int32_t *ref_obs,
                    const int32_t *feat_offsets, const RoSource &src, const vsm_fuse_params &prm, UseOf use_of) {
  HIPCHK(hipSetDevice(h->device));
  if (!h->fuse) h->fuse = new VsmFuse();
  VsmFuse &V = *h->fuse;
  VsmStage &S = V.st;
  const size_t F = (size_t)n_frames, T = (size_t)n_tracks, N = (size_t)n_obs, NF = F > 0 ? (size_t)feat_offsets[n_frames] : 0;
  const RoGrid grid = ro_grid(width, height);
  const size_t B = (size_t)ro_frame_bins(grid);
  if (F * B > 0x7fffffff || NF > 0x7fffffff) return VSM_EHIP;  // (an index the device cannot hold)
  const FuBlocks L(F, T, N, NF, src.feat ? NF : 0, B);
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
    L.use_rank.host(S)[t] = (int32_t)tracks_in_use;
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
  int64_t frames_searched = 0;
  for (size_t g = 0; g < F; g++) frames_searched += (L.valid.host(S)[g] && L.search.host(S)[g]) ? 1 : 0;
  if (frames_searched * tracks_in_use > 0x7fffffff) return VSM_EARG;  // (more candidates than an index counts: search fewer frames)
  // the search once with its proposals kept in places per track, or twice: by the option, else by the places' size
  const bool compact = h->sw.fuse_compact >= 0 ? h->sw.fuse_compact != 0 : FuSlotBlocks((size_t)tracks_in_use, (size_t)frames_searched).dev_bytes <= FU_PLACES_MAX;
  const FuSlotBlocks SL(compact ? (size_t)tracks_in_use : 0, (size_t)frames_searched);
  // ---- from here on the call replaces the last result ----
  HIPCHK(V.replace(L, h->stream, t0));
  HIPCHK(V.ps.events());
  if (compact) HIPCHK(V.ss.grow_dev(SL.dev_bytes + 256, h->stream));
  for (size_t g = 0; g < F; g++) L.frame_feat.host(S)[g] = src.feat ? L.feat.dev(S) + RO_FEAT_INTS * (size_t)feat_offsets[g] : src.resident[g];
  FuDevice d;
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
  d.use_rank = L.use_rank.dev(S);
  if (compact) {
    d.slots = SL.slots.dev(V.ss, SL.out_at);
    d.slots_uv = SL.uv.dev(V.ss, SL.out_at);
    d.slot_stride = (int32_t)frames_searched;
  }
  d.owner = L.owner.dev(S, L.out_at);
  d.bins = L.bins.dev(S, L.out_at);
  d.bins_part = L.bins_part.dev(S, L.out_at);
  d.bins_total = L.bins_total.dev(S, L.out_at);
  d.sorted = L.sorted.dev(S, L.out_at);
  d.scan = L.scan.dev(S, L.out_at);
  d.scan_part = L.scan_part.dev(S, L.out_at);
  d.choice = L.choice.dev(S, L.out_at);
  d.totals = L.totals.dev(S, L.out_at);
  d.partner = L.partner.dev(S, L.out_at);
  d.fused_into = L.fused_into.dev(S, L.out_at);
  d.offsets_after = L.offsets_after.dev(S, L.out_at);
  d.obs_src = L.obs_src.dev(S, L.out_at);
  d.frame_counts = L.frame_counts.dev(S, L.out_at);
  d.stats = L.stats.dev(S, L.out_at);
  d.f = f;
  d.cu = cu;
  d.cv = cv;
  d.prm = fu_as_reobserve(prm);
  d.grid = grid;
  d.n_frames = n_frames;
  d.n_tracks = n_tracks;
  d.n_obs = (int32_t)n_obs;
  d.n_feat = (int32_t)NF;
  d.width = width;
  d.height = height;
  int32_t n_prop = 0;
  FuPropBlocks C(0);
  // what a call without a launch returns: no proposals, no partners, the tracks as they are
  memset(S.pin_out, 0, L.out.at);
  memset(S.pin_out, 0xff, L.ones_bytes);
  memcpy(L.offsets_after.host(S), offsets, (T + 1) * 4);
  for (size_t i = 0; i < N; i++) L.obs_src.host(S)[i] = (int32_t)i;
  if (n_tracks > 0 && n_frames > 0) {
    const VsmDrain fail{h->stream};  // a call that fails after something was enqueued: drain the device, report
    VSM_CHK(hipEventRecord(S.ev[0], h->stream));
    VSM_CHK(hipMemcpyAsync(S.dev, S.pin_in, L.in.at, hipMemcpyHostToDevice, h->stream));
    // the counts the kernels add to and the bins start at zero; a track without partner or survivor, a feature nobody owns
    // and a track that has not bid hold all bits set
    VSM_CHK(hipMemsetAsync(S.dev + L.out_at, 0, L.bins.at + L.bins.n * 4, h->stream));
    VSM_CHK(hipMemsetAsync(S.dev + L.out_at, 0xff, L.ones_bytes, h->stream));
    if (NF > 0) VSM_CHK(hipMemsetAsync(d.owner, 0xff, NF * 4, h->stream));
    VSM_CHK(hipMemsetAsync(d.choice, 0xff, T * 8, h->stream));
    VSM_CHK(hipEventRecord(S.ev[1], h->stream));
    vsm_fuse_launch_count(h->stream, h->prof, d);
    VSM_CHK(hipGetLastError());
    // the first wait: the proposals' number sizes their block
    VSM_CHK(hipMemcpyAsync(L.totals.host(S), d.totals, 8, hipMemcpyDeviceToHost, h->stream));
    VSM_CHK(hipStreamSynchronize(h->stream));
    n_prop = L.totals.host(S)[0];
    if (n_prop < 0) return fail(VSM_EHIP);  // (cannot be: the bound was checked)
    C = FuPropBlocks((size_t)n_prop);
    VSM_CHK(V.ps.grow_dev(C.dev_bytes, h->stream));
    VSM_CHK(V.ps.grow_out(C.out.at, h->stream));
    d.prop = C.prop.dev(V.ps, C.out_at);
    d.prop_uv = C.uv.dev(V.ps, C.out_at);
    vsm_fuse_launch_fuse(h->stream, h->prof, d, n_prop);
    VSM_CHK(hipGetLastError());
    VSM_CHK(hipEventRecord(S.ev[2], h->stream));
    VSM_CHK(hipMemcpyAsync(S.pin_out, S.dev + L.out_at, L.out.at, hipMemcpyDeviceToHost, h->stream));
    if (n_prop > 0) VSM_CHK(hipMemcpyAsync(V.ps.pin_out, V.ps.dev + C.out_at, C.out.at, hipMemcpyDeviceToHost, h->stream));
    // the second wait: the call's end
    VSM_CHK(hipStreamSynchronize(h->stream));
    VSM_CHK(hipGetLastError());
    if (h->prof.on) h->prof.resolve();
    S.elapsed();
  }
  // ---- into the handle's vectors ----
  VsmKeep K(true);
  L.partner.keep(K, S, V.partner);
  L.fused_into.keep(K, S, V.fused_into);
  L.offsets_after.keep(K, S, V.offsets_after);
  L.obs_src.keep(K, S, V.obs_src);
  L.frame_counts.keep(K, S, V.frame_counts);
  K.add(V.prop, n_prop > 0 ? C.prop.host(V.ps) : nullptr, (size_t)n_prop * FU_PROP_INTS);
  K.add(V.prop_uv, n_prop > 0 ? C.uv.host(V.ps) : nullptr, (size_t)n_prop * 2);
  K.run(h->pool);
  for (int q = 0; q < FU_STATS; q++) V.stats[q] = (int64_t)L.stats.host(S)[q];
  V.close();
  return VSM_OK;
}

static const VsmFuse *fuse_result(vsm_handle *h) { return (h && h->fuse && h->fuse->have) ? h->fuse : nullptr; }

extern "C" {

int vsm_fuse_run(vsm_handle *h, int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *search, double f, double cu, double cv,
                 int32_t width, int32_t height, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const int32_t *obs_feat, const double *xyz,
                 const uint8_t *use, const int32_t *ref_obs, const int32_t *feat_offsets, const int32_t *feat, const vsm_fuse_params *params) {
  if (!h || !fu_params_ok(params)) return VSM_EARG;
  const double t0 = now_us();
  const vsm_reobserve_params ro = fu_as_reobserve(*params);
  if (ro_check_features(n_frames, width, height, feat_offsets, feat) < 0) return VSM_EARG;
  const int64_t n_obs = ro_check_tracks(&ro, n_frames, poses, width, height, n_tracks, offsets, obs_frames, obs_feat, xyz, ref_obs, feat_offsets);
  if (n_obs < 0) return VSM_EARG;
  const int32_t zero = 0;
  const RoSource src{nullptr, obs_frames, obs_feat, feat ? feat : &zero, nullptr};
  return fuse_run(h, t0, n_frames, poses, pose_valid, search, f, cu, cv, width, height, n_tracks, n_obs, n_tracks > 0 ? offsets : &zero, xyz, ref_obs, feat_offsets,
                  src, *params, [=](int32_t t) { return !use || use[t]; });
}

int vsm_points_fuse(vsm_handle *h, const double *poses, const uint8_t *pose_valid, const uint8_t *search, double f, double cu, double cv,
                    const vsm_fuse_params *params) {
  if (!h) return VSM_EARG;
  const double t0 = now_us();
  TracksInput in;
  const int rc = in.take(h, true, nullptr, nullptr);
  if (rc != VSM_OK) return rc;
  const VsmPairs *P = h->pairs;
  if (in.T->side != 0 || pairs_image(h, 0, 0) < 0 || P->n_frames != in.n_frames) return VSM_ENOTREADY;
  const int32_t width = P->ctx.dims.w, height = P->ctx.dims.h;
  if (!fu_params_ok(params) || !ro_dims_ok(width, height) || !poses) return VSM_EARG;
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
  return fuse_run(h, t0, in.n_frames, poses, pose_valid, search, f, cu, cv, width, height, in.n_tracks, in.n_obs, in.T->offsets.data(), in.P->xyz.data(), nullptr,
                  feat_offsets.data(), src, *params, [=](int32_t t) { return status[t] == 0; });
}

void vsm_fuse_count(vsm_handle *h, int32_t *n_prop, int32_t *n_fusions) {
  const VsmFuse *V = fuse_result(h);
  if (n_prop) *n_prop = V ? (int32_t)(V->prop.size() / FU_PROP_INTS) : 0;
  if (n_fusions) *n_fusions = V ? (int32_t)V->stats[FU_STAT_FUSIONS] : 0;
}
int32_t vsm_fuse_get(vsm_handle *h, int32_t *prop8, double *uv) {
  const VsmFuse *V = fuse_result(h);
  if (!V) return 0;
  vsm_copy_wanted(V->prop, prop8);
  vsm_copy_wanted(V->prop_uv, uv);
  return (int32_t)(V->prop.size() / FU_PROP_INTS);
}
int32_t vsm_fuse_get_tracks(vsm_handle *h, int32_t *partner, int32_t *fused_into) {
  const VsmFuse *V = fuse_result(h);
  if (!V) return 0;
  vsm_copy_wanted(V->partner, partner);
  vsm_copy_wanted(V->fused_into, fused_into);
  return (int32_t)V->partner.size();
}
int32_t vsm_fuse_get_merged(vsm_handle *h, int32_t *offsets_after, int32_t *obs_src) {
  const VsmFuse *V = fuse_result(h);
  if (!V) return 0;
  vsm_copy_wanted(V->offsets_after, offsets_after);
  vsm_copy_wanted(V->obs_src, obs_src);
  return (int32_t)V->obs_src.size();
}
int32_t vsm_fuse_get_frames(vsm_handle *h, int32_t *counts2) {
  const VsmFuse *V = fuse_result(h);
  if (!V) return 0;
  vsm_copy_wanted(V->frame_counts, counts2);
  return (int32_t)(V->frame_counts.size() / 2);
}
void vsm_fuse_get_stats(vsm_handle *h, int64_t *out13) { vsm_result_get(fuse_result(h), &VsmFuse::stats, out13); }
void vsm_fuse_get_timings(vsm_handle *h, double *out4) { vsm_result_get(fuse_result(h), &VsmFuse::timings, out4); }

}  // extern "C"
