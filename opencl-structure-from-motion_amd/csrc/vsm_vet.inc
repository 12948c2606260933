// Vetting of observations by reprojection error (included by vsm_api.cpp; DESIGN.md section 5, INTEGRATION.md).
//
// The step between rounds of adjustment: every observation's residual at the given poses and points, the verdicts, and the
// track set without the outliers (vsm_vet.h has the definition, vsm_vet.hip the kernels).  The host's part: the frames'
// states (12 doubles per frame), one pinned block with them, the validity bytes, the offsets, a frame index and a pixel per
// observation (12 bytes per observation), the points and the use bytes (29 bytes per track); one copy up, the kernels, one
// copy back at the results' upper bounds (9 bytes per observation, 36 per track, 12 per frame) - so the call waits once, at
// its end; then the counts per code and per status.  vsm_points_vet fills the same block from the handle's last track and
// point results, reading every observation's pixel from the match it names (tracks_gather, vsm_points.inc).  Blocks: VetBlocks
// (vsm_layouts.h); round trip, result record, keep (on the pool), getters' copies: vsm_stage.h; prologue: TracksInput.
struct VsmVet : VsmResult<VET_CODES + VET_STATUSES> {  // the staging and the last result's stats and timings (vsm_stage.h)
  std::vector<uint8_t> code;
  std::vector<float> r2;
  std::vector<int32_t> status, n_in, frame_lo, frame_hi, frame_counts, kept_offsets, kept_index;
  std::vector<double> ss, worst;
};

static void vet_destroy(vsm_handle *h) { vsm_result_destroy(h->vet); }

// The arguments have been checked.  fill(obs_frames, uv) writes the n_obs frame indices and pixels into the pinned block;
// use_of(t) is track t's use byte.
template <class Fill, class UseOf>
static int vet_run(vsm_handle *h, double t0, int32_t n_frames, const double *poses, const uint8_t *pose_valid, double f, double cu, double cv, int32_t n_tracks,
                   int64_t n_obs, const int32_t *offsets, const double *xyz, const vsm_vet_params &prm, Fill fill, UseOf use_of) {
  HIPCHK(hipSetDevice(h->device));
  if (!h->vet) h->vet = new VsmVet();
  VsmVet &V = *h->vet;
  VsmStage &S = V.st;
  const size_t F = (size_t)n_frames, T = (size_t)n_tracks, N = (size_t)n_obs;
  const VetBlocks L(F, T, N);
  HIPCHK(S.grow_in(L.in.at, h->stream));
  HIPCHK(S.grow_out(L.out.at, h->stream));
  // ---- pack ----
  for (size_t g = 0; g < F; g++) pts_rigid_inverse(poses + 12 * g, L.states.host(S) + 12 * g);
  vsm_mask_bytes(pose_valid, F, L.valid.host(S));
  memcpy(L.offsets.host(S), offsets, (T + 1) * 4);
  if (T > 0) memcpy(L.xyz.host(S), xyz, T * 24);
  for (size_t t = 0; t < T; t++) L.use.host(S)[t] = use_of((int32_t)t) ? 1 : 0;
  fill(L.obs_frames.host(S), L.uv.host(S));
  // ---- from here on the call replaces the last result ----
  HIPCHK(V.replace(L, h->stream, t0));
  VetDevice d;
  memset(&d, 0, sizeof(d));
  d.states = L.states.dev(S);
  d.valid = L.valid.dev(S);
  d.offsets = L.offsets.dev(S);
  d.obs_frames = L.obs_frames.dev(S);
  d.uv = L.uv.dev(S);
  d.xyz = L.xyz.dev(S);
  d.use = L.use.dev(S);
  d.code = L.code.dev(S, L.out_at);
  d.r2 = L.r2.dev(S, L.out_at);
  d.status = L.status.dev(S, L.out_at);
  d.n_in = L.n_in.dev(S, L.out_at);
  d.frame_lo = L.frame_lo.dev(S, L.out_at);
  d.frame_hi = L.frame_hi.dev(S, L.out_at);
  d.ss = L.ss.dev(S, L.out_at);
  d.worst = L.worst.dev(S, L.out_at);
  d.frame_counts = L.frame_counts.dev(S, L.out_at);
  d.kept_offsets = L.kept_offsets.dev(S, L.out_at);
  d.kept_index = L.kept_index.dev(S, L.out_at);
  d.totals = L.totals.dev(S, L.out_at);
  d.scan = L.scan.dev(S, L.out_at);
  d.scan_part = L.scan_part.dev(S, L.out_at);
  d.f = f;
  d.cu = cu;
  d.cv = cv;
  d.prm = prm;
  d.n_tracks = n_tracks;
  if (n_tracks > 0) {  // (the frames' counts are zero before the kernels add to them)
    const int rc = S.round_trip(
        h->stream, h->prof, L, [&] { return hipMemsetAsync(d.frame_counts, 0, F * 12 + 4, h->stream); }, [&] { vsm_vet_launch(h->stream, h->prof, d); });
    if (rc != VSM_OK) return rc;
  } else {  // no track: every frame's counts are zero, the pruned set is empty
    memset(L.frame_counts.host(S), 0, F * 12 + 4);
    memset(L.kept_offsets.host(S), 0, 4);
    memset(L.totals.host(S), 0, 8);
  }
  // ---- into the handle's vectors; the counts per code and per status ----
  const int32_t n_kept = L.totals.host(S)[1];
  VsmKeep K(true);
  L.code.keep(K, S, V.code);
  L.r2.keep(K, S, V.r2);
  L.status.keep(K, S, V.status);
  L.n_in.keep(K, S, V.n_in);
  L.frame_lo.keep(K, S, V.frame_lo);
  L.frame_hi.keep(K, S, V.frame_hi);
  L.ss.keep(K, S, V.ss);
  L.worst.keep(K, S, V.worst);
  L.frame_counts.keep(K, S, V.frame_counts);
  L.kept_offsets.keep(K, S, V.kept_offsets);
  K.add(V.kept_index, L.kept_index.host(S), n_kept > 0 ? (size_t)n_kept : 0);  // (the block holds n_obs at most)
  K.run(h->pool);
  // observations per code without a walk over them: the frames' counts have codes 0, 3 and 4, the unused tracks' lengths are
  // code 1, and code 2 is the rest
  for (size_t g = 0; g < F; g++) {
    V.stats[VET_INLIER] += V.frame_counts[3 * g];
    V.stats[VET_BEHIND] += V.frame_counts[3 * g + 1];
    V.stats[VET_GATED] += V.frame_counts[3 * g + 2];
  }
  for (size_t t = 0; t < T; t++) {
    if (V.status[t] >= 0 && V.status[t] < VET_STATUSES) V.stats[VET_CODES + V.status[t]]++;
    if (V.status[t] == 1) V.stats[VET_UNUSED] += offsets[t + 1] - offsets[t];
  }
  V.stats[VET_NO_POSE] = (int64_t)N - V.stats[VET_INLIER] - V.stats[VET_BEHIND] - V.stats[VET_GATED] - V.stats[VET_UNUSED];
  V.close();
  return VSM_OK;
}

static const VsmVet *vet_result(vsm_handle *h) { return (h && h->vet && h->vet->have) ? h->vet : nullptr; }

extern "C" {

int vsm_vet_run(vsm_handle *h, int32_t n_frames, const double *poses, const uint8_t *pose_valid, double f, double cu, double cv, int32_t n_tracks,
                const int32_t *offsets, const int32_t *obs_frames, const float *uv, const double *xyz, const uint8_t *use, const vsm_vet_params *params) {
  if (!h) return VSM_EARG;
  const double t0 = now_us();
  const int64_t n_obs = pts_check_points(vet_params_ok(params), n_frames, poses, n_tracks, offsets, obs_frames, uv, xyz);
  if (n_obs < 0) return VSM_EARG;
  const int32_t zero = 0;
  return vet_run(h, t0, n_frames, poses, pose_valid, f, cu, cv, n_tracks, n_obs, n_tracks > 0 ? offsets : &zero, xyz, *params, ObsCopy{n_obs, obs_frames, uv},
                 [=](int32_t t) { return !use || use[t]; });
}

int vsm_points_vet(vsm_handle *h, const vsm_p_match *const *lists, const int32_t *counts, const double *poses, const uint8_t *pose_valid, double f, double cu,
                   double cv, const vsm_vet_params *params) {
  if (!h) return VSM_EARG;
  const double t0 = now_us();
  TracksInput in;
  const int rc = in.take(h, true, lists, counts);
  if (rc != VSM_OK) return rc;
  if (!vet_params_ok(params) || (in.n_frames > 0 && !poses)) return VSM_EARG;
  const int32_t *status = in.P->status.data();
  return vet_run(
      h, t0, in.n_frames, poses, pose_valid, f, cu, cv, in.n_tracks, in.n_obs, in.T->offsets.data(), in.P->xyz.data(), *params,
      [&](int32_t *fr, float *px) { tracks_gather(h, *in.T, in.lists, fr, px); }, [=](int32_t t) { return status[t] == 0; });
}

int32_t vsm_tracks_pixels(vsm_handle *h, const vsm_p_match *const *lists, const int32_t *counts, int32_t *obs_frames_out, float *uv_out) {
  if (!h) return VSM_EARG;
  TracksInput in;
  const int rc = in.take(h, false, lists, counts);
  if (rc != VSM_OK) return rc;
  const size_t n_obs = (size_t)in.n_obs;
  if (n_obs > 0 && obs_frames_out && uv_out) {
    tracks_gather(h, *in.T, in.lists, obs_frames_out, uv_out);
  } else if (n_obs > 0 && (obs_frames_out || uv_out)) {  // one of the two: through a block for the other
    std::vector<int32_t> fr(obs_frames_out ? 0 : n_obs);
    std::vector<float> px(uv_out ? 0 : 2 * n_obs);
    tracks_gather(h, *in.T, in.lists, obs_frames_out ? obs_frames_out : fr.data(), uv_out ? uv_out : px.data());
  }
  return (int32_t)n_obs;
}

void vsm_vet_count(vsm_handle *h, int32_t *n_tracks, int32_t *n_obs, int32_t *n_kept) {
  const VsmVet *V = vet_result(h);
  if (n_tracks) *n_tracks = V ? (int32_t)V->status.size() : 0;
  if (n_obs) *n_obs = V ? (int32_t)V->code.size() : 0;
  if (n_kept) *n_kept = V ? (int32_t)V->kept_index.size() : 0;
}
int32_t vsm_vet_get_obs(vsm_handle *h, uint8_t *code, float *r2) {
  const VsmVet *V = vet_result(h);
  if (!V) return 0;
  vsm_copy_wanted(V->code, code);
  vsm_copy_wanted(V->r2, r2);
  return (int32_t)V->code.size();
}
int32_t vsm_vet_get_tracks(vsm_handle *h, int32_t *status, int32_t *n_in, int32_t *frame_lo, int32_t *frame_hi, double *ss, double *worst) {
  const VsmVet *V = vet_result(h);
  if (!V) return 0;
  vsm_copy_wanted(V->status, status);
  vsm_copy_wanted(V->n_in, n_in);
  vsm_copy_wanted(V->frame_lo, frame_lo);
  vsm_copy_wanted(V->frame_hi, frame_hi);
  vsm_copy_wanted(V->ss, ss);
  vsm_copy_wanted(V->worst, worst);
  return (int32_t)V->status.size();
}
int32_t vsm_vet_get_frames(vsm_handle *h, int32_t *counts3) {
  const VsmVet *V = vet_result(h);
  if (!V) return 0;
  vsm_copy_wanted(V->frame_counts, counts3);
  return (int32_t)(V->frame_counts.size() / 3);
}
int32_t vsm_vet_get_kept(vsm_handle *h, int32_t *kept_offsets, int32_t *kept_index) {
  const VsmVet *V = vet_result(h);
  if (!V) return 0;
  vsm_copy_wanted(V->kept_offsets, kept_offsets);
  vsm_copy_wanted(V->kept_index, kept_index);
  return (int32_t)V->kept_index.size();
}
void vsm_vet_get_stats(vsm_handle *h, int64_t *out9) { vsm_result_get(vet_result(h), &VsmVet::stats, out9); }
void vsm_vet_get_timings(vsm_handle *h, double *out4) { vsm_result_get(vet_result(h), &VsmVet::timings, out4); }

}  // extern "C"
