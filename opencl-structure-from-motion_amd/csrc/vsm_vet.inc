// Vetting of observations by reprojection error (included by vsm_api.cpp; DESIGN.md section 5, INTEGRATION.md).
//
// The step between rounds of adjustment: every observation's residual at the given poses and points, the verdicts, and the
// track set without the outliers (vsm_vet.h has the definition, vsm_vet.hip the kernels).  The host's part: the frames'
// states (12 doubles per frame), one pinned block with them, the validity bytes, the offsets, a frame index and a pixel per
// observation (12 bytes per observation), the points and the use bytes (29 bytes per track); one copy up, the kernels, one
// copy back at the results' upper bounds (9 bytes per observation, 36 per track, 12 per frame) - so the call waits once, at
// its end; then the counts per code and per status.  vsm_points_vet fills the same block from the handle's last track and
// point results, reading every observation's pixel from the match it names (tracks_gather, vsm_points.inc).
struct VsmVet {
  VsmStage st;  // pinned input and output, the device block, the events (vsm_stage.h)
  bool have = false;
  std::vector<uint8_t> code;
  std::vector<float> r2;
  std::vector<int32_t> status, n_in, frame_lo, frame_hi, frame_counts, kept_offsets, kept_index;
  std::vector<double> ss, worst;
  int64_t stats[VET_CODES + VET_STATUSES] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double timings[4] = {0, 0, 0, 0};
};

static void vet_destroy(vsm_handle *h) {
  VsmVet *V = h->vet;
  if (!V) return;
  V->st.release();
  delete V;
  h->vet = nullptr;
}

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
  VsmLayout in;
  const size_t o_states = in.take(F * 96 + 8), o_valid = in.take(F + 1), o_offsets = in.take((T + 1) * 4), o_fr = in.take(N * 4 + 4), o_uv = in.take(N * 8 + 8),
               o_xyz = in.take(T * 24 + 8), o_use = in.take(T + 1);
  VsmLayout out;
  const size_t r_code = out.take(N + 1), r_r2 = out.take(N * 4 + 4), r_status = out.take(T * 4 + 4), r_nin = out.take(T * 4 + 4), r_lo = out.take(T * 4 + 4),
               r_hi = out.take(T * 4 + 4), r_ss = out.take(T * 8 + 8), r_worst = out.take(T * 8 + 8), r_fc = out.take(F * 12 + 4), r_koff = out.take((T + 1) * 4),
               r_kidx = out.take(N * 4 + 4), r_totals = out.take(8);
  VsmLayout work = out;  // behind the results, not copied back
  const size_t w_scan = work.take(T * 8 + 8), w_part = work.take(trk_scan_part_items(n_tracks) * 8 + 8);
  HIPCHK(S.grow_in(in.at, h->stream));
  HIPCHK(S.grow_out(out.at, h->stream));
  // ---- pack ----
  double *p_states = (double *)(S.pin_in + o_states);
  for (size_t g = 0; g < F; g++) {
    pts_rigid_inverse(poses + 12 * g, p_states + 12 * g);
    S.pin_in[o_valid + g] = (!pose_valid || pose_valid[g]) ? 1 : 0;
  }
  memcpy(S.pin_in + o_offsets, offsets, (T + 1) * 4);
  if (T > 0) memcpy(S.pin_in + o_xyz, xyz, T * 24);
  for (size_t t = 0; t < T; t++) S.pin_in[o_use + t] = use_of((int32_t)t) ? 1 : 0;
  fill((int32_t *)(S.pin_in + o_fr), (float *)(S.pin_in + o_uv));
  // ---- from here on the call replaces the last result ----
  V.have = false;
  memset(V.stats, 0, sizeof(V.stats));
  memset(V.timings, 0, sizeof(V.timings));
  HIPCHK(S.grow_dev(al256(in.at) + work.at, h->stream));
  HIPCHK(S.events());
  const double t1 = now_us();
  V.timings[0] = t1 - t0;
  auto fail = [&](int rc) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipGetLastError();
    return rc;
  };
  uint8_t *dout = S.dev + al256(in.at);
  VetDevice d;
  memset(&d, 0, sizeof(d));
  d.states = (const double *)(S.dev + o_states);
  d.valid = S.dev + o_valid;
  d.offsets = (const int32_t *)(S.dev + o_offsets);
  d.obs_frames = (const int32_t *)(S.dev + o_fr);
  d.uv = (const float *)(S.dev + o_uv);
  d.xyz = (const double *)(S.dev + o_xyz);
  d.use = S.dev + o_use;
  d.code = dout + r_code;
  d.r2 = (float *)(dout + r_r2);
  d.status = (int32_t *)(dout + r_status);
  d.n_in = (int32_t *)(dout + r_nin);
  d.frame_lo = (int32_t *)(dout + r_lo);
  d.frame_hi = (int32_t *)(dout + r_hi);
  d.ss = (double *)(dout + r_ss);
  d.worst = (double *)(dout + r_worst);
  d.frame_counts = (int32_t *)(dout + r_fc);
  d.kept_offsets = (int32_t *)(dout + r_koff);
  d.kept_index = (int32_t *)(dout + r_kidx);
  d.totals = (int32_t *)(dout + r_totals);
  d.scan = (int32_t *)(dout + w_scan);
  d.scan_part = (int32_t *)(dout + w_part);
  d.f = f;
  d.cu = cu;
  d.cv = cv;
  d.prm = prm;
  d.n_tracks = n_tracks;
  float ms_up = 0, ms_k = 0;
  if (n_tracks > 0) {
    VSM_CHK(hipEventRecord(S.ev[0], h->stream));
    VSM_CHK(hipMemcpyAsync(S.dev, S.pin_in, in.at, hipMemcpyHostToDevice, h->stream));
    VSM_CHK(hipMemsetAsync(d.frame_counts, 0, F * 12 + 4, h->stream));
    VSM_CHK(hipEventRecord(S.ev[1], h->stream));
    vsm_vet_launch(h->stream, h->prof, d);
    VSM_CHK(hipGetLastError());
    VSM_CHK(hipEventRecord(S.ev[2], h->stream));
    VSM_CHK(hipMemcpyAsync(S.pin_out, dout, out.at, hipMemcpyDeviceToHost, h->stream));
    VSM_CHK(hipStreamSynchronize(h->stream));
    VSM_CHK(hipGetLastError());
    if (h->prof.on) h->prof.resolve();
    (void)hipEventElapsedTime(&ms_up, S.ev[0], S.ev[1]);
    (void)hipEventElapsedTime(&ms_k, S.ev[1], S.ev[2]);
  } else {  // no track: every frame's counts are zero, the pruned set is empty
    memset(S.pin_out + r_fc, 0, F * 12 + 4);
    memset(S.pin_out + r_koff, 0, 4);
    memset(S.pin_out + r_totals, 0, 8);
  }
  // ---- into the handle's vectors; the counts per code and per status ----
  const int32_t n_kept = ((const int32_t *)(S.pin_out + r_totals))[1];
  const uint8_t *o_code = S.pin_out + r_code;
  const float *o_r2 = (const float *)(S.pin_out + r_r2);
  const int32_t *o_st = (const int32_t *)(S.pin_out + r_status), *o_nin = (const int32_t *)(S.pin_out + r_nin), *o_lo = (const int32_t *)(S.pin_out + r_lo),
                *o_hi = (const int32_t *)(S.pin_out + r_hi), *o_fc = (const int32_t *)(S.pin_out + r_fc), *o_koff = (const int32_t *)(S.pin_out + r_koff),
                *o_kidx = (const int32_t *)(S.pin_out + r_kidx);
  const double *o_ss = (const double *)(S.pin_out + r_ss), *o_worst = (const double *)(S.pin_out + r_worst);
  // (the copies run on the handle's pool, half a megabyte per task: on one thread they were most of this part)
  struct Piece {
    uint8_t *dst;
    const uint8_t *src;
    size_t bytes;
  };
  std::vector<Piece> pieces;
  const auto keep = [&](auto &vec, const auto *src, size_t n) {
    vec.resize(n);
    const size_t bytes = n * sizeof(*src), step = (size_t)512 << 10;
    for (size_t at = 0; at < bytes; at += step) pieces.push_back({(uint8_t *)vec.data() + at, (const uint8_t *)src + at, std::min(step, bytes - at)});
  };
  keep(V.code, o_code, N);
  keep(V.r2, o_r2, N);
  keep(V.status, o_st, T);
  keep(V.n_in, o_nin, T);
  keep(V.frame_lo, o_lo, T);
  keep(V.frame_hi, o_hi, T);
  keep(V.ss, o_ss, T);
  keep(V.worst, o_worst, T);
  keep(V.frame_counts, o_fc, 3 * F);
  keep(V.kept_offsets, o_koff, T + 1);
  keep(V.kept_index, o_kidx, n_kept > 0 ? (size_t)n_kept : 0);
  if (!pieces.empty()) h->pool->run((int)pieces.size(), [&](int i) { memcpy(pieces[i].dst, pieces[i].src, pieces[i].bytes); });
  // observations per code without a walk over them: the frames' counts have codes 0, 3 and 4, the unused tracks' lengths are
  // code 1, and code 2 is the rest
  for (size_t g = 0; g < F; g++) {
    V.stats[VET_INLIER] += o_fc[3 * g];
    V.stats[VET_BEHIND] += o_fc[3 * g + 1];
    V.stats[VET_GATED] += o_fc[3 * g + 2];
  }
  for (size_t t = 0; t < T; t++) {
    if (o_st[t] >= 0 && o_st[t] < VET_STATUSES) V.stats[VET_CODES + o_st[t]]++;
    if (o_st[t] == 1) V.stats[VET_UNUSED] += offsets[t + 1] - offsets[t];
  }
  V.stats[VET_NO_POSE] = (int64_t)N - V.stats[VET_INLIER] - V.stats[VET_BEHIND] - V.stats[VET_GATED] - V.stats[VET_UNUSED];
  const double t2 = now_us();
  V.timings[1] = ms_up * 1e3;
  V.timings[2] = ms_k * 1e3;
  V.timings[3] = std::max(0.0, (t2 - t1) - V.timings[1] - V.timings[2]);
  V.have = true;
  return VSM_OK;
}

// a getter's array, where the caller wants it
template <typename E>
static inline void vet_copy(const std::vector<E> &v, E *out) {
  if (out && !v.empty()) memcpy(out, v.data(), v.size() * sizeof(E));
}
static const VsmVet *vet_result(vsm_handle *h) { return (h && h->vet && h->vet->have) ? h->vet : nullptr; }

extern "C" {

int vsm_vet_run(vsm_handle *h, int32_t n_frames, const double *poses, const uint8_t *pose_valid, double f, double cu, double cv, int32_t n_tracks,
                const int32_t *offsets, const int32_t *obs_frames, const float *uv, const double *xyz, const uint8_t *use, const vsm_vet_params *params) {
  if (!h) return VSM_EARG;
  const double t0 = now_us();
  const int64_t n_obs = vet_check_args(n_frames, poses, n_tracks, offsets, obs_frames, uv, xyz, params);
  if (n_obs < 0) return VSM_EARG;
  const int32_t zero = 0;
  return vet_run(
      h, t0, n_frames, poses, pose_valid, f, cu, cv, n_tracks, n_obs, n_tracks > 0 ? offsets : &zero, xyz, *params,
      [&](int32_t *fr, float *px) {
        if (n_obs > 0) {
          memcpy(fr, obs_frames, (size_t)n_obs * 4);
          memcpy(px, uv, (size_t)n_obs * 8);
        }
      },
      [=](int32_t t) { return !use || use[t]; });
}

int vsm_points_vet(vsm_handle *h, const vsm_p_match *const *lists, const int32_t *counts, const double *poses, const uint8_t *pose_valid, double f, double cu,
                   double cv, const vsm_vet_params *params) {
  if (!h) return VSM_EARG;
  const double t0 = now_us();
  const VsmTracks *Tp = h->tracks;
  const VsmPoints *Pp = points_result(h);
  if (!Tp || !Tp->have || !Pp || Pp->status.size() != Tp->flags.size()) return VSM_ENOTREADY;
  const VsmTracks &T = *Tp;
  std::vector<const vsm_p_match *> own;
  std::vector<int32_t> own_counts;
  const int rc = tracks_lists(h, T, lists, counts, own, own_counts);
  if (rc != VSM_OK) return rc;
  const int32_t n_tracks = (int32_t)T.flags.size(), n_frames = T.n_frames;
  // (the track result's own arrays satisfy the general form's checks: only the parameters and the poses are the caller's)
  const int32_t zero = 0;
  if (vet_check_args(n_frames, poses, 0, &zero, nullptr, nullptr, nullptr, params) < 0) return VSM_EARG;
  const int32_t *status = Pp->status.data();
  return vet_run(
      h, t0, n_frames, poses, pose_valid, f, cu, cv, n_tracks, (int64_t)T.obs.size() / 4, T.offsets.data(), Pp->xyz.data(), *params,
      [&](int32_t *fr, float *px) { tracks_gather(h, T, lists, fr, px); }, [=](int32_t t) { return status[t] == 0; });
}

int32_t vsm_tracks_pixels(vsm_handle *h, const vsm_p_match *const *lists, const int32_t *counts, int32_t *obs_frames_out, float *uv_out) {
  if (!h) return VSM_EARG;
  const VsmTracks *Tp = h->tracks;
  if (!Tp || !Tp->have) return VSM_ENOTREADY;
  const VsmTracks &T = *Tp;
  std::vector<const vsm_p_match *> own;
  std::vector<int32_t> own_counts;
  const int rc = tracks_lists(h, T, lists, counts, own, own_counts);
  if (rc != VSM_OK) return rc;
  const size_t n_obs = T.obs.size() / 4;
  if (n_obs > 0 && obs_frames_out && uv_out) {
    tracks_gather(h, T, lists, obs_frames_out, uv_out);
  } else if (n_obs > 0 && (obs_frames_out || uv_out)) {  // one of the two: through a block for the other
    std::vector<int32_t> fr(obs_frames_out ? 0 : n_obs);
    std::vector<float> px(uv_out ? 0 : 2 * n_obs);
    tracks_gather(h, T, lists, obs_frames_out ? obs_frames_out : fr.data(), uv_out ? uv_out : px.data());
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
  vet_copy(V->code, code);
  vet_copy(V->r2, r2);
  return (int32_t)V->code.size();
}
int32_t vsm_vet_get_tracks(vsm_handle *h, int32_t *status, int32_t *n_in, int32_t *frame_lo, int32_t *frame_hi, double *ss, double *worst) {
  const VsmVet *V = vet_result(h);
  if (!V) return 0;
  vet_copy(V->status, status);
  vet_copy(V->n_in, n_in);
  vet_copy(V->frame_lo, frame_lo);
  vet_copy(V->frame_hi, frame_hi);
  vet_copy(V->ss, ss);
  vet_copy(V->worst, worst);
  return (int32_t)V->status.size();
}
int32_t vsm_vet_get_frames(vsm_handle *h, int32_t *counts3) {
  const VsmVet *V = vet_result(h);
  if (!V) return 0;
  vet_copy(V->frame_counts, counts3);
  return (int32_t)(V->frame_counts.size() / 3);
}
int32_t vsm_vet_get_kept(vsm_handle *h, int32_t *kept_offsets, int32_t *kept_index) {
  const VsmVet *V = vet_result(h);
  if (!V) return 0;
  vet_copy(V->kept_offsets, kept_offsets);
  vet_copy(V->kept_index, kept_index);
  return (int32_t)V->kept_index.size();
}
void vsm_vet_get_stats(vsm_handle *h, int64_t *out9) {
  const VsmVet *V = vet_result(h);
  vsm_copy_or_zero(V ? &V->stats : nullptr, out9);
}
void vsm_vet_get_timings(vsm_handle *h, double *out4) {
  const VsmVet *V = vet_result(h);
  vsm_copy_or_zero(V ? &V->timings : nullptr, out4);
}

}  // extern "C"
