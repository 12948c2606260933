// Pose refinement against the points (included by vsm_api.cpp; DESIGN.md section 5, INTEGRATION.md).
//
// The step beside the triangulation: with the points fixed, every frame's pose moves to where its rows' reprojection error
// is smallest (vsm_resect.h has the per-frame definition, vsm_resect.hip the kernel).  The host's part: the rows grouped by
// frame with a stable counting sort on the pool - once per call, timed with the packing -, one pinned block with the poses,
// the two masks, the row offsets, the row table (12 bytes per row) and the points (24 bytes per track); one copy up, one
// kernel, one copy back (128 bytes per frame); then libm's sqrt on the two sums of squares.  vsm_points_resect fills the same block
// from the handle's last track and point results, reading every observation's pixel from the match it names.
struct VsmResect {
  VsmStage st;  // pinned input and output, the device block, the events (vsm_stage.h)
  bool have = false;
  std::vector<int32_t> status, updates, rows, used;
  std::vector<double> poses, ss_before, ss_after, rms_before, rms_after;
  std::vector<int32_t> g_count;  // the grouping's counts per (chunk of tracks, frame)
  std::vector<uint8_t> g_use;    // vsm_points_resect: the tracks whose point was kept
  int64_t stats[7] = {0, 0, 0, 0, 0, 0, 0};
  double timings[4] = {0, 0, 0, 0};
};

static void resect_destroy(vsm_handle *h) {
  VsmResect *R = h->resect;
  if (!R) return;
  R->st.release();
  delete R;
  h->resect = nullptr;
}

// The arguments have been checked.  frame_of(i) / pixel_of(i, &u, &v): observation i's frame and pixel (vsm_resect.h).
// The grouping runs on the handle's pool, a chunk of tracks per task: every chunk counts its rows per frame, the counts of
// the chunks in front give a chunk its place in every frame (so the order is that of one chunk: the sort is stable), and the
// chunks write their rows into the pinned block side by side.
template <class FrameOf, class PixelOf>
static int resect_run(vsm_handle *h, double t0, int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *refine, double f, double cu,
                      double cv, int32_t n_tracks, const int32_t *offsets, FrameOf frame_of, PixelOf pixel_of, const double *xyz, const uint8_t *use,
                      const vsm_resect_params &prm) {
  HIPCHK(hipSetDevice(h->device));
  VsmResect &R = *h->resect;
  VsmStage &S = R.st;
  const size_t F = (size_t)n_frames, T = (size_t)n_tracks;
  // ---- group: the counts first (they size the block) ----
  const int64_t n_obs = n_tracks > 0 ? offsets[n_tracks] : 0;
  const int chunks = (int)std::max<int64_t>(1, std::min<int64_t>(32, n_obs / 512));
  const auto first_track = [&](int c) { return (int32_t)((int64_t)n_tracks * c / chunks); };
  std::vector<int32_t> &cnt = R.g_count;  // [chunks][n_frames]: the counts, then the chunks' places
  cnt.assign((size_t)chunks * F, 0);
  std::vector<int32_t> row_off(F + 1, 0);
  if (n_tracks > 0 && F > 0) h->pool->run(chunks, [&](int c) { rs_group_count(first_track(c), first_track(c + 1), offsets, use, frame_of, cnt.data() + (size_t)c * F); });
  for (size_t g = 0; g < F; g++) {
    int32_t at = row_off[g];
    for (int c = 0; c < chunks; c++) {
      const int32_t n = cnt[(size_t)c * F + g];
      cnt[(size_t)c * F + g] = at;
      at += n;
    }
    row_off[g + 1] = at;
  }
  const size_t n_rows = (size_t)row_off[F];
  VsmLayout in;
  const size_t o_poses = in.take(F * 96 + 8), o_valid = in.take(F + 1), o_refine = in.take(F + 1), o_off = in.take((F + 1) * 4), o_rows = in.take(n_rows * sizeof(RsRow) + 4),
               o_xyz = in.take(T * 24 + 8);
  VsmLayout out;
  const size_t r_status = out.take(F * 4 + 4), r_updates = out.take(F * 4 + 4), r_used0 = out.take(F * 4 + 4), r_used = out.take(F * 4 + 4), r_poses = out.take(F * 96 + 8),
               r_ss0 = out.take(F * 8 + 8), r_ss1 = out.take(F * 8 + 8);
  HIPCHK(S.grow_in(in.at, h->stream));
  HIPCHK(S.grow_out(out.at, h->stream));
  if (F > 0) memcpy(S.pin_in + o_poses, poses, F * 96);
  for (size_t g = 0; g < F; g++) {
    S.pin_in[o_valid + g] = (!pose_valid || pose_valid[g]) ? 1 : 0;
    S.pin_in[o_refine + g] = (!refine || refine[g]) ? 1 : 0;
  }
  memcpy(S.pin_in + o_off, row_off.data(), (F + 1) * 4);
  if (n_rows > 0)
    h->pool->run(chunks, [&](int c) {
      rs_group_fill(first_track(c), first_track(c + 1), offsets, use, frame_of, pixel_of, cnt.data() + (size_t)c * F, (RsRow *)(S.pin_in + o_rows));
    });
  if (T > 0) memcpy(S.pin_in + o_xyz, xyz, T * 24);
  // ---- from here on the call replaces the last result ----
  R.have = false;
  memset(R.stats, 0, sizeof(R.stats));
  memset(R.timings, 0, sizeof(R.timings));
  HIPCHK(S.grow_dev(al256(in.at) + out.at, h->stream));
  HIPCHK(S.events());
  const double t1 = now_us();
  R.timings[0] = t1 - t0;
  auto fail = [&](int rc) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipGetLastError();
    return rc;
  };
  uint8_t *dout = S.dev + al256(in.at);
  RsDevice d;
  memset(&d, 0, sizeof(d));
  d.poses = (const double *)(S.dev + o_poses);
  d.valid = S.dev + o_valid;
  d.refine = S.dev + o_refine;
  d.row_off = (const int32_t *)(S.dev + o_off);
  d.rows = (const RsRow *)(S.dev + o_rows);
  d.xyz = (const double *)(S.dev + o_xyz);
  d.status = (int32_t *)(dout + r_status);
  d.updates = (int32_t *)(dout + r_updates);
  d.used_before = (int32_t *)(dout + r_used0);
  d.used = (int32_t *)(dout + r_used);
  d.out_poses = (double *)(dout + r_poses);
  d.ss_before = (double *)(dout + r_ss0);
  d.ss_after = (double *)(dout + r_ss1);
  d.f = f;
  d.cu = cu;
  d.cv = cv;
  d.prm = prm;
  d.n_frames = n_frames;
  float ms_up = 0, ms_k = 0;
  if (n_frames > 0) {
    VSM_CHK(hipEventRecord(S.ev[0], h->stream));
    VSM_CHK(hipMemcpyAsync(S.dev, S.pin_in, in.at, hipMemcpyHostToDevice, h->stream));
    VSM_CHK(hipEventRecord(S.ev[1], h->stream));
    vsm_resect_launch(h->stream, h->prof, d);
    VSM_CHK(hipGetLastError());
    VSM_CHK(hipEventRecord(S.ev[2], h->stream));
    VSM_CHK(hipMemcpyAsync(S.pin_out, dout, out.at, hipMemcpyDeviceToHost, h->stream));
    VSM_CHK(hipStreamSynchronize(h->stream));
    VSM_CHK(hipGetLastError());
    if (h->prof.on) h->prof.resolve();
    (void)hipEventElapsedTime(&ms_up, S.ev[0], S.ev[1]);
    (void)hipEventElapsedTime(&ms_k, S.ev[1], S.ev[2]);
  }
  // ---- into the handle's vectors; the two roots need libm ----
  const int32_t *o_st = (const int32_t *)(S.pin_out + r_status), *o_up = (const int32_t *)(S.pin_out + r_updates), *o_u0 = (const int32_t *)(S.pin_out + r_used0),
                *o_us = (const int32_t *)(S.pin_out + r_used);
  const double *o_po = (const double *)(S.pin_out + r_poses), *o_s0 = (const double *)(S.pin_out + r_ss0), *o_s1 = (const double *)(S.pin_out + r_ss1);
  R.status.assign(o_st, o_st + F);
  R.updates.assign(o_up, o_up + F);
  R.used.assign(o_us, o_us + F);
  R.poses.assign(o_po, o_po + 12 * F);
  R.ss_before.assign(o_s0, o_s0 + F);
  R.ss_after.assign(o_s1, o_s1 + F);
  R.rows.resize(F);
  R.rms_before.resize(F);
  R.rms_after.resize(F);
  for (size_t g = 0; g < F; g++) {
    R.rows[g] = row_off[g + 1] - row_off[g];
    R.rms_before[g] = rs_rms(o_s0[g], o_u0[g]);
    R.rms_after[g] = rs_rms(o_s1[g], (o_st[g] == 0 || o_st[g] == 6) ? o_us[g] : 0);
    if (o_st[g] >= 0 && o_st[g] < 7) R.stats[o_st[g]]++;
  }
  const double t2 = now_us();
  R.timings[1] = ms_up * 1e3;
  R.timings[2] = ms_k * 1e3;
  R.timings[3] = std::max(0.0, (t2 - t1) - R.timings[1] - R.timings[2]);
  R.have = true;
  return VSM_OK;
}

static const VsmResect *resect_result(vsm_handle *h) { return (h && h->resect && h->resect->have) ? h->resect : nullptr; }

extern "C" {

int vsm_resect_run(vsm_handle *h, int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *refine, double f, double cu, double cv,
                   int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv, const double *xyz, const uint8_t *use,
                   const vsm_resect_params *params) {
  if (!h) return VSM_EARG;
  const double t0 = now_us();
  if (rs_check_args(n_frames, poses, n_tracks, offsets, obs_frames, uv, xyz, params) < 0) return VSM_EARG;
  if (!h->resect) h->resect = new VsmResect();
  const int32_t zero = 0;
  return resect_run(
      h, t0, n_frames, poses, pose_valid, refine, f, cu, cv, n_tracks, n_tracks > 0 ? offsets : &zero, [=](int32_t i) { return obs_frames[i]; },
      [=](int32_t i, float *u, float *v) {
        *u = uv[2 * (size_t)i];
        *v = uv[2 * (size_t)i + 1];
      },
      xyz, use, *params);
}

int vsm_points_resect(vsm_handle *h, const vsm_p_match *const *lists, const int32_t *counts, const double *poses, const uint8_t *pose_valid,
                      const uint8_t *refine, double f, double cu, double cv, const vsm_resect_params *params) {
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
  if (rs_check_args(n_frames, poses, 0, &zero, nullptr, nullptr, nullptr, params) < 0) return VSM_EARG;
  if (!h->resect) h->resect = new VsmResect();
  VsmResect &R = *h->resect;
  R.g_use.resize((size_t)n_tracks + 1);
  for (int32_t t = 0; t < n_tracks; t++) R.g_use[t] = Pp->status[t] == 0 ? 1 : 0;
  // the pixels are read from the match lists inside the grouping, for the rows alone (tracks_pixel, vsm_points.inc)
  const int32_t *obs = T.obs.data();
  const int32_t side = T.side;
  return resect_run(
      h, t0, n_frames, poses, pose_valid, refine, f, cu, cv, n_tracks, T.offsets.data(), [=](int32_t i) { return obs[4 * (size_t)i]; },
      [=](int32_t i, float *u, float *v) { tracks_pixel(obs + 4 * (size_t)i, lists, side, u, v); },
      Pp->xyz.data(), R.g_use.data(), *params);
}

int32_t vsm_resect_count(vsm_handle *h) {
  const VsmResect *R = resect_result(h);
  return R ? (int32_t)R->status.size() : 0;
}
int32_t vsm_resect_get(vsm_handle *h, int32_t *status, double *poses, int32_t *updates, int32_t *rows, int32_t *used, double *ss_before, double *ss_after,
                       double *rms_before, double *rms_after) {
  const VsmResect *R = resect_result(h);
  if (!R) return 0;
  const size_t F = R->status.size();
  if (F > 0) {
    if (status) memcpy(status, R->status.data(), F * 4);
    if (poses) memcpy(poses, R->poses.data(), F * 96);
    if (updates) memcpy(updates, R->updates.data(), F * 4);
    if (rows) memcpy(rows, R->rows.data(), F * 4);
    if (used) memcpy(used, R->used.data(), F * 4);
    if (ss_before) memcpy(ss_before, R->ss_before.data(), F * 8);
    if (ss_after) memcpy(ss_after, R->ss_after.data(), F * 8);
    if (rms_before) memcpy(rms_before, R->rms_before.data(), F * 8);
    if (rms_after) memcpy(rms_after, R->rms_after.data(), F * 8);
  }
  return (int32_t)F;
}
void vsm_resect_get_stats(vsm_handle *h, int64_t *out7) {
  const VsmResect *R = resect_result(h);
  vsm_copy_or_zero(R ? &R->stats : nullptr, out7);
}
void vsm_resect_get_timings(vsm_handle *h, double *out4) {
  const VsmResect *R = resect_result(h);
  vsm_copy_or_zero(R ? &R->timings : nullptr, out4);
}

}  // extern "C"
