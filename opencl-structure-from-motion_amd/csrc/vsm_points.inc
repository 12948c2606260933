// Track triangulation (included by vsm_api.cpp; DESIGN.md section 5, INTEGRATION.md).
//
// The step after the tracks: a track's pixels and the frames' poses become a 3-D point, and the poorly conditioned points
// are marked (vsm_points.h has the per-track definition, vsm_points.hip the kernel).  The host's part: the per-frame
// matrices (27 doubles per frame), one pinned block with them, the offsets, a frame index and a pixel per observation (12
// bytes per observation) and the flags; one copy up, one kernel, one copy back (52 bytes per track); then libm's acos on the
// ray values, which decides status 9.  vsm_tracks_triangulate fills the same block from the handle's last track result,
// reading every observation's pixel from the match it names.
struct VsmPoints {
  VsmStage st;  // pinned input and output, the device block, the events (vsm_stage.h)
  bool have = false;
  std::vector<int32_t> status, type, updates;
  std::vector<double> xyz, dist, angle;
  int64_t stats[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  double timings[4] = {0, 0, 0, 0};
};

static void points_destroy(vsm_handle *h) {
  VsmPoints *P = h->points;
  if (!P) return;
  P->st.release();
  delete P;
  h->points = nullptr;
}

// The arguments have been checked.  fill(obs_frames, uv) writes the n_obs frame indices and pixels into the pinned block and
// returns false for an argument error it finds on the way (nothing is enqueued before it has returned true).
static int points_run(vsm_handle *h, double t0, int32_t n_frames, const double *poses, const uint8_t *pose_valid, double f, double cu, double cv, int32_t n_tracks,
                      int64_t n_obs, const int32_t *offsets, const uint8_t *flags, const vsm_triangulate_params &prm,
                      const std::function<bool(int32_t *, float *)> &fill) {
  HIPCHK(hipSetDevice(h->device));
  if (!h->points) h->points = new VsmPoints();
  VsmPoints &P = *h->points;
  VsmStage &S = P.st;
  const size_t T = (size_t)n_tracks;
  VsmLayout in;
  const size_t o_frames = in.take((size_t)n_frames * sizeof(PtsFrame) + 8), o_valid = in.take((size_t)n_frames + 1), o_offsets = in.take((T + 1) * 4),
               o_fr = in.take((size_t)n_obs * 4 + 4), o_uv = in.take((size_t)n_obs * 8 + 8), o_flags = in.take(T + 1);
  VsmLayout out;
  const size_t r_status = out.take(T * 4 + 4), r_type = out.take(T * 4 + 4), r_updates = out.take(T * 4 + 4), r_xyz = out.take(T * 24 + 8), r_dist = out.take(T * 8 + 8),
               r_ray = out.take(T * 8 + 8);
  HIPCHK(S.grow_in(in.at, h->stream));
  HIPCHK(S.grow_out(out.at, h->stream));
  // ---- pack ----
  PtsFrame *p_frames = (PtsFrame *)(S.pin_in + o_frames);
  uint8_t *p_valid = S.pin_in + o_valid;
  for (int32_t k = 0; k < n_frames; k++) {
    pts_frame(poses + 12 * (size_t)k, f, cu, cv, p_frames + k);
    p_valid[k] = (!pose_valid || pose_valid[k]) ? 1 : 0;
  }
  memcpy(S.pin_in + o_offsets, offsets, (T + 1) * 4);
  if (flags)
    memcpy(S.pin_in + o_flags, flags, T);
  else
    memset(S.pin_in + o_flags, 0, T);
  if (!fill((int32_t *)(S.pin_in + o_fr), (float *)(S.pin_in + o_uv))) return VSM_EARG;
  // ---- from here on the call replaces the last result ----
  P.have = false;
  memset(P.stats, 0, sizeof(P.stats));
  memset(P.timings, 0, sizeof(P.timings));
  HIPCHK(S.grow_dev(al256(in.at) + out.at, h->stream));
  HIPCHK(S.events());
  const double t1 = now_us();
  P.timings[0] = t1 - t0;
  auto fail = [&](int rc) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipGetLastError();
    return rc;
  };
  uint8_t *dout = S.dev + al256(in.at);
  PtsDevice d;
  memset(&d, 0, sizeof(d));
  d.frames = (const PtsFrame *)(S.dev + o_frames);
  d.valid = S.dev + o_valid;
  d.offsets = (const int32_t *)(S.dev + o_offsets);
  d.obs_frames = (const int32_t *)(S.dev + o_fr);
  d.uv = (const float *)(S.dev + o_uv);
  d.flags = S.dev + o_flags;
  d.status = (int32_t *)(dout + r_status);
  d.type = (int32_t *)(dout + r_type);
  d.updates = (int32_t *)(dout + r_updates);
  d.xyz = (double *)(dout + r_xyz);
  d.dist = (double *)(dout + r_dist);
  d.ray = (double *)(dout + r_ray);
  pts_road(prm.cam_pitch, prm.cam_height, d.road);
  d.max_dist = prm.max_dist;
  d.n_tracks = n_tracks;
  d.point_type = prm.point_type;
  d.min_track_length = prm.min_track_length;
  float ms_up = 0, ms_k = 0;
  if (n_tracks > 0) {
    VSM_CHK(hipEventRecord(S.ev[0], h->stream));
    VSM_CHK(hipMemcpyAsync(S.dev, S.pin_in, in.at, hipMemcpyHostToDevice, h->stream));
    VSM_CHK(hipEventRecord(S.ev[1], h->stream));
    vsm_points_launch(h->stream, h->prof, d);
    VSM_CHK(hipGetLastError());
    VSM_CHK(hipEventRecord(S.ev[2], h->stream));
    VSM_CHK(hipMemcpyAsync(S.pin_out, dout, out.at, hipMemcpyDeviceToHost, h->stream));
    VSM_CHK(hipStreamSynchronize(h->stream));
    VSM_CHK(hipGetLastError());
    if (h->prof.on) h->prof.resolve();
    (void)hipEventElapsedTime(&ms_up, S.ev[0], S.ev[1]);
    (void)hipEventElapsedTime(&ms_k, S.ev[1], S.ev[2]);
  }
  // ---- into the handle's vectors; the angle and status 9 need libm ----
  const int32_t *o_st = (const int32_t *)(S.pin_out + r_status), *o_ty = (const int32_t *)(S.pin_out + r_type), *o_up = (const int32_t *)(S.pin_out + r_updates);
  const double *o_xyz = (const double *)(S.pin_out + r_xyz), *o_di = (const double *)(S.pin_out + r_dist), *o_ray = (const double *)(S.pin_out + r_ray);
  P.status.assign(o_st, o_st + T);
  P.type.assign(o_ty, o_ty + T);
  P.updates.assign(o_up, o_up + T);
  P.xyz.assign(o_xyz, o_xyz + 3 * T);
  P.dist.assign(o_di, o_di + T);
  P.angle.assign(T, 0.0);
  pts_finish(n_tracks, prm.min_angle, P.status.data(), o_ray, P.angle.data());
  for (size_t t = 0; t < T; t++)
    if (P.status[t] >= 0 && P.status[t] < 10) P.stats[P.status[t]]++;
  const double t2 = now_us();
  P.timings[1] = ms_up * 1e3;
  P.timings[2] = ms_k * 1e3;
  P.timings[3] = std::max(0.0, (t2 - t1) - P.timings[1] - P.timings[2]);
  P.have = true;
  return VSM_OK;
}

static const VsmPoints *points_result(vsm_handle *h) { return (h && h->points && h->points->have) ? h->points : nullptr; }

// The match lists the observations of the track result T name (vsm_tracks_triangulate, vsm_points_resect): the caller's,
// checked against the result's counts, or - lists == NULL - those of the last vsm_pairs_run, if the tracks came from them
// (own / own_counts keep them).  VSM_OK, VSM_ENOTREADY or VSM_EARG.
static int tracks_lists(vsm_handle *h, const VsmTracks &T, const vsm_p_match *const *&lists, const int32_t *counts, std::vector<const vsm_p_match *> &own,
                        std::vector<int32_t> &own_counts) {
  const int32_t n_pairs = (int32_t)T.pair_base.size() - 1;
  if (!lists) {
    if (!T.from_pairs || !pairs_last_lists(h, own, own_counts) || (int32_t)own.size() != n_pairs) return VSM_ENOTREADY;
    for (int32_t k = 0; k < n_pairs; k++)
      if (own_counts[k] != T.pair_base[k + 1] - T.pair_base[k]) return VSM_ENOTREADY;  // (a later vsm_pairs_run has replaced them)
    lists = own.data();
  } else {
    if (n_pairs > 0 && !counts) return VSM_EARG;
    for (int32_t k = 0; k < n_pairs; k++)
      if (counts[k] != T.pair_base[k + 1] - T.pair_base[k] || (counts[k] > 0 && !lists[k])) return VSM_EARG;
  }
  return VSM_OK;
}

// the pixel of an observation {frame, feature, pair, 2 * match + end}, read from the match it names: end 0 = previous, 1 =
// current
static inline void tracks_pixel(const int32_t *row, const vsm_p_match *const *lists, int32_t side, float *u, float *v) {
  const vsm_p_match &m = lists[row[2]][row[3] >> 1];
  if (row[3] & 1) {
    *u = side ? m.u2c : m.u1c;
    *v = side ? m.v2c : m.v1c;
  } else {
    *u = side ? m.u2p : m.u1p;
    *v = side ? m.v2p : m.v1p;
  }
}

// every observation's frame and pixel
static void tracks_gather(vsm_handle *h, const VsmTracks &T, const vsm_p_match *const *lists, int32_t *fr, float *px) {
  const int32_t *obs = T.obs.data();
  const int32_t side = T.side;
  const int64_t n_obs = (int64_t)T.obs.size() / 4;
  const int chunks = (int)std::min<int64_t>(64, (n_obs + 4095) / 4096);
  if (chunks > 0)
    h->pool->run(chunks, [&](int c) {
      const int64_t a = n_obs * c / chunks, b = n_obs * (c + 1) / chunks;
      for (int64_t i = a; i < b; i++) {
        fr[i] = obs[4 * i];
        tracks_pixel(obs + 4 * i, lists, side, px + 2 * i, px + 2 * i + 1);
      }
    });
}

extern "C" {

int vsm_triangulate_run(vsm_handle *h, int32_t n_frames, const double *poses, const uint8_t *pose_valid, double f, double cu, double cv, int32_t n_tracks,
                        const int32_t *offsets, const int32_t *obs_frames, const float *uv, const uint8_t *flags, const vsm_triangulate_params *params) {
  if (!h) return VSM_EARG;
  const double t0 = now_us();
  const int64_t n_obs = pts_check_args(n_frames, poses, n_tracks, offsets, obs_frames, uv, params);
  if (n_obs < 0) return VSM_EARG;
  const int32_t zero = 0;
  return points_run(h, t0, n_frames, poses, pose_valid, f, cu, cv, n_tracks, n_obs, n_tracks > 0 ? offsets : &zero, flags, *params, [&](int32_t *fr, float *px) {
    if (n_obs > 0) {
      memcpy(fr, obs_frames, (size_t)n_obs * 4);
      memcpy(px, uv, (size_t)n_obs * 8);
    }
    return true;
  });
}

int vsm_tracks_triangulate(vsm_handle *h, const vsm_p_match *const *lists, const int32_t *counts, const double *poses, const uint8_t *pose_valid, double f,
                           double cu, double cv, const vsm_triangulate_params *params) {
  if (!h) return VSM_EARG;
  const double t0 = now_us();
  const VsmTracks *Tp = h->tracks;
  if (!Tp || !Tp->have) return VSM_ENOTREADY;
  const VsmTracks &T = *Tp;
  std::vector<const vsm_p_match *> own;
  std::vector<int32_t> own_counts;
  const int rc = tracks_lists(h, T, lists, counts, own, own_counts);
  if (rc != VSM_OK) return rc;
  const int32_t n_tracks = (int32_t)T.flags.size(), n_frames = T.n_frames;
  const int64_t n_obs = (int64_t)T.obs.size() / 4;
  if (!params || params->min_track_length < 1 || (n_frames > 0 && !poses)) return VSM_EARG;
  return points_run(h, t0, n_frames, poses, pose_valid, f, cu, cv, n_tracks, n_obs, T.offsets.data(), T.flags.data(), *params, [&](int32_t *fr, float *px) {
    tracks_gather(h, T, lists, fr, px);
    return true;
  });
}

int32_t vsm_points_count(vsm_handle *h) { return (h && h->points && h->points->have) ? (int32_t)h->points->status.size() : 0; }
int32_t vsm_points_get(vsm_handle *h, int32_t *status, double *xyz, int32_t *type, int32_t *updates, double *dist, double *angle) {
  if (!h || !h->points || !h->points->have) return 0;
  const VsmPoints &P = *h->points;
  const size_t T = P.status.size();
  if (T > 0) {
    if (status) memcpy(status, P.status.data(), T * 4);
    if (xyz) memcpy(xyz, P.xyz.data(), T * 24);
    if (type) memcpy(type, P.type.data(), T * 4);
    if (updates) memcpy(updates, P.updates.data(), T * 4);
    if (dist) memcpy(dist, P.dist.data(), T * 8);
    if (angle) memcpy(angle, P.angle.data(), T * 8);
  }
  return (int32_t)T;
}
void vsm_points_get_stats(vsm_handle *h, int64_t *out10) {
  const VsmPoints *P = points_result(h);
  vsm_copy_or_zero(P ? &P->stats : nullptr, out10);
}
void vsm_points_get_timings(vsm_handle *h, double *out4) {
  const VsmPoints *P = points_result(h);
  vsm_copy_or_zero(P ? &P->timings : nullptr, out4);
}

}  // extern "C"
