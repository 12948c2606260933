// Track triangulation (included by vsm_api.cpp; DESIGN.md section 5, INTEGRATION.md).
//
// The step after the tracks: a track's pixels and the frames' poses become a 3-D point, and the poorly conditioned points
// are marked (vsm_points.h has the per-track definition, vsm_points.hip the kernel).  The host's part: the per-frame
// matrices (27 doubles per frame), one pinned block with them, the offsets, a frame index and a pixel per observation (12
// bytes per observation) and the flags; one copy up, one kernel, one copy back (52 bytes per track); then libm's acos on the
// ray values, which decides status 9.  vsm_tracks_triangulate fills the same block from the handle's last track result,
// reading every observation's pixel from the match it names.  Blocks: PtsBlocks (vsm_layouts.h); round trip, result record,
// keep and getters' copies: vsm_stage.h.  The handle forms' prologue (TracksInput), their observations as a source for the
// grouping (TracksObs) and the pixels' gathering live here.
struct VsmPoints : VsmResult<10> {  // the staging and the last result's stats and timings (vsm_stage.h)
  std::vector<int32_t> status, type, updates;
  std::vector<double> xyz, dist, angle;
};

static void points_destroy(vsm_handle *h) { vsm_result_destroy(h->points); }

// The arguments have been checked.  fill(obs_frames, uv) writes the n_obs frame indices and pixels into the pinned block.
template <class Fill>
static int points_run(vsm_handle *h, double t0, int32_t n_frames, const double *poses, const uint8_t *pose_valid, double f, double cu, double cv, int32_t n_tracks,
                      int64_t n_obs, const int32_t *offsets, const uint8_t *flags, const vsm_triangulate_params &prm, Fill fill) {
  HIPCHK(hipSetDevice(h->device));
  if (!h->points) h->points = new VsmPoints();
  VsmPoints &P = *h->points;
  VsmStage &S = P.st;
  const size_t T = (size_t)n_tracks;
  const PtsBlocks L((size_t)n_frames, T, (size_t)n_obs);
  HIPCHK(S.grow_in(L.in.at, h->stream));
  HIPCHK(S.grow_out(L.out.at, h->stream));
  // ---- pack ----
  for (int32_t k = 0; k < n_frames; k++) pts_frame(poses + 12 * (size_t)k, f, cu, cv, L.frames.host(S) + k);
  vsm_mask_bytes(pose_valid, (size_t)n_frames, L.valid.host(S));
  memcpy(L.offsets.host(S), offsets, (T + 1) * 4);
  if (flags)
    memcpy(L.flags.host(S), flags, T);
  else
    memset(L.flags.host(S), 0, T);
  fill(L.obs_frames.host(S), L.uv.host(S));
  // ---- from here on the call replaces the last result ----
  HIPCHK(P.replace(L, h->stream, t0));
  PtsDevice d;
  memset(&d, 0, sizeof(d));
  d.frames = L.frames.dev(S);
  d.valid = L.valid.dev(S);
  d.offsets = L.offsets.dev(S);
  d.obs_frames = L.obs_frames.dev(S);
  d.uv = L.uv.dev(S);
  d.flags = L.flags.dev(S);
  d.status = L.status.dev(S, L.out_at);
  d.type = L.type.dev(S, L.out_at);
  d.updates = L.updates.dev(S, L.out_at);
  d.xyz = L.xyz.dev(S, L.out_at);
  d.dist = L.dist.dev(S, L.out_at);
  d.ray = L.ray.dev(S, L.out_at);
  pts_road(prm.cam_pitch, prm.cam_height, d.road);
  d.max_dist = prm.max_dist;
  d.n_tracks = n_tracks;
  d.point_type = prm.point_type;
  d.min_track_length = prm.min_track_length;
  if (n_tracks > 0) {
    const int rc = S.round_trip(h->stream, h->prof, L, vsm_no_pre, [&] { vsm_points_launch(h->stream, h->prof, d); });
    if (rc != VSM_OK) return rc;
  }
  // ---- into the handle's vectors; the angle and status 9 need libm ----
  VsmKeep K;
  L.status.keep(K, S, P.status);
  L.type.keep(K, S, P.type);
  L.updates.keep(K, S, P.updates);
  L.xyz.keep(K, S, P.xyz);
  L.dist.keep(K, S, P.dist);
  P.angle.assign(T, 0.0);
  pts_finish(n_tracks, prm.min_angle, P.status.data(), L.ray.host(S), P.angle.data());
  for (size_t t = 0; t < T; t++)
    if (P.status[t] >= 0 && P.status[t] < 10) P.stats[P.status[t]]++;
  P.close();
  return VSM_OK;
}

static const VsmPoints *points_result(vsm_handle *h) { return (h && h->points && h->points->have) ? h->points : nullptr; }

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

// The observation source (vsm_resect.h) "the handle's track result": an observation's frame from its row, its pixel from
// the match list the row names - read inside the grouping, for the rows alone.
struct TracksObs {
  const int32_t *obs;
  const vsm_p_match *const *lists;
  int32_t side;
  int32_t frame_of(int32_t i) const { return obs[4 * (size_t)i]; }
  void pixel_of(int32_t i, float *u, float *v) const { tracks_pixel(obs + 4 * (size_t)i, lists, side, u, v); }
};

// the grouping's runner of the device paths: the handle's pool
static inline auto pool_run(vsm_handle *h) {
  return [h](int n, const std::function<void(int)> &fn) { h->pool->run(n, fn); };
}

// What a handle form works on (vsm_tracks_triangulate, vsm_points_resect, vsm_points_vet, vsm_points_adjust, vsm_tracks_pixels).  take() tests
// in the order the callers see: the track result and - with_points - the point result of the same tracks, else
// VSM_ENOTREADY; then the match lists the observations name: the caller's, checked against the result's counts (VSM_EARG),
// or - lists == NULL - those of the last vsm_pairs_run, if the tracks came from them and they still stand (VSM_ENOTREADY).
// The form's own parameters come after it.
struct TracksInput {
  const VsmTracks *T = nullptr;
  const VsmPoints *P = nullptr;
  const vsm_p_match *const *lists = nullptr;
  int32_t n_tracks = 0, n_frames = 0;
  int64_t n_obs = 0;
  std::vector<const vsm_p_match *> own;  // the pairs run's lists
  std::vector<int32_t> own_counts;
  int take(vsm_handle *h, bool with_points, const vsm_p_match *const *caller_lists, const int32_t *counts) {
    T = tracks_result(h);
    P = with_points ? points_result(h) : nullptr;
    if (!T || (with_points && (!P || P->status.size() != T->flags.size()))) return VSM_ENOTREADY;
    const int32_t n_pairs = (int32_t)T->pair_base.size() - 1;
    lists = caller_lists;
    if (!lists) {
      if (!T->from_pairs || !pairs_last_lists(h, own, own_counts) || (int32_t)own.size() != n_pairs) return VSM_ENOTREADY;
      for (int32_t k = 0; k < n_pairs; k++)
        if (own_counts[k] != T->pair_base[k + 1] - T->pair_base[k]) return VSM_ENOTREADY;  // (a later vsm_pairs_run has replaced them)
      lists = own.data();
    } else {
      if (n_pairs > 0 && !counts) return VSM_EARG;
      for (int32_t k = 0; k < n_pairs; k++)
        if (counts[k] != T->pair_base[k + 1] - T->pair_base[k] || (counts[k] > 0 && !lists[k])) return VSM_EARG;
    }
    n_tracks = (int32_t)T->flags.size();
    n_frames = T->n_frames;
    n_obs = (int64_t)T->obs.size() / 4;
    return VSM_OK;
  }
  // What vsm_points_resect and vsm_points_adjust do behind take(): the tracks whose point was kept as use bytes, into the
  // stage's own vector, and the observations as a source.
  // (locals: the bytes stored may alias the vectors, and the loop would reload count and pointers for every track)
  TracksObs kept_obs(std::vector<uint8_t> &use) const {
    const int32_t n = n_tracks;
    const int32_t *status = P->status.data();
    use.resize((size_t)n + 1);
    uint8_t *u = use.data();
    for (int32_t t = 0; t < n; t++) u[t] = status[t] == 0 ? 1 : 0;
    return TracksObs{T->obs.data(), lists, T->side};
  }
};

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

// the fill of the general forms (vsm_triangulate_run, vsm_vet_run): the caller's arrays as they are
struct ObsCopy {
  int64_t n_obs;
  const int32_t *obs_frames;
  const float *uv;
  void operator()(int32_t *fr, float *px) const {
    if (n_obs > 0) {
      memcpy(fr, obs_frames, (size_t)n_obs * 4);
      memcpy(px, uv, (size_t)n_obs * 8);
    }
  }
};

extern "C" {

int vsm_triangulate_run(vsm_handle *h, int32_t n_frames, const double *poses, const uint8_t *pose_valid, double f, double cu, double cv, int32_t n_tracks,
                        const int32_t *offsets, const int32_t *obs_frames, const float *uv, const uint8_t *flags, const vsm_triangulate_params *params) {
  if (!h) return VSM_EARG;
  const double t0 = now_us();
  const int64_t n_obs = pts_check_args(n_frames, poses, n_tracks, offsets, obs_frames, uv, params);
  if (n_obs < 0) return VSM_EARG;
  const int32_t zero = 0;
  return points_run(h, t0, n_frames, poses, pose_valid, f, cu, cv, n_tracks, n_obs, n_tracks > 0 ? offsets : &zero, flags, *params, ObsCopy{n_obs, obs_frames, uv});
}

int vsm_tracks_triangulate(vsm_handle *h, const vsm_p_match *const *lists, const int32_t *counts, const double *poses, const uint8_t *pose_valid, double f,
                           double cu, double cv, const vsm_triangulate_params *params) {
  if (!h) return VSM_EARG;
  const double t0 = now_us();
  TracksInput in;
  const int rc = in.take(h, false, lists, counts);
  if (rc != VSM_OK) return rc;
  if (!params || params->min_track_length < 1 || (in.n_frames > 0 && !poses)) return VSM_EARG;
  return points_run(h, t0, in.n_frames, poses, pose_valid, f, cu, cv, in.n_tracks, in.n_obs, in.T->offsets.data(), in.T->flags.data(), *params,
                    [&](int32_t *fr, float *px) { tracks_gather(h, *in.T, in.lists, fr, px); });
}

int32_t vsm_points_count(vsm_handle *h) { return points_result(h) ? (int32_t)h->points->status.size() : 0; }
int32_t vsm_points_get(vsm_handle *h, int32_t *status, double *xyz, int32_t *type, int32_t *updates, double *dist, double *angle) {
  const VsmPoints *P = points_result(h);
  if (!P) return 0;
  vsm_copy_wanted(P->status, status);
  vsm_copy_wanted(P->xyz, xyz);
  vsm_copy_wanted(P->type, type);
  vsm_copy_wanted(P->updates, updates);
  vsm_copy_wanted(P->dist, dist);
  vsm_copy_wanted(P->angle, angle);
  return (int32_t)P->status.size();
}
void vsm_points_get_stats(vsm_handle *h, int64_t *out10) { vsm_result_get(points_result(h), &VsmPoints::stats, out10); }
void vsm_points_get_timings(vsm_handle *h, double *out4) { vsm_result_get(points_result(h), &VsmPoints::timings, out4); }

}  // extern "C"
