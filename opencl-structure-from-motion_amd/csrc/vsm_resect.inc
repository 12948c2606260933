// Pose refinement against the points (included by vsm_api.cpp; DESIGN.md section 5, INTEGRATION.md).
//
// The step beside the triangulation: with the points fixed, every frame's pose moves to where its rows' reprojection error
// is smallest (vsm_resect.h has the per-frame definition, vsm_resect.hip the kernel).  The host's part: the rows grouped by
// frame with a stable counting sort on the pool - once per call, timed with the packing -, one pinned block with the poses,
// the two masks, the row offsets, the row table (12 bytes per row) and the points (24 bytes per track); one copy up, one
// kernel, one copy back (128 bytes per frame); then libm's sqrt on the two sums of squares.  vsm_points_resect fills the same block
// from the handle's last track and point results, reading every observation's pixel from the match it names.  Grouping and
// the caller's arrays as observations: RsGroup, RsObsArrays (vsm_resect.h); blocks: RsBlocks (vsm_layouts.h); round trip,
// result record, keep, mask bytes, getters' copies: vsm_stage.h; prologue and the handle's observations: TracksInput, TracksObs
// (vsm_points.inc).
struct VsmResect : VsmResult<7> {  // the staging and the last result's stats and timings (vsm_stage.h)
  std::vector<int32_t> status, updates, rows, used;
  std::vector<double> poses, ss_before, ss_after, rms_before, rms_after;
  std::vector<int32_t> g_count;  // the grouping's counts per (chunk of tracks, frame)
  std::vector<uint8_t> g_use;    // vsm_points_resect: the tracks whose point was kept
};

static void resect_destroy(vsm_handle *h) { vsm_result_destroy(h->resect); }

// The arguments have been checked.  obs: the observation source (vsm_resect.h), grouped on the handle's pool.
template <class Obs>
static int resect_run(vsm_handle *h, double t0, int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *refine, double f, double cu,
                      double cv, int32_t n_tracks, const int32_t *offsets, const Obs &obs, const double *xyz, const uint8_t *use, const vsm_resect_params &prm) {
  HIPCHK(hipSetDevice(h->device));
  VsmResect &R = *h->resect;
  VsmStage &S = R.st;
  const size_t F = (size_t)n_frames, T = (size_t)n_tracks;
  // ---- group: the counts first (they size the block) ----
  RsGroup G(n_frames, n_tracks, offsets, use, obs, rs_group_chunks(n_tracks > 0 ? offsets[n_tracks] : 0), pool_run(h), R.g_count);
  const RsBlocks L(F, T, (size_t)G.row_off[F]);
  HIPCHK(S.grow_in(L.in.at, h->stream));
  HIPCHK(S.grow_out(L.out.at, h->stream));
  if (F > 0) memcpy(L.poses.host(S), poses, F * 96);
  vsm_mask_bytes(pose_valid, F, L.valid.host(S));
  vsm_mask_bytes(refine, F, L.refine.host(S));
  memcpy(L.row_off.host(S), G.row_off.data(), (F + 1) * 4);
  G.fill(L.rows.host(S));
  if (T > 0) memcpy(L.xyz.host(S), xyz, T * 24);
  // ---- from here on the call replaces the last result ----
  HIPCHK(R.replace(L, h->stream, t0));
  RsDevice d;
  memset(&d, 0, sizeof(d));
  d.poses = L.poses.dev(S);
  d.valid = L.valid.dev(S);
  d.refine = L.refine.dev(S);
  d.row_off = L.row_off.dev(S);
  d.rows = L.rows.dev(S);
  d.xyz = L.xyz.dev(S);
  d.status = L.status.dev(S, L.out_at);
  d.updates = L.updates.dev(S, L.out_at);
  d.used_before = L.used_before.dev(S, L.out_at);
  d.used = L.used.dev(S, L.out_at);
  d.out_poses = L.out_poses.dev(S, L.out_at);
  d.ss_before = L.ss_before.dev(S, L.out_at);
  d.ss_after = L.ss_after.dev(S, L.out_at);
  d.f = f;
  d.cu = cu;
  d.cv = cv;
  d.prm = prm;
  d.n_frames = n_frames;
  if (n_frames > 0) {
    const int rc = S.round_trip(h->stream, h->prof, L, vsm_no_pre, [&] { vsm_resect_launch(h->stream, h->prof, d); });
    if (rc != VSM_OK) return rc;
  }
  // ---- into the handle's vectors; the two roots need libm ----
  VsmKeep K;
  L.status.keep(K, S, R.status);
  L.updates.keep(K, S, R.updates);
  L.used.keep(K, S, R.used);
  L.out_poses.keep(K, S, R.poses);
  L.ss_before.keep(K, S, R.ss_before);
  L.ss_after.keep(K, S, R.ss_after);
  const int32_t *o_st = L.status.host(S), *o_u0 = L.used_before.host(S), *o_us = L.used.host(S);
  R.rows.resize(F);
  R.rms_before.resize(F);
  R.rms_after.resize(F);
  for (size_t g = 0; g < F; g++) {
    R.rows[g] = G.rows_of(g);
    R.rms_before[g] = rs_rms(R.ss_before[g], o_u0[g]);
    R.rms_after[g] = rs_rms(R.ss_after[g], (o_st[g] == 0 || o_st[g] == 6) ? o_us[g] : 0);
    if (o_st[g] >= 0 && o_st[g] < 7) R.stats[o_st[g]]++;
  }
  R.close();
  return VSM_OK;
}

static const VsmResect *resect_result(vsm_handle *h) { return (h && h->resect && h->resect->have) ? h->resect : nullptr; }

extern "C" {

int vsm_resect_run(vsm_handle *h, int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *refine, double f, double cu, double cv,
                   int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv, const double *xyz, const uint8_t *use,
                   const vsm_resect_params *params) {
  if (!h) return VSM_EARG;
  const double t0 = now_us();
  if (pts_check_points(rs_params_ok(params), n_frames, poses, n_tracks, offsets, obs_frames, uv, xyz) < 0) return VSM_EARG;
  if (!h->resect) h->resect = new VsmResect();
  return resect_run(h, t0, n_frames, poses, pose_valid, refine, f, cu, cv, n_tracks, offsets, RsObsArrays{obs_frames, uv}, xyz, use, *params);
}

int vsm_points_resect(vsm_handle *h, const vsm_p_match *const *lists, const int32_t *counts, const double *poses, const uint8_t *pose_valid,
                      const uint8_t *refine, double f, double cu, double cv, const vsm_resect_params *params) {
  if (!h) return VSM_EARG;
  const double t0 = now_us();
  TracksInput in;
  const int rc = in.take(h, true, lists, counts);
  if (rc != VSM_OK) return rc;
  if (!rs_params_ok(params) || (in.n_frames > 0 && !poses)) return VSM_EARG;
  if (!h->resect) h->resect = new VsmResect();
  const TracksObs obs = in.kept_obs(h->resect->g_use);
  return resect_run(h, t0, in.n_frames, poses, pose_valid, refine, f, cu, cv, in.n_tracks, in.T->offsets.data(), obs, in.P->xyz.data(), h->resect->g_use.data(), *params);
}

int32_t vsm_resect_count(vsm_handle *h) {
  const VsmResect *R = resect_result(h);
  return R ? (int32_t)R->status.size() : 0;
}
int32_t vsm_resect_get(vsm_handle *h, int32_t *status, double *poses, int32_t *updates, int32_t *rows, int32_t *used, double *ss_before, double *ss_after,
                       double *rms_before, double *rms_after) {
  const VsmResect *R = resect_result(h);
  if (!R) return 0;
  vsm_copy_wanted(R->status, status);
  vsm_copy_wanted(R->poses, poses);
  vsm_copy_wanted(R->updates, updates);
  vsm_copy_wanted(R->rows, rows);
  vsm_copy_wanted(R->used, used);
  vsm_copy_wanted(R->ss_before, ss_before);
  vsm_copy_wanted(R->ss_after, ss_after);
  vsm_copy_wanted(R->rms_before, rms_before);
  vsm_copy_wanted(R->rms_after, rms_after);
  return (int32_t)R->status.size();
}
void vsm_resect_get_stats(vsm_handle *h, int64_t *out7) { vsm_result_get(resect_result(h), &VsmResect::stats, out7); }
void vsm_resect_get_timings(vsm_handle *h, double *out4) { vsm_result_get(resect_result(h), &VsmResect::timings, out4); }

}  // extern "C"
