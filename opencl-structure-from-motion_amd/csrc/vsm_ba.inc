// Joint adjustment of poses and points (included by vsm_api.cpp; DESIGN.md section 5, INTEGRATION.md).
//
// The step that moves both sides at once (vsm_ba.h has the definition and the schedule, vsm_ba.hip the kernels).  The host's
// part is the resection's: the rows grouped by frame with the stable counting sort on the pool - 16 bytes per row here, the
// observation's index rides along -, one pinned block with the poses, the masks, the row table, the tracks' offsets and
// frames and the points; one copy up, the schedule's launches with a wait per round on the control block (or, with the
// option adjust_fixed, every launch at once: profiles/README.md has the comparison), one copy back.  vsm_points_adjust fills
// the same block from the handle's last track and point results, as vsm_points_resect does.  Blocks: BaBlocks
// (vsm_layouts.h); round trip, result record, keep, getters' copies: vsm_stage.h; prologue: TracksInput (vsm_points.inc).
struct VsmAdjust : VsmResult<16> {
  std::vector<int32_t> fstatus, rows, factive, tstatus, hist_i;
  std::vector<double> poses, xyz, hist_d;
  int32_t rounds = 0;
  std::vector<int32_t> g_count;  // the grouping's counts per (chunk of tracks, frame)
  std::vector<uint8_t> g_use;    // vsm_points_adjust: the tracks whose point was kept
};

static void adjust_destroy(vsm_handle *h) { vsm_result_destroy(h->adjust); }

// The arguments have been checked.  frame_of(i) / pixel_of(i, &u, &v): observation i's frame and pixel (vsm_resect.h).
template <class FrameOf, class PixelOf>
static int adjust_run(vsm_handle *h, double t0, int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *refine, double f, double cu,
                      double cv, int32_t n_tracks, const int32_t *offsets, FrameOf frame_of, PixelOf pixel_of, const double *xyz, const uint8_t *use,
                      const vsm_adjust_params &prm) {
  HIPCHK(hipSetDevice(h->device));
  VsmAdjust &R = *h->adjust;
  VsmStage &S = R.st;
  const size_t F = (size_t)n_frames, T = (size_t)n_tracks;
  // ---- group: the counts first (they size the block), as resect_run does ----
  const int64_t n_obs = n_tracks > 0 ? offsets[n_tracks] : 0;
  const int chunks = (int)std::max<int64_t>(1, std::min<int64_t>(32, n_obs / 512));
  const auto first_track = [&](int c) { return (int32_t)((int64_t)n_tracks * c / chunks); };
  std::vector<int32_t> &cnt = R.g_count;
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
  const BaBlocks L(F, T, (size_t)row_off[F], (size_t)n_obs, (size_t)prm.max_rounds);
  HIPCHK(S.grow_in(L.in.at, h->stream));
  HIPCHK(S.grow_out(L.out.at, h->stream));
  if (F > 0) memcpy(L.poses.host(S), poses, F * 96);
  for (size_t g = 0; g < F; g++) {
    L.valid.host(S)[g] = (!pose_valid || pose_valid[g]) ? 1 : 0;
    L.refine.host(S)[g] = (!refine || refine[g]) ? 1 : 0;
  }
  for (size_t t = 0; t < T; t++) L.use.host(S)[t] = (!use || use[t]) ? 1 : 0;
  memcpy(L.row_off.host(S), row_off.data(), (F + 1) * 4);
  if (L.rows.n > 0)
    h->pool->run(chunks, [&](int c) { ba_group_fill(first_track(c), first_track(c + 1), offsets, use, frame_of, pixel_of, cnt.data() + (size_t)c * F, L.rows.host(S)); });
  memcpy(L.offsets.host(S), offsets, (T + 1) * 4);
  for (int64_t i = 0; i < n_obs; i++) L.obs_frames.host(S)[i] = frame_of((int32_t)i);
  if (T > 0) memcpy(L.xyz.host(S), xyz, T * 24);
  // ---- from here on the call replaces the last result ----
  HIPCHK(R.replace(L, h->stream, t0));
  BaData d;
  memset(&d, 0, sizeof(d));
  d.poses = L.poses.dev(S);
  d.valid = L.valid.dev(S);
  d.refine = L.refine.dev(S);
  d.use = L.use.dev(S);
  d.row_off = L.row_off.dev(S);
  d.rows = L.rows.dev(S);
  d.offsets = L.offsets.dev(S);
  d.obs_frames = L.obs_frames.dev(S);
  d.xyz_in = L.xyz.dev(S);
  d.state = L.state.dev(S, L.out_at);
  d.trial_state = L.trial_state.dev(S, L.out_at);
  d.trial_X = L.trial_X.dev(S, L.out_at);
  d.active = L.active.dev(S, L.out_at);
  d.lin = L.lin.dev(S, L.out_at);
  d.usum = L.usum.dev(S, L.out_at);
  d.cnt = L.cnt.dev(S, L.out_at);
  d.ud = L.ud.dev(S, L.out_at);
  d.uinv = L.uinv.dev(S, L.out_at);
  d.vinv = L.vinv.dev(S, L.out_at);
  d.gp = L.gp.dev(S, L.out_at);
  d.zt = L.zt.dev(S, L.out_at);
  d.ffree = L.ffree.dev(S, L.out_at);
  d.tfree = L.tfree.dev(S, L.out_at);
  d.moved = L.moved.dev(S, L.out_at);
  d.b = L.cg.dev(S, L.out_at);
  d.x = d.b + 6 * F;
  d.r = d.x + 6 * F;
  d.z = d.r + 6 * F;
  d.p = d.z + 6 * F;
  d.q = d.p + 6 * F;
  d.tcost = L.tcost.dev(S, L.out_at);
  d.tbehind = L.tbehind.dev(S, L.out_at);
  d.ctl = L.ctl.dev(S, L.out_at);
  d.fstatus = L.fstatus.dev(S, L.out_at);
  d.factive = L.factive.dev(S, L.out_at);
  d.tstatus = L.tstatus.dev(S, L.out_at);
  d.out_poses = L.out_poses.dev(S, L.out_at);
  d.out_xyz = L.out_xyz.dev(S, L.out_at);
  d.hist_d = L.hist_d.dev(S, L.out_at);
  d.hist_i = L.hist_i.dev(S, L.out_at);
  d.f = f;
  d.cu = cu;
  d.cv = cv;
  d.prm = prm;
  d.n_frames = n_frames;
  d.n_tracks = n_tracks;
  hipError_t waited = hipSuccess;
  // (the waits per round land in the control block's place in the pinned output, which the final copy overwrites)
  const int rc = S.round_trip(h->stream, h->prof, L, vsm_no_pre, [&] { waited = vsm_ba_launch(h->stream, h->prof, d, L.ctl.host(S), h->sw.adjust_fixed != 0); });
  if (rc != VSM_OK) return rc;
  if (waited != hipSuccess) return VsmDrain{h->stream}(VSM_EHIP);
  // ---- into the handle's vectors ----
  const BaCtl ctl = *L.ctl.host(S);
  VsmKeep K;
  L.fstatus.keep(K, S, R.fstatus);
  L.factive.keep(K, S, R.factive);
  L.tstatus.keep(K, S, R.tstatus);
  L.out_poses.keep(K, S, R.poses);
  L.out_xyz.keep(K, S, R.xyz);
  L.hist_d.keep(K, S, R.hist_d);
  L.hist_i.keep(K, S, R.hist_i);
  R.rounds = ctl.round;
  R.rows.resize(F);
  for (size_t g = 0; g < F; g++) R.rows[g] = row_off[g + 1] - row_off[g];
  ba_stats(n_frames, R.fstatus.data(), n_tracks, R.tstatus.data(), ctl, R.stats);
  R.close();
  return VSM_OK;
}

static const VsmAdjust *adjust_result(vsm_handle *h) { return (h && h->adjust && h->adjust->have) ? h->adjust : nullptr; }

extern "C" {

int vsm_adjust_run(vsm_handle *h, int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *refine, double f, double cu, double cv,
                   int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv, const double *xyz, const uint8_t *use,
                   const vsm_adjust_params *params) {
  if (!h) return VSM_EARG;
  const double t0 = now_us();
  if (ba_check_args(n_frames, poses, n_tracks, offsets, obs_frames, uv, xyz, params) < 0) return VSM_EARG;
  if (!h->adjust) h->adjust = new VsmAdjust();
  const int32_t zero = 0;
  return adjust_run(
      h, t0, n_frames, poses, pose_valid, refine, f, cu, cv, n_tracks, n_tracks > 0 ? offsets : &zero, [=](int32_t i) { return obs_frames[i]; },
      [=](int32_t i, float *u, float *v) {
        *u = uv[2 * (size_t)i];
        *v = uv[2 * (size_t)i + 1];
      },
      xyz, use, *params);
}

int vsm_points_adjust(vsm_handle *h, const vsm_p_match *const *lists, const int32_t *counts, const double *poses, const uint8_t *pose_valid,
                      const uint8_t *refine, double f, double cu, double cv, const vsm_adjust_params *params) {
  if (!h) return VSM_EARG;
  const double t0 = now_us();
  TracksInput in;
  const int rc = in.take(h, true, lists, counts);
  if (rc != VSM_OK) return rc;
  if (!ba_params_ok(params) || (in.n_frames > 0 && !poses)) return VSM_EARG;
  if (!h->adjust) h->adjust = new VsmAdjust();
  VsmAdjust &R = *h->adjust;
  const int32_t n_tracks = in.n_tracks;
  const int32_t *status = in.P->status.data();
  R.g_use.resize((size_t)n_tracks + 1);
  uint8_t *g_use = R.g_use.data();
  for (int32_t t = 0; t < n_tracks; t++) g_use[t] = status[t] == 0 ? 1 : 0;
  const int32_t *obs = in.T->obs.data();
  const int32_t side = in.T->side;
  const vsm_p_match *const *ls = in.lists;
  return adjust_run(
      h, t0, in.n_frames, poses, pose_valid, refine, f, cu, cv, n_tracks, in.T->offsets.data(), [=](int32_t i) { return obs[4 * (size_t)i]; },
      [=](int32_t i, float *u, float *v) { tracks_pixel(obs + 4 * (size_t)i, ls, side, u, v); }, in.P->xyz.data(), g_use, *params);
}

void vsm_adjust_count(vsm_handle *h, int32_t *n_frames, int32_t *n_tracks, int32_t *n_rounds) {
  const VsmAdjust *R = adjust_result(h);
  if (n_frames) *n_frames = R ? (int32_t)R->fstatus.size() : 0;
  if (n_tracks) *n_tracks = R ? (int32_t)R->tstatus.size() : 0;
  if (n_rounds) *n_rounds = R ? R->rounds : 0;
}
int32_t vsm_adjust_get_frames(vsm_handle *h, int32_t *status, double *poses, int32_t *rows, int32_t *active) {
  const VsmAdjust *R = adjust_result(h);
  if (!R) return 0;
  vsm_copy_wanted(R->fstatus, status);
  vsm_copy_wanted(R->poses, poses);
  vsm_copy_wanted(R->rows, rows);
  vsm_copy_wanted(R->factive, active);
  return (int32_t)R->fstatus.size();
}
int32_t vsm_adjust_get_tracks(vsm_handle *h, int32_t *status, double *xyz) {
  const VsmAdjust *R = adjust_result(h);
  if (!R) return 0;
  vsm_copy_wanted(R->tstatus, status);
  vsm_copy_wanted(R->xyz, xyz);
  return (int32_t)R->tstatus.size();
}
int32_t vsm_adjust_get_history(vsm_handle *h, double *cost_before, double *cost_after, double *lambda, int32_t *cg_iters, int32_t *cg_end, int32_t *accepted,
                               int32_t *active) {
  const VsmAdjust *R = adjust_result(h);
  if (!R) return 0;
  for (int32_t k = 0; k < R->rounds; k++) {
    if (cost_before) cost_before[k] = R->hist_d[3 * (size_t)k];
    if (cost_after) cost_after[k] = R->hist_d[3 * (size_t)k + 1];
    if (lambda) lambda[k] = R->hist_d[3 * (size_t)k + 2];
    if (cg_iters) cg_iters[k] = R->hist_i[4 * (size_t)k];
    if (cg_end) cg_end[k] = R->hist_i[4 * (size_t)k + 1];
    if (accepted) accepted[k] = R->hist_i[4 * (size_t)k + 2];
    if (active) active[k] = R->hist_i[4 * (size_t)k + 3];
  }
  return R->rounds;
}
void vsm_adjust_get_stats(vsm_handle *h, int64_t *out16) { vsm_result_get(adjust_result(h), &VsmAdjust::stats, out16); }
void vsm_adjust_get_timings(vsm_handle *h, double *out4) { vsm_result_get(adjust_result(h), &VsmAdjust::timings, out4); }

}  // extern "C"
