// Joint adjustment of poses and points (included by vsm_api.cpp; DESIGN.md section 5, INTEGRATION.md).
//
// The step that moves both sides at once (vsm_ba.h has the definition and the schedule, vsm_ba.hip the kernels).  The host's
// part is the resection's: the rows grouped by frame with the stable counting sort on the pool - 16 bytes per row here, the
// observation's index rides along -, one pinned block with the poses, the masks, the row table, the tracks' offsets and
// frames and the points; one copy up, the schedule's launches with a wait per round on the control block (or, with the
// option adjust_fixed, every launch at once: profiles/README.md has the comparison), one copy back.  vsm_points_adjust fills
// the same block from the handle's last track and point results, as vsm_points_resect does.  Grouping and the caller's
// arrays as observations: RsGroup, RsObsArrays (vsm_resect.h); blocks, their packing and BaData's binding: BaBlocks
// (vsm_layouts.h); round trip, result record, keep, getters' copies: vsm_stage.h; prologue and the handle's observations:
// TracksInput, TracksObs (vsm_points.inc).
struct VsmAdjust : VsmResult<16> {
  std::vector<int32_t> fstatus, rows, factive, tstatus, hist_i;
  std::vector<double> poses, xyz, hist_d;
  int32_t rounds = 0;
  std::vector<int32_t> g_count;  // the grouping's counts per (chunk of tracks, frame)
  std::vector<uint8_t> g_use;    // vsm_points_adjust: the tracks whose point was kept
};

static void adjust_destroy(vsm_handle *h) { vsm_result_destroy(h->adjust); }

// The arguments have been checked.  obs: the observation source (vsm_resect.h), grouped on the handle's pool.
template <class Obs>
static int adjust_run(vsm_handle *h, double t0, int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *refine, double f, double cu,
                      double cv, int32_t n_tracks, const int32_t *offsets, const Obs &obs, const double *xyz, const uint8_t *use, const vsm_adjust_params &prm) {
  HIPCHK(hipSetDevice(h->device));
  VsmAdjust &R = *h->adjust;
  VsmStage &S = R.st;
  const size_t F = (size_t)n_frames;
  const int64_t n_obs = n_tracks > 0 ? offsets[n_tracks] : 0;
  // ---- group: the counts first (they size the block) ----
  RsGroup G(n_frames, n_tracks, offsets, use, obs, rs_group_chunks(n_obs), pool_run(h), R.g_count);
  const BaBlocks L(F, (size_t)n_tracks, (size_t)G.row_off[F], (size_t)n_obs, (size_t)prm.max_rounds);
  HIPCHK(S.grow_in(L.in.at, h->stream));
  HIPCHK(S.grow_out(L.out.at, h->stream));
  L.pack(S.pin_in, poses, pose_valid, refine, G, xyz);
  // ---- from here on the call replaces the last result ----
  HIPCHK(R.replace(L, h->stream, t0));
  const BaData d = L.bind(S.dev, S.dev + L.out_at, f, cu, cv, prm);
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
  for (size_t g = 0; g < F; g++) R.rows[g] = G.rows_of(g);
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
  if (pts_check_points(ba_params_ok(params), n_frames, poses, n_tracks, offsets, obs_frames, uv, xyz) < 0) return VSM_EARG;
  if (!h->adjust) h->adjust = new VsmAdjust();
  return adjust_run(h, t0, n_frames, poses, pose_valid, refine, f, cu, cv, n_tracks, offsets, RsObsArrays{obs_frames, uv}, xyz, use, *params);
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
  const TracksObs obs = in.kept_obs(h->adjust->g_use);
  return adjust_run(h, t0, in.n_frames, poses, pose_valid, refine, f, cu, cv, in.n_tracks, in.T->offsets.data(), obs, in.P->xyz.data(), h->adjust->g_use.data(), *params);
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
  ba_history(R->rounds, R->hist_d.data(), R->hist_i.data(), cost_before, cost_after, lambda, cg_iters, cg_end, accepted, active);
  return R->rounds;
}
void vsm_adjust_get_stats(vsm_handle *h, int64_t *out16) { vsm_result_get(adjust_result(h), &VsmAdjust::stats, out16); }
void vsm_adjust_get_timings(vsm_handle *h, double *out4) { vsm_result_get(adjust_result(h), &VsmAdjust::timings, out4); }

}  // extern "C"
