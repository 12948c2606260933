// Location of frames without a pose against the points (included by vsm_api.cpp; DESIGN.md section 5, INTEGRATION.md).
//
// The step that gives a frame a pose: RANSAC over a linear six-point resection per asked-for frame, the winner refined by the
// resection's kernel (vsm_locate.h has the definition, vsm_locate.hip the kernels).  The host's part: the rows grouped by
// frame as the resection groups them, the eligible rows and the samples of every job - a frame that is asked for and has
// enough rows - on the pool, every job from an engine of its own; one pinned block with the row offsets, the row table, the
// points, the job tables, the tiles of the count kernel and the samples; one copy up, the counts cleared, fit, count,
// winner and the resection's launch on the device-resident linear poses, one copy back, one wait; then libm's sqrt.
// vsm_points_locate fills the same block from the handle's last track and point results.  Grouping and observation sources:
// vsm_resect.h, vsm_points.inc; blocks: LcBlocks (vsm_layouts.h); round trip, result record, keep, getters' copies: vsm_stage.h.
struct VsmLocate : VsmResult<7> {  // the staging and the last result's stats and timings (vsm_stage.h)
  std::vector<int32_t> status, best, inliers, rows, eligible, updates, used;
  std::vector<double> poses, linear_poses, ss_after, rms_after;
  std::vector<int32_t> g_count;  // the grouping's counts per (chunk of tracks, frame)
  std::vector<uint8_t> g_use;    // vsm_points_locate: the tracks whose point was kept
  std::vector<int32_t> verdict, rs_status;  // what the device said, before the host's status
  size_t shape[6] = {};  // the last call's blocks: LcBlocks' F, T, R, J, K, NT (vsm_debug_locate_hypotheses finds the tables by them)
};

static void locate_destroy(vsm_handle *h) { vsm_result_destroy(h->locate); }

// The arguments have been checked.  obs: the observation source (vsm_resect.h), grouped on the handle's pool.
template <class Obs>
static int locate_run(vsm_handle *h, double t0, int32_t n_frames, const uint8_t *locate, double f, double cu, double cv, int32_t n_tracks,
                      const int32_t *offsets, const Obs &obs, const double *xyz, const uint8_t *use, const vsm_locate_params &prm) {
  HIPCHK(hipSetDevice(h->device));
  VsmLocate &R = *h->locate;
  VsmStage &S = R.st;
  const size_t F = (size_t)n_frames, T = (size_t)n_tracks, K = (size_t)prm.ransac_iters;
  // ---- group: the counts first (they size the block); the jobs and the tiles at their upper bounds ----
  RsGroup G(n_frames, n_tracks, offsets, use, obs, rs_group_chunks(n_tracks > 0 ? offsets[n_tracks] : 0), pool_run(h), R.g_count);
  std::vector<int32_t> frame_job(F, -1), job_frame, E(F, 0);
  size_t tiles_bound = 0;
  for (size_t g = 0; g < F; g++)
    if ((!locate || locate[g]) && G.rows_of(g) >= prm.min_inliers) {
      frame_job[g] = (int32_t)job_frame.size();
      job_frame.push_back((int32_t)g);
      tiles_bound += ((size_t)G.rows_of(g) + 255) / 256;
    }
  const size_t J = job_frame.size();
  const LcBlocks L(F, T, (size_t)G.row_off[F], J, K, tiles_bound);
  HIPCHK(S.grow_in(L.in.at, h->stream));
  HIPCHK(S.grow_out(L.out.at, h->stream));
  memcpy(L.row_off.host(S), G.row_off.data(), (F + 1) * 4);
  G.fill(L.rows.host(S));
  if (T > 0) memcpy(L.xyz.host(S), xyz, T * 24);
  if (F > 0) memcpy(L.frame_job.host(S), frame_job.data(), F * 4);
  if (J > 0) memcpy(L.job_frame.host(S), job_frame.data(), J * 4);
  // ---- the eligible rows of every asked-for frame and the samples of every job, a frame per task ----
  {
    const RsRow *table = L.rows.host(S);
    int32_t *job_E = L.job_E.host(S), *picks = L.picks.host(S);
    if (F > 0)
      h->pool->run(n_frames, [&](int g) {
        if (locate && !locate[g]) return;
        std::vector<int32_t> elig, deck;
        lc_eligible_rows(table + G.row_off[g], G.rows_of((size_t)g), xyz, elig);
        E[g] = (int32_t)elig.size();
        const int32_t j = frame_job[g];
        if (j < 0) return;
        job_E[j] = E[g] >= prm.min_inliers ? E[g] : 0;
        if (job_E[j]) lc_sample(prm.seed, elig.data(), E[g], (int32_t)K, picks + (size_t)j * K * LC_SAMPLE, deck);
      });
  }
  LcTile *tiles = L.tiles.host(S);
  size_t n_tiles = 0;
  for (size_t j = 0; j < J; j++)
    if (L.job_E.host(S)[j])
      for (int32_t off = 0; off < G.rows_of((size_t)job_frame[j]); off += 256) tiles[n_tiles++] = {(int32_t)j, off};
  // ---- from here on the call replaces the last result ----
  HIPCHK(R.replace(L, h->stream, t0));
  LcDevice d;
  memset(&d, 0, sizeof(d));
  d.row_off = L.row_off.dev(S);
  d.rows = L.rows.dev(S);
  d.xyz = L.xyz.dev(S);
  d.frame_job = L.frame_job.dev(S);
  d.job_frame = L.job_frame.dev(S);
  d.job_E = L.job_E.dev(S);
  d.tiles = L.tiles.dev(S);
  d.picks = L.picks.dev(S);
  d.states = L.states.dev(S, L.out_at);
  d.hvalid = L.hvalid.dev(S, L.out_at);
  d.counts = L.counts.dev(S, L.out_at);
  d.lin_valid = L.lin_valid.dev(S, L.out_at);
  d.verdict = L.verdict.dev(S, L.out_at);
  d.best = L.best.dev(S, L.out_at);
  d.inliers = L.inliers.dev(S, L.out_at);
  d.lin_poses = L.lin_poses.dev(S, L.out_at);
  d.f = f;
  d.cu = cu;
  d.cv = cv;
  d.prm = prm;
  d.n_frames = n_frames;
  d.n_jobs = (int32_t)J;
  d.n_tiles = (int32_t)n_tiles;
  // the refinement: the resection's kernel, as a caller would ask for it, on the linear poses where the winner left them
  RsDevice rd;
  memset(&rd, 0, sizeof(rd));
  rd.poses = d.lin_poses;
  rd.valid = d.lin_valid;
  rd.refine = d.lin_valid;
  rd.row_off = d.row_off;
  rd.rows = d.rows;
  rd.xyz = d.xyz;
  rd.status = L.rs_status.dev(S, L.out_at);
  rd.updates = L.rs_updates.dev(S, L.out_at);
  rd.used_before = L.rs_used_before.dev(S, L.out_at);
  rd.used = L.rs_used.dev(S, L.out_at);
  rd.out_poses = L.rs_poses.dev(S, L.out_at);
  rd.ss_before = L.rs_ss_before.dev(S, L.out_at);
  rd.ss_after = L.rs_ss_after.dev(S, L.out_at);
  rd.f = f;
  rd.cu = cu;
  rd.cv = cv;
  rd.prm = lc_resect_params(prm);
  rd.n_frames = n_frames;
  if (n_frames > 0) {
    const int rc = S.round_trip(
        h->stream, h->prof, L, [&] { return J * K > 0 ? hipMemsetAsync(d.counts, 0, J * K * 4, h->stream) : hipSuccess; },
        [&] {
          vsm_locate_launch(h->stream, h->prof, d);
          vsm_resect_launch(h->stream, h->prof, rd);
        });
    if (rc != VSM_OK) return rc;
  }
  // ---- into the handle's vectors; the status and the root on the host ----
  VsmKeep Kp;
  L.verdict.keep(Kp, S, R.verdict);
  L.rs_status.keep(Kp, S, R.rs_status);
  L.best.keep(Kp, S, R.best);
  L.inliers.keep(Kp, S, R.inliers);
  L.lin_poses.keep(Kp, S, R.linear_poses);
  L.rs_poses.keep(Kp, S, R.poses);
  L.rs_updates.keep(Kp, S, R.updates);
  L.rs_used.keep(Kp, S, R.used);
  L.rs_ss_after.keep(Kp, S, R.ss_after);
  R.status.resize(F);
  R.rows.resize(F);
  R.rms_after.resize(F);
  R.eligible = E;
  for (size_t g = 0; g < F; g++) {
    const int32_t st = lc_status(!locate || locate[g], E[g], prm.min_inliers, R.verdict[g], R.rs_status[g]);
    R.status[g] = st;
    R.rows[g] = G.rows_of(g);
    if (!(st == 0 || st == 5 || st == 6)) memset(&R.poses[12 * g], 0, 96);
    R.rms_after[g] = rs_rms(R.ss_after[g], (st == 0 || st == 6) ? R.used[g] : 0);
    R.stats[st]++;
  }
  const size_t shape[6] = {F, T, (size_t)G.row_off[F], J, K, tiles_bound};
  memcpy(R.shape, shape, sizeof(shape));
  R.close();
  return VSM_OK;
}

static const VsmLocate *locate_result(vsm_handle *h) { return (h && h->locate && h->locate->have) ? h->locate : nullptr; }

extern "C" {

int vsm_locate_run(vsm_handle *h, int32_t n_frames, const uint8_t *locate, double f, double cu, double cv, int32_t n_tracks, const int32_t *offsets,
                   const int32_t *obs_frames, const float *uv, const double *xyz, const uint8_t *use, const vsm_locate_params *params) {
  if (!h) return VSM_EARG;
  const double t0 = now_us();
  if (lc_check_args(n_frames, n_tracks, offsets, obs_frames, uv, xyz, params) < 0) return VSM_EARG;
  if (!h->locate) h->locate = new VsmLocate();
  return locate_run(h, t0, n_frames, locate, f, cu, cv, n_tracks, offsets, RsObsArrays{obs_frames, uv}, xyz, use, *params);
}

int vsm_points_locate(vsm_handle *h, const vsm_p_match *const *lists, const int32_t *counts, const uint8_t *locate, double f, double cu, double cv,
                      const vsm_locate_params *params) {
  if (!h) return VSM_EARG;
  const double t0 = now_us();
  TracksInput in;
  const int rc = in.take(h, true, lists, counts);
  if (rc != VSM_OK) return rc;
  if (!lc_params_ok(params)) return VSM_EARG;
  if (!h->locate) h->locate = new VsmLocate();
  const TracksObs obs = in.kept_obs(h->locate->g_use);
  return locate_run(h, t0, in.n_frames, locate, f, cu, cv, in.n_tracks, in.T->offsets.data(), obs, in.P->xyz.data(), h->locate->g_use.data(), *params);
}

int32_t vsm_locate_count(vsm_handle *h) {
  const VsmLocate *R = locate_result(h);
  return R ? (int32_t)R->status.size() : 0;
}
int32_t vsm_locate_get(vsm_handle *h, int32_t *status, double *poses, double *linear_poses, int32_t *best, int32_t *inliers, int32_t *rows,
                       int32_t *eligible, int32_t *updates, int32_t *used, double *ss_after, double *rms_after) {
  const VsmLocate *R = locate_result(h);
  if (!R) return 0;
  vsm_copy_wanted(R->status, status);
  vsm_copy_wanted(R->poses, poses);
  vsm_copy_wanted(R->linear_poses, linear_poses);
  vsm_copy_wanted(R->best, best);
  vsm_copy_wanted(R->inliers, inliers);
  vsm_copy_wanted(R->rows, rows);
  vsm_copy_wanted(R->eligible, eligible);
  vsm_copy_wanted(R->updates, updates);
  vsm_copy_wanted(R->used, used);
  vsm_copy_wanted(R->ss_after, ss_after);
  vsm_copy_wanted(R->rms_after, rms_after);
  return (int32_t)R->status.size();
}
// test hook: every hypothesis of the last call - the samples from the pinned block that went up, the states, their validity
// and the counts from the device block, where they lie behind the results and are never copied back by the call
int32_t vsm_debug_locate_hypotheses(vsm_handle *h, int32_t *picks, double *states, uint8_t *hvalid, int32_t *counts, int32_t *n_jobs, int32_t *n_hyps) {
  const VsmLocate *R = locate_result(h);
  if (!R) return h ? VSM_ENOTREADY : VSM_EARG;
  if (!n_jobs || !n_hyps) return VSM_EARG;
  const size_t *sh = R->shape, JK = sh[3] * sh[4];
  *n_jobs = (int32_t)sh[3];
  *n_hyps = (int32_t)sh[4];
  if (JK == 0 || sh[0] == 0) return VSM_OK;  // (a call without frames had no round trip)
  const LcBlocks L(sh[0], sh[1], sh[2], sh[3], sh[4], sh[5]);
  const VsmStage &S = R->st;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (picks) memcpy(picks, L.picks.host(S), JK * LC_SAMPLE * 4);
  if (states) HIPCHK(hipMemcpy(states, L.states.dev(S, L.out_at), JK * 96, hipMemcpyDeviceToHost));
  if (hvalid) HIPCHK(hipMemcpy(hvalid, L.hvalid.dev(S, L.out_at), JK, hipMemcpyDeviceToHost));
  if (counts) HIPCHK(hipMemcpy(counts, L.counts.dev(S, L.out_at), JK * 4, hipMemcpyDeviceToHost));
  return VSM_OK;
}
void vsm_locate_get_stats(vsm_handle *h, int64_t *out7) { vsm_result_get(locate_result(h), &VsmLocate::stats, out7); }
void vsm_locate_get_timings(vsm_handle *h, double *out4) { vsm_result_get(locate_result(h), &VsmLocate::timings, out4); }

}  // extern "C"
