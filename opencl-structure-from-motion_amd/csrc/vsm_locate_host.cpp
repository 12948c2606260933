// Location of frames against the points, the host side without HIP: the parameters' test, the eligible rows, the samples,
// and vsm_host_locate - one host thread walking the functions of vsm_locate.h with vsm_la::svd_nr for the two
// decompositions, then vsm_host_resect on the linear poses.  The host view is the CPU suite's subject, the device path's
// second opinion and the benchmark's baseline, never a fallback.
#include "vsm_locate.h"

#include <string.h>

#include <algorithm>
#include <vector>

#include "vsm_host.h"

bool lc_params_ok(const vsm_locate_params *p) {
  return p && p->ransac_iters >= 1 && p->inlier_threshold > 0 && p->inlier_threshold < HUGE_VAL && p->min_inliers >= LC_SAMPLE && p->max_updates >= 1 &&
         p->eps > 0 && p->eps < HUGE_VAL;
}

int64_t lc_check_args(int32_t n_frames, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv, const double *xyz,
                      const vsm_locate_params *params) {
  static const double no_poses = 0;  // (the shared check wants a pose array where there are frames; this call has none to give)
  return pts_check_points(lc_params_ok(params), n_frames, &no_poses, n_tracks, offsets, obs_frames, uv, xyz);
}

vsm_resect_params lc_resect_params(const vsm_locate_params &p) {
  vsm_resect_params r;
  memset(&r, 0, sizeof(r));
  r.min_observations = p.min_inliers;
  r.max_updates = p.max_updates;
  r.eps = p.eps;
  r.max_residual = p.inlier_threshold;
  r.min_depth = p.min_depth;
  return r;
}

void lc_eligible_rows(const RsRow *rows, int32_t n, const double *xyz, std::vector<int32_t> &elig) {
  elig.clear();
  for (int32_t i = 0; i < n; i++)
    if (lc_eligible(rows[i].u, rows[i].v, xyz + 3 * (size_t)rows[i].track)) elig.push_back(i);
}

// the mono fit's draw (MonoEgo::begin, vsm_mono.hip) with six cards: a partial Fisher-Yates on a persistent identity deck,
// undone after each hypothesis
void lc_sample(uint32_t seed, const int32_t *elig, int32_t E, int32_t K, int32_t *picks, std::vector<int32_t> &deck) {
  deck.resize((size_t)E);
  for (int32_t i = 0; i < E; i++) deck[i] = i;
  VsmDrawPlan plan[LC_SAMPLE];
  for (int i = 0; i < LC_SAMPLE; i++) plan[i] = vsm_sampler_plan((uint32_t)i, (uint32_t)(E - 1));
  uint32_t state = lc_seed_state(seed);
  for (int32_t k = 0; k < K; k++) {
    int32_t swapped[LC_SAMPLE];
    for (int i = 0; i < LC_SAMPLE; i++) {
      swapped[i] = (int32_t)vsm_minstd_draw(state, plan[i]);
      std::swap(deck[i], deck[swapped[i]]);
    }
    for (int i = 0; i < LC_SAMPLE; i++) picks[(size_t)k * LC_SAMPLE + i] = elig[deck[i]];
    for (int i = LC_SAMPLE - 1; i >= 0; i--) std::swap(deck[i], deck[swapped[i]]);
  }
}

namespace {

// one hypothesis on the host: LC_UNFIT, the sample is refused and S untouched; else S is written, and the hypothesis is
// LC_VALID or LC_INVALID (a state that is not finite, a sampled point not in front)
enum { LC_UNFIT = 0, LC_INVALID = 1, LC_VALID = 2 };
int host_fit(const RsRow *rows, const int32_t *pick, const double *xyz, double f, double cu, double cv, double min_depth, double *S) {
  double P[3 * LC_SAMPLE], m[3], s;
  for (int i = 0; i < LC_SAMPLE; i++)
    for (int c = 0; c < 3; c++) P[3 * i + c] = xyz[3 * (size_t)rows[pick[i]].track + c];
  if (!lc_condition(P, m, &s)) return LC_UNFIT;
  double A[LC_GROUP_DOUBLES], col[LC_N];
  for (int i = 0; i < LC_SAMPLE; i++) lc_rows(A + LC_U, i, rows[pick[i]].u, rows[pick[i]].v, P + 3 * i, m, s, f, cu, cv);
  vsm_la::svd_nr(A + LC_U, LC_N, LC_N, LC_N, A + LC_W, A + LC_V, A + LC_RV, col);
  double p[LC_N], U3[9], w3[3], V3[9], rv3[3], col3[3];
  for (int i = 0; i < LC_N; i++) p[i] = A[LC_V + i * LC_N + (LC_N - 1)];
  for (int i = 0; i < 9; i++) U3[i] = p[4 * (i / 3) + i % 3];
  vsm_la::svd_nr(U3, 3, 3, 3, w3, V3, rv3, col3);
  bool ok = lc_state(p, U3, w3, V3, m, s, S);
  for (int i = 0; i < LC_SAMPLE; i++) ok = ok && lc_in_front(S, P + 3 * i, min_depth);
  return ok ? LC_VALID : LC_INVALID;
}

// a row's vote among the frame's eligible rows elig[0 .. E) at the state S
int32_t host_count(const RsRow *rows, const int32_t *elig, int32_t E, const double *xyz, const double *S, double f, double cu, double cv, double min_depth,
                   double limit) {
  int32_t count = 0;
  for (int32_t q = 0; q < E; q++) {
    const RsRow &r = rows[elig[q]];
    if (lc_inlier(S, xyz + 3 * (size_t)r.track, r.u, r.v, f, cu, cv, min_depth, limit)) count++;
  }
  return count;
}

// the rows of the single-frame entries - pixels rows_uv[n][2], a point per row rows_xyz[n][3] - as a frame's row table
std::vector<RsRow> rows_of_arrays(int32_t n, const float *uv) {
  std::vector<RsRow> rows((size_t)n + 1);
  for (int32_t i = 0; i < n; i++) rows[i] = {i, uv[2 * (size_t)i], uv[2 * (size_t)i + 1]};
  return rows;
}

}  // namespace

extern "C" {

void vsm_locate_default_params(vsm_locate_params *p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->ransac_iters = 200;
  p->inlier_threshold = 2.0;
  p->min_inliers = 10;
  p->min_depth = 1e-10;
  p->seed = 71;
  p->max_updates = 20;
  p->eps = 1e-8;
}

int32_t vsm_host_locate(int32_t n_frames, const uint8_t *locate, double f, double cu, double cv, int32_t n_tracks, const int32_t *offsets,
                        const int32_t *obs_frames, const float *uv, const double *xyz, const uint8_t *use, const vsm_locate_params *params,
                        int32_t *status, double *poses, double *linear_poses, int32_t *best, int32_t *inliers, int32_t *rows, int32_t *eligible,
                        int32_t *updates, int32_t *used, double *ss_after, double *rms_after) {
  if (lc_check_args(n_frames, n_tracks, offsets, obs_frames, uv, xyz, params) < 0) return VSM_EARG;
  const vsm_locate_params &prm = *params;
  const size_t F = (size_t)n_frames;
  const int32_t K = prm.ransac_iters;
  // the rows by frame, one chunk
  std::vector<int32_t> at;
  RsGroup G(n_frames, n_tracks, offsets, use, RsObsArrays{obs_frames, uv}, 1, RsLoop(), at);
  std::vector<RsRow> table((size_t)G.row_off[F] + 1);
  G.fill(table.data());
  const double limit = rs_limit(prm.inlier_threshold);
  std::vector<int32_t> elig, deck, picks((size_t)K * LC_SAMPLE), E(F, 0), verdict(F, -1), win(F, -1), win_count(F, 0);
  std::vector<double> lin(12 * F, 0.0);
  std::vector<uint8_t> go(F + 1, 0);
  for (size_t g = 0; g < F; g++) {
    if (locate && !locate[g]) continue;
    const RsRow *fr = table.data() + G.row_off[g];
    lc_eligible_rows(fr, G.rows_of(g), xyz, elig);
    E[g] = (int32_t)elig.size();
    if (E[g] < prm.min_inliers) continue;
    lc_sample(prm.seed, elig.data(), E[g], K, picks.data(), deck);
    bool any_valid = false;
    double Sbest[12];
    for (int32_t k = 0; k < K; k++) {
      double S[12];
      if (host_fit(fr, &picks[(size_t)k * LC_SAMPLE], xyz, f, cu, cv, prm.min_depth, S) != LC_VALID) continue;
      any_valid = true;
      const int32_t count = host_count(fr, elig.data(), E[g], xyz, S, f, cu, cv, prm.min_depth, limit);
      if (count > win_count[g]) {
        win_count[g] = count;
        win[g] = k;
        memcpy(Sbest, S, sizeof(S));
      }
    }
    verdict[g] = lc_verdict(any_valid, win_count[g], prm.min_inliers);
    if (win[g] >= 0) pts_rigid_inverse(Sbest, &lin[12 * g]);
    go[g] = verdict[g] == 0;
  }
  // the refinement: the resection, as a caller would call it
  const vsm_resect_params rp = lc_resect_params(prm);
  std::vector<int32_t> r_status(F, 0), r_updates(F, 0), r_used(F, 0);
  std::vector<double> r_poses(12 * F, 0.0), r_ss(F, 0.0);
  if (F > 0 &&
      vsm_host_resect(n_frames, lin.data(), go.data(), go.data(), f, cu, cv, n_tracks, offsets, obs_frames, uv, xyz, use, &rp, r_status.data(), r_poses.data(),
                      r_updates.data(), nullptr, r_used.data(), nullptr, r_ss.data(), nullptr, nullptr) < 0)
    return VSM_EARG;
  for (size_t g = 0; g < F; g++) {
    const int32_t st = lc_status(!locate || locate[g], E[g], prm.min_inliers, verdict[g], r_status[g]);
    const bool posed = st == 0 || st == 5 || st == 6;
    if (status) status[g] = st;
    if (poses) {
      if (posed)
        memcpy(poses + 12 * g, &r_poses[12 * g], 96);
      else
        memset(poses + 12 * g, 0, 96);
    }
    if (linear_poses) memcpy(linear_poses + 12 * g, &lin[12 * g], 96);
    if (best) best[g] = win[g];
    if (inliers) inliers[g] = win_count[g];
    if (rows) rows[g] = G.rows_of(g);
    if (eligible) eligible[g] = E[g];
    if (updates) updates[g] = r_updates[g];
    if (used) used[g] = r_used[g];
    if (ss_after) ss_after[g] = r_ss[g];
    if (rms_after) rms_after[g] = rs_rms(r_ss[g], st == 0 || st == 6 ? r_used[g] : 0);
  }
  return n_frames;
}

// ---- the stages alone (include/visomatch.h, the debug section): what the loop above runs, on one frame of the caller ----
int32_t vsm_host_locate_sample(uint32_t seed, int32_t E, int32_t K, int32_t *picks) {
  if (E < LC_SAMPLE || K < 1 || !picks) return VSM_EARG;
  std::vector<int32_t> elig((size_t)E), deck;
  for (int32_t i = 0; i < E; i++) elig[i] = i;
  lc_sample(seed, elig.data(), E, K, picks, deck);
  return VSM_OK;
}

int32_t vsm_host_locate_fit(double f, double cu, double cv, double min_depth, int32_t n_rows, const float *rows_uv, const double *rows_xyz, const int32_t *picks,
                            int32_t K, double *states, uint8_t *valid) {
  if (n_rows < 1 || K < 1 || !rows_uv || !rows_xyz || !picks || !states || !valid) return VSM_EARG;
  for (size_t i = 0; i < (size_t)K * LC_SAMPLE; i++)
    if (picks[i] < 0 || picks[i] >= n_rows) return VSM_EARG;
  const std::vector<RsRow> rows = rows_of_arrays(n_rows, rows_uv);
  for (int32_t k = 0; k < K; k++) {
    double S[12];
    const int fit = host_fit(rows.data(), picks + (size_t)k * LC_SAMPLE, rows_xyz, f, cu, cv, min_depth, S);
    if (fit != LC_UNFIT) memcpy(states + 12 * (size_t)k, S, sizeof(S));
    valid[k] = fit == LC_VALID ? 1 : 0;
  }
  return VSM_OK;
}

int32_t vsm_host_locate_count(double f, double cu, double cv, int32_t n_rows, const float *rows_uv, const double *rows_xyz, const double *states,
                              const uint8_t *valid, int32_t K, double inlier_threshold, double min_depth, int32_t *counts) {
  if (n_rows < 0 || K < 1 || (n_rows > 0 && (!rows_uv || !rows_xyz)) || !states || !valid || !counts || !(inlier_threshold > 0)) return VSM_EARG;
  const std::vector<RsRow> rows = rows_of_arrays(n_rows, rows_uv);
  std::vector<int32_t> elig;
  lc_eligible_rows(rows.data(), n_rows, rows_xyz, elig);
  const double limit = rs_limit(inlier_threshold);
  for (int32_t k = 0; k < K; k++)
    counts[k] = valid[k] ? host_count(rows.data(), elig.data(), (int32_t)elig.size(), rows_xyz, states + 12 * (size_t)k, f, cu, cv, min_depth, limit) : 0;
  return VSM_OK;
}

}  // extern "C"
