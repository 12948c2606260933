// Re-observation, the host side without HIP: the default parameters, the argument checks of both forms and
// vsm_host_reobserve - one host thread walking the functions of vsm_reobserve.h.  Its index is a list per frame of the free
// features ordered by (class, v): a window's rows are a run of it, found by bisection, and ro_in_window is the test, as on
// the device.  The host view is the CPU suite's subject and the device path's second opinion, never its fallback.
#include "vsm_reobserve.h"

#include <string.h>

#include <algorithm>
#include <vector>

int64_t ro_check_tracks(const vsm_reobserve_params *params, int32_t n_frames, const double *poses, int32_t width, int32_t height, int32_t n_tracks,
                        const int32_t *offsets, const int32_t *obs_frames, const int32_t *obs_feat, const double *xyz, const int32_t *ref_obs,
                        const int32_t *feat_offsets) {
  if (!ro_params_ok(params) || !ro_dims_ok(width, height) || n_frames < 0 || n_tracks < 0) return -1;
  if (n_frames > 0 && !poses) return -1;
  if (n_tracks == 0) return 0;
  if (!offsets || offsets[0] != 0 || !xyz) return -1;
  for (int32_t t = 0; t < n_tracks; t++)
    if (offsets[t + 1] < offsets[t]) return -1;
  const int64_t n_obs = offsets[n_tracks];
  if (n_obs > 0 && (!obs_frames || !obs_feat)) return -1;
  for (int64_t i = 0; i < n_obs; i++) {
    const int32_t g = obs_frames[i];
    if (g < 0 || g >= n_frames || obs_feat[i] < 0 || obs_feat[i] >= feat_offsets[g + 1] - feat_offsets[g]) return -1;
  }
  if (ref_obs)
    for (int32_t t = 0; t < n_tracks; t++) {
      const int32_t n = offsets[t + 1] - offsets[t];
      if (n > 0 && (ref_obs[t] < 0 || ref_obs[t] >= n)) return -1;  // (a track without observations has no reference, and no candidates)
    }
  return n_obs;
}

int64_t ro_check_features(int32_t n_frames, int32_t width, int32_t height, const int32_t *feat_offsets, const int32_t *feat) {
  if (n_frames < 0 || !ro_dims_ok(width, height)) return -1;
  if (n_frames == 0) return 0;
  if (!feat_offsets || feat_offsets[0] != 0) return -1;
  for (int32_t g = 0; g < n_frames; g++)
    if (feat_offsets[g + 1] < feat_offsets[g]) return -1;
  const int64_t n_feat = feat_offsets[n_frames];
  if (n_feat > 0 && !feat) return -1;
  for (int64_t j = 0; j < n_feat; j++) {
    const int32_t *r = feat + RO_FEAT_INTS * j;
    if (r[0] < 0 || r[0] >= width || r[1] < 0 || r[1] >= height || r[3] < 0 || r[3] > 3) return -1;
  }
  return n_feat;
}

int64_t ro_candidate_bound(int32_t n_frames, const uint8_t *pose_valid, const uint8_t *search, int32_t n_tracks, const int32_t *offsets, const uint8_t *use) {
  int64_t frames = 0, tracks = 0;
  for (int32_t g = 0; g < n_frames; g++) frames += ((!pose_valid || pose_valid[g]) && (!search || search[g])) ? 1 : 0;
  for (int32_t t = 0; t < n_tracks; t++) tracks += ((!use || use[t]) && offsets[t + 1] > offsets[t]) ? 1 : 0;
  return frames * tracks;
}

extern "C" {

void vsm_reobserve_default_params(vsm_reobserve_params *p) {
  if (!p) return;
  p->radius = 4.0;
  p->min_depth = 1e-10;
  p->max_cost = 0;
  p->ratio_num = 0;
  p->ratio_den = 0;
}

int32_t vsm_host_reobserve(int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *search, double f, double cu, double cv, int32_t width,
                           int32_t height, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const int32_t *obs_feat, const double *xyz,
                           const uint8_t *use, const int32_t *ref_obs, const int32_t *feat_offsets, const int32_t *feat, const vsm_reobserve_params *params,
                           int32_t cap, int32_t *cand, double *cand_uv, int32_t *track_accepted, int32_t *frame_counts, int64_t *stats10) {
  const int64_t n_feat = ro_check_features(n_frames, width, height, feat_offsets, feat);
  if (n_feat < 0) return VSM_EARG;
  const int64_t n_obs = ro_check_tracks(params, n_frames, poses, width, height, n_tracks, offsets, obs_frames, obs_feat, xyz, ref_obs, feat_offsets);
  if (n_obs < 0 || cap < 0) return VSM_EARG;
  if (n_tracks > 0 && ro_candidate_bound(n_frames, pose_valid, search, n_tracks, offsets, use) > 0x7fffffff) return VSM_EARG;
  const vsm_reobserve_params &prm = *params;
  const size_t F = (size_t)n_frames, T = (size_t)n_tracks;
  std::vector<double> states(F * 12 + 1);
  for (size_t g = 0; g < F; g++) pts_rigid_inverse(poses + 12 * g, states.data() + 12 * g);
  // ---- occupied features; per frame the free ones by (class, v) ----
  std::vector<uint8_t> occupied((size_t)n_feat + 1, 0);
  for (int64_t i = 0; i < n_obs; i++) occupied[(size_t)feat_offsets[obs_frames[i]] + obs_feat[i]] = 1;
  std::vector<int32_t> order;  // feature indices within their frames, frame after frame at feat_offsets
  order.reserve((size_t)n_feat + 1);
  std::vector<int32_t> free_off(F + 1, 0);
  for (size_t g = 0; g < F; g++) {
    const int32_t *rec = feat + RO_FEAT_INTS * (size_t)feat_offsets[g];
    const size_t a = order.size();
    for (int32_t k = 0; k < feat_offsets[g + 1] - feat_offsets[g]; k++)
      if (!occupied[(size_t)feat_offsets[g] + k]) order.push_back(k);
    std::sort(order.begin() + a, order.end(), [rec](int32_t x, int32_t y) {
      const int32_t *p = rec + RO_FEAT_INTS * (size_t)x, *q = rec + RO_FEAT_INTS * (size_t)y;
      return p[3] != q[3] ? p[3] < q[3] : (p[1] != q[1] ? p[1] < q[1] : x < y);
    });
    free_off[g + 1] = (int32_t)order.size();
  }
  // ---- the candidates, in (track, frame) order, each with its window ----
  struct Cand {
    int32_t r[RO_CAND_INTS];
    double pu, pv;
  };
  std::vector<Cand> list;
  std::vector<uint64_t> claim((size_t)n_feat + 1, RO_NO_KEY);
  std::vector<int32_t> fc(2 * F + 1, 0), ta(T + 1, 0);
  int64_t stats[RO_STATS];
  memset(stats, 0, sizeof(stats));
  for (int32_t t = 0; t < n_tracks; t++) {
    const int32_t o = offsets[t], n = offsets[t + 1] - o;
    if (!((!use || use[t]) && n > 0)) continue;
    const int32_t ref = o + (ref_obs ? ref_obs[t] : ro_middle(n));
    const int32_t *ref_rec = feat + RO_FEAT_INTS * ((size_t)feat_offsets[obs_frames[ref]] + obs_feat[ref]);
    const int32_t cls = ref_rec[3];
    for (int32_t g = 0; g < n_frames; g++) {
      Cand c;
      const int32_t kind = ro_pair(!search || search[g], !pose_valid || pose_valid[g], obs_frames + o, n, g, states.data() + 12 * (size_t)g, xyz + 3 * (size_t)t, f, cu,
                                   cv, prm.min_depth, width, height, &c.pu, &c.pv);
      if (kind != RO_CANDIDATE) {
        stats[kind]++;
        continue;
      }
      const int32_t *rec = feat + RO_FEAT_INTS * (size_t)feat_offsets[g];
      const int32_t *lo = order.data() + free_off[g], *hi = order.data() + free_off[g + 1];
      // the run of class cls from the first row that can reach the window: v >= pv - radius - 1
      const double v_min = c.pv - prm.radius - 1.0;
      const int32_t *it = std::partition_point(lo, hi, [&](int32_t k) {
        const int32_t *p = rec + RO_FEAT_INTS * (size_t)k;
        return p[3] < cls || (p[3] == cls && (double)p[1] < v_min);
      });
      RoBest best;
      ro_best_init(&best);
      for (; it != hi; ++it) {
        const int32_t *p = rec + RO_FEAT_INTS * (size_t)*it;
        if (p[3] != cls || (double)p[1] > c.pv + prm.radius + 1.0) break;
        if (ro_in_window(p[0], p[1], c.pu, c.pv, prm.radius)) ro_best_add(&best, ro_sad((const uint32_t *)ref_rec + 4, (const uint32_t *)p + 4), *it);
      }
      const int32_t code = ro_window_code(best, prm);
      c.r[0] = t;
      c.r[1] = g;
      ro_record(c.r, best, code);
      if (code == RO_ACCEPTED) {
        uint64_t &w = claim[(size_t)feat_offsets[g] + c.r[2]];
        const uint64_t key = (best.key & 0xffffffff00000000ull) | (uint32_t)list.size();
        w = key < w ? key : w;
      }
      fc[2 * (size_t)g]++;
      list.push_back(c);
    }
  }
  // ---- the verdicts ----
  for (size_t i = 0; i < list.size(); i++) {
    int32_t *r = list[i].r;
    if (r[6] == RO_ACCEPTED) {
      if ((uint32_t)claim[(size_t)feat_offsets[r[1]] + r[2]] != (uint32_t)i) {
        r[6] = RO_LOST;
      } else {
        ta[r[0]]++;
        fc[2 * (size_t)r[1] + 1]++;
      }
    }
    stats[RO_REASONS + r[6]]++;
  }
  const size_t n_out = std::min(list.size(), (size_t)cap);
  for (size_t i = 0; i < n_out; i++) {
    if (cand) memcpy(cand + RO_CAND_INTS * i, list[i].r, sizeof(list[i].r));
    if (cand_uv) cand_uv[2 * i] = list[i].pu, cand_uv[2 * i + 1] = list[i].pv;
  }
  if (track_accepted && T > 0) memcpy(track_accepted, ta.data(), T * 4);
  if (frame_counts && F > 0) memcpy(frame_counts, fc.data(), F * 8);
  if (stats10) memcpy(stats10, stats, sizeof(stats));
  return (int32_t)list.size();
}

}  // extern "C"
