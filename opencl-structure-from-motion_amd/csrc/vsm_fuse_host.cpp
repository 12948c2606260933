// Fusion, the host side without HIP: the default parameters and vsm_host_fuse - one host thread walking the functions of
// vsm_fuse.h and vsm_reobserve.h.  Its index is a list per frame of the owned features ordered by (class, v): a window's
// rows are a run of it, found by bisection, and ro_in_window is the test, as on the device.  The merged set comes from a
// stable sort of the two tracks' observations, where the device ranks them (fu_rank): two ways to the one order.  The
// argument checks are the re-observation's (vsm_reobserve_host.cpp).  The host view is the CPU suite's subject and the
// device path's second opinion, never its fallback.
#include "vsm_fuse.h"

#include <string.h>

#include <algorithm>
#include <vector>

extern "C" {

void vsm_fuse_default_params(vsm_fuse_params *p) {
  if (!p) return;
  p->radius = 4.0;
  p->min_depth = 1e-10;
  p->max_cost = 0;
  p->ratio_num = 0;
  p->ratio_den = 0;
}

int32_t vsm_host_fuse(int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *search, double f, double cu, double cv, int32_t width,
                      int32_t height, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const int32_t *obs_feat, const double *xyz,
                      const uint8_t *use, const int32_t *ref_obs, const int32_t *feat_offsets, const int32_t *feat, const vsm_fuse_params *params, int32_t cap,
                      int32_t *prop, double *prop_uv, int32_t *partner, int32_t *fused_into, int32_t *offsets_after, int32_t *obs_src, int32_t *frame_counts,
                      int64_t *stats13) {
  if (!fu_params_ok(params)) return VSM_EARG;
  const vsm_reobserve_params prm = fu_as_reobserve(*params);
  const int64_t n_feat = ro_check_features(n_frames, width, height, feat_offsets, feat);
  if (n_feat < 0) return VSM_EARG;
  const int64_t n_obs = ro_check_tracks(&prm, n_frames, poses, width, height, n_tracks, offsets, obs_frames, obs_feat, xyz, ref_obs, feat_offsets);
  if (n_obs < 0 || cap < 0) return VSM_EARG;
  if (n_tracks > 0 && ro_candidate_bound(n_frames, pose_valid, search, n_tracks, offsets, use) > 0x7fffffff) return VSM_EARG;
  const size_t F = (size_t)n_frames, T = (size_t)n_tracks;
  auto in_use = [&](int32_t t) { return (!use || use[t]) && offsets[t + 1] > offsets[t]; };
  std::vector<double> states(F * 12 + 1);
  for (size_t g = 0; g < F; g++) pts_rigid_inverse(poses + 12 * g, states.data() + 12 * g);
  // ---- owners; per frame the owned features by (class, v) ----
  std::vector<uint32_t> owner((size_t)n_feat + 1, FU_NO_OWNER);
  for (int32_t t = 0; t < n_tracks; t++)
    if (in_use(t))
      for (int32_t i = offsets[t]; i < offsets[t + 1]; i++) {
        uint32_t &w = owner[(size_t)feat_offsets[obs_frames[i]] + obs_feat[i]];
        w = (uint32_t)t < w ? (uint32_t)t : w;
      }
  std::vector<int32_t> order;  // feature indices within their frames, frame after frame
  order.reserve((size_t)n_feat + 1);
  std::vector<int32_t> own_off(F + 1, 0);
  for (size_t g = 0; g < F; g++) {
    const int32_t *rec = feat + RO_FEAT_INTS * (size_t)feat_offsets[g];
    const size_t a = order.size();
    for (int32_t k = 0; k < feat_offsets[g + 1] - feat_offsets[g]; k++)
      if (owner[(size_t)feat_offsets[g] + k] != FU_NO_OWNER) order.push_back(k);
    std::sort(order.begin() + a, order.end(), [rec](int32_t x, int32_t y) {
      const int32_t *p = rec + RO_FEAT_INTS * (size_t)x, *q = rec + RO_FEAT_INTS * (size_t)y;
      return p[3] != q[3] ? p[3] < q[3] : (p[1] != q[1] ? p[1] < q[1] : x < y);
    });
    own_off[g + 1] = (int32_t)order.size();
  }
  // ---- the proposals, in (track, frame) order ----
  std::vector<int32_t> list;  // eight words each
  std::vector<double> uv;
  std::vector<int32_t> fc(2 * F + 1, 0);
  int64_t stats[FU_STATS];
  memset(stats, 0, sizeof(stats));
  for (int32_t t = 0; t < n_tracks; t++) {
    if (!in_use(t)) continue;
    const int32_t o = offsets[t], n = offsets[t + 1] - o;
    const int32_t ref = o + (ref_obs ? ref_obs[t] : ro_middle(n));
    const int32_t *ref_rec = feat + RO_FEAT_INTS * ((size_t)feat_offsets[obs_frames[ref]] + obs_feat[ref]);
    const int32_t cls = ref_rec[3];
    for (int32_t g = 0; g < n_frames; g++) {
      double pu, pv;
      const int32_t kind = ro_pair(!search || search[g], !pose_valid || pose_valid[g], obs_frames + o, n, g, states.data() + 12 * (size_t)g, xyz + 3 * (size_t)t, f, cu, cv,
                                   prm.min_depth, width, height, &pu, &pv);
      if (kind != RO_CANDIDATE) {
        stats[kind]++;
        continue;
      }
      fc[2 * (size_t)g]++;
      const int32_t *rec = feat + RO_FEAT_INTS * (size_t)feat_offsets[g];
      const int32_t *lo = order.data() + own_off[g], *hi = order.data() + own_off[g + 1];
      // the run of class cls from the first row that can reach the window: v >= pv - radius - 1
      const double v_min = pv - prm.radius - 1.0;
      const int32_t *it = std::partition_point(lo, hi, [&](int32_t k) {
        const int32_t *p = rec + RO_FEAT_INTS * (size_t)k;
        return p[3] < cls || (p[3] == cls && (double)p[1] < v_min);
      });
      RoBest best;
      ro_best_init(&best);
      for (; it != hi; ++it) {
        const int32_t *p = rec + RO_FEAT_INTS * (size_t)*it;
        if (p[3] != cls || (double)p[1] > pv + prm.radius + 1.0) break;
        if (ro_in_window(p[0], p[1], pu, pv, prm.radius)) ro_best_add(&best, ro_sad((const uint32_t *)ref_rec + 4, (const uint32_t *)p + 4), *it);
      }
      if (best.n == 0) {
        stats[RO_REASONS + FU_EMPTY]++;
        continue;
      }
      int32_t r[FU_PROP_INTS] = {t, g, 0, 0, 0, 0, 0, 0};
      ro_record(r, best, ro_window_code(best, prm));
      r[7] = (int32_t)owner[(size_t)feat_offsets[g] + r[2]];
      list.insert(list.end(), r, r + FU_PROP_INTS);
      uv.push_back(pu), uv.push_back(pv);
      fc[2 * (size_t)g + 1]++;
    }
  }
  const int32_t n_prop = (int32_t)(list.size() / FU_PROP_INTS);
  // ---- conflicts and bids, then the verdicts ----
  std::vector<unsigned long long> choice(T + 1, FU_NO_CHOICE);
  for (int32_t p = 0; p < n_prop; p++) {
    int32_t *r = list.data() + FU_PROP_INTS * (size_t)p;
    if (r[6] != FU_FUSED) continue;
    const int32_t a = r[0], b = r[7];
    if (fu_conflict(obs_frames + offsets[a], offsets[a + 1] - offsets[a], obs_frames + offsets[b], offsets[b + 1] - offsets[b], 0, 1)) {
      r[6] = FU_CONFLICT;
    } else {
      const unsigned long long bid = fu_bid(r[3], p);
      choice[a] = bid < choice[a] ? bid : choice[a];
    }
  }
  std::vector<int32_t> pa(T + 1, -1), fi(T + 1, -1);
  for (int32_t p = 0; p < n_prop; p++) {
    int32_t *r = list.data() + FU_PROP_INTS * (size_t)p;
    if (r[6] == FU_FUSED) {
      r[6] = fu_verdict(list.data(), choice.data(), p);
      if (r[6] != FU_OUTBID) pa[r[0]] = r[7];
      if (r[6] == FU_FUSED) {
        if (r[0] > r[7])
          fi[r[0]] = r[7];
        else
          stats[FU_STAT_FUSIONS]++;
      }
    }
    stats[RO_REASONS + r[6]]++;
  }
  // ---- the merged set ----
  if (offsets_after || obs_src) {
    std::vector<int32_t> both;
    int32_t at = 0;
    for (int32_t t = 0; t < n_tracks; t++) {
      if (offsets_after) offsets_after[t] = at;
      if (fi[t] >= 0) continue;
      const int32_t o = offsets[t], n = offsets[t + 1] - o;
      both.clear();
      for (int32_t i = 0; i < n; i++) both.push_back(o + i);
      if (fu_survivor(pa.data(), fi.data(), t)) {
        for (int32_t i = offsets[pa[t]]; i < offsets[pa[t] + 1]; i++) both.push_back(i);
        std::stable_sort(both.begin(), both.end(), [&](int32_t x, int32_t y) { return obs_frames[x] < obs_frames[y]; });
      }
      if (obs_src)
        for (size_t i = 0; i < both.size(); i++) obs_src[(size_t)at + i] = both[i];
      at += (int32_t)both.size();
    }
    if (offsets_after) offsets_after[T] = at;
  }
  const size_t n_out = std::min((size_t)n_prop, (size_t)cap);
  if (prop && n_out > 0) memcpy(prop, list.data(), n_out * FU_PROP_INTS * 4);
  if (prop_uv && n_out > 0) memcpy(prop_uv, uv.data(), n_out * 16);
  if (partner && T > 0) memcpy(partner, pa.data(), T * 4);
  if (fused_into && T > 0) memcpy(fused_into, fi.data(), T * 4);
  if (frame_counts && F > 0) memcpy(frame_counts, fc.data(), F * 8);
  if (stats13) memcpy(stats13, stats, sizeof(stats));
  return n_prop;
}

}  // extern "C"
