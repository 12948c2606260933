// Feature tracks, the host side without HIP: the argument checks and the packing the device path starts with, the ordering
// of the segments too long for a workgroup, and vsm_host_tracks - a plain sequential union-find over the same definition
// (vsm_tracks.h).  The host view is the CPU suite's subject and the device path's second opinion, never its fallback.
#include "vsm_tracks.h"

#include <algorithm>
#include <vector>

int64_t trk_check_args(int32_t n_frames, const int32_t *pairs, int32_t n_pairs, const vsm_p_match *const *lists, const int32_t *counts, int32_t side,
                       int32_t min_length) {
  if (side < 0 || side > 1 || min_length < 1 || n_frames < 0 || n_pairs < 0) return -1;
  if (n_pairs > 0 && (!pairs || !counts || !lists)) return -1;
  int64_t edges = 0;
  for (int32_t k = 0; k < n_pairs; k++) {
    const int32_t a = pairs[2 * k], b = pairs[2 * k + 1];
    if (a < 0 || a >= n_frames || b < 0 || b >= n_frames) return -1;  // (a previous frame of -1: a stereo-only list)
    if (counts[k] < 0 || (counts[k] > 0 && !lists[k])) return -1;
    edges += counts[k];
  }
  return edges <= TRK_MAX_EDGES ? edges : -1;
}

bool trk_pack_list(const vsm_p_match *list, int32_t n, int32_t side, int32_t *edges, int32_t *max_p, int32_t *max_c) {
  int32_t mp = -1, mc = -1, low = 0;
  for (int32_t m = 0; m < n; m++) {
    const int32_t ip = side ? list[m].i2p : list[m].i1p, ic = side ? list[m].i2c : list[m].i1c;
    edges[2 * m] = ip;
    edges[2 * m + 1] = ic;
    mp = std::max(mp, ip);
    mc = std::max(mc, ic);
    low = std::min(low, std::min(ip, ic));
  }
  *max_p = mp;
  *max_c = mc;
  return low >= 0;
}

bool trk_bases(int32_t n_frames, const int32_t *pairs, int32_t n_pairs, const int32_t *counts, const int32_t *max_p, const int32_t *max_c, int32_t *feat_base,
               int32_t *pair_base) {
  // a frame's node count, 1 + the largest index seen, is kept in feat_base[frame + 1] until the prefix sum
  std::fill(feat_base, feat_base + n_frames + 1, 0);
  pair_base[0] = 0;
  for (int32_t k = 0; k < n_pairs; k++) {
    pair_base[k + 1] = pair_base[k] + counts[k];
    if (counts[k] == 0) continue;
    int32_t &na = feat_base[pairs[2 * k] + 1], &nb = feat_base[pairs[2 * k + 1] + 1];
    if (max_p[k] == TRK_UNUSED || max_c[k] == TRK_UNUSED) return false;  // (1 + index does not fit)
    na = std::max(na, max_p[k] + 1);
    nb = std::max(nb, max_c[k] + 1);
  }
  int64_t total = 0;
  for (int32_t f = 0; f < n_frames; f++) {
    total += feat_base[f + 1];
    if (total > TRK_MAX_NODES) return false;
    feat_base[f + 1] = (int32_t)total;
  }
  return true;
}

int trk_sort_segment(int32_t *rows, int32_t n) {
  struct Row {
    int32_t frame, feature, pair, code;
  };
  Row *r = (Row *)rows;
  std::sort(r, r + n, [](const Row &a, const Row &b) { return a.frame != b.frame ? a.frame < b.frame : a.feature < b.feature; });
  for (int32_t i = 1; i < n; i++)
    if (r[i].frame == r[i - 1].frame) return 1;
  return 0;
}

extern "C" int32_t vsm_host_tracks(int32_t n_frames, const int32_t *pairs, int32_t n_pairs, const vsm_p_match *const *lists, const int32_t *counts,
                                   int32_t side, int32_t min_length, int32_t *offsets, int32_t *obs, uint8_t *flags, int32_t *track_of_match,
                                   int32_t *n_obs_out) {
  const int64_t n_edges = trk_check_args(n_frames, pairs, n_pairs, lists, counts, side, min_length);
  if (n_edges < 0) return VSM_EARG;
  // everything is worked out in vectors of its own first: an argument error leaves the caller's arrays untouched
  std::vector<int32_t> edges((size_t)n_edges * 2), max_p((size_t)n_pairs), max_c((size_t)n_pairs), feat_base((size_t)n_frames + 1), pair_base((size_t)n_pairs + 1);
  {
    int64_t at = 0;
    for (int32_t k = 0; k < n_pairs; k++) {
      if (!trk_pack_list(lists[k], counts[k], side, edges.data() + 2 * at, &max_p[k], &max_c[k])) return VSM_EARG;
      at += counts[k];
    }
  }
  if (!trk_bases(n_frames, pairs, n_pairs, counts, max_p.data(), max_c.data(), feat_base.data(), pair_base.data())) return VSM_EARG;
  const int32_t n_nodes = feat_base[n_frames];
  // sequential union-find: full path compression, the smaller root on top
  std::vector<int32_t> parent((size_t)n_nodes), first((size_t)n_nodes, TRK_UNUSED);
  for (int32_t v = 0; v < n_nodes; v++) parent[v] = v;
  auto find = [&](int32_t x) {
    int32_t r = x;
    while (parent[r] != r) r = parent[r];
    while (parent[x] != r) {
      const int32_t up = parent[x];
      parent[x] = r;
      x = up;
    }
    return r;
  };
  for (int32_t k = 0, e = 0; k < n_pairs; k++)
    for (int32_t m = 0; m < counts[k]; m++, e++) {
      const int32_t u = feat_base[pairs[2 * k]] + edges[2 * (size_t)e], v = feat_base[pairs[2 * k + 1]] + edges[2 * (size_t)e + 1];
      first[u] = std::min(first[u], 2 * e);
      first[v] = std::min(first[v], 2 * e + 1);
      const int32_t ru = find(u), rv = find(v);
      if (ru != rv) parent[std::max(ru, rv)] = std::min(ru, rv);
    }
  // sizes, kept roots in ascending order, offsets
  std::vector<int32_t> size((size_t)n_nodes, 0), track((size_t)n_nodes, -1);
  for (int32_t v = 0; v < n_nodes; v++)
    if (first[v] != TRK_UNUSED) size[find(v)]++;
  int32_t n_tracks = 0, n_obs = 0;
  for (int32_t v = 0; v < n_nodes; v++)
    if (parent[v] == v && size[v] >= min_length) {  // (a node no match names has size 0)
      track[v] = n_tracks++;
      n_obs += size[v];
    }
  if (n_obs_out) *n_obs_out = n_obs;
  if (offsets) {
    int32_t at = 0;
    for (int32_t v = 0; v < n_nodes; v++)
      if (track[v] >= 0) {
        offsets[track[v]] = at;
        at += size[v];
      }
    offsets[n_tracks] = at;
  }
  if (obs || flags) {
    // the nodes in ascending order fall into their segments in ascending order
    std::vector<int32_t> cursor((size_t)n_tracks + 1, 0), last_frame((size_t)n_tracks, -1);
    {
      int32_t at = 0;
      for (int32_t v = 0; v < n_nodes; v++)
        if (track[v] >= 0) {
          cursor[track[v]] = at;
          at += size[v];
        }
    }
    if (flags) std::fill(flags, flags + n_tracks, 0);
    int32_t frame = 0;
    for (int32_t v = 0; v < n_nodes; v++) {
      while (v >= feat_base[frame + 1]) frame++;
      if (first[v] == TRK_UNUSED) continue;
      const int32_t t = track[parent[v]];  // (find(v) above left parent[v] at the root)
      if (t < 0) continue;
      if (flags && last_frame[t] == frame) flags[t] |= 1;
      last_frame[t] = frame;
      if (obs) {
        const int32_t e = first[v] >> 1, end = first[v] & 1;
        const int32_t k = trk_owner(pair_base.data(), n_pairs, e);
        int32_t *row = obs + 4 * (size_t)cursor[t]++;
        row[0] = frame;
        row[1] = v - feat_base[frame];
        row[2] = k;
        row[3] = 2 * (e - pair_base[k]) + end;
      }
    }
  }
  if (track_of_match)
    for (int32_t k = 0, e = 0; k < n_pairs; k++)
      for (int32_t m = 0; m < counts[k]; m++, e++) track_of_match[e] = track[parent[feat_base[pairs[2 * k]] + edges[2 * (size_t)e]]];
  return n_tracks;
}
