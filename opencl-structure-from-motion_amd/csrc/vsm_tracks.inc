// Feature tracks from pair match lists (included by vsm_api.cpp; DESIGN.md section 5, INTEGRATION.md).
//
// vsm_pairs_run gives a structure-from-motion driver the match list of every frame pair it asked for; the driver's next
// step is to follow i1p / i1c from list to list until "feature 812 of frame 3 matches feature 790 of frame 4" has become one
// scene point seen in frames 3, 4, 5 and, through a loop-closure pair, 61.  For arbitrary pairs that is the connected
// components of a graph with a node per (frame, feature) and an edge per match; vsm_tracks_run computes them on the
// device (vsm_tracks.hip) from lists in host memory.  The host's part: the pool packs the lists' index pairs into one
// pinned block (8 bytes per match) and finds each frame's node count on the way, one copy takes the block up, one brings
// offsets, observations, flags and the track of every match back.  Segments longer than a workgroup orders are sorted here.
// The blocks are TrkBlocks (vsm_layouts.h), placed in the call's three steps; the call waits twice, so it keeps its own
// sequence of copies and launches and takes the drain, the keep and the timings' close of vsm_stage.h.
struct VsmTracks : VsmResult<8> {  // the staging and the last result's stats and timings (vsm_stage.h)
  std::vector<int32_t> offsets, obs, track_of_match, pair_base;
  std::vector<uint8_t> flags;
  std::vector<int32_t> max_p, max_c;
  std::vector<uint8_t> bad;
  // what vsm_tracks_triangulate needs to find the observations' pixels (vsm_points.inc)
  int32_t n_frames = 0, side = 0;
  bool from_pairs = false;  // the lists were those of vsm_pairs_run (vsm_pairs_tracks)
};

static void tracks_destroy(vsm_handle *h) { vsm_result_destroy(h->tracks); }

static int tracks_run(vsm_handle *h, int32_t n_frames, const int32_t *pairs, int32_t n_pairs, const vsm_p_match *const *lists, const int32_t *counts,
                      int32_t side, int32_t min_length) {
  const double t0 = now_us();
  const int64_t n_edges64 = trk_check_args(n_frames, pairs, n_pairs, lists, counts, side, min_length);
  if (n_edges64 < 0) return VSM_EARG;
  const int32_t n_edges = (int32_t)n_edges64;
  HIPCHK(hipSetDevice(h->device));
  if (!h->tracks) h->tracks = new VsmTracks();
  VsmTracks &T = *h->tracks;
  VsmStage &S = T.st;
  // ---- pack: (ip, ic) of every match, behind the three tables, in one pinned block ----
  TrkBlocks L((size_t)n_pairs, (size_t)n_frames, (size_t)n_edges);
  HIPCHK(S.grow_in(L.in.at, h->stream));
  int32_t *p_pair_base = L.pair_base.host(S), *p_pairs = L.pairs.host(S), *p_feat_base = L.feat_base.host(S), *p_edges = L.edges.host(S);
  T.max_p.assign((size_t)n_pairs, -1);
  T.max_c.assign((size_t)n_pairs, -1);
  T.bad.assign((size_t)n_pairs, 0);
  {
    std::vector<int64_t> start((size_t)n_pairs + 1, 0);
    for (int32_t k = 0; k < n_pairs; k++) start[k + 1] = start[k] + counts[k];
    if (n_pairs > 0) h->pool->run(n_pairs, [&](int k) { T.bad[k] = !trk_pack_list(lists[k], counts[k], side, p_edges + 2 * start[k], &T.max_p[k], &T.max_c[k]); });
  }
  for (int32_t k = 0; k < n_pairs; k++)
    if (T.bad[k]) return VSM_EARG;
  if (!trk_bases(n_frames, pairs, n_pairs, counts, T.max_p.data(), T.max_c.data(), p_feat_base, p_pair_base)) return VSM_EARG;
  if (n_pairs > 0) memcpy(p_pairs, pairs, (size_t)n_pairs * 8);
  const int32_t n_nodes = p_feat_base[n_frames];
  // ---- from here on the call replaces the last result ----
  T.have = false;
  T.n_frames = n_frames;
  T.side = side;
  T.from_pairs = false;
  memset(T.stats, 0, sizeof(T.stats));
  memset(T.timings, 0, sizeof(T.timings));
  T.stats[7] = TRK_SCAN_BLOCK;
  T.pair_base.assign(p_pair_base, p_pair_base + n_pairs + 1);
  T.track_of_match.assign((size_t)n_edges, -1);
  T.offsets.assign(1, 0);
  T.obs.clear();
  T.flags.clear();
  T.t1 = now_us();
  T.timings[0] = T.t1 - t0;
  if (n_edges == 0) {  // no pair with a match: no tracks
    T.have = true;
    return VSM_OK;
  }
  // ---- device memory: the uploaded block, the working set per node, the results (at their upper bounds) ----
  L.nodes((size_t)n_nodes);
  HIPCHK(S.fit_dev(L, h->stream));
  HIPCHK(S.grow_out(8, h->stream, 4096));  // (the totals; the first block is a page)
  const VsmDrain fail{h->stream};          // a call that fails after something was enqueued: drain the device, report
  TrkDevice d;
  memset(&d, 0, sizeof(d));
  d.pair_base = L.pair_base.dev(S);
  d.pairs = L.pairs.dev(S);
  d.feat_base = L.feat_base.dev(S);
  d.edges = L.edges.dev(S);
  d.parent = L.parent.dev(S);
  d.first = L.first.dev(S);
  d.size = L.size.dev(S);
  d.cursor = L.cursor.dev(S);
  d.scan = L.scan.dev(S);
  d.scan_part = L.scan_part.dev(S);
  d.totals = L.totals.dev(S);
  d.mid_list = L.mid_list.dev(S);
  d.counters = L.counters.dev(S, L.out_at);
  d.n_nodes = n_nodes;
  d.n_edges = n_edges;
  d.n_pairs = n_pairs;
  d.n_frames = n_frames;
  d.min_length = min_length;
  VSM_CHK(hipEventRecord(S.ev[0], h->stream));
  VSM_CHK(hipMemcpyAsync(S.dev, S.pin_in, L.in.at, hipMemcpyHostToDevice, h->stream));
  VSM_CHK(hipEventRecord(S.ev[1], h->stream));
  vsm_tracks_launch_link(h->stream, h->prof, d);
  VSM_CHK(hipGetLastError());
  // the totals size the results: the one place where the host waits in the middle of the call
  VSM_CHK(hipMemcpyAsync(S.pin_out, d.totals, 8, hipMemcpyDeviceToHost, h->stream));
  VSM_CHK(hipStreamSynchronize(h->stream));
  const int32_t n_tracks = ((int32_t *)S.pin_out)[0], n_obs = ((int32_t *)S.pin_out)[1];
  if (n_tracks < 0 || n_tracks > n_nodes || n_obs < 0 || n_obs > n_nodes) return fail(VSM_EHIP);  // (cannot be: nothing is sized by it then)
  L.results((size_t)n_tracks, (size_t)n_obs);
  d.offsets = L.offsets.dev(S, L.out_at);
  d.obs = L.obs.dev(S, L.out_at);
  d.track_of_match = L.track_of_match.dev(S, L.out_at);
  d.flags = L.flags.dev(S, L.out_at);
  VSM_CHK(S.grow_out(L.out.at, h->stream));
  vsm_tracks_launch_emit(h->stream, h->prof, d, n_tracks, n_obs);
  VSM_CHK(hipGetLastError());
  VSM_CHK(hipEventRecord(S.ev[2], h->stream));
  VSM_CHK(hipMemcpyAsync(S.pin_out, S.dev + L.out_at, L.out.at, hipMemcpyDeviceToHost, h->stream));
  VSM_CHK(hipStreamSynchronize(h->stream));
  VSM_CHK(hipGetLastError());
  if (h->prof.on) h->prof.resolve();
  // ---- into the handle's vectors; the segments no workgroup took are ordered here ----
  VsmKeep K;
  L.offsets.keep(K, S, T.offsets);
  L.obs.keep(K, S, T.obs);
  L.track_of_match.keep(K, S, T.track_of_match);
  L.flags.keep(K, S, T.flags);
  int64_t by_host = 0, inconsistent = 0;
  for (int32_t t = 0; t < n_tracks; t++) {
    const int32_t len = T.offsets[t + 1] - T.offsets[t];
    if (len > VSM_TRACKS_BLOCK_MAX) {
      T.flags[t] = (uint8_t)trk_sort_segment(T.obs.data() + 4 * (size_t)T.offsets[t], len);
      by_host++;
    }
    inconsistent += T.flags[t] & 1;
  }
  const int64_t by_block = L.counters.host(S)[0];
  T.stats[0] = n_nodes;
  T.stats[1] = n_edges;
  T.stats[2] = n_tracks;
  T.stats[3] = inconsistent;
  T.stats[4] = n_tracks - by_block - by_host;
  T.stats[5] = by_block;
  T.stats[6] = by_host;
  S.elapsed();
  T.close();
  return VSM_OK;
}

static const VsmTracks *tracks_result(vsm_handle *h) { return (h && h->tracks && h->tracks->have) ? h->tracks : nullptr; }

extern "C" {

int vsm_tracks_run(vsm_handle *h, int32_t n_frames, const int32_t *pairs, int32_t n_pairs, const vsm_p_match *const *lists, const int32_t *counts,
                   int32_t side, int32_t min_length) {
  if (!h) return VSM_EARG;
  return tracks_run(h, n_frames, pairs, n_pairs, lists, counts, side, min_length);
}

int vsm_pairs_tracks(vsm_handle *h, int32_t side, int32_t min_length) {
  if (!h) return VSM_EARG;
  std::vector<const vsm_p_match *> lists;
  std::vector<int32_t> counts;
  const VsmPairs *P = pairs_last_lists(h, lists, counts);
  if (!P) return VSM_ENOTREADY;
  if (P->method == 1) return VSM_EARG;  // (stereo-only lists: tracks across time are not defined)
  const int rc = tracks_run(h, P->n_frames, P->pair_list.data(), (int32_t)lists.size(), lists.data(), counts.data(), side, min_length);
  if (rc == VSM_OK) h->tracks->from_pairs = true;
  return rc;
}

int32_t vsm_tracks_count(vsm_handle *h) { return (h && h->tracks && h->tracks->have) ? (int32_t)h->tracks->flags.size() : 0; }
int32_t vsm_tracks_num_obs(vsm_handle *h) { return (h && h->tracks && h->tracks->have) ? (int32_t)(h->tracks->obs.size() / 4) : 0; }
int32_t vsm_tracks_get(vsm_handle *h, int32_t *offsets, int32_t *obs, uint8_t *flags) {
  if (!h || !h->tracks || !h->tracks->have) return 0;
  const VsmTracks &T = *h->tracks;
  if (offsets) memcpy(offsets, T.offsets.data(), T.offsets.size() * 4);
  if (obs && !T.obs.empty()) memcpy(obs, T.obs.data(), T.obs.size() * 4);
  if (flags && !T.flags.empty()) memcpy(flags, T.flags.data(), T.flags.size());
  return (int32_t)T.flags.size();
}
int32_t vsm_tracks_of_matches(vsm_handle *h, int32_t pair, int32_t *out, int32_t cap) {
  if (!h || !h->tracks || !h->tracks->have) return 0;
  const VsmTracks &T = *h->tracks;
  if (pair < 0 || pair + 1 >= (int32_t)T.pair_base.size()) return 0;
  const int32_t n = T.pair_base[pair + 1] - T.pair_base[pair];
  const int32_t m = std::min(n, cap);
  if (out && m > 0) memcpy(out, T.track_of_match.data() + T.pair_base[pair], (size_t)m * 4);
  return n;
}
void vsm_tracks_get_stats(vsm_handle *h, int64_t *out8) { vsm_result_get(tracks_result(h), &VsmTracks::stats, out8); }
void vsm_tracks_get_timings(vsm_handle *h, double *out4) { vsm_result_get(tracks_result(h), &VsmTracks::timings, out4); }

}  // extern "C"
