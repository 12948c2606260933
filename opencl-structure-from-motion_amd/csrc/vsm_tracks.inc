// Feature tracks from pair match lists (included by vsm_api.cpp; DESIGN.md section 5, INTEGRATION.md).
//
// vsm_pairs_run gives a structure-from-motion driver the match list of every frame pair it asked for; the driver's next
// step is to follow i1p / i1c from list to list until "feature 812 of frame 3 matches feature 790 of frame 4" has become one
// scene point seen in frames 3, 4, 5 and, through a loop-closure pair, 61.  For arbitrary pairs that is the connected
// components of a graph with a node per (frame, feature) and an edge per match; vsm_tracks_run computes them on the
// device (vsm_tracks.hip) from lists in host memory.  The host's part: the pool packs the lists' index pairs into one
// pinned block (8 bytes per match) and finds each frame's node count on the way, one copy takes the block up, one brings
// offsets, observations, flags and the track of every match back.  Segments longer than a workgroup orders are sorted here.
struct VsmTracks {
  VsmStage st;  // pinned input and output, the device block, the events (vsm_stage.h)
  bool have = false;
  std::vector<int32_t> offsets, obs, track_of_match, pair_base;
  std::vector<uint8_t> flags;
  int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double timings[4] = {0, 0, 0, 0};
  std::vector<int32_t> max_p, max_c;
  std::vector<uint8_t> bad;
  // what vsm_tracks_triangulate needs to find the observations' pixels (vsm_points.inc)
  int32_t n_frames = 0, side = 0;
  bool from_pairs = false;  // the lists were those of vsm_pairs_run (vsm_pairs_tracks)
};

static void tracks_destroy(vsm_handle *h) {
  VsmTracks *T = h->tracks;
  if (!T) return;
  T->st.release();
  delete T;
  h->tracks = nullptr;
}

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
  VsmLayout in;
  const size_t o_pair_base = in.take(((size_t)n_pairs + 1) * 4), o_pairs = in.take((size_t)n_pairs * 8 + 4), o_feat_base = in.take(((size_t)n_frames + 1) * 4),
               o_edges = in.take((size_t)n_edges * 8 + 4);
  HIPCHK(S.grow_in(in.at, h->stream));
  int32_t *p_pair_base = (int32_t *)(S.pin_in + o_pair_base), *p_pairs = (int32_t *)(S.pin_in + o_pairs), *p_feat_base = (int32_t *)(S.pin_in + o_feat_base),
          *p_edges = (int32_t *)(S.pin_in + o_edges);
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
  const double t1 = now_us();
  T.timings[0] = t1 - t0;
  if (n_edges == 0) {  // no pair with a match: no tracks
    T.have = true;
    return VSM_OK;
  }
  // ---- device memory: the uploaded block, the working set per node, the results (at their upper bounds) ----
  const size_t scan_part_items = trk_scan_part_items(n_nodes);
  VsmLayout dl = in;
  const size_t N = (size_t)n_nodes;
  const size_t o_parent = dl.take(N * 4), o_first = dl.take(N * 4), o_size = dl.take(N * 4), o_cursor = dl.take(N * 4), o_scan = dl.take(N * 8),
               o_part = dl.take(scan_part_items * 8 + 8), o_totals = dl.take(8), o_mid = dl.take((N / (VSM_TRACKS_WAVE_MAX + 1) + 1) * 4), o_out = dl.take(0);
  // the results' upper bounds: every node an observation, every node a track
  const size_t out_cap = al256(16) + al256((N + 1) * 4) + al256(N * 16) + al256((size_t)n_edges * 4) + al256(N);
  HIPCHK(S.grow_dev(o_out + out_cap, h->stream));
  HIPCHK(S.events());
  HIPCHK(S.grow_out(8, h->stream, 4096));  // (the totals; the first block is a page)
  // a call that fails after something was enqueued: drain the device, report
  auto fail = [&](int rc) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipGetLastError();
    return rc;
  };
  TrkDevice d;
  memset(&d, 0, sizeof(d));
  d.pair_base = (const int32_t *)(S.dev + o_pair_base);
  d.pairs = (const int32_t *)(S.dev + o_pairs);
  d.feat_base = (const int32_t *)(S.dev + o_feat_base);
  d.edges = (const int32_t *)(S.dev + o_edges);
  d.parent = (int32_t *)(S.dev + o_parent);
  d.first = (int32_t *)(S.dev + o_first);
  d.size = (int32_t *)(S.dev + o_size);
  d.cursor = (int32_t *)(S.dev + o_cursor);
  d.scan = (int32_t *)(S.dev + o_scan);
  d.scan_part = (int32_t *)(S.dev + o_part);
  d.totals = (int32_t *)(S.dev + o_totals);
  d.mid_list = (int32_t *)(S.dev + o_mid);
  d.counters = (int32_t *)(S.dev + o_out);
  d.n_nodes = n_nodes;
  d.n_edges = n_edges;
  d.n_pairs = n_pairs;
  d.n_frames = n_frames;
  d.min_length = min_length;
  VSM_CHK(hipEventRecord(S.ev[0], h->stream));
  VSM_CHK(hipMemcpyAsync(S.dev, S.pin_in, in.at, hipMemcpyHostToDevice, h->stream));
  VSM_CHK(hipEventRecord(S.ev[1], h->stream));
  vsm_tracks_launch_link(h->stream, h->prof, d);
  VSM_CHK(hipGetLastError());
  // the totals size the results: the one place where the host waits in the middle of the call
  VSM_CHK(hipMemcpyAsync(S.pin_out, d.totals, 8, hipMemcpyDeviceToHost, h->stream));
  VSM_CHK(hipStreamSynchronize(h->stream));
  const int32_t n_tracks = ((int32_t *)S.pin_out)[0], n_obs = ((int32_t *)S.pin_out)[1];
  if (n_tracks < 0 || n_tracks > n_nodes || n_obs < 0 || n_obs > n_nodes) return fail(VSM_EHIP);  // (cannot be: nothing is sized by it then)
  VsmLayout ol;
  ol.at = o_out;
  const size_t r_counters = ol.take(16), r_offsets = ol.take(((size_t)n_tracks + 1) * 4), r_obs = ol.take((size_t)n_obs * 16),
               r_tom = ol.take((size_t)n_edges * 4), r_flags = ol.take((size_t)n_tracks);
  d.offsets = (int32_t *)(S.dev + r_offsets);
  d.obs = (int32_t *)(S.dev + r_obs);
  d.track_of_match = (int32_t *)(S.dev + r_tom);
  d.flags = (uint8_t *)(S.dev + r_flags);
  const size_t out_bytes = ol.at - o_out;
  VSM_CHK(S.grow_out(out_bytes, h->stream));
  vsm_tracks_launch_emit(h->stream, h->prof, d, n_tracks, n_obs);
  VSM_CHK(hipGetLastError());
  VSM_CHK(hipEventRecord(S.ev[2], h->stream));
  VSM_CHK(hipMemcpyAsync(S.pin_out, S.dev + o_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
  VSM_CHK(hipStreamSynchronize(h->stream));
  VSM_CHK(hipGetLastError());
  if (h->prof.on) h->prof.resolve();
  // ---- into the handle's vectors; the segments no workgroup took are ordered here ----
  const uint8_t *out = S.pin_out;
  const int32_t *r_off = (const int32_t *)(out + (r_offsets - o_out));
  T.offsets.assign(r_off, r_off + n_tracks + 1);
  const int32_t *r_rows = (const int32_t *)(out + (r_obs - o_out));
  T.obs.assign(r_rows, r_rows + 4 * (size_t)n_obs);
  const int32_t *r_t = (const int32_t *)(out + (r_tom - o_out));
  T.track_of_match.assign(r_t, r_t + n_edges);
  T.flags.assign(out + (r_flags - o_out), out + (r_flags - o_out) + n_tracks);
  int64_t by_host = 0, inconsistent = 0;
  for (int32_t t = 0; t < n_tracks; t++) {
    const int32_t len = T.offsets[t + 1] - T.offsets[t];
    if (len > VSM_TRACKS_BLOCK_MAX) {
      T.flags[t] = (uint8_t)trk_sort_segment(T.obs.data() + 4 * (size_t)T.offsets[t], len);
      by_host++;
    }
    inconsistent += T.flags[t] & 1;
  }
  const int64_t by_block = ((const int32_t *)(out + (r_counters - o_out)))[0];
  T.stats[0] = n_nodes;
  T.stats[1] = n_edges;
  T.stats[2] = n_tracks;
  T.stats[3] = inconsistent;
  T.stats[4] = n_tracks - by_block - by_host;
  T.stats[5] = by_block;
  T.stats[6] = by_host;
  float ms_up = 0, ms_k = 0;
  (void)hipEventElapsedTime(&ms_up, S.ev[0], S.ev[1]);
  (void)hipEventElapsedTime(&ms_k, S.ev[1], S.ev[2]);
  const double t2 = now_us();
  T.timings[1] = ms_up * 1e3;
  T.timings[2] = ms_k * 1e3;
  T.timings[3] = std::max(0.0, (t2 - t1) - T.timings[1] - T.timings[2]);
  T.have = true;
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
void vsm_tracks_get_stats(vsm_handle *h, int64_t *out8) {
  const VsmTracks *T = tracks_result(h);
  vsm_copy_or_zero(T ? &T->stats : nullptr, out8);
}
void vsm_tracks_get_timings(vsm_handle *h, double *out4) {
  const VsmTracks *T = tracks_result(h);
  vsm_copy_or_zero(T ? &T->timings : nullptr, out4);
}

}  // extern "C"
