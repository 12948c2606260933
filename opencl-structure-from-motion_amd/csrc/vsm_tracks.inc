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
  uint8_t *pin_in = nullptr, *pin_out = nullptr, *dev = nullptr;  // sizes that only grow
  size_t pin_in_bytes = 0, pin_out_bytes = 0, dev_bytes = 0;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // (with timing) start, uploaded, kernels done
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
  if (T->pin_in) (void)hipHostFree(T->pin_in);
  if (T->pin_out) (void)hipHostFree(T->pin_out);
  if (T->dev) vsm_dev_free(T->dev);
  for (hipEvent_t e : T->ev)
    if (e) (void)hipEventDestroy(e);
  delete T;
  h->tracks = nullptr;
}

// byte offsets of consecutive blocks, each 256-aligned
struct TrkLayout {
  size_t at = 0;
  size_t take(size_t bytes) {
    const size_t o = at;
    at = al256(at + bytes);
    return o;
  }
};

static int tracks_run(vsm_handle *h, int32_t n_frames, const int32_t *pairs, int32_t n_pairs, const vsm_p_match *const *lists, const int32_t *counts,
                      int32_t side, int32_t min_length) {
  const double t0 = now_us();
  const int64_t n_edges64 = trk_check_args(n_frames, pairs, n_pairs, lists, counts, side, min_length);
  if (n_edges64 < 0) return VSM_EARG;
  const int32_t n_edges = (int32_t)n_edges64;
  HIPCHK(hipSetDevice(h->device));
  if (!h->tracks) h->tracks = new VsmTracks();
  VsmTracks &T = *h->tracks;
  // ---- pack: (ip, ic) of every match, behind the three tables, in one pinned block ----
  TrkLayout in;
  const size_t o_pair_base = in.take(((size_t)n_pairs + 1) * 4), o_pairs = in.take((size_t)n_pairs * 8 + 4), o_feat_base = in.take(((size_t)n_frames + 1) * 4),
               o_edges = in.take((size_t)n_edges * 8 + 4);
  if (in.at > T.pin_in_bytes) {
    (void)hipStreamSynchronize(h->stream);
    if (T.pin_in) (void)hipHostFree(T.pin_in);
    T.pin_in = nullptr;
    T.pin_in_bytes = 0;
    HIPCHK(hipHostMalloc((void **)&T.pin_in, in.at + in.at / 4, hipHostMallocDefault));
    T.pin_in_bytes = in.at + in.at / 4;
  }
  int32_t *p_pair_base = (int32_t *)(T.pin_in + o_pair_base), *p_pairs = (int32_t *)(T.pin_in + o_pairs), *p_feat_base = (int32_t *)(T.pin_in + o_feat_base),
          *p_edges = (int32_t *)(T.pin_in + o_edges);
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
  size_t scan_part_items = 0;
  for (int64_t n = n_nodes; n > TRK_SCAN_BLOCK;) {
    n = (n + TRK_SCAN_BLOCK - 1) / TRK_SCAN_BLOCK;
    scan_part_items += (size_t)n;
  }
  TrkLayout dl = in;
  const size_t N = (size_t)n_nodes;
  const size_t o_parent = dl.take(N * 4), o_first = dl.take(N * 4), o_size = dl.take(N * 4), o_cursor = dl.take(N * 4), o_scan = dl.take(N * 8),
               o_part = dl.take(scan_part_items * 8 + 8), o_totals = dl.take(8), o_mid = dl.take((N / (VSM_TRACKS_WAVE_MAX + 1) + 1) * 4), o_out = dl.take(0);
  // the results' upper bounds: every node an observation, every node a track
  const size_t out_cap = al256(16) + al256((N + 1) * 4) + al256(N * 16) + al256((size_t)n_edges * 4) + al256(N);
  const size_t need = o_out + out_cap;
  if (need > T.dev_bytes) {
    (void)hipStreamSynchronize(h->stream);
    if (T.dev) vsm_dev_free(T.dev);
    T.dev = nullptr;
    T.dev_bytes = 0;
    HIPCHK(vsm_dev_alloc((void **)&T.dev, need + need / 4));
    T.dev_bytes = need + need / 4;
  }
  for (hipEvent_t &e : T.ev)
    if (!e) HIPCHK(hipEventCreate(&e));
  if (T.pin_out_bytes < 256) {
    HIPCHK(hipHostMalloc((void **)&T.pin_out, 4096, hipHostMallocDefault));
    T.pin_out_bytes = 4096;
  }
  // a call that fails after something was enqueued: drain the device, report
  auto fail = [&](int rc) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipGetLastError();
    return rc;
  };
#define TRACKS_CHK(call)                                                           \
  do {                                                                             \
    const hipError_t e_ = (call);                                                  \
    if (e_ != hipSuccess) {                                                        \
      fprintf(stderr, "visomatch: %s failed: %s\n", #call, hipGetErrorString(e_)); \
      return fail(VSM_EHIP);                                                       \
    }                                                                              \
  } while (0)
  TrkDevice d;
  memset(&d, 0, sizeof(d));
  d.pair_base = (const int32_t *)(T.dev + o_pair_base);
  d.pairs = (const int32_t *)(T.dev + o_pairs);
  d.feat_base = (const int32_t *)(T.dev + o_feat_base);
  d.edges = (const int32_t *)(T.dev + o_edges);
  d.parent = (int32_t *)(T.dev + o_parent);
  d.first = (int32_t *)(T.dev + o_first);
  d.size = (int32_t *)(T.dev + o_size);
  d.cursor = (int32_t *)(T.dev + o_cursor);
  d.scan = (int32_t *)(T.dev + o_scan);
  d.scan_part = (int32_t *)(T.dev + o_part);
  d.totals = (int32_t *)(T.dev + o_totals);
  d.mid_list = (int32_t *)(T.dev + o_mid);
  d.counters = (int32_t *)(T.dev + o_out);
  d.n_nodes = n_nodes;
  d.n_edges = n_edges;
  d.n_pairs = n_pairs;
  d.n_frames = n_frames;
  d.min_length = min_length;
  TRACKS_CHK(hipEventRecord(T.ev[0], h->stream));
  TRACKS_CHK(hipMemcpyAsync(T.dev, T.pin_in, in.at, hipMemcpyHostToDevice, h->stream));
  TRACKS_CHK(hipEventRecord(T.ev[1], h->stream));
  vsm_tracks_launch_link(h->stream, h->prof, d);
  TRACKS_CHK(hipGetLastError());
  // the totals size the results: the one place where the host waits in the middle of the call
  TRACKS_CHK(hipMemcpyAsync(T.pin_out, d.totals, 8, hipMemcpyDeviceToHost, h->stream));
  TRACKS_CHK(hipStreamSynchronize(h->stream));
  const int32_t n_tracks = ((int32_t *)T.pin_out)[0], n_obs = ((int32_t *)T.pin_out)[1];
  if (n_tracks < 0 || n_tracks > n_nodes || n_obs < 0 || n_obs > n_nodes) return fail(VSM_EHIP);  // (cannot be: nothing is sized by it then)
  TrkLayout ol;
  ol.at = o_out;
  const size_t r_counters = ol.take(16), r_offsets = ol.take(((size_t)n_tracks + 1) * 4), r_obs = ol.take((size_t)n_obs * 16),
               r_tom = ol.take((size_t)n_edges * 4), r_flags = ol.take((size_t)n_tracks);
  d.offsets = (int32_t *)(T.dev + r_offsets);
  d.obs = (int32_t *)(T.dev + r_obs);
  d.track_of_match = (int32_t *)(T.dev + r_tom);
  d.flags = (uint8_t *)(T.dev + r_flags);
  const size_t out_bytes = ol.at - o_out;
  if (out_bytes > T.pin_out_bytes) {
    (void)hipHostFree(T.pin_out);
    T.pin_out = nullptr;
    T.pin_out_bytes = 0;
    TRACKS_CHK(hipHostMalloc((void **)&T.pin_out, out_bytes + out_bytes / 4, hipHostMallocDefault));
    T.pin_out_bytes = out_bytes + out_bytes / 4;
  }
  vsm_tracks_launch_emit(h->stream, h->prof, d, n_tracks, n_obs);
  TRACKS_CHK(hipGetLastError());
  TRACKS_CHK(hipEventRecord(T.ev[2], h->stream));
  TRACKS_CHK(hipMemcpyAsync(T.pin_out, T.dev + o_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
  TRACKS_CHK(hipStreamSynchronize(h->stream));
  TRACKS_CHK(hipGetLastError());
  if (h->prof.on) h->prof.resolve();
  // ---- into the handle's vectors; the segments no workgroup took are ordered here ----
  const uint8_t *out = T.pin_out;
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
  (void)hipEventElapsedTime(&ms_up, T.ev[0], T.ev[1]);
  (void)hipEventElapsedTime(&ms_k, T.ev[1], T.ev[2]);
  const double t2 = now_us();
  T.timings[1] = ms_up * 1e3;
  T.timings[2] = ms_k * 1e3;
  T.timings[3] = std::max(0.0, (t2 - t1) - T.timings[1] - T.timings[2]);
  T.have = true;
  return VSM_OK;
#undef TRACKS_CHK
}

extern "C" {

int vsm_tracks_run(vsm_handle *h, int32_t n_frames, const int32_t *pairs, int32_t n_pairs, const vsm_p_match *const *lists, const int32_t *counts,
                   int32_t side, int32_t min_length) {
  if (!h) return VSM_EARG;
  return tracks_run(h, n_frames, pairs, n_pairs, lists, counts, side, min_length);
}

int vsm_pairs_tracks(vsm_handle *h, int32_t side, int32_t min_length) {
  if (!h) return VSM_EARG;
  const VsmPairs *P = h->pairs;
  if (!P || !P->done) return VSM_ENOTREADY;
  if (P->method == 1) return VSM_EARG;  // (stereo-only lists: tracks across time are not defined)
  const int32_t n_pairs = (int32_t)P->lists.size();
  std::vector<const vsm_p_match *> lists((size_t)n_pairs);
  std::vector<int32_t> counts((size_t)n_pairs);
  for (int32_t k = 0; k < n_pairs; k++) {
    lists[k] = P->lists[k].data();
    counts[k] = (int32_t)P->lists[k].size();
  }
  const int rc = tracks_run(h, P->n_frames, P->pair_list.data(), n_pairs, lists.data(), counts.data(), side, min_length);
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
  if (h && h->tracks && h->tracks->have)
    memcpy(out8, h->tracks->stats, sizeof(h->tracks->stats));
  else
    memset(out8, 0, 8 * sizeof(int64_t));
}
void vsm_tracks_get_timings(vsm_handle *h, double *out4) {
  if (h && h->tracks && h->tracks->have)
    memcpy(out4, h->tracks->timings, sizeof(h->tracks->timings));
  else
    memset(out4, 0, 4 * sizeof(double));
}

}  // extern "C"
