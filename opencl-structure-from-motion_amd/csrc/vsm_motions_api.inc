// Monocular pair motions on a handle (included by vsm_api.cpp; the engine is vsm_motions.inc in vsm_mono.hip, DESIGN.md
// section 5).  The handle keeps the staging that only grows and the last result; the streaming ring, the pairs lists and the
// track and point results are neither read for writing nor touched.
struct VsmMotions {
  VsmMotionsDev dev;
  VsmMotionsResult res;
};

static void motions_destroy(vsm_handle *h) {
  if (!h->motions) return;
  vsm_motions_dev_release(h->motions->dev);
  delete h->motions;
  h->motions = nullptr;
}

static int motions_run(vsm_handle *h, const vsm_vo_mono_params *params, int32_t n_pairs, const vsm_p_match *const *lists, const int32_t *counts, int32_t bucket) {
  HIPCHK(hipSetDevice(h->device));
  if (!h->motions) h->motions = new VsmMotions();
  VsmMotions &M = *h->motions;
  M.res.have = false;  // from here on the call replaces the last result
  return vsm_motions_device(M.dev, h->stream, h->pool, *params, n_pairs, lists, counts, bucket != 0, h->sw.motions_chunk, M.res);
}

extern "C" {

int vsm_motions_run(vsm_handle *h, const vsm_vo_mono_params *params, int32_t n_pairs, const vsm_p_match *const *lists, const int32_t *counts, int32_t bucket) {
  if (!h || !vsm_motions_args_ok(params, n_pairs, lists, counts, bucket)) return VSM_EARG;
  return motions_run(h, params, n_pairs, lists, counts, bucket);
}

int vsm_pairs_motions(vsm_handle *h, const vsm_vo_mono_params *params, int32_t bucket) {
  if (!h) return VSM_EARG;
  std::vector<const vsm_p_match *> lists;
  std::vector<int32_t> counts;
  const VsmPairs *PR = pairs_last_lists(h, lists, counts);
  if (!PR) return VSM_ENOTREADY;
  if (PR->method == 1 || lists.empty()) return VSM_EARG;  // stereo matches have no previous frame to move from
  const int32_t n_pairs = (int32_t)lists.size();
  if (!vsm_motions_args_ok(params, n_pairs, lists.data(), counts.data(), bucket)) return VSM_EARG;
  return motions_run(h, params, n_pairs, lists.data(), counts.data(), bucket);
}

static const VsmMotionsResult *motions_result(vsm_handle *h) { return (h && h->motions && h->motions->res.have) ? &h->motions->res : nullptr; }

int32_t vsm_motions_count(vsm_handle *h) {
  const VsmMotionsResult *R = motions_result(h);
  return R ? (int32_t)R->rc.size() : 0;
}
int32_t vsm_motions_get(vsm_handle *h, int32_t *rc, int32_t *stage, double *tr6, double *T16, int32_t *n_inliers) {
  const VsmMotionsResult *R = motions_result(h);
  if (!R) return 0;
  const size_t P = R->rc.size();
  if (rc) memcpy(rc, R->rc.data(), P * 4);
  if (stage) memcpy(stage, R->stage.data(), P * 4);
  if (tr6) memcpy(tr6, R->tr6.data(), P * 6 * 8);
  if (T16) memcpy(T16, R->T16.data(), P * 16 * 8);
  if (n_inliers)
    for (size_t k = 0; k < P; k++) n_inliers[k] = (int32_t)R->inliers[k].size();
  return (int32_t)P;
}
int32_t vsm_motions_inliers(vsm_handle *h, int32_t pair, int32_t *out, int32_t cap) {
  const VsmMotionsResult *R = motions_result(h);
  if (!R || pair < 0 || pair >= (int32_t)R->rc.size()) return 0;
  const std::vector<int32_t> &v = R->inliers[pair];
  if (!out) return (int32_t)v.size();
  const int32_t n = std::min((int32_t)v.size(), cap);
  if (n > 0) memcpy(out, v.data(), (size_t)n * 4);
  return n;
}
int32_t vsm_motions_matches(vsm_handle *h, int32_t pair, vsm_p_match *out, int32_t cap) {
  const VsmMotionsResult *R = motions_result(h);
  if (!R || pair < 0 || pair >= (int32_t)R->rc.size()) return 0;
  const std::vector<vsm_p_match> &v = R->matches[pair];
  if (!out) return (int32_t)v.size();
  const int32_t n = std::min((int32_t)v.size(), cap);
  if (n > 0) memcpy(out, v.data(), (size_t)n * sizeof(vsm_p_match));
  return n;
}
void vsm_motions_get_stats(vsm_handle *h, int64_t *out13) {
  const VsmMotionsResult *R = motions_result(h);
  vsm_copy_or_zero(R ? &R->stats : nullptr, out13);
}
void vsm_motions_get_timings(vsm_handle *h, double *out6) {
  const VsmMotionsResult *R = motions_result(h);
  vsm_copy_or_zero(R ? &R->timings : nullptr, out6);
}
int vsm_motions_device_svd(vsm_handle *h) { return (h && h->motions && h->motions->dev.tested && h->motions->dev.svd_on_device) ? 1 : 0; }

}  // extern "C"
