// Monocular motion of every pair of a pair set in one call: what vsm_mono.hip's
// batch engine (vsm_motions.inc) and the handle's C ABI (vsm_motions_api.inc, in vsm_api.cpp) share.  Per pair the result
// is that of vsm_vo_sampler_seed(71) + vsm_host_estimate_motion_mono on the pair's list (bucketed first, if asked, like a
// fresh VisualOdometryMono's second process()); every pair owns its sampler and its rand() stream.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <cmath>

#include <vector>

#include "visomatch.h"
#include "vsm_host.h"
#include "vsm_stage.h"

// where a pair's estimate ended (vsm_motions_get's `stage`)
enum {
  VSM_MOT_FEW_MATCHES = 0,   // n < 10                                  rc -1
  VSM_MOT_DEGENERATE = 1,    // normalisation degenerate                rc -1
  VSM_MOT_FEW_INLIERS = 2,   // fewer than 10 inliers                   rc 0
  VSM_MOT_NONE_IN_FRONT = 3, // no R|t candidate with a point in front  rc 0
  VSM_MOT_FEW_IN_FRONT = 4,  // fewer than 10 points in front           rc 0
  VSM_MOT_MEDIAN = 5,        // median above motion_threshold           rc 0
  VSM_MOT_OK = 6             //                                         rc 1
};
// stats[0..6] pairs per stage, then the pairs whose fit / count / triangulation / vote came from the device, chunks, waits
enum { VSM_MOT_STAT_FIT = 7, VSM_MOT_STAT_COUNT = 8, VSM_MOT_STAT_TRI = 9, VSM_MOT_STAT_VOTE = 10, VSM_MOT_STAT_CHUNKS = 11, VSM_MOT_STAT_WAITS = 12, VSM_MOT_STATS = 13 };

struct VsmMotionsResult {
  bool have = false;
  std::vector<int32_t> rc, stage;
  std::vector<double> tr6, T16;  // zeros / the identity where rc != 1
  std::vector<std::vector<int32_t>> inliers;    // indices into matches[k]; empty where rc == -1
  std::vector<std::vector<vsm_p_match>> matches;  // the list the estimate saw (bucketed, if bucketing was on)
  int64_t stats[VSM_MOT_STATS] = {};
  double timings[6] = {0, 0, 0, 0, 0, 0};  // sampling + packing + upload, fit + count + winner, host fits + E -> R|t, triangulation, median + vote, total; us
  void reset(int32_t n) {
    have = false;
    rc.assign((size_t)n, -1);
    stage.assign((size_t)n, 0);
    tr6.assign((size_t)6 * n, 0.0);
    T16.assign((size_t)16 * n, 0.0);
    for (int32_t k = 0; k < n; k++)
      for (int i = 0; i < 4; i++) T16[(size_t)16 * k + 5 * i] = 1.0;
    inliers.assign((size_t)n, std::vector<int32_t>());
    matches.assign((size_t)n, std::vector<vsm_p_match>());
    memset(stats, 0, sizeof(stats));
    memset(timings, 0, sizeof(timings));
  }
};

// the device path's staging (its events stay unused: the call times itself on the host) and the self-test's verdict
struct VsmMotionsDev {
  VsmStage st;  // pinned input and output, the device block, the events (vsm_stage.h)
  bool tested = false, svd_on_device = false;
};
void vsm_motions_dev_release(VsmMotionsDev &D);

inline bool vsm_motions_args_ok(const vsm_vo_mono_params *p, int32_t n_pairs, const vsm_p_match *const *lists, const int32_t *counts, int bucket) {
  if (!p || n_pairs <= 0 || !lists || !counts || p->ransac_iters < 0) return false;
  for (int32_t k = 0; k < n_pairs; k++)
    if (counts[k] < 0 || (counts[k] > 0 && !lists[k])) return false;
  // A NaN or an infinity in a flow coordinate makes every matrix of the pair NaN, and the SVD's sweep (vsm_linalg.h, the
  // textbook routine) then walks off its arrays - on the device too.  The matcher never produces one; a caller's list may.
  if (bucket && !(p->bucket_width > 0 && p->bucket_height > 0)) return false;
  for (int32_t k = 0; k < n_pairs; k++)
    for (int32_t i = 0; i < counts[k]; i++) {
      const vsm_p_match &m = lists[k][i];
      if (!(std::isfinite(m.u1p) && std::isfinite(m.v1p) && std::isfinite(m.u1c) && std::isfinite(m.v1c))) return false;
      if (bucket && (m.u1c < 0 || m.v1c < 0)) return false;  // (bucketFeatures has no bucket left of or above the image)
    }
  return true;
}

// Every pair through bucketing + MonoEgo::estimate on `threads` host threads, no GPU (pool: the threads to use instead, if given).
void vsm_motions_host(const vsm_vo_mono_params &par, int32_t n_pairs, const vsm_p_match *const *lists, const int32_t *counts, int bucket, int threads,
                      VsmPool *pool, VsmMotionsResult &out);
// The device path on `stream` (the current device), host stages on `pool`; chunk 0 = the memory rule.
// VSM_OK, or VSM_EHIP after a HIP error (nothing further is launched; `out` is then not a result).
int vsm_motions_device(VsmMotionsDev &D, hipStream_t stream, VsmPool *pool, const vsm_vo_mono_params &par, int32_t n_pairs, const vsm_p_match *const *lists,
                       const int32_t *counts, int bucket, int chunk, VsmMotionsResult &out);
