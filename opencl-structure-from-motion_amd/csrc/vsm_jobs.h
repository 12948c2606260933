// The batched forms' pure arithmetic, each rule once: what a frame pair's job is, the job tables of
// a look-ahead chunk and of a pair list, the chunk plans of the two look-ahead forms, and the device chain's size limits.
// No HIP call and nothing of a handle in here, so the CPU suite pins it through the debug entries of include/visomatch.h
// (tests/test_chunk_jobs.py, test_pair_jobs.py, test_seq_plan.py) and tools/jobs_host_check.cpp under the sanitizers.
// Included by vsm_api.cpp in front of the .inc files.
#pragma once

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "vsm_dc_gpu.h"
#include "vsm_internal.h"

// sanity checks of viso/matcher.cpp:190-212 on feature counts n[image 1p,2p,1c,2c][set]
// (a NULL set and an empty set are both "count 0" here)
static inline bool match_ready(const vsm_params &p, int method, const int32_t n[4][2]) {
  if (method == 0) {
    if (n[0][1] == 0 || n[2][1] == 0) return false;
    if (p.multi_stage && (n[0][0] == 0 || n[2][0] == 0)) return false;
  } else if (method == 1) {
    if (n[2][1] == 0 || n[3][1] == 0) return false;
    if (p.multi_stage && (n[2][0] == 0 || n[3][0] == 0)) return false;
  } else {
    if (n[0][1] == 0 || n[1][1] == 0 || n[2][1] == 0 || n[3][1] == 0) return false;
    if (p.multi_stage && (n[0][0] == 0 || n[1][0] == 0 || n[2][0] == 0 || n[3][0] == 0)) return false;
  }
  return true;
}

static inline VsmMatchCfg make_cfg(const vsm_params &p, int method, int heads) {
  VsmMatchCfg cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.method = method;
  cfg.heads = heads;
  cfg.binsize = p.match_binsize;
  cfg.bin_magic = p.match_binsize >= 2 ? (uint32_t)(((1ull << 32) + (uint64_t)p.match_binsize - 1) / (uint64_t)p.match_binsize) : 0u;
  cfg.radius = p.match_radius;
  cfg.disp_tol = p.match_disp_tolerance;
  cfg.f = p.f;
  cfg.cu = p.cu;
  cfg.cv = p.cv;
  cfg.base = p.base;
  return cfg;
}

// a job that matches nothing: zeroed, with its image slots (left image ids; stereo matching only reads the current frame,
// so its callers name the current slot twice)
static inline void vsm_job_slots(VsmJob &jb, int img_prev, int img_curr) {
  memset(&jb, 0, sizeof(jb));
  jb.img_prev = img_prev;
  jb.img_curr = img_curr;
}

// The one statement of a frame pair's job: what Matcher::matchFeatures(method, Tr) does with images whose feature counts
// are cnt[image 1p,2p,1c,2c][set] (viso/matcher.cpp:190-216).  The job gets its slots; where matchFeatures would run
// (match_ready) - and only there - its query counts (quad matching iterates the previous left features, flow and stereo
// the current ones; the sparse pass only with multi_stage) and Tr (12 doubles, or NULL: none).  The query counts are folded
// into max_nq (may be NULL).  Returns whether matchFeatures would run.
static inline bool vsm_job_fill(const vsm_params &p, int method, const int32_t cnt[4][2], int img_prev, int img_curr, const double *Tr, VsmJob &jb,
                                int max_nq[2]) {
  vsm_job_slots(jb, img_prev, img_curr);
  if (!match_ready(p, method, cnt)) return false;
  const int qimg = method == 2 ? 0 : 2;
  jb.nq[0] = p.multi_stage ? cnt[qimg][0] : 0;
  jb.nq[1] = cnt[qimg][1];
  if (Tr) {
    jb.use_tr = 1;
    memcpy(jb.t, Tr, 12 * sizeof(double));
  }
  if (max_nq) {
    max_nq[0] = std::max(max_nq[0], jb.nq[0]);
    max_nq[1] = std::max(max_nq[1], jb.nq[1]);
  }
  return true;
}

// The job table of one chunk of a batched form: frames f0 .. f0 + n - 1, whose images stand in slots first_img, first_img +
// sides, ... (sides: images per frame) and whose feature counts the device has written into `counts` ([image][set], the
// layout of VsmCtx::hm_counts); img_before: the slot of frame f0 - 1, the last one of the previous chunk's bank.  That
// bank's counts may be gone by now: nprev[side][set] carries the counts of frame f0 - 1 in, and those of the chunk's last
// frame out.  Per frame: the job (vsm_job_fill; Tr / Tr_valid per FRAME), valid (may be NULL), and seq_src
// (vsm_handle::seq_src: a frame that is not matched keeps the list of the one before).
static inline void seq_chunk_jobs(const vsm_params &p, int method, int sides, int32_t f0, int n, int first_img, int img_before, const int32_t *counts,
                                  int32_t nprev[2][2], const double *Tr, const uint8_t *Tr_valid, VsmJob *jobs, char *valid, int max_nq[2],
                                  int32_t *seq_src) {
  max_nq[0] = max_nq[1] = 0;
  for (int i = 0; i < n; i++) {
    const int32_t f = f0 + i;
    const int img_c = first_img + sides * i;
    int img_p;
    int32_t cnt[4][2];
    for (int s = 0; s < 2; s++) {
      cnt[2][s] = counts[img_c * 2 + s];
      cnt[3][s] = sides == 2 ? counts[(img_c + 1) * 2 + s] : 0;
    }
    if (method == 1) {
      img_p = img_c;
      for (int s = 0; s < 2; s++) cnt[0][s] = cnt[1][s] = 0;
    } else if (i > 0) {
      img_p = img_c - sides;
      for (int s = 0; s < 2; s++) {
        cnt[0][s] = counts[img_p * 2 + s];
        cnt[1][s] = sides == 2 ? counts[(img_p + 1) * 2 + s] : 0;
      }
    } else {  // the previous frame is the last one of the previous chunk's bank
      img_p = img_before;
      for (int s = 0; s < 2; s++) {
        cnt[0][s] = f > 0 ? nprev[0][s] : 0;
        cnt[1][s] = f > 0 ? nprev[1][s] : 0;
      }
    }
    const bool ready = vsm_job_fill(p, method, cnt, img_p, img_c, Tr && (!Tr_valid || Tr_valid[f]) ? Tr + (size_t)f * 12 : nullptr, jobs[i], max_nq);
    if (valid) valid[i] = ready ? 1 : 0;
    seq_src[f] = ready ? f : (f > 0 ? seq_src[f - 1] : -1);
  }
  for (int s = 0; s < 2; s++) {  // remember the last frame's counts for the next chunk
    nprev[0][s] = counts[(first_img + sides * (n - 1)) * 2 + s];
    nprev[1][s] = sides == 2 ? counts[(first_img + sides * (n - 1) + 1) * 2 + s] : 0;
  }
}
// the slot of the frame in front of chunk k's first one: the last frame of chunk k - 1, in the bank before chunk k's
static inline int seq_slot_before(const std::vector<int32_t> &chunk_start, int k, int sides, int banks, int C) {
  return sides * ((k + banks - 1) % banks) * C + sides * ((k > 0 ? chunk_start[k] - chunk_start[k - 1] : 1) - 1);
}

// The job table of a list of arbitrary frame pairs (vsm_pairs_run): pair k = pairs[2 k], pairs[2 k + 1] = (previous frame,
// current frame) of a frame set whose images all stand in one context, frame f's at slots sides * f (+ 1: its right image),
// with the feature counts the device has written into `counts` ([image][set], the layout of VsmCtx::hm_counts).  Per pair
// what a fresh matcher does after pushBack(previous), pushBack(current), matchFeatures(method, Tr of the pair): the job
// (vsm_job_fill), valid, and the longest query lists.  Stereo matching does not read the previous frame: its slot is the
// current one's, whatever the pair names.  Tr / Tr_valid: per PAIR (NULL: none / all valid).
static inline void pair_jobs(const vsm_params &p, int method, int sides, const int32_t *counts, const int32_t *pairs, int n, const double *Tr,
                             const uint8_t *Tr_valid, VsmJob *jobs, char *valid, int max_nq[2]) {
  max_nq[0] = max_nq[1] = 0;
  for (int k = 0; k < n; k++) {
    const int img_c = sides * pairs[2 * k + 1], img_p = method == 1 ? img_c : sides * pairs[2 * k];
    int32_t cnt[4][2];
    for (int s = 0; s < 2; s++) {
      cnt[0][s] = method == 1 ? 0 : counts[img_p * 2 + s];
      cnt[1][s] = method == 1 || sides != 2 ? 0 : counts[(img_p + 1) * 2 + s];
      cnt[2][s] = counts[img_c * 2 + s];
      cnt[3][s] = sides == 2 ? counts[(img_c + 1) * 2 + s] : 0;
    }
    const bool ready = vsm_job_fill(p, method, cnt, img_p, img_c, Tr && (!Tr_valid || Tr_valid[k]) ? Tr + (size_t)k * 12 : nullptr, jobs[k], max_nq);
    if (valid) valid[k] = ready ? 1 : 0;
  }
}
// the argument checks of vsm_pairs_run on its pair list: every current frame inside the set, every previous one too - or,
// with stereo matching (which does not read it), -1
static inline bool pair_list_ok(int method, int32_t n_frames, const int32_t *pairs, int32_t n_pairs) {
  if (method < 0 || method > 2 || n_frames <= 0 || !pairs || n_pairs <= 0) return false;
  for (int32_t k = 0; k < n_pairs; k++) {
    const int32_t a = pairs[2 * k], b = pairs[2 * k + 1];
    if (b < 0 || b >= n_frames || a >= n_frames || a < (method == 1 ? -1 : 0)) return false;
  }
  return true;
}

// The chunk plan of a look-ahead call of the GPU-resident form (vsm_seq2.inc; vsm_pairs_run takes its chunk size from it):
// the chunk size C (the frame and pair banks' stride) and the frame every chunk starts at (start[nchunks] = n_frames).
// `plan`: the call passes getenv("VSM_SEQ_PLAN").
struct Seq2Plan {
  int C = 0;
  std::vector<int32_t> start;
};
static inline Seq2Plan seq2_plan(int32_t n_frames, int pool_threads, bool host_in, int seq_chunk, int seq_first_chunk, const char *plan) {
  // Chunk size.  A final chain is a row of latency-bound kernels and takes about as long for 50 lists as for 80, so fewer,
  // larger chunks pay as long as the host keeps up with their vertex sorts.  Measured (200 frames 1242x375, ms per sequence,
  // 14 pool threads, round 4's five-queue layout): 6.0 / 5.15 / 4.65 / 4.55 / 4.56 / 4.61 / 4.97 with chunks of 40 / 50 / 67 /
  // 80 / 84 / 90 / 100 (80: 80 + 80 + 40 - the last, short chain is the call's tail).  With the copy engine's order planned
  // (export_some) and the last chunk's sort + kd order in front of its predecessor's block kernel, TWO chunks beat three for
  // ranks with ten pool threads or more - 4.60 / 4.76 / 4.34 / 4.28 / 4.30 / 4.33 / 4.40 with 80 / 90 / 100 / 105 / 110 / 115 / 120
  // / 134 (110: 110 + 90) -; with eight threads the pool's vertex sorts bound the call either way (5.3 ms), with four 50 wins.
  // Host-resident inputs: the first chunk's upload is the one transfer nothing hides, so the first chunk is HALF a chunk
  // (and the chunks a little larger, so that 200 frames still make three): 40 + 80 + 80.
  // (three host threads or fewer: the device sorts a share of the final lists in one launch behind the call's last keys, and
  // every chunk's survivors cross PCIe behind that - two chunks of 100: 7.6 ms against 8.3 with four of 50)
  int C = seq_chunk > 0 ? seq_chunk : (pool_threads >= 10 && !host_in ? 110 : (pool_threads >= 6 ? 80 : (pool_threads <= 4 && !host_in ? 100 : 50)));
  if (C > n_frames) C = n_frames;
  if (seq_chunk <= 0 && n_frames > C && n_frames % C != 0 && n_frames % C < C / 2) {
    // (a short last chunk costs a whole chain's latency at the end of the call: 1000 frames are ten chunks of 100, not nine
    // of 110 and one of 10; 200 stay 110 + 90)
    const int nch = (n_frames + C - 1) / C;
    C = (n_frames + nch - 1) / nch;
  }
  Seq2Plan P;
  P.C = C;
  std::vector<int32_t> &chunk_start = P.start;
  if (host_in && plan) {  // (experiments: the chunks' sizes, "40,80,60,20")
    chunk_start.push_back(0);
    for (const char *q = plan; *q && chunk_start.back() < n_frames;) {
      const int v = std::min(std::max(atoi(q), 2), C);
      chunk_start.push_back(std::min(n_frames, chunk_start.back() + v));
      while (*q && *q != ',') q++;
      if (*q == ',') q++;
    }
    while (chunk_start.back() < n_frames) chunk_start.push_back(std::min(n_frames, chunk_start.back() + C));
    chunk_start.pop_back();
  } else if (host_in && n_frames > C && C >= 2) {
    chunk_start.push_back(0);
    for (int32_t f = C / 2; f < n_frames; f += C) chunk_start.push_back(f);
    // (the frames arrive at the link's rate and the GPU keeps up with them: what the call waits for at its end is everything
    // that follows the LAST frames' arrival - features, both passes, two chain latencies - so the last chunk is a short one)
    if (n_frames - chunk_start.back() > 30) chunk_start.push_back(n_frames - 20);
  } else if (seq_first_chunk > 0 && seq_first_chunk < C && n_frames > C) {
    chunk_start.push_back(0);
    for (int32_t f = seq_first_chunk; f < n_frames; f += C) chunk_start.push_back(f);
  } else {
    for (int32_t f = 0; f < n_frames; f += C) chunk_start.push_back(f);
  }
  chunk_start.push_back(n_frames);
  return P;
}

// The chunk boundaries of the host-shared form (vsm_seq1.inc), start[nchunks] = n_frames: chunks of C frames; a sequence of
// at least three chunks starts (and ends) with a half chunk - the host pool has nothing to do until the first chunk's lists
// exist, and nothing overlaps the last chunk's final stage
static inline std::vector<int32_t> seq1_plan(int32_t n_frames, int C) {
  std::vector<int32_t> chunk_start;
  const int32_t half = C / 2;
  int32_t f = 0;
  if (half >= 8 && n_frames >= 3 * C) {
    chunk_start.push_back(0);
    f = half;
    while (n_frames - f > C + half) {
      chunk_start.push_back(f);
      f += C;
    }
    if (n_frames - f > C) {  // between C and 3C/2 frames left: a full chunk and a short one
      chunk_start.push_back(f);
      f = n_frames - std::min<int32_t>(half, n_frames - f - 1);
    }
    chunk_start.push_back(f);
  } else {
    for (; f < n_frames; f += C) chunk_start.push_back(f);
  }
  chunk_start.push_back(n_frames);
  return chunk_start;
}

// Every size limit of the device chain on the longest first-pass and second-pass list a job table can give (max_nq): the
// triangulation's own limits on both, the limit of the sub-pixel fits' batched tail on the second, and max_p1 on the
// first - VSM_DC_KD_MAX_POINTS where the pool sorts the first-pass lists' vertices (vsm_step.inc), VSM_DC_TIE_POINTS where
// the device may (vsm_seq2.inc).
static inline bool vsm_chain_fits(const vsm_params &p, const int max_nq[2], int max_p1) {
  return max_nq[0] <= max_p1 && max_nq[1] <= VSM_DC_KD_MAX_POINTS && vsm_dc2_depth(std::max(max_nq[0], max_nq[1])) <= VSM_DC2_MAX_DEPTH &&
         !(p.refinement == 2 && max_nq[1] > VSM_PARA_MAX_LIST);
}
