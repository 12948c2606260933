// Host scaffolding the structure-from-motion stages of a handle share (tracks, points, motions):
// the 256-aligned layout of a block, a stage's staging that only grows, the host-mapped result arena of the pairs and
// multi calls, the check macro of a call that has enqueued work, and the "result or zeros" copy of the getters.
// Included by vsm_api.cpp and by vsm_mono.hip (the motions engine lives there).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "visomatch.h"

// Device memory of the library's large blocks (vsm_api.cpp): a released block of 8 MB or more goes to a process-wide cache
// instead of back to the driver, and the next request of about its size takes it from there.
hipError_t vsm_dev_alloc(void **p, size_t bytes);
void vsm_dev_free(void *p);

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// byte offsets of consecutive blocks, each 256-aligned
struct VsmLayout {
  size_t at = 0;
  size_t take(size_t bytes) {
    const size_t o = at;
    at = al256(at + bytes);
    return o;
  }
};

// A stage's staging: a pinned input block, a pinned output block, one device block and the events start, uploaded,
// kernels done (with timing).  The rule, kept here and nowhere else: a block only grows, to 1.25 times what was asked
// for, and nothing is released before the stage's stream is idle - a copy or a kernel of an earlier call may still use it.
// A failed growth leaves the pointer null and the size 0, so the next call tries again.
struct VsmStage {
  uint8_t *pin_in = nullptr, *pin_out = nullptr, *dev = nullptr;
  size_t pin_in_bytes = 0, pin_out_bytes = 0, dev_bytes = 0;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};

  hipError_t grow_in(size_t need, hipStream_t stream) { return grow(pin_in, pin_in_bytes, need, 0, stream, false); }
  hipError_t grow_out(size_t need, hipStream_t stream, size_t min_bytes = 0) { return grow(pin_out, pin_out_bytes, need, min_bytes, stream, false); }
  hipError_t grow_dev(size_t need, hipStream_t stream) { return grow(dev, dev_bytes, need, 0, stream, true); }
  hipError_t events() {
    for (hipEvent_t &e : ev)
      if (!e) {
        const hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
      }
    return hipSuccess;
  }
  // (the caller has waited for the stream: vsm_destroy does before it takes a handle apart)
  void release() {
    if (pin_in) (void)hipHostFree(pin_in);
    if (pin_out) (void)hipHostFree(pin_out);
    if (dev) vsm_dev_free(dev);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    *this = VsmStage();
  }

 private:
  static hipError_t grow(uint8_t *&p, size_t &have, size_t need, size_t min_bytes, hipStream_t stream, bool device) {
    if (need <= have) return hipSuccess;
    (void)hipStreamSynchronize(stream);
    if (p && device) vsm_dev_free(p);
    if (p && !device) (void)hipHostFree(p);
    p = nullptr;
    have = 0;
    const size_t bytes = std::max(need + need / 4, min_bytes);
    const hipError_t rc = device ? vsm_dev_alloc((void **)&p, bytes) : hipHostMalloc((void **)&p, bytes, hipHostMallocDefault);
    if (rc != hipSuccess) {
      p = nullptr;
      return rc;
    }
    have = bytes;
    return hipSuccess;
  }
};

// The survivors of a bank of pairs (vsm_pairs_run) or sequences (vsm_multi_process), host-mapped: slot i of `res` takes
// list i, res_cnt[i] its length; the kernels write through the *_dev views.
struct VsmResArena {
  uint8_t *res = nullptr, *res_dev = nullptr;
  int32_t *res_cnt = nullptr, *res_cnt_dev = nullptr;
  size_t slot = 0;
  void free() {
    if (res) (void)hipHostFree(res);
    if (res_cnt) (void)hipHostFree(res_cnt);
    res = res_dev = nullptr;
    res_cnt = res_cnt_dev = nullptr;
  }
  // n slots of slot_bytes; false: nothing is allocated (the caller's stream is idle: the last arena goes first)
  bool alloc(size_t slot_bytes, size_t n) {
    free();
    slot = slot_bytes;
    if (hipHostMalloc((void **)&res, slot * n, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer((void **)&res_dev, res, 0) != hipSuccess ||
        hipHostMalloc((void **)&res_cnt, n * 4, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&res_cnt_dev, res_cnt, 0) != hipSuccess) {
      (void)hipGetLastError();
      free();
      return false;
    }
    return true;
  }
};

// In a call that has enqueued work, with `fail(rc)` in scope (it drains the stream, clears the sticky error and whatever
// else the call owns, and returns rc): a HIP error is reported and ends the call with VSM_EHIP.
#define VSM_CHK(call)                                                              \
  do {                                                                             \
    const hipError_t e_ = (call);                                                  \
    if (e_ != hipSuccess) {                                                        \
      fprintf(stderr, "visomatch: %s failed: %s\n", #call, hipGetErrorString(e_)); \
      return fail(VSM_EHIP);                                                       \
    }                                                                              \
  } while (0)

// a stats or timings getter: the array of the stage's last result, or zeros where there is none (src null)
template <typename T, size_t N>
static inline void vsm_copy_or_zero(const T (*src)[N], T *out) {
  if (src)
    memcpy(out, *src, sizeof(*src));
  else
    memset(out, 0, sizeof(*src));
}
