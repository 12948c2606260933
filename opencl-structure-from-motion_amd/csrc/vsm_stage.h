// Host scaffolding the structure-from-motion stages of a handle share (tracks, points, resection, vetting, motions;
// DESIGN.md section 5): the 256-aligned layout of a block and the arrays placed in it, the check macro and the drain of a
// call that has enqueued work, a stage's staging that only grows with its one round trip, the copies that keep a result, the
// close of a call's timings, the getters' copies, and the host-mapped result arena of the pairs and multi calls.
// Included by vsm_api.cpp and by vsm_mono.hip (the motions engine lives there); vsm_layouts.h has the stages' blocks.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "visomatch.h"
#include "vsm_host.h"

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

// The end of a call that fails after it has enqueued work on nothing but its stream: drain the stream, clear the sticky
// error, return rc.  `const VsmDrain fail{stream};` is the `fail` VSM_CHK asks for.
struct VsmDrain {
  hipStream_t stream;
  int operator()(int rc) const {
    (void)hipStreamSynchronize(stream);
    (void)hipGetLastError();
    return rc;
  }
};

// In a call that has enqueued work, with `fail(rc)` in scope (a VsmDrain, or a call object's own that also clears whatever
// else the call owns): a HIP error is reported and ends the call with VSM_EHIP.
#define VSM_CHK(call)                                                              \
  do {                                                                             \
    const hipError_t e_ = (call);                                                  \
    if (e_ != hipSuccess) {                                                        \
      fprintf(stderr, "visomatch: %s failed: %s\n", #call, hipGetErrorString(e_)); \
      return fail(VSM_EHIP);                                                       \
    }                                                                              \
  } while (0)

// The copies of a result from the pinned output into the handle's vectors, one add() per array.  By default each is the
// vector's assign, on the caller's thread.  on_pool: add() only sizes the vector and run(pool) copies, in pieces of 512 KB on
// the handle's pool when there is more than one - for the vetting's 13 bytes per observation, whose copies were most of its
// host part on one thread.  Results of a few bytes per track or frame stay with assign: a pool task at a call's end was
// measured slower, and so was sizing the tracks' cleared vectors before copying into them (profiles/README.md).
struct VsmKeep {
  struct Piece { uint8_t *dst; const uint8_t *src; size_t bytes; };
  const bool on_pool;
  std::vector<Piece> pieces;
  explicit VsmKeep(bool pool = false) : on_pool(pool) {}
  template <typename E>
  void add(std::vector<E> &vec, const E *src, size_t n) {
    if (!on_pool) return vec.assign(src, src + n);
    vec.resize(n);
    const size_t bytes = n * sizeof(E), step = (size_t)512 << 10;
    for (size_t at = 0; at < bytes; at += step) pieces.push_back({(uint8_t *)vec.data() + at, (const uint8_t *)src + at, std::min(step, bytes - at)});
  }
  template <class Pool>
  void run(Pool *pool) {
    if (pieces.size() > 1)
      pool->run((int)pieces.size(), [&](int i) { memcpy(pieces[i].dst, pieces[i].src, pieces[i].bytes); });
    else
      for (const Piece &p : pieces) memcpy(p.dst, p.src, p.bytes);
    pieces.clear();
  }
};

// What a stage's layout (vsm_layouts.h) gives the staging: the uploaded block `in`, the block copied back `out`, where
// `out` starts in the device block and the device block's size (working arrays may lie between or behind the two).
struct VsmBlocks {
  VsmLayout in, out;
  size_t out_at = 0, dev_bytes = 0;
  void out_behind_in(size_t out_end) { out_at = al256(in.at), dev_bytes = out_at + out_end; }  // (out_end: out.at, or past a working set)
};

// A stage's staging: a pinned input block, a pinned output block, one device block and the events start, uploaded,
// kernels done (with timing).  The rule, kept here and nowhere else: a block only grows, to 1.25 times what was asked
// for, and nothing is released before the stage's stream is idle - a copy or a kernel of an earlier call may still use it.
// A failed growth leaves the pointer null and the size 0, so the next call tries again.
struct VsmStage {
  uint8_t *pin_in = nullptr, *pin_out = nullptr, *dev = nullptr;
  size_t pin_in_bytes = 0, pin_out_bytes = 0, dev_bytes = 0;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  float ms[2] = {0, 0};  // {upload, kernels} of the call's round trip as the events measured them; zeros without one

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
  // a layout's device block and the events
  hipError_t fit_dev(const VsmBlocks &L, hipStream_t stream) {
    const hipError_t rc = grow_dev(L.dev_bytes, stream);
    ms[0] = ms[1] = 0;
    return rc != hipSuccess ? rc : events();
  }
  // The round trip of a call whose input is packed in the blocks L: upload of L.in, pre() on the stream (what has to be in
  // place before the kernels and counts as upload; vsm_no_pre: nothing), launch(), download of L.out, the call's single wait,
  // the profiler's spans, and the two elapsed times.  VSM_OK, or VSM_EHIP with the stream drained.
  template <class Prof, class Pre, class Launch>
  int round_trip(hipStream_t stream, Prof &prof, const VsmBlocks &L, Pre pre, Launch launch) {
    const VsmDrain fail{stream};
    VSM_CHK(hipEventRecord(ev[0], stream));
    VSM_CHK(hipMemcpyAsync(dev, pin_in, L.in.at, hipMemcpyHostToDevice, stream));
    VSM_CHK(pre());
    VSM_CHK(hipEventRecord(ev[1], stream));
    launch();
    VSM_CHK(hipGetLastError());
    VSM_CHK(hipEventRecord(ev[2], stream));
    VSM_CHK(hipMemcpyAsync(pin_out, dev + L.out_at, L.out.at, hipMemcpyDeviceToHost, stream));
    VSM_CHK(hipStreamSynchronize(stream));
    VSM_CHK(hipGetLastError());
    if (prof.on) prof.resolve();
    elapsed();
    return VSM_OK;
  }
  // ms = {start to uploaded, uploaded to kernels done} of the events' last recording, which the stream has passed
  void elapsed() {
    (void)hipEventElapsedTime(&ms[0], ev[0], ev[1]);
    (void)hipEventElapsedTime(&ms[1], ev[1], ev[2]);
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

// One array of a stage's blocks.  Its element type is stated where the layout declares it, its count and the spare bytes
// behind it where the layout places it - once each; the views below and the copy into the handle's vector come from that.
template <typename E>
struct VsmArray {
  size_t at = 0, n = 0;  // byte offset in its block, elements
  void place(VsmLayout &l, size_t count, size_t spare) {
    n = count;
    at = l.take(count * sizeof(E) + spare);
  }
  E *in(uint8_t *block) const { return (E *)(block + at); }  // the array in a copy of its block that starts at `block`
};
// A block being laid out: VsmLayout's offsets and, for the layout hooks, a row per array - its name, its image or pair (-1:
// one per block), its feature set (-1: none), where it lies and the bytes asked for.
struct VsmPlacer : VsmLayout {
  struct Row { const char *name; int32_t index, set; size_t at, bytes; };
  std::vector<Row> rows;
  template <typename E>
  void put(VsmArray<E> &a, const char *name, int index, int set, size_t count, size_t spare = 0) {
    a.place(*this, count, spare);
    rows.push_back({name, index, set, a.at, count * sizeof(E) + spare});
  }
};
// an array of the device block alone: a working set behind the uploaded block
template <typename E>
struct VsmDev : VsmArray<E> {
  E *dev(const VsmStage &S) const { return this->in(S.dev); }
};
// an uploaded array: the same offset in the pinned input
template <typename E>
struct VsmIn : VsmDev<E> {
  E *host(const VsmStage &S) const { return this->in(S.pin_in); }
};
// an array of the block that is copied back (or of the working set placed behind it); `out_at` is its blocks' (VsmBlocks)
template <typename E>
struct VsmOut : VsmArray<E> {
  E *dev(const VsmStage &S, size_t out_at) const { return this->in(S.dev + out_at); }
  E *host(const VsmStage &S) const { return this->in(S.pin_out); }
  void keep(VsmKeep &K, const VsmStage &S, std::vector<E> &vec) const { K.add(vec, host(S), this->n); }
};
static inline hipError_t vsm_no_pre() { return hipSuccess; }
// a mask of the ABI (null: every entry set) as the n bytes 0 or 1 the kernels read
static inline void vsm_mask_bytes(const uint8_t *mask, size_t n, uint8_t *out) {
  for (size_t i = 0; i < n; i++) out[i] = (!mask || mask[i]) ? 1 : 0;
}

// a stats or timings getter: the array of the stage's last result, or zeros where there is none (src null)
template <typename T, size_t N>
static inline void vsm_copy_or_zero(const T (*src)[N], T *out) {
  if (src)
    memcpy(out, *src, sizeof(*src));
  else
    memset(out, 0, sizeof(*src));
}

// What a stage keeps on the handle beside its result's arrays: the staging, whether there is a last result, its NS stats
// and its timings {pack, upload, kernels, download + host}.  A stage's call goes replace(), the round trip, close().  The
// tracks call is the one exception, and no pattern for a further stage: it waits twice, so it has its results' vectors to
// reset where it replaces the last result, ends its packing before it sizes the device block, and reads the events itself.
template <size_t NS>
struct VsmResult {
  VsmStage st;
  bool have = false;
  int64_t stats[NS] = {};
  double timings[4] = {};
  double t1 = 0;  // when the call's packing ended
  // From here on the call replaces the last result: nothing of it is touched before (argument errors and not-ready calls
  // leave it readable).  The packing, which began at t0, ends with the device block and the events in place.
  hipError_t replace(const VsmBlocks &L, hipStream_t stream, double t0) {
    have = false;
    memset(stats, 0, sizeof(stats));
    memset(timings, 0, sizeof(timings));
    const hipError_t rc = st.fit_dev(L, stream);
    t1 = vsm_now_us();
    timings[0] = t1 - t0;
    return rc;
  }
  // the result stands
  void close() {
    timings[1] = st.ms[0] * 1e3;
    timings[2] = st.ms[1] * 1e3;
    timings[3] = std::max(0.0, (vsm_now_us() - t1) - timings[1] - timings[2]);
    have = true;
  }
};
// a stats or timings getter on a stage's last result (null: there is none, and the getter gives zeros)
template <class R, typename T, size_t N, class B>
static inline void vsm_result_get(const R *r, T (B::*arr)[N], T *out) {
  vsm_copy_or_zero(r ? &(r->*arr) : nullptr, out);
}
// a getter's array, where the caller wants it
template <typename E>
static inline void vsm_copy_wanted(const std::vector<E> &v, E *out) {
  if (out && !v.empty()) memcpy(out, v.data(), v.size() * sizeof(E));
}
// the handle is taken apart (the caller has waited for the stream)
template <class R>
static inline void vsm_result_destroy(R *&r) {
  if (r) r->st.release();
  delete r;
  r = nullptr;
}

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
