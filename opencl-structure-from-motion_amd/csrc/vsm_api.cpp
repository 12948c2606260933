// C-ABI of libvisomatch.so (include/visomatch.h): host orchestration of the matcher path.
//
//   vsm_push_back : H2D (or D2D) ingest -> [halve] -> Sobel full / Sobel+blob+corner -> NMS ->
//                   ordered feature emission + descriptors -> bin sort            (all on the GPU)
//   vsm_match     : pass-1 match chain -> export -> host Delaunay support + prior boxes -> H2D ->
//                   pass-2 match chain -> refinement -> export -> host Delaunay support
//   vsm_sequence_run : the same work for a whole sequence with look-ahead: the frames of a chunk
//                   go through every kernel in ONE launch each (grid z/y = image / frame pair) and
//                   the host stages of the chunk's pairs run in parallel on the pool.
//
// A VsmCtx is the device-resident working set for F frame slots and P frame pairs; the streaming
// ring buffer is the (F=2, P=1) instance, sequences use three banks of frame slots and two of pairs (F=6C images, P=2C).
// There is no CPU fallback: without a usable HIP device vsm_create() returns NULL.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <thread>
#include <unordered_map>
#include <vector>

#include "vsm_host.h"
#include "vsm_dc_gpu.h"
#include "vsm_internal.h"
#include "vsm_jobs.h"
#include "vsm_stage.h"
#include "vsm_ctx.h"
#include "vsm_layouts.h"
#include "vsm_tracks.h"
#include "vsm_points.h"
#include "vsm_resect.h"
#include "vsm_locate.h"
#include "vsm_ba.h"
#include "vsm_vet.h"
#include "vsm_motions.h"

#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) {                                                                       \
      fprintf(stderr, "visomatch: HIP error %s at %s:%d (%s)\n", hipGetErrorString(e_), __FILE__, \
              __LINE__, #expr);                                                                   \
      return VSM_EHIP;                                                                            \
    }                                                                                             \
  } while (0)

// CPUs this process may actually use: the cgroup CPU quota (containers), else the hardware
// thread count.  Spinning more threads than the quota only gets the whole process throttled.
static int cpu_budget() {
  unsigned hc = std::thread::hardware_concurrency();
  int budget = hc ? (int)hc : 8;
  if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[64];
    long period = 0;
    if (fscanf(f, "%63s %ld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
      long quota = atol(q);
      if (quota > 0) budget = std::min(budget, (int)std::max(1L, quota / period));
    }
    fclose(f);
  }
  return budget;
}

// VSM_DEBUG_TIMING=1: per-chunk phase times of vsm_sequence_run on stderr (read once)
static bool vsm_debug_timing() {
  static const bool on = getenv("VSM_DEBUG_TIMING") != nullptr;
  return on;
}

static inline double now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---------------------------------------------------------------------------------------
// device working set
// ---------------------------------------------------------------------------------------
// (the dimensions and capacities are its VsmGeom, the tables and host views that the layout binds its VsmCtxViews: vsm_ctx.h)
struct VsmCtx : VsmGeom, VsmCtxViews {
  bool ready = false;
  bool has_heads = false;  // the dense sets carry head records (option match_heads at the time the context was made)
  int nframes = 0, npairs = 0;
  uint8_t *arena = nullptr;
  size_t arena_bytes = 0;
  size_t pair_stride = 0;  // bytes from one pair's buffers (raw, lists, keys ...) to the next pair's
  // pinned host memory; hm_block is host-mapped (the hm_* views)
  uint8_t *hm_block = nullptr;
  float *h_ranges = nullptr;     // pinned [npairs][ranges_stride]
  VsmJob *h_jobs = nullptr;      // pinned [npairs]
  // the context is made for frames of this size and holds this many frame slots and pairs (what else a call compares - its
  // chunk size, the head records - stands at the call)
  bool holds(int32_t w, int32_t h, int frames, int pairs) const { return ready && dims.w == w && dims.h == h && nframes == frames && npairs == pairs; }
};

// ---------------------------------------------------------------------------------------
// Large device blocks are kept, not handed back.  The driver wipes released VRAM in the background - 23 GB/s on this box,
// 44 ms per GB - on a DMA engine the look-ahead path's own copies (keys, early export, host-fed frames) then queue behind:
// for that long every call of the process takes 6.8-7.0 ms instead of 4.0 (tools/hipfree_probe.py; a context re-created for
// another chunk size gave 3 GB back, a closed handle 4 GB - the "slower mode of whole processes" of rounds 3-4, and the
// reason bench.py's later legs ran 10-30 % below the same legs in a process of their own).  So: a released block of
// 8 MB or more waits in a process-wide cache and the next request of its size class (up to 1.5 x) takes it; beyond
// VSM_DEVICE_POOL_MB (default 24 GB, 0 = hand everything back at once) the oldest blocks do go back to the driver.
// ---------------------------------------------------------------------------------------
namespace {
struct DevPool {
  struct Block {
    void *p;
    size_t bytes;
    int device;
  };
  std::mutex mu;
  std::unordered_map<void *, Block> live;  // blocks handed out (8 MB and more only)
  std::vector<Block> cached;               // oldest first
  size_t cached_bytes = 0;
  static constexpr size_t kMin = (size_t)8 << 20;
  static size_t cap() {
    static const size_t v = (size_t)(getenv("VSM_DEVICE_POOL_MB") ? atoll(getenv("VSM_DEVICE_POOL_MB")) : 24 * 1024) << 20;
    return v;
  }
};
DevPool &dev_pool() {
  static DevPool *p = new DevPool();  // (never destroyed: handles may be closed from static destructors)
  return *p;
}
}  // namespace

hipError_t vsm_dev_alloc(void **out, size_t bytes) {
  *out = nullptr;
  if (bytes < DevPool::kMin || DevPool::cap() == 0) return hipMalloc(out, bytes);
  DevPool &P = dev_pool();
  int dev = 0;
  (void)hipGetDevice(&dev);
  {
    std::lock_guard<std::mutex> lk(P.mu);
    size_t best = P.cached.size();
    for (size_t i = 0; i < P.cached.size(); i++) {
      const DevPool::Block &b = P.cached[i];
      if (b.device == dev && b.bytes >= bytes && b.bytes <= bytes + bytes / 2 && (best == P.cached.size() || b.bytes < P.cached[best].bytes)) best = i;
    }
    if (best < P.cached.size()) {
      const DevPool::Block b = P.cached[best];
      P.cached.erase(P.cached.begin() + (long)best);
      P.cached_bytes -= b.bytes;
      P.live[b.p] = b;
      *out = b.p;
      return hipSuccess;
    }
  }
  hipError_t e = hipMalloc(out, bytes);
  if (e != hipSuccess) {  // (the cache may hold what is missing)
    (void)hipGetLastError();
    std::vector<DevPool::Block> drop;
    {
      std::lock_guard<std::mutex> lk(P.mu);
      drop.swap(P.cached);
      P.cached_bytes = 0;
    }
    for (const DevPool::Block &b : drop) (void)hipFree(b.p);
    e = hipMalloc(out, bytes);
    if (e != hipSuccess) return e;
  }
  std::lock_guard<std::mutex> lk(P.mu);
  P.live[*out] = DevPool::Block{*out, bytes, dev};
  return hipSuccess;
}

void vsm_dev_free(void *p) {
  if (!p) return;
  DevPool &P = dev_pool();
  std::vector<DevPool::Block> drop;
  {
    std::lock_guard<std::mutex> lk(P.mu);
    auto it = P.live.find(p);
    if (it == P.live.end()) {
      drop.push_back(DevPool::Block{p, 0, 0});  // (a small block: straight back)
    } else {
      P.cached.push_back(it->second);
      P.cached_bytes += it->second.bytes;
      P.live.erase(it);
      while (P.cached_bytes > DevPool::cap() && !P.cached.empty()) {
        drop.push_back(P.cached.front());
        P.cached_bytes -= P.cached.front().bytes;
        P.cached.erase(P.cached.begin());
      }
    }
  }
  for (const DevPool::Block &b : drop) (void)hipFree(b.p);
}

void vsm_device_pool_stats(int64_t out[3]) {
  DevPool &P = dev_pool();
  std::lock_guard<std::mutex> lk(P.mu);
  out[0] = (int64_t)P.cached.size();
  out[1] = (int64_t)P.cached_bytes;
  out[2] = (int64_t)P.live.size();
}

void vsm_device_pool_trim(void) {
  DevPool &P = dev_pool();
  std::vector<DevPool::Block> drop;
  {
    std::lock_guard<std::mutex> lk(P.mu);
    drop.swap(P.cached);
    P.cached_bytes = 0;
  }
  for (const DevPool::Block &b : drop) (void)hipFree(b.p);
}

static void ctx_destroy(VsmCtx &c) {
  if (c.arena) vsm_dev_free(c.arena);
  if (c.hm_block) (void)hipHostFree(c.hm_block);
  if (c.h_ranges) (void)hipHostFree(c.h_ranges);
  if (c.h_jobs) (void)hipHostFree(c.h_jobs);
  c = VsmCtx();
}

// One arena per context, zero-filled once, so row padding stays 0.
static int ctx_create(VsmCtx &c, const vsm_params &p, int32_t w, int32_t hh, int nframes, int npairs, hipStream_t stream, bool heads) {
  ctx_destroy(c);
  VsmGeom g;
  const int rc = vsm_ctx_geometry(p, w, hh, g);
  if (rc != VSM_OK) return rc;
  const VsmCtxLayout L(g, p, nframes, npairs, heads);
  static_cast<VsmGeom &>(c) = g;
  c.has_heads = heads;
  c.nframes = nframes;
  c.npairs = npairs;
  c.pair_stride = L.pair_stride;
  c.arena_bytes = L.arena.at;
  HIPCHK(vsm_dev_alloc((void **)&c.arena, c.arena_bytes));
  HIPCHK(hipMemsetAsync(c.arena, 0, c.arena_bytes, stream));
  // host-mapped result block: [image counts][list counts][list1, list2 per pair]
  HIPCHK(hipHostMalloc((void **)&c.hm_block, L.hm.at, hipHostMallocMapped));
  memset(c.hm_block, 0, L.hm_zeroed);
  uint8_t *dblock = nullptr;
  HIPCHK(hipHostGetDevicePointer((void **)&dblock, c.hm_block, 0));
  HIPCHK(hipHostMalloc((void **)&c.h_ranges, c.ranges_stride * 4 * npairs, hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void **)&c.h_jobs, sizeof(VsmJob) * npairs, hipHostMallocDefault));
  L.bind(c.arena, c.hm_block, dblock, c);
  {
    // (the tables cross by the copy kernel out of a page-locked twin, like every other host-to-device transfer of the path: a
    // runtime copy of more than 16 KB out of pageable memory that finds the DMA engine busy goes through a shader copy on a
    // hardware queue the runtime creates for it and keeps - DESIGN.md section 6)
    const size_t bi = c.h_imgs.size() * sizeof(VsmImage), bp = c.h_pairs.size() * sizeof(VsmPair);
    uint8_t *twin = nullptr;
    HIPCHK(hipHostMalloc((void **)&twin, al256(bi) + al256(bp), hipHostMallocDefault));
    memcpy(twin, c.h_imgs.data(), bi);
    memcpy(twin + al256(bi), c.h_pairs.data(), bp);
    hipError_t e = vsm_upload(stream, c.d_imgs, twin, bi);
    if (e == hipSuccess) e = vsm_upload(stream, c.d_pairs, twin + al256(bi), bp);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipHostFree(twin);
    HIPCHK(e);
  }
  c.ready = true;
  return VSM_OK;
}

// ---------------------------------------------------------------------------------------
// Measurement / test switches of a handle: read from the environment ONCE, at vsm_create (the calls themselves never
// look at the environment), and settable afterwards through vsm_set_option (bench.py's "alone" pass, tools/).
struct VsmSwitches {
  int seq_v2 = 1;          // VSM_SEQ_V2: 0 = the host-shared look-ahead form
  int seq_chunk = 0;       // VSM_SEQ_CHUNK: frames per look-ahead chunk (0 = by host threads)
  int seq_dc_streams = 3;  // VSM_SEQ_DC_STREAMS: side streams of the GPU-resident form (1..3; with the main and the null stream: five hardware queues)
  int seq_serial = 0;      // VSM_SEQ_SERIAL: nothing overlaps (every kernel's time alone)
  int seq_gpu_sorts = -1;  // VSM_SEQ_GPU_SORTS: percent of a chunk's vertex sorts done on the device (-1 = by host threads)
  int front = 1;           // option "front" (not read from the environment): the fused front end
  int seq_early_export = -1;  // VSM_SEQ_EARLY_EXPORT: the refined lists cross PCIe beside the triangulation, survivor bits follow, the pool
                              // closes the gaps (1); survivors compacted on the device, one DMA copy at the chain's end (0); -1: by pool size
  // settable through vsm_set_option only (tests, tools); none of them is read from the environment:
  int dc_gpu = -1;           // host-shared look-ahead form: the GPU's share of the final stage: -1 = chunks with at least as many pairs as host threads, 0 = never, 1 = always
  int dc_full = -1;          // ... everything after the vertex sort on the GPU: -1 = with six host threads or fewer, 0 / 1
  int dc_fault_inject = 0;   // ... tests: the completion callback of the GPU share is "lost" (dc_wait()'s watchdog has to notice)
  int dc_watchdog_ms = 20000;  // ... how long dc_wait() listens for that callback before it asks the stream itself
  int seq_keys_dma = -1;     // GPU-resident form: the keys reach the host's vertex sort by a DMA copy - 2: on the fifth stream behind an event, so that the chunk's mesh does not stand behind 6-8 MB crossing PCIe (ranks with ten pool threads and more, where the last mesh bounds the call: median step 3.90 -> 3.83 ms); 1: on the chain's own stream (fewer threads: the pool bounds the call and wants its keys first - 4.88 against 5.01 ms with eight threads, 6.71 against 7.14 with four) - or by the key kernel's own stores into host-mapped memory (0); -1: by pool size
  int seq_ties1_null = 1;    // ... the pass-1 chain's vertex sort (one wave per list) on the null stream (1) or on side stream cs[k + 2] (0)
  int seq_keys_pieces = 0;   // ... in this many pieces, an event behind each (the pool starts on the first lists while the others cross); 0: four with ten pool threads and more, else one
  int seq_warm_gaps = 1;     // ... the pool reads the last chunk's exported lists into its L3 caches while it waits for their survivor bits, and a list's gaps are closed by a thread of the domain that read it
  int seq_ties1_host = -1;   // ... the pass-1 lists' vertex sorts on the pool while the device triangulates (1) or on the device, one wave per list (0); -1: by pool size
  int seq_block_after_p2 = 0;  // ... a chunk's block kernel waits for the next chunk's second matching pass
  int seq_last_first = 1;    // ... a chain's sort + kd order kernel goes in with its head, and the block kernel of the last chunk but one waits for the last chunk's
  int seq_first_chunk = 0;   // ... frames of the call's first chunk (0: like the others)
  int seq_p2_first = -1;     // ... a chunk's second pass in front of the features of chunk k + 2 (the order host-resident inputs get): -1 = by pool size
  int seq_export_budget = 2; // ... pieces of the early export submitted behind a chunk's keys where the next chunk's keys follow at once (Seq2Call::export_some)
  int seq_null_stream = 1;   // ... its fifth stream (early exports, the device's vertex sorts) is the process's null stream (1) or a non-blocking stream of
                             // the library's own (0: for applications that keep work of their own on the null stream - INTEGRATION.md)
  int seq_host_inorder = 1;  // ... host-resident inputs: chunk by chunk in the order of arrival - the caller's thread waits for a chunk's feature counts only when everything of the chunk in front is enqueued (0: the run-ahead order of HBM-resident inputs)
  int seq_defer_refine = 0;  // ... a chunk's refinement behind the NEXT chunk's second-pass matching where that follows at once (the chain's keys do not need it)
  int seq_host_pinned = 0;   // ... host-resident input images are in page-locked memory (the caller's promise): DMA straight out of them, no gather pass
  int match_heads = 0;       // the second matching pass takes a bin's start and its first 15 candidates' coordinates from one 64-byte head record (k_feat_heads) instead of bin starts + coordinate runs: measured slower, off; read when a context is made
  int fused_features = 1;    // filters + suppression of the matching resolution out of one LDS tile (k_feat_dense / k_feat_sparse; default radii) or the separate kernels (0)
  int feat_order = 1;        // feature records + bin-sorted copy by k_feat_scan / k_feat_order (tiles of whole search bins) or by k_scan_cells / k_emit / k_bin_* (0)
  int multi_host_pass1 = -1; // vsm_multi_process: the first-pass lists' removeOutliers + prior boxes on the host pool (1) or by the device chain (0); -1: host for K <= pool threads
  int multi_shared_ego = 0;  // vsm_multi_process: idle pool threads take RANSAC hypotheses of the sequences' egomotion (1: measured, no gain), every sequence on one thread (0)
  int pairs_chunk = 0;       // vsm_pairs_run: pairs per step (0 = the look-ahead call's chunk rule for device-resident frames, seq2_plan)
  int motions_chunk = 0;     // vsm_motions_run / vsm_pairs_motions: pairs per chunk (0 = as many as the memory rule of vsm_motions.inc allows)
  int frame_early_xy = 1;    // per-frame path: the pass-2 list's pixels cross in front of the list, the host triangulates while the refinement and the export run (vsm_match)
  int fused_keys = 1;        // VSM_FUSED_KEYS: the batched forms' compactions write the Delaunay chains' keys with the lists and the chains' job tables are uploaded ahead of the
                             // matching launch (1), or every chain starts with
                             // its job table's upload and k_dc2_keys behind the compaction (0); refinement = 2 always takes 0
  int fuse_compact = -1;     // vsm_fuse_run / vsm_points_fuse: the search once, its proposals kept in places per track and compacted behind the scan (1), the search twice, counting and then listing (0), or the first where the places fit FU_PLACES_MAX (-1; profiles/README.md)
  int adjust_fixed = 0;      // vsm_adjust_run / vsm_points_adjust: every launch of max_rounds rounds enqueued at once (1) or a wait per round on the control block (0; profiles/README.md)
  int filter_planes = 0;     // vsm_push_back keeps f1 / f2 in HBM for vsm_get_filter_responses (the fused tiles write them on the side)
  static int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
  }
  void from_environment() {
    seq_v2 = env_int("VSM_SEQ_V2", 1) != 0;
    seq_chunk = std::max(0, env_int("VSM_SEQ_CHUNK", 0));
    seq_dc_streams = std::min(3, std::max(1, env_int("VSM_SEQ_DC_STREAMS", 3)));
    seq_serial = env_int("VSM_SEQ_SERIAL", 0) != 0;
    seq_gpu_sorts = env_int("VSM_SEQ_GPU_SORTS", -1);
    seq_early_export = env_int("VSM_SEQ_EARLY_EXPORT", -1);
    multi_host_pass1 = env_int("VSM_MULTI_HOST_PASS1", -1);    // (measurements: vsm_multi_create takes no options)
    multi_shared_ego = env_int("VSM_MULTI_SHARED_EGO", 0);
    fused_keys = env_int("VSM_FUSED_KEYS", 1) != 0;  // (likewise)
  }
  bool set(const char *name, int v) {
    if (!strcmp(name, "seq_v2")) seq_v2 = v != 0;
    else if (!strcmp(name, "seq_chunk")) seq_chunk = std::max(0, v);
    else if (!strcmp(name, "seq_dc_streams")) seq_dc_streams = std::min(3, std::max(1, v));
    else if (!strcmp(name, "seq_serial")) seq_serial = v != 0;
    else if (!strcmp(name, "seq_gpu_sorts")) seq_gpu_sorts = v;
    else if (!strcmp(name, "front")) front = v != 0;
    else if (!strcmp(name, "seq_early_export")) seq_early_export = v;
    else if (!strcmp(name, "dc_gpu")) dc_gpu = v;
    else if (!strcmp(name, "dc_full")) dc_full = v;
    else if (!strcmp(name, "dc_fault_inject")) dc_fault_inject = v;
    else if (!strcmp(name, "dc_watchdog_ms")) dc_watchdog_ms = std::max(1, v);
    else if (!strcmp(name, "seq_keys_dma")) seq_keys_dma = v;
    else if (!strcmp(name, "seq_export_budget")) seq_export_budget = v;
    else if (!strcmp(name, "seq_first_chunk")) seq_first_chunk = std::max(0, v);
    else if (!strcmp(name, "seq_p2_first")) seq_p2_first = v;
    else if (!strcmp(name, "seq_last_first")) seq_last_first = v != 0;
    else if (!strcmp(name, "seq_keys_pieces")) seq_keys_pieces = v;
    else if (!strcmp(name, "seq_block_after_p2")) seq_block_after_p2 = v != 0;
    else if (!strcmp(name, "seq_ties1_host")) seq_ties1_host = v;
    else if (!strcmp(name, "seq_warm_gaps")) seq_warm_gaps = v != 0;
    else if (!strcmp(name, "seq_ties1_null")) seq_ties1_null = v != 0;
    else if (!strcmp(name, "seq_null_stream")) seq_null_stream = v != 0;
    else if (!strcmp(name, "seq_host_pinned")) seq_host_pinned = v != 0;
    else if (!strcmp(name, "seq_defer_refine")) seq_defer_refine = v != 0;
    else if (!strcmp(name, "seq_host_inorder")) seq_host_inorder = v != 0;
    else if (!strcmp(name, "match_heads")) match_heads = v != 0;
    else if (!strcmp(name, "fused_features")) fused_features = v != 0;
    else if (!strcmp(name, "filter_planes")) filter_planes = v != 0;
    else if (!strcmp(name, "fused_keys")) fused_keys = v != 0;
    else if (!strcmp(name, "feat_order")) feat_order = v != 0;
    else if (!strcmp(name, "frame_early_xy")) frame_early_xy = v != 0;
    else if (!strcmp(name, "multi_host_pass1")) multi_host_pass1 = v;
    else if (!strcmp(name, "multi_shared_ego")) multi_shared_ego = v;
    else if (!strcmp(name, "pairs_chunk")) pairs_chunk = std::max(0, v);
    else if (!strcmp(name, "motions_chunk")) motions_chunk = std::max(0, v);
    else if (!strcmp(name, "adjust_fixed")) adjust_fixed = v != 0;
    else if (!strcmp(name, "fuse_compact")) fuse_compact = v;
    else return false;
    return true;
  }
};

struct vsm_handle {
  vsm_params param;  // match_radius already halved for half_resolution (viso/matcher.cpp:59-60)
  void *aff = nullptr;  // CPU record of the handle's device (vsm_host.h): where the threads created for this handle confine themselves
  VsmSwitches sw;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t input_ev = nullptr;   // vsm_wait_for_stream(): the producer stream's marker
  hipEvent_t idle_wait = nullptr;  // blocking-sync event (pass 2 of a chunk done): the look-ahead caller sleeps on it, its CPU goes to the host pool
  hipEvent_t seq_ev[2] = {nullptr, nullptr};  // look-ahead markers: features done / pass 1 done (blocking sync too)
  static constexpr int kDcBanks = 4;  // chunks whose final stage may be in flight at once
  struct DcBank *dc_bank[kDcBanks] = {nullptr, nullptr, nullptr, nullptr};  // look-ahead: GPU share of the exact Delaunay
  hipStream_t dc_stream[2] = {nullptr, nullptr};  // alternate per chunk: one chunk's records travel while the next one's kernels run
  std::vector<VsmHostWork> seq_work;               // per pair of every Delaunay bank: state between the two host halves
  VsmCtx ring;  // streaming ring buffer: 2 frame slots, 1 pair
  VsmCtx seq;   // look-ahead sequences: 3 banks of C frame slots, 2 banks of C pairs
  int seq_chunk = 0;

  // ring buffer state (Matcher's prev/curr pointers, viso/matcher.cpp:108-155)
  int cur = 0;
  bool have[2] = {false, false};   // frame slot holds a left image
  bool right[2] = {false, false};  // ... and a right image
  int32_t n_feat[2][2][2] = {};    // [slot][side][set]
  int32_t dims_p[3] = {0, 0, 0}, dims_c[3] = {0, 0, 0};
  bool f_valid = false;            // f1/f2 hold the responses of the current left image
  bool counts_pending = false;     // an asynchronous push is in flight
  int pending_slot = 0, pending_imgs = 0;

  // results of the streaming API
  std::vector<vsm_p_match> stage[5];
  std::vector<vsm_p_match> matched;
  std::vector<float> ranges;
  std::vector<int32_t> pf;
  int capture_stage2 = 0;
  bool stage3_in_hm = false;     // stage 3 is the ring's host-mapped pass-2 list as exported (vsm_stage_get)
  uint32_t *xy_host = nullptr, *xy_dev = nullptr;  // the pass-2 list's pixels, x | y << 16, host-mapped (vsm_match: early_xy)
  size_t xy_cap = 0;
  hipEvent_t xy_ev = nullptr, done_ev = nullptr, push_ev = nullptr;
  bool push_ev_set = false;      // push_ev is recorded behind the pending push (settle)
  VsmHostWork work;
  int64_t counters[5] = {0, 0, 0, 0, 0};
  double timings[5] = {0, 0, 0, 0, 0};
  std::vector<uint8_t> gainI[2];
  // results of the sequence API
  std::vector<std::vector<vsm_p_match>> seq_matches;
  // ... or, per frame, a view of 48-byte records that the device wrote straight into the host-mapped result arena (the
  // GPU-resident look-ahead form on hosts with few threads: no host copy inside the call at all)
  struct SeqView {
    const vsm_p_match *p = nullptr;
    int32_t n = 0;
  };
  std::vector<SeqView> seq_view;
  // per frame of the last look-ahead call: the frame whose list getMatches() shows after it - the frame itself where
  // matchFeatures ran, else the last one before it where it did (the reference returns early without touching p_matched,
  // viso/matcher.cpp:184-203), -1: none yet.  The batched forms fill it; the frame-by-frame form copies the lists themselves.
  std::vector<int32_t> seq_src;
  double seq_timings[4] = {0, 0, 0, 0};
  bool dc_gpu_broken = false;    // a Delaunay stream reported a HIP error once: the host-shared form keeps off the GPU share from then on
  std::atomic<int> seq_hip_error{0};  // set by a chunk whose GPU share failed during the current vsm_sequence_run
  struct Seq2 *seq2 = nullptr;   // GPU-resident look-ahead path (vsm_seq2.inc): streams, slabs, result arena
  int32_t seq_v2_frames = 0;     // > 0: the last sequence's results are in seq2's arena, not in seq_matches
  struct VsmPairs *pairs = nullptr;  // arbitrary frame pairs in one call (vsm_pairs.inc): its own context, banks and result lists
  struct VsmPoints *points = nullptr;  // track triangulation (vsm_points.inc): staging, device block, last result
  struct VsmResect *resect = nullptr;  // pose refinement against the points (vsm_resect.inc): staging, device block, last result
  struct VsmVet *vet = nullptr;        // vetting of observations (vsm_vet.inc): staging, device block, last result
  struct VsmAdjust *adjust = nullptr;  // joint adjustment of poses and points (vsm_ba.inc): staging, device block, last result
  struct VsmLocate *locate = nullptr;  // location of frames against the points (vsm_locate.inc): staging, device block, last result
  struct VsmReobserve *reobserve = nullptr;  // re-observation of the points (vsm_reobserve.inc): staging, device blocks, last result
  struct VsmFuse *fuse = nullptr;            // fusion of duplicate tracks (vsm_fuse.inc): staging, device blocks, last result
  struct VsmMotions *motions = nullptr;  // monocular pair motions (vsm_motions_api.inc): staging, device block, last result
  struct VsmTracks *tracks = nullptr;  // feature tracks from pair match lists (vsm_tracks.inc): staging, device block, last result

  uint8_t *stage_host = nullptr;  // pinned staging for host images
  size_t stage_bytes = 0;
  // look-ahead calls fed from host memory: two pinned slots a chunk's images are gathered into (by the pool, in parallel)
  // and their device twins; an event per slot says when its upload has been consumed
  uint8_t *seq_stage_h[2] = {nullptr, nullptr}, *seq_stage_d[2] = {nullptr, nullptr};
  size_t seq_stage_bytes = 0;
  hipEvent_t seq_stage_ev[2] = {nullptr, nullptr};
  int seq_stage_next = 0;
  VsmProf prof;
  VsmPool *pool = nullptr;
  VsmForkJoin *fj = nullptr;
};

// Matcher::range records (u_min[4], u_max[4], v_min[4], v_max[4], viso/matcher.h:152-157) go to the
// device stage-major -- {u_min, u_max, v_min, v_max} of stage 0, then stage 1, ... -- so that a chain
// fetches the box of one stage with a single 16-byte load
static void ranges_to_device_layout(float *dst, const float *src, size_t n_floats) {
  for (size_t b = 0; b + 16 <= n_floats; b += 16)
    for (int stage = 0; stage < 4; stage++)
      for (int k = 0; k < 4; k++) dst[b + stage * 4 + k] = src[b + k * 4 + stage];
}

VsmPool *vsm_pool_of(vsm_handle *h) { return h->pool; }
VsmForkJoin *vsm_forkjoin_of(vsm_handle *h) { return h->fj; }
double vsm_now_us() { return now_us(); }
static void seq1_destroy(vsm_handle *h);  // vsm_seq1.inc
static void seq2_destroy(vsm_handle *h);  // vsm_seq2.inc
static void pairs_destroy(vsm_handle *h);  // vsm_pairs.inc
static void tracks_destroy(vsm_handle *h);  // vsm_tracks.inc
static void points_destroy(vsm_handle *h);  // vsm_points.inc
static void resect_destroy(vsm_handle *h);  // vsm_resect.inc
static void vet_destroy(vsm_handle *h);     // vsm_vet.inc
static void adjust_destroy(vsm_handle *h);  // vsm_ba.inc
static void locate_destroy(vsm_handle *h);  // vsm_locate.inc
static void reobserve_destroy(vsm_handle *h);  // vsm_reobserve.inc
static void fuse_destroy(vsm_handle *h);       // vsm_fuse.inc
static void motions_destroy(vsm_handle *h);  // vsm_motions_api.inc

extern "C" {

const char *vsm_version(void) { return "visomatch 0.3 (gfx950)"; }

void vsm_default_params(vsm_params *p) {
  memset(p, 0, sizeof(*p));
  p->nms_n = 3;
  p->nms_tau = 50;
  p->match_binsize = 50;
  p->match_radius = 200;
  p->match_disp_tolerance = 2;
  p->outlier_disp_tolerance = 5;
  p->outlier_flow_tolerance = 5;
  p->multi_stage = 1;
  p->half_resolution = 1;
  p->refinement = 1;
}

vsm_handle *vsm_create(const vsm_params *p) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    fprintf(stderr, "visomatch: no HIP device available (this library has no CPU path)\n");
    return nullptr;
  }
  vsm_handle *h = new vsm_handle();
  h->param = *p;
  if (p->half_resolution) h->param.match_radius /= 2;
  h->sw.from_environment();
  {
    int dev = 0;
    char bdf[64] = {0};
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf), dev) == hipSuccess)
      vsm_affinity_from_device(bdf);  // (before the pools start their threads)
    h->aff = vsm_affinity_current();
    vsm_forkjoin_domain_hint(dev);  // (the fork-join workers' L3 domain: a domain per device of the socket)
  }
  {
    // host threads (the caller's thread included): VSM_HOST_THREADS frame-parallel workers for
    // the look-ahead API, at most 8 of them for the sub-problems of one triangulation (streaming)
    int nt = 16;
    if (const char *e = getenv("VSM_HOST_THREADS")) nt = atoi(e);
    nt = std::max(1, std::min(nt, cpu_budget()));
    // (the look-ahead caller sleeps in a blocking event wait while the GPU works, so all nt budgeted
    // CPUs go to pool workers: nt workers + the caller's thread)
    h->pool = new VsmPool(nt + 1);
    int fjt = nt < 8 ? nt : 8;
    if (const char *e = getenv("VSM_FJ_THREADS")) fjt = std::max(1, std::min(atoi(e), nt));  // (measurements: the fork-join pool of the per-frame path's Delaunay)
    h->fj = new VsmForkJoin(fjt);
    h->work.pool = h->fj;
    h->work.async = h->pool;
  }
  // k_dc_subtrees (vsm_dc.hip) recurses a few levels deep: make sure every thread has the stack for it
  {
    size_t cur = 0;
    if (hipDeviceGetLimit(&cur, hipLimitStackSize) == hipSuccess && cur < 4096) (void)hipDeviceSetLimit(hipLimitStackSize, 4096);
  }
  if (hipGetDevice(&h->device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&h->idle_wait, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->seq_ev[0], hipEventBlockingSync | hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->seq_ev[1], hipEventBlockingSync | hipEventDisableTiming) != hipSuccess) {
    fprintf(stderr, "visomatch: HIP initialisation failed: %s\n", hipGetErrorString(hipGetLastError()));
    delete h->pool;
    delete h->fj;
    delete h;
    return nullptr;
  }
  return h;
}

static void reset_ring_state(vsm_handle *h) {
  if (h->stage3_in_hm && h->ring.hm_lcount && !h->ring.hm_list2.empty()) {  // the ring's host-mapped block is about to go: stage 3 moves out of it
    const int32_t n = std::max(h->ring.hm_lcount[1], 0);
    h->stage[3].assign(h->ring.hm_list2[0], h->ring.hm_list2[0] + n);
  }
  h->stage3_in_hm = false;
  h->have[0] = h->have[1] = h->right[0] = h->right[1] = false;
  h->f_valid = false;
  h->counts_pending = false;
  h->push_ev_set = false;
  memset(h->n_feat, 0, sizeof(h->n_feat));
}

void vsm_destroy(vsm_handle *h) {
  if (!h) return;
  (void)hipStreamSynchronize(h->stream);
  for (hipStream_t st : h->dc_stream)
    if (st) (void)hipStreamSynchronize(st);
  seq2_destroy(h);
  pairs_destroy(h);
  tracks_destroy(h);
  points_destroy(h);
  resect_destroy(h);
  vet_destroy(h);
  adjust_destroy(h);
  locate_destroy(h);
  reobserve_destroy(h);
  fuse_destroy(h);
  motions_destroy(h);
  ctx_destroy(h->ring);
  ctx_destroy(h->seq);
  if (h->stage_host) (void)hipHostFree(h->stage_host);
  if (h->xy_host) (void)hipHostFree(h->xy_host);
  if (h->xy_ev) (void)hipEventDestroy(h->xy_ev);
  if (h->done_ev) (void)hipEventDestroy(h->done_ev);
  if (h->push_ev) (void)hipEventDestroy(h->push_ev);
  for (int k = 0; k < 2; k++) {
    if (h->seq_stage_h[k]) (void)hipHostFree(h->seq_stage_h[k]);
    if (h->seq_stage_d[k]) vsm_dev_free(h->seq_stage_d[k]);
    if (h->seq_stage_ev[k]) (void)hipEventDestroy(h->seq_stage_ev[k]);
  }
  seq1_destroy(h);
  for (hipStream_t st : h->dc_stream)
    if (st) (void)hipStreamDestroy(st);
  if (h->idle_wait) (void)hipEventDestroy(h->idle_wait);
  if (h->input_ev) (void)hipEventDestroy(h->input_ev);
  for (hipEvent_t e : h->seq_ev)
    if (e) (void)hipEventDestroy(e);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h->pool;
  delete h->fj;
  delete h;
}

void vsm_set_intrinsics(vsm_handle *h, double f, double cu, double cv, double base) {
  h->param.f = f;
  h->param.cu = cu;
  h->param.cv = cv;
  h->param.base = base;
}

// completes an asynchronous push: waits for the stream and takes the feature counts the
// kernels wrote into host-mapped memory
static int settle(vsm_handle *h) {
  if (!h->counts_pending) return VSM_OK;
  if (h->push_ev_set)
    HIPCHK(hipEventSynchronize(h->push_ev));  // (recorded behind the push's last kernel: cheaper to wait for than the stream)
  else
    HIPCHK(hipStreamSynchronize(h->stream));
  h->push_ev_set = false;
  HIPCHK(hipGetLastError());
  h->prof.resolve();
  const int slot = h->pending_slot;
  memset(h->n_feat[slot], 0, sizeof(h->n_feat[slot]));
  for (int k = 0; k < h->pending_imgs; k++)
    for (int s2 = 0; s2 < 2; s2++) h->n_feat[slot][k][s2] = h->ring.hm_counts[(slot * 2 + k) * 2 + s2];
  h->counts_pending = false;
  return VSM_OK;
}

// ---------------------------------------------------------------------------------------
// Steps that the per-frame path and the batched forms (vsm_seq1.inc, vsm_seq2.inc, vsm_multi.inc) share
// ---------------------------------------------------------------------------------------
// the fused front end (k_front) instead of the three separate passes - ingest, halving, full-resolution Sobel (option "front" = 0)
static bool fused_front(const vsm_handle *h) { return h->param.half_resolution && h->sw.front; }

// One front-end step on the handle's stream: `frames` frames from s0 - and their right images from s1, if there are any -,
// a frame every `stride` bytes in rows of `pitch` bytes, into images first, first + 1, ... of the context.  write_img: the
// fused front end also writes the padded copy of the source (the separate ingest pass always does).
static void enqueue_front(vsm_handle *h, VsmCtx &c, int first, const uint8_t *s0, const uint8_t *s1, size_t stride, int pitch, int frames,
                          int write_img) {
  if (frames <= 0) return;
  if (fused_front(h))
    vsm_launch_front(h->stream, h->prof, c.d_imgs, first, s0, s1, stride, pitch, frames, c.dims, write_img);
  else
    vsm_launch_ingest(h->stream, h->prof, c.d_imgs, first, s0, s1, stride, pitch, frames, c.dims);
}
// n frames of a batched form from s0, a frame every `step` bytes; sides == 2: their right images from s1, every `stride2` bytes.
// The front kernels number their images first + 2 * frame + side: consecutive mono frames go through as (even, odd) pairs,
// an odd last one alone.
static void enqueue_front_frames(vsm_handle *h, VsmCtx &c, int first_img, int sides, const uint8_t *s0, size_t step, const uint8_t *s1,
                                 size_t stride2, int pitch, int n) {
  if (sides == 2) {
    enqueue_front(h, c, first_img, s0, s1, stride2, pitch, n, 0);
  } else {
    enqueue_front(h, c, first_img, s0, s0 + step, 2 * step, pitch, n / 2, 0);
    if (n & 1) enqueue_front(h, c, first_img + n - 1, s0 + step * (size_t)(n - 1), nullptr, step, pitch, 1, 0);
  }
}
// every feature kernel over images first .. first + n_img - 1 (behind their front-end step); `extra`: further bits of the
// launcher's option mask (vsm_internal.h).  Returns what vsm_launch_features returns.
static int enqueue_features(vsm_handle *h, VsmCtx &c, int first, int n_img, int extra = 0) {
  const vsm_params &p = h->param;
  return vsm_launch_features(h->stream, h->prof, c.d_imgs, first, n_img, c.dims, c.f1, c.f2, c.f_stride, p.nms_tau, p.multi_stage,
                             p.half_resolution, p.match_binsize, c.h_imgs.data(), fused_front(h) ? 1 : 0,
                             (h->sw.fused_features ? 1 : 0) | (h->sw.feat_order ? 0 : 4) | extra);
}

static int push_common(vsm_handle *h, const uint8_t *I1, const uint8_t *I2, int32_t w, int32_t hh, int32_t bpl,
                       int replace, bool on_device) {
  if (w <= 0 || hh <= 0 || bpl < w || I1 == nullptr) {
    fprintf(stderr, "ERROR: Image dimension mismatch!\n");  // viso/matcher.cpp:103-106
    return VSM_EDIMS;
  }
  HIPCHK(hipSetDevice(h->device));
  VsmCtx &c = h->ring;
  if (!c.holds(w, hh, 2, 1)) {
    // a change of image size restarts the ring buffer (the reference would match across sizes)
    (void)hipStreamSynchronize(h->stream);
    reset_ring_state(h);
    int rc = ctx_create(c, h->param, w, hh, 2, 1, h->stream, h->sw.match_heads != 0);
    if (rc != VSM_OK) return rc;
  }
  if (h->counts_pending) {  // a previous asynchronous push has not been settled yet
    int rc = settle(h);
    if (rc != VSM_OK) return rc;
  }
  if (!replace) {  // viso/matcher.cpp:123-155: curr becomes prev
    h->cur ^= 1;
    memcpy(h->dims_p, h->dims_c, sizeof(h->dims_p));
  }
  const int slot = h->cur;
  h->dims_c[0] = w;
  h->dims_c[1] = hh;
  h->dims_c[2] = c.dims.bpl;
  const int n_img = I2 ? 2 : 1;
  if (on_device) {
    enqueue_front(h, c, slot * 2, I1, I2, 0, bpl, 1, 1);
  } else {
    // Host images: rows go through our own pinned, pre-padded staging buffer (a pageable 2-D copy
    // is staged row by row by the runtime and costs milliseconds).  The caller's buffer is free as
    // soon as the memcpy below returns; the staging buffer is reused only after settle().
    const size_t plane = (size_t)c.dims.bpl * hh;
    if (h->stage_bytes < 2 * plane) {
      if (h->stage_host) (void)hipHostFree(h->stage_host);
      HIPCHK(hipHostMalloc((void **)&h->stage_host, 2 * plane, hipHostMallocDefault));
      memset(h->stage_host, 0, 2 * plane);  // pad columns stay 0
      h->stage_bytes = 2 * plane;
    }
    const uint8_t *srcs[2] = {I1, I2};
    for (int k = 0; k < n_img; k++) {
      uint8_t *st = h->stage_host + k * plane;
      // only the w image bytes of a row are taken; pad bytes are 0 by definition
      for (int32_t v = 0; v < hh; v++) memcpy(st + (size_t)v * c.dims.bpl, srcs[k] + (size_t)v * bpl, w);
      HIPCHK(hipMemcpyAsync(c.h_imgs[slot * 2 + k].img, st, plane, hipMemcpyHostToDevice, h->stream));
    }
    // (the padded copies are in place: they are the fused front end's source)
    if (fused_front(h)) enqueue_front(h, c, slot * 2, c.h_imgs[slot * 2].img, I2 ? c.h_imgs[slot * 2 + 1].img : nullptr, 0, c.dims.bpl, 1, 0);
  }
  const int f_planes = enqueue_features(h, c, slot * 2, n_img, h->sw.filter_planes ? 2 : 0);
  HIPCHK(hipGetLastError());
  if (!h->push_ev) HIPCHK(hipEventCreateWithFlags(&h->push_ev, hipEventDisableTiming));
  HIPCHK(hipEventRecord(h->push_ev, h->stream));
  h->push_ev_set = true;
  h->have[slot] = true;
  h->right[slot] = (I2 != nullptr);
  h->pending_slot = slot;
  h->pending_imgs = n_img;
  h->counts_pending = true;
  h->f_valid = f_planes != 0;
  h->gainI[0].clear();
  h->gainI[1].clear();
  // Host images were copied into the staging buffer, so the caller may free or overwrite them as
  // soon as we return (matcherMex does).  Device-resident images: the source must stay valid until
  // the next call that needs the push's results settles it.  Either way the push is asynchronous.
  return VSM_OK;
}

int vsm_wait_for_stream(vsm_handle *h, void *hip_stream) {
  HIPCHK(hipSetDevice(h->device));
  if (!h->input_ev) HIPCHK(hipEventCreateWithFlags(&h->input_ev, hipEventDisableTiming));
  HIPCHK(hipEventRecord(h->input_ev, (hipStream_t)hip_stream));
  HIPCHK(hipStreamWaitEvent(h->stream, h->input_ev, 0));
  return VSM_OK;
}

int vsm_push_back(vsm_handle *h, const uint8_t *I1, const uint8_t *I2, int32_t w, int32_t hh, int32_t bpl, int replace) {
  return push_common(h, I1, I2, w, hh, bpl, replace, false);
}

int vsm_push_back_device(vsm_handle *h, const uint8_t *dI1, const uint8_t *dI2, int32_t w, int32_t hh, int32_t bpl,
                         int replace) {
  return push_common(h, dI1, dI2, w, hh, bpl, replace, true);
}

// a job with the ring's image slots: the previous frame's and the current one's left image (stereo matching only needs the
// current pair: "prev" then aliases the current slot)
static VsmJob ring_job(const vsm_handle *h, int method) {
  VsmJob jb;
  vsm_job_slots(jb, (method == 1 ? h->cur : h->cur ^ 1) * 2, h->cur * 2);
  return jb;
}

// The pass-1 host stage of n pairs, first_pair onwards, on the pool (viso/matcher.cpp:222-226): a pair's pass-1 list out of
// host-mapped memory (none for a pair that is not valid), removeOutliers, computePriorStatistics, the boxes in the device's
// layout; then the boxes' upload on the handle's stream.  task_ns (may be NULL): the two steps' task time is added to
// task_ns[0] and task_ns[1].
static hipError_t host_pass1_boxes(vsm_handle *h, VsmCtx &c, int first_pair, int n, const char *valid, int method, const int32_t dims_c[3],
                                   std::atomic<long long> *task_ns = nullptr) {
  const vsm_params &p = h->param;
  h->pool->run(n, [&](int i) {
    static thread_local VsmHostWork tw;
    static thread_local std::vector<float> rg;
    static thread_local std::vector<vsm_p_match> m1;
    const int pj = first_pair + i;
    const double t0 = now_us();
    m1.clear();
    if (valid[i]) m1.assign(c.hm_list1[pj], c.hm_list1[pj] + std::max(c.hm_lcount[2 * pj], 0));
    vsm_host_remove_outliers(tw, p, m1, method);
    const double t1 = now_us();
    vsm_host_prior_statistics(p, dims_c, m1, method, rg);
    ranges_to_device_layout(c.h_ranges + (size_t)pj * c.ranges_stride, rg.data(), rg.size());
    if (task_ns) {
      task_ns[0].fetch_add((long long)((t1 - t0) * 1e3), std::memory_order_relaxed);
      task_ns[1].fetch_add((long long)((now_us() - t1) * 1e3), std::memory_order_relaxed);
    }
  });
  return vsm_upload(h->stream, c.d_ranges + (size_t)first_pair * c.ranges_stride, c.h_ranges + (size_t)first_pair * c.ranges_stride,
                    c.ranges_stride * 4 * n);
}

int vsm_match(vsm_handle *h, int32_t method, const double *Tr) {
  VsmCtx &c = h->ring;
  if (!c.ready) return VSM_ENOTREADY;
  HIPCHK(hipSetDevice(h->device));
  {
    int rc = settle(h);
    if (rc != VSM_OK) return rc;
  }
  const vsm_params &p = h->param;
  const int sc = h->cur, sp = h->cur ^ 1;
  int32_t n[4][2];
  for (int s = 0; s < 2; s++) {
    n[0][s] = h->have[sp] ? h->n_feat[sp][0][s] : 0;
    n[1][s] = h->have[sp] ? h->n_feat[sp][1][s] : 0;
    n[2][s] = h->have[sc] ? h->n_feat[sc][0][s] : 0;
    n[3][s] = h->have[sc] ? h->n_feat[sc][1][s] : 0;
  }
  VsmJob job = ring_job(h, method);
  if (!vsm_job_fill(p, method, n, job.img_prev, job.img_curr, Tr, job, nullptr)) return VSM_ENOTREADY;
  const double t0 = now_us();
  for (int s = 0; s < 5; s++) h->stage[s].clear();
  h->matched.clear();
  memset(h->counters, 0, sizeof(h->counters));

  VsmMatchCfg cfg = make_cfg(p, method, h->sw.match_heads && c.has_heads);
  const int stages = method == 2 ? 4 : 2;
  const VsmDims dp = c.dims, dc = c.dims;  // one size per handle

  double t1 = t0, t2 = t0;
  if (p.multi_stage) {
    cfg.sparse = 1;
    cfg.use_prior = 0;
    if (!vsm_launch_match(h->stream, h->prof, c.d_imgs, c.d_pairs, nullptr, job, 1, c.dims, cfg, job.nq[0], 1))
      vsm_launch_export(h->stream, h->prof, c.d_pairs, 1, 0, job.nq[0]);
    if (!h->done_ev) HIPCHK(hipEventCreateWithFlags(&h->done_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(h->done_ev, h->stream));
    HIPCHK(hipEventSynchronize(h->done_ev));  // the list was written into host-mapped memory
    h->stage[0].assign(c.hm_list1[0], c.hm_list1[0] + c.hm_lcount[0]);
    h->counters[0] += (int64_t)job.nq[0] * stages;
    t1 = now_us();
    h->stage[1] = h->stage[0];
    vsm_host_remove_outliers(h->work, p, h->stage[1], method);
    const double ta = now_us();
    vsm_host_prior_statistics(p, h->dims_c, h->stage[1], method, h->ranges);
    const double tb = now_us();
    ranges_to_device_layout(c.h_ranges, h->ranges.data(), h->ranges.size());
    HIPCHK(vsm_upload(h->stream, c.d_ranges, c.h_ranges, h->ranges.size() * sizeof(float)));
    t2 = now_us();
    if (vsm_debug_timing()) {
      static double acc[3] = {0, 0, 0};
      static long calls = 0;
      acc[0] += ta - t1;
      acc[1] += tb - ta;
      acc[2] += t2 - tb;
      if (++calls % 100 == 0)
        fprintf(stderr, "  vsm_match pass-1 host stage, mean us: removeOutliers %.1f, prior statistics %.1f, boxes' upload %.1f (lists of %zu)\n",
                acc[0] / calls, acc[1] / calls, acc[2] / calls, h->stage[0].size());
    }
  }
  cfg.sparse = 0;
  cfg.use_prior = p.multi_stage ? 1 : 0;
  const int nq2 = job.nq[1];
  h->counters[0] += (int64_t)nq2 * stages;
  // The final removeOutliers' triangulation only needs the list's pixels (u1c, v1c), and those are final once the list is
  // compacted (the refinement moves the other three points, viso/matcher.cpp:1544-1577): they cross first, 4 bytes per
  // match, and the host triangulates while the refinement, the list's export and its 350 KB over PCIe are under way; the
  // support test then reads flow and disparity from the refined list.  (Not with refinement = 2, whose fits drop matches,
  // nor when the unrefined list is wanted as a stage view.)
  const bool early_xy = h->sw.frame_early_xy && p.refinement != 2 && !h->capture_stage2 && nq2 > 0;
  h->stage3_in_hm = false;
  if (early_xy) {
    if (h->xy_cap < (size_t)nq2) {
      if (h->xy_host) (void)hipHostFree(h->xy_host);
      h->xy_host = nullptr;
      h->xy_cap = 0;
      const size_t cap = ((size_t)nq2 + 4095) / 4096 * 4096;
      HIPCHK(hipHostMalloc((void **)&h->xy_host, cap * sizeof(uint32_t), hipHostMallocMapped));
      HIPCHK(hipHostGetDevicePointer((void **)&h->xy_dev, h->xy_host, 0));
      h->xy_cap = cap;
    }
    if (!h->xy_ev) HIPCHK(hipEventCreateWithFlags(&h->xy_ev, hipEventDisableTiming));
    if (!vsm_launch_match(h->stream, h->prof, c.d_imgs, c.d_pairs, nullptr, job, 1, c.dims, cfg, nq2, 2, h->xy_dev))
      vsm_launch_export_xy(h->stream, c.d_pairs, h->xy_dev, nq2);
    HIPCHK(hipEventRecord(h->xy_ev, h->stream));
  } else {
    vsm_launch_match(h->stream, h->prof, c.d_imgs, c.d_pairs, nullptr, job, 1, c.dims, cfg, nq2);
  }
  // The list size is still on the device: the refinement / export grids are sized for the worst
  // case (every query matched) and surplus threads exit at once.
  if (h->capture_stage2 && p.refinement == 1)  // debug view: keep the unrefined list (raw is free again)
    HIPCHK(hipMemcpyAsync(c.h_pairs[0].raw, c.h_pairs[0].list2, (size_t)nq2 * sizeof(vsm_p_match), hipMemcpyDeviceToDevice,
                          h->stream));
  if (p.refinement > 0)
    vsm_launch_refine(h->stream, h->prof, c.d_imgs, c.d_pairs, nullptr, job, 1, dp, dc, method, p.refinement, nq2);
  // sub-pixel refinement: the fits' least-squares tail and the removal of failed matches on the device too (as in the look-ahead
  // path; 7 k matches x 3 fits were 3 ms of one host thread) - unless the stage views are wanted, which show the list in between
  const bool fits_on_device = p.refinement == 2 && !h->capture_stage2 && nq2 <= VSM_PARA_MAX_LIST;
  if (fits_on_device) vsm_launch_parabolic_apply(h->stream, h->prof, c.d_pairs, 1);
  vsm_launch_export(h->stream, h->prof, c.d_pairs, 1, 1, nq2);
  if (early_xy) {
    // (an event behind the export: waiting for it when it has long fired costs 2 us, hipStreamSynchronize on the idle stream 18)
    if (!h->done_ev) HIPCHK(hipEventCreateWithFlags(&h->done_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(h->done_ev, h->stream));
    HIPCHK(hipEventSynchronize(h->xy_ev));
    const int32_t n2 = c.hm_lcount[1];  // (written by the compaction, in front of the pixels)
    const double tk = now_us();
    if (n2 > 3) {
      vsm_host_outliers_begin_xy(h->work, h->xy_host, n2);
      h->work.del.run(h->work.x.data(), h->work.y.data(), n2, h->work.pool, h->work.async);
    }
    const double td = now_us();
    HIPCHK(hipEventSynchronize(h->done_ev));
    HIPCHK(hipGetLastError());
    h->prof.resolve();
    const double ts = now_us();
    const vsm_p_match *in = c.hm_list2[0];  // stage 3 is read where the device left it (vsm_stage_get)
    h->stage3_in_hm = true;
    h->counters[3] = n2;
    double tf = ts;
    if (n2 > 3) {
      vsm_host_outliers_begin_flows(h->work, in, n2, method);
      tf = now_us();
      vsm_host_outliers_end(h->work, p, in, n2, method, h->stage[4]);
    } else {
      h->stage[4].assign(in, in + std::max(n2, 0));  // the reference leaves short lists alone (:1210)
    }
    const double te = now_us();
    h->matched = h->stage[4];
    h->counters[4] = (int64_t)h->matched.size();
    const double t4 = now_us();
    if (vsm_debug_timing()) {
      static double acc[5] = {0, 0, 0, 0, 0};
      static long calls = 0;
      acc[0] += td - tk;
      acc[1] += ts - td;
      acc[2] += tf - ts;
      acc[3] += te - tf;
      acc[4] += t4 - te;
      if (++calls % 100 == 0)
        fprintf(stderr, "  vsm_match final host stage, mean us: triangulation %.1f, wait for the list %.1f, flows %.1f, support + survivors %.1f, copy %.1f\n",
                acc[0] / calls, acc[1] / calls, acc[2] / calls, acc[3] / calls, acc[4] / calls);
    }
    h->timings[0] = t1 - t0;
    h->timings[1] = t2 - t1;
    h->timings[2] = tk - t2;  // until the pixels are on the host
    h->timings[3] = t4 - tk;
    h->timings[4] = t4 - t0;
    return VSM_OK;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  const int32_t n2 = c.hm_lcount[1];
  if (fits_on_device) {
    h->stage[3].assign(c.hm_list2[0], c.hm_list2[0] + n2);
  } else if (p.refinement == 1) {
    h->stage[3].assign(c.hm_list2[0], c.hm_list2[0] + n2);
    if (h->capture_stage2) {
      h->stage[2].resize(n2);
      if (n2) HIPCHK(hipMemcpy(h->stage[2].data(), c.h_pairs[0].raw, (size_t)n2 * sizeof(vsm_p_match), hipMemcpyDeviceToHost));
    }
  } else {
    h->stage[2].assign(c.hm_list2[0], c.hm_list2[0] + n2);
    if (p.refinement == 2) {
      const size_t nn2 = h->stage[2].size();
      h->pf.resize(nn2 * 36);
      if (nn2) HIPCHK(hipMemcpy(h->pf.data(), c.h_pairs[0].pf, nn2 * 36 * sizeof(int32_t), hipMemcpyDeviceToHost));
      h->stage[3].clear();
      for (size_t i = 0; i < nn2; i++) {  // viso/matcher.cpp:1541-1581: a failed fit drops the match
        vsm_p_match m = h->stage[2][i];
        bool ok = true;
        float *tu[3] = {&m.u1p, &m.u2c, &m.u2p}, *tv[3] = {&m.v1p, &m.v2c, &m.v2p};
        for (int st = 0; st < 3 && ok; st++) {
          const int32_t *r = &h->pf[(i * 3 + st) * 12];
          if (r[0] == 2) continue;
          ok = r[0] == 1 && vsm_host_parabolic_update(r + 3, r[1], r[2], *tu[st], *tv[st]);
        }
        if (ok) h->stage[3].push_back(m);
      }
    } else {
      h->stage[3] = h->stage[2];
    }
  }
  h->prof.resolve();
  const double t3 = now_us();
  h->counters[3] = (int64_t)h->stage[3].size();
  h->stage[4] = h->stage[3];
  vsm_host_remove_outliers(h->work, p, h->stage[4], method);
  h->matched = h->stage[4];
  h->counters[4] = (int64_t)h->matched.size();
  const double t4 = now_us();
  h->timings[0] = t1 - t0;
  h->timings[1] = t2 - t1;
  h->timings[2] = t3 - t2;
  h->timings[3] = t4 - t3;
  h->timings[4] = t4 - t0;
  return VSM_OK;
}

int32_t vsm_num_matches(vsm_handle *h) { return (int32_t)h->matched.size(); }

int32_t vsm_get_matches(vsm_handle *h, vsm_p_match *out, int32_t cap) {
  int32_t n = (int32_t)h->matched.size();
  if (n > cap) n = cap;
  if (n > 0) memcpy(out, h->matched.data(), (size_t)n * sizeof(vsm_p_match));
  return n;
}

int vsm_bucket(vsm_handle *h, int32_t max_features, float bw, float bh) {
  vsm_host_bucket(h->matched, max_features, bw, bh);
  return VSM_OK;
}

float vsm_gain(vsm_handle *h, const int32_t *inliers, int32_t n) {
  const int sc = h->cur, sp = h->cur ^ 1;
  VsmCtx &c = h->ring;
  if (!c.ready || !h->have[sp] || !h->have[sc] || h->matched.empty() || n == 0 || settle(h) != VSM_OK) return 1;
  const size_t bytes = (size_t)c.dims.bpl * c.dims.h;
  for (int k = 0; k < 2; k++) {  // left images come back from HBM on first use
    if (h->gainI[k].size() != bytes) {
      h->gainI[k].resize(bytes);
      if (hipMemcpy(h->gainI[k].data(), c.h_imgs[(k == 0 ? sp : sc) * 2].img, bytes, hipMemcpyDeviceToHost) != hipSuccess)
        return 1;
    }
  }
  return vsm_host_gain(h->gainI[0].data(), h->gainI[1].data(), h->dims_p, h->dims_c, h->matched, inliers, n);
}

// Host images of a look-ahead chunk: a pageable 2-D copy is staged row by row by the runtime (milliseconds per image), so
// the pool gathers the chunk's 2 n images into a pinned slot (w bytes per row), one upload follows, and k_ingest reads the
// device twin like any device-resident input.  Two slots alternate; a slot is reused once its ingest has run.
static int seq_ingest_host_frames(vsm_handle *h, VsmCtx &c, int first_img, const uint8_t *left, const uint8_t *right, int64_t frame_stride,
                                  int32_t bpl, int32_t w, int32_t hh, int32_t f0, int n) {
  const size_t img = (size_t)w * hh, need = 2 * img * (size_t)h->seq_chunk;
  if (h->seq_stage_bytes < need) {
    (void)hipStreamSynchronize(h->stream);
    for (int k = 0; k < 2; k++) {
      if (h->seq_stage_h[k]) (void)hipHostFree(h->seq_stage_h[k]);
      if (h->seq_stage_d[k]) vsm_dev_free(h->seq_stage_d[k]);
      h->seq_stage_h[k] = h->seq_stage_d[k] = nullptr;
      HIPCHK(hipHostMalloc((void **)&h->seq_stage_h[k], need, hipHostMallocDefault));
      HIPCHK(vsm_dev_alloc((void **)&h->seq_stage_d[k], need));
      if (!h->seq_stage_ev[k]) HIPCHK(hipEventCreateWithFlags(&h->seq_stage_ev[k], hipEventDisableTiming));
      HIPCHK(hipEventRecord(h->seq_stage_ev[k], h->stream));
    }
    h->seq_stage_bytes = need;
  }
  const int slot = h->seq_stage_next;
  h->seq_stage_next ^= 1;
  HIPCHK(hipEventSynchronize(h->seq_stage_ev[slot]));  // its previous content has been ingested
  uint8_t *dst = h->seq_stage_h[slot];
  const int sides = right ? 2 : 1;
  h->pool->run(sides * n, [&](int t) {
    const int i = right ? t >> 1 : t, side = right ? (t & 1) : 0;
    const uint8_t *src = (side ? right : left) + (size_t)(f0 + i) * frame_stride;
    uint8_t *d = dst + ((size_t)side * n + i) * img;
    if (bpl == w) {
      memcpy(d, src, img);
    } else {
      for (int32_t v = 0; v < hh; v++) memcpy(d + (size_t)v * w, src + (size_t)v * bpl, w);
    }
  });
  HIPCHK(hipMemcpyAsync(h->seq_stage_d[slot], dst, (size_t)sides * img * n, hipMemcpyHostToDevice, h->stream));
  const uint8_t *d0 = h->seq_stage_d[slot];
  enqueue_front_frames(h, c, first_img, sides, d0, img, d0 + img * n, img, w, n);
  HIPCHK(hipEventRecord(h->seq_stage_ev[slot], h->stream));
  return VSM_OK;
}

}  // extern "C"
#include "vsm_seq2.inc"
#include "vsm_seq1.inc"
#include "vsm_step.inc"
#include "vsm_multi.inc"
#include "vsm_pairs.inc"
#include "vsm_tracks.inc"
#include "vsm_points.inc"
#include "vsm_resect.inc"
#include "vsm_vet.inc"
#include "vsm_ba.inc"
#include "vsm_locate.inc"
#include "vsm_reobserve.inc"
#include "vsm_fuse.inc"
#include "vsm_motions_api.inc"
extern "C" {

// ---------------------------------------------------------------------------------------
// Look-ahead sequence API.  Semantics: exactly pushBack(frame f) + matchFeatures(method, Tr[f])
// for f = 0..n-1 on a fresh matcher.  Frames are processed in chunks of C: every kernel runs once
// per chunk over all its images / pairs, and the host stages (exact Delaunay support, prior
// statistics) of the chunk's pairs run concurrently on the pool, one pair per task.
// ---------------------------------------------------------------------------------------
static int sequence_fallback(vsm_handle *h, const uint8_t *left, const uint8_t *right, int64_t frame_stride, int on_device,
                             int32_t n_frames, int32_t w, int32_t hh, int32_t bpl, int32_t method, const double *Tr,
                             const uint8_t *Tr_valid) {
  // rarely used configurations (mono input, refinement==2) go frame by frame on a fresh ring
  (void)hipStreamSynchronize(h->stream);
  for (hipStream_t st : h->dc_stream)
    if (st) (void)hipStreamSynchronize(st);
  seq2_destroy(h);
  ctx_destroy(h->ring);
  reset_ring_state(h);
  h->matched.clear();
  for (int32_t f = 0; f < n_frames; f++) h->seq_src[f] = f;
  for (int32_t f = 0; f < n_frames; f++) {
    const uint8_t *l = left + (size_t)f * frame_stride, *r = right ? right + (size_t)f * frame_stride : nullptr;
    int rc = push_common(h, l, r, w, hh, bpl, 0, on_device != 0);
    if (rc != VSM_OK) return rc;
    const double *t = (Tr && (!Tr_valid || Tr_valid[f])) ? Tr + (size_t)f * 12 : nullptr;
    rc = vsm_match(h, method, t);
    if (rc != VSM_OK && rc != VSM_ENOTREADY) return rc;
    h->seq_matches[f] = h->matched;
  }
  return VSM_OK;
}

int vsm_sequence_run(vsm_handle *h, const uint8_t *left, const uint8_t *right, int64_t frame_stride, int on_device,
                     int32_t n_frames, int32_t w, int32_t hh, int32_t bpl, int32_t method, const double *Tr,
                     const uint8_t *Tr_valid) {
  if (w <= 0 || hh <= 0 || bpl < w || left == nullptr || n_frames <= 0) {
    fprintf(stderr, "ERROR: Image dimension mismatch!\n");
    return VSM_EDIMS;
  }
  HIPCHK(hipSetDevice(h->device));
  const vsm_params &p = h->param;
  h->seq_v2_frames = 0;
  h->seq_matches.resize(n_frames);  // keeps the capacity of earlier runs: no page-fault storm
  for (auto &v : h->seq_matches) v.clear();
  h->seq_view.assign(n_frames, vsm_handle::SeqView());
  h->seq_src.resize(n_frames);
  for (int32_t f = 0; f < n_frames; f++) h->seq_src[f] = f;
  // (mono input can only be flow-matched; the host-shared form (vsm_seq1.inc) has no sub-pixel refinement - its fits and dropped matches
  // are the GPU-resident form's, or the per-frame code's)
  if ((!right && (method != 0 || !h->sw.seq_v2)) || (p.refinement == 2 && !h->sw.seq_v2))
    return sequence_fallback(h, left, right, frame_stride, on_device, n_frames, w, hh, bpl, method, Tr, Tr_valid);

  // The GPU-resident form (vsm_seq2.inc) takes the run unless VSM_SEQ_V2=0 asks for the host-shared form (vsm_seq1.inc), or
  // it declines (lists beyond what its device-side vertex sort / kd order were written for).
  // The host-shared form lives off the rank's host threads (200 frames 1242x375, round 3: 7.6 ms with 14 pool threads, 15 with 8,
  // 24 with 2); the GPU-resident one keeps only Triangle's vertex sort and the closing of the result lists on the host (5.0-5.2 ms
  // with 14 threads, 6.3 with 8, 8.0 with 4, 8.9 with 2, 9.1 with 1 - results in host memory included), so it is the default
  // whatever the thread count.
  if (h->sw.seq_v2) {
    const int rc = sequence_run_v2(h, left, right, frame_stride, on_device, n_frames, w, hh, bpl, method, Tr, Tr_valid);
    if (rc != VSM_SEQ2_DECLINED) return rc;
    h->seq_v2_frames = 0;
    if (!right || p.refinement == 2) return sequence_fallback(h, left, right, frame_stride, on_device, n_frames, w, hh, bpl, method, Tr, Tr_valid);
  }
  return sequence_run_v1(h, left, right, frame_stride, on_device, n_frames, w, hh, bpl, method, Tr, Tr_valid);
}

// the frame whose list stands after `frame` (vsm_handle::seq_src), -1: no list yet
static int32_t seq_source_frame(const vsm_handle *h, int32_t frame) {
  if (frame < 0 || frame >= (int32_t)h->seq_matches.size()) return -1;
  return frame < (int32_t)h->seq_src.size() ? h->seq_src[frame] : frame;
}

int32_t vsm_sequence_num_matches(vsm_handle *h, int32_t frame) {
  frame = seq_source_frame(h, frame);
  if (frame < 0) return 0;
  if (frame < (int32_t)h->seq_view.size() && h->seq_view[frame].p) return h->seq_view[frame].n;
  return (int32_t)h->seq_matches[frame].size();
}

// (both look-ahead forms end with every frame's list in the reference's 48-byte p_match form in host memory)
int32_t vsm_sequence_get_matches(vsm_handle *h, int32_t frame, vsm_p_match *out, int32_t cap) {
  frame = seq_source_frame(h, frame);
  if (frame < 0) return 0;
  const bool view = frame < (int32_t)h->seq_view.size() && h->seq_view[frame].p;
  int32_t n = view ? h->seq_view[frame].n : (int32_t)h->seq_matches[frame].size();
  if (n > cap) n = cap;
  if (n > 0) memcpy(out, view ? h->seq_view[frame].p : h->seq_matches[frame].data(), (size_t)n * sizeof(vsm_p_match));
  return n;
}

void vsm_sequence_get_timings(vsm_handle *h, double *out4) { memcpy(out4, h->seq_timings, sizeof(h->seq_timings)); }
int32_t vsm_sequence_path(vsm_handle *h) { return h->seq_v2_frames > 0 ? 2 : 1; }
int32_t vsm_local_cpus(int32_t *out, int32_t cap) { return vsm_affinity_cpus(out, out ? cap : 0); }
int32_t vsm_forkjoin_cpus(int32_t *out, int32_t cap) {
  if (vsm_forkjoin_domain() < 0) return 0;
  if (vsm_forkjoin_per_core()) {  // the workers have a core each: the caller's is core 0 of their domain
    const int32_t n = vsm_affinity_core_cpus(nullptr, vsm_forkjoin_domain(), 0, out, out ? cap : 0);
    if (n > 0) return n;
  }
  return vsm_affinity_domain_cpus(nullptr, vsm_forkjoin_domain(), out, out ? cap : 0);
}

int vsm_host_register(const void *p, uint64_t bytes) {
  if (!p || bytes == 0) return VSM_EARG;
  const hipError_t e = hipHostRegister(const_cast<void *>(p), (size_t)bytes, hipHostRegisterDefault);
  if (e == hipSuccess) return VSM_OK;
  (void)hipGetLastError();
  return e == hipErrorHostMemoryAlreadyRegistered ? VSM_OK : VSM_EHIP;
}
int vsm_host_unregister(const void *p) {
  if (!p) return VSM_EARG;
  const hipError_t e = hipHostUnregister(const_cast<void *>(p));
  if (e != hipSuccess) (void)hipGetLastError();
  return e == hipSuccess ? VSM_OK : VSM_EHIP;
}
int vsm_set_option(vsm_handle *h, const char *name, int32_t value) { return (h && name && h->sw.set(name, value)) ? VSM_OK : VSM_EARG; }

// ---- stage-level views ----
static bool which_set(vsm_handle *h, int32_t which, int &img, int &set, int32_t &n) {
  if (which < 0 || which > 7 || !h->ring.ready) return false;
  if (settle(h) != VSM_OK) return false;
  const int prev = (which & 3) < 2, side = which & 1;
  set = which >> 2;
  const int slot = prev ? (h->cur ^ 1) : h->cur;
  img = slot * 2 + side;
  n = h->have[slot] ? h->n_feat[slot][side][set] : 0;
  return true;
}

int32_t vsm_num_features(vsm_handle *h, int32_t which) {
  int img, set;
  int32_t n;
  return which_set(h, which, img, set, n) ? n : 0;
}

int32_t vsm_get_features(vsm_handle *h, int32_t which, int32_t *out, int32_t cap) {
  int img, set;
  int32_t n;
  if (!which_set(h, which, img, set, n)) return 0;
  if (n > cap) n = cap;
  if (n > 0 && hipMemcpy(out, h->ring.h_imgs[img].set[set].feat, (size_t)n * 48, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return n;
}

void vsm_set_stage_capture(vsm_handle *h, int on) { h->capture_stage2 = on ? 1 : 0; }

// (stage 3 of the per-frame path - the refined list in front of the final removeOutliers - stays where the device exported
// it, in the ring's host-mapped block, until the next vsm_match: no copy of it inside the call)
int32_t vsm_stage_size(vsm_handle *h, int32_t s) {
  if (s == 3 && h->stage3_in_hm) return std::max(h->ring.hm_lcount[1], 0);
  return (s >= 0 && s < 5) ? (int32_t)h->stage[s].size() : 0;
}

int32_t vsm_stage_get(vsm_handle *h, int32_t s, vsm_p_match *out, int32_t cap) {
  if (s < 0 || s >= 5) return 0;
  const bool hm = s == 3 && h->stage3_in_hm;
  int32_t n = hm ? std::max(h->ring.hm_lcount[1], 0) : (int32_t)h->stage[s].size();
  if (n > cap) n = cap;
  if (n > 0) memcpy(out, hm ? h->ring.hm_list2[0] : h->stage[s].data(), (size_t)n * sizeof(vsm_p_match));
  return n;
}

int32_t vsm_num_ranges(vsm_handle *h) { return (int32_t)(h->ranges.size() / 16); }

int32_t vsm_get_ranges(vsm_handle *h, float *out, int32_t cap_bins) {
  int32_t n = (int32_t)(h->ranges.size() / 16);
  if (n > cap_bins) n = cap_bins;
  if (n > 0) memcpy(out, h->ranges.data(), (size_t)n * 64);
  return n;
}

int32_t vsm_get_gradients(vsm_handle *h, int32_t which, int32_t full, uint8_t *du, uint8_t *dv) {
  VsmCtx &c = h->ring;
  if (!c.ready || which < 0 || which > 3 || settle(h) != VSM_OK) return 0;
  const int slot = which < 2 ? (h->cur ^ 1) : h->cur, side = which & 1;
  if (!h->have[slot] || (side && !h->right[slot])) return 0;
  if (full && !h->param.half_resolution) return 0;
  const VsmImage &im = c.h_imgs[slot * 2 + side];
  const int32_t bytes = full ? c.dims.bpl * c.dims.h : c.dims.mbpl * c.dims.mh;
  if (full) {  // the tiled plane (8 x 8 tiles; a tile row = du 0-3, dv 0-3, du 4-7, dv 4-7: vsm_tiled_at in vsm_dev.h), un-tiled here
    const int bpl = c.dims.bpl, hh = c.dims.h;
    std::vector<uint8_t> t((size_t)bpl * ((hh + 7) & ~7) * 2);
    if (hipMemcpy(t.data(), im.duv_tiled, t.size(), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    for (int y = 0; y < hh; y++)
      for (int x = 0; x < bpl; x++) {
        const size_t a = ((size_t)(y >> 3) * (size_t)(bpl >> 3) + (size_t)(x >> 3)) * 128 + (size_t)((y & 7) * 16 + ((x & 4) << 1) + (x & 3));
        if (du) du[(size_t)y * bpl + x] = t[a];
        if (dv) dv[(size_t)y * bpl + x] = t[a + 4];
      }
    return bytes;
  }
  if (du && hipMemcpy(du, im.du, bytes, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  if (dv && hipMemcpy(dv, im.dv, bytes, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return bytes;
}

int32_t vsm_get_filter_responses(vsm_handle *h, int16_t *f1, int16_t *f2) {
  VsmCtx &c = h->ring;
  if (!c.ready || !h->f_valid || settle(h) != VSM_OK) return 0;
  const int32_t n = c.dims.mbpl * c.dims.mh;
  if (f1 && hipMemcpy(f1, c.f1, (size_t)n * 2, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  if (f2 && hipMemcpy(f2, c.f2, (size_t)n * 2, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return n;
}

static const char *kKernelNames[VSM_K_COUNT] = {
    "k_ingest", "k_halve", "k_filters<true>", "k_filters<false>", "k_nms:dense", "k_nms:sparse", "k_scan_cells", "k_emit", "k_bin_scan",
    "k_bin_scatter", "k_bin_rank", "k_match<16>:pass1", "k_compact_matches:pass1", "k_match<16>:pass2",
    "k_compact_matches:pass2", "k_refine", "k_export_list", "k_front",
    "k_dc_keys", "k_dc_vertex_sort", "k_dc_prepare_kd_order", "k_dc_block", "k_dc_merge", "k_dc_support", "k_dc_compact", "k_dc_prior",
    "k_feat_dense", "k_feat_sparse", "k_feat_scan", "k_feat_order", "k_parabolic_apply",
    "k_trk_init", "k_trk_hook", "k_trk_flatten", "k_trk_keep", "k_trk_scan_reduce", "k_trk_scan_top", "k_trk_scan_apply", "k_trk_match_tracks", "k_trk_fill",
    "k_trk_order_wave", "k_trk_order_block", "k_pts_triangulate", "k_rs_resect", "k_vet_obs", "k_vet_emit",
    "k_ba_init", "k_ba_linearise", "k_ba_tracks", "k_ba_frames<rhs>", "k_ba_cg_init", "k_ba_op_tracks", "k_ba_frames<op>", "k_ba_cg_step", "k_ba_back",
    "k_ba_trial_cost", "k_ba_decide", "k_ba_commit", "k_ba_finish", "k_locate_fit", "k_locate_count", "k_locate_winner",
    "k_ro_occupy", "k_ro_bin_count", "k_ro_scatter", "k_ro_project<count>", "k_ro_project<list>", "k_ro_search", "k_ro_verdict",
    "k_fu_owner", "k_fu_bin_count", "k_fu_scatter", "k_fu_search<count>", "k_fu_search<list>", "k_fu_conflict", "k_fu_verdict", "k_fu_lengths", "k_fu_merge", "k_fu_compact"};

void vsm_set_profiling(vsm_handle *h, int on) {
  h->prof.on = on != 0;
  h->prof.print_spans = on >= 1100;
  h->prof.only = on >= 1100 ? on - 1100 : (on >= 100 ? on - 100 : -1);
  if (on) {
    memset(h->prof.total_ms, 0, sizeof(h->prof.total_ms));
    memset(h->prof.launches, 0, sizeof(h->prof.launches));
  }
}

int32_t vsm_num_kernels(void) { return VSM_K_COUNT; }

const char *vsm_kernel_name(int32_t id) { return (id >= 0 && id < VSM_K_COUNT) ? kKernelNames[id] : ""; }

void vsm_get_kernel_stats(vsm_handle *h, double *total_ms, int64_t *launches) {
  memcpy(total_ms, h->prof.total_ms, sizeof(h->prof.total_ms));
  memcpy(launches, h->prof.launches, sizeof(h->prof.launches));
}

void vsm_get_counters(vsm_handle *h, int64_t *out5) { memcpy(out5, h->counters, sizeof(h->counters)); }
void vsm_get_timings(vsm_handle *h, double *out5) { memcpy(out5, h->timings, sizeof(h->timings)); }

}  // extern "C"
#include "vsm_debug.inc"
