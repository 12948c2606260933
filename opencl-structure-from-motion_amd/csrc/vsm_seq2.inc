// GPU-resident look-ahead path (included by vsm_api.cpp; DESIGN.md section 6).
//
// vsm_sequence_run's first form (further down in vsm_api.cpp) brings every match list to the host twice per frame
// pair - for the pass-1 outlier removal + prior statistics, and for the final outlier removal - and the host pool
// sets the pace.  Here the lists stay in HBM from the first matching pass to the survivors:
//
//   main stream    features(k+2) | pass 1 (k+2) | [wait: prior boxes of k] pass 2 (k) | refinement (k) | ...
//   side streams   cs[k % 3], pass-1 list of chunk k: keys | sort + duplicates + kd order -> block sub-trees -> merge levels ->
//                  support votes -> prior statistics, written where pass 2 reads them (the list's vertex sort, one wave per
//                  pair, beside it on the null stream);
//                  cs[k % 3] again, pass-2 list of chunk k: keys (a DMA copy takes them to the host) -> the same triangulation
//                  chain; then, behind the refinement and the host's vertex sorts: tie patches, support votes, survivor bits
//   null stream    the refined lists' early export to the host in DMA pieces, ordered behind the keys (one copy engine)
//   host pool      Triangle's randomised vertex sort of the pass-2 lists (strictly serial per list; it decides which match
//                  stands for a pixel that several share): keys in, (carried, right) index patches out; at the end the gaps
//                  the outliers leave in the exported lists are closed
//   (Seq2 below has the stream layout and why it is five hardware queues and no more; sequence_run_v2 the order of it all.)
//
// The caller's thread enqueues; it waits for feature counts (grid sizes) and for slabs to come free, nothing else.
#include "vsm_dc_gpu.h"

struct Dc2Bank {
  int npairs = 0, cap = 0;
  bool host_ties = false;
  uint8_t *d_block = nullptr, *h_block = nullptr, *h_block_dev = nullptr;
  VsmDc2Job *h_jobs = nullptr, *d_jobs = nullptr;  // pinned / device
  int32_t *d_ties = nullptr;                       // device verdicts of k_dc2_ties [npairs][VSM_DC_TIE_OUT_INTS]
  uint64_t *h_keys = nullptr;                      // host views of the host-mapped block
  int32_t *h_n = nullptr, *h_ties = nullptr, *h_error = nullptr;
  int ties_stride = 0;
  size_t pair_stride = 0;                 // bytes from one pair's device arrays to the next pair's
  size_t keys_pitch = 0, ties_pitch = 0;  // bytes from one pair's host keys / tie patches to the next pair's
  using PairPtr = Dc2PairPtr;
  std::vector<PairPtr> pp;
  void release() {
    if (d_block) vsm_dev_free(d_block);
    if (h_block) (void)hipHostFree(h_block);
    if (h_jobs) (void)hipHostFree(h_jobs);
    *this = Dc2Bank();
  }
  bool reserve(int pairs, int want_cap, bool with_host_ties) {
    if (pairs <= npairs && want_cap <= cap && (!with_host_ties || host_ties)) return true;
    const int ncap = std::max(((want_cap + 1023) / 1024) * 1024, cap), np = std::max(pairs, npairs);
    const bool ht = with_host_ties || host_ties;
    release();
    npairs = np;
    cap = ncap;
    host_ties = ht;
    const Dc2Layout L(npairs, cap, ht);  // (vsm_layouts.h)
    pair_stride = L.pair_stride, ties_stride = L.ties_stride, keys_pitch = L.keys_pitch, ties_pitch = L.ties_pitch;
    if (vsm_dev_alloc((void **)&d_block, L.dev.at) != hipSuccess || hipHostMalloc((void **)&h_block, L.host.at, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&h_block_dev, h_block, 0) != hipSuccess ||
        hipHostMalloc((void **)&h_jobs, sizeof(VsmDc2Job) * npairs, hipHostMallocDefault) != hipSuccess) {
      release();
      return false;
    }
    memset(h_block, 0, L.host.at);
    pp.resize(npairs);
    n_src.assign(npairs, nullptr);
    for (int i = 0; i < npairs; i++) pp[i] = L.bind(d_block, i);
    d_jobs = L.jobs.in(d_block);
    d_ties = L.ties.in(d_block);
    h_error = L.h_error.in(h_block);
    h_n = L.h_n.in(h_block);
    if (ht) h_keys = (uint64_t *)L.h_keys.in(h_block), h_ties = (int32_t *)L.h_ties.in(h_block);
    return true;
  }
  // list length of job i as the host sees it: the word k_dc2_keys writes (min(count, cap)), or - jobs whose keys the
  // compaction wrote, no key kernel - the count the compaction itself put into host-mapped memory (fill_job's host_count, the
  // pair's hcount[pass]).  That count is NOT clamped at cap: every reader checks n <= cap or takes the minimum itself, and the
  // device side declines a list beyond cap (k_dc2_prepare) whoever made its keys.
  std::vector<const int32_t *> n_src;  // per job; set by every fill_job
  int32_t list_n(int i) const { return n_src[i] ? *n_src[i] : h_n[i]; }
  uint64_t *host_keys(int i) const { return (uint64_t *)((uint8_t *)h_keys + keys_pitch * i); }
  int32_t *host_ties_of(int i) const { return (int32_t *)((uint8_t *)h_ties + ties_pitch * i); }
  // a pool task: Triangle's vertex sort of list i from its keys in host-mapped memory - the number of (carried, right) index
  // patches and the patches into host_ties_of(i); none for a list the chain leaves alone or declines.  (sort_ties works on a
  // copy of its own: one pass over the keys, then cache-resident work)
  void sort_ties_of(int i) const {
    static thread_local ExactDelaunay sorter;
    const int32_t n = list_n(i);
    int32_t *out = host_ties_of(i);
    out[0] = (n > 3 && n <= cap) ? sorter.sort_ties(host_keys(i), n, out + 1, (ties_stride - 1) / 2) : 0;
  }
  template <typename T>
  T *dev_of(T *host_ptr) const {  // device address of something inside the host-mapped block
    return (T *)(h_block_dev + ((uint8_t *)host_ptr - h_block));
  }
  // job i: the chain of list `list` / `count`; gpu_ties: the verdicts come from k_dc2_ties, else from the host
  // pair_keys: the list's keys are where the matching pass's compaction wrote them (VsmPair::keys, fused_keys) - no key
  // kernel runs for this job, the keys the pool sorts leave by a DMA copy out of the pair bank or by the compaction's own
  // stores, and host_count is the host view of the count that compaction writes (list_n)
  void fill_job(int i, const vsm_p_match *list, const int32_t *count, bool gpu_ties, vsm_p_match *out, int32_t *h_out_count,
                float *ranges, uint32_t *h_keep = nullptr, bool keys_by_dma = false, uint64_t *pair_keys = nullptr,
                const int32_t *host_count = nullptr) {
    const PairPtr &q = pp[i];
    n_src[i] = pair_keys ? host_count : nullptr;
    VsmDc2Job &jb = h_jobs[i];
    memset(&jb, 0, sizeof(jb));
    jb.list = list;
    jb.count = count;
    jb.cap = cap;
    jb.kd_stride = cap;
    jb.keys_in = pair_keys ? pair_keys : q.keys_in;
    // (keys_by_dma: the keys the pool sorts leave by a DMA copy of keys_in, not by stores of the key kernel)
    jb.h_keys = (!gpu_ties && host_ties && !keys_by_dma && !pair_keys) ? dev_of(host_keys(i)) : nullptr;
    jb.h_n = dev_of(h_n + i);
    jb.key_sorted = q.key_sorted;
    jb.key = q.key;
    jb.kd_scratch = q.kd;
    jb.pt = q.pt;
    jb.id = q.id;
    jb.tri = q.tri;
    jb.hulls = q.hulls;
    jb.mn = q.mn;
    jb.support = q.support;
    jb.remap = q.remap;
    jb.tie_out = gpu_ties ? d_ties + (size_t)i * VSM_DC_TIE_OUT_INTS : dev_of(host_ties_of(i));
    jb.out = out;
    jb.out_count = q.out_count;
    jb.h_out_count = h_out_count;
    jb.ranges = ranges;
    jb.error = dev_of(h_error);
    jb.long_seen = dev_of(h_error + 1);
    jb.h_keep = h_keep;
  }
};

// the part of the chain that only needs (u1c, v1c) of the list: keys, (x,y) order, duplicates, kd order, triangulation
// (pf: optional kernel timing, spans on the chain's own stream)
static VsmProf g_no_prof;

static void dc2_enqueue_triangulation(hipStream_t s, Dc2Bank &B, int n, int max_list, bool gpu_ties, VsmProf &pf = g_no_prof) {
  pf.begin(VSM_K_DC_KEYS, s);
  vsm_dc2_launch_keys(s, B.d_jobs, n, max_list);
  pf.end(s);
  if (gpu_ties) {
    pf.begin(VSM_K_DC_TIES, s);
    vsm_dc2_launch_ties(s, B.d_jobs, n, B.d_ties, VSM_DC_TIE_OUT_INTS);
    pf.end(s);
  }
}
// (a handle that has met a list beyond the LDS forms' 8192 points brings the long lists' kernel along from then on: Seq2::expect_long)
static void dc2_enqueue_prepare(hipStream_t s, Dc2Bank &B, int n, int max_list, VsmProf &pf = g_no_prof, bool expect_long = true) {
  pf.begin(VSM_K_DC_KD, s);
  vsm_dc2_launch_prepare(s, B.d_jobs, n, max_list, expect_long);
  pf.end(s);
}
// (prepared: the sort + kd order kernel went in with the chain's head; before_blocks: an event the block kernel waits for)
static void dc2_enqueue_mesh(hipStream_t s, Dc2Bank &B, int n, int max_list, VsmProf &pf = g_no_prof, bool prepared = false,
                             hipEvent_t before_blocks = nullptr, bool expect_long = true) {
  const int depth = vsm_dc2_depth(max_list);
  if (!prepared) dc2_enqueue_prepare(s, B, n, max_list, pf, expect_long);
  if (before_blocks) (void)hipStreamWaitEvent(s, before_blocks, 0);
  pf.begin(VSM_K_DC_BLOCK, s);
  vsm_dc2_launch_blocks(s, B.d_jobs, n, depth);
  pf.end(s);
  if (depth > 0) {
    pf.begin(VSM_K_DC_MERGE, s);
    vsm_dc2_launch_merges(s, B.d_jobs, n, depth, max_list);
    pf.end(s);
  }
}
static void dc2_enqueue_votes(hipStream_t s, Dc2Bank &B, int n, int max_list, int method, float ftol, float dtol, VsmProf &pf = g_no_prof,
                              bool flows_done = false) {
  pf.begin(VSM_K_DC_SUPPORT, s);
  if (!flows_done) vsm_dc2_launch_flows(s, B.d_jobs, n, max_list, method);
  vsm_dc2_launch_votes(s, B.d_jobs, n, max_list, method, ftol, dtol);
  pf.end(s);
}

// Who notices that an event of a side stream has happened - the pool's keys have crossed PCIe, a chain's last kernel is
// through - and starts what follows on the host.  Not a host function on the stream: whatever is enqueued behind it would wait
// for the runtime's callback thread, which answers after 0.1 .. 0.7 ms while the pool is busy.  Not a pool task that asks the
// event either: with few pool threads such tasks sit on top of each other (a waiting task that lends its thread to other
// tasks picks up the next waiting task) and unwind last in, first out.  One thread per handle asks the pending events in turn
// and sleeps 20 us between rounds while there are any (it exists only while a call is in flight).
struct Seq2Poller {
  struct Item {
    hipEvent_t ev;
    std::function<void(bool)> then;  // argument: the event completed (false: the query failed or timed out)
    double t0;
  };
  std::mutex mu;
  std::condition_variable cv;
  std::vector<Item> items;
  std::thread th;
  bool stop = false;
  int device = 0;
  bool spin = false;    // between rounds: yield (ranks with ten pool threads and more; VSM_POLL_SPIN=0 / 1 overrides) or sleep
  void *aff = nullptr;  // the handle's device's CPU record (vsm_affinity_current() at vsm_create)
  void start(int dev, void *affinity, bool spin_between_rounds) {
    if (th.joinable()) return;
    device = dev;
    aff = affinity;
    spin = getenv("VSM_POLL_SPIN") ? atoi(getenv("VSM_POLL_SPIN")) != 0 : spin_between_rounds;
    th = std::thread([this] { run(); });
  }
  void add(hipEvent_t ev, std::function<void(bool)> then) {
    {
      std::lock_guard<std::mutex> lk(mu);
      items.push_back(Item{ev, std::move(then), vsm_now_us()});
    }
    cv.notify_one();
  }
  void run() {
    vsm_pin_this_thread(aff);
    (void)hipSetDevice(device);
    std::vector<Item> ready;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || !items.empty(); });
        if (stop && items.empty()) return;
        for (size_t i = 0; i < items.size();) {
          const hipError_t e = hipEventQuery(items[i].ev);
          const bool failed = e != hipSuccess && (e != hipErrorNotReady || vsm_now_us() - items[i].t0 > 30e6);
          if (e == hipSuccess || failed) {
            if (failed) (void)hipGetLastError();
            ready.push_back(std::move(items[i]));
            ready.back().t0 = failed ? -1 : 0;
            items[i] = std::move(items.back());
            items.pop_back();
          } else {
            i++;
          }
        }
      }
      for (Item &it : ready) it.then(it.t0 == 0);
      if (ready.empty()) {
        // (sleep_for(20 us) comes back after 70-80 - the kernel's timer slack - and two of these waits lie on every call's
        // critical path, keys -> vertex sorts and survivor bits -> gap closing: ranks with CPUs to spare yield instead,
        // median step 3.91 -> 3.87 ms)
        if (spin)
          std::this_thread::yield();
        else
          std::this_thread::sleep_for(std::chrono::microseconds(20));
      }
      ready.clear();
    }
  }
  void shutdown() {
    if (!th.joinable()) return;
    {
      std::lock_guard<std::mutex> lk(mu);
      stop = true;
    }
    cv.notify_one();
    th.join();
    stop = false;
  }
};

// One chunk's final chain (pass-2 lists -> survivors) and what the pool and the HIP runtime's threads need to carry it on.
struct Seq2Chunk {
  vsm_handle *h = nullptr;
  int k = 0, n = 0, f0 = 0, max_list = 0, method = 0, gpu_sorts = 0;
  hipEvent_t ev_ties = nullptr;  // the device's share of the vertex sorts
  bool gate_deferred = false;    // the caller's half of the gate waits for that launch to be enqueued (caller's thread only)
  Dc2Bank *B = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev_c2 = nullptr;   // the chunk's second pass is done (main stream): the chain's keys start here
  hipEvent_t ev_jobs = nullptr; // the chain's job table and keys are in place (its own stream)
  hipEvent_t ev_keys = nullptr; // the pool's keys have crossed PCIe (chain stream)
  hipEvent_t ev_mesh = nullptr; // the chain's triangulation and per-match flows are done (its own stream): the second part waits for it
  hipEvent_t ev_ref = nullptr;  // the chunk's refinement is done (main stream)
  hipEvent_t ev_exp = nullptr;  // the refined lists have crossed PCIe (early export)
  hipEvent_t ev_prep = nullptr; // the chain's sort + kd order kernel (enqueued with its head) is through
  int exp_row = 0;              // ... rows (pairs) of the chunk whose copy has been submitted
  bool caller_gate = false;     // the caller's thread has opened its half of the gate (read by that thread only)
  float ftol = 0, dtol = 0;
  std::atomic<int> sorts_left{0};
  std::atomic<int> sort_tasks_left{0};  // the pool's vertex sorts of this chunk that have not finished (all pieces of the keys' copy)
  // the call's last chunk: between its last vertex sort and its survivor bits the pool has nothing to do - it reads the chunk's
  // exported lists (31 MB, through DRAM otherwise when the gaps are closed) into its threads' L3 caches; a list's gaps are then
  // closed by a thread of the L3 domain that read it
  bool warm = false;
  std::unique_ptr<std::atomic<signed char>[]> warm_domain;  // [n] L3 domain that has list i (-1: none)
  std::unique_ptr<std::atomic<unsigned char>[]> warm_claim; // [n] 1: a gap-closing task has taken list i
  // warm-up tasks not yet finished: they read the chunk and the arena, so the call does not return (and the next call does not
  // free the chunk) before they are through - they are queued behind everything else and may outlast the gap closing
  std::atomic<int> warm_left{0};
  // the second part (votes, survivors) needs the vertex sorts AND the refinement's event, which the caller's thread records:
  // whoever comes last enqueues it
  std::atomic<int> gate{2};
  std::atomic<int> unpack_left{0};  // gap-closing tasks of the chunk not yet finished (a frame each; the warm form: seq2_chunk_done)
  std::atomic<int> state{0};  // 0 idle, 1 triangulation enqueued, 2 second part enqueued, 3 done (views in vsm_handle::seq_view)
  std::atomic<int> hip_error{0};
  double t_keys = 0, t_sorted = 0, t_done = 0, t_ready = 0;
  std::atomic<long long> sort_ns{0};
};

struct Seq2 {
  // FIVE hardware queues carry the whole path, and no more: with a sixth queue in the process every kernel's workgroup
  // dispatch is throttled to a half or a quarter, whatever the other queues are doing (measured, tools/span_probe.py: the
  // second pass's compaction 28 us with up to five queues, 57 / 113 us with six and more; k_refine 100 -> 135 .. 180; the
  // command processor's compute pipes serve one queue each at a time).  The runtime hands hardware queues to streams as
  // they are created and, once GPU_MAX_HW_QUEUES of them exist, lets a new stream share the least used one - which one
  // that is cannot be chosen, and a stream that shares the main stream's queue runs in turns with it.  So the path has
  // exactly FOUR streams of its own beside the process's null stream: the handle's main stream and three side streams
  // cs[0..2] that take the chains in a rotation - and it uses the null stream (the fifth queue, which exists anyway and has
  // nothing to do during a call; all of these streams are non-blocking) for what must not stand in a chain's way:
  //   pass-1 chain of chunk j (keys, mesh, votes, prior boxes: wanted two chunks later)                 cs[j % 3]  (two slabs: chains of successive chunks overlap)
  //   pass-1 vertex sort of chunk j (one wave per list, 0.4 ms, beside the pass-1 mesh)                 null stream
  //   final chain of chunk j (head: jobs, keys, the keys' DMA copy to the pool; mesh; second part)   cs[j % 3]
  //   early export of chunk j's refined lists (28 MB per 80 pairs, in DMA copies of 20 pairs)           null stream, submitted in the order the copy engine
  //                                                                                                      should work in (Seq2Call::export_some)
  hipStream_t dc2[4] = {nullptr, nullptr, nullptr, nullptr};  // cs[]: dc_streams (1..3) of them
  // the device's share of the final chains' vertex sorts (ranks with few host threads): ONE launch for the lists of all the
  // chunks that are waiting for it - a wave per list takes 3.2 ms whatever the number of lists - on the null stream; its job
  // table is gathered from the chunks' slabs
  VsmDc2Job *tie_jobs_h = nullptr, *tie_jobs_d = nullptr;
  int tie_jobs_cap = 0;
  hipStream_t up = nullptr;   // host-resident inputs only: their uploads (3.7 ms of DMA per 200 frames).  Under the cap of five hardware queues it
                              // shares one with a stream of the path; it lives for the duration of a host-fed call only
  // The "fifth stream" of the plan above.  Default: the process's null stream.  NOTE FOR EMBEDDERS: the null stream is not the
  // library's - an application's blocking streams synchronise with it implicitly and PyTorch's default stream IS it - so an
  // application that keeps its own work there sets option "seq_null_stream" = 0 (vsm_set_option): the exports and the
  // device's vertex sorts then go to a non-blocking stream of the library's own (`aux`), at the price of a sixth stream that
  // shares a hardware queue with one of the others when the process caps them at five (INTEGRATION.md).
  hipStream_t aux = nullptr;
  hipStream_t ns = nullptr;   // what the call uses as its fifth stream: nullptr (the null stream) or aux
  hipStream_t cs(int j) const { return dc2[((j % dc_streams) + dc_streams) % dc_streams]; }
  uint8_t *res_stage = nullptr;  // device-side twin of the result arena: k_dc2_compact writes survivors there, a DMA copy takes them to the host
  size_t res_stage_bytes = 0;
  uint32_t *keep = nullptr, *keep_dev = nullptr;  // host-mapped survivor bits, keep_words per frame
  size_t keep_words = 0, keep_frames = 0;
  bool res_early = false;  // the arena holds every refined match, `keep` says which ones survive
  size_t res_slot = 0;     // bytes per frame in the arena
  Dc2Bank bank1[2];                    // pass-1 slabs: the chains of successive chunks alternate (the next one starts while the last still runs)
  static constexpr int kBanks = 4;
  Dc2Bank bank2[kBanks];
  // Host-resident inputs (Matcher::pushBack takes host pointers, viso/matcher.cpp:95-181): the frames cross PCIe in PIECES of
  // twenty frames - the pool gathers a piece into pinned memory (the caller's images are pageable: a copy straight out of them
  // is staged by the runtime at a fraction of the link's rate), whoever finishes a piece's last image enqueues its DMA copy
  // on a stream of its own - while the GPU works on what has arrived; only the first chunk's upload is not hidden.
  struct UpPiece {
    int32_t f0 = 0, n = 0;
    std::atomic<int> left{0};
    std::atomic<int> recorded{0};  // 1: copy + event are enqueued, -1: a HIP call failed
    hipEvent_t ev = nullptr;
    double t_recorded = 0, t_arrived = 0;
  };
  uint8_t *up_h = nullptr, *up_d = nullptr;
  size_t up_bytes = 0;
  // (measured on the MI355X box, tools/pcie_rate.py: one stream carries 52-57 GB/s host to device in pieces of 8 MB and more;
  // the same pieces alternating over two or three streams 28-40 GB/s)
  std::vector<std::unique_ptr<UpPiece>> up_pieces;
  Seq2Poller poller;
  std::vector<hipEvent_t> events;  // pool, reused across runs
  size_t ev_used = 0;
  // survivors of every frame land in one host-mapped arena; the getters read them there (vsm_handle::seq_view)
  uint8_t *res = nullptr, *res_dev = nullptr;
  size_t res_bytes = 0;
  int32_t *res_cnt = nullptr, *res_cnt_dev = nullptr;
  int res_frames = 0;
  std::vector<size_t> res_off;
  std::vector<std::unique_ptr<Seq2Chunk>> chunks;
  std::mutex enq_mu;                   // second parts are enqueued from pool threads
  hipEvent_t bank1_copied[2] = {nullptr, nullptr};  // a pass-1 slab's job table has been copied to the device (it is rewritten per use)
  int dc_streams = 3;                  // streams the final chains of successive chunks rotate over
  bool expect_long = false;            // a list of more than 8192 points has been seen (vsm_dc2_launch_prepare)
  std::mutex ev_mu;  // (events are also taken by pool threads: the second parts)
  hipEvent_t get_event() {
    std::lock_guard<std::mutex> lk(ev_mu);
    if (ev_used == events.size()) {
      hipEvent_t e = nullptr;
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
      events.push_back(e);
    }
    return events[ev_used++];
  }
  void release() {
    poller.shutdown();
    for (Dc2Bank &b : bank1) b.release();
    for (Dc2Bank &b : bank2) b.release();
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    events.clear();
    if (res) (void)hipHostFree(res);
    if (res_cnt) (void)hipHostFree(res_cnt);
    if (keep) (void)hipHostFree(keep);
    if (res_stage) vsm_dev_free(res_stage);
    if (up_h) (void)hipHostFree(up_h);
    if (up_d) vsm_dev_free(up_d);
    if (up) (void)hipStreamDestroy(up);
    if (aux) (void)hipStreamDestroy(aux);
    up = aux = ns = nullptr;
    if (tie_jobs_h) (void)hipHostFree(tie_jobs_h);
    if (tie_jobs_d) (void)hipFree(tie_jobs_d);
    tie_jobs_h = tie_jobs_d = nullptr;
    tie_jobs_cap = 0;
    for (hipStream_t &s : dc2)
      if (s) (void)hipStreamDestroy(s);
  }
};

static void seq2_destroy(vsm_handle *h) {
  h->seq_v2_frames = 0;
  if (!h->seq2) return;
  if (h->seq2->up) (void)hipStreamSynchronize(h->seq2->up);
  (void)hipStreamSynchronize(h->seq2->ns);  // (the fifth stream carries the exports and the device's vertex sorts)
  for (hipStream_t s : h->seq2->dc2)
    if (s) (void)hipStreamSynchronize(s);
  h->seq2->release();
  delete h->seq2;
  h->seq2 = nullptr;
}

// the gaps of list i of a chunk closed in place (the survivor bits are there): runs of consecutive survivors move in one piece
static void seq2_close_gaps(Seq2Chunk *ch, vsm_handle *h, int i) {
  Seq2 &S = *h->seq2;
  const int32_t f = ch->f0 + i;
  const int32_t cnt = std::max(S.res_cnt[f], 0), n_all = std::max(0, std::min(ch->B->list_n(i), ch->B->cap));
  vsm_p_match *rec = (vsm_p_match *)(S.res + S.res_off[f]);
  const uint32_t *keep = S.keep + S.keep_words * (size_t)f;
  // runs of consecutive survivors move in one piece each (a list loses a match in twelve or so: runs of a few hundred bytes)
  int32_t k = 0, e = 0;
  while (e < n_all && k < cnt) {
    uint32_t bits = keep[e >> 5] >> (e & 31);
    if (!(bits & 1u)) {  // skip the dropped matches up to the next survivor (or the end of the word)
      const int32_t skip = bits ? __builtin_ctz(bits) : 32 - (e & 31);
      e += skip;
      continue;
    }
    // length of the run of ones from e on, across words
    int32_t run = 0;
    for (;;) {
      const int32_t room = 32 - ((e + run) & 31);
      const uint32_t inv = ~(keep[(e + run) >> 5] >> ((e + run) & 31));
      const int32_t ones = (inv & (room == 32 ? 0xffffffffu : ((1u << room) - 1u))) ? __builtin_ctz(inv) : room;
      run += ones;
      if (ones < room || e + run >= n_all) break;
    }
    run = std::min(run, std::min(n_all - e, cnt - k));
    if (k != e) memmove(rec + k, rec + e, (size_t)run * sizeof(vsm_p_match));
    k += run;
    e += run;
  }
  h->seq_view[f].p = rec;
  h->seq_view[f].n = k;
}

// A chunk's chain is through.  The call has to end with every frame's p_matched in host memory as 48-byte p_match records
// (viso/matcher.h:86-100), like Matcher::matchFeatures leaves it (viso/matcher.cpp:229-232).
static void seq2_chunk_done(void *arg) {  // (the poller thread has seen the chain's last event)
  Seq2Chunk *ch = (Seq2Chunk *)arg;
  vsm_handle *h = ch->h;
  ch->t_done = vsm_now_us();
  Seq2 &S0 = *h->seq2;
  if (!S0.res_early) {  // the arena holds the survivors as the device compacted them: hand out views, nothing to copy
    for (int i = 0; i < ch->n; i++) {
      const int32_t f = ch->f0 + i;
      h->seq_view[f].p = (const vsm_p_match *)(S0.res + S0.res_off[f]);
      h->seq_view[f].n = std::max(S0.res_cnt[f], 0);
    }
    ch->state.store(3, std::memory_order_release);
    return;
  }
  // The arena holds every refined match of the chunk's frames (they crossed PCIe while the chain was triangulating) and one
  // bit per match says which ones survived: the pool closes the gaps in place, one frame per task (a move of what follows
  // the first dropped match), and the getters read the arena.
  const int n = std::max(ch->n, 1);
  ch->unpack_left.store(n, std::memory_order_relaxed);
  if (ch->warm && ch->n > 0) {  // (lists by L3 domain: a task takes what its own domain has read, then whatever is left)
    const int T = std::min(std::max(h->pool->size() - 1, 1), ch->n);
    // (counted in tasks: a task that finds every list taken still reads the chunk, so the chunk is done when the last task is)
    ch->unpack_left.store(T, std::memory_order_relaxed);
    h->pool->submit(T, [ch, h](int) {
      const int dom = vsm_thread_domain();
      for (int pass = 0; pass < 2; pass++)
        for (int i = 0; i < ch->n; i++) {
          if (pass == 0 && (int)ch->warm_domain[i].load(std::memory_order_relaxed) != dom) continue;
          if (ch->warm_claim[i].exchange(1, std::memory_order_acq_rel)) continue;
          seq2_close_gaps(ch, h, i);
        }
      if (ch->unpack_left.fetch_sub(1, std::memory_order_acq_rel) == 1) {
        ch->t_ready = vsm_now_us();
        ch->state.store(3, std::memory_order_release);
      }
    }, true);
    return;
  }
  h->pool->submit(n, [ch, h](int i) {
    if (i < ch->n) seq2_close_gaps(ch, h, i);
    if (ch->unpack_left.fetch_sub(1, std::memory_order_acq_rel) == 1) {
      ch->t_ready = vsm_now_us();
      ch->state.store(3, std::memory_order_release);
    }
  }, true);
}

// second part of a chunk's final chain (tie patches, votes, survivors): enqueued by whoever opens the gate last - the pool
// thread that finished the chunk's last vertex sort, or the caller's thread when it has recorded the refinement's event
static void seq2_enqueue_second_part(Seq2Chunk *ch) {
  vsm_handle *h = ch->h;
  std::lock_guard<std::mutex> lk(h->seq2->enq_mu);
  (void)hipSetDevice(h->device);
  ch->t_sorted = vsm_now_us();
  // (on the chain's own stream: with three side streams the next chain that uses it is chunk k + 3's, enqueued three chunks
  // later - by then this second part is normally in; the mesh event keeps the order where it is not)
  hipStream_t s = ch->stream;
  bool ok = hipStreamWaitEvent(s, ch->ev_mesh, 0) == hipSuccess;
  if (ok && ch->ev_ties) ok = hipStreamWaitEvent(s, ch->ev_ties, 0) == hipSuccess;
  if (ok && ch->ev_exp) ok = hipStreamWaitEvent(s, ch->ev_exp, 0) == hipSuccess;
  if (ok) {
    dc2_enqueue_votes(s, *ch->B, ch->n, ch->max_list, ch->method, ch->ftol, ch->dtol, h->prof, true);
    Seq2 &S = *h->seq2;
    const size_t row = std::min((size_t)std::max(ch->max_list, 0) * sizeof(vsm_p_match), S.res_slot);
    if (!S.res_early && row > 0)  // the survivors were written in HBM: one strided DMA copy takes the chunk's lists to the arena
      ok = hipMemcpy2DAsync(S.res + S.res_off[ch->f0], S.res_slot, S.res_stage + S.res_off[ch->f0], S.res_slot, row, (size_t)ch->n, hipMemcpyDeviceToHost,
                            s) == hipSuccess;
    // (who sees the chain's end: Seq2Poller)
    hipEvent_t ev_done = ok ? h->seq2->get_event() : nullptr;
    ok = ok && ev_done && hipGetLastError() == hipSuccess && hipEventRecord(ev_done, s) == hipSuccess;
    if (ok) {
      // (before the task can run: it ends in state 3, and a store of 2 behind it would undo that)
      ch->state.store(2, std::memory_order_release);
      h->seq2->poller.add(ev_done, [ch](bool done) {
        if (!done) ch->hip_error.store(1);
        seq2_chunk_done(ch);
      });
    }
  }
  if (!ok) {
    ch->hip_error.store(1);
    (void)hipStreamSynchronize(s);
    (void)hipStreamSynchronize(ch->stream);
    ch->state.store(3, std::memory_order_release);
    return;
  }
}
static inline void seq2_open_gate(Seq2Chunk *ch) {
  if (ch->gate.fetch_sub(1, std::memory_order_acq_rel) == 1) seq2_enqueue_second_part(ch);
}

// (the poller thread has seen a copy's event: the keys of the chunk's lists first .. last - 1 are in host memory; the copy
// comes in pieces, so that the pool starts on the first lists while the others still cross)
static void seq2_keys_ready(Seq2Chunk *ch, int first, int last) {
  vsm_handle *h = ch->h;
  if (ch->t_keys == 0) ch->t_keys = vsm_now_us();
  const int ntask = std::max(last - first, 1);  // (no list for the pool: one task that only hands over)
  h->pool->submit(ntask, [ch, first, last](int t) {
    const double t0 = vsm_now_us();
    Dc2Bank &B = *ch->B;
    const int i = first + t;
    if (i < last) B.sort_ties_of(i);
    ch->sort_ns.fetch_add((long long)((vsm_now_us() - t0) * 1e3), std::memory_order_relaxed);
    if (ch->sort_tasks_left.fetch_sub(1, std::memory_order_acq_rel) == 1) {
      ch->sorts_left.fetch_sub(1, std::memory_order_acq_rel);
      const bool warm = ch->warm;
      const int nw_tasks = ch->n;
      if (warm) ch->warm_left.store(nw_tasks, std::memory_order_release);  // (before the gate opens: the chunk cannot end first)
      seq2_open_gate(ch);
      if (warm) {  // (the pool is idle until this chunk's survivor bits arrive: see Seq2Chunk::warm)
        vsm_handle *h2 = ch->h;
        h2->pool->submit(nw_tasks, [ch, h2](int j) {
          if (!ch->warm_claim[j].load(std::memory_order_acquire)) {  // (a list whose gaps are being closed already needs no warming)
            Seq2 &S = *h2->seq2;
            const int32_t f = ch->f0 + j;
            const int32_t n_all = std::max(0, std::min(ch->B->list_n(j), ch->B->cap));
            const volatile uint64_t *p = (const volatile uint64_t *)(S.res + S.res_off[f]);
            uint64_t acc = 0;
            for (size_t w = 0, nw = (size_t)n_all * sizeof(vsm_p_match) / 8; w < nw; w += 8) acc += p[w];  // (one word per 64-byte line)
            (void)acc;
            ch->warm_domain[j].store((signed char)vsm_thread_domain(), std::memory_order_release);
          }
          ch->warm_left.fetch_sub(1, std::memory_order_acq_rel);  // (the last access to the chunk)
        });
      }
    }
  }, true);  // (in front of everything else the pool has: the chains wait for these)
}

// helper: the pool of a caller that has nothing left to enqueue - it takes tasks itself instead of sleeping (the end of a call
// is host work: the last chunk's vertex sorts and the closing of the gaps in its lists)
static bool seq2_wait_chunk(Seq2Chunk *ch, double timeout_us, VsmPool *helper = nullptr) {
  const double t0 = vsm_now_us();
  while ((ch->state.load(std::memory_order_acquire) != 3 && ch->state.load(std::memory_order_acquire) != 0) ||
         ch->warm_left.load(std::memory_order_acquire) > 0) {
    if (helper) {
      if (!helper->help()) std::this_thread::yield();
    } else {
      std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    if (vsm_now_us() - t0 > timeout_us) return false;
  }
  return true;
}

// Whatever way a look-ahead call is left, nothing of it may still be running: the last data member of Seq2Call, so that it
// waits - for the pool's tasks, the poller's, the streams - BEFORE anything else of the call is destroyed.
struct Seq2Drain {
  vsm_handle *h = nullptr;  // set = armed (sequence_run_v2: when the buffers exist, before the first upload task); until then the set-up's returns wait for nothing
  ~Seq2Drain() {
    if (!h) return;
    Seq2 &S = *h->seq2;
    for (auto &pc : S.up_pieces)  // (the gathers read the caller's images; the task that takes `left` to zero enqueues the piece's
                                  // DMA copy AFTERWARDS and says so in `recorded`: only then is everything of the piece on the stream)
      while (pc->left.load(std::memory_order_acquire) > 0 || pc->recorded.load(std::memory_order_acquire) == 0)
        if (!h->pool->help()) std::this_thread::yield();
    if (S.up) {  // (the upload stream lives for the host-fed call only: idle streams keep a share of a hardware queue)
      (void)hipStreamSynchronize(S.up);
      (void)hipStreamDestroy(S.up);
      S.up = nullptr;
    }
    for (auto &ch : S.chunks) {
      if (ch->state.load() == 1 && !ch->caller_gate) {  // left before the caller's half of the gate was opened: only the sorts are on their way
        (void)hipStreamSynchronize(ch->stream);
        const double t0 = vsm_now_us();
        while (ch->gate.load() > 1 && vsm_now_us() - t0 < 5e6) std::this_thread::sleep_for(std::chrono::microseconds(50));
        while (ch->warm_left.load() > 0 && vsm_now_us() - t0 < 10e6)  // (the last sort queued warm-up tasks behind the gate)
          if (!h->pool->help()) std::this_thread::yield();
        ch->state.store(0);
        continue;
      }
      if (!seq2_wait_chunk(ch.get(), 30e6)) {
        fprintf(stderr, "visomatch: the final stage of a look-ahead chunk did not complete: %s\n", hipGetErrorString(hipStreamQuery(ch->stream)));
        fprintf(stderr, "  chunk %d: state %d gate %d sorts_left %d unpack_left %d warm_left %d hip_error %d; events: keys %s, mesh %s, exp %s, ref %s\n", ch->k,
                ch->state.load(), ch->gate.load(), ch->sorts_left.load(), ch->unpack_left.load(), ch->warm_left.load(), ch->hip_error.load(),
                ch->ev_keys ? hipGetErrorString(hipEventQuery(ch->ev_keys)) : "-", ch->ev_mesh ? hipGetErrorString(hipEventQuery(ch->ev_mesh)) : "-",
                ch->ev_exp ? hipGetErrorString(hipEventQuery(ch->ev_exp)) : "-", ch->ev_ref ? hipGetErrorString(hipEventQuery(ch->ev_ref)) : "-");
        (void)hipStreamSynchronize(ch->stream);
        while (ch->sorts_left.load() > 0 || ch->unpack_left.load() > 0 || ch->warm_left.load() > 0)
          std::this_thread::sleep_for(std::chrono::microseconds(50));
      }
    }
    for (int i = 0; i < S.dc_streams; i++) (void)hipStreamSynchronize(S.dc2[i]);
    (void)hipStreamSynchronize(S.ns);
    (void)hipStreamSynchronize(h->stream);
  }
};

static bool seq2_make_stream(hipStream_t &st) { return st || hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess; }  // (priorities - main stream high, side streams low - change nothing: measured again in round 4)
// returns VSM_OK, an error, or VSM_SEQ2_DECLINED when this path does not take the run (the caller uses the first form)
#define VSM_SEQ2_DECLINED 1000
// One call of the GPU-resident form: what its steps share, by role, and the steps; sequence_run_v2 below is their order.
// The object lives on the caller's stack for the duration of the call, and only the caller's thread touches it.
//
// LIFETIME RULE.  A task handed to the pool (submit), to the poller or to a stream callback may outlive the step that made
// it - and, on an error return, everything but the drain's wait - so it holds only what outlives the call: vsm_handle*,
// Seq2*, Seq2Chunk*, Seq2::UpPiece*, and plain values (the caller's image pointers among them, which the caller keeps
// until the call returns).  It never holds this object, a reference into it or a [&] capture.  The one exception is a
// blocking pool->run, whose closure is dead when it returns (finish_chain1).  `drain` is the LAST data member and so the
// first to be destroyed: while it waits, every other member is still there - and by the rule nobody needs them.
struct Seq2Call {
  // Frame banks: the features run two chunks ahead of the second matching pass, and a chunk's first pair reads the previous
  // chunk's last frame: chunks k-1 .. k+2 are alive at once, and the bank of chunk k+3 must not be the one chunk k-1's chain
  // still reads.  Pair banks: a chunk's lists are read until its final chain is done (wait_for_chunk).
  static constexpr int kPairBanks = 4, kFrameBanks = 5;
  struct Ck {  // a chunk as the caller's thread sees it (no task holds one - the rule above - so nothing in it is shared: plain members)
    int32_t f0 = 0;
    int n = 0, first_img = 0, first_pair = 0;
    int max_nq[2] = {0, 0};
    hipEvent_t ev_prior = nullptr, ev_p1 = nullptr;
    hipEvent_t ev_k1 = nullptr;   // pass-1 chain with the vertex sorts on the pool: its keys are in host memory (chain stream)
    bool chain1_open = false;     // ... and its second part (tie patches, votes, boxes) is not enqueued yet (finish_chain1)
  };
  // --- inputs and references
  vsm_handle *const h;
  Seq2 &S;
  VsmCtx &c;
  const vsm_params &p;
  const VsmSwitches &sw;
  const uint8_t *const left, *const right;
  const int64_t frame_stride;
  const int on_device;
  const int32_t n_frames, w, hh, bpl, method;
  const double *const Tr;
  const uint8_t *const Tr_valid;
  // Mono input (right == NULL, flow matching: Matcher::pushBack(I1, dims, replace) + matchFeatures(0), viso/matcher.h:118,
  // viso/matcher.cpp:1006-1041) runs the same pipeline over one image per frame: image ids are then consecutive per frame
  // instead of (left, right) pairs.
  const int sides = right ? 2 : 1;
  // --- the plan: const once the set-up is through
  const bool host_in = !on_device;
  // (vsm_api.cpp: VsmSwitches; 0 = stores of k_dc2_keys, which fused_keys does not run: 1 then)
  const int keys_dma = sw.seq_keys_dma >= 0 ? ((sw.seq_keys_dma == 0 && sw.fused_keys && p.refinement != 2) ? 1 : sw.seq_keys_dma) : (h->pool->size() >= 10 ? 2 : 1);
  const Seq2Plan plan = seq2_plan(n_frames, h->pool->size(), host_in, sw.seq_chunk, sw.seq_first_chunk, getenv("VSM_SEQ_PLAN"));
  const int C = plan.C;
  const std::vector<int32_t> &chunk_start = plan.start;
  const int nchunks = (int)chunk_start.size() - 1;
  // option "seq_host_pinned": the caller vouches that its images lie in page-locked memory (hipHostMalloc, or registered once
  // with vsm_host_register / hipHostRegister): the pieces then cross by DMA straight out of them - no gather pass of the pool
  // (2.2 ms of its time per 200 frames), no pinned twin - enqueued here, all at once, in frame order
  const bool host_pinned = host_in && sw.seq_host_pinned;
  const bool inorder = host_in && !sw.seq_serial && sw.seq_host_inorder;
  // (pass-1 vertex sorts on the pool: ranks with ten pool threads and more, frames in HBM; option seq_ties1_host 0 / 1)
  const bool ties1_host = p.multi_stage && !sw.seq_serial && (sw.seq_ties1_host >= 0 ? sw.seq_ties1_host != 0 : (h->pool->size() >= 10 && !host_in));
  // seq_serial (VSM_SEQ_SERIAL=1, measurements): nothing overlaps - every group of launches drains before the next one is
  // enqueued, so each kernel's HIP-event time is its time with the GPU to itself (bench.py's "alone" figures).  Same
  // kernels, same data, same results.
  const bool serial = sw.seq_serial;
  // Option fused_keys: a chain's keys are written by the compaction of the matching pass in front of it, into the PAIR bank
  // (VsmPair::keys), and its job table is uploaded before that pass is launched - behind the compaction's event the chain
  // starts on its first real work.  Who guards the key arrays: the rule of the lists they lie beside - a pair bank comes round
  // after kPairBanks chunks and run_ahead / the in-order loop wait for the chunk that used it last (wait_for_chunk); a chain
  // slab (bank1[k & 1]) would not do, the first pass of chunk k runs while chunk k - 2's pass-1 chain may still read its slab.
  // (refinement = 2 shortens the lists behind the compaction: its chains make their keys themselves, k_dc2_keys behind ev_ref)
  const bool fused = sw.fused_keys && p.refinement != 2;
  const int gpu_sorts_default = h->pool->size() <= 2 ? 67 : (h->pool->size() == 3 ? 50 : (h->pool->size() == 4 ? 33 : 0));  // (four threads: 7.0 ms without a share, 8.3 with one)
  const bool split_sorts = nchunks == 2 && sw.seq_gpu_sorts < 0 && gpu_sorts_default > 0 && !serial;
  const bool p2_first = sw.seq_p2_first >= 0 ? sw.seq_p2_first != 0 : (h->pool->size() >= 5 && h->pool->size() < 10 && (sw.seq_gpu_sorts >= 0 ? sw.seq_gpu_sorts : gpu_sorts_default) == 0);
  const size_t img_bytes = (size_t)w * hh;
  size_t slot = 0;  // bytes per frame in the result arena (setup_results)
  // --- cursors: the caller's thread only
  std::vector<Ck> ck = std::vector<Ck>(nchunks);
  int32_t nprev[2][2] = {{0, 0}, {0, 0}};
  int chain1_next = 0;  // first chunk whose pass-1 chain has not been enqueued yet
  int chain_next = 0;  // first chunk whose final chain has not been enqueued yet
  int refine_pending = -1;  // chunk whose refinement waits for the next chunk's matching (seq_defer_refine)
  int exp_k = 0;  // first chunk with rows left to submit
  std::vector<int> ties_pending;   // chunks whose device share has not been launched yet
  // A sorting wave wants 139 KB of LDS, i.e. a compute unit to itself, and finds none while a block-kernel launch has five
  // workgroups on every unit: the triangulations that are enqueued behind the launch wait for this event - recorded right
  // in front of the sort kernel on its stream - so that the sorts are placed first and the meshes share what is left.
  hipEvent_t ev_ties_go = nullptr;
  int tie_jobs_at = 0;  // rows of the job table this call's launches have used (every launch its own rows: no launch waits for another's copy)
  double tstart = 0, tg = 0;  // the call's start; what the caller's thread has spent waiting (seq_timings[0])
  std::vector<double> dbg_counts, dbg_main;  // (VSM_DEBUG_TIMING: when the caller's thread had a chunk's counts / had enqueued its second pass)
  Seq2Drain drain;  // LAST: see the rule above

  Seq2Call(vsm_handle *h_, const uint8_t *left_, const uint8_t *right_, int64_t frame_stride_, int on_device_, int32_t n_frames_, int32_t w_, int32_t hh_,
           int32_t bpl_, int32_t method_, const double *Tr_, const uint8_t *Tr_valid_)
      : h(h_), S(*h_->seq2), c(h_->seq), p(h_->param), sw(h_->sw), left(left_), right(right_), frame_stride(frame_stride_), on_device(on_device_),
        n_frames(n_frames_), w(w_), hh(hh_), bpl(bpl_), method(method_), Tr(Tr_), Tr_valid(Tr_valid_) {}

  // set-up, in three steps that return VSM_OK, an error or VSM_SEQ2_DECLINED: the context and the streams ...
  int setup_streams() {
    if (!c.holds(w, hh, kFrameBanks * C, kPairBanks * C) || h->seq_chunk != C) {
      (void)hipStreamSynchronize(h->stream);
      int rc = ctx_create(c, p, w, hh, kFrameBanks * C, kPairBanks * C, h->stream, h->sw.match_heads != 0);
      if (rc != VSM_OK) return rc;
      h->seq_chunk = C;
    }
    if ((size_t)c.dims.ub * c.dims.vb > 1024) return VSM_SEQ2_DECLINED;  // (k_dc2_prior keeps the bins' minima and maxima in LDS)

    // (only the streams this run uses: the runtime deals its hardware queues out per stream, idle ones included, and a stream
    // that shares a hardware queue with another one runs in turns with it)
    S.poller.start(h->device, h->aff, h->pool->size() >= 10);
    // (host-resident inputs: the copy stream is one of the five, so the chains rotate over two streams - with a sixth stream in
    // the process two of them share a hardware queue and run in turns: 8.5-9.4 ms per 200 frames against 7.5-7.9; an idle
    // stream keeps its queue, so the third one is given back)
    S.dc_streams = host_in ? std::min(2, sw.seq_dc_streams) : sw.seq_dc_streams;
    for (int i = S.dc_streams; i < 4; i++)
      if (S.dc2[i]) {
        (void)hipStreamSynchronize(S.dc2[i]);
        (void)hipStreamDestroy(S.dc2[i]);
        S.dc2[i] = nullptr;
      }
    for (int i = 0; i < S.dc_streams; i++)
      if (!seq2_make_stream(S.dc2[i])) return VSM_SEQ2_DECLINED;
    if (sw.seq_null_stream) {
      S.ns = nullptr;
    } else {
      if (!seq2_make_stream(S.aux)) return VSM_SEQ2_DECLINED;
      S.ns = S.aux;
    }

    S.ev_used = 0;
    S.bank1_copied[0] = S.bank1_copied[1] = nullptr;
    return VSM_OK;
  }
  // ... the result arena, `keep` and `res_stage` ...
  int setup_results() {
    // result arena: one slot of `slot` matches per frame (no list is longer than its query count, which the host only
    // learns chunk by chunk: the dense feature capacity bounds it)
    slot = c.list_slot_bytes();
    if (S.res_bytes < slot * n_frames || S.res_frames < n_frames) {
      if (S.res) (void)hipHostFree(S.res);
      if (S.res_cnt) (void)hipHostFree(S.res_cnt);
      S.res = nullptr;
      S.res_cnt = nullptr;
      S.res_bytes = 0;
      if (hipHostMalloc((void **)&S.res, slot * n_frames, hipHostMallocMapped) != hipSuccess ||
          hipHostGetDevicePointer((void **)&S.res_dev, S.res, 0) != hipSuccess ||
          hipHostMalloc((void **)&S.res_cnt, (size_t)n_frames * 4, hipHostMallocMapped) != hipSuccess ||
          hipHostGetDevicePointer((void **)&S.res_cnt_dev, S.res_cnt, 0) != hipSuccess) {
        (void)hipGetLastError();
        return VSM_SEQ2_DECLINED;
      }
      S.res_bytes = slot * n_frames;
      S.res_frames = n_frames;
    }
    memset(S.res_cnt, 0, (size_t)n_frames * 4);
    // Result form.  Either the device compacts the survivors as 48-byte p_match records in HBM (res_stage) and one strided DMA
    // copy per chain takes them into the host-mapped arena - no host-side work at all -, or (res_early) the refined lists cross
    // PCIe as they are while the chain still triangulates, the chain ends with one survivor bit per match, and the pool closes
    // the gaps in the arena.  The getters read the arena either way.  (Round 2's 24-byte packed records, expanded by the pool
    // inside the call: 5.9 / 12.4 ms per 200 frames with 14 / 4 pool threads against 5.4 / 8.8 - removed.)
    // closing the gaps costs the pool ~30 us per list: worth it where the pool has threads to spare (measured: 5.4 against 5.6 ms per
    // 200 frames with 14 threads, 9.1 against 8.8 with 4, 11.4 against 9.0 with 1)
    S.res_early = sw.seq_early_export < 0 ? h->pool->size() >= 6 : sw.seq_early_export != 0;
    if (S.res_early) {
      const size_t kw = ((size_t)c.cap_set[1] + 31) / 32 + 1;
      if (S.keep_words < kw || S.keep_frames < (size_t)n_frames) {
        if (S.keep) (void)hipHostFree(S.keep);
        S.keep = nullptr;
        S.keep_words = S.keep_frames = 0;
        if (hipHostMalloc((void **)&S.keep, kw * n_frames * 4, hipHostMallocMapped) != hipSuccess ||
            hipHostGetDevicePointer((void **)&S.keep_dev, S.keep, 0) != hipSuccess) {
          (void)hipGetLastError();
          return VSM_SEQ2_DECLINED;
        }
        S.keep_words = kw;
        S.keep_frames = (size_t)n_frames;
      }
    }
    if (S.res_stage_bytes < slot * n_frames) {  // survivors are written in HBM and cross PCIe by DMA copies
      if (S.res_stage) vsm_dev_free(S.res_stage);
      S.res_stage = nullptr;
      S.res_stage_bytes = 0;
      if (vsm_dev_alloc((void **)&S.res_stage, slot * n_frames) != hipSuccess) {
        (void)hipGetLastError();
        return VSM_SEQ2_DECLINED;
      }
      S.res_stage_bytes = slot * n_frames;
    }
    S.res_slot = slot;
    S.res_off.assign(n_frames, 0);
    for (int32_t f = 0; f < n_frames; f++) S.res_off[f] = slot * f;
    S.chunks.clear();
    h->seq_hip_error.store(0);
    return VSM_OK;
  }
  // ... and, for host-resident inputs, the upload buffers and the pieces the frames cross in
  int setup_uploads() {
    S.up_pieces.clear();
    if (!host_in) return VSM_OK;
    const size_t need = (size_t)sides * n_frames * img_bytes;
    if (S.up_bytes < need || (!host_pinned && !S.up_h)) {
      if (S.up) HIPCHK(hipStreamSynchronize(S.up));
      if (S.up_h) (void)hipHostFree(S.up_h);
      if (S.up_d) vsm_dev_free(S.up_d);
      S.up_h = S.up_d = nullptr;
      S.up_bytes = 0;
      if ((!host_pinned && hipHostMalloc((void **)&S.up_h, need, hipHostMallocDefault) != hipSuccess) || vsm_dev_alloc((void **)&S.up_d, need) != hipSuccess) {
        (void)hipGetLastError();
        return VSM_SEQ2_DECLINED;
      }
      S.up_bytes = need;
    }
    if (!seq2_make_stream(S.up)) return VSM_SEQ2_DECLINED;
    // pieces of at most `per` frames, none across a chunk boundary (a chunk's features wait for its pieces only)
    // (a copy + its event cost ~50 us of the copy stream on top of the transfer: 20 frames = 18.6 MB = 0.33 ms at the link's 57 GB/s)
    constexpr int32_t per = 20;
    {
      // (pieces enter S.up_pieces - where Drain waits for them - only once every one of them has its event, i.e. right before
      // their tasks are submitted: a piece without tasks would never count down)
      std::vector<std::unique_ptr<Seq2::UpPiece>> pieces;
      for (int k = 0; k < nchunks; k++)
        for (int32_t f = chunk_start[k]; f < chunk_start[k + 1]; f += per) {
          std::unique_ptr<Seq2::UpPiece> pc(new Seq2::UpPiece());
          pc->f0 = f;
          pc->n = std::min<int32_t>(per, chunk_start[k + 1] - f);
          pc->left.store(sides * pc->n, std::memory_order_relaxed);
          pc->ev = S.get_event();
          if (!pc->ev) return VSM_EHIP;
          pieces.push_back(std::move(pc));
        }
      S.up_pieces = std::move(pieces);
    }
    return host_pinned ? enqueue_pinned_pieces() : submit_gathers();
  }
  int enqueue_pinned_pieces() {
    for (auto &pcu : S.up_pieces) {
      Seq2::UpPiece *pc = pcu.get();
      bool ok = true;
      for (int side = 0; side < sides && ok; side++) {
        // (device layout of this form: PLANAR - all left images, then all right images - so that a piece of contiguous
        // frames is ONE linear copy per side: the DMA engine runs linear copies at the link's rate, pitched ones at a
        // fraction of it)
        const uint8_t *src = (side ? right : left) + (size_t)pc->f0 * frame_stride;
        uint8_t *dst = S.up_d + ((size_t)side * n_frames + pc->f0) * img_bytes;
        if (bpl == w && (size_t)frame_stride == img_bytes) {
          ok = hipMemcpyAsync(dst, src, img_bytes * (size_t)pc->n, hipMemcpyHostToDevice, S.up) == hipSuccess;
        } else if (bpl == w) {  // an image is one row of the copy
          ok = hipMemcpy2DAsync(dst, img_bytes, src, (size_t)frame_stride, img_bytes, (size_t)pc->n, hipMemcpyHostToDevice, S.up) == hipSuccess;
        } else {
          for (int32_t i = 0; i < pc->n && ok; i++)
            ok = hipMemcpy2DAsync(dst + (size_t)i * img_bytes, (size_t)w, src + (size_t)i * frame_stride, (size_t)bpl, (size_t)w, (size_t)hh,
                                  hipMemcpyHostToDevice, S.up) == hipSuccess;
        }
      }
      ok = ok && hipEventRecord(pc->ev, S.up) == hipSuccess;
      pc->t_recorded = vsm_now_us();
      pc->left.store(0, std::memory_order_release);
      pc->recorded.store(ok ? 1 : -1, std::memory_order_release);
      if (ok && vsm_debug_timing()) S.poller.add(pc->ev, [pc](bool) { pc->t_arrived = vsm_now_us(); });
      if (!ok) {  // (nothing will ever count the other pieces down: Drain must not wait for them)
        for (auto &rest : S.up_pieces)
          if (rest->recorded.load() == 0) {
            rest->left.store(0, std::memory_order_release);
            rest->recorded.store(-1, std::memory_order_release);
          }
        return VSM_EHIP;
      }
    }
    return VSM_OK;
  }
  int submit_gathers() {
    for (auto &pcu : S.up_pieces) {
      Seq2::UpPiece *pc = pcu.get();
      h->pool->submit(sides * pc->n, [h = h, pc, left = left, right = right, frame_stride = frame_stride, bpl = bpl, w = w, hh = hh, sides = sides, img_bytes = img_bytes](int t) {  // (by value: the rule)
        Seq2 &S2 = *h->seq2;
        const int32_t f = pc->f0 + t / sides;
        const int side = t % sides;
        const uint8_t *src = (side ? right : left) + (size_t)f * frame_stride;
        uint8_t *dst = S2.up_h + ((size_t)sides * f + side) * img_bytes;
        if (bpl == w) {
          memcpy(dst, src, img_bytes);
        } else {
          for (int32_t v = 0; v < hh; v++) memcpy(dst + (size_t)v * w, src + (size_t)v * bpl, w);
        }
        if (pc->left.fetch_sub(1, std::memory_order_acq_rel) == 1) {  // the piece is in pinned memory: its DMA copy
          std::lock_guard<std::mutex> lk(S2.enq_mu);
          (void)hipSetDevice(h->device);
          const size_t off = (size_t)sides * pc->f0 * img_bytes, bytes = (size_t)sides * pc->n * img_bytes;
          const bool ok = hipMemcpyAsync(S2.up_d + off, S2.up_h + off, bytes, hipMemcpyHostToDevice, S2.up) == hipSuccess &&
                          hipEventRecord(pc->ev, S2.up) == hipSuccess;
          pc->t_recorded = vsm_now_us();
          pc->recorded.store(ok ? 1 : -1, std::memory_order_release);
        }
      });
    }
    return VSM_OK;
  }
  hipError_t launch_features_of(int k) {
    const int32_t f0 = chunk_start[k];
    const int n = chunk_start[k + 1] - f0;
    const int first_img = sides * (k % kFrameBanks) * C;
    if (on_device) {
      enqueue_front_frames(h, c, first_img, sides, left + (size_t)f0 * frame_stride, (size_t)frame_stride, right ? right + (size_t)f0 * frame_stride : nullptr,
                           (size_t)frame_stride, bpl, n);
    } else {
      for (auto &pc : S.up_pieces) {  // the chunk's pieces: their copies are (being) enqueued by the pool
        if (pc->f0 < f0 || pc->f0 >= f0 + n) continue;
        int r;
        while ((r = pc->recorded.load(std::memory_order_acquire)) == 0)
          if (!h->pool->help()) std::this_thread::yield();
        if (r < 0) return hipErrorUnknown;
        const hipError_t e = hipStreamWaitEvent(h->stream, pc->ev, 0);
        if (e != hipSuccess) return e;
      }
      // (the pieces arrive row-tight; page-locked input is planar - left images, then right images -, gathered input frame by frame)
      if (host_pinned)
        enqueue_front_frames(h, c, first_img, sides, S.up_d + (size_t)f0 * img_bytes, img_bytes, S.up_d + ((size_t)n_frames + f0) * img_bytes, img_bytes, w, n);
      else
        enqueue_front_frames(h, c, first_img, sides, S.up_d + (size_t)sides * f0 * img_bytes, img_bytes, S.up_d + ((size_t)sides * f0 + 1) * img_bytes, 2 * img_bytes,
                             w, n);
    }
    enqueue_features(h, c, first_img, sides * n);
    return hipEventRecord(h->seq_ev[0], h->stream);
  }
  // jobs of chunk k from its feature counts, pass 1 and the pass-1 chain
  int start_chunk(int k) {  // (VSM_SEQ2_DECLINED: a list of this chunk is longer than this form takes)
    Ck &q = ck[k];
    q.f0 = chunk_start[k];
    q.n = chunk_start[k + 1] - q.f0;
    q.first_img = sides * (k % kFrameBanks) * C;
    q.first_pair = (k % kPairBanks) * C;
    const int n = q.n, first_img = q.first_img, first_pair = q.first_pair;
    const VsmPair *d_pairs = c.d_pairs + first_pair;
    VsmJob *h_jobs = c.h_jobs + first_pair, *d_jobs = c.d_jobs + first_pair;
    // (the caller's thread is about to wait for this chunk's features: the pass-1 chains of the chunks in front that wait for
    // their vertex sorts get them now - their keys are long there - instead of when their second pass is enqueued, 0.2 ms later)
    for (int j = 0; j < k; j++) {
      const int rc = finish_chain1(j);
      if (rc != VSM_OK) return rc;
    }
    const double t0 = now_us();
    HIPCHK(hipEventSynchronize(h->seq_ev[0]));  // the chunk's feature counts are in host-mapped memory
    HIPCHK(hipGetLastError());
    tg += now_us() - t0;
    dbg_counts.push_back(now_us());
    seq_chunk_jobs(p, method, sides, q.f0, n, first_img, seq_slot_before(chunk_start, k, sides, kFrameBanks, C), c.hm_counts, nprev, Tr, Tr_valid, h_jobs,
                   nullptr, q.max_nq, h->seq_src.data());
    if (!vsm_chain_fits(p, q.max_nq, VSM_DC_TIE_POINTS)) {
      return VSM_SEQ2_DECLINED;  // (a pass-1 list longer than the device's vertex sort takes: the first form does this run)
    }
    HIPCHK(vsm_upload(h->stream, d_jobs, h_jobs, sizeof(VsmJob) * n));
    if (p.multi_stage) {
      if (fused) {  // (the pass-1 chain's job table: everything in it is known now)
        const int rc = upload_chain1_jobs(k);
        if (rc != VSM_OK) return rc;
      }
      VsmMatchCfg cfg = make_cfg(p, method, h->sw.match_heads && c.has_heads);
      VsmJob dummy;
      memset(&dummy, 0, sizeof(dummy));
      cfg.sparse = 1;
      cfg.use_prior = 0;
      const VsmKeyOut ko = {nullptr, 0, 0};  // (the keys the pool sorts leave by a DMA copy, start_chain1)
      vsm_launch_match(h->stream, h->prof, c.d_imgs, d_pairs, d_jobs, dummy, n, c.dims, cfg, q.max_nq[0], 0, nullptr, fused ? &ko : nullptr);
      q.ev_p1 = S.get_event();
      q.ev_prior = S.get_event();
      if (!q.ev_p1 || !q.ev_prior) return VSM_EHIP;
      HIPCHK(hipEventRecord(q.ev_p1, h->stream));
    }
    return VSM_OK;
  }
  // ... and the chain of its pass-1 lists (outlier removal + prior boxes) on a stream of its own: a dozen and a half enqueue
  // calls that the caller makes AFTER it has given the main stream its next kernels - the boxes are wanted two chunks later
  // fused_keys: the job table of chunk k's pass-1 chain, filled and sent on the chain's own stream BEFORE the first pass is
  // launched (start_chunk): nothing in it comes from the matching - list, count and key pointers of the pair bank, slab
  // pointers, the capacity.  The three waits for the slab bank1[k & 1] come along: the copy of its last job table out of the
  // pinned twin (bank1_copied: the caller's thread waits here, a copy enqueued two chunks ago), the slab's last chain
  // (ev_prior of chunk k - 2: the chain's stream waits in front of the upload; recorded by now - start_chunk has been
  // through finish_chain1 of every chunk in front) and, should the slab have to grow, the same event on the host.
  int upload_chain1_jobs(int k) {
    Ck &q = ck[k];
    const int n = q.n, first_pair = q.first_pair;
    Dc2Bank &B = S.bank1[k & 1];
    const int want = std::max(q.max_nq[0], 64);
    hipEvent_t last_chain = k > 1 ? ck[k - 2].ev_prior : nullptr;
    if (last_chain && (C > B.npairs || want > B.cap || (ties1_host && !B.host_ties))) HIPCHK(hipEventSynchronize(last_chain));
    if (!B.reserve(C, want, ties1_host)) return VSM_EHIP;
    if (S.bank1_copied[k & 1]) HIPCHK(hipEventSynchronize(S.bank1_copied[k & 1]));
    for (int i = 0; i < n; i++)
      B.fill_job(i, c.h_pairs[first_pair + i].list1, c.h_pairs[first_pair + i].count, !ties1_host, nullptr, nullptr, c.h_pairs[first_pair + i].ranges,
                 nullptr, false, c.h_pairs[first_pair + i].keys[0], c.hm_lcount + 2 * (first_pair + i));
    hipStream_t c1 = S.cs(k);
    if (last_chain) HIPCHK(hipStreamWaitEvent(c1, last_chain, 0));
    HIPCHK(vsm_upload(c1, B.d_jobs, B.h_jobs, sizeof(VsmDc2Job) * n));
    S.bank1_copied[k & 1] = S.get_event();
    if (!S.bank1_copied[k & 1]) return VSM_EHIP;
    HIPCHK(hipEventRecord(S.bank1_copied[k & 1], c1));
    return VSM_OK;
  }
  int start_chain1(int k) {
    Ck &q = ck[k];
    if (!p.multi_stage) return VSM_OK;
    const int n = q.n, first_pair = q.first_pair;
    {
      // (two slabs: a chunk's pass-1 chain takes half a millisecond, the first passes of the call's last chunks follow each other
      // faster than that - and the last chunk's boxes are what the main stream ends up waiting for)
      Dc2Bank &B = S.bank1[k & 1];
      hipStream_t c1 = S.cs(k);
      hipEvent_t ev_keys = S.get_event(), ev_ties = S.get_event();
      if (!ev_keys || !ev_ties) return VSM_EHIP;
      if (fused) {
        // the job table is in place (upload_chain1_jobs) and the first pass's compaction has written the keys: behind its event
        // the chain starts on sort + kd order.  The keys the pool sorts cross by a strided DMA copy out of the pair bank, on the
        // null stream beside the mesh (host-resident inputs keep that stream's engine busy with frames: the chain's own stream)
        HIPCHK(hipStreamWaitEvent(c1, q.ev_p1, 0));
        if (ties1_host) {
          hipStream_t ks = host_in ? c1 : S.ns;
          if (ks != c1) HIPCHK(hipStreamWaitEvent(ks, q.ev_p1, 0));
          HIPCHK(hipMemcpy2DAsync(B.host_keys(0), B.keys_pitch, c.h_pairs[first_pair].keys[0], c.pair_stride,
                                  (size_t)std::min(std::max(q.max_nq[0], 1), B.cap) * 8, (size_t)n, hipMemcpyDeviceToHost, ks));
          HIPCHK(hipEventRecord(ev_keys, ks));
        } else {
          HIPCHK(hipEventRecord(ev_keys, c1));
        }
      } else {
          if (!B.reserve(C, std::max(q.max_nq[0], 64), ties1_host)) return VSM_EHIP;
        if (S.bank1_copied[k & 1]) HIPCHK(hipEventSynchronize(S.bank1_copied[k & 1]));  // (the slab's last use: its copy of the job table)
        for (int i = 0; i < n; i++)
          B.fill_job(i, c.h_pairs[first_pair + i].list1, c.h_pairs[first_pair + i].count, !ties1_host, nullptr, nullptr,
                     c.h_pairs[first_pair + i].ranges);
        if (k > 1 && ck[k - 2].ev_prior) HIPCHK(hipStreamWaitEvent(c1, ck[k - 2].ev_prior, 0));  // (the slab's last chain is through)
        HIPCHK(hipStreamWaitEvent(c1, q.ev_p1, 0));
        HIPCHK(vsm_upload(c1, B.d_jobs, B.h_jobs, sizeof(VsmDc2Job) * n));
        S.bank1_copied[k & 1] = S.get_event();
        if (!S.bank1_copied[k & 1]) return VSM_EHIP;
        HIPCHK(hipEventRecord(S.bank1_copied[k & 1], c1));
        // keys, then the vertex sort (one wave per pair, a third of a millisecond) on a stream of its own beside kd order
        // and triangulation; the support votes wait for both
        h->prof.begin(VSM_K_DC_KEYS, c1);
        vsm_dc2_launch_keys(c1, B.d_jobs, n, q.max_nq[0]);
        h->prof.end(c1);
        HIPCHK(hipEventRecord(ev_keys, c1));
      }
      if (ties1_host) {
        // The vertex sorts of these lists on the POOL, which has nothing to do before the call's first final keys: the key
        // kernel has written keys and counts into host-mapped memory; the mesh goes in now, the second part (tie patches,
        // votes, boxes) when the caller's thread gets to this chunk's second pass (finish_chain1) - by then the keys are
        // there, and the sorts (10-70 us per list) run while the device triangulates.  The device's own sort of such a list
        // is one wave for 0.43 ms (1.85 ms for the 3.9 k lists of 2048 x 1024 images: twice the mesh beside it) on a
        // compute unit whose LDS it takes.
        q.ev_k1 = ev_keys;
        q.chain1_open = true;
        dc2_enqueue_mesh(c1, B, n, q.max_nq[0], h->prof, false, nullptr, S.expect_long);
        HIPCHK(hipGetLastError());
        return VSM_OK;
      }
      // (host-resident inputs, chunk by chunk: the main stream has nothing to do between a chunk's first pass and its boxes, which
      // need these sorts - while the null stream carries the early export of the chunk in front, 34 MB behind the frames that
      // still arrive on the same engine: a sort enqueued there started up to 1.3 ms late)
      hipStream_t ts1 = inorder ? h->stream : (sw.seq_ties1_null ? S.ns : S.cs(k + 2));
      HIPCHK(hipStreamWaitEvent(ts1, ev_keys, 0));
      h->prof.begin(VSM_K_DC_TIES, ts1);
      vsm_dc2_launch_ties(ts1, B.d_jobs, n, B.d_ties, VSM_DC_TIE_OUT_INTS, q.max_nq[0]);
      h->prof.end(ts1);
      HIPCHK(hipEventRecord(ev_ties, ts1));
      dc2_enqueue_mesh(c1, B, n, q.max_nq[0], h->prof, false, nullptr, S.expect_long);
      HIPCHK(hipStreamWaitEvent(c1, ev_ties, 0));
      dc2_enqueue_votes(c1, B, n, q.max_nq[0], method, (float)p.outlier_flow_tolerance, (float)p.outlier_disp_tolerance, h->prof);
      h->prof.begin(VSM_K_DC_PRIOR, c1);
      vsm_dc2_launch_prior(c1, B.d_jobs, n, method, p.match_binsize, p.match_radius, w, hh, c.dims.ub, c.dims.vb);
      h->prof.end(c1);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(q.ev_prior, c1));
    }
    return VSM_OK;
  }
  int finish_chain1(int k) {  // (the pool's share of a pass-1 chain)
    Ck &q = ck[k];
    if (!q.chain1_open) return VSM_OK;
    q.chain1_open = false;
    Dc2Bank &B = S.bank1[k & 1];
    const int n = q.n;
    const double t0 = now_us();
    HIPCHK(hipEventSynchronize(q.ev_k1));
    h->pool->run(n, [&](int i) { B.sort_ties_of(i); });
    tg += now_us() - t0;
    hipStream_t c1 = S.cs(k);
    std::lock_guard<std::mutex> lk(S.enq_mu);
    dc2_enqueue_votes(c1, B, n, q.max_nq[0], method, (float)p.outlier_flow_tolerance, (float)p.outlier_disp_tolerance, h->prof);
    h->prof.begin(VSM_K_DC_PRIOR, c1);
    vsm_dc2_launch_prior(c1, B.d_jobs, n, method, p.match_binsize, p.match_radius, w, hh, c.dims.ub, c.dims.vb);
    h->prof.end(c1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(q.ev_prior, c1));
    return VSM_OK;
  }
  // the refinement of a chunk on the main stream, enqueued right behind the chunk's second pass and in front of the chain's
  // two dozen enqueue calls, so that the main stream never waits for the caller's thread
  int launch_refine(Seq2Chunk *ch, int k) {
    const Ck &q = ck[k];
    VsmJob dummy;
    memset(&dummy, 0, sizeof(dummy));
    if (p.refinement > 0)
      vsm_launch_refine(h->stream, h->prof, c.d_imgs, c.d_pairs + q.first_pair, c.d_jobs + q.first_pair, dummy, q.n, c.dims, c.dims, method,
                        p.refinement, q.max_nq[1]);
    // sub-pixel refinement: the fits' least-squares tail and the removal of the matches whose fit fails - the list gets shorter,
    // so this chunk's chain starts behind it (ev_ref), not behind the second pass
    if (p.refinement == 2) vsm_launch_parabolic_apply(h->stream, h->prof, c.d_pairs + q.first_pair, q.n);
    ch->ev_ref = S.get_event();
    if (!ch->ev_ref) return VSM_EHIP;
    HIPCHK(hipEventRecord(ch->ev_ref, h->stream));
    return VSM_OK;
  }
  // The refined lists leave for the host beside the triangulation, as they are (48-byte p_match records), straight out of the
  // pair buffers by strided DMA copies (28 MB per 80 pairs, 0.58 ms at the link's 49 GB/s); the chain's end only adds a bit per
  // match.  The device has ONE engine for copies to the host and it takes them in the order they were SUBMITTED, waiting for
  // each one's dependencies in turn (tools/trace_copies.sh): a copy that stands in front of a chunk's keys in that order holds
  // the keys back - and with them the pool's vertex sorts, 25 ms of work that everything after waits for - for as long as it
  // takes, and one that waits for a late event holds everything behind it.  So the exports are cut into pieces of 20 pairs
  // (0.15 ms), go onto the NULL stream - the process's fifth hardware queue, which exists anyway and has nothing else to do
  // during the call; all streams of this path are non-blocking - and are submitted in the order the engine should work in:
  // behind a chunk's keys as many pieces as fit in front of the next chunk's keys (two where the next second pass follows at
  // once: the end of every call; otherwise all that are pending), the rest when the call's last keys are in.
  int export_some(int upto, int budget) {  // budget: pieces (< 0: all)
    if (!S.res_early) return VSM_OK;
    std::lock_guard<std::mutex> lk(S.enq_mu);
    hipStream_t xs = S.ns;
    const int per = 20;
    while (exp_k <= upto && exp_k < (int)S.chunks.size()) {
      Seq2Chunk *ch = S.chunks[exp_k].get();
      const Ck &q = ck[exp_k];
      if (ch->max_list <= 0 || !ch->ev_ref || !ch->ev_jobs) {
        if (ch->max_list > 0) return VSM_OK;  // (its refinement / head is not in yet)
        exp_k++;
        continue;
      }
      while (ch->exp_row < q.n) {
        if (budget == 0) return VSM_OK;
        const int r0 = ch->exp_row, rows = std::min(per, q.n - r0);
        if (r0 == 0) {
          HIPCHK(hipStreamWaitEvent(xs, ch->ev_ref, 0));
          HIPCHK(hipStreamWaitEvent(xs, ch->ev_jobs, 0));
        }
        const vsm_p_match *src = c.h_pairs[q.first_pair + r0].list2;
        const size_t pitch = q.n > 1 ? (size_t)((const char *)c.h_pairs[q.first_pair + 1].list2 - (const char *)c.h_pairs[q.first_pair].list2) : slot;
        HIPCHK(hipMemcpy2DAsync(S.res + S.res_off[ch->f0 + r0], slot, src, pitch, std::min((size_t)ch->max_list * sizeof(vsm_p_match), slot), (size_t)rows,
                                hipMemcpyDeviceToHost, xs));
        ch->exp_row += rows;
        if (budget > 0) budget--;
      }
      ch->ev_exp = S.get_event();
      if (!ch->ev_exp) return VSM_EHIP;
      HIPCHK(hipEventRecord(ch->ev_exp, xs));
      exp_k++;
    }
    return VSM_OK;
  }
  // The device's share of the final vertex sorts.  A wave sorts one list in 3.2 ms and a launch takes that long whatever the
  // number of lists, so the lists of ALL chunks that wait for the device go into one launch - on the null stream (a launch
  // per chunk needs a stream per chunk: a sixth, seventh, eighth hardware queue, and with those every kernel's dispatch is
  // throttled, DESIGN_HISTORY.md 6c) - when the call's last head is in, or earlier where a chunk has to be through before the
  // caller can go on (its slab or pair bank comes round).  The job table is gathered from the chunks' slabs; every job
  // carries the address its verdict goes to.  A chunk's second part waits for the launch's event, so the caller's half of
  // its gate stays shut until the launch is enqueued.
  // Share by pool size: the host has from the first keys (2 ms) to the end of that launch (last keys at 3 ms + 3.2) for its
  // part - 4.2 ms x threads / 125 us per list.
  int launch_pending_ties(hipStream_t ts) {
    if (ties_pending.empty()) return VSM_OK;
    std::vector<Seq2Chunk *> open;
    int total = 0, max_list = 0;
    for (int k : ties_pending) total += S.chunks[k]->gpu_sorts;
    if (tie_jobs_at + total > S.tie_jobs_cap) {
      HIPCHK(hipStreamSynchronize(S.ns));  // (an earlier launch may still read the old table)
      HIPCHK(hipStreamSynchronize(h->stream));
      tie_jobs_at = 0;
      if (S.tie_jobs_h) (void)hipHostFree(S.tie_jobs_h);
      if (S.tie_jobs_d) (void)hipFree(S.tie_jobs_d);
      S.tie_jobs_h = S.tie_jobs_d = nullptr;
      S.tie_jobs_cap = 0;
      const int cap = std::max(512, total * 2);
      if (hipHostMalloc((void **)&S.tie_jobs_h, sizeof(VsmDc2Job) * cap, hipHostMallocDefault) != hipSuccess ||
          hipMalloc((void **)&S.tie_jobs_d, sizeof(VsmDc2Job) * cap) != hipSuccess) {
        (void)hipGetLastError();
        return VSM_EHIP;
      }
      S.tie_jobs_cap = cap;
    }
    {
    std::lock_guard<std::mutex> lk(S.enq_mu);
    VsmDc2Job *rows_h = S.tie_jobs_h + tie_jobs_at, *rows_d = S.tie_jobs_d + tie_jobs_at;
    tie_jobs_at += total;
    int at = 0;
    for (int k : ties_pending) {
      Seq2Chunk *ch = S.chunks[k].get();
      memcpy(rows_h + at, ch->B->h_jobs, sizeof(VsmDc2Job) * ch->gpu_sorts);
      at += ch->gpu_sorts;
      max_list = std::max(max_list, ch->max_list);
      HIPCHK(hipStreamWaitEvent(ts, ch->ev_jobs, 0));  // (its keys are written)
    }
    HIPCHK(vsm_upload(ts, rows_d, rows_h, sizeof(VsmDc2Job) * total));
    ev_ties_go = S.get_event();
    if (!ev_ties_go) return VSM_EHIP;
    HIPCHK(hipEventRecord(ev_ties_go, ts));
    h->prof.begin(VSM_K_DC_TIES, ts);
    vsm_dc2_launch_ties(ts, rows_d, total, nullptr, 0, max_list);
    h->prof.end(ts);
    HIPCHK(hipGetLastError());
    hipEvent_t ev = S.get_event();
    if (!ev) return VSM_EHIP;
    HIPCHK(hipEventRecord(ev, ts));
    for (int k : ties_pending) {
      Seq2Chunk *ch = S.chunks[k].get();
      ch->ev_ties = ev;
      if (ch->gate_deferred) open.push_back(ch);
    }
    ties_pending.clear();
    }
    for (Seq2Chunk *ch : open) {  // (outside the lock: opening a gate may enqueue the second part, which takes it itself)
      ch->gate_deferred = false;
      ch->caller_gate = true;
      seq2_open_gate(ch);
    }
    return VSM_OK;
  }
  // the caller's half of the gate of the chain's second part (the export's event has to exist before it opens)
  int after_refine(Seq2Chunk *ch, int k) {
    int rc = export_some(k, -1);
    if (rc != VSM_OK) return rc;
    if (ch->gpu_sorts > 0 && !ch->ev_ties) {  // (its second part waits for an event that does not exist yet)
      if (!serial) {
        ch->gate_deferred = true;
        return VSM_OK;
      }
      rc = launch_pending_ties(S.ns);
      if (rc != VSM_OK) return rc;
    }
    ch->caller_gate = true;
    seq2_open_gate(ch);
    if (serial && !seq2_wait_chunk(ch, 60e6)) return VSM_EHIP;
    return VSM_OK;
  }
  // a slab or a pair bank comes round: the chunk that used it last must be through - which it cannot be while its share of the
  // vertex sorts has not been launched, so that goes in first; the wait is the caller's (tg)
  int wait_for_chunk(int j) {
    const int rc = launch_pending_ties(S.ns);
    if (rc != VSM_OK) return rc;
    const double t0 = now_us();
    if (!seq2_wait_chunk(S.chunks[j].get(), 30e6)) return VSM_EHIP;
    tg += now_us() - t0;
    return VSM_OK;
  }
  // Main stream, two chunks ahead with the features and the first pass:
  //   feat 0 | pass 1 (0) | feat 1 | pass 1 (1) | then per k: feat k+2 | pass 1 (k+2) | pass 2 (k) | refinement (k)
  // Between a chunk's first pass and its second the stream has two other chunks' work to do - more than the pass-1 chain
  // takes - so it does not wait for the prior boxes (two-chunk calls: 0.17 ms, DESIGN_HISTORY.md 6c); and a final chain's triangulation only needs (u1c, v1c), which
  // the refinement leaves alone: it starts behind pass 2, beside the refinement.
  // (the caller's order of enqueue calls: whatever the main stream runs next first, the side streams' rows of launches while
  // it is busy with that)
  int catch_up_chain1(int upto) {
    for (; chain1_next <= upto && chain1_next < nchunks; chain1_next++) {
      const int rc = start_chain1(chain1_next);
      if (rc != VSM_OK) return rc;
      if (serial) HIPCHK(hipDeviceSynchronize());
    }
    return VSM_OK;
  }
  // features + first pass of chunk k + 2 (the run-ahead of the main stream)
  int run_ahead(int k) {
    if (k + 2 >= nchunks) return VSM_OK;
    // the pair bank of chunk k + 2 was last used by chunk k + 2 - kPairBanks: that chunk's chain must be through
    int rc = k + 2 >= kPairBanks ? wait_for_chunk(k + 2 - kPairBanks) : VSM_OK;
    if (rc != VSM_OK) return rc;
    HIPCHK(launch_features_of(k + 2));
    rc = catch_up_chain1(k + 1);
    if (rc != VSM_OK) return rc;
    if (serial) HIPCHK(hipDeviceSynchronize());
    rc = start_chunk(k + 2);
    if (rc != VSM_OK) return rc;
    if (serial) HIPCHK(hipDeviceSynchronize());
    return VSM_OK;
  }
  // A chunk's second pass + refinement (main stream) and its final chain (side streams) are enqueued by two steps of the
  // caller's thread: the chain's thirty-odd HIP calls take the caller a few hundred microseconds, and while it makes them
  // the main stream must not run dry - where the next chunk's main-stream work needs nothing the caller would have to wait
  // for (no run-ahead block left: the end of every call), that work is enqueued FIRST and the chains follow.
  int enqueue_main(int k) {
    int rc = catch_up_chain1(k);  // (this chunk's second pass waits for its boxes: that event has to exist)
    if (rc != VSM_OK) return rc;
    const Ck &q = ck[k];
    const int n = q.n, first_pair = q.first_pair;
    const VsmPair *d_pairs = c.d_pairs + first_pair;
    const VsmJob *d_jobs = c.d_jobs + first_pair;
    VsmMatchCfg cfg = make_cfg(p, method, h->sw.match_heads && c.has_heads);
    VsmJob dummy;
    memset(&dummy, 0, sizeof(dummy));
    if (k >= Seq2::kBanks) rc = wait_for_chunk(k - Seq2::kBanks);  // this chunk's final-stage slab was last used by chunk k - kBanks
    if (rc != VSM_OK) return rc;
    Dc2Bank &B = S.bank2[k % Seq2::kBanks];
    if (!B.reserve(n, std::max(64, q.max_nq[1]), true)) return VSM_EHIP;
    S.chunks.emplace_back(new Seq2Chunk());
    Seq2Chunk *ch = S.chunks.back().get();
    ch->h = h;
    ch->k = k;
    ch->n = n;
    ch->f0 = q.f0;
    ch->method = method;  // (everything the pool's tasks read is in place before anything is enqueued)
    ch->max_list = q.max_nq[1];
    // (the last chunk of a call whose lists are exported early, on ranks with CPUs to spare: its gaps are closed out of the L3 caches)
    ch->warm = sw.seq_warm_gaps && S.res_early && k + 1 == nchunks && !host_in && !serial && h->pool->size() >= 10 && n > 0;
    if (ch->warm) {
      ch->warm_domain.reset(new std::atomic<signed char>[n]);
      ch->warm_claim.reset(new std::atomic<unsigned char>[n]);
      for (int i = 0; i < n; i++) {
        ch->warm_domain[i].store(-1, std::memory_order_relaxed);
        ch->warm_claim[i].store(0, std::memory_order_relaxed);
      }
    }
    ch->B = &B;
    ch->stream = S.cs(k);
    ch->ftol = (float)p.outlier_flow_tolerance;
    ch->dtol = (float)p.outlier_disp_tolerance;
    ch->sorts_left.store(1, std::memory_order_relaxed);
    if (p.multi_stage) {
      rc = finish_chain1(k);  // (the pool's share of the pass-1 chain, where it has one: the event below is recorded there)
      if (rc != VSM_OK) return rc;
      HIPCHK(hipStreamWaitEvent(h->stream, q.ev_prior, 0));
    }
    if (fused) {
      // the final chain's job table in front of the second pass's launch, on the chain's stream: its slab and the pinned twin
      // of the table were last used by chunk k - kBanks, which is through (wait_for_chunk above) - no event to wait for
      fill_chain_jobs(k);
      std::lock_guard<std::mutex> lk(S.enq_mu);
      HIPCHK(vsm_upload(ch->stream, B.d_jobs, B.h_jobs, sizeof(VsmDc2Job) * n));
    }
    cfg.sparse = 0;
    cfg.use_prior = p.multi_stage ? 1 : 0;
    const VsmKeyOut ko = {nullptr, 0, 0};  // (the final keys leave by DMA, enqueue_chain_head)
    vsm_launch_match(h->stream, h->prof, c.d_imgs, d_pairs, d_jobs, dummy, n, c.dims, cfg, q.max_nq[1], 0, nullptr, fused ? &ko : nullptr);
    ch->ev_c2 = S.get_event();
    if (!ch->ev_c2) return VSM_EHIP;
    HIPCHK(hipEventRecord(ch->ev_c2, h->stream));
    dbg_main.push_back(now_us());
    // The refinement is not what the chain waits for (its keys only need (u1c, v1c), which the refinement leaves alone): where
    // the next chunk's second pass follows at once on the main stream, this chunk's refinement goes BEHIND that pass's
    // matching - the call's last keys, and the last mesh with them, start a refinement earlier (option seq_defer_refine)
    if (refine_pending >= 0) {
      rc = launch_refine(S.chunks[refine_pending].get(), refine_pending);
      if (rc != VSM_OK) return rc;
      refine_pending = -1;
    }
    const bool next_follows = !serial && !host_in && !p2_first && k + 1 < nchunks && k + 3 >= nchunks && k + 1 < Seq2::kBanks + chain_next;
    if (sw.seq_defer_refine && next_follows && p.refinement == 1) {
      refine_pending = k;
    } else {
      rc = launch_refine(ch, k);
      if (rc != VSM_OK) return rc;
    }
    if (serial) HIPCHK(hipStreamSynchronize(h->stream));
    return VSM_OK;
  }
  // The chain comes in two steps as well.  Its HEAD - jobs, keys, the keys' DMA copy and the pool task that waits for it - goes in
  // right behind the chunk's main-stream work: the vertex sorts are 25 ms of pool work per call and want their keys early.
  // the final chain's job table on the host: who sorts which list, where everything lies (fused_keys: filled in front of the
  // second pass, enqueue_main; else with the head)
  void fill_chain_jobs(int k) {
    const Ck &q = ck[k];
    const int n = q.n, first_pair = q.first_pair;
    Seq2Chunk *ch = S.chunks[k].get();
    Dc2Bank &B = *ch->B;
    // Who sorts: the pool does a 7.4 k list in 125 us per thread, the device needs 3.2 ms for one (one wave, all dependent
    // scalar work) but does any number of lists side by side.  With six host threads or more the pool keeps up; below that it
    // is the longest pole (200 lists / 2 threads = 12.5 ms), so the device takes a share of every chunk (seq_gpu_sorts =
    // percent of the pairs; default by pool size, gpu_sorts_default) - in ONE launch per call, see launch_pending_ties.
    {
      int pct = sw.seq_gpu_sorts >= 0 ? sw.seq_gpu_sorts : gpu_sorts_default;
      if (split_sorts) {
        // (two chunks, a launch each - below: the pool has from the first keys to the end of the first launch, 3.2 ms, for
        // the first chunk's lists, and the 0.7 ms until the second launch ends for the second chunk's)
        const int sz = h->pool->size();
        pct = k == 0 ? (sz <= 2 ? 45 : (sz == 3 ? 18 : 0)) : (sz <= 2 ? 88 : (sz == 3 ? 82 : 66));
      }
      if (q.max_nq[1] > VSM_DC_TIE_POINTS) pct = 0;  // (a list the wave cannot take would send the whole run to the other form)
      ch->gpu_sorts = std::min(n, std::max(0, n * pct / 100));
    }
    for (int i = 0; i < n; i++) {
      const int32_t f = q.f0 + i;
      B.fill_job(i, c.h_pairs[first_pair + i].list2, c.h_pairs[first_pair + i].count + 1, i < ch->gpu_sorts,
                 (vsm_p_match *)(S.res_stage + S.res_off[f]), S.res_cnt_dev + f, nullptr, S.res_early ? S.keep_dev + S.keep_words * (size_t)f : nullptr, keys_dma != 0,
                 fused ? c.h_pairs[first_pair + i].keys[1] : nullptr, c.hm_lcount + 2 * (first_pair + i) + 1);
    }
  }
  int enqueue_chain_head(int k) {
    const Ck &q = ck[k];
    const int n = q.n, first_pair = q.first_pair;
    Seq2Chunk *ch = S.chunks[k].get();
    Dc2Bank &B = *ch->B;
    hipEvent_t ev_c2 = ch->ev_c2;
    if (!fused) fill_chain_jobs(k);
    hipStream_t s2 = ch->stream;
    hipEvent_t ev_jobs = nullptr;
    {
      // (the pool enqueues second parts on these streams too: what the caller puts on s2 here stays in one piece)
      std::lock_guard<std::mutex> lk(S.enq_mu);
      // jobs, keys (the chain itself only needs (u1c, v1c), which the refinement leaves alone)
      // (fused_keys: both are there when the second pass's compaction is through - the head is this wait and the keys' copies)
      HIPCHK(hipStreamWaitEvent(s2, p.refinement == 2 ? ch->ev_ref : ev_c2, 0));
      if (!fused) {
        HIPCHK(vsm_upload(s2, B.d_jobs, B.h_jobs, sizeof(VsmDc2Job) * n));
        h->prof.begin(VSM_K_DC_KEYS, s2);
        vsm_dc2_launch_keys(s2, B.d_jobs, n, q.max_nq[1]);
        h->prof.end(s2);
      }
      ev_jobs = S.get_event();
      if (!ev_jobs) return VSM_EHIP;
      HIPCHK(hipEventRecord(ev_jobs, s2));
      if (ch->gpu_sorts > 0) ties_pending.push_back(k);  // (its share of the vertex sorts goes with the next launch: launch_pending_ties)
      ch->state.store(1, std::memory_order_release);  // from here on the chunk completes by itself
      // the keys of the lists the pool sorts reach the host by a strided copy of the DMA engine on a stream of its own, not
      // by stores of the key kernel into host memory: a kernel that waits for PCIe holds the memory pipelines of its
      // compute units, and whatever else runs there (the refinement, the next chunk's matching) waits with it
      // (on the chain's own stream: the path's streams are all taken - five hardware queues, see Seq2 - and 4 MB at the link's
      // rate are 80 us in front of the mesh)
      // (seq_keys_dma 2: the copy on the fifth stream, behind an event of this one - the mesh does not wait for 6-8 MB to
      // cross: 130 us in front of the call's last mesh)
      hipStream_t ks = s2;
      if (n > ch->gpu_sorts && keys_dma) {
        if (keys_dma == 2 && !host_in) {
          hipEvent_t ev_k = S.get_event();
          if (!ev_k) {
            ch->state.store(0, std::memory_order_release);
            return VSM_EHIP;
          }
          HIPCHK(hipEventRecord(ev_k, s2));
          ks = S.ns;
          HIPCHK(hipStreamWaitEvent(ks, ev_k, 0));
        }
      }
      // The copy in pieces of a quarter of the lists, an event behind each: the pool starts on the first lists when they
      // are there (40 us), not when all 6-8 MB are (150-210 us behind the key kernel).
      // (who tells the pool that keys have arrived: Seq2Poller)
      {
        const int lists = n - ch->gpu_sorts;
        // (ranks with fewer than ten pool threads: one piece - their pool is busy anyway, and four events instead of one cost them
        // 2 %: 4.63 against 4.77 ms with eight threads)
        const int want = sw.seq_keys_pieces > 0 ? sw.seq_keys_pieces : (h->pool->size() >= 10 ? 4 : 1);
        const int pieces = (keys_dma && lists >= 32) ? std::max(1, std::min(want, 16)) : 1;
        ch->sort_tasks_left.store(std::max(lists, 1), std::memory_order_release);
        for (int pc = 0; pc < pieces; pc++) {
          const int r0 = ch->gpu_sorts + (int)((int64_t)lists * pc / pieces), r1 = ch->gpu_sorts + (int)((int64_t)lists * (pc + 1) / pieces);
          if (r1 > r0 && keys_dma)
            HIPCHK(hipMemcpy2DAsync(B.host_keys(r0), B.keys_pitch, fused ? c.h_pairs[first_pair + r0].keys[1] : B.pp[r0].keys_in,
                                    fused ? c.pair_stride : B.pair_stride,
                                    (size_t)std::min(std::max(q.max_nq[1], 1), B.cap) * 8, (size_t)(r1 - r0), hipMemcpyDeviceToHost, ks));
          hipEvent_t ev = S.get_event();
          if (!ev) {
            ch->state.store(0, std::memory_order_release);
            return VSM_EHIP;
          }
          HIPCHK(hipEventRecord(ev, ks));
          ch->ev_keys = ev;  // (the last piece's)
          S.poller.add(ev, [ch, r0, r1](bool done) {
            if (!done) ch->hip_error.store(1);  // (a failed stream: the sorts see stale keys, the chain's own calls report the error)
            seq2_keys_ready(ch, r0, r1);
          });
        }
      }
      // sort + kd order behind the keys: one workgroup per list with 128 KB of LDS, which finds no room on a compute unit
      // while an earlier chunk's block kernel (five workgroups of 21 KB each, everywhere) is resident - so it goes in with
      // the head, and the block kernel of the chunk in front of the call's LAST chunk waits for it (enqueue_chain_mesh): the
      // last chunk's chain is what the call ends with
      if (sw.seq_last_first && nchunks >= 3) {  // (with two chunks the first one's chain is as late as the last one's: 4.18 against 4.30 ms without)
        dc2_enqueue_prepare(s2, B, n, ch->max_list, h->prof, S.expect_long);
        ch->ev_prep = S.get_event();
        if (!ch->ev_prep) return VSM_EHIP;
        HIPCHK(hipEventRecord(ch->ev_prep, s2));
      }
    }
    ch->ev_jobs = ev_jobs;
    if (k + 1 == nchunks || split_sorts) {
      // the call's last head is in: the device's share of all pending chunks' vertex sorts.  (Two-chunk calls: a launch per
      // chunk - the first chunk's on the null stream behind its keys, the second's on the MAIN stream, which has nothing left
      // to do behind the last refinement - so that the first chunk's survivors cross PCIe while the second chunk still
      // sorts: without the early export every chunk's results are 0.7 ms of DMA behind its sorts, and behind one common
      // launch they queue up.)
      const int rc = launch_pending_ties(split_sorts && k + 1 == nchunks ? h->stream : S.ns);
      if (rc != VSM_OK) return rc;
    }
    if (!serial) {  // (the engine's order: these keys, then export pieces - see export_some)
      const bool tail = k + 1 < nchunks && k + 3 >= nchunks;   // the next chunk's second pass follows at once
      return export_some(k, k + 1 == nchunks ? -1 : (tail ? sw.seq_export_budget : -1));
    }
    return VSM_OK;
  }
  // ... and its mesh (sort + kd order, block sub-trees, merge levels, per-match flows), the early export and the caller's half of
  // the gate: a dozen and a half more calls, which may wait until the main stream has been given its next kernels
  int enqueue_chain_mesh(int k) {
    const Ck &q = ck[k];
    const int n = q.n;
    Seq2Chunk *ch = S.chunks[k].get();
    Dc2Bank &B = *ch->B;
    hipStream_t s2 = ch->stream;
    {
      std::lock_guard<std::mutex> lk(S.enq_mu);
      hipEvent_t last_prep = nullptr;
      if (sw.seq_last_first && k + 2 == nchunks && (int)S.chunks.size() == nchunks) last_prep = S.chunks[k + 1]->ev_prep;
      if (!last_prep && ev_ties_go && ch->gpu_sorts > 0 && ch->ev_ties) last_prep = ev_ties_go;  // (the sorts are placed first)
      // (seq_block_after_p2: the block kernel - 1760 workgroups that take every compute unit's LDS and most of its registers -
      // waits for the NEXT chunk's second matching pass, which it otherwise runs beside)
      if (!last_prep && sw.seq_block_after_p2 && k + 1 < nchunks && (int)S.chunks.size() > k + 1 && S.chunks[k + 1]->ev_c2) last_prep = S.chunks[k + 1]->ev_c2;
      dc2_enqueue_mesh(s2, B, n, ch->max_list, h->prof, ch->ev_prep != nullptr, last_prep, S.expect_long);
      // what the votes compare (flow, disparity per match) behind the triangulation: it needs the refined list, which is
      // there long before the merges are through, and is one launch less between the vertex sorts and the survivors
      HIPCHK(hipStreamWaitEvent(s2, ch->ev_ref, 0));
      vsm_dc2_launch_flows(s2, B.d_jobs, n, ch->max_list, method);
      HIPCHK(hipGetLastError());
      ch->ev_mesh = S.get_event();
      if (!ch->ev_mesh) return VSM_EHIP;
      HIPCHK(hipEventRecord(ch->ev_mesh, s2));
    }
    if (serial) HIPCHK(hipStreamSynchronize(s2));
    return after_refine(ch, k);
  }
  int flush_chains(int upto) {
    for (; chain_next <= upto; chain_next++) {
      const int rc = enqueue_chain_mesh(chain_next);
      if (rc != VSM_OK) return rc;
    }
    return VSM_OK;
  }
  // the bank's error word read and cleared (a list this form declines), and whether it met a list beyond the LDS forms
  int take_bank_errors(Dc2Bank &b) {
    if (!b.h_error) return 0;
    const int code = b.h_error[0];
    S.expect_long |= b.h_error[1] != 0;  // (a list beyond the LDS forms went through the narrow one: the long lists' kernel comes along from now on)
    b.h_error[0] = b.h_error[1] = 0;
    return code;
  }
  // the end of the call: the chunks' results, the banks' error codes, the VSM_DEBUG_TIMING report, seq_timings
  int finish() {
    const double t0 = now_us();
    for (auto &ch : S.chunks)
      if (!seq2_wait_chunk(ch.get(), 60e6, h->pool)) return VSM_EHIP;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->prof.on) {  // (every stream that carries spans has drained: the chunks are done)
      for (int i = 0; i < S.dc_streams; i++) HIPCHK(hipStreamSynchronize(S.dc2[i]));
      HIPCHK(hipStreamSynchronize(S.ns));
      h->prof.resolve();
    }
    tg += now_us() - t0;
    int declined_code = 0;
    for (Dc2Bank &b : S.bank1) declined_code |= take_bank_errors(b);
    for (Dc2Bank &b : S.bank2) declined_code |= take_bank_errors(b);
    int hip_failed = 0;
    for (auto &ch : S.chunks) hip_failed |= ch->hip_error.load();
    if (hip_failed) {  // a HIP call of a second part failed: that is an error, not a list this form declines
      fprintf(stderr, "visomatch: a final chain of the GPU-resident look-ahead path failed: %s\n", hipGetErrorString(hipGetLastError()));
      h->seq_hip_error.store(1);
      return VSM_EHIP;
    }
    if (declined_code) {
      fprintf(stderr, "visomatch: the GPU-resident look-ahead path declined a list (code %d), running the host-shared form\n", declined_code);
      return VSM_SEQ2_DECLINED;
    }
    if (vsm_debug_timing()) {
      if (!S.up_pieces.empty()) {
        fprintf(stderr, "  upload pieces enqueued at (us):");
        for (auto &pc : S.up_pieces) fprintf(stderr, " %d:%.0f", pc->f0, pc->t_recorded - tstart);
        fprintf(stderr, "\n  ... arrived at (us):");
        for (auto &pc : S.up_pieces) fprintf(stderr, " %d:%.0f", pc->f0, pc->t_arrived > 0 ? pc->t_arrived - tstart : -1.0);
        fprintf(stderr, "\n  chunks' feature counts known / second pass enqueued at (us):");
        for (size_t k = 0; k < dbg_counts.size(); k++) fprintf(stderr, " %zu:%.0f/%.0f", k, dbg_counts[k] - tstart, k < dbg_main.size() ? dbg_main[k] - tstart : -1.0);
        fprintf(stderr, "\n");
      }
      for (auto &ch : S.chunks)
        fprintf(stderr, "  chunk %d (%d pairs): keys on the host at %.0f us, sorted at %.0f (tasks %.0f us), chain done at %.0f, results in place at %.0f\n", ch->k, ch->n,
                ch->t_keys - tstart, ch->t_sorted - tstart, ch->sort_ns.load() * 1e-3, ch->t_done - tstart, (ch->t_ready > 0 ? ch->t_ready : ch->t_done) - tstart);
      fprintf(stderr, "  call returns at %.0f us\n", now_us() - tstart);
    }
    h->seq_v2_frames = n_frames;
    h->seq_timings[0] = tg;
    h->seq_timings[1] = 0;
    for (auto &ch : S.chunks) h->seq_timings[1] += ch->sort_ns.load() * 1e-3;
    h->seq_timings[2] = now_us() - tstart;
    h->seq_timings[3] = (double)C;
    return VSM_OK;
  }
};

// The order of it all, on the caller's thread.
static int sequence_run_v2(vsm_handle *h, const uint8_t *left, const uint8_t *right, int64_t frame_stride, int on_device, int32_t n_frames,
                           int32_t w, int32_t hh, int32_t bpl, int32_t method, const double *Tr, const uint8_t *Tr_valid) {
  if (!h->seq2) h->seq2 = new Seq2();
  Seq2Call q(h, left, right, frame_stride, on_device, n_frames, w, hh, bpl, method, Tr, Tr_valid);
  int rc = q.setup_streams();
  if (rc == VSM_OK) rc = q.setup_results();
  if (rc != VSM_OK) return rc;  // (nothing asynchronous has been started yet: no wait)
  q.drain.h = h;                // from here on every way out waits for what the call has started
  q.tstart = now_us();
  rc = q.setup_uploads();
  if (rc != VSM_OK) return rc;
  // Host-resident inputs arrive at the link's rate, which is what bounds the call: chunk by chunk in the order of arrival,
  // no run-ahead - the caller's thread blocks on a chunk's feature counts (i.e. on its frames' arrival) only when everything
  // of the chunk in front, final chain included, is enqueued.  (In the run-ahead order it waited for chunk k + 2's frames
  // before it enqueued chunk k + 1's second pass: the last two chunks' second passes and chains all started behind the last
  // frame's arrival - 7.4 ms per 200 frames against 3.3 ms of transfer.)
  if (q.inorder) {
    for (int k = 0; k < q.nchunks; k++) {
      if (k >= Seq2Call::kPairBanks) {  // the pair bank of chunk k was last used by chunk k - kPairBanks: that chunk's chain must be through
        rc = q.wait_for_chunk(k - Seq2Call::kPairBanks);
        if (rc != VSM_OK) return rc;
      }
      HIPCHK(q.launch_features_of(k));
      rc = q.start_chunk(k);
      if (rc == VSM_OK) rc = q.enqueue_main(k);  // (with the chunk's pass-1 chain in front)
      if (rc == VSM_OK) rc = q.enqueue_chain_head(k);
      if (rc == VSM_OK) rc = q.flush_chains(k);
      if (rc != VSM_OK) return rc;
    }
    return q.finish();
  }
  // features + first pass of chunks 0 and 1: the run-ahead of "chunks -2 and -1" (no bank to wait for; chunk 0's pass-1 chain
  // goes in behind chunk 1's feature kernels)
  for (int k = -2; k < 0; k++) {
    rc = q.run_ahead(k);
    if (rc != VSM_OK) return rc;
  }
  // Host-resident inputs arrive at the link's rate (0.94 MB per frame pair, ~20 us each at 50 GB/s: the 200 frames of the
  // benchmark sequence need 3.7 ms, three quarters of what the whole call takes from HBM), so the GPU works on what has
  // arrived: a chunk's second pass and its final chain go in FRONT of the features of chunk k + 2, whose frames are the last
  // to come.  (From HBM that order loses: the features then run beside a final chain, DESIGN_HISTORY.md section 6c.)
  // ... and so is the order for ranks whose POOL bounds the call (four to nine host threads: 25 ms of vertex sorts are 3-6 ms
  // of wall clock there, and they start with the first keys - 0.6 ms earlier this way: 8 threads 5.28 -> 4.89 ms, 6 threads
  // 6.1 -> 5.75, 4 threads 7.14 -> 7.03; with ten threads and more the two-chunk plan in the order below wins, with three and
  // fewer the device's share of the sorts wants the other order: 8.5 against 9.8 ms)
  // (Measured beside it, round 5: one chunk of run-ahead - 7.4-8.2 ms against 7.5-7.7 -, and the caller's thread as a scheduler
  // that enqueues a chunk's features / first pass / second pass when event queries say that the frames / counts / boxes are
  // there - 7.3-7.4 ms with calls of 13-18 ms in between.  What is left after the last frame's arrival at 3.9 ms is the chunk's
  // own row of latencies - features, first pass, pass-1 chain, second pass, keys, vertex sorts, final chain - beside the
  // chains of the chunks in front: 3.4 ms, 1.7 on an idle GPU.)
  if ((q.host_in || q.p2_first) && !q.serial) {
    for (int k = 0; k < q.nchunks; k++) {
      rc = q.catch_up_chain1(k + 1);  // (in front of this chunk's final chain: its vertex sort shares that chain's stream)
      if (rc == VSM_OK) rc = q.enqueue_main(k);
      if (rc == VSM_OK) rc = q.enqueue_chain_head(k);
      if (rc == VSM_OK) rc = q.flush_chains(k);
      if (rc == VSM_OK) rc = q.run_ahead(k);
      if (rc == VSM_OK) rc = q.catch_up_chain1(k + 2);
      if (rc != VSM_OK) return rc;
    }
    return q.finish();
  }
  for (int k = 0; k < q.nchunks; k++) {
    rc = q.run_ahead(k);
    if (rc == VSM_OK) rc = q.enqueue_main(k);
    if (rc == VSM_OK) rc = q.catch_up_chain1(k + 2);  // the pass-1 chain of the chunk whose first pass went in above (in front of the export on its stream)
    if (rc == VSM_OK) rc = q.enqueue_chain_head(k);
    // the next chunk's second pass can follow at once when no run-ahead block (and so no wait for feature counts) and no wait
    // for a slab lies between: the chains then go in behind it
    const bool next_main_free = !q.serial && k + 1 < q.nchunks && k + 3 >= q.nchunks && k + 1 < Seq2::kBanks + q.chain_next;
    if (rc == VSM_OK && !next_main_free) rc = q.flush_chains(k);
    if (rc != VSM_OK) return rc;
  }
  return q.finish();
}
