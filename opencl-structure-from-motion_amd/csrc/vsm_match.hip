// gfx950 (MI355X, CDNA4) kernels of the pair side of the matcher hot path: everything that sees a VsmPair / VsmJob - the match
// chain (find_match / k_match), the compaction and export of its lists, the refinement, the parabolic tail and the table upload.
// The image side (ingest .. records and bin order) is vsm_image.hip; what both use is vsm_dev.h.  Wave = 64 lanes, no MFMA.
//
// Semantics are those of the reference; file:line citations below refer to the reference repository.

#include <stdlib.h>

#include <algorithm>

#include "vsm_internal.h"
#include "vsm_dev.h"

// Tuned constants of k_match and its launch:
#define VSM_MATCH_BLOCK 256  // threads per block of k_match
#define VSM_MATCH_WAVES 5  // waves per SIMD the register allocator must leave room for (96 registers, no scratch; six would spill)
#define VSM_MATCH_GBIG 2  // lanes per query of the big batches (vsm_launch_match; one lane per query: no gain, DESIGN_HISTORY.md 6d)
#define VSM_STEREO_BY_BIN 1  // the stereo-type stages (window = a few rows x the disparity range: 2-3 bins, a few candidates each) scan by bin also under prior boxes: -3.5 %

// Experiments (tools/build_variant.sh NAME -DVSM_MATCH_TIMING[=3], tools/match_timing.py, tools/match_wave_life.py): the life of
// every wave of the dense pass - cycles of the whole chain, of its four stages and (mode 1) of find_match's two phases, bins +
// scan against judging; mode 3 takes life and start from the device-wide clock instead (100 MHz, one counter for the whole
// device: s_memtime runs per XCD).  The kernels below carry MT_* marks, which are empty in the normal build.
#ifdef VSM_MATCH_TIMING
#if VSM_MATCH_TIMING != 1 && VSM_MATCH_TIMING != 3
#error "VSM_MATCH_TIMING: 1 (cycles per stage and phase) or 3 (wave life on the device-wide clock)"
#endif
__device__ unsigned int vsm_mt_n;
__device__ unsigned int vsm_mt[1 << 18][8];  // life, stage 1..4, bins + scan, judging, start (low bits)
extern "C" int vsm_debug_match_timing(unsigned int *out, unsigned int cap, int reset) {
  unsigned int n = 0;
  if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(vsm_mt_n), 4) != hipSuccess) return -1;
  if (n > (1u << 18)) n = 1u << 18;
  if (n > cap) n = cap;
  if (n && hipMemcpyFromSymbol(out, HIP_SYMBOL(vsm_mt), (size_t)n * 32) != hipSuccess) return -1;
  if (reset) {
    const unsigned int z = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(vsm_mt_n), &z, 4) != hipSuccess) return -1;
  }
  return (int)n;
}
// find_match: MT_PHASE(0) before the scan, (1) behind it, (2) behind the judging; MT_PHASE_ADD(ph) adds the two lengths to ph[0..1]
#if VSM_MATCH_TIMING == 1
#define MT_PHASE(k) const long long mt_ph##k = clock64()
#define MT_PHASE_ADD(ph)           \
  do {                             \
    if (ph) {                      \
      (ph)[0] += mt_ph1 - mt_ph0;  \
      (ph)[1] += mt_ph2 - mt_ph1;  \
    }                              \
  } while (0)
#define MT_WALL_DECL
#define MT_WALL_REC(k, ph)                  \
  do {                                      \
    vsm_mt[k][6] = (unsigned int)(ph)[1];   \
    vsm_mt[k][7] = (unsigned int)mt_s[0];   \
  } while (0)
#else
#define MT_PHASE(k)
#define MT_PHASE_ADD(ph)
#define MT_WALL_DECL const long long mt_w0 = wall_clock64()
#define MT_WALL_REC(k, ph)                                     \
  do {                                                         \
    vsm_mt[k][6] = (unsigned int)(wall_clock64() - mt_w0);     \
    vsm_mt[k][7] = (unsigned int)mt_w0;                        \
  } while (0)
#endif
// k_match: MT_BEGIN(ph) at the chain's start (ph then points at the wave's two phase sums), MT_STAGE(k) behind stage k of
// the quad chain, MT_END(ph) behind the chain: the first lane of every wave of the dense pass writes the wave's record.
// (MT_STAGE stamps in every lane and in the sparse pass too, where nobody reads the stamp: the record is the same as with a
// stamp in the recording lane alone, only the instrumented build does a little more work.)
#define MT_BEGIN(ph)                  \
  const long long mt_t0 = clock64();  \
  MT_WALL_DECL;                       \
  long long mt_s[5] = {mt_t0, mt_t0, mt_t0, mt_t0, mt_t0}, mt_ph_[2] = {0, 0}; \
  ph = mt_ph_
#define MT_STAGE(k) mt_s[k] = clock64()
#define MT_END(ph)                                                     \
  do {                                                                 \
    if (!cfg.sparse && (threadIdx.x & 63) == 0) {                      \
      const long long mt_t1 = clock64();                               \
      const unsigned int mt_k = atomicAdd(&vsm_mt_n, 1u);              \
      if (mt_k < (1u << 18)) {                                         \
        vsm_mt[mt_k][0] = (unsigned int)(mt_t1 - mt_s[0]);             \
        for (int mt_i = 1; mt_i <= 4; mt_i++) vsm_mt[mt_k][mt_i] = (unsigned int)(mt_s[mt_i] - mt_s[mt_i - 1]); \
        vsm_mt[mt_k][5] = (unsigned int)(ph)[0];                       \
        MT_WALL_REC(mt_k, ph);                                         \
      }                                                                \
    }                                                                  \
  } while (0)
#else
#define MT_PHASE(k)
#define MT_PHASE_ADD(ph)
#define MT_BEGIN(ph)
#define MT_STAGE(k)
#define MT_END(ph)
#endif

// ---------------------------------------------------------------------------------------
// M2/M3 findMatch + matching, viso/matcher.cpp:892-963 and :965-1153.
// A group of G lanes owns one query and walks the whole dependent chain (2 stages for flow /
// stereo, 4 for quad).  In each stage the lanes stride over the candidates of the fine bins the
// window touches (packed 4-byte coordinates, 16-byte loads; 32-byte descriptor reads only for
// in-window candidates), cost = v_sad_u8 x 8 (+ 4*sqrt(du^2+dv^2) in double when a prediction is
// active), and the winner is the lexicographic minimum of (cost, place in the reference's visiting
// order) over the group -- exactly the reference's "first minimum in (u_bin, v_bin, index) order"
// (:937-958).  Measured on MI355X the kernel is bound by instruction issue and dependent L2 round
// trips, not by bytes (SQ counters in profiles/): fewer visited candidates, a 3-instruction window
// test and judging candidates per lane rather than per visited slot are what made it faster.
// ---------------------------------------------------------------------------------------
#define VSM_NONE 0xffffffffu

__device__ __forceinline__ uint32_t sad32(const uint4 &a0, const uint4 &a1, const uint4 &b0, const uint4 &b1) {
  uint32_t s = __builtin_amdgcn_sad_u8(a0.x, b0.x, 0u);
  s = __builtin_amdgcn_sad_u8(a0.y, b0.y, s);
  s = __builtin_amdgcn_sad_u8(a0.z, b0.z, s);
  s = __builtin_amdgcn_sad_u8(a0.w, b0.w, s);
  s = __builtin_amdgcn_sad_u8(a1.x, b1.x, s);
  s = __builtin_amdgcn_sad_u8(a1.y, b1.y, s);
  s = __builtin_amdgcn_sad_u8(a1.z, b1.z, s);
  s = __builtin_amdgcn_sad_u8(a1.w, b1.w, s);
  return s;
}

// the feature a chain stage starts from: position, class and 32-byte descriptor, in registers
struct VsmQuery {
  uint32_t uv;  // u | v << 16
  int c;
  uint4 da, db;
  __device__ __forceinline__ int u() const { return (int)(uv & 0xffffu); }
  __device__ __forceinline__ int v() const { return (int)(uv >> 16); }
};

__device__ __forceinline__ VsmQuery load_query(const VsmSet &A, int i) {
  const int32_t *rec = A.feat + (size_t)i * 12;
  const int4 hd = ldg_i4(rec);
  VsmQuery q;
  q.uv = (uint32_t)hd.x | ((uint32_t)hd.y << 16);
  q.c = hd.w;
  q.da = ldg_u4(rec + 4);
  q.db = ldg_u4(rec + 8);
  return q;
}

// One findMatch (viso/matcher.cpp:892-963) for the query held in `q` against feature set B.
// Returns the winner's position in B's bin-sorted arrays (VSM_NONE if the window is empty) and
// REPLACES q by the winner (the lane that found it broadcasts coordinates + descriptor with
// width-G shuffles), so the next stage of the chain starts without going back to memory; the
// winner's feature index is only looked up once, at the end of the chain.  An empty window
// yields feature 0 of B like the reference (min_ind = 0, :898), class included.
typedef unsigned short vsm_us2 __attribute__((ext_vector_type(2)));

template <int G, bool RELOAD = true, bool MAYPRED = true, bool BYBIN = false, bool HEADS = false>
__device__ __forceinline__ uint32_t find_match(VsmQuery &q, const VsmSet &B, const VsmDims &d, const VsmMatchCfg &cfg,
                                               bool prior, float r_umin, float r_umax, float r_vmin, float r_vmax,
                                               bool flow, double u_, double v_, int lane, long long *ph = nullptr) {
  float u_min, u_max, v_min, v_max;
  const int qu = q.u(), qv = q.v();
  if (prior) {
    u_min = (float)qu + r_umin;
    u_max = (float)qu + r_umax;
    v_min = (float)qv + r_vmin;
    v_max = (float)qv + r_vmax;
  } else {
    u_min = (float)(qu - cfg.radius);
    u_max = (float)(qu + cfg.radius);
    v_min = (float)(qv - cfg.radius);
    v_max = (float)(qv + cfg.radius);
  }
  if (!flow) {
    v_min = (float)(qv - cfg.disp_tol);
    v_max = (float)(qv + cfg.disp_tol);
  }
  // The reference tests (float)u2 >= u_min && (float)u2 <= u_max (viso/matcher.cpp:943) on integer
  // coordinates: the same as lo <= u2 <= hi with lo = ceil(u_min), hi = floor(u_max).  Coordinates
  // are < 16384, so with both axes packed as 16-bit halves the whole window test is one wrapping
  // packed subtract, one packed min and one compare per candidate.
  const int lo_u = max((int)ceilf(u_min), 0), hi_u = min((int)floorf(u_max), 65535);
  const int lo_v = max((int)ceilf(v_min), 0), hi_v = min((int)floorf(v_max), 65535);
  const bool empty = hi_u < lo_u || hi_v < lo_v;
  // u-bins that can hold an in-window candidate: those of lo_u .. hi_u (a feature's bin is u / binsize, k_emit) - inside
  // the reference's floor(u_min / binsize) .. floor(u_max / binsize) (:929-932), and every candidate takes the exact window
  // test anyway; who wins a tie is settled by the candidates' ranks, not by the order of the visit
  const int ubmin = min(div_bin(min(lo_u, 65535), cfg), d.ub - 1);
  const int ubmax = min(div_bin(max(hi_u, 0), cfg), d.ub - 1);
  // fine rows that can hold an in-window candidate (a subset of the reference's v-bins vbmin..vbmax,
  // :933-934; every candidate still takes the exact window test below)
  const int vrows = d.vb * VSM_VSUB;
  const int vfmin = vfine_fast(min(lo_v, d.vb * cfg.binsize - 1), cfg, d.vb);
  const int vfmax = vfine_fast(min(max(hi_v, 0), d.vb * cfg.binsize - 1), cfg, d.vb);
  const uint32_t lo_pk = (uint32_t)lo_u | ((uint32_t)lo_v << 16);
  const uint32_t rng_pk = (uint32_t)(hi_u - lo_u) | ((uint32_t)(hi_v - lo_v) << 16);
  const bool pred = MAYPRED && (u_ >= 0 && v_ >= 0);
  // Two phases per stage.  (1) Walk the candidates: coordinates are packed (u | v << 16) and sorted
  // by fine bin, so one 16-byte load brings 4 consecutive candidates of this lane (one such load in
  // flight: two cost the registers of the fifth wave per SIMD, 71 -> 56 us for the first pass, 180 -> 175
  // for the second); the positions of the few that fall inside the window are parked
  // in a 4-deep per-lane register queue.  (2) Judge the parked candidates: descriptor + reference
  // rank fetch, SAD, and the double-precision distance term of a predicted match (:948-953) only
  // when the integer SAD alone does not already exceed the best cost (cost >= SAD).  A wavefront
  // runs phase 2 as many times as its busiest lane has candidates, not once per visited slot.
  // The reference keeps the FIRST minimum in its (u_bin, v_bin, index) visiting order (:937-958):
  // that is the minimum of (cost, rank), whatever order the candidates are judged in.
  // A stage that cannot have a prediction (MAYPRED = false) compares one integer key, SAD << 32 | rank; the others keep
  // the cost in double as the reference does.  The updates are selects, not branches.
  // (Round 4 tried the judging spread over the wave instead - the lanes' parked candidates compacted onto one list per wave
  // in LDS by ballots, 64 entries judged per round whoever found them, the owner's descriptor by cross-lane reads, the
  // minimum of (cost, rank) per query by ds_min_u64: results identical, but a wave-stage has 56 candidates on average
  // (1.74 per query), so four rounds become two, and the list's bookkeeping costs more than that: 345-370 us against 322.)
  double best = 10000000.0;
  uint64_t bkey = ~0ull;
  uint32_t bestq = VSM_NONE, brank = VSM_NONE;
  int nq = 0, q0p = 0, q1p = 0, q2p = 0, q3p = 0;
  auto judge = [&](int p) {
    const uint4 a = ldg_u4_at(B.s_desc, (uint32_t)p * 32u), b = ldg_u4_at(B.s_desc, (uint32_t)p * 32u + 16u);
    const uint32_t rk = ldg_u32_at(B.s_rank, (uint32_t)p * 4u);
    const uint32_t sad = sad32(q.da, q.db, a, b);
    if (!MAYPRED) {
      const uint64_t key = ((uint64_t)sad << 32) | rk;
      const bool better = key < bkey;
      bkey = better ? key : bkey;
      bestq = better ? (uint32_t)p : bestq;
    } else {
      double cost = (double)sad;
      if (cost <= best) {
        if (pred) {
          const uint32_t w = ldg_u32_at(B.s_uv, (uint32_t)p * 4u);
          double du = (double)(int)(w & 0xffffu) - u_;
          double dv = (double)(int)(w >> 16) - v_;
          double dist = sqrt(du * du + dv * dv);
          cost += 4 * dist;
        }
        const bool better = cost < best || (cost == best && rk < brank);
        best = better ? cost : best;
        brank = better ? rk : brank;
        bestq = better ? (uint32_t)p : bestq;
      }
    }
  };
  auto pop_and_judge = [&]() {  // lanes with a parked candidate take their newest one
    if (nq > 0) {
      const int p = q0p;
      q0p = q1p;
      q1p = q2p;
      q2p = q3p;
      nq--;
      judge(p);
    }
  };
  MT_PHASE(0);
  if (HEADS) {
  // The window's u-bins one after the other; of a bin's head record (k_feat_heads: 64 bytes = the run's start + the first 15
  // candidates' coordinates) every lane of the group loads its 16 / G dwords, next to the run's end: one round trip for
  // what the forms below take two or more for (bin starts, then coordinate loads that need them).
  constexpr int NDW = 16 / G;  // record dwords per lane
  auto park = [&](uint32_t w, int p, int q1) {
    const vsm_us2 off = __builtin_bit_cast(vsm_us2, w) - __builtin_bit_cast(vsm_us2, lo_pk);
    const vsm_us2 cl = __builtin_elementwise_min(off, __builtin_bit_cast(vsm_us2, rng_pk));
    if (__builtin_bit_cast(uint32_t, cl) == __builtin_bit_cast(uint32_t, off) && p < q1) {
      if (nq == 4) {  // queue full (rare): make room first
        const int pf = q3p;
        nq = 3;
        judge(pf);
      }
      q3p = q2p;
      q2p = q1p;
      q1p = q0p;
      q0p = p;
      nq++;
    }
  };
  for (int ubin = ubmin; ubin <= ubmax && !empty; ubin++) {
    const int b0 = (q.c * d.ub + ubin) * vrows;
    const uint32_t hb = (uint32_t)(b0 + vfmin) * 64u + (uint32_t)lane * (uint32_t)(4 * NDW);
    uint32_t r[NDW];
    if (NDW >= 4) {
#pragma unroll
      for (int j = 0; j < NDW / 4; j++) {
        const uint4 v = ldg_u4_at(B.heads, hb + 16u * j);
        r[4 * j + 0] = v.x;
        r[4 * j + 1] = v.y;
        r[4 * j + 2] = v.z;
        r[4 * j + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < NDW; j++) r[j] = ldg_u32_at(B.heads, hb + 4u * j);
    }
    const int q1 = (int)ldg_u32_at(B.bin_start, (uint32_t)(b0 + vfmax + 1) * 4u);
    const int q0 = __shfl((int)r[0], 0, G);  // (the group's lane 0 holds the record's first dword: the start)
#pragma unroll
    for (int i = 0; i < NDW; i++) {
      const int k = lane * NDW + i - 1;  // candidate number of this dword (-1: the start itself)
      if (i > 0 || lane > 0) park(r[i], q0 + k, q1);
    }
    for (int p0 = q0 + 15 + 4 * lane; p0 < q1; p0 += 4 * G) {  // a run of more than 15 candidates: the rest in 16-byte loads
      const uint4 wk = ldg_u4_at_dw(B.s_uv, (uint32_t)p0 * 4u);
      park(wk.x, p0, q1);
      park(wk.y, p0 + 1, q1);
      park(wk.z, p0 + 2, q1);
      park(wk.w, p0 + 3, q1);
    }
  }
  } else if (BYBIN) {
  // The lanes of a group take the window's u-bins in turn, each scanning its bin's run alone: a stereo stage's disparity
  // range spans 2-3 bins and an unconstrained first-pass window nine, with a handful of candidates in each - the wave goes
  // round ceil(bins / G) times instead of once per bin with most of a 16- or 32-slot sweep empty.  (BYBIN: the launches without prior
  // boxes - 88 -> 70 us per 67 pairs; with them the windows are narrow and sharing a bin's run is 2 % quicker.)
  for (int ubin = ubmin + lane; ubin <= ubmax && !empty; ubin += G) {
    const int b0 = (q.c * d.ub + ubin) * vrows;
    const int q0 = (int)ldg_u32_at(B.bin_start, (uint32_t)(b0 + vfmin) * 4u), q1 = (int)ldg_u32_at(B.bin_start, (uint32_t)(b0 + vfmax + 1) * 4u);
    for (int p0 = q0; p0 < q1; p0 += 4) {
      const uint4 wk = ldg_u4_at_dw(B.s_uv, (uint32_t)p0 * 4u);
      const uint32_t w4[4] = {wk.x, wk.y, wk.z, wk.w};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int p = p0 + k;
        const vsm_us2 off = __builtin_bit_cast(vsm_us2, w4[k]) - __builtin_bit_cast(vsm_us2, lo_pk);
        const vsm_us2 cl = __builtin_elementwise_min(off, __builtin_bit_cast(vsm_us2, rng_pk));
        if (__builtin_bit_cast(uint32_t, cl) == __builtin_bit_cast(uint32_t, off) && p < q1) {
          if (nq == 4) {  // queue full (rare): make room first
            const int pf = q3p;
            nq = 3;
            judge(pf);
          }
          q3p = q2p;
          q2p = q1p;
          q1p = q0p;
          q0p = p;
          nq++;
        }
      }
    }
  }
  } else {
  for (int ubin = ubmin; ubin <= ubmax && !empty; ubin++) {
    const int b0 = (q.c * d.ub + ubin) * vrows;
    const int q0 = (int)ldg_u32_at(B.bin_start, (uint32_t)(b0 + vfmin) * 4u), q1 = (int)ldg_u32_at(B.bin_start, (uint32_t)(b0 + vfmax + 1) * 4u);
    for (int p0 = q0 + 4 * lane; p0 < q1; p0 += 4 * G) {  // (the run's first candidate first: only the tail needs a bound)
      const uint4 wk = ldg_u4_at_dw(B.s_uv, (uint32_t)p0 * 4u);
      const uint32_t w4[4] = {wk.x, wk.y, wk.z, wk.w};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int p = p0 + k;
        const vsm_us2 off = __builtin_bit_cast(vsm_us2, w4[k]) - __builtin_bit_cast(vsm_us2, lo_pk);
        const vsm_us2 cl = __builtin_elementwise_min(off, __builtin_bit_cast(vsm_us2, rng_pk));
        if (__builtin_bit_cast(uint32_t, cl) == __builtin_bit_cast(uint32_t, off) && p < q1) {
          if (nq == 4) {  // queue full (rare): make room first
            const int pf = q3p;
            nq = 3;
            judge(pf);
          }
          q3p = q2p;
          q2p = q1p;
          q1p = q0p;
          q0p = p;
          nq++;
        }
      }
    }
  }
  }
  MT_PHASE(1);
  while (__any(nq > 0)) pop_and_judge();
  MT_PHASE(2);
  MT_PHASE_ADD(ph);
#pragma unroll
  for (int m = G / 2; m >= 1; m >>= 1) {
    const uint32_t oq = (uint32_t)__shfl_xor((int)bestq, m, G);
    if (!MAYPRED) {
      const uint32_t olo = (uint32_t)__shfl_xor((int)(uint32_t)bkey, m, G), ohi = (uint32_t)__shfl_xor((int)(uint32_t)(bkey >> 32), m, G);
      const uint64_t ok = ((uint64_t)ohi << 32) | olo;
      const bool better = ok < bkey;
      bkey = better ? ok : bkey;
      bestq = better ? oq : bestq;
    } else {
      const double oc = __shfl_xor(best, m, G);
      const uint32_t ork = (uint32_t)__shfl_xor((int)brank, m, G);
      const bool better = oc < best || (oc == best && ork < brank);
      best = better ? oc : best;
      bestq = better ? oq : bestq;
      brank = better ? ork : brank;
    }
  }
  if (!RELOAD) return bestq;
  if (bestq == VSM_NONE) {  // group-uniform
    q = load_query(B, 0);
    return VSM_NONE;
  }
  // every lane of the group fetches the winner's record (just touched, so it is in cache; handing it over from the lane
  // that judged it costs 20 registers and was measured 3 % quicker on pass 2, 15 % slower on pass 1; fetched by ONE lane and
  // passed on in nine shuffles - round 5 - 251 against 226 us alone: the shuffles and 32 bytes of spills cost more than the
  // lane accesses they save)
  q.uv = ldg_u32_at(B.s_uv, bestq * 4u);
  q.da = ldg_u4_at(B.s_desc, bestq * 32u);
  q.db = ldg_u4_at(B.s_desc, bestq * 32u + 16u);
  return bestq;
}

// (floor((float)u / (float)binsize) of the reference, :1020-1022, is u / binsize for these integers: u < 2^14)
__device__ __forceinline__ int stat_bin_of(int u, int v, const VsmMatchCfg &cfg, int ub, int vb) {
  return min(div_bin(v, cfg), vb - 1) * ub + min(div_bin(u, cfg), ub - 1);
}

__device__ __forceinline__ int index_of(const VsmSet &B, uint32_t pos) { return pos == VSM_NONE ? 0 : ldg_i32(B.s_idx + pos); }

template <int G, bool BYBIN = false, bool HEADS = false>
__global__ void __launch_bounds__(VSM_MATCH_BLOCK, VSM_MATCH_WAVES)
    k_match(const VsmImage *__restrict__ imgs, const VsmPair *__restrict__ pairs, const VsmJob *__restrict__ jobs,
            VsmJob job0, VsmDims d, VsmMatchCfg cfg, int nbx, int npairs) {
  // flattened grid: logical block -> (frame pair, block within pair), XCD-contiguous
  // (jobs == nullptr: the single pair `job0`)
  const int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int pj = lb / nbx, bx = lb - pj * nbx;
  if (pj >= npairs) return;
  const VsmJob &jb = jobs ? jobs[pj] : job0;
  const VsmPair &pair = pairs[pj];
  const int lane = threadIdx.x & (G - 1);
  const int qi = (bx * blockDim.x + threadIdx.x) / G;
  const int si = cfg.sparse ? 0 : 1;
  if (qi >= jb.nq[si]) return;
  long long *mtph = nullptr;  // (where find_match adds its phases' cycles: nowhere, but for a timing build)
  MT_BEGIN(mtph);
  const int img_prev = jb.img_prev, img_curr = jb.img_curr;
  const VsmSet &s1p = imgs[img_prev].set[si], &s2p = imgs[img_prev + 1].set[si];
  const VsmSet &s1c = imgs[img_curr].set[si], &s2c = imgs[img_curr + 1].set[si];
  const bool prior = cfg.use_prior != 0;
  vsm_p_match m;
  bool ok = false;
  // the statistics bin of a chain is that of its start feature (:1020-1022, :1104-1106); its four
  // per-stage boxes are fetched once
  VsmQuery q = load_query(cfg.method == 2 ? s1p : s1c, qi);
  // (stage-major on the device: one 16-byte load per stage, issued one stage ahead of its use)
  const float *rg = pair.ranges + 16 * stat_bin_of(q.u(), q.v(), cfg, d.ub, d.vb);
  auto box = [&](int stage) {  // {u_min, u_max, v_min, v_max} offsets of a stage
    if (!prior) return make_float4(0, 0, 0, 0);
    const uint4 r = ldg_u4(rg + 4 * stage);
    return make_float4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w));
  };
  const uint32_t w0 = q.uv;
  const int u0 = q.u(), v0 = q.v();
  if (cfg.method == 0) {  // flow, :1006-1041
    const float4 r0 = box(0), r1 = box(1);
    const uint32_t p1 = find_match<G, true, false, BYBIN, HEADS>(q, s1p, d, cfg, prior, r0.x, r0.y, r0.z, r0.w, true, -1, -1, lane);
    const int u1p = q.u(), v1p = q.v();
    const uint32_t p2 = find_match<G, true, false, BYBIN, HEADS>(q, s1c, d, cfg, prior, r1.x, r1.y, r1.z, r1.w, true, -1, -1, lane);
    const int i1p = index_of(s1p, p1), i1c2 = index_of(s1c, p2);
    ok = (i1c2 == qi);
    m = {(float)u1p, (float)v1p, i1p, -1.f, -1.f, -1, (float)u0, (float)v0, qi, -1.f, -1.f, -1};
  } else if (cfg.method == 1) {  // stereo, :1045-1084
    const float4 r0 = box(0), r1 = box(1);
    const uint32_t p1 = find_match<G, true, false, BYBIN || VSM_STEREO_BY_BIN, HEADS>(q, s2c, d, cfg, prior, r0.x, r0.y, r0.z, r0.w, false, -1, -1, lane);
    const int u2c = q.u(), v2c = q.v();
    const uint32_t p2 = find_match<G, true, false, BYBIN || VSM_STEREO_BY_BIN, HEADS>(q, s1c, d, cfg, prior, r1.x, r1.y, r1.z, r1.w, false, -1, -1, lane);
    const int i2c = index_of(s2c, p1), i1c2 = index_of(s1c, p2);
    ok = (i1c2 == qi) && (u0 >= u2c);
    m = {-1.f, -1.f, -1, -1.f, -1.f, -1, (float)u0, (float)v0, qi, (float)u2c, (float)v2c, i2c};
  } else {  // quad, :1088-1153
    // (stage results stay packed u | v << 16 until the record is written: registers decide how many
    // chains a SIMD keeps in flight)
    const float4 r0 = box(0), r1 = box(1);
    const uint32_t p1 = find_match<G, true, false, BYBIN || VSM_STEREO_BY_BIN, HEADS>(q, s2p, d, cfg, prior, r0.x, r0.y, r0.z, r0.w, false, -1, -1, lane, mtph);
    const uint32_t w2p = q.uv;
    MT_STAGE(1);
    double u2c_ = -1, v2c_ = -1;
    if (jb.use_tr) {  // :1114-1126, contraction-free double arithmetic
      double dd = (double)u0 - (double)q.u();
      if (!(dd > 1.0)) dd = 1.0;
      double x1p = ((double)u0 - cfg.cu) * cfg.base / dd;
      double y1p = ((double)v0 - cfg.cv) * cfg.base / dd;
      double z1p = cfg.f * cfg.base / dd;
      double x2c = jb.t[0] * x1p + jb.t[1] * y1p + jb.t[2] * z1p + jb.t[3] - cfg.base;
      double y2c = jb.t[4] * x1p + jb.t[5] * y1p + jb.t[6] * z1p + jb.t[7];
      double z2c = jb.t[8] * x1p + jb.t[9] * y1p + jb.t[10] * z1p + jb.t[11];
      u2c_ = cfg.f * x2c / z2c + cfg.cu;
      v2c_ = cfg.f * y2c / z2c + cfg.cv;
    }
    const float4 r2 = box(2);
    const uint32_t p2 = find_match<G, true, true, BYBIN, HEADS>(q, s2c, d, cfg, prior, r1.x, r1.y, r1.z, r1.w, true, u2c_, v2c_, lane, mtph);
    const uint32_t w2c = q.uv;
    MT_STAGE(2);
    const float4 r3 = box(3);
    const uint32_t p3 = find_match<G, true, false, BYBIN || VSM_STEREO_BY_BIN, HEADS>(q, s1c, d, cfg, prior, r2.x, r2.y, r2.z, r2.w, false, -1, -1, lane, mtph);
    const uint32_t w1c = q.uv;
    MT_STAGE(3);
    // stage 4 predicts the chain's own start (:1134)
    const uint32_t p4 = find_match<G, true, true, BYBIN, HEADS>(q, s1p, d, cfg, prior, r3.x, r3.y, r3.z, r3.w, true,
                                      jb.use_tr ? (double)(int)(w0 & 0xffffu) : -1.0,
                                      jb.use_tr ? (double)(int)(w0 >> 16) : -1.0, lane, mtph);
    const int i1p2 = index_of(s1p, p4);
    MT_STAGE(4);
    const int u2p = (int)(w2p & 0xffffu), u2c = (int)(w2c & 0xffffu), u1c = (int)(w1c & 0xffffu);
    ok = (i1p2 == qi) && (u0 >= u2p) && (u1c >= u2c);
    if (ok)
      m = {(float)u0, (float)v0, qi, (float)u2p, (float)(int)(w2p >> 16), index_of(s2p, p1), (float)u1c,
           (float)(int)(w1c >> 16), index_of(s1c, p3), (float)u2c, (float)(int)(w2c >> 16), index_of(s2c, p2)};
  }
  if (lane == 0) {
    pair.flag[qi] = ok ? 1 : 0;
    if (ok) pair.raw[qi] = m;
  }
  MT_END(mtph);
}

// key of list entry `pos` for the exact Delaunay chain (VsmDc2Job::keys_in; the casts are k_dc2_keys')
__device__ __forceinline__ uint64_t vsm_chain_key(float u1c, float v1c, int pos) {
  return ((uint64_t)(uint32_t)(int32_t)u1c << 34) | ((uint64_t)(uint32_t)(int32_t)v1c << 20) | (uint32_t)pos;
}

// ordered compaction of the accepted queries (push_back order = ascending query index) with the
// first-come pixel de-dup of flow / stereo (M[] in viso/matcher.cpp:1036-1039, :1078-1081):
// features sharing a pixel come from one NMS cell, hence are at most 3 indices apart.
// Two small kernels, 256 queries per block: k_compact_count leaves one survivor count per
// block, k_compact_write sums the counts of the blocks before it (a few hundred at most) and
// writes its survivors; nothing is serialised through one block.
__device__ __forceinline__ bool match_kept(const VsmPair &pair, int method, int i) {
  if (!pair.flag[i]) return false;
  if (method < 2) {
    const float u = pair.raw[i].u1c, v = pair.raw[i].v1c;
    for (int j = max(i - 3, 0); j < i; j++)
      if (pair.flag[j] && pair.raw[j].u1c == u && pair.raw[j].v1c == v) return false;
  }
  return true;
}

__global__ void __launch_bounds__(256)
    k_compact_count(const VsmPair *__restrict__ pairs, const VsmJob *__restrict__ jobs, VsmJob job0, int method, int pass) {
  __shared__ int s_cnt[4];
  const VsmPair &pair = pairs[blockIdx.y];
  const int n_query = (jobs ? jobs[blockIdx.y] : job0).nq[pass];
  if ((int)blockIdx.x * 256 >= n_query && blockIdx.x > 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool keep = i < n_query && match_kept(pair, method, i);
  const unsigned long long b = __ballot(keep);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) pair.blockcnt[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// (keys: the Delaunay chain's key of every list entry goes out with it, see k_compact_quad)
__global__ void __launch_bounds__(256)
    k_compact_write(const VsmPair *__restrict__ pairs, const VsmJob *__restrict__ jobs, VsmJob job0, int method, int pass, int keys, VsmKeyOut ko) {
  __shared__ int s_red[4];
  __shared__ int s_cnt[4];
  const VsmPair &pair = pairs[blockIdx.y];
  const int n_query = (jobs ? jobs[blockIdx.y] : job0).nq[pass];
  const int nblk = max((n_query + 255) / 256, 1);  // blocks that hold queries of this pair
  if ((int)blockIdx.x >= nblk) return;
  vsm_p_match *__restrict__ list = pass ? pair.list2 : pair.list1;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // base = survivors of all earlier blocks
  int part = 0;
  for (int b = threadIdx.x; b < (int)blockIdx.x; b += 256) part += pair.blockcnt[b];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o, 64);
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool keep = i < n_query && match_kept(pair, method, i);
  const unsigned long long bal = __ballot(keep);
  if (lane == 0) {
    s_red[wv] = part;
    s_cnt[wv] = __popcll(bal);
  }
  __syncthreads();
  int pos = s_red[0] + s_red[1] + s_red[2] + s_red[3];
  for (int w = 0; w < wv; w++) pos += s_cnt[w];
  pos += __popcll(bal & ((1ull << lane) - 1ull));
  if (keep) {
    // the record as its three 16-byte pieces, read once: piece 1 holds (u1c, v1c), as in k_compact_quad
    const uint4 *src = (const uint4 *)(pair.raw + i);
    uint4 *dst = (uint4 *)(list + pos);
    const uint4 r0 = src[0], r1 = src[1], r2 = src[2];
    dst[0] = r0;
    dst[1] = r1;
    dst[2] = r2;
    if (keys && pos < pair.key_cap[pass]) {
      const uint64_t key = vsm_chain_key(__uint_as_float(r1.z), __uint_as_float(r1.w), pos);
      pair.keys[pass][pos] = key;
      if (ko.host && pos < ko.host_cap) ((uint64_t *)((uint8_t *)ko.host + blockIdx.y * ko.host_stride))[pos] = key;
    }
  }
  if ((int)blockIdx.x == nblk - 1 && threadIdx.x == 255) {
    const int total = pos + (keep ? 1 : 0);
    pair.count[pass] = total;
    pair.hcount[pass] = total;
  }
}

// Quad matching keeps every accepted query (no pixel de-dup, viso/matcher.cpp:1139-1151): ordered compaction of raw[] into
// the list in ONE launch (the lists behind it, and the Delaunay chain behind those, wait for it).  A workgroup of 256
// threads takes QUAD_SPAN consecutive queries of a pair: it counts the acceptance flags in front of its span itself (every
// workgroup reads the pair's flags up to its own - a few KB out of L2 - so no workgroup waits for another), scans its own and
// moves the records as 16-byte pieces, consecutive lanes consecutive pieces of raw[].  Round 3's form - four workgroups of
// 1024 threads and 16 KB of LDS per pair - took 35 us per 67 pairs with the GPU to itself and 100-170 us in the pipeline,
// whatever was in it: a 16-wave workgroup needs four free wave slots on every SIMD of one compute unit plus its LDS at the
// same moment, and beside the Delaunay chains it waits for that.  Four waves and 4 KB find a place at once.
// EXPORT (the per-frame path, where a launch of its own for the copy is 8 us of a 0.5 ms frame): 1 - every piece goes to the
// list's host-mapped copy as well (k_export_list's work), 2 - the pixel (u1c, v1c) of every match as x | y << 16 to xy_dst
// (k_export_xy's).
// EXPORT 3 (the batched forms): the Delaunay chain's key of every match - its pixel and its place in the list - to the pair's
// keys[pass], made from the two words of piece 1 that EXPORT 2 packs; the chain starts on its sort without a pass of its own
// over the list (k_dc2_keys: 48 bytes read per match for 8 written).  Places at and beyond key_cap[pass] get no key.
// EXPORT 4: the same, and every key to the host-mapped array ko names as well (the forms whose single stream has nothing
// beside it to hold up: the pool's vertex sorts read them there).
#define QUAD_SPAN 1024
template <int EXPORT>
__global__ void __launch_bounds__(256)
    k_compact_quad(const VsmPair *__restrict__ pairs, const VsmJob *__restrict__ jobs, VsmJob job0, int pass, uint32_t *__restrict__ xy_dst, VsmKeyOut ko) {
  __shared__ int s_w[5];
  __shared__ int s_base[4];
  __shared__ int s_dst[QUAD_SPAN];  // place of every query of the span in the list, -1 = not accepted
  const VsmPair &pair = pairs[blockIdx.y];
  const int n_query = (jobs ? jobs[blockIdx.y] : job0).nq[pass];
  const int q0 = (int)blockIdx.x * QUAD_SPAN, q1 = min(n_query, q0 + QUAD_SPAN);
  if (q0 >= n_query && !(blockIdx.x == 0 && n_query == 0)) return;
  vsm_p_match *__restrict__ list = pass ? pair.list2 : pair.list1;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  // accepted queries in front of this span: four flags per thread and load
  int before = 0;
  {
    const int4 *f4 = (const int4 *)pair.flag;  // (flag[] is 16-byte aligned, q0 a multiple of 4)
    for (int i0 = t; i0 < q0 / 4; i0 += 4 * 256) {
      int4 f[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int i = i0 + 256 * k;
        f[k] = i < q0 / 4 ? f4[i] : make_int4(0, 0, 0, 0);
      }
#pragma unroll
      for (int k = 0; k < 4; k++) before += (f[k].x ? 1 : 0) + (f[k].y ? 1 : 0) + (f[k].z ? 1 : 0) + (f[k].w ? 1 : 0);
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) before += __shfl_xor(before, o, 64);
  if (lane == 0) s_base[wv] = before;
  // own flags: thread t owns queries q0 + 4 t .. q0 + 4 t + 3
  constexpr int RUN = QUAD_SPAN / 256;
  int keep[RUN], cnt = 0;
#pragma unroll
  for (int k = 0; k < RUN; k++) {
    const int i = q0 + t * RUN + k;
    keep[k] = i < q1 ? (pair.flag[i] ? 1 : 0) : 0;
    cnt += keep[k];
  }
  // exclusive scan over the 256 threads
  int incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  if (lane == 63) s_w[wv] = incl;
  __syncthreads();
  int pos = incl - cnt, total = 0, base = 0;
#pragma unroll
  for (int w = 0; w < 4; w++) {
    pos += w < wv ? s_w[w] : 0;
    total += s_w[w];
    base += s_base[w];
  }
  pos += base;
#pragma unroll
  for (int k = 0; k < RUN; k++) s_dst[t * RUN + k] = keep[k] ? pos++ : -1;
  __syncthreads();
  {
    const uint4 *src = (const uint4 *)(pair.raw + q0);
    uint4 *dst = (uint4 *)list;
    uint4 *hdst = EXPORT == 1 ? (uint4 *)(pass ? pair.hlist2 : pair.hlist1) : nullptr;
    uint64_t *__restrict__ keys = EXPORT >= 3 ? pair.keys[pass] : nullptr;
    uint64_t *__restrict__ hkeys = EXPORT == 4 ? (uint64_t *)((uint8_t *)ko.host + blockIdx.y * ko.host_stride) : nullptr;
    const int key_cap = EXPORT >= 3 ? pair.key_cap[pass] : 0;
    const int pieces = 3 * (q1 - q0);
    for (int p0 = t; p0 < pieces; p0 += 4 * 256) {
      uint4 v[4];
      int d[4], part[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int p = p0 + 256 * k;
        const int e = p / 3;
        part[k] = p - 3 * e;
        d[k] = p < pieces ? s_dst[e] : -1;
        v[k] = d[k] >= 0 ? src[p] : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (d[k] >= 0) {
          dst[3 * (size_t)d[k] + part[k]] = v[k];
          if (EXPORT == 1) hdst[3 * (size_t)d[k] + part[k]] = v[k];
          if (EXPORT == 2 && part[k] == 1)  // (piece 1 of a record: v2p, i2p, u1c, v1c)
            xy_dst[d[k]] = (uint32_t)(int32_t)__uint_as_float(v[k].z) | ((uint32_t)(int32_t)__uint_as_float(v[k].w) << 16);
          if (EXPORT >= 3 && part[k] == 1 && d[k] < key_cap) {
            const uint64_t key = vsm_chain_key(__uint_as_float(v[k].z), __uint_as_float(v[k].w), d[k]);
            keys[d[k]] = key;
            if (EXPORT == 4 && d[k] < ko.host_cap) hkeys[d[k]] = key;
          }
        }
    }
  }
  if (q1 == n_query && t == 255) {  // the span that holds the last query
    pair.count[pass] = base + total;
    pair.hcount[pass] = base + total;
  }
}

// wide copy of a finished list into host-mapped pinned memory (16 bytes per lane over PCIe):
// the host reads it after the stream sync, no D2H copy call and no second round trip
__global__ void __launch_bounds__(256)
    k_export_list(const VsmPair *__restrict__ pairs, int pass) {
  const VsmPair &pair = pairs[blockIdx.y];
  const int n16 = pair.count[pass] * 3;
  const uint4 *src = (const uint4 *)(pass ? pair.list2 : pair.list1);
  uint4 *dst = (uint4 *)(pass ? pair.hlist2 : pair.hlist1);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n16; i += gridDim.x * 256) dst[i] = src[i];
}

// the pixel of every match of the compacted pass-2 list as x | y << 16, into host-mapped memory: all the final
// removeOutliers' triangulation needs of the list ((u1c, v1c), which the refinement leaves alone, viso/matcher.cpp:1544-1577) -
// the per-frame path's host starts on it while the refinement and the list's export still run
__global__ void __launch_bounds__(256) k_export_xy(const VsmPair *__restrict__ pairs, uint32_t *__restrict__ dst) {
  const VsmPair &pair = pairs[0];
  const int n = pair.count[1];
  const vsm_p_match *__restrict__ src = pair.list2;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
    dst[i] = (uint32_t)(int32_t)src[i].u1c | ((uint32_t)(int32_t)src[i].v1c << 16);
}

// ---------------------------------------------------------------------------------------
// R1 refinement, viso/matcher.cpp:1498-1585.  One thread per (match, relocation step) evaluates
// the 25 candidate positions with the 16-byte ELAS descriptor (computeSmallDescriptor, :479-506)
// from the full-resolution Sobel planes; first-wins argmin in (dv, du) order.  Steps: 0 -> (u1p,v1p) [flow, quad], 1 -> (u2c,v2c) [stereo,
// quad], 2 -> (u2p,v2p) [quad]; each uses the unrefined (u1c,v1c) as its reference (:1544-1577).
// refinement==2 (parabolicFitting, :1379-1454): 49 lanes of a wave evaluate the 7x7 costs, the
// 3x3 neighbourhood around the minimum goes to the host, which solves the 9x6 least squares in
// double exactly as Matrix::solve does.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 small_desc(const uint8_t *__restrict__ du, const uint8_t *__restrict__ dv, int bpl,
                                            int u, int v) {
  const int a2 = v * bpl + u, a1 = a2 - bpl, a0 = a1 - bpl, a3 = a2 + bpl, a4 = a3 + bpl;
  uint4 r;
  r.x = du[a0] | (du[a1 - 2] << 8) | (du[a1] << 16) | ((uint32_t)du[a1 + 2] << 24);
  r.y = du[a2 - 1] | (du[a2] << 8) | (du[a2] << 16) | ((uint32_t)du[a2 + 1] << 24);
  r.z = du[a3 - 2] | (du[a3] << 8) | (du[a3 + 2] << 16) | ((uint32_t)du[a4] << 24);
  r.w = dv[a1] | (dv[a2 - 1] << 8) | (dv[a2 + 1] << 16) | ((uint32_t)dv[a3] << 24);
  return r;
}

// the same descriptor from the tiled plane
__device__ __forceinline__ uint4 small_desc_tiled(const uint8_t *__restrict__ t, int bpl, int u, int v) {
#define TDU(x, y) ((uint32_t)t[vsm_tiled_at(bpl, (x), (y))])
#define TDV(x, y) ((uint32_t)t[vsm_tiled_at(bpl, (x), (y)) + VSM_TILED_DV])
  uint4 r;
  r.x = TDU(u, v - 2) | (TDU(u - 2, v - 1) << 8) | (TDU(u, v - 1) << 16) | (TDU(u + 2, v - 1) << 24);
  r.y = TDU(u - 1, v) | (TDU(u, v) << 8) | (TDU(u, v) << 16) | (TDU(u + 1, v) << 24);
  r.z = TDU(u - 2, v + 1) | (TDU(u, v + 1) << 8) | (TDU(u + 2, v + 1) << 16) | (TDU(u, v + 2) << 24);
  r.w = TDV(u, v - 1) | (TDV(u - 1, v) << 8) | (TDV(u + 1, v) << 16) | (TDV(u, v + 1) << 24);
#undef TDU
#undef TDV
  return r;
}

__device__ __forceinline__ uint32_t sad16(const uint4 &a, const uint4 &b) {
  uint32_t s = __builtin_amdgcn_sad_u8(a.x, b.x, 0u);
  s = __builtin_amdgcn_sad_u8(a.y, b.y, s);
  s = __builtin_amdgcn_sad_u8(a.z, b.z, s);
  return __builtin_amdgcn_sad_u8(a.w, b.w, s);
}

// reference descriptor at (u1c, v1c) of the current left image (computeSmallDescriptor, :479-506):
// 5 du rows + 3 dv rows, columns u-2..u+2, each as two aligned dwords re-based with a funnel shift
// (8 wide loads instead of 16 byte gathers)
template <bool TILED>
__device__ __forceinline__ uint4 refine_ref_desc(const VsmImage &ref, const VsmDims &dc, int ru, int rv) {
  uint4 rd;
  const int b0 = (ru - 2) & ~3, rsh = 8 * ((ru - 2) - b0);
  uint64_t wu[5], wv[3];
  if (TILED) {
    // the two 4-pixel blocks holding columns ru-2 .. ru+2 (vsm_tiled_at of their first pixels)
    const int j0 = b0 >> 2;
#pragma unroll
    for (int r = 0; r < 5; r++) {
      const uint8_t *row = ref.duv_tiled;
      const uint32_t lo = ldg_u32(row + vsm_tiled_at(dc.bpl, 4 * j0, rv - 2 + r)), hi = ldg_u32(row + vsm_tiled_at(dc.bpl, 4 * j0 + 4, rv - 2 + r));
      wu[r] = ((((uint64_t)hi) << 32) | lo) >> rsh;
      if (r >= 1 && r <= 3) {
        const uint32_t lv = ldg_u32(row + vsm_tiled_at(dc.bpl, 4 * j0, rv - 2 + r) + VSM_TILED_DV), hv = ldg_u32(row + vsm_tiled_at(dc.bpl, 4 * j0 + 4, rv - 2 + r) + VSM_TILED_DV);
        wv[r - 1] = ((((uint64_t)hv) << 32) | lv) >> rsh;
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < 5; r++) {
      const uint32_t *pr = (const uint32_t *)(ref.du_full + (size_t)(rv - 2 + r) * dc.bpl + b0);
      wu[r] = ((((uint64_t)pr[1]) << 32) | pr[0]) >> rsh;
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const uint32_t *pr = (const uint32_t *)(ref.dv_full + (size_t)(rv - 1 + r) * dc.bpl + b0);
      wv[r] = ((((uint64_t)pr[1]) << 32) | pr[0]) >> rsh;
    }
  }
#define WB(w, c) ((uint32_t)((w) >> (8 * (c))) & 0xffu)
  rd.x = WB(wu[0], 2) | (WB(wu[1], 0) << 8) | (WB(wu[1], 2) << 16) | (WB(wu[1], 4) << 24);
  rd.y = WB(wu[2], 1) | (WB(wu[2], 2) << 8) | (WB(wu[2], 2) << 16) | (WB(wu[2], 3) << 24);
  rd.z = WB(wu[3], 0) | (WB(wu[3], 2) << 8) | (WB(wu[3], 4) << 16) | (WB(wu[4], 2) << 24);
  rd.w = WB(wv[0], 2) | (WB(wv[1], 1) << 8) | (WB(wv[1], 3) << 16) | (WB(wv[2], 2) << 24);
#undef WB
  return rd;
}

template <bool TILED>
__global__ void __launch_bounds__(256)
    k_refine(const VsmImage *__restrict__ imgs, const VsmPair *__restrict__ pairs, const VsmJob *__restrict__ jobs,
             VsmJob job0, VsmDims dp, VsmDims dc, int method, int nbx, int npairs) {
  // One thread per (match, relocation step).  The 9 x 9 du / 7 x 9 dv neighbourhood of the target
  // is pulled into registers with 48 independent dword loads (rows are 16-byte aligned, each row is
  // re-based to column u2-4 with a funnel shift), then the 25 candidate descriptors are pure
  // register byte-picks + v_sad_u8: no dependent gathers, no cross-lane traffic.
  // flattened grid: logical block -> (pair, block within pair), XCD-contiguous
  const int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int pj = lb / nbx, bx = lb - pj * nbx;
  if (pj >= npairs) return;
  const VsmJob &jb = jobs ? jobs[pj] : job0;
  const VsmPair &pair = pairs[pj];
  const int g = bx * blockDim.x + threadIdx.x;
  const int mi = g / 3, step = g - mi * 3;
  const VsmImage &ref = imgs[jb.img_curr];
  // The reference descriptor of a match is the same for its three steps: lanes 0..21 of a wave compute those of the
  // wave's (at most 22) matches, one each - a third of the lanes in contiguous quads, which is what the texture
  // addresser's time goes by - and every lane picks its match's up with a cross-lane read.
  uint4 rd;
  {
    const int lane = threadIdx.x & 63;
    const int first_mi = (g - lane) / 3, rmi = first_mi + lane;
    uint4 mine = make_uint4(0, 0, 0, 0);
    if (lane < 22 && rmi < pair.count[1]) {
      const vsm_p_match *rm = pair.list2 + rmi;
      mine = refine_ref_desc<TILED>(ref, dc, (int)rm->u1c, (int)rm->v1c);
    }
    const int src = mi - first_mi;
    rd.x = (uint32_t)__shfl((int)mine.x, src, 64);
    rd.y = (uint32_t)__shfl((int)mine.y, src, 64);
    rd.z = (uint32_t)__shfl((int)mine.z, src, 64);
    rd.w = (uint32_t)__shfl((int)mine.w, src, 64);
  }
  if (mi >= pair.count[1]) return;
  if (step == 0 && !(method == 0 || method == 2)) return;
  if (step == 1 && !(method == 1 || method == 2)) return;
  if (step == 2 && method != 2) return;
  vsm_p_match *m = pair.list2 + mi;  // refined in place (each step owns its two fields)
  const VsmImage &tgt = step == 0 ? imgs[jb.img_prev] : (step == 1 ? imgs[jb.img_curr + 1] : imgs[jb.img_prev + 1]);
  const VsmDims &dt = step == 1 ? dc : dp;
  float *pu = step == 0 ? &m->u1p : (step == 1 ? &m->u2c : &m->u2p);
  float *pv = pu + 1;
  const float u2 = *pu, v2 = *pv;
  if (u2 - 2 < VSM_MARGIN || u2 + 2 > dt.w - 1 - VSM_MARGIN || v2 - 2 < VSM_MARGIN || v2 + 2 > dt.h - 1 - VSM_MARGIN)
    return;
  const int iu = (int)u2, iv = (int)v2;
  uint32_t U[9][3], V[9][3];
  if (TILED) {
    // tiled plane: the 9 columns iu-4 .. iu+4 start at pixel o = (iu-4) & 7 of a tile row and end in the next tile; one
    // 16-byte load per tile row brings du 0-3, dv 0-3, du 4-7, dv 4-7
    const int o = (iu - 4) & 7, b = o >> 2;
    const uint32_t sb = (uint32_t)(o & 3);
#pragma unroll
    for (int r = 0; r < 9; r++) {
      const uint8_t *pr = tgt.duv_tiled + vsm_tiled_at(dt.bpl, (iu - 4) & ~7, iv - 4 + r);
      const uint4 t0 = ldg_u4(pr), t1 = ldg_u4(pr + 128);
      const uint32_t d0 = b ? t0.z : t0.x, d1 = b ? t1.x : t0.z, d2 = b ? t1.z : t1.x;
      U[r][0] = __builtin_amdgcn_alignbyte(d1, d0, sb);
      U[r][1] = __builtin_amdgcn_alignbyte(d2, d1, sb);
      U[r][2] = d2 >> (8 * sb);
      const uint32_t e0 = b ? t0.w : t0.y, e1 = b ? t1.y : t0.w, e2 = b ? t1.w : t1.y;
      V[r][0] = __builtin_amdgcn_alignbyte(e1, e0, sb);
      V[r][1] = __builtin_amdgcn_alignbyte(e2, e1, sb);
      V[r][2] = e2 >> (8 * sb);
    }
  } else {
    const int a0 = (iu - 4) & ~3, sh = 8 * ((iu - 4) - a0);
#pragma unroll
    for (int r = 0; r < 9; r++) {
      const uint32_t *pr = (const uint32_t *)(tgt.du_full + (size_t)(iv - 4 + r) * dt.bpl + a0);
      const uint32_t d0 = pr[0], d1 = pr[1], d2 = pr[2];
      U[r][0] = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh);
      U[r][1] = (uint32_t)((((uint64_t)d2 << 32) | d1) >> sh);
      U[r][2] = d2 >> sh;
      if (r >= 1 && r <= 7) {
        const uint32_t *qr = (const uint32_t *)(tgt.dv_full + (size_t)(iv - 4 + r) * dt.bpl + a0);
        const uint32_t e0 = qr[0], e1 = qr[1], e2 = qr[2];
        V[r][0] = (uint32_t)((((uint64_t)e1 << 32) | e0) >> sh);
        V[r][1] = (uint32_t)((((uint64_t)e2 << 32) | e1) >> sh);
        V[r][2] = e2 >> sh;
      } else {
        V[r][0] = V[r][1] = V[r][2] = 0;
      }
    }
  }
#define UB(r, c) ((U[(r)][(c) >> 2] >> (8 * ((c)&3))) & 0xffu)
#define VB(r, c) ((V[(r)][(c) >> 2] >> (8 * ((c)&3))) & 0xffu)
  uint32_t best = 0xffffffffu;
  int ind = 0;
#pragma unroll
  for (int ddv = 0; ddv < 5; ddv++) {
#pragma unroll
    for (int ddu = 0; ddu < 5; ddu++) {
      const int r = ddv + 2, c = ddu + 2;  // candidate centre in window coordinates
      uint4 t;
      t.x = UB(r - 2, c) | (UB(r - 1, c - 2) << 8) | (UB(r - 1, c) << 16) | (UB(r - 1, c + 2) << 24);
      t.y = UB(r, c - 1) | (UB(r, c) << 8) | (UB(r, c) << 16) | (UB(r, c + 1) << 24);
      t.z = UB(r + 1, c - 2) | (UB(r + 1, c) << 8) | (UB(r + 1, c + 2) << 16) | (UB(r + 2, c) << 24);
      t.w = VB(r - 1, c) | (VB(r, c - 1) << 8) | (VB(r, c + 1) << 16) | (VB(r + 1, c) << 24);
      const uint32_t cost = sad16(rd, t);
      if (cost < best) {  // first minimum in (dv, du) order, viso/matcher.cpp:1484-1491
        best = cost;
        ind = ddv * 5 + ddu;
      }
    }
  }
#undef UB
#undef VB
  *pu = (float)((double)u2 + ((double)(float)(ind % 5) - 2.0));
  *pv = (float)((double)v2 + ((double)(float)(ind / 5) - 2.0));
}

__global__ void __launch_bounds__(256)
    k_parabolic_costs(const VsmImage *__restrict__ imgs, const VsmPair *__restrict__ pairs,
                      const VsmJob *__restrict__ jobs, VsmJob job0, VsmDims dp, VsmDims dc, int method) {
  const VsmJob &jb = jobs ? jobs[blockIdx.y] : job0;
  const VsmPair &pair = pairs[blockIdx.y];
  const int img_prev = jb.img_prev, img_curr = jb.img_curr;
  const int lane = threadIdx.x & 63;
  const int g = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // one wave per (match, step)
  const int mi = g / 3, step = g - mi * 3;
  if (mi >= pair.count[1]) return;
  int32_t *out = pair.pf + ((size_t)mi * 3 + step) * 12;
  bool active = !((step == 0 && !(method == 0 || method == 2)) || (step == 1 && !(method == 1 || method == 2)) ||
                  (step == 2 && method != 2));
  if (!active) {
    if (lane == 0) out[0] = 2;  // step not applicable
    return;
  }
  const vsm_p_match *m = pair.list2 + mi;
  const VsmImage &ref = imgs[img_curr];
  const VsmImage &tgt = step == 0 ? imgs[img_prev] : (step == 1 ? imgs[img_curr + 1] : imgs[img_prev + 1]);
  const VsmDims &dt = step == 1 ? dc : dp;
  const float u2 = step == 0 ? m->u1p : (step == 1 ? m->u2c : m->u2p);
  const float v2 = step == 0 ? m->v1p : (step == 1 ? m->v2c : m->v2p);
  if (u2 - 3 < VSM_MARGIN || u2 + 3 > dt.w - 1 - VSM_MARGIN || v2 - 3 < VSM_MARGIN || v2 + 3 > dt.h - 1 - VSM_MARGIN) {
    if (lane == 0) out[0] = 0;  // infeasible: match dropped (wave-uniform branch)
    return;
  }
  const bool tiled = ref.duv_tiled != nullptr;
  const uint4 r = tiled ? small_desc_tiled(ref.duv_tiled, dc.bpl, (int)m->u1c, (int)m->v1c)
                        : small_desc(ref.du_full, ref.dv_full, dc.bpl, (int)m->u1c, (int)m->v1c);
  uint32_t key = 0xffffffffu;
  int cost = 0;
  if (lane < 49) {
    const int ddv = lane / 7, ddu = lane - ddv * 7;
    const uint4 t = tiled ? small_desc_tiled(tgt.duv_tiled, dt.bpl, (int)u2 + ddu - 3, (int)v2 + ddv - 3)
                          : small_desc(tgt.du_full, tgt.dv_full, dt.bpl, (int)u2 + ddu - 3, (int)v2 + ddv - 3);
    cost = (int)sad16(r, t);
    key = ((uint32_t)cost << 6) | (uint32_t)lane;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, o, 64));
  // key is now wave-uniform: first minimum in (dv, du) order
  const int ind = key & 63, du = ind % 7, dv = ind / 7;
  const bool border = (du == 0 || du == 6 || dv == 0 || dv == 6);
  int c9[9];
#pragma unroll
  for (int k = 0; k < 9; k++) {
    int src = border ? 0 : (dv + k / 3 - 1) * 7 + (du + k % 3 - 1);
    c9[k] = __shfl(cost, src, 64);
  }
  if (lane == 0) {
    if (border) {
      out[0] = 0;
    } else {
      out[0] = 1;
      out[1] = du;
      out[2] = dv;
#pragma unroll
      for (int k = 0; k < 9; k++) out[3 + k] = c9[k];
    }
  }
}

// ---------------------------------------------------------------------------------------
// refinement==2 in the batched (look-ahead) path: the least-squares tail of parabolicFitting (viso/matcher.cpp:1425-1453;
// host form: vsm_host_parabolic_update, vsm_host.cpp) and the removal of the matches whose fit fails (:1541-1581), on the
// device.  Matrix::operator* and Matrix::solve (Gauss-Jordan with full pivoting, viso/matrix.cpp) are + - * / and
// comparisons in double, evaluated here in the reference's order: IEEE arithmetic on either side, contraction off, so the
// same bits.  One workgroup per pair: every thread fits its matches and parks the updated records in raw[], a scan over
// the verdicts gives the survivors their places, the records move back into the list as 16-byte pieces.
// ---------------------------------------------------------------------------------------
// The system matrix At*A is the same for every fit, so the elimination's pivots, row swaps and multipliers are too: the
// host runs Gauss-Jordan on it ONCE (same IEEE double arithmetic, contraction off) and records, per step, what the
// reference does to the right-hand side - swap B[irow], B[icol]; B[icol] *= pivinv; B[ll] -= B[icol] * dum[ll] - and the
// device replays exactly those operations on every fit's b: the same bits as solving the whole system each time, without
// a 6 x 6 matrix per thread.
struct VsmParaPlan {
  int32_t ok, irow[6], icol[6];
  double pivinv[6], dum[6][6];
};
static const double kParaA[9][6] = {{1, 1, 1, -1, -1, 1}, {0, 1, 0, 0, -1, 1}, {1, 1, -1, 1, -1, 1}, {1, 0, 0, -1, 0, 1}, {0, 0, 0, 0, 0, 1},
                                    {1, 0, 0, 1, 0, 1},   {1, 1, -1, -1, 1, 1}, {0, 1, 0, 0, 1, 1},  {1, 1, 1, 1, 1, 1}};
static VsmParaPlan make_para_plan() {  // Matrix::solve (viso/matrix.cpp) on At*A, the right-hand side's share recorded
  VsmParaPlan pl = VsmParaPlan();
  double A[6][6];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double t = 0;
      for (int k = 0; k < 9; k++) t += kParaA[k][i] * kParaA[k][j];
      A[i][j] = t;
    }
  int ipiv[6] = {0, 0, 0, 0, 0, 0};
  int icol = 0, irow = 0;
  pl.ok = 1;
  for (int i = 0; i < 6; i++) {
    double big = 0.0;
    for (int j = 0; j < 6; j++)
      if (ipiv[j] != 1)
        for (int k = 0; k < 6; k++)
          if (ipiv[k] == 0 && fabs(A[j][k]) >= big) {
            big = fabs(A[j][k]);
            irow = j;
            icol = k;
          }
    ++ipiv[icol];
    pl.irow[i] = irow;
    pl.icol[i] = icol;
    if (irow != icol)
      for (int l = 0; l < 6; l++) std::swap(A[irow][l], A[icol][l]);
    if (fabs(A[icol][icol]) < 1e-20) {
      pl.ok = 0;
      return pl;
    }
    const double pivinv = 1.0 / A[icol][icol];
    pl.pivinv[i] = pivinv;
    A[icol][icol] = 1.0;
    for (int l = 0; l < 6; l++) A[icol][l] *= pivinv;
    for (int ll = 0; ll < 6; ll++)
      if (ll != icol) {
        const double dum = A[ll][icol];
        pl.dum[i][ll] = dum;
        A[ll][icol] = 0.0;
        for (int l = 0; l < 6; l++) A[ll][l] -= A[icol][l] * dum;
      }
  }
  return pl;
}
__device__ inline double para_get(const double b[6], int i) {
  return i == 0 ? b[0] : (i == 1 ? b[1] : (i == 2 ? b[2] : (i == 3 ? b[3] : (i == 4 ? b[4] : b[5]))));
}
__device__ inline void para_set(double b[6], int i, double v) {
#pragma unroll
  for (int k = 0; k < 6; k++) b[k] = k == i ? v : b[k];
}
__device__ inline bool dev_parabolic_update(const VsmParaPlan &pl, const int32_t *c9, int du, int dv, float &u2, float &v2) {
  constexpr double kA[9][6] = {{1, 1, 1, -1, -1, 1}, {0, 1, 0, 0, -1, 1}, {1, 1, -1, 1, -1, 1}, {1, 0, 0, -1, 0, 1}, {0, 0, 0, 0, 0, 1},
                               {1, 0, 0, 1, 0, 1},   {1, 1, -1, -1, 1, 1}, {0, 1, 0, 0, 1, 1},  {1, 1, 1, 1, 1, 1}};
  double b[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {  // b = At * c (Matrix::operator*: the sum over k in order, zero terms included)
    double s = 0;
#pragma unroll
    for (int k = 0; k < 9; k++) s += kA[k][i] * (double)c9[k];
    b[i] = s;
  }
  if (!pl.ok) return false;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const int irow = pl.irow[i], icol = pl.icol[i];
    if (irow != icol) {
      const double x = para_get(b, irow), y = para_get(b, icol);
      para_set(b, irow, y);
      para_set(b, icol, x);
    }
    const double bc = para_get(b, icol) * pl.pivinv[i];
    para_set(b, icol, bc);
#pragma unroll
    for (int ll = 0; ll < 6; ll++)
      if (ll != icol) b[ll] -= bc * pl.dum[i][ll];
  }
  const float divisor = (float)(b[2] * b[2] - 4.0 * b[0] * b[1]);
  if ((double)fabsf(divisor) < 1e-8 || fabs(b[2]) < 1e-8) return false;
  const float ddv = (float)((2.0 * b[0] * b[4] - b[2] * b[3]) / (double)divisor);
  const float ddu = (float)(-(b[4] + 2.0 * b[1] * (double)ddv) / b[2]);
  if ((double)fabsf(ddu) >= 1.0 || (double)fabsf(ddv) >= 1.0) return false;
  u2 = (float)((double)u2 + ((double)(float)du - 3.0 + (double)ddu));
  v2 = (float)((double)v2 + ((double)(float)dv - 3.0 + (double)ddv));
  return true;
}
#define PARA_MAX_LIST 16384  // matches per pair this kernel takes (16-bit places in LDS)
__global__ void __launch_bounds__(1024) k_parabolic_apply(const VsmPair *__restrict__ pairs, VsmParaPlan pl) {
  __shared__ uint16_t s_dst[PARA_MAX_LIST];  // the match's place among the survivors, 0xffff = dropped
  __shared__ int s_w[17];
  const VsmPair &pair = pairs[blockIdx.x];
  const int n = min(pair.count[1], PARA_MAX_LIST);
  const int t = threadIdx.x;
  // thread t owns the run of matches [t * run, t * run + run)
  const int run = (n + 1023) / 1024;
  int cnt = 0;
  for (int k = 0; k < run; k++) {
    const int i = t * run + k;
    if (i >= n) break;
    vsm_p_match m = pair.list2[i];
    bool ok = true;
    float *tu[3] = {&m.u1p, &m.u2c, &m.u2p}, *tv[3] = {&m.v1p, &m.v2c, &m.v2p};
    for (int st = 0; st < 3 && ok; st++) {
      const int32_t *r = pair.pf + ((size_t)i * 3 + st) * 12;
      if (r[0] == 2) continue;  // step not applicable to the matching method
      ok = r[0] == 1 && dev_parabolic_update(pl, r + 3, r[1], r[2], *tu[st], *tv[st]);
    }
    pair.raw[i] = m;
    s_dst[i] = ok ? 1 : 0;
    cnt += ok ? 1 : 0;
  }
  int total;
  int pos = block_excl_scan_1024(cnt, total, s_w);
  for (int k = 0; k < run; k++) {
    const int i = t * run + k;
    if (i >= n) break;
    s_dst[i] = s_dst[i] ? (uint16_t)pos++ : (uint16_t)0xffffu;
  }
  __syncthreads();  // (raw[] written above is read below by other threads of this workgroup, and only by them)
  const uint4 *src = (const uint4 *)pair.raw;
  uint4 *dst = (uint4 *)pair.list2;
  for (int p = t; p < 3 * n; p += 1024) {
    const int e = p / 3;
    const uint32_t d = s_dst[e];
    if (d != 0xffffu) dst[3 * (size_t)d + (p - 3 * e)] = src[p];
  }
  if (t == 0) {
    pair.count[1] = total;
    pair.hcount[1] = total;
  }
}

// ---------------------------------------------------------------------------------------
// Small tables (job descriptions of a chunk: 10-20 KB) from pinned host memory to HBM by a kernel on the stream that needs
// them, not by hipMemcpyAsync.  The runtime takes a copy of more than 16 KB to a DMA engine, and when that engine is busy
// with another upload - two chunks' tables now and then - it falls back to a shader copy on a hardware queue of its own,
// which it creates then and there: 180 MB of context-save area mapped and touched, 6-7 ms during which every launch of
// the process waits (the "once per process" stall of round 4; tools/stall_probe.py, tools/shim/mmap_trace.c).
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_upload(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, int n_words) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_words) dst[i] = src[i];
}

hipError_t vsm_upload(hipStream_t s, void *dst_device, const void *src_pinned, size_t bytes) {
  if (bytes == 0) return hipSuccess;
  if ((bytes & 3) || ((uintptr_t)dst_device & 3) || ((uintptr_t)src_pinned & 3)) return hipMemcpyAsync(dst_device, src_pinned, bytes, hipMemcpyHostToDevice, s);
  const int n = (int)(bytes >> 2);
  hipLaunchKernelGGL(k_upload, dim3((n + 255) / 256), dim3(256), 0, s, (uint32_t *)dst_device, (const uint32_t *)src_pinned, n);
  return hipGetLastError();
}

// =======================================================================================
// launchers
// =======================================================================================

// One launch serves `npairs` frame pairs (blockIdx.y); jobs == nullptr: the single pair job0.
// pass: 0 = sparse lists (list1/hlist1/count[0]), 1 = dense lists.  max_nq bounds nq[pass].
bool vsm_launch_match(hipStream_t s, VsmProf &pf, const VsmImage *d_imgs, const VsmPair *d_pairs, const VsmJob *d_jobs,
                      const VsmJob &job0, int npairs, const VsmDims &d, const VsmMatchCfg &cfg, int max_nq, int fuse_export, uint32_t *xy_dst, const VsmKeyOut *keys) {
  // lanes per query: the chain is latency-bound per wavefront, so big batches want many
  // queries per wave (G = 2..4) and a lone frame pair wants more lanes per query (G = 8).
  const long total_q = (long)npairs * max_nq;
  const int G = total_q >= 200000 ? VSM_MATCH_GBIG : (total_q >= 30000 ? 4 : 8);
  const int pass = cfg.sparse ? 0 : 1;
  if (max_nq > 0) {
    pf.begin(cfg.sparse ? VSM_K_MATCH1 : VSM_K_MATCH2, s);
    const int nbx = cdiv(max_nq * G, VSM_MATCH_BLOCK);
    const dim3 grid(((nbx * npairs + 7) / 8) * 8);
    // without prior boxes (first pass, single-pass matching) the lanes of a group take whole u-bins
#define VSM_MATCH_LAUNCH(GG)                                                                                                       \
  do {                                                                                                                             \
    if (cfg.use_prior && cfg.heads && !cfg.sparse)                                                                                 \
      hipLaunchKernelGGL((k_match<GG, false, true>), grid, dim3(VSM_MATCH_BLOCK), 0, s, d_imgs, d_pairs, d_jobs, job0, d, cfg, nbx, npairs); \
    else if (cfg.use_prior)                                                                                                        \
      hipLaunchKernelGGL((k_match<GG, false>), grid, dim3(VSM_MATCH_BLOCK), 0, s, d_imgs, d_pairs, d_jobs, job0, d, cfg, nbx, npairs); \
    else                                                                                                                           \
      hipLaunchKernelGGL((k_match<GG, true>), grid, dim3(VSM_MATCH_BLOCK), 0, s, d_imgs, d_pairs, d_jobs, job0, d, cfg, nbx, npairs);  \
  } while (0)
    if (G == 1)
      VSM_MATCH_LAUNCH(1);
    else if (G == 2)
      VSM_MATCH_LAUNCH(2);
    else if (G == 4)
      VSM_MATCH_LAUNCH(4);
    else if (G == 16)
      VSM_MATCH_LAUNCH(16);
    else
      VSM_MATCH_LAUNCH(8);
    pf.end(s);
  }
  pf.begin(cfg.sparse ? VSM_K_COMPACT1 : VSM_K_COMPACT2, s);
  const bool fused = vsm_launch_compact(s, d_pairs, d_jobs, job0, npairs, cfg.method, pass, max_nq, keys, fuse_export, xy_dst);
  pf.end(s);
  return fused;  // the export asked for went along with the compaction (quad matching): no launch of its own
}

// the ordered compaction of a matching pass: which kernel form takes it (the one place that decides; the return value as above)
bool vsm_launch_compact(hipStream_t s, const VsmPair *d_pairs, const VsmJob *d_jobs, const VsmJob &job0, int npairs, int method, int pass, int max_nq,
                        const VsmKeyOut *keys, int fuse_export, uint32_t *xy_dst) {
  const VsmKeyOut ko = keys ? *keys : VsmKeyOut{nullptr, 0, 0};
  if (method == 2) {
    const dim3 grid(std::max(1, cdiv(max_nq, QUAD_SPAN)), npairs);
    const bool fused = fuse_export == 1 || (fuse_export == 2 && xy_dst && npairs == 1);
    if (keys && !fuse_export && ko.host)
      hipLaunchKernelGGL(k_compact_quad<4>, grid, dim3(256), 0, s, d_pairs, d_jobs, job0, pass, nullptr, ko);
    else if (keys && !fuse_export)
      hipLaunchKernelGGL(k_compact_quad<3>, grid, dim3(256), 0, s, d_pairs, d_jobs, job0, pass, nullptr, ko);
    else if (fuse_export == 1)
      hipLaunchKernelGGL(k_compact_quad<1>, grid, dim3(256), 0, s, d_pairs, d_jobs, job0, pass, nullptr, ko);
    else if (fused)
      hipLaunchKernelGGL(k_compact_quad<2>, grid, dim3(256), 0, s, d_pairs, d_jobs, job0, pass, xy_dst, ko);
    else
      hipLaunchKernelGGL(k_compact_quad<0>, grid, dim3(256), 0, s, d_pairs, d_jobs, job0, pass, nullptr, ko);
    return fused;
  }
  const int nblk = max(cdiv(max_nq, 256), 1);
  hipLaunchKernelGGL(k_compact_count, dim3(nblk, npairs), dim3(256), 0, s, d_pairs, d_jobs, job0, method, pass);
  hipLaunchKernelGGL(k_compact_write, dim3(nblk, npairs), dim3(256), 0, s, d_pairs, d_jobs, job0, method, pass, keys && !fuse_export ? 1 : 0, ko);
  return false;
}

void vsm_launch_export(hipStream_t s, VsmProf &pf, const VsmPair *d_pairs, int npairs, int pass, int n_upper) {
  pf.begin(VSM_K_EXPORT, s);
  hipLaunchKernelGGL(k_export_list, dim3(max(min(cdiv(n_upper * 3, 256), 256), 1), npairs), dim3(256), 0, s, d_pairs,
                     pass);
  pf.end(s);
}

void vsm_launch_export_xy(hipStream_t s, const VsmPair *d_pairs, uint32_t *dst_host_mapped, int n_upper) {
  hipLaunchKernelGGL(k_export_xy, dim3(max(min(cdiv(n_upper, 256), 64), 1)), dim3(256), 0, s, d_pairs, dst_host_mapped);
}

// the batched tail of refinement==2 (behind vsm_launch_refine): fits, dropped matches, the lists closed up again
void vsm_launch_parabolic_apply(hipStream_t s, VsmProf &pf, const VsmPair *d_pairs, int npairs) {
  if (npairs <= 0) return;
  static const VsmParaPlan plan = make_para_plan();
  pf.begin(VSM_K_PARA_APPLY, s);
  hipLaunchKernelGGL(k_parabolic_apply, dim3(npairs), dim3(1024), 0, s, d_pairs, plan);
  pf.end(s);
}

void vsm_launch_refine(hipStream_t s, VsmProf &pf, const VsmImage *d_imgs, const VsmPair *d_pairs, const VsmJob *d_jobs,
                       const VsmJob &job0, int npairs, const VsmDims &dp, const VsmDims &dc, int method, int refinement,
                       int n_upper) {
  // n_upper bounds the list sizes (they are still device-only); surplus groups exit at once
  if (n_upper <= 0) return;
  pf.begin(VSM_K_REFINE, s);
  if (refinement == 2)
    hipLaunchKernelGGL(k_parabolic_costs, dim3(cdiv(n_upper * 3 * 64, 256), npairs), dim3(256), 0, s, d_imgs, d_pairs,
                       d_jobs, job0, dp, dc, method);
  else
  {
    const int nbx = cdiv(n_upper * 3, 256), tot = ((nbx * npairs + 7) / 8) * 8;
    if (dc.scale == 2)
      hipLaunchKernelGGL(k_refine<true>, dim3(tot), dim3(256), 0, s, d_imgs, d_pairs, d_jobs, job0, dp, dc, method, nbx, npairs);
    else
      hipLaunchKernelGGL(k_refine<false>, dim3(tot), dim3(256), 0, s, d_imgs, d_pairs, d_jobs, job0, dp, dc, method, nbx, npairs);
  }
  pf.end(s);
}
