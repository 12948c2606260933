// Device-side helpers that both kernel units (vsm_image.hip, vsm_match.hip) use: global-address-space loaders, the XCD block
// remap, the tiled Sobel plane's addressing, the search-bin arithmetic and the block-wide scan.  A helper of one unit stays there.
#pragma once

#include "vsm_internal.h"

#define WAVE 64

// Pointers that come out of the VsmImage / VsmSet tables are "generic" to the compiler, which then
// emits flat_load (address-space check, and every wait on LDS traffic also waits for them).  They
// all point into HBM: these helpers load through an explicit global-address-space pointer.
#define VSM_AS1 __attribute__((address_space(1)))
typedef uint32_t vsm_u4 __attribute__((ext_vector_type(4)));
typedef int32_t vsm_i4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ldg_u4(const void *p) {
  const vsm_u4 v = *(const VSM_AS1 vsm_u4 *)p;
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ int4 ldg_i4(const void *p) {
  const vsm_i4 v = *(const VSM_AS1 vsm_i4 *)p;
  return make_int4(v.x, v.y, v.z, v.w);
}
// base + 32-bit byte offset: with a wave-uniform base the backend keeps the base in scalar registers and the offset in one
// vector register (global_load ... v_off, s[base]) instead of building a 64-bit address per lane
__device__ __forceinline__ uint4 ldg_u4_at(const void *base, uint32_t byte_off) {
  const vsm_u4 v = *(const VSM_AS1 vsm_u4 *)((const VSM_AS1 char *)base + byte_off);
  return make_uint4(v.x, v.y, v.z, v.w);
}
// 16 bytes at a dword-aligned (not 16-byte-aligned) offset: one global_load_dwordx4 all the same
typedef uint32_t vsm_u4_a4 __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ uint4 ldg_u4_at_dw(const void *base, uint32_t byte_off) {
  const vsm_u4_a4 v = *(const VSM_AS1 vsm_u4_a4 *)((const VSM_AS1 char *)base + byte_off);
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint32_t ldg_u32_at(const void *base, uint32_t byte_off) {
  return *(const VSM_AS1 uint32_t *)((const VSM_AS1 char *)base + byte_off);
}
__device__ __forceinline__ int32_t ldg_i32(const void *p) { return *(const VSM_AS1 int32_t *)p; }
__device__ __forceinline__ uint32_t ldg_u32(const void *p) { return *(const VSM_AS1 uint32_t *)p; }

// XCD-aware block remap (MI355X: 8 XCDs, each with a private 4 MiB L2; hardware deals blocks
// round-robin over the XCDs).  Batched launches are flattened to 1-D and logical block
// L = (b % 8) * ceil(n/8) + b / 8, so every XCD walks one contiguous eighth of the (pair-major)
// work and the eight L2s stop fetching the same image lines.  Speed only, never correctness.
__device__ __forceinline__ int xcd_remap(int b, int nblocks) {
  const int per = (nblocks + 7) >> 3;
  return (b & 7) * per + (b >> 3);
}

// ---------------------------------------------------------------------------------------
// Full-resolution Sobel planes of half_resolution = 1 (read by the refinement only, as scattered 9 x 9 neighbourhoods):
// ONE plane of 8 x 8-pixel tiles, 128 bytes each = one cache line; a tile row is 16 bytes: du of pixels 0-3, dv of pixels
// 0-3, du of 4-7, dv of 4-7 (what a filter thread produces for its 4-pixel patch row is one 8-byte store).  A refinement
// window (9 rows x 9 columns of both responses) lies in exactly 4 lines instead of 16, its row in two 16-byte loads.
// du of pixel (x, y) at vsm_tiled_at(bpl, x, y), dv VSM_TILED_DV bytes further.
// ---------------------------------------------------------------------------------------
#define VSM_TILED_DV 4
__host__ __device__ __forceinline__ size_t vsm_tiled_at(int bpl, int x, int y) {
  return ((size_t)(y >> 3) * (size_t)(bpl >> 3) + (size_t)(x >> 3)) * 128 + (size_t)((y & 7) * 16 + ((x & 4) << 1) + (x & 3));
}

// fine v row of a (non-negative) coordinate: v-bin * VSM_VSUB + sub-row inside the bin; monotonic in v
__device__ __forceinline__ int vfine_of(int v, int binsize, int vb) {
  const int vbin = min(v / binsize, vb - 1);
  return vbin * VSM_VSUB + min(((v - vbin * binsize) * VSM_VSUB) / binsize, VSM_VSUB - 1);
}

// fine bin id; id / VSM_VSUB is the reference's bin (class * ub + u_bin) * vb + v_bin (viso/matcher.cpp:881-888)
__device__ __forceinline__ int bin_of(int u, int v, int c, int binsize, int ub, int vb) {
  const int ubin = min(u / binsize, ub - 1);
  return (c * ub + ubin) * (vb * VSM_VSUB) + vfine_of(v, binsize, vb);
}

// the same with the division by the bin size as a multiply-high (cfg.bin_magic): k_match runs it several times per stage,
// and an integer division by a run-time value costs ~20 instructions.  Exact for 0 <= x < 2^32 / binsize; the arguments
// here are below 2^17 and the host refuses bin sizes above 32768.
__device__ __forceinline__ int div_bin(int x, const VsmMatchCfg &cfg) {
  return cfg.binsize == 1 ? x : (int)__umulhi((uint32_t)x, cfg.bin_magic);
}
__device__ __forceinline__ int vfine_fast(int v, const VsmMatchCfg &cfg, int vb) {
  const int vbin = min(div_bin(v, cfg), vb - 1);
  return vbin * VSM_VSUB + min(div_bin((v - vbin * cfg.binsize) * VSM_VSUB, cfg), VSM_VSUB - 1);
}

// block-wide exclusive scan of one int per thread (blockDim.x == 1024); returns the exclusive
// prefix and the block total.  Wave shuffles + one LDS hop.
__device__ __forceinline__ int block_excl_scan_1024(int v, int &total, int *s_w /*[17]*/) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  __syncthreads();  // protects s_w reuse across calls
  if (lane == 63) s_w[wv] = x;
  __syncthreads();
  if (wv == 0) {
    int w = lane < 16 ? s_w[lane] : 0;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      int y = __shfl_up(w, o, 64);
      if (lane >= o) w += y;
    }
    if (lane < 16) s_w[lane] = w;  // inclusive wave totals
  }
  __syncthreads();
  total = s_w[15];
  int wbase = wv ? s_w[wv - 1] : 0;
  return wbase + x - v;
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
