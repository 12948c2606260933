// gfx950 (MI355X, CDNA4) kernels of the image side of the matcher hot path: everything that only sees a VsmImage - ingest, front
// end, filters, suppression, the fused tiles, feature records and bin order.  The pair side (match chain .. refinement) is
// vsm_match.hip; what both use is vsm_dev.h.  Wave = 64 lanes.
//
// All kernels are integer/byte work bounded by HBM (or, for one 1242x375 pair, by launch and
// dependent-load latency): no MFMA anywhere.  Every kernel takes a z (or y) grid dimension
// over images / frame pairs so the same code serves the per-frame API (2 images, 1 pair) and
// batched sequences (hundreds of images per launch), which is what fills 256 CUs.
//
// Semantics are those of the reference (pad bytes pinned to 0, filters on the 1-D byte stream);
// file:line citations below refer to the reference repository.

#include <stdlib.h>

#include <algorithm>

#include "vsm_internal.h"
#include "vsm_dev.h"
#include "vsm_feat.h"

#ifdef VSM_FEAT_TIMING  // experiments (tools/build_variant.sh NAME -DVSM_FEAT_TIMING, tools/feat_timing.py): cycles per phase of every wave
__device__ unsigned int vsm_ft_rec[5][1 << 16][10];  // [kernel][wave] start (low bits), phase lengths ...
extern "C" int vsm_debug_feat_rec(unsigned int *out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(vsm_ft_rec), sizeof(vsm_ft_rec)) != hipSuccess) return -1;
  (void)reset;
  return 0;
}
#define FT_DECL unsigned long long ft_t[10]; int ft_n = 0
#define FT_STAMP ft_t[ft_n++] = __builtin_amdgcn_s_memtime()
#define FT_FLUSH(kern)                                                              \
  do {                                                                              \
    const unsigned wv = ((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6); \
    if ((threadIdx.x & 63) == 0 && wv < (1u << 16)) {                               \
      vsm_ft_rec[kern][wv][0] = (unsigned)ft_t[0] | 1u;                             \
      for (int q = 1; q < ft_n; q++) vsm_ft_rec[kern][wv][q] = (unsigned)(ft_t[q] - ft_t[q - 1]); \
    }                                                                               \
  } while (0)
#else
#define FT_DECL
#define FT_STAMP
#define FT_FLUSH(base)
#endif

// ---------------------------------------------------------------------------------------
// ingest: caller image (row stride src_bpl) -> padded HBM copy [h][bpl], pad bytes = 0
// (Matcher::pushBack row copy, viso/matcher.cpp:163-175, with the pad pinned to 0)
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_ingest(const VsmImage *__restrict__ imgs, int first, const uint8_t *__restrict__ src0,
                                                const uint8_t *__restrict__ src1, size_t frame_stride, int src_bpl,
                                                int sides, int w, int h, int bpl) {
  // blockIdx.z = frame*sides + side; image id = first + 2*frame + side.  Threads are laid over the
  // padded image as one stream of dwords.  Caller rows need not be dword aligned (a 1242-pixel row
  // stride is not): every output dword comes from the two aligned source dwords around it and a byte
  // funnel shift; nothing past the last pixel of a row is touched.
  const int fr = blockIdx.z / sides, side = blockIdx.z - fr * sides;
  const uint8_t *__restrict__ src = (side ? src1 : src0) + (size_t)fr * frame_stride;
  uint8_t *__restrict__ dst = imgs[first + 2 * fr + side].img;
  const int per_row = bpl >> 2;
  const int gidx = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = gidx / per_row, x4 = (gidx - y * per_row) * 4;
  if (y >= h) return;
  uint32_t v = 0;
  if (x4 < w) {
    const uintptr_t a = (uintptr_t)(src + (size_t)y * src_bpl + x4);
    const uint32_t sh = (uint32_t)(a & 3);
    const int nvalid = min(4, w - x4);  // bytes of this dword that belong to the row
    const uint32_t lo = ldg_u32((const void *)(a - sh));
    const uint32_t hi = ((int)(4 - sh) < nvalid) ? ldg_u32((const void *)(a - sh + 4)) : 0u;
    v = __builtin_amdgcn_alignbyte(hi, lo, sh);
    if (nvalid < 4) v &= (1u << (8 * nvalid)) - 1u;
  }
  *(VSM_AS1 uint32_t *)(dst + (size_t)y * bpl + x4) = v;
}

// ---------------------------------------------------------------------------------------
// F0 createHalfResolutionImage, viso/matcher.cpp:636-647: (a+b+c+d)/4 over 2x2, pad = 0
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_halve(const VsmImage *__restrict__ imgs, int first, VsmDims d) {
  const VsmImage &im = imgs[first + blockIdx.z];
  int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  int y = blockIdx.y;
  if (x4 >= d.mbpl) return;
  const uint8_t *r0 = im.img + (size_t)(2 * y) * d.bpl + 2 * x4;
  const uint8_t *r1 = r0 + d.bpl;
  uint32_t a0 = 0, a1 = 0, b0 = 0, b1 = 0;
  if (2 * x4 < d.bpl) {
    a0 = *(const uint32_t *)r0;
    b0 = *(const uint32_t *)r1;
  }
  if (2 * x4 + 4 < d.bpl) {
    a1 = *(const uint32_t *)(r0 + 4);
    b1 = *(const uint32_t *)(r1 + 4);
  }
  uint32_t out = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    uint32_t ta = k < 2 ? a0 : a1, tb = k < 2 ? b0 : b1;
    int sh = (k & 1) * 16;
    uint32_t s = ((ta >> sh) & 0xff) + ((ta >> (sh + 8)) & 0xff) + ((tb >> sh) & 0xff) + ((tb >> (sh + 8)) & 0xff);
    if (x4 + k < d.mw) out |= (s >> 2) << (8 * k);
  }
  *(uint32_t *)(im.imgm + (size_t)y * d.mbpl + x4) = out;
}

// ---------------------------------------------------------------------------------------
// F1-F3 image filters on the byte stream of one image (row wrap = the reference's SSE loops):
//   du,dv : filter::sobel5x5, viso/filter.cpp:316-324 (+128, >>7, unsigned saturate)
//   f1    : filter::blob5x5,  viso/filter.cpp:343-365  (-box5 + 2*box3 + 7*centre)
//   f2    : filter::checkerboard5x5, viso/filter.cpp:331-336 (c (x) c, c = 1,1,0,-1,-1)
// One thread produces a 4 x 4 pixel patch from an 8-row x 12-byte window held packed in 24
// registers (24 dword loads for 16 pixels; horizontal neighbours share lines in L1); per patch
// row it stores one dword of du, one of dv and, for the matching-resolution image, 8 bytes each
// of f1 and f2.  FULL = true: full-resolution image -> du_full,dv_full only.
// ---------------------------------------------------------------------------------------
#define FPB(r, i) ((int)((Wn[(r)][(i) >> 2] >> (8 * ((i)&3))) & 0xffu))
template <bool FULL>
__global__ void __launch_bounds__(256)
    k_filters(const VsmImage *__restrict__ imgs, int first, int bpl, int h, int16_t *__restrict__ f1base,
              int16_t *__restrict__ f2base, size_t f_stride) {
  const VsmImage &im = imgs[first + blockIdx.z];
  const uint8_t *__restrict__ in = FULL ? im.img : im.imgm;
  const int n = bpl * h;
  const int x4 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;  // 64 x 4 threads per block: 256 px x 16 rows
  const int y0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * 4;
  if (x4 >= bpl || y0 >= h) return;
  // window rows y0-2 .. y0+5, stream bytes x4-4 .. x4+7 of each
  uint32_t Wn[8][3];
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const int base = (y0 + r - 2) * bpl + x4;
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const int a = base + (q - 1) * 4;
      Wn[r][q] = (a >= 0 && a < n) ? *(const uint32_t *)(in + a) : 0u;
    }
  }
  const int lo = 2 * bpl, hi = (h - 2) * bpl;
  uint8_t *__restrict__ odu = FULL ? im.duv_tiled : im.du;
  uint8_t *__restrict__ odv = FULL ? im.duv_tiled + VSM_TILED_DV : im.dv;
  int16_t *f1 = FULL ? nullptr : f1base + (size_t)blockIdx.z * f_stride;
  int16_t *f2 = FULL ? nullptr : f2base + (size_t)blockIdx.z * f_stride;
#pragma unroll
  for (int rr = 0; rr < 4; rr++) {
    const int y = y0 + rr;
    if (y >= h) break;
    const int f0 = y * bpl + x4;
    // column pass at stream positions f0-2 .. f0+5 (window index 2..9); zero outside rows [2,h-3]
    int S[8], D[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int g = f0 + i - 2;
      const bool ok = g >= lo && g < hi;
      const int a = FPB(rr, i + 2), b = FPB(rr + 1, i + 2), c = FPB(rr + 2, i + 2), dd = FPB(rr + 3, i + 2),
                e = FPB(rr + 4, i + 2);
      S[i] = ok ? a + 4 * b + 6 * c + 4 * dd + e : 0;
      D[i] = ok ? a + 2 * b - 2 * dd - e : 0;
    }
    uint32_t du = 0, dv = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int hu = S[k] + 2 * S[k + 1] - 2 * S[k + 3] - S[k + 4];
      const int hv = D[k] + 4 * D[k + 1] + 6 * D[k + 2] + 4 * D[k + 3] + D[k + 4];
      du |= (uint32_t)min(max((hu >> 7) + 128, 0), 255) << (8 * k);
      dv |= (uint32_t)min(max((hv >> 7) + 128, 0), 255) << (8 * k);
    }
    const size_t o0 = FULL ? vsm_tiled_at(bpl, x4, y) : (size_t)f0;
    *(uint32_t *)(odu + o0) = du;
    *(uint32_t *)(odv + o0) = dv;
    if (!FULL) {
      int16_t o1[4], o2[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int i = 4 + k, x = x4 + k;
        int b5 = 0, b3 = 0, ck = 0;
#pragma unroll
        for (int r = 0; r < 5; r++) {
          const int r3 = FPB(rr + r, i - 1) + FPB(rr + r, i) + FPB(rr + r, i + 1);
          const int r5 = r3 + FPB(rr + r, i - 2) + FPB(rr + r, i + 2);
          const int rd = FPB(rr + r, i - 2) + FPB(rr + r, i - 1) - FPB(rr + r, i + 1) - FPB(rr + r, i + 2);
          b5 += r5;
          if (r >= 1 && r <= 3) b3 += r3;
          ck += (r < 2) ? rd : (r > 2 ? -rd : 0);
        }
        const bool in1 = x >= 3 && x <= bpl - 3 && y >= 3 && y <= h - 3;
        const bool in2 = x >= 2 && x <= bpl - 3 && y >= 2 && y <= h - 3;
        o1[k] = in1 ? (int16_t)(-b5 + 2 * b3 + 7 * FPB(rr + 2, i)) : (int16_t)0;
        o2[k] = in2 ? (int16_t)ck : (int16_t)0;
      }
      *(uint2 *)(f1 + f0) = make_uint2((uint16_t)o1[0] | ((uint32_t)(uint16_t)o1[1] << 16),
                                       (uint16_t)o1[2] | ((uint32_t)(uint16_t)o1[3] << 16));
      *(uint2 *)(f2 + f0) = make_uint2((uint16_t)o2[0] | ((uint32_t)(uint16_t)o2[1] << 16),
                                       (uint16_t)o2[2] | ((uint32_t)(uint16_t)o2[3] << 16));
    }
  }
}
#undef FPB

// ---------------------------------------------------------------------------------------
// Fused front end for half_resolution = 1: ONE pass over the caller's image produces what k_ingest + k_halve +
// k_filters<true> produced in three (each streaming the full image): the padded copy (only where something reads it
// later - the per-frame path's getGain), the half-resolution image (F0, viso/matcher.cpp:636-647) and the full-resolution
// Sobel planes (F1, viso/filter.cpp:316-324), which only the refinement reads.
// A block owns a tile of 128 x 64 pixels.  Its 68 x 136 bytes of input (2 rows / 4 bytes of halo) go to LDS as coalesced
// loads in the layout of the PADDED byte stream (row stride bpl, pad bytes 0, positions outside the image 0 - the
// reference's filters run over that stream and wrap at row ends): caller rows need no alignment (aligned loads and a
// byte funnel shift per LDS dword, as in k_ingest).  Then every thread takes an 8 x 4 patch from an 8-row x 16-byte LDS
// window (two pixels per instruction, vsm_feat.h) and 8 half-resolution pixels.
// ---------------------------------------------------------------------------------------
#define FRONT_TW 128
#define FRONT_TH 64
#define FRONT_LPAD 16  // (8 is all the patches read; with 16 a row is nine WHOLE 16-byte items and an interior tile never takes the dword path)
#define FRONT_LW (FRONT_TW + FRONT_LPAD)  // bytes per LDS row
#define FRONT_LH (FRONT_TH + 4)
__global__ void __launch_bounds__(256)
    k_front(const VsmImage *__restrict__ imgs, int first, const uint8_t *__restrict__ src0, const uint8_t *__restrict__ src1,
            size_t frame_stride, int src_bpl, int sides, VsmDims d, int write_img, int nbx, int nby, int n_img) {
  __shared__ __attribute__((aligned(16))) uint32_t s_in[FRONT_LH][FRONT_LW / 4];
  // (XCD-aware placement: neighbouring tiles share the 128-byte lines their unaligned rows straddle and two halo rows; dealt
  // round-robin over the eight L2s every such line was fetched from HBM twice: 1.41 x the kernel's bytes)
  const int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int zi = lb / (nbx * nby), rem = lb - zi * (nbx * nby);
  if (zi >= n_img) return;
  const int by = rem / nbx, bx = rem - by * nbx;
  const int fr = zi / sides, side = zi - fr * sides;
  const uint8_t *__restrict__ src = (side ? src1 : src0) + (size_t)fr * frame_stride;
  const VsmImage &im = imgs[first + 2 * fr + side];
  const int bpl = d.bpl, h = d.h, w = d.w;
  const int x0 = bx * FRONT_TW, y0 = by * FRONT_TH;
  const int t = threadIdx.x;
  // ---- tile of the padded stream into LDS ----
  // Items of four LDS dwords (16 stream bytes; a row is nine whole items).  An item that lies inside one image row
  // takes ONE aligned 16-byte load plus one dword and four byte-aligns; the others (row ends, tile edges, rows outside the
  // image) go dword by dword: two aligned dwords + an align each, bytes beyond the row's w and positions outside the
  // image 0.  (Every 4-byte piece used to cost two loads: the kernel was bound by the texture addresser's lane rate.)
  auto load_dword = [&](int y, int x) -> uint32_t {  // stream position y * bpl + x; x may run into the neighbouring stream rows
    if (x < 0) {
      x += bpl;
      y -= 1;
    } else if (x >= bpl) {
      x -= bpl;
      y += 1;
    }
    uint32_t v = 0;
    if (y >= 0 && y < h && x < w) {
      const uintptr_t a = (uintptr_t)(src + (size_t)y * src_bpl + x);
      const uint32_t sh = (uint32_t)(a & 3);
      const int nvalid = min(4, w - x);  // bytes of this dword that belong to the row
      const uint32_t lo = ldg_u32((const void *)(a - sh));
      const uint32_t hi = ((int)(4 - sh) < nvalid) ? ldg_u32((const void *)(a - sh + 4)) : 0u;
      v = __builtin_amdgcn_alignbyte(hi, lo, sh);
      if (nvalid < 4) v &= (1u << (8 * nvalid)) - 1u;
    }
    return v;
  };
  FT_DECL;
  FT_STAMP;
  static_assert((FRONT_LW & 15) == 0, "a row is whole 16-byte items");
  constexpr int kItems = FRONT_LW / 16;  // per row
  constexpr int kIters = (FRONT_LH * kItems + 255) / 256;
  // (all of a thread's wide loads are requested before the first LDS store waits for one: three round trips become one)
  uint4 q[kIters];
  uint32_t q4[kIters];
#pragma unroll
  for (int i = 0; i < kIters; i++) {
    const int e = t + 256 * i, r = e / kItems, g = e - r * kItems;
    const int y = y0 - 2 + r, x = x0 - 4 + 16 * g;
    // dwords of the item.  A row is whole items, so this is always 4; it stays a min() because the compiler does not see
    // that, keeps the dword loops below rolled, and so emits the device code of a9ef39f (1782 instructions; 2105 with a plain 4).
    const int nd = min(4, FRONT_LW / 4 - 4 * g);
    q[i] = make_uint4(0u, 0u, 0u, 0u);
    q4[i] = 0u;
    if (e < FRONT_LH * kItems && nd == 4 && y >= 0 && y < h && x >= 0 && x + 20 <= w) {
      const uintptr_t a = (uintptr_t)(src + (size_t)y * src_bpl + x);
      const uint32_t sh = (uint32_t)(a & 3);
      q[i] = ldg_u4((const void *)(a - sh));
      q4[i] = ldg_u32((const void *)(a - sh + 16));
    }
  }
#pragma unroll
  for (int i = 0; i < kIters; i++) {
    const int e = t + 256 * i, r = e / kItems, g = e - r * kItems;
    if (e >= FRONT_LH * kItems) continue;
    const int y = y0 - 2 + r, x = x0 - 4 + 16 * g;
    const int nd = min(4, FRONT_LW / 4 - 4 * g);  // (always 4; a min() for the same reason as above)
    if (nd == 4 && y >= 0 && y < h && x >= 0 && x + 20 <= w) {
      const uint32_t sh = (uint32_t)((uintptr_t)(src + (size_t)y * src_bpl + x) & 3);
      uint4 v;
      v.x = __builtin_amdgcn_alignbyte(q[i].y, q[i].x, sh);
      v.y = __builtin_amdgcn_alignbyte(q[i].z, q[i].y, sh);
      v.z = __builtin_amdgcn_alignbyte(q[i].w, q[i].z, sh);
      v.w = __builtin_amdgcn_alignbyte(q4[i], q[i].w, sh);
      *(uint4 *)&s_in[r][4 * g] = v;  // (rows of whole items are 16-byte aligned)
    } else if ((y < 0 || y >= h) && x >= 0 && x + 16 <= bpl) {  // a row outside the image whose item does not wrap into one inside
      for (int k = 0; k < nd; k++) s_in[r][4 * g + k] = 0u;
    } else {
      for (int k = 0; k < nd; k++) s_in[r][4 * g + k] = load_dword(y, x + 4 * k);
    }
  }
  FT_STAMP;
  __syncthreads();
  FT_STAMP;
  // ---- padded copy (pad bytes 0), where asked for ----
  if (write_img) {
    for (int e = t; e < FRONT_TH * (FRONT_TW / 4); e += 256) {
      const int r = e / (FRONT_TW / 4), c = e - r * (FRONT_TW / 4);
      const int y = y0 + r, x4 = x0 + 4 * c;
      if (y < h && x4 < bpl) *(VSM_AS1 uint32_t *)(im.img + (size_t)y * bpl + x4) = s_in[r + 2][c + 1];
    }
  }
  // ---- half-resolution image: 64 x 32 pixels of this tile, 2 x 4 per thread ----
#pragma unroll
  for (int k2 = 0; k2 < FRONT_TH / 32; k2++) {
    const int idx = t + 256 * k2, hy = idx >> 4, hx4 = (idx & 15) * 4;
    const int my = (y0 >> 1) + hy, mx4 = (x0 >> 1) + hx4;
    if (my < d.mh && mx4 < d.mbpl) {
      const uint32_t a0 = s_in[2 + 2 * hy][1 + (hx4 >> 1)], a1 = s_in[2 + 2 * hy][2 + (hx4 >> 1)];
      const uint32_t b0 = s_in[3 + 2 * hy][1 + (hx4 >> 1)], b1 = s_in[3 + 2 * hy][2 + (hx4 >> 1)];
      uint32_t out = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t ta = k < 2 ? a0 : a1, tb = k < 2 ? b0 : b1;
        const int sh = (k & 1) * 16;
        const uint32_t sum = ((ta >> sh) & 0xff) + ((ta >> (sh + 8)) & 0xff) + ((tb >> sh) & 0xff) + ((tb >> (sh + 8)) & 0xff);
        if (mx4 + k < d.mw) out |= (sum >> 2) << (8 * k);
      }
      *(VSM_AS1 uint32_t *)(im.imgm + (size_t)my * d.mbpl + mx4) = out;
    }
  }
  FT_STAMP;
  // ---- full-resolution Sobel: an 8 x 4 patch per thread from a window of 8 rows x 16 bytes, two pixels per instruction in
  // 16-bit lanes (vsm_feat.h: the same column / row passes as the matching-resolution tiles); a patch row = du 0-3, dv 0-3,
  // du 4-7, dv 4-7 = one 16-byte row of the tiled plane ----
  static_assert(FRONT_TW == 128 && FRONT_TH == 64, "16 x 16 patches of 8 x 4 pixels");
  const int tx = t & 15, ty = t >> 4;
  const int x8 = x0 + 8 * tx, yb = y0 + 4 * ty;
  if (x8 >= bpl || yb >= h) return;
  VfWindow<4> W;
#pragma unroll
  for (int r = 0; r < 8; r++) {
#pragma unroll
    for (int q = 0; q < 4; q++) W.w[r][q] = s_in[4 * ty + r][2 * tx + q];
  }
  // the column sums of the patch's four rows share their stages (vf_columns_sobel_all)
  vf_s2 Sa[4][6], Da[4][6];
#pragma unroll
  for (int j = 0; j < 6; j++) {
    vf_s2 sj[4], dj[4];
    vf_columns_sobel_all<4>(W, j, sj, dj);
#pragma unroll
    for (int rr = 0; rr < 4; rr++) Sa[rr][j] = sj[rr], Da[rr][j] = dj[rr];
  }
#pragma unroll
  for (int rr = 0; rr < 4; rr++) {
    const int y = yb + rr;
    if (y >= h) break;
    vf_s2 (&S)[6] = Sa[rr], (&D)[6] = Da[rr];
    if (y < 3 || y > h - 4) vf_sobel_zero_outside(S, D, y * bpl + x8, 2 * bpl, (h - 2) * bpl);
    uint32_t du[2], dv[2];
    vf_sobel_row(S, D, du, dv);
    vsm_u4 o;
    o.x = du[0];
    o.y = dv[0];
    o.z = du[1];
    o.w = dv[1];
    *(VSM_AS1 vsm_u4 *)(im.duv_tiled + vsm_tiled_at(bpl, x8, y)) = o;
  }
  FT_STAMP;
  FT_FLUSH(4);
}

// ---------------------------------------------------------------------------------------
// N1 nonMaximumSuppression, viso/matcher.cpp:330-431 (Neubeck & Van Gool alg. 4).
// One wavefront per (cell, filter).  Lanes load the (n+1)^2 cell pixels (u fastest: contiguous
// int16 rows) and a 64-lane min-reduction over the key (value, scan position) yields the
// reference's first-wins extremum ("u outer, v inner, strict compare", :356-380): position
// o = di*(n+1)+dj.  The (2n+1)^2 suppression windows (:383-428) are then tested lane-parallel and
// folded with a ballot.  blockIdx.y: 0 = f1, 1 = f2; blockIdx.z = image*2 + set.
// Survivors go to cand[cell*4 + class] as u | v<<14 | 1<<31.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}

__device__ __forceinline__ bool nms_suppressed_wave(const int16_t *__restrict__ f, int bpl, int w, int h, int n, int i,
                                                    int j, int ci, int cj, int val, bool want_min, int lane) {
  const int W = 2 * n + 1;
  const int i_hi = min(ci + n, w - 1 - VSM_MARGIN), j_hi = min(cj + n, h - 1 - VSM_MARGIN);
  bool hit = false;
  for (int e = lane; e < W * W; e += 64) {
    const int dj = e / W, di = e - dj * W;
    const int i2 = ci - n + di, j2 = cj - n + dj;
    if (i2 <= i_hi && j2 <= j_hi) {
      const int cur = f[j2 * bpl + i2];
      const bool better = want_min ? (cur < val) : (cur > val);
      hit |= better && (i2 < i || i2 > i + n || j2 < j || j2 > j + n);
    }
  }
  return __ballot(hit) != 0ull;
}

__global__ void __launch_bounds__(256) k_nms(const VsmImage *__restrict__ imgs, int first, VsmDims d,
                                             const int16_t *__restrict__ f1base, const int16_t *__restrict__ f2base,
                                             size_t f_stride, int tau, int set_lo, int set_hi) {
  const int zi = blockIdx.z >> 1, si = (blockIdx.z & 1);
  if (si < set_lo || si > set_hi) return;
  const VsmSet &st = imgs[first + zi].set[si];
  const int ncells = st.ncu * st.ncv;
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  if (t >= ncells) return;
  const int k = blockIdx.y;
  const int16_t *__restrict__ f = (k ? f2base : f1base) + (size_t)zi * f_stride;
  const int n = st.nms_n, n1 = n + 1;
  const int cj = t / st.ncu, ci = t - cj * st.ncu;
  const int i = n + VSM_MARGIN + ci * n1, j = n + VSM_MARGIN + cj * n1;
  uint32_t kmin = 0xffffffffu, kmax = 0xffffffffu;
  for (int e = lane; e < n1 * n1; e += 64) {
    const int dj = e / n1, di = e - dj * n1;
    const int val = f[(j + dj) * d.mbpl + i + di];
    const uint32_t o = (uint32_t)(di * n1 + dj);
    kmin = min(kmin, ((uint32_t)(val + 32768) << 10) | o);
    kmax = min(kmax, ((uint32_t)(32767 - val) << 10) | o);
  }
  kmin = wave_min_u32(kmin);
  kmax = wave_min_u32(kmax);
  const int mnv = (int)(kmin >> 10) - 32768, mno = kmin & 1023;
  const int mxv = 32767 - (int)(kmax >> 10), mxo = kmax & 1023;
  const int mni = i + mno / n1, mnj = j + mno % n1, mxi = i + mxo / n1, mxj = j + mxo % n1;
  bool vmin = mnv <= -tau, vmax = mxv >= tau;  // wave-uniform
  if (vmin) vmin = !nms_suppressed_wave(f, d.mbpl, d.mw, d.mh, n, i, j, mni, mnj, mnv, true, lane);
  if (vmax) vmax = !nms_suppressed_wave(f, d.mbpl, d.mw, d.mh, n, i, j, mxi, mxj, mxv, false, lane);
  if (lane == 0) {
    int32_t *c = st.cand + (size_t)(ci * st.ncv + cj) * 4 + 2 * k;
    c[0] = vmin ? (int32_t)(0x80000000u | (uint32_t)mni | ((uint32_t)mnj << 14)) : 0;
    c[1] = vmax ? (int32_t)(0x80000000u | (uint32_t)mxi | ((uint32_t)mxj << 14)) : 0;
  }
}

// Tile variant for small n (the dense set, n = nms_n <= 4): a 256-thread block stages the f1/f2
// responses of 16 x 8 cells plus the n-pixel halo in LDS (coalesced row reads, 11 KB at n = 3) and
// every thread then resolves one (cell, filter) entirely from LDS -- (n+1)^2 + 2 (2n+1)^2 reads --
// instead of spending a whole wavefront per cell.  Same scan order, same strict compares.
#define NMS_TCU 16
#define NMS_TCV 8
#define NMS_TILE_MAXN 4
__global__ void __launch_bounds__(256)
    k_nms_tile(const VsmImage *__restrict__ imgs, int first, VsmDims d, const int16_t *__restrict__ f1base,
               const int16_t *__restrict__ f2base, size_t f_stride, int tau, int si, int nbx, int n_img) {
  constexpr int MAXW = NMS_TCU * (NMS_TILE_MAXN + 1) + 2 * NMS_TILE_MAXN;  // 88
  constexpr int MAXH = NMS_TCV * (NMS_TILE_MAXN + 1) + 2 * NMS_TILE_MAXN;  // 48
  __shared__ int16_t s_f[2][MAXH][MAXW + 2];
  const int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int zi = lb / nbx, bx = lb - zi * nbx;  // (image, tile)
  if (zi >= n_img) return;
  const VsmSet &st = imgs[first + zi].set[si];
  const int n = st.nms_n, n1 = n + 1;
  const int tiles_u = (st.ncu + NMS_TCU - 1) / NMS_TCU;
  const int tu = bx % tiles_u, tv = bx / tiles_u;
  const int cu0 = tu * NMS_TCU, cv0 = tv * NMS_TCV;
  const int u0 = VSM_MARGIN + cu0 * n1, v0 = VSM_MARGIN + cv0 * n1;  // = first cell origin - n
  const int tw = NMS_TCU * n1 + 2 * n, th = NMS_TCV * n1 + 2 * n;
  const int16_t *__restrict__ f1 = f1base + (size_t)zi * f_stride;
  const int16_t *__restrict__ f2 = f2base + (size_t)zi * f_stride;
  for (int e = threadIdx.x; e < tw * th; e += 256) {
    const int y = e / tw, x = e - y * tw;
    const int u = u0 + x, v = v0 + y;
    const bool in = u < d.mbpl && v < d.mh;
    s_f[0][y][x] = in ? f1[v * d.mbpl + u] : (int16_t)0;
    s_f[1][y][x] = in ? f2[v * d.mbpl + u] : (int16_t)0;
  }
  __syncthreads();
  const int k = threadIdx.x & 1, cl = threadIdx.x >> 1;
  const int lcu = cl % NMS_TCU, lcv = cl / NMS_TCU;
  const int ci = cu0 + lcu, cj = cv0 + lcv;
  if (ci >= st.ncu || cj >= st.ncv) return;
  const int16_t(*f)[MAXW + 2] = s_f[k];
  // tile-local coordinates of the cell origin; image coordinates = local + (u0, v0)
  const int li = n + lcu * n1, lj = n + lcv * n1;
  int mni = li, mnj = lj, mxi = li, mxj = lj;
  int mnv = f[lj][li], mxv = mnv;
  for (int i2 = li; i2 <= li + n; i2++)
    for (int j2 = lj; j2 <= lj + n; j2++) {
      const int cur = f[j2][i2];
      if (cur < mnv) {
        mni = i2;
        mnj = j2;
        mnv = cur;
      } else if (cur > mxv) {
        mxi = i2;
        mxj = j2;
        mxv = cur;
      }
    }
  // clip limits of the suppression windows (w-1-margin, h-1-margin) in tile-local coordinates
  const int lim_i = d.mw - 1 - VSM_MARGIN - u0, lim_j = d.mh - 1 - VSM_MARGIN - v0;
  auto suppressed = [&](int ci2, int cj2, int val, bool want_min) -> bool {
    const int i_hi = min(ci2 + n, lim_i), j_hi = min(cj2 + n, lim_j);
    for (int i2 = ci2 - n; i2 <= i_hi; i2++)
      for (int j2 = cj2 - n; j2 <= j_hi; j2++) {
        const int cur = f[j2][i2];
        const bool better = want_min ? (cur < val) : (cur > val);
        if (better && (i2 < li || i2 > li + n || j2 < lj || j2 > lj + n)) return true;
      }
    return false;
  };
  const bool vmin = (mnv <= -tau) && !suppressed(mni, mnj, mnv, true);
  const bool vmax = (mxv >= tau) && !suppressed(mxi, mxj, mxv, false);
  int32_t *c = st.cand + (size_t)(ci * st.ncv + cj) * 4 + 2 * k;
  c[0] = vmin ? (int32_t)(0x80000000u | (uint32_t)(mni + u0) | ((uint32_t)(mnj + v0) << 14)) : 0;
  c[1] = vmax ? (int32_t)(0x80000000u | (uint32_t)(mxi + u0) | ((uint32_t)(mxj + v0) << 14)) : 0;
}

// Tile variant for mid-size n (the sparse set, 5 <= n <= 10): 4 x 4 cells + halo in LDS, 8 lanes
// per (cell, filter): the lanes stride over the cell / window pixels and combine with width-8
// shuffles (min of (value, scan position) keys, OR of the suppression hits).
#define NMS8_TC 4
#define NMS8_MAXN 10
__global__ void __launch_bounds__(256)
    k_nms_tile8(const VsmImage *__restrict__ imgs, int first, VsmDims d, const int16_t *__restrict__ f1base,
                const int16_t *__restrict__ f2base, size_t f_stride, int tau, int si, int nbx, int n_img) {
  constexpr int MAXD = NMS8_TC * (NMS8_MAXN + 1) + 2 * NMS8_MAXN;  // 64
  __shared__ int16_t s_f[2][MAXD][MAXD + 2];
  const int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int zi = lb / nbx, bx = lb - zi * nbx;  // (image, tile)
  if (zi >= n_img) return;
  const VsmSet &st = imgs[first + zi].set[si];
  const int n = st.nms_n, n1 = n + 1;
  const int tiles_u = (st.ncu + NMS8_TC - 1) / NMS8_TC;
  const int tu = bx % tiles_u, tv = bx / tiles_u;
  const int cu0 = tu * NMS8_TC, cv0 = tv * NMS8_TC;
  const int u0 = VSM_MARGIN + cu0 * n1, v0 = VSM_MARGIN + cv0 * n1;
  const int tw = NMS8_TC * n1 + 2 * n;
  const int16_t *__restrict__ f1 = f1base + (size_t)zi * f_stride;
  const int16_t *__restrict__ f2 = f2base + (size_t)zi * f_stride;
  for (int e = threadIdx.x; e < tw * tw; e += 256) {
    const int y = e / tw, x = e - y * tw;
    const int u = u0 + x, v = v0 + y;
    const bool in = u < d.mbpl && v < d.mh;
    s_f[0][y][x] = in ? f1[v * d.mbpl + u] : (int16_t)0;
    s_f[1][y][x] = in ? f2[v * d.mbpl + u] : (int16_t)0;
  }
  __syncthreads();
  const int l8 = threadIdx.x & 7, item = threadIdx.x >> 3;  // 32 items: 16 cells x 2 filters
  const int k = item & 1, cl = item >> 1;
  const int lcu = cl % NMS8_TC, lcv = cl / NMS8_TC;
  const int ci = cu0 + lcu, cj = cv0 + lcv;
  const bool live = ci < st.ncu && cj < st.ncv;  // dead items still take part in the shuffles
  const int16_t(*f)[MAXD + 2] = s_f[k];
  const int li = n + lcu * n1, lj = n + lcv * n1;
  uint32_t kmin = 0xffffffffu, kmax = 0xffffffffu;
  for (int e = l8; e < n1 * n1; e += 8) {
    const int dj = e / n1, di = e - dj * n1;
    const int val = f[lj + dj][li + di];
    const uint32_t o = (uint32_t)(di * n1 + dj);
    kmin = min(kmin, ((uint32_t)(val + 32768) << 10) | o);
    kmax = min(kmax, ((uint32_t)(32767 - val) << 10) | o);
  }
#pragma unroll
  for (int o = 4; o >= 1; o >>= 1) {
    kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, o, 8));
    kmax = min(kmax, (uint32_t)__shfl_xor((int)kmax, o, 8));
  }
  const int mnv = (int)(kmin >> 10) - 32768, mno = kmin & 1023;
  const int mxv = 32767 - (int)(kmax >> 10), mxo = kmax & 1023;
  const int mni = li + mno / n1, mnj = lj + mno % n1, mxi = li + mxo / n1, mxj = lj + mxo % n1;
  const int lim_i = d.mw - 1 - VSM_MARGIN - u0, lim_j = d.mh - 1 - VSM_MARGIN - v0;
  const int W = 2 * n + 1;
  auto suppressed = [&](int ci2, int cj2, int val, bool want_min) -> bool {
    const int i_hi = min(ci2 + n, lim_i), j_hi = min(cj2 + n, lim_j);
    int hit = 0;
    for (int e = l8; e < W * W; e += 8) {
      const int dj = e / W, di = e - dj * W;
      const int i2 = ci2 - n + di, j2 = cj2 - n + dj;
      if (i2 <= i_hi && j2 <= j_hi) {
        const int cur = f[j2][i2];
        const bool better = want_min ? (cur < val) : (cur > val);
        hit |= (better && (i2 < li || i2 > li + n || j2 < lj || j2 > lj + n)) ? 1 : 0;
      }
    }
#pragma unroll
    for (int o = 4; o >= 1; o >>= 1) hit |= __shfl_xor(hit, o, 8);
    return hit != 0;
  };
  // both tests run unconditionally so that all 8 lanes of every item reach the shuffles together
  const bool smin = suppressed(mni, mnj, mnv, true);
  const bool smax = suppressed(mxi, mxj, mxv, false);
  if (live && l8 == 0) {
    const bool vmin = (mnv <= -tau) && !smin, vmax = (mxv >= tau) && !smax;
    int32_t *c = st.cand + (size_t)(ci * st.ncv + cj) * 4 + 2 * k;
    c[0] = vmin ? (int32_t)(0x80000000u | (uint32_t)(mni + u0) | ((uint32_t)(mnj + v0) << 14)) : 0;
    c[1] = vmax ? (int32_t)(0x80000000u | (uint32_t)(mxi + u0) | ((uint32_t)(mxj + v0) << 14)) : 0;
  }
}

// Fixed-radius variants for the two radii the default parameters produce (dense n = 3, sparse n = 9;
// viso/matcher.cpp:685-687): same LDS tiling as above, but with n a compile-time constant every
// LDS read of the cell scan and of the (2n+1)^2 suppression window has an immediate offset from one
// per-thread base address, and the window test is branch-free: a candidate is the extremum of its
// own cell, so "no strictly better value in the window outside the cell" (:383-428) is simply
// "the window extremum equals the candidate's value".  Tiles that touch the right/bottom clip limit
// (w-1-margin, h-1-margin) take a bounded loop instead.  N = 3: one thread per (cell, filter);
// N = 9: 8 lanes per (cell, filter), each owning window rows l8, l8+8, l8+16.
template <int N, int TCU, int TCV, int LANES>
__global__ void __launch_bounds__(256)
    k_nms_fixed(const VsmImage *__restrict__ imgs, int first, VsmDims d, const int16_t *__restrict__ f1base,
                const int16_t *__restrict__ f2base, size_t f_stride, int tau, int si, int nbx, int n_img) {
  constexpr int N1 = N + 1, W = 2 * N + 1;
  constexpr int TW = TCU * N1 + 2 * N, TH = TCV * N1 + 2 * N;
  constexpr int STR = (((TW + 1) / 2) | 1) * 2;  // int16 per LDS row: an odd number of dwords
  static_assert(TCU * TCV * 2 * LANES == 256, "one item per LANES threads");
  static_assert((N1 & 1) == 0, "tile origins must stay dword aligned");
  __shared__ int16_t s_f[2][TH][STR];
  const int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int zi = lb / nbx, bx = lb - zi * nbx;  // (image, tile)
  if (zi >= n_img) return;
  const VsmSet &st = imgs[first + zi].set[si];
  const int tiles_u = (st.ncu + TCU - 1) / TCU;
  const int tu = bx % tiles_u, tv = bx / tiles_u;
  const int cu0 = tu * TCU, cv0 = tv * TCV;
  const int u0 = VSM_MARGIN + cu0 * N1, v0 = VSM_MARGIN + cv0 * N1;  // = first cell origin - N (even)
  const int16_t *__restrict__ f1 = f1base + (size_t)zi * f_stride;
  const int16_t *__restrict__ f2 = f2base + (size_t)zi * f_stride;
  for (int e = threadIdx.x; e < (TW / 2) * TH; e += 256) {  // two pixels per load
    const int y = e / (TW / 2), x = 2 * (e - y * (TW / 2));
    const int u = u0 + x, v = v0 + y;
    const bool in = u + 1 < d.mbpl && v < d.mh;
    const uint32_t a = in ? *(const uint32_t *)(f1 + v * d.mbpl + u) : 0u;
    const uint32_t b = in ? *(const uint32_t *)(f2 + v * d.mbpl + u) : 0u;
    *(uint32_t *)&s_f[0][y][x] = a;
    *(uint32_t *)&s_f[1][y][x] = b;
  }
  __syncthreads();
  const int l8 = threadIdx.x % LANES, item = threadIdx.x / LANES;
  const int k = item & 1, cl = item >> 1;
  const int lcu = cl % TCU, lcv = cl / TCU;
  const int ci = cu0 + lcu, cj = cv0 + lcv;
  const bool live = ci < st.ncu && cj < st.ncv;  // dead items still take part in the shuffles
  const int16_t(*f)[STR] = s_f[k];
  const int li = N + lcu * N1, lj = N + lcv * N1;  // tile-local cell origin
  // first-wins extrema of the cell in the reference's scan order (u outer, v inner, strict compare,
  // :356-380): minimum of the key (value, scan position)
  uint32_t kmin = 0xffffffffu, kmax = 0xffffffffu;
  {
    const int16_t *c0 = &f[lj][li];
#pragma unroll
    for (int t = 0; t < (N1 + LANES - 1) / LANES; t++) {
      const int di = l8 + t * LANES;  // this lane's column(s) of the cell
      if (di < N1) {
#pragma unroll
        for (int dj = 0; dj < N1; dj++) {
          const int val = c0[dj * STR + di];
          const uint32_t o = (uint32_t)(di * N1 + dj);
          kmin = min(kmin, ((uint32_t)(val + 32768) << 10) | o);
          kmax = min(kmax, ((uint32_t)(32767 - val) << 10) | o);
        }
      }
    }
  }
#pragma unroll
  for (int o = LANES / 2; o >= 1; o >>= 1) {
    kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, o, LANES));
    kmax = min(kmax, (uint32_t)__shfl_xor((int)kmax, o, LANES));
  }
  const int mnv = (int)(kmin >> 10) - 32768, mno = kmin & 1023;
  const int mxv = 32767 - (int)(kmax >> 10), mxo = kmax & 1023;
  const int mni = li + mno / N1, mnj = lj + mno % N1, mxi = li + mxo / N1, mxj = lj + mxo % N1;
  const int lim_i = d.mw - 1 - VSM_MARGIN - u0, lim_j = d.mh - 1 - VSM_MARGIN - v0;
  int wmn = 32767, wmx = -32768;  // extrema over this lane's share of the two windows
  if (lim_i >= TW - 1 && lim_j >= TH - 1) {  // block-uniform: no window of this tile is clipped
    // A window row is W = 2N+1 values from column mi-N on: (W+1)/2 aligned dwords cover it whatever the parity of that
    // column, with one value too many - the last one (even start) or the first (odd start) - which is replaced by the
    // neutral element; then two values per v_pk_min_i16 / v_pk_max_i16.  (Half the LDS reads of the value-by-value walk:
    // the kernels spend most of their time here.)
    typedef short vsm_s2 __attribute__((ext_vector_type(2)));
    constexpr int ND = (W + 1) / 2;
    const int cn = mni - N, cx = mxi - N;
    const bool pn1 = (cn & 1) != 0, px1 = (cx & 1) != 0;
    const uint32_t *pn = (const uint32_t *)&f[mnj - N][cn & ~1], *px = (const uint32_t *)&f[mxj - N][cx & ~1];
    vsm_s2 amn = {32767, 32767}, amx = {-32768, -32768};
#pragma unroll
    for (int t = 0; t < (W + LANES - 1) / LANES; t++) {
      const int r = l8 + t * LANES;
      if (r < W) {
        const uint32_t *rn = pn + r * (STR / 2), *rx = px + r * (STR / 2);
#pragma unroll
        for (int c = 0; c < ND; c++) {
          uint32_t vn = rn[c], vx = rx[c];
          if (c == 0) {
            vn = pn1 ? ((vn & 0xffff0000u) | 0x00007fffu) : vn;
            vx = px1 ? ((vx & 0xffff0000u) | 0x00008000u) : vx;
          }
          if (c == ND - 1) {
            vn = pn1 ? vn : ((vn & 0x0000ffffu) | 0x7fff0000u);
            vx = px1 ? vx : ((vx & 0x0000ffffu) | 0x80000000u);
          }
          amn = __builtin_elementwise_min(amn, __builtin_bit_cast(vsm_s2, vn));
          amx = __builtin_elementwise_max(amx, __builtin_bit_cast(vsm_s2, vx));
        }
      }
    }
    wmn = min((int)amn.x, (int)amn.y);
    wmx = max((int)amx.x, (int)amx.y);
  } else {
    for (int r = l8; r < W; r += LANES) {
      if (mnj - N + r <= lim_j)
        for (int c = 0; c < W && mni - N + c <= lim_i; c++) wmn = min(wmn, (int)f[mnj - N + r][mni - N + c]);
      if (mxj - N + r <= lim_j)
        for (int c = 0; c < W && mxi - N + c <= lim_i; c++) wmx = max(wmx, (int)f[mxj - N + r][mxi - N + c]);
    }
  }
#pragma unroll
  for (int o = LANES / 2; o >= 1; o >>= 1) {
    wmn = min(wmn, __shfl_xor(wmn, o, LANES));
    wmx = max(wmx, __shfl_xor(wmx, o, LANES));
  }
  if (live && l8 == 0) {
    const bool vmin = (mnv <= -tau) && wmn >= mnv, vmax = (mxv >= tau) && wmx <= mxv;
    int32_t *c = st.cand + (size_t)(ci * st.ncv + cj) * 4 + 2 * k;
    c[0] = vmin ? (int32_t)(0x80000000u | (uint32_t)(mni + u0) | ((uint32_t)(mnj + v0) << 14)) : 0;
    c[1] = vmax ? (int32_t)(0x80000000u | (uint32_t)(mxi + u0) | ((uint32_t)(mxj + v0) << 14)) : 0;
  }
}

// ---------------------------------------------------------------------------------------
// The fused matching-resolution image side for the default suppression radii (dense n = 3, sparse n = 9): F1-F3 + N1 out of
// one LDS tile per workgroup, f1 / f2 never in HBM.  All per-thread work is in vsm_feat.h (shared with the CPU emulation
// of the "not gpu" tests); here: the phases.
//   k_feat_dense   tile = 128 x 48 owned pixels: image tile (+ 8 / 6 pixels of halo) -> LDS, 17 x 14 patches of 8 x 4 pixels,
//                  one per thread: du / dv (HBM), f1 / f2 (LDS), then 32 x 12 cells x 2 filters, a thread each
//   k_feat_sparse  tile = 16 x 4 cells of 10 x 10 pixels: the 19 x 19 windows want 11 pixels of halo, so this scale gets its
//                  own coarser tile and recomputes f1 / f2 (12 of 26 operations per pixel) rather than doubling the dense
//                  tile's filter work: 23 x 10 patches of 8 x 6 pixels; one response plane in LDS at a time (34 KB: four
//                  workgroups per compute unit), f2 waits in registers; 8 lanes per (cell, filter)
// XCD-aware placement: neighbouring tiles (which share halo lines) follow each other on one XCD's L2.
// ---------------------------------------------------------------------------------------


template <bool DUMP>
__global__ void __launch_bounds__(256)
    k_feat_dense(const VsmImage *__restrict__ imgs, int first, VsmDims d, int tau, int tiles_x, int nbx, int n_img,
                 int16_t *__restrict__ f1base, int16_t *__restrict__ f2base, size_t f_stride) {
  typedef VfDense G;
  __shared__ __attribute__((aligned(16))) uint32_t s_img[G::IH * G::IWD];
  __shared__ __attribute__((aligned(16))) int16_t s_f[2 * G::FH * G::FS];
  const int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int zi = lb / nbx, bx = lb - zi * nbx;
  if (zi >= n_img) return;
  const VsmImage &im = imgs[first + zi];
  const VsmSet &st = im.set[1];
  const int ty = bx / tiles_x, tx = bx - ty * tiles_x;
  const int t = threadIdx.x;
  FT_DECL;
  FT_STAMP;
  vf_fill<G, 256>(s_img, im.imgm, d.mbpl * d.mh, d.mbpl, tx, ty, t);
  FT_STAMP;
  __syncthreads();
  FT_STAMP;
  if (t < G::PC * G::PR)
    vf_dense_patch(s_img, s_f, t, tx, ty, d.mbpl, d.mh, im.du, im.dv, DUMP ? f1base + (size_t)zi * f_stride : nullptr,
                   DUMP ? f2base + (size_t)zi * f_stride : nullptr);
  FT_STAMP;
  __syncthreads();
  FT_STAMP;
  for (int it = t; it < G::CU * G::CV * 2; it += 256) vf_dense_nms(s_f, it, tx, ty, d.mw, d.mh, VSM_MARGIN, tau, st.ncu, st.ncv, st.cand);
  FT_STAMP;
  FT_FLUSH(0);
}

__global__ void __launch_bounds__(256)
    k_feat_sparse(const VsmImage *__restrict__ imgs, int first, VsmDims d, int tau, int tiles_x, int nbx, int n_img) {
  typedef VfSparse G;
  __shared__ __attribute__((aligned(16))) uint32_t s_img[G::IH * G::IWD];
  __shared__ __attribute__((aligned(16))) int16_t s_f[G::FH * G::FS];
  const int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int zi = lb / nbx, bx = lb - zi * nbx;
  if (zi >= n_img) return;
  const VsmImage &im = imgs[first + zi];
  const VsmSet &st = im.set[0];
  const int ty = bx / tiles_x, tx = bx - ty * tiles_x;
  const int t = threadIdx.x;
  FT_DECL;
  FT_STAMP;
  vf_fill<G, 256>(s_img, im.imgm, d.mbpl * d.mh, d.mbpl, tx, ty, t);
  FT_STAMP;
  __syncthreads();
  FT_STAMP;
  VfSparseKeep keep;
  if (t < G::PC * G::PR) vf_sparse_patch(s_img, s_f, t, keep);
  FT_STAMP;
  __syncthreads();
  FT_STAMP;
  static_assert((G::CU * G::CV) % 32 == 0, "whole rounds of 32 items x 8 lanes");
  for (int it = t >> 3; it < G::CU * G::CV; it += 32) vf_sparse_nms<8>(s_f, it, t & 7, 0, tx, ty, d.mw, d.mh, VSM_MARGIN, tau, st.ncu, st.ncv, st.cand);
  FT_STAMP;
  __syncthreads();
  if (t < G::PC * G::PR) vf_sparse_store_f2(s_f, t, keep);
  __syncthreads();
  FT_STAMP;
  for (int it = t >> 3; it < G::CU * G::CV; it += 32) vf_sparse_nms<8>(s_f, it, t & 7, 1, tx, ty, d.mw, d.mh, VSM_MARGIN, tau, st.ncu, st.ncv, st.cand);
  FT_STAMP;
  FT_FLUSH(1);
}

// tiles per image of the two kernels (the CPU emulation mirrors this: tests/emu/feat_emu.cpp)
static void vsm_feat_tiles(const VsmDims &d, const VsmSet &dense, int &dx, int &dy) {
  dx = std::max((d.mbpl + 8 + 127) / 128, (dense.ncu + 3 + 31) / 32);
  dy = std::max((d.mh + 4 + 47) / 48, (dense.ncv + 2 + 11) / 12);
}

// ---------------------------------------------------------------------------------------
// Feature index = rank in the reference's emission order (cells u-major / v-minor, classes
// f1min,f1max,f2min,f2max inside a cell, viso/matcher.cpp:344-430): exclusive prefix sum of the
// per-cell survivor counts.  One 1024-thread block per (image, set); every thread owns a run of
// consecutive cells.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) k_scan_cells(const VsmImage *__restrict__ imgs, int first, int set_lo, int nb) {
  __shared__ int s_w[17];
  const VsmSet &st = imgs[first + blockIdx.z].set[blockIdx.y];
  if ((int)blockIdx.y < set_lo) {
    if (threadIdx.x == 0) {
      *st.count = 0;
      *st.count_host = 0;
    }
    return;
  }
  for (int b = threadIdx.x; b < nb; b += 1024) st.bin_cnt[b] = 0;  // histogram filled by k_emit
  const int ncells = st.ncu * st.ncv;
  const int chunk = (ncells + 1023) / 1024;
  const int c0 = min((int)threadIdx.x * chunk, ncells), c1 = min(c0 + chunk, ncells);
  int sum = 0, total, run;
  if (chunk <= 8) {  // (the usual case: all of a thread's cells requested at once, their counts kept for the second sweep)
    int cnt[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      cnt[k] = 0;
      if (c0 + k < c1) {
        const int4 v = ldg_i4(st.cand + (size_t)(c0 + k) * 4);
        cnt[k] = (v.x < 0) + (v.y < 0) + (v.z < 0) + (v.w < 0);
      }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) sum += cnt[k];
    run = block_excl_scan_1024(sum, total, s_w);
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (c0 + k < c1) {
        st.cell_off[c0 + k] = run;
        run += cnt[k];
      }
  } else {
    for (int c = c0; c < c1; c++) {
      const int4 v = *(const int4 *)(st.cand + (size_t)c * 4);
      sum += (v.x < 0) + (v.y < 0) + (v.z < 0) + (v.w < 0);
    }
    run = block_excl_scan_1024(sum, total, s_w);
    for (int c = c0; c < c1; c++) {
      const int4 v = *(const int4 *)(st.cand + (size_t)c * 4);
      st.cell_off[c] = run;
      run += (v.x < 0) + (v.y < 0) + (v.z < 0) + (v.w < 0);
    }
  }
  if (threadIdx.x == 0) {
    st.cell_off[ncells] = total;
    *st.count = total;
    *st.count_host = total;
  }
}

// ---------------------------------------------------------------------------------------
// T1 feature records (viso/matcher.cpp:707-731) + D1 descriptor gather (computeDescriptor,
// viso/matcher.cpp:433-477).  16 lanes per cell: lane j < 12 produces dword j of the 48-byte
// record {u*s, v*s, 0, class, d1..d8} of each survivor of the cell -- a descriptor dword is two
// taps x (du,dv) = 4 byte gathers -- so every record leaves as one coalesced 48-byte run.
// ---------------------------------------------------------------------------------------
__constant__ int8_t c_desc_dv[16] = {-1, +1, -1, +1, -1, +1, -1, +1, -5, +5, -5, +5, -3, +3, -3, +3};
__constant__ int8_t c_desc_du[16] = {-3, -3, -1, -1, +3, +3, +1, +1, -1, -1, +1, +1, -5, -5, +5, +5};

// Tile kernel: a block owns a rectangle of NMS cells (up to 128 x 32 matching-resolution pixels).
// It first stages the Sobel responses of that rectangle plus the 5-pixel descriptor halo in LDS,
// du and dv interleaved per pixel (coalesced dword row reads of both planes), then one thread per
// cell writes the records of the cell's survivors: the 16 taps of computeDescriptor are 16-bit LDS
// reads at compile-time offsets, already in the byte order of the record (du,dv of tap 0, du,dv of
// tap 1, ...; viso/matcher.cpp:445-476), and the 48 bytes leave as three 16-byte stores.
#define EMIT_TW 128
#define EMIT_TH 32
#define EMIT_HALO 5
#define EMIT_LW (EMIT_TW + 2 * EMIT_HALO + 4)  // + alignment slack of the row reads: 142 pixels
#define EMIT_LH (EMIT_TH + 2 * EMIT_HALO)
__global__ void __launch_bounds__(256) k_emit(const VsmImage *__restrict__ imgs, int first, VsmDims d, int set_lo,
                                              int binsize, int nbx, int n_img) {
  __shared__ uint16_t s_g[EMIT_LH][EMIT_LW + 2];  // du | dv << 8
  const int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int zi = lb / nbx, bx = lb - zi * nbx;
  if (zi >= n_img) return;
  const VsmImage &im = imgs[first + zi];
  const int si = blockIdx.y;
  if (si < set_lo) return;
  const VsmSet &st = im.set[si];
  const int n1 = st.nms_n + 1;
  const int tcu = max(EMIT_TW / n1, 1), tcv = max(EMIT_TH / n1, 1);  // cells per tile
  const int tiles_u = (st.ncu + tcu - 1) / tcu, tiles_v = (st.ncv + tcv - 1) / tcv;
  if (bx >= tiles_u * tiles_v) return;
  const int tu = bx % tiles_u, tv = bx / tiles_u;
  const int cu0 = tu * tcu, cv0 = tv * tcv;
  // pixel rectangle covered by the descriptors of this tile's cells; cells wider than the tile
  // (n > 31) cannot be staged and take the direct path below
  const int ut = st.nms_n + VSM_MARGIN + cu0 * n1 - EMIT_HALO, vt = st.nms_n + VSM_MARGIN + cv0 * n1 - EMIT_HALO;
  const int ua = ut & ~3;
  const bool staged = n1 <= EMIT_TH;
  if (staged) {
    for (int e = threadIdx.x; e < (EMIT_LW / 4 + 1) * EMIT_LH; e += 256) {
      const int y = e / (EMIT_LW / 4 + 1), x = 4 * (e - y * (EMIT_LW / 4 + 1));
      const int u = ua + x, v = vt + y;
      if (x + 3 < EMIT_LW + 2) {
        uint32_t a = 0, b = 0;
        if (u >= 0 && u + 3 < d.mbpl && v >= 0 && v < d.mh) {
          a = ldg_u32(im.du + (size_t)v * d.mbpl + u);
          b = ldg_u32(im.dv + (size_t)v * d.mbpl + u);
        }
        // interleave: pixel p -> du_p | dv_p << 8
        const uint32_t lo = (a & 0xffu) | ((b & 0xffu) << 8) | ((a & 0xff00u) << 8) | ((b & 0xff00u) << 16);
        const uint32_t hi = ((a >> 16) & 0xffu) | (((b >> 16) & 0xffu) << 8) | ((a >> 24) << 16) | ((b >> 24) << 24);
        *(uint2 *)&s_g[y][x] = make_uint2(lo, hi);
      }
    }
    __syncthreads();
  }
  for (int t = threadIdx.x; t < tcu * tcv; t += 256) {
    const int lcv = t % tcv, lcu = t / tcv;  // v fastest: neighbouring threads own neighbouring cand[] entries
    const int ci = cu0 + lcu, cj = cv0 + lcv;
    if (ci >= st.ncu || cj >= st.ncv) continue;
    const int cell = ci * st.ncv + cj;
    const int4 c4 = ldg_i4(st.cand + (size_t)cell * 4);
    if ((c4.x | c4.y | c4.z | c4.w) >= 0) continue;
    const int cc4[4] = {c4.x, c4.y, c4.z, c4.w};
    int pos = ldg_i32(st.cell_off + cell);
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const int cc = cc4[g];
      if (cc >= 0) continue;
      const int u = cc & 0x3fff, v = (cc >> 14) & 0x3fff;
      uint32_t t16[16];
      if (staged) {
        const uint16_t *c0 = &s_g[v - vt][u - ua];
#pragma unroll
        for (int m = 0; m < 16; m++) {
          constexpr int8_t kdv[16] = {-1, +1, -1, +1, -1, +1, -1, +1, -5, +5, -5, +5, -3, +3, -3, +3};
          constexpr int8_t kdu[16] = {-3, -3, -1, -1, +3, +3, +1, +1, -1, -1, +1, +1, -5, -5, +5, +5};
          t16[m] = c0[kdv[m] * (EMIT_LW + 2) + kdu[m]];
        }
      } else {
#pragma unroll
        for (int m = 0; m < 16; m++) {
          const int a = (v + c_desc_dv[m]) * d.mbpl + u + c_desc_du[m];
          t16[m] = (uint32_t)im.du[a] | ((uint32_t)im.dv[a] << 8);
        }
      }
      vsm_u4 r0, r1, r2;
      r0.x = (uint32_t)(u * d.scale);
      r0.y = (uint32_t)(v * d.scale);
      r0.z = 0u;
      r0.w = (uint32_t)g;
      r1.x = t16[0] | (t16[1] << 16);
      r1.y = t16[2] | (t16[3] << 16);
      r1.z = t16[4] | (t16[5] << 16);
      r1.w = t16[6] | (t16[7] << 16);
      r2.x = t16[8] | (t16[9] << 16);
      r2.y = t16[10] | (t16[11] << 16);
      r2.z = t16[12] | (t16[13] << 16);
      r2.w = t16[14] | (t16[15] << 16);
      VSM_AS1 vsm_u4 *rec = (VSM_AS1 vsm_u4 *)(st.feat + (size_t)pos * 12);
      rec[0] = r0;
      rec[1] = r1;
      rec[2] = r2;
      // M1 createIndexVector (viso/matcher.cpp:870-890): histogram of the search bins
      const int b = bin_of(u * d.scale, v * d.scale, g, binsize, d.ub, d.vb);
      st.binid[pos] = b;
      atomicAdd(&st.bin_cnt[b], 1);
      pos++;
    }
  }
}

// ---------------------------------------------------------------------------------------
// T1 + D1 + M1 in two kernels (the default path; k_scan_cells / k_emit / k_bin_* above and below remain for geometries it
// declines):
//   k_feat_scan   one workgroup per (image, set): ONE pass over the survivors gives the exclusive prefix of the cells'
//                 survivor counts (feature index = rank in the reference's emission order, viso/matcher.cpp:344-430) and,
//                 through a histogram in LDS, the start of every fine search bin (createIndexVector, :870-890)
//   k_feat_order  a workgroup owns a TILE OF WHOLE SEARCH BINS (bu coarse u-bins x one v-bin) of one image, both sets: it
//                 stages the Sobel responses of the tile's rectangle + the 5-pixel descriptor halo in LDS once, collects the
//                 survivors that fall into its bins from the cells overlapping the rectangle, and - because every feature
//                 of a bin is then in the workgroup - ranks them inside their fine bin and inside the reference's bin by
//                 counting smaller feature indices in a short LDS list per (bin, class).  Each survivor's 48-byte record
//                 goes to feat[index] and, in the same breath, its coordinates / descriptor / index / reference rank to
//                 their place in the bin-sorted arrays: no bin ids, scatter cursors or unordered slots in HBM, no second
//                 read of the records (k_bin_rank gathered them back: 2.5 x its algorithmic bytes).
// ---------------------------------------------------------------------------------------
// division by the search bin size as a multiply-high (exact for 0 <= x < 2^32 / binsize; the arguments are image coordinates)
struct VsmBinDiv {
  int32_t binsize;
  uint32_t magic;  // ceil(2^32 / binsize), 0 for binsize 1
  __device__ __forceinline__ int div(int x) const { return binsize == 1 ? x : (int)__umulhi((uint32_t)x, magic); }
  __device__ __forceinline__ int vsub(int v, int vbin) const { return min(div((v - vbin * binsize) * VSM_VSUB), VSM_VSUB - 1); }  // sub-row inside the bin
};
struct VsmOrderPlan {
  int32_t bu;                  // coarse u-bins per tile
  int32_t tiles_u, tiles_v;    // tiles per image (tiles_v = v-bins)
  int32_t stage_w, stage_h;    // staged Sobel responses: uint16 (du | dv << 8) per pixel
  int32_t cells_cap[2];        // cells of a set that can overlap a tile's rectangle
  int32_t cells_max;           // the larger of the two
  int32_t lcap[2];             // entries a (bin, class) list can take
  int32_t o_cand, o_bs, o_cnt, o_list, o_sv, lds_bytes;  // LDS layout (bytes)
};

__device__ __forceinline__ int ceil_div_pos(int a, int b) { return (a + b - 1) / b; }

__global__ void __launch_bounds__(1024) k_feat_scan(const VsmImage *__restrict__ imgs, int first, int set_lo, VsmDims d, VsmBinDiv bd, int nb) {
  extern __shared__ int s_dyn[];
  __shared__ int s_w[17];
  int *s_hist = s_dyn;
  const VsmSet &st = imgs[first + blockIdx.z].set[blockIdx.y];
  if ((int)blockIdx.y < set_lo) {
    if (threadIdx.x == 0) {
      *st.count = 0;
      *st.count_host = 0;
    }
    return;
  }
  FT_DECL;
  FT_STAMP;
  for (int b = threadIdx.x; b < nb; b += 1024) s_hist[b] = 0;
  __syncthreads();
  FT_STAMP;
  const int ncells = st.ncu * st.ncv;
  const int chunk = (ncells + 1023) / 1024;
  const int c0 = min((int)threadIdx.x * chunk, ncells), c1 = min(c0 + chunk, ncells);
  int sum = 0, total, run;
  auto tally = [&](const int4 &v) -> int {  // survivors of a cell into the histogram; returns their number
    const int cc[4] = {v.x, v.y, v.z, v.w};
    int n = 0;
#pragma unroll
    for (int g = 0; g < 4; g++)
      if (cc[g] < 0) {
        n++;
        const int u = (cc[g] & 0x3fff) * d.scale, v = ((cc[g] >> 14) & 0x3fff) * d.scale;
        const int ubin = min(bd.div(u), d.ub - 1), vbin = min(bd.div(v), d.vb - 1);
        atomicAdd(&s_hist[(g * d.ub + ubin) * (d.vb * VSM_VSUB) + vbin * VSM_VSUB + bd.vsub(v, vbin)], 1);  // = bin_of()
      }
    return n;
  };
  if (chunk <= 8) {  // (the usual case: all of a thread's cells requested at once, their counts kept for the second sweep)
    int4 v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = (c0 + k < c1) ? ldg_i4(st.cand + (size_t)(c0 + k) * 4) : make_int4(0, 0, 0, 0);
    int cnt[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      cnt[k] = tally(v[k]);
      sum += cnt[k];
    }
    FT_STAMP;
    run = block_excl_scan_1024(sum, total, s_w);
    FT_STAMP;
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (c0 + k < c1) {
        st.cell_off[c0 + k] = run;
        run += cnt[k];
      }
  } else {
    for (int c = c0; c < c1; c++) sum += tally(ldg_i4(st.cand + (size_t)c * 4));
    run = block_excl_scan_1024(sum, total, s_w);
    for (int c = c0; c < c1; c++) {
      const int4 v = ldg_i4(st.cand + (size_t)c * 4);  // (L2)
      st.cell_off[c] = run;
      run += (v.x < 0) + (v.y < 0) + (v.z < 0) + (v.w < 0);
    }
  }
  if (threadIdx.x == 0) {
    st.cell_off[ncells] = total;
    *st.count = total;
    *st.count_host = total;
  }
  // (block_excl_scan_1024's barriers also order the histogram's atomics before the reads below)
  const int bchunk = (nb + 1023) / 1024;
  const int b0 = min((int)threadIdx.x * bchunk, nb), b1 = min(b0 + bchunk, nb);
  int bsum = 0;
  for (int b = b0; b < b1; b++) bsum += s_hist[b];
  int btotal;
  FT_STAMP;
  int brun = block_excl_scan_1024(bsum, btotal, s_w);
  FT_STAMP;
  for (int b = b0; b < b1; b++) {
    st.bin_start[b] = brun;
    brun += s_hist[b];
  }
  if (threadIdx.x == 0) st.bin_start[nb] = btotal;
  FT_STAMP;
  FT_FLUSH(3);
}

__global__ void __launch_bounds__(256) k_feat_order(const VsmImage *__restrict__ imgs, int first, VsmDims d, int set_lo, VsmBinDiv bd,
                                                    VsmOrderPlan pl, int nbx, int n_img) {
  const int binsize = bd.binsize;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  uint16_t *s_g = (uint16_t *)s_raw;                      // [stage_h][stage_w]
  int4 *s_cand = (int4 *)(s_raw + pl.o_cand);            // [cells_max] the cells overlapping the rectangle (one set at a time)
  int *s_bs = (int *)(s_raw + pl.o_bs);                  // [2][bu * 4][VSM_VSUB + 1]: bin_start of the tile's fine bins, per set
  int *s_cnt = (int *)(s_raw + pl.o_cnt);                // [bu * 4] list lengths, [bu * 4] = number of survivors
  uint32_t *s_list = (uint32_t *)(s_raw + pl.o_list);    // [bu * 4][lcap]: index * 8 + v sub-row
  uint32_t *s_sv = (uint32_t *)(s_raw + pl.o_sv);        // survivors of the tile: feature index << 11 | cell slot * 4 + class
  const int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int zi = lb / nbx, bx = lb - zi * nbx;
  if (zi >= n_img) return;
  const VsmImage &im = imgs[first + zi];
  const int tv = bx / pl.tiles_u, tu = bx - tv * pl.tiles_u;
  const int t = threadIdx.x;
  // the tile's bins and their pixel rectangle at the matching resolution (bin = min(coordinate * scale / binsize, bins - 1))
  const int ub0 = tu * pl.bu, ub1 = min(ub0 + pl.bu, d.ub);
  const int x_lo = ub0 == 0 ? 0 : min(ceil_div_pos(ub0 * binsize, d.scale), d.mw);
  const int x_hi = ub1 == d.ub ? d.mw : min(ceil_div_pos(ub1 * binsize, d.scale), d.mw);
  const int y_lo = tv == 0 ? 0 : min(ceil_div_pos(tv * binsize, d.scale), d.mh);
  const int y_hi = tv + 1 == d.vb ? d.mh : min(ceil_div_pos((tv + 1) * binsize, d.scale), d.mh);
  const int nl = pl.bu * 4;
  FT_DECL;
  FT_STAMP;
  // ---- the starts of the tile's fine bins (both sets) and the Sobel responses of the rectangle + 5 pixels of halo, du | dv << 8
  // per pixel.  (Requesting EVERY load of the workgroup up front, the responses in registers too, was tried: what the extra
  // registers and LDS cost in resident workgroups made the kernel slower, 108 -> 114-150 us per 220 images.) ----
  for (int si = set_lo; si < 2; si++)
    for (int e = t; e < nl * (VSM_VSUB + 1); e += 256) {
      const int l = e / (VSM_VSUB + 1), k = e - l * (VSM_VSUB + 1);
      const int ubin = min(ub0 + (l >> 2), d.ub - 1);
      s_bs[si * nl * (VSM_VSUB + 1) + e] = ldg_i32(im.set[si].bin_start + ((l & 3) * d.ub + ubin) * (d.vb * VSM_VSUB) + tv * VSM_VSUB + k);
    }
  // the cells of both sets that can hold a pixel of the rectangle (<= 2 per thread and set: cells_cap <= 512), requested now,
  // kept in registers until their set's turn: their wait is over by the time the responses below have arrived
  int cell_h[2], ncell[2];
  int4 pc[2][2];
  int po[2][2];
#pragma unroll
  for (int si = 0; si < 2; si++) {
    const VsmSet &st = im.set[si];
    const int n = st.nms_n, n1 = n + 1, o0 = n + VSM_MARGIN;  // cell c covers pixels o0 + c * n1 .. + n
    const int cu_lo = max(0, ceil_div_pos(max(x_lo - n - o0, 0), n1)), cu_hi = min(st.ncu - 1, x_hi - 1 >= o0 ? (x_hi - 1 - o0) / n1 : -1);
    const int cv_lo = max(0, ceil_div_pos(max(y_lo - n - o0, 0), n1)), cv_hi = min(st.ncv - 1, y_hi - 1 >= o0 ? (y_hi - 1 - o0) / n1 : -1);
    const int cw = cu_hi - cu_lo + 1, ch = cv_hi - cv_lo + 1;
    cell_h[si] = ch;
    ncell[si] = (si >= set_lo && cw > 0 && ch > 0) ? cw * ch : 0;  // <= cells_cap[si] by the plan
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int e = t + 256 * i;
      pc[si][i] = make_int4(0, 0, 0, 0);
      po[si][i] = 0;
      if (e < ncell[si]) {
        const int lcu = e / ch, lcv = e - lcu * ch;  // v fastest: neighbouring threads read neighbouring cand[] entries
        const int cell = (cu_lo + lcu) * st.ncv + cv_lo + lcv;
        pc[si][i] = ldg_i4(st.cand + (size_t)cell * 4);
        po[si][i] = ldg_i32(st.cell_off + cell);
      }
    }
  }
  const int xa = (x_lo - EMIT_HALO) & ~3, ya = y_lo - EMIT_HALO;  // (may be negative: nothing there is ever read)
  const int sw4 = pl.stage_w >> 2;
  for (int e = t; e < sw4 * pl.stage_h; e += 256) {
    const int y = e / sw4, x = 4 * (e - y * sw4);
    const int u = xa + x, v = ya + y;
    uint32_t a = 0, b = 0;
    if (u >= 0 && u + 3 < d.mbpl && v >= 0 && v < d.mh && u < x_hi + EMIT_HALO && v < y_hi + EMIT_HALO) {
      a = ldg_u32(im.du + (size_t)v * d.mbpl + u);
      b = ldg_u32(im.dv + (size_t)v * d.mbpl + u);
    }
    const uint32_t lo = (a & 0xffu) | ((b & 0xffu) << 8) | ((a & 0xff00u) << 8) | ((b & 0xff00u) << 16);
    const uint32_t hi = ((a >> 16) & 0xffu) | (((b >> 16) & 0xffu) << 8) | ((a >> 24) << 16) | ((b >> 24) << 24);
    *(uint2 *)&s_g[y * pl.stage_w + x] = make_uint2(lo, hi);
  }
#pragma unroll
  for (int si = 0; si < 2; si++) {
    if (si < set_lo) continue;
    const VsmSet &st = im.set[si];
    const int lcap = pl.lcap[si];
    const int4 *cand = s_cand;
    FT_STAMP;
    __syncthreads();  // (stage complete; the previous set's lists and cells are no longer read)
    if (t <= nl) s_cnt[t] = 0;
    __syncthreads();
    FT_STAMP;
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int e = t + 256 * i;
      if (e >= ncell[si]) continue;
      const int4 c4 = pc[si][i];
      s_cand[e] = c4;
      if ((c4.x | c4.y | c4.z | c4.w) >= 0) continue;
      const int cc[4] = {c4.x, c4.y, c4.z, c4.w};
      int idx = po[si][i];
#pragma unroll
      for (int g = 0; g < 4; g++) {
        if (cc[g] >= 0) continue;
        const int u = (cc[g] & 0x3fff) * d.scale, v = ((cc[g] >> 14) & 0x3fff) * d.scale;
        const int ubin = min(bd.div(u), d.ub - 1), vbin = min(bd.div(v), d.vb - 1);
        if (ubin >= ub0 && ubin < ub1 && vbin == tv) {
          const int vsub = bd.vsub(v, vbin);
          const int l = (ubin - ub0) * 4 + g;
          const int p = atomicAdd(&s_cnt[l], 1);
          if (p < lcap) s_list[l * lcap + p] = (uint32_t)idx * 8u + (uint32_t)vsub;
          const int q = atomicAdd(&s_cnt[nl], 1);
          s_sv[q] = ((uint32_t)idx << 11) | (uint32_t)(e * 4 + g);
        }
        idx++;
      }
    }
    FT_STAMP;
    __syncthreads();
    const int nsv = s_cnt[nl];
    for (int q = t; q < nsv; q += 256) {
      const uint32_t sv = s_sv[q];
      const int e = (int)((sv >> 2) & 511u), g = (int)(sv & 3u);
      const uint32_t idx = sv >> 11;
      const int4 c4 = cand[e];
      const int cc = g == 0 ? c4.x : (g == 1 ? c4.y : (g == 2 ? c4.z : c4.w));
      const int u = cc & 0x3fff, v = (cc >> 14) & 0x3fff;
      const int us = u * d.scale, vs = v * d.scale;
      const int ubin = min(bd.div(us), d.ub - 1), vbin = min(bd.div(vs), d.vb - 1);
      const int vsub = bd.vsub(vs, vbin);
      const int l = (ubin - ub0) * 4 + g;
      // ranks: smaller indices in the reference's bin (all of the list) and in the fine bin (same sub-row)
      const int cnt = min(s_cnt[l], lcap);
      const uint32_t *L = s_list + l * lcap;
      int rank = 0, crank = 0;
      for (int k = 0; k < cnt; k += 4) {  // (lists are 16-byte aligned and a multiple of four long; entries beyond cnt do not count)
        const uint4 en4 = *(const uint4 *)(L + k);
        const uint32_t en[4] = {en4.x, en4.y, en4.z, en4.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int before = (k + j < cnt) && (en[j] >> 3) < idx;
          crank += before;
          rank += (before && (int)(en[j] & 7u) == vsub) ? 1 : 0;
        }
      }
      const int *bs = s_bs + (si * nl + l) * (VSM_VSUB + 1);  // bin_start of the fine bins (g, ubin, vbin, 0..)
      const int dst = bs[vsub] + rank, clo = bs[0];
      // descriptor (computeDescriptor, viso/matcher.cpp:433-477): 16 taps of (du, dv) from the staged rectangle
      const uint16_t *c0 = s_g + (v - ya) * pl.stage_w + (u - xa);
      uint32_t t16[16];
#pragma unroll
      for (int m = 0; m < 16; m++) {
        constexpr int8_t kdv[16] = {-1, +1, -1, +1, -1, +1, -1, +1, -5, +5, -5, +5, -3, +3, -3, +3};
        constexpr int8_t kdu[16] = {-3, -3, -1, -1, +3, +3, +1, +1, -1, -1, +1, +1, -5, -5, +5, +5};
        t16[m] = c0[kdv[m] * pl.stage_w + kdu[m]];
      }
      vsm_u4 r0, r1, r2;
      r0.x = (uint32_t)us;
      r0.y = (uint32_t)vs;
      r0.z = 0u;
      r0.w = (uint32_t)g;
      r1.x = t16[0] | (t16[1] << 16);
      r1.y = t16[2] | (t16[3] << 16);
      r1.z = t16[4] | (t16[5] << 16);
      r1.w = t16[6] | (t16[7] << 16);
      r2.x = t16[8] | (t16[9] << 16);
      r2.y = t16[10] | (t16[11] << 16);
      r2.z = t16[12] | (t16[13] << 16);
      r2.w = t16[14] | (t16[15] << 16);
      VSM_AS1 vsm_u4 *rec = (VSM_AS1 vsm_u4 *)(st.feat + (size_t)idx * 12);
      rec[0] = r0;
      rec[1] = r1;
      rec[2] = r2;
      VSM_AS1 vsm_u4 *sd = (VSM_AS1 vsm_u4 *)(st.s_desc + 2 * (size_t)dst);
      sd[0] = r1;
      sd[1] = r2;
      *(VSM_AS1 uint32_t *)(st.s_uv + dst) = (uint32_t)us | ((uint32_t)vs << 16);  // coordinates are < 16384
      *(VSM_AS1 int32_t *)(st.s_idx + dst) = (int32_t)idx;
      *(VSM_AS1 int32_t *)(st.s_rank + dst) = clo + crank;
    }
  }
  FT_STAMP;
  FT_FLUSH(2);
}

// ---------------------------------------------------------------------------------------
// M1 createIndexVector, viso/matcher.cpp:870-890, as a stable counting sort into the
// bin-contiguous SoA arrays (see VsmSet).  fine bin = (class*ub + u_bin)*(vb*VSM_VSUB) + v sub-row,
// so that the rows a query visits for one u_bin are one contiguous run.  Histogram: k_emit.  Then
//   k_bin_scan    exclusive scan of the histogram (one block per image/set)
//   k_bin_scatter every feature takes a slot of its bin (unordered, atomic cursor)
//   k_bin_rank    every slot finds its stable rank = number of smaller feature indices in its
//                 fine bin, and its place in the reference's coarser (u_bin, v_bin, index) order
//                 (a bin holds at most one feature per NMS cell and class: a few dozen), and
//                 writes the sorted coordinate / descriptor / index / reference-rank arrays
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) k_bin_scan(const VsmImage *__restrict__ imgs, int first, int set_lo, int nb) {
  __shared__ int s_w[17];
  if ((int)blockIdx.y < set_lo) return;
  const VsmSet &st = imgs[first + blockIdx.z].set[blockIdx.y];
  const int chunk = (nb + 1023) / 1024;
  const int b0 = min((int)threadIdx.x * chunk, nb), b1 = min(b0 + chunk, nb);
  int sum = 0;
  for (int b = b0; b < b1; b++) sum += st.bin_cnt[b];
  int total;
  int run = block_excl_scan_1024(sum, total, s_w);
  for (int b = b0; b < b1; b++) {
    const int c = st.bin_cnt[b];
    st.bin_start[b] = run;
    st.bin_cnt[b] = run;  // becomes the scatter cursor
    run += c;
  }
  if (threadIdx.x == 0) st.bin_start[nb] = total;
}

__global__ void __launch_bounds__(256) k_bin_scatter(const VsmImage *__restrict__ imgs, int first, int set_lo) {
  if ((int)blockIdx.y < set_lo) return;
  const VsmSet &st = imgs[first + blockIdx.z].set[blockIdx.y];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= *st.count) return;
  st.tmp[atomicAdd(&st.bin_cnt[st.binid[i]], 1)] = i;
}

__global__ void __launch_bounds__(256) k_bin_rank(const VsmImage *__restrict__ imgs, int first, int set_lo) {
  if ((int)blockIdx.y < set_lo) return;
  const VsmSet &st = imgs[first + blockIdx.z].set[blockIdx.y];
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= *st.count) return;
  const int idx = st.tmp[p];
  const int b = st.binid[idx];
  const int lo = st.bin_start[b], hi = st.bin_start[b + 1];
  // the reference's bin = the VSM_VSUB fine bins b - b % VSM_VSUB ..., contiguous in the sorted order
  const int cb = (b / VSM_VSUB) * VSM_VSUB;
  const int clo = st.bin_start[cb], chi = st.bin_start[cb + VSM_VSUB];
  int rank = 0, crank = 0;
  for (int q = clo; q < chi; q++) {
    const int before = st.tmp[q] < idx;
    crank += before;
    rank += (q >= lo && q < hi) ? before : 0;
  }
  const int dst = lo + rank;
  st.s_rank[dst] = clo + crank;
  const int32_t *rec = st.feat + (size_t)idx * 12;
  const int4 hd = *(const int4 *)rec;
  st.s_idx[dst] = idx;
  st.s_uv[dst] = (uint32_t)hd.x | ((uint32_t)hd.y << 16);  // coordinates are < 16384
  st.s_desc[2 * dst] = *(const uint4 *)(rec + 4);
  st.s_desc[2 * dst + 1] = *(const uint4 *)(rec + 8);
}

// Head records of the dense set's fine bins (VsmSet::heads): dword 0 = the bin's start in the sorted arrays, dwords 1..15 = the
// packed coordinates of the 15 candidates from there on, whatever bins they lie in (a search window's run of candidates is
// consecutive in that order: fine rows vfmin..vfmax of one (class, u-bin) column).  k_match's second pass reads a window's bin
// start AND its candidates' coordinates in one round trip: measured on the benchmark sequence (the trip-counting build of
// k_match that a9ef39f was the last commit to carry), 15 inline candidates cover every lane's longest run in 99.9-100 % of
// a wave's stages, 7 in 1.7 % (groups sharing a run) / 41.7 % (a lane per bin), 3 in 0.4 % - a wave saves the trip only if
// all of its lanes do.
// One thread per (bin, quarter of the record).
__global__ void __launch_bounds__(256) k_feat_heads(const VsmImage *__restrict__ imgs, int first, int nb) {
  const VsmSet &st = imgs[first + blockIdx.y].set[1];
  const int tid = blockIdx.x * 256 + threadIdx.x, b = tid >> 2, j = tid & 3;
  if (b >= nb || st.heads == nullptr) return;
  const int start = ldg_i32(st.bin_start + b);
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int at = min(start + 4 * j + i - 1, st.cap - 1);  // (beyond the set's count: whatever is there - a position >= the run's end is never taken)
    w[i] = (j == 0 && i == 0) ? (uint32_t)start : ldg_u32_at(st.s_uv, (uint32_t)max(at, 0) * 4u);
  }
  st.heads[b * 4 + j] = make_uint4(w[0], w[1], w[2], w[3]);
}

// =======================================================================================
// launchers
// =======================================================================================

// plan of k_feat_order for a geometry; false = it does not fit (huge search bins or suppression cells: the separate kernels)
static bool vsm_order_plan(const VsmDims &d, const VsmImage &im, int set_lo, int binsize, int nb, VsmOrderPlan &pl) {
  static bool attr_set = false;  // (the scan kernel's histogram may want more than the default 64 KB of dynamic LDS)
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_feat_scan), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    attr_set = true;
  }
  if ((size_t)nb * 4 > 150 * 1024) return false;
  const int bw = (binsize + d.scale - 1) / d.scale + 1;  // pixels of one search bin at the matching resolution (at most)
  if (bw > 72) return false;
  pl.bu = std::max(1, std::min(8, 128 / bw));
  pl.tiles_u = cdiv(d.ub, pl.bu);
  pl.tiles_v = d.vb;
  pl.stage_w = (pl.bu * bw + 13 + 3) & ~3;
  pl.stage_h = bw + 10;
  int maxcells = 0, maxl = 0;
  for (int k = 0; k < 2; k++) {
    const VsmSet &st = im.set[k];
    pl.cells_cap[k] = pl.lcap[k] = 0;
    if (k < set_lo || st.ncu * st.ncv <= 0) continue;
    const int n1 = st.nms_n + 1;
    const int cwt = std::min(st.ncu, (pl.bu * bw - 1) / n1 + 2), cht = std::min(st.ncv, (bw - 1) / n1 + 2);  // cells meeting a tile / ...
    const int cwb = std::min(st.ncu, (bw - 1) / n1 + 2);                                                  // ... one bin
    pl.cells_cap[k] = cwt * cht;
    pl.lcap[k] = (cwb * cht + 3) & ~3;
    maxcells = std::max(maxcells, pl.cells_cap[k]);
    maxl = std::max(maxl, pl.lcap[k]);
    if (st.cap >= (1 << 21)) return false;  // (survivor words: 21 bits of feature index)
  }
  if (maxcells <= 0 || maxcells > 512) return false;
  int o = pl.stage_w * pl.stage_h * 2;
  auto take = [&](int bytes) {
    o = (o + 15) & ~15;
    const int at = o;
    o += bytes;
    return at;
  };
  pl.cells_max = maxcells;
  pl.o_cand = take(maxcells * 16);
  pl.o_bs = take(2 * pl.bu * 4 * (VSM_VSUB + 1) * 4);
  pl.o_cnt = take((pl.bu * 4 + 1) * 4);
  pl.o_list = take(pl.bu * 4 * maxl * 4);
  pl.o_sv = take(maxcells * 4 * 4);
  pl.lds_bytes = (o + 15) & ~15;
  return pl.lds_bytes <= 64 * 1024;
}

void vsm_launch_ingest(hipStream_t s, VsmProf &pf, const VsmImage *d_imgs, int first, const uint8_t *src0,
                       const uint8_t *src1, size_t frame_stride, int32_t src_bpl, int n_frames, const VsmDims &d) {
  const int sides = src1 ? 2 : 1;
  dim3 grid(cdiv((d.bpl / 4) * d.h, 256), 1, n_frames * sides);
  pf.begin(VSM_K_INGEST, s);
  hipLaunchKernelGGL(k_ingest, grid, dim3(256), 0, s, d_imgs, first, src0, src1, frame_stride, src_bpl, sides, d.w, d.h,
                     d.bpl);
  pf.end(s);
}

void vsm_launch_front(hipStream_t s, VsmProf &pf, const VsmImage *d_imgs, int first, const uint8_t *src0, const uint8_t *src1,
                      size_t frame_stride, int32_t src_bpl, int n_frames, const VsmDims &d, int write_img) {
  const int sides = src1 ? 2 : 1;
  const int nbx = cdiv(d.bpl, FRONT_TW), nby = cdiv(d.h, FRONT_TH), n_img = n_frames * sides;
  dim3 grid(((nbx * nby * n_img + 7) / 8) * 8);
  pf.begin(VSM_K_FRONT, s);
  hipLaunchKernelGGL(k_front, grid, dim3(256), 0, s, d_imgs, first, src0, src1, frame_stride, src_bpl, sides, d, write_img, nbx, nby, n_img);
  pf.end(s);
}

int vsm_launch_features(hipStream_t s, VsmProf &pf, const VsmImage *d_imgs, int first, int n_img, const VsmDims &d,
                        int16_t *f1, int16_t *f2, size_t f_stride, int nms_tau, int multi_stage, int half_res,
                        int binsize, const VsmImage *h_imgs, int front_done, int fused) {
  if (half_res && !front_done) {
    pf.begin(VSM_K_HALVE, s);
    hipLaunchKernelGGL(k_halve, dim3(cdiv(d.mbpl / 4, 256), d.mh, n_img), dim3(256), 0, s, d_imgs, first, d);
    pf.end(s);
    pf.begin(VSM_K_SOBEL_FULL, s);
    hipLaunchKernelGGL(k_filters<true>, dim3(cdiv(d.bpl / 4, 64), cdiv(d.h, 16), n_img), dim3(256), 0, s, d_imgs, first,
                       d.bpl, d.h, (int16_t *)nullptr, (int16_t *)nullptr, (size_t)0);
    pf.end(s);
  }
  const int set_lo = multi_stage ? 0 : 1;
  const int nb = 4 * d.ub * d.vb * VSM_VSUB;  // fine bins
  int max_cells = 0, max_cap = 0;
  for (int k = 0; k < 2; k++) {
    max_cells = max(max_cells, h_imgs[first].set[k].ncu * h_imgs[first].set[k].ncv);
    max_cap = max(max_cap, h_imgs[first].set[k].cap);
  }
  // the fused tiles serve the default radii (dense 3, sparse 9: viso/matcher.cpp:685-687); other radii take the separate
  // filter + suppression kernels with f1 / f2 in HBM
  const VsmSet &sd = h_imgs[first].set[1], &ss = h_imgs[first].set[0];
  const bool fuse = (fused & 1) && sd.nms_n == 3 && sd.ncu * sd.ncv > 0 && (!multi_stage || (ss.nms_n == 9 && ss.ncu * ss.ncv > 0));
  if (fuse) {
    int dx, dy;
    vsm_feat_tiles(d, sd, dx, dy);
    const int nbx = dx * dy;
    pf.begin(VSM_K_FEAT_DENSE, s);
    if (fused & 2)
      hipLaunchKernelGGL(k_feat_dense<true>, dim3(((nbx * n_img + 7) / 8) * 8), dim3(256), 0, s, d_imgs, first, d, nms_tau, dx, nbx,
                         n_img, f1, f2, f_stride);
    else
      hipLaunchKernelGGL(k_feat_dense<false>, dim3(((nbx * n_img + 7) / 8) * 8), dim3(256), 0, s, d_imgs, first, d, nms_tau, dx, nbx,
                         n_img, f1, f2, f_stride);
    pf.end(s);
    if (multi_stage) {
      const int sx = cdiv(ss.ncu, VfSparse::CU), sy = cdiv(ss.ncv, VfSparse::CV);
      pf.begin(VSM_K_FEAT_SPARSE, s);
      hipLaunchKernelGGL(k_feat_sparse, dim3(((sx * sy * n_img + 7) / 8) * 8), dim3(256), 0, s, d_imgs, first, d, nms_tau, sx, sx * sy,
                         n_img);
      pf.end(s);
    }
  } else {
    pf.begin(VSM_K_FILTERS, s);
    hipLaunchKernelGGL(k_filters<false>, dim3(cdiv(d.mbpl / 4, 64), cdiv(d.mh, 16), n_img), dim3(256), 0, s, d_imgs, first,
                       d.mbpl, d.mh, f1, f2, f_stride);
    pf.end(s);
  }
  if (max_cells > 0 && !fuse) {
    // per set: small n -> LDS tile kernel, mid n -> 8-lane LDS tile kernel, else wave per cell
    for (int k = set_lo; k < 2; k++) {
      const VsmSet &st = h_imgs[first].set[k];
      if (st.ncu * st.ncv <= 0) continue;
      pf.begin(k == 1 ? VSM_K_NMS : VSM_K_NMS_SPARSE, s);
      if (st.nms_n == 3) {
        const int nbx = cdiv(st.ncu, 16) * cdiv(st.ncv, 8);
        hipLaunchKernelGGL((k_nms_fixed<3, 16, 8, 1>), dim3(((nbx * n_img + 7) / 8) * 8), dim3(256), 0, s, d_imgs, first, d,
                           f1, f2, f_stride, nms_tau, k, nbx, n_img);
      } else if (st.nms_n == 9) {
        const int nbx = cdiv(st.ncu, 4) * cdiv(st.ncv, 4);
        hipLaunchKernelGGL((k_nms_fixed<9, 4, 4, 8>), dim3(((nbx * n_img + 7) / 8) * 8), dim3(256), 0, s, d_imgs, first, d,
                           f1, f2, f_stride, nms_tau, k, nbx, n_img);
      } else if (st.nms_n <= NMS_TILE_MAXN) {
        const int nbx = cdiv(st.ncu, NMS_TCU) * cdiv(st.ncv, NMS_TCV);
        hipLaunchKernelGGL(k_nms_tile, dim3(((nbx * n_img + 7) / 8) * 8), dim3(256), 0, s, d_imgs, first, d, f1, f2, f_stride,
                           nms_tau, k, nbx, n_img);
      } else if (st.nms_n <= NMS8_MAXN) {
        const int nbx = cdiv(st.ncu, NMS8_TC) * cdiv(st.ncv, NMS8_TC);
        hipLaunchKernelGGL(k_nms_tile8, dim3(((nbx * n_img + 7) / 8) * 8), dim3(256), 0, s, d_imgs, first, d, f1, f2, f_stride,
                           nms_tau, k, nbx, n_img);
      }
      else
        hipLaunchKernelGGL(k_nms, dim3(cdiv(st.ncu * st.ncv, 4), 2, n_img * 2), dim3(256), 0, s, d_imgs, first, d, f1, f2,
                           f_stride, nms_tau, k, k);
      pf.end(s);
    }
  }
  // records + bin-sorted copy: the two-kernel form where a tile of whole search bins fits a workgroup's LDS
  VsmOrderPlan pl;
  if ((fused & 4) == 0 && max_cells > 0 && vsm_order_plan(d, h_imgs[first], set_lo, binsize, nb, pl)) {
    pf.begin(VSM_K_FEAT_SCAN, s);
    VsmBinDiv bd;
    bd.binsize = binsize;
    bd.magic = binsize >= 2 ? (uint32_t)(((1ull << 32) + (uint64_t)binsize - 1) / (uint64_t)binsize) : 0u;
    hipLaunchKernelGGL(k_feat_scan, dim3(1, 2, n_img), dim3(1024), (size_t)nb * 4, s, d_imgs, first, set_lo, d, bd, nb);
    pf.end(s);
    pf.begin(VSM_K_FEAT_ORDER, s);
    const int nbx = pl.tiles_u * pl.tiles_v;
    hipLaunchKernelGGL(k_feat_order, dim3(((nbx * n_img + 7) / 8) * 8), dim3(256), (size_t)pl.lds_bytes, s, d_imgs, first, d, set_lo, bd, pl,
                       nbx, n_img);
    pf.end(s);
    if (h_imgs[first].set[1].heads) hipLaunchKernelGGL(k_feat_heads, dim3(cdiv(nb * 4, 256), n_img), dim3(256), 0, s, d_imgs, first, nb);
    return (!fuse || (fused & 2)) ? 1 : 0;
  }
  pf.begin(VSM_K_SCAN, s);
  hipLaunchKernelGGL(k_scan_cells, dim3(1, 2, n_img), dim3(1024), 0, s, d_imgs, first, set_lo, nb);
  pf.end(s);
  if (max_cells > 0) {
    pf.begin(VSM_K_EMIT, s);
    int nbx = 1;  // tiles per image: the larger of the two sets decides the grid
    for (int k = set_lo; k < 2; k++) {
      const VsmSet &st = h_imgs[first].set[k];
      const int n1 = st.nms_n + 1;
      nbx = max(nbx, cdiv(st.ncu, max(EMIT_TW / n1, 1)) * cdiv(st.ncv, max(EMIT_TH / n1, 1)));
    }
    hipLaunchKernelGGL(k_emit, dim3(((nbx * n_img + 7) / 8) * 8, 2), dim3(256), 0, s, d_imgs, first, d, set_lo, binsize, nbx,
                       n_img);
    pf.end(s);
  }
  pf.begin(VSM_K_BINSCAN, s);
  hipLaunchKernelGGL(k_bin_scan, dim3(1, 2, n_img), dim3(1024), 0, s, d_imgs, first, set_lo, nb);
  pf.end(s);
  pf.begin(VSM_K_BINSCATTER, s);
  hipLaunchKernelGGL(k_bin_scatter, dim3(cdiv(max_cap, 256), 2, n_img), dim3(256), 0, s, d_imgs, first, set_lo);
  pf.end(s);
  pf.begin(VSM_K_BINRANK, s);
  hipLaunchKernelGGL(k_bin_rank, dim3(cdiv(max_cap, 256), 2, n_img), dim3(256), 0, s, d_imgs, first, set_lo);
  pf.end(s);
  if (h_imgs[first].set[1].heads) hipLaunchKernelGGL(k_feat_heads, dim3(cdiv(nb * 4, 256), n_img), dim3(256), 0, s, d_imgs, first, nb);
  return (!fuse || (fused & 2)) ? 1 : 0;
}

