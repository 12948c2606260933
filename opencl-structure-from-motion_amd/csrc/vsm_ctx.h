// A context's two long-lived blocks as pure arithmetic: the device arena and the host-mapped result
// block of a VsmCtx (vsm_api.cpp).  Every array is declared once - its element type - and placed once - its count and the
// spare bytes behind it -, as a function of the call's counts; bind() is the one place where an address inside a block is
// formed.  (Dc2Layout, vsm_layouts.h, does the same for the bank of a Delaunay chain.)  No HIP call in here: the CPU suite
// pins every offset through vsm_debug_ctx_layout (tests/test_ctx_layout_cpu.py) and tools/ctx_host_check.cpp runs the
// geometry's error paths and bind() under the sanitizers.
#pragma once

#include <math.h>

#include "vsm_internal.h"
#include "vsm_stage.h"

static inline int32_t bpl16(int32_t w) { return w + 15 - (w - 1) % 16; }  // viso/matcher.cpp:160
static inline int32_t nms_cells(int32_t len, int32_t n) {  // loop count of "for (i=n+margin; i<len-n-margin; i+=n+1)"
  const int32_t span = len - 2 * n - 2 * VSM_MARGIN;
  return span > 0 ? (span + n) / (n + 1) : 0;
}
// match bins along `len` pixels (binsize >= 1) and over a frame (0: there is no such bin size); k_dc2_prior keeps the
// statistics of at most 1024 bins in LDS
static inline size_t vsm_bins_along(int32_t len, int32_t binsize) { return (size_t)ceilf((float)len / (float)binsize); }
static inline size_t vsm_match_bins(const vsm_params &p, int32_t w, int32_t h) {
  return p.match_binsize >= 1 ? vsm_bins_along(w, p.match_binsize) * vsm_bins_along(h, p.match_binsize) : 0;
}

// What a context's blocks are sized by.  Set 0 is the sparse set, 1 the dense one.
struct VsmGeom {
  VsmDims dims{};
  int32_t nms[2] = {0, 0}, ncu[2] = {0, 0}, ncv[2] = {0, 0};  // suppression radius and cells per set
  int32_t cap_set[2] = {0, 0}, nb = 0;                        // features a set has room for; match bins x 4 classes
  size_t qcap = 0;           // queries a pair has room for
  size_t f_stride = 0;       // int16 elements per image plane of f1 / f2 (and the bytes of a matching-resolution plane)
  size_t ranges_stride = 0;  // floats per pair
  // a slot of a result arena (VsmResArena, the look-ahead call's): the longest list a pair or a frame can leave
  size_t list_slot_bytes() const { return al256((size_t)cap_set[1] * sizeof(vsm_p_match)); }
};
// VSM_OK, VSM_EDIMS, or VSM_EARG with a message on stderr
static inline int vsm_ctx_geometry(const vsm_params &p, int32_t w, int32_t hh, VsmGeom &g) {
  VsmDims &d = g.dims;
  d.w = w, d.h = hh, d.bpl = bpl16(w), d.scale = p.half_resolution ? 2 : 1;
  d.mw = p.half_resolution ? w / 2 : w, d.mh = p.half_resolution ? hh / 2 : hh, d.mbpl = p.half_resolution ? bpl16(d.mw) : d.bpl;
  if (d.mw <= 0 || d.mh <= 0 || d.w >= 16384 || d.h >= 16384) return VSM_EDIMS;  // 14-bit coordinates
  if (p.match_binsize < 1 || p.match_binsize > 32768) {  // (before anything divides by it)
    fprintf(stderr, "visomatch: match_binsize %d is not usable\n", p.match_binsize);
    return VSM_EARG;
  }
  d.ub = (int32_t)vsm_bins_along(w, p.match_binsize), d.vb = (int32_t)vsm_bins_along(hh, p.match_binsize);
  g.nb = 4 * d.ub * d.vb;
  if (g.nb > (1 << 22)) {
    fprintf(stderr, "visomatch: match_binsize %d is not usable (%d bins)\n", p.match_binsize, g.nb);
    return VSM_EARG;
  }
  if (p.nms_n < 1 || p.nms_n > 31) {
    fprintf(stderr, "visomatch: nms_n %d outside the supported range 1..31\n", p.nms_n);
    return VSM_EARG;
  }
  g.nms[0] = p.nms_n * 3, g.nms[1] = p.nms_n;  // viso/matcher.cpp:685-687
  if (g.nms[0] > 10) g.nms[0] = p.nms_n > 10 ? p.nms_n : 10;
  for (int k = 0; k < 2; k++) {
    g.ncu[k] = nms_cells(d.mw, g.nms[k]), g.ncv[k] = nms_cells(d.mh, g.nms[k]);
    g.cap_set[k] = std::max(4 * g.ncu[k] * g.ncv[k], 4);
  }
  g.qcap = (size_t)std::max(g.cap_set[0], g.cap_set[1]);
  g.f_stride = al256((size_t)d.mbpl * d.mh + 64);
  g.ranges_stride = (size_t)d.ub * d.vb * 16;
  return VSM_OK;
}

// the tables and views of a context's blocks that bind() fills
struct VsmCtxViews {
  std::vector<VsmImage> h_imgs;  // image id = frame_slot*2 + side
  std::vector<VsmPair> h_pairs;
  VsmImage *d_imgs = nullptr;
  VsmPair *d_pairs = nullptr;
  VsmJob *d_jobs = nullptr;
  int16_t *f1 = nullptr, *f2 = nullptr;  // transient filter responses of one feature launch
  float *d_ranges = nullptr;
  // host views of the host-mapped block: kernels write feature counts and exported match lists straight into it, so results
  // need a stream sync but no D2H copy
  int32_t *hm_counts = nullptr, *hm_lcount = nullptr;  // [nframes*2 images][2 sets], [npairs][2]
  std::vector<vsm_p_match *> hm_list1, hm_list2;       // per pair
};

// The blocks of a context of nframes frame slots (two images each) and npairs frame pairs.
struct VsmCtxLayout {
  struct Set {
    VsmArray<int32_t> feat, count, cand, cell_off, bin_start, bin_cnt, s_rank, binid, s_idx, tmp;
    VsmArray<uint32_t> s_uv;
    VsmArray<uint4> s_desc, heads;  // heads: the dense set with `heads` on
  };
  struct Image {
    VsmArray<uint8_t> img, imgm, du, dv, duvt;  // imgm is img at full resolution; duvt: half resolution only
    Set set[2];
  };
  struct Pair {
    VsmArray<vsm_p_match> raw, list1, list2, hlist1, hlist2;  // hlist*: in the host-mapped block
    VsmArray<int32_t> flag, blockcnt, count, pf;              // pf: refinement == 2 (per-frame ring: one pair; look-ahead banks: every pair)
    VsmArray<uint64_t> keys[2];
  };
  const VsmGeom g;
  const bool half;
  std::vector<Image> img;
  std::vector<Pair> pair;
  VsmArray<int16_t> f1, f2;
  VsmArray<float> ranges;
  VsmArray<VsmImage> imgs;
  VsmArray<VsmPair> pairs;
  VsmArray<VsmJob> jobs;
  VsmArray<int32_t> hm_counts, hm_lcount;
  VsmPlacer arena, hm;     // arena.at / hm.at: the blocks' sizes
  size_t pair_stride = 0;  // bytes from one pair's arrays (raw, lists, keys ...) to the next pair's
  size_t hm_zeroed = 0;    // the counts in front of the host-mapped block, which start at zero

  VsmCtxLayout(const VsmGeom &g_, const vsm_params &p, int nframes, int npairs, bool heads)
      : g(g_), half(p.half_resolution != 0), img((size_t)nframes * 2), pair((size_t)npairs) {
    const VsmDims &d = g.dims;
    const size_t full = (size_t)d.bpl * d.h, mres = (size_t)d.mbpl * d.mh, fine = (size_t)g.nb * VSM_VSUB, cap0 = (size_t)g.cap_set[0], q = g.qcap;
    VsmPlacer &a = arena;
    for (int i = 0; i < (int)img.size(); i++) {
      Image &im = img[i];
      a.put(im.img, "img", i, -1, full, 64);  // (+ 64 behind every plane)
      if (half) a.put(im.imgm, "imgm", i, -1, mres, 64);
      else im.imgm = im.img, a.rows.push_back({"imgm", i, -1, im.img.at, full + 64});
      a.put(im.du, "du", i, -1, mres, 64); a.put(im.dv, "dv", i, -1, mres, 64);
      if (half) a.put(im.duvt, "duvt", i, -1, (size_t)d.bpl * ((d.h + 7) & ~7) * 2, 256);  // (+ one tile row of slack: windows load the tile to their right)
      for (int k = 0; k < 2; k++) {
        Set &s = im.set[k];
        const size_t cap = (size_t)g.cap_set[k], cells = (size_t)g.ncu[k] * g.ncv[k];
        // (a record behind cand, two entries behind cell_off, one behind the fine bins' starts and counts)
        a.put(s.feat, "feat", i, k, cap * 12); a.put(s.count, "count", i, k, 1); a.put(s.cand, "cand", i, k, (cells + 1) * 4); a.put(s.cell_off, "cell_off", i, k, cells + 2);
        a.put(s.bin_start, "bin_start", i, k, fine + 1); a.put(s.bin_cnt, "bin_cnt", i, k, fine + 1); a.put(s.s_rank, "s_rank", i, k, cap); a.put(s.binid, "binid", i, k, cap);
        a.put(s.s_idx, "s_idx", i, k, cap); a.put(s.s_uv, "s_uv", i, k, cap * 2); a.put(s.s_desc, "s_desc", i, k, cap * 2); a.put(s.tmp, "tmp", i, k, cap);
        if (k == 1 && heads) a.put(s.heads, "heads", i, k, fine * 4);
      }
    }
    a.put(f1, "f1", -1, -1, g.f_stride * img.size()); a.put(f2, "f2", -1, -1, g.f_stride * img.size());
    hm.put(hm_counts, "hm_counts", -1, -1, img.size() * 2); hm.put(hm_lcount, "hm_lcount", -1, -1, pair.size() * 2);
    hm_zeroed = hm.at;
    for (int j = 0; j < npairs; j++) {
      Pair &pr = pair[j];
      a.put(pr.raw, "raw", j, -1, q); a.put(pr.flag, "flag", j, -1, q); a.put(pr.blockcnt, "blockcnt", j, -1, q / 256 + 2);  // (an entry more than the blocks of 256 queries and one)
      a.put(pr.list1, "list1", j, -1, cap0); a.put(pr.list2, "list2", j, -1, q); a.put(pr.count, "count", j, -1, 4);
      if (p.refinement == 2) a.put(pr.pf, "pf", j, -1, q * 3 * 12);
      // the chains' keys beside the lists they index (every pair takes the same room: one stride from pair to pair)
      a.put(pr.keys[0], "keys1", j, -1, cap0); a.put(pr.keys[1], "keys2", j, -1, q);
      pair_stride = a.at - pr.raw.at;
      hm.put(pr.hlist1, "hlist1", j, -1, cap0); hm.put(pr.hlist2, "hlist2", j, -1, q);
    }
    a.put(ranges, "ranges", -1, -1, g.ranges_stride * pair.size());
    a.put(imgs, "imgs", -1, -1, img.size()); a.put(pairs, "pairs", -1, -1, pair.size()); a.put(jobs, "jobs", -1, -1, pair.size());
  }

  // The image and pair tables and the views, for the arena at `b` and the host-mapped block at hm_host, which the device
  // sees at hm_dev.
  void bind(uint8_t *b, uint8_t *hm_host, uint8_t *hm_dev, VsmCtxViews &v) const {
    v.h_imgs.resize(img.size());
    for (size_t i = 0; i < img.size(); i++) {
      const Image &l = img[i];
      VsmImage &im = v.h_imgs[i];
      im.img = l.img.in(b); im.imgm = l.imgm.in(b); im.du = l.du.in(b); im.dv = l.dv.in(b);
      im.du_full = half ? nullptr : im.du; im.dv_full = half ? nullptr : im.dv; im.duv_tiled = half ? l.duvt.in(b) : nullptr;
      for (int k = 0; k < 2; k++) {
        const Set &ls = l.set[k];
        VsmSet &s = im.set[k];
        s.feat = ls.feat.in(b); s.count = ls.count.in(b); s.count_host = hm_counts.in(hm_dev) + (i * 2 + k); s.cand = ls.cand.in(b); s.cell_off = ls.cell_off.in(b);
        s.bin_start = ls.bin_start.in(b); s.bin_cnt = ls.bin_cnt.in(b); s.binid = ls.binid.in(b); s.s_rank = ls.s_rank.in(b); s.s_idx = ls.s_idx.in(b);
        s.s_uv = ls.s_uv.in(b); s.s_desc = ls.s_desc.in(b); s.tmp = ls.tmp.in(b); s.heads = ls.heads.n ? ls.heads.in(b) : nullptr;
        s.cap = g.cap_set[k]; s.nms_n = g.nms[k]; s.ncu = g.ncu[k]; s.ncv = g.ncv[k];
      }
    }
    v.f1 = f1.in(b); v.f2 = f2.in(b); v.d_ranges = ranges.in(b); v.d_imgs = imgs.in(b); v.d_pairs = pairs.in(b); v.d_jobs = jobs.in(b);
    v.hm_counts = hm_counts.in(hm_host); v.hm_lcount = hm_lcount.in(hm_host);
    v.h_pairs.resize(pair.size()); v.hm_list1.resize(pair.size()); v.hm_list2.resize(pair.size());
    for (size_t j = 0; j < pair.size(); j++) {
      const Pair &l = pair[j];
      VsmPair &pr = v.h_pairs[j];
      pr.raw = l.raw.in(b); pr.flag = l.flag.in(b); pr.blockcnt = l.blockcnt.in(b); pr.list1 = l.list1.in(b); pr.list2 = l.list2.in(b); pr.count = l.count.in(b);
      pr.ranges = v.d_ranges + j * g.ranges_stride;
      pr.pf = l.pf.n ? l.pf.in(b) : nullptr;
      for (int k = 0; k < 2; k++) pr.keys[k] = l.keys[k].in(b), pr.key_cap[k] = (int32_t)l.keys[k].n;
      v.hm_list1[j] = l.hlist1.in(hm_host); v.hm_list2[j] = l.hlist2.in(hm_host);
      pr.hlist1 = l.hlist1.in(hm_dev); pr.hlist2 = l.hlist2.in(hm_dev); pr.hcount = hm_lcount.in(hm_dev) + 2 * j;
    }
  }
};
