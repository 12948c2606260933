// Stand-alone host check of the matcher's device blocks (csrc/vsm_ctx.h, Dc2Layout of csrc/vsm_layouts.h): the geometry's result codes over its error
// cases - among them match_binsize = 0, which the context's set-up once divided by before it looked at it -, and bind() of
// the context (VsmCtxLayout) and of a chain's bank (Dc2Layout) into real buffers of the layouts' sizes at the three small
// frame sizes of the suite: every pointer of every VsmImage, VsmSet, VsmPair and Dc2PairPtr is its array's offset behind its
// block's base, and every array is written from end to end through its pointer.  The expected offsets themselves are not
// restated here: tests/test_ctx_layout_cpu.py owns them.  No HIP call is made.  Meant to be built with the sanitizers, e.g.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude \
//       -Iopencl-structure-from-motion_amd/csrc tools/ctx_host_check.cpp -o ctx_host_check
// Prints "ok" and returns 0, or says what differed.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "vsm_ctx.h"
#include "vsm_layouts.h"

static int fails = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); \
      fails++;                                               \
    }                                                        \
  } while (0)

// the pointer is the array's place behind `base`, and the array's elements can be written there
#define AT(ptr, arr, base)                                  \
  do {                                                      \
    CHECK((const uint8_t *)(ptr) == (base) + (arr).at);     \
    memset((void *)(ptr), 0x5a, (arr).n * sizeof(*(ptr)));  \
  } while (0)

static vsm_params params(int half, int refinement, int nms_n, int binsize) {
  vsm_params p;
  memset(&p, 0, sizeof(p));
  p.half_resolution = half, p.refinement = refinement, p.nms_n = nms_n, p.match_binsize = binsize;
  return p;
}

static void check_geometry_errors() {
  VsmGeom g;
  CHECK(vsm_ctx_geometry(params(1, 1, 3, 50), 16384, 48, g) == VSM_EDIMS);
  CHECK(vsm_ctx_geometry(params(1, 1, 3, 50), 48, 16384, g) == VSM_EDIMS);
  CHECK(vsm_ctx_geometry(params(1, 1, 3, 50), 1, 375, g) == VSM_EDIMS);   // a half image of no width
  CHECK(vsm_ctx_geometry(params(1, 1, 3, 0), 16384, 48, g) == VSM_EDIMS);  // dimensions first
  for (int binsize : {0, -1, 32769}) CHECK(vsm_ctx_geometry(params(1, 1, 3, binsize), 1242, 375, g) == VSM_EARG);
  CHECK(vsm_ctx_geometry(params(1, 1, 3, 1), 2048, 1024, g) == VSM_EARG);  // beyond 2^22 bins
  CHECK(vsm_ctx_geometry(params(1, 1, 0, 0), 1242, 375, g) == VSM_EARG);
  for (int nms_n : {0, 32}) CHECK(vsm_ctx_geometry(params(1, 1, nms_n, 50), 1242, 375, g) == VSM_EARG);
  CHECK(vsm_ctx_geometry(params(1, 1, 3, 50), 1242, 375, g) == VSM_OK && g.dims.ub == 25 && g.dims.vb == 8);
  CHECK(vsm_ctx_geometry(params(0, 1, 31, 32768), 16383, 16383, g) == VSM_OK && g.nb == 4);
  const vsm_params none = params(1, 1, 3, 0);
  CHECK(vsm_match_bins(none, 1242, 375) == 0 && vsm_match_bins(params(1, 1, 3, 50), 1242, 375) == 200);
}

static void check_ctx_bind(int32_t w, int32_t hh, int half, int refinement, bool heads, int nframes, int npairs) {
  const vsm_params p = params(half, refinement, 3, 50);
  VsmGeom g;
  CHECK(vsm_ctx_geometry(p, w, hh, g) == VSM_OK);
  const VsmCtxLayout L(g, p, nframes, npairs, heads);
  std::vector<uint8_t> arena(L.arena.at), host(L.hm.at), dev(L.hm.at);  // (the host-mapped block as the host and as the device see it)
  uint8_t *const b = arena.data(), *const hh_ = host.data(), *const hd = dev.data();
  VsmCtxViews v;
  L.bind(b, hh_, hd, v);
  CHECK(v.h_imgs.size() == (size_t)nframes * 2 && v.h_pairs.size() == (size_t)npairs && v.hm_list1.size() == (size_t)npairs && v.hm_list2.size() == (size_t)npairs);
  for (size_t i = 0; i < v.h_imgs.size(); i++) {
    const VsmCtxLayout::Image &l = L.img[i];
    const VsmImage &im = v.h_imgs[i];
    AT(im.img, l.img, b); AT(im.imgm, l.imgm, b); AT(im.du, l.du, b); AT(im.dv, l.dv, b);
    CHECK((im.imgm == im.img) == !half && im.du_full == (half ? nullptr : im.du) && im.dv_full == (half ? nullptr : im.dv));
    if (half) AT(im.duv_tiled, l.duvt, b);
    else CHECK(im.duv_tiled == nullptr && l.duvt.n == 0);
    for (int k = 0; k < 2; k++) {
      const VsmCtxLayout::Set &ls = l.set[k];
      const VsmSet &s = im.set[k];
      AT(s.feat, ls.feat, b); AT(s.count, ls.count, b); AT(s.cand, ls.cand, b); AT(s.cell_off, ls.cell_off, b); AT(s.bin_start, ls.bin_start, b);
      AT(s.bin_cnt, ls.bin_cnt, b); AT(s.binid, ls.binid, b); AT(s.s_rank, ls.s_rank, b); AT(s.s_idx, ls.s_idx, b); AT(s.s_uv, ls.s_uv, b);
      AT(s.s_desc, ls.s_desc, b); AT(s.tmp, ls.tmp, b);
      if (k == 1 && heads) AT(s.heads, ls.heads, b);
      else CHECK(s.heads == nullptr && ls.heads.n == 0);
      CHECK((const uint8_t *)s.count_host == hd + L.hm_counts.at + (i * 2 + k) * 4);
      CHECK(s.cap == g.cap_set[k] && s.nms_n == g.nms[k] && s.ncu == g.ncu[k] && s.ncv == g.ncv[k] && ls.feat.n == (size_t)s.cap * 12);
    }
  }
  AT(v.f1, L.f1, b); AT(v.f2, L.f2, b); AT(v.d_ranges, L.ranges, b); AT(v.d_imgs, L.imgs, b); AT(v.d_pairs, L.pairs, b); AT(v.d_jobs, L.jobs, b);
  AT(v.hm_counts, L.hm_counts, hh_); AT(v.hm_lcount, L.hm_lcount, hh_);
  CHECK(L.hm_zeroed == L.hm_lcount.at + al256(L.hm_lcount.n * 4));
  for (size_t j = 0; j < v.h_pairs.size(); j++) {
    const VsmCtxLayout::Pair &l = L.pair[j];
    const VsmPair &pr = v.h_pairs[j];
    AT(pr.raw, l.raw, b); AT(pr.flag, l.flag, b); AT(pr.blockcnt, l.blockcnt, b); AT(pr.list1, l.list1, b); AT(pr.list2, l.list2, b); AT(pr.count, l.count, b);
    AT(pr.keys[0], l.keys[0], b); AT(pr.keys[1], l.keys[1], b); AT(pr.hlist1, l.hlist1, hd); AT(pr.hlist2, l.hlist2, hd);
    AT(v.hm_list1[j], l.hlist1, hh_); AT(v.hm_list2[j], l.hlist2, hh_);
    if (refinement == 2) AT(pr.pf, l.pf, b);
    else CHECK(pr.pf == nullptr && l.pf.n == 0);
    CHECK(pr.ranges == v.d_ranges + j * g.ranges_stride && (const uint8_t *)pr.hcount == hd + L.hm_lcount.at + j * 8);
    CHECK(pr.key_cap[0] == g.cap_set[0] && pr.key_cap[1] == (int32_t)g.qcap);
    if (j > 0) CHECK((const uint8_t *)pr.raw - (const uint8_t *)v.h_pairs[j - 1].raw == (ptrdiff_t)L.pair_stride);
  }
}

static void check_dc2_bind(int npairs, int cap, bool host_ties) {
  const Dc2Layout L(npairs, cap, host_ties);
  std::vector<uint8_t> dev(L.dev.at), host(L.host.at);
  uint8_t *const b = dev.data(), *const hb = host.data();
  for (int i = 0; i < npairs; i++) {
    const Dc2Layout::Pair &l = L.pair[i];
    const Dc2PairPtr q = L.bind(b, i);
    AT(q.keys_in, l.keys_in, b); AT(q.key_sorted, l.key_sorted, b); AT(q.key, l.key, b); AT(q.kd, l.kd, b); AT(q.pt, l.pt, b); AT(q.id, l.id, b);
    AT(q.support, l.support, b); AT(q.remap, l.remap, b); AT(q.tri, l.tri, b); AT(q.mn, l.mn, b); AT(q.hulls, l.hulls, b);
    CHECK(q.out_count == q.mn + 4 && l.mn.n >= 5);
    if (i > 0) CHECK((size_t)((const uint8_t *)q.keys_in - (const uint8_t *)L.bind(b, i - 1).keys_in) == L.pair_stride);
  }
  AT(L.jobs.in(b), L.jobs, b); AT(L.ties.in(b), L.ties, b); AT(L.h_error.in(hb), L.h_error, hb); AT(L.h_n.in(hb), L.h_n, hb);
  CHECK(L.ties_stride == cap + 2 && L.keys_pitch >= (size_t)cap * 8 && L.ties_pitch >= (size_t)L.ties_stride * 4);
  if (host_ties) {
    AT(L.h_keys.in(hb), L.h_keys, hb); AT(L.h_ties.in(hb), L.h_ties, hb);
    CHECK(L.h_keys.n == L.keys_pitch * npairs && L.h_ties.n == L.ties_pitch * npairs && L.h_ties.at + L.h_ties.n == L.host.at);
  } else {
    CHECK(L.h_keys.n == 0 && L.h_ties.n == 0);
  }
}

int main() {
  check_geometry_errors();
  const int32_t shapes[3][2] = {{32, 32}, {304, 128}, {352, 160}};
  for (const auto &s : shapes)
    for (int half = 0; half < 2; half++)
      for (int refinement = 0; refinement < 3; refinement++)
        for (int heads = 0; heads < 2; heads++) {
          check_ctx_bind(s[0], s[1], half, refinement, heads != 0, 2, 1);
          check_ctx_bind(s[0], s[1], half, refinement, heads != 0, 6, 4);
          check_ctx_bind(s[0], s[1], half, refinement, heads != 0, 3, 0);
        }
  for (int cap : {1024, 8192})
    for (int npairs : {1, 3})
      for (int host_ties = 0; host_ties < 2; host_ties++) check_dc2_bind(npairs, cap, host_ties != 0);
  if (fails) return 1;
  printf("ok\n");
  return 0;
}
