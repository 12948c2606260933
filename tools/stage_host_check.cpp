// Stand-alone host check of the block layout the staged calls share (csrc/vsm_stage.h, VsmLayout): the offsets of a handful of
// take() sequences against the 256-alignment arithmetic written out by hand - sizes 0, 1, 255, 256, 257 and a block of
// 5 GB, which a 32-bit offset would not survive.  Then the five stages' blocks (csrc/vsm_layouts.h: tracks, points,
// resection, vetting, joint adjustment): every array's offset, in.at, out.at and the device block's size against the sequence of sizes the
// calls stated by hand before the arrays were typed, for every combination of the counts 0, 1, 5 and 257 and for an
// observation count whose arrays pass 2^31 bytes.  No HIP call is made (the header's staging functions are not
// instantiated here).  Meant to be built with the sanitizers, e.g.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude \
//       -Iopencl-structure-from-motion_amd/csrc tools/stage_host_check.cpp -o stage_host_check
// Prints "ok" and returns 0, or says what differed.
#include <cstdint>
#include <cstdio>

#include "vsm_layouts.h"

static int fails = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); \
      fails++;                                               \
    }                                                        \
  } while (0)

// an array of a stage's blocks lies where the call's next take() of that many bytes put it
#define SAME(arr, lay, bytes) CHECK((arr).at == (lay).take(bytes))

static void check_points(size_t F, size_t T, size_t N) {
  const PtsBlocks L(F, T, N);
  VsmLayout in, out;
  SAME(L.frames, in, F * sizeof(PtsFrame) + 8);
  SAME(L.valid, in, F + 1);
  SAME(L.offsets, in, (T + 1) * 4);
  SAME(L.obs_frames, in, N * 4 + 4);
  SAME(L.uv, in, N * 8 + 8);
  SAME(L.flags, in, T + 1);
  SAME(L.status, out, T * 4 + 4);
  SAME(L.type, out, T * 4 + 4);
  SAME(L.updates, out, T * 4 + 4);
  SAME(L.xyz, out, T * 24 + 8);
  SAME(L.dist, out, T * 8 + 8);
  SAME(L.ray, out, T * 8 + 8);
  CHECK(L.in.at == in.at && L.out.at == out.at && L.out_at == al256(in.at) && L.dev_bytes == al256(in.at) + out.at);
  CHECK(L.frames.n == F && L.uv.n == 2 * N && L.xyz.n == 3 * T && L.status.n == T);
}

static void check_resect(size_t F, size_t T, size_t R) {
  const RsBlocks L(F, T, R);
  VsmLayout in, out;
  SAME(L.poses, in, F * 96 + 8);
  SAME(L.valid, in, F + 1);
  SAME(L.refine, in, F + 1);
  SAME(L.row_off, in, (F + 1) * 4);
  SAME(L.rows, in, R * sizeof(RsRow) + 4);
  SAME(L.xyz, in, T * 24 + 8);
  SAME(L.status, out, F * 4 + 4);
  SAME(L.updates, out, F * 4 + 4);
  SAME(L.used_before, out, F * 4 + 4);
  SAME(L.used, out, F * 4 + 4);
  SAME(L.out_poses, out, F * 96 + 8);
  SAME(L.ss_before, out, F * 8 + 8);
  SAME(L.ss_after, out, F * 8 + 8);
  CHECK(L.in.at == in.at && L.out.at == out.at && L.out_at == al256(in.at) && L.dev_bytes == al256(in.at) + out.at);
  CHECK(L.out_poses.n == 12 * F && L.rows.n == R && L.status.n == F);
}

static void check_vet(size_t F, size_t T, size_t N) {
  const VetBlocks L(F, T, N);
  VsmLayout in, out;
  SAME(L.states, in, F * 96 + 8);
  SAME(L.valid, in, F + 1);
  SAME(L.offsets, in, (T + 1) * 4);
  SAME(L.obs_frames, in, N * 4 + 4);
  SAME(L.uv, in, N * 8 + 8);
  SAME(L.xyz, in, T * 24 + 8);
  SAME(L.use, in, T + 1);
  SAME(L.code, out, N + 1);
  SAME(L.r2, out, N * 4 + 4);
  SAME(L.status, out, T * 4 + 4);
  SAME(L.n_in, out, T * 4 + 4);
  SAME(L.frame_lo, out, T * 4 + 4);
  SAME(L.frame_hi, out, T * 4 + 4);
  SAME(L.ss, out, T * 8 + 8);
  SAME(L.worst, out, T * 8 + 8);
  SAME(L.frame_counts, out, F * 12 + 4);
  SAME(L.kept_offsets, out, (T + 1) * 4);
  SAME(L.kept_index, out, N * 4 + 4);
  SAME(L.totals, out, 8);
  VsmLayout work = out;  // behind the results, not copied back
  SAME(L.scan, work, T * 8 + 8);
  SAME(L.scan_part, work, trk_scan_part_items((int64_t)T) * 8 + 8);
  CHECK(L.in.at == in.at && L.out.at == out.at && L.out_at == al256(in.at) && L.dev_bytes == al256(in.at) + work.at);
  CHECK(L.code.n == N && L.frame_counts.n == 3 * F && L.kept_offsets.n == T + 1 && L.kept_index.n == N);
}

// F frames, T tracks, R rows, N observations, M rounds
static void check_adjust(size_t F, size_t T, size_t R, size_t N, size_t M) {
  const BaBlocks L(F, T, R, N, M);
  VsmLayout in, out;
  SAME(L.poses, in, F * 96 + 8);
  SAME(L.valid, in, F + 1);
  SAME(L.refine, in, F + 1);
  SAME(L.use, in, T + 1);
  SAME(L.row_off, in, (F + 1) * 4);
  SAME(L.rows, in, R * 16 + 16);
  SAME(L.offsets, in, (T + 1) * 4);
  SAME(L.obs_frames, in, N * 4 + 4);
  SAME(L.xyz, in, T * 24 + 8);
  SAME(L.fstatus, out, F * 4 + 4);
  SAME(L.factive, out, F * 4 + 4);
  SAME(L.tstatus, out, T * 4 + 4);
  SAME(L.out_poses, out, F * 96 + 8);
  SAME(L.out_xyz, out, T * 24 + 8);
  SAME(L.hist_d, out, M * 24 + 8);
  SAME(L.hist_i, out, M * 16 + 4);
  SAME(L.ctl, out, sizeof(BaCtl));
  VsmLayout work = out;  // behind the results, not copied back
  SAME(L.state, work, F * 96 + 8);
  SAME(L.trial_state, work, F * 96 + 8);
  SAME(L.trial_X, work, T * 24 + 8);
  SAME(L.active, work, N + 1);
  SAME(L.lin, work, N * 208 + 8);
  SAME(L.usum, work, F * 224 + 8);
  SAME(L.cnt, work, F * 4 + 4);
  SAME(L.ud, work, F * 288 + 8);
  SAME(L.uinv, work, F * 288 + 8);
  SAME(L.vinv, work, T * 72 + 8);
  SAME(L.gp, work, T * 24 + 8);
  SAME(L.zt, work, T * 24 + 8);
  SAME(L.ffree, work, F + 1);
  SAME(L.tfree, work, T + 1);
  SAME(L.moved, work, F + 1);
  SAME(L.cg, work, F * 288 + 8);
  SAME(L.tcost, work, F * 8 + 8);
  SAME(L.tbehind, work, F * 4 + 4);
  CHECK(L.in.at == in.at && L.out.at == out.at && L.out_at == al256(in.at) && L.dev_bytes == al256(in.at) + work.at);
  CHECK(sizeof(BaRow) == 16 && sizeof(BaCtl) == 80 && L.lin.n == 26 * N && L.cg.n == 36 * F && L.hist_d.n == 3 * M && L.ctl.n == 1);
}

// P pairs, F frames, E matches; then N nodes; then the totals the device reports
static void check_tracks(size_t P, size_t F, size_t E, size_t N, size_t n_tracks, size_t n_obs) {
  TrkBlocks L(P, F, E);
  VsmLayout in;
  SAME(L.pair_base, in, (P + 1) * 4);
  SAME(L.pairs, in, P * 8 + 4);
  SAME(L.feat_base, in, (F + 1) * 4);
  SAME(L.edges, in, E * 8 + 4);
  CHECK(L.in.at == in.at);
  L.nodes(N);
  VsmLayout dl = in;
  SAME(L.parent, dl, N * 4);
  SAME(L.first, dl, N * 4);
  SAME(L.size, dl, N * 4);
  SAME(L.cursor, dl, N * 4);
  SAME(L.scan, dl, N * 8);
  SAME(L.scan_part, dl, trk_scan_part_items((int64_t)N) * 8 + 8);
  SAME(L.totals, dl, 8);
  SAME(L.mid_list, dl, (N / (VSM_TRACKS_WAVE_MAX + 1) + 1) * 4);
  const size_t o_out = dl.take(0);
  CHECK(L.in.at == in.at && L.out_at == o_out);
  CHECK(L.dev_bytes == o_out + al256(16) + al256((N + 1) * 4) + al256(N * 16) + al256(E * 4) + al256(N));
  L.results(n_tracks, n_obs);
  VsmLayout ol;
  ol.at = o_out;  // (the call placed the results at their device offsets and took o_out off for the pinned block)
  CHECK(L.counters.at == ol.take(16) - o_out);
  CHECK(L.offsets.at == ol.take((n_tracks + 1) * 4) - o_out);
  CHECK(L.obs.at == ol.take(n_obs * 16) - o_out);
  CHECK(L.track_of_match.at == ol.take(E * 4) - o_out);
  CHECK(L.flags.at == ol.take(n_tracks) - o_out);
  CHECK(L.out.at == ol.at - o_out && L.out_at + L.out.at <= L.dev_bytes);
  CHECK(L.obs.n == 4 * n_obs && L.track_of_match.n == E && L.flags.n == n_tracks);
}

int main() {
  static_assert(sizeof(size_t) == 8, "offsets are 64-bit");
  CHECK(al256(0) == 0 && al256(1) == 256 && al256(255) == 256 && al256(256) == 256 && al256(257) == 512);
  {  // an empty block takes no room; a block of one byte takes a whole line
    VsmLayout l;
    CHECK(l.take(0) == 0 && l.at == 0);
    CHECK(l.take(0) == 0 && l.at == 0);
    CHECK(l.take(1) == 0 && l.at == 256);
    CHECK(l.take(0) == 256 && l.at == 256);
    CHECK(l.take(1) == 256 && l.at == 512);
  }
  {  // on either side of a line
    VsmLayout l;
    CHECK(l.take(255) == 0 && l.at == 256);
    CHECK(l.take(256) == 256 && l.at == 512);
    CHECK(l.take(257) == 512 && l.at == 1024);
    CHECK(l.take(1) == 1024 && l.at == 1280);
  }
  {  // a layout continued from another (the device block behind the uploaded one) and one that starts at a given offset
    VsmLayout in;
    in.take(100);
    in.take(300);
    CHECK(in.at == 256 + 512);
    VsmLayout dev = in;
    CHECK(dev.take(4) == 768 && dev.at == 1024 && in.at == 768);
    VsmLayout out;
    out.at = dev.at;
    CHECK(out.take(16) == 1024 && out.take(257) == 1280 && out.at == 1792);
  }
  {  // 5 GB: 5 * 2^30 = 5368709120 is a multiple of 256; one byte more takes the next line
    const size_t big = (size_t)5 << 30;
    VsmLayout l;
    CHECK(l.take(1) == 0);
    CHECK(l.take(big) == 256 && l.at == 5368709120ull + 256);
    CHECK(l.take(big + 1) == 5368709376ull && l.at == 5368709376ull + 5368709120ull + 256);
    CHECK(l.take(0) == 10737418752ull && l.at == 10737418752ull);
    CHECK(al256(big + 1) == big + 256 && al256(big - 1) == big);
  }
  {  // the stages' blocks
    const size_t counts[4] = {0, 1, 5, 257};
    const size_t big = ((size_t)1 << 29) + 3;  // observations: 4 bytes each pass 2^31, 8 and 16 bytes each pass 2^32
    for (size_t a : counts)
      for (size_t b : counts)
        for (size_t c : counts) {
          check_points(a, b, c);
          check_resect(a, b, c);
          check_vet(a, b, c);
          for (size_t n : counts) check_adjust(a, b, c, c + n, n + 1);
          for (size_t n : counts) check_tracks(a, b, c, n, std::min(n, b), n);
        }
    check_points(5, 257, big);
    check_resect(5, 257, big);
    check_vet(5, 257, big);
    check_adjust(5, 257, big / 2, big, 10);
    check_tracks(5, 257, big, big, 257, big);
  }
  if (fails) return 1;
  printf("ok\n");
  return 0;
}
