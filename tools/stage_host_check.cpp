// Stand-alone host check of the block layout the staged calls share (csrc/vsm_stage.h, VsmLayout): the offsets of a handful of
// take() sequences against the 256-alignment arithmetic written out by hand - sizes 0, 1, 255, 256, 257 and a block of
// 5 GB, which a 32-bit offset would not survive.  Then the five stages' blocks (csrc/vsm_layouts.h: tracks, points,
// resection, vetting, joint adjustment): every array's offset, in.at, out.at and the device block's size against the sequence of sizes the
// calls stated by hand before the arrays were typed, for every combination of the counts 0, 1, 5 and 257 and for an
// observation count whose arrays pass 2^31 bytes.  Then what the two refinement stages share in front of their kernels: the
// rows by frame (csrc/vsm_resect.h, RsGroup) at 1, 2, 3, 7 and 32 chunks, visited in reverse order, against one chunk, for
// both row types, and the joint adjustment's bound pointers (BaBlocks::bind) against the arrays' offsets.  No HIP call is
// made (the header's staging functions are not instantiated here).  Meant to be built with the sanitizers, e.g.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude \
//       -Iopencl-structure-from-motion_amd/csrc tools/stage_host_check.cpp -o stage_host_check
// Prints "ok" and returns 0, or says what differed.
#include <cstdint>
#include <cstdio>
#include <cstring>

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

// F frames, T tracks, R rows, J jobs, K hypotheses per job, NT tiles
static void check_locate(size_t F, size_t T, size_t R, size_t J, size_t K, size_t NT) {
  const LcBlocks L(F, T, R, J, K, NT);
  VsmLayout in, out;
  SAME(L.row_off, in, (F + 1) * 4);
  SAME(L.frame_job, in, F * 4 + 4);
  SAME(L.job_frame, in, J * 4 + 4);
  SAME(L.job_E, in, J * 4 + 4);
  SAME(L.rows, in, R * sizeof(RsRow) + 4);
  SAME(L.xyz, in, T * 24 + 8);
  SAME(L.tiles, in, NT * 8 + 8);
  SAME(L.picks, in, J * K * 24 + 4);
  SAME(L.verdict, out, F * 4 + 4);
  SAME(L.best, out, F * 4 + 4);
  SAME(L.inliers, out, F * 4 + 4);
  SAME(L.lin_poses, out, F * 96 + 8);
  SAME(L.rs_status, out, F * 4 + 4);
  SAME(L.rs_updates, out, F * 4 + 4);
  SAME(L.rs_used_before, out, F * 4 + 4);
  SAME(L.rs_used, out, F * 4 + 4);
  SAME(L.rs_poses, out, F * 96 + 8);
  SAME(L.rs_ss_before, out, F * 8 + 8);
  SAME(L.rs_ss_after, out, F * 8 + 8);
  VsmLayout work = out;  // behind the results, not copied back
  SAME(L.states, work, J * K * 96 + 8);
  SAME(L.counts, work, J * K * 4 + 4);
  SAME(L.hvalid, work, J * K + 1);
  SAME(L.lin_valid, work, F + 1);
  CHECK(L.in.at == in.at && L.out.at == out.at && L.out_at == al256(in.at) && L.dev_bytes == al256(in.at) + work.at);
  CHECK(sizeof(LcTile) == 8 && L.picks.n == 6 * J * K && L.states.n == 12 * J * K && L.lin_poses.n == 12 * F && L.tiles.n == NT);
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

// the chunks last to first: no chunk may depend on another having run
struct ReverseRun {
  template <class Fn>
  void operator()(int n, Fn fn) const {
    for (int c = n - 1; c >= 0; c--) fn(c);
  }
};

// a track set as the calls take it: lengths, every observation's frame below F, a use mask (or none)
struct GroupCase {
  int32_t F = 0;
  std::vector<int32_t> offsets{0}, frames;
  std::vector<float> uv;
  std::vector<uint8_t> use;
  bool masked = false;
  void track(int32_t length, int32_t first_frame, int32_t frame_step) {
    for (int32_t k = 0; k < length; k++) {
      const int32_t i = (int32_t)frames.size();
      frames.push_back((first_frame + k * frame_step) % F);
      uv.push_back(0.5f * (float)i);
      uv.push_back(-0.25f * (float)i);
    }
    offsets.push_back((int32_t)frames.size());
  }
  // drops the first track, the last track and every third
  void mask() {
    const size_t T = offsets.size() - 1;
    use.assign(T + 1, 1);
    for (size_t t = 0; t < T; t++)
      if (t == 0 || t + 1 == T || t % 3 == 2) use[t] = 0;
    masked = true;
  }
};

template <class Row>
static void group_rows(const GroupCase &c, int chunks, bool reverse, std::vector<int32_t> &row_off, std::vector<Row> &rows) {
  const int32_t T = (int32_t)c.offsets.size() - 1;
  const RsObsArrays obs{c.frames.data(), c.uv.data()};
  std::vector<int32_t> at;
  rows.clear();
  auto both = [&](auto &G) {  // the two phases, the rows sized in between as the calls size their block
    row_off = G.row_off;
    rows.resize((size_t)row_off[c.F] + 1);
    memset((void *)rows.data(), 0xee, rows.size() * sizeof(Row));
    G.fill(rows.data());
  };
  // (no track: the calls pass the caller's offsets, which may be null)
  if (reverse) {
    RsGroup G(c.F, T, T > 0 ? c.offsets.data() : nullptr, c.masked ? c.use.data() : nullptr, obs, chunks, ReverseRun(), at);
    both(G);
  } else {
    RsGroup G(c.F, T, T > 0 ? c.offsets.data() : nullptr, c.masked ? c.use.data() : nullptr, obs, chunks, RsLoop(), at);
    both(G);
  }
}

static int32_t row_obs(const RsRow &, int32_t fallback) { return fallback; }
static int32_t row_obs(const BaRow &r, int32_t) { return r.obs; }

template <class Row>
static void check_group_case(const GroupCase &c) {
  std::vector<int32_t> want_off, got_off;
  std::vector<Row> want, got;
  group_rows(c, 1, false, want_off, want);
  const int32_t T = (int32_t)c.offsets.size() - 1;
  // the one-chunk result itself: every observation of a track in use once, ascending (track, observation) within a frame
  CHECK((int32_t)want_off.size() == c.F + 1 && want_off[0] == 0);
  int64_t in_use = 0;
  for (int32_t t = 0; t < T; t++)
    if (!c.masked || c.use[t]) in_use += c.offsets[t + 1] - c.offsets[t];
  CHECK(want_off[c.F] == in_use);
  for (int32_t g = 0; g < c.F; g++) {
    int64_t last = -1;  // (a track's observations of one frame ascend with their index)
    for (int32_t k = want_off[g]; k < want_off[g + 1]; k++) {
      const Row &r = want[k];
      CHECK(r.track >= 0 && r.track < T && (!c.masked || c.use[r.track]));
      if (!(r.track >= 0 && r.track < T)) continue;
      // the observation: BaRow names it; RsRow's is found by its pixel, which the case made unique
      int32_t i = row_obs(r, -1);
      if (i < 0)
        for (int32_t j = c.offsets[r.track]; j < c.offsets[r.track + 1]; j++)
          if (c.uv[2 * (size_t)j] == r.u) i = j;
      CHECK(i >= c.offsets[r.track] && i < c.offsets[r.track + 1]);
      if (!(i >= c.offsets[r.track] && i < c.offsets[r.track + 1])) continue;
      CHECK(c.frames[i] == g && r.u == c.uv[2 * (size_t)i] && r.v == c.uv[2 * (size_t)i + 1]);
      const int64_t key = (int64_t)r.track * ((int64_t)c.frames.size() + 1) + i;
      CHECK(key > last);
      last = key;
    }
  }
  for (int chunks : {1, 2, 3, 7, 32}) {
    group_rows(c, chunks, true, got_off, got);
    CHECK(got_off == want_off);
    CHECK(got.size() == want.size() && memcmp((const void *)got.data(), (const void *)want.data(), want.size() * sizeof(Row)) == 0);
  }
}

static void check_grouping() {
  std::vector<GroupCase> cases;
  for (int masked = 0; masked < 2; masked++) {
    GroupCase none;  // T = 0, with frames
    none.F = 3;
    cases.push_back(none);
    GroupCase empty;  // F = 0: tracks can have no observation
    for (int t = 0; t < 4; t++) empty.track(0, 0, 0);
    cases.push_back(empty);
    GroupCase few;  // fewer tracks than chunks: empty chunks; frame 4 is named by nothing
    few.F = 5;
    few.track(33, 0, 1), few.track(1, 2, 0), few.track(0, 0, 0), few.track(4, 1, 1), few.track(2, 3, 0);
    for (int32_t &g : few.frames)
      if (g == 4) g = 0;
    cases.push_back(few);
    GroupCase many;  // more tracks than chunks, lengths 0, 1, 33 and others, frame 6 of 7 unnamed
    many.F = 7;
    for (int t = 0; t < 75; t++) many.track(t % 5 == 0 ? 0 : t % 5 == 1 ? 1 : t % 5 == 2 ? 33 : t % 7, t % 6, 1 + t % 3);
    for (int32_t &g : many.frames)
      if (g == 6) g = 2;
    cases.push_back(many);
    if (masked)
      for (size_t k = cases.size() - 4; k < cases.size(); k++) cases[k].mask();
  }
  for (const GroupCase &c : cases) {
    check_group_case<RsRow>(c);
    check_group_case<BaRow>(c);
  }
}

// every pointer of the bound BaData is its array's offset behind its block's base; the six vectors are cut out of cg
static void check_bind(size_t F, size_t T, size_t R, size_t N, size_t M) {
  const BaBlocks L(F, T, R, N, M);
  std::vector<uint8_t> block(L.dev_bytes + 1);  // as the host view binds: one buffer, the results at out_at
  uint8_t *const i = block.data(), *const o = block.data() + L.out_at;
  vsm_adjust_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.max_rounds = (int32_t)M;
  const BaData d = L.bind(i, o, 1.5, 2.5, 3.5, prm);
#define AT(member, arr, base) CHECK((const uint8_t *)d.member == (base) + L.arr.at)
  AT(poses, poses, i); AT(valid, valid, i); AT(refine, refine, i); AT(use, use, i); AT(row_off, row_off, i); AT(rows, rows, i);
  AT(offsets, offsets, i); AT(obs_frames, obs_frames, i); AT(xyz_in, xyz, i);
  AT(state, state, o); AT(trial_state, trial_state, o); AT(trial_X, trial_X, o); AT(active, active, o); AT(lin, lin, o); AT(usum, usum, o);
  AT(cnt, cnt, o); AT(ud, ud, o); AT(uinv, uinv, o); AT(vinv, vinv, o); AT(gp, gp, o); AT(zt, zt, o); AT(ffree, ffree, o); AT(tfree, tfree, o);
  AT(moved, moved, o); AT(b, cg, o); AT(tcost, tcost, o); AT(tbehind, tbehind, o); AT(ctl, ctl, o);
  AT(fstatus, fstatus, o); AT(factive, factive, o); AT(tstatus, tstatus, o); AT(out_poses, out_poses, o); AT(out_xyz, out_xyz, o);
  AT(hist_d, hist_d, o); AT(hist_i, hist_i, o);
#undef AT
  const ptrdiff_t f6 = (ptrdiff_t)(6 * F);
  CHECK(d.x - d.b == f6 && d.r - d.x == f6 && d.z - d.r == f6 && d.p - d.z == f6 && d.q - d.p == f6);
  CHECK((const uint8_t *)(d.q + f6) == o + L.cg.at + L.cg.n * 8);
  CHECK(d.f == 1.5 && d.cu == 2.5 && d.cv == 3.5 && d.prm.max_rounds == (int32_t)M && d.n_frames == (int32_t)F && d.n_tracks == (int32_t)T);
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
          for (size_t n : counts) check_bind(a, b, c, c + n, n + 1);
          for (size_t n : counts) check_tracks(a, b, c, n, std::min(n, b), n);
          for (size_t n : counts) check_locate(a, b, c, std::min(a, n), n + 1, c / 256 + n);
        }
    check_locate(5, 257, big, 5, 200, big / 256 + 5);
    check_locate(1 << 20, 257, 5, 1 << 20, 4096, 5);  // the hypotheses' states pass 2^38 bytes
    check_points(5, 257, big);
    check_resect(5, 257, big);
    check_vet(5, 257, big);
    check_adjust(5, 257, big / 2, big, 10);
    check_tracks(5, 257, big, big, 257, big);
  }
  check_grouping();
  if (fails) return 1;
  printf("ok\n");
  return 0;
}
