// The blocks of the staged calls: per stage one struct that declares every array once - its element
// type - and places it once - its count and the spare bytes behind it -, as a pure function of the call's counts.  No HIP
// call is made here, so tools/stage_host_check.cpp checks the offsets on the CPU.  vsm_stage.h has the arrays' views.  The
// joint adjustment's blocks also write their uploaded block (pack) and assign BaData (bind), for the device path and the host
// view alike.  Last comes the bank of a Delaunay chain of the look-ahead forms (Dc2Layout), stated the same way; a context's
// blocks are vsm_ctx.h.
#pragma once

#include "vsm_dc_gpu.h"
#include "vsm_stage.h"
#include "vsm_tracks.h"
#include "vsm_points.h"
#include "vsm_resect.h"
#include "vsm_vet.h"
#include "vsm_ba.h"
#include "vsm_locate.h"
#include "vsm_reobserve.h"
#include "vsm_fuse.h"

// vsm_points.inc: F frames, T tracks, N observations
struct PtsBlocks : VsmBlocks {
  VsmIn<PtsFrame> frames;
  VsmIn<uint8_t> valid, flags;
  VsmIn<int32_t> offsets, obs_frames;
  VsmIn<float> uv;
  VsmOut<int32_t> status, type, updates;
  VsmOut<double> xyz, dist, ray;
  PtsBlocks(size_t F, size_t T, size_t N) {
    frames.place(in, F, 8); valid.place(in, F, 1); offsets.place(in, T + 1, 0); obs_frames.place(in, N, 4); uv.place(in, 2 * N, 8); flags.place(in, T, 1);
    status.place(out, T, 4); type.place(out, T, 4); updates.place(out, T, 4); xyz.place(out, 3 * T, 8); dist.place(out, T, 8); ray.place(out, T, 8);
    out_behind_in(out.at);
  }
};

// vsm_resect.inc: F frames, T tracks, R rows (the observations of the tracks in use)
struct RsBlocks : VsmBlocks {
  VsmIn<double> poses, xyz;
  VsmIn<uint8_t> valid, refine;
  VsmIn<int32_t> row_off;
  VsmIn<RsRow> rows;
  VsmOut<int32_t> status, updates, used_before, used;
  VsmOut<double> out_poses, ss_before, ss_after;
  RsBlocks(size_t F, size_t T, size_t R) {
    poses.place(in, 12 * F, 8); valid.place(in, F, 1); refine.place(in, F, 1); row_off.place(in, F + 1, 0); rows.place(in, R, 4); xyz.place(in, 3 * T, 8);
    status.place(out, F, 4); updates.place(out, F, 4); used_before.place(out, F, 4); used.place(out, F, 4); out_poses.place(out, 12 * F, 8);
    ss_before.place(out, F, 8); ss_after.place(out, F, 8);
    out_behind_in(out.at);
  }
};

// vsm_vet.inc: F frames, T tracks, N observations; the scan's working set lies behind the results and is not copied back
struct VetBlocks : VsmBlocks {
  VsmIn<double> states, xyz;
  VsmIn<uint8_t> valid, use;
  VsmIn<int32_t> offsets, obs_frames;
  VsmIn<float> uv;
  VsmOut<uint8_t> code;
  VsmOut<float> r2;
  VsmOut<int32_t> status, n_in, frame_lo, frame_hi, frame_counts, kept_offsets, kept_index, totals, scan, scan_part;
  VsmOut<double> ss, worst;
  VetBlocks(size_t F, size_t T, size_t N) {
    states.place(in, 12 * F, 8); valid.place(in, F, 1); offsets.place(in, T + 1, 0); obs_frames.place(in, N, 4); uv.place(in, 2 * N, 8); xyz.place(in, 3 * T, 8);
    use.place(in, T, 1);
    code.place(out, N, 1); r2.place(out, N, 4); status.place(out, T, 4); n_in.place(out, T, 4); frame_lo.place(out, T, 4); frame_hi.place(out, T, 4);
    ss.place(out, T, 8); worst.place(out, T, 8); frame_counts.place(out, 3 * F, 4); kept_offsets.place(out, T + 1, 0); kept_index.place(out, N, 4);
    totals.place(out, 2, 0);
    VsmLayout work = out;
    scan.place(work, 2 * T, 8); scan_part.place(work, 2 * trk_scan_part_items((int64_t)T), 8);
    out_behind_in(work.at);
  }
};

// vsm_ba.inc: F frames, T tracks, R rows, N observations, M rounds at the most; the state, the round's linearisation and the
// conjugate gradient's vectors lie behind the results and are not copied back
struct BaBlocks : VsmBlocks {
  VsmIn<double> poses, xyz;
  VsmIn<uint8_t> valid, refine, use;
  VsmIn<int32_t> row_off, offsets, obs_frames;
  VsmIn<BaRow> rows;
  VsmOut<int32_t> fstatus, factive, tstatus, hist_i, cnt, tbehind;
  VsmOut<double> out_poses, out_xyz, hist_d, state, trial_state, trial_X, lin, usum, ud, uinv, vinv, gp, zt, cg, tcost;
  VsmOut<uint8_t> active, ffree, tfree, moved;
  VsmOut<BaCtl> ctl;
  BaBlocks(size_t F, size_t T, size_t R, size_t N, size_t M) {
    poses.place(in, 12 * F, 8); valid.place(in, F, 1); refine.place(in, F, 1); use.place(in, T, 1); row_off.place(in, F + 1, 0); rows.place(in, R, 16);
    offsets.place(in, T + 1, 0); obs_frames.place(in, N, 4); xyz.place(in, 3 * T, 8);
    fstatus.place(out, F, 4); factive.place(out, F, 4); tstatus.place(out, T, 4); out_poses.place(out, 12 * F, 8); out_xyz.place(out, 3 * T, 8);
    hist_d.place(out, 3 * M, 8); hist_i.place(out, 4 * M, 4); ctl.place(out, 1, 0);
    VsmLayout work = out;
    state.place(work, 12 * F, 8); trial_state.place(work, 12 * F, 8); trial_X.place(work, 3 * T, 8); active.place(work, N, 1); lin.place(work, BA_LIN * N, 8);
    usum.place(work, RS_SUMS * F, 8); cnt.place(work, F, 4); ud.place(work, 36 * F, 8); uinv.place(work, 36 * F, 8); vinv.place(work, 9 * T, 8); gp.place(work, 3 * T, 8); zt.place(work, 3 * T, 8);
    ffree.place(work, F, 1); tfree.place(work, T, 1); moved.place(work, F, 1); cg.place(work, 36 * F, 8); tcost.place(work, F, 8); tbehind.place(work, F, 4);
    out_behind_in(work.at);
  }
  // The uploaded block written at `block` (the pinned input; the host view's buffer).  G is the grouping whose counts sized
  // this layout (RsGroup, vsm_resect.h): it has the tracks, their use mask and the observation source, and fills the rows.
  template <class Group>
  void pack(uint8_t *block, const double *poses_, const uint8_t *pose_valid, const uint8_t *refine_, Group &G, const double *xyz_) const {
    const size_t F = valid.n, T = use.n;
    if (F > 0) memcpy(poses.in(block), poses_, F * 96);
    vsm_mask_bytes(pose_valid, F, valid.in(block)); vsm_mask_bytes(refine_, F, refine.in(block)); vsm_mask_bytes(G.use, T, use.in(block));
    memcpy(row_off.in(block), G.row_off.data(), (F + 1) * 4);
    G.fill(rows.in(block));
    offsets.in(block)[0] = 0;
    if (T > 0) memcpy(offsets.in(block), G.offsets, (T + 1) * 4), memcpy(xyz.in(block), xyz_, T * 24);
    for (size_t i = 0; i < obs_frames.n; i++) obs_frames.in(block)[i] = G.obs.frame_of((int32_t)i);
  }
  // BaData, assigned here and nowhere else: the uploaded arrays in the block at in_block, the results and the working set
  // in the block at out_block (the device path: S.dev and S.dev + out_at; the host view: the same two places of its buffer)
  BaData bind(uint8_t *in_block, uint8_t *out_block, double f, double cu, double cv, const vsm_adjust_params &prm) const {
    uint8_t *const i = in_block, *const o = out_block;
    const size_t F6 = cg.n / 6;
    BaData d;
    memset(&d, 0, sizeof(d));
    d.poses = poses.in(i); d.valid = valid.in(i); d.refine = refine.in(i); d.use = use.in(i); d.row_off = row_off.in(i); d.rows = rows.in(i);
    d.offsets = offsets.in(i); d.obs_frames = obs_frames.in(i); d.xyz_in = xyz.in(i);
    d.state = state.in(o); d.trial_state = trial_state.in(o); d.trial_X = trial_X.in(o); d.active = active.in(o); d.lin = lin.in(o); d.usum = usum.in(o);
    d.cnt = cnt.in(o); d.ud = ud.in(o); d.uinv = uinv.in(o); d.vinv = vinv.in(o); d.gp = gp.in(o); d.zt = zt.in(o);
    d.ffree = ffree.in(o); d.tfree = tfree.in(o); d.moved = moved.in(o); d.tcost = tcost.in(o); d.tbehind = tbehind.in(o); d.ctl = ctl.in(o);
    d.b = cg.in(o); d.x = d.b + F6; d.r = d.x + F6; d.z = d.r + F6; d.p = d.z + F6; d.q = d.p + F6;
    d.fstatus = fstatus.in(o); d.factive = factive.in(o); d.tstatus = tstatus.in(o); d.out_poses = out_poses.in(o); d.out_xyz = out_xyz.in(o);
    d.hist_d = hist_d.in(o); d.hist_i = hist_i.in(o);
    d.f = f; d.cu = cu; d.cv = cv; d.prm = prm; d.n_frames = (int32_t)valid.n; d.n_tracks = (int32_t)use.n;
    return d;
  }
};

// vsm_locate.inc: F frames, T tracks, R rows, J jobs (frames with hypotheses, at the most), K hypotheses per job, NT tiles of
// 256 rows (at the most); the hypotheses' states, validity and counts and the refinement's mask lie behind the results and
// are not copied back.  The resection's kernel refines in place: its inputs are lin_poses and lin_valid, its results rs_*.
struct LcBlocks : VsmBlocks {
  VsmIn<int32_t> row_off, frame_job, job_frame, job_E, picks;
  VsmIn<RsRow> rows;
  VsmIn<double> xyz;
  VsmIn<LcTile> tiles;
  VsmOut<int32_t> verdict, best, inliers, rs_status, rs_updates, rs_used_before, rs_used, counts;
  VsmOut<double> lin_poses, rs_poses, rs_ss_before, rs_ss_after, states;
  VsmOut<uint8_t> hvalid, lin_valid;
  LcBlocks(size_t F, size_t T, size_t R, size_t J, size_t K, size_t NT) {
    row_off.place(in, F + 1, 0); frame_job.place(in, F, 4); job_frame.place(in, J, 4); job_E.place(in, J, 4); rows.place(in, R, 4); xyz.place(in, 3 * T, 8);
    tiles.place(in, NT, 8); picks.place(in, J * K * LC_SAMPLE, 4);
    verdict.place(out, F, 4); best.place(out, F, 4); inliers.place(out, F, 4); lin_poses.place(out, 12 * F, 8); rs_status.place(out, F, 4);
    rs_updates.place(out, F, 4); rs_used_before.place(out, F, 4); rs_used.place(out, F, 4); rs_poses.place(out, 12 * F, 8); rs_ss_before.place(out, F, 8);
    rs_ss_after.place(out, F, 8);
    VsmLayout work = out;
    states.place(work, J * K * 12, 8); counts.place(work, J * K, 4); hvalid.place(work, J * K, 1); lin_valid.place(work, F, 1);
    out_behind_in(work.at);
  }
};

// vsm_reobserve.inc: F frames, T tracks, N observations, NF features of which NU are uploaded (the general form: all; the
// handle form: none, they are resident), B bins per frame.  The results here are those sized before the launch; the working
// set lies behind them and is not copied back - first what starts at zero (the occupied bytes, the bins), then the rest.
// The candidates have a block of their own (RoCandBlocks), sized once their number is back.
struct RoBlocks : VsmBlocks {
  VsmIn<double> states, xyz;
  VsmIn<uint8_t> valid, search, use;
  VsmIn<int32_t> offsets, obs_frames, obs_feat, ref_obs, feat_offsets, feat;
  VsmIn<const int32_t *> frame_feat;
  VsmOut<int32_t> track_accepted, frame_counts, totals, bins, bins_part, bins_total, sorted, scan, scan_part;
  VsmOut<unsigned long long> stats, claim;
  VsmOut<uint8_t> occupied;
  size_t zero_bytes = 0;  // from `occupied` on
  RoBlocks(size_t F, size_t T, size_t N, size_t NF, size_t NU, size_t B) {
    states.place(in, 12 * F, 8); valid.place(in, F, 1); search.place(in, F, 1); offsets.place(in, T + 1, 0); obs_frames.place(in, N, 4); obs_feat.place(in, N, 4);
    xyz.place(in, 3 * T, 8); use.place(in, T, 1); ref_obs.place(in, T, 4); feat_offsets.place(in, F + 1, 0); frame_feat.place(in, F, 8); feat.place(in, RO_FEAT_INTS * NU, 16);
    track_accepted.place(out, T, 4); frame_counts.place(out, 2 * F, 4); stats.place(out, RO_STATS, 0); totals.place(out, 2, 0);
    VsmLayout work = out;
    occupied.place(work, NF, 1); bins.place(work, 2 * F * B, 8);
    zero_bytes = work.at - occupied.at;
    bins_part.place(work, 2 * trk_scan_part_items((int64_t)(F * B)), 8); bins_total.place(work, 2, 0); claim.place(work, NF, 8); sorted.place(work, RO_FEAT_INTS * NF, 16);
    scan.place(work, 2 * T, 8); scan_part.place(work, 2 * trk_scan_part_items((int64_t)T), 8);
    out_behind_in(work.at);
  }
};
struct RoCandBlocks : VsmBlocks {
  VsmOut<int32_t> cand;
  VsmOut<double> uv;
  explicit RoCandBlocks(size_t n) {
    cand.place(out, RO_CAND_INTS * n, 4); uv.place(out, 2 * n, 8);
    out_behind_in(out.at);  // (in is empty: the block is the results)
  }
};

// vsm_fuse.inc: the counts of RoBlocks.  The results sized before the launch - the tracks' partners, the merged set, the
// frames' counts, the stats - are copied back; the working set lies behind them - first what starts at zero (the bins), then
// the rest.  The proposals have a block of their own (FuPropBlocks), sized once their number is back.
struct FuBlocks : VsmBlocks {
  VsmIn<double> states, xyz;
  VsmIn<uint8_t> valid, search, use;
  VsmIn<int32_t> offsets, obs_frames, obs_feat, ref_obs, use_rank, feat_offsets, feat;
  VsmIn<const int32_t *> frame_feat;
  VsmOut<int32_t> partner, fused_into, offsets_after, obs_src, frame_counts, totals, bins, bins_part, bins_total, sorted, scan, scan_part;
  VsmOut<unsigned long long> stats, choice;
  VsmOut<uint32_t> owner;
  size_t ones_bytes = 0;  // from `partner` on: what starts at all bits set (no partner, no survivor)
  FuBlocks(size_t F, size_t T, size_t N, size_t NF, size_t NU, size_t B) {
    states.place(in, 12 * F, 8); valid.place(in, F, 1); search.place(in, F, 1); offsets.place(in, T + 1, 0); obs_frames.place(in, N, 4); obs_feat.place(in, N, 4);
    xyz.place(in, 3 * T, 8); use.place(in, T, 1); ref_obs.place(in, T, 4); use_rank.place(in, T, 4); feat_offsets.place(in, F + 1, 0); frame_feat.place(in, F, 8);
    feat.place(in, RO_FEAT_INTS * NU, 16);
    partner.place(out, T, 4); fused_into.place(out, T, 4);
    ones_bytes = out.at;
    offsets_after.place(out, T + 1, 0); obs_src.place(out, N, 4); frame_counts.place(out, 2 * F, 4); stats.place(out, FU_STATS, 0); totals.place(out, 2, 0);
    VsmLayout work = out;
    bins.place(work, 2 * F * B, 8); bins_part.place(work, 2 * trk_scan_part_items((int64_t)(F * B)), 8); bins_total.place(work, 2, 0); owner.place(work, NF, 4);
    choice.place(work, T, 8); sorted.place(work, RO_FEAT_INTS * NF, 16); scan.place(work, 2 * T, 8); scan_part.place(work, 2 * trk_scan_part_items((int64_t)T), 8);
    out_behind_in(work.at);
  }
};
// the compacting form's places: U tracks in use, S frames searched with a pose
struct FuSlotBlocks : VsmBlocks {
  VsmOut<int32_t> slots;
  VsmOut<double> uv;
  FuSlotBlocks(size_t U, size_t S) {
    slots.place(out, FU_PROP_INTS * U * S, 4); uv.place(out, 2 * U * S, 8);
    out_behind_in(out.at);
  }
};
struct FuPropBlocks : VsmBlocks {
  VsmOut<int32_t> prop;
  VsmOut<double> uv;
  explicit FuPropBlocks(size_t n) {
    prop.place(out, FU_PROP_INTS * n, 4); uv.place(out, 2 * n, 8);
    out_behind_in(out.at);  // (in is empty: the block is the results)
  }
};

// vsm_tracks.inc, in the three steps of the call: the uploaded block from the arguments' counts; the working set per node
// behind it and the results' upper bounds (every node an observation, every node a track) once the packing has counted the
// nodes; the results themselves once the totals are back.
struct TrkBlocks : VsmBlocks {
  VsmIn<int32_t> pair_base, pairs, feat_base, edges;
  VsmDev<int32_t> parent, first, size, cursor, scan, scan_part, totals, mid_list;
  VsmOut<int32_t> counters, offsets, obs, track_of_match;
  VsmOut<uint8_t> flags;
  size_t n_edges;
  TrkBlocks(size_t P, size_t F, size_t E) : n_edges(E) { pair_base.place(in, P + 1, 0); pairs.place(in, 2 * P, 4); feat_base.place(in, F + 1, 0); edges.place(in, 2 * E, 4); }
  void nodes(size_t N) {
    VsmLayout dl = in;
    parent.place(dl, N, 0); first.place(dl, N, 0); size.place(dl, N, 0); cursor.place(dl, N, 0); scan.place(dl, 2 * N, 0);
    scan_part.place(dl, 2 * trk_scan_part_items((int64_t)N), 8); totals.place(dl, 2, 0); mid_list.place(dl, N / (VSM_TRACKS_WAVE_MAX + 1) + 1, 0);
    out_at = dl.at;
    dev_bytes = out_at + al256(16) + al256((N + 1) * 4) + al256(N * 16) + al256(n_edges * 4) + al256(N);
    results(0, 0);  // (the counters are in place for the first launch; the rest moves when the totals are back)
  }
  void results(size_t n_tracks, size_t n_obs) {
    out = VsmLayout();
    counters.place(out, 4, 0); offsets.place(out, n_tracks + 1, 0); obs.place(out, 4 * n_obs, 0); track_of_match.place(out, n_edges, 0); flags.place(out, n_tracks, 0);
  }
};

// one pair's device arrays of a chain's bank
struct Dc2PairPtr {
  uint64_t *keys_in, *key_sorted, *key;
  uint32_t *kd, *pt;
  int32_t *id, *tri, *mn, *support, *remap, *out_count;
  VsmDcHull *hulls;
};
// The blocks of a Delaunay chain's bank (Dc2Bank) of npairs lists of up to cap matches: the device block - per pair the
// chain's arrays, then the job table and the tie verdicts of k_dc2_ties [npairs][VSM_DC_TIE_OUT_INTS] - and the host-mapped
// block - error words, list lengths and, with host_ties, per pair the keys the pool sorts and the patches it answers with.
// The CPU suite pins it through vsm_debug_dc2_layout (tests/test_ctx_layout_cpu.py), tools/ctx_host_check.cpp checks bind().
struct Dc2Layout {
  struct Pair {
    VsmArray<uint64_t> keys_in, key_sorted, key;
    VsmArray<uint32_t> kd, pt;
    VsmArray<int32_t> id, support, remap, tri, mn;
    VsmArray<VsmDcHull> hulls;
  };
  std::vector<Pair> pair;
  VsmArray<VsmDc2Job> jobs;
  VsmArray<int32_t> ties, h_error, h_n;
  VsmArray<uint8_t> h_keys, h_ties;  // [npairs] rows of keys_pitch / ties_pitch bytes
  VsmPlacer dev, host;               // dev.at / host.at: the blocks' sizes
  const int ties_stride;             // ints of a pair's patches: the count, then (carried, right) pairs
  const size_t keys_pitch, ties_pitch;
  size_t pair_stride = 0;  // bytes from one pair's device arrays to the next pair's

  Dc2Layout(int npairs, int cap, bool host_ties)
      : pair((size_t)npairs), ties_stride(cap + 2), keys_pitch(al256((size_t)cap * 8)), ties_pitch(al256((size_t)ties_stride * 4)) {
    const size_t c = (size_t)cap;
    for (int i = 0; i < npairs; i++) {
      Pair &q = pair[i];
      dev.put(q.keys_in, "keys_in", i, -1, c); dev.put(q.key_sorted, "key_sorted", i, -1, c); dev.put(q.key, "key", i, -1, c); dev.put(q.kd, "kd", i, -1, c * VSM_DC_KD_SCRATCH);
      dev.put(q.pt, "pt", i, -1, c); dev.put(q.id, "id", i, -1, c); dev.put(q.support, "support", i, -1, c); dev.put(q.remap, "remap", i, -1, c); dev.put(q.tri, "tri", i, -1, c * 16);
      dev.put(q.mn, "mn", i, -1, 16); dev.put(q.hulls, "hulls", i, -1, (size_t)2 << VSM_DC2_MAX_DEPTH);
      pair_stride = dev.at - q.keys_in.at;
    }
    dev.put(jobs, "jobs", -1, -1, (size_t)npairs); dev.put(ties, "ties", -1, -1, (size_t)npairs * VSM_DC_TIE_OUT_INTS);
    host.put(h_error, "h_error", -1, -1, 16); host.put(h_n, "h_n", -1, -1, (size_t)npairs);
    if (host_ties) host.put(h_keys, "h_keys", -1, -1, keys_pitch * npairs), host.put(h_ties, "h_ties", -1, -1, ties_pitch * npairs);
  }
  Dc2PairPtr bind(uint8_t *b, int i) const {  // (out_count lies in the pair's mn)
    const Pair &q = pair[i];
    return {q.keys_in.in(b), q.key_sorted.in(b), q.key.in(b), q.kd.in(b), q.pt.in(b), q.id.in(b), q.tri.in(b), q.mn.in(b), q.support.in(b), q.remap.in(b), q.mn.in(b) + 4, q.hulls.in(b)};
  }
};
