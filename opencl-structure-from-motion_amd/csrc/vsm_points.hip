// Track triangulation on the device (vsm_points.h has the mathematics, vsm_points.inc the host side).
//
// A 16-lane group per track, four tracks per wave, sixteen per 256-thread workgroup; everything a group shares lives in
// LDS.  The 4x4 SVD of initPoint is vsm_la::svd_group (the lanes share its column / row loops); in an update lane i of the
// group computes the Jacobian rows of observation 16 * c + i for chunk after chunk c of sixteen observations, and lane s < 12
// walks sum s of the normal equations over the chunk in ascending order, keeping its running sum in a register from chunk
// to chunk - so every sum adds its terms in the order of vsm_points.h whatever the track's length.  Lane 0 solves the 3x3
// system in LDS; the cheap scalar steps (type, step, distance, ray) are evaluated redundantly by every lane: same operands,
// same order, same bits.
// The groups of a wave diverge on status and on the number of updates.  All control flow below is uniform inside a group,
// the only synchronisation is VSM_GROUP_SYNC (a fence for the compiler: a wave executes its LDS instructions in order), and
// there is no workgroup barrier anywhere - so a group that is done simply leaves, as in k_mono_fit.
#include "vsm_internal.h"
#include "vsm_points.h"
#include "vsm_svd_coop.h"

namespace {

// per group: the spare doubles, U 16 + V 16 + W 4 + RV 4 (the SVD; PTS_SVD_PAD in vsm_points.h says why in this order), 16 observations x 8
// (Jacobian rows and residuals), the 3x4 system
constexpr int kGroupDoubles = PTS_SVD_PAD + 16 + 16 + 4 + 4 + 16 * 8 + 12;

__global__ __launch_bounds__(256) void k_pts_triangulate(PtsDevice d) {
  __shared__ double s_m[16 * kGroupDoubles];
  __shared__ int32_t s_flag[16];
  const int grp = threadIdx.x >> 4, ln = threadIdx.x & 15;
  const int64_t t = (int64_t)blockIdx.x * 16 + grp;
  if (t >= d.n_tracks) return;  // whole groups leave together
  volatile double *U = s_m + grp * kGroupDoubles + PTS_SVD_PAD, *V = U + 16, *W = V + 16, *RV = W + 4, *rows = RV + 4, *ab = rows + 16 * 8;
  volatile int32_t *flag = s_flag + grp;
  const int32_t o = d.offsets[t], n = d.offsets[t + 1] - o;
  const int32_t *fr = d.obs_frames + o;
  const float *uv = d.uv + 2 * (size_t)o;
  int32_t status = 0, type = -2, updates = 0;
  double p[3] = {0, 0, 0}, dist = 0, ray = 0;
  do {
    if (d.flags && (d.flags[t] & 1)) {
      status = 1;
      break;
    }
    if (ln == 0) *flag = 0;
    VSM_GROUP_SYNC();
    for (int32_t i = ln; i < n; i += 16)
      if (!d.valid[fr[i]]) *flag = 1;
    VSM_GROUP_SYNC();
    if (*flag) {
      status = 2;
      break;
    }
    if (n < d.min_track_length) {
      status = 3;
      break;
    }
    const int32_t f1 = fr[0], f2 = fr[n - 1];
    const PtsFrame *F1 = d.frames + f1, *F2 = d.frames + f2;
    // ---- initPoint: lane 4 * r + j fills J[r][j] ----
    if (ln < PTS_SVD_PAD) U[-1 - ln] = 0;
    U[ln] = pts_init_entry(F1->proj, F2->proj, uv[0], uv[1], uv[2 * (size_t)(n - 1)], uv[2 * (size_t)(n - 1) + 1], ln >> 2, ln & 3);
    VSM_GROUP_SYNC();
    vsm_la::svd_group<4, 4>(U, V, W, RV, ln);
    VSM_GROUP_SYNC();
    if (!pts_init_point(V, p)) {
      p[0] = p[1] = p[2] = 0;
      status = 4;
      break;
    }
    type = pts_type(F1->inv, F2->inv, d.road, p);
    if (type < d.point_type) {
      status = 5;
      break;
    }
    // ---- refinePoint ----
    int result = PTS_UPDATED;
    for (int iter = 0; result == PTS_UPDATED;) {
      updates++;
      double acc = 0;
      VSM_GROUP_SYNC();
      if (ln == 0) *flag = 0;
      VSM_GROUP_SYNC();
      for (int32_t c0 = 0; c0 < n; c0 += 16) {
        const int32_t i = c0 + ln;
        if (i < n && !pts_row(d.frames[fr[i]].proj, p, uv[2 * (size_t)i], uv[2 * (size_t)i + 1], rows + ln * 8)) *flag = 1;
        VSM_GROUP_SYNC();
        if (*flag) break;  // (singular at some observation: the update has failed, the sums are not needed)
        if (ln < 12) {
          const int32_t cnt = n - c0 < 16 ? n - c0 : 16;
          for (int32_t k = 0; k < cnt; k++) acc = pts_add_obs(acc, ln, rows + k * 8);
        }
        VSM_GROUP_SYNC();
      }
      if (*flag) {
        result = PTS_FAILED;
      } else {
        if (ln < 12) ab[ln] = acc;
        VSM_GROUP_SYNC();
        if (ln == 0 && !pts_solve3(ab)) *flag = 1;
        VSM_GROUP_SYNC();
        result = *flag ? PTS_FAILED : pts_step(p, ab[3], ab[7], ab[11]);
      }
      if (iter++ > 20 || result == PTS_CONVERGED) break;
    }
    if (result == PTS_FAILED) {
      status = 6;
      break;
    }
    if (result != PTS_CONVERGED) {
      status = 7;
      break;
    }
    dist = pts_distance(d.frames[pts_mid_frame(d.valid, f1, f2)].c, p);
    if (!(dist < d.max_dist)) {
      status = 8;
      break;
    }
    ray = pts_ray(F1->c, F2->c, p);
  } while (0);
  if (ln == 0) {
    d.status[t] = status;
    d.type[t] = type;
    d.updates[t] = updates;
    d.xyz[3 * t + 0] = p[0];
    d.xyz[3 * t + 1] = p[1];
    d.xyz[3 * t + 2] = p[2];
    d.dist[t] = dist;
    d.ray[t] = ray;
  }
}

}  // namespace

void vsm_points_launch(hipStream_t s, VsmProf &pf, const PtsDevice &d) {
  if (d.n_tracks <= 0) return;
  pf.begin(VSM_K_PTS_TRIANGULATE, s);
  hipLaunchKernelGGL(k_pts_triangulate, dim3((d.n_tracks + 15) / 16), dim3(256), 0, s, d);
  pf.end(s);
}
