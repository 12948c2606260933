// Track triangulation, the host side without HIP: the argument checks, the parts that need libm (the road transform's sin
// and cos, the ray angle's acos) and vsm_host_triangulate - one host thread walking the per-track functions of
// vsm_points.h.  The host view is the CPU suite's subject and the device path's second opinion, never its fallback.
#include "vsm_points.h"

#include <math.h>
#include <string.h>

#include <vector>

int64_t pts_check_args(int32_t n_frames, const double *poses, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv,
                       const vsm_triangulate_params *params) {
  if (!params || params->min_track_length < 1) return -1;
  return pts_check_obs(n_frames, poses, n_tracks, offsets, obs_frames, uv);
}

int64_t pts_check_obs(int32_t n_frames, const double *poses, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv) {
  if (n_frames < 0 || n_tracks < 0) return -1;
  if (n_frames > 0 && !poses) return -1;
  if (n_tracks == 0) return 0;
  if (!offsets || offsets[0] != 0) return -1;
  for (int32_t t = 0; t < n_tracks; t++)
    if (offsets[t + 1] < offsets[t]) return -1;
  const int64_t n_obs = offsets[n_tracks];
  if (n_obs > 0 && (!obs_frames || !uv)) return -1;
  for (int64_t i = 0; i < n_obs; i++)
    if (obs_frames[i] < 0 || obs_frames[i] >= n_frames) return -1;
  return n_obs;
}

int64_t pts_check_points(bool params_ok, int32_t n_frames, const double *poses, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames,
                         const float *uv, const double *xyz) {
  if (!params_ok || (n_tracks > 0 && !xyz)) return -1;
  return pts_check_obs(n_frames, poses, n_tracks, offsets, obs_frames, uv);
}

void pts_road(double cam_pitch, double cam_height, double *road) {
  for (int i = 0; i < 12; i++) road[i] = 0;
  road[0 * 4 + 0] = 1;
  road[1 * 4 + 1] = +cos(cam_pitch);
  road[1 * 4 + 2] = -sin(cam_pitch);
  road[2 * 4 + 1] = +sin(cam_pitch);
  road[2 * 4 + 2] = +cos(cam_pitch);
  road[1 * 4 + 3] = -cam_height;
}

void pts_finish(int32_t n_tracks, double min_angle, int32_t *status, const double *ray, double *angle) {
  for (int32_t t = 0; t < n_tracks; t++) {
    angle[t] = 0;
    if (status[t] != 0) continue;
    angle[t] = ray[t] == PTS_RAY_DEGENERATE ? PTS_RAY_DEGENERATE : acos(ray[t]) * 180.0 / M_PI;
    if (!(angle[t] > min_angle)) status[t] = 9;  // (the reference keeps a point if rayAngle > min_angle)
  }
}

namespace {

// one track, up to the ray value: the statuses 0 (so far) .. 8
int32_t host_track(const PtsFrame *frames, const uint8_t *valid, const double *road, const int32_t *fr, const float *uv, int32_t n, int flagged,
                   const vsm_triangulate_params &prm, double *p, int32_t *type, int32_t *updates, double *dist, double *ray) {
  p[0] = p[1] = p[2] = 0;
  *type = -2;
  *updates = 0;
  *dist = *ray = 0;
  if (flagged) return 1;
  for (int32_t i = 0; i < n; i++)
    if (!valid[fr[i]]) return 2;
  if (n < prm.min_track_length) return 3;
  const PtsFrame &F1 = frames[fr[0]], &F2 = frames[fr[n - 1]];
  // initPoint
  // U, V, W, RV in one block behind PTS_SVD_PAD spare doubles, as in the kernel's LDS (vsm_points.h)
  double m[PTS_SVD_PAD + 16 + 16 + 4 + 4] = {0}, col[4];
  double *J = m + PTS_SVD_PAD, *V = J + 16, *w = V + 16, *rv1 = w + 4;
  for (int r = 0; r < 4; r++)
    for (int j = 0; j < 4; j++) J[r * 4 + j] = pts_init_entry(F1.proj, F2.proj, uv[0], uv[1], uv[2 * (n - 1)], uv[2 * (n - 1) + 1], r, j);
  vsm_la::svd_nr(J, 4, 4, 4, w, V, rv1, col);
  if (!pts_init_point(V, p)) {
    p[0] = p[1] = p[2] = 0;
    return 4;
  }
  *type = pts_type(F1.inv, F2.inv, road, p);
  if (*type < prm.point_type) return 5;
  // refinePoint
  int result = PTS_UPDATED;
  for (int iter = 0; result == PTS_UPDATED;) {
    ++*updates;
    double ab[12], row[8];
    for (int s = 0; s < 12; s++) ab[s] = 0;
    result = PTS_UPDATED;
    for (int32_t i = 0; i < n; i++) {
      if (!pts_row(frames[fr[i]].proj, p, uv[2 * i], uv[2 * i + 1], row)) {
        result = PTS_FAILED;
        break;
      }
      for (int s = 0; s < 12; s++) ab[s] = pts_add_obs(ab[s], s, row);
    }
    if (result != PTS_FAILED) result = pts_solve3(ab) ? pts_step(p, ab[3], ab[7], ab[11]) : PTS_FAILED;
    if (iter++ > 20 || result == PTS_CONVERGED) break;
  }
  if (result == PTS_FAILED) return 6;
  if (result != PTS_CONVERGED) return 7;
  *dist = pts_distance(frames[pts_mid_frame(valid, fr[0], fr[n - 1])].c, p);
  if (!(*dist < prm.max_dist)) return 8;  // (the reference keeps a point if pointDistance < max_dist)
  *ray = pts_ray(F1.c, F2.c, p);
  return 0;
}

}  // namespace

extern "C" {

void vsm_triangulate_default_params(vsm_triangulate_params *p) {
  if (!p) return;
  p->point_type = 1;
  p->min_track_length = 2;
  p->max_dist = 30.0;
  p->min_angle = 2.0;
  p->cam_pitch = -0.08;
  p->cam_height = 1.6;
}

int32_t vsm_host_triangulate(int32_t n_frames, const double *poses, const uint8_t *pose_valid, double f, double cu, double cv, int32_t n_tracks,
                             const int32_t *offsets, const int32_t *obs_frames, const float *uv, const uint8_t *flags,
                             const vsm_triangulate_params *params, int32_t *status, double *xyz, int32_t *type, int32_t *updates, double *dist,
                             double *angle) {
  if (pts_check_args(n_frames, poses, n_tracks, offsets, obs_frames, uv, params) < 0) return VSM_EARG;
  std::vector<PtsFrame> frames((size_t)n_frames);
  std::vector<uint8_t> valid((size_t)n_frames + 1, 1);
  for (int32_t k = 0; k < n_frames; k++) {
    pts_frame(poses + 12 * (size_t)k, f, cu, cv, &frames[k]);
    if (pose_valid) valid[k] = pose_valid[k] ? 1 : 0;
  }
  double road[12];
  pts_road(params->cam_pitch, params->cam_height, road);
  std::vector<int32_t> st((size_t)n_tracks), ty((size_t)n_tracks), up((size_t)n_tracks);
  std::vector<double> p((size_t)n_tracks * 3), di((size_t)n_tracks), ray((size_t)n_tracks), an((size_t)n_tracks);
  for (int32_t t = 0; t < n_tracks; t++) {
    const int32_t o = offsets[t], n = offsets[t + 1] - o;
    st[t] = host_track(frames.data(), valid.data(), road, obs_frames + o, uv + 2 * (size_t)o, n, flags ? (flags[t] & 1) : 0, *params, &p[3 * (size_t)t], &ty[t], &up[t],
                       &di[t], &ray[t]);
  }
  pts_finish(n_tracks, params->min_angle, st.data(), ray.data(), an.data());
  if (n_tracks > 0) {
    if (status) memcpy(status, st.data(), (size_t)n_tracks * 4);
    if (xyz) memcpy(xyz, p.data(), (size_t)n_tracks * 24);
    if (type) memcpy(type, ty.data(), (size_t)n_tracks * 4);
    if (updates) memcpy(updates, up.data(), (size_t)n_tracks * 4);
    if (dist) memcpy(dist, di.data(), (size_t)n_tracks * 8);
    if (angle) memcpy(angle, an.data(), (size_t)n_tracks * 8);
  }
  return n_tracks;
}

}  // extern "C"
