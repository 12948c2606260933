// Triangulation of multi-view feature tracks into 3-D points (vsm_points.hip, vsm_points_host.cpp,
// vsm_points.inc).
//
// One track = the pixels of one scene point in several frames; with the frames' poses it becomes a 3-D point by the
// per-track mathematics of the reference's Reconstruction class (viso/reconstruction.cpp:121-139): initPoint (:148-177),
// pointType (:231-253), refinePoint / updatePoint (:179-202, :255-343), pointDistance (:204-211), rayAngle (:213-229).
// This header is the one statement of that mathematics: every product, every sum and its order.  The kernel (a 16-lane
// group per track) and the host view (one thread) both call the functions below and differ only in who calls them: the
// group deals the Jacobian rows and the twelve sums of the normal equations to its lanes, the host walks them in a loop.
// Everything is double; build with -ffp-contract=off.  No trigonometric function is in here: the road transform comes in
// as numbers, the ray angle leaves as the cosine's absolute value (vsm_points_host.cpp applies libm to both).
#pragma once
#include <stdint.h>

#include "visomatch.h"
#include "vsm_linalg.h"

enum { PTS_FAILED = 0, PTS_UPDATED = 1, PTS_CONVERGED = 2 };  // Reconstruction::result
#define PTS_RAY_DEGENERATE 1000.0  // rayAngle's return value for a camera centre on the point
// Matrix::svd is not safe against NaNs: once one has entered (a NaN pixel, an overflow), its convergence test never holds, the
// search for a split runs down to l = -1, and the sweep that follows reads and writes element -1 of w and rv1 and column -1 of
// u and v - one element in front of each array, never further.  Kernel and host view therefore keep U, V, W, RV in this order
// in one block with spare doubles in front (zeroed): W[-1] is V[15], RV[-1] is W[3], V[-1] is U[15], U[-1] is the spare.  Nothing
// leaves the block, and both sides compute the same even then.  (Two doubles, so that U stays 16-byte aligned.)
#define PTS_SVD_PAD 2

// what a frame contributes, worked out once per frame on the host (pts_frame): 27 doubles
struct PtsFrame {
  double proj[12];  // K * inv
  double inv[12];   // world -> camera: [R^T | -R^T c]
  double c[3];      // the camera centre
};

// pose: rows 0..2 of the camera-to-world [R | c], row-major.  inv is the RIGID inverse (the reference calls the general
// Matrix::inv on its 4x4); every entry of -R^T c and of K * inv is a sum over k ascending that starts from the k = 0 product.
// the rigid inverse alone, [R | c] -> [R^T | -R^T c] (the pose refinement, vsm_resect.h, goes both ways with it)
template <class In, class Out>
VSM_HD inline void pts_rigid_inverse(In pose, Out inv) {
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) inv[i * 4 + j] = pose[j * 4 + i];
    double s = pose[0 * 4 + i] * pose[3];
    s += pose[1 * 4 + i] * pose[7];
    s += pose[2 * 4 + i] * pose[11];
    inv[i * 4 + 3] = -s;
  }
}
VSM_HD inline void pts_frame(const double *pose, double f, double cu, double cv, PtsFrame *F) {
  pts_rigid_inverse(pose, F->inv);
  for (int i = 0; i < 3; i++) F->c[i] = pose[i * 4 + 3];
  const double K[9] = {f, 0, cu, 0, f, cv, 0, 0, 1};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) {
      double s = K[i * 3 + 0] * F->inv[0 * 4 + j];
      s += K[i * 3 + 1] * F->inv[1 * 4 + j];
      s += K[i * 3 + 2] * F->inv[2 * 4 + j];
      F->proj[i * 4 + j] = s;
    }
}

// affineTransform (viso/matrix.cpp:37-44), row r of a 3x4
template <class M>
VSM_HD inline double pts_affine_row(M m, int r, double x, double y, double z) {
  return x * m[r * 4 + 0] + y * m[r * 4 + 1] + z * m[r * 4 + 2] + m[r * 4 + 3];
}

// initPoint: entry (r, j) of the 4x4 J from the first (P1, u1, v1) and last (P2, u2, v2) observation
VSM_HD inline double pts_init_entry(const double *P1, const double *P2, double u1, double v1, double u2, double v2, int r, int j) {
  switch (r) {
    case 0: return P1[2 * 4 + j] * u1 - P1[0 * 4 + j];
    case 1: return P1[2 * 4 + j] * v1 - P1[1 * 4 + j];
    case 2: return P2[2 * 4 + j] * u2 - P2[0 * 4 + j];
    default: return P2[2 * 4 + j] * v2 - P2[1 * 4 + j];
  }
}
// ... and the point from the last column of V (4x4, row-major): false = at infinity.  w stays a double.
template <class M>
VSM_HD inline bool pts_init_point(M V, double *p) {
  const double w = V[3 * 4 + 3];
  if (fabs(w) < 1e-10) return false;
  p[0] = V[0 * 4 + 3] / w;
  p[1] = V[1 * 4 + 3] / w;
  p[2] = V[2 * 4 + 3] / w;
  return true;
}

// pointType: -1 not visible, 0 below the road, 1 road, 2 obstacle (inv1 / inv2: first / last observation's frame)
VSM_HD inline int32_t pts_type(const double *inv1, const double *inv2, const double *road, const double *p) {
  const double z1 = pts_affine_row(inv1, 2, p[0], p[1], p[2]);
  const double x2 = pts_affine_row(inv2, 0, p[0], p[1], p[2]), y2 = pts_affine_row(inv2, 1, p[0], p[1], p[2]), z2 = pts_affine_row(inv2, 2, p[0], p[1], p[2]);
  const double yr = pts_affine_row(road, 1, x2, y2, z2);
  if (z1 <= 1 || z2 <= 1) return -1;
  if (yr > 0.5) return 0;
  if (yr > -1) return 1;
  return 2;
}

// computePredictionsAndJacobian for one observation: row[0..2] the u row of the Jacobian, row[3..5] the v row, row[6..7] the
// residuals (observed - predicted).  false = singular (cc < 1e-10), nothing written.
template <class M>
VSM_HD inline bool pts_row(const double *P, const double *p, float u, float v, M row) {
  const double a = P[0] * p[0] + P[1] * p[1] + P[2] * p[2] + P[3];
  const double b = P[4] * p[0] + P[5] * p[1] + P[6] * p[2] + P[7];
  const double c = P[8] * p[0] + P[9] * p[1] + P[10] * p[2] + P[11];
  const double cc = c * c;
  if (cc < 1e-10) return false;
  row[0] = (P[0] * c - P[8] * a) / cc;
  row[1] = (P[1] * c - P[9] * a) / cc;
  row[2] = (P[2] * c - P[10] * a) / cc;
  row[3] = (P[4] * c - P[8] * b) / cc;
  row[4] = (P[5] * c - P[9] * b) / cc;
  row[5] = (P[6] * c - P[10] * b) / cc;
  row[6] = (double)u - a / c;
  row[7] = (double)v - b / c;
  return true;
}

// updatePoint's sums.  Sum s = 4 * m + n of the augmented 3x4 system [A | B]: n < 3 is A[m][n], n = 3 is B[m].  Every sum
// runs over i = 0 .. 2 * observations - 1 ascending, that is observation after observation, u row then v row: this adds one
// observation's two terms to the running sum (which starts at 0).
template <class M>
VSM_HD inline double pts_add_obs(double acc, int s, M row) {
  const int m = s >> 2, n = s & 3;
  const double ju = row[m], jv = row[3 + m];
  const double ku = n < 3 ? row[n] : row[6], kv = n < 3 ? row[3 + n] : row[7];
  acc += ju * ku;
  acc += jv * kv;
  return acc;
}

// Matrix::solve (viso/matrix.cpp:424-519) for the 3x3 system in the augmented 3x4 `ab` (row-major): Gauss-Jordan with
// full pivoting, eps = 1e-20; on success column 3 holds the solution.  ipiv is kept as three 4-bit counters (it can
// pass 1 only if no pivot candidate compares, i.e. with NaNs).  The final unscrambling of A's columns is left out: A is not
// read again.
template <class M>
VSM_HD inline bool pts_solve3(M ab) {
  uint32_t ipiv = 0;
  int icol = 0, irow = 0;
  for (int i = 0; i < 3; i++) {
    double big = 0.0;
    for (int j = 0; j < 3; j++)
      if (((ipiv >> (4 * j)) & 15u) != 1u)
        for (int k = 0; k < 3; k++)
          if (((ipiv >> (4 * k)) & 15u) == 0u)
            if (fabs(ab[j * 4 + k]) >= big) {
              big = fabs(ab[j * 4 + k]);
              irow = j;
              icol = k;
            }
    ipiv += 1u << (4 * icol);
    if (irow != icol)
      for (int l = 0; l < 4; l++) {
        const double t = ab[irow * 4 + l];
        ab[irow * 4 + l] = ab[icol * 4 + l];
        ab[icol * 4 + l] = t;
      }
    if (fabs(ab[icol * 4 + icol]) < 1e-20) return false;
    const double pivinv = 1.0 / ab[icol * 4 + icol];
    ab[icol * 4 + icol] = 1.0;
    for (int l = 0; l < 4; l++) ab[icol * 4 + l] = ab[icol * 4 + l] * pivinv;
    for (int ll = 0; ll < 3; ll++)
      if (ll != icol) {
        const double dum = ab[ll * 4 + icol];
        ab[ll * 4 + icol] = 0.0;
        for (int l = 0; l < 4; l++) ab[ll * 4 + l] = ab[ll * 4 + l] - ab[icol * 4 + l] * dum;
      }
  }
  return true;
}

// the end of updatePoint(step 1, eps 1e-5): p += step * B, converged if every |B| < eps
VSM_HD inline int pts_step(double *p, double b0, double b1, double b2) {
  const double step = 1, eps = 1e-5;
  p[0] += step * b0;
  p[1] += step * b1;
  p[2] += step * b2;
  return (fabs(b0) < eps && fabs(b1) < eps && fabs(b2) < eps) ? PTS_CONVERGED : PTS_UPDATED;
}

// pointDistance's frame: (first + last) / 2 in integer division, then the nearest lower frame with a valid pose
VSM_HD inline int32_t pts_mid_frame(const uint8_t *valid, int32_t first, int32_t last) {
  int32_t mid = (first + last) / 2;
  while (mid > first && !valid[mid]) mid--;
  return mid;
}
VSM_HD inline double pts_distance(const double *c, const double *p) {
  const double dx = c[0] - p[0], dy = c[1] - p[1], dz = c[2] - p[2];
  return sqrt(dx * dx + dy * dy + dz * dz);
}
// rayAngle without its acos: |v1 . v2| of the unit rays from the point to the two centres, or PTS_RAY_DEGENERATE
VSM_HD inline double pts_ray(const double *c1, const double *c2, const double *p) {
  double v1[3], v2[3], n1 = 0, n2 = 0;
  for (int i = 0; i < 3; i++) {
    v1[i] = c1[i] - p[i];
    v2[i] = c2[i] - p[i];
  }
  for (int i = 0; i < 3; i++) n1 += v1[i] * v1[i];
  for (int i = 0; i < 3; i++) n2 += v2[i] * v2[i];
  n1 = sqrt(n1);
  n2 = sqrt(n2);
  if (n1 < 1e-10 || n2 < 1e-10) return PTS_RAY_DEGENERATE;
  double dot = 0;
  for (int i = 0; i < 3; i++) dot += (v1[i] / n1) * (v2[i] / n2);
  return fabs(dot);
}

// ---- host side (vsm_points_host.cpp; no HIP) ----
// the argument checks of vsm_triangulate_run / vsm_host_triangulate: the number of observations, or -1
int64_t pts_check_args(int32_t n_frames, const double *poses, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv,
                       const vsm_triangulate_params *params);
// its part without the parameters, which the resection and the vetting share: the frames, the offsets and the observations
int64_t pts_check_obs(int32_t n_frames, const double *poses, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv);
// the argument checks of the general forms that take points (resection, vetting, joint adjustment) and of their host views:
// the stage's own test of its parameters has passed, tracks come with their points, then pts_check_obs
int64_t pts_check_points(bool params_ok, int32_t n_frames, const double *poses, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames,
                         const float *uv, const double *xyz);
// rows 0..2 of Tr_cam_road (Reconstruction::setCalibration), with libm's sin and cos
void pts_road(double cam_pitch, double cam_height, double *road12);
// the last step, which needs libm: the angle from the ray value, status 9 where it is not above min_angle
void pts_finish(int32_t n_tracks, double min_angle, int32_t *status, const double *ray, double *angle);

// ---- device path (vsm_points.hip) ----
#ifdef __HIP__
struct VsmProf;
struct PtsDevice {
  // uploaded
  const PtsFrame *frames;
  const uint8_t *valid;      // per frame
  const int32_t *offsets;    // [n_tracks + 1]
  const int32_t *obs_frames; // per observation
  const float *uv;           // per observation, (u, v)
  const uint8_t *flags;      // per track
  // results, per track
  int32_t *status, *type, *updates;
  double *xyz, *dist, *ray;
  double road[12];
  double max_dist;
  int32_t n_tracks, point_type, min_track_length;
};
void vsm_points_launch(hipStream_t s, VsmProf &pf, const PtsDevice &d);
#endif
