// Stand-alone host check of the location code that needs no GPU (csrc/vsm_locate.h, csrc/vsm_locate_host.cpp): vsm_host_locate
// on scenes generated here - frames of 0 to 513 rows of clean pixels, a frame with 30 % planted outliers, NaN and infinite
// pixels and points, points behind the camera, a point at 1e200, twelve copies of one point, a plane, frames not asked for,
// hypothesis counts of 1, 17 and 200, argument errors and empty inputs - against (a) what the scenes are built to give: the
// status, the counts, the pose within the pixels' rounding of the truth, and (b) vsm_host_resect from the linear poses, byte for
// byte; and the stages' own entries (vsm_host_locate_sample / _fit / _count), put together again, against the host view's
// winner.  Meant to be built with the sanitizers, e.g.
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude \
//       -Iopencl-structure-from-motion_amd/csrc tools/locate_host_check.cpp opencl-structure-from-motion_amd/csrc/vsm_locate_host.cpp \
//       opencl-structure-from-motion_amd/csrc/vsm_resect_host.cpp opencl-structure-from-motion_amd/csrc/vsm_points_host.cpp -o locate_host_check
// Prints "ok" and returns 0, or says what differed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "vsm_locate.h"

static int fails = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); \
      fails++;                                               \
    }                                                        \
  } while (0)

struct Scene {
  std::vector<double> poses, xyz;
  std::vector<int32_t> offsets{0}, frames;
  std::vector<float> uv;
  double f = 645.24, cu = 635.96, cv = 194.13;
  std::mt19937 rng{5};
  double uni(double a, double b) { return a + (b - a) * (double)(rng() >> 8) / (double)(1u << 24); }
  // camera k: a small yaw and a step along a path
  void camera(int k) {
    const double a = 0.012 * k, c = std::cos(a), s = std::sin(a);
    const double P[12] = {c, 0, s, 0.4 * k, 0, 1, 0, -0.01 * k, -s, 0, c, 0.3 * k};
    poses.insert(poses.end(), P, P + 12);
  }
  void project(int k, const double *X, float *u, float *v) const {
    const double *P = &poses[12 * (size_t)k];
    double xc[3];
    for (int i = 0; i < 3; i++) xc[i] = P[0 * 4 + i] * (X[0] - P[3]) + P[1 * 4 + i] * (X[1] - P[7]) + P[2 * 4 + i] * (X[2] - P[11]);
    *u = (float)(f * xc[0] / xc[2] + cu);
    *v = (float)(f * xc[1] / xc[2] + cv);
  }
  int32_t point(double x, double y, double z) {
    xyz.insert(xyz.end(), {x, y, z});
    return (int32_t)(xyz.size() / 3 - 1);
  }
  int32_t random_point() {
    const double z = uni(5, 20);
    return point(uni(-0.25, 0.25) * z, uni(-0.12, 0.12) * z, z);
  }
  // a track of one observation: the last point, seen by frame k at its projection moved by (du, dv)
  void see(int k, float du = 0, float dv = 0) {
    float u, v;
    project(k, &xyz[xyz.size() - 3], &u, &v);
    frames.push_back(k);
    uv.push_back(u + du);
    uv.push_back(v + dv);
    offsets.push_back((int32_t)frames.size());
  }
};

struct Result {
  std::vector<int32_t> status, best, inliers, rows, eligible, updates, used;
  std::vector<double> poses, lin, ss, rms;
  explicit Result(size_t F) : status(F + 1), best(F + 1), inliers(F + 1), rows(F + 1), eligible(F + 1), updates(F + 1), used(F + 1), poses(12 * F + 1), lin(12 * F + 1), ss(F + 1), rms(F + 1) {}
};

static int32_t run(const Scene &s, const uint8_t *ask, const vsm_locate_params &p, Result &r) {
  const int32_t F = (int32_t)(s.poses.size() / 12), T = (int32_t)s.offsets.size() - 1;
  return vsm_host_locate(F, ask, s.f, s.cu, s.cv, T, s.offsets.data(), s.frames.data(), s.uv.data(), s.xyz.data(), nullptr, &p, r.status.data(), r.poses.data(),
                         r.lin.data(), r.best.data(), r.inliers.data(), r.rows.data(), r.eligible.data(), r.updates.data(), r.used.data(), r.ss.data(), r.rms.data());
}

// (b): the poses are the resection's from the linear poses
static void check_refinement(const Scene &s, const vsm_locate_params &p, const Result &r) {
  const int32_t F = (int32_t)(s.poses.size() / 12), T = (int32_t)s.offsets.size() - 1;
  std::vector<uint8_t> go((size_t)F + 1);
  for (int32_t g = 0; g < F; g++) go[g] = r.status[g] == 0 || r.status[g] == 5 || r.status[g] == 6;
  const vsm_resect_params rp = lc_resect_params(p);
  std::vector<double> out(12 * (size_t)F + 1);
  std::vector<int32_t> st((size_t)F + 1);
  CHECK(vsm_host_resect(F, r.lin.data(), go.data(), go.data(), s.f, s.cu, s.cv, T, s.offsets.data(), s.frames.data(), s.uv.data(), s.xyz.data(), nullptr, &rp, st.data(),
                        out.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == F);
  for (int32_t g = 0; g < F; g++)
    if (go[g]) {
      CHECK(memcmp(&out[12 * (size_t)g], &r.poses[12 * (size_t)g], 96) == 0);
    } else {
      for (int i = 0; i < 12; i++) CHECK(r.poses[12 * (size_t)g + i] == 0.0);
    }
}

// float32 pixels: half an ulp below 2048 px is 6e-5 px, 1e-7 rad at this focal length, 2e-6 m at 20 m; five times that
static const double POSE_TOLERANCE = 1e-5;
static double pose_error(const Scene &s, const Result &r, int g) {
  double e = 0;
  for (int i = 0; i < 12; i++) e = std::max(e, std::fabs(r.poses[12 * (size_t)g + i] - s.poses[12 * (size_t)g + i]));
  return e;
}

int main() {
  vsm_locate_params prm;
  vsm_locate_default_params(&prm);
  CHECK(prm.ransac_iters == 200 && prm.min_inliers == 10 && prm.seed == 71 && prm.max_updates == 20 && lc_params_ok(&prm));
  CHECK(lc_seed_state(0) == 1 && lc_seed_state(2147483647u) == 1 && lc_seed_state(71) == 71);
  {  // row counts: frame g sees the first counts[g] points
    const int counts[] = {0, 5, 9, 10, 11, 16, 17, 255, 256, 257, 513};
    const int F = (int)(sizeof(counts) / sizeof(counts[0]));
    Scene s;
    for (int g = 0; g < F; g++) s.camera(g);
    for (int i = 0; i < 513; i++) {
      s.random_point();  // one track over several frames
      for (int g = 0; g < F; g++)
        if (i < counts[g]) {
          s.see(g);
          s.offsets.pop_back();
        }
      s.offsets.push_back((int32_t)s.frames.size());
    }
    for (int K : {1, 17, 200}) {
      vsm_locate_params p = prm;
      p.ransac_iters = K;
      Result r((size_t)F);
      CHECK(run(s, nullptr, p, r) == F);
      for (int g = 0; g < F; g++) {
        CHECK(r.rows[g] == counts[g] && r.eligible[g] == counts[g]);
        CHECK(r.status[g] == (counts[g] < 10 ? 2 : 0));
        if (r.status[g] == 0) CHECK(r.inliers[g] == counts[g] && r.used[g] == counts[g] && r.best[g] == 0 && pose_error(s, r, g) < POSE_TOLERANCE);
      }
      check_refinement(s, p, r);
    }
  }
  {  // hard inputs, a frame each: [0] outliers, [1] NaN / infinite, [2] behind, [3] 1e200, [4] one point twelve times, [5] a plane, [6] not asked for
    Scene s;
    for (int g = 0; g < 7; g++) s.camera(g);
    int clean = 0;
    for (int i = 0; i < 60; i++) {
      s.random_point();
      const bool bad = i % 10 < 3;
      const double a = s.uni(0, 6.28), d = s.uni(50, 120);
      s.see(0, bad ? (float)(d * std::cos(a)) : 0.f, bad ? (float)(d * std::sin(a)) : 0.f);
      clean += !bad;
    }
    for (int i = 0; i < 40; i++) {
      s.random_point();
      s.see(1);
      if (i == 3) s.uv[s.uv.size() - 2] = NAN;
      if (i == 5) s.uv[s.uv.size() - 1] = -INFINITY;
      if (i == 7) s.xyz[s.xyz.size() - 1] = NAN;
      if (i == 9) s.xyz[s.xyz.size() - 3] = INFINITY;
    }
    for (int i = 0; i < 45; i++) {
      if (i % 3 == 2)
        s.point(s.uni(-2, 2), s.uni(-1, 1), -s.uni(2, 9));
      else
        s.random_point();
      s.see(2);
    }
    for (int i = 0; i < 30; i++) {
      s.random_point();
      s.see(3);
      if (i == 4) s.xyz[s.xyz.size() - 3] = 1e200, s.xyz[s.xyz.size() - 2] = -1e200, s.xyz[s.xyz.size() - 1] = 1e200;
    }
    for (int i = 0; i < 12; i++) {
      s.point(0.5, -0.25, 9.0);
      s.see(4);
    }
    for (int i = 0; i < 40; i++) {
      const double x = s.uni(-3, 3), y = s.uni(-1.5, 1.5);
      s.point(x, y, 12.0 + 0.3 * x - 0.2 * y);
      s.see(5);
    }
    for (int i = 0; i < 20; i++) {
      s.random_point();
      s.see(6);
    }
    const uint8_t ask[8] = {1, 1, 1, 1, 1, 1, 0, 0};
    Result r(7);
    CHECK(run(s, ask, prm, r) == 7);
    CHECK(r.status[0] == 0 && r.inliers[0] == clean && r.used[0] == clean && r.eligible[0] == 60 && pose_error(s, r, 0) < POSE_TOLERANCE);
    CHECK(r.status[1] == 0 && r.rows[1] == 40 && r.eligible[1] == 36 && r.inliers[1] == 36 && pose_error(s, r, 1) < POSE_TOLERANCE);
    CHECK(r.status[2] == 0 && r.eligible[2] == 45 && r.inliers[2] == 30 && pose_error(s, r, 2) < POSE_TOLERANCE);
    CHECK(r.status[3] == 0 && r.eligible[3] == 30 && r.inliers[3] == 29 && pose_error(s, r, 3) < POSE_TOLERANCE);
    CHECK(r.status[4] == 3 && r.best[4] == -1 && r.eligible[4] == 12);
    CHECK((r.status[5] == 3 || r.status[5] == 4) && r.eligible[5] == 40);
    CHECK(r.status[6] == 1 && r.eligible[6] == 0 && r.rows[6] == 20);
    for (double x : r.poses) CHECK(std::isfinite(x));
    check_refinement(s, prm, r);
  }
  {  // argument errors leave the outputs alone; empty inputs
    Scene s;
    s.camera(0);
    for (int i = 0; i < 12; i++) {
      s.random_point();
      s.see(0);
    }
    Result r(1);
    r.status[0] = 77;
    vsm_locate_params p = prm;
    p.min_inliers = 5;
    CHECK(run(s, nullptr, p, r) == VSM_EARG && r.status[0] == 77);
    p = prm;
    p.ransac_iters = 0;
    CHECK(run(s, nullptr, p, r) == VSM_EARG && r.status[0] == 77);
    p = prm;
    p.inlier_threshold = NAN;
    CHECK(run(s, nullptr, p, r) == VSM_EARG && r.status[0] == 77);
    s.frames[3] = 1;
    CHECK(run(s, nullptr, prm, r) == VSM_EARG && r.status[0] == 77);
    s.frames[3] = 0;
    CHECK(run(s, nullptr, prm, r) == 1 && r.status[0] == 0);
    CHECK(vsm_host_locate(0, nullptr, 1, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &prm, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr, nullptr, nullptr) == 0);
    Result none(2);  // frames without tracks
    CHECK(vsm_host_locate(2, nullptr, 1, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &prm, none.status.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr, nullptr, nullptr, nullptr) == 2);
    CHECK(none.status[0] == 2 && none.status[1] == 2);
  }
  {  // the stages alone (vsm_host_locate_sample / _fit / _count) put together again give the host view's winner
    Scene s;
    s.camera(1);
    std::vector<float> uv;
    std::vector<double> xyz;
    int clean = 0;
    for (int i = 0; i < 300; i++) {
      s.random_point();
      const bool bad = i % 10 < 3;
      s.see(0, bad ? 70.f : 0.f, bad ? -55.f : 0.f);
      clean += !bad;
    }
    s.xyz[3 * 7] = NAN;  // a row that is not eligible
    uv = s.uv;
    xyz = s.xyz;  // a point per row: the tracks have one observation each
    vsm_locate_params p = prm;
    p.ransac_iters = 33;
    Result r(1);
    CHECK(run(s, nullptr, p, r) == 1 && r.status[0] == 0 && r.eligible[0] == 299);
    const int32_t K = p.ransac_iters, E = r.eligible[0];
    std::vector<int32_t> picks((size_t)K * 6), counts((size_t)K, -1);
    CHECK(vsm_host_locate_sample(p.seed, E, K, picks.data()) == VSM_OK);
    for (int32_t &q : picks) {
      CHECK(q >= 0 && q < E);
      if (q >= 7) q++;  // position among the eligible rows -> row
    }
    std::vector<double> states((size_t)K * 12, -7.5);
    std::vector<uint8_t> valid((size_t)K, 9);
    CHECK(vsm_host_locate_fit(s.f, s.cu, s.cv, p.min_depth, 300, uv.data(), xyz.data(), picks.data(), K, states.data(), valid.data()) == VSM_OK);
    CHECK(vsm_host_locate_count(s.f, s.cu, s.cv, 300, uv.data(), xyz.data(), states.data(), valid.data(), K, p.inlier_threshold, p.min_depth, counts.data()) == VSM_OK);
    int32_t best = -1, top = 0;
    for (int32_t k = 0; k < K; k++) {
      CHECK(valid[k] <= 1 && counts[k] >= 0 && (valid[k] || counts[k] == 0));
      if (counts[k] > top) top = counts[k], best = k;
    }
    CHECK(best == r.best[0] && top == r.inliers[0] && top == clean - 1);
    double lin[12];
    pts_rigid_inverse(&states[12 * (size_t)best], lin);
    CHECK(memcmp(lin, &r.lin[0], sizeof(lin)) == 0);
    // a refused sample leaves its state alone; arguments
    const int32_t same[6] = {4, 4, 4, 4, 4, 4};
    double one[12];
    for (double &x : one) x = -7.5;
    uint8_t ok = 9;
    xyz[12] = 0.5, xyz[13] = -0.25, xyz[14] = 9.0;
    CHECK(vsm_host_locate_fit(s.f, s.cu, s.cv, p.min_depth, 300, uv.data(), xyz.data(), same, 1, one, &ok) == VSM_OK && ok == 0 && one[0] == -7.5 && one[11] == -7.5);
    const int32_t out_of_range[6] = {0, 1, 2, 3, 4, 300};
    CHECK(vsm_host_locate_fit(s.f, s.cu, s.cv, p.min_depth, 300, uv.data(), xyz.data(), out_of_range, 1, one, &ok) == VSM_EARG);
    CHECK(vsm_host_locate_sample(p.seed, 5, 1, picks.data()) == VSM_EARG && vsm_host_locate_sample(p.seed, 6, 0, picks.data()) == VSM_EARG);
    CHECK(vsm_host_locate_count(s.f, s.cu, s.cv, 300, uv.data(), xyz.data(), states.data(), valid.data(), K, 0.0, p.min_depth, counts.data()) == VSM_EARG);
  }
  if (fails) return 1;
  printf("ok\n");
  return 0;
}
