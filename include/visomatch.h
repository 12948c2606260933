/* visomatch.h -- C-ABI of libvisomatch.so, the MI355X-native (gfx950, HIP) replacement for
 * libviso2's per-frame matcher hot path as vendored in dphoyes/OpenCL-Structure-from-Motion.
 *
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference repository).  Plain pointers and sizes only; no C++/torch types cross this line.
 * The header-only C++ class in include/matcher.h forwards the reference's own
 * `class Matcher` surface (viso/matcher.h:37-136) to these functions.
 *
 * Error convention: functions returning int give 0 (VSM_OK) on success or a negative
 * VSM_E* code.  The reference's C++ API has no error returns (bad dims print
 * "ERROR: Image dimension mismatch!" to stderr and leave the state untouched,
 * viso/matcher.cpp:103-106; matchFeatures with missing buffers returns silently and keeps
 * the previous matches, :190-216); the C++ wrapper swallows the codes to keep that behaviour.
 *
 * Threading: one handle = one HIP device + one stream; a handle is not re-entrant.
 * Distinct handles are independent (unlike the reference, whose Delaunay code keeps
 * file-scope state, viso/triangle.cpp:541-550).
 */
#ifndef VISOMATCH_H
#define VISOMATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSM_OK 0
#define VSM_EDIMS (-1)     /* the reference's "Image dimension mismatch" */
#define VSM_ENOTREADY (-2) /* matchFeatures' silent early return: ring buffer not filled */
#define VSM_EHIP (-3)      /* HIP runtime error (message on stderr) */
#define VSM_EARG (-4)

typedef struct vsm_handle vsm_handle;

/* Matcher::parameters, viso/matcher.h:42-69 (same field order and defaults) */
typedef struct vsm_params {
  int32_t nms_n;
  int32_t nms_tau;
  int32_t match_binsize;
  int32_t match_radius;
  int32_t match_disp_tolerance;
  int32_t outlier_disp_tolerance;
  int32_t outlier_flow_tolerance;
  int32_t multi_stage;
  int32_t half_resolution;
  int32_t refinement;
  double f, cu, cv, base;
} vsm_params;

/* Matcher::p_match, viso/matcher.h:86-100 -- identical 48-byte layout */
typedef struct vsm_p_match {
  float u1p, v1p;
  int32_t i1p;
  float u2p, v2p;
  int32_t i2p;
  float u1c, v1c;
  int32_t i1c;
  float u2c, v2c;
  int32_t i2c;
} vsm_p_match;

/* Matcher::parameters::parameters(), viso/matcher.h:57-68 */
void vsm_default_params(vsm_params *p);

/* Matcher::Matcher(parameters), viso/matcher.cpp:33-61.  Binds the calling thread's current
 * HIP device.  Returns NULL if no HIP device is usable (never falls back to the CPU). */
vsm_handle *vsm_create(const vsm_params *p);

/* Matcher::~Matcher(), viso/matcher.cpp:64-93 */
void vsm_destroy(vsm_handle *h);

/* Matcher::setIntrinsics, viso/matcher.h:78-83 */
void vsm_set_intrinsics(vsm_handle *h, double f, double cu, double cv, double base);

/* Matcher::pushBack(I1,I2,dims,replace), viso/matcher.cpp:95-181 (I2 == NULL: the mono
 * overload viso/matcher.h:118).  Host images, row stride bpl.  The input may be reused as
 * soon as the call returns. */
int vsm_push_back(vsm_handle *h, const uint8_t *I1, const uint8_t *I2, int32_t width, int32_t height, int32_t bpl,
                  int replace);

/* Same, for images that already live in this device's HBM (the bench's resident-input path).
 * Ordering and lifetime contract of every entry point that takes device pointers (this one, vsm_sequence_run with
 * on_device = 1, vsm_vo_stereo_process_device, vsm_vo_mono_process_device):
 *  - the images are READ ASYNCHRONOUSLY on the handle's own (non-blocking) stream.  Work that produces them on another
 *    stream must have completed, or be ordered in front with vsm_wait_for_stream() right before the call;
 *  - they must stay valid and unchanged until the handle has consumed them: until the next synchronising call on the
 *    handle for a push (vsm_match, any getter), until the call returns for vsm_sequence_run and the VO entry points. */
int vsm_push_back_device(vsm_handle *h, const uint8_t *dI1, const uint8_t *dI2, int32_t width, int32_t height,
                         int32_t bpl, int replace);
/* orders everything the handle enqueues from now on behind the work `hip_stream` (a hipStream_t; NULL = the null stream)
 * holds at this moment: an event recorded there, a wait on the handle's stream - no host synchronisation */
int vsm_wait_for_stream(vsm_handle *h, void *hip_stream);

/* Matcher::matchFeatures(method, Tr_delta), viso/matcher.cpp:183-241.  method 0 flow, 1 stereo,
 * 2 quad.  Tr_delta: NULL or 12 doubles = rows 0..2 of the 4x4 matrix, row-major
 * (what viso/matcher.cpp:989-1002 reads). */
int vsm_match(vsm_handle *h, int32_t method, const double *Tr_delta);

/* Matcher::getMatches(), viso/matcher.h:131 */
int32_t vsm_num_matches(vsm_handle *h);
int32_t vsm_get_matches(vsm_handle *h, vsm_p_match *out, int32_t cap);

/* Matcher::bucketFeatures, viso/matcher.cpp:243-284 (uses the C library rand() like the reference) */
int vsm_bucket(vsm_handle *h, int32_t max_features, float bucket_width, float bucket_height);

/* Matcher::getGain, viso/matcher.cpp:286-324 */
float vsm_gain(vsm_handle *h, const int32_t *inliers, int32_t n);

/* ---- look-ahead API: a whole sequence at once ----
 * Semantically identical to
 *     for f in 0..n_frames-1:  pushBack(left[f], right[f], dims, false);  matchFeatures(method, Tr[f])
 * on a fresh Matcher (viso/matcher.cpp:95, :183), but the frames of a chunk (VSM_SEQ_CHUNK; default 110
 * with ten or more host-pool threads and device-resident frames, 80 with six to nine or host-resident frames, else 50, and 50 in
 * the host-shared form) go through every kernel in one launch and the host stages of the chunk's frame pairs run in
 * parallel.  left/right: n_frames images frame_stride bytes apart (host or, with on_device != 0,
 * HBM); right == NULL (mono) with stereo / quad matching goes frame by frame (the reference's matchFeatures returns early).
 * Tr_delta: NULL or n_frames x 12 doubles, Tr_valid: NULL (all valid) or n_frames flags.
 * The streaming ring buffer (vsm_push_back / vsm_match) is not touched except by the fallback.
 * STREAMS: besides the handle's own non-blocking streams the GPU-resident form uses the process's NULL stream (result
 * export copies, device vertex sorts) and drains it before it returns: an application that keeps work of its own on the
 * null stream - PyTorch's default stream is it, blocking streams synchronise with it - sets option "seq_null_stream" = 0
 * (vsm_set_option) and the library uses a non-blocking stream of its own instead. */
int vsm_sequence_run(vsm_handle *h, const uint8_t *left, const uint8_t *right, int64_t frame_stride, int on_device,
                     int32_t n_frames, int32_t width, int32_t height, int32_t bpl, int32_t method,
                     const double *Tr_delta, const uint8_t *Tr_valid);
/* getMatches() as it would read after frame `frame`: where matchFeatures returned early on a frame (an image without
 * features), the list of the last frame before it on which it ran */
int32_t vsm_sequence_num_matches(vsm_handle *h, int32_t frame);
int32_t vsm_sequence_get_matches(vsm_handle *h, int32_t frame, vsm_p_match *out, int32_t cap);
/* wall-clock split of the last vsm_sequence_run() on the caller's thread, microseconds: {launching and waiting
 * for the GPU, host stages it takes part in (prior statistics, final drain), total, chunk size} - the stages
 * overlap, so the first two are not what the GPU / the host pool were busy for */
void vsm_sequence_get_timings(vsm_handle *h, double *out4);
/* which form of the look-ahead path the last vsm_sequence_run took: 2 = GPU-resident (lists stay in HBM from the first
 * matching pass to the survivors; the host only runs Triangle's vertex sort), 1 = host-shared (VSM_SEQ_V2=0, or a list
 * the device chain declines) */
int32_t vsm_sequence_path(vsm_handle *h);
/* ---- arbitrary frame pairs of an image set in one call ----
 * left / right: n_frames images frame_stride bytes apart, host memory or (on_device != 0) HBM, laid out as for
 * vsm_sequence_run; right == NULL is mono input (one image per frame).  pairs: n_pairs x {previous frame, current frame}.
 * The list of pair k = (a, b) is, byte for byte, getMatches() of a FRESH Matcher with the handle's parameters and
 * intrinsics after
 *     pushBack(frame a);  pushBack(frame b);  matchFeatures(method, Tr_delta of pair k if given and valid)
 * so i1p / i2p index frame a's feature sets and i1c / i2c frame b's.  Where matchFeatures would return early (an image
 * without features; mono input with method 1 or 2) the pair's list is empty and the call still returns VSM_OK.  With
 * method 1 the previous frame is not read and may be -1.  a == b and repeated pairs are allowed.
 * Tr_delta: NULL or n_pairs x 12 doubles, Tr_valid: NULL (all valid) or n_pairs flags - both per PAIR.
 * VSM_EARG before anything is enqueued, the previous call's lists left in place: a frame index outside [0, n_frames) (a
 * previous frame of -1 with method 0 or 2 included), n_pairs <= 0, pairs == NULL, a method outside 0..2.
 * Every frame goes through the image side once, however many pairs name it, and all sides * n_frames images stay in HBM
 * for the call (INTEGRATION.md has the bytes per image); the pairs then go through both matching passes, the refinement
 * and the exact-Delaunay chains in chunks of at most C pairs (option "pairs_chunk"; 0 = the look-ahead call's chunk rule
 * for device-resident frames), a chunk's survivors are copied into per-pair host lists, so host memory grows with the
 * matches found.  What the device chain cannot take - more than 1024 statistics bins, a list beyond its limits, a list
 * it declined - goes pair by pair through the per-frame code: the call never fails where the per-frame API would succeed.
 * The streaming ring (vsm_push_back / vsm_match / vsm_get_matches and the stage views) and the results and state of
 * vsm_sequence_run are not touched; only the handle's own stream is used.  Device pointers follow the contract stated at
 * vsm_push_back_device: read asynchronously on the handle's stream, valid and unchanged until the call returns. */
int vsm_pairs_run(vsm_handle *h, const uint8_t *left, const uint8_t *right, int64_t frame_stride, int on_device,
                  int32_t n_frames, int32_t width, int32_t height, int32_t bpl, int32_t method,
                  const int32_t *pairs, int32_t n_pairs, const double *Tr_delta, const uint8_t *Tr_valid);
/* the list of pair `pair` of the last vsm_pairs_run (0 matches for an index outside it) */
int32_t vsm_pairs_num_matches(vsm_handle *h, int32_t pair);
int32_t vsm_pairs_get_matches(vsm_handle *h, int32_t pair, vsm_p_match *out, int32_t cap);
/* wall-clock split of the last vsm_pairs_run on the caller's thread, microseconds: {image side of all frames, first passes +
 * their outlier removal and prior boxes, second passes + refinement + final chains + copy-out, total} */
void vsm_pairs_get_timings(vsm_handle *h, double *out4);
/* ---- multi-view feature tracks from pair match lists ----
 * No counterpart in the reference, which links consecutive frames only, one list at a time: matlab/plotTrack.m walks
 * i_matched backwards frame by frame, Reconstruction::update (viso/reconstruction.cpp:71-104) keeps a track_map keyed by
 * last_idx.  These calls generalise both to arbitrary pairs.
 * Input: n_frames; pairs: n_pairs x {previous frame a, current frame b}; one match list per pair (lists[k], counts[k]);
 * side 0 links i1p -> i1c (the left images), 1 links i2p -> i2c.  A NODE is a (frame, feature index) that at least one match
 * names; match m of pair k is an edge between (a, ip) and (b, ic).  A TRACK is a connected component; its observations are
 * its nodes in ascending (frame, feature) order.  Tracks with fewer than min_length observations are dropped; the kept
 * ones are numbered 0 .. T-1 in ascending order of their smallest node.  Results, all exact integers:
 *   offsets[T + 1]   track t's observations are rows offsets[t] .. offsets[t + 1] - 1
 *   obs[n_obs][4]    {frame, feature, pair, 2 * match + end}: (pair, match, end 0 = previous / 1 = current) is the first
 *                    match, in that order, that names the node - pixel coordinates and, for quad lists, the other image's
 *                    index are read from it
 *   flags[T]         bit 0 = inconsistent: two observations in one frame (a self pair a == b; mismatches that merge two points)
 *   per pair, track_of_match[counts[k]]: the track of every match, -1 where its track was dropped
 * The result depends on the inputs only, not on thread order; the partition into tracks not on the order of the pairs.
 * VSM_EARG, nothing enqueued and the last result kept: side outside 0..1, min_length < 1, a frame index outside
 * [0, n_frames) (a previous frame of -1 is a stereo-only list: tracks across time are not defined for it), a negative
 * feature index on the chosen side, a NULL list with a positive count, more than 2^31 - 2 node ids (the sum over the frames
 * of 1 + the largest index named) or 2^30 - 1 matches.  No pair with a match: VSM_OK, 0 tracks.
 * vsm_tracks_run takes lists in host memory, wherever they came from (vsm_pairs_run, vsm_sequence_run with pairs
 * (f - 1, f), the per-frame API), and runs on the handle's device and stream: the index pairs go up in one copy (8 bytes
 * per match), the results come back in one.  It has no CPU path.  Segments of at most VSM_TRACKS_WAVE_MAX observations
 * are ordered by a wave, of at most VSM_TRACKS_BLOCK_MAX by a workgroup, longer ones by the host. */
#define VSM_TRACKS_WAVE_MAX 64
#define VSM_TRACKS_BLOCK_MAX 2048
int vsm_tracks_run(vsm_handle *h, int32_t n_frames, const int32_t *pairs, int32_t n_pairs, const vsm_p_match *const *lists,
                   const int32_t *counts, int32_t side, int32_t min_length);
/* the same on the pairs and lists of the last vsm_pairs_run, which stay as they are, like all other state of the handle.
 * VSM_ENOTREADY without such a run, VSM_EARG after one with method 1. */
int vsm_pairs_tracks(vsm_handle *h, int32_t side, int32_t min_length);
/* the handle's last track result: T; n_obs; the three arrays (any may be NULL; returns T); the tracks of pair `pair`'s
 * matches (copies at most cap, returns the pair's match count) */
int32_t vsm_tracks_count(vsm_handle *h);
int32_t vsm_tracks_num_obs(vsm_handle *h);
int32_t vsm_tracks_get(vsm_handle *h, int32_t *offsets, int32_t *obs, uint8_t *flags);
int32_t vsm_tracks_of_matches(vsm_handle *h, int32_t pair, int32_t *out, int32_t cap);
/* {node ids, edges, tracks kept, inconsistent tracks, segments ordered by a wave, by a workgroup, by the host, items per
 * workgroup of the device scan} */
void vsm_tracks_get_stats(vsm_handle *h, int64_t *out8);
/* wall-clock split of the last call, microseconds: {packing, upload, kernels (with the one wait for the totals), download +
 * host part} */
void vsm_tracks_get_timings(vsm_handle *h, double *out4);
/* The same definition by a plain sequential union-find on the host: no GPU, no handle (the CPU suite's subject and the
 * device path's second opinion - not a fallback).  Returns T, or VSM_EARG with the output arrays untouched.  Outputs may be
 * NULL: call once for T and *n_obs, then with offsets[T + 1], obs[n_obs][4], flags[T] and track_of_match[sum of counts]
 * (pair after pair). */
int32_t vsm_host_tracks(int32_t n_frames, const int32_t *pairs, int32_t n_pairs, const vsm_p_match *const *lists,
                        const int32_t *counts, int32_t side, int32_t min_length, int32_t *offsets, int32_t *obs, uint8_t *flags,
                        int32_t *track_of_match, int32_t *n_obs);
/* ---- triangulation of feature tracks into 3-D points ----
 * The per-track mathematics of the reference's Reconstruction class (viso/reconstruction.{h,cpp}), in a batch form of this
 * library's own: the class is incremental over consecutive frames, caps a track at 6 pixels, keeps points as float and pairs
 * a track's first and last pixel with the pose of the frame AFTER the one they were seen in; here every observation uses
 * its own frame's matrices, a track has any length and everything is double.
 * Input: n_frames poses, camera to world, 12 doubles each (rows 0..2 of [R | c], row-major), pose_valid: a byte per frame
 * (NULL: all valid); the intrinsics f, cu, cv; the tracks as vsm_tracks_get gives them: offsets[T + 1] (offsets[0] = 0),
 * per observation its frame (ascending within a track) and its pixel uv = (u, v) as two floats; flags[T] (may be NULL).
 * Per frame, once, on the host: inv = [R^T | -R^T c] - the rigid inverse, not the reference's general Matrix::inv - and
 * proj = K * inv, every entry a sum over k ascending from the k = 0 product.  Tr_cam_road is built on the host from
 * cam_pitch and cam_height as Reconstruction::setCalibration does.
 * Per track, the steps of reconstruction.cpp:121-139 in that order; the first status that applies wins:
 *   1  the track is flagged inconsistent (flags bit 0): not attempted
 *   2  an observation's frame has no valid pose
 *   3  fewer than min_track_length observations
 *   4  initPoint on the first and last observation (4x4 J, Matrix::svd, w = V[3][3] kept as a double): |w| < 1e-10
 *   5  pointType with the first and last observation's frames (-1 not visible, 0 below the road, 1 road, 2 obstacle) is
 *      below point_type
 *   6  refinePoint: an updatePoint(step 1, eps 1e-5) failed - cc < 1e-10 at an observation, or Matrix::solve (Gauss-Jordan,
 *      full pivoting, eps 1e-20) found no pivot.  Every update uses ALL the track's observations and sums over i ascending.
 *   7  not converged after the reference loop's 22 updates
 *   8  pointDistance from the centre of frame (first frame + last frame) / 2 (integer division; without a valid pose there,
 *      the nearest lower frame with one) is not below max_dist
 *   9  rayAngle between the rays to the first and last observation's centres is not above min_angle.  The device writes
 *      |v1 . v2| (1000 for a centre on the point); the host applies libm's acos(..) * 180 / pi and decides.
 *   0  kept
 * Results per track, all exact: status; xyz[3], the point as it stood when the status was decided (zeros for 1..4); type
 * (-2 where pointType was not reached); updates, the number of updatePoint calls; dist and angle (0 where not reached). */
typedef struct vsm_triangulate_params {
  int32_t point_type;        /* 1 */
  int32_t min_track_length;  /* 2 */
  double max_dist;           /* 30.0 */
  double min_angle;          /* 2.0 (degrees) */
  double cam_pitch;          /* -0.08 */
  double cam_height;         /* 1.6    (defaults: reconstruction.h:62, reconstruction.cpp:37-38) */
} vsm_triangulate_params;
void vsm_triangulate_default_params(vsm_triangulate_params *p);
/* The general form, on the caller's arrays.  Runs on the handle's device and stream: one copy up (27 doubles per frame, 12
 * bytes per observation, 5 per track), the kernel (a 16-lane group per track), one copy back (52 bytes per track).  It has
 * no CPU path.  VSM_EARG, nothing enqueued and the last result kept: a frame index outside [0, n_frames), offsets that do
 * not start at 0 or decrease, a NULL array with a positive count, params NULL or min_track_length < 1.  Nothing else of the
 * handle is touched: not the streaming ring, not the vsm_pairs_run lists, not the track result. */
int vsm_triangulate_run(vsm_handle *h, int32_t n_frames, const double *poses, const uint8_t *pose_valid, double f, double cu, double cv,
                        int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv, const uint8_t *flags,
                        const vsm_triangulate_params *params);
/* The same on the handle's last track result (frame count and side as given to that call; poses: one per frame).  The
 * pixel of observation {frame, feature, pair, 2 * match + end} is read from match `match` of lists[pair]: u1p / v1p (end 0)
 * or u1c / v1c (end 1) for side 0, u2p / v2p or u2c / v2c for side 1.  lists == NULL: the lists of the last vsm_pairs_run
 * (counts is not read).  VSM_ENOTREADY: no track result; or lists == NULL and the tracks did not come from vsm_pairs_tracks
 * (or a later vsm_pairs_run has replaced the lists).  VSM_EARG: counts disagree with the track result's, a NULL list with a
 * positive count, params as above. */
int vsm_tracks_triangulate(vsm_handle *h, const vsm_p_match *const *lists, const int32_t *counts, const double *poses,
                           const uint8_t *pose_valid, double f, double cu, double cv, const vsm_triangulate_params *params);
/* the handle's last point result: T; the six arrays (any may be NULL; returns T): status[T], xyz[T][3], type[T], updates[T],
 * dist[T], angle[T] */
int32_t vsm_points_count(vsm_handle *h);
int32_t vsm_points_get(vsm_handle *h, int32_t *status, double *xyz, int32_t *type, int32_t *updates, double *dist, double *angle);
/* tracks per status value 0..9 */
void vsm_points_get_stats(vsm_handle *h, int64_t *out10);
/* wall-clock split of the last call, microseconds: {gather / packing, upload, kernel, download + host part} */
void vsm_points_get_timings(vsm_handle *h, double *out4);
/* The same definition on one host thread: no GPU, no handle (the CPU suite's subject and the device path's second opinion -
 * not a fallback).  Returns T, or VSM_EARG with the output arrays untouched.  Outputs may be NULL. */
int32_t vsm_host_triangulate(int32_t n_frames, const double *poses, const uint8_t *pose_valid, double f, double cu, double cv,
                             int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv, const uint8_t *flags,
                             const vsm_triangulate_params *params, int32_t *status, double *xyz, int32_t *type, int32_t *updates,
                             double *dist, double *angle);
/* ---- refinement of camera poses against triangulated points ----
 * The other half of the alternation: the triangulation refines points with the poses fixed, this refines every frame's pose
 * with the points fixed - motion-only bundle adjustment, a Gauss-Newton resection per frame.  No counterpart in the
 * reference.  csrc/vsm_resect.h is the one statement of the arithmetic (every product, every sum and its order); what
 * follows is the contract.
 * Input: n_frames poses, camera to world, 12 doubles each (rows 0..2 of [R | c]); pose_valid, a byte per frame (NULL: all
 * valid); refine, a byte per frame (NULL: all) - a frame with 0 is left alone, which is how a caller pins the root; the
 * intrinsics f, cu, cv; the tracks exactly as vsm_triangulate_run takes them (offsets[T + 1], obs_frames, uv); xyz[T][3],
 * the tracks' points; use[T] bytes (NULL: all).
 * The ROWS of frame g are the observations (t, i) with obs_frames == g and use[t] != 0, in ascending (t, i); a row is
 * {track, u, v}.  The state is world to camera, [Rw | tw], the rigid inverse [R^T | -R^T c] of the input pose as the
 * triangulation forms it.  One UPDATE evaluates every row at the state: Xc = Rw X + tw; the row is USED if zc > min_depth
 * and ru^2 + rv^2 < max_residual^2 (max_residual = 0: below infinity), with ru = u - (f xc / zc + cu), rv = v - (f yc / zc
 * + cv) - so rows behind the camera, NaN pixels, NaN points and overflowing residuals are never used.  Over the used rows
 * it forms the 21 upper entries of J^T J, the 6 of J^T r (J the derivative of the prediction for Xc' = Xc + w x Xc + tau,
 * parameters (w, tau)) and the sum of ru^2 + rv^2: 28 double sums and a count.  Every sum is taken in one fixed order:
 * partial[l], l = 0..255, adds the terms of the frame's rows i with i mod 256 == l in ascending order starting from 0.0 (a
 * skipped row adds nothing); then for s = 128, 64, .., 1: partial[l] += partial[l + s] for l < s; the sum is partial[0].
 * The 6x6 system is solved by Gauss-Jordan with full pivoting (eps 1e-20, the stereo egomotion's Matrix::solve) and the
 * state moves by the Cayley rotation of a = w / 2, Rd = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a): Rw <- Rd Rw, tw <- Rd
 * tw + tau.  Only + - * / on doubles: the device equals the host view bit for bit.  Converged when all six |delta| <= eps.
 * Per frame, the first status that applies wins:
 *   1  no valid input pose
 *   2  not asked for (refine == 0)
 *   3  fewer than min_observations rows
 *   4  an update found fewer than min_observations used rows
 *   5  an update's system had no pivot
 *   6  not converged after max_updates updates: the estimate as it stands
 *   0  refined
 * Results per frame: status; pose[12], camera to world, the rigid inverse of the final state (status 0, 6) or the input
 * pose's bytes (1..5); updates, the number of updates applied to the state; rows; used, the rows used at the last
 * evaluation (0 for 1..3); ss_before, the sum of ru^2 + rv^2 over the rows used at the input pose (0 for 1..3); ss_after,
 * the same at the final state from one more evaluation (status 0, 6; else 0); rms_before / rms_after, libm's sqrt(ss /
 * rows used at that evaluation) applied by the host (0 where nothing was used). */
typedef struct vsm_resect_params {
  int32_t min_observations; /* 10 */
  int32_t max_updates;      /* 20 */
  double eps;               /* 1e-8 */
  double max_residual;      /* 0 = no gate (pixels) */
  double min_depth;         /* 1e-10 */
} vsm_resect_params;
void vsm_resect_default_params(vsm_resect_params *p);
/* The general form, on the caller's arrays.  Runs on the handle's device and stream: the host groups the rows by frame (a
 * stable counting sort, timed), one copy up (102 bytes per frame, 12 per row, 24 per track), the kernel (a 256-thread
 * workgroup per frame, the update loop inside), one copy back (128 bytes per frame).  It has no CPU path.  VSM_EARG,
 * nothing enqueued and the last result kept: what vsm_triangulate_run rejects (with params NULL), min_observations < 6,
 * max_updates < 1, eps not positive or not finite, xyz NULL with n_tracks > 0.  Nothing else of the handle is touched. */
int vsm_resect_run(vsm_handle *h, int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *refine, double f, double cu,
                   double cv, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv, const double *xyz,
                   const uint8_t *use, const vsm_resect_params *params);
/* The same on the handle's last track and point results: use = the point's status is 0, xyz the points, the pixels read
 * from the match lists as vsm_tracks_triangulate reads them (lists, counts: as there).  VSM_ENOTREADY: no track result or
 * no point result, or their track counts differ; lists == NULL as there.  VSM_EARG: as there, and params as above.  Both
 * results stay as they are. */
int vsm_points_resect(vsm_handle *h, const vsm_p_match *const *lists, const int32_t *counts, const double *poses, const uint8_t *pose_valid,
                      const uint8_t *refine, double f, double cu, double cv, const vsm_resect_params *params);
/* the handle's last resection result: the number of frames; the arrays (any may be NULL; returns the number of frames):
 * status[F], poses[F][12], updates[F], rows[F], used[F], ss_before[F], ss_after[F], rms_before[F], rms_after[F] */
int32_t vsm_resect_count(vsm_handle *h);
int32_t vsm_resect_get(vsm_handle *h, int32_t *status, double *poses, int32_t *updates, int32_t *rows, int32_t *used, double *ss_before,
                       double *ss_after, double *rms_before, double *rms_after);
/* frames per status value 0..6 */
void vsm_resect_get_stats(vsm_handle *h, int64_t *out7);
/* wall-clock split of the last call, microseconds: {gather + grouping + packing, upload, kernel, download + host part} */
void vsm_resect_get_timings(vsm_handle *h, double *out4);
/* The same definition on one host thread: no GPU, no handle (the CPU suite's subject and the device path's second opinion -
 * not a fallback).  Returns n_frames, or VSM_EARG with the output arrays untouched.  Outputs may be NULL. */
int32_t vsm_host_resect(int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *refine, double f, double cu, double cv,
                        int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv, const double *xyz,
                        const uint8_t *use, const vsm_resect_params *params, int32_t *status, double *out_poses, int32_t *updates,
                        int32_t *rows, int32_t *used, double *ss_before, double *ss_after, double *rms_before, double *rms_after);
/* ---- vetting of observations by reprojection error, and the pruned track set ----
 * The step between rounds of adjustment: the residual of every observation at the given poses and points, a verdict per
 * observation, per track and per frame, and the track set with the outliers taken out.  No counterpart in the reference.
 * csrc/vsm_vet.h is the one statement of the arithmetic; what follows is the contract.
 * Input: as vsm_resect_run takes it, without refine - n_frames poses (camera to world, 12 doubles each), pose_valid (NULL:
 * all valid), f, cu, cv, the tracks (offsets[T + 1], obs_frames, uv), xyz[T][3], use[T] bytes (NULL: all).
 * A frame's state is [Rw | tw], the rigid inverse of its pose as the resection forms it; observation i of track t in frame g
 * is a row of the resection: Xc = Rw X + tw, ru = u - (f xc / zc + cu), rv = v - (f yc / zc + cv).  Its CODE, the first that
 * applies:
 *   1  the track is not in use (use[t] == 0)
 *   2  frame g has no valid pose
 *   3  behind the camera: not zc > min_depth (a NaN point lands here: its depth is NaN)
 *   4  gated: not ru^2 + rv^2 < max_residual^2 (max_residual = 0: below infinity) - NaN and infinite pixels, and
 *      infinite residuals of whatever origin, land here by the comparison alone
 *   0  inlier: exactly the rows the resection uses at these poses with the same max_residual and min_depth
 * and r2, the float of the double ru^2 + rv^2 for codes 0 and 4, 0 for 1..3 (a NaN's sign and payload are not defined).
 * Per track: n_in, the number of inliers; frame_lo / frame_hi, the smallest / largest frame among them (-1, -1 without
 * any); worst, the largest double ru^2 + rv^2 among them (0 without any); ss, their sum in one fixed order: partial[l], l =
 * 0..15, adds the inliers whose position in the track i - offsets[t] is l mod 16, ascending, from +0.0 (a non-inlier is
 * passed over); then partial[l] += partial[l + s] for l < s, s = 8, 4, 2, 1; ss = partial[0].  The track's STATUS, the first
 * that applies:
 *   1  not in use
 *   2  n_in < min_observations
 *   3  all inliers in one frame (frame_lo == frame_hi): observations are match ends, a feature appears once per pair it
 *      takes part in, so two inliers need not be two views
 *   0  kept
 * Per frame three int32 counts of its observations: {inliers, behind (code 3), gated (code 4)}.
 * The pruned track set, over the same T tracks (so xyz and every per-track array stay aligned): kept_offsets[T + 1] - a
 * kept track has length n_in, every other track length 0 -, and kept_index[n_kept], the original indices of the kept
 * tracks' inliers, ascending. */
typedef struct vsm_vet_params {
  double max_residual;      /* 2.0 pixels; 0 = no gate, as in the resection */
  double min_depth;         /* 1e-10 */
  int32_t min_observations; /* 2: the inliers a track needs */
} vsm_vet_params;
void vsm_vet_default_params(vsm_vet_params *p);
/* The general form, on the caller's arrays.  Runs on the handle's device and stream: one copy up (97 bytes per frame, 12 per
 * observation, 29 per track), the kernels (a 16-lane group per track for the verdicts, the tracks' multi-level scan over
 * the kept lengths, the groups once more for kept_index), one copy back at the results' upper bounds - the call waits once,
 * at its end.  It has no CPU path.  VSM_EARG, nothing enqueued and the last result kept: what vsm_resect_run rejects for
 * these arrays, params NULL, min_observations < 1, max_residual negative or NaN, min_depth NaN.  VSM_EHIP after a HIP error
 * (nothing further is launched; there is then no result).  Nothing else of the handle is touched: not the streaming ring,
 * the pairs lists, the track, point, resect or motions results. */
int vsm_vet_run(vsm_handle *h, int32_t n_frames, const double *poses, const uint8_t *pose_valid, double f, double cu, double cv, int32_t n_tracks,
                const int32_t *offsets, const int32_t *obs_frames, const float *uv, const double *xyz, const uint8_t *use,
                const vsm_vet_params *params);
/* The same on the handle's last track and point results: use = the point's status is 0, xyz the points, the pixels read from
 * the match lists exactly as vsm_points_resect reads them (lists, counts: as there).  VSM_ENOTREADY and VSM_EARG as there,
 * with params as above.  Both results stay as they are. */
int vsm_points_vet(vsm_handle *h, const vsm_p_match *const *lists, const int32_t *counts, const double *poses, const uint8_t *pose_valid,
                   double f, double cu, double cv, const vsm_vet_params *params);
/* the handle's last vetting result (zeros / nothing written without one); any output may be NULL.
 * count: T, n_obs, n_kept.  get_obs: code[n_obs] (bytes), r2[n_obs]; returns n_obs.  get_tracks: status[T], n_in[T],
 * frame_lo[T], frame_hi[T], ss[T], worst[T]; returns T.  get_frames: counts[F][3]; returns F.  get_kept: kept_offsets[T + 1],
 * kept_index[n_kept]; returns n_kept. */
void vsm_vet_count(vsm_handle *h, int32_t *n_tracks, int32_t *n_obs, int32_t *n_kept);
int32_t vsm_vet_get_obs(vsm_handle *h, uint8_t *code, float *r2);
int32_t vsm_vet_get_tracks(vsm_handle *h, int32_t *status, int32_t *n_in, int32_t *frame_lo, int32_t *frame_hi, double *ss, double *worst);
int32_t vsm_vet_get_frames(vsm_handle *h, int32_t *counts3);
int32_t vsm_vet_get_kept(vsm_handle *h, int32_t *kept_offsets, int32_t *kept_index);
/* observations per code 0..4, then tracks per status 0..3 */
void vsm_vet_get_stats(vsm_handle *h, int64_t *out9);
/* wall-clock split of the last call, microseconds: {gather / packing, upload, kernels, download + host part} */
void vsm_vet_get_timings(vsm_handle *h, double *out4);
/* The same definition on one host thread: no GPU, no handle (the CPU suite's subject and the device path's second opinion -
 * not a fallback).  frame_counts[F][3], kept_offsets[T + 1], kept_index[n_obs] (room for the upper bound), *n_kept.  Returns
 * T, or VSM_EARG with the outputs untouched.  Outputs may be NULL. */
int32_t vsm_host_vet(int32_t n_frames, const double *poses, const uint8_t *pose_valid, double f, double cu, double cv, int32_t n_tracks,
                     const int32_t *offsets, const int32_t *obs_frames, const float *uv, const double *xyz, const uint8_t *use,
                     const vsm_vet_params *params, uint8_t *code, float *r2, int32_t *status, int32_t *n_in, int32_t *frame_lo,
                     int32_t *frame_hi, double *ss, double *worst, int32_t *frame_counts, int32_t *kept_offsets, int32_t *kept_index,
                     int32_t *n_kept);
/* The frame and the pixel of every observation of the handle's last track result, as vsm_tracks_triangulate gathers them
 * (host only; lists, counts: as there): what a caller of the handle forms needs to build the pruned arrays.  obs_frames_out[n_obs],
 * uv_out[n_obs][2], either may be NULL.  Returns n_obs, or VSM_ENOTREADY / VSM_EARG as vsm_tracks_triangulate does for the
 * lists. */
int32_t vsm_tracks_pixels(vsm_handle *h, const vsm_p_match *const *lists, const int32_t *counts, int32_t *obs_frames_out, float *uv_out);
/* ---- joint adjustment of poses and points ----
 * Poses and points move together: damped Gauss-Newton (Levenberg-Marquardt) rounds on the rows of the resection, the points
 * eliminated (Schur complement) and the reduced camera system solved by preconditioned conjugate gradients without ever
 * forming its matrix.  No counterpart in the reference.  csrc/vsm_ba.h is the one statement of the arithmetic (every product,
 * every sum and its order; only + - * / on doubles, so the device equals the host view bit for bit); what follows is the contract.
 * Input: exactly what vsm_resect_run takes.  State: per frame [Rw | tw], the rigid inverse of the input pose; per track X.
 * A ROW is an observation of a track in use in a frame with a valid pose.  One ROUND:
 *  - linearise: a row is ACTIVE if the resection would use it at the state (zc > min_depth, ru^2 + rv^2 < max_residual^2);
 *    the active set then stands for the whole round.  Per active row: Jc (2x6, the resection's), Jp (2x3, the derivative of
 *    the prediction by X), W = Jc^T Jp.  Per frame, over its active rows in the resection's order (256 partial sums, the
 *    tree): U = Jc^T Jc, gc = Jc^T r and the cost, the resection's 28 sums.  Per track, over its active observations
 *    ascending: V = Jp^T Jp, gp = Jp^T r.  The diagonals of U and V are multiplied by 1 + lambda.
 *  - a frame is FREE in the round if it is valid, asked for, has at least min_observations active rows and its damped U has
 *    a pivot (Gauss-Jordan, full pivoting, eps 1e-20); a track is free if it is in use, has at least min_track_observations
 *    active observations and its damped V has a pivot.  Everything else is HELD: its update is zero, its rows still count
 *    in the sums of the other side and in the cost.
 *  - solve (U - W V^-1 W^T) x = gc - W V^-1 gp over the free frames by conjugate gradients preconditioned with U^-1 per frame,
 *    from x = 0.  Scalar products: partial[l], l = 0..255, adds the products of the entries 6 g + m with (6 g + m) mod 256 == l
 *    ascending (held frames are passed over), then the tree.  It ends at the first of: rz <= cg_tol^2 rz0 (end 1); p.q not
 *    positive and finite, x kept as it stands (end 2); cg_iters iterations (end 3).
 *  - dX = V^-1 (gp - W^T x); trial poses by the resection's Cayley step of x, trial points X + dX.
 *  - the trial cost runs over the same active rows; one of them behind the camera (not zc > min_depth) rejects the step.
 *    Accepted if the trial cost is finite and strictly below the cost: lambda = max(lambda / 10, lambda_min); else the state
 *    is kept and lambda *= 10.
 * The call stops after an accepted round with cost - trial <= ftol * cost (stop 1), when lambda > lambda_max (stop 2), or
 * after max_rounds rounds (stop 3).
 * Frame status, from the last round: 1 no valid pose, 2 not asked for, 3 fewer than min_observations rows (the resection's
 * numbers), 7 held in the last round (too few active rows, or no pivot), 0 free in the last round.  Track status, from the
 * last round: 1 not in use, 2 fewer than min_track_observations active observations, 3 no pivot, 0 free.
 * Results: per frame status, pose[12] (camera to world: the rigid inverse of the final state if an accepted round moved the
 * frame, else the input pose's bytes), rows, active (the active rows of the last round); per track status and xyz[3] (the
 * input point's bytes unless an accepted round moved it); per round run the history: cost before, cost after (the trial
 * cost if accepted, else the cost before - it never rises), lambda of the round, the CG's iterations, how it ended (1..3),
 * accepted (0 / 1), active rows. */
typedef struct vsm_adjust_params {
  int32_t min_observations;       /* 10: the active rows a free frame needs (at least 6) */
  int32_t min_track_observations; /* 2: the active observations a free track needs */
  int32_t max_rounds;             /* 10 */
  int32_t cg_iters;               /* 40 */
  double lambda0;                 /* 1e-3 */
  double lambda_min;              /* 1e-9 */
  double lambda_max;              /* 1e6 */
  double cg_tol;                  /* 1e-2 */
  double ftol;                    /* 1e-6 */
  double max_residual;            /* 0 = no gate (pixels) */
  double min_depth;               /* 1e-10 */
} vsm_adjust_params;
void vsm_adjust_default_params(vsm_adjust_params *p);
/* The general form, on the caller's arrays (the argument list of vsm_resect_run).  Runs on the handle's device and stream:
 * the rows grouped by frame as the resection groups them (16 bytes per row: the observation's index rides along), one copy
 * up, the rounds' kernels with one wait per round on a control block of the device (launches behind a finished solve or a
 * finished call do nothing; option "adjust_fixed" = 1: every launch of max_rounds rounds enqueued at once and one wait, the
 * same bytes), one copy back.  It has no CPU path.  VSM_EARG, nothing enqueued and the last result kept: what
 * vsm_resect_run rejects for these arrays, params NULL, min_observations < 6, max_rounds < 1, cg_iters < 1, lambda0, cg_tol
 * or ftol not positive or not finite.  Nothing else of the handle is touched. */
int vsm_adjust_run(vsm_handle *h, int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *refine, double f, double cu,
                   double cv, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv, const double *xyz,
                   const uint8_t *use, const vsm_adjust_params *params);
/* The same on the handle's last track and point results, found exactly as vsm_points_resect finds them; VSM_ENOTREADY and
 * VSM_EARG as there, with params as above.  Both results stay as they are. */
int vsm_points_adjust(vsm_handle *h, const vsm_p_match *const *lists, const int32_t *counts, const double *poses, const uint8_t *pose_valid,
                      const uint8_t *refine, double f, double cu, double cv, const vsm_adjust_params *params);
/* the handle's last adjustment (zeros / nothing written without one); any output may be NULL.  count: F, T, rounds run.
 * get_frames: status[F], poses[F][12], rows[F], active[F]; returns F.  get_tracks: status[T], xyz[T][3]; returns T.
 * get_history, per round run: cost_before, cost_after, lambda (doubles), cg_iters, cg_end, accepted, active (int32); returns
 * the rounds run. */
void vsm_adjust_count(vsm_handle *h, int32_t *n_frames, int32_t *n_tracks, int32_t *n_rounds);
int32_t vsm_adjust_get_frames(vsm_handle *h, int32_t *status, double *poses, int32_t *rows, int32_t *active);
int32_t vsm_adjust_get_tracks(vsm_handle *h, int32_t *status, double *xyz);
int32_t vsm_adjust_get_history(vsm_handle *h, double *cost_before, double *cost_after, double *lambda, int32_t *cg_iters, int32_t *cg_end,
                               int32_t *accepted, int32_t *active);
/* frames per status value 0..7, tracks per status value 0..3, rounds run, rounds accepted, why it stopped (1..3), CG
 * iterations in all */
void vsm_adjust_get_stats(vsm_handle *h, int64_t *out16);
/* wall-clock split of the last call, microseconds: {gather + grouping + packing, upload, kernels (with the waits per round),
 * download + host part} */
void vsm_adjust_get_timings(vsm_handle *h, double *out4);
/* The same definition on one host thread: no GPU, no handle (the CPU suite's subject, the device path's second opinion and
 * the benchmark's baseline - not a fallback).  history arrays: room for max_rounds entries; *n_rounds the rounds run;
 * stats16 as vsm_adjust_get_stats.  Returns n_frames, or VSM_EARG with the outputs untouched.  Outputs may be NULL. */
int32_t vsm_host_adjust(int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *refine, double f, double cu, double cv,
                        int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const float *uv, const double *xyz,
                        const uint8_t *use, const vsm_adjust_params *params, int32_t *frame_status, double *out_poses, int32_t *rows,
                        int32_t *active, int32_t *track_status, double *out_xyz, double *cost_before, double *cost_after, double *lambda,
                        int32_t *cg_iters, int32_t *cg_end, int32_t *accepted, int32_t *round_active, int32_t *n_rounds, int64_t *stats16);
/* ---- location of frames without a pose against the points ----
 * The call that gives a frame a pose: every stage behind the motions takes pose_valid and has a status of its own for a frame
 * without one, this one estimates the pose of every asked-for frame from its observations of known 3-D points alone -
 * RANSAC over a linear six-point resection, inliers counted by the resection's row test, the winner handed to the
 * resection's update loop.  No counterpart in the reference.  csrc/vsm_locate.h is the one statement of the arithmetic (every
 * product, every sum and its order); what follows is the contract.
 * Input: what vsm_resect_run takes without poses and pose_valid - n_frames; locate, a byte per frame (NULL: all frames); f, cu,
 * cv; the tracks (offsets[T + 1], obs_frames, uv); xyz[T][3]; use[T] bytes (NULL: all).
 * A frame's ROWS are the resection's rows in the resection's grouping and order.  A row is ELIGIBLE if u, v and the three
 * coordinates of its point are finite; E is the frame's number of eligible rows, and position q in [0, E) names the q-th
 * eligible row in row order.
 * Sampling (host): every located frame owns a minstd state (x <- 16807 x mod 2^31 - 1) that starts at seed mod 2^31 - 1, or
 * at 1 where that is 0.  Hypothesis k = 0, 1, .. draws six distinct positions in [0, E) the way the egomotion's
 * getRandomSample draws: a partial Fisher-Yates on the identity deck of E cards, draw i (i = 0..5) uniform in [i, E - 1] by
 * std::uniform_int_distribution's rejection on the engine, the deck put back after each hypothesis.  No process-wide sampler is
 * read, so frame order, chunking and thread count cannot matter.
 * Fit, per (frame, hypothesis), from the six sampled rows i = 0..5 in sample order:
 *  1. x = (u - cu) / f, y = (v - cv) / f, in double.
 *  2. m = (((((X0 + X1) + X2) + X3) + X4) + X5) / 6 per coordinate; s = the largest |coordinate - m| over the eighteen.  The
 *     hypothesis is INVALID if s is not above zero or not below infinity (six identical points; an overflowed mean).  X' = (X - m) / s.
 *  3. The 12 x 12 matrix A, zero but for: row 2i = [X' 1, 0 0 0 0, -x X' -x], row 2i + 1 = [0 0 0 0, X' 1, -y X' -y].
 *  4. Its singular value decomposition by Matrix::svd's arithmetic (vsm_la::svd_nr), which leaves the singular values in
 *     decreasing order, equal ones in the order the routine's shell sort leaves them; p = column 11 of V, the right singular
 *     vector of the smallest singular value - picked exactly as the fundamental-matrix fit picks its ninth column.
 *  5. M = the left 3 x 3 block of p read as 3 x 4 (M[i][j] = p[4 i + j]); M = U diag(w) V^T by the same routine; R0 = U V^T
 *     (every entry summed over k ascending from the k = 0 product); d = det R0 by cofactors along row 0; sigma = 1 if d > 0,
 *     else -1; R = sigma R0; lambda = sigma (3 / ((w0 + w1) + w2)).
 *  6. tw[i] = (lambda p[4 i + 3]) s - ((R[i][0] m0 + R[i][1] m1) + R[i][2] m2).
 * The state [R | tw] is world to camera, as the resection's.  The hypothesis is VALID if its twelve numbers are finite and
 * all six sampled rows have zc > min_depth at it; an invalid hypothesis counts 0.
 * Count: the number of the frame's eligible rows that the resection would use at [R | tw] with max_residual =
 * inlier_threshold and min_depth (zc > min_depth and ru^2 + rv^2 < inlier_threshold^2).
 * Winner: the first hypothesis with strictly more inliers than all before it (none if every count is 0).
 * Refinement: the winner's state becomes the LINEAR POSE by the rigid inverse, as the resection forms poses, and is handed to
 * the resection exactly as a caller would hand it: refine = this frame alone, max_residual = inlier_threshold,
 * min_observations = min_inliers, max_updates, eps and min_depth as given.  So the located poses equal vsm_host_resect's
 * from the linear poses byte for byte.
 * Per frame, the first status that applies wins:
 *   1  not asked for (locate == 0)
 *   2  E < min_inliers
 *   3  no valid hypothesis
 *   4  the winner counts fewer than min_inliers (or every count is 0)
 *   5  the resection ended in its status 4 or 5: the pose is the linear one
 *   6  not converged after max_updates updates: the estimate as it stands
 *   0  located
 * Results per frame: status; pose[12], camera to world, zeros for 1..4; linear_pose[12], zeros where there is no winner;
 * best, the winner's index or -1; inliers, the winner's count; rows; eligible = E (0 for status 1); updates, used, ss_after as
 * the resection reports them (0 for 1..4); rms_after, libm's sqrt(ss_after / used) applied by the host (status 0, 6; else 0).
 * Known limit: the linear six-point fit is degenerate for coplanar points (the matrix then has a null space of four
 * dimensions, and the vector the decomposition returns is an arbitrary member of it): a planar scene ends in status 3 or 4. */
typedef struct vsm_locate_params {
  int32_t ransac_iters;     /* 200; at least 1 */
  double inlier_threshold;  /* 2.0 pixels; positive and finite */
  int32_t min_inliers;      /* 10; at least 6 */
  double min_depth;         /* 1e-10 */
  uint32_t seed;            /* 71 */
  int32_t max_updates;      /* 20; at least 1 */
  double eps;               /* 1e-8; positive and finite */
} vsm_locate_params;
void vsm_locate_default_params(vsm_locate_params *p);
/* The general form, on the caller's arrays.  Runs on the handle's device and stream: the host groups the rows by frame as the
 * resection does, finds the eligible rows and draws the samples on the pool (timed with the packing), one copy up (per frame
 * 16 bytes, per row 12, per track 24, per (located frame, hypothesis) 24, per tile of 256 rows 8), the kernels - a 16-lane
 * group per (frame, hypothesis) for the fit, (tiles of 256 rows) x (runs of 16 hypotheses) for the counts, a workgroup per
 * frame for the winner, the resection's kernel on the device-resident linear poses -, one copy back (236 bytes per frame),
 * one wait.  It has no CPU path.  VSM_EARG, nothing enqueued and the last result kept: what vsm_resect_run rejects for
 * these arrays, params NULL, ransac_iters < 1, inlier_threshold not positive or not finite, min_inliers < 6, max_updates < 1,
 * eps not positive or not finite.  VSM_EHIP after a HIP error.  Nothing else of the handle is touched. */
int vsm_locate_run(vsm_handle *h, int32_t n_frames, const uint8_t *locate, double f, double cu, double cv, int32_t n_tracks, const int32_t *offsets,
                   const int32_t *obs_frames, const float *uv, const double *xyz, const uint8_t *use, const vsm_locate_params *params);
/* The same on the handle's last track and point results, found exactly as vsm_points_resect finds them (lists, counts: as
 * there); VSM_ENOTREADY and VSM_EARG as there, with params as above.  Both results stay as they are. */
int vsm_points_locate(vsm_handle *h, const vsm_p_match *const *lists, const int32_t *counts, const uint8_t *locate, double f, double cu, double cv,
                      const vsm_locate_params *params);
/* the handle's last location result: the number of frames; the arrays (any may be NULL; returns the number of frames):
 * status[F], poses[F][12], linear_poses[F][12], best[F], inliers[F], rows[F], eligible[F], updates[F], used[F], ss_after[F],
 * rms_after[F] */
int32_t vsm_locate_count(vsm_handle *h);
int32_t vsm_locate_get(vsm_handle *h, int32_t *status, double *poses, double *linear_poses, int32_t *best, int32_t *inliers, int32_t *rows,
                       int32_t *eligible, int32_t *updates, int32_t *used, double *ss_after, double *rms_after);
/* frames per status value 0..6 */
void vsm_locate_get_stats(vsm_handle *h, int64_t *out7);
/* wall-clock split of the last call, microseconds: {gather + grouping + sampling + packing, upload, kernels, download + host part} */
void vsm_locate_get_timings(vsm_handle *h, double *out4);
/* The same definition on one host thread: no GPU, no handle (the CPU suite's subject, the device path's second opinion and the
 * benchmark's baseline - not a fallback).  Returns n_frames, or VSM_EARG with the output arrays untouched.  Outputs may be NULL. */
int32_t vsm_host_locate(int32_t n_frames, const uint8_t *locate, double f, double cu, double cv, int32_t n_tracks, const int32_t *offsets,
                        const int32_t *obs_frames, const float *uv, const double *xyz, const uint8_t *use, const vsm_locate_params *params,
                        int32_t *status, double *poses, double *linear_poses, int32_t *best, int32_t *inliers, int32_t *rows, int32_t *eligible,
                        int32_t *updates, int32_t *used, double *ss_after, double *rms_after);
/* ---- re-observation: new observations of the points, found by projection ----
 * Every stage behind the matcher consumes observations and the vetting removes them; this one adds them.  A point in use is
 * projected into every searched frame with a pose that does not observe it yet; among that frame's features near the
 * projection, the one whose descriptor is nearest the track's becomes a new observation.  No counterpart in the reference,
 * whose Reconstruction links consecutive frames only; the cost is the matcher's (Matcher::findMatch, viso/matcher.cpp:892-963):
 * the sum of absolute differences of the 32 descriptor bytes between features of one class.  csrc/vsm_reobserve.h is the one
 * statement of the arithmetic; what follows is the contract.
 * Input: as vsm_vet_run takes it - n_frames poses (camera to world, 12 doubles each), pose_valid (NULL: all valid), f, cu,
 * cv, the tracks' offsets[T + 1] and obs_frames, xyz[T][3], use[T] bytes (NULL: all) - and search, a byte per frame (NULL:
 * all): only frames with a non-zero byte are searched; the image's width and height, 1..16383; obs_feat[n_obs], the feature
 * index of each observation within its frame (column 1 of vsm_tracks_get's obs); ref_obs[T], the observation whose feature
 * lends the track its class and descriptor, an index into the track, 0 <= ref_obs[t] < length (NULL: the middle one,
 * (length - 1) / 2); and the features: feat_offsets[F + 1] and feat[n_feat][12], int32 records {u, v, 0, class, d1..d8}
 * exactly as vsm_get_features hands them out - image pixels, class 0..3, the 32 descriptor bytes in d1..d8.  A track without
 * observations has no reference: it counts as not in use.
 * Feature k of frame g is OCCUPIED if any observation of any track, in use or not, names (g, k); an occupied feature is never
 * found.  A CANDIDATE is a pair (t, g) with use[t] != 0, search[g] != 0, a valid pose of g, g not a frame of track t, and, with
 * [Rw | tw] the rigid inverse of the pose as the resection forms it and Xc = Rw X + tw: zc > min_depth, and pu = f xc / zc + cu,
 * pv = f yc / zc + cv with 0 <= pu <= width - 1 and 0 <= pv <= height - 1 (NaN fails by the comparison).  The candidates are
 * listed in ascending (t, g).  A candidate's WINDOW is the set of features k of frame g that are not occupied, have the
 * class of the track's reference feature, and satisfy u_k - pu <= radius, pu - u_k <= radius and the same in v, in double.
 * The COST of k is the sum over the 32 descriptor bytes of |a - b|, 0..8160.  best is the smallest (cost, k) - the lowest
 * index wins a tie -, second the smallest cost among the window's other features (-1: none), n_window the window's size.
 * The candidate's CODE, the first that applies:
 *   1  the window is empty (feature, cost and second are -1)
 *   2  max_cost > 0 and best cost > max_cost
 *   3  ratio_den > 0, there is a second, and not best * ratio_den < second * ratio_num (in 64-bit integers)
 *   4  lost: among the candidates that come this far naming the same (g, k), the smallest (cost, candidate index) keeps the
 *      feature; the others do not fall back to their second
 *   0  accepted
 * Results: per candidate seven int32 {track, frame, feature, cost, second, n_window, code} and the doubles (pu, pv); per
 * track the number accepted; per frame {candidates, accepted}. */
typedef struct vsm_reobserve_params {
  double radius;      /* 4.0 pixels: half the side of the window, finite and not negative */
  double min_depth;   /* 1e-10 */
  int32_t max_cost;   /* 0 = no cap */
  int32_t ratio_num;  /* 0 / 0 = no ratio test; else best / second has to be below ratio_num / ratio_den */
  int32_t ratio_den;
} vsm_reobserve_params;
void vsm_reobserve_default_params(vsm_reobserve_params *p);
/* The general form, on the caller's arrays.  Runs on the handle's device and stream: one copy up (110 bytes per frame, 8 per
 * observation, 33 per track, 48 per feature), the kernels - the occupied features, a counting sort of the free ones by
 * (frame, class, bin), a 16-lane group per track for the projections, the tracks' multi-level scan over the tracks' counts -,
 * the call's one wait in the middle for the number of candidates, which sizes their block (44 bytes each), then the list,
 * a 16-lane group per candidate for the search, a lane per candidate for the verdict, one copy back.  It has no CPU path.
 * VSM_EARG, nothing enqueued and the last result kept: what vsm_vet_run rejects for the shared arrays, params NULL, radius not
 * finite or negative, min_depth NaN, max_cost < 0, a negative ratio term or ratio_den > 0 with ratio_num <= 0, width or
 * height outside 1..16383, feat_offsets not starting at 0 or decreasing, an obs_feat or ref_obs out of range, a class
 * outside 0..3, a feature pixel outside the image, and more than 2^31 - 1 pairs of a track in use and a searched frame with
 * a pose (search fewer frames per call).  VSM_EHIP after a HIP error, a block the device cannot hold included (nothing
 * further is launched; there is then no result).  Nothing else of the handle is touched. */
int vsm_reobserve_run(vsm_handle *h, int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *search, double f, double cu, double cv,
                      int32_t width, int32_t height, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const int32_t *obs_feat, const double *xyz,
                      const uint8_t *use, const int32_t *ref_obs, const int32_t *feat_offsets, const int32_t *feat, const vsm_reobserve_params *params);
/* The same on the handle's own results: the tracks of the last vsm_pairs_tracks with side 0, xyz and use (status 0) from the
 * last point result, ref_obs NULL, and the features where the last vsm_pairs_run left them - set 1 of the left image of every
 * frame, resident in HBM: nothing is uploaded for them; width and height are that run's.  VSM_ENOTREADY: no such pairs run,
 * track result or point result, tracks not from those pairs or of side 1, lists replaced since, or a run that took the
 * whole-call per-frame path (more than 1024 statistics bins), which leaves no resident features.  VSM_EARG for params and a
 * NULL poses.  The lists and the other stages' results stay as they are. */
int vsm_points_reobserve(vsm_handle *h, const double *poses, const uint8_t *pose_valid, const uint8_t *search, double f, double cu, double cv,
                         const vsm_reobserve_params *params);
/* the handle's last re-observation result (zeros / nothing written without one); any output may be NULL.
 * count: the candidates, the accepted among them.  get: cand[n_cand][7], uv[n_cand][2]; returns n_cand.  get_tracks:
 * accepted[T]; returns T.  get_frames: counts[F][2]; returns F. */
void vsm_reobserve_count(vsm_handle *h, int32_t *n_cand, int32_t *n_accepted);
int32_t vsm_reobserve_get(vsm_handle *h, int32_t *cand7, double *uv);
int32_t vsm_reobserve_get_tracks(vsm_handle *h, int32_t *accepted);
int32_t vsm_reobserve_get_frames(vsm_handle *h, int32_t *counts2);
/* pairs (t, g) of tracks in use per reason they are no candidates, the first that applies - search[g] == 0, no valid pose, g
 * already a frame of the track, behind the camera, outside the image -, then candidates per code 0..4 */
void vsm_reobserve_get_stats(vsm_handle *h, int64_t *out10);
/* wall-clock split of the last call, microseconds: {gather / packing, upload, kernels with the one wait for the number of
 * candidates, download + host part} */
void vsm_reobserve_get_timings(vsm_handle *h, double *out4);
/* The same definition on one host thread: no GPU, no handle (the CPU suite's subject and the device path's second opinion -
 * not a fallback).  cand[cap][7] and cand_uv[cap][2] take the first cap candidates; track_accepted[T], frame_counts[F][2],
 * stats10 as above.  Returns the number of candidates (call with cap 0 to size the arrays), or VSM_EARG with the outputs
 * untouched.  Outputs may be NULL. */
int32_t vsm_host_reobserve(int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *search, double f, double cu, double cv, int32_t width,
                           int32_t height, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const int32_t *obs_feat, const double *xyz,
                           const uint8_t *use, const int32_t *ref_obs, const int32_t *feat_offsets, const int32_t *feat, const vsm_reobserve_params *params,
                           int32_t cap, int32_t *cand, double *cand_uv, int32_t *track_accepted, int32_t *frame_counts, int64_t *stats10);
/* The feature records of a frame of the last vsm_pairs_run, in vsm_get_features' layout: side 0 = left, 1 = right; set 0 =
 * sparse, 1 = dense (the set the match lists' indices count in).  num: the number of records; get: up to cap of them into
 * out[cap][12], returns how many.  0 where there is no such run, frame, side or set, or the run left no resident features. */
int32_t vsm_pairs_num_features(vsm_handle *h, int32_t frame, int32_t side, int32_t set);
int32_t vsm_pairs_get_features(vsm_handle *h, int32_t frame, int32_t side, int32_t set, int32_t *out, int32_t cap);
/* ---- fusion: duplicate tracks of one 3-D point joined ----
 * The tracks are connected components of the match graph: where one match is missed a point's track ends, and the point
 * comes back later as a second track with a second point.  The re-observation cannot repair that - the feature it would find
 * is occupied, by the duplicate.  This stage searches exactly those features and joins the two tracks.  No counterpart in
 * the reference.  csrc/vsm_fuse.h states what is new in the arithmetic; projection, window, cost, best and second are the
 * re-observation's, above.
 * Input: exactly what vsm_reobserve_run takes, with the same meanings.  A track without observations is not in use.
 * OWNER(g, k) is the smallest index of a track in use that has an observation (g, k); undefined where there is none.
 * A CANDIDATE is a pair (a, g) as for the re-observation, with the same reasons 0..4 for the pairs that are none.  Its WINDOW
 * is the set of features k of frame g with owner(g, k) defined, the class of a's reference feature, and inside the square of
 * half-side radius around the projection: the complement of the re-observation's window among the features that tracks in
 * use own.  best, second and n_window are as there.  A PROPOSAL is a candidate with a non-empty window; it names
 * b = owner(g, best).  The proposals are listed in ascending (a, g) and numbered in that order.  A proposal's CODE, the first
 * that applies:
 *   2  max_cost > 0 and best cost > max_cost
 *   3  the ratio test fails, as for the re-observation
 *   4  conflict: some frame occurs among the observations of both a and b - the merged track would see one frame twice
 *   5  outbid: among a's proposals that come this far another has the smaller (cost, proposal index); that one is a's choice,
 *      and partner(a) is its b
 *   6  one-sided: partner(b) is not a
 *   0  fused
 * Code 1, an empty window, is counted in the stats only.  The FUSIONS are the pairs {a, b} with partner(a) = b and
 * partner(b) = a: a matching, so no track is in two of them.  The smaller index survives, the larger is absorbed.  A point
 * in three fragments therefore needs two calls: the first joins two of them, the second the third - re-triangulate between.
 * The MERGED TRACK SET covers the same T tracks: a survivor's observations are its own followed by the absorbed track's,
 * stably sorted by frame; an absorbed track is empty; every other track is as it was.  offsets_after[T + 1] and
 * obs_src[n_obs] describe it: obs_src[i] is the input index of observation i of the merged set, a permutation.  xyz is not
 * touched: the caller triangulates the merged set again.
 * Results: per proposal eight int32 {a, g, feature, cost, second, n_window, code, b} and the doubles (pu, pv); per track
 * partner (-1: none) and fused_into (the survivor of an absorbed track, else -1); the merged set; per frame {candidates,
 * proposals}; stats. */
typedef struct vsm_fuse_params {
  double radius;      /* 4.0 pixels: half the side of the window, finite and not negative */
  double min_depth;   /* 1e-10 */
  int32_t max_cost;   /* 0 = no cap */
  int32_t ratio_num;  /* 0 / 0 = no ratio test; else best / second has to be below ratio_num / ratio_den */
  int32_t ratio_den;
} vsm_fuse_params;
void vsm_fuse_default_params(vsm_fuse_params *p);
/* The general form, on the caller's arrays.  Runs on the handle's device and stream: one copy up (as vsm_reobserve_run's),
 * the kernels - the owners by a 32-bit atomic minimum, a counting sort of the owned features by (frame, class, bin), a 16-lane
 * group per track that projects and searches and counts, the scan over the tracks' proposals -, the first wait, for the
 * number of proposals, which sizes their block (48 bytes each), then the list - the proposals the counting pass kept in places
 * per track (48 bytes per pair of a track in use and a searched frame with a pose, device only) moved to their prefix, or,
 * where those places would exceed 2 GiB, the same walk again (handle option "fuse_compact": 1 / 0 force either; the bytes are
 * the same) -, the conflict test, a 64-bit atomic minimum per track for its choice, the verdicts, a scan over the new lengths
 * and a merge per survivor, one copy back, the second wait: two waits, because the proposals' block cannot be sized before
 * their number is known.  The candidates are never listed and never copied: only the proposals reach the host.  It has no
 * CPU path.  VSM_EARG, VSM_EHIP: exactly as vsm_reobserve_run; VSM_EARG leaves the last result in place.  Nothing else of the
 * handle is touched. */
int vsm_fuse_run(vsm_handle *h, int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *search, double f, double cu, double cv,
                 int32_t width, int32_t height, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const int32_t *obs_feat, const double *xyz,
                 const uint8_t *use, const int32_t *ref_obs, const int32_t *feat_offsets, const int32_t *feat, const vsm_fuse_params *params);
/* The same on the handle's own results, as vsm_points_reobserve takes them: the tracks of the last vsm_pairs_tracks with side
 * 0, xyz and use from the last point result, the features resident in HBM.  VSM_ENOTREADY in the same states. */
int vsm_points_fuse(vsm_handle *h, const double *poses, const uint8_t *pose_valid, const uint8_t *search, double f, double cu, double cv,
                    const vsm_fuse_params *params);
/* the handle's last fusion result (zeros / nothing written without one); any output may be NULL.  count: the proposals, the
 * fusions.  get: prop[n_prop][8], uv[n_prop][2]; returns n_prop.  get_tracks: partner[T], fused_into[T]; returns T.
 * get_merged: offsets_after[T + 1], obs_src[n_obs]; returns n_obs.  get_frames: counts[F][2]; returns F. */
void vsm_fuse_count(vsm_handle *h, int32_t *n_prop, int32_t *n_fusions);
int32_t vsm_fuse_get(vsm_handle *h, int32_t *prop8, double *uv);
int32_t vsm_fuse_get_tracks(vsm_handle *h, int32_t *partner, int32_t *fused_into);
int32_t vsm_fuse_get_merged(vsm_handle *h, int32_t *offsets_after, int32_t *obs_src);
int32_t vsm_fuse_get_frames(vsm_handle *h, int32_t *counts2);
/* pairs per reason 0..4 as vsm_reobserve_get_stats, candidates per code 0..6 (code 1: empty windows), the number of fusions */
void vsm_fuse_get_stats(vsm_handle *h, int64_t *out13);
/* wall-clock split of the last call, microseconds: {gather / packing, upload, kernels with the wait for the number of
 * proposals, download + host part} */
void vsm_fuse_get_timings(vsm_handle *h, double *out4);
/* The same definition on one host thread: no GPU, no handle (not a fallback).  prop[cap][8] and prop_uv[cap][2] take the
 * first cap proposals; partner[T], fused_into[T], offsets_after[T + 1], obs_src[n_obs], frame_counts[F][2], stats13 as above.
 * Returns the number of proposals (call with cap 0 to size the arrays), or VSM_EARG with the outputs untouched.  Outputs may
 * be NULL. */
int32_t vsm_host_fuse(int32_t n_frames, const double *poses, const uint8_t *pose_valid, const uint8_t *search, double f, double cu, double cv, int32_t width,
                      int32_t height, int32_t n_tracks, const int32_t *offsets, const int32_t *obs_frames, const int32_t *obs_feat, const double *xyz,
                      const uint8_t *use, const int32_t *ref_obs, const int32_t *feat_offsets, const int32_t *feat, const vsm_fuse_params *params, int32_t cap,
                      int32_t *prop, double *prop_uv, int32_t *partner, int32_t *fused_into, int32_t *offsets_after, int32_t *obs_src, int32_t *frame_counts,
                      int64_t *stats13);
/* Measurement / test switches of a handle.  They are read from the environment once, by vsm_create (VSM_SEQ_V2,
 * VSM_SEQ_CHUNK, VSM_SEQ_DC_STREAMS, VSM_SEQ_SERIAL, VSM_SEQ_GPU_SORTS, VSM_SEQ_EARLY_EXPORT, VSM_FUSED_KEYS); this call changes one
 * afterwards: name = the variable's name without the VSM_ prefix, in lower case ("seq_serial", "seq_chunk", ...).
 * Option-only names (never read from the environment): "front" (0: separate ingest / halving / Sobel passes instead of the
 * fused front end), "dc_gpu", "dc_full", "dc_watchdog_ms", "dc_fault_inject" (the GPU's share of the final stage in the
 * host-shared form), and the scheduling experiments of the GPU-resident form recorded in DESIGN_HISTORY.md 6c:
 * "seq_keys_dma", "seq_keys_pieces", "seq_ties1_null", "seq_ties1_host", "seq_last_first", "seq_export_budget", "seq_first_chunk",
 * "seq_p2_first", "seq_block_after_p2", "seq_warm_gaps" (DESIGN.md 5, 9);
 * "seq_null_stream" (above); "seq_host_pinned" (below, vsm_host_register); "seq_host_inorder" (0: host-resident frames in the
 * run-ahead order of resident input instead of chunk by chunk as they arrive); "match_heads" (1, before the first image: the
 * second matching pass on 64-byte per-bin head records - measured slower); "fused_features" / "feat_order" (0: the separate filter, suppression, record and bin kernels
 * instead of k_feat_dense / k_feat_sparse / k_feat_scan / k_feat_order) and "filter_planes" (1: vsm_push_back keeps the
 * blob / corner responses in HBM for vsm_get_filter_responses; the fused kernels leave them in LDS otherwise).
 * "fused_keys" (VSM_FUSED_KEYS; 1, the default: the batched forms' compactions write the Delaunay chains' keys and the chains'
 * job tables go up ahead of the matching launches; 0: every chain uploads its table and makes its keys itself behind the
 * compaction, which refinement = 2 always does).
 * None of them changes a result.  Returns VSM_OK, or VSM_EARG for an unknown name.  (No counterpart in the reference.) */
int vsm_set_option(vsm_handle *h, const char *name, int32_t value);
/* Host threads near the GPU: the library confines the threads IT creates (host pool, look-ahead poller) to the CPUs of the
 * device's NUMA node (/sys/bus/pci/devices/<bus id>/local_cpulist, within what the process may use; looked up once per
 * process by the first vsm_create; spread over that node's L3 domains, thread i on domain i mod n; VSM_HOST_AFFINITY=1: the
 * node only, =0: off) - on a two-socket MI355X node a rank whose host
 * threads run on the other socket loses 6 % of the look-ahead rate.  The caller's threads are left alone; this returns the
 * CPUs chosen (up to cap of them in out; the return value is how many there are, 0 = none) so that the caller can put the
 * thread that calls vsm_sequence_run there too, as bench.py does. */
int32_t vsm_local_cpus(int32_t *out, int32_t cap);
/* The per-frame calls (vsm_match, vsm_vo_stereo_process) split ONE triangulation - the final Matcher::removeOutliers,
 * viso/matcher.cpp:1207-1377 - over up to eight fork-join threads that all sit in one L3 domain of that node (they take turns
 * on one mesh; domain = the device ordinal mod the domains, so the ranks of one socket take one each; VSM_FJ_DOMAIN=k: domain k,
 * -1: dealt over the domains), each worker on a physical core of its own (cores
 * 1, 2, ... of the domain; VSM_FJ_CORES=0: anywhere in the domain - then two of them may share a core's hardware threads and
 * halve each other between the phases they spin through).  The caller's thread takes part in that work: this returns the
 * CPUs of the domain's core 0, which is left to it (the whole domain with VSM_FJ_CORES=0), and a caller that confines the
 * thread calling vsm_match / vsm_vo_stereo_process to them (sched_setaffinity) saves the transfers between core complexes
 * and never shares a core with a worker - 0.55 -> 0.47-0.50 ms per 1242 x 375 stereo pair, live VO 0.70 -> 0.62 ms per
 * frame; bench.py does for its per-frame legs.
 * Same conventions as vsm_local_cpus; 0 = no such domain (no node found, affinity off, VSM_FJ_DOMAIN=-1). */
int32_t vsm_forkjoin_cpus(int32_t *out, int32_t cap);
/* Host-resident input at the link's rate.  Matcher::pushBack takes pageable host pointers (viso/matcher.cpp:95-181) and so do
 * vsm_push_back / vsm_sequence_run(on_device = 0): pageable memory is gathered into a pinned buffer by the host pool before it
 * can cross PCIe by DMA.  A caller whose images live in a buffer it reuses can page-lock that buffer ONCE
 * (vsm_host_register = hipHostRegister; or allocate it with hipHostMalloc) and promise so with
 * vsm_set_option(handle, "seq_host_pinned", 1): vsm_sequence_run then copies straight out of the caller's memory.  The promise is
 * the caller's: with the option set and pageable images the copies fall back to the runtime's staged path (slow, still correct).
 * Unregister before the buffer is freed.  (No counterpart in the reference.) */
int vsm_host_register(const void *p, uint64_t bytes);
int vsm_host_unregister(const void *p);
/* Device memory the process keeps: large blocks of closed handles and re-created contexts wait in a cache
 * for the next one instead of going back to the driver, whose background clear of released VRAM slows every call for
 * 44 ms per GB.  out[0] = blocks in the cache, out[1] = their bytes, out[2] = large blocks in use.  vsm_device_pool_trim()
 * hands the cached ones back now (an application about to need the memory for itself).  (No counterpart in the reference.) */
void vsm_device_pool_stats(int64_t out[3]);
void vsm_device_pool_trim(void);

/* ---- stage-level views for parity tests (the reference's private members) ---- */

/* m1p1.. / n1p1.. (viso/matcher.h:232-235).  which: 0=1p1 1=2p1 2=1c1 3=2c1 4=1p2 5=2p2 6=1c2 7=2c2;
 * records are int32[12] = {u,v,0,class,d1..d8} (viso/matcher.cpp:716-718). */
int32_t vsm_num_features(vsm_handle *h, int32_t which);
int32_t vsm_get_features(vsm_handle *h, int32_t which, int32_t *out, int32_t cap_records);

/* match list after each private stage of the last vsm_match():
 * 0 pass-1 matching(), 1 pass-1 removeOutliers(), 2 pass-2 matching(), 3 refinement(), 4 final */
void vsm_set_stage_capture(vsm_handle *h, int on); /* stage 2 costs one extra D2H: off by default */
int32_t vsm_stage_size(vsm_handle *h, int32_t stage);
int32_t vsm_stage_get(vsm_handle *h, int32_t stage, vsm_p_match *out, int32_t cap);

/* Matcher::ranges (viso/matcher.h:152-157,245): 16 floats per statistics bin */
int32_t vsm_num_ranges(vsm_handle *h);
int32_t vsm_get_ranges(vsm_handle *h, float *out, int32_t cap_bins);

/* I?{p,c}_du/_dv[_full] (viso/matcher.h:237-240).  which: 0=1p 1=2p 2=1c 3=2c.  Returns the
 * plane size in bytes (bpl*h) or 0 when absent; du/dv may be NULL to query the size. */
int32_t vsm_get_gradients(vsm_handle *h, int32_t which, int32_t full, uint8_t *du, uint8_t *dv);

/* blob / corner filter responses of the current left image (f1,f2 of viso/matcher.cpp:651-678;
 * transient in the reference - and here: with the default suppression radii they never leave LDS, so set option
 * "filter_planes" = 1 before the push whose responses are wanted).  Returns elements per plane or 0 (none kept). */
int32_t vsm_get_filter_responses(vsm_handle *h, int16_t *f1, int16_t *f2);

/* work counters of the last vsm_match(): {findMatch calls, 0, 0, matches refined, matches out}
 * (slots 1,2 are only counted by the CPU oracle) */
void vsm_get_counters(vsm_handle *h, int64_t *out5);

/* wall-clock split of the last vsm_match() in microseconds:
 * {pass-1 GPU+sync, pass-1 host (Delaunay+prior), pass-2 GPU+sync, final host Delaunay, total} */
void vsm_get_timings(vsm_handle *h, double *out5);

/* per-kernel device time measured with HIP events on the handle's own stream (bench.py's
 * roofline leg).  vsm_set_profiling(h,1) zeroes the accumulators and starts recording; vsm_set_profiling(h, 100 + id)
 * records kernel `id` only (vsm_kernel_name): every span costs two event records on the kernel's stream, and those of
 * all kernels on all streams together disturb the pipeline they measure (1100 + id: also prints every span on stderr). */
void vsm_set_profiling(vsm_handle *h, int on);
int32_t vsm_num_kernels(void);
const char *vsm_kernel_name(int32_t id);
void vsm_get_kernel_stats(vsm_handle *h, double *total_ms, int64_t *launches);

/* host-only view of the exact Delaunay used by removeOutliers (triangulate("zQB") of
 * viso/triangle.cpp:8500 on integer points in [0,16384)^2); needs no GPU.  Returns the number
 * of triangles; tris gets vertex triples by input index. */
int32_t vsm_host_delaunay(const int32_t *x, const int32_t *y, int32_t n, int32_t *tris, int32_t cap, int32_t threads);

/* the same triangulation computed in three steps -- prepare (sort, kd order, tree), independent
 * sub-trees of at most max_task_points points, merges above them -- the form in which the look-ahead
 * path shares the work between host and GPU; must equal vsm_host_delaunay() for every split */
int32_t vsm_host_delaunay_split(const int32_t *x, const int32_t *y, int32_t n, int32_t *tris, int32_t cap,
                                int32_t max_task_points, int32_t device_top_points);

/* test hook for the shared form: (device_kd != 0: the kd order of the sorted keys,) sub-trees (at most
 * max_task_points points) on the GPU, one thread each, then the merge nodes of at most device_top_points points
 * level by level (device_top_points < 0: one wave per sub-tree inside LDS instead, any max_task_points), the rest
 * on the host; -1 on a HIP error */
int32_t vsm_debug_delaunay_gpu(const int32_t *x, const int32_t *y, int32_t n, int32_t *tris, int32_t cap,
                               int32_t max_task_points, int32_t device_top_points, int32_t device_kd);

double vsm_debug_dc_bench(const int32_t *x, const int32_t *y, int32_t n, int32_t max_task_points, int32_t device_top_points,
                          int32_t device_kd, int32_t njobs, int32_t reps);   /* kernel microseconds for njobs triangulations at once */

/* test hooks: which of several matches at one pixel stands for the point in the exact Delaunay (Triangle's
 * randomised vertex sort decides, viso/triangle.cpp:5447 + :6183): (index of the smallest-index match, index of the
 * one the sort puts first) for every pixel where they differ - from the host emulation and from the GPU's
 * (k_dc_ties, one wave; kernel_us may be null); return the count, -1 where the GPU declines (list too long) */
int32_t vsm_host_ties(const int32_t *x, const int32_t *y, int32_t n, int32_t *pairs, int32_t cap);
int32_t vsm_debug_ties_gpu(const int32_t *x, const int32_t *y, int32_t n, int32_t *pairs, int32_t cap, double *kernel_us);

/* Matcher::removeOutliers (viso/matcher.cpp:1207-1377) and Matcher::computePriorStatistics (:734-868) on a match
 * list of the caller: the host code of the per-frame path, and the GPU-resident chain of the look-ahead path
 * (keys, vertex sort - on the device if gpu_ties, else on the host -, kd order, block sub-trees, cached merge levels,
 * support votes, survivors, prior statistics) run on `copies` identical jobs at once.  Test hooks: the two must
 * agree byte for byte.  out gets the survivors, ranges (may be null) the prior boxes in the device layout of the
 * match kernels ([bin][stage][u_min, u_max, v_min, v_max], p->match_radius as given); return the number of
 * survivors, -1 on a HIP error, -2 if the device chain declines the list; kernel_us (may be null): microseconds of
 * the device chain for all copies. */
int32_t vsm_host_outliers_and_prior(const vsm_params *p, const vsm_p_match *list, int32_t n, int32_t method, vsm_p_match *out,
                                    int32_t cap, float *ranges, int32_t w, int32_t h);
/* The same host code the way vsm_match runs it on a frame's final list: `threads` fork-join threads (the caller's among
 * them), the triangulation started from the packed pixels (x | y << 16) alone, flows, votes and the survivors' copy split
 * over the threads.  threads <= 1 is vsm_host_outliers_and_prior.  No GPU needed: the CPU suite compares it with the oracle. */
int32_t vsm_host_outliers_and_prior_threads(const vsm_params *p, const vsm_p_match *list, int32_t n, int32_t method, vsm_p_match *out,
                                            int32_t cap, float *ranges, int32_t w, int32_t h, int32_t threads);
int32_t vsm_debug_dc2(const vsm_params *p, const vsm_p_match *list, int32_t n, int32_t method, int32_t gpu_ties, int32_t copies,
                      vsm_p_match *out, int32_t cap, float *ranges, int32_t w, int32_t h, double *kernel_us);
/* Test hook of the device chain's merge levels: a node's band (the records near its cut) is cached in 256 + f * sqrt(points)
 * LDS lines; a node that needs more is redone by one lane in global memory.  f < 0 restores the default (12); a small f
 * forces that second path, which no list of the benchmark takes.  Process-wide. */
void vsm_debug_dc2_band_factor(int32_t f);
/* Test hook of the exact Delaunay's device predicates (vsm_dc_lds.h, the edge-word mesh of the device chain): for n
 * quadruples of packed points x | y << 16 (coordinates < 2^14) out[i*3..i*3+2] = orientation determinant of a, b, c,
 * sign of the in-circle determinant of a, b, c, d, and 1 if d lies strictly inside the circle through a, b, c, as the
 * GPU computes them.  0, or -1 on a HIP error. */
int32_t vsm_debug_predicates(const uint32_t *quads, int32_t n, int32_t *out);
/* Test hook of the look-ahead call's chunk plan (pure arithmetic, no GPU): how vsm_sequence_run's GPU-resident form cuts
 * n_frames frames into chunks for a host pool of pool_threads threads, frames in HBM (host_in = 0) or in host memory
 * (1), options seq_chunk / seq_first_chunk (0: default) and the plan string of VSM_SEQ_PLAN (NULL: none).  *chunk = the
 * banks' stride, starts[0 .. n] = first frame of each chunk and n_frames; returns the number of chunks n, or -1 (a bad
 * argument, or cap < n + 1). */
int32_t vsm_debug_seq_plan(int32_t n_frames, int32_t pool_threads, int32_t host_in, int32_t seq_chunk, int32_t seq_first_chunk,
                           const char *plan, int32_t *chunk, int32_t *starts, int32_t cap);
/* Test hooks of the matcher's device blocks (pure arithmetic, no GPU, no handle): where every array lies.
 * vsm_debug_ctx_layout: the working set of nframes frame slots (two images each) and npairs frame pairs for frames of
 * w x h pixels under *p, with the dense sets' head records (option match_heads) or without.  Returns what making that
 * working set would: VSM_OK, VSM_EDIMS (a side of 16384 pixels or more, no pixel at the matching resolution) or VSM_EARG
 * (match_binsize outside 1..32768 or more than 2^22 bins, nms_n outside 1..31; also a NULL or negative argument here).
 * With VSM_OK scalars[8] = bytes of the device arena, bytes of the host-mapped result block, bytes from one pair's arrays
 * to the next pair's, elements per plane of the filter responses, floats of a pair's prior boxes, capacity of the sparse
 * and of the dense feature set, queries per pair; *n_rows = the number of arrays, and, if cap >= *n_rows, per array in
 * the order they are placed rows[5] = block (0 the arena, 1 the host-mapped block), image or pair (-1: one per block),
 * feature set (-1: none), byte offset in its block, bytes asked for, and its name in names[16] (as in csrc/vsm_ctx.h; at
 * full resolution imgm is img: it has a row with img's offset and bytes).
 * vsm_debug_dc2_layout: the same for the bank of a Delaunay chain with npairs lists of up to list_cap matches (the look-ahead
 * call rounds that to 1024 before it gets here), with the host's vertex sort (keys and tie patches in host-mapped memory)
 * or without; scalars[6] = bytes of the device block, of the host-mapped block, from one pair's device arrays to the next
 * pair's, ints of a pair's tie patches, bytes from one pair's host keys to the next pair's, and the same for the patches.
 * VSM_OK, or VSM_EARG for a NULL or negative argument. */
int32_t vsm_debug_ctx_layout(const vsm_params *p, int32_t w, int32_t h, int32_t nframes, int32_t npairs, int32_t heads, int64_t *scalars,
                             int64_t *rows, char *names, int32_t cap, int32_t *n_rows);
int32_t vsm_debug_dc2_layout(int32_t npairs, int32_t list_cap, int32_t host_ties, int64_t *scalars, int64_t *rows, char *names, int32_t cap,
                             int32_t *n_rows);
/* Test hook of the batched forms' per-chunk job table (pure arithmetic, no GPU): a look-ahead call of matching method
 * `method` (0 flow, 1 stereo, 2 quad) over frames of `sides` images (1 or 2), cut into n_chunks chunks that start at
 * starts[0 .. n_chunks - 1] and end at starts[n_chunks] = the number of frames, with `banks` frame banks of `chunk` frames
 * each.  counts[frame][side][set]: the feature counts the device would report (set 0 sparse, 1 dense; side 1 is not read
 * with sides = 1); tr_valid: a byte per frame, or NULL (every frame brings a Tr).  The chunks are walked in order, a
 * chunk's counts overwriting its bank's as on the device.  frames_out[frame][7] = image slot of the previous frame, of
 * the frame, queries of the first and the second pass, use_tr, valid, and the frame whose list stands after the frame
 * (-1: none); max_nq_out[chunk][2] = the chunk's longest query lists.  0, or -1 on a bad argument. */
int32_t vsm_debug_chunk_jobs(int32_t method, int32_t multi_stage, int32_t sides, int32_t banks, int32_t chunk, const int32_t *starts,
                             int32_t n_chunks, const int32_t *counts, const uint8_t *tr_valid, int32_t *frames_out, int32_t *max_nq_out);
/* Test hook of vsm_pairs_run's job table (pure arithmetic, no GPU, no HIP call): pairs[n_pairs][2] = (previous, current)
 * frames of a set of n_frames frames of `sides` images whose feature counts are counts[frame][side][set] (as above), cut
 * into chunks of `chunk` pairs; tr_valid: a byte per pair, or NULL (every pair brings a Tr).  pairs_out[pair][7] = image
 * slot of the previous and of the current frame's left image (slot = sides * frame), queries of the first and the second
 * pass, use_tr, valid, and the number (from 1) of the pair whose Tr the job took (0: none); max_nq_out[chunk][2] = the
 * chunk's longest query lists.  Returns the number of chunks, or -1 on an argument vsm_pairs_run rejects. */
int32_t vsm_debug_pair_jobs(int32_t method, int32_t multi_stage, int32_t sides, int32_t n_frames, const int32_t *counts, const int32_t *pairs,
                            int32_t n_pairs, int32_t chunk, const uint8_t *tr_valid, int32_t *pairs_out, int32_t *max_nq_out);
/* Test hooks of the refinement kernels (Matcher::refinement, viso/matcher.cpp:1498-1585) on match lists of the caller.
 * vsm_debug_refine: P pass-2 lists (1 <= P <= 64; lists[k] holds counts[k] matches) as the P pairs of ONE launch, every pair
 * on the handle's current frames as vsm_push_back left them (no vsm_match needed; mono frames serve method 0) through a job
 * table: the relocation (refinement = 1) or the 7 x 7 costs and, always on the device, the fits and the removal of failed
 * matches (refinement = 2), with the handle's refinement and half_resolution.  out[k] (room for counts[k] matches) gets pair
 * k's refined list, out_counts[k] its length.  The handle's last match result (matches, stages) is invalidated.
 * The kernels read around (u1c, v1c) unguarded, so VSM_EARG - before anything is launched, the handle still usable - for: a
 * coordinate that is not finite, a u1c / v1c that is not integer-valued or lies outside [6, w - 7] x [6, h - 7], a count
 * above 16384 or below 0, P outside 1..64, a method outside 0..2, refinement = 0.  The other coordinates may be any finite
 * float (the kernels' margin tests guard them).  VSM_ENOTREADY: the frames the method needs have not been pushed.
 * vsm_debug_refine_check: the list checks alone for frames of w x h pixels (pure arithmetic, no GPU): VSM_OK or VSM_EARG.
 * vsm_debug_parabolic_apply: no images, no handle - k_parabolic_apply over P pairs on the caller's lists and the caller's
 * records[k][counts[k]][3][12] = {status (0 failed, 1 fit, 2 step not applicable), du, dv, c0..c8}; outputs as above.
 * VSM_EARG for a count above 16384 (the kernel would truncate the list) or below 0, P outside 1..64, a NULL argument.
 * vsm_host_parabolic_fits: the host's least-squares tail of the fit (no GPU) on n records [12] = {-, du, dv, c0..c8}:
 * uv[i][2] is updated where the fit succeeds, ok[i] = 1 / 0; returns n, or VSM_EARG. */
int32_t vsm_debug_refine(vsm_handle *h, int32_t method, const vsm_p_match *const *lists, const int32_t *counts, int32_t P,
                         vsm_p_match *const *out, int32_t *out_counts);
int32_t vsm_debug_refine_check(int32_t w, int32_t h, const vsm_p_match *const *lists, const int32_t *counts, int32_t P);
int32_t vsm_debug_parabolic_apply(const vsm_p_match *const *lists, const int32_t *const *records, const int32_t *counts, int32_t P,
                                  vsm_p_match *const *out, int32_t *out_counts);
int32_t vsm_host_parabolic_fits(const int32_t *records, int32_t n, float *uv, int32_t *ok);
/* Test hook of the matching passes' ordered compaction and the Delaunay chains' keys it writes (no images, no handle): P pairs
 * (1 <= P <= 64) in ONE launch, pair k with n_query[k] queries whose acceptance flags flag[k][n_query[k]] and per-query records
 * raw[k][n_query[k]] the caller gives; method 0 / 1 (flow, stereo: with the first-come pixel de-dup) or 2 (quad), pass 0 / 1.
 * Out per pair: list_out[k] (room for n_query[k] + 1 records), count_out[k], keys_out[k] (room for key_cap[k] + 8 words):
 * key[d] = (uint32)(int32)u1c << 34 | (uint32)(int32)v1c << 20 | d for every list position d < min(count, key_cap[k]).  List
 * and key arrays hold 0xA5 bytes before the launch, so everything the kernels leave alone - the record and the eight words
 * behind the arrays, keys from the count or the capacity on - comes back as that pattern.  old_keys = 1: the compaction
 * without its key store and k_dc2_keys behind it (what option fused_keys = 0 runs); the two must agree byte for byte.
 * old_keys = 2: the key store also writes a host-mapped array per pair (the batched forms' pool reads its keys there), and
 * keys_out gets that array.
 * VSM_OK, VSM_EARG, or VSM_EHIP. */
int32_t vsm_debug_compact_keys(int32_t method, int32_t pass, int32_t P, const int32_t *n_query, const int32_t *const *flag,
                               const vsm_p_match *const *raw, const int32_t *key_cap, int32_t old_keys, vsm_p_match *const *list_out,
                               int32_t *count_out, uint64_t *const *keys_out);
/* Test hooks of the location's stages (vsm_locate_run above has the definition): the host view's stages alone, and the three
 * kernels k_locate_fit, k_locate_count and k_locate_winner one by one.  The hooks take rows without tracks: row r of a frame
 * has the pixel rows_uv[r] and the point rows_xyz[r].  VSM_OK, VSM_EARG (nothing is touched, the device included), or
 * VSM_EHIP from a device hook.
 * Host side, one frame, no GPU:
 *   sample: picks[K][6] = the positions hypothesis 0 .. K - 1 of a frame with E eligible rows draws (6 <= E, 1 <= K).
 *   fit:    states[K][12] and valid[K] of the hypotheses picks[K][6] (row indices in [0, n_rows), eligible rows the caller's
 *           business).  states[k] is written whenever step 2 accepts the sample - also for a hypothesis that is invalid
 *           because its state is not finite or a sampled point is not in front - and is UNSPECIFIED (left as it was) where
 *           step 2 refuses it: an overflowed mean, or six identical points whose mean in doubles is the point again (where
 *           the sum of six x, rounded step by step, over 6 is an ulp off x, s is that ulp, the sample goes on and its state is
 *           arbitrary).
 *   count:  counts[k] = the eligible rows among the n_rows that vote for states[k]; 0 where valid[k] is 0.
 * Device side, each ONE launch of one kernel with the call's launch geometry, on allocations of the hook's own: n_frames
 * frames of rows (row_off[n_frames + 1], rows_uv[R][2], rows_xyz[R][3]) and n_jobs jobs, job j on frame job_frame[j] with
 * job_E[j] eligible rows (0: a job without hypotheses), K hypotheses each; at most 2^22 (job, hypothesis) pairs.
 *   fit:    picks[n_jobs][K][6], row indices in the job's frame.  states[n_jobs][K][12] and hvalid[n_jobs][K] go up as the
 *           caller filled them and come back, so what the kernel leaves alone - a job with job_E = 0, the state of a
 *           refused sample - is found again.
 *   count:  states and hvalid given; the tiles are built as the call builds them.  The kernel only ADDS to counts: whoever
 *           launches it clears them first, as vsm_locate_run does before its launches.  The hook clears once and launches
 *           `launches` (1 or 2) times: with 2 every count comes back doubled.
 *   winner: frame_job[n_frames] (-1: not a job), job_E[n_jobs], counts, hvalid and states given, min_inliers; per frame
 *           verdict (-1 no job or job_E = 0, else 3 / 4 / 0), best, inliers, lin_poses[12] and lin_valid.
 * vsm_debug_locate_hypotheses: the tables of the handle's last vsm_locate_run / vsm_points_locate as the call left them, at
 * the call's own launch geometry - n_jobs and n_hyps; picks[n_jobs][K][6] from the pinned block that went up (row indices in
 * the frame), states, hvalid and counts from the device block behind the results.  Any array may be NULL (a first call for
 * the sizes).  The jobs are the asked-for frames with at least min_inliers rows, in frame order; a job with fewer than
 * min_inliers eligible rows has no hypotheses and its entries are unspecified.  VSM_ENOTREADY: the handle holds no location. */
int32_t vsm_host_locate_sample(uint32_t seed, int32_t E, int32_t K, int32_t *picks);
int32_t vsm_host_locate_fit(double f, double cu, double cv, double min_depth, int32_t n_rows, const float *rows_uv, const double *rows_xyz,
                            const int32_t *picks, int32_t K, double *states, uint8_t *valid);
int32_t vsm_host_locate_count(double f, double cu, double cv, int32_t n_rows, const float *rows_uv, const double *rows_xyz, const double *states,
                              const uint8_t *valid, int32_t K, double inlier_threshold, double min_depth, int32_t *counts);
int32_t vsm_debug_locate_fit(double f, double cu, double cv, double min_depth, int32_t n_frames, const int32_t *row_off, const float *rows_uv,
                             const double *rows_xyz, int32_t n_jobs, const int32_t *job_frame, const int32_t *job_E, const int32_t *picks, int32_t K,
                             double *states, uint8_t *hvalid);
int32_t vsm_debug_locate_count(double f, double cu, double cv, int32_t n_frames, const int32_t *row_off, const float *rows_uv, const double *rows_xyz,
                               int32_t n_jobs, const int32_t *job_frame, const int32_t *job_E, int32_t K, const double *states, const uint8_t *hvalid,
                               double inlier_threshold, double min_depth, int32_t launches, int32_t *counts);
int32_t vsm_debug_locate_winner(int32_t n_frames, const int32_t *frame_job, int32_t n_jobs, const int32_t *job_E, int32_t K, int32_t min_inliers,
                                const int32_t *counts, const uint8_t *hvalid, const double *states, int32_t *verdict, int32_t *best, int32_t *inliers,
                                double *lin_poses, uint8_t *lin_valid);
int32_t vsm_debug_locate_hypotheses(vsm_handle *h, int32_t *picks, double *states, uint8_t *hvalid, int32_t *counts, int32_t *n_jobs, int32_t *n_hyps);

/* ---- stereo visual odometry on top of the matcher ----
 * class VisualOdometryStereo, viso/viso_stereo.h:28-88 + viso/viso.h:28-131: process() =
 * pushBack + matchFeatures(2, Tr_delta if valid) + bucketFeatures + getMatches + updateMotion
 * (viso/viso_stereo.cpp:33-40), with estimateMotion's RANSAC / Gauss-Newton
 * (viso/viso_stereo.cpp:42-315) spread over the matcher's host pool. */
typedef struct {
  vsm_params match;              /* VisualOdometry::parameters::match */
  int32_t bucket_max_features;   /* VisualOdometry::bucketing, viso/viso.h:45-54 */
  double bucket_width, bucket_height;
  double f, cu, cv;              /* VisualOdometry::calibration, viso/viso.h:33-42 */
  double base;                   /* VisualOdometryStereo::parameters, viso/viso_stereo.h:33-44 */
  int32_t ransac_iters;
  double inlier_threshold;
  int32_t reweighting;
} vsm_vo_stereo_params;
typedef struct vsm_vo_stereo vsm_vo_stereo;

void vsm_vo_stereo_default_params(vsm_vo_stereo_params *p);
/* VisualOdometryStereo::VisualOdometryStereo, viso/viso_stereo.cpp:27-29 (+ srand(0), viso/viso.cpp:35) */
vsm_vo_stereo *vsm_vo_stereo_create(const vsm_vo_stereo_params *p);
void vsm_vo_stereo_destroy(vsm_vo_stereo *v);
/* VisualOdometryStereo::process, viso/viso_stereo.cpp:33-40; returns 1 (true) / 0 (false) */
int vsm_vo_stereo_process(vsm_vo_stereo *v, const uint8_t *I1, const uint8_t *I2, int32_t width, int32_t height,
                          int32_t bpl, int replace);
int vsm_vo_stereo_process_device(vsm_vo_stereo *v, const uint8_t *dI1, const uint8_t *dI2, int32_t width,
                                 int32_t height, int32_t bpl, int replace);
/* VisualOdometry::process(std::vector<p_match>), viso/viso.h:74-77 */
int vsm_vo_stereo_process_matches(vsm_vo_stereo *v, const vsm_p_match *m, int32_t n);
/* getMotion(): row-major 4x4 Tr_delta, kept from the last success (viso/viso.h:79-87) */
void vsm_vo_stereo_get_motion(vsm_vo_stereo *v, double *T16);
int vsm_vo_stereo_motion_valid(vsm_vo_stereo *v);
/* getNumberOfMatches()/the bucketed p_matched, getNumberOfInliers()/getInlierIndices(), getGain() */
int32_t vsm_vo_stereo_num_matches(vsm_vo_stereo *v);
int32_t vsm_vo_stereo_get_matches(vsm_vo_stereo *v, vsm_p_match *out, int32_t cap);
int32_t vsm_vo_stereo_num_inliers(vsm_vo_stereo *v);
int32_t vsm_vo_stereo_get_inliers(vsm_vo_stereo *v, int32_t *out, int32_t cap);
float vsm_vo_stereo_gain(vsm_vo_stereo *v, const int32_t *inliers, int32_t n);
/* the Matcher inside (VisualOdometry::matcher) */
vsm_handle *vsm_vo_stereo_matcher(vsm_vo_stereo *v);
/* wall-clock split of the last process() in microseconds: {matchFeatures, bucketing + copy,
 * egomotion, total after the push} */
void vsm_vo_stereo_get_timings(vsm_vo_stereo *v, double *out4);
/* VisualOdometry::getRandomSample draws from ONE engine per process, seeded 71
 * (viso/viso.cpp:93); so does this library.  This re-seeds it (parity tests replay fixtures that
 * were recorded from a fresh process). */
void vsm_vo_sampler_seed(uint32_t seed);

/* ---- lock-step multi-sequence stereo visual odometry (multi-sequence per GPU) ----
 * K independent sequences advance together: vsm_multi_process is VisualOdometryStereo::process (viso/viso_stereo.cpp:33-40)
 * for the next stereo pair of EVERY sequence - pushBack, matchFeatures(2, live Tr_delta of that sequence), bucketFeatures,
 * updateMotion - with one launch per kernel over all K pairs and the K egomotion estimates side by side on the host pool.
 * Each sequence has the rand() stream (bucketing, srand(0) at construction, viso/viso.cpp:35) and the RANSAC sampler
 * (viso/viso.cpp:93) that a process of its own would have, so sequence k's matches, inliers and Tr_delta equal what the
 * reference gives for that sequence alone. */
typedef struct vsm_multi vsm_multi;
vsm_multi *vsm_multi_create(const vsm_vo_stereo_params *p, int32_t n_sequences);
void vsm_multi_destroy(vsm_multi *m);
/* left / right: n_sequences images seq_stride bytes apart (sequence k's pair at k * seq_stride), host memory or, with
 * on_device != 0, HBM; ok_out: NULL or n_sequences flags = process()'s return value per sequence */
int vsm_multi_process(vsm_multi *m, const uint8_t *left, const uint8_t *right, int64_t seq_stride, int on_device, int32_t width,
                      int32_t height, int32_t bpl, int32_t *ok_out);
int32_t vsm_multi_num_sequences(vsm_multi *m);
void vsm_multi_get_motion(vsm_multi *m, int32_t seq, double *T16);   /* VisualOdometry::getMotion */
int vsm_multi_motion_valid(vsm_multi *m, int32_t seq);
/* bucketed = 0: Matcher::getMatches() as matchFeatures left it; 1: VisualOdometry::getMatches() (after bucketFeatures) */
int32_t vsm_multi_num_matches(vsm_multi *m, int32_t seq, int bucketed);
int32_t vsm_multi_get_matches(vsm_multi *m, int32_t seq, int bucketed, vsm_p_match *out, int32_t cap);
int32_t vsm_multi_num_inliers(vsm_multi *m, int32_t seq);            /* VisualOdometry::getInlierIndices */
int32_t vsm_multi_get_inliers(vsm_multi *m, int32_t seq, int32_t *out, int32_t cap);
/* wall clock of the last step, microseconds: features, first pass + its chain, second pass + final chain, bucketing + egomotion */
void vsm_multi_get_timings(vsm_multi *m, double *out4);

/* ---- monocular visual odometry ----
 * class VisualOdometryMono, viso/viso_mono.h:28-90: process() = pushBack + matchFeatures(0) +
 * bucketFeatures + getMatches + updateMotion (viso/viso_mono.cpp:33-39); estimateMotion
 * (viso/viso_mono.cpp:103-187) with the two inner loops the reference offloads to OpenCL
 * (viso/viso_mono_cl.cpp, viso/kernels/plane_and_inliers.cl) as HIP kernels.  Results equal the
 * reference's CPU class (double arithmetic) bit for bit. */
typedef struct {
  vsm_params match;              /* VisualOdometry::parameters::match */
  int32_t bucket_max_features;   /* VisualOdometry::bucketing, viso/viso.h:45-54 */
  double bucket_width, bucket_height;
  double f, cu, cv;              /* VisualOdometry::calibration, viso/viso.h:33-42 */
  double height, pitch;          /* VisualOdometryMono::parameters, viso/viso_mono.h:33-46 */
  int32_t ransac_iters;
  double inlier_threshold, motion_threshold;
} vsm_vo_mono_params;
typedef struct vsm_vo_mono vsm_vo_mono;

void vsm_vo_mono_default_params(vsm_vo_mono_params *p);
vsm_vo_mono *vsm_vo_mono_create(const vsm_vo_mono_params *p);      /* viso/viso_mono.cpp:27-28 */
void vsm_vo_mono_destroy(vsm_vo_mono *v);
/* VisualOdometryMono::process, viso/viso_mono.cpp:33-39; returns 1 (true) / 0 (false) */
int vsm_vo_mono_process(vsm_vo_mono *v, const uint8_t *I, int32_t width, int32_t height, int32_t bpl, int replace);
int vsm_vo_mono_process_device(vsm_vo_mono *v, const uint8_t *dI, int32_t width, int32_t height, int32_t bpl, int replace);
int vsm_vo_mono_process_matches(vsm_vo_mono *v, const vsm_p_match *m, int32_t n);   /* viso/viso.h:74-77 */
void vsm_vo_mono_get_motion(vsm_vo_mono *v, double *T16);
int vsm_vo_mono_motion_valid(vsm_vo_mono *v);
int32_t vsm_vo_mono_num_matches(vsm_vo_mono *v);
int32_t vsm_vo_mono_get_matches(vsm_vo_mono *v, vsm_p_match *out, int32_t cap);
int32_t vsm_vo_mono_num_inliers(vsm_vo_mono *v);
int32_t vsm_vo_mono_get_inliers(vsm_vo_mono *v, int32_t *out, int32_t cap);
float vsm_vo_mono_gain(vsm_vo_mono *v, const int32_t *inliers, int32_t n);
vsm_handle *vsm_vo_mono_matcher(vsm_vo_mono *v);
/* 1 if the hypothesis fits and triangulations run on the GPU (the device reproduced the host's SVD
 * bit for bit in the creation-time self-test), 0 if they run on the host pool */
int vsm_vo_mono_device_svd(vsm_vo_mono *v);
/* which stages of the last estimate (process / process_matches) took their result from the GPU: bit 0 the hypothesis
 * fits, bit 1 the inlier counts, bit 2 the triangulation, bit 3 the plane vote (at least 512 points in front of the
 * camera).  A stage the estimate never reached, or ran on the host, leaves its bit clear. */
int vsm_vo_mono_device_stages(vsm_vo_mono *v);
/* Test hooks of the egomotion's four kernels: each runs ONE kernel on the caller's inputs, through the launch code the
 * estimator uses, and returns everything the kernel wrote.  0 = ok, -1 = a bad argument (a null pointer, n < 1, K < 1,
 * a pick outside [0, n)), -2 = a HIP error.
 *   fit:         pts = n x {u1p, v1p, u1c, v1c} (normalised already), picks = K x 8 indices; F = K x 9.
 *   count:       counts[k] = matches whose Sampson distance to F[k] is below thr; slice > 0 caps the hypotheses per
 *                launch (0: the device's grid limit).
 *   triangulate: the four candidates R[c] (3x3) | t[c] (3) with K = {f, cu, cv}; X[c][row][match] (4 x 4 x n), chir[4].
 *   vote:        the plane vote of d[0 .. np) as the estimator runs it: sums[i] = the device's proposal for candidate i
 *                (the 16 slices added up; 0 for d[i] <= threshold), *best = the chosen index.  Returns 1 where the host
 *                ran the vote (np < 512): sums are then the exact sums. */
int32_t vsm_debug_mono_fit(const float *pts, int32_t n, const int32_t *picks, int32_t K, double *F);
int32_t vsm_debug_mono_count(const float *pts, int32_t n, const double *F, int32_t K, double thr, int32_t slice, int32_t *counts);
int32_t vsm_debug_mono_triangulate(const vsm_p_match *m, int32_t n, double f, double cu, double cv, const double *R, const double *t,
                                   double *X, int32_t *chir);
int32_t vsm_debug_mono_vote(const double *d, int32_t np, double threshold, double weight, double *sums, int32_t *best);
/* microseconds of the last process(): {matchFeatures, bucketing + copy, egomotion, total after the
 * push, then inside the egomotion: fundamental matrices, inlier counting, R|t + triangulation,
 * plane vote, 0, 0} */
void vsm_vo_mono_get_timings(vsm_vo_mono *v, double *out10);
/* host-only view of VisualOdometryMono::estimateMotion (no GPU: the two inner loops run on the host
 * threads).  1 = success, 0 = failure, -1 = failure before the RANSAC (inliers untouched). */
int32_t vsm_host_estimate_motion_mono(const vsm_vo_mono_params *p, const vsm_p_match *m, int32_t n, int32_t threads,
                                      double *tr6, double *T16, int32_t *inliers, int32_t *n_inliers);

/* host-only view of the egomotion solver (VisualOdometryStereo::estimateMotion,
 * viso/viso_stereo.cpp:42-146); needs no GPU.  Returns 1 = success (tr6 = rx,ry,rz,tx,ty,tz),
 * 0 = failure, -1 = fewer than 6 matches (inliers/n_inliers untouched, like the reference's early
 * return).  On success T16 (may be NULL) gets transformationVectorToMatrix(tr6), viso/viso.cpp:60-89.
 * inliers must hold n entries. */
int32_t vsm_host_estimate_motion_stereo(const vsm_vo_stereo_params *p, const vsm_p_match *m, int32_t n, int32_t threads,
                                        double *tr6, double *T16, int32_t *inliers, int32_t *n_inliers);

/* ---- the monocular motion of every pair of a pair set in one call (no counterpart in the reference,
 * which estimates frame by frame) ----
 * For pair k with list m_k of n_k flow matches the result - the return value rc (1, 0 or -1), tr6, T16 and the inlier
 * indices - is byte for byte that of vsm_vo_sampler_seed(71) followed by vsm_host_estimate_motion_mono(params, m_k, n_k):
 * VisualOdometryMono::estimateMotion with the sampler of a fresh process (viso/viso.cpp:93).  With bucket != 0 the list is
 * first bucketed as a fresh VisualOdometryMono buckets on its second process() (the parameters' bucket_* fields, a rand()
 * stream seeded 0 of the pair's own); the bucketed list is part of the result and the inlier indices refer to it.  Every
 * pair owns its sampler and its rand() stream: the process-wide sampler and libc's rand() are neither read nor advanced, and
 * the result does not depend on the pairs' order, the chunking or the number of threads.
 * A pair that fails does not fail the call; `stage` says where its estimate ended: 0 fewer than 10 matches (rc -1),
 * 1 normalisation degenerate (rc -1), 2 fewer than 10 inliers, 3 no R|t candidate with a point in front, 4 fewer than 10
 * points in front, 5 median above motion_threshold (rc 0), 6 success (rc 1).  Where rc is not 1, tr6 is zero and T16 the
 * identity.  On rc -1 the inlier list is empty (this API's choice: the reference leaves the list of the estimate before).
 *
 * vsm_motions_run: lists in host memory, on the handle's device and stream.  Of params only the egomotion, calibration and
 * bucketing fields are read.  VSM_EARG - nothing enqueued, the last result kept - for NULL params, n_pairs <= 0, a NULL list
 * with a positive count, a negative count, ransac_iters < 0, a flow coordinate (u1p, v1p, u1c, v1c) that is not finite and, with
 * bucket != 0, a negative u1c or v1c or a bucket size that is not positive (bucketFeatures would index outside its buckets).  VSM_EHIP after a HIP error (nothing further is launched; there
 * is then no result).  Option "motions_chunk": pairs per chunk, 0 = the memory rule of INTEGRATION.md.
 * vsm_pairs_motions: the same on the lists of the last vsm_pairs_run, which stay untouched; VSM_ENOTREADY without such a run,
 * VSM_EARG after one with method 1.
 * Nothing else of the handle changes: not the streaming ring, the pairs lists, the track or the point results. */
int vsm_motions_run(vsm_handle *h, const vsm_vo_mono_params *params, int32_t n_pairs, const vsm_p_match *const *lists, const int32_t *counts,
                    int32_t bucket);
int vsm_pairs_motions(vsm_handle *h, const vsm_vo_mono_params *params, int32_t bucket);
/* the last result: the number of pairs (0: none); per-pair arrays rc[P], stage[P], tr6[P][6], T16[P][16], n_inliers[P], any
 * of them NULL; a pair's inlier indices / the list its estimate saw (out = NULL: their number) */
int32_t vsm_motions_count(vsm_handle *h);
int32_t vsm_motions_get(vsm_handle *h, int32_t *rc, int32_t *stage, double *tr6, double *T16, int32_t *n_inliers);
int32_t vsm_motions_inliers(vsm_handle *h, int32_t pair, int32_t *out, int32_t cap);
int32_t vsm_motions_matches(vsm_handle *h, int32_t pair, vsm_p_match *out, int32_t cap);
/* out13: pairs per stage value 0 .. 6; pairs whose hypothesis fits, inlier counts (with the winner and its inlier list),
 * triangulation and plane vote came from the device (the vote runs on the device for every pair that reaches it, whatever
 * its number of points); chunks; stream waits */
void vsm_motions_get_stats(vsm_handle *h, int64_t *out13);
/* microseconds, summed over the chunks: sampling + packing + upload; fit + count + winner; host fits and E -> R|t;
 * triangulation; median + vote; total (a handle's first call also runs the SVD self-test, which shows in the total only) */
void vsm_motions_get_timings(vsm_handle *h, double *out6);
/* 1 if the handle's self-test (run by the first motions call) found the device's SVD bit-equal to the host's, so that the
 * calls run on the device; 0 before such a call, or where it did not: the calls then go through the host view */
int vsm_motions_device_svd(vsm_handle *h);
/* The same definition on `threads` host threads, no GPU and no handle: a loop of bucketing + the host estimator with
 * per-pair samplers (the CPU suite's subject and the device path's second opinion - not a fallback).  Per-pair arrays as
 * above, any of them NULL; pair k's inlier indices start at inliers[counts[0] + .. + counts[k - 1]], the list its estimate saw
 * at the same offset of matches (both hold the sum of all counts).  Returns n_pairs, or VSM_EARG with the outputs untouched. */
int32_t vsm_host_pairs_motions(const vsm_vo_mono_params *params, int32_t n_pairs, const vsm_p_match *const *lists, const int32_t *counts,
                               int32_t bucket, int32_t threads, int32_t *rc, int32_t *stage, double *tr6, double *T16, int32_t *n_inliers,
                               int32_t *inliers, int32_t *n_matches, vsm_p_match *matches);
/* Pair motions into the camera-to-world poses vsm_tracks_triangulate takes (host only).  pose[root] = identity; repeated
 * passes over the pairs in index order: a pair (a, b) with rc 1 whose a has a pose and whose b has none gives pose[b] =
 * pose[a] * inv(T) (Tr_total = Tr_total * inv(motion), viso/sfm.hh:57-58), one whose b has a pose and whose a has none gives
 * pose[a] = pose[b] * T; self pairs and pairs between two posed frames are skipped; it stops after a pass that sets nothing.
 * inv is the rigid inverse [R' | -R' t]; every product entry is a sum over k ascending from the k = 0 product.  poses12 =
 * n_frames x 12 (rows 0..2, zero where invalid), pose_valid = n_frames bytes.  Returns the number of frames with a pose, or
 * VSM_EARG for a root or a frame index outside [0, n_frames). */
int32_t vsm_chain_poses(int32_t n_frames, const int32_t *pairs, int32_t n_pairs, const double *T16, const int32_t *rc, int32_t root,
                        double *poses12, uint8_t *pose_valid);

const char *vsm_version(void);

#ifdef __cplusplus
}
#endif
#endif
