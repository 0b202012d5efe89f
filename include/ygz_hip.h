/*
 * ygz_hip.h -- C ABI of the MI355X (gfx950) implementation of ygz-slam's per-frame hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  The C++
 * class surfaces (include/ygz/...: ygz::Frame, FeatureDetector, Matcher, Tracker, ba::)
 * sit on top of it; INTEGRATION.md shows the bindings.  Every entry point cites the
 * reference interface it replaces (paths relative to the reference tree).
 *
 * Conventions
 *  - every function returns int: YGZ_OK (0) or a negative YGZ_E_* code; nothing throws or
 *    aborts (reference error conventions are bool/count returns);
 *  - a context owns all device memory (HBM) and one HIP stream; functions on the same
 *    context are not thread-safe, different contexts are independent (one per GPU/thread);
 *  - compute entry points are asynchronous on the context's stream and operate on data that
 *    is already resident in HBM; the ygz_hip_*_upload / *_download / get_* functions move
 *    host data and synchronise;
 *  - "slot" = index of a frame resident in HBM ([0, max_frames)); kernels are batched over
 *    contiguous slot ranges;
 *  - poses are 7 doubles (qx,qy,qz,qw,tx,ty,tz) = Sophus::SE3 (unit quaternion+translation);
 *    descriptors are 32 bytes per row (8 x u32), byte i bit j = BRIEF test 8i+j.
 */
#ifndef YGZ_HIP_H_
#define YGZ_HIP_H_
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define YGZ_OK              0
#define YGZ_E_INVALID      -1   /* bad argument */
#define YGZ_E_HIP          -2   /* a HIP runtime call failed (see ygz_hip_last_hip_error) */
#define YGZ_E_NO_DEVICE    -3   /* no usable gfx950 device */
#define YGZ_E_CAPACITY     -4   /* slot / keypoint / batch capacity exceeded */
#define YGZ_E_STATE        -5   /* call order violated (e.g. detect before pyramid) */

#define YGZ_MAX_LEVELS      8

/* Bumped whenever an exported function changes its argument list under the same name (C has no mangling: a caller built against an older
 * header would still link).  Bindings compare ygz_hip_abi_version() with the header they were written against at load time
 * (ygz_slam_amd/_lib.py, include/ygz/hip/Runtime.h).  5: ygz_hip_kf_row_bytes / ygz_hip_kf_store_create / ygz_hip_ba_build_windows
 * gained their trailing int (round 4); ygz_hip_get_stream / device_alloc / copy added (round 5).  6: ygz_ceres_options gained trust_region_strategy
 * (in the struct's tail padding: same size); ygz_hip_find_direct_projection_mp (+ _begin / _end), ygz_hip_sparse_align_residuals, ygz_hip_ba_light_barrier added (round 6).
 * Still 6: the monocular Initializer added (ygz_init_params, ygz_init_result, ygz_hip_default_init_params, ygz_hip_initialize,
 * ygz_hip_init_sample_sets, ygz_hip_init_hypotheses, ygz_hip_init_reconstruct) -- no existing argument list changed.
 * Still 6: the relocalisation's PnP RANSAC added (ygz_pnp_params, ygz_pnp_result, ygz_hip_default_pnp_params, ygz_hip_pnp_sample_sets,
 * ygz_hip_pnp_ransac, ygz_hip_pnp_hypotheses) -- no existing argument list changed.
 * Still 6: the loop detection's Sim3 RANSAC added (ygz_sim3_params, ygz_sim3_result, ygz_hip_default_sim3_params, ygz_hip_sim3_ransac,
 * ygz_hip_sim3_hypotheses) -- no existing argument list changed.
 * Still 6: the projection-guided descriptor search added (ygz_proj_problem, ygz_proj_params, ygz_hip_default_proj_params,
 * ygz_hip_search_by_projection, ygz_hip_projection_candidates) -- no existing argument list changed.
 * Still 6: the Sim3 pose-graph optimiser added (ygz_pgo_params, ygz_pgo_result, ygz_hip_default_pgo_params, ygz_hip_pose_graph_optimize,
 * ygz_hip_pgo_linearize) -- no existing argument list changed.
 * Still 6: the map upkeep of loop fusion added (ygz_hip_distinctive_descriptors, ygz_hip_covisibility) -- no existing argument list changed.
 * Still 6: the global bundle adjustment added (ygz_gba_params, ygz_gba_result, ygz_hip_default_gba_params, ygz_hip_global_ba,
 * ygz_hip_gba_linearize) -- no existing argument list changed.
 * Still 6: the stereo bundle adjustment added (ygz_sba_params, ygz_sba_result, ygz_hip_default_sba_params, ygz_hip_stereo_ba,
 * ygz_hip_sba_linearize) -- no existing argument list changed.
 * Still 6: the keyframe database added (ygz_kfdb, ygz_hip_kfdb_create, ygz_hip_kfdb_destroy, ygz_hip_kfdb_add, ygz_hip_kfdb_erase,
 * ygz_hip_kfdb_clear, ygz_hip_kfdb_info, ygz_hip_kfdb_query) -- no existing argument list changed.
 * Still 6: keyframe culling added (ygz_cull_params, ygz_hip_default_cull_params, ygz_hip_keyframe_redundancy, ygz_hip_cull_keyframes) -- no
 * existing argument list changed.
 * Still 6: lens undistortion added (ygz_undistort_params, ygz_hip_default_undistort_params, ygz_hip_set_undistortion, ygz_hip_undistort_map,
 * ygz_hip_build_pyramid_undistorted) -- no existing argument list changed.
 * Still 6: stereo input added (ygz_stereo_params, ygz_hip_default_stereo_params, ygz_hip_stereo_depths_slots, ygz_hip_stereo_match,
 * ygz_hip_stereo_candidates) -- no existing argument list changed.
 * Still 6: stereo pose optimisation added (ygz_pose_opt_params, ygz_hip_default_pose_opt_params, ygz_hip_optimize_pose_stereo) -- no existing
 * argument list changed.
 * Still 6: stereo rectification added (ygz_rectify_params, ygz_hip_stereo_rectify, ygz_hip_default_rectify_params, ygz_hip_set_rectification,
 * ygz_hip_rectify_map, ygz_hip_build_pyramid_rectified) -- no existing argument list changed.
 * Still 6: stereo map-point creation added (ygz_smap_params, ygz_smap_problem, ygz_hip_default_smap_params, ygz_hip_stereo_create_map_points,
 * ygz_hip_stereo_keyframe_points) -- no existing argument list changed.
 * Still 6: local-map fusion search added (ygz_lfuse_params, ygz_lfuse_points, ygz_lfuse_problem, ygz_hip_default_lfuse_params,
 * ygz_hip_local_fuse_search) -- no existing argument list changed.
 * Still 6: the stereo tracking search added (ygz_strack_params, ygz_strack_points, ygz_strack_problem, ygz_hip_default_strack_params,
 * ygz_hip_stereo_track_search) -- no existing argument list changed.
 * Still 6: stereo odometry on resident slots added (ygz_svo_params, ygz_hip_default_svo_params, ygz_hip_stereo_odometry_slots) -- no existing
 * argument list changed.
 * Still 6: stereo local-map tracking on resident slots added (ygz_slm_params, ygz_hip_default_slm_params, ygz_hip_stereo_local_map_slots) --
 * no existing argument list changed.
 * Still 6: stereo reference-keyframe tracking on resident slots added (ygz_srk_params, ygz_hip_default_srk_params,
 * ygz_hip_stereo_ref_keyframe_slots) -- no existing argument list changed.
 * Still 6: stereo relocalisation on resident slots added (ygz_srl_params, ygz_hip_default_srl_params, ygz_hip_stereo_relocalize_slots) -- no
 * existing argument list changed.
 * Still 6: local-map selection added (ygz_lms_params, ygz_hip_default_lms_params, ygz_hip_local_map_select) -- no existing argument list
 * changed.
 * Still 6: map-point attributes and local-map tracking on an indexed map added (ygz_hip_map_point_attributes,
 * ygz_hip_stereo_local_map_indexed) -- no existing argument list changed.
 * Still 6: the resident map added (ygz_hip_map, ygz_map_arrays, ygz_map_info, ygz_hip_map_create, _destroy, _info, _upload, _update,
 * _download, ygz_hip_stereo_local_map_resident) -- no existing argument list changed. */
#define YGZ_HIP_ABI_VERSION 6

typedef struct ygz_hip_ctx ygz_hip_ctx;

typedef struct {
    int   image_width, image_height;  /* level-0 size; config/default.yaml:15-16 (640x480) */
    int   pyramid_levels;             /* Basic/Frame.h:23 (3) */
    int   cell_size;                  /* feature.cell, default.yaml:50 (10) */
    int   fast_threshold;             /* feature.detection_threshold, default.yaml:51 (15) */
    int   nms_tie_suppress;           /* 0: drop a corner iff a neighbour is strictly greater */
    int   max_frames;                 /* frame slots resident in HBM */
    float fx, fy, cx, cy;             /* PinholeCamera float intrinsics, Basic/Camera.h:107 */
    int   debug_maps;                 /* !=0: keep per-pixel FAST score / NMS maps for parity tests */
} ygz_hip_params;

/* keypoints of one frame, structure-of-arrays (mirror of ygz::Feature, Basic/Feature.h:15-36) */
typedef struct {
    double  *px;       /* [n][2] level-0 pixel  (Feature::_pixel) */
    int32_t *level;    /* [n]                   (Feature::_level) */
    float   *score;    /* [n] Shi-Tomasi        (Feature::_score) */
    float   *angle;    /* [n] degrees           (Feature::_angle) */
    uint8_t *desc;     /* [n][32]               (Feature::_desc) */
} ygz_kpt_soa;

/* ---- context ---------------------------------------------------------------------------- */
void ygz_hip_default_params(ygz_hip_params *p);
/* stream: an existing hipStream_t to launch on (e.g. torch's current stream), or NULL to create one */
int  ygz_hip_create(ygz_hip_ctx **out, int device, const ygz_hip_params *prm, void *stream);
void ygz_hip_destroy(ygz_hip_ctx *ctx);
int  ygz_hip_synchronize(ygz_hip_ctx *ctx);
/* the context's stream waits for every stage pending on a side stream (what ygz_hip_synchronize does first), without blocking the host:
 * an event recorded on the stream afterwards marks the end of everything enqueued so far (bench.py's per-step timing) */
int  ygz_hip_join(ygz_hip_ctx *ctx);
/* enable != 0: the resident stages that do not depend on each other -- ygz_hip_track_sparse_align,
 * ygz_hip_ba_linearize_resident, ygz_hip_match_slots_again -- are launched on side HIP streams forked from the context's
 * stream, so they overlap with whatever is enqueued after them (KLT, direct projection); every entry point that reads or
 * overwrites their data, and ygz_hip_synchronize, joins them first.  Off by default. */
int  ygz_hip_set_overlap(ygz_hip_ctx *ctx, int enable);
/* Host work of the caller's own while a single-frame call waits for its kernel: fn(user) is called ONCE by the next ygz_hip_sparse_align (the longest wait
 * of a frame: one Gauss-Newton problem, ~0.3 ms) between its launch and its wait, then the hook is cleared.  fn must not call into this context.
 * fn == NULL clears.  (The class surface gathers the candidates of the frame's speculative FindDirectProjection launch there.) */
int  ygz_hip_set_wait_hook(ygz_hip_ctx *ctx, void (*fn)(void *), void *user);
const char *ygz_hip_error_string(int code);
int  ygz_hip_last_hip_error(const ygz_hip_ctx *ctx);
int  ygz_hip_max_keypoints(const ygz_hip_ctx *ctx);     /* = number of grid cells */
int  ygz_hip_abi_version(void);                         /* YGZ_HIP_ABI_VERSION of the library that is loaded */
/* plumbing for host code that drives several contexts and a collective library (ygz_slam_amd/host/ygz_offline.cpp; no reference
 * counterpart -- the reference is single-GPU): the context's hipStream_t as an opaque pointer (RCCL calls are enqueued on it), its device
 * ordinal / CU count, zero-filled device memory for exchange buffers, and a copy ordered on the stream (kind 0: host -> device, 1: device ->
 * host, 2: device -> device; wait == 0 needs page-locked host memory) */
int  ygz_hip_get_stream(ygz_hip_ctx *ctx, void **stream);
int  ygz_hip_get_device(const ygz_hip_ctx *ctx, int *device, int *compute_units);
int  ygz_hip_make_current(ygz_hip_ctx *ctx);            /* hipSetDevice(the context's device) for the calling thread, left that way */
int  ygz_hip_device_alloc(ygz_hip_ctx *ctx, void **out, size_t bytes);
int  ygz_hip_device_free(ygz_hip_ctx *ctx, void *p);
int  ygz_hip_copy(ygz_hip_ctx *ctx, void *dst, const void *src, size_t bytes, int kind, int wait);
/* HIP-event timing on the context's stream (bench.py roofline leg) */
int  ygz_hip_timer_begin(ygz_hip_ctx *ctx);
int  ygz_hip_timer_end(ygz_hip_ctx *ctx, float *elapsed_ms);   /* synchronises */
/* HIP events around EVERY launch of one named kernel (e.g. "k_klt") until probe_end: total time and launch count */
int  ygz_hip_probe_begin(ygz_hip_ctx *ctx, const char *kernel_name, int max_launches);
int  ygz_hip_probe_end(ygz_hip_ctx *ctx, double *total_ms, int *launches);   /* synchronises */

/* ---- A1: frame store + pyramid -- replaces Frame::InitFrame / CreateImagePyramid
 *      (src/Basic/Frame.cpp:22-40: cv::cvtColor BGR2GRAY + cv::pyrDown per level) -------------- */
int  ygz_hip_upload_bgr(ygz_hip_ctx *ctx, int slot, const uint8_t *bgr, int stride_bytes);
int  ygz_hip_upload_gray(ygz_hip_ctx *ctx, int slot, const uint8_t *gray, int stride_bytes);
/* builds levels 1..pyramid_levels-1 (and level 0 from BGR when from_bgr!=0) for n slots */
int  ygz_hip_build_pyramid(ygz_hip_ctx *ctx, int slot_begin, int n_slots, int from_bgr);
int  ygz_hip_download_level(ygz_hip_ctx *ctx, int slot, int level, uint8_t *dst /* w_l*h_l */);
/* the tracker's working image of a level: the level inside a 24-pixel BORDER_REFLECT_101 frame (what cv::buildOpticalFlowPyramid makes with
 * copyMakeBorder), as the pyramid kernels wrote it once the tracker's buffers exist (first ygz_hip_track_klt / ygz_hip_klt_track).
 * dst [h + 48][w + 48]; YGZ_E_STATE when the slot has no current framed copy of the level.  (Test / debugging aid.) */
int  ygz_hip_download_framed_level(ygz_hip_ctx *ctx, int slot, int level, uint8_t *dst);
int  ygz_hip_level_size(const ygz_hip_ctx *ctx, int level, int *w, int *h);

/* ---- A0: lens undistortion in front of the pyramid -- the reference reads camera.k1, k2, p1, p2 (Basic/Camera.h) and never uses them; every
 * kernel behind level 0 assumes an ideal pinhole picture.  The model is OpenCV's: initUndistortRectifyMap with R = I, then remap with
 * INTER_LINEAR in its 5-bit fixed point and a constant border.  For output pixel (u, v) of the context's camera (its float intrinsics as
 * doubles, _d below), in FP64 without contraction:
 *   x = (u - cx_d) / fx_d, y = (v - cy_d) / fy_d; x2 = x x, y2 = y y, r2 = x2 + y2, xy2 = 2 (x y); kr = 1 + ((k3 r2 + k2) r2 + k1) r2;
 *   xd = (x kr + p1 xy2) + p2 (r2 + 2 x2); yd = (y kr + p1 (r2 + 2 y2)) + p2 xy2; mx = fx xd + cx, my = fy yd + cy.
 * Outside -- !(mx > -2 && mx < w + 1 && my > -2 && my < h + 1), NaN included -- the pixel is border_value and both map entries INT32_MIN.
 * Otherwise qx = (int32) rint(32 mx) (half to even), sx = qx >> 5, ax = qx & 31, the same for y, the four taps (sy, sx) .. (sy + 1, sx + 1)
 * with border_value outside the picture, and out = ((32-ax)(32-ay) t00 + ax (32-ay) t01 + (32-ax) ay t10 + ax ay t11 + 512) >> 10.  A BGR
 * picture is converted per tap with the gray formula of ygz_hip_build_pyramid.  The map and the image are bit-identical to tests/undist_ref.c
 * (DESIGN.md section 18); parity with OpenCV itself is unpinned. */
typedef struct {
    double k1, k2, p1, p2, k3;          /* Brown-Conrady coefficients of the camera that took the picture */
    double fx, fy, cx, cy;              /* its intrinsics (the output camera is the context's ygz_hip_params) */
    int    border_value;                /* gray value of what the picture does not cover, in [0, 255] */
} ygz_undistort_params;
/* zero coefficients, the context's intrinsics, border 0.  YGZ_E_INVALID for a null argument */
int  ygz_hip_default_undistort_params(const ygz_hip_ctx *ctx, ygz_undistort_params *p);
/* builds the map of the context's size (one launch, synchronous); p == NULL drops it.  YGZ_E_INVALID for a field that is not finite, fx or
 * fy <= 0, border_value outside [0, 255]; last, for a null context */
int  ygz_hip_set_undistortion(ygz_hip_ctx *ctx, const ygz_undistort_params *p);
/* the map, qx and qy [h][w] (test aid; synchronises).  YGZ_E_STATE without a map */
int  ygz_hip_undistort_map(ygz_hip_ctx *ctx, int32_t *qx, int32_t *qy);
/* ygz_hip_build_pyramid with level 0 = the undistorted gray of the uploaded picture (from_bgr: of the BGR upload, else of the gray upload, which
 * is first copied aside on the same stream).  One call: the remap, the pyramid and the tracker's framed copies follow one another on one
 * stream, also beside a trailing LK launch.  YGZ_E_STATE without a map.  ygz_hip_build_pyramid itself never undistorts. */
int  ygz_hip_build_pyramid_undistorted(ygz_hip_ctx *ctx, int slot_begin, int n_slots, int from_bgr);

/* ---- A0b: stereo rectification in front of the pyramid -- the raw pictures of a two-camera rig resampled so that both are seen by the
 * context's ideal camera and epipolar lines are image rows, which is what ygz_hip_stereo_depths_slots, ygz_hip_optimize_pose_stereo and
 * ygz_hip_stereo_ba assume.  The model is OpenCV's: stereoRectify (Bouguet's method) for the two rotations, initUndistortRectifyMap with
 * R = R1 or R2 for the map of each camera, remap as above.  The map of camera k differs from the lens-only one in its first step: with
 * (x0, y0) = ((u - cx_d) / fx_d, (v - cy_d) / fy_d) and r = R row-major,  X = (r0 x0 + r3 y0) + r6,  Y = (r1 x0 + r4 y0) + r7,
 * W = (r2 x0 + r5 y0) + r8  (that is R^T (x0, y0, 1)),  x = X / W,  y = Y / W;  !(W > 0) is outside.  The rotations, the maps and the images
 * are bit-identical to tests/rect_ref.c.  The output camera is the context's, so bf = fx * baseline. */
#define YGZ_RECT_CAMERAS 2
typedef struct {
    ygz_undistort_params lens;          /* the camera that took the picture */
    double R[9];                        /* row-major: R1 (camera 0) or R2 (camera 1) of ygz_hip_stereo_rectify */
} ygz_rectify_params;                   /* 152 bytes */
/* the rotations of a rig with X_right = R X_left + T (row-major): R1, R2 turn the left and the right camera's rays into the common rectified
 * frame, in which the right camera sits `baseline` to the right of the left one.  Host code: no device, no context.  YGZ_E_INVALID for a
 * null argument, a value that is not finite, T = 0, an R that is no rotation (max |R R^T - I| > 1e-6 or det <= 0), cameras 120 degrees or
 * more apart, and a second camera that is not to the right of the first (after the half rotation: t[0] >= 0 or |t[0]| < max(|t[1]|, |t[2]|)) */
int  ygz_hip_stereo_rectify(const double R[9], const double T[3], double R1[9], double R2[9], double *baseline);
/* the default lens (ygz_hip_default_undistort_params) and R = I.  YGZ_E_INVALID for a null argument */
int  ygz_hip_default_rectify_params(const ygz_hip_ctx *ctx, ygz_rectify_params *p);
/* builds the map of rig camera `camera` (0 or 1) and the table of its tiles' source boxes (two launches, synchronous); p == NULL drops them.
 * Independent of ygz_hip_set_undistortion.  YGZ_E_INVALID for a camera outside [0, YGZ_RECT_CAMERAS), the lens rules of
 * ygz_hip_set_undistortion, an R that is not finite or no rotation (as above); last, for a null context */
int  ygz_hip_set_rectification(ygz_hip_ctx *ctx, int camera, const ygz_rectify_params *p);
/* the map of a camera, qx and qy [h][w] (test aid; synchronises).  YGZ_E_STATE without a map */
int  ygz_hip_rectify_map(ygz_hip_ctx *ctx, int camera, int32_t *qx, int32_t *qy);
/* ygz_hip_build_pyramid with level 0 of slot slot_begin + i = its upload through the map of camera camera_of_slot[i] (0 or 1), all slots of
 * both cameras in one launch; otherwise as ygz_hip_build_pyramid_undistorted.  YGZ_E_INVALID for a null table or an entry outside
 * [0, YGZ_RECT_CAMERAS); YGZ_E_STATE when a named camera has no map */
int  ygz_hip_build_pyramid_rectified(ygz_hip_ctx *ctx, int slot_begin, int n_slots, int from_bgr, const uint8_t *camera_of_slot);

/* ---- A2-A7: extractor -- replaces FeatureDetector::Detect
 *      (src/Algorithm/FeatureDetector.cpp:345-444: fast_corner_detect_10 + fast_corner_score_10
 *      + fast_nonmax_3x3 per level, per-cell best Shi-Tomasi, IC_Angle, ComputeOrbDescriptor) ---- */
/* occupied: host [n_slots][cells] bytes (SetExistingFeatures, :446-464) or NULL.  Results stay
 * in HBM (keypoint SoA per slot, cell-index order == the order Detect pushes to _features). */
int  ygz_hip_detect(ygz_hip_ctx *ctx, int slot_begin, int n_slots, const uint8_t *occupied);
int  ygz_hip_keypoint_count(ygz_hip_ctx *ctx, int slot, int *n);
int  ygz_hip_get_keypoints(ygz_hip_ctx *ctx, int slot, ygz_kpt_soa *out, int capacity, int *n);
/* FeatureDetector::ComputeAngleAndDescriptor(Frame*) (:580-588): replaces the keypoint list of
 * `slot` by the given pixels/levels and (re)computes angle + descriptor for them */
int  ygz_hip_describe(ygz_hip_ctx *ctx, int slot, const double *px /*[n][2]*/, const int32_t *level, int n);
/* FeatureDetector::ComputeDescriptor(Feature*) (:591-594): descriptor only, with the given angles (degrees) */
int  ygz_hip_describe_given_angle(ygz_hip_ctx *ctx, int slot, const double *px, const int32_t *level, const float *angle, int n);
/* parity/debug (needs debug_maps): per-pixel maps of one level after ygz_hip_detect:
 * score[y*w+x] = 0 (no FAST-10 corner at the threshold) or fast_corner_score_10 + 1;
 * nms[y*w+x]   = 1 iff the corner survives fast_nonmax_3x3 */
int  ygz_hip_get_fast_maps(ygz_hip_ctx *ctx, int slot, int level, uint8_t *score, uint8_t *nms);

/* ---- M1-M3: 256-bit Hamming matcher -- replaces Matcher::DescriptorDistance
 *      (src/Algorithm/Matcher.cpp:30-43) and cv::BFMatcher(NORM_HAMMING, crossCheck).match()
 *      (test/test_orb_match.cpp:86-93) -------------------------------------------------------- */
/* descriptor sets of slots (query_slot[i], train_slot[i]), i < n_pairs, as left by detect/describe.
 * cross_check: 0 plain nearest neighbour, 1 OpenCV cross-check, 2 strict mutual NN.
 * Results per pair stay in HBM; fetch with ygz_hip_get_matches. */
int  ygz_hip_match_slots(ygz_hip_ctx *ctx, const int32_t *query_slot, const int32_t *train_slot,
                         int n_pairs, int cross_check);
/* re-run the matcher on the pair table uploaded by the last ygz_hip_match_slots (no host copies) */
int  ygz_hip_match_slots_again(ygz_hip_ctx *ctx, int cross_check);
int  ygz_hip_get_matches(ygz_hip_ctx *ctx, int pair, int32_t *train_idx /*[nq]*/, int32_t *dist /*[nq]*/,
                         int capacity, int *nq);
/* stand-alone form on host descriptor arrays (uploads, matches, downloads).  dist2 (second-best
 * distance, Matcher::SearchByBoW :242-246 ratio test) may be NULL and needs cross_check==0.
 * nq, nt <= grid cells x max_frames (the result rows of all pairs of the context), YGZ_E_CAPACITY beyond. */
int  ygz_hip_hamming_match(ygz_hip_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt,
                           int cross_check, int32_t *train_idx, int32_t *dist, int32_t *dist2);

/* ---- M3: the "good match" filter of test/test_orb_match.cpp:97-104 on the matcher's output: min_dis = the smallest distance
 *      among the matches, clamped to [min_floor, min_ceil] (20, 50); a match is good iff distance < factor * min_dis (3).
 *      Resident form: every pair of the current pair table in one launch, flags stay in HBM (ygz_hip_get_good_matches). */
int  ygz_hip_match_postfilter(ygz_hip_ctx *ctx, double min_floor, double min_ceil, double factor);
int  ygz_hip_get_good_matches(ygz_hip_ctx *ctx, int pair, uint8_t *good /*[nq]*/, int capacity, int *nq, int *n_good, double *min_dis);
/* the same on host arrays as ygz_hip_hamming_match returned them (train_idx < 0: no match).  nq == 0 (the reference dereferences
 * end() there) is defined as "nothing kept". */
/* M1-M3 over many host descriptor sets in one call (the matching a keyframe window needs: one set against several others):
 * desc[s] = count[s] rows of 32 bytes; pair p matches query set pair_q[p] against train set pair_t[p] with BFMatcher semantics
 * (test/test_orb_match.cpp:86-93) and, when any of good / n_good / min_dis is given, applies the good-match rule of :95-104.
 * train_idx / dist / good: [n_pairs][ygz_hip_max_keypoints()] rows (entries past count[pair_q[p]] are not written). */
int  ygz_hip_match_sets(ygz_hip_ctx *ctx, int n_sets, const uint8_t *const *desc, const int32_t *count, int n_pairs,
                        const int32_t *pair_q, const int32_t *pair_t, int cross_check, int32_t *train_idx, int32_t *dist,
                        uint8_t *good, int32_t *n_good, double *min_dis, double min_floor, double min_ceil, double factor);
int  ygz_hip_match_postfilter_host(ygz_hip_ctx *ctx, const int32_t *train_idx, const int32_t *dist, int nq, double min_floor,
                                   double min_ceil, double factor, uint8_t *good, int *n_good, double *min_dis);
/* ---- M6: Matcher::CheckFrameDescriptors (src/Algorithm/Matcher.cpp:45-84): Hamming distance of n given (index1, index2) feature
 *      pairs of two frames, best_dist = min clamped to [init_low, init_high] (Matcher.h:27-28), keep[i] = dist[i] < ratio * best_dist
 *      (initMatchRatio 3.0).  Slot form: resident descriptors of the two slots; pair form: host descriptors [n][32] row by row.
 *      n == 0 (UB in the reference) returns n_good = 0. */
int  ygz_hip_check_frame_descriptors(ygz_hip_ctx *ctx, int slot1, int slot2, const int32_t *idx1, const int32_t *idx2, int n,
                                     int init_low, int init_high, float ratio, int32_t *dist, uint8_t *keep, int *n_good, int *best_dist);
int  ygz_hip_check_descriptor_pairs(ygz_hip_ctx *ctx, const uint8_t *desc1, const uint8_t *desc2, int n, int init_low, int init_high,
                                    float ratio, int32_t *dist, uint8_t *keep, int *n_good, int *best_dist);

/* ---- L1-L2: patch alignment -- replaces Matcher::FindDirectProjection (Matcher.cpp:356-417:
 *      GetWarpAffineMatrix, GetBestSearchLevel, WarpAffine, cvutils::Align2D CVUtils.cpp:186-318) -- */
typedef struct {
    int    ref_slot, cur_slot;
    double T_ref[7], T_cur[7];      /* Frame::_TCW of the two frames */
} ygz_align_pair;
/* n candidates: px_ref [n][2], depth_ref [n] (>=0; Feature::_depth or z of World2Camera),
 * level_ref [n], px_cur [n][2] in (prediction) / out (refined), search_level [n] out,
 * ok [n] out (the bool FindDirectProjection returns).  Host arrays; synchronises. */
int  ygz_hip_find_direct_projection(ygz_hip_ctx *ctx, const ygz_align_pair *pair,
                                    const double *px_ref, const double *depth_ref, const int32_t *level_ref,
                                    double *px_cur, int32_t *search_level, uint8_t *ok, int n);
/* ---- LocalMapping::FindCandidates + ProjectMapPoints (src/Module/LocalMapping.cpp:47-120) in one call.
 * FindCandidates: each non-bad local map point is projected into the current frame (World2Camera, Camera2Pixel); behind the
 * camera or outside InFrame(px,20) -> in_view = 0.  ProjectMapPoints: every candidate (an observation of a point in one of
 * the K resident local keyframes: pixel and pyramid level of that observation) is refined by the MapPoint overload of
 * Matcher::FindDirectProjection (Matcher.cpp:356-383, depth = z of the point in that keyframe); per point the FIRST success
 * in candidate order is kept (the reference iterates a std::map<Feature*,...>, i.e. heap-address order; the order here is
 * the caller's).  Outputs per point: in_view, px_proj [P][2], match_cand (candidate index or -1), px_match [P][2]
 * (Feature::_pixel of the new feature), match_level (its _level).  Host arrays; synchronises. */
typedef struct {
    int n_points;      const double *pos_world /*[P][3]*/; const uint8_t *point_bad /*[P] or NULL*/;
    int n_keyframes;   const int32_t *kf_slot /*[K]*/;     const double *kf_T /*[K][7] Frame::_TCW*/;
    int n_candidates;  const int32_t *cand_point, *cand_kf, *cand_level /*[C]*/; const double *cand_px_ref /*[C][2]*/;
} ygz_local_map;
int  ygz_hip_track_local_map(ygz_hip_ctx *ctx, int cur_slot, const double T_cur[7], const ygz_local_map *m,
                             uint8_t *in_view, double *px_proj, int32_t *match_cand, double *px_match, int32_t *match_level,
                             int32_t *n_matched);
/* ---- the call the reference's UNCHANGED caller makes: bool Matcher::FindDirectProjection(Frame *ref, Frame *curr, MapPoint *mp, Vector2d &px_curr,
 * int &search_level) (src/Algorithm/Matcher.cpp:356-383), once per candidate from LocalMapping::ProjectMapPoints (src/Module/LocalMapping.cpp:88-118).
 * n independent candidates over K resident reference keyframes in ONE launch, every candidate evaluated (no first-success rule): candidate i =
 * map point pos_world[i] seen in keyframe cand_kf[i] at px_ref[i] / level_ref[i] (the Feature mp->_obs[ref->_keyframe_id]); depth =
 * World2Camera(pos_world, ref->_TCW)[2], sign not tested (as the reference).  px_in [n][2]: the caller's predictions; NULL: the prediction is
 * LocalMapping::FindCandidates' projection Camera2Pixel(World2Camera(pos_world, T_cur)) (LocalMapping.cpp:58-59), written to px_proj [n][2] with
 * in_view [n] = !(z < 0) && InFrame(px, 20); candidates out of view are not evaluated (ok = 0, px_cur undefined).  ok [n] = the bool returned,
 * px_cur [n][2] = refined pixel (level 0), search_level [n].  Host arrays; synchronises.  The class surface memoises one such launch per
 * current frame behind the per-candidate method (ygz_host.cpp: FdpMemo), bit-identical to n = 1 calls. */
int  ygz_hip_find_direct_projection_mp(ygz_hip_ctx *ctx, int cur_slot, const double T_cur[7], int n_keyframes, const int32_t *kf_slot,
                                       const double *kf_T /*[K][7]*/, int n, const int32_t *cand_kf, const double *pos_world /*[n][3]*/,
                                       const double *px_ref, const int32_t *level_ref, const double *px_in /*or NULL*/,
                                       uint8_t *in_view /*may be NULL with px_in*/, double *px_proj /*may be NULL with px_in*/,
                                       uint8_t *ok, double *px_cur, int32_t *search_level);
/* The same launch in two halves: _begin (the px_in = NULL form) queues uploads, kernels and the copy back and does not wait; _end (same n) waits and
 * hands out what ygz_hip_find_direct_projection_mp would have returned.  One run pending per context (a second _begin replaces it); YGZ_E_STATE from
 * _end when none is (or n differs); other calls on the context in between queue behind it.  The class surface queues its speculative launch at the
 * end of Matcher::SparseImageAlignment (src/Algorithm/Matcher.cpp:16-31) and collects at the first per-candidate call of the frame. */
int  ygz_hip_find_direct_projection_mp_begin(ygz_hip_ctx *ctx, int cur_slot, const double T_cur[7], int n_keyframes, const int32_t *kf_slot,
                                             const double *kf_T, int n, const int32_t *cand_kf, const double *pos_world, const double *px_ref,
                                             const int32_t *level_ref);
int  ygz_hip_find_direct_projection_mp_end(ygz_hip_ctx *ctx, int n, uint8_t *in_view, double *px_proj, uint8_t *ok, double *px_cur,
                                           int32_t *search_level);
/* bare cvutils::Align2D on host-provided patches against level `level` of `cur_slot`:
 * pwb [n][100], patch [n][64], uv [n][2] in/out (level pixels), ok [n], chi2 [n] (may be NULL) */
int  ygz_hip_align2d(ygz_hip_ctx *ctx, int cur_slot, int level, const uint8_t *pwb, const uint8_t *patch,
                     double *uv, uint8_t *ok, float *chi2, int n, int n_iter);

/* ---- L3: sparse image alignment -- replaces SparseImgAlign::run
 *      (src/Algorithm/SparseImageAlign.cpp:21-50 + NLLSSolver::optimizeGaussNewton,
 *      include/ygz/Algorithm/NLSSolver_impl.hpp:15-89; what Matcher::SparseImageAlignment calls) --- */
/* features of the reference frame: px [n][2], depth [n], has_mappoint [n].  T_cur in/out.
 * max_level/min_level/n_iter as SparseImgAlign ctor (Matcher.cpp:18: 2,0,30).  n_meas_out =
 * the size_t run() returns.  The whole Gauss-Newton loop runs on the GPU. */
int  ygz_hip_sparse_align(ygz_hip_ctx *ctx, int ref_slot, const double T_ref[7], int cur_slot, double T_cur[7],
                          const double *px, const double *depth, const uint8_t *has_mappoint, int n,
                          int max_level, int min_level, int n_iter, int *n_meas_out, int *iters_out /*[levels] or NULL*/);

/* One NLLSSolver::computeResiduals(model, linearize_system = true) of SparseImgAlign (src/Algorithm/SparseImageAlign.cpp:124-223, with
 * precomputeReferencePatches :59-122 for `level`) at a model the caller holds -- the step a solver other than the resident Gauss-Newton loop is
 * built from; SparseImgAlign(..., LevenbergMarquardt, ...) of the class surface (include/ygz/Algorithm/NLSSolver_impl.hpp:91-212) drives its
 * trials with it.  T_cur_from_ref = the solver's model (SparseImageAlign.cpp:37).  chi2_sum: the reference's float running sum of res^2 over the
 * features / pixels in order (exact); n_meas: measurements (16 per feature used); H [36] row-major symmetric and Jres [6] (either may be NULL):
 * H_ / Jres_ after the call.  Features as ygz_hip_sparse_align.  Host arrays; synchronises. */
int  ygz_hip_sparse_align_residuals(ygz_hip_ctx *ctx, int ref_slot, int cur_slot, const double T_cur_from_ref[7],
                                    const double *px, const double *depth, const uint8_t *has_mappoint, int n, int level,
                                    double *chi2_sum, int *n_meas, double *H, double *Jres);

/* ---- L4: pyramidal LK -- replaces cv::calcOpticalFlowPyrLK as called by Tracker::TrackKLT
 *      (src/Algorithm/Tracker.cpp:92-98) ------------------------------------------------------- */
typedef struct {
    int win, max_level, max_iter;     /* Tracker.h:25-27, Tracker.cpp:97 (21, 4, 30) */
    double eps, min_eig_threshold;    /* 0.001, 1e-4 */
    int use_initial_flow;             /* OPTFLOW_USE_INITIAL_FLOW */
} ygz_klt_params;
void ygz_hip_default_klt_params(ygz_klt_params *p);
/* level-0 images of prev_slot/cur_slot; prev_pts [n][2], next_pts [n][2] in/out, status [n], err [n]; any n (served in pieces of grid-cell size) */
int  ygz_hip_klt_track(ygz_hip_ctx *ctx, int prev_slot, int cur_slot, const float *prev_pts, float *next_pts,
                       int n, const ygz_klt_params *prm, uint8_t *status, float *err);

/* the same plus Tracker::TrackKLT's survivor rule (Tracker.cpp:100-112) evaluated on the device: keep[i] = status[i] != 0 and
 * InFrame(next_pts[i], border) (20 in the reference); n_keep = number of survivors */
int  ygz_hip_klt_track_filtered(ygz_hip_ctx *ctx, int prev_slot, int cur_slot, const float *prev_pts, float *next_pts, int n,
                                const ygz_klt_params *prm, int border, uint8_t *status, float *err, uint8_t *keep, int *n_keep);

/* ---- resident batched tracking: the same L1-L4 kernels over MANY frame pairs per launch, inputs taken from
 *      the keypoints the extractor left in HBM, no host round trip between stages.  This is the per-frame path
 *      of VisualOdometry::AddFrame (src/Module/VisualOdometry.cpp:38-107: Tracker::Track -> TrackRefFrame ->
 *      TrackLocalMap) restructured for throughput; pair i = (cur_slot[i], ref_slot[i]). ------------------------ */
/* Feature::_depth / Feature::_mappoint of the keypoints of `slot` (keypoint order of ygz_hip_get_keypoints) */
int  ygz_hip_set_keypoint_depths(ygz_hip_ctx *ctx, int slot, const double *depth, const uint8_t *has_mappoint, int n);
/* uploads the pair table + poses (T_* [n_pairs][7]) and loads the reference keypoints of every pair into its
 * track set on the device.  predict != 0: the direct-projection start pixel is the projection of the feature with
 * (T_cur, T_ref) (LocalMapping::FindCandidates, LocalMapping.cpp:47-80), else the reference pixel itself.
 * KLT starts from the reference pixels (Tracker::SetReference); sparse alignment starts from T_ref (Matcher.cpp:471). */
int  ygz_hip_track_begin(ygz_hip_ctx *ctx, const int32_t *cur_slot, const int32_t *ref_slot, const double *T_cur,
                         const double *T_ref, int n_pairs, int predict);
int  ygz_hip_track_reload(ygz_hip_ctx *ctx, int predict);       /* device-side reload only (next step, same pairs) */
int  ygz_hip_track_klt(ygz_hip_ctx *ctx, const ygz_klt_params *prm);
/* optional: the working images of calcOpticalFlowPyrLK (buildOpticalFlowPyramid's framed levels + Scharr derivatives, OpenCV
   lkpyramid.cpp; called from src/Algorithm/Tracker.cpp:97) for the current pair table, built ahead on a side stream -- call after
   ygz_hip_build_pyramid; ygz_hip_track_klt (default parameters) then skips them.  Same results with or without. */
int  ygz_hip_track_klt_prepare(ygz_hip_ctx *ctx);
int  ygz_hip_track_direct(ygz_hip_ctx *ctx);
int  ygz_hip_track_sparse_align(ygz_hip_ctx *ctx, int max_level, int min_level, int n_iter);
/* VisualOdometry::TrackRefFrame -> TrackLocalMap hand-over (src/Module/VisualOdometry.cpp:281-302, src/Module/LocalMapping.cpp:47-80)
 * on the device for every pair: the pose the sparse alignment left becomes the pair's current pose and every reference feature's
 * map point (Pixel2Camera(px, depth) taken to the world with T_ref) is re-projected with it -- the start pixel of the direct
 * projection; features without depth, behind the camera or outside InFrame(px, 20) stop being candidates (ok = 0 afterwards). */
int  ygz_hip_track_adopt_pose(ygz_hip_ctx *ctx);
/* LocalMapping::OptimizeCurrent -> ba::OptimizeCurrentPoseOnly (src/Module/LocalMapping.cpp:122-127, src/Algorithm/BA.cpp:188-264) for
 * every pair, on the features ProjectMapPoints created (the direct-projection successes: pixel = refined pixel, map point = the
 * reference feature's), starting from the pair's current pose.  Results stay in HBM. */
int  ygz_hip_track_pose_only(ygz_hip_ctx *ctx);
/* pose [6] = [t; log(so3)], T [7] = SE3(SO3::exp(.), t) (BA.cpp:254); bad/depth [n] per reference feature (bad = 1 also for
 * features that were not projected); any output may be NULL */
int  ygz_hip_track_get_pose_only(ygz_hip_ctx *ctx, int pair, double pose[6], double T[7], int *inliers, int *rounds, uint8_t *bad,
                                 double *depth, int capacity, int *n);
int  ygz_hip_track_get_klt(ygz_hip_ctx *ctx, int pair, float *pts, uint8_t *status, float *err, int capacity, int *n);
int  ygz_hip_track_get_direct(ygz_hip_ctx *ctx, int pair, double *px, int32_t *level, uint8_t *ok, int capacity, int *n);
int  ygz_hip_track_get_pose(ygz_hip_ctx *ctx, int pair, double T[7], int *n_meas, int *iters /*[levels] or NULL*/);

/* ---- bulk traffic for pipelines that stream frames through the context (offline run, bench.py --stream).  wait == 0: the
 *      copy is only enqueued on the context's stream -- host buffers must then be page-locked (ygz_hip_pinned_alloc) and stay
 *      valid until the next synchronising call; wait != 0: synchronises.  Layouts are the resident ones: [n_slots][cells][...]. */
int  ygz_hip_pinned_alloc(void **out, size_t bytes);
int  ygz_hip_pinned_free(void *p);
/* Frame::_color of n consecutive slots in one copy: bgr [n_slots][h][w][3], contiguous (src/Basic/Frame.cpp:22-30 input) */
int  ygz_hip_upload_bgr_batch(ygz_hip_ctx *ctx, int slot_begin, int n_slots, const uint8_t *bgr, int wait);
/* the same for frames that are already gray (level 0 of the pyramid): gray [n_slots][h][w] */
int  ygz_hip_upload_gray_batch(ygz_hip_ctx *ctx, int slot_begin, int n_slots, const uint8_t *gray, int wait);
/* Feature::_pixel of every keypoint of n slots: px [n_slots][cells][2], count [n_slots] */
int  ygz_hip_get_keypoint_pixels_batch(ygz_hip_ctx *ctx, int slot_begin, int n_slots, double *px, int32_t *count, int wait);
/* all keypoint fields of n slots (members of *out may be NULL): arrays [n_slots][cells][...] */
int  ygz_hip_get_keypoints_batch(ygz_hip_ctx *ctx, int slot_begin, int n_slots, ygz_kpt_soa *out, int32_t *count, int wait);
/* Feature::_depth / _mappoint != nullptr of n slots: depth [n_slots][cells], has_mappoint [n_slots][cells] */
int  ygz_hip_set_keypoint_depths_batch(ygz_hip_ctx *ctx, int slot_begin, int n_slots, const double *depth, const uint8_t *has_mappoint,
                                       int wait);
/* n_kp of n consecutive slots (what Frame::_features.size() would be), e.g. beside ygz_hip_track_get_summary */
int  ygz_hip_get_keypoint_counts(ygz_hip_ctx *ctx, int slot_begin, int n_slots, int32_t *count, int wait);
/* RGB-D style input: a depth image per slot, dw x dh samples covering the level-0 frame (dw <= width, dh <= height; kind 0: float32
 * metres, kind 1: uint16 with depth = value * scale, TUM RGB-D: 1 / 5000, kind 2: float64 metres); depth [n_slots][dh][dw].  ygz_hip_keypoint_depths_from_image
 * then sets Feature::_depth of every keypoint of the slots to the sample at ((int)x * dw / width, (int)y * dh / height) and
 * _mappoint != nullptr to depth > 0, on the device -- what ygz_hip_set_keypoint_depths[_batch] do from host arrays.  (In the reference
 * a feature's depth is the z of its map point, src/Module/LocalMapping.cpp:100-111; the offline run's depth image stands in for the map.) */
int  ygz_hip_upload_depth_batch(ygz_hip_ctx *ctx, int slot_begin, int n_slots, const void *depth, int dw, int dh, int kind, double scale,
                                int wait);
int  ygz_hip_keypoint_depths_from_image(ygz_hip_ctx *ctx, int slot_begin, int n_slots);
/* ---- S0: stereo input -- the depth of every left keypoint from a rectified pair (epipolar lines are image rows), both pictures resident as
 * slots of this context.  The reference is monocular and RGB-D only; Feature::_depth, ygz_hip_set_keypoint_depths[_batch] and
 * LoopClosing::Options::_fix_scale were waiting for this sensor.  The four steps are those of ORB-SLAM2's Frame::ComputeStereoMatches; the spec is
 * frozen in tests/stereo_ref.c and DESIGN.md section 19, and every output is bit-identical to it.  Per left keypoint (uL, vL, l), with
 * fx_d = (double)fx of the context, bf = fx_d * baseline, minD = min_disparity, maxD = max_disparity or fx_d when that is 0:
 *  1. uL - minD < 0: NO_CANDIDATE.  2. right keypoint j (uR, vR, lr) is a candidate when |lr - l| <= 1, floor(vR - r) <= floor(vL) <= ceil(vR + r)
 *  with r = 2 * 2^lr, and uL - maxD <= uR <= uL - minD; none: NO_CANDIDATE.  3. the candidate with the smallest 256-bit Hamming distance, a tie to
 *  the smallest j; distance >= th_dist: DESCRIPTOR.  4. s = 2^l, su = floor(uL / s + 0.5), sv = floor(vL / s + 0.5), sr = floor(uR / s + 0.5).
 *  5. unless 5 <= su < Wl - 5, 5 <= sv < Hl - 5, sr - 10 >= 0 and sr + 10 < Wl: BORDER.  6. D[inc], inc = -5 .. 5: the sum over the 11 x 11 window
 *  of |(IL(sv + dy, su + dx) - IL(sv, su)) - (IR(sv + dy, sr + inc + dx) - IR(sv, sr + inc))|; k = the smallest inc of the smallest D.
 *  7. k = -5 or 5: EDGE.  8. delta = (D[k-1] - D[k+1]) / (2 (D[k-1] + D[k+1] - 2 D[k])), u_right = s * ((sr + k) + delta), disp = uL - u_right.
 *  9. unless minD <= disp < maxD: DISPARITY; disp <= 0: disp = 0.01, u_right = uL - 0.01.  10. depth = bf / disp, sad = D[k], OK.
 * Per pair: med = element m / 2 of the ascending sad values of the m OK keypoints; an OK keypoint with 10 sad > 21 med becomes MEDIAN.
 * Pixels are finite and below 2^31; levels lie inside the pyramid. */
#define YGZ_STEREO_OK            0
#define YGZ_STEREO_NO_CANDIDATE  1
#define YGZ_STEREO_DESCRIPTOR    2
#define YGZ_STEREO_BORDER        3
#define YGZ_STEREO_EDGE          4
#define YGZ_STEREO_DISPARITY     5
#define YGZ_STEREO_MEDIAN        6
#define YGZ_STEREO_N_STATUS      7
typedef struct {
    double baseline;        /* metres between the two cameras, > 0 (0.1) */
    double min_disparity;   /* >= 0 (0) */
    double max_disparity;   /* >= 0; 0: the context's fx (0) */
    int    th_dist;         /* a best descriptor distance >= th_dist is no match; [0, 256] (75) */
    int    write_depths;    /* slot form: != 0 also sets the left slot's keypoint depths (1) */
} ygz_stereo_params;
void ygz_hip_default_stereo_params(ygz_stereo_params *p);
/* The resident keypoints (ygz_hip_detect) of n_pairs pairs of slots in one call: one upload of the pair table, two launches, one copy back, one
 * wait.  Outputs [n_pairs][max_keypoints] (counts [n_pairs][7], one count per status), each may be NULL; entries past a pair's left keypoints are
 * -1.  right_idx and sad are -1 unless the status is OK or MEDIAN, u_right and depth -1.0 unless it is OK.  With write_depths the left slot's
 * Feature::_depth = depth and _mappoint != nullptr = (status is OK), as ygz_hip_keypoint_depths_from_image sets them from a depth picture; the right
 * slot's are untouched.  YGZ_E_INVALID: a null context, params or slot array, n_pairs < 1, a slot out of range, left == right, a left slot named
 * twice, baseline <= 0, a non-finite or negative parameter, th_dist outside [0, 256]; YGZ_E_STATE: a slot without a pyramid or without keypoints. */
int  ygz_hip_stereo_depths_slots(ygz_hip_ctx *ctx, int n_pairs, const int32_t *left_slot, const int32_t *right_slot, const ygz_stereo_params *params,
                                 int32_t *right_idx, double *u_right, double *depth, int32_t *sad, int32_t *status, int32_t *counts);
/* The same kernels on one pair with the keypoints from host arrays (px [n][2] level-0 pixels, level [n], desc [n][32]) and the pictures of the two
 * slots; outputs [n_l] (counts [7]), each may be NULL.  Never writes depths.  n_l = 0 and n_r = 0 are legal.  In addition YGZ_E_INVALID: a level
 * outside the pyramid; YGZ_E_CAPACITY: n_l or n_r above ygz_hip_max_keypoints. */
int  ygz_hip_stereo_match(ygz_hip_ctx *ctx, int left_slot, int right_slot, const double *px_l, const int32_t *level_l, const uint8_t *desc_l, int n_l,
                          const double *px_r, const int32_t *level_r, const uint8_t *desc_r, int n_r, const ygz_stereo_params *params,
                          int32_t *right_idx, double *u_right, double *depth, int32_t *sad, int32_t *status, int32_t *counts);
/* The stages for tests, array form: best_idx / best_dist [n_l] after step 3 (-1 without a candidate), n_cand [n_l], sads [n_l][11] (-1 where step 6
 * was not reached); each may be NULL. */
int  ygz_hip_stereo_candidates(ygz_hip_ctx *ctx, int left_slot, int right_slot, const double *px_l, const int32_t *level_l, const uint8_t *desc_l, int n_l,
                               const double *px_r, const int32_t *level_r, const uint8_t *desc_r, int n_r, const ygz_stereo_params *params,
                               int32_t *best_idx, int32_t *best_dist, int32_t *n_cand, int32_t *sads);
/* Feature::_depth / _mappoint != nullptr of the keypoints of a slot as they stand on the device (either output may be NULL) */
int  ygz_hip_get_keypoint_depths(ygz_hip_ctx *ctx, int slot, double *depth, uint8_t *has_mappoint, int capacity, int *n);
/* per pair of the resident pair table 32 doubles, reduced on the device: [0..6] pose after sparse alignment, [7] its n_meas / 16,
 * [8..13] pose after pose-only BA [t; log so3], [14] inliers, [15] rounds, [16] cross-checked matches, [17] good matches (M3),
 * [18] min_dis, [19] KLT tracks with status 1, [20] direct-projection successes, [21] reference features, [22] query keypoints, [23] 0,
 * [24..30] the pose-only pose as (qx,qy,qz,qw,tx,ty,tz), [31] 0 */
int  ygz_hip_track_get_summary(ygz_hip_ctx *ctx, double *out /*[capacity_pairs][32]*/, int capacity_pairs, int *n_pairs, int wait);

/* ---- B1-B5: local-BA edge stack -- replaces the per-iteration work g2o does for
 *      EdgeSophusSE3ProjectXYZ (include/ygz/G2oTypes.h:84-132: computeError, linearizeOplus) plus
 *      BaseBinaryEdge::constructQuadraticForm with RobustKernelHuber, as driven by
 *      ba::LocalBAG2O (src/Algorithm/BA.cpp:386-543, optimize() at :501-502) ----------------------- */
typedef struct {
    int n_poses, n_points, n_edges;
    const double  *poses;        /* [n_poses][6]  g2o vertex order [omega; t] (G2oTypes.h:88) */
    const uint8_t *pose_fixed;   /* [n_poses] */
    const double  *points;       /* [n_points][3] */
    const int32_t *edge_pose;    /* [n_edges] */
    const int32_t *edge_point;   /* [n_edges] */
    const double  *obs;          /* [n_edges][2] pixels */
    double fx, fy, cx, cy;       /* G2oTypes.h:60-66 */
    double huber_delta;          /* BA.cpp:451 (5.991); <= 0: no robust kernel */
    int    formulation;          /* 0: pixel residual (G2oTypes.h); 1: normalised plane, pose order
                                    [t; omega] (legacy include/ygz/g2o_types.h:33-86, src/optimizer.cpp);
                                    2: the ceres functors (include/ygz/Ceres/CeresReprojectionError.h:33-69, ...PoseOnly.h:27-58,
                                    ...PointOnly.h:45-77): pose = [t; angle-axis] with additive update, obs in normalised
                                    coordinates, Jacobians = what AutoDiffCostFunction<...,2,6,3> returns */
    /* optional, any formulation (NULL = absent).  They express the ceres problems of src/Algorithm/BA.cpp on one edge
     * list: a PointOnly functor is an edge to a pose with pose_fixed, a PoseOnly functor an edge to a point with
     * point_fixed, SetEnable(false) is edge_enable = 0, ceres::HuberLoss(a) is edge_huber = a. */
    const uint8_t *point_fixed;  /* [n_points] */
    const double  *edge_huber;   /* [n_edges] per-edge Huber width (<= 0: none); NULL: huber_delta for every edge */
    const uint8_t *edge_enable;  /* [n_edges] */
} ygz_ba_problem;
/* Outputs (host, any may be NULL): Hpp [n_poses][36], bp [n_poses][6], Hll [n_points][9],
 * bl [n_points][3], Hpl [n_edges][18] (6x3 = Jpose^T w Jpoint), err [n_edges][2], chi2_edge [n_edges],
 * chi2 = sum of robustified chi2.  Uploads the problem, runs the kernels, downloads. */
int  ygz_hip_ba_linearize(ygz_hip_ctx *ctx, const ygz_ba_problem *pb, double *Hpp, double *bp, double *Hll,
                          double *bl, double *Hpl, double *err, double *chi2_edge, double *chi2);
/* An edge list may hold the same (point, pose) pair more than once (two features of one frame that share a map point, as
 * ba::OptimizeCurrent can produce): every edge contributes to chi2, Hll, bl, Hpp, bp and has its own Hpl block, as ceres / g2o count
 * every residual block.  Only ygz_hip_ba_optimize_resident refuses such a window (YGZ_E_INVALID); ygz_hip_ba_optimize then runs
 * the reduced system on the host. */
/* resident form: upload structure once, then re-linearise for new states without host copies */
int  ygz_hip_ba_upload(ygz_hip_ctx *ctx, int window, const ygz_ba_problem *pb);
int  ygz_hip_ba_set_state(ygz_hip_ctx *ctx, int window, const double *poses, const double *points);
/* same, state already in HBM (device pointers, e.g. the buffer an RCCL broadcast filled); asynchronous */
int  ygz_hip_ba_set_state_device(ygz_hip_ctx *ctx, int window, const double *d_poses, const double *d_points);
int  ygz_hip_ba_linearize_resident(ygz_hip_ctx *ctx, int window_begin, int n_windows);
int  ygz_hip_ba_download(ygz_hip_ctx *ctx, int window, double *Hpp, double *bp, double *Hll, double *bl,
                         double *Hpl, double *err, double *chi2_edge, double *chi2);
/* number of enabled edges whose point lay behind the camera (p_z < 0) in the last linearisation -- the condition on which
 * CeresReprojectionErrorPoseOnly::operator() reports failure (CeresReprojectionErrorPoseOnly.h:48-51) */
int  ygz_hip_ba_behind_camera(ygz_hip_ctx *ctx, int window, int *n_behind);
int  ygz_hip_ba_set_enable(ygz_hip_ctx *ctx, int window, const uint8_t *edge_enable);

/* ---- B4: the LM loop of ba::LocalBAG2O (src/Algorithm/BA.cpp:390-395,501-502: g2o OptimizationAlgorithmLevenberg +
 *      BlockSolver_6_3 with marginalised points).  Linearisations run on the GPU, the reduced pose system on the host.
 *      poses_io [n_poses][6] / points_io [n_points][3] are updated in place (pb->poses / pb->points are ignored). */
typedef struct {
    int    iterations, lm_trials;
    double chi2_initial, chi2_final, lambda_final;
} ygz_ba_stats;
int  ygz_hip_ba_optimize(ygz_hip_ctx *ctx, const ygz_ba_problem *pb, double *poses_io, double *points_io,
                         int max_iterations, ygz_ba_stats *stats);
/* The same plus the inlier pass that follows optimize() in ba::LocalBAG2O (src/Algorithm/BA.cpp:503-515): chi2_edge [n_edges] = every edge's chi2 at
 * the optimised state (what ygz_hip_ba_linearize would return for it), from one more linearisation of the window that is still resident --
 * no second upload of the graph.  chi2_edge == NULL: exactly ygz_hip_ba_optimize. */
int  ygz_hip_ba_optimize_chi2(ygz_hip_ctx *ctx, const ygz_ba_problem *pb, double *poses_io, double *points_io, int max_iterations,
                              ygz_ba_stats *stats, double *chi2_edge);
/* Which loop the last ygz_hip_ba_optimize / ygz_hip_ba_solve_ceres of the context ran.  Both route to the resident kernels
 * (ygz_hip_ba_optimize_resident / ygz_hip_ba_solve_ceres_resident) when the window has at most 20 free poses (14 for the ceres form) and no repeated (point, pose)
 * edge; otherwise the linearisations run on the GPU and the reduced system on the host -- the same results, about ten times slower.
 * Returns YGZ_BA_PATH_RESIDENT, or YGZ_BA_PATH_HOST_LOOP | the reason bits; 0 before the first call. */
enum { YGZ_BA_PATH_RESIDENT = 1, YGZ_BA_PATH_HOST_LOOP = 2, YGZ_BA_WHY_FREE_POSES = 16, YGZ_BA_WHY_REPEATED_EDGES = 32, YGZ_BA_WHY_FORCED = 64 };
int  ygz_hip_ba_last_path(const ygz_hip_ctx *ctx);
/* The resident LM's teams synchronise through a barrier in HBM; members that share an XCD take a light form of it (no L2 write-back).  The light
 * form is self-tested once per context before the first team launch (a message-passing litmus through the barrier itself): 1 = passed and in use,
 * 0 = failed on this device / partition mode (every barrier takes the full form), -1 = no team launch yet.  YGZ_LM_XCD_BARRIER=0 / 1 overrides. */
int  ygz_hip_ba_light_barrier(const ygz_hip_ctx *ctx);
/* The same loop entirely on the GPU for uploaded windows window_begin .. +n_windows-1 (formulation 0, at most 20 free
 * poses per window): one workgroup per window runs linearisation, Schur complement, Cholesky, back-substitution, update and
 * the lambda policy in HBM/LDS without a host round trip, all windows concurrently.  The windows' states are updated in
 * place (ygz_hip_ba_get_state reads them back); stats [n_windows] may be NULL (then the call is asynchronous). */
int  ygz_hip_ba_optimize_resident(ygz_hip_ctx *ctx, int window_begin, int n_windows, int max_iterations,
                                  ygz_ba_stats *stats);
/* A launch of few windows gives every window a TEAM of workgroups (up to 32; results are bit-identical for every team size) as long
 * as windows x team <= budget workgroups; each of them owns a CU for the whole launch.  Default (0): half of the device's CUs.  A
 * pipeline that runs the LM beside other kernels lowers it for those launches (a member that waits for a CU to drain keeps the
 * members already placed spinning) and restores it for the launch nothing else runs beside.  Clamped to [1, CUs]. */
int  ygz_hip_ba_set_team_budget(ygz_hip_ctx *ctx, int workgroups);
/* Where the members of a team run.  0 (default): one XCD per window -- its 32 CUs for the whole launch, the team barrier without an L2
 * write-back (fastest alone); 1: four CUs of every XCD -- the launch leaves seven eighths of every XCD to the kernels of other streams (a
 * pipeline that runs the LM BESIDE other work wants this: every kernel has workgroups on every XCD and waits for the one a team owns).
 * Results are bit-identical either way. */
int  ygz_hip_ba_set_team_placement(ygz_hip_ctx *ctx, int spread);
int  ygz_hip_ba_get_state(ygz_hip_ctx *ctx, int window, double *poses, double *points);
/* statistics of the last ygz_hip_ba_optimize_resident run on each window of the range (it may have been asynchronous) and the graph
 * sizes dims [n][4] = poses, points, edges, free poses; either output may be NULL.  YGZ_E_HIP: a team of workgroups timed out at a
 * barrier (its members were not resident together); YGZ_E_STATE: no resident run yet.  Synchronises. */
int  ygz_hip_ba_get_stats(ygz_hip_ctx *ctx, int window_begin, int n_windows, ygz_ba_stats *stats, int32_t *dims);

/* ---- the keyframe side of a batched run kept in HBM: what LocalMapping::LocalBA gathers on the host before ba::LocalBAG2O
 *      (src/Module/LocalMapping.cpp:149-208: the window's keyframes, their map points and observations; src/Algorithm/BA.cpp:397-470:
 *      vertices and edges) is assembled on the device from a store of keyframe rows, so a BA round moves no keypoint table and no graph
 *      across PCIe.  Contexts of one device share the store: tracking contexts copy their keyframes into it device to device. ---- */
/* order everything enqueued on `waiter` from now on behind everything enqueued on `signaler` so far (same device; no host wait) */
int  ygz_hip_stream_wait(ygz_hip_ctx *waiter, ygz_hip_ctx *signaler);
/* finer: ygz_hip_mark remembers what the context has enqueued so far (e.g. up to an upload); ygz_hip_wait_mark orders what `waiter`
 * enqueues from now on behind signaler's last mark only.  Uploads chained this way cross PCIe first-in-first-out at the full rate. */
int  ygz_hip_mark(ygz_hip_ctx *ctx);
int  ygz_hip_wait_mark(ygz_hip_ctx *waiter, ygz_hip_ctx *signaler);
/* host helper: T_out[0] = identity, T_out[i] = T_rel[i] * T_out[i - 1] (Sophus SE3 product; poses as 7 doubles): the trajectory of a
 * batched run from its per-pair relative poses (VisualOdometry.cpp:66 chains the same product frame by frame).  No device work. */
int  ygz_hip_se3_chain(const double *T_rel, int n, double *T_out);
/* bytes of one keyframe row for this context's grid: pixels f64 [cells][2] | depth f64 [cells] | level i32 [cells] | descriptors
 * [cells][32] | count i32 | (with_images != 0) the keyframe's pyramid, levels 0 .. pyramid_levels - 1 -- each part 64-byte aligned.
 * Rows are fixed-size so that the rows of other ranks arrive by ONE all-gather on the store's memory. */
size_t ygz_hip_kf_row_bytes(const ygz_hip_ctx *ctx, int with_images);
/* a store of n_keyframes rows (+ max_windows rows of work space behind them), the relative pose T_rel of n_frames frames (pose of
 * frame f in the frame of f - 1; (qx,qy,qz,qw,tx,ty,tz)).  rows_mem: device memory of the caller (>= (n_keyframes + max_windows) *
 * row bytes, e.g. a tensor its collectives can address) or NULL to let the library allocate.  with_images != 0: ygz_hip_kf_store_put also
 * copies the keyframe's pyramid into its row (what ygz_hip_ba_build_windows needs for obs_mode 1). */
int  ygz_hip_kf_store_create(ygz_hip_ctx *ctx, int n_keyframes, int n_frames, int max_windows, void *rows_mem, size_t rows_mem_bytes, int with_images);
int  ygz_hip_kf_store_info(ygz_hip_ctx *ctx, void **rows, size_t *row_bytes, void **trel, int *n_keyframes, int *n_frames);
/* row kf_index[i] <- the keypoints (Feature::_pixel, _level, _desc, _depth) of slot src_slot[i] of `src`; enqueued on src's stream */
int  ygz_hip_kf_store_put(ygz_hip_ctx *store, ygz_hip_ctx *src, int n, const int32_t *src_slot, const int32_t *kf_index);
/* T_rel[first_frame + i] <- the pose ygz_hip_track_pose_only left for pair first_pair + i of `src` (on src's stream); the host form
 * for frames tracked elsewhere (asynchronous on the store's stream) */
int  ygz_hip_kf_store_put_trel(ygz_hip_ctx *store, ygz_hip_ctx *src, int first_pair, int n_pairs, int first_frame);
int  ygz_hip_kf_store_set_trel(ygz_hip_ctx *ctx, int first_frame, int n, const double *T_rel);
/* call after a collective wrote rows into the store's memory (re-reads the rows' counts) */
int  ygz_hip_kf_store_refresh(ygz_hip_ctx *ctx);
/* BA windows whose graph the device builds: capacity K keyframes (pose 0 constant, BA.cpp:404) x max_points map points */
int  ygz_hip_ba_reserve_windows(ygz_hip_ctx *ctx, int window_begin, int n_windows, int K, int max_points, double huber_delta);
/* window i = the n_kfs[i] keyframes in store rows kf_index[i][0..K) = frames kf_frame[i][.] of the sequence (ascending; entry 0 is the
 * anchor).  Map points: the anchor's features with depth (first max_points in keypoint order), Pixel2Camera in the anchor's camera
 * (Camera.h:56-62); observations: the anchor's pixel plus, in every other keyframe of the window,
 *   obs_mode 0: the good cross-checked Hamming match of the anchor's descriptor (test/test_orb_match.cpp:86-104);
 *   obs_mode 1: what LocalMapping::ProjectMapPoints leaves there (src/Module/LocalMapping.cpp:47-120): the map point projected with the
 *               chained pose, kept if in front of the camera and InFrame(px, 20) (FindCandidates), refined by Matcher::FindDirectProjection
 *               (Matcher.cpp:356-383) from the anchor's image into the keyframe's; needs a store created with images;
 * points seen by fewer than two keyframes are dropped; vertex j = log of
 * T_rel(kf_frame[j]) * ... * T_rel(anchor + 1) as [omega; upsilon] (G2oTypes.h:88), the anchor at the identity.  Asynchronous;
 * ygz_hip_ba_optimize_resident / ygz_hip_ba_linearize_resident run on the result, ygz_hip_ba_get_stats returns the sizes. */
int  ygz_hip_ba_build_windows(ygz_hip_ctx *ctx, int window_begin, int n_windows, const int32_t *kf_index, const int32_t *kf_frame,
                              const int32_t *n_kfs, int obs_mode);
/* the inlier test after optimize() (src/Algorithm/BA.cpp:503-515): every enabled edge's chi2 (identity information, no robust kernel) at
 * the windows' current state against chi2_threshold (5.991); asynchronous, behind the resident LM of the same windows.  disable != 0:
 * outlier edges are switched off for later runs (the effect of Feature::_bad = true on the next LocalBAG2O, BA.cpp:436).
 * ygz_hip_ba_get_outlier_stats: out [n_windows][4] = edges tested, outliers, chi2 of the tested edges, chi2 of the inliers (-1: not
 * computed since the last resident LM); synchronises. */
int  ygz_hip_ba_mark_outliers(ygz_hip_ctx *ctx, int window_begin, int n_windows, double chi2_threshold, int disable);
int  ygz_hip_ba_get_outlier_stats(ygz_hip_ctx *ctx, int window_begin, int n_windows, double *out);
/* one row per window: [poses 6 K | points 3 max_points | K, P, E, iterations, lm_trials, chi2_initial, chi2_final, lambda_final | edges
 * tested, outliers, chi2 of the tested edges, chi2 of the inliers (ygz_hip_ba_mark_outliers)], unused entries 0, rows row_doubles
 * (>= 6 K + 3 max_points + 12) apart; dst in device memory (dst_on_device != 0: e.g. the buffer of the map exchange) or host memory */
int  ygz_hip_ba_pack_states(ygz_hip_ctx *ctx, int window_begin, int n_windows, double *dst, size_t row_doubles, int dst_on_device, int wait);


/* ---- B6/B7: ceres::Solve as the reference configures it (src/Algorithm/BA.cpp:219-226,372-375: default options =
 *      trust-region Levenberg-Marquardt, Jacobi scaling; :58-62 TwoViewBACeres: DOGLEG) around the GPU linearisation of a formulation-2 problem.
 *      ba::LocalBA, OptimizeCurrent, OptimizeCurrentPointOnly and TwoViewBACeres are this call on different edge lists. */
typedef struct {
    int    max_num_iterations;                       /* 50 */
    double function_tolerance, gradient_tolerance, parameter_tolerance;           /* 1e-6, 1e-10, 1e-8 */
    double initial_trust_region_radius, max_trust_region_radius, min_trust_region_radius;   /* 1e4, 1e16, 1e-32 */
    double min_relative_decrease, min_lm_diagonal, max_lm_diagonal;               /* 1e-3, 1e-6, 1e32 */
    int    jacobi_scaling, max_num_consecutive_invalid_steps;                     /* 1, 5 */
    int    fail_behind_camera;                       /* 1: evaluation fails when an enabled edge has p_z < 0 (PoseOnly) */
    int    trust_region_strategy;                    /* 0 LEVENBERG_MARQUARDT (default), 1 DOGLEG (TRADITIONAL_DOGLEG: ba::TwoViewBACeres, BA.cpp:59-60);
                                                        DOGLEG runs the loop on the host around the GPU linearisations (round 6) */
} ygz_ceres_options;
enum { YGZ_CERES_LEVENBERG_MARQUARDT = 0, YGZ_CERES_DOGLEG = 1 };
enum { YGZ_CERES_FUNCTION_TOLERANCE = 0, YGZ_CERES_GRADIENT_TOLERANCE, YGZ_CERES_PARAMETER_TOLERANCE, YGZ_CERES_MIN_RADIUS,
       YGZ_CERES_NO_CONVERGENCE, YGZ_CERES_FAILURE };
typedef struct {
    int    iterations, successful_steps, unsuccessful_steps, termination;
    double initial_cost, final_cost, final_radius;
} ygz_ceres_summary;
void ygz_hip_ceres_default_options(ygz_ceres_options *opt);
int  ygz_hip_ba_solve_ceres(ygz_hip_ctx *ctx, const ygz_ba_problem *pb, double *poses_io, double *points_io,
                            const ygz_ceres_options *opt, ygz_ceres_summary *summary);
/* The same loop entirely on the GPU for uploaded formulation-2 windows window_begin .. +n_windows-1 (at most 14 free and 16 poses per
 * window, no repeated (point, pose) pair): one workgroup per window runs every trust-region iteration (scaled Schur complement,
 * Cholesky, step validity, candidate cost, radius policy) in HBM / LDS, all windows concurrently; the windows' states are updated
 * in place (ygz_hip_ba_get_state).  summaries [n_windows] may be NULL (then the call is asynchronous).  ygz_hip_ba_solve_ceres
 * uses it when the window qualifies. */
int  ygz_hip_ba_solve_ceres_resident(ygz_hip_ctx *ctx, int window_begin, int n_windows, const ygz_ceres_options *opt,
                                     ygz_ceres_summary *summaries);

/* ---- B7: ba::OptimizeCurrentPoseOnly (src/Algorithm/BA.cpp:188-264; the per-frame call of
 *      LocalMapping::OptimizeCurrent, src/Module/LocalMapping.cpp:126) for a batch of frames: one workgroup per frame runs
 *      the four solve / re-classify rounds entirely on the GPU.  Frame f owns features frame_off[f] .. frame_off[f+1]-1:
 *      px [n][2] pixels (Feature::_pixel), pw [n][3] world points (MapPoint::_pos_world).  poses_io [n_frames][6] =
 *      [t; log(so3)] of _TCW in and out; bad [n] (Feature::_bad), depth [n] (Feature::_depth, written for inliers only,
 *      otherwise left), inliers / rounds [n_frames] (may be NULL).  Intrinsics are the context's camera. */
int  ygz_hip_optimize_pose_only(ygz_hip_ctx *ctx, int n_frames, const int32_t *frame_off, const double *px,
                                const double *pw, double *poses_io, uint8_t *bad, double *depth, int32_t *inliers,
                                int32_t *rounds);

/* ---- P0: stereo pose optimisation -- ORB-SLAM2's Optimizer::PoseOptimization for a batch of frames, the per-frame routine of every stereo and
 * RGB-D system of that family (ygz_hip_optimize_pose_only above is the reference's monocular ceres functor and stays as it is).  Frame f owns the
 * edges frame_off[f] .. frame_off[f+1]-1 (the CSR layout of ygz_hip_optimize_pose_only): pw [n][3] world points, obs [n][3] = (u, v, uR) level-0
 * pixels, level [n] (inside the context's pyramid), kind [n]: 0 absent (never used, never classified), 1 mono (u, v), 2 stereo (u, v, uR).
 * poses_io [n_frames][7] = T_cw as qx qy qz qw tx ty tz, in and out.  The spec is frozen in tests/popt_ref.c and DESIGN.md section 20, and every
 * output is bit-identical to it.  With fx_d .. cy_d the context's float intrinsics as doubles, bf = fx_d * baseline, w = 4^-level, P = R X + t:
 *   r0 = u - (fx x/z + cx), r1 = v - (fy y/z + cy), stereo r2 = uR - (fx x/z + cx - bf/z), chi2 = w |r|^2; an edge is rejected in an evaluation
 *   when !(z > 0) or a residual is not finite (it adds nothing and is counted); g2o's Huber kernel on chi2 with delta^2 = chi2_mono / chi2_stereo.
 * Round k = 0 .. rounds-1: T <- the entry pose; active edges: kind != 0 and not an outlier of the previous classification (round 0: all); the
 * kernel is on while k < robust_rounds; at most `iterations` Levenberg-Marquardt iterations under g2o's rules (lambda0 = 1e-5 max |diag H|, nu = 2,
 * at most max_trials trials per iteration, dense Cholesky of H + lambda I, gain ratio (chi - chi_trial) / (d (lambda d + b) + 1e-3), the
 * min_rel_decrease stop); a trial fails on a bad pivot, a non-finite cost or more rejected edges than the iteration's linearisation had; a round
 * whose first linearisation has fewer than min_edges accepted edges is FAILED and leaves T at the entry pose.  Then every edge with kind != 0 is
 * classified at the round's T by a fresh evaluation (rejected, or chi2 above its threshold: outlier); fewer than min_inliers inliers end the call
 * after this round.  The pose returned is the T of the last round that ran. */
#define YGZ_POPT_MAX_ROUNDS     8
#define YGZ_POPT_MAX_STEPS      64         /* the most `iterations` and the most `max_trials` may be: trials whose pivot fails are retried by one
                                            * lane without a pass in between, so the product bounds how long a frame can hold its workgroup */
#define YGZ_POPT_FAILED         0          /* the values of YGZ_GBA_*, with their meanings */
#define YGZ_POPT_CONVERGED      1
#define YGZ_POPT_MAX_ITERATIONS 2
#define YGZ_POPT_STALLED        3
typedef struct {
    double baseline;          /* metres between the two cameras; no default (0): must be > 0 when a stereo edge exists */
    double chi2_mono;         /* > 0 (5.991): Huber width and outlier threshold of a mono edge */
    double chi2_stereo;       /* > 0 (7.815): of a stereo edge */
    int    rounds;            /* 1 .. 8 (4) */
    int    iterations;        /* 1 .. 64 (10): LM iterations per round */
    int    max_trials;        /* 1 .. 64 (10): trials per iteration */
    int    robust_rounds;     /* the kernel is on in rounds 0 .. robust_rounds-1 (3: ORB-SLAM2 drops it for the last round) */
    int    min_edges;         /* (3) any value: <= 0 lets a frame without an accepted edge run (its trials fail at the pivot) */
    int    min_inliers;       /* (10) any value: <= 0 never ends the call early */
    double min_rel_decrease;  /* (0: off) a round is CONVERGED when an accepted step lowers the cost by no more than this share of it */
} ygz_pose_opt_params;
void ygz_hip_default_pose_opt_params(ygz_pose_opt_params *p);
/* One packed upload, one launch (k_pose_opt: one workgroup per frame), one copy back, one wait.  Outputs, each but poses_io may be NULL:
 * outlier [n] and chi2 [n] of the last classification (chi2 -1.0 for kind 0, 0.0 for a rejected edge, which is an outlier); inliers, rounds_run
 * [n_frames]; round_status (YGZ_POPT_*), round_iterations, round_cost_initial, round_cost_final, round_lambda [n_frames][8], unused rounds zero.
 * All checks run before the device is touched.  YGZ_E_INVALID: a null context, params or required array; n_frames < 0; frame_off[0] != 0 or a
 * non-monotone frame_off; a kind outside {0, 1, 2}; a level outside the context's pyramid; a non-finite parameter; baseline <= 0 with a stereo edge
 * present; a non-positive chi2_*; rounds outside 1 .. 8; iterations or max_trials outside 1 .. 64.  n_frames = 0 and frames without edges are legal: such a
 * frame is FAILED in round 0 and its pose is untouched. */
int  ygz_hip_optimize_pose_stereo(ygz_hip_ctx *ctx, int n_frames, const int32_t *frame_off, const double *pw, const double *obs, const int32_t *level,
                                  const uint8_t *kind, const ygz_pose_opt_params *params, double *poses_io, uint8_t *outlier, double *chi2,
                                  int32_t *inliers, int32_t *rounds_run, int32_t *round_status, int32_t *round_iterations,
                                  double *round_cost_initial, double *round_cost_final, double *round_lambda);

/* ---- cvutils::DepthFromTriangulation (include/ygz/Algorithm/CVUtils.h:18-38) for n ray pairs: the step after
 *      SearchForTriangulation in LocalMapping::CreateNewMapPoints (src/Module/LocalMapping.cpp:430-452).  f_ref / f_cur [n][3]
 *      normalised rays, T_search_ref = (qx,qy,qz,qw,tx,ty,tz); ok[i] = 0 when det(A^T A) < determinant_th (depths untouched). */
int  ygz_hip_depth_from_triangulation(ygz_hip_ctx *ctx, const double T_search_ref[7], const double *f_ref, const double *f_cur,
                                      int n, double determinant_th, double *depth1, double *depth2, uint8_t *ok);

/* ---- the triangulation loop of LocalMapping::CreateNewMapPoints (src/Module/LocalMapping.cpp:416-495, the branch where neither
 *      feature has a map point yet), for n matched pairs (SearchForTriangulation's output) of keyframes in slot1 (current keyframe,
 *      pose T1) and slot2 (neighbour, T2): parallax test, DepthFromTriangulation, Matcher::FindDirectProjection of feature 1 into
 *      frame 2 with the triangulated depth, second triangulation with the refined pixel, reprojection test (5.991 px), map point.
 *      px1 [n][2] / level1 [n]: Feature::_pixel / _level in frame 1; px2 [n][2] in/out: fea2->_pixel (overwritten once the direct
 *      projection succeeded, as the reference does); code [n]: 0 map point created, 1 parallel rays, 2 / 4 first / second
 *      triangulation rejected, 3 direct projection failed, 5 reprojection error; depth1 / depth2 / pos_world [n][3] for code 0. */
int  ygz_hip_create_map_points(ygz_hip_ctx *ctx, int slot1, const double T1[7], int slot2, const double T2[7], int n, const double *px1,
                               const int32_t *level1, double *px2, int32_t *code, double *depth1, double *depth2, double *pos_world,
                               int32_t *search_level, int *n_created);

/* ---- the depth filter of the legacy tree: DepthFilter::UpdateSeeds / UpdateSeed / ComputeTau (src/optimizer.cpp:537-735) with
 *      utils::FindEpipolarMatchDirect (src/utils.cpp:330-661: epipolar ZMSSD search + the legacy Align2D + DepthFromTriangulation),
 *      for n seeds against ONE new frame (cur_slot, T_cur).  Seed i belongs to reference frame seed_ref[i] (ref_slot / T_refs
 *      [n_refs]) whose id for the age test is seed_frame_id[i]; kp [n][2] = cv::KeyPoint::pt, octave [n]; a, b, mu, sigma2 [n] are
 *      updated in place (Seed's Beta / Gaussian parameters, float), z_range [n].  state [n]: 0 updated and kept; 1 behind the camera,
 *      2 outside the frame, 3 no epipolar match (kept unchanged); 4 erased, older than max_n_kfs (5); 5 erased, converged
 *      (sqrt(sigma2) < z_range / convergence_sigma2_thresh (100)): pos_world [n][3] = the new map point; 6 erased, NaN.
 *      z [n] = matched depth, matched_px [n][2].  Needs >= 3 pyramid levels. */
int  ygz_hip_depth_filter_update(ygz_hip_ctx *ctx, int cur_slot, const double T_cur[7], int n_refs, const int32_t *ref_slot,
                                 const double *T_refs, int batch_counter, int max_n_kfs, double convergence_sigma2_thresh, int n,
                                 const float *kp, const int32_t *octave, const int32_t *seed_ref, const uint64_t *seed_frame_id,
                                 float *a, float *b, float *mu, const float *z_range, float *sigma2, int32_t *state, double *z,
                                 double *matched_px, double *pos_world, int *n_updated);

/* ---- M4 / M5: BoW-guided matching -- replaces Frame::ComputeBoW (src/Basic/Frame.cpp:190-201 ->
 *      DBoW3::Vocabulary::transform, thirdparty/DBoW3/src/Vocabulary.cpp:706-835), Matcher::SearchByBoW
 *      (src/Algorithm/Matcher.cpp:196-292) and Matcher::SearchForTriangulation (:86-193, epipolar test :338-354).
 *      The vocabulary is the file ORBVocabulary::loadFromBinaryFile reads (test/test_orb_match.cpp:72-74): header
 *      {u32 nb_nodes, u32 size_node, i32 k, i32 L, i32 scoring, i32 weighting}, then per node {i32 parent, u8 desc[32],
 *      f32 weight, u8 is_leaf}; exactly nb_nodes records are read. */
int  ygz_hip_vocab_load(ygz_hip_ctx *ctx, const void *blob, size_t bytes);
int  ygz_hip_vocab_info(ygz_hip_ctx *ctx, int *k, int *L, int *n_nodes, int *n_words);
/* ComputeBoW over the resident keypoints of a slot range: word id, weight, FeatureVector node (levelsup levels above the leaf;
 * -1 when the word is stopped, i.e. weight <= 0) per keypoint, kept in HBM */
int  ygz_hip_compute_bow(ygz_hip_ctx *ctx, int slot_begin, int n_slots, int levelsup);
int  ygz_hip_get_bow(ygz_hip_ctx *ctx, int slot, int32_t *word, double *weight, int32_t *node, int capacity, int *n);
/* the same for host descriptors [n][32] */
int  ygz_hip_bow_transform(ygz_hip_ctx *ctx, const uint8_t *desc, int n, int levelsup, int32_t *word, double *weight,
                           int32_t *node);
/* mode 0: SearchByBoW (best < th_low and best < knn_ratio * second best); mode 1: SearchForTriangulation (E12 row-major,
 * per pair in the slot form).  match12: index in frame 2 or -1 per feature of frame 1 ([n_pairs][max_keypoints] in the slot
 * form); count(s): number of matches.  Slot form: all pairs in one launch, BoW from ygz_hip_compute_bow. */
int  ygz_hip_search_by_bow_slots(ygz_hip_ctx *ctx, int mode, int n_pairs, const int32_t *slot1, const int32_t *slot2,
                                 const double *E12, int th_low, float knn_ratio, double epipolar_dsqr, int32_t *match12,
                                 int32_t *counts);
int  ygz_hip_search_by_bow(ygz_hip_ctx *ctx, int mode, const uint8_t *desc1, const int32_t *node1, const double *px1, int n1,
                           const uint8_t *desc2, const int32_t *node2, const double *px2, int n2, const double *E12,
                           int th_low, float knn_ratio, double epipolar_dsqr, int32_t *match12, int *count);

/* Matcher::Options::checkOrientation (Matcher.h:24; Matcher.cpp:247-256, 271-289, ComputeThreeMaxima :293-336) on the result of a mode-0
 * search: the 30-bin histogram of rot = angle1 - angle2 over the matches, its three maxima, and kept = the count SearchByBoW returns with
 * the option on (matches outside the three fullest bins are subtracted; the reference does not remove them from the map -- its TODO at
 * :284 -- so match12 is left alone).  SearchForTriangulation only fills the histogram (:157-165) and never reads it: nothing to call.
 * Host form: one pair, Feature::_angle as doubles; slot form: the pairs of ygz_hip_search_by_bow_slots, the resident keypoints' angles.
 * hist ([30] per pair) and maxima ([3] per pair, -1 = none) may be NULL. */
int  ygz_hip_bow_orientation(ygz_hip_ctx *ctx, const double *angle1, int n1, const double *angle2, int n2, const int32_t *match12,
                             int *kept, int32_t *hist, int32_t *maxima);
int  ygz_hip_bow_orientation_slots(ygz_hip_ctx *ctx, int n_pairs, const int32_t *slot1, const int32_t *slot2, const int32_t *match12,
                                   int32_t *kept, int32_t *hist, int32_t *maxima);

/* ---- monocular initialisation: Initializer::TryInitialize (src/Algorithm/Initializer.cpp:9-87) ------------------------------
 * H / F RANSAC over the reference's 8-point sample sets (a fresh cv::RNG per call), model choice rh = sh / (sh + sf) > 0.4, then
 * ReconstructH (8 Faugeras solutions) or ReconstructF (4 solutions of E) with CheckRT per solution and point.  The arithmetic is that of
 * tests/init_ref.c: every output is bit-identical to it. */
#define YGZ_INIT_NONE  0
#define YGZ_INIT_H     1
#define YGZ_INIT_F     2
#define YGZ_INIT_MAX_ITER 1024            /* bound of max_iter */
typedef struct {                          /* Initializer::Option (Algorithm/Initializer.h:41-49) */
    float  sigma;                         /* 2.0 */
    float  sigma2;                        /* 4.0 */
    int    max_iter;                      /* 200 RANSAC iterations (H and F each) */
    double min_parallax;                  /* 1.0 degree (_min_parallex) */
    int    min_triangulated;              /* 8 */
    double good_point_ratio_h;            /* 0.9 */
} ygz_init_params;
typedef struct {
    double  H21[9], F21[9];               /* best homography / fundamental matrix (row-major; 0 when no hypothesis scored above 0) */
    double  R21[9], t21[3];               /* motion of the accepted solution, x2 = R21 x1 + t21 (|t21| = 1); I / 0 when not accepted */
    double  T21[7];                       /* SE3(R21, t21) as qx qy qz qw tx ty tz (Sophus SO3(const Matrix3d &)) */
    double  parallax;                     /* degrees, of the best solution (the 51st smallest parallax of its points) */
    float   score_h, score_f, rh;         /* best scores (float sums in point order), rh = sh / (sh + sf) */
    int32_t success;                      /* TryInitialize's return value */
    int32_t model;                        /* YGZ_INIT_NONE / _H / _F: the model reconstructed from */
    int32_t best_h, best_f;               /* winning hypotheses (-1: none scored above 0) */
    int32_t n_inliers;                    /* inliers of the model reconstructed from */
    int32_t solution;                     /* index of the best solution (0..7 for H, 0..3 for F; -1: none) */
    int32_t n_good, second_good;          /* points of the best and of the second-best solution that pass CheckRT */
    int32_t similar;                      /* F: solutions with more than 0.7 * n_good points (0 for H) */
    int32_t n_triangulated;               /* set entries of triangulated_out */
} ygz_init_result;
void ygz_hip_default_init_params(ygz_init_params *p);
/* The fused call: px1 / px2 [n][2] matched pixels of the reference and the current frame, K4 = fx fy cx cy (PinholeCamera::GetCameraMatrix),
 * params NULL: defaults.  pts3d_out [n][3] (camera-1 coordinates) and triangulated_out [n] (may be NULL) hold the accepted solution's points
 * (0 elsewhere and on failure).  One upload, the launches, one copy back and one wait.  8 <= n <= ygz_hip_max_keypoints (YGZ_E_INVALID /
 * YGZ_E_CAPACITY before anything is launched); result->success is the reference's return value. */
int  ygz_hip_initialize(ygz_hip_ctx *ctx, const double *px1, const double *px2, int n, const double K4[4], const ygz_init_params *params,
                        ygz_init_result *result, double *pts3d_out, uint8_t *triangulated_out);
/* stages, for tests and diagnosis.  The sample sets [max_iter][8] (host only, no context: they depend on n and max_iter alone). */
int  ygz_hip_init_sample_sets(int n, int max_iter, int32_t *sets);
/* every hypothesis: H21 / F21 [max_iter][9] and their scores [max_iter] (each may be NULL), the winners' inlier masks [n] (may be NULL) and
 * in result the fields of the model choice (H21, F21, score_h, score_f, rh, model, best_h, best_f; the rest 0) */
int  ygz_hip_init_hypotheses(ygz_hip_ctx *ctx, const double *px1, const double *px2, int n, const ygz_init_params *params, double *H21,
                             double *F21, float *score_h, float *score_f, uint8_t *inliers_h, uint8_t *inliers_f, ygz_init_result *result);
/* ReconstructH (model YGZ_INIT_H, M = H21) or ReconstructF (YGZ_INIT_F, M = F21) from a given model and its inlier mask [n]: result gets
 * the reconstruction's fields (model, R21, t21, T21, parallax, success, n_inliers, solution, n_good, second_good, similar, n_triangulated; the rest 0) */
int  ygz_hip_init_reconstruct(ygz_hip_ctx *ctx, const double *px1, const double *px2, int n, const double K4[4], const ygz_init_params *params,
                              int model, const double M[9], const uint8_t *inliers, ygz_init_result *result, double *pts3d_out,
                              uint8_t *triangulated_out);


/* ---- relocalisation: 2D-3D pose by P3P RANSAC -- nothing in the reference; it fills the stub at src/Module/VisualOdometry.cpp:101-104
 * ("try relocalization"), as ORB-SLAM2's Tracking::Relocalization does.  Several independent problems per call, one per candidate keyframe:
 * problem p owns the correspondences offsets[p] .. offsets[p+1]-1, a world point pw [N][3] and a level-0 pixel px [N][2] each.  Per problem
 * the sample sets of (n, max_iter) (3 indices per iteration, cv::RNG's scheme of Initializer.cpp:33-49), Lambda Twist P3P with up to 4
 * solutions per sample, the inlier count of every (sample, solution) hypothesis (z > 0 and squared reprojection error <= chi2), the highest
 * count (ties: smallest sample * 4 + solution).  The arithmetic is that of tests/pnp_ref.c: every output is
 * bit-identical to it. */
#define YGZ_PNP_MAX_ITER     1024         /* bound of max_iter */
#define YGZ_PNP_MAX_PROBLEMS 64           /* problems per call */
typedef struct {                          /* ORB-SLAM2 Tracking::Relocalization's values */
    int    max_iter;                      /* 300 */
    double chi2;                          /* 5.991: squared level-0 pixel error of an inlier (OptimizeCurrentPoseOnly's threshold) */
    int    min_inliers;                   /* 10 */
} ygz_pnp_params;
typedef struct {
    double  R[9], t[3];                   /* the winner: camera = R world + t (row-major); I / 0 when no hypothesis has an inlier */
    double  T_cw[7];                      /* SE3(R, t) as qx qy qz qw tx ty tz (Sophus SO3(const Matrix3d &)) */
    int32_t success;                      /* n_inliers >= min_inliers */
    int32_t n_inliers;                    /* inliers of the winner */
    int32_t best_sample, best_solution;   /* the winner (-1 / -1: every hypothesis scored 0) */
    int32_t n_hypotheses;                 /* real solutions over all samples */
} ygz_pnp_result;
void ygz_hip_default_pnp_params(ygz_pnp_params *p);
/* the sample sets [max_iter][3] of a problem of n correspondences (host only, no context: they depend on n and max_iter alone) */
int  ygz_hip_pnp_sample_sets(int n, int max_iter, int32_t *sets);
/* the fused call: K4 = fx fy cx cy, params NULL: defaults; results [n_problems], inliers [N] (may be NULL).  One upload, the launches, one
 * copy back and one wait.  YGZ_E_INVALID: a null context or array, n_problems < 1, offsets not starting at 0, a problem of fewer than 4
 * correspondences, max_iter outside [1, YGZ_PNP_MAX_ITER], chi2 <= 0; YGZ_E_CAPACITY: more than YGZ_PNP_MAX_PROBLEMS problems or a problem
 * larger than ygz_hip_max_keypoints -- all before the device is touched. */
int  ygz_hip_pnp_ransac(ygz_hip_ctx *ctx, int n_problems, const int32_t *offsets, const double *pw, const double *px, const double K4[4],
                        const ygz_pnp_params *params, ygz_pnp_result *results, uint8_t *inliers);
/* stage for tests: every hypothesis of ONE problem -- solutions [max_iter][4][12] (R row-major, t; 0 past n_solutions), n_solutions
 * [max_iter], counts [max_iter][4] (0 past n_solutions); each may be NULL */
int  ygz_hip_pnp_hypotheses(ygz_hip_ctx *ctx, const double *pw, const double *px, int n, const double K4[4], const ygz_pnp_params *params,
                            double *solutions, int32_t *n_solutions, int32_t *counts);

/* ---- loop detection: Sim3 by RANSAC and a 7-dof refinement -- nothing in the reference; LocalMapping.cpp:330 leaves the loop-detection
 * queue as a comment, and this is ORB-SLAM2's LoopClosing::ComputeSim3 (Sim3Solver + Optimizer::OptimizeSim3).  Several independent problems
 * per call, one per candidate keyframe: problem p owns the pairs offsets[p] .. offsets[p+1]-1, each a current-keyframe point X1 [N][3] in the
 * current camera, a candidate point X2 [N][3] in the candidate's camera, their level-0 pixels px1, px2 [N][2] and pyramid levels levels
 * [N][2] (sigma^2 = 4^level).  Per problem the sample sets of ygz_hip_pnp_sample_sets(n, max_iter), Horn's closed form per sample (S12 with
 * S12 X2 ~ X1), the inlier count of every sample (both projections in front and within chi2 sigma^2 of the pixel), the highest count (ties:
 * smallest sample); with min_inliers of them, g2o's LM on S12 over two Huber edges per inlier, a second round without the pairs above
 * chi2_refine.  The arithmetic is that of tests/sim3_ref.c: every output is bit-identical to it. */
#define YGZ_SIM3_MAX_ITER     1024        /* bound of max_iter */
#define YGZ_SIM3_MAX_PROBLEMS 64          /* problems per call */
typedef struct {                          /* ORB-SLAM2 LoopClosing::ComputeSim3 / Optimizer::OptimizeSim3's values */
    int    max_iter;                      /* 300 */
    double chi2;                          /* 9.210: RANSAC inlier threshold, times sigma^2 of the level */
    int    min_inliers;                   /* 20: for RANSAC success and for the refined count */
    double chi2_refine;                   /* 10: the edges' outlier threshold, and the Huber width sqrt(chi2_refine) */
    int    iters_first;                   /* 5: LM iterations of the first round */
    int    iters_more;                    /* 10: of the second round when the first dropped a pair */
    int    iters_again;                   /* 5: of the second round otherwise */
    int    fix_scale;                     /* 0; 1: s = 1 (6-dof) */
} ygz_sim3_params;
typedef struct {
    double  S12[8];                       /* qx qy qz qw tx ty tz s (the order of SE3::to7, then s): S12 X2 = s R X2 + t; identity without a winner */
    double  S21[8];                       /* its inverse */
    double  chi2_ransac;                  /* sum of rho over the winner's inliers before the refinement (0 without one) */
    double  chi2_refined;                 /* sum of rho over the kept pairs after it */
    int32_t success;                      /* n_inliers >= min_inliers and n_refined >= min_inliers */
    int32_t n_hypotheses;                 /* valid samples */
    int32_t best_sample;                  /* the winner (-1: every sample scored 0) */
    int32_t n_inliers;                    /* RANSAC inliers of the winner */
    int32_t n_refined;                    /* pairs with both chi2 <= chi2_refine after the refinement (0 when it did not run) */
    int32_t lm_iterations;                /* LM iterations of both rounds */
} ygz_sim3_result;
void ygz_hip_default_sim3_params(ygz_sim3_params *p);
/* the fused call: K4 = fx fy cx cy, params NULL: defaults; results [n_problems]; inliers [N] (may be NULL): bit 0 a RANSAC inlier of the
 * winner, bit 1 a refined inlier.  One upload, the launches, one copy back and one wait.  YGZ_E_INVALID: a null context or array,
 * n_problems < 1, offsets not starting at 0, a problem of fewer than 3 pairs, max_iter outside [1, YGZ_SIM3_MAX_ITER], chi2 or chi2_refine
 * <= 0, a negative iteration count; YGZ_E_CAPACITY: more than YGZ_SIM3_MAX_PROBLEMS problems or a problem larger than ygz_hip_max_keypoints
 * -- all before the device is touched. */
int  ygz_hip_sim3_ransac(ygz_hip_ctx *ctx, int n_problems, const int32_t *offsets, const double *X1, const double *X2, const double *px1,
                         const double *px2, const int32_t *levels, const double K4[4], const ygz_sim3_params *params, ygz_sim3_result *results,
                         uint8_t *inliers);
/* stage for tests: every sample of ONE problem -- hyps [max_iter][16] (S12 then S21; identities when invalid), valid [max_iter], counts
 * [max_iter] (0 when invalid); each may be NULL */
int  ygz_hip_sim3_hypotheses(ygz_hip_ctx *ctx, const double *X1, const double *X2, const double *px1, const double *px2, const int32_t *levels,
                             int n, const double K4[4], const ygz_sim3_params *params, double *hyps, int32_t *valid, int32_t *counts);

/* ---- loop closing: descriptor search guided by projection -- nothing in the reference; the primitive under ORB-SLAM2's
 * ORBmatcher::SearchBySim3, SearchByProjection(pKF, Scw, points, matched, th) and Fuse(pKF, Scw, points, th, replace).  A problem is one
 * target keyframe and one point set.  Per point, in this order: pt_skip set -> culled; Xc = s (R Pw) + t with R from the quaternion as
 * written (se3_dev.h's quat_to_R_d), kept when z > 0; u = fx (x / z) + cx, v likewise, kept when 0 <= u < image_width and 0 <= v <
 * image_height (the context's); d = |Xc|, culled when d < 0.8 dmax / 2^(L-1) or d > 1.2 dmax (L = the context's pyramid_levels); with
 * pt_normal culled when Xc . (R n) < 0.5 d; the predicted level = the smallest n in [0, L-1] with dmax / d <= 2^n (L-1 when there is none);
 * the candidates = the keypoints that are not taken, with |kx - u| < r and |ky - v| < r for r = th 2^pred, and pred - 1 <= level <= pred;
 * the point's list = the candidates with a 256-bit Hamming distance <= th_dist sorted by (distance, keypoint index), cut to the first
 * YGZ_PROJ_TOPK (a point with more is "overflowed").  Then the claim: claim == 0, a point's match is the head of its list; claim == 1, the
 * points are walked in index order and each takes the first entry of its list that no earlier point took (ORB-SLAM2's sequential
 * vpMatched[bestIdx] = pMP loop).  The arithmetic is that of tests/proj_ref.c: every output is bit-identical to it. */
#define YGZ_PROJ_MAX_PROBLEMS 64          /* problems per call */
#define YGZ_PROJ_TOPK         8           /* entries of a point's candidate list */
#define YGZ_PROJ_MAX_POINTS   65536       /* points per call, over all problems */
typedef struct {
    const double  *kp_px;     /* [n_kp][2] level-0 pixels */
    const int32_t *kp_level;  /* [n_kp] */
    const uint8_t *kp_desc;   /* [n_kp][32] */
    const uint8_t *kp_taken;  /* [n_kp] or NULL: a taken keypoint is never a candidate */
    int            n_kp;
    const double  *pw;        /* [n_pt][3] world position */
    const uint8_t *pt_desc;   /* [n_pt][32] */
    const double  *pt_dmax;   /* [n_pt] scale-invariance distance: |P - O_ref| 2^level_ref */
    const double  *pt_normal; /* [n_pt][3] or NULL: no viewing-angle test */
    const uint8_t *pt_skip;   /* [n_pt] or NULL */
    int            n_pt;
    double         S[8];      /* qx qy qz qw tx ty tz s, world -> target camera: Xc = s (R Pw) + t */
} ygz_proj_problem;
typedef struct {
    double th;                /* 10: window radius at level 0, pixels */
    int    th_dist;           /* 50: largest Hamming distance of a candidate (ORBmatcher::TH_LOW) */
    int    claim;             /* 1 */
} ygz_proj_params;
void ygz_hip_default_proj_params(ygz_proj_params *p);
/* the fused call: K4 = fx fy cx cy, params NULL: defaults.  The outputs are concatenated over the problems and may each be NULL: match [N]
 * keypoint index or -1, dist [N] that match's Hamming distance or -1, pred_level [N] the predicted level or -1 for a point culled before the
 * search, counts [n_problems][2] = matches, overflowed points.  One upload, the launch, one copy back and one wait; the claim is resolved
 * inside the call.  YGZ_E_INVALID: a null context, problem or required array, n_problems < 1, n_kp < 1 or n_pt < 1, th <= 0, th_dist
 * outside [0, 256], s <= 0 or a non-finite S; YGZ_E_CAPACITY: more than YGZ_PROJ_MAX_PROBLEMS problems, n_kp above ygz_hip_max_keypoints,
 * more than YGZ_PROJ_MAX_POINTS points in the call -- all before the device is touched. */
int  ygz_hip_search_by_projection(ygz_hip_ctx *ctx, int n_problems, const ygz_proj_problem *problems, const double K4[4],
                                  const ygz_proj_params *params, int32_t *match, int32_t *dist, int32_t *pred_level, int32_t *counts);
/* stage for tests: the candidate lists of ONE problem before any claim -- cand_idx / cand_dist [n_pt][YGZ_PROJ_TOPK] (-1 past the list),
 * n_cand [n_pt] the candidates within th_dist (above YGZ_PROJ_TOPK: overflowed, the list holds the first YGZ_PROJ_TOPK), pred_level [n_pt];
 * each may be NULL */
int  ygz_hip_projection_candidates(ygz_hip_ctx *ctx, const ygz_proj_problem *problem, const double K4[4], const ygz_proj_params *params,
                                   int32_t *cand_idx, int32_t *cand_dist, int32_t *n_cand, int32_t *pred_level);

/* ---- loop correction: Sim3 pose-graph optimisation -- nothing in the reference; ORB-SLAM2's Optimizer::OptimizeEssentialGraph.  N vertices
 * S [N][8] (qx qy qz qw tx ty tz s, world -> camera i), E edges (i, j) = edges [E][2] with a measurement M [E][8] ~ S_j o S_i^-1, fixed [N]
 * (non-zero: the vertex is not moved).  Minimises the sum over the edges of |lift(M o S_i o S_j^-1)|^2 (identity information) by
 * Levenberg-Marquardt with g2o's rules; every step is solved by block-Jacobi preconditioned conjugate gradients on (J^T J + lambda I) d = b
 * without assembling J^T J; the update is S_i <- Delta(d_i) o S_i with the Delta of the Sim3 refinement, lift is its inverse.  One resident
 * workgroup runs the whole loop.  The arithmetic is that of tests/pgo_ref.c: every output is bit-identical to it. */
#define YGZ_PGO_MAX_VERTICES 4096
#define YGZ_PGO_MAX_EDGES    32768
#define YGZ_PGO_FAILED         0          /* the residual is undefined at the input (a rotation error of 180 degrees, a non-finite value): S_out = S */
#define YGZ_PGO_CONVERGED      1          /* an accepted step lowered the cost by at most min_rel_decrease times the cost */
#define YGZ_PGO_MAX_ITERATIONS 2          /* max_iterations ran */
#define YGZ_PGO_STALLED        3          /* max_trials rejected steps in a row, a step that left the cost unchanged, or lambda overflowed */
typedef struct {
    int32_t max_iterations;               /* 20: LM iterations (ORB-SLAM2's optimize(20)), in [1, 1000] */
    int32_t max_trials;                   /* 10: trials of lambda per iteration, in [1, 100] */
    int32_t cg_max_iterations;            /* 0: min(7 free vertices, 2048); else the cap itself, up to 65536 */
    int32_t fix_scale;                    /* 0; 1: no vertex changes its scale (6-dof) */
    double  cg_tol;                       /* 1e-8: CG stops at r^T z <= cg_tol^2 r0^T z0; in (0, 1) */
    double  min_rel_decrease;             /* 1e-9: in [0, 1) */
} ygz_pgo_params;
typedef struct {
    double  cost_initial, cost_final;     /* the sum of squared residuals at S and at S_out */
    double  lambda;                       /* the final damping */
    int32_t status;                       /* YGZ_PGO_* */
    int32_t lm_iterations;
    int32_t n_solves;                     /* CG solves (trials whose preconditioner could be factored) */
    int32_t cg_iterations_total;
    int32_t cg_capped;                    /* solves that ended at the cap (not an error: the iterate is used) */
    int32_t pad;
} ygz_pgo_result;
void ygz_hip_default_pgo_params(ygz_pgo_params *p);
/* the whole optimisation: params NULL: defaults; S_out [N][8].  One upload, one launch, one copy back and one wait.  Checked in this order,
 * all before the device is touched: YGZ_E_INVALID for a null array or result; YGZ_E_CAPACITY above YGZ_PGO_MAX_VERTICES vertices or
 * YGZ_PGO_MAX_EDGES edges; YGZ_E_INVALID for N < 2, E < 1, no free vertex, an edge with i = j or an index out of range, a free vertex
 * without an edge, a scale <= 0 or a non-finite value in S or M, a parameter out of its range; last, YGZ_E_INVALID for a null context. */
int  ygz_hip_pose_graph_optimize(ygz_hip_ctx *ctx, int n_vertices, const double *S, const uint8_t *fixed, int n_edges, const int32_t *edges,
                                 const double *M, const ygz_pgo_params *params, double *S_out, ygz_pgo_result *result);
/* stage for tests: the linearisation at S -- residuals [E][7], Ji and Jj [E][49] (dr / dd_i and dr / dd_j, row-major), cost [1]; each may
 * be NULL.  The same checks.  Returns YGZ_E_STATE when the residual is undefined at S (the outputs are zero for such an edge). */
int  ygz_hip_pgo_linearize(ygz_hip_ctx *ctx, int n_vertices, const double *S, const uint8_t *fixed, int n_edges, const int32_t *edges,
                           const double *M, const ygz_pgo_params *params, double *residuals, double *Ji, double *Jj, double *cost);

/* ---- map upkeep after a loop correction -- nothing in the reference (MapPoint::ComputeDistinctiveDesc is shipped commented out, the
 * covisibility weights exist only as Frame::UpdateConnections); ORB-SLAM2's MapPoint::ComputeDistinctiveDescriptors and the counting of
 * KeyFrame::UpdateConnections, for many points at once.  The observations of point p are rows offsets[p] .. offsets[p+1]-1 of the per-
 * observation array, in the caller's order.  Every output is an integer and bit-identical to tests/map_ref.c. */
#define YGZ_MAP_MAX_OBS_PER_POINT 256     /* observations of one point (descriptors) */
#define YGZ_MAP_MAX_OBS           1048576 /* observations per call */
#define YGZ_MAP_MAX_KEYFRAMES     4096    /* K */
#define YGZ_COVIS_MAX_CELLS       4194304 /* n_rows x K */
/* per point with n observations desc [n_obs][32]: d(i, j) the 256-bit Hamming distance, d(i, i) = 0; the median of observation i is element
 * (n - 1) / 2 of its distance row sorted ascending, the self distance included; best [n_points] is the smallest i with the smallest median,
 * median [n_points] (or NULL) that value, out_desc [n_points][32] (or NULL) that observation's bytes; n = 0 gives -1, -1 and zeros.  One
 * upload, one launch, one copy back and one wait.  Checked in this order, all before the device is touched: YGZ_E_INVALID for a null offsets,
 * desc or best, n_points < 1, offsets[0] != 0 or a decreasing offset; YGZ_E_CAPACITY for a point with more than YGZ_MAP_MAX_OBS_PER_POINT
 * observations or more than YGZ_MAP_MAX_OBS in the call; last, YGZ_E_INVALID for a null context. */
int  ygz_hip_distinctive_descriptors(ygz_hip_ctx *ctx, int n_points, const int32_t *offsets, const uint8_t *desc, int32_t *best,
                                     int32_t *median, uint8_t *out_desc);
/* kf [n_obs] holds keyframe indices in [0, n_keyframes), strictly ascending within a point; rows [n_rows] distinct keyframe indices in any
 * order.  weights [n_rows][n_keyframes]: weights[r][b] for b != rows[r] is the number of points whose list holds both rows[r] and b,
 * weights[r][rows[r]] the number of points whose list holds rows[r].  One upload, the clear and the launch, one copy back and one wait.
 * Checked in this order, all before the device is touched: YGZ_E_INVALID for a null array; YGZ_E_CAPACITY for n_keyframes above
 * YGZ_MAP_MAX_KEYFRAMES; YGZ_E_INVALID for n_keyframes < 1 or n_rows < 1; YGZ_E_CAPACITY for n_rows x n_keyframes above YGZ_COVIS_MAX_CELLS;
 * YGZ_E_INVALID for n_points < 1, offsets[0] != 0 or a decreasing offset; YGZ_E_CAPACITY for more than YGZ_MAP_MAX_OBS observations;
 * YGZ_E_INVALID for an index out of range, a list that is not strictly ascending or a repeated row; last, for a null context. */
int  ygz_hip_covisibility(ygz_hip_ctx *ctx, int n_points, const int32_t *offsets, const int32_t *kf, int n_keyframes, int n_rows,
                          const int32_t *rows, int32_t *weights);

/* ---- global bundle adjustment after a loop closing -- nothing in the reference; ORB-SLAM2's Optimizer::GlobalBundleAdjustemnt.  N poses
 * [N][7] (qx qy qz qw tx ty tz, world -> camera), fixed [N] (non-zero: the pose is not moved), L points [L][3], E edges: edge e observes point
 * edge_point[e] from pose edge_pose[e] at the pixel obs[e]; a (point, pose) pair may appear more than once, and each edge counts.  One
 * pinhole camera K4 = fx fy cx cy.  Minimises the sum over the edges of rho(|obs - K (R X + t) / z|^2), identity information, rho g2o's Huber
 * kernel of width huber_delta (5.991 in ORB-SLAM2; <= 0: no kernel), by Levenberg-Marquardt with g2o's rules.  Every step marginalises the
 * points and solves the reduced camera system by preconditioned conjugate gradients without forming it (the preconditioner: every pose's
 * 6x6 diagonal block of that system); the update is T <- Delta(d) o T with q_Delta = normalise(omega / 2, 1), X <- X + d.  Many workgroups,
 * one short kernel per phase; the host queues CG iterations in batches and reads one small record back per batch.  The arithmetic is that
 * of tests/gba_ref.c: every output is bit-identical to it, whatever cg_batch is. */
#define YGZ_GBA_MAX_POSES  4096
#define YGZ_GBA_MAX_POINTS 1048576
#define YGZ_GBA_MAX_EDGES  4194304
#define YGZ_GBA_FAILED         0          /* at the input a point is not in front of one of its cameras, or a value is not finite: outputs = inputs */
#define YGZ_GBA_CONVERGED      1          /* the values of YGZ_PGO_*, with their meanings */
#define YGZ_GBA_MAX_ITERATIONS 2
#define YGZ_GBA_STALLED        3
typedef struct {
    int32_t max_iterations;               /* 10: LM iterations (the nIterations of ORB-SLAM2's RunGlobalBundleAdjustment), in [1, 1000] */
    int32_t max_trials;                   /* 10: trials of lambda per iteration, in [1, 100] */
    int32_t cg_max_iterations;            /* 0: min(6 free poses, 1024); else the cap itself, up to 65536 */
    int32_t cg_batch;                     /* 0: 8; CG iterations queued between two read-backs of the control record, up to 1024; no output depends on it */
    double  cg_tol;                       /* 1e-8: CG stops at r^T z <= cg_tol^2 r0^T z0; in (0, 1) */
    double  min_rel_decrease;             /* 1e-9: in [0, 1) */
} ygz_gba_params;
typedef struct {
    double  cost_initial, cost_final;     /* the robust cost at the input and at the output */
    double  lambda;                       /* the final damping */
    int32_t status;                       /* YGZ_GBA_* */
    int32_t lm_iterations;
    int32_t n_solves;                     /* CG solves (trials whose blocks could all be factored) */
    int32_t cg_iterations_total;
    int32_t cg_capped;                    /* solves that ended at the cap (not an error: the iterate is used) */
    int32_t pad;
} ygz_gba_result;
void ygz_hip_default_gba_params(ygz_gba_params *p);
/* the whole optimisation: params NULL: defaults; poses_out [N][7], points_out [L][3].  Checked in this order, all before the device is
 * touched: YGZ_E_INVALID for a null array, output or result; YGZ_E_CAPACITY, by the counts alone, above YGZ_GBA_MAX_POSES poses,
 * YGZ_GBA_MAX_POINTS points or YGZ_GBA_MAX_EDGES edges; YGZ_E_INVALID for N < 2, L < 1 or E < 1, a parameter out of its range, a non-finite
 * K4 or huber_delta or a focal length <= 0, an index out of range, a non-finite observation, pose or point, a zero quaternion, a free pose
 * without an edge, no free pose, a point with fewer than 2 edges; last, YGZ_E_INVALID for a null context. */
int  ygz_hip_global_ba(ygz_hip_ctx *ctx, int n_poses, const double *poses, const uint8_t *fixed, int n_points, const double *points, int n_edges,
                       const int32_t *edge_pose, const int32_t *edge_point, const double *obs, const double K4[4], double huber_delta,
                       const ygz_gba_params *params, double *poses_out, double *points_out, ygz_gba_result *result);
/* stage for tests: the linearisation at the input -- residuals [E][2], weights [E] (rho'), Jp [E][12] (dr / d(omega, t), 2x6 row-major), Jl
 * [E][6] (dr / dX, 2x3), Hpp [N][21] and Hll [L][6] (upper triangles row by row; rows of fixed poses are zero), bp [N][6], bl [L][3], cost
 * [1]; each may be NULL.  The same checks (without the outputs).  Returns YGZ_E_STATE when a residual is undefined (zeros for such an edge). */
int  ygz_hip_gba_linearize(ygz_hip_ctx *ctx, int n_poses, const double *poses, const uint8_t *fixed, int n_points, const double *points,
                           int n_edges, const int32_t *edge_pose, const int32_t *edge_point, const double *obs, const double K4[4],
                           double huber_delta, const ygz_gba_params *params, double *residuals, double *weights, double *Jp, double *Jl,
                           double *Hpp, double *bp, double *Hll, double *bl, double *cost);

/* ---- stereo bundle adjustment -- nothing in the reference; ORB-SLAM2's Optimizer::LocalBundleAdjustment / GlobalBundleAdjustemnt with mono
 * and stereo edges.  The problem of ygz_hip_global_ba with obs [E][3] = (u, v, uR), kind [E] (0 absent, 1 mono, 2 stereo: uR of a mono edge
 * and all of an absent edge are never read) and level [E] inside the context's pyramid: the information is 4^-level, a stereo edge adds the
 * residual uR - (fx x / z + cx - bf / z) with bf = fx * baseline, and g2o's Huber kernel acts on chi2 = w |r|^2 with delta^2 = chi2_mono or
 * chi2_stereo.  Round k = 0 .. rounds - 1: the active edges are the present ones that the last classification did not flag (round 0: all
 * present), the kernel is on while k < robust_rounds, the Levenberg-Marquardt loop and inner solve of ygz_hip_global_ba run from the
 * current estimate for at most iterations[k] iterations (lambda_0 anew, the counters from zero); then every present edge is classified at
 * the round's final state by a fresh evaluation without kernel: an edge whose point is not in front of its camera is an outlier with chi2
 * 0, chi2 above chi2_mono / chi2_stereo is an outlier.  An absent or inactive edge keeps its place in every sum and adds exact zeros, so a
 * call on the compacted edge list is not promised the same bits.  YGZ_GBA_FAILED (an active edge undefined at the input) can only arise in
 * round 0: the outputs are the inputs, the flags those of a classification at the input, rounds_run 1.  The arithmetic is that of
 * tests/sba_ref.c: every output is bit-identical to it, whatever cg_batch is. */
#define YGZ_SBA_MAX_ROUNDS 4
typedef struct {
    int32_t max_iterations;               /* 10: kept from ygz_gba_params and checked like it; the rounds use iterations[] */
    int32_t max_trials;                   /* 10 */
    int32_t cg_max_iterations;            /* 0 */
    int32_t cg_batch;                     /* 0 */
    double  cg_tol;                       /* 1e-8 */
    double  min_rel_decrease;             /* 1e-9 */
    double  baseline;                     /* 0: no default; > 0 when a stereo edge is present */
    double  chi2_mono, chi2_stereo;       /* 5.991, 7.815: > 0 */
    int32_t rounds;                       /* 2: in [1, YGZ_SBA_MAX_ROUNDS] */
    int32_t robust_rounds;                /* 1: in [0, YGZ_SBA_MAX_ROUNDS] */
    int32_t iterations[YGZ_SBA_MAX_ROUNDS];   /* 5, 10, 0, 0: each of the first `rounds` entries in [1, 1000] */
} ygz_sba_params;
typedef struct {                          /* per round; unused rounds are zero */
    double  cost_initial[YGZ_SBA_MAX_ROUNDS], cost_final[YGZ_SBA_MAX_ROUNDS], lambda[YGZ_SBA_MAX_ROUNDS];
    int32_t rounds_run;
    int32_t launches;                     /* kernels the call queued: a host count, what cg_batch trades against read-backs */
    int32_t status[YGZ_SBA_MAX_ROUNDS];   /* YGZ_GBA_* */
    int32_t lm_iterations[YGZ_SBA_MAX_ROUNDS], n_solves[YGZ_SBA_MAX_ROUNDS], cg_iterations[YGZ_SBA_MAX_ROUNDS], cg_capped[YGZ_SBA_MAX_ROUNDS];
    int32_t inliers[YGZ_SBA_MAX_ROUNDS];  /* present edges that the round's classification did not flag */
} ygz_sba_result;
void ygz_hip_default_sba_params(ygz_sba_params *p);
/* the whole optimisation: params NULL: defaults (refused when a stereo edge is present: the baseline has none); poses_out [N][7],
 * points_out [L][3]; outlier [E] and chi2 [E] (-1.0 for an absent edge) are those of the last classification and may be NULL.  Checked
 * in the order of ygz_hip_global_ba, all before the device is touched, the degree rules counting present edges only; in addition
 * YGZ_E_INVALID for chi2_mono or chi2_stereo not > 0 or not finite (and, with ygz_gba_params' rule, for a max_iterations outside [1, 1000]
 * although no round reads it: leave it at its default), rounds, robust_rounds or a used iterations entry out of range (with
 * the parameters), a kind above 2 or a level outside the pyramid (with the indices), a non-finite observation that the edge's kind uses,
 * a baseline not > 0 or not finite while a stereo edge is present; last, YGZ_E_INVALID for a null context. */
int  ygz_hip_stereo_ba(ygz_hip_ctx *ctx, int n_poses, const double *poses, const uint8_t *fixed, int n_points, const double *points, int n_edges,
                       const int32_t *edge_pose, const int32_t *edge_point, const double *obs, const uint8_t *kind, const int32_t *level,
                       const double K4[4], const ygz_sba_params *params, double *poses_out, double *points_out, uint8_t *outlier, double *chi2,
                       ygz_sba_result *result);
/* stage for tests: the linearisation at the input, every present edge active, the kernel on iff robust_rounds > 0 -- residuals [E][3],
 * weights [E] (rho' w), Jp [E][18] (3x6 row-major), Jl [E][9] (3x3), Hpp [N][21], bp [N][6], Hll [L][6], bl [L][3], cost [1]; each may be
 * NULL.  The same checks (without the outputs).  Returns YGZ_E_STATE when a present edge is undefined (zeros for such an edge). */
int  ygz_hip_sba_linearize(ygz_hip_ctx *ctx, int n_poses, const double *poses, const uint8_t *fixed, int n_points, const double *points,
                           int n_edges, const int32_t *edge_pose, const int32_t *edge_point, const double *obs, const uint8_t *kind,
                           const int32_t *level, const double K4[4], const ygz_sba_params *params, double *residuals, double *weights,
                           double *Jp, double *Jl, double *Hpp, double *bp, double *Hll, double *bl, double *cost);

/* ---- keyframe database: place-recognition queries -- nothing in the reference (its relocalisation and loop detection are stubs); ORB-SLAM2's
 * KeyFrameDatabase over DBoW3's L1 scoring.  The BoW vectors of the keyframes live in HBM; one launch gives, for up to YGZ_KFDB_MAX_QUERIES
 * query vectors, the common-word count and the L1 score against every stored row.
 *  - a vector is n pairs (word, weight): words >= 0 and strictly ascending, weights finite and > 0;
 *  - add appends a row and returns its entry id 0, 1, 2, ...; ids are never reused; n = 0 is a legal row; one upload;
 *  - erase marks a row dead (erasing a dead row is YGZ_OK and changes nothing); clear empties the database and restarts the ids at 0;
 *  - device memory grows geometrically with a device-to-device copy: add never fails for lack of room below the caps;
 *  - query, for every query q and every entry e < n_entries, at [q][e]: a dead entry gives common = -1 and score = 0; otherwise common is the
 *    number of words the two vectors share and score = -s / 2, where s starts at 0.0 and receives s += fabs(v - w) - fabs(v) - fabs(w) (v the
 *    query's weight, w the row's) for each shared word in ascending word order, one addition after the other: DBoW3::L1Scoring::score.  One
 *    upload of the queries, one launch on the context's stream, one copy back and one wait.
 * Every output is bit-identical to tests/kfdb_ref.c.  Checked in this order, all before the device is touched:
 * YGZ_E_INVALID for a null array or output (the arrays of an add with n = 0 may be null); YGZ_E_CAPACITY, by the counts alone, for a vector above
 * YGZ_KFDB_MAX_WORDS words, an add to a database that ever held YGZ_KFDB_MAX_ENTRIES rows since its last clear, more than YGZ_KFDB_MAX_QUERIES
 * queries; YGZ_E_INVALID for n < 0, n_queries < 1, q_offsets[0] != 0 or a decreasing offset, a negative or non-ascending word, a weight that
 * is not finite and > 0, an erase of an id never given, a query on a database without rows; last, YGZ_E_INVALID for a null db or ctx.  The
 * database belongs to its context, is used by one thread at a time like it, and is destroyed before it. */
#define YGZ_KFDB_MAX_ENTRIES 4096   /* rows ever added to one database (= YGZ_MAP_MAX_KEYFRAMES) */
#define YGZ_KFDB_MAX_WORDS   8192   /* words of one vector, stored or queried */
#define YGZ_KFDB_MAX_QUERIES 64     /* queries per call */
typedef struct ygz_kfdb ygz_kfdb;
int  ygz_hip_kfdb_create (ygz_hip_ctx *ctx, ygz_kfdb **db);
void ygz_hip_kfdb_destroy(ygz_kfdb *db);
int  ygz_hip_kfdb_add    (ygz_kfdb *db, const int32_t *word, const double *weight, int n, int32_t *entry);
int  ygz_hip_kfdb_erase  (ygz_kfdb *db, int32_t entry);
int  ygz_hip_kfdb_clear  (ygz_kfdb *db);
/* each output may be NULL; n_entries: ids given since the last clear; n_alive: those not erased; n_words: the words of all of them, dead rows
 * included (their memory comes back with clear) */
int  ygz_hip_kfdb_info   (const ygz_kfdb *db, int32_t *n_entries, int32_t *n_alive, int64_t *n_words);
/* q_offsets [n_queries + 1]: query q is q_word / q_weight [q_offsets[q] .. q_offsets[q + 1]); common and score [n_queries][n_entries] */
int  ygz_hip_kfdb_query  (ygz_kfdb *db, int n_queries, const int32_t *q_offsets, const int32_t *q_word, const double *q_weight,
                          int32_t *common, double *score);

/* ---- keyframe culling -- the reference has the stage written and switched off (LocalMapping::KeyFrameCulling, LocalMapping.cpp:579-618, its
 * call at :327 commented out); ORB-SLAM2's LocalMapping::KeyFrameCulling.  The input is ygz_hip_covisibility's point-major CSR plus one array:
 * kf [n_obs] keyframe indices in [0, n_keyframes), strictly ascending within a point, level [n_obs] the pyramid level of the observing
 * feature, in [0, 15].  The state is removed [K] (all 0), live [p] (the length of p's list) and dead [p] (all 0).  Under a state
 *  - tracked(a) is the number of points with dead = 0 whose list holds a;
 *  - redundant(a) the number of those for which at least th_obs entries b of the list have b != a, removed[b] = 0 and (level_slack < 0 or
 *    level_b <= level_a + level_slack): the reference's `_obs.size() > th_obs` followed by `nobs >= th_obs`.
 * The walk visits the candidates in the caller's order.  Candidate c is culled exactly when (double)redundant > ratio * (double)tracked (one
 * multiplication, one comparison: never when tracked is 0).  A cull sets removed[c] = 1 and takes one `live` from every point of c; a point
 * whose live falls below min_obs gets dead = 1 and never counts again.  A point is never dead before a removal has touched it.  Every output is
 * an integer and bit-identical to tests/cull_ref.c. */
#define YGZ_CULL_MAX_KEYFRAMES 4096       /* K and n_cand (= YGZ_MAP_MAX_KEYFRAMES) */
typedef struct {
    int32_t th_obs;                       /* 3 (LocalMapping.cpp:591): observers that make a point redundant, in [1, 256] */
    int32_t level_slack;                  /* -1: no scale test (the reference's rule); >= 0: ORB-SLAM2's scaleLevel_b <= scaleLevel_a + slack (it uses 1); in [-1, 15] */
    int32_t min_obs;                      /* 2: a point needs this many live observations to stay in the map, in [0, 256] */
    int32_t pad;
    double  ratio;                        /* 0.9 (LocalMapping.cpp:615), in [0, 1] */
} ygz_cull_params;
void ygz_hip_default_cull_params(ygz_cull_params *p);
/* the counts of every keyframe on the initial state: tracked and redundant [n_keyframes].  params NULL: defaults.  Many workgroups that reduce
 * in LDS before they touch a global counter; one upload, the clear and the launch, one copy back and one wait.  Checked in this order, all before
 * the device is touched: YGZ_E_INVALID for a null array; YGZ_E_CAPACITY for n_keyframes above YGZ_CULL_MAX_KEYFRAMES; YGZ_E_INVALID for th_obs
 * outside [1, 256], min_obs outside [0, 256], level_slack outside [-1, 15], a ratio that is not finite or outside [0, 1], n_points < 1,
 * n_keyframes < 1, offsets[0] != 0 or a decreasing offset; YGZ_E_CAPACITY for a point with more than YGZ_MAP_MAX_OBS_PER_POINT observations or
 * more than YGZ_MAP_MAX_OBS in the call; YGZ_E_INVALID for an index out of range, a list that is not strictly ascending or a level outside
 * [0, 15]; last, for a null context. */
int  ygz_hip_keyframe_redundancy(ygz_hip_ctx *ctx, int n_points, const int32_t *offsets, const int32_t *kf, const int32_t *level, int n_keyframes,
                                 const ygz_cull_params *params, int32_t *tracked, int32_t *redundant);
/* the whole walk over cand [n_cand], distinct keyframe indices: culled [n_cand] (0 / 1), tracked and redundant [n_cand] the counts each
 * decision was made on, point_dead [n_points] (or NULL) the dead flags of the final state.  The entry point builds the keyframe-major index of
 * the candidates' observations beside the upload; one resident workgroup steps through the candidates and strides over a candidate's
 * observations, however many.  One upload, one launch, one copy back and one wait.  The checks of ygz_hip_keyframe_redundancy, with n_cand
 * beside n_keyframes (YGZ_E_CAPACITY above YGZ_CULL_MAX_KEYFRAMES, YGZ_E_INVALID below 1) and, before the null context, YGZ_E_INVALID for a
 * candidate out of range or repeated. */
int  ygz_hip_cull_keyframes(ygz_hip_ctx *ctx, int n_points, const int32_t *offsets, const int32_t *kf, const int32_t *level, int n_keyframes,
                            int n_cand, const int32_t *cand, const ygz_cull_params *params, int32_t *culled, int32_t *tracked,
                            int32_t *redundant, uint8_t *point_dead);

/* ---- stereo map-point creation -- nothing in the reference, whose LocalMapping::CreateNewMapPoints (ygz_hip_create_map_points) is monocular;
 * ORB-SLAM2's two creation paths for a rectified rig (bf = fx * baseline; the pyramid's factor is 2: sigma^2 of level l is 4^l).  Poses are
 * qx qy qz qw tx ty tz, world -> camera, unit quaternions; K4 = fx fy cx cy.  The arithmetic is that of tests/smap_ref.c (DESIGN.md section
 * 24): FP64, uncontracted, no trigonometry; every output is bit-identical to it.
 *
 * Pairs (LocalMapping::CreateNewMapPoints with stereo): a problem is one (keyframe 1, keyframe 2) with its poses and n matched pairs -- px1,
 * px2 [n][2] level-0 pixels, level1, level2 [n], ur1, ur2 [n] (< 0: the side is mono), depth1, depth2 [n] (read only where the side's ur is
 * >= 0; may be NULL when no side of the problem is stereo).  Per pair, the first failing step sets the code:
 *   rays xn = ((u - cx) / fx, (v - cy) / fy, 1), ray = R^T xn, cosRays = ray1 . ray2 / (|ray1| |ray2|);
 *   stereo parallax cosS_k = (d_k^2 - b^2 / 4) / (d_k^2 + b^2 / 4) for side 1 when stereo, for side 2 only when side 1 is not stereo; a side
 *   without it keeps cosRays + 1; cosS = min(cosS_1, cosS_2);
 *   cosRays < cosS && cosRays > 0 && (stereo1 || stereo2 || cosRays < cos_parallax_max): method 1, linear triangulation (the null vector of the
 *   rows xn.x T.row(2) - T.row(0), xn.y T.row(2) - T.row(1) of both cameras by a one-sided Jacobi; a fourth component of 0 or a non-finite
 *   point: code 2); else stereo1 && cosS_1 < cosS_2: method 2, feature 1 un-projected with depth1; else stereo2 && cosS_2 < cosS_1: method 3,
 *   feature 2 with depth2; else code 1 (method 0);
 *   z1 <= 0: code 3; z2 <= 0: code 4; the reprojection in camera 1, then 2 (codes 5, 6): ex^2 + ey^2 > chi2_mono 4^level for a mono side,
 *   ex^2 + ey^2 + (u - bf / z - ur)^2 > chi2_stereo 4^level for a stereo side; a distance to a camera centre of 0: code 7; with ratioDist =
 *   dist2 / dist1 and ratioOctave = 2^level1 / 2^level2, ratioDist ratio_factor < ratioOctave || ratioDist > ratioOctave ratio_factor: code 8;
 *   code 0: pos_world is the point (zero for every other code). */
#define YGZ_SMAP_MAX_PROBLEMS 32
#define YGZ_SMAP_MAX_PAIRS    65536      /* per call, over all problems */
typedef struct {
    double  baseline;                     /* 0.1: metres between the rig's cameras, > 0 */
    double  chi2_mono, chi2_stereo;       /* 5.991, 7.8 (ORB-SLAM2's value in this function, not 7.815): > 0 */
    double  cos_parallax_max;             /* 0.9998: two mono sides are triangulated below it only; > 0 */
    double  ratio_factor;                 /* 3.0 = 1.5 x the pyramid's factor 2; >= 1 */
    double  th_depth;                     /* 3.5 metres: a keyframe's feature up to it is close; > 0 */
    int32_t min_close;                    /* 100: at least this many of the nearest features are walked; >= 0 */
    int32_t pad;
} ygz_smap_params;
typedef struct {
    double T1[7], T2[7];
    const double *px1, *px2, *ur1, *ur2, *depth1, *depth2;
    const int32_t *level1, *level2;
    int n;
} ygz_smap_problem;
void ygz_hip_default_smap_params(ygz_smap_params *p);
/* all pairs of all problems in one launch; the outputs run over the concatenated pairs in problem order: code, method [N], pos_world [N][3];
 * counts [n_problems][2] (created = code 0, triangulated = code 0 by method 1) may be NULL.  params NULL: defaults.  One upload, one launch,
 * one copy back and one wait.  Checked in this order, all before the device is touched: YGZ_E_INVALID for null problems, K4, code, method or
 * pos_world or n_problems < 1; YGZ_E_CAPACITY above YGZ_SMAP_MAX_PROBLEMS; YGZ_E_INVALID for a problem's n < 0; YGZ_E_CAPACITY above
 * YGZ_SMAP_MAX_PAIRS pairs in the call; YGZ_E_INVALID for a parameter that is not finite, baseline, a chi2, cos_parallax_max or th_depth <= 0,
 * ratio_factor < 1, min_close < 0, a non-finite K4 or a focal length <= 0, a non-finite pose, a null array of a problem with n > 0 (depth_k
 * only when a ur_k is >= 0), a non-finite pixel or ur, a non-finite depth of a stereo side; last, YGZ_E_INVALID for a null context and for a
 * level outside the context's pyramid.  A problem with n = 0 is allowed. */
int  ygz_hip_stereo_create_map_points(ygz_hip_ctx *ctx, int n_problems, const ygz_smap_problem *problems, const double K4[4],
                                      const ygz_smap_params *params, int32_t *code, int32_t *method, double *pos_world, int32_t *counts);
/* Keyframe insertion (Tracking::StereoInitialization / CreateNewKeyFrame): the features with depth > 0 are ranked by (depth, index)
 * ascending; c of them have depth <= th_depth; the ranks 0 .. min(n_depth - 1, max(c, min_close)) are walked (ORB-SLAM2's loop breaks behind
 * the first walked feature that is both beyond th_depth and past the min_close-th); selected = walked and has_point == 0.  rank [n]: the rank
 * of a walked feature, selected or not, -1 for every other; selected [n]; pos_world [n][3] = R^T (z xn - t) of a selected feature, zero
 * otherwise; n_depth, n_close (= c), n_selected may be NULL.  One upload, one launch (rank, selection and un-projection), one copy back and
 * one wait.  YGZ_E_INVALID for a null T, K4 or (n > 0) array or output, n < 0, the parameter rules above, a non-finite K4, pose, pixel or
 * depth; then for a null context; YGZ_E_CAPACITY for n above ygz_hip_max_keypoints.  n = 0 is allowed (no launch). */
int  ygz_hip_stereo_keyframe_points(ygz_hip_ctx *ctx, const double T[7], int n, const double *px, const double *depth, const uint8_t *has_point,
                                    const double K4[4], const ygz_smap_params *params, int32_t *rank, uint8_t *selected, double *pos_world,
                                    int *n_depth, int *n_close, int *n_selected);

/* ---- local-map fusion search -- nothing in the reference; the search of ORB-SLAM2's ORBmatcher::Fuse(pKF, vpMapPoints, th) as
 * LocalMapping::SearchInNeighbors calls it: many target keyframes look at the SAME points, and a keypoint is accepted only when the projection
 * lies within chi2 of it, the right column included on a stereo keypoint.  The arithmetic is that of tests/lfuse_ref.c (DESIGN.md section
 * 25); every output is bit-identical to it.
 *
 * A point set: pw [n_pt][3], pt_desc [n_pt][32], pt_dmax [n_pt], pt_normal [n_pt][3] (NULL: no viewing-angle test).  A problem is one target
 * keyframe: pose T = qx qy qz qw tx ty tz, world -> camera; keypoints kp_px [n_kp][2] (level-0 pixels), kp_level, kp_desc [n_kp][32], kp_ur
 * [n_kp] (< 0: a mono keypoint; NULL: all mono), kp_taken [n_kp] (optional); `set`, the point set it reads, and pt_skip [n_pt of that set]
 * (optional).  Per (problem, point), the first failing step sets the reason (0 searched, 1 skip, 2 behind, 3 outside, 4 range, 5 angle):
 *   steps 1-6 of ygz_hip_search_by_projection with s = 1 (bit-equal to it): skip flag, z > 0, u, v inside [0, w) x [0, h), the distance inside
 *   [0.8 dmin, 1.2 dmax], the viewing angle, the predicted level; ur = u - bf / z with bf = fx baseline;
 *   the window: keypoints that are not taken, of level pred-1 .. pred, with |kx - u| < r and |ky - v| < r, r = th 2^pred;
 *   the gate: e2 = (u - kx)^2 + (v - ky)^2; a mono keypoint is rejected when e2 > chi2_mono 4^level, a stereo keypoint when
 *   e2 + (ur - kp_ur)^2 > chi2_stereo 4^level; n_gated counts the keypoints of the window that the gate rejected;
 *   the match: the smallest (Hamming distance, keypoint index) of the survivors when its distance is <= th_dist, else match = dist = -1. */
#define YGZ_LFUSE_MAX_PROBLEMS 64
#define YGZ_LFUSE_MAX_SETS     8
#define YGZ_LFUSE_MAX_PAIRS    1048576    /* per call: the sum over the problems of their set's n_pt */
typedef struct {
    double  th;                           /* 3.0: the window is th 2^pred pixels; > 0 */
    double  baseline;                     /* 0.1: metres between the rig's cameras, > 0 */
    double  chi2_mono, chi2_stereo;       /* 5.99, 7.8: ORB-SLAM2's constants in this function (not 5.991 and 7.815); > 0 */
    int32_t th_dist;                      /* 50: the largest Hamming distance of a match, 0 .. 256 */
    int32_t pad;
} ygz_lfuse_params;
typedef struct {
    const double  *pw;
    const uint8_t *pt_desc;
    const double  *pt_dmax;
    const double  *pt_normal;
    int            n_pt;
} ygz_lfuse_points;
typedef struct {
    double         T[7];
    const double  *kp_px;
    const int32_t *kp_level;
    const uint8_t *kp_desc;
    const double  *kp_ur;
    const uint8_t *kp_taken;
    const uint8_t *pt_skip;
    int            n_kp;
    int            set;
} ygz_lfuse_problem;
void ygz_hip_default_lfuse_params(ygz_lfuse_params *p);
/* all problems in one launch, every point set uploaded once.  The outputs are concatenated in problem order, a problem contributing n_pt
 * entries of its set: match, dist, pred_level, reason, n_gated [N]; counts [n_problems][2] = matches, points searched (reason 0).  Every
 * output may be NULL.  params NULL: defaults.  One packed upload, one launch, one copy back and one wait.  Checked in this order, all before
 * the device is touched: YGZ_E_INVALID for null sets, problems or K4, n_sets < 1 or n_problems < 1; YGZ_E_CAPACITY above
 * YGZ_LFUSE_MAX_SETS or YGZ_LFUSE_MAX_PROBLEMS; YGZ_E_INVALID for a set's n_pt < 0 or a null pw, pt_desc or pt_dmax of a set with points, for
 * a problem's set index out of range, n_kp < 1 or a null kp_px, kp_level or kp_desc; YGZ_E_CAPACITY for n_kp above 2^20 or more than
 * YGZ_LFUSE_MAX_PAIRS pairs; YGZ_E_INVALID for th <= 0 or not finite, th_dist outside [0, 256], baseline <= 0, a chi2 <= 0 (or one of them
 * not finite), a non-finite K4, a focal length <= 0, a non-finite pose, point, dmax or kp_ur; last, YGZ_E_INVALID for a null context,
 * YGZ_E_CAPACITY for n_kp above ygz_hip_max_keypoints and YGZ_E_INVALID for a keypoint level outside the context's pyramid.  A set with n_pt
 * = 0 is allowed: a problem that reads it contributes nothing. */
int  ygz_hip_local_fuse_search(ygz_hip_ctx *ctx, int n_sets, const ygz_lfuse_points *sets, int n_problems, const ygz_lfuse_problem *problems,
                               const double K4[4], const ygz_lfuse_params *params, int32_t *match, int32_t *dist, int32_t *pred_level,
                               int32_t *reason, int32_t *n_gated, int32_t *counts);

/* ---- stereo tracking search -- nothing in the reference; ORB-SLAM2's two tracking searches on one kernel: ORBmatcher::SearchByProjection(
 * CurrentFrame, LastFrame, th, bMono) (mode 0, FRAME) and SearchByProjection(F, vpMapPoints, th) (mode 1, LOCAL), each with the right-column
 * test, the claim and (LOCAL) the ratio test, (FRAME) the rotation histogram.  The arithmetic is that of tests/strack_ref.c (DESIGN.md
 * section 26); every output is bit-identical to it.
 *
 * A point set: pw [n_pt][3], pt_desc [n_pt][32]; for FRAME problems pt_level [n_pt] (the level of the last frame's feature) and pt_angle
 * [n_pt] (degrees; NULL: no orientation check for the problems that read the set); for LOCAL problems pt_dmax [n_pt] and pt_normal [n_pt][3].
 * A problem is one current frame: pose T = qx qy qz qw tx ty tz, world -> camera; th; mode; direction (-1, 0, +1; FRAME); keypoints kp_px
 * [n_kp][2] (level-0 pixels), kp_level, kp_desc [n_kp][32], kp_ur [n_kp] (< 0: a mono keypoint; NULL: all mono), kp_angle [n_kp] (needed
 * when the set has pt_angle and the mode is FRAME), kp_taken [n_kp] (optional); `set`, and pt_skip [n_pt of that set] (optional).
 * Per (problem, point), on the device; the first failing step sets the reason (0 searched, 1 skip, 2 behind, 3 outside, 4 range, 5 angle):
 *   the skip flag; z > 0; u, v inside [0, w) x [0, h); ur = u - bf / z with bf = fx baseline;
 *   FRAME: lvl = pt_level, r = th 2^lvl, levels [lvl-1, lvl+1] (direction 0), [lvl, L-1] (+1), [0, lvl] (-1);
 *   LOCAL: the distance range and the viewing angle of ygz_hip_search_by_projection, its predicted level; r = th f 2^pred with f = r_near
 *   when Xc.(R n) > cos_near |Xc|, else r_wide; levels [pred-1, pred];
 *   candidates: keypoints not taken, of a level in the range, |kx - u| < r, |ky - v| < r; a stereo keypoint with |ur - kp_ur| > r is rejected
 *   (n_gated); n_cand counts the survivors; the list is the survivors sorted by (Hamming distance, index), the first YGZ_STRACK_TOPK.
 * Then on the host, inside the call, per problem and points in index order: e1, e2 the first two entries of the list no earlier point
 * took; outcome 1 without e1, 2 when dist(e1) > th_dist, 3 (LOCAL) when e2 has e1's level and dist(e1) > ratio dist(e2), else 0: match =
 * e1, claimed.  outcome -1: reason != 0.  FRAME with angles and check_orientation: the 30-bin histogram of pt_angle - kp_angle[match], its
 * three maxima; a match of another bin loses match and dist (outcome 4) and keeps its keypoint claimed.
 * sizeof: ygz_strack_params 48, ygz_strack_points 56, ygz_strack_problem 136. */
#define YGZ_STRACK_MAX_PROBLEMS 64
#define YGZ_STRACK_MAX_SETS     8
#define YGZ_STRACK_MAX_PAIRS    262144     /* per call: the sum over the problems of their set's n_pt */
#define YGZ_STRACK_TOPK         8
typedef struct {
    double  baseline;                     /* 0.1: metres between the rig's cameras, > 0 */
    double  ratio;                        /* 0.8: LOCAL's best / second-best rule, > 0 */
    double  r_near, r_wide;               /* 2.5, 4.0: LOCAL's radius factors, > 0 */
    double  cos_near;                     /* 0.998: the viewing cosine above which r_near applies */
    int32_t th_dist;                      /* 100: the largest Hamming distance of a match, 0 .. 256 */
    int32_t check_orientation;            /* 1: FRAME's rotation histogram */
} ygz_strack_params;
typedef struct {
    const double  *pw;
    const uint8_t *pt_desc;
    const int32_t *pt_level;
    const double  *pt_angle;
    const double  *pt_dmax;
    const double  *pt_normal;
    int            n_pt;
} ygz_strack_points;
typedef struct {
    double         T[7];
    double         th;                    /* the window is th 2^level (FRAME) or th f 2^pred (LOCAL) pixels; > 0 */
    const double  *kp_px;
    const int32_t *kp_level;
    const uint8_t *kp_desc;
    const double  *kp_ur;
    const double  *kp_angle;
    const uint8_t *kp_taken;
    const uint8_t *pt_skip;
    int            n_kp;
    int            set;
    int            mode;                  /* 0 FRAME, 1 LOCAL */
    int            direction;             /* FRAME: +1 forward (same or coarser levels), -1 backward, 0 neither */
} ygz_strack_problem;
void ygz_hip_default_strack_params(ygz_strack_params *p);
/* all problems in one launch, every point set uploaded once.  The outputs are concatenated in problem order, a problem contributing n_pt
 * entries of its set: match, dist, level, reason, outcome, n_cand, n_gated [N]; proj [N][3] = u, v, ur; cand [N][YGZ_STRACK_TOPK] the list
 * before the claim as keypoint indices, -1 padded; counts [n_problems][4] = matches, points searched, overflowed (n_cand above
 * YGZ_STRACK_TOPK), removed by the orientation check; rot [n_problems][33] the histogram and the three maxima (-1: none).  Every output may
 * be NULL.  params NULL: defaults.  One packed upload, one launch, one copy back and one wait.  Checked in this order, all before the device
 * is touched: YGZ_E_INVALID for null sets, problems or K4, n_sets < 1 or n_problems < 1; YGZ_E_CAPACITY above YGZ_STRACK_MAX_SETS or
 * YGZ_STRACK_MAX_PROBLEMS; YGZ_E_INVALID for a set's n_pt < 0 or a null pw or pt_desc of a set with points, for a problem's set index out of
 * range, n_kp < 1, a null kp_px, kp_level or kp_desc, a mode or direction out of range, th <= 0 or not finite, a FRAME problem whose set has
 * points and no pt_level or has pt_angle while the problem has no kp_angle, a LOCAL problem whose set has points and no pt_dmax or pt_normal;
 * YGZ_E_CAPACITY for n_kp above 2^20 or more than YGZ_STRACK_MAX_PAIRS pairs; YGZ_E_INVALID for th_dist outside [0, 256], baseline, ratio,
 * r_near or r_wide <= 0 or a parameter not finite, a non-finite K4, a focal length <= 0, a non-finite pose, point, dmax, normal, angle or
 * kp_ur; last, YGZ_E_INVALID for a null context, YGZ_E_CAPACITY for n_kp above ygz_hip_max_keypoints and YGZ_E_INVALID for a kp_level or
 * (FRAME) pt_level outside the context's pyramid.  A call whose every problem reads an empty set launches nothing. */
int  ygz_hip_stereo_track_search(ygz_hip_ctx *ctx, int n_sets, const ygz_strack_points *sets, int n_problems, const ygz_strack_problem *problems,
                                 const double K4[4], const ygz_strack_params *params, int32_t *match, int32_t *dist, int32_t *level,
                                 int32_t *reason, int32_t *outcome, int32_t *n_cand, int32_t *n_gated, double *proj, int32_t *cand,
                                 int32_t *counts, int32_t *rot);

/* ---- stereo odometry on resident slots -- nothing in the reference; ORB-SLAM2's TrackWithMotionModel on the last frame's own depths (the
 * visual-odometry points of UpdateLastFrame), for any number of (last, current) slot pairs in one call.  The result is the composition of two
 * frozen specifications, tests/strack_ref.c and tests/popt_ref.c, joined by three formulas (tests/svo_ref.py restates it),
 * and every output is bit-identical to that composition.  Per pair p, L = last_slot[p], C = cur_slot[p], K = the context's float intrinsics as
 * doubles, bf = fx baseline, T_init[p] = qx qy qz qw tx ty tz the guess of the pose that takes last-camera to current-camera coordinates:
 *   points: all of L's keypoints in keypoint order; point i has a depth z when kp_has_mp[i] != 0 and kp_depth[i] > 0 (a NaN does not count);
 *   without one it is skipped, with one pw = (((u - cx) / fx) z, ((v - cy) / fy) z, z); its level, angle and descriptor are the keypoint's;
 *   problem: C's keypoints, kp_ur[j] = u_j - bf / depth_j with a depth, else -1 (negative: a mono keypoint), mode FRAME, nothing taken,
 *   direction[p], pose T_init[p], window params.th;
 *   search, claim walk and orientation rule of ygz_hip_stereo_track_search; with fewer than min_matches matches all of it again from scratch
 *   with th doubled (retried = 1), and the second pass's outputs are the pair's; still fewer: status = 1;
 *   status 0: the matched points in point order are the edges (pw_i; kx_j, ky_j, kp_ur[j]; kp_level[j]; kind 2 when kp_ur[j] >= 0, else 1) of
 *   ygz_hip_optimize_pose_stereo from the entry pose T_init[p] with params.pose (its baseline is the call's); status 1: no edge, so the pair is
 *   FAILED in round 0 and keeps its pose.  T_rel[p] is the pose returned; current = T_rel last.
 * Every pair works in its last camera's frame, so pairs are independent and a slot may be the current frame of one and the last of another.
 * The keypoints and depths are read where ygz_hip_detect / ygz_hip_describe_given_angle and ygz_hip_set_keypoint_depths /
 * ygz_hip_stereo_depths_slots (write_depths) left them; the host reads no count before the launches.  One packed upload, the launches
 * (k_svo_gather, k_strack_search, k_svo_resolve, both again for the retry, k_pose_opt, k_svo_scatter), one copy back, one wait.
 * sizeof: ygz_svo_params 88. */
#define YGZ_SVO_MAX_PAIRS 1024
typedef struct {
    double  baseline;                     /* 0.1: metres between the rig's cameras, > 0 */
    double  th;                           /* 7.0: the window is th 2^level pixels, > 0; doubled for the retry */
    int32_t th_dist;                      /* 100: the largest Hamming distance of a match, 0 .. 256 */
    int32_t check_orientation;            /* 1: the rotation histogram */
    int32_t min_matches;                  /* 20: fewer matches retry, then fail; >= 0 */
    int32_t pad;
    ygz_pose_opt_params pose;             /* ygz_hip_default_pose_opt_params; its baseline is ignored: the call's is used */
} ygz_svo_params;
void ygz_hip_default_svo_params(ygz_svo_params *p);
/* T_init [n_pairs][7] (NULL: identity), direction [n_pairs] in {-1, 0, 1} (NULL: derived per pair on the host from T_init and the baseline:
 * +1 when the current camera is more than a baseline in front of the last one, -1 behind, else 0), params NULL: defaults.  Outputs, with cells =
 * ygz_hip_max_keypoints, any of them may be NULL except T_rel: T_rel [n][7]; status [n] (0 tracked, 1 too few matches); counts [n][8] = last
 * keypoints, points with a depth, current keypoints, matches, points searched, overflowed, removed by orientation, retried; match, dist,
 * level, reason, outcome, n_cand, n_gated [n][cells] indexed by L's keypoint (-1 past its last keypoint), proj [n][cells][3] (0 past it),
 * rot [n][33], as ygz_hip_stereo_track_search defines them; outlier [n][cells] (0 where there is no edge) and chi2 [n][cells] (-1.0 there) of
 * the pose optimiser in point order; inliers, rounds_run [n] and round_status, round_iterations, round_cost_initial, round_cost_final,
 * round_lambda [n][8].  Checked in this order, all before the device is touched: YGZ_E_INVALID for a null last_slot, cur_slot or T_rel or
 * n_pairs < 1; YGZ_E_CAPACITY above YGZ_SVO_MAX_PAIRS; YGZ_E_INVALID for a non-finite parameter, baseline <= 0, th <= 0, th_dist outside
 * [0, 256], min_matches < 0, the rules of ygz_hip_optimize_pose_stereo for params.pose (a chi2 <= 0, rounds outside 1 .. 8, iterations or
 * max_trials outside 1 .. 64), a non-finite T_init, a direction outside {-1, 0, 1}, a negative slot, last == cur in a pair; last,
 * YGZ_E_INVALID for a null context or a slot past the context's frames, YGZ_E_CAPACITY for a context of more than 32768 cells, YGZ_E_STATE for
 * a slot without keypoints (no pyramid was ever built for it) or a context whose keypoint depths were never written. */
int  ygz_hip_stereo_odometry_slots(ygz_hip_ctx *ctx, int n_pairs, const int32_t *last_slot, const int32_t *cur_slot, const double *T_init,
                                   const int32_t *direction, const ygz_svo_params *params, double *T_rel, int32_t *status, int32_t *counts,
                                   int32_t *match, int32_t *dist, int32_t *level, int32_t *reason, int32_t *outcome, int32_t *n_cand,
                                   int32_t *n_gated, double *proj, int32_t *rot, uint8_t *outlier, double *chi2, int32_t *inliers,
                                   int32_t *rounds_run, int32_t *round_status, int32_t *round_iterations, double *round_cost_initial,
                                   double *round_cost_final, double *round_lambda);

/* ---- stereo local-map tracking on resident slots -- nothing in the reference; ORB-SLAM2's TrackLocalMap (SearchByProjection(F, vpMapPoints,
 * th) and the pose optimisation on the frame's associations) for any number of resident frames in one call.  The result is the composition of
 * two frozen specifications, tests/strack_ref.c in mode LOCAL and tests/popt_ref.c, joined by four formulas (DESIGN.md section 28;
 * tests/slm_ref.py restates it), and every output is bit-identical to that composition.  The point sets (pw, pt_desc, pt_dmax, pt_normal of
 * ygz_strack_points; pt_level and pt_angle are not read) are shared between frames and go up once.  Per frame f, K = the context's float
 * intrinsics as doubles, bf = fx baseline formed once, T[f] = qx qy qz qw tx ty tz the entry pose from world to camera:
 *   keypoints: those of slot[f]; kp_ur[j] = u_j - bf / depth_j when kp_has_mp[j] != 0 and kp_depth[j] > 0 (a NaN does not count), else -1
 *   (negative: a mono keypoint);
 *   prior: prior[f][j] = i >= 0 says keypoint j already holds point i of set[f] (what a motion-model stage left on the frame), -1 free, a NULL
 *   array all free; kp_taken[j] = (prior[j] >= 0), pt_skip[i] = 1 for every i the prior names; two keypoints may name one point;
 *   search and claim walk of ygz_hip_stereo_track_search in mode LOCAL with th, r_near, r_wide, cos_near, ratio, th_dist and the entry pose;
 *   no rotation histogram, no retry;
 *   edges in KEYPOINT order: keypoint j with i = prior[j] >= 0, or else the point that claimed j, gives pw_i; kx_j, ky_j, kp_ur[j];
 *   kp_level[j]; kind 2 when kp_ur[j] >= 0, else 1 -- the order in which ygz::PoseOptimizer builds its edges from a frame's features;
 *   pose: with fewer than min_edges edges status = 1, the optimiser is given no edge, so the frame is FAILED in round 0 and T_out[f] is T[f]
 *   bitwise; otherwise ygz_hip_optimize_pose_stereo from T[f] with params.pose (its baseline is the call's).
 * The same slot may appear in several frame entries (two hypotheses of one frame); a set of 0 points is allowed: nothing is searched and the
 * frame's edges are its prior.  The host reads no count before the launches.  One packed upload, five launches (k_slm_gather,
 * k_strack_search, k_slm_resolve, k_pose_opt, k_slm_scatter), one copy back, one wait.
 * sizeof: ygz_slm_params 112. */
#define YGZ_SLM_MAX_FRAMES 1024
#define YGZ_SLM_MAX_SETS   64
#define YGZ_SLM_MAX_PAIRS  4194304        /* per call: the sum over the frames of their set's n_pt */
typedef struct {
    double  baseline;                     /* 0.1: metres between the rig's cameras, > 0 */
    double  th;                           /* 1.0: the window is th f 2^pred pixels, > 0 */
    double  ratio;                        /* 0.8: the best / second-best rule, > 0 */
    double  r_near, r_wide;               /* 2.5, 4.0: the radius factors, > 0 */
    double  cos_near;                     /* 0.998: the viewing cosine above which r_near applies */
    int32_t th_dist;                      /* 100: the largest Hamming distance of a match, 0 .. 256 */
    int32_t min_edges;                    /* 3: a frame with fewer edges is not optimised (status 1); >= 0 */
    ygz_pose_opt_params pose;             /* ygz_hip_default_pose_opt_params; its baseline is ignored: the call's is used */
} ygz_slm_params;
void ygz_hip_default_slm_params(ygz_slm_params *p);
/* slot, set [n_frames]; T [n_frames][7]; prior [n_frames][cells] with cells = ygz_hip_max_keypoints, or NULL; params NULL: defaults.
 * Outputs, any of them may be NULL except T_out: T_out [n][7]; status [n] (0 optimised, 1 too few edges); counts [n][8] = keypoints,
 * keypoints with a right column, prior edges, points, points searched, overflowed, new matches, edges; kp_point [n][cells] the point each
 * keypoint ends with (-1 without one and past the last keypoint); outlier [n][cells] (0 where there is no edge) and chi2 [n][cells] (-1.0
 * there) of the pose optimiser in keypoint order; inliers, rounds_run [n] and round_status, round_iterations, round_cost_initial,
 * round_cost_final, round_lambda [n][8]; match, dist, level, reason, outcome, n_cand, n_gated [N] and proj [N][3] as
 * ygz_hip_stereo_track_search defines them, concatenated in frame order, frame f contributing the n_pt entries of its set.  Checked in this
 * order, all before the device is touched: YGZ_E_INVALID for a null sets, slot, set, T or T_out, n_frames < 1 or n_sets < 1; YGZ_E_CAPACITY
 * above YGZ_SLM_MAX_FRAMES or YGZ_SLM_MAX_SETS; YGZ_E_INVALID for a non-finite parameter, baseline, th, ratio, r_near or r_wide <= 0, th_dist
 * outside [0, 256], min_edges < 0, the rules of ygz_hip_optimize_pose_stereo for params.pose, a set's n_pt < 0 or a null pw, pt_desc, pt_dmax
 * or pt_normal of a set with points, a negative slot, a set index out of range; YGZ_E_CAPACITY for more than YGZ_SLM_MAX_PAIRS pairs;
 * YGZ_E_INVALID for a non-finite T, point, dmax or normal; last, YGZ_E_INVALID for a null context or a slot past the context's frames,
 * YGZ_E_CAPACITY for a context of more than 32768 cells, YGZ_E_INVALID for a prior entry below -1 or not below its set's n_pt, YGZ_E_STATE
 * for a slot without keypoints (no pyramid was ever built for it) or a context whose keypoint depths were never written. */
int  ygz_hip_stereo_local_map_slots(ygz_hip_ctx *ctx, int n_sets, const ygz_strack_points *sets, int n_frames, const int32_t *slot,
                                    const int32_t *set, const double *T, const int32_t *prior, const ygz_slm_params *params, double *T_out,
                                    int32_t *status, int32_t *counts, int32_t *kp_point, uint8_t *outlier, double *chi2, int32_t *inliers,
                                    int32_t *rounds_run, int32_t *round_status, int32_t *round_iterations, double *round_cost_initial,
                                    double *round_cost_final, double *round_lambda, int32_t *match, int32_t *dist, int32_t *level,
                                    int32_t *reason, int32_t *outcome, int32_t *n_cand, int32_t *n_gated, double *proj);

/* ---- stereo reference-keyframe tracking on resident slots -- nothing in the reference; ORB-SLAM2's TrackReferenceKeyFrame (SearchByBoW between
 * the reference keyframe and the frame, then the pose optimisation on the associations) for any number of resident frames in one call.  The
 * result is the composition of frozen specifications, yo_search_by_bow and yo_bow_orientation of oracle/bow.c and tests/popt_ref.c, joined by
 * the formulas below (tests/srk_ref.py restates it), and every output is bit-identical to that composition.  Only n_pt
 * and pw of a point set are read, so the same set objects serve ygz_hip_stereo_local_map_slots afterwards; the sets are shared and go up once.
 * Keyframe k is slot kf_slot[k] with set kf_set[k]; kf_point[k][i] = p >= 0 says keypoint i of that slot carries point p of the set, -1 none;
 * two keypoints may name one point.  Frame f is slot[f], tracked against keyframe kf[f] from the entry pose T[f] (world to camera, qx qy qz qw
 * tx ty tz; ORB-SLAM2 uses the last frame's pose); several frames may name one keyframe and a slot may appear in several frame entries.
 *   1 BoW: ygz_hip_compute_bow with params.levelsup for every distinct slot the call names, frames and keyframes, once each -- the call needs no
 *     earlier ygz_hip_compute_bow and overwrites what one left;
 *   2 right columns: kp_ur[j] = u_j - bf / depth_j when kp_has_mp[j] != 0 and kp_depth[j] > 0 (a NaN does not count), else -1;
 *   3 search: yo_search_by_bow with the keyframe's keypoints as frame 1, node1[i] replaced by -1 where kf_point[i] < 0, the frame's keypoints
 *     as frame 2: best < th_low and (float)best < knn_ratio (float)second;
 *   4 claim: a frame keypoint j named by several keyframe features goes to the smallest i; the others get match -1, outcome 2;
 *   5 orientation (check_orientation != 0) over the claimed matches: the histogram and the three maxima of yo_bow_orientation (bin =
 *     round(rot / 30), the reference's factor) on the slots' float angles; a claimed match in another bin gets match -1, outcome 4, and j ends
 *     without a point;
 *   6 edges in keypoint order of the frame, j ascending: pw of kf_point[i] for the i that holds j; kx_j, ky_j, kp_ur[j]; kp_level[j]; kind 2
 *     when kp_ur[j] >= 0, else 1;
 *   7 pose: with fewer than min_matches edges status = 1, the optimiser is given no edge and T_out[f] is T[f] bitwise; otherwise
 *     ygz_hip_optimize_pose_stereo from T[f] with params.pose (its baseline is the call's); status = 2 when the inliers are fewer than
 *     min_inliers (the pose is still returned).
 * The host reads no count before the launches.  One packed upload, seven launches (k_srk_gather, k_bow_transform, k_srk_gather for the masked
 * node rows, k_bow_match<0>, k_srk_resolve, k_pose_opt, k_srk_scatter), one copy back, one wait.
 * sizeof: ygz_srk_params 88. */
#define YGZ_SRK_MAX_FRAMES    1024
#define YGZ_SRK_MAX_KEYFRAMES 256
#define YGZ_SRK_MAX_SETS      64
typedef struct {
    double  baseline;                     /* 0.1: metres between the rig's cameras, > 0 */
    int32_t th_low;                       /* 50: a match's Hamming distance is below it, 0 .. 256 */
    float   knn_ratio;                    /* 0.7: best against second best of the same node, > 0 */
    int32_t levelsup;                     /* 4: the FeatureVector's node is this many levels above the leaves, >= 0 */
    int32_t check_orientation;            /* 1: the rotation histogram removes matches */
    int32_t min_matches;                  /* 15: a frame with fewer edges is not optimised (status 1); >= 0 */
    int32_t min_inliers;                  /* 10: fewer inliers after the optimisation: status 2; >= 0 */
    ygz_pose_opt_params pose;             /* ygz_hip_default_pose_opt_params; its baseline is ignored: the call's is used */
} ygz_srk_params;
void ygz_hip_default_srk_params(ygz_srk_params *p);
/* sets [n_sets]; kf_slot, kf_set [n_keyframes]; kf_point [n_keyframes][cells] with cells = ygz_hip_max_keypoints; slot, kf [n_frames];
 * T [n_frames][7]; params NULL: defaults.  Outputs, any of them may be NULL except T_out: T_out [n][7]; status [n] (0 optimised, 1 too few
 * edges, 2 too few inliers); counts [n][8] = keyframe keypoints, those with a point, frame keypoints, those with a right column, search
 * matches, lost to the claim, removed by orientation, edges; kp_point [n][cells] the set index behind every frame keypoint after step 5 (-1
 * without one and past the last keypoint); prior [n][cells] = kp_point with the optimiser's outliers set to -1, in the layout and index space
 * ygz_hip_stereo_local_map_slots takes; outlier [n][cells] (0 where there is no edge) and chi2 [n][cells] (-1.0 there) in keypoint order;
 * inliers, rounds_run [n] and round_status, round_iterations, round_cost_initial, round_cost_final, round_lambda [n][8]; by keyframe keypoint,
 * match12 [n][cells] (the frame keypoint or -1) and outcome [n][cells] (0 matched, 1 no match, 2 lost the claim, 4 orientation, -1 no point
 * or past the last keypoint); rot [n][33] the histogram and its three maxima (zeros and -1 without the check).  Checked in this order, all
 * before the device is touched: YGZ_E_INVALID for a null sets, kf_slot, kf_set, kf_point, slot, kf, T or T_out, n_sets, n_keyframes or
 * n_frames < 1; YGZ_E_CAPACITY above YGZ_SRK_MAX_SETS, YGZ_SRK_MAX_KEYFRAMES or YGZ_SRK_MAX_FRAMES; YGZ_E_INVALID for a non-finite baseline
 * or knn_ratio, baseline <= 0, th_low outside [0, 256], knn_ratio <= 0, levelsup < 0, min_matches or min_inliers < 0, the rules of
 * ygz_hip_optimize_pose_stereo for params.pose; a set's n_pt < 0 or a null pw of a set with points, a negative slot, a set or keyframe index
 * out of range; a non-finite T or pw; last, YGZ_E_INVALID for a null context or a slot past the context's frames, YGZ_E_CAPACITY for a context
 * of more than 32768 cells, YGZ_E_INVALID for a kf_point entry below -1 or not below its set's n_pt, YGZ_E_STATE for a context without a
 * vocabulary, a slot without keypoints (no pyramid was ever built for it) or a context whose keypoint depths were never written. */
int  ygz_hip_stereo_ref_keyframe_slots(ygz_hip_ctx *ctx, int n_sets, const ygz_strack_points *sets, int n_keyframes, const int32_t *kf_slot,
                                       const int32_t *kf_set, const int32_t *kf_point, int n_frames, const int32_t *slot, const int32_t *kf,
                                       const double *T, const ygz_srk_params *params, double *T_out, int32_t *status, int32_t *counts,
                                       int32_t *kp_point, int32_t *prior, uint8_t *outlier, double *chi2, int32_t *inliers, int32_t *rounds_run,
                                       int32_t *round_status, int32_t *round_iterations, double *round_cost_initial, double *round_cost_final,
                                       double *round_lambda, int32_t *match12, int32_t *outcome, int32_t *rot);

/* ---- stereo relocalisation on resident slots -- nothing in the reference; ORB-SLAM2's Tracking::Relocalization up to and including its first
 * PoseOptimization, for any number of lost resident frames in one call, each with an ordered list of candidate keyframes.  The result is the
 * composition of frozen specifications -- yo_search_by_bow and yo_bow_orientation of oracle/bow.c, pr_ransac of tests/pnp_ref.c and
 * tests/popt_ref.c -- joined by the formulas below (tests/srl_ref.py restates it), and every output is bit-identical to
 * that composition.  Sets and keyframes are those of ygz_hip_stereo_ref_keyframe_slots.  Frame f is slot[f]; it has no entry pose.  Its
 * candidates are the keyframes cand_kf[q], cand_off[f] <= q < cand_off[f + 1], in the caller's order (best first); problem q is (frame f,
 * keyframe cand_kf[q]) and P = cand_off[n_frames] is the number of problems.  A keyframe may be the candidate of several frames, and of one
 * frame twice; a slot may appear in several frame entries; a frame may have no candidate.  Per problem:
 *   1 steps 1 to 6 of ygz_hip_stereo_ref_keyframe_slots with this call's th_low, knn_ratio, levelsup and check_orientation: the
 *     associations in keypoint order of the frame, j ascending: pw of the point, (kx_j, ky_j), kp_ur[j], kp_level[j]; n is their number;
 *   2 n < min_matches: status 1, no PnP and no optimisation; T_pnp and T_opt are 0 0 0 1 0 0 0, the ygz_pnp_result is that of a problem
 *     none of whose hypotheses has an inlier, with n_hypotheses = 0, and pnp_inlier, prior, outlier and chi2 are empty;
 *   3 PnP: ygz_hip_pnp_ransac's result (pr_ransac of tests/pnp_ref.c) on (pw, (kx, ky)) of the n associations in that order with
 *     params.pnp and the context's camera; the sample sets are ygz_hip_pnp_sample_sets(n, max_iter), formed on the device from n.  T_pnp is
 *     its T_cw.  success == 0: status 2, T_opt = T_pnp and no optimisation;
 *   4 pose: the edges are the PnP inliers in keypoint order, kind 2 where kp_ur[j] >= 0, else 1; ygz_hip_optimize_pose_stereo from T_pnp
 *     with params.pose (its baseline is the call's); T_opt is its pose; status 3 when its inliers are fewer than min_final_inliers (the pose
 *     is still returned), else 0;
 *   5 best[f] is the first q of frame f with status 0, or -1; T_out[f] is that problem's T_opt, or 0 0 0 1 0 0 0.
 * The host reads no count before the copy back.  One packed upload, thirteen launches (k_srl_gather, k_bow_transform, k_srl_gather for the
 * masked node rows, k_bow_match<0>, k_srl_resolve, k_srl_sets, k_pnp_solve, k_pnp_score, k_pnp_select, k_srl_edges, k_pose_opt,
 * k_srl_scatter, k_srl_pick), one copy back, one wait.
 * sizeof: ygz_srl_params 120. */
#define YGZ_SRL_MAX_FRAMES    256
#define YGZ_SRL_MAX_PROBLEMS  256
#define YGZ_SRL_MAX_KEYFRAMES 256
#define YGZ_SRL_MAX_SETS      64
#define YGZ_SRL_MAX_HYPOTHESIS_SETS 76800 /* bound of P * max_iter (256 problems of 300 iterations): 384 B of hypotheses each, 28 MiB */
typedef struct {
    double  baseline;                     /* 0.1: metres between the rig's cameras, > 0 */
    int32_t th_low;                       /* 50: a match's Hamming distance is below it, 0 .. 256 */
    float   knn_ratio;                    /* 0.75: best against second best of the same node, > 0 */
    int32_t levelsup;                     /* 4: the FeatureVector's node is this many levels above the leaves, >= 0 */
    int32_t check_orientation;            /* 1: the rotation histogram removes matches */
    int32_t min_matches;                  /* 15: a problem with fewer associations gets no PnP (status 1); >= 4, what a PnP problem needs */
    int32_t pad0;
    ygz_pnp_params pnp;                   /* ygz_hip_default_pnp_params: 300 iterations, chi2 5.991, 10 inliers for success */
    int32_t min_final_inliers;            /* 50: fewer inliers after the optimisation: status 3; >= 0 */
    int32_t pad1;
    ygz_pose_opt_params pose;             /* ygz_hip_default_pose_opt_params; its baseline is ignored: the call's is used */
} ygz_srl_params;
void ygz_hip_default_srl_params(ygz_srl_params *p);
/* sets [n_sets]; kf_slot, kf_set [n_keyframes]; kf_point [n_keyframes][cells] with cells = ygz_hip_max_keypoints; slot [n_frames]; cand_off
 * [n_frames + 1]; cand_kf [P]; params NULL: defaults.  Outputs, any of them may be NULL except T_out and best: T_out [n_frames][7]; best
 * [n_frames]; per problem status [P] (0 relocalised, 1 too few associations, 2 PnP without success, 3 too few inliers after the
 * optimisation), T_pnp, T_opt [P][7], pnp [P], counts [P][10] = the eight of ygz_hip_stereo_ref_keyframe_slots (the last is n), the PnP
 * inliers, the optimiser's inliers; inliers, rounds_run [P] and round_status, round_iterations, round_cost_initial, round_cost_final,
 * round_lambda [P][8] (those of an optimisation without edges for status 1 and 2); rot [P][33]; by frame keypoint, [P][cells]: kp_point (the
 * set index after step 1, -1 without one and past the last keypoint), pnp_inlier (1 where the keypoint's association is an inlier of the PnP
 * winner, also for status 2), prior = kp_point of the PnP inliers that are no outliers of the optimiser, -1 elsewhere, in the layout and index
 * space ygz_hip_stereo_local_map_slots takes, outlier (0 where there is no edge) and chi2 (-1.0 there); by keyframe keypoint, [P][cells]:
 * match12 and outcome as in ygz_hip_stereo_ref_keyframe_slots; sets_out [P][max_iter][3] the sample sets the device formed (zeros for
 * status 1).  Checked in this order, all before the device is touched: YGZ_E_INVALID for a null sets, kf_slot, kf_set, kf_point, slot,
 * cand_off, cand_kf, T_out or best, n_sets, n_keyframes or n_frames < 1; YGZ_E_CAPACITY above YGZ_SRL_MAX_SETS, YGZ_SRL_MAX_KEYFRAMES or
 * YGZ_SRL_MAX_FRAMES; YGZ_E_INVALID for cand_off[0] != 0, a decreasing cand_off or P < 1; YGZ_E_CAPACITY for P above YGZ_SRL_MAX_PROBLEMS;
 * YGZ_E_INVALID for a non-finite baseline, knn_ratio or pnp.chi2, baseline <= 0, th_low outside [0, 256], knn_ratio <= 0, levelsup < 0,
 * min_matches < 4, min_final_inliers < 0, pnp.max_iter outside [1, YGZ_PNP_MAX_ITER], pnp.chi2 <= 0, pnp.min_inliers < 0, the rules of
 * ygz_hip_optimize_pose_stereo for params.pose; YGZ_E_CAPACITY for P * pnp.max_iter above YGZ_SRL_MAX_HYPOTHESIS_SETS; YGZ_E_INVALID for a
 * set's n_pt < 0 or a null pw of a set with points, a negative slot, a set or keyframe index out of range; a non-finite pw; last,
 * YGZ_E_INVALID for a null context or a slot past the context's frames, YGZ_E_CAPACITY for a context of more than 32768 cells or P * cells
 * past 2^31 - 1, YGZ_E_INVALID for a kf_point entry below -1 or not below its set's n_pt, YGZ_E_STATE for a context without a vocabulary, a
 * slot without keypoints (no pyramid was ever built for it) or a context whose keypoint depths were never written. */
int  ygz_hip_stereo_relocalize_slots(ygz_hip_ctx *ctx, int n_sets, const ygz_strack_points *sets, int n_keyframes, const int32_t *kf_slot,
                                     const int32_t *kf_set, const int32_t *kf_point, int n_frames, const int32_t *slot, const int32_t *cand_off,
                                     const int32_t *cand_kf, const ygz_srl_params *params, double *T_out, int32_t *best, int32_t *status,
                                     double *T_pnp, double *T_opt, ygz_pnp_result *pnp, int32_t *counts, int32_t *inliers, int32_t *rounds_run,
                                     int32_t *round_status, int32_t *round_iterations, double *round_cost_initial, double *round_cost_final,
                                     double *round_lambda, int32_t *rot, int32_t *kp_point, uint8_t *pnp_inlier, int32_t *prior,
                                     uint8_t *outlier, double *chi2, int32_t *match12, int32_t *outcome, int32_t *sets_out);

/* ---- local-map selection -- nothing in the reference; ORB-SLAM2's Tracking::UpdateLocalKeyFrames in the form of
 * StereoTracker::LocalKeyFrames (no spanning tree: the data model has none) and Tracking::UpdateLocalPoints, for any number of frames on one
 * map in one call (tests/lms_ref.c is the frozen specification, and every output is an integer and bit-identical to it).
 * The map goes up once per call: kf_bad [n_keyframes]; cov [n_keyframes][n_cov], a keyframe's covisible keyframes, best first, in
 * [-1, n_keyframes), where a -1 is looked at and skipped (it ends nothing); the points in ygz_hip_covisibility's point-major CSR, offsets
 * [n_points + 1] and kf [n_obs] strictly ascending within a point, with feat [n_obs] the index of the observing feature in its keyframe, in
 * [0, YGZ_LMS_MAX_FEATURES); pt_bad [n_points] or NULL for "none bad".  The frames: fr_off [n_frames + 1]; fr_pt [fr_off[n_frames]] in
 * [-1, n_points), the points on a frame in feature order, -1 for no point; a point may stand on a frame twice.  Per frame f:
 *   1 votes[f][k] is the number of entries e of f with p = fr_pt[e] >= 0, pt_bad[p] == 0 and k in p's list (a point that stands twice votes
 *     twice: the host rule counts per feature);
 *   2 ref[f] is the smallest k with the largest vote > 0, bad keyframes included; -1 without a vote;
 *   3 the list: the voters with kf_bad == 0 in ascending k (n_voters[f] of them, never capped); then for voter i = 0 .. n_voters - 1 in order,
 *     while the list is shorter than max_keyframes (tested before each voter), the first c of cov[voter_i][0 .. n_cov) with c >= 0,
 *     kf_bad[c] == 0 and c not yet in the list is appended, at most one per voter.  n_local[f] is the length, local_kf[f][n_keyframes] the
 *     list, padded with -1; rank_f(k) is k's position in it;
 *   4 the point set: the points with pt_bad == 0 that have an observer in the list, ascending by the key (smallest rank_f over the point's
 *     observers, feat of that observation, p): on a map whose observations mirror the keyframes' features that is "keyframes in the given
 *     order, features by index, each point once", what ygz_hip_stereo_local_map_slots' callers build.  The first max_points are kept:
 *     local_pt[f][max_points] (padded with -1), n_pt[f] their number, n_cut[f] the number of the rest;
 *   5 fr_prior[e] is the position of fr_pt[e] in f's kept list, or -1 (no point, a bad point, no observer in the list, a cut point): a
 *     frame's slice is the `prior` row ygz_hip_stereo_local_map_slots takes once laid out at `cells`.
 * The entry point builds the keyframe-major index ((feature, point) pairs per keyframe, two counting passes) beside the upload.  One packed
 * upload, four launches (k_lms_vote, k_lms_points, k_lms_place, k_lms_prior), one copy back, one wait; the host decides nothing in between.
 * sizeof: ygz_lms_params 8. */
#define YGZ_LMS_MAX_KEYFRAMES 4096        /* n_keyframes and max_keyframes (= YGZ_MAP_MAX_KEYFRAMES) */
#define YGZ_LMS_MAX_COV       32          /* n_cov */
#define YGZ_LMS_MAX_FRAMES    1024        /* n_frames (= YGZ_SLM_MAX_FRAMES) */
#define YGZ_LMS_MAX_FEATURES  32768       /* entries of one frame; feat is below it */
typedef struct {
    int32_t max_keyframes;                /* 80: the extension stops at this length (the voters alone may exceed it), in [1, YGZ_LMS_MAX_KEYFRAMES] */
    int32_t max_points;                   /* 16384: points kept per frame, >= 1; n_frames * max_points <= YGZ_SLM_MAX_PAIRS */
} ygz_lms_params;
void ygz_hip_default_lms_params(ygz_lms_params *p);
/* params NULL: defaults.  Outputs, any of them may be NULL except n_local and local_kf: votes [n_frames][n_keyframes]; ref, n_voters, n_local
 * [n_frames]; local_kf [n_frames][n_keyframes]; n_pt, n_cut [n_frames]; local_pt [n_frames][max_points]; fr_prior [fr_off[n_frames]].  Checked
 * in this order, all before the device is touched: YGZ_E_INVALID for a null kf_bad, offsets, kf, feat, fr_off, fr_pt, n_local or local_kf, a
 * null cov with n_cov > 0, n_keyframes, n_points or n_frames < 1, n_cov < 0; YGZ_E_CAPACITY for n_keyframes above YGZ_LMS_MAX_KEYFRAMES,
 * n_cov above YGZ_LMS_MAX_COV or n_frames above YGZ_LMS_MAX_FRAMES; YGZ_E_INVALID for max_keyframes outside [1, YGZ_LMS_MAX_KEYFRAMES] or
 * max_points < 1; YGZ_E_CAPACITY for n_frames * max_points above YGZ_SLM_MAX_PAIRS or n_frames * n_keyframes above YGZ_COVIS_MAX_CELLS;
 * YGZ_E_INVALID for offsets[0] or fr_off[0] != 0 or a decreasing offset; YGZ_E_CAPACITY for a point with more than
 * YGZ_MAP_MAX_OBS_PER_POINT observations, more than YGZ_MAP_MAX_OBS in the call or a frame of more than YGZ_LMS_MAX_FEATURES entries;
 * YGZ_E_INVALID for a keyframe index out of range, a list that is not strictly ascending, a feat out of range, a cov entry outside
 * [-1, n_keyframes) or an fr_pt entry outside [-1, n_points); last, for a null context.  A refused call writes nothing. */
int  ygz_hip_local_map_select(ygz_hip_ctx *ctx, int n_keyframes, const uint8_t *kf_bad, int n_cov, const int32_t *cov, int n_points,
                              const int32_t *offsets, const int32_t *kf, const int32_t *feat, const uint8_t *pt_bad, int n_frames,
                              const int32_t *fr_off, const int32_t *fr_pt, const ygz_lms_params *params, int32_t *votes, int32_t *ref,
                              int32_t *n_voters, int32_t *n_local, int32_t *local_kf, int32_t *n_pt, int32_t *n_cut, int32_t *local_pt,
                              int32_t *fr_prior);

/* ---- map-point attributes -- nothing in the reference; ORB-SLAM2's MapPoint::UpdateNormalAndDepth as ygz::Matcher::PointAttributes states it,
 * for every point of a map in one call (tests/mpa_ref.c is the frozen specification, and every double is bit-identical
 * to it).  The map is a point-major CSR: point p owns the rows offsets[p] .. offsets[p + 1] - 1 in the caller's order, row e names the
 * observing keyframe obs_kf[e] (it need not ascend and may repeat) and the level obs_level[e] of the observation; kf_center
 * [n_keyframes][3] the camera centres, pw [n_points][3].  Per row r = pw_p - kf_center[obs_kf[e]], q = r0 r0, then q + r1 r1, then q + r2 r2,
 * d = sqrt(q), sum_k += r_k / d, every operation one IEEE double operation in this order, the sum sequential in row order;
 * normal = sum / (double)rows, dmax = d of the point's first row * 2^max(obs_level of that row, 0).  state [n_points]: 0 for a point without
 * a row, 2 when some d is 0 or an output is not finite, otherwise 1; with state 0 or 2 dmax and normal are zeros (no NaN leaves the call).
 * One packed upload, one launch (k_mpa_attr), one copy back, one wait. */
#define YGZ_MPA_MAX_POINTS 1048576        /* n_points */
/* Checked in this order, all before the device is touched: YGZ_E_INVALID for a null array, n_keyframes or n_points < 1; YGZ_E_CAPACITY for
 * n_keyframes above YGZ_MAP_MAX_KEYFRAMES or n_points above YGZ_MPA_MAX_POINTS; YGZ_E_INVALID for offsets[0] != 0 or a decreasing offset;
 * YGZ_E_CAPACITY for a point with more than YGZ_MAP_MAX_OBS_PER_POINT rows or more than YGZ_MAP_MAX_OBS rows in the call; YGZ_E_INVALID for
 * an obs_kf outside [0, n_keyframes), an obs_level above 30 or a centre or point that is not finite; last, for a null context.  A refused
 * call writes nothing. */
int  ygz_hip_map_point_attributes(ygz_hip_ctx *ctx, int n_keyframes, const double *kf_center, int n_points, const double *pw,
                                  const int32_t *offsets, const int32_t *obs_kf, const int32_t *obs_level, double *dmax, double *normal,
                                  int32_t *state);

/* ---- stereo local-map tracking on an indexed map -- ygz_hip_stereo_local_map_slots with the point sets given as index lists into ONE map
 * (DESIGN.md section 35).  The map: pw [n_points][3], pt_desc [n_points][32], pt_dmax [n_points], pt_normal [n_points][3], what
 * ygz_hip_map_point_attributes writes; it goes up once.  The lists: list_pt [n_lists][list_stride] and list_len [n_lists] are local_pt and
 * n_pt of ygz_hip_local_map_select, so its output goes in as it is; the entries past list_len[l] are not read; an index may stand in several
 * lists and twice in one.  Frame f has the keypoints of slot[f] and the points of list[f]; prior[f][j] is a position in that list.  On the
 * device k_slm_index (a lane per list entry) gathers every list into a packed point set, and the five launches of
 * ygz_hip_stereo_local_map_slots run on those sets unchanged: for every accepted input every output is bit-identical to that call on the sets
 * gathered by the lists on the host, and to tests/slm_ref.py on them.  YGZ_SLM_MAX_SETS does not apply.  One packed upload, six launches, one
 * copy back, one wait; the host decides nothing in between.
 * The outputs are those of ygz_hip_stereo_local_map_slots, frame f contributing list_len[list[f]] entries to the per-point ones.  Checked in
 * this order, all before the device is touched: YGZ_E_INVALID for a null list_pt, list_len, slot, list, T or T_out, n_frames < 1, n_lists < 1
 * or n_points < 0; YGZ_E_CAPACITY for n_frames or n_lists above YGZ_SLM_MAX_FRAMES or n_points above YGZ_MPA_MAX_POINTS; YGZ_E_INVALID for the
 * parameters as in ygz_hip_stereo_local_map_slots, a null pw, pt_desc, pt_dmax or pt_normal with n_points > 0, list_stride < 1, a list_len
 * outside [0, list_stride], a negative slot, a list index out of range, an entry below list_len outside [0, n_points); YGZ_E_CAPACITY for
 * more than YGZ_SLM_MAX_PAIRS pairs (the sum over the frames of their list's length); YGZ_E_INVALID for a non-finite T, or a non-finite
 * point, dmax or normal anywhere in the map; last, the context's checks of ygz_hip_stereo_local_map_slots in its order.  A refused call
 * writes nothing. */
int  ygz_hip_stereo_local_map_indexed(ygz_hip_ctx *ctx, int n_points, const double *pw, const uint8_t *pt_desc, const double *pt_dmax,
                                      const double *pt_normal, int n_lists, int list_stride, const int32_t *list_pt, const int32_t *list_len,
                                      int n_frames, const int32_t *slot, const int32_t *list, const double *T, const int32_t *prior,
                                      const ygz_slm_params *params, double *T_out, int32_t *status, int32_t *counts, int32_t *kp_point,
                                      uint8_t *outlier, double *chi2, int32_t *inliers, int32_t *rounds_run, int32_t *round_status,
                                      int32_t *round_iterations, double *round_cost_initial, double *round_cost_final, double *round_lambda,
                                      int32_t *match, int32_t *dist, int32_t *level, int32_t *reason, int32_t *outcome, int32_t *n_cand,
                                      int32_t *n_gated, double *proj);

/* ---- the resident map -- the map of the three calls above with a home in device memory, and local-map tracking on it in ONE call
 * (DESIGN.md section 36).  A ygz_hip_map belongs to the context it was created with and owns its device buffers (its own allocations, grown
 * by the rule of the context's scratch buffers; the context's table of scratch buffers is not used).  Several maps may live in one context;
 * ygz_hip_destroy frees the ones still alive.  Every call below refuses a null map or a map of another context with YGZ_E_INVALID, behind
 * its own argument checks and the null context, and before the device is touched.
 * ygz_map_arrays carries exactly what the three calls take, in their layouts: the selection side (n_keyframes, kf_bad, n_cov, cov, n_points,
 * offsets, kf, feat, pt_bad or NULL) as ygz_hip_local_map_select; the attribute side (n_centres, centre [n_centres][3], a_offsets
 * [n_points + 1], a_kf, a_level: the point-major CSR of ygz_hip_map_point_attributes with rows in the caller's order); the tracking side (pw
 * [n_points][3], pt_desc [n_points][32], pt_has_desc [n_points] or NULL for "every point has one").
 * sizeof: ygz_map_arrays 120, ygz_map_info 40. */
typedef struct ygz_hip_map ygz_hip_map;
typedef struct {
    int32_t n_keyframes, n_cov, n_points, n_centres;
    const uint8_t *kf_bad; const int32_t *cov; const int32_t *offsets, *kf, *feat; const uint8_t *pt_bad;
    const double *centre; const int32_t *a_offsets, *a_kf, *a_level;
    const double *pw; const uint8_t *pt_desc, *pt_has_desc;
} ygz_map_arrays;
typedef struct {
    int32_t n_keyframes, n_cov, n_points, n_obs, n_centres, n_rows;   /* of the resident map; zeros before the first upload */
    int32_t uploads, updates;                                         /* accepted ones since ygz_hip_map_create */
    uint64_t resident_bytes;                                          /* device memory the map holds, its call buffers included */
} ygz_map_info;
int  ygz_hip_map_create(ygz_hip_ctx *ctx, ygz_hip_map **map);         /* YGZ_E_INVALID for a null map or context */
int  ygz_hip_map_destroy(ygz_hip_ctx *ctx, ygz_hip_map *map);         /* waits for the stream, then frees */
int  ygz_hip_map_info(ygz_hip_ctx *ctx, ygz_hip_map *map, ygz_map_info *info);
/* Makes the whole map resident: the arrays go up, the keyframe-major index of the selection is built beside the upload and stays on the
 * device, and k_mpa_attr computes the attributes there.  dmax [n_points], normal [n_points][3] and state [n_points] come back when they are
 * not NULL, bit-identical to ygz_hip_map_point_attributes on the same arrays.  A later upload may be larger or smaller.  One upload, one
 * launch, one copy back, one wait.  Checked in this order, all before the device is touched: the map-side checks of
 * ygz_hip_local_map_select in its order (null kf_bad, offsets, kf or feat, null cov with n_cov > 0, n_keyframes or n_points < 1, n_cov < 0;
 * the capacities; the offsets; the observations; the cov entries), then those of ygz_hip_map_point_attributes in its order with n_centres
 * for n_keyframes (dmax, normal and state may be null), then YGZ_E_INVALID for a null pt_desc; last the null context and the map.  A refused
 * upload leaves the resident map as it was, and usable. */
int  ygz_hip_map_upload(ygz_hip_ctx *ctx, ygz_hip_map *map, const ygz_map_arrays *m, double *dmax, double *normal, int32_t *state);
/* The delta after a bundle adjustment or a culling; it changes no observation (a new keyframe or a new or erased observation is a new
 * upload).  n_pt point rows: pt_idx [n_pt] and, each NULL for "keep", pw [n_pt][3], pt_desc [n_pt][32], pt_bad [n_pt], pt_has_desc [n_pt];
 * n_kf keyframe rows kf_idx, kf_bad; n_c centre rows c_idx, centre [n_c][3].  k_rmap_scatter (a lane per row) writes them, then k_mpa_attr
 * recomputes the attributes of the whole map: afterwards the resident state is bit-identical to a fresh upload of the updated arrays.  One
 * upload, two launches, one wait.  Checked in this order, all before the device is touched: the null context and the map; YGZ_E_STATE for a
 * map without an upload; YGZ_E_INVALID for a negative count, a null index array with a count above 0, an index out of range or twice within
 * one array, a null kf_bad with n_kf > 0 or a null centre with n_c > 0, a pw or centre that is not finite.  A refused update writes
 * nothing. */
int  ygz_hip_map_update(ygz_hip_ctx *ctx, ygz_hip_map *map, int n_pt, const int32_t *pt_idx, const double *pw, const uint8_t *pt_desc,
                        const uint8_t *pt_bad, const uint8_t *pt_has_desc, int n_kf, const int32_t *kf_idx, const uint8_t *kf_bad, int n_c,
                        const int32_t *c_idx, const double *centre);
/* A test aid: the arrays as the device holds them, any of them may be NULL: pw, pt_desc, pt_bad, pt_has_desc, kf_bad [n_keyframes], centre
 * [n_centres][3], dmax, normal, state.  YGZ_E_STATE for a map without an upload. */
int  ygz_hip_map_download(ygz_hip_ctx *ctx, ygz_hip_map *map, double *pw, uint8_t *pt_desc, uint8_t *pt_bad, uint8_t *pt_has_desc,
                          uint8_t *kf_bad, double *centre, double *dmax, double *normal, int32_t *state);
/* Local-map selection and tracking of n_frames resident frames on the resident map.  Only the frames' entries (fr_off, fr_pt as
 * ygz_hip_local_map_select takes them), their slots and their poses go up.  For every accepted input every output is bit-identical to:
 *   1 ygz_hip_local_map_select on the map's selection arrays and the frames' entries (the cut at max_points happens here: a cut point is not
 *     re-admitted when a refused one leaves);
 *   2 point p is refused when state[p] != 1 (the resident attributes) or pt_has_desc[p] == 0;
 *   3 the refused entries leave every frame's list, the order of the rest is kept; moved[i] is an entry's new position or -1; n_removed[f]
 *     counts them; local_pt is padded with -1;
 *   4 prior[f][j] = moved[fr_prior[fr_off[f] + j]] when j is below the frame's number of entries and that fr_prior is >= 0, otherwise -1,
 *     for j up to the context's cells;
 *   5 ygz_hip_stereo_local_map_indexed on the resident map with list[f] = f, the filtered lists and that prior.
 * Outputs, any may be NULL except T_out: votes, ref, n_voters, n_local, local_kf, n_cut as the selection writes them; n_pt [n_frames] and
 * local_pt [n_frames][max_points] AFTER the filter; n_removed [n_frames]; prior [n_frames][cells]; then the outputs of
 * ygz_hip_stereo_local_map_indexed, the per-point ones laid out [n_frames][max_points] (proj [n_frames][max_points][3]): the first n_pt[f]
 * entries of row f are written, the rest are left untouched.  Two uploads (the tracking block, the frames' entries), eleven launches
 * (k_lms_vote, k_lms_points, k_lms_place, k_lms_prior, k_rmap_filter, k_slm_index and the five of ygz_hip_stereo_local_map_slots; k_lms_prior
 * is left out when no frame has an entry), two copies back, one wait; the host decides nothing in between and the map is not sent.
 * Checked in this order, all before the device is touched: YGZ_E_INVALID for a null slot, T, fr_off, fr_pt or T_out or n_frames < 1;
 * YGZ_E_CAPACITY for n_frames above YGZ_LMS_MAX_FRAMES; YGZ_E_INVALID for max_keyframes outside [1, YGZ_LMS_MAX_KEYFRAMES] or max_points < 1;
 * YGZ_E_CAPACITY for n_frames * max_points above YGZ_SLM_MAX_PAIRS; YGZ_E_INVALID for fr_off[0] != 0 or a decreasing offset; YGZ_E_CAPACITY for
 * a frame of more than YGZ_LMS_MAX_FEATURES entries; YGZ_E_INVALID for a null context or the map; YGZ_E_STATE for a map without an upload;
 * YGZ_E_CAPACITY for n_frames * n_keyframes above YGZ_COVIS_MAX_CELLS; YGZ_E_INVALID for an fr_pt entry outside [-1, n_points) or a frame
 * with more entries than cells; then the parameter, pose and context checks of ygz_hip_stereo_local_map_indexed in its order.  A refused
 * call writes nothing. */
int  ygz_hip_stereo_local_map_resident(ygz_hip_ctx *ctx, ygz_hip_map *map, int n_frames, const int32_t *slot, const double *T,
                                       const int32_t *fr_off, const int32_t *fr_pt, const ygz_lms_params *lms, const ygz_slm_params *params,
                                       int32_t *votes, int32_t *ref, int32_t *n_voters, int32_t *n_local, int32_t *local_kf, int32_t *n_cut,
                                       int32_t *n_pt, int32_t *local_pt, int32_t *n_removed, int32_t *prior, double *T_out, int32_t *status,
                                       int32_t *counts, int32_t *kp_point, uint8_t *outlier, double *chi2, int32_t *inliers,
                                       int32_t *rounds_run, int32_t *round_status, int32_t *round_iterations, double *round_cost_initial,
                                       double *round_cost_final, double *round_lambda, int32_t *match, int32_t *dist, int32_t *level,
                                       int32_t *reason, int32_t *outcome, int32_t *n_cand, int32_t *n_gated, double *proj);

#ifdef __cplusplus
}
#endif
#endif /* YGZ_HIP_H_ */
