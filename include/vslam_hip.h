/*
 * vslam_hip.h — C ABI of the MI355X (gfx950) implementation of gtsam-vSLAM's
 * per-frame tracking + local bundle-adjustment hot path.
 *
 * The reference has no FFI: its boundary is the set of C++ member functions
 * System.cpp and the two pipelines call.  Every entry point
 * below names the reference interface it replaces (file:line under the
 * reference root).  Plain pointers and sizes only; the caller owns every
 * buffer; every function returns a vslam_status and never throws.
 *
 * All compute runs in hand-written HIP kernels; there is no CPU fallback — if
 * no gfx950 device is usable the create functions return VSLAM_ERR_NO_DEVICE.
 */
#ifndef VSLAM_HIP_H
#define VSLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vslam_status {
    VSLAM_OK = 0,
    VSLAM_ERR_INVALID = 1,    /* bad argument / shape mismatch */
    VSLAM_ERR_NO_DEVICE = 2,  /* no usable HIP device (product path never falls back to CPU) */
    VSLAM_ERR_HIP = 3,        /* a HIP runtime call failed; see vslam_last_error() */
    VSLAM_ERR_CAPACITY = 4,   /* caller buffer / internal capacity too small */
    VSLAM_ERR_COMM = 5        /* RCCL failure */
} vslam_status;

const char* vslam_last_error(void);
/* number of visible HIP devices (0 if none); never initialises a context */
int vslam_device_count(void);

/* cv::KeyPoint, field for field (28 bytes) — reference include/FeatureExtractor.h:20 */
typedef struct vslam_keypoint {
    float x, y;
    float size;
    float angle;
    float response;
    int32_t octave;
    int32_t class_id;
} vslam_keypoint;

/* FeatureExtractor constructor arguments — reference include/FeatureExtractor.h:80,
 * src/FeatureExtractor.cpp:620 */
typedef struct vslam_fe_params {
    int32_t n_features;
    int32_t n_levels;
    float scale;
    int32_t edge_threshold;
    int32_t patch_size;
    int32_t max_fast_threshold;
    int32_t min_fast_threshold;
} vslam_fe_params;

/* ---------------------------------------------------------------------------
 * FeatureExtractor — replaces FeatureExtractor::FeatureExtractor and
 * FeatureExtractor::extractKeysNew (include/FeatureExtractor.h:80,87;
 * src/FeatureExtractor.cpp:481-533).  One object extracts `batch` same-sized
 * images per call (batch = 2 runs the left and the right image of a stereo
 * frame in the same launches, as the reference's two threads do,
 * src/FeatureTracker.cpp:58-61).  Not re-entrant, like the reference object.
 * ------------------------------------------------------------------------- */
typedef struct vslam_extractor vslam_extractor;

vslam_status vslam_extractor_create(const vslam_fe_params* params, int32_t width, int32_t height,
                                    int32_t batch, int32_t device, vslam_extractor** out);
void vslam_extractor_destroy(vslam_extractor* ex);

/* public tables of the reference object (scalePyramid, scaleInvPyramid, sigmaFactor,
 * InvSigmaFactor, scaledPatchSize, featurePerLevel — include/FeatureExtractor.h:71-77);
 * each out array holds n_levels entries, NULL pointers are skipped */
vslam_status vslam_extractor_tables(const vslam_extractor* ex, float* scale_pyramid,
                                    float* scale_inv_pyramid, float* sigma_factor,
                                    float* inv_sigma_factor, int32_t* scaled_patch_size,
                                    int32_t* feature_per_level);

/* extractKeysNew on host images: gray[i] is image i (u8, `stride` bytes per row).
 * kps: batch x cap keypoints, desc: batch x cap x 32 bytes, n_out: batch counts. */
vslam_status vslam_extract(vslam_extractor* ex, const uint8_t* const* gray, int32_t stride,
                           vslam_keypoint* kps, uint8_t* desc, int32_t cap, int32_t* n_out);

/* Split form used when inputs are already device-resident (bench, pipelines):
 *   set_image_device: copy a device image (u8, stride bytes per row) into pyramid level 0
 *   run:              enqueue + complete extraction, results stay in HBM
 *   fetch:            copy keypoints / descriptors of image i to host buffers */
vslam_status vslam_extractor_set_image_device(vslam_extractor* ex, int32_t image_index,
                                              const void* d_gray, int32_t stride);
vslam_status vslam_extractor_set_image_host(vslam_extractor* ex, int32_t image_index,
                                            const uint8_t* gray, int32_t stride);
/* Colour frames, as the reference's TrackImage receives them from cv::imread(IMREAD_COLOR) (src/VIOSlam.cpp:289-311) and
 * converts first (cvtColor BGR2GRAY / BGRA2GRAY, src/FeatureTracker.cpp:1130-1144): image `image_index` from interleaved
 * BGR (channels = 3) or BGRA (4, alpha ignored) bytes, `stride` bytes per row (at least width x channels), converted to
 * gray on the device while pyramid level 0 is written (gray = (1868 B + 9617 G + 4899 R + 8192) >> 14).  channels = 1 is
 * set_image_device / set_image_host.  Host sources are staged in a device buffer the extractor allocates on its first
 * colour host image; returns once the caller may reuse `src`.  Anything but channels 1 / 3 / 4 or a short stride:
 * VSLAM_ERR_INVALID before any work is queued. */
vslam_status vslam_extractor_set_image_color(vslam_extractor* ex, int32_t image_index, const void* src, int32_t stride,
                                             int32_t channels, int32_t on_device);
/* RAW (unrectified) frames, as the reference's frame loop has them before cv::remap (src/VIOSlam.cpp:278-311): image
 * `image_index` from a gray (channels = 1), BGR (3) or BGRA (4) source of the rectifier's SOURCE size, `stride` bytes per row
 * (at least src_width x channels), remapped through `rectifier`'s maps - and converted to gray, each channel rounded first,
 * as vslam_rectifier_remap_gray does - while pyramid level 0 is written: one launch, no rectified image in between, the
 * bytes of vslam_rectifier_remap(_gray) followed by set_image.  Ordering and synchronisation as set_image_color: the host
 * form returns once `src` may be reused, the other images keep their level 0.  The rectifier is borrowed for the call; its
 * output size must be the extractor's width x height and its device the extractor's.  VSLAM_ERR_INVALID (nothing queued)
 * for anything else, channels other than 1 / 3 / 4 or a short stride. */
typedef struct vslam_rectifier vslam_rectifier;
vslam_status vslam_extractor_set_image_raw(vslam_extractor* ex, int32_t image_index, const vslam_rectifier* rectifier, const void* src,
                                           int32_t stride, int32_t channels, int32_t on_device);
vslam_status vslam_extractor_run(vslam_extractor* ex);
vslam_status vslam_extractor_count(const vslam_extractor* ex, int32_t image_index, int32_t* n_out);
vslam_status vslam_extractor_fetch(vslam_extractor* ex, int32_t image_index, vslam_keypoint* kps,
                                   uint8_t* desc, int32_t cap, int32_t* n_out);

/* test / debug taps: pyramid level (blurred = 0|1) copied to a w*h host buffer,
 * and the pre-SSC FAST candidates of one level */
vslam_status vslam_extractor_level_size(const vslam_extractor* ex, int32_t level, int32_t* w, int32_t* h);
vslam_status vslam_extractor_level_copy(vslam_extractor* ex, int32_t image_index, int32_t level,
                                        int32_t blurred, uint8_t* out);
vslam_status vslam_extractor_candidates(vslam_extractor* ex, int32_t image_index, int32_t level,
                                        vslam_keypoint* out, int32_t cap, int32_t* n_out);

/* test tap: FeatureExtractor::ssc (src/FeatureExtractor.cpp:368-468) of pyramid level `level` on caller-supplied
 * candidates (x, y integer-valued < 4096, response 0..255; tol 0.1, numRetPoints = featurePerLevel[level], the level's
 * cols / rows) - the same kernel a frame runs, fed directly.  Invalidates the extractor's last frame. */
vslam_status vslam_extractor_ssc_level(vslam_extractor* ex, int32_t level, const vslam_keypoint* cand, int32_t n,
                                       vslam_keypoint* out, int32_t cap, int32_t* n_out);

/* test tap: orientation + descriptor (k_orient_desc alone, the kernel a frame runs) of caller-supplied keypoints of
 * pyramid level `level` of image `image_index`, on the pyramid and the blurred pyramid that the last
 * vslam_extractor_run() built.  kps[k].x / .y: integer-valued LEVEL coordinates with 19 <= x <= w_level - 20 and
 * 19 <= y <= h_level - 20 (the extractor's own guarantee; the kernel reads the patch unchecked), .response integer-valued
 * 0..255; the other fields are ignored.  Writes n keypoints (angle, size, octave, x / y scaled to level 0 as a frame's)
 * and n x 32 descriptor bytes.  VSLAM_ERR_INVALID before the first run and for a keypoint outside these ranges (nothing
 * is launched, vslam_last_error() names the keypoint), VSLAM_ERR_CAPACITY for more keypoints than an image can keep or
 * than `cap`.  Invalidates the extractor's last frame. */
vslam_status vslam_extractor_describe(vslam_extractor* ex, int32_t image_index, int32_t level, const vslam_keypoint* kps,
                                      int32_t n, vslam_keypoint* out_kps, uint8_t* out_desc, int32_t cap, int32_t* n_out);

/* per-kernel device time of the last run, in milliseconds (HIP events on the
 * extractor's stream).  names/ms hold up to cap entries; n_out = entries written. */
vslam_status vslam_extractor_timings(const vslam_extractor* ex, const char** names, float* ms,
                                     int32_t cap, int32_t* n_out);
/* per-kernel HIP-event timing on (default) / off for this extractor's following runs; off removes the
 * two event records per launch from the launch-bound path */
vslam_status vslam_extractor_set_timing(vslam_extractor* ex, int32_t on);
/* SSC placement: the suppression (FeatureExtractor::ssc, src/FeatureExtractor.cpp:368-468) runs in the k_ssc kernels
 * only - on_device is always 1 and host_fallbacks always 0 (kept for callers of the earlier interface).  A level with
 * more than 65 535 FAST candidates makes the run fail with VSLAM_ERR_CAPACITY.  VSLAM_SSC_FORCE_GLOBAL=1 (tests) sends
 * every level through the HBM-resident instantiation that levels above 16 384 candidates use. */
vslam_status vslam_extractor_ssc_stats(vslam_extractor* ex, int32_t* on_device, int32_t* host_fallbacks);


/* ---------------------------------------------------------------------------
 * FeatureMatcher — replaces FeatureMatcher::FeatureMatcher and its matching
 * members (include/FeatureMatcher.h:40-63).  Like the reference object it holds
 * the two extractors (feLeft / feRight) and reads their pyramids in place
 * (src/FeatureMatcher.cpp:606,623) — here device-resident, no copies.
 * ------------------------------------------------------------------------- */
/* the scalars of Camera / StereoCamera that enter the path (include/Camera.h:71,83-84) */
typedef struct vslam_rig {
    double fx, fy, cx, cy;
    float baseline;
    int32_t width, height;
} vslam_rig;

typedef struct vslam_matcher vslam_matcher;

/* left_image / right_image: index of the left / right image inside the extractors'
 * batches (one batch-2 extractor may serve as both feLeft and feRight). */
vslam_status vslam_matcher_create(const vslam_rig* rig, vslam_extractor* fe_left, int32_t left_image,
                                  vslam_extractor* fe_right, int32_t right_image, vslam_matcher** out);
void vslam_matcher_destroy(vslam_matcher* m);

/* By default the matcher uses the keypoints / descriptors of the extractors' last run where
 * they lie in HBM.  set_keys overrides one side (right = 0|1) with host arrays (tests, replays);
 * use_extractor_keys switches back. */
vslam_status vslam_matcher_set_keys(vslam_matcher* m, int32_t right, const vslam_keypoint* kps,
                                    const uint8_t* desc, int32_t n);
vslam_status vslam_matcher_use_extractor_keys(vslam_matcher* m);
/* Re-bind the matcher to another extractor pair of the same geometry (frame-level pipelining: extractor
 * pair B works on frame n+1 on its own stream while the matcher / tracker consumes pair A's frame n).
 * The matcher's map state is kept.  Ordering between the extractors' streams and the matcher's stream is
 * by HIP events, in both directions; matchers must be destroyed before the extractors they were bound to. */
vslam_status vslam_matcher_bind_extractors(vslam_matcher* m, vslam_extractor* fe_left, int32_t left_image,
                                           vslam_extractor* fe_right, int32_t right_image);

/* findStereoMatchesORB2R (include/FeatureMatcher.h:54, src/FeatureMatcher.cpp:528-708):
 * fills TrackedKeys::rightIdxs[nL], leftIdxs[nR], estimatedDepth[nL], close[nL] (device-resident;
 * fetch copies them out).  stats = {Hamming tests, SAD refinements, accepted before the
 * depth / SAD outlier cut} — the exact figures DESIGN.md's algorithmic-byte formula uses. */
vslam_status vslam_stereo_match(vslam_matcher* m);
vslam_status vslam_stereo_fetch(vslam_matcher* m, int32_t* right_idxs, int32_t* left_idxs,
                                float* estimated_depth, uint8_t* close_flags, int32_t cap_left,
                                int32_t cap_right, int64_t* stats3);

/* test tap: the tail of findStereoMatchesORB2R (src/FeatureMatcher.cpp:655-705 - accepted pairs entered in left
 * order, the nearest-1 % depth cut, the 2.1 x median-SAD cut) on caller-supplied per-left arrays: best[i] = accepted
 * right index or < 0, depth[i] and sad[i] of that pair - the same kernel a frame runs, fed directly.  The result is
 * read with vslam_stereo_fetch (stats all 0).  n_left above the matcher's left-key limit (7680) or more than 65535
 * keys give VSLAM_ERR_CAPACITY; best[i] >= n_right or negative sizes give VSLAM_ERR_INVALID.  Drops any set_keys
 * override: the next vslam_stereo_match reads the extractors' keys again unless set_keys is called anew. */
vslam_status vslam_stereo_finalize_arrays(vslam_matcher* m, const int32_t* best, const float* depth, const int32_t* sad,
                                          int32_t n_left, int32_t n_right);

/* matchByProjectionRPred (include/FeatureMatcher.h:57, src/FeatureMatcher.cpp:254-389).
 * vslam_mappoint_view flattens the MapPoint fields that function reads (desc, predL/predR,
 * scaleLevelL/R, inFrame/inFrameR — include/Map.h).  Map points are processed in array order
 * and claim keypoints greedily exactly like the reference loop.
 *   matched_idxs_l[nL], matched_idxs_r[nR]  in/out  claim tables (-1 = free)
 *   matches[M][2]                           in/out  (left idx, right idx) per map point
 * The call needs a completed vslam_stereo_match (it reads rightIdxs / leftIdxs). */
typedef struct vslam_mappoint_view {
    uint8_t desc[32];
    float pred_lx, pred_ly, pred_rx, pred_ry;
    int32_t scale_level_l, scale_level_r;
    uint8_t in_frame, in_frame_r;
    uint8_t pad_[2];
} vslam_mappoint_view;

vslam_status vslam_match_projection(vslam_matcher* m, const vslam_mappoint_view* mps, int32_t n_mps,
                                    float rad, int32_t* matched_idxs_l, int32_t* matched_idxs_r,
                                    int32_t* matches, int32_t* n_matches, int64_t* n_candidates);

/* FeatureMatcher::matchByProjectionMono (include/FeatureMatcher.h:57, src/FeatureMatcher.cpp:391-456): the left-only
 * variant of the mono + IMU mode (thresholds matchDistProj + 50 and ratioProj + 0.1); only matches[2i] is written.
 * Works on a stereo matcher and on a mono matcher (vslam_matcher_create with fe_right = NULL). */
vslam_status vslam_match_projection_mono(vslam_matcher* m, const vslam_mappoint_view* mps, int32_t n_mps, float rad,
                                         int32_t* matched_idxs_l, int32_t* matches, int32_t* n_matches,
                                         int64_t* n_candidates);
/* FeatureMatcher::matchByRadius (include/FeatureMatcher.h:60, src/FeatureMatcher.cpp:458-526): keypoints of the
 * last keyframe against the current frame's left keypoints inside rad * scalePyramid[octave], with the
 * Converter::checkPixelParallax gate (include/Conversions.h:25,140-144).  match_out[i] = index the reference
 * appends to keyframeIdxMatchs[i], or -1; matched_idxs_l (current keypoints) is in/out. */
vslam_status vslam_match_by_radius(vslam_matcher* m, const vslam_keypoint* last_kps, const uint8_t* last_desc,
                                   int32_t n_last, float rad, int32_t* matched_idxs_l, int32_t* match_out,
                                   int32_t* n_matches);
/* matchByRadius (src/FeatureMatcher.cpp:458-526) from one key set into n_targets key sets IN ORDER, sharing one claim table:
 * what addMappointsMono (src/FeatureTracker.cpp:1512-1519) does.  last_keys / target_keys[t]: device key blocks
 * (vslam_kf_keys_bytes(n, 0) bytes as written by vslam_kf_keys_upload, or a session's key slot), no right keys.
 * matched_idxs_l: in/out, n_matched entries, indexed by TARGET key index - a claim at index j made in one target blocks index j
 * in every later target; n_matched >= every n_target[t], else VSLAM_ERR_INVALID.  match_out[t * n_last + i] = index in target t
 * that the reference appends to keyframeIdxMatchs[i], or -1; n_matches[t] (may be NULL) = the call's return value for target t.
 * Grid and scalePyramid are the matcher's, as for vslam_match_by_radius; the matcher's current frame is neither read nor
 * changed.  Everything is enqueued on the matcher's stream: one launch builds all targets' cell buckets, one scans all
 * targets' candidates, the resolve runs per target on the shared table; the call waits once, at its end.  At most 64
 * targets. */
vslam_status vslam_match_by_radius_window(vslam_matcher* m, const void* last_keys, int32_t n_last,
                                          const void* const* target_keys, const int32_t* n_target, int32_t n_targets,
                                          float rad, int32_t* matched_idxs_l, int32_t n_matched,
                                          int32_t* match_out, int32_t* n_matches);

/* ---------------------------------------------------------------------------
 * Tracker steps — replace FeatureTracker::estimatePoseGTSAM (stereo-only branch) with
 * findOutliersR / check2dError (include/FeatureTracker.h, src/FeatureTracker.cpp:147-411,
 * 582-649) and worldToFrame + MapPoint::predictScale (src/FeatureTracker.cpp:685-741,
 * src/Map.cpp:13-23).  They act on the frame the matcher currently holds (keypoints, close,
 * rightIdxs/leftIdxs/estimatedDepth in HBM) and mutate it exactly like the reference.
 * ------------------------------------------------------------------------- */
typedef struct vslam_lm_report {
    int32_t iterations;        /* accepted outer iterations */
    int32_t inner_iterations;  /* lambda trials */
    double initial_error, final_error, lambda;
} vslam_lm_report;

typedef struct vslam_pose_problem {
    int32_t n_mps;                 /* active map points */
    const double* points_xyz;      /* n x 3 world positions (MapPoint::getWordPose3d) */
    const uint8_t* in_frame;       /* MapPoint::inFrame / inFrameR / GetIsOutlier */
    const uint8_t* in_frame_r;
    const uint8_t* mp_is_outlier;
    int32_t* matches;              /* n x 2 matchesIdxs, in/out */
    uint8_t* mps_outliers;         /* n MPsOutliers, in/out */
    double T_cw[16];               /* estimPose (camera <- world), row-major, in/out */
} vslam_pose_problem;

/* Motion-only LM (GTSAM 4.2 LevenbergMarquardt policy, 100 iterations max) in one kernel launch,
 * then the chi2 (7.815) inlier pass.  n_inliers / n_stereo = the pair estimatePoseGTSAM returns. */
vslam_status vslam_estimate_pose(vslam_matcher* m, vslam_pose_problem* prob, int32_t* n_inliers,
                                 int32_t* n_stereo, vslam_lm_report* report);

/* estimatePoseGTSAM, IMU branch (slamMode 0; src/FeatureTracker.cpp:301-406): the same vision factors plus a
 * CombinedImuFactor(x0,v0,x1,v1,b0,b1) built from the frame's IMU bucket (PreintegratedCombinedMeasurements,
 * tangent pre-integration, body_P_sensor = T_bc1), BetweenFactor<ConstantBias>(sigma 1e-3) and the two
 * unit-covariance priors on x1 / v1; x0, v0, b0 are pinned, x1 / v1 / b1 start at the IMU prediction.
 * prob->T_cw is OUTPUT only here (the optimised camera<-world pose). */
typedef struct vslam_imu_input {
    double gravity[3];                 /* Camera::mIMUGravity (src/VIOSlam.cpp:274) */
    double gyro_noise_density, gyro_random_walk, accel_noise_density, accel_random_walk;   /* IMUData */
    double T_body_sensor[16];          /* Camera::TBodyToCam (T_bc1), row-major */
    double T_wc_prev[16];              /* zedPtr->mCameraPose pose (x0) */
    double velocity_prev[3];           /* Camera::mVelocity (v0) */
    double bias_prev[6];               /* initialBias [accelerometer, gyroscope] (b0) */
    int32_t n_samples;
    int32_t hz;                        /* IMUData::mHz: dt of a single-sample bucket */
    const double* acceleration;        /* n x 3 */
    const double* angular_velocity;    /* n x 3 */
    const double* timestamps_ns;       /* n; dt_i = (t[i+1]-t[i])/1e9, the last sample reuses the previous dt (:338-353) */
} vslam_imu_input;

typedef struct vslam_imu_output {
    double velocity[3];                /* -> Camera::mNewVelocity */
    double bias[6];                    /* -> initialBias */
} vslam_imu_output;

vslam_status vslam_estimate_pose_imu(vslam_matcher* m, vslam_pose_problem* prob, const vslam_imu_input* imu,
                                     vslam_imu_output* out, int32_t* n_inliers, int32_t* n_stereo,
                                     vslam_lm_report* report);
/* FeatureTracker::estimatePoseGTSAMMono + findOutliersMono (src/FeatureTracker.cpp:413-580,651-683): the same IMU
 * solve over left GenericProjectionFactors only (in_frame_r and matches[2i+1] are ignored, may be NULL / -1). */
vslam_status vslam_estimate_pose_mono(vslam_matcher* m, vslam_pose_problem* prob, const vslam_imu_input* imu,
                                      vslam_imu_output* out, int32_t* n_inliers, vslam_lm_report* report);
/* FeatureTracker::PredictNextPoseIMU (src/FeatureTracker.cpp:1036-1106): pre-integrate the bucket and predict
 * from (imu->T_wc_prev, pred_velocity, imu->bias_prev).  dt0 = start value of the sample period: the reference
 * initialises it to mHz / mFps here (:1067) and to 1 / mHz in the pose solves (:337,510); a sample takes the
 * difference to the next timestamp, the last sample reuses the previous value, so dt0 only survives for a
 * single-sample bucket.  dt0 <= 0 selects 1 / hz. */
vslam_status vslam_imu_predict(vslam_matcher* m, const vslam_imu_input* imu, const double* pred_velocity, double dt0,
                               double* T_wc_out, double* velocity_out);
/* The IMU calls above and the tracking / system / batch calls in IMU mode return VSLAM_ERR_INVALID when the bucket's
 * 15x15 pre-integration covariance has no Cholesky factor (there would be no information matrix, so no IMU factor). */

/* test taps: the pre-integration of one bucket as a pose solve stages it (dt rule above, dt0 = 1 / hz) and runs it
 * (k_imu_preintegrate).  pim_out: 295 doubles (deltaTij, preint[9] = theta, position, velocity, H_biasAcc[27],
 * H_biasOmega[27] (9 x 3 row-major), cov[225], biasHat[6]); lam_out: the information matrix (225); pred_out: the state
 * predicted from (T_wc_prev, velocity_prev, bias_prev): R[9], t[3], v[3].  Errors as above. */
vslam_status vslam_imu_preintegrate(vslam_matcher* m, const vslam_imu_input* imu, double* pim_out, double* lam_out,
                                    double* pred_out);
/* the same for n_lanes buckets in ONE launch of the batched kernel (k_imu_preintegrate_b), outputs [n_lanes][295 | 225 |
 * 15].  A bucket with n_samples = 0 is an idle lane: its outputs are left as the caller filled them.  solve_io: NULL,
 * or [n_lanes] pointers, each NULL or the 9-double io block of a pose solve (velocity, bias): entries [3..8] become the
 * lane's integration bias on the device (the rechained pre-integration after a solve).  Invalidates the matcher's
 * staged IMU bucket. */
vslam_status vslam_imu_preintegrate_batch(vslam_matcher* m, int32_t n_lanes, const vslam_imu_input* imus,
                                          const double* const* solve_io, double* pim_out, double* lam_out, double* pred_out);

/* worldToFrame for n points and both cameras with pose T_cw: fills pred_l/pred_r (n x 2 floats),
 * scale_level_l/r, in_frame/in_frame_r.  log_scale = KeyFrame::logScale (float log(imScale)). */
vslam_status vslam_world_to_frame(vslam_matcher* m, const double* T_cw, int32_t n,
                                  const double* points_xyz, const float* max_scale_dist,
                                  float log_scale, float* pred_l, float* pred_r,
                                  int32_t* scale_level_l, int32_t* scale_level_r,
                                  uint8_t* in_frame, uint8_t* in_frame_r);

/* ---------------------------------------------------------------------------
 * Relocalisation — NO reference counterpart (the reference has nothing that recovers a lost tracker; DESIGN.md section 6
 * holds the exact rules, tests/reloc_ref.py restates them on the CPU).  Recovers the pose of the frame the matcher
 * currently holds (a completed vslam_stereo_match: keypoints, descriptors, rightIdxs, estimatedDepth in HBM) from a map,
 * without a pose prior:
 *   A  k_reloc_match_b: every map point against every left key, 256-bit Hamming.  d1 = smallest distance, i1 = lowest key
 *      index attaining it, d2 = smallest distance over all other keys (257 with a single key).  Point p proposes i1 iff
 *      d1 <= max_hamming and 100 * d1 < ratio_pct * d2; key i goes to the proposer with the smallest (d1 << 32 | p).
 *   B  k_reloc_pairs_b: winning pairs whose key has estimatedDepth > 0 and rightIdxs >= 0, in ascending key index, as
 *      correspondences {X_w, X_c (the key back-projected with its depth), kx, ky, kxr, octave, p, i}; C of them.
 *      C < 3: success = 0, status VSLAM_OK.
 *   C  k_reloc_ransac_b / k_reloc_best_b: n_hypotheses poses, each from three correspondences sampled by a counter hash of
 *      (seed, hypothesis, draw), built in fp64 from the two point triples' orthonormal frames; scored by the number of
 *      correspondences with z > 0 whose (left u, left v, right u) residual, weighted by the octave's InvSigmaFactor,
 *      passes the chi2 bound 7.815.  The winner is the largest (count << 32 | 0xFFFFFFFF - h).
 *   D  the winner's inliers, in correspondence order, refined from the hypothesis by the pose solve of vslam_estimate_pose
 *      (the problem is built on the device, k_reloc_problem_b, and solved by the batched pose kernel behind a gate: a winner
 *      without inliers or C < 3 is not refined); success = n_inliers >= min_inliers.  T_cw_out is written only on success.
 * params->mode = 1 builds the hypotheses from 2D-3D correspondences instead (no stereo depth is read before step D;
 * DESIGN.md section 6 item 22, restated by tests/reloc_p3p_ref.py).  Step A is unchanged; then
 *   B' k_reloc_pairs_p3p_b: EVERY winning pair, in ascending key index, as correspondences {X_w, y (the key's unit bearing:
 *      ((kx - cx) / fx, (ky - cy) / fy, 1) divided by its norm, fp64), kx, ky, kxr, octave, p, i, stereo}; stereo =
 *      estimatedDepth > 0 && rightIdxs >= 0, kxr is the matched right key's x with the flag and 0 without.  n_pairs = C.
 *   C' k_reloc_ransac_p3p_b / k_reloc_best_p3p_b: the sampling of step C; the three (X_w, y) pairs go through a P3P solver (fp64
 *      + - * / and sqrt in a fixed order: a degenerate conic of the pencil of the three distance equations, its real root by
 *      16 Newton steps, two quadratics, 3 Gauss-Newton steps on the depths) that fills up to four solution slots with
 *      camera <- world poses.  A slot is void for collinear world points or coincident bearings (|.|^2 < 1e-12), a
 *      non-finite value or a depth <= 0.  A correspondence counts for a slot iff z > 0 and its residual - (left u, left v,
 *      right u) with the stereo flag, (left u, left v) without, weighted by the octave's InvSigmaFactor - passes the same
 *      bound 7.815.  A hypothesis's count is the largest over its slots (the lowest slot on a tie) and its pose that slot's;
 *      the winner is chosen as in step C.
 *   D  as above; a correspondence without a right match enters with matches = (i, -1): a left-only factor.
 * Any other mode: VSLAM_ERR_INVALID, nothing launched.  The mode belongs to the call (one params set per batched call).
 * The call is the one-lane case of vslam_relocalize_batch below (same driver, same kernels): the map goes up from a pinned
 * block of the matcher's own (allocated by the first call, grown on demand), everything is enqueued on the matcher's stream,
 * and the call waits once, at its end.  Its error messages name no lane.
 * n_points <= 65536 and at most 7680 left keys, else VSLAM_ERR_CAPACITY; no completed stereo match, n_hypotheses above
 * 1024 or a negative parameter: VSLAM_ERR_INVALID.  Like vslam_estimate_pose, step D may clear the stereo match of a
 * key whose right observation fails the chi2 test.
 * ------------------------------------------------------------------------- */
typedef struct vslam_reloc_params {   /* a zero field takes the default in brackets (all zero / NULL = all defaults) */
    int32_t max_hamming;     /* [50]  accept a best distance <= this */
    int32_t ratio_pct;       /* [80]  and 100*d1 < ratio_pct*d2 */
    int32_t n_hypotheses;    /* [256] at most 1024 */
    uint32_t seed;           /* [0x52454C4F] */
    int32_t min_inliers;     /* [50]  the fleet's "lost" limit */
    int32_t mode;            /* [0]   0: hypotheses from stereo-triangulated keys (steps B, C); 1: from 2D-3D correspondences (B', C') */
} vslam_reloc_params;

typedef struct vslam_reloc_report {
    int32_t success, n_points, n_pairs, best_hypothesis, best_count;
    int32_t n_inliers, n_stereo;
    vslam_lm_report lm;
} vslam_reloc_report;

vslam_status vslam_relocalize(vslam_matcher* m, const double* points_xyz, const uint8_t* desc, int32_t n_points,
                              const vslam_reloc_params* params, double* T_cw_out,
                              int32_t* pairs_out /* n_points: key index of the point's correspondence or -1; may be NULL */,
                              vslam_reloc_report* report);
/* test tap: of the last vslam_relocalize call on this matcher, per map point (d1, i1, d2) [n_points][3], per left key the
 * winning map point or -1, per hypothesis its count, per correspondence the winner's inlier flag.  sizes4 = {n_points, left
 * keys, hypotheses, correspondences}; any array may be NULL; a capacity below its size: VSLAM_ERR_CAPACITY. */
vslam_status vslam_relocalize_debug(vslam_matcher* m, int32_t* d1_i1_d2, int32_t cap_points, int32_t* key_winner, int32_t cap_keys,
                                    int32_t* hyp_counts, int32_t cap_hypotheses, uint8_t* inlier_flags, int32_t cap_pairs,
                                    int32_t* sizes4);
/* vslam_relocalize for several matchers ("lanes") in one call: one launch per stage for all of them (k_reloc_match_b,
 * k_reloc_pairs_b, k_reloc_ransac_b, k_reloc_best_b with the lane as a grid dimension and a per-lane argument table), one
 * upload, one download, one wait.  A lane's result IS what vslam_relocalize returns for that matcher, points and parameters,
 * including step D's side effect on its stereo match: vslam_relocalize is this call with one lane.  Step D's problem is built
 * on the device (k_reloc_problem_b: the winner's inliers compacted in correspondence order into the lane's pose buffers, with
 * the problem size and a gate word the pose kernel reads there), so that no wait separates steps C and D; a lane with fewer
 * than three correspondences or no inlier is not refined.
 * matchers[b] = NULL: lane b is idle (its report, pairs and T_cw_out row are not written).  Every other matcher must be a
 * different stereo matcher with a completed stereo match, all on one device, else VSLAM_ERR_INVALID; per lane the limits of
 * vslam_relocalize (VSLAM_ERR_CAPACITY); after any error nothing has been launched.  params: one set for all lanes.
 * T_cw_out [lanes][16]: a lane's row is written only on its success.  pairs_out and its entries may be NULL.
 * Streams: matchers that do not share the first active matcher's stream are synchronised first (hipStreamSynchronize on
 * their own streams); all work then runs on the first active matcher's stream, and the call returns after it has finished.
 * vslam_relocalize_debug on a lane's matcher returns that lane's part of the last batched call. */
vslam_status vslam_relocalize_batch(vslam_matcher* const* matchers, int32_t lanes, const double* const* points_xyz,
                                    const uint8_t* const* desc, const int32_t* n_points, const vslam_reloc_params* params,
                                    double* T_cw_out, int32_t* const* pairs_out, vslam_reloc_report* reports);

/* ---------------------------------------------------------------------------
 * Pose-graph optimisation - NO reference counterpart (the reference closes no loops; DESIGN.md section 6 item 24 holds the
 * exact rules, tests/pgo_ref.py restates them on the CPU with a dense solve).  n poses T_wc [n][16] (row-major, world <-
 * camera, rigid), fixed[n], m edges {i, j, Z, w_rot, w_trans} where Z measures T_i^-1 * T_j:
 *   residual    E = Z^-1 * T_i^-1 * T_j (rigid inverses), r = (Log_SO3(R_E), t_E);  cost = sum w_rot |r_w|^2 + w_trans |r_t|^2
 *   retraction  T_k <- T_k * [Exp(a_k), b_k; 0, 1];  analytic Jacobians;  H = J^T W J, g = J^T W r
 *   LM          (H + lambda diag(H)) delta = -g; a trial is accepted iff it lowers the cost: lambda <- max(lambda / 3, 1e-12),
 *               else lambda <- 4 lambda and the trial is repeated from the same linearisation.  Stops after max_iterations
 *               accepted trials, when an accepted trial lowers the cost by less than 1e-10 of it, when |delta|_inf < 1e-12, or
 *               when lambda > 1e8.  An initial cost <= 1e-20 returns at once: zero iterations, poses unchanged.
 *   solve       direct: the free poses reordered on the host by reverse Cuthill-McKee over the free-free edges, H as a
 *               block-banded lower matrix of 6x6 fp64 blocks (half-bandwidth b blocks), factorised and solved on the device
 *               by one workgroup walking the block columns (k_pgo_band_chol_b).  A pivot that is not positive makes the trial
 *               a rejected one whatever its delta (it does not end the loop through the |delta|_inf rule).
 *   kernels     k_pgo_linearize_b (one thread per edge), k_pgo_assemble_b (one wave per free pose gathers its incidence list
 *               in ascending edge order: no atomics), k_pgo_band_copy_b, k_pgo_band_chol_b, k_pgo_retract_b / k_pgo_cost_b /
 *               k_pgo_reduce_b (fixed-order sum): two calls on the same input return the same bytes.  The accept / reject
 *               decision is taken on the device (k_pgo_decide_b, on a control block): the host waits once per trial, for one
 *               int, never inside factor / solve; the calling thread's block cache serves every buffer, so that a repeated
 *               call of unchanged size allocates and frees nothing.  The call is the ONE-LANE CASE of the batched call below:
 *               the same host function, the same kernels.
 * A free pose without any edge is treated as fixed (n_isolated); fixed and isolated poses come back bit for bit; an edge
 * between two fixed poses only adds to the cost; duplicate edges add up.
 * VSLAM_ERR_INVALID, nothing launched: i == j or an index out of range, a non-finite pose / measurement / weight / parameter,
 * a negative weight or parameter, a connected component of free poses without an edge to a fixed pose (a free gauge).
 * VSLAM_ERR_CAPACITY, nothing launched: n > 16384, m > 262144, (b + 1) * n_free > 262144 blocks.
 * ------------------------------------------------------------------------- */
typedef struct vslam_pgo_edge {
    int32_t i, j;
    double Z[16];             /* row-major measurement of T_i^-1 * T_j */
    double w_rot, w_trans;    /* weights of the rotation / translation part (>= 0) */
} vslam_pgo_edge;

typedef struct vslam_pgo_params {     /* a zero field takes the default in brackets (NULL = all defaults) */
    int32_t max_iterations;   /* [20]   accepted trials */
    double lambda0;           /* [1e-4] */
} vslam_pgo_params;

typedef struct vslam_pgo_report {
    int32_t iterations;       /* trials = accepted + rejected */
    int32_t accepted, rejected;
    int32_t n_free, n_isolated, half_bandwidth;
    double initial_cost, final_cost, final_lambda;
} vslam_pgo_report;

vslam_status vslam_pose_graph_optimize(const double* T_wc, const uint8_t* fixed, int32_t n, const vslam_pgo_edge* edges, int32_t m,
                                       const vslam_pgo_params* params, int32_t device, double* T_wc_out /* [n][16]; may be T_wc */,
                                       vslam_pgo_report* report);
/* The same for `lanes` independent graphs in one call, one launch per stage for all of them (the kernels of csrc/pgo.hip,
 * blockIdx = lane, each on a lane's part of concatenated arrays).  THE RULE: a lane's T_wc_out and report are, byte for byte,
 * what vslam_pose_graph_optimize returns for that graph alone with the same params (one params set per call) - by construction,
 * since that call is this one with one lane; order and company of the lanes do not matter.  A lane with n == 0 is idle: its
 * output and report are not written (the single call refuses n < 1).
 *   host      per lane validation, numbering, gauge check, reordering and packing
 *   device    the lanes' arrays concatenated in two blocks from the calling thread's cache (one upload); a lane table
 *             {n, m, n_free, b, offsets}; a control block per lane {active, need_linearize, cur, lambda, cost, accepted,
 *             rejected}.  One ROUND is one trial of every active lane: linearise (lanes whose last trial was accepted),
 *             assemble, copy of the active lanes' bands and gradients (k_pgo_band_copy_b), factor + solve
 *             (k_pgo_band_chol_b: one workgroup per lane), retract, cost, reduce, decide (k_pgo_decide_b: one thread per lane
 *             applies the accept / reject rule above in fp64; it is the only place that rule is written).  A lane that has
 *             stopped costs its workgroups one load.  The host waits once per round, for one int: the number of lanes still
 *             active.
 * VSLAM_ERR_INVALID, nothing launched, no lane written: lanes < 1, NULL graphs / reports, a bad parameter, or any lane the
 * single call would refuse as invalid (the error text names the lane).
 * VSLAM_ERR_CAPACITY, likewise: a lane beyond the single call's limits; lanes > 1024; in all lanes together more than 262144
 * poses, 1048576 edges or 1048576 band blocks (b + 1) * n_free. */
typedef struct vslam_pgo_graph {     /* one lane; n == 0: idle lane (its report and output are not written) */
    const double* T_wc; const uint8_t* fixed; int32_t n;
    const vslam_pgo_edge* edges; int32_t m;
    double* T_wc_out;                /* [n][16]; may be T_wc */
} vslam_pgo_graph;
vslam_status vslam_pose_graph_optimize_batch(const vslam_pgo_graph* graphs, int32_t lanes, const vslam_pgo_params* params,
                                             int32_t device, vslam_pgo_report* reports /* [lanes] */);
/* The YAW-ONLY (4-DoF) solve of the same graphs (csrc/pgo_yaw.hip, csrc/pgo_yaw_dev.hpp; DESIGN.md section 6 item 29, restated
 * by tests/pgo_yaw_ref.py): what a loop correction of a session with an IMU needs, whose world frame carries gravity.  Graph,
 * edges, residual, cost, weights, LM schedule, stopping rules, refusals, capacities and report are those of
 * vslam_pose_graph_optimize.  It differs in four ways:
 *   axis        g = axis / sqrt(x^2 + y^2 + z^2), in fp64 on the host (the axis needs no normalising by the caller).  A zero or
 *               non-finite axis: VSLAM_ERR_INVALID, nothing launched.
 *   parameters  four per free pose, (theta, delta);  retraction T_k <- [Exp(theta g) R_k, t_k + delta]: a rotation about g and a
 *               translation, both on the world side.  Hence R_new R_old^T g = g for every pose: roll and pitch about g never
 *               change (the 6-DoF solve tilts g by 1e-3 .. 6e-2 rad on the graphs of the tests).
 *   Jacobians   J4 = J6 * M_k with M_k = [[R_k^T g, 0], [0, R_k^T]] (6x4) and J6 the 6-DoF Jacobian, multiplied in registers
 *               (k_pgoy_linearize_b stores 24 doubles a side)
 *   solve       H block-banded with 4x4 fp64 blocks, g with 4 entries per pose; damping lambda diag(H), pivot rule and accept /
 *               reject rule are the existing ones.  k_pgoy_assemble_b carries THREE block columns per wave (20 lanes each, each
 *               walking its own incidence list in ascending order: no atomics); k_pgoy_band_chol_b is the walk of
 *               k_pgo_band_chol_b with 4x4 blocks.  Two calls on the same input return the same bytes; the host waits once per
 *               round, for one int.
 * The final cost is never below the 6-DoF solve's of the same graph started from the same poses when both converge (fewer
 * degrees of freedom).  The single call is the one-lane case of the batched one; a lane (graph and its own axis) returns, byte
 * for byte, what the single call returns for it; a lane with graph.n == 0 is idle.  vslam_pose_graph_set_timing /
 * vslam_pose_graph_timings serve these calls too; their groups are pgoy_linearize, pgoy_assemble, pgoy_band_chol, pgoy_retract,
 * pgoy_cost. */
typedef struct vslam_pgo_yaw_graph {     /* one lane of the yaw-only solve */
    vslam_pgo_graph graph;
    double axis[3];                      /* the world axis that rotations are confined to (gravity); any non-zero length */
} vslam_pgo_yaw_graph;
vslam_status vslam_pose_graph_optimize_yaw(const double* T_wc, const uint8_t* fixed, int32_t n, const vslam_pgo_edge* edges, int32_t m,
                                           const double axis[3], const vslam_pgo_params* params, int32_t device,
                                           double* T_wc_out /* [n][16]; may be T_wc */, vslam_pgo_report* report);
vslam_status vslam_pose_graph_optimize_yaw_batch(const vslam_pgo_yaw_graph* graphs, int32_t lanes, const vslam_pgo_params* params,
                                                 int32_t device, vslam_pgo_report* reports /* [lanes] */);
/* k_pgo_move_points_b with one lane: points_out[k] = T_new[r] * T_old[r]^-1 * points_xyz[k] with r = ref_index[k] (rigid inverse:
 * R^T (X - t)); r < 0 leaves the point as it is; r >= n_poses: VSLAM_ERR_INVALID, nothing launched.  points_out may be points_xyz. */
vslam_status vslam_pose_graph_move_points(const double* points_xyz, const int32_t* ref_index, const double* T_old, const double* T_new,
                                          int32_t n_points, int32_t n_poses, int32_t device, double* points_out);
/* measurement hook of tools/pgo_rate.py, not part of the supported surface: per-kernel-group device time of the calling
 * thread's last vslam_pose_graph_optimize or vslam_pose_graph_optimize_batch - the timers sit in the loop both share, so a
 * batched call's figures are those of all its lanes together (HIP events; off by default; thread-local state).  Groups:
 * pgo_linearize, pgo_assemble, pgo_band_chol (with the copy of band and right-hand side), pgo_retract, pgo_cost (k_pgo_cost_b,
 * k_pgo_reduce_b and k_pgo_decide_b, the initial reduce and decide included). */
vslam_status vslam_pose_graph_set_timing(int32_t on);
vslam_status vslam_pose_graph_timings(const char** names, float* ms, int32_t cap, int32_t* n_out);
/* the same hook: how many solves (calls of any of the four optimise entry points, a batched call counting once) have reached the
 * device on the calling thread since its last vslam_pose_graph_set_timing - what shows that a batched loop call made ONE solve */
vslam_status vslam_pose_graph_solve_count(int64_t* n_out);

/* ---------------------------------------------------------------------------
 * Global bundle adjustment (no reference counterpart: the reference closes no loops; DESIGN.md section 6 item 27, restated in
 * numpy by tests/gba_ref.py, which is the authority; csrc/gba.hip, csrc/gba_host.hpp).  Every keyframe and landmark of a
 * flattened problem (vslam_ba_problem, declared with the local BA below) in ONE Levenberg-Marquardt pass, without the local BA's
 * cap of 170 free keyframes: the landmarks are eliminated onto the keyframes and the reduced camera system is solved by the
 * pose-graph solve's block-banded Cholesky after its reordering.  THE RULES:
 *   factors     every set bit of pair_flags is one two-row factor (bit 0 the left camera, bit 1 the right one, displaced by the
 *               baseline), whitened by 1 / sigma, sigma = 1 / inv_sigma_factor[octave].  kf_id is not used: there is no
 *               implicit between-factor chain.  Relative-pose terms are the caller's `edges`, with the residual, weights and
 *               Jacobians of vslam_pose_graph_optimize.
 *   unknowns    poses by the pose-graph retraction T [Exp(a), b; 0, 1], landmarks additive.
 *   cost        sum of the whitened r^2 over the factors + the pose-graph cost of the edges (no 1/2).
 *   presence    a landmark is PRESENT iff it has at least two factors.  A thin landmark contributes nothing, comes back bit
 *               for bit and is counted (n_thin).  A keyframe is FREE iff it is not fixed and has a factor on a present
 *               landmark or an edge; other non-fixed keyframes are isolated, come back bit for bit and are counted.
 *   gauge       two free keyframes are connected iff they share a present landmark or an edge; a component that shares no
 *               present landmark and no edge with a fixed keyframe is refused (VSLAM_ERR_INVALID), as the pose-graph call
 *               refuses a free gauge.  All keyframes fixed is legal: structure only, the landmarks are still optimised.
 *   LM          one pass with the schedule of vslam_pose_graph_optimize (accept: lambda / 3, floor 1e-12; reject: 4 lambda;
 *               stop at lambda > 1e8, a relative decrease < 1e-10, |delta|_inf < 1e-12 over poses and landmarks, or
 *               max_iterations accepted trials; an initial cost <= 1e-20 returns at once).  Damping is lambda diag(H) on the
 *               pose AND the landmark diagonal, applied before the elimination.  A trial is rejected when a pivot of a
 *               landmark's damped 3x3 block or of the band is not positive, when its cost is not finite, or when a factor
 *               has z <= 0.
 *   flags       after the pass pair_wrong is the local BA's chi2 rule (squared pixel error > (float)(7.815f * sigma_factor
 *               [octave]) or z <= 0; left, then right) over the pairs of kf_local keyframes on present landmarks; other pairs
 *               get 0.  The call removes nothing itself: for a second pass clear the flagged pairs' flags and call again.
 * VSLAM_ERR_INVALID, nothing launched, nothing written: NULL arrays, n_kf < 1, an index out of range, an edge with i == j, a
 * non-finite value, a negative weight or parameter, an octave outside the tables, a free gauge, a factor on a present landmark
 * with z <= 0 at the initial values (the message names the pair).
 * VSLAM_ERR_CAPACITY, likewise, checked before anything is sized: n_kf > 16384, n_edges > 262144, n_pairs > 2097152,
 * n_lm > 1048576, the squares of the present landmarks' free-keyframe pair counts summing to more than 16777216 (the bound of
 * the block lists' length), a band of (b + 1) * n_free > 262144 blocks.
 * Per trial: linearise (only after an accepted trial), the landmarks' damped blocks, W and Y = W Hll^-1 per pair, the reduced
 * system GATHERED per block of the band over lists built once on the host (no floating-point atomics: two calls on the same
 * input return the same bytes), band copy, factor and solve (pgo_band_chol_walk), landmark back-substitution, retraction, cost,
 * fixed-order sum and the accept / reject rule on a device control block.  The host waits once per trial, for one int; every
 * buffer comes from the calling thread's block cache.
 * ------------------------------------------------------------------------- */
struct vslam_ba_problem;
typedef struct vslam_gba_params {     /* a zero field takes the default in brackets (NULL = all defaults) */
    int32_t max_iterations;   /* [20]   accepted trials */
    double lambda0;           /* [1e-4] */
} vslam_gba_params;

typedef struct vslam_gba_report {
    int32_t iterations;       /* trials = accepted + rejected */
    int32_t accepted, rejected;
    int32_t n_free, n_isolated;           /* keyframes */
    int32_t n_present, n_thin;            /* landmarks */
    int32_t n_factors;                    /* two-row factors on present landmarks */
    int32_t half_bandwidth;               /* b, in blocks, after the reordering */
    int32_t reserved;
    double initial_cost, final_cost, final_lambda;
} vslam_gba_report;

typedef struct vslam_gba_result {
    double* kf_pose_wc;       /* n_kf x 16 (may be the problem's array) */
    double* lm_xyz;           /* n_lm x 3  (may be the problem's array) */
    uint8_t* pair_wrong;      /* n_pairs */
    vslam_gba_report report;
} vslam_gba_result;

vslam_status vslam_global_ba(const struct vslam_ba_problem* problem, const vslam_pgo_edge* edges, int32_t n_edges,
                             const vslam_gba_params* params, int32_t device, vslam_gba_result* result);
/* vslam_global_ba_batch: several problems (lanes) at once, one launch per stage for all of them (csrc/gba.hip, the layout of
 * vslam_pose_graph_optimize_batch).  THE RULE: a lane's poses, landmarks, pair_wrong and report are, byte for byte, what
 * vslam_global_ba returns for that problem alone with the same params; the order and company of the lanes do not matter.  The
 * kernels of both calls run the same __device__ bodies (csrc/gba_dev.hpp) - the batched ones on a lane's part of concatenated
 * arrays, with the lane as a grid dimension, the lane's own camera (lanes may have different rigs) and the lane's own
 * Levenberg-Marquardt state and pivot flags.  A ROUND is one trial of every active lane: linearise, landmarks, W / Y, the
 * edges' columns and the gather (grids sized by the largest lane), band copy, the factorisation (k_gba_band_chol_b: one
 * workgroup per lane, so the lanes' dependency chains run side by side), back-substitution, retraction, cost, the per-lane
 * fixed-order sum (k_gba_reduce_b) and the rule (k_gba_decide_b: a thread per lane).  A lane that has stopped costs its
 * workgroups one load.  The host waits once per round, for one int: the number of lanes still active.  No floating-point atomics.
 * VSLAM_ERR_INVALID, nothing launched, no lane written: n_lanes < 1, NULL lanes, a lane with a problem and no result, a bad
 * parameter, or any lane the single call would refuse as invalid (the error text names the lane).
 * VSLAM_ERR_CAPACITY, likewise: a lane beyond the single call's limits; n_lanes > 1024; in all lanes together more than 262144
 * keyframes, 1048576 edges, 8388608 pairs, 4194304 landmarks, 1048576 band blocks (b + 1) * n_free or 67108864 block-list
 * entries (every offset of the lane table is an element count that fits int32). */
typedef struct vslam_gba_lane {            /* one lane; problem == NULL or problem->n_kf == 0: idle lane, nothing read or written */
    const struct vslam_ba_problem* problem;
    const vslam_pgo_edge* edges; int32_t n_edges;
    vslam_gba_result* result;              /* as for vslam_global_ba; its arrays may be the problem's */
} vslam_gba_lane;
vslam_status vslam_global_ba_batch(const vslam_gba_lane* lanes, int32_t n_lanes, const vslam_gba_params* params, int32_t device);
/* The global bundle adjustment with YAW-ONLY (4-DoF) keyframes (csrc/gba_yaw.hip, csrc/gba_yaw_dev.hpp; DESIGN.md section 6
 * item 30, restated by tests/gba_yaw_ref.py, which is the authority): what a stereo + IMU session needs from a global
 * adjustment, whose world frame carries gravity and whose roll and pitch the IMU observes.  THE RULES are those of
 * vslam_global_ba above - factors, presence, gauge, LM schedule, damping, flags, refusals and limits - with ONE change:
 *   axis        g = axis / sqrt(x^2 + y^2 + z^2), in fp64 on the host (the expression of vslam_pose_graph_optimize_yaw; the axis
 *               needs no normalising by the caller).  A zero or non-finite axis: VSLAM_ERR_INVALID, nothing launched, nothing
 *               written.  Every lane of the batched call has its own axis.
 *   parameters  four per free keyframe, (theta, delta);  retraction T <- [Exp(theta g) R, t + delta].  Hence
 *               R_new R_old^T g = g for every keyframe (to 1e-12): roll and pitch about g never change, where the 6-DoF call
 *               tilts g by 2e-3 .. 1.5e-1 rad on the problems of the tests.  Landmarks stay additive.  Fixed and isolated
 *               keyframes and thin landmarks come back bit for bit.
 *   Jacobians   projection factor: the 6-DoF factor unchanged, then Jp4 [2][4] = Jp6 [2][6] * M_k in registers, with
 *               M_k = [[R_k^T g, 0], [0, R_k^T]] (6x4); Jl, the residual and the cost term are unchanged.  Edges: the Jacobians of
 *               vslam_pose_graph_optimize_yaw (24 doubles a side).  The cost does not depend on the parameterisation.
 *   solve       W and Y are [4][3] per pair; the reduced camera system is block-banded with 4x4 fp64 blocks, gathered THREE
 *               listed blocks per wave (20 lanes each: 16 elements and, on a diagonal block, 4 gradient components; each block
 *               walks its own list in ascending order, so an element's sum does not depend on the block's company), factored and
 *               solved by the 4x4 walk of vslam_pose_graph_optimize_yaw, one workgroup per lane.  Damping is lambda diag(H) on
 *               the 4x4 pose diagonal and on the landmark diagonal, before the elimination.  The steps are laid out as
 *               n_free * 4 pose entries followed by n_lm * 3; |delta|_inf runs over both.
 * No floating-point atomics: the same input gives the same bytes, and a lane's bytes do not depend on the other lanes or on
 * their order.  vslam_global_ba_yaw is the one-lane case of vslam_global_ba_yaw_batch (one set of kernels); a lane whose problem
 * is NULL or has n_kf == 0 is idle (nothing read, its axis included, nothing written).  The batched call's refusals and sums
 * over all lanes are those of vslam_global_ba_batch.  With every keyframe fixed only bodies shared with vslam_global_ba run: the
 * result equals that call's byte for byte.  Without landmarks the call is vslam_pose_graph_optimize_yaw on the edges.
 * vslam_global_ba_set_timing / _timings below cover these calls too, with the same group names. */
typedef struct vslam_gba_yaw_lane {        /* one lane of the yaw-only adjustment */
    vslam_gba_lane lane;
    double axis[3];                        /* the world axis that keyframe rotations are confined to (gravity); any non-zero length */
} vslam_gba_yaw_lane;
vslam_status vslam_global_ba_yaw(const struct vslam_ba_problem* problem, const vslam_pgo_edge* edges, int32_t n_edges, const double axis[3],
                                 const vslam_gba_params* params, int32_t device, vslam_gba_result* result);
vslam_status vslam_global_ba_yaw_batch(const vslam_gba_yaw_lane* lanes, int32_t n_lanes, const vslam_gba_params* params, int32_t device);
/* measurement hook of tools/gba_rate.py, in the form of the pose-graph one: device time (HIP events) per kernel group of the
 * calling thread's last vslam_global_ba, vslam_global_ba_batch, vslam_global_ba_yaw or vslam_global_ba_yaw_batch (a batched
 * call's figures are those of all its lanes together) - gba_linearize, gba_landmarks, gba_assemble, gba_band_chol, gba_back,
 * gba_cost, gba_chi2; off by default; thread-local state. */
vslam_status vslam_global_ba_set_timing(int32_t on);
vslam_status vslam_global_ba_timings(const char** names, float* ms, int32_t cap, int32_t* n_out);

/* ---------------------------------------------------------------------------
 * Duplicate search between two copies of a place (no reference counterpart: the reference closes no loops; DESIGN.md section 6
 * item 26, restated in numpy by tests/fuse_ref.py; csrc/fuse.hip).  Set A is the new copy (it will be absorbed), set B the old
 * one (it is kept): world positions (fp64 [3]) and 256-bit descriptors (32 bytes) of up to 65536 points each.  Both are
 * projected into ONE camera, T_cw (camera <- world, row-major 4x4, rigid) with the intrinsics fx, fy, cx, cy and the image
 * size w x h, and every A point looks for its twin among the B points that land beside it.  THE RULES:
 *   1 projection  Xc[i] = (R[i][0] X[0] + R[i][1] X[1] + R[i][2] X[2]) + t[i] in fp64, no contraction.  Visible iff z > 0 and,
 *                 with invZ = 1.0 / z, u = fx * x * invZ + cx, v = fy * y * invZ + cy, not (u < 0 || v < 0 || u >= w || v >= h).
 *                 A visible point's record is ((float)u, (float)v, (float)z); an invisible point's record is (NaN, NaN, -1.f).
 *   2 gate        in float, no contraction: du = ua - ub, dv = va - vb; the pair passes iff du * du + dv * dv <= radius * radius
 *                 and zb <= depth_ratio * za and za <= depth_ratio * zb.  A comparison with NaN is false, so an invisible record
 *                 passes against nothing at any depth_ratio, without a visibility branch: an invisible A point proposes
 *                 nothing, an invisible B point is proposed to by nobody.  (z = -1 alone fails the depth compares against every
 *                 visible point, but two such records would pass each other at depth_ratio = 1: hence the NaN.)
 *   3 best target every visible A point a scans the B points in ascending index: d1 = the smallest 256-bit Hamming distance
 *                 among the gated ones, b1 = the lowest index attaining it, d2 = the smallest distance among the OTHER gated
 *                 points (257: none), n_gated = their number.  a proposes b1 iff n_gated > 0 and d1 <= max_hamming.  No ratio
 *                 test (inside a few pixels there are too few candidates for one to mean anything).
 *   4 one to one  B point b goes to the proposer with the smallest (d1 << 32 | a): a 64-bit integer atomicMin (deterministic, no
 *                 floating-point atomics).  A proposer that loses stays unmatched; it gets no second choice.
 *   5 outputs     match [n_a]: the B index or -1; best [n_a][4] = (d1, b1, d2, n_gated), (257, -1, 257, 0) for a point that
 *                 gated nothing; the report below.
 * Kernels, all with a per-lane argument table and the lane as a grid dimension: k_fuse_project_b (a thread per point of either
 * set: the 16-byte record), k_fuse_match_b (a thread per A point, B staged through LDS in tiles of 1024 targets, record and
 * descriptor together; the gate first, eight targets per wave vote, and a target's descriptor is read and counted only when some
 * lane of the wave passed its gate - wave-uniform, so results cannot depend on it; VSLAM_FUSE_SKIP=0, a developer switch read per call, counts every
 * target), k_fuse_resolve_b (a thread per A point reads the winner back; one workgroup per lane counts).  One upload, one launch
 * per stage for all lanes, one download, one wait, on the calling thread's device pool.  vslam_fuse_search is its own argument
 * checks and then the ONE-LANE CASE of the batched call: the same host function, the same kernels - a lane's bytes are the
 * single call's by construction, whatever the order and company of the lanes.
 * A lane with n_a = 0 or n_b = 0 is idle for the search: match entries, if any, are -1, best rows (257, -1, 257, 0), the report
 * counts what is visible.  A lane with both zero is not read and not written at all.
 * VSLAM_ERR_INVALID, nothing launched, every output and report as the caller left it (the batch names the lane): NULL arrays,
 * lanes < 1, a negative count, a non-finite pose / coordinate / intrinsic / parameter, w or h < 1, a negative parameter,
 * depth_ratio inside (0, 1).  VSLAM_ERR_CAPACITY, likewise: n_a or n_b > 65536, lanes > 256, more than 1048576 points over all
 * lanes.
 * ------------------------------------------------------------------------- */
typedef struct vslam_fuse_params {    /* a zero field takes the default in brackets (NULL = all defaults) */
    float radius;                     /* [4.0]  pixels */
    float depth_ratio;                /* [1.25] the larger depth over the smaller, at most */
    int32_t max_hamming;              /* [50]   vslam_relocalize's acceptance distance */
} vslam_fuse_params;

typedef struct vslam_fuse_report {
    int32_t n_visible_a, n_visible_b; /* points of either set inside the image */
    int32_t n_proposals;              /* A points that proposed a target */
    int32_t n_pairs;                  /* A points that won theirs */
} vslam_fuse_report;

typedef struct vslam_fuse_lane {      /* one lane; n_a == 0 and n_b == 0: idle lane (nothing read, nothing written) */
    const double* T_cw;               /* [16] */
    double fx, fy, cx, cy;
    int32_t w, h;
    const double* a_xyz; const uint8_t* a_desc; int32_t n_a;      /* [n_a][3], [n_a][32] */
    const double* b_xyz; const uint8_t* b_desc; int32_t n_b;
    int32_t* match;                   /* [n_a] */
    int32_t* best;                    /* [n_a][4] */
} vslam_fuse_lane;

vslam_status vslam_fuse_search_batch(const vslam_fuse_lane* lanes, int32_t n_lanes, const vslam_fuse_params* params, int32_t device,
                                     vslam_fuse_report* reports /* [n_lanes] */);
vslam_status vslam_fuse_search(const double* T_cw, double fx, double fy, double cx, double cy, int32_t w, int32_t h,
                               const double* a_xyz, const uint8_t* a_desc, int32_t n_a,
                               const double* b_xyz, const uint8_t* b_desc, int32_t n_b,
                               const vslam_fuse_params* params, int32_t device, int32_t* match, int32_t* best, vslam_fuse_report* report);
/* measurement hook of tools/fuse_rate.py, not part of the supported surface: device time (HIP events) of each stage of the
 * calling thread's last search - fuse_project, fuse_match, fuse_resolve; off by default; thread-local state. */
vslam_status vslam_fuse_set_timing(int32_t on);
vslam_status vslam_fuse_timings(const char** names, float* ms, int32_t cap, int32_t* n_out);

/* ---------------------------------------------------------------------------
 * Local bundle adjustment — replaces the numerical core of LocalMapper::localBA
 * (include/OptimizationBA.h:75, src/OptimizationBA.cpp:543-873): GenericProjectionFactor
 * (left, and right with the stereo extrinsics) per observation, BetweenFactor<Pose3>
 * (sigma 0.01) between id-consecutive keyframes, NonlinearEquality on fixed keyframes,
 * landmarks-first elimination (:942-953) = Schur complement onto the free keyframes, dense
 * Cholesky of the reduced camera system, two LM passes (5 then 10 iterations, tol 1e-5)
 * separated by the chi2 (7.815 * sigmaFactor) re-check (:787-871).  The walk over the
 * KeyFrame / MapPoint pointer graph that selects the window (:438-516) stays on the caller's
 * side; the problem arrives flattened, with dense keyframe / landmark indices.
 * ------------------------------------------------------------------------- */
typedef struct vslam_ba_problem {
    vslam_rig rig;
    int32_t n_levels;
    const float* sigma_factor;      /* KeyFrame::sigmaFactor[n_levels]    (chi2 threshold multiplier) */
    const float* inv_sigma_factor;  /* KeyFrame::InvSigmaFactor[n_levels] (noise sigma = 1/this)      */
    int32_t n_kf;
    const double* kf_pose_wc;       /* n_kf x 16 row-major, world <- camera (KeyFrame pose)           */
    const int64_t* kf_id;           /* KeyFrame::numb (orders the BetweenFactor chain)                 */
    const uint8_t* kf_fixed;        /* 1: pinned by NonlinearEquality (kf->fixed or a fixedKFs member) */
    const uint8_t* kf_local;        /* 1: member of localKFs (its observations are chi2-checked)       */
    int32_t n_lm;
    const double* lm_xyz;           /* n_lm x 3 */
    int32_t n_pairs;                /* (keyframe, landmark) entries of MapPoint::kFMatches             */
    const int32_t* pair_kf;
    const int32_t* pair_lm;
    const uint8_t* pair_flags;      /* bit0: left factor, bit1: right factor (right-only or `close`)   */
    const float* pair_uv;           /* n_pairs x 4: uL, vL, uR, vR (cv::KeyPoint::pt)                  */
    const int32_t* pair_octave;     /* n_pairs x 2: octave of the left / right keypoint                */
} vslam_ba_problem;

typedef struct vslam_ba_result {
    double* kf_pose_wc;             /* n_kf x 16 optimised poses (fixed ones unchanged)                */
    double* lm_xyz;                 /* n_lm x 3 */
    uint8_t* pair_wrong;            /* n_pairs: wrongMatches after the second pass                     */
    uint8_t* pair_wrong_pass1;      /* optional (may be NULL): wrongMatches after the first pass       */
    vslam_lm_report report[2];
    int64_t n_residuals, n_landmarks, n_free_kf, sum_k2;   /* work figures of the last pass           */
    int64_t rounds;                 /* trial rounds of both passes (one round = up to 4 lambda candidates evaluated at once) */
} vslam_ba_result;

/* Write-back of localBA, numerical part of MapPoint::updatePos (src/Map.cpp:212-234) as called from
 * src/OptimizationBA.cpp:913-933 after the keyframe poses were set (:891-910): for every (keyframe, landmark) entry
 * still in kFMatches (pair_wrong == 0) of a landmark that is not flagged an outlier, whose left keypoint currently
 * has estimatedDepth > 0:  estimatedDepth = (T_cw * wp).z  (stored as float),  close = true when that z <=
 * 40 * baseline (never reset).  Pair-parallel; the caller scatters depth_out / close_out into
 * TrackedKeys::estimatedDepth / close at keyPos.first where updated_out is 1.  (Entries with keyPos.first < 0
 * index estimatedDepth[-1] in the reference: pass cur_depth <= 0 for them; they are skipped.)
 * calcDescriptor of the same function is vslam_calc_descriptors. */
vslam_status vslam_ba_refresh_depth(const vslam_rig* rig, int32_t n_kf, const double* kf_pose_wc, int32_t n_lm,
                                    const double* lm_xyz, const uint8_t* lm_outlier, int32_t n_pairs,
                                    const int32_t* pair_kf, const int32_t* pair_lm, const uint8_t* pair_wrong,
                                    const float* cur_depth, int32_t device, float* depth_out, uint8_t* close_out,
                                    uint8_t* updated_out);
/* The same for n_req requests of DIFFERENT cameras staged together, as a lockstep group serves the write-backs of its
 * lanes: request r brings req_n_kf[r] keyframe poses and its rig rigs[r]; kf_pose_wc is the concatenation (pair_kf
 * indexes it), landmarks and pairs likewise.  ONE launch; every pair is tested against 40 * baseline of its own
 * keyframe's camera.  Outputs equal those of one vslam_ba_refresh_depth call per request. */
vslam_status vslam_ba_refresh_depth_merged(const vslam_rig* rigs, const int32_t* req_n_kf, int32_t n_req, const double* kf_pose_wc,
                                           int32_t n_lm, const double* lm_xyz, const uint8_t* lm_outlier, int32_t n_pairs,
                                           const int32_t* pair_kf, const int32_t* pair_lm, const uint8_t* pair_wrong,
                                           const float* cur_depth, int32_t device, float* depth_out, uint8_t* close_out,
                                           uint8_t* updated_out);

/* KeyFrame::updatePose(keyPose) (src/KeyFrame.cpp:6-76) — the per-keyframe step of FeatureTracker::changePosesLCA
 * (src/FeatureTracker.cpp:884-908), applied along the keyframe chain after a local BA / loop closure moved an earlier
 * keyframe: newPose = keyPose * refPose; map points created by this keyframe (kdx == numb) move with it
 * (newPose * (currPoseInv * p)); observations of older points (kdx < numb) are re-projected into the new left / right
 * camera and dropped when ((du^2 + dv^2) * InvSigmaFactor[octave]) > 7.815f.  slot_lm_l / slot_lm_r give the landmark
 * index of localMapPoints[idx] / localMapPointsR[idx] (-1 = nullptr).  Outputs: lm_xyz updated in place, drop_l /
 * drop_r = 1 where the reference nulls the slot (caller: unMatchedF[idx] = -1, eraseKFConnection), pose_out =
 * the keyframe's new pose (CameraPose::changePose).  A map point occupies at most one left slot (as in the reference's
 * localMapPoints).  Call per keyframe in chain order. */
typedef struct {
    vslam_rig rig;
    int32_t n_levels;
    const float* inv_sigma_factor;
    int64_t numb;                       /* KeyFrame::numb */
    const double* key_pose;             /* [16] pose of the previous keyframe in the chain (kf->getPose()) */
    const double* ref_pose;             /* [16] pose.refPose */
    const double* cur_pose_inv;         /* [16] pose.poseInverse before the update */
    int32_t n_left, n_right;
    const vslam_keypoint* kps_left; const vslam_keypoint* kps_right;
    const int32_t* slot_lm_l; const int32_t* slot_lm_r;
    int32_t n_lm;
    double* lm_xyz;                     /* in/out [n_lm][3] */
    const int64_t* lm_kdx;              /* MapPoint::kdx */
    const uint8_t* lm_outlier;          /* MapPoint::GetIsOutlier() */
} vslam_kf_update_problem;

vslam_status vslam_keyframe_update_pose(const vslam_kf_update_problem* problem, int32_t device, uint8_t* drop_l,
                                        uint8_t* drop_r, double* pose_out);

/* VSlamSystem::saveTrajectoryAndPosition (src/System.cpp:87-124), host only: one line per frame of allFramesPoses in
 * the KITTI format (the 12 entries of the first three rows of the camera-to-world pose, row-major, separated by
 * blanks, default ostream formatting = 6 significant digits) and, in the second file, its translation "tx ty tz ".
 * A keyframe contributes pose_or_ref[i] as its pose; any other frame pose(closest previous keyframe) * pose_or_ref[i]
 * (its refPose).  Before the first keyframe the closest keyframe is frame 0, as in the reference.
 * path_positions may be NULL. */
vslam_status vslam_save_trajectory(const char* path_trajectory, const char* path_positions, int32_t n_frames,
                                   const uint8_t* is_keyframe, const double* pose_or_ref);

/* Communicator for landmark-sharded BA (NULL = single GPU).  Every rank passes the SAME flattened problem;
 * rank r owns the landmarks with index % world == r, forms its partial reduced camera system, and one
 * all-reduce(sum, fp64) of [(6F)^2 + 6F] doubles per lambda trial (plus a 3-double cost reduction) makes the
 * system identical everywhere; every rank then solves it redundantly and back-substitutes its own landmarks.
 * Two transports:
 *   rccl  : one process per GPU, RCCL over xGMI.  Rank 0 calls vslam_comm_unique_id, the host program
 *           broadcasts the 128 bytes (e.g. torch.distributed), every rank calls vslam_comm_create_rccl.
 *   local : `world` host threads of ONE process sharing one GPU, exchanging through host memory in a
 *           fixed rank order (deterministic) — the single-box stand-in used by the tests.
 *   callback : see vslam_comm_create_callback below. */
typedef struct vslam_comm vslam_comm;
vslam_status vslam_comm_unique_id(uint8_t id_out[128]);
vslam_status vslam_comm_create_rccl(const uint8_t id[128], int32_t rank, int32_t world, int32_t device,
                                    vslam_comm** out);
vslam_status vslam_comm_create_local(int32_t world, vslam_comm** out_array /* world handles */);
/* callback: the caller supplies the collective - an in-place fp64 SUM over the ranks of n doubles in HOST memory (return 0 on success);
 *           the library stages the reduced camera systems through the host around it.  For process groups RCCL cannot serve
 *           (several ranks on one device, gloo / MPI worlds, mixed hosts): ranks may live in separate processes on any devices. */
typedef int (*vslam_allreduce_fn)(void* ctx, double* host_buf, size_t n);
vslam_status vslam_comm_create_callback(int32_t rank, int32_t world, int32_t device, vslam_allreduce_fn allreduce, void* ctx,
                                        vslam_comm** out);
void vslam_comm_destroy(vslam_comm* comm);

/* The same for n independent tracker-window problems at once (the local mapping of a lockstep group, vslam_batch): ONE kernel
 * launch per stage for all of them (per-problem argument blocks in a device table, grid z = problem; every problem keeps its
 * own device-side LM control block, so each follows exactly the LM trajectory of its own vslam_local_ba call).  Problems
 * outside that class (more than 20 free keyframes, empty graphs) are served by the one-problem path inside the call. */
vslam_status vslam_local_ba_batch(const vslam_ba_problem* const* problems, vslam_ba_result* const* results, int32_t n, int32_t device);

/* Launch plan of vslam_local_ba_batch.  The call measures each problem's first-pass graph (vslam_ba_lane_shape), sends the
 * problems outside the batched class to the one-problem path and picks the kernels and launch geometry of the others from
 * the cohort's maxima.  vslam_local_ba_batch_plan is that choice as a pure host function (no device needed); the batch
 * call uses the same function, and vslam_local_ba_last_batch_plan returns what it chose on the calling thread. */
typedef struct vslam_ba_lane_shape {
    int32_t n_free_kf;      /* free keyframes of the graph (6 unknowns each) */
    int32_t n_points;       /* landmarks of the graph */
    int32_t n_factors;      /* projection factors (left and right) */
    int32_t n_edges;        /* odometry edges */
    int32_t n_pairs;        /* the problem's (keyframe, landmark) pairs */
    int32_t max_slots;      /* most free keyframes observing one landmark */
    int32_t max_factors;    /* most factors of one landmark (fixed keyframes included) */
    int32_t own_rig;        /* 1: the problem runs on its own (vslam_local_ba_batch sets it for a pyramid depth other than the first
                             * problem's; camera rigs may differ between the problems of a batch) */
} vslam_ba_lane_shape;

typedef struct vslam_ba_batch_shape {
    int32_t n_lanes;
    const vslam_ba_lane_shape* lanes;
    int32_t lookahead;      /* lambda candidates per trial round, 1..4 (vslam_local_ba_set_lookahead) */
    int32_t solver;         /* 0 MFMA forms, 1 wave / LDS forms (vslam_local_ba_set_solver) */
} vslam_ba_batch_shape;

enum {
    VSLAM_BA_KERNEL_NONE = 0,
    VSLAM_BA_KERNEL_SCHUR = 1,      /* k_ba_schur: Schur accumulation staged by slots */
    VSLAM_BA_KERNEL_SCHUR2 = 2,     /* k_ba_schur2: tracker windows, staged by factors */
    VSLAM_BA_KERNEL_BACK = 3,       /* k_ba_back */
    VSLAM_BA_KERNEL_BACK2 = 4       /* k_ba_back2 */
};
enum { VSLAM_BA_SOLVE_MFMA64 = 1, VSLAM_BA_SOLVE_WAVE = 2, VSLAM_BA_SOLVE_MFMA = 4 };      /* bits of solve_kinds */

typedef struct vslam_ba_batch_plan {
    int32_t status;         /* VSLAM_OK, or VSLAM_ERR_CAPACITY when a launch cannot fit the LDS */
    int32_t n_batch;        /* problems run by the batched kernels */
    int32_t n_single;       /* problems sent to the one-problem path */
    int32_t lookahead;
    int32_t f_max, max_slots, max_factors, lp_max;      /* maxima over the batched problems */
    int32_t schur_kernel, schur_waves, schur_shared_w, schur_blocks, schur_lds;   /* waves per workgroup, dynamic LDS bytes */
    int32_t back_kernel, back_waves, back_shared, back_blocks, back_lds;
    int32_t solve_kinds;    /* VSLAM_BA_SOLVE_* bits of the solves launched */
    int32_t solve_lds;      /* dynamic LDS bytes of the MFMA solve (0 if it is not launched) */
} vslam_ba_batch_plan;

vslam_status vslam_local_ba_batch_plan(const vslam_ba_batch_shape* shape, vslam_ba_batch_plan* plan);
/* the plan of the calling thread's last vslam_local_ba_batch call (zeroed if that call returned before planning) */
vslam_status vslam_local_ba_last_batch_plan(vslam_ba_batch_plan* plan);

vslam_status vslam_local_ba(const vslam_ba_problem* problem, vslam_ba_result* result, int32_t device,
                            const vslam_comm* comm);
/* device time per kernel group of the last vslam_local_ba call on this thread */
vslam_status vslam_local_ba_timings(const char** names, float* ms, int32_t cap, int32_t* n_out);
/* event timing on (default) / off for the following vslam_local_ba calls of the calling thread */
vslam_status vslam_local_ba_set_timing(int32_t on);
int32_t vslam_local_ba_get_timing(void);      /* the calling thread's switch */
/* Scheduling knobs of the single-GPU path.  They do not change the algorithm (same LM trajectory; values equal up
 * to the summation order of fp64 atomics, which already varies from run to run):
 *   candidates (1..4, <= 0: default 4)  damping values lambda, 10 lambda, ... evaluated per trial round and then
 *                                       walked in GTSAM's sequential order on the device;
 *   speculative_linearize (0 / 1, < 0: default on)  linearise at every trial point, so an accepted step needs no
 *                                       launch of its own;
 *   mask_second_pass (0 / 1, default 1)  run the second optimisation on the first one's factor ordering with the
 *                                       rejected pairs' weights set to zero instead of rebuilding it on the host
 *                                       (falls back to the rebuild when a keyframe loses all its observations).
 * The settings belong to the CALLING THREAD (like the timing switch and the workspace: one optimizer thread = one
 * local-BA context), so sessions with different settings do not interact. */
vslam_status vslam_local_ba_set_lookahead(int32_t candidates, int32_t speculative_linearize, int32_t mask_second_pass);
/* Which reduced-camera solve serves the calling thread's following local BAs: -1 default (the MFMA forms: one wave with the
 * 16x16 tiles in accumulators up to 64 unknowns, eight waves up to 256, block-column Cholesky beyond; VSLAM_BA_NO_MFMA in the
 * environment flips the process default), 0 the MFMA forms, 1 the wave / LDS forms (matrix rows in registers with v_readlane
 * pivots up to 60 unknowns, LDS / L2-resident row-per-thread Cholesky beyond).  Same arithmetic up to the summation order. */
vslam_status vslam_local_ba_set_solver(int32_t kind);

/* ---------------------------------------------------------------------------
 * New-point pipeline of the optimizer thread — replaces the numerical part of LocalMapper::findNewPoints
 * (include/OptimizationBA.h:54-100, src/OptimizationBA.cpp:340-391): calcAllMpsOfKFROnlyEst (:234-287),
 * predictKeysPosR (:289-338), FeatureMatcher::matchByProjectionRPredLBA (src/FeatureMatcher.cpp:66-252),
 * triangulateNewPoints (:127-209, gtsam::triangulatePoint3<Cal3_S2>: DLT, rank_tol 1e-9, cheirality) and
 * checkReprojError (:14-88).  The KeyFrame / MapPoint pointer graph arrives flattened; creating the MapPoint
 * objects from the result (addMultiViewMapPointsR / addNewMapPoints) stays with the caller.
 * kfs[0] is lastKF (= actKeyF.front()), the others follow in the window's order.
 * ------------------------------------------------------------------------- */
/* A keyframe's IMMUTABLE TrackedKeys arrays (keypoints, descriptors, rightIdxs / leftIdxs of both sides) resident in HBM: a
 * keyframe is searched by the new-point pipeline of every later pass whose window holds it, so its ~200 KB travel to the device
 * once (at insertion) instead of once per pass.  A block is `vslam_kf_keys_bytes(n_left, n_right)` bytes of device memory owned by
 * the caller (e.g. a slot of a slab); vslam_kf_keys_upload fills it from host arrays. */
size_t vslam_kf_keys_bytes(int32_t n_left, int32_t n_right);

typedef struct {
    const double* T_wc;                /* KeyFrame::pose.pose, row-major 4x4 */
    int64_t id;                        /* KeyFrame::numb */
    int32_t n_left, n_right;
    const vslam_keypoint* kps_l; const uint8_t* desc_l;      /* keys.keyPoints / Desc */
    const vslam_keypoint* kps_r; const uint8_t* desc_r;      /* keys.rightKeyPoints / rightDesc */
    const int32_t* right_idxs; const int32_t* left_idxs;     /* keys.rightIdxs / leftIdxs */
    const int32_t* unmatched_f; const int32_t* unmatched_fr; /* KeyFrame::unMatchedF / unMatchedFR (>= 0: has a map point) */
    const void* device_keys;           /* NULL, or the keyframe's device block (vslam_kf_keys_upload): the six immutable arrays above are
                                          then read from it and only unmatched_f / unmatched_fr are uploaded */
    const float* estimated_depth; const uint8_t* close_flags;   /* vslam_kf_keys_upload only (may be NULL): the block also has room for
                                          keys.estimatedDepth / close as they were at insertion (the layout of a lockstep step's key block) */
} vslam_kf_view;
/* fills a device block of vslam_kf_keys_bytes(n_left, n_right) bytes from the view's host arrays (synchronous) */
vslam_status vslam_kf_keys_upload(const vslam_kf_view* view, int32_t device, void* device_block);

typedef struct {
    vslam_rig rig;
    int32_t n_levels;
    const float* scale_pyramid;        /* KeyFrame::scaleFactor */
    const float* sigma_factor;         /* KeyFrame::sigmaFactor */
    float log_scale;                   /* KeyFrame::logScale */
    int32_t n_kf;                      /* <= 16 */
    const vslam_kf_view* kfs;
    /* last keyframe only, one entry per left keypoint */
    const float* estimated_depth;      /* keys.estimatedDepth */
    const uint8_t* has_mp;             /* localMapPoints[i] != nullptr */
    const double* mp_xyz;              /* its world position (read where has_mp) */
    const uint8_t* mp_desc;            /* its descriptor, 32 B (read where has_mp) */
} vslam_new_points_problem;

typedef struct {
    int32_t capacity;                  /* entries the arrays below can hold (kfs[0].n_left is always enough) */
    int32_t n_candidates;              /* out: p4d.size() */
    int32_t* cand_left; int32_t* cand_right;   /* out: the candidate's (left, right) keypoint in lastKF */
    uint8_t* accepted;                 /* out: triangulated, in front of every camera, >= 3 keyframes left after the
                                          reprojection filter, lastKF among them */
    double* xyz;                       /* out [n][3]: triangulated position (valid where accepted) */
    int32_t* n_obs;                    /* out: matchesOfPoint.size() on exit */
    int32_t* obs;                      /* out [n][n_kf][3]: (keyframe index, left idx, right idx), -1 padded */
} vslam_new_points_result;

vslam_status vslam_find_new_points(const vslam_new_points_problem* problem, vslam_new_points_result* result,
                                   int32_t device);
/* the same for n windows at once (the cohort of a lockstep group): one upload, one launch per kernel for all of them (grid z =
 * window, arguments from a device table), one download; results equal n vslam_find_new_points calls */
vslam_status vslam_find_new_points_batch(const vslam_new_points_problem* const* problems, vslam_new_points_result* const* results,
                                         int32_t n, int32_t device);

/* Mono map-point creation — replaces the numerical part of FeatureTracker::addMappointsMono
 * (src/FeatureTracker.cpp:1497-1553) after its matchByRadius passes (vslam_match_by_radius):
 * calculateMPFromMono (:1580-1636: gtsam::triangulatePoint3 DLT over the left observations, cheirality, the
 * `p4d(2) < 0.1` test) and the mono checkReprojError (:1638-1684) for every keypoint of the last keyframe.
 * Quirks kept: that test looks at the WORLD z; the reprojection check projects with K * pose.block<3,4>() of
 * KeyFrame::pose.pose (camera-to-world), not its inverse.  KeyFrame construction (initializeMono,
 * insertKeyFrameMono) and MapPoint insertion stay with the caller. */
typedef struct {
    vslam_rig rig;
    int32_t n_levels;
    const float* sigma_factor;         /* KeyFrame::sigmaFactor */
    int32_t n_kf;                      /* <= 16; keyframe 0 = lastKF */
    const double* kf_pose_wc;          /* [n_kf][16] KeyFrame::pose.pose, row-major */
    const int32_t* kf_id;              /* KeyFrame::numb */
    int32_t n_points;                  /* keypoints of lastKF */
    const int32_t* n_views;            /* [n_points] keyframeIdxMatchs[i].size() (lastKF itself first) */
    const int32_t* view_kf;            /* [n_points][n_kf] keyframe index of each view */
    const float* view_xy;              /* [n_points][n_kf][2] keypoint position in that keyframe */
    const int32_t* view_octave;        /* [n_points][n_kf] its octave */
} vslam_mono_points_problem;

typedef struct {
    uint8_t* accepted;                 /* out [n_points]: calculateMPFromMono returned true */
    double* xyz;                       /* out [n_points][3]: triangulated position (valid where accepted) */
    int32_t* n_obs;                    /* out [n_points]: views left after checkReprojError (n_views if it was not reached) */
    uint8_t* keep;                     /* out [n_points][n_kf]: view e survived checkReprojError */
} vslam_mono_points_result;

vslam_status vslam_mono_new_points(const vslam_mono_points_problem* problem, vslam_mono_points_result* result,
                                   int32_t device);

/* MapPoint::calcDescriptor (src/Map.cpp:145-210) for a batch of map points: descs = the observation
 * descriptors of all points concatenated (32 B each, in the order the caller iterates kFMatches),
 * start[n_mp + 1] = first descriptor of each point; best_out[m] = index (within the point) of the descriptor
 * with the least median Hamming distance to the others (first minimum), -1 for a point without observations.
 * At most 64 observations per point. */
vslam_status vslam_calc_descriptors(const uint8_t* descs, const int32_t* start, int32_t n_mp, int32_t device,
                                    int32_t* best_out);

/* ---------------------------------------------------------------------------
 * Per-frame tracking loop on device-resident state — the stereo path of
 * FeatureTracker::TrackImage (src/FeatureTracker.cpp:1108-1278):
 *   init_map : initializeMap (:72-123) — every stereo keypoint of the matcher's current frame
 *              (estimatedDepth > 0) becomes an active map point (position, descriptor,
 *              MapPoint::maxScaleDist), replacing the tracker's map-point set;
 *   track    : removeOutOfFrameMPs (:910-939) with the predicted pose, then the retry loop
 *              { matchByProjectionRPred(rad 10|120, +30) ; estimatePoseGTSAM } while inliers < 50
 *              (:1184-1233), PredictMPsPosition (:969-1014), the rad-4 refine match and the final
 *              pose solve (:1236-1241).  Needs a completed extraction + stereo match of the NEW
 *              frame; the map points come from earlier init_map / track calls.
 * Keyframe insertion, map growth and culling stay on the caller's side.
 * ------------------------------------------------------------------------- */
typedef struct vslam_track_report {
    int32_t n_map_points;     /* map points held by the tracker */
    int32_t n_active;         /* visible in both cameras under the predicted pose */
    int32_t rounds;           /* match+solve rounds before the refine pass */
    int32_t n_inliers;        /* pair returned by the last estimatePoseGTSAM */
    int32_t n_stereo;
    int32_t lm_iterations;    /* summed over all solves of this frame */
    float last_radius;
} vslam_track_report;

vslam_status vslam_tracker_init_map(vslam_matcher* m, const double* T_wc);
vslam_status vslam_tracker_track(vslam_matcher* m, const double* T_wc_pred, int32_t frame_number,
                                 double* T_cw_out, vslam_track_report* report);
/* the same loop in stereo + IMU mode (slamMode 0): every pose solve of the frame is the IMU branch */
vslam_status vslam_tracker_track_imu(vslam_matcher* m, const double* T_wc_pred, int32_t frame_number,
                                     const vslam_imu_input* imu, double* T_cw_out, vslam_imu_output* imu_out,
                                     vslam_track_report* report);
/* Mono + IMU frame (slamMode 2): the tracking block of FeatureTracker::TrackImageMonoIMU (src/FeatureTracker.cpp:
 * 1379-1450): PredictNextPoseIMU, removeOutOfFrameMPsMono, {matchByProjectionMono (rad 1200, +30 per retry),
 * estimatePoseGTSAMMono} rounds while inliers < 50.  T_wc_pred_out / pred_velocity_out = predNPose / predVelocity. */
vslam_status vslam_tracker_track_mono_imu(vslam_matcher* m, const vslam_imu_input* imu, const double* pred_velocity, double fps,
                                          double* T_cw_out, vslam_imu_output* imu_out, double* T_wc_pred_out,
                                          double* pred_velocity_out, vslam_track_report* report);
/* Replace the tracker's map with a flattened activeMapPoints list (position, descriptor, maxScaleDist, outlier
 * flag): mono initialisation, the new-point pipeline and replays feed the device-resident tracker through it. */
vslam_status vslam_tracker_set_map(vslam_matcher* m, const double* xyz, const uint8_t* desc, const float* max_scale_dist,
                                   const uint8_t* is_outlier, int32_t n);
/* copies of the per-frame tracking state for tests: matches (n_active x 2), MPsOutliers (n_active),
 * source map-point index of every active point */
vslam_status vslam_tracker_fetch(vslam_matcher* m, int32_t* matches, uint8_t* mps_outliers,
                                 int32_t* active_index, int32_t cap, int32_t* n_active);

/* ---------------------------------------------------------------------------
 * The closed loop behind one handle - what VSlamSystem wires together (include/System.h:28-35, src/System.cpp:6-85):
 *   vslam_system_track_stereo  = VSlamSystem::TrackStereo / TrackStereoIMU -> FeatureTracker::TrackImage
 *                                (include/FeatureTracker.h:87-96, src/FeatureTracker.cpp:1108-1278): changePosesLCA when a
 *                                local BA has finished, extraction + stereo match, removeOutOfFrameMPs, the match / pose
 *                                retry loop, refinement, the keyframe rule (:1262) with insertKeyFrame (:743-842) or
 *                                addFrame, updatePoses, setActiveOutliers;
 *   the optimizer thread       = LocalMapper::beginLocalMapping (include/OptimizationBA.h:54-87, src/OptimizationBA.cpp:
 *                                955-982): getConnectedKFs window, findNewPoints, localBA on THAT window, write-back,
 *                                LBADone hand-over.  local_mapping = 1 runs a pass to completion right after the frame
 *                                that inserted the keyframe; local_mapping = 2 runs its device work on a library thread
 *                                beside tracking, on ONE FIXED interleaving of the reference's two threads
 *                                (mapping_delay = k): for a pass handed over after frame f, findNewPoints has written
 *                                its points before frame f + 1 is tracked, localBA collects its window at that moment,
 *                                and its write-back + LBADone land at the beginning of frame f + k (TrackImage :1115-1122
 *                                then runs changePosesLCA).  Frames f + 1 .. f + k - 1 track against the map with the new
 *                                points but without the BA's result, as the reference's tracker does while the optimizer
 *                                thread is inside LevenbergMarquardt.  Runs are reproducible and equal the test-side
 *                                restatement of the same schedule frame by frame; 0 disables local mapping.
 * Map / KeyFrame / MapPoint live inside the handle (index-based records); every numerical stage is a kernel of this
 * library.  Images: u8, `stride` bytes per row, host pointers (on_device = 0) or device pointers (1).
 * ------------------------------------------------------------------------- */
typedef struct vslam_system vslam_system;

typedef struct vslam_system_config {
    vslam_fe_params fe;
    vslam_rig rig;
    int32_t device;
    int32_t use_imu;              /* 0: slamMode 1 (stereo), 1: slamMode 0 (stereo + IMU: the IMU branch of estimatePoseGTSAM) */
    int32_t local_mapping;        /* 0 off, 1 synchronous, 2 library thread, fixed schedule (mapping_delay) */
    int32_t window;               /* actvKFMaxSize (include/OptimizationBA.h:46); 0 = 10, at most 16 */
    double T_wc_init[16];         /* zedPtr->mCameraPose at start, row-major; all zero = identity (the reference) */
    /* IMU constants (Camera::mIMUGravity, IMUData noise terms, Camera::TBodyToCam, IMUData::mHz) */
    double gravity[3];
    double gyro_noise_density, gyro_random_walk, accel_noise_density, accel_random_walk;
    double T_body_sensor[16];
    int32_t imu_hz;
    double velocity_init[3];      /* Camera::mVelocity at start (zero in the reference) */
    int32_t mapping_delay;        /* local_mapping = 2 only: k of the schedule above (0 = 1).  The tracker waits at frame f + 1 for
                                     the new-point search and at frame f + k for the local BA if they have not finished; a pass
                                     that finishes early is held back until then.  At the reference's camera rate a pass ends
                                     within a frame or two, i.e. k = 1..2. */
    int32_t mapping_np_delay;     /* local_mapping = 2 only: a of the schedule (0 = 1, at most mapping_delay): findNewPoints reads the map
                                     right after frame f, its points are written (addNewMapPoints) before frame f + a is tracked, and
                                     localBA collects its window at that moment. */
} vslam_system_config;

/* the IMU samples between the previous frame and this one (IMUData filled in src/VIOSlam.cpp:238-272) */
typedef struct vslam_imu_bucket {
    int32_t n;
    const double* acceleration;       /* n x 3 */
    const double* angular_velocity;   /* n x 3 */
    const double* timestamps_ns;      /* n */
} vslam_imu_bucket;

typedef struct vslam_frame_report {
    int32_t frame, keyframe_inserted;
    int32_t n_active;                 /* activeMpsTemp.size() after removeOutOfFrameMPs */
    int32_t n_inliers, n_stereo;      /* pair returned by the frame's last estimatePoseGTSAM */
    int32_t rounds, lm_iterations;
    int32_t n_keyframes, n_map_points, n_active_after;
    /* local mapping that completed since the previous report (synchronous mode: the one this frame triggered) */
    int32_t mapping_ran, new_points, ba_keyframes, ba_local, ba_landmarks, ba_pairs, ba_wrong, ba_outliers;
    int32_t ba_residuals, ba_free_kf, ba_sum_k2, ba_trials;   /* work figures of that local BA (vslam_ba_result), lambda trials of both passes */
    int32_t ba_rounds;                /* trial rounds of both passes (vslam_ba_result::rounds) */
    vslam_lm_report ba_report[2];
} vslam_frame_report;

vslam_status vslam_system_create(const vslam_system_config* config, vslam_system** out);
void vslam_system_destroy(vslam_system* sys);
vslam_status vslam_system_track_stereo(vslam_system* sys, const uint8_t* left, const uint8_t* right, int32_t stride,
                                       int32_t on_device, int32_t frame_number, const vslam_imu_bucket* imu,
                                       double* T_wc_out, vslam_frame_report* report);
/* the same for colour frames: what VSlamSystem::TrackStereo / TrackStereoIMU receive from the reference's frame loop
 * (src/VIOSlam.cpp:289-311: imread IMREAD_COLOR, remap, Track*) and TrackImage converts (src/FeatureTracker.cpp:1130-1144).
 * channels = 3 (BGR) or 4 (BGRA): both images converted to gray on the device by one launch before extraction; channels = 1
 * is vslam_system_track_stereo.  stride >= width x channels, else VSLAM_ERR_INVALID with nothing tracked. */
vslam_status vslam_system_track_stereo_color(vslam_system* sys, const uint8_t* left, const uint8_t* right, int32_t stride,
                                             int32_t channels, int32_t on_device, int32_t frame_number, const vslam_imu_bucket* imu,
                                             double* T_wc_out, vslam_frame_report* report);
/* RAW (unrectified) frames: the whole per-frame part of the reference's loop (src/VIOSlam.cpp:278-311: remap through the
 * per-camera maps, cvtColor, Track*) in one call.  vslam_system_set_rectifiers binds the left and right camera's rectifier
 * (both non-NULL, or both NULL to unbind): output size = the rig's width x height, the session's device, equal source sizes,
 * else VSLAM_ERR_INVALID.  The session borrows them: a bound rectifier must outlive the session or be unbound first (no
 * reference counting).  vslam_system_track_stereo_raw then takes source-sized frames (channels 1 / 3 / 4, stride >=
 * src_width x channels): both images are rectified (and converted) on the way into pyramid level 0 by one launch; everything
 * after level 0, and every result, is that of vslam_rectifier_remap(_gray) followed by vslam_system_track_stereo.  Without
 * bound rectifiers, with other channels or a short stride: VSLAM_ERR_INVALID with nothing tracked. */
vslam_status vslam_system_set_rectifiers(vslam_system* sys, const vslam_rectifier* left, const vslam_rectifier* right);
vslam_status vslam_system_track_stereo_raw(vslam_system* sys, const uint8_t* left, const uint8_t* right, int32_t stride,
                                           int32_t channels, int32_t on_device, int32_t frame_number, const vslam_imu_bucket* imu,
                                           double* T_wc_out, vslam_frame_report* report);
/* Relocalisation of a stereo session (use_imu = 0; gray frames) from its own map, without a pose prior - for a session whose
 * tracking is lost (fewer than 50 inliers).  No reference counterpart.  The call does what a tracked frame does first
 * (mapping results due at frame_number land, extraction, stereo match), then runs vslam_relocalize over every map point not
 * flagged an outlier, in creation order (the most recent 65536 if there are more) - as one lane of the batched stages, what a
 * lane of vslam_batch_relocalize runs; params out of range are refused before anything is done.
 * Failure (report->success = 0, VSLAM_OK): nothing else in the session changes, T_wc_out = the unchanged camera pose.
 * Success: the camera pose is the result; the predicted motion is the identity (predNPose = camPose, predNPoseRef = I);
 * camRefPose = lastKFPoseInv * pose; the frame is recorded as addFrame records a non-keyframe frame; activeMapPoints
 * becomes, in creation order, every non-outlier map point that the left-camera test of vslam_world_to_frame (run on the
 * device with the stage, k_reloc_inframe_b) places inside the left image under the new pose (MapPoint::inFrame follows); the last frame's match tables are cleared; no keyframe is inserted, and the next
 * vslam_system_track_stereo proceeds normally.  IMU sessions (their velocity would need re-initialising:
 * vslam_system_relocalize_imu below is their call) and mono sessions: VSLAM_ERR_INVALID with nothing changed. */
vslam_status vslam_system_relocalize(vslam_system* sys, const uint8_t* left, const uint8_t* right, int32_t stride,
                                     int32_t on_device, int32_t frame_number, const vslam_reloc_params* params,
                                     double* T_wc_out, vslam_reloc_report* report);
/* Relocalisation of a stereo + IMU session (use_imu = 1; gray frames): the pose as vslam_system_relocalize recovers it, and
 * the velocity from TWO relocalised poses and the IMU bucket between them (restated by
 * tests/reloc_imu_ref.py).  The session keeps two more pieces of state: a pending flag, and biasGood - the copy of the bias
 * taken at the end of every tracked frame whose final n_inliers >= 50 (it starts as the bias starts).  Every call runs the
 * front end and steps A-D of vslam_system_relocalize (mode 0 or 1); what a success commits depends on the flag:
 *   phase 1 (flag clear): the commit of vslam_system_relocalize (identity predicted motion); velocity and bias stay
 *     untouched; the flag is set.  imu is ignored and may be NULL.  imu_report->phase = 1.
 *   phase 2 (flag set): imu = the bucket since the previous call (n >= 1).  With T_prev = the camera pose (phase 1's) and
 *     T_new = the rigid inverse (R^T, -R^T t) of the refined T_cw: the bucket is pre-integrated as a pose solve stages it
 *     (dt rule of vslam_imu_predict, dt0 = 1 / hz) with the integration bias biasGood, and predicted from (T_prev, v = 0,
 *     biasGood): pred.R, pred.t, pred.v, dt = deltaTij (the pre-integration's own sum of sample periods).  Then, in fp64,
 *       velocity_prev[i] = (t_new[i] - pred.t[i]) / dt        velocity[i] = pred.v[i] + velocity_prev[i]
 *       rot_residual = sqrt(sum_ij (pred.R_ij - R_new_ij)^2)   (row-major order; reported, nothing is gated on it)
 *     - the prediction is affine in the start velocity, so velocity_prev is the v0 whose prediction lands on t_new and
 *     velocity the v1 it implies.  The pose is committed as in phase 1 but with the predicted motion of updatePoses
 *     (predNPoseRef = camPoseInv_prev * pose, predNPose = pose * predNPoseRef); the session's velocity = velocity, bias =
 *     biasGood; the flag is cleared.  imu_report->phase = 2 and its other fields are filled (bias = biasGood).  The next
 *     vslam_system_track_stereo is an ordinary IMU frame.
 *   failure in either phase (report->success = 0, VSLAM_OK): the flag is cleared, nothing else changes, T_wc_out = the
 *     unchanged camera pose, imu_report->phase = 0.  Phase 2 thus only ever follows a successful phase 1 by exactly one call.
 * While the flag is set every vslam_system_track_stereo* form on the session (and a vslam_batch_track_stereo* step in which
 * the lane is active) returns VSLAM_ERR_INVALID with nothing changed: relocalise once more.
 * VSLAM_ERR_INVALID with nothing changed and nothing launched: a session without IMU or a mono session (use
 * vslam_system_relocalize), no map, phase 2 with imu NULL or n < 1.  A phase-2 bucket whose 15x15 covariance has no
 * Cholesky factor: VSLAM_ERR_INVALID (the condition of the IMU calls), the session is not changed. */
typedef struct vslam_reloc_imu_report {
    int32_t phase;            /* 0 failed, 1 pose committed / velocity pending, 2 velocity re-initialised */
    double dt, velocity_prev[3], velocity[3], bias[6], rot_residual;   /* phase 2 only */
} vslam_reloc_imu_report;
vslam_status vslam_system_relocalize_imu(vslam_system* sys, const uint8_t* left, const uint8_t* right, int32_t stride,
                                         int32_t on_device, int32_t frame_number, const vslam_imu_bucket* imu,
                                         const vslam_reloc_params* params, double* T_wc_out, vslam_reloc_report* report,
                                         vslam_reloc_imu_report* imu_report);
/* ---------------------------------------------------------------------------
 * Loop closing of a stereo session (use_imu = 0) - NO reference counterpart.  Both calls are
 * made BETWEEN tracked frames, e.g. after a frame whose report has keyframe_inserted.
 *
 * vslam_system_correct_loop: the caller states that the CURRENT camera really is at T_wc_corrected and that keyframe kf_loop
 * anchors that knowledge (from vslam_system_close_loop's detection, a fiducial, an external detector).  With the drift
 * D = T_wc_corrected * T_wc^-1 a pose graph over EVERY keyframe is solved by vslam_pose_graph_optimize (params->pgo):
 *   fixed         keyframe 0 and kf_loop
 *   sequential    (prevKF, kf) for every keyframe with a predecessor, in keyframe order; Z from the current poses, weights 1 / 1
 *   covisibility  every sortedKFWeights entry (weight, other) of keyframe k with weight >= covis_min and other != k, keyframes
 *                 in ascending order and entries in list order; an unordered pair enters once, as (min, max); Z from the
 *                 current poses, weights 1 / 1.  (A pair that is also sequential is a duplicate edge: they add up.)
 *   loop          (kf_loop, latestKF), Z = T_w,kfloop^-1 * D * T_w,latestKF, weights loop_weight / loop_weight
 * with Z of a pair (a, b) = poseInv(a) * pose(b).  The commit, on the caller's (the tracker's) timeline under the map's mutex:
 * every keyframe takes its new pose (setPose) and, with a predecessor, refPose = poseInv(prevKF) * pose; the camera pose,
 * lastKFPoseInv and the predicted pose follow the latest keyframe as changePosesLCA derives them (camPose = pose(latestKF) *
 * camRefPose, predNPose = camPose * predNPoseRef); plain frames of the trajectory follow through their keyframe.  Every map
 * point with at least one observation moves with its first observing keyframe kFMatches[0] by vslam_pose_graph_move_points
 * (outliers included).  activeMapPoints becomes, in creation order, every non-outlier map point (the most recent 65536) that
 * vslam_world_to_frame places inside the left image under the new camera pose; MapPoint::inFrame follows; the last frame's
 * match tables are cleared (the rule of vslam_system_relocalize's commit): the old copy of the place is handed back to the
 * tracker.  No keyframe is inserted, no frame is recorded.  A local BA that has finished but whose changePosesLCA has not
 * run yet (local_mapping = 1, right after a keyframe) is propagated first, as the next frame would.  Stored stereo depths of
 * the keyframes are not refreshed (the next local BA over a keyframe does that).
 * report->busy = 1, VSLAM_OK, nothing changed: a local-mapping pass is handed over and has not landed (local_mapping = 2,
 * between hand-over and frame f + k); the call neither waits for it nor cancels it - call again after a later frame.
 * VSLAM_ERR_INVALID, nothing changed: mono sessions, use_imu = 1 sessions (velocity and gravity frame would have to follow),
 * no tracked frame yet, kf_loop out of range or equal to the latest keyframe, a non-finite T_wc_corrected, negative
 * parameters.
 *
 * vslam_system_close_loop: detection on the frame the session's matcher still holds from the last
 * vslam_system_track_stereo, then - unless detect_only - the correction above.  Candidates: map points that are not outliers,
 * NOT in activeMapPoints, created by a keyframe (MapPoint::kdx) <= latestKF - min_kf_gap; in creation order, the most recent
 * 65536.  Fewer than reloc.min_inliers candidates: success = 0.  Otherwise steps A-D of vslam_relocalize (params->reloc,
 * either mode) over them.  On success kf_loop = the keyframe other than the latest that observes the most map points among the
 * inliers of the winning hypothesis (the set step D refines; the lowest keyframe number on a tie; none: success = 0), and
 * T_wc_corrected = the rigid inverse of the refined T_cw.  Step D's side effect on the matcher's stereo match does not reach
 * the session: the four stereo arrays are saved before and restored after the stage.  A call that finds no loop, is busy or is
 * detect_only leaves the session in a state from which the following frames track bit for bit as without the call.
 * Refusals as above.
 * ------------------------------------------------------------------------- */
typedef struct vslam_loop_params {    /* a zero field takes the default in brackets (NULL = all defaults) */
    vslam_reloc_params reloc;         /* detection (vslam_system_close_loop only) */
    vslam_pgo_params pgo;
    int32_t min_kf_gap;               /* [20]  a candidate's creating keyframe is at most latestKF - min_kf_gap */
    int32_t covis_min;                /* [100] covisibility edges from this weight */
    double loop_weight;               /* [10]  both parts of the loop edge */
    int32_t detect_only;              /* 1: vslam_system_close_loop stops after detection */
} vslam_loop_params;

typedef struct vslam_loop_report {
    int32_t busy;                     /* 1: a mapping pass is in flight, nothing was done */
    int32_t success;                  /* detection found a loop (vslam_system_correct_loop: 1 unless busy) */
    int32_t corrected;                /* the correction was committed */
    int32_t kf_loop, n_candidates;
    int32_t n_nodes, n_sequential, n_covisibility, n_edges;
    int32_t points_moved, n_active_after;
    double drift_translation, drift_rotation;     /* |t_D| in metres, rotation angle of D in radians */
    double T_wc_corrected[16];
    double T_wc[16];                  /* the camera pose after the call (the unchanged one when nothing was committed) */
    vslam_reloc_report reloc;
    vslam_pgo_report pgo;
} vslam_loop_report;

vslam_status vslam_system_correct_loop(vslam_system* sys, int32_t kf_loop, const double* T_wc_corrected,
                                       const vslam_loop_params* params, vslam_loop_report* report);
vslam_status vslam_system_close_loop(vslam_system* sys, const vslam_loop_params* params, vslam_loop_report* report);
/* Loop closing for stereo + IMU sessions (use_imu = 1): the two calls above with a YAW-ONLY
 * correction.  The world frame of such a session carries cfg.gravity, and roll and pitch are observable from the IMU, so a
 * correction may rotate keyframes only about g = gravity / |gravity| and translate them; the calls above keep refusing IMU
 * sessions.  Signatures, `busy`, detect_only, detection (candidates, the relocalisation stage with save / restore of the four
 * stereo arrays, the vote), graph, fixed set, edges, the move of the map points, commit and activation are those of the calls
 * above, with three differences:
 *   projection  the claimed pose is projected first.  D = T_wc_corrected * T_wc^-1, q = (R32 - R23, R13 - R31, R21 - R12) of R_D,
 *               theta = atan2(g . q, tr R_D - g^T R_D g): the rotation about g closest to R_D (it maximises tr(Exp(theta g)^T R_D)).
 *               T' = [Exp(theta g) R_cam | t_corrected]; the loop edge is built from D' = T' * T_wc^-1.  What the projection
 *               drops (the rotation between T' and the claim) is reported, never applied.
 *   solve       vslam_pose_graph_optimize_yaw with axis cfg.gravity.  A map point whose first observing keyframe comes back
 *               with unchanged bytes is not touched (a claim without yaw and translation changes nothing, bit for bit);
 *               points_moved counts the map points that did move.
 *   IMU state   after the commit, with dR = R_cam,new * R_cam,old^T (a rotation about g): velocity <- dR velocity and the
 *               prediction's velocity likewise.  bias, the last good bias and gravity are untouched (body-frame quantities,
 *               and g is the axis of dR); nothing else of a session's IMU state lives in the world frame.
 * vslam_loop_report keeps its meaning: drift and T_wc_corrected are those of the UNPROJECTED claim.
 * detect_only: the IMU report holds the projection of the found claim under the camera pose AS IT IS (nothing is propagated,
 * nothing changes).  The applying path first propagates a finished local BA (local_mapping = 2), which may move the camera pose:
 * a following vslam_system_correct_loop_imu on the same claim can then report a slightly different yaw and T_wc_projected.
 * VSLAM_ERR_INVALID, nothing changed: a mono session, a session with use_imu = 0 (it has the calls above), a pending two-phase
 * relocalisation (vslam_system_relocalize_imu has committed a pose but no velocity yet), and everything the calls above refuse. */
typedef struct vslam_loop_imu_report {
    double yaw;                       /* theta: the rotation about g that is applied to the camera [rad] */
    double tilt_dropped;              /* rotation angle between the projected pose T' and the claim [rad] */
    double T_wc_projected[16];        /* T' */
    double velocity_before[3], velocity[3];      /* world-frame velocity before / after the call */
} vslam_loop_imu_report;
vslam_status vslam_system_correct_loop_imu(vslam_system* sys, int32_t kf_loop, const double* T_wc_corrected,
                                           const vslam_loop_params* params, vslam_loop_report* report, vslam_loop_imu_report* imu_report);
vslam_status vslam_system_close_loop_imu(vslam_system* sys, const vslam_loop_params* params, vslam_loop_report* report,
                                         vslam_loop_imu_report* imu_report);
/* test taps: activeMapPoints (map-point indices, in order); every sortedKFWeights entry as (keyframe, other, weight) triples,
 * keyframes ascending, entries in list order; per map point its first observing keyframe (-1: none) and creating keyframe */
vslam_status vslam_system_active_points(vslam_system* sys, int32_t cap, int32_t* n_out, int32_t* index);
vslam_status vslam_system_covisibility(vslam_system* sys, int32_t cap, int32_t* n_out, int32_t* triples);
vslam_status vslam_system_map_point_keyframes(vslam_system* sys, int32_t cap, int32_t* n_out, int32_t* first_observer, int32_t* creator);

/* vslam_system_fuse_loop: the duplicate map points of a revisited place become one.  A call of its
 * own, made BETWEEN tracked frames, normally right after a vslam_system_close_loop / _correct_loop whose report has
 * corrected = 1: the map then holds every revisited landmark twice, one copy triangulated on the first visit, one since the
 * return, and nothing connects them.
 * Sets, over the map points that are not outliers, in creation order: B (kept) = created by a keyframe (MapPoint::kdx) <=
 * latestKF - min_kf_gap, A (absorbed) = created later; each the most recent 65536.  vslam_fuse_search pairs them under the
 * current camera (camPoseInv, the session's rig and image size): only what the camera sees is fused - the place being revisited.
 * The commit, on the caller's timeline under the map's mutex, pairs (a, b) in ascending a:
 *   for every observation o = (kf, l, r) of a, in kFMatches order:
 *     b is not observed by kf:  o is appended to b's kFMatches; localMapPoints[l] = b, unMatchedF[l] = b.kdx (l >= 0), likewise
 *                               localMapPointsR / unMatchedFR (r >= 0)                                       [an observation moved]
 *     otherwise:                the keyframe's connection to a is erased as KeyFrame::eraseMPConnection does (-1 in the same four
 *                               tables)                                                                    [an observation dropped]
 *   a's kFMatches is cleared, a becomes an outlier and leaves the frame (inFrame = 0); b.lastObsKF = max of the two.
 *   b's position, descriptor, scale distances, kdx and idx are untouched (the old copy hangs on the keyframes the solve held
 *   fixed or moved least); no descriptor is re-selected.
 * Every keyframe whose tables changed (n_keyframes_touched) gets calcConnections again, and so does every keyframe that observes
 * a kept point - its weights towards the keyframes the point was moved into have grown although its own tables stand - all in
 * ascending keyframe number: the next local BA window can span the loop, from either end.  activeMapPoints becomes the old list without the absorbed points, order kept, then the kept points not yet in
 * it in ascending index; every kept point's inFrame = 1.  Iff at least one pair was committed the last frame's match tables are
 * cleared (the rule of the loop correction's commit).  With zero pairs the call changes nothing: the following frames track bit
 * for bit as without it.  A finished local BA whose changePosesLCA has not run yet is propagated first, as the next frame would.
 * report->busy = 1, VSLAM_OK, nothing changed: as for the loop calls.  VSLAM_ERR_INVALID, nothing changed: mono sessions,
 * use_imu = 1 sessions, no tracked frame yet, a negative or non-finite parameter, depth_ratio inside (0, 1). */
typedef struct vslam_fuse_loop_params {   /* a zero field takes the default in brackets (NULL = all defaults) */
    vslam_fuse_params search;
    int32_t min_kf_gap;                   /* [20] */
} vslam_fuse_loop_params;

typedef struct vslam_fuse_loop_report {
    int32_t busy;                         /* 1: a mapping pass is in flight, nothing was done */
    int32_t n_a, n_b;                     /* sizes of the two sets */
    vslam_fuse_report search;
    int32_t n_fused;                      /* pairs committed (= search.n_pairs) */
    int32_t n_obs_moved, n_obs_dropped;
    int32_t n_keyframes_touched;
    int32_t n_active_after;
} vslam_fuse_loop_report;

vslam_status vslam_system_fuse_loop(vslam_system* sys, const vslam_fuse_loop_params* params, vslam_fuse_loop_report* report);
/* test taps: descriptors (n x 32 bytes) of every map point in creation order; the observations of every map point as
 * offsets [n + 1] into (keyframe, left index, right index) triples, kFMatches order (triples may be NULL: n_obs_out only);
 * localMapPoints / localMapPointsR of one keyframe as map-point indices (-1: none); the (absorbed, kept) map-point pairs of the
 * last vslam_system_fuse_loop call, ascending absorbed index */
vslam_status vslam_system_map_point_descriptors(vslam_system* sys, int32_t cap, int32_t* n_out, uint8_t* desc);
vslam_status vslam_system_map_point_observations(vslam_system* sys, int32_t cap_points, int32_t cap_obs, int32_t* n_out, int32_t* n_obs_out,
                                                 int32_t* offsets, int32_t* triples);
vslam_status vslam_system_keyframe_points(vslam_system* sys, int32_t kf, int32_t cap_l, int32_t cap_r, int32_t* n_l_out, int32_t* n_r_out,
                                          int32_t* lmp_l, int32_t* lmp_r);
vslam_status vslam_system_fused_pairs(vslam_system* sys, int32_t cap, int32_t* n_out, int32_t* pairs);

/* vslam_system_global_ba: one vslam_global_ba over the whole map of a stereo session - what makes
 * reprojection error, not relative-pose error, decide where the keyframes and the fused points of a closed loop end up.
 * Refusals (VSLAM_ERR_INVALID, nothing changed): mono and IMU sessions, with the messages of the loop calls; a negative or
 * non-finite parameter.  report->busy = 1, VSLAM_OK, nothing changed: a local_mapping = 2 session with a mapping pass in flight.
 * A session with fewer than two keyframes: success = 0, nothing changed.  Otherwise, under the map's lock:
 *   1 a finished local BA is propagated first, as the next frame would
 *   2 ALL keyframes are flattened: keyframe 0 and every `fixed` one are fixed, all are kf_local
 *   3 all non-outlier map points with the pair flags of the local BA's collection (left: 1, left + right of a `close` key: 3,
 *     right only: 2); a point that is out of frame with fewer than three observations carries no pair
 *     PARALLAX GUARD: a point whose observation rays (from the observing camera centres, the right camera's for a right factor,
 *     at the current values) never open wider than acos(0.9998) = 1.15 degrees gets flags 0 on all its pairs: its depth is not
 *     observable, one pass would walk it towards infinity.  It stays where it is, as a thin landmark does
 *   4 sequential edges (prevKF -> keyframe, the current relative pose) at weight edge_weight on rotation and translation; 0: none
 *   5 vslam_global_ba with `gba`
 *   6 commit, the local BA's write-back: wrong pairs are erased from the map point and from the keyframe's tables, poses of
 *     non-fixed keyframes and positions of present points are stored, a point flagged in 3 or left out of frame with fewer than
 *     three observations becomes an outlier, the depth / close refresh and the descriptor selection of the moved points are served
 *   7 refPose of every keyframe re-derived, the camera re-anchored on the latest keyframe, the active set rebuilt by
 *     relocalisation's rule (as vslam_system_correct_loop ends)
 * A refusal of vslam_global_ba (a free gauge, a point behind a keyframe) is returned as it is, with nothing changed.
 * Lanes of a vslam_batch have vslam_batch_global_ba (one batched solve for all of them); vslam_fleet lanes have neither yet.
 * Not called from vslam_system_close_loop or vslam_system_fuse_loop: the caller decides when. */
typedef struct vslam_system_gba_params {  /* a zero field takes the default in brackets (NULL = all defaults) */
    vslam_gba_params gba;
    double edge_weight;                   /* [0: no edges] */
} vslam_system_gba_params;

typedef struct vslam_system_gba_report {
    int32_t busy;                         /* 1: a mapping pass is in flight, nothing was done */
    int32_t success;                      /* 1: the solve ran and was committed */
    int32_t n_keyframes, n_landmarks, n_pairs, n_edges;      /* the flattened problem */
    int32_t n_wrong;                      /* pairs erased */
    int32_t n_outliers;                   /* map points that became outliers */
    int32_t n_active_after;
    int32_t reserved;
    vslam_gba_report gba;
} vslam_system_gba_report;

vslam_status vslam_system_global_ba(vslam_system* sys, const vslam_system_gba_params* params, vslam_system_gba_report* report);
/* test tap: the flattened problem the call would build now (steps 1 - 4; step 1 is carried out).  sizes [5] = n_kf, n_lm,
 * n_pairs, n_edges, n_levels, always written; with arrays == 0 nothing else is.  Otherwise every array is written, each at least
 * as long as its size says: kf_pose_wc [n_kf][16], kf_fixed, kf_local, lm_xyz [n_lm][3], lm_index [n_lm] (map-point index),
 * pair_kf, pair_lm, pair_flags, pair_uv [n_pairs][4], pair_octave [n_pairs][2], edges [n_edges], sigma_factor and
 * inv_sigma_factor [n_levels].  The same refusals as the call; busy: VSLAM_ERR_INVALID. */
vslam_status vslam_system_global_ba_problem(vslam_system* sys, double edge_weight, int32_t arrays, int32_t* sizes, double* kf_pose_wc,
                                            uint8_t* kf_fixed, uint8_t* kf_local, double* lm_xyz, int32_t* lm_index, int32_t* pair_kf,
                                            int32_t* pair_lm, uint8_t* pair_flags, float* pair_uv, int32_t* pair_octave,
                                            vslam_pgo_edge* edges, float* sigma_factor, float* inv_sigma_factor);
/* Duplicate fusion and the global adjustment for stereo + IMU sessions (use_imu = 1): what follows
 * a vslam_system_close_loop_imu / _correct_loop_imu whose report has corrected = 1.  vslam_system_fuse_loop,
 * vslam_system_global_ba and vslam_system_global_ba_problem keep refusing IMU sessions; the three calls below are refused
 * (VSLAM_ERR_INVALID, nothing changed) for a mono session, a session with use_imu = 0 (it has the calls above) and while a
 * two-phase relocalisation is pending, with the messages of the IMU loop calls, and for everything the calls above refuse.
 *   vslam_system_fuse_loop_imu      the stages, parameters, report and `busy` of vslam_system_fuse_loop, unchanged: fusion is
 *                                   geometry and bookkeeping.  Nothing of the IMU state is touched (velocity, bias, last good
 *                                   bias and the pending flag come back with the same bytes).
 *   vslam_system_global_ba_imu      steps 1 - 4 of vslam_system_global_ba, then vslam_global_ba_yaw with axis cfg.gravity in
 *                                   place of step 5, then steps 6 and 7: every keyframe moves only by a rotation about
 *                                   g = gravity / |gravity| and a translation, so R_new R_old^T g = g for each of them and for
 *                                   the camera, which is re-anchored on the latest keyframe.  The world-frame IMU state follows
 *                                   the camera as after a loop correction: with dR = R_cam,new * R_cam,old^T (R_cam,old the
 *                                   camera after step 1, as the loop calls take it) velocity <- dR velocity and the prediction's
 *                                   velocity likewise, before the active set is rebuilt.  bias, the last good bias, gravity and
 *                                   the pending flag are untouched.  `busy` and a session with fewer than two keyframes
 *                                   (success = 0, nothing changed, both velocities of the IMU report the session's) are those
 *                                   of vslam_system_global_ba.
 *   vslam_system_global_ba_problem_imu   the test tap of vslam_system_global_ba_problem on an IMU session. */
typedef struct vslam_gba_imu_report {
    double yaw;                       /* the camera's yaw: the twist of dR about g [rad] */
    double velocity_before[3], velocity[3];      /* world-frame velocity before / after the call */
    double T_wc[16];                  /* the camera pose after the call (the unchanged one when nothing was committed) */
} vslam_gba_imu_report;
vslam_status vslam_system_fuse_loop_imu(vslam_system* sys, const vslam_fuse_loop_params* params, vslam_fuse_loop_report* report);
vslam_status vslam_system_global_ba_imu(vslam_system* sys, const vslam_system_gba_params* params, vslam_system_gba_report* report,
                                        vslam_gba_imu_report* imu_report);
vslam_status vslam_system_global_ba_problem_imu(vslam_system* sys, double edge_weight, int32_t arrays, int32_t* sizes, double* kf_pose_wc,
                                                uint8_t* kf_fixed, uint8_t* kf_local, double* lm_xyz, int32_t* lm_index, int32_t* pair_kf,
                                                int32_t* pair_lm, uint8_t* pair_flags, float* pair_uv, int32_t* pair_octave,
                                                vslam_pgo_edge* edges, float* sigma_factor, float* inv_sigma_factor);
/* test tap: the IMU state of a session; any pointer may be NULL */
vslam_status vslam_system_imu_state(vslam_system* sys, double* velocity3, double* bias6, double* bias_good6, int32_t* pending);
/* test taps for the velocity rule alone, on a bare matcher: the bucket of imu is pre-integrated (k_imu_preintegrate_b) with
 * the integration bias imu->bias_prev and predicted from (imu->T_wc_prev, v = 0: imu->velocity_prev is not read), then
 * k_reloc_velocity_b applies the rule to the camera <- world pose T_cw_new[16].  out[8]: dt, velocity_prev[3], velocity[3],
 * rot_residual.  Errors as vslam_imu_preintegrate.  Invalidates the matcher's staged IMU bucket. */
vslam_status vslam_imu_reinit_velocity(vslam_matcher* m, const vslam_imu_input* imu, const double* T_cw_new, double* out);
/* the same for n_lanes buckets with ONE launch of k_imu_preintegrate_b and ONE of k_reloc_velocity_b; T_cw_new [n_lanes][16],
 * out [n_lanes][8].  A bucket with n_samples = 0 is an idle lane: its out row is left as the caller filled it. */
vslam_status vslam_imu_reinit_velocity_batch(vslam_matcher* m, int32_t n_lanes, const vslam_imu_input* imus,
                                             const double* T_cw_new, double* out);
/* blocks until the device work of the pass in flight (local_mapping = 2) has finished; reports its failure, if any.
 * (Its results are still applied at the frames the schedule names.) */
vslam_status vslam_system_wait_mapping(vslam_system* sys);
/* VSlamSystem::saveTrajectoryAndPosition (src/System.cpp:87-124) over the frames tracked so far */
vslam_status vslam_system_save_trajectory(vslam_system* sys, const char* path_trajectory, const char* path_positions);
/* test taps: sizes of the map; keyframe poses (world <- camera) and frame indices; matchesIdxs / MPsOutliers of the last frame */
vslam_status vslam_system_counts(vslam_system* sys, int32_t* n_keyframes, int32_t* n_map_points, int32_t* n_active,
                                 int32_t* n_frames);
vslam_status vslam_system_keyframes(vslam_system* sys, int32_t cap, int32_t* n_out, int32_t* frame_idx, double* poses_wc);
vslam_status vslam_system_last_frame(vslam_system* sys, int32_t cap, int32_t* n_out, int32_t* matches, uint8_t* mps_outliers);
/* test tap: world positions (n x 3) and outlier flags of every map point, in creation order */
vslam_status vslam_system_map_points(vslam_system* sys, int32_t cap, int32_t* n_out, double* xyz, uint8_t* is_outlier);
/* key slots of the session's keyframes in HBM: slots handed out so far, bytes of the slabs they are carved from */
vslam_status vslam_system_memory(vslam_system* sys, int32_t* key_slots_used, int64_t* key_slab_bytes);

/* ---------------------------------------------------------------------------
 * Mono + IMU session (slamMode 2): VSlamSystem::TrackMonoIMU -> FeatureTracker::TrackImageMonoIMU (src/System.cpp:82-85,
 * src/FeatureTracker.cpp:1280-1495) behind the same handle; no LocalMapper exists in this mode (src/System.cpp:11-20).
 * Per call, as the reference: PredictNextPoseIMU first (it advances predVelocity even on a refused call); until the map is
 * initialised the movement gate (Converter::checkSufficientMovement: translation >= 0.1f m AND rotation >= 5 degrees between
 * the camera pose and the prediction) refuses the call before anything is extracted; the first three accepted calls insert a
 * keyframe at the predicted pose; the fourth inserts one, matches the FIRST keyframe by radius (120) into the other three on
 * one claim table (vslam_match_by_radius_window) and triangulates the initial map (vslam_mono_new_points); every later call
 * is tracked (vslam_tracker_track_mono_imu's block) and inserts a keyframe - the reference's keyframe rule is always true
 * here - whose window is empty, so the map only shrinks.
 * The claim table of the initialisation has max(current frame's keys, largest target) entries, all -1 (the reference sizes
 * it by the current frame and reads past its end for a larger target).
 * HBM: only keyframes that a later device step can read take a key slot - the bootstrap keyframes and the initialising one.
 * Keyframes inserted by tracked calls keep their host keys only: nothing on the device ever reads them.
 * ------------------------------------------------------------------------- */
typedef struct vslam_mono_frame_report {
    int32_t frame;
    int32_t state;            /* 0 refused by the movement gate, 1 bootstrap keyframe, 2 initialised by this call, 3 tracked */
    int32_t keyframe_inserted;
    int32_t n_active, n_inliers, rounds, lm_iterations;   /* state 3: as vslam_track_report */
    float   last_radius;
    int32_t new_points;       /* map points this call created */
    int32_t radius_matches;   /* state 2: summed matchByRadius matches over the targets */
    int32_t n_keyframes, n_map_points, n_active_after;
} vslam_mono_frame_report;

/* config->use_imu must be 1 and local_mapping 0, fps (zedPtr->mFps) > 0, else VSLAM_ERR_INVALID; rig.baseline is ignored.
 * The session owns a batch-1 extractor and a mono matcher. */
vslam_status vslam_system_create_mono(const vslam_system_config* config, double fps, vslam_system** out);
/* channels 1 / 3 / 4 (gray, BGR, BGRA: the extractor's gray / colour load), stride >= width x channels.  imu: the bucket since
 * the previous call, non-NULL with n >= 1, else VSLAM_ERR_INVALID with nothing changed.  A refused call extracts nothing and
 * returns the unchanged camera pose (state 0).  The stereo entry points on a mono session and this one on a stereo session
 * return VSLAM_ERR_INVALID with nothing changed.  vslam_system_counts / _keyframes / _last_frame / _save_trajectory work as
 * for a stereo session; n_frames counts accepted calls only. */
vslam_status vslam_system_track_mono_imu(vslam_system* sys, const uint8_t* left, int32_t stride, int32_t channels,
                                         int32_t on_device, int32_t frame_number, const vslam_imu_bucket* imu,
                                         double* T_wc_out, vslam_mono_frame_report* report);

/* per-kernel-group HIP-event timing of a session: extraction and tracking groups of the LAST frame, local-BA groups summed
 * over the ba_calls local BAs that completed since the previous read */
vslam_status vslam_system_set_timing(vslam_system* sys, int32_t on);
vslam_status vslam_system_timings(vslam_system* sys, const char** names, float* ms, int32_t cap, int32_t* n_out, int32_t* ba_calls_out);
/* the local-BA part alone (a vslam_batch lane: the extraction / tracking timers belong to the batch) */
vslam_status vslam_system_set_ba_timing(vslam_system* sys, int32_t on);
vslam_status vslam_system_ba_timings(vslam_system* sys, const char** names, float* ms, int32_t cap, int32_t* n_out, int32_t* ba_calls_out);

/* ---------------------------------------------------------------------------
 * vslam_batch - B independent sequences ("lanes") tracked in lockstep: every stage of FeatureTracker::TrackImage
 * (src/FeatureTracker.cpp:1108-1278) is ONE kernel launch for all lanes (lane = a grid dimension, arguments from a
 * per-lane table), because one sequence's frame is a chain of mostly one-workgroup kernels that cannot fill the GPU.
 * Each lane is a complete vslam_system (own map, keyframes, local mapping); its results are identical to the same
 * sequence run through vslam_system_track_stereo.  Local mapping of the lanes runs on `mapping_threads` library threads
 * (local_mapping = 2) or inside the step (1).
 * A lane is one robot.  Shared by all lanes of a batch (checked by vslam_batch_create and vslam_batch_restart_lane): device,
 * image size (rig.width x rig.height), extractor parameters (fe), IMU mode, mapping mode and mapping_delay /
 * mapping_np_delay - the extractor, the streams and the schedule are shared objects.  Per lane: the camera behind the
 * images (rig.fx, fy, cx, cy, baseline - with the lane's rectifiers for raw frames), T_wc_init, velocity_init, the IMU
 * constants, and the session's life: frame number 0 starts it, vslam_batch_restart_lane ends it and starts the next.
 * ------------------------------------------------------------------------- */
typedef struct vslam_batch vslam_batch;
/* host_threads: threads for the per-lane host phases (< 0: min(lanes, 8)); mapping_threads: <= 0: min(lanes, 3) */
vslam_status vslam_batch_create(const vslam_system_config* configs, int32_t lanes, int32_t host_threads, int32_t mapping_threads,
                                vslam_batch** out);
void vslam_batch_destroy(vslam_batch* batch);
/* one frame per lane.  left / right: [lanes] image pointers; frame_numbers: [lanes] (0 initialises that lane's map);
 * imu: [lanes] buckets (IMU mode, frames > 0) or NULL; lane_mask: [lanes] 0 = lane idle this step, NULL = all lanes;
 * T_wc_out: [lanes][16]; reports: [lanes] or NULL */
vslam_status vslam_batch_track_stereo(vslam_batch* batch, const uint8_t* const* left, const uint8_t* const* right, int32_t stride,
                                      int32_t on_device, const int32_t* frame_numbers, const vslam_imu_bucket* imu,
                                      const uint8_t* lane_mask, double* T_wc_out, vslam_frame_report* reports);
/* local-BA stage timing of the batch's mapping engine (local_mapping = 2: the cohorts' batched local BAs): switch, and
 * read-and-reset of the per-group sums ("<group>#n" entries: launches behind a sum), the cohorts and the lanes they served */
vslam_status vslam_batch_set_ba_timing(vslam_batch* batch, int32_t on);
vslam_status vslam_batch_ba_timings(vslam_batch* batch, const char** names, float* ms, int32_t cap, int32_t* n_out,
                                    int64_t* cohorts_out, int64_t* lanes_out);
/* the same for DEVICE images, and the images of the NEXT step (next_left / next_right / next_mask, may be NULL): their
 * extraction is enqueued as soon as this step's kernels have finished, so that it runs under this step's host phases; the
 * next call must then pass exactly those pointers (anything else is extracted afresh) */
vslam_status vslam_batch_track_stereo_prefetch(vslam_batch* batch, const uint8_t* const* left, const uint8_t* const* right, int32_t stride,
                                               const int32_t* frame_numbers, const vslam_imu_bucket* imu, const uint8_t* lane_mask,
                                               double* T_wc_out, vslam_frame_report* reports, const uint8_t* const* next_left,
                                               const uint8_t* const* next_right, const uint8_t* next_mask);
/* the two entry points above for colour frames (channels = 3 BGR / 4 BGRA, after stride; 1 = the gray entry points):
 * every active lane's pair converted to gray by one launch (host images: all lanes' uploads, one wait, one launch).  A
 * prefetch is used by the next call only if it passes exactly those pointers with the same channels. */
vslam_status vslam_batch_track_stereo_color(vslam_batch* batch, const uint8_t* const* left, const uint8_t* const* right, int32_t stride,
                                            int32_t channels, int32_t on_device, const int32_t* frame_numbers, const vslam_imu_bucket* imu,
                                            const uint8_t* lane_mask, double* T_wc_out, vslam_frame_report* reports);
vslam_status vslam_batch_track_stereo_prefetch_color(vslam_batch* batch, const uint8_t* const* left, const uint8_t* const* right,
                                                     int32_t stride, int32_t channels, const int32_t* frame_numbers,
                                                     const vslam_imu_bucket* imu, const uint8_t* lane_mask, double* T_wc_out,
                                                     vslam_frame_report* reports, const uint8_t* const* next_left,
                                                     const uint8_t* const* next_right, const uint8_t* next_mask);
/* the same for RAW (unrectified) frames.  vslam_batch_set_rectifiers binds lane `lane`'s cameras (-1 = every lane; the
 * rules and the lifetime of vslam_system_set_rectifiers; lanes may have different cameras), the _raw calls take the
 * parameter lists of the _color forms with source-sized frames: every active lane's pair is rectified (and converted)
 * through its own maps by ONE launch into level 0 - with device sources no host wait, no rectified image in HBM.  The
 * prefetch form loads the next step's raw frames the same way.  Every lane that is active in the step (or the prefetched
 * one) must have rectifiers bound; binding discards a pending prefetch. */
vslam_status vslam_batch_set_rectifiers(vslam_batch* batch, int32_t lane, const vslam_rectifier* left, const vslam_rectifier* right);
vslam_status vslam_batch_track_stereo_raw(vslam_batch* batch, const uint8_t* const* left, const uint8_t* const* right, int32_t stride,
                                          int32_t channels, int32_t on_device, const int32_t* frame_numbers, const vslam_imu_bucket* imu,
                                          const uint8_t* lane_mask, double* T_wc_out, vslam_frame_report* reports);
vslam_status vslam_batch_track_stereo_prefetch_raw(vslam_batch* batch, const uint8_t* const* left, const uint8_t* const* right,
                                                   int32_t stride, int32_t channels, const int32_t* frame_numbers,
                                                   const vslam_imu_bucket* imu, const uint8_t* lane_mask, double* T_wc_out,
                                                   vslam_frame_report* reports, const uint8_t* const* next_left,
                                                   const uint8_t* const* next_right, const uint8_t* next_mask);
/* Ends lane `lane`'s session and starts a new one in its place: new map, keyframes, trajectory, tracker state, IMU state.
 * config: the new session's configuration (NULL = the lane's previous one).  Same shared fields as vslam_batch_create
 * (device, width x height, fe, IMU mode, mapping mode / delays), else VSLAM_ERR_INVALID and the lane is left as it was;
 * rig intrinsics / baseline, T_wc_init, velocity_init and the IMU constants may differ.
 * Waits for THIS lane's mapping job in flight (its result is discarded); other lanes, their maps and their jobs are not
 * touched.  Discards a pending prefetch (as vslam_batch_set_rectifiers does) and unbinds the lane's rectifiers.  The
 * lane's next frame must carry frame_number 0.  A vslam_system* from vslam_batch_system(lane) is invalid afterwards.
 * Call it between two steps, on the thread that drives the batch.  A restart allocates and frees nothing on the device
 * (no hipFree / hipHostFree: they would wait for the kernels of every group on the device): the new session takes over
 * the lane's matcher buffers, and the old session's key slabs (HBM) go to a free list of the batch, from which the
 * sessions of all lanes take before new memory is allocated; vslam_batch_destroy frees it. */
vslam_status vslam_batch_restart_lane(vslam_batch* batch, int32_t lane, const vslam_system_config* config);
/* Relocalisation of the lanes in lane_mask (NULL = all) from their own maps, in lockstep: for every such lane exactly what
 * vslam_system_relocalize does for that session - mapping results due at frame_numbers[lane] land as in a tracked step, one
 * extraction enqueue and one stereo launch set for all of them, the lane's non-outlier map points (creation order, the most
 * recent 65536) gathered straight into the batch's pinned upload block, then the stages of vslam_relocalize_batch and
 * k_reloc_inframe_b (the left-image test of every uploaded map point under the refined pose, for lanes that succeeded), one
 * wait, one download.  Success and failure are committed per lane as vslam_system_relocalize commits them: on failure
 * (reports[lane].success = 0) nothing in that session changes and its T_wc_out row is the unchanged camera pose.
 * Gray, rectified frames; stereo lanes without IMU (an IMU batch: vslam_batch_relocalize_imu below).  Lanes outside the mask are not touched: session, matcher state,
 * mapping jobs in flight, T_wc_out row and report stay as they are.  VSLAM_ERR_INVALID, with a message that names the lane
 * and nothing changed: an IMU batch, a masked lane without a map (also a restarted lane whose frame 0 has not been tracked),
 * NULL images for a masked lane.  A pending prefetch is waited for and discarded (as vslam_batch_restart_lane does): the
 * next step extracts its frames itself.  With timing on, the stages show in vslam_batch_timings as reloc_match,
 * reloc_pairs, reloc_ransac, reloc_refine, reloc_inframe.  No device memory is allocated or freed in a steady-state call
 * (a lane's relocalisation buffers are allocated at its first use; the blocks grow as a step's do).
 * Intended use: the lanes that tracked go through vslam_batch_track_stereo with the lost lanes masked out, the lost lanes
 * through this call with the same frame numbers. */
vslam_status vslam_batch_relocalize(vslam_batch* batch, const uint8_t* const* left, const uint8_t* const* right, int32_t stride,
                                    int32_t on_device, const int32_t* frame_numbers, const uint8_t* lane_mask,
                                    const vslam_reloc_params* params, double* T_wc_out /* [lanes][16] */,
                                    vslam_reloc_report* reports /* [lanes] */);
/* The same call for a stereo + IMU batch: per masked lane what vslam_system_relocalize_imu does for that session, in the shape
 * of vslam_batch_relocalize - one launch per stage for all lanes, one pinned upload (the phase-2 lanes' IMU samples travel in
 * it), one wait, one download.  A call may hold lanes in both phases: the phase-2 lanes' buckets are pre-integrated by one
 * k_imu_preintegrate_b launch ahead of the relocalisation stages (phase-1 lanes are idle entries), and k_reloc_velocity_b
 * applies the velocity rule to the lanes whose refinement succeeded.  imu: [lanes] buckets, read for the masked lanes whose
 * flag is set; NULL if no masked lane is in phase 2.  imu_reports: [lanes], written for the masked lanes.
 * VSLAM_ERR_INVALID with a message that names the lane, nothing changed and nothing launched: a batch without IMU (use
 * vslam_batch_relocalize), a masked lane without a map, NULL images for a masked lane, a masked phase-2 lane without a bucket
 * or with n < 1.  A phase-2 bucket whose covariance has no Cholesky factor: VSLAM_ERR_INVALID naming the lane, no session is
 * changed by the call. */
vslam_status vslam_batch_relocalize_imu(vslam_batch* batch, const uint8_t* const* left, const uint8_t* const* right, int32_t stride,
                                        int32_t on_device, const int32_t* frame_numbers, const vslam_imu_bucket* imu /* [lanes] or NULL */,
                                        const uint8_t* lane_mask, const vslam_reloc_params* params, double* T_wc_out /* [lanes][16] */,
                                        vslam_reloc_report* reports /* [lanes] */, vslam_reloc_imu_report* imu_reports /* [lanes] */);
/* vslam_relocalize_debug on lane `lane`'s matcher: its part of the last vslam_batch_relocalize call (test tap) */
vslam_status vslam_batch_relocalize_debug(vslam_batch* batch, int32_t lane, int32_t* d1_i1_d2, int32_t cap_points, int32_t* key_winner,
                                          int32_t cap_keys, int32_t* hyp_counts, int32_t cap_hypotheses, uint8_t* inlier_flags,
                                          int32_t cap_pairs, int32_t* sizes4);
/* Loop closing of the lanes in lane_mask, between two vslam_batch_track_stereo calls: a masked lane gets what
 * vslam_system_close_loop / vslam_system_correct_loop does to a session - candidates, detection, kf_loop vote, graph, commit,
 * active set, busy, detect_only and every report field by the same rules - in the batch's
 * shape:
 *   detection   the batched relocalisation stage (one launch per stage) over the masked lanes that are not busy and have at least
 *               reloc.min_inliers candidates; each lane's four stereo arrays are saved before and restored after it
 *   correction  every lane that reaches it builds its graph (a finished local BA is propagated first), then ONE
 *               vslam_pose_graph_optimize_batch and ONE k_pgo_move_points_b launch for all of them, then the commit and the
 *               active set per lane.  If no lane reaches the solve, nothing is launched for it.
 * A lane's outcome does not depend on the other lanes: a busy lane reports busy = 1 and is untouched, a lane that finds nothing
 * reports success = 0 and is untouched, while the others proceed.  Lanes outside the mask are not touched: session, matcher
 * state, report entry.  reports [lanes]: written for the masked lanes.  vslam_batch_correct_loop reads kf_loop [lanes] and
 * T_wc_corrected [lanes][16] for the masked lanes.
 * VSLAM_ERR_INVALID with a message that names the lane, nothing changed in any lane: an IMU batch; a masked lane without a
 * tracked frame (also a restarted lane) or, for vslam_batch_close_loop, whose matcher holds no frame (also: a prefetched
 * extraction is in flight); for vslam_batch_correct_loop a masked lane's kf_loop out of range or the latest keyframe, or a
 * non-finite pose; negative parameters; a NULL mask or reports. */
vslam_status vslam_batch_correct_loop(vslam_batch* batch, const uint8_t* lane_mask, const int32_t* kf_loop /* [lanes] */,
                                      const double* T_wc_corrected /* [lanes][16] */, const vslam_loop_params* params,
                                      vslam_loop_report* reports /* [lanes] */);
vslam_status vslam_batch_close_loop(vslam_batch* batch, const uint8_t* lane_mask, const vslam_loop_params* params,
                                    vslam_loop_report* reports /* [lanes] */);
/* The same two calls for the lanes of an IMU batch (use_imu = 1): a masked lane gets what vslam_system_close_loop_imu /
 * vslam_system_correct_loop_imu does to a session (projection about the lane's own gravity, yaw-only solve, velocity rotated with
 * the camera), in the shape above: the detection batched as above, every lane that reaches the
 * correction builds its graph on its projected claim, then ONE vslam_pose_graph_optimize_yaw_batch (each lane with its own axis
 * cfg.gravity) and ONE k_pgo_move_points_b launch for all of them, then the commit per lane.  A lane's outcome is what a session
 * driven alone gets.  imu_reports [lanes]: written for the masked lanes, like reports.
 * VSLAM_ERR_INVALID, nothing changed in any lane: a batch without IMU (it has the calls above), a masked lane with a pending
 * two-phase relocalisation, NULL imu_reports, and everything the calls above refuse (they keep refusing IMU batches). */
vslam_status vslam_batch_correct_loop_imu(vslam_batch* batch, const uint8_t* lane_mask, const int32_t* kf_loop /* [lanes] */,
                                          const double* T_wc_corrected /* [lanes][16] */, const vslam_loop_params* params,
                                          vslam_loop_report* reports /* [lanes] */, vslam_loop_imu_report* imu_reports /* [lanes] */);
vslam_status vslam_batch_close_loop_imu(vslam_batch* batch, const uint8_t* lane_mask, const vslam_loop_params* params,
                                        vslam_loop_report* reports /* [lanes] */, vslam_loop_imu_report* imu_reports /* [lanes] */);
/* The two calls that finish a lane's loop closing, between two steps, in the shape of vslam_batch_close_loop: per masked lane what
 * vslam_system_fuse_loop, respectively vslam_system_global_ba, does to a session (their rules, reports and defaults), with the
 * device work of all lanes in ONE batched call.
 *   vslam_batch_fuse_loop  every masked lane's sets and upload arrays (its map locked from here to its commit), ONE
 *                          vslam_fuse_search_batch call for all lanes that reach it, the commits.  vslam_system_fused_pairs on
 *                          vslam_batch_system(lane) gives a lane's committed pairs.
 *   vslam_batch_global_ba  every masked lane's flattened problem (its map locked from here to its commit; each lane with its own
 *                          rig), ONE vslam_global_ba_batch call for all lanes that reach it - the lanes' factorisations run side by
 *                          side - then per lane the commit, the refresh request, every refPose, the camera and the active set.
 * A lane's outcome does not depend on the other lanes: a busy lane reports busy = 1 and is untouched; a lane with fewer than two
 * keyframes reports as the session call does (fuse: no old set, nothing fused; global BA: success = 0).  Lanes outside the mask are
 * not touched: session, matcher state, report entry.  reports [lanes]: written for the masked lanes.
 * VSLAM_ERR_INVALID, nothing changed in any lane: a NULL mask or reports; an IMU batch; a negative or non-finite parameter
 * (depth_ratio inside (0, 1)); a masked lane without a tracked frame (also a restarted lane; the message names the lane).  A
 * refusal of the batched solve for any lane (a free gauge, a point behind its keyframe, a capacity limit) is returned as it is,
 * its message naming the lane among those that reached the solve, with no lane changed.
 * Neither is called from vslam_batch_close_loop: the caller decides when. */
vslam_status vslam_batch_fuse_loop(vslam_batch* batch, const uint8_t* lane_mask, const vslam_fuse_loop_params* params,
                                   vslam_fuse_loop_report* reports /* [lanes] */);
vslam_status vslam_batch_global_ba(vslam_batch* batch, const uint8_t* lane_mask, const vslam_system_gba_params* params,
                                   vslam_system_gba_report* reports /* [lanes] */);
/* key slabs the batch has allocated in total (bytes), and how many of them sessions hold / the free list holds; any
 * pointer may be NULL */
vslam_status vslam_batch_memory(vslam_batch* batch, int64_t* key_slab_bytes, int32_t* slabs_in_use, int32_t* slabs_free);
/* a lane's session (borrowed: valid until vslam_batch_destroy or the lane's restart) for the vslam_system_* read-outs */
vslam_system* vslam_batch_system(vslam_batch* batch, int32_t lane);
int32_t vslam_batch_lanes(const vslam_batch* batch);
vslam_status vslam_batch_wait_mapping(vslam_batch* batch);
/* HIP-event timing of the batched launches (device milliseconds per stage for ALL lanes, summed since the last read) and
 * the host-side phases of the last step in seconds: {begin, images + extraction enqueue, upload block, tables + enqueue,
 * wait, retry, post} */
vslam_status vslam_batch_set_timing(vslam_batch* batch, int32_t on);
vslam_status vslam_batch_timings(vslam_batch* batch, const char** names, float* ms, int32_t cap, int32_t* n_out, double* host_phases7);

/* ---------------------------------------------------------------------------
 * vslam_fleet - the frame driver inside the library: S independent sessions (vslam_system each: own rig / sequence, map,
 * tracker, optimizer thread) on S host threads sharing one GPU.  Replaces the frame loop of the reference's main()
 * (src/VIOSlam.cpp:289-316) for throughput runs: the path has no cross-sequence exchange, sessions are
 * the unit that fills the chip.  The sequence is a set of stereo pairs resident in HBM (on_device = 1) or in host memory
 * (0: every frame pays its host-to-device copy inside the step); a session replays it as a ping-pong (0..n-1, n-2..0, ...),
 * i.e. one continuous camera motion of any length - map, keyframes and local BAs are the tracker's own.
 * ------------------------------------------------------------------------- */
typedef struct vslam_fleet vslam_fleet;

typedef struct vslam_fleet_sequence {
    int32_t n_frames;
    const void* const* left;              /* n_frames image pointers (u8, `stride` bytes per row) */
    const void* const* right;
    int32_t stride;
    int32_t on_device;
    const vslam_imu_bucket* imu_forward;  /* [n_frames] samples between frame i-1 and i (entry 0 unused); IMU mode only */
    const vslam_imu_bucket* imu_backward; /* [n_frames] samples of the reversed motion from frame i+1 to i (last unused) */
    const double* T_wc_true;              /* [n_frames][16] ground-truth poses: a session starts at the pose of its first frame;
                                             the run reports the position error against them (may be NULL without IMU) */
    const double* velocity_true;          /* [n_frames][3] forward-motion velocity at each frame (IMU mode start value; may be NULL) */
    int32_t start_span;                   /* session s starts at frame (5 s) mod start_span (0: n_frames - 1).  With start_span + the
                                             frames a run tracks <= n_frames no session turns around: it never revisits a place */
} vslam_fleet_sequence;

typedef struct vslam_fleet_report {
    int32_t n_sessions;
    int64_t frames, keyframes, mappings, new_points, ba_landmarks, ba_pairs;   /* summed over sessions */
    int64_t ba_residuals, ba_free_kf, ba_sum_k2, ba_trials, ba_iterations, ba_rounds;
    int64_t sum_inliers, sum_rounds, lost_frames;                               /* lost: fewer than 50 inliers after the frame */
    int64_t sum_active;                                                         /* active map points after removeOutOfFrameMPs, summed over frames */
    int32_t min_inliers;
    double seconds, max_session_seconds;
    double max_position_error, sum_sq_position_error;                           /* against T_wc_true */
} vslam_fleet_report;

vslam_status vslam_fleet_create(const vslam_system_config* config, int32_t n_sessions, const vslam_fleet_sequence* sequence,
                                vslam_fleet** out);
/* the same sessions as the lanes of ceil(n_sessions / lanes_per_group) lockstep groups (vslam_batch), one driver thread each
   (1 <= n_sessions <= 1024; bench.py: 384 sessions in three groups of 128 per GPU) */
vslam_status vslam_fleet_create_batched(const vslam_system_config* config, int32_t n_sessions, const vslam_fleet_sequence* sequence,
                                        int32_t lanes_per_group, vslam_fleet** out);
void vslam_fleet_destroy(vslam_fleet* fleet);
/* every session tracks its next n_steps frames; returns when all of them - and every local BA they triggered - are done */
vslam_status vslam_fleet_run(vslam_fleet* fleet, int32_t n_steps, vslam_fleet_report* report);
vslam_status vslam_fleet_system(vslam_fleet* fleet, int32_t session, vslam_system** out);
/* HIP-event timing of session 0 on every `every`-th frame (0 = off; two event records per launch are a real cost on this
 * launch-bound path); timings: per kernel group the device milliseconds summed over the sampled frames ("<group>#n" entries:
 * the launches behind a local-BA sum), counts4 = {sampled frames, pose solves in them, local BAs (lanes) timed, the batched
 * calls (cohorts) that served them}; read-and-reset */
vslam_status vslam_fleet_set_sampling(vslam_fleet* fleet, int32_t every);
vslam_status vslam_fleet_timings(vslam_fleet* fleet, const char** names, float* ms, int32_t cap, int32_t* n_out, int64_t* counts4);

/* ---------------------------------------------------------------------------
 * N3 - the step before the hot path in the reference's frame loop (src/VIOSlam.cpp:278-306) and the dataset bookkeeping
 * of its main() (:23-139, 176-272).
 * vslam_rectifier: cv::initUndistortRectifyMap(K, D, R, P[0:3,0:3], size, CV_32F) once, then cv::remap(INTER_LINEAR,
 * BORDER_CONSTANT 0) of n gray images per launch.  K, R, P_new: 3x3 row-major (R NULL = identity); D: n_dist of
 * (k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4).  OpenCV's published fixed-point semantics; parity against OpenCV itself unpinned.
 * The calls below are a stage of their own (own stream, synchronous, rectified images in the caller's buffers); the
 * closed-loop handles rectify inside their level-0 load instead (vslam_*_set_rectifiers, the *_raw entry points).
 * ------------------------------------------------------------------------- */
vslam_status vslam_rectifier_create(const double* K, const double* D, int32_t n_dist, const double* R, const double* P_new,
                                    int32_t src_width, int32_t src_height, int32_t width, int32_t height, int32_t device,
                                    vslam_rectifier** out);
void vslam_rectifier_destroy(vslam_rectifier* r);
vslam_status vslam_rectifier_maps(vslam_rectifier* r, float* map_x, float* map_y);           /* test tap: the CV_32F maps */
/* src / dst: n DEVICE image pointers each (u8, strides in bytes); synchronous */
vslam_status vslam_rectifier_remap(vslam_rectifier* r, const uint8_t* const* src, int32_t src_stride, uint8_t* const* dst,
                                   int32_t dst_stride, int32_t n);
/* the same with HOST images (upload, one launch, download) */
vslam_status vslam_rectifier_remap_host(vslam_rectifier* r, const uint8_t* const* src, int32_t src_stride, uint8_t* const* dst,
                                        int32_t dst_stride, int32_t n);
/* colour images, as the reference remaps them (src/VIOSlam.cpp:296-297: cv::remap of the 3-channel imread image, cvtColor
 * afterwards in TrackImage, src/FeatureTracker.cpp:1130-1144): remap each channel of BGR (channels = 3) / BGRA (4) sources
 * (src_stride >= src_width x channels), round it, then convert to gray, in one pass; dst: gray (dst_stride >= width).
 * channels = 1 is vslam_rectifier_remap / _remap_host.  Device and host forms; synchronous. */
vslam_status vslam_rectifier_remap_gray(vslam_rectifier* r, const uint8_t* const* src, int32_t src_stride, int32_t channels,
                                        uint8_t* const* dst, int32_t dst_stride, int32_t n);
vslam_status vslam_rectifier_remap_gray_host(vslam_rectifier* r, const uint8_t* const* src, int32_t src_stride, int32_t channels,
                                             uint8_t* const* dst, int32_t dst_stride, int32_t n);

/* vslam_dataset: EuRoC (kind 0: <images_path>cam0/data.csv + cam0/data/, cam1/data/) or KITTI (kind 1: image_0/, image_1/,
 * names by .png count); imu_path: directory with data.csv (timestamp, w_xyz, a_xyz) or NULL.  Host only. */
typedef struct vslam_dataset vslam_dataset;
vslam_status vslam_dataset_open(int32_t kind, const char* images_path, const char* imu_path, vslam_dataset** out);
void vslam_dataset_close(vslam_dataset* d);
int32_t vslam_dataset_frames(const vslam_dataset* d);
vslam_status vslam_dataset_frame(const vslam_dataset* d, int32_t i, const char** left_path, const char** right_path, double* timestamp);
vslam_status vslam_dataset_imu_bucket(const vslam_dataset* d, int32_t i, vslam_imu_bucket* bucket);
vslam_status vslam_dataset_gravity(const vslam_dataset* d, int32_t* imu_valid, double* gravity3);

/* The library caches device scratch memory, a stream and the local-BA workspace per calling thread.  Its own threads free
 * theirs; a thread of the caller that used vslam_local_ba / the new-point functions / vslam_system_* may call this before
 * it ends (otherwise the cache lives until the process exits - nothing is freed from thread-exit hooks, where profiler
 * libraries no longer tolerate HIP calls). */
void vslam_thread_release(void);

/* plain device buffers for callers that have no HIP binding of their own (the *_device entry points take such pointers) */
vslam_status vslam_device_alloc(int32_t device, size_t bytes, void** out);
vslam_status vslam_device_upload(int32_t device, void* dst, const void* src, size_t bytes);
vslam_status vslam_device_download(int32_t device, void* dst, const void* src, size_t bytes);
void vslam_device_free(int32_t device, void* p);

/* debug aid: fill every device allocation made from now on (and every reused scratch block) with `byte` (< 0: off; the
 * VSLAM_POISON environment variable sets the start value) - results must not depend on it */
void vslam_debug_poison(int32_t byte);

/* device time per kernel group since the previous call (summed over launches; read-and-reset) */
vslam_status vslam_matcher_timings(const vslam_matcher* m, const char** names, float* ms,
                                   int32_t cap, int32_t* n_out);
vslam_status vslam_matcher_set_timing(vslam_matcher* m, int32_t on);

#ifdef __cplusplus
}
#endif
#endif /* VSLAM_HIP_H */
