/* include/ekfvio.h — C-ABI of libekfvio_hip.so, the MI355X (gfx950) backend for the
 * per-frame hot path of k-sheridan/ekf_vio (predict -> KLT measure -> EKF update).
 *
 * The reference has no plugin/FFI layer: the seam is the public C++ surface of
 * `class TightlyCoupledEKF` (include/ekf_vio/TightlyCoupledEKF.h:25-68) and
 * `KLTTracker::findNewFeaturePositions` (include/ekf_vio/KLTTracker.h:88-90), both called
 * only from `EKFVIO::addFrame` (include/ekf_vio/EKFVIO.cpp:139-219).  Every entry point
 * below names the reference member it replaces.  Plain pointers and sizes only; the
 * caller owns every host buffer; all device state (mean, dense covariance, image
 * pyramids, work buffers) is owned by the opaque handle.  One handle = one HIP stream on
 * one device; calls on one handle must be serialised by the caller; different handles are
 * independent: no handle reads another's state.  The library's only process-wide state is a per-device count of live
 * handles (a device's SOLE handle may run the Cholesky sweep as one persistent launch, which needs every compute unit it
 * asks for; with several handles on a device each takes one launch per block step: same results) and the values of
 * diagnostic environment switches (EKFVIO_*), read once.
 *
 * Layouts: vectors of 2-D points are x,y interleaved f32 (std::vector<Eigen::Vector2f>);
 * 2x2 covariances are column-major f32 (std::vector<Eigen::Matrix2f>); flags are one byte
 * each (std::vector<bool>); dense matrices are column-major with an explicit leading
 * dimension; images are 8-bit single channel with a row stride in bytes.
 *
 * Errors: the reference aborts through ROS_ASSERT or logs and continues.  Here every
 * function returns an int status and never aborts or throws across the boundary.
 */
#ifndef EKFVIO_H_
#define EKFVIO_H_

#include <stdint.h>

/* The library is compiled with -fvisibility=hidden: the entry points marked EKFVIO_API are its ONLY dynamic symbols
 * (tests/test_abi_cpu.py compares the whole `nm -D --defined-only` set with this header), so nothing of its internals can
 * interpose on, or be interposed by, what else a ROS node links (OpenCV, tf, ...). */
#ifndef EKFVIO_API
#define EKFVIO_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define EKFVIO_BASE_STATE_SIZE 22 /* TightlyCoupledEKF.h:12 */

enum {
    EKFVIO_OK = 0,
    EKFVIO_EINVAL = 1,   /* what the reference ROS_ASSERTs (size mismatch, dt < 0, null) */
    EKFVIO_ENUMERIC = 2, /* The factorisation of S met a NON-POSITIVE pivot; the state is still updated, through a signed factor
                            S = U diag(+-1) U^T, as the reference's LDL^T carries a negative pivot along.  STRICTER than the reference's
                            log line: `ROS_ERROR_COND(solver.info() == Eigen::NumericalIssue, ...)` (TightlyCoupledEKF.cpp:579) fires only
                            for a pivot that is EXACTLY zero -- Eigen's simplicial LDL^T sets NumericalIssue for `d == 0` alone and then
                            abandons the factorisation, so what the reference computes behind it (:580) is undefined (it reads D entries
                            it never wrote); a negative pivot passes there without a word.  Here both are reported with this one code; on
                            an exactly zero pivot the state behind it is not finite (1 / 0 in the factor), as undefined as upstream's.
                            (tests/test_oracle_amd_cpu.py, tests/test_gpu_shapes.py: test_exactly_singular_s_*) */
    EKFVIO_ECAPACITY = 3,/* more landmarks than config.max_features */
    EKFVIO_EDEVICE = 4,  /* HIP runtime failure; ekfvio_last_error() has the text */
    EKFVIO_ESTATE = 5,   /* call sequence error (e.g. KLT track before two frames exist) */
    EKFVIO_EABORTED = 6  /* the persistent Cholesky sweep could not get its workgroups resident together (another process or
                            stream held compute units) and gave up.  NOT a numeric warning: the updates behind it were
                            skipped -- Sigma, mu are the propagated ones, never a half-finished factor's.  ekfvio_update and
                            ekfvio_step_image do not return it: they run the update again at once with one launch per block
                            step.  ekfvio_synchronize returns it for a device-resident run (ekfvio_run_uploaded), whose skipped
                            updates cannot be replayed.  Either way the handle uses the per-step sweep from then on. */
};

enum { EKFVIO_PREDICT_STRUCTURED = 0, /* exploits F = [[A,0],[B,D]] (nnz = 358+36N) */
       EKFVIO_PREDICT_DENSE = 1       /* dense F P F^T through the MFMA GEMM (north-star form) */ };

typedef struct ekfvio_filter ekfvio_filter; /* opaque */

/* The handful of Params.h globals the hot path reads, as a plain struct. */
typedef struct ekfvio_config {
    int32_t max_features;                  /* capacity; NUM_FEATURES (Params.h:46) */
    float default_point_depth;             /* Params.h:83, 0.5 */
    float default_point_depth_variance;    /* Params.h:84, 100 */
    float default_point_homogenous_variance; /* Params.h:86, 1e-5 */
    int32_t predict_mode;                  /* EKFVIO_PREDICT_* */
    /* KLT (KLTTracker.cpp:61-64, Params.h:33,36,103-104) */
    int32_t klt_window_size;               /* WINDOW_SIZE 21 */
    int32_t klt_max_pyramid_level;         /* MAX_PYRAMID_LEVEL 3 */
    int32_t klt_max_iterations;            /* 30 */
    float klt_epsilon;                     /* 0.01 */
    float klt_min_eigen;                   /* KLT_MIN_EIGEN 1e-4 */
    int32_t kill_pad;                      /* KILL_PAD 11 */
    int32_t max_image_width;               /* device pyramid capacity */
    int32_t max_image_height;
    int32_t use_principal_point;           /* 0 reproduces Feature.h:60-66 (cx,cy ignored) */
    /* frame ingest and landmark replenishment (Frame.cpp:15-42, EKFVIO.cpp:224-311, Params.h:24-28,43) */
    int32_t inverse_image_scale;           /* INVERSE_IMAGE_SCALE: frames are resized to (w/s, h/s), K/s; reference default 4, here 1 */
    int32_t fast_threshold;                /* FAST_THRESHOLD 50 */
    int32_t min_new_feature_dist;          /* MIN_NEW_FEATURE_DIST 30 (radius of the occupancy circles) */
    float fast_blur_sigma;                 /* FAST_BLUR_SIGMA: 0 = off (reference default), > 0: cv::GaussianBlur(5x5, sigma) before FAST */
    int32_t replenish;                     /* 1: ekfvio_step_image also runs replenishFeatures */
    int32_t sample_based_uncertainty;      /* 0 (reference behaviour): R = 1e-5 I px^2 (estimateUncertainty, KLTTracker.cpp:100-106);
                                              1: R from estimateUncertaintySampleBased (:111-175, dead code there) */
    /* IMU measurement update (the reference's imu_callback is a logging stub, EKFVIO.cpp:113-115) */
    int32_t use_imu;                       /* 0 (reference behaviour): ekfvio_imu does nothing; 1: propagate to the record's stamp, then update */
    float imu_gyro_variance;               /* (rad/s)^2 per axis, default 1e-4 */
    float imu_accel_variance;              /* (m/s^2)^2 per axis, default 1e-2 */
    float gravity[3];                      /* gravity in the filter's world frame (= the first camera frame), default (0, 9.81, 0):
                                              an optical frame, y down; the accelerometer model is a + b_acc - R(q)^T gravity */
    /* forward-backward check of the tracker (not in the reference; see ekfvio_set_klt_fb).  The struct carries no size, so every caller is
       compiled against the header it runs with, wherever a new field goes: this one stands in front of remove_lost, which
       tests/test_remove_cpu.py pins as the last field */
    float klt_fb_max_px;                   /* 0 (reference behaviour): off; > 0: a track that does not come back to within this many pixels is treated as lost */
    /* landmark removal (not in the reference, which flags a lost landmark, TightlyCoupledEKF.cpp:528, and keeps it) */
    int32_t remove_lost;                   /* 0 (reference behaviour): lost landmarks stay in the state, flagged; 1: ekfvio_step_image removes them */
} ekfvio_config;

/* Fills `cfg` with the reference defaults (Params.h D_* values). */
EKFVIO_API int ekfvio_default_config(ekfvio_config* cfg);

/* TightlyCoupledEKF::TightlyCoupledEKF() + initializeBaseState()
 * (TightlyCoupledEKF.cpp:10-56).  `device` is a HIP device ordinal.  `stream` is an
 * existing hipStream_t to enqueue on, or NULL to let the handle create its own.
 * On failure nothing is left allocated and *out is NULL. */
EKFVIO_API int ekfvio_create(const ekfvio_config* cfg, int device, void* stream, ekfvio_filter** out);
EKFVIO_API int ekfvio_destroy(ekfvio_filter* f);
/* initializeBaseState(): back to mu = [0,0,0,1,0...], Sigma diag [0x7,30x9,0.5x6], no landmarks.  (The innovation gate's counts start
 * over; its threshold stays.  The same holds for the tracker's forward-backward check.  The distortion coefficients of
 * ekfvio_set_distortion and the setting of ekfvio_set_camera_model stay too, and so does the setting of ekfvio_set_output_covariance.  The mask of ekfvio_set_mask stays as well, and the setting of ekfvio_set_equalize.
 * So does the tracker's gain/offset term, ekfvio_set_klt_photometric.)
 * (The landmark id counter does NOT start over: the first landmark behind a reset gets an id above every id the handle has handed out,
 * so a consumer never sees two points under one id.  The setting of ekfvio_set_ended_export stays; its report is empty and its total
 * starts over, as the gate's.  The same holds for ekfvio_set_zupt: the setting stays, its report and its count start over.) */
EKFVIO_API int ekfvio_reset(ekfvio_filter* f);
EKFVIO_API const char* ekfvio_last_error(const ekfvio_filter* f);

/* addNewFeatures(std::vector<Eigen::Vector2f>) (TightlyCoupledEKF.cpp:58-94). */
EKFVIO_API int ekfvio_add_features(ekfvio_filter* f, const float* uv, int32_t count);

/* process(float dt) (TightlyCoupledEKF.cpp:96-121): FD linearisation, mean propagation,
 * Sigma <- F Sigma F^T + Q(dt), flush below 1e-13. */
EKFVIO_API int ekfvio_process(ekfvio_filter* f, float dt);

/* numericallyLinearizeProcess (TightlyCoupledEKF.cpp:176-325): writes the dense n x n
 * Jacobian (column-major, ld = n) to host memory.  Does not change the state. */
EKFVIO_API int ekfvio_linearize(ekfvio_filter* f, float dt, float* F_dense);

/* updateWithFeaturePositions(z, R, pass) (TightlyCoupledEKF.cpp:475-628).  `count` must
 * equal the number of landmarks (reference ROS_ASSERT at :478).  Entries of z/R for
 * failed landmarks are ignored.  Returns EKFVIO_OK or EKFVIO_ENUMERIC (an aborted persistent sweep is
 * recovered inside the call, see EKFVIO_EABORTED).  The call returns as soon as the update's status is known -- when the
 * Cholesky sweep has ended; the covariance update behind it may still be running: every later call on this handle is ordered
 * behind it or waits for it (ekfvio_synchronize waits explicitly). */
EKFVIO_API int ekfvio_update(ekfvio_filter* f, const float* z, const float* R, const uint8_t* pass, int32_t count);

/* formFeatureMeasurementMap (TightlyCoupledEKF.cpp:634-661): state index of the single 1.0
 * in each row of H.  Writes 2*(#measured) ints, returns that count through *rows. */
EKFVIO_API int ekfvio_measurement_map(const ekfvio_filter* f, const uint8_t* measured, int32_t count, int32_t* idx, int32_t* rows);

/* previousFeaturePositionVector() (TightlyCoupledEKF.cpp:462-470) and the landmark records
 * (Feature.h:41-46).  Any pointer may be NULL. */
EKFVIO_API int ekfvio_num_features(const ekfvio_filter* f);
EKFVIO_API int ekfvio_dim(const ekfvio_filter* f); /* 22 + 3N */
EKFVIO_API int ekfvio_get_base_mu(ekfvio_filter* f, float base_mu[EKFVIO_BASE_STATE_SIZE]);
EKFVIO_API int ekfvio_get_features(ekfvio_filter* f, float* mu3N, float* last_klt2N, uint8_t* delete_flagN);
EKFVIO_API int ekfvio_get_sigma(ekfvio_filter* f, float* sigma, int32_t ld);
/* getFeatureHomogenousCovariance / getFeatureDepthVariance (TightlyCoupledEKF.cpp:663-681). */
EKFVIO_API int ekfvio_get_feature_cov(ekfvio_filter* f, int32_t index, float cov2x2[4]);
EKFVIO_API int ekfvio_get_depth_variance(ekfvio_filter* f, int32_t index, float* var);
/* setFeatureHomogenousCovariance(index, cov) (TightlyCoupledEKF.cpp:668-676): overwrites the 2x2 (u,v) block of Sigma
 * (column-major, like Eigen::Matrix2f). */
EKFVIO_API int ekfvio_set_feature_cov(ekfvio_filter* f, int32_t index, const float cov2x2[4]);
/* getMetric2PixelMap(K) / getPixel2MetricMap(K) (TightlyCoupledEKF.cpp:683-697): J = diag(K(0,0), K(1,1)) and
 * diag(1/K(0,0), 1/K(1,1)), column-major 2x2; K row-major 3x3 as in CameraInfo.K.  Pure functions of K. */
EKFVIO_API int ekfvio_metric2pixel_map(const float K[9], float J2x2[4]);
EKFVIO_API int ekfvio_pixel2metric_map(const float K[9], float J2x2[4]);
/* What EKFVIO::publishOdometry puts into nav_msgs/Odometry (EKFVIO.cpp:444-477): position base_mu[0..2], orientation
 * (w,x,y,z) base_mu[3..6], linear twist base_mu[7..9], angular twist base_mu[10..12].  Any pointer may be NULL. */
EKFVIO_API int ekfvio_get_odometry(ekfvio_filter* f, float position[3], float orientation_wxyz[4], float linear[3], float angular[3]);
/* What EKFVIO::publishPoints puts into sensor_msgs/PointCloud (EKFVIO.cpp:479-518), formed on the device: camera-frame
 * xyz = (u/rho, v/rho, 1/rho) per landmark and the "intensity" channel = byte of the current (resized) frame at the
 * landmark's pixel (Feature::getPixel, rounded like cv::Point(cv::Point2f)); 0 for a pixel outside the image (the
 * reference reads unchecked there) or before the first frame.  Either pointer may be NULL. */
EKFVIO_API int ekfvio_get_points(ekfvio_filter* f, float* xyz3N, float* intensityN);
/* checkSigma (TightlyCoupledEKF.cpp:699-714) as numbers: min diagonal, max |S_ij - S_ji|. */
EKFVIO_API int ekfvio_check_sigma(ekfvio_filter* f, float* min_diag, float* max_asym);

/* Checkpoint / teacher-forcing hook (the reference has none; its members are public). */
EKFVIO_API int ekfvio_set_state(ekfvio_filter* f, int32_t n_features, const float* base_mu, const float* mu3N,
                     const float* last_klt2N, const uint8_t* delete_flagN, const float* sigma, int32_t ld);

/* Removes landmarks from the state: mean, covariance rows/columns, last KLT results and flags, keeping the order of the rest
 * (marginalisation of a Gaussian: exact).  remove != NULL: count must equal the landmark count, nonzero bytes are removed;
 * remove == NULL: the landmarks flagged for deletion (the tracker lost them, TightlyCoupledEKF.cpp:528) are removed.
 * *removed (may be NULL) receives the number removed.  Not in the reference, which flags but never removes. */
EKFVIO_API int ekfvio_remove_features(ekfvio_filter* f, const uint8_t* remove, int32_t count, int32_t* removed);

/* ---- landmark identities and the tracks that ended (not in the reference, which never removes a landmark, so that a landmark's index
 * is its identity there) ---------------------------------------------------------------------------------------------------------------
 * A removal compacts the state: row i of ekfvio_get_points, ekfvio_get_points_covariance, ekfvio_get_features, ekfvio_get_gate,
 * ekfvio_get_klt_fb and ekfvio_get_mask_hits names another physical point from one frame to the next.  Two arrays travel with the state on
 * the device, through the kernels that move it, and say which (always on, no setting):
 *
 *     id    int64.  The handle keeps a counter next_id, 0 at ekfvio_create.  The k-th landmark a call appends (k = 0, 1, ...) gets
 *           next_id + k, and next_id advances by the number appended where the landmark count does: at the end of ekfvio_add_features,
 *           ekfvio_replenish and ekfvio_set_state, and in ekfvio_step_image with the frame's status word (a frame that returns an error
 *           without counting its new landmarks in does not advance it either: those ids were never visible).  ekfvio_set_state replaces
 *           the landmark set: all n_features landmarks get fresh ids, in order.  An id is never reused during the handle's lifetime;
 *           the counter does not start over at ekfvio_reset.
 *     born  double.  The stamp of the ekfvio_step_image call in which the landmark entered; for ekfvio_add_features, ekfvio_replenish and
 *           ekfvio_set_state outside a frame the handle's current time (the stamp of the last frame or IMU record), NaN before any stamp.
 *
 * A removal keeps the order of the rest and new landmarks are appended, so id is STRICTLY INCREASING in landmark order at all times: a
 * consumer associates two frames' clouds with one merge pass.  Nothing but an append, a removal and ekfvio_set_state touches either array:
 * process(dt), the updates and ekfvio_run_uploaded leave them alone (the measurement streams of ekfvio_run_uploaded carry no ids).
 *
 * ekfvio_get_landmark_ids: room for ekfvio_num_features entries each; either pointer may be NULL.  Rows are the rows of ekfvio_get_points
 * of the same moment.  Behind ekfvio_step_image both arrays arrive with the frame's other outputs and the call is a memcpy until the state
 * changes; otherwise it is a device-to-host copy on the handle's stream and a wait, as ekfvio_get_features. */
EKFVIO_API int ekfvio_get_landmark_ids(ekfvio_filter* f, int64_t* idN, double* bornN);
/* The tracks that ended.  A landmark that leaves the state takes a 3-D estimate and a covariance with it that the filter has paid for; the
 * removal is the only moment a sparse map point can be handed out.  With the setting on, every removal that is launched --
 * ekfvio_remove_features with a mask or with NULL, ekfvio_step_image with cfg.remove_lost = 1 -- is preceded on the stream by one launch
 * that reads the removal's own decision and writes one record per landmark about to leave, in landmark order:
 *
 *     id (int64)   born (double)   index_before (int32: the landmark's row in front of this removal -- the row numbering that ekfvio_get_gate,
 *                                  ekfvio_get_klt_fb and ekfvio_get_mask_hits of the same frame use; the caller joins them for a reason)
 *     xyz[3]       the camera-frame point, by the lines of ekfvio_get_points
 *     cov[9]       its covariance, row-major 3x3, by the lines of ekfvio_get_points_covariance
 *
 * from the mean and Sigma as they stand in front of the removal (in a frame: behind the update's last GEMM and behind the replenishment).
 * xyz and cov are, bit for bit, what the two getters would have returned for that row had they been called in front of the removal: the
 * device compiles one statement of that arithmetic for all of them.  Behind an aborted persistent sweep a frame's removal removes nothing,
 * and nothing ends.  Out of scope: a reason code per record, world-frame points (the frame's odometry is in the same output block), removal
 * or lookup by id, observation counts.
 *
 * on: 0 or 1, anything else EKFVIO_EINVAL.  A property of the handle: it holds from the next removal, survives ekfvio_reset and drops no
 * captured graph.  Off by default (then no launch differs, nothing is allocated and every output keeps its bits); on, it costs one launch of
 * one workgroup per removal and 68 bytes of pinned host memory per landmark of max_features, taken when it is first turned on (the kernel writes
 * the records there, and ekfvio_get_ended is a memcpy). */
EKFVIO_API int ekfvio_set_ended_export(ekfvio_filter* f, int32_t on);
/* The records of the MOST RECENT removal call since the setting was turned on (any pointer may be NULL; the arrays need room for *count
 * records).  *count = the host-known removed count of that call; a removal call that removes nothing -- an explicit mask of zeros, NULL with
 * nothing flagged, a frame with no landmark, an aborted sweep -- reports 0, and so does a handle with the setting off.  cap < *count:
 * EKFVIO_EINVAL, with *count and *total still set.  *total = records since create or the last ekfvio_reset.  Each removal overwrites the
 * last one's records: a consumer that wants every ended track reads them after every frame (and after every ekfvio_remove_features). */
EKFVIO_API int ekfvio_get_ended(ekfvio_filter* f, int64_t* id, double* born, int32_t* index_before, float* xyz3, float* cov9, int32_t cap,
                                int32_t* count, int64_t* total);

/* ---- innovation gate (not in the reference: its Params.h has an "OUTLIER DETECTION" section whose thresholds nothing reads) ---------
 * A chi-square test per landmark, evaluated on the device on the propagated state in front of the update's measurement bookkeeping
 * (ekfvio_update, ekfvio_run_uploaded, ekfvio_step_image; the IMU update is not gated).  For every landmark i with pass[i] != 0, with
 * s = 22 + 3 i, all in fp32, in this order, without fused multiply-add and with correctly rounded division (a NumPy float32
 * restatement of these lines gives the same bits):
 *
 *     y0 = z[2i]   - mu[s]          y1 = z[2i+1] - mu[s+1]
 *     a  = P(s,s)     + R_i(0,0)
 *     b  = P(s+1,s)   + R_i(1,0)          (the lower triangle's element of both)
 *     c  = P(s+1,s+1) + R_i(1,1)
 *     det = a*c - b*b
 *     q   = ((c*y0)*y0 - ((2*b)*y0)*y1) + (a*y1)*y1
 *     d2  = q / det
 *     accept  <=>  det > 0  and  d2 <= chi2        (a NaN anywhere rejects)
 *
 * mu, P: the state the update is about to read (behind process(dt)); R_i: the column-major 2x2 the caller or the tracker supplied.
 * H is a selection matrix, so [[a, b], [b, c]] is the landmark's 2x2 innovation covariance.  A rejected landmark is treated in every
 * respect as one the tracker failed (TightlyCoupledEKF.cpp:526-529): no measurement rows, last_klt kept, delete flag set -- and with
 * cfg.remove_lost = 1 ekfvio_step_image removes it in the same frame.  Landmarks with pass[i] == 0 are not evaluated.
 *
 * chi2 > 0: gate on from the next update; chi2 == 0: off (default).  Negative, NaN: EKFVIO_EINVAL.
 * Drops the handle's captured step graphs (the launch sequence differs). */
EKFVIO_API int ekfvio_set_gate(ekfvio_filter* f, float chi2);
/* Results of the most recent update (any pointer may be NULL): d2 per landmark as defined above
 * (-1: not evaluated) and a gated flag per landmark, both with room for max_features entries;
 * *n_landmarks = the landmark count that update saw (indices are its indices, before any removal or
 * replenishment of the same frame; 0 before the first gated update); number gated by that update;
 * total since create/reset. */
EKFVIO_API int ekfvio_get_gate(ekfvio_filter* f, float* d2, uint8_t* gated, int32_t* n_landmarks, int32_t* gated_last,
                               int64_t* gated_total);

/* ---- rectification of distorted frames (not in the reference: Frame.h:31 "for now the image must be undistorted for simplicity", its D
 * at :32 is never read, and its deployment runs image_proc/rectify in front of the node) ------------------------------------------------
 * With distortion coefficients set, every pushed frame (ekfvio_klt_push_frame, ekfvio_step_image) is rectified on the device between
 * its upload and the pyramid: cv::initUndistortRectifyMap(K, D, R = I, new camera matrix = K, CV_16SC2) + cv::remap(INTER_LINEAR,
 * BORDER_CONSTANT 0) of the full-size frame, plumb_bob model D = (k1, k2, p1, p2, k3).  The lines below are the specification; they
 * restate OpenCV's fixed-point remap (INTER_BITS = 5) from memory, not from its source, and a NumPy restatement of them
 * (tests/_rectify.py) is what the device is held to, bit for bit.  For destination pixel (x, y) of the full-size w x h frame, with
 * fx, cx, fy, cy = K[0], K[2], K[4], K[5] of the K passed with the frame (before the division by inverse_image_scale; cx, cy are the true
 * ones whatever use_principal_point says), everything in fp64, in this order, without fused multiply-add:
 *
 *     xn = (x - cx) / fx        yn = (y - cy) / fy
 *     xx = xn*xn   yy = yn*yn   xy = xn*yn   r2 = xx + yy
 *     rad = 1 + ((k3*r2 + k2)*r2 + k1)*r2
 *     xd = (xn*rad + (2*p1)*xy) + p2*(r2 + 2*xx)
 *     yd = (yn*rad + p1*(r2 + 2*yy)) + (2*p2)*xy
 *     u = fx*xd + cx            v = fy*yd + cy
 *     valid  <=>  |u| <= 2^20  and  |v| <= 2^20          (a NaN is invalid)
 *     sx = rint(u*32), sy = rint(v*32) as int32 (round half to even);  invalid: sx = sy = INT32_MIN
 *
 * then in integers: ix = sx >> 5, ax = sx & 31 (arithmetic shift), the same for y; the four taps (ix,iy), (ix+1,iy), (ix,iy+1),
 * (ix+1,iy+1) of the uploaded frame with the weights (32-ax)(32-ay), ax(32-ay), (32-ax)ay, ax*ay; a tap outside [0,w) x [0,h)
 * contributes 0 (so the sentinel gives 0 by itself); out = (sum + 512) >> 10.  With D = 0 the map is exactly (32x, 32y) and the frame
 * keeps every byte.  The rectified full-size frame then takes the road of an uploaded one: the resize and the pyramid read it, K is
 * unchanged, and the intensity channel of ekfvio_get_points reads it.  The map is formed on the device once per (fx, cx, fy, cy, D, w, h)
 * and kept.  The rational and the equidistant model and a new camera matrix: ekfvio_set_camera_model, below; out of scope: an alpha crop.
 * (The black border these lines leave, as image_proc/rectify does, is kept away from the detector and the tracker by ekfvio_set_mask, below.)
 *
 * count = 5: D as above; count = 4: k3 = 0; count = 0 (D may be NULL) or all coefficients zero: off (default; then no launch differs and
 * every output keeps its bits).  A non-finite coefficient, any other count, NULL with count > 0: EKFVIO_EINVAL, and the setting stays
 * what it was.  A property of the handle: it holds from the next pushed frame and survives ekfvio_reset. */
EKFVIO_API int ekfvio_set_distortion(ekfvio_filter* f, const double* D, int32_t count);
/* The map itself, sx and sy as defined above, row-major width x height int32 each: a pure host function (no handle, no device) that
 * compiles the very inline function the device's map kernel compiles.  Callers take the valid region of the rectified frame from it
 * (a tap outside the frame means no data there).  D, count as above (count = 0: the identity map). */
EKFVIO_API int ekfvio_rectify_map(const float K[9], const double* D, int32_t count, int32_t width, int32_t height, int32_t* sx,
                                  int32_t* sy);

/* ---- camera models: the rational and the equidistant lens, and a rectified camera of its own (not in the reference) -------------------
 * ekfvio_set_distortion knows the plumb_bob lens and rectifies onto the raw camera's own K.  This section adds the two models a wide-angle
 * camera is usually calibrated with -- rational_polynomial (8 coefficients, what ROS camera_calibration emits for a wide lens) and
 * equidistant (Kannala-Brandt, cv::fisheye, Kalibr's "equidistant": 4 coefficients) -- and P, the intrinsics of the RECTIFIED image
 * (CameraInfo.P), so that a fisheye frame can be zoomed out to keep its field of view or zoomed in to keep its resolution.  The lines below
 * are the specification; csrc/rectify_map.h implements them, one inline function for the host and the device, and a NumPy restatement
 * (tests/_camera_models.py) is what the device is held to, bit for bit.  Everything in fp64, in this order, without fused multiply-add;
 * division and square root are IEEE correctly rounded.
 *
 * Destination pixel (x, y) of the full-size w x h frame; (fx, cx, fy, cy) = K[0], K[2], K[4], K[5] of the K passed with the frame;
 * (fx', cx', fy', cy') = P where set, otherwise the same four values of K:
 *
 *     xn = (x - cx') / fx'      yn = (y - cy') / fy'
 *     xx = xn*xn   yy = yn*yn   xy = xn*yn   r2 = xx + yy
 *
 *     PLUMB_BOB   (k1,k2,p1,p2[,k3])          rad, xd, yd: the lines of ekfvio_set_distortion (with P absent: its bits)
 *     RATIONAL    (k1,k2,p1,p2,k3,k4,k5,k6)   num = 1 + ((k3*r2 + k2)*r2 + k1)*r2
 *                                             den = 1 + ((k6*r2 + k5)*r2 + k4)*r2
 *                                             rad = num / den
 *                                             xd, yd by the plumb_bob lines with this rad
 *     EQUIDISTANT (k1,k2,k3,k4)               r = sqrt(r2)     th = atan_spec(r)     t2 = th*th
 *                                             thd = th * (1 + (((k4*t2 + k3)*t2 + k2)*t2 + k1)*t2)
 *                                             sc = (r == 0) ? 1 : thd / r
 *                                             xd = xn*sc       yd = yn*sc
 *
 *     u = fx*xd + cx    v = fy*yd + cy    then valid / sx / sy / sentinel, and the integer remap, exactly as for ekfvio_set_distortion
 *
 * Two properties follow from the lines: RATIONAL with k4 = k5 = k6 = 0 has den == 1 and rad == num, so it gives the plumb_bob map; and a P
 * whose four floats equal K's gives the map without P.
 *
 * atan_spec(r), r >= 0, is a fixed fp64 recipe, so that the device, the host function and NumPy cannot disagree in the last place the way
 * three libm implementations can (within 3 ulp of a correctly rounded arctan over [0, 50] and over 1e-300 .. 1e300; atan_spec(0) = 0,
 * atan_spec(inf) = PI_2):
 *
 *     T8 = 0.41421356237309503    PI_4 = 0.7853981633974483    PI_2 = 1.5707963267948966      (the doubles these literals read as)
 *     inv = r > 1          t = inv ? 1/r : r
 *     sh  = t > T8         t = sh ? (t - 1)/(t + 1) : t
 *     q = t*t
 *     p = c19;  for k = 18 .. 0:  p = p*q + c_k        c_k = (k even ? +1 : -1) * (1.0 / (2k+1)), k = 0..19
 *     a = t*p
 *     if sh:  a = PI_4 + a
 *     if inv: a = PI_2 - a
 *
 * Where P goes.  The rectification reads the K as passed (the raw camera).  With P set, everything BEHIND the rectification sees the
 * rectified camera: the pushed frame's K takes P's four values in K's places before the division by inverse_image_scale, so the pixel <->
 * metric conversion, the tracker's guesses, R's scaling, replenishment and the point cloud's pixel all use P.  The K argument of
 * ekfvio_klt_push_frame and ekfvio_step_image stays "the raw camera's intrinsics".
 *
 * The device side: one instance of the map kernel per model, launched once per (K, model, coefficients, P, w, h) and kept; the per-frame
 * remap, the pyramid, the tracker and the update are the same code for every lens.  The mask's border term (ekfvio_set_mask) reads the
 * same map, whatever the model, and is live whenever this setting is on.
 *
 * ekfvio_set_camera_model.  count: PLUMB_BOB 0, 4 or 5; RATIONAL 8; EQUIDISTANT 4 (zeros allowed: the ideal fisheye lens).  P: fx', cx',
 * fy', cy', or NULL for K.  Off: PLUMB_BOB or RATIONAL with every coefficient zero and P == NULL (then no launch differs, nothing is
 * allocated and every output keeps its bits).  On otherwise -- that includes P alone (a pure re-projection) and EQUIDISTANT with zero
 * coefficients (atan is not the identity).  An unknown model, a wrong count, NULL with count > 0, a non-finite value, fx' <= 0 or fy' <= 0:
 * EKFVIO_EINVAL, and the setting stays what it was.  ekfvio_set_distortion is the PLUMB_BOB, P == NULL case of this call, and the last of the
 * two setters wins.  A property of the handle: it holds from the next pushed frame and survives ekfvio_reset.
 *
 * Out of scope: thin-prism and tilt coefficients (OpenCV's 12 and 14); choosing P automatically (alpha, balance); tracking on the raw
 * fisheye image without rectification; and the fold-over of a polynomial beyond its calibrated field, which these lines reproduce as they
 * stand (a rational den that crosses zero gives invalid entries and, behind it, a mirrored ring: mask it). */
enum { EKFVIO_CAMERA_PLUMB_BOB = 0, EKFVIO_CAMERA_RATIONAL = 1, EKFVIO_CAMERA_EQUIDISTANT = 2 };
EKFVIO_API int ekfvio_set_camera_model(ekfvio_filter* f, int32_t model, const double* D, int32_t count,
                                       const float P[4] /* fx', cx', fy', cy'; NULL: K */);
/* The setting as the handle holds it: the model, its coefficients in the setter's order (zeros behind *count), P (zeros unless *has_P),
 * and whether frames are rectified.  Any pointer may be NULL. */
EKFVIO_API int ekfvio_get_camera_model(ekfvio_filter* f, int32_t* model, double D[8], int32_t* count, float P[4], int32_t* has_P,
                                       int32_t* on);
/* ekfvio_rectify_map for any model and P: a pure host function (no handle, no device) over the very inline function the map kernels
 * compile.  Arguments as ekfvio_set_camera_model and ekfvio_rectify_map take them. */
EKFVIO_API int ekfvio_rectify_map_model(const float K[9], int32_t model, const double* D, int32_t count, const float P[4], int32_t width,
                                        int32_t height, int32_t* sx, int32_t* sy);

/* ---- no-data mask (not in the reference, which passes no mask to cv::FAST, EKFVIO.cpp:224-311) ----------------------------------------
 * Keeps the detector and the tracker off pixels that hold no scene.  Two sources: the black border that rectification leaves (FAST fires on
 * its edge, and the corners it finds there are fixed in the image: landmarks that contradict every camera motion, which neither the gate
 * nor the forward-backward check can see), and regions the caller knows are not scene (a bonnet, a gimbal arm, a burnt-in timestamp).  The
 * lines below are the specification; a NumPy restatement of them (tests/_mask.py) is what the device is held to, bit for bit.
 *
 * A pushed frame is w x h at full size; s = max(cfg.inverse_image_scale, 1); W = w / s, H = h / s (integer division: the size of level 0);
 * pad = max(cfg.kill_pad, 0).
 *
 *  1. Full-size no-data n(x, y), the OR of two terms.
 *     Caller's mask: a mask is set and mask[y * stride + x] == 0.
 *     Rectification border: EKFVIO_MASK_RECTIFY_BORDER is set and distortion is on.  With (sx, sy) the map entry of (x, y) (ekfvio_set_distortion,
 *     above), ix = sx >> 5, ax = sx & 31, iy = sy >> 5, ay = sy & 31 as there: no-data if any of the four taps (ix, iy), (ix+1, iy), (ix, iy+1),
 *     (ix+1, iy+1) with the weights (32-ax)(32-ay), ax(32-ay), (32-ax)ay, ax*ay has a non-zero weight and lies outside [0, w) x [0, h).  (The
 *     sentinel entry needs no special case: its first tap has weight 1024 and lies outside.  Nor does the identity map: its taps outside the
 *     frame have weight 0.)
 *  2. Level-0 no-data N(X, Y): the OR of n(x, y) over x in [s X, s X + s), y in [s Y, s Y + s).  Outside [0, W) x [0, H): N = 1.  (Every pixel the
 *     resize reads for (X, Y) lies in that block.)
 *  3. Blocked B(X, Y): the OR of N(X', Y') over X' in [X - pad, X + max(pad - 1, 0)] and Y' in the same window around Y.  The window is
 *     asymmetric by one on purpose: with no no-data pixel inside the frame, B is exactly the complement of Frame::isPixelInBox, whose test is
 *     x < pad || w - x < pad.  The mask generalises the kill box; it has no margin parameter of its own.
 *
 * Detector (ekfvio_replenish; ekfvio_step_image with cfg.replenish = 1): the occupancy image starts as B instead of empty; a blocked keypoint is
 * skipped exactly as an occupied one is.  The kill-box test stays.
 * Tracker (ekfvio_klt_track, ekfvio_step_image; with the constant R and with the sample-based R): pass additionally requires
 * B(cvRound(ox), cvRound(oy)) == 0 for the tracked pixel (ox, oy); cvRound is round-half-to-even, as Feature::getPixel's conversion; a rounded
 * pixel outside level 0 counts as blocked.  The order of verdicts: forward status, forward-backward check, kill box, mask: masked[i] = 1 only
 * for a landmark that everything before the mask let through.  A masked landmark takes in every respect the road of one the tracker lost:
 * pass = 0, z and R zero, no measurement rows, last_klt kept, delete flag set by the update -- and with cfg.remove_lost = 1 ekfvio_step_image
 * removes it in the same frame.  The innovation gate never sees it.  ekfvio_klt_track_points and ekfvio_klt_track_points_fb work in pixel
 * space, have no pass test and do not change.  ekfvio_add_features stays unchecked: a caller's own detector is the caller's business.
 *
 * B is formed on the device once per (rectification key where the border term is live, caller's mask, s, pad, w, h, flags), behind the
 * rectification of the frame that first needs it, and kept as bit words; per frame the detector copies it into its occupancy image and the
 * tracker reads one bit per landmark.
 *
 * ekfvio_set_mask.  mask: w x h bytes at the FULL frame size with a row stride, nonzero = scene; NULL (width = height = stride = 0): no caller's
 * mask.  mask == NULL and flags == 0: off (default; then no launch differs, nothing is allocated and every output keeps its bits).  The mask is
 * copied before the call returns (the call waits for the handle's stream first).  A property of the handle: it holds from the next pushed frame
 * and survives ekfvio_reset.  Unknown flag bits, NULL with a non-zero size, stride < width, a size outside [1, 16384]: EKFVIO_EINVAL, and the
 * setting stays what it was.  While a caller's mask is set, a frame pushed with another size is refused (EKFVIO_EINVAL, ekfvio_last_error has
 * the sizes) and not ingested.  The border flag with distortion off contributes nothing; it is not an error. */
enum { EKFVIO_MASK_RECTIFY_BORDER = 1 };
EKFVIO_API int ekfvio_set_mask(ekfvio_filter* f, const uint8_t* mask, int32_t width, int32_t height, int32_t stride, int32_t flags);
/* B as the device holds it, one byte (0/1) per level-0 pixel, row-major *w x *h, and its size; *w = *h = 0 before the first frame pushed with
 * the mask on (and again once a frame has been pushed with it off).  blocked may be NULL (the size alone); cap < *w * *h: EKFVIO_EINVAL. */
EKFVIO_API int ekfvio_get_mask(ekfvio_filter* f, uint8_t* blocked, int32_t cap, int32_t* w, int32_t* h);
/* Per landmark of the most recent track of the landmarks with the mask on: masked flag (room for max_features), the landmark count that
 * track saw (indices are its indices; 0 before the first such track), number masked.  Any pointer may be NULL. */
EKFVIO_API int ekfvio_get_mask_hits(ekfvio_filter* f, uint8_t* masked, int32_t* n_landmarks, int32_t* masked_last);
/* B on the host, width / s x height / s bytes: a pure host function (no handle, no device) that compiles the very inline functions the
 * kernels compile, as ekfvio_rectify_map does.  K, D, count as there (K may be NULL where the border term is not live); mask may be NULL. */
EKFVIO_API int ekfvio_mask_blocked(const float K[9], const double* D, int32_t count, const uint8_t* mask, int32_t width, int32_t height,
                                   int32_t stride, int32_t inverse_image_scale, int32_t kill_pad, int32_t flags, uint8_t* blocked);
/* The same for any camera model and P (ekfvio_set_camera_model): the border term is live where the flag is set and that setting is on, and
 * reads the map of ekfvio_rectify_map_model.  A pure host function. */
EKFVIO_API int ekfvio_mask_blocked_model(const float K[9], int32_t model, const double* D, int32_t count, const float P[4],
                                         const uint8_t* mask, int32_t width, int32_t height, int32_t stride, int32_t inverse_image_scale,
                                         int32_t kill_pad, int32_t flags, uint8_t* blocked);

/* ---- equalisation of pushed frames (not in the reference, whose detector runs at a fixed contrast threshold, EKFVIO.cpp:224-311, and whose
 * tracker assumes brightness constancy; VINS-style front ends run a cv::CLAHE pass on the host in front of the tracker) ----------------------
 * With the setting on, every pushed frame (ekfvio_klt_push_frame, ekfvio_step_image) is equalised on the device between its upload -- or its
 * rectification, where distortion is on -- and the pyramid: clip-limited histograms per tile, one table per tile, every pixel blended from the
 * four tables around it.  The lines below are the specification, restated from memory of cv::CLAHE, not from its source; a NumPy restatement of
 * them (tests/_equalize.py) is what the device is held to, bit for bit.
 *
 * Inputs: the full-size w x h frame (the rectified one where distortion is on), tiles tx x ty, clip_limit as fp32.
 * Host values, formed once and passed to the kernels as arguments:
 *
 *     tw = ceil(w / tx)    th = ceil(h / ty)    A = tw * th
 *     clip = max((int)floor((double)clip_limit * A / 256.0), 1)        (a value above A is taken as A: no bin holds more, the result is the same)
 *     scale = 255.0f / (float)A    inv_tw = 1.0f / (float)tw    inv_th = 1.0f / (float)th                                             (fp32)
 *
 *  1. Padded source.  Tile (i, j) covers X in [i tw, (i+1) tw) and Y in [j th, (j+1) th) of the padded frame and reads
 *     src(X >= w ? 2(w-1) - X : X,  Y >= h ? 2(h-1) - Y : Y)  (reflect-101; one reflection suffices because tx <= w and ty <= h are required:
 *     tx tw <= w + tx - 1 <= 2w - 1).  Every tile therefore has exactly A pixels.
 *  2. Histogram.  hist[256] of the tile, in integers.
 *  3. Clip and redistribute.  excess = sum max(hist[b] - clip, 0), then hist[b] = min(hist[b], clip).  batch = excess / 256,
 *     res = excess - 256 batch, then hist[b] += batch.  If res > 0: step = max(256 / res, 1), and bin b gets +1 iff b % step == 0 and
 *     b / step < res.  The sum stays A.
 *  4. Table.  lut[b] = saturate_u8(rint((float)(hist[0] + ... + hist[b]) * scale)): the integer sum converted to fp32 round-to-nearest, rint
 *     half to even.  So lut[255] = 255.
 *  5. Interpolation.  Per pixel (x, y) with value v, in fp32, without fused multiply-add:
 *         fx = (float)x * inv_tw - 0.5f    t = floorf(fx)    xa = fx - t    xa1 = 1.0f - xa
 *         i1 = max((int)t, 0)    i2 = min((int)t + 1, tx - 1)
 *     the same for y with inv_th, giving ya, ya1, j1, j2, and
 *         out = saturate_u8(rint((lut[j1][i1][v]*xa1 + lut[j1][i2][v]*xa)*ya1 + (lut[j2][i1][v]*xa1 + lut[j2][i2][v]*xa)*ya))
 *
 * The equalised full-size frame then takes the road of an uploaded one: the resize, the pyramid, FAST, the sample-based R and the intensity
 * channel of ekfvio_get_points all see it.  K, the rectification map and the mask's B do not change.  Two limits.  The black rectification
 * border and a caller's masked region are counted in the histograms; the clip bounds their influence to one bin's worth, and leaving no-data
 * pixels out is out of scope.  And cfg.fast_threshold now acts on stretched contrast, so the detector finds more.  Equalisation is no full
 * repair of a gain change either: the tracks it does not save are what the forward-backward check and the gate are for.
 *
 * ekfvio_set_equalize.  clip_limit == 0: off (default; then no launch differs, nothing is allocated and every output keeps its bits; the tile
 * counts are not looked at).  clip_limit > 0 and finite with tiles_x, tiles_y in [1, 16]: on from the next pushed frame.  A negative, NaN or
 * infinite clip_limit, tiles out of range: EKFVIO_EINVAL, and the setting stays what it was.  A property of the handle: it survives
 * ekfvio_reset.  While it is on, a frame with width < tiles_x or height < tiles_y is refused (EKFVIO_EINVAL, ekfvio_last_error has the sizes)
 * and not ingested.  The frame is equalised in place in the handle's own staging plane; the setting costs tiles_x * tiles_y * 256 bytes of
 * device memory, taken when the first frame arrives with it on. */
EKFVIO_API int ekfvio_set_equalize(ekfvio_filter* f, float clip_limit, int32_t tiles_x, int32_t tiles_y);
/* The equalised frame itself, width x height bytes tightly packed into out: a pure host function (no handle, no device) that compiles the very
 * inline functions the kernels compile, as ekfvio_rectify_map does.  image: width x height bytes with a row stride.  clip_limit > 0 and finite,
 * tiles in [1, 16] and not above the frame's size, a size in [1, 16384], stride >= width; anything else: EKFVIO_EINVAL. */
EKFVIO_API int ekfvio_equalize(const uint8_t* image, int32_t width, int32_t height, int32_t stride, float clip_limit, int32_t tiles_x,
                               int32_t tiles_y, uint8_t* out);

/* ---- covariances of the published outputs (not in the reference: EKFVIO.cpp:473 "TODO add convariance computation"; its Odometry
 * message carries two all-zero 6x6 covariances) -----------------------------------------------------------------------------------------
 * The covariance of what ekfvio_get_odometry and ekfvio_get_points return, formed on the device from the dense Sigma.  The lines below
 * are the specification: everything in fp32, without fused multiply-add; a sum runs over an ascending index and associates to the left;
 * a NumPy float32 restatement of them (tests/_covout.py) is what the device is held to, bit for bit.  S(i,j) always means Sigma's
 * LOWER-triangle element P(max(i,j), min(i,j)), as the gate reads it (both triangles agree only up to rounding, and the mirrored Joseph
 * GEMM writes one of them).  Of every result the lower triangle is computed and then mirrored: the outputs are exactly symmetric.
 *
 * Pose covariance: 6x6, row-major, ordered (x, y, z, rotation about X, Y, Z), in the filter's world frame with fixed axes -- what
 * nav_msgs/Odometry.pose.covariance asks for.  The rotation error is dtheta with q_true = [1, dtheta/2] (x) q; the state's quaternion is
 * body-to-world, so this left perturbation is in world axes.  With (qw, qx, qy, qz) = mu[3..6]:
 *
 *     J = 2 * [ -qx   qw  -qz   qy ]
 *             [ -qy   qz   qw  -qx ]          3x4, columns w, x, y, z (the doubling and the negation are exact)
 *             [ -qz  -qy   qx   qw ]
 *     A = blkdiag(I3, J)   (6x7)              C = A S[0:7, 0:7] A^T
 *
 *     T[r][j]   = S(r,j)                                                                      r < 3      (a copy, not a product)
 *     T[3+r][j] = ((J[r][0]*S(3,j) + J[r][1]*S(4,j)) + J[r][2]*S(5,j)) + J[r][3]*S(6,j)       r = 0..2, j = 0..6
 *     for a >= b:
 *         C[a][b] = S(a,b)                                                                    a < 3
 *         C[a][b] = T[a][b]                                                                   a >= 3 > b
 *         C[a][b] = ((T[a][3]*J[b-3][0] + T[a][4]*J[b-3][1]) + T[a][5]*J[b-3][2]) + T[a][6]*J[b-3][3]     otherwise
 *     C[b][a] = C[a][b]
 *
 * J q = 0: the direction of the quaternion's norm drops out by itself.  At q = (1,0,0,0) the rotation block is 4 S[4:7, 4:7].
 *
 * Twist covariance: 6x6, row-major, ordered (linear, angular): S[7:13, 7:13], copied and mirrored.  Both are body-frame quantities in this
 * motion model (the position advances by q * (dt vel + ...), omega is the body rate): what twist.covariance means for the child frame.
 *
 * Landmark covariance: one 3x3 per landmark, row-major, 9 floats: the covariance of the camera-frame point (u/rho, v/rho, 1/rho) that
 * ekfvio_get_points returns.  For landmark i with s = 22 + 3i, (u, v, rho) = mu[s..s+2]:
 *
 *     z = (float)(1.0 / (double)rho)     x = u*z     y = v*z                   (the very values of the point cloud)
 *     jx = -(x*z)     jy = -(y*z)     jz = -(z*z)                              Jl = [[z, 0, jx], [0, z, jy], [0, 0, jz]]
 *     L(a,b) = S(s+a, s+b)                                                     M = Jl L,  Cl = M Jl^T, structural zeros skipped:
 *     M00 = z*L(0,0) + jx*L(2,0)     M02 = z*L(0,2) + jx*L(2,2)
 *     M10 = z*L(1,0) + jy*L(2,0)     M11 = z*L(1,1) + jy*L(2,1)     M12 = z*L(1,2) + jy*L(2,2)
 *     M20 = jz*L(2,0)     M21 = jz*L(2,1)     M22 = jz*L(2,2)
 *     Cl[0][0] = M00*z + M02*jx
 *     Cl[1][0] = M10*z + M12*jx          Cl[1][1] = M11*z + M12*jy
 *     Cl[2][0] = M20*z + M22*jx          Cl[2][1] = M21*z + M22*jy          Cl[2][2] = M22*jz
 *     Cl[0][1] = Cl[1][0]     Cl[0][2] = Cl[2][0]     Cl[1][2] = Cl[2][1]
 *
 * A landmark no update has measured yet has L = diag(hv, hv, dv) (addNewFeatures), for which these lines give Jl diag(hv, hv, dv) Jl^T.
 * Cross-covariances between landmarks, or between a landmark and the pose, are not reported.
 *
 * Two roads.  On demand: the getters below launch their own kernel on the handle's stream (so behind an update's Joseph GEMM that is
 * still running) and wait for it -- one launch for all landmarks.  In the frame: with ekfvio_set_output_covariance(f, 1),
 * ekfvio_step_image writes the three results with the frame's other outputs and the status word, and the getters cost a memcpy until
 * the state changes.  Such a frame cannot publish in front of the update's last GEMM (Sigma' does not exist yet): its outputs go out
 * behind the frame's last launch, as those of a frame that replenishes or removes already do.  The setting changes WHEN a frame's
 * outputs are published, never what the filter computes.  Off by default (then no launch differs and every output keeps its bits).
 * A property of the handle: it survives ekfvio_reset.  Values other than 0 and 1: EKFVIO_EINVAL. */
EKFVIO_API int ekfvio_set_output_covariance(ekfvio_filter* f, int32_t on);
/* Either pointer may be NULL. */
EKFVIO_API int ekfvio_get_odometry_covariance(ekfvio_filter* f, float pose_cov[36], float twist_cov[36]);
/* cov9N: room for 9 floats per landmark (ekfvio_num_features), in landmark order. */
EKFVIO_API int ekfvio_get_points_covariance(ekfvio_filter* f, float* cov9N);
/* The J above for a quaternion (w, x, y, z), row-major 3x4: a pure host function (no handle, no device) that compiles the very inline
 * function the kernels compile.  For a caller that keeps its own Sigma, or wants the body-frame (right-perturbation) convention:
 * R(q)^T J is that convention's Jacobian. */
EKFVIO_API int ekfvio_rotation_error_jacobian(const float q_wxyz[4], float J3x4[12]);

/* ---- KLT (KLTTracker::findNewFeaturePositions, KLTTracker.cpp:29-95) ----------------- */
/* Uploads a frame (Frame.h:25-41: image + intrinsics K row-major 3x3 as in CameraInfo.K),
 * builds its pyramid and Scharr derivatives on the device and makes it the current frame;
 * the former current frame becomes the previous one (frame_buffer depth 2, Params.h:58). */
EKFVIO_API int ekfvio_klt_push_frame(ekfvio_filter* f, const uint8_t* image, int32_t width, int32_t height, int32_t stride,
                          const float K[9]);
/* Tracks every landmark from the previous into the current frame: reference points are the
 * landmarks' last KLT results, initial guesses the EKF-predicted positions.  Outputs metric
 * z (2N), metric R (4N, 1e-5 px^2 scaled by 1/fx^2, 1/fy^2), pass (N).  Host pointers; any may be NULL. */
EKFVIO_API int ekfvio_klt_track(ekfvio_filter* f, float* z2N, float* R4N, uint8_t* passN);
/* Pixel-space tracking of arbitrary points (calcOpticalFlowPyrLK semantics with
 * OPTFLOW_USE_INITIAL_FLOW) between the two resident frames; for tests. */
EKFVIO_API int ekfvio_klt_track_points(ekfvio_filter* f, const float* prev_px, const float* init_px, int32_t count,
                            float* out_px, uint8_t* status);

/* ---- forward-backward check (not in the reference, whose tracker trusts every converged track) --------------------------------------
 * A Lucas-Kanade track can converge, with status 1, on the wrong piece of image: a neighbouring corner, or whatever now covers the
 * landmark.  The check tracks the forward result back into the previous frame and rejects the track if it does not come home.  It runs
 * on the device, in the tracker's own launch, in ekfvio_klt_track and ekfvio_step_image.  LK(template; search) is the tracker as it is
 * (calcOpticalFlowPyrLK with OPTFLOW_USE_INITIAL_FLOW: template window around a point of one frame, searched in the other frame from a
 * guess; result and status).  For a point with p: reference pixel in the previous frame, g: initial guess in the current frame (for a
 * landmark: its last KLT result and its predicted position, both in pixels), all in fp32, in this order, without fused multiply-add
 * (a NumPy float32 restatement of these lines around two calls of the oracle's tracker gives the same bits):
 *
 *     forward (unchanged):   (q, s_f) = LK(template: previous frame at p; search: current frame from g)
 *     if s_f == 1:
 *         bx = qx - (gx - px)          by = qy - (gy - py)        (the predicted flow, applied backwards)
 *         (r, s_b) = LK(template: current frame at q; search: previous frame from b)   same window, levels, iterations, epsilon, min_eigen
 *         dx = rx - px   dy = ry - py   e2 = dx*dx + dy*dy
 *         fb_ok  <=>  s_b == 1  and  e2 <= t2        t2 = max_px*max_px, formed once on the host in fp32; a NaN rejects
 *     pass = s_f == 1 and fb_ok and inside the kill pad (as today, on q)
 *
 * A point that fails the check takes in every respect the road of a point the tracker lost: pass = 0, z and R zero, no measurement
 * rows, last_klt kept, delete flag set by the update (TightlyCoupledEKF.cpp:526-529) -- and with cfg.remove_lost = 1 ekfvio_step_image
 * removes it in the same frame.  The innovation gate never sees it (its d2 is -1).  q is never changed by the backward pass.
 *
 * max_px > 0: on from the next track; max_px == 0: off (default; then no launch differs and every output keeps its bits).  Negative,
 * NaN: EKFVIO_EINVAL.  The value is cfg.klt_fb_max_px of ekfvio_create until this call replaces it. */
EKFVIO_API int ekfvio_set_klt_fb(ekfvio_filter* f, float max_px);
/* Results of the most recent checked track of the landmarks (any pointer may be NULL): err2 = e2 per landmark as defined above
 * (-1: the forward track failed, so the point was not evaluated; -2: the backward track failed) and a rejected flag per landmark
 * (s_f == 1 and not fb_ok), both with room for max_features entries; *n_landmarks = the landmark count that track saw (0 before the
 * first checked track); number rejected by that track; total since create/reset. */
EKFVIO_API int ekfvio_get_klt_fb(ekfvio_filter* f, float* err2, uint8_t* rejected, int32_t* n_landmarks, int32_t* rejected_last,
                                 int64_t* rejected_total);
/* The check in pixel space, for arbitrary points between the two resident frames (tests, callers with their own points): out_px and
 * status as ekfvio_klt_track_points gives them (status keeps its forward meaning).  The backward pass runs whatever the handle's
 * threshold is; with a threshold of 0, fb_ok means s_b == 1 alone.  back_px = r where s_f == 1 (whatever s_b is), else p; err2 as
 * above; fb_ok = 0 where s_f == 0.  Output pointers may be NULL.  Leaves the results ekfvio_get_klt_fb reports untouched. */
EKFVIO_API int ekfvio_klt_track_points_fb(ekfvio_filter* f, const float* prev_px, const float* init_px, int32_t count, float* out_px,
                                          uint8_t* status, float* back_px, float* err2, uint8_t* fb_ok);

/* ---- gain/offset term of the tracker (not in the reference, whose Lucas-Kanade assumes brightness constancy) --------------------------
 * Auto-exposure changes gain and offset between two consecutive frames: J(x + d) = alpha * I(x) + beta.  Then diff = J - I holds a
 * component in span{1, I} that brightness-constancy Lucas-Kanade reads as motion.  With the setting on, span{1, I} is projected out of the
 * template's two gradient images, once per pyramid level, which makes b = sum diff * (Ix, Iy) blind to that component (the "project-out"
 * form of Hager-Belhumeur and Baker-Matthews); the iteration itself is unchanged.  This covers every Lucas-Kanade pass: the forward pass,
 * the backward pass of the forward-backward check, ekfvio_klt_track, ekfvio_klt_track_points, ekfvio_klt_track_points_fb and
 * ekfvio_step_image.  The lines below are the specification; a NumPy restatement of one pass with them (tests/_klt_photo.py) is what the
 * device is held to, bit for bit.
 *
 * The pass forms the template's Iv[t], Ix[t], Iy[t] over the n = win * win window pixels exactly as without the term, as integers, at
 * every pyramid level, before A11, A12, A22 are formed.  Then:
 *
 *     sI = sum Iv   sX = sum Ix   sY = sum Iy   sII = sum Iv*Iv   sIX = sum Iv*Ix   sIY = sum Iv*Iy      exact integers (64-bit where needed)
 *     VI = n*sII - sI*sI      CX = n*sIX - sI*sX      CY = n*sIY - sI*sY                                  exact int64 (VI >= 0)
 *     mI = (float)sI / (float)n     mX = (float)sX / (float)n     mY = (float)sY / (float)n             fp32, each conversion rounds once
 *     cx = VI > 0 ? (float)CX / (float)VI : 0.0f          cy likewise                                     correctly rounded division
 *     Ix'[t] = clamp((int)rint(((float)Ix[t] - mX) - cx * ((float)Iv[t] - mI)), -4080, 4080)              fp32, no fused multiply-add, rint half to even
 *     Iy'[t] likewise with mY, cy
 *
 * After that, everything runs on Ix', Iy': A11, A12, A22, the min-eigenvalue test and every iteration's b1, b2.  Iv and diff are unchanged.
 * The clamp keeps every bound the kernel's integer sums rely on (factors fit 24 bits, per-lane partials stay below 2^28); it only bites
 * on degenerate templates.  A constant template has VI == 0: it gets the mean removed and then fails the min-eigenvalue test as before.
 * Out of scope: the sample-based R (cfg.sample_based_uncertainty), whose SSD weights remain brightness-dependent; a per-landmark exposure
 * state in the filter; affine window warps; the detector.
 *
 * on: 0 or 1, anything else EKFVIO_EINVAL.  A property of the handle: it holds from the next track and survives ekfvio_reset.  Off by
 * default (then no launch differs and every output keeps its bits); on, the tracker's launch is the kernel's second instance with the same
 * arguments, and nothing is allocated. */
EKFVIO_API int ekfvio_set_klt_photometric(ekfvio_filter* f, int32_t on);
/* The projection itself, Ix' and Iy' of `count` window pixels from their Iv, Ix, Iy (n = count): a pure host function (no handle, no
 * device) that compiles the very inline functions the kernel compiles, as ekfvio_rectify_map does; the six sums come from a loop here and
 * from a wavefront there.  count in [1, 441] and no NULL pointer, else EKFVIO_EINVAL.  An output may be its own input. */
EKFVIO_API int ekfvio_klt_project_gradients(const int32_t* Iv, const int32_t* Ix, const int32_t* Iy, int32_t count, int32_t* Ix_out,
                                            int32_t* Iy_out);

/* KLTTracker::estimateUncertaintySampleBased (KLTTracker.cpp:111-175) between the two resident frames: for every
 * point a pixel-space 2x2 covariance (row-major, px^2) from 25 samples (offsets -10..10 step 5 around cur_px) of 5x5
 * sub-pixel patches (cv::getRectSubPix semantics) weighted by exp(-0.01 * mean squared difference to the 5x5
 * reference patch at ref_px in the previous frame).  Host pointers. */
EKFVIO_API int ekfvio_klt_uncertainty_points(ekfvio_filter* f, const float* ref_px, const float* cur_px, int32_t count, float* cov4);

/* Test hook: interior of pyramid level `level` of the current frame (8-bit image, w*h, and
 * interleaved int16 Scharr dx,dy, w*h*2).  Either output may be NULL. */
EKFVIO_API int ekfvio_klt_get_level(ekfvio_filter* f, int32_t level, int32_t* w, int32_t* h, uint8_t* img, int16_t* deriv);

/* EKFVIO::addFrame + updateStateWithNewImage (EKFVIO.cpp:139-219) without the ROS
 * publishing: first frame only stores the image and stamp; later frames run
 * process(dt = stamp - t), then KLT + update if landmarks exist.  With cfg.replenish = 1 the
 * two replenishFeatures calls of addFrame (:154, :172) run on the device as well; with 0 the
 * caller adds landmarks (ekfvio_replenish, or its own detector + ekfvio_add_features).
 * The image is copied before the call returns; the call waits for the device once, at its end
 * (status word), the pass flags of the tracker never travel to the host.  With cfg.remove_lost = 1 the landmarks flagged by this
 * frame's update (or left flagged by an earlier frame) are removed behind the replenishment, before the frame's outputs; the count
 * of landmarks the call leaves behind arrives with the same status word.  That wait (here, in ekfvio_update and in
 * ekfvio_synchronize) polls a word the device writes into pinned host memory for up to 300 us of the calling
 * thread's time, then blocks in hipStreamSynchronize.
 * Returns EKFVIO_OK or EKFVIO_ENUMERIC. */
EKFVIO_API int ekfvio_step_image(ekfvio_filter* f, double stamp, const uint8_t* image, int32_t width, int32_t height,
                      int32_t stride, const float K[9]);

/* EKFVIO::replenishFeatures (EKFVIO.cpp:224-311) on the current frame: cv::FAST(threshold, nonmax) on the
 * (resized) image, occupancy circles of radius min_new_feature_dist around the landmarks' pixels, first fit
 * in detector order with the kill-box test, addNewFeatures(pixel2Metric(.)) until max_features landmarks
 * exist.  `added` (may be NULL) receives the number of new landmarks, new_px_xy (may be NULL, room for
 * 2*max_features ints) their pixels. */
EKFVIO_API int ekfvio_replenish(ekfvio_filter* f, int32_t* added, int32_t* new_px_xy);

/* ---- new landmarks spread over the image (not in the reference, whose replenishFeatures takes FAST keypoints in raster order, first fit: a
 * filter that needs a few landmarks gets them all from the top rows, one that needs many fills from the top left) -------------------------
 * For a monocular EKF the spread of bearings conditions rotation against translation.  With the setting on, the replenishment lays a grid of
 * cells over level 0 and takes, round by round, the strongest free corner of every cell, emptier cells first.  The corner score is the
 * detector's own (cornerScore, what ekfvio_fast_detect reports).  A 1 x 1 grid is "globally strongest corner first".  The lines below are
 * the specification; all of it is integer work, so there is no floating-point order to fix, and a pure-Python restatement of them
 * (tests/_replenish_grid.py) is what the device and ekfvio_replenish_select are held to, pixel for pixel and in order.
 *
 * Frame and keypoints:
 *     level 0 of the current frame is W x H
 *     FAST (threshold, nonmax, optional blur) gives keypoints k = 0..nk-1 in raster order with pixel (x_k, y_k) and score s_k, exactly as
 *     without the setting
 *     wanted = max_features - N_old      radius = min_new_feature_dist      pad = kill_pad
 * Cells:
 *     cw = ceil(W / cells_x)      ch = ceil(H / cells_y)
 *     cell(x, y) = (y / ch) * cells_x + x / cw                    integer division
 * Start:
 *     O = the occupancy image as without the setting: B of ekfvio_set_mask where that is on, else empty
 *     stamp the circle of every landmark in the state at cvRound(u fx + cx, v fy + cy); flagged landmarks are included, as without the setting
 *     cnt[c] = the number of those landmarks whose rounded pixel lies inside [0,W) x [0,H) and in cell c
 *     added = 0
 * Repeat while added < wanted:
 *     1. a keypoint is a candidate when it passes the kill-box test (Frame::isPixelInBox, as without the setting) and O(x_k, y_k) == 0
 *     2. best[c] = the candidate of cell c with the largest s_k, ties to the smallest k; if no cell has one, stop
 *     3. L = the cells that have a best, ordered by cnt[c] ascending, then s descending, then k ascending (integer comparisons; no two keys
 *        are equal); cnt is read as it stood at the start of the round
 *     4. walk through L in order and stop at added == wanted: if O(x, y) is still 0, take the keypoint -- new_xy[added] and new_uv[added]
 *        by Feature::pixel2Metric as without the setting, added++, stamp its circle into O, cnt[c]++; otherwise skip it (a neighbouring
 *        cell's winner has covered it)
 * The first entry of L is always taken, so the loop ends after at most `wanted` rounds.
 *
 * What it does not do: another detector or score, sub-pixel refinement of the new corners, a cap on the landmarks per cell, removing landmarks
 * to rebalance the cells; ekfvio_add_features is untouched (a caller's own detector is the caller's business).
 *
 * ekfvio_set_replenish_grid.  (0, 0): off (default; then no launch differs, nothing is allocated and every output keeps its bits).  On: both
 * values >= 1 and cells_x * cells_y <= 256; anything else EKFVIO_EINVAL, and the setting stays what it was.  A property of the handle, not of
 * ekfvio_config: it holds from the next replenishment (ekfvio_replenish, and ekfvio_step_image with cfg.replenish = 1), survives ekfvio_reset and
 * drops no captured graph (the replenishment is in none).  On, the selection stays one launch of one workgroup, the kernel's grid instance; it
 * then passes over the keypoints once per round instead of once (README, "new landmarks spread over the image", has the measured cost). */
EKFVIO_API int ekfvio_set_replenish_grid(ekfvio_filter* f, int32_t cells_x, int32_t cells_y);
/* Reads the setting back (either pointer may be NULL). */
EKFVIO_API int ekfvio_get_replenish_grid(ekfvio_filter* f, int32_t* cells_x, int32_t* cells_y);
/* The selection itself: a pure host function (no handle, no device) that compiles the very inline functions the kernel compiles
 * (csrc/select.h: cell(), the keys and their order, the kill-box test, the circle's rows), as ekfvio_rectify_map and ekfvio_zupt_decide do; the
 * cells' maxima come from a loop here and from LDS atomics there.  kp_xy, score: `count` keypoints in raster order, x,y interleaved, inside the
 * frame, scores >= 0.  existing_px_xy: the rounded pixels of the n_existing landmarks in the state (any value; outside the frame they count for no
 * cell).  blocked: one byte per level-0 pixel, non-zero = blocked (ekfvio_mask_blocked's output), or NULL.  new_xy: room for 2 * wanted ints.
 * cells_x = cells_y = 0: the raster first fit of ekfvio_replenish without the setting.  A NULL among the needed pointers, a negative count, a
 * keypoint outside the frame, a radius outside [0, 63], or a grid that ekfvio_set_replenish_grid would refuse: EKFVIO_EINVAL. */
EKFVIO_API int ekfvio_replenish_select(const int32_t* kp_xy, const int32_t* score, int32_t count, const int32_t* existing_px_xy,
                                       int32_t n_existing, const uint8_t* blocked, int32_t W, int32_t H, int32_t radius, int32_t kill_pad,
                                       int32_t cells_x, int32_t cells_y, int32_t wanted, int32_t* new_xy, int32_t* added);
/* Test hook: cv::FAST(level 0 of the current frame, blurred first if cfg.fast_blur_sigma != 0, threshold, nonmax),
 * TYPE_9_16, keypoints in raster order. */
EKFVIO_API int ekfvio_fast_detect(ekfvio_filter* f, int32_t threshold, int32_t nonmax, int32_t cap, int32_t* xy, int32_t* score,
                       int32_t* count);
/* EKFVIO::imu_callback (EKFVIO.cpp:113-115), a logging stub in the reference: with cfg.use_imu = 0 (default) this does
 * nothing.  With cfg.use_imu = 1 the record first propagates the filter to its stamp -- process(dt = stamp - t),
 * the reference's motion model; the first record or frame only sets t -- and then updates with z = [gyro; accel],
 * h = [omega + b_gyr; a + b_acc - R(q)^T gravity], Joseph form (specification: oracle/ekf_oracle.hpp imu_update).
 * EKFVIO_EINVAL for a stamp before the filter's time.  Asynchronous. */
EKFVIO_API int ekfvio_imu(ekfvio_filter* f, double stamp, const float gyro[3], const float accel[3]);
/* The update alone (no propagation), whatever cfg.use_imu says: for tests and callers that propagate themselves. */
EKFVIO_API int ekfvio_imu_update(ekfvio_filter* f, const float gyro[3], const float accel[3]);

/* ---- the IMU in its own frame; gravity at run time (not in the reference, which has no IMU update) -------------------------------------------
 * The filter's body frame is the camera's optical frame (z forward, y down), and the model above takes the IMU's axes to be the camera's and
 * the sensor to sit in the optical centre.  ekfvio_set_imu_extrinsics gives the update the calibration every visual-inertial rig has:
 *
 *     R_ci  row-major 3 x 3, maps IMU coordinates to camera coordinates, v_cam = R_ci v_imu: the rotation block of Kalibr's T_cam_imu
 *     p_ci  the IMU's origin in the camera frame, metres: T_cam_imu's translation
 *           (EuRoC's T_BS with B = IMU is the inverse transform: R_ci = R_BS^T, p_ci = -R_BS^T p_BS)
 *
 * With them h(x) = [M omega + b_gyr ; M (a + omega x (omega x p) - R(q)^T g) + b_acc], M = R_ci^T.  The biases live in the sensor's own axes
 * (the IMU frame), where they physically are.  The accelerometer at p reads the centripetal term omega x (omega x p) more than the optical
 * centre does; the angular-acceleration term alpha x p is NEGLECTED: the state has no alpha, the motion model holds omega constant between
 * updates.  R = diag(gyro_var x3, accel_var x3) is isotropic per sensor and means the same in either frame.
 *
 * The lines below are the specification of the part in front of H and y; from H and y on the update is ekfvio_imu_update's, line for line
 * (W = H Sigma, S = W H^T + R, Cholesky, the gains per state row over all sixteen columns, T, G, the mean, the quaternion's renormalisation,
 * the Joseph pass).  Everything in fp32 without fused multiply-add, every sum associated as the brackets say; a NumPy restatement
 * (tests/_imu_extrinsics.py: kernel_order_fp32_ext) is what the device and ekfvio_imu_model are held to, bit for bit.
 * M[r][k] = R_ci[3 k + r]; w = mu[10..12], a = mu[13..15], p = p_ci; rg = R(q)^T g and jac = d rg / d(qw, qx, qy, qz) (3 x 4) as in the
 * model without extrinsics; cross(u, v) = (u_1*v_2 - u_2*v_1, u_2*v_0 - u_0*v_2, u_0*v_1 - u_1*v_0).
 *
 *     t = cross(w, p)        c = cross(w, t)
 *     s_k  = (a_k + c_k) - rg_k
 *     hg_r = ((M[r][0]*w_0 + M[r][1]*w_1) + M[r][2]*w_2) + mu[19+r]
 *     ha_r = ((M[r][0]*s_0 + M[r][1]*s_1) + M[r][2]*s_2) + mu[16+r]
 *     y_r  = gyro_r - hg_r        y_{3+r} = accel_r - ha_r
 *     d = (w_0*p_0 + w_1*p_1) + w_2*p_2
 *     C[i][j] = (w_i*p_j - (2*p_i)*w_j) + (i == j ? d : nothing added)                                   = d c / d w
 *     H on the sixteen state columns {3..6, 10..21}, position in that list in brackets, zero elsewhere:
 *       gyro row r :  omega [4+k] = M[r][k]         b_gyr [13+r] = 1
 *       accel row r:  q     [k]   = -((M[r][0]*jac[0][k] + M[r][1]*jac[1][k]) + M[r][2]*jac[2][k])      k = 0..3
 *                     omega [4+k] =   (M[r][0]*C[0][k]   + M[r][1]*C[1][k])   + M[r][2]*C[2][k]         k = 0..2
 *                     a     [7+k] = M[r][k]         b_acc [10+r] = 1
 *
 * ekfvio_set_imu_extrinsics.  Both pointers NULL: off (default; then no launch differs, nothing is allocated and every output keeps its
 * bits).  One NULL and the other not, a non-finite entry, det(R_ci) <= 0, or max |R_ci R_ci^T - I| > 1e-3 (evaluated in fp64 from the fp32
 * entries): EKFVIO_EINVAL, and the setting stays what it was.  The bound is a condition, not a measurement: a calibration printed to four
 * decimals passes it; a row-major / column-major mix-up cannot be told from a rotation and passes too, but a reflection, a scaled matrix or
 * the first nine numbers of a 4 x 4 with a translation in them do not; what it lets through scales gravity by at most about 1e-2 m/s^2,
 * against an accelerometer sigma of 0.1.  The values are stored as given, not re-orthonormalised.  A property of the handle, not of
 * ekfvio_config: it holds from the next IMU update (ekfvio_imu, ekfvio_imu_update), survives ekfvio_reset and drops no captured graph (the IMU
 * update is in none).  On, the update stays two launches on sixteen state columns; only H and the residual get denser. */
EKFVIO_API int ekfvio_set_imu_extrinsics(ekfvio_filter* f, const float R_ci[9], const float p_ci[3]);
/* Reads the setting back (any pointer may be NULL): the values as given and *on = 1; with the setting off the identity, zeros and *on = 0. */
EKFVIO_API int ekfvio_get_imu_extrinsics(ekfvio_filter* f, float R_ci[9], float p_ci[3], int32_t* on);
/* Replaces cfg.gravity (the gravity vector in the filter's world frame, m/s^2) from the next IMU update on; survives ekfvio_reset.  cfg.gravity's
 * default (0, 9.81, 0) assumes a camera that is level at the first frame; a rig that starts tilted has another g for its whole life (see
 * ekfvio_gravity_from_accel).  A non-finite value: EKFVIO_EINVAL, and the setting stays.  ekfvio_get_gravity reads it back. */
EKFVIO_API int ekfvio_set_gravity(ekfvio_filter* f, const float g[3]);
EKFVIO_API int ekfvio_get_gravity(ekfvio_filter* f, float g[3]);
/* The gravity vector in the camera frame of a rig AT REST whose accelerometer reads mean_accel on average (IMU axes; its bias negligible against
 * 9.81): g = -(R_ci mean_accel) * (magnitude > 0 ? magnitude / |mean_accel| : 1), evaluated in fp64 and rounded to fp32.  That frame is the
 * filter's world frame while q = (1, 0, 0, 0).  R_ci may be NULL: the identity.  A pure host function: no handle, no device.
 * |mean_accel| == 0 or a non-finite input: EKFVIO_EINVAL. */
EKFVIO_API int ekfvio_gravity_from_accel(const float R_ci[9], const double mean_accel[3], float magnitude, float g_out[3]);
/* The model alone: the residual y[6] and the 6 x 16 Jacobian H (row-major, on the sixteen state columns {3..6, 10..21}) of one IMU record at
 * the base state base_mu[22] with gravity g.  A pure host function (no handle, no device) that compiles the very inline functions the
 * kernel compiles (csrc/imu_model.h), as ekfvio_zupt_decide and ekfvio_rectify_map do.  R_ci = p_ci = NULL: the model without extrinsics.
 * A NULL among the other arguments, one of R_ci / p_ci NULL alone, or extrinsics that ekfvio_set_imu_extrinsics would refuse: EKFVIO_EINVAL. */
EKFVIO_API int ekfvio_imu_model(const float base_mu[22], const float g[3], const float R_ci[9], const float p_ci[3], const float gyro[3],
                                const float accel[3], float y[6], float H[96]);

/* ---- zero-velocity update (not in the reference, whose filter learns that the camera stands still only through noisy pixel measurements of
 * landmarks at uncertain depth, against a motion model whose Q keeps re-inflating velocity, body rate and acceleration) --------------------
 * A decision per frame, on the device, from the tracker's results, and -- when it says the camera stands still -- a pseudo-measurement
 * z = 0 of the velocity and the body rate.  The lines below are the specification: everything in fp32, the association order fixed, without
 * fused multiply-add, division and square root correctly rounded; a NumPy restatement of them (tests/_zupt.py) is what the device is held
 * to, bit for bit.
 *
 * Decision, per frame of ekfvio_step_image, behind the tracker, in front of the update's measurement bookkeeping and the innovation gate.
 * pass[i]: the tracker's final verdict as the update would receive it (behind the forward status, the forward-backward check, the kill box
 * and the mask).  (qx, qy): the tracked pixel.  (px, py): the reference pixel as the tracker forms it, last_klt[2i] * fx + cx and
 * last_klt[2i+1] * fy + cy with the PREVIOUS frame's intrinsics (multiply, then add).
 *
 *     for pass[i] != 0:   dx = qx - px    dy = qy - py    e2 = dx*dx + dy*dy    still_i  <=>  e2 <= t2
 *                         (t2 = max_flow_px*max_flow_px, formed once on the host in fp32; a NaN is not still)
 *     n_pass = #pass      n_still = #still
 *     stationary  <=>  n_pass >= min_tracks  and  (float)n_still >= min_ratio * (float)n_pass
 *     flow2[i] = e2, or -1 where pass[i] == 0
 *
 * Update, when stationary, on the propagated state, in front of the camera update (the gate and the camera update then read the state it
 * leaves): z = 0 on h(x) = [vel (mu[7..9]); omega (mu[10..12])], H the selection of state rows 7..12, R = diag(R_0 .. R_5) with
 * R_0..2 = vel_variance and R_3..5 = omega_variance, Joseph form.  It is the IMU update's arithmetic (ekfvio_imu_update) with H a selection.
 * P(i,j) is Sigma's element in row i, column j AS STORED (both triangles agree only up to rounding); r, s, c run over 0..5 and every sum
 * runs over an ascending index and associates to the left, starting from its first written term:
 *
 *     S(r,s) = P(7+r, 7+s) + (r == s ? R_r : nothing added)               r >= s: the lower triangle alone is read
 *     L: left-looking Cholesky, for j = 0..5:   d = S(j,j) - L(j,0)*L(j,0) - ... - L(j,j-1)*L(j,j-1)      L(j,j) = sqrt(d)
 *                                  for r > j:   v = S(r,j) - L(r,0)*L(j,0) - ... - L(r,j-1)*L(j,j-1)      L(r,j) = v / L(j,j)
 *     y_r = -mu[7+r]
 *     per state row i = 0 .. n-1:
 *         x_r = P(i, 7+r)          w_r = P(7+r, i)
 *         forward,  r = 0..5:      k_r = (x_r - k_0*L(r,0) - ... - k_{r-1}*L(r,r-1)) / L(r,r)
 *         backward, r = 5..0:      k_r = (k_r - k_{r+1}*L(r+1,r) - ... - k_5*L(5,r)) / L(r,r)
 *         t_c = x_c - k_0*P(7,7+c) - ... - k_5*P(12,7+c)
 *         g_r = k_r*R_r - t_r
 *         dm  = 0 + k_0*y_0 + ... + k_5*y_5
 *         mu'_i = mu_i + dm
 *     quaternion: qn = sqrt(mu'_3*mu'_3 + mu'_4*mu'_4 + mu'_5*mu'_5 + mu'_6*mu'_6), mu'_3..6 divided by qn
 *     Sigma'(i,j) = flush((P(i,j) - k_0(i)*w_0(j) - ... - k_5(i)*w_5(j)) + g_0(i)*k_0(j) + ... + g_5(i)*k_5(j))
 *     flush(v) = v where |v| > 1e-8f * 1e-5f, else 0 (the reference's prune)
 *
 * When not stationary, Sigma is untouched and the mean keeps every bit (the mean is updated in place: nothing is copied or swapped).  The
 * landmarks' last KLT results, delete flags, ids and birth stamps are never touched.  Behind an aborted persistent sweep the camera update
 * runs again from the state this update left; the zero-velocity update is not repeated.  ekfvio_run_uploaded and its captured graphs carry no
 * tracker results and run none; ekfvio_klt_track + ekfvio_update get none automatically: their caller decides and calls
 * ekfvio_zupt_update.
 *
 * What it does not do.  It is for standing still, not for braking: slammed onto the first frame of an abrupt stop it moves the position
 * through the cross-covariances by more than the filter's own convergence would (README, "zero-velocity update").  A distant scene under slow
 * translation looks still in pixels: no threshold is recommended beyond "off".  Acceleration and the biases are not measured.  The camera update
 * is not skipped.
 *
 * ekfvio_set_zupt.  max_flow_px == 0: off (default; then no launch differs, nothing is allocated and every output keeps its bits; the other
 * arguments are not looked at).  On: max_flow_px finite and > 0, min_tracks >= 1, 0 < min_ratio <= 1, both variances finite and > 0; anything
 * else EKFVIO_EINVAL, and the setting stays what it was.  A property of the handle: it holds from the next frame, survives ekfvio_reset (the
 * counts start over, as the gate's) and drops no captured graph.  On, it costs two launches per frame with landmarks -- every workgroup of the
 * gain kernel evaluates the decision for itself, and both kernels return at once on a "no" -- and 16 bytes of device and 16 + 4 max_features
 * bytes of pinned host memory, taken when it is first turned on. */
EKFVIO_API int ekfvio_set_zupt(ekfvio_filter* f, float max_flow_px, int32_t min_tracks, float min_ratio, float vel_variance,
                               float omega_variance);
/* The update alone, unconditional, whatever the setting says: for tests and for callers with a stop detector of their own (wheel odometry).
 * Both variances finite and > 0, else EKFVIO_EINVAL.  Asynchronous, as ekfvio_imu_update. */
EKFVIO_API int ekfvio_zupt_update(ekfvio_filter* f, float vel_variance, float omega_variance);
/* The decision of the most recent frame of ekfvio_step_image (any pointer may be NULL): flow2 per landmark as defined above, with room for
 * max_features entries; *n_landmarks = the landmark count that decision saw (indices are its indices, before any removal or replenishment of
 * the same frame); n_pass, n_still; *applied_last = 1 where that frame's update ran; the number of frames it ran in since create / reset.
 * A frame without a decision (the first frame, no landmark) reports zeros, and so does a handle with the setting off.  A memcpy: the
 * decision's words and flow2 arrive in pinned host memory in front of the frame's status word. */
EKFVIO_API int ekfvio_get_zupt(ekfvio_filter* f, float* flow2N, int32_t* n_landmarks, int32_t* n_pass, int32_t* n_still,
                               int32_t* applied_last, int64_t* applied_total);
/* The decision itself for `count` points: a pure host function (no handle, no device) that compiles the very inline functions the kernels
 * compile, as ekfvio_rectify_map does; the two counts come from a loop here and from wavefront ballots there.  prev_px, cur_px: the reference
 * and the tracked pixels, x,y interleaved; pass: one byte each.  flow2 (room for count entries), n_pass, n_still, stationary may be NULL.
 * A negative count, NULL inputs with count > 0, or max_flow_px, min_tracks, min_ratio that ekfvio_set_zupt would refuse as "on": EKFVIO_EINVAL. */
EKFVIO_API int ekfvio_zupt_decide(const float* prev_px, const float* cur_px, const uint8_t* pass, int32_t count, float max_flow_px,
                                  int32_t min_tracks, float min_ratio, float* flow2, int32_t* n_pass, int32_t* n_still, int32_t* stationary);

/* ---- linear aiding measurements of the base state (not in the reference, whose monocular filter has no metric input: with cfg.use_imu = 0 its
 * scale is set by default_point_depth and nothing else) ----------------------------------------------------------------------------------
 * z = H x[0:22] + v, v ~ N(0, R): k = 1..6 rows, H dense k x 22 row-major over the base state (pos 0..2, q 3..6, vel 7..9, omega 10..12,
 * a 13..15, b_acc 16..18, b_gyr 19..21), R full symmetric k x k row-major of which the LOWER triangle alone is read, Joseph form, on the
 * device.  Wheel speed, a position or altitude fix, a nonholonomic constraint.  The lines below are the specification: everything in fp32,
 * without fused multiply-add, division and square root correctly rounded, every sum over an ascending index, associated to the left and
 * starting from its first written term; a NumPy restatement of them (tests/_aid.py: kernel_order_fp32) is what the device is held to, bit
 * for bit.  P(i,j) is Sigma's element in row i, column j AS STORED; r, s run over 0..k-1, c over 0..21; R(r,s) with r < s reads R(s,r).
 *
 *     w_r(i) = H(r,0)*P(0,i) + ... + H(r,21)*P(21,i)          x_r(i) = P(i,0)*H(r,0) + ... + P(i,21)*H(r,21)      (all 22 terms, zeros of H included)
 *     A(r,s) = w_r(0)*H(s,0) + ... + w_r(21)*H(s,21)          (all k x k elements: t below reads both triangles)
 *     S(r,s) = A(r,s) + R(r,s)                                r >= s: the lower triangle alone is factored
 *     y_r    = z_r - (H(r,0)*mu_0 + ... + H(r,21)*mu_21)
 *     L: left-looking Cholesky, for j = 0..k-1:   d_j = S(j,j) - L(j,0)*L(j,0) - ... - L(j,j-1)*L(j,j-1)    L(j,j) = sqrt(d_j)
 *                                    for r > j:   v = S(r,j) - L(r,0)*L(j,0) - ... - L(r,j-1)*L(j,j-1)      L(r,j) = v / L(j,j)
 *        (it stops at the first pivot d_j that is not finite and > 0; d2 is then a NaN)
 *     e_r = (y_r - e_0*L(r,0) - ... - e_{r-1}*L(r,r-1)) / L(r,r)          d2 = e_0*e_0 + ... + e_{k-1}*e_{k-1}
 *     accepted  <=>  every pivot d_j finite and > 0   and   (chi2 == 0  or  d2 <= chi2)       (a NaN among the pivots, or a NaN d2 under a gate, rejects)
 *     accepted, per state row i = 0 .. n-1 (x_r = x_r(i), w_r = w_r(i)):
 *         forward,  r = 0..k-1:    k_r = (x_r - k_0*L(r,0) - ... - k_{r-1}*L(r,r-1)) / L(r,r)
 *         backward, r = k-1..0:    k_r = (k_r - k_{r+1}*L(r+1,r) - ... - k_{k-1}*L(k-1,r)) / L(r,r)
 *         t_c = x_c - k_0*A(0,c) - ... - k_{k-1}*A(k-1,c)
 *         g_r = (k_0*R(0,r) + ... + k_{k-1}*R(k-1,r)) - t_r
 *         dm  = 0 + k_0*y_0 + ... + k_{k-1}*y_{k-1}
 *         mu'_i = mu_i + dm
 *     quaternion: qn = sqrt(mu'_3*mu'_3 + mu'_4*mu'_4 + mu'_5*mu'_5 + mu'_6*mu'_6), mu'_3..6 divided by qn
 *     Sigma'(i,j) = flush((P(i,j) - k_0(i)*w_0(j) - ... - k_{k-1}(i)*w_{k-1}(j)) + g_0(i)*k_0(j) + ... + g_{k-1}(i)*k_{k-1}(j))
 *     flush(v) = v where |v| > 1e-8f * 1e-5f, else 0 (the reference's prune)
 *
 * Not accepted: Sigma is untouched and the mean keeps every bit (the mean is updated in place: nothing is copied or swapped).  The landmarks'
 * last KLT results, delete flags, ids and birth stamps are never touched either way.  With H the selection of state rows 7..12, z = 0 and a
 * diagonal R these lines are the zero-velocity update's (ekfvio_zupt_update), bit for bit.
 *
 * What it does not do.  H has no landmark columns and the measurement is linear: no range, no bearing, no attitude given as a quaternion.
 * Stamps must not run backwards.  A position fix is taken in the filter's own world frame (the camera's first pose): aligning a geodetic
 * frame with it is the caller's.  An altitude-only row makes nothing observable on a trajectory without vertical motion.
 *
 * Two launches per update, instantiated per k (a one-row update does not pay for six); H, z, R and chi2 travel as kernel arguments; both
 * kernels return at once on "not accepted".  The first aiding call of a handle takes 32 bytes of device and 32 bytes of pinned host memory.
 * Every entry point validates on the host and returns EKFVIO_EINVAL with nothing changed for: k outside 1..6, a NULL pointer, a non-finite
 * entry, chi2 < 0 or not finite, R not positive definite (fp64 Cholesky of the lower triangle).  All are asynchronous, as ekfvio_imu_update.
 *
 * ekfvio_aid_update: the update alone on the state as it stands. */
EKFVIO_API int ekfvio_aid_update(ekfvio_filter* f, int32_t k, const float* H, const float* z, const float* R, float chi2);
/* Propagates to `stamp` first, exactly as ekfvio_imu does with cfg.use_imu = 1 and whatever cfg.use_imu says: process(dt = stamp - t), then
 * the update.  The first stamp a handle sees only sets its time (nothing is applied); a stamp before the filter's time: EKFVIO_EINVAL. */
EKFVIO_API int ekfvio_aid(ekfvio_filter* f, double stamp, int32_t k, const float* H, const float* z, const float* R, float chi2);
/* A standing measurement, applied in every frame of ekfvio_step_image behind the first: behind the tracker, in front of the zero-velocity
 * update, the innovation gate and the camera update (which read the state it leaves), and outside what an aborted persistent sweep runs
 * again.  For constraints that need no sensor: the nonholonomic v_x = v_y = 0 of a forward-looking camera on a car, a planar robot's
 * v_y = 0.  k = 0: off (default; then no launch differs, nothing is allocated and every output keeps its bits; the other arguments are not
 * looked at).  A property of the handle: it holds from the next frame, survives ekfvio_reset (the counts start over) and drops no captured
 * graph (ekfvio_run_uploaded carries none).  A refused call leaves the setting what it was. */
EKFVIO_API int ekfvio_set_frame_aid(ekfvio_filter* f, int32_t k, const float* H, const float* z, const float* R, float chi2);
/* The most recent aiding update of the handle, standing or called (any pointer may be NULL): d2, the normalised innovation squared -- the
 * consistency figure R is tuned by: over many updates its mean should be near k; a NaN where a pivot failed --, *accepted_last, and how many
 * were applied and rejected since create / reset.  The gain kernel's first workgroup writes them into pinned host memory: behind
 * ekfvio_step_image this is a memcpy; behind a bare ekfvio_aid / ekfvio_aid_update it waits for the handle's stream.  Zeros on a handle
 * that never ran one. */
EKFVIO_API int ekfvio_get_aid(ekfvio_filter* f, float* d2_last, int32_t* accepted_last, int64_t* applied_total, int64_t* rejected_total);
/* The residual y[k], S[k*k] (row-major, S = A + R in full), d2 and *pd (1: every pivot finite and > 0; else 0 and d2 a NaN) of the lines
 * above, from base_mu[22] and Sigma's 22 x 22 base block (row-major, element (i,j) at 22 i + j), which is all of Sigma that enters them.
 * A pure host function (no handle, no device) that compiles the very inline functions the kernels compile (csrc/aid.h), as
 * ekfvio_zupt_decide and ekfvio_imu_model do.  y, S, d2, pd may be NULL.  What the entry points above refuse, a NULL base_mu or Sigma_bb, or
 * a non-finite entry of either: EKFVIO_EINVAL. */
EKFVIO_API int ekfvio_aid_innovation(const float base_mu[22], const float* Sigma_bb, int32_t k, const float* H, const float* z, const float* R,
                                     float* y, float* S, float* d2, int32_t* pd);
/* The three rows of a velocity v measured in a vehicle frame whose axes map to the camera's by R_cv (row-major, v_cam = R_cv v_vehicle) and
 * whose origin sits at p_cv in the camera frame: z = M (vel + omega x p_cv), M = R_cv^T, linear in state rows 7..12 (the angular-acceleration
 * term is neglected, as in the IMU model):
 *     H(r, 7+j) = M[r][j]        H(r, 10+j) = (M[r][0]*C[0][j] + M[r][1]*C[1][j]) + M[r][2]*C[2][j]        zero elsewhere
 *     M[r][j] = R_cv[3 j + r]    C = [[0, p_2, -p_1], [-p_2, 0, p_0], [p_1, -p_0, 0]]
 * H[66], z[3] = v, R[9] = cov with its lower triangle mirrored.  R_cv, p_cv NULL: the identity, zero.  A pure host function.  A NULL among
 * the others, a non-finite entry, an R_cv that ekfvio_set_imu_extrinsics would refuse, or a cov that is not positive definite: EKFVIO_EINVAL. */
EKFVIO_API int ekfvio_aid_rows_body_velocity(const float R_cv[9], const float p_cv[3], const float v[3], const float cov[9], float* H, float* z,
                                             float* R);

/* ---- device-resident measurement sequences (benchmark / replay) ---------------------- */
/* Copies `frames` consecutive (z, R, pass) triples for the current landmark count to HBM. */
EKFVIO_API int ekfvio_upload_measurements(ekfvio_filter* f, int32_t frames, const float* z, const float* R, const uint8_t* pass);
/* Runs process(dt) + update(frame i) for i = first .. first+count-1 (indices wrap modulo the
 * uploaded frame count) with no host<->device traffic.  Asynchronous; pair with
 * ekfvio_synchronize.  count = 0 runs nothing but prepares the launch graphs the runs replay (their
 * capture costs milliseconds: a caller that times a run prepares first). */
EKFVIO_API int ekfvio_run_uploaded(ekfvio_filter* f, int32_t first, int32_t count, float dt);
/* Waits for the handle's stream.  Returns EKFVIO_ENUMERIC (once) if a run since the last status read met a
 * non-positive pivot (reference: ROS_ERROR_COND at TightlyCoupledEKF.cpp:579, continues); EKFVIO_EABORTED if a persistent
 * sweep of the run gave up (the updates behind it were skipped; see the enum); else EKFVIO_OK. */
EKFVIO_API int ekfvio_synchronize(ekfvio_filter* f);

/* ---- instrumentation ----------------------------------------------------------------- */
/* Per-kernel-class device time accumulated with HIP events on the handle's stream while
 * profiling is on.  Classes: see ekfvio_profile_name.  Times in milliseconds. */
EKFVIO_API int ekfvio_profile_enable(ekfvio_filter* f, int32_t on);
EKFVIO_API int ekfvio_profile_reset(ekfvio_filter* f);
EKFVIO_API int ekfvio_profile_count(void);
EKFVIO_API const char* ekfvio_profile_name(int32_t cls);
EKFVIO_API int ekfvio_profile_get(ekfvio_filter* f, int32_t cls, double* total_ms, int64_t* launches, double* flops);
/* Mean launch duration (us) of the P-update GEMM(s) at the shape of the most recent update -- Sigma' = T + G K^T, and,
 * where the sweep does not produce T itself (EKFVIO_SCHUR=0, m >= 1024), T = Sigma - K W as well -- `reps` repetitions
 * replayed back to back from one hipGraph between two HIP events on the handle's stream; results go to scratch, the
 * state is untouched.  flops_per_launch (may be NULL) = the flops a launch EXECUTES, averaged over the update's P-update
 * launches: 2 n n m_pad, less where the second Joseph GEMM forms the lower triangle's tiles only (N > 334, round 6). */
EKFVIO_API int ekfvio_profile_update_gemms(ekfvio_filter* f, int32_t reps, double* avg_launch_us, double* flops_per_launch);

/* Diagnostic counters of a handle (no device work): counters[0] Cholesky sweeps that went out as the single persistent launch
 * (chol_persist_kernel; the others took one launch per block step), [1] sweeps with Sigma and the gain as Schur tiles (EKFVIO_SCHUR=1),
 * [2] updates run again behind an aborted persistent sweep, [3] the handle's sweep mode now (2: persistent where it applies, 0: one launch
 * per block step), [4] frames of ekfvio_step_image whose outputs and status were published in front of the update's last GEMM,
 * [5] updates whose right Joseph factor T2 = Sigma (I - K H)^T came out of the Cholesky sweep's launch (or the tile kernel that stands in for
 * it behind a per-step sweep), leaving ONE P-update GEMM behind it (where the fused persistent launch forms the gain: about 65 .. 265
 * landmarks, all measured), [6] filter steps of ekfvio_run_uploaded enqueued as replays of its captured graphs (the others ran as eager launches),
 * [7] process(dt) launches, replayed or eager, that found their linearisation and mean propagation already done by the previous update's
 * one P-update GEMM (inside a replayed graph of S steps in the T2 flow: S - 1 of them; EKFVIO_LIN_OVERLAP=0: none). */
EKFVIO_API int ekfvio_get_counters(ekfvio_filter* f, int64_t counters[8]);

#ifdef __cplusplus
}
#endif
#endif /* EKFVIO_H_ */
