// ekf_vio_amd/host/ekfvio.hpp — header-only C++ host shim over the C-ABI (include/ekfvio.h).
//
// Mirrors the three classes EKFVIO::addFrame touches in the reference, with the same member
// names and argument meaning, so that the reference's node (include/ekf_vio/EKFVIO.cpp) can
// swap its `TightlyCoupledEKF tc_ekf; KLTTracker tracker;` members (EKFVIO.h:70-72) for these
// and keep its call sites:
//   reference                                              here
//   tc_ekf.process(dt)                    EKFVIO.cpp:163   TightlyCoupledEKF::process
//   tc_ekf.previousFeaturePositionVector  EKFVIO.cpp:216   (kept on the device; getter provided)
//   tracker.findNewFeaturePositions(...)  EKFVIO.cpp:216   KLTTracker::findNewFeaturePositions
//   tc_ekf.updateWithFeaturePositions     EKFVIO.cpp:218   TightlyCoupledEKF::updateWithFeaturePositions
//   tc_ekf.addNewFeatures                 EKFVIO.cpp:308   TightlyCoupledEKF::addNewFeatures
// Eigen/OpenCV types are replaced by plain structs with the same memory layout
// (Eigen::Vector2f = 2 floats, Eigen::Matrix2f = 4 floats column-major, cv::Mat 8UC1 = pointer
// + step).  Errors the reference would ROS_ASSERT on surface as ekfvio::Error.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <deque>
#include <fstream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/ekfvio.h"

namespace ekfvio {

using Vector2f = std::array<float, 2>;
using Matrix2f = std::array<float, 4>;  // column-major
using Vector3f = std::array<float, 3>;

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

// EKFVIO::EKFVIO's parameter block (EKFVIO.cpp:19-67, defaults Params.h:18-125) without ROS: the node's private
// parameter names (without the "~") mapped onto ekfvio_config; node-level names (topics, frames, switches) are kept as
// strings for the node shim; parameters of subsystems the reference no longer calls (moba / sba / depth updates /
// variance boxes, all unused on the hot path) are accepted and ignored.  Unknown names are an error (a typo in a launch
// file should not pass silently).  Values arrive as text, as in a launch file or a `rosparam dump`.
struct Params {
    ekfvio_config cfg;
    float gate_chi2 = 0.f;  // not a field of ekfvio_config: set on the handle behind ekfvio_create (ekfvio_set_gate); 0 = off
    // Not in the reference, whose deployment rectifies in front of the node (image_proc/rectify): with rectify = 1 the camera topic carries RAW
    // frames and the handle rectifies them on the device (ekfvio_set_distortion).  The plumb_bob coefficients k1 k2 p1 p2 k3 come from
    // CameraInfo.D (the ROS node) or from the distortion_* parameters (a caller without CameraInfo, the replay driver); all zero = off.
    int rectify = 0;
    std::array<double, 5> distortion{};
    // Other lenses, another rectified camera (ekfvio_set_camera_model).  distortion_model: CameraInfo.distortion_model's names, "plumb_bob"
    // (default), "rational_polynomial" (k1 k2 p1 p2 k3 k4 k5 k6) or "equidistant" / "fisheye" (k1 k2 k3 k4); distortion_k4..k6 are the
    // coefficients the plumb_bob parameters lack.  rectified_fx/fy/cx/cy: the intrinsics P of the RECTIFIED image (CameraInfo.P); taken once
    // rectified_fx and rectified_fy are positive, otherwise frames are rectified onto the raw camera's own K.
    std::string distortion_model = "plumb_bob";
    std::array<double, 3> distortion_k456{};
    std::array<float, 4> rectified{};  // fx', cx', fy', cy'
    bool rectifiedSet() const { return rectified[0] > 0.f && rectified[2] > 0.f; }
    // CameraInfo.distortion_model's name -> EKFVIO_CAMERA_*; -1: a model the device does not know
    static int cameraModelOf(const std::string& name) {
        if (name == "plumb_bob") return EKFVIO_CAMERA_PLUMB_BOB;
        if (name == "rational_polynomial") return EKFVIO_CAMERA_RATIONAL;
        if (name == "equidistant" || name == "fisheye") return EKFVIO_CAMERA_EQUIDISTANT;
        return -1;
    }
    // the coefficients of the distortion_* parameters in the order ekfvio_set_camera_model takes them for distortion_model
    std::vector<double> cameraCoefficients() const {
        const int m = cameraModelOf(distortion_model);
        if (m == EKFVIO_CAMERA_EQUIDISTANT) return {distortion[0], distortion[1], distortion[4], distortion_k456[0]};
        std::vector<double> D(distortion.begin(), distortion.end());
        if (m == EKFVIO_CAMERA_RATIONAL) D.insert(D.end(), distortion_k456.begin(), distortion_k456.end());
        return D;
    }
    // Not in the reference, which publishes all-zero covariances (EKFVIO.cpp:473): with publish_covariance = 1 every frame carries the covariances of
    // its odometry and point cloud (ekfvio_set_output_covariance) and the node fills nav_msgs/Odometry's two 6x6 blocks from them.
    int publish_covariance = 0;
    // Not in the reference, which passes no mask to cv::FAST: with mask_rectify_border = 1 the black border that rectification leaves is no-data
    // (ekfvio_set_mask, EKFVIO_MASK_RECTIFY_BORDER): no landmark is detected or passed within the kill-pad window of it.  Nothing to mask while rectify = 0.
    int mask_rectify_border = 0;
    // Not in the reference, whose detector has a fixed contrast threshold and whose tracker assumes brightness constancy: with equalize_clip_limit > 0
    // every frame is equalised on the device between its rectification and the pyramid (ekfvio_set_equalize: clip-limited histograms over
    // equalize_tiles_x x equalize_tiles_y tiles, each in [1, 16]); 0 = off.
    float equalize_clip_limit = 0.f;
    int equalize_tiles_x = 8, equalize_tiles_y = 8;
    // Not in the reference, whose Lucas-Kanade assumes brightness constancy: with klt_photometric = 1 the tracker matches up to a gain and an offset
    // (ekfvio_set_klt_photometric: span{1, I} projected out of the template's gradients, once per pyramid level); 0 = off.
    int klt_photometric = 0;
    // Not in the reference, where a landmark's index is its identity: publish_ids = 1 adds a channel "id" to the node's PointCloud (the landmark's
    // id of ekfvio_get_landmark_ids as a float: exact below 2^24, then id mod 2^24); publish_ended = 1 turns the export of the tracks that ended
    // on (ekfvio_set_ended_export) and the node publishes their records as a second PointCloud on ended_topic.
    int publish_ids = 0, publish_ended = 0;
    // Not in the reference, whose filter learns that the camera stands still only through the landmarks' pixels: with zupt_max_flow_px > 0 a frame in
    // which at least zupt_min_tracks landmarks passed the tracker and at least zupt_min_ratio of them moved no more than that many pixels of the
    // RESIZED frame updates the velocity and the body rate with z = 0 (ekfvio_set_zupt; variances zupt_vel_variance, zupt_omega_variance); 0 = off.
    float zupt_max_flow_px = 0.f;
    int zupt_min_tracks = 8;
    float zupt_min_ratio = 0.75f, zupt_vel_variance = 1e-4f, zupt_omega_variance = 1e-4f;
    // Not in the reference, which has no IMU update: the IMU in its own frame (ekfvio_set_imu_extrinsics).  imu_rotation: nine numbers, row-major,
    // IMU -> camera axes (the rotation of Kalibr's T_cam_imu); imu_position: three numbers, the IMU's origin in the camera frame in metres (its
    // translation).  Either one given turns the setting on (the other then defaults to the identity / zero).  gravity_align_samples = K > 0: the
    // first K IMU records that come up for application are averaged instead of applied and set the gravity vector (ekfvio_gravity_from_accel,
    // ekfvio_set_gravity): the rig is taken to stand still through them, with an accelerometer bias negligible against 9.81.
    std::array<float, 9> imu_rotation{{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}};
    std::array<float, 3> imu_position{{0.f, 0.f, 0.f}};
    int imu_extrinsics = 0, gravity_align_samples = 0;
    // Not in the reference, whose replenishFeatures takes the detector's corners in raster order, first fit: with replenish_grid_x, replenish_grid_y >= 1
    // (at most 256 cells together) new landmarks are the strongest free corner of every cell of that grid over the resized frame, emptier cells first
    // (ekfvio_set_replenish_grid); both 0 = off.  One of them alone is an error when the handle is made.
    int replenish_grid_x = 0, replenish_grid_y = 0;
    // Not in the reference, whose monocular filter has no metric input: the nonholonomic constraint of a wheeled vehicle as a standing aiding
    // measurement (ekfvio_set_frame_aid).  nhc_variance > 0: every frame measures the velocity along the vehicle's y and z axes (x is forward) as
    // zero with that variance, (m/s)^2; 0 = off.  nhc_R_cv: nine numbers, row-major, vehicle -> camera axes (v_cam = R_cv v_vehicle); the default
    // is a forward-looking camera in its optical frame (z forward, x right, y down) on a vehicle with x forward, y left, z up, for which the
    // constraint reads v_x = v_y = 0 in the camera frame.
    float nhc_variance = 0.f;
    std::array<float, 9> nhc_R_cv{{0.f, -1.f, 0.f, 0.f, 0.f, -1.f, 1.f, 0.f, 0.f}};
    std::map<std::string, std::string> node;  // odom_topic, camera_topic, base_frame, use_imu, publish_insight, ...

    Params() {
        ekfvio_default_config(&cfg);
        cfg.inverse_image_scale = 4;  // D_INVERSE_IMAGE_SCALE (Params.h:28); the C-ABI's own default is 1
        node = {{"publish_insight", "true"}, {"insight_topic", "invio/insight"}, {"insight_camera_info_topic", "invio/camera_info"},
                {"analyze_runtime", "true"}, {"odom_topic", "invio/odom"}, {"odom_frame", "invio_odom"},
                {"point_topic", "invio/points"}, {"camera_topic", "/camera/image_rect"}, {"base_frame", "base_link"},
                {"world_frame", "world"}, {"camera_frame", "camera"}, {"imu_topic", "imu/measurement"},
                {"imu_frame", "imu"}, {"use_imu", "true"}, {"ended_topic", "invio/ended_points"}};
    }

    static double number(const std::string& key, const std::string& v) {
        char* end = nullptr;
        const double x = std::strtod(v.c_str(), &end);
        if (end == v.c_str() || *end != '\0' || !std::isfinite(x)) throw Error(EKFVIO_EINVAL, "parameter " + key + ": not a number: " + v);
        return x;
    }
    static int integer(const std::string& key, const std::string& v) {
        const double x = number(key, v);
        if (x != std::floor(x) || std::fabs(x) > 1e9) throw Error(EKFVIO_EINVAL, "parameter " + key + ": not an integer: " + v);
        return (int)x;
    }
    // `count` numbers separated by commas and / or blanks, with or without brackets around them: "[0, -1, 0, ...]" or "0 -1 0 ..."
    static void numbers(const std::string& key, std::string v, float* out, int count) {
        for (char& c : v)
            if (c == '[' || c == ']' || c == ',') c = ' ';
        std::istringstream in(v);
        std::string tok;
        int k = 0;
        while (in >> tok) {
            if (k == count) throw Error(EKFVIO_EINVAL, "parameter " + key + ": more than " + std::to_string(count) + " numbers: " + v);
            out[k++] = (float)number(key, tok);
        }
        if (k != count) throw Error(EKFVIO_EINVAL, "parameter " + key + ": needs " + std::to_string(count) + " numbers: " + v);
    }

    void set(std::string key, const std::string& value) {
        while (!key.empty() && (key[0] == '~' || key[0] == '/')) key.erase(0, 1);
        const size_t slash = key.rfind('/');  // "/ekf_vio/num_features" from a rosparam dump
        if (slash != std::string::npos) key = key.substr(slash + 1);
        if (key == "num_features") cfg.max_features = integer(key, value);
        else if (key == "fast_threshold") cfg.fast_threshold = integer(key, value);
        else if (key == "fast_blur_sigma") cfg.fast_blur_sigma = (float)number(key, value);
        else if (key == "inverse_image_scale") cfg.inverse_image_scale = integer(key, value);  // Frame.cpp:15-42; integral scales only
        else if (key == "kill_pad") cfg.kill_pad = integer(key, value);
        else if (key == "min_klt_eigen_val") cfg.klt_min_eigen = (float)number(key, value);
        else if (key == "min_new_feature_dist") cfg.min_new_feature_dist = (int)number(key, value);  // a double there, used as a radius
        else if (key == "max_pyramids") cfg.klt_max_pyramid_level = integer(key, value);
        else if (key == "klt_window_size") cfg.klt_window_size = integer(key, value);
        else if (key == "default_point_depth") cfg.default_point_depth = (float)number(key, value);
        else if (key == "default_point_depth_variance") cfg.default_point_depth_variance = (float)number(key, value);
        else if (key == "default_point_homogenous_variance") cfg.default_point_homogenous_variance = (float)number(key, value);
        else if (key == "imu_update") cfg.use_imu = (value == "true" || value == "1") ? 1 : 0;  // not a reference parameter: SURVEY 8(f) F4
        else if (key == "remove_lost") cfg.remove_lost = (value == "true" || value == "1") ? 1 : 0;  // not a reference parameter: removes lost landmarks
        else if (key == "gate_chi2") {  // not a reference parameter: the innovation gate's threshold on d2 (0 = off)
            gate_chi2 = (float)number(key, value);
            if (gate_chi2 < 0.f) throw Error(EKFVIO_EINVAL, "parameter gate_chi2: negative: " + value);
        }
        else if (key == "klt_fb_max_px") {  // not a reference parameter: the tracker's forward-backward check, in pixels of the RESIZED frame (0 = off)
            cfg.klt_fb_max_px = (float)number(key, value);
            if (cfg.klt_fb_max_px < 0.f) throw Error(EKFVIO_EINVAL, "parameter klt_fb_max_px: negative: " + value);
        }
        else if (key == "rectify") rectify = (value == "true" || value == "1") ? 1 : 0;
        else if (key == "publish_covariance") publish_covariance = (value == "true" || value == "1") ? 1 : 0;
        else if (key == "mask_rectify_border") mask_rectify_border = (value == "true" || value == "1") ? 1 : 0;
        else if (key == "equalize_clip_limit") {
            equalize_clip_limit = (float)number(key, value);
            if (equalize_clip_limit < 0.f) throw Error(EKFVIO_EINVAL, "parameter equalize_clip_limit: negative: " + value);
        }
        else if (key == "equalize_tiles_x" || key == "equalize_tiles_y") {
            const int t = integer(key, value);
            if (t < 1 || t > 16) throw Error(EKFVIO_EINVAL, "parameter " + key + ": not in [1, 16]: " + value);
            (key == "equalize_tiles_x" ? equalize_tiles_x : equalize_tiles_y) = t;
        }
        else if (key == "klt_photometric") {
            klt_photometric = value == "true" ? 1 : (value == "false" ? 0 : integer(key, value));  // (a launch file's bool arrives as text)
            if (klt_photometric != 0 && klt_photometric != 1) throw Error(EKFVIO_EINVAL, "parameter klt_photometric: not 0 or 1: " + value);
        }
        else if (key == "publish_ids") publish_ids = (value == "true" || value == "1") ? 1 : 0;
        else if (key == "publish_ended") publish_ended = (value == "true" || value == "1") ? 1 : 0;
        else if (key == "zupt_max_flow_px") {
            zupt_max_flow_px = (float)number(key, value);
            // (number() refuses NaN and infinities as text; the narrowing to float can still overflow: what ekfvio_set_zupt would refuse is refused here)
            if (!(zupt_max_flow_px >= 0.f) || !std::isfinite(zupt_max_flow_px)) throw Error(EKFVIO_EINVAL, "parameter zupt_max_flow_px: not a finite value >= 0: " + value);
        }
        else if (key == "zupt_min_tracks") {
            zupt_min_tracks = integer(key, value);
            if (zupt_min_tracks < 1) throw Error(EKFVIO_EINVAL, "parameter zupt_min_tracks: below 1: " + value);
        }
        else if (key == "zupt_min_ratio") {
            zupt_min_ratio = (float)number(key, value);
            if (!(zupt_min_ratio > 0.f && zupt_min_ratio <= 1.f)) throw Error(EKFVIO_EINVAL, "parameter zupt_min_ratio: not in (0, 1]: " + value);
        }
        else if (key == "zupt_vel_variance" || key == "zupt_omega_variance") {
            const float v = (float)number(key, value);
            if (!(v > 0.f) || !std::isfinite(v)) throw Error(EKFVIO_EINVAL, "parameter " + key + ": not a finite value > 0: " + value);
            (key == "zupt_vel_variance" ? zupt_vel_variance : zupt_omega_variance) = v;
        }
        else if (key == "replenish_grid_x" || key == "replenish_grid_y") {
            const int c = integer(key, value);
            if (c < 0 || c > 256) throw Error(EKFVIO_EINVAL, "parameter " + key + ": not in [0, 256]: " + value);
            (key == "replenish_grid_x" ? replenish_grid_x : replenish_grid_y) = c;
        }
        else if (key == "nhc_variance") {
            nhc_variance = (float)number(key, value);
            if (!(nhc_variance >= 0.f) || !std::isfinite(nhc_variance)) throw Error(EKFVIO_EINVAL, "parameter nhc_variance: not a finite value >= 0: " + value);
        }
        else if (key == "nhc_R_cv") {  // (what ekfvio_aid_rows_body_velocity refuses is refused here: a pure host function)
            std::array<float, 9> r{};
            numbers(key, value, r.data(), 9);
            float H[44], z[2], R[4];
            if (!nhcRows(r.data(), 1.f, H, z, R)) throw Error(EKFVIO_EINVAL, "parameter nhc_R_cv: not a rotation: " + value);
            nhc_R_cv = r;
        }
        else if (key == "imu_rotation") {  // (what ekfvio_set_imu_extrinsics would refuse is refused when the handle is made)
            numbers(key, value, imu_rotation.data(), 9);
            imu_extrinsics = 1;
        }
        else if (key == "imu_position") {
            numbers(key, value, imu_position.data(), 3);
            imu_extrinsics = 1;
        }
        else if (key == "gravity_align_samples") {
            gravity_align_samples = integer(key, value);
            if (gravity_align_samples < 0) throw Error(EKFVIO_EINVAL, "parameter gravity_align_samples: negative: " + value);
        }
        else if (key == "distortion_k1") distortion[0] = number(key, value);
        else if (key == "distortion_k2") distortion[1] = number(key, value);
        else if (key == "distortion_p1") distortion[2] = number(key, value);
        else if (key == "distortion_p2") distortion[3] = number(key, value);
        else if (key == "distortion_k3") distortion[4] = number(key, value);
        else if (key == "distortion_k4") distortion_k456[0] = number(key, value);
        else if (key == "distortion_k5") distortion_k456[1] = number(key, value);
        else if (key == "distortion_k6") distortion_k456[2] = number(key, value);
        else if (key == "distortion_model") {
            if (cameraModelOf(value) < 0) throw Error(EKFVIO_EINVAL, "parameter distortion_model: not plumb_bob, rational_polynomial, equidistant or fisheye: " + value);
            distortion_model = value;
        }
        else if (key == "rectified_fx" || key == "rectified_cx" || key == "rectified_fy" || key == "rectified_cy") {
            const float v = (float)number(key, value);
            if (!std::isfinite(v) || ((key == "rectified_fx" || key == "rectified_fy") && v < 0.f))
                throw Error(EKFVIO_EINVAL, "parameter " + key + ": not a finite value (a focal length: >= 0, 0 = unset): " + value);
            rectified[key == "rectified_fx" ? 0 : key == "rectified_cx" ? 1 : key == "rectified_fy" ? 2 : 3] = v;
        }
        else if (key == "imu_gyro_variance") cfg.imu_gyro_variance = (float)number(key, value);
        else if (key == "imu_accel_variance") cfg.imu_accel_variance = (float)number(key, value);
        else if (key == "gravity_x") cfg.gravity[0] = (float)number(key, value);
        else if (key == "gravity_y") cfg.gravity[1] = (float)number(key, value);
        else if (key == "gravity_z") cfg.gravity[2] = (float)number(key, value);
        else if (key == "frame_buffer_size") {
            if (integer(key, value) != 2) throw Error(EKFVIO_EINVAL, "frame_buffer_size: the device keeps exactly two frames (Params.h:58)");
        } else if (node.count(key)) node[key] = value;
        else if (ignored().count(key)) (void)number(key, value);
        else throw Error(EKFVIO_EINVAL, "unknown parameter: " + key);
    }

    // The two rows of the nonholonomic constraint: rows 1 and 2 (the vehicle's y and z axes) of ekfvio_aid_rows_body_velocity at zero velocity
    // and without a lever arm, z = 0, R = variance I.  H: 2 x 22 row-major.  false: R_cv or the variance is refused.
    static bool nhcRows(const float* R_cv, float variance, float* H, float* z, float* R) {
        const float v[3] = {0.f, 0.f, 0.f}, cov[9] = {variance, 0.f, 0.f, 0.f, variance, 0.f, 0.f, 0.f, variance};
        float H3[66], z3[3], R3[9];
        if (ekfvio_aid_rows_body_velocity(R_cv, nullptr, v, cov, H3, z3, R3) != EKFVIO_OK) return false;
        for (int e = 0; e < 44; e++) H[e] = H3[22 + e];
        z[0] = z[1] = 0.f;
        R[0] = R[3] = variance, R[1] = R[2] = 0.f;
        return true;
    }

    // every private parameter name the node accepts (EKFVIO.cpp:20-67): what a ROS front end asks the parameter server for
    static std::vector<std::string> names() {
        std::vector<std::string> out = {"num_features", "fast_threshold", "fast_blur_sigma", "inverse_image_scale", "kill_pad",
                                        "min_klt_eigen_val", "min_new_feature_dist", "max_pyramids", "klt_window_size",
                                        "default_point_depth", "default_point_depth_variance",
                                        "default_point_homogenous_variance", "frame_buffer_size", "imu_update",
                                        "imu_gyro_variance", "imu_accel_variance", "gravity_x", "gravity_y", "gravity_z", "remove_lost", "gate_chi2",
                                        "klt_fb_max_px", "rectify", "publish_covariance", "mask_rectify_border", "equalize_clip_limit", "equalize_tiles_x", "equalize_tiles_y", "klt_photometric", "publish_ids", "publish_ended", "zupt_max_flow_px", "zupt_min_tracks", "zupt_min_ratio", "zupt_vel_variance", "zupt_omega_variance", "imu_rotation", "imu_position", "gravity_align_samples", "replenish_grid_x", "replenish_grid_y", "nhc_variance", "nhc_R_cv", "distortion_k1", "distortion_k2", "distortion_p1", "distortion_p2", "distortion_k3",
                                        "distortion_model", "distortion_k4", "distortion_k5", "distortion_k6", "rectified_fx", "rectified_fy", "rectified_cx", "rectified_cy"};
        for (const auto& e : Params().node) out.push_back(e.first);
        for (const auto& e : ignored()) out.push_back(e.first);
        return out;
    }

    static Params fromMap(const std::map<std::string, std::string>& kv) {
        Params p;
        for (const auto& e : kv) p.set(e.first, e.second);
        return p;
    }
    // "key: value" lines (the flat YAML a launch file's <rosparam> block or `rosparam dump` of the node produces);
    // '#' starts a comment, quotes around values are dropped.
    static Params fromFile(const std::string& path) {
        std::ifstream in(path);
        if (!in) throw Error(EKFVIO_EINVAL, "cannot open " + path);
        Params p;
        std::string line;
        while (std::getline(in, line)) {
            const size_t hash = line.find('#');
            if (hash != std::string::npos) line.erase(hash);
            const size_t colon = line.find(':');
            if (colon == std::string::npos) {
                if (line.find_first_not_of(" \t\r") != std::string::npos) throw Error(EKFVIO_EINVAL, "not a 'key: value' line: " + line);
                continue;
            }
            auto trim = [](std::string t) {
                const size_t a = t.find_first_not_of(" \t\r\"'"), b = t.find_last_not_of(" \t\r\"'");
                return a == std::string::npos ? std::string() : t.substr(a, b - a + 1);
            };
            p.set(trim(line.substr(0, colon)), trim(line.substr(colon + 1)));
        }
        return p;
    }

   private:
    static const std::map<std::string, int>& ignored() {
        static const std::map<std::string, int> names = {
            {"border_weight_exponent", 0}, {"start_feature_count", 0}, {"dangerous_mature_feature_count", 0},
            {"minimum_trackable_features", 0}, {"minimum_keyframe_count_for_optimization", 0},
            {"maximum_keyframe_count_for_optimization", 0}, {"depth_translation_ratio", 0}, {"max_depth_updates_per_frame", 0},
            {"maximum_reprojection_error", 0}, {"moba_candidate_variance", 0}, {"maximum_candidate_reprojection_error", 0},
            {"eps_moba", 0}, {"eps_sba", 0}, {"huber_width", 0}, {"minumum_depth_determinant", 0}, {"moba_max_iterations", 0},
            {"sba_max_iterations", 0}, {"max_point_z", 0}, {"min_point_z", 0}, {"min_variance_box_size", 0},
            {"max_variance_box_size", 0}};
        return names;
    }
};

// Frame.h:25-41 without OpenCV: 8-bit single-channel image + intrinsics + stamp.
struct Frame {
    const uint8_t* img = nullptr;
    int cols = 0, rows = 0, step = 0;
    std::array<float, 9> K{};  // row-major, as sensor_msgs/CameraInfo.K
    double t = 0;
};

class TightlyCoupledEKF {
   public:
    explicit TightlyCoupledEKF(int max_features = 100, int device = 0, const ekfvio_config* cfg = nullptr) {
        ekfvio_config c;
        if (cfg) c = *cfg;
        else ekfvio_default_config(&c);
        if (!cfg) c.max_features = max_features;
        max_features_ = c.max_features;
        int rc = ekfvio_create(&c, device, nullptr, &h_);
        if (rc != EKFVIO_OK) {
            std::string msg = h_ ? ekfvio_last_error(h_) : "ekfvio_create failed";
            if (h_) ekfvio_destroy(h_);
            h_ = nullptr;
            throw Error(rc, msg);
        }
    }
    ~TightlyCoupledEKF() {
        if (h_) ekfvio_destroy(h_);
    }
    TightlyCoupledEKF(const TightlyCoupledEKF&) = delete;
    TightlyCoupledEKF& operator=(const TightlyCoupledEKF&) = delete;

    void initializeBaseState() { chk(ekfvio_reset(h_)); }
    void addNewFeatures(const std::vector<Vector2f>& new_homogenous_features) {
        chk(ekfvio_add_features(h_, new_homogenous_features.empty() ? nullptr : new_homogenous_features[0].data(),
                                (int)new_homogenous_features.size()));
    }
    void process(float dt) { chk(ekfvio_process(h_, dt)); }
    // returns false when the factorisation met a non-positive pivot (reference: ROS_ERROR_COND, continues)
    bool updateWithFeaturePositions(const std::vector<Vector2f>& measured_positions,
                                    const std::vector<Matrix2f>& estimated_covariance, const std::vector<uint8_t>& pass) {
        if (measured_positions.size() != estimated_covariance.size() || pass.size() != estimated_covariance.size())
            throw Error(EKFVIO_EINVAL, "size mismatch (TightlyCoupledEKF.cpp:478)");
        int rc = ekfvio_update(h_, measured_positions.empty() ? nullptr : measured_positions[0].data(),
                               estimated_covariance.empty() ? nullptr : estimated_covariance[0].data(), pass.data(),
                               (int)pass.size());
        if (rc == EKFVIO_ENUMERIC) return false;
        chk(rc);
        return true;
    }
    // Not in the reference: the innovation gate (ekfvio_set_gate).  chi2 > 0: a landmark whose squared Mahalanobis distance on the propagated
    // state exceeds it is treated as one the tracker failed; 0: off.
    void setGate(float chi2) { chk(ekfvio_set_gate(h_, chi2)); }
    struct Gate {
        std::vector<float> d2;       // per landmark of the most recent update (-1: not evaluated)
        std::vector<uint8_t> gated;
        int32_t gated_last = 0;
        int64_t gated_total = 0;
    };
    Gate gate() {
        Gate g;
        g.d2.assign((size_t)(max_features_ > 0 ? max_features_ : 1), -1.f);
        g.gated.assign(g.d2.size(), 0);
        int32_t n = 0;
        chk(ekfvio_get_gate(h_, g.d2.data(), g.gated.data(), &n, &g.gated_last, &g.gated_total));
        g.d2.resize((size_t)n), g.gated.resize((size_t)n);
        return g;
    }
    // Not in the reference: the tracker's forward-backward check (ekfvio_set_klt_fb).  max_px > 0: a landmark whose forward track, tracked back
    // into the previous frame, ends more than max_px pixels from where it started is treated as one the tracker lost; 0: off.
    void setKltFb(float max_px) { chk(ekfvio_set_klt_fb(h_, max_px)); }
    struct KltFb {
        std::vector<float> err2;     // per landmark of the most recent checked track (-1: forward track failed, -2: backward track failed)
        std::vector<uint8_t> rejected;
        int32_t rejected_last = 0;
        int64_t rejected_total = 0;
    };
    KltFb kltFb() {
        KltFb r;
        r.err2.assign((size_t)(max_features_ > 0 ? max_features_ : 1), -1.f);
        r.rejected.assign(r.err2.size(), 0);
        int32_t n = 0;
        chk(ekfvio_get_klt_fb(h_, r.err2.data(), r.rejected.data(), &n, &r.rejected_last, &r.rejected_total));
        r.err2.resize((size_t)n), r.rejected.resize((size_t)n);
        return r;
    }
    // Not in the reference, which assumes a pinhole image (Frame.h:31): the camera's plumb_bob coefficients k1 k2 p1 p2 [k3] (ekfvio_set_distortion).
    // From the next frame on, frames are rectified on the device between the upload and the pyramid; empty or all zero: off.
    void setDistortion(const std::vector<double>& D) { chk(ekfvio_set_distortion(h_, D.empty() ? nullptr : D.data(), (int32_t)D.size())); }
    // Not in the reference: the camera's lens model (EKFVIO_CAMERA_PLUMB_BOB with 0, 4 or 5 coefficients, EKFVIO_CAMERA_RATIONAL with 8,
    // EKFVIO_CAMERA_EQUIDISTANT with 4) and, optionally, the rectified camera P = fx', cx', fy', cy' (nullptr: the raw camera's own K)
    // (ekfvio_set_camera_model).  With P, everything behind the rectification takes P for the frame's intrinsics.  The last of the two setters wins.
    void setCameraModel(int model, const std::vector<double>& D, const float* P = nullptr) {
        chk(ekfvio_set_camera_model(h_, model, D.empty() ? nullptr : D.data(), (int32_t)D.size(), P));
    }
    // the rectified camera where one is set (ekfvio_get_camera_model): what level 0 of a pushed frame is then the image of
    bool rectifiedCamera(float P[4]) {
        int32_t has = 0;
        chk(ekfvio_get_camera_model(h_, nullptr, nullptr, nullptr, P, &has, nullptr));
        return has != 0;
    }
    // Not in the reference, which passes no mask to cv::FAST: the no-data mask (ekfvio_set_mask).  mask: w x h bytes at the FULL frame size with a row
    // stride, nonzero = scene, or nullptr (w = h = stride = 0); flags: EKFVIO_MASK_RECTIFY_BORDER or 0.  From the next frame on no landmark is
    // detected or passed within the kill-pad window of a no-data pixel; nullptr and 0: off.  While a mask is set, frames of another size are refused.
    void setMask(const uint8_t* mask, int w, int h, int stride, int flags) { chk(ekfvio_set_mask(h_, mask, w, h, stride, flags)); }
    // Not in the reference: clip-limited tile histogram equalisation of every pushed frame on the device, between the rectification and the pyramid
    // (ekfvio_set_equalize).  clip_limit > 0 with tiles in [1, 16]: on from the next frame; clip_limit == 0: off.
    void setEqualize(float clip_limit, int tiles_x = 8, int tiles_y = 8) { chk(ekfvio_set_equalize(h_, clip_limit, tiles_x, tiles_y)); }
    // Not in the reference, whose tracker assumes brightness constancy: the gain/offset term of every Lucas-Kanade pass
    // (ekfvio_set_klt_photometric).  On from the next track; off by default.
    void setKltPhotometric(bool on) { chk(ekfvio_set_klt_photometric(h_, on ? 1 : 0)); }
    // New landmarks spread over the image (ekfvio_set_replenish_grid): from the next replenishment on the strongest free corner of every cell of a
    // cells_x x cells_y grid, emptier cells first, instead of the raster first fit.  (0, 0): off, the default; (1, 1): strongest corner first.
    void setReplenishGrid(int cells_x, int cells_y) { chk(ekfvio_set_replenish_grid(h_, cells_x, cells_y)); }
    // Not in the reference: the zero-velocity update (ekfvio_set_zupt).  max_flow_px > 0: a frame in which at least min_tracks landmarks passed the
    // tracker and at least min_ratio of those moved no more than max_flow_px pixels updates the velocity and the body rate with z = 0 in front of
    // the camera update; 0: off.  zuptUpdate: that update alone, unconditional, for a caller with a stop detector of its own.
    void setZupt(float max_flow_px, int min_tracks = 8, float min_ratio = 0.75f, float vel_variance = 1e-4f, float omega_variance = 1e-4f) {
        chk(ekfvio_set_zupt(h_, max_flow_px, min_tracks, min_ratio, vel_variance, omega_variance));
    }
    void zuptUpdate(float vel_variance = 1e-4f, float omega_variance = 1e-4f) { chk(ekfvio_zupt_update(h_, vel_variance, omega_variance)); }
    // Not in the reference: a linear aiding measurement of the base state, z = H x[0:22] + v, v ~ N(0, R) (ekfvio_aid_update): k = 1..6 rows, H k x 22
    // row-major, R k x k row-major (lower triangle read), Joseph form on the device; chi2 > 0 gates it on the normalised innovation squared.
    // aidUpdate: on the state as it stands; aid: behind process(dt) to `stamp`, whatever use_imu says (the first stamp only sets the time);
    // setFrameAid: a standing measurement applied in every frame behind the tracker, in front of the zero-velocity and the camera update
    // (k = 0: off).  All asynchronous.  aidStatus: the most recent one's d2, verdict and counts.
    void aidUpdate(int k, const float* H, const float* z, const float* R, float chi2 = 0.f) { chk(ekfvio_aid_update(h_, k, H, z, R, chi2)); }
    void aid(double stamp, int k, const float* H, const float* z, const float* R, float chi2 = 0.f) { chk(ekfvio_aid(h_, stamp, k, H, z, R, chi2)); }
    void setFrameAid(int k, const float* H = nullptr, const float* z = nullptr, const float* R = nullptr, float chi2 = 0.f) {
        chk(ekfvio_set_frame_aid(h_, k, H, z, R, chi2));
    }
    struct AidStatus {
        float d2_last = 0.f;
        int32_t accepted_last = 0;
        int64_t applied_total = 0, rejected_total = 0;
    };
    AidStatus aidStatus() {
        AidStatus r;
        chk(ekfvio_get_aid(h_, &r.d2_last, &r.accepted_last, &r.applied_total, &r.rejected_total));
        return r;
    }
    // Not in the reference: the IMU in its own frame (ekfvio_set_imu_extrinsics).  R_ci: nine floats, row-major, IMU -> camera axes (the rotation of
    // Kalibr's T_cam_imu); p_ci: the IMU's origin in the camera frame, metres (its translation); both nullptr: off.  From the next IMU update on.
    void setImuExtrinsics(const float* R_ci, const float* p_ci) { chk(ekfvio_set_imu_extrinsics(h_, R_ci, p_ci)); }
    bool getImuExtrinsics(std::array<float, 9>& R_ci, std::array<float, 3>& p_ci) {
        int32_t on = 0;
        chk(ekfvio_get_imu_extrinsics(h_, R_ci.data(), p_ci.data(), &on));
        return on != 0;
    }
    // ekfvio_set_gravity: the gravity vector in the filter's world frame replaces the configuration's from the next IMU update on.
    void setGravity(const Vector3f& g) { chk(ekfvio_set_gravity(h_, g.data())); }
    Vector3f getGravity() {
        Vector3f g{};
        chk(ekfvio_get_gravity(h_, g.data()));
        return g;
    }
    struct Zupt {
        std::vector<float> flow2;  // per landmark of the most recent frame's decision: squared pixel flow (-1: the tracker did not pass it)
        int32_t n_pass = 0, n_still = 0, applied_last = 0;
        int64_t applied_total = 0;
    };
    Zupt getZupt() {
        Zupt r;
        r.flow2.assign((size_t)(max_features_ > 0 ? max_features_ : 1), -1.f);
        int32_t n = 0;
        chk(ekfvio_get_zupt(h_, r.flow2.data(), &n, &r.n_pass, &r.n_still, &r.applied_last, &r.applied_total));
        r.flow2.resize((size_t)n);
        return r;
    }
    struct Mask {
        int width = 0, height = 0;     // level 0; 0 x 0 before the first frame pushed with the mask on
        std::vector<uint8_t> blocked;  // height x width, 1 = blocked
    };
    Mask getMask() {
        Mask m;
        int32_t w = 0, h = 0;
        chk(ekfvio_get_mask(h_, nullptr, 0, &w, &h));
        m.blocked.assign((size_t)w * (size_t)h, 0);
        if (!m.blocked.empty()) chk(ekfvio_get_mask(h_, m.blocked.data(), (int32_t)m.blocked.size(), &w, &h));
        m.width = w, m.height = h;
        return m;
    }
    struct MaskHits {
        std::vector<uint8_t> masked;  // per landmark of the most recent track: let through by everything else, and on a blocked pixel
        int32_t masked_last = 0;
    };
    MaskHits getMaskHits() {
        MaskHits r;
        r.masked.assign((size_t)(max_features_ > 0 ? max_features_ : 1), 0);
        int32_t n = 0;
        chk(ekfvio_get_mask_hits(h_, r.masked.data(), &n, &r.masked_last));
        r.masked.resize((size_t)n);
        return r;
    }
    // Not in the reference (EKFVIO.cpp:473 "TODO add convariance computation"): the covariances of the published outputs (include/ekfvio.h).
    // setOutputCovariance(true): every frame of addFrame carries them with its other outputs, and the two getters cost a memcpy behind a frame
    // (such a frame's outputs never go out in front of the update's last GEMM); otherwise each getter is one launch and one wait.
    void setOutputCovariance(bool on) { chk(ekfvio_set_output_covariance(h_, on ? 1 : 0)); }
    struct OdometryCovariance {
        std::array<float, 36> pose{};   // row-major 6x6 over (x, y, z, rotation about X, Y, Z), world frame: nav_msgs/Odometry.pose.covariance
        std::array<float, 36> twist{};  // row-major 6x6 over (linear, angular), body frame: twist.covariance
    };
    OdometryCovariance getOdometryCovariance() {
        OdometryCovariance c;
        chk(ekfvio_get_odometry_covariance(h_, c.pose.data(), c.twist.data()));
        return c;
    }
    // one row-major 3x3 per landmark: the covariance of the camera-frame point (u/rho, v/rho, 1/rho) of the point cloud
    std::vector<std::array<float, 9>> getPointsCovariance() {
        std::vector<std::array<float, 9>> out(numFeatures());
        chk(ekfvio_get_points_covariance(h_, out.empty() ? nullptr : out[0].data()));
        return out;
    }
    // Not in the reference, where a landmark's index is its identity (it never removes one): the landmarks' ids and birth stamps, rows as the point
    // cloud's of the same moment (ekfvio_get_landmark_ids).  An id is never reused during the handle's lifetime and ids rise strictly in landmark
    // order; born is the stamp of the frame a landmark entered in (NaN before any stamp).  A memcpy behind a frame.
    struct LandmarkIds {
        std::vector<int64_t> id;
        std::vector<double> born;
    };
    LandmarkIds getLandmarkIds() {
        LandmarkIds r;
        r.id.resize((size_t)numFeatures()), r.born.resize(r.id.size());
        chk(ekfvio_get_landmark_ids(h_, r.id.empty() ? nullptr : r.id.data(), r.born.empty() ? nullptr : r.born.data()));
        return r;
    }
    // Not in the reference: with the export on, every removal (removeFeatures, addFrame with cfg.remove_lost = 1) first writes one record per landmark
    // about to leave (ekfvio_set_ended_export); getEnded reads the records of the most recent removal, so a consumer that wants every ended track
    // reads them after every frame.  xyz and cov carry the bits getPoints / getPointsCovariance would have returned in front of the removal.
    void setEndedExport(bool on) { chk(ekfvio_set_ended_export(h_, on ? 1 : 0)); }
    struct Ended {
        std::vector<int64_t> id;
        std::vector<double> born;
        std::vector<int32_t> index_before;        // the landmark's row in front of the removal (the rows of gate(), kltFb(), getMaskHits() of the frame)
        std::vector<Vector3f> xyz;                // camera frame
        std::vector<std::array<float, 9>> cov;    // row-major 3x3
        int64_t total = 0;                        // records since create / reset
    };
    Ended getEnded() {
        Ended r;
        int32_t k = 0;
        chk(ekfvio_get_ended(h_, nullptr, nullptr, nullptr, nullptr, nullptr, max_features_ > 0 ? max_features_ : 1, &k, &r.total));
        r.id.resize((size_t)k), r.born.resize((size_t)k), r.index_before.resize((size_t)k), r.xyz.resize((size_t)k), r.cov.resize((size_t)k);
        if (k > 0) chk(ekfvio_get_ended(h_, r.id.data(), r.born.data(), r.index_before.data(), r.xyz[0].data(), r.cov[0].data(), k, &k, &r.total));
        return r;
    }
    // Not in the reference (it flags lost landmarks, TightlyCoupledEKF.cpp:528, and keeps them): removes the landmarks whose byte
    // of `remove` is nonzero (one per landmark), or, with no mask, those flagged for deletion.  Returns the number removed.
    int removeFeatures(const std::vector<uint8_t>* remove = nullptr) {
        int32_t removed = 0;
        chk(ekfvio_remove_features(h_, remove ? remove->data() : nullptr, remove ? (int32_t)remove->size() : 0, &removed));
        return removed;
    }
    std::vector<int> formFeatureMeasurementMap(const std::vector<uint8_t>& measured) const {
        std::vector<int> idx(2 * measured.size() + 1);
        int rows = 0;
        chk(ekfvio_measurement_map(h_, measured.data(), (int)measured.size(), idx.data(), &rows));
        idx.resize(rows);
        return idx;
    }
    std::vector<Vector2f> previousFeaturePositionVector() {
        std::vector<Vector2f> out(numFeatures());
        chk(ekfvio_get_features(h_, nullptr, out.empty() ? nullptr : out[0].data(), nullptr));
        return out;
    }
    Matrix2f getFeatureHomogenousCovariance(int index) {
        Matrix2f m;
        chk(ekfvio_get_feature_cov(h_, index, m.data()));
        return m;
    }
    // TightlyCoupledEKF.cpp:668-676
    void setFeatureHomogenousCovariance(int index, const Matrix2f& cov) { chk(ekfvio_set_feature_cov(h_, index, cov.data())); }
    // TightlyCoupledEKF.cpp:683-697 (K row-major 3x3 as in CameraInfo.K; the reference returns a 2x2 sparse matrix)
    static Matrix2f getMetric2PixelMap(const std::array<float, 9>& K) {
        Matrix2f J;
        ekfvio_metric2pixel_map(K.data(), J.data());
        return J;
    }
    static Matrix2f getPixel2MetricMap(const std::array<float, 9>& K) {
        Matrix2f J;
        ekfvio_pixel2metric_map(K.data(), J.data());
        return J;
    }
    float getFeatureDepthVariance(int index) {
        float v = 0;
        chk(ekfvio_get_depth_variance(h_, index, &v));
        return v;
    }
    // checkSigma (TightlyCoupledEKF.cpp:699-714): true iff diag >= 0 and |S_ij - S_ji| <= 1e-3
    bool checkSigma(float* min_diag = nullptr, float* max_asym = nullptr) {
        float a = 0, b = 0;
        chk(ekfvio_check_sigma(h_, &a, &b));
        if (min_diag) *min_diag = a;
        if (max_asym) *max_asym = b;
        return a >= 0 && b <= 1e-3f;
    }
    std::array<float, EKFVIO_BASE_STATE_SIZE> base_mu() {
        std::array<float, EKFVIO_BASE_STATE_SIZE> b;
        chk(ekfvio_get_base_mu(h_, b.data()));
        return b;
    }
    std::vector<Vector3f> featureMus() {
        std::vector<Vector3f> out(numFeatures());
        chk(ekfvio_get_features(h_, out.empty() ? nullptr : out[0].data(), nullptr, nullptr));
        return out;
    }
    // Feature::getDeleteFlag per landmark (set when the tracker lost it, TightlyCoupledEKF.cpp:528; read by publishInsight)
    std::vector<uint8_t> deleteFlags() {
        std::vector<uint8_t> out(numFeatures());
        chk(ekfvio_get_features(h_, nullptr, nullptr, out.empty() ? nullptr : out.data()));
        return out;
    }
    int numFeatures() const { return ekfvio_num_features(h_); }
    int maxFeatures() const { return max_features_; }
    int dim() const { return ekfvio_dim(h_); }
    ekfvio_filter* handle() { return h_; }

    void chk(int rc) const {
        if (rc != EKFVIO_OK) throw Error(rc, ekfvio_last_error(h_));
    }

   private:
    ekfvio_filter* h_ = nullptr;
    int max_features_ = 0;
};

class KLTTracker {
   public:
    explicit KLTTracker(TightlyCoupledEKF& ekf) : ekf_(ekf) {}
    // Uploads `cf`; the previously pushed frame becomes `lf` (the reference passes both by reference).
    void pushFrame(const Frame& cf) {
        ekf_.chk(ekfvio_klt_push_frame(ekf_.handle(), cf.img, cf.cols, cf.rows, cf.step, cf.K.data()));
    }
    void findNewFeaturePositions(std::vector<Vector2f>& measured_positions, std::vector<Matrix2f>& estimated_uncertainty,
                                 std::vector<uint8_t>& passed) {
        const int N = ekf_.numFeatures();
        measured_positions.resize(N);
        estimated_uncertainty.resize(N);
        passed.resize(N);
        ekf_.chk(ekfvio_klt_track(ekf_.handle(), N ? measured_positions[0].data() : nullptr,
                                  N ? estimated_uncertainty[0].data() : nullptr, passed.data()));
    }

    // KLTTracker::estimateUncertaintySampleBased (KLTTracker.cpp:111-175) for n points between the two frames pushed
    // last: pixel-space covariances (px^2).  mu_ref in the previous frame, mu in the current one.
    void estimateUncertaintySampleBased(const std::vector<Vector2f>& mu_ref, const std::vector<Vector2f>& mu,
                                        std::vector<Matrix2f>& cov) {
        if (mu_ref.size() != mu.size()) throw Error(EKFVIO_EINVAL, "estimateUncertaintySampleBased: size mismatch");
        cov.resize(mu.size());
        if (mu.empty()) return;
        ekf_.chk(ekfvio_klt_uncertainty_points(ekf_.handle(), mu_ref[0].data(), mu[0].data(), (int32_t)mu.size(), cov[0].data()));
    }

   private:
    TightlyCoupledEKF& ekf_;
};

// publishOdometry's payload (EKFVIO.cpp:444-477) and publishPoints' (EKFVIO.cpp:479-518) as plain records: what the
// node copies into nav_msgs/Odometry (+ the world -> odom tf) and sensor_msgs/PointCloud with its "intensity" channel.
struct Odometry {
    double stamp = 0;
    Vector3f position{};
    std::array<float, 4> orientation_wxyz{};
    Vector3f linear{}, angular{};
};
struct PointCloud {
    double stamp = 0;
    std::vector<Vector3f> points;   // camera frame: (u/rho, v/rho, 1/rho)
    std::vector<float> intensity;   // image byte at the landmark's pixel
};

// publishInsight's payload (EKFVIO.cpp:379-442): the RESIZED frame as BGR8 with a green 22-pixel square marker
// (cv::drawMarker(..., MARKER_SQUARE, 22, 1)) at the pixel of every landmark that is not flagged for deletion, and the
// CameraInfo numbers the reference fills in (its K/P entries come from linear indexing of a column-major Matrix3f:
// K is published transposed, P(0,2) and P(1,2) are the zero entries K(2,0), K(2,1); reproduced as they are).
struct Insight {
    double stamp = 0;
    int width = 0, height = 0;
    std::vector<uint8_t> bgr;  // height x width x 3
    std::array<double, 9> K{};
    std::array<double, 12> P{};
};

// The step sequence of EKFVIO::addFrame (EKFVIO.cpp:139-196) with the ROS plumbing removed.
class EKFVIO {
   public:
    explicit EKFVIO(int max_features = 100, int device = 0, const ekfvio_config* cfg = nullptr)
        : tc_ekf(max_features, device, cfg), tracker(tc_ekf), use_imu_(cfg ? cfg->use_imu != 0 : false),
          scale_(cfg && cfg->inverse_image_scale > 1 ? cfg->inverse_image_scale : 1) {
        if (cfg) gravity_magnitude_ = std::sqrt((double)cfg->gravity[0] * cfg->gravity[0] + (double)cfg->gravity[1] * cfg->gravity[1] +
                                                (double)cfg->gravity[2] * cfg->gravity[2]);
    }
    // the node's constructor (EKFVIO.cpp:19-67): parameters by the reference's names (see Params)
    explicit EKFVIO(const Params& p, int device = 0)
        : tc_ekf(p.cfg.max_features, device, &p.cfg), tracker(tc_ekf), params(p.node), use_imu_(p.cfg.use_imu != 0),
          scale_(p.cfg.inverse_image_scale > 1 ? p.cfg.inverse_image_scale : 1) {
        if (p.gate_chi2 > 0.f) tc_ekf.setGate(p.gate_chi2);  // (behind ekfvio_create: the gate is a property of the handle)
        // (likewise; a node replaces them with CameraInfo.D.  The plumb_bob model without a rectified camera stays ekfvio_set_distortion's call)
        if (p.rectify && Params::cameraModelOf(p.distortion_model) == EKFVIO_CAMERA_PLUMB_BOB && !p.rectifiedSet())
            tc_ekf.setDistortion(std::vector<double>(p.distortion.begin(), p.distortion.end()));
        else if (p.rectify)
            tc_ekf.setCameraModel(Params::cameraModelOf(p.distortion_model), p.cameraCoefficients(), p.rectifiedSet() ? p.rectified.data() : nullptr);
        if (p.publish_covariance) tc_ekf.setOutputCovariance(true);  // (likewise)
        if (p.mask_rectify_border) tc_ekf.setMask(nullptr, 0, 0, 0, EKFVIO_MASK_RECTIFY_BORDER);  // (likewise; live once the coefficients are nonzero)
        if (p.equalize_clip_limit > 0.f) tc_ekf.setEqualize(p.equalize_clip_limit, p.equalize_tiles_x, p.equalize_tiles_y);  // (likewise)
        if (p.klt_photometric) tc_ekf.setKltPhotometric(true);  // (likewise)
        if (p.replenish_grid_x || p.replenish_grid_y) tc_ekf.setReplenishGrid(p.replenish_grid_x, p.replenish_grid_y);  // (likewise; one of the two alone is refused here)
        if (p.publish_ended) tc_ekf.setEndedExport(true);  // (likewise)
        if (p.zupt_max_flow_px > 0.f) tc_ekf.setZupt(p.zupt_max_flow_px, p.zupt_min_tracks, p.zupt_min_ratio, p.zupt_vel_variance, p.zupt_omega_variance);  // (likewise)
        if (p.imu_extrinsics) tc_ekf.setImuExtrinsics(p.imu_rotation.data(), p.imu_position.data());  // (likewise)
        if (p.nhc_variance > 0.f) {  // (likewise: the nonholonomic constraint as the handle's standing aiding measurement)
            float H[44], z[2], R[4];
            if (!Params::nhcRows(p.nhc_R_cv.data(), p.nhc_variance, H, z, R)) throw Error(EKFVIO_EINVAL, "nhc_variance / nhc_R_cv refused");
            tc_ekf.setFrameAid(2, H, z, R);
        }
        gravity_magnitude_ = std::sqrt((double)p.cfg.gravity[0] * p.cfg.gravity[0] + (double)p.cfg.gravity[1] * p.cfg.gravity[1] +
                                       (double)p.cfg.gravity[2] * p.cfg.gravity[2]);
        setGravityAlignSamples(p.gravity_align_samples);
    }
    // K > 0: the next K IMU records that come up for application (drainImu) are not applied: their accelerometer readings are averaged in
    // double precision, and behind the K-th the gravity vector is set from the mean (ekfvio_gravity_from_accel with the handle's R_ci and the
    // configured gravity's magnitude; ekfvio_set_gravity).  The assumption: the rig stands still through them and the accelerometer's bias is
    // negligible against 9.81.  Frames meanwhile are processed as without an IMU.  0: off.  Starts the averaging over.
    void setGravityAlignSamples(int k) {
        align_samples_ = align_left_ = k > 0 ? k : 0;
        align_sum_[0] = align_sum_[1] = align_sum_[2] = 0.0;
    }
    // initializeBaseState, an empty IMU queue, and the gravity alignment starts over (the extrinsics and the gravity set so far stay)
    void reset() {
        tc_ekf.initializeBaseState();
        imu_queue_.clear();
        have_time_ = false;  // (ekfvio_reset forgets the filter's clock)
        setGravityAlignSamples(align_samples_);
    }
    TightlyCoupledEKF tc_ekf;
    KLTTracker tracker;
    std::map<std::string, std::string> params;  // node-level parameters (topics, frames, switches) for the ROS side

    // EKFVIO::replenishFeatures (EKFVIO.cpp:224-311) on the frame pushed last: FAST-9/16 + occupancy first fit +
    // addNewFeatures, all on the device.  Returns the number of landmarks added.  With cfg.replenish = 1
    // addFrame() does this itself at the two places the reference does (:154, :172).
    int replenishFeatures(std::vector<int32_t>* new_pixels_xy = nullptr) {
        int32_t added = 0;
        if (new_pixels_xy) new_pixels_xy->assign(2 * (size_t)tc_ekf.maxFeatures(), 0);
        tc_ekf.chk(ekfvio_replenish(tc_ekf.handle(), &added, new_pixels_xy ? new_pixels_xy->data() : nullptr));
        if (new_pixels_xy) new_pixels_xy->resize(2 * (size_t)added);
        return added;
    }

    // returns false on a numeric warning (see updateWithFeaturePositions)
    bool addFrame(const Frame& f) {
        drainImu(f.t);  // IMU records up to this frame's stamp, in stamp order, before the frame itself
        int rc = ekfvio_step_image(tc_ekf.handle(), f.t, f.img, f.cols, f.rows, f.step, f.K.data());
        // ekfvio_step_image moves the device clock as soon as process(dt) is enqueued; only EINVAL / ECAPACITY refuse the frame
        // before that.  The queue clock follows whenever the predict went out, whatever happened behind it.
        if (rc != EKFVIO_EINVAL && rc != EKFVIO_ECAPACITY) {
            last_stamp_ = f.t;
            if (!have_time_ || f.t > t_filter_) t_filter_ = f.t;
            have_time_ = true;
            for (int i = 0; i < 9; i++) last_K_[i] = f.K[i];
        }
        if (rc == EKFVIO_ENUMERIC) return false;
        tc_ekf.chk(rc);
        return true;
    }
    // what publishOdometry(cf) / publishPoints(cf) send after addFrame (EKFVIO.cpp:182-188)
    Odometry odometry() {
        Odometry o;
        o.stamp = last_stamp_;
        tc_ekf.chk(ekfvio_get_odometry(tc_ekf.handle(), o.position.data(), o.orientation_wxyz.data(), o.linear.data(), o.angular.data()));
        return o;
    }
    PointCloud points() {
        PointCloud c;
        c.stamp = last_stamp_;
        const int N = tc_ekf.numFeatures();
        c.points.resize(N);
        c.intensity.resize(N);
        tc_ekf.chk(ekfvio_get_points(tc_ekf.handle(), N ? c.points[0].data() : nullptr, N ? c.intensity.data() : nullptr));
        return c;
    }
    // what publishInsight(cf) sends (EKFVIO.cpp:379-442); needs a frame
    Insight insight() {
        if (!have_time_) throw Error(EKFVIO_ESTATE, "insight() before the first frame");
        Insight o;
        o.stamp = last_stamp_;
        int32_t w = 0, h = 0;
        tc_ekf.chk(ekfvio_klt_get_level(tc_ekf.handle(), 0, &w, &h, nullptr, nullptr));
        std::vector<uint8_t> grey((size_t)w * h);
        tc_ekf.chk(ekfvio_klt_get_level(tc_ekf.handle(), 0, &w, &h, grey.data(), nullptr));
        o.width = w;
        o.height = h;
        o.bgr.resize((size_t)w * h * 3);
        for (size_t i = 0; i < grey.size(); i++) o.bgr[3 * i] = o.bgr[3 * i + 1] = o.bgr[3 * i + 2] = grey[i];  // CV_GRAY2BGR
        // Frame::Frame's K (Frame.cpp:26-33), then Feature::getPixel with the K(2) / K(5) indexing quirk (Feature.h:60-66)
        // (with a rectified camera set, ekfvio_set_camera_model, the frame is that camera's: P in K's places)
        float P[4];
        const bool hasP = tc_ekf.rectifiedCamera(P);
        const float fx = (float)((double)(hasP ? P[0] : last_K_[0]) / scale_), fy = (float)((double)(hasP ? P[2] : last_K_[4]) / scale_);
        const float cx = (float)((double)(hasP ? P[1] : last_K_[2]) / scale_), cy = (float)((double)(hasP ? P[3] : last_K_[5]) / scale_);
        const std::vector<Vector3f> mus = tc_ekf.featureMus();
        const std::vector<uint8_t> flags = tc_ekf.deleteFlags();
        auto put = [&](int x, int y) {
            if (x < 0 || y < 0 || x >= w || y >= h) return;
            uint8_t* p = &o.bgr[3 * ((size_t)y * w + x)];
            p[0] = 0, p[1] = 255, p[2] = 0;  // cv::Scalar(0, 255, 0) in BGR
        };
        for (size_t i = 0; i < mus.size(); i++) {
            if (flags[i]) continue;  // if(!e.flaggedForDeletion()) (:386)
            const int px = (int)std::nearbyint(mus[i][0] * fx), py = (int)std::nearbyint(mus[i][1] * fy);  // cv::Point(Point2f): cvRound
            const int r = 22 / 2;  // drawMarker MARKER_SQUARE: the square (x +- size/2, y +- size/2), thickness 1
            for (int d = -r; d <= r; d++) {
                put(px + d, py - r), put(px + d, py + r);
                put(px - r, py + d), put(px + r, py + d);
            }
        }
        // cinfo.K.at(i) = f.K(i), linear index into a column-major Matrix3f (:408-416): the transpose of K
        const double Kcm[9] = {fx, 0, 0, 0, fy, 0, cx, cy, 1.0};
        for (int i = 0; i < 9; i++) o.K[i] = Kcm[i];
        o.P[0] = Kcm[0], o.P[2] = Kcm[2], o.P[5] = Kcm[4], o.P[6] = Kcm[5], o.P[10] = 1.0;  // (:419-423)
        return o;
    }
    // EKFVIO::imu_callback (EKFVIO.cpp:113-115).  With cfg.use_imu = 0 (the reference's behaviour) nothing happens.  With
    // cfg.use_imu = 1 the record is queued and applied, in stamp order, in front of the next frame whose stamp is not
    // older: ROS delivers 200 Hz IMU messages stamped AFTER an image before that image arrives, and a filter that had
    // already moved to the IMU stamp would have to refuse the image (dt < 0).  A record older than the filter's time
    // (it arrived after the frame that should have followed it) is dropped and counted, never an error.
    void imu_callback(double stamp, const Vector3f& gyro, const Vector3f& accel) {
        if (!use_imu_) {
            tc_ekf.chk(ekfvio_imu(tc_ekf.handle(), stamp, gyro.data(), accel.data()));  // the no-op, kept at the boundary
            return;
        }
        if (have_time_ && stamp < t_filter_) {
            dropped_imu_++;
            return;
        }
        ImuRecord r{stamp, gyro, accel};
        auto it = imu_queue_.end();
        while (it != imu_queue_.begin() && (it - 1)->stamp > stamp) --it;  // stable: equal stamps keep arrival order
        imu_queue_.insert(it, r);
        if (imu_queue_.size() > 1000) {  // the reference's subscriber queue length (EKFVIO.cpp:80)
            imu_queue_.pop_front();
            dropped_imu_++;
        }
    }
    // applies the queued IMU records with stamp <= until (addFrame does this itself)
    void drainImu(double until) {
        while (!imu_queue_.empty() && imu_queue_.front().stamp <= until) {
            const ImuRecord r = imu_queue_.front();
            imu_queue_.pop_front();
            if (have_time_ && r.stamp < t_filter_) {
                dropped_imu_++;
                continue;
            }
            if (align_left_ > 0) {  // the gravity alignment: averaged, not applied
                for (int k = 0; k < 3; k++) align_sum_[k] += (double)r.accel[k];
                align_left_--;
                if (!have_time_) {  // the first message of all only sets the filter's clock (ekfvio_imu), as without the alignment
                    tc_ekf.chk(ekfvio_imu(tc_ekf.handle(), r.stamp, r.gyro.data(), r.accel.data()));
                    t_filter_ = r.stamp;
                    have_time_ = true;
                }
                if (align_left_ == 0) {
                    const double mean[3] = {align_sum_[0] / align_samples_, align_sum_[1] / align_samples_, align_sum_[2] / align_samples_};
                    std::array<float, 9> R{};
                    std::array<float, 3> p{};
                    const bool on = tc_ekf.getImuExtrinsics(R, p);
                    Vector3f g{};
                    tc_ekf.chk(ekfvio_gravity_from_accel(on ? R.data() : nullptr, mean, (float)gravity_magnitude_, g.data()));
                    tc_ekf.setGravity(g);
                }
                continue;
            }
            tc_ekf.chk(ekfvio_imu(tc_ekf.handle(), r.stamp, r.gyro.data(), r.accel.data()));
            t_filter_ = r.stamp;
            have_time_ = true;
        }
    }
    // An aiding record in arrival order (ekfvio_aid): the IMU records up to its stamp first, then process(dt) to the stamp and the update.  A stamp
    // older than the filter's time is not applied (out-of-order records are not supported) and false is returned; the first stamp of all only
    // sets the filter's clock.
    bool aid(double stamp, int k, const float* H, const float* z, const float* R, float chi2 = 0.f) {
        drainImu(stamp);
        if (have_time_ && stamp < t_filter_) return false;
        tc_ekf.aid(stamp, k, H, z, R, chi2);
        t_filter_ = stamp;
        have_time_ = true;
        return true;
    }
    int droppedImuRecords() const { return dropped_imu_; }
    size_t queuedImuRecords() const { return imu_queue_.size(); }

   private:
    struct ImuRecord {
        double stamp;
        Vector3f gyro, accel;
    };
    double last_stamp_ = 0;
    double t_filter_ = 0;  // the stamp the device state stands at (last frame or IMU record applied)
    bool have_time_ = false;
    bool use_imu_ = false;
    int scale_ = 1;
    std::array<float, 9> last_K_{};
    std::deque<ImuRecord> imu_queue_;
    int dropped_imu_ = 0;
    int align_samples_ = 0, align_left_ = 0;  // the gravity alignment: records to average in all, and still to come
    double align_sum_[3] = {0.0, 0.0, 0.0};
    double gravity_magnitude_ = 9.81;  // |cfg.gravity|
};

}  // namespace ekfvio
