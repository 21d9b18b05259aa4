// ekf_vio_amd/host/replay_main.cpp — ROS-free replay / smoke driver for the C++ host shim.
//
// Runs the synthetic closed loop of the reference's test/analyzeEKFSimulation.cpp:10-125
// (N landmarks, truth integrated with the filter's own motion model, perfect projections,
// R = 1e-5 I, every landmark measured) through ekfvio::TightlyCoupledEKF and prints the
// final odometry next to the ground truth, the checkSigma numbers and the step rate.
// Usage: ekfvio_replay [landmarks=256] [frames=300] [seed=0] [dt=0.0333333]
//        ekfvio_replay --print-config [params.yaml] [--nhc-variance v] [--nhc-R-cv "r00 ... r22"]
//                                                      (no GPU work: the node's parameter file -> ekfvio_config as JSON)
//        ekfvio_replay --records <dir> [--out <dir>] [--params params.yaml] [--device n] [--insight] [--covariance]
//                                [--equalize-clip-limit c] [--equalize-tiles-x n] [--equalize-tiles-y n] [--tracks FILE] [--ended FILE]
//                                [--zupt-max-flow-px p] [--zupt-min-tracks n] [--zupt-min-ratio r] [--zupt-vel-variance v] [--zupt-omega-variance v]
//                                [--imu-rotation "r00 r01 ... r22"] [--imu-position "x y z"] [--gravity-align-samples k]
//                                [--replenish-grid-x n] [--replenish-grid-y n] [--nhc-variance v] [--nhc-R-cv "r00 r01 ... r22"]
//                                [--distortion-model plumb_bob|rational_polynomial|equidistant|fisheye] [--rectified-camera "fx fy cx cy"]
//
// --distortion-model and --rectified-camera are the node parameters distortion_model and rectified_fx/fy/cx/cy (ekfvio_set_camera_model; live
// with rectify: 1 and the distortion_* coefficients in the parameter file): the records' K stays the raw camera's, the outputs are the
// rectified camera's.
// --records replays what the node's two subscriptions deliver (EKFVIO.cpp:69-81) and writes what its two publishers
// send (EKFVIO.cpp:444-518), with no ROS in between.  <dir>/records.txt holds one record per line, in arrival order:
//     image <stamp> <file> <K0> ... <K8>      8-bit binary PGM (P5), intrinsics row-major as in sensor_msgs/CameraInfo.K
//     imu   <stamp> <gx> <gy> <gz> <ax> <ay> <az>
//     aid   <stamp> <k> <H: 22 k numbers, row-major> <z: k> <R: k k, row-major, lower triangle read> [chi2]
// An aid record is a linear aiding measurement of the base state (ekfvio_aid: wheel speed, a position fix): the filter is propagated to its
// stamp and updated; a record older than the filter's time is counted and skipped.  --nhc-variance v (and --nhc-R-cv, vehicle -> camera axes)
// are the node parameters nhc_variance / nhc_R_cv: the nonholonomic constraint as a standing measurement in every frame (ekfvio_set_frame_aid).
// Every image record goes through EKFVIO::addFrame (frame ingest, process(dt), KLT, update, FAST replenishment:
// cfg.replenish = 1); after it one odometry record and one point-cloud record are appended to
//     <out>/odom.txt     stamp px py pz qw qx qy qz vx vy vz wx wy wz numeric_ok
//     <out>/points.txt   "cloud <stamp> <n>" followed by n lines "x y z intensity"
// (floats printed with %.9g: exact).  IMU records go to imu_callback, a logging stub in the reference (with imu_update: 1 in
// the parameter file they are queued and applied in stamp order in front of the next frame).  --insight also writes what
// publishInsight sends, <out>/insight_NNN.ppm.  --covariance turns on the covariances of the outputs (ekfvio_set_output_covariance) and
// prints, per frame, the diagonals of the pose and twist covariances the node would put into nav_msgs/Odometry:
//     cov <stamp> <6 pose variances: x y z rotX rotY rotZ> <6 twist variances: linear, angular>
// --equalize-clip-limit / --equalize-tiles-x / --equalize-tiles-y are the node parameters of the same names (ekfvio_set_equalize), applied
// behind the parameter file, and so are the five --zupt-* options (ekfvio_set_zupt; --print-config echoes the parameters) and --imu-rotation (nine numbers, row-major,
// IMU -> camera axes) / --imu-position (three numbers, metres) / --gravity-align-samples (ekfvio_set_imu_extrinsics, ekfvio_set_gravity: the node
// parameters imu_rotation, imu_position, gravity_align_samples).  --replenish-grid-x / --replenish-grid-y set the grid the new landmarks are
// spread over (ekfvio_set_replenish_grid: the node parameters replenish_grid_x, replenish_grid_y; 0 0 = off).  --tracks FILE writes one line per live landmark per frame, behind the frame,
//     frame stamp id born x y z
// (ekfvio_get_landmark_ids beside the cloud: one landmark's depth over time is the lines with its id).  --ended FILE turns the export of the
// tracks that ended on (ekfvio_set_ended_export; the replay itself removes lost landmarks only with remove_lost: 1 in the parameter file) and
// writes one line per ended record, read after every frame:
//     frame stamp id born index_before x y z c00 c01 c02 c10 c11 c12 c20 c21 c22
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>

#include "ekfvio.hpp"

namespace {
struct SplitMix64 {
    uint64_t s;
    uint64_t next() {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double uniform(double lo, double hi) { return lo + (hi - lo) * ((next() >> 11) * (1.0 / 9007199254740992.0)); }
    double gaussian(double sigma) {
        double u1 = std::fmax(uniform(0, 1), 1e-300), u2 = uniform(0, 1);
        return sigma * std::sqrt(-2.0 * std::log(u1)) * std::cos(2.0 * M_PI * u2);
    }
};
struct V3 {
    double x, y, z;
};
struct Q {
    double w, x, y, z;
};
V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
V3 rot(Q q, V3 v) {
    V3 qv{q.x, q.y, q.z}, uv = cross(qv, v);
    uv = {2 * uv.x, 2 * uv.y, 2 * uv.z};
    V3 c = cross(qv, uv);
    return {v.x + q.w * uv.x + c.x, v.y + q.w * uv.y + c.y, v.z + q.w * uv.z + c.z};
}
Q mul(Q a, Q b) {
    return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
            a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z, a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
}
}  // namespace

static int print_config(const char* path, const std::vector<std::pair<std::string, std::string>>& overrides) {
    try {
        ekfvio::Params p = path ? ekfvio::Params::fromFile(path) : ekfvio::Params();
        for (const auto& kv : overrides) p.set(kv.first, kv.second);
        const ekfvio_config& c = p.cfg;
        std::printf("{\"max_features\": %d, \"fast_threshold\": %d, \"fast_blur_sigma\": %.9g, \"inverse_image_scale\": %d, "
                    "\"kill_pad\": %d, \"klt_min_eigen\": %.9g, \"min_new_feature_dist\": %d, \"klt_max_pyramid_level\": %d, "
                    "\"klt_window_size\": %d, \"default_point_depth\": %.9g, \"default_point_depth_variance\": %.9g, "
                    "\"default_point_homogenous_variance\": %.9g, \"sample_based_uncertainty\": %d, \"gate_chi2\": %.9g, "
                    "\"klt_fb_max_px\": %.9g, \"rectify\": %d, \"publish_covariance\": %d, \"mask_rectify_border\": %d, \"equalize_clip_limit\": %.9g, \"equalize_tiles_x\": %d, \"equalize_tiles_y\": %d, \"klt_photometric\": %d, \"publish_ids\": %d, \"publish_ended\": %d, \"zupt_max_flow_px\": %.9g, \"zupt_min_tracks\": %d, \"zupt_min_ratio\": %.9g, \"zupt_vel_variance\": %.9g, \"zupt_omega_variance\": %.9g, \"imu_extrinsics\": %d, \"imu_rotation\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g], \"imu_position\": [%.9g, %.9g, %.9g], \"gravity_align_samples\": %d, \"replenish_grid_x\": %d, \"replenish_grid_y\": %d, \"nhc_variance\": %.9g, \"nhc_R_cv\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g], \"distortion\": [%.17g, %.17g, %.17g, %.17g, %.17g], \"distortion_model\": \"%s\", \"distortion_k456\": [%.17g, %.17g, %.17g], \"rectified\": [%.9g, %.9g, %.9g, %.9g], \"node\": {",
                    c.max_features, c.fast_threshold, (double)c.fast_blur_sigma, c.inverse_image_scale, c.kill_pad,
                    (double)c.klt_min_eigen, c.min_new_feature_dist, c.klt_max_pyramid_level, c.klt_window_size,
                    (double)c.default_point_depth, (double)c.default_point_depth_variance,
                    (double)c.default_point_homogenous_variance, c.sample_based_uncertainty, (double)p.gate_chi2,
                    (double)c.klt_fb_max_px, p.rectify, p.publish_covariance, p.mask_rectify_border, (double)p.equalize_clip_limit, p.equalize_tiles_x, p.equalize_tiles_y, p.klt_photometric, p.publish_ids, p.publish_ended, (double)p.zupt_max_flow_px, p.zupt_min_tracks, (double)p.zupt_min_ratio, (double)p.zupt_vel_variance, (double)p.zupt_omega_variance, p.imu_extrinsics,
                    (double)p.imu_rotation[0], (double)p.imu_rotation[1], (double)p.imu_rotation[2], (double)p.imu_rotation[3], (double)p.imu_rotation[4],
                    (double)p.imu_rotation[5], (double)p.imu_rotation[6], (double)p.imu_rotation[7], (double)p.imu_rotation[8],
                    (double)p.imu_position[0], (double)p.imu_position[1], (double)p.imu_position[2], p.gravity_align_samples, p.replenish_grid_x, p.replenish_grid_y, (double)p.nhc_variance,
                    (double)p.nhc_R_cv[0], (double)p.nhc_R_cv[1], (double)p.nhc_R_cv[2], (double)p.nhc_R_cv[3], (double)p.nhc_R_cv[4], (double)p.nhc_R_cv[5],
                    (double)p.nhc_R_cv[6], (double)p.nhc_R_cv[7], (double)p.nhc_R_cv[8], p.distortion[0], p.distortion[1], p.distortion[2], p.distortion[3], p.distortion[4],
                    p.distortion_model.c_str(), p.distortion_k456[0], p.distortion_k456[1], p.distortion_k456[2],
                    (double)p.rectified[0], (double)p.rectified[1], (double)p.rectified[2], (double)p.rectified[3]);
        bool first = true;
        for (const auto& e : p.node) {
            std::printf("%s\"%s\": \"%s\"", first ? "" : ", ", e.first.c_str(), e.second.c_str());
            first = false;
        }
        std::printf("}}\n");
        return 0;
    } catch (const ekfvio::Error& e) {
        std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 2;
    }
}


// 8-bit binary PGM ("P5", optional comments, maxval 255)
static bool read_pgm(const std::string& path, std::vector<uint8_t>& px, int& w, int& h) {
    std::ifstream in(path, std::ios::binary);
    if (!in) return false;
    std::string magic;
    in >> magic;
    if (magic != "P5") return false;
    int vals[3], got = 0;
    while (got < 3) {
        int c = in.peek();
        if (c == '#') {
            std::string skip;
            std::getline(in, skip);
        } else if (std::isspace(c)) {
            in.get();
        } else if (!(in >> vals[got++])) {
            return false;
        }
    }
    in.get();  // the single whitespace byte behind maxval
    w = vals[0];
    h = vals[1];
    if (w < 1 || h < 1 || vals[2] != 255) return false;
    px.resize((size_t)w * h);
    in.read(reinterpret_cast<char*>(px.data()), (std::streamsize)px.size());
    return (size_t)in.gcount() == px.size();
}

static int replay_records(const std::string& dir, const std::string& out_dir, const char* params_path, int device, bool insight, bool covariance,
                          const std::vector<std::pair<std::string, std::string>>& overrides, const char* tracks_path, const char* ended_path) {
    try {
        ekfvio::Params p = params_path ? ekfvio::Params::fromFile(params_path) : ekfvio::Params();
        for (const auto& kv : overrides) p.set(kv.first, kv.second);
        if (!params_path) p.cfg.inverse_image_scale = 1;  // no parameter file: frames are used as recorded
        p.cfg.replenish = 1;                              // addFrame runs replenishFeatures itself (EKFVIO.cpp:154, :172)
        if (covariance) p.publish_covariance = 1;
        if (ended_path) p.publish_ended = 1;
        std::ifstream rec(dir + "/records.txt");
        if (!rec) throw ekfvio::Error(EKFVIO_EINVAL, "cannot open " + dir + "/records.txt");
        // no image size anywhere: the device planes grow with the first frame that needs it (Frame::Frame takes any image)
        std::vector<uint8_t> px;
        ekfvio::EKFVIO node(p, device);
        FILE* fo = std::fopen((out_dir + "/odom.txt").c_str(), "w");
        FILE* fp = std::fopen((out_dir + "/points.txt").c_str(), "w");
        if (!fo || !fp) throw ekfvio::Error(EKFVIO_EINVAL, "cannot write into " + out_dir);
        FILE* ft = tracks_path ? std::fopen(tracks_path, "w") : nullptr;
        FILE* fe = ended_path ? std::fopen(ended_path, "w") : nullptr;
        if ((tracks_path && !ft) || (ended_path && !fe)) throw ekfvio::Error(EKFVIO_EINVAL, "cannot write the tracks / ended file");
        std::string line;
        int images = 0, imus = 0, aids = 0, aids_late = 0, lineno = 0;
        const auto t0 = std::chrono::steady_clock::now();
        while (std::getline(rec, line)) {
            lineno++;
            std::istringstream ls(line);
            std::string kind;
            if (!(ls >> kind) || kind[0] == '#') continue;
            double stamp;
            if (!(ls >> stamp)) throw ekfvio::Error(EKFVIO_EINVAL, "records.txt line " + std::to_string(lineno) + ": no stamp");
            if (kind == "imu") {
                ekfvio::Vector3f g, a;
                if (!(ls >> g[0] >> g[1] >> g[2] >> a[0] >> a[1] >> a[2]))
                    throw ekfvio::Error(EKFVIO_EINVAL, "records.txt line " + std::to_string(lineno) + ": imu needs 6 numbers");
                node.imu_callback(stamp, g, a);
                imus++;
            } else if (kind == "aid") {
                int k = 0;
                if (!(ls >> k) || k < 1 || k > 6) throw ekfvio::Error(EKFVIO_EINVAL, "records.txt line " + std::to_string(lineno) + ": aid needs a row count 1..6");
                std::vector<float> v((size_t)(22 * k + k + k * k));
                for (float& x : v)
                    if (!(ls >> x)) throw ekfvio::Error(EKFVIO_EINVAL, "records.txt line " + std::to_string(lineno) + ": aid needs 22 k + k + k k numbers");
                float chi2 = 0.f;
                ls >> chi2;  // (optional)
                if (node.aid(stamp, k, v.data(), v.data() + 22 * k, v.data() + 23 * k, chi2)) aids++;
                else aids_late++;
            } else if (kind == "image") {
                std::string file;
                ekfvio::Frame f;
                ls >> file;
                for (int i = 0; i < 9; i++)
                    if (!(ls >> f.K[i])) throw ekfvio::Error(EKFVIO_EINVAL, "records.txt line " + std::to_string(lineno) + ": image needs a file and K (9 numbers)");
                int fw, fh;
                if (!read_pgm(dir + "/" + file, px, fw, fh)) throw ekfvio::Error(EKFVIO_EINVAL, "cannot read " + file);
                f.img = px.data();
                f.cols = fw;
                f.rows = fh;
                f.step = fw;
                f.t = stamp;
                const bool ok = node.addFrame(f);
                const ekfvio::Odometry od = node.odometry();     // publishOdometry (EKFVIO.cpp:444-477)
                const ekfvio::PointCloud pc = node.points();     // publishPoints   (EKFVIO.cpp:479-518)
                std::fprintf(fo, "%.9f %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %d\n", od.stamp, od.position[0],
                             od.position[1], od.position[2], od.orientation_wxyz[0], od.orientation_wxyz[1], od.orientation_wxyz[2],
                             od.orientation_wxyz[3], od.linear[0], od.linear[1], od.linear[2], od.angular[0], od.angular[1],
                             od.angular[2], (int)ok);
                std::fprintf(fp, "cloud %.9f %zu\n", pc.stamp, pc.points.size());
                for (size_t i = 0; i < pc.points.size(); i++)
                    std::fprintf(fp, "%.9g %.9g %.9g %.9g\n", pc.points[i][0], pc.points[i][1], pc.points[i][2], pc.intensity[i]);
                if (ft) {  // the landmarks' identities beside the cloud: a memcpy behind the frame
                    const ekfvio::TightlyCoupledEKF::LandmarkIds li = node.tc_ekf.getLandmarkIds();
                    for (size_t i = 0; i < pc.points.size(); i++)
                        std::fprintf(ft, "%d %.9f %lld %.9f %.9g %.9g %.9g\n", images, pc.stamp, (long long)li.id[i], li.born[i], pc.points[i][0],
                                     pc.points[i][1], pc.points[i][2]);
                }
                if (fe) {  // the records of the landmarks this frame's removal took out
                    const ekfvio::TightlyCoupledEKF::Ended en = node.tc_ekf.getEnded();
                    for (size_t i = 0; i < en.id.size(); i++) {
                        std::fprintf(fe, "%d %.9f %lld %.9f %d %.9g %.9g %.9g", images, pc.stamp, (long long)en.id[i], en.born[i], en.index_before[i],
                                     en.xyz[i][0], en.xyz[i][1], en.xyz[i][2]);
                        for (int c = 0; c < 9; c++) std::fprintf(fe, " %.9g", en.cov[i][c]);
                        std::fprintf(fe, "\n");
                    }
                }
                if (covariance) {  // what the node fills pose.covariance / twist.covariance from: a memcpy behind the frame
                    const ekfvio::TightlyCoupledEKF::OdometryCovariance oc = node.tc_ekf.getOdometryCovariance();
                    std::printf("cov %.9f", od.stamp);
                    for (int i = 0; i < 6; i++) std::printf(" %.9g", oc.pose[7 * i]);
                    for (int i = 0; i < 6; i++) std::printf(" %.9g", oc.twist[7 * i]);
                    std::printf("\n");
                }
                if (insight) {  // publishInsight (EKFVIO.cpp:379-442) as a binary PPM (RGB order on disk)
                    const ekfvio::Insight in = node.insight();
                    char name[64];
                    std::snprintf(name, sizeof name, "/insight_%03d.ppm", images);
                    FILE* fi = std::fopen((out_dir + name).c_str(), "wb");
                    if (!fi) throw ekfvio::Error(EKFVIO_EINVAL, "cannot write into " + out_dir);
                    std::fprintf(fi, "P6\n%d %d\n255\n", in.width, in.height);
                    std::vector<uint8_t> rgb(in.bgr.size());
                    for (size_t i = 0; i + 2 < rgb.size(); i += 3) rgb[i] = in.bgr[i + 2], rgb[i + 1] = in.bgr[i + 1], rgb[i + 2] = in.bgr[i];
                    std::fwrite(rgb.data(), 1, rgb.size(), fi);
                    std::fclose(fi);
                }
                images++;
            } else {
                throw ekfvio::Error(EKFVIO_EINVAL, "records.txt line " + std::to_string(lineno) + ": unknown record kind " + kind);
            }
        }
        std::fclose(fo);
        std::fclose(fp);
        if (ft) std::fclose(ft);
        if (fe) std::fclose(fe);
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("records: %d images, %d imu; %d landmarks; %.1f frames/s (file reading included)\n", images, imus,
                    node.tc_ekf.numFeatures(), images / el);
        if (aids || aids_late || p.nhc_variance > 0.f) {
            const ekfvio::TightlyCoupledEKF::AidStatus as = node.tc_ekf.aidStatus();
            std::printf("aid: %d records applied to the filter, %d skipped (older than the filter's time); updates accepted %lld, rejected %lld, last d2 %.6g\n",
                        aids, aids_late, (long long)as.applied_total, (long long)as.rejected_total, (double)as.d2_last);
        }
        if (p.cfg.use_imu)
            std::printf("imu: %d records dropped (older than the filter's time), %zu still queued behind the last frame\n",
                        node.droppedImuRecords(), node.queuedImuRecords());
        return 0;
    } catch (const ekfvio::Error& e) {
        std::fprintf(stderr, "ekfvio error %d: %s\n", e.code, e.what());
        return 1;
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--print-config") == 0) {
        const char* path = argc > 2 && std::strncmp(argv[2], "--", 2) != 0 ? argv[2] : nullptr;
        std::vector<std::pair<std::string, std::string>> overrides;
        for (int i = path ? 3 : 2; i < argc; i += 2) {
            if (i + 1 < argc && std::strcmp(argv[i], "--nhc-variance") == 0) overrides.emplace_back("nhc_variance", argv[i + 1]);
            else if (i + 1 < argc && std::strcmp(argv[i], "--nhc-R-cv") == 0) overrides.emplace_back("nhc_R_cv", argv[i + 1]);
            else {
                std::fprintf(stderr, "error: --print-config takes a parameter file, --nhc-variance v and --nhc-R-cv \"...\"\n");
                return 2;
            }
        }
        return print_config(path, overrides);
    }
    if (argc > 2 && std::strcmp(argv[1], "--records") == 0) {
        std::string dir = argv[2], out = argv[2];
        const char* params = nullptr;
        int device = 0;
        bool insight = false, covariance = false;
        const char *tracks = nullptr, *ended = nullptr;
        std::vector<std::pair<std::string, std::string>> overrides;  // options that are node parameters, by the parameter's name
        for (int i = 3; i < argc; i += 2) {
            if (std::strcmp(argv[i], "--insight") == 0 || std::strcmp(argv[i], "--covariance") == 0) {
                (std::strcmp(argv[i], "--insight") == 0 ? insight : covariance) = true;
                i--;
                continue;
            }
            if (i + 1 >= argc) {
                std::fprintf(stderr, "option %s needs a value\n", argv[i]);
                return 2;
            }
            if (std::strcmp(argv[i], "--out") == 0) out = argv[i + 1];
            else if (std::strcmp(argv[i], "--params") == 0) params = argv[i + 1];
            else if (std::strcmp(argv[i], "--device") == 0) device = std::atoi(argv[i + 1]);
            else if (std::strcmp(argv[i], "--tracks") == 0) tracks = argv[i + 1];
            else if (std::strcmp(argv[i], "--ended") == 0) ended = argv[i + 1];
            else if (std::strcmp(argv[i], "--equalize-clip-limit") == 0) overrides.emplace_back("equalize_clip_limit", argv[i + 1]);
            else if (std::strcmp(argv[i], "--equalize-tiles-x") == 0) overrides.emplace_back("equalize_tiles_x", argv[i + 1]);
            else if (std::strcmp(argv[i], "--equalize-tiles-y") == 0) overrides.emplace_back("equalize_tiles_y", argv[i + 1]);
            else if (std::strcmp(argv[i], "--zupt-max-flow-px") == 0) overrides.emplace_back("zupt_max_flow_px", argv[i + 1]);
            else if (std::strcmp(argv[i], "--zupt-min-tracks") == 0) overrides.emplace_back("zupt_min_tracks", argv[i + 1]);
            else if (std::strcmp(argv[i], "--zupt-min-ratio") == 0) overrides.emplace_back("zupt_min_ratio", argv[i + 1]);
            else if (std::strcmp(argv[i], "--zupt-vel-variance") == 0) overrides.emplace_back("zupt_vel_variance", argv[i + 1]);
            else if (std::strcmp(argv[i], "--zupt-omega-variance") == 0) overrides.emplace_back("zupt_omega_variance", argv[i + 1]);
            else if (std::strcmp(argv[i], "--imu-rotation") == 0) overrides.emplace_back("imu_rotation", argv[i + 1]);
            else if (std::strcmp(argv[i], "--imu-position") == 0) overrides.emplace_back("imu_position", argv[i + 1]);
            else if (std::strcmp(argv[i], "--gravity-align-samples") == 0) overrides.emplace_back("gravity_align_samples", argv[i + 1]);
            else if (std::strcmp(argv[i], "--replenish-grid-x") == 0) overrides.emplace_back("replenish_grid_x", argv[i + 1]);
            else if (std::strcmp(argv[i], "--replenish-grid-y") == 0) overrides.emplace_back("replenish_grid_y", argv[i + 1]);
            else if (std::strcmp(argv[i], "--nhc-variance") == 0) overrides.emplace_back("nhc_variance", argv[i + 1]);
            else if (std::strcmp(argv[i], "--nhc-R-cv") == 0) overrides.emplace_back("nhc_R_cv", argv[i + 1]);
            else if (std::strcmp(argv[i], "--distortion-model") == 0) overrides.emplace_back("distortion_model", argv[i + 1]);
            else if (std::strcmp(argv[i], "--rectified-camera") == 0) {  // "fx fy cx cy": the four rectified_* parameters
                std::istringstream in(argv[i + 1]);
                std::string tok[4], extra;
                if (!(in >> tok[0] >> tok[1] >> tok[2] >> tok[3]) || (in >> extra)) {
                    std::fprintf(stderr, "option --rectified-camera needs \"fx fy cx cy\"\n");
                    return 2;
                }
                const char* names[4] = {"rectified_fx", "rectified_fy", "rectified_cx", "rectified_cy"};
                for (int k = 0; k < 4; k++) overrides.emplace_back(names[k], tok[k]);
            }
            else {
                std::fprintf(stderr, "unknown option %s\n", argv[i]);
                return 2;
            }
        }
        return replay_records(dir, out, params, device, insight, covariance, overrides, tracks, ended);
    }
    const int N = argc > 1 ? std::atoi(argv[1]) : 256;
    const int frames = argc > 2 ? std::atoi(argv[2]) : 300;
    const uint64_t seed = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 0;
    const float dt = argc > 4 ? (float)std::atof(argv[4]) : (float)(1.0 / 30.0);
    try {
        ekfvio::TightlyCoupledEKF ekf(N, 0);
        SplitMix64 rng{seed};
        std::vector<V3> pts(N);
        std::vector<ekfvio::Vector2f> uv(N);
        for (int i = 0; i < N; i++) {
            double z = 0.5 + rng.gaussian(0.01);
            double x = rng.uniform(-1.5, 1.5) * z, y = rng.uniform(-1.5, 1.5) * z;
            pts[i] = {x, y, z};
            uv[i] = {(float)(x / z), (float)(y / z)};
        }
        ekf.addNewFeatures(uv);
        V3 pos{0, 0, 0}, vel{-0.1, 0, -0.1}, acc{0, 0, 0}, om{0, 0.1, 0};
        Q quat{1, 0, 0, 0};
        std::vector<ekfvio::Vector2f> z(N);
        std::vector<ekfvio::Matrix2f> R(N, ekfvio::Matrix2f{1e-5f, 0, 0, 1e-5f});
        std::vector<uint8_t> pass(N, 1);
        bool numeric_ok = true;
        auto t0 = std::chrono::steady_clock::now();
        for (int s = 0; s < frames; s++) {
            const double d = dt;
            V3 tr{d * vel.x + 0.5 * d * d * acc.x, d * vel.y + 0.5 * d * d * acc.y, d * vel.z + 0.5 * d * d * acc.z};
            V3 dp = rot(quat, tr);
            pos = {pos.x + dp.x, pos.y + dp.y, pos.z + dp.z};
            const double on = std::sqrt(om.x * om.x + om.y * om.y + om.z * om.z), th = d * on;
            Q dq = on < 1e-10 ? Q{1, 0, 0, 0} : Q{std::cos(th / 2), om.x / on * std::sin(th / 2), om.y / on * std::sin(th / 2),
                                                   om.z / on * std::sin(th / 2)};
            Q dqi{dq.w, -dq.x, -dq.y, -dq.z};
            vel = rot(dqi, {vel.x + d * acc.x, vel.y + d * acc.y, vel.z + d * acc.z});
            acc = rot(dqi, acc);
            quat = mul(quat, dq);
            Q qi{quat.w, -quat.x, -quat.y, -quat.z};
            for (int i = 0; i < N; i++) {
                V3 fp = rot(qi, {pts[i].x - pos.x, pts[i].y - pos.y, pts[i].z - pos.z});
                z[i] = {(float)(fp.x / fp.z), (float)(fp.y / fp.z)};
            }
            ekf.process(dt);
            numeric_ok &= ekf.updateWithFeaturePositions(z, R, pass);
        }
        auto b = ekf.base_mu();
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        float md = 0, ma = 0;
        ekf.checkSigma(&md, &ma);
        std::printf("landmarks %d frames %d steps_per_s %.1f numeric_ok %d\n", N, frames, frames / el, (int)numeric_ok);
        std::printf("est_pos %.6f %.6f %.6f truth_pos %.6f %.6f %.6f\n", b[0], b[1], b[2], pos.x, pos.y, pos.z);
        std::printf("est_vel %.6f %.6f %.6f truth_vel %.6f %.6f %.6f\n", b[7], b[8], b[9], vel.x, vel.y, vel.z);
        std::printf("est_quat %.6f %.6f %.6f %.6f truth_quat %.6f %.6f %.6f %.6f\n", b[3], b[4], b[5], b[6], quat.w, quat.x,
                    quat.y, quat.z);
        std::printf("min_diag %.3e max_asym %.3e\n", md, ma);
        const double perr = std::fmax(std::fabs(b[0] - pos.x), std::fmax(std::fabs(b[1] - pos.y), std::fabs(b[2] - pos.z)));
        return (frames >= 60 && perr > 0.02) || md < 0 ? 2 : 0;
    } catch (const ekfvio::Error& e) {
        std::fprintf(stderr, "ekfvio error %d: %s\n", e.code, e.what());
        return 1;
    }
}
