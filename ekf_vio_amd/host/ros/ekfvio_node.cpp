// ekf_vio_amd/host/ros/ekfvio_node.cpp -- the ROS1 front end of the reference node (src/ekfvio_node.cpp:14-21,
// include/ekf_vio/EKFVIO.cpp:10-137 and :379-518) over the MI355X backend: same private parameters, same subscriptions
// (image_transport camera topic, queue 10; IMU topic, queue 1000), same publications (nav_msgs/Odometry, sensor_msgs/
// PointCloud with an "intensity" channel, optional insight image + camera info, the world -> odom transform) and the same
// start-up wait for the base -> camera transform.  Everything between the callbacks and the publishers is
// ekfvio::EKFVIO::addFrame, i.e. the C-ABI of libekfvio_hip.so.
//
// Built only inside a catkin workspace (INTEGRATION.md section 5 has the CMake lines); this repository's own build and
// tests never compile it: neither the build container nor the GPU boxes have ROS.  Without <ros/ros.h> on the include
// path the translation unit is empty.
//
// Names: the reference's launch files still start `invio_node` from package `invio` (launch/simLaunch.launch:9) while
// its CMake builds `ekfvio_node` in package `ekf_vio` (CMakeLists.txt:2,77); the topics keep their `invio/...` defaults
// (Params.h:19-20,111-113).  This node is `ekfvio_node`, and the topic defaults are the reference's.
#if __has_include(<ros/ros.h>)
#include <image_transport/image_transport.h>
#include <nav_msgs/Odometry.h>
#include <ros/ros.h>
#include <sensor_msgs/CameraInfo.h>
#include <sensor_msgs/Image.h>
#include <sensor_msgs/Imu.h>
#include <sensor_msgs/PointCloud.h>
#include <sensor_msgs/image_encodings.h>
#include <tf/transform_broadcaster.h>
#include <tf/transform_listener.h>

#include <memory>
#include <sstream>

#include "../ekfvio.hpp"

namespace {

std::string to_text(XmlRpc::XmlRpcValue& v) {
    std::ostringstream os;
    os.precision(17);
    switch (v.getType()) {
        case XmlRpc::XmlRpcValue::TypeBoolean: os << (static_cast<bool>(v) ? "true" : "false"); break;
        case XmlRpc::XmlRpcValue::TypeInt: os << static_cast<int>(v); break;
        case XmlRpc::XmlRpcValue::TypeDouble: os << static_cast<double>(v); break;
        case XmlRpc::XmlRpcValue::TypeString: os << static_cast<std::string>(v); break;
        default: throw ekfvio::Error(EKFVIO_EINVAL, "parameter of unsupported type");
    }
    return os.str();
}

// 8-bit grey view of an incoming image.  The reference hands the image to OpenCV in whatever encoding arrives
// (EKFVIO.cpp:124); the device pyramid is single-channel, so colour is reduced with the BT.601 integer weights.
bool to_grey(const sensor_msgs::Image& img, std::vector<uint8_t>& grey, const uint8_t*& data, int& step) {
    namespace enc = sensor_msgs::image_encodings;
    if (img.encoding == enc::MONO8 || img.encoding == enc::TYPE_8UC1) {
        data = img.data.data();
        step = (int)img.step;
        return true;
    }
    const bool rgb = img.encoding == enc::RGB8, bgr = img.encoding == enc::BGR8;
    const bool rgba = img.encoding == enc::RGBA8, bgra = img.encoding == enc::BGRA8;
    if (!(rgb || bgr || rgba || bgra)) return false;
    const int ch = (rgb || bgr) ? 3 : 4;
    grey.resize((size_t)img.width * img.height);
    for (uint32_t y = 0; y < img.height; y++) {
        const uint8_t* row = img.data.data() + (size_t)y * img.step;
        for (uint32_t x = 0; x < img.width; x++) {
            const uint8_t* p = row + (size_t)x * ch;
            const int r = (rgb || rgba) ? p[0] : p[2], g = p[1], b = (rgb || rgba) ? p[2] : p[0];
            grey[(size_t)y * img.width + x] = (uint8_t)((77 * r + 150 * g + 29 * b + 128) >> 8);
        }
    }
    data = grey.data();
    step = (int)img.width;
    return true;
}

// CameraInfo.distortion_model where the message type carries it (sensor_msgs of every ROS release does; a declaration-only stand-in
// for the header may carry D alone, and is then taken at its word)
template <class Info>
auto distortion_model_of(const Info& c, int) -> decltype(std::string(c.distortion_model)) {
    return c.distortion_model;
}
template <class Info>
std::string distortion_model_of(const Info&, long) {
    return "plumb_bob";
}

// pose.covariance / twist.covariance (row-major 6x6, float64) where the message type carries them (geometry_msgs/PoseWithCovariance and
// TwistWithCovariance of every ROS release do; a declaration-only stand-in for the header may not, and then has nothing to fill)
template <class WithCovariance>
auto fill_covariance(WithCovariance& m, const std::array<float, 36>& c, int) -> decltype((void)(m.covariance[0] = 0.0)) {
    for (size_t i = 0; i < 36; i++) m.covariance[i] = (double)c[i];  // widened, never recomputed
}
template <class WithCovariance>
void fill_covariance(WithCovariance&, const std::array<float, 36>&, long) {}
#ifdef EKFVIO_NODE_REQUIRE_COVARIANCE  // for a build that must not lose the covariances to the fallback above (tests/test_gpu_host_shim_covout.py)
static_assert(sizeof(nav_msgs::Odometry().pose.covariance) == 36 * sizeof(double) && sizeof(nav_msgs::Odometry().twist.covariance) == 36 * sizeof(double),
              "nav_msgs/Odometry without pose.covariance / twist.covariance");
#endif

class EkfvioNode {
   public:
    EkfvioNode() : it_(nh_) {
        // the ~48 private parameters of EKFVIO::EKFVIO (EKFVIO.cpp:20-67) by the reference's names
        // (and this backend's own: imu_update, remove_lost, gate_chi2, klt_fb_max_px -- the tracker's forward-backward threshold in pixels of
        // the resized frame, which reaches the handle inside ekfvio_config -- and publish_covariance, default false: with it the handle is
        // told at start-up, by ekfvio::EKFVIO's constructor, to deliver the covariances with every frame's outputs; mask_rectify_border, default
        // false: with it, and rectify = 1, the black border that rectification leaves is no-data for the detector and the tracker, ekfvio_set_mask;
        // equalize_clip_limit, default 0 = off, with equalize_tiles_x / equalize_tiles_y, default 8: every frame is equalised on the device in front
        // of its pyramid, ekfvio_set_equalize; klt_photometric, default 0 = off: the tracker matches up to a gain and an offset,
        // ekfvio_set_klt_photometric; publish_ids, default false: the PointCloud gets a second channel "id" with every landmark's id as a float --
        // exact below 2^24 = 16 777 216, beyond that id mod 2^24, so that equal floats within one cloud still mean one landmark;
        // publish_ended, default false: the handle is told to export the tracks that ended, ekfvio_set_ended_export, and their records go out
        // behind every frame as a second PointCloud on ended_topic, default invio/ended_points, with the channels "id", "born" (seconds before
        // the message's stamp: a float cannot hold a ROS stamp), "index_before" and the nine covariance entries "c00" .. "c22";
        // zupt_max_flow_px, default 0 = off, with zupt_min_tracks 8, zupt_min_ratio 0.75, zupt_vel_variance and zupt_omega_variance 1e-4: a frame
        // whose tracks stand still updates the velocity and the body rate with z = 0 on the device, ekfvio_set_zupt, told at start-up likewise;
        // imu_rotation, nine numbers row-major, and imu_position, three numbers in metres, each given as ONE STRING of numbers separated by
        // blanks or commas (a YAML list is a parameter of unsupported type here): the rotation and translation of Kalibr's T_cam_imu,
        // ekfvio_set_imu_extrinsics, so that imu_update models the IMU in its own frame; gravity_align_samples, default 0 = off: that many IMU
        // records at the start are averaged, not applied, and set the gravity vector, ekfvio_set_gravity -- the rig has to stand still;
        // replenish_grid_x and replenish_grid_y, default 0 0 = off: new landmarks are the strongest free corner of every cell of that grid over
        // the resized frame, emptier cells first, instead of the detector's raster order, ekfvio_set_replenish_grid -- at most 256 cells;
        // nhc_variance, default 0 = off, in (m/s)^2: the nonholonomic constraint of a wheeled vehicle -- no velocity along the vehicle's y and z
        // axes -- as a standing aiding measurement in every frame, ekfvio_set_frame_aid, told at start-up likewise; nhc_R_cv, nine numbers
        // row-major as ONE STRING, vehicle -> camera axes, default a forward-looking camera in its optical frame.  There is no wheel-odometry
        // subscription: measured speed reaches the filter through ekfvio::EKFVIO::aid from the integrator's own callback)
        for (const std::string& name : ekfvio::Params::names()) {
            XmlRpc::XmlRpcValue v;
            if (ros::param::get("~" + name, v)) params_.set(name, to_text(v));
        }
        params_.cfg.replenish = 1;  // addFrame runs replenishFeatures itself (EKFVIO.cpp:154, :172)
        int device = 0;
        ros::param::param<int>("~hip_device", device, 0);
        // rectify_use_p, default false: with rectify = 1 the frames are rectified onto CameraInfo.P (the calibration's rectified camera) instead
        // of the raw camera's K, and odometry, cloud and insight are that camera's (ekfvio_set_camera_model)
        ros::param::param<bool>("~rectify_use_p", rectify_use_p_, false);
        vio_.reset(new ekfvio::EKFVIO(params_, device));
        const auto& p = params_.node;
        cam_sub_ = it_.subscribeCamera(p.at("camera_topic"), 10, &EkfvioNode::cameraCallback, this);
        publish_insight_ = p.at("publish_insight") == "true" || p.at("publish_insight") == "1";
        if (publish_insight_) {
            insight_pub_ = nh_.advertise<sensor_msgs::Image>(p.at("insight_topic"), 1);
            insight_cinfo_pub_ = nh_.advertise<sensor_msgs::CameraInfo>(p.at("insight_camera_info_topic"), 1);
        }
        if (p.at("use_imu") == "true" || p.at("use_imu") == "1")  // "if(USE_IMU)" (EKFVIO.cpp:79-81; default true, Params.h)
            imu_sub_ = nh_.subscribe(p.at("imu_topic"), 1000, &EkfvioNode::imuCallback, this);
        odom_pub_ = nh_.advertise<nav_msgs::Odometry>(p.at("odom_topic"), 1);
        points_pub_ = nh_.advertise<sensor_msgs::PointCloud>(p.at("point_topic"), 1);
        if (params_.publish_ended) ended_pub_ = nh_.advertise<sensor_msgs::PointCloud>(p.at("ended_topic"), 10);
    }

    // EKFVIO.cpp:87-107: wait up to 10 s for base -> camera, else shut down
    bool waitForCameraTransform() {
        const auto& p = params_.node;
        ROS_INFO_STREAM("waiting for the transform from " << p.at("base_frame") << " to " << p.at("camera_frame"));
        if (!tf_listener_.waitForTransform(p.at("base_frame"), p.at("camera_frame"), ros::Time(0), ros::Duration(10))) {
            ROS_FATAL("could not get the base -> camera transform");
            return false;
        }
        try {
            tf::StampedTransform st;
            tf_listener_.lookupTransform(p.at("base_frame"), p.at("camera_frame"), ros::Time(0), st);
            b2c_ = tf::Transform(st);
        } catch (tf::TransformException& e) {
            ROS_WARN_STREAM(e.what());
        }
        return true;
    }

   private:
    // The model and its coefficients travel with every CameraInfo: "plumb_bob" (k1 k2 p1 p2 [k3]: 0, 4 or 5 coefficients), "rational_polynomial"
    // (8) and "equidistant" / "fisheye" (4) map onto ekfvio_set_camera_model's models; with rectify_use_p the rectified camera is CameraInfo.P's
    // fx', cx', fy', cy' (P[0], P[2], P[5], P[6]), else frames are rectified onto K.  The handle is told when any of it changes.  A model that is
    // still unknown (or a count that does not fit its model) is refused loudly and the frames go through as they are.
    void setDistortionFrom(const sensor_msgs::CameraInfo& cam) {
        int model = ekfvio::Params::cameraModelOf(distortion_model_of(cam, 0));
        const size_t n = cam.D.size();
        const bool known = (model == EKFVIO_CAMERA_PLUMB_BOB && (n == 0 || n == 4 || n == 5)) || (model == EKFVIO_CAMERA_RATIONAL && n == 8) ||
                           (model == EKFVIO_CAMERA_EQUIDISTANT && n == 4);
        if (!known)
            ROS_ERROR_THROTTLE(5.0, "rectify: only the plumb_bob model with 4 or 5 coefficients, rational_polynomial with 8 and equidistant with 4 are supported; frames are not rectified");
        if (!known) model = EKFVIO_CAMERA_PLUMB_BOB;
        const std::vector<double> D = known ? cam.D : std::vector<double>();
        std::vector<float> P;
        if (known && rectify_use_p_) {
            if (cam.P[0] > 0.0 && cam.P[5] > 0.0) P = {(float)cam.P[0], (float)cam.P[2], (float)cam.P[5], (float)cam.P[6]};
            else ROS_ERROR_THROTTLE(5.0, "rectify_use_p: CameraInfo.P has no positive focal lengths; frames are rectified onto K");
        }
        if (have_D_ && D == last_D_ && model == last_model_ && P == last_P_) return;
        if (model == EKFVIO_CAMERA_PLUMB_BOB && P.empty()) vio_->tc_ekf.setDistortion(D);
        else vio_->tc_ekf.setCameraModel(model, D, P.empty() ? nullptr : P.data());
        last_D_ = D, last_model_ = model, last_P_ = P;
        have_D_ = true;
    }

    void imuCallback(const sensor_msgs::ImuConstPtr& msg) {
        const ekfvio::Vector3f gyro{(float)msg->angular_velocity.x, (float)msg->angular_velocity.y, (float)msg->angular_velocity.z};
        const ekfvio::Vector3f acc{(float)msg->linear_acceleration.x, (float)msg->linear_acceleration.y,
                                   (float)msg->linear_acceleration.z};
        // EKFVIO.cpp:113-115 (a logging stub there).  With imu_update the record is queued and applied in stamp order in
        // front of the next frame (ekfvio::EKFVIO::imu_callback); nothing it can throw may unwind through ros::spin
        try {
            vio_->imu_callback(msg->header.stamp.toSec(), gyro, acc);
        } catch (const ekfvio::Error& e) {
            ROS_ERROR_STREAM_THROTTLE(1.0, "ekfvio (imu): " << e.what());
        }
    }

    void cameraCallback(const sensor_msgs::ImageConstPtr& img, const sensor_msgs::CameraInfoConstPtr& cam) {
        const ros::WallTime start = ros::WallTime::now();
        ekfvio::Frame f;
        int step = 0;
        if (!to_grey(*img, grey_, f.img, step)) {
            ROS_ERROR_STREAM_THROTTLE(5.0, "unsupported image encoding " << img->encoding);
            return;
        }
        f.cols = (int)img->width;
        f.rows = (int)img->height;
        f.step = step;
        for (int i = 0; i < 9; i++) f.K[i] = (float)cam->K[i];
        f.t = img->header.stamp.toSec();
        try {
            if (params_.rectify) setDistortionFrom(*cam);  // rectify = 1: the topic carries raw frames, the device rectifies them
            if (!vio_->addFrame(f)) ROS_ERROR_THROTTLE(1.0, "innovation covariance not positive definite (NumericalIssue)");
        } catch (const ekfvio::Error& e) {
            ROS_ERROR_STREAM("ekfvio: " << e.what());
            return;
        }
        if (publish_insight_) publishInsight(img->header.stamp);
        publishOdometry(img->header.stamp);
        publishPoints(img->header.stamp);
        if (params_.publish_ended) publishEnded(img->header.stamp, f.t);
        const double ms = (ros::WallTime::now() - start).toSec() * 1e3;
        dt_sum_ += ms;
        ROS_INFO_STREAM("average dt: " << dt_sum_ / ++dt_count_ << " this dt: " << ms);  // EKFVIO.cpp:132-136
    }

    // EKFVIO.cpp:444-477
    void publishOdometry(const ros::Time& stamp) {
        const auto& p = params_.node;
        const ekfvio::Odometry o = vio_->odometry();
        const tf::Transform pose(tf::Quaternion(o.orientation_wxyz[1], o.orientation_wxyz[2], o.orientation_wxyz[3], o.orientation_wxyz[0]),
                                 tf::Vector3(o.position[0], o.position[1], o.position[2]));
        br_.sendTransform(tf::StampedTransform(pose, stamp, p.at("world_frame"), p.at("odom_frame")));
        nav_msgs::Odometry msg;
        msg.header.stamp = stamp;
        msg.header.frame_id = p.at("world_frame");
        msg.child_frame_id = p.at("camera_frame");
        msg.pose.pose.position.x = o.position[0];
        msg.pose.pose.position.y = o.position[1];
        msg.pose.pose.position.z = o.position[2];
        msg.pose.pose.orientation.w = o.orientation_wxyz[0];
        msg.pose.pose.orientation.x = o.orientation_wxyz[1];
        msg.pose.pose.orientation.y = o.orientation_wxyz[2];
        msg.pose.pose.orientation.z = o.orientation_wxyz[3];
        msg.twist.twist.linear.x = o.linear[0];
        msg.twist.twist.linear.y = o.linear[1];
        msg.twist.twist.linear.z = o.linear[2];
        msg.twist.twist.angular.x = o.angular[0];
        msg.twist.twist.angular.y = o.angular[1];
        msg.twist.twist.angular.z = o.angular[2];
        // the reference leaves both covariances zero (:473 "TODO add convariance computation"), and so does publish_covariance = false: the
        // message is then byte for byte what it was.  With it on: pose in the world frame over (x, y, z, rotation about X, Y, Z), twist in the
        // child frame over (linear, angular) -- the frame's own outputs, a memcpy behind addFrame
        if (params_.publish_covariance) {
            const ekfvio::TightlyCoupledEKF::OdometryCovariance c = vio_->tc_ekf.getOdometryCovariance();
            fill_covariance(msg.pose, c.pose, 0);
            fill_covariance(msg.twist, c.twist, 0);
        }
        odom_pub_.publish(msg);
    }

    // EKFVIO.cpp:479-518
    void publishPoints(const ros::Time& stamp) {
        const ekfvio::PointCloud pc = vio_->points();
        sensor_msgs::PointCloud msg;
        msg.header.stamp = stamp;
        msg.header.frame_id = params_.node.at("odom_frame");
        sensor_msgs::ChannelFloat32 ch;
        ch.name = "intensity";
        msg.points.resize(pc.points.size());
        for (size_t i = 0; i < pc.points.size(); i++) {
            msg.points[i].x = pc.points[i][0];
            msg.points[i].y = pc.points[i][1];
            msg.points[i].z = pc.points[i][2];
        }
        ch.values = pc.intensity;
        msg.channels.push_back(ch);
        if (params_.publish_ids) {  // rows of the ids are the rows of the cloud: both arrived with the frame's outputs
            const ekfvio::TightlyCoupledEKF::LandmarkIds li = vio_->tc_ekf.getLandmarkIds();
            sensor_msgs::ChannelFloat32 ids;
            ids.name = "id";
            ids.values.resize(li.id.size());
            for (size_t i = 0; i < li.id.size(); i++) ids.values[i] = id_as_float(li.id[i]);
            msg.channels.push_back(ids);
        }
        points_pub_.publish(msg);
    }

    // a float holds every integer below 2^24 exactly
    static float id_as_float(int64_t id) { return (float)(id % (int64_t(1) << 24)); }

    // The landmarks the frame's removal took out (remove_lost = 1), each with the last estimate the filter had of it: a sparse map point.
    // Nothing is published for a frame in which no track ended.
    void publishEnded(const ros::Time& stamp, double t) {
        const ekfvio::TightlyCoupledEKF::Ended en = vio_->tc_ekf.getEnded();
        if (en.id.empty()) return;
        static const char* const names[12] = {"id", "born", "index_before", "c00", "c01", "c02", "c10", "c11", "c12", "c20", "c21", "c22"};
        sensor_msgs::PointCloud msg;
        msg.header.stamp = stamp;
        msg.header.frame_id = params_.node.at("odom_frame");
        msg.points.resize(en.id.size());
        msg.channels.resize(12);
        for (int c = 0; c < 12; c++) {
            msg.channels[c].name = names[c];
            msg.channels[c].values.resize(en.id.size());
        }
        for (size_t i = 0; i < en.id.size(); i++) {
            msg.points[i].x = en.xyz[i][0];
            msg.points[i].y = en.xyz[i][1];
            msg.points[i].z = en.xyz[i][2];
            msg.channels[0].values[i] = id_as_float(en.id[i]);
            msg.channels[1].values[i] = (float)(t - en.born[i]);  // the track's age in seconds
            msg.channels[2].values[i] = (float)en.index_before[i];
            for (int c = 0; c < 9; c++) msg.channels[3 + c].values[i] = en.cov[i][c];
        }
        ended_pub_.publish(msg);
    }

    // EKFVIO.cpp:379-442: the resized frame as BGR8 with a green square marker at every landmark that is not flagged for
    // deletion, and a CameraInfo with the reference's K / P entries; frame id ODOM_FRAME on both (ekfvio::EKFVIO::insight)
    void publishInsight(const ros::Time& stamp) {
        const ekfvio::Insight in = vio_->insight();
        sensor_msgs::CameraInfo cinfo;
        cinfo.header.frame_id = params_.node.at("odom_frame");
        cinfo.header.stamp = stamp;
        cinfo.height = in.height;
        cinfo.width = in.width;
        for (int i = 0; i < 9; i++) cinfo.K[i] = in.K[i];
        for (int i = 0; i < 12; i++) cinfo.P[i] = in.P[i];
        insight_cinfo_pub_.publish(cinfo);
        sensor_msgs::Image out;
        out.header.frame_id = params_.node.at("odom_frame");
        out.header.stamp = stamp;
        out.width = in.width;
        out.height = in.height;
        out.encoding = sensor_msgs::image_encodings::BGR8;
        out.step = 3 * in.width;
        out.data = in.bgr;
        insight_pub_.publish(out);
    }

    ros::NodeHandle nh_;
    image_transport::ImageTransport it_;
    image_transport::CameraSubscriber cam_sub_;
    ros::Subscriber imu_sub_;
    ros::Publisher insight_pub_, insight_cinfo_pub_, odom_pub_, points_pub_, ended_pub_;
    tf::TransformListener tf_listener_;
    tf::TransformBroadcaster br_;
    tf::Transform b2c_;
    ekfvio::Params params_;
    std::unique_ptr<ekfvio::EKFVIO> vio_;
    std::vector<uint8_t> grey_;
    bool publish_insight_ = false;
    std::vector<double> last_D_;  // the coefficients the handle was told last (rectify = 1)
    bool have_D_ = false;
    int last_model_ = 0;         // ... and the model and the rectified camera that went with them
    std::vector<float> last_P_;
    bool rectify_use_p_ = false;  // ~rectify_use_p: rectify onto CameraInfo.P instead of K
    double dt_sum_ = 0;
    int dt_count_ = 0;
};

}  // namespace

int main(int argc, char** argv) {
    ros::init(argc, argv, "ekfvio_node");
    try {
        EkfvioNode node;
        if (!node.waitForCameraTransform()) {
            ros::shutdown();
            return 1;
        }
        ros::spin();  // single-threaded spinner: callbacks are serialised, as in the reference (EKFVIO.cpp:109)
    } catch (const ekfvio::Error& e) {
        ROS_FATAL_STREAM("ekfvio: " << e.what());
        return 1;
    }
    return 0;
}
#endif  // __has_include(<ros/ros.h>)
