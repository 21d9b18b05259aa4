// stand-in: see tests/ros_stubs/README.md.  This one goes IN FRONT of tests/ros_stubs on the include path
// (tests/test_gpu_host_shim_covout.py): nav_msgs/Odometry with the two covariance arrays of geometry_msgs/PoseWithCovariance and
// TwistWithCovariance (row-major 6x6 float64, boost::array<double, 36> in ROS Noetic), so that the node's publish_covariance branch is
// type-checked against a message that carries them.
#pragma once
#include <array>

#include <sensor_msgs/Imu.h>
namespace nav_msgs {
struct Odometry {
    std_msgs::Header header;
    std::string child_frame_id;
    struct {
        struct { geometry_msgs::Point position; geometry_msgs::Quaternion orientation; } pose;
        std::array<double, 36> covariance;
    } pose;
    struct {
        struct { geometry_msgs::Vector3 linear, angular; } twist;
        std::array<double, 36> covariance;
    } twist;
};
}  // namespace nav_msgs
