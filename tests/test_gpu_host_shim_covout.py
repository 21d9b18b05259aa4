"""The covariances of the published outputs through the C++ host shim (ekf_vio_amd/host/ekfvio.hpp), the replay driver's --covariance
switch and the node shim's publish_covariance parameter: compiled C++ against the C-ABI, as tests/test_gpu_host_shim.py does it."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "ekfvio.hpp"
int main() {
    try {
        ekfvio::TightlyCoupledEKF ekf(8, 0);
        ekf.addNewFeatures({{0.1f, -0.2f}, {0.3f, 0.25f}, {-0.4f, 0.05f}});
        ekf.process(0.05f);
        std::vector<ekfvio::Vector2f> z = {{0.11f, -0.19f}, {0.29f, 0.26f}, {-0.41f, 0.04f}};
        std::vector<ekfvio::Matrix2f> R(3, ekfvio::Matrix2f{1e-5f, 0, 0, 1e-5f});
        ekf.updateWithFeaturePositions(z, R, std::vector<uint8_t>(3, 1));
        const auto oc = ekf.getOdometryCovariance();
        const auto pc = ekf.getPointsCovariance();
        float pose[36], twist[36], cov[27];
        if (ekfvio_get_odometry_covariance(ekf.handle(), pose, twist) != EKFVIO_OK || ekfvio_get_points_covariance(ekf.handle(), cov) != EKFVIO_OK) return 3;
        if (pc.size() != 3 || std::memcmp(oc.pose.data(), pose, sizeof pose) || std::memcmp(oc.twist.data(), twist, sizeof twist) ||
            std::memcmp(pc[0].data(), cov, sizeof cov))
            return 4;
        bool any = false;
        for (int i = 0; i < 36; i++) any = any || pose[i] != 0.f;
        if (!any || !(cov[8] > 0.f)) return 5;
        ekf.setOutputCovariance(true);
        ekf.setOutputCovariance(false);
        std::printf("wrapper equals the C getters: 72 + 27 floats\n");
        return 0;
    } catch (const ekfvio::Error& e) {
        std::fprintf(stderr, "ekfvio error %d: %s\n", e.code, e.what());
        return 1;
    }
}
"""


@pytest.mark.gpu
def test_cpp_wrapper_returns_the_c_getters_bytes(tmp_path):
    from ekf_vio_amd import _build
    _build.build()
    src, exe = tmp_path / "covout.cpp", tmp_path / "covout"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", _build.HOST_DIR, "-o", str(exe), str(src), "-L" + _build.LIB_DIR,
                           "-lekfvio_hip", "-Wl,-rpath," + _build.LIB_DIR, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    assert "wrapper equals the C getters" in out.stdout


@pytest.mark.gpu
def test_replay_covariance_switch_prints_the_python_nodes_diagonals(tmp_path):
    """ekfvio_replay --records ... --covariance: one `cov` line per frame with the two diagonals (%.9g: exact for fp32), equal to the Python
    mirror's on the same records with output_covariance on; the odometry records are unchanged by the switch."""
    from PIL import Image
    from ekf_vio_amd import EKFVIO, _build
    from ekf_vio_amd.sim import translated_sequence
    _build.build()
    exe = _build.build_host()
    base = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "images", "640_480_test_gray.png")))
    imgs = translated_sequence(base, 4)
    K = [500.0, 0.0, 320.0, 0.0, 500.0, 240.0, 0.0, 0.0, 1.0]
    lines = []
    for i, im in enumerate(imgs):
        name = "frame_%03d.pgm" % i
        with open(tmp_path / name, "wb") as fh:
            fh.write(b"P5\n640 480\n255\n" + im.tobytes())
        lines.append("image %.9f %s %s" % (100.0 + i / 30.0, name, " ".join("%.9g" % k for k in K)))
    (tmp_path / "records.txt").write_text("\n".join(lines) + "\n")
    (tmp_path / "params.yaml").write_text("num_features: 48\ninverse_image_scale: 1\n")
    cmd = [exe, "--records", str(tmp_path), "--params", str(tmp_path / "params.yaml")]
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "cov " not in plain.stdout, plain.stdout + plain.stderr
    odom_plain = (tmp_path / "odom.txt").read_text()
    out = subprocess.run(cmd + ["--covariance"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert (tmp_path / "odom.txt").read_text() == odom_plain
    cov = np.array([[float(x) for x in ln.split()[2:]] for ln in out.stdout.splitlines() if ln.startswith("cov ")], np.float32)
    assert cov.shape == (4, 12)
    v = EKFVIO(max_features=48, replenish=1, inverse_image_scale=1, output_covariance=True)
    for i, im in enumerate(imgs):
        v.addFrame(float("%.9f" % (100.0 + i / 30.0)), im, np.array(K, np.float32))
        pose, twist = v.odometry_covariance()
        assert np.array_equal(cov[i], np.concatenate([np.diag(pose), np.diag(twist)])), i
    assert cov[-1, 3:6].min() > 0  # an updated attitude has a variance
    v.tc_ekf.close()


def test_node_shim_type_checks_with_publish_covariance():
    """No GPU, no ROS: the node source against the declaration-only stand-ins, once with the nav_msgs/Odometry that carries the two
    covariance arrays in front of them (-DEKFVIO_NODE_REQUIRE_COVARIANCE: the filling overload must be the one that applies) and once
    against the older stand-in, which has none: that must still compile (the message is then what it was), and must NOT compile with the
    define, which shows that the define bites."""
    src = os.path.join(ROOT, "ekf_vio_amd", "host", "ros", "ekfvio_node.cpp")
    base = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror"]
    old, new = os.path.join(ROOT, "tests", "ros_stubs"), os.path.join(ROOT, "tests", "ros_stubs_covout")
    out = subprocess.run(base + ["-DEKFVIO_NODE_REQUIRE_COVARIANCE", "-I", new, "-I", old, src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    out = subprocess.run(base + ["-I", old, src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    out = subprocess.run(base + ["-DEKFVIO_NODE_REQUIRE_COVARIANCE", "-I", old, src], capture_output=True, text=True)
    assert out.returncode != 0 and "covariance" in out.stderr
    text = open(src).read()
    for needle in ("publish_covariance", "getOdometryCovariance", "fill_covariance(msg.pose", "fill_covariance(msg.twist"):
        assert needle in text, needle
    assert "no covariance, as in the reference" not in text


def test_publish_covariance_is_a_node_parameter(tmp_path):
    """--print-config (no GPU work) reports the parameter: default false, true from a parameter file."""
    import json
    from ekf_vio_amd import _build
    _build.build()
    exe = _build.build_host()
    d = json.loads(subprocess.run([exe, "--print-config"], capture_output=True, text=True, timeout=120, check=True).stdout)
    assert d["publish_covariance"] == 0
    f = tmp_path / "params.yaml"
    f.write_text("publish_covariance: true\n")
    d = json.loads(subprocess.run([exe, "--print-config", str(f)], capture_output=True, text=True, timeout=120, check=True).stdout)
    assert d["publish_covariance"] == 1
