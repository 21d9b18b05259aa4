"""Equalisation through the C++ host shim (ekf_vio_amd/host/ekfvio.hpp: setEqualize) and the node shim's equalize_clip_limit /
equalize_tiles_x / equalize_tiles_y parameters: compiled C++ against the C-ABI, as tests/test_gpu_host_shim_mask.py does it.  The C++
program writes the level 0 it gets; it must be the Python handle's, and the host function's."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "ekfvio.hpp"
int main(int argc, char** argv) {
    if (argc < 3) return 20;
    try {
        const int w = 96, h = 64;
        std::vector<uint8_t> img((size_t)w * h), want((size_t)w * h, 7), got((size_t)w * h, 9);
        FILE* in = std::fopen(argv[1], "rb");
        if (!in || std::fread(img.data(), 1, img.size(), in) != img.size()) return 21;
        std::fclose(in);
        const float K[9] = {100.f, 0, 48.f, 0, 100.f, 32.f, 0, 0, 1.f};
        ekfvio::TightlyCoupledEKF ekf(8, 0);
        ekf.setEqualize(3.0f, 4, 4);
        if (ekfvio_klt_push_frame(ekf.handle(), img.data(), w, h, w, K) != EKFVIO_OK) return 3;
        int32_t lw = 0, lh = 0;
        if (ekfvio_klt_get_level(ekf.handle(), 0, &lw, &lh, got.data(), nullptr) != EKFVIO_OK || lw != w || lh != h) return 4;
        if (ekfvio_equalize(img.data(), w, h, w, 3.0f, 4, 4, want.data()) != EKFVIO_OK) return 5;
        if (std::memcmp(got.data(), want.data(), want.size()) != 0) return 6;
        if (std::memcmp(got.data(), img.data(), img.size()) == 0) return 7;
        FILE* out = std::fopen(argv[2], "wb");
        if (!out || std::fwrite(got.data(), 1, got.size(), out) != got.size()) return 22;
        std::fclose(out);
        // a frame with fewer columns than tiles is refused while the setting is on
        if (ekfvio_klt_push_frame(ekf.handle(), img.data(), 3, h, w, K) != EKFVIO_EINVAL) return 8;
        ekf.setEqualize(0.f);  // off: the raw frame
        if (ekfvio_klt_push_frame(ekf.handle(), img.data(), w, h, w, K) != EKFVIO_OK) return 9;
        if (ekfvio_klt_get_level(ekf.handle(), 0, &lw, &lh, got.data(), nullptr) != EKFVIO_OK || std::memcmp(got.data(), img.data(), img.size()) != 0) return 10;
        try {
            ekf.setEqualize(3.0f, 17, 4);
            return 11;
        } catch (const ekfvio::Error& e) {
            if (e.code != EKFVIO_EINVAL) return 12;
        }
        ekfvio::Params p;
        if (p.equalize_clip_limit != 0.f || p.equalize_tiles_x != 8 || p.equalize_tiles_y != 8) return 13;
        p.set("equalize_clip_limit", "2.5");
        p.set("equalize_tiles_x", "4");
        p.set("~equalize_tiles_y", "6");
        p.set("num_features", "8");
        if (p.equalize_clip_limit != 2.5f || p.equalize_tiles_x != 4 || p.equalize_tiles_y != 6) return 14;
        for (const char* bad : {"0", "17", "2.5"}) {
            try {
                ekfvio::Params q;
                q.set("equalize_tiles_x", bad);
                return 15;
            } catch (const ekfvio::Error& e) {
                if (e.code != EKFVIO_EINVAL) return 16;
            }
        }
        try {
            ekfvio::Params q;
            q.set("equalize_clip_limit", "-1");
            return 17;
        } catch (const ekfvio::Error& e) {
            if (e.code != EKFVIO_EINVAL) return 18;
        }
        p.cfg.inverse_image_scale = 1;
        ekfvio::EKFVIO vio(p);  // the parameters are applied where rectify is applied: behind ekfvio_create
        if (ekfvio_klt_push_frame(vio.tc_ekf.handle(), img.data(), w, h, w, K) != EKFVIO_OK) return 19;
        if (ekfvio_klt_get_level(vio.tc_ekf.handle(), 0, &lw, &lh, got.data(), nullptr) != EKFVIO_OK) return 23;
        if (ekfvio_equalize(img.data(), w, h, w, 2.5f, 4, 6, want.data()) != EKFVIO_OK || std::memcmp(got.data(), want.data(), want.size()) != 0) return 24;
        std::printf("wrapper equals ekfvio_equalize: %d bytes\n", (int)want.size());
        return 0;
    } catch (const ekfvio::Error& e) {
        std::fprintf(stderr, "ekfvio error %d: %s\n", e.code, e.what());
        return 1;
    }
}
"""


@pytest.mark.gpu
def test_cpp_wrapper_gives_the_python_handles_level0(tmp_path):
    from ekf_vio_amd import KLTTracker, TightlyCoupledEKF, _build
    import _equalize as eq
    _build.build()
    img = np.ascontiguousarray(eq.crop(200, 150, 96, 64))
    (tmp_path / "in.bin").write_bytes(img.tobytes())
    src, exe = tmp_path / "equalize.cpp", tmp_path / "equalize"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", _build.HOST_DIR, "-o", str(exe), str(src), "-L" + _build.LIB_DIR,
                           "-lekfvio_hip", "-Wl,-rpath," + _build.LIB_DIR, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    assert "wrapper equals ekfvio_equalize" in out.stdout
    cpp = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.uint8).reshape(64, 96)
    g = TightlyCoupledEKF(max_features=8, equalize=(3.0, 4, 4))
    t = KLTTracker(g)
    t.push_frame(img, np.array([100.0, 0, 48.0, 0, 100.0, 32.0, 0, 0, 1.0], np.float32))
    py = t.level(0)[0]
    g.close()
    assert np.array_equal(cpp, py) and np.array_equal(py, eq.restate(img, 3.0, 4, 4))


def test_node_shim_type_checks_with_the_equalize_parameters():
    """No GPU, no ROS: the node source against the declaration-only stand-ins; the node asks the parameter server for every name of
    Params::names(), which now holds the three."""
    src = os.path.join(ROOT, "ekf_vio_amd", "host", "ros", "ekfvio_node.cpp")
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "ros_stubs"), src],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "ekfvio::Params::names()" in open(src).read()
    hpp = open(os.path.join(ROOT, "ekf_vio_amd", "host", "ekfvio.hpp")).read()
    names = hpp[hpp.index("static std::vector<std::string> names()"):]
    names = names[:names.index("};")]
    for n in ("equalize_clip_limit", "equalize_tiles_x", "equalize_tiles_y"):
        assert '"%s"' % n in names, n


def test_equalize_parameters_are_node_parameters(tmp_path):
    """--print-config (no GPU work) reports the parameters: off and 8 x 8 by default, the values of a parameter file; a bad one is refused."""
    from ekf_vio_amd import _build
    _build.build()
    exe = _build.build_host()
    d = json.loads(subprocess.run([exe, "--print-config"], capture_output=True, text=True, timeout=120, check=True).stdout)
    assert (d["equalize_clip_limit"], d["equalize_tiles_x"], d["equalize_tiles_y"]) == (0, 8, 8)
    f = tmp_path / "params.yaml"
    f.write_text("equalize_clip_limit: 3.0\nequalize_tiles_x: 6\nequalize_tiles_y: 4\n")
    d = json.loads(subprocess.run([exe, "--print-config", str(f)], capture_output=True, text=True, timeout=120, check=True).stdout)
    assert (d["equalize_clip_limit"], d["equalize_tiles_x"], d["equalize_tiles_y"]) == (3.0, 6, 4)
    f.write_text("equalize_tiles_x: 17\n")
    assert subprocess.run([exe, "--print-config", str(f)], capture_output=True, text=True, timeout=120).returncode != 0
