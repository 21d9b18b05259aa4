"""The no-data mask through the C++ host shim (ekf_vio_amd/host/ekfvio.hpp: setMask, getMask, getMaskHits) and the node shim's
mask_rectify_border parameter: compiled C++ against the C-ABI, as tests/test_gpu_host_shim_covout.py does it."""
import json
import subprocess

import pytest

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "ekfvio.hpp"
int main() {
    try {
        const int w = 96, h = 64, stride = 100;
        std::vector<uint8_t> img((size_t)w * h), mask((size_t)stride * h, 0);  // (the slack of every mask row is zero: it must not be read)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                img[(size_t)y * w + x] = (uint8_t)((x * 7 + y * 13) & 255);
                mask[(size_t)y * stride + x] = (x >= 40 && x < 50 && y >= 20 && y < 30) ? 0 : 255;
            }
        const float K[9] = {100.f, 0, 48.f, 0, 100.f, 32.f, 0, 0, 1.f};
        ekfvio::TightlyCoupledEKF ekf(8, 0);
        if (ekf.getMask().width != 0 || !ekf.getMask().blocked.empty() || !ekf.getMaskHits().masked.empty()) return 2;
        ekf.setMask(mask.data(), w, h, stride, 0);
        if (ekfvio_klt_push_frame(ekf.handle(), img.data(), w, h, w, K) != EKFVIO_OK) return 3;
        const ekfvio::TightlyCoupledEKF::Mask m = ekf.getMask();
        std::vector<uint8_t> want((size_t)w * h, 7);
        if (ekfvio_mask_blocked(K, nullptr, 0, mask.data(), w, h, stride, 1, 11, 0, want.data()) != EKFVIO_OK) return 4;
        if (m.width != w || m.height != h || m.blocked.size() != want.size() || std::memcmp(m.blocked.data(), want.data(), want.size())) return 5;
        if (!m.blocked[(size_t)25 * w + 45] || !m.blocked[(size_t)25 * w + 35] || m.blocked[(size_t)32 * w + 70] || !m.blocked[0]) return 6;
        // a frame of another size is refused while the mask is set
        if (ekfvio_klt_push_frame(ekf.handle(), img.data(), w - 8, h, w, K) != EKFVIO_EINVAL) return 7;
        ekf.setMask(nullptr, 0, 0, 0, EKFVIO_MASK_RECTIFY_BORDER);  // the flag alone: nothing to mask without distortion, any size is taken
        if (ekfvio_klt_push_frame(ekf.handle(), img.data(), w - 8, h, w, K) != EKFVIO_OK || ekf.getMask().width != w - 8) return 8;
        ekf.setMask(nullptr, 0, 0, 0, 0);
        if (ekfvio_klt_push_frame(ekf.handle(), img.data(), w, h, w, K) != EKFVIO_OK || ekf.getMask().width != 0) return 9;
        try {
            ekf.setMask(mask.data(), w, h, w - 1, 0);
            return 10;
        } catch (const ekfvio::Error& e) {
            if (e.code != EKFVIO_EINVAL) return 11;
        }
        ekfvio::Params p;
        if (p.mask_rectify_border != 0) return 12;
        p.set("mask_rectify_border", "true");
        p.set("num_features", "8");
        if (p.mask_rectify_border != 1) return 13;
        ekfvio::EKFVIO vio(p);  // the parameter is applied where rectify is applied: behind ekfvio_create
        std::printf("wrapper equals ekfvio_mask_blocked: %d bytes\n", (int)want.size());
        return 0;
    } catch (const ekfvio::Error& e) {
        std::fprintf(stderr, "ekfvio error %d: %s\n", e.code, e.what());
        return 1;
    }
}
"""


@pytest.mark.gpu
def test_cpp_wrapper_sets_and_returns_the_mask(tmp_path):
    from ekf_vio_amd import _build
    _build.build()
    src, exe = tmp_path / "mask.cpp", tmp_path / "mask"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", _build.HOST_DIR, "-o", str(exe), str(src), "-L" + _build.LIB_DIR,
                           "-lekfvio_hip", "-Wl,-rpath," + _build.LIB_DIR, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    assert "wrapper equals ekfvio_mask_blocked" in out.stdout


def test_mask_rectify_border_is_a_node_parameter(tmp_path):
    """--print-config (no GPU work) reports the parameter: default false, true from a parameter file; the node source reads every name."""
    from ekf_vio_amd import _build
    _build.build()
    exe = _build.build_host()
    d = json.loads(subprocess.run([exe, "--print-config"], capture_output=True, text=True, timeout=120, check=True).stdout)
    assert d["mask_rectify_border"] == 0
    f = tmp_path / "params.yaml"
    f.write_text("mask_rectify_border: true\nrectify: 1\n")
    d = json.loads(subprocess.run([exe, "--print-config", str(f)], capture_output=True, text=True, timeout=120, check=True).stdout)
    assert d["mask_rectify_border"] == 1 and d["rectify"] == 1
