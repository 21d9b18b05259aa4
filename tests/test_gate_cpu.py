"""The innovation gate's interface (ekfvio_set_gate, ekfvio_get_gate) without a GPU: declared with the documented signatures, exported,
bound, null handles refused, and known to the C++ shim's parameter block.  What the gate computes is checked on the device
(tests/test_gpu_gate.py)."""
import ctypes as C
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ekfvio.h")).read()


def _decl(name):
    m = re.search(r"EKFVIO_API\s+int\s+%s\s*\(([^;]*?)\)\s*;" % name, HEADER, re.S)
    assert m, name + " is not declared in include/ekfvio.h"
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_entry_points_are_declared_with_the_documented_signatures():
    assert _decl("ekfvio_set_gate") == ["ekfvio_filter* f", "float chi2"]
    assert _decl("ekfvio_get_gate") == ["ekfvio_filter* f", "float* d2", "uint8_t* gated", "int32_t* n_landmarks", "int32_t* gated_last",
                                        "int64_t* gated_total"]
    # the association order is part of the interface: the device test restates these lines in float32
    for line in ("y0 = z[2i]   - mu[s]", "a  = P(s,s)     + R_i(0,0)", "b  = P(s+1,s)   + R_i(1,0)", "c  = P(s+1,s+1) + R_i(1,1)",
                 "det = a*c - b*b", "q   = ((c*y0)*y0 - ((2*b)*y0)*y1) + (a*y1)*y1", "d2  = q / det",
                 "accept  <=>  det > 0  and  d2 <= chi2"):
        assert line in HEADER, line


def test_entry_points_are_exported_and_bound():
    from ekf_vio_amd import _build, capi
    assert "ekfvio_set_gate" in capi.SYMBOLS and "ekfvio_get_gate" in capi.SYMBOLS
    lib = capi.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _build.LIB_PATH]).decode()
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"ekfvio_set_gate", "ekfvio_get_gate"} <= exported
    vp, fp, u8p, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    assert lib.ekfvio_set_gate.argtypes == [vp, C.c_float]
    assert lib.ekfvio_get_gate.argtypes == [vp, fp, u8p, ip, ip, C.POINTER(C.c_int64)]


def test_null_handle_is_rejected():
    from ekf_vio_amd import capi
    lib = capi.load()
    assert lib.ekfvio_set_gate(None, 1.0) == capi.EINVAL
    n, last, total = C.c_int32(7), C.c_int32(7), C.c_int64(7)
    assert lib.ekfvio_get_gate(None, None, None, C.byref(n), C.byref(last), C.byref(total)) == capi.EINVAL
    assert (n.value, last.value, total.value) == (7, 7, 7)  # nothing written through a refused call
    assert lib.ekfvio_get_gate(None, None, None, None, None, None) == capi.EINVAL


def test_python_mirror_has_the_gate():
    from ekf_vio_amd import EKFVIO, TightlyCoupledEKF
    import inspect
    assert callable(TightlyCoupledEKF.setGate) and callable(TightlyCoupledEKF.gate)
    assert "gate_chi2" in inspect.signature(TightlyCoupledEKF.__init__).parameters  # EKFVIO(gate_chi2=...) hands it through
    assert EKFVIO.__init__ is not None


def test_shim_knows_gate_chi2(tmp_path):
    src = open(os.path.join(ROOT, "ekf_vio_amd", "host", "ekfvio.hpp")).read()
    assert '"gate_chi2"' in src and "ekfvio_set_gate" in src and "setGate" in src
    from ekf_vio_amd import _build
    _build.build()
    exe = _build.build_host()
    f = tmp_path / "params.yaml"
    f.write_text("gate_chi2: 0.25\nnum_features: 50\n")
    out = subprocess.run([exe, "--print-config", str(f)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    d = json.loads(out.stdout)
    assert d["gate_chi2"] == 0.25 and d["max_features"] == 50
    out = subprocess.run([exe, "--print-config"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and json.loads(out.stdout)["gate_chi2"] == 0  # off by default
    f.write_text("gate_chi2: -1\n")
    out = subprocess.run([exe, "--print-config", str(f)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "error" in out.stderr
