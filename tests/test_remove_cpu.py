"""CPU-side checks of landmark removal's boundary: ekfvio_remove_features is declared, exported and bound, and the configuration's
new field comes last and defaults to the reference's behaviour (lost landmarks stay in the state)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_remove_features_is_declared_exported_and_bound():
    from ekf_vio_amd import capi
    hdr = open(os.path.join(ROOT, "include", "ekfvio.h")).read()
    assert re.search(r"^EKFVIO_API int ekfvio_remove_features\(ekfvio_filter\* f, const uint8_t\* remove, int32_t count, int32_t\* removed\);",
                     hdr, re.M)
    assert "ekfvio_remove_features" in capi.SYMBOLS
    lib = capi.load()
    assert lib.ekfvio_remove_features.argtypes is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()]).decode()
    assert "ekfvio_remove_features" in {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert lib.ekfvio_remove_features(None, None, 0, None) == capi.EINVAL


def test_config_remove_lost_is_last_and_off_by_default():
    from ekf_vio_amd import capi
    assert capi.Config._fields_[-1] == ("remove_lost", C.c_int32)
    hdr = open(os.path.join(ROOT, "include", "ekfvio.h")).read()
    body = hdr[hdr.index("typedef struct ekfvio_config"):hdr.index("} ekfvio_config;")]
    fields = re.findall(r"^\s*(?:int32_t|float)\s+(\w+)", body, re.M)
    assert fields[-1] == "remove_lost" and [f[0] for f in capi.Config._fields_] == fields
    cfg = capi.Config()
    cfg.remove_lost = 7
    assert capi.load().ekfvio_default_config(C.byref(cfg)) == capi.OK
    assert cfg.remove_lost == 0


def test_host_shim_knows_the_remove_lost_key():
    src = open(os.path.join(ROOT, "ekf_vio_amd", "host", "ekfvio.hpp")).read()
    assert '"remove_lost"' in src and "cfg.remove_lost" in src and "removeFeatures" in src
