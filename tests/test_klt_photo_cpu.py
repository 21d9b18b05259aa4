"""The tracker's gain/offset term (include/ekfvio.h, ekfvio_set_klt_photometric), the part that needs no GPU.  tests/_klt_photo.py
restates one Lucas-Kanade pass in NumPy: without the term it is held to the CPU oracle's tracker, bit for bit, so that with the term it
can be what the device is held to (tests/test_gpu_klt_photo.py).  ekfvio_klt_project_gradients is a host function that compiles the
inline functions the kernel compiles (csrc/klt_photo.h): the device's projection arithmetic is held to the restatement here.  And what
the term is for -- tracks that survive an exposure change -- is measured with the restatement against the oracle's tracker."""
import ctypes as C
import functools
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

from ekf_vio_amd import EkfvioError, capi, klt_project_gradients
from oracle import KltFrame, klt_track, replenish

import _equalize as eq
import _klt_fb as fb
import _klt_photo as kp

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ekfvio.h")).read()
EMPTY = np.zeros((0, 2), F32)
OTHER_POINTS = np.vstack([fb.grid_points(10), [[5.0, 5.0], [-40.0, 100.0], [639.0, 479.0], [320.5, 0.25], [2.0, 470.0]]]).astype(F32)


# ---- the restatement without the term is the oracle's tracker ---------------------------------------------------------------------

def test_restatement_without_the_term_has_the_oracles_bits():
    """Every point of test_gpu_klt.py::test_tracked_points_bit_exact_and_flow's set (219: two grids, the border and out-of-image
    points) on the moved pair: positions and status."""
    pts = fb.all_points()
    assert len(pts) == 219
    A, B = fb.frame("first"), fb.frame("moved")
    on, os_, _ = klt_track(A, B, pts, pts.copy())
    rn, rs = kp.track(kp.Pyramid(A), kp.Pyramid(B), pts, pts.copy(), photo=False)
    assert np.array_equal(rs, os_)
    assert np.array_equal(rn, on), float(np.abs(rn - on).max())
    assert os_.sum() >= 200 and (os_ == 0).sum() >= 3  # both roads are taken


@pytest.mark.parametrize("win,levels,iters", [(3, 3, 30), (7, 3, 30), (21, 0, 3)])
def test_restatement_without_the_term_other_windows(win, levels, iters):
    """Windows 3, 7 and 21 of test_gpu_klt.py::test_other_windows_levels_and_iteration_budgets_bit_exact, its points and its guess."""
    guess = (OTHER_POINTS + np.array([-20.0, -6.0], F32)).astype(F32)
    A, B = fb.frame("first", win, levels), fb.frame("moved", win, levels)
    on, os_, _ = klt_track(A, B, OTHER_POINTS, guess.copy(), win=win, max_iter=iters)
    rn, rs = kp.track(kp.Pyramid(A), kp.Pyramid(B), OTHER_POINTS, guess, photo=False, win=win, max_iter=iters)
    assert np.array_equal(rs, os_)
    assert np.array_equal(rn, on), float(np.abs(rn - on).max())


# ---- the host function against the restatement's projection -----------------------------------------------------------------------

def _real_windows():
    P = kp.Pyramid(fb.frame("first"))
    out = {}
    for i, p in enumerate(fb.grid_points(8)[[0, 9, 27, 36, 63]]):
        for level in (0, 3):
            out["real_%d_l%d" % (i, level)] = kp.template_at(P, level, p + F32(0.37))
    out["real_border"] = kp.template_at(P, 0, (2.0, 470.0))  # zero derivatives and mirrored pixels in the window
    out["real_win7"] = kp.template_at(P, 1, (320.25, 240.5), win=7)
    return out


def _spike():
    """A one-pixel spike template: the regression on Iv fits the spike pixel alone, so the other 440 keep their deviation from THEIR
    mean -- one of them at +4080 among -4080s ends near 8141 and is clamped."""
    iv = np.zeros(441, np.int64)
    iv[220] = 8160
    ix = np.full(441, -4080, np.int64)
    ix[5] = 4080
    iy = np.full(441, 4080, np.int64)
    iy[17] = -4080
    return iv, ix, iy


def _cases():
    rng = np.random.RandomState(11)
    c = _real_windows()
    c["constant"] = (np.full(441, 3744, np.int64), rng.randint(-4080, 4081, 441), rng.randint(-4080, 4081, 441))  # VI == 0
    c["spike"] = _spike()
    for n in (1, 9, 441):
        c["count_%d" % n] = (rng.randint(0, 8161, n), rng.randint(-4080, 4081, n), rng.randint(-4080, 4081, n))
    c["extremes"] = (np.where(np.arange(441) % 2, 8160, 0), np.where(np.arange(441) % 3, 4080, -4080), np.where(np.arange(441) % 5, -4080, 4080))
    return c


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_projection_has_the_bits_of_the_restatement(name):
    iv, ix, iy = CASES[name]
    rx, ry, info = kp.project(iv, ix, iy)
    if name == "constant":
        assert info["VI"] == 0
    if name == "spike":
        assert info["clamped"] >= 2 and rx.reshape(-1)[5] == 4080 and ry.reshape(-1)[17] == -4080
    if name.startswith("real"):
        assert info["VI"] > 0 and info["clamped"] == 0
    gx, gy = klt_project_gradients(iv, ix, iy)
    assert gx.dtype == np.int32 and gx.shape == np.asarray(iv).shape
    assert np.array_equal(gx, rx) and np.array_equal(gy, ry)
    assert np.abs(gx).max() <= 4080 and np.abs(gy).max() <= 4080


def test_constant_template_gets_the_mean_removed():
    iv, ix, iy = CASES["constant"]
    gx, gy = klt_project_gradients(iv, ix, iy)
    mX = F32(np.float64(int(np.sum(ix)))) / F32(441.0)
    assert np.array_equal(gx, np.clip(np.rint(np.asarray(ix).astype(F32) - mX), -4080, 4080).astype(np.int32))
    assert abs(int(gx.sum())) <= 441  # (each value rounds by at most a half)


def test_projected_gradients_are_blind_to_gain_and_offset():
    """What the term is for.  The exact projection is orthogonal to 1 and to Iv; Ix' differs from it by e, |e| <= 0.5 from rint plus the
    fp32 rounding of three operations on values below 2^14 (< 0.01).  So |sum Ix'| <= 0.51 n and |sum (Iv - mean Iv) Ix'| <= 0.51 sum |Iv -
    mean Iv|: a gain and an offset on the second image add alpha Iv + beta to diff and next to nothing to b.  That the check is not empty:
    the raw gradients of this textured window exceed the bound."""
    iv, ix, iy = (np.asarray(a, np.float64).reshape(-1) for a in CASES["real_2_l0"])
    gx, gy = (g.astype(np.float64).reshape(-1) for g in klt_project_gradients(*CASES["real_2_l0"]))
    dev = iv - iv.mean()
    bound = 0.51 * np.abs(dev).sum()
    for g in (gx, gy):
        assert abs(g.sum()) <= 0.51 * iv.size
        assert abs((dev * g).sum()) <= bound
    print("sum dev*Ix", (dev * ix).sum(), "sum dev*Iy", (dev * iy).sum(), "bound", bound)
    assert max(abs((dev * ix).sum()), abs((dev * iy).sum())) > bound


def test_arguments():
    lib = capi.load()
    ip = C.POINTER(C.c_int32)
    a = np.arange(441, dtype=np.int32)
    ox, oy = np.full(441, 7, np.int32), np.full(441, 7, np.int32)
    p = lambda x: x.ctypes.data_as(ip)
    assert lib.ekfvio_klt_project_gradients(p(a), p(a), p(a), 441, p(ox), p(oy)) == capi.OK
    ox[:], oy[:] = 7, 7
    for args in ((None, p(a), p(a), 441, p(ox), p(oy)), (p(a), None, p(a), 441, p(ox), p(oy)), (p(a), p(a), None, 441, p(ox), p(oy)),
                 (p(a), p(a), p(a), 441, None, p(oy)), (p(a), p(a), p(a), 441, p(ox), None), (p(a), p(a), p(a), 0, p(ox), p(oy)),
                 (p(a), p(a), p(a), -1, p(ox), p(oy)), (p(a), p(a), p(a), 442, p(ox), p(oy))):
        assert lib.ekfvio_klt_project_gradients(*args) == capi.EINVAL
    assert (ox == 7).all() and (oy == 7).all()  # nothing written through a refused call
    with pytest.raises(EkfvioError) as e:
        klt_project_gradients(np.zeros(442), np.zeros(442), np.zeros(442))
    assert e.value.code == capi.EINVAL
    with pytest.raises(EkfvioError):
        klt_project_gradients(np.zeros(4), np.zeros(5), np.zeros(4))
    # an output may be its own input
    iv, ix, iy = (np.ascontiguousarray(v, np.int32) for v in CASES["real_0_l0"])
    want = klt_project_gradients(iv, ix, iy)
    assert lib.ekfvio_klt_project_gradients(p(iv), p(ix), p(iy), iv.size, p(ix), p(iy)) == capi.OK
    assert np.array_equal(ix, want[0]) and np.array_equal(iy, want[1])


# ---- the interface ----------------------------------------------------------------------------------------------------------------

def _decl(name):
    m = re.search(r"EKFVIO_API\s+int\s+%s\s*\(([^;]*?)\)\s*;" % name, HEADER, re.S)
    assert m, name + " is not declared in include/ekfvio.h"
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_entry_points_are_declared_with_the_documented_signatures():
    assert _decl("ekfvio_set_klt_photometric") == ["ekfvio_filter* f", "int32_t on"]
    assert _decl("ekfvio_klt_project_gradients") == ["const int32_t* Iv", "const int32_t* Ix", "const int32_t* Iy", "int32_t count",
                                                     "int32_t* Ix_out", "int32_t* Iy_out"]
    # the lines are part of the interface: the restatement and the kernel follow them
    for line in ("sI = sum Iv   sX = sum Ix   sY = sum Iy   sII = sum Iv*Iv   sIX = sum Iv*Ix   sIY = sum Iv*Iy",
                 "VI = n*sII - sI*sI      CX = n*sIX - sI*sX      CY = n*sIY - sI*sY",
                 "mI = (float)sI / (float)n     mX = (float)sX / (float)n     mY = (float)sY / (float)n",
                 "cx = VI > 0 ? (float)CX / (float)VI : 0.0f",
                 "Ix'[t] = clamp((int)rint(((float)Ix[t] - mX) - cx * ((float)Iv[t] - mI)), -4080, 4080)",
                 "Iy'[t] likewise with mY, cy", "SSD weights remain brightness-dependent", "survives ekfvio_reset"):
        assert line in HEADER, line
    assert "klt_photo" not in re.search(r"typedef struct ekfvio_config \{.*?\} ekfvio_config;", HEADER, re.S).group(0)  # no field of the configuration


def test_entry_points_are_exported_and_bound():
    from ekf_vio_amd import _build
    names = {"ekfvio_set_klt_photometric", "ekfvio_klt_project_gradients"}
    assert names <= set(capi.SYMBOLS)
    lib = capi.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _build.LIB_PATH]).decode()
    assert names <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    ip = C.POINTER(C.c_int32)
    assert lib.ekfvio_set_klt_photometric.argtypes == [C.c_void_p, C.c_int32]
    assert lib.ekfvio_klt_project_gradients.argtypes == [ip, ip, ip, C.c_int32, ip, ip]
    assert not hasattr(capi.Config, "klt_photometric")


def test_null_handle_is_rejected():
    lib = capi.load()
    for on in (0, 1, 2, -1):
        assert lib.ekfvio_set_klt_photometric(None, on) == capi.EINVAL


def test_python_mirror_has_the_term():
    from ekf_vio_amd import EKFVIO, TightlyCoupledEKF
    assert callable(TightlyCoupledEKF.setKltPhotometric) and callable(EKFVIO.setKltPhotometric)
    assert inspect.signature(TightlyCoupledEKF.__init__).parameters["klt_photometric"].default is False  # EKFVIO(klt_photometric=...) hands it through


def test_shim_knows_klt_photometric(tmp_path):
    src = open(os.path.join(ROOT, "ekf_vio_amd", "host", "ekfvio.hpp")).read()
    assert '"klt_photometric"' in src and "ekfvio_set_klt_photometric" in src and "setKltPhotometric" in src
    assert "klt_photometric" in open(os.path.join(ROOT, "ekf_vio_amd", "host", "ros", "ekfvio_node.cpp")).read()
    from ekf_vio_amd import _build
    _build.build()
    exe = _build.build_host()
    f = tmp_path / "params.yaml"
    f.write_text("klt_photometric: 1\nnum_features: 50\n")
    out = subprocess.run([exe, "--print-config", str(f)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    d = json.loads(out.stdout)
    assert d["klt_photometric"] == 1 and d["max_features"] == 50
    out = subprocess.run([exe, "--print-config"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and json.loads(out.stdout)["klt_photometric"] == 0  # off by default
    for bad in ("2", "-1", "0.5"):
        f.write_text("klt_photometric: %s\n" % bad)
        out = subprocess.run([exe, "--print-config", str(f)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and "error" in out.stderr, bad


# ---- what it restores -------------------------------------------------------------------------------------------------------------
# The second image of the fixture pair changed by rint(g I + o) (tests/_equalize.py, contrast); guess = point; the figure is how many
# tracks end within 1 px of the clean pair's result (oracle tracker, window 21, 4 levels).  Raw: the oracle's tracker on the changed
# pair; with the term: the restatement.  Measured with this file (the constants below are its print-out); the asserted bounds are formed
# from them.  case: (gain, offset) -> (raw, with the term)
CHANGES = ((1.0, 0), (0.9, 0), (0.8, 0), (0.6, 0), (1.0, -15), (1.0, 15), (0.7, 40))
MEASURED_LANDMARKS = {(1.0, 0): (86, 85), (0.9, 0): (82, 85), (0.8, 0): (59, 85), (0.6, 0): (9, 85), (1.0, -15): (80, 85), (1.0, 15): (78, 85),
                      (0.7, 40): (69, 85)}   # the detector's 88 landmarks, 86 of which track on the clean pair
MEASURED_GRID = {(1.0, 0): (63, 63), (0.9, 0): (34, 63), (0.8, 0): (22, 63), (0.6, 0): (4, 62), (1.0, -15): (27, 63), (1.0, 15): (25, 63),
                 (0.7, 40): (27, 62)}        # the 8 x 8 grid, 63 of which track on the clean pair


@functools.lru_cache(maxsize=None)
def _restored(which):
    a, b = fb.image("first"), fb.image("moved")
    pts = replenish(a, EMPTY, 1000).astype(F32) if which == "landmarks" else fb.grid_points(8)
    A, PA = fb.frame("first"), kp.Pyramid(fb.frame("first"))
    clean, st, _ = klt_track(A, fb.frame("moved"), pts, pts.copy())
    ok = st == 1
    out = {"points": len(pts), "clean": int(ok.sum())}
    for g, o in CHANGES:
        B = KltFrame(eq.contrast(b, g, o))
        figures = []
        for photo in (False, True):
            if photo:
                q, s = kp.track(PA, kp.Pyramid(B), pts, pts.copy(), photo=True)
            else:
                q, s, _ = klt_track(A, B, pts, pts.copy())
            d = np.hypot(*(q - clean).astype(np.float64).T)
            near = ok & (s == 1) & (d < 1.0)
            figures += [int(near.sum()), float(np.median(d[ok & (s == 1)]))]
        out[(g, o)] = tuple(figures)
        print(which, "gain", g, "offset", o, "within 1 px: raw %d (median %.4f px), with the term %d (median %.4f px)" % tuple(figures))
    return out


@pytest.mark.parametrize("which,measured", [("landmarks", MEASURED_LANDMARKS), ("grid", MEASURED_GRID)])
def test_tracks_survive_an_exposure_change(which, measured):
    """Asserted: at gain 0.8 the term keeps at least 0.9 x its measured count and at least raw + 10; on the unchanged pair at most 3 of
    the tracked points move beyond 1 px.  Every other case of the table: the term keeps at least 0.9 x its measured count (the same
    form of bound), and the raw figure is the recorded one (the oracle's tracker is deterministic)."""
    r = _restored(which)
    print(which, r)
    assert r["points"] == (88 if which == "landmarks" else 64) and r["clean"] == (86 if which == "landmarks" else 63)
    raw, term = r[(0.8, 0)][0], r[(0.8, 0)][2]
    assert term >= 0.9 * measured[(0.8, 0)][1]
    assert term >= raw + 10
    assert r["clean"] - r[(1.0, 0)][2] <= 3
    for case in CHANGES:
        assert r[case][0] == measured[case][0], case
        assert r[case][2] >= 0.9 * measured[case][1], case
