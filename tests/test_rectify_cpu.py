"""Rectification of distorted frames (include/ekfvio.h, ekfvio_set_distortion), the part that needs no GPU: ekfvio_rectify_map is a
host function that compiles the inline function the device's map kernel compiles, so the device's arithmetic is held to the NumPy
restatement (tests/_rectify.py) here; and the specification itself is held to an independent model of a distorting camera through the
CPU oracle's tracker."""
import ctypes as C

import numpy as np
import pytest

from ekf_vio_amd import EkfvioError, capi, rectify_map
from oracle import KltFrame, klt_track

import _klt_fb as fb
import _rectify as rc

CASES = [(rc.K_CENTRE, 640, 480), (rc.K_OFF, 77, 53)]
D_SETS = {"zero": rc.D_ZERO, "barrel1": rc.D_BARREL1, "barrel2": rc.D_BARREL2, "pincushion4": rc.D_PINCUSHION}


@pytest.mark.parametrize("dname", sorted(D_SETS))
@pytest.mark.parametrize("K,w,h", CASES, ids=["640x480", "77x53"])
def test_map_has_the_bits_of_the_restatement(K, w, h, dname):
    D = D_SETS[dname]
    sx, sy = rectify_map(rc.kmat(*K), D, w, h)
    rx, ry, valid = rc.restate_map(rc.kmat(*K), D, w, h)
    assert valid.all()
    assert np.array_equal(sx, rx) and np.array_equal(sy, ry)


@pytest.mark.parametrize("w,h,cx,cy", [(640, 480, 320.0, 240.0), (77, 53, 40.25, 71.5)])
def test_map_carries_the_sentinel_where_the_restatement_says_invalid(w, h, cx, cy):
    K = rc.kmat(1e-3, 1e-3, cx, cy)
    sx, sy = rectify_map(K, rc.D_HUGE, w, h)
    rx, ry, valid = rc.restate_map(K, rc.D_HUGE, w, h)
    assert (~valid).any()
    if (cx, cy) == (320.0, 240.0):
        assert valid.any()  # both kinds occur: the entry at the principal point stays in range
    assert np.array_equal(sx, rx) and np.array_equal(sy, ry)
    assert (sx[~valid] == rc.SENTINEL).all() and (sy[~valid] == rc.SENTINEL).all()
    assert (sx[valid] != rc.SENTINEL).all()
    # a sentinel entry gives 0 by itself: all four taps lie outside the frame
    img = np.full((h, w), 255, np.uint8)
    assert (rc.restate_remap(img, rx, ry)[~valid] == 0).all()


@pytest.mark.parametrize("count", [0, 4, 5])
def test_zero_coefficients_are_the_identity(count):
    img = rc.fixture()
    h, w = img.shape
    sx, sy = rectify_map(rc.kmat(*rc.K_CENTRE), (0.0,) * count, w, h)
    x, y = np.meshgrid(np.arange(w, dtype=np.int32), np.arange(h, dtype=np.int32))
    assert np.array_equal(sx, 32 * x) and np.array_equal(sy, 32 * y)
    assert np.array_equal(rc.restate_remap(img, sx, sy), img)
    sx, sy = rectify_map(rc.kmat(*rc.K_OFF), (0.0,) * count, 77, 53)
    assert np.array_equal(sx, 32 * x[:53, :77]) and np.array_equal(sy, 32 * y[:53, :77])


# max displacement measured with this file's helpers (see the docstring below); the bound is 1.25 x the measured value
MEASURED_MAX_PX = {"barrel1": 0.3996, "barrel2": 0.4067}


@pytest.mark.parametrize("dname", ["barrel1", "barrel2"])
def test_the_specification_rectifies(dname):
    """remap(distort(original)) is the original again, to the tracker: from the original into it, with guess = point, the 8 x 8 grid
    comes back with zero flow, and into the unrectified distort(original) it does not.  distort() (tests/_rectify.py) inverts the model
    by fixed-point iteration and shares no line with the restatement; a mirrored map, a transposed one or one that is half a pixel off
    fails here.  Measured with these helpers (CPU oracle tracker, window 21, 4 levels), K = (400, 400, 320, 240):
        barrel1 (-0.28, 0.07, 2e-4, -1e-4, 0):     63 of 64 status 1, max 0.3996 px, mean 0.0742 px; unrectified median 10.14 px
        barrel2 (-0.4, 0.2, 1e-3, -2e-3, -0.05):   63 of 64 status 1, max 0.4067 px, mean 0.0740 px; unrectified median 13.47 px
    Asserted: at least 60 of 64 tracked, their max displacement below 1 px (the condition) and at most 1.25 x the measured value; the
    unrectified median above 5 px.  (The pincushion set is left out on purpose: its distorted image has no data in the corners.)"""
    D = D_SETS[dname]
    original = KltFrame(rc.fixture())
    pts = fb.grid_points(8)
    rect = KltFrame(rc.remap(rc.distorted(D), rc.kmat(*rc.K_CENTRE), D))
    out, st, _ = klt_track(original, rect, pts, pts.copy())
    ok = st == 1
    disp = np.hypot(*(out[ok] - pts[ok]).astype(np.float64).T)
    print(dname, "tracked", int(ok.sum()), "max", float(disp.max()), "mean", float(disp.mean()))
    raw = KltFrame(rc.distorted(D))
    out_raw, st_raw, _ = klt_track(original, raw, pts, pts.copy())
    disp_raw = np.hypot(*(out_raw[st_raw == 1] - pts[st_raw == 1]).astype(np.float64).T)
    print(dname, "unrectified: tracked", int((st_raw == 1).sum()), "median", float(np.median(disp_raw)))
    assert ok.sum() >= 60
    assert disp.max() < 1.0
    assert disp.max() <= 1.25 * MEASURED_MAX_PX[dname]
    assert np.median(disp_raw) > 5.0


def test_arguments():
    lib = capi.load()
    d = (C.c_double * 5)(*rc.D_BARREL1)
    assert lib.ekfvio_set_distortion(None, d, 5) == capi.EINVAL
    assert lib.ekfvio_set_distortion(None, None, 0) == capi.EINVAL
    K = rc.kmat(*rc.K_OFF)
    for bad in ((0.1, 0.2, 0.3), (0.1,) * 6, (float("nan"), 0, 0, 0), (0, 0, 0, 0, float("inf"))):
        with pytest.raises(EkfvioError) as e:
            rectify_map(K, bad, 8, 8)
        assert e.value.code == capi.EINVAL
    sx = np.zeros((8, 8), np.int32)
    ip = sx.ctypes.data_as(C.POINTER(C.c_int32))
    kp = K.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.ekfvio_rectify_map(kp, None, 4, 8, 8, ip, ip) == capi.EINVAL  # NULL with count > 0
    assert lib.ekfvio_rectify_map(None, d, 5, 8, 8, ip, ip) == capi.EINVAL
    assert lib.ekfvio_rectify_map(kp, d, 5, 8, 8, None, ip) == capi.EINVAL
    assert lib.ekfvio_rectify_map(kp, d, 5, 0, 8, ip, ip) == capi.EINVAL
    assert lib.ekfvio_rectify_map(kp, None, 0, 8, 8, ip, ip) == capi.OK
    assert "ekfvio_set_distortion" in capi.SYMBOLS and "ekfvio_rectify_map" in capi.SYMBOLS
