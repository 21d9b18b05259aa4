"""Equalisation of pushed frames (include/ekfvio.h, ekfvio_set_equalize), the part that needs no GPU: ekfvio_equalize is a host function
that compiles the inline functions the device's kernels compile (csrc/equalize.h), so the device's arithmetic is held to the NumPy
restatement (tests/_equalize.py) here; and what the stage is for -- a detector with a fixed threshold and a tracker that assumes brightness
constancy -- is held to the CPU oracle's detector and tracker."""
import ctypes as C

import numpy as np
import pytest

from ekf_vio_amd import EkfvioError, capi, equalize
from oracle import KltFrame, klt_track, replenish

import _equalize as eq

EMPTY = np.zeros((0, 2), np.float32)


def _inputs():
    fx = eq.fixture()
    return {
        "640x480_3_8_8": (fx, 3.0, 8, 8),
        "640x480_2_4_4": (fx, 2.0, 4, 4),
        "640x480_40_8_8": (fx, 40.0, 8, 8),
        "77x53_3_8_8": (eq.crop(100, 100, 77, 53), 3.0, 8, 8),      # tw = 10, th = 7: three reflected columns and rows
        "64x48_3_3_5": (eq.crop(100, 100, 64, 48), 3.0, 3, 5),
        "9x8_3_8_8": (eq.crop(100, 100, 9, 8), 3.0, 8, 8),          # tiles 2 x 1, clip = 1; whole tiles lie in the reflected part
        "33x17_3_1_1": (eq.crop(100, 100, 33, 17), 3.0, 1, 1),      # one tile: the interpolation is clamped on all sides
        "211x157_stride640": (fx[50:50 + 157, 30:30 + 211], 3.0, 8, 8),
        "constant": (eq.constant(), 3.0, 8, 8),                     # one bin holds A, the excess is A - clip
        "checkerboard": (eq.checkerboard(), 3.0, 8, 8),
        "res_above_128": (eq.spiky(), 1.0, 2, 2),
    }


INPUTS = _inputs()


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_host_function_has_the_bits_of_the_restatement(name):
    img, clip, tx, ty = INPUTS[name]
    if name == "211x157_stride640":
        assert img.strides == (640, 1)
    if name == "77x53_3_8_8":
        p = eq.params(77, 53, clip, tx, ty)
        assert (p["tw"], p["th"]) == (10, 7) and 8 * 10 - 77 == 3 and 8 * 7 - 53 == 3
    if name == "9x8_3_8_8":
        p = eq.params(9, 8, clip, tx, ty)
        assert (p["tw"], p["th"], p["clip"]) == (2, 1, 1)
    if name == "constant":
        _, info = eq.restate_tiles(img, clip, tx, ty)
        p = eq.params(640, 480, clip, tx, ty)
        assert (info["excess"] == p["A"] - p["clip"]).all()
    if name == "res_above_128":
        _, info = eq.restate_tiles(img, clip, tx, ty)
        assert (info["res"] > 128).any() and (info["step"][info["res"] > 128] == 1).all()
    out = equalize(img, clip, tx, ty)
    ref = eq.restate(img, clip, tx, ty)
    assert out.shape == ref.shape and np.array_equal(out, ref)


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_tables_end_at_255_and_never_decrease(name):
    img, clip, tx, ty = INPUTS[name]
    lut, _ = eq.restate_tiles(img, clip, tx, ty)
    assert (lut[:, :, 255] == 255).all()
    assert (np.diff(lut.astype(np.int32), axis=2) >= 0).all()


def test_one_tile_is_a_table_lookup():
    img, clip, tx, ty = INPUTS["33x17_3_1_1"]
    lut, _ = eq.restate_tiles(img, clip, tx, ty)
    assert np.array_equal(equalize(img, clip, tx, ty), lut[0, 0][img])


# measured with the committed restatement (see the docstrings); the bounds below are formed from these
MEASURED_QUARTER = (7, 56)   # landmarks taken on the quarter-contrast frame: raw, equalised
MEASURED_GAIN08 = (59, 82)   # tracks within 1 px of the clean pair's at gain 0.8: raw, equalised (of 86 that track on the clean pair)


def test_detection_comes_back_on_a_low_contrast_frame():
    """replenish (CPU oracle; threshold 50, radius 30, pad 11, an empty filter) on rint(0.25 I + 96) of the 640 x 480 fixture, raw and
    equalised at (3, 8, 8).  Measured with tests/_equalize.py: 7 landmarks raw, 56 equalised (the unchanged fixture: 88 and 136; half
    contrast 57 and 92; dark, g = 0.3: 19 and 66).  Asserted: raw at most 16; equalised at least 0.8 x 56 and at least 3 x raw."""
    raw = len(replenish(eq.quarter_contrast(), EMPTY, 1000))
    equalised = len(replenish(eq.restated("quarter", *eq.SETTING), EMPTY, 1000))
    print("quarter contrast: landmarks raw", raw, "equalised", equalised)
    assert raw <= 16
    assert equalised >= 0.8 * MEASURED_QUARTER[1]
    assert equalised >= 3 * raw


def test_tracking_survives_a_gain_change():
    """The detector's landmarks of the first image (88; 86 track into the moved image, guess = point) tracked into gain-0.8 of the moved
    image (CPU oracle tracker, window 21, 4 levels), raw and with both frames equalised at (3, 8, 8); the figure is how many end within
    1 px of the clean pair's result.  Measured with tests/_equalize.py: 59 raw (median 0.33 px), 82 equalised (median 0.09 px); on the
    unchanged pair equalisation keeps 85 of the 86 within 1 px (median 0.04 px).  Asserted: equalised at least 0.9 x 82 and at least
    raw + 10; on the unchanged pair at most 3 of the tracked points lost to beyond 1 px."""
    a, b = eq.fixture("first"), eq.fixture("moved")
    pts = replenish(a, EMPTY, 1000).astype(np.float32)
    clean, st, _ = klt_track(KltFrame(a), KltFrame(b), pts, pts.copy())
    ok = st == 1

    def within(f1, f2):
        out, s, _ = klt_track(KltFrame(f1), KltFrame(f2), pts, pts.copy())
        d = np.hypot(*(out - clean).astype(np.float64).T)
        return int((ok & (s == 1) & (d < 1.0)).sum())

    b08 = eq.contrast(b, 0.8, 0)
    ea = eq.restated("first", *eq.SETTING)
    raw = within(a, b08)
    equalised = within(ea, eq.restate(b08, *eq.SETTING))
    same = within(ea, eq.restated("moved", *eq.SETTING))
    print("points", len(pts), "tracked clean", int(ok.sum()), "gain 0.8 within 1 px: raw", raw, "equalised", equalised, "unchanged pair equalised", same)
    assert equalised >= 0.9 * MEASURED_GAIN08[1]
    assert equalised >= raw + 10
    assert int(ok.sum()) - same <= 3


def test_arguments():
    lib = capi.load()
    assert "ekfvio_set_equalize" in capi.SYMBOLS and "ekfvio_equalize" in capi.SYMBOLS
    assert lib.ekfvio_set_equalize(None, 3.0, 8, 8) == capi.EINVAL
    img = np.ascontiguousarray(eq.crop(100, 100, 64, 48))
    out = np.zeros_like(img)
    ip, op = img.ctypes.data_as(C.POINTER(C.c_uint8)), out.ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.ekfvio_equalize(ip, 64, 48, 64, 3.0, 8, 8, op) == capi.OK
    assert lib.ekfvio_equalize(None, 64, 48, 64, 3.0, 8, 8, op) == capi.EINVAL
    assert lib.ekfvio_equalize(ip, 64, 48, 64, 3.0, 8, 8, None) == capi.EINVAL
    assert lib.ekfvio_equalize(ip, 0, 48, 64, 3.0, 8, 8, op) == capi.EINVAL
    assert lib.ekfvio_equalize(ip, 64, 0, 64, 3.0, 8, 8, op) == capi.EINVAL
    assert lib.ekfvio_equalize(ip, 64, 48, 63, 3.0, 8, 8, op) == capi.EINVAL      # stride < width
    assert lib.ekfvio_equalize(ip, 16385, 1, 16385, 3.0, 1, 1, op) == capi.EINVAL
    assert lib.ekfvio_equalize(ip, 8, 48, 64, 3.0, 9, 8, op) == capi.EINVAL       # fewer columns than tiles
    assert lib.ekfvio_equalize(ip, 64, 4, 64, 3.0, 8, 5, op) == capi.EINVAL       # fewer rows than tiles
    for clip, tx, ty in ((0.0, 8, 8), (-1.0, 8, 8), (float("nan"), 8, 8), (float("inf"), 8, 8), (3.0, 0, 8), (3.0, 8, 0), (3.0, 17, 8),
                         (3.0, 8, 17), (3.0, -1, 8)):
        assert lib.ekfvio_equalize(ip, 64, 48, 64, clip, tx, ty, op) == capi.EINVAL, (clip, tx, ty)
        with pytest.raises(EkfvioError) as e:
            equalize(img, clip, tx, ty)
        assert e.value.code == capi.EINVAL
    # a huge finite limit clips nothing and is no error
    assert np.array_equal(equalize(img, 3.0e38, 4, 4), eq.restate(img, 3.0e38, 4, 4))
