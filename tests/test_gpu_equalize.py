"""Equalisation of pushed frames on the device (include/ekfvio.h, ekfvio_set_equalize): with the setting on, level 0 of a pushed frame's
pyramid must be, byte for byte, the NumPy restatement (tests/_equalize.py) of that frame -- at full size, on an odd crop with a row stride,
on ragged tiles, on a constant frame, behind the resize and behind the rectification; the tables must follow the setting and the frame
size; switched off it must leave no trace, in the outputs or in the handle's memory; and the image loop fed raw frames must be the image
loop fed the restated ones.  Handles that are compared run one after the other, each as the device's only live handle."""
import ctypes as C
import gc

import numpy as np
import pytest

from ekf_vio_amd import EKFVIO, KLTTracker, TightlyCoupledEKF, capi
from oracle import frame_resize, replenish

import _equalize as eq
import _rectify as rc

pytestmark = pytest.mark.gpu
K = eq.kmat(*eq.K_CENTRE)
S = eq.SETTING


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def handle(equalize=S, **cfg):
    g = TightlyCoupledEKF(max_features=256, equalize=equalize, **cfg)
    return g, KLTTracker(g)


def level0(t, img, Kx=K):
    t.push_frame(img, Kx)
    return t.level(0)[0]


# ---- 1: level 0 is the restatement --------------------------------------------------------------------------------------------------------
def test_level0_at_full_size():
    g, t = handle()
    got, want = level0(t, eq.fixture()), eq.restated("first", *S)
    assert np.array_equal(got, want), int((got != want).sum())
    assert not np.array_equal(want, eq.fixture())
    g.close()


def test_level0_on_an_odd_crop_pushed_with_a_stride():
    """211 x 157 out of the 640-wide fixture: tw = 27, th = 20, five reflected columns and three reflected rows, rows that start at every
    alignment, a partial last group of four pixels."""
    box = (101, 59, 211, 157)
    x0, y0, w, h = box
    base = np.ascontiguousarray(eq.fixture())
    g, t = handle()
    ptr = C.cast(base.ctypes.data + y0 * 640 + x0, C.POINTER(C.c_uint8))
    g._chk(g.lib.ekfvio_klt_push_frame(g.h, ptr, w, h, 640, K.ctypes.data_as(C.POINTER(C.c_float))))
    got, want = t.level(0)[0], eq.restated(box, *S)
    assert got.shape == (157, 211) and np.array_equal(got, want), int((got != want).sum())
    g.close()


@pytest.mark.parametrize("w,h,setting", [(77, 53, (3.0, 8, 8)), (64, 48, (3.0, 3, 5)), (9, 8, (3.0, 8, 8)), (33, 17, (3.0, 1, 1))],
                         ids=["77x53_8x8", "64x48_3x5", "9x8_8x8", "33x17_1x1"])
def test_level0_on_ragged_tiles(w, h, setting):
    img = eq.crop(100, 100, w, h)
    g, t = handle(setting)
    got, want = level0(t, img), eq.restate(img, *setting)
    assert np.array_equal(got, want), int((got != want).sum())
    g.close()


def test_level0_of_a_constant_frame_and_of_two_values():
    g, t = handle()
    got, want = level0(t, eq.constant()), eq.restated("constant", *S)
    assert np.array_equal(got, want) and len(np.unique(want)) == 1
    cb = eq.checkerboard()
    assert np.array_equal(level0(t, cb), eq.restate(cb, *S))
    sp = eq.spiky()
    g.setEqualize(1.0, 2, 2)  # res above 128 in every tile: step = 1
    assert np.array_equal(level0(t, sp), eq.restate(sp, 1.0, 2, 2))
    g.close()


def test_level0_behind_the_resize():
    g, t = handle(inverse_image_scale=2)
    got, want = level0(t, eq.fixture()), frame_resize(eq.restated("first", *S), 2)
    assert got.shape == (240, 320) and np.array_equal(got, want)
    assert not np.array_equal(want, frame_resize(eq.fixture(), 2))
    g.close()


def test_level0_behind_the_rectification():
    g, t = handle(distortion=rc.D_BARREL1)
    got, want = level0(t, eq.fixture()), eq.restate(rc.remapped(rc.D_BARREL1), *S)
    assert np.array_equal(got, want), int((got != want).sum())
    assert not np.array_equal(want, eq.restated("first", *S))
    g.close()


# ---- 2: the tables follow the setting -------------------------------------------------------------------------------------------------------
def test_the_tables_follow_the_setting_and_the_frame_size():
    g, t = handle()
    img = eq.fixture()
    assert np.array_equal(level0(t, img), eq.restated("first", 3.0, 8, 8))
    g.setEqualize(2.0, 4, 4)
    assert np.array_equal(level0(t, img), eq.restated("first", 2.0, 4, 4))
    g.setEqualize(0.0)
    assert np.array_equal(level0(t, img), img)  # off: the raw frame
    g.setEqualize(3.0, 8, 8)
    assert np.array_equal(level0(t, img), eq.restated("first", 3.0, 8, 8))
    box = (0, 0, 320, 200)
    assert np.array_equal(level0(t, eq.crop(*box)), eq.restated(box, 3.0, 8, 8))
    g.setEqualize(3.0, 16, 16)  # more tiles than the tables were allocated for
    assert np.array_equal(level0(t, img), eq.restated("first", 3.0, 16, 16))
    assert np.array_equal(level0(t, eq.fixture("moved")), eq.restated("moved", 3.0, 16, 16))
    g.close()


# ---- 3: off leaves no trace -----------------------------------------------------------------------------------------------------------------
def image_loop(frames, equalize=None, toggle=False, n=32, **kw):
    v = EKFVIO(max_features=n, replenish=1, remove_lost=1, equalize=equalize, **kw)
    if toggle:
        v.setEqualize(*S)
        v.tracker.push_frame(eq.fixture(), K)  # (the tables now exist)
        assert np.array_equal(v.tracker.level(0)[0], eq.restated("first", *S))
        v.setEqualize(0.0)
        v.tc_ekf.initializeBaseState()
    out = []
    for i, img in enumerate(frames):
        v.addFrame(10.0 + i / 30.0, img, K)
        st = v.tc_ekf.get_state()
        xyz, inten = v.points()
        out.append((st["base_mu"], st["feat_mu"], st["last_klt"], st["del_flag"], st["Sigma"], xyz, inten))
    v.tc_ekf.close()
    return out


BOXES = [(5 * i, 3 * i, 560, 400) for i in range(6)]


def same_loops(a, b):
    for i, (fa, fb_) in enumerate(zip(a, b)):
        for j, (x, y) in enumerate(zip(fa, fb_)):
            assert x.shape == y.shape and np.array_equal(raw(x), raw(y)), (i, j)


def test_off_leaves_no_trace_in_the_image_loop():
    frames = [eq.crop(*b) for b in BOXES]
    never, toggled = image_loop(frames), image_loop(frames, toggle=True)
    same_loops(never, toggled)
    assert never[-1][1].shape[0] >= 16


def test_off_allocates_nothing_and_on_allocates_the_tables_once():
    gc.collect()
    lib = capi.load(hooks=True)
    DEV_LIVE, DEV_BYTES, PIN_LIVE, PIN_BYTES, DEV_ACQ, DEV_REL = range(6)

    def mem(g):
        out = (C.c_int64 * 8)()
        assert lib.ekfvio_test_mem(g.h, out) == capi.OK
        return np.array(list(out), np.int64)

    a, b = eq.crop(0, 0, 160, 120), eq.crop(3, 2, 160, 120)
    never = TightlyCoupledEKF(max_features=8, hooks=True, max_image_width=160, max_image_height=120)
    tn = KLTTracker(never)
    created = mem(never)
    tn.push_frame(a, K), tn.push_frame(b, K)
    assert np.array_equal(mem(never), created)  # a handle that never had it on: its frames allocate nothing, as before
    never.close()
    g = TightlyCoupledEKF(max_features=8, hooks=True, max_image_width=160, max_image_height=120)
    t = KLTTracker(g)
    assert np.array_equal(mem(g), created)
    g.setEqualize(*S)
    assert np.array_equal(mem(g), created)  # the setting alone: nothing
    t.push_frame(a, K)
    m1 = mem(g)
    assert m1[DEV_LIVE] == created[DEV_LIVE] + 1 and m1[DEV_BYTES] == created[DEV_BYTES] + 8 * 8 * 256 and m1[DEV_REL] == created[DEV_REL]
    assert m1[PIN_LIVE] == created[PIN_LIVE] and m1[PIN_BYTES] == created[PIN_BYTES]
    t.push_frame(b, K)
    g.setEqualize(2.0, 4, 4), t.push_frame(a, K)  # fewer tiles: the tables stay
    g.setEqualize(0.0), t.push_frame(b, K)
    assert np.array_equal(mem(g), m1)
    g.setEqualize(3.0, 16, 8), t.push_frame(a, K)  # more tiles: replaced, never added to
    m2 = mem(g)
    assert m2[DEV_LIVE] == m1[DEV_LIVE] and m2[DEV_BYTES] == created[DEV_BYTES] + 16 * 8 * 256 and m2[DEV_REL] == m1[DEV_REL] + 1
    g.close()


# ---- 4: end to end --------------------------------------------------------------------------------------------------------------------------
def test_image_loop_on_raw_frames_is_the_loop_on_restated_ones():
    a = image_loop([eq.crop(*b) for b in BOXES], equalize=S, n=64)
    b = image_loop([eq.restated(bx, *S) for bx in BOXES], n=64)
    same_loops(a, b)
    assert a[-1][1].shape[0] >= 32 and a[-1][6].max() > 0  # landmarks were found and followed, their intensities read from the equalised frame
    assert not np.array_equal(a[-1][0], a[1][0])


def test_replenish_on_the_quarter_contrast_frame_takes_the_oracles_picks():
    v = EKFVIO(max_features=256, equalize=S)
    assert v.addFrame(1.0, eq.quarter_contrast(), K) == capi.OK
    px = v.replenishFeatures()
    ref = replenish(eq.restated("quarter", *S), np.zeros((0, 2), np.float32), 256)
    assert len(ref) >= 40 and np.array_equal(px, ref)
    assert len(replenish(eq.quarter_contrast(), np.zeros((0, 2), np.float32), 256)) <= 16
    v.tc_ekf.close()


# ---- 5: refusal and reset -------------------------------------------------------------------------------------------------------------------
def test_a_frame_with_fewer_columns_than_tiles_is_refused_and_reset_keeps_the_setting():
    g, t = handle()
    first = eq.crop(100, 100, 64, 48)
    assert np.array_equal(level0(t, first), eq.restate(first, *S))
    kp = K.ctypes.data_as(C.POINTER(C.c_float))
    narrow, flat = np.ascontiguousarray(eq.crop(0, 0, 7, 48)), np.ascontiguousarray(eq.crop(0, 0, 64, 5))
    for img in (narrow, flat):
        h, w = img.shape
        assert g.lib.ekfvio_klt_push_frame(g.h, img.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, w, kp) == capi.EINVAL
        assert b"tiles" in g.lib.ekfvio_last_error(g.h)
        assert g.lib.ekfvio_step_image(g.h, 1.0, img.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, w, kp) == capi.EINVAL
        assert np.array_equal(t.level(0)[0], eq.restate(first, *S))  # not ingested: the previous frame is still current
    # refused settings change nothing
    for clip, tx, ty in ((-1.0, 8, 8), (float("nan"), 8, 8), (float("inf"), 8, 8), (3.0, 0, 8), (3.0, 8, 0), (3.0, 17, 8), (3.0, 8, 17)):
        assert g.lib.ekfvio_set_equalize(g.h, clip, tx, ty) == capi.EINVAL, (clip, tx, ty)
    assert np.array_equal(level0(t, eq.fixture()), eq.restated("first", *S))
    g.initializeBaseState()  # ekfvio_reset: the setting is a property of the handle
    assert np.array_equal(level0(t, eq.fixture()), eq.restated("first", *S))
    g.setEqualize(0.0, 0, 0)  # off: the tile counts are not looked at
    assert np.array_equal(level0(t, eq.fixture()), eq.fixture())
    g.close()
