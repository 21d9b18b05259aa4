"""Rectification of distorted frames on the device (include/ekfvio.h, ekfvio_set_distortion): with coefficients set, level 0 of a pushed
frame's pyramid must be, byte for byte, the NumPy restatement's remap (tests/_rectify.py) of that frame, at full size, on an odd crop
with a row stride, behind the resize, across changes of K and D; switched off it must leave no trace; and the image loop fed raw frames
must be the image loop fed the restated-remapped ones.  Handles that are compared run one after the other, each as the device's only
live handle."""
import ctypes as C

import numpy as np
import pytest

from ekf_vio_amd import EKFVIO, KLTTracker, TightlyCoupledEKF, capi
from oracle import frame_resize

import _klt_fb as fb
import _rectify as rc

pytestmark = pytest.mark.gpu
K = rc.kmat(*rc.K_CENTRE)
D_SETS = {"barrel1": rc.D_BARREL1, "barrel2": rc.D_BARREL2, "pincushion4": rc.D_PINCUSHION}


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def handle(D=None, **cfg):
    g = TightlyCoupledEKF(max_features=256, distortion=D, **cfg)
    return g, KLTTracker(g)


# ---- 1-3: level 0 is the restated remap ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", sorted(D_SETS))
def test_level0_at_full_size(dname):
    D = D_SETS[dname]
    g, t = handle(D)
    t.push_frame(rc.fixture(), K)
    got, _ = t.level(0)
    want = rc.remapped(D)
    assert np.array_equal(got, want), (dname, int((got != want).sum()))
    assert not np.array_equal(want, rc.fixture())
    if dname == "pincushion4":
        assert (want[:2, :2] == 0).all() and (want[-2:, -2:] == 0).all()  # taps outside the frame: black corners
    g.close()


@pytest.mark.parametrize("dname", ["barrel1", "pincushion4"])
def test_level0_on_an_odd_crop_pushed_with_a_stride(dname):
    """211 x 157 out of the 640-wide fixture: partial groups of four pixels, partial pyramid tiles, an odd pitch, an off-centre camera."""
    D, box = D_SETS[dname], (101, 59, 211, 157)
    Koff = rc.kmat(*rc.K_OFF)
    base = np.ascontiguousarray(rc.fixture())
    x0, y0, w, h = box
    g, t = handle(D)
    ptr = C.cast(base.ctypes.data + y0 * 640 + x0, C.POINTER(C.c_uint8))
    g._chk(g.lib.ekfvio_klt_push_frame(g.h, ptr, w, h, 640, Koff.ctypes.data_as(C.POINTER(C.c_float))))
    got, _ = t.level(0)
    want = rc.remapped(D, rc.K_OFF, box)
    assert got.shape == (157, 211)
    assert np.array_equal(got, want), (dname, int((got != want).sum()))
    assert not np.array_equal(want, rc.crop(*box))
    g.close()


def test_level0_behind_the_resize():
    g, t = handle(rc.D_BARREL1, inverse_image_scale=2)
    t.push_frame(rc.fixture(), K)
    got, _ = t.level(0)
    want = frame_resize(rc.remapped(rc.D_BARREL1), 2)
    assert got.shape == (240, 320) and np.array_equal(got, want)
    assert not np.array_equal(want, frame_resize(rc.fixture(), 2))
    g.close()


# ---- 4: the map follows the camera ------------------------------------------------------------------------------------------------------
def test_map_is_formed_again_when_the_camera_or_the_coefficients_change():
    K1, K2 = rc.K_CENTRE, (380.0, 410.0, 300.5, 250.25)
    g, t = handle(rc.D_BARREL1)
    for Kx in (K1, K2, K1, K1):
        t.push_frame(rc.fixture(), rc.kmat(*Kx))
        assert np.array_equal(t.level(0)[0], rc.remapped(rc.D_BARREL1, Kx)), Kx
    assert not np.array_equal(rc.remapped(rc.D_BARREL1, K1), rc.remapped(rc.D_BARREL1, K2))
    g.setDistortion(rc.D_BARREL2)
    t.push_frame(rc.fixture(), rc.kmat(*K1))
    assert np.array_equal(t.level(0)[0], rc.remapped(rc.D_BARREL2, K1))
    # another size with the same camera: the crop's own map
    box = (0, 0, 320, 200)
    t.push_frame(rc.crop(*box), rc.kmat(*K1))
    assert np.array_equal(t.level(0)[0], rc.remapped(rc.D_BARREL2, K1, box))
    g.close()


# ---- 5: off means off -------------------------------------------------------------------------------------------------------------------
def test_off_means_off():
    pts, guess, _ = fb.reference("moved", True, 0.5)

    def run(toggle):
        g, t = handle()
        if toggle:
            g.setDistortion(rc.D_BARREL1)
            t.push_frame(rc.fixture(), K)  # (the map and the second staging plane now exist)
            assert np.array_equal(t.level(0)[0], rc.remapped(rc.D_BARREL1))
            g.setDistortion(rc.D_ZERO)
        t.push_frame(fb.image("first"), K), t.push_frame(fb.image("moved"), K)
        out = t.level(0) + t.track_points(pts, guess)
        g.close()
        return out
    ref, got = run(False), run(True)
    assert np.array_equal(ref[0], fb.image("moved"))
    for a, b in zip(got, ref):
        assert np.array_equal(raw(a), raw(b))
    for off in (None, (), (0.0,) * 4, (-0.0, 0.0, 0.0, 0.0, 0.0)):
        g, t = handle(rc.D_BARREL1)
        g.setDistortion(off)
        t.push_frame(rc.fixture(), K)
        assert np.array_equal(t.level(0)[0], rc.fixture()), off
        g.close()


def test_reset_keeps_the_coefficients_and_a_refused_call_changes_nothing():
    g, t = handle(rc.D_BARREL1)
    t.push_frame(rc.fixture(), K)
    assert np.array_equal(t.level(0)[0], rc.remapped(rc.D_BARREL1))
    g.initializeBaseState()
    t.push_frame(rc.fixture(), K)
    assert np.array_equal(t.level(0)[0], rc.remapped(rc.D_BARREL1))
    d5 = (C.c_double * 5)(float("nan"), 0.0, 0.0, 0.0, 0.0)
    d3 = (C.c_double * 3)(0.1, 0.1, 0.1)
    assert g.lib.ekfvio_set_distortion(g.h, d5, 5) == capi.EINVAL
    assert g.lib.ekfvio_set_distortion(g.h, d3, 3) == capi.EINVAL
    assert g.lib.ekfvio_set_distortion(g.h, None, 5) == capi.EINVAL
    t.push_frame(rc.fixture(), K)
    assert np.array_equal(t.level(0)[0], rc.remapped(rc.D_BARREL1))
    g.close()


# ---- 6: the image loop ------------------------------------------------------------------------------------------------------------------
def test_image_loop_on_raw_frames_is_the_loop_on_remapped_ones():
    Kc = (400.0, 400.0, 280.0, 200.0)
    boxes = [(5 * i, 3 * i, 560, 400) for i in range(6)]

    def loop(D, frames):
        v = EKFVIO(max_features=32, replenish=1, remove_lost=1, fast_threshold=20, distortion=D)
        out = []
        for i, img in enumerate(frames):
            v.addFrame(10.0 + i / 30.0, img, rc.kmat(*Kc))
            st = v.tc_ekf.get_state()
            xyz, inten = v.points()
            out.append((st["base_mu"], st["feat_mu"], st["last_klt"], st["del_flag"], st["Sigma"], xyz, inten))
        v.tc_ekf.close()
        return out
    a = loop(rc.D_BARREL1, [rc.crop(*b) for b in boxes])
    b = loop(None, [rc.remapped(rc.D_BARREL1, Kc, bx) for bx in boxes])
    for i, (fa, fb_) in enumerate(zip(a, b)):
        for j, (x, y) in enumerate(zip(fa, fb_)):
            assert x.shape == y.shape and np.array_equal(raw(x), raw(y)), (i, j)
    assert a[-1][1].shape[0] >= 16 and a[-1][6].max() > 0  # landmarks were found and followed, their intensities read from the rectified frame
    assert not np.array_equal(a[-1][0], a[1][0])
