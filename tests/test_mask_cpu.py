"""The no-data mask (include/ekfvio.h, ekfvio_set_mask), the part that needs no GPU: ekfvio_mask_blocked is a pure host function that
compiles the inline functions the kernels compile, and must give, byte for byte, the NumPy restatement of the three specification steps
(tests/_mask.py); with nothing to mask the blocked map is the complement of Frame::isPixelInBox; the restated first fit with an empty map
is the oracle's replenishment; and the premise -- the unmasked detector does put landmarks on the rectification border -- is measured."""
import ctypes as C

import numpy as np
import pytest

from ekf_vio_amd import EkfvioError, capi, mask_blocked
from oracle import replenish

import _mask as mk
import _rectify as rc

CASES = {"640x480": (rc.K_CENTRE, 640, 480), "77x53": (rc.K_OFF, 77, 53)}
# coefficient sets; "sentinel": D_HUGE seen through fx = fy = 1e-3, where the map holds the sentinel (tests/test_rectify_cpu.py)
D_SETS = {"zero": rc.D_ZERO, "pincushion4": rc.D_PINCUSHION, "tangential4": mk.D_TANGENTIAL, "huge": rc.D_HUGE, "sentinel": rc.D_HUGE}
MASKS = [None, "rect", "pixel", "lastcol"]


def camera(case, dname):
    K, w, h = CASES[case]
    if dname == "sentinel":
        K = (1e-3, 1e-3, K[2], K[3])
    return K, w, h


@pytest.mark.parametrize("dname", sorted(D_SETS))
@pytest.mark.parametrize("case", sorted(CASES))
def test_blocked_map_has_the_bytes_of_the_restatement(case, dname):
    """s in {1, 2, 3} (at 77 x 53, s = 3 leaves a remainder), pad in {0, 1, 11}, without a caller's mask and with one pushed with
    stride > width: a rectangle, a single zero pixel, a zero pixel in the last column."""
    K, w, h = camera(case, dname)
    D = D_SETS[dname]
    nd_border = mk.nodata_for(w, h, K, D, None, mk.BORDER)
    if dname == "zero":
        assert not nd_border.any()
    elif dname == "sentinel":
        assert nd_border.mean() > 0.99
    else:
        assert nd_border.any()
    for kind in MASKS:
        m = None if kind is None else mk.with_stride(mk.user_mask(kind, w, h))
        assert m is None or m.strides[0] > w
        for s in (1, 2, 3):
            for pad in (0, 1, 11):
                got = mask_blocked(rc.kmat(*K), D, m, w, h, s, pad, mk.BORDER)
                want = mk.blocked_for(w, h, K, D, kind, s, pad, mk.BORDER)
                assert got.shape == (h // s, w // s) == want.shape
                assert np.array_equal(got, want), (case, dname, kind, s, pad, int((got != want).sum()))
    # without the flag the border contributes nothing, whatever the coefficients
    got = mask_blocked(rc.kmat(*K), D, mk.user_mask("rect", w, h), w, h, 2, 11, 0)
    assert np.array_equal(got, mk.blocked_for(w, h, None, None, "rect", 2, 11, 0))


@pytest.mark.parametrize("pad", [0, 1, 11])
def test_with_nothing_no_data_the_map_is_the_complement_of_the_kill_box(pad):
    for case, dname in (("640x480", "zero"), ("77x53", "zero"), ("640x480", "barrel1"), ("640x480", "barrel2")):
        K, w, h = CASES[case]
        D = {"zero": rc.D_ZERO, "barrel1": rc.D_BARREL1, "barrel2": rc.D_BARREL2}[dname]
        assert not mk.nodata_for(w, h, K, D, None, mk.BORDER).any()  # barrel lenses leave no border with the same camera matrix
        for s in (1, 2, 3):
            want = mk.kill_box_complement(w // s, h // s, pad)
            assert np.array_equal(mk.blocked_for(w, h, K, D, None, s, pad, mk.BORDER), want), (case, dname, s)
            assert np.array_equal(mask_blocked(rc.kmat(*K), D, mk.user_mask("ones", w, h), w, h, s, pad, mk.BORDER), want), (case, dname, s)
    if pad == 0:
        assert not mk.kill_box_complement(64, 48, 0).any()


@pytest.mark.parametrize("frame", ["fixture", "pincushion"])
def test_restated_first_fit_with_an_empty_map_is_the_oracles_replenishment(frame):
    img = rc.fixture() if frame == "fixture" else rc.remapped(rc.D_PINCUSHION)
    ex = np.array([[100.4, 100.5], [320.0, 240.0], [630.0, 470.0]], np.float32)
    for existing, num in ((np.zeros((0, 2), np.float32), 256), (ex, 40), (ex, 3)):
        want = replenish(img, existing, num, 50, 30, 11)
        got = mk.replenish_masked(img, existing, num, np.zeros(img.shape, np.uint8), 50, 30, 11)
        assert np.array_equal(got, want), (frame, num)
    assert len(replenish(img, np.zeros((0, 2), np.float32), 256, 50, 30, 11)) >= 50


def test_premise_the_unmasked_detector_takes_landmarks_on_the_border_and_the_masked_one_does_not():
    """Measured with this file's helpers on remapped(D_PINCUSHION): the oracle's replenishment takes 91 landmarks, 13 of them on
    blocked pixels.  The conditions: at least one without the mask, none with it, and still at least half as many landmarks."""
    img = rc.remapped(rc.D_PINCUSHION)
    B = mk.blocked_for(640, 480, rc.K_CENTRE, rc.D_PINCUSHION, None, 1, 11, mk.BORDER)
    none = np.zeros((0, 2), np.float32)
    plain = replenish(img, none, 256, 50, 30, 11)
    on_blocked = int(B[plain[:, 1], plain[:, 0]].sum())
    print("unmasked: %d landmarks, %d on blocked pixels; no-data pixels: %d" %
          (len(plain), on_blocked, int(mk.nodata_for(640, 480, rc.K_CENTRE, rc.D_PINCUSHION, None, mk.BORDER).sum())))
    assert on_blocked >= 1
    masked = mk.replenish_masked(img, none, 256, B, 50, 30, 11)
    print("masked: %d landmarks" % len(masked))
    assert int(B[masked[:, 1], masked[:, 0]].sum()) == 0
    assert 2 * len(masked) >= len(plain)


def test_arguments():
    lib = capi.load()
    for name in ("ekfvio_set_mask", "ekfvio_get_mask", "ekfvio_get_mask_hits", "ekfvio_mask_blocked"):
        assert name in capi.SYMBOLS and hasattr(lib, name)
    K = rc.kmat(*rc.K_OFF)
    kp = K.ctypes.data_as(C.POINTER(C.c_float))
    d = (C.c_double * 5)(0.15, -0.05, 0.0, 0.0, 0.0)
    m = np.full((8, 12), 255, np.uint8)
    mp = m.ctypes.data_as(C.POINTER(C.c_uint8))
    out = np.full((8, 8), 7, np.uint8)
    op = out.ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.ekfvio_mask_blocked(kp, d, 5, mp, 8, 8, 12, 1, 1, 1, op) == capi.OK and out.max() <= 1
    out[:] = 7
    assert lib.ekfvio_mask_blocked(kp, d, 5, mp, 8, 8, 12, 1, 1, 2, op) == capi.EINVAL   # unknown flag bits
    assert lib.ekfvio_mask_blocked(kp, d, 5, mp, 8, 8, 7, 1, 1, 1, op) == capi.EINVAL    # stride < width
    assert lib.ekfvio_mask_blocked(kp, d, 5, mp, 0, 8, 12, 1, 1, 1, op) == capi.EINVAL   # sizes outside [1, 16384]
    assert lib.ekfvio_mask_blocked(kp, d, 5, mp, 8, 16385, 12, 1, 1, 1, op) == capi.EINVAL
    assert lib.ekfvio_mask_blocked(kp, d, 3, mp, 8, 8, 12, 1, 1, 1, op) == capi.EINVAL   # D, count as ekfvio_rectify_map takes them
    assert lib.ekfvio_mask_blocked(kp, None, 5, mp, 8, 8, 12, 1, 1, 1, op) == capi.EINVAL
    assert lib.ekfvio_mask_blocked(None, d, 5, mp, 8, 8, 12, 1, 1, 1, op) == capi.EINVAL  # the border term is live and needs K
    assert lib.ekfvio_mask_blocked(kp, d, 5, mp, 8, 8, 12, 9, 1, 1, op) == capi.EINVAL   # level 0 would be empty
    assert lib.ekfvio_mask_blocked(kp, d, 5, mp, 8, 8, 12, 1, 1, 1, None) == capi.EINVAL
    assert (out == 7).all()  # a refused call writes nothing
    assert lib.ekfvio_mask_blocked(None, None, 0, None, 8, 8, 0, 1, 1, 0, op) == capi.OK  # no mask, no border: the kill box alone
    assert np.array_equal(out, mk.kill_box_complement(8, 8, 1))
    # the handle's entry points refuse a null handle before anything else
    assert lib.ekfvio_set_mask(None, mp, 8, 8, 12, 0) == capi.EINVAL
    assert lib.ekfvio_get_mask(None, None, 0, None, None) == capi.EINVAL
    assert lib.ekfvio_get_mask_hits(None, None, None, None) == capi.EINVAL
    with pytest.raises(EkfvioError) as e:
        mask_blocked(K, rc.D_PINCUSHION, None, 8, 8, 1, 11, 4)
    assert e.value.code == capi.EINVAL
    assert capi.MASK_RECTIFY_BORDER == mk.BORDER == 1
