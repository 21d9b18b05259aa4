"""Camera models on the device (include/ekfvio.h, ekfvio_set_camera_model): the map each instance of the map kernel writes must be,
entry for entry, the NumPy restatement (tests/_camera_models.py), and level 0 of the pushed frame its restated remap, byte for byte; the
map follows the model, the coefficients and P; with P set everything behind the rectification takes P for the frame's intrinsics; the
mask's border term reads the new map; and the plumb_bob, no-P case and the off case keep the parent's bytes.  Handles that are compared run
one after the other, each as the device's only live handle."""
import ctypes as C

import numpy as np
import pytest

from ekf_vio_amd import EKFVIO, KLTTracker, TightlyCoupledEKF, capi, mask_blocked_model

import _camera_models as cm
import _mask as mk
import _rectify as rc

pytestmark = pytest.mark.gpu

MODELS = {"plumb_bob": (cm.PLUMB_BOB, rc.D_BARREL2), "rational": (cm.RATIONAL, cm.D_RATIONAL), "equidistant": (cm.EQUIDISTANT, cm.D_EQUI),
          "equidistant0": (cm.EQUIDISTANT, cm.D_EQUI_ZERO)}
# 67 x 45: a tail group of four entries (3015 = 4 * 753 + 3) and more than one block; 64 x 48: a width that is a multiple of 4, full groups
FRAMES = {"67x45": (cm.K_SMALL, (101, 59, 67, 45)), "64x48": ((41.5, 38.25, 30.75, 24.5), (300, 200, 64, 48))}


def device_map(g):
    w, h = C.c_int32(0), C.c_int32(0)
    g._chk(g.lib.ekfvio_test_rectify_map(g.h, None, None, 0, C.byref(w), C.byref(h)))
    sx, sy = np.zeros((h.value, w.value), np.int32), np.zeros((h.value, w.value), np.int32)
    ip = C.POINTER(C.c_int32)
    g._chk(g.lib.ekfvio_test_rectify_map(g.h, sx.ctypes.data_as(ip), sy.ctypes.data_as(ip), sx.size, C.byref(w), C.byref(h)))
    return sx, sy


def check(g, t, K, model, D, P, box):
    """Pushes the crop `box` and holds the device's map and level 0 to the restatement."""
    x0, y0, w, h = box
    t.push_frame(rc.crop(*box), rc.kmat(*K))
    sx, sy = device_map(g)
    rx, ry, _ = cm.map_for(K, model, D, P, w, h)
    assert sx.shape == (h, w)
    assert np.array_equal(sx, rx) and np.array_equal(sy, ry), (int((sx != rx).sum()), int((sy != ry).sum()))
    got, want = t.level(0)[0], cm.remapped(K, model, D, P, box)
    assert np.array_equal(got, want), int((got != want).sum())
    return got


# ---- 1: the map and level 0 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_P", [False, True], ids=["K", "P"])
@pytest.mark.parametrize("frame", sorted(FRAMES))
@pytest.mark.parametrize("mname", sorted(MODELS))
def test_map_and_level0_are_the_restatement(mname, frame, with_P):
    model, D = MODELS[mname]
    K, box = FRAMES[frame]
    P = cm.P_SMALL if with_P else None
    g = TightlyCoupledEKF(max_features=16, hooks=True, camera_model=(model, D, None if P is None else cm.p4(*P)))
    got = check(g, KLTTracker(g), K, model, D, P, box)
    assert not np.array_equal(got, rc.crop(*box))
    g.close()


def test_the_full_map_at_640x480_is_the_restatement():
    """Every entry of the largest frame of the tests, for the two new instances: where the device's fp64 square root, division or the
    polynomial differed from IEEE in the last place of some entry, it would show here."""
    g = TightlyCoupledEKF(max_features=16, hooks=True)
    t = KLTTracker(g)
    for model, D, P in ((cm.EQUIDISTANT, cm.D_EQUI, None), (cm.EQUIDISTANT, cm.D_EQUI_ZERO, cm.P_ZOOM), (cm.RATIONAL, cm.D_RATIONAL, cm.P_ZOOM),
                        (cm.RATIONAL, cm.D_RATIONAL_POLE, None)):
        g.setCameraModel(model, D, None if P is None else cm.p4(*P))
        check(g, t, rc.K_CENTRE, model, D, P, (0, 0, 640, 480))
    assert (device_map(g)[0] == rc.SENTINEL).any()  # the pole's entries carry the sentinel on the device too
    g.close()


# ---- 2: the map follows its key ---------------------------------------------------------------------------------------------------------
def test_map_is_formed_again_when_the_model_the_coefficients_or_P_change():
    K, box = FRAMES["67x45"]
    g = TightlyCoupledEKF(max_features=16, hooks=True)
    t = KLTTracker(g)
    seq = [(cm.EQUIDISTANT, cm.D_EQUI, None), (cm.EQUIDISTANT, cm.D_EQUI_TUMVI, None), (cm.RATIONAL, cm.D_RATIONAL, None),
           (cm.RATIONAL, cm.D_RATIONAL, cm.P_SMALL), (cm.RATIONAL, cm.D_RATIONAL, (101.0, 90.0, 35.5, 20.25)), (cm.PLUMB_BOB, rc.D_BARREL2, None),
           (cm.EQUIDISTANT, cm.D_EQUI, None)]
    seen = []
    for model, D, P in seq:
        g.setCameraModel(model, D, None if P is None else cm.p4(*P))
        seen.append(check(g, t, K, model, D, P, box).copy())
        check(g, t, K, model, D, P, box)  # a second frame with the same key: the kept map
    for i in range(len(seq) - 2):
        assert not np.array_equal(seen[i], seen[i + 1]), i
    assert np.array_equal(seen[0], seen[-1])  # switching back gives the first bytes again
    st = g.cameraModel()
    assert st["model"] == cm.EQUIDISTANT and np.array_equal(st["D"], np.array(cm.D_EQUI)) and st["P"] is None and st["on"]
    g.close()


# ---- 3: P downstream --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2])
def test_with_P_the_landmarks_are_the_rectified_cameras(s):
    """ekfvio_replenish's pixels and ekfvio_get_features' (u, v) satisfy Feature::pixel2Metric (u = x / fx in fp32, the reference's
    cx = cy = 0 quirk) with fx = (float)((double)fx' / s) -- and not with K's."""
    K, P = rc.K_CENTRE, cm.P_ZOOM
    v = EKFVIO(max_features=64, inverse_image_scale=s, fast_threshold=20, camera_model=(cm.RATIONAL, cm.D_RATIONAL, cm.p4(*P)))
    v.tracker.push_frame(rc.fixture(), rc.kmat(*K))
    px = v.replenishFeatures()
    assert len(px) >= 16
    st = v.tc_ekf.get_state()

    def metric(cam):
        fx, fy = np.float32(np.float64(np.float32(cam[0])) / s), np.float32(np.float64(np.float32(cam[1])) / s)
        return np.stack([px[:, 0].astype(np.float32) / fx, px[:, 1].astype(np.float32) / fy], axis=1)
    assert np.array_equal(st["feat_mu"][:, :2], metric(P)) and np.array_equal(st["last_klt"], metric(P))
    assert not np.array_equal(st["feat_mu"][:, :2], metric(K))
    # ... and the pixels were found on the rectified frame
    want = cm.remapped(K, cm.RATIONAL, cm.D_RATIONAL, P)
    if s == 1:
        assert np.array_equal(v.tracker.level(0)[0], want)
    v.tc_ekf.close()


# ---- 4: the mask's border term ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2])
def test_blocked_map_on_the_device_reads_the_new_map(s):
    """Equidistant, D = 0, K = (400, 400, 320, 240), P = (200, 200, 320, 240): the border is live by construction."""
    K, P, w, h = rc.K_CENTRE, (200.0, 200.0, 320.0, 240.0), 640, 480
    g = TightlyCoupledEKF(max_features=16, camera_model=(cm.EQUIDISTANT, cm.D_EQUI_ZERO, cm.p4(*P)), mask_rectify_border=True, inverse_image_scale=s)
    KLTTracker(g).push_frame(rc.fixture(), rc.kmat(*K))
    got = g.mask_blocked()
    want = mask_blocked_model(rc.kmat(*K), cm.EQUIDISTANT, cm.D_EQUI_ZERO, cm.p4(*P), None, w, h, s, 11, mk.BORDER)
    assert got.shape == (h // s, w // s) and np.array_equal(got, want), int((got != want).sum())
    assert got[240 // s, 0] == 1 and got[240 // s, 320 // s] == 0 and 0.05 < got.mean() < 0.95
    # P alone, then the flag with the setting off: a border of a re-projection, then none but the kill box
    g.setCameraModel(cm.PLUMB_BOB, (), cm.p4(*P))
    KLTTracker(g).push_frame(rc.fixture(), rc.kmat(*K))
    assert np.array_equal(g.mask_blocked(), mask_blocked_model(rc.kmat(*K), cm.PLUMB_BOB, (), cm.p4(*P), None, w, h, s, 11, mk.BORDER))
    g.setCameraModel(cm.RATIONAL, (0.0,) * 8, None)
    KLTTracker(g).push_frame(rc.fixture(), rc.kmat(*K))
    assert np.array_equal(g.mask_blocked(), mk.kill_box_complement(w // s, h // s, 11))
    g.close()


# ---- 5: unchanged behaviour -------------------------------------------------------------------------------------------------------------
def frame_bytes(g, t, img, K):
    t.push_frame(img, K)
    return [np.ascontiguousarray(a).view(np.uint8).copy() for l in range(4) for a in t.level(l)]


def test_plumb_bob_through_the_new_setter_is_ekfvio_set_distortion():
    K = rc.kmat(*rc.K_CENTRE)
    a = TightlyCoupledEKF(max_features=16, distortion=rc.D_BARREL2)
    ref = frame_bytes(a, KLTTracker(a), rc.fixture(), K)
    assert np.array_equal(ref[0].reshape(480, 640), rc.remapped(rc.D_BARREL2))
    a.close()
    b = TightlyCoupledEKF(max_features=16, camera_model=(cm.PLUMB_BOB, rc.D_BARREL2, None))
    got = frame_bytes(b, KLTTracker(b), rc.fixture(), K)
    st = b.cameraModel()
    assert st["model"] == cm.PLUMB_BOB and len(st["D"]) == 5 and st["P"] is None and st["on"]
    b.close()
    assert len(ref) == len(got) and all(np.array_equal(x, y) for x, y in zip(ref, got))


def test_off_after_on_is_a_handle_that_never_had_it():
    K = rc.kmat(*rc.K_CENTRE)
    a = TightlyCoupledEKF(max_features=16)
    ref = frame_bytes(a, KLTTracker(a), rc.fixture(), K)
    assert np.array_equal(ref[0].reshape(480, 640), rc.fixture())
    a.close()
    for off in ((cm.PLUMB_BOB, (), None), (cm.PLUMB_BOB, (0.0,) * 5, None), (cm.RATIONAL, (0.0,) * 8, None)):
        b = TightlyCoupledEKF(max_features=16, camera_model=(cm.EQUIDISTANT, cm.D_EQUI, cm.p4(*cm.P_ZOOM)))
        t = KLTTracker(b)
        t.push_frame(rc.fixture(), K)  # (the map and the second staging plane now exist)
        assert np.array_equal(t.level(0)[0], cm.remapped(rc.K_CENTRE, cm.EQUIDISTANT, cm.D_EQUI, cm.P_ZOOM))
        b.setCameraModel(*off)
        assert not b.cameraModel()["on"]
        got = frame_bytes(b, t, rc.fixture(), K)
        b.close()
        assert all(np.array_equal(x, y) for x, y in zip(ref, got)), off


def test_a_refused_call_changes_nothing_and_reset_keeps_the_setting():
    K, box = FRAMES["67x45"]
    g = TightlyCoupledEKF(max_features=16, hooks=True, camera_model=(cm.EQUIDISTANT, cm.D_EQUI, cm.p4(*cm.P_SMALL)))
    t = KLTTracker(g)
    check(g, t, K, cm.EQUIDISTANT, cm.D_EQUI, cm.P_SMALL, box)
    d8 = (C.c_double * 8)(*cm.D_RATIONAL)
    dnan = (C.c_double * 4)(float("nan"), 0.0, 0.0, 0.0)
    bad_P = (C.c_float * 4)(0.0, 1.0, 100.0, 1.0)
    for model, d, n, p in ((3, d8, 8, None), (cm.RATIONAL, d8, 5, None), (cm.EQUIDISTANT, d8, 8, None), (cm.EQUIDISTANT, dnan, 4, None),
                           (cm.RATIONAL, None, 8, None), (cm.RATIONAL, d8, 8, bad_P)):
        assert g.lib.ekfvio_set_camera_model(g.h, model, d, n, p) == capi.EINVAL
    g.initializeBaseState()
    st = g.cameraModel()
    assert st["model"] == cm.EQUIDISTANT and np.array_equal(st["D"], np.array(cm.D_EQUI)) and np.array_equal(st["P"], cm.p4(*cm.P_SMALL)) and st["on"]
    check(g, t, K, cm.EQUIDISTANT, cm.D_EQUI, cm.P_SMALL, box)
    g.setDistortion(rc.D_BARREL1)  # the last setter wins: plumb_bob, no P
    st = g.cameraModel()
    assert st["model"] == cm.PLUMB_BOB and st["P"] is None and len(st["D"]) == 5
    check(g, t, K, cm.PLUMB_BOB, rc.D_BARREL1, None, box)
    g.close()
