"""The no-data mask on the device (include/ekfvio.h, ekfvio_set_mask): the blocked map B the handle forms must be, byte for byte, the NumPy
restatement's (tests/_mask.py); the detector's landmarks must be the restated first fit's that starts from B; the tracker's pass flags the
oracle's tracker plus the restated rule; and switched off, or on with nothing to mask, it must leave no trace.  Handles that are compared
run one after the other, each as the device's only live handle."""
import ctypes as C

import numpy as np
import pytest

from ekf_vio_amd import EKFVIO, KLTTracker, TightlyCoupledEKF, capi, EkfvioError

import _klt_fb as fb
import _mask as mk
import _rectify as rc

pytestmark = pytest.mark.gpu
K = rc.kmat(*rc.K_CENTRE)
PINC = rc.D_PINCUSHION
STATE_KEYS = ("base_mu", "feat_mu", "last_klt", "del_flag", "Sigma")


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def pyramid_launches(g):
    return g.profile_report()["klt_pyramid"]["launches"]


# ---- 1: B is the restatement's --------------------------------------------------------------------------------------------------------------
# the smallest shapes that reach every tail: a row whose last word is partial (77, 25, 96 / 1 = three full words for contrast), a block
# remainder (77 x 53 at s = 3), a window wider than a word boundary (pad 11 at every multiple of 32), a last-column pixel
B_CASES = {
    "77x53 border s=1": dict(K=rc.K_OFF, box=(101, 59, 77, 53), D=PINC, kind=None, s=1, pad=11),
    "77x53 s=3": dict(K=rc.K_OFF, box=(101, 59, 77, 53), D=PINC, kind="lastcol", s=3, pad=3),  # (25 x 17: pad 11 would block every pixel)
    "77x53 s=3 pad=11": dict(K=rc.K_OFF, box=(101, 59, 77, 53), D=PINC, kind="lastcol", s=3, pad=11),  # every pixel blocked
    "640x480 s=2 mask+border": dict(K=rc.K_CENTRE, box=None, D=PINC, kind="rect", s=2, pad=11),
    "96x64 pad=1": dict(K=rc.K_OFF, box=(40, 30, 96, 64), D=PINC, kind="pixel", s=1, pad=1),
}


@pytest.mark.parametrize("name", sorted(B_CASES))
def test_blocked_map_on_the_device_is_the_restatement(name):
    c = B_CASES[name]
    img = rc.fixture() if c["box"] is None else rc.crop(*c["box"])
    h, w = img.shape
    m = None if c["kind"] is None else mk.user_mask(c["kind"], w, h)
    g = TightlyCoupledEKF(max_features=16, distortion=c["D"], mask=m, mask_rectify_border=True, inverse_image_scale=c["s"], kill_pad=c["pad"])
    assert g.mask_blocked().shape == (0, 0)  # before the first frame pushed with the mask on
    KLTTracker(g).push_frame(img, rc.kmat(*c["K"]))
    got = g.mask_blocked()
    want = mk.blocked_for(w, h, c["K"], c["D"], c["kind"], c["s"], c["pad"], mk.BORDER)
    assert got.shape == want.shape == (h // c["s"], w // c["s"])
    assert np.array_equal(got, want), (name, int((got != want).sum()))
    assert (0 < want.mean() < 1 or name == "77x53 s=3 pad=11") and mk.nodata_for(w, h, c["K"], c["D"], None, mk.BORDER).any()
    g.close()


# ---- 2: B follows what it was formed for ----------------------------------------------------------------------------------------------------
def test_map_is_formed_again_when_the_mask_the_coefficients_or_the_flag_change_and_not_otherwise():
    box = (0, 0, 320, 200)
    img = rc.crop(*box)
    g = TightlyCoupledEKF(max_features=16, distortion=PINC, mask_rectify_border=True)
    t = KLTTracker(g)
    g.profile(True)

    def push():
        before = pyramid_launches(g)
        t.push_frame(img, K)
        return pyramid_launches(g) - before
    first = push()   # the rectification map, the remap, the two mask kernels, the pyramid
    steady = push()  # the remap and the pyramid
    assert (first, steady) == (5, 2)
    assert np.array_equal(g.mask_blocked(), mk.blocked_for(320, 200, rc.K_CENTRE, PINC, None, 1, 11, mk.BORDER))
    g.setMask(mk.user_mask("rect", 320, 200), rectify_border=True)  # a caller's mask arrives
    assert push() == steady + 2 and push() == steady
    assert np.array_equal(g.mask_blocked(), mk.blocked_for(320, 200, rc.K_CENTRE, PINC, "rect", 1, 11, mk.BORDER))
    g.setMask(mk.user_mask("pixel", 320, 200), rectify_border=True)  # ... and another one
    assert push() == steady + 2 and push() == steady
    assert np.array_equal(g.mask_blocked(), mk.blocked_for(320, 200, rc.K_CENTRE, PINC, "pixel", 1, 11, mk.BORDER))
    g.setDistortion(mk.D_TANGENTIAL)  # the coefficients: the rectification map and B
    assert push() == steady + 3 and push() == steady
    assert np.array_equal(g.mask_blocked(), mk.blocked_for(320, 200, rc.K_CENTRE, mk.D_TANGENTIAL, "pixel", 1, 11, mk.BORDER))
    g.setMask(mk.user_mask("pixel", 320, 200), rectify_border=False)  # the flag (and the caller's mask counts as a new one)
    assert push() == steady + 2 and push() == steady
    assert np.array_equal(g.mask_blocked(), mk.blocked_for(320, 200, None, None, "pixel", 1, 11, 0))
    g.setMask(None)  # off: nothing but the remap and the pyramid, and no B
    assert push() == steady and g.mask_blocked().shape == (0, 0)
    g.close()


# ---- 3: the detector ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,Kc", [(640, 480, rc.K_CENTRE), (1024, 600, (400.0, 400.0, 512.0, 300.0))], ids=["lds mask", "global mask"])
def test_replenish_returns_the_pixels_of_the_restated_first_fit(w, h, Kc):
    """640 x 480: the occupancy image lives in LDS; 1024 x 600 (the fixture tiled): 19 200 words, more than the 16 384 that fit, so the
    variant with the mask in global memory runs."""
    assert ((w + 31) // 32) * h > 16384 if w == 1024 else ((w + 31) // 32) * h <= 16384
    img = mk.tiled_fixture(w, h)
    v = EKFVIO(max_features=256, distortion=PINC, mask_rectify_border=True)
    v.tracker.push_frame(img, rc.kmat(*Kc))
    got = v.replenishFeatures()
    B = mk.blocked_for(w, h, Kc, PINC, None, 1, 11, mk.BORDER)
    assert np.array_equal(v.tc_ekf.mask_blocked(), B)
    rect = rc.remap(img, rc.kmat(*Kc), PINC)
    want = mk.replenish_masked(rect, np.zeros((0, 2), np.float32), 256, B, 50, 30, 11)
    assert np.array_equal(got, want), (len(got), len(want))
    assert len(want) >= 40 and int(B[got[:, 1], got[:, 0]].sum()) == 0
    # the mask matters here: without it the first fit takes other pixels, some of them blocked
    plain = mk.replenish_masked(rect, np.zeros((0, 2), np.float32), 256, np.zeros_like(B), 50, 30, 11)
    assert int(B[plain[:, 1], plain[:, 0]].sum()) >= 1
    # a second call sees the landmarks of the first: their circles are stamped on top of B
    st = v.tc_ekf.get_state()
    px = np.stack([st["feat_mu"][:, 0] * np.float32(Kc[0]), st["feat_mu"][:, 1] * np.float32(Kc[1])], axis=1).astype(np.float32)
    assert np.array_equal(v.replenishFeatures(), mk.replenish_masked(rect, px, 256, B, 50, 30, 11))
    v.tc_ekf.close()


# ---- 4: the tracker -------------------------------------------------------------------------------------------------------------------------
KT = np.array([500.0, 0, 320.0, 0, 500.0, 240.0, 0, 0, 1.0], np.float32)
T0, T1 = 10.0, 10.0 + 1.0 / 30.0
DT = np.float32(np.float64(T1) - np.float64(T0))
# the 8-grid and four points whose destination (flow -21, -7) lies inside the kill box: the mask never counts those
TRACK_PX = np.vstack([fb.grid_points(8), [[31.0, 100.0], [31.5, 200.0], [30.0, 300.0], [200.0, 17.0]]]).astype(np.float32)
UV = np.stack([TRACK_PX[:, 0] / KT[0], TRACK_PX[:, 1] / KT[4]], axis=1).astype(np.float32)
RECT = (200, 140, 460, 340)  # x0, y0, x1, y1 of the caller's no-data rectangle: around the pasted block of "blocked", and wider


def track_mask():
    m = np.full((480, 640), 255, np.uint8)
    m[RECT[1]:RECT[3], RECT[0]:RECT[2]] = 0
    return m


def landmark_handle(second, uv=UV, max_features=80, **cfg):
    g = TightlyCoupledEKF(max_features=max_features, **cfg)
    t = KLTTracker(g)
    t.push_frame(fb.image("first"), KT)
    g.addNewFeatures(uv)
    t.push_frame(fb.image(second), KT)
    g.process(DT)
    return g, t


@pytest.mark.parametrize("second,max_px,sample_based", [("blocked", 0.5, 0), ("blocked", 0.5, 1), ("moved", 0.0, 0)])
def test_tracker_passes_what_the_oracle_passes_less_the_blocked_pixels(second, max_px, sample_based):
    cfg = dict(sample_based_uncertainty=sample_based, klt_fb_max_px=max_px)
    g0, t0 = landmark_handle(second, **cfg)
    z0, R0, p0 = t0.findNewFeaturePositions()
    off = g0.mask_hits()
    assert (off["n_landmarks"], off["masked_last"], len(off["masked"])) == (0, 0, 0) and g0.mask_blocked().shape == (0, 0)
    g0.close()
    g, t = landmark_handle(second, mask=track_mask(), **cfg)
    st = g.get_state()
    # what klt_track_kernel forms from the state, restated (tests/test_gpu_klt_fb.py): reference pixel from last_klt, guess from the prediction
    p = np.stack([st["last_klt"][:, 0] * KT[0], st["last_klt"][:, 1] * KT[4]], axis=1).astype(np.float32)
    gs = np.stack([KT[0] * st["feat_mu"][:, 0], KT[4] * st["feat_mu"][:, 1]], axis=1).astype(np.float32)
    r = fb.restate_fb(fb.frame("first"), fb.frame(second), p, gs, max_px)
    before = (r["s_f"] == 1) & ((r["fb_ok"] == 1) if max_px > 0 else True)
    B = mk.blocked_for(640, 480, None, None, None, 1, 11, 0).copy()
    B |= mk.restate(640, 480, mask=track_mask(), pad=11)
    assert np.array_equal(g.mask_blocked(), B)
    want_pass, want_masked = mk.track_rule(r["q"], before, B, 11)
    z, R, pp = t.findNewFeaturePositions()
    hits = g.mask_hits()
    print(second, max_px, sample_based, "pass", int(pp.sum()), "masked", int(want_masked.sum()), "lost", int((r["s_f"] == 0).sum()),
          "rejected", int(r["rejected"].sum()), "kill box", int((before & (want_pass == 0) & (want_masked == 0)).sum()))
    assert np.array_equal(pp, want_pass)
    assert np.array_equal(hits["masked"], want_masked) and (hits["n_landmarks"], hits["masked_last"]) == (68, int(want_masked.sum()))
    m = want_masked == 1
    assert m.sum() >= 4 and want_pass.sum() >= 20
    assert np.array_equal(pp, np.where(m, 0, p0))  # the unmasked handle's verdicts, less the masked
    assert np.array_equal(bits(z), bits(np.where(m[:, None], np.float32(0), z0)))
    assert np.array_equal(bits(R.reshape(-1, 4)), bits(np.where(m[:, None], np.float32(0), R0.reshape(-1, 4))))
    if not sample_based:  # the constant R and the metric conversion, restated (KLTTracker.cpp:72-92)
        zq = np.stack([r["q"][:, 0] / KT[0], r["q"][:, 1] / KT[4]], axis=1).astype(np.float32)
        assert np.array_equal(bits(z), bits(np.where(want_pass[:, None] == 1, zq, np.float32(0))))
    # a point the kill box or the forward-backward check already failed is not counted, although its pixel is blocked
    box = before & (want_pass == 0) & ~m
    assert box.sum() >= 1 and not hits["masked"][box].any()
    if max_px > 0:
        rej = r["rejected"] == 1
        assert rej.sum() >= 8 and not hits["masked"][rej].any()
    # the update's bookkeeping: a masked landmark is flagged and keeps its last_klt, as a lost one
    assert g.updateWithFeaturePositions(z, R, pp) in (capi.OK, capi.ENUMERIC)
    s1 = g.get_state()
    assert np.array_equal(s1["del_flag"], st["del_flag"] | (pp == 0))
    assert np.array_equal(bits(s1["last_klt"][m]), bits(st["last_klt"][m]))
    g.close()


def test_step_image_removes_a_masked_landmark_in_the_frame_that_masks_it():
    """(The 8-grid alone at a capacity of 64, as tests/test_gpu_klt_fb.py compares the two roads: there the update's launches have one
    geometry whether the host knows the row count or not.)"""
    def step(**cfg):
        v = EKFVIO(max_features=64, mask=track_mask(), **cfg)
        v.addFrame(T0, fb.image("first"), KT)
        v.tc_ekf.addNewFeatures(UV[:64])
        rc_ = v.addFrame(T1, fb.image("moved"), KT)
        out = rc_, v.tc_ekf.get_state(), v.tc_ekf.mask_hits(), v.tc_ekf.num_features
        v.tc_ekf.close()
        return out
    rc_a, sa, ha, _ = step()
    w, t = landmark_handle("moved", uv=UV[:64], max_features=64, mask=track_mask())
    z, R, p = t.findNewFeaturePositions()
    rc_b = w.updateWithFeaturePositions(z, R, p)
    sb, hb = w.get_state(), w.mask_hits()
    w.close()
    assert rc_a == rc_b
    for k in STATE_KEYS:
        assert np.array_equal(raw(sa[k]), raw(sb[k])), k
    assert ha["masked_last"] == hb["masked_last"] >= 4 and np.array_equal(ha["masked"], hb["masked"])
    assert (sa["del_flag"][ha["masked"] == 1] == 1).all()
    _, _, hr, n_left = step(remove_lost=1)
    assert n_left == int(p.sum()) and np.array_equal(hr["masked"], hb["masked"])


# ---- 5: the image loop ----------------------------------------------------------------------------------------------------------------------
def test_image_loop_with_the_border_mask():
    """6 frames at N = 64 with remove_lost = 1, the border mask and pincushion coefficients, on raw frames; and the same loop fed the
    restated-remapped frames with the restated border as a caller's mask (the way the rectification's loop test builds its reference): B
    reaches the device by another road, and every state must have the same bits.  Against the restated pieces: the first frame's landmarks
    are the restated first fit's, every landmark lies on an unblocked pixel when it is added, and each one leaves the state in the frame
    in which it is masked."""
    Kc = (400.0, 400.0, 280.0, 200.0)
    boxes = [(9 * i, 6 * i, 560, 400) for i in range(6)]
    B = mk.blocked_for(560, 400, Kc, PINC, None, 1, 11, mk.BORDER)
    fx, fy = np.float32(Kc[0]), np.float32(Kc[1])

    def loop(frames, **kw):
        v = EKFVIO(max_features=64, replenish=1, remove_lost=1, fast_threshold=20, **kw)
        out, masked_total, added_total = [], 0, 0
        for i, img in enumerate(frames):
            prev = v.tc_ekf.get_state()
            v.addFrame(10.0 + i / 30.0, img, rc.kmat(*Kc))
            st = v.tc_ekf.get_state()
            hits = v.tc_ekf.mask_hits() if i > 0 else dict(masked=np.zeros(0, np.uint8), n_landmarks=0, masked_last=0)
            out.append(tuple(st[k] for k in STATE_KEYS) + (hits["masked"],))
            assert np.array_equal(v.tc_ekf.mask_blocked(), B)
            assert not st["del_flag"].any()
            # the survivors keep their order, the new landmarks follow them: everything new lies on an unblocked pixel
            px = np.rint(np.stack([st["feat_mu"][:, 0] * fx, st["feat_mu"][:, 1] * fy], axis=1).astype(np.float32)).astype(np.int64)
            if i == 0:
                assert np.array_equal(px, mk.replenish_masked(rc.remapped(PINC, Kc, boxes[0]), np.zeros((0, 2), np.float32), 64, B, 20, 30, 11))
                assert int(B[px[:, 1], px[:, 0]].sum()) == 0
            else:
                assert hits["n_landmarks"] == prev["feat_mu"].shape[0]
                m = hits["masked"] == 1
                masked_total += int(m.sum())
                # a masked landmark kept its last_klt until the removal took it: no row of the new state carries it
                gone = [tuple(r) for r in bits(prev["last_klt"][m])]
                have = set(tuple(r) for r in bits(st["last_klt"]))
                assert not any(r in have for r in gone)
            # a landmark that has just been added is exactly pixel2Metric of a whole pixel: such rows lie on unblocked pixels
            uv = st["feat_mu"][:, :2]
            fresh = (bits((px[:, 0].astype(np.float32) / fx)) == bits(uv[:, 0])) & (bits((px[:, 1].astype(np.float32) / fy)) == bits(uv[:, 1]))
            added_total += int(fresh.sum())
            assert int(B[px[fresh, 1], px[fresh, 0]].sum()) == 0
        v.tc_ekf.close()
        assert added_total > 64  # landmarks were added behind the first frame too
        return out, masked_total
    a, masked_a = loop([rc.crop(*b) for b in boxes], distortion=PINC, mask_rectify_border=True)
    user = np.where(mk.nodata_for(560, 400, Kc, PINC, None, mk.BORDER), 0, 255).astype(np.uint8)
    b, masked_b = loop([rc.remapped(PINC, Kc, bx) for bx in boxes], mask=user)
    print("landmarks per frame", [f[1].shape[0] for f in a], "masked in all", masked_a)
    for i, (fa, fb_) in enumerate(zip(a, b)):
        for j, (x, y) in enumerate(zip(fa, fb_)):
            assert x.shape == y.shape and np.array_equal(raw(x), raw(y)), (i, j)
    assert masked_a == masked_b >= 1
    assert a[-1][1].shape[0] >= 16 and not np.array_equal(a[-1][0], a[1][0])


# ---- 6: off means off, and on with nothing to mask means the same bits ------------------------------------------------------------------------
def test_off_and_on_with_nothing_to_mask_leave_every_bit():
    boxes = [(5 * i, 3 * i, 560, 400) for i in range(6)]

    def loop(how):
        v = EKFVIO(max_features=64, replenish=1, remove_lost=1, fast_threshold=20)
        if how == "ones":
            v.setMask(np.full((400, 560), 255, np.uint8))
        elif how == "toggled":
            v.setMask(mk.user_mask("rect", 560, 400), rectify_border=True)
            v.setMask(None)
        out = []
        for i, b in enumerate(boxes):
            v.addFrame(10.0 + i / 30.0, rc.crop(*b), K)
            st = v.tc_ekf.get_state()
            xyz, inten = v.points()
            out.append(tuple(st[k] for k in STATE_KEYS) + (xyz, inten))
        if how == "ones":
            assert np.array_equal(v.tc_ekf.mask_blocked(), mk.kill_box_complement(560, 400, 11))
            assert v.tc_ekf.mask_hits()["masked_last"] == 0
        else:
            assert v.tc_ekf.mask_blocked().shape == (0, 0) and v.tc_ekf.mask_hits()["n_landmarks"] == 0
        v.tc_ekf.close()
        return out
    ref = loop("off")
    assert ref[-1][1].shape[0] >= 16
    for how in ("ones", "toggled"):
        got = loop(how)
        for i, (fa, fb_) in enumerate(zip(got, ref)):
            for j, (x, y) in enumerate(zip(fa, fb_)):
                assert x.shape == y.shape and np.array_equal(raw(x), raw(y)), (how, i, j)


# ---- 7: a property of the handle ------------------------------------------------------------------------------------------------------------
def test_reset_keeps_the_mask_a_wrong_size_is_refused_and_a_refused_call_changes_nothing():
    m = mk.user_mask("rect", 320, 200)
    img = rc.crop(0, 0, 320, 200)
    want = mk.blocked_for(320, 200, None, None, "rect", 1, 11, 0)
    g = TightlyCoupledEKF(max_features=16, mask=m)
    t = KLTTracker(g)
    t.push_frame(img, K)
    assert np.array_equal(g.mask_blocked(), want)
    g.initializeBaseState()
    t.push_frame(img, K)
    assert np.array_equal(g.mask_blocked(), want)
    # a frame of another size is refused and not ingested; the handle works on afterwards
    level0 = t.level(0)[0]
    with pytest.raises(EkfvioError) as e:
        t.push_frame(rc.crop(0, 0, 300, 200), K)
    assert e.value.code == capi.EINVAL and "320 x 200" in str(e.value) and "300 x 200" in str(e.value)
    v8 = np.ascontiguousarray(rc.crop(0, 0, 300, 200))
    assert g.lib.ekfvio_step_image(g.h, 1.0, v8.ctypes.data_as(C.POINTER(C.c_uint8)), 300, 200, 300, K.ctypes.data_as(C.POINTER(C.c_float))) == capi.EINVAL
    assert np.array_equal(t.level(0)[0], level0)
    t.push_frame(img, K)
    assert np.array_equal(g.mask_blocked(), want)
    # every refused ekfvio_set_mask leaves the setting what it was
    mp = np.ascontiguousarray(m).ctypes.data_as(C.POINTER(C.c_uint8))
    lib = g.lib
    assert lib.ekfvio_set_mask(g.h, mp, 320, 200, 320, 2) == capi.EINVAL      # unknown flag bits
    assert lib.ekfvio_set_mask(g.h, None, 320, 200, 320, 0) == capi.EINVAL    # NULL with a non-zero size
    assert lib.ekfvio_set_mask(g.h, None, 0, 0, 0, 4) == capi.EINVAL
    assert lib.ekfvio_set_mask(g.h, mp, 320, 200, 319, 0) == capi.EINVAL      # stride < width
    assert lib.ekfvio_set_mask(g.h, mp, 0, 200, 320, 0) == capi.EINVAL        # sizes outside [1, 16384]
    assert lib.ekfvio_set_mask(g.h, mp, 320, 16385, 320, 0) == capi.EINVAL
    t.push_frame(img, K)
    assert np.array_equal(g.mask_blocked(), want)
    with pytest.raises(EkfvioError):
        t.push_frame(rc.crop(0, 0, 300, 200), K)  # the size rule still holds: the mask is still set
    # ekfvio_get_mask: the size alone, and a buffer that is too small
    w, h = C.c_int32(0), C.c_int32(0)
    assert lib.ekfvio_get_mask(g.h, None, 0, C.byref(w), C.byref(h)) == capi.OK and (w.value, h.value) == (320, 200)
    small = np.zeros(10, np.uint8)
    assert lib.ekfvio_get_mask(g.h, small.ctypes.data_as(C.POINTER(C.c_uint8)), 10, C.byref(w), C.byref(h)) == capi.EINVAL
    # the border flag with distortion off contributes nothing and is no error; without a caller's mask any size is taken
    g.setMask(None, rectify_border=True)
    t.push_frame(rc.crop(0, 0, 300, 200), K)
    assert np.array_equal(g.mask_blocked(), mk.kill_box_complement(300, 200, 11))
    g.close()
