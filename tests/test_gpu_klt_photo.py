"""The tracker's gain/offset term on the device (include/ekfvio.h, ekfvio_set_klt_photometric): with the setting on, klt_track_kernel's
second instance must give, bit for bit, the NumPy restatement of a Lucas-Kanade pass with the term (tests/_klt_photo.py, which without the
term is held to the CPU oracle's tracker in tests/test_klt_photo_cpu.py) -- forward, and back in the forward-backward check; switched off
it must leave no trace; and in the image loop it must be the call-by-call path and keep landmarks that the tracker without it loses to
an exposure flicker.  References are computed once per case and shared."""
import functools

import numpy as np
import pytest

from ekf_vio_amd import EKFVIO, KLTTracker, TightlyCoupledEKF, capi
from ekf_vio_amd.sim import translated_sequence
from oracle import KltFrame, klt_track

import _equalize as eq
import _klt_fb as fb
import _klt_photo as kp

pytestmark = pytest.mark.gpu
F32 = np.float32
K = np.array([500.0, 0, 320.0, 0, 500.0, 240.0, 0, 0, 1.0], F32)
OFFSET = np.array([-20.0, -6.0], F32)  # a coarse prediction, as the filter would give
OTHER_POINTS = np.vstack([fb.grid_points(10), [[5.0, 5.0], [-40.0, 100.0], [639.0, 479.0], [320.5, 0.25], [2.0, 470.0]]]).astype(F32)


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


@functools.lru_cache(maxsize=None)
def changed():
    """The second image of the fixture pair behind an exposure change: rint(0.8 I + 10)."""
    out = eq.contrast(fb.image("moved"), 0.8, 10)
    out.setflags(write=False)
    return out


def handle(photo=True, **cfg):
    g = TightlyCoupledEKF(max_features=256, klt_photometric=photo, **cfg)
    return g, KLTTracker(g)


@functools.lru_cache(maxsize=None)
def pyramids(win=21, levels=3):
    A, B = fb.frame("first", win, levels), KltFrame(changed(), win=win, max_level=levels)
    return A, B, kp.Pyramid(A), kp.Pyramid(B)


# ---- 1: the forward pass ------------------------------------------------------------------------------------------------------------
def test_track_points_through_an_exposure_change_has_the_restatements_bits():
    """The 219 points of test_gpu_klt.py (two grids, the border and the points outside the frame), guess = point.  The raw tracker's
    result on this pair is another one: the comparison is not met by a kernel that ignores the setting."""
    pts = fb.all_points()
    A, B, PA, PB = pyramids()
    want, ws = kp.track(PA, PB, pts, pts.copy(), photo=True)
    g, t = handle()
    t.push_frame(fb.image("first"), K), t.push_frame(changed(), K)
    got, gs = t.track_points(pts, pts.copy())
    g.close()
    assert np.array_equal(gs, ws)
    assert np.array_equal(raw(got), raw(want)), float(np.abs(got - want).max())
    on, os_, _ = klt_track(A, B, pts, pts.copy())
    assert (np.abs(on - want).max(axis=1) > 0.01).sum() >= 50
    outside = np.array([len(pts) - 4, len(pts) - 3])  # (-40, 100) and (700, 100)
    assert (gs[outside] == 0).all() and gs.sum() >= 200


@pytest.mark.parametrize("win,levels,iters", [(3, 3, 30), (7, 3, 30), (21, 0, 3)])
def test_other_windows_have_the_restatements_bits(win, levels, iters):
    """Windows 3 and 7 (lanes and slots past the window hold zeros before AND behind the projection; n = 9, 49) and 21 on one level."""
    guess = (OTHER_POINTS + OFFSET).astype(F32)
    _, _, PA, PB = pyramids(win, levels)
    want, ws = kp.track(PA, PB, OTHER_POINTS, guess, photo=True, win=win, max_iter=iters)
    g, t = handle(klt_window_size=win, klt_max_pyramid_level=levels, klt_max_iterations=iters)
    t.push_frame(fb.image("first"), K), t.push_frame(changed(), K)
    got, gs = t.track_points(OTHER_POINTS, guess.copy())
    g.close()
    assert np.array_equal(gs, ws)
    assert np.array_equal(raw(got), raw(want)), float(np.abs(got - want).max())
    assert gs.sum() >= 40


def test_small_image_with_three_levels_and_a_flat_patch():
    """160 x 120: level 3 would not be larger than the window.  And a constant frame: VI == 0, the mean is removed, the min-eigenvalue
    test fails as before."""
    img = np.ascontiguousarray(fb.image("first")[::4, ::4])
    nxt = eq.contrast(np.roll(img, 2, axis=1), 0.8, 10)
    o1, o2 = KltFrame(img), KltFrame(nxt)
    assert o1.levels == 3
    pts = np.array([[40.0, 40.0], [80.0, 60.0], [120.0, 90.0], [3.0, 3.0], [158.5, 118.0], [-30.0, 60.0]], F32)
    want, ws = kp.track(kp.Pyramid(o1), kp.Pyramid(o2), pts, pts.copy(), photo=True)
    g, t = handle()
    t.push_frame(img, K), t.push_frame(nxt, K)
    got, gs = t.track_points(pts, pts.copy())
    assert np.array_equal(gs, ws) and np.array_equal(raw(got), raw(want))
    assert gs[:3].all() and gs[5] == 0
    flat = np.full((120, 160), 90, np.uint8)
    t.push_frame(flat, K), t.push_frame(flat, K)
    _, st = t.track_points([[80.0, 60.0]], [[80.0, 60.0]])
    assert list(st) == [0]
    g.close()


# ---- 2: the backward pass -----------------------------------------------------------------------------------------------------------
def test_forward_backward_check_runs_both_passes_with_the_term():
    pts = fb.all_points()
    guess = (pts + OFFSET).astype(F32)
    _, _, PA, PB = pyramids()
    wq, ws, wback, werr2, wok = kp.track_fb(PA, PB, pts, guess, max_px=1.0, photo=True)
    g, t = handle(klt_fb_max_px=1.0)
    t.push_frame(fb.image("first"), K), t.push_frame(changed(), K)
    q, s, back, err2, ok = t.track_points_fb(pts, guess.copy())
    g.close()
    assert np.array_equal(s, ws) and np.array_equal(raw(q), raw(wq))
    assert np.array_equal(raw(back), raw(wback)), float(np.abs(back - wback).max())
    assert np.array_equal(raw(err2), raw(werr2))
    assert np.array_equal(ok, wok)
    assert ok.sum() >= 150 and (s == 0).sum() >= 2 and ((s == 1) & (ok == 0)).sum() >= 1  # every verdict occurs


# ---- 3: off means off ---------------------------------------------------------------------------------------------------------------
def test_off_means_off():
    """A handle switched on and then off gives the oracle's bits again; a handle never switched on gives the bits of one set to 0; the
    setting moves no counter."""
    pts = fb.all_points()
    A, B, _, _ = pyramids()
    on, os_, _ = klt_track(A, B, pts, pts.copy())
    g, t = handle(photo=False)
    t.push_frame(fb.image("first"), K), t.push_frame(changed(), K)
    never, never_s = t.track_points(pts, pts.copy())
    c0 = g.counters()
    g.setKltPhotometric(True)
    with_term, _ = t.track_points(pts, pts.copy())
    g.setKltPhotometric(False)
    again, again_s = t.track_points(pts, pts.copy())
    assert g.counters() == c0
    g.close()
    z, tz = handle(photo=False)
    z.setKltPhotometric(0)
    tz.push_frame(fb.image("first"), K), tz.push_frame(changed(), K)
    zero, zero_s = tz.track_points(pts, pts.copy())
    assert z.counters() == c0
    z.close()
    assert not np.array_equal(raw(with_term), raw(never))
    for got, gs in ((never, never_s), (again, again_s), (zero, zero_s)):
        assert np.array_equal(gs, os_) and np.array_equal(raw(got), raw(on))


def test_values_other_than_0_and_1_are_refused_and_reset_keeps_the_setting():
    pts = fb.grid_points(8)
    g, t = handle()
    for bad in (2, -1, 255):
        assert g.lib.ekfvio_set_klt_photometric(g.h, bad) == capi.EINVAL
    g.initializeBaseState()
    t.push_frame(fb.image("first"), K), t.push_frame(changed(), K)
    got, gs = t.track_points(pts, pts.copy())
    g.close()
    _, _, PA, PB = pyramids()
    want, ws = kp.track(PA, PB, pts, pts.copy(), photo=True)
    assert np.array_equal(gs, ws) and np.array_equal(raw(got), raw(want))


# ---- 4: the image loop --------------------------------------------------------------------------------------------------------------
def flicker_sequence(frames=8):
    seq = translated_sequence(fb.image("first"), frames, dx=-3.1, dy=-1.3)
    return [eq.contrast(img, 0.8, 0) if i % 2 else img for i, img in enumerate(seq)]


def step_image_loop(seq, photo):
    v = EKFVIO(max_features=64, klt_photometric=photo)
    rows = []
    try:
        for i, img in enumerate(seq):
            assert v.addFrame(5.0 + i / 30.0, img, K) == capi.OK, i
            if i == 0:
                assert len(v.replenishFeatures()) >= 48
            rows.append(v.tc_ekf.get_state())
    finally:
        v.tc_ekf.close()
    return rows


def test_image_loop_is_the_call_by_call_path_and_keeps_its_landmarks_through_a_flicker():
    """Eight frames of the translated plane, the odd ones at gain 0.8, 64 landmarks at most.  ekfvio_step_image with the term against a
    handle with the term driven call by call (process, push_frame, findNewFeaturePositions, updateWithFeaturePositions): the same bits
    behind every frame.  And against a twin without the term: fewer landmarks carry the delete flag at the end (measured on an MI355X: 5
    of 64 with the term, all 64 without; both counts are printed)."""
    seq = flicker_sequence()
    stamps = [5.0 + i / 30.0 for i in range(len(seq))]
    rows = step_image_loop(seq, True)
    b = EKFVIO(max_features=64, klt_photometric=True)
    try:
        for i, img in enumerate(seq):
            if i == 0:
                assert b.addFrame(stamps[0], img, K) == capi.OK
                b.replenishFeatures()
            else:
                b.tc_ekf.process(float(np.float32(stamps[i] - stamps[i - 1])))
                b.tracker.push_frame(img, K)
                z, R, p = b.tracker.findNewFeaturePositions()
                assert b.tc_ekf.updateWithFeaturePositions(z, R, p) == capi.OK, i
            sb = b.tc_ekf.get_state()
            for k in ("base_mu", "feat_mu", "last_klt", "del_flag", "Sigma"):
                assert rows[i][k].shape == sb[k].shape and np.array_equal(raw(rows[i][k]), raw(sb[k])), (i, k)
    finally:
        b.tc_ekf.close()
    twin = step_image_loop(seq, False)
    assert np.array_equal(raw(twin[0]["last_klt"]), raw(rows[0]["last_klt"]))  # the same landmarks to begin with
    with_term, without = int(rows[-1]["del_flag"].sum()), int(twin[-1]["del_flag"].sum())
    print("landmarks", len(rows[-1]["del_flag"]), "flagged at the end: with the term", with_term, "without", without,
          "per frame with", [int(r["del_flag"].sum()) for r in rows], "without", [int(r["del_flag"].sum()) for r in twin])
    assert with_term < without
