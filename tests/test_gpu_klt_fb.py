"""The tracker's forward-backward check on the device (include/ekfvio.h, ekfvio_set_klt_fb): the backward pass runs in the tracker's
own launch and must give, bit for bit, what the CPU oracle's tracker gives when it is called a second time with the frames swapped
(tests/_klt_fb.py, restate_fb).  640 x 480 images, at most 256 points.
Handles that are compared run one after the other, each as the device's only live handle."""
import numpy as np
import pytest

from ekf_vio_amd import EKFVIO, KLTTracker, TightlyCoupledEKF, capi, EkfvioError

import _klt_fb as fb

pytestmark = pytest.mark.gpu
K = np.array([500.0, 0, 320.0, 0, 500.0, 240.0, 0, 0, 1.0], np.float32)
FLT_MAX = float(np.finfo(np.float32).max)
T0, T1 = 10.0, 10.0 + 1.0 / 30.0
DT = np.float32(np.float64(T1) - np.float64(T0))
STATE_KEYS = ("base_mu", "feat_mu", "last_klt", "del_flag", "Sigma")


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_fb_equal(got, ref, what):
    """(out_px, status, back_px, err2, fb_ok) of track_points_fb against the restatement, for every point, forward failures included."""
    out, st, back, e2, ok = got
    assert np.array_equal(st, ref["s_f"]), what
    assert np.array_equal(bits(out), bits(ref["q"])), (what, "out_px")
    assert np.array_equal(ok, ref["fb_ok"]), (what, "fb_ok", np.flatnonzero(ok != ref["fb_ok"]))
    assert np.array_equal(bits(e2), bits(ref["err2"])), (what, "err2", np.flatnonzero(bits(e2) != bits(ref["err2"])))
    assert np.array_equal(bits(back), bits(ref["back"])), (what, "back_px")


def tracker(second, shrink=1, max_features=256, **cfg):
    g = TightlyCoupledEKF(max_features=max_features, **cfg)
    t = KLTTracker(g)
    a, b = fb.image("first"), fb.image(second)
    if shrink > 1:
        a, b = np.ascontiguousarray(a[::shrink, ::shrink]), np.ascontiguousarray(b[::shrink, ::shrink])
    t.push_frame(a, K), t.push_frame(b, K)
    return g, t


# ---- 1-3: bit-exactness of the pixel-space form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset_guess", [False, True], ids=["guess=point", "guess=offset"])
@pytest.mark.parametrize("second", ["moved", "shear", "identical", "blocked"])
def test_track_points_fb_is_the_oracle_called_twice(second, offset_guess):
    pts, guess, ref = fb.reference(second, offset_guess, 0.5)
    g, t = tracker(second, klt_fb_max_px=0.5)
    got = t.track_points_fb(pts, guess)
    assert_fb_equal(got, ref, (second, offset_guess))
    # the forward pass is the plain entry point's, which stays what it was
    out, st = t.track_points(pts, guess)
    assert np.array_equal(st, got[1]) and np.array_equal(bits(out), bits(got[0]))
    assert g.klt_fb()["n_landmarks"] == 0  # the landmarks' results are not this call's
    g.close()


@pytest.mark.parametrize("win,levels,iters", [(3, 3, 30), (15, 2, 8), (21, 0, 3)])
def test_other_windows_levels_and_iteration_budgets(win, levels, iters):
    """The lane geometry changes with the window, and the second pass must follow it."""
    pts, guess, ref = fb.reference("blocked", True, 0.5, win=win, levels=levels, iters=iters)
    g, t = tracker("blocked", klt_window_size=win, klt_max_pyramid_level=levels, klt_max_iterations=iters, klt_fb_max_px=0.5)
    assert_fb_equal(t.track_points_fb(pts, guess), ref, (win, levels, iters))
    assert (ref["s_f"] == 1).sum() >= 100 and (ref["err2"] == -1).sum() >= 3
    g.close()


@pytest.mark.parametrize("offset_guess", [False, True], ids=["guess=point", "guess=offset"])
def test_small_image_where_the_level_count_reduces(offset_guess):
    assert fb.frame("first", shrink=4).levels == 3  # 160 x 120: level 3 would be 20 x 15, not larger than the window
    pts, guess, ref = fb.reference("moved", offset_guess, 0.5, shrink=4)
    g, t = tracker("moved", shrink=4, klt_fb_max_px=0.5)
    assert_fb_equal(t.track_points_fb(pts, guess), ref, "160x120")
    assert (ref["s_f"] == 1).sum() >= 50
    g.close()


# ---- 4: verdicts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset_guess", [False, True], ids=["guess=point", "guess=offset"])
def test_verdicts_at_half_a_pixel(offset_guess):
    """Every point whose true destination lies at least 11 px inside the pasted block is rejected or lost; on the plain pairs nothing
    the tracker kept is rejected.  No case is too close to call: the verdicts are the restatement's."""
    g, t = tracker("blocked", klt_fb_max_px=0.5)
    pts, guess, ref = fb.reference("blocked", offset_guess, 0.5)
    _, st, _, _, ok = t.track_points_fb(pts, guess)
    assert np.array_equal(ok, ref["fb_ok"]) and np.array_equal(st, ref["s_f"])
    inside = fb.inside_block(pts + np.array(fb.FLOW["blocked"]), 11)
    assert inside.sum() == 4 + 9  # the 8-grid's four and the 13-grid's nine (all among its first 150 points)
    assert not ((st[inside] == 1) & (ok[inside] == 1)).any()
    assert (st[inside] == 1).sum() >= inside.sum() - 1  # ... although the forward track kept (all but one of) them
    # threshold 0 on the same handle: the backward pass still runs, and fb_ok is its status alone
    g.setKltFb(0.0)
    assert_fb_equal(t.track_points_fb(pts, guess), fb.reference("blocked", offset_guess, 0.0)[2], "threshold 0")
    g.close()
    for second in ("moved", "identical"):
        g, t = tracker(second, klt_fb_max_px=0.5)
        pts, guess, ref = fb.reference(second, offset_guess, 0.5)
        _, st, _, _, ok = t.track_points_fb(pts, guess)
        assert np.array_equal(ok, ref["fb_ok"]) and np.array_equal(ok, st), second  # kept forward = kept by the check
        assert (st == 1).sum() >= 200
        g.close()


# ---- 5-8: the landmark path -------------------------------------------------------------------------------------------------------------
def metric(px):
    """Feature::pixel2Metric with the reference's K indexing quirk (cx = cy = 0), Feature.h:60-62."""
    return np.stack([px[:, 0] / K[0], px[:, 1] / K[4]], axis=1).astype(np.float32)


UV = metric(fb.grid_points(8))


def landmark_handle(second="blocked", **cfg):
    """64 landmarks from the 8-grid on the first image, the second image pushed and the state propagated: ready to track."""
    g, t = TightlyCoupledEKF(max_features=64, **cfg), None
    t = KLTTracker(g)
    t.push_frame(fb.image("first"), K)
    g.addNewFeatures(UV)
    t.push_frame(fb.image(second), K)
    g.process(DT)
    return g, t


def landmark_restatement(st, second="blocked", max_px=0.5):
    """What klt_track_kernel forms from the state (reference pixel from last_klt, guess from the predicted landmark), restated."""
    p = np.stack([st["last_klt"][:, 0] * K[0], st["last_klt"][:, 1] * K[4]], axis=1).astype(np.float32)
    gs = np.stack([K[0] * st["feat_mu"][:, 0], K[4] * st["feat_mu"][:, 1]], axis=1).astype(np.float32)
    r = fb.restate_fb(fb.frame("first"), fb.frame(second), p, gs, max_px)
    q, kp = r["q"], 11
    inside = ~((q[:, 0] < kp) | (q[:, 1] < kp) | (640 - q[:, 0] < kp) | (480 - q[:, 1] < kp))
    return r, ((r["s_f"] == 1) & (r["fb_ok"] == 1) & inside).astype(np.uint8)


@pytest.mark.parametrize("sample_based", [0, 1])
def test_landmark_path_treats_a_rejected_track_as_a_lost_one(sample_based):
    g0, t0 = landmark_handle(sample_based_uncertainty=sample_based)
    z0, R0, p0 = t0.findNewFeaturePositions()
    off = g0.klt_fb()
    assert off["n_landmarks"] == 0 and off["rejected_total"] == 0 and len(off["err2"]) == 0
    g0.close()
    g, t = landmark_handle(sample_based_uncertainty=sample_based, klt_fb_max_px=0.5)
    st = g.get_state()
    r, want_pass = landmark_restatement(st)
    rej = r["rejected"] == 1
    assert rej.sum() >= 8 and want_pass.sum() >= 40 and (r["s_f"] == 0).sum() >= 1
    z, R, p = t.findNewFeaturePositions()
    assert np.array_equal(p, want_pass) and np.array_equal(p, np.where(rej, 0, p0))
    assert np.array_equal(bits(z), bits(np.where(rej[:, None], np.float32(0), z0)))
    assert np.array_equal(bits(R.reshape(-1, 4)), bits(np.where(rej[:, None], np.float32(0), R0.reshape(-1, 4))))
    res = g.klt_fb()
    assert np.array_equal(bits(res["err2"]), bits(r["err2"])) and np.array_equal(res["rejected"], r["rejected"])
    assert (res["n_landmarks"], res["rejected_last"], res["rejected_total"]) == (64, int(rej.sum()), int(rej.sum()))
    t.findNewFeaturePositions()  # the same track again: the frame's count starts over, the total goes on
    res = g.klt_fb()
    assert (res["n_landmarks"], res["rejected_last"], res["rejected_total"]) == (64, int(rej.sum()), 2 * int(rej.sum()))
    assert np.array_equal(res["rejected"], r["rejected"])
    # the update's bookkeeping: delete flag set, last_klt kept, for the rejected as for the lost
    assert g.updateWithFeaturePositions(z, R, p) in (capi.OK, capi.ENUMERIC)
    s1 = g.get_state()
    assert np.array_equal(s1["del_flag"], st["del_flag"] | (p == 0))
    assert np.array_equal(bits(s1["last_klt"][p == 0]), bits(st["last_klt"][p == 0]))
    assert np.array_equal(bits(s1["last_klt"][p == 1]), bits(z[p == 1]))
    g.close()


def test_step_image_with_the_check_is_the_explicit_sequence():
    def step(**cfg):
        v = EKFVIO(max_features=64, klt_fb_max_px=0.5, **cfg)
        v.addFrame(T0, fb.image("first"), K)
        v.tc_ekf.addNewFeatures(UV)
        rc = v.addFrame(T1, fb.image("blocked"), K)
        out = rc, v.tc_ekf.get_state(), v.tc_ekf.klt_fb(), v.tc_ekf.num_features
        v.tc_ekf.close()
        return out
    rc_a, sa, fa, _ = step()
    w, t = landmark_handle(klt_fb_max_px=0.5)
    z, R, p = t.findNewFeaturePositions()
    rc_b = w.updateWithFeaturePositions(z, R, p)
    sb, fw = w.get_state(), w.klt_fb()
    w.close()
    assert rc_a == rc_b
    for k in STATE_KEYS:
        assert np.array_equal(sa[k], sb[k]), k
    assert fa["rejected_last"] == fw["rejected_last"] >= 8 and np.array_equal(fa["rejected"], fw["rejected"])
    assert np.array_equal(bits(fa["err2"]), bits(fw["err2"]))
    assert sa["del_flag"].sum() == 64 - int(p.sum())
    # with remove_lost = 1 the rejected landmarks leave the state in the same frame, with the lost ones
    _, _, fr, n_left = step(remove_lost=1)
    assert n_left == int(p.sum()) and np.array_equal(fr["rejected"], fw["rejected"])


def test_off_means_off():
    g0, t0 = landmark_handle()
    ref = t0.findNewFeaturePositions()
    g0.close()
    g, t = landmark_handle()
    g.setKltFb(0.5)
    g.setKltFb(0.0)
    got = t.findNewFeaturePositions()
    for a, b in zip(got, ref):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    for bad in (-1.0, float("nan")):
        with pytest.raises(EkfvioError) as e:
            g.setKltFb(bad)
        assert e.value.code == capi.EINVAL
        with pytest.raises(EkfvioError) as e:
            TightlyCoupledEKF(max_features=4, klt_fb_max_px=bad)
        assert e.value.code == capi.EINVAL
    g.close()

    def loop(toggle):
        v = EKFVIO(max_features=64)
        if toggle:
            v.tc_ekf.setKltFb(0.5), v.tc_ekf.setKltFb(0.0)
        v.addFrame(T0, fb.image("first"), K)
        v.tc_ekf.addNewFeatures(UV)
        v.addFrame(T1, fb.image("blocked"), K)
        st = v.tc_ekf.get_state()
        v.tc_ekf.close()
        return st
    sa, sb = loop(False), loop(True)
    for k in STATE_KEYS:
        assert np.array_equal(sa[k], sb[k]), k


def test_totals_restart_at_reset_and_the_threshold_stays():
    g, t = landmark_handle(klt_fb_max_px=0.5)
    t.findNewFeaturePositions()
    first = g.klt_fb()
    assert first["rejected_total"] == first["rejected_last"] >= 8
    g.initializeBaseState()
    res = g.klt_fb()
    assert (res["n_landmarks"], res["rejected_last"], res["rejected_total"]) == (0, 0, 0)
    t.push_frame(fb.image("first"), K)
    g.addNewFeatures(UV)
    t.push_frame(fb.image("blocked"), K)
    g.process(DT)
    t.findNewFeaturePositions()
    again = g.klt_fb()
    assert again["rejected_total"] == again["rejected_last"] == first["rejected_last"]  # the threshold stayed: the same verdicts
    assert np.array_equal(again["rejected"], first["rejected"])
    g.close()


def test_gate_and_check_together_count_nothing_twice():
    g, t = landmark_handle(klt_fb_max_px=0.5, gate_chi2=FLT_MAX)
    st = g.get_state()
    r, want_pass = landmark_restatement(st)
    z, R, p = t.findNewFeaturePositions()
    assert np.array_equal(p, want_pass)
    assert g.updateWithFeaturePositions(z, R, p) in (capi.OK, capi.ENUMERIC)
    gate, res = g.gate(), g.klt_fb()
    assert gate["n_landmarks"] == 64 and gate["gated_last"] == 0 and gate["gated_total"] == 0 and gate["gated"].sum() == 0
    assert np.array_equal(gate["d2"] == -1, p == 0)  # the gate never saw what the check (or the tracker) turned away
    assert (gate["d2"][r["rejected"] == 1] == -1).all() and (gate["d2"][p == 1] >= 0).all()
    assert res["rejected_last"] == int(r["rejected"].sum()) == res["rejected_total"]
    assert g.get_state()["del_flag"].sum() == 64 - int(p.sum())  # every landmark turned away is flagged once, by one of the two
    g.close()
