"""The zero-velocity update on the device (include/ekfvio.h, ekfvio_set_zupt; ekf_vio_amd/csrc/zupt.hip) against its NumPy restatements
(tests/_zupt.py; what they are held to without a GPU: tests/test_zupt_cpu.py).

 1. ekfvio_zupt_update from set_state: the bits of the fp32 restatement, and what _zupt.hold asserts against the fp64 one (an a-priori
    rounding bound per element; the criterion of tests/_imu_cases.py with a second, independent fp32 rounding order as its fp32 error, on
    every state but the one hold() names), at n = 22, 25, 256, 259, 532 (on and beside the 256-row workgroup edge), and with capacity above
    N behind a camera update.
 2. The device's decision through the test hook: the bits of ekfvio_zupt_decide, hence of the restatement.
 3. A still image loop: applied every tracked frame; 4. a moving one: never applied, every bit of a handle without the setting, and the
    reported flow that of the sequence (1.47 px a frame, real intrinsics); both with the gain kernel as one workgroup and as two.
 5. the setting: off, invalid, across a reset, on a fresh handle.

Each handle is closed before the next is created (the persistent sweep is for a device's sole handle).
"""
import ctypes as C
import os

import numpy as np
import pytest
from PIL import Image

from ekf_vio_amd import EKFVIO, TightlyCoupledEKF, capi
from ekf_vio_amd.sim import translated_sequence
from oracle import set_threads

import _imu_cases as I
import _zupt as Z
from test_zupt_cpu import assert_decision, edge_cases, host_decide, random_case

pytestmark = pytest.mark.gpu

K = np.array([500.0, 0, 320.0, 0, 500.0, 240.0, 0, 0, 1.0], np.float32)
KEYS = ("base_mu", "feat_mu", "last_klt", "del_flag", "Sigma")
SETTING = (0.25, 8, 0.75, 1e-4, 1e-4)
NODE = dict(max_features=64, replenish=1, fast_threshold=20, min_new_feature_dist=12)
VAR = (1e-4, 1e-4)


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    I.use_threads()
    yield
    set_threads(1)


def fixture_frame():
    return np.ascontiguousarray(np.asarray(Image.open(os.path.join(os.path.dirname(__file__), "golden", "images", "640_480_test_gray.png"))), np.uint8)


def assert_same_bits(a, b, what):
    for key in KEYS:
        assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (what, key)


# ---- 1: the update alone ----------------------------------------------------------------------------------------------------------------
def run_update(N, cap, camera_first):
    st, frame = I.start(N)
    h = TightlyCoupledEKF(max_features=max(cap, 1))
    try:
        if camera_first:  # the borrowed Km / Gm / Wt hold a camera update's leftovers, and ld > n + 1
            h.set_state(st)
            h.process(I.DT)
            assert h.updateWithFeaturePositions(*frame) in (capi.OK, capi.ENUMERIC)
        h.set_state(st)
        h.zuptUpdate(*VAR)
        got = h.get_state()
        assert h.dim == 22 + 3 * N and h.num_features == N
    finally:
        h.close()
    return st, got


@pytest.mark.parametrize("N,cap,camera_first", [(0, 0, False), (1, 1, False), (78, 78, False), (79, 79, False), (170, 170, False), (79, 256, True)],
                         ids=["n22", "n25", "n256", "n259", "n532", "n259-cap256-camera-first"])
def test_update_is_the_restatement_bit_for_bit_and_meets_the_criterion(N, cap, camera_first):
    st, got = run_update(N, cap, camera_first)
    k32 = Z.kernel_order_fp32(st, *VAR)
    for key in ("base_mu", "feat_mu", "Sigma"):
        bad = np.argwhere(got[key] != k32[key])
        assert bad.shape[0] == 0, (N, key, bad.shape[0], "elements differ, the first at", bad[0])
    # (the device equals the restatement in every bit, so this repeats the CPU test's verdict on purpose: it is the device's result that is held)
    Z.hold("device N%d" % N, got, st, *VAR)
    t = I.tolerances(*Z.reference(st, *VAR))
    assert abs(np.linalg.norm(got["base_mu"][3:7].astype(np.float64)) - 1) < 1e-6
    assert np.array_equal(got["last_klt"], st["last_klt"]) and np.array_equal(got["del_flag"], st["del_flag"])
    Rd = np.array([np.float32(VAR[0])] * 3 + [np.float32(VAR[1])] * 3, np.float64)
    after, before = np.diag(got["Sigma"]).astype(np.float64)[7:13], np.diag(st["Sigma"]).astype(np.float64)[7:13]
    assert (after <= np.minimum(before, Rd) + t["sig_elementwise"]).all() and (after > 0).all(), (after, before)


def test_update_refuses_bad_variances():
    h = TightlyCoupledEKF(max_features=4)
    try:
        before = h.get_state()
        for vv, ov in ((0.0, 1e-4), (1e-4, -1.0), (float("nan"), 1e-4), (1e-4, float("inf"))):
            assert h.lib.ekfvio_zupt_update(h.h, vv, ov) == capi.EINVAL
        assert_same_bits(h.get_state(), before, "refused")
    finally:
        h.close()


# ---- 2: the decision on the device ------------------------------------------------------------------------------------------------------
def test_device_decision_is_the_host_functions_bit_for_bit():
    h = TightlyCoupledEKF(max_features=1024, hooks=True)
    try:
        fn = h.lib.ekfvio_test_zupt_decide
        verdicts = set()
        for count in (1, 63, 64, 65, 1024):
            for seed in range(2):
                prev, cur, ok, mf, mt, mr = random_case(count, seed)
                for ratio in (mr, 0.9):
                    want = host_decide(prev, cur, ok, mf, mt, ratio)
                    assert_decision(want, Z.decide(prev, cur, ok, mf, mt, ratio), ("host", count, seed))
                    assert_decision(host_decide(prev, cur, ok, mf, mt, ratio, fn=fn, handle=h.h), want, ("device", count, seed, ratio))
                    verdicts.add(want[3])
        assert verdicts == {0, 1}
        for name, prev, cur, ok, mf, mt, mr, expected in edge_cases():
            got = host_decide(prev, cur, ok, mf, mt, mr, fn=fn, handle=h.h)
            assert_decision(got, host_decide(prev, cur, ok, mf, mt, mr), name)
            assert got[1:] == expected, (name, got[1:], expected)
        z = np.zeros(2, np.float32).ctypes.data_as(C.POINTER(C.c_float))
        one = np.ones(1, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
        assert fn(h.h, z, z, one, 1025, 0.25, 1, 0.75, None, None, None, None) == capi.ECAPACITY
        assert fn(h.h, z, z, one, 1, 0.0, 1, 0.75, None, None, None, None) == capi.EINVAL
    finally:
        h.close()


# ---- 3-5: the frame loop ----------------------------------------------------------------------------------------------------------------
def run_loop(frames, zupt=None, before=None, each=None, max_features=64):
    """The frames through a node of its own; before(v): settings in front of the first frame; each(v, i): after frame i.  Returns the final
    state and the last zupt() report."""
    v = EKFVIO(zupt=zupt, **dict(NODE, max_features=max_features))
    try:
        if before:
            before(v)
        for i, img in enumerate(frames):
            assert v.addFrame(3.0 + i / 30.0, img, K) in (capi.OK, capi.ENUMERIC)
            if each:
                each(v, i)
        st = v.tc_ekf.get_state()
        st["ids"] = v.landmark_ids()[0]
        return st, v.zupt()
    finally:
        v.tc_ekf.close()


@pytest.mark.parametrize("cap", [64, 128], ids=["one-workgroup", "two-workgroups"])
def test_still_loop_applies_every_tracked_frame(cap):
    """cap = 128: n = 22 + 3 N > 256, so the gain kernel runs as two workgroups, each decides for itself and workgroup 0 alone publishes."""
    frames = [fixture_frame()] * 6
    seen = []

    def each(v, i):
        z = v.zupt()
        seen.append(z)
        if i == 0:
            assert (z["n_landmarks"], z["n_pass"], z["applied_last"], z["applied_total"]) == (0, 0, 0, 0)  # the first frame tracks nothing
            return
        assert z["n_still"] == z["n_pass"] >= 8 and z["applied_last"] == 1 and z["applied_total"] == i, (i, z)
        assert z["n_landmarks"] == z["flow2"].shape[0] >= z["n_pass"]
        passed = z["flow2"] >= 0
        assert passed.sum() == z["n_pass"] and (z["flow2"][passed] <= np.float32(0.25) ** 2).all() and (z["flow2"][~passed] == -1).all()
        print("ZUPT-STILL cap %d frame %d: landmarks %d, largest squared flow %.3g" % (cap, i, z["n_landmarks"], float(z["flow2"].max())))
        # identical frames: the guess is the reference pixel, diff = 0, so b = 0 and the track does not move -- exactly zero flow, which also
        # says the reference pixel is formed as the tracker forms it (measured on the MI355X: 0 in every frame at both sizes)
        assert (z["flow2"][passed] == 0).all(), (i, z["flow2"][passed].max())
        if cap > 64:
            assert z["n_landmarks"] > 78, z["n_landmarks"]  # n > 256: more than one workgroup

    on, z = run_loop(frames, zupt=SETTING, each=each, max_features=cap)
    assert z["applied_total"] == 5
    d = np.diag(on["Sigma"]).astype(np.float64)[7:13]
    print("\nZUPT-STILL diag[7:13] on:", d)
    assert (d <= 1e-4 * (1 + 2.0 ** -20)).all(), d
    off, z_off = run_loop(frames, max_features=cap)
    assert z_off["applied_total"] == 0 and z_off["n_landmarks"] == 0
    tr_on, tr_off = float(np.trace(on["Sigma"][7:13, 7:13].astype(np.float64))), float(np.trace(off["Sigma"][7:13, 7:13].astype(np.float64)))
    print("ZUPT-STILL trace Sigma[7:13, 7:13] on / off: %.6g / %.6g" % (tr_on, tr_off))
    assert tr_off > tr_on


@pytest.mark.parametrize("cap", [64, 128], ids=["one-workgroup", "two-workgroups"])
def test_moving_loop_never_applies_and_keeps_every_bit(cap):
    frames = translated_sequence(fixture_frame(), 6)  # 1.47 px per frame

    def each(v, i):
        z = v.zupt()
        if i > 0:
            assert z["n_pass"] >= 8 and z["applied_last"] == 0 and z["n_still"] < 0.75 * z["n_pass"], (i, z)
            passed = z["flow2"] >= 0
            # 1.47 px a frame: the passed landmarks' squared flow lies around 2.16 (the reference pixel and the tracked one, real intrinsics),
            # far from the threshold's 0.0625; a few tracks may have converged elsewhere
            f2 = z["flow2"][passed]
            print("ZUPT-MOVING cap %d frame %d: landmarks %d, squared flow median %.3f min %.3f max %.3f" % (cap, i, z["n_landmarks"], np.median(f2), f2.min(), f2.max()))
            assert passed.sum() == z["n_pass"] and 1.8 < float(np.median(f2)) < 2.6 and ((f2 > 1.0) & (f2 < 4.0)).mean() >= 0.9, (i, f2)
            if cap > 64:
                assert z["n_landmarks"] > 78, z["n_landmarks"]

    on, z = run_loop(frames, zupt=SETTING, each=each, max_features=cap)
    assert z["applied_total"] == 0
    off, _ = run_loop(frames, max_features=cap)
    for key in KEYS + ("ids",):
        assert on[key].shape == off[key].shape and on[key].tobytes() == off[key].tobytes(), key
    # set and turned off again: the bits of a handle that was never set (the other arguments are not looked at)
    if cap > 64:
        return
    cleared, zc = run_loop(frames, before=lambda v: (v.setZupt(*SETTING), v.tc_ekf._chk(v.tc_ekf.lib.ekfvio_set_zupt(v.tc_ekf.h, 0.0, -7, float("nan"), -1.0, 0.0))))
    assert zc["applied_total"] == 0 and zc["n_landmarks"] == 0
    for key in KEYS + ("ids",):
        assert cleared[key].tobytes() == off[key].tobytes(), key


def test_setting_invalid_arguments_reset_and_fresh_handle():
    v = EKFVIO(**NODE)
    try:
        g, lib = v.tc_ekf, v.tc_ekf.lib
        z = v.zupt()
        assert (z["n_landmarks"], z["n_pass"], z["n_still"], z["applied_last"], z["applied_total"]) == (0, 0, 0, 0, 0) and z["flow2"].size == 0
        assert lib.ekfvio_get_zupt(g.h, None, None, None, None, None, None) == capi.OK  # any pointer may be NULL
        v.setZupt(*SETTING)
        for bad in ((-0.25, 8, 0.75, 1e-4, 1e-4), (float("nan"), 8, 0.75, 1e-4, 1e-4), (float("inf"), 8, 0.75, 1e-4, 1e-4), (0.25, 0, 0.75, 1e-4, 1e-4),
                    (0.25, 8, 0.0, 1e-4, 1e-4), (0.25, 8, 1.25, 1e-4, 1e-4), (0.25, 8, 0.75, 0.0, 1e-4), (0.25, 8, 0.75, 1e-4, float("nan")),
                    (1e6, 1000, 0.75, -1.0, 1e-4)):
            assert lib.ekfvio_set_zupt(g.h, *bad) == capi.EINVAL, bad
        img = fixture_frame()
        for i in range(3):  # the setting is what it was: a still loop applies
            v.addFrame(1.0 + i / 30.0, img, K)
        z = v.zupt()
        assert z["applied_last"] == 1 and z["applied_total"] == 2 and z["n_still"] == z["n_pass"] >= 8
        g.initializeBaseState()  # the setting survives, the counts start over
        z = v.zupt()
        assert (z["n_landmarks"], z["applied_last"], z["applied_total"]) == (0, 0, 0)
        for i in range(3):
            v.addFrame(5.0 + i / 30.0, img, K)
        z = v.zupt()
        assert z["applied_last"] == 1 and z["applied_total"] == 2
    finally:
        v.tc_ekf.close()
