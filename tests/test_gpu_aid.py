"""The linear aiding measurement of the base state on the device (include/ekfvio.h, ekfvio_aid_update; ekf_vio_amd/csrc/aid.hip) against
its NumPy restatement (tests/_aid.py; what that is held to without a GPU: tests/test_aid_cpu.py).

 1. ekfvio_aid_update from set_state: the bits of the fp32 restatement -- mean, all of Sigma, d2 and the verdict -- and what _aid.hold asserts
    against the fp64 one, at n = 22, 25, 256, 259 (on and beside the 256-row workgroup edge) and with capacity above N behind a camera
    update; k = 1, 3, 6, selection, dense and quaternion-touching H, diagonal and full R, an exactly zero innovation.
 2. A rejected update, by the gate and by a non-positive pivot: every byte of the state stays, and it is counted.
 3. Buffer ownership: a camera update behind the aiding update gives the bits it gives on a fresh handle set to the same state.
 4. ekfvio_aid = ekfvio_process(dt) + ekfvio_aid_update; the first stamp only sets the time; a stamp that runs backwards is refused.
 5. What the entry points refuse, with nothing changed.
 6. The scale experiment (tests/_aid.py: experiment_inputs) through the device at D = 2.

Each handle is closed before the next is created (the persistent sweep is for a device's sole handle).
"""
import ctypes as C

import numpy as np
import pytest

from ekf_vio_amd import TightlyCoupledEKF, capi
from oracle import set_threads

import _aid as A
import _imu_cases as I
from test_aid_cpu import _p, refused_rows

pytestmark = pytest.mark.gpu

KEYS = ("base_mu", "feat_mu", "last_klt", "del_flag", "Sigma")


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    I.use_threads()
    yield
    set_threads(1)


def assert_same_bits(a, b, what):
    for key in KEYS:
        assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (what, key)


def bits(x):
    return np.float32(x).tobytes()


# ---- 1: the update alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap,camera_first", [(0, 0, False), (1, 1, False), (78, 78, False), (79, 79, False), (79, 256, True)],
                         ids=["n22", "n25", "n256", "n259", "n259-cap256-camera-first"])
def test_update_is_the_restatement_bit_for_bit_and_meets_the_criterion(N, cap, camera_first):
    st, frame = I.start(N)
    h = TightlyCoupledEKF(max_features=max(cap, 1))
    try:
        assert h.aid_status() == dict(d2_last=0.0, accepted_last=0, applied_total=0, rejected_total=0)
        applied = 0
        for name, (H, z, R) in A.measurement_cases(st).items():
            if camera_first:  # the borrowed Km / Gm / Wt hold a camera update's leftovers, and ld > n + 1
                h.set_state(st)
                h.process(I.DT)
                assert h.updateWithFeaturePositions(*frame) in (capi.OK, capi.ENUMERIC)
            h.set_state(st)
            h.aidUpdate(H, z, R)
            got, status = h.get_state(), h.aid_status()
            applied += 1
            assert h.dim == 22 + 3 * N and h.num_features == N
            k32, info = A.kernel_order_fp32(st, H, z, R)
            assert info["accepted"], name
            for key in ("base_mu", "feat_mu", "Sigma"):
                bad = np.argwhere(got[key] != k32[key])
                assert bad.shape[0] == 0, (N, name, key, bad.shape[0], "elements differ, the first at", bad[0])
            assert bits(status["d2_last"]) == bits(info["d2"]), (name, status, info["d2"])
            assert (status["accepted_last"], status["applied_total"], status["rejected_total"]) == (1, applied, 0), (name, status)
            # (the device equals the restatement in every bit, so this repeats the CPU test's verdict on purpose: it is the device's result that is held)
            A.hold("device N%d %s" % (N, name), got, st, H, z, R, exempt=A.exceptions(N, name))
            assert abs(np.linalg.norm(got["base_mu"][3:7].astype(np.float64)) - 1) < 1e-6
            assert np.array_equal(got["last_klt"], st["last_klt"]) and np.array_equal(got["del_flag"], st["del_flag"])
    finally:
        h.close()


# ---- 2: rejected ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 79], ids=["n25", "n259"])
def test_a_rejected_update_leaves_every_byte_and_is_counted(N):
    st = I.fresh(I.start(N)[0])
    H, R = A.selection([7, 8, 9]), np.array([4e-4] * 3, np.float32)
    z = (np.asarray(st["base_mu"], np.float32)[7:10] + np.float32(1.0)).astype(np.float32)
    _, info = A.kernel_order_fp32(st, H, z, R)
    d2 = float(info["d2"])
    below = float(np.nextafter(info["d2"], np.float32(0)))
    h = TightlyCoupledEKF(max_features=N)
    try:
        h.set_state(st)
        before = h.get_state()
        h.aidUpdate(H, z, R, chi2=below)  # d2 one ulp above the gate: rejected
        s = h.aid_status()
        assert_same_bits(h.get_state(), before, "gated")
        assert bits(s["d2_last"]) == bits(d2) and (s["accepted_last"], s["applied_total"], s["rejected_total"]) == (0, 0, 1), s
        h.aidUpdate(H, z, R, chi2=d2)     # d2 == chi2: accepted, and the restatement's bits
        s = h.aid_status()
        got = h.get_state()
        want, _ = A.kernel_order_fp32(st, H, z, R, chi2=d2)
        for key in ("base_mu", "feat_mu", "Sigma"):
            assert got[key].tobytes() == want[key].tobytes(), key
        assert (s["accepted_last"], s["applied_total"], s["rejected_total"]) == (1, 1, 1), s
        # a non-positive pivot: S(1,1) = Sigma(8,8) + R < 0 (R itself is positive definite: the host lets it through)
        neg = I.fresh(st)
        neg["Sigma"][8, 8] = np.float32(-1.0)
        _, info = A.kernel_order_fp32(neg, H, z, R)
        assert not info["pd"] and not info["accepted"]
        h.set_state(neg)
        before = h.get_state()
        h.aidUpdate(H, z, R)
        s = h.aid_status()
        assert_same_bits(h.get_state(), before, "pivot")
        assert np.isnan(s["d2_last"]) and (s["accepted_last"], s["applied_total"], s["rejected_total"]) == (0, 1, 2), s
        h.initializeBaseState()  # ekfvio_reset: the counts start over
        assert h.aid_status() == dict(d2_last=0.0, accepted_last=0, applied_total=0, rejected_total=0)
    finally:
        h.close()


# ---- 3: buffer ownership ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", [(79, 79), (30, 100)], ids=["n259", "n112-cap100"])
def test_camera_update_behind_the_aiding_update_is_a_fresh_handles(N, cap):
    st, frame = I.start(N)
    H, z, R = A.measurement_cases(st)["k6-dense-fullR"]
    h = TightlyCoupledEKF(max_features=cap)
    try:
        h.set_state(st)
        h.aidUpdate(H, z, R)
        behind = h.get_state()
        rc1 = h.updateWithFeaturePositions(*frame)
        one = h.get_state()
    finally:
        h.close()
    h = TightlyCoupledEKF(max_features=cap)
    try:
        h.set_state(behind)
        rc2 = h.updateWithFeaturePositions(*frame)
        two = h.get_state()
    finally:
        h.close()
    assert rc1 == rc2 and rc1 in (capi.OK, capi.ENUMERIC)
    assert_same_bits(one, two, "camera update behind the aiding update")
    assert one["Sigma"].tobytes() != behind["Sigma"].tobytes()


# ---- 4: ekfvio_aid ------------------------------------------------------------------------------------------------------------------------
def test_aid_is_process_then_update():
    N = 30
    st = I.fresh(I.start(N)[0])
    H, z, R = A.measurement_cases(st)["k3-body-velocity-lever"]
    t0, t1 = 5.0, 5.0 + 1.0 / 30.0
    dt = np.float32(np.float64(t1) - np.float64(t0))
    h = TightlyCoupledEKF(max_features=N)  # (use_imu = 0, the default: ekfvio_aid propagates whatever it says)
    try:
        assert h.cfg.use_imu == 0
        h.set_state(st)
        before = h.get_state()
        h.aid(t0, H, z, R)  # the first stamp only sets the time
        assert_same_bits(h.get_state(), before, "first stamp")
        assert h.aid_status()["applied_total"] == 0
        k, Hf, zf, Rf = TightlyCoupledEKF._aid_rows(H, z, R)
        assert h.lib.ekfvio_aid(h.h, t0 - 0.01, k, _p(Hf), _p(zf), _p(Rf), 0.0) == capi.EINVAL  # a stamp before the filter's time
        assert_same_bits(h.get_state(), before, "refused stamp")
        h.aid(t1, H, z, R)
        one, s1 = h.get_state(), h.aid_status()
        h.aid(t1, H, z, R)  # the same stamp again: process(0), then the update
        again = h.get_state()
    finally:
        h.close()
    h = TightlyCoupledEKF(max_features=N)
    try:
        h.set_state(st)
        h.process(float(dt))
        h.aidUpdate(H, z, R)
        two, s2 = h.get_state(), h.aid_status()
        h.process(0.0)
        h.aidUpdate(H, z, R)
        again2 = h.get_state()
    finally:
        h.close()
    assert_same_bits(one, two, "aid against process + aid_update")
    assert_same_bits(again, again2, "a second record on the same stamp")
    assert s1 == s2 and s1["applied_total"] == 1
    assert one["Sigma"].tobytes() != before["Sigma"].tobytes()


# ---- 5: refusals ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_rows_with_nothing_changed():
    f = np.float32
    h = TightlyCoupledEKF(max_features=4)
    try:
        before = h.get_state()
        for name, k, H, z, R, chi2 in refused_rows():
            a = [None if x is None else np.ascontiguousarray(x, f) for x in (H, z, R)]
            assert h.lib.ekfvio_aid_update(h.h, k, _p(a[0]), _p(a[1]), _p(a[2]), chi2) == capi.EINVAL, name
            assert h.lib.ekfvio_aid(h.h, 1.0, k, _p(a[0]), _p(a[1]), _p(a[2]), chi2) == capi.EINVAL, name
            if k != 0:  # (k = 0 turns the standing measurement off)
                assert h.lib.ekfvio_set_frame_aid(h.h, k, _p(a[0]), _p(a[1]), _p(a[2]), chi2) == capi.EINVAL, name
        assert h.lib.ekfvio_set_frame_aid(h.h, 0, None, None, None, -1.0) == capi.OK
        assert_same_bits(h.get_state(), before, "refused")
        assert h.aid_status() == dict(d2_last=0.0, accepted_last=0, applied_total=0, rejected_total=0)
        # (the refused ekfvio_aid calls did not set the filter's time either: this one is still the first stamp)
        H, z, R = np.ascontiguousarray(A.selection([9])), np.zeros(1, f), np.array([1e-2], f)
        assert h.lib.ekfvio_aid(h.h, 0.5, 1, _p(H), _p(z), _p(R), 0.0) == capi.OK
        assert_same_bits(h.get_state(), before, "first stamp")
    finally:
        h.close()


# ---- 6: the experiment ------------------------------------------------------------------------------------------------------------------
def test_scale_experiment_on_the_device():
    """tests/test_aid_cpu.py: test_scale_experiment at D = 2, N = 16, 150 frames, through the device: process, the aiding update with the
    measured body velocity, the camera update.  The same two conditions.  Measured on the MI355X: see the README's table."""
    D = 2.0
    uv0, recs, dt, truth = A.experiment_inputs(D)
    out = {}
    for mode in (None, "vel"):
        h = TightlyCoupledEKF(max_features=16)
        try:
            h.addNewFeatures(uv0)
            for z, R, p, v, d in recs:
                h.process(dt)
                if mode:
                    h.aidUpdate(*A.velocity_rows(v, mode, d))
                assert h.updateWithFeaturePositions(z, R, p) in (capi.OK, capi.ENUMERIC)
            st, status = h.get_state(), h.aid_status()
        finally:
            h.close()
        out[mode] = A.figures(st["base_mu"], st["feat_mu"], truth)
        print("\nAID-EXPERIMENT-DEVICE D=%g %s: position error %.3f of %.3f travelled (%.3f), median depth ratio %.3f; aiding updates applied %d, rejected %d, last d2 %.3g"
              % (D, mode or "no aiding", out[mode][0], out[mode][1], out[mode][0] / out[mode][1], out[mode][2], status["applied_total"],
                 status["rejected_total"], status["d2_last"]))
        assert status["applied_total"] == (len(recs) if mode else 0) and status["rejected_total"] == 0
    vel, off = out["vel"], out[None]
    assert vel[0] <= 0.1 * vel[1], vel
    assert 0.9 <= vel[2] <= 1.1, vel
    assert off[0] >= 0.5 * off[1], off


# ---- 7: the replay driver ---------------------------------------------------------------------------------------------------------------
def test_replay_driver_takes_aid_records_and_the_constraint(tmp_path):
    """ekfvio_replay --records with two `aid` records between three frames and --nhc-variance: the records reach ekfvio_aid through the C++ shim,
    the constraint runs in the two frames behind the first, and the driver reports the counts."""
    import os
    import re
    import subprocess
    from PIL import Image
    from ekf_vio_amd import _build
    from ekf_vio_amd.sim import translated_sequence
    exe = _build.build_host()
    base = np.asarray(Image.open(os.path.join(os.path.dirname(__file__), "golden", "images", "640_480_test_gray.png")))
    lines = []
    for i, img in enumerate(translated_sequence(base, 3, dx=-1.4, dy=-0.45)):
        with open(tmp_path / ("f%d.pgm" % i), "wb") as fh:
            fh.write(b"P5\n640 480\n255\n" + np.ascontiguousarray(img, np.uint8).tobytes())
        lines.append("image %.6f f%d.pgm 400 0 320 0 400 240 0 0 1" % (1.0 + i / 30.0, i))
        if i < 2:  # a forward-speed record half way to the next frame: k = 1, H = e_9, z = 0.3 m/s, R = 1e-2
            H = " ".join("1" if c == 9 else "0" for c in range(22))
            lines.append("aid %.6f 1 %s 0.3 0.01" % (1.0 + (i + 0.5) / 30.0, H))
    (tmp_path / "records.txt").write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, "--records", str(tmp_path), "--nhc-variance", "1e-3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    m = re.search(r"aid: (\d+) records applied to the filter, (\d+) skipped.*accepted (\d+), rejected (\d+)", out.stdout)
    assert m, out.stdout
    # (the first record propagates and updates: the first frame set the filter's time)
    assert [int(x) for x in m.groups()] == [2, 0, 4, 0], out.stdout
    odom = np.loadtxt(tmp_path / "odom.txt")
    assert odom.shape[0] == 3 and np.isfinite(odom).all()
    assert odom[2, 10] > 0.05  # v_z: the measured forward speed reached the state
    bad = tmp_path / "bad"
    bad.mkdir()
    (bad / "records.txt").write_text("aid 1.0 7 0 0\n")
    out = subprocess.run([exe, "--records", str(bad)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "aid needs a row count" in out.stderr
