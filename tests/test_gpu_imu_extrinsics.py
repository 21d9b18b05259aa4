"""The IMU update with the IMU in its own frame (imu_gain_kernel<true>: ekf_vio_amd/csrc/imu.hip, imu_model.h) and gravity at run time, on the
device (cases, restatements and criterion: tests/_imu_extrinsics.py; what the cases can see: tests/test_imu_extrinsics_cpu.py).

Per case one teacher-forced update on a handle of its own (set_state, setImuExtrinsics, imuUpdate, get_state): the mean and all of Sigma
equal kernel_order_fp32_ext in every bit, and the criterion of _imu_cases holds against the fp64 evaluation with a numeric Jacobian.  Then:
off means off (a handle that set and cleared the extrinsics gives the bits of one that never set them), the setting survives ekfvio_reset,
is read back, and a refused matrix leaves the previous one in force; ekfvio_imu with a stamp and EKFVIO.imu_callback in front of a frame take
the same instance; nothing is left behind for the camera update; ekfvio_set_gravity equals a handle created with that gravity; and the
host class's gravity alignment.

Each handle is closed before the next is created (the persistent sweep is for a device's sole handle).

MEASURED ON THE MI355X: the kernels' results equalled kernel_order_fp32_ext's in every bit of every case (mean and all of Sigma, up to
n = 1222); err / tolerance of the criterion is at most 0.25 on every quantity from N = 30 on and at N = 0, and 0.87 at N = 1 (landmark block
of Sigma: the second fp32 order's own error is small there) -- the figures of the restatement on the CPU, as the bits are the same.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from ekf_vio_amd import EKFVIO, TightlyCoupledEKF, capi
from oracle import set_threads

import _imu_cases as I
import _imu_extrinsics as X

pytestmark = pytest.mark.gpu

KEYS = ("base_mu", "feat_mu", "last_klt", "del_flag", "Sigma")


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    I.use_threads()
    yield
    set_threads(1)


def handle(cap, g, gv, av, cls=TightlyCoupledEKF, **kw):
    return cls(max_features=max(cap, 1), use_imu=1, gravity=[float(x) for x in g], imu_gyro_variance=float(gv), imu_accel_variance=float(av), **kw)


def camera_step(h, frame):
    z, R, p = frame
    h.process(I.DT)
    rc = h.updateWithFeaturePositions(z, R, p)
    assert rc in (capi.OK, capi.ENUMERIC)
    return rc


def assert_same_bits(a, b, what):
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), (what, key, int(np.count_nonzero(a[key] != b[key])), "elements differ")


def assert_restatement_bits(got, k32, what):
    for key in ("base_mu", "feat_mu", "Sigma"):
        bad = np.argwhere(got[key] != k32[key])
        assert bad.shape[0] == 0, (what, key, bad.shape[0], "elements differ, the first at", bad[0])


@functools.lru_cache(maxsize=None)
def run_case(case):
    st, gyro, acc, gv, av, g, R, p = X.inputs(case)
    h = handle(case.cap, g, gv, av)
    try:
        if case.camera_first:  # the borrowed buffers hold a camera update's leftovers, and ld > n + 1
            st0, frame = I.start(case.N)
            h.set_state(st0)
            camera_step(h, frame)
        h.set_state(st)
        h.setImuExtrinsics(R, p)
        h.imuUpdate(gyro, acc)
        got = h.get_state()
        assert h.dim == 22 + 3 * case.N and h.num_features == case.N
    finally:
        h.close()
    return got


@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_the_device_computes_the_restatement_bit_for_bit(case):
    st, gyro, acc, gv, av, g, R, p = X.inputs(case)
    got = run_case(case)
    assert_restatement_bits(got, X.kernel_order_fp32_ext(st, gyro, acc, gv, av, g, R, p), X.case_id(case))
    assert np.array_equal(got["last_klt"], st["last_klt"]) and np.array_equal(got["del_flag"], st["del_flag"])


@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_the_device_meets_the_criterion_against_fp64(case):
    s32, s64 = X.reference(case)
    got = run_case(case)
    for key in ("base_mu", "feat_mu", "Sigma"):
        assert np.isfinite(got[key]).all(), key
    r = I.ratios(got, s32, s64)
    print("\nIMU-EXT-RATIO %s: %s" % (X.case_id(case), "  ".join("%s %.3f" % kv for kv in r.items())))
    assert abs(np.linalg.norm(got["base_mu"][3:7].astype(np.float64)) - 1) < 1e-6
    e, t = I.errors(got, s64), I.tolerances(s32, s64)
    for key in I.QUANTITIES:
        assert e[key] <= t[key], (key, "error", e[key], "allowed", t[key], "second fp32 order", I.errors(s32, s64)[key])


# ---------------------------------------------------------------------------------------------------------------- off means off
OFF_CASES = [I.Case("attitude", 30, 30, "1.03u", "ggen", "noise", I.DEFAULT_VAR, False), I.Case("size", 79, 79, "1.03u", "ggen", "noise", I.DEFAULT_VAR, False)]


@pytest.mark.parametrize("case", OFF_CASES, ids=I.case_id)
def test_set_then_cleared_is_never_set(case):
    st, gyro, acc, gv, av, g = I.inputs(case)
    R, p = X.ext32("generic-p")
    out = []
    for touch in (False, True):
        h = handle(case.cap, g, gv, av)
        try:
            h.set_state(st)
            if touch:
                h.setImuExtrinsics(R, p)
                assert h.imuExtrinsics()[2]
                h.setImuExtrinsics(None, None)
            Rg, pg, on = h.imuExtrinsics()
            assert not on and np.array_equal(Rg, np.eye(3, dtype=np.float32)) and not pg.any()
            h.imuUpdate(gyro, acc)
            out.append(h.get_state())
        finally:
            h.close()
    assert_same_bits(out[0], out[1], "extrinsics set and cleared against never set")
    assert_restatement_bits(out[1], I.kernel_order_fp32(st, gyro, acc, gv, av, g), "off")


def test_the_setting_is_read_back_survives_reset_and_a_refused_matrix_changes_nothing():
    case = X.CASES[3]  # the generic rotation with the lever arm
    st, gyro, acc, gv, av, g, R, p = X.inputs(case)
    want = X.kernel_order_fp32_ext(st, gyro, acc, gv, av, g, R, p)
    h = handle(case.cap, g, gv, av)
    try:
        h.setImuExtrinsics(R, p)
        Rg, pg, on = h.imuExtrinsics()
        assert on and np.array_equal(Rg, R) and np.array_equal(pg, p)  # as given, not re-orthonormalised
        h.initializeBaseState()  # ekfvio_reset
        Rg, pg, on = h.imuExtrinsics()
        assert on and np.array_equal(Rg, R) and np.array_equal(pg, p)
        nan = R.copy()
        nan[2, 0] = np.nan
        for bad_R, bad_p in ((R * np.float32(1.01), p), (R * np.array([1, -1, 1], np.float32), p), (nan, p), (R, None), (None, p)):
            with pytest.raises(capi.EkfvioError) as ex:
                h.setImuExtrinsics(bad_R, bad_p)
            assert ex.value.code == capi.EINVAL
        with pytest.raises(capi.EkfvioError) as ex:
            h.setGravity([0.0, np.inf, 0.0])
        assert ex.value.code == capi.EINVAL
        assert np.array_equal(h.gravity(), g)
        Rg, pg, on = h.imuExtrinsics()
        assert on and np.array_equal(Rg, R) and np.array_equal(pg, p)
        h.set_state(st)
        h.imuUpdate(gyro, acc)
        got = h.get_state()
    finally:
        h.close()
    assert_restatement_bits(got, want, "behind a reset and five refused settings")


# ---------------------------------------------------------------------------------------------------------------- every way in
def test_a_stamped_record_and_the_callback_take_the_same_instance():
    """ekfvio_imu with a stamp (process(dt) + update) and EKFVIO.imu_callback drained by imu records in stamp order give the bits of process(dt)
    followed by imuUpdate on a twin handle."""
    case = X.CASES[3]
    st, gyro, acc, gv, av, g, R, p = X.inputs(case)
    twin = handle(case.cap, g, gv, av, imu_extrinsics=(R, p))
    try:
        twin.set_state(st)
        twin.process(np.float32(1.005 - 1.000))
        twin.imuUpdate(gyro, acc)
        want = twin.get_state()
    finally:
        twin.close()
    assert not np.array_equal(want["Sigma"], st["Sigma"])
    v = handle(case.cap, g, gv, av, cls=EKFVIO, imu_extrinsics=(R, p))
    try:
        v.tc_ekf.set_state(st)
        v.imu_now(1.000, gyro, acc)  # the first record only sets the filter's clock
        assert_same_bits(v.tc_ekf.get_state(), st, "the first record")
        v.imu_now(1.005, gyro, acc)
        got = v.tc_ekf.get_state()
    finally:
        v.tc_ekf.close()
    assert_same_bits(got, want, "ekfvio_imu with a stamp against process + imuUpdate")
    v = handle(case.cap, g, gv, av, cls=EKFVIO, imu_extrinsics=(R, p))
    try:
        v.tc_ekf.set_state(st)
        v.imu_callback(1.005, gyro, acc)  # out of order on purpose: the queue sorts
        v.imu_callback(1.000, gyro, acc)
        assert_same_bits(v.tc_ekf.get_state(), st, "queued records")
        v._drain_imu(1.005)  # what addFrame does in front of the frame itself
        got = v.tc_ekf.get_state()
    finally:
        v.tc_ekf.close()
    assert_same_bits(got, want, "imu_callback in front of a frame against process + imuUpdate")


def test_imu_update_with_extrinsics_leaves_nothing_behind_for_the_camera_update():
    """Handle A: set_state, imuUpdate, get_state (S), process, camera update.  Handle B: set_state(S), process, camera update.  Same bits."""
    N = 30
    st0, frame = I.start(N)
    _, gyro, acc, gv, av, g, R, p = X.inputs(X.Case("size", N, N, "identity", "ggen", "noise", "generic-p", False))
    a = handle(N, g, gv, av, imu_extrinsics=(R, p))
    try:
        a.set_state(st0)
        a.imuUpdate(gyro, acc)
        S = a.get_state()
        rc_a = camera_step(a, frame)
        fa = a.get_state()
    finally:
        a.close()
    assert not np.array_equal(S["Sigma"], st0["Sigma"])
    b = handle(N, g, gv, av, imu_extrinsics=(R, p))
    try:
        b.set_state(S)
        rc_b = camera_step(b, frame)
        fb = b.get_state()
    finally:
        b.close()
    assert rc_a == rc_b
    assert_same_bits(fa, fb, "camera update behind an IMU update with extrinsics against the same from set_state")


# ---------------------------------------------------------------------------------------------------------------- gravity
def test_set_gravity_is_a_handle_created_with_that_gravity():
    case = X.CASES[3]
    st, gyro, acc, gv, av, g2, R, p = X.inputs(case)
    g1 = np.array(I.GRAVS["gy"], np.float32)
    out = []
    for created, later in ((g2, None), (g1, g2)):
        h = handle(case.cap, created, gv, av, imu_extrinsics=(R, p))
        try:
            assert np.array_equal(h.gravity(), created)
            if later is not None:
                h.setGravity(later)
                h.initializeBaseState()  # survives ekfvio_reset
                assert np.array_equal(h.gravity(), later)
            h.set_state(st)
            h.imuUpdate(gyro, acc)
            out.append(h.get_state())
        finally:
            h.close()
    assert_same_bits(out[0], out[1], "ekfvio_set_gravity(g2) on a handle created with g1 against a handle created with g2")
    assert_restatement_bits(out[1], X.kernel_order_fp32_ext(st, gyro, acc, gv, av, g2, R, p), "set gravity")


def test_gravity_alignment_swallows_its_records_and_sets_gravity():
    case = X.CASES[2]  # the permutation with the lever arm
    st, gyro, acc, gv, av, g, R, p = X.inputs(case)
    rng = np.random.default_rng(9)
    # a rig at rest, pitched: what its accelerometer reads, in IMU axes, with noise
    g_cam = X.axis_angle((1, 0, 0), 20.0) @ np.array([0.0, 9.81, 0.0])
    recs = [(R.astype(np.float64).T @ (-g_cam) + rng.normal(0, 0.05, 3)).astype(np.float32) for _ in range(4)]
    v = handle(case.cap, g, gv, av, cls=EKFVIO, imu_extrinsics=(R, p), gravity_align_samples=4)
    e = v.tc_ekf
    try:
        e.set_state(st)
        for k, a in enumerate(recs):
            assert np.array_equal(e.gravity(), g)
            v.imu_now(1.000 + 0.005 * k, gyro, a)
            assert_same_bits(e.get_state(), st, "swallowed record %d" % k)
        total = np.zeros(3, np.float64)
        for a in recs:
            total += a.astype(np.float64)
        mean = np.ascontiguousarray(total / 4)
        want_g = np.zeros(3, np.float32)
        mag = float(np.linalg.norm(g.astype(np.float64)))
        assert e.lib.ekfvio_gravity_from_accel(R.ctypes.data_as(C.POINTER(C.c_float)), mean.ctypes.data_as(C.POINTER(C.c_double)), mag,
                                               want_g.ctypes.data_as(C.POINTER(C.c_float))) == capi.OK
        got_g = e.gravity()
        assert np.array_equal(got_g, want_g) and np.abs(got_g - g_cam).max() < 0.2, (got_g, want_g, g_cam)
        v.imu_now(1.025, gyro, acc)  # the fifth record: process(1.025 - 1.000) and the update, with the aligned gravity
        got = e.get_state()
    finally:
        e.close()
    twin = handle(case.cap, want_g, gv, av, imu_extrinsics=(R, p))
    try:
        twin.set_state(st)
        twin.process(np.float32(1.025 - 1.000))
        twin.imuUpdate(gyro, acc)
        want = twin.get_state()
    finally:
        twin.close()
    assert not np.array_equal(want["Sigma"], st["Sigma"])
    assert_same_bits(got, want, "the fifth record against process + imuUpdate on a handle created with the aligned gravity")
