"""The IMU measurement update (imu_gain_kernel, imu_joseph_kernel: ekf_vio_amd/csrc/imu.hip) against its specification away from the identity
attitude (cases and criterion: tests/_imu_cases.py; what the cases can see: tests/test_imu_cases_cpu.py).

tests/test_gpu_imu.py runs near q = (1, 0, 0, 0) with gravity along the rotation axis, where the d/dw and d/dy columns and the e_k x uv term
of the accelerometer rows of H vanish, with floors some 200 x the arithmetic and one Frobenius norm over all of Sigma.  Here, per case: one
teacher-forced update (set_state, imuUpdate, get_state) on a handle of its own, held per quantity -- base mean, landmark means, Sigma's
quaternion rows, its base / base x landmark / landmark blocks, Sigma elementwise -- to

    err(HIP, fp64 oracle) <= 4 x err(fp32 oracle, fp64 oracle) + 2^-23 x scale

over seven attitudes x three gravities, n = 22 + 3 N on and beside the 256-row workgroup edge, handles whose capacity exceeds N with a
camera update's leftovers in the borrowed Km / Gm / Wt buffers, a large and an exactly-zero innovation, and three other variance pairs.
The kernels' results are also held bit for bit to a numpy fp32 restatement of their order of operations, which the CPU test holds to the same
criterion.  Then: the IMU update leaves nothing behind for the camera update that follows it (and the other way round), bit for bit, in three update
flows; and ekfvio_imu with two records on one stamp (dt = 0).

Each handle is closed before the next is created (the persistent sweep is for a device's sole handle).
"""
import functools

import numpy as np
import pytest

from ekf_vio_amd import EKFVIO, TightlyCoupledEKF, capi
from oracle import OracleFilter, set_threads

import _imu_cases as I

pytestmark = pytest.mark.gpu

KEYS = ("base_mu", "feat_mu", "last_klt", "del_flag", "Sigma")


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    I.use_threads()
    yield
    set_threads(1)


def handle(cap, g, gv, av, cls=TightlyCoupledEKF):
    return cls(max_features=max(cap, 1), use_imu=1, gravity=[float(x) for x in g], imu_gyro_variance=float(gv), imu_accel_variance=float(av))


def camera_step(h, frame):
    """process(dt) and a camera update of every landmark; returns the return code and what the counters say ran: (rc, persistent, t2_updates)."""
    z, R, p = frame
    c0 = h.counters()
    h.process(I.DT)
    rc = h.updateWithFeaturePositions(z, R, p)
    assert rc in (capi.OK, capi.ENUMERIC)
    c1 = h.counters()
    return rc, c1["persistent"] - c0["persistent"], c1["t2_updates"] - c0["t2_updates"]


def assert_same_bits(a, b, what):
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), (what, key, int(np.count_nonzero(a[key] != b[key])), "elements differ")


def hold(what, got, s32, s64):
    """The criterion of _imu_cases for one result; prints each figure before it asserts."""
    for key in ("base_mu", "feat_mu", "Sigma"):
        assert np.isfinite(got[key]).all(), (what, key)
    r = I.ratios(got, s32, s64)
    print("\nIMU-RATIO %s: %s" % (what, "  ".join("%s %.3f" % kv for kv in r.items())))
    assert abs(np.linalg.norm(got["base_mu"][3:7].astype(np.float64)) - 1) < 1e-6, what
    e, t = I.errors(got, s64), I.tolerances(s32, s64)
    for key in I.QUANTITIES:
        assert e[key] <= t[key], (what, key, "error", e[key], "allowed", t[key], "fp32 oracle", I.errors(s32, s64)[key])
    return r


@functools.lru_cache(maxsize=None)
def run_case(case):
    """set_state, imuUpdate, get_state on a handle of the case's own."""
    st, gyro, acc, gv, av, g = I.inputs(case)
    h = handle(case.cap, g, gv, av)
    try:
        if case.camera_first:  # the borrowed buffers hold a camera update's leftovers, and ld > n + 1
            st0, frame = I.start(case.N)
            h.set_state(st0)
            camera_step(h, frame)
        h.set_state(st)
        h.imuUpdate(gyro, acc)
        got = h.get_state()
        assert h.dim == 22 + 3 * case.N and h.num_features == case.N
    finally:
        h.close()
    return got


@pytest.mark.parametrize("case", I.CASES, ids=I.case_id)
def test_imu_update_against_the_fp64_oracle(case):
    st, gyro, acc, gv, av, g = I.inputs(case)
    s32, s64 = I.reference(case)
    got = run_case(case)
    hold(I.case_id(case), got, s32, s64)
    # what the specification leaves alone: the bookkeeping; with no landmark, that there is none
    assert np.array_equal(got["last_klt"], st["last_klt"]) and np.array_equal(got["del_flag"], st["del_flag"])
    if case.N == 0:
        for key in ("feat_mu", "last_klt", "del_flag"):
            assert got[key].shape == st[key].shape and got[key].size == 0 and np.array_equal(got[key], st[key]), key
        assert got["Sigma"].shape == (22, 22)
    if case.reading == "zero":  # an innovation of exactly zero moves no mean; the quaternion is only renormalised
        keep = np.r_[0:3, 7:22]
        assert np.array_equal(got["base_mu"][keep], st["base_mu"][keep]) and np.array_equal(got["feat_mu"], st["feat_mu"])


@pytest.mark.parametrize("case", I.CASES, ids=I.case_id)
def test_imu_kernels_compute_their_numpy_restatement_bit_for_bit(case):
    """_imu_cases.kernel_order_fp32 restates imu.hip's order of operations in numpy fp32 (no fused multiply-add, correctly rounded division
    and square root); tests/test_imu_cases_cpu.py holds that restatement to the criterion without a GPU.  On the MI355X the kernels gave its
    bits in every element of every case, so that is what they are held to: a change of the kernels' arithmetic shows here first, in the
    element it touches, and is then made to the restatement too."""
    st, gyro, acc, gv, av, g = I.inputs(case)
    got, k32 = run_case(case), I.kernel_order_fp32(st, gyro, acc, gv, av, g)
    for key in ("base_mu", "feat_mu", "Sigma"):
        bad = np.argwhere(got[key] != k32[key])
        assert bad.shape[0] == 0, (I.case_id(case), key, bad.shape[0], "elements differ, the first at", bad[0])


def test_the_cases_cover_the_workgroup_edge_and_a_capacity_above_n():
    size = [c for c in I.CASES if c.family == "size"]
    ns = {22 + 3 * c.N for c in size}
    edges = [n for n in ns if n % 256 == 0]
    assert edges, ns
    for n in edges:
        assert n - 3 in ns and n + 3 in ns, (n, ns)
    assert any(n > 4 * 256 for n in ns) and 22 in ns  # more than four workgroups; no landmark at all
    above = [c for c in size if c.cap > c.N]
    assert above and all(c.camera_first for c in above)
    assert {(c.quat, c.grav) for c in I.CASES if c.family == "attitude"} == {(q, g) for q in I.QUATS for g in I.GRAVS}
    assert {c.reading for c in I.CASES if c.family == "reading"} == {"large", "zero", "noise"}
    assert {c.var for c in I.CASES if c.family == "reading" and c.reading == "noise"} == set(I.VARS)


def _shared_buffer_inputs(N):
    case = I.Case("size", N, N, "identity", "ggen", "noise", I.DEFAULT_VAR, False)
    st0, frame = I.start(N)   # the warmed state itself: physically consistent, so that the camera update is an ordinary one
    _, gyro, acc, gv, av, g = I.inputs(case)
    return st0, frame, gyro, acc, gv, av, g


# the camera update's flow with every landmark measured (tests/_update_cases.py FLOWS): (persistent, t2_updates)
CAMERA_FLOW = {30: (0, 0), 256: (1, 1), 400: (0, 0)}


@pytest.mark.parametrize("N", sorted(CAMERA_FLOW))
def test_imu_update_leaves_nothing_behind_for_the_camera_update(N):
    """Handle A: set_state, imuUpdate, get_state (S), process, camera update.  Handle B: set_state(S), process, camera update.  Same bits."""
    st0, frame, gyro, acc, gv, av, g = _shared_buffer_inputs(N)
    a = handle(N, g, gv, av)
    try:
        a.set_state(st0)
        a.imuUpdate(gyro, acc)
        S = a.get_state()
        flow_a = camera_step(a, frame)
        fa = a.get_state()
    finally:
        a.close()
    assert not np.array_equal(S["Sigma"], st0["Sigma"])
    b = handle(N, g, gv, av)
    try:
        b.set_state(S)
        flow_b = camera_step(b, frame)
        fb = b.get_state()
    finally:
        b.close()
    print("\nN = %d: camera update (return code, persistent, t2_updates) %s" % (N, flow_a))
    assert flow_a == flow_b and flow_a[1:] == CAMERA_FLOW[N], (flow_a, flow_b)
    assert_same_bits(fa, fb, "camera update behind an IMU update against the same from set_state, N = %d" % N)


@pytest.mark.parametrize("N", sorted(CAMERA_FLOW))
def test_camera_update_leaves_nothing_behind_for_the_imu_update(N):
    """Handle A: set_state, process, camera update, get_state (S), imuUpdate.  Handle B: set_state(S), imuUpdate.  Same bits."""
    st0, frame, gyro, acc, gv, av, g = _shared_buffer_inputs(N)
    a = handle(N, g, gv, av)
    try:
        a.set_state(st0)
        flow_a = camera_step(a, frame)
        S = a.get_state()
        a.imuUpdate(gyro, acc)
        fa = a.get_state()
    finally:
        a.close()
    assert flow_a[1:] == CAMERA_FLOW[N], flow_a
    b = handle(N, g, gv, av)
    try:
        b.set_state(S)
        b.imuUpdate(gyro, acc)
        fb = b.get_state()
    finally:
        b.close()
    assert not np.array_equal(fb["Sigma"], S["Sigma"])
    assert_same_bits(fa, fb, "IMU update behind a camera update against the same from set_state, N = %d" % N)


def test_two_imu_records_on_one_stamp():
    """ekfvio_imu with dt = 0: the second record of a stamp is process(0) + the update, from the state the first one left."""
    case = I.Case("reading", 30, 30, "1.03u", "ggen", "noise", I.DEFAULT_VAR, False)
    st, gyro, acc, gv, av, g = I.inputs(case)
    v = handle(case.cap, g, gv, av, cls=EKFVIO)
    e = v.tc_ekf
    try:
        e.set_state(st)
        v.imu_now(1.000, gyro, acc)  # the first record of all only sets the filter's clock
        assert_same_bits(e.get_state(), st, "the first record")
        v.imu_now(1.005, gyro, acc)
        mid = e.get_state()
        rng = np.random.default_rng(5)
        h = I.h_imu(mid["base_mu"].astype(np.float64), g.astype(np.float64))
        z2 = (h + np.concatenate([rng.normal(0, I.NOISE[0], 3), rng.normal(0, I.NOISE[1], 3)])).astype(np.float32)
        v.imu_now(1.005, z2[:3], z2[3:])  # the same stamp again
        got = e.get_state()
    finally:
        e.close()
    assert not np.array_equal(mid["Sigma"], st["Sigma"]) and not np.array_equal(got["Sigma"], mid["Sigma"])
    s32 = I.oracle_imu_update(np.float32, mid, z2[:3], z2[3:], gv, av, g, dt=0.0)
    s64 = I.oracle_imu_update(np.float64, mid, z2[:3], z2[3:], gv, av, g, dt=0.0)
    hold("two-records-one-stamp", got, s32, s64)
    # sharper than the criterion, whose allowance here is mostly process(0)'s own fp32 error: process(dt) is bit-equal to the fp32 oracle's
    # (tests/test_gpu_parity.py), and the update behind it is the kernels' numpy restatement from that state
    o = OracleFilter(np.float32)
    o.set_state(mid)
    o.process(np.float32(0.0))
    k32 = I.kernel_order_fp32(o.get_state(), z2[:3], z2[3:], gv, av, g)
    o.close()
    for key in ("base_mu", "feat_mu", "Sigma"):
        assert np.array_equal(got[key], k32[key]), (key, int(np.count_nonzero(got[key] != k32[key])), "elements differ")
    assert np.array_equal(got["last_klt"], mid["last_klt"]) and np.array_equal(got["del_flag"], mid["del_flag"])
