"""The IMU in its own frame, without a GPU (cases, restatements and criterion: tests/_imu_extrinsics.py; the model: include/ekfvio.h,
ekfvio_set_imu_extrinsics).

  * Both fp32 restatements meet the criterion of _imu_cases against the fp64 evaluation with a numeric Jacobian on every case.
  * ekfvio_imu_model -- the pure host function that compiles the inline functions the kernel compiles (csrc/imu_model.h) -- gives
    kernel_order_fp32_ext's y and H in every bit on every case, and with NULL, NULL the model of _imu_cases.kernel_order_fp32.
  * Anchors to what exists: for the signed permutation with p = 0 the fp64 update equals the unchanged oracle's imu_update fed with rotated
    readings and rotated bias states; for the identity with p = 0 it equals _imu_cases.np_imu_update.
  * Sensitivity, in _imu_cases' manner (run with -s for the table): each of _imu_extrinsics.DEFECTS put into the analytic fp64 evaluation
    must move some quantity by MARGIN = 10 tolerances in at least one case.
  * ekfvio_gravity_from_accel against a three-line fp64 evaluation; every EKFVIO_EINVAL path of the pure functions; the symbols.
  * experiment(): what the extrinsics buy on a rotating rig, in the fp64 oracle (printed; README, "IMU extrinsics").

SENSITIVITY as measured here (largest ratio fp64 result moved / tolerance over the 17 cases; "seen in" counts the cases at or above MARGIN;
the identity, p = 0 control is blind to all eight, 1e-4 tolerances each -- with M = I a bias added in front of M is the same bias):
    defect                        largest   in case (quantity)                              seen in   blind besides the control
    M_transposed                  2.3e7     identity, gy, permutation with P (base)         16 of 17
    M_missing_from_q_columns      2.0e6     N = 400 (quaternion rows of Sigma)              16
    c_missing_from_residual       2.9e5     identity, gy, permutation with P (base)         14        permutation p = 0; p parallel to omega
    C_missing_from_H              2.9e5     identity, gy, permutation with P (base block)   15        permutation p = 0
    C_minus_2pw_dropped           3.3e5     identity, gy, permutation with P (base block)   15        permutation p = 0
    C_transposed                  4.2e5     identity, gy, permutation with P (base block)   14        permutation p = 0; p parallel to omega
    p_in_imu_frame                4.8e5     identity, gy, permutation with P (base)         15        permutation p = 0
    biases_in_camera_frame        3.9e6     identity, gy, permutation with P (base block)   16
Both fp32 restatements use at most 0.87 of the tolerance (N = 1, landmark block; at most 0.25 from N = 30 on).

EXPERIMENT as measured here (attitude rad / position m / accelerometer bias m/s^2 after 150 frames): A raw readings 0.604 / 97.4 / 7.32;
B pre-rotated on the host, no lever arm 1.50e-3 / 7.75e-2 / 7.94e-2; C extrinsics set 1.44e-3 / 7.73e-2 / 3.76e-3.  B equals C within noise in
attitude and position at this lever arm and body rate; B's accelerometer bias absorbs the centripetal term (|w x (w x p)| = 0.08 m/s^2).
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

from ekf_vio_amd import capi
from ekf_vio_amd.sim import Scenario
from oracle import OracleFilter, set_threads

import _imu_cases as I
import _imu_extrinsics as X

NEW_SYMBOLS = ("ekfvio_set_imu_extrinsics", "ekfvio_get_imu_extrinsics", "ekfvio_set_gravity", "ekfvio_get_gravity", "ekfvio_gravity_from_accel",
               "ekfvio_imu_model")
ANCHOR_TOL = 1e-10  # x scale, per quantity: both sides exact up to the order of 16-term fp64 sums; five orders under the fp32 errors


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    I.use_threads()
    yield
    set_threads(1)


@pytest.fixture(scope="module")
def lib():
    return capi.load()


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def imu_model(lib, mu, g, R, p, gyro, acc):
    y, H = np.zeros(6, np.float32), np.zeros(96, np.float32)
    arr = [np.ascontiguousarray(a, np.float32) for a in (mu, g, gyro, acc)]
    Rp = [None, None] if R is None else [_fp(np.ascontiguousarray(R, np.float32)), _fp(np.ascontiguousarray(p, np.float32))]
    rc = lib.ekfvio_imu_model(_fp(arr[0]), _fp(arr[1]), Rp[0], Rp[1], _fp(arr[2]), _fp(arr[3]), _fp(y), _fp(H))
    return rc, y, H.reshape(6, 16)


def test_the_case_table_is_sound():
    assert len(X.CASES) == len(set(X.CASES)) == len({X.case_id(c) for c in X.CASES}) == 17
    assert X.CONTROL in X.CASES and X.ANCHOR in X.CASES
    assert sorted({22 + 3 * c.N for c in X.CASES if c.family == "size"}) == [22, 25, 256, 259, 1222]
    assert [c for c in X.CASES if c.camera_first] == [X.Case("size", 79, 256, "1.03u", "ggen", "noise", "generic-p", True)]
    for name, (R, p) in X.EXTS.items():
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1) < 1e-14, name
    assert np.abs(np.cross(X.OMEGA, X.P_PAR)).max() < 1e-16 and np.linalg.norm(X.P_PAR) > 0.05
    # IMU x forward -> optical z, IMU z up -> optical -y
    assert np.array_equal(X.R_PERM @ [1, 0, 0], [0, 0, 1]) and np.array_equal(X.R_PERM @ [0, 0, 1], [0, -1, 0])
    assert np.abs(X.R_GEN - X.R_PERM).max() > 0.05 and np.abs(X.R_GEN - X.R_GEN.T).max() > 0.5  # generic, and far from symmetric
    for c in X.CASES:
        st, gyro, acc, gv, av, g, R, p = X.inputs(c)
        assert np.array_equal(st["base_mu"][10:13], X.OMEGA.astype(np.float32))
        assert all(a.dtype == np.float32 for a in (st["base_mu"], st["feat_mu"], st["Sigma"], gyro, acc, g, R, p))


@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_both_fp32_restatements_meet_the_criterion(case):
    st, gyro, acc, gv, av, g, R, p = X.inputs(case)
    s32, s64 = X.reference(case)
    # the analytic fp64 evaluation agrees with the numeric one: the written-out H is the derivative of h_ext
    ana = X.np_state(X.np_ext_update(st["base_mu"], st["feat_mu"], st["Sigma"], gyro, acc, float(gv), float(av), g, R, p, "analytic"), st)
    ra = I.ratios(ana, s32, s64)
    assert max(ra.values()) < 0.05, ra
    r1 = I.ratios(s32, s32, s64, factor=1.0)
    assert all(np.isfinite(v) and v <= 1.0 for v in r1.values()), r1
    k32 = X.kernel_order_fp32_ext(st, gyro, acc, gv, av, g, R, p)
    rk = I.ratios(k32, s32, s64)
    print("\n%-56s kernel order / tolerance: %s" % (X.case_id(case), "  ".join("%s %.2f" % kv for kv in rk.items())))
    assert max(rk.values()) <= 1.0, rk
    # ... and the other way round: the second order against the kernel's
    ro = I.ratios(s32, k32, s64)
    assert max(ro.values()) <= 1.0, ro


@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_the_host_function_gives_the_restatement_bit_for_bit(case, lib):
    st, gyro, acc, gv, av, g, R, p = X.inputs(case)
    rc, y, H = imu_model(lib, st["base_mu"], g, R, p, gyro, acc)
    assert rc == capi.OK
    y2, H2 = X.ext_model_fp32(st["base_mu"], g, R, p, gyro, acc)
    assert np.array_equal(y, y2), (y, y2)
    assert np.array_equal(H, H2), np.argwhere(H != H2)
    # without extrinsics: the model of _imu_cases.kernel_order_fp32
    rc, y, H = imu_model(lib, st["base_mu"], g, None, None, gyro, acc)
    assert rc == capi.OK
    y2, H2 = X.plain_model_fp32(st["base_mu"], g, gyro, acc)
    assert np.array_equal(y, y2) and np.array_equal(H, H2)


@pytest.mark.parametrize("case", [c for c in I.CASES if c.family == "attitude" and c.grav == "ggen"] + [I.CONTROL], ids=I.case_id)
def test_the_restated_tail_is_imu_cases_kernel_order(case):
    """update_tail_fp32 behind plain_model_fp32 is _imu_cases.kernel_order_fp32, which the device without extrinsics is held to."""
    st, gyro, acc, gv, av, g = I.inputs(case)
    a, b = X.kernel_order_fp32_ext(st, gyro, acc, gv, av, g, None, None), I.kernel_order_fp32(st, gyro, acc, gv, av, g)
    for key in ("base_mu", "feat_mu", "Sigma"):
        assert np.array_equal(a[key], b[key]), key


def _within(a, b, what):
    qa, qb = I.quantities(a), I.quantities(b)
    for k in I.QUANTITIES:
        err, scale = I._size(qa[k][0], qa[k][1] - qb[k][1]), I._size(*qb[k])
        assert err <= ANCHOR_TOL * scale, (what, k, err, scale)


def test_the_permutation_with_p0_is_the_unchanged_oracle_on_rotated_readings():
    st, gyro, acc, gv, av, g, R, p = X.inputs(X.ANCHOR)
    assert not p.any()
    _, s64 = X.reference(X.ANCHOR)
    R64 = R.astype(np.float64)
    n = st["Sigma"].shape[0]
    T = np.eye(n)
    T[16:19, 16:19] = T[19:22, 19:22] = R64  # b' = R_ci b on both bias triples
    fed = I.fresh(st)
    fed = dict(fed, base_mu=fed["base_mu"].astype(np.float64), feat_mu=fed["feat_mu"].astype(np.float64),
               Sigma=T @ st["Sigma"].astype(np.float64) @ T.T)
    fed["base_mu"][16:19] = R64 @ st["base_mu"][16:19].astype(np.float64)
    fed["base_mu"][19:22] = R64 @ st["base_mu"][19:22].astype(np.float64)
    o = OracleFilter(np.float64)
    o.set_state(fed)
    o.imu_update(R64 @ gyro.astype(np.float64), R64 @ acc.astype(np.float64), float(gv), float(av), g.astype(np.float64))
    out = o.get_state()
    o.close()
    back = dict(out, base_mu=out["base_mu"].copy(), Sigma=T.T @ out["Sigma"] @ T)
    back["base_mu"][16:19] = R64.T @ out["base_mu"][16:19]
    back["base_mu"][19:22] = R64.T @ out["base_mu"][19:22]
    _within(back, s64, "oracle imu_update on rotated readings")


def test_the_identity_with_p0_is_the_model_without_extrinsics():
    st, gyro, acc, gv, av, g, R, p = X.inputs(X.CONTROL)
    _, s64 = X.reference(X.CONTROL)
    plain = I.np_state(I.np_imu_update(st["base_mu"], st["feat_mu"], st["Sigma"], gyro, acc, float(gv), float(av), g), st)
    _within(plain, s64, "np_imu_update")
    # (in fp32 the two are not the same bits: the accelerometer row is ((a + c) - rg) + b_acc with c = 0 here, against (a + b_acc) - rg)


# ---------------------------------------------------------------------------------------------------------------- sensitivity
@pytest.fixture(scope="module")
def table():
    out = {}
    for d in X.DEFECTS:
        rows = []
        for c in X.CASES:
            st, gyro, acc, gv, av, g, R, p = X.inputs(c)
            s32, s64 = X.reference(c)
            bad = X.np_state(X.np_ext_update(st["base_mu"], st["feat_mu"], st["Sigma"], gyro, acc, float(gv), float(av), g, R, p, "analytic", d), st)
            r = I.ratios(bad, s32, s64)
            k = max(r, key=r.get)
            rows.append((r[k], k, c))
        out[d] = rows
    return out


def test_every_defect_moves_the_fp64_result_by_ten_tolerances_somewhere(table):
    print("\n%-28s %-10s %-64s %s" % ("defect", "largest", "in case (quantity)", "cases at or above MARGIN"))
    short = []
    for d in X.DEFECTS:
        rows = table[d]
        r, k, c = max(rows, key=lambda t: t[0])
        blind = [X.case_id(t[2]) for t in rows if t[0] < I.MARGIN]
        print("%-28s %-10.3g %-64s %d of %d" % (d, r, "%s (%s)" % (X.case_id(c), k), len(rows) - len(blind), len(rows)))
        print("%-28s blind: %s" % ("", ", ".join(blind) or "none"))
        if r < I.MARGIN:
            short.append((d, r))
    assert not short, short


def test_the_control_is_blind_to_what_the_cases_are_for(table):
    """Identity with p = 0: M = I and every term with p vanishes, so no defect of the new arithmetic shows there.  (With M = I a bias added
    in front of M is the same bias: the control cannot see that defect either, which is printed, not asserted.)"""
    print()
    for d in X.DEFECTS:
        (r, k, c), = [t for t in table[d] if t[2] == X.CONTROL]
        print("%-28s at the control (identity, p = 0): %.3g tolerances (%s)" % (d, r, k))
        if d != "biases_in_camera_frame":
            assert r < 1.0, (d, r, k)


# ---------------------------------------------------------------------------------------------------------------- gravity from the accelerometer
def gravity_from_accel(lib, R, mean, magnitude):
    out = np.zeros(3, np.float32)
    m = np.ascontiguousarray(mean, np.float64)
    Rp = None if R is None else _fp(np.ascontiguousarray(R, np.float32))
    rc = lib.ekfvio_gravity_from_accel(Rp, m.ctypes.data_as(C.POINTER(C.c_double)), float(magnitude), _fp(out))
    return rc, out


@pytest.mark.parametrize("pitch_deg", [0.0, 30.0])
@pytest.mark.parametrize("ext", [None, "perm-p", "generic-p"])
@pytest.mark.parametrize("magnitude", [9.81, 0.0])
def test_gravity_from_accel(lib, pitch_deg, ext, magnitude):
    """A rig at rest reads the reaction to gravity: f_cam = -g_cam.  Level: g_cam = (0, 9.79, 0); pitched: rotated about the camera's x."""
    R32 = None if ext is None else X.ext32(ext)[0]
    R = np.eye(3) if ext is None else R32.astype(np.float64)
    g_cam = X.axis_angle((1, 0, 0), pitch_deg) @ np.array([0.0, 9.79, 0.0])
    mean = R.T @ (-g_cam) + np.array([0.01, -0.02, 0.015])  # (a small bias: the function does not know)
    rc, got = gravity_from_accel(lib, R32, mean, magnitude)
    assert rc == capi.OK
    want = -(R @ mean)
    if magnitude > 0:
        want = want * (float(np.float32(magnitude)) / np.linalg.norm(mean))
    assert np.abs(got.astype(np.float64) - want).max() <= np.spacing(np.float32(np.abs(want).max())), (got, want)
    if magnitude > 0:
        assert abs(np.linalg.norm(got.astype(np.float64)) - 9.81) < 2e-6
    assert np.abs(got - g_cam).max() < 0.05  # the rig's gravity, up to the bias


def test_einval_paths_of_the_pure_functions(lib):
    st, gyro, acc, gv, av, g, R, p = X.inputs(X.CASES[3])
    mu = st["base_mu"]
    ok = lambda R_, p_: imu_model(lib, mu, g, R_, p_, gyro, acc)[0]
    assert ok(R, p) == capi.OK and ok(None, None) == capi.OK
    y, H = np.zeros(6, np.float32), np.zeros(96, np.float32)
    args = [_fp(mu), _fp(g), _fp(R), _fp(p), _fp(gyro), _fp(acc), _fp(y), _fp(H)]
    for k in range(8):  # any single NULL: the two extrinsics alone are a pair
        a = list(args)
        a[k] = None
        assert lib.ekfvio_imu_model(*a) == capi.EINVAL, k
    bad = R.copy()
    bad[1, 1] = np.nan
    assert ok(bad, p) == capi.EINVAL
    assert ok(R, np.array([0, np.inf, 0], np.float32)) == capi.EINVAL
    assert ok((R * np.float32(1.01)), p) == capi.EINVAL                      # scaled
    assert ok(R * np.array([1, 1, -1], np.float32), p) == capi.EINVAL        # a reflection: det = -1
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R, (0.1, 0.2, 0.3)
    assert ok(T.ravel()[:9].reshape(3, 3).copy(), p) == capi.EINVAL          # the first nine numbers of a 4 x 4
    assert ok(np.round(R.astype(np.float64), 4).astype(np.float32), p) == capi.OK  # printed to four decimals
    assert ok(np.zeros((3, 3), np.float32), p) == capi.EINVAL
    # ekfvio_gravity_from_accel
    out = np.zeros(3, np.float32)
    m = np.array([0.0, -9.81, 0.0])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.ekfvio_gravity_from_accel(None, dp(m), 9.81, _fp(out)) == capi.OK
    assert lib.ekfvio_gravity_from_accel(None, None, 9.81, _fp(out)) == capi.EINVAL
    assert lib.ekfvio_gravity_from_accel(None, dp(m), 9.81, None) == capi.EINVAL
    assert lib.ekfvio_gravity_from_accel(None, dp(np.zeros(3)), 9.81, _fp(out)) == capi.EINVAL
    assert lib.ekfvio_gravity_from_accel(None, dp(np.array([0.0, np.nan, 1.0])), 9.81, _fp(out)) == capi.EINVAL
    assert lib.ekfvio_gravity_from_accel(None, dp(np.array([0.0, np.inf, 1.0])), 0.0, _fp(out)) == capi.EINVAL
    assert lib.ekfvio_gravity_from_accel(None, dp(m), float("nan"), _fp(out)) == capi.EINVAL
    assert lib.ekfvio_gravity_from_accel(_fp(bad), dp(m), 9.81, _fp(out)) == capi.EINVAL


def test_the_symbols_are_exported_and_bound(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in NEW_SYMBOLS:
        assert s in capi.SYMBOLS and s in exported and getattr(lib, s).argtypes is not None, s


# ---------------------------------------------------------------------------------------------------------------- what it buys
def _angle(q_est, q_true):
    d = abs(float(np.dot(q_est / np.linalg.norm(q_est), q_true / np.linalg.norm(q_true))))
    return 2.0 * np.arccos(min(d, 1.0))


def experiment(frames=150, per_frame=10, N=16, seed=11):
    """Scenario(16, omega = (0.3, 0.8, -0.2)), 150 frames at 30 Hz, ten IMU records per frame, the IMU mounted by the generic rotation at
    p = (0.10, 0, 0.05); readings M w and M (a + w x (w x p) - R(q_true)^T g) plus the NOISE sigmas.  Three fp64 filters: (A) raw readings,
    no extrinsics; (B) readings rotated into the camera's axes on the host, no lever arm; (C) extrinsics set.  Returns
    {name: (attitude error rad, position error m, accelerometer-bias error m/s^2)}."""
    R, p = X.R_GEN, np.array([0.10, 0.0, 0.05])
    g = np.array([0.0, 9.81, 0.0])
    gv, av = I.DEFAULT_VAR
    eye, zero = np.eye(3), np.zeros(3)
    setups = {"A raw": (lambda z: z, eye, zero), "B pre-rotated": (lambda z: R @ z, eye, zero), "C extrinsics": (lambda z: z, R, p)}
    out = {}
    for name, (feed, Rf, pf) in setups.items():
        sc = Scenario(N, seed=SEED_SCENARIO, omega=(0.3, 0.8, -0.2), dt=(1.0 / 30.0) / per_frame)
        rng = np.random.default_rng(seed)
        o = OracleFilter(np.float64)
        o.add_new_features(sc.initial_features())
        for k in range(frames * per_frame):
            sc.advance()
            o.process(sc.dt)
            w, a = sc.omega, sc.acc
            z_g = R.T @ w + rng.normal(0, I.NOISE[0], 3)
            z_a = R.T @ (a + np.cross(w, np.cross(w, p)) - I.rot_t(sc.quat, g)) + rng.normal(0, I.NOISE[1], 3)
            st = o.get_state()
            up = X.np_ext_update(st["base_mu"], st["feat_mu"], st["Sigma"], feed(z_g), feed(z_a), gv, av, g, Rf, pf, "analytic")
            o.set_state(dict(st, **X.np_state(up, st)))
            if (k + 1) % per_frame == 0:
                z, Rm, ps = sc.measure()
                o.update(z, Rm, ps)
        b = o.get_state()["base_mu"]
        o.close()
        out[name] = (_angle(b[3:7], sc.quat), float(np.linalg.norm(b[0:3] - sc.pos)), float(np.linalg.norm(b[16:19])))
    return out


SEED_SCENARIO = 3


def test_the_extrinsics_beat_raw_readings_on_a_rotating_rig():
    res = experiment()
    print("\n%-16s %-22s %-20s %s" % ("filter", "attitude error (rad)", "position error (m)", "accel-bias error (m/s^2)"))
    for name, (ea, ep, eb) in res.items():
        print("%-16s %-22.4g %-20.4g %.4g" % (name, ea, ep, eb))
    assert res["C extrinsics"][0] < res["A raw"][0] and res["C extrinsics"][1] < res["A raw"][1], res


def test_node_parameters_reach_the_replay_driver(tmp_path):
    """imu_rotation, imu_position and gravity_align_samples by name through ekfvio::Params, echoed by --print-config."""
    import json
    from ekf_vio_amd import _build
    _build.build()
    exe = _build.build_host()

    def run(text):
        args = [exe, "--print-config"]
        if text is not None:
            f = tmp_path / "params.yaml"
            f.write_text(text)
            args.append(str(f))
        out = subprocess.run(args, capture_output=True, text=True, timeout=120)
        return out.returncode, (json.loads(out.stdout) if out.returncode == 0 else out.stderr)

    rc, d = run(None)
    assert rc == 0 and d["imu_extrinsics"] == 0 and d["gravity_align_samples"] == 0
    assert d["imu_rotation"] == [1, 0, 0, 0, 1, 0, 0, 0, 1] and d["imu_position"] == [0, 0, 0]
    rc, d = run("imu_rotation: [0, -1, 0, 0, 0, -1, 1, 0, 0]\nimu_position: 0.05 -0.02 0.11\n~gravity_align_samples: 200\n")
    assert rc == 0, d
    assert d["imu_extrinsics"] == 1 and d["gravity_align_samples"] == 200 and d["imu_rotation"] == [0, -1, 0, 0, 0, -1, 1, 0, 0]
    assert np.allclose(d["imu_position"], [0.05, -0.02, 0.11], rtol=0, atol=1e-8)
    rc, d = run("imu_position: [0.1, 0, 0.05]\n")  # one of the two alone: the other keeps its default
    assert rc == 0 and d["imu_extrinsics"] == 1 and d["imu_rotation"] == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    for bad in ("imu_rotation: [1, 0, 0, 0, 1, 0, 0, 0]\n", "imu_rotation: 1 0 0 0 1 0 0 0 1 0\n", "imu_position: [0, 0]\n", "imu_position: [0, x, 0]\n",
                "imu_position: [0, nan, 0]\n", "gravity_align_samples: -1\n", "gravity_align_samples: 2.5\n"):
        rc, err = run(bad)
        assert rc == 2 and "error" in err, (bad, err)
