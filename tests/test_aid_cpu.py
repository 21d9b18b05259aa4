"""The linear aiding measurement of the base state without a GPU (include/ekfvio.h, ekfvio_aid_update; restatements: tests/_aid.py).

  * ekfvio_aid_innovation and ekfvio_aid_rows_body_velocity, the host functions that compile the kernels' inline functions (csrc/aid.h),
    against the NumPy restatement, bit for bit: k = 1, 3, 6; selection, dense and quaternion-touching H; diagonal and full R; on filter
    states and on random covariance blocks.  Refused inputs are refused.
  * The header's order of operations restated in fp32 against the same lines in fp64 (themselves held to the textbook's product form,
    numpy.linalg, fp64) by _aid.hold: an a-priori rounding bound on every element, and the criterion of tests/_imu_cases.py -- 4 x the error
    of a second honest fp32 order plus 2^-23 of the scale -- on every case whose own cancellation figure is at most 1, with ONE named
    exception (_aid.EXCEPTIONS: N = 1, six dense rows, the landmark block of Sigma, 1.263 of the allowance; why, and what it is held to
    instead, is written there).  With H the selection of rows 7..12, z = 0 and a diagonal R the restatement is
    tests/_zupt.py's, bit for bit.
  * The scale experiment of the README's table (run with -s for the figures), asserted as conditions.
  * The boundary: header, exports, ctypes signatures, the parameter blocks of the replay driver and of the Python classes.
"""
import ctypes as C
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

from ekf_vio_amd import capi
from oracle import set_threads

import _aid as A
import _imu_cases as I
import _zupt as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 30, 78, 79)
NEW = ("ekfvio_aid_update", "ekfvio_aid", "ekfvio_set_frame_aid", "ekfvio_get_aid", "ekfvio_aid_innovation", "ekfvio_aid_rows_body_velocity")
fp = C.POINTER(C.c_float)


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    I.use_threads()
    yield
    set_threads(1)


def _p(a):
    return None if a is None else a.ctypes.data_as(fp)


def host_innovation(base_mu, Sbb, H, z, R):
    """ekfvio_aid_innovation -> (rc, y, S, d2, pd); R as the caller holds it (lower triangle read)."""
    z = np.ascontiguousarray(z, np.float32).ravel()
    k = z.shape[0]
    H = np.ascontiguousarray(H, np.float32).ravel()
    R = np.asarray(R, np.float32)
    R = np.ascontiguousarray(np.diag(R) if (R.ndim == 1 and k > 1) else R.reshape(k, k))
    mu = np.ascontiguousarray(base_mu, np.float32).ravel()
    S0 = np.ascontiguousarray(Sbb, np.float32)
    y, S = np.full(k, 7.0, np.float32), np.full((k, k), 7.0, np.float32)
    d2, pd = C.c_float(-5), C.c_int32(-5)
    rc = capi.load().ekfvio_aid_innovation(_p(mu), _p(S0), k, _p(H), _p(z), _p(R), _p(y), _p(S), C.byref(d2), C.byref(pd))
    return rc, y, S, np.float32(d2.value), pd.value


def assert_innovation(what, base_mu, Sbb, H, z, R):
    rc, y, S, d2, pd = host_innovation(base_mu, Sbb, H, z, R)
    assert rc == capi.OK, what
    ry, rA, rS, rL, rd2, rok = A.innovation(base_mu, Sbb, H, z, R)
    assert y.tobytes() == ry.tobytes(), (what, "y", y, ry)
    assert S.tobytes() == rS.tobytes(), (what, "S", S, rS)
    assert pd == int(rok), (what, pd, rok)
    assert (np.isnan(d2) and np.isnan(rd2)) or d2.tobytes() == np.float32(rd2).tobytes(), (what, "d2", d2, rd2)
    return d2, pd


# ---- 1: the host functions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 30])
def test_host_innovation_is_the_restatement_on_filter_states(N):
    st = I.fresh(I.start(N)[0])
    Sbb = st["Sigma"][:22, :22]
    seen = set()
    for name, (H, z, R) in A.measurement_cases(st).items():
        d2, pd = assert_innovation((N, name), st["base_mu"], Sbb, H, z, R)
        assert pd == 1 and d2 >= 0
        seen.add(len(np.ravel(z)))
        if name == "k3-zero-innovation":
            assert d2 == 0
    assert seen == {1, 3, 6}


def test_host_innovation_is_the_restatement_on_random_blocks():
    f = np.float32
    for seed in range(6):
        rng = np.random.default_rng([11, seed])
        B = rng.normal(size=(22, 22))
        Sbb = (B @ B.T * 10.0 ** rng.uniform(-4, 1)).astype(f)  # (both triangles as rounded: they agree only up to rounding, as Sigma's do)
        Sbb[3, 5] = np.nextafter(Sbb[3, 5], f(1))               # ... and here not even that: the lines say which triangle each sum reads
        mu = rng.normal(size=22).astype(f)
        for k in (1, 2, 3, 4, 5, 6):
            H = rng.normal(size=(k, 22)).astype(f)
            if seed % 2:
                H[rng.random((k, 22)) < 0.7] = 0
            Bk = rng.normal(size=(k, k))
            R = ((Bk @ Bk.T + k * np.eye(k)) * 1e-3).astype(f)
            R[np.triu_indices(k, 1)] = 99.0                     # the upper triangle is never read
            z = rng.normal(size=k).astype(f)
            assert_innovation((seed, k), mu, Sbb, H, z, R)
    # a block that is not positive definite against a small R: the verdict and the NaN
    Sbb = -np.eye(22, dtype=f)
    d2, pd = assert_innovation("indefinite", np.zeros(22, f), Sbb, A.selection([7, 8]), np.zeros(2, f), np.array([1e-3, 1e-3], f))
    assert pd == 0 and np.isnan(d2)


def host_rows(R_cv, p_cv, v, cov):
    H, z, R = np.full(66, 7.0, np.float32), np.full(3, 7.0, np.float32), np.full(9, 7.0, np.float32)
    a = [None if x is None else np.ascontiguousarray(x, np.float32).ravel() for x in (R_cv, p_cv, v, cov)]
    rc = capi.load().ekfvio_aid_rows_body_velocity(_p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(H), _p(z), _p(R))
    return rc, H.reshape(3, 22), z, R.reshape(3, 3)


def test_host_body_velocity_rows_are_the_restatement():
    f = np.float32
    rng = np.random.default_rng(5)
    car = np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]], f)  # v_cam = R_cv v_vehicle: vehicle x forward = camera z, y left = camera -x, z up = camera -y
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    gen = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                    [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]).astype(f)
    cov_full = np.array([[4e-4, 1e-4, 0], [1e-4, 5e-4, -1e-4], [0, -1e-4, 3e-4]], f)
    cov_lower = cov_full.copy()
    cov_lower[np.triu_indices(3, 1)] = 99.0  # only the lower triangle is read
    cov_nan = cov_full.copy()
    cov_nan[np.triu_indices(3, 1)] = np.nan  # ... not even for finiteness, as R's upper triangle in ekfvio_aid_update
    rc, _, _, R_nan = host_rows(None, None, np.zeros(3, f), cov_nan)
    assert rc == capi.OK and R_nan.tobytes() == A.body_velocity_rows(None, None, np.zeros(3, f), cov_full)[2].tobytes()
    for name, Rcv, p, cov in (("identity, no lever", None, None, np.diag([4e-4] * 3).astype(f)), ("car", car, np.array([0.1, -0.05, 0.3], f), cov_full),
                              ("generic", gen, rng.normal(size=3).astype(f), cov_lower), ("lever alone", None, np.array([0, 0.2, -1.5], f), cov_full)):
        v = rng.normal(size=3).astype(f)
        rc, H, zz, R = host_rows(Rcv, p, v, cov)
        assert rc == capi.OK, name
        rH, rz, rR = A.body_velocity_rows(Rcv, p, v, cov)
        assert H.tobytes() == rH.tobytes() and zz.tobytes() == rz.tobytes() and R.tobytes() == rR.tobytes(), name
        # the model itself, in fp64: z = R_cv^T (vel + omega x p)
        x22 = rng.normal(size=22)
        Rc = np.eye(3) if Rcv is None else Rcv.astype(np.float64)
        pp = np.zeros(3) if p is None else p.astype(np.float64)
        assert np.abs(H.astype(np.float64) @ x22 - Rc.T @ (x22[7:10] + np.cross(x22[10:13], pp))).max() < 1e-5, name
        assert not H[:, :7].any() and not H[:, 13:].any()
    eye, zero3, ok_cov = np.eye(3, dtype=f), np.zeros(3, f), np.diag([1e-4] * 3).astype(f)
    assert host_rows(eye, zero3, zero3, ok_cov)[0] == capi.OK
    for name, args in (("a reflection", (np.diag([1, 1, -1]).astype(f), zero3, zero3, ok_cov)), ("a scaled rotation", (2 * eye, zero3, zero3, ok_cov)),
                       ("a NaN lever", (eye, np.array([0, np.nan, 0], f), zero3, ok_cov)), ("an infinite velocity", (eye, zero3, np.array([np.inf, 0, 0], f), ok_cov)),
                       ("an indefinite covariance", (eye, zero3, zero3, np.diag([1e-4, -1e-4, 1e-4]).astype(f))), ("no velocity", (eye, zero3, None, ok_cov)),
                       ("no covariance", (eye, zero3, zero3, None))):
        assert host_rows(*args)[0] == capi.EINVAL, name
    H = np.zeros(66, f)
    assert capi.load().ekfvio_aid_rows_body_velocity(None, None, _p(zero3), _p(ok_cov), None, _p(zero3.copy()), _p(np.zeros(9, f))) == capi.EINVAL
    assert capi.load().ekfvio_aid_rows_body_velocity(None, None, _p(zero3), _p(ok_cov), _p(H), None, _p(np.zeros(9, f))) == capi.EINVAL


def refused_rows():
    """(name, k, H, z, R, chi2) that every entry point refuses; k is passed as given."""
    f = np.float32
    H, z, R = A.selection([7, 8, 9]), np.zeros(3, f), np.diag([1e-4] * 3).astype(f)
    nanH, infz, nanR = H.copy(), z.copy(), R.copy()
    nanH[1, 4], infz[2], nanR[2, 0] = np.nan, np.inf, np.nan
    ind = np.array([[1, 2, 0], [2, 1, 0], [0, 0, 1]], f) * f(1e-4)  # symmetric, indefinite
    return [("k = 0", 0, H, z, R, 0.0), ("k = 7", 7, np.zeros((7, 22), f), np.zeros(7, f), np.eye(7, dtype=f), 0.0), ("k < 0", -1, H, z, R, 0.0),
            ("no H", 3, None, z, R, 0.0), ("no z", 3, H, None, R, 0.0), ("no R", 3, H, z, None, 0.0), ("a NaN in H", 3, nanH, z, R, 0.0),
            ("an infinite z", 3, H, infz, R, 0.0), ("a NaN in R's lower triangle", 3, H, z, nanR, 0.0), ("chi2 < 0", 3, H, z, R, -1.0),
            ("chi2 NaN", 3, H, z, R, float("nan")), ("R indefinite", 3, H, z, ind, 0.0), ("R zero", 3, H, z, np.zeros((3, 3), f), 0.0),
            ("R negative, k = 1", 1, A.selection([9]), np.zeros(1, f), np.array([-1e-4], f), 0.0)]


def test_host_innovation_refuses_what_the_entry_points_refuse():
    f = np.float32
    fn = capi.load().ekfvio_aid_innovation
    mu, Sbb = np.zeros(22, f), np.eye(22, dtype=f)
    y, S, d2, pd = np.zeros(7, f), np.zeros(49, f), C.c_float(0), C.c_int32(0)
    for name, k, H, z, R, chi2 in refused_rows():
        if "chi2" in name:
            continue  # (the innovation takes no gate)
        a = [None if x is None else np.ascontiguousarray(x, f) for x in (H, z, R)]
        assert fn(_p(mu), _p(Sbb), k, _p(a[0]), _p(a[1]), _p(a[2]), _p(y), _p(S), C.byref(d2), C.byref(pd)) == capi.EINVAL, name
    H, z, R = np.ascontiguousarray(A.selection([9])), np.zeros(1, f), np.array([1e-4], f)
    assert fn(None, _p(Sbb), 1, _p(H), _p(z), _p(R), None, None, None, None) == capi.EINVAL
    assert fn(_p(mu), None, 1, _p(H), _p(z), _p(R), None, None, None, None) == capi.EINVAL
    bad = Sbb.copy()
    bad[4, 4] = np.nan
    assert fn(_p(mu), _p(bad), 1, _p(H), _p(z), _p(R), None, None, None, None) == capi.EINVAL
    assert fn(_p(mu), _p(Sbb), 1, _p(H), _p(z), _p(R), None, None, None, None) == capi.OK  # (every output may be NULL)


# ---- 2: the restatement against fp64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_kernel_order_restatement_against_fp64(N):
    st = I.fresh(I.start(N)[0])
    for name, (H, z, R) in A.measurement_cases(st).items():
        k32, info = A.kernel_order_fp32(st, H, z, R)
        assert info["accepted"] and info["pd"], name
        s32, s64 = A.reference(st, H, z, R)
        # the yardstick itself against the textbook's product form, fp64 both: two formulas, one update
        p64 = A.plain_update(st, H, z, R)
        for key in ("base_mu", "feat_mu", "Sigma"):
            scale = max(float(np.abs(p64[key]).max()), 1e-30) if p64[key].size else 1.0
            assert p64[key].size == 0 or float(np.abs(s64[key] - p64[key]).max()) <= 1e-9 * max(scale, float(np.abs(st[key]).max())), (name, key)
        for key in ("base_mu", "feat_mu", "Sigma"):
            assert k32[key].dtype == np.float32 and np.isfinite(k32[key]).all(), (name, key)
        A.hold("N%d %s" % (N, name), k32, st, H, z, R, exempt=A.exceptions(N, name))
        assert abs(np.linalg.norm(k32["base_mu"][3:7].astype(np.float64)) - 1) < 1e-6
        assert np.array_equal(k32["last_klt"], st["last_klt"]) and np.array_equal(k32["del_flag"], st["del_flag"])
        if name == "k3-zero-innovation":  # nothing moves the mean but the quaternion's renormalisation
            keep = np.r_[0:3, 7:22]
            assert k32["base_mu"][keep].tobytes() == np.asarray(st["base_mu"], np.float32)[keep].tobytes() and info["d2"] == 0
            assert k32["feat_mu"].tobytes() == np.asarray(st["feat_mu"], np.float32).tobytes()


@pytest.mark.parametrize("N", [0, 1, 30, 79])
def test_restatement_is_the_zero_velocity_updates_bit_for_bit(N):
    st = I.fresh(I.start(N)[0])
    H, z = A.selection(range(7, 13)), np.zeros(6, np.float32)
    for vv, ov in ((1e-4, 1e-4), (1e-2, 1e-6), (1.0, 1.0)):
        want = Z.kernel_order_fp32(st, vv, ov)
        Rd = np.array([vv] * 3 + [ov] * 3, np.float32)
        for R in (Rd, np.diag(Rd)):
            got, info = A.kernel_order_fp32(st, H, z, R)
            assert info["accepted"]
            for key in ("base_mu", "feat_mu", "Sigma"):
                assert got[key].tobytes() == want[key].tobytes(), (N, vv, ov, key)


def test_gate_and_pivots_decide():
    st = I.fresh(I.start(30)[0])
    H, R = A.selection([7, 8, 9]), np.array([4e-4] * 3, np.float32)
    z = (np.asarray(st["base_mu"], np.float32)[7:10] + np.float32(1.0)).astype(np.float32)  # an innovation of 1 m/s per axis
    got, info = A.kernel_order_fp32(st, H, z, R, chi2=0.0)
    assert info["accepted"] and info["d2"] > 100
    for chi2, verdict in ((float(info["d2"]), True), (float(np.nextafter(info["d2"], np.float32(0))), False), (7.81, False)):
        got, i2 = A.kernel_order_fp32(st, H, z, R, chi2=chi2)
        assert i2["accepted"] is verdict and i2["d2"].tobytes() == info["d2"].tobytes()
        if not verdict:
            for key in ("base_mu", "feat_mu", "Sigma"):
                assert got[key].tobytes() == np.asarray(st[key]).tobytes()
    neg = I.fresh(st)
    neg["Sigma"] = neg["Sigma"].copy()
    neg["Sigma"][8, 8] = np.float32(-1.0)  # S(1,1) = Sigma(8,8) + R < 0: the second pivot fails
    got, info = A.kernel_order_fp32(neg, H, z, R)
    assert not info["accepted"] and not info["pd"] and np.isnan(info["d2"])
    assert got["Sigma"].tobytes() == neg["Sigma"].tobytes()


def test_the_criterion_can_fail():
    """tests/test_zupt_cpu.py's counter-check on this module's hold(): one digit worse misses the 4 x criterion, half precision the bound."""
    st = I.fresh(I.start(30)[0])
    H, z, R = A.measurement_cases(st)["k3-velocity-fullR"]
    k32, _ = A.kernel_order_fp32(st, H, z, R)
    worse = I.fresh(k32)
    worse["Sigma"] = (k32["Sigma"].astype(np.float64) * (1 + 2.0 ** -19)).astype(np.float32)
    with pytest.raises(AssertionError):
        A.hold("one digit worse", worse, st, H, z, R)
    bad = I.fresh(k32)
    bad["Sigma"] = k32["Sigma"].astype(np.float16).astype(np.float32)
    with pytest.raises(AssertionError, match="a-priori"):
        A.hold("half precision", bad, st, H, z, R)
    assert max(I.ratios(k32, *A.reference(st, H, z, R)).values()) < 1


# ---- 3: the experiment --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [0.5, 2.0, 5.0])
def test_scale_experiment(D):
    """Scenario(16, seed=3) at true depth D, landmarks born at the default depth 0.5, 150 frames, sd 1e-3 on z: a body-velocity measurement
    (sd 0.02 m/s per axis) in front of every camera update makes the scale metric.  Measured when the feature was proposed: position error
    <= 0.031 of the distance travelled and median depth ratio 0.988 .. 1.025 with the aiding; 0.60 and 0.84 of the distance without it at
    D = 2 and 5."""
    off, vel, track = A.experiment(D, None), A.experiment(D, "vel"), A.experiment(D, "track")
    for name, r in (("no aiding", off), ("[vel] measured", vel), ("speed along track + zero across", track)):
        print("\nAID-EXPERIMENT D=%g %s: position error %.3f of %.3f travelled (%.3f), median depth ratio %.3f" % (D, name, r[0], r[1], r[0] / r[1], r[2]))
    assert vel[0] <= 0.1 * vel[1], vel
    assert 0.9 <= vel[2] <= 1.1, vel
    if D != 0.5:
        assert off[0] >= 0.5 * off[1], off


# ---- 4: the boundary ----------------------------------------------------------------------------------------------------------------------
def test_exports_equal_the_header():
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "ekfvio.h")).read()
    marked = set(re.findall(r"^EKFVIO_API [a-z \*]*?\b(ekfvio_[a-z0-9_]+)\s*\(", hdr, re.M))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in NEW:
        assert s in marked and s in exported and s in capi.SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
    assert marked == exported
    assert lib.ekfvio_aid_update(None, 1, None, None, None, 0.0) == capi.EINVAL
    assert lib.ekfvio_get_aid(None, None, None, None, None) == capi.EINVAL
    assert lib.ekfvio_set_frame_aid(None, 0, None, None, None, 0.0) == capi.EINVAL
    hpp = open(os.path.join(ROOT, "ekf_vio_amd", "host", "ekfvio.hpp")).read()
    for name in ("aidUpdate", "aid", "setFrameAid", "aidStatus"):
        assert re.search(r"\b%s\(" % name, hpp), name


def test_python_classes_take_the_new_arguments():
    from ekf_vio_amd import EKFVIO, TightlyCoupledEKF
    assert "frame_aid" in inspect.signature(TightlyCoupledEKF.__init__).parameters
    for cls in (TightlyCoupledEKF, EKFVIO):
        for name in ("aidUpdate", "aid", "setFrameAid", "aid_status"):
            assert callable(getattr(cls, name)), (cls, name)
    k, H, z, R = TightlyCoupledEKF._aid_rows(A.selection([7, 8]), [0, 0], [1e-4, 2e-4])
    assert k == 2 and H.shape == (44,) and R.reshape(2, 2)[1, 1] == np.float32(2e-4) and R.reshape(2, 2)[0, 1] == 0
    with pytest.raises(capi.EkfvioError):
        TightlyCoupledEKF._aid_rows(A.selection([7, 8]), [0, 0, 0], [1e-4] * 3)


def test_node_parameters_reach_the_replay_driver(tmp_path):
    """nhc_variance and nhc_R_cv by name through ekfvio::Params, echoed by --print-config; out-of-range values are errors."""
    from ekf_vio_amd import _build
    _build.build()
    exe = _build.build_host()

    def run(text, extra=()):
        args = [exe, "--print-config"]
        if text is not None:
            f = tmp_path / "params.yaml"
            f.write_text(text)
            args.append(str(f))
        out = subprocess.run(args + list(extra), capture_output=True, text=True, timeout=120)
        return out.returncode, (json.loads(out.stdout) if out.returncode == 0 else out.stderr)

    rc, d = run(None)
    # off by default; the default axes are a forward-looking optical camera's (vehicle x forward = camera z, y left = -x, z up = -y)
    assert rc == 0 and d["nhc_variance"] == 0 and d["nhc_R_cv"] == [0, -1, 0, 0, 0, -1, 1, 0, 0]
    rc, d = run("nhc_variance: 1e-3\nnhc_R_cv: [1, 0, 0, 0, 0, 1, 0, -1, 0]\n")
    assert rc == 0, d
    assert abs(d["nhc_variance"] - 1e-3) < 1e-9 and d["nhc_R_cv"] == [1, 0, 0, 0, 0, 1, 0, -1, 0]
    rc, d = run(None, ("--nhc-variance", "0.01"))
    assert rc == 0 and abs(d["nhc_variance"] - 0.01) < 1e-8, d
    for bad in ("nhc_variance: -1\n", "nhc_variance: nan\n", "nhc_variance: 1e39\n", "nhc_R_cv: [1, 0, 0]\n", "nhc_R_cv: [2, 0, 0, 0, 2, 0, 0, 0, 2]\n",
                "nhc_R_cv: [1, 0, 0, 0, 1, 0, 0, 0, -1]\n"):
        rc, err = run(bad)
        assert rc == 2 and "error" in err, (bad, err)
