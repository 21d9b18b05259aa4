"""The zero-velocity update without a GPU (include/ekfvio.h, ekfvio_set_zupt; restatements: tests/_zupt.py).

  * ekfvio_zupt_decide, the host function that compiles the decision's inline functions (csrc/zupt.h), against the NumPy restatement, bit
    for bit, on random points and at the edges.
  * zupt.hip's order of operations restated in fp32 against the specification's lines in fp64 (themselves held to the textbook's product
    form, numpy.linalg, fp64), on the states of _imu_cases.start(N), by _zupt.hold: an a-priori rounding bound on every element of every
    state, and the criterion of tests/_imu_cases.py -- 4 x the fp32 error plus 2^-23 of the scale -- with a second, independent fp32
    rounding order of the same formula as the fp32 error, on every state whose subtracted products do not cancel among themselves
    (_zupt.cancellation <= 1).  _zupt.hold says why the factor 4 is not asserted on the one state where they do (N = 1: one landmark,
    depth and speed unobservable together) and records its figures: 4.96 there with variances 1e-4.
  * After one update Sigma'(k,k) <= min(Sigma(k,k), R_k) for k = 7..12 (exact in real arithmetic), up to that criterion's allowance.
  * The standing-still experiment of the README's table and its braking counter-finding (run with -s for the figures).
"""
import ctypes as C

import numpy as np
import pytest

from ekf_vio_amd import capi
from oracle import set_threads

import _imu_cases as I
import _zupt as Z

SIZES = (0, 1, 30, 78, 79, 170)
VARS = ((1e-4, 1e-4), (1e-2, 1e-6), (1.0, 1.0))


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    I.use_threads()
    yield
    set_threads(1)


def host_decide(prev, cur, passed, max_flow_px, min_tracks, min_ratio, fn=None, handle=None):
    """ekfvio_zupt_decide (or, with fn and handle, the device hook of the same signature) -> (flow2, n_pass, n_still, stationary)."""
    p = np.ascontiguousarray(prev, np.float32).reshape(-1, 2)
    q = np.ascontiguousarray(cur, np.float32).reshape(-1, 2)
    ok = np.ascontiguousarray(passed, np.uint8).ravel()
    n = ok.shape[0]
    flow2 = np.full(max(n, 1), 7.0, np.float32)
    a, b, c = C.c_int32(-5), C.c_int32(-5), C.c_int32(-5)
    fp, u8 = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    args = [p.ctypes.data_as(fp) if n else None, q.ctypes.data_as(fp) if n else None, ok.ctypes.data_as(u8) if n else None, n, float(max_flow_px),
            int(min_tracks), float(min_ratio), flow2.ctypes.data_as(fp), C.byref(a), C.byref(b), C.byref(c)]
    rc = fn(handle, *args) if fn else capi.load().ekfvio_zupt_decide(*args)
    assert rc == capi.OK, rc
    return flow2[:n].copy(), a.value, b.value, c.value


def assert_decision(got, want, what):
    assert got[0].tobytes() == want[0].tobytes(), (what, "flow2", got[0], want[0])
    assert got[1:] == want[1:], (what, got[1:], want[1:])


def edge_cases():
    """(name, prev, cur, pass, max_flow_px, min_tracks, min_ratio, expected (n_pass, n_still, stationary) or None)."""
    f = np.float32
    z4 = np.zeros((4, 2), f)
    out = []
    # e2 exactly t2: a flow of (0.25, 0) squares to 0.0625 exactly, and so does the threshold 0.25
    t = f(0.25)
    cur = np.array([[t, 0]] * 4, f)  # dx = 0.25 exactly, e2 = 0.0625 = t2
    out.append(("e2 == t2 accepted", z4, cur, [1] * 4, 0.25, 4, 1.0, (4, 4, 1)))
    out.append(("one ulp above t2", z4, np.array([[np.nextafter(t, f(1)), 0]] * 4, f), [1] * 4, 0.25, 4, 1.0, (4, 0, 0)))
    nan = z4.copy()
    nan[1, 0] = np.nan
    out.append(("a NaN pixel is not still", z4, nan, [1] * 4, 0.25, 1, 1.0, (4, 3, 0)))
    out.append(("a NaN pixel, ratio 0.75", z4, nan, [1] * 4, 0.25, 1, 0.75, (4, 3, 1)))
    out.append(("n_pass == min_tracks - 1", z4, z4, [1, 1, 1, 0], 0.25, 4, 0.5, (3, 3, 0)))
    out.append(("n_pass == min_tracks", z4, z4, [1, 1, 1, 0], 0.25, 3, 0.5, (3, 3, 1)))
    far = z4.copy()
    far[0] = (3, 4)
    out.append(("3 of 4 still at 0.75", z4, far, [1] * 4, 0.25, 1, 0.75, (4, 3, 1)))
    far2 = far.copy()
    far2[2] = (-2, 0)
    out.append(("2 of 4 still at 0.75", z4, far2, [1] * 4, 0.25, 1, 0.75, (4, 2, 0)))
    out.append(("count 0", np.zeros((0, 2), f), np.zeros((0, 2), f), [], 0.25, 1, 0.75, (0, 0, 0)))
    out.append(("all-zero pass", z4, z4, [0] * 4, 0.25, 1, 0.75, (0, 0, 0)))
    out.append(("a failed landmark's NaN is not looked at", z4, nan, [1, 0, 1, 1], 0.25, 3, 1.0, (3, 3, 1)))
    return out


def random_case(count, seed):
    rng = np.random.default_rng([count, seed])
    prev = rng.uniform(0, 640, (count, 2)).astype(np.float32)
    flow = rng.normal(0, 0.3, (count, 2)) * (rng.random((count, 1)) < 0.8) + rng.normal(0, 5, (count, 2)) * (rng.random((count, 1)) < 0.1)
    cur = (prev + flow).astype(np.float32)
    ok = (rng.random(count) < 0.85).astype(np.uint8)
    if count > 3:
        cur[rng.integers(count)] = np.nan
    return prev, cur, ok, 0.5, max(count // 2, 1), 0.6


def test_host_decision_matches_the_restatement_at_the_edges():
    for name, prev, cur, ok, mf, mt, mr, want in edge_cases():
        ref = Z.decide(prev, cur, ok, mf, mt, mr)
        assert ref[1:] == want, (name, ref[1:], want)  # the restatement itself says what the issue says
        assert_decision(host_decide(prev, cur, ok, mf, mt, mr), ref, name)
        assert np.array_equal(ref[0] == -1, np.asarray(ok, np.uint8) == 0), name


@pytest.mark.parametrize("count", [1, 63, 64, 65, 1024])
def test_host_decision_matches_the_restatement_on_random_points(count):
    seen = set()
    for seed in range(4):
        prev, cur, ok, mf, mt, mr = random_case(count, seed)
        for ratio in (mr, 0.9):
            ref = Z.decide(prev, cur, ok, mf, mt, ratio)
            assert_decision(host_decide(prev, cur, ok, mf, mt, ratio), ref, (count, seed, ratio))
            seen.add(ref[3])
    if count >= 63:
        assert seen == {0, 1}, seen  # both verdicts occur


def test_host_decision_refuses_what_the_setting_refuses():
    lib = capi.load()
    z = np.zeros(2, np.float32)
    p = z.ctypes.data_as(C.POINTER(C.c_float))
    one = np.ones(1, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
    good = (0.25, 1, 0.75)
    assert lib.ekfvio_zupt_decide(p, p, one, 1, *good, None, None, None, None) == capi.OK  # every output may be NULL
    for bad in ((0.0, 1, 0.75), (-1.0, 1, 0.75), (float("nan"), 1, 0.75), (float("inf"), 1, 0.75), (0.25, 0, 0.75), (0.25, 1, 0.0), (0.25, 1, 1.5),
                (0.25, 1, float("nan"))):
        assert lib.ekfvio_zupt_decide(p, p, one, 1, *bad, None, None, None, None) == capi.EINVAL, bad
    assert lib.ekfvio_zupt_decide(p, p, one, -1, *good, None, None, None, None) == capi.EINVAL
    assert lib.ekfvio_zupt_decide(None, p, one, 1, *good, None, None, None, None) == capi.EINVAL


def test_the_abi_covers_the_new_symbols():
    lib = capi.load()
    for s in ("ekfvio_set_zupt", "ekfvio_zupt_update", "ekfvio_get_zupt", "ekfvio_zupt_decide"):
        assert s in capi.SYMBOLS and hasattr(lib, s), s
    assert "ekfvio_test_zupt_decide" in capi.HOOK_SYMBOLS and not hasattr(lib, "ekfvio_test_zupt_decide")
    assert lib.ekfvio_set_zupt(None, 0.25, 8, 0.75, 1e-4, 1e-4) == capi.EINVAL
    assert lib.ekfvio_zupt_update(None, 1e-4, 1e-4) == capi.EINVAL
    assert lib.ekfvio_get_zupt(None, None, None, None, None, None, None) == capi.EINVAL


def test_node_parameters_reach_the_replay_driver(tmp_path):
    """zupt_* by name through ekfvio::Params, echoed by --print-config; out-of-range values are errors."""
    import json
    import subprocess
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
    assert rc == 0 and d["zupt_max_flow_px"] == 0 and d["zupt_min_tracks"] == 8 and d["zupt_min_ratio"] == 0.75
    assert abs(d["zupt_vel_variance"] - 1e-4) < 1e-10 and abs(d["zupt_omega_variance"] - 1e-4) < 1e-10
    rc, d = run("zupt_max_flow_px: 0.25\nzupt_min_tracks: 12\nzupt_min_ratio: 0.5\nzupt_vel_variance: 1e-3\n~zupt_omega_variance: 1e-5\n")
    assert rc == 0, d
    assert (d["zupt_max_flow_px"], d["zupt_min_tracks"], d["zupt_min_ratio"]) == (0.25, 12, 0.5)
    assert abs(d["zupt_vel_variance"] - 1e-3) < 1e-9 and abs(d["zupt_omega_variance"] - 1e-5) < 1e-11
    for bad in ("zupt_max_flow_px: -1\n", "zupt_min_tracks: 0\n", "zupt_min_ratio: 1.5\n", "zupt_min_ratio: 0\n", "zupt_vel_variance: 0\n",
                "zupt_omega_variance: -1e-4\n", "zupt_min_tracks: 2.5\n", "zupt_max_flow_px: nan\n", "zupt_max_flow_px: 1e39\n", "zupt_vel_variance: 1e39\n",
                "zupt_omega_variance: inf\n"):
        rc, err = run(bad)
        assert rc == 2 and "error" in err, (bad, err)


@pytest.mark.parametrize("N", SIZES)
def test_kernel_order_restatement_against_fp64(N):
    st = I.fresh(I.start(N)[0])
    for vv, ov in VARS:
        k32 = Z.kernel_order_fp32(st, vv, ov)
        s32, s64 = Z.reference(st, vv, ov)
        # the yardstick itself against the textbook's product form, fp64 both: two formulas, one update
        p64 = Z.plain_update(st, vv, ov, np.float64)
        for key in ("base_mu", "feat_mu", "Sigma"):
            scale = max(float(np.abs(p64[key]).max()), 1e-30) if p64[key].size else 1.0
            assert p64[key].size == 0 or float(np.abs(s64[key] - p64[key]).max()) <= 1e-9 * max(scale, float(np.abs(st[key]).max())), key
        for key in ("base_mu", "feat_mu", "Sigma"):
            assert k32[key].dtype == np.float32 and np.isfinite(k32[key]).all(), key
        Z.hold("N%d var%g,%g" % (N, vv, ov), k32, st, vv, ov)
        assert abs(np.linalg.norm(k32["base_mu"][3:7].astype(np.float64)) - 1) < 1e-6
        # the measured rows' variances: at most min(Sigma(k,k), R_k), exact in real arithmetic; the allowance is the criterion's, elementwise
        allow = I.tolerances(s32, s64)["sig_elementwise"]
        Rd = np.array([np.float32(vv)] * 3 + [np.float32(ov)] * 3, np.float64)
        before, after = np.diag(st["Sigma"]).astype(np.float64)[7:13], np.diag(k32["Sigma"]).astype(np.float64)[7:13]
        print("ZUPT-DIAG N%d var%g,%g: before %s after %s allowance %.3g" % (N, vv, ov, before, after, allow))
        assert (after <= np.minimum(before, Rd) + allow).all(), (N, vv, ov, after, np.minimum(before, Rd), allow)
        assert (after > 0).all()
        assert np.array_equal(k32["last_klt"], st["last_klt"]) and np.array_equal(k32["del_flag"], st["del_flag"])


@pytest.mark.parametrize("N", [16, 64])
def test_standing_still_experiment(N):
    """Scenario(N, seed=3): 20 moving frames, then the truth stops; 200 still frames with sd 1e-3 of metric noise; the pseudo-measurement
    (both variances 1e-4) in front of every still frame's update from the second.  Measured when the feature was proposed: |v| falls by a
    factor of 17 at the least; the 2 asserted is the margin for the noise stream's handling."""
    off = Z.experiment(N, 1e-3, False)
    on = Z.experiment(N, 1e-3, True)
    print("\nZUPT-EXPERIMENT N=%d sd=1e-3: drift off/on %.3g / %.3g   |v| off/on %.3g / %.3g   |omega| off/on %.3g / %.3g"
          % (N, off[0], on[0], off[1], on[1], off[2], on[2]))
    assert on[1] < 0.5 * off[1], (on, off)
    assert on[2] < 0.5 * off[2], (on, off)
    assert on[0] < off[0], (on, off)


def test_the_criterion_can_fail():
    """A result that is honest fp32 but one digit worse -- the kernels' order with its gains rounded to 20 bits -- misses the 4 x criterion, and
    one that loses half the digits misses the a-priori bound too: neither check is empty."""
    st = I.fresh(I.start(30)[0])
    k32 = Z.kernel_order_fp32(st, 1e-4, 1e-4)
    s32, s64 = Z.reference(st, 1e-4, 1e-4)
    worse = I.fresh(k32)
    worse["Sigma"] = (k32["Sigma"].astype(np.float64) * (1 + 2.0 ** -19)).astype(np.float32)
    with pytest.raises(AssertionError):
        Z.hold("one digit worse", worse, st, 1e-4, 1e-4)
    bad = I.fresh(k32)
    bad["Sigma"] = k32["Sigma"].astype(np.float16).astype(np.float32)
    with pytest.raises(AssertionError, match="a-priori"):
        Z.hold("half precision", bad, st, 1e-4, 1e-4)
    assert max(I.ratios(k32, s32, s64).values()) < 1  # ... and the restatement itself passes with room


def test_braking_counter_finding():
    """Noise-free abrupt stop at N = 16: the filter reaches zero velocity by itself, and a pseudo-measurement slammed onto the FIRST still frame
    moves the position through the cross-covariances: it ends further from the truth than without.  The README's figures are these lines."""
    off, at0, at1 = Z.braking(16, None), Z.braking(16, 0), Z.braking(16, 1)
    for name, r in (("never", off), ("from still frame 0", at0), ("from still frame 1", at1)):
        print("\nZUPT-BRAKING N=16 %s: position moved in still frame 0 by %.3g, ends %.3g from the truth, |v| %.3g" % ((name,) + r))
    assert off[2] < 1e-6  # zero velocity by itself
    assert at0[1] > off[1] and at0[0] > 10 * off[0]  # the first-frame pseudo-measurement costs position
    assert at1[0] == off[0]
