"""One teacher-forced update of tests/_update_cases.py on the GPU, shared by tests/test_gpu_update_matrix.py (a handle of its own per case) and
tests/test_gpu_update_history.py (the same step on a handle that has run other updates before).  A plain module, imported like _update_cases.py;
importing it needs no GPU, calling it does."""
import functools

import numpy as np

from ekf_vio_amd import TightlyCoupledEKF, capi

import _update_cases as U

KEYS = ("base_mu", "feat_mu", "last_klt", "del_flag", "Sigma")


def step_on(g, st0, sp, dt, z, R, p, device_sized, fill=None):
    """set_state(st0), process(dt) (bit-equal to `sp`, the fp32 oracle's; sp None: not compared) and the update on the handle g, whatever g ran before.
    fill: the word ekfvio_test_fill_update_scratch writes in front of process(dt) and again in front of the update (hooks build).  A device-sized step
    switches the gate on (FLT_MAX) and off again.  Returns (rc, state, gate, signature, propagated state)."""
    g.set_state(st0)
    if device_sized:
        g.setGate(U.FLT_MAX)
    if fill is not None:
        g.fill_update_scratch(fill)
    g.process(dt)
    prop = g.get_state()
    if sp is not None:
        for key in KEYS:
            assert np.array_equal(prop[key], sp[key]), ("process(dt) against the fp32 oracle", key)
    if fill is not None:
        g.fill_update_scratch(fill)
    g.profile(1)
    c0 = g.counters()
    rc = g.updateWithFeaturePositions(z, R, p)
    c1, rep = g.counters(), g.profile_report()
    g.profile(0)
    sig = (c1["persistent"] - c0["persistent"], rep["solve"]["launches"], rep["gemm_update"]["launches"],
           c1["t2_updates"] - c0["t2_updates"])
    got = g.get_state()
    gate = None
    if device_sized:
        gate = g.gate()
        g.setGate(0.0)
    return rc, got, gate, sig, prop


def hip_update(cap, st0, sp, dt, z, R, p, device_sized, **handle_kw):
    """process(dt) (bit-equal to the fp32 oracle's `sp`) and the update on a handle of its own.  Returns (rc, state, gate, signature)."""
    g = TightlyCoupledEKF(max_features=cap, **handle_kw)
    try:
        return step_on(g, st0, sp, dt, z, R, p, device_sized)[:4]
    finally:
        g.close()


@functools.lru_cache(maxsize=None)
def run_case(case):
    N, cap, k, layout, sizing, kind = case
    dt, st0, sp, z, R, p = U.inputs(N, k, layout, kind)
    return hip_update(cap, st0, sp, dt, z, R, p, sizing == "device")


def check_against_oracles(what, sp, z, p, rc, got, ref):
    """Section 2 of test_gpu_update_matrix.py's docstring for one result; prints each figure before it asserts."""
    s64 = ref["s64"]
    assert np.array_equal(got["del_flag"], ref["del_flag32"]) and np.array_equal(got["last_klt"], ref["last_klt32"]), what
    assert (rc == capi.OK) == (ref["info32"] == 0) and rc in (capi.OK, capi.ENUMERIC), (what, rc, ref["info32"])
    assert abs(np.linalg.norm(got["base_mu"][3:7].astype(np.float64)) - 1) < 1e-6, what
    assert np.isfinite(got["Sigma"]).all() and np.isfinite(got["feat_mu"]).all() and np.isfinite(got["base_mu"]).all(), what
    err, tol = U.errors(got, s64), U.tolerances(s64, ref["scatter"])
    print("%s: %s" % (what, "  ".join("%s %.3g of %.3g" % (key, err[key], tol[key]) for key in tol)))
    for key in tol:
        assert err[key] <= tol[key], (what, key, err[key], tol[key], ref["scatter"])
    # every measured landmark moves towards its measurement, where the fp64 evaluation says it does
    in64 = U.moves_towards_z(sp, s64, z, p)
    assert (~in64).sum() <= 0.05 * p.sum(), (what, "the inputs do not support this check", np.nonzero(~in64)[0])
    bad = np.nonzero(in64 & ~U.moves_towards_z(sp, got, z, p))[0]
    assert bad.size == 0, (what, "landmarks that moved away from their measurement", bad[:16], "state rows", U.BASE + 3 * bad[:16])
