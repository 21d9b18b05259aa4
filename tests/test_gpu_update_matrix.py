"""The measurement update against the fp64 oracle in every flow, row count and R shape (cases: tests/_update_cases.py).

The update is the one part of the product that is not bit-exact by construction, and since plan_update (plan.h) it takes one of several
kernel flows chosen from the number of rows measured IN THAT FRAME.  The rest of the suite compares it with an independent reference almost
only at "everything measured", with a constant diagonal R, and otherwise HIP against HIP.  Here: one teacher-forced update per case from a
dense warmed state, evaluated by the HIP kernels, the fp32 oracle and the fp64 oracle from identical fp32 inputs,
  * at both edges of every boundary between flows for N = 100, 256, 400, 600 (and a capacity above N), with four layouts of the failed
    landmarks, host-sized and device-sized (the gate at FLT_MAX: planned for m = 2N, most block columns identity padding);
  * with R diagonal but uneven, full symmetric, and NON-symmetric (the sample-based path's blocks with fx != fy), which the kernels read
    in a dozen places with two index conventions;
and per case
  * bookkeeping bit-equal to the fp32 oracle, the return code OK exactly when the fp32 oracle meets no non-positive pivot;
  * base state, landmark means and Sigma within ACC_FACTOR x (the fp32 oracle's worst error over six landmark orderings) + floor of the
    fp64 result -- the constants of tests/test_gpu_parity.py, the triangle form of tests/test_gpu_gate.py for N > 334;
  * every measured landmark's mean moves towards its z (where it does in fp64), which names a landmark when a block column is mixed up;
  * THE FLOW THAT RAN, from the handle's counters and profiler classes, equals the one the case table expects, so that the coverage
    this module claims cannot rot silently; the closing test checks that the cases cover every flow of the table.
tests/test_update_matrix_cpu.py shows without a GPU that the defects in view (R transposed, off-diagonals dropped, u and v swapped, a
neighbour's R, a pass mask off by one landmark) move the fp64 answer by at least ten of these tolerances.

Each handle is closed before the next is created (a second live handle moves every update to the per-step sweep).
"""
import numpy as np
import pytest

from ekf_vio_amd import TightlyCoupledEKF, capi
from ekf_vio_amd.sim import Scenario
from oracle import OracleFilter, set_threads

import _update_cases as U
from _update_run import check_against_oracles, hip_update, run_case  # (shared with tests/test_gpu_update_history.py)

pytestmark = pytest.mark.gpu

RAN = {}  # case -> the flow signature observed, for the closing test


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    """The oracle's OpenMP products on up to 16 cores while this module runs (U.use_threads), one again behind it."""
    U.use_threads()
    yield
    set_threads(1)


@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_update_against_the_fp64_oracle(case):
    N, cap, k, layout, sizing, kind = case
    dt, st0, sp, z, R, p = U.inputs(N, k, layout, kind)
    ref = U.reference(N, k, layout, kind)
    y = (z - sp["feat_mu"][:, :2])[p.astype(bool)]
    assert np.abs(y).max() > 0
    rc, got, gate, sig = run_case(case)
    RAN[case] = sig
    flow = U.expected_flow(N, cap, sizing, k)
    assert sig == U.SIGNATURE[flow], (U.case_id(case), "expected", flow, U.SIGNATURE[flow], "ran (persistent, solve, gemm_update, t2)", sig)
    check_against_oracles(U.case_id(case), sp, z, p, rc, got, ref)
    if sizing == "device":
        # nothing gated, and the bookkeeping of the host-sized twin bit for bit.  (The state's bits need not agree: the two plans differ
        # wherever the count does not fill the last block column of m = 2N, and both are held to the fp64 result above.)
        assert gate["gated_last"] == 0 and gate["n_landmarks"] == N and not gate["gated"].any()
        _, twin, _, _ = run_case((N, cap, k, layout, "host", kind))
        assert np.array_equal(got["del_flag"], twin["del_flag"]) and np.array_equal(got["last_klt"], twin["last_klt"])


def test_one_step_n1024_with_non_symmetric_r():
    """The shape of tests/test_gpu_shapes.py::test_teacher_forced_one_step_n1024 (start state made the same way: three HIP steps from a
    tightened prior, dense and well conditioned; split look-ahead sweep, gain GEMM, two Joseph GEMMs) with R of kind "d"."""
    N = 1024
    U.use_threads()
    sc = Scenario(N, seed=0)
    g = TightlyCoupledEKF(max_features=N)
    try:
        g.addNewFeatures(sc.initial_features())
        st = g.get_state()
        d = np.diag(st["Sigma"]).copy()
        d[7:16] = 0.05
        d[24::3] = 1.0
        st["Sigma"] = np.diag(d).astype(np.float32)
        st["base_mu"][7:10] = (-0.1, 0.0, -0.1)
        st["base_mu"][10:13] = (0.0, 0.1, 0.0)
        g.set_state(st)
        frames = list(sc.frames(4))
        for z, R, p in frames[:3]:
            g.process(sc.dt)
            assert g.updateWithFeaturePositions(z, R, p) == capi.OK
        st0 = g.get_state()
    finally:
        g.close()
    assert np.isfinite(st0["Sigma"]).all() and np.count_nonzero(st0["Sigma"]) > 0.9 * st0["Sigma"].size
    z, Rs, _ = frames[3]
    R = U.make_R("d", N, Rs)
    p = U.pass_mask(N, 1020, "every")
    o = OracleFilter(np.float32)
    o.set_state(st0)
    o.process(sc.dt)
    sp = o.get_state()
    o.close()
    rc, got, _, sig = hip_update(N, st0, sp, sc.dt, z, R, p, False)
    assert sig == U.SIGNATURE[("split", "launch", "joseph")], sig
    check_against_oracles("N1024-k1020-every-host-Rd", sp, z, p, rc, got, U.make_reference(sp, z, R, p))


def test_the_cases_cover_every_flow_of_the_table():
    """Host- and device-sized: every (sweep, gain, tail) the table lists is the expected flow of at least one case, and every case that ran
    in this session ran it (asserted per case above; listed here)."""
    listed = {(s, f) for (_, _, s, _, _, f) in U.FLOWS}
    hit = {}
    for c in U.CASES:
        N, cap, k, layout, sizing, kind = c
        hit.setdefault((sizing, U.expected_flow(N, cap, sizing, k)), []).append(c)
    for key in sorted(listed):
        cases = hit.get(key, [])
        ran = [c for c in cases if c in RAN]
        print("%-6s %-30s %2d cases, %2d ran here" % (key[0], "/".join(key[1]), len(cases), len(ran)))
        assert cases, ("no case expects", key)
        for c in ran:
            assert RAN[c] == U.SIGNATURE[key[1]], (U.case_id(c), RAN[c])
    assert set(hit) == listed
    for kind in "bcd":  # every R kind meets every flow, host-sized, that N = 256 and N = 400 have
        flows = {U.expected_flow(N, cap, s, k) for (N, cap, k, _, s, r) in U.CASES if r == kind and s == "host" and N in (256, 400)}
        assert flows == {f for (n, c, s, _, _, f) in U.FLOWS if s == "host" and n in (256, 400) and c == n}, (kind, flows)
