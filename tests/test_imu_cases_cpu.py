"""The cases of tests/test_gpu_imu_matrix.py would notice (no GPU needed: the oracles and numpy alone).

The criterion of tests/_imu_cases.py means something only if the defects in view move the answer by more than it allows.  Each of
_imu_cases.DEFECTS -- a quaternion column of the accelerometer rows of H zeroed, the d/dw column's sign, the e_k x uv or the c x ev term
dropped, the (x, y, z) part transposed, the residual formed with + R(q)^T g, the bias columns exchanged, the variances exchanged, the
quaternion left un-normalised, gravity's components rotated by one place -- is put into the numpy fp64 evaluation with the analytic H, and
must move some quantity of the criterion by MARGIN = 10 tolerances in at least one case of the families "attitude" and "reading".  Run
with -s for the table; _imu_cases.SENSITIVITY records it.

Also here: the control case (identity attitude, gravity along y: the regime of tests/test_gpu_imu.py) does NOT see the d/dw, d/dy and
e_k x uv defects, which is why the attitude family exists; for every case the fp32 oracle meets the criterion with ACC_FACTOR = 1 (by
construction of the criterion this holds whenever its result is finite: it excludes a case whose fp32 evaluation breaks down), imu.hip's
order of operations restated in numpy fp32 meets it as the GPU test states it (a second honest fp32 rounding order: a case that rounding
order alone would fail is excluded), and S is comfortably positive definite in fp64.
"""
import numpy as np
import pytest

from oracle import OracleFilter, set_threads

import _imu_cases as I

SEEN = [c for c in I.CASES if c.family in ("attitude", "reading")]
COND_S_MAX = 1e5  # fp32 carries 7 digits: a Cholesky of S keeps two or more


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    I.use_threads()
    yield
    set_threads(1)


def defective(case, defect):
    st, gyro, acc, gv, av, g = I.inputs(case)
    out = I.np_imu_update(st["base_mu"], st["feat_mu"], st["Sigma"], gyro, acc, float(gv), float(av), g, "analytic", defect)
    return I.np_state(out, st)


def worst(r):
    k = max(r, key=r.get)
    return r[k], k


def test_the_case_table_is_sound():
    assert len(I.CASES) == len(set(I.CASES)) == 21 + 10 + 5
    assert len({I.case_id(c) for c in I.CASES}) == len(I.CASES)
    assert I.CONTROL in I.CASES
    att = [c for c in I.CASES if c.family == "attitude"]
    assert {(c.quat, c.grav) for c in att} == {(q, g) for q in I.QUATS for g in I.GRAVS}
    for name, q in I.QUATS.items():
        norm = np.linalg.norm(q)
        assert abs(norm - {"1.03u": 1.03, "0.97u": 0.97}.get(name, 1.0)) < 1e-12
    assert I.QUATS["-u"][0] < 0 and I.QUATS["w0"][0] == 0
    sizes = sorted({22 + 3 * c.N for c in I.CASES if c.family == "size"})
    assert sizes == [22, 25, 112, 253, 256, 259, 511, 514, 1222]
    for c in I.CASES:  # the start state really carries the case's quaternion, and nothing but fp32 numbers goes in
        st, gyro, acc, gv, av, g = I.inputs(c)
        assert np.array_equal(st["base_mu"][3:7], I.QUATS[c.quat].astype(np.float32))
        assert all(a.dtype == np.float32 for a in (st["base_mu"], st["feat_mu"], st["Sigma"], gyro, acc, g))
        assert st["feat_mu"].shape[0] == c.N and c.cap >= c.N
        if c.N >= 30:  # (the bias rows start uncorrelated with the rest and stay so)
            S = st["Sigma"]
            assert np.count_nonzero(S) > 0.8 * S.size, "the start covariance is not dense"


def test_the_readings_are_what_the_case_says():
    for c in I.CASES:
        st, gyro, acc, gv, av, g = I.inputs(c)
        y = np.concatenate([gyro, acc]).astype(np.float64) - I.h_imu(st["base_mu"].astype(np.float64), g.astype(np.float64))
        s32, s64 = I.reference(c)
        if c.reading == "zero":
            # exactly zero in the fp32 specification: every mean but the quaternion keeps its bits, the quaternion is only renormalised
            keep = np.r_[0:3, 7:22]
            assert np.array_equal(s32["base_mu"][keep], st["base_mu"][keep]) and np.array_equal(s32["feat_mu"], st["feat_mu"])
            assert np.abs(y).max() < 1e-5
            q = st["base_mu"][3:7].astype(np.float64)
            assert np.abs(s32["base_mu"][3:7] - q / np.linalg.norm(q)).max() < 2e-7
        elif c.reading == "large":
            assert np.allclose(y, np.concatenate(I.LARGE_OFFSET), rtol=0, atol=1e-5)
            q = st["base_mu"][3:7].astype(np.float64)
            assert np.abs(s64["base_mu"][3:7] - q / np.linalg.norm(q)).max() > 1e-4  # the attitude itself moves, by a thousand fp32 units
        else:
            assert 1e-3 < np.abs(y[:3]).max() < 5e-2 and 1e-2 < np.abs(y[3:]).max() < 5e-1


@pytest.mark.parametrize("case", I.CASES, ids=I.case_id)
def test_case_is_sound_in_fp64_and_fp32(case):
    st, gyro, acc, gv, av, g = I.inputs(case)
    s32, s64 = I.reference(case)
    # the independent evaluation agrees with the specification: numeric and analytic H
    tol = I.tolerances(s32, s64)
    for jac in ("numeric", "analytic"):
        out = I.np_imu_update(st["base_mu"], st["feat_mu"], st["Sigma"], gyro, acc, float(gv), float(av), g, jac)
        r = I.ratios(I.np_state(out, st), s32, s64)
        assert max(r.values()) < 0.05, (jac, r)
    # S comfortably positive definite
    ev = np.linalg.eigvalsh(out["S"])
    assert ev[0] >= 0.99 * min(float(gv), float(av)) and ev[-1] / ev[0] < COND_S_MAX, ev
    # the fp32 oracle alone, ACC_FACTOR = 1
    for k in I.QUANTITIES:
        assert np.isfinite(tol[k])
    r1 = I.ratios(s32, s32, s64, factor=1.0)
    assert all(np.isfinite(v) and v <= 1.0 for v in r1.values()), r1
    # a second honest fp32 rounding order: the kernel's, restated in numpy
    rk = I.ratios(I.kernel_order_fp32(st, gyro, acc, gv, av, g), s32, s64)
    e32 = I.errors(s32, s64)
    print("\n%-44s cond S %8.3g  fp32 oracle: base %.2g quat rows %.2g elementwise %.2g   kernel order / tolerance: %s"
          % (I.case_id(case), ev[-1] / ev[0], e32["base"], e32["sig_quat_rows"] / max(I._size(*I.quantities(s64)["sig_quat_rows"]), 1e-300),
             e32["sig_elementwise"], "  ".join("%s %.2f" % kv for kv in rk.items())))
    assert max(rk.values()) <= 1.0, rk


@pytest.fixture(scope="module")
def table():
    """defect -> list of (largest ratio over the quantities, the quantity, the case) over SEEN."""
    out = {}
    for d in I.DEFECTS:
        rows = []
        for c in SEEN:
            s32, s64 = I.reference(c)
            r, k = worst(I.ratios(defective(c, d), s32, s64))
            rows.append((r, k, c))
        out[d] = rows
    return out


def test_every_defect_moves_the_fp64_result_by_ten_tolerances_somewhere(table):
    print("\n%-28s %-10s %-44s %s" % ("defect", "largest", "in case (quantity)", "cases at or above MARGIN"))
    short = []
    for d in I.DEFECTS:
        rows = table[d]
        r, k, c = max(rows, key=lambda t: t[0])
        seen = sum(1 for t in rows if t[0] >= I.MARGIN)
        print("%-28s %-10.3g %-44s %d of %d" % (d, r, "%s (%s)" % (I.case_id(c), k), seen, len(rows)))
        if r < I.MARGIN:
            short.append((d, r))
    assert not short, short


def test_every_attitude_away_from_the_control_sees_the_jacobian(table):
    """Printed per defect: the smallest ratio over the generic-gravity attitudes other than the identity -- not one lucky case."""
    print()
    for d in I.JACOBIAN_DEFECTS:
        rows = [t for t in table[d] if t[2].family == "attitude" and t[2].grav == "ggen" and t[2].quat in ("1.03u", "0.97u", "-u")]
        r, k, c = min(rows, key=lambda t: t[0])
        print("%-28s smallest over +-u, generic gravity: %-10.3g %s (%s)" % (d, r, I.case_id(c), k))
        assert r >= I.MARGIN, (d, r, I.case_id(c))


def test_the_control_attitude_is_blind_to_what_the_family_is_for(table):
    print()
    for d in I.BLIND_AT_CONTROL:
        (r, k, c), = [t for t in table[d] if t[2] == I.CONTROL]
        print("%-28s at the control (identity, g along y): %.3g tolerances (%s)" % (d, r, k))
        assert r < 1.0, (d, r, k)  # it would pass the criterion there
