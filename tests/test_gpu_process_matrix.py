"""process(dt) against its oracle in every launch form, size and state (cases, references and criteria: tests/_process_cases.py; what the
cases can see: tests/test_process_cases_cpu.py).

process(dt) runs in front of every update and every other parity statement leans on it, yet it had met the oracle only at N = 0, 3, 12, 30,
100, 256 and 1024, always on a handle filled to its capacity, from the scenario's near-identity states, at dt = 0.05 or 0.1.  Here, per
case: set_state of ONE fp32 state, one or two process(dt) calls, get_state, on a handle of its own.
  * Structured forms -- predict_fused_kernel<true> ("inside"), linearize_kernel + predict_fused_kernel<false> ("front",
    EKFVIO_FUSE_LINEARIZE=0), and whichever of the two the planner takes at N = 512 and 513 -- give the fp32 oracle's process(dt) in every bit
    of base_mu, feat_mu and Sigma; a mismatch names the count, the first element and the workgroup (base block, base-row chunk c,
    base-column chunk c, tile (tI, tJ)).  Sizes on and beside every edge of the launch (PREDICT_PC = 3, LIN_LM = 8, PREDICT_PT = 16,
    n = 64, ld == n + 1), three handles whose capacity exceeds N behind a camera update (two consecutive calls: P -> P2 -> P), eight
    states at four dt, and a covariance scaled so that every predict_finish site both prunes and keeps.
  * Dense form: means bit for bit; every element of Sigma within 2 (22 + 4) * 6e-8 * (|F| |P| |F|^T + Q) + 1e-13 of E = prune(F P F^T + Q)
    in fp64 with the fp32 oracle's F, and 0 or above the flush threshold.  The figure max |got - E| / (6e-8 mag) is printed per case.
  * The riding linearisation ("pre"): run_uploaded(0, 4, dt) against four per-call process + update pairs, bit for bit, at five N the
    planner gives the T2 tail, with prelinearized_steps asserted.
  * numericallyLinearizeProcess at N = 7, 8, 9, 33 against the oracle's linearize, bit for bit; process(-0.05) and process(nan) refused
    with every bit of the state left.

MEASURED ON THE MI355X (256 compute units; every N up to 512 linearised inside, 513 in front): all 112 structured cases bit-identical to
the fp32 oracle; the dense form's worst |got - E| / (6e-8 mag), of 52 allowed, with the fp32 oracle's own figure in that case in brackets:
family dense 7.12 (8.02) at N = 513, dt = 0.05; family flush 0.75 (0.75).  Per case: _process_cases' docstring and DESIGN.md section 5.

Each handle is closed before the next is created (the persistent sweep is for a device's sole handle).
"""
import functools

import numpy as np
import pytest

from ekf_vio_amd import EkfvioError, TightlyCoupledEKF, capi
from ekf_vio_amd.sim import Scenario
from oracle import set_threads

import _process_cases as P
import _resident_cases as RC

pytestmark = pytest.mark.gpu

KEYS = ("base_mu", "feat_mu", "last_klt", "del_flag", "Sigma")
WORST = {}  # family -> (largest dense figure of the HIP path so far, the fp32 oracle's in that case, the case): printed, never asserted


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    P.use_threads()
    yield
    set_threads(1)


@functools.lru_cache(maxsize=None)
def compute_units():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def set_form(monkeypatch, form):
    """The launch form is a switch read once per handle, in ekfvio_create (and by the planner behind predict_plan)."""
    if form == "front":
        monkeypatch.setenv("EKFVIO_FUSE_LINEARIZE", "0")
    else:
        monkeypatch.delenv("EKFVIO_FUSE_LINEARIZE", raising=False)


def run_case(case):
    """(the state after each process(dt), dim, num_features) of the case on a handle of its own."""
    st = P.inputs(case)
    h = TightlyCoupledEKF(max_features=P.handle_capacity(case), predict_mode=capi.PREDICT_DENSE if case.form == "dense" else capi.PREDICT_STRUCTURED)
    try:
        if case.camera_first:  # P2 / Fdense / FA / FB / FD and column n hold a camera step's leftovers, and ld > n + 1
            st0, frame = P.start(case.N)
            h.set_state(st0)
            h.process(P.DT)
            assert h.updateWithFeaturePositions(*frame) in (capi.OK, capi.ENUMERIC)
        h.set_state(st)
        out = []
        for _ in range(case.steps):
            h.process(case.dt)
            out.append(h.get_state())
        return out, h.dim, h.num_features
    finally:
        h.close()


def assert_bookkeeping(case, got, dim, num):
    st = P.inputs(case)
    assert dim == P.BASE + 3 * case.N and num == case.N
    for s in got:
        assert np.array_equal(s["last_klt"], st["last_klt"]) and np.array_equal(s["del_flag"], st["del_flag"])
        assert s["Sigma"].shape == (dim, dim) and s["feat_mu"].shape == (case.N, 3)


@pytest.mark.parametrize("case", P.STRUCTURED, ids=P.case_id)
def test_structured_process_gives_the_fp32_oracles_bits(monkeypatch, case):
    set_form(monkeypatch, case.form)
    ran = P.form_name(P.predict_plan(case.N, compute_units()))
    print("\n%s: %d compute units, the planner takes the form \"%s\"" % (P.case_id(case), compute_units(), ran))
    if case.form != "default" and compute_units() == P.CUS_MI355X:
        assert ran == case.form
    s32, _ = P.reference(case)
    got, dim, num = run_case(case)
    for step, (g, want) in enumerate(zip(got, s32)):
        bad = P.mismatch(g, want)
        assert bad is None, "%s, process(dt) call %d, form %s: %s" % (P.case_id(case), step + 1, ran, bad)
    assert_bookkeeping(case, got, dim, num)


@pytest.mark.parametrize("case", P.DENSE, ids=P.case_id)
def test_dense_process_within_the_gemm_bound_of_the_fp64_product(case):
    s32, _ = P.reference(case)
    E, mag, bound = P.dense_reference(case)
    got, dim, num = run_case(case)
    g = got[0]
    for key in ("base_mu", "feat_mu"):  # the same linearize_kernel
        assert np.array_equal(g[key], s32[0][key]), P.mismatch(g, dict(s32[0], Sigma=g["Sigma"]))
    S = g["Sigma"]
    assert np.isfinite(S).all()
    units, own = P.dense_units(S, case), P.dense_units(s32[0]["Sigma"], case)
    print("\nDENSE-UNITS %s: HIP %.2f, fp32 oracle %.2f, of %d" % (P.case_id(case), units, own, P.DENSE_UNITS))
    if units >= WORST.get(case.family, (-1.0,))[0]:
        WORST[case.family] = (units, own, P.case_id(case))
    print("DENSE-WORST so far, family %s: HIP %.2f (fp32 oracle there: %.2f) in %s" % ((case.family,) + WORST[case.family]))
    err = np.abs(S.astype(np.float64) - E)
    over = np.argwhere(err > bound)
    assert over.shape[0] == 0, (P.case_id(case), over.shape[0], "elements outside the bound, the first at", tuple(over[0]),
                                P.region_of(*over[0]), "error", err[tuple(over[0])], "allowed", bound[tuple(over[0])], "units", units)
    small = np.argwhere((S != 0) & ~(np.abs(S) > P.FLUSH))
    assert small.shape[0] == 0, (P.case_id(case), small.shape[0], "entries below the flush threshold survive, the first at", tuple(small[0]))
    assert_bookkeeping(case, got, dim, num)


@pytest.mark.parametrize("N", P.LINEARIZE_NS)
def test_linearize_kernel_gives_the_oracles_jacobian_bits(N):
    """ekfvio_linearize: the stand-alone linearize_kernel (LIN_LM = 8 landmarks per workgroup) at N = 7, 8, 9 and 33."""
    case = P.Case("size", N, N, "rotated", P.DT, "inside", False, 1, 0)
    assert case in P.CASES
    want, _ = P.jacobian(case)
    h = TightlyCoupledEKF(max_features=N)
    try:
        h.set_state(P.inputs(case))
        got = h.numericallyLinearizeProcess(case.dt)
    finally:
        h.close()
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (N, bad.shape[0], "elements of F differ, the first at", tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("N", P.RIDING_CANDIDATES)
def test_riding_linearisation_gives_the_per_call_bits(N):
    """The `pre` form: inside a device-resident run the update's last GEMM linearises for the next process(dt), which is then
    predict_fused_kernel<false> alone.  Four frames are two replays of the two-step graph: two pre-linearised steps."""
    cus = compute_units()
    sc = Scenario(N, seed=P.SEED)
    fr = list(sc.frames(4))
    z, R, p = (np.stack([f[i] for f in fr]) for i in range(3))
    want = RC.expected_counters(N, N, p, 4, sc.dt, cus)
    if cus == P.CUS_MI355X:
        assert want == dict(graph_steps=4, prelinearized_steps=2), want  # (pinned without a GPU by test_process_cases_cpu.py)
    a = TightlyCoupledEKF(max_features=N)
    try:
        a.addNewFeatures(sc.initial_features())
        a.upload_measurements(z, R, p)
        c0 = a.counters()
        a.run_uploaded(0, 4, sc.dt)
        status_a = a.synchronize()
        c1 = a.counters()
        sa = a.get_state()
    finally:
        a.close()
    b = TightlyCoupledEKF(max_features=N)
    try:
        b.addNewFeatures(sc.initial_features())
        status_b = capi.OK
        for i in range(4):
            b.process(sc.dt)
            status_b |= b.updateWithFeaturePositions(z[i], R[i], p[i])
        sb = b.get_state()
    finally:
        b.close()
    delta = {k: c1[k] - c0[k] for k in want}
    print("\nN = %d on %d compute units: %s (expected %s)" % (N, cus, delta, want))
    assert delta == want and status_a == status_b
    if cus == P.CUS_MI355X:
        assert c1["prelinearized_steps"] > c0["prelinearized_steps"]
    for key in KEYS:
        bad = np.argwhere(sa[key] != sb[key])
        assert bad.shape[0] == 0, (N, key, bad.shape[0], "elements differ, the first at", tuple(bad[0]),
                                   P.region_of(*bad[0]) if key == "Sigma" else "")


@pytest.mark.parametrize("dt", [-0.05, float("nan")])
def test_process_refuses_a_negative_or_nan_dt_and_leaves_the_state(dt):
    case = P.Case("state", P.STATE_N, P.STATE_N, "rotated", P.DT, "inside", False, 1, 0)
    assert case in P.CASES
    h = TightlyCoupledEKF(max_features=case.cap)
    try:
        h.set_state(P.inputs(case))
        before = h.get_state()
        with pytest.raises(EkfvioError) as e:
            h.process(dt)
        assert e.value.code == capi.EINVAL
        after = h.get_state()
        for key in KEYS:
            assert np.array_equal(before[key], after[key]), key
            assert np.array_equal(after[key], P.inputs(case)[key]), key
        # ... and the handle is as good as before: the next process(dt) gives the oracle's bits
        h.process(case.dt)
        assert P.mismatch(h.get_state(), P.reference(case)[0][0]) is None
    finally:
        h.close()
