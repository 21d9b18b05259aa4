"""The device-resident run, ekfvio_run_uploaded, where its captured graphs and the linearisation overlap really engage (cases and the
expectations they are held to: tests/_resident_cases.py, pinned without a GPU by tests/test_resident_cases_cpu.py).

The headline throughput is this path's: replays of captured graphs of 32, 8 and 2 filter steps, the measurement bookkeeping inside the
process(dt) launch, the frame index a device-side counter that advances modulo the sequence length, and -- in the T2 flow -- the next step's
linearisation and mean propagation inside the update's one GEMM launch.

A. Against the per-call path, bit for bit: every case is a script applied to one handle through ekfvio_run_uploaded and to a second one as
   one ekfvio_process + ekfvio_update per frame from the same start; base state, landmark means, last KLT results, deletion flags and Sigma
   must agree exactly, and the status the run's synchronize() reports must be the OR of the per-call return codes.  Every case also holds the
   handle's counters `graph_steps` and `prelinearized_steps` to what the host rule and the planner say the run must have done, so that
   no case can fall back to the eager loop (or lose the overlap) and still pass.  Covered: every sweep the graphs can contain, every cut of a
   count into graphs, the device counter's wrap inside a 32-step graph and over several laps, runs behind runs (the ping-pong flipped by an
   odd step, a per-call step in between, the same with the dense predict, another dt, dt = 0, ekfvio_set_state, another uploaded sequence, the profiler's own capture), a second live handle, a ragged
   sequence with the gate off (the eager fallback, named) and on (graphs), and EKFVIO_LIN_OVERLAP=0.
B. Against the fp64 oracle, independently of the per-call path: the two-step graph is the smallest run with a pre-linearised process(dt).

Handles are created one after another, each closed before the next (a second live handle changes the sweep; one case does that on purpose).
"""
import functools

import numpy as np
import pytest

from ekf_vio_amd import TightlyCoupledEKF, capi
from ekf_vio_amd.sim import Scenario
from oracle import OracleFilter, set_threads

import _resident_cases as RC
import _update_cases as U

pytestmark = pytest.mark.gpu

KEYS = ("base_mu", "feat_mu", "last_klt", "del_flag", "Sigma")
COUNTERS = ("graph_steps", "prelinearized_steps")


@functools.lru_cache(maxsize=None)
def compute_units():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@functools.lru_cache(maxsize=None)
def scenario(N):
    """(dt, initial features, z[frames, N, 2], R[frames, N, 4]) of the scenario the cases upload from."""
    sc = Scenario(N, seed=RC.SEED)
    uv = sc.initial_features()
    fr = list(sc.frames(RC.BASE_FRAMES if N <= 256 else RC.FRAMES))
    return sc.dt, uv, np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr])


def sequence(case, shift, frames):
    dt, uv, z, R = scenario(case.N)
    return z[shift:shift + frames], R[shift:shift + frames], RC.passes_for(case.N, case.k, frames, shift, case.ragged)


def fresh(case):
    dt, uv, _, _ = scenario(case.N)
    g = TightlyCoupledEKF(max_features=case.cap, predict_mode=capi.PREDICT_DENSE if case.dense else capi.PREDICT_STRUCTURED)
    g.addNewFeatures(uv)
    if case.gated:
        g.setGate(U.FLT_MAX)
    return g


def drive(case, resident):
    """The case's script on a handle of its own: through ekfvio_run_uploaded (resident) or frame by frame.
    Returns (state, status, counter deltas, gate totals, state before the first operation)."""
    dt = scenario(case.N)[0]
    other = fresh(case) if (case.second and resident) else None  # idle, alive on the device while the resident handle captures and runs
    g = fresh(case)
    try:
        start = g.get_state()
        z, R, p = sequence(case, 0, case.frames)
        if resident:
            g.upload_measurements(z, R, p)
        c0 = g.counters()
        status = capi.OK
        for op in case.ops:
            if op[0] == "run":
                _, first, count, scale = op
                if resident:
                    g.run_uploaded(first, count, scale * dt)
                    status |= g.synchronize()
                else:
                    for s in range(count):
                        i = (first + s) % p.shape[0]
                        g.process(scale * dt)
                        status |= g.updateWithFeaturePositions(z[i], R[i], p[i])
            elif op[0] == "step":
                g.process(dt)
                status |= g.updateWithFeaturePositions(z[op[1]], R[op[1]], p[op[1]])
            elif op[0] == "reset":
                g.set_state(start)
            elif op[0] == "upload":
                z, R, p = sequence(case, op[1], op[2])
                if resident:
                    g.upload_measurements(z, R, p)
            elif op[0] == "gemms":
                if resident:
                    g.profile_update_gemms(op[1])
            else:
                raise ValueError(op)
        c1 = g.counters()
        delta = {key: c1[key] - c0[key] for key in c1 if key != "mode"}
        return g.get_state(), status, delta, (g.gate()["gated_total"] if case.gated else None), start
    finally:
        g.close()
        if other is not None:
            other.close()


# ---------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_run_uploaded_gives_the_per_call_bits_and_took_the_graphs_it_should(monkeypatch, case):
    assert capi.OK == 0
    if case.overlap_off:
        monkeypatch.setenv("EKFVIO_LIN_OVERLAP", "0")  # read once per handle at create, and by the planner behind expected_counters
    cus = compute_units()
    dt = scenario(case.N)[0]
    want, cuts = RC.case_counters(case, cus, dt)
    sa, status_a, ca, gate_a, start = drive(case, resident=True)
    print("%s: %s; (32, 8, 2, eager) per run %s; graph_steps +%d (expected %d), prelinearized_steps +%d (expected %d)" % (
        case.id, case.label, cuts, ca["graph_steps"], want["graph_steps"], ca["prelinearized_steps"], want["prelinearized_steps"]))
    for key in COUNTERS:
        assert ca[key] == want[key], (case.id, key, ca, want, cuts)
    steps = sum(count for (_, _, count, _) in RC.walk(case))
    # the label is the flow that ran (launches are counted when enqueued OR captured: once per graph, so only "none" against "some")
    if cus == RC.CUS_MI355X and steps >= 2:
        if case.overlap_off:
            assert ca["prelinearized_steps"] == 0 and ca["graph_steps"] == steps and ca["t2_updates"] > 0, ca
        elif case.label == "overlap":
            assert ca["prelinearized_steps"] > 0 and ca["t2_updates"] > 0 and (ca["persistent"] > 0) == (not case.second), ca
        elif case.label == "T2-less persistent":
            assert ca["graph_steps"] == steps - steps % 2 and ca["persistent"] > 0 and ca["t2_updates"] == 0, ca
        elif case.label == "eager fallback":
            assert ca["graph_steps"] == 0 and ca["prelinearized_steps"] == 0, ca
            assert ca["persistent"] == steps and ca["t2_updates"] == steps, ca  # (N = 256, 254 or 256 measured: every eager update counted)
        else:  # per-step sweep, split sweep, one block column
            assert ca["graph_steps"] == steps - steps % 2 and ca["persistent"] == 0 and ca["t2_updates"] == 0, ca
    if steps == 0:  # count 0 only prepares: every bit of the state stands
        assert ca["graph_steps"] == 0
        for key in KEYS:
            assert np.array_equal(sa[key], start[key]), (case.id, "count 0 changed", key)
    sb, status_b, cb, gate_b, _ = drive(case, resident=False)
    assert cb["graph_steps"] == 0 and cb["prelinearized_steps"] == 0, cb
    for key in KEYS:
        assert np.array_equal(sa[key], sb[key]), (case.id, key, "run_uploaded against one process + update per frame")
    assert status_a == status_b and status_a in (capi.OK, capi.ENUMERIC), (case.id, status_a, status_b)
    assert np.isfinite(sa["Sigma"]).all()
    if case.gated:
        assert gate_a == gate_b, (case.id, gate_a, gate_b)


# ---------------------------------------------------------------------------------------------------------------- B
@pytest.fixture(scope="module")
def oracle_threads():
    U.use_threads()
    yield
    set_threads(1)


def two_frames(N):
    sc = Scenario(N, seed=U.SEED, dt=U.DT)
    fr = list(sc.frames(U.WARM_FRAMES + 2))
    return fr[U.WARM_FRAMES], fr[U.WARM_FRAMES + 1]


def oracle_two_steps(dtype, st0, dt, frames):
    o = OracleFilter(dtype)
    o.set_state(st0)
    info = 0
    for z, R, p in frames:
        o.process(dt)
        info |= int(o.update(z, R, p) != 0)
    st = o.get_state()
    o.close()
    return info, st


@pytest.mark.parametrize("N", [100, 256])
def test_two_step_graph_against_the_fp64_oracle(oracle_threads, N):
    """run_uploaded(0, 2) -- the pair graph: process, update (whose GEMM linearises for the next step), pre-linearised process, update --
    from the warmed fp32 state of tests/_update_cases.py, against process, update, process, update of the fp32 and fp64 oracles from that
    same state.  Bookkeeping bit-equal to the fp32 oracle; base state, landmark means and Sigma within ACC_FACTOR x the fp32 oracle's own
    error + the floors (U.ACC_FACTOR, U.MU_FLOOR, U.SIG_FLOOR), for the run and for its per-call twin.
    Measured on an MI355X, error / bound for base state, landmark means, Sigma (run and twin agree bit for bit):
    N = 100: 0.20, 0.27, 0.28; N = 256: 0.24, 0.25, 0.24."""
    dt, st0, _, frame0 = U.warmed(N)
    frames = two_frames(N)
    for a, b in zip(frames[0], frame0):
        assert np.array_equal(a, b)
    assert all(f[2].all() for f in frames)
    info32, s32 = oracle_two_steps(np.float32, st0, dt, frames)
    _, s64 = oracle_two_steps(np.float64, st0, dt, frames)
    yard = U.errors(s32, s64)
    tol = U.tolerances(s64, yard)
    z, R, p = (np.stack([f[i] for f in frames]) for i in range(3))
    got = {}
    for how in ("run", "per call"):
        g = TightlyCoupledEKF(max_features=N)
        try:
            g.set_state(st0)
            c0 = g.counters()
            if how == "run":
                g.upload_measurements(z, R, p)
                g.run_uploaded(0, 2, dt)
                rc = g.synchronize()
                c1 = g.counters()
                want = RC.expected_counters(N, N, p, 2, dt, compute_units())
                assert {key: c1[key] - c0[key] for key in COUNTERS} == want, (c0, c1, want)
                if compute_units() == RC.CUS_MI355X:
                    assert want == dict(graph_steps=2, prelinearized_steps=1)
            else:
                rc = capi.OK
                for i in range(2):
                    g.process(dt)
                    rc |= g.updateWithFeaturePositions(z[i], R[i], p[i])
            got[how] = (rc, g.get_state())
        finally:
            g.close()
    verdict = {}
    for how, (rc, st) in got.items():
        err = U.errors(st, s64)
        print("N = %d, %s: %s" % (N, how, "  ".join("%s %.3g of %.3g (%.2f of the bound, %.2f x the fp32 oracle's %.3g)" % (
            key, err[key], tol[key], err[key] / tol[key], err[key] / max(yard[key], 1e-300), yard[key]) for key in tol)))
        verdict[how] = {key: err[key] <= tol[key] for key in tol}
    for how, (rc, st) in got.items():
        assert np.array_equal(st["del_flag"], s32["del_flag"]) and np.array_equal(st["last_klt"], s32["last_klt"]), how
        assert (rc == capi.OK) == (info32 == 0) and rc in (capi.OK, capi.ENUMERIC), (how, rc, info32)
    assert all(verdict["run"].values()), ("the run misses the bound", verdict, "(the per-call twin's verdict tells whose failure it is)")
    assert all(verdict["per call"].values()), ("the per-call twin misses the bound", verdict)
