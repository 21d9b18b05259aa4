"""An update's result does not depend on what the handle ran before (tables: tests/_history_cases.py, checked by tests/test_update_history_cpu.py).

The rest of the suite holds the update to the fp64 oracle on handles that have never run anything else (tests/test_gpu_update_matrix.py: one
handle per case, every work buffer still the zero fill of its allocation), or compares two handles with the SAME history.  A real handle takes
another flow whenever the row count crosses a boundary, and all flows share Saug, Laug, Linv, Km, Wt, Gm, Rm, yres, idx, inv_idx, Lsign and the
dense-F buffer; the kernels' contracts lean on padding that is zero on a fresh handle whether or not anything maintains it.  Two ways that cover
each other's blind side:

1. Filled scratch (hooks build).  ekfvio_test_fill_update_scratch writes one word into every float work buffer in front of process(dt) and again
   in front of the update: a quiet NaN (0x7fc00000), and 1.5f (0x3fc00000: the prune of the GEMM epilogue turns a NaN into 0 and would hide it;
   1.5 is large against a warmed Sigma).  One representative per row of U.FLOWS.  The state behind process(dt) is the fp32 oracle's bit for bit;
   the return code and the state behind the update are those of a fresh hooks handle that was never filled; the flow is the table's.  The first
   test shows that two fresh handles agree bit for bit, so that a later mismatch means history, not irreproducibility.
2. Predecessor x successor (product build).  One handle per (group, predecessor) runs, for every successor of its group, the predecessor and then
   the successor; the successor's return code, state and flow are those of a fresh handle (for G1 - G5: _update_run.run_case, which
   test_gpu_update_matrix.py holds to the fp64 oracle; for the handles of another capacity or predict mode a twin run and held to the oracles
   here).  The integer buffers (stale but in-range indices) and non-finite leftovers (the exactly singular update) are reached this way only.
   Behind the successors of G2 and the N = 256 ones of G6 the filter grows by eight landmarks and runs three rounds of process(dt) and an
   all-passed update (the growth tail).  Every step of a pair starts with ekfvio_set_state, which zeroes both covariance buffers outside n x n, so
   the fresh twin alone cannot show non-zero padding of P or a K y left in column n: the twin's tail is also run "laundered", with
   ekfvio_set_state(ekfvio_get_state()) behind every entry point, and must give the same bits.

Only one handle is alive at a time (a second one moves every update to the per-step sweep, which the flow assertion would report).  Nothing here
injects a fault, fills an integer or flag buffer, or waits.
"""
import functools

import numpy as np
import pytest

from ekf_vio_amd import TightlyCoupledEKF, capi
from ekf_vio_amd.sim import Scenario
from oracle import OracleFilter, set_threads

import _history_cases as H
import _update_cases as U
from _update_run import KEYS, check_against_oracles, run_case, step_on

pytestmark = pytest.mark.gpu

WORDS = (0x7FC00000, 0x3FC00000)  # quiet NaN, 1.5f
REPRESENTATIVES = H.representatives()


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    U.use_threads()
    yield
    set_threads(1)


def differing(a, b):
    """The keys of two states whose bits differ, with the number of elements (bit-equal: NaN equals the same NaN, 0 differs from -0)."""
    out = []
    for key in KEYS:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        if x.shape != y.shape or x.dtype != y.dtype:
            out.append((key, "shape", x.shape, y.shape))
        elif x.tobytes() != y.tobytes():
            d = x.view(np.uint8).reshape(x.shape + (-1,)) != y.view(np.uint8).reshape(y.shape + (-1,))
            where = np.argwhere(d.any(axis=-1))
            out.append((key, int(d.any(axis=-1).sum()), "first at", tuple(int(v) for v in where[0]), "last at", tuple(int(v) for v in where[-1])))
    return out


def handle(cap, hooks=False, dense=False):
    return TightlyCoupledEKF(max_features=cap, hooks=hooks, predict_mode=capi.PREDICT_DENSE if dense else capi.PREDICT_STRUCTURED)


# ------------------------------------------------------------------------------------------------------------ 1. filled scratch
def hooks_update(case, fill=None):
    N, cap, k, layout, sizing, kind = case
    dt, st0, sp, z, R, p = U.inputs(N, k, layout, kind)
    g = handle(cap, hooks=True)
    try:
        rc, got, _, sig, _ = step_on(g, st0, sp, dt, z, R, p, sizing == "device", fill=fill)
    finally:
        g.close()
    return rc, got, sig


@functools.lru_cache(maxsize=None)
def never_filled(case):
    return hooks_update(case)


@pytest.mark.parametrize("case", REPRESENTATIVES, ids=U.case_id)
def test_two_fresh_handles_agree_bit_for_bit(case):
    rc, got, sig = never_filled(case)
    rc2, got2, sig2 = hooks_update(case)
    assert (rc, sig) == (rc2, sig2) and not differing(got, got2), (U.case_id(case), rc, rc2, sig, sig2, differing(got, got2))


@pytest.mark.parametrize("word", WORDS, ids=["nan", "1.5"])
@pytest.mark.parametrize("case", REPRESENTATIVES, ids=U.case_id)
def test_update_does_not_see_filled_work_buffers(case, word):
    N, cap, k, layout, sizing, kind = case
    rc0, want, _ = never_filled(case)
    rc, got, sig = hooks_update(case, fill=word)  # (asserts process(dt) against the fp32 oracle between the two fills)
    flow = U.expected_flow(N, cap, sizing, k)
    assert sig == U.SIGNATURE[flow], (U.case_id(case), "expected", flow, "ran (persistent, solve, gemm_update, t2)", sig)
    assert rc == rc0 and not differing(got, want), (U.case_id(case), "filled with 0x%08x" % word, rc, rc0, differing(got, want))


# ------------------------------------------------------------------------------------------------------------ 2. predecessor x successor
@functools.lru_cache(maxsize=None)
def singular_inputs(N):
    """tests/test_gpu_shapes.py::test_exactly_singular_s_is_flagged_and_never_hangs: zero prior, zero measurement noise."""
    sc = Scenario(N, seed=3)
    z, R, p = list(sc.frames(1))[0]
    o = OracleFilter(np.float32)
    o.add_new_features(sc.initial_features())
    st = o.get_state()
    o.close()
    return {**st, "Sigma": np.zeros_like(st["Sigma"])}, z, np.zeros_like(R), p


@functools.lru_cache(maxsize=None)
def resident_inputs(N):
    """The warmed state of the cases and the scenario's next RESIDENT_FRAMES frames, every landmark passed."""
    dt, st0, _, _ = U.warmed(N)
    sc = Scenario(N, seed=U.SEED, dt=U.DT)
    fr = list(sc.frames(U.WARM_FRAMES + H.RESIDENT_FRAMES))[U.WARM_FRAMES:]
    z = np.stack([f[0] for f in fr]).astype(np.float32)
    R = np.stack([f[1] for f in fr]).astype(np.float32)
    return dt, st0, z, R, np.ones(z.shape[:2], np.uint8)


@functools.lru_cache(maxsize=None)
def growth_uv(N):
    return Scenario(N + H.GROWTH, seed=U.SEED + 1).initial_features()[N:].astype(np.float32).copy()


def growth_tail(g, case, launder=False):
    """Behind the case's update: GROWTH new landmarks, then GROWTH_ROUNDS x (process(dt), an all-passed update with the scenario's R).  Three rounds:
    process(dt) writes the other of the two covariance buffers, so what an update leaves outside n x n (K y in column n) meets the next update
    but one.  launder: ekfvio_set_state(ekfvio_get_state()) behind every entry point, which zeroes both buffers outside n x n -- the straight run
    must give the same bits, or something reads padding that nothing maintains."""
    N, _, k, layout, _, _ = case
    dt, _, _, z, Ra, _ = U.inputs(N, k, layout, "a")
    uv = growth_uv(N)
    wash = (lambda: g.set_state(g.get_state())) if launder else (lambda: None)
    wash()
    g.addNewFeatures(uv)
    wash()
    rcs = []
    for _ in range(H.GROWTH_ROUNDS):
        g.process(dt)
        wash()
        rcs.append(g.updateWithFeaturePositions(np.concatenate([z, uv]), np.concatenate([Ra, np.repeat(Ra[:1], H.GROWTH, axis=0)]),
                                                np.ones(N + H.GROWTH, np.uint8)))
        wash()
    return tuple(rcs), g.get_state()


def run_step(g, group, step, tail):
    """One step of _history_cases.py on the handle g.  Returns dict(rc, state, sig[, prop, tail])."""
    grp = H.GROUPS[group]
    if step[0] == "singular":
        st0, z, R, p = singular_inputs(step[1])
        g.set_state(st0)
        rc = g.updateWithFeaturePositions(z, R, p)
        assert rc == capi.ENUMERIC, rc
        return dict(rc=rc, state=g.get_state(), sig=None)
    if step[0] == "resident":
        dt, st0, z, R, p = resident_inputs(step[1])
        g.set_state(st0)
        g.upload_measurements(z, R, p)
        c0 = g.counters()
        g.run_uploaded(0, H.RESIDENT_STEPS, dt)
        rc = g.synchronize()
        c1 = g.counters()
        sig = tuple(c1[key] - c0[key] for key in ("graph_steps", "prelinearized_steps", "persistent", "t2_updates"))
        assert sig[0] == H.RESIDENT_STEPS and sig[1] > 0, ("the run did not engage graphs and the riding linearisation", sig)
        return dict(rc=rc, state=g.get_state(), sig=sig)
    N, cap, k, layout, sizing, kind = step[1]
    dt, st0, sp, z, R, p = U.inputs(N, k, layout, kind)
    # (the dense predict is not bit-equal to the fp32 oracle's process(dt) by construction: its twin is held to the oracles from ITS propagated state)
    rc, got, _, sig, prop = step_on(g, st0, None if grp["dense"] else sp, dt, z, R, p, sizing == "device")
    out = dict(rc=rc, state=got, sig=sig, prop=prop)
    if tail:
        out["tail"] = growth_tail(g, step[1], launder=tail == "launder")
    return out


def has_tail(group, step):
    return step[0] == "case" and step[1][0] in H.GROUPS[group]["growth"]


@functools.lru_cache(maxsize=None)
def fresh(group, step, tail=False):
    """The step on a handle that has run nothing else.  Matrix groups: run_case's result (held to the fp64 oracle in test_gpu_update_matrix.py);
    where a growth tail follows, a handle made here, whose update must give run_case's bits.  Twin groups: a handle of the group's capacity and
    mode, held to the oracles here."""
    grp = H.GROUPS[group]
    matrix = grp["oracle"] == "matrix" and step[0] == "case"
    if matrix and not tail:
        rc, got, _, sig = run_case(step[1])
        return dict(rc=rc, state=got, sig=sig)
    g = handle(grp["cap"], dense=grp["dense"])
    try:
        out = run_step(g, group, step, tail)
    finally:
        g.close()
    if tail:  # the same on a second fresh handle with the padding of both covariance buffers zeroed behind every entry point
        g = handle(grp["cap"], dense=grp["dense"])
        try:
            washed = run_step(g, group, step, "launder")
        finally:
            g.close()
        assert washed["tail"][0] == out["tail"][0] and not differing(washed["tail"][1], out["tail"][1]), (
            group, H.step_id(step), "the growth tail reads what lies outside n x n", washed["tail"][0], out["tail"][0],
            differing(washed["tail"][1], out["tail"][1]))
    if matrix:
        rc, got, _, sig = run_case(step[1])
        assert (rc, sig) == (out["rc"], out["sig"]) and not differing(out["state"], got), (group, H.step_id(step), differing(out["state"], got))
    elif step[0] == "case":
        N, cap, k, layout, sizing, kind = step[1]
        dt, st0, sp, z, R, p = U.inputs(N, k, layout, kind)
        same = not differing(out["prop"], sp)
        ref = U.reference(N, k, layout, kind) if same else U.make_reference(out["prop"], z, R, p)
        check_against_oracles("%s twin %s" % (group, H.step_id(step)), sp if same else out["prop"], z, p, out["rc"], out["state"], ref)
    return out


@pytest.mark.parametrize("test", H.TESTS, ids=H.test_id)
def test_successor_behind_predecessor_gives_the_fresh_handles_bits(test):
    group, pred = test
    grp = H.GROUPS[group]
    successors = H.successors_behind(group, pred)
    want_pred = fresh(group, pred)
    wants = [fresh(group, s, has_tail(group, s)) for s in successors]  # (every fresh handle is closed before the one with the history opens)
    failed = []
    g = handle(grp["cap"], dense=grp["dense"])
    try:
        for s, want in zip(successors, wants):
            if pred[0] == "case" and s[0] == "case":  # otherwise the pair is blind
                a, b = want_pred["state"]["Sigma"], want["state"]["Sigma"]
                assert a.shape != b.shape or not np.array_equal(a, b), ("the fresh results do not differ", H.step_id(pred), H.step_id(s))
            run_step(g, group, pred, False)
            got = run_step(g, group, s, "tail" in want)
            what = "%s behind %s" % (H.step_id(s), H.step_id(pred))
            if s[0] == "case" and grp["oracle"] == "matrix":
                N, cap, k, layout, sizing, kind = s[1]
                flow = U.expected_flow(N, cap, sizing, k)
                assert want["sig"] == U.SIGNATURE[flow], (what, "the fresh handle", want["sig"])
            if got["sig"] != want["sig"]:
                failed.append((what, "flow", got["sig"], want["sig"]))
            if got["rc"] != want["rc"] or differing(got["state"], want["state"]):
                failed.append((what, "rc", got["rc"], want["rc"], differing(got["state"], want["state"])))
            if "tail" in want and (got["tail"][0] != want["tail"][0] or differing(got["tail"][1], want["tail"][1])):
                failed.append((what, "growth tail: rc", got["tail"][0], want["tail"][0], differing(got["tail"][1], want["tail"][1])))
    finally:
        g.close()
    print("%s: %d successors" % (H.test_id(test), len(successors)))
    assert not failed, failed
