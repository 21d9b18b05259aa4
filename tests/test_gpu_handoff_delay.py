"""Every hand-off of the persistent sweep, delayed, must leave the update's bits alone (cases and targets: tests/_handoff.py).

chol_persist_kernel's owners pass tiles and panel blocks to each other through flags.  The rest of the suite holds the launch to the per-step
sweep's bits, which sees a wrong operation but not a missing wait: on an idle device the producer is always faster.  Here the order of arrival
is the test's: per (case, point) ONE hooks handle with the production sweep, and for every owner h of the launch
  1. poison -- an update of ANOTHER state (Sigma x 3, z shifted by one landmark, the same landmarks measured) with no delay: S, L, Linv, T2 and K
     now hold finished data of the wrong values exactly where the next update writes;
  2. the case's update with owner h 200 us late (ekfvio_test_sweep_delay) in front of the store of its finished tile (point 0) or of its panel
     block (point 1): about three whole launches, a fifteenth of the wait bound;
  3. the result must be, bit for bit, the per-step sweep's (a handle created under EKFVIO_SWEEP=0), with the persistent launch counted, no abort
     and no recovery.  A consumer that read h's block without waiting for its flag has read the poison.
All owners are walked at both points (a (case, point) takes under a second: 50 .. 150 owners x two updates and three state transfers).
Point 1 delays something only for an owner that stores a panel block through the flags: an X or identity row block off the diagonal.  For the
owners of A's own tiles (i < mb, the diagonal included) the point-1 iteration repeats the undelayed update; they are walked all the same, so
that the list of targets needs no knowledge of the kernel.

Not covered either: the panel solve of the last block column by its owners, the branch a launch WITHOUT the gain inside takes (all four cases form
the gain inside the launch, where the gain tiles solve those blocks themselves); the hook has no delay there.

Not covered: the workgroups that publish fin[1][cb] without being owners (GRID_FUSED's two step-0 gatherers, GRID_COMPACT's two
ROLE_LEAD_GATHER0 workgroups) -- the hook numbers owners only, like stall_workgroup; their consumers are the chain's two looks per step, which
the owners of every later step exercise.

Found with these tests (profiles/handoff_delay.txt): gain_tile2<true> gathered rows of Y from every X row block alo .. ahi of its block column's
measurement rows but looked at the flags of alo .. alo+2 only; with clustered failures (cases B and C) every owner of a row block beyond made the
update wrong when late.  It now looks at all of them.

Each handle is closed before the next is created (a second live handle moves every update to the per-step sweep).
"""
import contextlib
import functools
import os
import time

import numpy as np
import pytest

from ekf_vio_amd import EkfvioError, TightlyCoupledEKF, capi

import _handoff as H
import _resident_cases as RC
import _update_cases as U

pytestmark = pytest.mark.gpu

KEYS = ("base_mu", "feat_mu", "Sigma", "last_klt", "del_flag")


@pytest.fixture(autouse=True)
def production_switches(monkeypatch):
    for name in ("SWEEP", "SWEEP_LA", "T2", "SCHUR", "PERSIST_OVERSUB", "PERSIST_GAIN", "PERSIST_EARLY", "FUSE_SWEEP", "FUSE_GATHER", "SWEEP_WAIT_MS"):
        monkeypatch.delenv("EKFVIO_" + name, raising=False)


@contextlib.contextmanager
def per_step_sweep():
    """EKFVIO_SWEEP=0 while a handle is created (the switches are read once, in ekfvio_create)."""
    old = os.environ.get("EKFVIO_SWEEP")
    os.environ["EKFVIO_SWEEP"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["EKFVIO_SWEEP"]
        else:
            os.environ["EKFVIO_SWEEP"] = old


def case_update(g, cid):
    sp, z, R, p, measured = H.inputs(cid)
    if H.CASES[cid].sizing == "device":
        g.setGate(H.CHI2)
    g.set_state(sp)
    return g.updateWithFeaturePositions(z, R, p)


def poison_update(g, cid):
    st, z, R, p = H.poison_inputs(cid)
    if H.CASES[cid].sizing == "device":
        g.setGate(U.FLT_MAX)
    g.set_state(st)
    return g.updateWithFeaturePositions(z, R, p)


@functools.lru_cache(maxsize=None)
def reference(cid):
    """(return code, state) of the case's update with one launch per block step; computed once, shared, never changed."""
    with per_step_sweep():
        g = TightlyCoupledEKF(max_features=H.CAP)
    try:
        rc = case_update(g, cid)
        st = g.get_state()
        c = g.counters()
        assert c["persistent"] == 0 and c["recoveries"] == 0, c
        if H.CASES[cid].sizing == "device":
            sp, z, R, p, measured = H.inputs(cid)
            assert np.array_equal(g.gate()["gated"].astype(bool), p.astype(bool) & H.outliers())  # the gate rejects the outliers and nothing else
        assert not np.array_equal(st["Sigma"], H.inputs(cid)[0]["Sigma"]) and np.isfinite(st["Sigma"]).all()
        return rc, st
    finally:
        g.close()


def differing(got, want):
    return [k for k in KEYS if not np.array_equal(got[k], want[k])]


@pytest.mark.parametrize("point", H.POINTS)
@pytest.mark.parametrize("cid", sorted(H.CASES))
def test_a_late_owner_leaves_the_bits_alone(cid, point):
    rc_ref, want = reference(cid)
    targets = H.targets(cid)
    bad = []
    t0 = time.perf_counter()
    g = TightlyCoupledEKF(max_features=H.CAP, hooks=True)
    try:
        for n, t in enumerate(targets):
            g.sweep_delay(-1, point, 0)
            poison_update(g, cid)
            if n == 0:  # otherwise stale equals fresh and the test is blind
                assert not np.array_equal(g.get_state()["Sigma"], want["Sigma"]), "the poison update gives the case's Sigma"
            c0 = g.counters()
            g.sweep_delay(t.workgroup, point, H.DELAY_TICKS)
            rc = case_update(g, cid)
            got, c1 = g.get_state(), g.counters()
            what = H.describe(cid, t, point)
            assert c1["persistent"] == c0["persistent"] + 1 and c1["recoveries"] == c0["recoveries"] and c1["mode"] == c0["mode"] != 0, (what, c0, c1)
            assert rc == rc_ref, (what, rc, rc_ref)
            keys = differing(got, want)
            if keys:
                bad.append("%s: %s differ from the per-step sweep's" % (what, ", ".join(keys)))
                print("DIFFERS", bad[-1])
    finally:
        g.close()
    print("case %s point %d: %d owners, %d uncovered producers, %d differ, %.2f s" % (
        cid, point, len(targets), sum(t.uncovered for t in targets), len(bad), time.perf_counter() - t0))
    assert not bad, "\n".join(bad)


def last_row_uncovered(cid="B"):
    """The uncovered producer of the LAST row block of a span, in block column 1: that row block holds a measured row by definition (ahi is the
    block of the span's last row), so the gather selects what it loads from it.  (An uncovered row block in the middle of a run of failed
    landmarks holds none: its stale data is loaded and thrown away.)"""
    late = [t for t in H.targets(cid) if t.uncovered]
    return min(late, key=lambda t: (-t.i, t.j))


def test_case_b_through_run_uploaded_with_a_late_uncovered_producer():
    """Three uploaded frames with case B's mask as ONE device-resident run (a replay of the two-step graph and an eager step, as
    _resident_cases predicts), an uncovered producer late at point 1 in every one of its launches -- set before the run, so the captured launch
    carries it: the bits of one process + update per frame with one launch per block step.  Behind the first step the buffers hold the
    previous step's data, another Sigma's."""
    import torch
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    dt, st0, sp, (z, R, _) = U.warmed(H.N)
    p = H.inputs("B")[3]
    zz, RR, pp = (np.stack([a] * 3) for a in (z, R, p))
    with per_step_sweep():
        ref = TightlyCoupledEKF(max_features=H.CAP)
    try:
        ref.set_state(st0)
        status_ref = capi.OK
        for i in range(3):
            ref.process(dt)
            status_ref |= ref.updateWithFeaturePositions(zz[i], RR[i], pp[i])
        want = ref.get_state()
        assert ref.counters()["persistent"] == 0
    finally:
        ref.close()
    t = last_row_uncovered()
    want_counters = RC.expected_counters(H.N, H.CAP, pp, 3, dt, cus)
    g = TightlyCoupledEKF(max_features=H.CAP, hooks=True)
    try:
        poison_update(g, "B")
        g.set_state(st0)
        g.upload_measurements(zz, RR, pp)
        g.sweep_delay(t.workgroup, 1, H.DELAY_TICKS)
        c0 = g.counters()
        g.run_uploaded(0, 3, dt)
        status = g.synchronize()
        got, c1 = g.get_state(), g.counters()
    finally:
        g.close()
    what = H.describe("B", t, 1)
    assert c1["graph_steps"] - c0["graph_steps"] == want_counters["graph_steps"] == 2, (c0, c1, want_counters)
    assert c1["prelinearized_steps"] - c0["prelinearized_steps"] == want_counters["prelinearized_steps"], (c0, c1, want_counters)
    if cus == H.CUS_MI355X:
        assert c1["persistent"] > c0["persistent"] and c1["t2_updates"] > c0["t2_updates"], (c0, c1)
    assert c1["recoveries"] == c0["recoveries"] and c1["mode"] == c0["mode"] != 0, (c0, c1)
    assert status == status_ref, (status, status_ref)
    assert differing(got, want) == [], (what, "run_uploaded against one process + update per frame")


def test_the_hook_delays_refuses_more_than_a_millisecond_and_switches_off():
    """The delay really happens (a launch with an owner 1 ms late cannot end sooner: twenty of them take at least 20 ms, at either point), more
    than 1 ms -- a third of the wait bound -- is refused and leaves the hook as it was, and with the hook off again the bits are the reference's."""
    cid = "B"
    rc_ref, want = reference(cid)
    t = last_row_uncovered(cid)
    sp, z, R, p, measured = H.inputs(cid)
    g = TightlyCoupledEKF(max_features=H.CAP, hooks=True)
    try:
        for args in ((t.workgroup, 1, H.DELAY_MAX_TICKS + 1), (t.workgroup, 2, 10), (t.workgroup, 0, -1)):
            with pytest.raises(EkfvioError) as e:
                g.sweep_delay(*args)
            assert e.value.code == capi.EINVAL, args
        reps = 20
        took = {}
        for label, args in (("off", (-1, 0, 0)), ("point 0", (t.workgroup, 0, H.DELAY_MAX_TICKS)), ("point 1", (t.workgroup, 1, H.DELAY_MAX_TICKS))):
            g.sweep_delay(*args)
            g.set_state(sp)
            g.synchronize()
            c0 = g.counters()
            t0 = time.perf_counter()
            for _ in range(reps):
                g.updateWithFeaturePositions(z, R, p)
            g.synchronize()
            took[label] = time.perf_counter() - t0
            c1 = g.counters()
            assert c1["persistent"] == c0["persistent"] + reps and c1["recoveries"] == c0["recoveries"], (label, c0, c1)  # 1 ms never becomes an abort
        print("20 updates: " + ", ".join("%s %.1f ms" % (k, 1e3 * v) for k, v in took.items()))
        assert took["point 0"] >= reps * 1e-3 and took["point 1"] >= reps * 1e-3, took
        g.sweep_delay(-1, 1, H.DELAY_TICKS)
        poison_update(g, cid)
        assert case_update(g, cid) == rc_ref
        assert differing(g.get_state(), want) == []
    finally:
        g.close()
    plain = TightlyCoupledEKF(max_features=4)
    try:
        with pytest.raises(RuntimeError):
            plain.sweep_delay(1, 0, 10)  # the product library has no such entry point
    finally:
        plain.close()
