"""An owner's panel block is announced (`pan`) BEFORE its finished tile (`fin`): whoever reads the tile must wait for `fin` itself.

chol_persist_kernel's owners of X and identity row blocks store the panel block (i, j-1) right behind their last step's substitution and raise
pan[i][j-1] behind the step's product; the finished tile (i, j) and fin[i][j] follow.  The gain and T2 tiles formed inside the launch solve the
LAST block column's panel blocks themselves, from the finished tiles of block column mb-1 -- the same owners' whose `pan` flags of block column
mb-2 they have just waited for.  While the tile was published first, `pan` up implied `fin` up, and a consumer could do without looking at `fin`.
It no longer does: the wait for the last block column names ready[mb-1] and every finished tile it reads (gain_tile2<true>: its Y tile, its Z
tile and one tile per X row block of its measurement rows; t2_tile<true>: its two tiles).

The protocol of tests/test_gpu_handoff_delay.py (cases: tests/_handoff.py), at the smallest shapes that can go wrong -- per (N, point) ONE hooks
handle, closed before the next is created, and for every owner h of block columns mb-1 and mb-2
  1. poison: an update of ANOTHER state (Sigma x 3, z shifted by one landmark) with no delay;
  2. the shape's update with owner h 200 us late (ekfvio_test_sweep_delay) in front of the store of its finished tile (point 0) or of its
     panel block (point 1);
  3. the result is, bit for bit, the per-step sweep's (a handle created under EKFVIO_SWEEP=0), with the persistent launch and its T2 counted, no
     abort and no recovery.
Point 0 on an owner of block column mb-1 is the case the order of publication used to cover: its `pan` is up, its tile is 200 us late, and a
consumer that does not wait for `fin` solves the last block column from the poison.

  N = 65, all measured:  m = 130, mb = 3 -- the smallest persistent shape (64 landmarks are two block columns: one launch per block step); the
                         tiles' loop over block columns runs kb = 0, 1
  N = 128, all measured: m = 256, mb = 4
Both take ("persist", "sweep", "t2") on 256 compute units (ekfvio_test_plan, asserted below).
"""
import contextlib
import ctypes as C
import functools
import os
import time

import numpy as np
import pytest

from ekf_vio_amd import TightlyCoupledEKF, capi

import _handoff as H
import _resident_cases as RC
import _update_cases as U

pytestmark = pytest.mark.gpu

SHAPES = (65, 128)
MB = {65: 3, 128: 4}
GAIN_SWEEP = 0  # GainBy (plan.h), as tests/test_plan_cpu.py
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


@functools.lru_cache(maxsize=None)
def inputs(N):
    """(the warmed state behind process(dt), z, R, passed): every landmark measured."""
    dt, st0, sp, (z, R, _) = U.warmed(N)
    return sp, z, R, np.ones(N, np.uint8)


def case_update(g, N):
    sp, z, R, p = inputs(N)
    g.set_state(sp)
    return g.updateWithFeaturePositions(z, R, p)


def poison_update(g, N):
    sp, z, R, p = inputs(N)
    st = dict(sp)
    st["Sigma"] = (sp["Sigma"] * np.float32(3)).astype(np.float32)
    g.set_state(st)
    return g.updateWithFeaturePositions(np.roll(z, 1, axis=0), R, p)


def planned_flow(N):
    p = RC.plan(N, N, 2 * N, H.CUS_MI355X)
    return ("persist" if p["sweep"] == RC.PERSIST_FUSED else "other", "sweep" if p["gain"] == GAIN_SWEEP else "launch",
            {RC.TAIL_T2: "t2", RC.TAIL_JOSEPH: "joseph"}[p["tail"]]), p["m_pad"] // H.TILE


@functools.lru_cache(maxsize=None)
def targets(N):
    """Every owner of block columns mb-1 and mb-2 of the shape's launch, in owner order (ekfvio_test_persist_grid; sweep_delay numbers the
    owners from 1)."""
    roles, out = (C.c_int32 * (4 * H.MAX_BLOCKS))(), (C.c_int32 * 10)()
    rc = capi.load(hooks=True).ekfvio_test_persist_grid(H.CUS_MI355X, N, N, 2 * N, 0, 1, 0, 0, -1.0, roles, H.MAX_BLOCKS, out)
    assert rc == capi.OK and out[0] > 0, (N, rc, out[0])
    mb = MB[N]
    found, h = [], 0
    for b in range(out[0]):
        kind, i, j, back = roles[4 * b:4 * b + 4]
        if kind != H.OWNER:
            continue
        assert back == b
        if j >= mb - 2:
            found.append(H.Target(h + 1, b, i, j, False))
        h += 1
    return tuple(found)


@functools.lru_cache(maxsize=None)
def reference(N):
    """(return code, state) of the shape's update with one launch per block step; computed once, shared, never changed."""
    with per_step_sweep():
        g = TightlyCoupledEKF(max_features=N)
    try:
        rc = case_update(g, N)
        st, c = g.get_state(), g.counters()
        assert c["persistent"] == 0 and c["recoveries"] == 0, c
        assert not np.array_equal(st["Sigma"], inputs(N)[0]["Sigma"]) and np.isfinite(st["Sigma"]).all()
        return rc, st
    finally:
        g.close()


def test_both_shapes_take_the_t2_flow_and_have_owners_to_walk():
    for N in SHAPES:
        flow, mb = planned_flow(N)
        assert flow == ("persist", "sweep", "t2") and mb == MB[N], (N, flow, mb)
        t = targets(N)
        nX = (U.BASE + 3 * N + H.TILE - 1) // H.TILE
        late_tile = [x for x in t if x.j == mb - 1 and x.i >= mb]  # point 0 on these: `pan` up, the tile late
        assert len(late_tile) == nX + mb - 1, (N, len(late_tile))    # every X row block, the identity row blocks 0 .. mb-2 (compact launch)
        assert {x.j for x in t} == {mb - 1, mb - 2}


@pytest.mark.parametrize("point", H.POINTS)
@pytest.mark.parametrize("N", SHAPES)
def test_a_late_owner_of_the_last_two_block_columns_leaves_the_bits_alone(N, point):
    assert planned_flow(N) == (("persist", "sweep", "t2"), MB[N])
    rc_ref, want = reference(N)
    bad = []
    t0 = time.perf_counter()
    g = TightlyCoupledEKF(max_features=N, hooks=True)
    try:
        for n, t in enumerate(targets(N)):
            g.sweep_delay(-1, point, 0)
            poison_update(g, N)
            if n == 0:  # otherwise stale equals fresh and the test is blind
                assert not np.array_equal(g.get_state()["Sigma"], want["Sigma"]), "the poison update gives the shape's Sigma"
            c0 = g.counters()
            g.sweep_delay(t.workgroup, point, H.DELAY_TICKS)
            rc = case_update(g, N)
            got, c1 = g.get_state(), g.counters()
            what = "N = %d: owner %d (block %d) of tile (%d, %d) late at point %d" % (N, t.workgroup - 1, t.block, t.i, t.j, point)
            assert c1["persistent"] == c0["persistent"] + 1 and c1["t2_updates"] == c0["t2_updates"] + 1, (what, c0, c1)
            assert c1["recoveries"] == c0["recoveries"] and c1["mode"] == c0["mode"] != 0, (what, c0, c1)
            assert rc == rc_ref, (what, rc, rc_ref)
            keys = [k for k in KEYS if not np.array_equal(got[k], want[k])]
            if keys:
                bad.append("%s: %s differ from the per-step sweep's" % (what, ", ".join(keys)))
                print("DIFFERS", bad[-1])
    finally:
        g.close()
    print("N = %d point %d: %d owners, %d differ, %.2f s" % (N, point, len(targets(N)), len(bad), time.perf_counter() - t0))
    assert not bad, "\n".join(bad)
