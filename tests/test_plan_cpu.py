"""The decision table of the product, checked without a GPU: which sweep, gain and tail an update takes is integer arithmetic over the
switches (Tuning), a PlanShape and the row count (ekf_vio_amd/csrc/plan.h, plan_update).  ekfvio_test_plan (hooks build) calls it with no
handle and no HIP call: the switches from the environment, the sizes of a handle of the given capacity on a device of the given number of
compute units.

Known, and not changed here: the FLOWS row (600, 600, "host", 1, 480) -> per-step sweep of tests/_update_cases.py was observed on the
device at 480 measured only; the planner gives persistent sweeps for 65 .. 224 measured of 600.  The table is compared at the CASES only
-- the points that ran on an MI355X; correcting the row needs a device run of such a case.
"""
import ctypes as C
import os
import subprocess

import pytest

import _update_cases as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256  # MI355X
NS = (20, 64, 100, 256, 300, 400, 600)
# SweepKind, GainBy, UpdateTail of plan.h
SCHUR, PERSIST_FUSED, PERSIST, STEP, SPLIT, SPLIT_LA = 1, 2, 3, 4, 5, 6
GAIN_SWEEP, GAIN_GEMM = 0, 3
TAIL_T2, TAIL_JOSEPH = 2, 3
FIELDS = ("m", "m_pad", "n_pad", "sweep", "fused_gather", "with_wt", "gain", "tail", "t2_skip", "t2_by_sweep", "compact", "lin_blocks")


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in ("SWEEP", "SWEEP_LA", "T2", "SCHUR", "PERSIST_OVERSUB", "PERSIST_GAIN", "FUSE_SWEEP", "FUSE_GATHER", "LIN_OVERLAP", "FUSE_LINEARIZE"):
        monkeypatch.delenv("EKFVIO_" + name, raising=False)  # every switch plan_update reads


def plan(N, m, cap=None, cus=CUS, m_on_device=False, sole=True, latched_off=False, dense=False, next_dt=-1.0):
    from ekf_vio_amd import capi
    out = (C.c_int32 * 12)()
    rc = capi.load(hooks=True).ekfvio_test_plan(cus, cap or N, N, m, int(m_on_device), int(sole), int(latched_off), int(dense), next_dt, out)
    assert rc == capi.OK
    p = dict(zip(FIELDS, out))
    # every plan any test asks for: a gain tile of the T2 flow looks at n_pad / 64 + 2 flags in ONE look of a wavefront, a lane each, and lane 63
    # is the abort word's (plan.h, PERSIST_POLL_FLAGS; chol_persist.inc, gain_tile2)
    assert p["t2_skip"] < 0 or p["n_pad"] // 64 + 2 <= 63, (N, m, p)
    return p


def all_counts(**kw):
    return [plan(N, 2 * k, **kw) for N in NS for k in range(1, N + 1)]


def flow(p):
    sweep = {PERSIST_FUSED: "persist", PERSIST: "persist", STEP: "step", SPLIT: "split", SPLIT_LA: "split"}[p["sweep"]]
    return (sweep, "sweep" if p["gain"] == GAIN_SWEEP else "launch", {TAIL_T2: "t2", TAIL_JOSEPH: "joseph"}[p["tail"]])


def test_plans_are_the_flows_recorded_on_the_device():
    shapes = sorted({(N, cap, k, sizing) for (N, cap, k, layout, sizing, kind) in U.CASES})
    assert len(shapes) == 43
    for N, cap, k, sizing in shapes:
        p = plan(N, 2 * k, cap=cap, m_on_device=sizing == "device")
        assert flow(p) == U.expected_flow(N, cap, sizing, k), (N, cap, k, sizing, p)


def test_tail_and_gain_kind_belong_to_the_shape_not_to_the_neighbours():
    """Eight handles on one GPU give each one's solo bits (tests/test_gpu_shapes.py) because of this."""
    solo = all_counts()
    for kw in (dict(sole=False), dict(latched_off=True), dict(sole=False, latched_off=True)):
        other = all_counts(**kw)
        assert not any(p["sweep"] in (PERSIST_FUSED, PERSIST) for p in other)
        for a, b in zip(solo, other):
            assert a["tail"] == b["tail"] and (a["gain"] == GAIN_GEMM) == (b["gain"] == GAIN_GEMM), (kw, a, b)


def test_sweep_switch(monkeypatch):
    assert any(p["sweep"] == PERSIST_FUSED for p in all_counts())
    monkeypatch.setenv("EKFVIO_SWEEP", "0")
    assert not any(p["sweep"] in (PERSIST_FUSED, PERSIST) for p in all_counts())


def test_t2_switch(monkeypatch):
    assert any(p["tail"] == TAIL_T2 for p in all_counts())
    monkeypatch.setenv("EKFVIO_T2", "0")
    assert not any(p["tail"] == TAIL_T2 for p in all_counts())


def test_schur_switch(monkeypatch):
    assert not any(p["sweep"] == SCHUR for p in all_counts())
    monkeypatch.setenv("EKFVIO_SCHUR", "1")
    for p in all_counts():
        assert (p["sweep"] == SCHUR) == (p["m_pad"] // 64 < 16), p


def test_persist_oversub_switch(monkeypatch):
    assert plan(400, 800)["sweep"] == STEP
    monkeypatch.setenv("EKFVIO_PERSIST_OVERSUB", "2")
    assert plan(400, 800)["sweep"] in (PERSIST_FUSED, PERSIST)


def test_sweep_la_switch(monkeypatch):
    default = all_counts()
    monkeypatch.setenv("EKFVIO_SWEEP_LA", "0")
    seen = 0
    for a, b in zip(default, all_counts()):
        if a["m_pad"] // 64 >= 16:
            assert (a["sweep"], b["sweep"]) == (SPLIT_LA, SPLIT), (a, b)
            seen += 1
        else:
            assert a == b
        assert dict(a, sweep=0) == dict(b, sweep=0)
    assert seen


def test_front_fusion_switches(monkeypatch):
    assert plan(256, 512)["sweep"] == PERSIST_FUSED
    monkeypatch.setenv("EKFVIO_FUSE_SWEEP", "0")
    assert not any(p["sweep"] == PERSIST_FUSED for p in all_counts())
    p = plan(256, 512)
    assert p["sweep"] == PERSIST and p["fused_gather"] == 1  # the persistent launch behind gather + first diagonal tile in one launch
    monkeypatch.delenv("EKFVIO_FUSE_SWEEP")
    monkeypatch.setenv("EKFVIO_FUSE_GATHER", "0")
    assert not any(p["sweep"] == PERSIST_FUSED or p["fused_gather"] for p in all_counts())
    assert plan(256, 512)["sweep"] == PERSIST


def test_linearisation_rides_only_where_everything_allows_it(monkeypatch):
    assert not any(p["lin_blocks"] for p in all_counts())  # no next_dt
    assert plan(256, 512, next_dt=0.05)["lin_blocks"] == 33 and plan(100, 200, next_dt=0.05)["lin_blocks"] == 14
    assert plan(256, 512, next_dt=0.0)["lin_blocks"] == 33
    assert not any(p["lin_blocks"] for p in all_counts(next_dt=0.05, dense=True))
    for name in ("EKFVIO_LIN_OVERLAP", "EKFVIO_FUSE_LINEARIZE"):
        monkeypatch.setenv(name, "0")
        assert not any(p["lin_blocks"] for p in all_counts(next_dt=0.05)), name
        monkeypatch.delenv(name)
    for p in all_counts(next_dt=0.05):  # ... and only in the one GEMM of the T2 tail
        assert p["lin_blocks"] == 0 or p["tail"] == TAIL_T2


def test_plan_header_needs_no_hip():
    hdr = os.path.join(ROOT, "ekf_vio_amd", "csrc", "plan.h")
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", hdr], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    assert '#include "' not in open(hdr).read()  # no project header either
