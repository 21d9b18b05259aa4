"""The expectations tests/test_gpu_resident_run.py holds the device-resident run to (tests/_resident_cases.py), checked without a GPU: the
replay decomposition on hand-written examples and against the library's own rule (plan.h, plan_run through ekfvio_test_run_plan), the labels of the case table against the planner at 256 compute units, and the host rule
that sends a sequence with one ragged frame through the eager loop."""
import ctypes as C

import numpy as np
import pytest

import _resident_cases as RC
import _update_cases as U

CUS = RC.CUS_MI355X


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in ("SWEEP", "SWEEP_LA", "T2", "SCHUR", "PERSIST_OVERSUB", "PERSIST_GAIN", "FUSE_SWEEP", "FUSE_GATHER", "LIN_OVERLAP", "FUSE_LINEARIZE"):
        monkeypatch.delenv("EKFVIO_" + name, raising=False)  # every switch plan_update reads


def test_replay_decomposition_on_hand_written_examples():
    assert RC.replays(43, 64) == (1, 1, 1, 1)
    assert RC.replays(40, 40) == (0, 5, 0, 0)  # no 32-step graph below 64 uploaded frames
    assert RC.replays(1, 72) == (0, 0, 0, 1)   # a single step is eager
    assert RC.replays(0, 72) == (0, 0, 0, 0)
    assert RC.replays(72, 72) == (2, 1, 0, 0)
    assert RC.replays(136, 64) == (4, 1, 0, 0)
    assert RC.replays(64, 63) == (0, 8, 0, 0) and RC.replays(64, 64) == (2, 0, 0, 0)
    assert RC.replays(2, 2) == (0, 0, 1, 0) and RC.replays(3, 72) == (0, 0, 1, 1) and RC.replays(9, 72) == (0, 1, 0, 1)
    assert RC.replays(10, 10) == (0, 1, 1, 0) and RC.replays(34, 72) == (1, 0, 1, 0)
    assert RC.replays(43, 64, uniform=False) == (0, 0, 0, 43)
    for count in range(0, 200):
        for frames in (2, 63, 64, 72):
            n32, n8, n2, eager = RC.replays(count, frames)
            assert 32 * n32 + 8 * n8 + 2 * n2 + eager == count and n8 < 4 + 100 * (frames < 64) and n2 < 4 and eager < 2


def run_plan(rows, N, gated, profiling, count):
    """plan_run (plan.h) through ekfvio_test_run_plan: what ekfvio_run_uploaded executes.  rows: measurement rows per uploaded frame."""
    from ekf_vio_amd import capi
    rows = np.ascontiguousarray(rows, np.int32)
    out = (C.c_int32 * 6)()
    rc = capi.load(hooks=True).ekfvio_test_run_plan(int(N), int(gated), int(profiling), len(rows), rows.ctypes.data_as(C.POINTER(C.c_int32)), int(count), out)
    assert rc == capi.OK
    return bool(out[0]), out[1], tuple(out[2:6])


def layouts(N, k, frames):
    """The four sequence layouts: uniform, one ragged frame, one frame without any measurement, all frames empty."""
    ragged = RC.passes_for(N, k, frames, ragged=(frames // 2, np.flatnonzero(RC.passes_for(N, k, frames)[frames // 2])[:2]))
    none_once = RC.passes_for(N, k, frames)
    none_once[frames // 3] = 0
    return dict(uniform=RC.passes_for(N, k, frames), ragged=ragged, none_once=none_once, empty=np.zeros((frames, N), np.uint8))


def test_the_librarys_run_plan_is_the_restated_rule():
    """plan_run against replays(), geometry() and is_uniform(): graphs iff the geometry is uniform, profiling is off and count is not 1; the cut;
    and the geometry the graphs are captured for.  (The profiler is not part of the restatement: with it on, the rule is the non-uniform one.)"""
    N, k = 16, 12
    for frames in (1, 2, 63, 64, 72, 144):
        for name, p in layouts(N, k, frames).items():
            rows = 2 * p.astype(np.int64).sum(axis=1)
            assert (name == "uniform") == bool((rows == 2 * k).all()) and (name != "empty" or not rows.any()), (name, frames)
            for gated in (False, True):
                uniform, geom = RC.is_uniform(p, gated), RC.geometry(p, gated)
                for profiling in (False, True):
                    for count in range(0, 201):
                        graphs, m, cut = run_plan(rows, N, gated, profiling, count)
                        what = (frames, name, gated, profiling, count)
                        assert graphs == (uniform and not profiling and count != 1), what
                        assert cut == RC.replays(count, frames, uniform and not profiling), what
                        assert sum(s * c for s, c in zip((RC.GRAPH_BIG, RC.GRAPH, RC.GRAPH_PAIR, 1), cut)) == count, what
                        if graphs:
                            assert m == int(geom[0]), what
                        else:
                            assert cut[:3] == (0, 0, 0), what


def test_the_librarys_run_plan_cuts_the_cases_as_restated():
    for c in RC.CASES:
        for p, first, count, scale in RC.walk(c):
            uniform = RC.is_uniform(p, c.gated)
            graphs, m, cut = run_plan(2 * p.astype(np.int64).sum(axis=1), c.N, c.gated, False, count)
            assert cut == RC.replays(count, p.shape[0], uniform), (c.id, cut)
            assert graphs == (uniform and count != 1) and (not graphs or m == int(RC.geometry(p, c.gated)[0])), (c.id, graphs, m)
    assert RC.case_counters(next(c for c in RC.CASES if c.id == "seq-run-gemms-run"), CUS)[1] == [(0, 1, 1, 0), (0, 2, 0, 0)]


def test_uniform_sequences_measure_k_landmarks_at_moving_positions():
    p = RC.passes_for(256, 200, 72)
    assert p.shape == (72, 256) and (p.sum(axis=1) == 200).all()
    assert all((p[i] != p[i + 1]).any() for i in range(71))
    assert np.array_equal(RC.passes_for(256, 200, 64, shift=8), p[8:72])
    assert RC.passes_for(256, 256, 72).all()


def test_labels_of_the_case_table_are_the_planners():
    """lin_blocks > 0 at 256 compute units exactly where a case is labelled "overlap": the T2 rows of _update_cases.FLOWS for N = 256
    (161 .. 256 measured; 161 .. 224 under a capacity of 320) and N = 100 (97 .. 100); other sizes as ekfvio_test_plan says."""
    dt = 1.0 / 30.0
    for c in RC.CASES:
        for p, first, count, scale in RC.walk(c):
            gated = c.gated
            label = RC.classify(c.N, c.cap, p, CUS, gated=gated, sole=not c.second, dt=scale * dt, dense=c.dense)
            assert label == c.label, (c.id, label)
            if label == "eager fallback":
                continue
            m = int(RC.geometry(p, gated)[0])
            pl = RC.plan(c.N, c.cap, m, CUS, m_on_device=gated, sole=not c.second, next_dt=scale * dt, dense=c.dense)
            assert (pl["lin_blocks"] > 0) == (c.label == "overlap"), (c.id, pl)
            if c.N in (100, 256):  # ... and the table recorded on the device agrees
                flow = U.expected_flow(c.N, c.cap, "device" if gated else "host", c.N if gated else c.k)
                assert (flow[2] == "t2") == (c.label == "overlap"), (c.id, flow)
                if not c.second:
                    assert (flow[0] == "persist") == (pl["sweep"] in (RC.PERSIST_FUSED, RC.PERSIST)), (c.id, flow, pl)
            if c.second:
                assert pl["sweep"] == RC.STEP and pl["tail"] == RC.TAIL_T2, (c.id, pl)  # per-step sweep, still the T2 shape
    # the boundaries of the overlap, from the planner: one count either side
    for N, cap, k, want in ((256, 256, 161, True), (256, 256, 160, False), (256, 320, 224, True), (256, 320, 225, False), (100, 100, 97, True),
                            (100, 100, 96, False)):
        assert (RC.plan(N, cap, 2 * k, CUS, next_dt=dt)["lin_blocks"] > 0) == want, (N, cap, k)


def test_every_label_is_hit():
    hit = {c.label for c in RC.CASES}
    assert hit == set(RC.LABELS), (hit, RC.LABELS)
    assert len({c.id for c in RC.CASES}) == len(RC.CASES)


def test_a_ragged_frame_without_the_gate_is_the_eager_fallback():
    """What tests/test_gpu_parity.py::test_linearisation_inside_the_update_gemm_gives_the_per_call_bits once got wrong: the row count of
    every uploaded frame is counted on the host, one frame with two failed landmarks makes the geometry non-uniform, and every step of the
    run then goes through the eager loop -- no graph, no pre-linearised step."""
    p = RC.passes_for(256, 256, 72, ragged=(7, (1, 128)))
    assert p[7].sum() == 254 and p.sum() == 72 * 256 - 2
    assert not RC.is_uniform(p, gated=False) and RC.is_uniform(p, gated=True)
    assert RC.classify(256, 256, p, CUS) == "eager fallback"
    assert RC.expected_counters(256, 256, p, 72, 1 / 30, CUS) == dict(graph_steps=0, prelinearized_steps=0)
    assert RC.replays(72, 72, RC.is_uniform(p, False)) == (0, 0, 0, 72)
    # with the gate on every frame in which a landmark passed is planned for m = 2N: graphs, and at N = 256 the overlap
    assert RC.expected_counters(256, 256, p, 72, 1 / 30, CUS, gated=True) == dict(graph_steps=72, prelinearized_steps=69)
    p[9] = 0  # ... but a frame without any measurement is a geometry of its own, gate or not
    assert not RC.is_uniform(p, gated=True)


def test_expected_counters_of_the_cases():
    want = {"shape-N256-cap256-k256": (72, 69), "shape-N256-cap256-k160": (72, 0), "shape-N600-cap600-k600": (10, 0), "count-0": (0, 0),
            "count-1": (0, 0), "count-2": (2, 1), "count-3": (2, 1), "count-9": (8, 7), "count-43": (42, 39),  # 72 frames: 32 + 8 + 2 + 1
            "wrap-first50-count43": (42, 39), "wrap-first63-count2": (2, 1), "wrap-count136": (136, 4 * 31 + 7),
            "seq-odd-then-even": (8 + 34, 7 + 31 + 1), "seq-odd-then-even-dense-predict": (8 + 34, 0), "seq-run-step-run": (26, 8 + 14), "seq-run-gemms-run": (26, 8 + 14), "seq-second-upload": (10 + 40, 8 + 31 + 7),
            "second-handle": (72, 69), "ragged": (0, 0), "ragged-gated": (72, 69), "overlap-off": (72, 69)}
    for c in RC.CASES:
        total, cuts = RC.case_counters(c, CUS)
        if c.id in want:
            assert (total["graph_steps"], total["prelinearized_steps"]) == want[c.id], (c.id, total, cuts)
        assert total["prelinearized_steps"] <= total["graph_steps"]


def test_overlap_switch_reaches_the_expectation(monkeypatch):
    c = next(c for c in RC.CASES if c.id == "overlap-off")
    monkeypatch.setenv("EKFVIO_LIN_OVERLAP", "0")
    assert RC.case_counters(c, CUS)[0] == dict(graph_steps=72, prelinearized_steps=0)
