"""Shared case definitions of tests/test_gpu_resident_run.py and tests/test_resident_cases_cpu.py (a plain module, imported like
_update_cases.py): the device-resident run, ekfvio_run_uploaded, where its captured graphs and the linearisation overlap engage.

Nothing here looks at what a run returns.  What a run is EXPECTED to do is written down twice, independently of the library's control flow:
  * replays(): how ekfvio_run_uploaded cuts `count` steps into replays of its 32-, 8- and 2-step graphs and eager steps -- the rule of
    plan.h's plan_run restated (the 32-step graph exists only for sequences of at least 64 frames; greedy 32, 8, 2; an odd last step is eager; a
    single step, or a sequence whose frames do not all have one launch geometry, runs eager throughout);
  * expected_counters(): the deltas of the handle's counters `graph_steps` and `prelinearized_steps` that follow from it.  Whether a graph's
    steps are pre-linearised is the PLANNER's decision (plan.h, plan_update: lin_blocks), asked of ekfvio_test_plan with the compute-unit
    count of the device the test runs on, so the expectation follows the planner on a partitioned device; the labels of the case table
    are pinned against the planner at 256 compute units by tests/test_resident_cases_cpu.py.

A case is a small script of operations that the GPU test applies to a device-resident handle and, frame by frame, to a per-call one:
  ("run", first, count, dt_scale)   ekfvio_run_uploaded(first, count, dt_scale * dt)  | process + update of frames (first + s) % frames
  ("step", i)                       one ekfvio_process + ekfvio_update with frame i of the uploaded sequence, on both
  ("reset",)                        ekfvio_set_state back to the start state, on both
  ("upload", shift, frames)         upload frames shift .. shift + frames of the scenario (the per-call twin indexes the new sequence)
  ("gemms", reps)                   ekfvio_profile_update_gemms(reps) on the device-resident handle (a capture of its own, into scratch) | nothing
"""
import collections
import ctypes as C

import numpy as np

import _update_cases as U

SEED = 6
BASE_FRAMES = 144  # frames of the scenario a case may upload from
FRAMES = 72        # uploaded unless a case says otherwise: 2 x 32 + 8
GRAPH_BIG, GRAPH, GRAPH_PAIR = 32, 8, 2
BIG_FROM_FRAMES = 64  # the 32-step graph is captured for sequences at least this long
CUS_MI355X = 256

LABELS = ("overlap", "T2-less persistent", "per-step sweep", "split sweep", "one block column", "eager fallback")

# SweepKind, GainBy, UpdateTail of plan.h (as tests/test_plan_cpu.py)
PERSIST_FUSED, PERSIST, STEP, SPLIT, SPLIT_LA = 2, 3, 4, 5, 6
TAIL_T2, TAIL_JOSEPH = 2, 3
PLAN_FIELDS = ("m", "m_pad", "n_pad", "sweep", "fused_gather", "with_wt", "gain", "tail", "t2_skip", "t2_by_sweep", "compact", "lin_blocks")


# ---------------------------------------------------------------------------------------------------------------- the host rules
def replays(count, seq_frames, uniform=True):
    """(replays of the 32-step graph, of the 8-step graph, of the 2-step graph, eager steps) of ekfvio_run_uploaded(first, count, dt)."""
    assert count >= 0 and seq_frames > 0
    if count == 0:
        return (0, 0, 0, 0)
    if not uniform or count < 2:
        return (0, 0, 0, count)
    n32 = count // GRAPH_BIG if seq_frames >= BIG_FROM_FRAMES else 0
    n8, rest = divmod(count - GRAPH_BIG * n32, GRAPH)
    n2, eager = divmod(rest, GRAPH_PAIR)
    return (n32, n8, n2, eager)


def geometry(passes, gated):
    """The launch geometry of every uploaded frame: its measurement rows as the host counts them; with the gate on, 2N for every frame in
    which any landmark passed (the count is then device data)."""
    p = np.asarray(passes)
    rows = 2 * np.count_nonzero(p, axis=1)
    return np.where(rows > 0, 2 * p.shape[1], rows) if gated else rows


def is_uniform(passes, gated):
    g = geometry(passes, gated)
    return bool(np.all(g == g[0]))


def plan(N, cap, m, cus, m_on_device=False, sole=True, next_dt=-1.0, dense=False):
    """plan_update through ekfvio_test_plan (hooks build; no device, no handle): the switches come from the environment."""
    from ekf_vio_amd import capi
    out = (C.c_int32 * 12)()
    rc = capi.load(hooks=True).ekfvio_test_plan(int(cus), int(cap), int(N), int(m), int(m_on_device), int(sole), 0, int(dense), float(next_dt), out)
    assert rc == capi.OK
    return dict(zip(PLAN_FIELDS, out))


def expected_counters(N, cap, passes, count, dt, cus, gated=False, sole=True, dense=False):
    """dict(graph_steps, prelinearized_steps): what ONE ekfvio_run_uploaded(first, count, dt) over the uploaded `passes` adds to the counters.
    A graph of S steps holds S - 1 pre-linearised process(dt) launches where the planner lets the update's GEMM linearise (its last update is
    given no next dt, so a graph needs nothing from whatever ran before it); eager steps are never pre-linearised."""
    uniform = is_uniform(passes, gated)
    n32, n8, n2, eager = replays(count, np.asarray(passes).shape[0], uniform)
    out = dict(graph_steps=GRAPH_BIG * n32 + GRAPH * n8 + GRAPH_PAIR * n2, prelinearized_steps=0)
    if out["graph_steps"]:
        m = int(geometry(passes, gated)[0])
        p = plan(N, cap, m, cus, m_on_device=gated and m > 0, sole=sole, next_dt=dt, dense=dense)
        if p["lin_blocks"] > 0:
            out["prelinearized_steps"] = (GRAPH_BIG - 1) * n32 + (GRAPH - 1) * n8 + (GRAPH_PAIR - 1) * n2
    return out


def classify(N, cap, passes, cus, gated=False, sole=True, dt=1.0 / 30.0, dense=False):
    """The label of a sequence's runs, from the host rule and the planner."""
    if not is_uniform(passes, gated):
        return "eager fallback"
    m = int(geometry(passes, gated)[0])
    p = plan(N, cap, m, cus, m_on_device=gated and m > 0, sole=sole, next_dt=dt, dense=dense)
    if p["lin_blocks"] > 0:
        assert p["tail"] == TAIL_T2
        return "overlap"
    if p["m_pad"] == 64:
        return "one block column"
    if p["sweep"] in (SPLIT, SPLIT_LA):
        return "split sweep"
    if p["sweep"] in (PERSIST_FUSED, PERSIST):
        return "T2-less persistent" if p["tail"] == TAIL_JOSEPH else "persistent, T2 tail without overlap"
    assert p["sweep"] == STEP
    return "per-step sweep" if p["tail"] == TAIL_JOSEPH else "per-step sweep, T2 tail without overlap"


# ---------------------------------------------------------------------------------------------------------------- the sequences
def passes_for(N, k, frames, shift=0, ragged=None):
    """Uniform k: every frame measures k landmarks, at positions that differ from frame to frame (the "every" layout rotated by the frame's
    index in the scenario).  ragged = (frame, landmarks): those landmarks fail in that one frame as well."""
    base = U.pass_mask(N, k, "every")
    p = np.stack([np.roll(base, i) for i in range(shift, shift + frames)]).astype(np.uint8)
    if ragged is not None:
        frame, which = ragged
        p[frame - shift, list(which)] = 0
    return p


Case = collections.namedtuple("Case", "id N cap k frames ops label gated second ragged overlap_off dense")


def _case(id, N, k, ops, label, cap=None, frames=FRAMES, gated=False, second=False, ragged=None, overlap_off=False, dense=False):
    return Case(id, N, cap or N, k, frames, tuple(ops), label, gated, second, ragged, overlap_off, dense)


def _run(count, first=0, dt_scale=1.0):
    return ("run", first, count, dt_scale)


def _cases():
    out = []
    # shapes, 72 steps = 2 x 32 + 8.  (256, 256, 64): m = 128 rows are two block columns, one short of the persistent launch's three
    for N, cap, k, label in ((256, 256, 256, "overlap"), (256, 256, 200, "overlap"), (256, 320, 224, "overlap"), (100, 100, 100, "overlap"),
                             (96, 96, 96, "overlap"), (256, 256, 160, "T2-less persistent"), (256, 256, 64, "per-step sweep"),
                             (30, 30, 30, "one block column"), (400, 400, 400, "per-step sweep")):
        out.append(_case("shape-N%d-cap%d-k%d" % (N, cap, k), N, k, [_run(FRAMES)], label, cap=cap))
    out.append(_case("shape-N600-cap600-k600", 600, 600, [_run(10)], "split sweep", frames=10))
    # decomposition (count 72 is the first shape case)
    for count in (0, 1, 2, 3, 9, 43):
        out.append(_case("count-%d" % count, 256, 256, [_run(count)], "overlap"))
    # the device counter and its wrap, 64 frames uploaded
    out.append(_case("wrap-first50-count43", 256, 256, [_run(43, first=50)], "overlap", frames=64))  # wraps inside the 32-step graph
    out.append(_case("wrap-first63-count2", 256, 256, [_run(2, first=63)], "overlap", frames=64))
    out.append(_case("wrap-count136", 256, 256, [_run(136)], "overlap", frames=64))                  # more than two laps
    # calls in sequence
    out.append(_case("seq-odd-then-even", 256, 256, [_run(9), _run(34, first=9)], "overlap"))  # the eager ninth step flips the ping-pong
    # ... and with the dense predict, which flips the mean's ping-pong alone (Sigma is propagated in place): GraphKey::mu is the only key that sees it
    out.append(_case("seq-odd-then-even-dense-predict", 30, 30, [_run(9), _run(34, first=9)], "one block column", dense=True))
    out.append(_case("seq-run-step-run", 256, 256, [_run(10), ("step", 10), _run(16, first=11)], "overlap"))
    out.append(_case("seq-dt-changed", 256, 256, [_run(10), _run(10, first=10, dt_scale=0.5)], "overlap"))
    out.append(_case("seq-dt-zero", 256, 256, [_run(10, dt_scale=0.0)], "overlap"))
    out.append(_case("seq-set-state", 256, 256, [_run(9), ("reset",), _run(16, first=9)], "overlap"))
    out.append(_case("seq-second-upload", 256, 256, [_run(10), ("upload", 8, 64), _run(40, first=2)], "overlap"))
    # the profiler's capture between two runs (the capture helper the step graphs share): the graphs and the host's mirror of the sweep's flags stand
    out.append(_case("seq-run-gemms-run", 100, 100, [_run(10), ("gemms", 2), _run(16, first=10)], "overlap"))
    # a second, idle handle alive on the device: per-step sweep in the graphs, the T2 shape and the overlap stay
    out.append(_case("second-handle", 256, 256, [_run(FRAMES)], "overlap", second=True))
    # one frame with two failed landmarks: eager throughout with the gate off; with the gate on the geometry is 2N for every frame
    out.append(_case("ragged", 256, 256, [_run(FRAMES)], "eager fallback", ragged=(7, (1, 128))))
    out.append(_case("ragged-gated", 256, 256, [_run(FRAMES)], "overlap", ragged=(7, (1, 128)), gated=True))
    out.append(_case("overlap-off", 256, 256, [_run(FRAMES)], "overlap", overlap_off=True))  # EKFVIO_LIN_OVERLAP=0: the label is the SHAPE's
    return out


CASES = _cases()


def case_id(c):
    return c.id


def walk(case):
    """The runs of a case with the sequence each one sees: [(passes, first, count, dt_scale)]."""
    out = []
    shift, frames = 0, case.frames
    for op in case.ops:
        if op[0] == "upload":
            shift, frames = op[1], op[2]
        elif op[0] == "run":
            out.append((passes_for(case.N, case.k, frames, shift, case.ragged), op[1], op[2], op[3]))
    return out


def case_counters(case, cus, dt=1.0 / 30.0):
    """The counter deltas of the whole case and its replay decompositions, one per run."""
    total, cuts = dict(graph_steps=0, prelinearized_steps=0), []
    for p, first, count, scale in walk(case):
        e = expected_counters(case.N, case.cap, p, count, scale * dt, cus, gated=case.gated, sole=not case.second, dense=case.dense)
        for key in total:
            total[key] += e[key]
        cuts.append(replays(count, p.shape[0], is_uniform(p, case.gated)))
    return total, cuts
