"""The tables of tests/test_gpu_update_history.py, part 2: which update runs behind which on ONE handle (a plain module, imported like
_update_cases.py; tests/test_update_history_cpu.py checks the tables without a GPU).  Nothing in this file looks at a result.

The update's flow is chosen per frame from the row count, and every flow works in the same buffers (Saug, Laug, Linv, Km, Wt, Gm, Rm, yres, idx,
inv_idx, Lsign, the dense-F buffer).  A step here is what a handle runs between two ekfvio_set_state calls:
  ("case", c)            c a case of _update_cases.py, (N, capacity of the handle, measured, layout, sizing, R kind): process(dt) and the update;
  ("singular", N)        the exactly singular update of tests/test_gpu_shapes.py::test_exactly_singular_s_is_flagged_and_never_hangs: Sigma = 0 and
                         R = 0 on the measured rows, EKFVIO_ENUMERIC, non-finite values left in the work buffers;
  ("resident", N)        a device-resident run: RESIDENT_FRAMES all-passed frames uploaded, ekfvio_run_uploaded(0, RESIDENT_STEPS, dt) -- graphs, and
                         the next step's linearisation riding in the update's last GEMM.
A group is one handle shape; a GPU test is one (group, predecessor): for every successor of the group the handle runs the predecessor and then the
successor, and the successor's bits must be those of a fresh handle.  The handle lives through all the successors, so history accumulates.
"""
import _update_cases as U

RESIDENT_FRAMES, RESIDENT_STEPS = 16, 10
GROWTH = 8  # landmarks the growth tail adds behind a successor
GROWTH_ROUNDS = 3  # process(dt) + all-passed update behind them: the two covariance buffers alternate, the third update meets what the first left


def case(N, k, layout="every", sizing="host", kind="a", cap=None):
    return ("case", (N, cap or N, k, layout, sizing, kind))


def _matrix(N, cap):
    """Every kind-"a" case of U.CASES on that handle shape, host- and device-sized."""
    return [("case", c) for c in U.CASES if c[:2] == (N, cap) and c[5] == "a"]


# oracle "matrix": the fresh result is _update_run.run_case, held to the fp64 oracle by tests/test_gpu_update_matrix.py, and the flow is U.FLOWS';
# oracle "twin": a fresh handle of the same capacity and mode run in the history module, held to the oracles there; the flow is the twin's.
# growth: the N of the successors behind which the growth tail runs (addNewFeatures of GROWTH landmarks, GROWTH_ROUNDS x process(dt) and an all-passed update).
GROUPS = {
    "G1": dict(cap=256, dense=False, oracle="matrix", growth=(),
               successors=_matrix(256, 256) + [case(256, 128, kind="c"), ("resident", 256)],
               predecessors=[case(256, 64), case(256, 160, "run"), case(256, 255), case(256, 255, sizing="device"), case(256, 255, kind="d"),
                             ("resident", 256)]),
    "G2": dict(cap=320, dense=False, oracle="matrix", growth=(256,),
               successors=[case(256, k, cap=320) for k in (64, 128, 192, 224, 225, 255)],
               predecessors=[case(256, k, cap=320) for k in (64, 128, 224, 255)]),
    "G3": dict(cap=100, dense=False, oracle="matrix", growth=(),
               successors=[case(100, k) for k in (1, 64, 65, 96, 97)] + [case(100, 10, sizing="device")],
               predecessors=[case(100, 64), case(100, 96), case(100, 97), case(100, 10, sizing="device"), ("singular", 100)]),
    "G4": dict(cap=400, dense=False, oracle="matrix", growth=(),
               successors=[case(400, k) for k in (64, 65, 192, 193, 288, 289, 399)] + [case(400, k, sizing="device") for k in (50, 250)],
               predecessors=[case(400, 64), case(400, 192), case(400, 288), case(400, 399), case(400, 250, sizing="device"),
                             case(400, 399, kind="d")]),
    "G5": dict(cap=600, dense=False, oracle="matrix", growth=(),
               successors=[case(600, 480), case(600, 481)],
               predecessors=[case(600, 480), case(600, 481)]),
    "G6": dict(cap=400, dense=False, oracle="twin", growth=(256,),
               successors=[case(256, k, cap=400) for k in (64, 128, 255)] + [case(400, 288)],
               predecessors=[case(400, 399), case(400, 288), case(100, 97, cap=400)]),
    "G7": dict(cap=256, dense=True, oracle="twin", growth=(),
               successors=[case(256, k) for k in (161, 65, 64)],
               predecessors=[case(256, 255)]),
}
MATRIX_GROUPS = tuple(g for g in GROUPS if GROUPS[g]["oracle"] == "matrix")
# the resident successor runs behind this predecessor only (it is a ten-step run, not one update)
RESIDENT_BEHIND = case(256, 64)


def step_id(s):
    return U.case_id(s[1]) if s[0] == "case" else "%s-N%d" % (s[0], s[1])


def what_differs(a, b):
    """What makes (a behind b) a pair that can see history: the steps differ in N, count, layout or R kind (sizing alone does not count: a
    device-sized update of the same inputs computes the same thing).  The GPU test asserts that their fresh covariances differ."""
    if a[0] != "case" or b[0] != "case":
        return a != b
    (N1, _, k1, l1, _, r1), (N2, _, k2, l2, _, r2) = a[1], b[1]
    return (N1, k1, l1, r1) != (N2, k2, l2, r2)


def pairs(group):
    """[(predecessor, [successors behind it])] of a group."""
    g = GROUPS[group]
    out = []
    for pred in g["predecessors"]:
        succ = [s for s in g["successors"] if what_differs(pred, s) and (s[0] != "resident" or pred == RESIDENT_BEHIND)]
        out.append((pred, succ))
    return out


TESTS = [(group, pred) for group in GROUPS for pred, _ in pairs(group)]


def test_id(t):
    return "%s-behind-%s" % (t[0], step_id(t[1]))


def successors_behind(group, pred):
    return dict((step_id(p), s) for p, s in pairs(group))[step_id(pred)]


def m_pad(c):
    """Rows of the update's block columns that carry measurements: 2 x measured, rounded up to the 64-row block."""
    return (2 * c[2] + 63) // 64 * 64


def flow_row(c):
    """The row of U.FLOWS a case falls in."""
    N, cap, k, _, sizing, _ = c
    rows = [i for i, (n, cp, s, lo, hi, _) in enumerate(U.FLOWS) if (n, cp, s) == (N, cap, sizing) and lo <= k <= hi]
    assert len(rows) == 1, c
    return rows[0]


def representatives():
    """Part 1 (filled scratch): per row of U.FLOWS the kind-"a" case of U.CASES with the largest count; N = 256, k = 255 with R kind "d"; N = 256,
    k = 160 with the failures in one run."""
    out = []
    for i in range(len(U.FLOWS)):
        row = [c for c in U.CASES if c[5] == "a" and flow_row(c) == i]
        assert row, U.FLOWS[i]
        out.append(max(row, key=lambda c: c[2]))
    for extra in (case(256, 255, kind="d")[1], case(256, 160, "run")[1]):
        assert extra in U.CASES
        if extra not in out:
            out.append(extra)
    return out
