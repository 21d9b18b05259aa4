"""Shared case definitions of tests/test_gpu_handoff_delay.py and tests/test_handoff_cases_cpu.py (a plain module, imported like
_update_cases.py): the hand-offs inside the persistent sweep launch (ekf_vio_amd/csrc/chol_persist.inc), with the ORDER OF ARRIVAL under the
test's control.

The launch's ~150 owner workgroups pass tiles to each other through flags.  Comparing its result with the per-step sweep's sees a wrong
operation; it cannot see a missing wait, because a consumer that reads a block without waiting for its flag still gets the right bits
whenever the producer was faster -- on an idle device, always.  ekfvio_test_sweep_delay (hooks build) makes one owner late by 200 us, IN
FRONT of the store of its finished tile (point 0) or of its panel block (point 1); the buffers it is late for hold the previous update's
data, which the test has made an update of another state.  Whoever reads without waiting then reads the other state's numbers.

Nothing here looks at what the kernels return, and nothing is read from the kernel: spans() restates the measurement map.

A case is one update at N = 256 on a handle of capacity 256 from _update_cases.warmed(256):
  A  all 256 measured, host-sized          ("persist", "sweep", "t2"), 8 block columns
  B  pass_mask(256, 161, "run"), host      the T2 flow, 6 block columns; block column 1 holds landmarks 32..39 and 135..158: X row blocks 1..7
  C  outliers on landmarks 100..149 (rejected by the gate at CHI2) and default_rng(11).choice(256, 51) failed, device-sized: planned for
     m = 2N, 8 block columns (tests/test_gpu_gate.py::test_clustered_rejections_give_the_same_bits_under_both_sweeps' mask)
  D  pass_mask(256, 128, "every"), host    ("persist", "sweep", "joseph"): gain_tile instead of gain_tile2<true>, no T2 tiles
"""
import collections
import ctypes as C
import functools

import numpy as np

import _update_cases as U

N = CAP = 256
CUS_MI355X = 256
TILE = 64
DELAY_TICKS = 20000       # 200 us of the 100 MHz clock: about three whole persistent launches (71.6 us, profiles/r06_kernel_stats_n256.csv) and a
DELAY_MAX_TICKS = 100000  # fifteenth of the 3 ms wait bound; the hook refuses more than 1 ms
CHI2 = 0.01               # tests/test_gpu_gate.py: the scenario's own measurements lie far below it, an offset of OFFSET far above
OFFSET = np.float32(0.05)
POINTS = (0, 1)           # 0: the finished tile's store, 1: the panel block's
OWNER = 4                 # PersistRoleKind (plan.h)
MAX_BLOCKS = 1024

Case = collections.namedtuple("Case", "id sizing flow mb owners")
CASES = {
    "A": Case("A", "host", ("persist", "sweep", "t2"), 8, 146),
    "B": Case("B", "host", ("persist", "sweep", "t2"), 6, 94),
    "C": Case("C", "device", ("persist", "sweep", "t2"), 8, 146),
    "D": Case("D", "host", ("persist", "sweep", "joseph"), 4, 53),
}
Target = collections.namedtuple("Target", "workgroup block i j uncovered")  # workgroup: what sweep_delay / sweep_fault take (owner number + 1)


def outliers():
    out = np.zeros(N, bool)
    out[100:150] = True
    return out


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """(sp, z, R, passed as handed to the update, the landmarks that end up measured) of a case; sp: the warmed state behind process(dt)."""
    dt, st0, sp, (z, R, _) = U.warmed(N)
    z = z.copy()
    if cid == "A":
        p = np.ones(N, np.uint8)
    elif cid == "B":
        p = U.pass_mask(N, 161, "run")
    elif cid == "C":
        p = np.ones(N, np.uint8)
        p[np.random.default_rng(11).choice(N, size=N // 5, replace=False)] = 0
        z[outliers()] += OFFSET
        return sp, z, R, p, (p.astype(bool) & ~outliers()).astype(np.uint8)
    elif cid == "D":
        p = U.pass_mask(N, 128, "every")
    else:
        raise ValueError(cid)
    return sp, z, R, p, p.copy()


def poison_inputs(cid):
    """Another update into the same buffers: Sigma scaled by 3, z shifted by one landmark, the same landmarks measured (case C: handed over as
    tracker failures with the gate at FLT_MAX -- shifted measurements would all be rejected -- so it stays device-sized)."""
    sp, z, R, p, measured = inputs(cid)
    st = dict(sp)
    st["Sigma"] = (sp["Sigma"] * np.float32(3)).astype(np.float32)
    return st, np.roll(z, 1, axis=0), R, measured


def measurement_map(measured):
    """idx[2q], idx[2q+1] = 22 + 3 i_q, 22 + 3 i_q + 1 for the q-th measured landmark i_q."""
    i = np.nonzero(np.asarray(measured))[0]
    idx = np.empty(2 * i.size, np.int64)
    idx[0::2], idx[1::2] = U.BASE + 3 * i, U.BASE + 3 * i + 1
    return idx


def spans(measured, n_landmarks=N):
    """Per block column cb of the measurement map: (alo, ahi), the first and last 64-row block of the state that the measurement rows
    64 cb .. 64 cb + 63 lie in (as X row blocks of [A; X; I] they are row blocks mb + alo .. mb + ahi)."""
    assert len(measured) == n_landmarks
    idx = measurement_map(measured)
    return [(int(idx[c]) // TILE, int(idx[min(c + TILE, idx.size) - 1]) // TILE) for c in range(0, idx.size, TILE)]


def plan(cid):
    """plan_update's fields for the case (ekfvio_test_plan; no device)."""
    import _resident_cases as RC
    case = CASES[cid]
    m = 2 * int(np.count_nonzero(inputs(cid)[3]))
    return RC.plan(N, CAP, m, CUS_MI355X, m_on_device=case.sizing == "device")


def role_table(cid):
    """(roles [(kind, a, b)] per block, owner_block() of each owner's number or -1, mb, nX) from ekfvio_test_persist_grid."""
    from ekf_vio_amd import capi
    case = CASES[cid]
    m = 2 * int(np.count_nonzero(inputs(cid)[3]))
    roles, out = (C.c_int32 * (4 * MAX_BLOCKS))(), (C.c_int32 * 10)()
    rc = capi.load(hooks=True).ekfvio_test_persist_grid(CUS_MI355X, CAP, N, m, int(case.sizing == "device"), 1, 0, 0, -1.0, roles, MAX_BLOCKS, out)
    assert rc == capi.OK and out[0] > 0, (cid, rc, out[0])
    total = out[0]
    p = plan(cid)
    return ([tuple(roles[4 * b:4 * b + 3]) for b in range(total)], [roles[4 * b + 3] for b in range(total)], p["m_pad"] // TILE, p["n_pad"] // TILE)


def uncovered_rows(cid):
    """The X row blocks a gain tile's row gather reads beyond the first three of its span: a in alo + 3 .. ahi, over all block columns cb."""
    rows = set()
    for alo, ahi in spans(inputs(cid)[4]):
        rows.update(range(alo + 3, ahi + 1))
    return sorted(rows)


@functools.lru_cache(maxsize=None)
def targets(cid):
    """Every owner of the case's launch, in owner order.  uncovered: the owner of a tile (mb + a, kb + 1) whose panel block (mb + a, kb) a gain
    tile of some block column cb gathers rows from with alo + 3 <= a <= ahi -- every kb = 0 .. mb-2 is read that way, the last one together with
    the finished tile (mb + a, mb-1) itself -- so: every owner in one of uncovered_rows()."""
    roles, back, mb, nX = role_table(cid)
    assert mb == CASES[cid].mb
    late = set(uncovered_rows(cid)) if CASES[cid].flow[2] == "t2" else set()  # (gain_tile gathers no rows)
    out, h = [], 0
    for b, (kind, i, j) in enumerate(roles):
        if kind != OWNER:
            continue
        assert back[b] == b
        out.append(Target(h + 1, b, i, j, mb <= i < mb + nX and (i - mb) in late))
        h += 1
    return tuple(out)


def describe(cid, t, point):
    return "case %s: owner %d (block %d) of tile (%d, %d) late at point %d%s" % (
        cid, t.workgroup - 1, t.block, t.i, t.j, point, "" if cid in "AD" else ", an uncovered producer" if t.uncovered else ", not an uncovered producer")
