"""The cases of tests/test_gpu_update_matrix.py would notice (no GPU needed: the oracles alone).

A tolerance of ACC_FACTOR x scatter + floor means something only if the defects in view move the answer by more than that.  For every R
kind b-d and every (N, measured) it is used with, the fp64 oracle is evaluated with the case's R and with R mutated -- off-diagonals
swapped (R^T), off-diagonals zeroed, the u and v variances swapped, landmark i given landmark i+1's block -- and every mutation that changes
R at all must move the fp64 result by at least MARGIN = 10 tolerances of that case in at least one of base state / landmark means / Sigma.
Ten is a margin, not a measurement: it leaves room for the GPU's own rounding on top of the defect.  Likewise the failure layouts: the pass
mask rotated by one landmark.  Run with -s for the table of measured ratios (recorded in tests/_update_cases.py, SENSITIVITY).

Every mutation reaches the margin through Sigma (the smallest: R^T at N = 400, 64 measured).  The means alone would not: the warmed
filter's innovation is 1e-4 .. 3e-4, so a wrong gain moves a mean by a few tolerances at most.

Not held to the margin, only printed: the rotated mask where the layout axis is not varied.  With a single failed landmark (255 of 256,
399 of 400) rotating the mask exchanges one measured landmark for its neighbour, which moves Sigma by 7 .. 11 tolerances only.
"""
import numpy as np
import pytest

from oracle import set_threads

import _scatter
import _update_cases as U

R_CASES = sorted({(N, k, layout, kind) for (N, cap, k, layout, sizing, kind) in U.CASES if kind != "a" and N <= 400})
LAYOUT_CASES = sorted({(N, k, layout) for (N, cap, k, layout, sizing, kind) in U.CASES if kind == "a" and layout != "every"}
                      | {(N, k, "every") for (N, cap, k, layout, sizing, kind) in U.CASES if kind == "a" and layout != "every"})


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    """The oracle's OpenMP products on up to 16 cores while this module runs (U.use_threads), one again behind it."""
    U.use_threads()
    yield
    set_threads(1)


def ratios(state, s64, tol):
    e = U.errors(state, s64)
    return {key: e[key] / tol[key] for key in tol}


def fmt(r):
    return "  ".join("%s %8.3g" % kv for kv in r.items())


def assert_fp64_moves_towards_z(sp, s64, z, p, what):
    away = ~U.moves_towards_z(sp, s64, z, p)
    assert away.sum() <= 0.05 * p.sum(), (what, "measured landmarks whose fp64 mean moves away from z", np.nonzero(away)[0])


def test_the_case_table_is_sound():
    assert len(U.CASES) == len(set(U.CASES)) and 90 <= len(U.CASES) + 1 <= 120  # (+ the N = 1024 step of the GPU module)
    for c in U.CASES:
        N, cap, k, layout, sizing, kind = c
        assert U.expected_flow(N, cap, sizing, k) in U.SIGNATURE
        if sizing == "device":  # its host-sized twin's bookkeeping is compared: any flow, same inputs
            U.expected_flow(N, cap, "host", k)
    # the four layouts of one count are four different masks, and "run" starts inside a 64-row block of Sigma
    for k in (65, 160, 161):
        masks = {U.pass_mask(256, k, layout).tobytes() for layout in U.LAYOUTS}
        assert len(masks) == 4
    assert (U.BASE + 3 * U.RUN_START) % 64 not in (0, 63, 62)
    for kind in "bcd":
        R = U.make_R(kind, 256, np.zeros((256, 4), np.float32))
        assert R[:, 0].max() / R[:, 0].min() > 300 and np.all(R[:, 0] != R[:, 3])
        assert np.array_equal(R[:, 1], R[:, 2]) == (kind != "d") and np.any(R[:, 1] != 0) == (kind != "b")
    Rd = U.make_R("d", 256, np.zeros((256, 4), np.float32))
    assert np.allclose(Rd[:, 2] / Rd[:, 1], U.FX_OVER_FY ** 2, rtol=1e-6)


def test_every_case_has_an_innovation():
    worst = np.inf
    for (N, cap, k, layout, sizing, kind) in U.CASES:
        dt, st0, sp, z, R, p = U.inputs(N, k, layout, kind)
        y = np.abs((z - sp["feat_mu"][:, :2])[p.astype(bool)]).max()
        worst = min(worst, y)
        assert y > 0, (N, k, layout)
    print("\nsmallest max |z - H mu| over the cases: %.3g" % worst)
    for N in sorted({c[0] for c in U.CASES}):
        dt, st0, sp, (z, R, p) = U.warmed(N)
        print("N = %d: max |z - H mu| %.3g" % (N, np.abs(z - sp["feat_mu"][:, :2]).max()))


def test_scatter6_is_fp32_scatter():
    N, k = 100, 65
    dt, st0, sp, z, R, p = U.inputs(N, k, "every", "d")
    ref = U.reference(N, k, "every", "d")
    w = _scatter.fp32_scatter(sp, z, R, p, ref["s64"])
    for key in ("mu", "feat", "sig"):
        assert w[key] == ref["scatter"][key], key


@pytest.mark.parametrize("N,k,layout,kind", R_CASES, ids=lambda v: str(v))
def test_a_wrong_r_moves_the_fp64_result_by_ten_tolerances(N, k, layout, kind):
    dt, st0, sp, z, R, p = U.inputs(N, k, layout, kind)
    ref = U.reference(N, k, layout, kind)
    tol = U.tolerances(ref["s64"], ref["scatter"])
    assert ref["info32"] == 0
    assert_fp64_moves_towards_z(sp, ref["s64"], z, p, (N, k, kind))
    print()
    changed = 0
    for how in U.MUTATIONS:
        M = U.mutate_R(R, how)
        if np.array_equal(M, R):
            continue
        changed += 1
        _, s = U.oracle_update(np.float64, sp, z, M, p)
        r = ratios(s, ref["s64"], tol)
        print("N=%d k=%d R%s %-20s %s" % (N, k, kind, how, fmt(r)))
        assert max(r.values()) >= U.MARGIN, (N, k, kind, how, r)
    assert changed == {"b": 2, "c": 3, "d": 4}[kind]


@pytest.mark.parametrize("N,k,layout", LAYOUT_CASES, ids=lambda v: str(v))
def test_a_pass_mask_off_by_one_landmark_moves_the_fp64_result_by_ten_tolerances(N, k, layout):
    dt, st0, sp, z, R, p = U.inputs(N, k, layout, "a")
    ref = U.reference(N, k, layout, "a")
    tol = U.tolerances(ref["s64"], ref["scatter"])
    assert_fp64_moves_towards_z(sp, ref["s64"], z, p, (N, k, layout))
    q = np.roll(p, 1)
    assert not np.array_equal(p, q)
    _, s = U.oracle_update(np.float64, sp, z, R, q)
    r = ratios(s, ref["s64"], tol)
    print("\nN=%d k=%d %-5s mask rotated  %s" % (N, k, layout, fmt(r)))
    assert max(r.values()) >= U.MARGIN, (N, k, layout, r)


def test_a_single_failure_moved_by_one_landmark_is_printed_not_held_to_the_margin():
    """(module docstring: the layout axis is not varied at these counts)"""
    for N, k in ((256, 255), (400, 399)):
        dt, st0, sp, z, R, p = U.inputs(N, k, "every", "a")
        ref = U.reference(N, k, "every", "a")
        _, s = U.oracle_update(np.float64, sp, z, R, np.roll(p, 1))
        r = ratios(s, ref["s64"], U.tolerances(ref["s64"], ref["scatter"]))
        print("\nN=%d k=%d every mask rotated  %s" % (N, k, fmt(r)))
        assert max(r.values()) > 1


def test_backward_yardstick_reads_the_column_major_block():
    """_scatter.backward_yardstick built R's 2 x 2 block transposed, harmless only while R is symmetric: with a non-symmetric R its
    unperturbed evaluation (c = 0) must reproduce the fp64 oracle's update."""
    N, k = 100, 65
    dt, st0, sp, z, R, p = U.inputs(N, k, "every", "d")
    assert np.any(R[:, 1] != R[:, 2])
    _, s64 = U.oracle_update(np.float64, sp, z, R, p)
    w = _scatter.backward_yardstick(sp, z, R, p, s64, c=0.0, trials=1)
    print("\nbackward_yardstick(c = 0) against the fp64 oracle:", w)
    assert w["mu"] <= 1e-9 and w["feat"] <= 1e-9 and w["sig"] <= 1e-9, w
    # ... and it would not with the block transposed (what the function did before)
    Rt = U.mutate_R(R, "transposed")
    wt = _scatter.backward_yardstick(sp, z, Rt, p, s64, c=0.0, trials=1)
    assert wt["sig"] > 1e-6, wt
