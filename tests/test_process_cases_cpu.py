"""The cases of tests/test_gpu_process_matrix.py would notice (no GPU needed: the oracles and numpy alone).

Holding process(dt) to the fp32 oracle's bits means something only at shapes and states where a wrong index changes bits, and the dense form's
elementwise bound only if the defects in view move the answer by more than it allows.  Each of _process_cases.DEFECTS -- Sigma read
transposed, landmark f's B block taken from f + 1, D transposed, a process-noise class boundary (7, 10, 16, 22) shifted by one, the last
landmark of a ragged base-row / base-column chunk left unpropagated, the landmark means propagated with the NEW base state, the flush left
out -- is put into the numpy fp64 evaluation of the structured product and must (1) change at least one bit of the fp32-rounded result in
EVERY size / state / flush case it applies to, and (2) move E by MARGIN = 10 dense bounds in some element of every dense case it applies
to.  Run with -s for the tables; _process_cases' docstring records them.

Also here: the edge coverage of the case table as set arithmetic (residues mod 3, 8 and 16, ld == n + 1, n a multiple of 64, both sides
of the planner's boundary), that both oracles are finite on every case, that the start covariance is what the cases need (dense,
not symmetric), that the flush case prunes AND keeps in each of the four regions, and the dense bound for the fp32 oracle itself.
"""
import numpy as np
import pytest

from oracle import set_threads

import _process_cases as P
import _resident_cases as RC


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    P.use_threads()
    yield
    set_threads(1)


def one_per_input(cases):
    """The cases that differ in more than the launch form."""
    seen, out = set(), []
    for c in cases:
        key = (c.N, c.state, c.dt, c.steps, c.scale_exp)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


BITS_CASES = one_per_input([c for c in P.CASES if c.family in ("size", "state", "flush")])
DENSE_CASES = one_per_input(P.DENSE)


def test_the_case_table_is_sound():
    assert len(P.CASES) == len(set(P.CASES)) and len({P.case_id(c) for c in P.CASES}) == len(P.CASES)
    size = [c for c in P.CASES if c.family == "size"]
    ns = {c.N for c in size}
    # PREDICT_PC = 3: every residue, the empty filter and a single chunk; N % 3 == 2 more than once
    assert {N % P.PCH for N in ns} == {0, 1, 2} and {0, 1, 2, 3} <= ns and len([N for N in ns if N % P.PCH == 2]) >= 3
    # LIN_LM = 8 and PREDICT_PT = 16: on and beside the edge; one and two tiles per side
    assert {P.LIN_LM - 1, P.LIN_LM, P.LIN_LM + 1} <= ns and {P.LIN_LM - 1, 0, 1} <= {N % P.LIN_LM for N in ns}
    for tiles in (1, 2):
        assert {tiles * P.PT - 1, tiles * P.PT, tiles * P.PT + 1} <= ns
    assert {P.PT - 1, 0, 1} <= {N % P.PT for N in ns}
    # more residues mod 16 than the five the suite saw before (0, 3, 4, 12, 14)
    assert len({c.N % P.PT for c in P.CASES}) >= 10
    # n a multiple of 64; ld == n + 1 exactly on a handle of its own; ld > n + 1 with a camera update's leftovers
    assert any((P.BASE + 3 * c.N) % 64 == 0 for c in size)
    assert any(c.cap == c.N and P.ld_of(c.cap) == P.BASE + 3 * c.N + 1 for c in size)
    above = [c for c in size if c.cap > c.N]
    assert {(c.N, c.cap) for c in above} == set(P.CAPACITY) and all(c.camera_first and c.steps == 2 for c in above)
    assert all(P.ld_of(c.cap) > P.BASE + 3 * c.N + 1 for c in above)
    # both structured forms up to 257; the planner's own choice on both sides of its boundary on 256 compute units
    for N in P.SIZE_NS:
        assert {c.form for c in size if c.N == N and c.cap == N} == {"inside", "front"}
    lo, hi = P.PLANNER_NS
    assert hi == lo + 1 and {c.form for c in size if c.N in P.PLANNER_NS} == {"default"}
    assert P.form_name(P.predict_plan(lo)) == "inside" and P.form_name(P.predict_plan(hi)) == "front"
    for N in P.SIZE_NS:
        assert P.form_name(P.predict_plan(N)) == "inside"
    # the state family: N % 3 == 2, a ragged tile, every state at every dt in both forms
    st = [c for c in P.CASES if c.family == "state"]
    assert P.STATE_N % P.PCH == 2 and P.STATE_N % P.PT != 0
    assert {(c.state, c.dt, c.form) for c in st} == {(s, float(np.float32(dt)), f) for s in P.STATES for dt in P.DTS for f in ("inside", "front")}
    assert {c.form for c in P.CASES if c.family == "flush"} == {"inside", "front", "dense"}
    assert {(c.N, c.cap) for c in P.DENSE if c.family == "dense"} == set(P.DENSE_NS)
    assert max(P.BASE + 3 * c.N for c in P.CASES) == 1561


def test_the_start_states_are_what_the_cases_need():
    for N, asym, fill in ((20, 1e-4, 0.8), (513, 1e-2, 0.95)):
        S = P.start(N)[0]["Sigma"]
        a, nz = float(np.abs(S - S.T).max()), np.count_nonzero(S) / S.size
        print("\nN = %d: max |S - S^T| = %.2g, %.0f %% non-zero" % (N, a, 100 * nz))
        assert a > asym and nz > fill
    for c in one_per_input(P.CASES):
        st = P.inputs(c)
        assert all(st[k].dtype == np.float32 for k in ("base_mu", "feat_mu", "Sigma")) and st["feat_mu"].shape[0] == c.N
        assert not np.array_equal(st["Sigma"], st["Sigma"].T), P.case_id(c)  # (N = 0 too: one process(dt) from the diagonal prior)
        if c.state == "rotated":
            assert np.array_equal(st["base_mu"][3:7], np.asarray(P.ROTATED["quat"], np.float32)) and st["base_mu"][10] != 0
        if c.state == "omega0":
            assert not st["base_mu"][10:13].any() and st["base_mu"][7:10].all()
        if c.state == "omega1e-11":
            assert 0 < st["base_mu"][10] < 1e-10
    assert P.start(50)[1][2].all()  # the camera step in front of a capacity case measures every landmark


@pytest.mark.parametrize("case", one_per_input(P.CASES), ids=P.case_id)
def test_both_oracles_are_finite_and_the_restatement_is_the_oracles(case):
    s32, s64 = P.reference(case)
    st = P.inputs(case)
    for s in s32 + s64:
        for key in ("base_mu", "feat_mu", "Sigma"):
            assert np.isfinite(s[key]).all(), (P.case_id(case), key)
        for key in ("last_klt", "del_flag"):
            assert np.array_equal(s[key], st[key])
    F, q = P.jacobian(case)
    n = P.BASE + 3 * case.N
    assert np.isfinite(F).all() and np.array_equal(q, P.noise_diag(n, case.dt))
    # structured_fp64 is the product the oracle forms: against the dense fp64 product, and the oracle's fp32 result within the dense bound
    E, mag, bound = P.dense_reference(case)
    F64, S64 = F.astype(np.float64), st["Sigma"].astype(np.float64)
    full = F64 @ S64 @ F64.T + np.diag(q.astype(np.float64))
    full[~(np.abs(full) > P.FLUSH)] = 0
    assert np.abs(full - E).max() <= 1e-12 * max(np.abs(E).max(), 1e-300) + 2 * P.FLUSH
    err = np.abs(s32[0]["Sigma"].astype(np.float64) - E)
    units = P.dense_units(s32[0]["Sigma"], case)
    agree = bool(((s32[0]["Sigma"] == 0) == (E == 0)).all())
    print("\n%-44s fp32 oracle: %.2f of %d units; prunes what E prunes: %s" % (P.case_id(case), units, P.DENSE_UNITS, agree))
    assert (err <= bound).all(), (P.case_id(case), units)
    S = s32[0]["Sigma"]
    assert ((S == 0) | (np.abs(S) > P.FLUSH)).all()


def test_the_flush_case_prunes_and_keeps_in_every_region():
    case = [c for c in P.CASES if c.family == "flush"][0]
    st, (s32, _) = P.inputs(case), P.reference(case)
    assert np.array_equal(st["Sigma"].astype(np.float64) * 2.0 ** P.FLUSH_EXP, P.start(case.N)[0]["Sigma"].astype(np.float64))  # exact
    F, _ = P.jacobian(case)
    raw = P.structured_fp64(F, st["Sigma"], case.dt, case.N, flush=False)
    S = s32[0]["Sigma"]
    print()
    for name, m in P.region_masks(S.shape[0]).items():
        pruned, kept = int(((S[m] == 0) & (raw[m] != 0)).sum()), int((S[m] != 0).sum())
        print("flush 2^-%d, %-15s pruned %4d, kept %4d, structurally zero %4d of %d" % (P.FLUSH_EXP, name, pruned, kept, int((raw[m] == 0).sum()), int(m.sum())))
        assert pruned > 0 and kept > 0, name
    # the defect: without the flush, entries below the threshold survive -- what "0 or above the threshold" is asserted for
    left = P.structured_fp64(F, st["Sigma"], case.dt, case.N, defect="flush_left_out")
    below = (left != 0) & ~(np.abs(left) > P.FLUSH)
    print("flush left out: %d entries below the threshold survive" % int(below.sum()))
    assert below.sum() > 0 and not np.array_equal(left.astype(np.float32), P.dense_reference(case)[0].astype(np.float32))


def _clean_and_defective(case, defect):
    st = P.inputs(case)
    F, _ = P.jacobian(case)
    return P.dense_reference(case), P.structured_fp64(F, st["Sigma"], case.dt, case.N, defect=defect)


def test_every_defect_changes_bits_in_every_case_it_applies_to():
    print("\n%-28s %s" % ("defect", "cases whose fp32-rounded result changes / cases it applies to"))
    short = []
    for d in P.DEFECTS:
        if d == "flush_left_out":
            continue  # (test_the_flush_case_prunes_and_keeps_in_every_region)
        seen = total = 0
        for c in BITS_CASES + (DENSE_CASES if d == "means_from_new_base" else []):
            if not P.applies(d, c):
                continue
            total += 1
            if d == "means_from_new_base":
                changed = not np.array_equal(P.defective_means(c), P.reference(c)[0][0]["feat_mu"])
            else:
                (E, _, _), bad = _clean_and_defective(c, d)
                changed = not np.array_equal(E.astype(np.float32), bad.astype(np.float32))
            seen += changed
            if not changed:
                short.append((d, P.case_id(c)))
        print("%-28s %d of %d" % (d, seen, total))
        assert total > 0
    assert not short, short


def test_every_defect_moves_the_dense_reference_by_ten_bounds():
    print("\n%-28s %-10s %s" % ("defect", "smallest", "over the dense cases it applies to, of the largest |E_defect - E| / bound"))
    short = []
    for d in P.SIGMA_DEFECTS:
        if d == "flush_left_out":
            continue  # moves E by at most one threshold, which the floor allows: seen by the "0 or above the threshold" assertion
        rows = []
        for c in DENSE_CASES:
            if not P.applies(d, c):
                continue
            (E, _, bound), bad = _clean_and_defective(c, d)
            rows.append((float((np.abs(bad - E) / bound).max()), c))
        r, c = min(rows, key=lambda t: t[0])
        print("%-28s %-10.3g %s (%d cases)" % (d, r, P.case_id(c), len(rows)))
        for r, c in rows:
            need = P.BELOW_MARGIN.get((d, c.N, c.dt), P.MARGIN)
            if need < P.MARGIN:
                print("%-28s %-10.3g %s: the one pair below MARGIN (_process_cases.BELOW_MARGIN), held to > %g" % (d, r, P.case_id(c), need))
            if (r <= need) if need < P.MARGIN else (r < need):
                short.append((d, r, P.case_id(c)))
    assert not short, short
    assert len(P.BELOW_MARGIN) == 1


def test_the_planner_takes_the_riding_form_at_the_riding_sizes():
    """The riding linearisation exists only where the update's tail is the T2 one: ekfvio_test_plan's lin_blocks > 0, on 256 compute units."""
    lo, hi = P.RIDING_RANGE
    ns = P.RIDING_CANDIDATES
    assert len(ns) == 5 and all(lo <= N <= hi for N in ns)
    for N in ns:
        p = RC.plan(N, N, 2 * N, P.CUS_MI355X, next_dt=P.DT)
        assert p["lin_blocks"] > 0 and p["tail"] == RC.TAIL_T2, (N, p)
    assert {N % 3 for N in ns} == {0, 1, 2}
    for edge in (8, 16):
        # a full last block (N on the multiple), one landmark into the next block, and a ragged block below the multiple
        assert [M for M in ns if M % edge == 0 and M + 1 in ns and any(N < M and N % edge for N in ns)], edge
