"""The cases of tests/test_gpu_handoff_delay.py (tests/_handoff.py), checked without a GPU: each takes the flow it is there for, the two with
clustered failures really spread a block column's measurement rows over more than three X row blocks, and every owner of each launch is a
target exactly once."""
import collections

import numpy as np
import pytest

from test_plan_cpu import flow, no_switches  # noqa: F401  (no_switches: autouse, clears every switch plan_update reads)

import _handoff as H
import _update_cases as U


@pytest.mark.parametrize("cid", sorted(H.CASES))
def test_each_case_takes_its_flow(cid):
    case = H.CASES[cid]
    p = H.plan(cid)
    measured = int(np.count_nonzero(H.inputs(cid)[3]))
    assert flow(p) == case.flow == U.expected_flow(H.N, H.CAP, case.sizing, measured), (cid, p)
    assert p["m_pad"] // 64 == case.mb, (cid, p)
    assert bool(p["compact"]) == (case.flow[2] == "t2")


def test_spans_restates_the_measurement_map():
    # everything measured: 64 rows are 32 landmarks are 96 state rows from 22 + 96 cb on
    assert H.spans(np.ones(H.N, np.uint8)) == [((22 + 96 * cb) // 64, (22 + 96 * cb + 94) // 64) for cb in range(8)]
    # the issue's example: block column 1 of case B holds landmarks 32..39 and 135..158, state rows 118..497
    sp = H.spans(H.inputs("B")[4])
    assert len(sp) == 6 and sp[1] == (1, 7), sp
    idx = H.measurement_map(H.inputs("B")[4])
    assert (idx[64], idx[127]) == (118, 497) and idx.size == 322


@pytest.mark.parametrize("cid", ["B", "C"])
def test_clustered_failures_spread_a_block_column_over_more_than_three_row_blocks(cid):
    sp = H.spans(H.inputs(cid)[4])
    print(cid, "spans", sp, "uncovered X row blocks", H.uncovered_rows(cid))
    assert any(ahi - alo >= 3 for alo, ahi in sp), sp
    late = [t for t in H.targets(cid) if t.uncovered]
    assert late, cid
    mb = H.CASES[cid].mb
    # per uncovered row block one owner in every block column 1 .. mb-1
    assert collections.Counter(t.i - mb for t in late) == {a: mb - 1 for a in H.uncovered_rows(cid)}


def test_the_other_two_cases_have_no_uncovered_producer():
    """A: every block column's rows lie in at most three row blocks.  D: every second landmark measured spreads 64 rows over 192 state rows, four
    row blocks -- but its flow forms the gain with gain_tile, which gathers no rows of Y at all (the row gather belongs to the T2 flow's
    gain_tile2), so nothing is read beyond the tile's own two panel blocks."""
    sp = H.spans(H.inputs("A")[4])
    assert len(sp) == 8 and all(0 <= ahi - alo <= 2 for alo, ahi in sp), sp
    assert H.spans(H.inputs("D")[4]) == [(0, 3), (3, 6), (6, 9), (9, 12)] and H.CASES["D"].flow[2] == "joseph"
    for cid in "AD":
        assert not any(t.uncovered for t in H.targets(cid))


def test_case_c_is_the_clustered_rejections_mask():
    sp, z, R, p, measured = H.inputs("C")
    assert int(p.sum()) == 256 - 51 and np.array_equal(np.nonzero(H.outliers())[0], np.arange(100, 150))
    assert np.array_equal(measured.astype(bool), p.astype(bool) & ~H.outliers())
    z0 = U.warmed(H.N)[3][0]
    assert np.array_equal(z[H.outliers()], z0[H.outliers()] + H.OFFSET) and np.array_equal(z[~H.outliers()], z0[~H.outliers()])


@pytest.mark.parametrize("cid", sorted(H.CASES))
def test_every_owner_is_a_target_exactly_once(cid):
    roles, back, mb, nX = H.role_table(cid)
    ts = H.targets(cid)
    assert len(ts) == H.CASES[cid].owners == sum(1 for r in roles if r[0] == H.OWNER), (cid, len(ts))
    assert [t.workgroup for t in ts] == list(range(1, len(ts) + 1))
    assert sorted(t.block for t in ts) == [b for b, r in enumerate(roles) if r[0] == H.OWNER]
    assert len({(t.i, t.j) for t in ts}) == len(ts)
    assert all(roles[t.block] == (H.OWNER, t.i, t.j) and back[t.block] == t.block for t in ts)


def test_poison_differs_from_the_case_in_what_the_sweep_stores():
    for cid in sorted(H.CASES):
        sp = H.inputs(cid)[0]
        st, z, R, p = H.poison_inputs(cid)
        assert np.array_equal(p, H.inputs(cid)[4]) and not np.array_equal(st["Sigma"], sp["Sigma"]) and not np.array_equal(z, H.inputs(cid)[1])


def test_delay_is_inside_its_limits():
    """More than two and a half 71.6 us launches (profiles/r06_kernel_stats_n256.csv), and no more than the hook accepts: the limit is read from
    include/ekfvio_test_hooks.h (the GPU test holds the library to it: 100 001 ticks are refused)."""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ekfvio_test_hooks.h")).read()
    limit = int(re.search(r"#define EKFVIO_TEST_SWEEP_DELAY_MAX_TICKS (\d+)", hdr).group(1))
    assert H.DELAY_MAX_TICKS == limit
    assert 2.5 * 7160 < H.DELAY_TICKS <= limit
