"""The tables of tests/_history_cases.py (which update runs behind which on one handle, tests/test_gpu_update_history.py), checked without a GPU:
the cases exist, the pairs cover the flows in both orders and a larger update in front of a smaller one of the same flow, and no pair is blind
by construction."""
import _history_cases as H
import _update_cases as U


def _case_steps(group):
    g = H.GROUPS[group]
    return [s for s in g["predecessors"] + g["successors"] if s[0] == "case"]


def _case_pairs(groups):
    for group in groups:
        for pred, succ in H.pairs(group):
            for s in succ:
                if pred[0] == "case" and s[0] == "case":
                    yield group, pred[1], s[1]


def test_every_case_of_the_matrix_groups_is_a_case_of_the_update_matrix():
    for group in H.MATRIX_GROUPS:
        for s in _case_steps(group):
            assert s[1] in U.CASES, (group, s)
            assert s[1][1] == H.GROUPS[group]["cap"], (group, s)
    assert H.MATRIX_GROUPS == ("G1", "G2", "G3", "G4", "G5")
    assert len([s for s in H.GROUPS["G1"]["successors"] if s[0] == "case" and s[1][5] == "a"]) == 23


def test_every_ordered_pair_of_a_groups_flow_rows_runs():
    for group in H.MATRIX_GROUPS:
        cap = H.GROUPS[group]["cap"]
        N = _case_steps(group)[0][1][0]
        rows = [i for i, f in enumerate(U.FLOWS) if f[:2] == (N, cap)]
        seen = {(H.flow_row(p), H.flow_row(s)) for g, p, s in _case_pairs([group])}
        for a in rows:
            for b in rows:
                if a != b:
                    assert (a, b) in seen, (group, "no pair runs", U.FLOWS[b], "behind", U.FLOWS[a])


def test_every_flow_runs_behind_itself_with_fewer_block_columns():
    """A flow (sizing, (sweep, gain, tail)) behind the same flow with a LARGER m_pad: the earlier update's outer block columns are then the later
    one's padding.  The split look-ahead sweep is the one flow U.CASES reaches at a single count (N = 600, k = 481; the kind-"d" case has the same
    m_pad), so no such pair exists for it: it runs behind and in front of the per-step sweep (G5)."""
    key = lambda c: (c[4], U.expected_flow(c[0], c[1], c[4], c[2]))
    listed = {(s, f) for (_, _, s, _, _, f) in U.FLOWS}
    shrinking = {key(s) for g, p, s in _case_pairs(H.MATRIX_GROUPS) if key(p) == key(s) and H.m_pad(s) < H.m_pad(p)}
    single = {k for k in listed if len({H.m_pad(c) for c in U.CASES if key(c) == k}) < 2}
    assert single == {("host", ("split", "launch", "joseph"))}, single
    assert shrinking == listed - single, listed - single - shrinking


def test_no_pair_is_a_case_behind_itself():
    n = 0
    for group in H.GROUPS:
        for pred, succ in H.pairs(group):
            assert succ, (group, pred)
            for s in succ:
                n += 1
                assert s != pred and H.what_differs(pred, s), (group, pred, s)
    assert len(H.TESTS) == len({H.test_id(t) for t in H.TESTS}) == sum(len(g["predecessors"]) for g in H.GROUPS.values())
    print("%d (group, predecessor) tests, %d pairs" % (len(H.TESTS), n))


def test_every_flow_is_a_predecessor_and_a_successor_somewhere():
    key = lambda c: (c[4], U.expected_flow(c[0], c[1], c[4], c[2]))
    listed = {(s, f) for (_, _, s, _, _, f) in U.FLOWS}
    pairs = list(_case_pairs(H.MATRIX_GROUPS))
    assert {key(p) for g, p, s in pairs} == listed
    assert {key(s) for g, p, s in pairs} == listed


def test_the_representatives_of_the_filled_scratch_tests():
    reps = H.representatives()
    assert len(reps) == len(set(reps)) == len(U.FLOWS) + 2
    for i, f in enumerate(U.FLOWS):
        c = reps[i]
        assert c in U.CASES and c[5] == "a" and H.flow_row(c) == i
        assert c[2] == max(d[2] for d in U.CASES if d[5] == "a" and H.flow_row(d) == i)
    assert (256, 256, 255, "every", "host", "d") in reps and (256, 256, 160, "run", "host", "a") in reps


def test_growth_tails_fit_the_capacity():
    for group, g in H.GROUPS.items():
        for s in g["successors"]:
            if s[0] == "case" and s[1][0] in g["growth"]:
                assert s[1][0] + H.GROWTH <= g["cap"], (group, s)
    assert H.GROUPS["G2"]["growth"] == (256,) and H.GROUPS["G6"]["growth"] == (256,)
