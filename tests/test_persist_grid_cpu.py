"""The grid and the flags of the persistent sweep launch, checked without a GPU: which workgroup of chol_persist_kernel does what is
PersistGrid::role(block index) (ekf_vio_amd/csrc/plan.h), which the planner's residency conditions, the launchers' grid sizes and the
kernel's decode all call; the flags in sweep_sync are laid out by PersistFlags.  ekfvio_test_persist_grid (hooks build) evaluates both for
the launch plan_update selects, with no handle and no HIP call.  The layout is restated here, in spec(), as the specification."""
import collections
import ctypes as C

import pytest

from test_plan_cpu import CUS, NS, no_switches, plan  # noqa: F401  (no_switches: autouse, clears every switch plan_update reads)

PERSIST_FUSED, PERSIST = 2, 3                                  # SweepKind
PLAIN, FUSED, COMPACT = 0, 1, 2                                # PersistGridKind
CHAIN, LEAD, LEAD_GATHER0, GATHER0, OWNER = 0, 1, 2, 3, 4      # PersistRoleKind
MAX_BLOCKS = 1024
Grid = collections.namedtuple("Grid", "total kind owners ready fin pan abort words zero_words sync_words roles back mb nX lead_rows")


def grid(N, m, cap=None):
    """The grid of the update plan(N, m) selects, None where its sweep is not persistent."""
    from ekf_vio_amd import capi
    roles, out = (C.c_int32 * (4 * MAX_BLOCKS))(), (C.c_int32 * 10)()
    rc = capi.load(hooks=True).ekfvio_test_persist_grid(CUS, cap or N, N, m, 0, 1, 0, 0, -1.0, roles, MAX_BLOCKS, out)
    assert rc == capi.OK
    p = plan(N, m, cap=cap)
    assert (out[0] > 0) == (p["sweep"] in (PERSIST_FUSED, PERSIST)), (N, m, p)
    if not out[0]:
        return None
    total = out[0]
    r = [tuple(roles[4 * b:4 * b + 3]) for b in range(total)]
    ldp = (22 + 3 * (cap or N) + 1 + 63) // 64 * 64
    return Grid(*out, roles=r, back=[roles[4 * b + 3] for b in range(total)], mb=p["m_pad"] // 64, nX=p["n_pad"] // 64, lead_rows=ldp // 64)


def spec(kind, mb, nX, lead_rows):
    """chain; lead blocks; two gatherers unless compact; then per block column j = 1 .. mb-1 the rows of A from the diagonal down
    without (1,1), the X row blocks, and the identity row blocks 0 .. j (0 .. j-1 when compact)."""
    blocks = [(CHAIN, 0, 0)]
    if kind != PLAIN:
        for tb in range(mb * lead_rows):
            ib, cb = divmod(tb, mb)
            first_gathers = kind == COMPACT and cb == mb - 1 and ib < 2  # the compact launch's two step-0 gatherers: tile (1, ib)
            blocks.append((LEAD_GATHER0 if first_gathers else LEAD, ib, cb))
    if kind == FUSED:
        blocks += [(GATHER0, 0, 0), (GATHER0, 1, 0)]
    idb0 = mb + nX
    for j in range(1, mb):
        rows = [i for i in range(j, mb) if (i, j) != (1, 1)] + [mb + x for x in range(nX)] + [idb0 + c for c in range(j + (kind != COMPACT))]
        blocks += [(OWNER, i, j) for i in rows]
    return blocks


def check_grid(g, checked):
    key = (g.kind, g.mb, g.nX, g.lead_rows)
    want = spec(*key)
    assert g.roles == want and g.total == len(want), key
    if key in checked:
        return
    checked.add(key)
    owners = [(b, r[1], r[2]) for b, r in enumerate(g.roles) if r[0] == OWNER]
    assert g.owners == len(owners)
    # coverage: every tile the specification gives an owner has exactly one; both step-0 tiles exactly one gatherer in each fused kind
    count = collections.Counter((i, j) for _, i, j in owners)
    assert set(count.values()) == {1} and set(count) == {(r[1], r[2]) for r in want if r[0] == OWNER}, key
    assert sorted(r[1] for r in g.roles if r[0] in (GATHER0, LEAD_GATHER0)) == ([] if g.kind == PLAIN else [0, 1]), key
    # owner_block() inverts the owner numbering
    assert [g.back[b] for b, _, _ in owners] == [b for b, _, _ in owners], key
    assert all(g.back[b] == -1 for b, r in enumerate(g.roles) if r[0] != OWNER)
    # column order (the dispatch-order argument at plan.h, persist_shape): the owners of an owner's panel sources have lower block indices
    block_of = {(i, j): b for b, i, j in owners}
    idb0 = g.mb + g.nX
    for b, i, j in owners:
        for k in range(1, j):
            assert block_of[(j, k)] < b, (key, i, j, k)
            if i < idb0:
                assert block_of[(i, k)] < b, (key, i, j, k)
            elif (i, k) in block_of:  # (an identity row block c has tiles from block column c, or c + 1, on)
                assert block_of[(i, k)] < b, (key, i, j, k)
    # the flags
    rows = 2 * g.mb + g.nX
    assert (g.ready, g.fin, g.pan, g.abort) == (0, g.mb, g.mb + rows * g.mb, g.mb + 2 * rows * g.mb + 1), key
    assert g.zero_words == g.abort and g.abort < g.words and g.words % 4 == 0 and g.words - g.abort <= 4, key
    assert g.words <= g.sync_words, key  # wherever the planner admits the shape


def sweep_all(extra=()):
    checked, kinds = set(), collections.Counter()
    shapes = [(N, 2 * k, None) for N in NS for k in range(1, N + 1)] + list(extra)
    for N, m, cap in shapes:
        g = grid(N, m, cap)
        if g:
            check_grid(g, checked)
            kinds[g.kind] += 1
    return kinds


def test_every_planned_grid_is_the_documented_layout():
    kinds = sweep_all()
    print("persistent shapes over NS by kind (plain, fused, compact):", [kinds[k] for k in (PLAIN, FUSED, COMPACT)])
    assert kinds[FUSED] >= 1 and kinds[COMPACT] >= 1 and kinds[PLAIN] == 0  # not vacuous


def test_plain_launch_grids(monkeypatch):
    monkeypatch.setenv("EKFVIO_FUSE_SWEEP", "0")
    kinds = sweep_all()
    assert kinds[PLAIN] >= 1 and kinds[FUSED] == kinds[COMPACT] == 0
    assert grid(256, 512).total == 154


def test_fused_launch_grids_without_the_t2_flow(monkeypatch):
    monkeypatch.setenv("EKFVIO_T2", "0")
    kinds = sweep_all()
    assert kinds[FUSED] >= 1 and kinds[COMPACT] == kinds[PLAIN] == 0
    assert grid(256, 512).total == 260


def test_oversubscribed_grid(monkeypatch):
    assert grid(400, 800) is None
    monkeypatch.setenv("EKFVIO_PERSIST_OVERSUB", "2")
    g = grid(400, 800)
    check_grid(g, set())
    assert (g.total, g.owners, g.kind) == (670, 407, FUSED)


def test_pinned_totals_and_flag_extents():
    g = grid(256, 512)
    assert (g.total, g.kind) == (251, COMPACT)
    assert (g.words, g.zero_words) == (476, 473)  # the memsets' and gather_potrf_kernel's extent / the last GEMM's
    assert grid(128, 256).total == 61
    g = grid(65, 130)  # the smallest persistent shape: 3 block columns
    assert g is not None and g.kind == COMPACT and g.mb == 3
    assert grid(64, 128) is None
    g = grid(300, 600)
    assert (g.words, g.zero_words) == (712, 711)


def test_t2_pair_is_a_bijection_onto_the_lower_triangle():
    from ekf_vio_amd import capi
    lib, pair = capi.load(hooks=True), (C.c_int32 * 2)()
    pairs = []
    for p in range(30 * 31 // 2):
        assert lib.ekfvio_test_t2_pair(p, pair) == capi.OK
        pairs.append((pair[0], pair[1]))
    for nX in range(1, 31):
        mine = pairs[:nX * (nX + 1) // 2]
        assert len(set(mine)) == len(mine) and set(mine) == {(ta, tb) for ta in range(nX) for tb in range(ta + 1)}, nX
