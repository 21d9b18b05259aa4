"""New landmarks spread over the image (include/ekfvio.h, ekfvio_set_replenish_grid), without a GPU: the host function
ekfvio_replenish_select, which compiles the inline functions the selection kernel compiles (csrc/select.h), against the pure-Python
restatement of the specification (tests/_replenish_grid.py), pixel for pixel and in order; the properties the specification promises, on
the output; the grid (0, 0) against the oracle's replenishFeatures; what the grid buys on the fixture, printed (-s); and the arguments'
validation."""
import ctypes as C

import numpy as np
import pytest

from ekf_vio_amd import capi, mask_blocked, replenish_select
from oracle import replenish

import _mask as mk
import _replenish_grid as rg

GRIDS = {"640x480": [(1, 1), (2, 2), (8, 6), (16, 16)], "64x48": [(1, 1), (2, 2), (8, 6), (16, 16)],
         "67x45": [(1, 1), (2, 2), (8, 6), (16, 16), (5, 3)], "periodic": [(1, 1), (2, 2), (8, 6)]}
CASES = [(n, g) for n in GRIDS for g in GRIDS[n]]
HUGE = 4096  # a `wanted` no frame here can hold


def blocked_map(name):
    """B of ekfvio_mask_blocked for a caller's mask with a no-data rectangle, at the image's kill pad."""
    h, w = rg.image(name).shape
    return mask_blocked(None, None, mk.user_mask("rect", w, h), w, h, 1, rg.params(name)[2], 0)


def check_properties(name, px, kp, sc, ex, B, grid, wanted):
    """What the specification promises of the output, whatever the grid."""
    h, w = rg.image(name).shape
    _, radius, pad = rg.params(name)
    assert len(px) <= wanted
    spans = rg.circle_spans(radius)
    O = np.zeros((h, w), np.uint8)
    for x, y in ex:
        rg.stamp(O, int(x), int(y), spans)
    for x, y in px:
        x, y = int(x), int(y)
        assert rg.in_box(x, y, w, h, pad) and (B is None or B[y, x] == 0)
        assert O[y, x] == 0, "inside the circle of a landmark or of an earlier pick"
        rg.stamp(O, x, y, spans)
    for i, (x, y) in enumerate(px):  # ... and no earlier pick inside a later one's circle either (the circle is symmetric)
        for x2, y2 in px[i + 1:]:
            dy = int(y2) - int(y)
            assert not (dy in spans and abs(int(x2) - int(x)) <= spans[dy])
    if grid == (1, 1) and len(px):
        # strongest corner first: every pick is the strongest candidate not covered at its time, so the picks' scores never increase
        score_at = {(int(x), int(y)): int(s) for (x, y), s in zip(kp, sc)}
        got = [score_at[(int(x), int(y))] for x, y in px]
        assert all(a >= b for a, b in zip(got, got[1:])), got
        if len(px) < wanted:  # it stopped for want of candidates: no keypoint in the box is left free
            Bz = np.zeros((h, w), np.uint8) if B is None else B
            assert all(O[y, x] or Bz[y, x] or not rg.in_box(int(x), int(y), w, h, pad) for x, y in kp)


@pytest.mark.parametrize("name,grid", CASES, ids=["%s %dx%d" % (n, g[0], g[1]) for n, g in CASES])
def test_host_function_takes_the_restatements_pixels_in_order(name, grid):
    h, w = rg.image(name).shape
    _, radius, pad = rg.params(name)
    kp, sc = rg.keypoints(name)
    assert len(kp) >= 6
    B = blocked_map(name)
    assert 0 < B.mean() < 1
    differs = 0
    for ex in (np.zeros((0, 2), np.int32), rg.crowd(w, h, 7)):
        for wanted in (1, 3, HUGE):
            for b in (None, B):
                want = rg.select(kp, sc, ex, b, w, h, radius, pad, grid[0], grid[1], wanted)
                got = replenish_select(kp, sc, ex, b, w, h, radius, pad, grid[0], grid[1], wanted)
                assert got.dtype == want.dtype and np.array_equal(got, want), (name, grid, len(ex), wanted, b is not None, got[:8], want[:8])
                check_properties(name, got, kp, sc, ex, b, grid, wanted)
                raster = rg.select(kp, sc, ex, b, w, h, radius, pad, 0, 0, wanted)
                differs += not np.array_equal(raster, want)
                if wanted == HUGE:
                    assert 1 <= len(want) < HUGE
    # (the periodic image's corners all tie, so a grid with one cell, or with one corner per cell, IS the raster order: there the tie-break
    # is what is checked)
    assert differs >= 1 or name == "periodic", "the grid takes what the raster first fit takes: the case shows nothing"


def test_score_ties_go_to_the_smallest_keypoint_index():
    """The periodic image: every corner has the same score, so within a cell and between cells with equal counts k alone decides."""
    name = "periodic"
    h, w = rg.image(name).shape
    _, radius, pad = rg.params(name)
    kp, sc = rg.keypoints(name)
    assert len(kp) >= 12 and len(set(sc.tolist())) == 1
    got = replenish_select(kp, sc, np.zeros((0, 2), np.int32), None, w, h, radius, pad, 1, 1, 4)
    inbox = [k for k in range(len(kp)) if rg.in_box(int(kp[k, 0]), int(kp[k, 1]), w, h, pad)]
    assert np.array_equal(got[0], kp[inbox[0]])  # one cell, all tie: the first keypoint of the raster order
    got = replenish_select(kp, sc, np.zeros((0, 2), np.int32), None, w, h, radius, pad, 2, 2, 4)
    want = rg.select(kp, sc, np.zeros((0, 2), np.int32), None, w, h, radius, pad, 2, 2, 4)
    assert np.array_equal(got, want) and len(got) == 4
    cells = ((got[:, 1] // -(-h // 2)) * 2 + got[:, 0] // -(-w // 2)).tolist()
    assert cells == [0, 1, 2, 3]  # equal counts, equal scores: the cells' winners in the order of their k, which is the raster order


@pytest.mark.parametrize("name", ["640x480", "67x45"])
def test_grid_off_is_the_oracles_first_fit(name):
    img = rg.image(name)
    h, w = img.shape
    thr, radius, pad = rg.params(name)
    kp, sc = rg.keypoints(name)
    for ex in (np.zeros((0, 2), np.int32), rg.crowd(w, h, 7, quadrant=0)):
        for total in (len(ex) + 1, len(ex) + 3, 400):
            want = replenish(img, ex.astype(np.float32), total, threshold=thr, min_dist=radius, kill_pad=pad)
            got = replenish_select(kp, sc, ex, None, w, h, radius, pad, 0, 0, total - len(ex))
            assert np.array_equal(got, want), (name, len(ex), total)
            assert np.array_equal(got, rg.select(kp, sc, ex, None, w, h, radius, pad, 0, 0, total - len(ex)))


def test_what_the_grid_buys_on_the_fixture(capsys):
    """Printed with -s (README, "new landmarks spread over the image").  Asserted: only what the specification guarantees -- with `wanted` at or
    below the number of cells that hold a candidate, the grid places the new landmarks in `wanted` distinct cells."""
    name = "640x480"
    h, w = rg.image(name).shape
    _, radius, pad = rg.params(name)
    kp, sc = rg.keypoints(name)
    score_at = {(int(x), int(y)): int(s) for (x, y), s in zip(kp, sc)}
    lines = []
    for label, ex, wanted in (("lower half full, wanted 8", rg.lower_half(w, h), 8), ("lower half full, wanted 32", rg.lower_half(w, h), 32),
                              ("first fill, wanted 100", np.zeros((0, 2), np.int32), 100), ("first fill, wanted 256", np.zeros((0, 2), np.int32), 256)):
        row = [label]
        for grid in ((0, 0), (8, 6)):
            rounds = []
            px = rg.select(kp, sc, ex, None, w, h, radius, pad, grid[0], grid[1], wanted, rounds)
            assert np.array_equal(px, replenish_select(kp, sc, ex, None, w, h, radius, pad, grid[0], grid[1], wanted))
            cells, mean_row = rg.spread(px, w, h)
            mean_score = float(np.mean([score_at[(int(x), int(y))] for x, y in px])) if len(px) else float("nan")
            row.append("%s: %3d taken, %2d cells of 48, mean row %5.1f, mean score %5.1f%s" %
                       ("raster" if grid == (0, 0) else "8x6   ", len(px), cells, mean_row, mean_score, "" if grid == (0, 0) else ", rounds %d" % len(rounds)))
            if grid == (8, 6):
                # the cells that hold a candidate at the start: what the first round's list is made of
                spans = rg.circle_spans(radius)
                O = np.zeros((h, w), np.uint8)
                for x, y in ex:
                    rg.stamp(O, int(x), int(y), spans)
                start = {(int(y) // -(-h // 6)) * 8 + int(x) // -(-w // 8) for x, y in kp if rg.in_box(int(x), int(y), w, h, pad) and O[y, x] == 0}
                row.append("cells with a candidate at the start: %d" % len(start))
                if wanted <= len(start):
                    assert cells == wanted, (label, cells, wanted)
        lines.append(" | ".join(row))
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_distinct_cells_while_wanted_is_at_most_the_cells_with_a_candidate():
    """The guarantee at its edge.  The picks of ONE round lie in distinct cells whatever the radius (a winner that a neighbouring cell's winner
    has covered is skipped, not replaced), so with `wanted` up to what the first round takes the new landmarks lie in `wanted` distinct cells."""
    for name, grid in (("64x48", (2, 2)), ("67x45", (5, 3)), ("640x480", (8, 6))):
        h, w = rg.image(name).shape
        _, radius, pad = rg.params(name)
        kp, sc = rg.keypoints(name)
        rounds = []
        rg.select(kp, sc, np.zeros((0, 2), np.int32), None, w, h, radius, pad, grid[0], grid[1], HUGE, rounds)
        first = rounds[0]
        assert first >= 2
        for wanted in (1, first):
            px = replenish_select(kp, sc, np.zeros((0, 2), np.int32), None, w, h, radius, pad, grid[0], grid[1], wanted)
            assert len(px) == wanted and rg.spread(px, w, h, *grid)[0] == wanted


def test_arguments_are_validated():
    """ekfvio_set_replenish_grid refuses what ekfvio_replenish_select refuses (one inline function, csrc/select.h): here through the host
    function, which needs no device."""
    lib = capi.load()
    for s in ("ekfvio_set_replenish_grid", "ekfvio_get_replenish_grid", "ekfvio_replenish_select"):
        assert s in capi.SYMBOLS and hasattr(lib, s)
    ip = C.POINTER(C.c_int32)
    kp = np.array([[20, 20], [40, 30]], np.int32)
    sc = np.array([60, 70], np.int32)
    out, k = np.zeros((4, 2), np.int32), C.c_int32(-1)

    def call(cx, cy, kp_=kp, sc_=sc, count=2, W=64, H=48, radius=5, wanted=2, out_=out, added=k):
        return lib.ekfvio_replenish_select(None if kp_ is None else kp_.ctypes.data_as(ip), None if sc_ is None else sc_.ctypes.data_as(ip), count, None, 0,
                                           None, W, H, radius, 4, cx, cy, wanted, None if out_ is None else out_.ctypes.data_as(ip),
                                           None if added is None else C.byref(added))
    for good in ((0, 0), (1, 1), (8, 6), (16, 16), (256, 1), (1, 256), (2, 128)):
        assert call(*good) == capi.OK and k.value == 2, good
    for bad in ((0, 1), (1, 0), (-1, -1), (-8, -6), (17, 16), (257, 1), (1, 257), (65536, 65536), (2 ** 31 - 1, 2), (0, -1)):
        k.value = -1
        assert call(*bad) == capi.EINVAL and k.value == -1, bad
    assert call(8, 6, count=-1) == capi.EINVAL and call(8, 6, wanted=-1) == capi.EINVAL
    assert call(8, 6, kp_=None) == capi.EINVAL and call(8, 6, sc_=None) == capi.EINVAL and call(8, 6, out_=None) == capi.EINVAL
    assert call(8, 6, added=None) == capi.EINVAL
    assert call(8, 6, W=0) == capi.EINVAL and call(8, 6, H=0) == capi.EINVAL
    assert call(8, 6, radius=-1) == capi.EINVAL and call(8, 6, radius=64) == capi.EINVAL and call(8, 6, radius=63) == capi.OK
    assert call(8, 6, W=40) == capi.EINVAL  # a keypoint outside the frame
    assert call(8, 6, sc_=np.array([60, -1], np.int32)) == capi.EINVAL
    assert call(8, 6, count=0, kp_=None, sc_=None) == capi.OK and k.value == 0  # nothing to choose from
    assert call(8, 6, wanted=0, out_=None) == capi.OK and k.value == 0


def test_node_parameters_reach_the_replay_driver(tmp_path):
    """replenish_grid_x / replenish_grid_y by name through ekfvio::Params, echoed by --print-config; values outside [0, 256] are errors."""
    import json
    import subprocess
    from ekf_vio_amd import _build
    _build.build()
    exe = _build.build_host()

    def run(text):
        args = [exe, "--print-config"]
        if text is not None:
            f = tmp_path / "params.yaml"
            f.write_text(text)
            args.append(str(f))
        out = subprocess.run(args, capture_output=True, text=True, timeout=120)
        return out.returncode, (json.loads(out.stdout) if out.returncode == 0 else out.stderr)

    rc, d = run(None)
    assert rc == 0 and (d["replenish_grid_x"], d["replenish_grid_y"]) == (0, 0)
    rc, d = run("replenish_grid_x: 8\n~replenish_grid_y: 6\n")
    assert rc == 0 and (d["replenish_grid_x"], d["replenish_grid_y"]) == (8, 6), d
    for bad in ("replenish_grid_x: -1\n", "replenish_grid_y: 257\n", "replenish_grid_x: 2.5\n", "replenish_grid_y: many\n"):
        rc, err = run(bad)
        assert rc == 2 and "error" in err, (bad, err)


def test_a_winner_covered_by_a_neighbouring_cells_winner_is_skipped_not_replaced():
    """Synthetic keypoints on a 64 x 48 frame, a 2 x 1 grid (cells 32 wide), radius 5: the left cell's winner at x = 30 covers the right
    cell's winner at x = 33.  The right cell has a weaker, free corner at x = 50, but the round does not fall back to it: the covered winner
    is skipped, the round ends with one landmark, and the weaker corner is the right cell's winner of the NEXT round."""
    W, H, radius, pad = 64, 48, 5, 4
    none = np.zeros((0, 2), np.int32)
    # raster order: k = 0 (10, 10) s 60, left; k = 1 (30, 24) s 90, left; k = 2 (33, 24) s 80, right; k = 3 (50, 24) s 70, right
    kp = np.array([[10, 10], [30, 24], [33, 24], [50, 24]], np.int32)
    sc = np.array([60, 90, 80, 70], np.int32)
    rounds = []
    want = rg.select(kp, sc, none, None, W, H, radius, pad, 2, 1, 4, rounds)
    # round 1: the winners are (30, 24) and (33, 24); the first covers the second, which is skipped: ONE landmark.  Round 2: the counts are
    # left 1, right 0, so the right cell's new winner (50, 24) goes in front of the left cell's (10, 10): two landmarks.  (A round that
    # replaced its covered winner would have taken two landmarks, then one.)
    assert want.tolist() == [[30, 24], [50, 24], [10, 10]] and rounds == [1, 2]
    for wanted in (1, 2, 3, 4):
        got = replenish_select(kp, sc, none, None, W, H, radius, pad, 2, 1, wanted)
        assert np.array_equal(got, want[:wanted]), wanted
    # the same keypoints on a 3 x 1 grid (cells 22 wide): (30, 24) and (33, 24) share the middle cell, no winner covers another: one round
    rounds3 = []
    want3 = rg.select(kp, sc, none, None, W, H, radius, pad, 3, 1, 4, rounds3)
    assert want3.tolist() == [[30, 24], [50, 24], [10, 10]] and rounds3 == [3]
    assert np.array_equal(replenish_select(kp, sc, none, None, W, H, radius, pad, 3, 1, 4), want3)
    # ... and where the rule changes the OUTPUT: three cells, the left one's winner (20, 24) covers the middle one's (23, 24), whose weaker
    # free corner (40, 24) has to wait for the next round, behind the right cell's winner (55, 24)
    kp = np.array([[20, 24], [23, 24], [40, 24], [55, 24]], np.int32)
    sc = np.array([90, 80, 50, 70], np.int32)
    rounds = []
    want = rg.select(kp, sc, none, None, W, H, radius, pad, 3, 1, 4, rounds)
    assert want.tolist() == [[20, 24], [55, 24], [40, 24]] and rounds == [2, 1]  # (replaced within the round: (40, 24) would come second)
    for wanted in (1, 2, 3, 4):
        assert np.array_equal(replenish_select(kp, sc, none, None, W, H, radius, pad, 3, 1, wanted), want[:wanted]), wanted
