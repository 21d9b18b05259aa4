"""Shared by tests/test_replenish_grid_cpu.py and tests/test_gpu_replenish_grid.py: the replenishment's selection with the grid
(include/ekfvio.h, ekfvio_set_replenish_grid) restated in pure Python, line by line, and the fixtures both files use.  Nothing here touches a
GPU, and nothing here calls the library under test: the circle is drawing.cpp's midpoint walk written out again, the cells' maxima and their
order are Python's max() and sorted() on tuples."""
import functools

import numpy as np

from oracle import fast_detect

import _rectify as rc


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def circle_spans(radius):
    """drawing.cpp Circle(), filled: {row offset: half-width} of the spans the midpoint walk draws (the widest where a row is drawn twice)."""
    spans = {}

    def hline(dy, half):
        spans[dy] = max(spans.get(dy, -1), half)
    err, dx, dy, plus, minus = 0, radius, 0, 1, (radius << 1) - 1
    while dx >= dy:
        hline(-dy, dx), hline(dy, dx), hline(-dx, dy), hline(dx, dy)
        dy += 1
        err += plus
        plus += 2
        m = (1 if err <= 0 else 0) - 1  # 0 or -1
        err -= minus & m
        dx += m
        minus -= m & 2
    return spans


def stamp(O, cx, cy, spans):
    H, W = O.shape
    for dy, half in spans.items():
        y = cy + dy
        if 0 <= y < H:
            xa, xb = max(cx - half, 0), min(cx + half, W - 1)
            if xa <= xb:
                O[y, xa:xb + 1] = 1


def in_box(x, y, W, H, pad):
    """Frame::isPixelInBox"""
    return not (x < pad or y < pad or W - x < pad or H - y < pad)


def select(kp_xy, score, existing_px, B, W, H, radius, pad, cells_x, cells_y, wanted, rounds=None):
    """The specification.  kp_xy int [nk, 2] in raster order, score int [nk], existing_px int [n, 2] (the landmarks' ROUNDED pixels), B uint8
    [H, W] or None.  Returns int32 [added, 2] in the order taken.  cells_x = cells_y = 0: the raster first fit.  rounds: a list that receives
    the number of landmarks each round took."""
    kp = [(int(x), int(y)) for x, y in np.asarray(kp_xy).reshape(-1, 2)]
    s = [int(v) for v in np.asarray(score).reshape(-1)]
    ex = [(int(x), int(y)) for x, y in np.asarray(existing_px).reshape(-1, 2)]
    spans = circle_spans(int(radius))
    O = np.zeros((H, W), np.uint8) if B is None else (np.asarray(B) != 0).astype(np.uint8)
    assert O.shape == (H, W)
    for px, py in ex:
        stamp(O, px, py, spans)
    out = []
    if cells_x == 0 and cells_y == 0:
        for x, y in kp:
            if len(out) >= wanted:
                break
            if in_box(x, y, W, H, pad) and O[y, x] == 0:
                out.append((x, y))
                stamp(O, x, y, spans)
        return np.array(out, np.int32).reshape(-1, 2)
    cw, ch = -(-W // cells_x), -(-H // cells_y)

    def cell(x, y):
        return (y // ch) * cells_x + x // cw
    cnt = [0] * (cells_x * cells_y)
    for px, py in ex:
        if 0 <= px < W and 0 <= py < H:
            cnt[cell(px, py)] += 1
    # (per keypoint, once: the kill-box test and the cell; NumPy only to keep the rounds of a large frame quick)
    xs, ys = np.array([p[0] for p in kp], np.int64), np.array([p[1] for p in kp], np.int64)
    boxed = np.array([in_box(x, y, W, H, pad) for x, y in kp], bool)
    cells = np.array([cell(x, y) for x, y in kp], np.int64)
    while len(out) < wanted:
        best = {}
        for k in np.flatnonzero(boxed & (O[ys, xs] == 0)) if len(kp) else []:  # the candidates, k ascending
            c, k = int(cells[k]), int(k)
            if c not in best or s[k] > s[best[c]]:  # (ties stay with the smaller k, which came first)
                best[c] = k
        if not best:
            break
        L = sorted(best.items(), key=lambda ck: (cnt[ck[0]], -s[ck[1]], ck[1]))  # cnt as it stands now: the walk below changes it
        took = 0
        for c, k in L:
            if len(out) >= wanted:
                break
            x, y = kp[k]
            if O[y, x] == 0:
                out.append((x, y))
                stamp(O, x, y, spans)
                cnt[c] += 1
                took += 1
        assert took >= 1  # the first entry of L is always taken
        if rounds is not None:
            rounds.append(took)
    return np.array(out, np.int32).reshape(-1, 2)


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------------
THRESHOLD, RADIUS, PAD = 50, 30, 11  # Params.h defaults: FAST_THRESHOLD, MIN_NEW_FEATURE_DIST, KILL_PAD
SMALL_THRESHOLD, SMALL_RADIUS, SMALL_PAD = 20, 5, 4  # the crops: enough corners, and circles that leave room for more than one landmark
CROP = {"64x48": (300, 200, 64, 48), "67x45": (131, 77, 67, 45)}  # x0, y0, w, h in the 640 x 480 fixture


@functools.lru_cache(maxsize=None)
def image(name):
    """'640x480': the fixture; '64x48', '67x45': its crops; 'periodic': a synthetic 96 x 80 image of identical bright pixels on a 16-pixel lattice,
    whose corners tie in score; '1024x768': the fixture tiled (more level-0 pixels than the occupancy image in LDS holds)."""
    if name == "640x480":
        return rc.fixture()
    if name in CROP:
        return rc.crop(*CROP[name])
    if name == "1024x768":
        return _frozen(np.tile(rc.fixture(), (2, 2))[:768, :1024])
    if name == "periodic":
        img = np.full((80, 96), 40, np.uint8)
        for y0 in range(8, 80 - 8, 16):
            for x0 in range(8, 96 - 8, 16):
                img[y0, x0] = 220  # (one pixel: FAST's ring around it is all dark, and no neighbour is a corner for the non-maximum suppression to compare)
        return _frozen(img)
    raise KeyError(name)


def params(name):
    """(threshold, radius, kill_pad) the tests use with image(name)."""
    return (THRESHOLD, RADIUS, PAD) if name in ("640x480", "1024x768") else (SMALL_THRESHOLD, SMALL_RADIUS, SMALL_PAD)


@functools.lru_cache(maxsize=None)
def keypoints(name):
    """The oracle's cv::FAST(image(name), threshold, nonmax): (xy, score), read-only."""
    xy, sc = fast_detect(image(name), params(name)[0], True)
    return _frozen(xy), _frozen(sc)


def crowd(W, H, n, quadrant=3):
    """n existing landmark pixels crowded into one quadrant (0: top left .. 3: bottom right), int32 [n, 2]; some share a pixel's neighbourhood,
    one lies outside the frame (it stamps what of its circle reaches in and counts for no cell)."""
    x0, y0 = (quadrant % 2) * (W // 2), (quadrant // 2) * (H // 2)
    rng = np.random.RandomState(1234 + n + quadrant)
    px = np.stack([x0 + rng.randint(0, max(W // 2, 1), n), y0 + rng.randint(0, max(H // 2, 1), n)], axis=1).astype(np.int32)
    if n:
        px[-1] = (W + 2, H // 2)
    return px


def lower_half(W, H, step=40):
    """Existing landmarks that fill the lower half of the frame on a `step` lattice."""
    xs, ys = np.meshgrid(np.arange(step // 2, W, step), np.arange(H // 2 + step // 2, H, step))
    return np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int32)


def spread(px, W, H, cells_x=8, cells_y=6):
    """(distinct cells of a cells_x x cells_y grid that hold one of the pixels, their mean row)."""
    px = np.asarray(px).reshape(-1, 2)
    if len(px) == 0:
        return 0, float("nan")
    cw, ch = -(-W // cells_x), -(-H // cells_y)
    return len(set(((px[:, 1] // ch) * cells_x + px[:, 0] // cw).tolist())), float(px[:, 1].mean())
