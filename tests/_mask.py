"""Shared by tests/test_mask_cpu.py and tests/test_gpu_mask.py: the no-data mask (include/ekfvio.h, ekfvio_set_mask) restated in NumPy, step
by step, the detector's first fit and the tracker's pass rule restated on top of it, and the fixtures both files use.  Nothing here touches
a GPU.  References are computed once per case (lru_cache) and handed out as read-only arrays."""
import functools

import numpy as np

from oracle import circle_fill, fast_detect

import _rectify as rc

F32 = np.float32
BORDER = 1  # EKFVIO_MASK_RECTIFY_BORDER
D_TANGENTIAL = (0.0, 0.0, 0.02, -0.015)
K_HUGE = (1e-3, 1e-3, 320.0, 240.0)  # with D_HUGE: every map entry is the sentinel


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def nodata_full(w, h, K=None, D=None, mask=None, flags=0):
    """Step 1: n(x, y), bool [h, w]: the caller's mask is zero there, or (flag set, some coefficient nonzero) one of the four taps of the
    rectification map's entry has a non-zero weight and lies outside the frame."""
    n = np.zeros((h, w), bool)
    if mask is not None:
        n |= np.asarray(mask)[:h, :w] == 0
    if (flags & BORDER) and D is not None and any(float(v) != 0.0 for v in D):
        sx, sy, _ = rc.restate_map(K, D, w, h)
        sx, sy = sx.astype(np.int64), sy.astype(np.int64)
        ix, ax, iy, ay = sx >> 5, sx & 31, sy >> 5, sy & 31  # (arithmetic shift)

        def outside(xx, yy):
            return ~((xx >= 0) & (xx < w) & (yy >= 0) & (yy < h))
        n |= ((((32 - ax) * (32 - ay)) != 0) & outside(ix, iy)) | (((ax * (32 - ay)) != 0) & outside(ix + 1, iy)) | \
             ((((32 - ax) * ay) != 0) & outside(ix, iy + 1)) | (((ax * ay) != 0) & outside(ix + 1, iy + 1))
    return n


def nodata_level0(n, s):
    """Step 2: N(X, Y) = OR of n over the s x s block, bool [h // s, w // s]."""
    s = max(int(s), 1)
    h, w = n.shape
    H, W = h // s, w // s
    return n[:H * s, :W * s].reshape(H, s, W, s).any(axis=(1, 3))


def blocked(N, pad):
    """Step 3: B(X, Y) = OR of N over [X - pad, X + max(pad - 1, 0)] x the same window around Y, with N = 1 outside.  uint8 [H, W]."""
    pad = max(int(pad), 0)
    hi = max(pad - 1, 0)
    H, W = N.shape
    P = np.ones((H + pad + hi, W + pad + hi), bool)
    P[pad:pad + H, pad:pad + W] = N
    R = np.zeros((H + pad + hi, W), bool)
    for d in range(pad + hi + 1):  # X' = X - pad + d
        R |= P[:, d:d + W]
    B = np.zeros((H, W), bool)
    for d in range(pad + hi + 1):
        B |= R[d:d + H, :]
    return B.astype(np.uint8)


def restate(w, h, K=None, D=None, mask=None, s=1, pad=11, flags=0):
    """The three steps in a row."""
    return blocked(nodata_level0(nodata_full(w, h, K, D, mask, flags), s), pad)


def kill_box_complement(W, H, pad):
    """1 where Frame::isPixelInBox is false: x < pad || y < pad || W - x < pad || H - y < pad."""
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    return ((x < pad) | (y < pad) | (W - x < pad) | (H - y < pad)).astype(np.uint8)


def replenish_masked(img, existing_px, num_features, blocked_map, threshold=50, min_dist=30, kill_pad=11):
    """EKFVIO::replenishFeatures' first fit (oracle/fast_oracle.cpp, orc_replenish, line by line) with the occupancy image starting as
    `blocked_map` instead of empty: pixels (int32 [k, 2]) of the landmarks to add."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    ex = np.ascontiguousarray(existing_px, F32).reshape(-1, 2)
    if ex.shape[0] >= num_features:
        return np.zeros((0, 2), np.int32)
    xy, _ = fast_detect(img, threshold, True)
    occ = np.ascontiguousarray(np.where(np.asarray(blocked_map) != 0, 255, 0).astype(np.uint8))
    assert occ.shape == (h, w)
    for px, py in ex:
        circle_fill(occ, int(np.rint(px)), int(np.rint(py)), min_dist)  # cvRound: half to even
    needed, out, i = num_features - ex.shape[0], [], 0
    while i < needed and i < len(xy):
        x, y = int(xy[i, 0]), int(xy[i, 1])
        i += 1
        if occ[y, x] or x < kill_pad or y < kill_pad or w - x < kill_pad or h - y < kill_pad:
            needed += 1
            continue
        circle_fill(occ, x, y, min_dist)
        out.append((x, y))
    return np.array(out, np.int32).reshape(-1, 2)


def track_rule(q, before, B, pad):
    """The tracker's rule.  q: tracked pixels float32 [n, 2]; before: bool [n], the forward status and the forward-backward verdict; B: the
    blocked map of level 0.  Returns (pass, masked): the kill box in fp32 as the kernels test it, then B at cvRound(q), a rounded pixel
    outside level 0 counting as blocked; masked only where everything before the mask let the point through."""
    q = np.asarray(q, F32)
    H, W = B.shape
    ox, oy = q[:, 0], q[:, 1]
    with np.errstate(all="ignore"):
        box = (ox < pad) | (oy < pad) | (F32(W) - ox < pad) | (F32(H) - oy < pad)
        ix, iy = np.rint(ox).astype(np.int64), np.rint(oy).astype(np.int64)
    inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    blk = np.where(inside, B[np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)] != 0, True)
    p0 = np.asarray(before, bool) & ~box
    masked = p0 & blk
    return (p0 & ~masked).astype(np.uint8), masked.astype(np.uint8)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------
def user_mask(kind, w, h):
    """Caller's masks of the tests, uint8 [h, w], nonzero = scene."""
    m = np.full((h, w), 255, np.uint8)
    if kind == "rect":
        m[h // 3:h // 3 + max(h // 5, 2), w // 4:w // 4 + max(w // 3, 2)] = 0
    elif kind == "pixel":
        m[h // 2, w // 2 + 1] = 0
    elif kind == "lastcol":
        m[h // 3, w - 1] = 0
    elif kind != "ones":
        raise KeyError(kind)
    return m


def with_stride(m, extra=5):
    """The same mask as a view into a wider array (stride > width), the slack filled with zeros that must not be read as mask."""
    h, w = m.shape
    big = np.zeros((h, w + extra), np.uint8)
    big[:, :w] = m
    return big[:, :w]


@functools.lru_cache(maxsize=None)
def nodata_for(w, h, K, D, mask_kind, flags):
    mask = None if mask_kind is None else user_mask(mask_kind, w, h)
    return _frozen(nodata_full(w, h, None if K is None else rc.kmat(*K), D, mask, flags))


@functools.lru_cache(maxsize=None)
def blocked_for(w, h, K, D, mask_kind, s, pad, flags):
    """restate() for the fixtures' cases, cached: K = (fx, fy, cx, cy) or None, mask_kind = a name of user_mask or None."""
    return _frozen(blocked(nodata_level0(nodata_for(w, h, K, D, mask_kind, flags), s), pad))


@functools.lru_cache(maxsize=None)
def tiled_fixture(w, h):
    """The 640 x 480 fixture tiled to w x h."""
    f = rc.fixture()
    return _frozen(np.tile(f, ((h + 479) // 480, (w + 639) // 640))[:h, :w])
