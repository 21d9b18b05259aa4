"""Shared by tests/test_rectify_cpu.py and tests/test_gpu_rectify.py: the rectification of distorted frames (include/ekfvio.h,
ekfvio_set_distortion) restated in NumPy, line by line, and the helpers and fixtures both files use.  Nothing here touches a GPU.
References are computed once per case (lru_cache) and handed out as read-only arrays."""
import functools

import numpy as np

import _klt_fb as fb

F64 = np.float64
SENTINEL = np.int32(np.iinfo(np.int32).min)
K_CENTRE = (400.0, 400.0, 320.0, 240.0)   # fx, fy, cx, cy of the 640 x 480 fixture
K_OFF = (123.4, 98.7, 40.25, 71.5)        # an off-centre camera for small frames
# plumb_bob coefficient sets (k1, k2, p1, p2[, k3])
D_ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)
D_BARREL1 = (-0.28, 0.07, 2e-4, -1e-4, 0.0)
D_BARREL2 = (-0.4, 0.2, 1e-3, -2e-3, -0.05)
D_PINCUSHION = (0.15, -0.05, 0.0, 0.0)    # count 4: k3 = 0
D_HUGE = (50.0, 0.0, 0.0, 0.0, 0.0)       # with fx = 1e-3: u, v beyond 2^20, invalid entries


def kmat(fx, fy, cx, cy):
    """Row-major 3x3 as in CameraInfo.K, float32 (what the entry points take)."""
    return np.array([fx, 0, cx, 0, fy, cy, 0, 0, 1], np.float32)


def _cam(K):
    K = np.asarray(K, np.float32).reshape(9)
    return F64(K[0]), F64(K[2]), F64(K[4]), F64(K[5])


def _coeffs(D):
    d = [F64(v) for v in D] + [F64(0.0)] * (5 - len(D))
    assert len(D) in (0, 4, 5)
    return d


def restate_map(K, D, w, h):
    """include/ekfvio.h, rectification, the fp64 block line by line (NumPy's float64 operations are IEEE, one rounding each, nothing
    fused).  Returns (sx, sy, valid): int32 [h, w] with SENTINEL where invalid."""
    fx, cx, fy, cy = _cam(K)
    k1, k2, p1, p2, k3 = _coeffs(D)
    x, y = np.meshgrid(np.arange(w, dtype=F64), np.arange(h, dtype=F64))
    with np.errstate(all="ignore"):
        xn = (x - cx) / fx
        yn = (y - cy) / fy
        xx = xn * xn
        yy = yn * yn
        xy = xn * yn
        r2 = xx + yy
        rad = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = (xn * rad + (2.0 * p1) * xy) + p2 * (r2 + 2.0 * xx)
        yd = (yn * rad + p1 * (r2 + 2.0 * yy)) + (2.0 * p2) * xy
        u = fx * xd + cx
        v = fy * yd + cy
        valid = (np.abs(u) <= 2.0 ** 20) & (np.abs(v) <= 2.0 ** 20)  # (a NaN compares false)
        sx = np.where(valid, np.rint(np.where(valid, u, 0.0) * 32.0), F64(SENTINEL)).astype(np.int32)  # rint: half to even
        sy = np.where(valid, np.rint(np.where(valid, v, 0.0) * 32.0), F64(SENTINEL)).astype(np.int32)
    return sx, sy, valid


def restate_remap(img, sx, sy):
    """The integer half: four taps with 5-bit weights, a tap outside the frame contributes 0, (sum + 512) >> 10."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    sx, sy = sx.astype(np.int64), sy.astype(np.int64)
    ix, ax, iy, ay = sx >> 5, sx & 31, sy >> 5, sy & 31  # (arithmetic shift)

    def tap(xx, yy):
        inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(inside, img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64), 0)
    s = (tap(ix, iy) * (32 - ax) * (32 - ay) + tap(ix + 1, iy) * ax * (32 - ay) + tap(ix, iy + 1) * (32 - ax) * ay +
         tap(ix + 1, iy + 1) * ax * ay)
    out = (s + 512) >> 10
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def remap(img, K, D):
    """What a handle with coefficients D makes of the uploaded frame `img` with intrinsics K: the restated map, then the restated remap."""
    h, w = np.asarray(img).shape
    sx, sy, _ = restate_map(K, D, w, h)
    return restate_remap(img, sx, sy)


def distort(img, K, D):
    """What a camera with the coefficients D sees where a pinhole camera with the same K sees `img`.  For every pixel (u, v) of the
    distorted image the model is inverted by 50 fixed-point iterations in fp64 (xn <- (xd - tangential(xn)) / rad(xn), from xn = xd),
    the original is sampled there with float bilinear weights, and a sample that needs a pixel outside the original is 0.
    Independent of the restatement above: it shares no line with it but the model."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    fx, cx, fy, cy = _cam(K)
    k1, k2, p1, p2, k3 = _coeffs(D)
    u, v = np.meshgrid(np.arange(w, dtype=F64), np.arange(h, dtype=F64))
    xd, yd = (u - cx) / fx, (v - cy) / fy
    xn, yn = xd.copy(), yd.copy()
    for _ in range(50):
        r2 = xn * xn + yn * yn
        rad = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        dx = 2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn)
        dy = p1 * (r2 + 2.0 * yn * yn) + 2.0 * p2 * xn * yn
        xn, yn = (xd - dx) / rad, (yd - dy) / rad
    px, py = fx * xn + cx, fy * yn + cy
    x0, y0 = np.floor(px), np.floor(py)
    a, b = px - x0, py - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    inside = (x0 >= 0) & (x0 + 1 < w) & (y0 >= 0) & (y0 + 1 < h)
    xc, yc = np.clip(x0, 0, w - 2), np.clip(y0, 0, h - 2)
    f = img.astype(F64)
    val = (f[yc, xc] * (1 - a) * (1 - b) + f[yc, xc + 1] * a * (1 - b) + f[yc + 1, xc] * (1 - a) * b + f[yc + 1, xc + 1] * a * b)
    return np.where(inside, np.clip(np.rint(val), 0, 255), 0).astype(np.uint8)


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def fixture():
    return fb.image("first")  # 640 x 480, read-only


@functools.lru_cache(maxsize=None)
def crop(x0, y0, w, h):
    return _frozen(fixture()[y0:y0 + h, x0:x0 + w])


@functools.lru_cache(maxsize=None)
def remapped(D, K=K_CENTRE, box=None):
    """remap(fixture or its crop `box` = (x0, y0, w, h), kmat(*K), D), cached."""
    img = fixture() if box is None else crop(*box)
    return _frozen(remap(img, kmat(*K), D))


@functools.lru_cache(maxsize=None)
def distorted(D, K=K_CENTRE):
    return _frozen(distort(fixture(), kmat(*K), D))
