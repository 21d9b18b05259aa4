"""Shared by tests/test_camera_models_cpu.py and tests/test_gpu_camera_models.py: the camera models of include/ekfvio.h
(ekfvio_set_camera_model) restated in NumPy, line by line, atan_spec included; an independent inverse of each model, used to synthesise the
raw frames a distorting camera would deliver; and the fixtures both files use.  Nothing here touches a GPU.  References are computed once per
case (lru_cache) and handed out as read-only arrays.

Conventions: K is the row-major 3 x 3 of the entry points (tests/_rectify.py, kmat); P is (fx', cx', fy', cy') as the entry points take it, or
None; the (fx, fy, cx, cy) order of tests/_rectify.py's K tuples is turned into either by kmat() and p4()."""
import functools

import numpy as np

import _rectify as rc

F64 = np.float64
PLUMB_BOB, RATIONAL, EQUIDISTANT = 0, 1, 2
COUNTS = {PLUMB_BOB: (0, 4, 5), RATIONAL: (8,), EQUIDISTANT: (4,)}
NAMES = {PLUMB_BOB: "plumb_bob", RATIONAL: "rational", EQUIDISTANT: "equidistant"}

# coefficient sets of the tests
D_EQUI_ZERO = (0.0, 0.0, 0.0, 0.0)                       # the ideal fisheye lens
D_EQUI = (-0.02, 0.01, -0.005, 0.001)
D_EQUI_TUMVI = (0.0034823894022493434, 0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182)
D_RATIONAL = (-0.28, 0.07, 2e-4, -1e-4, 0.01, 0.05, -0.02, 0.003)
D_RATIONAL_POLE = (0.0, 0.0, 0.0, 0.0, 0.0, -4.0, 0.0, 0.0)  # den = 1 - 4 r2: zero on the circle r = 1/2, inside a 640 x 480 frame with f = 400
K_TUMVI = (190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504)  # fx, fy, cx, cy
P_ZOOM = (440.0, 440.0, 330.0, 236.0)                    # fx, fy, cx, cy of a rectified camera that is not the raw one
P_SMALL = (100.0, 90.0, 35.5, 20.25)                     # likewise for the 67 x 45 frames
K_SMALL = (40.0, 40.0, 33.0, 22.0)


def p4(fx, fy, cx, cy):
    """(fx, fy, cx, cy) of tests/_rectify.py -> P as the entry points take it: float32 (fx', cx', fy', cy')."""
    return np.array([fx, cx, fy, cy], np.float32)


def _coeffs(model, D):
    assert len(D) in COUNTS[model], (model, len(D))
    return [F64(v) for v in D] + [F64(0.0)] * (8 - len(D))


def _primed(K, P):
    fx, cx, fy, cy = rc._cam(K)
    if P is None:
        return fx, cx, fy, cy
    P = np.asarray(P, np.float32).reshape(4)
    return F64(P[0]), F64(P[1]), F64(P[2]), F64(P[3])


# c_k = (k even ? +1 : -1) * (1.0 / (2k + 1)), k = 0 .. 19
ATAN_C = [(1.0 if k % 2 == 0 else -1.0) * (1.0 / (2 * k + 1)) for k in range(20)]
T8, PI_4, PI_2 = 0.41421356237309503, 0.7853981633974483, 1.5707963267948966


def atan_spec(r):
    """include/ekfvio.h, atan_spec, line by line for an array of r >= 0 (NumPy's float64 operations are IEEE, one rounding each)."""
    r = np.asarray(r, F64)
    with np.errstate(all="ignore"):
        inv = r > 1.0
        t = np.where(inv, 1.0 / r, r)
        sh = t > T8
        t = np.where(sh, (t - 1.0) / (t + 1.0), t)
        q = t * t
        p = np.full_like(q, ATAN_C[19])
        for k in range(18, -1, -1):
            p = p * q + ATAN_C[k]
        a = t * p
        a = np.where(sh, PI_4 + a, a)
        a = np.where(inv, PI_2 - a, a)
    return a


def restate_map(K, model, D, P, w, h, atan=atan_spec):
    """include/ekfvio.h, camera models, the fp64 block line by line.  Returns (sx, sy, valid): int32 [h, w] with SENTINEL where invalid.
    atan: what the equidistant line calls (atan_spec; np.arctan for the comparison of the two)."""
    fx, cx, fy, cy = rc._cam(K)
    fxp, cxp, fyp, cyp = _primed(K, P)
    d = _coeffs(model, D)
    x, y = np.meshgrid(np.arange(w, dtype=F64), np.arange(h, dtype=F64))
    with np.errstate(all="ignore"):
        xn = (x - cxp) / fxp
        yn = (y - cyp) / fyp
        xx = xn * xn
        yy = yn * yn
        xy = xn * yn
        r2 = xx + yy
        if model == EQUIDISTANT:
            k1, k2, k3, k4 = d[:4]
            r = np.sqrt(r2)
            th = atan(r)
            t2 = th * th
            thd = th * (1.0 + (((k4 * t2 + k3) * t2 + k2) * t2 + k1) * t2)
            sc = np.where(r == 0.0, 1.0, thd / r)
            xd = xn * sc
            yd = yn * sc
        else:
            k1, k2, p1, p2, k3, k4, k5, k6 = d
            rad = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
            if model == RATIONAL:
                den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2
                rad = rad / den
            xd = (xn * rad + (2.0 * p1) * xy) + p2 * (r2 + 2.0 * xx)
            yd = (yn * rad + p1 * (r2 + 2.0 * yy)) + (2.0 * p2) * xy
        u = fx * xd + cx
        v = fy * yd + cy
        valid = (np.abs(u) <= 2.0 ** 20) & (np.abs(v) <= 2.0 ** 20)  # (a NaN compares false)
        sx = np.where(valid, np.rint(np.where(valid, u, 0.0) * 32.0), F64(rc.SENTINEL)).astype(np.int32)  # rint: half to even
        sy = np.where(valid, np.rint(np.where(valid, v, 0.0) * 32.0), F64(rc.SENTINEL)).astype(np.int32)
    return sx, sy, valid


def remap(img, K, model, D, P):
    """What a handle with this camera model makes of the uploaded frame `img` with intrinsics K: the restated map, then tests/_rectify.py's
    restated integer remap (which no model changes)."""
    h, w = np.asarray(img).shape
    sx, sy, _ = restate_map(K, model, D, P, w, h)
    return rc.restate_remap(img, sx, sy)


def nodata_from_map(sx, sy, w, h):
    """include/ekfvio.h, mask, step 1, the border term on a given map: a tap with a non-zero weight lies outside the frame."""
    sx, sy = sx.astype(np.int64), sy.astype(np.int64)
    ix, ax, iy, ay = sx >> 5, sx & 31, sy >> 5, sy & 31  # (arithmetic shift)

    def outside(xx, yy):
        return ~((xx >= 0) & (xx < w) & (yy >= 0) & (yy < h))
    return ((((32 - ax) * (32 - ay)) != 0) & outside(ix, iy)) | (((ax * (32 - ay)) != 0) & outside(ix + 1, iy)) | \
           ((((32 - ax) * ay) != 0) & outside(ix, iy + 1)) | (((ax * ay) != 0) & outside(ix + 1, iy + 1))


# ---- the independent inverse: what a distorting camera sees --------------------------------------------------------------------------
def undistort_points(model, D, xd, yd):
    """Distorted normalised coordinates -> ideal ones, (xn, yn, ok).  Shares no line with restate_map but the model: the equidistant
    model by Newton on theta (np.tan for the way back), the polynomial ones by the fixed-point iteration of tests/_rectify.py's distort
    with rad = num / den."""
    d = _coeffs(model, D)
    with np.errstate(all="ignore"):
        if model == EQUIDISTANT:
            k1, k2, k3, k4 = d[:4]
            thd = np.hypot(xd, yd)
            th = thd.copy()
            for _ in range(30):
                t2 = th * th
                f = th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - thd
                fp = 1.0 + t2 * (3.0 * k1 + t2 * (5.0 * k2 + t2 * (7.0 * k3 + t2 * 9.0 * k4)))
                th = th - f / fp
            ok = (th >= 0.0) & (th < 1.55)  # (a ray at 90 degrees has no pinhole image)
            scale = np.where(thd > 0.0, np.tan(np.where(ok, th, 0.0)) / np.where(thd > 0.0, thd, 1.0), 1.0)
            return xd * scale, yd * scale, ok
        k1, k2, p1, p2, k3, k4, k5, k6 = d
        xn, yn = xd.copy(), yd.copy()
        for _ in range(50):
            r2 = xn * xn + yn * yn
            rad = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
            dx = 2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn)
            dy = p1 * (r2 + 2.0 * yn * yn) + 2.0 * p2 * xn * yn
            xn, yn = (xd - dx) / rad, (yd - dy) / rad
        return xn, yn, np.isfinite(xn) & np.isfinite(yn)


def distort(img, model, K, D, P):
    """What a camera (K, D) of this model sees where a pinhole camera P (None: K) sees `img`.  For every pixel (u, v) of the raw image the
    model is inverted (undistort_points), the original is sampled at (fx' xn + cx', fy' yn + cy') with float bilinear weights, and a sample
    that needs a pixel outside the original is 0."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    fx, cx, fy, cy = rc._cam(K)
    fxp, cxp, fyp, cyp = _primed(K, P)
    u, v = np.meshgrid(np.arange(w, dtype=F64), np.arange(h, dtype=F64))
    xn, yn, ok = undistort_points(model, D, (u - cx) / fx, (v - cy) / fy)
    px, py = np.where(ok, fxp * xn + cxp, -10.0), np.where(ok, fyp * yn + cyp, -10.0)
    x0, y0 = np.floor(px), np.floor(py)
    a, b = px - x0, py - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    inside = ok & (x0 >= 0) & (x0 + 1 < w) & (y0 >= 0) & (y0 + 1 < h)
    xc, yc = np.clip(x0, 0, w - 2), np.clip(y0, 0, h - 2)
    f = img.astype(F64)
    val = (f[yc, xc] * (1 - a) * (1 - b) + f[yc, xc + 1] * a * (1 - b) + f[yc + 1, xc] * (1 - a) * b + f[yc + 1, xc + 1] * a * b)
    return np.where(inside, np.clip(np.rint(val), 0, 255), 0).astype(np.uint8)


# ---- cached references -------------------------------------------------------------------------------------------------------------------
def _p(P):
    return None if P is None else p4(*P)


@functools.lru_cache(maxsize=None)
def map_for(K, model, D, P, w, h):
    """restate_map for K, P = (fx, fy, cx, cy) tuples (P may be None), cached: (sx, sy, valid), read-only."""
    return tuple(rc._frozen(a) for a in restate_map(rc.kmat(*K), model, D, _p(P), w, h))


@functools.lru_cache(maxsize=None)
def remapped(K, model, D, P, box=None):
    """remap(fixture or its crop `box` = (x0, y0, w, h)) for K, P = (fx, fy, cx, cy) tuples, cached."""
    img = rc.fixture() if box is None else rc.crop(*box)
    h, w = img.shape
    sx, sy, _ = map_for(K, model, D, P, w, h)
    return rc._frozen(rc.restate_remap(img, sx, sy))


@functools.lru_cache(maxsize=None)
def distorted(K, model, D, P):
    return rc._frozen(distort(rc.fixture(), model, rc.kmat(*K), D, _p(P)))
