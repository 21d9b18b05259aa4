"""Shared by tests/test_equalize_cpu.py, tests/test_gpu_equalize.py and tests/test_gpu_host_shim_equalize.py: the equalisation of pushed
frames (include/ekfvio.h, ekfvio_set_equalize) restated in NumPy, step by step, and the helpers and fixtures the files use.  Nothing here
touches a GPU.  References are computed once per case (lru_cache) and handed out as read-only arrays."""
import functools
import math

import numpy as np

import _klt_fb as fb

F32 = np.float32
K_CENTRE = (400.0, 400.0, 320.0, 240.0)
SETTING = (3.0, 8, 8)


def kmat(fx, fy, cx, cy):
    return np.array([fx, 0, cx, 0, fy, cy, 0, 0, 1], np.float32)


def params(w, h, clip_limit, tx, ty):
    """The host values of the specification: dict(tw, th, A, clip, scale, inv_tw, inv_th), the last three fp32."""
    assert 1 <= tx <= w and 1 <= ty <= h
    tw, th = -(-w // tx), -(-h // ty)
    A = tw * th
    c = math.floor(float(np.float64(F32(clip_limit)) * np.float64(A) / np.float64(256.0)))
    clip = max(int(min(c, A)), 1)  # (a value above A is taken as A: no bin holds more)
    return dict(tw=tw, th=th, A=A, clip=clip, scale=F32(255.0) / F32(A), inv_tw=F32(1.0) / F32(tw), inv_th=F32(1.0) / F32(th))


def _reflect(n_padded, n):
    X = np.arange(n_padded)
    r = np.where(X >= n, 2 * (n - 1) - X, X)
    assert r.min() >= 0
    return r


def restate_tiles(img, clip_limit, tx, ty):
    """Steps 1-4.  Returns (lut uint8 [ty, tx, 256], info) with info = dict(excess, res, step: int arrays [ty, tx]; hist_sum_ok)."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    p = params(w, h, clip_limit, tx, ty)
    tw, th, A, clip = p["tw"], p["th"], p["A"], p["clip"]
    padded = img[_reflect(ty * th, h)][:, _reflect(tx * tw, w)]  # step 1
    lut = np.zeros((ty, tx, 256), np.uint8)
    excess_all, res_all, step_all = (np.zeros((ty, tx), np.int64) for _ in range(3))
    b = np.arange(256)
    for j in range(ty):
        for i in range(tx):
            tile = padded[j * th:(j + 1) * th, i * tw:(i + 1) * tw]
            hist = np.bincount(tile.reshape(-1), minlength=256).astype(np.int64)  # step 2
            assert hist.sum() == A
            excess = int(np.maximum(hist - clip, 0).sum())  # step 3
            hist = np.minimum(hist, clip)
            batch = excess // 256
            res = excess - 256 * batch
            hist = hist + batch
            step = 1
            if res > 0:
                step = max(256 // res, 1)
                hist = hist + ((b % step == 0) & (b // step < res)).astype(np.int64)
            assert hist.sum() == A
            cum = np.cumsum(hist)  # step 4: the integer sum -> fp32 (exact below 2^24), one fp32 product, rint half to even
            lut[j, i] = np.clip(np.rint(cum.astype(F32) * p["scale"]), 0, 255).astype(np.uint8)
            excess_all[j, i], res_all[j, i], step_all[j, i] = excess, res, step
    return lut, dict(excess=excess_all, res=res_all, step=step_all)


def _axis(n, inv_t, tiles):
    x = np.arange(n, dtype=np.int64).astype(F32)
    fx = (x * F32(inv_t)).astype(F32) - F32(0.5)
    t = np.floor(fx).astype(F32)
    a = (fx - t).astype(F32)
    a1 = (F32(1.0) - a).astype(F32)
    ti = t.astype(np.int64)
    return np.maximum(ti, 0), np.minimum(ti + 1, tiles - 1), a, a1


def restate(img, clip_limit, tx, ty):
    """include/ekfvio.h, equalisation, steps 1-5 (NumPy's float32 operations are IEEE, one rounding each, nothing fused)."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    p = params(w, h, clip_limit, tx, ty)
    lut, _ = restate_tiles(img, clip_limit, tx, ty)
    i1, i2, xa, xa1 = _axis(w, p["inv_tw"], tx)
    j1, j2, ya, ya1 = _axis(h, p["inv_th"], ty)
    v = img.astype(np.int64)
    J1, J2, I1, I2 = j1[:, None], j2[:, None], i1[None, :], i2[None, :]
    xa, xa1, ya, ya1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    l11, l12 = lut[J1, I1, v].astype(F32), lut[J1, I2, v].astype(F32)
    l21, l22 = lut[J2, I1, v].astype(F32), lut[J2, I2, v].astype(F32)
    top = ((l11 * xa1).astype(F32) + (l12 * xa).astype(F32)).astype(F32)
    bot = ((l21 * xa1).astype(F32) + (l22 * xa).astype(F32)).astype(F32)
    out = ((top * ya1).astype(F32) + (bot * ya).astype(F32)).astype(F32)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def contrast(img, gain, offset):
    """The synthetic photometric change: rint(g * I + o) clipped to a byte."""
    return np.clip(np.rint(np.float64(gain) * np.asarray(img, np.float64) + np.float64(offset)), 0, 255).astype(np.uint8)


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def fixture(which="first"):
    return fb.image(which)  # 640 x 480, read-only


@functools.lru_cache(maxsize=None)
def crop(x0, y0, w, h):
    return _frozen(fixture()[y0:y0 + h, x0:x0 + w])


@functools.lru_cache(maxsize=None)
def quarter_contrast():
    return _frozen(contrast(fixture(), 0.25, 96))


@functools.lru_cache(maxsize=None)
def constant(w=640, h=480, value=117):
    return _frozen(np.full((h, w), value, np.uint8))


@functools.lru_cache(maxsize=None)
def checkerboard(w=96, h=64, lo=40, hi=200):
    y, x = np.mgrid[0:h, 0:w]
    return _frozen(np.where((x + y) % 2 == 0, lo, hi).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def spiky(w=64, h=64):
    """A frame whose tiles hold 200 equally filled grey levels: with 2 x 2 tiles of 32 x 32 and clip limit 1 (clip = 4) every such level
    loses the same amount, and `res` comes out above 128 (so step = 1)."""
    rng = np.random.RandomState(7)
    vals = np.repeat(np.arange(200, dtype=np.uint8), 5)  # 1000 of a tile's 1024 pixels: five per level
    out = np.zeros((h, w), np.uint8)
    for j in range(2):
        for i in range(2):
            t = np.concatenate([vals, rng.randint(200, 256, 24).astype(np.uint8)])
            rng.shuffle(t)
            out[j * 32:(j + 1) * 32, i * 32:(i + 1) * 32] = t.reshape(32, 32)
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def restated(key, clip_limit, tx, ty):
    """restate() of a named input, cached: key is "first", "moved", "quarter", "constant", or a crop box (x0, y0, w, h) of the fixture."""
    if isinstance(key, tuple):
        img = crop(*key)
    elif key == "quarter":
        img = quarter_contrast()
    elif key == "constant":
        img = constant()
    else:
        img = fixture(key)
    return _frozen(restate(img, clip_limit, tx, ty))
