"""NumPy restatement of one Lucas-Kanade pass of the tracker (csrc/klt.hip, klt_lk_pass; oracle/klt_oracle.cpp, orc_klt_track), with the
gain/offset term of include/ekfvio.h (ekfvio_set_klt_photometric) behind a switch.  One point at a time: nothing is vectorised over
points, a window is.  It works on KltFrame.level(l) of the oracle: image borders are reflect-101, derivative borders zero.  Every fp32
line is one NumPy float32 operation (IEEE, one rounding each, nothing fused); the sums are exact Python integers."""
import numpy as np

F32 = np.float32
W_BITS = 14
FLT_SCALE = F32(1.0 / (1 << 20))
FLT_EPSILON = F32(1.1920929e-07)
CLAMP = 4080


def reflect101(p, n):
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    period = 2 * (n - 1)
    p = np.mod(p, period)
    return np.where(p >= n, period - p, p)


class Pyramid:
    """The levels of an oracle KltFrame as int32 arrays: img [h, w], dx and dy [h, w]."""

    def __init__(self, frame):
        self.levels = frame.levels
        self.lv = []
        for l in range(frame.levels):
            img, der = frame.level(l)
            self.lv.append((img.astype(np.int32), der[:, :, 0].astype(np.int32), der[:, :, 1].astype(np.int32)))


def _rows(img, x0, y0, n):
    """img at rows y0 .. y0+n-1, columns x0 .. x0+n-1, through the reflect-101 border"""
    h, w = img.shape
    return img[reflect101(np.arange(y0, y0 + n), h)][:, reflect101(np.arange(x0, x0 + n), w)]


def _rows_zero(a, x0, y0, n):
    """the same with a zero border"""
    h, w = a.shape
    ys, xs = np.arange(y0, y0 + n), np.arange(x0, x0 + n)
    out = a[np.clip(ys, 0, h - 1)][:, np.clip(xs, 0, w - 1)].copy()
    out[(ys < 0) | (ys >= h), :] = 0
    out[:, (xs < 0) | (xs >= w)] = 0
    return out


def _weights(a, b):
    one, s = F32(1.0), F32(1 << W_BITS)
    iw00 = int(np.rint(((one - a) * (one - b)) * s))
    iw01 = int(np.rint((a * (one - b)) * s))
    iw10 = int(np.rint(((one - a) * b) * s))
    return iw00, iw01, iw10, (1 << W_BITS) - iw00 - iw01 - iw10


def _bilinear(p, win, iw, shift):
    """p: (win + 1) x (win + 1) integers; descale(p00 iw00 + p01 iw01 + p10 iw10 + p11 iw11, shift)"""
    p = p.astype(np.int64)
    v = p[:win, :win] * iw[0] + p[:win, 1:] * iw[1] + p[1:, :win] * iw[2] + p[1:, 1:] * iw[3]
    return (v + (1 << (shift - 1))) >> shift


def _f32_of_int(v):
    """(float) of an exact integer below 2^53: one rounding"""
    assert abs(int(v)) < (1 << 53)
    return F32(np.float64(int(v)))


def project(Iv, Ix, Iy):
    """include/ekfvio.h, the gain/offset term: (Ix', Iy', info) of one window's pixels (any shape; n = their count)."""
    iv, ix, iy = (np.asarray(a, np.int64) for a in (Iv, Ix, Iy))
    n = int(iv.size)
    sI, sX, sY = int(iv.sum()), int(ix.sum()), int(iy.sum())
    sII, sIX, sIY = int((iv * iv).sum()), int((iv * ix).sum()), int((iv * iy).sum())
    VI, CX, CY = n * sII - sI * sI, n * sIX - sI * sX, n * sIY - sI * sY
    assert VI >= 0
    fn = _f32_of_int(n)
    mI, mX, mY = _f32_of_int(sI) / fn, _f32_of_int(sX) / fn, _f32_of_int(sY) / fn
    cx = _f32_of_int(CX) / _f32_of_int(VI) if VI > 0 else F32(0.0)
    cy = _f32_of_int(CY) / _f32_of_int(VI) if VI > 0 else F32(0.0)
    dI = iv.astype(F32) - mI

    def one(g, m, c):
        r = np.rint((g.astype(F32) - m) - c * dI)
        assert r.dtype == F32
        return r.astype(np.int64)

    rx, ry = one(ix, mX, cx), one(iy, mY, cy)
    info = dict(VI=VI, clamped=int((np.abs(rx) > CLAMP).sum() + (np.abs(ry) > CLAMP).sum()))
    return np.clip(rx, -CLAMP, CLAMP), np.clip(ry, -CLAMP, CLAMP), info


def _template(lv, ppx, ppy, ipx, ipy, win):
    img, dx, dy = lv
    iw = _weights(ppx - F32(ipx), ppy - F32(ipy))
    return (_bilinear(_rows(img, ipx, ipy, win + 1), win, iw, W_BITS - 5), _bilinear(_rows_zero(dx, ipx, ipy, win + 1), win, iw, W_BITS),
            _bilinear(_rows_zero(dy, ipx, ipy, win + 1), win, iw, W_BITS))


def template_at(P, level, p, win=21):
    """(Iv, Ix, Iy), win x win integers each: the template a pass forms at `level` for the point p (level-0 pixels)."""
    sc, half = F32(1.0 / (1 << level)), F32((win - 1) * 0.5)
    ppx, ppy = F32(p[0]) * sc - half, F32(p[1]) * sc - half
    return _template(P.lv[level], ppx, ppy, int(np.floor(ppx)), int(np.floor(ppy)), win)


def lk_pass(P, Q, p, guess, win=21, max_iter=30, epsilon=0.01, min_eig=1e-4, photo=False):
    """One pass for one point: template = pyramid P at p, search in pyramid Q from guess.  Returns ((ox, oy) float32, status)."""
    levels = min(P.levels, Q.levels)
    eps2 = F32(epsilon) * F32(epsilon)
    min_eig = F32(min_eig)
    half = F32((win - 1) * 0.5)
    px, py = F32(p[0]), F32(p[1])
    ox, oy = F32(guess[0]), F32(guess[1])
    ok = True
    for level in range(levels - 1, -1, -1):
        Iimg, Idx, Idy = P.lv[level]
        Jimg = Q.lv[level][0]
        Ih, Iw = Iimg.shape
        Jh, Jw = Jimg.shape
        sc = F32(1.0 / (1 << level))
        ppx, ppy = px * sc, py * sc
        if level == levels - 1:
            ox, oy = ox * sc, oy * sc
        else:
            ox, oy = ox * F32(2.0), oy * F32(2.0)
        ppx, ppy = ppx - half, ppy - half
        ipx, ipy = int(np.floor(ppx)), int(np.floor(ppy))
        if ipx < -win or ipx >= Iw or ipy < -win or ipy >= Ih:
            if level == 0:
                ok = False
            continue
        Iv, Ix, Iy = _template(P.lv[level], ppx, ppy, ipx, ipy, win)
        if photo:
            Ix, Iy, _ = project(Iv, Ix, Iy)
        A11 = _f32_of_int((Ix * Ix).sum()) * FLT_SCALE
        A12 = _f32_of_int((Ix * Iy).sum()) * FLT_SCALE
        A22 = _f32_of_int((Iy * Iy).sum()) * FLT_SCALE
        D = A11 * A22 - A12 * A12
        minEig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F32(4.0) * A12 * A12)) / F32(2 * win * win)
        if minEig < min_eig or D < FLT_EPSILON:
            if level == 0:
                ok = False
            continue
        D = F32(1.0) / D
        nx, ny = ox - half, oy - half
        pdx = pdy = F32(0.0)
        for j in range(max_iter):
            inx, iny = int(np.floor(nx)), int(np.floor(ny))
            if inx < -win or inx >= Jw or iny < -win or iny >= Jh:
                if level == 0:
                    ok = False
                break
            jw = _weights(nx - F32(inx), ny - F32(iny))
            diff = _bilinear(_rows(Jimg, inx, iny, win + 1), win, jw, W_BITS - 5) - Iv
            b1 = _f32_of_int((diff * Ix).sum()) * FLT_SCALE
            b2 = _f32_of_int((diff * Iy).sum()) * FLT_SCALE
            dx = (A12 * b2 - A22 * b1) * D
            dy = (A12 * b1 - A11 * b2) * D
            nx, ny = nx + dx, ny + dy
            ox, oy = nx + half, ny + half
            if dx * dx + dy * dy <= eps2:
                break
            if j > 0 and abs(dx + pdx) < F32(0.01) and abs(dy + pdy) < F32(0.01):
                ox, oy = ox - dx * F32(0.5), oy - dy * F32(0.5)
                break
            pdx, pdy = dx, dy
        if ok and level == 0:
            fx, fy = int(np.floor(ox - half)), int(np.floor(oy - half))
            if fx < -win or fx >= Jw or fy < -win or fy >= Jh:
                ok = False
    for v in (ox, oy):
        assert type(v) is F32, type(v)
    return (ox, oy), ok


def track(P, Q, prev_px, init_px, photo=False, **kw):
    """klt_track's outputs for every point: (next_px [n, 2] float32, status [n] uint8)."""
    prev_px = np.asarray(prev_px, F32).reshape(-1, 2)
    init_px = np.asarray(init_px, F32).reshape(-1, 2)
    out, st = np.zeros_like(prev_px), np.zeros(len(prev_px), np.uint8)
    for i in range(len(prev_px)):
        (out[i, 0], out[i, 1]), ok = lk_pass(P, Q, prev_px[i], init_px[i], photo=photo, **kw)
        st[i] = 1 if ok else 0
    return out, st


def track_fb(P, Q, prev_px, init_px, max_px=0.0, photo=False, **kw):
    """ekfvio_klt_track_points_fb's outputs (include/ekfvio.h, forward-backward check): the forward pass and, from its result, the pass
    back.  Returns (next_px, status, back_px, err2, fb_ok)."""
    prev_px = np.asarray(prev_px, F32).reshape(-1, 2)
    init_px = np.asarray(init_px, F32).reshape(-1, 2)
    n = len(prev_px)
    t2 = F32(max_px) * F32(max_px)
    out, st = np.zeros_like(prev_px), np.zeros(n, np.uint8)
    back, err2, fb_ok = prev_px.copy(), np.full(n, -1.0, F32), np.zeros(n, np.uint8)
    for i in range(n):
        p, g = prev_px[i], init_px[i]
        (qx, qy), ok = lk_pass(P, Q, p, g, photo=photo, **kw)
        out[i], st[i] = (qx, qy), 1 if ok else 0
        if not ok:
            continue
        bx, by = qx - (g[0] - p[0]), qy - (g[1] - p[1])
        (rx, ry), sb = lk_pass(Q, P, (qx, qy), (bx, by), photo=photo, **kw)
        dx, dy = rx - p[0], ry - p[1]
        e2 = dx * dx + dy * dy
        back[i] = (rx, ry)
        err2[i] = e2 if sb else F32(-2.0)
        fb_ok[i] = 1 if (sb and (e2 <= t2 if t2 > 0 else True)) else 0
    return out, st, back, err2, fb_ok
