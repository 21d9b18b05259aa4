"""Shared by tests/test_klt_fb_cpu.py and tests/test_gpu_klt_fb.py: the forward-backward check of the tracker (include/ekfvio.h,
ekfvio_set_klt_fb) restated around two calls of the CPU oracle's tracker, and the fixtures both files use.  Nothing here touches a
GPU.  References are computed once per case (lru_cache) and handed out as read-only arrays."""
import functools
import os

import numpy as np
from PIL import Image

from oracle import KltFrame, klt_track

IMG = os.path.join(os.path.dirname(__file__), "golden", "images")
F32 = np.float32
BLOCK = (250, 180, 400, 300)  # x0, y0, x1, y1 of the pasted texture in the second image
FLOW = {"moved": (-21.0, -7.0), "blocked": (-21.0, -7.0), "identical": (0.0, 0.0)}  # true flow of the plain pairs
EDGE_POINTS = [[5.0, 5.0], [-40.0, 100.0], [700.0, 100.0], [639.0, 479.0], [320.5, 0.25]]


def grey(name):
    return np.asarray(Image.open(os.path.join(IMG, name + "_gray.png")))


@functools.lru_cache(maxsize=None)
def image(which):
    """The first image ("first") and the second ones: "moved", "shear", "identical", and "blocked" = the moved image with a 150 x 120
    block of foreign texture (another part of the first image) pasted over it, built here from the committed images."""
    a = grey("640_480_test")
    if which in ("first", "identical"):
        out = a
    elif which == "moved":
        out = grey("640_480_moved_test")
    elif which == "shear":
        out = grey("640_480_shear_test")
    elif which == "blocked":
        out = grey("640_480_moved_test").copy()
        out[180:300, 250:400] = a[40:160, 60:210]
    elif which == "blocked_identical":
        out = a.copy()
        out[180:300, 250:400] = a[40:160, 60:210]
    else:
        raise KeyError(which)
    out = np.ascontiguousarray(out)
    out.setflags(write=False)
    return out


def grid_points(n=8):
    xs, ys = np.linspace(80, 560, n), np.linspace(60, 420, n)
    return np.array([[x, y] for y in ys for x in xs], F32)


def all_points():
    """The 8-grid, 150 points of the 13-grid and the border / out-of-image points of tests/test_gpu_klt.py: 219 points."""
    return np.vstack([grid_points(8), grid_points(13)[:150], EDGE_POINTS]).astype(F32)


def inside_block(dest, margin=11):
    """True where a destination pixel lies at least `margin` px inside the pasted block."""
    x0, y0, x1, y1 = BLOCK
    d = np.asarray(dest, np.float64)
    return (d[:, 0] >= x0 + margin) & (d[:, 0] <= x1 - 1 - margin) & (d[:, 1] >= y0 + margin) & (d[:, 1] <= y1 - 1 - margin)


def restate_fb(A, B, p, g, max_px, **klt):
    """include/ekfvio.h, forward-backward check, line by line: klt_track(A, B, p, g), then klt_track(B, A, q, b), then the three fp32
    lines.  A, B: oracle KltFrame of the previous / current image; klt: win, max_iter, epsilon, min_eig of klt_track.
    Returns dict(q, s_f, back, err2, fb_ok, rejected): back = r where s_f == 1 else p; err2 = e2, -1 where s_f == 0, -2 where the
    backward track failed; fb_ok = 0 where s_f == 0; with max_px == 0, fb_ok is the backward status alone."""
    p = np.ascontiguousarray(p, F32).reshape(-1, 2)
    g = np.ascontiguousarray(g, F32).reshape(-1, 2)
    q, s_f, _ = klt_track(A, B, p, g.copy(), **klt)
    fwd = s_f == 1
    with np.errstate(all="ignore"):
        b = (q - (g - p)).astype(F32)  # bx = qx - (gx - px): two fp32 subtractions
        # (the backward call is made for every point; where s_f == 0 its input is replaced and its output ignored)
        r, s_b, _ = klt_track(B, A, np.where(fwd[:, None], q, p).astype(F32), np.where(fwd[:, None], b, p).astype(F32), **klt)
        d = (r - p).astype(F32)
        e2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F32)  # each product and the sum rounded to fp32: nothing fused
        t2 = F32(max_px) * F32(max_px)
        within = (e2 <= t2) if max_px > 0 else np.ones(len(p), bool)  # (a NaN compares false: rejected)
    fb_ok = fwd & (s_b == 1) & within
    err2 = np.where(fwd, np.where(s_b == 1, e2, F32(-2.0)), F32(-1.0)).astype(F32)
    out = dict(q=q, s_f=s_f, back=np.where(fwd[:, None], r, p).astype(F32), err2=err2, fb_ok=fb_ok.astype(np.uint8),
               rejected=(fwd & ~fb_ok).astype(np.uint8))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def frame(which, win=21, levels=3, shrink=1):
    img = image(which)
    if shrink > 1:
        img = np.ascontiguousarray(img[::shrink, ::shrink])
    return KltFrame(img, win=win, max_level=levels)


@functools.lru_cache(maxsize=None)
def reference(second, offset_guess, max_px, win=21, levels=3, iters=30, shrink=1):
    """restate_fb for all_points() (divided by `shrink` on a subsampled image) from "first" into `second`; guess = the points, or
    the points + (-20, -6) (a coarse prediction, as the filter would give).  Returns (points, guess, restatement)."""
    pts = (all_points() / F32(shrink)).astype(F32)
    guess = (pts + np.array([-20.0, -6.0], F32) / F32(shrink)).astype(F32) if offset_guess else pts.copy()
    A, B = frame("first", win, levels, shrink), frame(second, win, levels, shrink)
    ref = restate_fb(A, B, pts, guess, max_px, win=win, max_iter=iters)
    pts.setflags(write=False), guess.setflags(write=False)
    return pts, guess, ref
