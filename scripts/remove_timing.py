"""Cost of landmark removal on the device (ekfvio_remove_features, cfg.remove_lost).

  * the removal's device time at N = 256 and N = 1024, with 10 % and 50 % of the landmarks removed: HIP events on the handle's
    stream around ekfvio_remove_features(NULL), whose device work is the removal kernel and the one-thread kernel that
    publishes the count; and the wall time of the whole call with a host mask (staging copy, launch, wait);
  * frames/s of ekfvio_step_image with remove_lost = 0 and 1 on a long translated_sequence (same run, replenish = 1).

Usage: python scripts/remove_timing.py [--frames 400] [--reps 20]; prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ekf_vio_amd import EKFVIO, TightlyCoupledEKF  # noqa: E402
from ekf_vio_amd.sim import translated_sequence  # noqa: E402

K = np.array([500.0, 0, 320.0, 0, 500.0, 240.0, 0, 0, 1.0], np.float32)


def removal_us(N, frac, reps):
    """Median wall time of ekfvio_remove_features(mask) over `reps` calls, each from the same state."""
    rng = np.random.default_rng(N)
    n = 22 + 3 * N
    A = rng.standard_normal((n, n)).astype(np.float32)
    st = dict(base_mu=np.r_[np.zeros(3), [1, 0, 0, 0], np.zeros(15)].astype(np.float32),
              feat_mu=rng.standard_normal((N, 3)).astype(np.float32), last_klt=rng.standard_normal((N, 2)).astype(np.float32),
              del_flag=np.zeros(N, np.uint8), Sigma=np.ascontiguousarray((A + A.T) / 2))
    m = np.zeros(N, np.uint8)
    m[rng.choice(N, int(round(frac * N)), replace=False)] = 1
    g = TightlyCoupledEKF(max_features=N)
    times = []
    for r in range(reps + 2):
        g.set_state(st)
        t0 = time.perf_counter()
        g.removeFeatures(m)
        t1 = time.perf_counter()
        if r >= 2:
            times.append(1e6 * (t1 - t0))
    g.close()
    return float(np.median(times))


def _hip():
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    for name in ("hipStreamCreate", "hipEventCreate", "hipEventRecord", "hipEventSynchronize", "hipEventElapsedTime",
                 "hipEventDestroy", "hipStreamDestroy"):
        getattr(hip, name).restype = C.c_int
    return hip


def kernel_us(N, frac):
    """Median device time between two HIP events around ekfvio_remove_features(NULL) on the handle's stream: the removal kernel
    and the one-thread kernel that publishes the count."""
    import ctypes as C
    hip = _hip()
    rng = np.random.default_rng(N + 1)
    n = 22 + 3 * N
    A = rng.standard_normal((n, n)).astype(np.float32)
    st = dict(base_mu=np.r_[np.zeros(3), [1, 0, 0, 0], np.zeros(15)].astype(np.float32),
              feat_mu=rng.standard_normal((N, 3)).astype(np.float32), last_klt=rng.standard_normal((N, 2)).astype(np.float32),
              del_flag=np.zeros(N, np.uint8), Sigma=np.ascontiguousarray((A + A.T) / 2))
    m = np.zeros(N, np.uint8)
    m[rng.choice(N, int(round(frac * N)), replace=False)] = 1
    s, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0 and hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    g = TightlyCoupledEKF(max_features=N, stream=s.value)
    out = []
    for r in range(12):
        g.set_state(dict(st, del_flag=m))  # the flags decide (remove == NULL): no staging copy
        hip.hipEventRecord(e0, s)
        g.removeFeatures(None)
        hip.hipEventRecord(e1, s)
        hip.hipEventSynchronize(e1)
        ms = C.c_float(0)
        hip.hipEventElapsedTime(C.byref(ms), e0, e1)
        if r >= 2:
            out.append(1e3 * ms.value)
    g.close()
    hip.hipEventDestroy(e0), hip.hipEventDestroy(e1), hip.hipStreamDestroy(s)
    return float(np.median(out))


def loop_fps(seq, remove_lost, chunks=4):
    v = EKFVIO(max_features=256, replenish=1, remove_lost=remove_lost, fast_threshold=20, min_new_feature_dist=12)
    for i in range(8):  # warm-up: first frame, replenishment, graph-free steady state
        v.addFrame(i / 30.0, seq[i % len(seq)], K)
    per = (len(seq) - 8) // chunks
    rates, live = [], []
    f = 8
    for c in range(chunks):
        t0 = time.perf_counter()
        for _ in range(per):
            v.addFrame(f / 30.0, seq[f], K)
            f += 1
        rates.append(per / (time.perf_counter() - t0))
    st = v.tc_ekf.get_state()
    live = int((st["del_flag"] == 0).sum())
    n = v.tc_ekf.num_features
    v.tc_ekf.close()
    return float(np.median(rates)), n, live


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    res = {"removal_call_us": {}, "removal_kernel_us": {}}
    for N in (256, 1024):
        for frac in (0.1, 0.5):
            key = "N%d_%d%%" % (N, int(100 * frac))
            res["removal_call_us"][key] = removal_us(N, frac, args.reps)
            res["removal_kernel_us"][key] = kernel_us(N, frac)
    seq = translated_sequence(np.asarray(__import__("PIL.Image", fromlist=["Image"]).open(
        os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "images", "640_480_test_gray.png"))),
        args.frames, dx=-1.4, dy=-0.45)
    for rl in (0, 1):
        fps, n, live = loop_fps(seq, rl)
        res["image_loop_remove_lost_%d" % rl] = {"frames_per_s": fps, "final_landmarks": n, "final_live": live}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
