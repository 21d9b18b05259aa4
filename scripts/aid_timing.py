"""Cost of the linear aiding measurement (ekfvio_aid_update, ekfvio_set_frame_aid).

Two measurements at N = 256, `reps` runs per case, alternating, every run a process of its own (one handle), started one after the other:

 1. Frames/s of ekfvio_step_image over 640 x 480 frames (replenish = 1: the loop a node runs):
      parent       the same loop on ANOTHER build of this repository (`--parent-tree`: a checkout of the parent commit with its library built
                   there): whether the feature, with nothing called, costs anything against the code before it
      off          this build, nothing called
      frame_aid    this build, the nonholonomic constraint v_x = v_y = 0 (variance 1e-3) as the standing measurement: two more launches
                   per frame behind the first
 2. Microseconds per call on the state that loop leaves (case `calls`): CALLS back-to-back ekfvio_aid_update calls with k = 1, 3, 6 (selection
    rows of the velocity and the body rate, diagonal R) and as many ekfvio_zupt_update calls, each batch timed from the first call to the
    end of ekfvio_synchronize, on the same handle.  The zero-velocity update is the same arithmetic at k = 6: the yardstick.

The kernels' durations and the launch lists come from a kernel trace of one run per case (the trace tool in front, this program behind `--`;
no counters in the same run):
    <trace tool> --kernel-trace --stats -d <dir> -- python scripts/aid_timing.py --child --case frame_aid
With nothing called the trace must list the parent's kernels, grids and counts: trace `--child --case off` and `--child --case parent --tree DIR`
and compare the two lists.  Tracing slows the host, so rates are taken without it.  The third part of "indistinguishable from the parent" is a
step of its own as well: `python bench.py --gpus 1 --steps 300 --warmup 20 --landmarks 256 --dump-outputs DIR` in both trees, the dumps compared
byte for byte.  Neither is done by this script.

Usage: python scripts/aid_timing.py [--frames 400] [--reps 9] [--parent-tree DIR] [--cases a b ...]
prints one JSON line per run and a last line with medians, ranges and the cost per frame, per launch and per call.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = np.array([400.0, 0, 320.0, 0, 400.0, 240.0, 0, 0, 1.0], np.float32)
WARM = 8
CASES = ("parent", "off", "frame_aid", "calls")
DEFAULT = ("off", "frame_aid", "calls")
LAUNCHES = 2  # per update: aid_gain_kernel, aid_joseph_kernel
CALLS = 2000
NHC_VARIANCE = 1e-3
CALL_VARIANCE = 1e-2  # (loose, so that 2000 updates in a row leave a usable covariance)


def selection(cols):
    H = np.zeros((len(cols), 22), np.float32)
    H[np.arange(len(cols)), list(cols)] = 1
    return H


def sequence(tree, frames):
    sys.path.insert(0, tree)
    from PIL import Image
    from ekf_vio_amd.sim import translated_sequence
    base = np.asarray(Image.open(os.path.join(HERE, "tests", "golden", "images", "640_480_test_gray.png")))
    return np.stack(translated_sequence(base, frames, dx=-1.4, dy=-0.45))


def per_call_us(v, fn):
    e = v.tc_ekf
    for _ in range(20):
        fn()
    e.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    e.synchronize()
    return 1e6 * (time.perf_counter() - t0) / CALLS


def child(a):
    """One run: a fresh handle of the build in a.tree, WARM frames untimed, the rest in four chunks; the rate is the median chunk's."""
    seq = np.load(a.seq) if a.seq else sequence(a.tree, WARM + a.frames)
    sys.path.insert(0, a.tree)
    from ekf_vio_amd import EKFVIO
    extra = {}  # (a build without the feature is never asked for it)
    if a.case == "frame_aid":
        extra["frame_aid"] = (-selection([7, 8]), np.zeros(2, np.float32), np.array([NHC_VARIANCE] * 2, np.float32))
    v = EKFVIO(max_features=256, replenish=1, fast_threshold=20, min_new_feature_dist=12, **extra)
    for i in range(WARM):  # first frame, replenishment, steady state
        v.addFrame(i / 30.0, seq[i], K)
    v.tc_ekf.synchronize()
    per, f, rates = (len(seq) - WARM) // 4, WARM, []
    t_all = time.perf_counter()
    for _ in range(4):
        t0 = time.perf_counter()
        for _ in range(per):
            v.addFrame(f / 30.0, seq[f], K)
            f += 1
        v.tc_ekf.synchronize()
        rates.append(per / (time.perf_counter() - t0))
    whole = 4 * per / (time.perf_counter() - t_all)
    st = v.tc_ekf.get_state()
    out = dict(case=a.case, frames=4 * per, frames_per_s=round(float(np.median(rates)), 1), frames_per_s_whole=round(whole, 1),
               landmarks=v.tc_ekf.num_features, live=int((st["del_flag"] == 0).sum()))
    if a.case == "frame_aid":
        out.update(v.aid_status())
    if a.case == "calls":
        e = v.tc_ekf
        us = {}
        for k, cols in ((1, [9]), (3, [7, 8, 9]), (6, [7, 8, 9, 10, 11, 12])):
            H, z, R = selection(cols), np.zeros(k, np.float32), np.array([CALL_VARIANCE] * k, np.float32)
            us["aid_k%d" % k] = round(per_call_us(v, lambda: e.aidUpdate(H, z, R)), 3)
        us["zupt"] = round(per_call_us(v, lambda: e.zuptUpdate(CALL_VARIANCE, CALL_VARIANCE)), 3)
        out.update(us_per_call=us, dim=e.dim, **e.aid_status())
    v.tc_ekf.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its loop as a further case")
    ap.add_argument("--cases", nargs="+", default=list(DEFAULT), choices=[c for c in CASES if c != "parent"])
    ap.add_argument("--child", action="store_true", help="one run in this process (what the driver starts; also the program to trace)")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--seq", default=None)
    ap.add_argument("--case", default="off", choices=CASES)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.reps < 1 or a.frames < 8:
        raise SystemExit("at least one run of at least 8 frames")
    cases = [(name, HERE) for name in a.cases]
    if a.parent_tree:
        cases.insert(0, ("parent", os.path.abspath(a.parent_tree)))
    res = {name: [] for name, _ in cases}
    calls = []
    with tempfile.TemporaryDirectory() as tmp:
        seq = os.path.join(tmp, "seq.npy")
        np.save(seq, sequence(HERE, WARM + a.frames))  # the same frames for every run of every case
        for rep in range(a.reps):
            for name, tree in cases:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--seq", seq, "--case", name]
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                if out.returncode != 0:  # a run that failed ends the measurement: nothing is started behind it
                    raise SystemExit("run %d of case %s failed (%d): %s" % (rep, name, out.returncode, out.stderr[-2000:]))
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
                print(line, flush=True)
                res[name].append(json.loads(line)["frames_per_s"])
                if name == "calls":
                    calls.append(json.loads(line)["us_per_call"])
    summary = dict(landmarks=256, frames=a.frames, reps=a.reps, launches_per_update=LAUNCHES, calls_per_batch=CALLS)
    for name, v in res.items():
        summary[name] = dict(median=float(np.median(v)), min=min(v), max=max(v), runs=v)
    overlap = lambda x, y: min(x) <= max(y) and min(y) <= max(x)
    if a.parent_tree and "off" in res:
        summary["off_vs_parent_ranges_overlap"] = bool(overlap(res["off"], res["parent"]))
    if "frame_aid" in res and "off" in res:
        us = round(1e6 * (1 / np.median(res["frame_aid"]) - 1 / np.median(res["off"])), 2)
        summary["us_per_frame_added_frame_aid_vs_off"] = us
        summary["us_per_launch_added_frame_aid_vs_off"] = round(us / LAUNCHES, 2)
    if calls:
        summary["us_per_call"] = {key: dict(median=float(np.median([c[key] for c in calls])), min=min(c[key] for c in calls),
                                            max=max(c[key] for c in calls)) for key in calls[0]}
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
