"""Cost of the camera models (ekfvio_set_camera_model) in the image loop.

Frames/s of ekfvio_step_image on the 640 x 480 translated sequence at N = 256 (replenish = 1: the loop a node runs), `reps` runs per case,
alternating, every run a process of its own (one handle, the same frames), started one after the other, each under a time limit of its
own; the first run that fails ends the measurement:
    parent         the same loop on ANOTHER build of this repository (`--parent-tree`: a checkout of the parent commit with its library
                   built there): whether the setting, switched off, costs anything against the code before it
    off            this build, no camera model set
    plumb_bob      this build, frames rectified with plumb_bob coefficients through ekfvio_set_camera_model (no P)
    equidistant    ... with the equidistant model
    equidistant_P  ... and a rectified camera P that zooms out (fx' = fy' = 300 over 400)

The lens model lives in the map alone, which is formed once per camera: the per-frame kernel (rectify_kernel) is the same code in the three
"on" cases and differs only in which bytes of the frame it taps.  The one-off durations of the three map kernel instances come from a kernel
trace of one run per case (the trace tool in front, this program behind `--`; no counters in the same run):
    <trace tool> --kernel-trace --stats -d <dir> -- python scripts/camera_model_timing.py --child --case equidistant
Tracing slows the host, so frames/s are taken without it.

Usage: python scripts/camera_model_timing.py [--frames 400] [--reps 9] [--parent-tree DIR]
prints one JSON line per run and a last line with medians and ranges.
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
CASES = ("parent", "off", "plumb_bob", "equidistant", "equidistant_P")
TRACE_ONLY = ("rational",)  # a case for `--child` alone: the third map instance's one-off duration in a trace
PLUMB_BOB, RATIONAL, EQUIDISTANT = 0, 1, 2
D_RATIONAL = (-0.28, 0.07, 2e-4, -1e-4, 0.01, 0.05, -0.02, 0.003)
D_PLUMB_BOB = (-0.28, 0.07, 2e-4, -1e-4, 0.0)
D_EQUIDISTANT = (-0.02, 0.01, -0.005, 0.001)
P_ZOOM_OUT = (300.0, 320.0, 300.0, 240.0)  # fx', cx', fy', cy'


def sequence(tree, frames):
    sys.path.insert(0, tree)
    from PIL import Image
    from ekf_vio_amd.sim import translated_sequence
    base = np.asarray(Image.open(os.path.join(HERE, "tests", "golden", "images", "640_480_test_gray.png")))
    return np.stack(translated_sequence(base, frames, dx=-1.4, dy=-0.45))


def child(a):
    """One run: a fresh handle of the build in a.tree, WARM frames untimed, the rest in four chunks; the rate is the median chunk's."""
    seq = np.load(a.seq) if a.seq else sequence(a.tree, WARM + a.frames)
    sys.path.insert(0, a.tree)
    from ekf_vio_amd import EKFVIO
    extra = {}  # (a build without the setting is never asked for it)
    if a.case == "plumb_bob":
        extra["camera_model"] = (PLUMB_BOB, D_PLUMB_BOB, None)
    elif a.case == "equidistant":
        extra["camera_model"] = (EQUIDISTANT, D_EQUIDISTANT, None)
    elif a.case == "rational":
        extra["camera_model"] = (RATIONAL, D_RATIONAL, None)
    elif a.case == "equidistant_P":
        extra["camera_model"] = (EQUIDISTANT, D_EQUIDISTANT, P_ZOOM_OUT)
    v = EKFVIO(max_features=256, replenish=1, fast_threshold=20, min_new_feature_dist=12, **extra)
    for i in range(WARM):  # first frame (with the setting on: its map), replenishment, steady state
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
    v.tc_ekf.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its loop as a further case")
    ap.add_argument("--child", action="store_true", help="one run in this process (what the driver starts; also the program to trace)")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--seq", default=None)
    ap.add_argument("--case", default="off", choices=CASES + TRACE_ONLY)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.reps < 1 or a.frames < 8:
        raise SystemExit("at least one run of at least 8 frames")
    cases = [(name, HERE) for name in CASES if name != "parent"]
    if a.parent_tree:
        cases.insert(0, ("parent", os.path.abspath(a.parent_tree)))
    res = {name: [] for name, _ in cases}
    with tempfile.TemporaryDirectory() as tmp:
        seq = os.path.join(tmp, "seq.npy")
        np.save(seq, sequence(HERE, WARM + a.frames))  # the same frames for every run of every case
        for rep in range(a.reps):
            for name, tree in cases:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--seq", seq, "--case", name]
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)  # (a run that hangs raises: nothing is started behind it)
                if out.returncode != 0:  # a run that failed ends the measurement likewise
                    raise SystemExit("run %d of case %s failed (%d): %s" % (rep, name, out.returncode, out.stderr[-2000:]))
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
                print(line, flush=True)
                res[name].append(json.loads(line)["frames_per_s"])
    summary = dict(landmarks=256, frames=a.frames, reps=a.reps)
    for name, v in res.items():
        summary[name] = dict(median=float(np.median(v)), min=min(v), max=max(v), runs=v)
    overlap = lambda x, y: min(x) <= max(y) and min(y) <= max(x)
    if a.parent_tree:
        summary["off_vs_parent_ranges_overlap"] = bool(overlap(res["off"], res["parent"]))
    us = lambda on, off: round(1e6 * (1 / np.median(res[on]) - 1 / np.median(res[off])), 2)
    summary["us_per_frame_added_by_plumb_bob"] = us("plumb_bob", "off")
    summary["us_per_frame_equidistant_over_plumb_bob"] = us("equidistant", "plumb_bob")
    summary["us_per_frame_equidistant_P_over_plumb_bob"] = us("equidistant_P", "plumb_bob")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
