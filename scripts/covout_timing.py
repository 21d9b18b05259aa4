"""Cost of publishing the covariances of the outputs (ekfvio_set_output_covariance) in the image loop.

Frames/s of ekfvio_step_image on the 640 x 480 translated sequence at N = 256 (replenish = 1: the loop a node runs) with the setting off
and with it on, `reps` runs each, alternating.  Every run is a process of its own (one handle, the same frames), started one after the
other, so that a third case can take part: the same loop on ANOTHER build of this repository (`--parent-tree`: a checkout of the parent
commit, e.g. `git worktree add <dir> HEAD~1` and its library built there), which shows whether the feature, switched off, costs anything
against the code before it.  With the setting on a frame loses its early publication (its outputs go out behind the update's last GEMM,
not in front of it) and its outputs kernel runs longer; the runs of this build also time the two on-demand getters (one launch and one
wait per call, the setting off), which is what a caller pays who asks for a covariance now and then.

The durations of frame_outputs_kernel, odom_cov_kernel and points_cov_kernel come from a kernel trace of one run (the trace tool in front,
this program behind `--`):
    <trace tool> --kernel-trace --stats -d <dir> -- python scripts/covout_timing.py --child --on
and the rows of the kernels in its kernel statistics; the same trace of a run without `--on`, and of the parent's build, lists the kernels,
grids and counts of the off path.  Tracing slows the host, so frames/s are taken without it.

Usage: python scripts/covout_timing.py [--frames 400] [--reps 9] [--parent-tree DIR]
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
GETTER_CALLS = 200


def sequence(tree, frames):
    sys.path.insert(0, tree)
    from PIL import Image
    from ekf_vio_amd.sim import translated_sequence
    base = np.asarray(Image.open(os.path.join(HERE, "tests", "golden", "images", "640_480_test_gray.png")))
    return np.stack(translated_sequence(base, frames, dx=-1.4, dy=-0.45))


def child(a):
    """One run: a fresh handle of the build in a.tree, WARM frames untimed, the rest in four chunks; the rate is the median chunk's.  As in a
    node, every frame's outputs are read: odometry and cloud always, the covariances too where the setting is on."""
    seq = np.load(a.seq) if a.seq else sequence(a.tree, WARM + a.frames)
    sys.path.insert(0, a.tree)
    from ekf_vio_amd import EKFVIO
    extra = {"output_covariance": True} if a.on else {}  # (a build without the feature is never asked for it)
    v = EKFVIO(max_features=256, replenish=1, fast_threshold=20, min_new_feature_dist=12, **extra)

    def frame(f):
        v.addFrame(f / 30.0, seq[f], K)
        v.odometry()
        v.points()
        if a.on:
            v.odometry_covariance()
            v.points_covariance()

    for i in range(WARM):  # first frame, replenishment, steady state
        frame(i)
    v.tc_ekf.synchronize()
    per, f, rates = (len(seq) - WARM) // 4, WARM, []
    t_all = time.perf_counter()
    for _ in range(4):
        t0 = time.perf_counter()
        for _ in range(per):
            frame(f)
            f += 1
        v.tc_ekf.synchronize()
        rates.append(per / (time.perf_counter() - t0))
    whole = 4 * per / (time.perf_counter() - t_all)
    c = v.tc_ekf.counters()
    out = dict(case=a.case, on=bool(a.on), frames=4 * per, frames_per_s=round(float(np.median(rates)), 1), frames_per_s_whole=round(whole, 1),
               landmarks=v.tc_ekf.num_features, early_output_frames=c["early_output_frames"])
    if a.getters:  # the on-demand road: the setting off, so each call is one launch and one wait
        v.setOutputCovariance(False)
        for name, fn in (("odometry_covariance_us", v.odometry_covariance), ("points_covariance_us", v.points_covariance)):
            fn()
            t0 = time.perf_counter()
            for _ in range(GETTER_CALLS):
                fn()
            out[name] = round(1e6 * (time.perf_counter() - t0) / GETTER_CALLS, 2)
    v.tc_ekf.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its loop as a third case")
    ap.add_argument("--child", action="store_true", help="one run in this process (what the driver starts; also the program to trace)")
    ap.add_argument("--on", action="store_true", help="(child) with the covariances in every frame's outputs")
    ap.add_argument("--getters", action="store_true", help="(child) also time the on-demand getters behind the loop")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--seq", default=None)
    ap.add_argument("--case", default="run")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.reps < 1 or a.frames < 8:
        raise SystemExit("at least one run of at least 8 frames")
    cases = [("off", HERE, False), ("on", HERE, True)]
    if a.parent_tree:
        cases.insert(0, ("parent", os.path.abspath(a.parent_tree), False))
    res = {name: [] for name, _, _ in cases}
    getters = {"odometry_covariance_us": [], "points_covariance_us": []}
    with tempfile.TemporaryDirectory() as tmp:
        seq = os.path.join(tmp, "seq.npy")
        np.save(seq, sequence(HERE, WARM + a.frames))  # the same frames for every run of every case
        for rep in range(a.reps):
            for name, tree, on in cases:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--seq", seq, "--case", name]
                cmd += (["--on"] if on else []) + (["--getters"] if name == "off" else [])
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                if out.returncode != 0:  # a run that failed ends the measurement: nothing is started behind it
                    raise SystemExit("run %d of case %s failed (%d): %s" % (rep, name, out.returncode, out.stderr[-2000:]))
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
                print(line, flush=True)
                row = json.loads(line)
                res[name].append(row["frames_per_s"])
                for k in getters:
                    if k in row:
                        getters[k].append(row[k])
    summary = dict(landmarks=256, frames=a.frames, reps=a.reps)
    for name, v in res.items():
        summary[name] = dict(median=float(np.median(v)), min=min(v), max=max(v), runs=v)
    for k, v in getters.items():
        summary[k] = dict(median=float(np.median(v)), min=min(v), max=max(v))
    overlap = lambda x, y: min(x) <= max(y) and min(y) <= max(x)
    if a.parent_tree:
        summary["off_vs_parent_ranges_overlap"] = bool(overlap(res["off"], res["parent"]))
    summary["us_per_frame_added_by_the_setting"] = round(1e6 * (1 / np.median(res["on"]) - 1 / np.median(res["off"])), 2)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
