"""Cost of rectifying distorted frames on the device (ekfvio_set_distortion) in the image loop.

Frames/s of ekfvio_step_image on the 640 x 480 translated sequence at N = 256 (replenish = 1: the loop a node runs) with the
rectification off and with it on (plumb_bob coefficients `--distortion`), `reps` runs each, alternating.  Every run is a process of its
own (one handle, the same frames), started one after the other, so that a third case can take part: the same loop on ANOTHER build of
this repository (`--parent-tree`: a checkout of the parent commit, e.g. `git worktree add <dir> HEAD~1` and its library built there),
which shows whether the rectification, switched off, costs anything against the code before it.

The durations of rectify_kernel and of the one-off rectify_map_kernel come from a kernel trace of one run (the trace tool in front, this
program behind `--`):
    <trace tool> --kernel-trace --stats -d <dir> -- python scripts/rectify_timing.py --child --on
and the rows of the two kernels in its kernel statistics; the same trace of a run without `--on`, and of the parent's build, lists the
kernels, grids and counts of the off path.  Tracing slows the host, so frames/s are taken without it.

Usage: python scripts/rectify_timing.py [--frames 400] [--reps 9] [--distortion k1 k2 p1 p2 k3] [--parent-tree DIR]
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
    extra = {"distortion": a.distortion} if a.on else {}  # (a build without the rectification is never asked for it)
    v = EKFVIO(max_features=256, replenish=1, fast_threshold=20, min_new_feature_dist=12, **extra)
    for i in range(WARM):  # first frame (with the rectification on: its map), replenishment, steady state
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
    out = dict(case=a.case, on=bool(a.on), frames=4 * per, frames_per_s=round(float(np.median(rates)), 1), frames_per_s_whole=round(whole, 1),
               landmarks=v.tc_ekf.num_features, live=int((st["del_flag"] == 0).sum()))
    v.tc_ekf.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--distortion", type=float, nargs=5, default=[-0.28, 0.07, 2e-4, -1e-4, 0.0], metavar=("K1", "K2", "P1", "P2", "K3"))
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its loop as a third case")
    ap.add_argument("--child", action="store_true", help="one run in this process (what the driver starts; also the program to trace)")
    ap.add_argument("--on", action="store_true", help="(child) with the rectification on")
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
    with tempfile.TemporaryDirectory() as tmp:
        seq = os.path.join(tmp, "seq.npy")
        np.save(seq, sequence(HERE, WARM + a.frames))  # the same frames for every run of every case
        for rep in range(a.reps):
            for name, tree, on in cases:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--seq", seq, "--case", name, "--distortion"] + [repr(d) for d in a.distortion]
                out = subprocess.run(cmd + (["--on"] if on else []), capture_output=True, text=True, timeout=300)
                if out.returncode != 0:  # a run that failed ends the measurement: nothing is started behind it
                    raise SystemExit("run %d of case %s failed (%d): %s" % (rep, name, out.returncode, out.stderr[-2000:]))
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
                print(line, flush=True)
                res[name].append(json.loads(line)["frames_per_s"])
    summary = dict(landmarks=256, frames=a.frames, reps=a.reps, distortion=a.distortion)
    for name, v in res.items():
        summary[name] = dict(median=float(np.median(v)), min=min(v), max=max(v), runs=v)
    overlap = lambda x, y: min(x) <= max(y) and min(y) <= max(x)
    if a.parent_tree:
        summary["off_vs_parent_ranges_overlap"] = bool(overlap(res["off"], res["parent"]))
    summary["us_per_frame_added_by_the_rectification"] = round(1e6 * (1 / np.median(res["on"]) - 1 / np.median(res["off"])), 2)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
