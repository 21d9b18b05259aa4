"""Cost of spreading new landmarks over a grid (ekfvio_set_replenish_grid) in the image loop.

Frames/s of ekfvio_step_image on the 640 x 480 translated sequence at N = 256, `reps` runs per case and loop, alternating, every run a
process of its own (one handle, the same frames), started one after the other.  Two loops:
    plain      replenish = 1: the filter fills on the first frame and the detector does not run again while it stays full
    churn      replenish = 1, remove_lost = 1: lost landmarks leave in their frame, so the detector and the selection run in every frame
and four cases:
    parent     the same loop on ANOTHER build of this repository (`--parent-tree`: a checkout of the parent commit with its library built
               there): whether the grid, switched off, costs anything against the code before it
    off        this build, the grid off: the raster first fit
    8x6        this build, the grid at 8 x 6
    1x1        this build, the grid at 1 x 1: strongest corner first, one landmark per round -- the most rounds a frame can need
Every run also reports the first frame's wall time (the first fill: up to 256 wanted, the most rounds of the run), the landmarks it took,
and the landmarks added per later frame: a round adds at least one landmark, so a frame that adds k ran between 1 and k rounds.

The duration of replenish_select_kernel and the launch list come from a kernel trace of one run per case (the trace tool in front, this
program behind `--`; no counters in the same run):
    <trace tool> --kernel-trace --stats -d <dir> -- python scripts/replenish_grid_timing.py --child --case 8x6 --loop churn
Tracing slows the host, so frames/s are taken without it.

Usage: python scripts/replenish_grid_timing.py [--frames 400] [--reps 9] [--parent-tree DIR]
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
CASES = ("parent", "off", "8x6", "1x1")
LOOPS = ("plain", "churn")
GRID = {"8x6": (8, 6), "1x1": (1, 1)}


def sequence(tree, frames):
    sys.path.insert(0, tree)
    from PIL import Image
    from ekf_vio_amd.sim import translated_sequence
    base = np.asarray(Image.open(os.path.join(HERE, "tests", "golden", "images", "640_480_test_gray.png")))
    return np.stack(translated_sequence(base, frames, dx=-1.4, dy=-0.45))


def child(a):
    """One run: a fresh handle of the build in a.tree, WARM frames untimed (the first one timed on its own), the rest in four chunks; the
    rate is the median chunk's."""
    seq = np.load(a.seq) if a.seq else sequence(a.tree, WARM + a.frames)
    sys.path.insert(0, a.tree)
    from ekf_vio_amd import EKFVIO
    extra = dict(remove_lost=1) if a.loop == "churn" else {}
    v = EKFVIO(max_features=256, replenish=1, fast_threshold=20, min_new_feature_dist=12, **extra)
    if a.case in GRID:  # (a build without the grid is never asked for it)
        v.setReplenishGrid(*GRID[a.case])
    v.tc_ekf.synchronize()
    t0 = time.perf_counter()
    v.addFrame(0.0, seq[0], K)  # the first fill
    v.tc_ekf.synchronize()
    first_ms = 1e3 * (time.perf_counter() - t0)
    first_taken = v.tc_ekf.num_features
    for i in range(1, WARM):
        v.addFrame(i / 30.0, seq[i], K)
    v.tc_ekf.synchronize()
    per, f, rates, added = (len(seq) - WARM) // 4, WARM, [], []
    last_id = int(v.landmark_ids()[0].max()) if v.tc_ekf.num_features else -1
    t_all = time.perf_counter()
    for _ in range(4):
        t0 = time.perf_counter()
        for _ in range(per):
            v.addFrame(f / 30.0, seq[f], K)
            f += 1
        v.tc_ekf.synchronize()
        rates.append(per / (time.perf_counter() - t0))
        # (between the chunks, outside the timed part: how many landmarks entered during the chunk)
        ids = v.landmark_ids()[0]
        top = int(ids.max()) if len(ids) else last_id
        added.append(top - last_id)
        last_id = top
    whole = 4 * per / (time.perf_counter() - t_all)
    st = v.tc_ekf.get_state()
    out = dict(case=a.case, loop=a.loop, frames=4 * per, frames_per_s=round(float(np.median(rates)), 1), frames_per_s_whole=round(whole, 1),
               first_frame_ms=round(first_ms, 3), first_fill_taken=first_taken, landmarks=v.tc_ekf.num_features,
               live=int((st["del_flag"] == 0).sum()), entered_per_frame=round(sum(added) / (4.0 * per), 3))
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
    ap.add_argument("--case", default="off", choices=CASES)
    ap.add_argument("--loop", default="churn", choices=LOOPS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.reps < 1 or a.frames < 8:
        raise SystemExit("at least one run of at least 8 frames")
    cases = [(name, HERE) for name in CASES if name != "parent"]
    if a.parent_tree:
        cases.insert(0, ("parent", os.path.abspath(a.parent_tree)))
    res = {(loop, name): [] for loop in LOOPS for name, _ in cases}
    first = {(loop, name): [] for loop in LOOPS for name, _ in cases}
    entered = {(loop, name): [] for loop in LOOPS for name, _ in cases}
    with tempfile.TemporaryDirectory() as tmp:
        seq = os.path.join(tmp, "seq.npy")
        np.save(seq, sequence(HERE, WARM + a.frames))  # the same frames for every run of every case
        for rep in range(a.reps):
            for loop in LOOPS:
                for name, tree in cases:
                    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--seq", seq, "--case", name, "--loop", loop]
                    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                    if out.returncode != 0:  # a run that failed ends the measurement: nothing is started behind it
                        raise SystemExit("run %d of case %s, loop %s failed (%d): %s" % (rep, name, loop, out.returncode, out.stderr[-2000:]))
                    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
                    print(line, flush=True)
                    d = json.loads(line)
                    res[(loop, name)].append(d["frames_per_s"])
                    first[(loop, name)].append(d["first_frame_ms"])
                    entered[(loop, name)].append(d["entered_per_frame"])
    summary = dict(landmarks=256, frames=a.frames, reps=a.reps)
    overlap = lambda x, y: min(x) <= max(y) and min(y) <= max(x)
    us = lambda loop, on, off: round(1e6 * (1 / np.median(res[(loop, on)]) - 1 / np.median(res[(loop, off)])), 2)
    for loop in LOOPS:
        s = {}
        for name, _ in cases:
            v = res[(loop, name)]
            s[name] = dict(median=float(np.median(v)), min=min(v), max=max(v), runs=v, first_frame_ms_median=float(np.median(first[(loop, name)])),
                           entered_per_frame=float(np.median(entered[(loop, name)])))
        if a.parent_tree:
            s["off_vs_parent_ranges_overlap"] = bool(overlap(res[(loop, "off")], res[(loop, "parent")]))
        s["us_per_frame_added_by_the_8x6_grid"] = us(loop, "8x6", "off")
        s["us_per_frame_added_by_the_1x1_grid"] = us(loop, "1x1", "off")
        summary[loop] = s
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
