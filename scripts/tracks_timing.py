"""Cost of the landmark identities (always on) and of the export of the tracks that ended (ekfvio_set_ended_export) in the image loop.

Frames/s of ekfvio_step_image on the 640 x 480 translated sequence at N = 256 (replenish = 1: the loop a node runs), `reps` runs per case,
alternating.  Every run is a process of its own (one handle, the same frames), started one after the other.  Cases:

    keep            this build, remove_lost = 0
    remove          this build, remove_lost = 1
    remove_ended    this build, remove_lost = 1, the export on; every frame also reads its ids and its ended records, as a consumer would
    parent_keep     (`--parent-tree`: a checkout of the parent commit with its library built there) remove_lost = 0
    parent_remove   ... remove_lost = 1

The ids ride in three kernels that exist anyway (add_features_kernel, remove_features_kernel, frame_outputs_kernel): the yardstick for them
is the parent's own run-to-run range, case by case.  The export's cost is one more launch per removing frame.

The durations of the kernels come from a kernel trace of one run per case (the trace tool in front, this program behind `--`):
    <trace tool> --kernel-trace --stats -d <dir> -- python scripts/tracks_timing.py --child --remove-lost 1 --ended
and the rows of remove_features_kernel, frame_outputs_kernel, add_features_kernel and ended_tracks_kernel in its kernel statistics; the
same trace of the parent's build lists the kernels, grids and counts there.  Tracing slows the host, so frames/s are taken without it.

Usage: python scripts/tracks_timing.py [--frames 400] [--reps 9] [--parent-tree DIR]
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
    """One run: a fresh handle of the build in a.tree, WARM frames untimed, the rest in four chunks; the rate is the median chunk's.  As in a
    node, every frame's outputs are read: odometry and cloud always, the ids and the ended records too where the export is on."""
    seq = np.load(a.seq) if a.seq else sequence(a.tree, WARM + a.frames)
    sys.path.insert(0, a.tree)
    from ekf_vio_amd import EKFVIO
    extra = {"ended_export": True} if a.ended else {}  # (a build without the feature is never asked for it)
    v = EKFVIO(max_features=256, replenish=1, remove_lost=a.remove_lost, fast_threshold=20, min_new_feature_dist=12, **extra)
    ended = 0

    def frame(f):
        nonlocal ended
        v.addFrame(f / 30.0, seq[f], K)
        v.odometry()
        v.points()
        if a.ended:
            v.landmark_ids()
            ended += v.ended()["count"]

    for i in range(WARM):  # first frame, replenishment, steady state
        frame(i)
    v.tc_ekf.synchronize()
    per, f, rates = (len(seq) - WARM) // 4, WARM, []
    for _ in range(4):
        t0 = time.perf_counter()
        for _ in range(per):
            frame(f)
            f += 1
        v.tc_ekf.synchronize()
        rates.append(per / (time.perf_counter() - t0))
    out = dict(case=a.case, remove_lost=a.remove_lost, ended_export=bool(a.ended), frames=4 * per, frames_per_s=round(float(np.median(rates)), 1),
               landmarks=v.tc_ekf.num_features, ended_records=ended, early_output_frames=v.tc_ekf.counters()["early_output_frames"])
    v.tc_ekf.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its loops as two more cases")
    ap.add_argument("--child", action="store_true", help="one run in this process (what the driver starts; also the program to trace)")
    ap.add_argument("--remove-lost", type=int, default=0, help="(child) cfg.remove_lost")
    ap.add_argument("--ended", action="store_true", help="(child) with the export of the tracks that ended on, read every frame")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--seq", default=None)
    ap.add_argument("--case", default="run")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.reps < 1 or a.frames < 8:
        raise SystemExit("at least one run of at least 8 frames")
    cases = [("keep", HERE, 0, False), ("remove", HERE, 1, False), ("remove_ended", HERE, 1, True)]
    if a.parent_tree:
        parent = os.path.abspath(a.parent_tree)
        cases = [("parent_keep", parent, 0, False), ("parent_remove", parent, 1, False)] + cases
    res = {c[0]: [] for c in cases}
    with tempfile.TemporaryDirectory() as tmp:
        seq = os.path.join(tmp, "seq.npy")
        np.save(seq, sequence(HERE, WARM + a.frames))  # the same frames for every run of every case
        for rep in range(a.reps):
            for name, tree, remove_lost, ended in cases:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--seq", seq, "--case", name, "--remove-lost", str(remove_lost)]
                cmd += ["--ended"] if ended else []
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                if out.returncode != 0:  # a run that failed ends the measurement: nothing is started behind it
                    raise SystemExit("run %d of case %s failed (%d): %s" % (rep, name, out.returncode, out.stderr[-2000:]))
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
                print(line, flush=True)
                res[name].append(json.loads(line)["frames_per_s"])
    summary = dict(landmarks=256, frames=a.frames, reps=a.reps)
    for name, v in res.items():
        summary[name] = dict(median=float(np.median(v)), min=min(v), max=max(v), runs=v)
    overlap = lambda x, y: min(x) <= max(y) and min(y) <= max(x)
    if a.parent_tree:
        summary["keep_vs_parent_ranges_overlap"] = bool(overlap(res["keep"], res["parent_keep"]))
        summary["remove_vs_parent_ranges_overlap"] = bool(overlap(res["remove"], res["parent_remove"]))
    summary["us_per_frame_added_by_the_export"] = round(1e6 * (1 / np.median(res["remove_ended"]) - 1 / np.median(res["remove"])), 2)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
