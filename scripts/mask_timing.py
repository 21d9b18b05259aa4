"""Cost of the no-data mask (ekfvio_set_mask) in the image loop.

Frames/s of ekfvio_step_image on the 640 x 480 translated sequence at N = 256 (replenish = 1: the loop a node runs), `reps` runs per case,
alternating, every run a process of its own (one handle, the same frames), started one after the other:
    parent     the same loop on ANOTHER build of this repository (`--parent-tree`: a checkout of the parent commit with its library built
               there): whether the mask, switched off, costs anything against the code before it
    off        this build, the mask off
    ones       this build with an all-ones caller's mask: the blocked map is the kill box's complement, every output keeps its bits, and the
               detector and the tracker do the mask's work (the copy of B into the occupancy image, one word per landmark)
    rectified  this build, frames rectified with pincushion coefficients (`--distortion`), no mask: the base line of the next case
    border     ... and EKFVIO_MASK_RECTIFY_BORDER on top: landmarks stay off the black border

The durations of klt_track_kernel, replenish_select_kernel and of the two one-off kernels (mask_nodata_kernel, mask_dilate_kernel) come
from a kernel trace of one run per case (the trace tool in front, this program behind `--`; no counters in the same run):
    <trace tool> --kernel-trace --stats -d <dir> -- python scripts/mask_timing.py --child --case border
Tracing slows the host, so frames/s are taken without it.

Usage: python scripts/mask_timing.py [--frames 400] [--reps 9] [--distortion k1 k2 p1 p2 k3] [--parent-tree DIR]
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
CASES = ("parent", "off", "ones", "rectified", "border")


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
    extra = {}  # (a build without the mask is never asked for it)
    if a.case in ("rectified", "border"):
        extra["distortion"] = a.distortion
    if a.case == "border":
        extra["mask_rectify_border"] = True
    if a.case == "ones":
        extra["mask"] = np.full(seq[0].shape, 255, np.uint8)
    v = EKFVIO(max_features=256, replenish=1, fast_threshold=20, min_new_feature_dist=12, **extra)
    for i in range(WARM):  # first frame (with the mask on: its blocked map), replenishment, steady state
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
    if a.case in ("ones", "border"):
        out["blocked_pixels"] = int(v.tc_ekf.mask_blocked().sum())
    v.tc_ekf.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--distortion", type=float, nargs=5, default=[0.15, -0.05, 0.0, 0.0, 0.0], metavar=("K1", "K2", "P1", "P2", "K3"))
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its loop as a further case")
    ap.add_argument("--child", action="store_true", help="one run in this process (what the driver starts; also the program to trace)")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--seq", default=None)
    ap.add_argument("--case", default="off", choices=CASES)
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
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--seq", seq, "--case", name, "--distortion"] + [repr(d) for d in a.distortion]
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
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
    us = lambda on, off: round(1e6 * (1 / np.median(res[on]) - 1 / np.median(res[off])), 2)
    summary["us_per_frame_added_by_an_all_ones_mask"] = us("ones", "off")
    summary["us_per_frame_added_by_the_border_mask"] = us("border", "rectified")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
