"""Cost of the IMU extrinsics (ekfvio_set_imu_extrinsics) in the IMU update.

Microseconds per ekfvio_imu_update at N = 256 (n = 790): `updates` calls enqueued back to back and one synchronize per run, `reps` runs per
case, alternating, every run a process of its own (one handle), started one after the other:
    parent   the same loop on ANOTHER build of this repository (`--parent-tree`: a checkout of the parent commit with its library built there):
             whether the template, with the setting off, costs anything against the kernel before it
    off      this build, the setting off: imu_gain_kernel<false>
    on       this build, a generic rotation and a lever arm set: imu_gain_kernel<true>

The two kernels' durations and the launch lists come from a kernel trace of one run per case (the trace tool in front, this program behind
`--`; no counters in the same run):
    <trace tool> --kernel-trace --stats -d <dir> -- python scripts/imu_extrinsics_timing.py --child --case on
With the setting off the trace lists the parent's kernels, grids and counts.  Tracing slows the host, so the times per update are taken
without it.

Usage: python scripts/imu_extrinsics_timing.py [--updates 2000] [--reps 9] [--parent-tree DIR]
prints one JSON line per run and a last line with medians, ranges and the time the setting adds per update.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 256
WARM = 50
CASES = ("parent", "off", "on")
# a signed permutation (IMU x forward, z up -> optical z forward, y down) times 10 degrees about (1, 2, -1); 11 cm of lever arm
P_CI = (0.05, -0.02, 0.11)


def rotation():
    a = np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(10.0)
    return np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]) @ (np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K))


def child(a):
    """One run: a fresh handle of the build in a.tree, five camera frames to fill the covariance, WARM updates untimed, then a.updates."""
    sys.path.insert(0, a.tree)
    from ekf_vio_amd import TightlyCoupledEKF
    from ekf_vio_amd.sim import Scenario
    sc = Scenario(N, seed=7, dt=0.05)
    h = TightlyCoupledEKF(max_features=N, use_imu=1)
    h.addNewFeatures(sc.initial_features())
    for z, R, p in sc.frames(5):
        h.process(sc.dt)
        h.updateWithFeaturePositions(z, R, p)
    if a.case == "on":  # (a build without the setting is never asked for it)
        h.setImuExtrinsics(rotation(), P_CI)
    gyro, acc = np.array([0.01, 0.11, -0.02], np.float32), np.array([0.05, -9.78, 0.1], np.float32)
    if a.case == "on":
        gyro, acc = (rotation().T @ gyro).astype(np.float32), (rotation().T @ acc).astype(np.float32)
    for _ in range(WARM):
        h.imuUpdate(gyro, acc)
    h.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.updates):
        h.imuUpdate(gyro, acc)
    h.synchronize()
    us = 1e6 * (time.perf_counter() - t0) / a.updates
    st = h.get_state()
    ok = bool(np.isfinite(st["Sigma"]).all() and np.isfinite(st["base_mu"]).all())
    h.close()
    print(json.dumps(dict(case=a.case, updates=a.updates, us_per_update=round(us, 3), finite=ok)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its loop as a further case")
    ap.add_argument("--child", action="store_true", help="one run in this process (what the driver starts; also the program to trace)")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--case", default="off", choices=CASES)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.reps < 1 or a.updates < 1:
        raise SystemExit("at least one run of at least one update")
    cases = [("off", HERE), ("on", HERE)]
    if a.parent_tree:
        cases.insert(0, ("parent", os.path.abspath(a.parent_tree)))
    res = {name: [] for name, _ in cases}
    for rep in range(a.reps):
        for name, tree in cases:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--case", name, "--updates", str(a.updates)]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:  # a run that failed ends the measurement: nothing is started behind it
                raise SystemExit("run %d of case %s failed (%d): %s" % (rep, name, out.returncode, out.stderr[-2000:]))
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            res[name].append(json.loads(line)["us_per_update"])
    summary = dict(landmarks=N, updates=a.updates, reps=a.reps)
    for name, v in res.items():
        summary[name] = dict(median=float(np.median(v)), min=min(v), max=max(v), runs=v)
    if a.parent_tree:
        summary["off_vs_parent_ranges_overlap"] = bool(min(res["off"]) <= max(res["parent"]) and min(res["parent"]) <= max(res["off"]))
    summary["us_per_update_added_on_vs_off"] = round(float(np.median(res["on"]) - np.median(res["off"])), 3)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
