"""Cost of the innovation gate (ekfvio_set_gate) in a device-resident run.

Steps/s of ekfvio_run_uploaded at N landmarks with the gate off and with chi2 = FLT_MAX (every landmark evaluated, none
rejected: the same update behind another launch sequence -- gate + bookkeeping as a launch of their own behind process(dt)
instead of a workgroup inside it), alternating, `reps` timed runs each on one handle.  The duration of the gate + bookkeeping
launch itself comes from a kernel trace of this script (the trace tool in front, this program behind `--`): the rows
gate_bookkeeping_kernel of its kernel statistics.

Every timed run covers the same frames from the same state, inside the valid part of the synthetic sequence (bench.py,
VALID_FRAMES: the camera reaches its landmarks near frame 580).

Usage: python scripts/gate_timing.py [--landmarks 256] [--steps 384] [--warmup 64] [--reps 9]; prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ekf_vio_amd import TightlyCoupledEKF  # noqa: E402
from ekf_vio_amd.sim import Scenario  # noqa: E402

FLT_MAX = float(np.finfo(np.float32).max)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--landmarks", type=int, default=256)
    ap.add_argument("--steps", type=int, default=384)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    if a.warmup + a.steps > 448:
        raise SystemExit("warmup + steps must stay inside the sequence's 448 valid frames")
    N = a.landmarks
    sc = Scenario(N, seed=0)
    fr = list(sc.frames(a.warmup + a.steps))
    z, R, p = (np.stack([f[i] for f in fr]) for i in range(3))
    g = TightlyCoupledEKF(max_features=N)
    g.addNewFeatures(sc.initial_features())
    g.upload_measurements(z, R, p)
    g.run_uploaded(0, a.warmup, sc.dt)
    g.synchronize()
    start = g.get_state()
    rates = {"off": [], "flt_max": []}
    for rep in range(a.reps):
        for name, chi2 in (("off", 0.0), ("flt_max", FLT_MAX)):
            g.set_state(start)
            g.setGate(chi2)
            g.run_uploaded(a.warmup, 0, sc.dt)   # captures the launch graphs (nothing runs)
            g.run_uploaded(a.warmup, 32, sc.dt)  # ... and runs them once untimed
            g.synchronize()
            g.set_state(start)
            t0 = time.perf_counter()
            g.run_uploaded(a.warmup, a.steps, sc.dt)
            g.synchronize()
            rates[name].append(a.steps / (time.perf_counter() - t0))
    gate = g.gate()
    g.close()
    if gate["gated_total"]:
        raise SystemExit("the gate at FLT_MAX rejected %d measurements: the two runs did not do the same work" % gate["gated_total"])
    off, on = np.array(rates["off"]), np.array(rates["flt_max"])
    print(json.dumps(dict(landmarks=N, steps=a.steps, reps=a.reps, steps_per_s_gate_off=[round(x, 1) for x in off],
                          steps_per_s_gate_flt_max=[round(x, 1) for x in on], median_off=round(float(np.median(off)), 1),
                          median_flt_max=round(float(np.median(on)), 1),
                          us_per_step_added=round(1e6 * (1 / np.median(on) - 1 / np.median(off)), 3),
                          gated_total=gate["gated_total"])))


if __name__ == "__main__":
    main()
