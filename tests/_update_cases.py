"""Shared case definitions of tests/test_gpu_update_matrix.py and tests/test_update_matrix_cpu.py (a plain module, imported like _scatter.py).

One measurement update per case, teacher-forced: the start state is the fp32 oracle's behind WARM_FRAMES teacher-forced frames of
Scenario(N, seed, dt=0.05) -- a dense covariance -- propagated by process(dt); from that one fp32 state the update is evaluated with the
same z, R, passed by the HIP kernels, the fp32 oracle and the fp64 oracle.  Everything here runs on the CPU: the oracles, the inputs
and the tolerances.  Nothing in this file looks at what the HIP kernels return.

A case is (N, capacity, measured, layout, sizing, R kind):
  * measured: how many of the N landmarks the tracker passes; the flow an update takes depends on it (FLOWS below);
  * layout: WHICH landmarks fail -- "head" (the first N-k), "tail" (the last N-k), "every" (spread evenly), "run" (one contiguous run
    that starts at landmark 40: state row 22 + 120 = 142, in the middle of the third 64-row block of Sigma);
  * sizing: "host" (ekfvio_update sizes the launches from the pass flags) or "device" (the gate at FLT_MAX: the plan is made for
    m = 2N, the kernels read the count on the device and the block columns past it are identity padding);
  * R kind: "a" the scenario's 1e-5 I; "b" diagonal, three decades across landmarks, u and v different; "c" full symmetric blocks,
    correlation +-0.6; "d" the non-symmetric blocks of the sample-based path with fx = 1.3 fy:
    [s0 c00, s0 c10, s1 c01, s1 c11] (column-major), s0 / s1 = 1 / 1.69.

z is the scenario's own exact projection for every kind (the innovation is the warmed filter's remaining error, 1e-4 .. 3e-4, consistent
across landmarks: every measured landmark's mean then moves towards its z in the fp64 evaluation, which moves_towards_z relies on).

WARM_FRAMES = 6 and the R magnitudes of kinds b-d (R_LO .. R_HI, R_CORR) were tuned on the CPU until both held: every defect in view moves
the fp64 result by ten tolerances, and in fp64 at most 5 % of a case's measured landmarks move away from their z.
tests/test_update_matrix_cpu.py measures and prints the ratios, SENSITIVITY below records them.  Tried and dropped:
  * 3 warm-up frames: the base state's common correction is still large and pushes landmarks with a large R AWAY from their own z in
    fp64 -- 16 % of the measured ones with R = 1e-5 .. 1e-2, 9 % with 1e-6 .. 1e-3 (where R^T is only 10.8 tolerances away at 255 of 256
    measured), 2 % with 1e-7 .. 1e-4 (R^T 3.8 tolerances);
  * 6 warm-up frames with R = 1e-5 .. 1e-2: R^T at least 54 tolerances away, but with correlated blocks 9 - 11 % of the measured
    landmarks still move away from z;
  * measurement noise of one standard deviation of R on z: half of the landmarks move away.
"""
import functools

import numpy as np

from ekf_vio_amd.sim import Scenario
from oracle import OracleFilter, max_threads, set_threads

import _scatter

BASE = 22
SEED = 0
DT = 0.05
WARM_FRAMES = 6
FLT_MAX = float(np.finfo(np.float32).max)
# the update's policy against the fp64 oracle: the constants of tests/test_gpu_parity.py, copied, not new ones
ACC_FACTOR = 4.0
MU_FLOOR = 2e-5
SIG_FLOOR = 2e-6
SYM_N = 334  # above it the update's last GEMM forms the lower triangle and mirrors it: the triangle form of the yardstick (test_gpu_gate.py)
MARGIN = 10.0  # a defect in view must move the fp64 answer by this many tolerances (test_update_matrix_cpu.py)

# R of kinds b-d: the diagonal runs over three decades, R_LO .. R_HI, log-uniform across the landmarks (the warmed Sigma's (u, v) blocks are
# ~ 1e-5); v's variance is 0.3 .. 3 x u's; |off-diagonal| = R_CORR sqrt(R00 R11), sign by landmark.
# SENSITIVITY, measured by test_update_matrix_cpu.py: the smallest "fp64 result moved by the defect / tolerance of the case" over the
# (N, measured) the kind is used with (N = 256: 32, 128, 255; N = 400: 64, 192, 288, 399), always reached in Sigma:
#   kind b: u/v variances swapped 124, neighbour's R 2010           kind c: off-diagonals zeroed 354, swapped 210, neighbour's 1320
#   kind d: R^T 28.7 (N = 400, 64 measured), off-diagonals zeroed 140, swapped 191, neighbour's 573
#   pass mask rotated by one landmark at the 65 / 160 / 161 counts of N = 256: head 23.4, tail 29.7, run 92.9, every 4110
#   (a single failure moved by one landmark: 10.8 at 255 of 256, 7.4 at 399 of 400 -- printed, not held to the margin)
# In the fp64 evaluation at most one measured landmark of a case was seen to move away from its z (asserted: at most 5 %).
R_LO, R_HI = 1e-6, 1e-3
R_CORR = 0.6
FX_OVER_FY = 1.3

LAYOUTS = ("head", "tail", "every", "run")
RUN_START = 40


def use_threads():
    """The oracle's OpenMP products on up to 16 cores (results do not depend on the thread count, tests/test_gpu_shapes.py)."""
    set_threads(min(max_threads(), 16))


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def warmed(N, seed=SEED):
    """(state before process(dt), the fp32 oracle's state behind process(dt), the next frame's (z, R, passed))."""
    use_threads()
    sc = Scenario(N, seed=seed, dt=DT)
    o = OracleFilter(np.float32)
    o.add_new_features(sc.initial_features())
    fr = list(sc.frames(WARM_FRAMES + 1))
    for z, R, p in fr[:WARM_FRAMES]:
        o.process(sc.dt)
        o.update(z, R, p)
    st0 = o.get_state()
    o.process(sc.dt)
    sp = o.get_state()
    o.close()
    S = sp["Sigma"]
    assert np.isfinite(S).all() and np.count_nonzero(S) > 0.9 * S.size, "the warmed covariance is not dense"
    return sc.dt, st0, sp, fr[WARM_FRAMES]


def pass_mask(N, k, layout):
    """k of N landmarks measured."""
    assert 0 < k <= N and layout in LAYOUTS
    p = np.ones(N, np.uint8)
    nf = N - k
    if nf == 0:
        return p
    if layout == "head":
        p[:nf] = 0
    elif layout == "tail":
        p[k:] = 0
    elif layout == "run":
        s = min(RUN_START, N - nf)
        p[s:s + nf] = 0
    else:  # nf failures spread evenly, none twice
        p[(np.arange(nf) * N) // nf] = 0
    assert int(p.sum()) == k
    return p


def make_R(kind, N, R_scenario):
    """R[N, 4], column-major quadruples (R00, R10, R01, R11), float32."""
    if kind == "a":
        return R_scenario.copy()
    rng = np.random.default_rng(1000 + ord(kind))
    c00 = 10.0 ** rng.uniform(np.log10(R_LO), np.log10(R_HI), N)
    c11 = c00 * 10.0 ** rng.uniform(np.log10(0.3), np.log10(3.0), N)
    R = np.zeros((N, 4))
    R[:, 0], R[:, 3] = c00, c11
    if kind in "cd":
        off = R_CORR * np.sqrt(c00 * c11) * np.where(rng.uniform(size=N) < 0.5, -1.0, 1.0)
        R[:, 1] = R[:, 2] = off
    if kind == "d":
        s0, s1 = 1.0 / FX_OVER_FY ** 2, 1.0
        R[:, 0] *= s0
        R[:, 1] *= s0
        R[:, 2] *= s1
        R[:, 3] *= s1
    R = R.astype(np.float32)
    for b in (R[:, 1], R[:, 2]):  # the gate's determinant stays positive whichever off-diagonal it reads
        assert np.all(R[:, 0].astype(np.float64) * R[:, 3] - b.astype(np.float64) ** 2 > 0)
    return R


def inputs(N, k, layout, kind, seed=SEED):
    """(dt, st0, sp, z, R, passed) of a case."""
    dt, st0, sp, (z, R, _) = warmed(N, seed)
    Rk = make_R(kind, N, R)
    return dt, st0, sp, z.copy(), Rk, pass_mask(N, k, layout)


MUTATIONS = ("transposed", "off_diagonal_zeroed", "diagonal_swapped", "next_landmarks")


def mutate_R(R, how):
    M = R.copy()
    if how == "transposed":
        M[:, 1], M[:, 2] = R[:, 2], R[:, 1]
    elif how == "off_diagonal_zeroed":
        M[:, 1] = M[:, 2] = 0
    elif how == "diagonal_swapped":
        M[:, 0], M[:, 3] = R[:, 3], R[:, 0]
    elif how == "next_landmarks":
        M = np.roll(R, -1, axis=0)
    else:
        raise ValueError(how)
    return M


# ---------------------------------------------------------------------------------------------------------------- references
def oracle_update(dtype, sp, z, R, p):
    o = OracleFilter(dtype)
    o.set_state(sp)
    info = o.update(z, R, p)
    st = o.get_state()
    o.close()
    return info, st


def _tri(n):
    lower = np.tril(np.ones((n, n), dtype=bool))
    return lower, ~lower


def scatter6(sp, z, R, p, s64, nperm=6, seed=0):
    """_scatter.fp32_scatter (same orderings, same numbers: asserted in test_update_matrix_cpu.py) plus the worst error on Sigma's lower
    triangle as an absolute Frobenius norm, which the N > SYM_N form of the yardstick needs."""
    N = sp["feat_mu"].shape[0]
    rng = np.random.default_rng(seed)
    S64 = s64["Sigma"].astype(np.float64)
    lower, _ = _tri(S64.shape[0])
    worst = dict(mu=0.0, feat=0.0, sig=0.0, sig_lower=0.0)
    for j in range(nperm):
        perm = np.arange(N) if j == 0 else rng.permutation(N)
        spp, idx = _scatter._perm_state(sp, perm)
        _, out = oracle_update(np.float32, spp, np.asarray(z)[perm], np.asarray(R)[perm], np.asarray(p)[perm])
        inv = np.empty_like(perm)
        inv[perm] = np.arange(N)
        iidx = np.empty_like(idx)
        iidx[idx] = np.arange(idx.shape[0])
        sig = out["Sigma"][np.ix_(iidx, iidx)].astype(np.float64)
        D = sig - S64
        worst["mu"] = max(worst["mu"], float(np.abs(out["base_mu"].astype(np.float64) - s64["base_mu"]).max()))
        worst["feat"] = max(worst["feat"], float(np.abs(out["feat_mu"][inv].astype(np.float64) - s64["feat_mu"]).max()))
        worst["sig"] = max(worst["sig"], float(np.linalg.norm(D) / np.linalg.norm(S64)))
        worst["sig_lower"] = max(worst["sig_lower"], float(np.linalg.norm(D[lower])))
    return worst


def make_reference(sp, z, R, p):
    """What an update from `sp` is held to: the fp32 oracle's return value and bookkeeping, the fp64 oracle's state, the fp32 scatter."""
    use_threads()
    info32, s32 = oracle_update(np.float32, sp, z, R, p)
    _, s64 = oracle_update(np.float64, sp, z, R, p)
    return dict(info32=info32, del_flag32=s32["del_flag"], last_klt32=s32["last_klt"], s64=s64, scatter=scatter6(sp, z, R, p, s64))


@functools.lru_cache(maxsize=None)
def reference(N, k, layout, kind, seed=SEED):
    """make_reference of a case; host- and device-sized twins and handles of another capacity share it."""
    dt, st0, sp, z, R, p = inputs(N, k, layout, kind, seed)
    return make_reference(sp, z, R, p)


def errors(got, s64):
    """How far a result is from the fp64 one, in the yardstick's three (N <= SYM_N) or four measures."""
    S, S64 = got["Sigma"].astype(np.float64), s64["Sigma"].astype(np.float64)
    n = S.shape[0]
    e = dict(mu=float(np.abs(got["base_mu"].astype(np.float64) - s64["base_mu"]).max()),
             feat=float(np.abs(got["feat_mu"].astype(np.float64) - s64["feat_mu"]).max()))
    if (n - BASE) // 3 <= SYM_N:
        e["sig"] = float(np.linalg.norm(S - S64) / np.linalg.norm(S64))
    else:
        lower, upper = _tri(n)
        e["sig_lower"] = float(np.linalg.norm((S - S64)[lower]))
        e["sig_upper"] = float(np.linalg.norm((S - S64)[upper]))
    return e


def tolerances(s64, scatter):
    """ACC_FACTOR x the fp32 reference's worst error over its six orderings + floor, in the measures of errors()."""
    S64 = s64["Sigma"].astype(np.float64)
    n = S64.shape[0]
    t = dict(mu=ACC_FACTOR * scatter["mu"] + MU_FLOOR, feat=ACC_FACTOR * scatter["feat"] + MU_FLOOR)
    if (n - BASE) // 3 <= SYM_N:
        t["sig"] = ACC_FACTOR * scatter["sig"] + SIG_FLOOR
    else:  # tests/test_gpu_gate.py, test_gpu_shapes.py::test_symmetric_second_joseph_gemm_is_the_full_one_mirrored
        lower, upper = _tri(n)
        nl, nu = float(np.linalg.norm(S64[lower])), float(np.linalg.norm(S64[upper]))
        t["sig_lower"] = ACC_FACTOR * scatter["sig_lower"] + SIG_FLOOR * nl
        t["sig_upper"] = float(np.linalg.norm((S64 - S64.T)[upper])) + ACC_FACTOR * scatter["sig_lower"] + SIG_FLOOR * nu
    return t


def moves_towards_z(sp, got, z, p):
    """Per measured landmark: |z - mu'| <= |z - mu| + MU_FLOOR in both coordinates."""
    before = np.abs(z.astype(np.float64) - sp["feat_mu"][:, :2])
    after = np.abs(z.astype(np.float64) - got["feat_mu"][:, :2])
    return np.all(after <= before + MU_FLOOR, axis=1) | ~np.asarray(p).astype(bool)


# ---------------------------------------------------------------------------------------------------------------- the flows
# What ran on an MI355X (256 compute units), recorded through the handle's counters and profiler classes -- not derived from the
# product's formulae.  (N, capacity, sizing, first count, last count) -> (sweep, gain, tail):
#   sweep "persist": the counter `persistent` went up by one (the fused persistent launch); "step" / "split": it did not (one launch
#         per block step; from 16 block columns on the split look-ahead sweep -- the counters do not tell these two apart, the table
#         records which one the shape takes by EKF_SWEEP_SPLIT_MB);
#   gain  "sweep": the profiler's `solve` class saw no launch (the gain came out of the sweep's launch); "launch": it saw one;
#   tail  "t2": `t2_updates` went up and `gemm_update` saw ONE launch; "joseph": it did not and `gemm_update` saw two.
FLOWS = [
    (256, 256, "host", 1, 64, ("step", "launch", "joseph")),
    (256, 256, "host", 65, 160, ("persist", "sweep", "joseph")),
    (256, 256, "host", 161, 256, ("persist", "sweep", "t2")),
    (256, 256, "device", 1, 256, ("persist", "sweep", "t2")),
    (256, 320, "host", 1, 64, ("step", "launch", "joseph")),
    (256, 320, "host", 65, 160, ("persist", "sweep", "joseph")),
    (256, 320, "host", 161, 224, ("persist", "sweep", "t2")),
    (256, 320, "host", 225, 256, ("persist", "launch", "joseph")),  # (the capacity's row blocks no longer fit beside the sweep)
    (100, 100, "host", 1, 64, ("step", "launch", "joseph")),
    (100, 100, "host", 65, 96, ("persist", "sweep", "joseph")),
    (100, 100, "host", 97, 100, ("persist", "sweep", "t2")),
    (100, 100, "device", 1, 100, ("persist", "sweep", "t2")),
    (400, 400, "host", 1, 64, ("step", "launch", "joseph")),
    (400, 400, "host", 65, 192, ("persist", "sweep", "joseph")),
    (400, 400, "host", 193, 288, ("persist", "launch", "joseph")),
    (400, 400, "host", 289, 400, ("step", "launch", "joseph")),
    (400, 400, "device", 1, 400, ("step", "launch", "joseph")),
    (600, 600, "host", 1, 480, ("step", "launch", "joseph")),
    (600, 600, "host", 481, 600, ("split", "launch", "joseph")),
]
SIGNATURE = {  # flow -> (persistent, solve launches, gemm_update launches, t2_updates), the deltas of one update
    ("step", "launch", "joseph"): (0, 1, 2, 0),
    ("split", "launch", "joseph"): (0, 1, 2, 0),
    ("persist", "sweep", "joseph"): (1, 0, 2, 0),
    ("persist", "launch", "joseph"): (1, 1, 2, 0),
    ("persist", "sweep", "t2"): (1, 0, 1, 1),
}


def expected_flow(N, cap, sizing, k):
    rows = [f for (n, c, s, lo, hi, f) in FLOWS if (n, c, s) == (N, cap, sizing) and lo <= k <= hi]
    assert len(rows) == 1, (N, cap, sizing, k)
    return rows[0]


# ---------------------------------------------------------------------------------------------------------------- the cases
def _cases():
    out = []

    def add(N, k, layout="every", sizing="host", kind="a", cap=None):
        out.append((N, cap or N, k, layout, sizing, kind))

    # shape: every regime at both edges of every boundary (33: m = 66, the second block column two rows deep)
    for k in (1, 32, 33, 64, 128, 255):
        add(256, k)
    for k in (65, 160, 161):
        for layout in LAYOUTS:
            add(256, k, layout)
    for k in (1, 64, 65, 96, 97):
        add(100, k)
    for k in (64, 65, 192, 193, 288, 289, 399):
        add(400, k)
    for k in (480, 481):
        add(600, k)
    for k in (64, 128, 192, 224, 225, 255):  # a capacity above N: ldp enters the plan and the Wt tiling separately from n
        add(256, k, cap=320)
    # device-sized: the plan is made for m = 2N, most block columns are identity padding
    for k in (1, 30, 65, 161, 255):
        add(256, k, sizing="device")
    add(100, 10, sizing="device")
    for k in (50, 250):
        add(400, k, sizing="device")
    # R: one count per regime, host- and device-sized
    for N, counts in ((256, (32, 128, 255)), (400, (64, 192, 288, 399))):
        for k in counts:
            for kind in "bcd":
                for sizing in ("host", "device"):
                    add(N, k, sizing=sizing, kind=kind)
    add(600, 481, kind="d")
    return out


CASES = _cases()


def case_id(c):
    N, cap, k, layout, sizing, kind = c
    return "N%d%s-k%d-%s-%s-R%s" % (N, "" if cap == N else "cap%d" % cap, k, layout, sizing, kind)
