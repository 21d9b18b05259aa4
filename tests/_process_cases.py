"""Shared case definitions of tests/test_gpu_process_matrix.py and tests/test_process_cases_cpu.py (a plain module, imported like
_imu_cases.py): process(dt) -- predict_fused_kernel<LIN>, linearize_kernel, the dense two-GEMM path and the linearisation that rides in the
update's last GEMM (ekf_vio_amd/csrc/ekf_kernels.hip, motion_model.inc) -- in every launch form, at the sizes where its workgroups are
ragged, from states away from the identity attitude, and with a covariance whose entries sit around the flush threshold.

One teacher-forced process(dt) per case, from ONE fp32 state loaded with set_state.  Everything here runs on the CPU; nothing in this file
looks at what the HIP kernels return.

The start state.  Scenario(N, seed=0, dt=0.05) warmed in the fp32 oracle by process + update (5 frames up to N = 100, 3 above; N = 0: the
initial state after one process(0.05)) and NOT symmetrised: max |S - S^T| is 7e-4 at N = 20 and 0.09 at N = 513, so a transposed read of
Sigma changes bits.  The base state is then overwritten with the rotated, moving state of
test_process_follows_the_sse2_eigen_build_on_a_rotated_state (tests/test_gpu_parity.py) unless the case names another: at q = identity
most products of the quaternion multiplication are exact zeros.  The state need not be physically consistent for one teacher-forced step.

Families (CASES):
  * "size"  (rotated state, dt = 0.05): N = 0 .. 5 (all residues mod PREDICT_PC = 3, empty and single chunks), 7, 8, 9 (LIN_LM = 8),
    15, 16, 17, 31, 32, 33 (PREDICT_PT = 16: one and two tiles per side), 14 (n = 64), 35 (n + 1 = 128: ld == n + 1 on its own handle),
    50, 257, each in both structured forms -- "inside" (predict_fused_kernel<true>, the default) and "front" (EKFVIO_FUSE_LINEARIZE=0:
    linearize_kernel, then predict_fused_kernel<false>) -- and 512, 513 in the form the planner chooses (ts * ts <= 4 * num_cus: on 256
    compute units 512 linearises inside and 513 in front).  Three handles whose capacity exceeds N (17 in 100, 50 in 64, 257 in 320): a
    camera process + update runs before the case's set_state, so that P2 / Fdense / FA / FB / FD and column n hold leftovers and ld > n + 1;
    the case is then TWO consecutive process(dt) calls, P -> P2 -> P.
  * "state" (N = 20: N % 3 == 2 and a ragged tile; both forms; dt in 0, 1e-4, 0.05, 1): the initial base state; the rotated state; the
    quaternions 1.03 u and -u of tests/_imu_cases.py; omega exactly 0 with a velocity (delta_quat's small-angle branch in the unperturbed and
    the velocity columns); omega = (1e-11, 0, 0), below the 1e-10 switch; omega = (3.1415, 0.5, -0.2); landmarks at (1.4, -1.1, rho = 1e-3),
    (-1.5, 1.2, rho = 5) and rho = -0.5.
  * "flush" (N = 20, rotated, dt = 0.05; both forms and the dense one): Sigma scaled exactly by 2^-FLUSH_EXP, so that each of the four
    predict_finish sites (base block, base rows, base columns, landmark tiles) and add_noise_flush_kernel both prunes and keeps.
  * "dense" (predict_mode = PREDICT_DENSE): N = 2, 14, 20, 35, 50 in 64 behind a camera step, 257, 513; dt in 0, 0.05, 1.

Criteria.
  Structured forms: base_mu, feat_mu and all of Sigma equal the fp32 oracle's process(dt) in every bit (mismatch() names the count, the first
  element and the launch region -- base block, base-row chunk c, base-column chunk c, tile (tI, tJ)).
  Dense form: the means equal the oracle's bits (the same linearize_kernel).  For Sigma the fp64 ORACLE is no yardstick -- its finite
  differences differ from fp32's by 1e-4 relative -- so the reference is E = prune(F P F^T + Q) evaluated in fp64 with F the fp32 oracle's
  linearize(dt), mag = |F| |P| |F|^T + Q, and every element is held to
        |got - E| <= 2 (22 + 4) * 6e-8 * mag + 1e-13
  which is the suite's own GEMM bound (tests/test_gpu_parity.py: (K + 4) u sum|a||b|) for two chained products whose chains hold at most
  22 non-zero terms (zero products add exactly); the floor is one flush threshold, for an entry that one side prunes and the other keeps.
  The bound is derived, not measured.  Every entry must also be 0 or above the threshold in magnitude.

WHAT THE CASES CAN SEE, measured on the CPU by tests/test_process_cases_cpu.py (run with -s): each defect of DEFECTS put into
structured_fp64, the numpy fp64 evaluation of the structured product.  "bits": the distinct inputs of the families size / state / flush it
applies to (applies()), in ALL of which it changes at least one bit of the fp32-rounded result; "dense": the smallest, over the 22 dense
cases it applies to, of the largest |E_defect - E| / bound, held to MARGIN = 10.
    defect                         bits (inputs)  smallest dense ratio
    P read transposed              57 of 57       3.47 (N = 2, dt = 1: BELOW_MARGIN, see there), then 38 (flush case); 22 cases
    B of landmark f from f + 1     47 of 47       2.6e3 (flush case); 15 cases (dt > 0: at dt = 0 B is exactly zero)
    D transposed                   48 of 48       3.8e3 (flush case); 15 cases (dt > 0: at dt = 0 D is diagonal up to rounding)
    noise boundary shifted         49 of 49       1.6e5 (N = 2, dt = 0.05); 15 cases (dt > 0: Q(0) = 0)
    ragged chunk's last landmark   43 of 43       1.0e3 (flush case); 13 cases (N % 3 != 0, dt > 0)
    means from the new base state  60 of 60       --    (the means are held to bits in the dense form too: its cases are counted under
                                                         "bits"; dt > 0, N >= 1 and a base state that moves)
    flush left out                 the flush case: 143 entries below the threshold survive.  It moves E by less than one threshold, which the
                                   floor allows; the "0 or above the threshold" assertion of the dense test sees it, and the bits do.
The flush case (Sigma * 2^-28), entries the fp32 oracle prunes / keeps per region: base block 48 / 214 (of 484, 222 structurally zero), base
rows 41 / 919 and base columns 40 / 920 (of 1320, 360 structurally zero), landmark block 14 / 3586 (of 3600).
The fp32 oracle itself uses at most 8.02 of the 52 units of the dense bound (N = 513, dt = 0.05; 7.53 at dt = 1) and prunes exactly the
entries E prunes, in every case.

MEASURED ON THE MI355X (tests/test_gpu_process_matrix.py; 256 compute units: the planner linearises inside the propagation kernel at every
N up to 512 and in front of it at 513).  All 112 structured cases gave the fp32 oracle's bits in the means and in every element of Sigma, as
did numericallyLinearizeProcess at N = 7, 8, 9, 33 and the riding form at N = 103, 104, 105, 112, 113 against the per-call path; no change
to the kernels was needed.  The dense form's worst |got - E| / (6e-8 mag) per family, of 52 allowed, the fp32 oracle's figure in the same case
in brackets:
    dense   7.12 (8.02)   N = 513, dt = 0.05    [per N, worst over dt: 2: 3.4, 14: 5.0, 20: 4.9, 35: 4.5, 50 in 64: 4.8, 257: 6.9, 513: 7.1]
    flush   0.75 (0.75)   N = 20, dt = 0.05
and no entry below the flush threshold survived in any case.
"""
import collections
import ctypes as C
import functools

import numpy as np

from ekf_vio_amd.sim import Scenario
from oracle import OracleFilter, max_threads, set_threads

BASE = 22
SEED = 0
DT = float(np.float32(0.05))
PT, PCH, LIN_LM = 16, 3, 8   # PREDICT_PT, PREDICT_PC, LIN_LM of ekf_vio_amd/csrc/plan.h
CUS_MI355X = 256
FLUSH = float(np.float32(1e-8) * np.float32(1e-5))  # EKF_FLUSH_THRESH (common.h), the oracle's flush_thresh()
FLUSH_EXP = 28                # the flush family scales Sigma by 2^-28
UNIT = 6e-8                   # the suite's fp32 unit (tests/test_gpu_parity.py)
DENSE_UNITS = 2 * (22 + 4)    # two chained products of at most 22 non-zero terms each
DENSE_FLOOR = 1e-13           # one flush threshold
MARGIN = 10.0
DTS = (0.0, 1e-4, 0.05, 1.0)
DENSE_DTS = (0.0, 0.05, 1.0)

_Q = np.array([0.61, -0.37, 0.52, 0.47])
_U = np.array([0.6, -0.5, 0.4, 0.48])   # u of tests/_imu_cases.py
ROTATED = dict(pos=(0.3, -1.2, 0.7), quat=tuple(_Q / np.linalg.norm(_Q)), vel=(0.4, -0.3, 0.9), omega=(0.31, -0.23, 0.52),
               accel=(0.8, 0.1, -0.6))
STATES = ("initial", "rotated", "1.03u", "-u", "omega0", "omega1e-11", "omega-pi", "landmarks")
SIZE_NS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 14, 15, 16, 17, 31, 32, 33, 35, 50, 257)
PLANNER_NS = (512, 513)
CAPACITY = ((17, 100), (50, 64), (257, 320))
DENSE_NS = ((2, 2), (14, 14), (20, 20), (35, 35), (50, 64), (257, 257), (513, 513))
STATE_N = 20
LINEARIZE_NS = (7, 8, 9, 33)
RIDING_CANDIDATES = (103, 104, 105, 112, 113)
RIDING_RANGE = (97, 120)

# family, landmarks, capacity of the handle, base / landmark state, dt, launch form ("inside" | "front" | "default" | "dense"),
# a camera step before set_state, consecutive process(dt) calls, Sigma scaled by 2^-scale_exp
Case = collections.namedtuple("Case", "family N cap state dt form camera_first steps scale_exp")


def _cases():
    out = []
    for N in SIZE_NS:
        for form in ("inside", "front"):
            out.append(Case("size", N, N, "rotated", DT, form, False, 1, 0))
    for N in PLANNER_NS:
        out.append(Case("size", N, N, "rotated", DT, "default", False, 1, 0))
    for N, cap in CAPACITY:
        for form in ("inside", "front"):
            out.append(Case("size", N, cap, "rotated", DT, form, True, 2, 0))
    for s in STATES:
        for dt in DTS:
            for form in ("inside", "front"):
                out.append(Case("state", STATE_N, STATE_N, s, float(np.float32(dt)), form, False, 1, 0))
    for form in ("inside", "front", "dense"):
        out.append(Case("flush", STATE_N, STATE_N, "rotated", DT, form, False, 1, FLUSH_EXP))
    for N, cap in DENSE_NS:
        for dt in DENSE_DTS:
            out.append(Case("dense", N, cap, "rotated", float(np.float32(dt)), "dense", cap > N, 1, 0))
    return out


CASES = _cases()
STRUCTURED = [c for c in CASES if c.form != "dense"]
DENSE = [c for c in CASES if c.form == "dense"]


def case_id(c):
    s = "%s-N%d%s-%s-dt%g-%s" % (c.family, c.N, "" if c.cap == c.N else "cap%d" % c.cap, c.state, c.dt, c.form)
    return s + ("-x%d" % c.steps if c.steps > 1 else "")


def handle_capacity(c):
    """max_features of the case's handle (a handle cannot be created for no landmark at all)."""
    return max(c.cap, 1)


def ld_of(cap):
    """The leading dimension of a handle of that capacity (plan.h, filter_dims: n_cap + 1 rounded up to 64)."""
    return (BASE + 3 * max(cap, 1) + 1 + 63) // 64 * 64


_THREADS = min(max_threads(), 16)  # asked at import: another module's teardown leaves the oracle at one thread, which max_threads() then reports


def use_threads():
    set_threads(_THREADS)


def predict_plan(N, cus=CUS_MI355X, dense=False):
    """plan_predict through ekfvio_test_predict_plan (hooks build; no device, no handle): the switches come from the environment."""
    from ekf_vio_amd import capi
    out = (C.c_int32 * 8)()
    assert capi.load(hooks=True).ekfvio_test_predict_plan(int(cus), int(N), int(dense), 0, 0, out) == capi.OK
    return dict(zip(("dense", "pre", "lin_inside", "lin_in_front", "ts", "chunks", "book_rides", "grid"), out))


def form_name(p):
    return "dense" if p["dense"] else "inside" if p["lin_inside"] else "front" if p["lin_in_front"] else "pre"


# ---------------------------------------------------------------------------------------------------------------- inputs
def fresh(st):
    return {k: v.copy() for k, v in st.items()}


@functools.lru_cache(maxsize=None)
def start(N):
    """(the warmed fp32 state of N landmarks, as the fp32 oracle left it; the scenario's next frame (z, R, passed) for a camera update)."""
    use_threads()
    o = OracleFilter(np.float32)
    frame = None
    if N:
        sc = Scenario(N, seed=SEED, dt=DT)
        o.add_new_features(sc.initial_features())
        warm = 5 if N <= 100 else 3
        fr = list(sc.frames(warm + 1))
        for z, R, p in fr[:warm]:
            o.process(sc.dt)
            o.update(z, R, p)
        frame = tuple(a.copy() for a in fr[warm])
    else:
        o.process(DT)
    st = o.get_state()
    o.close()
    assert all(st[k].dtype == np.float32 for k in ("base_mu", "feat_mu", "Sigma")) and np.isfinite(st["Sigma"]).all()
    return st, frame


def apply_state(st, name):
    """The case's base (and landmark) state written over the warmed one; every number an fp32 one."""
    b = st["base_mu"]
    if name == "initial":
        b[:] = 0
        b[3] = 1
        return st
    b[0:3], b[3:7], b[7:10] = ROTATED["pos"], ROTATED["quat"], ROTATED["vel"]
    b[10:13], b[13:16] = ROTATED["omega"], ROTATED["accel"]
    if name == "1.03u":
        b[3:7] = 1.03 * _U / np.linalg.norm(_U)
    elif name == "-u":
        b[3:7] = -_U / np.linalg.norm(_U)
    elif name == "omega0":
        b[10:13] = 0
    elif name == "omega1e-11":
        b[10:13] = (1e-11, 0, 0)
    elif name == "omega-pi":
        b[10:13] = (3.1415, 0.5, -0.2)
    elif name == "landmarks":
        st["feat_mu"][0] = (1.4, -1.1, 1e-3)
        st["feat_mu"][1] = (-1.5, 1.2, 5.0)
        st["feat_mu"][2, 2] = -0.5
    else:
        assert name == "rotated", name
    return st


@functools.lru_cache(maxsize=None)
def _inputs(N, state, scale_exp):
    st = apply_state(fresh(start(N)[0]), state)
    if scale_exp:
        st["Sigma"] = st["Sigma"] * np.float32(2.0 ** -scale_exp)  # exact: a power of two, and nothing here is near the subnormals
    return st


def inputs(case):
    """The fp32 state the case loads with set_state; left unchanged by everything that reads it."""
    return _inputs(case.N, case.state, case.scale_exp)


def _oracle(dtype):
    return OracleFilter(dtype, emulate_static_cache=False)  # (a fresh oracle per case: the reference's stale dq_inv cache never shows)


@functools.lru_cache(maxsize=None)
def _reference(N, state, scale_exp, dt, steps):
    use_threads()
    st = _inputs(N, state, scale_exp)
    out = {}
    for dtype in (np.float32, np.float64):
        o = _oracle(dtype)
        o.set_state(st)
        if dtype == np.float32:
            out["F"] = o.linearize(np.float32(dt))
            out["q"] = o.process_noise_diag(np.float32(dt))
        states = []
        for _ in range(steps):
            o.process(dtype(np.float32(dt)))
            states.append(o.get_state())
        o.close()
        out[dtype] = states
    return out


def reference(case):
    """(the fp32 oracle's state after each of the case's process(dt) calls, the fp64 oracle's) -- shared, left unchanged."""
    r = _reference(case.N, case.state, case.scale_exp, case.dt, case.steps)
    return r[np.float32], r[np.float64]


def jacobian(case):
    """(the fp32 oracle's linearize(dt) on the case's start state, its process-noise diagonal)."""
    r = _reference(case.N, case.state, case.scale_exp, case.dt, case.steps)
    return r["F"], r["q"]


# ---------------------------------------------------------------------------------------------------------------- the product, in numpy
NOISE_BOUNDS = (7, 10, 16, 22)
DEFECTS = ("p_transposed", "b_from_next", "d_transposed", "noise_boundary_shifted", "ragged_last_unpropagated", "means_from_new_base",
           "flush_left_out")
SIGMA_DEFECTS = tuple(d for d in DEFECTS if d != "means_from_new_base")
# The one (defect, dense case) pair that stays below MARGIN, with the reason.  A transposed read moves E by F (P^T - P) F^T, so what the dense
# bound can see of it is the start covariance's own asymmetry.  After five frames at N = 2 that is 2.6e-5 of the largest entry (1.2e-4 at
# N = 14, 1.3e-3 at N = 513), and at dt = 1 the bound, which grows with |F| |P| |F|^T, is widest: the defect still FAILS the criterion there
# (3.5 bounds), but not by ten.  At N = 2 with dt = 0 and 0.05 it moves E by 1.4e3 and 59 bounds, and in the structured forms it changes bits.
BELOW_MARGIN = {("p_transposed", 2, 1.0): 1.0}


def noise_diag(n, dt, bounds=NOISE_BOUNDS):
    """generateProcessNoise restated: the diagonal of Q(dt) in fp32, the class boundaries a parameter."""
    dt = float(np.float32(dt))
    f = np.float32
    vals = (f(0.0001 * dt), f(0.01 * dt), f(5) * f(dt), f(0.001 * dt), f(0.0001 * dt))
    q = np.empty(n, np.float32)
    for i in range(n):
        k = sum(1 for b in bounds if i >= b)
        q[i] = vals[k]
    return q


def split_F(F, N):
    """A (22 x 22), B (N, 3, 9: columns 7 .. 15), D (N, 3, 3) of F = [[A 0], [B D]]; asserts that F is zero everywhere else."""
    F = np.asarray(F)
    n = BASE + 3 * N
    assert F.shape == (n, n)
    A = F[:BASE, :BASE]
    Fl = F[BASE:, :].reshape(N, 3, n)
    B = Fl[:, :, 7:16]
    idx = np.arange(N)
    D = Fl[:, :, BASE:].reshape(N, 3, N, 3)[idx, :, idx, :] if N else np.zeros((0, 3, 3), F.dtype)
    rest = F.copy()
    rest[:BASE, :BASE] = 0
    rest[BASE:, 7:16] = 0
    for f in range(N):
        rest[BASE + 3 * f:BASE + 3 * f + 3, BASE + 3 * f:BASE + 3 * f + 3] = 0
    assert not rest.any(), "F has entries outside A, B (columns 7 .. 15) and D"
    return A.copy(), B.copy(), D.copy()


def applies(defect, case):
    """Whether a defect can show in a case at all (by construction of the defect, not by looking at a result)."""
    N, dt = case.N, case.dt
    if defect == "p_transposed":
        return True                      # the start covariance is not symmetric (asserted)
    if defect == "b_from_next":
        return N >= 2 and dt > 0         # landmark f takes the B block of (f + 1) % N; at dt = 0 no landmark depends on the base state: B = 0
    if defect == "d_transposed":
        return N >= 1 and dt > 0         # at dt = 0 a landmark stays where it is: D is diagonal up to the finite differences' rounding
    if defect == "noise_boundary_shifted":
        return dt > 0                    # Q(0) = 0
    if defect == "ragged_last_unpropagated":
        return N % PCH != 0 and dt > 0   # at dt = 0 F is the identity up to the finite differences' rounding: nothing to propagate
    if defect == "means_from_new_base":
        return N >= 1 and dt > 0 and case.state != "initial"  # the base state must move
    if defect == "flush_left_out":
        return case.family == "flush"
    raise ValueError(defect)


def structured_fp64(F, P, dt, N, defect=None, absolute=False, flush=True):
    """P' = prune(F P F^T + Q) by the structure of F -- X = F P (base rows: A; landmark rows: 9 + 3 terms), P' = X F^T (base columns: A;
    landmark columns: 9 + 3 terms) -- in numpy fp64, with one of SIGMA_DEFECTS.  absolute: |F| |P| |F|^T + Q, unpruned (the bound's mag)."""
    assert defect is None or defect in SIGMA_DEFECTS
    n = BASE + 3 * N
    A, B, D = (a.astype(np.float64) for a in split_F(F, N))
    P = np.asarray(P, np.float64)
    q = noise_diag(n, dt, tuple(b + 1 for b in NOISE_BOUNDS) if defect == "noise_boundary_shifted" else NOISE_BOUNDS).astype(np.float64)
    P0 = P
    if absolute:
        A, B, D, P = np.abs(A), np.abs(B), np.abs(D), np.abs(P)
    if defect == "p_transposed":
        P = P.T
    if defect == "b_from_next":
        B = np.roll(B, -1, axis=0)
    if defect == "d_transposed":
        D = D.transpose(0, 2, 1)
    X = np.empty((n, n))
    X[:BASE] = A @ P[:BASE]
    if N:
        Pl = P[BASE:].reshape(N, 3, n)
        X[BASE:] = (np.einsum("frc,cj->frj", B, P[7:16]) + np.einsum("frq,fqj->frj", D, Pl)).reshape(3 * N, n)
    Pn = np.empty((n, n))
    Pn[:, :BASE] = X[:, :BASE] @ A.T
    if N:
        Xl = X[:, BASE:].reshape(n, N, 3)
        Pn[:, BASE:] = (np.einsum("ic,gsc->igs", X[:, 7:16], B) + np.einsum("igq,gsq->igs", Xl, D)).reshape(n, 3 * N)
    if defect == "ragged_last_unpropagated" and N % PCH:
        r = slice(BASE + 3 * (N - 1), n)
        Pn[:BASE, r] = P0[:BASE, r]
        Pn[r, :BASE] = P0[r, :BASE]
    Pn[np.arange(n), np.arange(n)] += q
    if flush and not absolute and defect != "flush_left_out":
        Pn[~(np.abs(Pn) > FLUSH)] = 0
    return Pn


@functools.lru_cache(maxsize=None)
def _dense_reference(N, state, scale_exp, dt):
    st = _inputs(N, state, scale_exp)
    r = _reference(N, state, scale_exp, dt, 1)
    E = structured_fp64(r["F"], st["Sigma"], dt, N)
    mag = structured_fp64(r["F"], st["Sigma"], dt, N, absolute=True)
    return E, mag, DENSE_UNITS * UNIT * mag + DENSE_FLOOR


def dense_reference(case):
    """(E, mag, the elementwise bound) of the case's (first) process(dt); shared, left unchanged."""
    return _dense_reference(case.N, case.state, case.scale_exp, case.dt)


def dense_units(got, case):
    """max |got - E| / (6e-8 mag) over the elements the floor does not cover alone: the figure the tests print and the documents record (of DENSE_UNITS)."""
    E, mag, _ = dense_reference(case)
    err = np.abs(np.asarray(got, np.float64) - E)
    sel = err > DENSE_FLOOR
    return float((err[sel] / (UNIT * mag[sel])).max()) if sel.any() else 0.0


def defective_means(case):
    """The landmark means propagated with the NEW base state (the fp32 oracle's own convolve functions)."""
    st = inputs(case)
    o = _oracle(np.float32)
    nb = o.convolve_base_state(st["base_mu"], np.float32(case.dt))
    out = np.stack([o.convolve_feature(nb, f, np.float32(case.dt)) for f in st["feat_mu"]])
    o.close()
    return out


# ---------------------------------------------------------------------------------------------------------------- naming a mismatch
REGIONS = ("base block", "base rows", "base columns", "landmark block")


def region_masks(n):
    i, j = np.indices((n, n))
    return {"base block": (i < BASE) & (j < BASE), "base rows": (i < BASE) & (j >= BASE), "base columns": (i >= BASE) & (j < BASE),
            "landmark block": (i >= BASE) & (j >= BASE)}


def region_of(i, j):
    """The workgroup of predict_fused_kernel that writes Sigma(i, j)."""
    if i < BASE and j < BASE:
        return "base block"
    if i < BASE:
        return "base-row chunk %d" % ((j - BASE) // (3 * PCH))
    if j < BASE:
        return "base-column chunk %d" % ((i - BASE) // (3 * PCH))
    return "tile (%d, %d)" % ((i - BASE) // (3 * PT), (j - BASE) // (3 * PT))


def mismatch(got, want):
    """None if two states agree in every bit of the mean and of Sigma, else a sentence that names where they do not."""
    for key in ("base_mu", "feat_mu"):
        bad = np.argwhere(np.asarray(got[key]) != np.asarray(want[key]))
        if bad.shape[0]:
            k = tuple(int(x) for x in bad[0])
            return "%s: %d elements differ, the first at %s (%r against %r)" % (key, bad.shape[0], k, got[key][k], want[key][k])
    bad = np.argwhere(np.asarray(got["Sigma"]) != np.asarray(want["Sigma"]))
    if bad.shape[0]:
        i, j = int(bad[0][0]), int(bad[0][1])
        regions = sorted({region_of(int(a), int(b)) for a, b in bad[:4096]})
        return "Sigma: %d elements differ, the first at (%d, %d) in %s (%r against %r); regions touched: %s" % (
            bad.shape[0], i, j, region_of(i, j), got["Sigma"][i, j], want["Sigma"][i, j], ", ".join(regions[:12]))
    return None
