"""NumPy restatements of the zero-velocity update (include/ekfvio.h, ekfvio_set_zupt; ekf_vio_amd/csrc/zupt.hip, zupt.h), shared by
tests/test_zupt_cpu.py and tests/test_gpu_zupt.py (a plain module, imported like _imu_cases.py).  Everything here runs on the CPU; nothing
in this file looks at what the HIP kernels return.

  decide(...)              the decision, fp32, line by line: what ekfvio_zupt_decide and the device are held to, bit for bit.
  kernel_order_fp32(...)   the update in zupt.hip's order of operations, fp32, multiply and add rounded separately (the library is built
                           without contraction): what the device is held to, bit for bit.  It fixes what the header leaves open.
  kernel_order(..., dtype, second_order)
                           the same lines in fp64: the yardstick of the criterion of tests/_imu_cases.py (reference()); and in fp32 in a
                           second honest rounding order, a printed figure.
  plain_update(..., dtype) the update as a textbook would write it -- K = Sigma H^T S^-1 by numpy.linalg, (I - K H) Sigma (I - K H)^T + K R K^T
                           as products -- independent of the specification's formula: the fp64 cross-check of the yardstick, and what the experiment runs.
  experiment(...)          the standing-still experiment of the README's table, in the fp64 oracle.
"""
import numpy as np

import _imu_cases as ic
from ekf_vio_amd.sim import Scenario
from oracle import OracleFilter

BASE = 22
ROWS = np.arange(7, 13)  # the state rows H selects: vel 7..9, omega 10..12
FLUSH = ic.FLUSH


# ------------------------------------------------------------------------------------------------------------------ the decision
def decide(prev_px, cur_px, passed, max_flow_px, min_tracks, min_ratio):
    """(flow2[count] fp32, n_pass, n_still, stationary) by the header's lines."""
    f = np.float32
    p = np.asarray(prev_px, f).reshape(-1, 2)
    q = np.asarray(cur_px, f).reshape(-1, 2)
    ok = np.asarray(passed, np.uint8).ravel() != 0
    t2 = f(max_flow_px) * f(max_flow_px)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = q[:, 0] - p[:, 0], q[:, 1] - p[:, 1]
        e2 = dx * dx + dy * dy
        still = ok & (e2 <= t2)  # (a NaN compares false)
    assert e2.dtype == f
    flow2 = np.where(ok, e2, f(-1)).astype(f)
    n_pass, n_still = int(ok.sum()), int(still.sum())
    stationary = int(n_pass >= int(min_tracks) and f(n_still) >= f(min_ratio) * f(n_pass))
    return flow2, n_pass, n_still, stationary


# ------------------------------------------------------------------------------------------------------------------ the update
def _mu_of(st):
    return np.concatenate([np.asarray(st["base_mu"]).ravel(), np.asarray(st["feat_mu"]).ravel()])


def _state_of(mu, Sig, like):
    N = np.asarray(like["feat_mu"]).reshape(-1, 3).shape[0]
    out = {k: np.array(v, copy=True) for k, v in like.items()}
    out["base_mu"], out["feat_mu"], out["Sigma"] = mu[:BASE].copy(), mu[BASE:].reshape(N, 3).copy(), Sig
    return out


def kernel_order(st, vel_var, omega_var, dtype=np.float32, second_order=False):
    """zupt_gain_kernel + zupt_joseph_kernel restated, multiply and add rounded separately.  P[i, j] is Sigma's element in row i, column j as
    stored.  dtype = float32: the kernels' bits (kernel_order_fp32); float64: the same lines in fp64, the yardstick of the criterion.
    second_order: the same formula in a second honest rounding order -- every six-term sum formed by itself, descending, and then added or
    subtracted as a whole (Sigma' = (Sigma - (K W)) + (G K^T), t = x - (k Pb), dm likewise): a figure tests/test_zupt_cpu.py prints beside
    the criterion (how far two honest fp32 orders of one formula lie apart), not a yardstick."""
    f = dtype
    mu = _mu_of(st).astype(f)
    P = np.asarray(st["Sigma"]).astype(f)
    n = P.shape[0]
    Rd = np.array([np.float32(vel_var)] * 3 + [np.float32(omega_var)] * 3).astype(f)
    Pb = P[np.ix_(ROWS, ROWS)]  # P(7+r, 7+c)
    L = np.zeros((6, 6), f)
    for j in range(6):
        d = Pb[j, j] + Rd[j]
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        L[j, j] = np.sqrt(d)
        for r in range(j + 1, 6):
            v = Pb[r, j]
            for k in range(j):
                v = v - L[r, k] * L[j, k]
            L[r, j] = v / L[j, j]
    y = -mu[ROWS]
    x = P[:, ROWS].copy()     # x_r(i) = P(i, 7+r)
    w = P[ROWS, :].T.copy()   # w_r(i) = P(7+r, i)
    kk = np.zeros((n, 6), f)
    for r in range(6):
        v = x[:, r]
        for k in range(r):
            v = v - kk[:, k] * L[r, k]
        kk[:, r] = v / L[r, r]
    for r in range(5, -1, -1):
        v = kk[:, r]
        for k in range(r + 1, 6):
            v = v - kk[:, k] * L[k, r]
        kk[:, r] = v / L[r, r]
    if not second_order:
        t = x.copy()
        for s in range(6):
            t = t - kk[:, s:s + 1] * Pb[s][None, :]
        dm = np.zeros(n, f)
        for r in range(6):
            dm = dm + kk[:, r] * y[r]
    else:
        acc = np.zeros((n, 6), f)
        dm = np.zeros(n, f)
        for s in range(5, -1, -1):
            acc = acc + kk[:, s:s + 1] * Pb[s][None, :]
            dm = dm + kk[:, s] * y[s]
        t = x - acc
    G = kk * Rd[None, :] - t
    mu2 = mu + dm
    q = mu2[3:7]
    qn = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    mu2[3:7] = q / qn
    if not second_order:
        V = P.copy()
        for s in range(6):
            V = V - kk[:, s:s + 1] * w[:, s][None, :]
        for s in range(6):
            V = V + G[:, s:s + 1] * kk[:, s][None, :]
    else:
        KW, GK = np.zeros((n, n), f), np.zeros((n, n), f)
        for s in range(5, -1, -1):
            KW = KW + kk[:, s:s + 1] * w[:, s][None, :]
            GK = GK + G[:, s:s + 1] * kk[:, s][None, :]
        V = (P - KW) + GK
    V[~(np.abs(V) > f(FLUSH))] = 0
    assert V.dtype == f and mu2.dtype == f
    return _state_of(mu2, V, st)


def kernel_order_fp32(st, vel_var, omega_var):
    return kernel_order(st, vel_var, omega_var, np.float32)


def reference(st, vel_var, omega_var):
    """(s32, s64) of the criterion of tests/_imu_cases.py (errors / tolerances / ratios): the SECOND fp32 rounding order, independent of the
    order under test, whose error scales the allowance, and the specification's lines in fp64."""
    return kernel_order(st, vel_var, omega_var, np.float32, second_order=True), kernel_order(st, vel_var, omega_var, np.float64)


CANCELLATION_MAX = 1.0  # beyond it the 4 x criterion is not asserted (hold): see there
U = 2.0 ** -24      # unit roundoff of fp32


def cond_S(st, vel_var, omega_var):
    P = np.asarray(st["Sigma"], np.float64)
    S = np.tril(P[np.ix_(ROWS, ROWS)])
    S = S + np.tril(S, -1).T + np.diag([float(np.float32(vel_var))] * 3 + [float(np.float32(omega_var))] * 3)
    return float(np.linalg.cond(S))


def cancellation(st, vel_var, omega_var):
    """max over the unmeasured state rows i with Sigma(i,i) > 0 of  sum_s |k_s(i) w_s(i)| / Sigma(i,i), in fp64.  The update takes
    sum_s k_s(i) w_s(i) out of the variance Sigma(i,i), and in exact arithmetic that sum lies in [0, Sigma(i,i)].  A value above 1 says
    the six products are larger than the variance they are subtracted from and cancel among themselves first."""
    P = np.asarray(st["Sigma"], np.float64)
    Rd = np.array([float(np.float32(vel_var))] * 3 + [float(np.float32(omega_var))] * 3)
    Pb = P[np.ix_(ROWS, ROWS)]
    S = np.tril(Pb) + np.tril(Pb, -1).T + np.diag(Rd)
    K = np.linalg.solve(S, P[:, ROWS].T).T
    d = np.diag(P)
    keep = d > 0
    keep[ROWS] = False
    return float(((np.abs(K) * np.abs(P[ROWS, :].T)).sum(axis=1)[keep] / d[keep]).max()) if keep.any() else 0.0


def apriori_bounds(st, vel_var, omega_var):
    """Elementwise bounds on |fp32 result - fp64 result| of the specification's lines, from the number format alone (first order in u = 2^-24),
    evaluated in fp64.  Nothing here looks at an fp32 result.
      * A sum of k products accumulated term by term, stored once: at most (k + 1) u times the sum of the terms' magnitudes (the standard
        gamma_k bound).  Sigma'(i,j) has 12 products behind P(i,j): 13 u (|P| + sum |k_s w_s| + sum |g_s k_s|).  mu' has 6: 7 u (..) + u |mu|.
      * The gain comes out of a 6 x 6 Cholesky solve: normwise relative error at most 6 cond(S) u =: eK (n cond u, the textbook first-order
        bound of a backward-stable solve), taken per component.  It enters every product with a gain in it, and g = k R - (x - k Pb) inherits
        it at the size of its TERMS, not of its (cancelled) value: |dg_r| <= eK (|k_r| R_r + sum_s |k_s| |Pb(s,r)|).
    Returns (bound on the mean [n], bound on Sigma [n, n]).  Loose by construction (every rounding at its worst, all aligned), so it is the
    backstop, not the yardstick: it catches an order of operations that loses digits wholesale, on every state, whatever cond(S) is."""
    mu = _mu_of(st).astype(np.float64)
    P = np.asarray(st["Sigma"], np.float64)
    Rd = np.array([float(np.float32(vel_var))] * 3 + [float(np.float32(omega_var))] * 3)
    Pb = P[np.ix_(ROWS, ROWS)]
    S = np.tril(Pb) + np.tril(Pb, -1).T + np.diag(Rd)
    K = np.linalg.solve(S, P[:, ROWS].T).T
    W = P[ROWS, :]
    T = P[:, ROWS] - K @ Pb
    G = K * Rd[None, :] - T
    aK, aG = np.abs(K), np.abs(G)
    eK = 6.0 * cond_S(st, vel_var, omega_var) * U
    dG = eK * (aK * Rd[None, :] + aK @ np.abs(Pb))
    # rounding of g itself: 7 products and differences at the size of its terms
    dG = dG + 8.0 * U * (aK * Rd[None, :] + np.abs(P[:, ROWS]) + aK @ np.abs(Pb))
    terms = np.abs(P) + aK @ np.abs(W) + aG @ aK.T
    bS = 13.0 * U * terms + eK * (aK @ np.abs(W)) + dG @ aK.T + eK * (aG @ aK.T)
    y = np.abs(mu[ROWS])
    bm = U * np.abs(mu) + (7.0 * U + eK) * (aK @ y)
    bm[3:7] = bm[3:7] + 4.0 * bm[3:7].max() + 6.0 * U  # the renormalisation: each component moves with the norm's error, and five more roundings
    return bm, bS


def hold(what, got, st, vel_var, omega_var):
    """What an fp32 result `got` of the update from `st` is held to; prints each figure before it asserts.  Shared by the CPU test (got: the
    kernels' order restated) and the GPU test (got: the device).
      A. apriori_bounds, elementwise, on every state.
      B. the criterion of tests/_imu_cases.py against reference(): err(got, fp64) <= 4 x err(second fp32 order, fp64) + 2^-23 scale, per
         quantity, on every state with cancellation() <= 1.  The factor 4 presumes that two honest fp32 orders of one formula err alike.
         That holds while each element's error is set by roundings at the size of the element.  Where the products subtracted from a
         variance exceed it and cancel among themselves, the partial sums are larger than every operand and each order rounds at the
         size of ITS partial sums: their errors are two draws whose ratio no fixed factor bounds.  Of the states here that is the one of
         N = 1 alone (2.03 and 1.95 with variances 1e-4 and 1e-2/1e-6; every other state and pair is below 1): one landmark leaves depth
         and speed unobservable together, the depth variance falls from 74.3 to 64.1 through products of size up to 80 with partial sums
         near 130, and there, with variances 1e-4, the kernels' order is 7.1e-5 off in that element, the second order 1.6e-6, a BLAS
         evaluation 1.4e-5, the kernels' order with the exact gain rounded to fp32 3.3e-5; 12 roundings at 130 have a width of 2.6e-5.
         On such a state the ratios are printed and A alone is asserted.
    Returns the ratios of B."""
    for key in ("base_mu", "feat_mu", "Sigma"):
        assert np.isfinite(got[key]).all(), (what, key)
    s32, s64 = reference(st, vel_var, omega_var)
    cond, canc = cond_S(st, vel_var, omega_var), cancellation(st, vel_var, omega_var)
    bm, bS = apriori_bounds(st, vel_var, omega_var)
    em = np.abs(_mu_of(got).astype(np.float64) - _mu_of(s64))
    eS = np.abs(np.asarray(got["Sigma"], np.float64) - s64["Sigma"])
    FL = float(FLUSH)  # (an element either side of the prune threshold differs by at most the threshold)
    worst_m = float((em / np.maximum(bm, 1e-300)).max()) if em.size else 0.0
    worst_S = float((eS / (bS + FL)).max())
    r = ic.ratios(got, s32, s64)
    print("\nZUPT-HOLD %s: cond(S) %.3g cancellation %.3g  a-priori mean %.3g Sigma %.3g of the bound;  4x criterion: %s"
          % (what, cond, canc, worst_m, worst_S, "  ".join("%s %.3f" % kv for kv in r.items())))
    assert (em <= bm).all(), (what, "mean beyond the a-priori bound", int(np.argmax(em / np.maximum(bm, 1e-300))), worst_m)
    assert (eS <= bS + FL).all(), (what, "Sigma beyond the a-priori bound", np.unravel_index(int(np.argmax(eS / (bS + FL))), eS.shape), worst_S)
    if canc <= CANCELLATION_MAX:
        e, t = ic.errors(got, s64), ic.tolerances(s32, s64)
        for key in ic.QUANTITIES:
            assert e[key] <= t[key], (what, key, "error", e[key], "allowed", t[key], "second fp32 order", ic.errors(s32, s64)[key])
    return r


def plain_update(st, vel_var, omega_var, dtype=np.float64):
    """z = 0 on [vel; omega], R = diag, Joseph form, with numpy.linalg in `dtype` from the numbers of st as they are."""
    mu = _mu_of(st).astype(dtype)
    P = np.asarray(st["Sigma"]).astype(dtype)
    n = P.shape[0]
    H = np.zeros((6, n), dtype)
    H[np.arange(6), ROWS] = 1
    R = np.diag(np.array([np.float32(vel_var)] * 3 + [np.float32(omega_var)] * 3).astype(dtype))
    S = H @ P @ H.T + R
    K = (P @ H.T @ np.linalg.inv(S)).astype(dtype)
    A = np.eye(n, dtype=dtype) - K @ H
    P2 = A @ P @ A.T + K @ R @ K.T
    mu2 = mu + K @ (-(H @ mu))
    mu2[3:7] = mu2[3:7] / np.linalg.norm(mu2[3:7])
    P2[~(np.abs(P2) > dtype(FLUSH))] = 0
    assert P2.dtype == dtype and mu2.dtype == dtype
    return _state_of(mu2, P2, st)


# ------------------------------------------------------------------------------------------------------------------ the experiment
def experiment(N, sd, zupt, var=1e-4, moving=20, still=200, ref_frame=10, scenario_seed=3, noise_seed=1):
    """Scenario(N, seed=3) in the fp64 oracle: `moving` frames, then the truth stops; `still` frames with Gaussian noise (sd, metric) on z.
    zupt: the pseudo-measurement in front of every still frame's update from the second one.  Returns (position drift against the state
    after still frame `ref_frame`, |v| at the end, |omega| at the end)."""
    ic.use_threads()
    sc = Scenario(N, seed=scenario_seed)
    rng = np.random.default_rng(noise_seed)
    o = OracleFilter(np.float64)
    o.add_new_features(sc.initial_features())
    for z, R, p in sc.frames(moving):
        o.process(sc.dt), o.update(z, R, p)
    sc.vel[:] = 0
    sc.omega[:] = 0
    sc.acc[:] = 0
    z0, R, p = sc.measure()
    ref = None
    for k in range(still):
        z = (z0.astype(np.float64) + rng.normal(0.0, sd, z0.shape)).astype(np.float32)
        o.process(sc.dt)
        if zupt and k >= 1:
            o.set_state(plain_update(o.get_state(), var, var, np.float64))
        o.update(z, R, p)
        if k == ref_frame:
            ref = o.get_state()["base_mu"][:3].copy()
    b = o.get_state()["base_mu"]
    o.close()
    return float(np.linalg.norm(b[:3] - ref)), float(np.linalg.norm(b[7:10])), float(np.linalg.norm(b[10:13]))


def braking(N, first, var=1e-4, moving=20, still=30, scenario_seed=3):
    """The abrupt stop, noise-free: the scenario of experiment() with exact measurements for `still` frames behind the stop, the
    pseudo-measurement from still frame `first` on (None: never).  Returns (how far the position moved in still frame 0, the position's
    distance from the truth at the end, |v| at the end)."""
    ic.use_threads()
    sc = Scenario(N, seed=scenario_seed)
    o = OracleFilter(np.float64)
    o.add_new_features(sc.initial_features())
    for z, R, p in sc.frames(moving):
        o.process(sc.dt), o.update(z, R, p)
    sc.vel[:] = 0
    sc.omega[:] = 0
    sc.acc[:] = 0
    z, R, p = sc.measure()
    before = o.get_state()["base_mu"][:3].copy()
    jump = 0.0
    for k in range(still):
        o.process(sc.dt)
        if first is not None and k >= first:
            o.set_state(plain_update(o.get_state(), var, var, np.float64))
        o.update(z, R, p)
        if k == 0:
            jump = float(np.linalg.norm(o.get_state()["base_mu"][:3] - before))
    b = o.get_state()["base_mu"]
    o.close()
    return jump, float(np.linalg.norm(b[:3] - sc.pos)), float(np.linalg.norm(b[7:10]))
