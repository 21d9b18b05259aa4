"""Shared case definitions of tests/test_gpu_imu_extrinsics.py and tests/test_imu_extrinsics_cpu.py (a plain module, imported like _imu_cases.py,
whose start states, criterion and constants it reuses): the IMU update with the IMU in its own frame (include/ekfvio.h,
ekfvio_set_imu_extrinsics; ekf_vio_amd/csrc/imu_model.h, imu.hip).

    h(x) = [M w + b_gyr ; M (a + w x (w x p) - R(q)^T g) + b_acc]        M = R_ci^T, p = p_ci, w = mu[10:13], a = mu[13:16]

Four evaluations of one update from one fp32 state, none of which looks at what the HIP kernels return:
  * np_ext_update: fp64, H by central differences of h_ext, numpy.linalg, Joseph form -- the yardstick, independent of both fp32
    restatements and of the oracle (whose imu_update has no extrinsics); with jacobian="analytic" it writes H out and accepts one of
    DEFECTS.
  * kernel_order_fp32_ext: the header's lines in NumPy fp32, multiply and add rounded separately; from H and y on, imu.hip's order (the tail
    of _imu_cases.kernel_order_fp32, restated here with H and y as inputs: test_imu_extrinsics_cpu.py holds the two to the same bits on
    the model without extrinsics).  The device and ekfvio_imu_model are held to this bit for bit.
  * oracle_order_fp32_ext: a second honest fp32 rounding order -- c = w (w.p) - p (w.w) instead of the two cross products, C from the same
    closed form, the products with M summed from the last term to the first, S from Sigma H^T as the oracle's imu_update takes it, every
    sixteen-term sum in descending order.  It supplies err(fp32, fp64) of the project's criterion

        err(got, fp64) <= ACC_FACTOR * err(fp32 reference, fp64) + 2^-23 * scale            (_imu_cases: ACC_FACTOR = 4, QUANTITIES)

The start states are _imu_cases.start(N) with the case's quaternion, and base_mu[10:13] overwritten by OMEGA = (0.7, -1.1, 0.9) rad/s: the
scenario's own body rate is 0.1 rad/s about one axis, where c is below the noise and half of C vanishes.

Cases (17):
  extrinsics (N = 30, 0.97 u, generic gravity): the identity with p = 0 (the CONTROL: today's model), a signed permutation (IMU x forward,
      z up -> optical z forward, y down) with p = 0, the same with P = (0.05, -0.02, 0.11), a generic rotation (the permutation times 10
      degrees about (1, 2, -1)) with P, and the generic rotation with p parallel to omega (c = 0 up to rounding, C != 0); the permutation
      with P at the identity attitude with gravity along y (a level rig), the generic rotation at a quarter turn about x, gravity along -z.
  attitude (N = 30, generic rotation, P, generic gravity): identity, 1.03 u, w0.
  size (generic rotation, P, 1.03 u, generic gravity): N = 0, 1, 78 (n = 256, the workgroup edge), 79, 400; and 79 in a handle of capacity
      256 behind a camera update (camera_first).
  reading: a large innovation (_imu_cases.LARGE_OFFSET).
"""
import collections
import functools

import numpy as np

import _imu_cases as I

OMEGA = np.array([0.7, -1.1, 0.9])
P_ARM = np.array([0.05, -0.02, 0.11])
P_PAR = 0.1 * OMEGA / np.linalg.norm(OMEGA)
# IMU x forward, y left, z up -> optical x right, y down, z forward: v_cam = R_ci v_imu
R_PERM = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])


def axis_angle(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


R_GEN = R_PERM @ axis_angle((1, 2, -1), 10.0)
EXTS = collections.OrderedDict([
    ("identity-p0", (np.eye(3), np.zeros(3))),
    ("perm-p0", (R_PERM, np.zeros(3))),
    ("perm-p", (R_PERM, P_ARM)),
    ("generic-p", (R_GEN, P_ARM)),
    ("generic-ppar", (R_GEN, P_PAR)),
])

Case = collections.namedtuple("Case", "family N cap quat grav reading ext camera_first")
CONTROL = Case("extrinsics", 30, 30, "0.97u", "ggen", "noise", "identity-p0", False)
ANCHOR = Case("extrinsics", 30, 30, "0.97u", "ggen", "noise", "perm-p0", False)


def _cases():
    out = [Case("extrinsics", 30, 30, "0.97u", "ggen", "noise", e, False) for e in EXTS]
    out.append(Case("extrinsics", 30, 30, "identity", "gy", "noise", "perm-p", False))
    out.append(Case("extrinsics", 30, 30, "quarter-x", "g-z", "noise", "generic-p", False))
    for q in ("identity", "1.03u", "w0"):
        out.append(Case("attitude", 30, 30, q, "ggen", "noise", "generic-p", False))
    for N in (0, 1, 78, 79, 400):
        out.append(Case("size", N, N, "1.03u", "ggen", "noise", "generic-p", False))
    out.append(Case("size", 79, 256, "1.03u", "ggen", "noise", "generic-p", True))
    out.append(Case("reading", 30, 30, "1.03u", "ggen", "large", "generic-p", False))
    return out


CASES = _cases()


def case_id(c):
    s = "%s-N%d%s-%s-%s-%s" % (c.family, c.N, "" if c.cap == c.N else "cap%d" % c.cap, c.quat, c.grav, c.ext)
    return s if c.reading == "noise" else s + "-" + c.reading


def ext32(name):
    """(R_ci, p_ci) of EXTS as the fp32 numbers every evaluation starts from."""
    R, p = EXTS[name]
    return R.astype(np.float32), p.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the model, fp64
def h_ext(base, g, R, p):
    M = np.asarray(R, np.float64).T
    w, a = base[10:13], base[13:16]
    c = np.cross(w, np.cross(w, p))
    return np.concatenate([M @ w + base[19:22], M @ (a + c - I.rot_t(base[3:7], np.asarray(g, np.float64))) + base[16:19]])


DEFECTS = ("M_transposed", "M_missing_from_q_columns", "c_missing_from_residual", "C_missing_from_H", "C_minus_2pw_dropped", "C_transposed",
           "p_in_imu_frame", "biases_in_camera_frame")


def np_ext_update(base, feat, Sig, gyro, acc, gv, av, g, R, p, jacobian="numeric", defect=None):
    """The update in plain numpy fp64: H by central differences of h_ext ("numeric") or written out ("analytic", which accepts one of
    DEFECTS), K = Sigma H^T S^-1 by numpy.linalg, Joseph form.  Returns dict(mu, Sigma, H, y, R, S)."""
    base, Sig = np.asarray(base, np.float64), np.asarray(Sig, np.float64)
    feat = np.asarray(feat, np.float64).ravel()
    gyro, acc, g, R, p = (np.asarray(a, np.float64) for a in (gyro, acc, g, R, p))
    assert defect is None or (defect in DEFECTS and jacobian == "analytic")
    n = Sig.shape[0]
    H = np.zeros((6, n))
    if jacobian == "numeric":
        for k in range(I.BASE):
            d = np.zeros(I.BASE)
            d[k] = 1e-6
            H[:, k] = (h_ext(base + d, g, R, p) - h_ext(base - d, g, R, p)) / 2e-6
        y = np.concatenate([gyro, acc]) - h_ext(base, g, R, p)
    else:
        M = R if defect == "M_transposed" else R.T
        pp = M @ p if defect == "p_in_imu_frame" else p
        w, a = base[10:13], base[13:16]
        c = np.cross(w, np.cross(w, pp))
        C = (w @ pp) * np.eye(3) + np.outer(w, pp) - 2.0 * np.outer(pp, w)
        if defect == "C_minus_2pw_dropped":
            C = (w @ pp) * np.eye(3) + np.outer(w, pp)
        if defect == "C_transposed":
            C = C.T
        jac = I.rt_gravity_jacobian(base[3:7], g)
        s = a + (0.0 if defect == "c_missing_from_residual" else c) - I.rot_t(base[3:7], g)
        H[0:3, 10:13] = M
        H[3:6, 13:16] = M
        H[3:6, 3:7] = -jac if defect == "M_missing_from_q_columns" else -M @ jac
        H[3:6, 10:13] = 0.0 if defect == "C_missing_from_H" else M @ C
        if defect == "biases_in_camera_frame":
            H[0:3, 19:22] = H[3:6, 16:19] = M
            h = np.concatenate([M @ (w + base[19:22]), M @ (s + base[16:19])])
        else:
            H[0:3, 19:22] = H[3:6, 16:19] = np.eye(3)
            h = np.concatenate([M @ w + base[19:22], M @ s + base[16:19]])
        y = np.concatenate([gyro, acc]) - h
    Rn = np.diag([gv] * 3 + [av] * 3)
    S = H @ Sig @ H.T + Rn
    K = Sig @ H.T @ np.linalg.inv(S)
    I_KH = np.eye(n) - K @ H
    Sig2 = I_KH @ Sig @ I_KH.T + K @ Rn @ K.T
    mu = np.concatenate([base, feat]) + K @ y
    mu[3:7] /= np.linalg.norm(mu[3:7])
    return dict(mu=mu, Sigma=Sig2, H=H, y=y, R=Rn, S=S)


# ---------------------------------------------------------------------------------------------------------------- fp32 restatements
def _cross32(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], np.float32)


def rt_gravity32(mu, g):
    """rt_gravity of imu_model.h in numpy fp32: (rg[3], jac[3, 4]) -- _imu_cases.kernel_order_fp32's lines."""
    f = np.float32
    w, c = mu[3], np.array([-mu[4], -mu[5], -mu[6]], f)
    uv = _cross32(c, g)
    uv = uv + uv
    cu = _cross32(c, uv)
    rg = (g + w * uv) + cu
    jac = np.zeros((3, 4), f)
    jac[:, 0] = uv
    for k in range(3):
        e = np.zeros(3, f)
        e[k] = 1
        ev = _cross32(e, g)
        ev = ev + ev
        a, b = _cross32(e, uv), _cross32(c, ev)
        jac[:, 1 + k] = -((w * ev + a) + b)
    return rg, jac


def plain_model_fp32(mu, g, gyro, acc):
    """(y[6], H[6, 16]) of the model without extrinsics, as _imu_cases.kernel_order_fp32 forms them."""
    f = np.float32
    rg, jac = rt_gravity32(mu, g)
    H, y = np.zeros((6, 16), f), np.zeros(6, f)
    for r in range(3):
        H[r, 4 + r] = H[r, 13 + r] = H[3 + r, 7 + r] = H[3 + r, 10 + r] = 1
        H[3 + r, :4] = -jac[r]
        y[r] = gyro[r] - (mu[10 + r] + mu[19 + r])
        y[3 + r] = acc[r] - ((mu[13 + r] + mu[16 + r]) - rg[r])
    return y, H


def ext_model_fp32(mu, g, R, p, gyro, acc):
    """(y[6], H[6, 16]): the header's lines (include/ekfvio.h, ekfvio_set_imu_extrinsics) in numpy fp32, one rounding per operation."""
    f = np.float32
    mu, g, R, p, gyro, acc = (np.asarray(a, f) for a in (mu, g, R, p, gyro, acc))
    M = R.T.copy()  # M[r][k] = R_ci[3 k + r]
    w, a = mu[10:13], mu[13:16]
    rg, jac = rt_gravity32(mu, g)
    t = _cross32(w, p)
    c = _cross32(w, t)
    s = (a + c) - rg
    d = (w[0] * p[0] + w[1] * p[1]) + w[2] * p[2]
    C = np.zeros((3, 3), f)
    for i in range(3):
        for j in range(3):
            v = w[i] * p[j] - (f(2) * p[i]) * w[j]
            C[i, j] = v + d if i == j else v
    H, y = np.zeros((6, 16), f), np.zeros(6, f)
    for r in range(3):
        hg = ((M[r, 0] * w[0] + M[r, 1] * w[1]) + M[r, 2] * w[2]) + mu[19 + r]
        ha = ((M[r, 0] * s[0] + M[r, 1] * s[1]) + M[r, 2] * s[2]) + mu[16 + r]
        y[r] = gyro[r] - hg
        y[3 + r] = acc[r] - ha
        for k in range(3):
            H[r, 4 + k] = M[r, k]
            H[3 + r, 7 + k] = M[r, k]
            H[3 + r, 4 + k] = (M[r, 0] * C[0, k] + M[r, 1] * C[1, k]) + M[r, 2] * C[2, k]
        H[r, 13 + r] = 1
        H[3 + r, 10 + r] = 1
        for k in range(4):
            H[3 + r, k] = -((M[r, 0] * jac[0, k] + M[r, 1] * jac[1, k]) + M[r, 2] * jac[2, k])
    assert H.dtype == f and y.dtype == f
    return y, H


def ext_model_fp32_other_order(mu, g, R, p, gyro, acc):
    """The same model by other formulas and sums: c = w (w.p) - p (w.w), the products with M summed from the last term to the first."""
    f = np.float32
    mu, g, R, p, gyro, acc = (np.asarray(a, f) for a in (mu, g, R, p, gyro, acc))
    M = R.T.copy()
    w, a = mu[10:13], mu[13:16]
    rg, jac = rt_gravity32(mu, g)
    wp = w[2] * p[2] + (w[1] * p[1] + w[0] * p[0])
    ww = w[2] * w[2] + (w[1] * w[1] + w[0] * w[0])
    c = w * wp - p * ww
    s = a + (c - rg)

    def mv(row, v):
        return row[2] * v[2] + (row[1] * v[1] + row[0] * v[0])

    C = np.zeros((3, 3), f)
    for i in range(3):
        for j in range(3):
            C[i, j] = (wp if i == j else f(0)) + (w[i] * p[j] - f(2) * (p[i] * w[j]))
    H, y = np.zeros((6, 16), f), np.zeros(6, f)
    for r in range(3):
        y[r] = (gyro[r] - mu[19 + r]) - mv(M[r], w)
        y[3 + r] = (acc[r] - mu[16 + r]) - mv(M[r], s)
        H[r, 4:7] = M[r]
        H[3 + r, 7:10] = M[r]
        H[r, 13 + r] = H[3 + r, 10 + r] = 1
        for k in range(3):
            H[3 + r, 4 + k] = mv(M[r], C[:, k])
        for k in range(4):
            H[3 + r, k] = -mv(M[r], jac[:, k])
    assert H.dtype == f and y.dtype == f
    return y, H


def update_tail_fp32(st, y, H, gv, av, order="kernel"):
    """From H and y on.  order="kernel": imu.hip's order of operations (the tail of _imu_cases.kernel_order_fp32, every sum ascending over all
    sixteen columns, S = W H^T + R).  order="oracle": S from Sigma H^T as oracle/ekf_oracle.hpp's imu_update takes it, and every sixteen-term
    sum descending."""
    f = np.float32
    mu = np.concatenate([st["base_mu"], st["feat_mu"].ravel()]).astype(f)
    P = np.asarray(st["Sigma"], f)
    n = P.shape[0]
    gv, av = f(gv), f(av)
    cols = list(range(16)) if order == "kernel" else list(range(15, -1, -1))
    pc = P[:, I.COLS]        # Sigma(i, cols[c])
    pr = P[I.COLS, :].T      # Sigma(cols[c], i)
    Pb = P[np.ix_(I.COLS, I.COLS)]
    Wb = np.zeros((6, 16), f)
    for cc in cols:
        Wb = Wb + H[:, cc:cc + 1] * Pb[cc:cc + 1, :]
    S = np.zeros((6, 6), f)
    if order == "kernel":
        for cc in cols:
            S = S + Wb[:, cc:cc + 1] * H[:, cc][None, :]
    else:
        Xb = np.zeros((16, 6), f)  # (Sigma H^T)(cols[c], s)
        for cc in cols:
            Xb = Xb + Pb[:, cc:cc + 1] * H[:, cc][None, :]
        for cc in cols:
            S = S + H[:, cc:cc + 1] * Xb[cc:cc + 1, :]
    S = S + np.diag(np.array([gv] * 3 + [av] * 3, f))
    L = np.zeros((6, 6), f)
    for j in range(6):
        d = S[j, j]
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        L[j, j] = np.sqrt(d)
        for r in range(j + 1, 6):
            v = S[r, j]
            for k in range(j):
                v = v - L[r, k] * L[j, k]
            L[r, j] = v / L[j, j]
    x, wm = np.zeros((n, 6), f), np.zeros((n, 6), f)
    for cc in cols:
        x = x + pc[:, cc:cc + 1] * H[:, cc][None, :]
        wm = wm + H[:, cc][None, :] * pr[:, cc:cc + 1]
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
    tc = pc.copy()
    for s in range(6):
        tc = tc - kk[:, s:s + 1] * Wb[s][None, :]
    th = np.zeros((n, 6), f)
    for cc in cols:
        th = th + tc[:, cc:cc + 1] * H[:, cc][None, :]
    Rd = np.array([gv] * 3 + [av] * 3, f)
    G = kk * Rd[None, :] - th
    dm = np.zeros(n, f)
    for r in range(6):
        dm = dm + kk[:, r] * y[r]
    mu2 = mu + dm
    q = mu2[3:7]
    qn = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    mu2[3:7] = q / qn
    V = P.copy()
    for s in range(6):
        V = V - kk[:, s:s + 1] * wm[:, s][None, :]
    for s in range(6):
        V = V + G[:, s:s + 1] * kk[:, s][None, :]
    V[~(np.abs(V) > I.FLUSH)] = 0
    assert V.dtype == f and mu2.dtype == f
    N = st["feat_mu"].shape[0]
    return dict(base_mu=mu2[:I.BASE].copy(), feat_mu=mu2[I.BASE:].reshape(N, 3).copy(), Sigma=V)


def kernel_order_fp32_ext(st, gyro, acc, gv, av, g, R, p):
    """The header's lines and imu.hip's order in numpy fp32: what the device is held to, bit for bit.  R = p = None: the model without."""
    mu = st["base_mu"].astype(np.float32)
    g, gyro, acc = (np.asarray(a, np.float32) for a in (g, gyro, acc))
    y, H = plain_model_fp32(mu, g, gyro, acc) if R is None else ext_model_fp32(mu, g, R, p, gyro, acc)
    return update_tail_fp32(st, y, H, gv, av, "kernel")


def oracle_order_fp32_ext(st, gyro, acc, gv, av, g, R, p):
    """The second, independent fp32 rounding order: err(fp32, fp64) of the criterion."""
    y, H = ext_model_fp32_other_order(st["base_mu"].astype(np.float32), g, R, p, gyro, acc)
    return update_tail_fp32(st, y, H, gv, av, "oracle")


# ---------------------------------------------------------------------------------------------------------------- inputs and references
@functools.lru_cache(maxsize=None)
def inputs(case):
    """(start state, gyro, accel, gyro variance, accel variance, gravity, R_ci, p_ci), every number an fp32 one."""
    st = I.fresh(I.start(case.N)[0])
    st["base_mu"][3:7] = I.QUATS[case.quat].astype(np.float32)
    st["base_mu"][10:13] = OMEGA.astype(np.float32)
    g = np.array(I.GRAVS[case.grav], np.float32)
    gv, av = np.float32(I.DEFAULT_VAR[0]), np.float32(I.DEFAULT_VAR[1])
    R, p = ext32(case.ext)
    h = h_ext(st["base_mu"].astype(np.float64), g.astype(np.float64), R.astype(np.float64), p.astype(np.float64))
    if case.reading == "large":
        d = np.concatenate(I.LARGE_OFFSET)
    else:
        rng = np.random.default_rng([case.N, list(I.QUATS).index(case.quat), list(I.GRAVS).index(case.grav), list(EXTS).index(case.ext)])
        d = np.concatenate([rng.normal(0, I.NOISE[0], 3), rng.normal(0, I.NOISE[1], 3)])
    z = (h + d).astype(np.float32)
    return st, z[:3].copy(), z[3:].copy(), gv, av, g, R, p


def np_state(out, like):
    return I.np_state(out, like)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(the second fp32 order's result, the fp64 yardstick's result) of a case; left unchanged by everything that reads it."""
    st, gyro, acc, gv, av, g, R, p = inputs(case)
    s64 = np_state(np_ext_update(st["base_mu"], st["feat_mu"], st["Sigma"], gyro, acc, float(gv), float(av), g, R, p), st)
    return oracle_order_fp32_ext(st, gyro, acc, gv, av, g, R, p), s64
