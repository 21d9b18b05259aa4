"""Shared case definitions of tests/test_gpu_imu_matrix.py and tests/test_imu_cases_cpu.py (a plain module, imported like _update_cases.py),
and the independent numpy evaluation of the IMU update that tests/test_imu_oracle_cpu.py checks the specification with.

One IMU update per case (imu_gain_kernel + imu_joseph_kernel, ekf_vio_amd/csrc/imu.hip), teacher-forced from ONE fp32 state: the HIP
kernels, the fp32 oracle and the fp64 oracle (oracle/ekf_oracle.hpp: imu_update, the specification) evaluate the same update from the same
fp32 numbers.  Everything here runs on the CPU; nothing in this file looks at what the HIP kernels return.

The start state is tests/test_gpu_imu.py's -- Scenario(N, seed=7, dt=0.05), five frames of process + update in the fp64 oracle, rounded to
fp32 (N = 0: one process(0.05) from the initial state) -- with base_mu[3:7] overwritten by the case's quaternion.  The state need not be
physically consistent for one teacher-forced step.  The readings are h(x) of that state plus seeded noise (sigma 1e-2 rad/s, 1e-1 m/s^2)
unless the case says otherwise.

Why the families exist.  tests/test_gpu_imu.py runs near q = (1, 0, 0, 0) with gravity (0, 9.81, 0), parallel to the scenario's rotation
axis: uv = 2 c x g of rt_gravity is then ~0, and with it the whole d/dw column, the whole d/dy column and the e_k x uv term of the other
columns of the accelerometer rows of H.  A kernel that gets any of these wrong passes there (asserted in test_imu_cases_cpu.py on the
control case).
  * "attitude" (N = 30): QUATS x GRAVS, 7 x 3 -- the identity (the old regime, the control), 1.03 u and 0.97 u (not unit, as the
    specification allows), -u (w < 0), (0, 1, 0, 0) (w = 0), quarter turns about z and x; gravity along y, along -z, and generic.
  * "size" (1.03 u, generic gravity): n = 22 + 3 N on and beside the 256-row workgroup edge of both kernels -- N = 0 (n = 22), 1 (25),
    77 (253), 78 (256), 79 (259), 163 (511), 164 (514), 400 (1222: five workgroups) -- and two handles whose capacity exceeds N (79 in 256,
    30 in 100), on which a camera process + update runs immediately before the state is loaded: the Km / Gm / Wt buffers the IMU update
    borrows then hold a camera update's leftovers, and ld > n + 1.
  * "reading" (N = 30, 1.03 u, generic gravity): a large innovation (gyro off by (0.5, -0.3, 0.4) rad/s, accel by (2, -1.5, 1) m/s^2: the
    quaternion renormalisation matters), an innovation of exactly zero in the fp32 specification, and the variance pairs VARS.

The criterion, per quantity X of QUANTITIES (base mean, landmark means, Sigma's quaternion rows 3-6, its base block, both base x landmark
blocks, its landmark block, all of Sigma elementwise):

    err(HIP, fp64) <= ACC_FACTOR * err(fp32 oracle, fp64) + 2^-23 * scale(X)

err and scale are max-abs for the means and the elementwise measure, Frobenius norms for the blocks; scale is taken of the fp64 result.
ACC_FACTOR = 4.0 is the project's constant (tests/test_gpu_parity.py), copied.  The floor is derived, not measured: one unit in the last
place of fp32 at the quantity's own magnitude, below which a stored fp32 result carries no information.  The camera update's MU_FLOOR /
SIG_FLOOR are not used.

SENSITIVITY, measured on the CPU by tests/test_imu_cases_cpu.py (run with -s): each defect put into the numpy fp64 evaluation with the
analytic H; "largest" is the largest (fp64 result moved by the defect / tolerance of the case) over the 26 cases of the families attitude and
reading, held to MARGIN = 10; "seen in" counts the cases at or above MARGIN.
    defect                        largest   in case (quantity)                                 seen in
    d/dw column zeroed            3.8e5     w0, generic gravity (quaternion rows of Sigma)     22 of 26
    d/dx column zeroed            8.6e5     w0, gravity along y (landmark x base block)        26
    d/dy column zeroed            5.7e5     1.03 u, generic gravity (quaternion rows)          24
    d/dz column zeroed            7.1e5     quarter turn about z, gravity along y (q. rows)    23
    d/dw column's sign flipped    7.5e5     w0, generic gravity (quaternion rows)              22
    e_k x uv term dropped         5.6e5     w0, generic gravity (quaternion rows)              22
    c x ev term dropped           5.1e5     w0, generic gravity (quaternion rows)              23
    (x, y, z) part transposed     1.8e6     1.03 u, generic gravity (quaternion rows)          26
    residual with + R(q)^T g      2.5e7     w0, gravity along y (base mean)                    26
    bias columns exchanged        3.6e6     w0, gravity along y (base block)                   26
    variances exchanged           3.0e5     variances (1e-6, 1e-1) (base block)                25
    quaternion not normalised     4.8e4     variances (1, 1) (base mean)                       20
    gravity rotated one place     1.3e7     w0, gravity along y (base mean)                    26
Over +-u (1.03 u, 0.97 u, -u) with the generic gravity alone every Jacobian defect reaches at least 2.7e5.  At the control (identity,
gravity along y) the d/dw, d/dy and e_k x uv defects move nothing (6.7e-10 tolerances: uv = 2 c x g is exactly zero).  The fp32 oracle
is 5e-8 .. 5e-7 from fp64 on the base mean on every case and, from N = 30 on, 5e-8 .. 9e-8 relative on the quaternion rows (7.5e-7 at N = 0,
1.3e-6 at N = 1); cond(S) is 4.9 at N = 0, 168 at N = 1 and 1.2 .. 1.6 from N = 30 on.

KERNEL_ORDER: kernel_order_fp32() restates imu.hip's order of operations in numpy fp32 (all sixteen columns summed where the oracle skips
H's zeros, S from H Sigma where the oracle uses Sigma H^T, multiply and add rounded separately: the library is built with
-ffp-contract=off).  On the CPU it uses at most 0.25 of the tolerance on every quantity of every case.

MEASURED ON THE MI355X (tests/test_gpu_imu_matrix.py), the worst err(HIP, fp64) / tolerance per family and quantity -- the unchanged
kernels sit inside 4 x oracle error + 1 ulp everywhere, at about the fp32 oracle's own error (0.25 would be exactly the oracle's):
    family     base   landmarks  quat rows  base block  base x lm  lm x base  lm block  elementwise
    attitude   0.242  0.166      0.183      0.178       0.184      0.183      0.176     0.190
    size       0.231  0.163      0.251      0.221       0.201      0.219      0.199     0.201
    reading    0.232  0.159      0.176      0.171       0.172      0.169      0.172     0.149
    two records on one stamp (process(0) + update): 0.25 on every quantity (0.231 landmarks): process(0)'s own error, which the HIP path
    shares bit for bit with the fp32 oracle, dominates both sides.
The kernels' results equalled kernel_order_fp32's in every bit of every case (mean and all of Sigma, up to n = 1222), which the GPU test
now asserts.  No floor beyond the derived one and no change to imu.hip was needed.
"""
import collections
import functools

import numpy as np

from ekf_vio_amd.sim import Scenario
from oracle import OracleFilter, max_threads, set_threads

BASE = 22
SEED = 7
DT = 0.05
WARM_FRAMES = 5
ACC_FACTOR = 4.0  # tests/test_gpu_parity.py, copied
ULP = 2.0 ** -23  # the floor: one fp32 unit in the last place of the quantity's magnitude
MARGIN = 10.0     # a defect in view must move the fp64 answer by this many tolerances (test_imu_cases_cpu.py)
FLUSH = np.float32(1e-8) * np.float32(1e-5)  # EKF_FLUSH_THRESH (common.h), the oracle's flush_thresh()
COLS = np.array([3, 4, 5, 6, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21])  # the sixteen state columns H touches

_U = np.array([0.6, -0.5, 0.4, 0.48])
_U = _U / np.linalg.norm(_U)
_H = np.sqrt(0.5)
QUATS = collections.OrderedDict([
    ("identity", np.array([1.0, 0.0, 0.0, 0.0])),
    ("1.03u", 1.03 * _U),
    ("0.97u", 0.97 * _U),
    ("-u", -_U),
    ("w0", np.array([0.0, 1.0, 0.0, 0.0])),
    ("quarter-z", np.array([_H, 0.0, 0.0, _H])),
    ("quarter-x", np.array([_H, _H, 0.0, 0.0])),
])
GRAVS = collections.OrderedDict([
    ("gy", (0.0, 9.81, 0.0)),
    ("g-z", (0.0, 0.0, -9.81)),
    ("ggen", (5.0, 7.0, -4.6)),
])
DEFAULT_VAR = (1e-4, 1e-2)  # ekfvio_default_config: imu_gyro_variance, imu_accel_variance
VARS = ((1e-6, 1e-1), (1.0, 1.0), (1e-4, 1e-8))
LARGE_OFFSET = (np.array([0.5, -0.3, 0.4]), np.array([2.0, -1.5, 1.0]))
NOISE = (1e-2, 1e-1)

Case = collections.namedtuple("Case", "family N cap quat grav reading var camera_first")
CONTROL = Case("attitude", 30, 30, "identity", "gy", "noise", DEFAULT_VAR, False)


def _cases():
    out = []
    for q in QUATS:
        for g in GRAVS:
            out.append(Case("attitude", 30, 30, q, g, "noise", DEFAULT_VAR, False))
    for N in (0, 1, 77, 78, 79, 163, 164, 400):
        out.append(Case("size", N, N, "1.03u", "ggen", "noise", DEFAULT_VAR, False))
    out.append(Case("size", 79, 256, "1.03u", "ggen", "noise", DEFAULT_VAR, True))
    out.append(Case("size", 30, 100, "1.03u", "ggen", "noise", DEFAULT_VAR, True))
    out.append(Case("reading", 30, 30, "1.03u", "ggen", "large", DEFAULT_VAR, False))
    out.append(Case("reading", 30, 30, "1.03u", "ggen", "zero", DEFAULT_VAR, False))
    for v in VARS:
        out.append(Case("reading", 30, 30, "1.03u", "ggen", "noise", v, False))
    return out


CASES = _cases()


def case_id(c):
    s = "%s-N%d%s-%s-%s" % (c.family, c.N, "" if c.cap == c.N else "cap%d" % c.cap, c.quat, c.grav)
    if c.reading != "noise":
        s += "-" + c.reading
    if c.var != DEFAULT_VAR:
        s += "-var%g,%g" % c.var
    return s


def handle_capacity(c):
    """max_features of the case's handle (a handle cannot be created for no landmark at all)."""
    return max(c.cap, 1)


def use_threads():
    set_threads(min(max_threads(), 16))


# ---------------------------------------------------------------------------------------------------------------- the model, in numpy
def rot_t(q, v):
    """R(q)^T v with the filter's rotation formula on the conjugate (q need not be normalised)."""
    w, c = q[0], -np.asarray(q[1:])
    uv = 2.0 * np.cross(c, v)
    return v + w * uv + np.cross(c, uv)


def h_imu(base, g):
    return np.concatenate([base[10:13] + base[19:22], base[13:16] + base[16:19] - rot_t(base[3:7], np.asarray(g, np.float64))])


JACOBIAN_DEFECTS = ("col_w_zeroed", "col_x_zeroed", "col_y_zeroed", "col_z_zeroed", "col_w_sign_flipped", "ek_x_uv_dropped",
                    "c_x_ev_dropped", "xyz_transposed")
DEFECTS = JACOBIAN_DEFECTS + ("residual_plus_rtg", "bias_columns_exchanged", "variances_exchanged", "quaternion_not_normalised",
                              "gravity_rotated_one_place")
BLIND_AT_CONTROL = ("col_w_zeroed", "col_w_sign_flipped", "col_y_zeroed", "ek_x_uv_dropped")  # uv = 2 c x g ~ 0 there


def rt_gravity_jacobian(q, g, defect=None):
    """d(R(q)^T g) / d(w, x, y, z), 3 x 4, written out as the specification does (ekf_oracle.hpp: rt_gravity), with one named defect."""
    q, g = np.asarray(q, np.float64), np.asarray(g, np.float64)
    w, c = q[0], -q[1:]
    uv = 2.0 * np.cross(c, g)
    jac = np.zeros((3, 4))
    jac[:, 0] = uv
    for k in range(3):
        e = np.zeros(3)
        e[k] = 1.0
        ev = 2.0 * np.cross(e, g)
        a = np.zeros(3) if defect == "ek_x_uv_dropped" else np.cross(e, uv)
        b = np.zeros(3) if defect == "c_x_ev_dropped" else np.cross(c, ev)
        jac[:, 1 + k] = -(w * ev + a + b)
    if defect == "col_w_sign_flipped":
        jac[:, 0] = -jac[:, 0]
    for k, name in enumerate(("col_w_zeroed", "col_x_zeroed", "col_y_zeroed", "col_z_zeroed")):
        if defect == name:
            jac[:, k] = 0.0
    if defect == "xyz_transposed":
        jac[:, 1:] = jac[:, 1:].T.copy()
    return jac


def np_imu_update(base, feat, Sig, gyro, acc, gv, av, g, jacobian="numeric", defect=None):
    """The IMU update in plain numpy fp64, independent of the oracle: H by central differences of h(x) ("numeric") or written out
    ("analytic", which accepts one of DEFECTS), K = Sigma H^T S^-1 by numpy.linalg, Joseph form.  Returns dict(mu, Sigma, H, R, S)."""
    base, Sig = np.asarray(base, np.float64), np.asarray(Sig, np.float64)
    feat = np.asarray(feat, np.float64).ravel()
    gyro, acc, g = (np.asarray(a, np.float64) for a in (gyro, acc, g))
    assert defect is None or (defect in DEFECTS and jacobian == "analytic")
    n = Sig.shape[0]
    if defect == "gravity_rotated_one_place":
        g = np.roll(g, 1)
    if defect == "variances_exchanged":
        gv, av = av, gv
    H = np.zeros((6, n))
    if jacobian == "numeric":
        for k in range(BASE):
            d = np.zeros(BASE)
            d[k] = 1e-6
            H[:, k] = (h_imu(base + d, g) - h_imu(base - d, g)) / 2e-6
    else:
        H[0:3, 10:13] = H[0:3, 19:22] = np.eye(3)
        H[3:6, 13:16] = H[3:6, 16:19] = np.eye(3)
        if defect == "bias_columns_exchanged":
            H[:, 16:22] = H[:, [19, 20, 21, 16, 17, 18]]
        H[3:6, 3:7] = -rt_gravity_jacobian(base[3:7], g, defect if defect in JACOBIAN_DEFECTS else None)
    y = np.concatenate([gyro, acc]) - h_imu(base, g)
    if defect == "residual_plus_rtg":
        y[3:] = acc - (base[13:16] + base[16:19] + rot_t(base[3:7], g))
    R = np.diag([gv] * 3 + [av] * 3)
    S = H @ Sig @ H.T + R
    K = Sig @ H.T @ np.linalg.inv(S)
    I_KH = np.eye(n) - K @ H
    Sig2 = I_KH @ Sig @ I_KH.T + K @ R @ K.T
    mu = np.concatenate([base, feat]) + K @ y
    if defect != "quaternion_not_normalised":
        mu[3:7] /= np.linalg.norm(mu[3:7])
    return dict(mu=mu, Sigma=Sig2, H=H, R=R, S=S)


def np_state(out, like):
    """np_imu_update's result in the layout of a filter state."""
    N = like["feat_mu"].shape[0]
    return dict(base_mu=out["mu"][:BASE].copy(), feat_mu=out["mu"][BASE:].reshape(N, 3).copy(), Sigma=out["Sigma"])


def kernel_order_fp32(st, gyro, acc, gv, av, g):
    """imu.hip's order of operations restated in numpy fp32, multiply and add rounded separately (the library is built without
    contraction): rt_gravity; H on its sixteen columns; W = H Sigma on them; S = W H^T + R; its Cholesky; per state row x = Sigma(i, cols) H^T
    and w = H Sigma(cols, i) over ALL sixteen columns (the oracle skips H's zeros), k = x S^-1, T = Sigma(i, cols) - k W,
    G = k R - T H^T, mu + k y; then Sigma - K W + G K^T elementwise, pruned."""
    f = np.float32
    mu = np.concatenate([st["base_mu"], st["feat_mu"].ravel()]).astype(f)
    P = np.asarray(st["Sigma"], f)
    n = P.shape[0]
    gyro, acc, g = (np.asarray(a, f) for a in (gyro, acc, g))
    gv, av = f(gv), f(av)

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f)

    w, c = mu[3], np.array([-mu[4], -mu[5], -mu[6]], f)
    uv = cross(c, g)
    uv = uv + uv
    cu = cross(c, uv)
    rg = (g + w * uv) + cu
    jac = np.zeros((3, 4), f)
    jac[:, 0] = uv
    for k in range(3):
        e = np.zeros(3, f)
        e[k] = 1
        ev = cross(e, g)
        ev = ev + ev
        a, b = cross(e, uv), cross(c, ev)
        jac[:, 1 + k] = -((w * ev + a) + b)
    H = np.zeros((6, 16), f)
    y = np.zeros(6, f)
    for r in range(3):
        H[r, 4 + r] = H[r, 13 + r] = H[3 + r, 7 + r] = H[3 + r, 10 + r] = 1
        H[3 + r, :4] = -jac[r]
        y[r] = gyro[r] - (mu[10 + r] + mu[19 + r])
        y[3 + r] = acc[r] - ((mu[13 + r] + mu[16 + r]) - rg[r])
    Pb = P[np.ix_(COLS, COLS)]
    Wb = np.zeros((6, 16), f)
    for cc in range(16):
        Wb = Wb + H[:, cc:cc + 1] * Pb[cc:cc + 1, :]
    S = np.zeros((6, 6), f)
    for cc in range(16):
        S = S + Wb[:, cc:cc + 1] * H[:, cc][None, :]
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
    pc = P[:, COLS]        # Sigma(i, cols[c])
    pr = P[COLS, :].T      # Sigma(cols[c], i)
    x, wm = np.zeros((n, 6), f), np.zeros((n, 6), f)
    for cc in range(16):
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
    for cc in range(16):
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
    V[~(np.abs(V) > FLUSH)] = 0
    assert V.dtype == f and mu2.dtype == f
    N = st["feat_mu"].shape[0]
    return dict(base_mu=mu2[:BASE].copy(), feat_mu=mu2[BASE:].reshape(N, 3).copy(), Sigma=V)


# ---------------------------------------------------------------------------------------------------------------- inputs
def _f32(st):
    return {k: (v.astype(np.float32) if v.dtype == np.float64 else v.copy()) for k, v in st.items()}


@functools.lru_cache(maxsize=None)
def start(N):
    """(the fp32 start state of N landmarks, the scenario's next frame (z, R, passed) for a camera update from it)."""
    use_threads()
    sc = Scenario(max(N, 1), seed=SEED, dt=DT)
    o = OracleFilter(np.float64)
    frame = None
    if N:
        o.add_new_features(sc.initial_features()[:N])
        fr = list(sc.frames(WARM_FRAMES + 1))
        for z, R, p in fr[:WARM_FRAMES]:
            o.process(sc.dt), o.update(z[:N], R[:N], p[:N])
        z, R, p = fr[WARM_FRAMES]
        frame = (z[:N].copy(), R[:N].copy(), p[:N].copy())
    else:
        o.process(DT)
    st = _f32(o.get_state())
    o.close()
    assert np.isfinite(st["Sigma"]).all()
    return st, frame


def fresh(st):
    return {k: v.copy() for k, v in st.items()}


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(start state with the case's quaternion, gyro, accel, gyro variance, accel variance, gravity), every number an fp32 one."""
    st = fresh(start(case.N)[0])
    st["base_mu"][3:7] = QUATS[case.quat].astype(np.float32)
    g = np.array(GRAVS[case.grav], np.float32)
    gv, av = np.float32(case.var[0]), np.float32(case.var[1])
    b = st["base_mu"]
    if case.reading == "zero":  # exactly zero in the fp32 specification's own arithmetic
        o = OracleFilter(np.float32)
        rg, _ = o.rt_gravity(b[3:7], g)
        o.close()
        gyro = b[10:13] + b[19:22]
        acc = (b[13:16] + b[16:19]) - rg
        assert gyro.dtype == np.float32 and acc.dtype == np.float32
    else:
        h = h_imu(b.astype(np.float64), g.astype(np.float64))
        if case.reading == "large":
            d = np.concatenate(LARGE_OFFSET)
        else:
            rng = np.random.default_rng([case.N, list(QUATS).index(case.quat), list(GRAVS).index(case.grav)])
            d = np.concatenate([rng.normal(0, NOISE[0], 3), rng.normal(0, NOISE[1], 3)])
        z = (h + d).astype(np.float32)
        gyro, acc = z[:3].copy(), z[3:].copy()
    return st, gyro, acc, gv, av, g


def oracle_imu_update(dtype, st, gyro, acc, gv, av, g, dt=None):
    """(process(dt) and) imu_update of the oracle in `dtype` from fp32 inputs."""
    o = OracleFilter(dtype)
    o.set_state(st)
    if dt is not None:
        o.process(dtype(dt))
    o.imu_update(np.asarray(gyro, np.float32).astype(dtype), np.asarray(acc, np.float32).astype(dtype), dtype(np.float32(gv)),
                 dtype(np.float32(av)), np.asarray(g, np.float32).astype(dtype))
    out = o.get_state()
    o.close()
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """(the fp32 oracle's result, the fp64 oracle's result) of a case; left unchanged by everything that reads it."""
    st, gyro, acc, gv, av, g = inputs(case)
    return oracle_imu_update(np.float32, st, gyro, acc, gv, av, g), oracle_imu_update(np.float64, st, gyro, acc, gv, av, g)


# ---------------------------------------------------------------------------------------------------------------- the criterion
QUANTITIES = ("base", "feat", "sig_quat_rows", "sig_base", "sig_base_feat", "sig_feat_base", "sig_feat", "sig_elementwise")


def quantities(st):
    """name -> (measure, values in fp64)."""
    S = np.asarray(st["Sigma"], np.float64)
    return dict(base=("max", np.asarray(st["base_mu"], np.float64)), feat=("max", np.asarray(st["feat_mu"], np.float64)),
                sig_quat_rows=("fro", S[3:7, :]), sig_base=("fro", S[:BASE, :BASE]), sig_base_feat=("fro", S[:BASE, BASE:]),
                sig_feat_base=("fro", S[BASE:, :BASE]), sig_feat=("fro", S[BASE:, BASE:]), sig_elementwise=("max", S))


def _size(measure, a):
    if a.size == 0:
        return 0.0
    return float(np.abs(a).max()) if measure == "max" else float(np.linalg.norm(a))


def errors(got, s64):
    a, b = quantities(got), quantities(s64)
    return {k: _size(a[k][0], a[k][1] - b[k][1]) for k in QUANTITIES}


def tolerances(s32, s64, factor=ACC_FACTOR):
    e32, b = errors(s32, s64), quantities(s64)
    return {k: factor * e32[k] + ULP * _size(*b[k]) for k in QUANTITIES}


def ratios(got, s32, s64, factor=ACC_FACTOR):
    """err / tolerance per quantity (0 for a quantity the case does not have: no landmarks)."""
    e, t = errors(got, s64), tolerances(s32, s64, factor)
    return {k: (e[k] / t[k] if t[k] > 0 else 0.0 if e[k] == 0 else np.inf) for k in QUANTITIES}
