"""Covariances of the published outputs (include/ekfvio.h, ekfvio_get_odometry_covariance / ekfvio_get_points_covariance), the part that
needs no GPU: the two Jacobians of the specification are held to what they are Jacobians OF, the float32 restatement the device is held
to (tests/_covout.py) is held to an fp64 evaluation within a derived bound, and ekfvio_rotation_error_jacobian -- a host function that
compiles the inline function the kernels compile -- gives the restatement's bits."""
import ctypes as C

import numpy as np

from ekf_vio_amd import capi, rotation_error_jacobian

import _covout as co

U = 2.0 ** -24  # unit roundoff of fp32


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def rotmat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def unit_quaternions(n, seed):
    q = np.random.default_rng(seed).standard_normal((n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def random_state(N, seed):
    """A dense SPD Sigma with eigenvalues >= 0.1, a unit quaternion away from the identity, rho in [0.2, 2]."""
    rng = np.random.default_rng(seed)
    n = co.BASE + 3 * N
    B = rng.standard_normal((n, n))
    Sigma = (B @ B.T / n + 0.1 * np.eye(n)).astype(np.float32)
    base = rng.standard_normal(co.BASE).astype(np.float32)
    q = rng.standard_normal(4)
    base[3:7] = (q / np.linalg.norm(q)).astype(np.float32)
    feat = np.stack([rng.uniform(-1, 1, N), rng.uniform(-1, 1, N), rng.uniform(0.2, 2.0, N)], axis=1).astype(np.float32)
    return base, feat, Sigma


def test_J_is_the_jacobian_of_the_world_frame_rotation_error():
    """dtheta = 2 vec(q_true (x) q*) for q_true = (q + dq) / |q + dq|: J dq agrees to second order (|dq| ~ 1e-6: <= 1e-9), J q = 0 (the norm
    direction drops out), and the dtheta it measures is the one with R(q_true) = (I + [dtheta]x) R(q): world axes, left perturbation."""
    rng = np.random.default_rng(1)
    worst_lin, worst_null, worst_rot = 0.0, 0.0, 0.0
    for q in unit_quaternions(100, 0):
        J = co.jacobian64(q)
        dq = rng.standard_normal(4)
        dq *= 1e-6 / np.linalg.norm(dq)
        qt = (q + dq) / np.linalg.norm(q + dq)
        qc = q * np.array([1, -1, -1, -1])
        dtheta = 2.0 * qmul(qt, qc)[1:]
        worst_lin = max(worst_lin, np.abs(dtheta - J @ dq).max())
        worst_null = max(worst_null, np.abs(J @ q).max())
        # the convention: a rotation by a small dtheta about WORLD axes in front of q
        th = rng.standard_normal(3) * 1e-6
        qt = qmul(np.concatenate([[1.0], th / 2]), q)
        qt /= np.linalg.norm(qt)
        worst_rot = max(worst_rot, np.abs(rotmat(qt) - (np.eye(3) + skew(th)) @ rotmat(q)).max(), np.abs(J @ (qt - q) - th).max())
    print("J dq against 2 vec(.): %.3g   J q: %.3g   R(q_true) against (I + [dtheta]x) R(q): %.3g" % (worst_lin, worst_null, worst_rot))
    assert worst_lin <= 1e-9 and worst_null <= 1e-15 and worst_rot <= 1e-9


def test_J_of_the_restatement_is_that_J_and_the_identity_attitude_gives_four_sigma():
    for q in unit_quaternions(20, 2).astype(np.float32):
        assert np.array_equal(co.jacobian32(q), co.jacobian64(q.astype(np.float64)).astype(np.float32))  # doubling and negation are exact
    base, feat, Sigma = random_state(2, 3)
    base[3:7] = (1, 0, 0, 0)
    C = co.pose_cov32(base, Sigma)
    S = co.sym_lower64(Sigma)
    assert np.array_equal(C[3:, 3:], (4.0 * S[4:7, 4:7]).astype(np.float32))  # exact: every other term is an exact zero
    assert np.array_equal(C[:3, :3], S[:3, :3].astype(np.float32)) and np.array_equal(C[3:, :3], (2.0 * S[4:7, :3]).astype(np.float32))


def test_Jl_is_the_jacobian_of_the_camera_frame_point():
    """Central differences of (u/rho, v/rho, 1/rho) in fp64 with h = 1e-6: truncation h^2/6 |f'''| <= 1e-12 |u| / rho^4 <= 6.3e-10 and
    roundoff 2^-53 |f| / h <= 6e-10 at rho >= 0.2, |u| <= 1: within 1e-8.  The float32 entries the specification forms (z, -(x z), -(y z),
    -(z z): at most four roundings each) are then within 4 * 2^-24 relative of it."""
    f = lambda p: np.array([p[0] / p[2], p[1] / p[2], 1.0 / p[2]])
    _, feat, _ = random_state(50, 4)
    worst = 0.0
    for ft in feat:
        p = ft.astype(np.float64)
        exact = np.array([[1 / p[2], 0, -p[0] / p[2] ** 2], [0, 1 / p[2], -p[1] / p[2] ** 2], [0, 0, -1 / p[2] ** 2]])
        num = np.stack([(f(p + 1e-6 * e) - f(p - 1e-6 * e)) / 2e-6 for e in np.eye(3)], axis=1)
        worst = max(worst, np.abs(num - exact).max())
        assert (np.abs(co.point_Jl64(ft) - exact) <= 4 * U * np.abs(exact)).all()
    print("Jl against central differences: %.3g" % worst)
    assert worst <= 1e-8


def test_restatement_is_within_the_running_error_bound_of_fp64_symmetric_and_psd():
    """Two nested sums of at most seven unfused terms round at most 16 times: |C32 - C64| <= 16 * 2^-24 * (|A| |S| |A|^T), elementwise, and the
    same form with |Jl|, |L|.  The outputs are exactly symmetric, and the pose covariance of an SPD Sigma is positive semidefinite within
    that bound (Weyl: its smallest eigenvalue is no further below that of the fp64 product than the bound's Frobenius norm)."""
    for seed, N in [(5, 0), (6, 1), (7, 5)]:
        base, feat, Sigma = random_state(N, seed)
        pose, twist, pts = co.covariances32(base, feat, Sigma)
        C64, mag = co.pose_cov64(base, Sigma)
        err = np.abs(pose.astype(np.float64) - C64)
        print("pose: worst error / bound %.3f" % (err / (16 * U * mag)).max())
        assert (err <= 16 * U * mag).all()
        assert np.array_equal(pose, pose.T) and np.array_equal(twist, twist.T)
        assert np.array_equal(twist, co.sym_lower64(Sigma)[7:13, 7:13].astype(np.float32))
        assert np.linalg.eigvalsh(C64).min() > 0
        assert np.linalg.eigvalsh(pose.astype(np.float64)).min() >= -np.linalg.norm(16 * U * mag)
        P64, pmag = co.points_cov64(feat, Sigma)
        assert pts.shape == (N, 3, 3)
        if N:
            perr = np.abs(pts.astype(np.float64) - P64)
            print("landmarks: worst error / bound %.3f" % (perr / (16 * U * pmag)).max())
            assert (perr <= 16 * U * pmag).all()
            assert np.array_equal(pts, pts.transpose(0, 2, 1))


def test_a_fresh_landmark_gets_Jl_diag_Jl_transposed():
    """addNewFeatures leaves L = diag(hv, hv, dv): the lines of the specification give Jl diag Jl^T by themselves."""
    base, feat, Sigma = random_state(2, 8)
    s = co.BASE + 3
    Sigma[s:s + 3, :] = 0
    Sigma[:, s:s + 3] = 0
    Sigma[s, s] = Sigma[s + 1, s + 1] = 1e-5
    Sigma[s + 2, s + 2] = 100.0
    got = co.points_cov32(feat, Sigma)[1].astype(np.float64)
    Jl = co.point_Jl64(feat[1])
    want = Jl @ np.diag(Sigma[[s, s + 1, s + 2], [s, s + 1, s + 2]].astype(np.float64)) @ Jl.T
    assert (np.abs(got - want) <= 16 * U * np.abs(want)).all()


def test_host_jacobian_has_the_bits_of_the_restatement():
    lib = capi.load()
    for q in unit_quaternions(50, 9).astype(np.float32):
        assert np.array_equal(rotation_error_jacobian(q), co.jacobian32(q))
    q, J = np.zeros(4, np.float32), np.zeros(12, np.float32)
    fp = C.POINTER(C.c_float)
    assert lib.ekfvio_rotation_error_jacobian(None, J.ctypes.data_as(fp)) == capi.EINVAL
    assert lib.ekfvio_rotation_error_jacobian(q.ctypes.data_as(fp), None) == capi.EINVAL


def test_null_handle_is_rejected():
    lib = capi.load()
    buf = np.zeros(36, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    assert lib.ekfvio_get_odometry_covariance(None, buf, buf) == capi.EINVAL
    assert lib.ekfvio_get_points_covariance(None, buf) == capi.EINVAL
    assert lib.ekfvio_set_output_covariance(None, 1) == capi.EINVAL
    assert lib.ekfvio_set_output_covariance(None, 0) == capi.EINVAL
