"""NumPy restatement of the covariances of the published outputs (include/ekfvio.h, "covariances of the published outputs").

The float32 functions are the header's lines, one NumPy float32 operation per line's operation, in its order: what the device is held
to bit for bit.  The fp64 functions evaluate A S A^T and Jl L Jl^T from the symmetrised lower triangle, with the elementwise magnitude
|A| |S| |A|^T beside them for the running-error bound of tests/test_covout_cpu.py.

Sigma is [row, col] (TightlyCoupledEKF.Sigma); S(i,j) is its LOWER-triangle element Sigma[max(i,j), min(i,j)].
"""
import numpy as np

F = np.float32
BASE = 22


def S_of(Sigma):
    Sg = np.asarray(Sigma, np.float32)
    return lambda i, j: Sg[max(i, j), min(i, j)]


def jacobian32(q):
    """J = 2 [[-qx, qw, -qz, qy], [-qy, qz, qw, -qx], [-qz, -qy, qx, qw]], columns w, x, y, z."""
    w, x, y, z = (F(v) for v in np.asarray(q, np.float32).reshape(4))
    two = F(2.0)
    return np.array([[two * -x, two * w, two * -z, two * y],
                     [two * -y, two * z, two * w, two * -x],
                     [two * -z, two * -y, two * x, two * w]], np.float32)


def jacobian64(q):
    """The same J in fp64, for a quaternion given in fp64."""
    w, x, y, z = np.asarray(q, np.float64).reshape(4)
    return 2.0 * np.array([[-x, w, -z, y], [-y, z, w, -x], [-z, -y, x, w]])


def pose_cov32(base_mu, Sigma):
    S = S_of(Sigma)
    J = jacobian32(np.asarray(base_mu, np.float32)[3:7])
    T = np.zeros((6, 7), np.float32)
    for j in range(7):
        for r in range(3):
            T[r, j] = S(r, j)  # a copy, not a product
            T[3 + r, j] = ((J[r, 0] * S(3, j) + J[r, 1] * S(4, j)) + J[r, 2] * S(5, j)) + J[r, 3] * S(6, j)
    C = np.zeros((6, 6), np.float32)
    for a in range(6):
        for b in range(a + 1):
            if a < 3:
                v = S(a, b)
            elif b < 3:
                v = T[a, b]
            else:
                v = ((T[a, 3] * J[b - 3, 0] + T[a, 4] * J[b - 3, 1]) + T[a, 5] * J[b - 3, 2]) + T[a, 6] * J[b - 3, 3]
            C[a, b] = C[b, a] = v
    return C


def twist_cov32(Sigma):
    S = S_of(Sigma)
    C = np.zeros((6, 6), np.float32)
    for a in range(6):
        for b in range(a + 1):
            C[a, b] = C[b, a] = S(7 + a, 7 + b)
    return C


def point_jacobian32(feat):
    """(z, jx, jy, jz) of Jl = [[z, 0, jx], [0, z, jy], [0, 0, jz]] for one landmark (u, v, rho)."""
    u, v, rho = (F(t) for t in feat)
    z = F(1.0 / np.float64(rho))
    x, y = u * z, v * z
    return z, -(x * z), -(y * z), -(z * z)


def points_cov32(feat_mu, Sigma):
    feat_mu = np.asarray(feat_mu, np.float32).reshape(-1, 3)
    S = S_of(Sigma)
    out = np.zeros((feat_mu.shape[0], 3, 3), np.float32)
    with np.errstate(all="ignore"):
        for i, ft in enumerate(feat_mu):
            s = BASE + 3 * i
            z, jx, jy, jz = point_jacobian32(ft)
            L = lambda a, b: S(s + a, s + b)
            M00, M02 = z * L(0, 0) + jx * L(2, 0), z * L(0, 2) + jx * L(2, 2)
            M10, M11, M12 = z * L(1, 0) + jy * L(2, 0), z * L(1, 1) + jy * L(2, 1), z * L(1, 2) + jy * L(2, 2)
            M20, M21, M22 = jz * L(2, 0), jz * L(2, 1), jz * L(2, 2)
            C = out[i]
            C[0, 0] = M00 * z + M02 * jx
            C[1, 0] = C[0, 1] = M10 * z + M12 * jx
            C[1, 1] = M11 * z + M12 * jy
            C[2, 0] = C[0, 2] = M20 * z + M22 * jx
            C[2, 1] = C[1, 2] = M21 * z + M22 * jy
            C[2, 2] = M22 * jz
    return out


def covariances32(base_mu, feat_mu, Sigma):
    """(pose 6x6, twist 6x6, landmarks N x 3 x 3) from a state as TightlyCoupledEKF.get_state() returns it."""
    return pose_cov32(base_mu, Sigma), twist_cov32(Sigma), points_cov32(feat_mu, Sigma)


# ---- fp64 evaluation from the same float32 inputs (symmetrised lower triangle) -------------------------------------------------------
def sym_lower64(Sigma):
    L = np.tril(np.asarray(Sigma, np.float32).astype(np.float64))
    return L + np.tril(L, -1).T


def pose_A64(base_mu):
    A = np.zeros((6, 7))
    A[:3, :3] = np.eye(3)
    A[3:, 3:] = jacobian32(np.asarray(base_mu, np.float32)[3:7]).astype(np.float64)  # (doubling and negation are exact)
    return A


def pose_cov64(base_mu, Sigma):
    """(C, magnitude): A S A^T in fp64 and |A| |S| |A|^T."""
    A, S = pose_A64(base_mu), sym_lower64(Sigma)[:7, :7]
    return A @ S @ A.T, np.abs(A) @ np.abs(S) @ np.abs(A).T


def point_Jl64(feat):
    """Jl from the float32 values z, jx, jy, jz the specification forms (their own rounding belongs to the Jacobian, not to the product)."""
    z, jx, jy, jz = (np.float64(t) for t in point_jacobian32(feat))
    return np.array([[z, 0, jx], [0, z, jy], [0, 0, jz]])


def points_cov64(feat_mu, Sigma):
    feat_mu = np.asarray(feat_mu, np.float32).reshape(-1, 3)
    S = sym_lower64(Sigma)
    C, mag = np.zeros((feat_mu.shape[0], 3, 3)), np.zeros((feat_mu.shape[0], 3, 3))
    for i, ft in enumerate(feat_mu):
        s = BASE + 3 * i
        Jl, L = point_Jl64(ft), S[s:s + 3, s:s + 3]
        C[i], mag[i] = Jl @ L @ Jl.T, np.abs(Jl) @ np.abs(L) @ np.abs(Jl).T
    return C, mag
