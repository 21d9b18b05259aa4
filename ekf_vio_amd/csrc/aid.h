// ekf_vio_amd/csrc/aid.h — the linear aiding measurement of the base state (include/ekfvio.h, ekfvio_aid_update): the lines of its
// specification, shared by the kernels of aid.hip and the host functions ekfvio_aid_innovation and ekfvio_aid_rows_body_velocity: one set
// of inline functions, compiled for the host and for the device, fp32 without contraction, so that both give the bits of a NumPy
// restatement (tests/_aid.py).  K, the row count, is a template argument wherever a loop bound depends on it: every instance unrolls
// fully and nothing is indexed by a run-time row count.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

constexpr int AID_BASE = 22;     // the state columns H has
constexpr int AID_MAX_ROWS = 6;

// h_0*p[0] + h_1*p[stride] + ... + h_21*p[21 stride]: all 22 terms, ascending, associated to the left
__host__ __device__ inline float aid_dot22(const float* h, const float* p, size_t stride) {
    float v = h[0] * p[0];
    for (int c = 1; c < AID_BASE; c++) v = v + h[c] * p[(size_t)c * stride];
    return v;
}
// R(r, s) of a row-major k x k matrix whose lower triangle alone is read
__host__ __device__ inline float aid_R(const float* R, int k, int r, int s) { return r >= s ? R[r * k + s] : R[s * k + r]; }

// Left-looking Cholesky of the lower triangle of S (row-major K x K) into L's lower triangle.  false at the first pivot that is not finite
// and > 0 (a NaN fails both comparisons); what lies behind it in L is then not written
template <int K>
__host__ __device__ inline bool aid_factor(const float* S, float* L) {
#pragma unroll
    for (int j = 0; j < K; j++) {
        float dd = S[j * K + j];
#pragma unroll
        for (int k = 0; k < j; k++) dd = dd - L[j * K + k] * L[j * K + k];
        if (!(dd > 0.f) || !(dd <= 3.402823466e+38f)) return false;
        L[j * K + j] = sqrtf(dd);
#pragma unroll
        for (int r = j + 1; r < K; r++) {
            float v = S[r * K + j];
#pragma unroll
            for (int k = 0; k < j; k++) v = v - L[r * K + k] * L[j * K + k];
            L[r * K + j] = v / L[j * K + j];
        }
    }
    return true;
}
// e = L^-1 y by forward substitution, d2 = e_0*e_0 + ... + e_{K-1}*e_{K-1}
template <int K>
__host__ __device__ inline float aid_d2(const float* L, const float* y) {
    float e[K];
    float d2 = 0.f;
#pragma unroll
    for (int r = 0; r < K; r++) {
        float v = y[r];
#pragma unroll
        for (int k = 0; k < r; k++) v = v - e[k] * L[r * K + k];
        e[r] = v / L[r * K + r];
        d2 = r == 0 ? e[0] * e[0] : d2 + e[r] * e[r];
    }
    return d2;
}
// (a NaN d2 is rejected by a gate that is on)
__host__ __device__ inline bool aid_accept(bool pivots_ok, float d2, float chi2) { return pivots_ok && (chi2 == 0.f || d2 <= chi2); }

// the gains of one state row: kk = x S^-1 = (x L^-T) L^-1, forward then backward
template <int K>
__host__ __device__ inline void aid_gain_row(const float* x, const float* L, float* kk) {
#pragma unroll
    for (int r = 0; r < K; r++) {
        float v = x[r];
#pragma unroll
        for (int k = 0; k < r; k++) v = v - kk[k] * L[r * K + k];
        kk[r] = v / L[r * K + r];
    }
#pragma unroll
    for (int r = K - 1; r >= 0; r--) {
        float v = kk[r];
#pragma unroll
        for (int k = r + 1; k < K; k++) v = v - kk[k] * L[k * K + r];
        kk[r] = v / L[r * K + r];
    }
}

// The part of the update that needs the 22 x 22 base block of Sigma alone (Pb, column-major with leading dimension ld: P(i,j) = Pb[j ld + i]):
// W = H P on the base columns, A = W H^T (all K x K), S = A + R (lower triangle), y, the factor, d2.  On the device these lines are spread
// over a workgroup's threads (aid_gain_kernel); the host's ekfvio_aid_innovation runs them here.  Returns the pivots' verdict; d2 is a NaN
// where it fails
template <int K>
inline bool aid_innovation(const float* mu, const float* Pb, size_t ld, const float* H, const float* z, const float* R, float* y, float* A,
                           float* S, float* d2) {
    float W[K * AID_BASE], L[K * K];
    for (int r = 0; r < K; r++)
        for (int c = 0; c < AID_BASE; c++) W[r * AID_BASE + c] = aid_dot22(H + r * AID_BASE, Pb + (size_t)c * ld, 1);
    for (int r = 0; r < K; r++)
        for (int s = 0; s < K; s++) {
            A[r * K + s] = aid_dot22(W + r * AID_BASE, H + s * AID_BASE, 1);
            S[r * K + s] = A[r * K + s] + aid_R(R, K, r, s);
        }
    for (int r = 0; r < K; r++) y[r] = z[r] - aid_dot22(H + r * AID_BASE, mu, 1);
    const bool ok = aid_factor<K>(S, L);
    *d2 = ok ? aid_d2<K>(L, y) : NAN;
    return ok;
}

// what the entry points accept: k in 1..6, finite entries, chi2 >= 0, R positive definite (fp64 Cholesky of its lower triangle)
inline bool aid_rows_valid(int k, const float* H, const float* z, const float* R, float chi2) {
    if (k < 1 || k > AID_MAX_ROWS || !H || !z || !R || !(chi2 >= 0.f) || !isfinite(chi2)) return false;
    for (int e = 0; e < k * AID_BASE; e++)
        if (!isfinite(H[e])) return false;
    for (int e = 0; e < k; e++)
        if (!isfinite(z[e])) return false;
    for (int e = 0; e < k * k; e++)
        if (!isfinite(R[e])) return false;
    double L[AID_MAX_ROWS * AID_MAX_ROWS];
    for (int j = 0; j < k; j++) {
        double dd = (double)R[j * k + j];
        for (int c = 0; c < j; c++) dd -= L[j * k + c] * L[j * k + c];
        if (!(dd > 0.0)) return false;
        L[j * k + j] = sqrt(dd);
        for (int r = j + 1; r < k; r++) {
            double v = (double)R[r * k + j];
            for (int c = 0; c < j; c++) v -= L[r * k + c] * L[j * k + c];
            L[r * k + j] = v / L[j * k + j];
        }
    }
    return true;
}

// The rows of a velocity measured in a vehicle frame, z = M (vel + omega x p) with M = R_cv^T (M[r][j] = R_cv[3 j + r]) and p = p_cv:
//     H(r, 7+j)  = M[r][j]
//     H(r, 10+j) = (M[r][0]*C[0][j] + M[r][1]*C[1][j]) + M[r][2]*C[2][j],   C = d(omega x p)/d omega = [[0, p_2, -p_1], [-p_2, 0, p_0], [p_1, -p_0, 0]]
// and zero elsewhere.  H: 3 x 22 row-major
inline void aid_body_velocity_rows(const float* R_cv, const float* p, float* H) {
    const float C[9] = {0.f, p[2], -p[1], -p[2], 0.f, p[0], p[1], -p[0], 0.f};
    for (int e = 0; e < 3 * AID_BASE; e++) H[e] = 0.f;
    for (int r = 0; r < 3; r++) {
        const float m0 = R_cv[r], m1 = R_cv[3 + r], m2 = R_cv[6 + r];
        float* h = H + r * AID_BASE;
        h[7] = m0, h[8] = m1, h[9] = m2;
        for (int j = 0; j < 3; j++) h[10 + j] = (m0 * C[j] + m1 * C[3 + j]) + m2 * C[6 + j];
    }
}
