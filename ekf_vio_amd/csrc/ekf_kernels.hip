// ekf_vio_amd/csrc/ekf_kernels.hip — process model, finite-difference linearisation,
// structured covariance propagation and the gather/scatter kernels of the update.
//
// Reference: include/ekf_vio/TightlyCoupledEKF.cpp — process :96-121, Q :123-174, FD
// Jacobian :176-325, convolveBaseState :328-395, convolveFeature :397-460, update
// bookkeeping :486-541, residual :554-555, mean update :600-620.
//
// This translation unit is compiled with -ffp-contract=off and evaluates every expression
// in the reference's operation order (including the places where a double literal makes the
// reference compute in double), so the Jacobian blocks and propagated means agree with an
// x86-64 build of the same formulas to the last bit wherever the math library does.
#include <algorithm>
#include <utility>

#include "common.h"

namespace {

#include "motion_model.inc"

// ---------------------------------------------------------------------------------------
// numericallyLinearizeProcess + mean propagation in one launch.
// Workgroups 0 .. ceil(N/8)-1: 8 landmarks each, 32 lanes per landmark.  Every workgroup
// first evaluates the 19 base-state variants (unperturbed + 9 columns x {+,-}) the landmark
// rows need into LDS; then lane e < 25 of a landmark evaluates ONE motion (18 base
// perturbations, 6 own perturbations, the propagated mean) and the finite differences are
// formed through LDS.  The last workgroup produces the 22x22 base block A (32 evaluations of
// convolveBaseState on 32 lanes) and the propagated base mean.
// ---------------------------------------------------------------------------------------
// Body of the bookkeeping (formFeatureMeasurementMap :634-661 and the per-landmark loop of :492-530) for one
// workgroup of NT threads.  zrow receives the measured coordinate of every measurement row (the residual
// z - H mu is formed by gather_kernel, once the propagated mean exists), so this depends only on the frame's
// measurements: it can run as an extra workgroup of the linearisation launch (BookArgs) or on its own.
// EFF (gate_bookkeeping_kernel): the flags are the frame's effective ones, a.pass_eff, which the same thread wrote for its landmarks.
template <int NT, bool EFF = false>
__device__ __forceinline__ void bookkeeping_body(const BookArgs& a) {
    __shared__ int s_cnt[32];
    __shared__ int s_total;
    const int tid = threadIdx.x;
    const int N = a.N, m_pad = a.m_pad;
    const float* z = a.z;
    const float* R = a.R;
    const uint8_t* pass = a.pass;
    if (a.frame_counter) {
        const int fi = *a.frame_counter;
        z += (size_t)fi * 2 * N;
        R += (size_t)fi * 4 * N;
        pass += (size_t)fi * N;
    }
    if (EFF) pass = a.pass_eff;
    const int per = (N + NT - 1) / NT;
    const int lo = tid * per;
    const int hi = min(N, lo + per);
    int c = 0;
    for (int i = lo; i < hi; i++) c += pass[i] ? 1 : 0;
    // exclusive scan of the NT per-thread counts: shuffle scan inside each wavefront, then
    // the wavefront totals are scanned by wavefront 0 (two barriers in all)
    const int lane = tid & 63, wv = tid >> 6;
    constexpr int NW = NT / 64;
    int incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    if (lane == 63) s_cnt[wv] = incl;
    __syncthreads();
    if (wv == 0) {
        int t = (lane < NW) ? s_cnt[lane] : 0;
        int ti = t;
#pragma unroll
        for (int off = 1; off < NW; off <<= 1) {
            const int v = __shfl_up(ti, off, 64);
            if (lane >= off) ti += v;
        }
        if (lane < NW) s_cnt[16 + lane] = ti - t;  // exclusive prefix of the wavefront totals
        if (lane == NW - 1) s_total = ti;
    }
    __syncthreads();
    int base = s_cnt[16 + wv] + incl - c;
    for (int i = lo; i < hi; i++) {
        if (pass[i]) {
            const int r = 2 * base;
            const int s = EKF_BASE + 3 * i;
            a.last_klt[2 * i] = z[2 * i];
            a.last_klt[2 * i + 1] = z[2 * i + 1];
            a.idx[r] = s;
            a.idx[r + 1] = s + 1;
            a.zrow[r] = z[2 * i];
            a.zrow[r + 1] = z[2 * i + 1];
            // Rm[2c] = R(c,c), Rm[2c+1] = R(c^1,c) (the off-diagonal element of column c);
            // input is a column-major 2x2: [cov(0,0), cov(1,0), cov(0,1), cov(1,1)]
            a.Rm[2 * r] = R[4 * i + 0];
            a.Rm[2 * r + 1] = R[4 * i + 1];
            a.Rm[2 * r + 2] = R[4 * i + 3];
            a.Rm[2 * r + 3] = R[4 * i + 2];
            a.inv_idx[s] = r;
            a.inv_idx[s + 1] = r + 1;
            a.inv_idx[s + 2] = -1;
            base++;
        } else {
            a.del_flag[i] = 1;
            a.inv_idx[EKF_BASE + 3 * i] = a.inv_idx[EKF_BASE + 3 * i + 1] = a.inv_idx[EKF_BASE + 3 * i + 2] = -1;
        }
    }
    __syncthreads();
    const int m = 2 * s_total;
    if (tid == 0 && a.m_out) *a.m_out = m;
    for (int r = m + tid; r < m_pad; r += NT) {
        a.idx[r] = -1;
        a.zrow[r] = 0.f;
        a.Rm[2 * r] = 0.f;
        a.Rm[2 * r + 1] = 0.f;
    }
    if (tid <= EKF_BASE) a.inv_idx[tid == EKF_BASE ? EKF_BASE + 3 * N : tid] = -1;  // base state and the K*y column
}

__global__ __launch_bounds__(256) void linearize_kernel(const float* __restrict__ mu, int N, float dt, float* FA,
                                                        float* FB, float* FD, float* mu_next, BookArgs book) {
    // device-resident sequences: the measurement bookkeeping of the coming update rides along as one more
    // workgroup (it does not depend on the propagated state)
    if (book.enabled && blockIdx.x == gridDim.x - 1) {
        bookkeeping_body<256>(book);
        return;
    }
    const int base_block = (int)gridDim.x - 1 - (book.enabled ? 1 : 0);
    __shared__ LinLds l;
    linearize_block([mu](int e) { return mu[e]; }, N, dt, FA, FB, FD, mu_next, (int)blockIdx.x, base_block, l, (int)threadIdx.x);
}

// Scatter the Jacobian blocks into a dense n x n matrix (column-major, ld), zero elsewhere.
__global__ void build_dense_F_kernel(const float* FA, const float* FB, const float* FD, int N, int n, int ld, float* F) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int j = blockIdx.y;
    if (i >= ld || j >= ld) return;
    float v = 0.f;
    if (i < n && j < n) {
        if (i < EKF_BASE) {
            if (j < EKF_BASE) v = FA[j * EKF_BASE + i];
        } else {
            int f = (i - EKF_BASE) / 3, r = (i - EKF_BASE) % 3;
            if (j >= 7 && j <= 15)
                v = FB[(size_t)f * 27 + (j - 7) * 3 + r];
            else if (j >= EKF_BASE && (j - EKF_BASE) / 3 == f)
                v = FD[(size_t)f * 9 + ((j - EKF_BASE) % 3) * 3 + r];
        }
    }
    F[(size_t)j * ld + i] = v;
}

// ---------------------------------------------------------------------------------------
// Structured covariance propagation.  F = [[A 0],[B D]] with B non-zero only in state
// columns 7..15 and D block-diagonal 3x3, so
//   X = F*P      : row i<22 : sum_{k<22} A(i,k) P(k,j);  landmark row: 9 + 3 terms
//   P'= X*F^T + Q: col j<22 : sum_{k<22} X(i,k) A(j,k);  landmark col: 9 + 3 terms
// Terms are accumulated in ascending state index with separate multiply and add, i.e. the
// order of the reference's sparse products (and of the dense oracle, whose extra terms are
// exact zeros).
// ---------------------------------------------------------------------------------------
__device__ inline float process_noise(int i, float dt) {
    // generateProcessNoise (:123-174)
    if (i < 7) return (float)(0.0001 * (double)dt);
    if (i < 10) return (float)(0.01 * (double)dt);
    if (i < 16) return 5 * dt;
    if (i < 22) return (float)(0.001 * (double)dt);
    return (float)(0.0001 * (double)dt);
}

// ---------------------------------------------------------------------------------------
// Fused structured propagation  P' = F P F^T + Q  in ONE pass (out of place).
// Because F = [[A 0],[B D]], the 3x3 block of P' for the landmark pair (f,g) depends only on
// the 12x12 sub-block P[{7..15} U own(f), {7..15} U own(g)], so a workgroup owning 16x16
// landmark pairs stages the shared parts (9x9 base block, 9x3 / 3x9 strips, Jacobian blocks)
// in LDS and every thread finishes one 3x3 block with the intermediate X = F P kept in
// registers.  Base rows / columns are handled by extra workgroups of the same launch, one
// thread per element.  Every sum runs in ascending state index with separate multiply and
// add (X = F*P first, then X*F^T), i.e. the order of the reference's sparse products.
// ---------------------------------------------------------------------------------------
// ---- the pieces of numericallyLinearizeProcess (:176-325) as device functions, shared by linearize_kernel's
// formulation (one motion per lane) and by the propagation kernel when it linearises in place (LIN = true) ----
// Derivative column e of landmark (u, v, rho): e = 0..8 -> d/d(base state 7+e) (a column of B, :223-253),
// e = 9..11 -> d/d(own component e-9) (a column of D, :262-321).  bm[0] is the unperturbed base motion,
// bm[1+2c] / bm[2+2c] the ones with base state 7+c at +delta / -delta.
__device__ __forceinline__ void lin_column(const BaseMotion* bm, float u, float v, float rho, int e, float td, float out[3]) {
    V3 hi, lo;
    if (e < 9) {
        hi = convolve_feature(bm[1 + 2 * e], u, v, rho);
        lo = convolve_feature(bm[2 + 2 * e], u, v, rho);
    } else {
        const int c = e - 9;
        float t0 = u, t1 = v, t2 = rho;
        if (c == 0) t0 = plus_delta(t0);
        if (c == 1) t1 = plus_delta(t1);
        if (c == 2) t2 = plus_delta(t2);
        hi = convolve_feature(bm[0], t0, t1, t2);
        if (c == 0) t0 = minus_2delta(t0);
        if (c == 1) t1 = minus_2delta(t1);
        if (c == 2) t2 = minus_2delta(t2);
        lo = convolve_feature(bm[0], t0, t1, t2);
    }
    out[0] = (hi.x - lo.x) / td;
    out[1] = (hi.y - lo.y) / td;
    out[2] = (hi.z - lo.z) / td;
}
// base motion variant v of the 19 the landmark rows need (0: unperturbed, 1+2c: column 7+c plus, 2+2c: minus)
__device__ __forceinline__ BaseMotion lin_base_motion(const float* s_base, int v, float dt) {
    float t[EKF_BASE];
#pragma unroll
    for (int i = 0; i < EKF_BASE; i++) t[i] = s_base[i];
    if (v > 0) {
        const int c = 7 + (v - 1) / 2;
#pragma unroll
        for (int i = 7; i < 16; i++) {
            if (i == c) {
                t[i] = plus_delta(t[i]);
                if (((v - 1) & 1) == 1) t[i] = minus_2delta(t[i]);
            }
        }
    }
    return base_motion(t, dt);
}
// convolveBaseState at test point q (column q>>1 at +delta for even q, -delta for odd q) -> out[22]
__device__ __forceinline__ void lin_base_test_point(const float* s_base, int q, float dt, float* out) {
    const int j = q >> 1;
    float t[EKF_BASE], o[EKF_BASE];
#pragma unroll
    for (int i = 0; i < EKF_BASE; i++) t[i] = (i == j) ? plus_delta(s_base[i]) : s_base[i];
    if (q & 1) {
#pragma unroll
        for (int i = 0; i < EKF_BASE; i++) t[i] = (i == j) ? minus_2delta(t[i]) : t[i];
    }
    convolve_base(t, dt, o);
#pragma unroll
    for (int i = 0; i < EKF_BASE; i++) out[i] = o[i];
}

#define PT PREDICT_PT  // landmarks per tile side (landmark x landmark tiles; plan.h)
#define PC PREDICT_PC  // landmarks per base-row / base-column workgroup (3*PC <= 64)

__device__ __forceinline__ float predict_finish(float acc, int i, int j, float dt) {
    if (i == j) acc = acc + process_noise(i, dt);
    return (fabsf(acc) > EKF_FLUSH_THRESH) ? acc : 0.f;
}

// grid.x = tiles_side^2 landmark tiles + (1 + chunks) base-row workgroups + chunks base-column workgroups
//          (+ 1 bookkeeping workgroup with LIN and book.enabled)
// LIN = true: process(dt) in ONE launch.  Every workgroup forms the Jacobian blocks it needs itself, with the device
// functions linearize_kernel uses (same values, same bits) and straight into LDS: a landmark tile its 2 x 16 B and D
// blocks (384 derivative columns over 256 threads), a base workgroup A (and the B, D of its three landmarks).  The
// propagated mean is written by the diagonal tiles (landmarks) and base workgroup 0; the coming update's measurement
// bookkeeping rides along as one more workgroup.  The redundant arithmetic (each landmark's columns are formed by
// 2 * tiles_side workgroups) is ~1 % of an MI355X-microsecond; what it buys is a kernel boundary and a trip through HBM.
template <bool LIN>
__global__ __launch_bounds__(256) void predict_fused_kernel(const float* __restrict__ P, int ld, int N, int n,
                                                            const float* __restrict__ FA, const float* __restrict__ FB,
                                                            const float* __restrict__ FD, float dt,
                                                            float* __restrict__ Pout, int tiles_side, int chunks,
                                                            const float* __restrict__ mu, float* __restrict__ mu_next, BookArgs book,
                                                            long long* dbg) {
    const int tid = threadIdx.x;
    const int ntile = tiles_side * tiles_side;
    // diagnostic phase stamps (scripts/predict_stamps.py; dbg is null in production): one diagonal tile, one off-diagonal
    // tile, base workgroup 0, one base-row and one base-column workgroup
#define PSTAMP_(slot)                                                                                               \
    do {                                                                                                            \
        if (dbg && tid == 0) {                                                                                      \
            const int b_ = (int)blockIdx.x;                                                                         \
            const int w_ = b_ == 0 ? 0 : b_ == 1 ? 1 : b_ == ntile ? 2 : b_ == ntile + 1 ? 3 : b_ == ntile + chunks + 1 ? 4 : -1; \
            if (w_ >= 0) dbg[900 + 8 * w_ + (slot)] = (long long)__builtin_amdgcn_s_memtime();                      \
        }                                                                                                           \
    } while (0)
    PSTAMP_(0);
    __shared__ float sm[4096];
    __shared__ float s_base[EKF_BASE];
    __shared__ BaseMotion s_bm[19];
    const float td = two_delta();
    if (book.enabled && blockIdx.x == gridDim.x - 1) {  // (LIN, or a step whose linearisation ran inside the previous update's last GEMM)
        bookkeeping_body<256>(book);
        return;
    }
    if (LIN) {
        if (tid < EKF_BASE) s_base[tid] = mu[tid];
    }
    if ((int)blockIdx.x < ntile) {
        float* sPbb = sm;                 // [81]      P(7+a, 7+b) at a*9+b
        float* sPbg = sm + 96;            // [PT][27]  P(7+a, 22+3g+s) at a*3+s
        float* sPfb = sPbg + PT * 27;     // [PT][27]  P(22+3f+q, 7+b) at q*9+b
        float* sBf = sPfb + PT * 27;      // [PT][27]  B_f(r,c) at c*3+r
        float* sBg = sBf + PT * 27;
        float* sDf = sBg + PT * 27;       // [PT][9]   D_f(r,q) at q*3+r
        float* sDg = sDf + PT * 9;
        float* sXb = sDg + PT * 9;        // [PT][27]  X(22+3f+r, 7+b) at r*9+b
        const int tI = blockIdx.x / tiles_side, tJ = blockIdx.x % tiles_side;
        const int f0 = tI * PT, g0 = tJ * PT;
        if (tid < 81) sPbb[tid] = P[(size_t)(7 + tid % 9) * ld + 7 + tid / 9];
        // LIN: the two derivative columns this thread forms: task = side*192 + landmark*12 + column, tasks tid and
        // tid + 256 (< 384); on the diagonal tiles threads 128..143 propagate the landmarks' means in their second slot
        float lu[2] = {0.f, 0.f}, lv[2] = {0.f, 0.f}, lrho[2] = {1.f, 1.f};
        if (LIN) {
#pragma unroll
            for (int sl = 0; sl < 2; sl++) {
                const int task = tid + 256 * sl;
                int lmk = -1;
                if (task < 384) lmk = ((task >= 192) ? g0 : f0) + (task % 192) / 12;
                else if (tI == tJ && tid >= 128 && tid < 128 + PT) lmk = f0 + tid - 128;
                if (lmk >= 0 && lmk < N) {
                    lu[sl] = mu[EKF_BASE + 3 * lmk];
                    lv[sl] = mu[EKF_BASE + 3 * lmk + 1];
                    lrho[sl] = mu[EKF_BASE + 3 * lmk + 2];
                }
            }
        }
#ifndef EKF_PREDICT_LIN_TWO_BARRIERS
        if (LIN) {
            // the staged operands are requested first; while they fly, 19 threads of the last wavefront form the base
            // motions from the base state read straight from global memory (no LDS hop, no extra barrier)
            float pg[2], pf[2];
#pragma unroll
            for (int it = 0; it < 2; it++) {
                const int e = tid + 256 * it;
                const int l = e / 27, w = e % 27;
                const int f = f0 + l, g = g0 + l;
                const bool in = e < PT * 27;
                pg[it] = (in && g < N) ? P[(size_t)(EKF_BASE + 3 * g + w % 3) * ld + 7 + w / 3] : 0.f;
                pf[it] = (in && f < N) ? P[(size_t)(7 + w % 9) * ld + EKF_BASE + 3 * f + w / 9] : 0.f;
            }
            if (tid >= 192 && tid < 192 + 19) {
                float b[EKF_BASE];
#pragma unroll
                for (int i = 0; i < EKF_BASE; i++) b[i] = mu[i];
                s_bm[tid - 192] = lin_base_motion(b, tid - 192, dt);
            }
#pragma unroll
            for (int it = 0; it < 2; it++) {
                const int e = tid + 256 * it;
                if (e < PT * 27) {
                    sPbg[e] = pg[it];
                    sPfb[e] = pf[it];
                }
            }
        } else
#endif
        for (int e = tid; e < PT * 27; e += 256) {
            const int l = e / 27, w = e % 27;
            const int f = f0 + l, g = g0 + l;
            sPbg[e] = (g < N) ? P[(size_t)(EKF_BASE + 3 * g + w % 3) * ld + 7 + w / 3] : 0.f;
            sPfb[e] = (f < N) ? P[(size_t)(7 + w % 9) * ld + EKF_BASE + 3 * f + w / 9] : 0.f;
            if (!LIN) {
                sBf[e] = (f < N) ? FB[(size_t)f * 27 + w] : 0.f;
                sBg[e] = (g < N) ? FB[(size_t)g * 27 + w] : 0.f;
            }
        }
        if (!LIN) {
            for (int e = tid; e < PT * 9; e += 256) {
                const int l = e / 9, w = e % 9;
                sDf[e] = (f0 + l < N) ? FD[(size_t)(f0 + l) * 9 + w] : 0.f;
                sDg[e] = (g0 + l < N) ? FD[(size_t)(g0 + l) * 9 + w] : 0.f;
            }
        }
        __syncthreads();
        PSTAMP_(1);
        if (LIN) {
#ifdef EKF_PREDICT_LIN_TWO_BARRIERS
            if (tid < 19) s_bm[tid] = lin_base_motion(s_base, tid, dt);
            __syncthreads();
#endif
#pragma unroll
            for (int sl = 0; sl < 2; sl++) {
                const int task = tid + 256 * sl;
                if (task < 384) {
                    const int side = task >= 192, l = (task % 192) / 12, e = task % 12;
                    const int lmk = (side ? g0 : f0) + l;
                    float o[3] = {0.f, 0.f, 0.f};
                    if (lmk < N) lin_column(s_bm, lu[sl], lv[sl], lrho[sl], e, td, o);
                    float* dst = (e < 9) ? ((side ? sBg : sBf) + l * 27 + e * 3) : ((side ? sDg : sDf) + l * 9 + (e - 9) * 3);
                    dst[0] = o[0];
                    dst[1] = o[1];
                    dst[2] = o[2];
                } else if (tI == tJ && tid >= 128 && tid < 128 + PT && f0 + tid - 128 < N) {
                    // mean propagation with the OLD base state (:102-104)
                    const V3 o = convolve_feature(s_bm[0], lu[sl], lv[sl], lrho[sl]);
                    const int lmk = f0 + tid - 128;
                    mu_next[EKF_BASE + 3 * lmk] = o.x;
                    mu_next[EKF_BASE + 3 * lmk + 1] = o.y;
                    mu_next[EKF_BASE + 3 * lmk + 2] = o.z;
                }
            }
            __syncthreads();
        }
        PSTAMP_(2);
        // X on the base columns, once per landmark row of the tile
        for (int e = tid; e < PT * 27; e += 256) {
            const int l = e / 27, r = (e % 27) / 9, b = e % 9;
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < 9; c++) acc = acc + sBf[l * 27 + c * 3 + r] * sPbb[c * 9 + b];
#pragma unroll
            for (int q = 0; q < 3; q++) acc = acc + sDf[l * 9 + q * 3 + r] * sPfb[l * 27 + q * 9 + b];
            sXb[e] = acc;
        }
        __syncthreads();
        PSTAMP_(3);
        // Lanes run along f, the ROW landmark: the 16 lanes of a group read / write 48 contiguous floats of a column of Sigma (three
        // floats each, one 12-byte access), four columns groups per wavefront.  (Rounds 1-4 had the lanes along g: sixteen
        // columns per access, 12 bytes apart in each -- 1.8 TB/s of the 8 n^2 bytes at N = 1024, where Sigma is 38 MB.)
        // (Requesting this block in front of the staging instead -- it is not needed before here -- was tried in round 6 and is SLOWER, 9.0 -> 9.3 us
        // at N = 256 and 30 -> 35.5 us at N = 1024: vmcnt retires in order, so the staged operands' first barrier then waits for these loads too.)
        const int lf = tid % PT, lg = tid / PT;
        const int f = f0 + lf, g = g0 + lg;
        if (f >= N || g >= N) return;
        float Pfg[3][3];  // own block P(22+3f+q, 22+3g+s)
#pragma unroll
        for (int sIdx = 0; sIdx < 3; sIdx++) {
            const float3 c3 = *reinterpret_cast<const float3*>(P + (size_t)(EKF_BASE + 3 * g + sIdx) * ld + EKF_BASE + 3 * f);
            Pfg[0][sIdx] = c3.x;
            Pfg[1][sIdx] = c3.y;
            Pfg[2][sIdx] = c3.z;
        }
        float Xg[3][3];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int sIdx = 0; sIdx < 3; sIdx++) {
                float acc = 0.f;
#pragma unroll
                for (int c = 0; c < 9; c++) acc = acc + sBf[lf * 27 + c * 3 + r] * sPbg[lg * 27 + c * 3 + sIdx];
#pragma unroll
                for (int q = 0; q < 3; q++) acc = acc + sDf[lf * 9 + q * 3 + r] * Pfg[q][sIdx];
                Xg[r][sIdx] = acc;
            }
#pragma unroll
        for (int sIdx = 0; sIdx < 3; sIdx++) {
            float o3[3];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                float acc = 0.f;
#pragma unroll
                for (int c = 0; c < 9; c++) acc = acc + sXb[lf * 27 + r * 9 + c] * sBg[lg * 27 + c * 3 + sIdx];
#pragma unroll
                for (int q = 0; q < 3; q++) acc = acc + Xg[r][q] * sDg[lg * 9 + q * 3 + sIdx];
                const int i = EKF_BASE + 3 * f + r, j = EKF_BASE + 3 * g + sIdx;
                o3[r] = predict_finish(acc, i, j, dt);
            }
            *reinterpret_cast<float3*>(Pout + (size_t)(EKF_BASE + 3 * g + sIdx) * ld + EKF_BASE + 3 * f) = make_float3(o3[0], o3[1], o3[2]);
        }
        PSTAMP_(4);
        return;
    }
    const int wb = (int)blockIdx.x - ntile;
    float* sA = sm;                        // [22*22]  A(i,l) at l*22+i
    float* sLB = sm + 3072;                // LIN: [PC][27] B and [PC][9] D of this workgroup's landmarks
    float* sLD = sLB + PC * 27;
    const float* FBp = FB;                 // where this workgroup reads its landmarks' B / D blocks from
    const float* FDp = FD;
    int lm0 = 0;                           // ... and the landmark index that corresponds to offset 0 there
    if (LIN) {
        float* s_hi = sm + 2048;           // [16][22] convolveBaseState at +delta / -delta
        float* s_lo = s_hi + 16 * EKF_BASE;
        lm0 = (wb == 0) ? 0 : ((wb <= chunks) ? (wb - 1) * PC : (wb - chunks - 1) * PC);
        const int lt = tid - 128;          // threads 128..163: the 36 derivative columns of the PC landmarks
        float u = 0.f, v = 0.f, rho = 1.f;
        const bool ltask = wb > 0 && lt >= 0 && lt < PC * 12 && lm0 + lt / 12 < N;
        if (ltask) {
            const int lmk = lm0 + lt / 12;
            u = mu[EKF_BASE + 3 * lmk];
            v = mu[EKF_BASE + 3 * lmk + 1];
            rho = mu[EKF_BASE + 3 * lmk + 2];
        }
        __syncthreads();                   // s_base
        if (tid < 32) {
            lin_base_test_point(s_base, tid, dt, ((tid & 1) ? s_lo : s_hi) + (tid >> 1) * EKF_BASE);
        } else if (tid == 32 && wb == 0) {
            float o[EKF_BASE];
            convolve_base(s_base, dt, o);
#pragma unroll
            for (int i = 0; i < EKF_BASE; i++) mu_next[i] = o[i];
        } else if (tid >= 64 && tid < 64 + 19) {
            s_bm[tid - 64] = lin_base_motion(s_base, tid - 64, dt);
        }
        __syncthreads();
        for (int e = tid; e < EKF_BASE * EKF_BASE; e += 256) {
            const int j = e / EKF_BASE, i = e % EKF_BASE;
            sA[e] = (j < 16) ? (s_hi[j * EKF_BASE + i] - s_lo[j * EKF_BASE + i]) / td : ((i == j) ? 1.f : 0.f);
        }
        if (wb > 0 && lt >= 0 && lt < PC * 12) {
            float o[3] = {0.f, 0.f, 0.f};
            const int l = lt / 12, e = lt % 12;
            if (ltask) lin_column(s_bm, u, v, rho, e, td, o);
            float* dst = (e < 9) ? (sLB + l * 27 + e * 3) : (sLD + l * 9 + (e - 9) * 3);
            dst[0] = o[0];
            dst[1] = o[1];
            dst[2] = o[2];
        }
        FBp = sLB;
        FDp = sLD;
        __syncthreads();  // A and the landmarks' B, D blocks are in LDS
        PSTAMP_(1);
    } else {
        for (int e = tid; e < EKF_BASE * EKF_BASE; e += 256) sA[e] = FA[e];
    }
    if (wb <= chunks) {
        // ---- base rows: i < 22; columns j < 22 (wb == 0) or the 63 columns of landmark chunk wb-1 ----
        float* sX1 = sm + 512;             // [22][22]  X(i,k), k < 22, at k*22+i
        float* sX2 = sm + 1024;            // [63][22]  X(i, j0+jc) at jc*22+i
        __syncthreads();
        for (int e = tid; e < EKF_BASE * EKF_BASE; e += 256) {
            const int i = e % EKF_BASE, k = e / EKF_BASE;
            const float* pc = P + (size_t)k * ld;
            float acc = 0.f;
            for (int l = 0; l < EKF_BASE; l++) acc = acc + sA[l * EKF_BASE + i] * pc[l];
            sX1[e] = acc;
        }
        if (wb == 0) {
            __syncthreads();
            for (int e = tid; e < EKF_BASE * EKF_BASE; e += 256) {
                const int i = e % EKF_BASE, j = e / EKF_BASE;
                float acc = 0.f;
                for (int k = 0; k < EKF_BASE; k++) acc = acc + sX1[k * EKF_BASE + i] * sA[k * EKF_BASE + j];
                Pout[(size_t)j * ld + i] = predict_finish(acc, i, j, dt);
            }
            PSTAMP_(4);
            return;
        }
        const int g0 = (wb - 1) * PC, j0 = EKF_BASE + 3 * g0;
        const int ncol = min(3 * PC, n - j0);
        for (int e = tid; e < EKF_BASE * ncol; e += 256) {
            const int i = e % EKF_BASE, jc = e / EKF_BASE;
            const float* pc = P + (size_t)(j0 + jc) * ld;
            float acc = 0.f;
            for (int l = 0; l < EKF_BASE; l++) acc = acc + sA[l * EKF_BASE + i] * pc[l];
            sX2[e] = acc;
        }
        __syncthreads();
        for (int e = tid; e < EKF_BASE * ncol; e += 256) {
            const int i = e % EKF_BASE, jc = e / EKF_BASE;
            const int g = g0 + jc / 3, sIdx = jc % 3, j = j0 + jc;
            const float* b = FBp + (size_t)(g - lm0) * 27 + sIdx;
            const float* d = FDp + (size_t)(g - lm0) * 9 + sIdx;
            float acc = 0.f;
            for (int c = 0; c < 9; c++) acc = acc + sX1[(7 + c) * EKF_BASE + i] * b[c * 3];
            for (int q = 0; q < 3; q++) acc = acc + sX2[(3 * (jc / 3) + q) * EKF_BASE + i] * d[q * 3];
            Pout[(size_t)j * ld + i] = predict_finish(acc, i, j, dt);
        }
        PSTAMP_(4);
        return;
    }
    // ---- base columns: j < 22; rows of landmark chunk wb-chunks-1 ----
    {
        float* sX3 = sm + 512;             // [22][64]  X(i0+ic, k), k < 22, at k*64+ic
        const int f0 = (wb - chunks - 1) * PC, i0 = EKF_BASE + 3 * f0;
        const int nrow = min(3 * PC, n - i0);
        for (int e = tid; e < nrow * EKF_BASE; e += 256) {
            const int ic = e % nrow, k = e / nrow;
            const int f = f0 + ic / 3, r = ic % 3;
            const float* pc = P + (size_t)k * ld;
            const float* b = FBp + (size_t)(f - lm0) * 27 + r;
            const float* d = FDp + (size_t)(f - lm0) * 9 + r;
            float acc = 0.f;
            for (int c = 0; c < 9; c++) acc = acc + b[c * 3] * pc[7 + c];
            for (int q = 0; q < 3; q++) acc = acc + d[q * 3] * pc[EKF_BASE + 3 * f + q];
            sX3[k * 64 + ic] = acc;
        }
        __syncthreads();
        for (int e = tid; e < nrow * EKF_BASE; e += 256) {
            const int ic = e % nrow, j = e / nrow;
            float acc = 0.f;
            for (int k = 0; k < EKF_BASE; k++) acc = acc + sX3[k * 64 + ic] * sA[k * EKF_BASE + j];
            const int i = i0 + ic;
            Pout[(size_t)j * ld + i] = predict_finish(acc, i, j, dt);
        }
        PSTAMP_(4);
    }
#undef PSTAMP_
}

// dense mode epilogue: P += Q(dt) on the diagonal, then prune
__global__ void add_noise_flush_kernel(float* P, int ld, int n, float dt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (i >= n) return;
    float v = P[(size_t)j * ld + i];
    if (i == j) v = v + process_noise(i, dt);
    if (!(fabsf(v) > EKF_FLUSH_THRESH)) v = 0.f;
    P[(size_t)j * ld + i] = v;
}

// ---------------------------------------------------------------------------------------
// Update bookkeeping (:486-541, :554-555): one workgroup scans the pass flags into the
// measurement map idx (formFeatureMeasurementMap :634-661), stores last_klt / delete flags,
// z - H*mu and the per-row measurement noise.  Integer work is bit-exact by construction.
// ---------------------------------------------------------------------------------------
// With a frame counter (device-resident sequences replayed from a hipGraph) the measurement
// of frame *frame_counter is used and the counter advances modulo `frames`.
__global__ __launch_bounds__(1024) void update_bookkeeping_kernel(BookArgs a) { bookkeeping_body<1024>(a); }

// The innovation gate (include/ekfvio.h, ekfvio_set_gate) and the bookkeeping behind it in ONE launch of the same single workgroup: every
// thread first evaluates the squared Mahalanobis distance of the landmarks the scan will give it -- H is a selection, so the 2 x 2 innovation
// covariance is Sigma's (u,v) block + R: three strided loads from Sigma, two from mu, six from z / R -- and leaves the effective flag
// pass && accepted in a.pass_eff; the bookkeeping then runs over those flags, so a rejected landmark takes the road of one the tracker failed
// (:526-529: no rows, last_klt kept, delete flag set).  Runs behind process(dt): mu and Sigma are the propagated state.  fp32, in the order the
// header states (this file is compiled with -ffp-contract=off), so a float32 restatement of those lines gives the same bits.
__global__ __launch_bounds__(1024) void gate_bookkeeping_kernel(BookArgs a) {
    __shared__ int s_gated;
    const int tid = threadIdx.x, N = a.N;
    const float* z = a.z;
    const float* R = a.R;
    const uint8_t* pass = a.pass;
    if (a.frame_counter) {
        const int fi = *a.frame_counter;
        z += (size_t)fi * 2 * N;
        R += (size_t)fi * 4 * N;
        pass += (size_t)fi * N;
    }
    if (tid == 0) s_gated = 0;
    __syncthreads();
    const int per = (N + 1023) / 1024;  // (the partition of bookkeeping_body<1024>: a thread reads back only flags it wrote itself)
    const int lo = tid * per, hi = min(N, lo + per);
    int rejected = 0;
    for (int i = lo; i < hi; i++) {
        float d2 = -1.f;
        uint8_t eff = 0, rej = 0;
        if (pass[i]) {
            const int s = EKF_BASE + 3 * i;
            const float* Ps = a.P + (size_t)s * a.ldp + s;
            const float y0 = z[2 * i] - a.mu[s], y1 = z[2 * i + 1] - a.mu[s + 1];
            const float ca = Ps[0] + R[4 * i];
            const float cb = Ps[1] + R[4 * i + 1];  // the lower triangle's element of both
            const float cc = Ps[a.ldp + 1] + R[4 * i + 3];
            const float det = ca * cc - cb * cb;
            const float q = ((cc * y0) * y0 - ((2.f * cb) * y0) * y1) + (ca * y1) * y1;
            d2 = q / det;
            eff = (det > 0.f && d2 <= a.chi2) ? 1 : 0;  // (a NaN anywhere rejects)
            rej = eff ^ 1;
            rejected += rej;
        }
        a.d2[i] = d2;
        a.gated[i] = rej;
        a.pass_eff[i] = eff;
    }
    if (rejected) atomicAdd(&s_gated, rejected);
    __syncthreads();
    if (tid == 0) {
        a.gate_words[0] = s_gated;
        a.gate_words[1] = N;
        if (a.count_total) {
            long long* total = reinterpret_cast<long long*>(a.gate_words + 2);
            *total = *total + s_gated;
        }
    }
    bookkeeping_body<1024, true>(a);
}

#include "gather_body.inc"

__global__ __launch_bounds__(256) void gather_kernel(GatherArgs a) {
    __shared__ float tile[64 * 65];
    gather_body(a, blockIdx.x, tile);
}

// (G = K*R - T[:, idx] and mu += K*y are epilogues of the two Joseph GEMMs: see GemmEpi.)
// Stand-alone mean update, used when no landmark was measured (m = 0):
// mu += K*y (:600), quaternion renormalisation (:605-609).  64 state rows per workgroup;
// the four wavefronts each sum a quarter of the measurement rows (coalesced along the state
// index), combined in ascending order.
__global__ __launch_bounds__(256) void mean_update_kernel(const float* __restrict__ K, int ld, int n, int m,
                                                          const float* __restrict__ y, float* mu, int* frame_counter,
                                                          int frames) {
    __shared__ float s_part[4][64];
    __shared__ float s_q[4];
    const int rl = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + rl;
    const int chunk = (m + 3) / 4;
    const int r0 = w * chunk, r1 = min(m, r0 + chunk);
    float acc = 0.f;
    if (i < n) {
#pragma unroll 8
        for (int r = r0; r < r1; r++) acc = acc + K[(size_t)r * ld + i] * y[r];
    }
    s_part[w][rl] = acc;
    __syncthreads();
    float v = 0.f;
    if (w == 0 && i < n) v = mu[i] + (((s_part[0][rl] + s_part[1][rl]) + s_part[2][rl]) + s_part[3][rl]);
    if (blockIdx.x == 0) {
        if (w == 0 && rl >= 3 && rl <= 6) s_q[rl - 3] = v;
        __syncthreads();
        if (w == 0 && rl >= 3 && rl <= 6) {
            float qn = sqrtf(s_q[0] * s_q[0] + s_q[1] * s_q[1] + s_q[2] * s_q[2] + s_q[3] * s_q[3]);
            v = v / qn;
        }
    }
    if (w == 0 && i < n) mu[i] = v;
    if (frame_counter && blockIdx.x == 0 && threadIdx.x == 0) {
        const int fi = *frame_counter + 1;
        *frame_counter = (fi >= frames) ? 0 : fi;
    }
}

__global__ void check_sigma_kernel(const float* P, int ld, int n, float* out) {
    // out[0] = min diagonal, out[1] = max |P(i,j)-P(j,i)|; single block
    __shared__ float s_min[256], s_max[256];
    float mn = 3.4e38f, mx = 0.f;
    for (size_t e = threadIdx.x; e < (size_t)n * n; e += 256) {
        int i = e % n, j = e / n;
        if (i == j) mn = fminf(mn, P[(size_t)j * ld + i]);
        if (i > j) mx = fmaxf(mx, fabsf(P[(size_t)j * ld + i] - P[(size_t)i * ld + j]));
    }
    s_min[threadIdx.x] = mn;
    s_max[threadIdx.x] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            s_min[threadIdx.x] = fminf(s_min[threadIdx.x], s_min[threadIdx.x + s]);
            s_max[threadIdx.x] = fmaxf(s_max[threadIdx.x], s_max[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = s_min[0];
        out[1] = s_max[0];
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------
void launch_linearize(ekfvio_filter* f, float dt, const BookArgs* book) {
    ProfScope ps(f, PC_LINEARIZE);
    BookArgs b;
    if (book) b = *book;
    // landmark workgroups + the base-block workgroup (+ the bookkeeping workgroup)
    const int blocks = (f->N + LIN_LM - 1) / LIN_LM + 1 + (b.enabled ? 1 : 0);
    hipLaunchKernelGGL(linearize_kernel, dim3(blocks), dim3(256), 0, f->stream, f->mu, f->N, dt, f->FA, f->FB, f->FD,
                       f->mu_next, b);
}

BookArgs make_book_args(ekfvio_filter* f, int m, const float* d_z, const float* d_R, const uint8_t* d_pass, const int* d_frame_counter) {
    BookArgs a;
    a.enabled = 1;
    a.N = f->N;
    a.m_pad = round_up(m > 0 ? m : 1, EKF_TILE);
    a.z = d_z;
    a.R = d_R;
    a.pass = d_pass;
    a.last_klt = f->last_klt;
    a.del_flag = f->del_flag;
    a.idx = f->idx;
    a.inv_idx = f->inv_idx;
    a.zrow = f->yres;
    a.Rm = f->Rm;
    a.frame_counter = d_frame_counter;
    return a;
}

void launch_build_dense_F(ekfvio_filter* f, float* Fdense) {
    dim3 grid((f->ldp + 255) / 256, f->ldp);
    hipLaunchKernelGGL(build_dense_F_kernel, grid, dim3(256), 0, f->stream, f->FA, f->FB, f->FD, f->N, f->n, f->ldp,
                       Fdense);
}

// process(dt) (:96-121): executes a PredictPlan (plan.h, plan_predict)
bool launch_predict(ekfvio_filter* f, float dt, const BookArgs* book, bool prelinearized) {
    // structured mode linearises inside the propagation kernel (predict_fused_kernel<true>) or in a launch in front; the dense mode and
    // ekfvio_linearize keep the stand-alone linearize_kernel.  pre (round 6): the previous update's last GEMM has linearised for this step
    // already (launch_update, GemmEpi::lin_blocks): FA / FB / FD and the propagated mean are in place, the propagation kernel only carries
    // the bookkeeping along
    const PredictPlan p = plan_predict(f->tune, plan_shape(f), prelinearized);
    if (p.lin_in_front) launch_linearize(f, dt, book);
    const int n = f->n, ld = f->ldp;
    if (p.dense) {
        launch_build_dense_F(f, f->Fdense);
        {
            ProfScope ps(f, PC_GEMM_PREDICT, 4.0 * n * (double)n * n);
            // X = F*P (B = P is [K x N]); P' = X*F^T (B = F is [N x K])
            GemmCall g;
            g.M = g.N = n, g.K = round_up(n, 32), g.A = f->Fdense, g.lda = ld, g.B = f->P, g.ldb = ld, g.C = f->P2, g.ldc = ld;
            launch_gemm(f, g);
            g.transB = true, g.A = f->P2, g.B = f->Fdense, g.C = f->P;
            launch_gemm(f, g);
        }
        ProfScope ps(f, PC_PREDICT);
        hipLaunchKernelGGL(add_noise_flush_kernel, dim3((n + 255) / 256, n), dim3(256), 0, f->stream, f->P, ld, n, dt);
    } else {
        ProfScope ps(f, PC_PREDICT, 4.0 * n * (358.0 + 36.0 * f->N));
        BookArgs b;
        if (book && p.book_rides()) b = *book;
        const dim3 grid(p.grid(b.enabled != 0));
        if (p.lin_inside)
            hipLaunchKernelGGL(predict_fused_kernel<true>, grid, dim3(256), 0, f->stream, f->P, ld, f->N, n, f->FA, f->FB, f->FD, dt, f->P2,
                               p.ts, p.chunks, f->mu, f->mu_next, b, f->sweep_dbg);
        else
            hipLaunchKernelGGL(predict_fused_kernel<false>, grid, dim3(256), 0, f->stream, f->P, ld, f->N, n, f->FA, f->FB, f->FD, dt, f->P2,
                               p.ts, p.chunks, f->mu, f->mu_next, b, f->sweep_dbg);
        std::swap(f->P, f->P2);  // out of place; P2's padding is zero as well (never written outside n x n)
    }
    // the propagated mean becomes the state (landmarks used the OLD base state, :102-107)
    std::swap(f->mu, f->mu_next);
    return p.pre;
}

// The P-update GEMMs behind the sweep and the gain, described ONCE for the update itself and for the profiler's scratch launches.
//   TAIL_JOSEPH, two GEMMs, both triangles:   T = Sigma - K*(H Sigma)   (I_KH * Sigma, :594) in place; also G and K*y (column n)
//                                             Sigma' = T + G*K^T, pruned (:594-596, :625), mirrored in the throughput regime (plan_gemm)
//   else ONE GEMM, the left Joseph factor applied to T2 = Sigma - X A^-1 X^T = Sigma (I - K H)^T, the RIGHT one (X = Sigma H^T; Sigma is symmetric
//   only to rounding, so this is not the transpose of the reference's (I - K H) Sigma): Sigma' = (I - K H) T2 + K R K^T = T2 + K G'^T, which is the
//   reference's (I - K H) Sigma (I - K H)^T + K R K^T (:594-596), pruned (:625).
// `from` -> `to`: the covariance read and written (the two-GEMM tail passes through `to`).  What touches the filter's state -- the mean, the frame
// counter, the sweep's flags and abort word, the riding linearisation -- is the update's to add (launch_update); as built here the last GEMM is
// EPI_MEAN with nothing to finish.
struct TailGemms {
    int count;
    GemmCall g[2];
    GemmCall& last() { return g[count - 1]; }
};
static TailGemms update_tail_gemms(ekfvio_filter* f, const UpdatePlan& p, const float* from, float* to) {
    const int n = f->n, ld = f->ldp;
    TailGemms t;
    GemmCall c;
    c.M = c.N = n, c.K = p.m_pad, c.transB = true, c.lda = c.ldb = c.ldcin = c.ldc = ld, c.beta = 1.f, c.Cin = from, c.C = to;
    t.g[0] = t.g[1] = c;
    GemmCall& g2 = t.g[1];
    if (p.tail != TAIL_JOSEPH) {
        t.count = 1;
        GemmCall& g = t.g[0];
        g.A = f->Km, g.B = f->Gm, g.flush = true, g.epi.mode = EPI_MEAN;
        return t;
    }
    t.count = 2;
    GemmCall& g1 = t.g[0];
    g1.N = n + 1, g1.alpha = -1.f, g1.A = f->Km, g1.B = f->Wt;
    g1.epi.mode = EPI_JOSEPH1, g1.epi.inv_idx = f->inv_idx, g1.epi.Rm = f->Rm, g1.epi.G = f->Gm, g1.epi.ldg = ld;
    g2.A = f->Gm, g2.B = f->Km, g2.Cin = to, g2.flush = true, g2.epi.mode = EPI_MEAN, g2.epi.sym = 1;
    return t;
}

// updateWithFeaturePositions (:475-628) on device-resident z/R/pass; m = 2*(#passed) known to the host
UpdateResult launch_update(ekfvio_filter* f, const UpdateInputs& in) {
    // The innovation gate (ekfvio_set_gate): the device decides which landmarks are measured, so the host no longer knows m -- the count is on
    // the device for every caller.  What the host still knows is "no landmark passed": nothing to gate, m = 0 (the gate kernel still runs, so that
    // ekfvio_get_gate reports this update).
    const bool gate = f->gate_chi2 > 0.f && f->N > 0;
    const UpdatePlan p = plan_update(f, in.m, in.m_on_device || (gate && in.m > 0), in.next_dt, in.recoverable);
    const int m = p.m, m_pad = p.m_pad, n_pad = p.n_pad, n = f->n, ld = f->ldp;
    UpdateResult out;
    f->last_m = m;
    {
        ProfScope ps(f, PC_GATHER);
        if (!in.bookkeeping_done) {
            BookArgs bk = make_book_args(f, m, in.z, in.R, in.pass, in.frame_counter);
            if (p.m_on_device) bk.m_out = f->info + 2;
            if (gate) {
                bk.pass_eff = f->gate_pass, bk.mu = f->mu, bk.P = f->P, bk.ldp = ld, bk.chi2 = f->gate_chi2;
                bk.d2 = f->gate_d2, bk.gated = f->gate_flag, bk.gate_words = f->gate_words, bk.count_total = in.gate_counted ? 0 : 1;
                hipLaunchKernelGGL(gate_bookkeeping_kernel, dim3(1), dim3(1024), 0, f->stream, bk);
            } else
                hipLaunchKernelGGL(update_bookkeeping_kernel, dim3(1), dim3(1024), 0, f->stream, bk);
        }
        if (p.fused_gather) {
            // the gather and the factorisation of the first diagonal tile share one launch (chol.hip)
            launch_gather_potrf(f, p);
        } else if (m > 0 && p.sweep != SWEEP_PERSIST_FUSED) {
            const GatherArgs ga = make_gather_args(f, p);
            const int nb2 = p.with_wt ? (m_pad / 64) * (ld / 64) : 0;  // 64x64 transposing tiles of Wt
            hipLaunchKernelGGL(gather_kernel, dim3(ga.nb1 + nb2), dim3(256), 0, f->stream, ga);
        }
    }
    if (m <= 0) {
        // no measurement: products are empty, only the quaternion renormalisation remains (:605-609)
        ProfScope ps(f, PC_UPDATE_MISC);
        hipLaunchKernelGGL(mean_update_kernel, dim3((n + 63) / 64), dim3(256), 0, f->stream, f->Km, ld, n, 0, f->yres, f->mu,
                           in.frame_counter, in.frames);
        return out;
    }
    // [A; Sigma H^T; I] -> [L; Y; L^-T]; a persistent sweep finds its flags zero behind an update of this handle or behind gather_potrf_kernel
    const bool zero_flags = p.persistent() && !p.fused_gather && !f->sweep_flags_clean;
    const int* abort = p.sweep == SWEEP_PERSIST_FUSED ? launch_persist_fused(f, p, zero_flags)
                                                      : launch_chol_sweep(f, p, f->Saug, f->Laug, f->Linv, f->ld_aug, zero_flags);
    // (ekfvio_update: the update's status is final here -- the host gets it now and returns while the GEMMs below run)
    if (in.publish_seq) launch_publish_status(f, in.publish_seq), out.published = true;
    TailGemms tail = update_tail_gemms(f, p, p.tail == TAIL_T2 ? t2_buffer(f) : f->P, f->P);
    GemmEpi& e2 = tail.last().epi;  // the update's last GEMM finishes the mean
    e2.mu = f->mu, e2.Pcol = f->P + (size_t)n * ld, e2.n = n;
    e2.frame_counter = in.frame_counter, e2.frames = in.frames;
    e2.abort = abort;        // a persistent sweep that gave up: the GEMMs write nothing (T2, K, G' are scratch)
    if (p.persistent()) {    // ... and one that ran: the update's last GEMM leaves its flags zero for the next one
        e2.zero_words = f->sweep_sync, e2.n_zero = persist_zero_words(m_pad, n_pad);
        f->sweep_flags_clean = true;
    }
    if (p.tail == TAIL_T2) f->t2_updates++;
    // K = (Sigma H^T) A^-1  (:577-580), unless the sweep formed it
    if (p.gain == GAIN_SCHUR) launch_joseph_g(f, m, m_pad, n_pad, p.m_on_device);
    else if (p.gain == GAIN2_T2_TILES) launch_gain2_tiles(f, p);  // (K, G', K y and T2 in one launch behind the per-step sweep)
    else if (p.gain != GAIN_SWEEP) launch_gain_from_sweep(f, p, f->Laug, f->ld_aug, n, f->Km, f->Gm, ld, 0);
    if (p.tail == TAIL_JOSEPH) {
        // back to back (one profiler scope, two launches)
        tail.g[0].epi.abort = abort;
        ProfScope ps(f, PC_GEMM_UPDATE, 2.0 * n * (double)(n + 1) * m_pad + 2.0 * n * (double)n * m_pad, 2);
        launch_gemm(f, tail.g[0]);
        if (in.between) out.between_seq = in.between(f, 0);  // (ekfvio_step_image: the frame's outputs, from mu and K y in column n of P)
        launch_gemm(f, tail.g[1]);
        return out;
    }
    // TAIL_SCHUR: [A; Sigma H^T; I] was swept with Sigma and the gain as Schur tiles (chol.hip), T2 in place in f->P; joseph_g_kernel pruned K and left
    // G' = K R^T - (H T2)^T and K y.  TAIL_T2 (round 6): T2 came out of the persistent launch itself (freed owners, chol_persist.inc t2_tile; behind any
    // other sweep of such a shape gain2_t2_tiles_kernel forms the same T2 from the stored panel blocks), in the dense-F buffer; the gain tiles of the
    // same launch left K, G' and the partial sums of K y.
    if (p.tail == TAIL_T2 && in.between) out.between_seq = in.between(f, m_pad / 64);  // (ekfvio_step_image: the frame's outputs, from mu and the partial sums of K y)
    ProfScope ps(f, PC_GEMM_UPDATE, 2.0 * n * (double)n * m_pad, 1);
    // the mean takes K y from the partial sums (joseph_g_kernel / gain_tile2: Kyp = Wt, one row of sums per block column): plan.h, tail_gemm_shape
    e2.mode = EPI_MEAN_PARTIAL;
    e2.Kyp = f->Wt, e2.kyp_blocks = m_pad / 64, e2.kyp_ld = ld;
    if (p.lin_blocks) {  // (plan_update: the next process(dt)'s linearisation rides in this launch)
        e2.lin_blocks = p.lin_blocks, e2.lin_N = f->N, e2.lin_dt = in.next_dt;
        e2.lin_FA = f->FA, e2.lin_FB = f->FB, e2.lin_FD = f->FD, e2.lin_mu_next = f->mu_next;
        out.linearised_next = true;
    }
    launch_gemm(f, tail.last());
    return out;
}

// into scratch (P2, Gm): no mean, no frame counter, no abort word, no flag zeroing -- the tail as update_tail_gemms builds it
int launch_update_gemms_scratch(ekfvio_filter* f, const UpdatePlan& p, int reps, double* last_flops) {
    TailGemms tail = update_tail_gemms(f, p, f->P, f->P2);
    for (int r = 0; r < reps; r++)
        for (int k = 0; k < tail.count; k++) launch_gemm(f, tail.g[k]);
    const GemmShape sh = gemm_shape(tail.last());
    *last_flops = gemm_executed_flops(sh, plan_gemm(f->tune, f->num_cus, sh));
    return tail.count;
}

void launch_check_sigma(ekfvio_filter* f, float* d_out) {
    hipLaunchKernelGGL(check_sigma_kernel, dim3(1), dim3(256), 0, f->stream, f->P, f->ldp, f->n, d_out);
}
