// ekf_vio_amd/csrc/aid.hip — a linear aiding measurement of the base state, z = H x[0:22] + v, v ~ N(0, R), with H (k x 22), z and R (k x k)
// given by the caller (include/ekfvio.h, ekfvio_aid_update): wheel speed, a position or altitude fix, a nonholonomic constraint.  Not in the
// reference, whose monocular filter has no metric input at all.  It is the arithmetic of the IMU update (imu.hip) and of the zero-velocity
// update (zupt.hip) with a dense H: gains per state row with S (k x k) factored by every workgroup for itself, then one elementwise Joseph
// pass; aid.h has the lines both the kernels and the host's ekfvio_aid_innovation compile.
//
// TWO launches, instantiated per k = 1..6, so that a one-row update does not pay for six and no private array is indexed by a run-time
// row count.  H, z, R and the gate travel as kernel arguments.  Every workgroup of the gain kernel forms H Sigma on the base columns, S,
// the factor and the verdict for itself; workgroup 0 publishes the verdict, d2 and the two counts to device words (the Joseph kernel reads
// the first) and to pinned host memory.  Both kernels return at once on "not accepted"; the mean is updated IN PLACE by the Joseph kernel's
// first column of workgroups, so a rejected update touches neither Sigma nor the mean.
#include <stddef.h>
#include <string.h>

#include "common.h"
#include "aid.h"
#include "imu_model.h"

namespace {

constexpr int AID_THREADS = 256;

template <int K>
struct AidArgs {
    float H[K * AID_BASE];
    float z[K];
    float R[K * K];
    float chi2;
};

// words (device) and host_words (pinned): [0] accepted, [1] applied since create / reset, [2] rejected likewise, [3] d2's bits
template <int K>
__global__ __launch_bounds__(AID_THREADS) void aid_gain_kernel(const float* __restrict__ P, int ld, int n, const float* __restrict__ mu, AidArgs<K> a,
                                                               float* __restrict__ Km, float* __restrict__ Gm, float* __restrict__ Wm,
                                                               float* __restrict__ dmu, long long* __restrict__ words,
                                                               long long* __restrict__ host_words) {
    constexpr int NA = K * AID_BASE + K + K * K;  // H, z, R as they lie in the arguments
    __shared__ float sArg[NA];
    __shared__ float sWb[K * AID_BASE];  // (H Sigma)(r, c) on the base columns
    __shared__ float sA[K * K], sS[K * K], sL[K * K];
    __shared__ float sy[K];
    __shared__ int s_ok;
    const float* sH = sArg;
    const float* sz = sArg + K * AID_BASE;
    const float* sR = sz + K;
    const int tid = threadIdx.x;
    const int i = blockIdx.x * AID_THREADS + tid;
    {
        const float* af = reinterpret_cast<const float*>(&a);  // (H, z and R are consecutive floats of the argument block)
        static_assert(offsetof(AidArgs<K>, z) == sizeof(float) * K * AID_BASE && offsetof(AidArgs<K>, R) == sizeof(float) * (K * AID_BASE + K), "layout");
        if (tid < NA) sArg[tid] = af[tid];
    }
    __syncthreads();
    if (tid < K * AID_BASE) {
        const int r = tid / AID_BASE, c = tid % AID_BASE;
        sWb[tid] = aid_dot22(sH + r * AID_BASE, P + (size_t)c * ld, 1);  // sum_c' H(r, c') Sigma(c', c)
    }
    if (tid >= AID_THREADS - K) {  // (another wavefront than the one above)
        const int r = tid - (AID_THREADS - K);
        sy[r] = sz[r] - aid_dot22(sH + r * AID_BASE, mu, 1);
    }
    __syncthreads();
    if (tid < K * K) {
        const int r = tid / K, s = tid % K;
        const float v = aid_dot22(sWb + r * AID_BASE, sH + s * AID_BASE, 1);
        sA[tid] = v;
        sS[tid] = v + aid_R(sR, K, r, s);
    }
    __syncthreads();
    if (tid == 0) {
        const bool ok = aid_factor<K>(sS, sL);
        const float d2 = ok ? aid_d2<K>(sL, sy) : NAN;
        const int acc = aid_accept(ok, d2, a.chi2) ? 1 : 0;
        s_ok = acc;
        if (blockIdx.x == 0) {
            const long long applied = words[1] + acc, rejected = words[2] + (1 - acc);
            const long long d2bits = (long long)__float_as_uint(d2);
            words[0] = acc, words[1] = applied, words[2] = rejected, words[3] = d2bits;
            host_words[0] = acc, host_words[1] = applied, host_words[2] = rejected, host_words[3] = d2bits;
            __threadfence_system();  // (the host reads them behind a stream wait or behind the frame's status word, which a later launch publishes)
        }
    }
    __syncthreads();
    if (!s_ok) return;  // (uniform over the workgroup)
    if (i < n) {
        float x[K], w[K], kk[K];
#pragma unroll
        for (int r = 0; r < K; r++) x[r] = aid_dot22(sH + r * AID_BASE, P + i, (size_t)ld);       // sum_c Sigma(i, c) H(r, c): coalesced over i
#pragma unroll
        for (int r = 0; r < K; r++) w[r] = aid_dot22(sH + r * AID_BASE, P + (size_t)i * ld, 1);   // sum_c H(r, c) Sigma(c, i)
        aid_gain_row<K>(x, sL, kk);
        float dm = 0.f;
#pragma unroll
        for (int r = 0; r < K; r++) {
            float t = x[r];
#pragma unroll
            for (int s = 0; s < K; s++) t = t - kk[s] * sA[s * K + r];
            float kr = kk[0] * aid_R(sR, K, 0, r);
#pragma unroll
            for (int s = 1; s < K; s++) kr = kr + kk[s] * aid_R(sR, K, s, r);
            Km[(size_t)r * ld + i] = kk[r];
            Gm[(size_t)r * ld + i] = kr - t;
            Wm[(size_t)r * ld + i] = w[r];
            dm = dm + kk[r] * sy[r];
        }
        dmu[i] = dm;
    }
}

// Sigma <- Sigma - K (H Sigma) + G K^T, pruned: one element per thread, column per blockIdx.y (zupt_joseph_kernel with K terms); the
// workgroups of column 0 also add the mean's increments, in place, and workgroup (0, 0) renormalises the quaternion
template <int K>
__global__ __launch_bounds__(AID_THREADS) void aid_joseph_kernel(float* __restrict__ P, int ld, int n, float* __restrict__ mu,
                                                                 const long long* __restrict__ words, const float* __restrict__ Km,
                                                                 const float* __restrict__ Gm, const float* __restrict__ Wm,
                                                                 const float* __restrict__ dmu) {
    __shared__ float sq[4];
    if (words[0] == 0) return;  // (uniform: every thread reads the same word)
    const int i = blockIdx.x * AID_THREADS + threadIdx.x, j = blockIdx.y;
    if (i < n) {
        float v = P[(size_t)j * ld + i];
#pragma unroll
        for (int s = 0; s < K; s++) v = v - Km[(size_t)s * ld + i] * Wm[(size_t)s * ld + j];
#pragma unroll
        for (int s = 0; s < K; s++) v = v + Gm[(size_t)s * ld + i] * Km[(size_t)s * ld + j];
        P[(size_t)j * ld + i] = (fabsf(v) > EKF_FLUSH_THRESH) ? v : 0.f;
    }
    if (j == 0) {
        if (i < n) {
            const float v = mu[i] + dmu[i];
            if (i >= 3 && i <= 6) sq[i - 3] = v;  // workgroup 0
            else mu[i] = v;
        }
        if (blockIdx.x == 0) {
            __syncthreads();
            if (threadIdx.x < 4) {
                const float qn = sqrtf(sq[0] * sq[0] + sq[1] * sq[1] + sq[2] * sq[2] + sq[3] * sq[3]);
                mu[3 + threadIdx.x] = sq[threadIdx.x] / qn;
            }
        }
    }
}

// the verdict's memory, made when a handle first asks for an aiding update (a handle that never does allocates and launches nothing it did
// not before): four device words and the same four in pinned, device-mapped host memory
int aid_ensure(ekfvio_filter* f) {
    if (f->aid_words && f->d_haid) return EKFVIO_OK;
    HIP_TRY(f, hipSetDevice(f->device));
    if (!f->h_aid) {
        HIP_TRY(f, host_alloc(f, &f->h_aid, sizeof(long long) * 4, MEM_PINNED_COHERENT));
        memset(f->h_aid, 0, sizeof(long long) * 4);
    }
    if (!f->d_haid) HIP_TRY(f, hipHostGetDevicePointer((void**)&f->d_haid, f->h_aid, 0));
    if (!f->aid_words) HIP_TRY(f, dev_alloc(f, &f->aid_words, 4));
    return EKFVIO_OK;
}

template <int K>
void launch_aid_k(ekfvio_filter* f, const float* H, const float* z, const float* R, float chi2) {
    const int n = f->n, ld = f->ldp;
    AidArgs<K> a;
    memcpy(a.H, H, sizeof(a.H)), memcpy(a.z, z, sizeof(a.z)), memcpy(a.R, R, sizeof(a.R));
    a.chi2 = chi2;
    // the three n x k work matrices live in the first k columns of the camera update's buffers (free between updates), as the IMU update's and
    // the zero-velocity update's; the mean's increments in the seventh of Km
    float* dmu = f->Km + (size_t)6 * ld;
    hipLaunchKernelGGL(aid_gain_kernel<K>, dim3((n + AID_THREADS - 1) / AID_THREADS), dim3(AID_THREADS), 0, f->stream, f->P, ld, n, f->mu, a, f->Km,
                       f->Gm, f->Wt, dmu, f->aid_words, f->d_haid);
    hipLaunchKernelGGL(aid_joseph_kernel<K>, dim3((n + AID_THREADS - 1) / AID_THREADS, n), dim3(AID_THREADS), 0, f->stream, f->P, ld, n, f->mu,
                       (const long long*)f->aid_words, f->Km, f->Gm, f->Wt, dmu);
}

// (the caller has validated the rows and made the verdict's memory)
void launch_aid(ekfvio_filter* f, int k, const float* H, const float* z, const float* R, float chi2) {
    ProfScope ps(f, PC_UPDATE_MISC, 0, 2);
    switch (k) {
        case 1: launch_aid_k<1>(f, H, z, R, chi2); break;
        case 2: launch_aid_k<2>(f, H, z, R, chi2); break;
        case 3: launch_aid_k<3>(f, H, z, R, chi2); break;
        case 4: launch_aid_k<4>(f, H, z, R, chi2); break;
        case 5: launch_aid_k<5>(f, H, z, R, chi2); break;
        default: launch_aid_k<6>(f, H, z, R, chi2); break;
    }
    f->aid_pending = true;
}

template <int K>
int innovation_k(const float* mu, const float* Pb, const float* H, const float* z, const float* R, float* y, float* S, float* d2, int32_t* pd) {
    float yy[K], A[K * K], SS[K * K], dd;
    const bool ok = aid_innovation<K>(mu, Pb, AID_BASE, H, z, R, yy, A, SS, &dd);
    if (y) memcpy(y, yy, sizeof(yy));
    if (S) memcpy(S, SS, sizeof(SS));
    if (d2) *d2 = dd;
    if (pd) *pd = ok ? 1 : 0;
    return EKFVIO_OK;
}

}  // namespace

// ekfvio_step_image, behind the tracker and in front of the zero-velocity update, the gate and the camera update: the standing measurement
// of ekfvio_set_frame_aid on the propagated state.  The caller has checked that the setting is on
void launch_aid_frame(ekfvio_filter* f) { launch_aid(f, f->frame_aid_k, f->frame_aid_H, f->frame_aid_z, f->frame_aid_R, f->frame_aid_chi2); }
// ... and the host's end of it: the frame's one wait lies behind every aiding launch enqueued so far
void aid_note_frame(ekfvio_filter* f) { f->aid_pending = false; }
// ekfvio_reset: the counts and the report start over; the standing measurement stays.  The device words are zeroed in front of the reset's
// wait, the pinned ones behind it (an aiding launch still in flight publishes into them)
hipError_t aid_reset_enqueue(ekfvio_filter* f) {
    if (!f->aid_words) return hipSuccess;
    return hipMemsetAsync(f->aid_words, 0, sizeof(long long) * 4, f->stream);
}
void aid_reset_done(ekfvio_filter* f) {
    if (f->h_aid) memset(f->h_aid, 0, sizeof(long long) * 4);
    f->aid_pending = false;
}

extern "C" {

int ekfvio_aid_update(ekfvio_filter* f, int32_t k, const float* H, const float* z, const float* R, float chi2) {
    if (!f || !aid_rows_valid(k, H, z, R, chi2)) return EKFVIO_EINVAL;
    const int rc = aid_ensure(f);
    if (rc != EKFVIO_OK) return rc;
    f->out_fresh = f->out_cov_fresh = false;
    HIP_TRY(f, hipSetDevice(f->device));
    launch_aid(f, k, H, z, R, chi2);
    HIP_TRY(f, hipGetLastError());
    return EKFVIO_OK;
}

int ekfvio_aid(ekfvio_filter* f, double stamp, int32_t k, const float* H, const float* z, const float* R, float chi2) {
    if (!f || !aid_rows_valid(k, H, z, R, chi2) || !isfinite(stamp)) return EKFVIO_EINVAL;
    if (!f->have_stamp) {  // the first stamp only sets the time, as ekfvio_imu's
        f->out_fresh = false;
        f->t_stamp = stamp;
        f->have_stamp = true;
        return EKFVIO_OK;
    }
    const double dt = stamp - f->t_stamp;
    if (!(dt >= 0)) return EKFVIO_EINVAL;
    const int rc = aid_ensure(f);
    if (rc != EKFVIO_OK) return rc;
    f->out_fresh = f->out_cov_fresh = false;
    HIP_TRY(f, hipSetDevice(f->device));
    launch_predict(f, (float)dt);
    f->t_stamp = stamp;
    launch_aid(f, k, H, z, R, chi2);
    HIP_TRY(f, hipGetLastError());
    return EKFVIO_OK;
}

int ekfvio_set_frame_aid(ekfvio_filter* f, int32_t k, const float* H, const float* z, const float* R, float chi2) {
    if (!f) return EKFVIO_EINVAL;
    if (k == 0) {  // off: the other arguments are not looked at
        f->frame_aid_k = 0;
        return EKFVIO_OK;
    }
    if (!aid_rows_valid(k, H, z, R, chi2)) return EKFVIO_EINVAL;  // (the setting stays what it was)
    const int rc = aid_ensure(f);
    if (rc != EKFVIO_OK) return rc;
    // (read by the next ekfvio_step_image; the frame loop is in no captured graph)
    memcpy(f->frame_aid_H, H, sizeof(float) * k * AID_BASE);
    memcpy(f->frame_aid_z, z, sizeof(float) * k);
    memcpy(f->frame_aid_R, R, sizeof(float) * k * k);
    f->frame_aid_chi2 = chi2;
    f->frame_aid_k = k;
    return EKFVIO_OK;
}

int ekfvio_get_aid(ekfvio_filter* f, float* d2_last, int32_t* accepted_last, int64_t* applied_total, int64_t* rejected_total) {
    if (!f) return EKFVIO_EINVAL;
    long long w[4] = {0, 0, 0, 0};
    if (f->h_aid) {
        if (f->aid_pending) {  // a bare ekfvio_aid* call since the last frame's wait
            HIP_TRY(f, hipSetDevice(f->device));
            HIP_TRY(f, hipStreamSynchronize(f->stream));
            f->aid_pending = false;
        }
        w[0] = __atomic_load_n(&f->h_aid[0], __ATOMIC_ACQUIRE);
        w[1] = f->h_aid[1], w[2] = f->h_aid[2], w[3] = f->h_aid[3];
    }
    if (d2_last) {
        const uint32_t bits = (uint32_t)w[3];
        memcpy(d2_last, &bits, sizeof(float));
    }
    if (accepted_last) *accepted_last = (int32_t)w[0];
    if (applied_total) *applied_total = w[1];
    if (rejected_total) *rejected_total = w[2];
    return EKFVIO_OK;
}

int ekfvio_aid_innovation(const float* base_mu, const float* Sigma_bb, int32_t k, const float* H, const float* z, const float* R, float* y,
                          float* S, float* d2, int32_t* pd) {
    if (!base_mu || !Sigma_bb || !aid_rows_valid(k, H, z, R, 0.f)) return EKFVIO_EINVAL;
    for (int e = 0; e < AID_BASE; e++)
        if (!isfinite(base_mu[e])) return EKFVIO_EINVAL;
    for (int e = 0; e < AID_BASE * AID_BASE; e++)
        if (!isfinite(Sigma_bb[e])) return EKFVIO_EINVAL;
    // Sigma_bb is row-major: element (i, j) at 22 i + j.  The lines read P(i, j) at Pb[j ld + i]: the transpose of what the caller handed over
    float Pb[AID_BASE * AID_BASE];
    for (int i = 0; i < AID_BASE; i++)
        for (int j = 0; j < AID_BASE; j++) Pb[j * AID_BASE + i] = Sigma_bb[i * AID_BASE + j];
    switch (k) {
        case 1: return innovation_k<1>(base_mu, Pb, H, z, R, y, S, d2, pd);
        case 2: return innovation_k<2>(base_mu, Pb, H, z, R, y, S, d2, pd);
        case 3: return innovation_k<3>(base_mu, Pb, H, z, R, y, S, d2, pd);
        case 4: return innovation_k<4>(base_mu, Pb, H, z, R, y, S, d2, pd);
        case 5: return innovation_k<5>(base_mu, Pb, H, z, R, y, S, d2, pd);
        default: return innovation_k<6>(base_mu, Pb, H, z, R, y, S, d2, pd);
    }
}

int ekfvio_aid_rows_body_velocity(const float* R_cv, const float* p_cv, const float* v, const float* cov, float* H, float* z, float* R) {
    static const float eye[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, zero[3] = {0.f, 0.f, 0.f};
    if (!v || !cov || !H || !z || !R) return EKFVIO_EINVAL;
    const float* Rc = R_cv ? R_cv : eye;
    const float* pc = p_cv ? p_cv : zero;
    if (!imu_extrinsics_valid(Rc, pc)) return EKFVIO_EINVAL;
    float Hh[3 * AID_BASE], zz[3], RR[9];
    aid_body_velocity_rows(Rc, pc, Hh);
    for (int r = 0; r < 3; r++) zz[r] = v[r];
    for (int r = 0; r < 3; r++) {
        if (!isfinite(v[r])) return EKFVIO_EINVAL;
        for (int s = 0; s < 3; s++) RR[3 * r + s] = aid_R(cov, 3, r, s);  // the lower triangle of cov, mirrored: the upper one is never read
    }
    if (!aid_rows_valid(3, Hh, zz, RR, 0.f)) return EKFVIO_EINVAL;
    memcpy(H, Hh, sizeof(Hh)), memcpy(z, zz, sizeof(zz)), memcpy(R, RR, sizeof(RR));
    return EKFVIO_OK;
}

}  // extern "C"
