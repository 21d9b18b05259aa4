// ekf_vio_amd/csrc/zupt.hip — zero-velocity update (include/ekfvio.h, ekfvio_set_zupt).  Not in the reference, whose filter learns that
// the camera stands still only through the landmarks' pixel measurements.  Two parts: the DECISION, per frame of ekfvio_step_image, from
// the tracker's pass flags and pixel results, which never leave the device (zupt.h: the inline functions the host's ekfvio_zupt_decide
// compiles too); and the UPDATE z = 0 on h(x) = [vel; omega], H a selection of state rows 7..12, in the shape of the IMU update's pair
// (imu.hip): gains per state row with S (6 x 6) factored by every workgroup for itself, then one elementwise Joseph pass.
//
// TWO launches per frame, not three: every workgroup of the gain kernel evaluates the decision for itself, as it factors S for itself
// (at most max_features flags and pixel pairs, a strided loop with wavefront ballots), and workgroup 0 publishes it.  A launch of its
// own for the decision would have cost more than the loop does in each of the gain kernel's few workgroups.  Both kernels return at once on a
// "no"; the mean is updated IN PLACE by the Joseph kernel's first column of workgroups from the increments the gain kernel left, so a
// "no" touches neither Sigma nor the mean and the host swaps nothing.
#include <string.h>

#include "common.h"
#include "zupt.h"

namespace {

constexpr int ZU_THREADS = 256;

// The decision's inputs and where it is published.  The reference pixel is last_klt * f + c, as the tracker forms it (klt_track_kernel)
struct ZuptDecide {
    const uint8_t* pass = nullptr;    // [N] the tracker's final verdict
    const float* next_px = nullptr;   // [2N] the tracked pixels
    const float* last_klt = nullptr;  // [2N]
    float fxp = 1.f, fyp = 1.f, cxp = 0.f, cyp = 0.f;  // the previous frame's intrinsics
    int N = 0;
    float t2 = 0.f;
    int min_tracks = 0;
    float min_ratio = 0.f;
    int* words = nullptr;        // device [4]: stationary, n_pass, n_still, N
    int* host_words = nullptr;   // the same in pinned host memory ...
    float* host_flow2 = nullptr; // ... and flow2 [N]
};

// All ZU_THREADS threads of a workgroup; every thread returns the verdict.  s_cnt: 8 ints of LDS.  publish (uniform): this workgroup writes
// the words and flow2
__device__ inline int zupt_decide_wg(const ZuptDecide& d, bool publish, int* s_cnt) {
    const int tid = threadIdx.x;
    int np = 0, ns = 0;  // this wavefront's counts (the same in every lane)
    for (int base = 0; base < d.N; base += ZU_THREADS) {
        const int i = base + tid;
        bool p = false, s = false;
        float e2 = -1.f;
        if (i < d.N && d.pass[i] != 0) {
            p = true;
            const float px = d.last_klt[2 * i] * d.fxp + d.cxp;
            const float py = d.last_klt[2 * i + 1] * d.fyp + d.cyp;
            e2 = zupt_flow2(d.next_px[2 * i], d.next_px[2 * i + 1], px, py);
            s = zupt_still(e2, d.t2);
        }
        np += __popcll(__ballot(p));
        ns += __popcll(__ballot(s));
        if (publish && i < d.N) d.host_flow2[i] = e2;
    }
    if ((tid & 63) == 0) s_cnt[tid >> 6] = np, s_cnt[4 + (tid >> 6)] = ns;
    __syncthreads();
    const int n_pass = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    const int n_still = (s_cnt[4] + s_cnt[5]) + (s_cnt[6] + s_cnt[7]);
    const int st = zupt_stationary(n_pass, n_still, d.min_tracks, d.min_ratio);
    if (publish) {
        if (tid == 0) {
            d.words[0] = st, d.words[1] = n_pass, d.words[2] = n_still, d.words[3] = d.N;
            d.host_words[0] = st, d.host_words[1] = n_pass, d.host_words[2] = n_still, d.host_words[3] = d.N;
        }
        __threadfence_system();  // (the host reads them behind the frame's status word, which a later launch publishes)
    }
    return st;
}

#ifdef EKFVIO_TEST_HOOKS
// The decision alone, one workgroup: the test hook's launch (arbitrary points); the product library does not carry it
__global__ __launch_bounds__(ZU_THREADS) void zupt_decide_kernel(ZuptDecide d) {
    __shared__ int s_cnt[8];
    (void)zupt_decide_wg(d, true, s_cnt);
}
#endif

// Gains, G = K R - T H^T, W = H Sigma and the mean's increment, one state row per thread: imu_gain_kernel with H the selection of state
// rows 7..12 (include/ekfvio.h has the lines).  forced == 0: the workgroup decides first (d) and returns on a "no"
__global__ __launch_bounds__(ZU_THREADS) void zupt_gain_kernel(const float* __restrict__ P, int ld, int n, const float* __restrict__ mu, int forced,
                                                               ZuptDecide d, float vel_var, float omega_var, float* __restrict__ K6,
                                                               float* __restrict__ G6, float* __restrict__ W6, float* __restrict__ dmu) {
    __shared__ float sPb[6][6];  // Sigma(7+r, 7+c) as stored
    __shared__ float sL[6][6];
    __shared__ float sy[6];
    __shared__ int s_cnt[8];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * ZU_THREADS + tid;
    if (!forced && !zupt_decide_wg(d, blockIdx.x == 0, s_cnt)) return;  // (uniform over the workgroup)
    if (tid < 36) {
        const int r = tid / 6, c = tid % 6;
        sPb[r][c] = P[(size_t)(7 + c) * ld + 7 + r];
    }
    if (tid < 6) sy[tid] = -mu[7 + tid];  // z - h(x), z = 0
    __syncthreads();
    if (tid == 0) {  // Cholesky of the lower triangle of S = Sigma[7..12, 7..12] + R
        for (int j = 0; j < 6; j++) {
            float dd = sPb[j][j] + (j < 3 ? vel_var : omega_var);
            for (int k = 0; k < j; k++) dd = dd - sL[j][k] * sL[j][k];
            sL[j][j] = sqrtf(dd);
            for (int r = j + 1; r < 6; r++) {
                float v = sPb[r][j];
                for (int k = 0; k < j; k++) v = v - sL[r][k] * sL[j][k];
                sL[r][j] = v / sL[j][j];
            }
        }
    }
    __syncthreads();
    if (i < n) {
        float x[6], w[6], kk[6];
#pragma unroll
        for (int r = 0; r < 6; r++) x[r] = P[(size_t)(7 + r) * ld + i];  // Sigma(i, 7+r): coalesced over i
#pragma unroll
        for (int r = 0; r < 6; r++) w[r] = P[(size_t)i * ld + 7 + r];    // Sigma(7+r, i)
        // k = x S^-1 = (x L^-T) L^-1
#pragma unroll
        for (int r = 0; r < 6; r++) {
            float v = x[r];
#pragma unroll
            for (int k = 0; k < r; k++) v = v - kk[k] * sL[r][k];
            kk[r] = v / sL[r][r];
        }
#pragma unroll
        for (int r = 5; r >= 0; r--) {
            float v = kk[r];
#pragma unroll
            for (int k = r + 1; k < 6; k++) v = v - kk[k] * sL[k][r];
            kk[r] = v / sL[r][r];
        }
        float dm = 0.f;
#pragma unroll
        for (int r = 0; r < 6; r++) {
            float t = x[r];  // T on column 7+r
#pragma unroll
            for (int s = 0; s < 6; s++) t = t - kk[s] * sPb[s][r];
            const float g = kk[r] * (r < 3 ? vel_var : omega_var) - t;
            K6[(size_t)r * ld + i] = kk[r];
            G6[(size_t)r * ld + i] = g;
            W6[(size_t)r * ld + i] = w[r];
            dm = dm + kk[r] * sy[r];
        }
        dmu[i] = dm;
    }
}

// Sigma <- Sigma - K (H Sigma) + G K^T, pruned: one element per thread, column per blockIdx.y (imu_joseph_kernel); the workgroups of
// column 0 also add the mean's increments, in place, and workgroup (0, 0) renormalises the quaternion.  decision != null: 0 there returns
__global__ __launch_bounds__(ZU_THREADS) void zupt_joseph_kernel(float* __restrict__ P, int ld, int n, float* __restrict__ mu,
                                                                 const int* __restrict__ decision, const float* __restrict__ K6,
                                                                 const float* __restrict__ G6, const float* __restrict__ W6,
                                                                 const float* __restrict__ dmu) {
    __shared__ float sq[4];
    if (decision && *decision == 0) return;  // (uniform: every thread reads the same word)
    const int i = blockIdx.x * ZU_THREADS + threadIdx.x, j = blockIdx.y;
    if (i < n) {
        float v = P[(size_t)j * ld + i];
#pragma unroll
        for (int s = 0; s < 6; s++) v = v - K6[(size_t)s * ld + i] * W6[(size_t)s * ld + j];
#pragma unroll
        for (int s = 0; s < 6; s++) v = v + G6[(size_t)s * ld + i] * K6[(size_t)s * ld + j];
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

// the decision's memory, made when a handle first asks for it (a handle that never does allocates and launches nothing it did not
// before): four device words, and four words plus flow2[max_features] of pinned, device-mapped host memory, as h_out
int zupt_ensure(ekfvio_filter* f) {
    if (f->zupt_words && f->d_hzupt) return EKFVIO_OK;
    HIP_TRY(f, hipSetDevice(f->device));
    // (each step on its own pointer: a call behind one that failed half way takes up where that one stopped and acquires nothing twice)
    if (!f->h_zupt) {
        const size_t maxf = (size_t)(f->cfg.max_features > 0 ? f->cfg.max_features : 1);
        HIP_TRY(f, host_alloc(f, &f->h_zupt, sizeof(int) * 4 + sizeof(float) * maxf, MEM_PINNED_COHERENT));
        memset(f->h_zupt, 0, sizeof(int) * 4 + sizeof(float) * maxf);
    }
    if (!f->d_hzupt) HIP_TRY(f, hipHostGetDevicePointer((void**)&f->d_hzupt, f->h_zupt, 0));
    if (!f->zupt_words) HIP_TRY(f, dev_alloc(f, &f->zupt_words, 4));
    return EKFVIO_OK;
}

void zupt_publish_to(ekfvio_filter* f, ZuptDecide& d) {
    d.words = f->zupt_words;
    d.host_words = f->d_hzupt;
    d.host_flow2 = reinterpret_cast<float*>(f->d_hzupt + 4);
}

// d == null: unconditional (ekfvio_zupt_update)
void launch_zupt(ekfvio_filter* f, const ZuptDecide* d, float vel_var, float omega_var) {
    const int n = f->n, ld = f->ldp;
    ProfScope ps(f, PC_UPDATE_MISC, 0, 2);
    // the three n x 6 work matrices live in the first six columns of the camera update's buffers (free between updates), as the IMU update's;
    // the mean's increments in the seventh of Km
    float* dmu = f->Km + (size_t)6 * ld;
    hipLaunchKernelGGL(zupt_gain_kernel, dim3((n + ZU_THREADS - 1) / ZU_THREADS), dim3(ZU_THREADS), 0, f->stream, f->P, ld, n, f->mu, d ? 0 : 1,
                       d ? *d : ZuptDecide(), vel_var, omega_var, f->Km, f->Gm, f->Wt, dmu);
    hipLaunchKernelGGL(zupt_joseph_kernel, dim3((n + ZU_THREADS - 1) / ZU_THREADS, n), dim3(ZU_THREADS), 0, f->stream, f->P, ld, n, f->mu,
                       d ? (const int*)f->zupt_words : (const int*)nullptr, f->Km, f->Gm, f->Wt, dmu);
}

}  // namespace

// ekfvio_step_image, behind the tracker and in front of the update: the decision over the tracker's results as they lie on the device and,
// on a "yes", the update of the propagated state.  The caller has checked that the setting is on and that there are landmarks
void launch_zupt_frame(ekfvio_filter* f) {
    ZuptDecide d;
    d.pass = f->pass, d.next_px = f->klt_next_px, d.last_klt = f->last_klt;
    klt_intrinsics(f, f->frames[f->cur ^ 1].K, &d.fxp, &d.fyp, &d.cxp, &d.cyp);
    d.N = f->N;
    d.t2 = f->zupt_max_flow_px * f->zupt_max_flow_px;
    d.min_tracks = f->zupt_min_tracks, d.min_ratio = f->zupt_min_ratio;
    zupt_publish_to(f, d);
    launch_zupt(f, &d, f->zupt_vel_var, f->zupt_omega_var);
}

// ... and the host's end of it, with the frame's status word in hand: decided = launch_zupt_frame ran in this frame
void zupt_note_frame(ekfvio_filter* f, bool decided) {
    if (!decided) {
        f->zupt_n = f->zupt_pass = f->zupt_still = f->zupt_applied_last = 0;
        return;
    }
    f->zupt_applied_last = __atomic_load_n(&f->h_zupt[0], __ATOMIC_ACQUIRE) != 0;
    f->zupt_pass = f->h_zupt[1], f->zupt_still = f->h_zupt[2], f->zupt_n = f->h_zupt[3];
    f->zupt_applied_total += f->zupt_applied_last;
}

extern "C" {

int ekfvio_set_zupt(ekfvio_filter* f, float max_flow_px, int32_t min_tracks, float min_ratio, float vel_variance, float omega_variance) {
    if (!f) return EKFVIO_EINVAL;
    if (max_flow_px == 0.f) {  // off: the other arguments are not looked at
        f->zupt_max_flow_px = 0.f;
        f->zupt_n = f->zupt_pass = f->zupt_still = f->zupt_applied_last = 0;
        return EKFVIO_OK;
    }
    if (!zupt_decision_valid(max_flow_px, min_tracks, min_ratio) || !zupt_variances_valid(vel_variance, omega_variance)) return EKFVIO_EINVAL;
    const int rc = zupt_ensure(f);
    if (rc != EKFVIO_OK) return rc;
    // (read by the next ekfvio_step_image; the frame loop is in no captured graph)
    f->zupt_max_flow_px = max_flow_px, f->zupt_min_tracks = min_tracks, f->zupt_min_ratio = min_ratio;
    f->zupt_vel_var = vel_variance, f->zupt_omega_var = omega_variance;
    return EKFVIO_OK;
}

int ekfvio_zupt_update(ekfvio_filter* f, float vel_variance, float omega_variance) {
    if (!f || !zupt_variances_valid(vel_variance, omega_variance)) return EKFVIO_EINVAL;
    f->out_fresh = f->out_cov_fresh = false;
    HIP_TRY(f, hipSetDevice(f->device));
    launch_zupt(f, nullptr, vel_variance, omega_variance);
    HIP_TRY(f, hipGetLastError());
    return EKFVIO_OK;
}

int ekfvio_get_zupt(ekfvio_filter* f, float* flow2N, int32_t* n_landmarks, int32_t* n_pass, int32_t* n_still, int32_t* applied_last,
                    int64_t* applied_total) {
    if (!f) return EKFVIO_EINVAL;
    const bool on = f->zupt_max_flow_px > 0.f;
    const int n = on ? f->zupt_n : 0;
    if (n_landmarks) *n_landmarks = n;
    if (n_pass) *n_pass = on ? f->zupt_pass : 0;
    if (n_still) *n_still = on ? f->zupt_still : 0;
    if (applied_last) *applied_last = on ? f->zupt_applied_last : 0;
    if (applied_total) *applied_total = f->zupt_applied_total;
    // (flow2 is in pinned host memory, and the frame that wrote it has read its status word behind the decision's launch)
    if (flow2N && n > 0) memcpy(flow2N, f->h_zupt + 4, sizeof(float) * n);
    return EKFVIO_OK;
}

int ekfvio_zupt_decide(const float* prev_px, const float* cur_px, const uint8_t* pass, int32_t count, float max_flow_px, int32_t min_tracks,
                       float min_ratio, float* flow2, int32_t* n_pass, int32_t* n_still, int32_t* stationary) {
    if (count < 0 || (count > 0 && (!prev_px || !cur_px || !pass)) || !zupt_decision_valid(max_flow_px, min_tracks, min_ratio)) return EKFVIO_EINVAL;
    const float t2 = max_flow_px * max_flow_px;
    int np = 0, ns = 0;
    for (int i = 0; i < count; i++) {
        float e2 = -1.f;
        if (pass[i] != 0) {
            np++;
            e2 = zupt_flow2(cur_px[2 * i], cur_px[2 * i + 1], prev_px[2 * i], prev_px[2 * i + 1]);
            if (zupt_still(e2, t2)) ns++;
        }
        if (flow2) flow2[i] = e2;
    }
    if (n_pass) *n_pass = np;
    if (n_still) *n_still = ns;
    if (stationary) *stationary = zupt_stationary(np, ns, min_tracks, min_ratio);
    return EKFVIO_OK;
}

#ifdef EKFVIO_TEST_HOOKS
int ekfvio_test_zupt_decide(ekfvio_filter* f, const float* prev_px, const float* cur_px, const uint8_t* pass, int32_t count, float max_flow_px,
                            int32_t min_tracks, float min_ratio, float* flow2, int32_t* n_pass, int32_t* n_still, int32_t* stationary) {
    if (!f || count < 0 || (count > 0 && (!prev_px || !cur_px || !pass)) || !zupt_decision_valid(max_flow_px, min_tracks, min_ratio)) return EKFVIO_EINVAL;
    if (count > f->cfg.max_features) return EKFVIO_ECAPACITY;
    const int rc = zupt_ensure(f);
    if (rc != EKFVIO_OK) return rc;
    HIP_TRY(f, hipSetDevice(f->device));
    // the points stand in the tracker's own buffers; the reference pixel is prev_px * 1 + 0, exact
    if (count > 0) {
        HIP_TRY(f, hipMemcpyAsync(f->klt_prev_px, prev_px, sizeof(float) * 2 * count, hipMemcpyHostToDevice, f->stream));
        HIP_TRY(f, hipMemcpyAsync(f->klt_next_px, cur_px, sizeof(float) * 2 * count, hipMemcpyHostToDevice, f->stream));
        HIP_TRY(f, hipMemcpyAsync(f->pass, pass, count, hipMemcpyHostToDevice, f->stream));
    }
    ZuptDecide d;
    d.pass = f->pass, d.next_px = f->klt_next_px, d.last_klt = f->klt_prev_px;
    d.N = count;
    d.t2 = max_flow_px * max_flow_px;
    d.min_tracks = min_tracks, d.min_ratio = min_ratio;
    zupt_publish_to(f, d);
    hipLaunchKernelGGL(zupt_decide_kernel, dim3(1), dim3(ZU_THREADS), 0, f->stream, d);
    HIP_TRY(f, hipGetLastError());
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    if (stationary) *stationary = f->h_zupt[0];
    if (n_pass) *n_pass = f->h_zupt[1];
    if (n_still) *n_still = f->h_zupt[2];
    if (flow2 && count > 0) memcpy(flow2, f->h_zupt + 4, sizeof(float) * count);
    return EKFVIO_OK;
}
#endif

}  // extern "C"
