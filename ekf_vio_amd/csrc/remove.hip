// ekf_vio_amd/csrc/remove.hip — removal of landmarks from the state (ekfvio_remove_features, ekfvio_step_image with
// cfg.remove_lost = 1).  Not in the reference, which flags a lost landmark (TightlyCoupledEKF.cpp:528) and keeps it for good.
// Marginalising landmarks out of a Gaussian is exact: their entries leave mu, their rows and columns leave Sigma, and the kept
// ones keep their order.  A pure copy: the result is bit for bit the compacted state.
#include <string.h>

#include <algorithm>

#include "common.h"

namespace {

constexpr int RM_THREADS = 256;
constexpr int RM_COLS = RM_THREADS / 64;  // one source column per wavefront

struct RemoveArgs {
    float* P;                // Sigma, column-major, ld (cleared outside the new block behind the reads)
    float* P2;               // its ping-pong partner: receives Sigma' (written only if something is removed)
    float* mu_src;           // (zeroed in [n', n_old) behind the reads)
    float* mu_dst;           // receives mu' (always: the host swaps the mean after every launch)
    float* last_klt;         // compacted in place
    uint8_t* del_flag;       // compacted in place
    int* id32;               // the landmarks' ids (int64) and birth stamps (double), compacted in place: moved as pairs of 32-bit
    int* born32;             // words, two per landmark
    const uint8_t* remove;   // the decision per landmark: nonzero = remove.  May be del_flag itself.
    int ld;
    int N_host;              // landmarks the host knows of ...
    const int* added;        // ... plus these, from device memory (the replenishment's count; may be null)
    const int* info;         // non-null: info[0] bit 1 (the persistent sweep gave up) -> nothing is removed
    int* words;              // [0] added - removed, [1] removed, [2] ticket (zero between launches)
    int* host_removed;       // may be null: the removed count, also into pinned host memory (d_hinfo + HW_REMOVED)
};

// The decision and its prefix sum over the landmarks, formed by every workgroup in LDS: pre[i] = kept landmarks in front of i,
// src_of[k] = the source landmark of kept landmark k.  Returns the number kept.
__device__ int scan_keep(const RemoveArgs& a, int N_old, bool keep_all, int* pre, int* src_of, int* wsum) {
    const int t = threadIdx.x;
    const int chunk = (N_old + RM_THREADS - 1) / RM_THREADS;
    const int i0 = min(t * chunk, N_old), i1 = min(i0 + chunk, N_old);
    int c = 0;
    for (int i = i0; i < i1; i++) c += (keep_all || a.remove[i] == 0) ? 1 : 0;
    wsum[t] = c;
    __syncthreads();
    // inclusive Hillis-Steele scan of the 256 chunk counts
    for (int s = 1; s < RM_THREADS; s <<= 1) {
        const int v = t >= s ? wsum[t - s] : 0;
        __syncthreads();
        wsum[t] += v;
        __syncthreads();
    }
    int k = wsum[t] - c;
    for (int i = i0; i < i1; i++) {
        pre[i] = k;
        if (keep_all || a.remove[i] == 0) src_of[k++] = i;
    }
    const int kept = wsum[RM_THREADS - 1];
    __syncthreads();
    return kept;
}

// An array of two 32-bit words per landmark, compacted in place by the LAST workgroup through `stage` (2 * kept ints of LDS that nothing
// else uses any more).  Every thread has passed a barrier behind the last use of `stage` when it gets here.
__device__ __forceinline__ void compact_pairs(int* arr, const int* src_of, int kept, int* stage) {
    for (int k = threadIdx.x; k < kept; k += RM_THREADS) {
        const int s = src_of[k];
        stage[2 * k] = arr[2 * s];
        stage[2 * k + 1] = arr[2 * s + 1];
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kept; k += RM_THREADS) {
        arr[2 * k] = stage[2 * k];
        arr[2 * k + 1] = stage[2 * k + 1];
    }
    __syncthreads();
}

// state index of row r of the compacted state (r < n')
__device__ __forceinline__ int src_row(const int* src_of, int r) {
    if (r < EKF_BASE) return r;
    const int q = r - EKF_BASE, l = q / 3;
    return EKF_BASE + 3 * src_of[l] + (q - 3 * l);
}

// Zeroes rows [lo, hi) of one column (hi <= ld, ld a multiple of 4): 16-byte stores where a run of four lies inside.
__device__ __forceinline__ void zero_rows(float* col, int lo, int hi, int lane) {
    for (int r4 = (lo & ~3) + 4 * lane; r4 < hi; r4 += 4 * 64) {
        if (r4 >= lo && r4 + 4 <= hi) {
            *reinterpret_cast<float4*>(col + r4) = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (int u = 0; u < 4; u++)
                if (r4 + u >= lo && r4 + u < hi) col[r4 + u] = 0.f;
        }
    }
}

// ONE launch: Sigma' = Sigma[keep, keep] into P2 (padding up to the old n zeroed in both P and P2), mu' = mu[keep] into mu_dst
// (mu_src zeroed in [n', n_old)), last_klt, del_flag, the ids and the birth stamps compacted in place, the counts into `words`.
// Grid: one source column j per wavefront, sized for the most columns the state can have; surplus workgroups only take part in
// the ticket.  Source column j is read by the wavefront that owns it and by no other, so that wavefront may clear it behind its
// reads: no workgroup waits for another.  The mean, last_klt, del_flag, the ids and the birth stamps are compacted by the LAST workgroup
// to take a ticket -- the decision may be del_flag itself, which every workgroup has finished reading by then.  The ids and the stamps
// take their turn in s_klt's 2 N ints, one after the other, once last_klt is back in global memory: the LDS size does not grow.
__global__ __launch_bounds__(RM_THREADS) void remove_features_kernel(RemoveArgs a) {
    extern __shared__ int lds[];
    __shared__ int wsum[RM_THREADS];
    __shared__ int s_last;
    const int N_old = a.N_host + (a.added ? *a.added : 0);
    const bool keep_all = a.info && (a.info[0] & 2);
    const int cap = N_old > 0 ? N_old : 1;
    int* pre = lds;                                         // [N_old]
    int* src_of = lds + cap;                                // [N_old]
    float* s_klt = reinterpret_cast<float*>(lds + 2 * cap);  // [2 N_old]
    uint8_t* s_del = reinterpret_cast<uint8_t*>(lds + 4 * cap);  // [N_old]
    const int kept = scan_keep(a, N_old, keep_all, pre, src_of, wsum);
    const int removed = N_old - kept;
    const int n_old = EKF_BASE + 3 * N_old, n_new = EKF_BASE + 3 * kept;
    if (threadIdx.x == 0) {
        // every workgroup's reads of the decision are behind this point
        const int t = __hip_atomic_fetch_add(a.words + 2, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (t == (int)gridDim.x - 1);
    }
    __syncthreads();
    const bool last = s_last != 0;

    if (removed > 0) {
        const int lane = threadIdx.x & 63;
        const int j = blockIdx.x * RM_COLS + (threadIdx.x >> 6);
        const float* src = a.P + (size_t)j * a.ld;
        if (j < n_old) {
            int c = -1;  // destination column of source column j (-1: removed)
            if (j < EKF_BASE) {
                c = j;
            } else {
                const int l = (j - EKF_BASE) / 3;
                const int k = pre[l];
                if (k < kept && src_of[k] == l) c = EKF_BASE + 3 * k + (j - EKF_BASE - 3 * l);
            }
            if (c >= 0) {
                float* dst = a.P2 + (size_t)c * a.ld;
                for (int r4 = 4 * lane; r4 < n_old; r4 += 4 * 64) {
                    float v[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) v[u] = (r4 + u < n_new) ? src[src_row(src_of, r4 + u)] : 0.f;
                    *reinterpret_cast<float4*>(dst + r4) = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
        }
        __syncthreads();  // the column's reads are done before it is cleared
        if (j < n_old) {
            zero_rows(a.P + (size_t)j * a.ld, j < n_new ? n_new : 0, n_old, lane);  // (P is the wavefront's own source column)
            if (j >= n_new) zero_rows(a.P2 + (size_t)j * a.ld, 0, n_old, lane);
        }
    }

    if (!last) return;
    // the mean, out of place (mu_dst is never read here)
    for (int e = threadIdx.x; e < n_old; e += RM_THREADS) a.mu_dst[e] = (e < n_new) ? a.mu_src[src_row(src_of, e)] : 0.f;
    // last_klt and del_flag, in place through LDS
    for (int k = threadIdx.x; k < kept; k += RM_THREADS) {
        const int s = src_of[k];
        s_klt[2 * k] = a.last_klt[2 * s];
        s_klt[2 * k + 1] = a.last_klt[2 * s + 1];
        s_del[k] = a.del_flag[s];
    }
    __syncthreads();
    for (int e = n_new + threadIdx.x; e < n_old; e += RM_THREADS) a.mu_src[e] = 0.f;
    for (int k = threadIdx.x; k < kept; k += RM_THREADS) {
        a.last_klt[2 * k] = s_klt[2 * k];
        a.last_klt[2 * k + 1] = s_klt[2 * k + 1];
        a.del_flag[k] = s_del[k];
    }
    __syncthreads();  // s_klt is free
    compact_pairs(a.id32, src_of, kept, reinterpret_cast<int*>(s_klt));
    compact_pairs(a.born32, src_of, kept, reinterpret_cast<int*>(s_klt));
    if (threadIdx.x == 0) {
        a.words[0] = (a.added ? *a.added : 0) - removed;
        a.words[1] = removed;
        a.words[2] = 0;  // the ticket, for the next launch
        if (a.host_removed) {
            *a.host_removed = removed;
            __threadfence_system();
        }
    }
}

}  // namespace

size_t remove_lds_bytes(const ekfvio_filter* f) {
    const size_t cap = (size_t)std::max(f->cfg.max_features, 1);
    return cap * (4 * sizeof(int) + 1);
}

// Enqueues the removal.  N_host + *added (added may be null) landmarks; the decision from `remove` (device memory), where null
// from del_flag.  abort_aware: nothing is removed behind an aborted persistent sweep (ekfvio_step_image).  The caller swaps
// mu <-> mu_next after every launch, P <-> P2 when something was removed (words[1] > 0), and applies words[0] to N.
void launch_remove_features(ekfvio_filter* f, const uint8_t* remove, const int* added, bool abort_aware, bool host_removed) {
    // the records of the landmarks about to leave are formed first, from the same decision and the same counts (ended.hip)
    if (f->ended_on) launch_ended_tracks(f, remove, added, abort_aware);
    RemoveArgs a;
    a.P = f->P;
    a.P2 = f->P2;
    a.mu_src = f->mu;
    a.mu_dst = f->mu_next;
    a.last_klt = f->last_klt;
    a.del_flag = f->del_flag;
    a.id32 = reinterpret_cast<int*>(f->lm_id);
    a.born32 = reinterpret_cast<int*>(f->lm_born);
    a.remove = remove ? remove : f->del_flag;
    a.ld = f->ldp;
    a.N_host = f->N;
    a.added = added;
    a.info = abort_aware ? f->info : nullptr;
    a.words = f->remove_words;
    a.host_removed = host_removed ? f->d_hinfo + HW_REMOVED : nullptr;
    const int n_bound = added ? f->n_cap : f->n;  // (the device count is at most max_features - N)
    const int grid = std::max(1, (n_bound + RM_COLS - 1) / RM_COLS);
    hipLaunchKernelGGL(remove_features_kernel, dim3(grid), dim3(RM_THREADS), remove_lds_bytes(f), f->stream, a);
}

// What a removal that took effect means for the host's mirror of the state.
void remove_applied(ekfvio_filter* f, int delta, int removed) {
    std::swap(f->mu, f->mu_next);
    if (removed > 0) {
        std::swap(f->P, f->P2);
        drop_graph(f);  // captured step graphs are for the old shape: recaptured at the next run
    }
    f->N += delta;
    f->n = EKF_BASE + 3 * f->N;
}

extern "C" {

int ekfvio_remove_features(ekfvio_filter* f, const uint8_t* remove, int32_t count, int32_t* removed) {
    if (!f) return EKFVIO_EINVAL;
    if (remove && count != f->N) return EKFVIO_EINVAL;
    if (removed) *removed = 0;
    if (remove_lds_bytes(f) > 64 * 1024) {
        f->last_error = "ekfvio_remove_features: max_features too large for the removal kernel's LDS";
        return EKFVIO_ECAPACITY;
    }
    HIP_TRY(f, hipSetDevice(f->device));
    if (remove) {
        int k = 0;
        for (int i = 0; i < count; i++) k += remove[i] ? 1 : 0;
        if (k == 0) {  // nothing launched, the state untouched
            ended_note_removal(f, 0);
            return EKFVIO_OK;
        }
        f->out_fresh = false;
        // staged through the tracker's pass buffer (free between calls: ekfvio_step_image rewrites it before it reads it)
        HIP_TRY(f, hipMemcpyAsync(f->pass, remove, count, hipMemcpyHostToDevice, f->stream));
        launch_remove_features(f, f->pass, nullptr, false, false);
        HIP_TRY(f, hipGetLastError());
        HIP_TRY(f, hipStreamSynchronize(f->stream));  // (remove is the caller's memory)
        remove_applied(f, -k, k);
        ended_note_removal(f, k);
        if (removed) *removed = k;
        return EKFVIO_OK;
    }
    if (f->N == 0) {
        ended_note_removal(f, 0);
        return EKFVIO_OK;
    }
    f->out_fresh = false;
    // the flags are on the device: one status poll brings the count back
    launch_remove_features(f, nullptr, nullptr, false, false);
    int bad = 0, k = 0;
    const int rc = wait_status(f, &bad, f->remove_words + 1, &k);
    if (rc != EKFVIO_OK) return rc;
    remove_applied(f, -k, k);
    ended_note_removal(f, k);
    if (removed) *removed = k;
    return EKFVIO_OK;
}

}  // extern "C"
