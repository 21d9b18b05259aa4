// ekf_vio_amd/csrc/ended.hip — the tracks that ended (ekfvio_set_ended_export, ekfvio_get_ended).  Not in the reference, which never
// removes a landmark.  A landmark that leaves the state takes a converged 3-D estimate and its covariance with it; the moment of removal
// is the only moment they can be handed out.  With the export on, every removal launch (remove.hip) is preceded by ONE launch of
// ended_tracks_kernel, which reads the removal's own decision and writes one record per landmark about to leave, in landmark order.
#include <string.h>

#include <algorithm>

#include "common.h"
#include "points.h"

namespace {

constexpr int EN_THREADS = 256;

struct EndedArgs {
    const float* mu;         // the mean and Sigma as they stand in front of the removal
    const float* P;
    int ld;
    const uint8_t* remove;   // the removal's decision per landmark: nonzero = leaves
    int N_host;              // landmarks the host knows of ...
    const int* added;        // ... plus these, from device memory (may be null), as the removal counts them
    int N_cap;               // max_features: what the arrays below have room for
    const int* info;         // non-null: info[0] bit 1 (the persistent sweep gave up) -> the removal removes nothing, nothing ends
    const int64_t* id;
    const double* born;
    int64_t* out_id;
    double* out_born;
    int* out_index;
    float* out_xyz;
    float* out_cov;
};

// One workgroup.  Each thread owns a run of consecutive landmarks (one each up to 256 landmarks), counts the leaving ones, the counts
// are scanned in LDS as scan_keep (remove.hip) scans the kept ones, and the thread then writes its records from its exclusive prefix on:
// record r is the r-th leaving landmark in landmark order, whatever the scheduling.  The record's values come from points_one and
// points_cov_one on the landmark's own slice of mu and Sigma: the bits ekfvio_get_points and ekfvio_get_points_covariance would return.
__global__ __launch_bounds__(EN_THREADS) void ended_tracks_kernel(EndedArgs a) {
    __shared__ int wsum[EN_THREADS];
    const int t = threadIdx.x;
    if (a.info && (a.info[0] & 2)) return;  // (uniform: every thread reads the same word)
    const int N = min(a.N_host + (a.added ? *a.added : 0), a.N_cap);
    const int chunk = (N + EN_THREADS - 1) / EN_THREADS;
    const int i0 = min(t * chunk, N), i1 = min(i0 + chunk, N);
    int c = 0;
    for (int i = i0; i < i1; i++) c += a.remove[i] != 0 ? 1 : 0;
    wsum[t] = c;
    __syncthreads();
    for (int s = 1; s < EN_THREADS; s <<= 1) {  // inclusive Hillis-Steele scan of the 256 counts
        const int v = t >= s ? wsum[t - s] : 0;
        __syncthreads();
        wsum[t] += v;
        __syncthreads();
    }
    int r = wsum[t] - c;
    for (int i = i0; i < i1; i++) {
        if (a.remove[i] == 0) continue;
        a.out_id[r] = a.id[i];
        a.out_born[r] = a.born[i];
        a.out_index[r] = i;
        // landmark i as landmark 0 of a state that starts 3 i entries further on
        float intensity;  // (no image: 0, not part of a record)
        points_one(a.mu + 3 * i, 0, nullptr, 0, 0, 0, 0.f, 0.f, 0.f, 0.f, a.out_xyz + 3 * (size_t)r, &intensity);
        points_cov_one(a.mu + 3 * i, a.P + (size_t)(3 * i) * a.ld + 3 * i, a.ld, 0, a.out_cov + 9 * (size_t)r);
        r++;
    }
}

}  // namespace

void launch_ended_tracks(ekfvio_filter* f, const uint8_t* remove, const int* added, bool abort_aware) {
    EndedArgs a;
    a.mu = f->mu, a.P = f->P, a.ld = f->ldp;
    a.remove = remove ? remove : f->del_flag;
    a.N_host = f->N, a.added = added, a.N_cap = f->cfg.max_features;
    a.info = abort_aware ? f->info : nullptr;
    a.id = f->lm_id, a.born = f->lm_born;
    a.out_id = f->ended_id, a.out_born = f->ended_born, a.out_index = f->ended_index, a.out_xyz = f->ended_xyz, a.out_cov = f->ended_cov;
    ProfScope ps(f, PC_UPDATE_MISC);  // (the handle's profile counts it: the one launch the export adds)
    hipLaunchKernelGGL(ended_tracks_kernel, dim3(1), dim3(EN_THREADS), 0, f->stream, a);
}

void ended_note_removal(ekfvio_filter* f, int removed) {
    if (!f->ended_on) return;
    f->ended_count = removed;
    f->ended_total += removed;
}

extern "C" {

int ekfvio_set_ended_export(ekfvio_filter* f, int32_t on) {
    if (!f || (on != 0 && on != 1)) return EKFVIO_EINVAL;
    if (on && !f->ended_id) {
        // the export's memory, ONE allocation made when a handle first asks for it (a handle that never does allocates and launches nothing
        // it did not before): pinned and device-mapped, as h_out -- the kernel writes the records straight into host memory, every removal
        // call waits for the stream behind it anyway, and ekfvio_get_ended is a memcpy.  The 8-byte arrays first
        HIP_TRY(f, hipSetDevice(f->device));
        const size_t maxf = (size_t)(f->cfg.max_features > 0 ? f->cfg.max_features : 1);
        HIP_TRY(f, host_alloc(f, &f->h_ended, maxf * (sizeof(int64_t) + sizeof(double) + 12 * sizeof(float) + sizeof(int)), MEM_PINNED_COHERENT));
        unsigned char* buf = nullptr;
        HIP_TRY(f, hipHostGetDevicePointer((void**)&buf, f->h_ended, 0));
        f->ended_id = reinterpret_cast<int64_t*>(buf);
        f->ended_born = reinterpret_cast<double*>(f->ended_id + maxf);
        f->ended_xyz = reinterpret_cast<float*>(f->ended_born + maxf);
        f->ended_cov = f->ended_xyz + 3 * maxf;
        f->ended_index = reinterpret_cast<int*>(f->ended_cov + 9 * maxf);
    }
    if ((on != 0) != f->ended_on) f->ended_count = 0;  // the report is of removals since the setting went on
    f->ended_on = on != 0;  // (read by the next removal; removals are in no captured graph)
    return EKFVIO_OK;
}

int ekfvio_get_ended(ekfvio_filter* f, int64_t* id, double* born, int32_t* index_before, float* xyz3, float* cov9, int32_t cap, int32_t* count,
                     int64_t* total) {
    if (!f) return EKFVIO_EINVAL;
    const int k = f->ended_on ? f->ended_count : 0;
    if (count) *count = k;
    if (total) *total = f->ended_total;
    if (cap < k) return EKFVIO_EINVAL;
    if (k == 0) return EKFVIO_OK;
    // (the records are in pinned host memory, and the removal call that wrote them has waited for the stream behind their kernel)
    const size_t maxf = (size_t)(f->cfg.max_features > 0 ? f->cfg.max_features : 1);
    const unsigned char* h = f->h_ended;
    if (id) memcpy(id, h, sizeof(int64_t) * k);
    if (born) memcpy(born, h + 8 * maxf, sizeof(double) * k);
    if (xyz3) memcpy(xyz3, h + 16 * maxf, sizeof(float) * 3 * k);
    if (cov9) memcpy(cov9, h + 28 * maxf, sizeof(float) * 9 * k);
    if (index_before) memcpy(index_before, h + 64 * maxf, sizeof(int32_t) * k);
    return EKFVIO_OK;
}

}  // extern "C"
