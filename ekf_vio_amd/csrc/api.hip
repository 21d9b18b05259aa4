// ekf_vio_amd/csrc/api.hip — the C-ABI of libekfvio_hip.so (include/ekfvio.h).
// Host-side orchestration only: every numeric step is a HIP kernel on the handle's stream.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>

#include <unistd.h>

#include "common.h"

// ---- the library's memory backend (mem.h): the ONLY calls of the runtime's allocation functions under csrc/ -------------------
static_assert((int)hipErrorOutOfMemory == MEM_ERR_OUT_OF_MEMORY && (int)hipSuccess == MEM_OK, "mem.h's codes are the runtime's");
namespace {
// what this copy of the library holds through every ledger, handles' and test hooks' alike (ekfvio_test_mem with a null handle)
struct MemTotal {
    std::atomic<int64_t> live{0}, live_bytes{0}, acquired{0}, released{0};
} g_mem_total[MEM_KINDS];
int hip_mem_allocate(MemKind kind, size_t bytes, void** out) {
    static const unsigned host_flags[MEM_KINDS] = {0, hipHostMallocDefault, hipHostMallocMapped, hipHostMallocMapped | hipHostMallocCoherent};
    void* p = nullptr;
    const hipError_t e = kind == MEM_DEVICE ? hipMalloc(&p, bytes) : hipHostMalloc(&p, bytes, host_flags[kind]);
    if (e != hipSuccess) return (int)e;
    g_mem_total[kind].live++, g_mem_total[kind].live_bytes += (int64_t)bytes, g_mem_total[kind].acquired++;
    *out = p;
    return MEM_OK;
}
void hip_mem_free(MemKind kind, void* p, size_t bytes) {
    (void)(kind == MEM_DEVICE ? hipFree(p) : hipHostFree(p));
    g_mem_total[kind].live--, g_mem_total[kind].live_bytes -= (int64_t)bytes, g_mem_total[kind].released++;
}
#ifdef EKFVIO_TEST_HOOKS
std::atomic<int> g_next_create_fail{0};  // ekfvio_test_mem_fail(NULL, k): armed on the ledger of the next ekfvio_create
#endif
}  // namespace
const MemBackend& hip_mem_backend() {
    static const MemBackend b = {hip_mem_allocate, hip_mem_free};
    return b;
}

namespace {

__global__ void init_sigma_kernel(float* P, int ld) {
    // initializeBaseState (TightlyCoupledEKF.cpp:23-56): diag [0x7, 30x9, 0.5x6]
    int i = threadIdx.x;
    if (i >= 7 && i <= 15) P[(size_t)i * ld + i] = 30.f;
    if (i >= 16 && i <= 21) P[(size_t)i * ld + i] = 0.5f;
}

// addNewFeatures (:58-94): new rows/columns are zero, new diagonal [hv, hv, dv]
// k_dev != nullptr: the count comes from device memory (the first-fit selection's result, ekfvio_step_image: the host
// learns it with the frame's status word, not in the middle of the frame)
__global__ void add_features_kernel(float* P, int ld, int n_old, int k, float hv, float dv, float* mu, float* last_klt,
                                    uint8_t* del_flag, const float* uv, int N_old, float inv_depth, const int* k_dev, int64_t* id,
                                    double* born, int64_t id_base, double stamp) {
    if (k_dev) k = *k_dev;
    const int n_new = n_old + 3 * k;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < (size_t)3 * k * n_new;
         e += (size_t)gridDim.x * blockDim.x) {
        int q = e / n_new;      // which new row/col
        int i = e % n_new;
        int s = n_old + q;
        P[(size_t)s * ld + i] = (i == s) ? ((q % 3 == 2) ? dv : hv) : 0.f;  // new column
        P[(size_t)i * ld + s] = (i == s) ? ((q % 3 == 2) ? dv : hv) : 0.f;  // new row
    }
    for (int fidx = blockIdx.x * blockDim.x + threadIdx.x; fidx < k; fidx += gridDim.x * blockDim.x) {
        float u = uv[2 * fidx], v = uv[2 * fidx + 1];
        mu[n_old + 3 * fidx] = u;
        mu[n_old + 3 * fidx + 1] = v;
        mu[n_old + 3 * fidx + 2] = inv_depth;
        last_klt[2 * (N_old + fidx)] = u;
        last_klt[2 * (N_old + fidx) + 1] = v;
        del_flag[N_old + fidx] = 0;
        id[N_old + fidx] = id_base + fidx;  // (the host advances its counter by k where it counts the landmarks in)
        born[N_old + fidx] = stamp;
    }
}

int count_rows(const uint8_t* pass, int N) {
    int c = 0;
    for (int i = 0; i < N; i++) c += pass[i] ? 1 : 0;
    return 2 * c;
}
}  // namespace

static const char* kProfNames[PC_COUNT] = {"linearize",   "predict_structured", "gemm_predict", "gather",
                                           "cholesky",    "solve",              "gemm_update",  "update_misc",
                                           "klt_pyramid", "klt_track"};

// addNewFeatures (:58-94) with the `count` new (u,v) pairs already in f->zmeas on the device
int add_features_device(ekfvio_filter* f, int count) {
    if (count <= 0) return EKFVIO_OK;
    if (f->N + count > f->cfg.max_features) return EKFVIO_ECAPACITY;
    const float depth = f->cfg.default_point_depth;
    const float inv_depth = (float)(1.0 / (double)depth);  // Feature.cpp:18  mu(2) = 1.0/depth
    hipLaunchKernelGGL(add_features_kernel, dim3(64), dim3(256), 0, f->stream, f->P, f->ldp, f->n, count,
                       f->cfg.default_point_homogenous_variance, f->cfg.default_point_depth_variance, f->mu,
                       f->last_klt, f->del_flag, f->zmeas, f->N, inv_depth, nullptr, f->lm_id, f->lm_born, f->next_id, born_stamp(f));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    f->N += count;
    f->n += 3 * count;
    f->next_id += count;
    return EKFVIO_OK;
}
// The same with the count in device memory (at most max_features - N, by construction of the selection): enqueued only.
// The caller adds the count to f->N / f->n and to f->next_id once it has read it (wait_status's extra word).
void add_features_enqueue_device_count(ekfvio_filter* f, const int* count_dev) {
    const float inv_depth = (float)(1.0 / (double)f->cfg.default_point_depth);
    hipLaunchKernelGGL(add_features_kernel, dim3(64), dim3(256), 0, f->stream, f->P, f->ldp, f->n, 0,
                       f->cfg.default_point_homogenous_variance, f->cfg.default_point_depth_variance, f->mu,
                       f->last_klt, f->del_flag, f->zmeas, f->N, inv_depth, count_dev, f->lm_id, f->lm_born, f->next_id, born_stamp(f));
}

// one workgroup; publishes the status word itself once its own writes are out (see wait_status / poll_status)
__global__ void copy_small_kernel(const float* __restrict__ src, float* __restrict__ dst, int n, const int* __restrict__ info,
                                  int* host_word, int seq) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) publish_host_words(host_word, info, 0, seq);
}

// The host's wait at the end of a frame.  A one-thread kernel behind everything else on the stream writes the status
// word and a sequence number straight into pinned host memory; the host polls the sequence number.  Against a 4-byte
// device-to-host copy plus hipStreamSynchronize this saves the copy's command and the interrupt-driven wake-up (≈10 us
// per frame).  Polling is bounded: after 300 us (a long device-resident run is in flight) the host blocks in
// hipStreamSynchronize like before.
__global__ void publish_status_kernel(const int* __restrict__ info, int* host_word, int seq, const int* __restrict__ extra) {
    publish_host_words(host_word, info, extra ? *extra : 0, seq);
}
void launch_publish_status(ekfvio_filter* f, int seq) {
    hipLaunchKernelGGL(publish_status_kernel, dim3(1), dim3(1), 0, f->stream, f->info, f->d_hinfo, seq, (const int*)nullptr);
}
int wait_status(ekfvio_filter* f, int* status, const int* extra_dev, int* extra_out) {
    const int seq = ++f->status_seq;
    hipLaunchKernelGGL(publish_status_kernel, dim3(1), dim3(1), 0, f->stream, f->info, f->d_hinfo, seq, extra_dev);
    return poll_status(f, seq, status, extra_out);
}
// The polling half: for a caller whose own last kernel publishes sequence number `seq` (from next_status_seq).
int next_status_seq(ekfvio_filter* f) { return ++f->status_seq; }
int poll_status(ekfvio_filter* f, int seq, int* status, int* extra_out) {
    HIP_TRY(f, hipGetLastError());
    volatile int* hw = f->h_info;
    const auto t0 = std::chrono::steady_clock::now();
    int spins = 0;
    while (__atomic_load_n(&hw[HW_SEQ], __ATOMIC_ACQUIRE) != seq) {
        if ((++spins & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(300)) {
            HIP_TRY(f, hipStreamSynchronize(f->stream));
            break;
        }
    }
    if (__atomic_load_n(&hw[HW_SEQ], __ATOMIC_ACQUIRE) != seq) {
        f->last_error = "status word not published";
        return EKFVIO_EDEVICE;
    }
    *status = hw[HW_STATUS];
    if (extra_out) *extra_out = hw[HW_EXTRA];
    return EKFVIO_OK;
}

extern "C" {

int ekfvio_default_config(ekfvio_config* c) {
    if (!c) return EKFVIO_EINVAL;
    c->max_features = 100;                        // D_NUM_FEATURES
    c->default_point_depth = 0.5f;                // D_DEFAULT_POINT_DEPTH
    c->default_point_depth_variance = 100.f;      // D_DEFAULT_POINT_DEPTH_VARIANCE
    c->default_point_homogenous_variance = 1e-5f; // D_DEFAULT_POINT_HOMOGENOUS_VARIANCE
    c->predict_mode = EKFVIO_PREDICT_STRUCTURED;
    c->klt_window_size = 21;
    c->klt_max_pyramid_level = 3;
    c->klt_max_iterations = 30;
    c->klt_epsilon = 0.01f;
    c->klt_min_eigen = 1e-4f;
    c->kill_pad = 11;
    c->max_image_width = 640;
    c->max_image_height = 480;
    c->use_principal_point = 0;
    c->inverse_image_scale = 1;   // D_INVERSE_IMAGE_SCALE is 4; 1 = the caller hands over frames already at working size
    c->fast_threshold = 50;       // D_FAST_THRESHOLD
    c->min_new_feature_dist = 30; // D_MIN_NEW_FEATURE_DIST
    c->fast_blur_sigma = 0.f;     // D_FAST_BLUR_SIGMA (0 = no blur)
    c->replenish = 0;             // 1: ekfvio_step_image runs replenishFeatures (EKFVIO.cpp:154,172) itself
    c->sample_based_uncertainty = 0;  // reference behaviour: estimateUncertainty's constant (KLTTracker.cpp:100-106)
    c->use_imu = 0;                   // reference behaviour: imu_callback only logs (EKFVIO.cpp:113-115)
    c->imu_gyro_variance = 1e-4f;
    c->imu_accel_variance = 1e-2f;
    c->gravity[0] = 0.f;
    c->gravity[1] = 9.81f;
    c->gravity[2] = 0.f;
    c->klt_fb_max_px = 0.f;           // reference behaviour: no forward-backward check of the tracker's results
    c->remove_lost = 0;               // reference behaviour: a lost landmark stays in the state, flagged (TightlyCoupledEKF.cpp:528)
    return EKFVIO_OK;
}

static int create_body(ekfvio_filter* f, const ekfvio_config* cfg, int device, void* stream) {
    HIP_TRY(f, hipSetDevice(device));
    if (stream) {
        f->stream = (hipStream_t)stream;
    } else {
        HIP_TRY(f, hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
        f->own_stream = true;
    }
    const int maxf = cfg->max_features;
    const FilterDims dims = filter_dims(maxf);  // (plan.h)
    f->n_cap = dims.n_cap, f->ldp = dims.ldp, f->m_cap = dims.m_cap, f->ld_aug = dims.ld_aug, f->sweep_sync_words = dims.sweep_sync_words;
    f->tune = tuning_from_env();  // every switch, once per handle
    const size_t pp = (size_t)f->ldp * f->ldp, pm = (size_t)f->ldp * f->m_cap;
    HIP_TRY(f, dev_alloc(f, &f->mu, f->ldp));
    HIP_TRY(f, dev_alloc(f, &f->mu_next, f->ldp));
    HIP_TRY(f, dev_alloc(f, &f->last_klt, 2 * (size_t)maxf));
    HIP_TRY(f, dev_alloc(f, &f->del_flag, (size_t)maxf));
    HIP_TRY(f, dev_alloc(f, &f->lm_id, (size_t)maxf));
    HIP_TRY(f, dev_alloc(f, &f->lm_born, (size_t)maxf));
    HIP_TRY(f, dev_alloc(f, &f->P, pp));
    HIP_TRY(f, dev_alloc(f, &f->P2, pp));
    HIP_TRY(f, dev_alloc(f, &f->FA, EKF_BASE * EKF_BASE));
    HIP_TRY(f, dev_alloc(f, &f->FB, 27 * (size_t)maxf));
    HIP_TRY(f, dev_alloc(f, &f->FD, 9 * (size_t)maxf));
    HIP_TRY(f, dev_alloc(f, &f->Fdense, pp));
    HIP_TRY(f, dev_alloc(f, &f->idx, (size_t)f->m_cap));
    HIP_TRY(f, dev_alloc(f, &f->inv_idx, (size_t)f->ldp));
    HIP_TRY(f, dev_alloc(f, &f->zmeas, 2 * (size_t)maxf));
    HIP_TRY(f, dev_alloc(f, &f->Rmeas, 4 * (size_t)maxf));
    HIP_TRY(f, dev_alloc(f, &f->pass, (size_t)maxf));
    HIP_TRY(f, dev_alloc(f, &f->yres, (size_t)f->m_cap));
    HIP_TRY(f, dev_alloc(f, &f->Rm, 2 * (size_t)f->m_cap));
    HIP_TRY(f, dev_alloc(f, &f->Saug, (size_t)f->ld_aug * f->m_cap));
    HIP_TRY(f, dev_alloc(f, &f->Laug, (size_t)f->ld_aug * f->m_cap));
    HIP_TRY(f, dev_alloc(f, &f->Linv, 64 * (size_t)f->m_cap));
    HIP_TRY(f, dev_alloc(f, &f->Lsign, (size_t)(f->m_cap / 64 > 256 ? f->m_cap / 64 : 256)));  // 256: the raw-solve test hook goes up to m = 16384
    HIP_TRY(f, dev_alloc(f, &f->sweep_sync, f->sweep_sync_words));  // flags of the persistent sweeps (chol_persist.inc)
    {
        hipDeviceProp_t prop;
        HIP_TRY(f, hipGetDeviceProperties(&prop, device));
        f->num_cus = prop.multiProcessorCount;
    }
    HIP_TRY(f, dev_alloc(f, &f->Km, pm));
    HIP_TRY(f, dev_alloc(f, &f->Wt, pm));
    HIP_TRY(f, dev_alloc(f, &f->Gm, pm));
    HIP_TRY(f, dev_alloc(f, &f->info, 4));
    HIP_TRY(f, dev_alloc(f, &f->remove_words, 4));
    HIP_TRY(f, host_alloc(f, &f->h_info, 16 * sizeof(int), MEM_PINNED_COHERENT));
    memset(f->h_info, 0, 16 * sizeof(int));
    HIP_TRY(f, hipHostGetDevicePointer((void**)&f->d_hinfo, f->h_info, 0));
    {
        const size_t words = out_words(f);
        HIP_TRY(f, host_alloc(f, &f->h_out, words * sizeof(float), MEM_PINNED_COHERENT));
        HIP_TRY(f, hipHostGetDevicePointer((void**)&f->d_out, f->h_out, 0));
    }
    {
        const size_t cap = (size_t)(f->cfg.max_features > 0 ? f->cfg.max_features : 1);
        HIP_TRY(f, host_alloc(f, &f->h_meas, 25 * cap, MEM_PINNED));
        HIP_TRY(f, dev_alloc_bare(f, &f->d_meas, 25 * cap));
    }
    HIP_TRY(f, hipEventCreate(&f->ev0));
    HIP_TRY(f, hipEventCreate(&f->ev1));
    int rc = klt_alloc(f);
    if (rc != EKFVIO_OK) return rc;
    rc = fast_alloc(f);
    if (rc != EKFVIO_OK) return rc;
    return ekfvio_reset(f);
}

}  // extern "C"

// Live handles per device in this process.  The persistent sweep needs all its workgroups resident together; two such
// launches from different handles' streams can each get part of the compute units and wait for workgroups the other one
// keeps out (every wait is bounded, but that ends in an aborted update, not in a result).  It is therefore used only by
// a device's sole handle; with several handles on a device every one of them takes one launch per block step.
// Live handles per device, PROCESS-wide: the product library and the hooks build of the same sources can be loaded into one
// process (the tests do; a node that links one and dlopens a tool built on the other could), each with its own statics -- two copies of a
// per-library count would each see a "sole handle" and let two persistent launches loose on one device.  The first copy to need the
// registry allocates it and leaves its address in the process environment under a name that carries the pid (so a forked child's or an
// exec'ed program's copy of the variable is ignored); every later copy picks it up there.  No exported symbol, no file.
static std::atomic<int>* live_registry() {
    static std::atomic<int>* reg = [] {
        char name[64], val[32];
        snprintf(name, sizeof(name), "EKFVIO_LIVE_HANDLES_%ld", (long)getpid());
        if (const char* e = getenv(name)) {
            void* p = nullptr;
            if (sscanf(e, "%p", &p) == 1 && p) return static_cast<std::atomic<int>*>(p);
        }
        auto* a = new std::atomic<int>[64];
        for (int i = 0; i < 64; i++) a[i].store(0, std::memory_order_relaxed);
        snprintf(val, sizeof(val), "%p", static_cast<void*>(a));
        setenv(name, val, 1);
        return a;
    }();
    return reg;
}
int live_handles_on(int device) { return (device >= 0 && device < 64) ? live_registry()[device].load(std::memory_order_relaxed) : 2; }

void drop_graph(ekfvio_filter* f) {
    for (GraphCache::Entry& e : f->graphs.g) {
        if (e.exec) (void)hipGraphExecDestroy(e.exec);
        e = GraphCache::Entry();
    }
}
// What `body` enqueues on the handle's stream as an executable graph: the stream is drained, the launches are recorded (thread-local capture:
// nothing runs) and instantiated.  Whatever host state the body's launchers mirror of the device is the caller's to put back.
template <class Body>
static int capture_graph(ekfvio_filter* f, hipGraphExec_t* out, Body body) {
    hipGraph_t g = nullptr;
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    HIP_TRY(f, hipStreamBeginCapture(f->stream, hipStreamCaptureModeThreadLocal));
    body();
    const hipError_t ce = hipStreamEndCapture(f->stream, &g);
    if (ce != hipSuccess || !g) {
        f->last_error = std::string("graph capture: ") + hipGetErrorString(ce);
        return EKFVIO_EDEVICE;
    }
    HIP_TRY(f, hipGraphInstantiate(out, g, nullptr, nullptr, 0));
    (void)hipGraphDestroy(g);
    return EKFVIO_OK;
}

extern "C" {

int ekfvio_create(const ekfvio_config* cfg, int device, void* stream, ekfvio_filter** out) {
    if (!out) return EKFVIO_EINVAL;
    *out = nullptr;
    if (!cfg || cfg->max_features < 0) return EKFVIO_EINVAL;
    if (cfg->remove_lost != 0 && cfg->remove_lost != 1) return EKFVIO_EINVAL;
    if (cfg->remove_lost && (size_t)cfg->max_features * 17 > 64 * 1024) return EKFVIO_ECAPACITY;  // the removal kernel's LDS (remove.hip)
    if (!(cfg->klt_fb_max_px >= 0.f)) return EKFVIO_EINVAL;  // (negative, NaN)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return EKFVIO_EDEVICE;
    ekfvio_filter* f = new ekfvio_filter();
#ifdef EKFVIO_TEST_HOOKS
    f->mem.fail_nth(g_next_create_fail.exchange(0));
#endif
    f->cfg = *cfg;
    for (int k = 0; k < 3; k++) f->imu_gravity[k] = cfg->gravity[k];  // until ekfvio_set_gravity says otherwise
    f->device = device;
    if (device < 64) live_registry()[device].fetch_add(1, std::memory_order_relaxed);
    const int rc = create_body(f, cfg, device, stream);
    if (rc != EKFVIO_OK) {
        // a half-built handle never leaves the library: whatever its ledger holds is released here
        fprintf(stderr, "ekfvio_create: %s\n", f->last_error.c_str());
        (void)ekfvio_destroy(f);
        return rc;
    }
    *out = f;
    return EKFVIO_OK;
}

int ekfvio_destroy(ekfvio_filter* f) {
    if (!f) return EKFVIO_EINVAL;
    (void)hipSetDevice(f->device);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    drop_graph(f);
    f->mem.release_all();  // every buffer of the handle, whichever file acquired it and whichever field holds it now
    if (f->ev0) hipEventDestroy(f->ev0);
    if (f->ev1) hipEventDestroy(f->ev1);
    if (f->own_stream && f->stream) hipStreamDestroy(f->stream);
    if (f->device >= 0 && f->device < 64) live_registry()[f->device].fetch_sub(1, std::memory_order_relaxed);
    delete f;
    return EKFVIO_OK;
}

const char* ekfvio_last_error(const ekfvio_filter* f) {
    return f ? f->last_error.c_str() : "null handle (a failed ekfvio_create leaves none behind: its return code says why)";
}

int ekfvio_reset(ekfvio_filter* f) {
    if (!f) return EKFVIO_EINVAL;
    f->out_fresh = false;
    HIP_TRY(f, hipSetDevice(f->device));
    f->N = 0;
    f->n = EKF_BASE;
    HIP_TRY(f, hipMemsetAsync(f->P, 0, sizeof(float) * (size_t)f->ldp * f->ldp, f->stream));
    HIP_TRY(f, hipMemsetAsync(f->P2, 0, sizeof(float) * (size_t)f->ldp * f->ldp, f->stream));  // ping-pong partner: padding must be zero
    HIP_TRY(f, hipMemsetAsync(f->mu, 0, sizeof(float) * f->ldp, f->stream));
    const float one = 1.f;
    HIP_TRY(f, hipMemcpyAsync(f->mu + 3, &one, sizeof(float), hipMemcpyHostToDevice, f->stream));
    hipLaunchKernelGGL(init_sigma_kernel, dim3(1), dim3(32), 0, f->stream, f->P, f->ldp);
    HIP_TRY(f, hipMemsetAsync(f->info, 0, 4 * sizeof(int), f->stream));
    if (f->gate_words) HIP_TRY(f, hipMemsetAsync(f->gate_words, 0, 4 * sizeof(int), f->stream));  // the gate's counts start over; its threshold stays
    if (f->fb_words) HIP_TRY(f, hipMemsetAsync(f->fb_words, 0, 8 * sizeof(int), f->stream));  // ... and the forward-backward check's, likewise
    HIP_TRY(f, aid_reset_enqueue(f));  // ... and the aiding measurement's verdict and counts; the standing measurement stays (ekfvio_set_frame_aid)
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    aid_reset_done(f);
    f->have_stamp = false;
    f->frames[0].valid = f->frames[1].valid = false;
    f->mask_hits_n = 0;  // the mask's hits of the last track go with the landmarks; the mask itself stays (ekfvio_set_mask)
    // next_id goes on: no two landmarks of a handle's lifetime share an id.  The ended tracks' report and total start over; the setting stays
    f->ended_count = 0, f->ended_total = 0;
    // ... and so do the zero-velocity update's report and total (ekfvio_set_zupt)
    f->zupt_n = f->zupt_pass = f->zupt_still = f->zupt_applied_last = 0, f->zupt_applied_total = 0;
    return EKFVIO_OK;
}

int ekfvio_add_features(ekfvio_filter* f, const float* uv, int32_t count) {
    if (!f || count < 0 || (count > 0 && !uv)) return EKFVIO_EINVAL;
    f->out_fresh = false;
    if (count == 0) return EKFVIO_OK;  // reference: early return (:59)
    if (f->N + count > f->cfg.max_features) return EKFVIO_ECAPACITY;
    HIP_TRY(f, hipSetDevice(f->device));
    // stage uv through the (free between updates) zmeas buffer in chunks of max_features
    HIP_TRY(f, hipMemcpyAsync(f->zmeas, uv, sizeof(float) * 2 * count, hipMemcpyHostToDevice, f->stream));
    return add_features_device(f, count);
}

int ekfvio_process(ekfvio_filter* f, float dt) {
    if (!f || !(dt >= 0.f)) return EKFVIO_EINVAL;  // ROS_ASSERT(dt >= 0) EKFVIO.cpp:162
    f->out_fresh = false;
    HIP_TRY(f, hipSetDevice(f->device));
    launch_predict(f, dt);
    HIP_TRY(f, hipGetLastError());
    return EKFVIO_OK;
}

int ekfvio_linearize(ekfvio_filter* f, float dt, float* F_dense) {
    if (!f || !F_dense) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    launch_linearize(f, dt);
    launch_build_dense_F(f, f->Fdense);
    HIP_TRY(f, hipMemcpy2DAsync(F_dense, sizeof(float) * f->n, f->Fdense, sizeof(float) * f->ldp, sizeof(float) * f->n,
                             f->n, hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    return EKFVIO_OK;
}

}  // extern "C"

// The status word f->info[0]: bit 0 = a non-positive pivot was met (a warning: the reference logs and carries on,
// TightlyCoupledEKF.cpp:577-580), bit 1 = the persistent sweep ran out of patience (its workgroups were not all
// resident: another process or stream held compute units).  Behind an aborted sweep the Joseph GEMMs write nothing, so
// Sigma, mu and the frame counter stand where process(dt) left them, and the handle stops using the persistent launch.
void sweep_abort_latch(ekfvio_filter* f) {
    f->sweep_latched_off = true;  // the following sweeps of this handle: one launch per block step (no co-residency needed)
    drop_graph(f);      // captured steps contain the persistent launch
    // ... and a way back: what kept the workgroups from being resident -- another process or stream on the device, a
    // compute-unit mask -- may be gone later.  The persistent launch is tried again after a pause that doubles with every abort
    // (2 s, 4 s, ... 64 s), checked at the entry points that enqueue updates (sweep_maybe_retry).
    f->sweep_retry_pause_s = f->sweep_retry_pause_s <= 0 ? f->tune.sweep_retry_first_s : std::min(64.0, 2.0 * f->sweep_retry_pause_s);
    f->sweep_retry_at = std::chrono::steady_clock::now() + std::chrono::milliseconds((long long)(1e3 * f->sweep_retry_pause_s));
    f->sweep_retry_armed = true;
}
// Called ONLY from the entry points that can run an aborted update again (ekfvio_update, ekfvio_step_image): a retry that fails costs
// one recovery there, nothing else.
void sweep_maybe_retry(ekfvio_filter* f) {
    if (!f->sweep_retry_armed || !f->sweep_latched_off || std::chrono::steady_clock::now() < f->sweep_retry_at) return;
    f->sweep_retry_armed = false;
    f->sweep_latched_off = false;
    f->sweep_probation = 8;  // clean persistent sweeps until the pause starts from its first value again (sweep_clean_update)
    drop_graph(f);  // captured steps contain the per-step sweep
    // the flags AND the abort word (which no kernel ever zeroes) start from zero again
    (void)hipMemsetAsync(f->sweep_sync, 0, sizeof(int) * f->sweep_sync_words, f->stream);
    f->sweep_flags_clean = false;
}
// An update whose persistent sweep came through: after a few of them in a row behind a retry the pause of the NEXT abort starts from
// its first value again (it only ever doubled, so a handle that met a few transient aborts early waited 64 s on the slow
// sweep after any later one, even after hours of clean persistent sweeps).
void sweep_clean_update(ekfvio_filter* f) {
    if (f->sweep_probation > 0 && f->tune.persist_sweep && !f->sweep_latched_off && --f->sweep_probation == 0) f->sweep_retry_pause_s = 0.0;
}
// The host's end of an update (common.h).  read_status waits for the stream's work up to the publishing launch and reads the status
// word; a word that was set is cleared on the device for the next update.
int read_status(ekfvio_filter* f, int seq, const int* extra_dev, int* bad, int* extra) {
    const int rc = seq ? poll_status(f, seq, bad, extra) : wait_status(f, bad, extra_dev, extra);  // (seq: the caller's launches publish it)
    if (rc != EKFVIO_OK) return rc;
    if (*bad) HIP_TRY(f, hipMemsetAsync(f->info, 0, sizeof(int), f->stream));
    return EKFVIO_OK;
}
// An aborted update is enqueued again by `rerun` (null: the caller cannot, e.g. a graph replay of many steps: EKFVIO_EABORTED) with
// the per-step sweep and awaited: fresh launches, same inputs, and the state comes out as if the per-step sweep had run in the first place.
int settle_update(ekfvio_filter* f, int bad, void (*rerun)(ekfvio_filter*, void*), void* ctx, bool counts_as_clean) {
    if (bad & 2) {
        sweep_abort_latch(f);
        if (!rerun) {
            f->last_error = "persistent sweep aborted (compute units shared with other work): updates behind it were skipped, the state is "
                            "the propagated one; this handle now takes one launch per block step";
            return EKFVIO_EABORTED;
        }
        f->sweep_recoveries++;
        f->out_fresh = false;  // (outputs that went out with the aborted update's status are the propagated state's)
        rerun(f, ctx);
        HIP_TRY(f, hipGetLastError());
        const int rc = read_status(f, 0, nullptr, &bad, nullptr);
        if (rc != EKFVIO_OK) return rc;
        if (bad & 2) return EKFVIO_EABORTED;  // (cannot happen: the per-step sweep has no waits)
    } else if (counts_as_clean) sweep_clean_update(f);
    return (bad & 1) ? EKFVIO_ENUMERIC : EKFVIO_OK;
}

extern "C" {

int ekfvio_update(ekfvio_filter* f, const float* z, const float* R, const uint8_t* pass, int32_t count) {
    if (!f || count != f->N) return EKFVIO_EINVAL;  // ROS_ASSERT :478
    f->out_fresh = false;
    if (count > 0 && (!z || !R || !pass)) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    sweep_maybe_retry(f);
    const int m = count_rows(pass, count);
    // the frame's three host arrays travel as ONE copy from pinned memory (three pageable copies cost ~25 us per step);
    // the previous call's synchronisation (read_status) guarantees the staging buffer is free
    const size_t cap = (size_t)(f->cfg.max_features > 0 ? f->cfg.max_features : 1);
    float* dz = reinterpret_cast<float*>(f->d_meas);
    float* dR = reinterpret_cast<float*>(f->d_meas + 8 * cap);
    uint8_t* dp = f->d_meas + 24 * cap;
    if (count > 0) {
        memcpy(f->h_meas, z, sizeof(float) * 2 * count);
        memcpy(f->h_meas + 8 * cap, R, sizeof(float) * 4 * count);
        memcpy(f->h_meas + 24 * cap, pass, count);
        HIP_TRY(f, hipMemcpyAsync(f->d_meas, f->h_meas, 24 * cap + count, hipMemcpyHostToDevice, f->stream));
    }
    // The status of an update -- a non-positive pivot, a sweep that gave up -- is final when the Cholesky sweep is: the status word goes to
    // the host right behind the sweep, and the call returns while the two Joseph GEMMs are still running (everything the caller can do next
    // is ordered behind them on the handle's stream, or synchronises).  A step-by-step caller then keeps the GPU fed: the next step's
    // launches are in the queue before this step's last kernel ends (EKFVIO_EARLY_STATUS=0: publish behind the last kernel, as rounds 1-3).
    const bool early = f->tune.early_status != 0;  // (per handle, read at create like every other knob: ADVICE r04)
    const int seq = next_status_seq(f);
    UpdateInputs in;
    in.m = m, in.z = dz, in.R = dR, in.pass = dp;
    in.publish_seq = early ? seq : 0;
    if (!launch_update(f, in).published) launch_publish_status(f, seq);  // (not early, or no sweep ran: nothing was published yet)
    HIP_TRY(f, hipGetLastError());
    in.publish_seq = 0;
    in.gate_counted = true;  // (a re-run gates the same propagated state again: same verdicts, counted once)
    int bad = 0;
    const int rc = read_status(f, seq, nullptr, &bad, nullptr);
    if (rc != EKFVIO_OK) return rc;
    return settle_update(f, bad, [](ekfvio_filter* g, void* c) {
        launch_update(g, *static_cast<const UpdateInputs*>(c));  // the staged measurement is still in d_meas; the bookkeeping is idempotent
    }, &in, true);  // (clean whenever it did not abort, an update without landmarks included)
}

int ekfvio_measurement_map(const ekfvio_filter* f, const uint8_t* measured, int32_t count, int32_t* idx, int32_t* rows) {
    if (!f || !measured || !idx || !rows || count != f->N) return EKFVIO_EINVAL;  // ROS_ASSERT :636
    int r = 0;
    for (int i = 0; i < count; i++)
        if (measured[i]) {
            idx[r++] = EKF_BASE + 3 * i;
            idx[r++] = EKF_BASE + 3 * i + 1;
        }
    *rows = r;
    return EKFVIO_OK;
}

int ekfvio_num_features(const ekfvio_filter* f) { return f ? f->N : -1; }
int ekfvio_dim(const ekfvio_filter* f) { return f ? f->n : -1; }

int ekfvio_get_base_mu(ekfvio_filter* f, float* base_mu) {
    if (!f || !base_mu) return EKFVIO_EINVAL;
    if (f->out_fresh) {  // written with the frame's status word (ekfvio_step_image): nothing to launch, nothing to wait for
        memcpy(base_mu, f->h_out, sizeof(float) * EKF_BASE);
        return EKFVIO_OK;
    }
    HIP_TRY(f, hipSetDevice(f->device));
    // 22 floats: written by a kernel straight into pinned host memory and awaited like the status word (the node reads
    // its odometry every frame: a device-to-host copy into pageable memory plus a synchronise cost three times as much)
    const int seq = next_status_seq(f);
    hipLaunchKernelGGL(copy_small_kernel, dim3(1), dim3(64), 0, f->stream, f->mu, f->d_out, EKF_BASE, f->info, f->d_hinfo, seq);
    int bad = 0;
    const int rc = poll_status(f, seq, &bad, nullptr);
    if (rc != EKFVIO_OK) return rc;
    memcpy(base_mu, f->h_out, sizeof(float) * EKF_BASE);
    return EKFVIO_OK;
}

int ekfvio_get_features(ekfvio_filter* f, float* mu3N, float* last_klt2N, uint8_t* delN) {
    if (!f) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    if (f->N > 0) {
        if (mu3N) HIP_TRY(f, hipMemcpyAsync(mu3N, f->mu + EKF_BASE, sizeof(float) * 3 * f->N, hipMemcpyDeviceToHost, f->stream));
        if (last_klt2N) HIP_TRY(f, hipMemcpyAsync(last_klt2N, f->last_klt, sizeof(float) * 2 * f->N, hipMemcpyDeviceToHost, f->stream));
        if (delN) HIP_TRY(f, hipMemcpyAsync(delN, f->del_flag, f->N, hipMemcpyDeviceToHost, f->stream));
    }
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    return EKFVIO_OK;
}

int ekfvio_get_sigma(ekfvio_filter* f, float* sigma, int32_t ld) {
    if (!f || !sigma || ld < f->n) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    HIP_TRY(f, hipMemcpy2DAsync(sigma, sizeof(float) * ld, f->P, sizeof(float) * f->ldp, sizeof(float) * f->n, f->n,
                             hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    return EKFVIO_OK;
}

int ekfvio_get_feature_cov(ekfvio_filter* f, int32_t index, float cov[4]) {
    if (!f || !cov || index < 0 || index >= f->N) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    const int s = EKF_BASE + 3 * index;  // Sigma.block(start,start,2,2), column-major out
    HIP_TRY(f, hipMemcpy2DAsync(cov, sizeof(float) * 2, f->P + (size_t)s * f->ldp + s, sizeof(float) * f->ldp,
                             sizeof(float) * 2, 2, hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    return EKFVIO_OK;
}

int ekfvio_get_depth_variance(ekfvio_filter* f, int32_t index, float* var) {
    if (!f || !var || index < 0 || index >= f->N) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    const int s = EKF_BASE + 3 * index + 2;
    HIP_TRY(f, hipMemcpyAsync(var, f->P + (size_t)s * f->ldp + s, sizeof(float), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    return EKFVIO_OK;
}

// setFeatureHomogenousCovariance (TightlyCoupledEKF.cpp:668-676): the four coeffRef writes of the (u,v) block
int ekfvio_set_feature_cov(ekfvio_filter* f, int32_t index, const float cov[4]) {
    if (!f || !cov || index < 0 || index >= f->N) return EKFVIO_EINVAL;
    f->out_cov_fresh = false;  // (the mean and the cloud stay what they are: out_fresh is kept)
    HIP_TRY(f, hipSetDevice(f->device));
    const int s = EKF_BASE + 3 * index;  // column-major in, column-major block of Sigma out
    HIP_TRY(f, hipMemcpy2DAsync(f->P + (size_t)s * f->ldp + s, sizeof(float) * f->ldp, cov, sizeof(float) * 2, sizeof(float) * 2, 2,
                             hipMemcpyHostToDevice, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));  // cov is the caller's memory
    return EKFVIO_OK;
}

// getMetric2PixelMap / getPixel2MetricMap (TightlyCoupledEKF.cpp:683-697): J = diag(K(0,0), K(1,1)) and
// diag(1.0f / K(0,0), 1.0f / K(1,1)) -- proper 2-D indexing of K here (unlike Feature.h:60-66), no state involved.
int ekfvio_metric2pixel_map(const float K[9], float J[4]) {
    if (!K || !J) return EKFVIO_EINVAL;
    J[0] = K[0]; J[1] = 0.f; J[2] = 0.f; J[3] = K[4];
    return EKFVIO_OK;
}
int ekfvio_pixel2metric_map(const float K[9], float J[4]) {
    if (!K || !J) return EKFVIO_EINVAL;
    J[0] = 1.0f / K[0]; J[1] = 0.f; J[2] = 0.f; J[3] = 1.0f / K[4];
    return EKFVIO_OK;
}

// publishOdometry's payload (EKFVIO.cpp:444-477): the slices of base_mu the message is filled from
int ekfvio_get_odometry(ekfvio_filter* f, float position[3], float orientation_wxyz[4], float linear[3], float angular[3]) {
    if (!f) return EKFVIO_EINVAL;
    float b[EKF_BASE];
    const int rc = ekfvio_get_base_mu(f, b);
    if (rc != EKFVIO_OK) return rc;
    for (int i = 0; i < 3; i++) {
        if (position) position[i] = b[i];
        if (linear) linear[i] = b[7 + i];
        if (angular) angular[i] = b[10 + i];
    }
    if (orientation_wxyz)
        for (int i = 0; i < 4; i++) orientation_wxyz[i] = b[3 + i];
    return EKFVIO_OK;
}

int ekfvio_check_sigma(ekfvio_filter* f, float* min_diag, float* max_asym) {
    if (!f || !min_diag || !max_asym) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    launch_check_sigma(f, f->yres);  // yres is free between updates
    float out[2];
    HIP_TRY(f, hipMemcpyAsync(out, f->yres, 2 * sizeof(float), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    *min_diag = out[0];
    *max_asym = out[1];
    return EKFVIO_OK;
}

int ekfvio_set_state(ekfvio_filter* f, int32_t N, const float* base_mu, const float* mu3N, const float* last_klt2N,
                     const uint8_t* delN, const float* sigma, int32_t ld) {
    if (!f || N < 0 || !base_mu || !sigma) return EKFVIO_EINVAL;
    f->out_fresh = false;
    if (N > f->cfg.max_features) return EKFVIO_ECAPACITY;
    const int n = EKF_BASE + 3 * N;
    if (ld < n || (N > 0 && (!mu3N || !last_klt2N || !delN))) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    HIP_TRY(f, hipMemsetAsync(f->P, 0, sizeof(float) * (size_t)f->ldp * f->ldp, f->stream));
    HIP_TRY(f, hipMemsetAsync(f->P2, 0, sizeof(float) * (size_t)f->ldp * f->ldp, f->stream));
    HIP_TRY(f, hipMemsetAsync(f->mu, 0, sizeof(float) * f->ldp, f->stream));
    HIP_TRY(f, hipMemcpyAsync(f->mu, base_mu, sizeof(float) * EKF_BASE, hipMemcpyHostToDevice, f->stream));
    if (N > 0) {
        HIP_TRY(f, hipMemcpyAsync(f->mu + EKF_BASE, mu3N, sizeof(float) * 3 * N, hipMemcpyHostToDevice, f->stream));
        HIP_TRY(f, hipMemcpyAsync(f->last_klt, last_klt2N, sizeof(float) * 2 * N, hipMemcpyHostToDevice, f->stream));
        HIP_TRY(f, hipMemcpyAsync(f->del_flag, delN, N, hipMemcpyHostToDevice, f->stream));
    }
    // the landmark set is replaced: all N get fresh ids, in order, and the handle's current time as their birth stamp
    std::vector<int64_t> ids((size_t)N);
    const std::vector<double> born((size_t)N, born_stamp(f));
    for (int i = 0; i < N; i++) ids[i] = f->next_id + i;
    if (N > 0) {
        HIP_TRY(f, hipMemcpyAsync(f->lm_id, ids.data(), sizeof(int64_t) * N, hipMemcpyHostToDevice, f->stream));
        HIP_TRY(f, hipMemcpyAsync(f->lm_born, born.data(), sizeof(double) * N, hipMemcpyHostToDevice, f->stream));
    }
    HIP_TRY(f, hipMemcpy2DAsync(f->P, sizeof(float) * f->ldp, sigma, sizeof(float) * ld, sizeof(float) * n, n,
                             hipMemcpyHostToDevice, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    f->N = N;
    f->n = n;
    f->next_id += N;
    return EKFVIO_OK;
}

int ekfvio_imu_update(ekfvio_filter* f, const float* gyro, const float* accel) {
    if (!f || !gyro || !accel) return EKFVIO_EINVAL;
    f->out_fresh = false;
    HIP_TRY(f, hipSetDevice(f->device));
    launch_imu_update(f, gyro, accel);
    HIP_TRY(f, hipGetLastError());
    return EKFVIO_OK;
}

int ekfvio_imu(ekfvio_filter* f, double stamp, const float* gyro, const float* accel) {
    if (!f) return EKFVIO_EINVAL;
    f->out_fresh = false;
    if (!f->cfg.use_imu) return EKFVIO_OK;  // the reference's callback only logs
    if (!gyro || !accel) return EKFVIO_EINVAL;
    if (!f->have_stamp) {  // tc_ekf.t is set by the first message (EKFVIO.cpp:148-150 does it for the first frame)
        f->t_stamp = stamp;
        f->have_stamp = true;
        return EKFVIO_OK;
    }
    const double dt = stamp - f->t_stamp;
    if (!(dt >= 0)) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    launch_predict(f, (float)dt);
    f->t_stamp = stamp;
    launch_imu_update(f, gyro, accel);
    HIP_TRY(f, hipGetLastError());
    return EKFVIO_OK;
}

// ---- uploaded measurement sequences ---------------------------------------------------
// the three buffers of a sequence (the previous upload's are released as each is acquired) and their contents, waited for
static int upload_sequence(ekfvio_filter* f, int32_t frames, const float* z, const float* R, const uint8_t* pass) {
    const size_t N = f->N;
    HIP_TRY(f, dev_alloc(f, &f->seq_z, frames * 2 * N));
    HIP_TRY(f, dev_alloc(f, &f->seq_R, frames * 4 * N));
    HIP_TRY(f, dev_alloc(f, &f->seq_pass, frames * N));
    HIP_TRY(f, hipMemcpyAsync(f->seq_z, z, sizeof(float) * frames * 2 * N, hipMemcpyHostToDevice, f->stream));
    HIP_TRY(f, hipMemcpyAsync(f->seq_R, R, sizeof(float) * frames * 4 * N, hipMemcpyHostToDevice, f->stream));
    HIP_TRY(f, hipMemcpyAsync(f->seq_pass, pass, frames * N, hipMemcpyHostToDevice, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    return EKFVIO_OK;
}
int ekfvio_upload_measurements(ekfvio_filter* f, int32_t frames, const float* z, const float* R, const uint8_t* pass) {
    if (!f || frames <= 0 || !z || !R || !pass || f->N <= 0) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    drop_graph(f);  // the captured launches hold pointers into the old sequence buffers
    // no sequence while this one is on its way: an upload that fails leaves a handle ekfvio_run_uploaded refuses, holding no sequence memory
    f->seq_frames = 0, f->seq_N = 0;
    f->seq_m.clear();
    const int rc = upload_sequence(f, frames, z, R, pass);
    if (rc != EKFVIO_OK) {
        f->mem.release(&f->seq_z), f->mem.release(&f->seq_R), f->mem.release(&f->seq_pass);
        return rc;
    }
    const size_t N = f->N;
    f->seq_frames = frames;
    f->seq_N = (int)N;
    f->seq_m.resize(frames);
    for (int i = 0; i < frames; i++) f->seq_m[i] = count_rows(pass + (size_t)i * N, (int)N);
    return EKFVIO_OK;
}

// An update of ekfvio_run_uploaded: frame i of the uploaded sequence, or the one the device-side counter names.  These launches and captures
// carry the long wait bound (plan.h, Tuning::sweep_wait_ticks): nothing can run their updates again
static UpdateInputs uploaded_update(ekfvio_filter* f, int m, int i, int* counter) {
    UpdateInputs in;
    in.m = m, in.z = f->seq_z + (size_t)i * 2 * f->N, in.R = f->seq_R + (size_t)i * 4 * f->N, in.pass = f->seq_pass + (size_t)i * f->N;
    in.frame_counter = counter, in.frames = counter ? f->seq_frames : 0;
    in.recoverable = false;
    return in;
}
// One filter step of the uploaded sequence, enqueued or captured: process(dt) and the update with m measurement rows of frame i, or of the frame
// the device-side counter names.  The three arguments behind it are a captured step's; an eager one leaves them alone.
//   book_rides     the frame's measurement bookkeeping rides in the process(dt) launch
//   prelinearized  the step in front of this one linearised for it (its StepDone::linearised_next)
//   next_dt        >= 0: this step's update may linearise for the step behind it (round 6; plan_update decides whether the shape allows it)
struct StepDone {
    bool pre;              // process(dt) went out pre-linearised
    bool linearised_next;  // the update's last GEMM linearised for the next process(dt)
};
static StepDone enqueue_uploaded_step(ekfvio_filter* f, float dt, int m, int i, int* counter, bool book_rides = false, bool prelinearized = false,
                                      float next_dt = -1.f) {
    BookArgs bk;
    if (book_rides) bk = make_book_args(f, m, f->seq_z, f->seq_R, f->seq_pass, counter);
    StepDone d;
    d.pre = launch_predict(f, dt, book_rides ? &bk : nullptr, prelinearized);
    UpdateInputs in = uploaded_update(f, m, i, counter);
    in.bookkeeping_done = book_rides;
    in.next_dt = next_dt;
    d.linearised_next = launch_update(f, in).linearised_next;
    return d;
}
// Captures `steps` filter steps (m measurement rows each, bookkeeping driven by the device-side frame counter) into entry e of the handle's
// cache.  `steps` is even: the mean / covariance ping-pong nets to zero (the captured launches do not execute).
static int capture_steps(ekfvio_filter* f, GraphCache::Entry* e, int steps, int m, float dt, int* counter) {
    // sweep_flags_clean mirrors DEVICE state on the host, and a capture records launches without running them: the
    // graph must not inherit the mirror's value of the moment it was captured at -- its first sweep always zeroes the flags itself (one
    // memset node per replay) -- and the mirror must come out of the capture as it went in.  What a replay leaves behind is recorded
    // with the cache (leaves_flags_clean) and applied after the replays.
    const bool mirror = f->sweep_flags_clean;
    f->sweep_flags_clean = false;
    // the bookkeeping rides in the process(dt) launch -- unless the handle gates its measurements: the gate reads the PROPAGATED state, so
    // gate + bookkeeping are a launch of their own between process(dt) and the update (launch_update)
    const bool gate = f->gate_chi2 > 0.f;
    e->steps = steps, e->pre = 0;
    const int rc = capture_graph(f, &e->exec, [&] {
        // inside a graph the next step's dt is known: every update but the graph's last lets its last GEMM linearise for the step behind it
        // (the graph's last update leaves the next replay's first step to linearise for itself, so a graph needs nothing from whatever ran
        // before it)
        StepDone d = {false, false};
        for (int k = 0; k < steps; k++) {
            d = enqueue_uploaded_step(f, dt, m, 0, counter, !gate, d.linearised_next, (k + 1 < steps) ? dt : -1.f);
            e->pre += d.pre ? 1 : 0;
        }
    });
    f->graphs.leaves_flags_clean = f->sweep_flags_clean;
    f->sweep_flags_clean = mirror;
    return rc;
}

// Executes a RunPlan (plan.h, plan_run): it does not decide
int ekfvio_run_uploaded(ekfvio_filter* f, int32_t first, int32_t count, float dt) {
    if (!f || f->seq_frames <= 0 || f->seq_N != f->N || count < 0 || first < 0 || !(dt >= 0.f)) return EKFVIO_EINVAL;
    f->out_fresh = false;
    HIP_TRY(f, hipSetDevice(f->device));
    // (no sweep_maybe_retry here -- ADVICE r05: a device-resident run cannot run an aborted update again, so a handle whose persistent
    // sweep once gave up keeps the per-step sweep for its graph replays until ekfvio_update / ekfvio_step_image, which CAN recover,
    // have tried the persistent launch again and it has come through; with a permanent obstacle (a compute-unit mask, a co-tenant
    // process) a retry from here would skip a replay's remaining updates every 2 .. 64 s for the handle's whole life)
    const RunPlan run = plan_run(f->seq_m.data(), f->seq_frames, f->N, f->gate_chi2 > 0.f, f->prof_on, count);
    if (!run.graphs) {
        for (int s = 0; s < run.eager; s++) {
            const int i = (first + s) % f->seq_frames;
            enqueue_uploaded_step(f, dt, f->seq_m[i], i, nullptr);
        }
        HIP_TRY(f, hipGetLastError());
        return EKFVIO_OK;
    }
    // the bookkeeping kernel reads the frame index from a device counter, set here
    // by value (a copy from a host scalar could be overtaken by the next call's write to that scalar)
    int* counter = f->info + 1;
    HIP_TRY(f, hipMemsetD32Async((hipDeviceptr_t)counter, first % f->seq_frames, 1, f->stream));
    GraphCache& c = f->graphs;
    GraphKey key;
    key.N = f->N, key.m = run.m, key.frames = f->seq_frames, key.dt = dt, key.mu = f->mu, key.P = f->P, key.seq = f->seq_z;
    key.sole = live_handles_on(f->device) <= 1;
    if (!(c.key == key)) {
        drop_graph(f);
        c.key = key;
    }
    // whatever is missing is captured now, the long graph together with the others (i.e. in a caller's warm-up call), never lazily inside a long run
    for (int g = 0; g < RUN_GRAPHS; g++)
        if (run_graph_used(g, f->seq_frames) && !c.g[g].exec) {
            const int rc = capture_steps(f, &c.g[g], run_graph_steps(g), run.m, dt, counter);
            if (rc != EKFVIO_OK) return rc;
        }
    // (a replay runs no host code: its steps and its pre-linearised ones are counted here, ekfvio_get_counters [6] and [7])
    bool replayed = false;
    for (int g = 0; g < RUN_GRAPHS; g++)
        for (int r = 0; r < run.replays[g]; r++) {
            HIP_TRY(f, hipGraphLaunch(c.g[g].exec, f->stream));
            f->graph_steps += c.g[g].steps, f->prelinearized_steps += c.g[g].pre;
            replayed = true;
        }
    if (replayed) f->sweep_flags_clean = c.leaves_flags_clean;  // what the last replayed step left in device memory
    for (int s = 0; s < run.eager; s++) enqueue_uploaded_step(f, dt, run.m, 0, counter);  // an odd last step, same counter-driven bookkeeping
    HIP_TRY(f, hipGetLastError());
    return EKFVIO_OK;
}

int ekfvio_synchronize(ekfvio_filter* f) {
    if (!f) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    // a non-positive pivot met by an asynchronous run (ekfvio_run_uploaded) surfaces here, once
    int bad = 0;
    const int rc = read_status(f, 0, nullptr, &bad, nullptr);
    if (rc != EKFVIO_OK) return rc;
    return settle_update(f, bad, nullptr, nullptr, false);
}

// ---- instrumentation ------------------------------------------------------------------
int ekfvio_profile_enable(ekfvio_filter* f, int32_t on) {
    if (!f) return EKFVIO_EINVAL;
    hipStreamSynchronize(f->stream);
    f->prof_on = on != 0;
    if (f->prof_on) {
        // calibrate the cost of an (ev0, ev1) pair with nothing in between
        double acc = 0;
        const int reps = 32;
        for (int i = 0; i < reps + 4; i++) {
            (void)hipEventRecord(f->ev0, f->stream);
            (void)hipEventRecord(f->ev1, f->stream);
            (void)hipEventSynchronize(f->ev1);
            float ms = 0;
            (void)hipEventElapsedTime(&ms, f->ev0, f->ev1);
            if (i >= 4) acc += ms;
        }
        f->prof_overhead_ms = (float)(acc / reps);
    }
    return EKFVIO_OK;
}
// Mean launch duration of the two P-update GEMMs at the shape of the most recent update, measured the way the
// timed region runs them: `reps` pairs captured into one hipGraph (back-to-back launches on the handle's stream),
// replayed once between two HIP events.  Outputs go to scratch; the filter state is unchanged.
int ekfvio_profile_update_gemms(ekfvio_filter* f, int32_t reps, double* avg_launch_us, double* flops_per_launch) {
    if (!f || reps <= 0 || !avg_launch_us) return EKFVIO_EINVAL;
    if (f->last_m <= 0 || f->N <= 0) return EKFVIO_ESTATE;
    HIP_TRY(f, hipSetDevice(f->device));
    hipGraphExec_t ge = nullptr;
    double last_flops = 0;
    int per_rep = 0;
    const int rc = capture_graph(f, &ge, [&] { per_rep = launch_update_gemms_scratch(f, plan_update(f, f->last_m), reps, &last_flops); });
    if (rc != EKFVIO_OK) return rc;
    HIP_TRY(f, hipGraphLaunch(ge, f->stream));  // warm-up
    HIP_TRY(f, hipEventRecord(f->ev0, f->stream));
    HIP_TRY(f, hipGraphLaunch(ge, f->stream));
    HIP_TRY(f, hipEventRecord(f->ev1, f->stream));
    HIP_TRY(f, hipEventSynchronize(f->ev1));
    float ms = 0;
    HIP_TRY(f, hipEventElapsedTime(&ms, f->ev0, f->ev1));
    (void)hipGraphExecDestroy(ge);
    // P2 is the predict's scratch and must stay zero outside the live block
    HIP_TRY(f, hipMemsetAsync(f->P2, 0, sizeof(float) * (size_t)f->ldp * f->ldp, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    *avg_launch_us = 1e3 * ms / ((double)per_rep * reps);
    // EXECUTED flops, averaged over the launches of one update: the second Joseph GEMM of the throughput regime forms the lower triangle's
    // 64 x 64 tiles only (GemmPlan::sym); the first is counted over n x n (its column n is the rider K y)
    if (flops_per_launch) *flops_per_launch = per_rep == 2 ? 0.5 * (2.0 * f->n * (double)f->n * round_up(f->last_m, 64) + last_flops) : last_flops;
    return EKFVIO_OK;
}
int ekfvio_profile_reset(ekfvio_filter* f) {
    if (!f) return EKFVIO_EINVAL;
    for (int i = 0; i < PC_COUNT; i++) f->prof[i] = ProfSlot();
    return EKFVIO_OK;
}
int ekfvio_profile_count(void) { return PC_COUNT; }
const char* ekfvio_profile_name(int32_t cls) { return (cls >= 0 && cls < PC_COUNT) ? kProfNames[cls] : ""; }
int ekfvio_profile_get(ekfvio_filter* f, int32_t cls, double* total_ms, int64_t* launches, double* flops) {
    if (!f || cls < 0 || cls >= PC_COUNT) return EKFVIO_EINVAL;
    if (total_ms) *total_ms = f->prof[cls].ms;
    if (launches) *launches = f->prof[cls].launches;
    if (flops) *flops = f->prof[cls].flops;
    return EKFVIO_OK;
}

// ---- innovation gate --------------------------------------------------------------------
int ekfvio_set_gate(ekfvio_filter* f, float chi2) {
    if (!f || !(chi2 >= 0.f)) return EKFVIO_EINVAL;  // (negative, NaN)
    if (chi2 > 0.f && !f->gate_words) {
        // the gate's device memory, ONE allocation made when a handle first asks for the gate (a handle that never does launches and
        // allocates nothing it did not before): [4] words, then d2, verdicts and effective flags per landmark
        HIP_TRY(f, hipSetDevice(f->device));
        const size_t maxf = (size_t)(f->cfg.max_features > 0 ? f->cfg.max_features : 1);
        unsigned char* buf = nullptr;
        HIP_TRY(f, dev_alloc(f, &buf, 4 * sizeof(int) + maxf * (sizeof(float) + 2)));
        f->gate_words = reinterpret_cast<int*>(buf);
        f->gate_d2 = reinterpret_cast<float*>(buf + 4 * sizeof(int));
        f->gate_flag = buf + 4 * sizeof(int) + maxf * sizeof(float);
        f->gate_pass = f->gate_flag + maxf;
    }
    f->gate_chi2 = chi2;
    drop_graph(f);  // gated steps are another launch sequence: gate + bookkeeping behind process(dt), not inside it
    return EKFVIO_OK;
}

int ekfvio_get_gate(ekfvio_filter* f, float* d2, uint8_t* gated, int32_t* n_landmarks, int32_t* gated_last, int64_t* gated_total) {
    if (!f) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    int w[4] = {0, 0, 0, 0};
    if (f->gate_words) {  // (null: the handle never gated)
        HIP_TRY(f, hipMemcpyAsync(w, f->gate_words, sizeof(w), hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(f, hipStreamSynchronize(f->stream));
    }
    const int seen = std::min(std::max(w[1], 0), f->cfg.max_features);
    if (seen > 0) {
        if (d2) HIP_TRY(f, hipMemcpyAsync(d2, f->gate_d2, sizeof(float) * seen, hipMemcpyDeviceToHost, f->stream));
        if (gated) HIP_TRY(f, hipMemcpyAsync(gated, f->gate_flag, seen, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(f, hipStreamSynchronize(f->stream));
    }
    if (n_landmarks) *n_landmarks = seen;
    if (gated_last) *gated_last = w[0];
    if (gated_total) memcpy(gated_total, w + 2, sizeof(int64_t));
    return EKFVIO_OK;
}

// ---- forward-backward check of the tracker (the kernel side: klt.hip) ----------------------
int ekfvio_set_klt_fb(ekfvio_filter* f, float max_px) {
    if (!f || !(max_px >= 0.f)) return EKFVIO_EINVAL;  // (negative, NaN)
    f->cfg.klt_fb_max_px = max_px;  // (read by the next track; the tracker is in no captured graph)
    return EKFVIO_OK;
}

int ekfvio_get_klt_fb(ekfvio_filter* f, float* err2, uint8_t* rejected, int32_t* n_landmarks, int32_t* rejected_last, int64_t* rejected_total) {
    if (!f) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    int w[4] = {0, 0, 0, 0};
    if (f->fb_words) {  // (null: no track of this handle ran the check)
        HIP_TRY(f, hipMemcpyAsync(w, f->fb_words, sizeof(w), hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(f, hipStreamSynchronize(f->stream));
    }
    const int seen = std::min(std::max(w[1], 0), f->cfg.max_features);
    if (seen > 0) {
        if (err2) HIP_TRY(f, hipMemcpyAsync(err2, f->fb_err2, sizeof(float) * seen, hipMemcpyDeviceToHost, f->stream));
        if (rejected) HIP_TRY(f, hipMemcpyAsync(rejected, f->fb_flag, seen, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(f, hipStreamSynchronize(f->stream));
    }
    if (n_landmarks) *n_landmarks = seen;
    if (rejected_last) *rejected_last = w[0];
    if (rejected_total) memcpy(rejected_total, w + 2, sizeof(int64_t));
    return EKFVIO_OK;
}

int ekfvio_get_counters(ekfvio_filter* f, int64_t counters[8]) {
    if (!f || !counters) return EKFVIO_EINVAL;
    counters[0] = f->persistent_sweeps;
    counters[1] = f->schur_sweeps;
    counters[2] = f->sweep_recoveries;
    counters[3] = (f->tune.persist_sweep && !f->sweep_latched_off) ? 2 : 0;
    counters[4] = f->early_output_frames;
    counters[5] = f->t2_updates;
    counters[6] = f->graph_steps;
    counters[7] = f->prelinearized_steps;
    return EKFVIO_OK;
}

#ifdef EKFVIO_TEST_HOOKS  // include/ekfvio_test_hooks.h: only in libekfvio_hip_hooks.so
// ---- raw kernels for unit tests -------------------------------------------------------
int ekfvio_test_gemm(ekfvio_filter* f, int32_t transB, int32_t M, int32_t N, int32_t K, float alpha, const float* A,
                     int32_t lda, const float* B, int32_t ldb, float beta, float* C, int32_t ldc, int32_t variant) {
    if (!f || M <= 0 || N <= 0 || K <= 0 || !A || !B || !C) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    // device copies padded to the kernels' contract (64-row/col slack, K to 64, zero fill);
    // packed on the host so that only flat copies are issued
    const int Mp = round_up(M, 64), Np = round_up(N, 64), Kp = round_up(K, 64);
    const int brows = transB ? Np : Kp, bcols = transB ? Kp : Np;
    std::vector<float> hA((size_t)Mp * Kp, 0.f), hB((size_t)brows * bcols, 0.f), hC((size_t)Mp * Np, 0.f);
    for (int k = 0; k < K; k++)
        for (int i = 0; i < M; i++) hA[(size_t)k * Mp + i] = A[(size_t)k * lda + i];
    for (int c = 0; c < (transB ? K : N); c++)
        for (int r = 0; r < (transB ? N : K); r++) hB[(size_t)c * brows + r] = B[(size_t)c * ldb + r];
    for (int j = 0; j < N; j++)
        for (int i = 0; i < M; i++) hC[(size_t)j * Mp + i] = C[(size_t)j * ldc + i];
    MemLedger tmp(hip_mem_backend());  // the call's own device memory: released on every return
    float *dA = nullptr, *dB = nullptr, *dC = nullptr;
    HIP_TRY(f, dev_alloc(tmp, f->stream, &dA, hA.size()));
    HIP_TRY(f, dev_alloc(tmp, f->stream, &dB, hB.size()));
    HIP_TRY(f, dev_alloc(tmp, f->stream, &dC, hC.size()));
    HIP_TRY(f, hipMemcpyAsync(dA, hA.data(), sizeof(float) * hA.size(), hipMemcpyHostToDevice, f->stream));
    HIP_TRY(f, hipMemcpyAsync(dB, hB.data(), sizeof(float) * hB.size(), hipMemcpyHostToDevice, f->stream));
    HIP_TRY(f, hipMemcpyAsync(dC, hC.data(), sizeof(float) * hC.size(), hipMemcpyHostToDevice, f->stream));
    GemmCall g;
    g.M = M, g.N = N, g.K = Kp, g.transB = transB != 0, g.alpha = alpha, g.A = dA, g.lda = Mp, g.B = dB, g.ldb = brows;
    g.beta = beta, g.Cin = dC, g.ldcin = Mp, g.C = dC, g.ldc = Mp, g.variant = variant;
    launch_gemm(f, g);
    HIP_TRY(f, hipMemcpyAsync(hC.data(), dC, sizeof(float) * hC.size(), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    for (int j = 0; j < N; j++)
        for (int i = 0; i < M; i++) C[(size_t)j * ldc + i] = hC[(size_t)j * Mp + i];
    return EKFVIO_OK;
}

// Times `reps` back-to-back launches of the GEMM at one shape (operands resident, random
// fill); returns the mean launch-to-launch time in microseconds.  variant selects a tile
// configuration (0 = production).
int ekfvio_test_gemm_bench(ekfvio_filter* f, int32_t transB, int32_t lowerB, int32_t M, int32_t N, int32_t K,
                           int32_t reps, int32_t variant, double* mean_us) {
    if (!f || M <= 0 || N <= 0 || K <= 0 || reps <= 0 || !mean_us) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    const int Mp = round_up(M, 128), Np = round_up(N, 128), Kp = round_up(K, 64);
    const int brows = transB ? Np : Kp, bcols = transB ? Kp : Np;
    std::vector<float> hA((size_t)Mp * Kp), hB((size_t)brows * bcols), hC((size_t)Mp * Np);
    uint32_t st = 12345u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) & 0xffff) / 32768.0f - 1.0f; };
    for (auto& v : hA) v = rnd();
    for (auto& v : hB) v = rnd();
    for (auto& v : hC) v = rnd();
    MemLedger tmp(hip_mem_backend());  // the call's own device memory: released on every return
    float *dA = nullptr, *dB = nullptr, *dC = nullptr;
    HIP_TRY(f, dev_alloc(tmp, f->stream, &dA, hA.size()));
    HIP_TRY(f, dev_alloc(tmp, f->stream, &dB, hB.size()));
    HIP_TRY(f, dev_alloc(tmp, f->stream, &dC, hC.size()));
    HIP_TRY(f, hipMemcpyAsync(dA, hA.data(), sizeof(float) * hA.size(), hipMemcpyHostToDevice, f->stream));
    HIP_TRY(f, hipMemcpyAsync(dB, hB.data(), sizeof(float) * hB.size(), hipMemcpyHostToDevice, f->stream));
    HIP_TRY(f, hipMemcpyAsync(dC, hC.data(), sizeof(float) * hC.size(), hipMemcpyHostToDevice, f->stream));
    const bool stamped = variant >= 10000;  // library built with -DEKF_GEMM_STAMPS
    GemmCall g;
    g.M = M, g.N = N, g.K = Kp, g.transB = transB != 0, g.lowerB = lowerB != 0, g.alpha = -1e-3f, g.A = dA, g.lda = Mp, g.B = dB, g.ldb = brows;
    g.beta = 1.f, g.Cin = dC, g.ldcin = Mp, g.C = dC, g.ldc = Mp, g.variant = variant % 10000;
    for (int w = 0; w < 3; w++)
        launch_gemm(f, g);
    HIP_TRY(f, hipEventRecord(f->ev0, f->stream));
    for (int r = 0; r < reps; r++)
        launch_gemm(f, g);
    HIP_TRY(f, hipEventRecord(f->ev1, f->stream));
    HIP_TRY(f, hipEventSynchronize(f->ev1));
    float ms = 0;
    HIP_TRY(f, hipEventElapsedTime(&ms, f->ev0, f->ev1));
    *mean_us = 1e3 * ms / reps;
    if (stamped) {  // diagnostic: one stamped launch, stamps returned through mean_us[1..40]
        long long* dst = nullptr;
        HIP_TRY(f, dev_alloc(tmp, f->stream, &dst, 40));
        f->gemm_stamps = dst;  // (no return between set and reset: the handle's next GEMM launch must not find a temporary here)
        launch_gemm(f, g);
        f->gemm_stamps = nullptr;
        long long hst[40];
        HIP_TRY(f, hipMemcpyAsync(hst, dst, sizeof(hst), hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(f, hipStreamSynchronize(f->stream));
        for (int i = 0; i < 40; i++) mean_us[1 + i] = (double)hst[i];
    }
    return EKFVIO_OK;
}

// Diagnostic: cycle stamps (s_memtime) of the phases of one 64x64 diagonal-block factorisation
// on an SPD test block; stamps[0..11]: start, loaded, then after each panel factor / trailing
// update (x4), inverse done, stored; stamps[16 + 16*wave + i]: per-wavefront end of work of
// phase i (2p: factor phase of panel p, 2p+1: column-update phase, 8: final phase).
int ekfvio_test_potrf_stamps(ekfvio_filter* f, int64_t stamps[80]) {
    if (!f || !stamps) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    std::vector<float> hs(64 * 64);
    for (int c = 0; c < 64; c++)
        for (int r = 0; r < 64; r++) hs[c * 64 + r] = (r == c ? 2.0f : 0.f) + 0.3f / (1.0f + (r > c ? r - c : c - r));
    MemLedger tmp(hip_mem_backend());
    float *dS = nullptr, *dL = nullptr, *dLi = nullptr;
    long long* dst = nullptr;
    HIP_TRY(f, dev_alloc(tmp, f->stream, &dS, hs.size()));
    HIP_TRY(f, dev_alloc(tmp, f->stream, &dL, hs.size()));
    HIP_TRY(f, dev_alloc(tmp, f->stream, &dLi, 4096));
    HIP_TRY(f, dev_alloc(tmp, f->stream, &dst, 80));
    HIP_TRY(f, hipMemsetAsync(dst, 0, sizeof(long long) * 80, f->stream));
    HIP_TRY(f, hipMemcpyAsync(dS, hs.data(), sizeof(float) * hs.size(), hipMemcpyHostToDevice, f->stream));
    for (int rep = 0; rep < 3; rep++) launch_potrf_stamps(f, dS, 64, dL, dLi, dst);
    HIP_TRY(f, hipMemcpyAsync(stamps, dst, sizeof(long long) * 80, hipMemcpyDeviceToHost, f->stream));
    std::vector<uint32_t> hl(64 * 64), hi(4096);
    HIP_TRY(f, hipMemcpyAsync(hl.data(), dL, sizeof(float) * hl.size(), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipMemcpyAsync(hi.data(), dLi, sizeof(float) * hi.size(), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    // stamps[12], [13]: FNV-1a hashes of the bits of L and of the 16x16 inverses (variants must agree bit for bit)
    uint64_t h1 = 1469598103934665603ull, h2 = h1;
    for (uint32_t v : hl) h1 = (h1 ^ v) * 1099511628211ull;
    for (uint32_t v : hi) h2 = (h2 ^ v) * 1099511628211ull;
    stamps[12] = (int64_t)h1;
    stamps[13] = (int64_t)h2;
    return EKFVIO_OK;
}

// Diagnostic: stamps[512] of the persistent sweep's last run (chain: [0],[1], then 8 per block step
// from [8]; first helper: 8 per block step from [256]).  enable != 0 allocates and arms the buffer.
int ekfvio_test_sweep_stamps(ekfvio_filter* f, int enable, int64_t* stamps /* [1024] */) {
    if (!f) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    if (enable && !f->sweep_dbg) {
        HIP_TRY(f, dev_alloc(f, &f->sweep_dbg, 1024));
        HIP_TRY(f, hipMemsetAsync(f->sweep_dbg, 0, 1024 * sizeof(long long), f->stream));
    }
    if (stamps && f->sweep_dbg) {
        HIP_TRY(f, hipMemcpyAsync(stamps, f->sweep_dbg, 1024 * sizeof(long long), hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(f, hipStreamSynchronize(f->stream));
    }
    return EKFVIO_OK;
}

int ekfvio_test_sweep_fault(ekfvio_filter* f, int32_t spin_limit, int32_t stall_workgroup) {
    if (!f || spin_limit < 0) return EKFVIO_EINVAL;
    f->sweep_spin_limit = spin_limit;
    f->sweep_stall_wg = stall_workgroup;
    drop_graph(f);  // captured launches carry the old arguments
    return EKFVIO_OK;
}

int ekfvio_test_sweep_delay(ekfvio_filter* f, int32_t workgroup, int32_t point, int32_t ticks) {
    // at most 1 ms, a third of the DEFAULT wait bound (Tuning::sweep_wait_ticks, 3 ms): under that bound a delay cannot turn into an abort.  A handle
    // created with EKFVIO_SWEEP_WAIT_MS below 1 has a shorter bound and can abort on a long delay: the tests clear that variable
    if (!f || (point != 0 && point != 1) || ticks < 0 || ticks > EKFVIO_TEST_SWEEP_DELAY_MAX_TICKS) return EKFVIO_EINVAL;
    f->sweep_delay_wg = workgroup >= 0 ? workgroup : -1;
    f->sweep_delay_point = point;
    f->sweep_delay_ticks = ticks;
    drop_graph(f);  // captured launches carry the old arguments
    return EKFVIO_OK;
}

int ekfvio_test_cholesky_solve(ekfvio_filter* f, int32_t m, int32_t nrhs, const float* S, const float* Crhs,
                               float* L_out, float* X_out, int32_t* info) {
    // S: m x m (ld m) SPD; Crhs: nrhs x m (ld nrhs); L_out m x m; X_out = Crhs * S^-1 (nrhs x m).
    // Runs the production path: augmented sweep + gain GEMMs.
    if (!f || m <= 0 || nrhs <= 0 || !S || !Crhs) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    const int mp = round_up(m, 64), rp = round_up(nrhs, 64);
    const int ld = mp + rp + mp;
    std::vector<float> hs((size_t)ld * mp, 0.f);
    for (int c = 0; c < mp; c++) {
        for (int r = 0; r < mp; r++) hs[(size_t)c * ld + r] = (r < m && c < m) ? S[(size_t)c * m + r] : (r == c ? 1.f : 0.f);
        if (c < m)
            for (int r = 0; r < nrhs; r++) hs[(size_t)c * ld + mp + r] = Crhs[(size_t)c * nrhs + r];
        hs[(size_t)c * ld + mp + rp + c] = 1.f;
    }
    MemLedger tmp(hip_mem_backend());
    float *dS = nullptr, *dL = nullptr, *dLi = nullptr, *dK = nullptr, *dW = nullptr;
    HIP_TRY(f, dev_alloc(tmp, f->stream, &dS, hs.size()));
    HIP_TRY(f, dev_alloc(tmp, f->stream, &dL, hs.size()));
    HIP_TRY(f, dev_alloc(tmp, f->stream, &dLi, (size_t)64 * mp));
    HIP_TRY(f, dev_alloc(tmp, f->stream, &dK, (size_t)rp * mp));
    HIP_TRY(f, dev_alloc(tmp, f->stream, &dW, (size_t)rp * mp));
    HIP_TRY(f, hipMemcpyAsync(dS, hs.data(), sizeof(float) * hs.size(), hipMemcpyHostToDevice, f->stream));
    // the flow the handle's knobs and the process's handle count select for this shape, as for an update of the filter (plan_raw_sweep)
    UpdatePlan plan = plan_raw_sweep(f->tune, plan_shape(f), mp, rp);
    launch_chol_sweep(f, plan, dS, dL, dLi, ld, plan.persistent() && !f->sweep_flags_clean);
    if (plan.persistent()) f->sweep_flags_clean = false;  // (no GEMM of an update behind this sweep zeroes its flags)
    // one step of residual refinement against L, unless a block went through the U S U^T path (K L = Y S then, not Y)
    std::vector<unsigned long long> hsign(mp / 64);
    HIP_TRY(f, hipMemcpyAsync(hsign.data(), f->Lsign, sizeof(unsigned long long) * hsign.size(), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    int refine = 1;
    for (unsigned long long v : hsign) refine &= (v == 0ull);
    if (refine) plan.gain = GAIN_GEMM;
    launch_gain_from_sweep(f, plan, dL, ld, nrhs, dK, dW, rp, refine);
    std::vector<float> hl(hs.size()), hk((size_t)rp * mp);
    HIP_TRY(f, hipMemcpyAsync(hl.data(), dL, sizeof(float) * hl.size(), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipMemcpyAsync(hk.data(), dK, sizeof(float) * hk.size(), hipMemcpyDeviceToHost, f->stream));
    if (info) {
        HIP_TRY(f, hipMemcpyAsync(info, f->info, sizeof(int), hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(f, hipMemsetAsync(f->info, 0, sizeof(int), f->stream));
    }
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    if (const char* dp = getenv("EKFVIO_DEBUG_DUMP_LAUG")) {  // diagnostic: the whole swept matrix [L; Y; L^-T]
        if (FILE* fp = fopen(dp, "wb")) {
            const int hdr[3] = {ld, mp, rp};
            fwrite(hdr, sizeof(int), 3, fp);
            fwrite(hl.data(), sizeof(float), hl.size(), fp);
            fclose(fp);
        }
    }
    if (L_out)
        for (int c = 0; c < m; c++)
            for (int r = 0; r < m; r++) L_out[(size_t)c * m + r] = (r >= c) ? hl[(size_t)c * ld + r] : 0.f;
    if (X_out)
        for (int c = 0; c < m; c++)
            for (int r = 0; r < nrhs; r++) X_out[(size_t)c * nrhs + r] = hk[(size_t)c * rp + r];
    return EKFVIO_OK;
}

// What a ledger holds (mem.h): the handle's, or with a null handle everything this copy of the library holds, the test hooks' scratch included
int ekfvio_test_mem(ekfvio_filter* f, int64_t out[8]) {
    if (!out) return EKFVIO_EINVAL;
    MemCounts c[2];  // device; pinned, whatever its flags
    for (int k = 0; k < MEM_KINDS; k++) {
        MemCounts& d = c[k == MEM_DEVICE ? 0 : 1];
        const MemTotal& t = g_mem_total[k];
        const MemCounts s = f ? f->mem.counts((MemKind)k) : MemCounts{t.live.load(), t.live_bytes.load(), t.acquired.load(), t.released.load()};
        d.live += s.live, d.live_bytes += s.live_bytes, d.acquired += s.acquired, d.released += s.released;
    }
    const int64_t res[8] = {c[0].live, c[0].live_bytes, c[1].live, c[1].live_bytes, c[0].acquired, c[0].released, c[1].acquired, c[1].released};
    std::copy(res, res + 8, out);
    return EKFVIO_OK;
}
int ekfvio_test_mem_fail(ekfvio_filter* f, int32_t nth) {
    if (nth < 0) return EKFVIO_EINVAL;
    if (f)
        f->mem.fail_nth(nth);
    else
        g_next_create_fail.store(nth);
    return EKFVIO_OK;
}

// No handle, no HIP call: plan_update (plan.h) over the environment's Tuning and the PlanShape of a capacity on a device of `num_cus` compute units
int ekfvio_test_plan(int32_t num_cus, int32_t max_features, int32_t N, int32_t m, int32_t m_on_device, int32_t sole_handle,
                     int32_t latched_off, int32_t dense_predict, float next_dt, int32_t plan[12]) {
    if (!plan || max_features < 0 || N < 0 || N > max_features) return EKFVIO_EINVAL;
    const FilterDims d = filter_dims(max_features);
    PlanShape s;
    s.num_cus = num_cus, s.ldp = d.ldp, s.sweep_sync_words = d.sweep_sync_words, s.N = N, s.n = EKF_BASE + 3 * N;
    s.dense_predict = dense_predict != 0, s.sole_handle = sole_handle != 0, s.latched_off = latched_off != 0;
    const UpdatePlan p = plan_update(tuning_from_env(), s, m, m_on_device != 0, next_dt);
    const int32_t out[12] = {p.m, p.m_pad, p.n_pad, p.sweep, p.fused_gather, p.with_wt, p.gain, p.tail, p.t2_skip, p.t2_by_sweep, p.compact, p.lin_blocks};
    std::copy(out, out + 12, plan);
    return EKFVIO_OK;
}

// ... plan_gemm for one shape; behind the GemmPlan's words: gemm_throughput_regime, gemm_tile_height
int ekfvio_test_gemm_plan(int32_t num_cus, int32_t M, int32_t N, int32_t K, int32_t transB, int32_t lowerB, int32_t epi, int32_t mean,
                          int32_t lin_blocks, int32_t sym, int32_t variant, int32_t plan[18]) {
    if (!plan || M <= 0 || N <= 0 || K <= 0 || epi < EPI_NONE || epi > EPI_MEAN_PARTIAL) return EKFVIO_EINVAL;
    GemmShape s;
    s.M = M, s.N = N, s.K = K, s.transB = transB != 0, s.lowerB = lowerB != 0, s.epi = epi, s.mean = mean != 0;
    s.lin_blocks = lin_blocks, s.sym = sym != 0, s.variant = variant;
    const GemmPlan p = plan_gemm(tuning_from_env(), num_cus, s);
    const int32_t out[18] = {p.k16, p.bm, p.wps, p.groups, p.threads(), p.tiles_x, p.tiles_y, p.tiles, p.grid_x, p.grid_y, p.mean_wg, p.lin_blocks,
                             p.mean_keep, p.sym, p.sym_w, p.order2d, gemm_throughput_regime(num_cus, M, N, K), gemm_tile_height(num_cus, M, N, K, s.transB)};
    std::copy(out, out + 18, plan);
    return EKFVIO_OK;
}
// ... and plan_predict for a handle holding N landmarks
int ekfvio_test_predict_plan(int32_t num_cus, int32_t N, int32_t dense_predict, int32_t prelinearized, int32_t bookkeeping, int32_t plan[8]) {
    if (!plan || N < 0) return EKFVIO_EINVAL;
    PlanShape s;
    s.num_cus = num_cus, s.N = N, s.n = EKF_BASE + 3 * N, s.dense_predict = dense_predict != 0;
    const PredictPlan p = plan_predict(tuning_from_env(), s, prelinearized != 0);
    const int32_t out[8] = {p.dense, p.pre, p.lin_inside, p.lin_in_front, p.ts, p.chunks, p.book_rides(), p.grid(bookkeeping != 0)};
    std::copy(out, out + 8, plan);
    return EKFVIO_OK;
}
// ... and plan_run for ekfvio_run_uploaded(first, count, dt) over `frames` uploaded frames of rows[i] measurement rows
int ekfvio_test_run_plan(int32_t N, int32_t gated, int32_t profiling, int32_t frames, const int32_t* rows, int32_t count, int32_t out[6]) {
    if (!out || !rows || N < 0 || frames <= 0 || count < 0) return EKFVIO_EINVAL;
    const RunPlan p = plan_run(rows, frames, N, gated != 0, profiling != 0, count);
    const int32_t res[6] = {p.graphs, p.m, p.replays[0], p.replays[1], p.replays[2], p.eager};
    std::copy(res, res + 6, out);
    return EKFVIO_OK;
}

// No handle, no HIP call: the grid and the flag layout (plan.h, PersistGrid / PersistFlags) of the persistent launch that plan selects
int ekfvio_test_persist_grid(int32_t num_cus, int32_t max_features, int32_t N, int32_t m, int32_t m_on_device, int32_t sole_handle,
                             int32_t latched_off, int32_t dense_predict, float next_dt, int32_t* roles, int32_t max_blocks, int32_t out[10]) {
    if (!out || max_features < 0 || N < 0 || N > max_features) return EKFVIO_EINVAL;
    const FilterDims d = filter_dims(max_features);
    PlanShape s;
    s.num_cus = num_cus, s.ldp = d.ldp, s.sweep_sync_words = d.sweep_sync_words, s.N = N, s.n = EKF_BASE + 3 * N;
    s.dense_predict = dense_predict != 0, s.sole_handle = sole_handle != 0, s.latched_off = latched_off != 0;
    const UpdatePlan p = plan_update(tuning_from_env(), s, m, m_on_device != 0, next_dt);
    std::fill(out, out + 10, 0);
    if (!p.persistent()) return EKFVIO_OK;
    const PersistGrid g = persist_grid(p, d.ldp);
    const PersistFlags fl(p.m_pad, p.n_pad);
    const int32_t res[10] = {g.total(), g.kind, g.owners(), fl.ready(), fl.fin(), fl.pan(), fl.abort_word(), (int32_t)fl.words(), fl.zero_words(),
                             (int32_t)d.sweep_sync_words};
    std::copy(res, res + 10, out);
    if (!roles) return EKFVIO_OK;
    if (max_blocks < g.total()) return EKFVIO_ECAPACITY;
    for (int b = 0; b < g.total(); b++) {
        const PersistRole r = g.role(b);
        roles[4 * b] = r.kind, roles[4 * b + 1] = r.a, roles[4 * b + 2] = r.b;
        roles[4 * b + 3] = r.kind == ROLE_OWNER ? g.owner_block(r.n) : -1;
    }
    return EKFVIO_OK;
}
// ... and tile pair p of T2 (plan.h, t2_pair)
int ekfvio_test_t2_pair(int32_t p, int32_t pair[2]) {
    if (p < 0 || !pair) return EKFVIO_EINVAL;
    int ta, tb;
    t2_pair(p, ta, tb);
    pair[0] = ta, pair[1] = tb;
    return EKFVIO_OK;
}

// `word` into every 32-bit element of the float buffers process(dt) and the update use as scratch, on the handle's stream: what a long-lived
// handle finds there is then no longer the zero fill of dev_alloc.  The state (P, P2, mu and the landmark bookkeeping), the measurement inputs,
// the sweep's flags and every integer buffer (idx, inv_idx, Lsign, info) are left alone: a garbage index would send a load out of its
// allocation.  None of the regions filled is written once at create and only read later ("Who owns the update's work buffers"), so
// nothing is put back here.
int ekfvio_test_fill_update_scratch(ekfvio_filter* f, uint32_t word) {
    if (!f) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    const size_t maxf = (size_t)(f->cfg.max_features > 0 ? f->cfg.max_features : 0);
    const size_t aug = (size_t)f->ld_aug * f->m_cap, pm = (size_t)f->ldp * f->m_cap;
    const struct { float* p; size_t count; } regions[] = {
        {f->Saug, aug}, {f->Laug, aug}, {f->Linv, 64 * (size_t)f->m_cap}, {f->Km, pm}, {f->Wt, pm}, {f->Gm, pm},
        {f->yres, (size_t)f->m_cap}, {f->Rm, 2 * (size_t)f->m_cap}, {f->Fdense, (size_t)f->ldp * f->ldp},
        {f->FA, (size_t)EKF_BASE * EKF_BASE}, {f->FB, 27 * maxf}, {f->FD, 9 * maxf}, {f->mu_next, (size_t)f->ldp},
    };
    for (const auto& r : regions)
        if (r.p && r.count) HIP_TRY(f, hipMemsetD32Async((hipDeviceptr_t)r.p, (int)word, r.count, f->stream));
    return EKFVIO_OK;
}
#endif  // EKFVIO_TEST_HOOKS

}  // extern "C"
