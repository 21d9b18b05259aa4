// ekf_vio_amd/csrc/common.h — internal declarations shared by the HIP translation units.
// gfx950 (MI355X / CDNA4) only: 64-wide wavefronts, fp32 MFMA, 160 KiB LDS per CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <string>
#include <vector>

#include "../../include/ekfvio.h"
#include "mem.h"   // HIP-free: MemLedger, what owns a handle's device and pinned memory
#include "plan.h"  // HIP-free: the switches (Tuning), the sizes a capacity implies, the flow of an update (UpdatePlan, plan_update)
#ifdef EKFVIO_TEST_HOOKS
#include "../../include/ekfvio_test_hooks.h"
#endif

// prune(SPARSE_THRESH, SPARSE_EPS) keeps |x| > 1e-8f*1e-5f (TightlyCoupledEKF.h:13-14, .cpp:117,580,591,625)
#ifndef EKF_POTRF_FV
#define EKF_POTRF_FV 12       // factor-phase variant of potrf64_lds (chol.hip): 12 = generated stream incl. its LDS traffic, LDS latency off the
                              // pivot chain (gen_ls3); 13 = the same with wider fill slots; 10 = round 1's stream; 8 = without the LDS traffic; 0 = plain
#endif
#define EKF_FLUSH_THRESH (1e-8f * 1e-5f)

// A HIP call inside a function that returns an ekfvio status: on failure the call's text and the runtime's message go to the handle's
// last_error and the function returns EKFVIO_EDEVICE.
#define HIP_TRY(f, expr)                                                           \
    do {                                                                           \
        hipError_t e__ = (expr);                                                   \
        if (e__ != hipSuccess) {                                                   \
            (f)->last_error = std::string(#expr) + ": " + hipGetErrorString(e__);  \
            return EKFVIO_EDEVICE;                                                 \
        }                                                                          \
    } while (0)

// The words of ekfvio_filter::h_info (pinned, device-mapped; d_hinfo on the device): what a kernel publishes and poll_status reads.
enum HostWord {
    HW_STATUS = 0,   // info[0]: bit 0 a non-positive pivot was met, bit 1 the persistent sweep gave up
    HW_SEQ = 1,      // the sequence number of the launch that published (next_status_seq), stored last with release at system scope
    HW_EXTRA = 2,    // one more device word for the caller (landmarks added, or added - removed; 0 where not asked)
    HW_REMOVED = 3,  // landmarks the frame's removal kernel took out (remove.hip; written in front of the publishing launch)
};
// One thread, behind the launch's own writes and its __threadfence_system(): the host reads the other words once it sees `seq`.
__device__ __forceinline__ void publish_host_words(int* host_word, const int* __restrict__ info, int extra, int seq) {
    host_word[HW_STATUS] = info[0];
    host_word[HW_EXTRA] = extra;
    __hip_atomic_store(host_word + HW_SEQ, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Kernel classes for the built-in event profiler (ekfvio_profile_*).
enum ProfClass {
    PC_LINEARIZE = 0,
    PC_PREDICT,
    PC_GEMM_PREDICT,
    PC_GATHER,
    PC_CHOL,
    PC_SOLVE,
    PC_GEMM_UPDATE,
    PC_UPDATE_MISC,
    PC_KLT_PYRAMID,
    PC_KLT_TRACK,
    PC_COUNT
};

struct ProfSlot {
    double ms = 0;
    int64_t launches = 0;
    double flops = 0;
};

struct KltFrame {
    // Pyramid level l: 8-bit image with a border of `border` pixels on every side
    // (reflect-101), and interleaved int16 (dx,dy) Scharr derivatives with a zero border.
    uint8_t* img[8] = {nullptr};
    short* deriv[8] = {nullptr};
    int w[8] = {0}, h[8] = {0};
    int levels = 0;  // number of valid levels (maxLevel+1)
    float K[9] = {0};
    bool valid = false;
    int cap_w = 0, cap_h = 0;  // level-0 size the planes were allocated for (they grow with the first larger frame)
};

// What the rectification map of a handle was formed for (rectify.hip): compared as bits
struct RectifyKey {
    float K[4];   // fx, cx, fy, cy of the K passed with the frame
    double D[8];  // the model's coefficients in the caller's order
    float P[4];   // fx', cx', fy', cy' where has_P, else zeros
    int model, has_P;
    int w, h;
};

// What the blocked map of a handle was formed for (mask.hip): compared as bits
struct MaskKey {
    RectifyKey rect;    // the rectification key where the border term is live (flag set and distortion on), else zeros
    int rect_live;
    unsigned user_gen;  // generation of the caller's mask (0: none)
    int s, pad, w, h, flags;
};

// The captured step graphs of a device-resident run (api.hip, ekfvio_run_uploaded executes a RunPlan of plan.h with them).  A graph holds an
// even number of filter steps: the mean / covariance ping-pong is back in its starting orientation behind a replay.
// GraphKey: the VALUES the captured launches depend on; a run whose key differs drops all graphs and captures again.  Events that change a
// captured launch -- the gate, the latch and its retry, a test hook's arguments, a new upload, a removal -- call drop_graph instead.
struct GraphKey {
    int N = -1, m = -1, frames = -1;  // landmarks, launch geometry (RunPlan::m), frames of the uploaded sequence
    bool sole = true;                 // captured while this was the device's only handle (decides which sweep the captured steps contain)
    float dt = -1.f;                  // compared exactly
    const float *mu = nullptr, *P = nullptr;  // orientation of the mean / covariance ping-pong at capture time
    const void* seq = nullptr;        // the uploaded sequence (seq_z)
    bool operator==(const GraphKey& o) const {
        return N == o.N && m == o.m && frames == o.frames && sole == o.sole && dt == o.dt && mu == o.mu && P == o.P && seq == o.seq;
    }
};
struct GraphCache {
    struct Entry {
        hipGraphExec_t exec = nullptr;
        int steps = 0;  // filter steps per replay (plan.h, run_graph_steps)
        int pre = 0;    // ... of which this many process(dt) launches were captured pre-linearised: a replay runs no host code (prelinearized_steps)
    };
    GraphKey key;
    Entry g[RUN_GRAPHS];  // longest first, as RunPlan::replays
    bool leaves_flags_clean = false;  // ekfvio_filter::sweep_flags_clean as a replay leaves it (the same for every entry: the last update's last GEMM decides)
};

const MemBackend& hip_mem_backend();  // api.hip: the runtime's device and pinned allocation, the only place that calls it

struct ekfvio_filter {
    ekfvio_config cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string last_error;
    MemLedger mem{hip_mem_backend()};  // owns every device and pinned buffer below, the lazily allocated ones included: ekfvio_destroy releases the ledger, no list of fields

    int N = 0;      // landmarks
    int n = EKF_BASE;
    int n_cap = 0, ldp = 0, m_cap = 0;  // filter_dims(cfg.max_features), plan.h (as ld_aug and sweep_sync_words below)
    Tuning tune;    // the run-time switches: written once, in ekfvio_create (plan.h, tuning_from_env)

    // --- state (device) ---
    float* mu = nullptr;       // [ldp]  base (22) then [u,v,1/d] per landmark
    float* mu_next = nullptr;  // [ldp]  scratch for the propagated mean
    float* last_klt = nullptr; // [2*max_features]
    uint8_t* del_flag = nullptr;  // [max_features]
    // Identity per landmark (include/ekfvio.h, "landmark identities"): row i of both names the landmark in row i of the state.
    // INVARIANT: exactly two kernels write them -- add_features_kernel (api.hip) appends, remove_features_kernel (remove.hip) compacts them with
    // last_klt and del_flag, in the kept order -- and ekfvio_set_state replaces them.  Nothing else moves landmarks: process(dt), the update
    // and ekfvio_run_uploaded leave both arrays alone.  Compaction keeps the order and new landmarks are appended with rising ids, so lm_id
    // is STRICTLY INCREASING in landmark order at all times.
    int64_t* lm_id = nullptr;     // [max_features] next_id + k for the k-th landmark of an append
    double* lm_born = nullptr;    // [max_features] the stamp of the frame the landmark entered in (born_stamp below)
    int64_t next_id = 0;          // ids handed out so far: advances where N does, never goes back, survives ekfvio_reset
    float* P = nullptr;        // [ldp*ldp] dense covariance, column-major
    float* P2 = nullptr;       // [ldp*ldp] ping-pong / scratch (X = F P, dense F)
    // --- process Jacobian blocks ---
    float* FA = nullptr;       // [22*22] column-major
    float* FB = nullptr;       // [max_features*27]  per landmark [9 cols (state 7..15)][3 rows]
    float* FD = nullptr;       // [max_features*9]   per landmark [3 cols][3 rows]
    float* Fdense = nullptr;   // [ldp*ldp] only in dense predict mode / ekfvio_linearize
    // --- update work ---
    int* idx = nullptr;        // [m_cap] state index of measurement row r
    int* inv_idx = nullptr;    // [ldp]   measurement row of state index j, or -1
    float* zmeas = nullptr;    // [2*max_features] device copy of z
    float* Rmeas = nullptr;    // [4*max_features]
    uint8_t* pass = nullptr;   // [max_features]
    float* yres = nullptr;     // [m_cap] measured coordinate per measurement row (the residual is formed in gather_kernel)
    float* Rm = nullptr;       // [m_cap*2] per measurement row r: R(r,r) and the off-diagonal partner
    // Augmented sweep matrices, ld_aug x m_cap, column-major.  Row blocks of Saug:
    //   [0, m_pad)                 A = (H Sigma H^T + R)^T           -> Laug: L (Cholesky factor)
    //   [m_pad, m_pad+n_pad)       Sigma H^T                         -> Laug: Y = Sigma H^T L^-T
    //   [m_pad+n_pad, +m_pad)      identity                          -> Laug: L^-T
    float* Saug = nullptr;
    float* Laug = nullptr;
    int ld_aug = 0;            // m_cap + ldp + m_cap
    float* Linv = nullptr;     // [64*m_cap] inverses of the 16x16 diagonal blocks of L
    unsigned long long* Lsign = nullptr;  // [>= m_cap/64] per block column: mask of negative pivots (0 = positive definite block)
    int* sweep_sync = nullptr; // flags of the persistent sweep, laid out by plan.h's PersistFlags (sweep_sync_words ints)
    size_t sweep_sync_words = 0;
    bool sweep_latched_off = false;  // an aborted persistent sweep has retired the persistent launch (sweep_abort_latch sets it, sweep_maybe_retry clears it)
    long long persistent_sweeps = 0;  // sweeps enqueued (or captured) as chol_persist_kernel: ekfvio_test_persistent_sweeps
    long long schur_sweeps = 0;       // sweeps enqueued with Sigma and the gain as Schur tiles (EKFVIO_SCHUR=1): ekfvio_test_sweep_counts
    long long sweep_recoveries = 0;   // updates run again with the per-step sweep behind an aborted persistent launch
    long long early_output_frames = 0;  // frames whose outputs went out between the update's two Joseph GEMMs (Tuning::early_outputs; test hook)
    int sweep_spin_limit = 0;         // > 0: looks per wait of the persistent sweep (test hook ekfvio_test_sweep_fault); 0: SWEEP_SPIN_LIMIT
    int sweep_stall_wg = -1;          // fault injection: this workgroup of the persistent launch never raises its flag
#ifdef EKFVIO_TEST_HOOKS
    int sweep_delay_wg = -1, sweep_delay_point = 0, sweep_delay_ticks = 0;  // ekfvio_test_sweep_delay: this owner of the persistent launch stores late (PersistArgs::delay_wg)
#endif
    bool sweep_retry_armed = false;    // sweep_latched_off is tried again at sweep_retry_at (api.hip, sweep_maybe_retry)
    double sweep_retry_pause_s = 0.0;  // (its first value: Tuning::sweep_retry_first_s)
    int sweep_probation = 0;           // > 0: clean persistent sweeps still to come behind a retry before sweep_retry_pause_s starts over (api.hip)
    std::chrono::steady_clock::time_point sweep_retry_at;
    bool sweep_flags_clean = false;   // the persistent sweep's flags are zero for the launch enqueued next (zeroed by the last GEMM of the
                                      // previous update); otherwise gather_potrf_kernel zeroes them in front, or launch_update has a memset enqueued
    bool persist_attr_set = false;
    bool gain2_attr_set = false;
    bool gather_attr_set = false;
    long long t2_updates = 0;  // updates enqueued (or captured) with the T2 flow: ONE P-update GEMM behind the sweep (ekfvio_get_counters [5])
    long long graph_steps = 0;          // filter steps enqueued as graph replays (ekfvio_run_uploaded; ekfvio_get_counters [6])
    long long prelinearized_steps = 0;  // replayed process(dt) launches that found their linearisation done by the previous update's GEMM ([7]; GraphCache::Entry::pre)
    int num_cus = 0;
    int last_m = 0;            // measurement rows of the most recent update (shape of its GEMMs)
    long long* sweep_dbg = nullptr;  // [512] s_memtime stamps of the persistent sweep (diagnostic; null = off)
    long long* gemm_stamps = nullptr;  // diagnostic stamp buffer handed to the next GEMM launches (null = off)
    float* Km = nullptr;       // [ldp*m_cap]  Sigma H^T, solved in place into the Kalman gain
    float* Wt = nullptr;       // [ldp*m_cap]  (H Sigma)^T
    float* Gm = nullptr;       // [ldp*m_cap]  K R - T[:,idx]
    int* info = nullptr;       // [4] device words: [0] non-positive pivot seen, [1] frame counter of uploaded sequences, [2] device-side m
    // --- innovation gate (ekfvio_set_gate; gate_bookkeeping_kernel in ekf_kernels.hip) ---
    float gate_chi2 = 0.f;        // > 0: landmarks whose squared Mahalanobis distance exceeds it are treated as failed by the tracker; 0: off
    // (device memory: one allocation, made by the first ekfvio_set_gate with chi2 > 0; gate_words is its base)
    float* gate_d2 = nullptr;     // [max_features] d2 of the most recent gated update (-1: not evaluated)
    uint8_t* gate_flag = nullptr; // [max_features] 1: rejected by that update's gate
    uint8_t* gate_pass = nullptr; // [max_features] the effective pass flags of that update (per-frame scratch: an uploaded sequence is never written)
    int* gate_words = nullptr;    // [4] device words: [0] gated by the last update, [1] landmarks it saw, [2..3] total since create/reset (one 64-bit word)
    // --- forward-backward check of the tracker (ekfvio_set_klt_fb; threshold: cfg.klt_fb_max_px, 0 = off; klt_track_kernel in klt.hip) ---
    // (device memory: one allocation, made by the first track that needs it; fb_words is its base)
    int* fb_words = nullptr;      // [8] device words: [0] landmarks rejected by the last track, [1] landmarks it saw, [2..3] total since create/reset (one 64-bit
                                  // word), [4] the running count and [5] the ticket of a launch (zero between launches)
    float* fb_err2 = nullptr;     // [max_features] squared round-trip error of the last track (-1: forward track failed, -2: backward track failed)
    uint8_t* fb_flag = nullptr;   // [max_features] 1: tracked forward and rejected by the check
    float* fb_pt_err2 = nullptr;  // [max_features], fb_pt_back [2*max_features], fb_pt_flag [max_features]: the same and the backward result for the
    float* fb_pt_back = nullptr;  // points of ekfvio_klt_track_points_fb
    uint8_t* fb_pt_flag = nullptr;
    // --- the tracks that ended (ekfvio_set_ended_export; ended.hip): one record per landmark a removal is about to take out ---
    bool ended_on = false;        // every launched removal is preceded by ended_tracks_kernel
    // (pinned, device-mapped host memory: one allocation, made by the first ekfvio_set_ended_export(f, 1); h_ended is its base and ended_id the
    // device's address of it.  Layout, all sized for max_features: id, born, xyz, cov, index)
    unsigned char* h_ended = nullptr;
    int64_t* ended_id = nullptr;
    double* ended_born = nullptr;
    float* ended_xyz = nullptr;   // [3 max_features]
    float* ended_cov = nullptr;   // [9 max_features]
    int* ended_index = nullptr;   // the landmark's row in front of the removal
    int ended_count = 0;          // records of the most recent removal call since the setting went on (the host-known removed count)
    int64_t ended_total = 0;      // since create / reset
    // --- zero-velocity update (ekfvio_set_zupt; zupt.hip): the decision from the tracker's results and the update on state rows 7..12 ---
    float zupt_max_flow_px = 0.f;  // > 0: ekfvio_step_image decides behind the tracker and updates in front of the camera update; 0: off
    int zupt_min_tracks = 0;
    float zupt_min_ratio = 0.f, zupt_vel_var = 0.f, zupt_omega_var = 0.f;
    // (memory: made by the first ekfvio_set_zupt that turns the setting on)
    int* zupt_words = nullptr;     // [4] device words: stationary, n_pass, n_still, landmarks seen (the Joseph kernel reads the first)
    int* h_zupt = nullptr;         // pinned, device-mapped: the same four words, then flow2[max_features] as floats
    int* d_hzupt = nullptr;        // the device's address of h_zupt
    int zupt_n = 0, zupt_pass = 0, zupt_still = 0, zupt_applied_last = 0;  // the most recent frame's decision as the host read it with the status word
    int64_t zupt_applied_total = 0;  // since create / reset
    // --- linear aiding measurement of the base state (ekfvio_aid_update, ekfvio_set_frame_aid; aid.hip) ---
    int frame_aid_k = 0;           // > 0: ekfvio_step_image applies the standing measurement behind the tracker, in front of the zero-velocity update; 0: off
    float frame_aid_H[6 * 22] = {}, frame_aid_z[6] = {}, frame_aid_R[36] = {}, frame_aid_chi2 = 0.f;  // as given; survive ekfvio_reset
    // (memory: made by the first aiding call or the first ekfvio_set_frame_aid that turns the setting on)
    long long* aid_words = nullptr;  // [4] device words: accepted, applied and rejected since create / reset, d2's bits (the Joseph kernel reads the first)
    long long* h_aid = nullptr;      // pinned, device-mapped: the same four words
    long long* d_haid = nullptr;     // the device's address of h_aid
    bool aid_pending = false;        // an aiding launch is enqueued that no wait of the host lies behind yet: ekfvio_get_aid waits for the stream
    // --- the IMU in its own frame and gravity at run time (ekfvio_set_imu_extrinsics, ekfvio_set_gravity; imu.hip): host values alone, handed to
    // the IMU update's launch as kernel arguments; both survive ekfvio_reset ---
    bool imu_ext_on = false;      // launch_imu_update takes imu_gain_kernel<true>
    float imu_R_ci[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};  // as given: row-major, IMU -> camera axes
    float imu_p_ci[3] = {0.f, 0.f, 0.f};                                  // the IMU's origin in the camera frame (m)
    float imu_gravity[3] = {0.f, 0.f, 0.f};  // cfg.gravity at ekfvio_create, then whatever ekfvio_set_gravity said last
    int* remove_words = nullptr;  // [4] device words of the removal kernel (remove.hip): [0] landmarks added - removed, [1] removed, [2] its ticket
    int* h_info = nullptr;     // pinned, device-mapped: the words of enum HostWord
    int* d_hinfo = nullptr;    // the device's address of h_info
    int status_seq = 0;
    // small per-frame outputs (odometry, point cloud): kernels write them straight into pinned host memory and the host
    // waits with wait_status: no device-to-host copy into pageable memory, no interrupt-driven synchronise
    float* h_out = nullptr;    // pinned, device-mapped: base_mu[22], xyz[3 N], intensity[N] in the first EKF_BASE + 4 * max_features floats, then
                               // at fixed offsets (out_cov_offset) pose_cov[36], twist_cov[36], cov[9 N]: EKF_BASE + 72 + 13 * max_features floats,
                               // then, 8-byte aligned (out_ids_offset), id[max_features] as int64 and born[max_features] as double
    float* d_out = nullptr;    // the device's address of h_out
    bool out_fresh = false;    // h_out holds base_mu and the point cloud of the CURRENT state and frame: ekfvio_step_image's last
                               // kernel writes them with the status word, and every call that changes the state or the frame
                               // clears the flag; while it is set the node's getters cost a memcpy
    bool output_cov = false;   // ekfvio_set_output_covariance: the frame's outputs include the covariances of include/ekfvio.h (and never go out early)
    bool out_cov_fresh = false;  // ... and the fresh outputs (out_fresh) do include them: cleared, besides, by what changes Sigma alone (ekfvio_set_feature_cov)
    unsigned char* h_meas = nullptr;  // pinned staging for one frame's (z, R, pass): one H2D copy per ekfvio_update
    unsigned char* d_meas = nullptr;  // its device image: z at 0, R at 8N_cap, pass at 24N_cap bytes
    // uploaded measurement sequences
    float* seq_z = nullptr;
    float* seq_R = nullptr;
    uint8_t* seq_pass = nullptr;
    int seq_frames = 0;
    int seq_N = 0;
    std::vector<int> seq_m;                 // measurement rows per uploaded frame
    std::vector<std::vector<uint8_t>> seq_pass_host;

    // --- KLT ---
    KltFrame frames[2];
    int cur = 0;          // index of the current frame in frames[]
    int klt_border = 0;
    float* klt_prev_px = nullptr;  // [2*max_features]
    float* klt_next_px = nullptr;  // [2*max_features]
    uint8_t* klt_status = nullptr; // [max_features]
    float* klt_cov_px = nullptr;   // [4*max_features] sample-based pixel covariances (cfg.sample_based_uncertainty)
    bool klt_photo = false;        // ekfvio_set_klt_photometric: the tracker's launches take klt_track_kernel<true> (gain/offset term; klt_photo.h)
    uint8_t* staging = nullptr;    // device staging for the uploaded image
    uint8_t* h_image = nullptr;    // pinned host staging: the caller's frame is copied here, so its buffer is free on return without a stream sync
    size_t src_cap = 0;            // bytes of staging / h_image (the uploaded, un-resized frame)
    // --- rectification of distorted frames (ekfvio_set_distortion; rectify.hip) ---
    double dist[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the model's coefficients in the caller's order (ekfvio_set_camera_model), zeros behind dist_count
    int dist_count = 0;            // the count the last setter was given
    int cam_model = 0;             // EKFVIO_CAMERA_*: which instance of rectify_map_kernel forms the map
    float cam_P[4] = {0, 0, 0, 0}; // fx', cx', fy', cy' of the rectified camera, where cam_has_P
    bool cam_has_P = false;        // frames are rectified onto P, and everything behind the rectification takes P for the frame's K
    bool rect_on = false;          // the setting is on (a coefficient, the equidistant model or P): frames pass rectify_kernel between the upload and the pyramid
    // (device memory: allocated with the first frame pushed while rect_on, ensure_frame_capacity in klt.hip)
    int* rect_sx = nullptr;        // [rect_cap + 16] the map, fixed point with 5 fractional bits; INT32_MIN: no source pixel
    int* rect_sy = nullptr;
    uint8_t* rect_img = nullptr;   // [rect_cap + 16] the rectified full-size frame: a second staging plane, what the pyramid kernel then reads
    size_t rect_cap = 0;           // pixels the three were allocated for
    RectifyKey rect_key;           // what the map in rect_sx / rect_sy was formed for
    bool rect_key_valid = false;
    // --- no-data mask (ekfvio_set_mask; mask.hip): the blocked map B of include/ekfvio.h, read by the detector and the tracker ---
    bool mask_on = false;          // a caller's mask or a flag is set: B is formed (once per MaskKey) behind the rectification of a pushed frame
    int mask_flags = 0;            // EKFVIO_MASK_*
    // (device memory: the caller's copy is allocated by ekfvio_set_mask, the rest with the first frame pushed while mask_on, mask_ensure)
    uint8_t* mask_user = nullptr;  // [mask_uw * mask_uh] the caller's mask, tightly packed (null: none)
    int mask_uw = 0, mask_uh = 0;  // its size: the FULL frame size every pushed frame must then have
    unsigned mask_user_gen = 0;    // counts the caller's masks this handle has been given
    unsigned* mask_nodata = nullptr;   // [mask_cap_words] N, in OccMask's layout (fast.hip): (W + 31) / 32 words per row, tail bits 1
    unsigned* mask_blocked = nullptr;  // [mask_cap_words] B, likewise
    size_t mask_cap_words = 0;
    MaskKey mask_key;              // what B was formed for
    bool mask_key_valid = false;
    int mask_bw = 0, mask_bh = 0;  // level-0 size of the B the device holds (0: none -- no frame pushed with the mask on, or off since)
    uint8_t* mask_hit = nullptr;   // [max_features] 1: the most recent track's landmark was let through by everything else and masked
    int mask_hits_n = 0;           // the landmark count that track saw
    // --- equalisation of pushed frames (ekfvio_set_equalize; equalize.hip): clip-limited tile histograms, in place on the full-size frame ---
    bool eq_on = false;            // clip limit > 0: frames pass the two equalize kernels between the rectification and the pyramid
    float eq_clip = 0.f;           // the setting as given
    int eq_tx = 0, eq_ty = 0;
    // (device memory: allocated with the first frame pushed while eq_on, ensure_frame_capacity in klt.hip)
    uint8_t* eq_lut = nullptr;     // [eq_lut_cap] one 256-byte table per tile, row-major tiles
    size_t eq_lut_cap = 0;
    // --- frame ingest + replenishment (fast.hip) ---
    uint8_t* blurred = nullptr;    // replenishFeatures' cv::GaussianBlur output (only with cfg.fast_blur_sigma != 0)
    unsigned* fast_row_kp = nullptr;  // [w*h] per image row its keypoints in x order, (score << 16) | x
    int* fast_kp_xy = nullptr;     // keypoints in raster order
    short* fast_kp_score = nullptr;
    int fast_kp_cap = 0;
    uint8_t* occ_mask = nullptr;   // replenishFeatures' checkImg as a bit mask (global fallback for large frames)
    int* fast_row_cnt = nullptr;   // [max_image_height] keypoints per row
    int* new_xy = nullptr;         // pixels of the landmarks added by the last replenishment
    int* fast_counts = nullptr;    // [0] keypoints found, [1] landmarks added
    int fast_cap_w = 0, fast_cap_h = 0;  // level-0 size the detector's buffers were allocated for
    int replenish_cells_x = 0, replenish_cells_y = 0;  // ekfvio_set_replenish_grid: (0, 0) = off, the raster first fit; else replenish_select_kernel's grid instance
    double t_stamp = 0;
    bool have_stamp = false;

    GraphCache graphs;  // hipGraph replay of device-resident sequences (ekfvio_run_uploaded)

    // --- profiler ---
    bool prof_on = false;
    float prof_overhead_ms = 0.f;  // elapsed time of an empty event pair, subtracted from every scope
    ProfSlot prof[PC_COUNT];
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

// ---- memory: every allocation of the library is an acquire on a ledger (mem.h) ---------
// A non-null *p is released first (a grow); on failure *p is null.  dev_alloc: `count` elements, zero-filled on stream s -- nothing in this
// library relies on the legacy null stream, which a non-blocking stream does not wait for; dev_alloc_bare: `bytes` as they come.
inline hipError_t mem_error(int rc) { return rc == MEM_ERR_FOREIGN ? hipErrorInvalidDevicePointer : (hipError_t)rc; }
template <class T>
hipError_t dev_alloc(MemLedger& mem, hipStream_t s, T** p, size_t count) {
    const size_t bytes = sizeof(T) * (count ? count : 1);
    hipError_t e = mem_error(mem.acquire(p, bytes, MEM_DEVICE));
    if (e == hipSuccess) e = hipMemsetAsync(*p, 0, bytes, s);
    return e;
}
template <class T>
hipError_t dev_alloc(ekfvio_filter* f, T** p, size_t count) { return dev_alloc(f->mem, f->stream, p, count); }
template <class T>
hipError_t dev_alloc_bare(ekfvio_filter* f, T** p, size_t bytes) { return mem_error(f->mem.acquire(p, bytes, MEM_DEVICE)); }
template <class T>
hipError_t host_alloc(ekfvio_filter* f, T** p, size_t bytes, MemKind kind) { return mem_error(f->mem.acquire(p, bytes, kind)); }

// ---- launchers implemented across the translation units -------------------------------
// C[MxN] = beta*Cin + alpha * A[MxK] * op(B); all column-major.  transB: B is [NxK]
// (op = transpose) else [KxN].  K must be a multiple of 32 and the K-padding of both
// operands finite*0-safe (zero).  flush != 0 applies the reference's prune (|x|<=1e-13 -> 0).
// Filter-specific epilogues of the P-update GEMMs (GemmEpi::mode, a GemmEpiMode of plan.h):
//  EPI_JOSEPH1 (1)       T = Sigma - K (H Sigma): besides T, writes G = K R - T[:, idx] for the measured columns (inv_idx: state
//                        index -> measurement row or -1) so that no separate pass re-reads T; the residual rides as an extra row of
//                        (H Sigma)^T, so output column n receives K*y.
//  EPI_MEAN (2)          Sigma' = T + G K^T: with n > 0 one more workgroup (gemm16_kernel; workgroup (0,0) of the 64 x 64 kernel) also
//                        finishes the mean: mu += column n, quaternion renormalised (:600-609), column n zeroed again, frame counter
//                        advanced, the persistent sweep's flags zeroed.  In the throughput regime the product may be formed mirrored (sym).
//  EPI_MEAN_PARTIAL (3)  Sigma' = T2 + K G'^T, the ONE GEMM of the T2 tail (the default where it applies) and of the Schur tail: the same
//                        finish with K y taken from per-column-block partial sums (Kyp); the only mode the next process(dt)'s
//                        linearisation rides in (lin_blocks).
// The caller fills what the epilogue works on; how the launch is shaped (lin_blocks as kept, mean_keep, sym as heeded, sym_w, order2d) is
// plan_gemm's answer (plan.h), written into the kernel's copy by launch_gemm.
struct GemmEpi {
    int mode = 0;
    const int* inv_idx = nullptr;
    const float* Rm = nullptr;
    float* G = nullptr;
    int ldg = 0;
    float* mu = nullptr;
    float* Pcol = nullptr;  // column n of P
    const float* Kyp = nullptr;  // mode 3: K y as `kyp_blocks` partial sums (rows of ld kyp_ld), added in order, instead of Pcol
    int kyp_blocks = 0, kyp_ld = 0;
    int n = 0;
    int* frame_counter = nullptr;
    int frames = 0;
    long long* stamps = nullptr;  // diagnostic s_memtime stamps (library built with -DEKF_GEMM_STAMPS), per handle
    int* zero_words = nullptr;    // modes 2-3: the persistent sweep's flags, zeroed by workgroup (0,0) for the NEXT update's sweep
    int n_zero = 0;               // (everything but the abort word, which only ever goes up and retires the persistent path)
    int order2d = 0;              // gemm_f32_mfma_kernel: each XCD's run of tiles is a compact 2-D patch (GemmPlan::order2d)
    // round 6 (mode 3, gemm16_kernel): the linearisation of the NEXT process(dt) in `lin_blocks` workgroups behind the tiles' and the mean's -- a device-resident run
    // knows the next dt, and K y is final before the launch (Kyp), so numericallyLinearizeProcess (:176-325) and the mean propagation at mu + K y run while
    // this launch's tiles do, and the covariance propagation behind it only has the strips left (motion_model.inc, launch_update)
    int lin_blocks = 0;
    int lin_N = 0;
    float lin_dt = 0.f;
    float* lin_FA = nullptr;
    float* lin_FB = nullptr;
    float* lin_FD = nullptr;
    float* lin_mu_next = nullptr;
    int mean_keep = 0;            // (GemmPlan::mean_keep, with lin_blocks) gemm16_finish_mean leaves mu alone
    int sym_w = 1;                // ... in strips of sym_w tile columns, each walked row by row
    int sym = 0;                  // EPI_MEAN: the caller asks for the mirrored form; where plan_gemm heeds it (gemm_f32_mfma_kernel) only the lower triangle's tiles are formed, each also writes its transpose
    const int* abort = nullptr;   // modes 1-3: abort word of the persistent sweep in front (non-zero: the factor is unfinished) --
                                  // the kernel then writes nothing: Sigma, mu and the frame counter stay as process(dt) left them
};
// One GEMM launch by name: operands with their leading dimensions, the scalars, and the epilogue
struct GemmCall {
    int M = 0, N = 0, K = 0;
    bool transB = false;
    bool flush = false, lowerB = false;  // the reference's prune on the way out; B is lower triangular (the contraction starts at the tile's column)
    float alpha = 1.f, beta = 0.f;
    const float *A = nullptr, *B = nullptr, *Cin = nullptr;  // Cin: read only with beta != 0
    float* C = nullptr;
    int lda = 0, ldb = 0, ldcin = 0, ldc = 0;
    GemmEpi epi;
    int variant = 0;  // GemmShape::variant (the two GEMM test hooks; no epilogue)
};
inline GemmShape gemm_shape(const GemmCall& c) {  // what plan_gemm (plan.h) may depend on
    GemmShape s;
    s.M = c.M, s.N = c.N, s.K = c.K, s.transB = c.transB, s.lowerB = c.lowerB;
    s.epi = c.epi.mode, s.mean = c.epi.n > 0, s.lin_blocks = c.epi.lin_blocks, s.sym = c.epi.sym != 0, s.variant = c.variant;
    return s;
}
void launch_gemm(ekfvio_filter* f, const GemmCall& c);  // plans (plan_gemm) and launches

// Measurement bookkeeping of one update (device pointers); see bookkeeping_body in ekf_kernels.hip
struct BookArgs {
    int enabled = 0;
    int N = 0, m_pad = 0;
    const float* z = nullptr;
    const float* R = nullptr;
    const uint8_t* pass = nullptr;
    float* last_klt = nullptr;
    uint8_t* del_flag = nullptr;
    int* idx = nullptr;
    int* inv_idx = nullptr;
    float* zrow = nullptr;  // measured coordinate per measurement row (f->yres)
    float* Rm = nullptr;
    const int* frame_counter = nullptr;
    int* m_out = nullptr;   // receives the number of measurement rows 2 * (#passed) (device-side m, ekfvio_step_image)
    // innovation gate (gate_bookkeeping_kernel only): the bookkeeping then runs over pass_eff, which the gate fills for this frame
    uint8_t* pass_eff = nullptr;  // [N] effective flags = pass && accepted (never offset by the frame counter)
    const float* mu = nullptr;    // the propagated state the update is about to read
    const float* P = nullptr;
    int ldp = 0;
    float chi2 = 0.f;
    float* d2 = nullptr;          // [N] (-1: not evaluated)
    uint8_t* gated = nullptr;     // [N]
    int* gate_words = nullptr;    // ekfvio_filter::gate_words
    int count_total = 0;          // 0: a re-run of an update already counted (UpdateInputs::gate_counted)
};
BookArgs make_book_args(ekfvio_filter* f, int m, const float* d_z, const float* d_R, const uint8_t* d_pass, const int* d_frame_counter);
void launch_linearize(ekfvio_filter* f, float dt, const BookArgs* book = nullptr);
void launch_build_dense_F(ekfvio_filter* f, float* Fdense);
// prelinearized: the previous update's last GEMM linearised for this step (UpdateResult::linearised_next): FA / FB / FD / mu_next hold its Jacobian
// blocks and propagated mean.  Returns whether the launch relied on that (PredictPlan::pre)
bool launch_predict(ekfvio_filter* f, float dt, const BookArgs* book = nullptr, bool prelinearized = false);
// m_on_device: the host does not know how many landmarks passed (no D2H of the flags): launches are sized for m = 2N,
// the kernels read the true row count from f->info[2] (written by the bookkeeping) and treat the rest as padding
struct UpdateInputs {
    int m = 0;  // measurement rows 2 * (#passed) as the host knows them (ignored with m_on_device)
    const float *z = nullptr, *R = nullptr;  // device-resident measurement: z, R, pass flags
    const uint8_t* pass = nullptr;
    int* frame_counter = nullptr;  // device-side frame index of an uploaded sequence (null: z / R / pass are one frame), of `frames` frames
    int frames = 0;
    bool bookkeeping_done = false;  // the measurement bookkeeping ran already (in the process(dt) launch, or in the update this one runs again)
    bool m_on_device = false;
    bool gate_counted = false;  // the gate of this update has been added to the running total already (the re-run behind an aborted persistent sweep)
    float next_dt = -1.f;  // >= 0 (capture_steps): the next process(dt)'s dt -- the update's last GEMM may linearise for it; mu is then stale until that process(dt)
    int publish_seq = 0;       // ekfvio_update: the status word goes out with this sequence number right behind the sweep (0: not asked)
    // ekfvio_step_image: called between the update's two Joseph GEMMs, or in front of the T2 flow's one (the frame's outputs); kyp_blocks > 0: K y is
    // Wt's first rows (one per block column), not column n of P.  Returns the status sequence number its launch publishes
    int (*between)(ekfvio_filter*, int kyp_blocks) = nullptr;
    bool recoverable = true;   // false (ekfvio_run_uploaded): nothing can run an aborted update again -- the persistent sweep waits the long bound
};
struct UpdateResult {
    bool published = false;  // the status went out behind the sweep (publish_seq; false: no sweep ran)
    int between_seq = 0;     // what `between` returned (0: not reached -- no measurement, or the Schur flow)
    bool linearised_next = false;  // the last GEMM linearised for the next process(dt) (UpdateInputs::next_dt, Tuning::lin_overlap): hand it to that launch_predict
};
UpdateResult launch_update(ekfvio_filter* f, const UpdateInputs& in);
void launch_check_sigma(ekfvio_filter* f, float* d_out);
// klt.hip helpers shared with fast.hip and frame.hip
int klt_level_pitch(int w);
int klt_border();
void klt_intrinsics(const ekfvio_filter* f, const float* K, float* fx, float* fy, float* cx, float* cy);
// Level 0 of the current frame as the frame's outputs and the replenishment see it: img = pixel (0,0) inside the border, pitch in
// pixels, and the intrinsics of klt_intrinsics.  All zeros (img null) while no frame has been pushed.
struct Level0View {
    const uint8_t* img = nullptr;
    int pitch = 0, w = 0, h = 0;
    float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f;
};
Level0View klt_level0(const ekfvio_filter* f);
// Where the covariances lie in h_out / d_out (frame.hip): pose_cov[36], twist_cov[36], then 9 floats per landmark; out_words: the whole allocation
inline size_t out_cov_offset(const ekfvio_filter* f) { return EKF_BASE + 4 * (size_t)(f->cfg.max_features > 0 ? f->cfg.max_features : 1); }
// ... and the landmark ids and birth stamps behind them, in a region of their own that starts on an 8-byte boundary (in floats, as the others)
inline size_t out_ids_offset(const ekfvio_filter* f) {
    return (out_cov_offset(f) + 72 + 9 * (size_t)(f->cfg.max_features > 0 ? f->cfg.max_features : 1) + 1) & ~(size_t)1;
}
inline size_t out_words(const ekfvio_filter* f) { return out_ids_offset(f) + 4 * (size_t)(f->cfg.max_features > 0 ? f->cfg.max_features : 1); }
// What add_features_kernel stamps a new landmark with: the handle's current time, the stamp of the frame inside ekfvio_step_image; NaN before any stamp
inline double born_stamp(const ekfvio_filter* f) { return f->have_stamp ? f->t_stamp : __builtin_nan(""); }
// what the frame loop (frame.hip) enqueues of the tracker's file
int push_frame_check(ekfvio_filter* f, const uint8_t* image, int32_t width, int32_t height, int32_t stride, const float K[9]);
int push_frame_enqueue(ekfvio_filter* f, const uint8_t* image, int32_t width, int32_t height, int32_t stride, const float K[9]);
int klt_track_device(ekfvio_filter* f);  // the tracker over the current landmarks; results in f->zmeas / Rmeas / pass (device)
// imu.hip
void launch_imu_update(ekfvio_filter* f, const float gyro[3], const float accel[3]);
// zupt.hip: the frame's zero-velocity decision and update, enqueued behind the tracker (setting on, N > 0), and the host's end of it behind
// the frame's status word (decided: launch_zupt_frame ran in this frame)
void launch_zupt_frame(ekfvio_filter* f);
void zupt_note_frame(ekfvio_filter* f, bool decided);
// aid.hip: the frame's standing aiding measurement (ekfvio_set_frame_aid), enqueued behind the tracker and in front of the zero-velocity update
// (setting on), the host's end of it behind the frame's status word, and ekfvio_reset's two parts (in front of its wait and behind it): the counts start over
void launch_aid_frame(ekfvio_filter* f);
void aid_note_frame(ekfvio_filter* f);
hipError_t aid_reset_enqueue(ekfvio_filter* f);
void aid_reset_done(ekfvio_filter* f);
// fast.hip
int fast_alloc(ekfvio_filter* f);
int fast_ensure(ekfvio_filter* f, int w, int h);  // grows the detector's per-pixel buffers to a w x h level 0 (synchronises if it must)
// Waits for everything on the handle's stream and returns the factorisation's status word through *status (api.hip).
// extra_dev (may be null): one more device word delivered with it through *extra_out.
void launch_publish_status(ekfvio_filter* f, int seq);  // the status word and `seq` to pinned host memory, stream-ordered (api.hip)
int wait_status(ekfvio_filter* f, int* status, const int* extra_dev = nullptr, int* extra_out = nullptr);
// the same in two halves, for a caller whose own (single-workgroup) kernel publishes the words itself
int next_status_seq(ekfvio_filter* f);
// api.hip: what a host does when the status word says the persistent sweep gave up (bit 1): the handle goes to the per-step
// sweep for good and its captured graphs are dropped
void sweep_abort_latch(ekfvio_filter* f);
void sweep_clean_update(ekfvio_filter* f);  // an update whose persistent sweep came through (api.hip)
// api.hip: the host's end of an update, in two halves so that a caller can act between them (ekfvio_step_image).
// read_status: the status word into *bad (and HW_EXTRA into *extra, may be null) -- polled under `seq` where the caller's own launch
// publishes it, published here (with *extra_dev, may be null) where seq == 0 -- and info[0] cleared on the device if it was set.
int read_status(ekfvio_filter* f, int seq, const int* extra_dev, int* bad, int* extra);
// settle_update: an aborted persistent sweep (bit 1) latches and the update runs again through `rerun` (null: EKFVIO_EABORTED); a clean
// one counts towards the retry's probation where counts_as_clean; bit 0 of the last status read comes back as EKFVIO_ENUMERIC.
int settle_update(ekfvio_filter* f, int bad, void (*rerun)(ekfvio_filter*, void*), void* ctx, bool counts_as_clean);
void sweep_maybe_retry(ekfvio_filter* f);  // at the entry points that enqueue updates: the persistent sweep again, some time after an abort
int poll_status(ekfvio_filter* f, int seq, int* status, int* extra_out);
// api.hip: addNewFeatures with the k new (u,v) already in f->zmeas on the device
int add_features_device(ekfvio_filter* f, int k);
void add_features_enqueue_device_count(ekfvio_filter* f, const int* count_dev);  // enqueue only; the caller updates N / n
int replenish_enqueue(ekfvio_filter* f, int* enqueued);  // fast.hip: FAST + selection (first fit, or the grid's rounds), count left in f->fast_counts[1]

int live_handles_on(int device);  // api.hip: handles alive on that device in this process
void drop_graph(ekfvio_filter* f);  // api.hip: the ONE invalidation of ekfvio_filter::graphs (the next run captures again)
// The flow of ONE update is decided in one place (plan.h, plan_update: a pure function of the handle's Tuning, a PlanShape and the row count) and handed
// to the launchers as a value: they execute, they do not decide.  This is the ONE adapter from a handle to what a plan may depend on; the handle
// count is asked per plan (ekfvio_run_uploaded re-captures on it: GraphKey::sole), never cached.
inline PlanShape plan_shape(const ekfvio_filter* f) {
    PlanShape s;
    s.num_cus = f->num_cus, s.ldp = f->ldp, s.sweep_sync_words = f->sweep_sync_words, s.N = f->N, s.n = f->n;
    s.dense_predict = f->cfg.predict_mode == EKFVIO_PREDICT_DENSE;
    s.sole_handle = live_handles_on(f->device) <= 1;
    s.latched_off = f->sweep_latched_off;
    return s;
}
inline UpdatePlan plan_update(const ekfvio_filter* f, int m, bool m_on_device = false, float next_dt = -1.f, bool recoverable = true) {
    return plan_update(f->tune, plan_shape(f), m, m_on_device, next_dt, recoverable);
}
// The P-update GEMM launches of an update with plan p, `reps` times, into scratch (P2, Gm): the
// filter state is not touched.  For timing the kernel under its production shape (ekfvio_profile_update_gemms).
// Returns the GEMM launches per repetition (2 with the two-GEMM tail, else 1); last_flops: the EXECUTED flops of the last of them (gemm_executed_flops)
int launch_update_gemms_scratch(ekfvio_filter* f, const UpdatePlan& p, int reps, double* last_flops);
// Augmented blocked Cholesky sweep (chol.hip): Saug = [A; X; I] (row blocks of 64; A is
// m_pad x m_pad, X has n_pad rows) -> Laug = [L; X L^-T; L^-T], both ld x m_pad column-major.
// zero_flags: a memset of the persistent sweep's flags goes in front.  Returns the abort word of the persistent launch (null: another sweep)
const int* launch_chol_sweep(ekfvio_filter* f, const UpdatePlan& p, float* Saug, float* Laug, float* Linv, int ld, bool zero_flags);
const int* launch_persist_fused(ekfvio_filter* f, const UpdatePlan& p, bool zero_flags);
// K pruned, G = K R - T[:, idx], K y partial sums (one row of f->Wt per 64 measurement columns)
void launch_joseph_g(ekfvio_filter* f, int m, int m_pad, int n_pad, bool m_on_device, const float* T = nullptr);  // T: the covariance G' is taken from (null: f->P)
// Where T2 lives between the sweep and the one GEMM behind it: the dense-F buffer, dead during an update in either predict mode (the dense
// mode rebuilds F at the next process(dt)).  Not f->P2: that is process(dt)'s next output, and with T2 written there by other XCDs moments
// earlier process(dt) measured 0.6 us longer (same-box rocprofv3: 9.51 against 8.90 us).
inline float* t2_buffer(ekfvio_filter* f) { return f->Fdense; }
void launch_gain2_tiles(ekfvio_filter* f, const UpdatePlan& p);
void launch_gather_potrf(ekfvio_filter* f, const UpdatePlan& p);
void launch_potrf_stamps(ekfvio_filter* f, const float* S, int ld, float* L, float* Linv, long long* d_stamps);
// K = X A^-1 (n rows, ldk) from the sweep output, as the plan says: gain_tiles_kernel, or the GEMM K = Y L^-1 (+ optional residual refinement).
void launch_gain_from_sweep(ekfvio_filter* f, const UpdatePlan& p, const float* Laug, int ld, int n, float* K, float* scratch, int ldk, int refine);

// ended.hip: with ekfvio_set_ended_export on, launch_remove_features puts this in front of its own launch with its own arguments: one record
// per landmark the removal is about to take out, from the mean and Sigma as they stand (f->mu, f->P)
void launch_ended_tracks(ekfvio_filter* f, const uint8_t* remove, const int* added, bool abort_aware);
void ended_note_removal(ekfvio_filter* f, int removed);  // the host-known count of a removal call (0 included) behind it
// remove.hip: Sigma, mu, last_klt, del_flag, lm_id, lm_born compacted in ONE launch over N + *added landmarks (added may be null); decision from
// `remove` (device memory), null: del_flag; abort_aware: nothing removed behind an aborted persistent sweep; host_removed: the
// count into the pinned host word HW_REMOVED too
void launch_remove_features(ekfvio_filter* f, const uint8_t* remove, const int* added, bool abort_aware, bool host_removed);
size_t remove_lds_bytes(const ekfvio_filter* f);
void remove_applied(ekfvio_filter* f, int delta, int removed);  // the host side behind a launch: pointer swaps, N, n, graphs
// rectify.hip
int rectify_ensure(ekfvio_filter* f, size_t src);  // the map planes and the second staging buffer for a frame of src pixels (the caller has waited for the stream)
const uint8_t* rectify_enqueue(ekfvio_filter* f, const uint8_t* src, int w, int h, const float K[9], hipStream_t st);  // returns the rectified frame
// mask.hip
int mask_check_frame(ekfvio_filter* f, int width, int height);  // EKFVIO_EINVAL (and last_error) for a frame that is not the caller's mask's size
int mask_ensure(ekfvio_filter* f, int w, int h);  // the bit planes for a w x h level 0 and the hit flags (waits for the stream if it must allocate)
void mask_enqueue(ekfvio_filter* f, int width, int height, int w, int h, int s, hipStream_t st);  // forms B if its key changed; behind rectify_enqueue
// B for a w x h level 0 as the device holds it (words per row: (w + 31) / 32), or null: the mask is off, or was formed for another size
inline const unsigned* mask_blocked_for(const ekfvio_filter* f, int w, int h) {
    return (f->mask_bw == w && f->mask_bh == h && w > 0) ? f->mask_blocked : nullptr;
}
// equalize.hip
int equalize_check_frame(ekfvio_filter* f, int width, int height);  // EKFVIO_EINVAL (and last_error) for a frame with fewer columns or rows than tiles
int equalize_ensure(ekfvio_filter* f);  // the tables for the current setting (the caller has waited for the stream)
void equalize_enqueue(ekfvio_filter* f, uint8_t* full, int w, int h, hipStream_t st);  // equalises the full-size frame in place; behind rectify_enqueue
int klt_alloc(ekfvio_filter* f);  // klt.hip

struct ProfScope {
    ekfvio_filter* f;
    int cls;
    int launches;
    ProfScope(ekfvio_filter* f_, int cls_, double flops = 0, int launches_ = 1) : f(f_), cls(cls_), launches(launches_) {
        if (f->prof_on) {
            (void)hipEventRecord(f->ev0, f->stream);
            f->prof[cls].flops += flops;
        }
    }
    ~ProfScope() {
        if (f->prof_on) {
            (void)hipEventRecord(f->ev1, f->stream);
            (void)hipEventSynchronize(f->ev1);
            float ms = 0;
            (void)hipEventElapsedTime(&ms, f->ev0, f->ev1);
            f->prof[cls].ms += ms;  // raw: includes the event-pair overhead (f->prof_overhead_ms, reported separately)
            f->prof[cls].launches += launches;
        }
    }
};
