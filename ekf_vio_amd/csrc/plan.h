// ekf_vio_amd/csrc/plan.h — everything that DECIDES: the run-time switches, the sizes a capacity implies, and the flow of one update.
// Standard headers only (no HIP, no project header): integer arithmetic over a Tuning, a PlanShape and a row count, so the decision
// table of the product is checked on a machine without a GPU (include/ekfvio_test_hooks.h: ekfvio_test_plan, ekfvio_test_gemm_plan,
// ekfvio_test_predict_plan, ekfvio_test_run_plan; tests/test_plan_cpu.py, tests/test_gemm_plan_cpu.py, tests/test_resident_cases_cpu.py).
// The launchers execute what is planned here, they do not decide: an UpdatePlan (chol.hip, ekf_kernels.hip: launch_update), a GemmPlan per GEMM
// launch (gemm.hip: launch_gemm), a PredictPlan per process(dt) (ekf_kernels.hip: launch_predict), a RunPlan per device-resident run (api.hip:
// ekfvio_run_uploaded).
#ifndef EKFVIO_PLAN_H_
#define EKFVIO_PLAN_H_
#include <stddef.h>
#include <stdlib.h>

#include <algorithm>

#define EKF_BASE 22
#define EKF_TILE 64  // block size of every blocked algorithm (GEMM tile edge, Cholesky nb; chol.hip's PB)
#ifndef EKF_SWEEP_SPLIT_MB
#define EKF_SWEEP_SPLIT_MB 16  // from this many 64-wide block steps on, the sweep solves each panel block once (chol.hip)
#endif
#define LIN_LM 8  // landmarks per linearising workgroup (32 lanes each; motion_model.inc)
#define GC 4      // measurement columns whose loads one element workgroup of the gather keeps in flight together (gather_body.inc)
#define GCI 4     // ... and how many such groups it walks through (GC*GCI columns per workgroup)

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// ---- the switches --------------------------------------------------------------------------------------------------------------
// Read ONCE per handle, in ekfvio_create; every member's default is the production flow.
struct Tuning {
    int early_status = 1;    // EKFVIO_EARLY_STATUS: ekfvio_update returns behind the sweep, the Joseph GEMMs still running (api.hip); 0: behind the update's last kernel (rounds 1-3)
    int upload_kernel = 1;   // EKFVIO_UPLOAD_KERNEL: the frame's trip to device memory is a kernel reading mapped host memory (klt.hip); 0: the copy engine
    int sweep_wait_ticks = 300000;  // the persistent sweep's patience per wait in 100 MHz ticks (3 ms; EKFVIO_SWEEP_WAIT_MS) where an aborted update
                                    // is run again at once (ekfvio_update, ekfvio_step_image); a device-resident run (ekfvio_run_uploaded), which
                                    // cannot, waits SWEEP_WAIT_TICKS_UNRECOVERABLE (100 ms): the counter also runs while a healthy sweep's
                                    // wavefronts are descheduled (time slicing, a profiler's serialisation), ADVICE r05
    double sweep_retry_first_s = 2.0;  // EKFVIO_SWEEP_RETRY_S: the first pause before a handle whose persistent sweep gave up tries it again
    int persist_sweep = 1;   // 1: ONE persistent launch with per-tile hand-offs behind the first diagonal tile (chol_persist.inc), where it pays and applies
                             // (3 .. 15 block columns, grid co-resident; two block columns: 43.5 against 43.0 us per step); EKFVIO_SWEEP=0: one launch per block step
    int sweep_la = 1;        // EKFVIO_SWEEP_LA=0 (diagnostic): the two-launch split sweep (panel launch + tile launch per block step)
    int fuse_gather = 1;     // 1: the gather and the first diagonal tile's factorisation share a launch (EKFVIO_FUSE_GATHER)
    int fuse_sweep = 1;      // 1: gather + first diagonal tile + sweep in ONE launch where the persistent sweep applies (EKFVIO_FUSE_SWEEP; 0: two launches, round 3)
    int t2_flow = 1;         // 1 (EKFVIO_T2=0 turns it off: rounds 4-5): where the fused persistent launch forms the gain, freed owners also form T2 = Sigma (I - K H)^T
                             // (chol_persist.inc, t2_tile): Sigma' = T2 + K G'^T is the ONE P-update GEMM behind the launch (round 6)
    int schur = 0;           // 1 (EKFVIO_SCHUR=1): T2 and K as Schur tiles of the sweep; 0: gain GEMM + first Joseph GEMM behind it.
                             // Measured equal in step time at N = 256, so the simpler flow is the default.
    int persist_oversub = 0; // > 0 (EKFVIO_PERSIST_OVERSUB): owner workgroups allowed per compute unit's worth of the persistent launch (persist_shape)
    int persist_gain = 1;    // 1 (EKFVIO_PERSIST_GAIN=0 turns it off): the gain's tiles are formed inside the fused persistent launch (chol_persist.inc)
    int persist_early = 1;   // 1 (EKFVIO_PERSIST_EARLY=0 turns it off): owners fetch their panel sources in front of the wait for ready[k] (chol_persist.inc)
    int frame_outputs = 1;   // 1: ekfvio_step_image's last kernel also writes the node's outputs (EKFVIO_FRAME_OUTPUTS=0: status word only)
    int early_outputs = 1;   // EKFVIO_EARLY_OUTPUTS: a frame's outputs and status go out between the update's two Joseph GEMMs (klt.hip); 0: behind its last kernel
    int gemm_order2d = 1;    // EKFVIO_GEMM_ORDER2D=0: the 64 x 64 GEMM's tiles in block-index order (rounds 1-4)
    int lin_overlap = 1;     // EKFVIO_LIN_OVERLAP=0: every process(dt) of a device-resident run linearises for itself (rounds 3-5)
    int sym_joseph = 1;      // EKFVIO_SYM_JOSEPH=0: the second Joseph GEMM of the throughput regime forms both triangles (rounds 1-5)
    int fuse_linearize = 1;  // 1: structured process(dt) is one launch, the Jacobian blocks are formed inside it (EKFVIO_FUSE_LINEARIZE; 0: two launches)
};

// The ONE place the environment is read for a switch.  FLAG: atoi(e) ? 1 : 0; RAW: atoi(e); WAIT_MS: only if atof(e) > 0, in 100 MHz
// ticks; POSITIVE: only if atof(e) > 0.
inline Tuning tuning_from_env() {
    enum Kind { FLAG, RAW, WAIT_MS, POSITIVE };
    struct Entry {
        const char* name;
        Kind kind;
        int Tuning::*i;
        double Tuning::*d;
    };
    static const Entry table[] = {
        {"EKFVIO_EARLY_STATUS", FLAG, &Tuning::early_status, nullptr},
        {"EKFVIO_UPLOAD_KERNEL", FLAG, &Tuning::upload_kernel, nullptr},
        {"EKFVIO_SWEEP_WAIT_MS", WAIT_MS, &Tuning::sweep_wait_ticks, nullptr},
        {"EKFVIO_SWEEP_RETRY_S", POSITIVE, nullptr, &Tuning::sweep_retry_first_s},
        {"EKFVIO_SWEEP", FLAG, &Tuning::persist_sweep, nullptr},
        {"EKFVIO_SWEEP_LA", FLAG, &Tuning::sweep_la, nullptr},
        {"EKFVIO_FUSE_GATHER", FLAG, &Tuning::fuse_gather, nullptr},
        {"EKFVIO_FUSE_SWEEP", FLAG, &Tuning::fuse_sweep, nullptr},
        {"EKFVIO_T2", FLAG, &Tuning::t2_flow, nullptr},
        {"EKFVIO_SCHUR", FLAG, &Tuning::schur, nullptr},
        {"EKFVIO_PERSIST_OVERSUB", RAW, &Tuning::persist_oversub, nullptr},
        {"EKFVIO_PERSIST_GAIN", FLAG, &Tuning::persist_gain, nullptr},
        {"EKFVIO_PERSIST_EARLY", FLAG, &Tuning::persist_early, nullptr},
        {"EKFVIO_FRAME_OUTPUTS", FLAG, &Tuning::frame_outputs, nullptr},
        {"EKFVIO_EARLY_OUTPUTS", FLAG, &Tuning::early_outputs, nullptr},
        {"EKFVIO_GEMM_ORDER2D", FLAG, &Tuning::gemm_order2d, nullptr},
        {"EKFVIO_LIN_OVERLAP", FLAG, &Tuning::lin_overlap, nullptr},
        {"EKFVIO_SYM_JOSEPH", FLAG, &Tuning::sym_joseph, nullptr},
        {"EKFVIO_FUSE_LINEARIZE", FLAG, &Tuning::fuse_linearize, nullptr},
    };
    Tuning t;
    for (const Entry& k : table) {
        const char* e = getenv(k.name);
        if (!e) continue;
        if (k.kind == FLAG) t.*k.i = atoi(e) ? 1 : 0;
        else if (k.kind == RAW) t.*k.i = atoi(e);
        else if (atof(e) > 0) {
            if (k.kind == WAIT_MS) t.*k.i = (int)std::min(2.0e9, 1e5 * atof(e));
            else t.*k.d = atof(e);
        }
    }
    return t;
}

// ---- the persistent sweep's flags (chol_persist.inc): laid out HERE, once, for the allocation, the planner, the launchers and the GEMM epilogue ----
#ifdef __HIPCC__
#define PLAN_HD __host__ __device__ __forceinline__  // (inlined: a call would take the address of the kernel's by-value arguments and send them to scratch)
#else
#define PLAN_HD inline
#endif
// The flags in ekfvio_filter::sweep_sync, in words: ready[mb], fin[rows x mb], pan[rows x mb] (panel blocks of the X / identity rows, for the
// gain tiles formed inside the launch), one spare word, the abort word.  Two extents are zeroed, as found: the update's last GEMM zeroes
// zero_words(), which stops short of the abort word; gather_potrf_kernel and the launchers' memsets zero words(), which includes it.
struct PersistFlags {
    int mb, rows;  // block columns, row blocks of [A; X; I]
    PersistFlags(int m_pad, int n_pad) : mb(m_pad / EKF_TILE), rows(2 * (m_pad / EKF_TILE) + n_pad / EKF_TILE) {}
    int ready() const { return 0; }
    int fin() const { return mb; }
    int pan() const { return fin() + rows * mb; }
    int abort_word() const { return pan() + rows * mb + 1; }
    int zero_words() const { return abort_word(); }
    size_t words() const { return ((size_t)abort_word() + 1 + 3) & ~(size_t)3; }  // a multiple of 16 bytes
};
inline size_t persist_flag_words(int m_pad, int n_pad) { return PersistFlags(m_pad, n_pad).words(); }
inline int persist_zero_words(int m_pad, int n_pad) { return PersistFlags(m_pad, n_pad).zero_words(); }
// Flags ONE look of a waiting wavefront can carry: a lane each, lane 63 the abort word (chol_persist.inc, persist_poll).  A gain tile of the T2
// flow looks at its two panel blocks and at one flag per X row block its measurement rows span -- at most nX + 2 (gain_tile2, column_flags); for
// the last block column at ready[mb-1], its two finished tiles and one finished tile per such row block -- at most nX + 3 (last_flags).
#define PERSIST_POLL_FLAGS 63

// ---- the sizes a capacity implies ----------------------------------------------------------------------------------------------
struct FilterDims {
    int n_cap;   // 22 + 3*max_features
    int ldp;     // leading dimension of every n-row matrix (multiple of 64); one spare row/column: the K*y column of the Joseph-1 GEMM
    int m_cap;   // 2*max_features rounded up to 64; leading dimension of S/L
    int ld_aug;  // m_cap + ldp + m_cap
    size_t sweep_sync_words;  // flags of the persistent sweeps (PersistFlags; >= 1024: the test hooks sweep matrices that are not the filter's)
};
inline FilterDims filter_dims(int max_features) {
    FilterDims d;
    d.n_cap = EKF_BASE + 3 * max_features;
    d.ldp = round_up(d.n_cap + 1, 64);
    d.m_cap = round_up(2 * max_features > 0 ? 2 * max_features : 1, 64);
    d.ld_aug = d.m_cap + d.ldp + d.m_cap;
    // (as allocated so far: the layout of the largest sweep with one row block more, and seven words)
    d.sweep_sync_words = std::max((size_t)1024, (size_t)PersistFlags(d.m_cap, d.ldp + EKF_TILE).abort_word() + 7);
    return d;
}

// What a plan may depend on besides the Tuning and the row count -- and nothing else (common.h, plan_shape fills it from a handle).
struct PlanShape {
    int num_cus = 0;              // compute units of the handle's device
    int ldp = 0;                  // FilterDims::ldp
    size_t sweep_sync_words = 0;  // FilterDims::sweep_sync_words
    int N = 0, n = EKF_BASE;      // landmarks in the state, and its dimension 22 + 3 N
    bool dense_predict = false;   // cfg.predict_mode == EKFVIO_PREDICT_DENSE
    bool sole_handle = true;      // the only live handle on its device in this process (api.hip, live_handles_on: evaluated per plan)
    bool latched_off = false;     // an aborted persistent sweep has retired the persistent launch for now (api.hip, sweep_abort_latch)
};

// ---- the launch of ONE GEMM, C[MxN] = beta Cin + alpha A op(B): decided HERE, executed by launch_gemm (gemm.hip) ---------------------
// The tile height of A * op(B): 32 / 48 / 64 = gemm16_kernel at the smallest height whose grid is still a single wave of workgroups
// (latency regime; only A * B^T with K a multiple of 64), 0 = the 64 x 64 kernel (throughput regime).
inline int gemm_tiles(int bm, int M, int N) { return ((M + bm - 1) / bm) * ((N + 63) / 64); }
inline int gemm_tile_height(int cus, int M, int N, int K, bool transB) {
    if (cus <= 0) cus = 256;
    if (!transB || K % 64 != 0) return 0;
    for (int bm : {32, 48, 64})
        if (gemm_tiles(bm, M, N) <= cus) return bm;
    return 0;
}
// true where A * B^T runs on the 64 x 64 kernel (more 64-row tiles than compute units): the regime in which GemmShape::sym is heeded
inline bool gemm_throughput_regime(int cus, int M, int N, int K) { return gemm_tile_height(cus, M, N, K, true) == 0; }
// What a GEMM does besides the product (GemmEpi::mode in common.h; the kernels' EPI template argument, so the values are fixed)
enum GemmEpiMode { EPI_NONE = 0,
                   EPI_JOSEPH1 = 1,        // T = Sigma - K (H Sigma), the first Joseph GEMM: also G = K R - T[:, idx]; output column n receives K y
                   EPI_MEAN = 2,           // Sigma' = T + G K^T, the second Joseph GEMM: one more workgroup finishes the mean from column n of P
                   EPI_MEAN_PARTIAL = 3 }; // Sigma' = T2 + K G'^T, the one GEMM of the T2 and Schur tails: the same with K y as per-block partial sums
struct GemmShape {
    int M = 0, N = 0, K = 0;
    bool transB = false, lowerB = false;  // lowerB: B is lower triangular, the contraction starts at the tile's column
    int epi = EPI_NONE;
    bool mean = false;   // there is a mean to finish (GemmEpi::n > 0; the scratch launches of the profiler have none)
    int lin_blocks = 0;  // asked for: workgroups that linearise for the next process(dt) (UpdatePlan::lin_blocks)
    bool sym = false;    // asked for: the result is symmetric, its lower triangle's tiles may be formed alone and mirrored
    int variant = 0;     // test hooks only: 0 = by shape, 1 / 2 = the 64 x 64 kernel with 256 / 512 threads, 32 / 48 / 64 = gemm16_kernel with that
                         // tile height, + 100 = with one wavefront per SIMD
};
struct GemmPlan {
    bool k16 = false;            // gemm16_kernel<bm, wps, epi>; false: gemm_f32_mfma_kernel<transB, groups, epi>
    int bm = 64, wps = 2, groups = 1;
    int tiles_x = 0, tiles_y = 0;  // tiles of bm x 64 over C
    int tiles = 0;               // ... that the launch forms: tiles_x * tiles_y, or the lower triangle's with sym
    int grid_x = 0, grid_y = 1;
    bool mean_wg = false;        // gemm16_kernel: one workgroup behind the tiles' finishes the mean (gemm16_finish_mean)
    int lin_blocks = 0;          // ... and this many behind it linearise: what was asked for where it fits one wave of workgroups, else 0
    int mean_keep = 0;           // ... in which case the mean is left to them (GemmEpi::mean_keep)
    int sym = 0, sym_w = 1;      // 64 x 64 kernel: sym as heeded, in strips of sym_w tile columns
    int order2d = 0;             // 64 x 64 kernel: each XCD's run of tiles is a compact 2-D patch
    int threads() const { return 256 * (k16 ? wps : groups); }
};
inline GemmPlan plan_gemm(const Tuning& t, int cus, const GemmShape& s) {
    GemmPlan p;
    if (cus <= 0) cus = 256;
    int v = s.variant;
    if (v >= 32 && (!s.transB || s.K % 64 != 0)) v = 1;  // gemm16_kernel is A * B^T over whole 64-deep K-tiles
    if (v >= 32 && v % 100 != 32 && v % 100 != 48 && v % 100 != 64) v = 0;
    if (v == 0) v = std::max(1, gemm_tile_height(cus, s.M, s.N, s.K, s.transB));
    p.tiles_y = (s.N + 63) / 64;
    if (v >= 32) {
        p.k16 = true, p.bm = v % 100;
        p.wps = (v >= 100 && s.epi == EPI_NONE) ? 1 : 2;  // (one wavefront per SIMD: micro-benchmark only)
        p.tiles_x = (s.M + p.bm - 1) / p.bm;
        p.tiles = p.tiles_x * p.tiles_y;
        p.mean_wg = (s.epi == EPI_MEAN || s.epi == EPI_MEAN_PARTIAL) && s.mean;
        // the ONE fit test of the riding linearisation (plan_update asks it through this function): tiles, mean and linearising workgroups are one wave
        if (s.epi == EPI_MEAN_PARTIAL && s.mean && p.tiles + 1 + s.lin_blocks <= cus) p.lin_blocks = s.lin_blocks;
        p.mean_keep = p.lin_blocks > 0 ? 1 : 0;
        p.grid_x = p.tiles + (p.mean_wg ? 1 : 0) + p.lin_blocks;
        return p;
    }
    p.bm = 64, p.wps = 1;
    p.groups = (v == 2 && s.epi == EPI_NONE) ? 2 : 1;
    p.tiles_x = (s.M + 63) / 64;
    p.sym = (s.sym && t.sym_joseph && s.epi == EPI_MEAN && s.M == s.N && s.transB) ? 1 : 0;
    if (p.sym) {
        // strips of ceil(tn / 8) tile columns, as order2d's: measured at tn = 49 (FETCH_SIZE x 2 per launch, scripts/sym_w_sweep.sh) row by row 572 MB,
        // strips of 12 / 7 / 4 / 3 columns 296 / 258 / 277 / 312 MB, the launch's duration the same within 0.5 % (it is MFMA-bound)
        p.sym_w = (p.tiles_x + 7) >> 3;
        p.tiles = p.grid_x = p.tiles_x * (p.tiles_x + 1) / 2;  // a 1-D grid over the lower triangle's tiles
    } else {
        p.grid_x = p.tiles_x, p.grid_y = p.tiles_y;
        p.tiles = p.tiles_x * p.tiles_y;
    }
    // throughput regime (several tiles per compute unit and a full contraction per tile): compact 2-D patches per XCD.  Not for the
    // triangular-aware gain GEMM: its tiles' work falls with the tile column, and strips of columns would load the XCDs unevenly.
    p.order2d = (!p.sym && t.gemm_order2d && !s.lowerB && p.tiles >= 2 * cus) ? 1 : 0;
    return p;
}
// EXECUTED flops of a planned GEMM: the mirrored form multiplies for the lower triangle's 64 x 64 tiles only
inline double gemm_executed_flops(const GemmShape& s, const GemmPlan& p) {
    return p.sym ? 2.0 * 64.0 * 64.0 * s.K * p.tiles : 2.0 * s.M * (double)s.N * s.K;
}

// ---- process(dt)'s launches: decided HERE, executed by launch_predict (ekf_kernels.hip) ---------------------------------------------
#define PREDICT_PT 16  // landmarks per tile side of predict_fused_kernel (landmark x landmark tiles)
#define PREDICT_PC 3   // landmarks per base-row / base-column workgroup (3 * PREDICT_PC <= 64)
struct PredictPlan {
    bool dense = false;         // F formed densely, two GEMMs and add_noise_flush_kernel; else predict_fused_kernel
    bool pre = false;           // the previous update's last GEMM has linearised for this step (GemmEpi::lin_blocks): nothing linearises
    bool lin_inside = false;    // predict_fused_kernel<true> forms the Jacobian blocks itself
    bool lin_in_front = false;  // a linearize_kernel launch in front
    int ts = 0, chunks = 0;     // predict_fused_kernel: tiles per side, base-row / base-column workgroups
    // the measurement bookkeeping rides in predict_fused_kernel as one more workgroup (else in the linearize_kernel launch in front)
    bool book_rides() const { return lin_inside || pre; }
    int grid(bool bookkeeping) const { return ts * ts + 1 + 2 * chunks + (bookkeeping && book_rides() ? 1 : 0); }
};
// prelinearized: the previous update's last GEMM linearised for this step (UpdateResult::linearised_next; only inside a captured graph)
inline PredictPlan plan_predict(const Tuning& t, const PlanShape& s, bool prelinearized) {
    PredictPlan p;
    p.dense = s.dense_predict;
    p.pre = prelinearized && !p.dense;
    p.ts = (s.N + PREDICT_PT - 1) / PREDICT_PT, p.chunks = (s.N + PREDICT_PC - 1) / PREDICT_PC;
    // inside while the landmark tiles are a few rounds of workgroups: with thousands of tiles (N = 1024) the Jacobian blocks formed
    // 2 * 64 times over cost more than the launch they save
    p.lin_inside = !p.pre && !p.dense && t.fuse_linearize && p.ts * p.ts <= 4 * s.num_cus;
    p.lin_in_front = !p.lin_inside && !p.pre;
    return p;
}

// The gather's element workgroups (gather_body.inc): gx per GC*GCI measurement columns; the Wt tiles come behind them
inline int gather_gx(int ldp, int m_pad) { return (std::max(ldp, m_pad) + 255) / 256; }
inline int gather_element_wgs(int ldp, int m_pad) { return gather_gx(ldp, m_pad) * ((m_pad + GC * GCI - 1) / (GC * GCI)); }

// ---- the flow of ONE update ----------------------------------------------------------------------------------------------------
enum SweepKind { SWEEP_NONE,           // no measurement
                 SWEEP_SCHUR,          // one launch per block step, T2 (in place in f->P) and K (f->Km) as Schur tiles of the sweep (EKFVIO_SCHUR=1)
                 SWEEP_PERSIST_FUSED,  // gather + first diagonal tile + persistent sweep in ONE launch (launch_persist_fused)
                 SWEEP_PERSIST,        // the persistent launch behind a front of its own
                 SWEEP_STEP,           // one launch per block step
                 SWEEP_SPLIT, SWEEP_SPLIT_LA };  // m_pad >= 64 * EKF_SWEEP_SPLIT_MB: panel blocks solved once; _LA: as look-ahead tile tasks (chol_step_la.inc)
enum GainBy { GAIN_SWEEP, GAIN_TILES, GAIN2_T2_TILES, GAIN_GEMM, GAIN_SCHUR };  // the sweep itself / gain_tiles_kernel / gain2_t2_tiles_kernel / launch_gemm / Schur tiles + joseph_g_kernel
enum UpdateTail { TAIL_NONE, TAIL_SCHUR, TAIL_T2, TAIL_JOSEPH };  // ONE GEMM from the Schur tiles' T2 in f->P / ONE GEMM from t2_buffer / the two Joseph GEMMs
struct UpdatePlan {
    int m = 0, m_pad = 64, n_pad = 0;  // m: 2N with m_on_device (sizes the launches; the kernels read the true count from f->info[2])
    bool m_on_device = false, recoverable = true;  // (UpdateInputs)
    SweepKind sweep = SWEEP_NONE;
    bool fused_gather = false;  // the gather and the first diagonal tile's factorisation share a launch (gather_potrf_kernel)
    bool with_wt = false;       // the gather also transposes (H Sigma)^T into Wt (only the first Joseph GEMM reads it)
    GainBy gain = GAIN_GEMM;
    UpdateTail tail = TAIL_NONE;
    int t2_skip = -1;           // PersistGrid::t2_skip (>= 0: the shape takes the T2 flow)
    bool t2_by_sweep = false, compact = false;  // PersistArgs::t2, GRID_COMPACT
    int lin_blocks = 0;         // > 0: the last GEMM linearises for the next process(dt) in that many extra workgroups (GemmEpi::lin_blocks)
    // chol_persist_kernel runs: its abort word goes into the GEMM epilogues, the last GEMM zeroes its flags for the next update, and in
    // front gather_potrf_kernel zeroes them (fused_gather) or a memset does unless they are clean (ekfvio_filter::sweep_flags_clean)
    bool persistent() const { return sweep == SWEEP_PERSIST_FUSED || sweep == SWEEP_PERSIST; }
};

// ---- the persistent sweep's grid: chol_persist_kernel's workgroups by block index, described HERE for the planner, the launchers and the kernel ----
//   block 0              the chain
//   lead workgroups tb   (fused kinds) mb * lead_rows, (ib, cb) = (tb / mb, tb % mb).  GRID_FUSED: transposes tile tb of (H Sigma)^T.  Where the launch forms
//                        the gain (PersistArgs::gain) and ib < nX: tile (ib, cb) of the gain; otherwise it leaves.  GRID_COMPACT: (0, mb-1) and (1, mb-1) --
//                        gain tiles with one product to form, at the very end -- first gather the chain's step-0 tiles (1,0), (1,1): ROLE_LEAD_GATHER0
//   step-0 gatherers cb  (GRID_FUSED only) two: tile (1, cb)
//   owners h             of tile (i, j), block column by block column (the tiles the chain asks for first are dispatched first): in column j = 1 .. mb-1
//                        the rows j .. mb-1 of A (without (1,1): the chain's from the start), the nX row blocks of X, and the identity row blocks 0 .. j
//                        (GRID_COMPACT: 0 .. j-1; tile (idb0 + j, j) is the identity and nobody's)
// An owner's panel sources (i,k), (j,k), k < j, lie in earlier block columns: their owners have LOWER block indices (persist_shape's dispatch-order
// argument).  tests/test_persist_grid_cpu.py holds role() to this description for every block of every planned shape.
enum PersistGridKind { GRID_PLAIN,      // the sweep behind a front of its own (launch_chol_sweep)
                       GRID_FUSED,      // gather + first diagonal tile + sweep in one launch (launch_persist_fused)
                       GRID_COMPACT };  // ... that fits the compute units with nobody waiting for one (the T2 flow)
enum PersistRoleKind { ROLE_CHAIN, ROLE_LEAD, ROLE_LEAD_GATHER0, ROLE_GATHER0, ROLE_OWNER, ROLE_NONE };
struct PersistRole {
    int kind, a, b, n;  // lead: (a, b) = (ib, cb); a step-0 gatherer of either kind: tile (1, a); owner: tile (a, b).  n: its number among its role's (tb, cb, h)
};
// tile pairs (ta, tb), ta >= tb, of the nX x nX tiles of T2 (chol_persist.inc, t2_tile), and pair p of them
PLAN_HD constexpr int t2_pairs(int nX) { return nX * (nX + 1) / 2; }
PLAN_HD void t2_pair(int p, int& ta, int& tb) {
    ta = 0;
    while ((ta + 1) * (ta + 2) / 2 <= p) ta++;
    tb = p - ta * (ta + 1) / 2;
}
struct PersistGrid {
    int kind = GRID_PLAIN;
    int mb = 0, nX = 0;  // block columns, row blocks of X
    int lead_rows = 0;   // ldp / 64: tile rows of the lead workgroups (fused kinds)
    int t2_skip = 0;     // the first t2_skip owners leave instead of adopting a tile pair of T2 (UpdatePlan::t2_skip)
    PLAN_HD bool fused() const { return kind != GRID_PLAIN; }
    PLAN_HD bool compact() const { return kind == GRID_COMPACT; }
    PLAN_HD int lead() const { return fused() ? mb * lead_rows : 0; }
    PLAN_HD int gatherers() const { return kind == GRID_FUSED ? 2 : 0; }
    PLAN_HD int a_rows(int j) const { return mb - j - (j == 1 ? 1 : 0); }
    PLAN_HD int column_owners(int j) const { return a_rows(j) + nX + (j + 1 - (compact() ? 1 : 0)); }
    PLAN_HD int owners() const {
        int h = 0;
        for (int j = 1; j < mb; j++) h += column_owners(j);
        return h;
    }
    PLAN_HD int owner_block(int h) const { return 1 + lead() + gatherers() + h; }
    PLAN_HD int total() const { return owner_block(owners()); }
    // the tile pair of T2 owner h adopts once its tile is finished, -1: none
    PLAN_HD int t2_pair_of(int h) const { return (h >= t2_skip && h - t2_skip < t2_pairs(nX)) ? h - t2_skip : -1; }
    PLAN_HD PersistRole role(int block) const {  // (chol_persist_kernel sits at its register limit: compare its resource usage after touching this)
        if (block == 0) return {ROLE_CHAIN, 0, 0, 0};
        int h = block - 1;
        if (h < lead()) {
            const int ib = h / mb, cb = h % mb;
            if (compact() && cb == mb - 1 && ib < 2) return {ROLE_LEAD_GATHER0, ib, cb, h};
            return {ROLE_LEAD, ib, cb, h};
        }
        h -= lead();
        if (h < gatherers()) return {ROLE_GATHER0, h, 0, h};
        h -= gatherers();
        const int n = h;
        for (int j = 1; j < mb; j++) {
            const int nA = a_rows(j);
            if (h < column_owners(j)) {
                const int i = h < nA ? j + h + (j == 1 ? 1 : 0) : h < nA + nX ? mb + (h - nA) : mb + nX + (h - nA - nX);
                return {ROLE_OWNER, i, j, n};
            }
            h -= column_owners(j);
        }
        return {ROLE_NONE, 0, 0, n};  // (past total(): never launched)
    }
};
// The shapes the persistent launch takes: 3 .. EKF_SWEEP_SPLIT_MB - 1 block columns.  Up to round 3: chain + owners co-resident
// (PersistGrid::total() <= compute units).  Round 4: up to EKF_PERSIST_OVERSUB x that.  An owner waits only for workgroups with a LOWER block
// index (PersistGrid), so with workgroups dispatched in index order -- what the hardware does, though HIP does not promise it -- the resident ones can always
// finish, and the later columns' owners take over their compute units and catch up (their flags are all up: ~10 k cycles per step
// against the chain's ~15.5 k).  N = 400 (params/fast_with_insight.yaml: 13 block columns, 407 owners) runs the sweep in one launch
// this way.  Should the order ever not hold, the bounded waits end the launch and the update is run again per step (EKFVIO_EABORTED).
// Measured (profiles/r04_oversubscribed_persistent_sweep.txt): bit-identical, the sweep itself 155.7 -> 121.2 us at N = 400, but the gain
// kernel behind it then runs 2x longer on operands the persistent launch has left in other XCDs' L2s; +2.9 % per step in all.  Off by
// default (1); EKFVIO_PERSIST_OVERSUB=2 turns it on, tests/test_gpu_parity.py exercises it.
#ifndef EKF_PERSIST_OVERSUB
#define EKF_PERSIST_OVERSUB 1
#endif
inline bool persist_shape(const Tuning& t, const PlanShape& s, int m_pad, int n_pad) {
    const int mb = m_pad / EKF_TILE;
    const int over = t.persist_oversub > 0 ? t.persist_oversub : EKF_PERSIST_OVERSUB;
    return mb >= 3 && mb < EKF_SWEEP_SPLIT_MB && PersistGrid{GRID_PLAIN, mb, n_pad / EKF_TILE}.total() <= (over > 1 ? over : 1) * s.num_cus &&
           persist_flag_words(m_pad, n_pad) <= s.sweep_sync_words;
}
// ... and of those, the shapes whose gain is formed inside the fused launch: (nearly) every workgroup of that launch finds a compute unit
// at once (the transposing / gain workgroups hold theirs to the end).  Behind every other sweep of such a shape gain_tiles_kernel runs
// the same arithmetic; all other shapes take the gain GEMM, whichever sweep ran.
inline bool gain_in_sweep_shape(const Tuning& t, const PlanShape& s, int m_pad, int n_pad) {
    const int mb = m_pad / EKF_TILE;
    return persist_shape(t, s, m_pad, n_pad) && PersistGrid{GRID_FUSED, mb, n_pad / EKF_TILE, s.ldp / 64}.total() <= s.num_cus + 8;
}
// ... and of those, the shapes whose T2 = Sigma (I - K H)^T is formed by freed owners inside the launch (round 6, chol_persist.inc, t2_tile): there
// must be an owner per tile pair once enough of the first owners have LEFT for every workgroup of the launch to find a compute unit (the two
// step-0 gatherers and the gain workgroups beyond the state's row blocks leave at once).  Returns the number of owners that leave (PersistGrid::t2_skip),
// -1 where the flow does not apply.  The flow is a property of the SHAPE, not of the sweep that runs: behind a per-step sweep of such a shape
// gain2_t2_tiles_kernel forms the same T2, so a sequence's bits do not depend on what else the device runs.
inline int t2_skip_owners(const Tuning& t, const PlanShape& s, int m_pad, int n_pad) {
    if (!t.t2_flow || !t.persist_gain || t.schur || !gain_in_sweep_shape(t, s, m_pad, n_pad)) return -1;
    const PersistGrid g{GRID_COMPACT, m_pad / EKF_TILE, n_pad / EKF_TILE, s.ldp / 64};
    if (g.total() > s.num_cus) return -1;  // the compact launch: every workgroup has its compute unit from the start
    if (g.nX + 3 > PERSIST_POLL_FLAGS) return -1;  // the gain tiles' waits: one flag per X row block in ONE look (the last block column's: and three more)
                                                   // (out of reach today: t2_pairs(nX) <= owners() holds nX to 38 below EKF_SWEEP_SPLIT_MB block columns, to 22 on 256 compute units)
    return (t2_pairs(g.nX) <= g.owners()) ? 0 : -1;
}
// The grid of the persistent launch a plan selects (launch_persist_fused / launch_chol_sweep); ldp: FilterDims::ldp
inline PersistGrid persist_grid(const UpdatePlan& p, int ldp) {
    return {p.sweep != SWEEP_PERSIST_FUSED ? GRID_PLAIN : p.compact ? GRID_COMPACT : GRID_FUSED, p.m_pad / EKF_TILE, p.n_pad / EKF_TILE, ldp / 64, p.t2_skip};
}
// Which sweep runs.  filter_update: the filter's own matrices (Schur tiles and the fused front are possible); else another caller's [A; X; I].
inline SweepKind choose_sweep(const Tuning& t, const PlanShape& s, int m_pad, int n_pad, bool filter_update) {
    const int mb = m_pad / EKF_TILE;
    // (EKFVIO_SCHUR=1 takes precedence over the persistent launch, for every sweep of the handle; not in the split sweep)
    const bool schur_shape = t.schur && mb < EKF_SWEEP_SPLIT_MB;
    if (schur_shape && filter_update) return SWEEP_SCHUR;
    // (only for a device's sole handle: two persistent launches in flight together could starve each other of compute units)
    if (t.persist_sweep && !s.latched_off && !schur_shape && s.sole_handle && persist_shape(t, s, m_pad, n_pad))
        // round 4: where the persistent sweep applies, the gather and the first tile are part of ITS launch (launch_persist_fused)
        return (filter_update && t.fuse_sweep && t.fuse_gather) ? SWEEP_PERSIST_FUSED : SWEEP_PERSIST;
    // many tiles per step: panel blocks once per step in a launch of their own instead of twice per tile
    return mb < EKF_SWEEP_SPLIT_MB ? SWEEP_STEP : t.sweep_la ? SWEEP_SPLIT_LA : SWEEP_SPLIT;
}
// a shape the persistent launch forms the gain for when it runs: behind any other sweep the tile kernel whose arithmetic that launch's
// in-sweep gain shares (chol_persist.inc, gain_tile), so that a sequence gives the same bits whichever sweep its updates take (eight
// handles on one GPU against each one's solo run, tests/test_gpu_shapes.py)
inline bool gain_tiles_shape(const Tuning& t, const PlanShape& s, int m_pad, int n_pad) { return t.persist_gain && gain_in_sweep_shape(t, s, m_pad, n_pad); }

// A sweep over matrices that are not the filter's (ekfvio_test_cholesky_solve): the same choice of sweep for [A; X; I] with m_pad
// columns and n_pad rows of X, without the update's front, Schur tiles and tail; the gain by gain_tiles_kernel or the gain GEMM
inline UpdatePlan plan_raw_sweep(const Tuning& t, const PlanShape& s, int m_pad, int n_pad) {
    UpdatePlan p;
    p.m = p.m_pad = m_pad, p.n_pad = n_pad;
    p.sweep = choose_sweep(t, s, m_pad, n_pad, false);
    p.gain = gain_tiles_shape(t, s, m_pad, n_pad) ? GAIN_TILES : GAIN_GEMM;
    return p;
}

// The one GEMM of the T2 and Schur tails, Sigma' = T2 + K G'^T over n x n x m_pad, as the update itself launches it: the mean is finished from the
// partial sums of K y, and lin_blocks workgroups are asked to linearise (plan_update asks plan_gemm whether they fit; launch_update launches this shape)
inline GemmShape tail_gemm_shape(int n, int m_pad, int lin_blocks) {
    GemmShape g;
    g.M = g.N = n, g.K = m_pad, g.transB = true, g.epi = EPI_MEAN_PARTIAL, g.mean = true, g.lin_blocks = lin_blocks;
    return g;
}
// m_on_device: the host does not know the row count; next_dt >= 0: the next process(dt)'s dt of a device-resident run (UpdateInputs)
inline UpdatePlan plan_update(const Tuning& t, const PlanShape& s, int m, bool m_on_device = false, float next_dt = -1.f, bool recoverable = true) {
    UpdatePlan p;
    if (m_on_device) m = 2 * s.N;  // upper bound: sizes the launches; the kernels read the true count from f->info[2]
    const int n = s.n, ld = s.ldp, m_pad = round_up(m > 0 ? m : 1, EKF_TILE), n_pad = round_up(n, EKF_TILE);
    p.m = m, p.m_pad = m_pad, p.n_pad = n_pad, p.m_on_device = m_on_device, p.recoverable = recoverable;
    if (m <= 0) return p;
    p.sweep = choose_sweep(t, s, m_pad, n_pad, true);
    // T = Sigma - X A^-1 X^T and K = X A^-1 as Schur tiles of the sweep (no gain GEMM, no first Joseph GEMM, no (H Sigma)^T)
    const bool schur = p.sweep == SWEEP_SCHUR, fused = p.sweep == SWEEP_PERSIST_FUSED;
    p.with_wt = !schur;
    // The gather and the first diagonal tile's factorisation share a launch while that launch is a single round of
    // workgroups at one per compute unit (gather_potrf_kernel); beyond that (N = 1024: thousands of gather
    // workgroups) the gather wants several workgroups per compute unit and the two stay separate.
    if (t.fuse_gather && !fused)
        p.fused_gather = 1 + gather_element_wgs(ld, m_pad) + (schur ? 0 : (m_pad / 64) * (ld / 64)) <= s.num_cus;
    if (schur) return p.gain = GAIN_SCHUR, p.tail = TAIL_SCHUR, p;
    p.t2_skip = t2_skip_owners(t, s, m_pad, n_pad);
    if (p.t2_skip < 0) {
        // the transposing workgroups of the fused launch stay and form the gain while the sweep runs, as long as (nearly) every workgroup of the
        // launch finds a compute unit at once: they hold theirs to the end
        p.gain = !gain_tiles_shape(t, s, m_pad, n_pad) ? GAIN_GEMM : fused ? GAIN_SWEEP : GAIN_TILES;
        return p.tail = TAIL_JOSEPH, p;
    }
    p.tail = TAIL_T2;
    p.t2_by_sweep = p.compact = fused;
    p.gain = fused ? GAIN_SWEEP : GAIN2_T2_TILES;
    // a device-resident run (capture_steps): the next process(dt)'s linearisation and mean propagation ride in the one GEMM's launch, in workgroups
    // of their own behind the tiles' (K y is final: the gain tiles' partial sums); launch_predict then only propagates Sigma
    const int lin_blocks = (s.N + LIN_LM - 1) / LIN_LM + 1;
    if (next_dt >= 0.f && t.lin_overlap && !s.dense_predict && t.fuse_linearize)
        p.lin_blocks = plan_gemm(t, s.num_cus, tail_gemm_shape(n, m_pad, lin_blocks)).lin_blocks;  // (all of them or none: they must fit the GEMM's one wave)
    return p;
}

// ---- the device-resident run: decided HERE, executed by ekfvio_run_uploaded (api.hip) ---------------------------------------------------
// Steps per captured graph: even (the mean / covariance ping-pong is back in its starting orientation) and large enough to amortise the
// ~8 us a hipGraphLaunch costs between replays
#ifndef EKF_GRAPH_STEPS
#define EKF_GRAPH_STEPS 8
#endif
#define EKF_GRAPH_STEPS_BIG 32  // second, longer graph for runs of at least two of them (+0.6 % steps/s at N=256)
#define EKF_GRAPH_STEPS_PAIR 2  // tails and short runs
// ... of which the long one exists only for sequences long enough to make runs of that length plausible
#define EKF_GRAPH_BIG_FROM_FRAMES (2 * EKF_GRAPH_STEPS_BIG)
#define RUN_GRAPHS 3
// The graphs of a run, longest first: the order of the greedy cut, and of the cache's table (common.h, GraphCache)
inline int run_graph_steps(int g) { return g == 0 ? EKF_GRAPH_STEPS_BIG : g == 1 ? EKF_GRAPH_STEPS : EKF_GRAPH_STEPS_PAIR; }
inline bool run_graph_used(int g, int frames) { return g != 0 || frames >= EKF_GRAPH_BIG_FROM_FRAMES; }
struct RunPlan {
    bool graphs = false;  // the steps are replays of captured graphs (bookkeeping driven by the device-side frame counter); else every step is eager
    int m = 0;            // with graphs: the one launch geometry of the sequence
    int replays[RUN_GRAPHS] = {0, 0, 0};  // of the graph of run_graph_steps(g) steps
    int eager = 0;        // with graphs: the odd last step, counter-driven like the replays; without: all `count` steps, each with its own frame's rows
};
// The launch geometry of uploaded frame i: its measurement rows as the host counted them; on a gated handle 2N for every frame in which any
// landmark passed (the count is then on the device: launch_update)
inline int run_geometry(const int* seq_m, int i, int N, bool gated) { return gated && seq_m[i] > 0 ? 2 * N : seq_m[i]; }
// ekfvio_run_uploaded(first, count, dt) over `frames` uploaded frames of seq_m[i] rows.  Graphs need one launch geometry for every frame and
// profiling off; a single step runs eager; count == 0 only prepares: the graphs are captured, nothing runs (callers that time a run call
// this first)
inline RunPlan plan_run(const int* seq_m, int frames, int N, bool gated, bool profiling, int count) {
    RunPlan p;
    p.eager = count;
    p.graphs = !profiling && (count >= 2 || count == 0);
    for (int i = 0; p.graphs && i < frames; i++) p.graphs = run_geometry(seq_m, i, N, gated) == run_geometry(seq_m, 0, N, gated);
    if (!p.graphs) return p;
    p.m = run_geometry(seq_m, 0, N, gated);
    for (int g = 0; g < RUN_GRAPHS; g++)
        if (run_graph_used(g, frames)) p.replays[g] = p.eager / run_graph_steps(g), p.eager %= run_graph_steps(g);
    return p;
}
#endif  // EKFVIO_PLAN_H_
