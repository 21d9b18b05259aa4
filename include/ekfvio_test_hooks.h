/* ekfvio_test_hooks.h -- raw kernels, in-kernel stamps and fault injection for the tests and the profiling scripts.
 *
 * NOT part of the drop-in boundary (include/ekfvio.h) and NOT in the product library: these entry points exist only in
 * libekfvio_hip_hooks.so, the same sources compiled with -DEKFVIO_TEST_HOOKS (ekf_vio_amd/_build.py builds both; the
 * Python mirror loads the hooks build only for TightlyCoupledEKF(..., hooks=True)).  libekfvio_hip.so exports no
 * ekfvio_test_* symbol (tests/test_abi_cpu.py).
 */
#ifndef EKFVIO_TEST_HOOKS_H_
#define EKFVIO_TEST_HOOKS_H_
#include "ekfvio.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Test hook: the same level WITH its border as the tracker reads it: (w + 2 border) x (h + 2 border) image bytes
 * (reflect-101 border) and int16 pairs (zero border).  `border` (may be NULL) receives the border width (24). */
EKFVIO_API int ekfvio_test_klt_padded_level(ekfvio_filter* f, int32_t level, int32_t* border, uint8_t* img, int16_t* deriv);
/* Test hook: the blurred level 0 (w*h bytes) the last FAST run saw; cfg.fast_blur_sigma must be non-zero. */
EKFVIO_API int ekfvio_test_blurred_level0(ekfvio_filter* f, uint8_t* out);
/* Raw kernels for unit tests (column-major, device copies made internally).  variant: 0 = the
 * production tile choice, 1 / 2 = 64x64 tiles with 256 / 512 threads, 32 / 48 / 64 = BM x 64 tiles. */
EKFVIO_API int ekfvio_test_gemm(ekfvio_filter* f, int32_t transB, int32_t M, int32_t N, int32_t K, float alpha, const float* A,
                     int32_t lda, const float* B, int32_t ldb, float beta, float* C, int32_t ldc, int32_t variant);
/* Mean time (us) of `reps` back-to-back GEMM launches at one shape, operands resident. */
EKFVIO_API int ekfvio_test_gemm_bench(ekfvio_filter* f, int32_t transB, int32_t lowerB, int32_t M, int32_t N, int32_t K,
                           int32_t reps, int32_t variant, double* mean_us);
/* Diagnostic: s_memtime stamps of the phases of one 64x64 diagonal-block factorisation. */
EKFVIO_API int ekfvio_test_potrf_stamps(ekfvio_filter* f, int64_t stamps[80]);
EKFVIO_API int ekfvio_test_sweep_stamps(ekfvio_filter* f, int enable, int64_t stamps[1024]);
/* Fault injection for the persistent sweep: at most `spin_limit` looks per wait (0: the production limit), and workgroup
   `stall_workgroup` of the launch never raises its tile's flag (-1: none), so every wait behind it runs out. */
EKFVIO_API int ekfvio_test_sweep_fault(ekfvio_filter* f, int32_t spin_limit, int32_t stall_workgroup);
/* Arrival order of the persistent sweep's hand-offs (NOT fault injection: nothing is withheld and no wait runs out).  Owner workgroup `workgroup`
   of the launch -- numbered like stall_workgroup, mapped through PersistGrid::owner_block; -1: none -- idles `ticks` of the 100 MHz clock and then
   goes on as always.  point 0: in front of the store of its finished tile (the store behind which fin[i][j] goes up); point 1: in front of the
   store of its panel block (the store behind which pan[i][j-1] goes up).  The panel block leaves first, right behind the owner's last
   substitution, and the tile after the last product: late at point 1 an owner is late with both, late at point 0 its `pan` is up while its
   tile is not (tests/test_gpu_early_panel.py).  The idling comes BEFORE the data, not between data and flag: a consumer
   that reads without waiting for the flag finds what the previous update left there.  EKFVIO_EINVAL for another point or more than
   EKFVIO_TEST_SWEEP_DELAY_MAX_TICKS (1 ms, a third of the default 3 ms wait bound; EKFVIO_SWEEP_WAIT_MS can set a shorter one).  An owner
   has a panel block to store only where it is an operand of the gain formed inside the launch (an X or identity row block off the diagonal);
   for every other owner point 1 does nothing.  A launch that forms no gain inside solves the last block column's panel blocks in a branch
   the hook does not reach. */
#define EKFVIO_TEST_SWEEP_DELAY_MAX_TICKS 100000
EKFVIO_API int ekfvio_test_sweep_delay(ekfvio_filter* f, int32_t workgroup, int32_t point, int32_t ticks);
EKFVIO_API int ekfvio_test_cholesky_solve(ekfvio_filter* f, int32_t m, int32_t nrhs, const float* S, const float* Crhs,
                               float* L_out, float* X_out, int32_t* info);
/* The flow an update would take (csrc/plan.h, plan_update), without a handle or a device: the switches from the environment, the sizes of a
 * handle of `max_features` on a device of `num_cus` compute units holding N landmarks.  plan[12] = m, m_pad, n_pad, sweep (SweepKind),
 * fused_gather, with_wt, gain (GainBy), tail (UpdateTail), t2_skip, t2_by_sweep, compact, lin_blocks. */
EKFVIO_API int ekfvio_test_plan(int32_t num_cus, int32_t max_features, int32_t N, int32_t m, int32_t m_on_device, int32_t sole_handle,
                                int32_t latched_off, int32_t dense_predict, float next_dt, int32_t plan[12]);
/* How ONE GEMM would be launched (csrc/plan.h, plan_gemm), likewise: epi is a GemmEpiMode (0 .. 3), mean: there is a mean to finish, lin_blocks
 * and sym as asked for, variant as ekfvio_test_gemm's.  plan[18] = gemm16_kernel (0: the 64 x 64 kernel), bm, wavefronts per SIMD (gemm16_kernel),
 * groups (64 x 64 kernel), threads, tiles_x, tiles_y, tiles formed, grid x, grid y, mean workgroup, lin_blocks kept, mean_keep, sym heeded, sym_w,
 * order2d; and gemm_throughput_regime, gemm_tile_height of the shape. */
EKFVIO_API int ekfvio_test_gemm_plan(int32_t num_cus, int32_t M, int32_t N, int32_t K, int32_t transB, int32_t lowerB, int32_t epi, int32_t mean,
                                     int32_t lin_blocks, int32_t sym, int32_t variant, int32_t plan[18]);
/* How process(dt) would be launched (csrc/plan.h, plan_predict) with N landmarks.  plan[8] = dense, pre, linearises inside predict_fused_kernel,
 * linearize_kernel in front, ts, chunks, the bookkeeping rides in predict_fused_kernel, its grid (with the bookkeeping workgroup where asked). */
EKFVIO_API int ekfvio_test_predict_plan(int32_t num_cus, int32_t N, int32_t dense_predict, int32_t prelinearized, int32_t bookkeeping,
                                        int32_t plan[8]);
/* How ekfvio_run_uploaded(first, count, dt) would cut its steps (csrc/plan.h, plan_run) on a handle of N landmarks, gate and profiler on or off,
 * over `frames` uploaded frames of rows[i] measurement rows as the host counts them.  out[6] = graphs are used, their launch geometry m, replays of
 * the 32-, 8- and 2-step graph, eager steps. */
EKFVIO_API int ekfvio_test_run_plan(int32_t N, int32_t gated, int32_t profiling, int32_t frames, const int32_t* rows, int32_t count, int32_t out[6]);
/* The grid and the flag layout of the persistent sweep launch that plan selects (csrc/plan.h, PersistGrid / PersistFlags), likewise without a
 * handle or a device.  out[10] = total() (0: the planned sweep is not persistent, nothing else is filled), kind (PersistGridKind), owners,
 * the offsets of ready, fin, pan and the abort word, words(), zero_words(), FilterDims::sweep_sync_words.  roles (may be NULL; room for
 * max_blocks blocks of four words, EKFVIO_ECAPACITY if that is fewer than total()) receives per block: role (PersistRoleKind), a, b, and
 * for an owner the block owner_block() gives for its owner number (-1 for every other role). */
EKFVIO_API int ekfvio_test_persist_grid(int32_t num_cus, int32_t max_features, int32_t N, int32_t m, int32_t m_on_device, int32_t sole_handle,
                                        int32_t latched_off, int32_t dense_predict, float next_dt, int32_t* roles, int32_t max_blocks,
                                        int32_t out[10]);
/* Tile pair p of T2's (csrc/plan.h, t2_pair): pair[2] = ta, tb. */
EKFVIO_API int ekfvio_test_t2_pair(int32_t p, int32_t pair[2]);
/* What the handle's memory ledger holds (csrc/mem.h).  out[8] = device: live allocations, live bytes; pinned host memory (mapped or not):
 * live allocations, live bytes; then device: acquisitions ever, releases ever; pinned: acquisitions ever, releases ever (successful
 * acquisitions only: live = acquired - released).  f == NULL: the totals over every ledger of this copy of the library, the scratch
 * ledgers of the hooks above included. */
EKFVIO_API int ekfvio_test_mem(ekfvio_filter* f, int64_t out[8]);
/* Failure injection for the ledger: the handle's nth acquisition from now reports out-of-memory WITHOUT calling the runtime, once; 0 disarms.
 * f == NULL arms the ledger of the next ekfvio_create of this copy of the library. */
EKFVIO_API int ekfvio_test_mem_fail(ekfvio_filter* f, int32_t nth);
/* History of a handle (NOT fault injection): writes `word` into every 32-bit element of the floating-point buffers that process(dt) and the
 * update use as scratch -- Saug, Laug, Linv, Km, Wt, Gm, yres, Rm, the dense-F / T2 buffer, FA, FB, FD and mu_next -- on the handle's stream,
 * so that an update no longer finds the zero fill of a fresh handle there.  An update's result must not depend on `word`.  Left alone: the
 * state and its padding (P, P2, mu, the landmark bookkeeping), the measurement inputs, the persistent sweep's flag words and every integer
 * buffer (idx, inv_idx, Lsign, info).  No filled region is written at create and only read afterwards, so none is restored ("Who
 * owns the update's work buffers").  mu_next and mu swap roles with every process(dt): the entries of a filled mu_next from 22 + 3N on become
 * mu's padding, which nothing reads.  Call it between entry points, not inside a device-resident run. */
EKFVIO_API int ekfvio_test_fill_update_scratch(ekfvio_filter* f, uint32_t word);
/* The zero-velocity decision (include/ekfvio.h) on the device for `count` arbitrary points, arguments and results as ekfvio_zupt_decide's: the
 * points are uploaded into the tracker's own buffers (count above max_features: EKFVIO_ECAPACITY) and one workgroup runs the device function
 * every workgroup of the frame's gain kernel runs -- the same inline functions, ballots and publication into pinned host memory; the
 * reference pixel is formed as prev_px * 1 + 0, which is exact.  Overwrites the flow2 that ekfvio_get_zupt reports; waits for the stream. */
EKFVIO_API int ekfvio_test_zupt_decide(ekfvio_filter* f, const float* prev_px, const float* cur_px, const uint8_t* pass, int32_t count,
                                       float max_flow_px, int32_t min_tracks, float min_ratio, float* flow2, int32_t* n_pass, int32_t* n_still,
                                       int32_t* stationary);
/* The rectification map as the device holds it (include/ekfvio.h, ekfvio_set_distortion and ekfvio_set_camera_model): the two fixed-point
 * planes the map kernel wrote for the frame pushed last, row-major *w x *h int32 each.  sx, sy may be NULL (the size alone); cap < *w * *h:
 * EKFVIO_EINVAL; no map formed yet: EKFVIO_ESTATE.  Waits for the stream. */
EKFVIO_API int ekfvio_test_rectify_map(ekfvio_filter* f, int32_t* sx, int32_t* sy, int32_t cap, int32_t* w, int32_t* h);
/* The tracker's pixel buffers as the most recent track of the handle's landmarks (ekfvio_klt_track, ekfvio_step_image) left them: the
 * reference pixels it tracked from and the pixels it tracked to, x,y interleaved, one pair per landmark; read-only.  These are the pixels the
 * frame's zero-velocity decision reads (include/ekfvio.h).  Either pointer may be NULL; cap (in points) below the landmark count:
 * EKFVIO_EINVAL.  An entry point that uploads points of its own (ekfvio_klt_track_points, ...) overwrites them.  Waits for the stream. */
EKFVIO_API int ekfvio_test_klt_pixels(ekfvio_filter* f, float* prev_px, float* next_px, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* EKFVIO_TEST_HOOKS_H_ */
