// chol_persist.inc -- the sweep over [A; X; I] as ONE persistent launch with per-tile hand-offs (round 3).  Included inside
// chol.hip's anonymous namespace behind the tile movers, the substitution helpers and potrf64_lds.
//
// The one-launch-per-block-step sweep pays, on its sequential chain, a kernel boundary (~1.5 us) and a cold reload of
// L_kk, its inverses and two tiles (~0.9 us) per block step.  Rounds 1-2 tried a persistent launch whose helpers met at a
// counter once per block step ("every helper has finished step k-1"): that barrier among ~170 workgroups cost more than
// the boundary it replaced (92 against 88 us).  Here nothing is a grid-wide meeting:
//
//   * STATIC OWNERSHIP.  Helper workgroup h owns tile (i,j) of the trailing matrix for the whole sweep and keeps it in
//     registers: it applies steps k = 0 .. j-1 to it (each time solving the two panel blocks it needs itself, from the
//     FINAL tiles (i,k), (j,k) of block column k, exactly as chol_step_kernel's tiles do), writes the finished tile once
//     and raises fin[i][j].  A tile is read by others only when final (it is then the panel source of step j).
//   * The chain workgroup keeps L_kk and its inverses in LDS from one step to the next; per step it needs two tiles,
//     (k+1,k) final and (k+1,k+1) with steps 0 .. k-1 applied (the diagonal tile's owner stops one step early and hands
//     it over), solves, updates, factors, publishes ready[k+1].  Those two tiles' owners were released by ready[k-1], a
//     whole chain step earlier: their flags are up ~2 k cycles before the chain looks (details at the chain's code).
//   * A helper in the last block column ends with its own panel solve against L_last (what chol_panel_kernel did in a
//     launch of its own).
//
// Visibility (MI355X_MICROARCH.md, inter-workgroup visibility): everything handed over inside the launch is stored with
// agent-scope (sc1, write-through) 16-byte buffer stores; every storing wavefront waits for its stores (vmcnt) and the flag
// goes up behind that -- a helper's by one lane behind the workgroup's barrier, ready[k] by each of the chain's four
// wavefronts adding 1 for itself.  A consumer looks at its flags with ONE load instruction (a lane per flag, lane 63
// the abort word; relaxed agent-scope loads: persist_poll) and reads the data with sc1 loads only, behind a barrier or, a wavefront for
// itself, behind its own match.  Every wait is bounded: after PersistArgs::bound.wait_ticks of wall clock (3 ms; or bound.spin_limit looks, the
// fault-injection hook's bound) the abort word is raised, every wait
// falls through and info bit 1 reports it (the grid always drains); the kernels behind the sweep then leave Sigma and mu
// untouched and the host runs the update again with one launch per block step (EKFVIO_EABORTED, api.hip settle_update).  Which workgroup does what,
// the shapes whose grid is admitted and the flags' layout and zeroing: plan.h (PersistGrid, persist_shape / choose_sweep, PersistFlags).
//
// Bits: a tile receives its steps in ascending order, one subtraction of a k-ascending MFMA product per step, and the panel
// blocks are the same substitutions on the same final tiles as in chol_step_kernel: identical to the per-step sweep.

#ifndef PERSIST_POLL_SLEEP_LAZY
#define PERSIST_POLL_SLEEP_LAZY 12
#endif
#ifndef PERSIST_POLL_SLEEP
#define PERSIST_POLL_SLEEP 2  // 64-cycle units between two looks of a wavefront the chain waits for; the others: _LAZY (same-box A/B at N=256:
                               // every waiting wavefront looking back to back, the first version, costs 1.5 % of the step -- the looks load the
                               // fabric the chain reads through; 12 .. 24 units for the others and 2 .. 4 for the critical ones measure the same)
#endif

struct PollBound {
    int spin_limit, wait_ticks;
};
struct PersistArgs {
    float* S;           // augmented matrix [A; X; I], ld lds
    int lds;
    float* L;           // factor / panel blocks out, ld ldl
    int ldl;
    float* Linv;        // 16x16 inverse blocks per block column
    int mb, idb0;       // block columns; first identity row block
    int* info;
    unsigned long long* Lsign;
    int* ready;         // [mb]   4 (one per wavefront of the chain): L_kk, its inverses and Lsign[k] are in memory
    int* fin;           // [row blocks * mb] tile (i,j) is final in S
    int* abort_flag;
    long long* dbg;
    PersistGrid grid;   // which workgroup does what (plan.h); fused(): the measurement gather and the first diagonal tile are part of this launch (round 4)
    int gain;           // 1 (fused launch only): the transposing workgroups stay and form the Kalman gain K = Y L^-1 tile by tile as the panel blocks
                        // of the X rows (Y) and of the identity rows (L^-T) come out of the sweep (round 4): no gain GEMM behind the launch
    float* K;           // gain out, column-major, ld ldk
    int ldk;
    int* pan;           // [row blocks * mb] panel block (i,k), i >= mb, is in L (write-through) -- raised by whoever stores it
    int early_sources;  // 1: an owner fetches its two panel sources as soon as THEY are final, in front of its wait for ready[k] (EKFVIO_PERSIST_EARLY)
    PollBound bound;    // spin_limit: looks per wait before the sweep is given up (the fault-injection hook's bound; production: SWEEP_SPIN_LIMIT, never
                        // reached); wait_ticks: the production bound, wall-clock time in 100 MHz s_memrealtime ticks per wait, checked every 32 looks
                        // (3 ms by default where the update can be run again, 100 ms in a device-resident run: chol.hip, ekfvio_filter::sweep_wait_ticks)
    int stall_wg;       // fault injection (ekfvio_test_sweep_fault): this workgroup never raises its tile's flag; -1 = none
    int t2;             // 1 (fused launch with the gain inside, round 6): owners whose tile is finished adopt a tile pair (a,b) / (b,a) of
                        // T2 = Sigma - Y S Y^T = Sigma (I - K H)^T and subtract Y_ak S_k Y_bk^T block column by block column as the X rows' panel
                        // blocks come out of the sweep (t2_tile, grid.t2_pair_of): no first Joseph GEMM behind the launch.  With it the grid is compact
                        // (plan.h, GRID_COMPACT): whoever needs an identity row block's diagonal tile (idb0 + c, c) as a panel source writes it into LDS
                        // itself.  (Measured, profiles/r06_persistent_t2.txt: a workgroup past the 256th of a launch does not get the first compute unit
                        // that falls free on its XCC but waits for particular ones; with the owners staying for T2 that was 35 us later than before, and
                        // the gain tiles that need its tile ended the launch 12 us late.)
    const float* Sg;    // Sigma (n_pad x n_pad readable, zero padding), ld ldsg
    int ldsg;
    float* T2;          // T2 out (another buffer than Sigma: late owners may still be gathering from Sigma), ld ldt
    int ldt;
    int nstate;         // n: T2 is written as zero outside n x n
#ifdef EKFVIO_TEST_HOOKS
    int delay_wg;       // hooks build only (ekfvio_test_sweep_delay): this owner workgroup arrives late -- it waits delay_ticks of the 100 MHz clock in FRONT
    int delay_point;    // of the store of its finished tile (point 0) or of its panel block (point 1), so that a consumer that did not wait for the flag
    int delay_ticks;    // finds the previous update's contents there; -1 = none.  Nothing is withheld: the store and the flag follow as always
#endif
};

// 16-byte agent-scope (sc1, write-through) accesses for the data handed over inside the launch: buffer loads / stores
// with the sc1 bit (aux 16), which the compiler tracks like any other load (it places the waits; a load can stay in flight
// across other work).  Offsets are in floats from the buffer's base.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t persist_rsrc(const float* p, unsigned floats) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, floats * 4u, 0x00020000);
}
__device__ __forceinline__ float4 ld_sc1(__amdgpu_buffer_rsrc_t b, unsigned off) {
    const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(b, off * 4u, 0, 16));
    return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void st_sc1(__amdgpu_buffer_rsrc_t b, unsigned off, float4 q) {
    const f32x4 v = {q.x, q.y, q.z, q.w};
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), b, off * 4u, 0, 16);
}
__device__ __forceinline__ void wait_vm0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// A 64x64 tile on its way from memory to an LDS tile, in registers (four 16-byte pieces per thread): requested with sc1 loads at float offset
// `base` (leading dimension ld), put once it is wanted -- the loads stay in flight across whatever lies between the two
struct RegTile {
    float4 v[4];
    __device__ __forceinline__ void request(__amdgpu_buffer_rsrc_t b, unsigned base, int ld, int tid) {
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const int e = tid + it * 256;
            v[it] = ld_sc1(b, base + (unsigned)(e >> 4) * (unsigned)ld + (unsigned)(e & 15) * 4u);
        }
    }
    __device__ __forceinline__ void put(float* T, int tid) const {
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const int e = tid + it * 256;
            *reinterpret_cast<float4*>(T + (e >> 4) * PLD + (e & 15) * 4) = v[it];
        }
    }
};
// a thread's 16 bytes of a block column's 16x16 inverses (requested at float offset base + 4 tid) into their LDS layout
__device__ __forceinline__ void inv_put(float4 v, float* Tinv, int tid) {
    const int p = tid >> 6, c = (tid >> 2) & 15, r4 = (tid & 3) * 4;
    float* t = Tinv + p * 16 * ILD + c * ILD + r4;
    t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
}
// 64x64 tile at float offset `base` (leading dimension ld) <-> LDS tile
__device__ __forceinline__ void load_tile_sc1(float* T, __amdgpu_buffer_rsrc_t b, unsigned base, int ld, int tid) {
    RegTile t;
    t.request(b, base, ld, tid);
    t.put(T, tid);
}
__device__ __forceinline__ void load_inv_sc1(float* Tinv, __amdgpu_buffer_rsrc_t b, unsigned base, int tid) {
    inv_put(ld_sc1(b, base + tid * 4), Tinv, tid);
}
template <bool LOWER>
__device__ __forceinline__ void store_tile_sc1(const float* T, __amdgpu_buffer_rsrc_t b, unsigned base, int ld, int tid) {
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const int e = tid + it * 256;
        const int c = e >> 4, r4 = (e & 15) * 4;
        const float4 q = *reinterpret_cast<const float4*>(T + c * PLD + r4);
        st_sc1(b, base + (unsigned)c * (unsigned)ld + (unsigned)r4,
               LOWER ? make_float4(r4 >= c ? q.x : 0.f, r4 + 1 >= c ? q.y : 0.f, r4 + 2 >= c ? q.z : 0.f, r4 + 3 >= c ? q.w : 0.f) : q);
    }
}
__device__ __forceinline__ void store_inv_sc1(const float* Tinv, __amdgpu_buffer_rsrc_t b, unsigned base, int tid) {
    const int p = tid >> 6, c = (tid >> 2) & 15, r4 = (tid & 3) * 4;
    const float* t = Tinv + p * 16 * ILD + c * ILD + r4;
    st_sc1(b, base + tid * 4, make_float4(t[0], t[1], t[2], t[3]));
}

// the 64x64 identity into an LDS tile (compact launch: tile (idb0 + c, c) of [A; X; I] has no owner)
__device__ __forceinline__ void identity_tile(float* T, int tid) {
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const int e = tid + it * 256;
        const int c = e >> 4, r4 = (e & 15) * 4;
        *reinterpret_cast<float4*>(T + c * PLD + r4) = make_float4(r4 == c ? 1.f : 0.f, r4 + 1 == c ? 1.f : 0.f, r4 + 2 == c ? 1.f : 0.f, r4 + 3 == c ? 1.f : 0.f);
    }
}
// a panel block of the identity rows with the column signs of its block column applied (store_tile_signed), write-through
__device__ __forceinline__ void store_tile_signed_sc1(const float* T, __amdgpu_buffer_rsrc_t b, unsigned base, int ld, int tid, unsigned long long neg) {
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const int e = tid + it * 256;
        const int c = e >> 4, r4 = (e & 15) * 4;
        const float* t = T + c * PLD + r4;
        const float sg = ((neg >> c) & 1ull) ? -1.f : 1.f;
        st_sc1(b, base + (unsigned)c * (unsigned)ld + (unsigned)r4, make_float4(sg * t[0], sg * t[1], sg * t[2], sg * t[3]));
    }
}

// What ONE lane of the polling wavefront looks at: a flag and the value it waits for (a count for ready[]: 4; 0 / 1 for the others).
// flag == nullptr: nothing.  Lanes 0 .. PERSIST_POLL_FLAGS - 1 (plan.h) have a flag each, lane 63 always looks at the abort word.
struct PollLane {
    const int* flag;
    int need;
};
// Every flag a consumer needs and the abort word in ONE load instruction, one memory round trip per look (three flags and the abort word
// looked at one after the other by one lane cost four round trips per look: that was most of a helper's reaction time).  A look is one
// instruction however many lanes take part, so a wait names ALL its flags here, lane by lane, from the same range its loads are addressed by.
__device__ __forceinline__ void persist_poll(const PersistArgs& a, PollLane pl, int lane, bool lazy) {
    const int* p = lane == 63 ? a.abort_flag : pl.flag;
    const int need = pl.need;
    int spins = 0;
    unsigned long long t0 = 0ull;  // (read at the first re-look only: a wait that is satisfied at once costs nothing)
    for (;;) {
        int v = need;
        if (p) v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool more = lane < 63 && v < need;
        const bool aborted = lane == 63 && v != 0;
        if (__ballot(more) == 0ull || __ballot(aborted) != 0ull) break;
        if (lazy) __builtin_amdgcn_s_sleep(PERSIST_POLL_SLEEP_LAZY);  // (whose result the chain does not wait for: fewer looks on the fabric)
        else if (PERSIST_POLL_SLEEP) __builtin_amdgcn_s_sleep(PERSIST_POLL_SLEEP);
        // Bounded by wall-clock time (ADVICE r04): a workgroup that is not resident -- compute units masked, or held by another
        // process or stream -- must cost milliseconds, not the seconds 2^22 looks of ~1 us are, before the update falls back to one
        // launch per block step.  The 100 MHz counter is read every 32 looks.
        bool timed_out = false;
        if ((spins & 31) == 0) {
            const unsigned long long now = __builtin_amdgcn_s_memrealtime();
            if (spins == 0) t0 = now;
            else timed_out = now - t0 > (unsigned long long)(unsigned)a.bound.wait_ticks;
        }
        if (++spins > a.bound.spin_limit || timed_out) {
            if (lane == 0) {
                __hip_atomic_store(a.abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                atomicOr(a.info, 2);
            }
            break;
        }
    }
}
// up to three flags, lanes 0-2 (null = nothing to wait for).  need0: the first flag is a count (ready: 4), the others are 0 / 1
__device__ __forceinline__ PollLane poll_lane3(const int* f0, const int* f1, const int* f2, int need0, int lane) {
    return {lane == 0 ? f0 : lane == 1 ? f1 : lane == 2 ? f2 : nullptr, lane == 0 ? need0 : 1};
}
__device__ __forceinline__ void persist_poll(const PersistArgs& a, const int* f0, const int* f1, const int* f2, int lane, int need0 = 1, bool lazy = false) {
    persist_poll(a, poll_lane3(f0, f1, f2, need0, lane), lane, lazy);
}
// The first wavefront polls (pl: what thread tid < 64 looks at), then the workgroup meets at a barrier.
__device__ __forceinline__ void persist_wait(const PersistArgs& a, PollLane pl, int tid, bool lazy) {
    if (tid < 64) persist_poll(a, pl, tid, lazy);
    __syncthreads();
}
__device__ __forceinline__ void persist_wait(const PersistArgs& a, const int* f0, const int* f1, const int* f2, int tid, int need0 = 1, bool lazy = false) {
    persist_wait(a, poll_lane3(f0, f1, f2, need0, tid), tid, lazy);
}
// every wavefront's write-through stores have completed, then one lane raises the flag
__device__ __forceinline__ void persist_publish(int* flag, int tid) {
    wait_vm0();
    __syncthreads();
    if (tid == 0) __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// per wavefront: its own write-through stores have completed, then one lane adds 1 to the flag (consumers wait for 4)
__device__ __forceinline__ void persist_publish_wave(int* flag, int lane) {
    wait_vm0();
    if (lane == 0) __hip_atomic_fetch_add(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#ifdef EKFVIO_TEST_HOOKS
// ekfvio_test_sweep_delay: the chosen workgroup idles `delay_ticks` of the 100 MHz clock here (every wavefront for itself, on scalar registers only;
// at most 1 ms, a third of the shortest wait bound: api.hip refuses more), then goes on as it would have
#define PERSIST_TEST_DELAY(a, point)                                                                                        \
    do {                                                                                                                    \
        if ((int)blockIdx.x == (a).delay_wg && (a).delay_point == (point)) {                                                \
            const unsigned long long t0_ = __builtin_amdgcn_s_memrealtime();                                                \
            while (__builtin_amdgcn_s_memrealtime() - t0_ < (unsigned long long)(unsigned)(a).delay_ticks) __builtin_amdgcn_s_sleep(8); \
        }                                                                                                                   \
    } while (0)
#else
#define PERSIST_TEST_DELAY(a, point) do { } while (0)
#endif
__device__ __forceinline__ unsigned long long ld_sign_sc1(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One 64x64 tile of the Kalman gain, K(ib, cb) = sum_{kb >= cb} Y(ib,kb) Z(cb,kb)^T with Y(ib,kb) the panel block of X row block ib and
// Z(cb,kb) that of identity row block cb (= block (cb,kb) of L^-T, signs applied) in block column kb: K = Y L^-1 with the structurally
// zero blocks skipped (TightlyCoupledEKF.cpp:577-580).  Per kb one k-ascending MFMA product from zero, added in ascending kb; then the
// reference's sparseView prune (:580).  Inside the persistent launch: the operands arrive while the sweep runs.  The stand-alone form of
// the same arithmetic, behind every other sweep of fewer than EKF_SWEEP_SPLIT_MB block columns, is gain_tiles_kernel: identical bits.
__device__ __forceinline__ void gain_tile(const PersistArgs& a, float* Ti, float* Tj, float* Tl, float* Tinv, int ib, int cb, int tid) {
    const int lane = tid & 63, wave = tid >> 6, wr = wave & 1, wc = wave >> 1;
    const int r = wr * 32 + (lane & 31);
    const int mb = a.mb, ldl = a.ldl;
    const __amdgpu_buffer_rsrc_t bL = persist_rsrc(a.L, (unsigned)ldl * (unsigned)(mb * PB));
    float kv[16];
#pragma unroll
    for (int q = 0; q < 16; q++) kv[q] = 0.f;
    const int iy = mb + ib, iz = a.idb0 + cb;
    for (int kb = cb; kb < mb; kb++) {
        bool signed_last = false;
        unsigned long long negl = 0ull;
        if (kb == mb - 1) {
            // The LAST block column's two panel blocks are solved here, not by their tiles' owners (who would store them, flag them, and
            // be noticed): the launch ends with this product, and the detour is ~3 k cycles of it.  Same substitution on the same
            // final tiles as the owners' (chol_panel_kernel's in the per-step sweep): the same bits.
            const __amdgpu_buffer_rsrc_t bS = persist_rsrc(a.S, (unsigned)a.lds * (unsigned)(mb * PB));
            const __amdgpu_buffer_rsrc_t bI = persist_rsrc(a.Linv, (unsigned)(mb * PB * PB));
            const bool zi = a.grid.compact() && cb == kb;  // (compact launch: tile (idb0 + mb-1, mb-1) is the identity and nobody's)
            persist_wait(a, nullptr, a.fin + iy * mb + kb, zi ? nullptr : a.fin + iz * mb + kb, tid, 1, true);
            load_tile_sc1(Ti, bS, (unsigned)(kb * PB) * (unsigned)a.lds + (unsigned)(iy * PB), a.lds, tid);
            if (zi) identity_tile(Tj, tid);
            else load_tile_sc1(Tj, bS, (unsigned)(kb * PB) * (unsigned)a.lds + (unsigned)(iz * PB), a.lds, tid);
            persist_wait(a, a.ready + kb, nullptr, nullptr, tid, 4, false);
            load_tile_sc1(Tl, bL, (unsigned)(kb * PB) * (unsigned)ldl + (unsigned)(kb * PB), ldl, tid);
            load_inv_sc1(Tinv, bI, (unsigned)(kb * PB * PB), tid);
            negl = ld_sign_sc1(a.Lsign + kb);
            __syncthreads();
            tri_solve_fwd2(Ti, Tj, Tl, Tinv, wave, lane);
            if (a.dbg && tid == 0 && ib * mb + cb < 104) a.dbg[400 + ib * mb + cb] = (long long)__builtin_amdgcn_s_memrealtime();
            signed_last = negl != 0ull;  // (the identity rows' block carries the column signs into the gain: applied inside the product)
        } else {
            persist_wait(a, nullptr, a.pan + iy * mb + kb, a.pan + iz * mb + kb, tid, 1, true);
            load_tile_sc1(Ti, bL, (unsigned)(kb * PB) * (unsigned)ldl + (unsigned)(iy * PB), ldl, tid);
            load_tile_sc1(Tj, bL, (unsigned)(kb * PB) * (unsigned)ldl + (unsigned)(iz * PB), ldl, tid);
        }
        __syncthreads();
        const f32x16 up = signed_last ? mma64_signed(Ti, 1, PLD, Tj, 1, PLD, wr, wc, lane, negl) : mma64(Ti, 1, PLD, Tj, 1, PLD, wr, wc, lane);
#pragma unroll
        for (int q = 0; q < 16; q++) kv[q] = kv[q] + up[q];
    }
    float* Kt = a.K + (size_t)(cb * PB) * a.ldk + (size_t)ib * PB;
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int c = mma64_col(wc, lane, q);
        Kt[(size_t)c * a.ldk + r] = (fabsf(kv[q]) > EKF_FLUSH_THRESH) ? kv[q] : 0.f;  // .sparseView(SPARSE_THRESH, SPARSE_EPS)
    }
}

// The column signs of an indefinite block column applied to a panel block in LDS, T(:, q) = -T(:, q) for the bits set in `neg`, or a signed copy of it
// (dst != src): what mma64_signed does to its left operand as it reads it.  The stand-alone tile kernels use this (rare, workgroup-uniform) in front
// of a plain mma64: a call to the out-of-line mma64_signed inside their block-column loop made hipcc wait for every outstanding load in front of
// each product and stopped it from reading operands ahead of the MFMAs (profiles/r06_persistent_t2.txt).
__device__ __forceinline__ void sign_cols(float* dst, const float* src, unsigned long long neg, int tid) {
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const int e = tid + it * 256;
        const int c = e >> 4, r4 = (e & 15) * 4;
        const float sg = ((neg >> c) & 1ull) ? -1.f : 1.f;
        const float4 v = *reinterpret_cast<const float4*>(src + c * PLD + r4);
        *reinterpret_cast<float4*>(dst + c * PLD + r4) = make_float4(sg * v.x, sg * v.y, sg * v.z, sg * v.w);
    }
}

// Round 6: one 64x64 tile of the gain AND everything of the update's second Joseph term that belongs to it, so that ONE GEMM is left behind the
// launch: Sigma' = T2 + K G'^T with T2 = Sigma (I - K H)^T from t2_tile and G' = K R^T - (H T2)^T (chol.hip, SchurArgs; TightlyCoupledEKF.cpp:586-600).
//   K(ib,cb)  = sum_{kb >= cb} Y(ib,kb) Z(cb,kb)^T                                  as gain_tile: the same products, the same order, the same prune;
//   W2(ib,cb) = (H T2)^T's tile = (H Sigma)^T(ib,cb) - sum_kb Y(ib,kb) S_kb HY(cb,kb)^T, HY(cb,kb) = the rows idx[64 cb ..] of block column kb of Y
//               (a row gather out of the X row blocks alo .. ahi the tile's measurement rows lie in -- one to three while every landmark is measured, more
//               with failed landmarks in between, and each one's flag is awaited: column_flags; X L^-T acts on rows one by one, so the
//               gathered rows of Y are the rows of Y whoever solves them) -- the tile's own copy of the rows idx[.] of T2, summed like t2_tile's;
//   G'(ib,cb) = K R^T - W2 (the pruned K, ascending measurement index, as joseph_g_kernel), K y's partial sums over the tile's columns -> Kyp[cb].
// WAIT: inside the persistent launch (operands awaited per block column; the LAST block column's three panel blocks are solved here from the
// finished tiles); otherwise gain2_t2_tiles_kernel, behind every other sweep of such a shape, from the stored panel blocks: the same bits.
// Th: a fourth LDS tile (the fused launch's dynamic LDS); it first serves as the 64 x 65 turning tile of (H Sigma)^T.  tab: 3 x 64 floats of LDS -- what
// the tile's epilogue needs per measurement column (residual, the two entries of R), fetched at the START: read in the epilogue they were two
// dependent memory round trips (idx, then mu) on the launch's tail.
template <bool WAIT>
__device__ __forceinline__ void gain_tile2(const PersistArgs& a, const GatherArgs& ga, float* Ti, float* Tj, float* Tl, float* Tinv, float* Th, float* tab,
                                           int ib, int cb, int tid) {
    const int lane = tid & 63, wave = tid >> 6, wr = wave & 1, wc = wave >> 1;
    const int r = wr * 32 + (lane & 31);
    const int mb = a.mb, ldl = a.ldl;
    const int m = ga.m_dev ? *ga.m_dev : ga.m;
    const __amdgpu_buffer_rsrc_t bL = persist_rsrc(a.L, (unsigned)ldl * (unsigned)(mb * PB));
    const __amdgpu_buffer_rsrc_t bS = persist_rsrc(a.S, (unsigned)a.lds * (unsigned)(mb * PB));
    const int iy = mb + ib, iz = a.idb0 + cb;
    // this lane's measurement row (for the row gathers: lanes along the measurement index) and the X row blocks the tile's rows lie in
    const int cq = cb * PB + lane;
    const int sq = (cq < m) ? ga.idx[cq] : -1;
    const unsigned sqc = (unsigned)max(sq, 0);  // the row gathers load unconditionally from a clamped row and select afterwards: written as
                                                // `(sq >= 0) ? load : 0` hipcc branches around every load and the sixteen of a column go out one by one
    int alo = 0, ahi = -1;  // (no measured row in this block column: nothing to gather, W2 = 0)
    if (cb * PB < m) {
        alo = ga.idx[cb * PB] / PB;
        ahi = ga.idx[min(cb * PB + PB - 1, m - 1)] / PB;
    }
    if (tid < 64) {
        float yq = 0.f, rd = 0.f, ro = 0.f;
        if (sq >= 0) {
            yq = ga.zrow[cq] - ga.mu[sq];
            rd = ga.Rm[2 * cq];
            ro = ga.Rm[2 * (cq ^ 1) + 1];
        }
        tab[tid] = yq, tab[64 + tid] = rd, tab[128 + tid] = ro;
    }
    // What a wait for block column kb's operands looks at, lane by lane: lane 0 the tile's own Y panel block, lane 1 its Z panel block (zflag; null:
    // none), lanes 2 .. the panel block of EVERY X row block alo .. ahi -- the range the row gather's addresses (sqc) come from.  One to three row
    // blocks while every landmark is measured (64 rows are 96 state rows); with failed landmarks in between more -- pass_mask(256, 161, "run"): block
    // column 1 holds landmarks 32..39 and 135..158, row blocks 1 .. 7 (tests/test_gpu_handoff_delay.py); never more than the nX <=
    // PERSIST_POLL_FLAGS - 2 of a shape that takes this flow (plan.h, t2_skip_owners).
    auto column_flags = [&](int kb, const int* zflag) -> PollLane {
        const int ax = alo + tid - 2;
        return {tid == 0 ? a.pan + iy * mb + kb : tid == 1 ? zflag : (tid >= 2 && ax <= ahi) ? a.pan + (mb + ax) * mb + kb : nullptr, 1};
    };
    float kv[16], w2[16];
    {   // (H Sigma)^T(ib, cb): Sigma(idx[c], i) with the lanes along c, turned through LDS (gather_body's Wt tile, without the residual row)
        float wv[16];
        const int scl = max(sq, 0);
#pragma unroll
        for (int ps = 0; ps < 16; ps++) wv[ps] = ga.P[(size_t)min(ib * PB + wave + 4 * ps, ga.n - 1) * ga.ld + scl];
#pragma unroll
        for (int ps = 0; ps < 16; ps++) asm volatile("" : "+v"(wv[ps]));
#pragma unroll
        for (int ps = 0; ps < 16; ps++) Th[(wave + 4 * ps) * 65 + lane] = (sq >= 0 && ib * PB + wave + 4 * ps < ga.n) ? wv[ps] : 0.f;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; q++) {
            kv[q] = 0.f;
            w2[q] = Th[r * 65 + mma64_col(wc, lane, q)];
        }
    }
    // one block column's operands into LDS (inside the launch: every block column but the last; behind a sweep: all of them)
    auto fetch = [&](int kb) -> unsigned long long {
        const bool gk = kb >= cb;  // (the gain's structurally zero blocks skipped)
        float hv[16];
        unsigned long long neg;
        if constexpr (WAIT) {
            persist_wait(a, column_flags(kb, gk ? a.pan + iz * mb + kb : nullptr), tid, kb < mb - 2);
            load_tile_sc1(Ti, bL, (unsigned)(kb * PB) * (unsigned)ldl + (unsigned)(iy * PB), ldl, tid);
            if (gk) load_tile_sc1(Tj, bL, (unsigned)(kb * PB) * (unsigned)ldl + (unsigned)(iz * PB), ldl, tid);
#pragma unroll
            for (int ps = 0; ps < 16; ps++)
                hv[ps] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(bL, ((unsigned)(kb * PB + wave + 4 * ps) * (unsigned)ldl + (unsigned)(mb * PB) + sqc) * 4u, 0, 16));
#pragma unroll
            for (int ps = 0; ps < 16; ps++) hv[ps] = (sq >= 0) ? hv[ps] : 0.f;
#pragma unroll
            for (int ps = 0; ps < 16; ps++) Th[(wave + 4 * ps) * PLD + lane] = hv[ps];
            neg = ld_sign_sc1(a.Lsign + kb);
        } else {
            load_tile(Ti, a.L + (size_t)kb * PB * ldl + (size_t)iy * PB, ldl, tid);
            if (gk) load_tile(Tj, a.L + (size_t)kb * PB * ldl + (size_t)iz * PB, ldl, tid);
#pragma unroll
            for (int ps = 0; ps < 16; ps++) hv[ps] = a.L[(size_t)(kb * PB + wave + 4 * ps) * ldl + (size_t)(mb * PB) + sqc];
#pragma unroll
            for (int ps = 0; ps < 16; ps++) hv[ps] = (sq >= 0) ? hv[ps] : 0.f;
#pragma unroll
            for (int ps = 0; ps < 16; ps++) Th[(wave + 4 * ps) * PLD + lane] = hv[ps];
            neg = a.Lsign[kb];
        }
        return neg;
    };
    // the block column's two products: K += Y Z^T (the structurally zero blocks skipped), W2 -= Y S HY^T
    auto products = [&](int kb, unsigned long long neg, bool z_unsigned) {
        if (kb >= cb) {
            // (z_unsigned: inside the launch the last block column's identity-row block is solved here and carries no column signs yet)
            const f32x16 up = (z_unsigned && neg != 0ull) ? mma64_signed(Ti, 1, PLD, Tj, 1, PLD, wr, wc, lane, neg) : mma64(Ti, 1, PLD, Tj, 1, PLD, wr, wc, lane);
#pragma unroll
            for (int q = 0; q < 16; q++) kv[q] = kv[q] + up[q];
        }
        if (alo <= ahi) {
            f32x16 up;
            if constexpr (WAIT) {
                up = (neg == 0ull) ? mma64(Ti, 1, PLD, Th, 1, PLD, wr, wc, lane) : mma64_signed(Ti, 1, PLD, Th, 1, PLD, wr, wc, lane, neg);
            } else {
                if (__builtin_amdgcn_readfirstlane((int)(neg != 0ull))) {  // (rare, uniform: the signs go onto Y's block in LDS; the gain's product is done with it)
                    __syncthreads();
                    sign_cols(Ti, Ti, neg, tid);
                    __syncthreads();
                }
                up = mma64(Ti, 1, PLD, Th, 1, PLD, wr, wc, lane);
            }
#pragma unroll
            for (int q = 0; q < 16; q++) w2[q] = w2[q] - up[q];
        }
        if (WAIT && a.dbg && tid == 0 && mb <= 8 && (ib == 0 || ib == 6) && (cb == 0 || cb == 3 || cb == 7))
            a.dbg[100 + 8 * ((ib ? 3 : 0) + (cb == 0 ? 0 : cb == 3 ? 1 : 2)) + kb] = (long long)__builtin_amdgcn_s_memrealtime();
    };
    if constexpr (WAIT) {
        for (int kb = 0; kb < mb - 1; kb++) {  // (block column mb-2: an ordinary column, but its wait is not lazy -- the launch's tail begins with it)
            __syncthreads();  // (the previous block column's readers of Ti / Tj / Th)
            const unsigned long long neg = fetch(kb);
            __syncthreads();
            products(kb, neg, false);
        }
    } else {
        // behind a sweep everything is in memory: one block column after the other, operands straight into the LDS tiles.  (Requesting column
        // kb + 1 under column kb's products was tried three ways -- staging registers carried round the loop: hipcc keeps them in scratch; a second
        // set of LDS tiles with swapped pointers: the products lose their compile-time LDS addresses and hipcc stops reading operands ahead of
        // the MFMAs; both measured 40-55 us for the stand-alone kernel against ~25 for this plain loop.)
        for (int kb = 0; kb < mb; kb++) {
            __syncthreads();  // (the previous block column's readers of Ti / Tj / Th; first round: the turning tile's)
            const unsigned long long neg = fetch(kb);
            __syncthreads();
            products(kb, neg, false);
        }
    }
    if constexpr (WAIT) {
        // The last block column.  An owner of an X or identity row block announces its panel block (`pan`, behind its last step's product) BEFORE its
        // finished tile (`fin`): nothing follows from column mb-2's `pan` flags about column mb-1's finished tiles, although the same owners raise
        // both.  So the wait names ready[mb-1] and EVERY finished tile read below, in ONE look; ONE round trip then brings the three tiles' data,
        // L_last, its inverses and its signs, through registers.  (Measured, profiles/early_panel.txt: that round trip requested in front of column
        // mb-2's products, or between its two products, costs more than it hides -- the wait in front of it then delays products that could run.)
        const int kl = mb - 1;
        const __amdgpu_buffer_rsrc_t bI = persist_rsrc(a.Linv, (unsigned)(mb * PB * PB));
        const bool zi = a.grid.compact() && cb == kl;  // (compact launch: tile (idb0 + mb-1, mb-1) is the identity and nobody's)
        // What the wait for the last block column looks at, lane by lane: lane 0 ready[mb-1] (the chain's four wavefronts), lane 1 the finished tile
        // (iy, mb-1), lane 2 the finished tile (iz, mb-1) (zi: none), lanes 3 .. the finished tile of EVERY X row block alo .. ahi, the range the row
        // gather hq is addressed by -- at most nX + 3 lanes, which a shape that takes this flow has (plan.h, t2_skip_owners).
        const int axl = alo + tid - 3;
        const PollLane last_flags = {tid == 0 ? a.ready + kl : tid == 1 ? a.fin + iy * mb + kl : tid == 2 ? (zi ? nullptr : a.fin + iz * mb + kl)
                                     : (axl <= ahi) ? a.fin + (mb + axl) * mb + kl : nullptr, tid == 0 ? 4 : 1};
        __syncthreads();  // (column mb-2's readers of Ti / Tj / Th)
        RegTile ql, qi, qj;
        float hq[16];
        persist_wait(a, last_flags, tid, false);
        ql.request(bL, (unsigned)(kl * PB) * (unsigned)ldl + (unsigned)(kl * PB), ldl, tid);
        qi.request(bS, (unsigned)(kl * PB) * (unsigned)a.lds + (unsigned)(iy * PB), a.lds, tid);
        if (!zi) qj.request(bS, (unsigned)(kl * PB) * (unsigned)a.lds + (unsigned)(iz * PB), a.lds, tid);
        const float4 qv = ld_sc1(bI, (unsigned)(kl * PB * PB) + tid * 4);
        const unsigned long long neg7 = ld_sign_sc1(a.Lsign + kl);
#pragma unroll
        for (int ps = 0; ps < 16; ps++)
            hq[ps] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(bS, ((unsigned)(kl * PB + wave + 4 * ps) * (unsigned)a.lds + (unsigned)(mb * PB) + sqc) * 4u, 0, 16));
        ql.put(Tl, tid);
        qi.put(Ti, tid);
        if (zi) identity_tile(Tj, tid);
        else qj.put(Tj, tid);
        inv_put(qv, Tinv, tid);
#pragma unroll
        for (int ps = 0; ps < 16; ps++) Th[(wave + 4 * ps) * PLD + lane] = (sq >= 0) ? hq[ps] : 0.f;
        __syncthreads();
        float* const t3[3] = {Ti, Tj, Th};
        tri_solve_fwd_n<3>(t3, Tl, Tinv, wave, lane);
        __syncthreads();
        products(kl, neg7, true);
    }
    // K pruned (.sparseView(SPARSE_THRESH, SPARSE_EPS), :580); G' = K R^T - W2; K (z - H mu) over the tile's columns (:554-555, :600)
#pragma unroll
    for (int q = 0; q < 16; q++) kv[q] = (fabsf(kv[q]) > EKF_FLUSH_THRESH) ? kv[q] : 0.f;
    float* Kt = a.K + (size_t)(cb * PB) * a.ldk + (size_t)ib * PB;
    float* Gt = ga.G + (size_t)(cb * PB) * ga.ld + (size_t)ib * PB;
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int c = mma64_col(wc, lane, q), cg = cb * PB + c;
        Kt[(size_t)c * a.ldk + r] = kv[q];
        float g = 0.f;
        if (cg < m) {
            // (K R^T)(i,q) = K(i,q) R(q,q) + K(i,q^1) R(q,q^1), ascending measurement index (the partner column is this thread's kv[q ^ 1])
            const float x = kv[q] * tab[64 + c], y = kv[q ^ 1] * tab[128 + c];
            const float kr = ((cg ^ 1) < cg) ? (y + x) : (x + y);
            g = kr - w2[q];
            acc = acc + kv[q] * tab[c];
        }
        Gt[(size_t)c * ga.ld + r] = g;
    }
    __syncthreads();
    float* part = Th;  // [4][64]: this tile's K y, summed over (column half, lane half) in a fixed order
    part[(wc * 2 + (lane >> 5)) * 64 + r] = acc;
    __syncthreads();
    if (tid < 64) ga.Wt[(size_t)cb * ga.ld + (size_t)ib * PB + tid] = ((part[tid] + part[64 + tid]) + part[128 + tid]) + part[192 + tid];
}

// One tile pair of T2 = Sigma - Y S Y^T (round 6).  X = Sigma H^T, so Y S Y^T = X A^-1 X^T = Sigma H^T K^T and T2 = Sigma (I - K H)^T: the Schur
// complement of A in [[A, X^T], [X, Sigma]], i.e. just more trailing tiles of the sweep (chol.hip, SchurArgs, for which Joseph factor this is and
// how the update is finished: Sigma' = T2 + K (R K^T - H T2), TightlyCoupledEKF.cpp:594-596).  Tile (ta, tb), ta >= tb, and its mirror image from
// the same product: per block column k one k-ascending MFMA product Y(ta,k) S_k Y(tb,k)^T from zero, subtracted in ascending k (the mirror tile
// gets the product turned through LDS: the same sums).  WAIT: inside the persistent launch, the operands arrive while the sweep runs (`pan`
// flags; the LAST block column's two panel blocks are solved here from the owners' finished tiles, like gain_tile's); otherwise
// (gain2_t2_tiles_kernel, behind every other sweep of such a shape) they are read back from L.  The same operands in the same order: the same bits.
template <bool WAIT>
__device__ __forceinline__ void t2_tile(const PersistArgs& a, float* Ti, float* Tj, float* Tl, float* Tinv, int ta, int tb, int tid, long long* dbg = nullptr) {
    const int lane = tid & 63, wave = tid >> 6, wr = wave & 1, wc = wave >> 1;
    const int r = wr * 32 + (lane & 31);
    const int mb = a.mb, ldl = a.ldl;
    const bool diag = ta == tb;
    const __amdgpu_buffer_rsrc_t bL = persist_rsrc(a.L, (unsigned)ldl * (unsigned)(mb * PB));
    float tab[16], tba[16];
    {
        const float* sab = a.Sg + (size_t)tb * PB * a.ldsg + (size_t)ta * PB;
        const float* sba = a.Sg + (size_t)ta * PB * a.ldsg + (size_t)tb * PB;
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int c = mma64_col(wc, lane, q);
            tab[q] = sab[(size_t)c * a.ldsg + r];
            tba[q] = diag ? 0.f : sba[(size_t)c * a.ldsg + r];
        }
    }
    const int ia = mb + ta, ib = mb + tb;
    // a block column's product from the operands in LDS: subtracted from the tile, and, turned through LDS (L_kk's tile: nobody reads it
    // past the substitution), from its mirror image
    auto apply = [&](int kb, unsigned long long neg) {
        const float* Bj = diag ? Ti : Tj;
        f32x16 up;
        if constexpr (WAIT) {
            up = (neg == 0ull) ? mma64(Ti, 1, PLD, Bj, 1, PLD, wr, wc, lane) : mma64_signed(Ti, 1, PLD, Bj, 1, PLD, wr, wc, lane, neg);
        } else if (__builtin_amdgcn_readfirstlane((int)(neg != 0ull))) {
            // (rare, uniform: a signed copy of the left operand in the turning tile -- on the diagonal both operands are Ti, so not in place)
            sign_cols(Tl, Ti, neg, tid);
            __syncthreads();
            up = mma64(Tl, 1, PLD, Bj, 1, PLD, wr, wc, lane);
            __syncthreads();
        } else {
            up = mma64(Ti, 1, PLD, Bj, 1, PLD, wr, wc, lane);
        }
#pragma unroll
        for (int q = 0; q < 16; q++) tab[q] = tab[q] - up[q];
        if (!diag) {
#pragma unroll
            for (int q = 0; q < 16; q++) Tl[r * PLD + mma64_col(wc, lane, q)] = up[q];
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 16; q++) tba[q] = tba[q] - Tl[mma64_col(wc, lane, q) * PLD + r];
        }
        if (dbg && tid == 0) dbg[kb] = (long long)__builtin_amdgcn_s_memrealtime();
    };
    if constexpr (WAIT) {
        for (int kb = 0; kb < mb - 1; kb++) {
            __syncthreads();  // (the previous product's readers of Ti / Tj, the previous turn's of Tl)
            persist_wait(a, nullptr, a.pan + ia * mb + kb, diag ? nullptr : a.pan + ib * mb + kb, tid, 1, kb < mb - 2);
            load_tile_sc1(Ti, bL, (unsigned)(kb * PB) * (unsigned)ldl + (unsigned)(ia * PB), ldl, tid);
            if (!diag) load_tile_sc1(Tj, bL, (unsigned)(kb * PB) * (unsigned)ldl + (unsigned)(ib * PB), ldl, tid);
            const unsigned long long neg = ld_sign_sc1(a.Lsign + kb);
            __syncthreads();
            apply(kb, neg);
        }
    } else {
        for (int kb = 0; kb < mb; kb++) {  // behind a sweep: one block column after the other (see gain_tile2)
            __syncthreads();  // (the previous product's readers of Ti / Tj, the previous turn's of Tl)
            load_tile(Ti, a.L + (size_t)kb * PB * ldl + (size_t)ia * PB, ldl, tid);
            if (!diag) load_tile(Tj, a.L + (size_t)kb * PB * ldl + (size_t)ib * PB, ldl, tid);
            const unsigned long long neg = a.Lsign[kb];
            __syncthreads();
            apply(kb, neg);
        }
    }
    if constexpr (WAIT) {
        // The last block column (column mb-2 was an ordinary column of the loop, its wait not lazy).  Nothing follows from column mb-2's `pan` flags
        // about the finished tiles of column mb-1 -- their owners announce the panel block first and the tile later -- so the ONE look names
        // ready[mb-1] and both finished tiles read here; ONE round trip then brings the tiles, L_last, its inverses and its signs.
        const int kl = mb - 1;
        const __amdgpu_buffer_rsrc_t bS = persist_rsrc(a.S, (unsigned)a.lds * (unsigned)(mb * PB));
        const __amdgpu_buffer_rsrc_t bI = persist_rsrc(a.Linv, (unsigned)(mb * PB * PB));
        __syncthreads();
        RegTile ql, qi, qj;
        persist_wait(a, a.ready + kl, a.fin + ia * mb + kl, diag ? nullptr : a.fin + ib * mb + kl, tid, 4, false);
        ql.request(bL, (unsigned)(kl * PB) * (unsigned)ldl + (unsigned)(kl * PB), ldl, tid);
        qi.request(bS, (unsigned)(kl * PB) * (unsigned)a.lds + (unsigned)(ia * PB), a.lds, tid);
        if (!diag) qj.request(bS, (unsigned)(kl * PB) * (unsigned)a.lds + (unsigned)(ib * PB), a.lds, tid);
        const float4 qv = ld_sc1(bI, (unsigned)(kl * PB * PB) + tid * 4);
        const unsigned long long neg7 = ld_sign_sc1(a.Lsign + kl);
        ql.put(Tl, tid);
        qi.put(Ti, tid);
        if (!diag) qj.put(Tj, tid);
        inv_put(qv, Tinv, tid);
        __syncthreads();
        if (diag) tri_solve_fwd(Ti, Tl, Tinv, wave, lane);
        else tri_solve_fwd2(Ti, Tj, Tl, Tinv, wave, lane);
        __syncthreads();
        apply(kl, neg7);
    }
    // out, whole lines through LDS; zero outside n x n (the padding of the covariance buffers stays zero whatever the factor held)
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int c = mma64_col(wc, lane, q);
        Ti[c * PLD + r] = (ta * PB + r < a.nstate && tb * PB + c < a.nstate) ? tab[q] : 0.f;
        if (!diag) Tj[c * PLD + r] = (tb * PB + r < a.nstate && ta * PB + c < a.nstate) ? tba[q] : 0.f;
    }
    __syncthreads();
    store_tile(Ti, a.T2 + (size_t)tb * PB * a.ldt + (size_t)ta * PB, a.ldt, tid);
    if (!diag) store_tile(Tj, a.T2 + (size_t)ta * PB * a.ldt + (size_t)tb * PB, a.ldt, tid);
    if (dbg && tid == 0) dbg[15] = (long long)__builtin_amdgcn_s_memrealtime();
}

template <bool SC1>
__device__ __forceinline__ float persist_ldf(const float* p) {
    if constexpr (SC1) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}
// a 64x64 tile's rows 16*wave .. +15 in the substitution's register layout (tri_solve_load_x), straight from memory
template <bool SC1>
__device__ __forceinline__ void persist_tile_x(f32x4 (&x)[4], const float* G, int ld, int wave, int lane) {
    const int li = lane & 15, g = lane >> 4;
#pragma unroll
    for (int b = 0; b < 4; b++)
#pragma unroll
        for (int v = 0; v < 4; v++) x[b][v] = persist_ldf<SC1>(G + (size_t)(16 * b + 4 * g + v) * ld + 16 * wave + li);
}
// 16x16 block (tr, tc) of a diagonal tile in LDS: D -= P S P^T over the 64 columns of the panel block P (LDS), one
// wavefront.  The product is a k-ascending chain of fused multiply-adds like mma64's: the same bits.
__device__ __forceinline__ void persist_diag_block(float* D, const float* P, int tr, int tc, int lane, unsigned long long neg) {
    const int li = lane & 15, lk = lane >> 4;
    const int rb = 16 * tr, cb = 16 * tc;
    const float* ap = P + rb + li + lk * PLD;
    const float* bp = P + cb + li + lk * PLD;
    f32x4 u = {0.f, 0.f, 0.f, 0.f};
    if (neg == 0ull) {
#pragma unroll
        for (int q = 0; q < PB; q += 4) u = __builtin_amdgcn_mfma_f32_16x16x4f32(bp[q * PLD], ap[q * PLD], u, 0, 0, 0);
    } else {
#pragma unroll 4
        for (int q = 0; q < PB; q += 4) {
            float av = ap[q * PLD];
            if ((neg >> (q + lk)) & 1ull) av = -av;
            u = __builtin_amdgcn_mfma_f32_16x16x4f32(bp[q * PLD], av, u, 0, 0, 0);
        }
    }
    float t[4];
#pragma unroll
    for (int gq = 0; gq < 4; gq++) t[gq] = D[(cb + 4 * lk + gq) * PLD + rb + li];
#pragma unroll
    for (int gq = 0; gq < 4; gq++) D[(cb + 4 * lk + gq) * PLD + rb + li] = t[gq] - u[gq];
}


// ---- fused launch (round 4): a 64x64 tile of the augmented matrix [A; X; I] gathered straight from Sigma into an LDS tile ----
// (what gather_body writes to Saug in the two-launch form: the same elements through the same gather_a_elem).  Row block rb,
// column block cb.  Three phases so that several tiles' loads travel together: indices, values, LDS writes.
//   A tile (rb < mb):          (r,c) = S(c,r) = Sigma(idx[c], idx[r]) + R; lanes along c (P[idx[r]*ld + idx[c]] is nearly contiguous in c)
//   X tile (mb <= rb < idb0):  (r,c) = Sigma(x, idx[c]), x = 64 (rb - mb) + r; lanes along r (contiguous)
//   I tile (rb >= idb0):       the identity block when rb - idb0 == cb, else zero
struct GTile {
    int ia[16];     // A: idx of the 16 rows of this thread;  X: idx of its 16 columns
    int ib;         // A: idx of its column
    float v[16], rd[16], ro[16];
};
__device__ __forceinline__ void gtile_idx(GTile& t, const GatherArgs& ga, int m, int rb, int cb, int mb, int idb0, int tid) {
    if (rb < mb) {
        const int c = cb * PB + (tid & 63);
        t.ib = (c < m) ? ga.idx[c] : 0;
#pragma unroll
        for (int ps = 0; ps < 16; ps++) {
            const int rc = max(min(rb * PB + (tid >> 6) + 4 * ps, m - 1), 0);  // m may be 0 when it is only known on the device
            t.ia[ps] = max(ga.idx[rc], 0);
            t.rd[ps] = ga.Rm[2 * rc];
            t.ro[ps] = ga.Rm[2 * rc + 1];
        }
    } else if (rb < idb0) {
#pragma unroll
        for (int ps = 0; ps < 16; ps++) {
            const int c = cb * PB + (tid >> 6) + 4 * ps;
            t.ia[ps] = (c < m) ? ga.idx[c] : 0;
        }
    }
}
__device__ __forceinline__ void gtile_val(GTile& t, const GatherArgs& ga, int m, int rb, int cb, int mb, int idb0, int tid) {
    if (rb < mb) {
#pragma unroll
        for (int ps = 0; ps < 16; ps++) t.v[ps] = ga.P[(size_t)t.ia[ps] * ga.ld + t.ib];
    } else if (rb < idb0) {
        const int x = min((rb - mb) * PB + (tid & 63), ga.ld - 1);
#pragma unroll
        for (int ps = 0; ps < 16; ps++) t.v[ps] = ga.P[(size_t)t.ia[ps] * ga.ld + x];
    }
}
__device__ __forceinline__ void gtile_put(const GTile& t, float* T, const GatherArgs& ga, int m, int rb, int cb, int mb, int idb0, int tid) {
    if (rb < mb) {
        const int cl = tid & 63, c = cb * PB + cl;
#pragma unroll
        for (int ps = 0; ps < 16; ps++) {
            const int rl = (tid >> 6) + 4 * ps;
            T[cl * PLD + rl] = gather_a_elem(t.v[ps], rb * PB + rl, c, m, t.rd[ps], t.ro[ps]);
        }
    } else if (rb < idb0) {
        const int rl = tid & 63, x = (rb - mb) * PB + rl;
#pragma unroll
        for (int ps = 0; ps < 16; ps++) {
            const int cl = (tid >> 6) + 4 * ps;
            T[cl * PLD + rl] = (cb * PB + cl < m && x < ga.n) ? t.v[ps] : 0.f;
        }
    } else {
        const int rl = tid & 63;
#pragma unroll
        for (int ps = 0; ps < 16; ps++) {
            const int cl = (tid >> 6) + 4 * ps;
            T[cl * PLD + rl] = (rb - idb0 == cb && rl == cl) ? 1.f : 0.f;
        }
    }
}
__device__ __forceinline__ void gtile_pin(GTile& t) {
#pragma unroll
    for (int ps = 0; ps < 16; ps++) asm volatile("" : "+v"(t.ia[ps]));
}
__device__ __forceinline__ void gtile_pinv(GTile& t) {
#pragma unroll
    for (int ps = 0; ps < 16; ps++) asm volatile("" : "+v"(t.v[ps]));
}

// persist_tile_x for the chain's hot path: the same sixteen values per lane as buffer loads whose sixteen 32-bit offsets are all formed
// (and pinned) BEFORE the first load is issued.  Written as persist_tile_x, the compiler forms each 64-bit address in registers that are
// still the destination of an earlier load of the batch and puts a counted wait in front of it: the batch trickles out behind
// `s_waitcnt vmcnt(15)`s, and since vmcnt retires in order those waits also drain the factor's write-through stores issued just before --
// ~1 k cycles per block step on the chain.
__device__ __forceinline__ void persist_tile_x_buf(f32x4 (&x)[4], __amdgpu_buffer_rsrc_t b, unsigned base, int ld, int wave, int lane) {
    const int li = lane & 15, g = lane >> 4;
    unsigned off[16];
#pragma unroll
    for (int q = 0; q < 16; q++) off[q] = (base + (unsigned)(16 * (q >> 2) + 4 * g + (q & 3)) * (unsigned)ld + (unsigned)(16 * wave + li)) * 4u;
#pragma unroll
    for (int q = 0; q < 16; q++) asm volatile("" : "+v"(off[q]));
#pragma unroll
    for (int q = 0; q < 16; q++) x[q >> 2][q & 3] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(b, off[q], 0, 16));
}

__global__ __launch_bounds__(256) void chol_persist_kernel(PersistArgs a, GatherArgs ga) {
    extern __shared__ __attribute__((aligned(16))) float persist_dyn_lds[];  // fused launch: the gather's transposing tile (and one workgroup per compute unit)
    __shared__ __attribute__((aligned(16))) float Ti[PB * PLD];
    __shared__ __attribute__((aligned(16))) float Tj[PB * PLD];
    __shared__ __attribute__((aligned(16))) float Tl[PB * PLD];
    __shared__ float Tinv[INV_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave & 1, wc = wave >> 1;
    const int r = wr * 32 + (lane & 31);
    const int mb = a.mb, lds = a.lds, ldl = a.ldl;
    const bool fused = a.grid.fused(), compact = a.grid.compact();
    const PersistRole role = a.grid.role((int)blockIdx.x);  // (plan.h, PersistGrid: the grid is described there)
    float* S = a.S;
    float* L = a.L;
    const __amdgpu_buffer_rsrc_t bS = persist_rsrc(S, (unsigned)lds * (unsigned)(mb * PB));
    const __amdgpu_buffer_rsrc_t bL = persist_rsrc(L, (unsigned)ldl * (unsigned)(mb * PB));
    const __amdgpu_buffer_rsrc_t bI = persist_rsrc(a.Linv, (unsigned)(mb * PB * PB));
#define PSTAMP(slot)                                                                               \
    do {                                                                                           \
        if (a.dbg && tid == 0) a.dbg[(slot)] = (long long)__builtin_amdgcn_s_memtime();            \
    } while (0)

    // diagnostic (scripts/t2_stamps.py): when the launch's last workgroup leaves, on the one clock all XCDs share, and who it was
#define PEXIT()                                                                                                         \
    do {                                                                                                                \
        if (a.dbg && tid == 0) {                                                                                        \
            const unsigned long long t_ = __builtin_amdgcn_s_memrealtime();                                             \
            if (atomicMax(reinterpret_cast<unsigned long long*>(a.dbg + 898), t_) < t_) a.dbg[899] = (long long)blockIdx.x; \
        }                                                                                                               \
        return;                                                                                                         \
    } while (0)
    if (a.dbg && tid == 0 && blockIdx.x >= 252 && blockIdx.x < 268) {  // (diagnostic: when the blocks past the 256th get their compute unit, and which XCC)
        a.dbg[160 + blockIdx.x - 252] = (long long)__builtin_amdgcn_s_memrealtime();
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        a.dbg[176 + blockIdx.x - 252] = (long long)(xcc & 15);
    }
    if (role.kind == ROLE_CHAIN) {
        // ---------------- the chain ----------------
        // Per step k: L_ik = A_ik L_kk^-T (i = k+1), A_ii -= L_ik S L_ik^T, A_ii = L_ii L_ii^T.  What is on the path between two
        // pivot chains is kept short:
        //   * the substitution's operands (L_kk, its inverses) go to registers from LDS BEFORE anything is waited for, and
        //     tile (i,k) arrives in the substitution's register layout straight from memory (no LDS staging);
        //   * the two flags of a step are looked at once right behind the previous factorisation (the answer travels while
        //     the factor is stored and the operands are fetched): when both are up, as they are unless the helpers are late,
        //     the step starts with its loads instead of a poll;
        //   * of the diagonal tile's update only block column 0 (what panel 0's pivot chain reads) is formed before the
        //     factorisation starts; the six other lower 16x16 blocks are formed by wavefronts 1-3 while wavefront 0 runs
        //     panel 0 (they have nothing else to do there), in place in LDS;
        //   * the factor, its inverses and the sign mask go out write-through and nobody here waits for them: each wavefront
        //     raises ready[i] by one once ITS stores have completed, at the top of the next step behind the operand fetches.
        // L_kk and the tile being factored alternate between two LDS tiles.
        // (Measured and dropped: wavefronts 1-3 fetching the next step's two tiles under the last panel's pivot chain --
        // the helpers' flags are up too late for it every other step, no gain; a second group of four wavefronts in this
        // workgroup applying the last step to those tiles from LDS -- scripts/experiments/chol_persist_band_group.inc.txt:
        // eight wavefronts share the compute unit's LDS and matrix pipes with the pivot chain, 24 k cycles per step
        // against 17 k.  Round 5: tile (0,0)'s factorisation and the loop's are two inlined copies of potrf64_lds and each runs once from a
        // cold instruction cache (11 k cycles instead of 8.9 k).  One copy -- the loop entered at "step -1", or an out-of-line function
        // -- was built both ways, bit-identical: the first costs the loop's steady state what it saves up front (hipcc's schedule of the store
        // phase, +0.5 k cycles per step: 99.4 against 98.4 us per filter step), the second loses the compile-time LDS addresses (10.3 k
        // cycles per factorisation).  Two copies stay.)
        PSTAMP(0);
        if (a.dbg && tid == 0) a.dbg[896] = (long long)__builtin_amdgcn_s_memrealtime();
        float* Lk = Tl;   // L_kk
        float* Dn = Tj;   // the next diagonal tile
        unsigned long long neg;
        if (fused) {
            // ---- tile (0,0): gathered straight from Sigma (the elements the two-launch form's gather writes to Saug, through the same
            // gather_a_elem), factored here and kept in LDS for step 0; it leaves write-through for the owners.  (Step 0's two tiles,
            // (1,0) and (1,1), are gathered by two workgroups of their own meanwhile and arrive like every later step's: a 64x64
            // gather is ~5 k cycles of scattered loads per tile, three of them in front of the first pivot cost 8 k.) ----
            // Three dependent round trips stood in front of the first pivot (m on the device, then idx / R, then Sigma).  Round 6: they travel
            // as ONE batch -- idx[0..63] and R are readable whatever m is (m_cap >= 64), and Sigma is requested at the places the first 32
            // landmarks' (u, v) rows have when all of them are measured, idx[r] = 22 + 3 (r / 2) + (r & 1).  The guess is then CHECKED against
            // m and idx; a frame it does not hold for (a failed landmark among the first 32) asks for Sigma again at the real places: the
            // same elements through the same gather_a_elem either way.
            // (m through a lane offset the compiler cannot see through: read as a uniform value it is moved to a scalar register at once,
            // `s_waitcnt vmcnt(0); v_readfirstlane`, a round trip of its own in front of the batch)
            unsigned zoff = 0;
            asm volatile("" : "+v"(zoff));
            const int m = ga.m_dev ? ga.m_dev[zoff] : ga.m;
            {
                GTile t0;
                int all_hit = 0;
                {
                    const int c0 = tid & 63;
                    const int gib = EKF_BASE + 3 * (c0 >> 1) + (c0 & 1);
                    t0.ib = ga.idx[c0];
                    bool hit = true;
#pragma unroll
                    for (int ps = 0; ps < 16; ps++) {
                        const int r0 = (tid >> 6) + 4 * ps;
                        t0.ia[ps] = ga.idx[r0];
                        t0.rd[ps] = ga.Rm[2 * r0];
                        t0.ro[ps] = ga.Rm[2 * r0 + 1];
                        t0.v[ps] = ga.P[(size_t)(EKF_BASE + 3 * (r0 >> 1) + (r0 & 1)) * ga.ld + gib];
                    }
#pragma unroll
                    for (int ps = 0; ps < 16; ps++) {
                        const int r0 = (tid >> 6) + 4 * ps;
                        hit = hit && t0.ia[ps] == EKF_BASE + 3 * (r0 >> 1) + (r0 & 1);
                    }
                    hit = hit && t0.ib == gib && m >= PB;
                    all_hit = __syncthreads_and(hit);
                }
                if (a.dbg && tid == 0) a.dbg[900] = all_hit;
                if (!all_hit) {
                    gtile_idx(t0, ga, m, 0, 0, mb, a.idb0, tid);
                    gtile_pin(t0);
                    gtile_val(t0, ga, m, 0, 0, mb, a.idb0, tid);
                    gtile_pinv(t0);
                }
                gtile_put(t0, Lk, ga, m, 0, 0, mb, a.idb0, tid);
            }
            __syncthreads();
            PSTAMP(1);
            const bool bad0 = potrf64_lds<EKF_POTRF_FV>(Lk, Tinv, tid);
            neg = 0ull;
            if (bad0) {  // workgroup-uniform, rare: gathered again and factored as U S U^T
                __syncthreads();
                GTile t0;
                gtile_idx(t0, ga, m, 0, 0, mb, a.idb0, tid);
                gtile_val(t0, ga, m, 0, 0, mb, a.idb0, tid);
                gtile_put(t0, Lk, ga, m, 0, 0, mb, a.idb0, tid);
                neg = potrf64_signed(Lk, Tinv, tid);
            }
            PSTAMP(2);
            store_tile_sc1<true>(Lk, bL, 0u, ldl, tid);
            store_inv_sc1(Tinv, bI, 0u, tid);
            if (tid == 0) {
                __hip_atomic_store(a.Lsign, neg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (bad0) atomicOr(a.info, 1);
            }
            asm volatile("" ::: "memory");  // (ready[0] goes up at the top of step 0, behind its tile requests, like every ready[k])
            PSTAMP(3);
        } else {
            load_tile(Lk, L, ldl, tid);  // L_00 and its inverses: written by the previous launch
            load_inv(Tinv, a.Linv, tid);
            neg = a.Lsign[0];
            __syncthreads();
        }
        const int li = lane & 15, g = lane >> 4;
        int seen = 1;  // lanes 0 / 1 of every wavefront: the early look at the next step's two flags
        const int kf = fused ? 0 : 1;  // the first step whose tiles (and whose ready[k]) are handed over inside this launch
        if (fused && lane < 2) seen = __hip_atomic_load(lane == 0 ? a.fin + 1 * mb + 0 : a.fin + 1 * mb + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int k = 0; k + 1 < mb; k++) {
            const int i = k + 1;
            PSTAMP(32 + 8 * k + 0);
            TriOps ops;
            tri_solve_preload(ops, Lk, Tinv, lane);
            const unsigned oik = (unsigned)(k * PB) * (unsigned)lds + (unsigned)(i * PB);  // tile (i,k)
            const unsigned oii = (unsigned)(i * PB) * (unsigned)lds + (unsigned)(i * PB);  // tile (i,i)
            f32x4 x[1][4];
            RegTile dt;
            // final column tile (i,k), and the diagonal tile with steps 0 .. k-1 applied.  Every wavefront has looked at the
            // two flags for itself right behind the previous factorisation; if both were up (they are, unless the helpers
            // are late) it requests its rows of tile (i,k) and its share of the diagonal tile now, behind its own match.
            // (One look only, issued BEFORE the factor's stores.  A second look behind the stores -- tried in round 4 -- makes the compiler wait
            // for vmcnt(0) here, i.e. for the write-through stores themselves, ~1 k cycles per step: its result register is the newest
            // outstanding memory operation, and any use of it, or re-use of its register, needs everything older to have completed.)
            const bool hit = k >= kf && __ballot(lane < 2 && seen == 0) == 0ull;
            if (a.dbg && tid == 0 && k >= kf) a.dbg[500 + k] = hit ? 100 : 101;
            if (hit) {
                unsigned od[4];
#pragma unroll
                for (int it = 0; it < 4; it++) {
                    const int e = tid + it * 256;
                    od[it] = oii + (unsigned)(e >> 4) * (unsigned)lds + (unsigned)(e & 15) * 4u;
                    asm volatile("" : "+v"(od[it]));
                }
                persist_tile_x_buf(x[0], bS, oik, lds, wave, lane);
#pragma unroll
                for (int it = 0; it < 4; it++) dt.v[it] = ld_sc1(bS, od[it]);
                // the previous step's factor is out: this wavefront's stores were issued in front of these 20 loads
                asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
                if (lane == 0) __hip_atomic_fetch_add(a.ready + k, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else if (k >= kf) {
                persist_publish_wave(a.ready + k, lane);  // the previous step's factor is out
                persist_poll(a, a.fin + i * mb + k, a.fin + i * mb + i, nullptr, lane);  // (per wavefront: no barrier here, the wavefronts need not agree on `hit`)
                persist_tile_x<true>(x[0], S + oik, lds, wave, lane);
                dt.request(bS, oii, lds, tid);
            } else {
                persist_tile_x<false>(x[0], S + oik, lds, wave, lane);
#pragma unroll
                for (int it = 0; it < 4; it++) {
                    const int e = tid + it * 256;
                    dt.v[it] = *reinterpret_cast<const float4*>(S + oii + (size_t)(e >> 4) * lds + (e & 15) * 4);
                }
            }
            PSTAMP(32 + 8 * k + 1);
            tri_solve_pin(ops);
            PSTAMP(32 + 8 * k + 2);
            float* const txs[1] = {Ti};
            tri_solve_run<1>(x, txs, ops, wave, lane);  // L_ik into Ti
            dt.put(Dn, tid);  // the diagonal tile has had the substitution's time to arrive
            {   // the panel block (read by later launches only) leaves from the registers
                float* Pdst = L + (size_t)k * PB * ldl + (size_t)i * PB + 16 * wave + li;
#pragma unroll
                for (int bq = 0; bq < 4; bq++)
#pragma unroll
                    for (int v = 0; v < 4; v++) Pdst[(size_t)(16 * bq + 4 * g + v) * ldl] = x[0][bq][v];
            }
            __syncthreads();
            PSTAMP(32 + 8 * k + 3);
            persist_diag_block(Dn, Ti, wave, 0, lane, neg);  // block column 0 of the updated tile, one 16x16 block per wavefront
            __syncthreads();
            PSTAMP(32 + 8 * k + 4);
            float* Dn_c = Dn;
            const float* Ti_c = Ti;
            const unsigned long long neg_c = neg;
            auto idle = [&](auto pc, int wv) {
                constexpr int p = decltype(pc)::value;
                if constexpr (p == 0) {  // the rest of the update's lower triangle
                    if (wv == 1) {
                        persist_diag_block(Dn_c, Ti_c, 1, 1, lane, neg_c);
                        persist_diag_block(Dn_c, Ti_c, 2, 1, lane, neg_c);
                    } else if (wv == 2) {
                        persist_diag_block(Dn_c, Ti_c, 3, 1, lane, neg_c);
                        persist_diag_block(Dn_c, Ti_c, 2, 2, lane, neg_c);
                    } else {
                        persist_diag_block(Dn_c, Ti_c, 3, 2, lane, neg_c);
                        persist_diag_block(Dn_c, Ti_c, 3, 3, lane, neg_c);
                    }
                }
            };
            const bool bad = potrf64_lds<EKF_POTRF_FV>(Dn, Tinv, tid, nullptr, idle);
            unsigned long long neg1 = 0ull;
            PSTAMP(32 + 8 * k + 5);
            if (a.dbg && tid == 0) a.dbg[700 + k] = (long long)__builtin_amdgcn_s_memrealtime();  // (100 MHz, one clock for all XCDs: against the owners' 720 + j)
            // the early look at the next step's flags (tiles (i+1,i) and (i+1,i+1))
            seen = 1;
            if (k + 2 < mb && lane < 2)
                seen = __hip_atomic_load(lane == 0 ? a.fin + (i + 1) * mb + i : a.fin + (i + 1) * mb + (i + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (bad) {  // workgroup-uniform, rare: the updated tile is formed again and factored as U S U^T
                __syncthreads();
                if (k >= kf) load_tile_sc1(Dn, bS, oii, lds, tid);
                else load_tile(Dn, S + oii, lds, tid);
                __syncthreads();
                const f32x16 up = (neg == 0ull) ? mma64(Ti, 1, PLD, Ti, 1, PLD, wr, wc, lane) : mma64_signed(Ti, 1, PLD, Ti, 1, PLD, wr, wc, lane, neg);
#pragma unroll
                for (int q = 0; q < 16; q++) {
                    const int c = mma64_col(wc, lane, q);
                    Dn[c * PLD + r] = Dn[c * PLD + r] - up[q];
                }
                neg1 = potrf64_signed(Dn, Tinv, tid);
            }
            store_tile_sc1<true>(Dn, bL, (unsigned)(i * PB) * (unsigned)ldl + (unsigned)(i * PB), ldl, tid);
            store_inv_sc1(Tinv, bI, (unsigned)(i * PB * PB), tid);
            if (tid == 0) {
                __hip_atomic_store(a.Lsign + i, neg1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (bad) atomicOr(a.info, 1);
            }
            asm volatile("" ::: "memory");  // (the next step's loads are issued behind these stores: it counts on that)
            neg = neg1;
            float* t = Lk;
            Lk = Dn;
            Dn = t;
        }
        persist_publish_wave(a.ready + (mb - 1), lane);
        PSTAMP(32 + 8 * (mb - 1));
        if (a.dbg && tid == 0) a.dbg[897] = (long long)__builtin_amdgcn_s_memrealtime();
        PEXIT();
    }

    // ---------------- a helper: tile (i,j) for the whole sweep (block (I_c, j) of an identity row block c is zero, and stays unused, for j < c) ----
    if (role.kind == ROLE_LEAD || role.kind == ROLE_LEAD_GATHER0) {
        // ---- a transposing workgroup of the fused launch: its 64x64 tile of Wt = (H Sigma)^T (read by the first Joseph GEMM, a
        // later launch: plain stores) and the zero padding columns of G.  It waits for nothing. ----
        if (!compact) gather_body<false>(ga, ga.nb1 + role.n, persist_dyn_lds);
        else if (role.kind == ROLE_LEAD_GATHER0) {
            // compact launch: first the chain's step-0 tile (1, cb), stored write-through and announced like an owner's finished tile
            const int cb = role.a;
            const int m = ga.m_dev ? *ga.m_dev : ga.m;
            GTile t;
            gtile_idx(t, ga, m, 1, cb, mb, a.idb0, tid);
            gtile_pin(t);
            gtile_val(t, ga, m, 1, cb, mb, a.idb0, tid);
            gtile_pinv(t);
            gtile_put(t, Tl, ga, m, 1, cb, mb, a.idb0, tid);
            __syncthreads();
            store_tile_sc1<false>(Tl, bS, (unsigned)(cb * PB) * (unsigned)lds + (unsigned)PB, lds, tid);
            persist_publish(a.fin + 1 * mb + cb, tid);
        }
        if (a.gain) {  // ... and stays: tile (ib, cb) of the gain, formed as its operands come out of the sweep
            const int tb = role.n;
            __syncthreads();
            if (role.a < a.idb0 - mb) {  // (Wt has tiles up to the handle's capacity; the gain only X's row blocks)
                if (a.t2) gain_tile2<true>(a, ga, Ti, Tj, Tl, Tinv, persist_dyn_lds, persist_dyn_lds + PB * PLD, role.a, role.b, tid);
                else gain_tile(a, Ti, Tj, Tl, Tinv, role.a, role.b, tid);
                if (a.dbg && tid == 0 && tb < 104) a.dbg[200 + tb] = (long long)__builtin_amdgcn_s_memrealtime();
            }
        }
        PEXIT();
    }
    const int idb0 = a.idb0;
    if (role.kind == ROLE_GATHER0) {
        // ---- fused launch: the two tiles of the chain's step 0, (1,0) and (1,1), gathered from Sigma by a workgroup each, stored
        // write-through and announced like an owner's finished tile ----
        const int cb = role.a;  // 0: tile (1,0), 1: tile (1,1)
        const int m = ga.m_dev ? *ga.m_dev : ga.m;
        GTile t;
        gtile_idx(t, ga, m, 1, cb, mb, idb0, tid);
        gtile_pin(t);
        gtile_val(t, ga, m, 1, cb, mb, idb0, tid);
        gtile_pinv(t);
        gtile_put(t, Tl, ga, m, 1, cb, mb, idb0, tid);
        __syncthreads();
        store_tile_sc1<false>(Tl, bS, (unsigned)(cb * PB) * (unsigned)lds + (unsigned)PB, lds, tid);
        persist_publish(a.fin + 1 * mb + cb, tid);
        PEXIT();
    }
    const int i = role.a, j = role.b, hidx = role.n;
    const int k0 = (i >= idb0) ? (i - idb0) : 0;     // identity block row c: block (i,k) is zero for k < c
    const int klast = (i == j) ? j - 2 : j - 1;       // a diagonal tile is handed to the chain one step early
    const unsigned oij = (unsigned)(j * PB) * (unsigned)lds + (unsigned)(i * PB);
    float tv[16];                                     // the tile, in the product's accumulator layout, for the whole sweep
    if (fused) {
        // the owner gathers ITS tile of [A; X; I] straight from Sigma (through L_kk's LDS tile into the accumulator layout), and with it
        // the two panel sources of step 0, (i,0) and (j,0): block column 0 exists nowhere but in Sigma
        const int m = ga.m_dev ? *ga.m_dev : ga.m;
        const bool step0 = k0 == 0 && klast >= 0;
        GTile tn, ti_, tj_;
        gtile_idx(tn, ga, m, i, j, mb, idb0, tid);
        if (step0) {
            gtile_idx(ti_, ga, m, i, 0, mb, idb0, tid);
            if (i != j) gtile_idx(tj_, ga, m, j, 0, mb, idb0, tid);
        }
        gtile_pin(tn);
        if (step0) gtile_pin(ti_);
        gtile_val(tn, ga, m, i, j, mb, idb0, tid);
        if (step0) {
            gtile_val(ti_, ga, m, i, 0, mb, idb0, tid);
            if (i != j) gtile_val(tj_, ga, m, j, 0, mb, idb0, tid);
        }
        gtile_pinv(tn);
        gtile_put(tn, Tl, ga, m, i, j, mb, idb0, tid);
        if (step0) {
            gtile_put(ti_, Ti, ga, m, i, 0, mb, idb0, tid);
            if (i != j) gtile_put(tj_, Tj, ga, m, j, 0, mb, idb0, tid);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; q++) tv[q] = Tl[mma64_col(wc, lane, q) * PLD + r];
        __syncthreads();  // (Tl is loaded with L_00 below)
    } else {
#pragma unroll
        for (int q = 0; q < 16; q++) tv[q] = S[oij + (size_t)mma64_col(wc, lane, q) * lds + r];
    }
    // diagnostic stamps of the sub-diagonal tiles' last steps (the tiles the chain waits for)
#define HSTAMP(n)                                                                                                       \
    do {                                                                                                                \
        if (a.dbg && i == j + 1 && i < mb && k == klast && tid == 0) a.dbg[600 + 8 * j + (n)] = (long long)__builtin_amdgcn_s_memtime(); \
    } while (0)
    // ... and of the last step of block column mb-1's owners of X / identity row blocks (scripts/t2_stamps.py): 0 the panel block (i, mb-2) is final
    // in LDS, 1 `fin` is up, 2 `pan` is up -- what the gain and T2 tiles' last two block columns wait for, on the 100 MHz clock
#define OSTAMP(n)                                                                                                       \
    do {                                                                                                                \
        if (a.dbg && tid == 0 && j == mb - 1 && i >= mb && i - mb < 40) a.dbg[904 + 3 * (i - mb) + (n)] = (long long)__builtin_amdgcn_s_memrealtime(); \
    } while (0)
    // an X or identity row block off the diagonal, with the gain formed inside this launch: its panel block (i, j-1) is an operand of the gain and T2
    // tiles and leaves write-through right behind the last step's substitution, with a flag (`pan`) of its own
    const bool early_pan = a.gain && i >= mb && i != j;
    unsigned long long neg = 0ull;
    int k = k0;
    for (; k <= klast; k++) {
        HSTAMP(0);
        // L_kk is out; the two panel sources (i,k), (j,k) are final (block column 0 is the gather's: final from the start)
        // (the chain waits for two tiles per step, (k+2,k+1) and (k+2,k+2), on their owners' last steps: those look often)
        const bool lazy = !(k == klast && i <= j + 1);
        const bool early = a.early_sources && k >= 1;
        // compact launch: an identity row block's first step takes its own diagonal tile (idb0 + c, c) as panel source: the identity, nobody's
        const bool src_ident = compact && k >= 1 && i >= idb0 && i - idb0 == k;
        const int* fin_ik = src_ident ? nullptr : a.fin + i * mb + k;
        if (early) {
            // the panel sources (i,k), (j,k) are final about a third of a chain step before L_kk is: they are in LDS when ready[k] comes
            // up, and only L_kk, its inverses and the sign mask are left for the round trip behind it
            persist_wait(a, nullptr, fin_ik, (i != j) ? a.fin + j * mb + k : nullptr, tid, 1, lazy);
            if (src_ident) identity_tile(Ti, tid);
            else load_tile_sc1(Ti, bS, (unsigned)(k * PB) * (unsigned)lds + (unsigned)(i * PB), lds, tid);
            if (i != j) load_tile_sc1(Tj, bS, (unsigned)(k * PB) * (unsigned)lds + (unsigned)(j * PB), lds, tid);
            persist_wait(a, a.ready + k, nullptr, nullptr, tid, 4, lazy);
        } else if (k >= 1) persist_wait(a, a.ready + k, fin_ik, (i != j) ? a.fin + j * mb + k : nullptr, tid, 4, lazy);
        else if (fused) persist_wait(a, a.ready, nullptr, nullptr, tid, 4, lazy);  // L_00 of this launch
        else __syncthreads();  // (the barrier: the previous step's readers of Ti / Tj / Tl are done)
        HSTAMP(1);
        if (k >= 1 || fused) {  // four requests in flight together: one round trip
            load_tile_sc1(Tl, bL, (unsigned)(k * PB) * (unsigned)ldl + (unsigned)(k * PB), ldl, tid);
            load_inv_sc1(Tinv, bI, (unsigned)(k * PB * PB), tid);
            if (k >= 1 && !early) {  // (fused launch, step 0: the two panel sources were gathered from Sigma at the start)
                if (src_ident) identity_tile(Ti, tid);
                else load_tile_sc1(Ti, bS, (unsigned)(k * PB) * (unsigned)lds + (unsigned)(i * PB), lds, tid);
                if (i != j) load_tile_sc1(Tj, bS, (unsigned)(k * PB) * (unsigned)lds + (unsigned)(j * PB), lds, tid);
            }
            neg = ld_sign_sc1(a.Lsign + k);
        } else {
            load_tile(Tl, L, ldl, tid);
            load_inv(Tinv, a.Linv, tid);
            load_tile(Ti, S + (size_t)i * PB, lds, tid);
            if (i != j) load_tile(Tj, S + (size_t)j * PB, lds, tid);
            neg = a.Lsign[0];
        }
        __syncthreads();
        HSTAMP(2);
        if (i != j)
            tri_solve_fwd2(Ti, Tj, Tl, Tinv, wave, lane);
        else
            tri_solve_fwd(Ti, Tl, Tinv, wave, lane);
        __syncthreads();
        HSTAMP(3);
        if (k == klast) OSTAMP(0);
        if (early_pan && k == klast) {
            // The panel block (i, j-1) is final in Ti: it leaves NOW, write-through, and travels under the product below, which only reads Ti.  Its flag
            // goes up behind the product (every wavefront's wait for its stores, the barrier, one lane).  Nothing follows from `pan` about this
            // owner's finished tile any more: that one is stored and announced (`fin`) later, and whoever reads it waits for `fin`.
            const unsigned od = (unsigned)(klast * PB) * (unsigned)ldl + (unsigned)(i * PB);
            PERSIST_TEST_DELAY(a, 1);
            if (neg != 0ull && i >= idb0) store_tile_signed_sc1(Ti, bL, od, ldl, tid, neg);
            else store_tile_sc1<false>(Ti, bL, od, ldl, tid);
        }
        const float* Bj = (i != j) ? Tj : Ti;
        const f32x16 up = (neg == 0ull) ? mma64(Ti, 1, PLD, Bj, 1, PLD, wr, wc, lane) : mma64_signed(Ti, 1, PLD, Bj, 1, PLD, wr, wc, lane, neg);
#pragma unroll
        for (int q = 0; q < 16; q++) tv[q] = tv[q] - up[q];
        HSTAMP(4);
    }
    k = klast;
    if (early_pan && klast >= k0) {  // the panel block left in front of the last product: announced, in the publishing form, before anything else
        persist_publish(a.pan + i * mb + klast, tid);
        OSTAMP(2);
    }
    // the finished tile goes out once (write-through, whole 128-byte lines through L_kk's LDS tile, free since the
    // substitutions) and is announced
    if (klast >= k0 || fused) {  // (fused launch: a tile without steps -- an identity block -- exists nowhere yet either)
        if (klast < k0) __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; q++) Tl[mma64_col(wc, lane, q) * PLD + r] = tv[q];
        __syncthreads();
        PERSIST_TEST_DELAY(a, 0);
        store_tile_sc1<false>(Tl, bS, oij, lds, tid);
    }
    if ((int)blockIdx.x != a.stall_wg) persist_publish(a.fin + i * mb + j, tid);
    else __syncthreads();
    HSTAMP(5);
    OSTAMP(1);
    if (a.dbg && tid == 0 && i < mb && (i == j + 1 || i == j)) a.dbg[(i == j ? 740 : 720) + j] = (long long)__builtin_amdgcn_s_memrealtime();
    if (klast >= k0 && i != j && !early_pan) {  // the panel block of row block i in block column j-1: read by later launches only
        // (an X or identity row block's, with the gain formed inside this launch, is an operand of the gain and T2 tiles: out already, see the last step)
        float* dst = L + (size_t)klast * PB * ldl + (size_t)i * PB;
        if (neg != 0ull && i >= idb0) store_tile_signed(Ti, dst, ldl, tid, neg);
        else store_tile(Ti, dst, ldl, tid);
    }
    if (a.t2) {
        // round 6: this workgroup's tile is done and nothing else is left for an owner of a launch that forms the gain itself -- it adopts
        // a tile pair of T2 (the first t2_skip owners leave: the launch has a few more workgroups than compute units).  It starts with
        // the block columns that are out already (their `pan` flags are up) and then keeps step with the sweep.
        const int p = a.grid.t2_pair_of(hidx);
        if (a.dbg && tid == 0 && hidx < 8) {
            a.dbg[192 + hidx] = (long long)__builtin_amdgcn_s_memrealtime();
        }
        if (p >= 0) {
            int ta, tb;
            t2_pair(p, ta, tb);
            long long* td = nullptr;  // diagnostic (scripts/t2_stamps.py): the first, a middle and the last pair's block-column times on the 100 MHz clock
            const int np_ = t2_pairs(a.grid.nX);
            if (a.dbg && (p == 0 || p == np_ / 2 || p == np_ - 1)) {
                td = a.dbg + 840 + 16 * (p == 0 ? 0 : p == np_ - 1 ? 2 : 1);
                if (tid == 0) td[14] = (long long)__builtin_amdgcn_s_memrealtime();  // adopted
            }
            t2_tile<true>(a, Ti, Tj, Tl, Tinv, ta, tb, tid, td);
            if (a.dbg && tid == 0 && p < 91) a.dbg[304 + p] = (long long)__builtin_amdgcn_s_memrealtime();
        }
        PEXIT();
    }
    if (j == mb - 1 && i >= mb) {
        // last block column: this row block's panel solve against L_last (was chol_panel_kernel's launch)
        if (i >= idb0 && i - idb0 > j) PEXIT();  // identity block row beyond the last column: block stays zero, unused
        if (a.gain) PEXIT();  // (the gain workgroups solve the last block column's panel blocks themselves: gain_tile)
        persist_wait(a, a.ready + j, nullptr, nullptr, tid, 4, false);  // (its barrier: the tile's store has left Tl)
        load_tile_sc1(Tj, bL, (unsigned)(j * PB) * (unsigned)ldl + (unsigned)(j * PB), ldl, tid);
        load_inv_sc1(Tinv, bI, (unsigned)(j * PB * PB), tid);
        const unsigned long long negl = ld_sign_sc1(a.Lsign + j);
        if (klast < k0) {  // (otherwise the finished tile is in Tl already)
#pragma unroll
            for (int q = 0; q < 16; q++) Tl[mma64_col(wc, lane, q) * PLD + r] = tv[q];
        }
        __syncthreads();
        tri_solve_fwd(Tl, Tj, Tinv, wave, lane);
        __syncthreads();
        if (a.gain) {
            const unsigned od = (unsigned)(j * PB) * (unsigned)ldl + (unsigned)(i * PB);
            if (negl != 0ull && i >= idb0) store_tile_signed_sc1(Tl, bL, od, ldl, tid, negl);
            else store_tile_sc1<false>(Tl, bL, od, ldl, tid);
            persist_publish(a.pan + i * mb + j, tid);
        } else {
            float* dst = L + (size_t)j * PB * ldl + (size_t)i * PB;
            if (negl != 0ull && i >= idb0) store_tile_signed(Tl, dst, ldl, tid, negl);
            else store_tile(Tl, dst, ldl, tid);
        }
    }
    PEXIT();
#undef PEXIT
#undef HSTAMP
#undef OSTAMP
#undef PSTAMP
}

// The gain behind every other sweep of fewer than EKF_SWEEP_SPLIT_MB block columns (per-step sweep, Schur-free): one workgroup per
// 64x64 tile of K, the arithmetic of gain_tile -- the persistent launch and the per-step sweep stay bit-identical end to end.
// (round 5: gain_tile's arithmetic with a block column's two operands requested TWO products ahead, into one of two register sets, the loop
// unrolled by two so that the sets are compile-time: one ahead left 1-2 k cycles of their latency in front of every product.  The same products from
// zero, added in the same ascending order, the same prune: the same bits as gain_tile inside the persistent launch.)
__global__ __launch_bounds__(256) void gain_tiles_kernel(PersistArgs a) {
    __shared__ __attribute__((aligned(16))) float Ti[PB * PLD];
    __shared__ __attribute__((aligned(16))) float Tj[PB * PLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave & 1, wc = wave >> 1;
    const int r = wr * 32 + (lane & 31);
    const int mb = a.mb, ldl = a.ldl;
    const int ib = (int)blockIdx.x / mb, cb = (int)blockIdx.x % mb;
    const int iy = mb + ib, iz = a.idb0 + cb;
    float kv[16];
#pragma unroll
    for (int q = 0; q < 16; q++) kv[q] = 0.f;
    // (scalars, not arrays: hipcc sends a loop-carried float4 array to scratch -- the round-4 form of this kernel did exactly that)
#define GT_DECL(S) float4 ya##S##0, ya##S##1, ya##S##2, ya##S##3, za##S##0, za##S##1, za##S##2, za##S##3;
#define GT_REQ1(S, IT, KB)                                                                                                                    \
    ya##S##IT = *reinterpret_cast<const float4*>(a.L + (size_t)(KB) * PB * ldl + (size_t)iy * PB + (size_t)((tid + IT * 256) >> 4) * ldl + ((tid + IT * 256) & 15) * 4); \
    za##S##IT = *reinterpret_cast<const float4*>(a.L + (size_t)(KB) * PB * ldl + (size_t)iz * PB + (size_t)((tid + IT * 256) >> 4) * ldl + ((tid + IT * 256) & 15) * 4);
#define GT_REQ(S, KB) GT_REQ1(S, 0, KB) GT_REQ1(S, 1, KB) GT_REQ1(S, 2, KB) GT_REQ1(S, 3, KB)
#define GT_PUT1(S, IT)                                                                                        \
    *reinterpret_cast<float4*>(Ti + ((tid + IT * 256) >> 4) * PLD + ((tid + IT * 256) & 15) * 4) = ya##S##IT; \
    *reinterpret_cast<float4*>(Tj + ((tid + IT * 256) >> 4) * PLD + ((tid + IT * 256) & 15) * 4) = za##S##IT;
#define GT_STEP(S, KB)                                                      \
    do {                                                                    \
        __syncthreads();                                                    \
        GT_PUT1(S, 0) GT_PUT1(S, 1) GT_PUT1(S, 2) GT_PUT1(S, 3)             \
        __syncthreads();                                                    \
        if ((KB) + 2 < mb) { GT_REQ(S, (KB) + 2) }                          \
        const f32x16 up = mma64(Ti, 1, PLD, Tj, 1, PLD, wr, wc, lane);      \
        _Pragma("unroll") for (int q = 0; q < 16; q++) kv[q] = kv[q] + up[q]; \
    } while (0)
    GT_DECL(0)
    GT_DECL(1)
    GT_REQ(0, cb)
    if (cb + 1 < mb) { GT_REQ(1, cb + 1) }
    else { ya10 = ya11 = ya12 = ya13 = za10 = za11 = za12 = za13 = make_float4(0.f, 0.f, 0.f, 0.f); }
    for (int kb = cb; kb < mb; kb += 2) {
        GT_STEP(0, kb);
        if (kb + 1 < mb) GT_STEP(1, kb + 1);
    }
#undef GT_DECL
#undef GT_REQ1
#undef GT_REQ
#undef GT_PUT1
#undef GT_STEP
    float* Kt = a.K + (size_t)(cb * PB) * a.ldk + (size_t)ib * PB;
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int c = mma64_col(wc, lane, q);
        Kt[(size_t)c * a.ldk + r] = (fabsf(kv[q]) > EKF_FLUSH_THRESH) ? kv[q] : 0.f;  // .sparseView(SPARSE_THRESH, SPARSE_EPS)
    }
}

// Both behind a per-step sweep in ONE launch (round 6): workgroups 0 .. gain_wgs-1 are gain_tile2's, the tile pairs of T2 follow -- one kernel
// boundary less, and the two sets run side by side (104 + 91 workgroups at N = 256).
__global__ __launch_bounds__(256) void gain2_t2_tiles_kernel(PersistArgs a, GatherArgs ga, int gain_wgs) {
    extern __shared__ float g2_dyn_lds[];  // (requested only to keep a compute unit to one of these matrix-pipe-bound workgroups)
    __shared__ __attribute__((aligned(16))) float Ti[PB * PLD];
    __shared__ __attribute__((aligned(16))) float Tj[PB * PLD];
    __shared__ __attribute__((aligned(16))) float Th[PB * PLD];
    __shared__ float tab[192];
    if ((int)blockIdx.x < gain_wgs) {
        gain_tile2<false>(a, ga, Ti, Tj, nullptr, nullptr, Th, tab, (int)blockIdx.x / a.mb, (int)blockIdx.x % a.mb, threadIdx.x);
    } else {
        int ta, tb;
        t2_pair((int)blockIdx.x - gain_wgs, ta, tb);
        t2_tile<false>(a, Ti, Tj, Th, nullptr, ta, tb, threadIdx.x);
    }
}
