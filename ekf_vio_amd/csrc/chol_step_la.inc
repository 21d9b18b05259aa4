// chol_step_la.inc -- the split sweep (mb >= EKF_SWEEP_SPLIT_MB block columns: panel blocks solved ONCE and stored) as tile tasks, one
// launch per block step (chol_step_la_kernel, rounds 2-3).  Included inside chol.hip's anonymous namespace.
// (Round 4 also drove the same tasks from ONE persistent launch -- chain workgroup, a row worker per row block, far-tile owners, flags:
// measured slower in nine schedules, profiles/r04_persistent_split_sweep_experiment.txt; that driver and the write-through / agent-scope
// variants of the tasks it needed live in scripts/experiments/chol_persist_la.inc.txt since round 5.)
//
// The tasks of block step ("round") l:
//   near tiles  (i, l+1), every row block i below the diagonal and all extra rows: step l-1's update from the STORED
//               panel blocks L_i,l-1, L_l+1,l-1, then step l's from panel blocks the tile solves itself (L_il = A_il
//               L_ll^-T, stored for the later rounds; A_il is final: column l was the near column of round l-1);
//               tile (l+1, l+1) is the chain: updated, factored, stored, as in chol_step_kernel;
//   far tiles   (i, j), j = l+2, l+4, ...: steps l-2 AND l-1 from stored panel blocks.  A column is visited every second
//               round and takes two steps per visit, so the trailing matrix -- whose read-modify-write out of Infinity
//               Cache is what bounds the far work -- is read and written half as often for the same arithmetic.  Column
//               j's last far visit is round j-2 (steps j-4, j-3); round j-1 is its near visit (steps j-2, j-1).
// Every tile receives its updates in ascending step order, one subtraction per step: bit-identical to the two-launch form
// (chol_panel_kernel + chol_step_kernel<false>) and the same in both drivers below.  Far tiles need no solve, near tiles fetch the
// solve's operands into registers and then re-use L_ll's LDS tile for their second row block, so a workgroup stays at two LDS
// tiles (four workgroups per compute unit).
//
//
// One launch per round: a round costs the chain tile's latency plus a kernel boundary -- 11 us at N = 1024 even where the far work is a
// fraction of that (rocprofv3: 31 launches of 10 - 19 us, ~450 us).

struct LaArgs {
    float* S;           // augmented matrix [A; X; I], ld lds
    int lds;
    float* L;           // factor / panel blocks out, ld ldl
    int ldl;
    float* Linv;        // 16x16 inverse blocks per block column
    int mb, rb, idb0;   // block columns; extra row blocks (X then I); first identity row block
    int* info;
    unsigned long long* Lsign;
};

// a 64x64 tile (leading dimension ld) requested into four float4 of every thread, and written to an LDS tile later
__device__ __forceinline__ void tile_request(float4& v0, float4& v1, float4& v2, float4& v3, const float* G, int ld, int tid) {
    const float* g = G + (size_t)(tid >> 4) * ld + (tid & 15) * 4;
    v0 = *reinterpret_cast<const float4*>(g);
    v1 = *reinterpret_cast<const float4*>(g + (size_t)16 * ld);
    v2 = *reinterpret_cast<const float4*>(g + (size_t)32 * ld);
    v3 = *reinterpret_cast<const float4*>(g + (size_t)48 * ld);
}
__device__ __forceinline__ void tile_commit(float* T, float4 v0, float4 v1, float4 v2, float4 v3, int tid) {
    float* t = T + (tid >> 4) * PLD + (tid & 15) * 4;
    *reinterpret_cast<float4*>(t) = v0;
    *reinterpret_cast<float4*>(t + 16 * PLD) = v1;
    *reinterpret_cast<float4*>(t + 32 * PLD) = v2;
    *reinterpret_cast<float4*>(t + 48 * PLD) = v3;
}

// One tile task of round l: tile (i,j), near (j == l+1) or far (j = l+2, l+4, ...).  256 threads; Ti, Tj, Tinv: the workgroup's LDS.
__device__ __forceinline__ void la_tile(const LaArgs& a, int l, bool near, int i, int j, float* Ti, float* Tj, float* Tinv, int tid) {
    float* const S = a.S;
    float* const L = a.L;
    float* const Linv = a.Linv;
    const int lds = a.lds, ldl = a.ldl;
    const int mb = a.mb, idb0 = a.idb0;
    unsigned long long* const Lsign = a.Lsign;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave & 1, wc = wave >> 1;
    const int ic = i - idb0;                       // identity block row c: block (i,k) is zero for k < c
    const bool has0 = l >= 1 && !(ic > l - 1);      // step l-1 reaches this row block
    const bool has1 = near && !(ic > l);            // step l does
    if (!has0 && !has1) return;
    const bool chain = near && i == j;
    unsigned long long neg0 = 0ull, neg1 = 0ull;
    float* Sij = S + (size_t)j * PB * lds + (size_t)i * PB;
    const int rw = wr * 32 + (lane & 31);
    (void)mb;
    f32x16 up0;
#pragma unroll
    for (int q = 0; q < 16; q++) up0[q] = 0.f;

    if (!near) {  // far tile: steps l-2 (if it reaches this row block) and l-1 from stored panel blocks
        const bool hasa = l >= 2 && !(ic > l - 2);
        f32x16 upa;
#pragma unroll
        for (int q = 0; q < 16; q++) upa[q] = 0.f;
        if (hasa) {
            unsigned long long nega = sign_mask_request(Lsign + l - 2);
            load_tile(Ti, L + (size_t)(l - 2) * PB * ldl + (size_t)i * PB, ldl, tid);
            if (i != j) load_tile(Tj, L + (size_t)(l - 2) * PB * ldl + (size_t)j * PB, ldl, tid);
            __syncthreads();
            nega = sign_mask_value(nega);
            const float* Ba = (i != j) ? Tj : Ti;
            upa = (nega == 0ull) ? mma64(Ti, 1, PLD, Ba, 1, PLD, wr, wc, lane) : mma64_signed(Ti, 1, PLD, Ba, 1, PLD, wr, wc, lane, nega);
            __syncthreads();
        }
        neg0 = sign_mask_request(Lsign + l - 1);
        load_tile(Ti, L + (size_t)(l - 1) * PB * ldl + (size_t)i * PB, ldl, tid);
        if (i != j) load_tile(Tj, L + (size_t)(l - 1) * PB * ldl + (size_t)j * PB, ldl, tid);
        __syncthreads();
        neg0 = sign_mask_value(neg0);
        const float* Bj = (i != j) ? Tj : Ti;
        float tv[16];  // the target tile's round trip runs under the product
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int c = mma64_col(wc, lane, q);
            tv[q] = Sij[(size_t)c * lds + rw];
        }
        const f32x16 up = (neg0 == 0ull) ? mma64(Ti, 1, PLD, Bj, 1, PLD, wr, wc, lane) : mma64_signed(Ti, 1, PLD, Bj, 1, PLD, wr, wc, lane, neg0);
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int c = mma64_col(wc, lane, q);
            const float v0 = hasa ? tv[q] - upa[q] : tv[q];
            Sij[(size_t)c * lds + rw] = v0 - up[q];
        }
        return;
    }

    if (!chain) {
        // ---- near tile below the diagonal / extra row ----
        TriOps ops;
        if (has0) {
            neg0 = sign_mask_request(Lsign + l - 1);
            load_tile(Ti, L + (size_t)(l - 1) * PB * ldl + (size_t)i * PB, ldl, tid);
            load_tile(Tj, L + (size_t)(l - 1) * PB * ldl + (size_t)j * PB, ldl, tid);
            __syncthreads();
            neg0 = sign_mask_value(neg0);
            up0 = (neg0 == 0ull) ? mma64(Ti, 1, PLD, Tj, 1, PLD, wr, wc, lane) : mma64_signed(Ti, 1, PLD, Tj, 1, PLD, wr, wc, lane, neg0);
            __syncthreads();
        }
        // L_ll and its inverses -> the solve's operands in registers; then the two row blocks take the tiles' place
        neg1 = sign_mask_request(Lsign + l);
        load_tile(Tj, L + (size_t)l * PB * ldl + (size_t)l * PB, ldl, tid);
        load_inv(Tinv, Linv + (size_t)l * PB * PB, tid);
        __syncthreads();
        neg1 = sign_mask_value(neg1);
        tri_solve_preload(ops, Tj, Tinv, lane);
        tri_solve_pin(ops);
        __syncthreads();
        load_tile(Ti, S + (size_t)l * PB * lds + (size_t)i * PB, lds, tid);
        load_tile(Tj, S + (size_t)l * PB * lds + (size_t)j * PB, lds, tid);
        __syncthreads();
        {
            float* const tt[2] = {Ti, Tj};
            f32x4 x[2][4];
            tri_solve_load_x<2>(x, tt, wave, lane);
            tri_solve_run<2>(x, tt, ops, wave, lane);
        }
        __syncthreads();
        // unsigned: read back as an operand (sign_irows_kernel puts the identity rows' signs on behind the sweep)
        store_tile(Ti, L + (size_t)l * PB * ldl + (size_t)i * PB, ldl, tid);
        float tv[16];
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int c = mma64_col(wc, lane, q);
            tv[q] = Sij[(size_t)c * lds + rw];
        }
        const f32x16 up1 = (neg1 == 0ull) ? mma64(Ti, 1, PLD, Tj, 1, PLD, wr, wc, lane) : mma64_signed(Ti, 1, PLD, Tj, 1, PLD, wr, wc, lane, neg1);
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int c = mma64_col(wc, lane, q);
            const float v0 = has0 ? tv[q] - up0[q] : tv[q];
            Sij[(size_t)c * lds + rw] = v0 - up1[q];
        }
        return;
    }

    // ---- the chain: tile (l+1, l+1) ----
    // everything it reads from memory is requested at once: the stored block L_j,l-1 -> Ti, L_ll -> Tj (stays: i == j
    // leaves the second row-block tile unused), and A_jl into registers, written to Ti once step l-1's product has read it
    if (has0) neg0 = sign_mask_request(Lsign + l - 1);
    neg1 = sign_mask_request(Lsign + l);
    float4 ar0, ar1, ar2, ar3;  // (scalars: a float4 array went to scratch, a memory round trip of its own on the chain)
    tile_request(ar0, ar1, ar2, ar3, S + (size_t)l * PB * lds + (size_t)j * PB, lds, tid);
    float tgt[16];
    auto request_target = [&]() {  // the target tile: requested before the products, used behind them (see chol_step_kernel)
        const unsigned off0 = ((unsigned)(wc * 32 + 4 * (lane >> 5)) * (unsigned)lds + (unsigned)rw) * 4u;
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const unsigned off = off0 + (unsigned)((q & 3) + 8 * (q >> 2)) * (unsigned)lds * 4u;
            tgt[q] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(Sij) + off);
        }
    };
    if (has0) load_tile(Ti, L + (size_t)(l - 1) * PB * ldl + (size_t)j * PB, ldl, tid);
    load_tile(Tj, L + (size_t)l * PB * ldl + (size_t)l * PB, ldl, tid);
    load_inv(Tinv, Linv + (size_t)l * PB * PB, tid);
    __syncthreads();
    if (has0) neg0 = sign_mask_value(neg0);
    neg1 = sign_mask_value(neg1);
    if (has0) {
        up0 = (neg0 == 0ull) ? mma64(Ti, 1, PLD, Ti, 1, PLD, wr, wc, lane) : mma64_signed(Ti, 1, PLD, Ti, 1, PLD, wr, wc, lane, neg0);
        __syncthreads();
    }
    tile_commit(Ti, ar0, ar1, ar2, ar3, tid);
    __syncthreads();
    tri_solve_fwd(Ti, Tj, Tinv, wave, lane);  // L_jl = A_jl L_ll^-T
    __syncthreads();
    request_target();
    const f32x16 up1 = (neg1 == 0ull) ? mma64(Ti, 1, PLD, Ti, 1, PLD, wr, wc, lane) : mma64_signed(Ti, 1, PLD, Ti, 1, PLD, wr, wc, lane, neg1);
    float* Tl = Tj;  // every wavefront is past its substitution (barrier above): L_ll's tile takes the updated diagonal tile
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int c = mma64_col(wc, lane, q);
        const float v0 = has0 ? tgt[q] - up0[q] : tgt[q];
        Tl[c * PLD + rw] = v0 - up1[q];
    }
    __syncthreads();
    float* Ldst = L + (size_t)j * PB * ldl + (size_t)j * PB;
    float* Idst = Linv + (size_t)(l + 1) * PB * PB;
    float* Pdst = L + (size_t)l * PB * ldl + (size_t)j * PB;
    const float* Tl_c = Tl;
    const float* Ti_c = Ti;
    const float* Tinv_c = Tinv;
    auto idle = [&](auto pc, int wv) {  // stores under the pivot chain (see chol_step_kernel)
        constexpr int p = decltype(pc)::value;
        if constexpr (p == 2) {
            if (wv >= 2) store_cols<0, 32, 128, true>(Tl_c, Ldst, ldl, tid - 128);
        } else if constexpr (p == 3) {
            store_cols<32, 16, 192, true>(Tl_c, Ldst, ldl, tid - 64);
            store_inv_blocks(Tinv_c, Idst, 0, tid - 64);
            store_cols<0, 64, 192, false>(Ti_c, Pdst, ldl, tid - 64);
        }
    };
    const bool bad = potrf64_lds<EKF_POTRF_FV>(Tl, Tinv, tid, nullptr, idle);
    unsigned long long negn = 0ull;
    if (bad) {  // workgroup-uniform, rare: the updated tile is formed again and factored as U S U^T
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int c = mma64_col(wc, lane, q);
            const float v0 = has0 ? Sij[(size_t)c * lds + rw] - up0[q] : Sij[(size_t)c * lds + rw];
            Tl[c * PLD + rw] = v0 - up1[q];
        }
        negn = potrf64_signed(Tl, Tinv, tid);
        store_tile_lower(Tl, Ldst, ldl, tid);
        store_inv(Tinv, Idst, tid);
    } else {
        store_cols<48, 16, 256, true>(Tl_c, Ldst, ldl, tid);
        if (tid < 64) store_inv_blocks(Tinv_c, Idst, 3, tid);
    }
    if (tid == 0) {
        Lsign[l + 1] = negn;
        if (bad) atomicOr(a.info, 1);
    }
}

// One launch per round: workgroup t of launch l takes task t of the round (near tiles first, the chain is task 0).
// Round 6, which tiles and in what order:
//   * identity row blocks that the round's steps do not reach yet (block row c of the identity rows is zero left of block column c) are not
//     enumerated at all -- they were a third of the early rounds' workgroups (1 454 -> 1 005 in round 2), dispatched to return at once;
//   * far tiles are enumerated ROW by row and every XCD takes one contiguous run of that list (workgroups are dealt round-robin to the eight
//     XCDs by block index): a run of ~14 row blocks with all ~15 far columns shares ~1 MB of stored panel blocks in ITS L2, where the
//     column-by-column order had every XCD read every row block of both panel columns (3.6 MB against 4 MB of L2).
//   Together: 461 -> 449 us for the 31 rounds at N = 1024 (rocprofv3, same visit).  What a middle round lasts (17 us with 1 000 tiles, 15 us with
//   600) is NOT the far work: profiles/r06_la_sweep_experiments.txt.
// The same tiles receive the same updates in the same order: the same bits.
__host__ __device__ inline int la_near_tasks(int mb, int idb0, int rb, int l) {
    const int nX = idb0 - mb, nI = mb + rb - idb0;
    return (mb - 1 - l) + nX + min(l + 1, nI);  // chain + A rows below it, X rows, identity rows 0 .. l
}
__host__ __device__ inline int la_far_tasks(int mb, int idb0, int rb, int l) {
    if (l < 1 || l + 2 >= mb) return 0;
    const int nX = idb0 - mb, nI = mb + rb - idb0;
    const int nA = mb - (l + 2);            // A rows l+2 .. mb-1; row l+2+k has k/2 + 1 far columns (l+2, l+4, ... <= the row)
    const int nf = (mb - 1 - (l + 2)) / 2 + 1;
    const int totA = (nA & 1) ? ((nA + 1) / 2) * ((nA + 1) / 2) : (nA / 2) * (nA / 2 + 1);
    return totA + (nX + min(l, nI)) * nf;   // identity rows 0 .. l-1
}
__global__ __launch_bounds__(256, 4) void chol_step_la_kernel(LaArgs a, int l) {
    __shared__ __attribute__((aligned(16))) float Ti[PB * PLD];
    __shared__ __attribute__((aligned(16))) float Tj[PB * PLD];
    __shared__ float Tinv[INV_LDS];
    const int mb = a.mb, rb = a.rb, idb0 = a.idb0;
    const int r = mb - 1 - l;       // block columns right of l
    const int nnear = la_near_tasks(mb, idb0, rb, l);
    int t = blockIdx.x, i, j;
    const bool near = t < nnear;
    if (near) {
        j = l + 1;
        i = (t < r) ? l + 1 + t : mb + (t - r);  // (X rows, then identity rows 0 .. l: contiguous behind the A rows)
    } else {
        const int T = (int)gridDim.x - nnear, Lf = t - nnear;
        const int bq = T >> 3, br = T & 7, x = Lf & 7;
        int s = x * bq + min(x, br) + (Lf >> 3);  // XCD x: the x-th contiguous run of the row-major list
        const int j0 = l + 2;
        const int nA = mb - j0;
        const int nf = (mb - 1 - j0) / 2 + 1;
        const int totA = (nA & 1) ? ((nA + 1) / 2) * ((nA + 1) / 2) : (nA / 2) * (nA / 2 + 1);
        if (s < totA) {
            int k = 0;
            while (s >= k / 2 + 1) {
                s -= k / 2 + 1;
                k++;
            }
            i = j0 + k;
            j = j0 + 2 * s;
        } else {
            s -= totA;
            const int row = s / nf;   // X rows, then identity rows 0 .. l-1
            i = mb + row;
            j = j0 + 2 * (s - row * nf);
        }
    }
    la_tile(a, l, near, i, j, Ti, Tj, Tinv, (int)threadIdx.x);
}
