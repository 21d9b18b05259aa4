// gather_body.inc — the measurement gather of updateWithFeaturePositions (TightlyCoupledEKF.cpp:554-561, :578), shared by
// gather_kernel (ekf_kernels.hip) and gather_potrf_kernel (chol.hip: the same work plus the factorisation of the first
// diagonal tile in one launch).  Included inside each file's anonymous namespace.
//
// A = (H Sigma H^T + R)^T (:559-561, :578), padded with the identity.  The reference hands
// S.transpose() to SimplicialLDLT, which reads the LOWER triangle of what it is given, i.e.
// the UPPER triangle of S.  Sigma is only symmetric to rounding (~1e-6) and S^-1 amplifies
// by 1/lambda_min ~ 5e4, so the choice of triangle is visible at the 1e-4 level: store
// A(r,c) = S(c,r) so that the Cholesky kernels (which read the lower triangle) factor the
// same numbers as the reference.  C = Sigma H^T (columns of Sigma); Wt = (H Sigma)^T (rows
// of Sigma, transposed so that it is state-major).
// A, the identity and C are one thread per element (coalesced along the state index); Wt goes through 64x64
// LDS tiles in extra workgroups of the same launch.
struct GatherArgs {
    const float* P;      // propagated Sigma (column-major, ld)
    int ld, n;
    const int* idx;      // state index of measurement row c
    const float* Rm;     // (R(c,c), R(c^1,c)) per measurement row
    int m, m_pad, n_pad;
    const int* m_dev;    // non-null: the true row count lives on the device (m is then the upper bound 2N)
    float* Saug;         // [A; C; I], column c at Saug + c*lda
    int lda;
    float* Wt;           // (H Sigma)^T, state-major, plus row n = -(z - H mu)
    const float* zrow;
    const float* mu;
    float* G;            // padding columns are zeroed here
    int gx, nb1;         // element workgroups: gx per GC*GCI columns, nb1 in total; then the Wt tiles
    int* zero_words;     // gather_potrf_kernel: the persistent sweep's flags, zeroed here for the launch behind it (or null)
    int n_zero;
};

// (GC, GCI: plan.h -- the plan counts these workgroups too)
// S(c,r) = Sigma(idx[c], idx[r]) + R(c,r), identity outside the measured block: element (r,c) of A = S^T
__device__ __forceinline__ float gather_a_elem(float sigma_cr, int r, int c, int m, float rd, float ro) {
    if (r < m && c < m) {
        float v = sigma_cr;
        if (r == c)
            v = v + rd;
        else if ((r ^ 1) == c)
            v = v + ro;  // R(c,r): the off-diagonal element of column r
        return v;
    }
    return (r == c) ? 1.f : 0.f;
}

// WT: the augmented matrix leaves write-through (agent scope): the fused launch (chol_persist.inc) hands it to other workgroups of
// the SAME launch; the other outputs (Wt, G's padding) are read by later launches only
template <bool WT>
__device__ __forceinline__ void gather_st(float* p, float v) {
    if constexpr (WT) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}
template <bool WT = false>
__device__ __forceinline__ void gather_body(const GatherArgs& a, int block, float* tile /* 64*65 floats of LDS */) {
    const float* __restrict__ P = a.P;
    const int* __restrict__ idx = a.idx;
    const int ld = a.ld, n = a.n, m = a.m_dev ? *a.m_dev : a.m, m_pad = a.m_pad, n_pad = a.n_pad, lda = a.lda;
    float* Saug = a.Saug;
    if (block >= a.nb1) {
        // ---- Wt = (H Sigma)^T: Wt(i, c) = Sigma(idx[c], i) = P[i*ld + idx[c]] ----
        // For a fixed i the wanted elements are (nearly) contiguous in c, but Wt is contiguous in i: a 64x64 tile
        // goes through LDS so that both the reads (lanes along c) and the writes (lanes along i) are coalesced.
        // (Read straight, with lanes along i, every lane touches its own 64-B sector: 26 MB of sector traffic
        // for 1.6 MB of data, the bulk of this kernel's time.)
        const int tb = block - a.nb1, tiles_c = m_pad / 64;
        const int c0 = (tb % tiles_c) * 64, i0 = (tb / tiles_c) * 64;
        const int l64 = threadIdx.x & 63, q4 = threadIdx.x >> 6;
        const int c = c0 + l64;
        const int sc = (c < m) ? idx[c] : -1;
        float wv[16];  // all 16 loads in flight before the first LDS write
        const int scl = max(sc, 0);
#pragma unroll
        for (int ps = 0; ps < 16; ps++) {
            const int i = min(i0 + q4 + 4 * ps, n - 1);  // clamped: unconditional loads issue as one batch
            wv[ps] = P[(size_t)i * ld + scl];
        }
#pragma unroll
        for (int ps = 0; ps < 16; ps++) asm volatile("" : "+v"(wv[ps]));
        // extra row n: -(z - H mu) (:554-555), so that the Joseph-1 GEMM yields K*y in column n
        const bool has_n = (n >= i0 && n < i0 + 64);
        const float ny = (has_n && sc >= 0) ? -(a.zrow[c] - a.mu[sc]) : 0.f;
#pragma unroll
        for (int ps = 0; ps < 16; ps++) {
            const int ii = q4 + 4 * ps;
            float w = (sc >= 0 && i0 + ii < n) ? wv[ps] : 0.f;
            if (i0 + ii == n) w = ny;
            tile[ii * 65 + l64] = w;
        }
        __syncthreads();
        const int i = i0 + l64;
#pragma unroll
        for (int ps = 0; ps < 16; ps++) {
            const int cc = q4 + 4 * ps, cw = c0 + cc;
            if (i < ld) {
                a.Wt[(size_t)cw * ld + i] = tile[l64 * 65 + cc];
                if (cw >= m) a.G[(size_t)cw * ld + i] = 0.f;  // padding columns of G stay zero (also done below: the fused launch runs only this branch)
            }
        }
        return;
    }
    // ---- A = (H Sigma H^T + R)^T, the identity block and C = Sigma H^T: one thread per row, GC columns at a time
    // (the row's own index lookups are shared by the columns and all their loads are in flight together) ----
    const int x = (block % a.gx) * blockDim.x + threadIdx.x;
    const int r = x;
    const int ir = (r < m) ? idx[r] : 0;
    const float rd = (r < m) ? a.Rm[2 * r] : 0.f, ro = (r < m) ? a.Rm[2 * r + 1] : 0.f;
    // all GC*GCI columns of the workgroup at once: their index lookups, then their 2*GC*GCI loads, are in flight together
    // (m_pad is a multiple of 64, so every column of a launched workgroup exists)
    constexpr int GCT = GC * GCI;
    const int cbase = (block / a.gx) * GCT;
    int scv[GCT];
    float sv[GCT], cv[GCT];
#pragma unroll
    for (int q = 0; q < GCT; q++) scv[q] = (cbase + q < m) ? idx[cbase + q] : 0;
#pragma unroll
    for (int q = 0; q < GCT; q++) {
        const int c = cbase + q;
        sv[q] = (x < m_pad && r < m && c < m) ? P[(size_t)ir * ld + scv[q]] : 0.f;  // Sigma(idx[c], idx[r]) = S(c,r)
        cv[q] = (x < ld && c < m && x < n) ? P[(size_t)scv[q] * ld + x] : 0.f;    // Sigma(i, idx[c])
    }
#pragma unroll
    for (int q = 0; q < GCT; q++) {
        asm volatile("" : "+v"(sv[q]));
        asm volatile("" : "+v"(cv[q]));
    }
#pragma unroll
    for (int q = 0; q < GCT; q++) {
        const int c = cbase + q;
        if (x < m_pad) {
            gather_st<WT>(Saug + (size_t)c * lda + r, gather_a_elem(sv[q], r, c, m, rd, ro));
            gather_st<WT>(Saug + (size_t)c * lda + m_pad + n_pad + r, (r == c) ? 1.f : 0.f);  // identity block
        }
        if (x < ld) {
            if (x < n_pad) gather_st<WT>(Saug + (size_t)c * lda + m_pad + x, cv[q]);
            if (c >= m) a.G[(size_t)c * ld + x] = 0.f;   // padding columns of G stay zero
        }
    }
}

static GatherArgs make_gather_args(ekfvio_filter* f, const UpdatePlan& p) {
    const int m_pad = p.m_pad;
    GatherArgs a;
    a.P = f->P;
    a.ld = f->ldp;
    a.n = f->n;
    a.idx = f->idx;
    a.Rm = f->Rm;
    a.m = p.m;
    a.m_dev = p.m_on_device ? f->info + 2 : nullptr;
    a.m_pad = m_pad;
    a.n_pad = p.n_pad;
    a.Saug = f->Saug;
    a.lda = f->ld_aug;
    a.Wt = f->Wt;
    a.zrow = f->yres;
    a.mu = f->mu;
    a.G = f->Gm;
    a.gx = gather_gx(f->ldp, m_pad);
    a.nb1 = gather_element_wgs(f->ldp, m_pad);
    a.zero_words = nullptr;
    a.n_zero = 0;
    return a;
}
