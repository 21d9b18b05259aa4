// motion_model.inc -- the reference's motion model (convolveBaseState, TightlyCoupledEKF.cpp:328-395; convolveFeature, :397-460) and one workgroup's share of
// numericallyLinearizeProcess (:176-325) with the mean propagation (:102-107), as device functions.  Included inside an anonymous namespace by
// ekf_kernels.hip (process(dt), ekfvio_linearize) and by gemm.hip (round 6: inside a device-resident run the update's last GEMM carries the NEXT
// process(dt)'s linearisation in spare workgroups of its launch -- the same text, compiled with the same flags: the same bits).

struct Q4 {
    float w, x, y, z;
};
struct V3 {
    float x, y, z;
};

__device__ inline V3 cross3(const V3& a, const V3& b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// Eigen QuaternionBase::_transformVector: v + w*uv + qv x uv, uv = 2 (qv x v)
__device__ inline V3 qrot(const Q4& q, const V3& v) {
    V3 qv{q.x, q.y, q.z};
    V3 uv = cross3(qv, v);
    uv = {uv.x + uv.x, uv.y + uv.y, uv.z + uv.z};
    V3 c = cross3(qv, uv);
    return {v.x + q.w * uv.x + c.x, v.y + q.w * uv.y + c.y, v.z + q.w * uv.z + c.z};
}
// The reference is an x86-64 build of Eigen with its vectorisation on (CMakeLists.txt:15 overwrites the -msse* flags of
// :9, so plain x86-64: SSE2, no SSE3 / FMA): the three functions below follow that build's rounding order (the CPU
// restatement used by the tests follows the same order by default and measures how far the other builds are away:
// tests/test_oracle_variants_cpu.py, DESIGN.md section 5).
// Vector4f::squaredNorm() over the coefficients (x,y,z,w): a packet of squares reduced by SSE2 predux, (c0+c2)+(c1+c3)
__device__ inline float squared_norm4(const Q4& q) { return (q.x * q.x + q.z * q.z) + (q.y * q.y + q.w * q.w); }
__device__ inline Q4 qinverse(const Q4& q) {
    float n2 = squared_norm4(q);
    if (n2 > 0.f) return {q.w / n2, -q.x / n2, -q.y / n2, -q.z / n2};
    return {0.f, 0.f, 0.f, 0.f};
}
__device__ inline Q4 qnormalized(const Q4& q) {
    float n = sqrtf(squared_norm4(q));
    return {q.w / n, q.x / n, q.y / n, q.z / n};
}
// Geometry_SSE.h quat_product<Architecture::SSE, ., ., float>:
// (a * b.wwww - a.zxyx * b.yzxx) + (+,+,+,-)(a.yzxz * b.zxyz + a.wwwy * b.xyzy)
__device__ inline Q4 qmul(const Q4& a, const Q4& b) {
    Q4 r;
    r.x = (a.x * b.w - a.z * b.y) + (a.y * b.z + a.w * b.x);
    r.y = (a.y * b.w - a.x * b.z) + (a.z * b.x + a.w * b.y);
    r.z = (a.z * b.w - a.y * b.x) + (a.x * b.y + a.w * b.z);
    r.w = (a.w * b.w - a.x * b.x) + (-(a.z * b.z + a.y * b.y));
    return r;
}
__device__ inline float norm3(const V3& v) { return sqrtf(v.x * v.x + (v.y * v.y + v.z * v.z)); }

// dt*vel + 0.5*dt*dt*accel with the 0.5*dt*dt factor evaluated in double (:338, :420)
__device__ inline V3 translation(const V3& vel, const V3& acc, float dt) {
    float h = (float)(0.5 * (double)dt * (double)dt);
    return {dt * vel.x + h * acc.x, dt * vel.y + h * acc.y, dt * vel.z + h * acc.z};
}
// exp(omega dt) (:340-355); sign = -1 is the conjugate built by convolveFeature (:427-440)
__device__ inline Q4 delta_quat(const V3& om, float dt, float sign) {
    float on = norm3(om);
    if (on < 1e-10f) {
        Q4 q{1.f, sign * om.x * dt, sign * om.y * dt, sign * om.z * dt};
        return qnormalized(q);
    }
    float theta = dt * on;
    V3 oh{om.x / on, om.y / on, om.z / on};
    float half = theta / 2;
    float st2 = (float)sin((double)half);
    float ct2 = (float)cos((double)half);
    return {ct2, sign * oh.x * st2, sign * oh.y * st2, sign * oh.z * st2};
}

// convolveBaseState (:328-395)
__device__ inline void convolve_base(const float* last, float dt, float* out) {
    V3 pos{last[0], last[1], last[2]};
    Q4 quat{last[3], last[4], last[5], last[6]};
    V3 vel{last[7], last[8], last[9]};
    V3 om{last[10], last[11], last[12]};
    V3 acc{last[13], last[14], last[15]};
    V3 d = qrot(quat, translation(vel, acc, dt));
    pos = {pos.x + d.x, pos.y + d.y, pos.z + d.z};
    Q4 dq = delta_quat(om, dt, 1.f);
    Q4 dqi = qinverse(dq);
    V3 va{vel.x + dt * acc.x, vel.y + dt * acc.y, vel.z + dt * acc.z};
    vel = qrot(dqi, va);
    acc = qrot(dqi, acc);
    quat = qmul(quat, dq);
    out[0] = pos.x; out[1] = pos.y; out[2] = pos.z;
    out[3] = quat.w; out[4] = quat.x; out[5] = quat.y; out[6] = quat.z;
    out[7] = vel.x; out[8] = vel.y; out[9] = vel.z;
    out[10] = last[10]; out[11] = last[11]; out[12] = last[12];
    out[13] = acc.x; out[14] = acc.y; out[15] = acc.z;
    for (int i = 16; i < EKF_BASE; i++) out[i] = last[i];
}

// The part of convolveFeature that depends on the base state only (:405-446): the inverse
// frame rotation and the rotated translation are shared by all landmarks.
struct BaseMotion {
    Q4 dqi;
    V3 rt;  // dq_inv * translation
};
__device__ inline BaseMotion base_motion(const float* base, float dt) {
    V3 vel{base[7], base[8], base[9]};
    V3 acc{base[13], base[14], base[15]};
    V3 om{base[10], base[11], base[12]};
    BaseMotion bm;
    bm.dqi = delta_quat(om, dt, -1.f);
    bm.rt = qrot(bm.dqi, translation(vel, acc, dt));
    return bm;
}
// convolveFeature (:397-460) given the base-dependent part
__device__ inline V3 convolve_feature(const BaseMotion& bm, float u, float v, float rho) {
    V3 p;
    p.z = (float)(1.0 / (double)rho);
    p.x = u * p.z;
    p.y = v * p.z;
    V3 a = qrot(bm.dqi, p);
    p = {a.x + (-bm.rt.x), a.y + (-bm.rt.y), a.z + (-bm.rt.z)};
    p.x /= p.z;
    p.y /= p.z;
    p.z = (float)(1.0 / (double)p.z);
    return p;
}

__device__ inline float plus_delta(float x) { return (float)((double)x + 1e-3); }
__device__ inline float minus_2delta(float x) { return (float)((double)x - 2 * 1e-3); }
__device__ inline float two_delta() { return (float)(2 * 1e-3); }

struct LinLds {
    float s_base[EKF_BASE];
    BaseMotion s_bm[19];        // 0: unperturbed, 1+2c: col 7+c plus, 2+2c: minus
    float s_hi[16][EKF_BASE];   // base workgroup: convolveBaseState at +delta
    float s_lo[16][EKF_BASE];
    float s_res[LIN_LM][25][3];
};
// Workgroup `blk` of the linearisation at the state mean(e) (e = 0 .. 21 the base state, 22 + 3 f + c landmark f): blk < base_block: landmarks
// LIN_LM blk ..: their B (9 columns) and D (3 columns) blocks and their propagated means; blk == base_block: the 22 x 22 block A and the propagated
// base mean.  256 threads, all of them must call (barriers).
template <class Mean>
__device__ __forceinline__ void linearize_block(Mean mean, int N, float dt, float* FA, float* FB, float* FD, float* mu_next, int blk, int base_block,
                                                LinLds& l, int tid) {
    if (tid < EKF_BASE) l.s_base[tid] = mean(tid);
    __syncthreads();
    const float td = two_delta();
    if (blk == base_block) {
        if (tid < 32) {
            // 32 evaluations of convolveBaseState: column j = 0..15, high and low test points
            const int j = tid >> 1;
            float t[EKF_BASE], o[EKF_BASE];
#pragma unroll
            for (int i = 0; i < EKF_BASE; i++) t[i] = (i == j) ? plus_delta(l.s_base[i]) : l.s_base[i];
            if (tid & 1) {
#pragma unroll
                for (int i = 0; i < EKF_BASE; i++) t[i] = (i == j) ? minus_2delta(t[i]) : t[i];
            }
            convolve_base(t, dt, o);
#pragma unroll
            for (int i = 0; i < EKF_BASE; i++) (tid & 1 ? l.s_lo : l.s_hi)[j][i] = o[i];
        } else if (tid == 32) {
            float o[EKF_BASE];
            convolve_base(l.s_base, dt, o);
#pragma unroll
            for (int i = 0; i < EKF_BASE; i++) mu_next[i] = o[i];
        }
        __syncthreads();
        for (int e = tid; e < EKF_BASE * EKF_BASE; e += 256) {
            const int j = e / EKF_BASE, i = e % EKF_BASE;
            FA[e] = (j < 16) ? (l.s_hi[j][i] - l.s_lo[j][i]) / td : ((i == j) ? 1.f : 0.f);
        }
        return;
    }
    if (tid < 19) {
        float t[EKF_BASE];
#pragma unroll
        for (int i = 0; i < EKF_BASE; i++) t[i] = l.s_base[i];
        if (tid > 0) {
            const int c = 7 + (tid - 1) / 2;
#pragma unroll
            for (int i = 7; i < 16; i++) {
                if (i == c) {
                    t[i] = plus_delta(t[i]);
                    if (((tid - 1) & 1) == 1) t[i] = minus_2delta(t[i]);
                }
            }
        }
        l.s_bm[tid] = base_motion(t, dt);
    }
    __syncthreads();
    const int lm = tid >> 5, e = tid & 31;
    const int f = blk * LIN_LM + lm;
    const bool live = f < N;
    float u = 0.f, v = 0.f, rho = 1.f;
    if (live) {
        u = mean(EKF_BASE + 3 * f);
        v = mean(EKF_BASE + 3 * f + 1);
        rho = mean(EKF_BASE + 3 * f + 2);
    }
    if (live && e < 25) {
        V3 o;
        if (e < 18) {
            o = convolve_feature(l.s_bm[1 + e], u, v, rho);  // column 7 + e/2, plus (even) / minus (odd)  (:223-253)
        } else if (e < 24) {
            // the landmark's own 3x3 block (:262-321): component (e-18)/2, plus then minus
            const int c = (e - 18) >> 1;
            float t0 = u, t1 = v, t2 = rho;
            if (c == 0) t0 = plus_delta(t0);
            if (c == 1) t1 = plus_delta(t1);
            if (c == 2) t2 = plus_delta(t2);
            if (e & 1) {
                if (c == 0) t0 = minus_2delta(t0);
                if (c == 1) t1 = minus_2delta(t1);
                if (c == 2) t2 = minus_2delta(t2);
            }
            o = convolve_feature(l.s_bm[0], t0, t1, t2);
        } else {
            o = convolve_feature(l.s_bm[0], u, v, rho);  // mean propagation with the OLD base state (:102-104)
        }
        l.s_res[lm][e][0] = o.x;
        l.s_res[lm][e][1] = o.y;
        l.s_res[lm][e][2] = o.z;
    }
    __syncthreads();
    if (!live) return;
    if (e < 12) {
        // derivative column e: 0..8 -> state columns 7..15 (FB), 9..11 -> own block (FD)
        float* o = (e < 9) ? (FB + (size_t)f * 27 + e * 3) : (FD + (size_t)f * 9 + (e - 9) * 3);
#pragma unroll
        for (int r = 0; r < 3; r++) o[r] = (l.s_res[lm][2 * e][r] - l.s_res[lm][2 * e + 1][r]) / td;
    } else if (e == 24) {
        mu_next[EKF_BASE + 3 * f] = l.s_res[lm][24][0];
        mu_next[EKF_BASE + 3 * f + 1] = l.s_res[lm][24][1];
        mu_next[EKF_BASE + 3 * f + 2] = l.s_res[lm][24][2];
    }
}
