// ekf_vio_amd/csrc/frame.hip — the frame loop: ekfvio_step_image and what it publishes.
//
// ekfvio_step_image orchestrates one frame of EKFVIO::addFrame: process(dt), the frame's ingest and the tracker (klt.hip), the update
// (ekf_kernels.hip, chol.hip, gemm.hip), the replenishment (fast.hip), the removal of lost landmarks (remove.hip) and the frame's
// outputs, enqueued back to back with ONE host wait at the end (read_status / settle_update, api.hip).  The outputs -- odometry and
// point cloud -- are written by frame_outputs_kernel into pinned host memory together with the status word; ekfvio_get_points is the
// getter that launches points_kernel when they are not fresh.  The covariances of those outputs (include/ekfvio.h) are formed here too:
// by the getters' own kernels, or, with ekfvio_set_output_covariance, by frame_outputs_kernel with everything else.
#include <string.h>

#include "common.h"
#include "points.h"

namespace {

// (points_one, the point of one landmark: points.h)
// host_word != nullptr (single-workgroup launches only): the kernel publishes the status word itself behind its writes
__global__ void points_kernel(const float* __restrict__ mu, int N, const uint8_t* __restrict__ img, int pitch, int w, int h,
                              float fx, float fy, float cx, float cy, float* __restrict__ xyz, float* __restrict__ intensity,
                              const int* __restrict__ info, int* host_word, int seq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) points_one(mu, i, img, pitch, w, h, fx, fy, cx, cy, xyz, intensity);
    if (host_word) {
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) publish_host_words(host_word, info, 0, seq);
    }
}

// ---- covariances of the outputs (include/ekfvio.h, "covariances of the published outputs": the lines there are the specification, the
// functions below are those lines; fp32, no contraction, sums ascending and left-associated) ------------------------------------------
// S(i,j): Sigma's lower-triangle element
__device__ inline float cov_S(const float* __restrict__ P, int ld, int i, int j) {
    const int r = i > j ? i : j, c = i > j ? j : i;
    return P[(size_t)c * ld + r];
}
// Row r of J = 2 [[-qx, qw, -qz, qy], [-qy, qz, qw, -qx], [-qz, -qy, qx, qw]] (columns w, x, y, z); compiled for the host too
// (ekfvio_rotation_error_jacobian).  Selections, not an indexed table: a lane's row stays in registers
__host__ __device__ inline void rot_err_jacobian_row(const float* q, int r, float* Jr) {
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    Jr[0] = 2.f * -(r == 0 ? x : r == 1 ? y : z);
    Jr[1] = 2.f * (r == 0 ? w : r == 1 ? z : -y);
    Jr[2] = 2.f * (r == 0 ? -z : r == 1 ? w : x);
    Jr[3] = 2.f * (r == 0 ? y : r == 1 ? -x : w);
}
// T[3+r][j] of the specification from row r of J
__device__ inline float cov_T(const float* __restrict__ P, int ld, const float* Jr, int j) {
    return ((Jr[0] * cov_S(P, ld, 3, j) + Jr[1] * cov_S(P, ld, 4, j)) + Jr[2] * cov_S(P, ld, 5, j)) + Jr[3] * cov_S(P, ld, 6, j);
}
// Element e (0 .. 71) of out72 = pose_cov[36], twist_cov[36]: one lane per element; the lane of (a,b) forms the lower triangle's
// element (max, min), so both halves hold the same bits
__device__ inline void odom_cov_one(const float* __restrict__ mu, const float* __restrict__ P, int ld, int e, float* __restrict__ out72) {
    const int blk = e / 36, k = e - 36 * blk, r0 = k / 6, c0 = k - 6 * r0;
    const int a = r0 > c0 ? r0 : c0, b = r0 > c0 ? c0 : r0;
    float v;
    if (blk == 1) {
        v = cov_S(P, ld, 7 + a, 7 + b);
    } else if (a < 3) {
        v = cov_S(P, ld, a, b);
    } else {
        float Ja[4], Jb[4];
        rot_err_jacobian_row(mu + 3, a - 3, Ja);
        if (b < 3) {
            v = cov_T(P, ld, Ja, b);
        } else {
            rot_err_jacobian_row(mu + 3, b - 3, Jb);
            v = ((cov_T(P, ld, Ja, 3) * Jb[0] + cov_T(P, ld, Ja, 4) * Jb[1]) + cov_T(P, ld, Ja, 5) * Jb[2]) + cov_T(P, ld, Ja, 6) * Jb[3];
        }
    }
    out72[e] = v;
}
// (points_cov_one, landmark i's 3x3: points.h)
// The on-demand road (ekfvio_get_odometry_covariance / ekfvio_get_points_covariance), in the shape of points_kernel.
// One workgroup; it publishes the status word itself
__global__ __launch_bounds__(128) void odom_cov_kernel(const float* __restrict__ mu, const float* __restrict__ P, int ld, float* __restrict__ out72,
                                                       const int* __restrict__ info, int* host_word, int seq) {
    if (threadIdx.x < 72) odom_cov_one(mu, P, ld, threadIdx.x, out72);
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) publish_host_words(host_word, info, 0, seq);
}
// host_word != nullptr (single-workgroup launches only): as points_kernel
__global__ __launch_bounds__(256) void points_cov_kernel(const float* __restrict__ mu, const float* __restrict__ P, int ld, int N,
                                                         float* __restrict__ out9N, const int* __restrict__ info, int* host_word, int seq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) points_cov_one(mu, P, ld, i, out9N);
    if (host_word) {
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) publish_host_words(host_word, info, 0, seq);
    }
}

// The last kernel of a frame (ekfvio_step_image): what the node publishes after addFrame -- publishOdometry's slices of
// base_mu and publishPoints' cloud (EKFVIO.cpp:444-518) -- written into pinned host memory TOGETHER with the status word
// the host is waiting for anyway.  ekfvio_get_odometry / ekfvio_get_points then cost a memcpy instead of a launch and a
// wait each (the node's loop with outputs: 164 -> 140 us per frame at the node's defaults).  One workgroup; the number of
// landmarks is N_old plus what the replenishment just added (added_dev, may be null).
// Layout of out: base_mu[22], xyz[3 N], intensity[N]; the landmarks' ids and birth stamps in a region of their own (FrameIdsOut).
// Pcol != null (round 4): launched BETWEEN the update's two Joseph GEMMs.  The mean update mu += K y, quaternion renormalised, is the
// second GEMM's (gemm.hip, mode 2, :600-609) from K y in column n of P, which the first one has just left there: the same sums are
// formed here (into LDS, mu itself is not touched), so the frame's outputs and status reach the host while the second GEMM still runs
// -- the host's next frame (copying the image, ~15 us) starts that much earlier.  Same values, same bits as behind the update.
// cov.S != null (ekfvio_set_output_covariance; never with Pcol / Kyp: Sigma' does not exist in front of the last GEMM): pose_cov[36], twist_cov[36] and
// cov[9 N] of the frame's FINAL Sigma go out too, at cov.out.  Behind a removal that took landmarks out that Sigma is the buffer the removal wrote.
struct FrameCovOut {
    const float* S = nullptr;          // Sigma (null: no covariances, today's path)
    const float* S_removed = nullptr;  // ... or this one where removed_dev[1] > 0 (remove.hip: words[1], the removed count)
    const int* removed_dev = nullptr;
    int ld = 0;
    float* out = nullptr;
};
// The landmarks' ids and birth stamps (include/ekfvio.h, "landmark identities") go out with the cloud, rows as the cloud's: behind a removal
// the arrays are compacted already (in place, remove.hip), and a frame that publishes early can neither add nor remove.
struct FrameIdsOut {
    const int64_t* id = nullptr;
    const double* born = nullptr;
    int64_t* out_id = nullptr;   // h_out at out_ids_offset, [max_features]
    double* out_born = nullptr;  // ... behind it
};
__global__ __launch_bounds__(256) void frame_outputs_kernel(const float* __restrict__ mu, int N_old, const int* __restrict__ added_dev,
                                                            const uint8_t* __restrict__ img, int pitch, int w, int h, float fx, float fy,
                                                            float cx, float cy, float* __restrict__ out, const int* __restrict__ info,
                                                            int* host_word, int seq, const float* __restrict__ Pcol,
                                                            const float* __restrict__ Kyp, int kyp_blocks, int kyp_ld, FrameCovOut cov, FrameIdsOut ids) {
    extern __shared__ float s_mu[];  // Pcol / Kyp: the updated mean, EKF_BASE + 3 N floats
    const int added = added_dev ? *added_dev : 0;
    const int N = N_old + added;
    if (Pcol || Kyp) {
        const int n = EKF_BASE + 3 * N;
        if (Kyp) {
            // (round 6, T2 flow: K y as the gain tiles' partial sums, one row per block column, added as gemm16_finish_mean<3> adds them -- and requested as
            // it requests them: up to four elements per thread and sixteen block columns each as ONE batch from clamped addresses.  The loop with a
            // run-time bound it replaces was compiled load - wait - add: a memory round trip per block column and element, ~30 in a row at N = 256;
            // image loop at N = 256, same box: 5 622 -> 5 798 frames/s.)
            float v4[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int e = min((int)threadIdx.x + 256 * u, n - 1);
                float pk[16];
#pragma unroll
                for (int cb = 0; cb < 16; cb++) pk[cb] = Kyp[(size_t)min(cb, kyp_blocks - 1) * kyp_ld + e];
                const float m0 = mu[e];
                float ky = pk[0];
#pragma unroll
                for (int cb = 1; cb < 16; cb++) ky = (cb < kyp_blocks) ? ky + pk[cb] : ky;
                for (int cb = 16; cb < kyp_blocks; cb++) ky = ky + Kyp[(size_t)cb * kyp_ld + e];
                v4[u] = m0 + ky;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int e = (int)threadIdx.x + 256 * u;
                if (e < n) s_mu[e] = v4[u];
            }
            for (int e = threadIdx.x + 1024; e < n; e += 256) {
                float ky = Kyp[e];
                for (int cb = 1; cb < kyp_blocks; cb++) ky = ky + Kyp[(size_t)cb * kyp_ld + e];
                s_mu[e] = mu[e] + ky;
            }
        } else {
            for (int e = threadIdx.x; e < n; e += 256) s_mu[e] = mu[e] + Pcol[e];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const float q0 = s_mu[3], q1 = s_mu[4], q2 = s_mu[5], q3 = s_mu[6];
            const float qn = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
            s_mu[3] = q0 / qn, s_mu[4] = q1 / qn, s_mu[5] = q2 / qn, s_mu[6] = q3 / qn;
        }
        __syncthreads();
        mu = s_mu;
    }
    if (threadIdx.x < EKF_BASE) out[threadIdx.x] = mu[threadIdx.x];
    float* xyz = out + EKF_BASE;
    float* inten = xyz + 3 * (size_t)N;
    for (int i = threadIdx.x; i < N; i += 256) points_one(mu, i, img, pitch, w, h, fx, fy, cx, cy, xyz, inten);
    for (int i = threadIdx.x; i < N; i += 256) ids.out_id[i] = ids.id[i], ids.out_born[i] = ids.born[i];
    if (cov.S) {
        const float* S = (cov.removed_dev && cov.removed_dev[1] > 0) ? cov.S_removed : cov.S;
        if (threadIdx.x < 72) odom_cov_one(mu, S, cov.ld, threadIdx.x, cov.out);
        for (int i = threadIdx.x; i < N; i += 256) points_cov_one(mu, S, cov.ld, i, cov.out + 72);
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) publish_host_words(host_word, info, added, seq);
}

}  // namespace

// Enqueues frame_outputs_kernel over level 0 of the current frame and returns the status sequence number it publishes.
// early: between the update's two Joseph GEMMs, or in front of the T2 flow's one -- the updated mean is formed in LDS (n floats) from
// `mu` and K y, which is column n of P or, with kyp_blocks > 0, Wt's first rows.  Otherwise behind the frame's last launch: `mu` is
// final, and count_dev (may be null) holds the landmarks added meanwhile.  removed: a removal is enqueued in front (its words say whether Sigma moved).
static int launch_frame_outputs(ekfvio_filter* f, const float* mu, const int* count_dev, int kyp_blocks, bool early, bool removed = false) {
    const Level0View v = klt_level0(f);
    const int seq = next_status_seq(f);
    const float* Pcol = early && kyp_blocks == 0 ? f->P + (size_t)f->n * f->ldp : nullptr;
    const float* Kyp = early && kyp_blocks > 0 ? f->Wt : nullptr;
    FrameCovOut cov;
    if (f->output_cov && !early) {
        cov.S = f->P, cov.ld = f->ldp, cov.out = f->d_out + out_cov_offset(f);
        if (removed) cov.S_removed = f->P2, cov.removed_dev = f->remove_words;
    }
    FrameIdsOut ids;
    ids.id = f->lm_id, ids.born = f->lm_born;
    ids.out_id = reinterpret_cast<int64_t*>(f->d_out + out_ids_offset(f));
    ids.out_born = reinterpret_cast<double*>(ids.out_id + (f->cfg.max_features > 0 ? f->cfg.max_features : 1));
    hipLaunchKernelGGL(frame_outputs_kernel, dim3(1), dim3(256), early ? sizeof(float) * (size_t)f->n : 0, f->stream, mu, f->N, count_dev, v.img,
                       v.pitch, v.w, v.h, v.fx, v.fy, v.cx, v.cy, f->d_out, f->info, f->d_hinfo, seq, Pcol, Kyp, kyp_blocks, early ? f->ldp : 0, cov,
                       ids);
    return seq;
}

extern "C" {

// publishPoints' payload (EKFVIO.cpp:479-518), formed on the device: xyz3N = (u/rho, v/rho, 1/rho) per landmark in the
// camera frame, intensityN = the current (resized) frame's byte at the landmark's pixel (0 outside the image or before
// the first frame).  Either pointer may be NULL.
int ekfvio_get_points(ekfvio_filter* f, float* xyz3N, float* intensityN) {
    if (!f) return EKFVIO_EINVAL;
    const int N = f->N;
    if (N == 0) return EKFVIO_OK;
    if (f->out_fresh) {  // the frame's last kernel wrote them with the status word (frame_outputs_kernel)
        if (xyz3N) memcpy(xyz3N, f->h_out + EKF_BASE, sizeof(float) * 3 * N);
        if (intensityN) memcpy(intensityN, f->h_out + EKF_BASE + 3 * (size_t)N, sizeof(float) * N);
        return EKFVIO_OK;
    }
    HIP_TRY(f, hipSetDevice(f->device));
    const Level0View v = klt_level0(f);  // (all zeros before the first frame: intensity 0)
    // the kernel writes into pinned host memory (behind the 22 floats ekfvio_get_base_mu uses): xyz, then the intensities
    float* d_xyz = f->d_out + EKF_BASE;
    float* d_int = d_xyz + 3 * (size_t)N;
    int bad = 0, rc;
    if (N <= 256) {  // one workgroup: it publishes the status word itself
        const int seq = next_status_seq(f);
        hipLaunchKernelGGL(points_kernel, dim3(1), dim3(256), 0, f->stream, f->mu, N, v.img, v.pitch, v.w, v.h, v.fx, v.fy, v.cx, v.cy, d_xyz, d_int,
                           f->info, f->d_hinfo, seq);
        rc = poll_status(f, seq, &bad, nullptr);
    } else {
        hipLaunchKernelGGL(points_kernel, dim3((N + 255) / 256), dim3(256), 0, f->stream, f->mu, N, v.img, v.pitch, v.w, v.h, v.fx, v.fy, v.cx, v.cy,
                           d_xyz, d_int, nullptr, nullptr, 0);
        rc = wait_status(f, &bad);
    }
    if (rc != EKFVIO_OK) return rc;
    if (xyz3N) memcpy(xyz3N, f->h_out + EKF_BASE, sizeof(float) * 3 * N);
    if (intensityN) memcpy(intensityN, f->h_out + EKF_BASE + 3 * (size_t)N, sizeof(float) * N);
    return EKFVIO_OK;
}

// The landmarks' ids and birth stamps (include/ekfvio.h, "landmark identities"), rows as ekfvio_get_points' of the same moment: a memcpy
// while the frame's outputs are fresh, else a device-to-host copy on the handle's stream and a wait, as ekfvio_get_features.
int ekfvio_get_landmark_ids(ekfvio_filter* f, int64_t* idN, double* bornN) {
    if (!f) return EKFVIO_EINVAL;
    const int N = f->N;
    if (N == 0) return EKFVIO_OK;
    if (f->out_fresh) {
        const int64_t* h_id = reinterpret_cast<const int64_t*>(f->h_out + out_ids_offset(f));
        if (idN) memcpy(idN, h_id, sizeof(int64_t) * N);
        if (bornN) memcpy(bornN, h_id + (f->cfg.max_features > 0 ? f->cfg.max_features : 1), sizeof(double) * N);
        return EKFVIO_OK;
    }
    HIP_TRY(f, hipSetDevice(f->device));
    if (idN) HIP_TRY(f, hipMemcpyAsync(idN, f->lm_id, sizeof(int64_t) * N, hipMemcpyDeviceToHost, f->stream));
    if (bornN) HIP_TRY(f, hipMemcpyAsync(bornN, f->lm_born, sizeof(double) * N, hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    return EKFVIO_OK;
}

// The covariances of the outputs (include/ekfvio.h): a memcpy while the frame's outputs are fresh and include them, else one launch on the
// handle's stream -- behind whatever is still running there, an update's Joseph GEMM included -- and one wait.
int ekfvio_set_output_covariance(ekfvio_filter* f, int32_t on) {
    if (!f || (on != 0 && on != 1)) return EKFVIO_EINVAL;
    f->output_cov = on != 0;  // (read by the next ekfvio_step_image; the frame loop is in no captured graph)
    if (!on) f->out_cov_fresh = false;
    return EKFVIO_OK;
}

int ekfvio_get_odometry_covariance(ekfvio_filter* f, float pose_cov[36], float twist_cov[36]) {
    if (!f) return EKFVIO_EINVAL;
    const size_t off = out_cov_offset(f);
    if (!(f->out_fresh && f->out_cov_fresh)) {
        HIP_TRY(f, hipSetDevice(f->device));
        const int seq = next_status_seq(f);
        hipLaunchKernelGGL(odom_cov_kernel, dim3(1), dim3(128), 0, f->stream, f->mu, f->P, f->ldp, f->d_out + off, f->info, f->d_hinfo, seq);
        int bad = 0;
        const int rc = poll_status(f, seq, &bad, nullptr);
        if (rc != EKFVIO_OK) return rc;
    }
    if (pose_cov) memcpy(pose_cov, f->h_out + off, sizeof(float) * 36);
    if (twist_cov) memcpy(twist_cov, f->h_out + off + 36, sizeof(float) * 36);
    return EKFVIO_OK;
}

int ekfvio_get_points_covariance(ekfvio_filter* f, float* cov9N) {
    if (!f) return EKFVIO_EINVAL;
    const int N = f->N;
    if (N == 0) return EKFVIO_OK;
    if (!cov9N) return EKFVIO_EINVAL;
    const size_t off = out_cov_offset(f) + 72;
    if (!(f->out_fresh && f->out_cov_fresh)) {
        HIP_TRY(f, hipSetDevice(f->device));
        int bad = 0, rc;
        if (N <= 256) {  // one workgroup: it publishes the status word itself
            const int seq = next_status_seq(f);
            hipLaunchKernelGGL(points_cov_kernel, dim3(1), dim3(256), 0, f->stream, f->mu, f->P, f->ldp, N, f->d_out + off, f->info, f->d_hinfo, seq);
            rc = poll_status(f, seq, &bad, nullptr);
        } else {
            hipLaunchKernelGGL(points_cov_kernel, dim3((N + 255) / 256), dim3(256), 0, f->stream, f->mu, f->P, f->ldp, N, f->d_out + off, nullptr, nullptr, 0);
            rc = wait_status(f, &bad);
        }
        if (rc != EKFVIO_OK) return rc;
    }
    memcpy(cov9N, f->h_out + off, sizeof(float) * 9 * (size_t)N);
    return EKFVIO_OK;
}

int ekfvio_rotation_error_jacobian(const float q_wxyz[4], float J3x4[12]) {
    if (!q_wxyz || !J3x4) return EKFVIO_EINVAL;
    for (int r = 0; r < 3; r++) rot_err_jacobian_row(q_wxyz, r, J3x4 + 4 * r);
    return EKFVIO_OK;
}

// EKFVIO::addFrame + updateStateWithNewImage (EKFVIO.cpp:139-219) minus ROS publishing; with
// cfg.replenish the FAST replenishment of :154 / :172 runs on the device too (otherwise the caller
// adds landmarks with ekfvio_add_features).
int ekfvio_step_image(ekfvio_filter* f, double stamp, const uint8_t* image, int32_t width, int32_t height, int32_t stride,
                      const float K[9]) {
    if (!f) return EKFVIO_EINVAL;
    f->out_fresh = f->out_cov_fresh = false;
    const bool first = !f->frames[f->cur].valid;
    if (!first && f->have_stamp && !(stamp - f->t_stamp >= 0)) return EKFVIO_EINVAL;  // ROS_ASSERT(dt >= 0)
    // nothing below waits for the device until the status word is read at the very end: process(dt), the frame
    // upload, the pyramid, the tracker and the update are enqueued back to back.  process(dt) goes first: it does not
    // depend on the image, so the device runs it while the host copies the frame into the pinned buffer.
    // everything that can refuse the frame (sizes, capacity growth) comes before the first launch
    int rc = push_frame_check(f, image, width, height, stride, K);
    if (rc != EKFVIO_OK) return rc;
    sweep_maybe_retry(f);
    const float dt = first ? 0.f : (float)(stamp - f->t_stamp);
    // an error return from here on has work enqueued behind it: wait for it (the pinned frame buffer is rewritten by the
    // next call) and leave the stamp with the state it belongs to
    auto fail = [&](int code) {
        (void)hipStreamSynchronize(f->stream);
        return code;
    };
    if (!first) {
        HIP_TRY(f, hipSetDevice(f->device));
        launch_predict(f, dt);
        f->t_stamp = stamp;  // tc_ekf.t = f.t (:164): the state now stands at this stamp whatever happens below
        f->have_stamp = true;
    }
    rc = push_frame_enqueue(f, image, width, height, stride, K);
    if (rc != EKFVIO_OK) return fail(rc);
    if (first) {
        // first frame: remember the stamp (tc_ekf.t = f.t) and return; the caller replenishes
        if (!f->have_stamp) {
            f->t_stamp = stamp;
            f->have_stamp = true;
        }
        if (f->cfg.remove_lost) ended_note_removal(f, 0);  // (a removing frame with no landmark: no track ended)
        if (f->cfg.replenish) return ekfvio_replenish(f, nullptr, nullptr);  // replenishFeatures(first frame) (:154)
        HIP_TRY(f, hipStreamSynchronize(f->stream));
        return EKFVIO_OK;
    }
    int early_seq = 0;
    UpdateInputs in;  // the frame's update (and its re-run behind an aborted persistent sweep)
    in.z = f->zmeas, in.R = f->Rmeas, in.pass = f->pass, in.m_on_device = true;
    const bool zupt = f->zupt_max_flow_px > 0.f && f->N > 0;  // (off, or no landmark: nothing is launched)
    const bool aid = f->frame_aid_k > 0;  // ekfvio_set_frame_aid: the standing measurement, landmarks or not
    if (aid && f->N <= 0) launch_aid_frame(f);
    if (f->N > 0) {  // "run update if we have enough features" (EKFVIO.cpp:166)
        rc = klt_track_device(f);
        if (rc != EKFVIO_OK) return fail(rc);
        // ekfvio_set_zupt: the zero-velocity decision over the tracker's results and, on a "yes", its update of the propagated state: the
        // gate and the update below read the state it leaves.  Outside `in`: the re-run behind an aborted sweep does not repeat it
        // ekfvio_set_frame_aid sits in front of it, likewise outside `in`: the zero-velocity update reads the state the aiding update leaves
        if (aid) launch_aid_frame(f);
        if (zupt) launch_zupt_frame(f);
        // the pass flags stay on the device: the update is launched for m = 2N measurement rows and its kernels take
        // the true count from the bookkeeping (rows beyond it are identity padding, exact zeros in every product)
        // A frame that adds no landmarks publishes its outputs and its status BETWEEN the update's two Joseph GEMMs (frame_outputs_kernel,
        // Pcol): launch_update calls back there.  (With landmarks to add the selection reads the updated mean and the outputs carry the count:
        // behind the update, as before.  EKFVIO_EARLY_OUTPUTS=0: always behind.)
        // (Nor with cfg.remove_lost: the frame's final landmark count is known only behind the removal, as with a replenishing frame.)
        // (Nor with ekfvio_set_output_covariance: the outputs then include covariances of Sigma', which the last GEMM is still to write.)
        if (f->tune.early_outputs && f->tune.frame_outputs && !(f->cfg.replenish && f->N < f->cfg.max_features) && !f->cfg.remove_lost && !f->output_cov &&
            sizeof(float) * (size_t)f->n <= 48 * 1024) {  // (the updated mean is formed in LDS)
            // (two-GEMM flow: K y is column n of P, left there by the first Joseph GEMM; T2 flow: the gain tiles' partial sums in Wt, and the
            // outputs go out in front of the update's ONE GEMM)
            in.between = [](ekfvio_filter* g, int kyp_blocks) { return launch_frame_outputs(g, g->mu, nullptr, kyp_blocks, true); };
        }
        early_seq = launch_update(f, in).between_seq;  // 0: the hook was not reached (no measurement, another flow of the update)
        if (early_seq) f->early_output_frames++;
    }
    if (hipGetLastError() != hipSuccess) {
        f->last_error = "launch failed in ekfvio_step_image";
        return fail(EKFVIO_EDEVICE);
    }
    // "try to get more features if needed" (:172): detection, first-fit selection and the growth of the state are
    // enqueued behind the update with the number of new landmarks left on the device; the host reads it with the status
    // word, in the frame's single wait, and only then counts the landmarks in
    int replenishing = 0;
    if (f->cfg.replenish) {
        rc = replenish_enqueue(f, &replenishing);
        if (rc != EKFVIO_OK) return fail(rc);
        if (replenishing) add_features_enqueue_device_count(f, f->fast_counts + 1);
    }
    // cfg.remove_lost: every flagged landmark leaves the state behind the replenishment (which still saw them), in front of the
    // frame's outputs (remove.hip).  The kernel takes the landmark count from the device (N + what the replenishment added) and leaves
    // `added - removed` in remove_words[0]: the outputs kernel counts the landmarks from it and the host reads it with the status word,
    // so the frame keeps its single wait.  Flags only come from an update, and the flagged landmarks of earlier frames are gone: with
    // no landmark before the frame there is nothing to remove.  Behind an aborted persistent sweep the kernel removes nothing (the
    // update is run again below over the layout it was enqueued for); the flags stay and the next frame removes those landmarks.
    const bool removing = f->cfg.remove_lost && f->N > 0;
    const int* count_dev = replenishing ? f->fast_counts + 1 : nullptr;
    if (removing) {
        launch_remove_features(f, nullptr, count_dev, true, true);  // (with ekfvio_set_ended_export: the ended tracks' records in front of it)
        count_dev = f->remove_words;
    } else if (f->cfg.remove_lost) {
        ended_note_removal(f, 0);
    }
    // the frame's one wait: the status word, the number of new landmarks and what the node publishes after addFrame
    // (odometry, point cloud) arrive together in pinned host memory (frame_outputs_kernel)
    // (EKFVIO_FRAME_OUTPUTS=0: the status word and the count alone, published by read_status itself)
    int seq = early_seq;  // (non-zero: the outputs went out between the Joseph GEMMs, launch_update's hook)
    // (behind a removal the mean is in mu_next: the host swaps the two once it has the status word)
    if (!seq && f->tune.frame_outputs) seq = launch_frame_outputs(f, removing ? f->mu_next : f->mu, count_dev, 0, false, removing);
    int bad = 0, added = 0;
    rc = read_status(f, seq, count_dev, &bad, &added);
    if (rc != EKFVIO_OK) return rc;
    f->out_fresh = f->tune.frame_outputs != 0;
    f->out_cov_fresh = f->out_fresh && f->output_cov;
    if (aid) aid_note_frame(f);  // (its words likewise)
    if (f->zupt_max_flow_px > 0.f) zupt_note_frame(f, zupt);  // the decision's words arrived in pinned host memory in front of the status word
    // (in front of a re-run, which reads f->mu and f->P as the swap leaves them; the count of landmarks: below, with `added`)
    const int removed = removing ? __atomic_load_n(&f->h_info[HW_REMOVED], __ATOMIC_ACQUIRE) : 0;
    if (removing) {
        remove_applied(f, 0, removed);
        ended_note_removal(f, removed);
    }
    // Bit 1: the persistent sweep gave up (chol_persist.inc), the Joseph GEMMs wrote nothing, the state is the propagated one.
    // The update runs again now, with one launch per block step, over the landmarks it was enqueued for (the count is
    // bumped below): idx, the measured coordinates per row, R and the row count are where the bookkeeping left them.
    // Landmarks the replenishment has added meanwhile lie outside n, with ONE exception the re-run relies on an invariant for
    // (ADVICE r04): the first Joseph GEMM writes n + 1 columns -- column n carries K y -- and the second zeroes rows 0 .. n-1 of
    // column n again; column n is now the first new landmark's column.  addNewFeatures leaves a new landmark's cross-covariances
    // exactly zero and its measurement-map entries at -1, so "zero before, K y in between, zero after" is what an update without
    // new landmarks does to that padding column too (tests/test_gpu_sweep_abort.py, the replenishing-frame case).  (Those
    // landmarks were picked around the predicted, not the updated, landmark pixels: a valid state, not bit for bit the
    // frame an unshared GPU produces.)
    const int status = settle_update(f, bad, [](ekfvio_filter* g, void* c) {
        UpdateInputs& again = *static_cast<UpdateInputs*>(c);
        again.between = nullptr, again.bookkeeping_done = true;
        launch_update(g, again);
    }, &in, f->N > 0);
    if (status != EKFVIO_OK && status != EKFVIO_ENUMERIC) return status;  // (aborted again, or the device failed: the landmarks are not counted in)
    if (added != 0) {  // (added - removed with cfg.remove_lost)
        f->N += added;
        f->n += 3 * added;
    }
    f->next_id += added + removed;  // what the replenishment appended: its ids are visible from here on (not counted in above: never visible)
    return status;
}

}  // extern "C"
