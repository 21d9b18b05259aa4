// ekf_vio_amd/csrc/zupt.h — the zero-velocity decision (include/ekfvio.h, ekfvio_set_zupt): the lines of its specification, shared by the
// kernels of zupt.hip and the host function ekfvio_zupt_decide: one set of inline functions, compiled for the host and for the device, fp32
// without contraction, so that both give the bits of a NumPy restatement (tests/_zupt.py).  The two counts come from wavefront ballots on
// the device and from a loop on the host.
#pragma once
#include <math.h>
#include <stdint.h>

// e2 of one passed landmark: the squared pixel distance between the tracked pixel (qx, qy) and the reference pixel (px, py)
__host__ __device__ inline float zupt_flow2(float qx, float qy, float px, float py) {
    const float dx = qx - px, dy = qy - py;
    return dx * dx + dy * dy;
}
// (a NaN is not still)
__host__ __device__ inline bool zupt_still(float e2, float t2) { return e2 <= t2; }
__host__ __device__ inline int zupt_stationary(int n_pass, int n_still, int min_tracks, float min_ratio) {
    return (n_pass >= min_tracks && (float)n_still >= min_ratio * (float)n_pass) ? 1 : 0;
}
// what ekfvio_set_zupt accepts as "on" (ekfvio_zupt_decide and the test hook: the first three)
inline bool zupt_decision_valid(float max_flow_px, int min_tracks, float min_ratio) {
    return isfinite(max_flow_px) && max_flow_px > 0.f && min_tracks >= 1 && min_ratio > 0.f && min_ratio <= 1.f;
}
inline bool zupt_variances_valid(float vel_variance, float omega_variance) {
    return isfinite(vel_variance) && vel_variance > 0.f && isfinite(omega_variance) && omega_variance > 0.f;
}
