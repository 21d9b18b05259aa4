// ekf_vio_amd/csrc/points.h — a landmark's camera-frame point and its covariance, the lines of ekfvio_get_points and
// ekfvio_get_points_covariance (include/ekfvio.h).  ONE statement of that arithmetic for everything that publishes it: the getters' kernels
// and frame_outputs_kernel (frame.hip), and the records of the tracks that ended (ended.hip), which must carry the getters' bits.
#pragma once
#include "common.h"

// EKFVIO::publishPoints (EKFVIO.cpp:479-518): camera-frame point (u/rho, v/rho, 1/rho) per landmark -- p(2) = 1.0/p(2)
// in double, narrowed, then two float products -- and the "intensity" channel f.img.at<uchar>(e.getPixel(f)): the byte
// at the landmark's pixel (Feature::getPixel: K(0)*mu(0) + K(2), K(4)*mu(1) + K(5); cv::Point2f -> cv::Point rounds
// to nearest even, cvRound).  The reference reads outside the image unchecked; here such a landmark gets intensity 0.
// img = pixel (0,0) of level 0 of the current frame, or null when no frame has been pushed (intensity 0 then).
__device__ inline void points_one(const float* __restrict__ mu, int i, const uint8_t* __restrict__ img, int pitch, int w, int h,
                                  float fx, float fy, float cx, float cy, float* __restrict__ xyz, float* __restrict__ intensity) {
    const float u = mu[EKF_BASE + 3 * i], v = mu[EKF_BASE + 3 * i + 1], rho = mu[EKF_BASE + 3 * i + 2];
    const float z = (float)(1.0 / (double)rho);
    xyz[3 * i] = u * z;
    xyz[3 * i + 1] = v * z;
    xyz[3 * i + 2] = z;
    float in = 0.f;
    if (img) {
        const float px = fx * u + cx, py = fy * v + cy;
        // cvRound; compared as floats first so that NaN / huge values never reach the conversion
        if (px >= -0.5f && px < (float)w && py >= -0.5f && py < (float)h) {
            const int ix = __float2int_rn(px), iy = __float2int_rn(py);
            if (ix >= 0 && ix < w && iy >= 0 && iy < h) in = (float)img[(size_t)iy * pitch + ix];
        }
    }
    intensity[i] = in;
}

// Landmark i's 3x3 into out9N[9 i ..] (include/ekfvio.h, "covariances of the published outputs": fp32, no contraction): one lane per
// landmark; its six Sigma entries lie in three columns
__device__ inline void points_cov_one(const float* __restrict__ mu, const float* __restrict__ P, int ld, int i, float* __restrict__ out9N) {
    const int s = EKF_BASE + 3 * i;
    const float u = mu[s], v = mu[s + 1], rho = mu[s + 2];
    const float z = (float)(1.0 / (double)rho);
    const float x = u * z, y = v * z;
    const float jx = -(x * z), jy = -(y * z), jz = -(z * z);
    const float* c0 = P + (size_t)s * ld + s;  // column s from its diagonal element down
    const float* c1 = c0 + ld + 1;
    const float L00 = c0[0], L10 = c0[1], L20 = c0[2], L11 = c1[0], L21 = c1[1], L22 = c1[ld + 1];
    const float M00 = z * L00 + jx * L20, M02 = z * L20 + jx * L22;
    const float M10 = z * L10 + jy * L20, M11 = z * L11 + jy * L21, M12 = z * L21 + jy * L22;
    const float M20 = jz * L20, M21 = jz * L21, M22 = jz * L22;
    const float C00 = M00 * z + M02 * jx;
    const float C10 = M10 * z + M12 * jx, C11 = M11 * z + M12 * jy;
    const float C20 = M20 * z + M22 * jx, C21 = M21 * z + M22 * jy, C22 = M22 * jz;
    float* o = out9N + 9 * (size_t)i;
    o[0] = C00, o[1] = C10, o[2] = C20;
    o[3] = C10, o[4] = C11, o[5] = C21;
    o[6] = C20, o[7] = C21, o[8] = C22;
}
