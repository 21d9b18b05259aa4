// ekf_vio_amd/csrc/klt_photo.h — the gain/offset term of the tracker (include/ekfvio.h, ekfvio_set_klt_photometric): the lines of its
// specification behind the six sums, shared by klt_lk_pass (klt.hip) and the host function ekfvio_klt_project_gradients: one set of
// inline functions, compiled for the host and for the device, exact integers and fp32 without contraction, so that both give the bits of
// a NumPy restatement (tests/_klt_photo.py).  The sums themselves come from a wavefront on the device and from a loop on the host.
#pragma once
#include <math.h>
#include <stdint.h>

#define KLT_PHOTO_MAX_COUNT 441  // 21 x 21, the largest window
#define KLT_PHOTO_CLAMP 4080     // the bound of a Scharr derivative of bytes: what the tracker's integer sums are sized for

// sum Iv, Ix, Iy, Iv*Iv, Iv*Ix, Iv*Iy over the window's n pixels, exact
struct KltPhotoSums {
    long long sI, sX, sY, sII, sIX, sIY;
};
// what the projection of one pixel needs: the three means and the two regression coefficients on Iv
struct KltPhotoCoef {
    float mI, mX, mY, cx, cy;
};
__host__ __device__ inline KltPhotoCoef klt_photo_coef(const KltPhotoSums& s, int n) {
    const long long nn = n;
    const long long VI = nn * s.sII - s.sI * s.sI;  // >= 0 (Cauchy-Schwarz); 0: a constant template
    const long long CX = nn * s.sIX - s.sI * s.sX, CY = nn * s.sIY - s.sI * s.sY;
    KltPhotoCoef c;
    c.mI = (float)s.sI / (float)n;
    c.mX = (float)s.sX / (float)n;
    c.mY = (float)s.sY / (float)n;
    c.cx = VI > 0 ? (float)CX / (float)VI : 0.0f;
    c.cy = VI > 0 ? (float)CY / (float)VI : 0.0f;
    return c;
}
// one gradient value g (Ix[t] or Iy[t]) of a pixel with template value iv, with span{1, Iv} projected out: m and c are the gradient
// image's mean and coefficient (mX, cx or mY, cy)
__host__ __device__ inline int klt_photo_project(int g, int iv, float m, float c, float mI) {
    const float r = rintf(((float)g - m) - c * ((float)iv - mI));  // (round half to even: the default rounding mode)
    const int i = (int)r;                                           // |r| < 2^25: exact
    return i < -KLT_PHOTO_CLAMP ? -KLT_PHOTO_CLAMP : (i > KLT_PHOTO_CLAMP ? KLT_PHOTO_CLAMP : i);
}
