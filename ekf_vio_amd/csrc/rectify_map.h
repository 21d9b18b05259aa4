// ekf_vio_amd/csrc/rectify_map.h — the rectification map's fp64 block (include/ekfvio.h, ekfvio_set_distortion and ekfvio_set_camera_model),
// shared by rectify.hip (the map kernels, ekfvio_rectify_map, ekfvio_rectify_map_model) and mask.hip (ekfvio_mask_blocked forms the border's
// no-data pixels from the same entries): one set of lines, compiled for the host and for the device, in fp64 without contraction.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/ekfvio.h"  // EKFVIO_CAMERA_*

struct RectifyCam {
    double fx, cx, fy, cy;
    double k1, k2, p1, p2, k3;
    double fxp, cxp, fyp, cyp;  // the rectified camera: P where set, else the four values above
    double k4, k5, k6;          // RATIONAL: the denominator; EQUIDISTANT: k4 alone (its k1..k4 sit in k1, k2, k3, k4; p1, p2 are not read)
};

// include/ekfvio.h, atan_spec: arctan of r >= 0 by a fixed recipe (two argument reductions, a 20-term odd polynomial by Horner), so that
// the device, the host and NumPy give one result where three libm implementations give three
__host__ __device__ inline double rectify_atan_spec(double r) {
    const double T8 = 0.41421356237309503, PI_4 = 0.7853981633974483, PI_2 = 1.5707963267948966;
    const bool inv = r > 1.0;
    double t = inv ? 1.0 / r : r;
    const bool sh = t > T8;
    t = sh ? (t - 1.0) / (t + 1.0) : t;
    const double q = t * t;
    // c_k = (k even ? +1 : -1) * (1.0 / (2k + 1)): the quotients are formed by the compiler, correctly rounded
    const double c[20] = {1.0 / 1.0,   -(1.0 / 3.0),  1.0 / 5.0,  -(1.0 / 7.0),  1.0 / 9.0,  -(1.0 / 11.0), 1.0 / 13.0,
                          -(1.0 / 15.0), 1.0 / 17.0, -(1.0 / 19.0), 1.0 / 21.0, -(1.0 / 23.0), 1.0 / 25.0, -(1.0 / 27.0),
                          1.0 / 29.0,  -(1.0 / 31.0), 1.0 / 33.0, -(1.0 / 35.0), 1.0 / 37.0, -(1.0 / 39.0)};
    double p = c[19];
#pragma unroll
    for (int k = 18; k >= 0; k--) p = p * q + c[k];
    double a = t * p;
    if (sh) a = PI_4 + a;
    if (inv) a = PI_2 - a;
    return a;
}

// include/ekfvio.h, rectification: the fp64 block, line by line, one instance per camera model
template <int MODEL>
__host__ __device__ inline void rectify_map_entry(const RectifyCam& c, int x, int y, int* sx, int* sy) {
    const double xn = ((double)x - c.cxp) / c.fxp, yn = ((double)y - c.cyp) / c.fyp;
    const double xx = xn * xn, yy = yn * yn, xy = xn * yn, r2 = xx + yy;
    double xd, yd;
    if (MODEL == EKFVIO_CAMERA_EQUIDISTANT) {
        const double r = sqrt(r2);  // (IEEE: correctly rounded on the host and on the device)
        const double th = rectify_atan_spec(r), t2 = th * th;
        const double thd = th * (1.0 + (((c.k4 * t2 + c.k3) * t2 + c.k2) * t2 + c.k1) * t2);
        const double sc = (r == 0.0) ? 1.0 : thd / r;
        xd = xn * sc, yd = yn * sc;
    } else {
        double rad = 1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2;
        if (MODEL == EKFVIO_CAMERA_RATIONAL) rad = rad / (1.0 + ((c.k6 * r2 + c.k5) * r2 + c.k4) * r2);
        xd = (xn * rad + (2.0 * c.p1) * xy) + c.p2 * (r2 + 2.0 * xx);
        yd = (yn * rad + c.p1 * (r2 + 2.0 * yy)) + (2.0 * c.p2) * xy;
    }
    const double u = c.fx * xd + c.cx, v = c.fy * yd + c.cy;
    const bool valid = fabs(u) <= 1048576.0 && fabs(v) <= 1048576.0;  // (a NaN compares false)
    *sx = valid ? (int)rint(u * 32.0) : INT32_MIN;  // |u * 32| <= 2^25: the conversion is exact
    *sy = valid ? (int)rint(v * 32.0) : INT32_MIN;
}

// the instance for a model known only at run time (the host entry points)
inline void rectify_map_entry_of(int model, const RectifyCam& c, int x, int y, int* sx, int* sy) {
    if (model == EKFVIO_CAMERA_EQUIDISTANT) rectify_map_entry<EKFVIO_CAMERA_EQUIDISTANT>(c, x, y, sx, sy);
    else if (model == EKFVIO_CAMERA_RATIONAL) rectify_map_entry<EKFVIO_CAMERA_RATIONAL>(c, x, y, sx, sy);
    else rectify_map_entry<EKFVIO_CAMERA_PLUMB_BOB>(c, x, y, sx, sy);
}

// D: the model's eight coefficients in the caller's order (zeros behind its count); P: fx', cx', fy', cy' or null (K's four)
inline RectifyCam rectify_cam(const float K[9], int model, const double D[8], const float* P) {
    RectifyCam c;
    c.fx = (double)K[0], c.cx = (double)K[2], c.fy = (double)K[4], c.cy = (double)K[5];
    c.fxp = P ? (double)P[0] : c.fx, c.cxp = P ? (double)P[1] : c.cx, c.fyp = P ? (double)P[2] : c.fy, c.cyp = P ? (double)P[3] : c.cy;
    if (model == EKFVIO_CAMERA_EQUIDISTANT) {
        c.k1 = D[0], c.k2 = D[1], c.k3 = D[2], c.k4 = D[3];
        c.p1 = c.p2 = c.k5 = c.k6 = 0.0;
    } else {
        c.k1 = D[0], c.k2 = D[1], c.p1 = D[2], c.p2 = D[3], c.k3 = D[4], c.k4 = D[5], c.k5 = D[6], c.k6 = D[7];
    }
    return c;
}

// model, D, count, P of the entry points -> eight coefficients; false: EKFVIO_EINVAL
inline bool rectify_model_arguments(int32_t model, const double* D, int32_t count, const float* P, double out[8]) {
    bool count_ok = false;
    if (model == EKFVIO_CAMERA_PLUMB_BOB) count_ok = count == 0 || count == 4 || count == 5;
    else if (model == EKFVIO_CAMERA_RATIONAL) count_ok = count == 8;
    else if (model == EKFVIO_CAMERA_EQUIDISTANT) count_ok = count == 4;
    if (!count_ok || (count > 0 && !D)) return false;
    for (int i = 0; i < 8; i++) out[i] = i < count ? D[i] : 0.0;
    for (int i = 0; i < 8; i++)
        if (!__builtin_isfinite(out[i])) return false;
    if (P) {
        for (int i = 0; i < 4; i++)
            if (!__builtin_isfinite(P[i])) return false;
        if (!(P[0] > 0.f) || !(P[2] > 0.f)) return false;
    }
    return true;
}

// the setting is on: frames are rectified (include/ekfvio.h: off only for PLUMB_BOB or RATIONAL with every coefficient zero and no P)
inline bool rectify_model_on(int32_t model, const double D[8], const float* P) {
    bool on = P != nullptr || model == EKFVIO_CAMERA_EQUIDISTANT;
    for (int i = 0; i < 8; i++) on = on || D[i] != 0.0;
    return on;
}

// D, count of ekfvio_set_distortion and its kin: the plumb_bob counts
inline bool rectify_coefficients(const double* D, int32_t count, double out[8]) {
    return rectify_model_arguments(EKFVIO_CAMERA_PLUMB_BOB, D, count, nullptr, out);
}
