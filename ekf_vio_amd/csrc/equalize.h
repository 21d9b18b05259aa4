// ekf_vio_amd/csrc/equalize.h — the lines of the equalisation's specification (include/ekfvio.h, ekfvio_set_equalize), shared by the
// kernels of equalize.hip and the host function ekfvio_equalize: one set of inline functions, compiled for the host and for the device,
// integers and fp32 without contraction, so that both give the bits of a NumPy restatement (tests/_equalize.py).
#pragma once
#include <math.h>
#include <stdint.h>

#define EQ_MAX_TILES 16  // per axis (tile counts above it are out of scope)

// The host values of the specification: formed once per frame size and setting, passed to the kernels as ONE argument
struct EqualizeParams {
    int tx, ty;    // tiles
    int tw, th;    // tile size: ceil(w / tx), ceil(h / ty)
    int A;         // tw * th: every tile's pixel count (the padding is reflected in)
    int clip;      // max(floor(clip_limit * A / 256), 1)
    float scale;   // 255 / A
    float inv_tw, inv_th;
};

// clip_limit: finite, > 0; 1 <= tx <= w, 1 <= ty <= h (the callers have checked)
inline EqualizeParams equalize_params(int w, int h, float clip_limit, int tx, int ty) {
    EqualizeParams p;
    p.tx = tx, p.ty = ty;
    p.tw = (w + tx - 1) / tx, p.th = (h + ty - 1) / ty;
    p.A = p.tw * p.th;
    // (no bin ever holds more than A: a clip of A and above clips nothing, and the conversion to int stays defined for a huge limit)
    const double c = floor((double)clip_limit * (double)p.A / 256.0);
    p.clip = c >= (double)p.A ? p.A : (c < 1.0 ? 1 : (int)c);
    p.scale = 255.0f / (float)p.A;
    p.inv_tw = 1.0f / (float)p.tw, p.inv_th = 1.0f / (float)p.th;
    return p;
}

// the setting's own test (ekfvio_set_equalize, ekfvio_equalize); clip_limit == 0 is "off" and the caller's case
inline bool equalize_setting_ok(float clip_limit, int tx, int ty) {
    return __builtin_isfinite(clip_limit) && clip_limit > 0.f && tx >= 1 && tx <= EQ_MAX_TILES && ty >= 1 && ty <= EQ_MAX_TILES;
}

// step 1: reflect-101 of a padded coordinate X in [0, n + tile) back into [0, n)
__host__ __device__ inline int equalize_reflect(int X, int n) { return X >= n ? 2 * (n - 1) - X : X; }

// step 3: what the tile's `excess` becomes -- batch per bin, res bins that get one more, every step-th from bin 0
struct EqualizeSpread {
    int batch, res, step;
};
__host__ __device__ inline EqualizeSpread equalize_spread(int excess) {
    EqualizeSpread s;
    s.batch = excess / 256;
    s.res = excess - 256 * s.batch;
    s.step = s.res > 0 ? (256 / s.res > 1 ? 256 / s.res : 1) : 1;
    return s;
}
__host__ __device__ inline int equalize_excess(int hist, int clip) { return hist > clip ? hist - clip : 0; }
// ... and bin b afterwards
__host__ __device__ inline int equalize_bin(int hist, int clip, const EqualizeSpread& s, int b) {
    const int clipped = hist > clip ? clip : hist;
    const int one = (s.res > 0 && b % s.step == 0 && b / s.step < s.res) ? 1 : 0;
    return clipped + s.batch + one;
}

__host__ __device__ inline uint8_t equalize_saturate(float r) { return r <= 0.f ? (uint8_t)0 : (r >= 255.f ? (uint8_t)255 : (uint8_t)(int)r); }
// step 4: the LUT byte from the inclusive sum hist[0] + ... + hist[b]
__host__ __device__ inline uint8_t equalize_lut_byte(int cum, float scale) { return equalize_saturate(rintf((float)cum * scale)); }

// step 5: the two tile indices and weights along one axis
struct EqualizeAxis {
    int i1, i2;
    float a, a1;
};
__host__ __device__ inline EqualizeAxis equalize_axis(int x, float inv_t, int tiles) {
    const float fx = (float)x * inv_t - 0.5f;
    const float t = floorf(fx);
    EqualizeAxis r;
    r.a = fx - t, r.a1 = 1.0f - r.a;
    const int ti = (int)t;
    r.i1 = ti > 0 ? ti : 0;
    r.i2 = ti + 1 < tiles - 1 ? ti + 1 : tiles - 1;
    return r;
}
// ... and the pixel from the four tables' bytes for its value (l11 = lut[j1][i1][v], l12 = lut[j1][i2][v], l21 = lut[j2][i1][v], l22 = lut[j2][i2][v])
__host__ __device__ inline uint8_t equalize_blend(int l11, int l12, int l21, int l22, const EqualizeAxis& ax, const EqualizeAxis& ay) {
    const float top = (float)l11 * ax.a1 + (float)l12 * ax.a;
    const float bot = (float)l21 * ax.a1 + (float)l22 * ax.a;
    return equalize_saturate(rintf(top * ay.a1 + bot * ay.a));
}
