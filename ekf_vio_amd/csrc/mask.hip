// ekf_vio_amd/csrc/mask.hip — the no-data mask: keeps the detector and the tracker off pixels that hold no scene.
//
// Not in the reference, which passes no mask to cv::FAST (EKFVIO.cpp:224-311).  Two sources of such pixels: the black border that
// rectification leaves (rectify.hip: a tap outside the frame contributes 0) and regions the caller knows are not scene (a bonnet, a
// gimbal arm, a burnt-in timestamp).  The three steps are specified in include/ekfvio.h (ekfvio_set_mask): full-size no-data n,
// level-0 no-data N (OR over the s x s block the resize reads), blocked B (OR of N over the kill-pad window, outside = 1).  The inline
// functions below are those lines, compiled for the host (ekfvio_mask_blocked) and for the device out of the same text.
//
// Kernels: mask_nodata_kernel (a lane per level-0 pixel, a wavefront's 64 verdicts packed by a ballot into two words) and
// mask_dilate_kernel (the window OR on the bit rows), both launched once per MaskKey behind the rectification of a pushed frame, never
// per frame.  B is kept as bit words in the layout of the detector's occupancy image (fast.hip, OccMask).  The per-frame work is the
// two consumers': replenish_select_kernel starts its occupancy image from B, the tracker's pass test reads one bit of it.  With the mask
// off nothing here is launched and nothing allocated.
#include <string.h>

#include <vector>

#include "common.h"
#include "rectify_map.h"

namespace {

// include/ekfvio.h, mask, step 1: the four taps rectify_kernel reads for the map entry (sx, sy); no-data if a tap with a non-zero
// weight lies outside [0, w) x [0, h)
__host__ __device__ inline bool mask_tap_nodata(int sx, int sy, int w, int h) {
    const int ix = sx >> 5, ax = sx & 31, iy = sy >> 5, ay = sy & 31;
    const bool x0 = ix >= 0 && ix < w, x1 = ix + 1 >= 0 && ix + 1 < w, y0 = iy >= 0 && iy < h, y1 = iy + 1 >= 0 && iy + 1 < h;
    return ((32 - ax) * (32 - ay) != 0 && !(x0 && y0)) || (ax * (32 - ay) != 0 && !(x1 && y0)) || ((32 - ax) * ay != 0 && !(x0 && y1)) ||
           (ax * ay != 0 && !(x1 && y1));
}
// step 3: the window around X (and around Y), asymmetric by one: [X - pad, X + max(pad - 1, 0)]
__host__ __device__ inline int mask_pad(int kill_pad) { return kill_pad > 0 ? kill_pad : 0; }
__host__ __device__ inline int mask_window_lo(int X, int pad) { return X - pad; }
__host__ __device__ inline int mask_window_hi(int X, int pad) { return X + (pad > 1 ? pad - 1 : 0); }

// Step 1 and 2.  A wavefront owns 64 consecutive columns of one level-0 row: lane l reduces the s x s block of column 64 c + l (the map's
// two planes, the caller's bytes, or both; a null pointer: that term is absent), a column at or beyond W counts as no-data (outside), and
// the ballot's two halves are the row's words 2 c and 2 c + 1 -- so the tail bits of a row's last word are ones.
__global__ __launch_bounds__(256) void mask_nodata_kernel(const int* __restrict__ sx, const int* __restrict__ sy,
                                                          const uint8_t* __restrict__ user, int w, int h, int s, int W, int H, int wpr,
                                                          unsigned* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int chunks = (wpr + 1) / 2;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= chunks * H) return;  // (the whole wavefront)
    const int Y = g / chunks, c = g - Y * chunks, X = 64 * c + lane;
    bool nd = true;
    if (X < W) {
        nd = false;
        for (int dy = 0; dy < s; dy++)
            for (int dx = 0; dx < s; dx++) {
                const size_t i = (size_t)(s * Y + dy) * w + (s * X + dx);  // s X + dx < s W <= w, likewise the row
                if (user) nd = nd || user[i] == 0;
                if (sx) nd = nd || mask_tap_nodata(sx[i], sy[i], w, h);
            }
    }
    const unsigned long long bal = __ballot(nd);
    if (lane == 0) {
        out[(size_t)Y * wpr + 2 * c] = (unsigned)bal;
        if (2 * c + 1 < wpr) out[(size_t)Y * wpr + 2 * c + 1] = (unsigned)(bal >> 32);
    }
}

// Step 3.  A lane per output word.  The vertical OR comes first (a word column over the window's rows; a row or a column outside the
// frame enters as all ones), then the horizontal one: the output word is the OR of the 32-bit pieces of that row at the bit offsets
// 32 wd + d, d over the window -- a funnel shift of two neighbouring column words each, which are formed again only when the offset
// crosses a word boundary.
__global__ __launch_bounds__(256) void mask_dilate_kernel(const unsigned* __restrict__ N, int H, int wpr, int pad, unsigned* __restrict__ B) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= wpr * H) return;
    const int Y = t / wpr, wd = t - Y * wpr;
    const int ylo = mask_window_lo(Y, pad), yhi = mask_window_hi(Y, pad);
    auto column = [&](int q) -> unsigned {
        if (q < 0 || q >= wpr || ylo < 0 || yhi >= H) return 0xffffffffu;
        unsigned v = 0u;
        for (int y = ylo; y <= yhi; y++) v |= N[(size_t)y * wpr + q];
        return v;
    };
    const int olo = mask_window_lo(32 * wd, pad), ohi = mask_window_hi(32 * wd, pad);
    int q = olo >> 5;  // (arithmetic shift: the floor)
    unsigned v0 = column(q), v1 = column(q + 1), out = 0u;
    for (int o = olo; o <= ohi && out != 0xffffffffu; o++) {
        if ((o >> 5) != q) {
            q = o >> 5;
            v0 = v1;
            v1 = column(q + 1);
        }
        const int sh = o & 31;
        out |= sh ? (v0 >> sh) | (v1 << (32 - sh)) : v0;
    }
    B[t] = out;
}

// one byte per pixel from the bit rows (ekfvio_get_mask, on the host)
void mask_unpack(const unsigned* words, int W, int H, uint8_t* out) {
    const int wpr = (W + 31) / 32;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) out[(size_t)y * W + x] = (words[(size_t)y * wpr + (x >> 5)] >> (x & 31)) & 1u;
}

// the window OR of one line of `len` entries with stride `st`, outside = 1, through a running count
void mask_window_or_line(const uint8_t* in, uint8_t* out, int len, size_t st, int pad, std::vector<int>& pre) {
    pre.resize((size_t)len + 1);
    pre[0] = 0;
    for (int i = 0; i < len; i++) pre[i + 1] = pre[i] + (in[i * st] ? 1 : 0);
    for (int i = 0; i < len; i++) {
        const int lo = mask_window_lo(i, pad), hi = mask_window_hi(i, pad);
        out[i * st] = (lo < 0 || hi >= len || pre[hi + 1] - pre[lo] > 0) ? 1 : 0;
    }
}

bool mask_flags_ok(int32_t flags) { return (flags & ~(int32_t)EKFVIO_MASK_RECTIFY_BORDER) == 0; }

}  // namespace

int mask_check_frame(ekfvio_filter* f, int width, int height) {
    if (!f->mask_user || (width == f->mask_uw && height == f->mask_uh)) return EKFVIO_OK;
    f->last_error = "the frame is " + std::to_string(width) + " x " + std::to_string(height) + ", the mask of ekfvio_set_mask " +
                    std::to_string(f->mask_uw) + " x " + std::to_string(f->mask_uh);
    return EKFVIO_EINVAL;
}

// The two bit planes for a w x h level 0, and the hit flags: allocated with the first frame pushed while the mask is on, regrown with a
// larger frame (push_frame_check, klt.hip: in front of the frame's first launch).
int mask_ensure(ekfvio_filter* f, int w, int h) {
    if (!f->mask_on) return EKFVIO_OK;
    const size_t words = (size_t)((w + 31) / 32) * h;
    if (words <= f->mask_cap_words && f->mask_hit) return EKFVIO_OK;
    HIP_TRY(f, hipSetDevice(f->device));
    HIP_TRY(f, hipStreamSynchronize(f->stream));  // nothing in flight may still read the old planes
    if (words > f->mask_cap_words) {
        f->mask_cap_words = 0;
        f->mask_key_valid = false;
        f->mask_bw = f->mask_bh = 0;
        HIP_TRY(f, dev_alloc_bare(f, &f->mask_nodata, words * sizeof(unsigned)));
        HIP_TRY(f, dev_alloc_bare(f, &f->mask_blocked, words * sizeof(unsigned)));
        f->mask_cap_words = words;
    }
    if (!f->mask_hit) HIP_TRY(f, dev_alloc(f, &f->mask_hit, (size_t)(f->cfg.max_features > 0 ? f->cfg.max_features : 1)));
    return EKFVIO_OK;
}

// Behind rectify_enqueue (the map is the one this frame is rectified through): B for this frame's size, formed again only if what it
// was formed for -- the rectification key where the border term is live, the caller's mask, s, pad, the size, the flags -- has changed.
void mask_enqueue(ekfvio_filter* f, int width, int height, int w, int h, int s, hipStream_t st) {
    if (!f->mask_on) {
        f->mask_bw = f->mask_bh = 0;  // off: the consumers get no B, whatever the planes still hold
        return;
    }
    const bool border = (f->mask_flags & EKFVIO_MASK_RECTIFY_BORDER) && f->rect_on;
    MaskKey key;
    memset(&key, 0, sizeof(key));
    if (border) key.rect = f->rect_key, key.rect_live = 1;
    key.user_gen = f->mask_user ? f->mask_user_gen : 0u;
    key.s = s, key.pad = mask_pad(f->cfg.kill_pad), key.w = width, key.h = height, key.flags = f->mask_flags;
    f->mask_bw = w, f->mask_bh = h;
    if (f->mask_key_valid && memcmp(&key, &f->mask_key, sizeof(key)) == 0) return;
    const int wpr = (w + 31) / 32, chunks = (wpr + 1) / 2;
    ProfScope ps(f, PC_KLT_PYRAMID, 0, 2);
    hipLaunchKernelGGL(mask_nodata_kernel, dim3((chunks * h + 3) / 4), dim3(256), 0, st, border ? f->rect_sx : (const int*)nullptr,
                       border ? f->rect_sy : (const int*)nullptr, f->mask_user, width, height, s, w, h, wpr, f->mask_nodata);
    hipLaunchKernelGGL(mask_dilate_kernel, dim3((wpr * h + 255) / 256), dim3(256), 0, st, f->mask_nodata, h, wpr, key.pad, f->mask_blocked);
    f->mask_key = key;
    f->mask_key_valid = true;
}

extern "C" {

int ekfvio_set_mask(ekfvio_filter* f, const uint8_t* mask, int32_t width, int32_t height, int32_t stride, int32_t flags) {
    if (!f || !mask_flags_ok(flags)) return EKFVIO_EINVAL;
    if (!mask && (width != 0 || height != 0 || stride != 0)) return EKFVIO_EINVAL;
    if (mask && (width < 1 || height < 1 || width > 16384 || height > 16384 || stride < width)) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    HIP_TRY(f, hipStreamSynchronize(f->stream));  // a frame in flight may still read the device copy
    if (mask) {
        const size_t px = (size_t)width * height;
        std::vector<uint8_t> packed(px);
        for (int y = 0; y < height; y++) memcpy(packed.data() + (size_t)y * width, mask + (size_t)y * stride, (size_t)width);
        uint8_t* dev = nullptr;  // the old copy stays the handle's until the new one is complete
        HIP_TRY(f, dev_alloc_bare(f, &dev, px));
        hipError_t e = hipMemcpyAsync(dev, packed.data(), px, hipMemcpyHostToDevice, f->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(f->stream);  // copied before the call returns
        if (e != hipSuccess) {
            f->mem.release(&dev);
            f->last_error = std::string("ekfvio_set_mask: ") + hipGetErrorString(e);
            return EKFVIO_EDEVICE;
        }
        f->mem.release(&f->mask_user);
        f->mask_user = dev;
        f->mask_uw = width, f->mask_uh = height;
        f->mask_user_gen++;
    } else {
        f->mem.release(&f->mask_user);
        f->mask_uw = f->mask_uh = 0;
    }
    f->mask_flags = flags;
    f->mask_on = mask != nullptr || flags != 0;  // (read by the next pushed frame; frame ingest is in no captured graph)
    return EKFVIO_OK;
}

int ekfvio_get_mask(ekfvio_filter* f, uint8_t* blocked, int32_t cap, int32_t* w, int32_t* h) {
    if (!f || cap < 0) return EKFVIO_EINVAL;
    const int W = f->mask_bw, H = f->mask_bh;
    if (w) *w = W;
    if (h) *h = H;
    if (!blocked || W == 0) return EKFVIO_OK;
    if ((size_t)cap < (size_t)W * H) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    std::vector<unsigned> words((size_t)((W + 31) / 32) * H);
    HIP_TRY(f, hipMemcpyAsync(words.data(), f->mask_blocked, words.size() * sizeof(unsigned), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    mask_unpack(words.data(), W, H, blocked);
    return EKFVIO_OK;
}

int ekfvio_get_mask_hits(ekfvio_filter* f, uint8_t* masked, int32_t* n_landmarks, int32_t* masked_last) {
    if (!f) return EKFVIO_EINVAL;
    const int n = f->mask_hit ? f->mask_hits_n : 0;
    if (n_landmarks) *n_landmarks = n;
    if (masked_last) *masked_last = 0;
    if (n == 0) return EKFVIO_OK;
    HIP_TRY(f, hipSetDevice(f->device));
    std::vector<uint8_t> hit((size_t)n);
    HIP_TRY(f, hipMemcpyAsync(hit.data(), f->mask_hit, (size_t)n, hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    int cnt = 0;
    for (int i = 0; i < n; i++) cnt += hit[i] ? 1 : 0;
    if (masked) memcpy(masked, hit.data(), (size_t)n);
    if (masked_last) *masked_last = cnt;
    return EKFVIO_OK;
}

// B on the host, by the three steps as they are written: n per full-size pixel (the map entry from rectify_map_entry, the taps from
// mask_tap_nodata), N per s x s block, then the window OR along rows and along columns (an OR over a rectangle is separable).
int ekfvio_mask_blocked_model(const float K[9], int32_t model, const double* D, int32_t count, const float P[4], const uint8_t* mask, int32_t width,
                              int32_t height, int32_t stride, int32_t inverse_image_scale, int32_t kill_pad, int32_t flags, uint8_t* blocked) {
    double d[8];
    if (!blocked || !mask_flags_ok(flags) || width < 1 || height < 1 || width > 16384 || height > 16384 || (mask && stride < width) ||
        !rectify_model_arguments(model, D, count, P, d))
        return EKFVIO_EINVAL;
    const int s = inverse_image_scale > 1 ? inverse_image_scale : 1, pad = mask_pad(kill_pad);
    const int W = width / s, H = height / s;
    if (W < 1 || H < 1) return EKFVIO_EINVAL;
    const bool border = rectify_model_on(model, d, P) && (flags & EKFVIO_MASK_RECTIFY_BORDER);  // live as on the handle: flag set and the setting on
    if (border && !K) return EKFVIO_EINVAL;
    RectifyCam cam;
    memset(&cam, 0, sizeof(cam));
    if (border) cam = rectify_cam(K, model, d, P);
    std::vector<uint8_t> N((size_t)W * H, 0), Bh((size_t)W * H);
    for (int Y = 0; Y < H; Y++)
        for (int X = 0; X < W; X++) {
            bool nd = false;
            for (int dy = 0; dy < s && !nd; dy++)
                for (int dx = 0; dx < s && !nd; dx++) {
                    const int x = s * X + dx, y = s * Y + dy;
                    if (mask) nd = nd || mask[(size_t)y * stride + x] == 0;
                    if (border && !nd) {
                        int vx, vy;
                        rectify_map_entry_of(model, cam, x, y, &vx, &vy);
                        nd = mask_tap_nodata(vx, vy, width, height);
                    }
                }
            N[(size_t)Y * W + X] = nd ? 1 : 0;
        }
    std::vector<int> pre;
    for (int Y = 0; Y < H; Y++) mask_window_or_line(N.data() + (size_t)Y * W, Bh.data() + (size_t)Y * W, W, 1, pad, pre);
    for (int X = 0; X < W; X++) mask_window_or_line(Bh.data() + X, blocked + X, H, (size_t)W, pad, pre);
    return EKFVIO_OK;
}

// the plumb_bob, no-P case
int ekfvio_mask_blocked(const float K[9], const double* D, int32_t count, const uint8_t* mask, int32_t width, int32_t height, int32_t stride,
                        int32_t inverse_image_scale, int32_t kill_pad, int32_t flags, uint8_t* blocked) {
    return ekfvio_mask_blocked_model(K, EKFVIO_CAMERA_PLUMB_BOB, D, count, nullptr, mask, width, height, stride, inverse_image_scale, kill_pad, flags,
                                     blocked);
}

}  // extern "C"
