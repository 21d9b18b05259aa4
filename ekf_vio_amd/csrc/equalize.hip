// ekf_vio_amd/csrc/equalize.hip — clip-limited tile histogram equalisation of a pushed frame on the device, between its rectification
// (or its upload) and the pyramid.
//
// What VINS-style front ends run on the host in front of their tracker (a cv::CLAHE pass); the reference has no photometric stage at all
// (FAST at a fixed threshold, EKFVIO.cpp:224-311, Lucas-Kanade without gain or offset).  The arithmetic is specified line by line in
// include/ekfvio.h (ekfvio_set_equalize): equalize.h is those lines, compiled for the host (ekfvio_equalize) and for the device out of the
// same inline functions, so that both give the bits of a NumPy restatement (tests/_equalize.py).
//
// Kernels: equalize_lut_kernel forms one 256-byte table per tile (one workgroup each); equalize_apply_kernel then rewrites the frame IN
// PLACE through the four tables around each pixel.  In place is sound: each lane reads its own four pixels as one dword and writes that
// dword back, nothing else reads the plane in that launch, and the table kernel has finished with it (stream order).  So the setting costs
// tx * ty * 256 bytes of device memory and no second plane.  With the setting off neither is launched and nothing is allocated.
#include <math.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "equalize.h"

namespace {

// One workgroup of 256 lanes per tile; src is the full-size frame as ONE run of w * h bytes (no pitch) with at least 3 bytes of slack
// behind it (the staging planes have 16).
//  1. Histogram: one private copy per wavefront in LDS, one LDS atomic per pixel.  (Built and dropped: a wavefront-level test in front of the
//     atomic -- two ballots and a lane read; a wavefront whose lanes all hold one value, as every wavefront of a flat region does, then sends
//     ONE atomic with the lane count.  On a constant 640 x 480 frame, the contention worst case, this kernel measured 6.99 us with the test
//     and 7.02 us without: the LDS does not serialise same-address atomics of a wavefront the way the test assumed.  On the textured
//     fixture the test cost 1.0 us, 6.76 against 5.76 us.  profiles/equalize_timing.txt.)  The tile's in-frame part of a row is read as
//     ALIGNED dwords -- the row's first byte sits at any alignment (y * w + i * tw), so the first and last dword of a row are masked by
//     position -- and the reflected columns (the last tile columns only) by single bytes.  Rows below the frame are reflected rows, read
//     the same way.
//  2. One bin per lane: the four copies merged, the clip, `excess` by a wavefront shuffle reduction and one LDS hop, the redistribution in
//     the closed form of equalize_bin, an inclusive scan (shuffles within the wavefront, one LDS hop across the four), the table byte.
__global__ __launch_bounds__(256) void equalize_lut_kernel(const uint8_t* __restrict__ src, int w, int h, EqualizeParams p, uint8_t* __restrict__ lut) {
    __shared__ unsigned s_hist[4][256];
    __shared__ int s_excess[4], s_total[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tile = blockIdx.x, ti = tile % p.tx, tj = tile / p.tx;
#pragma unroll
    for (int k = 0; k < 4; k++) s_hist[k][tid] = 0u;
    __syncthreads();
    unsigned* hist = s_hist[wv];
    const int x0 = ti * p.tw, y0 = tj * p.th;
    const int n_in = min(max(w - x0, 0), p.tw);  // the tile's columns inside the frame; the other tw - n_in are reflected ones
    const unsigned* __restrict__ src32 = reinterpret_cast<const unsigned*>(src);
    if (n_in > 0) {
        const int ndmax = (p.tw + 3) / 4 + 1;  // dwords a row's in-frame part can touch
        const int total = p.th * ndmax;
        for (int item = tid; item < total; item += 256) {
            const int r = item / ndmax, k = item - r * ndmax;
            const int sy = equalize_reflect(y0 + r, h);
            const int base = sy * w + x0, end = base + n_in;  // (w * h <= 2^28)
            const int d = (base >> 2) + k;
            if (4 * d >= end) continue;  // (a row that touches fewer than ndmax dwords)
            const unsigned word = src32[d];
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int pos = 4 * d + b;
                if (pos >= base && pos < end) atomicAdd(&hist[(word >> (8 * b)) & 255u], 1u);
            }
        }
    }
    const int n_tail = p.tw - n_in;
    if (n_tail > 0) {
        const int total = p.th * n_tail;
        for (int item = tid; item < total; item += 256) {
            const int r = item / n_tail, c = item - r * n_tail;
            const int sy = equalize_reflect(y0 + r, h);
            const int sx = equalize_reflect(x0 + n_in + c, w);
            atomicAdd(&hist[src[(size_t)sy * w + sx]], 1u);
        }
    }
    __syncthreads();
    const int hsum = (int)(s_hist[0][tid] + s_hist[1][tid] + s_hist[2][tid] + s_hist[3][tid]);
    int ex = equalize_excess(hsum, p.clip);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ex += __shfl_xor(ex, off);
    if (lane == 0) s_excess[wv] = ex;
    __syncthreads();
    const EqualizeSpread sp = equalize_spread(s_excess[0] + s_excess[1] + s_excess[2] + s_excess[3]);
    int cum = equalize_bin(hsum, p.clip, sp, tid);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(cum, off);
        if (lane >= off) cum += up;
    }
    if (lane == 63) s_total[wv] = cum;
    __syncthreads();
    for (int k = 0; k < wv; k++) cum += s_total[k];
    lut[(size_t)tile * 256 + tid] = equalize_lut_byte(cum, p.scale);
}

// Four consecutive pixels per lane, one dword in and the same dword out (img is read and written in place), in the shape of
// rectify_kernel.  n4 = ceil(w h / 4); the lanes' pixels behind the frame's last one fall into the plane's slack.  The sixteen table bytes
// of a lane are all requested before the first is used.
__device__ __forceinline__ void equalize_apply_lane(unsigned* img, int i, int w, int h, const EqualizeParams& p, const uint8_t* __restrict__ lut) {
    const unsigned word = img[i];
    int y = (4 * i) / w, x = 4 * i - y * w;
    EqualizeAxis ax[4], ay[4];
    int l[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int v = (int)((word >> (8 * k)) & 255u);
        ax[k] = equalize_axis(x, p.inv_tw, p.tx);
        ay[k] = equalize_axis(min(y, h - 1), p.inv_th, p.ty);
        const uint8_t* r1 = lut + (size_t)ay[k].i1 * p.tx * 256 + v;
        const uint8_t* r2 = lut + (size_t)ay[k].i2 * p.tx * 256 + v;
        l[k][0] = r1[ax[k].i1 * 256], l[k][1] = r1[ax[k].i2 * 256], l[k][2] = r2[ax[k].i1 * 256], l[k][3] = r2[ax[k].i2 * 256];
        if (++x == w) x = 0, y++;
    }
    unsigned out = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) out |= (unsigned)equalize_blend(l[k][0], l[k][1], l[k][2], l[k][3], ax[k], ay[k]) << (8 * k);
    img[i] = out;
}
// The table bytes come from global memory: the whole table is at most 64 KiB and stays in L2.  (Built and dropped: every workgroup whose 1024
// pixels touch at most three tile rows copies those rows' tables, at most 12 KiB, into LDS and reads its bytes from there.  640 x 480 at
// (3, 8, 8): 4.94 us against 4.91 us from L2, 4.79 against 4.80 on a constant frame, the image loop's frames/s within each other's range.
// profiles/equalize_timing.txt.)
__global__ __launch_bounds__(256) void equalize_apply_kernel(unsigned* img, int w, int h, int n4, EqualizeParams p, const uint8_t* __restrict__ lut) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n4) equalize_apply_lane(img, i, w, h, p, lut);
}

}  // namespace

// EKFVIO_EINVAL (and last_error) for a frame with fewer columns than tiles_x or fewer rows than tiles_y while the setting is on
int equalize_check_frame(ekfvio_filter* f, int width, int height) {
    if (!f->eq_on || (width >= f->eq_tx && height >= f->eq_ty)) return EKFVIO_OK;
    f->last_error = "frame " + std::to_string(width) + " x " + std::to_string(height) + " is smaller than the equalisation's " +
                    std::to_string(f->eq_tx) + " x " + std::to_string(f->eq_ty) + " tiles (ekfvio_set_equalize)";
    return EKFVIO_EINVAL;
}

// The tables (ensure_frame_capacity, klt.hip, which has waited for the stream): allocated when the first frame arrives with the setting
// on, regrown for a setting with more tiles.
int equalize_ensure(ekfvio_filter* f) {
    const size_t bytes = f->eq_on ? (size_t)f->eq_tx * f->eq_ty * 256 : 0;
    if (bytes <= f->eq_lut_cap) return EKFVIO_OK;
    f->eq_lut_cap = 0;
    HIP_TRY(f, dev_alloc_bare(f, &f->eq_lut, bytes));
    f->eq_lut_cap = bytes;
    return EKFVIO_OK;
}

// full (w x h, tightly packed, the upload staging or the rectified plane) is equalised in place
void equalize_enqueue(ekfvio_filter* f, uint8_t* full, int w, int h, hipStream_t st) {
    const EqualizeParams p = equalize_params(w, h, f->eq_clip, f->eq_tx, f->eq_ty);
    const int n4 = (w * h + 3) / 4;
    ProfScope ps(f, PC_KLT_PYRAMID, 0, 2);
    hipLaunchKernelGGL(equalize_lut_kernel, dim3(p.tx * p.ty), dim3(256), 0, st, full, w, h, p, f->eq_lut);
    hipLaunchKernelGGL(equalize_apply_kernel, dim3((n4 + 255) / 256), dim3(256), 0, st, reinterpret_cast<unsigned*>(full), w, h, n4, p, f->eq_lut);
}

extern "C" {

int ekfvio_set_equalize(ekfvio_filter* f, float clip_limit, int32_t tiles_x, int32_t tiles_y) {
    if (!f) return EKFVIO_EINVAL;
    if (clip_limit == 0.f) {  // off: the tile counts are not looked at
        f->eq_on = false;
        return EKFVIO_OK;
    }
    if (!equalize_setting_ok(clip_limit, tiles_x, tiles_y)) return EKFVIO_EINVAL;
    f->eq_clip = clip_limit, f->eq_tx = tiles_x, f->eq_ty = tiles_y;
    f->eq_on = true;  // (read by the next pushed frame; frame ingest is in no captured graph)
    return EKFVIO_OK;
}

// The five steps on the host, as they are written: per tile the histogram of the reflected source, the clip and the redistribution, the
// table; then per pixel the blend of four tables.  out may be the image itself only if nothing else is: the tables are complete first.
int ekfvio_equalize(const uint8_t* image, int32_t width, int32_t height, int32_t stride, float clip_limit, int32_t tiles_x, int32_t tiles_y,
                    uint8_t* out) {
    if (!image || !out || width < 1 || height < 1 || width > 16384 || height > 16384 || stride < width) return EKFVIO_EINVAL;
    if (!equalize_setting_ok(clip_limit, tiles_x, tiles_y) || width < tiles_x || height < tiles_y) return EKFVIO_EINVAL;
    const EqualizeParams p = equalize_params(width, height, clip_limit, tiles_x, tiles_y);
    std::vector<uint8_t> lut((size_t)p.tx * p.ty * 256);
    for (int tj = 0; tj < p.ty; tj++)
        for (int ti = 0; ti < p.tx; ti++) {
            int hist[256] = {0};
            for (int Y = tj * p.th; Y < (tj + 1) * p.th; Y++)
                for (int X = ti * p.tw; X < (ti + 1) * p.tw; X++)
                    hist[image[(size_t)equalize_reflect(Y, height) * stride + equalize_reflect(X, width)]]++;
            int excess = 0;
            for (int b = 0; b < 256; b++) excess += equalize_excess(hist[b], p.clip);
            const EqualizeSpread sp = equalize_spread(excess);
            int cum = 0;
            uint8_t* t = lut.data() + ((size_t)tj * p.tx + ti) * 256;
            for (int b = 0; b < 256; b++) {
                cum += equalize_bin(hist[b], p.clip, sp, b);
                t[b] = equalize_lut_byte(cum, p.scale);
            }
        }
    std::vector<EqualizeAxis> axs((size_t)width);
    for (int x = 0; x < width; x++) axs[x] = equalize_axis(x, p.inv_tw, p.tx);
    for (int y = 0; y < height; y++) {
        const EqualizeAxis ay = equalize_axis(y, p.inv_th, p.ty);
        const uint8_t* r1 = lut.data() + (size_t)ay.i1 * p.tx * 256;
        const uint8_t* r2 = lut.data() + (size_t)ay.i2 * p.tx * 256;
        for (int x = 0; x < width; x++) {
            const EqualizeAxis& ax = axs[x];
            const int v = image[(size_t)y * stride + x];
            out[(size_t)y * width + x] = equalize_blend(r1[ax.i1 * 256 + v], r1[ax.i2 * 256 + v], r2[ax.i1 * 256 + v], r2[ax.i2 * 256 + v], ax, ay);
        }
    }
    return EKFVIO_OK;
}

}  // extern "C"
