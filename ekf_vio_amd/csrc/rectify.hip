// ekf_vio_amd/csrc/rectify.hip — rectification of distorted frames on the device, between a frame's upload and its pyramid.
//
// What a deployment of the reference runs in front of the node (image_proc/rectify: cv::initUndistortRectifyMap with R = I and the new
// camera matrix = K, then cv::remap(INTER_LINEAR, BORDER_CONSTANT 0)); the reference itself assumes a pinhole image (Frame.h:31, its D at
// :32 is never read; EKFVIO.cpp:429 "TODO add distortion coeffs").  The arithmetic is specified line by line in include/ekfvio.h
// (ekfvio_set_distortion; ekfvio_set_camera_model for the rational and the equidistant lens and for a rectified camera P of its own):
// rectify_map_entry (rectify_map.h) is that block, compiled for the host (ekfvio_rectify_map, ekfvio_rectify_map_model) and for the device
// (rectify_map_kernel) out of the same lines, in fp64 without contraction, so that both give the bits of a NumPy restatement.
//
// Kernels: rectify_map_kernel, one instance per camera model, writes the two fixed-point planes (once per camera: the host keeps the key
// it was formed for; the lens model lives in the map alone, so what reads the planes is the same code for every lens);
// rectify_kernel reads the uploaded frame through them and writes a second staging plane, which the pyramid kernel is then given in
// place of the first.  With distortion off neither is launched and nothing is allocated.
#include <math.h>
#include <string.h>

#include "common.h"
#include "rectify_map.h"  // RectifyCam, rectify_map_entry: the specification's fp64 block, shared with mask.hip

namespace {

// The frame as ONE run of w * h pixels, the planes likewise (no pitch: every row of four entries is 16-byte aligned whatever the
// width).  n4 = ceil(w h / 4) lanes' worth of entries are written; those behind the frame's last pixel hold the sentinel.
template <int MODEL>
__global__ __launch_bounds__(256) void rectify_map_kernel(RectifyCam c, int w, int npix, int n4, int* __restrict__ sx, int* __restrict__ sy) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 4 * n4) return;
    int vx = INT32_MIN, vy = INT32_MIN;
    if (i < npix) rectify_map_entry<MODEL>(c, i % w, i / w, &vx, &vy);
    sx[i] = vx;
    sy[i] = vy;
}

// Four consecutive destination pixels per lane: the map arrives as two 16-byte loads per lane (a wavefront reads 2 x 1 KiB in a row),
// the result leaves as one dword.  The taps are single bytes of the uploaded frame, which neighbouring lanes share and L2 holds (a
// 640 x 480 frame is 300 KB): all sixteen of a lane are requested from clamped addresses before the first is used, and a tap outside
// the frame is multiplied by zero instead of branched around.
__global__ __launch_bounds__(256) void rectify_kernel(const uint8_t* __restrict__ src, int w, int h, int n4, const int4* __restrict__ sx4,
                                                      const int4* __restrict__ sy4, unsigned* __restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int4 mx = sx4[i], my = sy4[i];
    const int sxs[4] = {mx.x, mx.y, mx.z, mx.w}, sys[4] = {my.x, my.y, my.z, my.w};
    int t[4][4], wt[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ix = sxs[k] >> 5, ax = sxs[k] & 31, iy = sys[k] >> 5, ay = sys[k] & 31;
        const bool x0 = ix >= 0 && ix < w, x1 = ix + 1 >= 0 && ix + 1 < w, y0 = iy >= 0 && iy < h, y1 = iy + 1 >= 0 && iy + 1 < h;
        const int cx0 = min(max(ix, 0), w - 1), cx1 = min(max(ix + 1, 0), w - 1);
        const size_t r0 = (size_t)min(max(iy, 0), h - 1) * w, r1 = (size_t)min(max(iy + 1, 0), h - 1) * w;
        t[k][0] = src[r0 + cx0], t[k][1] = src[r0 + cx1], t[k][2] = src[r1 + cx0], t[k][3] = src[r1 + cx1];
        wt[k][0] = (x0 && y0) ? (32 - ax) * (32 - ay) : 0;
        wt[k][1] = (x1 && y0) ? ax * (32 - ay) : 0;
        wt[k][2] = (x0 && y1) ? (32 - ax) * ay : 0;
        wt[k][3] = (x1 && y1) ? ax * ay : 0;
    }
    unsigned out = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int sum = t[k][0] * wt[k][0] + t[k][1] * wt[k][1] + t[k][2] * wt[k][2] + t[k][3] * wt[k][3];
        out |= (unsigned)((sum + 512) >> 10) << (8 * k);  // at most 255 * 1024 + 512: a byte
    }
    dst[i] = out;
}

}  // namespace

// The planes and the second staging buffer for an uploaded frame of `src` bytes (ensure_frame_capacity, klt.hip, which has waited
// for the stream): allocated when the first frame arrives with distortion on, regrown with a larger frame.
int rectify_ensure(ekfvio_filter* f, size_t src) {
    if (!f->rect_on || src <= f->rect_cap) return EKFVIO_OK;
    // the old planes go before the new ones come, and with them the map they held
    f->mem.release(&f->rect_sx), f->mem.release(&f->rect_sy), f->mem.release(&f->rect_img);
    f->rect_cap = 0;
    f->rect_key_valid = false;
    // (+16: the kernels move whole groups of four entries, and the pyramid's source has the slack of the upload staging)
    HIP_TRY(f, dev_alloc_bare(f, &f->rect_sx, sizeof(int) * (src + 16)));
    HIP_TRY(f, dev_alloc_bare(f, &f->rect_sy, sizeof(int) * (src + 16)));
    HIP_TRY(f, dev_alloc_bare(f, &f->rect_img, src + 16));
    f->rect_cap = src;
    return EKFVIO_OK;
}

// staging (w x h, tightly packed) -> the rectified frame, which is returned: what build_pyramid reads in its place.  The map is
// formed first if the camera, the coefficients or the size are not the ones it was formed for (compared as bits).
const uint8_t* rectify_enqueue(ekfvio_filter* f, const uint8_t* src, int w, int h, const float K[9], hipStream_t st) {
    RectifyKey key;
    memset(&key, 0, sizeof(key));
    key.K[0] = K[0], key.K[1] = K[2], key.K[2] = K[4], key.K[3] = K[5];
    for (int i = 0; i < 8; i++) key.D[i] = f->dist[i];
    key.model = f->cam_model, key.has_P = f->cam_has_P ? 1 : 0;
    if (f->cam_has_P)
        for (int i = 0; i < 4; i++) key.P[i] = f->cam_P[i];
    key.w = w, key.h = h;
    const int npix = w * h, n4 = (npix + 3) / 4;
    ProfScope ps(f, PC_KLT_PYRAMID);
    if (!f->rect_key_valid || memcmp(&key, &f->rect_key, sizeof(key)) != 0) {
        // one instance per model; the plumb_bob one with or without P (without: K twice)
        const RectifyCam cam = rectify_cam(K, f->cam_model, f->dist, f->cam_has_P ? f->cam_P : nullptr);
        const dim3 grid((4 * n4 + 255) / 256), block(256);
        if (f->cam_model == EKFVIO_CAMERA_EQUIDISTANT)
            hipLaunchKernelGGL(rectify_map_kernel<EKFVIO_CAMERA_EQUIDISTANT>, grid, block, 0, st, cam, w, npix, n4, f->rect_sx, f->rect_sy);
        else if (f->cam_model == EKFVIO_CAMERA_RATIONAL)
            hipLaunchKernelGGL(rectify_map_kernel<EKFVIO_CAMERA_RATIONAL>, grid, block, 0, st, cam, w, npix, n4, f->rect_sx, f->rect_sy);
        else
            hipLaunchKernelGGL(rectify_map_kernel<EKFVIO_CAMERA_PLUMB_BOB>, grid, block, 0, st, cam, w, npix, n4, f->rect_sx, f->rect_sy);
        f->rect_key = key;
        f->rect_key_valid = true;
        ps.launches = 2;
    }
    hipLaunchKernelGGL(rectify_kernel, dim3((n4 + 255) / 256), dim3(256), 0, st, src, w, h, n4, reinterpret_cast<const int4*>(f->rect_sx),
                       reinterpret_cast<const int4*>(f->rect_sy), reinterpret_cast<unsigned*>(f->rect_img));
    return f->rect_img;
}

namespace {

// the one setter behind ekfvio_set_distortion and ekfvio_set_camera_model (the last call wins)
int set_camera_model(ekfvio_filter* f, int32_t model, const double* D, int32_t count, const float* P) {
    double d[8];
    if (!f || !rectify_model_arguments(model, D, count, P, d)) return EKFVIO_EINVAL;
    for (int i = 0; i < 8; i++) f->dist[i] = d[i];
    f->dist_count = count, f->cam_model = model;
    f->cam_has_P = P != nullptr;
    for (int i = 0; i < 4; i++) f->cam_P[i] = P ? P[i] : 0.f;
    f->rect_on = rectify_model_on(model, d, P);  // (read by the next pushed frame; frame ingest is in no captured graph)
    return EKFVIO_OK;
}

int rectify_map_host(const float K[9], int32_t model, const double D[8], const float* P, int32_t width, int32_t height, int32_t* sx, int32_t* sy) {
    const RectifyCam c = rectify_cam(K, model, D, P);
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            int vx, vy;
            rectify_map_entry_of(model, c, x, y, &vx, &vy);
            sx[(size_t)y * width + x] = vx;
            sy[(size_t)y * width + x] = vy;
        }
    return EKFVIO_OK;
}

}  // namespace

extern "C" {

int ekfvio_set_distortion(ekfvio_filter* f, const double* D, int32_t count) {
    return set_camera_model(f, EKFVIO_CAMERA_PLUMB_BOB, D, count, nullptr);  // the plumb_bob, no-P case
}

int ekfvio_set_camera_model(ekfvio_filter* f, int32_t model, const double* D, int32_t count, const float P[4]) {
    return set_camera_model(f, model, D, count, P);
}

int ekfvio_get_camera_model(ekfvio_filter* f, int32_t* model, double D[8], int32_t* count, float P[4], int32_t* has_P, int32_t* on) {
    if (!f) return EKFVIO_EINVAL;
    if (model) *model = f->cam_model;
    if (D)
        for (int i = 0; i < 8; i++) D[i] = f->dist[i];
    if (count) *count = f->dist_count;
    if (P)
        for (int i = 0; i < 4; i++) P[i] = f->cam_P[i];
    if (has_P) *has_P = f->cam_has_P ? 1 : 0;
    if (on) *on = f->rect_on ? 1 : 0;
    return EKFVIO_OK;
}

int ekfvio_rectify_map(const float K[9], const double* D, int32_t count, int32_t width, int32_t height, int32_t* sx, int32_t* sy) {
    double d[8];
    if (!K || !sx || !sy || width < 1 || height < 1 || width > 16384 || height > 16384 || !rectify_coefficients(D, count, d)) return EKFVIO_EINVAL;
    return rectify_map_host(K, EKFVIO_CAMERA_PLUMB_BOB, d, nullptr, width, height, sx, sy);
}

int ekfvio_rectify_map_model(const float K[9], int32_t model, const double* D, int32_t count, const float P[4], int32_t width, int32_t height,
                             int32_t* sx, int32_t* sy) {
    double d[8];
    if (!K || !sx || !sy || width < 1 || height < 1 || width > 16384 || height > 16384 || !rectify_model_arguments(model, D, count, P, d))
        return EKFVIO_EINVAL;
    return rectify_map_host(K, model, d, P, width, height, sx, sy);
}

#ifdef EKFVIO_TEST_HOOKS  // include/ekfvio_test_hooks.h: only in libekfvio_hip_hooks.so
int ekfvio_test_rectify_map(ekfvio_filter* f, int32_t* sx, int32_t* sy, int32_t cap, int32_t* w, int32_t* h) {
    if (!f || cap < 0) return EKFVIO_EINVAL;
    if (!f->rect_key_valid) return EKFVIO_ESTATE;
    const int W = f->rect_key.w, H = f->rect_key.h;
    if (w) *w = W;
    if (h) *h = H;
    if (!sx || !sy) return EKFVIO_OK;
    const size_t n = (size_t)W * H;
    if ((size_t)cap < n || n > f->rect_cap) return EKFVIO_EINVAL;
    HIP_TRY(f, hipSetDevice(f->device));
    HIP_TRY(f, hipMemcpyAsync(sx, f->rect_sx, n * sizeof(int), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipMemcpyAsync(sy, f->rect_sy, n * sizeof(int), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    return EKFVIO_OK;
}
#endif

}  // extern "C"
