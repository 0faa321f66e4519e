// letterbox_area.hip -- the detection input path: letterbox of cached uint8 images of any size into a batch of any size, minifying by
// area averaging on the device.  One upload of the original pixels serves every network size (detect.py --multi-scale); the output is the
// engines' input layout (bf16 [N][H][W][8], channels 3..7 zero: an NHWC8Batch), as csrc/augment.hip makes it.
//
// DEFINITION (include/ryolo.h: ryolo_letterbox_area; restated in float64 by tests/letterbox_area_reference.py).  The unit is built with
// -ffp-contract=off and IEEE divide, so the operations below are the operations executed.
//
//   Slot n shows cached image src_index[n] (h x w) resized to new_w x new_h with its top left corner at (left, top): place[n] = (left, top,
//   new_w, new_h).  Output pixel (x, y) with left <= x < left + new_w and top <= y < top + new_h is inside the picture; every other pixel,
//   and every pixel of a slot whose src_index is outside [0, n_cache), is 128.  A hard edge, as cv2.copyMakeBorder makes it.
//
//   Each axis (source length s, output length n, output index k = x - left or y - top) has a list of taps i_0 < i_1 < .. with INTEGER
//   weights W_t that sum to a divisor D:
//     n <  s   exact coverage of the source interval [k s, (k + 1) s) in units of 1/n source pixel: taps i = (k s) div n while i n < (k + 1) s,
//              W = min((k + 1) s, (i + 1) n) - max(k s, i n),  D = s.  64-bit integers.
//     n >= s   bilinear with aligned pixel centres: c = (2 k + 1) s - n, q = floor(c / (2 n)), r = c - 2 n q in [0, 2 n): taps q and q + 1, each
//              clamped to [0, s - 1], W = (2 n - r, r), D = 2 n.  n == s gives r = 0: the pixel itself.
//   Per channel, in fp32, with p the source byte as a float and every sum taken from the first tap up, starting from that tap's product:
//     row_j = (sum_t float(Wx_t) * p[iy_j][ix_t]) / float(Dx)                 (0..255 scale)
//     v     = (sum_j float(Wy_j) * row_j) / float(Dy)                         (0..255 scale, never rounded to uint8)
//     out   = bf16_rne(v / 255.0f)
//   Channels 3..7 are zero; one 16-byte store per pixel.
//
//   float(W) * p is exact (both are small integers) and so is the row sum while 255 s < 2^24; n == s on both axes therefore gives
//   p / 255.0f exactly, and a 2:1 reduction the exact mean of the 2 x 2 block.
//
// SHAPE.  As augment.hip: 256-thread workgroups own a 32 x 32 output tile of one slot, thread -> column tid % 32, rows tid / 32 + 8 j, so a
// wave stores two full 512-byte row segments.  The tap lists depend on the column alone (x) or the row alone (y): the first wave works the
// 32 + 32 of them out once per tile (the 64-bit divisions live there) and leaves (first tap, count, first weight, last weight, divisor) in
// LDS -- 1.25 KiB; every weight between the first and the last is n.  The pixel loop then is byte loads, converts, multiplies and adds.
// Neighbouring lanes read neighbouring runs of a source row, so a wave's loads of one row are one contiguous run of 32 * 3 * s / n bytes.
// place is HOST memory: it is validated before anything is enqueued and travels in the kernel arguments, 64 slots per launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ryolo.h"

namespace {

constexpr int TILE = 32, CHUNK = 64;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct Places { int v[CHUNK][4]; };
struct Taps { int i0, cnt, wf, wl, D; };      // taps i0 .. i0 + cnt - 1 (clamped), weights wf, mid, .., mid, wl

__device__ __forceinline__ Taps make_taps(int k, int s, int n) {
    Taps t;
    if (n < s) {
        const long long lo = (long long)k * s, end = lo + s;
        const long long i0 = lo / n, i1 = (end - 1) / n;
        t.i0 = (int)i0;
        t.cnt = (int)(i1 - i0) + 1;
        const long long first_hi = (i0 + 1) * n < end ? (i0 + 1) * n : end;
        t.wf = (int)(first_hi - lo);
        t.wl = (int)(end - (i1 * n > lo ? i1 * n : lo));
        t.D = s;
    } else {
        const long long c = (2LL * k + 1) * s - n, d = 2LL * n;
        const long long q = c >= 0 ? c / d : -((-c + d - 1) / d);
        const int r = (int)(c - q * d);
        t.i0 = (int)q;
        t.cnt = 2;
        t.wf = (int)d - r;
        t.wl = r;
        t.D = (int)d;
    }
    return t;
}

__device__ __forceinline__ int clampi(int i, int hi) { return i < 0 ? 0 : (i > hi ? hi : i); }

__device__ __forceinline__ void store_px(__bf16 *y, size_t pix, float r, float g, float b) {
    bf16x8 o;
    o[0] = (__bf16)(r / 255.0f);
    o[1] = (__bf16)(g / 255.0f);
    o[2] = (__bf16)(b / 255.0f);
#pragma unroll
    for (int e = 3; e < 8; e++) o[e] = (__bf16)0.f;
    *(bf16x8 *)(y + pix * 8) = o;
}

__global__ __launch_bounds__(256) void letterbox_area_kernel(const uint8_t *__restrict__ pixels, const long long *__restrict__ img_offset,
                                                             const int *__restrict__ img_hw, int n_cache,
                                                             const int *__restrict__ src_index, Places places, int H, int W,
                                                             __bf16 *__restrict__ y) {
    __shared__ Taps tx[TILE], ty[TILE];
    const int n = blockIdx.z, x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE, tid = threadIdx.x;
    const int left = places.v[n][0], top = places.v[n][1];
    int new_w = places.v[n][2], new_h = places.v[n][3];
    const int s = src_index[n];
    const uint8_t *src = pixels;
    int h = 0, w = 0;
    if (s >= 0 && s < n_cache) {
        src = pixels + img_offset[s];
        h = img_hw[2 * s];
        w = img_hw[2 * s + 1];
    }
    if (h < 1 || w < 1) new_w = new_h = 0;      // nothing to read: the slot is all border
    const size_t img_base = (size_t)n * H * W;
    // does this tile touch the picture at all?  (uniform over the workgroup)
    const bool touches = new_w > 0 && x0 < left + new_w && x0 + TILE > left && y0 < top + new_h && y0 + TILE > top;
    if (touches) {
        if (tid < TILE) {
            const int k = x0 + tid - left;
            if (k >= 0 && k < new_w) tx[tid] = make_taps(k, w, new_w);
        } else if (tid < 2 * TILE) {
            const int k = y0 + tid - TILE - top;
            if (k >= 0 && k < new_h) ty[tid - TILE] = make_taps(k, h, new_h);
        }
        __syncthreads();
    }
    const int lx = tid & 31, gx = x0 + lx;
    if (gx >= W) return;
    const bool in_x = touches && gx >= left && gx < left + new_w;
    Taps ax{0, 0, 0, 0, 1};
    if (in_x) ax = tx[lx];
    const float Dx = (float)ax.D;
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
        const int ly = (tid >> 5) + 8 * j, gy = y0 + ly;
        if (gy >= H) break;
        const size_t pix = img_base + (size_t)gy * W + gx;
        if (!(in_x && gy >= top && gy < top + new_h)) {
            store_px(y, pix, 128.f, 128.f, 128.f);
            continue;
        }
        const Taps ay = ty[ly];
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
        for (int a = 0; a < ay.cnt; a++) {
            const int iy = clampi(ay.i0 + a, h - 1);
            const float wy = (float)(a == 0 ? ay.wf : (a == ay.cnt - 1 ? ay.wl : new_h));
            const uint8_t *row = src + (size_t)iy * w * 3;
            float r0 = 0.f, r1 = 0.f, r2 = 0.f;
            for (int b = 0; b < ax.cnt; b++) {
                const int ix = clampi(ax.i0 + b, w - 1);
                const float wx = (float)(b == 0 ? ax.wf : (b == ax.cnt - 1 ? ax.wl : new_w));
                const uint8_t *p = row + (size_t)ix * 3;
                r0 += wx * (float)p[0];
                r1 += wx * (float)p[1];
                r2 += wx * (float)p[2];
            }
            v0 += wy * (r0 / Dx);
            v1 += wy * (r1 / Dx);
            v2 += wy * (r2 / Dx);
        }
        const float Dy = (float)ay.D;
        store_px(y, pix, v0 / Dy, v1 / Dy, v2 / Dy);
    }
}

}  // namespace

extern "C" {

int ryolo_letterbox_area(const uint8_t *pixels, const long long *img_offset, const int *img_hw, int n_cache, const int *src_index,
                         const int *place, int N, int H, int W, void *y, void *stream) {
    if (!pixels || !img_offset || !img_hw || !src_index || !place || !y || N < 1 || H < 1 || W < 1 || n_cache < 1) return RYOLO_EINVAL;
    if (N > 65535 || (H + TILE - 1) / TILE > 65535 || ((uintptr_t)y & 15)) return RYOLO_EINVAL;
    for (int n = 0; n < N; n++) {
        const long long left = place[4 * n], top = place[4 * n + 1], nw = place[4 * n + 2], nh = place[4 * n + 3];
        if (nw < 1 || nh < 1 || left < 0 || top < 0 || left + nw > W || top + nh > H) return RYOLO_EINVAL;
    }
    for (int n0 = 0; n0 < N; n0 += CHUNK) {
        const int cnt = N - n0 < CHUNK ? N - n0 : CHUNK;
        Places pl;
        for (int i = 0; i < cnt * 4; i++) pl.v[i / 4][i % 4] = place[4 * n0 + i];
        for (int i = cnt * 4; i < CHUNK * 4; i++) pl.v[i / 4][i % 4] = 0;
        const dim3 grid((W + TILE - 1) / TILE, (H + TILE - 1) / TILE, cnt);
        hipLaunchKernelGGL(letterbox_area_kernel, grid, dim3(256), 0, (hipStream_t)stream, pixels, img_offset, img_hw, n_cache,
                           src_index + n0, pl, H, W, (__bf16 *)y + (size_t)n0 * H * W * 8);
        if (hipGetLastError() != hipSuccess) return RYOLO_ELAUNCH;
    }
    return RYOLO_OK;
}

}  // extern "C"
