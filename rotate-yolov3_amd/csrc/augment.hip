// augment.hip -- the real-data input path: letterbox + random affine + flips + photometric augmentation of cached uint8 images, one
// launch per batch, straight into the engines' input layout (bf16 [N][H][W][8], channels 3..7 zero: an NHWC8Batch).
//
// DEFINITION (include/ryolo.h: ryolo_letterbox_augment; restated in float64 by tests/augment_reference.py).  Everything is fp32 on a
// 0..255 scale, per output pixel, never quantised between stages; the unit is built with -ffp-contract=off and IEEE divide, so the
// operations below are the operations executed.  A parameter row is
//     m00 m01 m02 m10 m11 m12  noise_sigma  gamma  gamma_max  blur_sigma  sat_gain  val_gain  gray_alpha  0 0 0
//
//   1. sample   sx = (m00*x + m01*y) + m02, sy = (m10*x + m11*y) + m12 of the output pixel index (x, y); x0 = floor(sx), fx = sx - x0
//               (y alike); tap(ix, iy) = the source byte when 0 <= ix < w and 0 <= iy < h, else 128;
//               v = (1-fy)*((1-fx)*t00 + fx*t01) + fy*((1-fx)*t10 + fx*t11).  A coordinate that is not inside (-1, w) x (-1, h) -- NaN
//               included -- gives 128 (all four taps are outside).
//   2. noise    v += noise_sigma * z on all three channels, then clamp to [0, 255];  z = sqrtf(-2 logf(u1)) * cosf(2 pi u2),
//               u1 = ((r1 >> 8) + 1) * 2^-24 in (0, 1], u2 = (r2 >> 8) * 2^-24 in [0, 1), 2 pi = 6.2831853071795865f, and with
//                   mix(h):  h ^= h >> 16;  h *= 0x7feb352d;  h ^= h >> 15;  h *= 0x846ca68b;  h ^= h >> 16      (uint32, wrapping)
//                   k  = mix(mix(mix(mix(mix((uint32)seed + 0x9e3779b9) ^ (uint32)(seed >> 32)) ^ n) ^ y) ^ x)
//                   r1 = mix(k + 0x9e3779b9),  r2 = mix(k + 0x3c6ef372)
//               (n: the image's slot in the batch; x, y: the output pixel the value belongs to).
//   3. gamma    v = powf(v / gamma_max, gamma) * gamma_max         (skipped when gamma == 1 or gamma_max <= 0)
//   4. blur     separable Gaussian over the OUTPUT grid, taps |d| <= 4, g[0] = 1, g[d] = expf(-(d*d) / (2 sigma^2)), w[d] = g[d] / sum(g), rows then
//               columns, each sum taken from d = -4 up to d = +4; sigma above 1.5 is taken as 1.5; BORDER_REFLECT_101 at the output's
//               edges: a halo pixel is the stage 1-3 value of the reflected output pixel (its noise is that pixel's).
//   5. sat/val  M = max, m = min of the pixel; V' = min(val_gain * M, 255); M <= 0: c' = 0; M == m: c' = V';
//               else S' = min(sat_gain * (M - m) / M, 1), c' = V' * (1 - S' * (M - c) / (M - m)).
//   6. gray     L = (0.299 R + 0.587 G) + 0.114 B;  c = (1 - alpha) * c + alpha * L.
//   7. output   clamp to [0, 255];  c / 255.0f (a division);  round to nearest even bf16;  channels 3..7 zero; one 16-byte store.
//
// A stage whose parameter is neutral (noise_sigma 0, gamma 1, blur_sigma 0, both gains 1, alpha 0) is skipped, so its absence is exact.
//
// SHAPE.  256-thread workgroups own a 32 x 32 output tile of one image (grid: tiles x, tiles y, N); the row's parameters are uniform
// over the workgroup and every stage test is a uniform branch.  Without blur a thread computes its four pixels in registers: no LDS,
// no barrier.  With blur the stage 1-3 values of the 40 x 40 haloed tile go to LDS (3 x 40 x 40 fp32, 18.75 KiB), the horizontal pass
// writes 3 x 40 x 32 fp32 (15 KiB) and the vertical pass reads from there.  Tiles at the right / bottom edge are partial: pixels past
// the edge are computed from reflected coordinates (always inside the image) and not stored.  No workspace, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ryolo.h"

namespace {

constexpr int TILE = 32, RAD = 4, HALO = TILE + 2 * RAD, NPARAM = 16;
constexpr float MAX_BLUR_SIGMA = 1.5f;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct Px { float r, g, b; };

struct Row {             // one parameter row + the source image, uniform over the workgroup
    float m00, m01, m02, m10, m11, m12, noise, gamma, gamma_max, blur, sat, val, alpha;
    const uint8_t *src;
    int h, w;
    uint32_t key;        // the hash of (seed, n)
};

__device__ __forceinline__ uint32_t mix(uint32_t h) {
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    return h;
}

__device__ __forceinline__ float tap(const Row &p, int ix, int iy, int c) {
    return (ix >= 0 && ix < p.w && iy >= 0 && iy < p.h) ? (float)p.src[((size_t)iy * p.w + ix) * 3 + c] : 128.f;
}

// stages 1-3 of output pixel (x, y)
__device__ __forceinline__ Px stage123(const Row &p, int x, int y) {
    const float fxo = (float)x, fyo = (float)y;
    const float sx = (p.m00 * fxo + p.m01 * fyo) + p.m02, sy = (p.m10 * fxo + p.m11 * fyo) + p.m12;
    Px v{128.f, 128.f, 128.f};
    if (sx > -1.f && sx < (float)p.w && sy > -1.f && sy < (float)p.h) {
        const float x0f = floorf(sx), y0f = floorf(sy);
        const float fx = sx - x0f, fy = sy - y0f;
        const int x0 = (int)x0f, y0 = (int)y0f;
        float out[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float t00 = tap(p, x0, y0, c), t01 = tap(p, x0 + 1, y0, c), t10 = tap(p, x0, y0 + 1, c), t11 = tap(p, x0 + 1, y0 + 1, c);
            out[c] = (1.f - fy) * ((1.f - fx) * t00 + fx * t01) + fy * ((1.f - fx) * t10 + fx * t11);
        }
        v = Px{out[0], out[1], out[2]};
    }
    if (p.noise != 0.f) {
        const uint32_t k = mix(mix(p.key ^ (uint32_t)y) ^ (uint32_t)x);
        const uint32_t r1 = mix(k + 0x9e3779b9u), r2 = mix(k + 0x3c6ef372u);
        const float u1 = (float)((r1 >> 8) + 1u) * 5.9604644775390625e-08f, u2 = (float)(r2 >> 8) * 5.9604644775390625e-08f;
        const float z = sqrtf(-2.f * logf(u1)) * cosf(6.2831853071795865f * u2);
        const float d = p.noise * z;
        v.r = fminf(fmaxf(v.r + d, 0.f), 255.f);
        v.g = fminf(fmaxf(v.g + d, 0.f), 255.f);
        v.b = fminf(fmaxf(v.b + d, 0.f), 255.f);
    }
    if (p.gamma != 1.f && p.gamma_max > 0.f) {
        v.r = powf(v.r / p.gamma_max, p.gamma) * p.gamma_max;
        v.g = powf(v.g / p.gamma_max, p.gamma) * p.gamma_max;
        v.b = powf(v.b / p.gamma_max, p.gamma) * p.gamma_max;
    }
    return v;
}

__device__ __forceinline__ float satval(float c, float M, float m, float V, float sat) {
    if (M <= 0.f) return 0.f;
    if (M == m) return V;
    const float S = fminf(sat * (M - m) / M, 1.f);
    return V * (1.f - S * (M - c) / (M - m));
}

// stages 5-7 and the store of output pixel (x, y) of image n
__device__ __forceinline__ void finish(const Row &p, Px v, __bf16 *y, size_t pix) {
    if (p.sat != 1.f || p.val != 1.f) {
        const float M = fmaxf(v.r, fmaxf(v.g, v.b)), m = fminf(v.r, fminf(v.g, v.b));
        const float V = fminf(p.val * M, 255.f);
        v = Px{satval(v.r, M, m, V, p.sat), satval(v.g, M, m, V, p.sat), satval(v.b, M, m, V, p.sat)};
    }
    if (p.alpha != 0.f) {
        const float L = (0.299f * v.r + 0.587f * v.g) + 0.114f * v.b, a = p.alpha, na = 1.f - p.alpha;
        v = Px{na * v.r + a * L, na * v.g + a * L, na * v.b + a * L};
    }
    bf16x8 o;
    o[0] = (__bf16)(fminf(fmaxf(v.r, 0.f), 255.f) / 255.0f);
    o[1] = (__bf16)(fminf(fmaxf(v.g, 0.f), 255.f) / 255.0f);
    o[2] = (__bf16)(fminf(fmaxf(v.b, 0.f), 255.f) / 255.0f);
#pragma unroll
    for (int e = 3; e < 8; e++) o[e] = (__bf16)0.f;
    *(bf16x8 *)(y + pix * 8) = o;
}

// BORDER_REFLECT_101 of any integer onto [0, n)
__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    int t = i % period;
    if (t < 0) t += period;
    return t < n ? t : period - t;
}

__global__ __launch_bounds__(256) void letterbox_augment_kernel(const uint8_t *__restrict__ pixels, const long long *__restrict__ img_offset,
                                                                const int *__restrict__ img_hw, int n_cache,
                                                                const int *__restrict__ src_index, const float *__restrict__ params,
                                                                long long seed, int H, int W, __bf16 *__restrict__ y) {
    __shared__ float sa[3][HALO][HALO];     // stage 1-3 values of the haloed tile
    __shared__ float sb[3][HALO][TILE];     // after the horizontal pass
    const int n = blockIdx.z, x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE, tid = threadIdx.x;
    const float *q = params + (size_t)n * NPARAM;
    Row p;
    p.m00 = q[0]; p.m01 = q[1]; p.m02 = q[2]; p.m10 = q[3]; p.m11 = q[4]; p.m12 = q[5];
    p.noise = q[6]; p.gamma = q[7]; p.gamma_max = q[8]; p.blur = fminf(q[9], MAX_BLUR_SIGMA);
    p.sat = q[10]; p.val = q[11]; p.alpha = q[12];
    const int s = src_index[n];
    if (s >= 0 && s < n_cache) {            // an index outside the cache reads nothing: the image is all border
        p.src = pixels + img_offset[s];
        p.h = img_hw[2 * s];
        p.w = img_hw[2 * s + 1];
    } else {
        p.src = pixels;
        p.h = p.w = 0;
    }
    p.key = mix(mix(mix((uint32_t)(unsigned long long)seed + 0x9e3779b9u) ^ (uint32_t)((unsigned long long)seed >> 32)) ^ (uint32_t)n);
    const size_t img_base = (size_t)n * H * W;

    if (!(p.blur > 0.f)) {
        // thread -> column tid % 32, rows tid / 32 + 8 j: a wave stores two full 512-byte row segments
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int gx = x0 + (tid & 31), gy = y0 + (tid >> 5) + 8 * j;
            if (gx < W && gy < H) finish(p, stage123(p, gx, gy), y, img_base + (size_t)gy * W + gx);
        }
        return;
    }

    float wgt[2 * RAD + 1];
    {
        const float inv = 2.f * p.blur * p.blur;
        float sum = 0.f;
#pragma unroll
        for (int d = -RAD; d <= RAD; d++) {
            wgt[d + RAD] = d == 0 ? 1.f : expf(-(float)(d * d) / inv);
            sum += wgt[d + RAD];
        }
#pragma unroll
        for (int d = 0; d <= 2 * RAD; d++) wgt[d] = wgt[d] / sum;
    }
    for (int i = tid; i < HALO * HALO; i += 256) {
        const int ly = i / HALO, lx = i % HALO;
        const Px v = stage123(p, reflect101(x0 + lx - RAD, W), reflect101(y0 + ly - RAD, H));
        sa[0][ly][lx] = v.r; sa[1][ly][lx] = v.g; sa[2][ly][lx] = v.b;
    }
    __syncthreads();
    for (int i = tid; i < HALO * TILE; i += 256) {
        const int ly = i / TILE, lx = i % TILE;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float acc = 0.f;
#pragma unroll
            for (int d = 0; d <= 2 * RAD; d++) acc += wgt[d] * sa[c][ly][lx + d];
            sb[c][ly][lx] = acc;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int lx = tid & 31, ly = (tid >> 5) + 8 * j;
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx < W && gy < H) {
            float out[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                float acc = 0.f;
#pragma unroll
                for (int d = 0; d <= 2 * RAD; d++) acc += wgt[d] * sb[c][ly + d][lx];
                out[c] = acc;
            }
            finish(p, Px{out[0], out[1], out[2]}, y, img_base + (size_t)gy * W + gx);
        }
    }
}

}  // namespace

extern "C" {

int ryolo_aug_nparam(void) { return NPARAM; }

float ryolo_aug_max_blur_sigma(void) { return MAX_BLUR_SIGMA; }

int ryolo_letterbox_augment(const uint8_t *pixels, const long long *img_offset, const int *img_hw, int n_cache, const int *src_index,
                            const float *params, long long seed, int N, int H, int W, void *y, void *stream) {
    if (!pixels || !img_offset || !img_hw || !src_index || !params || !y || N < 1 || H < 1 || W < 1 || n_cache < 1) return RYOLO_EINVAL;
    if (N > 65535 || (H + TILE - 1) / TILE > 65535 || ((uintptr_t)y & 15)) return RYOLO_EINVAL;
    const dim3 grid((W + TILE - 1) / TILE, (H + TILE - 1) / TILE, N);
    hipLaunchKernelGGL(letterbox_augment_kernel, grid, dim3(256), 0, (hipStream_t)stream, pixels, img_offset, img_hw, n_cache, src_index,
                       params, seed, H, W, (__bf16 *)y);
    return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH;
}

}  // extern "C"
