// rotate-yolov3_amd/csrc/se.hip -- squeeze-and-excitation block, inference (include/ryolo.h: ryolo_se_nhwc).
//
// Replaces SELayer.forward (model/models.py:27-31) on an NHWC bf16 tensor:
//   m[n,c] = mean over H,W of x[n,c,:,:]               (AdaptiveAvgPool2d(1))
//   g[n,:] = sigmoid(W2 . relu(W1 . m[n,:]))           (fc: Linear(C, C/16), ReLU, Linear(C/16, C), Sigmoid; no biases)
//   y      = x * g[n,c]
// Three launches, all HBM-bound: x is read twice and y written once (3 x the tensor, the traffic of ryolo_add_nhwc).
//   se_pool   grid (pixel chunks, N).  A lane owns 8 consecutive channels of a pixel (one 16-byte load); the 256 lanes of a workgroup
//             are (C/8 channel groups) x (pixel rows), a lane walks its row's pixels of the chunk four loads at a time.  fp32 sums,
//             combined across the pixel rows through LDS in row order; one fp32 row [n][chunk][C] per workgroup.  No atomics: the
//             chunking depends on (H, W, C) only, so the sums are the same bits from run to run and for any batch size.
//   se_gate   one workgroup (16 waves) per image: partial rows summed in chunk order, times 1/(H*W); hidden unit h is one wave's dot
//             product (lane-strided, then an xor butterfly: every lane holds the same bits), ReLU; channel c is the dot product of a
//             group of lanes over the hidden units (lane-strided, butterfly inside the group), then 1 / (1 + expf(-t)).
//   se_scale  the pool's lane layout; a lane reads its 8 gate values once, then y = bf16(float(x) * g) with 16-byte loads and stores.
// x and y may be channel slices of wider buffers (pixel strides), which is how a route source is written into its concat buffer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ryolo.h"
#include "se_common.h"

namespace {

using namespace ryolo_se;      // csrc/se_common.h: the chunking (SeGeom), the gate's forward, the overlap rule

__global__ void __launch_bounds__(SE_THREADS)
se_pool_kernel(const __bf16 *__restrict__ x, int cs, int HW, int C, int rows, int chunk_pix, float *__restrict__ part) {
    __shared__ float red[SE_THREADS * 8];        // [rows][C], rows * C <= 2048
    const int G = C >> 3;
    const int r = threadIdx.x / G, g = threadIdx.x - r * G;
    const int n = blockIdx.y, chunk = blockIdx.x;
    const int p0 = chunk * chunk_pix, p1 = min(p0 + chunk_pix, HW);
    if (r < rows) {
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; e++) acc[e] = 0.f;
        const __bf16 *base = x + (size_t)n * HW * cs + g * 8;
        int p = p0 + r;
        for (; p + 3 * rows < p1; p += 4 * rows) {
            const bf16x8 v0 = *(const bf16x8 *)(base + (size_t)p * cs);
            const bf16x8 v1 = *(const bf16x8 *)(base + (size_t)(p + rows) * cs);
            const bf16x8 v2 = *(const bf16x8 *)(base + (size_t)(p + 2 * rows) * cs);
            const bf16x8 v3 = *(const bf16x8 *)(base + (size_t)(p + 3 * rows) * cs);
#pragma unroll
            for (int e = 0; e < 8; e++) acc[e] = (((acc[e] + (float)v0[e]) + (float)v1[e]) + (float)v2[e]) + (float)v3[e];
        }
        for (; p < p1; p += rows) {
            const bf16x8 v = *(const bf16x8 *)(base + (size_t)p * cs);
#pragma unroll
            for (int e = 0; e < 8; e++) acc[e] += (float)v[e];
        }
#pragma unroll
        for (int e = 0; e < 8; e++) red[r * C + g * 8 + e] = acc[e];
    }
    __syncthreads();
    float *out = part + ((size_t)n * gridDim.x + chunk) * C;
    for (int c = threadIdx.x; c < C; c += SE_THREADS) {
        float s = 0.f;
        for (int q = 0; q < rows; q++) s += red[q * C + c];
        out[c] = s;
    }
}

__global__ void __launch_bounds__(SE_GATE_THREADS)
se_gate_kernel(const float *__restrict__ part, int chunks, int C, int hidden, float inv_hw, const float *__restrict__ w1,
               const float *__restrict__ w2, float *__restrict__ gate, float *__restrict__ gate_out) {
    __shared__ float m[SE_MAX_C];
    __shared__ float z[SE_MAX_HIDDEN];
    const int n = blockIdx.x;
    se_gate_forward(part + (size_t)n * chunks * C, (size_t)C, chunks, C, hidden, inv_hw, w1, w2, m, z, [&](int c, float gv) {
        gate[(size_t)n * C + c] = gv;
        if (gate_out) gate_out[(size_t)n * C + c] = gv;
    });
}

__global__ void __launch_bounds__(SE_THREADS)
se_scale_kernel(const __bf16 *__restrict__ x, int x_cs, const float *__restrict__ gate, __bf16 *__restrict__ y, int y_cs, int HW,
                int C, int rows, int chunk_pix) {
    const int G = C >> 3;
    const int r = threadIdx.x / G, g = threadIdx.x - r * G;
    if (r >= rows) return;
    const int n = blockIdx.y;
    const int p0 = blockIdx.x * chunk_pix, p1 = min(p0 + chunk_pix, HW);
    float gv[8];
    {
        const float4 a = *(const float4 *)(gate + (size_t)n * C + g * 8), b = *(const float4 *)(gate + (size_t)n * C + g * 8 + 4);
        gv[0] = a.x; gv[1] = a.y; gv[2] = a.z; gv[3] = a.w; gv[4] = b.x; gv[5] = b.y; gv[6] = b.z; gv[7] = b.w;
    }
    const __bf16 *xb = x + (size_t)n * HW * x_cs + g * 8;
    __bf16 *yb = y + (size_t)n * HW * y_cs + g * 8;
    int p = p0 + r;
    for (; p + 3 * rows < p1; p += 4 * rows) {
        bf16x8 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = *(const bf16x8 *)(xb + (size_t)(p + u * rows) * x_cs);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; e++) o[e] = (__bf16)((float)v[u][e] * gv[e]);
            *(bf16x8 *)(yb + (size_t)(p + u * rows) * y_cs) = o;
        }
    }
    for (; p < p1; p += rows) {
        const bf16x8 v = *(const bf16x8 *)(xb + (size_t)p * x_cs);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = (__bf16)((float)v[e] * gv[e]);
        *(bf16x8 *)(yb + (size_t)p * y_cs) = o;
    }
}

inline int ok_launch() { return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH; }

}  // namespace

extern "C" {

size_t ryolo_se_workspace_bytes(int N, int H, int W, int C) {
    SeGeom g;
    if (!se_geom(N, H, W, C, &g)) return 0;
    return ((size_t)N * g.chunks * C + (size_t)N * C) * sizeof(float);      // the partial rows, then the gates
}

int ryolo_se_nhwc(const void *x, int x_cstride, const float *w1, const float *w2, int hidden, void *y, int y_cstride, int N, int H,
                  int W, int C, float *gate_out, void *workspace, size_t workspace_bytes, void *stream) {
    SeGeom g;
    if (!x || !w1 || !w2 || !y || !workspace || !se_geom(N, H, W, C, &g) || hidden < 1 || hidden > SE_MAX_HIDDEN) return RYOLO_EINVAL;
    if (x_cstride < C || y_cstride < C || (x_cstride & 7) || (y_cstride & 7) || (((uintptr_t)x | (uintptr_t)y) & 15) ||
        (((uintptr_t)workspace | (uintptr_t)w1 | (uintptr_t)w2) & 3) || ((uintptr_t)workspace & 15))
        return RYOLO_EINVAL;
    if (workspace_bytes < ryolo_se_workspace_bytes(N, H, W, C)) return RYOLO_EINVAL;
    const int HW = H * W;
    if (se_overlap(x, x_cstride, y, y_cstride, (long long)N * HW, C)) return RYOLO_EINVAL;
    float *part = (float *)workspace;
    float *gate = part + (size_t)N * g.chunks * C;       // N * chunks * C * 4 bytes: a multiple of 16 (C % 8 == 0)
    const dim3 grid(g.chunks, N);
    hipLaunchKernelGGL(se_pool_kernel, grid, dim3(SE_THREADS), 0, (hipStream_t)stream, (const __bf16 *)x, x_cstride, HW, C, g.rows,
                       g.chunk_pix, part);
    hipLaunchKernelGGL(se_gate_kernel, dim3(N), dim3(SE_GATE_THREADS), 0, (hipStream_t)stream, (const float *)part, g.chunks, C, hidden,
                       1.0f / (float)HW, w1, w2, gate, gate_out);
    hipLaunchKernelGGL(se_scale_kernel, grid, dim3(SE_THREADS), 0, (hipStream_t)stream, (const __bf16 *)x, x_cstride,
                       (const float *)gate, (__bf16 *)y, y_cstride, HW, C, g.rows, g.chunk_pix);
    return ok_launch();
}

}  // extern "C"
