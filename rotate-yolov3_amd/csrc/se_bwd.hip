// rotate-yolov3_amd/csrc/se_bwd.hip -- squeeze-and-excitation block, backward (include/ryolo.h: ryolo_se_bwd_nhwc).
//
// The gradients of SELayer.forward (model/models.py:27-31) as csrc/se.hip computes it, given dy as NHWC bf16.  Saved from the forward:
// x and the two weights, nothing else -- the pass that forms s reads x anyway, so it forms the pixel sums of x too and the gate is
// recomputed.  fp32 on the bf16 values throughout:
//   s[n,c]  = sum_hw dy * x                 dt = s * g * (1 - g)
//   dW2[c,h] (+)= sum_n dt[n,c] * z[n,h]    dz[n,h] = sum_c dt[n,c] * W2[c,h]      du = dz where z > 0, else 0 (threshold_backward)
//   dW1[h,c] (+)= sum_n du[n,h] * m[n,c]    dm[n,c] = sum_h du[n,h] * W1[h,c]
//   dx = bf16(float(dy) * g + dm / (H*W) [+ float(dx_old)])                         one rounding
// At most four launches, no atomics, nothing allocated; x is read once, dy twice, dx written once (four tensor passes):
//   se_bwd_reduce  se_pool's grid, lane layout and chunking (csrc/se_common.h), with a second 16-byte load per pixel for dy.  A lane owns
//                  8 channels of a pixel and walks its row's pixels of the chunk four pixels (eight loads) at a time; the sums of x are
//                  formed by se_pool's expression, so they are se_pool's bits.  Both sums are combined across the pixel rows through LDS
//                  in row order; one fp32 row pair [n][chunk][2][C] per workgroup.
//   se_gate_bwd    one workgroup (16 waves) per image.  m, z, g by se_gate_forward -- the forward kernel's code, the same bits.  Then
//                  dt (LDS); dz: lane (j, h) sums dt[c] * W2[c,h] over its channels c = j, j+J, .. (consecutive lanes read consecutive
//                  addresses of W2), the J partial sums of a hidden unit are combined by one wave's xor butterfly; du; dm: lane c sums
//                  du[h] * W1[h,c] over h ascending (coalesced rows of W1).  Writes g and dm / (H*W) for the apply pass and the
//                  per-image rows dt, m, z, du for the weight gradients.
//   se_wgrad       one lane per element of dW1 / dW2, the sum over n in ascending order, then one add of the old value when accumulating.
//   se_bwd_apply   se_scale's layout: a lane reads its 8 gates and 8 dm / (H*W) once, then 16-byte loads of dy (and dx) and stores of dx.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ryolo.h"
#include "se_common.h"

namespace {

using namespace ryolo_se;

__global__ void __launch_bounds__(SE_THREADS)
se_bwd_reduce_kernel(const __bf16 *__restrict__ x, int x_cs, const __bf16 *__restrict__ dy, int dy_cs, int HW, int C, int rows,
                     int chunk_pix, float *__restrict__ part) {
    __shared__ float red[2 * SE_THREADS * 8];    // [2][rows][C], rows * C <= 2048
    const int G = C >> 3;
    const int r = threadIdx.x / G, g = threadIdx.x - r * G;
    const int n = blockIdx.y, chunk = blockIdx.x;
    const int p0 = chunk * chunk_pix, p1 = min(p0 + chunk_pix, HW);
    const int RC = rows * C;
    if (r < rows) {
        float ax[8], as[8];
#pragma unroll
        for (int e = 0; e < 8; e++) ax[e] = as[e] = 0.f;
        const __bf16 *xb = x + (size_t)n * HW * x_cs + g * 8;
        const __bf16 *db = dy + (size_t)n * HW * dy_cs + g * 8;
        int p = p0 + r;
        for (; p + 3 * rows < p1; p += 4 * rows) {
            bf16x8 v[4], d[4];
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = *(const bf16x8 *)(xb + (size_t)(p + u * rows) * x_cs);
#pragma unroll
            for (int u = 0; u < 4; u++) d[u] = *(const bf16x8 *)(db + (size_t)(p + u * rows) * dy_cs);
#pragma unroll
            for (int e = 0; e < 8; e++) {
                ax[e] = (((ax[e] + (float)v[0][e]) + (float)v[1][e]) + (float)v[2][e]) + (float)v[3][e];      // se_pool's expression
#pragma unroll
                for (int u = 0; u < 4; u++) as[e] = fmaf((float)d[u][e], (float)v[u][e], as[e]);
            }
        }
        for (; p < p1; p += rows) {
            const bf16x8 v = *(const bf16x8 *)(xb + (size_t)p * x_cs);
            const bf16x8 d = *(const bf16x8 *)(db + (size_t)p * dy_cs);
#pragma unroll
            for (int e = 0; e < 8; e++) {
                ax[e] += (float)v[e];
                as[e] = fmaf((float)d[e], (float)v[e], as[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < 8; e++) {
            red[r * C + g * 8 + e] = ax[e];
            red[RC + r * C + g * 8 + e] = as[e];
        }
    }
    __syncthreads();
    float *out = part + ((size_t)n * gridDim.x + chunk) * 2 * C;
    for (int c = threadIdx.x; c < 2 * C; c += SE_THREADS) {
        const float *col = c < C ? red + c : red + RC + (c - C);
        float s = 0.f;
        for (int q = 0; q < rows; q++) s += col[q * C];
        out[c] = s;
    }
}

// rows: the per-image vectors the weight-gradient launch reads (all four null when no weight gradient is wanted); dmh null: no data gradient
__global__ void __launch_bounds__(SE_GATE_THREADS)
se_gate_bwd_kernel(const float *__restrict__ part, int chunks, int C, int hidden, float inv_hw, const float *__restrict__ w1,
                   const float *__restrict__ w2, float *__restrict__ gate, float *__restrict__ gate_out, float *__restrict__ dmh,
                   float *__restrict__ dt_rows, float *__restrict__ m_rows, float *__restrict__ z_rows, float *__restrict__ du_rows) {
    __shared__ float m[SE_MAX_C];
    __shared__ float z[SE_MAX_HIDDEN];
    __shared__ float dt[SE_MAX_C];
    __shared__ float du[SE_MAX_HIDDEN];
    __shared__ float pz[SE_GATE_THREADS];        // [J][Hp] partial sums of dz
    const int n = blockIdx.x;
    const float *p = part + (size_t)n * chunks * 2 * C;
    for (int c = threadIdx.x; c < C; c += SE_GATE_THREADS) {       // s = sum_hw dy * x: the second row of each pair, in chunk order
        float s = 0.f;
#pragma unroll 4
        for (int k = 0; k < chunks; k++) s += p[((size_t)2 * k + 1) * C + c];
        dt[c] = s;                                                 // (read after the barriers inside se_gate_forward)
    }
    se_gate_forward(p, (size_t)2 * C, chunks, C, hidden, inv_hw, w1, w2, m, z, [&](int c, float gv) {
        gate[(size_t)n * C + c] = gv;
        if (gate_out) gate_out[(size_t)n * C + c] = gv;
        const float v = dt[c] * gv * (1.f - gv);
        dt[c] = v;
        if (dt_rows) dt_rows[(size_t)n * C + c] = v;
    });
    if (m_rows) {
        for (int c = threadIdx.x; c < C; c += SE_GATE_THREADS) m_rows[(size_t)n * C + c] = m[c];
        for (int h = threadIdx.x; h < hidden; h += SE_GATE_THREADS) z_rows[(size_t)n * hidden + h] = z[h];
    }
    __syncthreads();
    // dz[h] = sum_c dt[c] * W2[c,h].  Hp = the power of two >= hidden, J = min(1024 / Hp, 64) channel classes: lane (j, h) of the first J * Hp
    int Hp = 1;
    while (Hp < hidden) Hp <<= 1;
    const int J = min(SE_GATE_THREADS / Hp, 64);
    {
        const int j = threadIdx.x / Hp, h = threadIdx.x & (Hp - 1);
        if (j < J) {
            float s = 0.f;
            if (h < hidden) {
#pragma unroll 4
                for (int c = j; c < C; c += J) s += dt[c] * w2[(size_t)c * hidden + h];
            }
            pz[j * Hp + h] = s;
        }
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int h = wave; h < hidden; h += SE_GATE_THREADS / 64) {
        float s = lane < J ? pz[lane * Hp + h] : 0.f;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) {
            const float v = z[h] > 0.f ? s : 0.f;
            du[h] = v;
            if (du_rows) du_rows[(size_t)n * hidden + h] = v;
        }
    }
    if (!dmh) return;
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += SE_GATE_THREADS) {
        float s = 0.f;
#pragma unroll 4
        for (int h = 0; h < hidden; h++) s += du[h] * w1[(size_t)h * C + c];
        dmh[(size_t)n * C + c] = s * inv_hw;
    }
}

__global__ void __launch_bounds__(SE_THREADS)
se_wgrad_kernel(const float *__restrict__ dt_rows, const float *__restrict__ m_rows, const float *__restrict__ z_rows,
                const float *__restrict__ du_rows, int N, int C, int hidden, float *__restrict__ dw1, float *__restrict__ dw2,
                int accumulate) {
    const int total = C * hidden;
    int i = blockIdx.x * SE_THREADS + threadIdx.x;
    if (i >= 2 * total) return;
    const float *a, *b;
    float *out;
    int sa, sb;
    if (i < total) {                 // dW1[h][c] = sum_n du[n,h] * m[n,c]
        const int h = i / C, c = i - h * C;
        a = du_rows + h, sa = hidden, b = m_rows + c, sb = C, out = dw1 + i;
    } else {                         // dW2[c][h] = sum_n dt[n,c] * z[n,h]
        i -= total;
        const int c = i / hidden, h = i - c * hidden;
        a = dt_rows + c, sa = C, b = z_rows + h, sb = hidden, out = dw2 + i;
    }
    float s = 0.f;
#pragma unroll 4
    for (int n = 0; n < N; n++) s += a[(size_t)n * sa] * b[(size_t)n * sb];
    *out = accumulate ? *out + s : s;
}

template <bool ACC>
__global__ void __launch_bounds__(SE_THREADS)
se_bwd_apply_kernel(const __bf16 *__restrict__ dy, int dy_cs, const float *__restrict__ gate, const float *__restrict__ dmh,
                    __bf16 *dx, int dx_cs, int HW, int C, int rows, int chunk_pix) {
    const int G = C >> 3;
    const int r = threadIdx.x / G, g = threadIdx.x - r * G;
    if (r >= rows) return;
    const int n = blockIdx.y;
    const int p0 = blockIdx.x * chunk_pix, p1 = min(p0 + chunk_pix, HW);
    float gv[8], mv[8];
    {
        const float4 a = *(const float4 *)(gate + (size_t)n * C + g * 8), b = *(const float4 *)(gate + (size_t)n * C + g * 8 + 4);
        gv[0] = a.x; gv[1] = a.y; gv[2] = a.z; gv[3] = a.w; gv[4] = b.x; gv[5] = b.y; gv[6] = b.z; gv[7] = b.w;
        const float4 c = *(const float4 *)(dmh + (size_t)n * C + g * 8), d = *(const float4 *)(dmh + (size_t)n * C + g * 8 + 4);
        mv[0] = c.x; mv[1] = c.y; mv[2] = c.z; mv[3] = c.w; mv[4] = d.x; mv[5] = d.y; mv[6] = d.z; mv[7] = d.w;
    }
    const __bf16 *yb = dy + (size_t)n * HW * dy_cs + g * 8;
    __bf16 *xb = dx + (size_t)n * HW * dx_cs + g * 8;
    int p = p0 + r;
    for (; p + 3 * rows < p1; p += 4 * rows) {
        bf16x8 v[4], old[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = *(const bf16x8 *)(yb + (size_t)(p + u * rows) * dy_cs);
        if (ACC) {
#pragma unroll
            for (int u = 0; u < 4; u++) old[u] = *(const bf16x8 *)(xb + (size_t)(p + u * rows) * dx_cs);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float t = fmaf((float)v[u][e], gv[e], mv[e]);
                o[e] = (__bf16)(ACC ? t + (float)old[u][e] : t);
            }
            *(bf16x8 *)(xb + (size_t)(p + u * rows) * dx_cs) = o;
        }
    }
    for (; p < p1; p += rows) {
        const bf16x8 v = *(const bf16x8 *)(yb + (size_t)p * dy_cs);
        bf16x8 old, o;
        if (ACC) old = *(const bf16x8 *)(xb + (size_t)p * dx_cs);
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const float t = fmaf((float)v[e], gv[e], mv[e]);
            o[e] = (__bf16)(ACC ? t + (float)old[e] : t);
        }
        *(bf16x8 *)(xb + (size_t)p * dx_cs) = o;
    }
}

// the workspace, in floats: [N][chunks][2][C] partial sums, then g [N][C], dm / (H*W) [N][C] (both read with 16-byte loads: every offset
// so far is a multiple of 8 floats), then the rows dt [N][C], m [N][C], z [N][hidden], du [N][hidden]
struct SeBwdWs {
    size_t part, gate, dmh, dt, m, z, du, total;
};

inline bool se_bwd_ws(int N, int H, int W, int C, int hidden, SeGeom *g, SeBwdWs *w) {
    if (!se_geom(N, H, W, C, g) || hidden < 1 || hidden > SE_MAX_HIDDEN) return false;
    const size_t nc = (size_t)N * C, nh = (size_t)N * hidden;
    w->part = 0;
    w->gate = (size_t)N * g->chunks * 2 * C;
    w->dmh = w->gate + nc;
    w->dt = w->dmh + nc;
    w->m = w->dt + nc;
    w->z = w->m + nc;
    w->du = w->z + nh;
    w->total = w->du + nh;
    return true;
}

inline int ok_launch() { return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH; }

}  // namespace

extern "C" {

size_t ryolo_se_bwd_workspace_bytes(int N, int H, int W, int C, int hidden) {
    SeGeom g;
    SeBwdWs w;
    if (!se_bwd_ws(N, H, W, C, hidden, &g, &w)) return 0;
    return w.total * sizeof(float);
}

int ryolo_se_bwd_nhwc(const void *x, int x_cstride, const void *dy, int dy_cstride, const float *w1, const float *w2, int hidden, void *dx,
                      int dx_cstride, int dx_accumulate, float *dw1, float *dw2, int accumulate_w, int N, int H, int W, int C,
                      float *gate_out, void *workspace, size_t workspace_bytes, void *stream) {
    SeGeom g;
    SeBwdWs w;
    if (!x || !dy || !w1 || !w2 || !workspace || !se_bwd_ws(N, H, W, C, hidden, &g, &w)) return RYOLO_EINVAL;
    if ((dw1 == nullptr) != (dw2 == nullptr) || (!dx && !dw1)) return RYOLO_EINVAL;
    if (x_cstride < C || dy_cstride < C || (x_cstride & 7) || (dy_cstride & 7) || (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)workspace) & 15) ||
        (((uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)dw1 | (uintptr_t)dw2 | (uintptr_t)gate_out) & 3))
        return RYOLO_EINVAL;
    if (workspace_bytes < w.total * sizeof(float)) return RYOLO_EINVAL;
    const int HW = H * W;
    if (dx) {
        if (dx_cstride < C || (dx_cstride & 7) || ((uintptr_t)dx & 15)) return RYOLO_EINVAL;
        if (se_overlap(x, x_cstride, dx, dx_cstride, (long long)N * HW, C) || se_overlap(dy, dy_cstride, dx, dx_cstride, (long long)N * HW, C))
            return RYOLO_EINVAL;
    }
    float *ws = (float *)workspace;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(g.chunks, N);
    const float inv_hw = 1.0f / (float)HW;
    hipLaunchKernelGGL(se_bwd_reduce_kernel, grid, dim3(SE_THREADS), 0, st, (const __bf16 *)x, x_cstride, (const __bf16 *)dy, dy_cstride, HW,
                       C, g.rows, g.chunk_pix, ws + w.part);
    hipLaunchKernelGGL(se_gate_bwd_kernel, dim3(N), dim3(SE_GATE_THREADS), 0, st, (const float *)(ws + w.part), g.chunks, C, hidden, inv_hw,
                       w1, w2, ws + w.gate, gate_out, dx ? ws + w.dmh : (float *)nullptr, dw1 ? ws + w.dt : (float *)nullptr,
                       dw1 ? ws + w.m : (float *)nullptr, dw1 ? ws + w.z : (float *)nullptr, dw1 ? ws + w.du : (float *)nullptr);
    if (dw1) {
        const int total = 2 * C * hidden;
        hipLaunchKernelGGL(se_wgrad_kernel, dim3((total + SE_THREADS - 1) / SE_THREADS), dim3(SE_THREADS), 0, st, (const float *)(ws + w.dt),
                           (const float *)(ws + w.m), (const float *)(ws + w.z), (const float *)(ws + w.du), N, C, hidden, dw1, dw2,
                           accumulate_w ? 1 : 0);
    }
    if (dx) {
        if (dx_accumulate)
            hipLaunchKernelGGL(se_bwd_apply_kernel<true>, grid, dim3(SE_THREADS), 0, st, (const __bf16 *)dy, dy_cstride,
                               (const float *)(ws + w.gate), (const float *)(ws + w.dmh), (__bf16 *)dx, dx_cstride, HW, C, g.rows, g.chunk_pix);
        else
            hipLaunchKernelGGL(se_bwd_apply_kernel<false>, grid, dim3(SE_THREADS), 0, st, (const __bf16 *)dy, dy_cstride,
                               (const float *)(ws + w.gate), (const float *)(ws + w.dmh), (__bf16 *)dx, dx_cstride, HW, C, g.rows, g.chunk_pix);
    }
    return ok_launch();
}

}  // extern "C"
