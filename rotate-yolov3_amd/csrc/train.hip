// rotate-yolov3_amd/csrc/train.hip -- the elementwise and reduction passes of the training step on gfx950: BatchNorm (batch statistics) +
// PReLU forward / backward, nearest-upsample backward, head-gradient layout conversion.
//
// Replaces what the reference gets from autograd + ATen for `loss.backward()` (train.py:278-282) over the nn.BatchNorm2d / nn.PReLU chain
// of model/models.py:49-66.  The convolution's gradients are units of their own: the weight gradient in csrc/wgrad.hip, the data gradient
// (the forward implicit-GEMM kernels on a flipped / transposed filter) in csrc/conv_dgrad.hip.  Bound: HBM.
#include "conv_common.h"

using namespace ryolo_detail;

namespace {

// ------------------------------------------------------------------------------------------------ BatchNorm + PReLU
// statistics finalisation: partial rows [R][2][cpad] -> mean, invstd, folded scale/shift, running stats (momentum m)
__global__ void __launch_bounds__(1024) bn_finalize_kernel(double *__restrict__ part, int R, int cpad, int C, float count, float eps,
                                   float momentum, const float *__restrict__ gamma, const float *__restrict__ beta,
                                   float *__restrict__ mean, float *__restrict__ invstd, float *__restrict__ scale,
                                   float *__restrict__ shift, float *__restrict__ run_mean, float *__restrict__ run_var) {
    // block = 32 channels x 32 row lanes (latency-bound: many short independent chains); coalesced 128-B reads across
    // the channels of one partial row
    __shared__ double red[2][32][33];
    const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cx;
    double s = 0.0, q = 0.0;
    if (c < C) {
        // latency-bound (a few KB per block): all of a thread's rows are requested before the first is consumed
        for (int r0 = ry; r0 < R; r0 += 32 * 8) {
            double a[8], b[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int r = r0 + 32 * u;
                a[u] = r < R ? part[(size_t)r * 2 * cpad + c] : 0.0;
                b[u] = r < R ? part[(size_t)r * 2 * cpad + cpad + c] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int r = r0 + 32 * u;
                s += a[u];
                q += b[u];
                if (r < R) {                                 // leave the scratch zeroed for the next conv that uses it
                    part[(size_t)r * 2 * cpad + c] = 0.0;
                    part[(size_t)r * 2 * cpad + cpad + c] = 0.0;
                }
            }
        }
    }
    red[0][ry][cx] = s;
    red[1][ry][cx] = q;
    __syncthreads();
    if (ry != 0 || c >= C) return;
    for (int k = 1; k < 32; k++) { s += red[0][k][cx]; q += red[1][k][cx]; }
    const double mu = s / count;
    double var = q / count - mu * mu;
    if (var < 0) var = 0;
    const float is = (float)(1.0 / sqrt(var + (double)eps));
    mean[c] = (float)mu;
    invstd[c] = is;
    scale[c] = gamma[c] * is;
    shift[c] = beta[c] - (float)mu * gamma[c] * is;
    if (run_mean) {
        const double unb = count > 1.f ? var * count / (count - 1.0) : var;
        run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * (float)mu;
        run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)unb;
    }
}

// Mish (x * tanh(softplus x), the north star's activation; not in the reference): value and derivative.
//   with e = exp(x), n = (1 + e)^2:  tanh(softplus x) = (n - 1) / (n + 1) =: t;  d/dx = t + x * (1 - t^2) * e / (1 + e)
__device__ __forceinline__ float mish_f(float x) {
    const float e = __expf(fminf(x, 20.f));
    const float n = (1.f + e) * (1.f + e);
    return x * (n - 1.f) / (n + 1.f);
}
__device__ __forceinline__ float mish_grad(float x) {
    const float e = __expf(fminf(x, 20.f));
    const float n = (1.f + e) * (1.f + e);
    const float t = (n - 1.f) / (n + 1.f);
    return t + x * (1.f - t * t) * (e / (1.f + e));
}

// Streaming policy of the elementwise passes.  Tensors that cannot stay in the 256-MiB Infinity Cache anyway (>= 128 MiB each)
// are read and written NON-TEMPORALLY: measured on the bs-64 shapes (tools/bn_tune.py) +6..8 % on the backward passes of the
// 76^2 x 256, 152^2, 304^2 and 608^2 tensors; smaller tensors keep the default policy -- the apply pass re-reads what the reduce
// pass just fetched and the following convs read what these passes wrote (non-temporal there: -4..-13 %).
constexpr long long NT_MIN_BYTES = 128ll << 20;
#ifdef RYOLO_MP_ABLATION
static int g_nt[3] = {-1, -1, -1};      // ablation build: forward / reduce / apply: -1 = by size (the product's rule), 0 never, 1 always
inline bool nt_pass(int kind, long long npix, int C) { return g_nt[kind] < 0 ? npix * C * 2 >= NT_MIN_BYTES : g_nt[kind] != 0; }
#else
inline bool nt_pass(int, long long npix, int C) { return npix * C * 2 >= NT_MIN_BYTES; }
#endif
template <bool NTL>
__device__ __forceinline__ bf16x8 ld8(const __bf16 *p) {
    if constexpr (NTL) return __builtin_nontemporal_load((const bf16x8 *)p);
    else return *(const bf16x8 *)p;
}
template <bool NTL>
__device__ __forceinline__ void st8(__bf16 *p, const bf16x8 &v) {
    if constexpr (NTL) __builtin_nontemporal_store(v, (bf16x8 *)p);
    else *(bf16x8 *)p = v;
}

// y = act(z*scale + shift) (+ residual); ACT: 0 linear, 1 leaky/PReLU(slope), 2 mish.  The activation is a template
// parameter: as a run-time switch the compiler evaluated the Mish exp/divide chain for every element of every PReLU layer
// (if-conversion), which turned these HBM-bound passes ALU-bound (measured: apply pass 95 -> 578 us per layer).
template <int ACT, bool NTL = false>
__global__ void bn_act_fwd_kernel(const __bf16 *__restrict__ z, int z_cs, const float *__restrict__ scale,
                                  const float *__restrict__ shift, const float *__restrict__ slope_p,
                                  const __bf16 *__restrict__ res, int res_cs, __bf16 *__restrict__ y, int y_cs,
                                  long long npix, int C) {
    const int cpr = C / 8;
    const long long total = npix * cpr;
    const float slope = slope_p ? slope_p[0] : 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long pix = i / cpr;
        const int c = (int)(i % cpr) * 8;
        const bf16x8 v = ld8<NTL>(z + pix * z_cs + c);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            float u = (float)v[e] * scale[c + e] + shift[c + e];
            if (ACT == 1) u = u > 0.f ? u : u * slope;
            else if (ACT == 2) u = mish_f(u);
            o[e] = (__bf16)u;
        }
        if (res) {
            const bf16x8 r = ld8<NTL>(res + pix * res_cs + c);
#pragma unroll
            for (int e = 0; e < 8; e++) o[e] = (__bf16)((float)o[e] + (float)r[e]);
        }
        st8<NTL>(y + pix * y_cs + c, o);
    }
}

// backward pass 1: per-channel sums over pixels of g = dy*act'(u), g*xhat, and dy*min(u,0) (PReLU slope gradient).
// grid (channel tiles of 256, pixel slabs); block = CT chunk lanes (16-B = 8 channels each, contiguous -> coalesced rows)
// x (256/CT) pixel lanes; each block reduces its slab and writes part[slab][3][C].
constexpr int BWD_SLAB_MIN = 128;      // (round 5: 256 left the 19^2 / 38^2 tensors with 1.4 workgroups per CU, eight dependent trips each:
                                       //  23 launches of 25 us at 3.4 TB/s; 128: step 48.39 -> 48.18 / 49.25 -> 49.16 ms on two boxes, 64 and 32 lose
                                       //  it again in the finalise, profiles/r05_ab_log.txt)
#ifdef RYOLO_MP_ABLATION
static int g_bwd_slabs = 1024, g_bwd_slab_min = BWD_SLAB_MIN;   // tuning knobs of the ablation build (tools/bn_tune.py)
inline long long bwd_slab(long long npix) {
    long long s = (npix + g_bwd_slabs - 1) / g_bwd_slabs;
    return s < g_bwd_slab_min ? g_bwd_slab_min : s;
}
#else
inline long long bwd_slab(long long npix) {   // ~<=1024 slabs, at least 128 pixels each (the measurement build sweeps both: ryolo_debug_bn_set, tools/bn_tune.py)
    const long long s = (npix + 1023) / 1024;
    return s < BWD_SLAB_MIN ? BWD_SLAB_MIN : s;
}
#endif
template <int ACT, bool NTL = false>
__global__ void __launch_bounds__(256)
bn_act_bwd_reduce_kernel(const __bf16 *__restrict__ z, int z_cs, const __bf16 *__restrict__ dy, int dy_cs,
                         const float *__restrict__ scale, const float *__restrict__ shift,
                         const float *__restrict__ mean, const float *__restrict__ invstd,
                         const float *__restrict__ slope_p, long long npix, int C, int CT, float *__restrict__ part, long long SL) {
    __shared__ float red[256][25];
    const int cl = threadIdx.x % CT, pl = threadIdx.x / CT, npl = 256 / CT;
    const int c = (blockIdx.x * CT + cl) * 8;          // first of this thread's 8 channels (a block covers CT 8-channel chunks)
    const int slab = blockIdx.y;
    const long long p0 = (long long)slab * SL;
    const long long p1 = p0 + SL < npix ? p0 + SL : npix;
    const float slope = slope_p ? slope_p[0] : 0.f;
    float s1[8], s2[8], s3[8];
#pragma unroll
    for (int e = 0; e < 8; e++) s1[e] = s2[e] = s3[e] = 0.f;
    if (c < C) {
        float sc[8], sh[8], mu[8], is[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            sc[e] = scale ? scale[c + e] : 1.f; sh[e] = scale ? shift[c + e] : 0.f;
            mu[e] = scale ? mean[c + e] : 0.f; is[e] = scale ? invstd[c + e] : 0.f;
        }
        // s2 accumulates g * (z - mean); the invstd factor is applied once at the end.  Four pixels per trip: eight
        // independent 16-B loads in flight per thread (the pass is HBM-bound, latency hiding is what it needs).
        auto accum = [&](const bf16x8 &zv, const bf16x8 &gv) {
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float zf = (float)zv[e], d = (float)gv[e];
                float g = d;
                if (scale) {
                    const float u = zf * sc[e] + sh[e];
                    if (ACT == 1 && u <= 0.f) { g = d * slope; s3[e] += d * u; }
                    else if (ACT == 2) g = d * mish_grad(u);
                    s2[e] += g * (zf - mu[e]);
                }
                s1[e] += g;
            }
        };
        long long pix = p0 + pl;
        for (; pix + 3 * npl < p1; pix += 4 * npl) {
            bf16x8 zv[4], gv[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                zv[k] = ld8<NTL>(z + (pix + k * npl) * z_cs + c);
                gv[k] = ld8<NTL>(dy + (pix + k * npl) * dy_cs + c);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) accum(zv[k], gv[k]);
        }
        for (; pix < p1; pix += npl) accum(*(const bf16x8 *)(z + pix * z_cs + c), *(const bf16x8 *)(dy + pix * dy_cs + c));
#pragma unroll
        for (int e = 0; e < 8; e++) s2[e] *= is[e];
    }
#pragma unroll
    for (int e = 0; e < 8; e++) { red[threadIdx.x][e] = s1[e]; red[threadIdx.x][8 + e] = s2[e]; red[threadIdx.x][16 + e] = s3[e]; }
    __syncthreads();
    // thread t < CT*24: (chunk lane, stat*8+e) -> sum over the pixel lanes
    for (int t = threadIdx.x; t < CT * 24; t += 256) {
        const int l = t / 24, k = t % 24;
        float v = 0.f;
        for (int q = 0; q < npl; q++) v += red[q * CT + l][k];
        const int ch = (blockIdx.x * CT + l) * 8 + (k & 7);
        if (ch < C) part[((size_t)slab * 3 + (k >> 3)) * C + ch] = v;
    }
}

// finalise: sums over slabs -> ds1[c], ds2[c]; parameter gradients (accumulated): dgamma += s2, dbeta += s1,
// dslope += sum_c s3 (one scalar); for a no-BN (bias) conv: dbias += s1
__global__ void __launch_bounds__(1024)
bn_act_bwd_finalize_kernel(const float *__restrict__ part, int nslab, int C, float *__restrict__ s1o,
                           float *__restrict__ s2o, float *__restrict__ dgamma, float *__restrict__ dbeta,
                           float *__restrict__ s3o) {
    // block = 32 channels x 32 slab lanes (coalesced 128-B reads across channels)
    __shared__ float red[3][32][33];
    const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cx;
    float a = 0.f, b = 0.f, d = 0.f;
    if (c < C) {
        for (int s0 = ry; s0 < nslab; s0 += 32 * 8) {       // latency-bound: 24 loads in flight per thread
            float va[8], vb[8], vd[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int s = s0 + 32 * u;
                va[u] = s < nslab ? part[((size_t)s * 3 + 0) * C + c] : 0.f;
                vb[u] = s < nslab ? part[((size_t)s * 3 + 1) * C + c] : 0.f;
                vd[u] = s < nslab ? part[((size_t)s * 3 + 2) * C + c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; u++) { a += va[u]; b += vb[u]; d += vd[u]; }
        }
    }
    red[0][ry][cx] = a; red[1][ry][cx] = b; red[2][ry][cx] = d;
    __syncthreads();
    if (ry != 0) return;
    for (int k = 1; k < 32; k++) { a += red[0][k][cx]; b += red[1][k][cx]; d += red[2][k][cx]; }
    if (c < C) {
        s1o[c] = a;
        s2o[c] = b;
        if (dgamma) dgamma[c] += b;
        if (dbeta) dbeta[c] += a;
        // the PReLU slope gradient is ONE scalar over all channels: per-channel sums go out here and the apply kernel adds them
        // up in a fixed order (an atomicAdd per block made the step's last bit depend on the blocks' arrival order)
        if (s3o) s3o[c] = d;
    }
}

// Partial rows written by a data-gradient launch with one row per pixel tile (ryolo_conv2d_dgrad_bnreduce on the one-tile-per-workgroup
// kernels: up to 23 k rows for the 304^2 layers) are first folded to BWD_FOLD rows -- the finalise kernel above walks the rows with
// C / 32 workgroups only.  Group g sums rows g*per .. (g+1)*per - 1 in a fixed order (32 row lanes striding the group, then the lanes in
// order), so the result is reproducible.
constexpr int BWD_FOLD = 64, BWD_FOLD_MIN_ROWS = 2048;
__global__ void __launch_bounds__(1024)
bn_act_bwd_fold_kernel(const float *__restrict__ part, int nrows, int C, int per, float *__restrict__ out) {
    __shared__ float red[3][32][33];
    const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cx, g = blockIdx.y;
    const int r0 = g * per, r1 = min(nrows, r0 + per);
    float a = 0.f, b = 0.f, d = 0.f;
    if (c < C) {
        for (int s0 = r0 + ry; s0 < r1; s0 += 32 * 4) {
            float va[4], vb[4], vd[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int s = s0 + 32 * u;
                va[u] = s < r1 ? part[((size_t)s * 3 + 0) * C + c] : 0.f;
                vb[u] = s < r1 ? part[((size_t)s * 3 + 1) * C + c] : 0.f;
                vd[u] = s < r1 ? part[((size_t)s * 3 + 2) * C + c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) { a += va[u]; b += vb[u]; d += vd[u]; }
        }
    }
    red[0][ry][cx] = a; red[1][ry][cx] = b; red[2][ry][cx] = d;
    __syncthreads();
    if (ry != 0 || c >= C) return;
    for (int k = 1; k < 32; k++) { a += red[0][k][cx]; b += red[1][k][cx]; d += red[2][k][cx]; }
    out[((size_t)g * 3 + 0) * C + c] = a;
    out[((size_t)g * 3 + 1) * C + c] = b;
    out[((size_t)g * 3 + 2) * C + c] = d;
}

// The head convs' bias gradient from rows the loss's dense pass wrote (csrc/loss.hip: row slab * npl + l = the per-channel sums of the
// stored head gradient over the pixels of pixel lane l of slab `slab` -- the streams of bn_act_bwd_reduce_kernel's bias form, added in
// its order).  Two steps that add what is left in the order of that kernel's block reduce and of bn_act_bwd_finalize_kernel, so dbias
// receives the bits the separate pass over the head gradient would have given it:
//   lanes    out[slab][c] = ((0 + row[slab*npl + 0][c]) + row[slab*npl + 1][c]) + ...           (the reduce kernel's sum over pixel lanes)
//   finalize slab lane ry adds slabs ry, ry + 32, ... ascending, then the 32 lanes in order; dbias[c] += g[0] * that
__global__ void __launch_bounds__(256)
head_bias_lanes_kernel(const float *__restrict__ rows, int npl, int cs, int C, float *__restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x, slab = blockIdx.y;
    if (c >= C) return;
    float v = 0.f;
    for (int q = 0; q < npl; q++) v += rows[((size_t)slab * npl + q) * cs + c];
    out[(size_t)slab * C + c] = v;
}

__global__ void __launch_bounds__(1024)
head_bias_finalize_kernel(const float *__restrict__ part, int nslab, int C, const float *__restrict__ gsc, float *__restrict__ dbias) {
    __shared__ float red[32][33];
    const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cx;
    float a = 0.f;
    if (c < C) {
        for (int s0 = ry; s0 < nslab; s0 += 32 * 8) {
            float va[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int s = s0 + 32 * u;
                va[u] = s < nslab ? part[(size_t)s * C + c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; u++) a += va[u];
        }
    }
    red[ry][cx] = a;
    __syncthreads();
    if (ry != 0 || c >= C) return;
    for (int k = 1; k < 32; k++) a += red[k][cx];
    dbias[c] += gsc[0] * a;
}

// backward pass 2: dz = scale_c * (g - s1/M - xhat * s2/M), g = dy * act'(u).  4096 blocks whose grid stride is a multiple of
// the 8-channel chunks per pixel whenever that count is a power of two: a thread then keeps ONE chunk for its whole walk, its
// per-channel constants live in registers (with k = scale*invstd*s2/M the result is scale*g - k*z + (k*mean - scale*s1/M)),
// and four pixels (8 independent 16-B loads) are in flight per trip.  One chunk per thread with the six constant arrays
// re-read through L1 for every chunk (192 B of constant loads per 48 B of tensor traffic) held this pass at 4.3 TB/s; now
// 4.8-5.4 (measured A/B on one box, tools/bn_bench.py).  The forward pass keeps the one-chunk-per-thread grid: with two
// constant arrays it runs at 5.7 TB/s and every fixed-chunk variant tried was slower (4.6-5.3).  Other channel counts (the
// 504-channel heads) take the generic loop.
template <int ACT, bool NTL = false>
__global__ void __launch_bounds__(256) bn_act_bwd_apply_kernel(const __bf16 *__restrict__ z, int z_cs, const __bf16 *__restrict__ dy, int dy_cs,
                                        const float *__restrict__ scale, const float *__restrict__ shift,
                                        const float *__restrict__ mean, const float *__restrict__ invstd,
                                        const float *__restrict__ s1, const float *__restrict__ s2, float inv_count,
                                        const float *__restrict__ slope_p, __bf16 *__restrict__ dz, int dz_cs,
                                        long long npix, int C, const float *__restrict__ s3, float *__restrict__ dslope) {
    if (dslope && blockIdx.x == 0 && threadIdx.x < 64) {      // dslope += sum_c s3[c], fixed order (lane-strided, then butterfly)
        float v = 0.f;
        for (int c = threadIdx.x; c < C; c += 64) v += s3[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (threadIdx.x == 0) dslope[0] += v;
    }
    const int cpr = C / 8;
    const long long total = npix * cpr;
    const float slope = slope_p ? slope_p[0] : 0.f;
    const long long stride = (long long)gridDim.x * blockDim.x;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (stride % cpr == 0) {
        if (i >= total) return;
        const int c = (int)(i % cpr) * 8;
        const long long dp = stride / cpr;
        float sc[8], sh[8], kb[8], kd[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            sc[e] = scale[c + e];
            sh[e] = shift[c + e];
            const float k = sc[e] * invstd[c + e] * s2[c + e] * inv_count;
            kb[e] = -k;
            kd[e] = k * mean[c + e] - sc[e] * s1[c + e] * inv_count;
        }
        auto one = [&](const bf16x8 &zv, const bf16x8 &gv) {
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float zf = (float)zv[e];
                float g = (float)gv[e];
                const float u = zf * sc[e] + sh[e];
                if (ACT == 1 && u <= 0.f) g *= slope;
                else if (ACT == 2) g *= mish_grad(u);
                o[e] = (__bf16)(sc[e] * g + (kb[e] * zf + kd[e]));
            }
            return o;
        };
        long long pix = i / cpr;
        for (; pix + 3 * dp < npix; pix += 4 * dp) {
            bf16x8 zv[4], gv[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                zv[k] = ld8<NTL>(z + (pix + k * dp) * z_cs + c);
                gv[k] = ld8<NTL>(dy + (pix + k * dp) * dy_cs + c);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) st8<NTL>(dz + (pix + k * dp) * dz_cs + c, one(zv[k], gv[k]));
        }
        for (; pix < npix; pix += dp)
            *(bf16x8 *)(dz + pix * dz_cs + c) = one(*(const bf16x8 *)(z + pix * z_cs + c), *(const bf16x8 *)(dy + pix * dy_cs + c));
        return;
    }
    for (; i < total; i += stride) {
        const long long pix = i / cpr;
        const int c = (int)(i % cpr) * 8;
        const bf16x8 zv = *(const bf16x8 *)(z + pix * z_cs + c);
        const bf16x8 gv = *(const bf16x8 *)(dy + pix * dy_cs + c);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const float zf = (float)zv[e];
            float g = (float)gv[e];
            const float u = zf * scale[c + e] + shift[c + e];
            if (ACT == 1 && u <= 0.f) g *= slope;
            else if (ACT == 2) g *= mish_grad(u);
            const float xh = (zf - mean[c + e]) * invstd[c + e];
            o[e] = (__bf16)(scale[c + e] * (g - s1[c + e] * inv_count - xh * s2[c + e] * inv_count));
        }
        *(bf16x8 *)(dz + pix * dz_cs + c) = o;
    }
}

// dx[n,h,w,c] (+)= sum of the 2x2 block of dy (gradient of nearest x2 upsampling)
__global__ void upsample2x_bwd_kernel(const __bf16 *__restrict__ dy, int dy_cs, __bf16 *__restrict__ dx, int dx_cs, int N,
                                      int H, int W, int C, int accumulate) {
    const int cpr = C / 8;
    const long long total = (long long)N * H * W * cpr;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % cpr) * 8;
        const long long pix = i / cpr;
        const int w = (int)(pix % W);
        const long long t = pix / W;
        const int h = (int)(t % H);
        const long long n = t / H;
        float s[8];
#pragma unroll
        for (int e = 0; e < 8; e++) s[e] = 0.f;
        for (int a = 0; a < 2; a++)
            for (int b = 0; b < 2; b++) {
                const bf16x8 v = *(const bf16x8 *)(dy + ((n * 2 * H + 2 * h + a) * 2 * W + 2 * w + b) * dy_cs + c);
#pragma unroll
                for (int e = 0; e < 8; e++) s[e] += (float)v[e];
            }
        bf16x8 o;
        if (accumulate) {
            const bf16x8 old = *(const bf16x8 *)(dx + pix * dx_cs + c);
#pragma unroll
            for (int e = 0; e < 8; e++) s[e] += (float)old[e];
        }
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = (__bf16)s[e];
        *(bf16x8 *)(dx + pix * dx_cs + c) = o;
    }
}

// p-gradient fp32 [bs, na, ny, nx, no] -> NHWC bf16 [bs, ny, nx, na*no] (channel = a*no + k)
__global__ void pgrad_to_nhwc_kernel(const float *__restrict__ g, int bs, int na, int ny, int nx, int no,
                                     __bf16 *__restrict__ out, int out_cs) {
    const long long total = (long long)bs * na * ny * nx * no;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(i % no);
        long long t = i / no;
        const int x = (int)(t % nx); t /= nx;
        const int y = (int)(t % ny); t /= ny;
        const int a = (int)(t % na);
        const long long n = t / na;
        out[((n * ny + y) * nx + x) * out_cs + a * no + k] = (__bf16)g[i];
    }
}

// tiled variant: a workgroup owns 32 consecutive pixels; per anchor their `no` values are one contiguous run in g
// (coalesced reads), staged in LDS as [pixel][a*no + k] and written as coalesced 16-B rows of the NHWC gradient.
constexpr int PG_PIX = 32;
__global__ void __launch_bounds__(256) pgrad_to_nhwc_tiled_kernel(const float *__restrict__ g, int na, int plane, int no,
                                                                  __bf16 *__restrict__ out, int out_cs, int npix) {
    extern __shared__ __attribute__((aligned(16))) __bf16 pg_lds[];     // [PG_PIX][na*no]
    const int C = na * no;
    const int p0 = blockIdx.x * PG_PIX;
    const int per_a = PG_PIX * no;
    for (int idx = threadIdx.x; idx < na * per_a; idx += 256) {
        const int a = idx / per_a, rem = idx - a * per_a;
        const int pl = rem / no, k = rem - pl * no;
        const int gp = p0 + pl;
        if (gp < npix) {
            const int n = gp / plane, pp = gp - n * plane;
            pg_lds[pl * C + a * no + k] = (__bf16)g[((size_t)(n * na + a) * plane + pp) * no + k];
        }
    }
    __syncthreads();
    const int cpr = C / 8;
    for (int idx = threadIdx.x; idx < PG_PIX * cpr; idx += 256) {
        const int pl = idx / cpr, c = (idx - pl * cpr) * 8;
        if (p0 + pl < npix) *(bf16x8 *)(out + (size_t)(p0 + pl) * out_cs + c) = *(const bf16x8 *)(pg_lds + pl * C + c);
    }
}

constexpr int ELEM_BLOCKS = 4096;   // blocks of the fixed-chunk elementwise passes (16 per CU: every thread walks >= a few pixels)
inline int ok_launch() { return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH; }

}  // namespace

extern "C" {

int ryolo_bn_finalize(double *stat_part, int rows, int cpad, int C, long long count, float eps, float momentum,
                      const float *gamma, const float *beta, float *mean, float *invstd, float *scale, float *shift,
                      float *running_mean, float *running_var, void *stream) {
    if (!stat_part || !gamma || !beta || !mean || !invstd || !scale || !shift || rows <= 0 || C <= 0 || count <= 0)
        return RYOLO_EINVAL;
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 31) / 32), dim3(1024), 0, (hipStream_t)stream, stat_part, rows, cpad, C,
                       (float)count, eps, momentum, gamma, beta, mean, invstd, scale, shift, running_mean, running_var);
    return ok_launch();
}

int ryolo_bn_act_fwd(const void *z, int z_cstride, const float *scale, const float *shift, int act, const float *slope,
                     const void *residual, int res_cstride, void *y, int y_cstride, long long npix, int C, void *stream) {
    if (!z || !scale || !shift || !y || npix <= 0 || C <= 0 || (C & 7) || (z_cstride & 7) || (y_cstride & 7))
        return RYOLO_EINVAL;
    if (residual && (res_cstride & 7)) return RYOLO_EINVAL;    // read with the same 16-byte loads as z
    if (act < 0 || act > 2) return RYOLO_EINVAL;
    const bool ntl = nt_pass(0, npix, C);
#define RYOLO_BN_FWD(A)                                                                                                   \
    hipLaunchKernelGGL((ntl ? bn_act_fwd_kernel<A, true> : bn_act_fwd_kernel<A, false>), dim3(grid_for(npix * (C / 8))), dim3(256), 0, (hipStream_t)stream,           \
                       (const __bf16 *)z, z_cstride, scale, shift, slope, (const __bf16 *)residual, res_cstride,          \
                       (__bf16 *)y, y_cstride, npix, C)
    if (act == 0) RYOLO_BN_FWD(0); else if (act == 1) RYOLO_BN_FWD(1); else RYOLO_BN_FWD(2);
#undef RYOLO_BN_FWD
    return ok_launch();
}

size_t ryolo_bn_act_bwd_workspace_bytes(long long npix, int C) {
    const long long nslab = (npix + bwd_slab(npix) - 1) / bwd_slab(npix);
    return (size_t)nslab * 3 * C * 4 + (size_t)3 * C * 4;
}

/* Backward of y = act(BN_batchstats(z)) w.r.t. z and the parameters.  scale == NULL: the block has no BatchNorm
 * (bias conv, linear): dz = dy is NOT written (the caller uses dy directly) and only dbeta (= dbias) is accumulated. */
static int bn_act_bwd_impl(const void *z, int z_cstride, const void *dy, int dy_cstride, const float *scale, const float *shift,
                           const float *mean, const float *invstd, int act, const float *slope, void *dz, int dz_cstride,
                           long long npix, int C, float *dgamma, float *dbeta, float *dslope, void *workspace,
                           size_t workspace_bytes, const float *pre_part, int pre_rows, void *stream_);

int ryolo_bn_act_bwd(const void *z, int z_cstride, const void *dy, int dy_cstride, const float *scale, const float *shift,
                     const float *mean, const float *invstd, int act, const float *slope, void *dz, int dz_cstride,
                     long long npix, int C, float *dgamma, float *dbeta, float *dslope, void *workspace,
                     size_t workspace_bytes, void *stream_) {
    return bn_act_bwd_impl(z, z_cstride, dy, dy_cstride, scale, shift, mean, invstd, act, slope, dz, dz_cstride, npix, C, dgamma, dbeta,
                           dslope, workspace, workspace_bytes, nullptr, 0, stream_);
}

/* The same backward when the first pass has already run inside the launch that produced dy (ryolo_conv2d_dgrad_bnreduce):
 * `part` = [rows][3][C] partial sums in the layout of the stand-alone pass; finalise + apply only.  workspace: 3*C floats. */
int ryolo_bn_act_bwd_reduced(const void *z, int z_cstride, const void *dy, int dy_cstride, const float *scale, const float *shift,
                             const float *mean, const float *invstd, int act, const float *slope, void *dz, int dz_cstride,
                             long long npix, int C, float *dgamma, float *dbeta, float *dslope, const float *part, int rows,
                             void *workspace, size_t workspace_bytes, void *stream_) {
    if (!part || rows <= 0 || !scale || act != 1) return RYOLO_EINVAL;
    return bn_act_bwd_impl(z, z_cstride, dy, dy_cstride, scale, shift, mean, invstd, act, slope, dz, dz_cstride, npix, C, dgamma, dbeta,
                           dslope, workspace, workspace_bytes, part, rows, stream_);
}

static int bn_act_bwd_impl(const void *z, int z_cstride, const void *dy, int dy_cstride, const float *scale, const float *shift,
                           const float *mean, const float *invstd, int act, const float *slope, void *dz, int dz_cstride,
                           long long npix, int C, float *dgamma, float *dbeta, float *dslope, void *workspace,
                           size_t workspace_bytes, const float *pre_part, int pre_rows, void *stream_) {
    if (!z || !dy || npix <= 0 || C <= 0 || (C & 7) || (z_cstride & 7) || (dy_cstride & 7) || !workspace) return RYOLO_EINVAL;
    if (workspace_bytes < (pre_part ? (size_t)3 * C * 4 : ryolo_bn_act_bwd_workspace_bytes(npix, C))) return RYOLO_EINVAL;
    if (scale && (!shift || !mean || !invstd || !dz || (dz_cstride & 7))) return RYOLO_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    int nslab = pre_part ? pre_rows : (int)((npix + bwd_slab(npix) - 1) / bwd_slab(npix));
    float *part = pre_part ? const_cast<float *>(pre_part) : (float *)workspace;
    float *s1 = pre_part ? (float *)workspace : part + (size_t)nslab * 3 * C, *s2 = s1 + C, *s3 = s2 + C;
    if (pre_part && pre_rows >= BWD_FOLD_MIN_ROWS && workspace_bytes >= (size_t)(3 + 3 * BWD_FOLD) * C * 4) {
        float *folded = s3 + C;
        const int per = (pre_rows + BWD_FOLD - 1) / BWD_FOLD;
        hipLaunchKernelGGL(bn_act_bwd_fold_kernel, dim3((C + 31) / 32, BWD_FOLD), dim3(1024), 0, stream, part, pre_rows, C, per, folded);
        part = folded;
        nslab = (pre_rows + per - 1) / per;
    }
    float *dsl = (scale && act == 1) ? dslope : nullptr;
    int CT = 32;
    while (CT > 1 && CT > C / 8) CT >>= 1;
    // CT = the largest power of two <= min(32, C/8): chunk counts that are not a power of two (C = 56: 7 chunks, CT = 4) need
    // ceil(chunks / CT) blocks -- striding the blocks by 32 chunks regardless left channels >= 8*CT unreduced (found by
    // tests/test_train_engine_gpu.py::test_composed_backward_is_sharp...)
    if (act < 0 || act > 2) return RYOLO_EINVAL;
    const bool nt_red = nt_pass(1, npix, C), nt_app = nt_pass(2, npix, C);
#define RYOLO_BN_REDK(A) (nt_red ? bn_act_bwd_reduce_kernel<A, true> : bn_act_bwd_reduce_kernel<A, false>)
#define RYOLO_BN_RED(A)                                                                                                   \
    hipLaunchKernelGGL(RYOLO_BN_REDK(A), dim3((C / 8 + CT - 1) / CT, nslab), dim3(256), 0, stream,             \
                       (const __bf16 *)z, z_cstride, (const __bf16 *)dy, dy_cstride, scale, shift, mean, invstd, slope,   \
                       npix, C, CT, part, bwd_slab(npix))
    if (pre_part) { /* the producer of dy already wrote the partial rows */ }
    else if (act == 0) RYOLO_BN_RED(0); else if (act == 1) RYOLO_BN_RED(1); else RYOLO_BN_RED(2);
#undef RYOLO_BN_RED
    hipLaunchKernelGGL(bn_act_bwd_finalize_kernel, dim3((C + 31) / 32), dim3(1024), 0, stream, part, nslab, C, s1, s2,
                       scale ? dgamma : nullptr, dbeta, dsl ? s3 : nullptr);
#define RYOLO_BN_APP(A)                                                                                                   \
    hipLaunchKernelGGL((nt_app ? bn_act_bwd_apply_kernel<A, true> : bn_act_bwd_apply_kernel<A, false>), dim3(grid_for(npix * (C / 8), 256, ELEM_BLOCKS)), dim3(256), 0, stream,                  \
                       (const __bf16 *)z, z_cstride, (const __bf16 *)dy, dy_cstride, scale, shift, mean, invstd, s1, s2,  \
                       1.0f / (float)npix, slope, (__bf16 *)dz, dz_cstride, npix, C, s3, dsl)
    if (scale) {
        if (act == 0) RYOLO_BN_APP(0); else if (act == 1) RYOLO_BN_APP(1); else RYOLO_BN_APP(2);
    }
#undef RYOLO_BN_APP
    return ok_launch();
}

/* slabs and pixel lanes of the reduce pass's bias form (scale == NULL) for a [npix][C] gradient: pixel lane l of slab s adds pixels
 * s * slab_pixels + l, + pixel_lanes, ... (below the slab's end) one after the other.  Returns the number of slabs (0: bad arguments). */
int ryolo_bn_act_bwd_bias_order(long long npix, int C, long long *slab_pixels, int *pixel_lanes) {
    if (npix <= 0 || C <= 0 || (C & 7) || !slab_pixels || !pixel_lanes) return 0;
    int CT = 32;
    while (CT > 1 && CT > C / 8) CT >>= 1;
    const long long SL = bwd_slab(npix), nslab = (npix + SL - 1) / SL;
    if (nslab > 0x7fffffffll) return 0;
    *slab_pixels = SL;
    *pixel_lanes = 256 / CT;
    return (int)nslab;
}

size_t ryolo_head_bias_workspace_bytes(long long npix, int C) {
    long long SL;
    int npl;
    const int nslab = ryolo_bn_act_bwd_bias_order(npix, C, &SL, &npl);
    return (size_t)nslab * C * 4;
}

int ryolo_head_bias_finalize(const float *bias_part, long long npix, int bias_cstride, int C, const float *g, float *dbias, void *workspace,
                             size_t workspace_bytes, void *stream_) {
    long long SL;
    int npl;
    const int nslab = ryolo_bn_act_bwd_bias_order(npix, C, &SL, &npl);
    if (!bias_part || !g || !dbias || nslab <= 0 || bias_cstride < C || !workspace || workspace_bytes < (size_t)nslab * C * 4 || nslab > 65535)
        return RYOLO_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(head_bias_lanes_kernel, dim3((C + 255) / 256, nslab), dim3(256), 0, stream, bias_part, npl, bias_cstride, C,
                       (float *)workspace);
    hipLaunchKernelGGL(head_bias_finalize_kernel, dim3((C + 31) / 32), dim3(1024), 0, stream, (const float *)workspace, nslab, C, g, dbias);
    return ok_launch();
}

#ifdef RYOLO_MP_ABLATION
void ryolo_debug_bn_set(int slabs, int slab_min, int nt_fwd, int nt_red, int nt_app) {
    g_bwd_slabs = slabs; g_bwd_slab_min = slab_min; g_nt[0] = nt_fwd; g_nt[1] = nt_red; g_nt[2] = nt_app;
}
#endif

int ryolo_upsample2x_bwd(const void *dy, int dy_cstride, void *dx, int dx_cstride, int N, int H, int W, int C,
                         int accumulate, void *stream) {
    if (!dy || !dx || N <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 7) || (dy_cstride & 7) || (dx_cstride & 7))
        return RYOLO_EINVAL;
    hipLaunchKernelGGL(upsample2x_bwd_kernel, dim3(grid_for((long long)N * H * W * (C / 8))), dim3(256), 0,
                       (hipStream_t)stream, (const __bf16 *)dy, dy_cstride, (__bf16 *)dx, dx_cstride, N, H, W, C, accumulate);
    return ok_launch();
}

int ryolo_pgrad_to_nhwc(const float *pgrad, int bs, int na, int ny, int nx, int no, void *out, int out_cstride,
                        void *stream) {
    if (!pgrad || !out || bs <= 0 || na <= 0 || ny <= 0 || nx <= 0 || no <= 0 || out_cstride < na * no) return RYOLO_EINVAL;
    const long long npix = (long long)bs * ny * nx;
    const size_t smem = (size_t)PG_PIX * na * no * 2;
    if ((na * no) % 8 == 0 && (out_cstride & 7) == 0 && (((uintptr_t)out) & 15) == 0 && smem <= 64 * 1024 && npix < 0x7fffffffll) {
        hipLaunchKernelGGL(pgrad_to_nhwc_tiled_kernel, dim3((unsigned)((npix + PG_PIX - 1) / PG_PIX)), dim3(256), smem,
                           (hipStream_t)stream, pgrad, na, ny * nx, no, (__bf16 *)out, out_cstride, (int)npix);
        return ok_launch();
    }
    hipLaunchKernelGGL(pgrad_to_nhwc_kernel, dim3(grid_for((long long)bs * na * ny * nx * no)), dim3(256), 0,
                       (hipStream_t)stream, pgrad, bs, na, ny, nx, no, (__bf16 *)out, out_cstride);
    return ok_launch();
}

}  // extern "C"
