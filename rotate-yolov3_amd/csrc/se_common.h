// rotate-yolov3_amd/csrc/se_common.h -- what the two squeeze-and-excitation units share: the pixel chunking (se.hip: se_pool / se_scale;
// se_bwd.hip: se_bwd_reduce / se_bwd_apply), the forward of the gate (se_gate; recomputed by se_gate_bwd) and the overlap rule of the C ABI.
// One definition of the gate, the same instructions in the same order in both kernels: the backward's gate is the forward's bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ryolo_se {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

constexpr int SE_THREADS = 256;
constexpr int SE_PIX_PER_ROW = 16;   // pixels a lane visits per chunk
constexpr int SE_MAX_C = 2048;       // C/8 <= 256 lanes: at least one pixel row
constexpr int SE_MAX_HIDDEN = 128;
// 16 waves per image: the gate kernels are chains of short dependent steps on one workgroup, so their time is load latency -- every step
// keeps its loads coalesced and independent of the running sum.
constexpr int SE_GATE_THREADS = 1024;

struct SeGeom {
    int rows;        // pixel rows of the workgroup's lane grid: 256 / (C/8)
    int chunk_pix;   // pixels per workgroup
    int chunks;      // workgroups per image
};

// the chunking: a function of (H, W, C) alone.  Darknet-53 at 608^2: 46 / 23 / 12 chunks per image at 76^2 x 256 / 38^2 x 512 /
// 19^2 x 1024, i.e. 1472 / 736 / 384 workgroups at bs 32 for 256 CUs.
inline bool se_geom(int N, int H, int W, int C, SeGeom *g) {
    if (N <= 0 || N > 65535 || H <= 0 || W <= 0 || C < 16 || C > SE_MAX_C || (C & 7)) return false;
    const long long hw = (long long)H * W;
    if (hw > (1ll << 30)) return false;
    g->rows = SE_THREADS / (C / 8);
    g->chunk_pix = g->rows * SE_PIX_PER_ROW;
    g->chunks = (int)((hw + g->chunk_pix - 1) / g->chunk_pix);
    return true;
}

// The gate of image n, by one workgroup of SE_GATE_THREADS lanes.  `part`: the image's partial pixel sums, row k (of `chunks`) at
// part + k * row_stride.  Leaves m[0..C) = the channel means and z[0..hidden) = relu(W1 . m) in LDS (valid for every lane after the call's
// last barrier, which the caller places) and hands each channel's gate to emit(c, g), once, from one lane.
//   m: partial rows summed in chunk order, times 1/(H*W)
//   z: hidden unit h is one wave's dot product over C, lane-strided, then an xor butterfly (every lane ends with the same bits); ReLU
//   g: channel c is the dot product of a group of S lanes (S = the power of two >= hidden, at most 64) that reads its row of W2
//      contiguously, lane-strided over the hidden units, then a butterfly inside the group; 1 / (1 + expf(-t))
template <class Emit>
__device__ __forceinline__ void se_gate_forward(const float *__restrict__ part, size_t row_stride, int chunks, int C, int hidden,
                                                float inv_hw, const float *__restrict__ w1, const float *__restrict__ w2, float *m, float *z,
                                                Emit emit) {
    for (int c = threadIdx.x; c < C; c += SE_GATE_THREADS) {
        float s = 0.f;
#pragma unroll 4
        for (int k = 0; k < chunks; k++) s += part[(size_t)k * row_stride + c];
        m[c] = s * inv_hw;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int h = wave; h < hidden; h += SE_GATE_THREADS / 64) {
        const float *w = w1 + (size_t)h * C;
        float s = 0.f;
#pragma unroll 4
        for (int c = lane; c < C; c += 64) s += w[c] * m[c];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) z[h] = fmaxf(s, 0.f);
    }
    __syncthreads();
    int S = 1;
    while (S < hidden && S < 64) S <<= 1;
    const int sub = lane & (S - 1), per_wave = 64 / S;
    const int per_pass = (SE_GATE_THREADS / 64) * per_wave;
    for (int c0 = 0; c0 < C; c0 += per_pass) {               // uniform trip count: the shuffles below need every lane of the wave
        const int c = c0 + wave * per_wave + lane / S;
        float t = 0.f;
        if (c < C) {
            const float *w = w2 + (size_t)c * hidden;
            for (int h = sub; h < hidden; h += S) t += w[h] * z[h];
        }
        for (int off = S >> 1; off >= 1; off >>= 1) t += __shfl_xor(t, off, 64);
        if (c < C && sub == 0) emit(c, 1.f / (1.f + expf(-t)));
    }
}

// do the elements of slice y (pixel stride y_cs) share a byte with those of slice x?  Two slices of one buffer (equal strides, disjoint
// channel intervals) interleave in memory without overlapping; anything else whose address ranges meet is taken as an overlap.
inline bool se_overlap(const void *x, int x_cs, const void *y, int y_cs, long long npix, int C) {
    const uintptr_t xa = (uintptr_t)x, ya = (uintptr_t)y;
    const uintptr_t xe = xa + (uintptr_t)(((npix - 1) * x_cs + C) * 2), ye = ya + (uintptr_t)(((npix - 1) * y_cs + C) * 2);
    if (xe <= ya || ye <= xa) return false;
    if (x_cs != y_cs) return true;
    const long long row = (long long)x_cs * 2;
    long long d = (long long)(ya % (uintptr_t)row) - (long long)(xa % (uintptr_t)row);   // byte offset of y's slice inside x's pixel frame
    if (d < 0) d += row;
    return !(d >= (long long)C * 2 && d + (long long)C * 2 <= row);
}

}  // namespace ryolo_se
