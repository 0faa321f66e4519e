// rotate-yolov3_amd/csrc/conv_dgrad.hip -- the data gradient of the convolutions: the tap classes of the stride-2 layers, the weight
// packers (classic, x-fused, batched), and the entry points and queries: they build each class's launch through the shape code the
// forward uses (conv_dispatch.hip: conv_shape), plan it with conv_plan() -- the folded BatchNorm-backward reduce included -- and
// execute the plans with conv_launch().
#include <cstring>

#include "conv_common.h"

using namespace ryolo_detail;

extern "C" {

// ------------------------------------------------------------------------------------------------ dgrad
// dx[n, hi, wi, ci] (+)= sum_{kh,kw,co} dz[n, ho, wo, co] * W[co, ci, kh, kw],  ho*s - pad + kh = hi (same for w).
// stride 1: a plain convolution of dz with the spatially flipped, channel-transposed filter.
// stride 2 (3x3, pad 1): four output-parity classes (hi%2, wi%2) = (a, b); class (a, b) only sees the taps with
// kh = a+1 (mod 2), kw = b+1 (mod 2) -> 1, 2, 2 or 4 taps, each a stride-1 gather dz[(hi+1-kh)/2, (wi+1-kw)/2];
// each class is one launch of the same kernel with its own tap list, packed filter and strided output placement.
static int dgrad_classes(int ks, int stride, int pad, int cls, int *dy, int *dx, int *khs, int *kws) {
    // returns ntaps of class `cls` (stride 1: cls must be 0); tap t reads dz pixel (i + dy[t], j + dx[t]) * of the class grid
    if (stride == 1) {
        int n = 0;
        for (int kh = 0; kh < ks; kh++)
            for (int kw = 0; kw < ks; kw++) {   // dz pixel = hi + pad - kh' where kh' runs over the flipped filter
                dy[n] = kh; dx[n] = kw; khs[n] = ks - 1 - kh; kws[n] = ks - 1 - kw;
                n++;
            }
        return n;
    }
    const int a = cls >> 1, b = cls & 1;
    int n = 0;
    for (int kh = ks - 1; kh >= 0; kh--) {
        if (((a + pad - kh) & 1) != 0) continue;
        for (int kw = ks - 1; kw >= 0; kw--) {
            if (((b + pad - kw) & 1) != 0) continue;
            // hi = 2i + a -> ho = (2i + a + pad - kh) / 2 = i + (a + pad - kh) / 2
            dy[n] = (a + pad - kh) / 2; dx[n] = (b + pad - kw) / 2; khs[n] = kh; kws[n] = kw;
            n++;
        }
    }
    return n;
}

// x-fused stride-2 classes (3x3, pad 1, C_in a multiple of 32 and <= 64 -- the stem, where one input pixel is only 64-128 B):
// the two column parities of a row parity `a` become ONE launch whose output "pixel" (i, j) is the pair of input pixels
// (2i+a, 2j), (2i+a, 2j+1) = 2*C_in contiguous channels, so a store writes whole lines and dz is read twice, not four times.
// Taps (kh, dxo in {0,1}) read dz pixel (i + dy, j + dxo); the weight of output half b at a tap is the filter column
// b == 0 ? (dxo == 0 ? 1 : none) : (dxo == 0 ? 2 : 0).
static inline bool dgrad_xfusable(int Cin, int ksize, int stride) {
    return stride == 2 && ksize == 3 && Cin <= 64 && Cin % 32 == 0;
}
static int dgrad_xfused_class(int a, int *dy, int *dx, int *khs, int *kw0, int *kw1) {
    int n = 0;
    for (int kh = 2; kh >= 0; kh--) {
        if (((a + 1 - kh) & 1) != 0) continue;
        for (int dxo = 0; dxo < 2; dxo++) {
            dy[n] = (a + 1 - kh) / 2; dx[n] = dxo; khs[n] = kh;
            kw0[n] = dxo == 0 ? 1 : -1;
            kw1[n] = dxo == 0 ? 2 : 0;
            n++;
        }
    }
    return n;
}
static size_t dgrad_classic_bytes(int Cout, int Cin, int ksize, int stride) {
    const size_t rows = ((size_t)Cin + 127) / 128 * 128;
    size_t total = 0;
    int dy[9], dx[9], khs[9], kws[9];
    for (int cls = 0; cls < (stride == 1 ? 1 : 4); cls++) {
        const int nt = dgrad_classes(ksize, stride, (ksize - 1) / 2, cls, dy, dx, khs, kws);
        const size_t Kpad = ((size_t)nt * Cout + BK - 1) / BK * BK;
        total += (rows * Kpad + 128) * 2;
    }
    return total;
}

size_t ryolo_conv_packed_dgrad_bytes(int Cout, int Cin, int ksize, int stride) {
    if (Cout <= 0 || Cin <= 0 || (ksize != 1 && ksize != 3) || (stride != 1 && stride != 2)) return 0;
    size_t total = dgrad_classic_bytes(Cout, Cin, ksize, stride);
    if (dgrad_xfusable(Cin, ksize, stride)) {       // the x-fused images follow the four classic ones
        const size_t rows = ((size_t)2 * Cin + 127) / 128 * 128;
        int dy[9], dx[9], khs[9], k0[9], k1[9];
        for (int a = 0; a < 2; a++) {
            const int nt = dgrad_xfused_class(a, dy, dx, khs, k0, k1);
            const size_t Kpad = ((size_t)nt * Cout + BK - 1) / BK * BK;
            total += (rows * Kpad + 128) * 2;
        }
    }
    return total;
}

struct XfTaps { int khs[9], kw0[9], kw1[9]; };
__global__ void pack_dgrad_xfused_kernel(const float *__restrict__ w, int Cout, int Cin, int ntaps, XfTaps tp, int Kpad, int rows,
                                         __bf16 *__restrict__ out) {
    // out[b*Cin + ci][t*Cout + co] = w[co][ci][kh_t][kw_{b,t}] (0 where the half has no column at that tap)
    const size_t total = (size_t)rows * Kpad + 128;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        float v = 0.f;
        if (i < (size_t)rows * Kpad) {
            const int rr = (int)(i / Kpad), k = (int)(i % Kpad);
            const int t = k / Cout, co = k % Cout;
            if (rr < 2 * Cin && t < ntaps) {
                const int b = rr / Cin, ci = rr - b * Cin;
                const int kw = b ? tp.kw1[t] : tp.kw0[t];
                if (kw >= 0) v = w[(((size_t)co * Cin + ci) * 3 + tp.khs[t]) * 3 + kw];
            }
        }
        out[i] = (__bf16)v;
    }
}

__global__ void pack_dgrad_kernel(const float *__restrict__ w, int Cout, int Cin, int KS, int ntaps, const int *khs_kws,
                                  int Kpad, int rows, __bf16 *__restrict__ out) {
    // out[ci][t*Cout + co] = w[co][ci][kh_t][kw_t]
    const size_t total = (size_t)rows * Kpad + 128;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        float v = 0.f;
        if (i < (size_t)rows * Kpad) {
            const int ci = (int)(i / Kpad), k = (int)(i % Kpad);
            const int t = k / Cout, co = k % Cout;
            if (ci < Cin && t < ntaps) v = w[(((size_t)co * Cin + ci) * KS + khs_kws[t]) * KS + khs_kws[9 + t]];
        }
        out[i] = (__bf16)v;
    }
}

// ---- all weight packs of a training step in ONE launch (forward layout + every dgrad class of every conv) ----------
// 160 small launches per step otherwise (1.1 ms of launch-bound time at bs 32).  `jobs` is a device array built once by
// the caller with ryolo_conv_pack_job_fill; workgroup b serves the job whose [block_begin, block_end) contains b.
constexpr int PK_ROWS = 4;            // forward layout: output rows (c_out) per workgroup
constexpr int PK_CI = 32, PK_CO = 64;  // dgrad layout: (c_in rows) x (c_out columns) per workgroup
constexpr int PK_PAD = 2;             // dgrad sub-block: bf16 elements added to each c_out's run in LDS.  The transposing read walks c_out
                                      // across the lanes; 288 elements = 144 words per run put 64 lanes on 4 banks (16-way conflict),
                                      // 145 words spread them over all 64
constexpr int PK_UB = 6;              // 16-B loads a thread keeps in flight while it stages a tile (one per trip left the pass latency-bound)
constexpr int PK_LDS = PK_CO * (PK_CI * 9 + PK_PAD);   // bf16 elements: one [64 c_out][32 c_in][9 taps] sub-block, or one forward row
__global__ void __launch_bounds__(256) pack_batch_kernel(const ryolo_pack_job *__restrict__ jobs, int njobs) {
    // Both layouts are transposes of the OIHW parameter, so each workgroup moves a TILE through LDS: it reads the fp32
    // source in its own order (whole [c_in][taps] rows / 32-channel runs of them: coalesced) and writes bf16 runs that are
    // contiguous in the destination.  The element-wise gather this replaces read the 250 MB of weights through 36-byte
    // (forward) and 4.6-KB (dgrad) strides: 0.92 ms per step.
    __shared__ __bf16 sm[PK_LDS];
    int lo = 0;                             // last job with block_begin <= blockIdx.x (block_begin ascending, jobs[0] starts at 0)
    if (njobs <= 256) {                     // one round of parallel loads + a count, not eight dependent loads of a binary search
        lo = __syncthreads_count((int)threadIdx.x < njobs && jobs[threadIdx.x].block_begin <= (int)blockIdx.x) - 1;
    } else {
        int hi = njobs - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (jobs[mid].block_begin <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
        }
    }
    const ryolo_pack_job j = jobs[lo];
    const int blk = (int)blockIdx.x - j.block_begin;
    const float *__restrict__ w = (const float *)j.src;
    __bf16 *__restrict__ out = (__bf16 *)j.dst;
    const int KK = j.KS * j.KS;
    const int tid = threadIdx.x;
    if (blk == 0)                           // the 128-element zero page behind the body
        for (int i = tid; i < 128; i += 256) out[(size_t)j.rows * j.Kpad + i] = (__bf16)0.f;
    if (j.kind == 0) {                      // forward: out[co][tap*Cin_pad + c] = w[co][c][tap]
        const int rowlen = j.Cin * KK;
        const int rl4 = (rowlen + 3) & ~3;                       // a row's slot in LDS (8-B aligned)
        const int fit = PK_LDS / rl4 < PK_ROWS ? (PK_LDS / rl4 < 1 ? 1 : PK_LDS / rl4) : PK_ROWS;   // rows staged together: one load
        for (int rr0 = 0; rr0 < PK_ROWS; rr0 += fit) {           // round and one barrier pair for all of them when they fit
            const int rbase = blk * PK_ROWS + rr0;
            if (rbase >= j.rows) break;
            for (int rr = 0; rr < fit && rr0 + rr < PK_ROWS; rr++) {
                const int r = rbase + rr;
                if (r >= j.Cout) break;                          // (rows past C_out are zero rows: nothing to stage)
                __bf16 *dst = sm + rr * rl4;
                if ((rowlen & 3) == 0 && ((uintptr_t)w & 15) == 0) {    // 16-B loads (a row starts at a multiple of 4 floats then, and the parameter itself at a
                                                                        // 16-B boundary: a view into a flat buffer may not -- those take the scalar path)
                    const float4 *w4 = (const float4 *)(w + (size_t)r * rowlen);
                    for (int i0 = tid; i0 < rowlen / 4; i0 += 256 * PK_UB) {     // PK_UB independent loads in flight per thread
                        float4 v[PK_UB];
#pragma unroll
                        for (int u = 0; u < PK_UB; u++)
                            if (i0 + u * 256 < rowlen / 4) v[u] = w4[i0 + u * 256];
#pragma unroll
                        for (int u = 0; u < PK_UB; u++) {
                            if (i0 + u * 256 >= rowlen / 4) break;
                            bf16x4 o;
                            o[0] = (__bf16)v[u].x; o[1] = (__bf16)v[u].y; o[2] = (__bf16)v[u].z; o[3] = (__bf16)v[u].w;
                            *(bf16x4 *)(dst + 4 * (i0 + u * 256)) = o;
                        }
                    }
                } else {
                    for (int i = tid; i < rowlen; i += 256) dst[i] = (__bf16)w[(size_t)r * rowlen + i];
                }
            }
            __syncthreads();
            for (int rr = 0; rr < fit && rr0 + rr < PK_ROWS; rr++) {
                const int r = rbase + rr;
                if (r >= j.rows) break;
                const bool real = r < j.Cout;
                const __bf16 *src = sm + rr * rl4;
                if ((j.Cin_pad & 7) == 0) {     // 8 consecutive k share a tap: one 16-B store per thread and trip (Kpad % 64 == 0)
                    for (int k8 = tid * 8; k8 < j.Kpad; k8 += 256 * 8) {
                        const int tap = k8 / j.Cin_pad, c0 = k8 - tap * j.Cin_pad;
                        bf16x8 v;
#pragma unroll
                        for (int e = 0; e < 8; e++) v[e] = (real && tap < KK && c0 + e < j.Cin) ? src[(c0 + e) * KK + tap] : (__bf16)0.f;
                        *(bf16x8 *)(out + (size_t)r * j.Kpad + k8) = v;
                    }
                } else {
                    for (int k = tid; k < j.Kpad; k += 256) {
                        const int tap = k / j.Cin_pad, c = k - tap * j.Cin_pad;
                        out[(size_t)r * j.Kpad + k] = (real && tap < KK && c < j.Cin) ? src[c * KK + tap] : (__bf16)0.f;
                    }
                }
            }
            __syncthreads();
        }
        return;
    }
    // dgrad class: out[ci][t*Cout + co] = w[co][ci][kh_t][kw_t]; kind 2 (x-fused stride-2 class): rows are (b, ci), the
    // filter column of tap t is nibble b of kws[t] minus 1 (-1: this half has no column there)
    const int cob = (j.Cout + PK_CO - 1) / PK_CO;
    const int row0 = (blk / cob) * PK_CI, co0 = (blk % cob) * PK_CO;
    const int half = (j.kind == 2 && row0 >= j.Cin) ? 1 : 0;
    const int ci0 = j.kind == 2 ? row0 - half * j.Cin : row0;
    const bool live = j.kind != 2 || row0 < 2 * j.Cin;
    const int run = PK_CI * KK;             // one c_out's share of the sub-block: 32 c_in x taps, contiguous in w
    const int pitch = run + PK_PAD;
    if ((run & 3) == 0 && (j.Cin & 3) == 0 && ci0 + PK_CI <= j.Cin && ((uintptr_t)w & 15) == 0) {
        // whole 32-channel runs: 16-B loads (a run starts at (co * Cin + ci0) * KK floats, a multiple of 4); the LDS pitch is odd in
        // words, so the four bf16 go out as two 4-B stores
        static_assert((PK_CI * 9 + PK_PAD) % 2 == 0, "4-B aligned runs in LDS");
        const int run4 = run / 4;
        for (int i0 = tid; i0 < PK_CO * run4; i0 += 256 * PK_UB) {       // PK_UB independent loads in flight per thread
            float4 v[PK_UB];
#pragma unroll
            for (int u = 0; u < PK_UB; u++) {
                const int i = i0 + u * 256;
                const int col = i / run4, q = i - col * run4;
                v[u] = float4{0.f, 0.f, 0.f, 0.f};
                if (i < PK_CO * run4 && live && co0 + col < j.Cout) v[u] = *(const float4 *)(w + ((size_t)(co0 + col) * j.Cin + ci0) * KK + 4 * q);
            }
#pragma unroll
            for (int u = 0; u < PK_UB; u++) {
                const int i = i0 + u * 256;
                if (i >= PK_CO * run4) break;
                const int col = i / run4, q = i - col * run4;
                bf16x2 lo, hi;
                lo[0] = (__bf16)v[u].x; lo[1] = (__bf16)v[u].y; hi[0] = (__bf16)v[u].z; hi[1] = (__bf16)v[u].w;
                *(bf16x2 *)(sm + col * pitch + 4 * q) = lo;
                *(bf16x2 *)(sm + col * pitch + 4 * q + 2) = hi;
            }
        }
    } else {
        for (int i = tid; i < PK_CO * run; i += 256) {
            const int col = i / run, rem = i - col * run;
            const int co = co0 + col, ci = ci0 + rem / KK;
            sm[col * pitch + rem] = (live && co < j.Cout && ci < j.Cin) ? (__bf16)w[((size_t)co * j.Cin + ci0) * KK + rem] : (__bf16)0.f;
        }
    }
    __syncthreads();
    if ((j.Cout & 7) == 0) {                // 8 consecutive c_out per thread: 16-B stores (every row offset is a multiple of 8 elements)
        for (int i = tid; i < PK_CI * j.ntaps * (PK_CO / 8); i += 256) {
            const int col = (i % (PK_CO / 8)) * 8, t = (i / (PK_CO / 8)) % j.ntaps, cil = i / ((PK_CO / 8) * j.ntaps);
            if (co0 + col < j.Cout) {
                const int kw = j.kind == 2 ? ((j.kws[t] >> (4 * half)) & 15) - 1 : j.kws[t];
                const int src = cil * KK + j.khs[t] * j.KS + kw;
                bf16x8 v;
#pragma unroll
                for (int e = 0; e < 8; e++) v[e] = kw >= 0 ? sm[(col + e) * pitch + src] : (__bf16)0.f;
                *(bf16x8 *)(out + (size_t)(row0 + cil) * j.Kpad + t * j.Cout + co0 + col) = v;
            }
        }
    } else {
        for (int i = tid; i < PK_CI * j.ntaps * PK_CO; i += 256) {
            const int col = i % PK_CO, t = (i / PK_CO) % j.ntaps, cil = i / (PK_CO * j.ntaps);
            if (co0 + col < j.Cout) {
                const int kw = j.kind == 2 ? ((j.kws[t] >> (4 * half)) & 15) - 1 : j.kws[t];
                out[(size_t)(row0 + cil) * j.Kpad + t * j.Cout + co0 + col] =
                    kw >= 0 ? sm[col * pitch + cil * KK + j.khs[t] * j.KS + kw] : (__bf16)0.f;
            }
        }
    }
    if (co0 == 0) {                         // K padding behind the last tap of these 32 rows
        const int kreal = j.ntaps * j.Cout, padn = j.Kpad - kreal;
        for (int i = tid; i < PK_CI * padn; i += 256) out[(size_t)(row0 + i / padn) * j.Kpad + kreal + i % padn] = (__bf16)0.f;
    }
}

int ryolo_conv_pack_job_fill(ryolo_pack_job *host_jobs /* room for 7 */, const float *w_oihw, int Cout, int Cin, int ksize,
                             int stride, int Cin_pad, void *packed_fwd, void *packed_dgrad /* or NULL */) {
    if (!host_jobs || !w_oihw || !packed_fwd || Cout <= 0 || Cin <= 0 || Cin_pad < Cin || (ksize != 1 && ksize != 3) ||
        (stride != 1 && stride != 2))
        return -1;
    int n = 0;
    {
        ryolo_pack_job &j = host_jobs[n++];
        j = ryolo_pack_job{};
        j.src = w_oihw; j.dst = packed_fwd; j.kind = 0; j.Cout = Cout; j.Cin = Cin; j.KS = ksize; j.Cin_pad = Cin_pad;
        j.Kpad = (ksize * ksize * Cin_pad + BK - 1) / BK * BK;
        j.rows = (Cout + 127) / 128 * 128;
        j.block_begin = 0; j.block_end = (j.rows + PK_ROWS - 1) / PK_ROWS;      // workgroups of pack_batch_kernel
        if (Cin * ksize * ksize > PK_LDS) return -1;
    }
    if (packed_dgrad) {
        if (ryolo_conv_packed_dgrad_bytes(Cout, Cin, ksize, stride) == 0) return -1;
        char *dst = (char *)packed_dgrad;
        for (int cls = 0; cls < (stride == 1 ? 1 : 4); cls++) {
            int dy[9], dx[9], khs[9], kws[9];
            const int nt = dgrad_classes(ksize, stride, (ksize - 1) / 2, cls, dy, dx, khs, kws);
            ryolo_pack_job &j = host_jobs[n++];
            j = ryolo_pack_job{};
            j.src = w_oihw; j.dst = dst; j.kind = 1; j.Cout = Cout; j.Cin = Cin; j.KS = ksize; j.ntaps = nt;
            for (int t = 0; t < nt; t++) { j.khs[t] = khs[t]; j.kws[t] = kws[t]; }
            j.Kpad = (nt * Cout + BK - 1) / BK * BK;
            j.rows = (Cin + 127) / 128 * 128;
            j.block_begin = 0; j.block_end = (j.rows / PK_CI) * ((Cout + PK_CO - 1) / PK_CO);
            dst += ((size_t)j.rows * j.Kpad + 128) * 2;
        }
        if (dgrad_xfusable(Cin, ksize, stride)) {
            for (int a = 0; a < 2; a++) {
                int dy[9], dx[9], khs[9], k0[9], k1[9];
                const int nt = dgrad_xfused_class(a, dy, dx, khs, k0, k1);
                ryolo_pack_job &j = host_jobs[n++];
                j = ryolo_pack_job{};
                j.src = w_oihw; j.dst = dst; j.kind = 2; j.Cout = Cout; j.Cin = Cin; j.KS = ksize; j.ntaps = nt;
                for (int t = 0; t < nt; t++) { j.khs[t] = khs[t]; j.kws[t] = (k0[t] + 1) | ((k1[t] + 1) << 4); }
                j.Kpad = (nt * Cout + BK - 1) / BK * BK;
                j.rows = (2 * Cin + 127) / 128 * 128;
                j.block_begin = 0; j.block_end = (j.rows / PK_CI) * ((Cout + PK_CO - 1) / PK_CO);
                dst += ((size_t)j.rows * j.Kpad + 128) * 2;
            }
        }
    }
    return n;
}

int ryolo_conv_pack_batch(const ryolo_pack_job *device_jobs, int njobs, int total_blocks, void *stream) {
    if (!device_jobs || njobs <= 0 || total_blocks <= 0) return RYOLO_EINVAL;
    hipLaunchKernelGGL(pack_batch_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, device_jobs, njobs);
    return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH;
}

int ryolo_conv_dgrad_tap_table(int ksize, int stride, int *host_out /* int[72] */) {
    if (!host_out || (ksize != 1 && ksize != 3) || (stride != 1 && stride != 2)) return RYOLO_EINVAL;
    for (int i = 0; i < 72; i++) host_out[i] = 0;
    for (int cls = 0; cls < (stride == 1 ? 1 : 4); cls++) {
        int dy[9], dx[9];
        dgrad_classes(ksize, stride, (ksize - 1) / 2, cls, dy, dx, host_out + cls * 18, host_out + cls * 18 + 9);
    }
    return RYOLO_OK;
}

int ryolo_conv_pack_weights_dgrad(const float *w_oihw, int Cout, int Cin, int ksize, int stride, void *packed,
                                  const int *taps_table /* device int[72] from ryolo_conv_dgrad_tap_table */, void *stream_) {
    if (!w_oihw || !packed || !taps_table || ryolo_conv_packed_dgrad_bytes(Cout, Cin, ksize, stride) == 0) return RYOLO_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    const int rows = (Cin + 127) / 128 * 128;
    char *dst = (char *)packed;
    for (int cls = 0; cls < (stride == 1 ? 1 : 4); cls++) {
        int dy[9], dx[9], kk[18];
        const int nt = dgrad_classes(ksize, stride, (ksize - 1) / 2, cls, dy, dx, kk, kk + 9);
        const int Kpad = (nt * Cout + BK - 1) / BK * BK;
        const size_t total = (size_t)rows * Kpad + 128;
        const int nb = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
        hipLaunchKernelGGL(pack_dgrad_kernel, dim3(nb), dim3(256), 0, stream, w_oihw, Cout, Cin, ksize, nt,
                           taps_table + cls * 18, Kpad, rows, (__bf16 *)dst);
        dst += total * 2;
    }
    if (dgrad_xfusable(Cin, ksize, stride)) {
        const int rows2 = (2 * Cin + 127) / 128 * 128;
        for (int a = 0; a < 2; a++) {
            int dy[9], dx[9];
            XfTaps tp;
            const int nt = dgrad_xfused_class(a, dy, dx, tp.khs, tp.kw0, tp.kw1);
            for (int t = nt; t < 9; t++) { tp.khs[t] = 0; tp.kw0[t] = -1; tp.kw1[t] = -1; }
            const int Kpad = (nt * Cout + BK - 1) / BK * BK;
            const size_t total = (size_t)rows2 * Kpad + 128;
            const int nb = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
            hipLaunchKernelGGL(pack_dgrad_xfused_kernel, dim3(nb), dim3(256), 0, stream, w_oihw, Cout, Cin, nt, tp, Kpad, rows2,
                               (__bf16 *)dst);
            dst += total * 2;
        }
    }
    return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH;
}

}  // extern "C"

// The launches of one data gradient and their plans: the stem kernel (one launch, conv_stem.hip), or one implicit-GEMM launch per
// output-parity class (stride 1: one; stride 2: two x-fused or four classic; a class without pixels has none)
struct DgradPlan {
    bool stem = false;
    ConvPlan stem_plan;
    int n = 0;
    ConvParams p[4];
    ConvPlan pl[4];
    int nt_out = 0;
    // every launch has a kernel
    bool launchable() const {
        for (int i = 0; i < n; i++)
            if (pl[i].kernel < 0) return false;
        return true;
    }
    // the kernel the queries report: the last non-empty class's (-1: refused, or nothing to launch)
    int kernel() const { return stem ? stem_plan.kernel : (n > 0 && launchable() ? pl[n - 1].kernel : -1); }
};

// Builds the launches of the data gradient of `d` (the FORWARD conv) behind ryolo_conv2d_dgrad[_bnreduce] and the queries; false: the
// descriptor is refused.  Each class is a convolution of dz in the gradient's direction -- C_out -> C_in channels, stride 1 -- whose
// ConvParams come from conv_shape() like the forward's; the class then gets its tap list, filter image, pixel grid and output placement.
// (The queries pass stand-ins for the pointers and a dense dz: the plans depend only on whether `accumulate` is set.)
static bool dgrad_plan(const ryolo_conv_desc *d, const void *dz, int dz_cstride, const void *packed_dgrad, const float *ones, const float *zeros,
                       void *dx, int accumulate, bool want_reduce, DgradPlan &out) {
    if (conv_validate(d) != RYOLO_OK) return false;
    if (d->stride != 1 && !(d->stride == 2 && d->ksize == 3 && d->pad == 1)) return false;
    if ((dz_cstride & 7) || dz_cstride < d->Cout || (want_reduce && d->stride != 1)) return false;
    if ((long long)d->N * d->H * d->W > 0x7fffffffLL - 512) return false;      // dx is indexed by pixel, like every launch's output (conv_pixels)
    const int Ho = (d->H + 2 * d->pad - d->ksize) / d->stride + 1, Wo = (d->W + 2 * d->pad - d->ksize) / d->stride + 1;
    const int rows = (d->Cin + 127) / 128 * 128;
    const unsigned long long dz_pix = (unsigned long long)d->N * Ho * Wo;
    out.nt_out = (long long)d->N * d->H * d->W * d->Cin * 2 >= nt_out_min_bytes() ? 1 : 0;
    const char *wsrc = (const char *)packed_dgrad;
    // x-fused stride-2 classes when the input gradient is dense and its rows hold an even number of pixels (tile bit 0x8000
    // forces the four classic classes: tests / A-B)
    const bool xfuse = dgrad_xfusable(d->Cin, d->ksize, d->stride) && d->pad == 1 && (d->W & 1) == 0 &&
                       d->in_cstride == d->Cin && !(d->tile & 0x8000);
    if (xfuse) wsrc += dgrad_classic_bytes(d->Cout, d->Cin, d->ksize, d->stride);
    // Darknet-53 layers 1 and 3 (3x3, 32 -> 64, stride 2 / 1) and 5 (3x3 / 2, 64 -> 128): one persistent launch with the dz patch staged
    // once and the filter in registers (conv_stem.hip); tile bit 0x8000 (the classic classes), a forced tile and RYOLO_STEM_DGRAD (bit 0:
    // the 64 -> 32 kernels, bit 1: the 128 -> 64 one; A/B, ryolo_set_tuning) keep the implicit-GEMM launches, which also serve what its
    // plan refuses (dz of 2 GiB and more: they did before this kernel existed)
    // (the stride-1 64 -> 128 layers keep the 256 x 64 tile: it carries the folded BatchNorm reduce, and the channel-split kernel measured
    // 286 us against its 278 / 332 with the reduce -- step 48.50 vs 48.44 ms)
    if (!want_reduce && !(d->tile & 0x80ff)) {
        const char *e = tune(TUNE_STEM_DGRAD);
        const int knob = e ? atoi(e) : 3;
        if ((knob & (d->Cout == 64 ? 1 : 2)) && conv_stem_dgrad_plan(d, dz_cstride, out.stem_plan)) {
            out.stem = true;
            return true;
        }
    }
    ryolo_conv_desc g = *d;      // the gradient's direction: dz -> dx
    g.H = Ho; g.W = Wo; g.Cin = d->Cout; g.in_cstride = dz_cstride;
    g.Cout = d->Cin; g.out_cstride = d->in_cstride; g.res_cstride = d->in_cstride;
    g.stride = 1; g.pad = d->ksize - 1 - d->pad;
    g.act = RYOLO_ACT_LINEAR; g.slope = 0.f; g.upsample = 1;
    const int ncls = d->stride == 1 ? 1 : (xfuse ? 2 : 4);
    const int wrows = xfuse ? (2 * d->Cin + 127) / 128 * 128 : rows;
    for (int cls = 0; cls < ncls; cls++) {
        int dy[9], dxx[9], khs[9], kws[9];
        const int nt = xfuse ? dgrad_xfused_class(cls, dy, dxx, khs, kws, kws)
                             : dgrad_classes(d->ksize, d->stride, d->pad, cls, dy, dxx, khs, kws);
        ConvParams &p = out.p[out.n];
        p = ConvParams{};
        if (!conv_shape(&g, p)) return false;
        p.x = (const __bf16 *)dz;
        p.w = (const __bf16 *)wsrc;
        p.scale = ones; p.shift = zeros;
        // (the folded reduce is planned for the accumulating form whatever `accumulate` says, as its rows query plans it: a launch that
        // only stores stays within every guard of the one that also reads dx)
        p.res = accumulate || want_reduce ? (const __bf16 *)dx : nullptr;
        p.y = (__bf16 *)dx;
        p.K = nt * d->Cout;
        p.Kpad = (p.K + BK - 1) / BK * BK;
        p.cin_log2 = ilog2_exact(d->Cout);
        p.ntaps = nt;
        for (int t = 0; t < 9; t++) { p.tap_dy[t] = t < nt ? dy[t] : 0; p.tap_dx[t] = t < nt ? dxx[t] : 0; }
        wsrc += ((size_t)wrows * p.Kpad + 128) * 2;
        if (d->stride == 2) {
            // the class's grid of input pixels, placed with step 2 in dx; its taps carry their own offsets (no padding)
            const int a = xfuse ? cls : cls >> 1, b = cls & 1;
            p.pad = 0;
            p.OH = d->H;
            p.os = 2; p.ooy = a;
            if (xfuse) {      // rows of parity `cls` x pixel PAIRS
                p.Cout = 2 * d->Cin; p.out_cs = 2 * d->in_cstride; p.res_cs = 2 * d->in_cstride;
                p.osx = 1; p.OW = d->W / 2;
                if ((d->H - a + 1) / 2 <= 0 || d->W / 2 <= 0) continue;
                if (!conv_pixels(p, (d->H - a + 1) / 2, d->W / 2)) return false;
            } else {
                p.osx = 2; p.oox = b; p.OW = d->W;
                if ((d->H - a + 1) / 2 <= 0 || (d->W - b + 1) / 2 <= 0) continue;
                if (!conv_pixels(p, (d->H - a + 1) / 2, (d->W - b + 1) / 2)) return false;
            }
        }
        p.fast = (d->Cout % BK == 0) && buffer_extent(dz_pix, dz_cstride, d->Cout, &p.x_bytes) && buffer_extent(wrows, p.Kpad, p.Kpad + 128, &p.w_bytes);
        if (!p.fast) p.x_bytes = p.w_bytes = 0;
        if (!p.fast && (d->stride != 1 || (d->ksize == 3 && p.cin_log2 < 0))) return false;
        p.no_persist = (d->tile & 0x200) ? 1 : 0;
        p.pw_grid_cap = (d->tile & 0xff) == 13 ? (d->tile >> 16) & 0xff : 0;
        p.nt_out = out.nt_out;
        out.pl[out.n] = conv_plan(p, d->ksize, d->tile & 0xff, want_reduce);
        if (!accumulate) p.res = nullptr;
        out.n++;
    }
    return true;
}

static int dgrad_launch(DgradPlan &dp, const ryolo_conv_desc *d, const void *dz, int dz_cstride, const void *packed_dgrad, void *dx, int accumulate,
                        const ConvLaunch &lc) {
    if (dp.stem) return launch_conv_stem_dgrad(dp.stem_plan, d, dz, dz_cstride, packed_dgrad, dx, accumulate, dp.nt_out, lc);
    if (!dp.launchable()) return RYOLO_EINVAL;
    for (int i = 0; i < dp.n; i++) {
        const int rc = conv_launch(dp.pl[i], dp.p[i], lc);
        if (rc != RYOLO_OK) return rc;
    }
    return RYOLO_OK;
}

// the plan the queries read: the accumulating data gradient of `d` over a dense dz
static bool dgrad_query(const ryolo_conv_desc *d, bool want_reduce, DgradPlan &dp) {
    void *fake = (void *)(uintptr_t)4096;      // never dereferenced: nothing is launched
    return d && dgrad_plan(d, fake, d->Cout, fake, (const float *)fake, (const float *)fake, fake, 1, want_reduce, dp);
}

extern "C" {

// rows of partial sums the fused launch writes (= workgroups of a persistent launch, pixel tiles of a one-tile-per-workgroup launch), 0 when
// this conv's data gradient cannot carry the reduce: stride 1, and one of the kernels with the folded pass (conv_plan(): the persistent
// 2x2 tile / conv_pw.hip for 1x1 layers with whole 128-channel tiles, the narrow and the 128 x 128 one-tile kernels otherwise)
int ryolo_conv2d_dgrad_bnreduce_rows(const ryolo_conv_desc *d) {
    DgradPlan dp;
    return dgrad_query(d, true, dp) && dp.n == 1 ? dp.pl[0].rows : 0;
}

int ryolo_conv2d_dgrad(const ryolo_conv_desc *d /* the FORWARD conv */, const void *dz, int dz_cstride,
                       const void *packed_dgrad, const float *ones, const float *zeros, void *dx, int accumulate,
                       void *stream_) {
    if (!dz || !packed_dgrad || !ones || !zeros || !dx) return RYOLO_EINVAL;
    DgradPlan dp;
    if (!dgrad_plan(d, dz, dz_cstride, packed_dgrad, ones, zeros, dx, accumulate, false, dp)) return RYOLO_EINVAL;
    ConvLaunch lc;
    lc.stream = (hipStream_t)stream_;
    return dgrad_launch(dp, d, dz, dz_cstride, packed_dgrad, dx, accumulate, lc);
}

int ryolo_conv2d_dgrad_bnreduce(const ryolo_conv_desc *d, const void *dz, int dz_cstride, const void *packed_dgrad, const float *ones,
                                const float *zeros, void *dx, int accumulate, const void *z, int z_cstride, const float *scale,
                                const float *shift, const float *mean, const float *invstd, const float *slope, float *part,
                                void *stream_) {
    if (!d || !z || (z_cstride & 7) || z_cstride < d->Cin || !scale || !shift || !mean || !invstd || !slope || !part || d->in_cstride != d->Cin ||
        !dz || !packed_dgrad || !ones || !zeros || !dx)
        return RYOLO_EINVAL;
    DgradPlan dp, asked;
    if (!dgrad_plan(d, dz, dz_cstride, packed_dgrad, ones, zeros, dx, accumulate, true, dp) || dp.n != 1 || dp.pl[0].kernel < 0 || dp.pl[0].rows <= 0)
        return RYOLO_EINVAL;
    // the caller sized `part` by ryolo_conv2d_dgrad_bnreduce_rows(), which plans a dense dz: a strided one must come to the same rows
    if (dz_cstride != d->Cout && (!dgrad_query(d, true, asked) || asked.n != 1 || asked.pl[0].rows != dp.pl[0].rows)) return RYOLO_EINVAL;
    BnRed br;
    br.z = (const __bf16 *)z; br.z_cs = z_cstride; br.scale = scale; br.shift = shift; br.mean = mean; br.invstd = invstd;
    br.slope = slope; br.part = part;
    ConvLaunch lc;
    lc.bnred = &br;
    lc.stream = (hipStream_t)stream_;
    return dgrad_launch(dp, d, dz, dz_cstride, packed_dgrad, dx, accumulate, lc);
}

int ryolo_conv_dgrad_kernel_choice(const ryolo_conv_desc *d, int with_bn_reduce) {
    DgradPlan dp;
    return dgrad_query(d, with_bn_reduce != 0, dp) ? dp.kernel() : -1;
}

}  // extern "C"
