// rotate-yolov3_amd/csrc/wgrad_dil.hip -- the weight gradient of the 3x3 / stride 1 DILATED convolution of conv_dil.hip (dilation (dh, dw),
// padding (dh, dw)) on gfx950:
//     dW[co][ci][r][s] = sum_{n,h,w} dy[n][h][w][co] * x[n][h + (r-1)*dh][w + (s-1)*dw][ci],   zero outside the image.
//
// What it is for: training the "matrix" cfgs of the reference, whose d-convolutional blocks with weight_from = s run
// F.conv2d(x, module_list[s].Conv2d.weight, padding=dil, dilation=dil) (model/models.py:254-267) and get this sum from autograd; several
// sharers add their gradients into the one source weight (accumulate = 1, in launch order).
//
// GEMM view, as in wgrad.hip: M = c_out, N = c_in of ONE tap, K = the N*H*W pixels.  Both operands are pixel-major NHWC bf16 with pixel
// strides (channel slices of wider buffers work), i.e. K is the slow index of both, so the tiles are staged [pixel][channel] with 16-B
// direct-to-LDS loads and the MFMA fragments are read TRANSPOSED from LDS (ds_read_b64_tr_b16, two reads per 8-pixel fragment; the 32-B
// chunk-pair XOR of wgrad.hip keeps the eight rows of a service group on distinct banks).
//
// This first version is the plain ONE-TAP tile: a workgroup owns (split, tap, c_out tile, c_in tile), T x T with T = 128 (64 when a
// channel count does not fill 128), 4 waves as 2 x 2, 64 pixels per K step, two stages, one barrier per step -- the two-stage square tile
// of wgrad.hip with the tap's pixel shift dilated.  (The three-taps-per-workgroup form that shares the staged dy rows of a filter row, the
// wgrad_wide<128, 3 x 64> tile, is not built yet.)
//
// Border: decided per staged pixel and per tap, the row and the column tested separately -- tap (r, s) of image 1 above row 0 is a valid
// flat offset that lands in image 0 (conv_dil.hip says the same of the forward), so a test of the flat offset would sum a neighbour's
// pixels.  A masked lane gets an out-of-range buffer offset: the hardware writes zeros to LDS, nothing is read.
//
// Split-K: the pixel range is cut into S chunks (a multiple of the 64-pixel K step); every workgroup writes its fp32 partial tile to
// part[split][co][tap*C_in + ci] in the caller's workspace and ONE launch sums the S tiles in a fixed order into the fp32 OIHW gradient
// (overwrite or add).  No atomics: the result is bit-reproducible and does not depend on what the workspace held.  S is a function of the
// shape alone (never of the device), so the bits do not depend on the machine either.
#include "conv_common.h"

using namespace ryolo_detail;

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));

// [4 pixel rows][16 channels] -> lane (channel) holds the 4 pixels: lane i, element j <- element i&3 of the 8 bytes addressed by lane 4j + (i>>2)
__device__ __forceinline__ s16x4 lds_read_tr16(const char *addr) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(addr));
#else
    return s16x4{0, 0, 0, 0};
#endif
}

// XOR applied to the 32-B chunk-pair index of staged pixel row `row` (row stride T*2 bytes): rows {0..3, 8..11} (+4, +32) are read together
// by one 32-lane service group and must cover 8 distinct 32-B bank groups of the 256-B bank line
template <int T>
__device__ __forceinline__ int wd_swz(int row) {
    if (T >= 128) return (row & 3) | (((row >> 3) & 1) << 2);
    return ((row >> 1) & 1) | (((row >> 3) & 1) << 1);
}

constexpr int KP = 64;            // pixels per K step
constexpr int WD_TARGET = 512;    // workgroups the split aims at: two per CU of a 256-CU part (a constant: the split must not depend on the device)

struct WgDilParams {
    const __bf16 *x;     // forward input, NHWC, pixel stride x_cs
    const __bf16 *dz;    // gradient of the conv output, NHWC, pixel stride dz_cs
    float *part;         // [S][Cout_pad][Kpad] fp32 partial tiles
    int N, H, W, Cin, x_cs, Cout, dz_cs;
    int dil_h, dil_w;
    int Kpad, Cout_pad;  // 9 * Cin; Cout rounded up to 128
    int M;               // N*H*W
    int S, chunk;        // splits, pixels per split (multiple of KP)
    int co_tiles, ci_tiles, T;
    unsigned x_bytes, dz_bytes;
};

template <int T>   // workgroup tile T x T (co x ci), 4 waves as 2 x 2, wave tile (T/2) x (T/2)
__global__ void __launch_bounds__(256) wgrad_dil_kernel(const WgDilParams p) {
    constexpr int WT = T / 2, NF = WT / 16;           // frags per wave per operand
    constexpr int CHUNKS = T / 8;                     // 16-B chunks per staged pixel row
    constexpr int ROWB = T * 2;                       // bytes per staged pixel row
    constexpr int TILE_B = KP * ROWB;                 // one operand tile
    constexpr int PIECES = TILE_B / 1024;             // 1-KiB direct-to-LDS pieces per operand tile
    constexpr int PPW = PIECES / 4;                   // pieces per wave
    constexpr int PIX_PER_PIECE = 64 / CHUNKS;        // pixels covered by one piece
    static_assert(T == 64 || T == 128, "tile");
    static_assert(PIECES % 4 == 0, "pieces must split over the 4 waves");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 stages][A tile | B tile]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // workgroups are dealt to the 8 XCDs round-robin; give each XCD a CONTIGUOUS range of logical ids so the taps / channel tiles of one
    // pixel split (which stream the same dz and x rows) share one L2
    int b = blockIdx.x;
    {
        const int per = gridDim.x >> 3;
        if (b < per * 8) b = (b & 7) * per + (b >> 3);
    }
    const int ci_t = b % p.ci_tiles; b /= p.ci_tiles;
    const int co_t = b % p.co_tiles; b /= p.co_tiles;
    const int tap = b % 9; b /= 9;
    const int split = b;
    const int dy = (tap / 3 - 1) * p.dil_h, dx = (tap % 3 - 1) * p.dil_w;       // the tap's pixel shift
    const int co0 = co_t * T, ci0 = ci_t * T;
    const int pix_lo = split * p.chunk, pix_hi = min(p.M, pix_lo + p.chunk);

    // staging bookkeeping: lane -> (pixel within piece, chunk slot); the lane's pixel as (img, ho, wo), advanced by KP per step
    const int lp = lane / CHUNKS, lc = lane % CHUNKS;
    int b_img[PPW], b_ho[PPW], b_wo[PPW], s_pix[PPW];
#pragma unroll
    for (int j = 0; j < PPW; j++) {
        const int tp = (wave * PPW + j) * PIX_PER_PIECE + lp;       // tile-local pixel
        s_pix[j] = tp;
        const int pg = pix_lo + tp;
        b_wo[j] = pg % p.W;
        const int t = pg / p.W;
        b_ho[j] = t % p.H;
        b_img[j] = t / p.H;
    }

    auto stage = [&](int kt, int buf) {
        char *abuf = smem + buf * 2 * TILE_B;
        char *bbuf = abuf + TILE_B;
#pragma unroll
        for (int j = 0; j < PPW; j++) {
            const int piece = wave * PPW + j;
            const int pg = pix_lo + kt * KP + s_pix[j];
            const int chunk = lc ^ (wd_swz<T>(s_pix[j]) << 1);       // logical chunk stored at slot lc
            const bool in_rng = pg < pix_hi;
            // A: dz row (contiguous pixel order); channels past C_out (ragged last tile) are zeros
            const bool a_ok = in_rng && (co0 + chunk * 8 < p.Cout);
            const int a_v = a_ok ? (int)(((unsigned)pg * p.dz_cs + co0 + chunk * 8) * 2u) : (int)0x80000000;      // (the host checked: below 2^31 bytes)
            buffer_load_lds16(p.dz, p.dz_bytes, abuf + piece * 1024, a_v, 0);
            // B: x row of the tap-shifted pixel; row and column tested separately
            const int hi = b_ho[j] + dy, wi = b_wo[j] + dx;
            const bool b_ok = in_rng && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W && (ci0 + chunk * 8 < p.Cin);
            const int b_v = b_ok ? (int)(((unsigned)((b_img[j] * p.H + hi) * p.W + wi) * p.x_cs + ci0 + chunk * 8) * 2u) : (int)0x80000000;
            buffer_load_lds16(p.x, p.x_bytes, bbuf + piece * 1024, b_v, 0);
            // advance this lane's pixel by KP for the next call
            b_wo[j] += KP;
            while (b_wo[j] >= p.W) {
                b_wo[j] -= p.W;
                if (++b_ho[j] == p.H) { b_ho[j] = 0; b_img[j]++; }
            }
        }
    };

    // transpose-read addressing: in k-group kg, lane fr addresses pixel row kg*8 + (fr>>2) (+4 for the second read, +32 for the second
    // k-substep) and the 8 bytes of channels 4*(fr&3).. of the fragment's 16-channel pair
    const int wr = wave >> 1, wc = wave & 1;
    const int fr = lane & 15, kg = lane >> 4;
    const int trow = kg * 8 + (fr >> 2);
    const int tsw = wd_swz<T>(trow);
    const int tbase = trow * ROWB + (fr & 3) * 8;
    int offa[NF], offb[NF];
#pragma unroll
    for (int f = 0; f < NF; f++) {
        offa[f] = tbase + ((((wr * WT) >> 4) + f) ^ tsw) * 32;
        offb[f] = tbase + ((((wc * WT) >> 4) + f) ^ tsw) * 32;
    }

    f32x4 acc[NF][NF];
#pragma unroll
    for (int a = 0; a < NF; a++)
#pragma unroll
        for (int c = 0; c < NF; c++) acc[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nsteps = (pix_hi - pix_lo + KP - 1) / KP;
    if (nsteps > 0) stage(0, 0);
    for (int kt = 0; kt < nsteps; kt++) {
        __syncthreads();   // drains this wave's direct-to-LDS loads and orders all waves: step kt landed, nobody still reads the other buffer
        if (kt + 1 < nsteps) stage(kt + 1, (kt + 1) & 1);
        const char *abuf = smem + (kt & 1) * 2 * TILE_B;
        const char *bbuf = abuf + TILE_B;
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            bf16x8 af[NF], bfr[NF];
#pragma unroll
            for (int f = 0; f < NF; f++) {
                const s16x4 a0 = lds_read_tr16(abuf + offa[f] + (ks * 32) * ROWB);
                const s16x4 a1 = lds_read_tr16(abuf + offa[f] + (ks * 32 + 4) * ROWB);
                const s16x4 b0 = lds_read_tr16(bbuf + offb[f] + (ks * 32) * ROWB);
                const s16x4 b1 = lds_read_tr16(bbuf + offb[f] + (ks * 32 + 4) * ROWB);
                af[f] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7));
                bfr[f] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7));
            }
#pragma unroll
            for (int a = 0; a < NF; a++)
#pragma unroll
                for (int c = 0; c < NF; c++)
                    acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bfr[c], acc[a][c], 0, 0, 0);
        }
    }
    // D[row = co (kg*4 + r)][col = ci (fr)]  ->  part[split][co][tap*Cin + ci]; the rows past C_out are not stored
    float *out = p.part + (size_t)split * p.Cout_pad * p.Kpad;
#pragma unroll
    for (int a = 0; a < NF; a++)
#pragma unroll
        for (int c = 0; c < NF; c++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int co = co0 + wr * WT + a * 16 + kg * 4 + r;
                const int ci = ci0 + wc * WT + c * 16 + fr;
                if (co < p.Cout && ci < p.Cin) out[(size_t)co * p.Kpad + tap * p.Cin + ci] = acc[a][c][r];
            }
}

// Sum the S partial tiles into the OIHW fp32 gradient: g[co][ci][r][s] (+)= sum_split part[split][co][tap*Cin + ci].  Threads walk the
// SOURCE order (co, tap, ci): the S reads are coalesced, the one write (read-modify-write with accumulate) of g is strided.  The four waves
// of a workgroup take a quarter of the splits each for the same 64 elements and the quarters are added in a fixed order through LDS: the
// order in which an element's partial values are added depends on S alone.
__global__ void __launch_bounds__(256) wgrad_dil_reduce_kernel(const float *__restrict__ part, int S, int Cout, int Cin, int Kpad, int Cout_pad,
                                                               float *__restrict__ g, int accumulate) {
    __shared__ float sm[256];
    const unsigned per_co = (unsigned)(9 * Cin);
    const unsigned total = (unsigned)Cout * per_co;
    const size_t sstride = (size_t)Cout_pad * Kpad;
    const int e = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int per = (S + 3) / 4;
    const int s_lo = q * per, s_hi = min(S, s_lo + per);
    for (unsigned base = blockIdx.x * 64u; base < total; base += gridDim.x * 64u) {      // (workgroup-uniform trip count)
        const unsigned i = base + e;
        const bool ok = i < total;
        const unsigned co = ok ? i / per_co : 0, rem = ok ? i - co * per_co : 0;
        const unsigned tap = rem / (unsigned)Cin, ci = rem - tap * (unsigned)Cin;
        const float *src = part + (size_t)co * Kpad + rem;
        float v = 0.f;
        if (ok) {
            int s = s_lo;
            for (; s + 4 <= s_hi; s += 4) {      // independent loads in flight
                const float a0 = src[(size_t)s * sstride], a1 = src[(size_t)(s + 1) * sstride];
                const float a2 = src[(size_t)(s + 2) * sstride], a3 = src[(size_t)(s + 3) * sstride];
                v += (a0 + a1) + (a2 + a3);
            }
            for (; s < s_hi; s++) v += src[(size_t)s * sstride];
        }
        sm[threadIdx.x] = v;
        __syncthreads();
        if (ok && q == 0) {
            v = (sm[e] + sm[64 + e]) + (sm[128 + e] + sm[192 + e]);
            const size_t dst = ((size_t)co * Cin + ci) * 9 + tap;
            g[dst] = accumulate ? g[dst] + v : v;
        }
        __syncthreads();
    }
}

// what the kernel serves, and the launch geometry of a served descriptor (no device call)
bool wgrad_dil_params(const ryolo_conv_desc *d, int dil_h, int dil_w, int dz_cstride, WgDilParams &p) {
    if (conv_validate(d) != RYOLO_OK) return false;
    if (d->ksize != 3 || d->stride != 1 || d->pad != 1 || d->upsample != 1 || (d->Cin % 64)) return false;
    if (dil_h < 1 || dil_h > 32 || dil_w < 1 || dil_w > 32) return false;
    if ((dz_cstride & 7) || dz_cstride < d->Cout) return false;
    const long long M = (long long)d->N * d->H * d->W;
    if (M > 0x7fffffffLL - 512) return false;
    // 31-bit byte offsets over both operands
    if (!buffer_extent((unsigned long long)M, d->in_cstride, d->Cin, &p.x_bytes) ||
        !buffer_extent((unsigned long long)M, dz_cstride, d->Cout, &p.dz_bytes))
        return false;
    p.N = d->N; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.Cout = d->Cout;
    p.x_cs = d->in_cstride; p.dz_cs = dz_cstride;
    p.dil_h = dil_h; p.dil_w = dil_w;
    p.M = (int)M;
    p.Kpad = 9 * d->Cin;
    p.Cout_pad = (d->Cout + 127) / 128 * 128;
    p.T = (d->Cin % 128 == 0 && d->Cout >= 128) ? 128 : 64;
    p.co_tiles = (d->Cout + p.T - 1) / p.T;
    p.ci_tiles = d->Cin / p.T;
    // the split (wgrad.hip's rule): ONE round of at most two workgroups per CU of a 256-CU part -- a few workgroups more than a round cost a
    // whole second round; with few splits the count (<= 5) that wastes the least of the last round; at most one split per K step, partial
    // tiles within 512 MiB
    const long long base = 9ll * p.co_tiles * p.ci_tiles, max_s = (M + KP - 1) / KP;
    long long S = WD_TARGET / base;
    if (2 * base > WD_TARGET) {
        double best = -1.0;
        for (int c = 1; c <= 5; c++) {
            const long long blocks = c * base;
            const double eff = (double)blocks / (double)((blocks + WD_TARGET - 1) / WD_TARGET * WD_TARGET);
            if (eff > best + 0.02) { best = eff; S = c; }
        }
    }
    if (S > max_s) S = max_s;
    const long long per = (long long)p.Cout_pad * p.Kpad * 4;
    while (S > 1 && per * S > (512ll << 20)) S--;
    if (S < 1) S = 1;
    long long chunk = (M + S - 1) / S;
    chunk = (chunk + KP - 1) / KP * KP;
    p.S = (int)((M + chunk - 1) / chunk);
    p.chunk = (int)chunk;
    return base * p.S <= 0x7fffffffLL && per <= (512ll << 20);
}

size_t wgrad_dil_part_bytes(const WgDilParams &p) { return (size_t)p.S * p.Cout_pad * p.Kpad * 4; }

}  // namespace

extern "C" {

int ryolo_conv2d_dilated_wgrad_supported(const ryolo_conv_desc *d, int dil_h, int dil_w) {
    WgDilParams p{};
    return d && wgrad_dil_params(d, dil_h, dil_w, d->out_cstride, p) ? 1 : 0;
}

size_t ryolo_conv2d_dilated_wgrad_workspace_bytes(const ryolo_conv_desc *d, int dil_h, int dil_w) {
    WgDilParams p{};
    return d && wgrad_dil_params(d, dil_h, dil_w, d->out_cstride, p) ? wgrad_dil_part_bytes(p) : 0;
}

int ryolo_conv2d_dilated_wgrad(const ryolo_conv_desc *d, int dil_h, int dil_w, const void *x, const void *dz, int dz_cstride,
                               float *grad_oihw, int accumulate, void *workspace, size_t workspace_bytes, void *stream_) {
    if (!d || !x || !dz || !grad_oihw || !workspace) return RYOLO_EINVAL;
    if (((uintptr_t)x | (uintptr_t)dz | (uintptr_t)workspace) & 15 || ((uintptr_t)grad_oihw & 3)) return RYOLO_EINVAL;
    WgDilParams p{};
    if (!wgrad_dil_params(d, dil_h, dil_w, dz_cstride, p)) return RYOLO_EINVAL;
    if (workspace_bytes < wgrad_dil_part_bytes(p)) return RYOLO_EINVAL;
    p.x = (const __bf16 *)x;
    p.dz = (const __bf16 *)dz;
    p.part = (float *)workspace;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)(9 * p.co_tiles * p.ci_tiles * p.S)), block(256);
    const int rc = p.T == 128 ? launch_kernel<wgrad_dil_kernel<128>>(grid, block, (size_t)4 * KP * 128 * 2, stream, p)
                              : launch_kernel<wgrad_dil_kernel<64>>(grid, block, (size_t)4 * KP * 64 * 2, stream, p);
    if (rc != RYOLO_OK) return rc;
    const long long total = (long long)p.Cout * 9 * p.Cin;
    return launch_kernel<wgrad_dil_reduce_kernel>(dim3((unsigned)grid_for(total, 64, 8192)), dim3(256), 0, stream, (const float *)p.part, p.S,
                                                  p.Cout, p.Cin, p.Kpad, p.Cout_pad, grad_oihw, accumulate ? 1 : 0);
}

}  // extern "C"
