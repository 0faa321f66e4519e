// rotate-yolov3_amd/csrc/conv_dil.hip -- 3x3 / stride 1 DILATED convolution (dilation (dh, dw), padding (dh, dw), output H x W) as an
// NHWC bf16 implicit GEMM on MFMA for gfx950, with the block epilogue of include/ryolo.h:
//     y = bf16(act(acc * scale[c] + shift[c])), then bf16(y + residual) when a residual is given.
//
// What it is for: the "matrix" cfgs of the reference (cfg/HRSC+/yolov3_512_matrix.cfg, cfg/yolov3-m.cfg) hang shared-weight branches off
// the FPN levels whose 3x3 convs are anisotropically dilated -- F.conv2d(x, module_list[s].Conv2d.weight, padding=dil, dilation=dil),
// model/models.py:254-267.  The filter is the packed image ryolo_conv_pack_weights makes for the source layer's own (undilated) launch:
// k = (r*3 + s)*C_in + c, so one packed copy serves the source and every sharer.
//
// GEMM view: D[c_out][pixel] = sum_k Wp[c_out][k] * X[pixel][k], M = N*H*W pixels, K = 9*C_in, C_in % 64 == 0 so that a 64-wide K step
// lies inside ONE tap: tap (r, s) of output pixel (img, ho, wo) reads input pixel (ho + (r-1)*dh, wo + (s-1)*dw).  The row and the
// column are tested separately -- a tap above row 0 of image 1 is a valid flat offset (it lands in image 0), so a test of the flat offset
// would read a neighbour's pixels -- and the nine results are a per-lane bit mask built once per tile.  A lane whose tap is outside gets
// an out-of-range buffer offset: the hardware writes zeros to LDS, nothing is read.
//
// It is the one-tile-per-workgroup kernel of conv.hip (same LDS image: [row][8 x 16-B slots], slot ^= (row >> 1) & 7; direct-to-LDS
// 16-B buffer loads, double buffered, one barrier per K step; weights as the MFMA A operand so a lane holds 4 consecutive channels of a
// pixel), reduced to what this layer family needs and with a tile choice for ITS shapes: the maps are 16^2 .. 64^2 at 512^2 input, so at
// batch 1 a level has 256 .. 4096 pixels and a 128 x 128 tile leaves most of the chip idle.  Two instantiations:
//     128 pixels x 128 channels, 2 x 2 waves    when that tile list fills the CUs
//      64 pixels x  64 channels, 2 x 2 waves    otherwise (4 x the workgroups, K loop unchanged)
// No split-K and no atomics on the output: every output element has one writer and a fixed summation order, the result is bit-reproducible.
#include "conv_common.h"

using namespace ryolo_detail;

namespace {

struct DilParams {
    const __bf16 *x;       // input, NHWC, pixel stride in_cs; already offset to its channel slice
    const __bf16 *w;       // packed filter [cpad(Cout)][9*Cin] + zero tail
    const float *scale;    // [cpad(Cout)]
    const float *shift;
    const __bf16 *res;     // residual on the output's pixel grid, or nullptr
    __bf16 *y;
    int N, H, W, Cin, Cout, in_cs, out_cs, res_cs;
    int dil_h, dil_w;
    int M, Kpad, nt;
    int act;
    float slope;
    unsigned x_bytes, w_bytes;
};

template <int BM, int BN, int WGM, int WGN>
__global__ void __launch_bounds__(WGM *WGN * 64) conv_dil_kernel(const DilParams p) {
    constexpr int NW = WGM * WGN, NT = NW * 64;
    constexpr int WPIX = BM / WGM, WCH = BN / WGN, PF = WPIX / 16, CF = WCH / 16;
    constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE = A_BYTES + B_BYTES;
    constexpr int A_PPW = (BM / 8) / NW, B_PPW = (BN / 8) / NW;   // 1-KiB pieces (8 tile rows) per wave
    static_assert(A_PPW >= 1 && B_PPW >= 1, "tile too small for the wave count");
    constexpr int SROW = BN * 2 + 16;                              // epilogue staging row pitch (bytes)
    static_assert(BM * SROW <= 2 * STAGE, "staging tile must fit in the operand buffers");

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // XCD-aware tile assignment (bijective for any grid size): channel tiles fastest, contiguous chunks per XCD
    int m_tile, n_tile;
    {
        const int nblk = gridDim.x, bid = blockIdx.x;
        const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7, loc = bid >> 3;
        const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
        n_tile = id % p.nt;
        m_tile = id / p.nt;
    }
    const int m0 = m_tile * BM, n0 = n_tile * BN;

    // ---- per-lane staging bookkeeping.  Lane l of a wave fills 16-B slot (l & 7) of tile row 8*piece + (l >> 3).
    int a_off32[A_PPW];          // byte offset of (img, ho, wo, slot*8): the CENTRE tap; only used where the tap's mask bit is set
    unsigned a_mask[A_PPW];      // bit t: tap t = (t / 3, t % 3) reads inside the image for this lane's pixel
    int b_off32[B_PPW];
#pragma unroll
    for (int j = 0; j < A_PPW; j++) {
        const int row = (wave * A_PPW + j) * 8 + (lane >> 3);
        const int slot = (lane & 7) ^ ((row >> 1) & 7);
        const int m = m0 + row;
        unsigned mk = 0;
        a_off32[j] = 0;
        if (m < p.M) {
            const int t = m / p.W, wo = m - t * p.W, img = t / p.H, ho = t - img * p.H;
            a_off32[j] = m * p.in_cs * 2 + slot * 16;       // (the host checked that the tensor's extent fits 31 bits)
#pragma unroll
            for (int tap = 0; tap < 9; tap++) {
                const int hi = ho + (tap / 3 - 1) * p.dil_h, wi = wo + (tap % 3 - 1) * p.dil_w;
                if ((unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W) mk |= 1u << tap;
            }
        }
        a_mask[j] = mk;
    }
#pragma unroll
    for (int j = 0; j < B_PPW; j++) {
        const int row = (wave * B_PPW + j) * 8 + (lane >> 3);
        const int slot = (lane & 7) ^ ((row >> 1) & 7);
        b_off32[j] = ((n0 + row) * p.Kpad + slot * 8) * 2;      // rows up to cpad(Cout) exist in the packed image
    }

    // running (scalar) position of the K loop: tap (f_r, f_s), channel offset inside the tap
    int f_tap = 0, f_r = 0, f_s = 0, f_c0 = 0;
    auto stage = [&](int kt, int buf) {
        char *abuf = smem + buf * STAGE;
        char *bbuf = abuf + A_BYTES;
        const int tapoff = (((f_r - 1) * p.dil_h * p.W + (f_s - 1) * p.dil_w) * p.in_cs + f_c0) * 2;      // scalar
#pragma unroll
        for (int j = 0; j < A_PPW; j++) {
            const bool ok = (a_mask[j] >> f_tap) & 1u;
            const int voff = ok ? a_off32[j] + tapoff : (int)0x80000000;
            buffer_load_lds16(p.x, p.x_bytes, abuf + (wave * A_PPW + j) * 1024, voff, 0);
        }
#pragma unroll
        for (int j = 0; j < B_PPW; j++)
            buffer_load_lds16(p.w, p.w_bytes, bbuf + (wave * B_PPW + j) * 1024, b_off32[j], kt * (BK * 2));
        f_c0 += BK;
        if (f_c0 >= p.Cin) {
            f_c0 = 0;
            f_tap++;
            if (++f_s == 3) { f_s = 0; f_r++; }
        }
    };

    // ---- fragment read offsets (bytes within a tile image)
    const int wm = wave / WGN, wn = wave % WGN;
    const int frow = lane & 15, fk = lane >> 4;
    int a_off[PF][2], b_off[CF][2];
#pragma unroll
    for (int f = 0; f < PF; f++) {
        const int row = wm * WPIX + f * 16 + frow;
#pragma unroll
        for (int ks = 0; ks < 2; ks++) a_off[f][ks] = row * 128 + (((ks * 4 + fk) ^ ((row >> 1) & 7)) << 4);
    }
#pragma unroll
    for (int f = 0; f < CF; f++) {
        const int row = wn * WCH + f * 16 + frow;
#pragma unroll
        for (int ks = 0; ks < 2; ks++) b_off[f][ks] = row * 128 + (((ks * 4 + fk) ^ ((row >> 1) & 7)) << 4);
    }

    f32x4 acc[CF][PF];
#pragma unroll
    for (int c = 0; c < CF; c++)
#pragma unroll
        for (int f = 0; f < PF; f++) acc[c][f] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int KT = p.Kpad / BK;
    auto compute = [&](int buf) {
        const char *abuf = smem + buf * STAGE;
        const char *bbuf = abuf + A_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            bf16x8 wf[CF], xf[PF];
#pragma unroll
            for (int c = 0; c < CF; c++) wf[c] = *(const bf16x8 *)(bbuf + b_off[c][ks]);
#pragma unroll
            for (int f = 0; f < PF; f++) xf[f] = *(const bf16x8 *)(abuf + a_off[f][ks]);
#pragma unroll
            for (int c = 0; c < CF; c++)
#pragma unroll
                for (int f = 0; f < PF; f++)
                    acc[c][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[c], xf[f], acc[c][f], 0, 0, 0);
        }
    };
    stage(0, 0);
    for (int kt = 0; kt + 1 < KT; kt++) {
        __syncthreads();   // drains this wave's direct-to-LDS loads and orders all waves: tile kt landed, and nobody still reads the
                           // buffer that the next stage() overwrites
        stage(kt + 1, (kt + 1) & 1);
        compute(kt & 1);
    }
    __syncthreads();
    compute((KT - 1) & 1);

    // ---- epilogue 1: scale/shift/activation on the fp32 accumulators -> bf16 -> LDS staging tile
    __syncthreads();
    auto epilogue1 = [&](auto actfn) {
#pragma unroll
        for (int c = 0; c < CF; c++) {
            const int ch_local = wn * WCH + c * 16 + fk * 4;
            const f32x4 sc = *(const f32x4 *)(p.scale + n0 + ch_local);      // scale / shift are padded to cpad(Cout) like the filter rows
            const f32x4 sh = *(const f32x4 *)(p.shift + n0 + ch_local);
#pragma unroll
            for (int f = 0; f < PF; f++) {
                const int pix_local = wm * WPIX + f * 16 + frow;
                bf16x4 o;
#pragma unroll
                for (int r = 0; r < 4; r++) o[r] = (__bf16)actfn(acc[c][f][r] * sc[r] + sh[r]);
                *(bf16x4 *)(smem + pix_local * SROW + ch_local * 2) = o;
            }
        }
    };
    const float slope = p.slope;
    if (p.act == RYOLO_ACT_LEAKY) epilogue1([slope](float v) { return v > 0.f ? v : v * slope; });
    else epilogue1([](float v) { return v; });
    __syncthreads();

    // ---- epilogue 2: coalesced 16-B rows: (+ residual, fp32 add, one more bf16 rounding) -> global.  Chunks past M or Cout are skipped:
    // nothing is written outside the output's channel slice
    constexpr int CPR = BN / 8;              // 16-B chunks per staged row
    constexpr int NIT = BM * CPR / NT;       // chunks per thread
    static_assert(BM * CPR % NT == 0, "tile chunks must divide evenly over the threads");
    bf16x8 rv[NIT];
    if (p.res) {
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int idx = it * NT + tid;
            const int m = m0 + idx / CPR, c = n0 + (idx % CPR) * 8;
            const bool ok = (m < p.M) && (c < p.Cout);
            rv[it] = ok ? *(const bf16x8 *)(p.res + (size_t)m * p.res_cs + c) : bf16x8{};
        }
    }
#pragma unroll
    for (int it = 0; it < NIT; it++) {
        const int idx = it * NT + tid;
        const int pix = idx / CPR, ch = (idx % CPR) * 8;
        const int m = m0 + pix, c = n0 + ch;
        if (m >= p.M || c >= p.Cout) continue;
        bf16x8 v = *(const bf16x8 *)(smem + pix * SROW + ch * 2);
        if (p.res) {
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = (__bf16)((float)v[e] + (float)rv[it][e]);
        }
        *(bf16x8 *)(p.y + (size_t)m * p.out_cs + c) = v;
    }
}

template <int BM, int BN>
int launch_dil(DilParams &p, hipStream_t stream) {
    constexpr size_t smem = 2 * (BM + BN) * BK * 2;
    p.nt = (p.Cout + BN - 1) / BN;
    const dim3 grid((unsigned)(((long long)p.M + BM - 1) / BM * p.nt)), block(256);
    return launch_kernel<conv_dil_kernel<BM, BN, 2, 2>>(grid, block, smem, stream, p);
}

// what the kernel serves, and the launch geometry of a served descriptor
bool dil_params(const ryolo_conv_desc *d, int dil_h, int dil_w, DilParams &p) {
    if (conv_validate(d) != RYOLO_OK) return false;
    if (d->ksize != 3 || d->stride != 1 || d->pad != 1 || d->upsample != 1 || (d->Cin % BK)) return false;
    if (dil_h < 1 || dil_h > 32 || dil_w < 1 || dil_w > 32) return false;
    if (d->act != RYOLO_ACT_LINEAR && d->act != RYOLO_ACT_LEAKY) return false;
    if (d->res_cstride && ((d->res_cstride & 7) || d->res_cstride < d->Cout)) return false;
    const long long M = (long long)d->N * d->H * d->W;
    if (M > 0x7fffffffLL - 512) return false;
    p.N = d->N; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.Cout = d->Cout;
    p.in_cs = d->in_cstride; p.out_cs = d->out_cstride; p.res_cs = d->res_cstride;
    p.dil_h = dil_h; p.dil_w = dil_w;
    p.M = (int)M;
    p.Kpad = 9 * d->Cin;                 // a multiple of BK: the packed image has no K padding
    p.act = d->act; p.slope = d->slope;
    // 31-bit byte offsets over the input slice and the packed filter (rows up to cpad(Cout), + the zero tail)
    return buffer_extent((unsigned long long)M, d->in_cstride, d->Cin, &p.x_bytes) &&
           buffer_extent((d->Cout + 127) / 128 * 128, p.Kpad, p.Kpad + 128, &p.w_bytes);
}

// The data gradient of the forward conv `f`: dx[n,h,w,ci] = sum_{r,s,co} dy[n, h-(r-1)*dh, w-(s-1)*dw, co] * W[co,ci,r,s] is the same dilated
// convolution applied to dy with the spatially flipped, channel-transposed filter and the same dilation -- the kernel above on a descriptor
// with the channel counts swapped, the packed image of W'[ci][co][r][s] = W[co][ci][2-r][2-s] (for these shapes exactly the stride-1 image
// of ryolo_conv_pack_weights_dgrad), scale 1, shift 0, linear.  Served when the forward is and C_out (the K channel count here) % 64 == 0.
bool dil_dgrad_params(const ryolo_conv_desc *f, int dil_h, int dil_w, int dz_cstride, DilParams &p) {
    DilParams fwd{};
    if (!dil_params(f, dil_h, dil_w, fwd) || (f->Cout % BK) || (f->Cin & 7)) return false;
    ryolo_conv_desc g = *f;
    g.Cin = f->Cout; g.Cout = f->Cin;
    g.in_cstride = dz_cstride; g.out_cstride = f->in_cstride; g.res_cstride = 0;
    g.act = RYOLO_ACT_LINEAR;
    return dil_params(&g, dil_h, dil_w, p);
}

// the 128 x 128 tile when its tile list gives every CU a workgroup, else the 64 x 64 tile (four times the workgroups)
int launch_dil_auto(DilParams &p, hipStream_t stream) {
    const long long big = ((long long)p.M + 127) / 128 * ((p.Cout + 127) / 128);
    if (big >= cu_count()) return launch_dil<128, 128>(p, stream);
    return launch_dil<64, 64>(p, stream);
}

}  // namespace

extern "C" {

int ryolo_conv2d_dilated_dgrad_supported(const ryolo_conv_desc *f, int dil_h, int dil_w) {
    DilParams p{};
    return f && dil_dgrad_params(f, dil_h, dil_w, f->out_cstride, p) ? 1 : 0;
}

int ryolo_conv2d_dilated_dgrad(const ryolo_conv_desc *f /* the FORWARD conv */, int dil_h, int dil_w, const void *dz, int dz_cstride,
                               const void *packed_dgrad, const float *ones, const float *zeros, void *dx, void *stream) {
    if (!f || !dz || !packed_dgrad || !ones || !zeros || !dx) return RYOLO_EINVAL;
    if (((uintptr_t)dz | (uintptr_t)dx | (uintptr_t)packed_dgrad | (uintptr_t)ones | (uintptr_t)zeros) & 15) return RYOLO_EINVAL;
    DilParams p{};
    if (!dil_dgrad_params(f, dil_h, dil_w, dz_cstride, p)) return RYOLO_EINVAL;
    p.x = (const __bf16 *)dz;
    p.w = (const __bf16 *)packed_dgrad;
    p.scale = ones;
    p.shift = zeros;
    p.res = nullptr;
    p.y = (__bf16 *)dx;
    return launch_dil_auto(p, (hipStream_t)stream);
}

int ryolo_conv2d_dilated_supported(const ryolo_conv_desc *d, int dil_h, int dil_w) {
    DilParams p{};
    return dil_params(d, dil_h, dil_w, p) ? 1 : 0;
}

int ryolo_conv2d_dilated(const ryolo_conv_desc *d, int dil_h, int dil_w, const void *x, const void *w_packed, const float *scale,
                         const float *shift, const void *residual, void *y, void *stream) {
    if (!x || !w_packed || !scale || !shift || !y) return RYOLO_EINVAL;
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)w_packed | (uintptr_t)residual | (uintptr_t)scale | (uintptr_t)shift) & 15) return RYOLO_EINVAL;
    DilParams p{};
    if (!dil_params(d, dil_h, dil_w, p)) return RYOLO_EINVAL;
    if (residual && !d->res_cstride) return RYOLO_EINVAL;
    p.x = (const __bf16 *)x;
    p.w = (const __bf16 *)w_packed;
    p.scale = scale;
    p.shift = shift;
    p.res = (const __bf16 *)residual;
    p.y = (__bf16 *)y;
    return launch_dil_auto(p, (hipStream_t)stream);
}

}  // extern "C"
