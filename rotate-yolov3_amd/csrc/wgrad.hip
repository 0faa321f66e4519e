// rotate-yolov3_amd/csrc/wgrad.hip -- the weight gradient of the convolutions on gfx950: implicit GEMM over pixels on MFMA, split-K,
// fp32 partial tiles and the kernels that reduce them; the plan of a launch and every ryolo_conv*wgrad* entry point.
//
// Replaces what the reference gets from autograd + cuDNN/ATen for `loss.backward()` (train.py:278-282) over the nn.Conv2d of
// model/models.py:49-66.
//
// wgrad:  dW[co][tap][ci] = sum_pix dz[pix][co] * x[pix (+) tap][ci].  GEMM with M = co, N = ci, K = pixels.  Both
// operands are pixel-major (NHWC), i.e. K is the SLOW index of both, so the MFMA fragments (8 consecutive k per lane)
// are read TRANSPOSED from LDS: the tiles are staged [pixel][channel] with 16-B direct-to-LDS loads and each 16-lane
// group pulls its [4 pixels][16 channels] block with the gfx950 transpose read (ds_read_b64_tr_b16: lane i, element j
// <- element i&3 of the 8 bytes addressed by lane 4j + (i>>2)), two reads per 8-pixel fragment.  A 32-B chunk-pair
// XOR keyed on the pixel row (wg_swz) puts the eight rows a 32-lane service group touches on distinct banks.  The pixel
// range is split over workgroups (split-K); partial tiles go to an fp32 workspace and one kernel reduces them and
// un-packs into the OIHW gradient.  Bound: MFMA.
#include "conv_common.h"

using namespace ryolo_detail;

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// [4 pixel rows][16 channels] -> lane (channel) holds the 4 pixels; see the header comment for the lane mapping
__device__ __forceinline__ s16x4 lds_read_tr16(const char *addr) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(addr));
#else
    return s16x4{0, 0, 0, 0};
#endif
}

// XOR applied to the 32-B chunk-pair index of staged pixel row `row` (row stride T*2 bytes): rows {0..3, 8..11} (+4, +32)
// are read together by one 32-lane service group and must cover 8 distinct 32-B bank groups of the 256-B bank line.
template <int T>
__device__ __forceinline__ int wg_swz(int row) {
    if (T >= 128) return (row & 3) | (((row >> 3) & 1) << 2);
    if (T == 64) return ((row >> 1) & 1) | (((row >> 3) & 1) << 1);
    return (row >> 3) & 1;
}

// The same 16-B direct-to-LDS load as inline assembly: the compiler's waitcnt pass puts a full `s_waitcnt vmcnt(0)` in
// front of every LDS read that follows a direct-to-LDS load it knows about, which defeats a multi-stage pipeline retired by
// counted waits (wgrad_wide_kernel); loads issued here are invisible to it and are retired by the kernel's own s_waitcnt.
// (s_nop: one wait state between an SALU write of M0 and the LDS-DMA instruction that reads it.)
typedef int i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ i32x4 make_rsrc_words(const void *base, unsigned bytes) {
    const unsigned long long a = (unsigned long long)base;
    i32x4 r;
    r[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
    r[1] = __builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32));
    r[2] = __builtin_amdgcn_readfirstlane((int)bytes);
    r[3] = 0x00020000;
    return r;
}
__device__ __forceinline__ void buffer_load_lds16_raw(i32x4 rsrc, unsigned lds_addr /* wave-uniform */, int voffset) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lds_addr), "v"(voffset), "s"(rsrc) : "memory", "m0");
#endif
}

constexpr int KP = 64;   // pixels per K step

struct WgradParams {
    const __bf16 *x;     // forward input, NHWC, pixel stride x_cs
    const __bf16 *dz;    // gradient of the conv output, NHWC, pixel stride dz_cs
    float *part;         // [S][Cout_pad][Kpad] fp32 partial tiles
    int N, H, W, Cin, x_cs;
    int Ho, Wo, Cout, dz_cs;
    int ks, stride, pad;
    int Kpad, Cout_pad;
    int M;               // N*Ho*Wo
    int S, chunk;        // splits, pixels per split (multiple of KP)
    int co_tiles, ci_tiles;
    unsigned x_bytes, dz_bytes;
};

template <int T>   // workgroup tile T x T (co x ci), 4 waves as 2 x 2, wave tile (T/2) x (T/2)
__global__ void __launch_bounds__(256) wgrad_kernel(const WgradParams p) {
    constexpr int WT = T / 2, NF = WT / 16;           // frags per wave per operand
    constexpr int CHUNKS = T / 8;                     // 16-B chunks per staged pixel row
    constexpr int ROWB = T * 2;                       // bytes per staged pixel row
    constexpr int TILE_B = KP * ROWB;                 // one operand tile
    constexpr int PIECES = TILE_B / 1024;             // 1-KiB direct-to-LDS pieces per operand tile
    constexpr int PPW = PIECES / 4 > 0 ? PIECES / 4 : 1;
    constexpr int PIX_PER_PIECE = 64 / CHUNKS;        // pixels covered by one piece
    static_assert(PIECES % 4 == 0 || PIECES < 4, "pieces must split over the 4 waves");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 stages][A tile | B tile]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // workgroups are dealt to the 8 XCDs round-robin; give each XCD a CONTIGUOUS range of logical ids so the taps / channel
    // tiles of one pixel split (which stream the same dz and x rows) share one L2 instead of fetching them 8 times
    int b = blockIdx.x;
    {
        const int per = gridDim.x >> 3;
        if (b < per * 8) b = (b & 7) * per + (b >> 3);
    }
    const int ci_t = b % p.ci_tiles; b /= p.ci_tiles;
    const int co_t = b % p.co_tiles; b /= p.co_tiles;
    const int tap = b % (p.ks * p.ks); b /= (p.ks * p.ks);
    const int split = b;
    const int kh = tap / p.ks, kw = tap % p.ks;
    const int co0 = co_t * T, ci0 = ci_t * T;
    const int pix_lo = split * p.chunk, pix_hi = min(p.M, pix_lo + p.chunk);

    // staging bookkeeping: lane -> (pixel within piece, chunk slot)
    const int lp = lane / CHUNKS, lc = lane % CHUNKS;
    int a_off[PPW], b_img[PPW], b_ho[PPW], b_wo[PPW], s_pix[PPW];
#pragma unroll
    for (int j = 0; j < PPW; j++) {
        const int piece = wave * PPW + j;
        const int tp = piece * PIX_PER_PIECE + lp;       // tile-local pixel
        s_pix[j] = tp;
        const int pg = pix_lo + tp;
        const int chunk = lc ^ (wg_swz<T>(tp) << 1);       // logical chunk stored at slot lc
        a_off[j] = (int)(((long long)pg * p.dz_cs + co0 + chunk * 8) * 2);
        b_wo[j] = pg % p.Wo;
        const int t = pg / p.Wo;
        b_ho[j] = t % p.Ho;
        b_img[j] = t / p.Ho;
    }
    const bool piece_active = (wave * PPW) < PIECES;

    auto stage = [&](int kt, int buf) {
        char *abuf = smem + buf * 2 * TILE_B;
        char *bbuf = abuf + TILE_B;
#pragma unroll
        for (int j = 0; j < PPW; j++) {
            if (!piece_active) continue;
            const int piece = wave * PPW + j;
            const int pg = pix_lo + kt * KP + s_pix[j];
            const int chunk = lc ^ (wg_swz<T>(s_pix[j]) << 1);
            const bool in_rng = pg < pix_hi;
            // A: dz row (contiguous pixel order)
            const bool a_ok = in_rng && (co0 + chunk * 8 < p.Cout);
            const int a_v = a_ok ? a_off[j] + kt * KP * p.dz_cs * 2 : (int)0x80000000;
            buffer_load_lds16(p.dz, p.dz_bytes, abuf + piece * 1024, a_v, 0);
            // B: x row of the tap-shifted pixel
            const int hi = b_ho[j] * p.stride - p.pad + kh, wi = b_wo[j] * p.stride - p.pad + kw;
            const bool b_ok = in_rng && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W &&
                              (ci0 + chunk * 8 < p.Cin);
            const int b_v = b_ok ? (int)((((long long)(b_img[j] * p.H + hi) * p.W + wi) * p.x_cs + ci0 + chunk * 8) * 2)
                                 : (int)0x80000000;
            buffer_load_lds16(p.x, p.x_bytes, bbuf + piece * 1024, b_v, 0);
            // advance this lane's pixel by KP for the next call
            b_wo[j] += KP;
            while (b_wo[j] >= p.Wo) {
                b_wo[j] -= p.Wo;
                if (++b_ho[j] == p.Ho) { b_ho[j] = 0; b_img[j]++; }
            }
        }
    };

    // transpose-read addressing: in k-group kg, lane fr addresses pixel row kg*8 + (fr>>2) (+4 for the second read,
    // +32 for the second k-substep) and the 8 bytes of channels 4*(fr&3).. of the fragment's 16-channel pair
    const int wr = wave >> 1, wc = wave & 1;
    const int fr = lane & 15, kg = lane >> 4;
    const int trow = kg * 8 + (fr >> 2);
    const int tsw = wg_swz<T>(trow);
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
        __syncthreads();
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
    // D[row = co (kg*4 + r)][col = ci (fr)]  ->  part[split][co][tap*Cin + ci]
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

// ------------------------------------------------------------------------------------------------ wgrad, wide tile
// The T x T kernel above is LDS-bound by construction: a 64 x 64 wave tile pulls 16 transposed fragments (8 KiB) per 16
// MFMAs, i.e. the CU's whole 128 B/clk LDS port at MFMA peak, before the direct-to-LDS fills are counted (bound: 58 % of
// peak at T = 128; measured 24-30 % on the 128->256 / 256->512 / 512->1024 layers).  Here the workgroup tile is
// TM x TN = 256 (c_out) x 128 (c_in), 4 waves as 2 x 2 with a 128 x 64 wave tile: 12 fragments per 32 MFMAs (-25 % LDS
// reads per MFMA; bound 80 %).  K step = 32 pixels, three stages in LDS (72 KiB, two workgroups per CU), the fills of step
// k+2 are issued under the MFMAs of step k and retired with a COUNTED s_waitcnt (each wave issues exactly NLD
// direct-to-LDS loads per step, out-of-range ones with the buffer's out-of-bounds offset), one barrier per step.
// ABL: timing-only ablations, instantiated in the ablation build only (tools/wgrad_ablate.py; wrong results on purpose): bit 0 no
// partial-tile stores, 1 fragments read from LDS in the first K step only, 2 no direct-to-LDS fills inside the loop
// Fill addresses (round 6): the dz operand goes through a buffer descriptor that SLIDES (base += one step, num_records -= one step: three
// scalar instructions per step; the lanes' offsets are constants and the split's end is the descriptor's bound), the x operand from per-lane
// running (h_in, w_in, byte offset) advanced with adds and selects only.  Rounds 2-5 derived both from the pixel index per piece and step
// (64-bit multiply-adds, 32-bit multiplies, a per-lane wrap loop): 75 VALU + 50 SALU instructions per step in front of the fills they feed,
// 2.2 VALU per MFMA (profiles/r06_pmc_wgrad.txt); isolated launches went 985 -> 1100 TF/s (3x3 128->256 @76^2), 1107 -> 1209 (256->512
// @38^2), bit-identical partial tiles (profiles/r06_wgrad_addr_ab.txt).
// NW = 8 (round 6, MEASUREMENT BUILD ONLY): the same workgroup tile on EIGHT waves as 4 x 2 with 64 x 64 wave tiles (122 registers, two
// workgroups = four waves per SIMD).  Same MFMAs on the same operands in the same K order: bit-identical partial tiles.  The 3x3 launches do
// not care (-1 ... +5 %: at 1100-1250 TF/s they sit at the chip's power-limited MFMA rate either way); the 1x1 launches -- short K loops, one
// workgroup per CU by their split target -- gain 7-14 % as ISOLATED launches and LOSE 0.15-0.25 ms per step inside the step (three A/B blocks
// in both engine orders, profiles/r06_wgrad_nw8.txt): not dispatched.  ryolo_debug_wgrad_set(8) selects it for every 256 x 128 launch.
// (A 256 x 256 tile on eight 64 x 128 waves, one workgroup per CU, a third fewer fill bytes per flop: 17 % SLOWER on 3x3 256->512 @38^2 --
//  the two waves of a SIMD share one barrier and fall into lock step; measurement build only, ryolo_debug_wgrad_set(9).)
// NT = 3 (round 6, the 3x3 layers with C_in = 64): the N dimension of the workgroup's GEMM is THREE TAPS x 64 input channels -- the taps
// kw = 0, 1, 2 of one filter row share the staged dz rows (the A operand); the B operand is three [32 pixels][64 channels] images, one per
// tap, each filled from its own tap-shifted pixels.  A 128 x 64 tile moved 12 KiB of fills and 6 fragment reads per 8 MFMAs of a wave
// (twice the big tile's bytes per flop: 313 us = 0.28 of peak for the 218 GFLOP of 64->128 @152^2); three taps per workgroup: 20 KiB and 10
// fragment reads per 24 MFMAs, the 256 x 128 tile's ratios.  The partial tile layout ([split][c_out][tap * C_in + c_in]) does not change:
// the N index of an accumulator column IS (tap - tap0) * 64 + c_in.
template <int TM, int TN, int ABL = 0, int NW = 4, int NT = 1>
__global__ void __launch_bounds__(NW * 64, NW == 8 ? (TM * TN > 256 * 128 ? 2 : 4) : 1) wgrad_wide_kernel(const WgradParams p) {
    constexpr int KPX = 32, NST = 3;
    constexpr int WM = TM / (NW / 2), WN = NT * TN / 2, NFA = WM / 16, NFB = WN / 16;
    constexpr int ROW_A = TM * 2, ROW_B = TN * 2;                  // bytes per staged pixel row
    constexpr int TILE_A = KPX * ROW_A, TILE_B = KPX * ROW_B, STAGE = TILE_A + NT * TILE_B;
    constexpr int CH_A = TM / 8, CH_B = TN / 8;                    // 16-B chunks per row
    constexpr int PPP_A = 64 / CH_A, PPP_B = 64 / CH_B;            // pixels per 1-KiB piece
    constexpr int PPW_A = TILE_A / 1024 / NW, PPW_B = NT * TILE_B / 1024 / NW;   // pieces per wave
    constexpr int PPT_B = TILE_B / 1024;                           // pieces per tap image
    constexpr int NLD = PPW_A + PPW_B;
    static_assert(TM >= 64 && TN >= 64 && CH_A <= 64 && TILE_A % (1024 * NW) == 0 && (NT * TILE_B) % (1024 * NW) == 0, "tile shape");
    static_assert(NT == 1 || (NT * TN) % 32 == 0, "whole fragments per wave column");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [NST][A tile | B tile]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // workgroups are dealt to the 8 XCDs round-robin; give each XCD a CONTIGUOUS range of logical ids so the taps / channel
    // tiles of one pixel split (which stream the same dz and x rows) share one L2 instead of fetching them 8 times
    int b = blockIdx.x;
    {
        const int per = gridDim.x >> 3;
        if (b < per * 8) b = (b & 7) * per + (b >> 3);
    }
    const int ci_t = b % p.ci_tiles; b /= p.ci_tiles;
    const int co_t = b % p.co_tiles; b /= p.co_tiles;
    const int ntg = (p.ks * p.ks) / NT;                // tap groups (NT = 3: the filter rows)
    const int tap = (b % ntg) * NT; b /= ntg;          // first tap of this workgroup
    const int split = b;
    const int kh = tap / p.ks, kw = tap % p.ks;
    const int co0 = co_t * TM, ci0 = ci_t * TN;
    const int pix_lo = split * p.chunk, pix_hi = min(p.M, pix_lo + p.chunk);

    // staging bookkeeping: A piece j of this wave covers tile pixels (wave*PPW_A + j)*PPP_A + lane / CH_A
    int a_pix[PPW_A], a_col[PPW_A];
#pragma unroll
    for (int j = 0; j < PPW_A; j++) {
        const int tp = (wave * PPW_A + j) * PPP_A + lane / CH_A;
        a_pix[j] = tp;
        a_col[j] = (co0 + (((lane % CH_A) ^ (wg_swz<TM>(tp) << 1)) * 8)) * 2;
    }
    // B piece j of this wave: piece (wave*PPW_B + j) % PPT_B of tap image (wave*PPW_B + j) / PPT_B (wave-uniform)
    int b_pix[PPW_B], b_col[PPW_B], b_kw[PPW_B];
#pragma unroll
    for (int j = 0; j < PPW_B; j++) {
        const int q = wave * PPW_B + j;
        const int tp = (NT == 1 ? q : q % PPT_B) * PPP_B + lane / CH_B;
        b_pix[j] = tp;
        b_kw[j] = kw + (NT == 1 ? 0 : q / PPT_B);
        b_col[j] = (ci0 + (((lane % CH_B) ^ (wg_swz<TN>(tp) << 1)) * 8)) * 2;
    }

    const i32x4 rs_x = make_rsrc_words(p.x, p.x_bytes);
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem;
    // dz: descriptor of the split's rows [pix_lo, pix_hi), advanced by one step per stage() call (scalar registers)
    const unsigned a_step = (unsigned)(KPX * p.dz_cs * 2);
    unsigned long long a_base = (unsigned long long)p.dz + (unsigned long long)pix_lo * (unsigned long long)(p.dz_cs * 2);
    unsigned a_rec = (unsigned)((pix_hi - pix_lo) * p.dz_cs * 2);         // (< 2^31: the launcher checks the tensor's extent)
    int a_vo[PPW_A];
#pragma unroll
    for (int j = 0; j < PPW_A; j++) a_vo[j] = a_pix[j] * p.dz_cs * 2 + a_col[j];
    // x: per lane h_in / w_in of the tap-shifted input pixel and its byte offset (+ column); advanced by KPX output pixels per call
    const int x_cs2 = p.x_cs * 2;
    const int b_dw = KPX * p.stride, b_doff = KPX * p.stride * x_cs2;
    const int wi_wrap0 = p.Wo * p.stride - p.pad, hi_top = p.Ho * p.stride - p.pad + kh;
    const int b_wos = p.Wo * p.stride, b_hos = p.Ho * p.stride;
    const int b_rowjump = (p.stride * p.W - p.Wo * p.stride) * x_cs2, b_imgjump = (p.H - p.Ho * p.stride) * p.W * x_cs2;
    int b_rem = pix_hi - pix_lo;                                          // pixels of the split not yet staged (scalar)
    int b_hi[PPW_B], b_wi[PPW_B], b_off[PPW_B];
#pragma unroll
    for (int j = 0; j < PPW_B; j++) {
        const int pg = pix_lo + b_pix[j];
        const int wo = pg % p.Wo, t = pg / p.Wo;
        b_hi[j] = (t % p.Ho) * p.stride - p.pad + kh;
        b_wi[j] = wo * p.stride - p.pad + b_kw[j];
        b_off[j] = (int)(((long long)((t / p.Ho) * p.H + b_hi[j]) * p.W + b_wi[j]) * x_cs2) + b_col[j];
    }
    auto stage_a = [&](int buf, int j) __attribute__((always_inline)) {
        i32x4 r;
        r[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)a_base);
        r[1] = __builtin_amdgcn_readfirstlane((int)(unsigned)(a_base >> 32));
        r[2] = __builtin_amdgcn_readfirstlane((int)a_rec);
        r[3] = 0x00020000;
        buffer_load_lds16_raw(r, lds0 + buf * STAGE + (wave * PPW_A + j) * 1024, a_vo[j]);      // rows past the split's end: outside the descriptor
    };
    auto stage_b = [&](int buf, int j) __attribute__((always_inline)) {
        const bool ok = b_pix[j] < b_rem && (unsigned)b_hi[j] < (unsigned)p.H && (unsigned)b_wi[j] < (unsigned)p.W;
        buffer_load_lds16_raw(rs_x, lds0 + buf * STAGE + TILE_A + (wave * PPW_B + j) * 1024, ok ? b_off[j] : (int)0x80000000);
        b_wi[j] += b_dw;                                       // this lane's pixel of the next step
        b_off[j] += b_doff;
        const int wi_wrap = wi_wrap0 + b_kw[j];
        auto wrap = [&]() __attribute__((always_inline)) {
            const bool w = b_wi[j] >= wi_wrap;                 // past the row's end: next output row
            b_wi[j] -= w ? b_wos : 0;
            b_off[j] += w ? b_rowjump : 0;
            b_hi[j] += w ? p.stride : 0;
            const bool t = b_hi[j] >= hi_top;                  // past the image's last row: next image
            b_hi[j] -= t ? b_hos : 0;
            b_off[j] += t ? b_imgjump : 0;
        };
        wrap();
        if (p.Wo < KPX) wrap();                                // (wave-uniform) rows shorter than a step: a second wrap covers W_o >= 16
        if (p.Wo < KPX / 2)
            while (b_wi[j] >= wi_wrap) wrap();
    };
    auto stage = [&](int buf) __attribute__((always_inline)) {   // the next K step (calls are in step order): exactly NLD loads per wave, in or out of range
#pragma unroll
        for (int j = 0; j < PPW_A; j++) stage_a(buf, j);
#pragma unroll
        for (int j = 0; j < PPW_B; j++) stage_b(buf, j);
        a_base += a_step;
        a_rec = a_rec > a_step ? a_rec - a_step : 0u;
        b_rem -= KPX;
    };

    const int wr = wave >> 1, wc = wave & 1;
    const int fr = lane & 15, kg = lane >> 4;
    const int trow = kg * 8 + (fr >> 2);
    const int tswa = wg_swz<TM>(trow), tswb = wg_swz<TN>(trow);     // each operand's rows are swizzled for its own row length
    int offa[NFA], offb[NFB];
#pragma unroll
    for (int f = 0; f < NFA; f++) offa[f] = trow * ROW_A + (fr & 3) * 8 + ((((wr * WM) >> 4) + f) ^ tswa) * 32;
#pragma unroll
    for (int f = 0; f < NFB; f++) {
        const int gf = ((wc * WN) >> 4) + f;                   // 16-channel fragment of the N extent: tap image gf / (TN / 16), fragment gf % (TN / 16)
        offb[f] = TILE_A + (NT == 1 ? 0 : gf / (TN / 16)) * TILE_B + trow * ROW_B + (fr & 3) * 8 + (((NT == 1 ? gf : gf % (TN / 16))) ^ tswb) * 32;
    }

    f32x4 acc[NFA][NFB];
#pragma unroll
    for (int a = 0; a < NFA; a++)
#pragma unroll
        for (int c = 0; c < NFB; c++) acc[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nsteps = (pix_hi - pix_lo + KPX - 1) / KPX;
    stage(0);
    stage(1);
    int cur = 0, nxt = 2;
    bf16x8 af[NFA], bfr[NFB];
    for (int kt = 0; kt < nsteps; kt++) {
        // stage kt has landed when only the NLD loads of stage kt+1 are still in flight; the barrier also says every wave
        // is done reading the buffer of step kt-1, which stage kt+2 now overwrites
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD) : "memory");
        __builtin_amdgcn_s_barrier();
        if (!(ABL & 4)) stage(nxt);
        const char *base = smem + cur * STAGE;
        if (!(ABL & 2) || kt == 0) {
#pragma unroll
        for (int f = 0; f < NFB; f++) {
            const s16x4 b0 = lds_read_tr16(base + offb[f]);
            const s16x4 b1 = lds_read_tr16(base + offb[f] + 4 * ROW_B);
            bfr[f] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7));
        }
#pragma unroll
        for (int f = 0; f < NFA; f++) {
            const s16x4 a0 = lds_read_tr16(base + offa[f]);
            const s16x4 a1 = lds_read_tr16(base + offa[f] + 4 * ROW_A);
            af[f] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7));
        }
        }
        // s_setprio around the MFMA block: +1.5 ... 5 % on the 3x3 layers (profiles/r06_wgrad_setprio.txt).  The opposite assignment (priority
        // on the fills and reads) measures the same, so what helps is the fence the instruction puts between the two phases for the
        // compiler's scheduler, not the arbitration between the two resident waves.
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int a = 0; a < NFA; a++)
#pragma unroll
            for (int c = 0; c < NFB; c++)
                acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bfr[c], acc[a][c], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        cur = cur == NST - 1 ? 0 : cur + 1;
        nxt = nxt == NST - 1 ? 0 : nxt + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // drain the look-ahead fills before the workgroup can retire
    float *out = p.part + (size_t)split * p.Cout_pad * p.Kpad;
    if (ABL & 1) {         // no stores: keep the accumulators live through one value nobody produces
        float t = 0.f;
#pragma unroll
        for (int a = 0; a < NFA; a++)
#pragma unroll
            for (int c = 0; c < NFB; c++) t += acc[a][c][0] + acc[a][c][1] + acc[a][c][2] + acc[a][c][3];
        if (t == 1234.5678f) out[0] = t;
        return;
    }
#pragma unroll
    for (int a = 0; a < NFA; a++)
#pragma unroll
        for (int c = 0; c < NFB; c++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int co = co0 + wr * WM + a * 16 + kg * 4 + r;
                const int nn = wc * WN + c * 16 + fr;                        // column of the N extent: tap image nn / TN, channel nn % TN
                const int ci = ci0 + (NT == 1 ? nn : nn % TN);
                if (co < p.Cout && ci < p.Cin) out[(size_t)co * p.Kpad + (tap + (NT == 1 ? 0 : nn / TN)) * p.Cin + ci] = acc[a][c][r];
            }
}

// ------------------------------------------------------------------------------------------------ wgrad, few channels
// The stem layers (C_in, C_out <= 64 at 304^2 / 608^2) under the kernel above re-read dz and x once per filter tap and
// per channel tile -- 9-18x through L2, which is their bound.  Here ONE workgroup owns ALL taps and channels of its pixel
// range: per K step (64 consecutive output pixels of one image row) it stages the dz rows once and the KS input rows
// they touch once (with the (KS-1)-pixel halo), and every tap's B fragment is read from that halo tile at a per-lane
// shifted address (the transpose read takes one address per lane, so a tap shift or a stride-2 walk is free).
// GEMM: M = C_out (MF fragments, every wave), N = taps x C_in in 16-wide fragments dealt round-robin to the 4 waves,
// K = pixels.  Same split-K partial layout as wgrad_kernel ([split][co][tap*C_in + ci]) -> same reduce kernel.
struct WgradTapsParams {
    const __bf16 *x, *dz;
    float *part;
    int N, H, W, x_cs, Ho, Wo, dz_cs, pad;
    int Cout, Kpad;
    int nseg, nsteps, steps_per_split;
    unsigned x_bytes, dz_bytes;
};

template <int CO, int CI, int KS, int ST>
__global__ void __launch_bounds__(256) wgrad_taps_kernel(const WgradTapsParams p) {
    constexpr int A_ROWB = CO * 2, A_TILE = KP * A_ROWB, A_PIECES = A_TILE / 1024;
    constexpr int QP = (KP - 1) * ST + KS;                   // input pixels one halo row needs
    constexpr int B_ROWB = CI * 2;
    constexpr int PPR = (QP * B_ROWB + 1023) / 1024;         // 1-KiB pieces per halo row
    constexpr int QPP = PPR * 1024 / B_ROWB;                 // halo row pitch in pixels
    constexpr int B_TILE = KS * PPR * 1024, B_PIECES = KS * PPR;
    constexpr int STAGE = A_TILE + B_TILE, PIECES = A_PIECES + B_PIECES, PPW = (PIECES + 3) / 4;
    constexpr int NREAL = KS * KS * CI;                      // real N (taps x channels); the last fragment may be ragged
    constexpr int MF = CO / 16, NFR = (NREAL + 15) / 16, NJ = (NFR + 3) / 4;
    constexpr int A_CPR = A_ROWB / 16, B_CPR = B_ROWB / 16;  // 16-B chunks per staged pixel
    static_assert(CO % 16 == 0 && (CI == 8 || CI % 16 == 0), "fragment-aligned channel counts");
    static_assert(CI != 8 || QPP > QP, "C_in = 8 needs a padding pixel (always zero) in the halo row");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = blockIdx.x;
    const int s_lo = split * p.steps_per_split, s_hi = min(p.nsteps, s_lo + p.steps_per_split);

    auto stage = [&](int s, int buf) {
        const int seg = s % p.nseg, t = s / p.nseg;
        const int ho = t % p.Ho, img = t / p.Ho;
        const int wo0 = seg * KP;
        char *base = smem + buf * STAGE;
#pragma unroll
        for (int u = 0; u < PPW; u++) {
            const int pi = wave + 4 * u;
            if (pi >= PIECES) continue;
            if (pi < A_PIECES) {
                const int pix = pi * (1024 / A_ROWB) + lane / A_CPR;
                const int chunk = (lane % A_CPR) ^ (wg_swz<CO>(pix) << 1);
                const bool ok = (wo0 + pix < p.Wo) && (chunk * 8 < p.Cout);
                const int off = (int)((((long long)(img * p.Ho + ho) * p.Wo + wo0 + pix) * p.dz_cs + chunk * 8) * 2);
                buffer_load_lds16(p.dz, p.dz_bytes, base + pi * 1024, ok ? off : (int)0x80000000, 0);
            } else {
                const int bi = pi - A_PIECES;
                const int kh = bi / PPR, r = bi % PPR;
                const int q = r * (1024 / B_ROWB) + lane / B_CPR;
                const int chunk = B_CPR > 1 ? ((lane % B_CPR) ^ (wg_swz<CI>(q) << 1)) : 0;
                const int hi = ho * ST - p.pad + kh, wi = wo0 * ST - p.pad + q;
                const bool ok = q < QP && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
                const int off = (int)((((long long)(img * p.H + hi) * p.W + wi) * p.x_cs + chunk * 8) * 2);
                buffer_load_lds16(p.x, p.x_bytes, base + A_TILE + bi * 1024, ok ? off : (int)0x80000000, 0);
            }
        }
    };

    // fragment addresses (bytes inside a stage): k-group kg, lane fr -> pixel kg*8 + (fr>>2) (+4: second read, +32: second
    // k-substep), 8 bytes = channels 4*(fr&3).. of the fragment's 16-channel pair
    const int fr = lane & 15, kg = lane >> 4;
    int a_addr[MF];
    {
        const int pix = kg * 8 + (fr >> 2);
        const int sw = wg_swz<CO>(pix);
#pragma unroll
        for (int m = 0; m < MF; m++) a_addr[m] = pix * A_ROWB + ((m ^ sw) << 5) + (fr & 3) * 8;
    }
    int b_addr[NJ][2][2];
#pragma unroll
    for (int jj = 0; jj < NJ; jj++) {
        const int j = wave + 4 * jj;
        if constexpr (CI == 8) {
            // 16 N columns = two taps x 8 channels: the lane's 4 channels sit in tap (n0 >> 3); a tap index past the window
            // (ragged last fragment) reads the halo row's padding pixel, which is always zero
            const int n0 = j * 16 + (fr & 3) * 4;
            const int tap = n0 >> 3, cio = n0 & 7;
            const bool real = tap < KS * KS;
            const int kh = real ? tap / KS : 0, kw = real ? tap % KS : 0;
#pragma unroll
            for (int ks = 0; ks < 2; ks++)
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int k = ks * 32 + kg * 8 + (fr >> 2) + 4 * h;
                    const int q = real ? k * ST + kw : QPP - 1;
                    b_addr[jj][ks][h] = A_TILE + (kh * QPP + q) * B_ROWB + cio * 2;
                }
        } else {
            const int tap = (j * 16) / CI, pr = ((j * 16) % CI) / 16;
            const int kh = tap / KS, kw = tap % KS;
#pragma unroll
            for (int ks = 0; ks < 2; ks++)
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int k = ks * 32 + kg * 8 + (fr >> 2) + 4 * h;
                    const int q = k * ST + kw;
                    b_addr[jj][ks][h] = A_TILE + (kh * QPP + q) * B_ROWB + ((pr ^ wg_swz<CI>(q)) << 5) + (fr & 3) * 8;
                }
        }
    }

    f32x4 acc[MF][NJ];
#pragma unroll
    for (int m = 0; m < MF; m++)
#pragma unroll
        for (int jj = 0; jj < NJ; jj++) acc[m][jj] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nst = s_hi - s_lo;
    if (nst > 0) stage(s_lo, 0);
    for (int it = 0; it < nst; it++) {
        __syncthreads();
        if (it + 1 < nst) stage(s_lo + it + 1, (it + 1) & 1);
        const char *sb = smem + (it & 1) * STAGE;
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            bf16x8 af[MF];
#pragma unroll
            for (int m = 0; m < MF; m++) {
                const s16x4 a0 = lds_read_tr16(sb + a_addr[m] + (ks * 32) * A_ROWB);
                const s16x4 a1 = lds_read_tr16(sb + a_addr[m] + (ks * 32 + 4) * A_ROWB);
                af[m] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7));
            }
#pragma unroll
            for (int jj = 0; jj < NJ; jj++) {
                if (wave + 4 * jj >= NFR) continue;
                const s16x4 b0 = lds_read_tr16(sb + b_addr[jj][ks][0]);
                const s16x4 b1 = lds_read_tr16(sb + b_addr[jj][ks][1]);
                const bf16x8 bfr = __builtin_bit_cast(bf16x8, __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
                for (int m = 0; m < MF; m++)
                    acc[m][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[m], bfr, acc[m][jj], 0, 0, 0);
            }
        }
    }
    // D[row = co (kg*4 + r)][col = n (fr)] -> part[split][co][n],  n = tap*CI + ci
    float *out = p.part + (size_t)split * CO * p.Kpad;
#pragma unroll
    for (int m = 0; m < MF; m++)
#pragma unroll
        for (int jj = 0; jj < NJ; jj++) {
            const int j = wave + 4 * jj;
            if (j >= NFR) continue;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int co = m * 16 + kg * 4 + r;
                if (co < p.Cout && j * 16 + fr < NREAL) out[(size_t)co * p.Kpad + j * 16 + fr] = acc[m][jj][r];
            }
        }
}

// sum the S partial tiles and accumulate into the OIHW fp32 gradient: g[co][ci][kh][kw] += sum_s part[s][co][tap*Cin_k + ci].
// Threads walk the SOURCE order (co, tap, ci): the S reads are coalesced, the one read-modify-write of g is strided.
// The pass is latency-bound on the layers with many splits and few weights (3x3 128 -> 256: 295 k elements x 56 splits -- one
// thread per element walked its 56 loads four at a time, 14 round trips with 18 waves per CU: 2.1 TB/s over the step).  Q = 4: the
// four waves of a workgroup take a quarter of the splits each for the same 64 elements (8 loads in flight per thread) and the
// quarters are added in a fixed order through LDS; Q = 1 (few splits): one element per thread as before.
// (the body is shared with wgrad_reduce_batch_kernel: `bid` / `nblk` = this launch's or this job's block index / block count; the order in
// which an element's S partial values are added depends on S and Q only, so both launch forms give the same bits)
template <int Q>
__device__ __forceinline__ void wgrad_reduce_body(float *sm, unsigned bid, unsigned nblk, const float *__restrict__ part, int S, int Cout, int Cin,
                                                  int Cin_k, int ks, int Kpad, int Cout_pad, float *__restrict__ g, int accumulate) {
    constexpr int EPB = 256 / Q;
    const int taps = ks * ks;
    const unsigned per_co = (unsigned)(taps * Cin);
    const unsigned total = (unsigned)Cout * per_co;
    const size_t sstride = (size_t)Cout_pad * Kpad;
    const int e = threadIdx.x % EPB, q = threadIdx.x / EPB;
    const int per = (S + Q - 1) / Q;
    const int s_lo = q * per, s_hi = min(S, s_lo + per);
    for (unsigned base = bid * EPB; base < total; base += nblk * EPB) {      // (workgroup-uniform trip count)
        const unsigned i = base + e;
        const bool ok = i < total;
        const unsigned co = ok ? i / per_co : 0, rem = ok ? i - co * per_co : 0;
        const unsigned tap = rem / (unsigned)Cin, ci = rem - tap * (unsigned)Cin;
        const float *src = part + (size_t)co * Kpad + tap * Cin_k + ci;
        float v = 0.f;
        if (ok) {
            int s = s_lo;
            for (; s + 8 <= s_hi; s += 8) {      // independent loads in flight
                float a[8];
#pragma unroll
                for (int u = 0; u < 8; u++) a[u] = src[(size_t)(s + u) * sstride];
                v += ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
            }
            for (; s + 4 <= s_hi; s += 4) {
                const float a0 = src[(size_t)s * sstride], a1 = src[(size_t)(s + 1) * sstride];
                const float a2 = src[(size_t)(s + 2) * sstride], a3 = src[(size_t)(s + 3) * sstride];
                v += (a0 + a1) + (a2 + a3);
            }
            for (; s < s_hi; s++) v += src[(size_t)s * sstride];
        }
        if constexpr (Q > 1) {
            sm[threadIdx.x] = v;
            __syncthreads();
            if (q == 0) {
                static_assert(Q == 1 || Q == 4, "fixed combine order below");
                v = (sm[e] + sm[EPB + e]) + (sm[2 * EPB + e] + sm[3 * EPB + e]);
            }
        }
        if (ok && q == 0) {
            const size_t dst = ((size_t)co * Cin + ci) * taps + tap;
            g[dst] = accumulate ? g[dst] + v : v;
        }
        if constexpr (Q > 1) __syncthreads();
    }
}
template <int Q>
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float *__restrict__ part, int S, int Cout, int Cin, int Cin_k, int ks, int Kpad,
                                                           int Cout_pad, float *__restrict__ g, int accumulate) {
    __shared__ float sm[Q > 1 ? 256 : 1];
    wgrad_reduce_body<Q>(sm, blockIdx.x, gridDim.x, part, S, Cout, Cin, Cin_k, ks, Kpad, Cout_pad, g, accumulate);
}

// The same reduce for the 3x3 layers with few splits and many weights (512 -> 1024: 4.7 M elements, S = 3): there the strided
// read-modify-write of g is what costs (a wave's 64 floats land 36 B apart: 18 cache lines per 256 B).  A workgroup takes one c_out and
// 64 input channels -- nine 256-B runs in the source, ONE contiguous run of 576 floats in g -- sums the splits in source order and
// transposes (tap, ci) -> (ci, tap) through LDS, so both sides are coalesced.  Same per-element summation order as Q = 1 above.
__device__ __forceinline__ void wgrad_reduce_t3_body(float *sm, unsigned bid, const float *__restrict__ part, int S, int Cin, int Cin_k, int Kpad,
                                                     int Cout_pad, float *__restrict__ g, int accumulate) {
    const int cib = Cin / 64;
    const int co = bid / cib, c0 = (bid % cib) * 64;
    const size_t sstride = (size_t)Cout_pad * Kpad;
    for (int idx = threadIdx.x; idx < 576; idx += 256) {
        const int tap = idx >> 6, cl = idx & 63;
        const float *src = part + (size_t)co * Kpad + tap * Cin_k + c0 + cl;
        float v = 0.f;
        int s = 0;
        for (; s + 4 <= S; s += 4) {
            const float a0 = src[(size_t)s * sstride], a1 = src[(size_t)(s + 1) * sstride];
            const float a2 = src[(size_t)(s + 2) * sstride], a3 = src[(size_t)(s + 3) * sstride];
            v += (a0 + a1) + (a2 + a3);
        }
        for (; s < S; s++) v += src[(size_t)s * sstride];
        sm[tap * 65 + cl] = v;
    }
    __syncthreads();
    float *dst = g + ((size_t)co * Cin + c0) * 9;
    for (int j = threadIdx.x; j < 576; j += 256) {
        const int cl = j / 9, tap = j - cl * 9;
        const float v = sm[tap * 65 + cl];
        dst[j] = accumulate ? dst[j] + v : v;
    }
}
__global__ void __launch_bounds__(256) wgrad_reduce_t3_kernel(const float *__restrict__ part, int S, int Cin, int Cin_k, int Kpad, int Cout_pad,
                                                              float *__restrict__ g, int accumulate) {
    __shared__ float sm[9 * 65];
    wgrad_reduce_t3_body(sm, blockIdx.x, part, S, Cin, Cin_k, Kpad, Cout_pad, g, accumulate);
}

// The four-quarter reduce for the batched launch (job kind 3; C_in % 4 == 0): in a launch that streams 3.7 GB the per-layer body above is
// bound by its dependent round trips (8 four-byte loads in flight per thread, then the next batch, then LDS, then the gradient: 1.08 ms per
// step = 3.4 TB/s, profiles/r05_train_kernel_stats.txt).  Here a thread takes FOUR consecutive input channels (16-B loads) and has all the
// loads of its split quarter in flight at once (<= 16 per pass: 16 KB per wave).  The order in which an element's partial values are added
// is the body's above -- quarters of ceil(S / 4) splits, inside a quarter groups of 8 as ((a0+a1)+(a2+a3))+((a4+a5)+(a6+a7)), then one
// group of 4, then single values, the quarters as (q0+q1)+(q2+q3) -- so the bits are the same (tests/test_train_ops_gpu.py).
typedef __attribute__((address_space(1))) float *glb_f32;      // (the job's pointers come out of a table: say "global", not flat)
__device__ __forceinline__ f32x4 f4_tree4(const f32x4 *a) { return (a[0] + a[1]) + (a[2] + a[3]); }
__device__ __forceinline__ f32x4 f4_tree8(const f32x4 *a) { return f4_tree4(a) + f4_tree4(a + 4); }
template <int K0>
__device__ __forceinline__ f32x4 f4_singles(f32x4 v, const f32x4 *a, int n) {
    if (n > 0) v = v + a[K0];
    if (n > 1) v = v + a[K0 + 1];
    if (n > 2) v = v + a[K0 + 2];
    return v;
}
// one pass over P splits of the quarter starting at split `s` (P in {4, 8, 16}; r = splits left, > 0): the P loads are issued back to back --
// the ones past the quarter's end go out of the descriptor's range (no memory request, the repository's 0x80000000 idiom) -- and only then
// the (wave-uniform) case analysis on r picks the additions.
template <int P>
__device__ __forceinline__ void wgrad_reduce_v4_load(f32x4 *a, __amdgpu_buffer_rsrc_t rs, unsigned off, unsigned step, int r) {
#pragma unroll
    for (int u = 0; u < P; u++)
        a[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, u < r ? (int)(off + (unsigned)u * step) : (int)0x80000000, 0, 0));
}
template <int P>
__device__ __forceinline__ f32x4 wgrad_reduce_v4_sum(f32x4 v, const f32x4 *a, int r) {
    if constexpr (P == 16) {
        if (r >= 16) {
            v = v + f4_tree8(a);
            return v + f4_tree8(a + 8);
        }
    }
    if constexpr (P >= 8) {
        if (r >= 8) {               // (P == 8: r == 8 or, with more passes to come, more; P == 16: 8 .. 15)
            v = v + f4_tree8(a);
            if constexpr (P == 16) {
                if (r & 4) {
                    v = v + f4_tree4(a + 8);
                    return f4_singles<12>(v, a, r & 3);
                }
                return f4_singles<8>(v, a, r & 3);
            }
            return v;
        }
    }
    if (r >= 4) {                   // (P == 4: r >= 4 means a full group)
        v = v + f4_tree4(a);
        if constexpr (P >= 8) return f4_singles<4>(v, a, r & 3);
        return v;
    }
    return f4_singles<0>(v, a, r);
}
// A workgroup pass covers 256 * G consecutive elements: G groups of four channels per thread.  P = 16, G = 1 covers any quarter length in
// passes of 16 splits; P = 8 / 4 (quarters of AT MOST 8 / 4 splits: one pass, so the groups of additions are the per-layer body's) take
// G = 2 / 4 groups so that a thread still has 16 loads in flight and a workgroup >= 16 KB per trip -- a workgroup's trip is a chain of
// ~6 us of latencies (job lookup, the loads, LDS, the gradient's read-modify-write), and with 14 KB per trip the 3x3 256 -> 512 layers
// (S = 14) streamed at 3 TB/s.  Wave q' adds the quarters of group q' and writes its gradient values.
template <int P, int G>
__device__ __forceinline__ void wgrad_reduce_v4_loop(f32x4 *sm4, unsigned bid, unsigned nblk, __amdgpu_buffer_rsrc_t rs, unsigned step, int n, int q, int e,
                                                     unsigned total, unsigned per_co, int Cin, int Cin_k, int Kpad, int taps, glb_f32 g, int accumulate) {
    static_assert(G == 1 || P * G == 16, "16 loads in flight per thread");
    for (unsigned base = bid * (256u * G); base < total; base += nblk * (256u * G)) {      // (workgroup-uniform trip count)
        unsigned voff[G];
#pragma unroll
        for (int gi = 0; gi < G; gi++) {
            const unsigned i = base + (unsigned)(gi * 64 + e) * 4u;
            const bool ok = i < total;
            const unsigned co = ok ? i / per_co : 0, rem = ok ? i - co * per_co : 0;
            const unsigned tap = rem / (unsigned)Cin, ci = rem - tap * (unsigned)Cin;
            voff[gi] = ok ? (co * (unsigned)Kpad + tap * (unsigned)Cin_k + ci) * 4u : 0x80000000u;
        }
        f32x4 v[G];
#pragma unroll
        for (int gi = 0; gi < G; gi++) v[gi] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (G == 1) {
            for (int s = 0; s < n; s += P) {
                f32x4 a[P];
                wgrad_reduce_v4_load<P>(a, rs, voff[0] + (unsigned)s * step, step, n - s);
                v[0] = wgrad_reduce_v4_sum<P>(v[0], a, n - s);
            }
        } else if (n > 0) {             // (n <= P: one pass per group, the loads of all groups first)
            f32x4 a[G][P];
#pragma unroll
            for (int gi = 0; gi < G; gi++) wgrad_reduce_v4_load<P>(a[gi], rs, voff[gi], step, n);
#pragma unroll
            for (int gi = 0; gi < G; gi++) v[gi] = wgrad_reduce_v4_sum<P>(v[gi], a[gi], n);
        }
#pragma unroll
        for (int gi = 0; gi < G; gi++) sm4[gi * 256 + threadIdx.x] = v[gi];
        __syncthreads();
        if (q < G) {
            const unsigned i = base + (unsigned)(q * 64 + e) * 4u;
            if (i < total) {
                const f32x4 t = (sm4[q * 256 + e] + sm4[q * 256 + 64 + e]) + (sm4[q * 256 + 128 + e] + sm4[q * 256 + 192 + e]);
                const unsigned co = i / per_co, rem = i - co * per_co;
                const unsigned tap = rem / (unsigned)Cin, ci = rem - tap * (unsigned)Cin;
                const size_t dst = ((size_t)co * Cin + ci) * taps + tap;
                float old[4];
#pragma unroll
                for (int c = 0; c < 4; c++) old[c] = accumulate ? g[dst + (size_t)c * taps] : 0.f;
#pragma unroll
                for (int c = 0; c < 4; c++) g[dst + (size_t)c * taps] = accumulate ? old[c] + t[c] : t[c];
            }
        }
        __syncthreads();
    }
}
__host__ __device__ inline int wgrad_reduce_v4_groups(int S) {       // G of a job: 4 for quarters of <= 4 splits, 2 for <= 8, else 1
    const int per = (S + 3) / 4;
    return per <= 4 ? 4 : (per <= 8 ? 2 : 1);
}
__device__ __forceinline__ void wgrad_reduce_v4_body(float *sm, unsigned bid, unsigned nblk, const float *__restrict__ part, int S, int Cout, int Cin,
                                                     int Cin_k, int ks, int Kpad, int Cout_pad, float *__restrict__ g_, int accumulate, int wide) {
    const int taps = ks * ks;
    const unsigned per_co = (unsigned)(taps * Cin);
    const unsigned total = (unsigned)Cout * per_co;
    const unsigned step = (unsigned)Cout_pad * (unsigned)Kpad * 4u;                 // bytes between two splits of an element
    const int e = threadIdx.x & 63, q = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (the wave's quarter, in an SGPR)
    const int per = (S + 3) / 4;
    const int s_lo = q * per, n = min(S, s_lo + per) - s_lo;        // this wave's quarter: n <= 0 when S < 4 q
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char *>((const char *)part + (size_t)s_lo * step), 0, n > 0 ? (unsigned)n * step : 0u, 0x00020000);
    f32x4 *sm4 = (f32x4 *)sm;
    glb_f32 g = (glb_f32)g_;
    const int G = wide ? wgrad_reduce_v4_groups(S) : 1;
    if (G == 4) wgrad_reduce_v4_loop<4, 4>(sm4, bid, nblk, rs, step, n, q, e, total, per_co, Cin, Cin_k, Kpad, taps, g, accumulate);
    else if (G == 2) wgrad_reduce_v4_loop<8, 2>(sm4, bid, nblk, rs, step, n, q, e, total, per_co, Cin, Cin_k, Kpad, taps, g, accumulate);
    else wgrad_reduce_v4_loop<16, 1>(sm4, bid, nblk, rs, step, n, q, e, total, per_co, Cin, Cin_k, Kpad, taps, g, accumulate);
}

// The transposing 3x3 reduce for the batched launch (job kind 4; S < 8): the per-layer body walks its (at most three) elements one after
// the other and a runtime S loop one load at a time -- about nine dependent round trips per workgroup for 9 KB.  Here every load of the
// workgroup is issued before the first addition, and a workgroup takes R of the per-layer body's (c_out, 64 input channels) units (R = 4
// for S <= 3, 2 for S <= 7: 28 / 32 KB per trip instead of 7); the additions are the per-layer body's: one group of four as
// (a0+a1)+(a2+a3) when S >= 4, then single values.
template <int SMAX, int R>
__device__ __forceinline__ void wgrad_reduce_t3v_units(float *sm, unsigned bid, const float *__restrict__ part, int S, int Cout, int Cin, int Cin_k, int Kpad,
                                                       int Cout_pad, float *__restrict__ g_, int accumulate) {
    const int cib = Cin / 64;
    const unsigned nunits = (unsigned)Cout * (unsigned)cib;
    const unsigned step = (unsigned)Cout_pad * (unsigned)Kpad * 4u;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(part), 0, (unsigned)S * step, 0x00020000);
    float a[R][3][SMAX];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const unsigned unit = bid * R + r;
        const int co = unit / cib, c0 = (unit % cib) * 64;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int idx = threadIdx.x + 256 * k;
            const int tap = idx >> 6, cl = idx & 63;
            const unsigned off = ((unsigned)co * (unsigned)Kpad + (unsigned)(tap * Cin_k + c0 + cl)) * 4u;
#pragma unroll
            for (int s = 0; s < SMAX; s++)
                a[r][k][s] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                    rs, (unit < nunits && idx < 576 && s < S) ? (int)(off + (unsigned)s * step) : (int)0x80000000, 0, 0));
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int idx = threadIdx.x + 256 * k;
            float v = 0.f;
            if constexpr (SMAX >= 4) {
                if (S >= 4) {
                    v += (a[r][k][0] + a[r][k][1]) + (a[r][k][2] + a[r][k][3]);
#pragma unroll
                    for (int s = 4; s < SMAX; s++)
                        if (S > s) v += a[r][k][s];
                } else {
#pragma unroll
                    for (int s = 0; s < 3; s++)
                        if (S > s) v += a[r][k][s];
                }
            } else {
#pragma unroll
                for (int s = 0; s < SMAX; s++)
                    if (S > s) v += a[r][k][s];
            }
            if (idx < 576) sm[r * 9 * 65 + (idx >> 6) * 65 + (idx & 63)] = v;
        }
    __syncthreads();
    float gv[R][3];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const unsigned unit = bid * R + r;
        glb_f32 dst = (glb_f32)(g_ + (size_t)unit * 576);         // ((co * Cin + c0) * 9 with c0 = 64 * (unit % cib): units are contiguous in g)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int j = threadIdx.x + 256 * k;
            gv[r][k] = (accumulate && unit < nunits && j < 576) ? dst[j] : 0.f;
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        const unsigned unit = bid * R + r;
        glb_f32 dst = (glb_f32)(g_ + (size_t)unit * 576);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int j = threadIdx.x + 256 * k;
            const int cl = j / 9, tap = j - cl * 9;
            if (unit < nunits && j < 576) {
                const float v = sm[r * 9 * 65 + tap * 65 + cl];
                dst[j] = accumulate ? gv[r][k] + v : v;
            }
        }
    }
}
__host__ __device__ inline int wgrad_reduce_t3v_units_per_block(int S) { return S <= 3 ? 4 : 2; }
__device__ __forceinline__ void wgrad_reduce_t3v_body(float *sm, unsigned bid, const float *__restrict__ part, int S, int Cout, int Cin, int Cin_k,
                                                      int Kpad, int Cout_pad, float *__restrict__ g_, int accumulate, int wide) {
    if (!wide) wgrad_reduce_t3v_units<7, 1>(sm, bid, part, S, Cout, Cin, Cin_k, Kpad, Cout_pad, g_, accumulate);
    else if (S <= 3) wgrad_reduce_t3v_units<3, 4>(sm, bid, part, S, Cout, Cin, Cin_k, Kpad, Cout_pad, g_, accumulate);
    else wgrad_reduce_t3v_units<7, 2>(sm, bid, part, S, Cout, Cin, Cin_k, Kpad, Cout_pad, g_, accumulate);
}

// Round 5: ALL split-K reduces of a backward segment as ONE launch.  Per layer the reduce is a latency-bound kernel of 5-30 us (66 + 8
// launches, 1.04 ms per bs-64 step at 3.4-3.8 TB/s: profiles/r05_train_kernel_stats.txt) that the layer's weight gradient does not need
// before the optimizer (or the bucket's all-reduce) reads it.  With one partial workspace PER LAYER (3.2 GB at bs 64 of the 288) the
// reduces of a whole segment become one streaming launch over a job table (the construction of pack_batch_kernel): a block finds its job
// by one round of parallel loads + a count and runs the per-layer body on the job's own block range -- the same bits as the per-layer
// launches (the summation order of an element depends on S and the kernel kind only).
__global__ void __launch_bounds__(256) wgrad_reduce_batch_kernel(const ryolo_wgrad_reduce_job *__restrict__ jobs, int njobs) {
    __shared__ __attribute__((aligned(16))) float sm[4096];       // (kind 3: up to four groups of 256 x 16 B)
    int lo = 0;                             // last job with block_begin <= blockIdx.x (block_begin ascending, jobs[0] starts at 0)
    if (njobs <= 256) {
        lo = __syncthreads_count((int)threadIdx.x < njobs && jobs[threadIdx.x].block_begin <= (int)blockIdx.x) - 1;
    } else {
        int hi = njobs - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (jobs[mid].block_begin <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
        }
    }
    lo = __builtin_amdgcn_readfirstlane(lo);          // (workgroup-uniform by construction: the job is read with scalar loads)
    const ryolo_wgrad_reduce_job j = jobs[lo];
    const unsigned bid = (unsigned)((int)blockIdx.x - j.block_begin), nblk = (unsigned)(j.block_end - j.block_begin);
    if (j.kind == 3) wgrad_reduce_v4_body(sm, bid, nblk, j.part, j.S, j.Cout, j.Cin_real, j.Cin_k, j.ks, j.Kpad, j.Cout_pad, j.g, j.accumulate, j.wide);
    else if (j.kind == 4) wgrad_reduce_t3v_body(sm, bid, j.part, j.S, j.Cout, j.Cin_real, j.Cin_k, j.Kpad, j.Cout_pad, j.g, j.accumulate, j.wide);
    else if (j.kind == 2) wgrad_reduce_t3_body(sm, bid, j.part, j.S, j.Cin_real, j.Cin_k, j.Kpad, j.Cout_pad, j.g, j.accumulate);
    else if (j.kind == 1) wgrad_reduce_body<4>(sm, bid, nblk, j.part, j.S, j.Cout, j.Cin_real, j.Cin_k, j.ks, j.Kpad, j.Cout_pad, j.g, j.accumulate);
    else wgrad_reduce_body<1>(sm, bid, nblk, j.part, j.S, j.Cout, j.Cin_real, j.Cin_k, j.ks, j.Kpad, j.Cout_pad, j.g, j.accumulate);
}

// ------------------------------------------------------------------------------------------------ host side: the plan of one launch
// The kernel of a launch.  The values are the public codes of ryolo_conv_wgrad_kernel_choice (include/ryolo.h): bench.py and the tools
// decode these numbers.
enum WgradKernel : int {
    WG_SQ32 = 32, WG_SQ64 = 64, WG_SQ128 = 128,                             // wgrad_kernel<T>: the square two-stage tile
    WG_256x128 = 256, WG_128x256, WG_128x3x64, WG_128x128, WG_64x128,       // wgrad_wide_kernel: the three-stage tile, c_out x c_in (x 3 taps)
    WG_ABL_256x256 = 261, WG_ABL_128x64 = 263,                              // measurement build only (ryolo_debug_wgrad_set 9 / 11)
    WG_TAPS = RYOLO_WGRAD_KERNEL_TAPS,                                      // + v: wgrad_taps_kernel on the stem shape v of wgrad_taps_variant()
};

// What the host knows about a kernel, stated once: the plan's split rule and the launch switch both read it.
struct WgradTile {
    int tm, tn;            // workgroup tile: c_out rows x c_in columns (of one tap)
    int taps;              // filter taps one workgroup owns: 1, a filter row (3), or all of them (the per-tap kernels)
    int waves, stages;     // waves per workgroup; LDS stages (2: wgrad_kernel / wgrad_taps_kernel, 3: wgrad_wide_kernel)
    int lds;               // dynamic LDS bytes
    int split3, split1;    // split target of a 3x3 / 1x1 layer: the workgroups the launch should have
};
// `stages` stages of [dz tile | x tiles], KP pixel rows each (the three-stage kernel: 32)
constexpr int wgrad_tile_lds(int stages, int tm, int tn, int taps) { return stages * (stages == 2 ? KP : 32) * (tm + taps * tn) * 2; }
// wgrad_taps_kernel<CO, CI, KS, ST>: two stages of the dz rows and the KS halo rows of 1-KiB pieces
constexpr int wgrad_taps_lds(int co, int ci, int ks, int st) {
    const int qp = (KP - 1) * st + ks, ppr = (qp * ci * 2 + 1023) / 1024;
    return 2 * (KP * co * 2 + ks * ppr * 1024);
}
// Split targets: measured on MI355X (tools/layer_bench.py --wgrad --sweep).  The kernel is fastest when the grid is about one full round of
// resident workgroups (2 per CU at the 128-row tiles; more at the smaller ones; one per CU on eight waves), and 1x1 layers (HBM-bound,
// partial tiles as large as the inputs) want fewer, longer splits (1x1 on the 128+ tiles: 256 since round 6 -- 320 / 256 / 512 measured
// 49.43 / 49.28 / 49.64 ms per step, profiles/r05_ab_log.txt).  The per-tap kernels: one workgroup per split, 512, except the first layer
// (two 10-KiB stages per workgroup, almost no MFMA work per step: four resident workgroups per CU hide its fill latency better; measured
// bs 64: 0.86 -> 0.61 ms; the C_in 32/64 variants are fastest at 512).
constexpr WgradTile wgrad_tile(int kernel) {
    switch (kernel) {
    case WG_SQ32:        return {32, 32, 1, 4, 2, wgrad_tile_lds(2, 32, 32, 1), 768, 768};
    case WG_SQ64:        return {64, 64, 1, 4, 2, wgrad_tile_lds(2, 64, 64, 1), 768, 384};
    case WG_SQ128:       return {128, 128, 1, 4, 2, wgrad_tile_lds(2, 128, 128, 1), 512, 256};
    case WG_256x128:     return {256, 128, 1, 4, 3, wgrad_tile_lds(3, 256, 128, 1), 512, 256};
    case WG_128x256:     return {128, 256, 1, 4, 3, wgrad_tile_lds(3, 128, 256, 1), 512, 256};
    case WG_128x3x64:    return {128, 64, 3, 4, 3, wgrad_tile_lds(3, 128, 64, 3), 512, 256};
    case WG_128x128:     return {128, 128, 1, 4, 3, wgrad_tile_lds(3, 128, 128, 1), 512, 256};
    case WG_64x128:      return {64, 128, 1, 4, 3, wgrad_tile_lds(3, 64, 128, 1), 384, 384};
    case WG_ABL_256x256: return {256, 256, 1, 8, 3, wgrad_tile_lds(3, 256, 256, 1), 256, 256};
    case WG_ABL_128x64:  return {128, 64, 1, 4, 3, wgrad_tile_lds(3, 128, 64, 1), 512, 256};
    case WG_TAPS + 1:    return {64, 32, 9, 4, 2, wgrad_taps_lds(64, 32, 3, 1), 512, 512};
    case WG_TAPS + 2:    return {64, 32, 9, 4, 2, wgrad_taps_lds(64, 32, 3, 2), 512, 512};     // (stride 2: 70 KiB)
    case WG_TAPS + 3:    return {32, 64, 1, 4, 2, wgrad_taps_lds(32, 64, 1, 1), 512, 512};
    case WG_TAPS + 4:    return {32, 8, 9, 4, 2, wgrad_taps_lds(32, 8, 3, 1), 1024, 1024};
    }
    return {};
}

// the all-taps kernel covers the stem shapes: (C_in, C_out, k, stride) in {(32,64,3,1), (32,64,3,2), (64,32,1,1), (8,32,3,1)}
inline int wgrad_taps_variant(const ryolo_conv_desc *d) {
    if (d->tile & 0x1000) return 0;                       // test / A-B switch: always the general kernel
    if (d->Cin == 32 && d->Cout == 64 && d->ksize == 3 && d->pad == 1 && d->stride == 1) return 1;
    if (d->Cin == 32 && d->Cout == 64 && d->ksize == 3 && d->pad == 1 && d->stride == 2) return 2;
    if (d->Cin == 64 && d->Cout == 32 && d->ksize == 1 && d->pad == 0 && d->stride == 1) return 3;
    if (d->Cin == 8 && d->Cout == 32 && d->ksize == 3 && d->pad == 1 && d->stride == 1 && d->in_cstride == 8) return 4;
    return 0;
}

#ifdef RYOLO_MP_ABLATION
int g_wgrad_abl = 0;      // ryolo_debug_wgrad_set()
#endif

// the descriptors the weight gradient serves; every query answers 0 / -1 for the others and the launch refuses them
inline bool wgrad_validate(const ryolo_conv_desc *d) { return d && (d->ksize == 1 || d->ksize == 3) && d->Cin > 0 && d->Cout > 0; }

// Everything the host decides about one launch of ryolo_conv2d_wgrad(d, ..., Cin_real, ...), computed once: the queries, the batched
// reduce's job and the launch all read it.
struct WgradPlan {
    int kernel;                    // WgradKernel
    int Ho, Wo, M;                 // output grid, N * Ho * Wo
    int Kpad, Cout_pad;            // a partial tile is [Cout_pad][Kpad] fp32
    int co_tiles, ci_tiles, tap_groups;
    int S, chunk;                  // splits; pixels per split (a multiple of KP) -- the per-tap kernels: K steps per split
    int nseg, nsteps;              // per-tap kernels: KP-pixel segments of an output row, K steps of the whole tensor
    unsigned blocks, threads;
    size_t lds, part_bytes;
    int reduce_kind;               // 0: one element per thread, 1: four split quarters per workgroup, 2: the transposing 3x3 variant
    unsigned reduce_blocks;
};

WgradPlan wgrad_plan(const ryolo_conv_desc *d, int Cin_real) {
    WgradPlan w{};
    const int ks = d->ksize, forced_s = d->tile >> 16;       // tile bits 16+: tuning aid, forced split count
    w.Ho = (d->H + 2 * d->pad - ks) / d->stride + 1;
    w.Wo = (d->W + 2 * d->pad - ks) / d->stride + 1;
    const long long M = (long long)d->N * w.Ho * w.Wo;
    w.M = (int)M;
    w.Kpad = (ks * ks * d->Cin + 63) / 64 * 64;
    if (const int variant = wgrad_taps_variant(d)) {
        w.kernel = WG_TAPS + variant;
        w.Cout_pad = d->Cout;                                // the per-tap kernels write unpadded rows
        w.co_tiles = w.ci_tiles = w.tap_groups = 1;
        w.nseg = (w.Wo + KP - 1) / KP;
        const long long nsteps = (long long)d->N * w.Ho * w.nseg, smax = wgrad_tile(w.kernel).split3;
        w.nsteps = (int)nsteps;
        long long S = nsteps < smax ? nsteps : smax;         // split count (= workgroups)
        if (forced_s) S = forced_s;
        if (S > nsteps) S = nsteps;
        if (S < 1) S = 1;
        const long long per = (nsteps + S - 1) / S;
        w.S = (int)((nsteps + per - 1) / per);
        w.chunk = (int)per;
    } else {
        const int mn = d->Cin < d->Cout ? d->Cin : d->Cout;
        const bool square = d->tile & 0x2000;                // tile bit 0x2000 forces the square two-stage tile
        const int co256 = (d->Cout + 255) / 256;
        w.kernel = mn >= 128 ? WG_SQ128 : (mn >= 64 ? WG_SQ64 : WG_SQ32);
        // wide tile (256 c_out x 128 c_in) when both channel counts fill it
        // (round 6: also ragged C_out >= 256 whose last 256-row tile is at least 7/8 full -- the 504-channel heads, which ran the two-stage square
        //  tile at 268 / 145 / 82 us.  Rows past C_out read whatever follows in the dz row (the next pixel's channels; past the tensor's end the
        //  descriptor returns zeros): their products land in accumulator rows the epilogue does not store.)
        if (d->Cout >= 256 && (co256 * 256 - d->Cout) * 8 <= 256 && d->Cin % 128 == 0 && !square) {
            w.kernel = WG_256x128;
#ifdef RYOLO_MP_ABLATION
            if (g_wgrad_abl == 9 && d->Cin % 256 == 0) w.kernel = WG_ABL_256x256;       // experiment: eight waves of 64 x 128, one workgroup per CU
#endif
        } else if (d->Cout % 128 == 0 && d->Cin == 64 && ks == 3 && !square) {
            // the 64 -> 128 layers at 152^2: the same three-stage kernel on a 128 x (3 taps x 64) tile (64 x 96 wave tiles, 60 KiB of LDS; rounds
            // 3-5: one tap per workgroup, 128 x 64)
            w.kernel = WG_128x3x64;
#ifdef RYOLO_MP_ABLATION
            if (g_wgrad_abl == 11) w.kernel = WG_ABL_128x64;                            // A/B: one tap per workgroup on the 128 x 64 tile (rounds 3-5)
#endif
        } else if (d->Cout == 64 && d->Cin % 128 == 0 && !square) {
            // (round 6) the 128 -> 64 1x1 bottlenecks at 152^2: the three-stage kernel on a 64 x 128 tile (two-stage square tile: 145 us each)
            w.kernel = WG_64x128;
        } else if (d->Cout % 128 == 0 && d->Cin % 128 == 0 && !square) {
            // the remaining 128-multiples (the 256 -> 128 / 384 -> 128 1x1 bottlenecks): the three-stage kernel on the square tile --
            // same fragments and summation order as wgrad_kernel<128> (bit-identical results), counted waits instead of a full drain
            // per step: 0.088 -> 0.075 ms on 256->128@76^2 at bs 64
            w.kernel = WG_128x128;
        } else if (d->Cout % 128 == 0 && d->Cin % 256 == 0 && (d->tile & 0x4000)) {
            // the same tile transposed; off by default -- on the 256->128 1x1 bottlenecks it measured 9 % SLOWER than the
            // square tile (0.093 vs 0.085 ms at bs 64: HBM-bound, the partial tiles double); tile bit 0x4000 selects it for tests
            w.kernel = WG_128x256;
        }
        const WgradTile t = wgrad_tile(w.kernel);
        w.Cout_pad = (d->Cout + 127) / 128 * 128;
        w.co_tiles = (d->Cout + t.tm - 1) / t.tm;
        w.ci_tiles = (d->Cin + t.tn - 1) / t.tn;
        w.tap_groups = ks * ks / t.taps;                     // workgroups per (channel tile, split): one per tap, or one per filter row
        const int base = w.co_tiles * w.ci_tiles * w.tap_groups;
        const int target = (ks == 3 ? t.split3 : t.split1) * (d->Cin <= 8 ? 2 : 1);      // (the first layer's 8 channels: twice the 32-tile's target)
        int S = target / base;
        if (2 * base > target) {   // few splits: pick the one (<= 5) that wastes the least of the last round
            double best = -1.0;
            for (int c = 1; c <= 5; c++) {
                const int blocks = c * base;
                const double eff = (double)blocks / (double)((blocks + 511) / 512 * 512);
                if (eff > best + 0.02) { best = eff; S = c; }
            }
        }
        if (forced_s) S = forced_s;
        const long long max_s = (M + KP - 1) / KP;
        if (S > max_s) S = (int)max_s;
        const size_t per = (size_t)w.Cout_pad * w.Kpad * 4;
        while (S > 1 && per * S > (size_t)512 << 20) S--;
        if (S < 1) S = 1;
        long long chunk = (M + S - 1) / S;
        chunk = (chunk + KP - 1) / KP * KP;
        w.S = (int)((M + chunk - 1) / chunk);
        w.chunk = (int)chunk;
    }
    const WgradTile t = wgrad_tile(w.kernel);
    w.blocks = (unsigned)(w.co_tiles * w.ci_tiles * w.tap_groups * w.S);
    w.threads = (unsigned)t.waves * 64;
    w.lds = (size_t)t.lds;
    w.part_bytes = (size_t)w.S * w.Cout_pad * w.Kpad * 4;
    // the per-layer reduce
    const long long total = (long long)d->Cout * Cin_real * ks * ks;
    if (w.S < 8 && ks == 3 && Cin_real % 64 == 0 && total >= (1 << 20)) {
        w.reduce_kind = 2;
        w.reduce_blocks = (unsigned)(d->Cout * (Cin_real / 64));
    } else {
        w.reduce_kind = w.S >= 8 ? 1 : 0;
        w.reduce_blocks = (unsigned)grid_for(total, w.S >= 8 ? 64 : 256);
    }
    return w;
}

// ------------------------------------------------------------------------------------------------ host side: the launches
// the tile kernel of the plan: the instantiation of code K is the one its table row describes
template <int K>
int launch_wgrad_tiles(const WgradPlan &w, const WgradParams &p, hipStream_t stream) {
    constexpr WgradTile t = wgrad_tile(K);
    const dim3 grid(w.blocks), block(w.threads);
#ifdef RYOLO_MP_ABLATION      // ryolo_debug_wgrad_set: the timing-only ablations of the wide tile (1, 2, 4, 6, 7) and its eight-wave instantiation (8)
    if constexpr (K == WG_256x128) {
#define RYOLO_WG_ABL(A, NW) \
    if (g_wgrad_abl == (NW == 8 ? 8 : A)) return launch_kernel<wgrad_wide_kernel<t.tm, t.tn, A, NW>>(grid, dim3(NW * 64), w.lds, stream, p);
        RYOLO_WG_ABL(1, 4) RYOLO_WG_ABL(2, 4) RYOLO_WG_ABL(4, 4) RYOLO_WG_ABL(6, 4) RYOLO_WG_ABL(7, 4) RYOLO_WG_ABL(0, 8)
#undef RYOLO_WG_ABL
    }
#endif
    if constexpr (t.stages == 2) return launch_kernel<wgrad_kernel<t.tm>>(grid, block, w.lds, stream, p);
    else return launch_kernel<wgrad_wide_kernel<t.tm, t.tn, 0, t.waves, t.taps>>(grid, block, w.lds, stream, p);
}

// the same launch as the per-tap kernels take it
template <int CO, int CI, int KS, int ST>
int launch_wgrad_taps(const WgradPlan &w, const WgradParams &p, hipStream_t stream) {
    WgradTapsParams q;
    q.x = p.x; q.dz = p.dz; q.part = p.part;
    q.N = p.N; q.H = p.H; q.W = p.W; q.x_cs = p.x_cs; q.Ho = p.Ho; q.Wo = p.Wo; q.dz_cs = p.dz_cs; q.pad = p.pad;
    q.Cout = p.Cout; q.Kpad = p.Kpad;
    q.nseg = w.nseg; q.nsteps = w.nsteps; q.steps_per_split = w.chunk;
    q.x_bytes = p.x_bytes; q.dz_bytes = p.dz_bytes;
    return launch_kernel<wgrad_taps_kernel<CO, CI, KS, ST>>(dim3(w.blocks), dim3(w.threads), w.lds, stream, q);
}

enum WgradPhase { WG_BOTH, WG_TILES_ONLY, WG_REDUCE_ONLY };

// the launches of one planned weight gradient: the tile kernel into the partial tiles, the reduce into the gradient
int wgrad_launch(const WgradPlan &w, const ryolo_conv_desc *d, const void *x, const void *dz, int dz_cstride, int Cin_real, float *grad_oihw,
                 int accumulate, void *workspace, WgradPhase phase, hipStream_t stream) {
    WgradParams p;
    p.x = (const __bf16 *)x; p.dz = (const __bf16 *)dz; p.part = (float *)workspace;
    p.N = d->N; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.x_cs = d->in_cstride;
    p.Ho = w.Ho; p.Wo = w.Wo; p.Cout = d->Cout; p.dz_cs = dz_cstride;
    p.ks = d->ksize; p.stride = d->stride; p.pad = d->pad;
    p.Kpad = w.Kpad; p.Cout_pad = w.Cout_pad; p.M = w.M;
    p.S = w.S; p.chunk = w.chunk; p.co_tiles = w.co_tiles; p.ci_tiles = w.ci_tiles;
    if (!buffer_extent((unsigned long long)d->N * d->H * d->W, d->in_cstride, d->Cin, &p.x_bytes) ||
        !buffer_extent((unsigned long long)w.M, dz_cstride, d->Cout, &p.dz_bytes))
        return RYOLO_EINVAL;
    int rc = RYOLO_OK;
    if (phase != WG_REDUCE_ONLY) switch (w.kernel) {
    case WG_TAPS + 1: rc = launch_wgrad_taps<64, 32, 3, 1>(w, p, stream); break;
    case WG_TAPS + 2: rc = launch_wgrad_taps<64, 32, 3, 2>(w, p, stream); break;
    case WG_TAPS + 3: rc = launch_wgrad_taps<32, 64, 1, 1>(w, p, stream); break;
    case WG_TAPS + 4: rc = launch_wgrad_taps<32, 8, 3, 1>(w, p, stream); break;
    case WG_256x128: rc = launch_wgrad_tiles<WG_256x128>(w, p, stream); break;
    case WG_128x256: rc = launch_wgrad_tiles<WG_128x256>(w, p, stream); break;
    case WG_128x3x64: rc = launch_wgrad_tiles<WG_128x3x64>(w, p, stream); break;
    case WG_128x128: rc = launch_wgrad_tiles<WG_128x128>(w, p, stream); break;
    case WG_64x128: rc = launch_wgrad_tiles<WG_64x128>(w, p, stream); break;
#ifdef RYOLO_MP_ABLATION
    case WG_ABL_256x256: rc = launch_wgrad_tiles<WG_ABL_256x256>(w, p, stream); break;
    case WG_ABL_128x64: rc = launch_wgrad_tiles<WG_ABL_128x64>(w, p, stream); break;
#endif
    case WG_SQ128: rc = launch_wgrad_tiles<WG_SQ128>(w, p, stream); break;
    case WG_SQ64: rc = launch_wgrad_tiles<WG_SQ64>(w, p, stream); break;
    default: rc = launch_wgrad_tiles<WG_SQ32>(w, p, stream); break;
    }
    if (rc != RYOLO_OK || phase == WG_TILES_ONLY) return rc;
    const float *part = (const float *)workspace;
    const dim3 grid(w.reduce_blocks), block(256);
    if (w.reduce_kind == 2)
        return launch_kernel<wgrad_reduce_t3_kernel>(grid, block, 0, stream, part, w.S, Cin_real, d->Cin, w.Kpad, w.Cout_pad, grad_oihw, accumulate);
    if (w.reduce_kind == 1)
        return launch_kernel<wgrad_reduce_kernel<4>>(grid, block, 0, stream, part, w.S, d->Cout, Cin_real, d->Cin, d->ksize, w.Kpad, w.Cout_pad,
                                                     grad_oihw, accumulate);
    return launch_kernel<wgrad_reduce_kernel<1>>(grid, block, 0, stream, part, w.S, d->Cout, Cin_real, d->Cin, d->ksize, w.Kpad, w.Cout_pad, grad_oihw,
                                                 accumulate);
}

// the three entry points of one weight gradient: argument checks, the plan, the launches of `phase`
int wgrad_call(WgradPhase phase, const ryolo_conv_desc *d, const void *x, const void *dz, int dz_cstride, int Cin_real, float *grad_oihw,
               int accumulate, void *workspace, size_t workspace_bytes, void *stream) {
    if (!x || !dz || !grad_oihw || !workspace || !wgrad_validate(d)) return RYOLO_EINVAL;
    if ((d->Cin & 7) || (d->Cout & 7) || (d->in_cstride & 7) || (dz_cstride & 7) || Cin_real <= 0 || Cin_real > d->Cin) return RYOLO_EINVAL;
    const WgradPlan w = wgrad_plan(d, Cin_real);
    if (workspace_bytes < w.part_bytes) return RYOLO_EINVAL;
    return wgrad_launch(w, d, x, dz, dz_cstride, Cin_real, grad_oihw, accumulate, workspace, phase, (hipStream_t)stream);
}

}  // namespace

extern "C" {

#ifdef RYOLO_MP_ABLATION
void ryolo_debug_wgrad_set(int abl) { g_wgrad_abl = abl; }
#endif

size_t ryolo_conv_wgrad_workspace_bytes(const ryolo_conv_desc *d) { return wgrad_validate(d) ? wgrad_plan(d, d->Cin).part_bytes : 0; }

int ryolo_conv_wgrad_kernel_choice(const ryolo_conv_desc *d) { return wgrad_validate(d) ? wgrad_plan(d, d->Cin).kernel : -1; }

int ryolo_conv2d_wgrad(const ryolo_conv_desc *d, const void *x, const void *dz, int dz_cstride, int Cin_real, float *grad_oihw, int accumulate,
                       void *workspace, size_t workspace_bytes, void *stream) {
    return wgrad_call(WG_BOTH, d, x, dz, dz_cstride, Cin_real, grad_oihw, accumulate, workspace, workspace_bytes, stream);
}
// measurement: the two launches of ryolo_conv2d_wgrad as separate calls (bench.py's in-run kernel table brackets library calls with
// events; the tile kernel and the split-K reduce get a row each).  Same arguments, same results as the one call.
int ryolo_conv2d_wgrad_partials(const ryolo_conv_desc *d, const void *x, const void *dz, int dz_cstride, int Cin_real, float *grad_oihw,
                                int accumulate, void *workspace, size_t workspace_bytes, void *stream) {
    return wgrad_call(WG_TILES_ONLY, d, x, dz, dz_cstride, Cin_real, grad_oihw, accumulate, workspace, workspace_bytes, stream);
}
int ryolo_conv2d_wgrad_reduce(const ryolo_conv_desc *d, const void *x, const void *dz, int dz_cstride, int Cin_real, float *grad_oihw,
                              int accumulate, void *workspace, size_t workspace_bytes, void *stream) {
    return wgrad_call(WG_REDUCE_ONLY, d, x, dz, dz_cstride, Cin_real, grad_oihw, accumulate, workspace, workspace_bytes, stream);
}

/* the reduce of one layer as a job of ryolo_conv_wgrad_reduce_batch: what ryolo_conv2d_wgrad_reduce(d, ..., workspace) would launch.  Returns the
 * job's block count (also left in job->block_end, block_begin = 0: the caller lays the jobs out back to back) or 0. */
int ryolo_conv_wgrad_reduce_job_fill(ryolo_wgrad_reduce_job *job, const ryolo_conv_desc *d, int Cin_real, const void *workspace, float *grad_oihw,
                                     int accumulate) {
    if (!job || !workspace || !grad_oihw || !wgrad_validate(d) || Cin_real <= 0 || Cin_real > d->Cin) return 0;
    const WgradPlan w = wgrad_plan(d, Cin_real);
    *job = ryolo_wgrad_reduce_job{};
    job->part = (const float *)workspace; job->g = grad_oihw; job->accumulate = accumulate ? 1 : 0;
    job->S = w.S; job->Cout = d->Cout; job->Cin_real = Cin_real; job->Cin_k = d->Cin; job->ks = d->ksize;
    job->Kpad = w.Kpad; job->Cout_pad = w.Cout_pad; job->kind = w.reduce_kind;
    unsigned blocks = w.reduce_blocks;
    // the batched launch's own form of the four-quarter reduce: four input channels per thread, every load of a quarter in flight
    // (RYOLO_WGRAD_REDUCE_V4=0: the per-layer body, for the A/B).  Needs 16-B aligned partial rows: C_in % 4, workspace % 16.
    const char *env = abl_env("RYOLO_WGRAD_REDUCE_V4");         // (measurement build) 0: the per-layer bodies, 1: kind 3 only, 2: kinds 3 and 4, default: + wide
    const bool v4 = !(env && env[0] == '0'), t3v = !(env && (env[0] == '0' || env[0] == '1'));
    const int wide = !(env && env[0] >= '0' && env[0] <= '2');         // (2: kinds 3 and 4 with one group / unit per workgroup)
    const long long step_bytes = (long long)w.Cout_pad * w.Kpad * 4;                // (32-bit buffer offsets: a quarter + one pass of 16)
    if (job->kind == 1 && v4 && Cin_real % 4 == 0 && d->Cin % 4 == 0 && ((uintptr_t)workspace & 15) == 0 &&
        ((w.S + 3) / 4 + 17) * step_bytes < (1ll << 31)) {
        job->kind = 3;
        job->wide = wide;
        blocks = (unsigned)grid_for((long long)d->Cout * Cin_real * d->ksize * d->ksize, 256 * (wide ? wgrad_reduce_v4_groups(w.S) : 1));
    }
    if (job->kind == 2 && t3v && w.S < 8 && 8 * step_bytes < (1ll << 31)) {      // (every load in flight, 4 or 2 of kind 2's units per workgroup)
        job->kind = 4;
        job->wide = wide;
        const int r = wide ? wgrad_reduce_t3v_units_per_block(w.S) : 1;
        blocks = (blocks + r - 1) / r;
    }
    job->block_begin = 0;
    job->block_end = (int)blocks;
    return (int)blocks;
}

int ryolo_conv_wgrad_reduce_batch(const ryolo_wgrad_reduce_job *device_jobs, int njobs, int total_blocks, void *stream) {
    if (!device_jobs || njobs <= 0 || total_blocks <= 0) return RYOLO_EINVAL;
    return launch_kernel<wgrad_reduce_batch_kernel>(dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, device_jobs, njobs);
}

}  // extern "C"
