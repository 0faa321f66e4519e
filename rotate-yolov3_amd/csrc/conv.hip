// rotate-yolov3_amd/csrc/conv.hip -- NHWC bf16 implicit-GEMM convolution on MFMA for gfx950 (MI355X), with the
// Darknet block epilogue fused:  y = [upsample2x]( act( conv(x, W) * scale[c] + shift[c] ) [+ residual] ).
//
// Replaces, for the Darknet-53 stack, the reference's per-layer operator chain
//   nn.Conv2d -> nn.BatchNorm2d(eval) -> nn.PReLU            (model/models.py:49-66)
//   x + layer_outputs[from]                                   (shortcut, model/models.py:281-282)
//   nn.Upsample(nearest, x2) + torch.cat(.., 1)               (model/models.py:93-94, :269-278)
// which the reference dispatches to cuDNN / ATen as separate kernels.  scale/shift are the folded eval-mode
// BatchNorm (utils/torch_utils.py:45-69 computes the same fold into the weights; here it stays in fp32 and is
// applied to the fp32 accumulator), or (1, bias) for the three head convs.  Channel-sliced input / output /
// residual tensors (pixel stride != channel count) let route/concat layers be written in place, no copy.
//
// GEMM view:  D[c_out][pixel] = sum_k Wp[c_out][k] * X[pixel][k],  k = (kh*KS + kw)*C_in + c,  pixel = (img, ho, wo).
//   - MFMA 16x16x32 bf16, weights as the A operand so that each lane ends up with 4 CONSECUTIVE output channels
//     of one pixel (NHWC-contiguous) in its accumulator fragment.
//   - Tiles BM pixels x BN channels x BK=64; 4 waves; both operands staged HBM->LDS with 16-B direct-to-LDS loads
//     (global_load_lds_dwordx4), double buffered, one barrier per K step.  The LDS image of a tile is
//     [row][8 x 16-B slots] with slot ^= (row>>1)&7 so the ds_read_b128 fragment reads are bank-conflict free;
//     direct-to-LDS writes are lane-linear, so the XOR is applied to the per-lane SOURCE address (and again on
//     the read).  Zero padding, M/K tails: the lane's source pointer is redirected to a zero page.
//   - Epilogue: scale/shift/activation in fp32 on the accumulators -> bf16 -> LDS staging tile -> coalesced
//     16-B rows: + residual (fp32 add, one more bf16 rounding, i.e. the unfused layer-by-layer result) -> store
//     (optionally replicated 2x2 for the fused nearest upsample).
//   - Workgroup -> tile map is XCD-aware: the 8 XCDs get contiguous chunks of the tile list, channel tiles
//     fastest, so the blocks that share an activation tile run on one XCD's L2 back to back.
#include "conv_common.h"

using namespace ryolo_detail;

namespace {

// GEN = false: inference instantiation (no BatchNorm-statistics epilogue, dense output placement);
// GEN = true : training instantiation (statistics partials, strided output placement for the stride-2 dgrad classes).
// BNRED (training backward, stride-1 data gradients that are the LAST writer of a BatchNorm block's output gradient): epilogue 2 --
// where a thread holds 8 consecutive channels of a pixel exactly as they are stored -- also runs the first pass of that block's
// BatchNorm/activation backward on them (see the persistent kernel below for the arithmetic), one extra 16-B read of z per chunk.
// A thread keeps the same 8 channels for all its chunks; its 24 sums are combined over the workgroup in a fixed order and stored
// (not added) into row m_tile of part[m_tiles][3][C]: every (row, channel) has exactly one writer.
template <int KS, int BM, int BN, int WGM, int WGN, int NSTAGE, bool FAST, bool GEN, bool BNRED = false>
__global__ void __launch_bounds__(WGM *WGN * 64) conv_igemm_kernel(const ConvParams p, const BnRed br = BnRed()) {
    constexpr int NW = WGM * WGN, NT = NW * 64;
    constexpr int WPIX = BM / WGM, WCH = BN / WGN, PF = WPIX / 16, CF = WCH / 16;
    constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE = A_BYTES + B_BYTES;
    constexpr int A_PPW = (BM / 8) / NW, B_PPW = (BN / 8) / NW;   // 1-KiB pieces (8 tile rows) per wave
    static_assert(A_PPW >= 1 && B_PPW >= 1, "tile too small for the wave count");
    constexpr int SROW = BN * 2 + 16;                              // epilogue staging row pitch (bytes)
    static_assert(BM * SROW + WGM * 2 * BN * 4 <= NSTAGE * STAGE, "staging tile + statistics slots must fit in the operand buffers");
    constexpr int LOADS_PER_STAGE = A_PPW + B_PPW;   // direct-to-LDS instructions one wave issues per K step

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // ---- XCD-aware tile assignment (bijective for any grid size)
    int m_tile, n_tile;
    {
        const int nblk = gridDim.x, bid = blockIdx.x;
        const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7, loc = bid >> 3;
        const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
        n_tile = id % p.nt;
        m_tile = id / p.nt;
    }
    const int m0 = m_tile * BM, n0 = n_tile * BN;

    const __bf16 *zero_page = p.w + (size_t)(((p.Cout + 127) >> 7) << 7) * p.Kpad;
    const long long zero_off = zero_page - p.x;   // element distance; both bf16 arrays (any two device pointers)

    // ---- BNRED: the consumer block's z for the chunks this thread stores in epilogue 2, and its BatchNorm constants, are requested
    // FIRST -- z was written a whole forward pass ago (an HBM miss, unlike the running gradient the epilogue also reads), and loaded in
    // the epilogue its latency was exposed once per tile (+16 % on the 128 x 128 data gradients); here it hides under the K loop.
    constexpr int BR_CPR = BN / 8, BR_NIT = BM * BR_CPR / NT;
    bf16x8 zv[BNRED ? BR_NIT : 1];
    if constexpr (BNRED) {
        const int c = n0 + (tid % BR_CPR) * 8;
#pragma unroll
        for (int it = 0; it < BR_NIT; it++) {
            const int m = m0 + (it * NT + tid) / BR_CPR;
            zv[it] = *(const bf16x8 *)((m < p.M && c < p.Cout) ? br.z + (size_t)m * br.z_cs + c : zero_page);
        }
    }

    // ---- per-lane staging bookkeeping.  Lane l of a wave fills 16-B slot (l & 7) of tile row 8*piece + (l >> 3).
    long long a_base[A_PPW];   // element offset of (img, hi0, wi0, c=0); may be negative (padding)
    int a_hi0[A_PPW], a_wi0[A_PPW], a_slot[A_PPW];
#pragma unroll
    for (int j = 0; j < A_PPW; j++) {
        const int piece = wave * A_PPW + j;
        const int row = piece * 8 + (lane >> 3);
        a_slot[j] = (lane & 7) ^ ((row >> 1) & 7);
        const int m = m0 + row;
        if (m < p.M) {
            int wo, ho, img;
            split_pixel(m, p.Wo, p.Ho, p.magic_wo, p.magic_ho, p.use_magic, wo, ho, img);
            a_hi0[j] = ho * p.stride - p.pad;
            a_wi0[j] = wo * p.stride - p.pad;
            a_base[j] = (((long long)img * p.H + a_hi0[j]) * p.W + a_wi0[j]) * p.in_cs;
        } else {
            a_hi0[j] = -(1 << 28);   // always out of bounds -> zero page
            a_wi0[j] = -(1 << 28);
            a_base[j] = 0;
        }
    }
    const __bf16 *b_ptr[B_PPW];
#pragma unroll
    for (int j = 0; j < B_PPW; j++) {
        const int piece = wave * B_PPW + j;
        const int row = piece * 8 + (lane >> 3);
        const int slot = (lane & 7) ^ ((row >> 1) & 7);
        b_ptr[j] = p.w + (size_t)(n0 + row) * p.Kpad + slot * 8;
    }

    // FAST path (Cin % 64 == 0, tensors < 2 GiB): a whole K step lies inside one filter tap, so the tap offset is a
    // SCALAR and the per-lane work per 1-KiB piece is one 32-bit add and one select.  Loads are buffer loads with a
    // per-lane byte offset: an invalid (padding / M-tail) lane gets an out-of-range offset and the hardware
    // writes zeros to LDS -- no zero page, no 64-bit address arithmetic, no branches in the K loop.
    int a_off32[A_PPW];          // byte offset of (img, hi0, wi0, slot*8); wraps for border pixels, only used when valid
    unsigned a_mask[A_PPW];      // bit t: tap t of the tap list reads inside the image for this lane's pixel
    int b_off32[B_PPW];
    if constexpr (FAST) {
#pragma unroll
        for (int j = 0; j < A_PPW; j++) {
            // taps2 (C_in == 32, one K step = two taps): the slot's low 2 bits pick the channels, bit 2 picks the tap
            a_off32[j] = (int)(a_base[j] * 2) + (p.taps2 ? (a_slot[j] & 3) : a_slot[j]) * 16;
            unsigned mk = 0;
            if constexpr (GEN) {          // arbitrary tap list (dgrad parity classes)
#pragma unroll
                for (int t = 0; t < 9; t++) {     // branch-free: 72 scalar branches per tile cost as much as a short K loop
                    const int hi = a_hi0[j] + p.tap_dy[t], wi = a_wi0[j] + p.tap_dx[t];
                    const unsigned in = (unsigned)(t < p.ntaps) & (unsigned)((unsigned)hi < (unsigned)p.H) & (unsigned)((unsigned)wi < (unsigned)p.W);
                    mk |= in << t;
                }
            } else {                      // the regular KS x KS window
#pragma unroll
                for (int t = 0; t < KS * KS; t++) {
                    const int hi = a_hi0[j] + t / KS, wi = a_wi0[j] + t % KS;
                    if ((unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W) mk |= 1u << t;
                }
            }
            a_mask[j] = mk;
        }
#pragma unroll
        for (int j = 0; j < B_PPW; j++) b_off32[j] = (int)((b_ptr[j] - p.w) * 2);
    }
    // running (scalar) position of the K loop for the FAST path: tap index, channel offset inside the tap
    int f_tap = 0, f_c0 = 0;
    // lane t keeps the byte offset of tap t; the K loop fetches the current one with v_readlane (no memory access)
    int lane_tapoff = 0;
    int f_kh = 0, f_kw = 0;       // GEN = false: plain scalar counters over the KS x KS window
    if constexpr (FAST && GEN) {
        const int t = lane < p.ntaps ? lane : 0;
        lane_tapoff = ((p.tap_dy[t] * p.W + p.tap_dx[t]) * p.in_cs) * 2;
    }

    auto stage_fast = [&](int kt, int buf) {
        char *abuf = smem + buf * STAGE;
        char *bbuf = abuf + A_BYTES;
        int tapoff;                                                                   // scalar
        if constexpr (GEN) tapoff = __builtin_amdgcn_readlane(lane_tapoff, f_tap) + f_c0 * 2;
        else tapoff = ((f_kh * p.W + f_kw) * p.in_cs + f_c0) * 2;
        if (p.taps2) {
            // C_in == 32 (regular KS x KS window only): K step kt = taps 2kt and 2kt+1 (tap 9 = K padding, its mask bit is 0);
            // two scalar tap offsets, each lane picks by bit 2 of its logical slot
            const int t0 = 2 * kt, t1 = 2 * kt + 1;
            int off0, off1;
            if constexpr (GEN) {       // the training instantiation keeps its window as a tap list (lane t: tap t's offset)
                off0 = __builtin_amdgcn_readlane(lane_tapoff, t0);
                off1 = __builtin_amdgcn_readlane(lane_tapoff, t1);
            } else {
                const int kh0 = (t0 * 11) >> 5, kw0 = t0 - 3 * kh0, kh1 = (t1 * 11) >> 5, kw1 = t1 - 3 * kh1;
                off0 = ((kh0 * p.W + kw0) * p.in_cs) * 2;
                off1 = ((kh1 * p.W + kw1) * p.in_cs) * 2;
            }
#pragma unroll
            for (int j = 0; j < A_PPW; j++) {
                const int hi = a_slot[j] >> 2;
                const bool ok = (a_mask[j] >> (t0 + hi)) & 1u;
                const int voff = ok ? a_off32[j] + (hi ? off1 : off0) : (int)0x80000000;
                buffer_load_lds16(p.x, p.x_bytes, abuf + (wave * A_PPW + j) * 1024, voff, 0);
            }
#pragma unroll
            for (int j = 0; j < B_PPW; j++)
                buffer_load_lds16(p.w, p.w_bytes, bbuf + (wave * B_PPW + j) * 1024, b_off32[j], kt * (BK * 2));
            return;
        }
#pragma unroll
        for (int j = 0; j < A_PPW; j++) {
            const bool ok = (a_mask[j] >> f_tap) & 1u;
            const int voff = ok ? a_off32[j] + tapoff : (int)0x80000000;
            buffer_load_lds16(p.x, p.x_bytes, abuf + (wave * A_PPW + j) * 1024, voff, 0);
        }
#pragma unroll
        for (int j = 0; j < B_PPW; j++)
            buffer_load_lds16(p.w, p.w_bytes, bbuf + (wave * B_PPW + j) * 1024, b_off32[j], kt * (BK * 2));
        // advance the scalar K position (stage() is called with consecutive kt)
        f_c0 += BK;
        if (f_c0 >= p.Cin) {
            f_c0 = 0;
            f_tap++;
            if constexpr (!GEN) {
                if (++f_kw == KS) { f_kw = 0; f_kh++; }
            }
        }
    };

    auto stage_slow = [&](int kt, int buf) {
        char *abuf = smem + buf * STAGE;
        char *bbuf = abuf + A_BYTES;
#pragma unroll
        for (int j = 0; j < A_PPW; j++) {
            const int k = kt * BK + a_slot[j] * 8;
            long long off;
            bool ok;
            if (KS == 1) {
                ok = (a_hi0[j] >= 0) && (k < p.K);
                off = a_base[j] + k;
            } else {
                int tap, c;
                if (p.cin_log2 >= 0) {            // power-of-two Cin: shifts
                    tap = k >> p.cin_log2;
                    c = k & (p.Cin - 1);
                } else {                          // Cin % 64 == 0: a whole K step lies inside one tap (uniform divide)
                    tap = (kt * BK) / p.Cin;
                    c = k - tap * p.Cin;
                }
                const int kh = (tap * 11) >> 5, kw = tap - 3 * kh;
                const int hi = a_hi0[j] + kh, wi = a_wi0[j] + kw;
                ok = (k < p.K) && ((unsigned)hi < (unsigned)p.H) && ((unsigned)wi < (unsigned)p.W);
                off = a_base[j] + (long long)(kh * p.W + kw) * p.in_cs + c;
            }
            const __bf16 *src = p.x + (ok ? off : zero_off);   // select, no branch
            __builtin_amdgcn_global_load_lds((glb_vp)src, (lds_vp)(abuf + (wave * A_PPW + j) * 1024), 16, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < B_PPW; j++) {
            __builtin_amdgcn_global_load_lds((glb_vp)(b_ptr[j] + kt * BK),
                                             (lds_vp)(bbuf + (wave * B_PPW + j) * 1024), 16, 0, 0);
        }
    };

    auto stage = [&](int kt, int buf) {
        if constexpr (FAST) stage_fast(kt, buf);
        else stage_slow(kt, buf);
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
    if constexpr (NSTAGE == 2) {
        stage(0, 0);
        for (int kt = 0; kt + 1 < KT; kt++) {
            __syncthreads();   // drains this wave's direct-to-LDS loads (vmcnt(0)) and orders all waves: tile kt landed,
                               // and nobody still reads the buffer that the next stage() overwrites
            stage(kt + 1, (kt + 1) & 1);
            compute(kt & 1);
        }
        __syncthreads();
        compute((KT - 1) & 1);
    } else {
        // NSTAGE-deep ring with COUNTED waits: tiles kt+1 .. kt+NSTAGE-2 stay in flight across the barrier, so the
        // HBM/L2 latency of a tile (~2000 cycles under load, longer than one K step of MFMA work) is covered by
        // NSTAGE-1 steps of compute.  hipcc's __syncthreads() would drain vmcnt to 0 while direct-to-LDS loads are
        // pending, hence the raw s_barrier + explicit s_waitcnt (cdna_hip_programming.md, "Pipelining across barriers").
#pragma unroll
        for (int t = 0; t < NSTAGE - 1; t++)
            if (t < KT) stage(t, t);
        int buf = 0;
        for (int kt = 0; kt < KT; kt++) {
            // tiles kt .. min(kt+NSTAGE-2, KT-1) have been issued; wait until only the younger ones are outstanding
            const int younger = min(NSTAGE - 2, KT - 1 - kt);
            if (younger >= NSTAGE - 2) {
                if constexpr (NSTAGE == 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LOADS_PER_STAGE) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LOADS_PER_STAGE) : "memory");
            } else if (NSTAGE == 4 && younger == 1) {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LOADS_PER_STAGE) : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();   // every wave's share of tile kt has landed; tile kt-1's buffer is free
            if (kt + NSTAGE - 1 < KT) {
                int nb = buf + NSTAGE - 1;
                if (nb >= NSTAGE) nb -= NSTAGE;
                stage(kt + NSTAGE - 1, nb);
            }
            compute(buf);
            buf = (buf + 1 == NSTAGE) ? 0 : buf + 1;
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }

    // ---- epilogue 1: scale/shift/activation on the fp32 accumulators -> bf16 -> LDS staging tile
    float st_sum[CF][4], st_sq[CF][4];
#pragma unroll
    for (int c = 0; c < CF; c++)
#pragma unroll
        for (int r = 0; r < 4; r++) st_sum[c][r] = st_sq[c][r] = 0.f;
    __syncthreads();
    auto epilogue1 = [&](auto actfn) {
#pragma unroll
        for (int c = 0; c < CF; c++) {
            const int ch_local = wn * WCH + c * 16 + fk * 4;
            const f32x4 sc = *(const f32x4 *)(p.scale + n0 + ch_local);
            const f32x4 sh = *(const f32x4 *)(p.shift + n0 + ch_local);
#pragma unroll
            for (int f = 0; f < PF; f++) {
                const int pix_local = wm * WPIX + f * 16 + frow;
                bf16x4 o;
#pragma unroll
                for (int r = 0; r < 4; r++) o[r] = (__bf16)actfn(acc[c][f][r] * sc[r] + sh[r]);
                *(bf16x4 *)(smem + pix_local * SROW + ch_local * 2) = o;
                if (GEN && p.stat_part) {   // statistics of the values as stored (bf16); rows past M hold exact zeros
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const float v = (float)o[r];
                        st_sum[c][r] += v;
                        st_sq[c][r] += v * v;
                    }
                }
            }
        }
    };
    const float slope = p.slope;
    if (p.act == RYOLO_ACT_LEAKY) epilogue1([slope](float v) { return v > 0.f ? v : v * slope; });
    else if (p.act == RYOLO_ACT_MISH) epilogue1([](float v) { return mish(v); });
    else epilogue1([](float v) { return v; });
    if (GEN && p.stat_part) {
        // the 16 lanes of a k-group hold the same channels: DPP row sum over them leaves every total in all 16 lanes; lane
        // frow then keeps total number frow (channel fragment frow / 4, register frow % 4) and parks it in this wave row's
        // slot behind the staging tile
        static_assert(CF <= 4, "one total per lane of a 16-lane row");
        float ta = 0.f, tb = 0.f;
#pragma unroll
        for (int c = 0; c < CF; c++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float a = row16_sum(st_sum[c][r]), b = row16_sum(st_sq[c][r]);
                if (frow == c * 4 + r) {
                    ta = a;
                    tb = b;
                }
            }
        float *slot = (float *)(smem + BM * SROW) + wm * 2 * BN;
        const int ch = wn * WCH + (frow >> 2) * 16 + fk * 4 + (frow & 3);
        if (frow < CF * 4) {
            slot[ch] = ta;
            slot[BN + ch] = tb;
        }
    }
    __syncthreads();
    if (GEN && p.stat_part) {
        // the wave rows' totals are added in a fixed order (the fp32 sums stay reproducible), then ONE 64-bit atomic per
        // channel and statistic per workgroup into partial row (m_tile mod STAT_ROWS)
        static_assert(NT >= 2 * BN, "one thread per (statistic, channel)");
        if (tid < 2 * BN) {
            const float *slot = (const float *)(smem + BM * SROW);
            float v = slot[tid];
#pragma unroll
            for (int w = 1; w < WGM; w++) v += slot[w * 2 * BN + tid];
            const int st = tid / BN, ch = tid % BN;
            if (n0 + ch < p.Cout)
                atomicAdd(p.stat_part + (size_t)(m_tile % STAT_ROWS) * 2 * p.stat_cpad + (size_t)st * p.stat_cpad + n0 + ch, (double)v);
        }
    }

    // ---- epilogue 2: coalesced 16-B rows: (+ residual) -> global (optionally 2x2 replicated).
    // All residual loads of a thread are issued before any is consumed (NIT independent 16-B loads in flight).
    constexpr int CPR = BN / 8;              // 16-B chunks per staged row
    constexpr int NIT = BM * CPR / NT;       // chunks per thread
    static_assert(BM * CPR % NT == 0, "tile chunks must divide evenly over the threads");
    auto opix = [&](int m) -> size_t {
        int j, i, img;
        split_pixel(m, p.Wo, p.Ho, p.magic_wo, p.magic_ho, p.use_magic, j, i, img);
        return ((size_t)img * p.OH + (size_t)(i * p.os + p.ooy)) * p.OW + (size_t)(j * p.osx + p.oox);
    };
    bf16x8 rv[NIT];
    if (p.res) {
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int idx = it * NT + tid;
            const int m = m0 + idx / CPR, c = n0 + (idx % CPR) * 8;
            const bool ok = (m < p.M) && (c < p.Cout);
            rv[it] = *(const bf16x8 *)(ok ? p.res + ((!GEN || p.os == 1) ? (size_t)m : opix(m)) * p.res_cs + c : zero_page);
        }
    }
    static_assert(!BNRED || (NT % CPR == 0 && CPR <= 16 && !GEN && CPR == BR_CPR && NIT == BR_NIT), "a thread keeps one 8-channel chunk for all its pixels");
    float bn_sc[8], bn_sh[8], bn_mu[8], bn_is[8], bs1[8], bs2[8], bs3[8];      // (the BatchNorm constants of the thread's 8 channels: L2 hits, not held over the K loop)
    float bn_slope = 0.f;
    if constexpr (BNRED) {
        bn_slope = br.slope[0];
        const int c = n0 + (tid % CPR) * 8;
        const bool okc = c < p.Cout;                    // whole 8-channel chunks (C % 8 == 0)
        const f32x4 z4 = f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 a0 = okc ? *(const f32x4 *)(br.scale + c) : z4, a1 = okc ? *(const f32x4 *)(br.scale + c + 4) : z4;
        const f32x4 b0 = okc ? *(const f32x4 *)(br.shift + c) : z4, b1 = okc ? *(const f32x4 *)(br.shift + c + 4) : z4;
        const f32x4 u0 = okc ? *(const f32x4 *)(br.mean + c) : z4, u1 = okc ? *(const f32x4 *)(br.mean + c + 4) : z4;
        const f32x4 i0 = okc ? *(const f32x4 *)(br.invstd + c) : z4, i1 = okc ? *(const f32x4 *)(br.invstd + c + 4) : z4;   // (for the flush: its latency is not exposed there)
#pragma unroll
        for (int e = 0; e < 4; e++) {
            bn_sc[e] = a0[e]; bn_sc[4 + e] = a1[e]; bn_sh[e] = b0[e]; bn_sh[4 + e] = b1[e]; bn_mu[e] = u0[e]; bn_mu[4 + e] = u1[e];
            bn_is[e] = i0[e]; bn_is[4 + e] = i1[e];
        }
#pragma unroll
        for (int e = 0; e < 8; e++) bs1[e] = bs2[e] = bs3[e] = 0.f;
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
        if constexpr (BNRED) {       // the arithmetic of bn_act_bwd_reduce_kernel<1> (train.hip) on the value as it is stored (bf16)
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float zf = (float)zv[it][e], d = (float)v[e];
                const float u = zf * bn_sc[e] + bn_sh[e];
                float g = d;
                if (u <= 0.f) { g = d * bn_slope; bs3[e] += d * u; }
                bs2[e] += g * (zf - bn_mu[e]);
                bs1[e] += g;
            }
        }
        if (p.ups == 1 && (!GEN || p.os == 1)) {
            if (p.nt_out) __builtin_nontemporal_store(v, (bf16x8 *)(p.y + (size_t)m * p.out_cs + c));
            else *(bf16x8 *)(p.y + (size_t)m * p.out_cs + c) = v;
        } else if (p.ups == 1) {     // strided placement (stride-2 dgrad parity classes)
            if (p.nt_out) __builtin_nontemporal_store(v, (bf16x8 *)(p.y + opix(m) * p.out_cs + c));
            else *(bf16x8 *)(p.y + opix(m) * p.out_cs + c) = v;
        } else {
            int wo, ho, img;
            split_pixel(m, p.Wo, p.Ho, p.magic_wo, p.magic_ho, p.use_magic, wo, ho, img);
            const size_t W2 = (size_t)p.Wo * 2;
            const size_t o00 = (((size_t)img * p.Ho * 2 + ho * 2) * W2 + wo * 2) * p.out_cs + c;
            *(bf16x8 *)(p.y + o00) = v;
            *(bf16x8 *)(p.y + o00 + p.out_cs) = v;
            *(bf16x8 *)(p.y + o00 + W2 * p.out_cs) = v;
            *(bf16x8 *)(p.y + o00 + (W2 + 1) * p.out_cs) = v;
        }
    }
    if constexpr (BNRED) {
        // lanes cch, cch + CPR, ... of a wave hold the same channels: xor-butterfly pair sums (fixed order), then the waves' totals
        // through the slots behind the staging tile (other threads may still be reading the tile itself), summed in wave order
        const int cch = tid % CPR;
        static_assert(BM * SROW + NW * CPR * 24 * 4 <= NSTAGE * STAGE, "staging tile + reduce slots must fit in the operand buffers");
        float *slots = (float *)(smem + BM * SROW);                // [NW][CPR][24] (extra LDS would cost the second workgroup per CU)
#pragma unroll
        for (int e = 0; e < 8; e++) {
            float a = bs1[e], b = bs2[e] * bn_is[e], d = bs3[e];
            a = lane_class_sum<CPR>(a); b = lane_class_sum<CPR>(b); d = lane_class_sum<CPR>(d);
            if (lane < CPR) {
                slots[(wave * CPR + cch) * 24 + e] = a;
                slots[(wave * CPR + cch) * 24 + 8 + e] = b;
                slots[(wave * CPR + cch) * 24 + 16 + e] = d;
            }
        }
        __syncthreads();
        for (int t = tid; t < CPR * 24; t += NT) {
            const int l = t / 24, k = t % 24;
            float v = slots[l * 24 + k];
#pragma unroll
            for (int w = 1; w < NW; w++) v += slots[(w * CPR + l) * 24 + k];
            const int ch = n0 + l * 8 + (k & 7);
            if (ch < p.Cout) br.part[((size_t)m_tile * 3 + (k >> 3)) * p.Cout + ch] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------ persistent variant
// The FAST inference kernel as a PERSISTENT grid: two workgroups per CU walk a tile list (XCD-contiguous chunks), and
// the per-tile fixed cost is taken off the critical path --
//   * during the LAST K step of a tile the workgroup computes the next tile's lane bookkeeping and issues that tile's
//     first K step into the idle LDS stage buffer, so the loads fly while the epilogue runs;
//   * the residual rows of the current tile are requested before that prefetch (vector-memory results return in
//     order: the epilogue then waits for the residual only, not for the prefetch);
//   * the epilogue stages the bf16 tile in the stage buffer the last K step read (chunk-XOR swizzle instead of padding
//     so that it fits) and uses raw s_barrier + lgkmcnt waits, which leave the prefetch in flight.
// Pixel decomposition uses multiply-high by ceil(2^32/d) (exact while M*d < 2^32; checked by the host).
// STATS (training forward): every lane keeps the per-channel sums of z and z*z of the values it stored in registers
// over ALL the tiles the workgroup walks; the cross-lane sum, the LDS combine of the wave rows and the 64-bit atomics
// into partial row (workgroup mod STAT_ROWS) run once at the end (or when the channel tile changes), not per tile.
// BNRED (training backward, 1x1 data gradient): the tile this kernel stores is the FINAL gradient dy of the block whose output the
// 1x1 conv consumed (dx, after the accumulation into the shortcut chain's running gradient), so the first pass of that block's
// BatchNorm/activation backward -- per-channel sums of g = dy*act'(u), g*(z - mean)*invstd and dy*min(u, 0) over all pixels --
// runs here on the values in registers, for one extra read of z, instead of as a pass of its own over z AND dy.  Each lane owns
// the same 8 channels for every tile of a channel column and keeps the 24 sums in registers over ALL the tiles the workgroup
// walks; they are combined once per workgroup (fixed order) into row blockIdx.x of part[grid][3][C], which
// bn_act_bwd_finalize_kernel (train.hip) reduces exactly like the slab rows of the stand-alone pass.
template <int KS, int BM, int BN, int WGM, int WGN, bool STATS, bool BNRED = false>
__global__ void __launch_bounds__(WGM *WGN * 64, 2) conv_igemm_persist_kernel(const ConvParams p, const BnRed br = BnRed()) {
    constexpr int NW = WGM * WGN, NT = NW * 64;
    constexpr int WPIX = BM / WGM, WCH = BN / WGN, PF = WPIX / 16, CF = WCH / 16;
    constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE = A_BYTES + B_BYTES;
    constexpr int A_PPW = (BM / 8) / NW, B_PPW = (BN / 8) / NW;
    constexpr int CPR = BN / 8, NIT = BM * CPR / NT, SROW = BN * 2;
    static_assert(A_PPW >= 1 && B_PPW >= 1, "tile too small for the wave count");
    static_assert(BM * SROW <= STAGE, "the staging tile must fit in one stage buffer");
    static_assert(BM * CPR % NT == 0, "tile chunks must divide evenly over the threads");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // this workgroup's tile list: XCD x (= blockIdx & 7) owns the x-th contiguous chunk of tile ids
    const int T = p.ntiles, G = gridDim.x;
    const int q = T >> 3, r = T & 7, xcd = blockIdx.x & 7, loc = blockIdx.x >> 3, nloc = G >> 3;
    const int start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    const int len = q + (xcd < r ? 1 : 0);
    if constexpr (BNRED) {       // this workgroup's row of partial sums starts at zero (flush_bn adds: a row may be flushed per channel column)
        for (int t = tid; t < 3 * p.Cout; t += NT) br.part[(size_t)blockIdx.x * 3 * p.Cout + t] = 0.f;
    }
    if (loc >= len) return;

    int a_off32[A_PPW], b_off32[B_PPW];
    unsigned a_mask[A_PPW];
    unsigned a_tapsel = 0;       // taps2: bit j = which of the K step's two taps piece j of this lane stages
    int f_tap = 0, f_c0 = 0, f_kh = 0, f_kw = 0;
    int nm0 = 0, nn0 = 0;
    auto setup = [&](int id) {
        const int m_tile = udiv_magic(id, p.magic_nt);
        const int n_tile = id - m_tile * p.nt;
        nm0 = m_tile * BM;
        nn0 = n_tile * BN;
#pragma unroll
        for (int j = 0; j < A_PPW; j++) {
            const int row = (wave * A_PPW + j) * 8 + (lane >> 3);
            const int slot = (lane & 7) ^ ((row >> 1) & 7);
            const int m = nm0 + row;
            const int t = udiv_magic(m, p.magic_wo);
            const int wo = m - t * p.Wo;
            const int img = udiv_magic(t, p.magic_ho);
            const int ho = t - img * p.Ho;
            const int hi0 = ho * p.stride - p.pad, wi0 = wo * p.stride - p.pad;
            // taps2 (3x3, C_in == 32: one K step = two taps): the slot's low 2 bits pick the channels, bit 2 picks the tap
            a_off32[j] = (((img * p.H + hi0) * p.W + wi0) * p.in_cs) * 2 + ((KS == 3 && p.taps2) ? (slot & 3) : slot) * 16;
            if (KS == 3) a_tapsel = (a_tapsel & ~(1u << j)) | ((unsigned)(slot >> 2) << j);
            unsigned rb = 0, cb = 0;
#pragma unroll
            for (int k = 0; k < KS; k++) {
                rb |= ((unsigned)(hi0 + k) < (unsigned)p.H ? 1u : 0u) << k;
                cb |= ((unsigned)(wi0 + k) < (unsigned)p.W ? 1u : 0u) << k;
            }
            unsigned mk = 0;
#pragma unroll
            for (int k = 0; k < KS; k++) mk |= ((rb >> k) & 1u) ? (cb << (k * KS)) : 0u;
            a_mask[j] = m < p.M ? mk : 0u;
        }
#pragma unroll
        for (int j = 0; j < B_PPW; j++) {
            const int row = (wave * B_PPW + j) * 8 + (lane >> 3);
            const int slot = (lane & 7) ^ ((row >> 1) & 7);
            b_off32[j] = ((nn0 + row) * p.Kpad + slot * 8) * 2;
        }
        f_tap = f_c0 = f_kh = f_kw = 0;
    };

    // live = false: the same instructions with every lane out of range (zeros to LDS, no memory traffic) -- keeps the
    // instruction stream, and with it the compiler's vmcnt bookkeeping, identical whether or not a next tile exists
    auto stage = [&](int kt, int buf, bool live) {
        char *abuf = smem + buf * STAGE;
        char *bbuf = abuf + A_BYTES;
        if (KS == 3 && p.taps2) {
            // C_in == 32: K step kt = taps 2kt and 2kt+1 of the 3x3 window (tap 9 = K padding: its mask bit is 0)
            const int t0 = 2 * kt, t1 = 2 * kt + 1;
            const int kh0 = (t0 * 11) >> 5, kw0 = t0 - 3 * kh0, kh1 = (t1 * 11) >> 5, kw1 = t1 - 3 * kh1;
            const int off0 = ((kh0 * p.W + kw0) * p.in_cs) * 2, off1 = ((kh1 * p.W + kw1) * p.in_cs) * 2;
#pragma unroll
            for (int j = 0; j < A_PPW; j++) {
                const unsigned hi = (a_tapsel >> j) & 1u;
                const bool ok = ((a_mask[j] >> (t0 + hi)) & 1u) && live;
                const int voff = ok ? a_off32[j] + (hi ? off1 : off0) : (int)0x80000000;
                buffer_load_lds16(p.x, p.x_bytes, abuf + (wave * A_PPW + j) * 1024, voff, 0);
            }
#pragma unroll
            for (int j = 0; j < B_PPW; j++)
                buffer_load_lds16(p.w, p.w_bytes, bbuf + (wave * B_PPW + j) * 1024, live ? b_off32[j] : (int)0x80000000,
                                  kt * (BK * 2));
            return;
        }
        const int tapoff = ((f_kh * p.W + f_kw) * p.in_cs + f_c0) * 2;   // scalar
#pragma unroll
        for (int j = 0; j < A_PPW; j++) {
            const bool ok = ((a_mask[j] >> f_tap) & 1u) && live;
            const int voff = ok ? a_off32[j] + tapoff : (int)0x80000000;
            buffer_load_lds16(p.x, p.x_bytes, abuf + (wave * A_PPW + j) * 1024, voff, 0);
        }
#pragma unroll
        for (int j = 0; j < B_PPW; j++)
            buffer_load_lds16(p.w, p.w_bytes, bbuf + (wave * B_PPW + j) * 1024, live ? b_off32[j] : (int)0x80000000,
                              kt * (BK * 2));
        f_c0 += BK;
        if (f_c0 >= p.Cin) {
            f_c0 = 0;
            f_tap++;
            if (++f_kw == KS) { f_kw = 0; f_kh++; }
        }
    };

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
        for (int ks = 0; ks < 2; ks++) b_off[f][ks] = A_BYTES + row * 128 + (((ks * 4 + fk) ^ ((row >> 1) & 7)) << 4);
    }

    const __bf16 *zero_page = p.w + (size_t)(((p.Cout + 127) >> 7) << 7) * p.Kpad;
    const int KT = p.Kpad / BK;
    const float slope = p.slope;
    f32x4 acc[CF][PF];

    int i = loc;
    setup(start + i);
    int m0 = nm0, n0 = nn0;
    int buf = 0;
    stage(0, buf, true);
    // folded-BN scale / shift of this lane's output channels: reloaded only when the channel tile changes (never when
    // the XCD's workgroup count is a multiple of nt, i.e. for every power-of-two nt)
    f32x4 ep_sc[CF], ep_sh[CF];
    auto load_scale_shift = [&]() {
#pragma unroll
        for (int c = 0; c < CF; c++) {
            const int ch_local = wn * WCH + c * 16 + fk * 4;
            ep_sc[c] = *(const f32x4 *)(p.scale + n0 + ch_local);
            ep_sh[c] = *(const f32x4 *)(p.shift + n0 + ch_local);
        }
    };
    load_scale_shift();
    float st_sum[CF][4], st_sq[CF][4];
#pragma unroll
    for (int c = 0; c < CF; c++)
#pragma unroll
        for (int r = 0; r < 4; r++) st_sum[c][r] = st_sq[c][r] = 0.f;
    auto flush_stats = [&]() {    // workgroup-uniform call sites only
        static_assert(!STATS || (CF <= 4 && NT >= 2 * BN), "one total per lane of a 16-lane row; one thread per (statistic, channel)");
        float ta = 0.f, tb = 0.f;
#pragma unroll
        for (int c = 0; c < CF; c++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float a = row16_sum(st_sum[c][r]), b = row16_sum(st_sq[c][r]);
                if (frow == c * 4 + r) {
                    ta = a;
                    tb = b;
                }
                st_sum[c][r] = st_sq[c][r] = 0.f;
            }
        float *slots = (float *)(smem + 2 * STAGE);            // [WGM][2][BN], behind the two stage buffers
        const int ch = wn * WCH + (frow >> 2) * 16 + fk * 4 + (frow & 3);
        if (frow < CF * 4) {
            slots[wm * 2 * BN + ch] = ta;
            slots[wm * 2 * BN + BN + ch] = tb;
        }
        __syncthreads();
        if (tid < 2 * BN) {
            float v = slots[tid];
#pragma unroll
            for (int w = 1; w < WGM; w++) v += slots[w * 2 * BN + tid];     // fixed order: reproducible fp32 sums
            const int st = tid / BN, c = tid % BN;
            if (n0 + c < p.Cout)
                atomicAdd(p.stat_part + ((size_t)(blockIdx.x % STAT_ROWS) * 2 + st) * p.stat_cpad + n0 + c, (double)v);
        }
        __syncthreads();
    };
    // ---- BNRED state: this lane's 8 channels are n0 + (tid % CPR) * 8 .. + 7 in every tile of the channel column
    static_assert(!BNRED || (NT % CPR == 0 && CPR == 16 && !STATS), "a lane keeps one 8-channel chunk; 4 lanes of a wave share it");
    float bs1[8], bs2[8], bs3[8];                       // the only BNRED state that lives across the K loops (24 registers)
#pragma unroll
    for (int e = 0; e < 8; e++) bs1[e] = bs2[e] = bs3[e] = 0.f;
    const float bn_slope = BNRED ? br.slope[0] : 0.f;
    auto flush_bn = [&]() {        // workgroup-uniform call sites only
        if constexpr (BNRED) {
            const int cch = tid % CPR, c = n0 + cch * 8;
            float *slots = (float *)(smem + 2 * STAGE);        // [NW][CPR][24]
#pragma unroll
            for (int e = 0; e < 8; e++) {
                float a = bs1[e], b = bs2[e] * (c + e < p.Cout ? br.invstd[c + e] : 0.f), d = bs3[e];
                // lanes cch, cch + 16, cch + 32, cch + 48 of a wave hold the same channels: fixed-order pair sums
                a += __shfl_xor(a, 16); b += __shfl_xor(b, 16); d += __shfl_xor(d, 16);
                a += __shfl_xor(a, 32); b += __shfl_xor(b, 32); d += __shfl_xor(d, 32);
                if (lane < CPR) {
                    slots[(wave * CPR + cch) * 24 + e] = a;
                    slots[(wave * CPR + cch) * 24 + 8 + e] = b;
                    slots[(wave * CPR + cch) * 24 + 16 + e] = d;
                }
                bs1[e] = bs2[e] = bs3[e] = 0.f;
            }
            __syncthreads();
            for (int t = tid; t < CPR * 24; t += NT) {
                const int l = t / 24, k = t % 24;
                float v = slots[l * 24 + k];
#pragma unroll
                for (int w = 1; w < NW; w++) v += slots[(w * CPR + l) * 24 + k];      // fixed order
                const int ch = n0 + l * 8 + (k & 7);
                if (ch < p.Cout) br.part[((size_t)blockIdx.x * 3 + (k >> 3)) * p.Cout + ch] += v;   // row owned by this workgroup
            }
            __syncthreads();
        }
    };
    while (true) {
        const int inext = i + nloc;
        const bool has_next = inext < len;
#pragma unroll
        for (int c = 0; c < CF; c++)
#pragma unroll
            for (int f = 0; f < PF; f++) acc[c][f] = f32x4{0.f, 0.f, 0.f, 0.f};
        auto compute = [&](int cb) {
            const char *sb = smem + cb * STAGE;
#pragma unroll
            for (int ks = 0; ks < 2; ks++) {
                bf16x8 wf[CF], xf[PF];
#pragma unroll
                for (int c = 0; c < CF; c++) wf[c] = *(const bf16x8 *)(sb + b_off[c][ks]);
#pragma unroll
                for (int f = 0; f < PF; f++) xf[f] = *(const bf16x8 *)(sb + a_off[f][ks]);
#pragma unroll
                for (int c = 0; c < CF; c++)
#pragma unroll
                    for (int f = 0; f < PF; f++)
                        acc[c][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[c], xf[f], acc[c][f], 0, 0, 0);
            }
        };
        for (int kt = 0; kt + 1 < KT; kt++) {
            // tile step kt landed (explicit vmcnt(0): the compiler's own count does not reliably cover direct-to-LDS
            // loads across the loop back edge); nobody still reads the buffer overwritten next
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            stage(kt + 1, buf ^ 1, true);
            compute(buf);
            buf ^= 1;
        }
        // last K step (peeled): residual request, then the next tile's bookkeeping and first K step, then the MFMAs
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        bf16x8 rv[NIT];
        const bool has_res = !STATS && p.res;      // the statistics instantiation has no residual operand (registers)
        if (has_res) {
#pragma unroll
            for (int it = 0; it < NIT; it++) {
                const int idx = it * NT + tid;
                const int m = m0 + idx / CPR, c = n0 + (idx % CPR) * 8;
                const bool ok = (m < p.M) && (c < p.Cout);
                rv[it] = *(const bf16x8 *)(ok ? p.res + (size_t)m * p.res_cs + c : zero_page);
            }
        }
        setup(start + (has_next ? inext : i));
        stage(0, buf ^ 1, has_next);
        compute(buf);
        buf ^= 1;
        // the last K step read buffer buf^1: it becomes the staging tile; buffer `buf` receives the next tile's step 0
        char *st = smem + (buf ^ 1) * STAGE;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        auto epilogue1 = [&](auto actfn) {
#pragma unroll
            for (int c = 0; c < CF; c++) {
                const int ch_local = wn * WCH + c * 16 + fk * 4;
                const f32x4 sc = ep_sc[c], sh = ep_sh[c];
#pragma unroll
                for (int f = 0; f < PF; f++) {
                    const int pix_local = wm * WPIX + f * 16 + frow;
                    bf16x4 o;
#pragma unroll
                    for (int rr = 0; rr < 4; rr++) o[rr] = (__bf16)actfn(acc[c][f][rr] * sc[rr] + sh[rr]);
                    *(bf16x4 *)(st + pix_local * SROW + (((ch_local >> 3) ^ (pix_local & (CPR - 1))) << 4) + (fk & 1) * 8) = o;
                    if constexpr (STATS) {     // statistics of the values as stored (bf16); rows past M hold exact zeros
#pragma unroll
                        for (int rr = 0; rr < 4; rr++) {
                            const float q = (float)o[rr];
                            st_sum[c][rr] += q;
                            st_sq[c][rr] += q * q;
                        }
                    }
                }
            }
        };
        if (p.act == RYOLO_ACT_LEAKY) epilogue1([slope](float v) { return v > 0.f ? v : v * slope; });
        else if (p.act == RYOLO_ACT_MISH) epilogue1([](float v) { return mish(v); });
        else epilogue1([](float v) { return v; });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        bf16x8 zv[BNRED ? NIT : 1];
        float bn_sc[8], bn_sh[8], bn_mu[8];
        if constexpr (BNRED) {       // the consumer block's z for this lane's chunks (the accumulators are dead: registers are free)
            {   // and its BatchNorm constants for the lane's 8 channels: re-read per tile (L1/L2 hits) rather than held over the K loop
                const int c = n0 + (tid % CPR) * 8;
                const bool ok = c < p.Cout;             // whole 8-channel chunks (C % 8 == 0)
                const f32x4 z4 = f32x4{0.f, 0.f, 0.f, 0.f};
                const f32x4 a0 = ok ? *(const f32x4 *)(br.scale + c) : z4, a1 = ok ? *(const f32x4 *)(br.scale + c + 4) : z4;
                const f32x4 b0 = ok ? *(const f32x4 *)(br.shift + c) : z4, b1 = ok ? *(const f32x4 *)(br.shift + c + 4) : z4;
                const f32x4 m0_ = ok ? *(const f32x4 *)(br.mean + c) : z4, m1_ = ok ? *(const f32x4 *)(br.mean + c + 4) : z4;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    bn_sc[e] = a0[e]; bn_sc[4 + e] = a1[e]; bn_sh[e] = b0[e]; bn_sh[4 + e] = b1[e]; bn_mu[e] = m0_[e]; bn_mu[4 + e] = m1_[e];
                }
            }
#pragma unroll
            for (int it = 0; it < NIT; it++) {
                const int idx = it * NT + tid;
                const int m = m0 + idx / CPR, c = n0 + (idx % CPR) * 8;
                const bool ok = (m < p.M) && (c < p.Cout);
                zv[it] = *(const bf16x8 *)(ok ? br.z + (size_t)m * br.z_cs + c : zero_page);
            }
        }
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int idx = it * NT + tid;
            const int pix = idx / CPR, cch = idx % CPR;
            const int m = m0 + pix, c = n0 + cch * 8;
            if (m >= p.M || c >= p.Cout) continue;
            bf16x8 v = *(const bf16x8 *)(st + pix * SROW + ((cch ^ (pix & (CPR - 1))) << 4));
            if (has_res) {
#pragma unroll
                for (int e = 0; e < 8; e++) v[e] = (__bf16)((float)v[e] + (float)rv[it][e]);
            }
            if constexpr (BNRED) {   // the arithmetic of bn_act_bwd_reduce_kernel<1> on the value as it is stored (bf16)
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const float zf = (float)zv[it][e], d = (float)v[e];
                    const float u = zf * bn_sc[e] + bn_sh[e];
                    float g = d;
                    if (u <= 0.f) { g = d * bn_slope; bs3[e] += d * u; }
                    bs2[e] += g * (zf - bn_mu[e]);
                    bs1[e] += g;
                }
            }
            if (p.ups == 1) {
                if (p.nt_out) __builtin_nontemporal_store(v, (bf16x8 *)(p.y + (size_t)m * p.out_cs + c));
                else *(bf16x8 *)(p.y + (size_t)m * p.out_cs + c) = v;
            } else {
                const int t = udiv_magic(m, p.magic_wo);
                const int wo = m - t * p.Wo;
                const int img = udiv_magic(t, p.magic_ho);
                const int ho = t - img * p.Ho;
                const size_t W2 = (size_t)p.Wo * 2;
                const size_t o00 = (((size_t)img * p.Ho * 2 + ho * 2) * W2 + wo * 2) * p.out_cs + c;
                *(bf16x8 *)(p.y + o00) = v;
                *(bf16x8 *)(p.y + o00 + p.out_cs) = v;
                *(bf16x8 *)(p.y + o00 + W2 * p.out_cs) = v;
                *(bf16x8 *)(p.y + o00 + (W2 + 1) * p.out_cs) = v;
            }
        }
        if (!has_next) break;
        i = inext;
        m0 = nm0;
        if (nn0 != n0) {
            if constexpr (STATS) flush_stats();
            flush_bn();
            n0 = nn0;
            load_scale_shift();
        }
    }
    if constexpr (STATS) flush_stats();
    flush_bn();
}


// ------------------------------------------------------------------------------------------------ first layer, direct
// 3x3 / stride 1 / pad 1 on the 8-channel (3 real) NHWC input -> 32 channels (Darknet-53 layer 0: 11.8 M pixels per bs-32
// batch, 0.95 GB of algorithmic traffic, HBM-bound).  K = 9 taps x 8 channels: the 16 bytes one lane needs for a B
// fragment (8 consecutive k of one pixel) are exactly the 8 channels of ONE tap of ONE input pixel, i.e. one aligned
// 16-B load -- so the fragments are loaded straight from global memory (L1/L2 serve the 9x tap re-reads), no LDS, no
// barrier, and the weights (72 x 32) live in registers for the whole kernel.  A wave walks groups of 16 consecutive output
// pixels: 3 loads, 6 MFMAs (2 channel fragments x 3 k-substeps of 32 = taps 0-3, 4-7, 8 + zeros), 1 store.
// The walk is software-pipelined and branch-free: the next group's three fragments are requested (buffer loads; padding,
// K-padding taps and the M tail are out-of-range offsets = hardware zeros) before the current group's MFMAs, the pixel
// coordinates advance incrementally (one division per wave, W_o >= 16), the activation is a template parameter, and the
// lane regrouping for the 64-B row store is two v_permlane16_swap.  (The first version branched per element on the
// activation, per load on the padding test and waited vmcnt(0) in front of its MFMAs: 2.5 TB/s.)
// Training of layer 0 WITHOUT its conv output (MODE 1..3).  z0 = conv(x) is 4 x the size of x (8 padded channels in, 32 out: 1.5 GB
// against 0.38 GB at bs 64) and costs 27 MACs per value, so it is cheaper to recompute it than to store and re-read it:
//   MODE 1  statistics only (sums of z, z^2 of the bf16-rounded values, nothing stored)         -> ryolo_bn_finalize
//   MODE 0  y = act(z * scale + shift) with the batch statistics folded in = the inference epilogue (no STATS)
//   MODE 2  backward reduce: recompute z, read dy, per-channel sums of g = dy * act'(u), g * (z - mean), dy * min(u, 0)
//   MODE 3  backward apply:  recompute z, read dy, write dz = scale * g + kb * z + kd  (kb, kd from the sums; bn_act_bwd_apply's form)
// Same recomputed bits as the stored z would hold (same MFMAs, same bf16 rounding); per step 4.9 GB less traffic than
// conv -> z, bn_act_fwd(z), bn_act_bwd(z, dy) (tools/step_ab.py).
struct C8Bwd {
    const __bf16 *dy = nullptr; int dy_cs = 0;   // gradient of the block output, NHWC
    const float *mean = nullptr;             // [32]
    const float *kb = nullptr, *kd = nullptr;    // MODE 3: per-channel constants
    const float *slope = nullptr;            // device scalar (a learnable PReLU slope) or nullptr: ConvParams::slope
    double *part = nullptr;                  // MODE 2: [STAT_ROWS][3][32] partial sums (fp64 atomics), zeroed by the caller
    unsigned dy_bytes = 0;
    int round_z = 0;                         // MODE 0 of the training engine: BatchNorm is applied to z ROUNDED to bf16, as if it had been stored
};

template <bool STATS, int ACT, int MODE = 0>   // STATS: also the per-channel sums of z and z^2 (BatchNorm batch statistics), like the GEN epilogue
__global__ void __launch_bounds__(256) conv3x3_c8_direct_kernel(const ConvParams p, int groups_per_wave, const C8Bwd bw = C8Bwd()) {
    const int lane = threadIdx.x & 63;
    const int fr = lane & 15, g = lane >> 4;
    const long long wave_id = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long g0 = wave_id * groups_per_wave;
    if (g0 * 16 >= p.M) return;                                   // wave-uniform
    const int n_it = (int)(((long long)p.M - g0 * 16 + 15) / 16 < groups_per_wave ? ((long long)p.M - g0 * 16 + 15) / 16 : groups_per_wave);
    bf16x8 wfr[2][3];
#pragma unroll
    for (int cf = 0; cf < 2; cf++)
#pragma unroll
        for (int ks = 0; ks < 3; ks++)
            wfr[cf][ks] = *(const bf16x8 *)(p.w + (size_t)(cf * 16 + fr) * p.Kpad + ks * 32 + g * 8);
    f32x4 sc[2], sh[2];
#pragma unroll
    for (int cf = 0; cf < 2; cf++) {
        sc[cf] = *(const f32x4 *)(p.scale + cf * 16 + g * 4);
        sh[cf] = *(const f32x4 *)(p.shift + cf * 16 + g * 4);
    }
    const float slope = bw.slope ? bw.slope[0] : p.slope;
#if defined(__HIP_DEVICE_COMPILE__)
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16 *>(p.x), 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, p.w_bytes, 0x00020000);   // w_bytes: bytes of y here
    const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16 *>(MODE >= 2 ? bw.dy : p.x), 0, MODE >= 2 ? bw.dy_bytes : 0u, 0x00020000);
#endif
    // backward modes: this lane's per-channel constants (channels cf*16 + 4g .. +3) and sums
    f32x4 mu[2], kbv[2], kdv[2];
    float b1[2][4], b2[2][4], b3[2][4];
    if constexpr (MODE >= 2) {
#pragma unroll
        for (int cf = 0; cf < 2; cf++) {
            mu[cf] = *(const f32x4 *)(bw.mean + cf * 16 + g * 4);
            if constexpr (MODE == 3) {
                kbv[cf] = *(const f32x4 *)(bw.kb + cf * 16 + g * 4);
                kdv[cf] = *(const f32x4 *)(bw.kd + cf * 16 + g * 4);
            }
#pragma unroll
            for (int r = 0; r < 4; r++) b1[cf][r] = b2[cf][r] = b3[cf][r] = 0.f;
        }
    }
    // lane-constant tap geometry of the three k-substeps: tap = 4 ks + g (taps >= 9 are K padding)
    int dkh[3], dkw[3];
    bool tok[3];
#pragma unroll
    for (int ks = 0; ks < 3; ks++) {
        const int tap = ks * 4 + g;
        dkh[ks] = ((tap * 11) >> 5) - 1;
        dkw[ks] = tap - 3 * ((tap * 11) >> 5) - 1;
        tok[ks] = tap < 9;
    }
    float st_sum[2][4], st_sq[2][4];                             // this lane's 8 channels over all its pixels
#pragma unroll
    for (int cf = 0; cf < 2; cf++)
#pragma unroll
        for (int r = 0; r < 4; r++) st_sum[cf][r] = st_sq[cf][r] = 0.f;
    // this lane's pixel of the wave's first group (clamped into range for the coordinate split; the tail is masked by m < M)
    int m = (int)(g0 * 16) + fr;
    int wo, ho, img;
    {
        const int mc = m < p.M ? m : p.M - 1;
        const int t = mc / p.Wo;
        wo = mc - t * p.Wo;
        img = t / p.Ho;
        ho = t - img * p.Ho;
    }
    typedef __attribute__((ext_vector_type(4))) unsigned int u4;
    typedef __attribute__((ext_vector_type(2))) unsigned int u2;
    auto request_dy = [&](u2(&d)[2], int mcur, bool live) {        // backward modes: dy of this lane's 8 channels of pixel mcur
        if constexpr (MODE >= 2) {
#pragma unroll
            for (int cf = 0; cf < 2; cf++) {
                const int off = (mcur * bw.dy_cs + cf * 16 + g * 4) * 2;
#if defined(__HIP_DEVICE_COMPILE__)
                d[cf] = __builtin_amdgcn_raw_buffer_load_b64(drs, (live && mcur < p.M) ? off : (int)0x80000000, 0, 0);
#endif
            }
        }
    };
    auto request = [&](u4(&x)[3], bool live) {                    // the three fragments of pixel (img, ho, wo)
#pragma unroll
        for (int ks = 0; ks < 3; ks++) {
            const int hi = ho + dkh[ks], wi = wo + dkw[ks];
            const bool ok = live && tok[ks] && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
            const int off = ((img * p.H + hi) * p.W + wi) * 16;
#if defined(__HIP_DEVICE_COMPILE__)
            x[ks] = __builtin_amdgcn_raw_buffer_load_b128(xrs, ok ? off : (int)0x80000000, 0, 0);
#endif
        }
    };
    auto advance = [&]() {                                        // +16 pixels (W_o >= 16: at most one row wrap)
        m += 16;
        wo += 16;
        const bool wrap = wo >= p.Wo;
        wo -= wrap ? p.Wo : 0;
        ho += wrap ? 1 : 0;
        const bool wrap2 = ho >= p.Ho;
        ho = wrap2 ? 0 : ho;
        img += wrap2 ? 1 : 0;
    };
    auto finish = [&](const u4(&x)[3], const u2(&dyv)[2], int mcur, bool live) {     // MFMAs + epilogue + store of the group whose fragments are x
        f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < 3; ks++)
#pragma unroll
            for (int cf = 0; cf < 2; cf++)
                acc[cf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr[cf][ks], __builtin_bit_cast(bf16x8, x[ks]), acc[cf], 0, 0, 0);
        const bool mok = live && mcur < p.M;
        unsigned o2[2][2];
        if constexpr (MODE >= 2) {
            // z as the forward stored it (bf16), u = z * scale + shift, g = dy * act'(u)
#pragma unroll
            for (int cf = 0; cf < 2; cf++) {
                const bf16x4 dq = __builtin_bit_cast(bf16x4, dyv[cf]);
                bf16x4 o;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float zf = (float)(__bf16)acc[cf][r];
                    const float d = (float)dq[r];
                    const float u = zf * sc[cf][r] + sh[cf][r];
                    float gg = d;
                    if constexpr (ACT == RYOLO_ACT_LEAKY) {
                        if (u <= 0.f) {
                            gg = d * slope;
                            if (MODE == 2 && mok) b3[cf][r] += d * u;
                        }
                    } else if constexpr (ACT == RYOLO_ACT_MISH) {
                        const float e = __expf(fminf(u, 20.f)), n1 = (1.f + e) * (1.f + e), t = (n1 - 1.f) / (n1 + 1.f);
                        gg = d * (t + u * (1.f - t * t) * (e / (1.f + e)));
                    }
                    if constexpr (MODE == 2) {
                        if (mok) {
                            b1[cf][r] += gg;
                            b2[cf][r] += gg * (zf - mu[cf][r]);
                        }
                    } else {
                        o[r] = (__bf16)(sc[cf][r] * gg + (kbv[cf][r] * zf + kdv[cf][r]));
                    }
                }
                if constexpr (MODE == 3) {
                    const uint2 u_ = __builtin_bit_cast(uint2, o);
                    o2[cf][0] = u_.x;
                    o2[cf][1] = u_.y;
                }
            }
            if constexpr (MODE == 2) return;
        } else {
#pragma unroll
        for (int cf = 0; cf < 2; cf++) {
            bf16x4 o;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float a_ = (MODE == 0 && bw.round_z) ? (float)(__bf16)acc[cf][r] : acc[cf][r];
                float v = a_ * sc[cf][r] + sh[cf][r];
                if constexpr (ACT == RYOLO_ACT_LEAKY) v = v > 0.f ? v : v * slope;
                else if constexpr (ACT == RYOLO_ACT_MISH) v = mish(v);
                o[r] = (__bf16)v;
                if (STATS) {                                     // statistics of the values as stored (bf16)
                    const float q = mok ? (float)o[r] : 0.f;
                    st_sum[cf][r] += q;
                    st_sq[cf][r] += q * q;
                }
            }
            const uint2 u = __builtin_bit_cast(uint2, o);
            o2[cf][0] = u.x;
            o2[cf][1] = u.y;
        }
        }
        if constexpr (MODE == 1) return;                           // statistics only: nothing is stored
        // each lane holds channels 4g..4g+3 of both channel fragments; the odd rows of fragment 0 trade places with the even
        // rows of fragment 1, after which every lane owns ONE 16-B run (even g: channels 8(g/2).. of fragment 0, odd g: of
        // fragment 1) and the four lanes of a pixel cover its 64-B row
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
        for (int d = 0; d < 2; d++) {
            auto sw = __builtin_amdgcn_permlane16_swap(o2[0][d], o2[1][d], false, false);
            o2[0][d] = sw[0];
            o2[1][d] = sw[1];
        }
        const u4 out = u4{o2[0][0], o2[0][1], o2[1][0], o2[1][1]};
        const int voff = mok ? (mcur * p.out_cs + ((g & 1) ? 16 : 0) + (g >> 1) * 8) * 2 : (int)0x80000000;
        if (p.nt_out) __builtin_amdgcn_raw_buffer_store_b128(out, yrs, voff, 0, 2);      // non-temporal
        else __builtin_amdgcn_raw_buffer_store_b128(out, yrs, voff, 0, 0);
#endif
    };
    u4 xa[3], xb[3];
    u2 da[2], db[2];
    request(xa, true);
    request_dy(da, m, true);
    for (int it = 0; it < n_it; it += 2) {
        const int m_a = m;
        advance();
        request(xb, it + 1 < n_it);
        request_dy(db, m, it + 1 < n_it);
        finish(xa, da, m_a, true);
        const int m_b = m;
        advance();
        request(xa, it + 2 < n_it);
        request_dy(da, m, it + 2 < n_it);
        finish(xb, db, m_b, it + 1 < n_it);
    }
    if constexpr (MODE == 2) {
        // 16-lane DPP row sums; lane fr < 8 keeps the totals of (fragment fr / 4, register fr % 4) and adds them to the partial row
        float t1 = 0.f, t2 = 0.f, t3 = 0.f;
#pragma unroll
        for (int cf = 0; cf < 2; cf++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float a1 = row16_sum(b1[cf][r]), a2 = row16_sum(b2[cf][r]), a3 = row16_sum(b3[cf][r]);
                if (fr == cf * 4 + r) {
                    t1 = a1;
                    t2 = a2;
                    t3 = a3;
                }
            }
        if (fr < 8) {
            const int ch = (fr >> 2) * 16 + g * 4 + (fr & 3);
            double *row = bw.part + (size_t)(wave_id % STAT_ROWS) * 3 * 32;
            atomicAdd(row + ch, (double)t1);
            atomicAdd(row + 32 + ch, (double)t2);
            atomicAdd(row + 64 + ch, (double)t3);
        }
        return;
    }
    if (STATS) {
        // the 16 lanes of a k-group hold the same channels: DPP row sum over them, lane fr keeps total number fr (fragment
        // fr / 4, register fr % 4), one atomic instruction per statistic into partial row (wave id mod STAT_ROWS)
        float ta = 0.f, tb = 0.f;
#pragma unroll
        for (int cf = 0; cf < 2; cf++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float a = row16_sum(st_sum[cf][r]), b = row16_sum(st_sq[cf][r]);
                if (fr == cf * 4 + r) {
                    ta = a;
                    tb = b;
                }
            }
        if (fr < 8) {
            const int ch = (fr >> 2) * 16 + g * 4 + (fr & 3);
            double *row = p.stat_part + (size_t)(wave_id % STAT_ROWS) * 2 * p.stat_cpad;
            atomicAdd(row + ch, (double)ta);
            atomicAdd(row + p.stat_cpad + ch, (double)tb);
        }
    }
}

// layer-0 backward, between the reduce and the apply pass: partial rows -> s1, s2 (x invstd), dgamma += s2, dbeta += s1, the
// slope gradient (one scalar: fixed-order sum over the 32 channels), and the apply pass's per-channel constants
// kb = -scale * invstd * s2 / M, kd = -kb * mean - scale * s1 / M.  One block of 32 threads; re-zeroes the partial rows.
__global__ void conv0_bwd_finalize_kernel(double *__restrict__ part, const float *__restrict__ scale, const float *__restrict__ mean,
                                          const float *__restrict__ invstd, float inv_count, float *__restrict__ kb, float *__restrict__ kd,
                                          float *__restrict__ dgamma, float *__restrict__ dbeta, float *__restrict__ dslope) {
    const int c = threadIdx.x;            // 32 threads
    double a = 0.0, b = 0.0, d = 0.0;
    for (int r = 0; r < STAT_ROWS; r++) {
        double *row = part + (size_t)r * 96;
        a += row[c]; b += row[32 + c]; d += row[64 + c];
        row[c] = 0.0; row[32 + c] = 0.0; row[64 + c] = 0.0;
    }
    const float s1 = (float)a, s2 = (float)b * invstd[c];
    if (dgamma) dgamma[c] += s2;
    if (dbeta) dbeta[c] += s1;
    const float k = scale[c] * invstd[c] * s2 * inv_count;
    kb[c] = -k;
    kd[c] = k * mean[c] - scale[c] * s1 * inv_count;
    if (dslope) {
        float v = (float)d;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 32);
        if (c == 0) dslope[0] += v;
    }
}

template <int ACT>
static int launch_c8_bwd(ConvParams &p, int gpw, unsigned nblk, const C8Bwd &bw, int mode, hipStream_t stream) {
    if (mode == 0) return launch_kernel<conv3x3_c8_direct_kernel<false, ACT, 0>>(dim3(nblk), dim3(256), 0, stream, p, gpw, bw);
    if (mode == 2) return launch_kernel<conv3x3_c8_direct_kernel<false, ACT, 2>>(dim3(nblk), dim3(256), 0, stream, p, gpw, bw);
    return launch_kernel<conv3x3_c8_direct_kernel<false, ACT, 3>>(dim3(nblk), dim3(256), 0, stream, p, gpw, bw);
}
// mode 0: the training forward (round_z), 2 / 3: the two backward passes
static int launch_c8_mode(int act, ConvParams &p, int gpw, unsigned nblk, const C8Bwd &bw, int mode, hipStream_t stream) {
    if (act == RYOLO_ACT_LEAKY) return launch_c8_bwd<RYOLO_ACT_LEAKY>(p, gpw, nblk, bw, mode, stream);
    if (act == RYOLO_ACT_MISH) return launch_c8_bwd<RYOLO_ACT_MISH>(p, gpw, nblk, bw, mode, stream);
    return launch_c8_bwd<RYOLO_ACT_LINEAR>(p, gpw, nblk, bw, mode, stream);
}

template <bool STATS>
int launch_c8_direct(ConvParams &p, int gpw, unsigned nblk, hipStream_t stream) {
    const dim3 g(nblk), b(256);
    if (STATS && p.y == nullptr)          // statistics only (layer 0 of the training engine: z is recomputed, never stored)
        return launch_kernel<conv3x3_c8_direct_kernel<true, RYOLO_ACT_LINEAR, 1>>(g, b, 0, stream, p, gpw, C8Bwd());
    if (p.act == RYOLO_ACT_LEAKY) return launch_kernel<conv3x3_c8_direct_kernel<STATS, RYOLO_ACT_LEAKY>>(g, b, 0, stream, p, gpw, C8Bwd());
    if (p.act == RYOLO_ACT_MISH) return launch_kernel<conv3x3_c8_direct_kernel<STATS, RYOLO_ACT_MISH>>(g, b, 0, stream, p, gpw, C8Bwd());
    return launch_kernel<conv3x3_c8_direct_kernel<STATS, RYOLO_ACT_LINEAR>>(g, b, 0, stream, p, gpw, C8Bwd());
}

__global__ void pack_weights_kernel(const float *__restrict__ w, int Cout, int Cin, int KS, int Cin_pad, int Kpad,
                                    int Cout_pad, __bf16 *__restrict__ out) {
    // out[co][ (kh*KS + kw)*Cin_pad + c ] = w[co][c][kh][kw]  (OIHW in), zero elsewhere, + 128 zero elements tail
    const size_t total = (size_t)Cout_pad * Kpad + 128;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        float v = 0.f;
        if (i < (size_t)Cout_pad * Kpad) {
            const int co = (int)(i / Kpad), k = (int)(i % Kpad);
            const int tap = k / Cin_pad, c = k % Cin_pad;
            if (co < Cout && tap < KS * KS && c < Cin) {
                const int kh = tap / KS, kw = tap % KS;
                v = w[(((size_t)co * Cin + c) * KS + kh) * KS + kw];
            }
        }
        out[i] = (__bf16)v;
    }
}

__global__ void nchw_f32_to_nhwc_bf16_kernel(const float *__restrict__ x, int N, int C, int H, int W, int Cpad,
                                             __bf16 *__restrict__ y) {
    // one thread per output pixel; channels C..Cpad-1 zero.  Cpad == 8: one 16-B store per pixel.
    const size_t npix = (size_t)N * H * W;
    for (size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x; pix < npix; pix += (size_t)gridDim.x * blockDim.x) {
        const size_t hw = pix % ((size_t)H * W), n = pix / ((size_t)H * W);
        for (int c0 = 0; c0 < Cpad; c0 += 8) {
            bf16x8 v;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int c = c0 + e;
                v[e] = (__bf16)(c < C ? x[((size_t)n * C + c) * H * W + hw] : 0.f);
            }
            *(bf16x8 *)(y + pix * Cpad + c0) = v;
        }
    }
}

__global__ void nhwc_bf16_to_nchw_f32_kernel(const __bf16 *__restrict__ x, int N, int C, int H, int W, int cs,
                                             float *__restrict__ y) {
    const size_t total = (size_t)N * C * H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t hw = i % ((size_t)H * W);
        const size_t t = i / ((size_t)H * W);
        const int c = (int)(t % C);
        const size_t n = t / C;
        y[i] = (float)x[(n * H * W + hw) * cs + c];
    }
}

// the persistent kernel exists for the two-stage tiles whose epilogue staging fits beside one stage of operands
constexpr bool igemm_persist_tile(const IgemmTile &t) { return t.NSTAGE == 2 && t.BM * t.BN * 2 <= (t.BM + t.BN) * BK * 2; }
// the instantiations with the folded BatchNorm reduce -- one tile per workgroup: the tiles the stride-1 data gradients of the 3x3 layers
// with C_in <= 128 (128 x 128, 8 waves) and of the narrow layers (256 x 64, 256 x 32) take; persistent: the 1x1 128 x 128 2x2-wave tile
constexpr bool igemm_reduce_tile(int ks, const IgemmTile &t, bool persist) {
    return persist ? ks == 1 && t.code == 7 : (t.code == 1 && ks == 3) || t.code == 2 || t.code == 3;
}

// The launches of tile T = IGEMM_TILES[I].  One tile per workgroup: FAST / general addressing x GEN (statistics, strided output
// placement), and the folded BatchNorm reduce where igemm_reduce_tile() has it.
template <int KS, int I, bool FAST, bool GEN>
int launch_one_tile(const ConvPlan &pl, ConvParams &p, const ConvLaunch &lc) {
    constexpr IgemmTile T = IGEMM_TILES[I];
    constexpr size_t smem = T.NSTAGE * (T.BM + T.BN) * BK * 2;
    const dim3 grid((unsigned)pl.grid), block(T.WGM * T.WGN * 64);
    if (lc.bnred) {
        if constexpr (FAST && !GEN && igemm_reduce_tile(KS, T, false))
            return launch_kernel<conv_igemm_kernel<KS, T.BM, T.BN, T.WGM, T.WGN, T.NSTAGE, true, false, true>>(grid, block, smem, lc.stream, p, *lc.bnred);
        else
            return RYOLO_EINVAL;
    }
    return launch_kernel<conv_igemm_kernel<KS, T.BM, T.BN, T.WGM, T.WGN, T.NSTAGE, FAST, GEN>>(grid, block, smem, lc.stream, p, BnRed());
}

// the persistent kernel's instantiations: plain for every tile; with statistics for the 4-wave tiles (1x1 layers, short-K 3x3 layers);
// with the folded BatchNorm reduce for the 1x1 128 x 128 2x2 tile
template <int KS, int I>
int launch_persist(const ConvPlan &pl, ConvParams &p, const ConvLaunch &lc) {
    constexpr IgemmTile T = IGEMM_TILES[I];
    constexpr int BM = T.BM, BN = T.BN, WGM = T.WGM, WGN = T.WGN;
    constexpr size_t smem = 2 * (BM + BN) * BK * 2;
    const dim3 g((unsigned)pl.grid), b(WGM * WGN * 64);
    p.ntiles = (int)(((long long)p.M + BM - 1) / BM * p.nt);
    p.magic_nt = magic_u32(p.nt);
    if (lc.bnred) {
        if constexpr (igemm_reduce_tile(KS, T, true)) {
            constexpr size_t smem_bn = smem + (size_t)WGM * WGN * (BN / 8) * 24 * 4;
            return launch_kernel<conv_igemm_persist_kernel<KS, BM, BN, WGM, WGN, false, true>>(g, b, smem_bn, lc.stream, p, *lc.bnred);
        } else {
            return RYOLO_EINVAL;
        }
    }
    if constexpr (WGM * WGN == 4) {
        if (p.stat_part) {
            constexpr size_t smem_st = smem + (size_t)WGM * 2 * BN * 4;
            return launch_kernel<conv_igemm_persist_kernel<KS, BM, BN, WGM, WGN, true>>(g, b, smem_st, lc.stream, p, BnRed());
        }
    }
    if (p.stat_part) return RYOLO_EINVAL;
    return launch_kernel<conv_igemm_persist_kernel<KS, BM, BN, WGM, WGN, false>>(g, b, smem, lc.stream, p, BnRed());
}

// IGEMM_TILES[I], I + 1 ... -> the plan's tile: the divisions its kernels make, then the plan's grid
template <int KS, int I = 0>
int launch_igemm_tile(const ConvPlan &pl, ConvParams &p, const ConvLaunch &lc) {
    if constexpr (I < IGEMM_NTILES) {
        constexpr IgemmTile T = IGEMM_TILES[I];
        if (pl.kernel != RYOLO_CONV_KERNEL_IGEMM + T.code) return launch_igemm_tile<KS, I + 1>(pl, p, lc);
        const bool gen = p.stat_part != nullptr || p.os != 1;
        const long long dmax = p.Wo > p.Ho ? p.Wo : p.Ho, mpad = ((long long)p.M + T.BM - 1) / T.BM * T.BM;
        p.use_magic = mpad * dmax < 0x100000000ll ? 1 : 0;
        p.magic_wo = magic_u32(p.Wo);
        p.magic_ho = magic_u32(p.Ho);
        p.nt = (p.Cout + T.BN - 1) / T.BN;
        if constexpr (igemm_persist_tile(T)) if (pl.persist) return launch_persist<KS, I>(pl, p, lc);
        if (pl.persist) return RYOLO_EINVAL;
        if (p.fast) return gen ? launch_one_tile<KS, I, true, true>(pl, p, lc) : launch_one_tile<KS, I, true, false>(pl, p, lc);
        return gen ? launch_one_tile<KS, I, false, true>(pl, p, lc) : launch_one_tile<KS, I, false, false>(pl, p, lc);
    } else {
        return RYOLO_EINVAL;
    }
}

}  // namespace

// measured (tools/layer_bench.py, MI355X): the persistent grid wins on the short-K 1x1 layers (fixed per-tile cost
// dominates: 64->32 @304 0.146 -> 0.112 ms, 256->128 @76 0.034 -> 0.031) and loses 3-5 % on the long-K 3x3 layers
// (0.120 -> 0.127 ms), so only the 1x1 launches take it unless the caller forces it -- when the tile list is deep enough and the
// multiply-high divisions are exact (persist_grid), with the 4-wave layout (the 8-wave persistent variant is slower: 0.031)
// (the training forward of a 1x1 layer takes it too: the 4-wave tiles have a statistics instantiation)
bool ryolo_detail::conv_igemm_plan(const ConvParams &p, int ksize, int tile, bool no_persist, bool force_persist, bool reduce, ConvPlan &pl) {
    const IgemmTile *t = igemm_tile(tile);
    if (!t || (ksize != 1 && ksize != 3)) return false;
    const bool gen = p.stat_part != nullptr || p.os != 1;
    const bool persist_ok = p.os == 1 && (!p.stat_part || (t->WGM * t->WGN == 4 && !p.res));
    const int mtiles = (p.M + t->BM - 1) / t->BM, nt = (p.Cout + t->BN - 1) / t->BN;
    pl.persist = false;
    pl.grid = mtiles * nt;
    if (igemm_persist_tile(*t) && p.fast && persist_ok && !no_persist && (ksize == 1 || force_persist)) {
        const PersistGrid pg = persist_grid(p.M, t->BM, p.Cout, t->BN, p.Ho, p.Wo, force_persist);
        if (pg.deep && pg.exact) {
            pl.persist = true;
            pl.grid = pg.grid;
        }
    }
    pl.rows = 0;
    if (reduce) {
        if (p.stat_part || p.ups != 1 || !igemm_reduce_tile(ksize, *t, pl.persist) || (!pl.persist && (!p.fast || gen))) return false;
        pl.rows = pl.persist ? pl.grid : mtiles;
    }
    pl.kernel = RYOLO_CONV_KERNEL_IGEMM + tile;
    return true;
}

int ryolo_detail::launch_conv_igemm(const ConvPlan &pl, ConvParams &p, const ConvLaunch &lc) {
    return pl.ksize == 1 ? launch_igemm_tile<1>(pl, p, lc) : launch_igemm_tile<3>(pl, p, lc);
}

int ryolo_detail::launch_conv0_direct(const ConvPlan &pl, ConvParams &p, const ConvLaunch &lc) {
    return p.stat_part ? launch_c8_direct<true>(p, pl.bm, (unsigned)pl.grid, lc.stream) : launch_c8_direct<false>(p, pl.bm, (unsigned)pl.grid, lc.stream);
}

extern "C" {

size_t ryolo_conv_packed_weight_bytes(int Cout, int Cin_pad, int ksize) {
    if (Cout <= 0 || Cin_pad <= 0 || (ksize != 1 && ksize != 3)) return 0;
    const size_t K = (size_t)ksize * ksize * Cin_pad;
    const size_t Kpad = (K + BK - 1) / BK * BK;
    const size_t Cout_pad = ((size_t)Cout + 127) / 128 * 128;
    return (Cout_pad * Kpad + 128) * 2;
}

int ryolo_conv_pack_weights(const float *w_oihw, int Cout, int Cin, int ksize, int Cin_pad, void *packed,
                            void *stream) {
    if (!w_oihw || !packed || Cout <= 0 || Cin <= 0 || Cin_pad < Cin || (Cin_pad & 7) || (ksize != 1 && ksize != 3))
        return RYOLO_EINVAL;
    const int K = ksize * ksize * Cin_pad, Kpad = (K + BK - 1) / BK * BK, Cout_pad = (Cout + 127) / 128 * 128;
    const size_t total = (size_t)Cout_pad * Kpad + 128;
    const int nb = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(pack_weights_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, w_oihw, Cout, Cin, ksize,
                       Cin_pad, Kpad, Cout_pad, (__bf16 *)packed);
    return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH;
}

int ryolo_nchw_f32_to_nhwc_bf16(const float *x, int N, int C, int H, int W, int Cpad, void *y, void *stream) {
    if (!x || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0 || Cpad < C || (Cpad & 7)) return RYOLO_EINVAL;
    const size_t npix = (size_t)N * H * W;
    const int nb = (int)((npix + 255) / 256 < 16384 ? (npix + 255) / 256 : 16384);
    hipLaunchKernelGGL(nchw_f32_to_nhwc_bf16_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, x, N, C, H, W, Cpad,
                       (__bf16 *)y);
    return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH;
}

int ryolo_nhwc_bf16_to_nchw_f32(const void *x, int N, int C, int H, int W, int cstride, float *y, void *stream) {
    if (!x || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0 || cstride < C) return RYOLO_EINVAL;
    const size_t total = (size_t)N * C * H * W;
    const int nb = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    hipLaunchKernelGGL(nhwc_bf16_to_nchw_f32_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const __bf16 *)x, N,
                       C, H, W, cstride, y);
    return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH;
}

int ryolo_conv0_bn_act_fwd(const ryolo_conv_desc *d, const void *x, const void *w_packed, const float *scale, const float *shift,
                           int act, const float *slope, void *y, void *stream_) {
    if (!ryolo_conv0_recompute_supported(d) || !x || !w_packed || !scale || !shift || !y) return RYOLO_EINVAL;
    if (act < 0 || act > 2 || (act == RYOLO_ACT_LEAKY && !slope)) return RYOLO_EINVAL;
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)w_packed) & 15) return RYOLO_EINVAL;
    ConvParams p{};
    const int gpw = 32;
    unsigned nblk;
    if (!conv0_params(d, d->out_cstride, p, gpw, &nblk)) return RYOLO_EINVAL;
    p.x = (const __bf16 *)x; p.w = (const __bf16 *)w_packed; p.scale = scale; p.shift = shift; p.y = (__bf16 *)y;
    p.act = act; p.slope = 0.f;
    C8Bwd bw;
    bw.slope = act == RYOLO_ACT_LEAKY ? slope : nullptr;
    bw.round_z = 1;
    ConvLaunch lc;
    lc.stream = (hipStream_t)stream_;
    if (conv0_halo_on()) return launch_conv0_halo(p, bw.slope, 1, lc);
    return launch_c8_mode(act, p, gpw, nblk, bw, 0, lc.stream);
}

size_t ryolo_conv0_bn_bwd_workspace_bytes(void) { return (size_t)STAT_ROWS * 96 * 8 + 64 * 4; }

int ryolo_conv0_bn_bwd(const ryolo_conv_desc *d, const void *x, const void *w_packed, const void *dy, int dy_cstride,
                       const float *scale, const float *shift, const float *mean, const float *invstd, int act, const float *slope,
                       void *dz, int dz_cstride, float *dgamma, float *dbeta, float *dslope, void *workspace, size_t workspace_bytes,
                       int workspace_is_zero, void *stream_) {
    if (!ryolo_conv0_recompute_supported(d) || !x || !w_packed || !dy || !scale || !shift || !mean || !invstd || !dz || !workspace)
        return RYOLO_EINVAL;
    if (workspace_bytes < ryolo_conv0_bn_bwd_workspace_bytes() || (dy_cstride & 7) || (dz_cstride & 7) || dy_cstride < 32 || dz_cstride < 32)
        return RYOLO_EINVAL;
    if (act < 0 || act > 2 || (act == RYOLO_ACT_LEAKY && !slope)) return RYOLO_EINVAL;
    if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dz | (uintptr_t)w_packed | (uintptr_t)workspace) & 15) return RYOLO_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    ConvParams p{};
    const int gpw = 32;
    unsigned nblk;
    C8Bwd bw;
    if (!conv0_params(d, dz_cstride, p, gpw, &nblk) || !buffer_extent(p.M, dy_cstride, 32, &bw.dy_bytes)) return RYOLO_EINVAL;   // (the launch writes dz)
    p.x = (const __bf16 *)x; p.w = (const __bf16 *)w_packed; p.scale = scale; p.shift = shift; p.y = (__bf16 *)dz;
    p.act = act; p.slope = 0.f;
    bw.slope = act == RYOLO_ACT_LEAKY ? slope : nullptr;            // the learnable slope stays on the device
    bw.dy = (const __bf16 *)dy; bw.dy_cs = dy_cstride; bw.mean = mean;
    double *part = (double *)workspace;
    float *kb = (float *)(part + (size_t)STAT_ROWS * 96), *kd = kb + 32;
    bw.part = part; bw.kb = kb; bw.kd = kd;
    if (!workspace_is_zero && hipMemsetAsync(part, 0, (size_t)STAT_ROWS * 96 * 8, stream) != hipSuccess) return RYOLO_ELAUNCH;
    int rc = launch_c8_mode(act, p, gpw, nblk, bw, 2, stream);
    if (rc != RYOLO_OK) return rc;
    rc = launch_kernel<conv0_bwd_finalize_kernel>(dim3(1), dim3(32), 0, stream, part, scale, mean, invstd, 1.0f / (float)p.M, kb, kd, dgamma, dbeta,
                                                  act == RYOLO_ACT_LEAKY ? dslope : nullptr);
    if (rc != RYOLO_OK) return rc;
    return launch_c8_mode(act, p, gpw, nblk, bw, 3, stream);
}

}  // extern "C"
