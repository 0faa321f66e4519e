// rotate-yolov3_amd/csrc/conv_common.h -- types, device helpers and host launch helpers shared by the convolution translation units
// (and, for the types and launch helpers, by the training units wgrad.hip and train.hip):
// conv.hip (128x128 / 256x64 / 256x32 tiles, first-layer direct kernel, packers), conv_mp.hip (256-wide multi-phase kernel), conv_mq.hip
// (two workgroups per CU), conv_pw.hip (weight-stationary 1x1), conv_stem.hip (stem layers) -- the kernel families, each with a planning
// function (does the family serve this launch? every eligibility rule and size guard, nothing written) and a launch function (derives
// what its kernel reads, picks the instantiation, launches); conv_dispatch.hip (host only: descriptor -> ConvParams, conv_plan() over the
// families in order, conv_launch(), the forward entry points and queries); conv_dgrad.hip (data gradient: tap classes, packers, its
// launches built through the same shape code and planned by conv_plan()).  Internal to libryolo_hip.so; the C ABI is include/ryolo.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/ryolo.h"

namespace ryolo_detail {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((address_space(3))) void *lds_vp;
typedef const __attribute__((address_space(1))) void *glb_vp;

constexpr int BK = 64;   // K elements per step: one 128-B LDS row per tile row
// Outputs of this size and more are stored non-temporally (measured: layer 0 at bs 32, 757 MB of output, 0.284 -> 0.177 ms;
// smaller outputs are re-read from L2 / the Infinity Cache by the next kernel and keep the default policy)
constexpr long long NT_OUT_MIN_BYTES = 128ll << 20;
constexpr int STAT_ROWS = 128;   // partial rows the statistic atomics are spread over (tile or workgroup index mod STAT_ROWS); every flush is per
                                 // workgroup now, so 128 rows keep the fp64 atomics uncontended and bn_finalize reads a quarter of what 512 cost

struct ConvParams {
    const __bf16 *x;       // input, NHWC, pixel stride in_cs (elements); already offset to its channel slice
    const __bf16 *w;       // packed weights [Cout_pad][Kpad] + 256-B zero tail
    const float *scale;    // [Cout_pad]
    const float *shift;    // [Cout_pad]
    const __bf16 *res;     // residual (same pixel grid as the output, before upsampling) or nullptr
    __bf16 *y;             // output, NHWC, pixel stride out_cs
    int N, H, W, Cin, in_cs;
    int Ho, Wo, Cout, out_cs, res_cs;
    int stride, pad;
    int K, Kpad, M;
    int cin_log2;          // 3x3 only: log2(Cin) when Cin is a power of two, else -1 (then Cin % 64 == 0)
    int act;               // RYOLO_ACT_*
    float slope;
    int ups;               // 1, or 2 = write every output pixel to its 2x2 nearest-upsampled positions
    int nt;                // number of channel tiles
    unsigned x_bytes, w_bytes;   // FAST path buffer descriptors
    int fast;
    int taps2;             // FAST path with C_in == 32: two filter taps per 64-wide K step (3x3, regular window)
    int no_persist;        // tile bit 0x200: keep the one-tile-per-workgroup grid (tests, A/B timing)
    int force_persist;     // tile bit 0x800: persistent grid also for 3x3 (tests, A/B timing)
    // generalisations used by the training kernels (FAST path only):
    int ntaps;             // taps actually visited by the K loop (forward: KS*KS)
    int tap_dy[9], tap_dx[9];   // tap t reads input pixel (hi0 + tap_dy[t], wi0 + tap_dx[t])
    int os, ooy, oox, OH, OW;   // output pixel of grid cell (i, j): (i*os + ooy, j*osx + oox) in an [N, OH, OW] tensor
    int osx;                    // column step (== os except for the x-fused stride-2 dgrad: rows step 2, super-pixels step 1)
    int ntiles;            // persistent kernel: number of (m, n) tiles
    unsigned magic_wo, magic_ho, magic_nt;   // ceil(2^32 / d): multiply-high division by Wo, Ho, nt
    int use_magic;         // the multiply-high divisions by Wo / Ho are exact for every m < M (host check)
    unsigned y_bytes, res_bytes;   // conv_mp.hip: extents of the output / residual tensors (buffer descriptors)
    double *stat_part;     // optional [STAT_ROWS][2][Cout_pad] partial sums of z and z*z (BatchNorm statistics); zeroed by the caller.
                           // fp64: the per-wave fp32 sums are added with 64-bit atomics, so the order in which the waves arrive
                           // does not show in the fp32 mean / invstd (an fp32 accumulator made the step irreproducible at 1e-7)
    int stat_cpad;
    int nt_out;            // the output tensor is too large to stay in the caches until it is read again (>= NT_OUT_MIN_BYTES): non-temporal stores
    int reg3;              // conv_mq.hip: the taps are the regular 3x3 window, tap t = (t / 3, t % 3) (cheap border masks)
    int korder = 0;        // conv_mq.hip: K-tile visiting order, 0 tap-major, 1 channel-major (the nine taps of a 64-channel slice back to back)
    int dbg0, dbg1;        // ablation builds (-DRYOLO_MP_ABLATION) only
    int pw_nb, pw_mb;      // conv_pw.hip: channel blocks, row blocks of the launch
    unsigned *trace;       // ablation builds only (conv_pw.hip cycle stamps)
    int pw_grid_cap;       // conv_pw.hip, tests: workgroups per XCD (0 = fill the chip); lets a small tensor reach the steady state of the ring
};

// BatchNorm-backward reduce folded into the 1x1 data gradient that stores the block's final dy (conv.hip: conv_igemm_persist_kernel<..., BNRED>,
// conv_pw.hip MODE 3)
struct BnRed {
    const __bf16 *z;        // the consumer block's conv output (what its BatchNorm normalised), pixel stride z_cs
    int z_cs;
    const float *scale, *shift, *mean, *invstd;   // [C] of that BatchNorm (batch statistics of the forward)
    const float *slope;     // PReLU / leaky slope (device scalar)
    float *part;            // [gridDim.x][3][C] fp32; every workgroup zeroes its row first
    unsigned z_bytes = 0;   // conv_mq.hip: extent of z (buffer descriptor), filled by its launcher
};

__device__ __forceinline__ float mish(float v) {
    // x * tanh(softplus(x)) = x * (n - 1) / (n + 1) with n = (1 + e^x)^2; e^x clamped so n stays finite
    const float e = __expf(fminf(v, 20.f));
    const float n = (1.f + e) * (1.f + e);
    return v * (n - 1.f) / (n + 1.f);
}

// Sum over the 16 lanes of a DPP row (lanes 16k .. 16k+15), result in every lane.  Four v_add_f32 with DPP operands
// (the two quad swaps, half-row mirror, row mirror): pure VALU, where the ds_bpermute behind __shfl_xor would take LDS
// issue slots from the K loops of the co-resident workgroups.  Same pairing as the xor butterfly (1, 2, 4, 8), so the
// sums are bit-identical to it.
__device__ __forceinline__ float row16_sum(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));   // row_mirror
#endif
    return v;
}

// v(lane) + v(lane ^ O) for O = 4 / 8 (DPP rotation inside the 16-lane row: lane + O mod 16, the same partner set once both steps ran),
// 16 / 32 (v_permlane16_swap / v_permlane32_swap of the value with itself: both operands then hold the two halves side by side).  Pure
// VALU: the ds_bpermute behind __shfl_xor costs an LDS round trip per call (48 of them per output tile made the folded BatchNorm reduce
// of the one-tile-per-workgroup kernels 16 % slower than the plain data gradient).
template <int O>
__device__ __forceinline__ float lane_xor_sum(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (O == 4) {
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xF, 0xF, true));   // row_ror:4
    } else if constexpr (O == 8) {
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xF, 0xF, true));   // row_ror:8
    } else if constexpr (O == 16) {
        const unsigned u = __builtin_bit_cast(unsigned, v);
        const auto s = __builtin_amdgcn_permlane16_swap(u, u, false, false);
        v = __builtin_bit_cast(float, (unsigned)s[0]) + __builtin_bit_cast(float, (unsigned)s[1]);
    } else {
        static_assert(O == 32, "partner distance");
        const unsigned u = __builtin_bit_cast(unsigned, v);
        const auto s = __builtin_amdgcn_permlane32_swap(u, u, false, false);
        v = __builtin_bit_cast(float, (unsigned)s[0]) + __builtin_bit_cast(float, (unsigned)s[1]);
    }
#endif
    return v;
}
// sum over the lanes that share (lane mod CPR), CPR in {4, 8, 16}: every lane of the class ends with the same total
template <int CPR>
__device__ __forceinline__ float lane_class_sum(float v) {
    if constexpr (CPR <= 4) v = lane_xor_sum<4>(v);
    if constexpr (CPR <= 8) v = lane_xor_sum<8>(v);
    v = lane_xor_sum<16>(v);
    return lane_xor_sum<32>(v);
}

// 16-B-per-lane buffer load straight into LDS (lane-linear at `lds`); lanes whose byte offset is outside
// [0, bytes) get zeros.  The builtins exist only in the device pass.
__device__ __forceinline__ void buffer_load_lds16(const void *base, unsigned bytes, char *lds, int voffset, int soffset) {
#if defined(__HIP_DEVICE_COMPILE__)
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, bytes, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_vp)lds, 16, voffset, soffset, 0, 0);
#endif
}

// 16-B buffer store whose soffset is an SGPR, safe against the store-data hazard.  A VMEM store of more than 64 bits reads
// its data VGPRs a cycle after issue, and a VALU instruction that overwrites them right behind the store races that read.
// The compiler inserts the required wait state only when soffset is NOT a register (LLVM GCNHazardRecognizer,
// createsVALUHazard); on gfx950 the race is real with a register soffset too: with `store v[138:141] ... s85` directly
// followed by `v_pk_fma_f32 v[138:139]`, lanes 12-15 of every 16-lane row of the second data dword reached memory as the
// NEXT fragment's bits (found as wrong z in the statistics instantiation; the same fault was the unexplained Mish garbage
// of conv_tw.hip).  The asm below READS the data registers, so no write to them can be scheduled in front of it, and its
// s_nop supplies the wait states; tools/check_mp_isa.py fails the build if any 12-/16-B store in the library has its data
// overwritten with fewer than two wait states in between.
template <int AUX = 0>
__device__ __forceinline__ void buffer_store16_soff(u32x4 v, __amdgpu_buffer_rsrc_t rsrc, int voffset, int soffset) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, voffset, soffset, AUX);
    asm volatile("s_nop 1" ::"v"(v));
#endif
}

// n / d by multiply-high with magic = ceil(2^32 / d); magic == 0 encodes d == 1
__device__ __forceinline__ int udiv_magic(int n, unsigned magic) {
    return magic ? (int)__umulhi((unsigned)n, magic) : n;
}

// m -> (t = m / Wo, wo = m % Wo), t -> (img = t / Ho, ho): multiply-high when the host found it exact (use_magic), else `/`
__device__ __forceinline__ void split_pixel(int m, int Wo, int Ho, unsigned magic_wo, unsigned magic_ho, int use_magic, int &wo,
                                            int &ho, int &img) {
    if (use_magic) {
        const int t = udiv_magic(m, magic_wo);
        wo = m - t * Wo;
        img = udiv_magic(t, magic_ho);
        ho = t - img * Ho;
    } else {
        const int t = m / Wo;
        wo = m % Wo;
        ho = t % Ho;
        img = t / Ho;
    }
}


// ---- host side --------------------------------------------------------------------------------------------------------------------
// What a launch needs besides its ConvParams and its plan: the stream, and the operands of the folded BatchNorm-backward reduce when the
// plan carries one (plan.rows > 0: ryolo_conv2d_dgrad_bnreduce)
struct ConvLaunch {
    hipStream_t stream = nullptr;
    const BnRed *bnred = nullptr;
};

// The six implicit-GEMM tiles of conv.hip, stated once: `code` is the tile as ryolo_conv_desc::tile forces it and as
// RYOLO_CONV_KERNEL_IGEMM + code names it; BM pixels x BN channels, WGM x WGN waves, NSTAGE operand buffers
struct IgemmTile {
    int code, BM, BN, WGM, WGN, NSTAGE;
};
constexpr IgemmTile IGEMM_TILES[] = {{1, 128, 128, 2, 4, 2}, {2, 256, 64, 4, 1, 2}, {3, 256, 32, 4, 1, 2},
                                     {4, 256, 128, 4, 2, 3}, {6, 128, 128, 4, 2, 2}, {7, 128, 128, 2, 2, 2}};
constexpr int IGEMM_NTILES = sizeof(IGEMM_TILES) / sizeof(IGEMM_TILES[0]);
constexpr const IgemmTile *igemm_tile(int code) {
    for (int i = 0; i < IGEMM_NTILES; i++)
        if (IGEMM_TILES[i].code == code) return &IGEMM_TILES[i];
    return nullptr;
}

// Everything decided about one launch.  conv_plan() makes it -- a value, computed per call from the ConvParams alone, nothing kept
// between calls -- and the queries (ryolo_conv_kernel_choice, ryolo_conv_dgrad_kernel_choice, ryolo_conv2d_dgrad_bnreduce_rows) read the
// same plan conv_launch() executes.
struct ConvPlan {
    int kernel = -1;        // RYOLO_CONV_KERNEL_* (igemm: RYOLO_CONV_KERNEL_IGEMM + tile code); -1: no family serves the launch
    int ksize = 0;
    int bm = 0;             // pixel rows of the tile where a family has several (conv_mp 256 / 192, the 128-channel conv_mq 128 / 64);
                            // layer 0: 16-pixel groups per wave
    bool persist = false;   // igemm: the persistent grid
    int grid = 0;           // workgroups
    int rows = 0;           // with the folded BatchNorm reduce: rows of part[][3][C] the launch writes (one per workgroup of a persistent
                            // launch, one per pixel tile of a one-tile-per-workgroup launch); 0: no reduce
    int variant = 0;        // measurement build: schedule variant of conv_mp / conv_mq
};

// compute units of the current device (256 when it cannot be asked), read once
inline int cu_count() {
    static const int cus = [] {
        int dev = 0, n = 0;
        return hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 256;
    }();
    return cus;
}

// Launch KFN; RYOLO_OK or RYOLO_ELAUNCH.  A kernel that takes more than 64 KiB of dynamic LDS has its limit raised first, once per kernel
// function (the static belongs to this instantiation, i.e. to KFN, and its initialisation is thread-safe).
template <auto KFN, typename... Args>
int launch_kernel(dim3 grid, dim3 block, size_t smem, hipStream_t stream, Args... args) {
    if (smem > 64 * 1024) {
        static const hipError_t raised = hipFuncSetAttribute((const void *)KFN, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (raised != hipSuccess) return RYOLO_ELAUNCH;
    }
    hipLaunchKernelGGL(KFN, grid, block, smem, stream, args...);
    return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH;
}

// Bytes of `npix` NHWC bf16 pixels of stride `cs` of which the last uses `c` channels, as the extent of a buffer descriptor; false when
// the kernels' 31-bit byte offsets do not reach that far.  (A packed filter of `rows` rows: npix = rows, cs = Kpad, c = Kpad + 128.)
inline bool buffer_extent(unsigned long long npix, long long cs, long long c, unsigned *bytes = nullptr) {
    const unsigned long long b = ((npix - 1) * (unsigned long long)cs + (unsigned long long)c) * 2ull;
    if (b >= 0x7fffff00ull) return false;
    if (bytes) *bytes = (unsigned)b;
    return true;
}

// The persistent grid of the implicit-GEMM tiles over M pixels x Cout channels in BM x BN tiles: its size (two workgroups per CU, a
// multiple of 8 for the XCD chunking), whether the tile list is deep enough for it to win -- at least rounds2 / 2 rounds (measured at 2.5:
// 1444 tiles 0.030 -> 0.028 ms, 722 tiles 0.021 -> 0.022), or just more than one round when forced -- and whether the kernel's
// multiply-high divisions are exact.  The one statement of that rule: conv_igemm_plan(), conv_plan()'s 1x1 pick and the conv_mq128 picks
// ask here; the launch and the rows of a folded reduce read the plan.
struct PersistGrid {
    int grid, nt;
    long long tiles;
    bool deep, exact;
};
inline PersistGrid persist_grid(long long M, int BM, int Cout, int BN, int Ho, int Wo, bool force = false, int rounds2 = 5) {
    const long long mt = (M + BM - 1) / BM, nt = (Cout + BN - 1) / BN, dmax = Wo > Ho ? Wo : Ho;
    PersistGrid g;
    g.grid = (2 * cu_count()) & ~7;
    g.nt = (int)nt;
    g.tiles = mt * nt;
    g.deep = force ? g.tiles > g.grid : 2 * g.tiles >= (long long)rounds2 * g.grid;
    g.exact = g.grid >= 8 && mt * BM * dmax < 0x100000000ll && g.tiles * nt < 0x100000000ll;
    return g;
}

inline unsigned magic_u32(int d) { return d <= 1 ? 0u : (unsigned)((0x100000000ull + (unsigned)d - 1) / (unsigned)d); }   // udiv_magic's operand

// The tile list of a persistent conv_mp / conv_mq launch over bm-pixel x bn-channel tiles, and the extents of its output and residual
// tensors.  fits: within the kernels' 32-bit tile / pixel arithmetic and 31-bit byte offsets -- the planning functions ask, the launch
// functions write the fields into the ConvParams (set_tile_list)
struct TileList {
    int nt;
    long long T;
    unsigned y_bytes, res_bytes;
    bool fits;
};
inline TileList tile_list(const ConvParams &p, int bm, int bn) {
    TileList t;
    const long long mt = ((long long)p.M + bm - 1) / bm, dmax = p.Wo > p.Ho ? p.Wo : p.Ho;
    t.nt = (p.Cout + bn - 1) / bn;
    t.T = mt * t.nt;
    const unsigned long long yb = (((unsigned long long)p.N * p.OH * p.OW - 1) * p.out_cs + p.Cout) * 2ull;
    const unsigned long long rb = p.res ? (((unsigned long long)p.N * p.OH * p.OW - 1) * p.res_cs + p.Cout) * 2ull : 0ull;
    t.fits = mt * bm * dmax < 0x100000000ll && t.T * t.nt < 0x100000000ll && t.T <= 0x7fffffffll && yb < 0x7fffff00ull && rb < 0x7fffff00ull;
    t.y_bytes = (unsigned)yb;
    t.res_bytes = (unsigned)rb;
    return t;
}
inline void set_tile_list(ConvParams &p, const TileList &t) {
    p.nt = t.nt;
    p.ntiles = (int)t.T;
    p.use_magic = 1;
    p.magic_wo = magic_u32(p.Wo);
    p.magic_ho = magic_u32(p.Ho);
    p.magic_nt = magic_u32(p.nt);
    p.y_bytes = t.y_bytes;
    p.res_bytes = t.res_bytes;
}

// blocks of `tb` threads for `total` work items, at least one and at most `cap` (the elementwise passes and the split-K reduces)
inline int grid_for(long long total, int tb = 256, int cap = 32768) {
    long long nb = (total + tb - 1) / tb;
    return (int)(nb < 1 ? 1 : (nb > cap ? cap : nb));
}

inline int ilog2_exact(int v) {
    int l = 0;
    while ((1 << l) < v) l++;
    return (1 << l) == v ? l : -1;
}

// conv_dispatch.hip: descriptor check; the shape part of a launch from its descriptor (tensor geometry, GEMM sizes, the regular tap window,
// dense output placement, the epilogue) and the pixel grid of a launch (Ho x Wo per image, M = N * Ho * Wo; false: no pixels, or more than
// the 31-bit pixel index holds); layer 0's shape and launch parameters; the plan of one launch and its execution; the switches several
// units read
int conv_validate(const ryolo_conv_desc *d);
bool conv_shape(const ryolo_conv_desc *d, ConvParams &p);
bool conv_pixels(ConvParams &p, long long Ho, long long Wo);
bool conv0_shape(const ryolo_conv_desc *d, int out_cs);
bool conv0_params(const ryolo_conv_desc *d, int out_cs, ConvParams &p, int gpw, unsigned *nblk);
bool conv0_halo_on();
// The plan of the launch `p` describes: the forced family (pick = ryolo_conv_desc::tile's low byte) or, for pick 0, the first family in the
// dispatch order whose planning function accepts.  want_reduce: the launch must carry the folded BatchNorm-backward reduce (stride-1 data
// gradients, pick 0); the plan then holds the rows it writes.  kernel < 0: refused.
ConvPlan conv_plan(const ConvParams &p, int ksize, int pick, bool want_reduce);
int conv_launch(const ConvPlan &pl, ConvParams &p, const ConvLaunch &lc);
long long nt_out_min_bytes();

// Every family below: X_plan() answers whether the family serves the launch -- eligibility and every size guard -- and fills its part of
// the plan; it writes nothing into the ConvParams.  launch_X() executes such a plan: it derives the ConvParams fields its kernel reads,
// picks the instantiation and launches; RYOLO_ELAUNCH, or RYOLO_EINVAL for a plan that names no instantiation (an internal error).
// conv.hip: the implicit-GEMM tiles (IGEMM_TILES), one tile per workgroup or -- short-K launches with a deep tile list -- a persistent
// grid; no_persist / force_persist: the caller's say on that grid (tile bits 0x200 / 0x800, conv_plan()'s rules); reduce: the folded
// BatchNorm reduce (the persistent 1x1 2x2-wave tile; the 256 x 64 / 256 x 32 tiles and the 3x3 128 x 128 tile one tile per workgroup)
bool conv_igemm_plan(const ConvParams &p, int ksize, int tile, bool no_persist, bool force_persist, bool reduce, ConvPlan &pl);
int launch_conv_igemm(const ConvPlan &pl, ConvParams &p, const ConvLaunch &lc);
// ... and Darknet-53 layer 0 on conv3x3_c8_direct_kernel: pl.bm 16-pixel groups per wave, pl.grid blocks
int launch_conv0_direct(const ConvPlan &pl, ConvParams &p, const ConvLaunch &lc);
// conv_mp.hip: 256-channel x BM-pixel workgroup tile, 8 waves, multi-phase K loop (FAST path only); bm 256, 192 or 0 = pick per shape
bool conv_mp_eligible(const ConvParams &p);
int conv_mp_pick_bm(const ConvParams &p);
bool conv_mp_plan(const ConvParams &p, int bm, int variant, ConvPlan &pl);
int launch_conv_mp(const ConvPlan &pl, ConvParams &p, const ConvLaunch &lc);
// conv_mq.hip: 128-pixel x 256-channel tile, 4 waves, two independent workgroups per CU (same eligibility as conv_mp)
bool conv_mq_plan(const ConvParams &p, int variant, ConvPlan &pl);
int launch_conv_mq(const ConvPlan &pl, ConvParams &p, const ConvLaunch &lc);
// ... and its 128-CHANNEL members (measurement build only): bm = 128 or 64 pixels per tile; C_out % 128 == 0, otherwise conv_mq's
// conditions.  reduce (stride-1 launches without statistics): the folded BatchNorm reduce, one row per workgroup
bool conv_mq128_eligible(const ConvParams &p);
bool conv_mq128_plan(const ConvParams &p, int bm, bool reduce, ConvPlan &pl);
int launch_conv_mq128(const ConvPlan &pl, ConvParams &p, const ConvLaunch &lc);
// conv_stem.hip: 3x3, C_in 32 -> C_out 64, stride 1 / 2: the input patch of an 8 x 32 output block staged once, the filter in registers
bool conv_stem_plan(const ConvParams &p, int ksize, ConvPlan &pl);
int launch_conv_stem(const ConvPlan &pl, ConvParams &p, const ConvLaunch &lc);
bool conv_stem64_plan(const ConvParams &p, int ksize, ConvPlan &pl);      // conv_stem.hip: 3x3 / 1, 64 -> 128
int launch_conv_stem64(const ConvPlan &pl, ConvParams &p, const ConvLaunch &lc);
// conv_stem.hip: Darknet-53 layer 0 (3x3, 8 -> 32) forward with its input patch staged in LDS (no statistics); slope_dev: optional device
// scalar for leaky / PReLU; round_z: BatchNorm applied to z rounded to bf16 (training recompute)
int launch_conv0_halo(ConvParams &p, const float *slope_dev, int round_z, const ConvLaunch &lc);
// conv_stem.hip: the data gradients of the two 3x3 32 -> 64 stem layers (64 -> 32 channels in the gradient's direction) as one persistent
// launch each -- stride 2: all four output-parity classes from one staged dz patch, w_classes = the four classic class images of
// ryolo_conv_pack_weights_dgrad; stride 1: its single nine-tap image -- and of the 3x3 / 2 64 -> 128 layer (the waves split the output
// channels).  d: the FORWARD conv; the plan: those shapes, dz and dx within 31-bit byte offsets
bool conv_stem_dgrad_plan(const ryolo_conv_desc *d, int dz_cs, ConvPlan &pl);
int launch_conv_stem_dgrad(const ConvPlan &pl, const ryolo_conv_desc *d, const void *dz, int dz_cs, const void *w_classes, void *dx, int accumulate,
                           int nt_out, const ConvLaunch &lc);
// ... and two stem layers in one launch (inference): the 32-channel tensor between them is computed into LDS, never stored
int conv_stem_pair_kind(const ryolo_conv_desc *first, const ryolo_conv_desc *second, int shortcut_from_input);
int launch_conv_stem_pair(int kind, ConvParams &p /* the second layer */, const void *x, unsigned x_bytes, int in_cs, int H, int W,
                          const void *w_first, int kpad_first, const float *scale_first, const float *shift_first, int act_first,
                          float slope_first, hipStream_t stream);
// conv_pw.hip: 1x1 stride-1 layers (and their data gradients), weight-stationary: the filter slice in registers, rows through an LDS ring
// (reduce: the folded BatchNorm reduce, MODE 3, one row per workgroup)
bool conv_pw_plan(const ConvParams &p, int ksize, bool reduce, ConvPlan &pl);
bool conv_pw_preferred(const ConvParams &p);        // the shapes on which it beats the 128 x 128 tile (auto dispatch)
int launch_conv_pw(const ConvPlan &pl, ConvParams &p, const ConvLaunch &lc);
// a YOLO head (1x1, K = 256, na*no <= 512 channels) decoded from the accumulators: io / p rows out, no head tensor; with `head` (the
// training forward) p rows and the bf16 head tensor [M][head_cs] out, no io rows
bool conv_pw_decode_supported(const ConvParams &p, int na, int no);
int launch_conv_pw_decode(ConvParams &p, float *io, long long io_img_rows, long long io_row0, float *pout, const float *anchors, int na, int no,
                          float stride, float cf, int arc, hipStream_t stream, void *head = nullptr, int head_cs = 0);
#ifdef RYOLO_MP_ABLATION
int ryolo_mp_ablation_variant(int slot);   // conv_mp.hip: VAR code stored in debug slot `slot` (ablation builds only)
#endif

// Tuning switches.  The shipped library knows SIX: the dispatch selections the tests and the A/B legs of tools/measure_round.sh use.  They are
// read from the environment ONCE (first use) and can be changed in-process through ryolo_set_tuning() (include/ryolo.h) -- no getenv on a
// launch path, no race with a setenv from another thread.  Every other environment switch of rounds 3-5 (thresholds, sweep orders, slab
// sizes, the 128-channel conv_mq family ...) exists in the measurement build only (-DRYOLO_MP_ABLATION, abl_env()).
enum TuneKey { TUNE_CONV3X3 = 0, TUNE_CONV1X1, TUNE_RNMS_TILES, TUNE_MQ_KORDER, TUNE_BN_REDUCE_TILES, TUNE_STEM_DGRAD, TUNE_COUNT };
const char *tune(TuneKey k);               // conv_dispatch.hip: the switch's value, nullptr = unset
#ifdef RYOLO_MP_ABLATION
inline const char *abl_env(const char *name) { return getenv(name); }
#else
inline const char *abl_env(const char *) { return nullptr; }
#endif

}  // namespace ryolo_detail
