// rotate-yolov3_amd/csrc/conv_dispatch.hip -- the host side of the convolutions, no kernel: descriptor -> ConvParams (conv_shape, the one
// builder the forward and the data gradient share), conv_plan() -- which kernel family serves a launch, decided once as a value -- and
// conv_launch(), the tuning switches, and the forward entry points and queries.  The families' planning and launch functions live with
// their kernels (conv.hip, conv_mp.hip, conv_mq.hip, conv_pw.hip, conv_stem.hip; conv_common.h declares them).
#include <cstring>

#include <mutex>

#include "conv_common.h"

using namespace ryolo_detail;

// ---- the tuning switches of the shipped library (conv_common.h: TuneKey).  One getenv per switch, once.
static const char *const TUNE_NAMES[TUNE_COUNT] = {"RYOLO_CONV3X3", "RYOLO_CONV1X1", "RYOLO_RNMS_TILES", "RYOLO_MQ_KORDER", "RYOLO_BN_REDUCE_TILES",
                                                   "RYOLO_STEM_DGRAD"};
static char g_tune_val[TUNE_COUNT][24];
static bool g_tune_set[TUNE_COUNT];
static std::once_flag g_tune_once;
static void tune_store(int k, const char *v) {
    g_tune_set[k] = v != nullptr && v[0] != 0;
    if (g_tune_set[k]) {
        strncpy(g_tune_val[k], v, sizeof(g_tune_val[k]) - 1);
        g_tune_val[k][sizeof(g_tune_val[k]) - 1] = 0;
    }
}
static void tune_init() {
    for (int k = 0; k < TUNE_COUNT; k++) tune_store(k, getenv(TUNE_NAMES[k]));
}
namespace ryolo_detail {
const char *tune(TuneKey k) {
    std::call_once(g_tune_once, tune_init);
    return g_tune_set[k] ? g_tune_val[k] : nullptr;
}
}  // namespace ryolo_detail
extern "C" int ryolo_set_tuning(const char *name, const char *value) {
    if (!name) return RYOLO_EINVAL;
    std::call_once(g_tune_once, tune_init);
    for (int k = 0; k < TUNE_COUNT; k++)
        if (!strcmp(name, TUNE_NAMES[k])) {
            tune_store(k, value);         // (not synchronised with launches in flight on other threads: a test / A-B facility)
            return RYOLO_OK;
        }
    return RYOLO_EINVAL;
}

static int pick_tile(const ryolo_conv_desc *d) {
    return d->tile & 0xff;   // 0 = auto (conv_plan decides); bit 8 (0x100) forces the general (slow-address) path, for tests
}

// Which 256-channel tile a 3x3 layer takes: conv_mp.hip (one 8-wave workgroup per CU, 256 or 192 pixel rows) or conv_mq.hip (two
// 4-wave workgroups per CU, 128 rows).  Estimated launch time = (tiles of the busiest CU) x (time per tile), time per tile
// linear in the K depth; coefficients (us, bs 32 / 608^2 layers with the fused shortcut, MI355X) from tools/mp_ablate.py,
// profiles/r03_mp_vs_mq.txt.  conv_mq wins where the tile list is deep enough to keep both workgroups of every CU busy (the
// 76^2 and 38^2 layers), conv_mp's 192-row tile where one round of tiles fills the chip better (19^2: 244 tiles on 256 CUs).
// Returns 0 = conv_mq, else the BM of conv_mp.  RYOLO_CONV3X3 = mp | mq overrides (A/B timing, tests).
static int pick_wide_tile(const ConvParams &p) {
    const char *e = tune(TUNE_CONV3X3);
    const int forced = !e ? 0 : (!strcmp(e, "mp") ? 1 : (!strcmp(e, "mq") ? 2 : 0));
    if (forced == 2) return 0;
    const int bm_mp = conv_mp_pick_bm(p);
    if (forced == 1) return bm_mp;
    // Cost model in microseconds, calibrated on tools/mp_ablate.py --exp mq at bs 32 and bs 64 (K tiles 18 / 36 / 72 = the 76^2 /
    // 38^2 / 19^2 layers; piecewise linear in between, the last slope beyond):
    //   conv_mp   rounds of the persistent grid x the time of one tile;
    //   conv_mq   the busiest CU hosts workgroups `loc` and `loc + wgx/2` of an XCD with a >= b tiles: b tile slots run with both
    //             workgroups resident (c2 per slot), the a - b slots after the partner has finished run alone at 0.7 c2.
    const long long cus = cu_count() & ~7, nt = (p.Cout + 255) / 256, kt = p.Kpad / BK;
    auto interp = [&](double v18, double v36, double v72) {
        return kt <= 36 ? v18 + (kt - 18) * (v36 - v18) / 18.0 : v36 + (kt - 36) * (v72 - v36) / 36.0;
    };
    auto rounds = [&](int bm) { return ((((long long)p.M + bm - 1) / bm) * nt + cus - 1) / cus; };
    const double t256 = rounds(256) * interp(35.5, 59.5, 102.0), t192 = rounds(192) * interp(30.5, 53.0, 92.0);
    // conv_mq: XCD chunks of the tile list, 2 x cus / 8 workgroups per XCD, CU c hosts workgroups c and c + cus / 8
    const long long tq = ((((long long)p.M + 127) / 128) * nt + 7) / 8, wgx = 2 * cus / 8;
    auto ntile = [&](long long loc) { return loc < tq ? (tq - loc + wgx - 1) / wgx : 0; };
    const double c2 = interp(32.5, 59.0, 97.0);
    const double tq_ = (double)ntile(wgx / 2) * c2 + (double)(ntile(0) - ntile(wgx / 2)) * 0.7 * c2;
    if (tq_ < t256 && tq_ < t192) return 0;
    return t192 < t256 ? 192 : 256;
}

static long long g_nt_out_min = NT_OUT_MIN_BYTES;      // (settable in ablation builds: ryolo_debug_conv_nt_min)
// (measurement build: RYOLO_NT_OUT_MIN_MB overrides the threshold (MiB) per call -- the in-chain sweep of tools/step_ab.py, profiles/r05_ab_log.txt)
long long ryolo_detail::nt_out_min_bytes() {
    const char *e = abl_env("RYOLO_NT_OUT_MIN_MB");
    return e ? (long long)atoll(e) << 20 : g_nt_out_min;
}
// (sc1 write-through stores for the outputs below that threshold -- no dirty lines left in L2 at the kernel boundary -- were tried in the chain
// in round 5 and lost: bs-32 forward 6.105 ms default / 6.148 from 32 MiB / 6.191 from 8 MiB / 6.130 everywhere, profiles/r05_ab_log.txt; removed)
#ifdef RYOLO_MP_ABLATION
extern "C" void ryolo_debug_conv_nt_min(long long bytes) { g_nt_out_min = bytes; }
#endif

// RYOLO_CONV1X1 = igemm keeps the 1x1 layers on the 128 x 128 tiles (A/B timing; ryolo_set_tuning)
static bool conv_pw_disabled() {
    const char *e = tune(TUNE_CONV1X1);
    return e && !strcmp(e, "igemm");
}

// conv_mq.hip's 128-channel tiles (round 5).  RYOLO_MQ128 = 0 (default): off -- the 128 x 128 / 256 x 64 tiles of conv.hip as in round 4;
// 1: the 3x3 layers and data gradients with C_out % 256 != 0; 2: also the 1x1 layers whose 128-pixel tile list is short (38^2 / 19^2).
// OPT-IN because they measure no faster than the tiles they would replace (profiles/r05_mq128_bench.txt, r05_ab_log.txt: bs-64 step 49.27 ms
// off / 49.59 on / 49.85 with the 1x1 layers; bs-32 forward 6.08 / 6.07 / 6.30 ms): with 32 channels per wave a K tile moves 0.625 KiB of
// LDS fragments per MFMA against 0.375 for the 256-channel tile -- the LDS pipe, not the schedule, bounds these layers.
// MEASUREMENT BUILD ONLY (round 6): the shipped library has neither the switch nor the instantiations (conv_mq128_plan refuses).
static int mq128_knob() {
    const char *e = abl_env("RYOLO_MQ128");
    return e ? atoi(e) : 0;
}
// pixels per tile: 64 when the list of 128-pixel tiles is less than 2.5 rounds of the two-workgroups-per-CU grid deep
static int mq128_pick_bm(const ConvParams &p) {
    return persist_grid(p.M, 128, p.Cout, 128, p.Ho, p.Wo).deep ? 128 : 64;
}
// does the auto dispatch send this launch to the 128-channel family?  (3x3: every eligible shape the 256-channel tiles do not serve;
// 1x1 (knob 2): K >= 256 and a short tile list -- the 76^2 layers stay on conv_pw.hip, HBM-bound and at their floor there)
static bool mq128_auto(const ConvParams &p, int ksize) {
    const int knob = mq128_knob();
    if (knob <= 0 || !conv_mq128_eligible(p)) return false;
    if (ksize == 3) return !conv_mp_eligible(p);
    if (knob < 2 || p.Kpad < 4 * BK) return false;
    return !persist_grid(p.M, 128, p.Cout, 128, p.Ho, p.Wo, false, 8).deep;      // fewer than FOUR rounds of 128-pixel tiles
}

// RYOLO_CONV0=direct keeps layer 0 on conv3x3_c8_direct_kernel (fragments from global memory); default: the LDS-staged kernel of
// conv_stem.hip (measurement build only since round 6: A/B timing)
bool ryolo_detail::conv0_halo_on() {
    const char *e = abl_env("RYOLO_CONV0");
    return !(e && !strcmp(e, "direct"));
}

// ---- the plan of one launch
namespace {

// a forced ryolo_conv_desc::tile low byte -> its family and parameter; the implicit-GEMM tiles are forced by their codes (IGEMM_TILES)
enum Family { F_MP, F_MQ, F_STEM, F_PW, F_MQ128, F_STEM64 };
struct ForcedPick {
    int pick;
    Family family;
    int bm;      // pixel rows (0: per shape)
};
constexpr ForcedPick FORCED_PICKS[] = {{8, F_MP, 256}, {9, F_MQ, 0},      {11, F_MP, 192},   {12, F_STEM, 0},  {13, F_PW, 0},
                                       {14, F_MP, 0},  {15, F_MQ128, 128}, {16, F_MQ128, 64}, {17, F_STEM64, 0}};

bool forced_plan(const ForcedPick &f, const ConvParams &p, int ksize, ConvPlan &pl) {
    switch (f.family) {
        case F_MP: return conv_mp_plan(p, f.bm, 0, pl);
        case F_MQ: return conv_mq_plan(p, 0, pl);
        case F_STEM: return conv_stem_plan(p, ksize, pl);
        case F_PW: return conv_pw_plan(p, ksize, false, pl);
        case F_MQ128: return conv_mq128_plan(p, f.bm, false, pl);
        case F_STEM64: return conv_stem64_plan(p, ksize, pl);
    }
    return false;
}

// an implicit-GEMM tile as the dispatch asks for it: a 1x1 launch on the 128 x 128 tile runs 8 waves of 64 pixels x 32 channels one tile
// per workgroup, except where the persistent grid wins -- that one has the 4-wave layout (tile 7)
bool igemm_plan(const ConvParams &p, int ksize, int tile, bool no_persist, bool force_persist, bool reduce, ConvPlan &pl) {
    if (ksize == 1 && tile == 1) {
        if (p.fast && p.os == 1 && !(p.stat_part && p.res) && !no_persist && (force_persist || persist_grid(p.M, 128, p.Cout, 128, p.Ho, p.Wo).deep))
            tile = 7;
        else
            no_persist = true;
    }
    return conv_igemm_plan(p, ksize, tile, no_persist, force_persist, reduce, pl);
}

// the tile the auto dispatch takes by output channels
int igemm_auto_tile(const ConvParams &p) { return p.Cout <= 32 ? 3 : (p.Cout <= 64 ? 2 : 1); }

// The folded BatchNorm-backward reduce of a stride-1 data gradient `p`: which kernel carries it, and the rows of partial sums that launch
// writes.  In order:
//   the 128-channel conv_mq tiles (measurement build) where they are the plain data gradient's kernel;
//   1x1 layers with whole 128-channel tiles: conv_pw.hip where it is the faster data gradient (K = 128: the 76^2 residual blocks, 127 vs
//   133 us at bs 64) and where the persistent 128 x 128 tile does not apply (tile lists less than 2.5 rounds deep: 19^2); that persistent
//   2x2-wave tile elsewhere (38^2: 68 vs 70 us, 19^2 K 512: 49 vs 54 us; tools/pw_bench.py --train);
//   a one-tile-per-workgroup tile where that tile is the plain (accumulating) data gradient's kernel too -- the 3x3 layers with C_in <= 128,
//   the 1x1 layers with C_in <= 64; a layer that conv_mq / conv_mp serve keeps them: the reduce is not worth a slower conv.
//   RYOLO_BN_REDUCE_TILES = 0 turns these off, 2 keeps only the 256 x 64 tile (A/B timing; ryolo_set_tuning).
void reduce_plan(const ConvParams &p, int ksize, ConvPlan &pl) {
    ConvParams acc = p;
    acc.res = p.y;
    const ConvPlan natural = conv_plan(acc, ksize, 0, false);
    const bool dense = p.out_cs == p.Cout;
    ConvPlan c;
    if (mq128_knob() > 0 && dense && (p.Cout & 127) == 0 && (natural.kernel == RYOLO_CONV_KERNEL_MQ128 || natural.kernel == RYOLO_CONV_KERNEL_MQ64) &&
        conv_mq128_plan(p, natural.bm, true, c)) {
        pl = c;
        return;
    }
    if (ksize == 1 && (p.Cout & 127) == 0 && (p.Cin & 63) == 0) {
        ConvPlan pw, ps;
        // (conv_pw.hip with the margin this fold was measured with: 1024 look-ahead row blocks of dz and a dense dx within 31-bit offsets)
        const bool pw_ok = !conv_pw_disabled() && dense && buffer_extent((unsigned long long)p.M + 1024 * 128, p.in_cs, p.Cin) &&
                           buffer_extent(p.M, p.Cout, p.Cout) && conv_pw_plan(p, ksize, true, pw);
        const bool ps_ok = conv_igemm_plan(p, ksize, 7, false, false, true, ps) && ps.persist;
        if (pw_ok && (p.Cin == 128 || !ps_ok)) {
            pl = pw;
            return;
        }
        if (ps_ok) {
            // tile bit 0x200 (tests: no persistent grid) refuses this launch and offers no other: the rows keep saying what the fold
            // launches without the bit, the kernel says refused -- as before this plan existed
            if (p.no_persist) ps.kernel = -1;
            pl = ps;
            return;
        }
    }
    const char *e = tune(TUNE_BN_REDUCE_TILES);
    const int knob = e ? atoi(e) : 1;
    const int tile = igemm_auto_tile(p);
    if (knob == 0 || !dense || natural.kernel < 0 || !igemm_plan(p, ksize, tile, true, false, true, c) || c.kernel != natural.kernel) return;
    if (tile == 3) return;           // 256 x 32: the plain data gradient runs on the persistent grid (short K), 233 us faster than this launch
    if (tile == 1 && knob == 2) return;
    pl = c;
}

}  // namespace

ConvPlan ryolo_detail::conv_plan(const ConvParams &p, int ksize, int pick, bool want_reduce) {
    ConvPlan pl;
    auto take = [&](bool accepted) {
        if (!accepted) pl = ConvPlan();      // a refused candidate leaves no trace
        pl.ksize = ksize;
        return accepted;
    };
    if (want_reduce) {
        if (pick == 0 && p.os == 1) reduce_plan(p, ksize, pl);
        pl.ksize = ksize;
        return pl;
    }
    if (pick != 0) {
        for (const ForcedPick &f : FORCED_PICKS)
            if (f.pick == pick) {
                take(forced_plan(f, p, ksize, pl));
                return pl;
            }
#ifdef RYOLO_MP_ABLATION
        if (pick >= 32 && pick < 64) {
            take(conv_mp_plan(p, (pick & 16) ? 192 : 256, ryolo_mp_ablation_variant(pick & 15), pl));
            return pl;
        }
        if (pick >= 64 && pick < 80) {
            take(conv_mq_plan(p, ryolo_mp_ablation_variant(pick & 15), pl));
            return pl;
        }
#endif
        take(igemm_plan(p, ksize, pick, p.no_persist != 0, p.force_persist != 0, false, pl));      // (no such tile: refused)
        return pl;
    }
    // auto: the first family that accepts.  The stem kernels (conv_stem.hip: 3x3 32 -> 64, and 64 -> 128 -- measurement build:
    // RYOLO_STEM64=0 keeps the 128 x 128 tiles, A/B timing)
    if (take(conv_stem_plan(p, ksize, pl))) return pl;
    const char *e64 = abl_env("RYOLO_STEM64");
    if (!(e64 && !strcmp(e64, "0")) && take(conv_stem64_plan(p, ksize, pl))) return pl;
    if (mq128_auto(p, ksize) && take(conv_mq128_plan(p, mq128_pick_bm(p), false, pl))) return pl;
    // the weight-stationary 1x1 kernel (conv_pw.hip) on the shapes it wins; RYOLO_CONV1X1 = igemm keeps the 128 x 128 tiles (A/B timing, tests)
    if (!conv_pw_disabled() && conv_pw_preferred(p) && take(conv_pw_plan(p, ksize, false, pl))) return pl;
    // 3x3 layers with 256-multiple output channels take one of the persistent multi-phase tiles (the 1x1 layers are faster on the 128 x 128
    // tiles, tools/mp_tune.py)
    if (ksize == 3 && conv_mp_eligible(p)) {
        const int bm = pick_wide_tile(p);
        if (take(bm == 0 ? conv_mq_plan(p, 0, pl) : conv_mp_plan(p, bm, 0, pl))) return pl;
    }
    // the implicit-GEMM tiles serve everything the families above refused (2 GiB slices, 2^32 pixel * extent products included)
    int tile = igemm_auto_tile(p);
    bool force = p.force_persist != 0;
    // 3x3 layers with a short K loop (C_in <= 64: at most 9 K steps) are all tile prologue / epilogue on the one-tile-per-
    // workgroup grid; the persistent 4-wave tiles prefetch the next tile's first K step under the epilogue (measured bs 32:
    // 3x3/2 32->64@304 0.339 -> 0.297 ms, 3x3 64->128@152 0.151 -> 0.136, 3x3/2 64->128@152 0.178 -> 0.165; long-K layers lose)
    // (not the statistics instantiation of the 256 x 64 tile: under the two-workgroup register cap it spills 54 VGPRs and runs
    // 2.2 x slower than the one-tile grid; with 512 registers and one workgroup per CU it is no faster than that grid either)
    if (ksize == 3 && p.os == 1 && p.fast && p.Kpad / BK <= 9 && !p.no_persist && !(p.stat_part && (p.res || tile == 2))) {
        force = true;
        if (tile == 1) tile = 7;
    }
    take(igemm_plan(p, ksize, tile, p.no_persist != 0, force, false, pl));
    return pl;
}

int ryolo_detail::conv_launch(const ConvPlan &pl, ConvParams &p, const ConvLaunch &lc) {
    if ((pl.rows > 0) != (lc.bnred != nullptr)) return RYOLO_EINVAL;
    switch (pl.kernel) {
        case RYOLO_CONV_KERNEL_MP256:
        case RYOLO_CONV_KERNEL_MP192: return launch_conv_mp(pl, p, lc);
        case RYOLO_CONV_KERNEL_MQ: return launch_conv_mq(pl, p, lc);
        case RYOLO_CONV_KERNEL_MQ128:
        case RYOLO_CONV_KERNEL_MQ64: return launch_conv_mq128(pl, p, lc);
        case RYOLO_CONV_KERNEL_DIRECT8: return launch_conv0_direct(pl, p, lc);
        case RYOLO_CONV_KERNEL_STEM0: return launch_conv0_halo(p, nullptr, 0, lc);
        case RYOLO_CONV_KERNEL_STEM: return launch_conv_stem(pl, p, lc);
        case RYOLO_CONV_KERNEL_STEM64: return launch_conv_stem64(pl, p, lc);
        case RYOLO_CONV_KERNEL_PW: return launch_conv_pw(pl, p, lc);
        default: return pl.kernel >= RYOLO_CONV_KERNEL_IGEMM ? launch_conv_igemm(pl, p, lc) : RYOLO_EINVAL;
    }
}

// ---- descriptor -> ConvParams
int ryolo_detail::conv_validate(const ryolo_conv_desc *d) {
    if (!d) return RYOLO_EINVAL;
    if (d->ksize != 1 && d->ksize != 3) return RYOLO_EINVAL;
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Cin <= 0 || d->Cout <= 0 || d->stride <= 0) return RYOLO_EINVAL;
    if ((d->Cin & 7) || (d->Cout & 7) || (d->in_cstride & 7) || (d->out_cstride & 7)) return RYOLO_EINVAL;
    if (d->in_cstride < d->Cin || d->out_cstride < d->Cout) return RYOLO_EINVAL;
    if (d->upsample != 1 && d->upsample != 2) return RYOLO_EINVAL;
    if (d->ksize == 1 && d->pad != 0) return RYOLO_EINVAL;
    return RYOLO_OK;
}

bool ryolo_detail::conv_pixels(ConvParams &p, long long Ho, long long Wo) {
    const long long M = (long long)p.N * Ho * Wo;
    if (Ho <= 0 || Wo <= 0 || M > 0x7fffffffLL - 512) return false;
    p.Ho = (int)Ho; p.Wo = (int)Wo; p.M = (int)M;
    return true;
}

// Everything of `p` the descriptor does not decide is the caller's (value-initialised: what a path does not set is zero).
bool ryolo_detail::conv_shape(const ryolo_conv_desc *d, ConvParams &p) {
    p.N = d->N; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.in_cs = d->in_cstride;
    p.stride = d->stride; p.pad = d->pad;
    p.Cout = d->Cout; p.out_cs = d->out_cstride; p.res_cs = d->res_cstride;
    p.K = d->ksize * d->ksize * d->Cin;
    p.Kpad = (p.K + BK - 1) / BK * BK;
    if (!conv_pixels(p, ((long long)d->H + 2 * d->pad - d->ksize) / d->stride + 1, ((long long)d->W + 2 * d->pad - d->ksize) / d->stride + 1)) return false;
    p.ntaps = d->ksize * d->ksize;
    for (int t = 0; t < 9; t++) { p.tap_dy[t] = t / d->ksize; p.tap_dx[t] = t % d->ksize; }
    p.os = 1; p.osx = 1; p.ooy = 0; p.oox = 0; p.OH = p.Ho; p.OW = p.Wo;
    p.act = d->act; p.slope = d->slope; p.ups = d->upsample;
    return true;
}

// Darknet-53 layer 0 as conv3x3_c8_direct_kernel / conv0_halo_kernel serve it: 3x3 / 1 pad 1, 8 (padded) -> 32 channels, rows of at
// least 16 pixels, 32-bit buffer offsets over x and y (out_cs: the pixel stride of what the launch writes)
bool ryolo_detail::conv0_shape(const ryolo_conv_desc *d, int out_cs) {
    const unsigned long long M = (unsigned long long)d->N * d->H * d->W;
    return d->ksize == 3 && d->stride == 1 && d->pad == 1 && d->Cin == 8 && d->in_cstride == 8 && d->Cout == 32 && d->upsample == 1 &&
           !(d->tile & 0x1ff) && d->W >= 16 && buffer_extent(M, 8, 8) && buffer_extent(M, out_cs, 32);
}
// ... and its launch: the two descriptors (the second one covers y), 16-pixel groups, gpw of them per wave, 4 waves per block
bool ryolo_detail::conv0_params(const ryolo_conv_desc *d, int out_cs, ConvParams &p, int gpw, unsigned *nblk) {
    if (!conv_shape(d, p) || !buffer_extent(p.M, 8, 8, &p.x_bytes) || !buffer_extent(p.M, out_cs, 32, &p.w_bytes)) return false;
    p.out_cs = out_cs; p.res_cs = 0;
    p.nt_out = (long long)p.M * 64 >= nt_out_min_bytes() ? 1 : 0;
    const long long groups = ((long long)p.M + 15) / 16, waves = (groups + gpw - 1) / gpw;
    *nblk = (unsigned)((waves + 3) / 4);
    return true;
}

// The launch behind ryolo_conv2d_bn_act_stats and ryolo_conv_kernel_choice: its ConvParams and its plan; false: the descriptor is refused.
// (The query passes stand-ins for the pointers: the plan depends only on whether residual / y / stat_part are null.)
static bool conv_forward_plan(const ryolo_conv_desc *d, const void *x, const void *w_packed, const float *scale, const float *shift,
                              const void *residual, void *y, double *stat_part, ConvParams &p, ConvPlan &pl) {
    if (conv_validate(d) != RYOLO_OK) return false;
    if (residual && ((d->res_cstride & 7) || d->res_cstride < d->Cout)) return false;
    p.x = (const __bf16 *)x;
    p.w = (const __bf16 *)w_packed;
    p.scale = scale;
    p.shift = shift;
    p.res = (const __bf16 *)residual;
    p.y = (__bf16 *)y;
    p.stat_part = stat_part;
    if (!residual && conv0_shape(d, d->out_cstride)) {
        // Darknet-53 layer 0: fragments straight from global memory (conv3x3_c8_direct_kernel); 32-bit buffer offsets
        const int gpw = (d->tile >> 16) ? (d->tile >> 16) : 32;   // groups of 16 pixels per wave (upper tile bits: tuning)
        unsigned nblk;
        if (!conv0_params(d, d->out_cstride, p, gpw, &nblk)) return false;
        p.cin_log2 = 3;
        p.stat_cpad = 128;
        // (the statistics-only pass stays on the direct kernel: 284 us against 320 for the staged one -- that pass is bound by its per-element
        // arithmetic, not by the fragment path)
        // (... and so do the statistics of the stored-z form: the two statistics passes must add the same values in the same order)
        const bool staged = conv0_halo_on() && !(d->tile >> 16) && y && !stat_part;
        pl.kernel = staged ? RYOLO_CONV_KERNEL_STEM0 : RYOLO_CONV_KERNEL_DIRECT8;
        pl.ksize = 3; pl.bm = gpw; pl.grid = (int)nblk;
        return true;
    }
    if (!conv_shape(d, p)) return false;
    p.cin_log2 = ilog2_exact(d->Cin);
    if (d->ksize == 3 && p.cin_log2 < 0 && (d->Cin % BK)) return false;
    p.taps2 = (d->Cin == 32 && d->ksize == 3) ? 1 : 0;
    p.fast = (d->Cin % BK == 0 || p.taps2) && !(d->tile & 0x100) && buffer_extent((unsigned long long)d->N * d->H * d->W, d->in_cstride, d->Cin, &p.x_bytes) &&
             buffer_extent((d->Cout + 127) / 128 * 128, p.Kpad, p.Kpad + 128, &p.w_bytes);
    if (!p.fast) p.taps2 = p.x_bytes = p.w_bytes = 0;
    p.no_persist = (d->tile & 0x200) ? 1 : 0;
    p.force_persist = (d->tile & 0x800) ? 1 : 0;
    p.pw_grid_cap = (d->tile & 0xff) == 13 ? (d->tile >> 16) & 0xff : 0;
#ifdef RYOLO_MP_ABLATION
    if ((d->tile & 0x400) && p.fast) p.x_bytes = p.w_bytes = 0;   // timing experiment: every load out of range (zeros, no traffic)
#endif
    p.nt_out = (long long)p.M * d->upsample * d->upsample * d->Cout * 2 >= nt_out_min_bytes() ? 1 : 0;
    p.stat_cpad = (d->Cout + 127) / 128 * 128;
    pl = conv_plan(p, d->ksize, pick_tile(d), false);
    return pl.kernel >= 0;
}

// a YOLO head as conv_pw.hip's decode launch sees it: 1x1 / 1, K = C_in a multiple of 64, dense output rows
static bool head_params(const ryolo_conv_desc *d, ConvParams &p) {
    if (conv_validate(d) != RYOLO_OK || d->ksize != 1 || d->stride != 1 || d->pad != 0 || d->upsample != 1 || (d->Cin % BK)) return false;
    if (!conv_shape(d, p)) return false;
    p.out_cs = d->Cout; p.res_cs = 0; p.Kpad = d->Cin;
    if (!buffer_extent(p.M, d->in_cstride, d->Cin, &p.x_bytes) || !buffer_extent((d->Cout + 127) / 128 * 128, p.Kpad, p.Kpad + 128, &p.w_bytes)) return false;
    p.fast = 1; p.use_magic = 1;
    return true;
}

extern "C" {

int ryolo_conv_stat_rows(const ryolo_conv_desc *d) {
    if (conv_validate(d) != RYOLO_OK) return 0;
    return STAT_ROWS;
}

int ryolo_conv2d_bn_act_stats(const ryolo_conv_desc *d, const void *x, const void *w_packed, const float *scale,
                              const float *shift, const void *residual, void *y, double *stat_part, void *stream_) {
    if (!x || !w_packed || !scale || !shift) return RYOLO_EINVAL;
    if (!y && !(stat_part && ryolo_conv0_recompute_supported(d))) return RYOLO_EINVAL;     // y == NULL: statistics only, layer-0 kernel only
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)w_packed | (uintptr_t)residual | (uintptr_t)scale | (uintptr_t)shift) & 15)
        return RYOLO_EINVAL;
    ConvParams p{};
    ConvPlan pl;
    if (!conv_forward_plan(d, x, w_packed, scale, shift, residual, y, stat_part, p, pl)) return RYOLO_EINVAL;
    ConvLaunch lc;
    lc.stream = (hipStream_t)stream_;
    return conv_launch(pl, p, lc);
}

int ryolo_conv2d_bn_act(const ryolo_conv_desc *d, const void *x, const void *w_packed, const float *scale,
                        const float *shift, const void *residual, void *y, void *stream_) {
    return ryolo_conv2d_bn_act_stats(d, x, w_packed, scale, shift, residual, y, nullptr, stream_);
}

int ryolo_conv_kernel_choice(const ryolo_conv_desc *d, int with_residual, int with_statistics) {
    void *fake = (void *)(uintptr_t)4096;      // never dereferenced: nothing is launched
    ConvParams p{};
    ConvPlan pl;
    return conv_forward_plan(d, fake, fake, (const float *)fake, (const float *)fake, with_residual ? fake : nullptr, fake,
                             with_statistics ? (double *)fake : nullptr, p, pl)
               ? pl.kernel
               : -1;
}

int ryolo_conv_head_decode_supported(const ryolo_conv_desc *d, int na, int no) {
    ConvParams p{};
    return head_params(d, p) && conv_pw_decode_supported(p, na, no) ? 1 : 0;
}

int ryolo_conv_head_decode(const ryolo_conv_desc *d, const void *x, const void *w_packed, const float *scale, const float *shift,
                           const float *anchors, int na, int no, float stride, float context_factor, int arc, float *io,
                           long long io_rows_per_image, long long io_row_offset, float *pout, void *stream_) {
    ConvParams p{};
    if (!x || !w_packed || !scale || !shift || !anchors || !io || !head_params(d, p) || !conv_pw_decode_supported(p, na, no)) return RYOLO_EINVAL;
    if (arc < 0 || arc > 2 || !(stride > 0.f) || !(context_factor > 0.f)) return RYOLO_EINVAL;
    if (((uintptr_t)x | (uintptr_t)w_packed) & 15) return RYOLO_EINVAL;
    p.x = (const __bf16 *)x; p.w = (const __bf16 *)w_packed; p.scale = scale; p.shift = shift;
    return launch_conv_pw_decode(p, io, io_rows_per_image, io_row_offset, pout, anchors, na, no, stride, context_factor, arc, (hipStream_t)stream_);
}

int ryolo_conv_head_decode_store(const ryolo_conv_desc *d, const void *x, const void *w_packed, const float *scale, const float *shift,
                                 int na, int no, void *head, int head_cstride, float *pout, void *stream_) {
    ConvParams p{};
    if (!x || !w_packed || !scale || !shift || !head || !pout || !head_params(d, p) || !conv_pw_decode_supported(p, na, no)) return RYOLO_EINVAL;
    if (((uintptr_t)x | (uintptr_t)w_packed) & 15) return RYOLO_EINVAL;
    p.x = (const __bf16 *)x; p.w = (const __bf16 *)w_packed; p.scale = scale; p.shift = shift;
    return launch_conv_pw_decode(p, nullptr, 0, 0, pout, nullptr, na, no, 1.f, 1.f, 0, (hipStream_t)stream_, head, head_cstride);
}

int ryolo_conv_pair_supported(const ryolo_conv_desc *first, const ryolo_conv_desc *second, int shortcut_from_input) {
    if (conv_validate(first) != RYOLO_OK || conv_validate(second) != RYOLO_OK) return 0;
    return conv_stem_pair_kind(first, second, shortcut_from_input) != 0 ? 1 : 0;
}

int ryolo_conv2d_bn_act_pair(const ryolo_conv_desc *a, const ryolo_conv_desc *b, const void *x, const void *w_first, const float *scale_first,
                             const float *shift_first, const void *w_second, const float *scale_second, const float *shift_second,
                             int shortcut_from_input, void *y, void *stream_) {
    if (conv_validate(a) != RYOLO_OK || conv_validate(b) != RYOLO_OK || !x || !w_first || !scale_first || !shift_first || !w_second || !scale_second ||
        !shift_second || !y)
        return RYOLO_EINVAL;
    const int kind = conv_stem_pair_kind(a, b, shortcut_from_input);
    if (!kind) return RYOLO_EINVAL;
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)w_first | (uintptr_t)w_second) & 15) return RYOLO_EINVAL;
    ConvParams p{};           // the second layer; its input is the first layer's output in LDS: dense, never in memory
    if (!conv_shape(b, p)) return RYOLO_EINVAL;
    p.w = (const __bf16 *)w_second; p.scale = scale_second; p.shift = shift_second; p.y = (__bf16 *)y;
    p.in_cs = b->Cin; p.res_cs = 0;
    p.nt_out = (long long)p.M * b->Cout * 2 >= nt_out_min_bytes() ? 1 : 0;
    const unsigned long long xb = (((unsigned long long)a->N * a->H * a->W - 1) * a->in_cstride + a->Cin) * 2ull;   // (< 2^31: conv_stem_pair_kind)
    const int kpad_first = (a->ksize * a->ksize * a->Cin + BK - 1) / BK * BK;
    return launch_conv_stem_pair(kind, p, x, (unsigned)xb, a->in_cstride, a->H, a->W, w_first, kpad_first, scale_first, shift_first, a->act,
                                 a->slope, (hipStream_t)stream_);
}

int ryolo_conv0_recompute_supported(const ryolo_conv_desc *d) {
    return conv_validate(d) == RYOLO_OK && conv0_shape(d, d->out_cstride) ? 1 : 0;
}

}  // extern "C"
