// Which kernel a launch runs, decided on the host BEFORE the launch: tile shapes, kernel families and flag words of the split-fp16
// GEMMs, the row tile of the GEMM + LayerNorm kernels, the variant of the attention kernels.  Host code only - no kernel lives here.
// The planner makes these plans once per call and chunk size (jmid_planner.hip::plan_step), a diagnostics entry point once per
// launch; the launchers of the kernel headers execute them and decide nothing.  Every rule reads its knobs from an explicit Tuning.
#pragma once
#include "common.hpp"

namespace jmid {

enum GemmEpi { EPI_BIAS = 0, EPI_BIAS_RELU = 1, EPI_CSL = 2 };
enum GemmOut { OUT_F32 = 0, OUT_SPLIT = 1, OUT_QKV = 2, OUT_LNX = 4 };     // OUT_LNX (gemm_small.hpp only): + residual + LayerNorm, every workgroup normalising its own
                                                                        // 64 columns after exchanging the row statistics with the seven others of its row tile

// What a call knows before its first launch and no chunk of it changes (run_network).  Facts, not knobs: jmid_set_tuning has no say.
struct CallFacts {
    // the small-launch GEMMs (gemm_small.hpp: one workgroup per CU, most of its LDS): 1 = one chunk in flight, 0 = several (their
    // launches would collide: 4 episodes as 2 x 2 measured 4 % slower with them), 2 = experiment "small_lanes" = 2: only the
    // two-workgroups-per-CU shape.  (A single launch on an idle handle: 1.)
    int small_now = 1;
    // the call is ONE chunk, run eagerly (OUT_LNX of gemm_small.hpp only then, whatever the lanes: a call's bits do not depend on
    // its chunk plan; a captured loop would replay that kernel's launch tags)
    int one_chunk = 1;
    int attn_nsplit = 1;      // split-KV factor of the attention launches: per call, never per chunk (run_network)
    int qkv0_steps = 1;       // steps a chunk's coefficient table of layer 0 holds (qkv0.hpp): all of the call's, or 1 = rebuilt at the head of every step
    int tail_steps = 1;       // the same for the folded tail's table of 2 x d maps (tail_fold.hpp)
};

// the arithmetic of a split-fp16 GEMM: a template parameter of every kernel (a run-time flag in the K loops cost F16X3 4 %)
enum GemmMode { GM_X3 = 0, GM_X2 = 1, GM_MX = 2 };      // (the values of gemm_small.hpp's SmallMode)

enum GemmShape {
    GS_NONE = 0,              // OUT_LNX only: the launch does not fit the chip (the caller takes GEMM + add_ln)
    // launches of at most one workgroup per CU (gemm_small.hpp): 64-row tiles, 64 or 128 columns; _TWO: two workgroups per CU
    GS_SMALL_64x64, GS_SMALL_64x128, GS_SMALL_64x128_TWO,
    GS_SMALL_64x64_TWO,       // (OUT_LNX at 33 ... 64 row tiles)
    // the LDS-DMA kernels of gemm_f16x3.hpp (F16X3 / F16X2: gemm_f16x3_dma*_kernel; F16MX: gemm_mx_kernel)
    GS_64, GS_128, GS_256x128, GS_256x256,
    GS_128x256, GS_256x256_NS3,      // diagnostics flavour, F16MX: 128 x 256 two per CU, 256 x 256 with a three-stage ring
    GS_REG_64, GS_REG_128,    // register-staged (gemm_f16x3_kernel; F16X3 / F16X2 only)
};
constexpr int gemm_shape_bm(GemmShape s) {
    return s == GS_256x128 || s == GS_256x256 || s == GS_256x256_NS3 ? 256 : s == GS_128 || s == GS_128x256 || s == GS_REG_128 ? 128 : 64;
}
constexpr int gemm_shape_bn(GemmShape s) {
    return s == GS_256x256 || s == GS_128x256 || s == GS_256x256_NS3 ? 256
           : s == GS_SMALL_64x64 || s == GS_SMALL_64x64_TWO || s == GS_64 || s == GS_REG_64 ? 64 : 128;
}
constexpr bool gemm_shape_small(GemmShape s) { return s >= GS_SMALL_64x64 && s <= GS_SMALL_64x64_TWO; }

// Is there a kernel of this shape for the mode and epilogue?  THE list of what is not instantiated:
//   * 256 x 256 / 128 x 256 accumulators next to the ConcatSquash epilogue spill;
//   * so does F16MX's 256 x 128 with the ConcatSquash epilogue into fp32 (concat4: N = 128, never enough tiles for it);
//   * two small workgroups per CU: not F16X3 (two k64 stages of its four operand planes do not fit half a CU's LDS); with the
//     LayerNorm inside, F16MX only;
//   * the register-staged kernels are F16X3 / F16X2's (no fp8 path), the diagnostics shapes F16MX's.
constexpr bool gemm_shape_built(GemmMode mode, int epi, int out, GemmShape s) {
    switch (s) {
        case GS_SMALL_64x64: return true;
        case GS_SMALL_64x128: return out != OUT_LNX;
        case GS_SMALL_64x128_TWO: return out != OUT_LNX && mode != GM_X3;
        case GS_SMALL_64x64_TWO: return out == OUT_LNX && mode == GM_MX;
        case GS_64:
        case GS_128: return out != OUT_LNX;
        case GS_256x128: return out != OUT_LNX && !(mode == GM_MX && epi == EPI_CSL && out == OUT_F32);
        case GS_256x256: return out != OUT_LNX && epi != EPI_CSL;
        case GS_128x256:
        case GS_256x256_NS3: return out != OUT_LNX && epi != EPI_CSL && mode == GM_MX;
        case GS_REG_64:
        case GS_REG_128: return out != OUT_LNX && mode != GM_MX;
        default: return false;
    }
}

// One split-fp16 GEMM launch.  flags: the word its kernel decodes (gemm_flags; F16X3 / F16X2 large tiles: only 256 x 256 takes
// one, bits 0-1).  group_tiles: N-tiles per column group of the XCD tile order (small launches: always set; F16MX large tiles:
// 0 = N fastest over all N-tiles, "gemm_pn"; F16X3 / F16X2 256 x 128: N-tiles per L2 group, 0 = auto, "gemm_ng"; 0 elsewhere).
// abl: timing ablations (-DJMID_ABLATIONS only).
struct GemmPlan {
    GemmMode mode;
    GemmShape shape;
    int flags, group_tiles, abl;
};

constexpr int kLnxMaxTiles = 64;      // row tiles of an OUT_LNX launch: its exchange buffer (gemm_small.hpp, SM_LNX_MAX_TILES)

// Does this GEMM run on the small-launch kernel, and in which shape?  One workgroup per CU: at most 256 tiles.  "gemm_small": 0 auto,
// 1 never, 2 only up to one workgroup per CU.
// OUT_LNX - out_proj / linear2 + residual + LayerNorm as ONE small launch with the statistics exchange (N = 512: 8 workgroups per
// 64-row tile) -: nothing else in flight on the handle (small_now == 1), calls of ONE chunk (whatever the lanes, a call's bits must
// not depend on its chunk plan), and EVERY workgroup of the launch resident at once - the waiting workgroups need their partners:
// against the device's compute units (Tuning::cus, from the device at jmid_create - a partitioned or smaller device takes the
// unfused pair), one per CU, or two per CU on half the LDS each ("small_lnx2" = 2 off), and at most kLnxMaxTiles row tiles.
// "small_lnx" = 2: off (GEMM + add_ln2, the same bits).
inline GemmShape small_gemm_shape(GemmMode mode, int out, int M, int N, int K, const CallFacts& cf, const Tuning& t) {
    if (t.gemm_small == 1 || t.gemm_h_variant != 0 || !cf.small_now || K % 128 != 0) return GS_NONE;       // (k128 ring stages)
    const long ntm = (M + 63) / 64;
    if (out == OUT_LNX) {
        if (cf.small_now != 1 || cf.one_chunk != 1 || t.small_lnx == 2 || ntm > kLnxMaxTiles) return GS_NONE;
        if (ntm * 8 <= t.cus) return GS_SMALL_64x64;
        return gemm_shape_built(mode, 0, out, GS_SMALL_64x64_TWO) && ntm * 8 <= 2L * t.cus && t.small_lnx2 != 2 ? GS_SMALL_64x64_TWO : GS_NONE;
    }
    if (N % 128 != 0) return GS_NONE;
    // 257 ... 512 tiles of 64 x 128 (two scenes; the reference's shipped K = 100): the same kernel, two workgroups per CU
    // (F16X3 at 257 ... 512 tiles in two rounds of one workgroup per CU measured slower than the round-3 kernels: 0.996 vs 0.977 ms
    //  per shipped-point call)
    const bool two = gemm_shape_built(mode, 0, out, GS_SMALL_64x128_TWO) && ntm * (N / 128) <= 512;
    if (cf.small_now == 2) return two ? GS_SMALL_64x128_TWO : GS_NONE;      // (experiment "small_lanes" = 2)
    if (ntm * (N / 64) <= 256) return GS_SMALL_64x64;
    if (ntm * (N / 128) <= 256) return GS_SMALL_64x128;
    return two && t.gemm_small != 2 ? GS_SMALL_64x128_TWO : GS_NONE;
}

// The tile shape of a launch that fills the chip.  "gemm_h_variant": 0 auto, 1 = 64 x 64 register-staged, 2 = 128 x 128
// register-staged, 3 = 128 x 128, 4 = 256 x 128, 5 = 64 x 64, 6 = 256 x 256 (N % 256 == 0), 7 / 8 = the diagnostics shapes; a forced
// shape that is not built for the mode and epilogue leaves the choice to the automatic rule.
inline GemmShape large_gemm_shape(GemmMode mode, int epi, int out, int M, int N, const Tuning& t) {
    const auto usable = [&](GemmShape s) { return gemm_shape_built(mode, epi, out, s) && N % gemm_shape_bn(s) == 0; };
    constexpr GemmShape forced[9] = {GS_NONE, GS_REG_64, GS_REG_128, GS_128, GS_256x128, GS_64, GS_256x256, GS_128x256, GS_256x256_NS3};
    const GemmShape f = forced[t.gemm_h_variant >= 0 && t.gemm_h_variant <= 8 ? t.gemm_h_variant : 0];
    if (f != GS_NONE && gemm_shape_built(mode, epi, out, f) && (gemm_shape_bn(f) != 256 || N % 256 == 0)) return f;
    const long mt256 = (M + 255) / 256, big = (long)((M + 127) / 128) * ((N + 127) / 128);
    if (big < 256) return GS_64;
    // a coarser grid unless it quantises badly onto the 256 CUs (one workgroup per CU)
    const auto eff = [](long nb) { return (double)nb / (double)(((nb + 255) / 256) * 256); };
    const long nb256 = mt256 * ((N + 127) / 128);
    // 256 x 256 when N allows it (in_proj, linear1) and the grid still fills the chip - also below one workgroup per CU from
    // `rows` rows: two chunks are in flight, and the larger tile moves a third fewer operand bytes per FLOP.  F16MX from 7168
    // (2 x 12 episodes per call 60.6 vs 67.6 ms, 2 x 8: 45.1 vs 47.4, 2 x 6 equal, 2 x 5: 35.8 vs 33.4; tools/single_scene_sweep.py
    // gemm_h_variant=0,6 f16mx E), F16X2 / F16X3 from 12288 (2 x 12 episodes 76.0 vs 79.7 ms in F16X2, 102.2 vs 107.5 in F16X3;
    // 2 x 8: within 1 %)
    const int rows = mode == GM_MX ? 7168 : 12288;
    if (usable(GS_256x256)) {
        const long nbq = mt256 * (N / 256);
        if ((nbq >= 256 && 1.2 * eff(nbq) >= eff(nb256)) || (nbq < 256 && M >= rows)) return GS_256x256;
    }
    if (gemm_shape_built(mode, epi, out, GS_256x128) && nb256 >= 256 && 1.2 * eff(nb256) >= eff(big)) return GS_256x128;
    return GS_128;
}

// The flag word of the GEMM kernels, from the knobs.  Large tiles - bits 0-1: V^T (1) and Q / K (2) tiles out through LDS in full
// rows ("vt_stage": 0 / 1 both, 2 neither, 3 V^T only); bit 4: linear1's tile out through LDS ("h1_stage" = 2 off).  Small
// launches - bit 4 SET: the generic epilogue instead of Q / K through LDS ("small_qk" = 2).  Both - bit 2: transposed product +
// row-wise epilogue for the ConcatSquash GEMMs, bit 3: for linear1 too ("csl_swap": 2 neither, 3 both).
inline int gemm_flags(const Tuning& t, bool small) {
    const int csl = (t.csl_swap == 2 ? 0 : 4) | (t.csl_swap == 3 ? 8 : 0);
    if (small) return csl | (t.small_qk == 2 ? 16 : 0);
    return (t.vt_stage == 2 ? 0 : (t.vt_stage == 3 ? 1 : 3)) | csl | (t.h1_stage == 2 ? 0 : 16);
}

// column groups of a small launch by the bytes all eight XCDs pull from the Infinity Cache with pn of them: every XCD its column
// group's share of W and the A rows of its part of the M range
inline int small_pick_groups(int M, int N, int K, int ntn, double w_bytes_per_el, double a_bytes_per_el) {
    const double wb = (double)N * K * w_bytes_per_el, ab = (double)M * K * a_bytes_per_el;
    int best = 1;
    double best_bytes = 8.0 * wb + ab;
    for (int pn = 2; pn <= 8; pn *= 2) {
        if (ntn % pn != 0) break;
        const double bytes = 8.0 * wb / pn + pn * ab;
        if (bytes < best_bytes) {
            best = pn;
            best_bytes = bytes;
        }
    }
    return best;
}

// THE function that plans a split-fp16 GEMM launch.  want: the mode of the call, GM_MX only where the weight has its bf8 image.
// Every shape of F16MX has its fp8-correction kernel for N a multiple of 128 and K of 64 (all of the net's GEMMs at d_model 512);
// anything else, and the register-staged shapes a knob can force, run F16X2's kernels.
inline GemmPlan plan_gemm(GemmMode want, int epi, int out, int M, int N, int K, const CallFacts& cf, const Tuning& t) {
    GemmPlan p{};
    const bool mx_ok = K % 64 == 0 && N % 128 == 0 && t.gemm_h_variant != 1 && t.gemm_h_variant != 2;
    p.mode = want == GM_MX && !mx_ok ? GM_X2 : want;
    p.abl = gemm_abl_bits(t);
    p.shape = small_gemm_shape(p.mode, out, M, N, K, cf, t);
    const bool small = p.shape != GS_NONE;
    if (!small && out != OUT_LNX) p.shape = large_gemm_shape(p.mode, epi, out, M, N, t);
    if (p.shape == GS_NONE) return p;
    p.flags = small || p.mode == GM_MX ? gemm_flags(t, small) : p.shape == GS_256x256 ? gemm_flags(t, false) & 3 : 0;
    const int ntn = N / gemm_shape_bn(p.shape);
    if (small) {
        const int pn = t.small_pn > 0 ? (ntn % t.small_pn == 0 ? t.small_pn : 1)
                                      : small_pick_groups(M, N, K, ntn, p.mode == GM_MX ? 3.0 : 4.0, p.mode == GM_X3 ? 4.0 : 2.0);
        p.group_tiles = ntn / pn;
    } else if (p.mode == GM_MX) {
        p.group_tiles = t.gemm_pn > 1 && ntn % t.gemm_pn == 0 ? ntn / t.gemm_pn : 0;
    } else if (p.shape == GS_256x128) {
        p.group_tiles = t.gemm_ng;
    }
    return p;
}

// Row tile of the row-complete GEMM + LayerNorm kernels (N = 512).  First generation (gemm_ln_f16x3.hpp): by how well the grid
// fills whole rounds of the 256 CUs (one workgroup per CU); at equal fill the 128-row kernel is ~4 % faster (W streams through
// L2 -> LDS half as often).  Second generation (gemm_ln2_mx.hpp): 128 rows; the 64-row shape (two workgroups per CU; measured
// 10 % slower on full launches, and hipcc spills 48 registers in it) exists in the diagnostics flavour only, behind "ln_rows".
inline int plan_ln_rows(bool second_generation, int M, const Tuning& t) {
    if (second_generation) return t.ln_rows == 64 ? 64 : 128;
    const auto fill = [](long n) { return (double)n / (double)(((n + 255) / 256) * 256); };
    const long n128 = (M + 127) / 128, n64 = (M + 63) / 64;
    return t.ln_rows == 128 || (t.ln_rows == 0 && 1.04 * fill(n128) >= fill(n64)) ? 128 : 64;
}

// One attention launch of the split-fp16 modes (attn_f16x3.hpp) or of the exact-fp32 kernel (attn_f32.hpp: `pack` only).
struct AttnPlan {
    bool dma;            // head_dim 128: the LDS-DMA kernel ("attn_h_variant" = 1: the register-staged one, which does not split)
    bool p1, pf;         // F16X2 / F16MX: one fp16 plane of P ("attn_mx" = 1: P_hi + P_lo); its fragment reads three steps ahead ("attn_pf" = 2: one)
    bool old_softmax;    // diagnostics flavour, "attn_sm" = 2: the round 2-5 softmax (A/B; other bits, same softmax)
    bool one_wg;         // (probe) the CU's whole 160 KB of LDS: one workgroup per CU
    int prio;            // AttnHArgs::prio
    int abl;             // timing ablations (-DJMID_ABLATIONS only)
    int bystander_lds;   // dynamic LDS of the split-KV merge kernel (common.hpp::bystander_lds)
    bool pack;           // exact-fp32 kernel: several short sequences (S <= 16) per wave
    bool masked;         // a padded call (padded.hpp): the MASK instantiations, key-mask words in AttnArgs::mask / AttnHArgsM::mask
};
inline AttnPlan plan_attn(int head_dim, const Tuning& t) {
    AttnPlan p{};
    p.dma = head_dim == 128 && t.attn_h_variant != 1;
    p.p1 = t.attn_mx != 1;
    p.pf = t.attn_pf != 2;
    p.old_softmax = t.attn_sm == 2;
    p.one_wg = t.attn_one_wg != 0;
    p.prio = t.attn_prio;
    p.abl = attn_abl_bits(t);
    p.bystander_lds = t.bystander_lds;
    p.pack = t.attn_pack != 0;
    return p;
}

// The masked LDS-DMA kernel exists as the instantiation the default plan picks for each of F16X3, F16X2 and F16MX (with or without the
// bf8 K images): in no mode with the round 2-5 softmax ("attn_sm" = 2) or the timing ablations, and in the two-term modes (x2: F16X2 /
// F16MX) neither with P_hi + P_lo ("attn_mx" = 1) nor with the one-step fragment reads ("attn_pf" = 2) - F16X3 has one instantiation,
// which those two knobs do not select.  A padded call under such a knob is JMID_EINVAL.
inline bool attn_masked_built(const AttnPlan& p, bool x2) { return !p.dma || (!p.old_softmax && !p.abl && (!x2 || (p.p1 && p.pf))); }

// does the out-projection's OUT_LNX launch also merge the partial outputs of a split-KV attention launch (lnx_combine)?  "small_cmb": 0 on, 2 off
inline bool small_cmb_fits(const AttnPlan& ap, int nsplit, int x2, const Tuning& t) {
    return t.small_cmb != 2 && ap.dma && nsplit > 1 && nsplit <= 8 && x2;
}

}  // namespace jmid
