// Which kernel form a keds_gemm_bt* / keds_gemm_x3 call gets: the one place that decides.  Host C++ without a HIP header, a
// device call or a getenv, so that a plain host compiler builds it into a stand-alone program; gemm.hip launches what
// gemm_plan() returns, keds_gemm_plan_query (keds_hip.h) answers from it without a GPU, and tests/test_host_gemm_plan.py holds it
// against a Python model and against the form table of docs/kernels.md.
#pragma once
#include <stddef.h>
#include "../../include/keds_hip.h"
#include "../../include/keds_knowledge_f16.h"      // ids 32-34: the knowledge stream's fp16 epilogues

namespace {

// ---- epilogue classes ------------------------------------------------------------------------------------------------
// KEDS_EPI_LN_*_H: the same epilogues with fp16 operands (A = the fp16 residual stream, W' folded to fp16)
// KEDS_EPI_X3_*: split-operand GEMMs (keds_hip.h): fp16 MFMA, three K segments (hi.hi, hi.lo, lo.hi) over two operand planes
constexpr bool epi_x3(int e) { return e == KEDS_EPI_X3_BIAS_F32 || e == KEDS_EPI_X3_RESID_F32 || e == KEDS_EPI_X3_QGELU_PAIR; }
// KEDS_EPI_*_F16_H / *_F32_H ("fp16" operating point): fp16 A and W; the LN / QuickGELU forms store fp16 (range-guarded)
constexpr bool epi_ln_h(int e) {
    return e == KEDS_EPI_LN_BIAS_BF16_H || e == KEDS_EPI_LN_QGELU_BF16_H || e == KEDS_EPI_LN_BIAS_F16_H || e == KEDS_EPI_LN_QGELU_F16_H;
}
// the knowledge stream's fp16 ids (32..34, keds_knowledge_f16.h): 128^2 kernel forms only
constexpr bool epi_kf16(int e) { return e == KEDS_EPI_BIAS_F16_H || e == KEDS_EPI_BIAS_RELU_F16_H || e == KEDS_EPI_BIAS_F16_H_HEADF32; }
constexpr bool epi_h16(int e) {        // the fp16 operating point's own ids (16..22, 32..34)
    return e == KEDS_EPI_LN_BIAS_F16_H || e == KEDS_EPI_LN_QGELU_F16_H || e == KEDS_EPI_RESID_STATS_F16_H || e == KEDS_EPI_BIAS_RESID_F32_H ||
           e == KEDS_EPI_BIAS_QGELU_F16_H || e == KEDS_EPI_PATCH_F32_H || e == KEDS_EPI_BIAS_F32_H || epi_kf16(e);
}
constexpr bool epi_f16(int e) { return epi_ln_h(e) || epi_x3(e) || epi_h16(e); }          // fp16 (not bf16) MFMA operands
constexpr bool epi_is_ln(int e) { return e == KEDS_EPI_LN_BIAS_BF16 || e == KEDS_EPI_LN_QGELU_BF16 || epi_ln_h(e); }
// the fp16-residual epilogue (residual stream read-modify-written in fp16 + row statistics), bf16 or fp16 A / W
constexpr bool epi_resid16(int e) { return e == KEDS_EPI_RESID_STATS_F16 || e == KEDS_EPI_RESID_STATS_F16_H; }
// library-internal: the plain fp16-output store the LN-folded fp16 epilogue ends in (its public name: KEDS_EPI_BIAS_F16_H)
constexpr int EPI_INT_BIAS_F16 = 100;
constexpr int epi_base(int e) {
    return (e == KEDS_EPI_LN_BIAS_BF16 || e == KEDS_EPI_LN_BIAS_BF16_H)     ? KEDS_EPI_BIAS_BF16
           : (e == KEDS_EPI_LN_QGELU_BF16 || e == KEDS_EPI_LN_QGELU_BF16_H) ? KEDS_EPI_BIAS_QGELU_BF16
           : e == KEDS_EPI_LN_BIAS_F16_H || e == KEDS_EPI_BIAS_F16_H        ? EPI_INT_BIAS_F16
           : e == KEDS_EPI_LN_QGELU_F16_H                                   ? KEDS_EPI_BIAS_QGELU_F16_H
           : e == KEDS_EPI_X3_BIAS_F32 || e == KEDS_EPI_BIAS_F32_H          ? KEDS_EPI_BIAS_F32
           : e == KEDS_EPI_X3_RESID_F32 || e == KEDS_EPI_BIAS_RESID_F32_H   ? KEDS_EPI_BIAS_RESID_F32
           : e == KEDS_EPI_PATCH_F32_H                                      ? KEDS_EPI_PATCH_F32
                                                                            : e;
}
constexpr bool epi_qgelu(int e) { return epi_base(e) == KEDS_EPI_BIAS_QGELU_BF16 || epi_base(e) == KEDS_EPI_BIAS_QGELU_F16_H; }
// epilogues that store fp16 values: the range guard applies (|v| > 65504 or non-finite raises the numerics-guard flag)
constexpr bool epi_out_f16(int e) {
    return epi_base(e) == EPI_INT_BIAS_F16 || epi_base(e) == KEDS_EPI_BIAS_QGELU_F16_H || e == KEDS_EPI_BIAS_RELU_F16_H ||
           e == KEDS_EPI_BIAS_F16_H_HEADF32;
}

// ---- switches ------------------------------------------------------------------------------------------------------------
// Everything that steers the decision besides the call's own arguments.  The defaults are the product's; keds_gemm_force_small
// (tests, A/B tools) changes them (gemm.hip keeps the instance).
struct GemmSwitches {
    bool force_small = false;       // bit 0: everything on the 128^2 kernel
    bool no_split = false;          // bit 9: no split-K anywhere
    bool resid_prologue = false;    // bit 10: 8-wave kernel, fp16-residual epilogues: residual + bias as the accumulators' initial value
                                    // (built, bit-compatible within the fp32 addition order and SLOWER: out-proj 75.5 vs 73.0 us, c_proj
                                    // 232.4 vs 229.0 -- tools/ab_resid_prologue.py; off)
    int quad = -1;                  // bits 11-12: 256^2 tiles on the 4-wave kernel: -1 by shape, 0 never, 1 always with
                                    // one tile per workgroup, 2 always, persistent where the launch allows it
    bool quad3 = true;              // bit 16 clears it: 4-wave kernel, fp16-residual epilogues: three-deep A ring
    bool quad_defer = true;         // bit 17 clears it: persistent 4-wave kernel, LayerNorm epilogues: 12 of a tile's
                                    // 32 stores per lane wait for the next K-loop
    int resid_quad_min_k = 1024;    // fp16-residual GEMMs go to the 4-wave kernel from this K on (round 4: out-proj too,
                                    // +0.35 % on the headline: its A operand is cold in the step and the three-deep ring tolerates that)
    bool x3_quad = true;            // the split-operand GEMMs on the 4-wave kernel
    int big_tiles_pct = 85;         // the fill of its CU-rounds a 256^2 launch needs
    bool small_lds = false;         // every 128^2 launch takes the 64 KiB-LDS form
};

// the argument of keds_gemm_force_small over `base` (the defaults); bits 8 and 13-15 are refused before this is called
inline GemmSwitches gemm_switches_decode(int bits, const GemmSwitches& base) {
    GemmSwitches s = base;
    s.force_small = bits & 1;
    s.no_split = base.no_split || ((bits >> 9) & 1);
    s.resid_prologue = (bits >> 10) & 1;
    const int q = (bits >> 11) & 3;                       // 0 = by shape, 3 = never
    if (q) s.quad = q == 3 ? 0 : q;
    s.quad3 = !((bits >> 16) & 1);
    s.quad_defer = base.quad_defer && !((bits >> 17) & 1);
    return s;
}

// ---- the plan ------------------------------------------------------------------------------------------------------------
struct GemmPlan {
    struct Part {
        int form = KEDS_GEMM_FORM_NONE;     // KEDS_GEMM_FORM_*
        int ring = 0;                       // K-tiles of the A operand in flight; the 128^2 kernel's ring template argument
        int splits = 0;                     // split-K slices (1: no split, no reduce kernel)
        int rows = 0;
        // the main launch only
        int persistent = 0;                 // one workgroup per CU walks the tiles ...
        int workgroups = 0;                 // ... this many of them: T = min(cus, 256) & ~7 (whole XCD groups)
        int defer = 0;                      // the persistent kernel's aux_i for the LayerNorm epilogues: deferred stores on (whatever K is)
        int flags = 0;                      // KEDS_GEMM_FLAG_*
    };
    Part main;      // all rows, or the full 256-row tiles
    Part tail;      // the M % 256 remainder rows behind a 256^2 main launch, on the 128^2 kernel
    // the layout of keds_gemm_last_launch
    void info(int out[8]) const {
        const int v[8] = {main.form, tail.form, main.ring, tail.ring, main.splits, tail.splits, main.persistent, main.flags};
        for (int i = 0; i < 8; ++i) out[i] = v[i];
    }
};

// 256^2 tiles at all.  The 256^2 kernels run one workgroup per CU: their full tiles must keep >= 85 % of the CU-rounds busy (a
// single round counts: 19,712 x 768 x 3072 runs at 1.13 PF on 231 tiles vs 0.96 on 924 tiles of 128^2); otherwise the 128^2
// kernel's finer tiles quantise better.
// (round 5) A launch whose rows are whole 256-row tiles (no remainder launch behind it) and whose K-loop is short needs only HALF
// of its last round filled: the 128^2 kernel's alternative is four times the workgroups on 512 slots, and 11,008 x 768 x 768 (the
// dual workload's 2B-row text pass at 43 columns: 516 workgroups, four more than fit at once) pays a whole second round for
// them -- 60 us against 30 on 129 tiles of 256^2; in_proj 61 -> 43, c_fc 82 -> 70.  Not for long K (c_proj, K = 3072: 76 us on the
// one-tile-per-workgroup kernel against 60).  profiles/r05_text_big_tiles_ab.txt
inline bool gemm_big_tiles_fill(int M, int N, int K, const GemmSwitches& sw) {
    const long bt = (long)(M / 256) * (N / 256);
    const long rounds = (bt + 255) / 256;
    int pct = sw.big_tiles_pct;
    if (pct == 85 && M % 256 == 0 && K <= 1024) pct = 50;
    return !sw.force_small && N % 256 == 0 && K % 64 == 0 && K >= 128 && bt > 0 && bt * 100 >= rounds * 256 * pct;
}
inline bool gemm_big_tiles(int epi, int M, int N, int K, long long lda, long long ldc, const GemmSwitches& sw) {
    return gemm_big_tiles_fill(M, N, K, sw) && lda == K && ldc == N && (epi_base(epi) != KEDS_EPI_PATCH_F32 || M % 256 == 0) &&
           epi != KEDS_EPI_BIAS_BF16_HEADF32 &&    // (its fp32 head rows are numbered from row 0 of the launch)
           !epi_kf16(epi);                         // (the knowledge stream fills under 85 % of a 256^2 round: no 256^2 kernel is built for them)
}

// 256^2 tiles on the 4-wave kernel (0: the 8-wave kernel, 1: one tile per workgroup, 2: persistent where the launch allows it).
// Same-process A/B on the ViT-L/14 shapes at B = 128 (tools/ab_quad.py, medians of 5 x 20 launches, round 3; 8 waves /
// 4 waves / 4 waves persistent, us): qkv 189.4 / 184.1 / 179.2, c_fc 243.6 / 239.5 / 236.3, c_proj 216.3 / 214.7 / (212.5),
// out-proj 66.3 / 67.7 / -- : the 4-wave kernel wins where the K-loop dominates the tile and its persistent form where the
// LayerNorm epilogues (no loads of their own) leave registers for the tile loop.
inline int gemm_quad_mode(int epi, int K, const GemmSwitches& sw) {
    if (sw.quad >= 0) return sw.quad;
    const bool by_shape = epi_is_ln(epi)     ? K >= 512
                          : epi_resid16(epi) ? K >= sw.resid_quad_min_k
                          : epi_x3(epi)      ? sw.x3_quad      // a K-loop of 3 K / 64 K-tiles: the form that wins where the K-loop dominates
                                             : false;
    return by_shape ? 2 : 0;
}

// a 128^2 launch of `rows` rows that splits K if the scratch allows it: too few tiles to fill 256 CUs, so that ~128+ workgroups
// stream the weights in parallel (at K = 1024 the second launch costs what the split saves)
inline bool gemm_may_split(int epi, int rows, int N, int K, const GemmSwitches& sw) {
    const long tiles = (long)((rows + 127) / 128) * (N / 128);
    return tiles <= 64 && K >= 2048 && !sw.no_split && !epi_x3(epi);
}

inline GemmPlan::Part gemm_plan_small(int epi, int rows, int N, int K, size_t splitk_bytes, bool small_lds, const GemmSwitches& sw) {
    GemmPlan::Part p;
    p.form = KEDS_GEMM_FORM_SMALL;
    p.rows = rows;
    p.splits = 1;
    const long m_tiles = (rows + 127) / 128, tiles = m_tiles * (N / 128);
    small_lds = small_lds || sw.small_lds;
    if (gemm_may_split(epi, rows, N, K, sw)) {
        int splits = 1;
        while (splits < 16 && tiles * splits * 2 <= 256 && K % (splits * 2 * 64) == 0 && K / (splits * 2) >= 128) splits *= 2;
        if (splits > 1 && (size_t)splits * (m_tiles * 128) * N * sizeof(float) <= splitk_bytes) {
            p.splits = splits;
            p.ring = small_lds ? 2 : 4;
            return p;
        }
    }
    // fewer workgroups than 2 per CU: nothing else hides the DMA latency, so use the deep ring -- unless the launch is meant to run
    // BESIDE another kernel's workgroups (small_lds: the towers' remainder-row chain beside the attention launch, round 5): the deep
    // ring's 128 KiB of LDS needs an EMPTY CU, the two-deep ring's 64 KiB fits next to one resident attention workgroup (74 KiB)
    // (round 6: the deep ring only while ONE round of it holds the launch.  Its 128 KiB of LDS mean one workgroup per CU, 256 at a
    // time: 324 workgroups -- the packed text tower's c_proj -- ran two rounds, the second a quarter full, where the two-deep form's
    // 512 slots take them in one and the second resident workgroup hides the DMA latency the deep ring was there for)
    p.ring = tiles <= 256 && !small_lds ? 4 : 2;
    return p;
}

// what gemm_plan() will read of its two inputs that cost a lock to obtain (the caller asks for those only)
struct GemmPlanNeeds {
    bool cus, splitk;
};
inline GemmPlanNeeds gemm_plan_needs(int epi, int M, int N, int K, long long lda, long long ldc, const GemmSwitches& sw) {
    const bool big = gemm_big_tiles(epi, M, N, K, lda, ldc, sw);
    const int small_rows = big ? M % 256 : M;
    return GemmPlanNeeds{big && gemm_quad_mode(epi, K, sw) == 2, small_rows > 0 && gemm_may_split(epi, small_rows, N, K, sw)};
}

// cus: compute units of the device; splitk_bytes: the split-K scratch this call may use (0: none); small_lds: the calling
// composite wants the 64 KiB-LDS form of the 128^2 kernel
inline GemmPlan gemm_plan(int epi, int M, int N, int K, long long lda, long long ldc, int cus, size_t splitk_bytes, bool small_lds,
                          const GemmSwitches& sw) {
    GemmPlan plan;
    // Large problems: full 256-row tiles go to a 256^2 kernel, the remainder rows (< 256) to the 128^2 one.
    // (ViT-L/14 at B=128: M = 32896 = 128*256 + 128, so 512..2048 big tiles = whole rounds on 256 CUs.)
    if (!gemm_big_tiles(epi, M, N, K, lda, ldc, sw)) {
        plan.main = gemm_plan_small(epi, M, N, K, splitk_bytes, small_lds, sw);
        return plan;
    }
    GemmPlan::Part& p = plan.main;
    p.rows = M / 256 * 256;
    p.ring = 2;
    p.splits = 1;
    const int quad = gemm_quad_mode(epi, K, sw);
    const int tiles = (p.rows / 256) * (N / 256);
    const int T = (cus > 256 ? 256 : cus) & ~7;       // whole XCD groups: workgroup b and tile ids b, b + T, ... share an XCD label
    // (the fp16-residual epilogue holds 16 residual chunks per lane beside the read-back accumulators: in the tile loop it spills,
    // out-proj 94 vs 70 us -- that epilogue keeps one tile per workgroup.  Late in round 3, with the quarter-wise read-back
    // the tile loop no longer spills (209 VGPRs), and still does not pay: out-proj 66.7 vs 66.3 us, c_proj 216 vs 203.5 on
    // its three-deep ring -- two tiles per workgroup leave one prologue to hide, and the epilogue's residual loads queue
    // behind the 32 DMA pieces of the next tile in the in-order vmcnt)
    if (quad == 2 && tiles > T && T >= 8 && !epi_resid16(epi) && epi != KEDS_EPI_X3_RESID_F32) {
        p.form = KEDS_GEMM_FORM_QUAD;
        p.persistent = 1;
        p.workgroups = T;
        p.defer = epi_is_ln(epi) && sw.quad_defer;
        if (p.defer && !epi_qgelu(epi) && K / 64 >= 8) p.flags = KEDS_GEMM_FLAG_DEFER;
    } else if (quad && epi_resid16(epi) && sw.quad3 && K >= 1024 && K / 64 >= 4) {       // long K: A operand through a three-deep ring
        p.form = KEDS_GEMM_FORM_QUAD3;
        p.ring = 3;
    } else if (quad) {
        p.form = KEDS_GEMM_FORM_QUAD;
    } else {
        p.form = KEDS_GEMM_FORM_PAIR;
        if (epi_resid16(epi) && sw.resid_prologue) p.flags = KEDS_GEMM_FLAG_RESID_PROLOGUE;
    }
    if (p.rows != M) plan.tail = gemm_plan_small(epi, M - p.rows, N, K, splitk_bytes, small_lds, sw);
    return plan;
}

// ---- the MXFP8 GEMMs (gemm_fp8.hip: keds_gemm_mxfp8_ex launches from this, keds_gemm_mxfp8_plan_query answers from it) ---------------
// The 4-wave kernel walks K-tiles of 128 in pairs and needs at least four.  debug (keds_mxfp8_debug) 16: the 8-wave kernel whatever
// the shape (the bit-identity test's reference).  The fp32-residual epilogue (API only, the towers keep their stream in fp16) stays on
// the 8-wave kernel: beside its 256-bit residual chunks the 4-wave K-loop has no registers left.
inline bool mxfp8_quad(int epilogue, int K, int debug) {
    return debug == 0 && K % 256 == 0 && K >= 512 && epilogue != KEDS_FP8_EPI_RESID_STATS_MX;
}
struct Mxfp8Plan {
    int form, grid, tiles;      // the layout of keds_gemm_mxfp8_last_launch (+ [3] = grid < tiles: persistent)
};
// cus: compute units of the device (read for the 4-wave form only)
inline Mxfp8Plan mxfp8_plan(int epilogue, int M, int N, int K, int cus, int debug) {
    const int tiles = (M / 256) * (N / 256);
    if (!mxfp8_quad(epilogue, K, debug)) return Mxfp8Plan{KEDS_FP8_FORM_PAIR, tiles, tiles};
    const int T = (cus > 256 ? 256 : cus) & ~7;       // whole XCD groups: workgroup b and its tile ids b, b + grid, ... share an XCD label
    // (A/B, round 4: the residual epilogues with one tile per workgroup, so that the hardware deals the tiles and the side lane's
    // small launches slot in between them: the GEMM class takes 0.5 ms more per step, the gaps in front of the attention launches
    // shrink by as much -- 14.87-15.06 against 14.92-15.00 ms per step, four alternating runs on one box)
    return Mxfp8Plan{KEDS_FP8_FORM_QUAD, T >= 8 && tiles > T ? T : tiles, tiles};
}

}  // namespace
