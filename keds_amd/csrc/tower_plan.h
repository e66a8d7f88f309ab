// What a tower pass launches (keds_tower_forward, keds_vit_run*, keds_text_run*, keds_readout): the one place that says.  Host C++
// without a HIP header, a device call or a getenv, exactly as gemm_plan.h and attention_plan.h are.  tower_layout() names the buffers
// of one tower's scratch and tower_plan() emits the ordered steps of its blocks; pass_layout() and pass_plan() do the same for a WHOLE
// pass: the front end (ViT: im2col, patch GEMM, CLS rows, ln_pre; text: the embedding) in front of the blocks and the read-out
// (LayerNorm of the read-out rows, projection, L2 normalisation) behind them.  The executor of towers.hip runs the steps one by one,
// keds_pass_plan_query / keds_tower_plan_query (keds_hip.h) answer from the same functions without a GPU, and
// tests/test_host_tower_plan.py holds the steps to tests/tower_check.py's plan() / plan_pass(), pins the enqueue order and checks that
// no two steps that share rows (or, through an alias, bytes) of a buffer are left unordered.
//
// The per-flow table of a pass -- which kernel, on which rows, reading and writing what, on which lane -- is read off tower_plan():
//   unfolded  stand-alone LayerNorm launches and plain bias epilogues, fp32 residual stream in x (KEDS_DETERMINISTIC / no folded weights)
//   bf16/fp16 LayerNorm folded into the GEMMs (keds_hip.h, KEDS_EPI_LN_*): the residual stream lives in `h` as fp16 (the reference's own
//             storage type after convert_weights, model.py:531-548): one copy that the residual GEMMs update in place (fp32 sum, rounded
//             once) and the LN-folded GEMMs read as their fp16 operand; st1 / st2 hold the {sum, sum sq} of its rows as seen by ln_1 /
//             ln_2.  Each LN-consuming GEMM also clears the statistics buffer the next producer accumulates into, so no memset sits
//             between the launches.  fp16 (keds_tower_params.f16): qkv, the attention output and the MLP hidden layer are fp16 and
//             out_w / proj_w fp16 weights (KEDS_EPI_*_F16_H); otherwise those are bf16.
//   fp8       BASELINE config 5: the four GEMMs of every block on MXFP8 operands (gemm_fp8.hip).  The MXFP8 copy of the stream (xq, xs),
//             the attention output (aq) and the MLP hidden (hq) are e4m3 + one e8m0 scale per 32 columns, produced by the GEMM
//             epilogues themselves (the attention output by the attention kernel).  Rows beyond the last full 256-row tile (128 of
//             32,896 at B = 128) keep the bf16 path, on the side lane: every producer has a bf16 twin for them.  Fewer than 256 rows:
//             everything is "remainder rows" and the pass is the bf16 one.
//   f32       the fp32-accurate flow (f32path.hip): fp32 everywhere, stand-alone LayerNorm, no side lane
//   x3        keds_tower_params.f32 == 2, the "fp32x3" operating point (round 5).  The same fp32 flow -- fp32 residual stream, fp32
//             LayerNorm / attention / QuickGELU -- with the four block GEMMs on SPLIT fp16 operands (keds_gemm_x3: x = hi + lo to 22
//             bits, products hi.hi + hi.lo + lo.hi on the fp16 MFMA, fp32 accumulate): fp32-grade results at about a third of the bf16
//             GEMMs' rate instead of the f32-input MFMA's sixteenth.  The weights arrive as fp16 planes [2][N][K] (keds_split_f16_pair
//             at packing time); LayerNorm writes its output as planes, the attention writes the out-projection's A operand planes
//             itself (no fp32 copy of its output, no split pass), c_fc's epilogue writes the MLP hidden layer as planes.  A value
//             beyond the fp16 range raises the caller's numerics guard (the host falls back to f32 = 1).
//
// Two lanes for one tower pass.  At B = 128 a ViT-L/14 tower has 32,896 rows = 128 full 256-row tiles + 128 remainder rows; every GEMM
// of the remainder is a handful of workgroups whose time is pure latency (13-14 us each, 61 us per block, 5.6 % of the step when it
// runs between the full-tile launches; 150 us per block in the x3 flow).  Rows only meet in the attention, so per block the remainder
// chain (out-proj, fc, proj, next qkv; x3: out-proj, ln_2, MLP, next ln_1, next in_proj) runs on the side lane while the caller's
// stream runs the same chain on the full tiles: fork behind the attention, join in front of the next one.
// Measured in round 2 (bench step, 128 images): 21.85 ms with the side lane, 22.85 ms with the remainder launches between the
// full-tile ones, 21.46 ms with the remainder rows not computed at all (timing only) -- the lane recovers 0.6 of the 1.0 ms these
// 0.39 % of the rows cost.  A side workgroup cannot share a CU with a 256 x 256 tile (registers), so each one displaces a tile of the
// kernel running beside it; forking the chain behind the out-proj launch instead of in front of it (so that it runs under c_fc's
// eight rounds of tiles rather than out-proj's two) changes nothing measurable.
// The fork behind a 16-bit attention is the launch's own stop event where the kernel form takes one (no marker packet between it and
// the next GEMM on the main stream); kernel forms that do not take it, and the x3 attention, get a recorded event.
// (The ragged last row tile as a full tile on filler rows -- round 3, 4 ms per step slower: docs/findings_r03.md -- and the tail
// samples' attention on the side lane -- round 4, neutral: profiles/r04_tail_attention_ab.txt -- last existed at 14f64ac.)
//
// After the last block only one row per sample is read: token 0 (ln_post(x[:,0,:]), model.py:412; tail CLS) or the EOT column
// (+ n_tok - 1 with spliced pseudo tokens; model.py:587-589, 847-849; tail READOUT: a different row per sample, known on the device
// only).  CLS: the attention computes one query per sample and out-proj, ln_2 and the MLP run on those B rows in place (row step S in
// x / att; the folded flows bring the CLS rows of the fp16 stream back to fp32 first).  READOUT: the block's in_proj and attention
// run on all rows (every key is needed; the attention is 1.6 % of a block), then the B read-out rows of the attention output and of
// the residual stream are gathered into the compact buffers att_c / x_c (in the qkv buffer, which nobody reads any more) and
// out-proj, ln_2 and the MLP run on those; on return the first B rows of x hold the block's output for sample b in row b (the caller
// reads out with S = 1, row 0).  With packed rows the read-out rows are GLOBAL row indices (off[b] + the sample's column).  The x3
// flow takes the compact form for the CLS rows too and copies them back with row step S.  Tails are fp32 rows on the plain kernels.
#pragma once
#include "../../include/keds_hip.h"
#include <initializer_list>
#include <stddef.h>
#include <stdint.h>

bool keds_gemm_splits_rows(int M, int N, int K);      // gemm.hip (the rule: gemm_plan.h, gemm_big_tiles_fill)

namespace {

inline size_t tower_align(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline size_t tower_pad_rows(size_t m) { return tower_align(m, 256); }      // (256: whole row tiles; packed rows run up to the next one)

// ---- the buffers ---------------------------------------------------------------------------------------------------------------
// (the MXFP8 scale buffer of xq / aq / hq is the next id)
enum {
    TB_NONE = KEDS_TOWER_BUF_NONE, TB_X = KEDS_TOWER_BUF_X, TB_H = KEDS_TOWER_BUF_H, TB_QKV = KEDS_TOWER_BUF_QKV,
    TB_ATT = KEDS_TOWER_BUF_ATT, TB_HID = KEDS_TOWER_BUF_HID, TB_ST1 = KEDS_TOWER_BUF_ST1, TB_ST2 = KEDS_TOWER_BUF_ST2,
    TB_XQ = KEDS_TOWER_BUF_XQ, TB_XS = KEDS_TOWER_BUF_XS, TB_AQ = KEDS_TOWER_BUF_AQ, TB_AS = KEDS_TOWER_BUF_AS,
    TB_HQ = KEDS_TOWER_BUF_HQ, TB_HS = KEDS_TOWER_BUF_HS, TB_SPLITK = KEDS_TOWER_BUF_SPLITK, TB_LN = KEDS_TOWER_BUF_LN,
    TB_ATT_C = KEDS_TOWER_BUF_ATT_C, TB_X_C = KEDS_TOWER_BUF_X_C, TB_N = KEDS_TOWER_BUF_COUNT,
    // a whole pass: the im2col matrix, the read-out rows, and the caller's embeddings / token output / images or token ids
    TB_COL = KEDS_PASS_BUF_COL, TB_RO = KEDS_PASS_BUF_RO, TB_OUT = KEDS_PASS_BUF_OUT, TB_TOK = KEDS_PASS_BUF_TOK, TB_SRC = KEDS_PASS_BUF_SRC,
    PB_N = KEDS_PASS_BUF_COUNT
};
constexpr size_t TOWER_SPLITK_BYTES = (size_t)8 << 20;      // (keds_common.h, KEDS_SPLITK_BYTES)

// The scratch of one tower for B x seq rows (Mp = rows padded to 256; packed rows use the same carving), every buffer on a 256-byte
// boundary, in this order:
//   16-bit flows  h [Mp,w] | qkv [Mp,3w] | att [Mp,w] | hid [Mp,4w] (16-bit) | st1, st2 [Mp,2] 64-bit fixed point |
//                 xq xs aq as hq hs: the MXFP8 operands of the Mm = B seq / 256 * 256 full-tile rows (1 scale byte / 32) |
//                 splitk: fp32 partial tiles of the split-K launches of THIS call (remainder rows, CLS tail)
//   f32 / x3      ln [Mp,w] | qkv [Mp,3w] | att [Mp,w] | hid [Mp,4w], 4 bytes per element: fp32, or two fp16 planes (x3: ln, hid)
//                 (1.2 GB at B = 128, ViT-L/14)
// No buffer aliases another -- the remainder-row chain runs beside the full-tile chain and the two touch disjoint ROWS of every buffer,
// which only keeps them apart if the buffers themselves are distinct -- except the compact tail buffers att_c [B,w] | x_c [B,w] fp32,
// declared aliases of the head of qkv (dead behind the last attention): 6 B w <= 6 w Mp bytes (16-bit), 8 B w <= 12 w Mp (fp32).
// x is the caller's fp32 stream [Mp,w], outside the scratch.
struct TowerBuf {
    size_t off = 0, bytes = 0;      // bytes 0: the flow has no such buffer
    int cols = 0, esize = 0;        // a row is cols elements of esize bytes (planes: of ONE plane)
    int alias_of = TB_NONE;
    bool caller = false;            // the caller's own buffer, outside the workspace (off means nothing)
};
struct TowerLayout {
    TowerBuf b[PB_N];               // (ids >= TB_N: a whole pass, pass_layout())
    size_t total = 0;
};

inline bool tower_flow_f32(int flow) { return flow == KEDS_TOWER_FLOW_F32 || flow == KEDS_TOWER_FLOW_X3; }

inline TowerLayout tower_layout(int flow, int width, int seq, int B) {
    TowerLayout L;
    const size_t w = (size_t)width, Mp = tower_pad_rows((size_t)B * seq), Mm = (size_t)B * seq / 256 * 256;
    auto take = [&](int id, size_t rows, size_t cols, int esize, size_t row_bytes) {
        L.b[id].off = L.total;
        L.b[id].bytes = rows * row_bytes;
        L.b[id].cols = (int)cols;
        L.b[id].esize = esize;
        L.total += tower_align(rows * row_bytes, 256);
    };
    L.b[TB_X].bytes = Mp * w * 4;
    L.b[TB_X].cols = width;
    L.b[TB_X].esize = 4;
    L.b[TB_X].caller = true;
    const bool f32 = tower_flow_f32(flow), pair = flow == KEDS_TOWER_FLOW_X3;
    if (f32) {
        take(TB_LN, Mp, w, pair ? 2 : 4, w * 4);
        take(TB_QKV, Mp, 3 * w, 4, 3 * w * 4);
        take(TB_ATT, Mp, w, 4, w * 4);
        take(TB_HID, Mp, 4 * w, pair ? 2 : 4, 4 * w * 4);
    } else {
        take(TB_H, Mp, w, 2, w * 2);
        take(TB_QKV, Mp, 3 * w, 2, 3 * w * 2);
        take(TB_ATT, Mp, w, 2, w * 2);
        take(TB_HID, Mp, 4 * w, 2, 4 * w * 2);
        take(TB_ST1, Mp, 2, 8, 16);
        take(TB_ST2, Mp, 2, 8, 16);
        take(TB_XQ, Mm, w, 1, w);
        take(TB_XS, Mm, w / 32, 1, w / 32);
        take(TB_AQ, Mm, w, 1, w);
        take(TB_AS, Mm, w / 32, 1, w / 32);
        take(TB_HQ, Mm, 4 * w, 1, 4 * w);
        take(TB_HS, Mm, 4 * w / 32, 1, 4 * w / 32);
        take(TB_SPLITK, 1, TOWER_SPLITK_BYTES, 1, TOWER_SPLITK_BYTES);
    }
    const int ea = f32 ? 4 : 2;                                      // [B, w] of the attention output's type (2 w bytes per row: a multiple of 256)
    L.b[TB_ATT_C] = TowerBuf{L.b[TB_QKV].off, (size_t)B * w * ea, width, ea, TB_QKV, false};
    L.b[TB_X_C] = TowerBuf{L.b[TB_QKV].off + (size_t)B * w * ea, (size_t)B * w * 4, width, 4, TB_QKV, false};
    return L;
}

// ---- flows ---------------------------------------------------------------------------------------------------------------------
// keds_tower_params -> KEDS_TOWER_FLOW_*, or -1 with *why set (the caller's error text).  An fp8 tower of fewer than 256 rows is
// still KEDS_TOWER_FLOW_FP8 here: tower_plan() runs it as the bf16 flow.
inline int tower_flow(const keds_tower_params* p, const char** why) {
    if (p->f32) return p->f32 == 2 ? KEDS_TOWER_FLOW_X3 : KEDS_TOWER_FLOW_F32;
    bool folded = true, have8 = true;
    for (int l = 0; l < p->layers; ++l) {
        const keds_block_params& k = p->blocks[l];
        folded = folded && k.qkv_wf && k.fc_wf && k.qkv_bc && k.fc_bc;
        have8 = have8 && k.qkv_q8 && k.out_q8 && k.fc_q8 && k.proj_q8 && k.qkv_s8 && k.out_s8 && k.fc_s8 && k.proj_s8 && k.qkv_bc8 &&
                k.fc_bc8;
    }
    if (p->fp8 && !(folded && have8 && p->width % 256 == 0)) {
        *why = "keds_tower_forward: fp8 needs the folded and MXFP8 weights and width % 256 == 0";
        return -1;
    }
    if (p->f16 && (p->fp8 || !folded)) {
        *why = "keds_tower_forward: f16 needs the folded weights and excludes fp8 / f32";
        return -1;
    }
    return p->fp8 ? KEDS_TOWER_FLOW_FP8 : !folded ? KEDS_TOWER_FLOW_UNFOLDED : p->f16 ? KEDS_TOWER_FLOW_FP16 : KEDS_TOWER_FLOW_BF16;
}

// When every GEMM of the block would split into full 256-row tiles + a remainder launch anyway, the remainder rows become their own
// chain on the side lane; otherwise one span covers all rows.  The three rules:
inline bool tower_splits_rows(int flow, int M, int w) {
    const int Mm = M / 256 * 256;
    switch (flow) {
        case KEDS_TOWER_FLOW_BF16:
        case KEDS_TOWER_FLOW_FP16:      // all four GEMMs split
            return keds_gemm_splits_rows(M, 3 * w, w) && keds_gemm_splits_rows(M, w, w) && keds_gemm_splits_rows(M, 4 * w, w) &&
                   keds_gemm_splits_rows(M, w, 4 * w);
        case KEDS_TOWER_FLOW_X3:        // the in_proj splits
            return Mm > 0 && Mm < M && keds_gemm_splits_rows(M, 3 * w, w);
        case KEDS_TOWER_FLOW_FP8:       // full tiles on the MXFP8 kernels, the rest on the bf16 ones
            return M >= 256 && M % 256 != 0;
    }
    return false;
}

// ---- the steps -----------------------------------------------------------------------------------------------------------------
enum { TW_NONE = 0, TW_QKV, TW_OUT, TW_FC, TW_PROJ, TW_QKV_FOLDED, TW_FC_FOLDED, TW_LN1, TW_LN2,
       TW_CONV, TW_LN_PRE, TW_LN_OUT, TW_PROJ_T };      // a whole pass: patch embedding, ln_pre, ln_post / ln_final, the projection
enum { TAIL_ALL = KEDS_TOWER_TAIL_ALL, TAIL_CLS = KEDS_TOWER_TAIL_CLS, TAIL_READOUT = KEDS_TOWER_TAIL_READOUT };

// One launch (or stream operation) of a pass; the int32 record of keds_pass_plan_query / keds_tower_plan_query in this order (keds_hip.h
// documents it)
struct TowerStep {
    int op = 0, layer = -1, weight = TW_NONE, epi = 0;
    int in = TB_NONE, in_r0 = 0, in_step = 1;
    int out = TB_NONE, out_r0 = 0, out_step = 1;
    int n = 0;                      // rows
    int out2 = TB_NONE;             // the MXFP8 copy a launch writes beside `out` (its scales: the next buffer id)
    int plane_rows = 0;             // x3: rows of one fp16 plane of `in` / `out` (plane stride = plane_rows * the buffer's columns)
    int st_read = TB_NONE, st_add = TB_NONE, st_clear = TB_NONE, st_r0 = 0;
    int q_limit = 0, q8_rows = 0, packed = 0;
    int bound = 0, global = 0;      // gather: rows outside [0, bound) come out as NaN; global (packed) or per-sample row indices
                                    // residual GEMM of a packed folded pass: rows >= bound of out and st_add are zeroed behind it (0: none)
    int lane = 0;                   // 0: the caller's stream, 1: the side lane
    int rows = 0;                   // LayerNorm of the read-out: sample b's row is in_r0 + b * in_step + its read-out column (device)
};
static_assert(sizeof(TowerStep) == KEDS_TOWER_STEP_INTS * sizeof(int), "the record of keds_tower_plan_query");

struct TowerPlanArgs {
    int flow, width, heads, seq, causal, layers, B;
    int tail;                       // KEDS_TOWER_TAIL_*
    int packed_rows, packed_valid;  // packed rows: the rows the pass runs and off[B] (rows [valid, rows) are zero rows); 0, 0: none
    bool taps;
    bool split;                     // tower_splits_rows(): the remainder rows are a span of their own (fp8: decided by the rows alone)
    bool lane;                      // a side lane exists
};

inline const char* tower_plan_check(const TowerPlanArgs& a) {
    if (a.flow < KEDS_TOWER_FLOW_UNFOLDED || a.flow > KEDS_TOWER_FLOW_X3) return "keds_tower_forward: unknown flow";
    if (a.width <= 0 || a.width % 128 != 0 || a.width != a.heads * 64 || a.seq < 1 || a.layers < 1 || a.B < 1 || a.tail < TAIL_ALL ||
        a.tail > TAIL_READOUT)
        return "keds_tower_forward: bad tower geometry";
    if (a.packed_rows &&
        (a.flow == KEDS_TOWER_FLOW_FP8 || !a.causal || a.tail != TAIL_READOUT || a.packed_valid < 1 || a.packed_valid > a.packed_rows ||
         (size_t)a.packed_rows > tower_pad_rows((size_t)a.B * a.seq)))
        return "keds_tower_forward: packed rows need a causal bf16 / fp16 / fp32 / fp32x3 tower with a read-out row per sample";
    return nullptr;
}

// emit(const TowerStep&) -> bool (false: stop).  Returns false when emit stopped the plan.  The order of the steps is the enqueue
// order of the pass.  front(): pass_plan()'s steps that fill x, behind the clearing of the packed zero rows of x.
template <typename Emit, typename Front>
inline bool tower_plan(const TowerPlanArgs& a, Emit&& emit, Front&& front) {
    const int S = a.seq, B = a.B;
    const int M = a.packed_rows ? a.packed_rows : B * S, Mm = M / 256 * 256;
    const int Mp = (int)tower_pad_rows((size_t)B * S), Bp = (int)tower_pad_rows((size_t)B);
    int flow = a.flow;
    if (flow == KEDS_TOWER_FLOW_FP8 && Mm == 0) flow = KEDS_TOWER_FLOW_BF16;      // fewer than 256 rows: the bf16 kernels
    const bool fp8 = flow == KEDS_TOWER_FLOW_FP8, x3 = flow == KEDS_TOWER_FLOW_X3, f32 = tower_flow_f32(flow);
    const bool f16 = flow == KEDS_TOWER_FLOW_FP16;
    const bool folded = fp8 || f16 || flow == KEDS_TOWER_FLOW_BF16;
    const int stream = folded ? TB_H : TB_X;                        // where the residual stream lives between the blocks
    const int lnbuf = f32 ? TB_LN : TB_H;
    const int gemm_op = x3 ? KEDS_TOWER_OP_GEMM_X3 : f32 ? KEDS_TOWER_OP_GEMM_F32 : KEDS_TOWER_OP_GEMM16;
    const bool packed = a.packed_rows != 0;

    struct Span {
        int r0, n;
        bool mx;
        int lane;
    };
    const bool two = fp8 ? M > Mm : (a.split && a.lane && (f16 || x3 || flow == KEDS_TOWER_FLOW_BF16) && Mm > 0 && Mm < M);
    const bool lane = two && a.lane;
    const Span spans[2] = {{0, two ? Mm : M, fp8, 0}, {Mm, M - Mm, false, lane ? 1 : 0}};
    const int nspan = two ? 2 : 1;

    bool go = true;
    auto put = [&](const TowerStep& s) { go = go && emit(s); };
    auto stream_op = [&](int op) {
        TowerStep s;
        s.op = op;
        put(s);
    };
    // the plain (not LayerNorm-folded) GEMM of a block on the flow's kernel family
    auto gemm = [&](int l, int wt, int in, int in_r0, int in_step, int out, int out_r0, int out_step, int n, int lane_, int plane_rows) {
        TowerStep s;
        s.op = gemm_op;
        s.layer = l;
        s.weight = wt;
        const bool resid = wt == TW_OUT || wt == TW_PROJ;
        if (x3) s.epi = wt == TW_QKV ? KEDS_EPI_X3_BIAS_F32 : wt == TW_FC ? KEDS_EPI_X3_QGELU_PAIR : KEDS_EPI_X3_RESID_F32;
        else if (f32) s.epi = wt == TW_QKV ? KEDS_F32_EPI_BIAS : wt == TW_FC ? KEDS_F32_EPI_QGELU : KEDS_F32_EPI_RESID;
        else if (resid) s.epi = f16 ? KEDS_EPI_BIAS_RESID_F32_H : KEDS_EPI_BIAS_RESID_F32;
        else if (wt == TW_FC) s.epi = f16 ? KEDS_EPI_BIAS_QGELU_F16_H : KEDS_EPI_BIAS_QGELU_BF16;
        else s.epi = KEDS_EPI_BIAS_BF16;
        s.in = in, s.in_r0 = in_r0, s.in_step = in_step;
        s.out = out, s.out_r0 = out_r0, s.out_step = out_step;
        s.n = n, s.lane = lane_, s.plane_rows = x3 ? plane_rows : 0;
        put(s);
    };
    auto layernorm = [&](int l, int wt, int in, int in_r0, int in_step, int r0, int n, int lane_, int plane_rows) {
        TowerStep s;
        s.op = x3 ? KEDS_TOWER_OP_LN_PAIR : KEDS_TOWER_OP_LN;
        s.layer = l;
        s.weight = wt;
        s.epi = f32 ? 1 : f16 ? 2 : 0;                              // the output type of keds_layernorm_ex
        s.in = in, s.in_r0 = in_r0, s.in_step = in_step;
        s.out = lnbuf, s.out_r0 = r0, s.n = n, s.lane = lane_, s.plane_rows = x3 ? plane_rows : 0;
        put(s);
    };
    // a GEMM of the folded flows on a span: the bf16 / fp16 kernels, or (sp.mx) the MXFP8 ones
    auto folded_gemm = [&](int l, int wt, const Span& sp, bool last) {
        TowerStep s;
        s.op = sp.mx ? KEDS_TOWER_OP_GEMM_MX : KEDS_TOWER_OP_GEMM16;
        s.layer = l;
        s.in_r0 = s.out_r0 = s.st_r0 = sp.r0;
        s.n = sp.n, s.lane = sp.lane;
        const int act = sp.mx ? TB_XQ : TB_H;
        switch (wt) {
            case TW_QKV:
                s.weight = sp.mx ? TW_QKV : TW_QKV_FOLDED;
                s.epi = sp.mx ? KEDS_FP8_EPI_LN_BIAS_BF16 : f16 ? KEDS_EPI_LN_BIAS_F16_H : KEDS_EPI_LN_BIAS_BF16_H;
                s.in = act, s.out = TB_QKV, s.st_read = TB_ST1, s.st_clear = TB_ST2;
                break;
            case TW_OUT:
                s.weight = TW_OUT;
                s.epi = sp.mx ? KEDS_FP8_EPI_RESID_STATS_MX_H : f16 ? KEDS_EPI_RESID_STATS_F16_H : KEDS_EPI_RESID_STATS_F16;
                s.in = sp.mx ? TB_AQ : TB_ATT, s.out = TB_H, s.out2 = sp.mx ? TB_XQ : TB_NONE, s.st_add = TB_ST2;
                break;
            case TW_FC:
                s.weight = sp.mx ? TW_FC : TW_FC_FOLDED;
                s.epi = sp.mx ? KEDS_FP8_EPI_LN_QGELU_MX : f16 ? KEDS_EPI_LN_QGELU_F16_H : KEDS_EPI_LN_QGELU_BF16_H;
                s.in = act, s.out = sp.mx ? TB_HQ : TB_HID, s.st_read = TB_ST2, s.st_clear = TB_ST1;
                break;
            default:      // (the last block's output feeds no further ln_1: no statistics; the MXFP8 epilogue always adds them)
                s.weight = TW_PROJ;
                s.epi = sp.mx ? KEDS_FP8_EPI_RESID_STATS_MX_H : f16 ? KEDS_EPI_RESID_STATS_F16_H : KEDS_EPI_RESID_STATS_F16;
                s.in = sp.mx ? TB_HQ : TB_HID, s.out = TB_H, s.out2 = sp.mx ? TB_XQ : TB_NONE;
                s.st_add = last && !sp.mx ? TB_NONE : TB_ST1;
        }
        // packed rows: a residual GEMM leaves its bias (and what the zero rows' hidden values project to) in the zero rows of the
        // stream, and their statistics with it -- a row of mean 0.2 and deviation 0.001 that no caption owns would trip the numerics
        // guard of the LayerNorm-folded GEMM that reads them next.  `bound` on such a step: the rows of `out` and of `st_add` from
        // `bound` on go back to zero behind the launch; the next GEMM sees mean 0, variance 0 there and writes its bias.
        if (packed && M > a.packed_valid && s.st_add != TB_NONE && !sp.mx && sp.r0 + sp.n > a.packed_valid)
            s.bound = a.packed_valid > sp.r0 ? a.packed_valid : sp.r0;
        put(s);
    };
    auto pre = [&](int l, const Span& sp) {      // ln_1 + in_proj
        if (folded) return folded_gemm(l, TW_QKV, sp, false);
        layernorm(l, TW_LN1, TB_X, sp.r0, 1, sp.r0, sp.n, sp.lane, Mp);
        gemm(l, TW_QKV, lnbuf, sp.r0, 1, TB_QKV, sp.r0, 1, sp.n, sp.lane, Mp);
    };
    auto tap = [&](int l, const Span& sp) {      // each span on the lane that produced it, behind its c_proj
        if (!a.taps) return;
        TowerStep s;
        s.op = KEDS_TOWER_OP_TAP;
        s.layer = l;
        s.epi = folded ? 2 : 1;                  // the source type of keds_tap_rows: fp16 / fp32 rows
        s.in = stream, s.in_r0 = sp.r0, s.n = sp.n, s.lane = sp.lane;
        put(s);
    };
    // fork: the attention of the folded flows with the side lane forked behind it
    auto attention = [&](int q_limit, int out, bool fork, bool pk, bool q8) {
        TowerStep s;
        s.op = fork ? KEDS_TOWER_OP_ATTN_FORK : KEDS_TOWER_OP_ATTN;
        s.in = TB_QKV, s.out = out, s.n = M, s.q_limit = q_limit, s.packed = pk;
        if (q8) s.q8_rows = Mm, s.out2 = TB_AQ;      // rows < q8_rows as MXFP8 into aq / as, the rest bf16 into att
        if (out == TB_LN) s.plane_rows = Mp;
        put(s);
    };
    auto rows_op = [&](int op, int epi, int in, int in_step, int out, int out_step, int n) {      // B rows of a tail, or all rows
        TowerStep s;
        s.op = op, s.epi = epi;
        s.in = in, s.in_step = in_step, s.out = out, s.out_step = out_step, s.n = n;
        put(s);
    };

    // packed rows: the zero rows up to the next 256-row tile belong to no sample.  Their x rows are cleared (the embedding goes
    // behind that), and they are nobody's queries -- their attention output is cleared once so that they stay finite through the blocks
    // (x3: the out-projection reads ln_1's output there, which is finite)
    auto zero_rows = [&](int buf) {
        TowerStep s;
        s.op = KEDS_TOWER_OP_ZERO;
        s.out = buf, s.out_r0 = a.packed_valid, s.n = M - a.packed_valid;
        put(s);
    };
    if (packed && M > a.packed_valid) zero_rows(TB_X);
    front();
    if (packed && M > a.packed_valid && !x3) zero_rows(TB_ATT);
    if (folded) {      // h = the fp16 copy of the stream, st1 = its row statistics; fp8: the MXFP8 copy of the full-tile rows
        TowerStep s;
        s.op = KEDS_TOWER_OP_STATS_CAST, s.epi = 1;
        s.in = TB_X, s.out = TB_H, s.n = M, s.st_add = TB_ST1;
        put(s);
        if (fp8) {
            TowerStep q;
            q.op = KEDS_TOWER_OP_QUANT;
            q.in = TB_X, q.out = TB_XQ, q.n = Mm;
            put(q);
        }
    }
    if (lane) stream_op(KEDS_TOWER_OP_FORK);
    const bool one = a.tail != TAIL_ALL;
    for (int l = 0; l < a.layers && go; ++l) {
        const bool last = l == a.layers - 1;
        if (!x3 || l == 0)      // (x3: the first `pre` sits in front of the loop, the others ride behind their span's `post`)
            for (int i = 0; i < nspan; ++i) pre(l, spans[i]);
        if (lane) stream_op(KEDS_TOWER_OP_JOIN);      // every row's q, k, v before the attention (and before a tail)
        if (last && one) break;
        attention(S, x3 ? TB_LN : TB_ATT, lane && folded, packed, fp8);
        if (lane && !folded) stream_op(KEDS_TOWER_OP_FORK);
        if (folded) {      // body and remainder interleave per GEMM
            for (const int wt : {TW_OUT, TW_FC, TW_PROJ})
                for (int i = 0; i < nspan; ++i) {
                    folded_gemm(l, wt, spans[i], last);
                    if (wt == TW_PROJ) tap(l, spans[i]);
                }
            continue;
        }
        for (int i = 0; i < nspan; ++i) {      // a span's whole chain, then the next span
            const Span& sp = spans[i];
            gemm(l, TW_OUT, x3 ? TB_LN : TB_ATT, sp.r0, 1, TB_X, sp.r0, 1, sp.n, sp.lane, Mp);
            layernorm(l, TW_LN2, TB_X, sp.r0, 1, sp.r0, sp.n, sp.lane, Mp);
            gemm(l, TW_FC, lnbuf, sp.r0, 1, TB_HID, sp.r0, 1, sp.n, sp.lane, Mp);
            gemm(l, TW_PROJ, TB_HID, sp.r0, 1, TB_X, sp.r0, 1, sp.n, sp.lane, Mp);
            tap(l, sp);
            if (x3 && !last) pre(l + 1, sp);
        }
    }
    if (!one) {
        if (lane) stream_op(KEDS_TOWER_OP_JOIN);
        if (folded) rows_op(KEDS_TOWER_OP_CAST, 0, TB_H, 1, TB_X, 1, M);      // the caller reads x in fp32
        return go;
    }
    // ---- the tail: one row per sample behind the last block's in_proj (see the head of this file) -------------------------------
    const int l = a.layers - 1;
    const bool compact = a.tail == TAIL_READOUT || x3;
    if (a.tail == TAIL_CLS) {
        if (folded) rows_op(KEDS_TOWER_OP_CAST, 0, TB_H, S, TB_X, S, B);
        attention(1, TB_ATT, false, false, false);
        if (compact) {
            rows_op(KEDS_TOWER_OP_COPY, 1, TB_ATT, S, TB_ATT_C, 1, B);
            rows_op(KEDS_TOWER_OP_COPY, 1, TB_X, S, TB_X_C, 1, B);
        }
    } else {
        attention(S, TB_ATT, false, packed, false);
        for (const int src : {(int)TB_ATT, stream}) {
            TowerStep s;
            s.op = KEDS_TOWER_OP_GATHER;
            s.epi = src == TB_ATT ? (f32 ? 2 : 0) : folded ? 1 : 2;      // keds_gather_rows: 16-bit rows, fp16 -> fp32, fp32 rows
            s.in = src, s.out = src == TB_ATT ? TB_ATT_C : TB_X_C, s.n = B;
            s.bound = packed ? a.packed_valid : S, s.global = packed;
            put(s);
        }
    }
    const int xa = compact ? TB_X_C : TB_X, xs = compact ? 1 : S;
    int aa = compact ? TB_ATT_C : TB_ATT;
    if (x3) {      // the out-projection's A operand as planes of Bp rows
        TowerStep s;
        s.op = KEDS_TOWER_OP_SPLIT;
        s.in = TB_ATT_C, s.out = TB_LN, s.n = B, s.plane_rows = Bp;
        put(s);
        aa = TB_LN;
    }
    gemm(l, TW_OUT, aa, 0, aa == TB_ATT ? S : 1, xa, 0, xs, B, 0, Bp);
    layernorm(l, TW_LN2, xa, 0, xs, 0, B, 0, Bp);
    gemm(l, TW_FC, lnbuf, 0, 1, TB_HID, 0, 1, B, 0, Bp);
    gemm(l, TW_PROJ, TB_HID, 0, 1, xa, 0, xs, B, 0, Bp);
    // the caller reads row b of a compact x (read-out rows) or row b * S (x3: CLS rows back in place)
    if (compact) rows_op(KEDS_TOWER_OP_COPY, x3 ? 1 : 0, TB_X_C, 1, TB_X, a.tail == TAIL_READOUT ? 1 : S, B);
    return go;
}
template <typename Emit>
inline bool tower_plan(const TowerPlanArgs& a, Emit&& emit) {
    return tower_plan(a, emit, [] {});
}

// ---- a whole pass --------------------------------------------------------------------------------------------------------------
// When a text batch whose captions end at different columns runs on packed rows (keds_text_run_packed: rows_total = the sum of the
// captions' lengths) instead of B x seq_used rectangular ones: a causal tower that is not the MXFP8 one, on the default trim mode,
// and at least an eighth of the rows saved.
inline bool text_runs_packed(bool causal, bool fp8, int trim, long long rows_total, int B, int seq_used) {
    return causal && !fp8 && trim == 1 && rows_total * 8 <= (long long)B * seq_used * 7;
}

// ln_post / ln_final of one row per sample (row b * in_step, + the sample's read-out column with `rows`) into ro, the projection into
// out, L2 normalisation in place.  type: keds_layernorm_ex's output type of the flow (0 bf16, 1 fp32, 2 fp16).  The fp32 flows
// normalise with the fp32 rows kernel, the 16-bit flows with keds_l2_normalize's.
template <typename Put>
inline void readout_plan(int type, int B, int in_step, bool rows, bool normalize, Put&& put) {
    TowerStep ln;
    ln.op = KEDS_TOWER_OP_LN, ln.weight = TW_LN_OUT, ln.epi = type;
    ln.in = TB_X, ln.in_step = in_step, ln.rows = rows, ln.out = TB_RO, ln.n = B;
    put(ln);
    TowerStep g;
    g.op = type == 1 ? KEDS_TOWER_OP_GEMM_F32 : KEDS_TOWER_OP_GEMM16, g.weight = TW_PROJ_T;
    g.epi = type == 1 ? KEDS_F32_EPI_BIAS : type == 2 ? KEDS_EPI_BIAS_F32_H : KEDS_EPI_BIAS_F32;
    g.in = TB_RO, g.out = TB_OUT, g.n = B;
    put(g);
    if (!normalize) return;
    TowerStep l2;
    l2.op = KEDS_TOWER_OP_L2NORM, l2.epi = type == 1;
    l2.in = l2.out = TB_OUT, l2.n = B;
    put(l2);
}

struct PassArgs {
    int kind;                       // KEDS_PASS_*
    TowerPlanArgs t;                // the blocks: seq = the columns that run (text), tail and packed rows as the kind and trim mode say
    int resolution, patch, kpad, embed_dim;
    int context;                    // text: L, the columns of a token row (t.seq <= L run)
    int n_tok, insert_col;          // text: the splice of pseudo tokens (n_tok 0: none)
    int trim;                       // text: keds_text_trim_enable's mode 0 - 3
    int normalize, out_type;        // out_type: the token output of text_tokens (keds_layernorm_ex)
    bool readout;                   // vit_tokens without `out`: no read-out
};

// keds_pass_shape (keds_hip.h) -> PassArgs: which columns run, what the tail is, how many packed rows.  t.split / t.lane as given
// (> 0); the caller resolves -1.
inline PassArgs pass_args(const keds_pass_shape& q) {
    PassArgs a{};
    a.kind = q.kind;
    a.resolution = q.resolution, a.patch = q.patch, a.kpad = q.kpad, a.embed_dim = q.embed_dim;
    a.context = q.context, a.n_tok = q.n_tok, a.insert_col = q.insert_col, a.trim = q.trim;
    a.normalize = q.normalize, a.out_type = q.out_type, a.readout = q.readout != 0;
    TowerPlanArgs& t = a.t;
    t = TowerPlanArgs{q.flow, q.width, q.heads, q.seq, q.causal != 0, q.layers, q.B, q.cls_only ? TAIL_CLS : TAIL_ALL, 0, 0, false,
                      q.split > 0, q.lane > 0};
    const int L = q.context;
    switch (q.kind) {
        case KEDS_PASS_VIT_TOKENS:      // the last block on every row; the CLS read-out comes from the full stream
            t.tail = TAIL_ALL, t.taps = true;
            break;
        case KEDS_PASS_TEXT: {
            // (no rounding of the cut to whole row tiles: measured at B = 128 -- tools/text_shapes.py, profiles/r05_text_shapes.txt --
            // the four GEMMs of a block take 161 us at 43 columns, 170 at 44, 172-174 at 46-48: at these sizes the 128 x 128 kernel's
            // rounds of 512 workgroups decide, and fewer rows are never slower)
            const bool cut = q.trim == 1 || q.trim == 2, trim = q.trim == 1 || q.trim == 3;
            t.seq = cut && q.seq_used > 0 && q.seq_used < L && q.causal ? q.seq_used : L;
            if (trim) t.tail = TAIL_READOUT;
            a.readout = true;
            break;
        }
        case KEDS_PASS_TEXT_PACKED:
            // the tower runs WHOLE 256-row tiles: the rows between rows_total and the next multiple of 256 are zero rows that belong to
            // no sample (no attention reads them, nothing gathers them; the pass clears them in front of the embedding).  A ragged
            // last tile would send every GEMM of every block through the remainder-row launches and the stricter fill rule of the
            // 256 x 256 kernels (gemm_plan.h, gemm_big_tiles_fill).
            t.seq = q.seq_used, t.tail = TAIL_READOUT;
            t.packed_valid = q.rows_total, t.packed_rows = (q.rows_total + 255) / 256 * 256;
            if ((size_t)t.packed_rows > tower_pad_rows((size_t)q.B * t.seq)) t.packed_rows = q.rows_total;
            a.readout = true;
            break;
        case KEDS_PASS_TEXT_TOKENS:     // every column is an output: no cut, no read-out-row tail
            t.seq = L, t.tail = TAIL_ALL;
            break;
    }
    return a;
}
inline bool pass_is_vit(int kind) { return kind == KEDS_PASS_VIT || kind == KEDS_PASS_VIT_TOKENS; }
inline bool pass_is_text(int kind) { return kind >= KEDS_PASS_TEXT && kind <= KEDS_PASS_TEXT_TOKENS; }
// the rows of a pass's blocks; whether the library's own rule gives them a remainder span (keds_tower_side_rows)
inline int pass_rows(const TowerPlanArgs& t) { return t.packed_rows ? t.packed_rows : t.B * t.seq; }
inline bool pass_splits_rows(const TowerPlanArgs& t) {
    const int M = pass_rows(t);
    return tower_splits_rows(t.flow == KEDS_TOWER_FLOW_FP8 && M < 256 ? KEDS_TOWER_FLOW_BF16 : t.flow, M, t.width);
}

inline const char* pass_plan_check(const PassArgs& a) {
    if (a.kind < KEDS_PASS_TOWER || a.kind > KEDS_PASS_TEXT_TOKENS) return "keds_pass_plan_query: unknown kind";
    if (pass_is_vit(a.kind)) {
        const int g = a.patch > 0 ? a.resolution / a.patch : 0;
        if (a.patch <= 0 || a.resolution % a.patch != 0 || g * g + 1 != a.t.seq) return "keds_pass_plan_query: seq must be (res/patch)^2 + 1";
        if (a.kpad % 64 != 0 || a.kpad < 3 * a.patch * a.patch) return "keds_pass_plan_query: bad kpad";
    }
    if (pass_is_text(a.kind)) {
        if (a.t.seq < 1 || a.t.seq > a.context || a.trim < 0 || a.trim > 3) return "keds_pass_plan_query: columns outside the context, or a trim mode outside 0 - 3";
        if (a.n_tok && (a.insert_col < 0 || a.insert_col + a.n_tok > a.context)) return "keds_pass_plan_query: splice outside the context";
        if (a.kind == KEDS_PASS_TEXT_PACKED &&
            (a.t.packed_valid < a.t.B || (long long)a.t.packed_valid > (long long)a.t.B * a.t.seq || a.trim != 1))
            return "keds_pass_plan_query: packed rows do not fit B sequences, or a trim mode other than 1";
    }
    if (a.readout && a.kind != KEDS_PASS_TOWER && a.embed_dim % 128 != 0) return "keds_pass_plan_query: embed_dim must be a multiple of 128";
    if (a.out_type < 0 || a.out_type > 2) return "keds_pass_plan_query: out_type outside 0 - 2";
    return tower_plan_check(a.t);
}

// The workspace of a pass, every buffer on a 256-byte boundary:
//   x [Mp, w] fp32 | the tower scratch (tower_layout) | ro: the LayerNorm of the read-out rows, [B up to 128, w] of the flow's type
// ViT: col, the im2col matrix [B (S - 1) up to 256, kpad] of the flow's type, is a declared alias: it starts where the tower scratch
// starts and runs over as many of its buffers as it needs -- it is dead behind the patch GEMM, in front of the first step of the
// blocks -- and the scratch is at least as large as col.  out / the token output / the images or token ids are the caller's, as x is
// for the kind "tower", whose layout is tower_layout().
inline TowerLayout pass_layout(const PassArgs& a) {
    const TowerPlanArgs& t = a.t;
    TowerLayout L = tower_layout(t.flow, t.width, t.seq, t.B);
    if (a.kind == KEDS_PASS_TOWER) return L;
    const bool f32 = tower_flow_f32(t.flow);
    const int e = f32 ? 4 : 2;
    const size_t w = (size_t)t.width, xb = tower_align(L.b[TB_X].bytes, 256);
    for (int id = TB_H; id < TB_N; ++id) L.b[id].off += xb;
    L.b[TB_X].caller = false;
    size_t tb = L.total;
    if (pass_is_vit(a.kind)) {
        L.b[TB_COL] = TowerBuf{xb, tower_pad_rows((size_t)t.B * (t.seq - 1)) * a.kpad * e, a.kpad, e, f32 ? TB_LN : TB_H, false};
        if (tower_align(L.b[TB_COL].bytes, 256) > tb) tb = tower_align(L.b[TB_COL].bytes, 256);
        L.b[TB_SRC] = TowerBuf{0, (size_t)t.B * 3 * a.resolution * a.resolution * 4, 3 * a.resolution * a.resolution, 4, TB_NONE, true};
    } else {
        L.b[TB_SRC] = TowerBuf{0, (size_t)t.B * a.context * 4, a.context, 4, TB_NONE, true};
    }
    L.b[TB_RO] = TowerBuf{xb + tb, tower_align((size_t)t.B, 128) * w * e, t.width, e, TB_NONE, false};
    L.total = xb + tb + tower_align(L.b[TB_RO].bytes, 256);
    if (a.kind == KEDS_PASS_TEXT_TOKENS) {
        const int eo = a.out_type == 1 ? 4 : 2;
        L.b[TB_TOK] = TowerBuf{0, (size_t)t.B * t.seq * w * eo, t.width, eo, TB_NONE, true};
    } else if (a.readout) {
        L.b[TB_OUT] = TowerBuf{0, (size_t)t.B * a.embed_dim * 4, a.embed_dim, 4, TB_NONE, true};
    }
    return L;
}

// The steps of a whole pass in enqueue order: the front end, exactly tower_plan()'s steps, the read-out.
template <typename Emit>
inline bool pass_plan(const PassArgs& a, Emit&& emit) {
    const TowerPlanArgs& t = a.t;
    const int S = t.seq, B = t.B;
    const bool f32 = tower_flow_f32(t.flow);
    const int type = f32 ? 1 : t.flow == KEDS_TOWER_FLOW_FP16 ? 2 : 0;      // keds_layernorm_ex's output type of the flow's operands
    bool go = true;
    auto put = [&](const TowerStep& s) { go = go && emit(s); };
    if (pass_is_vit(a.kind)) {
        TowerStep c;
        c.op = KEDS_TOWER_OP_IM2COL, c.epi = type;
        c.in = TB_SRC, c.out = TB_COL, c.n = B * (S - 1);
        put(c);
        TowerStep g;                    // patch rows + positional embedding: row i of col is row i / (S - 1) * S + 1 + i % (S - 1) of x
        g.op = f32 ? KEDS_TOWER_OP_GEMM_F32 : KEDS_TOWER_OP_GEMM16, g.weight = TW_CONV;
        g.epi = f32 ? KEDS_F32_EPI_PATCH : type == 2 ? KEDS_EPI_PATCH_F32_H : KEDS_EPI_PATCH_F32;
        g.in = TB_COL, g.out = TB_X, g.n = B * (S - 1);
        put(g);
        TowerStep k;
        k.op = KEDS_TOWER_OP_CLS;
        k.out = TB_X, k.out_step = S, k.n = B;
        put(k);
        TowerStep ln;                   // ln_pre in place (each wave holds its whole row in registers before it stores)
        ln.op = KEDS_TOWER_OP_LN, ln.weight = TW_LN_PRE, ln.epi = 1;
        ln.in = ln.out = TB_X, ln.n = B * S;
        put(ln);
    }
    go = go && tower_plan(t, [&](const TowerStep& s) { put(s); return go; }, [&] {
        if (!pass_is_text(a.kind)) return;
        TowerStep e;                    // the first S columns of every token row (packed: of sample b, its own rows' worth)
        e.op = KEDS_TOWER_OP_EMBED;
        e.in = TB_SRC, e.out = TB_X, e.n = B * S, e.packed = t.packed_rows != 0;
        put(e);
    });
    if (a.kind == KEDS_PASS_TEXT_TOKENS) {
        TowerStep ln;                   // ln_final over all rows, as out_type
        ln.op = KEDS_TOWER_OP_LN, ln.weight = TW_LN_OUT, ln.epi = a.out_type;
        ln.in = TB_X, ln.out = TB_TOK, ln.n = B * S;
        put(ln);
    } else if (a.readout && a.kind != KEDS_PASS_TOWER) {
        // behind a read-out-row tail row b of x is sample b's; else the CLS row, or the read-out column of the sample's S rows
        const bool compact = t.tail == TAIL_READOUT;
        readout_plan(type, B, compact ? 1 : S, pass_is_text(a.kind) && !compact, a.normalize != 0, put);
    }
    return go;
}

}  // namespace
