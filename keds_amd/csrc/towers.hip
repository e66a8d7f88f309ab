// Whole-tower forward passes built from the kernels in gemm/attention/elementwise/f32path:
//   keds_tower_forward : N pre-LN residual blocks        (src/model/model.py:305-326,372-373)
//   keds_vit_run   : CLIP.encode_image, ViT branch   (src/model/model.py:569-575,393-415)
//   keds_text_run  : CLIP.encode_text / encode_text_img_retrieval (src/model/model.py:577-590,808-851)
//   keds_vit_run_tokens / keds_text_run_tokens : encode_image(mid_feature=True), VisualTransformer.get_tokens,
//                    CLIP.get_text_tokens (model.py:337-342, 393-427, 592-605): per-block taps / all tokens of the same passes
// What a pass launches -- front end, blocks and read-out, flow by flow -- is decided in tower_plan.h (pass_plan); every entry here
// checks its arguments, describes its pass as a keds_pass_shape and hands it to run_pass(); tower_step() runs one step and is the
// only place a pass calls a GEMM, attention, LayerNorm, embedding or normalisation entry from.
// Host code only: every launch is asynchronous on the caller's stream, the caller owns the
// workspace, nothing is allocated or synchronised here.
#include "keds_common.h"
#include "tower_plan.h"
#include <cstdlib>
#include <cstring>
#include <optional>

namespace {

static_assert(TOWER_SPLITK_BYTES == KEDS_SPLITK_BYTES, "tower_plan.h carves the split-K scratch");

// What the front end and the read-out of a pass read (the blocks' weights: keds_tower_params)
struct PassWeights {
    const void *conv_w = nullptr, *proj_t = nullptr;
    const float *pos_emb = nullptr, *class_emb = nullptr, *token_emb = nullptr;
    const float *ln_pre_g = nullptr, *ln_pre_b = nullptr, *ln_out_g = nullptr, *ln_out_b = nullptr;      // ln_out: ln_post / ln_final
};

// One pass in flight: where the plan's buffer ids and lanes point
struct TowerRun {
    const keds_tower_params* p = nullptr;
    PassArgs a{};
    PassWeights fw;
    int flow = 0, B = 0;
    TowerLayout L;
    char* base[PB_N] = {};          // every buffer's first byte: in the workspace, or the caller's own
    hipStream_t main = nullptr;
    KedsSideLane* lane = nullptr;   // its stream and its own two events, created once (round 1 made and destroyed a pair on every tower call)
    const int32_t *rows = nullptr, *seq_off = nullptr;  // device: the read-out row of every sample; the packed rows' offsets
    const float* img_tokens = nullptr;                  // device: the pseudo tokens the embedding splices in
    const KedsTaps* tp = nullptr;
    int* guard = nullptr;           // x3: the numerics guard of the calling thread's composite call
    char* at(int buf, int r0 = 0) const { return base[buf] + (size_t)r0 * L.b[buf].cols * L.b[buf].esize; }
    char* at_or_null(int buf, int r0 = 0) const { return buf == TB_NONE ? nullptr : at(buf, r0); }
    long long ld(int buf, int step) const { return (long long)step * L.b[buf].cols; }
};

struct TowerWeight {
    const void *w, *scales;         // (scales: MXFP8)
    const float* bias;
    int N, K, x3_exp;
    const float* aux = nullptr;     // the patch embedding: the positional embedding and the patches per image
    int aux_i = 0;
};
TowerWeight tower_weight(const TowerRun& r, const TowerStep& s) {
    const int w = r.p->width;
    if (s.weight == TW_CONV) return TowerWeight{r.fw.conv_w, nullptr, nullptr, w, r.a.kpad, 0, r.fw.pos_emb, r.a.t.seq - 1};
    if (s.weight == TW_PROJ_T) return TowerWeight{r.fw.proj_t, nullptr, nullptr, r.L.b[TB_OUT].cols, w, 0};
    const keds_block_params& k = r.p->blocks[s.layer];
    const bool mx = s.op == KEDS_TOWER_OP_GEMM_MX;
    switch (s.weight) {
        case TW_QKV: return mx ? TowerWeight{k.qkv_q8, k.qkv_s8, k.qkv_bc8, 3 * w, w, 0} : TowerWeight{k.qkv_w, nullptr, k.qkv_b, 3 * w, w, k.x3_exp[0]};
        case TW_OUT: return mx ? TowerWeight{k.out_q8, k.out_s8, k.out_b, w, w, 0} : TowerWeight{k.out_w, nullptr, k.out_b, w, w, k.x3_exp[1]};
        case TW_FC: return mx ? TowerWeight{k.fc_q8, k.fc_s8, k.fc_bc8, 4 * w, w, 0} : TowerWeight{k.fc_w, nullptr, k.fc_b, 4 * w, w, k.x3_exp[2]};
        case TW_PROJ: return mx ? TowerWeight{k.proj_q8, k.proj_s8, k.proj_b, w, 4 * w, 0} : TowerWeight{k.proj_w, nullptr, k.proj_b, w, 4 * w, k.x3_exp[3]};
        case TW_QKV_FOLDED: return TowerWeight{k.qkv_wf, nullptr, k.qkv_bc, 3 * w, w, 0};
        case TW_FC_FOLDED: return TowerWeight{k.fc_wf, nullptr, k.fc_bc, 4 * w, w, 0};
    }
    return TowerWeight{};
}

// the attention of a step: bf16 or fp16, rectangular or packed rows, and for the fp8 tower rows < q8_rows as MXFP8 into aq / as (the
// 16-bit flows); fp32; split fp16 with its output as fp32 rows or as the out-projection's operand planes.  stop / taken: AttnArgs
int tower_attention(const TowerRun& r, const TowerStep& s, hipEvent_t stop, bool* taken) {
    const keds_tower_params* p = r.p;
    const int S = r.a.t.seq;
    const int32_t* off = s.packed ? r.seq_off : nullptr;
    const float* qkv = (const float*)r.at(s.in);
    if (r.flow == KEDS_TOWER_FLOW_F32) return attention_f32_impl(qkv, (float*)r.at(s.out), r.B, S, p->heads, p->causal, s.q_limit, off, r.main);
    if (r.flow == KEDS_TOWER_FLOW_X3) {
        const bool planes = s.out == TB_LN;
        return keds_attention_x3_impl(qkv, planes ? nullptr : (float*)r.at(s.out), planes ? r.at(s.out) : nullptr, r.ld(s.out, planes ? s.plane_rows : 0),
                                      r.B, S, p->heads, p->causal, s.q_limit, r.guard, off, r.main);
    }
    const AttnArgs a{qkv, r.at(s.out), r.B, S, p->heads, r.at_or_null(s.out2), s.out2 ? r.at(s.out2 + 1) : nullptr, s.q8_rows, off, r.main, stop};
    return keds_attention16(a, p->f16, p->causal, s.q_limit, taken);
}

int tower_hip_error(const char* what) {
    keds_set_error("keds_tower_forward: %s: %s", what, hipGetErrorString(hipGetLastError()));
    return KEDS_E_LAUNCH;
}

// One step of a pass.  Every kernel entry a pass uses has its one call site here.
int tower_step(const TowerRun& r, const TowerStep& s) {
    const keds_tower_params* p = r.p;
    const PassArgs& a = r.a;
    const int w = p->width;
    hipStream_t st = s.lane ? r.lane->s : r.main;
    const keds_block_params* k = s.layer >= 0 ? &p->blocks[s.layer] : nullptr;
    const void* in = r.at_or_null(s.in, s.in_r0);
    void* out = r.at_or_null(s.out, s.out_r0);
    // the statistics a LayerNorm-folded GEMM reads or a residual GEMM adds into, and the buffer the former clears for the next producer
    float* stats = (float*)r.at_or_null(s.st_read ? s.st_read : s.st_add, s.st_r0);
    void* stats_clear = r.at_or_null(s.st_clear, s.st_r0);
    const size_t out_row_bytes = s.out ? (size_t)r.L.b[s.out].cols * r.L.b[s.out].esize : 0;
    switch (s.op) {
        case KEDS_TOWER_OP_IM2COL:
            if (s.epi == 1) return keds_im2col_f32((const float*)in, (float*)out, r.B, a.resolution, a.patch, a.kpad, st);
            return keds_im2col_ex((const float*)in, out, s.epi == 2, r.B, a.resolution, a.patch, a.kpad, st);
        case KEDS_TOWER_OP_CLS: return keds_cls_rows_impl((float*)out, r.fw.class_emb, r.fw.pos_emb, s.n, s.out_step, w, st);
        case KEDS_TOWER_OP_EMBED:
            return keds_embed_tokens_impl((const int32_t*)in, r.fw.token_emb, r.fw.pos_emb, r.img_tokens, a.n_tok, a.insert_col, (float*)out, r.B,
                                          a.context, s.n / r.B, w, st, s.packed ? r.seq_off : nullptr);
        case KEDS_TOWER_OP_L2NORM:
            if (s.epi) return keds_l2norm_rows_f32_impl((float*)out, s.n, r.L.b[s.out].cols, st);
            return keds_l2_normalize((const float*)in, (float*)out, s.n, r.L.b[s.out].cols, st);
        case KEDS_TOWER_OP_ZERO:
            return hipMemsetAsync(out, 0, (size_t)s.n * out_row_bytes, st) == hipSuccess ? KEDS_OK : tower_hip_error("packed rows");
        case KEDS_TOWER_OP_STATS_CAST: return keds_rowstats_cast_ex((const float*)in, out, s.epi, stats, s.n, w, st);
        case KEDS_TOWER_OP_QUANT: return keds_quantize_mxfp8(in, 0, s.n, w, s.n, out, r.at(s.out + 1), st);
        case KEDS_TOWER_OP_CAST: return keds_cast_rows_f16_f32_impl(in, (float*)out, s.n, w, r.ld(s.in, s.in_step), st);
        case KEDS_TOWER_OP_COPY: {
            const hipError_t e = s.epi ? hipMemcpy2DAsync(out, s.out_step * out_row_bytes, in, s.in_step * out_row_bytes, out_row_bytes, s.n,
                                                          hipMemcpyDeviceToDevice, st)
                                       : hipMemcpyAsync(out, in, s.n * out_row_bytes, hipMemcpyDeviceToDevice, st);
            return e == hipSuccess ? KEDS_OK : tower_hip_error("read-out rows");
        }
        case KEDS_TOWER_OP_SPLIT: return keds_split_f16_pair((const float*)in, w, s.n, w, out, r.ld(s.out, s.plane_rows), r.guard, st);
        case KEDS_TOWER_OP_GATHER: return keds_gather_rows_impl(in, out, r.rows, s.bound, s.n, w, s.epi, st, s.global != 0);
        case KEDS_TOWER_OP_LN:
        case KEDS_TOWER_OP_LN_PAIR: {
            const float *g = nullptr, *b = nullptr;
            switch (s.weight) {
                case TW_LN1: g = k->ln1_g, b = k->ln1_b; break;
                case TW_LN2: g = k->ln2_g, b = k->ln2_b; break;
                case TW_LN_PRE: g = r.fw.ln_pre_g, b = r.fw.ln_pre_b; break;
                case TW_LN_OUT: g = r.fw.ln_out_g, b = r.fw.ln_out_b; break;
            }
            if (s.op == KEDS_TOWER_OP_LN)
                return keds_layernorm_impl((const float*)in, w, s.rows ? r.rows : nullptr, s.in_step, g, b, out, s.epi, s.n, w, st);
            return keds_layernorm_pair_impl((const float*)in, w, g, b, out, r.ld(s.out, s.plane_rows), s.n, w, st);
        }
        case KEDS_TOWER_OP_ATTN: {
            bool taken = false;
            return tower_attention(r, s, nullptr, &taken);
        }
        case KEDS_TOWER_OP_ATTN_FORK: {
            // the launch records the fork event itself (its stop event); kernel forms that do not take it get the recorded event
            bool taken = false;
            keds_order_lock();
            int rc = tower_attention(r, s, r.lane->fork, &taken);
            if (!rc && taken) rc = keds_stream_wait_locked(r.lane->fork, r.lane->s);
            keds_order_unlock();
            if (!rc && !taken) rc = keds_stream_order(r.main, r.lane->fork, r.lane->s);
            return rc;
        }
        case KEDS_TOWER_OP_GEMM16: {       // (aux: the row statistics of the folded flows, or the patch embedding's positions)
            const TowerWeight wt = tower_weight(r, s);
            if (int rc = keds_gemm_bt_ex2(in, r.ld(s.in, s.in_step), wt.w, wt.bias, out, r.ld(s.out, s.out_step), s.n, wt.N, wt.K, s.epi,
                                          wt.aux ? wt.aux : stats, wt.aux_i, stats_clear, st))
                return rc;
            if (s.bound > 0) {      // packed rows: the zero rows of the stream and of their statistics stay zero (tower_plan.h, folded_gemm)
                const size_t n = (size_t)(s.out_r0 + s.n - s.bound);
                if (hipMemsetAsync(r.at(s.out, s.bound), 0, n * out_row_bytes, st) != hipSuccess ||
                    hipMemsetAsync(r.at(s.st_add, s.bound), 0, n * 2 * sizeof(keds_stat_t), st) != hipSuccess)
                    return tower_hip_error("packed rows");
            }
            return KEDS_OK;
        }
        case KEDS_TOWER_OP_GEMM_MX: {      // (m_pad and q_pad: the s.n full-tile rows the MXFP8 buffers are carved for)
            const TowerWeight wt = tower_weight(r, s);
            const bool mx_out = s.out == TB_HQ;      // c_fc writes the MLP hidden layer as MXFP8 only
            const int q = mx_out ? s.out : s.out2;
            return keds_gemm_mxfp8_ex(in, r.at(s.in + 1), s.n, wt.w, wt.scales, wt.N, wt.bias, mx_out ? nullptr : out, s.n, wt.N, wt.K, s.epi,
                                      stats, (float*)stats_clear, r.at_or_null(q), q ? r.at(q + 1) : nullptr, q ? s.n : 0, st);
        }
        case KEDS_TOWER_OP_GEMM_F32: {
            const TowerWeight wt = tower_weight(r, s);
            return keds_gemm_f32((const float*)in, r.ld(s.in, s.in_step), (const float*)wt.w, wt.bias, (float*)out, r.ld(s.out, s.out_step), s.n,
                                 wt.N, wt.K, s.epi, wt.aux, wt.aux_i, st);
        }
        case KEDS_TOWER_OP_GEMM_X3: {      // operand planes plane_rows apart; c_fc writes the MLP hidden layer as planes too
            const TowerWeight wt = tower_weight(r, s);
            return keds_gemm_x3(in, r.ld(s.in, s.plane_rows), r.ld(s.in, s.in_step), wt.w, (long long)wt.N * wt.K, wt.bias, out,
                                r.ld(s.out, s.out_step), s.n, wt.N, wt.K, s.epi,
                                s.epi == KEDS_EPI_X3_QGELU_PAIR ? (int)r.ld(s.out, s.plane_rows) : 0, wt.x3_exp, st);
        }
        case KEDS_TOWER_OP_TAP: return keds_tap_rows(r.tp, s.layer, p->layers, r.at(s.in), s.epi, s.in_r0, s.n, w, st);
        case KEDS_TOWER_OP_FORK: return keds_stream_order(r.main, r.lane->fork, r.lane->s);
        case KEDS_TOWER_OP_JOIN: return keds_stream_order(r.lane->s, r.lane->join, r.main);
    }
    keds_set_error("keds_tower_forward: unknown step %d", s.op);
    return KEDS_E_ARG;
}

int tower_bad(const char* why) {
    keds_set_error("%s", why);
    return KEDS_E_ARG;
}

// Runs the pass an entry has described: q carries the entry's own fields (the tower's geometry, its flow and the lanes are filled in
// here), r what the steps read and the caller's own buffers -- p, fw, tp (nullable: keds_vit_run_tokens' taps), rows (the read-out
// column of every sample; packed rows: its GLOBAL row), seq_off (packed rows), img_tokens, and base[] of x (keds_tower_forward: the
// other kinds keep x in the workspace), src, out and tok
int run_pass(TowerRun& r, keds_pass_shape q, void* workspace, void* stream) {
    const keds_tower_params* p = r.p;
    const char* why = nullptr;
    q.flow = tower_flow(p, &why);
    if (q.flow < 0) return tower_bad(why);
    q.width = p->width, q.heads = p->heads, q.layers = p->layers, q.causal = p->causal;
    r.a = pass_args(q);
    TowerPlanArgs& t = r.a.t;
    if ((why = tower_plan_check(t))) return tower_bad(why);
    t.split = pass_splits_rows(t);
    r.lane = t.split ? keds_side_lane() : nullptr;      // (created on first use; null: disabled, everything on `stream`)
    t.lane = r.lane != nullptr;
    r.flow = q.flow, r.B = q.B, r.main = (hipStream_t)stream;
    r.guard = q.flow == KEDS_TOWER_FLOW_X3 ? keds_numerics_guard() : nullptr;
    r.L = pass_layout(r.a);
    for (int id = 0; id < PB_N; ++id)
        if (!r.L.b[id].caller) r.base[id] = (char*)workspace + r.L.b[id].off;
    std::optional<KedsSplitKScope> splitk;      // this call's GEMMs split K into this call's scratch only
    if (r.L.b[TB_SPLITK].bytes) splitk.emplace(r.at(TB_SPLITK), KEDS_SPLITK_BYTES);
    int rc = KEDS_OK;
    pass_plan(r.a, [&](const TowerStep& s) {
        rc = tower_step(r, s);
        return rc == KEDS_OK;
    });
    return rc;
}

// the workspace of a pass kind on `seq` rows per sample (tower_plan.h, pass_layout: the 16-bit flows share one size, the fp32 flows another)
size_t pass_bytes(int kind, const keds_tower_params& tw, int seq, int B, int kpad) {
    PassArgs a{};
    a.kind = kind, a.kpad = kpad;
    a.t.flow = tw.f32 ? KEDS_TOWER_FLOW_F32 : KEDS_TOWER_FLOW_BF16, a.t.width = tw.width, a.t.seq = seq, a.t.B = B;
    return pass_layout(a).total;
}

int check_tower(const keds_tower_params* p, const char* who) {
    if (!p || !p->blocks || p->layers <= 0) {
        keds_set_error("%s: missing tower parameters", who);
        return KEDS_E_ARG;
    }
    if (p->width % 128 != 0 || p->width != p->heads * 64) {
        keds_set_error("%s: width %d must be heads*64 and a multiple of 128", who, p->width);
        return KEDS_E_ARG;
    }
    if (p->seq < 1 || p->seq > 288) {
        keds_set_error("%s: sequence length %d unsupported", who, p->seq);
        return KEDS_E_ARG;
    }
    if (p->f16 && (p->fp8 || p->f32)) {
        keds_set_error("%s: f16 (the fp16 operating point) excludes fp8 and f32", who);
        return KEDS_E_ARG;
    }
    return KEDS_OK;
}

// steps, buffer table (the first n_buffers ids) and workspace bytes of a checked pass, for the two queries
int pass_query_out(const PassArgs& a, int32_t* steps, int max_steps, int* n_steps, int64_t* buffers, int n_buffers, size_t* workspace_bytes) {
    int n = 0;
    pass_plan(a, [&](const TowerStep& s) {
        if (n < max_steps) memcpy(steps + (size_t)n * KEDS_TOWER_STEP_INTS, &s, sizeof s);
        ++n;
        return true;
    });
    *n_steps = n;
    const TowerLayout L = pass_layout(a);
    for (int id = 0; buffers && id < n_buffers; ++id) {
        const int64_t row[4] = {id, L.b[id].caller ? -1 : (int64_t)L.b[id].off, (int64_t)L.b[id].bytes, L.b[id].alias_of};
        memcpy(buffers + 4 * id, row, sizeof row);
    }
    if (workspace_bytes) *workspace_bytes = L.total;
    return KEDS_OK;
}

}  // namespace

// ln_post / ln_final of the read-out rows + projection (+ L2 normalisation) as keds_readout runs them (elementwise.hip checks the
// arguments): the read-out steps of a bf16 pass on the caller's buffers
int keds_run_readout(const float* x, int S, const int32_t* row, const float* gamma, const float* beta, const void* proj_t, float* out,
                     int B, int d, int E, int normalize, void* workspace, hipStream_t st) {
    keds_tower_params tw{};
    tw.width = d;
    TowerRun r;
    r.p = &tw, r.B = B, r.main = st, r.rows = row;
    r.fw.ln_out_g = gamma, r.fw.ln_out_b = beta, r.fw.proj_t = proj_t;
    r.L.b[TB_X] = TowerBuf{0, 0, d, 4, TB_NONE, true};
    r.L.b[TB_RO] = TowerBuf{0, 0, d, 2, TB_NONE, true};
    r.L.b[TB_OUT] = TowerBuf{0, 0, E, 4, TB_NONE, true};
    r.base[TB_X] = (char*)x, r.base[TB_RO] = (char*)workspace, r.base[TB_OUT] = (char*)out;
    int rc = KEDS_OK;
    readout_plan(0, B, S, row != nullptr, normalize != 0, [&](const TowerStep& s) {
        if (!rc) rc = tower_step(r, s);
    });
    return rc;
}

extern "C" size_t keds_tower_workspace_bytes(int width, int seq, int B) {
    return tower_layout(KEDS_TOWER_FLOW_BF16, width, seq, B).total;
}

extern "C" size_t keds_tower_workspace_bytes_ex(const keds_tower_params* p, int B) {
    if (!p || B <= 0) return 0;
    return tower_layout(p->f32 ? KEDS_TOWER_FLOW_F32 : KEDS_TOWER_FLOW_BF16, p->width, p->seq, B).total;
}

extern "C" int keds_tower_side_rows(int width, int seq, int B, int fp8) {
    if (width <= 0 || seq <= 0 || B <= 0) return 0;
    const int M = B * seq;
    const bool split = tower_splits_rows(fp8 ? KEDS_TOWER_FLOW_FP8 : KEDS_TOWER_FLOW_BF16, M, width);
    return split && keds_side_lane_enabled() ? M % 256 : 0;    // only a query: no stream is created here (no GPU needed)
}

extern "C" int keds_tower_plan_query(int flow, int width, int heads, int seq, int causal, int layers, int B, int tail, int packed_rows,
                                     int packed_valid, int taps, int split, int lane, int32_t* steps, int max_steps, int* n_steps,
                                     int64_t* buffers, size_t* workspace_bytes) {
    PassArgs a{};
    a.kind = KEDS_PASS_TOWER;
    a.t = TowerPlanArgs{flow, width, heads, seq, causal != 0, layers, B, tail, packed_rows, packed_valid, taps != 0, split > 0, lane > 0};
    if (const char* why = tower_plan_check(a.t)) return tower_bad(why);
    KEDS_REQUIRE(n_steps && (steps || max_steps <= 0), "keds_tower_plan_query: null pointer");
    if (split < 0) a.t.split = pass_splits_rows(a.t);
    if (lane < 0) a.t.lane = keds_side_lane_enabled();
    return pass_query_out(a, steps, max_steps, n_steps, buffers, TB_N, workspace_bytes);
}

extern "C" int keds_pass_plan_query(const keds_pass_shape* shape, int32_t* steps, int max_steps, int* n_steps, int64_t* buffers,
                                    size_t* workspace_bytes) {
    KEDS_REQUIRE(shape && n_steps && (steps || max_steps <= 0), "keds_pass_plan_query: null pointer");
    PassArgs a = pass_args(*shape);
    if (const char* why = pass_plan_check(a)) return tower_bad(why);
    if (shape->split < 0) a.t.split = pass_splits_rows(a.t);
    if (shape->lane < 0) a.t.lane = keds_side_lane_enabled();
    return pass_query_out(a, steps, max_steps, n_steps, buffers, PB_N, workspace_bytes);
}

extern "C" int keds_text_runs_packed(int causal, int fp8, int trim, int64_t rows_total, int B, int seq_used) {
    return text_runs_packed(causal != 0, fp8 != 0, trim, rows_total, B, seq_used);
}

extern "C" int keds_tower_forward(const keds_tower_params* p, float* x, int B, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    int rc = check_tower(p, "keds_tower_forward");
    if (rc) return rc;
    KEDS_REQUIRE(x && workspace && B > 0, "keds_tower_forward: bad argument");
    if (workspace_bytes < keds_tower_workspace_bytes_ex(p, B)) {
        keds_set_error("keds_tower_forward: workspace too small");
        return KEDS_E_WORKSPACE;
    }
    keds_pass_shape q{};
    q.kind = KEDS_PASS_TOWER, q.B = B, q.seq = p->seq, q.cls_only = p->last_cls_only;
    TowerRun r;
    r.p = p, r.base[TB_X] = (char*)x;
    return run_pass(r, q, workspace, stream);
}

// ---- ViT -------------------------------------------------------------------------------------
extern "C" size_t keds_vit_workspace_bytes(const keds_vit_params* p, int B) {
    if (!p || B <= 0) return 0;
    return pass_bytes(KEDS_PASS_VIT, p->tower, p->tower.seq, B, p->kpad);
}

namespace {
// keds_vit_run and keds_vit_run_tokens.  tp (nullable): per-block taps / last-block tokens -- the last block then runs on every row
// and the CLS read-out comes from the full stream (KEDS_PASS_VIT_TOKENS); out nullable (no read-out) only with tp
int vit_run(const keds_vit_params* p, const float* image, int B, float* out, int normalize, void* workspace, size_t workspace_bytes,
            void* stream, const KedsTaps* tp, const char* who) {
    int rc = check_tower(&p->tower, who);
    if (rc) return rc;
    const int G = p->tower.seq - 1;
    const int g = p->resolution / p->patch;
    KEDS_REQUIRE(p->resolution % p->patch == 0 && g * g == G, "%s: seq must be (res/patch)^2 + 1", who);
    KEDS_REQUIRE(p->kpad % 64 == 0 && p->kpad >= 3 * p->patch * p->patch, "%s: bad kpad", who);
    KEDS_REQUIRE(p->embed_dim % 128 == 0, "%s: embed_dim must be a multiple of 128", who);
    const size_t need = keds_vit_workspace_bytes(p, B);
    if (workspace_bytes < need) {
        keds_set_error("%s: workspace %zu < %zu", who, workspace_bytes, need);
        return KEDS_E_WORKSPACE;
    }
    keds_pass_shape q{};
    q.kind = tp ? KEDS_PASS_VIT_TOKENS : KEDS_PASS_VIT, q.B = B, q.seq = p->tower.seq, q.cls_only = p->tower.last_cls_only;
    q.resolution = p->resolution, q.patch = p->patch, q.kpad = p->kpad, q.embed_dim = p->embed_dim;
    q.readout = out != nullptr, q.normalize = normalize;
    TowerRun r;
    r.p = &p->tower, r.tp = tp, r.base[TB_SRC] = (char*)image, r.base[TB_OUT] = (char*)out;
    PassWeights& fw = r.fw;               // (the fp32 flows: every weight pointer of the structs is an fp32 array; fp16: conv_w / proj_t fp16 too)
    fw.conv_w = p->conv_w, fw.proj_t = p->proj_t, fw.pos_emb = p->pos_emb, fw.class_emb = p->class_emb;
    fw.ln_pre_g = p->ln_pre_g, fw.ln_pre_b = p->ln_pre_b, fw.ln_out_g = p->ln_post_g, fw.ln_out_b = p->ln_post_b;
    return run_pass(r, q, workspace, stream);
}
}  // namespace

extern "C" int keds_vit_run(const keds_vit_params* p, const float* image, int B, float* out, int normalize,
                                void* workspace, size_t workspace_bytes, void* stream) {
    KEDS_REQUIRE(p && image && out && workspace && B > 0, "keds_vit_run: bad argument");
    return vit_run(p, image, B, out, normalize, workspace, workspace_bytes, stream, nullptr, "keds_vit_run");
}

// CLIP.encode_image(mid_feature=True) / VisualTransformer.get_tokens (model.py:393-427): the same pass with the residual stream
// after every block (taps [layers, B, S, w]) and / or after the last one (tokens [B, S, w]) written out as out_type.  Same
// workspace as keds_vit_run.
extern "C" int keds_vit_run_tokens(const keds_vit_params* p, const float* image, int B, float* out, int normalize, void* taps,
                                   void* tokens, int out_type, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "keds_vit_run_tokens";
    KEDS_REQUIRE(B >= 1, "%s: B = %d, at least 1 image", who, B);
    KEDS_REQUIRE(out || taps || tokens, "%s: no output requested (out, taps and tokens are all null)", who);
    KEDS_REQUIRE(out_type >= 0 && out_type <= 2, "%s: out_type %d (0 bf16, 1 fp32, 2 fp16)", who, out_type);
    KEDS_REQUIRE(p && image && workspace, "%s: bad argument (null params, image or workspace)", who);
    const KedsTaps tp{taps, tokens, out_type, (size_t)B * p->tower.seq};
    return vit_run(p, image, B, out, normalize, workspace, workspace_bytes, stream, taps || tokens ? &tp : nullptr, who);
}

// ---- text ------------------------------------------------------------------------------------
extern "C" size_t keds_text_workspace_bytes(const keds_text_params* p, int B) {
    if (!p || B <= 0) return 0;
    return pass_bytes(KEDS_PASS_TEXT, p->tower, p->tower.seq, B, 0);
}

namespace {
// the prologue the text entries share: the tower's shape (and the projection's), then the workspace for all L columns (a pass on
// fewer columns carves the same buffers for those columns: never more bytes)
int text_check(const keds_text_params* p, bool projects, const char* who) {
    int rc = check_tower(&p->tower, who);
    if (rc) return rc;
    KEDS_REQUIRE(!projects || p->embed_dim % 128 == 0, "%s: embed_dim must be a multiple of 128", who);
    return KEDS_OK;
}
int text_workspace(const keds_text_params* p, int B, size_t workspace_bytes, const char* who) {
    const size_t need = keds_text_workspace_bytes(p, B);
    if (workspace_bytes < need) {
        keds_set_error("%s: workspace %zu < %zu", who, workspace_bytes, need);
        return KEDS_E_WORKSPACE;
    }
    return KEDS_OK;
}
// a text pass of the entry's `kind`: q and r carry the entry's own fields and buffers
int text_run(const keds_text_params* p, keds_pass_shape q, TowerRun& r, const int32_t* tokens, int B, void* workspace, void* stream) {
    q.B = B, q.context = p->tower.seq, q.embed_dim = p->embed_dim, q.cls_only = p->tower.last_cls_only;
    r.p = &p->tower, r.base[TB_SRC] = (char*)tokens;
    PassWeights& fw = r.fw;
    fw.token_emb = p->token_emb, fw.pos_emb = p->pos_emb, fw.proj_t = p->proj_t, fw.ln_out_g = p->ln_final_g, fw.ln_out_b = p->ln_final_b;
    return run_pass(r, q, workspace, stream);
}
}  // namespace

// KEDS_TEXT_TRIM=0 in the environment: the round-4 flow (all L columns through all blocks) for an A/B or a bisect
static bool text_trim_on() {
    static int v = -1;
    if (v < 0) {
        const char* e = getenv("KEDS_TEXT_TRIM");
        v = !(e && e[0] == '0');
    }
    return v != 0;
}
static int g_text_trim = -1;                     // run-time override (keds_text_trim_enable: tests, A/B); -1: the environment
extern "C" int keds_text_trim_enable(int on) {   // 0 off, 1 on, 2 the column cut only, 3 the read-out-row tail only
    g_text_trim = on < 0 || on > 3 ? -1 : on;
    return KEDS_OK;
}
extern "C" int keds_text_trim_mode(void) {       // the flow in force: 1 = cut + read-out-row tail (the default; what packed rows build on)
    return g_text_trim < 0 ? (text_trim_on() ? 1 : 0) : g_text_trim;
}

// Work that cannot reach the read-out is not done (round 5):
//  * the mask is causal (model.py:543-549), so columns to the right of the last read-out column change no row that is read:
//    `seq_used` (host-known: max(readout_row) + 1; 0 = unknown, all L columns) cuts the sequence there for the embedding, all
//    blocks and the workspace layout ([B, columns, w]);
//  * the last block's out-proj, ln_2 and MLP run on the B read-out rows only (tower_plan.h, the READOUT tail), as the ViT's do on the CLS rows.
// Which of the two the trim mode in force keeps: tower_plan.h, pass_args().
extern "C" int keds_text_run_ex(const keds_text_params* p, const int32_t* tokens, const int32_t* readout_row,
                                const float* img_tokens, int n_tok, int insert_col, int B, int seq_used, float* out,
                                int normalize, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "keds_text_run";
    KEDS_REQUIRE(p && tokens && readout_row && out && workspace && B > 0, "%s: bad argument", who);
    int rc = text_check(p, true, who);
    if (rc) return rc;
    KEDS_REQUIRE(seq_used >= 0 && seq_used <= p->tower.seq, "%s: seq_used %d outside [0, %d]", who, seq_used, p->tower.seq);
    if ((rc = text_workspace(p, B, workspace_bytes, who))) return rc;
    keds_pass_shape q{};
    q.kind = KEDS_PASS_TEXT, q.seq_used = seq_used, q.trim = keds_text_trim_mode();
    q.n_tok = n_tok, q.insert_col = insert_col, q.normalize = normalize;
    TowerRun r;
    r.img_tokens = img_tokens, r.rows = readout_row, r.base[TB_OUT] = (char*)out;
    return text_run(p, q, r, tokens, B, workspace, stream);
}

// The same on PACKED rows (round 6).  Captions end at different columns and under the causal mask (model.py:543-549) a column to
// the right of a caption's own read-out column reaches nothing that is read of THAT caption: sample b needs columns
// [0, len_b) only, len_b = its read-out column + 1.  keds_text_run_ex cuts every sample at the batch's longest caption (B x max len
// rows); here sample b owns rows [seq_off[b], seq_off[b + 1]) and the tower runs sum(len_b) rows -- at bench.py's captions (read-out
// columns 10 .. 42) 6.9 k instead of 11 k rows for the dual workload's 2B-row pass, whole rounds of workgroups fewer in every GEMM.
//   seq_off         device int32 [B + 1]: 0 = seq_off[0] <= ... <= seq_off[B] = rows_total, 1 <= len_b <= seq_max
//   readout_global  device int32 [B]: seq_off[b] + the read-out column of sample b (a row outside [0, rows_total) comes out as NaN)
// Causal bf16 / fp32 / fp32x3 towers with the read-out-row tail (the default flow); anything else (the MXFP8 tower,
// KEDS_TEXT_TRIM=0) is the caller's to route through keds_text_run_ex.
extern "C" int keds_text_run_packed(const keds_text_params* p, const int32_t* tokens, const int32_t* seq_off,
                                    const int32_t* readout_global, int rows_total, int seq_max, const float* img_tokens, int n_tok,
                                    int insert_col, int B, float* out, int normalize, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    const char* who = "keds_text_run_packed";
    KEDS_REQUIRE(p && tokens && seq_off && readout_global && out && workspace && B > 0, "%s: bad argument", who);
    int rc = text_check(p, true, who);
    if (rc) return rc;
    const int L = p->tower.seq;
    KEDS_REQUIRE(p->tower.causal && !p->tower.fp8, "%s: a causal bf16 / fp32 / fp32x3 tower (the MXFP8 tower keeps the rectangular layout)", who);
    KEDS_REQUIRE(keds_text_trim_mode() == 1, "%s: the A/B flows of keds_text_trim_enable / KEDS_TEXT_TRIM=0 go through keds_text_run_ex", who);
    KEDS_REQUIRE(seq_max >= 1 && seq_max <= L && rows_total >= B && (long long)rows_total <= (long long)B * seq_max,
                 "%s: rows_total %d / seq_max %d do not fit B = %d sequences of <= %d columns", who, rows_total, seq_max, B, L);
    if ((rc = text_workspace(p, B, workspace_bytes, who))) return rc;
    keds_pass_shape q{};
    q.kind = KEDS_PASS_TEXT_PACKED, q.seq_used = seq_max, q.rows_total = rows_total, q.trim = 1;
    q.n_tok = n_tok, q.insert_col = insert_col, q.normalize = normalize;
    TowerRun r;
    r.img_tokens = img_tokens, r.rows = readout_global, r.seq_off = seq_off, r.base[TB_OUT] = (char*)out;
    return text_run(p, q, r, tokens, B, workspace, stream);
}

// CLIP.get_text_tokens (model.py:592-605): ln_final over the residual stream of ALL L columns of every sample after the last block,
// out [B, L, w] as out_type -- the rectangular flow whatever keds_text_trim_enable / KEDS_TEXT_TRIM say (no column cut, no
// read-out-row tail, no packed rows; every column is an output), no projection.  Workspace: keds_text_workspace_bytes.
extern "C" int keds_text_run_tokens(const keds_text_params* p, const int32_t* tokens, int B, void* out, int out_type, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    const char* who = "keds_text_run_tokens";
    KEDS_REQUIRE(B >= 1, "%s: B = %d, at least 1 sequence", who, B);
    KEDS_REQUIRE(out, "%s: no output requested (out is null)", who);
    KEDS_REQUIRE(out_type >= 0 && out_type <= 2, "%s: out_type %d (0 bf16, 1 fp32, 2 fp16)", who, out_type);
    KEDS_REQUIRE(p && tokens && workspace, "%s: bad argument (null params, tokens or workspace)", who);
    int rc = text_check(p, false, who);
    if (rc) return rc;
    if ((rc = text_workspace(p, B, workspace_bytes, who))) return rc;
    keds_pass_shape q{};
    q.kind = KEDS_PASS_TEXT_TOKENS, q.out_type = out_type;
    TowerRun r;
    r.base[TB_TOK] = (char*)out;
    return text_run(p, q, r, tokens, B, workspace, stream);
}

extern "C" int keds_text_run(const keds_text_params* p, const int32_t* tokens, const int32_t* readout_row,
                                 const float* img_tokens, int n_tok, int insert_col, int B, float* out, int normalize,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    return keds_text_run_ex(p, tokens, readout_row, img_tokens, n_tok, insert_col, B, 0, out, normalize, workspace,
                            workspace_bytes, stream);
}
