// Whole-tower forward passes built from the kernels in gemm/attention/elementwise/f32path:
//   keds_tower_forward : N pre-LN residual blocks        (src/model/model.py:305-326,372-373)
//   keds_vit_run   : CLIP.encode_image, ViT branch   (src/model/model.py:569-575,393-415)
//   keds_text_run  : CLIP.encode_text / encode_text_img_retrieval (src/model/model.py:577-590,808-851)
//   keds_vit_run_tokens / keds_text_run_tokens : encode_image(mid_feature=True), VisualTransformer.get_tokens,
//                    CLIP.get_text_tokens (model.py:337-342, 393-427, 592-605): per-block taps / all tokens of the same passes
// What a pass launches, flow by flow, is decided in tower_plan.h; tower_step() below runs one step of it and is the only place a
// tower pass calls a GEMM, attention or LayerNorm entry from.
// Host code only: every launch is asynchronous on the caller's stream, the caller owns the
// workspace, nothing is allocated or synchronised here.
#include "keds_common.h"
#include "tower_plan.h"
#include <cstdlib>
#include <cstring>
#include <optional>

namespace {

static_assert(TOWER_SPLITK_BYTES == KEDS_SPLITK_BYTES, "tower_plan.h carves the split-K scratch");

size_t pad_rows(size_t m) { return tower_pad_rows(m); }

// One pass in flight: where the plan's buffer ids and lanes point
struct TowerRun {
    const keds_tower_params* p;
    int flow, B;
    char *x, *ws;                   // the caller's fp32 stream; the tower scratch (TowerLayout)
    TowerLayout L;
    hipStream_t main;
    KedsSideLane* lane;             // its stream and its own two events, created once (round 1 made and destroyed a pair on every tower call)
    const int32_t *rows, *seq_off;  // device: the read-out row of every sample; the packed rows' offsets
    const KedsTaps* tp;
    int* guard;                     // x3: the numerics guard of the calling thread's composite call
    char* at(int buf, int r0 = 0) const {
        const TowerBuf& b = L.b[buf];
        return (buf == TB_X ? x : ws + b.off) + (size_t)r0 * b.cols * b.esize;
    }
    char* at_or_null(int buf, int r0 = 0) const { return buf == TB_NONE ? nullptr : at(buf, r0); }
    long long ld(int buf, int step) const { return (long long)step * L.b[buf].cols; }
};

struct TowerWeight {
    const void *w, *scales;         // (scales: MXFP8)
    const float* bias;
    int N, K, x3_exp;
};
TowerWeight tower_weight(const keds_block_params& k, const TowerStep& s, int w) {
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
    const int32_t* off = s.packed ? r.seq_off : nullptr;
    const float* qkv = (const float*)r.at(s.in);
    if (r.flow == KEDS_TOWER_FLOW_F32) return attention_f32_impl(qkv, (float*)r.at(s.out), r.B, p->seq, p->heads, p->causal, s.q_limit, off, r.main);
    if (r.flow == KEDS_TOWER_FLOW_X3) {
        const bool planes = s.out == TB_LN;
        return keds_attention_x3_impl(qkv, planes ? nullptr : (float*)r.at(s.out), planes ? r.at(s.out) : nullptr, r.ld(s.out, planes ? s.plane_rows : 0),
                                      r.B, p->seq, p->heads, p->causal, s.q_limit, r.guard, off, r.main);
    }
    const AttnArgs a{qkv, r.at(s.out), r.B, p->seq, p->heads, r.at_or_null(s.out2), s.out2 ? r.at(s.out2 + 1) : nullptr, s.q8_rows, off, r.main, stop};
    return keds_attention16(a, p->f16, p->causal, s.q_limit, taken);
}

int tower_hip_error(const char* what) {
    keds_set_error("keds_tower_forward: %s: %s", what, hipGetErrorString(hipGetLastError()));
    return KEDS_E_LAUNCH;
}

// One step of a pass.  Every kernel entry a tower pass uses has its one call site here.
int tower_step(const TowerRun& r, const TowerStep& s) {
    const keds_tower_params* p = r.p;
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
            const float *g = s.weight == TW_LN1 ? k->ln1_g : k->ln2_g, *b = s.weight == TW_LN1 ? k->ln1_b : k->ln2_b;
            if (s.op == KEDS_TOWER_OP_LN) return keds_layernorm_impl((const float*)in, w, nullptr, s.in_step, g, b, out, s.epi, s.n, w, st);
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
        case KEDS_TOWER_OP_GEMM16: {
            const TowerWeight wt = tower_weight(*k, s, w);
            return keds_gemm_bt_ex2(in, r.ld(s.in, s.in_step), wt.w, wt.bias, out, r.ld(s.out, s.out_step), s.n, wt.N, wt.K, s.epi, stats, 0,
                                    stats_clear, st);
        }
        case KEDS_TOWER_OP_GEMM_MX: {      // (m_pad and q_pad: the s.n full-tile rows the MXFP8 buffers are carved for)
            const TowerWeight wt = tower_weight(*k, s, w);
            const bool mx_out = s.out == TB_HQ;      // c_fc writes the MLP hidden layer as MXFP8 only
            const int q = mx_out ? s.out : s.out2;
            return keds_gemm_mxfp8_ex(in, r.at(s.in + 1), s.n, wt.w, wt.scales, wt.N, wt.bias, mx_out ? nullptr : out, s.n, wt.N, wt.K, s.epi,
                                      stats, (float*)stats_clear, r.at_or_null(q), q ? r.at(q + 1) : nullptr, q ? s.n : 0, st);
        }
        case KEDS_TOWER_OP_GEMM_F32: {
            const TowerWeight wt = tower_weight(*k, s, w);
            return keds_gemm_f32((const float*)in, r.ld(s.in, s.in_step), (const float*)wt.w, wt.bias, (float*)out, r.ld(s.out, s.out_step), s.n,
                                 wt.N, wt.K, s.epi, nullptr, 0, st);
        }
        case KEDS_TOWER_OP_GEMM_X3: {      // operand planes plane_rows apart; c_fc writes the MLP hidden layer as planes too
            const TowerWeight wt = tower_weight(*k, s, w);
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

// last_rows (device int32 [B], nullable): the one row of every sample that is read after the last block: on return x[b] (row b of
// the first B rows) holds that row of sample b; without it x holds every row (p->last_cls_only: the CLS rows)
// pk (nullable): packed rows -- M = pk->rows <= B * seq, the workspace is carved for B * seq; last_rows are global rows
// tp (nullable): per-block taps (KedsTaps, keds_vit_run_tokens); the caller clears last_cls_only for such a pass
// front: what the pass entry enqueues behind the clearing of the packed zero rows of x and in front of everything else (the embedding)
template <typename Front>
int run_tower(const keds_tower_params* p, float* x, int B, void* ws, hipStream_t st, const int32_t* last_rows, const PackedRows* pk,
              const KedsTaps* tp, Front&& front) {
    const char* why = nullptr;
    const int flow = tower_flow(p, &why);
    if (flow < 0) return tower_bad(why);
    TowerPlanArgs a{flow, p->width, p->heads, p->seq, p->causal != 0, p->layers, B,
                    last_rows ? TAIL_READOUT : p->last_cls_only ? TAIL_CLS : TAIL_ALL, pk ? pk->rows : 0, pk ? pk->valid : 0, tp != nullptr,
                    false, false};
    if ((why = tower_plan_check(a))) return tower_bad(why);
    const int M = pk ? pk->rows : B * p->seq;
    a.split = tower_splits_rows(flow == KEDS_TOWER_FLOW_FP8 && M < 256 ? KEDS_TOWER_FLOW_BF16 : flow, M, p->width);
    KedsSideLane* lane = a.split ? keds_side_lane() : nullptr;      // (created on first use; null: disabled, everything on `st`)
    a.lane = lane != nullptr;
    const TowerRun r{p, flow, B, (char*)x, (char*)ws, tower_layout(flow, p->width, p->seq, B), st, lane, last_rows, pk ? pk->off : nullptr, tp,
                     flow == KEDS_TOWER_FLOW_X3 ? keds_numerics_guard() : nullptr};
    std::optional<KedsSplitKScope> splitk;      // this call's GEMMs split K into this call's scratch only
    if (r.L.b[TB_SPLITK].bytes) splitk.emplace(r.at(TB_SPLITK), KEDS_SPLITK_BYTES);
    int rc = KEDS_OK;
    bool fronted = false;
    tower_plan(a, [&](const TowerStep& s) {
        if (!fronted && !(s.op == KEDS_TOWER_OP_ZERO && s.out == TB_X)) {
            fronted = true;
            if ((rc = front())) return false;
        }
        rc = tower_step(r, s);
        return rc == KEDS_OK;
    });
    return rc;
}
int run_tower(const keds_tower_params* p, float* x, int B, void* ws, hipStream_t st, const int32_t* last_rows = nullptr,
              const PackedRows* pk = nullptr, const KedsTaps* tp = nullptr) {
    return run_tower(p, x, B, ws, st, last_rows, pk, tp, [] { return KEDS_OK; });
}

// ln_post / ln_final of the read-out rows + projection (+ L2 normalisation), in the tower's arithmetic
size_t readout_bytes(const keds_tower_params& t, int B) {
    return t.f32 ? keds_readout_f32_workspace_bytes(B, t.width) : keds_readout_workspace_bytes(B, t.width);
}
int run_readout(const keds_tower_params& t, const float* x, int S, const int32_t* row, const float* gamma, const float* beta,
                const void* proj_t, float* out, int B, int E, int normalize, void* ro, void* stream) {
    if (t.f32) return keds_readout_f32(x, S, row, gamma, beta, (const float*)proj_t, out, B, t.width, E, normalize, ro, (hipStream_t)stream);
    return keds_readout_impl(x, S, row, gamma, beta, proj_t, out, B, t.width, E, normalize, ro, keds_readout_workspace_bytes(B, t.width), stream,
                             t.f16);
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

}  // namespace

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
    TowerPlanArgs a{flow, width, heads, seq, causal != 0, layers, B, tail, packed_rows, packed_valid, taps != 0, split > 0, lane > 0};
    if (const char* why = tower_plan_check(a)) return tower_bad(why);
    KEDS_REQUIRE(n_steps && (steps || max_steps <= 0), "keds_tower_plan_query: null pointer");
    const int M = packed_rows ? packed_rows : B * seq;
    if (split < 0) a.split = tower_splits_rows(flow == KEDS_TOWER_FLOW_FP8 && M < 256 ? KEDS_TOWER_FLOW_BF16 : flow, M, width);
    if (lane < 0) a.lane = keds_side_lane_enabled();
    int n = 0;
    tower_plan(a, [&](const TowerStep& s) {
        if (n < max_steps) memcpy(steps + (size_t)n * KEDS_TOWER_STEP_INTS, &s, sizeof s);
        ++n;
        return true;
    });
    *n_steps = n;
    const TowerLayout L = tower_layout(flow, width, seq, B);
    for (int id = 0; buffers && id < TB_N; ++id) {
        const int64_t row[4] = {id, id == TB_X ? -1 : (int64_t)L.b[id].off, (int64_t)L.b[id].bytes, L.b[id].alias_of};
        memcpy(buffers + 4 * id, row, sizeof row);
    }
    if (workspace_bytes) *workspace_bytes = L.total;
    return KEDS_OK;
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
    return run_tower(p, x, B, workspace, (hipStream_t)stream);
}

// ---- ViT -------------------------------------------------------------------------------------
namespace {
struct VitWs {
    float* x;      // [Mp, w] fp32 residual stream
    char* tower;   // tower scratch (the im2col matrix aliases its head)
    char* ro;      // read-out scratch
    size_t bytes;
};
VitWs carve_vit(const keds_vit_params* p, int B, void* ws) {
    VitWs v;
    char* base = (char*)ws;
    const int w = p->tower.width, S = p->tower.seq;
    const size_t Mp = pad_rows((size_t)B * S);
    const size_t xb = keds_align_up(Mp * w * sizeof(float), 256);
    size_t tb = keds_tower_workspace_bytes_ex(&p->tower, B);
    const size_t colb = keds_align_up(pad_rows((size_t)B * (S - 1)) * p->kpad * (p->tower.f32 ? 4 : 2), 256);
    if (colb > tb) tb = colb;
    const size_t rb = keds_align_up(readout_bytes(p->tower, B), 256);
    v.x = (float*)base;
    v.tower = base ? base + xb : nullptr;
    v.ro = base ? base + xb + tb : nullptr;
    v.bytes = xb + tb + rb;
    return v;
}
}  // namespace

extern "C" size_t keds_vit_workspace_bytes(const keds_vit_params* p, int B) {
    if (!p || B <= 0) return 0;
    return carve_vit(p, B, nullptr).bytes;
}

namespace {
// keds_vit_run and keds_vit_run_tokens.  tp (nullable): per-block taps / last-block tokens -- the last block then runs on every row
// (a local copy of the tower parameters with last_cls_only cleared) and the CLS read-out comes from the full stream; out nullable
// (no read-out) only with tp
int vit_run(const keds_vit_params* p, const float* image, int B, float* out, int normalize, void* workspace, size_t workspace_bytes,
            void* stream, const KedsTaps* tp, const char* who) {
    int rc = check_tower(&p->tower, who);
    if (rc) return rc;
    const int w = p->tower.width, S = p->tower.seq, G = S - 1;
    const int g = p->resolution / p->patch;
    KEDS_REQUIRE(p->resolution % p->patch == 0 && g * g == G, "%s: seq must be (res/patch)^2 + 1", who);
    KEDS_REQUIRE(p->kpad % 64 == 0 && p->kpad >= 3 * p->patch * p->patch, "%s: bad kpad", who);
    KEDS_REQUIRE(p->embed_dim % 128 == 0, "%s: embed_dim must be a multiple of 128", who);
    VitWs v = carve_vit(p, B, workspace);
    if (workspace_bytes < v.bytes) {
        keds_set_error("%s: workspace %zu < %zu", who, workspace_bytes, v.bytes);
        return KEDS_E_WORKSPACE;
    }
    keds_tower_params full;
    const keds_tower_params* tw = &p->tower;
    if (tp) {
        full = p->tower;
        full.last_cls_only = 0;
        tw = &full;
    }
    hipStream_t st = (hipStream_t)stream;
    void* col = v.tower;
    if (p->tower.f32) {
        // the fp32-accurate flow (f32path.hip): every weight pointer of the structs is an fp32 array
        if ((rc = keds_im2col_f32(image, (float*)col, B, p->resolution, p->patch, p->kpad, stream))) return rc;
        if ((rc = keds_gemm_f32((const float*)col, p->kpad, (const float*)p->conv_w, nullptr, v.x, w, B * G, w, p->kpad,
                                KEDS_F32_EPI_PATCH /* patch rows + positional embedding */, p->pos_emb, G, stream)))
            return rc;
    } else {
        const bool h = p->tower.f16;              // (conv_w / proj_t fp16 too)
        if ((rc = keds_im2col_ex(image, col, h ? 1 : 0, B, p->resolution, p->patch, p->kpad, stream))) return rc;
        if ((rc = keds_gemm_bt(col, p->conv_w, nullptr, v.x, B * G, w, p->kpad, h ? KEDS_EPI_PATCH_F32_H : KEDS_EPI_PATCH_F32, p->pos_emb, G,
                               stream)))
            return rc;
    }
    if ((rc = keds_cls_rows_impl(v.x, p->class_emb, p->pos_emb, B, S, w, st))) return rc;
    // ln_pre in place (each wave holds its whole row in registers before it stores)
    if ((rc = keds_layernorm_impl(v.x, w, nullptr, 1, p->ln_pre_g, p->ln_pre_b, v.x, 1, B * S, w, st))) return rc;
    if ((rc = run_tower(tw, v.x, B, v.tower, st, nullptr, nullptr, tp))) return rc;
    if (!out) return KEDS_OK;
    return run_readout(p->tower, v.x, S, nullptr, p->ln_post_g, p->ln_post_b, p->proj_t, out, B, p->embed_dim, normalize, v.ro, stream);
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
namespace {
struct TextWs {
    float* x;
    char* tower;
    char* ro;
    size_t bytes;
};
TextWs carve_text_cols(const keds_text_params* p, int B, int S, void* ws) {        // the layout for S columns per sequence
    TextWs v;
    char* base = (char*)ws;
    const int w = p->tower.width;
    const size_t Mp = pad_rows((size_t)B * S);
    const size_t xb = keds_align_up(Mp * w * sizeof(float), 256);
    keds_tower_params tp = p->tower;
    tp.seq = S;
    const size_t tb = keds_tower_workspace_bytes_ex(&tp, B);
    const size_t rb = keds_align_up(readout_bytes(p->tower, B), 256);
    v.x = (float*)base;
    v.tower = base ? base + xb : nullptr;
    v.ro = base ? base + xb + tb : nullptr;
    v.bytes = xb + tb + rb;
    return v;
}
TextWs carve_text(const keds_text_params* p, int B, void* ws) { return carve_text_cols(p, B, p->tower.seq, ws); }

// the prologue the text entries share: the tower's shape (and the projection's), then the workspace for all L columns
int text_check(const keds_text_params* p, bool projects, const char* who) {
    int rc = check_tower(&p->tower, who);
    if (rc) return rc;
    KEDS_REQUIRE(!projects || p->embed_dim % 128 == 0, "%s: embed_dim must be a multiple of 128", who);
    return KEDS_OK;
}
int text_workspace(const keds_text_params* p, int B, size_t workspace_bytes, const char* who) {
    const size_t need = carve_text(p, B, nullptr).bytes;
    if (workspace_bytes < need) {
        keds_set_error("%s: workspace %zu < %zu", who, workspace_bytes, need);
        return KEDS_E_WORKSPACE;
    }
    return KEDS_OK;
}
// the tower on `cols` columns per sequence (never larger than the full layout text_workspace covers), then ln_final of the read-out
// rows + projection.  last_rows: the read-out-row tail (the read-out then takes row b of the compact x); front: run_tower
template <typename Front>
int text_tower_readout(const keds_text_params* p, int cols, const int32_t* readout_row, const int32_t* last_rows, const PackedRows* pk,
                       int B, float* out, int normalize, void* workspace, void* stream, Front&& front) {
    keds_tower_params tp = p->tower;              // the tower on the columns that are computed
    tp.seq = cols;
    const TextWs v = carve_text_cols(p, B, cols, workspace);
    int rc = run_tower(&tp, v.x, B, v.tower, (hipStream_t)stream, last_rows, pk, nullptr, front);
    if (rc) return rc;
    return run_readout(tp, v.x, last_rows ? 1 : cols, last_rows ? nullptr : readout_row, p->ln_final_g, p->ln_final_b, p->proj_t, out, B,
                       p->embed_dim, normalize, v.ro, stream);
}
}  // namespace

extern "C" size_t keds_text_workspace_bytes(const keds_text_params* p, int B) {
    if (!p || B <= 0) return 0;
    return carve_text(p, B, nullptr).bytes;
}

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
extern "C" int keds_text_run_ex(const keds_text_params* p, const int32_t* tokens, const int32_t* readout_row,
                                const float* img_tokens, int n_tok, int insert_col, int B, int seq_used, float* out,
                                int normalize, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "keds_text_run";
    KEDS_REQUIRE(p && tokens && readout_row && out && workspace && B > 0, "%s: bad argument", who);
    int rc = text_check(p, true, who);
    if (rc) return rc;
    KEDS_REQUIRE(seq_used >= 0 && seq_used <= p->tower.seq, "%s: seq_used %d outside [0, %d]", who, seq_used, p->tower.seq);
    if ((rc = text_workspace(p, B, workspace_bytes, who))) return rc;
    const int w = p->tower.width, L = p->tower.seq;
    const int mode = keds_text_trim_mode();
    const bool cut = mode == 1 || mode == 2, trim = mode == 1 || mode == 3;
    int Lx = L;
    // (no rounding of the cut to whole row tiles: measured at B = 128 -- tools/text_shapes.py, profiles/r05_text_shapes.txt --
    // the four GEMMs of a block take 161 us at 43 columns, 170 at 44, 172-174 at 46-48: at these sizes the 128 x 128 kernel's
    // rounds of 512 workgroups decide, and fewer rows are never slower)
    if (cut && seq_used > 0 && seq_used < L && p->tower.causal) Lx = seq_used;
    return text_tower_readout(p, Lx, readout_row, trim ? readout_row : nullptr, nullptr, B, out, normalize, workspace, stream, [&] {
        return keds_embed_tokens_impl(tokens, p->token_emb, p->pos_emb, img_tokens, n_tok, insert_col, (float*)workspace, B, L, Lx, w, stream);
    });
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
    const int w = p->tower.width, L = p->tower.seq;
    KEDS_REQUIRE(p->tower.causal && !p->tower.fp8, "%s: a causal bf16 / fp32 / fp32x3 tower (the MXFP8 tower keeps the rectangular layout)", who);
    KEDS_REQUIRE(keds_text_trim_mode() == 1, "%s: the A/B flows of keds_text_trim_enable / KEDS_TEXT_TRIM=0 go through keds_text_run_ex", who);
    KEDS_REQUIRE(seq_max >= 1 && seq_max <= L && rows_total >= B && (long long)rows_total <= (long long)B * seq_max,
                 "%s: rows_total %d / seq_max %d do not fit B = %d sequences of <= %d columns", who, rows_total, seq_max, B, L);
    if ((rc = text_workspace(p, B, workspace_bytes, who))) return rc;
    // the tower runs WHOLE 256-row tiles: the rows between rows_total and the next multiple of 256 are zero rows that belong to no
    // sample (no attention reads them, nothing gathers them; the pass clears them in front of the embedding).  A ragged last tile
    // would send every GEMM of every block through the remainder-row launches and the stricter fill rule of the 256 x 256 kernels
    // (gemm_plan.h, gemm_big_tiles_fill).
    int rows_run = (rows_total + 255) / 256 * 256;
    if ((size_t)rows_run > pad_rows((size_t)B * seq_max)) rows_run = rows_total;
    const PackedRows pk{seq_off, rows_run, rows_total};
    return text_tower_readout(p, seq_max, nullptr, readout_global, &pk, B, out, normalize, workspace, stream, [&] {
        return keds_embed_tokens_impl(tokens, p->token_emb, p->pos_emb, img_tokens, n_tok, insert_col, (float*)workspace, B, L, seq_max, w, stream,
                                      seq_off);
    });
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
    const TextWs v = carve_text(p, B, workspace);
    const int w = p->tower.width, L = p->tower.seq;
    hipStream_t st = (hipStream_t)stream;
    keds_tower_params tp = p->tower;
    tp.last_cls_only = 0;
    if ((rc = keds_embed_tokens_impl(tokens, p->token_emb, p->pos_emb, nullptr, 0, 0, v.x, B, L, L, w, stream))) return rc;
    if ((rc = run_tower(&tp, v.x, B, v.tower, st))) return rc;
    return keds_layernorm_impl(v.x, w, nullptr, 1, p->ln_final_g, p->ln_final_b, out, out_type, B * L, w, st);
}

extern "C" int keds_text_run(const keds_text_params* p, const int32_t* tokens, const int32_t* readout_row,
                                 const float* img_tokens, int n_tok, int insert_col, int B, float* out, int normalize,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    return keds_text_run_ex(p, tokens, readout_row, img_tokens, n_tok, insert_col, B, 0, out, normalize, workspace,
                            workspace_bytes, stream);
}
