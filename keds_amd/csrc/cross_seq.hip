// Multi-query cross-attention core (the CrossFormer on sequences that runs on it: keds_crossformer_forward_seq, knowledge.hip):
//   out[b, i, h] = softmax(Q[b, i, h] . K[b, :, h]^T / 8) . V[b, :, h]        (no mask, dim_head = 64, bf16 operands)
// with Lq queries and Lk <= 288 keys per sample, Q / K / V / out in four buffers with their own row counts and strides.
// Reference: CrossAttention.forward (src/model/model.py:56-79), written for any number of queries and keys, as Transformer.forward
// (model.py:343-371) and the late-fusion call of eval_utils.py:249 (one query over the 77 text tokens) use it.
//
// The arithmetic and the LDS image are attention_kernel's (attention.hip), as one piece of code: attn_tile.h holds the K / V^T staging
// (attn_stage_kv) and the tile routine (attn_tiles), and this kernel instantiates them for bf16 with the causal, tail and MXFP8
// branches switched off at compile time (attn_tiles<bf16_t, NKT, false, NFULL, NQ, false, false>): all of a (sample, head)'s K rows
// (swizzled 128-byte rows) and V^T (permuted key order) resident in LDS, scores computed swapped, S^T = K . Q^T on
// v_mfma_f32_16x16x32_bf16, so a lane holds one query column and four keys per 16-key tile: row maximum and sum are in-lane plus two
// shuffles, exp2 with the folded 1 / sqrt(64) . log2 e, the probabilities rounded to bf16 in registers are the B operand of
// O^T = V^T . P^T, and the sum is taken over the unrounded probabilities.
// What differs from the self-attention kernel: a sample's query rows start at b Lq and its key rows at b Lk (two offsets, three
// strides, all products in size_t); only columns [64 h, 64 h + 64) of the rows the call owns are ever read (K and V may be column
// ranges of one wide buffer whose other columns hold anything); the query rows of a partly filled last tile are clamped on load and
// never stored; pad keys >= Lk are zero in LDS (K and V^T: a NaN there would survive a zero probability) and -inf before the row
// maximum.  Which template arguments, grid and LDS a call gets is decided in cross_seq_plan.h and nowhere else.
#include "keds_common.h"
#include "cross_seq_plan.h"      // DH, AttnCfg (attention_plan.h) and cross_seq_plan()
#include "attn_tile.h"           // attn_stage_kv, attn_tiles

namespace {

// One workgroup per (sample, head, chunk of q_per_wg queries); chunks = workgroups per (sample, head), the chunk fastest.
// NFULL: key tiles [0, NFULL) are known at compile time to lie entirely below Lk and need no mask.
template <int NKT, int NFULL>
__global__ __launch_bounds__(256, 2) void cross_attn_seq_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ Kp,
                                                                const bf16_t* __restrict__ Vp, bf16_t* __restrict__ out, int Lq,
                                                                int Lk, int heads, int q_ld, int kv_ld, int o_ld, int q_per_wg,
                                                                int chunks) {
    using C = AttnCfg<NKT>;
    constexpr bool NQ2 = NKT == 18;     // two query tiles per step share every K / V^T fragment read (attention_kernel's rule)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* k_lds = smem;
    char* vt_lds = smem + C::K_BYTES;
    const int bh = blockIdx.x / chunks, chunk = blockIdx.x - bh * chunks;
    const int b = bh / heads, h = bh - b * heads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const bf16_t* kbase = Kp + (size_t)b * Lk * (size_t)kv_ld + h * DH;
    const bf16_t* vbase = Vp + (size_t)b * Lk * (size_t)kv_ld + h * DH;

    attn_stage_kv<bf16_t, NKT, false>(kbase, vbase, kv_ld, Lk, k_lds, vt_lds, tid);     // keys >= Lk are zero
    __syncthreads();

    // ---- this workgroup's queries: rows [q0, q_end) of the sample, in 16-query tiles dealt over the four waves
    const int q0 = chunk * q_per_wg;
    const int q_end = q0 + q_per_wg < Lq ? q0 + q_per_wg : Lq;
    const int nqt = (q_end - q0 + 15) >> 4;
    const AttnCtx<bf16_t> cx{Q + (size_t)b * Lq * (size_t)q_ld + h * DH, out + (size_t)b * Lq * (size_t)o_ld + h * DH, k_lds, vt_lds,
                             (size_t)q_ld, (size_t)o_ld, Lq, Lk, q_end, g, c};
    if constexpr (NQ2) {
        const int npair = nqt >> 1;
        for (int qp = wave; qp < npair; qp += 4) attn_tiles<bf16_t, NKT, false, NFULL, 2, false, false>(cx, q0 + 32 * qp);
        if ((nqt & 1) && wave == ((blockIdx.x + npair) & 3)) attn_tiles<bf16_t, NKT, false, NFULL, 1, false, false>(cx, q0 + 16 * (nqt - 1));
    } else {
        for (int qt = wave; qt < nqt; qt += 4) attn_tiles<bf16_t, NKT, false, NFULL, 1, false, false>(cx, q0 + 16 * qt);
    }
}

// ---- host: the launch is planned by cross_seq_plan() (cross_seq_plan.h); launch_plan() runs the plan -----------------------------

// What the last keds_cross_attn_seq call of this thread launched (keds_cross_seq_last_launch): written at the launch site with the
// literal template arguments of the kernel launched there, and compared with the plan afterwards
thread_local CrossSeqPlan tl_seq_rec = {};

struct SeqArgs {
    const bf16_t *Q, *Kp, *Vp;
    bf16_t* out;
    int B, Lq, Lk, heads, q_ld, kv_ld, o_ld;
    hipStream_t stream;
};

template <int NKT, int NFULL>
int launch_seq(const SeqArgs& a, const CrossSeqPlan& p) {
    const auto kernel = cross_attn_seq_kernel<NKT, NFULL>;
    const CrossSeqPlan rec{KEDS_CROSS_SEQ_FORM_TILE, NKT, NFULL, p.q_per_wg, a.B * a.heads * p.chunks, 256, AttnCfg<NKT>::LDS, p.chunks};
    if (int rc = keds_func_lds_once((const void*)kernel, rec.lds, "cross_attn_seq_kernel")) return rc;
    KedsProfScope prof(KEDS_PROF_ATTN, a.stream);
    tl_seq_rec = rec;
    kernel<<<rec.grid, rec.block, rec.lds, a.stream>>>(a.Q, a.Kp, a.Vp, a.out, a.Lq, a.Lk, a.heads, a.q_ld, a.kv_ld, a.o_ld, rec.q_per_wg,
                                                     rec.chunks);
    return keds_check_launch("cross_attn_seq_kernel");
}

// (nkt, nfull) -> the template instantiation: the only place that names them
int launch_plan(const SeqArgs& a, const CrossSeqPlan& p) {
    if (p.form == KEDS_CROSS_SEQ_FORM_TILE && p.nkt == 2 && !p.nfull) return launch_seq<2, 0>(a, p);
    if (p.form == KEDS_CROSS_SEQ_FORM_TILE && p.nkt == 6 && !p.nfull) return launch_seq<6, 0>(a, p);
    if (p.form == KEDS_CROSS_SEQ_FORM_TILE && p.nkt == 18 && p.nfull == 16) return launch_seq<18, 16>(a, p);
    if (p.form == KEDS_CROSS_SEQ_FORM_TILE && p.nkt == 18 && !p.nfull) return launch_seq<18, 0>(a, p);
    keds_set_error("keds_cross_attn_seq: no kernel of form %d with %d key tiles, %d unmasked", p.form, p.nkt, p.nfull);
    return KEDS_E_LAUNCH;
}

int cross_seq(const SeqArgs& a) {
    const CrossSeqPlan p = cross_seq_plan(a.B, a.Lq, a.Lk, a.heads);
    tl_seq_rec = CrossSeqPlan{};
    if (int rc = launch_plan(a, p)) return rc;
    // keds_cross_seq_last_launch reports what the launch site recorded, not the plan: the two must agree
    int want[8], got[8];
    p.info(want);
    tl_seq_rec.info(got);
    return keds_launch_is_planned(want, got, "keds_cross_attn_seq", "B %d, Lq %d, Lk %d, heads %d", a.B, a.Lq, a.Lk, a.heads);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// every argument rule of keds_cross_attn_seq (keds_hip.h), before any launch
int check_seq(const void* Q, const void* Kp, const void* Vp, const void* out, int B, int Lq, int Lk, int heads, int q_ld, int kv_ld, int o_ld) {
    KEDS_REQUIRE(Q && Kp && Vp && out, "keds_cross_attn_seq: null pointer");
    KEDS_REQUIRE(B >= 1 && Lq >= 1 && heads >= 1, "keds_cross_attn_seq: B=%d, Lq=%d, heads=%d must be at least 1", B, Lq, heads);
    KEDS_REQUIRE(Lk >= 1 && Lk <= KEDS_CROSS_SEQ_MAX_KEYS, "keds_cross_attn_seq: Lk=%d must be in [1,%d]", Lk, KEDS_CROSS_SEQ_MAX_KEYS);
    KEDS_REQUIRE(heads <= (1 << 20) && cross_seq_grid_fits(B, Lq, heads), "keds_cross_attn_seq: B=%d x heads=%d x Lq=%d is too large for one launch", B, heads, Lq);
    const int inner = DH * heads;
    KEDS_REQUIRE(q_ld >= inner && kv_ld >= inner && o_ld >= inner, "keds_cross_attn_seq: q_ld=%d, kv_ld=%d, o_ld=%d must be at least 64 heads = %d",
                 q_ld, kv_ld, o_ld, inner);
    KEDS_REQUIRE(q_ld % 8 == 0 && kv_ld % 8 == 0 && o_ld % 8 == 0, "keds_cross_attn_seq: q_ld=%d, kv_ld=%d, o_ld=%d must be multiples of 8", q_ld,
                 kv_ld, o_ld);
    KEDS_REQUIRE(aligned16(Q) && aligned16(Kp) && aligned16(Vp) && aligned16(out), "keds_cross_attn_seq: Q, Kp, Vp and out must be 16-byte aligned");
    return KEDS_OK;
}

}  // namespace

extern "C" int keds_cross_seq_plan_query(int B, int Lq, int Lk, int heads, int* info) {
    KEDS_REQUIRE(info && B >= 1 && Lq >= 1 && heads >= 1 && heads <= (1 << 20) && cross_seq_grid_fits(B, Lq, heads),
                 "keds_cross_seq_plan_query: bad argument (B, Lq, heads >= 1, one launch's grid)");
    KEDS_REQUIRE(Lk >= 1 && Lk <= KEDS_CROSS_SEQ_MAX_KEYS, "keds_cross_seq_plan_query: Lk=%d must be in [1,%d]", Lk, KEDS_CROSS_SEQ_MAX_KEYS);
    cross_seq_plan(B, Lq, Lk, heads).info(info);
    return KEDS_OK;
}

extern "C" int keds_cross_seq_last_launch(int* info) {
    KEDS_REQUIRE(info, "keds_cross_seq_last_launch: null pointer");
    tl_seq_rec.info(info);
    return KEDS_OK;
}

extern "C" int keds_cross_attn_seq(const void* Q, const void* Kp, const void* Vp, void* out, int B, int Lq, int Lk, int heads, int q_ld,
                                   int kv_ld, int o_ld, void* stream) {
    if (int rc = check_seq(Q, Kp, Vp, out, B, Lq, Lk, heads, q_ld, kv_ld, o_ld)) return rc;
    return cross_seq(SeqArgs{(const bf16_t*)Q, (const bf16_t*)Kp, (const bf16_t*)Vp, (bf16_t*)out, B, Lq, Lk, heads, q_ld, kv_ld, o_ld,
                             (hipStream_t)stream});
}
