// Which launch a keds_cross_attn_seq call gets (and through it keds_crossformer_forward_seq): the one place that decides.  Host C++
// without a HIP header, a device call or a getenv, exactly as attention_plan.h is; cross_seq.hip launches what cross_seq_plan()
// returns, keds_cross_seq_plan_query (keds_hip.h) answers from it without a GPU, and tests/test_host_cross_seq_plan.py holds it
// against a Python model and against the form table of docs/kernels.md.
#pragma once
#include "attention_plan.h"      // DH, AttnCfg: cross_attn_seq_kernel keeps attention_kernel's LDS image of K and V^T

namespace {

// Queries one workgroup takes.  A workgroup stages all of its (sample, head)'s K and V (256 B per key) and then walks 16-query tiles,
// four waves side by side, so the staging is paid once per workgroup.  Up to 288 queries (18 tiles: what the self-attention kernel
// runs per workgroup at S <= 288, and every Lq the reference's own calls have -- 1 query, or the 257 image tokens) one workgroup
// takes them all.  Beyond that the rows of one (sample, head) are cut into chunks of 256 queries (16 tiles = two 32-query steps per
// wave, balanced), each its own workgroup that stages K / V again: restaging costs at most 72 KB of L2 reads per 256 queries, against
// 256 x 288 scores of work, and a launch with few (sample, head) pairs and many queries still fills the machine.  Decided from the
// code, not measured.
constexpr int CROSS_SEQ_ONE_WG_MAX = 288;
constexpr int CROSS_SEQ_CHUNK = 256;

struct CrossSeqPlan {                   // (an aggregate: the plan and the launch site of cross_seq.hip fill it in this order)
    int form = KEDS_CROSS_SEQ_FORM_NONE;
    int nkt = 0;                        // 16-key tiles the kernel holds in LDS: 2, 6 or 18
    int nfull = 0;                      // key tiles [0, nfull) are known to lie below Lk and are not masked: 0 or 16
    int q_per_wg = 0;                   // query rows of one workgroup (the last chunk of a (sample, head) may hold fewer)
    int grid = 0, block = 0, lds = 0;
    int chunks = 0;                     // workgroups per (sample, head)
    // the layout of keds_cross_seq_plan_query / keds_cross_seq_last_launch
    void info(int out[8]) const {
        const int v[8] = {form, nkt, nfull, q_per_wg, grid, block, lds, chunks};
        for (int i = 0; i < 8; ++i) out[i] = v[i];
    }
};

// false: a grid of B * heads * chunks workgroups does not fit an int (the entries refuse such a call)
inline bool cross_seq_grid_fits(int B, int Lq, int heads) {
    const long long chunks = Lq <= CROSS_SEQ_ONE_WG_MAX ? 1 : ((long long)Lq + CROSS_SEQ_CHUNK - 1) / CROSS_SEQ_CHUNK;
    return (long long)B * heads * chunks <= 0x7FFFFFFFLL;
}

inline CrossSeqPlan cross_seq_plan(int B, int Lq, int Lk, int heads) {
    const int nkt = Lk <= 32 ? 2 : Lk <= 96 ? 6 : 18;
    const int lds = nkt == 2 ? AttnCfg<2>::LDS : nkt == 6 ? AttnCfg<6>::LDS : AttnCfg<18>::LDS;
    const int nfull = Lk >= 256 ? 16 : 0;      // as attention_plan: below 256 keys every tile is masked (the mask is cheap there)
    const bool one = Lq <= CROSS_SEQ_ONE_WG_MAX;
    const int chunks = one ? 1 : (Lq + CROSS_SEQ_CHUNK - 1) / CROSS_SEQ_CHUNK;
    const int q_per_wg = one ? Lq : CROSS_SEQ_CHUNK;
    return CrossSeqPlan{KEDS_CROSS_SEQ_FORM_TILE, nkt, nfull, q_per_wg, B * heads * chunks, 256, lds, chunks};
}

}  // namespace
