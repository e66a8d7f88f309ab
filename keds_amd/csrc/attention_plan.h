// Which kernel form a 16-bit attention call gets (keds_attention, _ex, _mx, _h, _packed, _packed_h and the towers): the one place
// that decides.  Host C++ without a HIP header, a device call or a getenv, exactly as gemm_plan.h is; attention.hip launches what
// attention_plan() returns, keds_attention_plan_query (keds_hip.h) answers from it without a GPU, and
// tests/test_host_attention_plan.py holds it against a Python model and against the form table of docs/kernels.md.
#pragma once
#include "../../include/keds_hip.h"

namespace {

// ---- the kernels' LDS layouts (what the plan's `lds` is made of; the kernels of attention.hip index with the same constants) ------
constexpr int DH = 64;

template <int NKT>
struct AttnCfg {
    static constexpr int KEYS = NKT * 16;
    static constexpr int K_BYTES = KEYS * DH * 2;          // [key][64] bf16, 128-byte rows, swizzled
    static constexpr int VT_ROW = KEYS * 2 + 16;           // bytes per dh row of V^T (+16: odd chunk stride)
    static constexpr int VT_BYTES = DH * VT_ROW;
    static constexpr int LDS = K_BYTES + VT_BYTES;
    static_assert(NKT % 2 == 0, "PV consumes key tiles in pairs");
};

// attention_tail1_kernel, behind AttnCfg<16>::LDS
constexpr int TAIL_LDS = 256 + 2 * 1056;      // last key's K and V rows | scores [257+] | probabilities [257+]

// attention_s257_kernel
namespace s257 {
constexpr int K_OFF = 0, V_OFF = 32768, TAIL_OFF = 65536;    // tail: row 256's q | k | v (128 B each)
constexpr int SC_OFF = TAIL_OFF + 384;                        // last query: f32 scores [264]
constexpr int PART_OFF = SC_OFF + 264 * 4;                    // last query: per wave {max, sum, -, ..., partial output [64]}: 72 floats
constexpr int CNT_OFF = PART_OFF + 8 * 72 * 4;                // last query: arrival counter
constexpr int LDS = CNT_OFF + 16 + 256;                       // 69,552 B -> two workgroups per CU (the last 256 B are unused)
}  // namespace s257

// ---- switches ------------------------------------------------------------------------------------------------------------
// The defaults are the product's; keds_attention_debug (tests, A/B tools) changes them (attention.hip keeps the instance).
struct AttnSwitches {
    bool tail = true;       // bit 4 clears it: S = 257 through the generic (padded) kernel
    bool s257 = true;       // bit 5 clears it: S = 257 through the 4-wave tail kernel
};
// the argument of keds_attention_debug; bits 0-3 and 6 are refused before this is called
inline AttnSwitches attn_switches_decode(int bits) { return AttnSwitches{!((bits >> 4) & 1), !((bits >> 5) & 1)}; }

// ---- the plan ------------------------------------------------------------------------------------------------------------
struct AttnPlan {                       // (an aggregate: the plan and the launch sites of attention.hip fill it in this order)
    int form = KEDS_ATTN_FORM_NONE;     // KEDS_ATTN_FORM_*
    int nkt = 0;                        // 16-key tiles the kernel holds: 2, 6, 18; 16 (+ the rank-1 last key) for the two S = 257 forms
    int nfull = 0;                      // key tiles [0, nfull) are known to lie below S and are not masked: 0 or 16
    bool causal = false, f16 = false, q8 = false, packed = false;
    bool takes_stop_event = false;      // the launch records the caller's event as its stop event (the fork behind the attention, towers.hip)
    int grid = 0, block = 0, lds = 0;
    int q_limit = 0;                    // the effective one: query rows computed and stored per sample
    // the layout of keds_attention_last_launch
    void info(int out[8]) const {
        const int flags = (causal ? KEDS_ATTN_FLAG_CAUSAL : 0) | (f16 ? KEDS_ATTN_FLAG_F16 : 0) | (q8 ? KEDS_ATTN_FLAG_Q8 : 0) |
                          (packed ? KEDS_ATTN_FLAG_PACKED : 0) | (takes_stop_event ? KEDS_ATTN_FLAG_STOP_EVENT : 0);
        const int v[8] = {form, nkt, nfull, flags, grid, block, lds, q_limit};
        for (int i = 0; i < 8; ++i) out[i] = v[i];
    }
};

// S: the sequence length, or s_max of a packed call.  q8: the caller passes MXFP8 output rows (keds_attention_mx).
inline AttnPlan attention_plan(int B, int S, int heads, bool causal, int q_limit, bool f16, bool q8, bool packed, const AttnSwitches& sw) {
    // intended: only keds_attention_mx has MXFP8 output rows.  The fp16 operating point excludes the fp8 tower and the packed rows
    // are the text tower's, so neither entry has the arguments and their launches pass null
    q8 = q8 && !f16 && !packed;
    // intended: q_limit <= 0 or > S means every row; a packed call has no q_limit (every sample's own length, bounded by s_max)
    const int ql = packed || q_limit <= 0 || q_limit > S ? S : q_limit;
    const int grid = B * heads;         // one workgroup per (sample, head) in every form
    // The S = 257 kernels are the ViT's: no mask, and sample b at rows [257 b, 257 b + 257).  Intended, not a quirk: a causal call
    // needs the mask and a packed call's rows start at seq_off[b], so neither ever takes them, whatever s_max is.
    const bool vit257 = !causal && !packed && S == 257;
    // (its Q8 instantiation when q8.  Only this form takes a stop event -- merely preserved: the others could; only the ViT tower's
    // launch is forked behind)
    if (vit257 && sw.tail && sw.s257) return AttnPlan{KEDS_ATTN_FORM_S257, 16, 16, false, f16, q8, false, true, grid, 512, s257::LDS, ql};
    // merely preserved: the tail kernel has no MXFP8 store path, so with MXFP8 rows hook 32 (tail && !s257) lands on the generic
    // kernel like hook 16 does -- nobody chose that, it is what the ladder's `!q8` left over
    if (vit257 && sw.tail && !q8) return AttnPlan{KEDS_ATTN_FORM_TAIL1, 16, 16, false, f16, false, false, false, grid, 256, AttnCfg<16>::LDS + TAIL_LDS, ql};
    const int nkt = S <= 32 ? 2 : S <= 96 ? 6 : 18;
    const int lds = nkt == 2 ? AttnCfg<2>::LDS : nkt == 6 ? AttnCfg<6>::LDS : AttnCfg<18>::LDS;
    // Unmasked leading tiles from S >= 256 (ViT-L/14).  Intended: a causal row masks inside every tile, and s_max >= 256 says
    // nothing about a packed sample's own length (unmasked tiles would weigh its zero pad keys), so both stay at 0.
    const int nfull = !causal && !packed && S >= 256 ? 16 : 0;
    return AttnPlan{KEDS_ATTN_FORM_GENERIC, nkt, nfull, causal, f16, q8, packed, false, grid, 256, lds, ql};
}

}  // namespace
