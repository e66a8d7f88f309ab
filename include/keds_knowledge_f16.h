/*
 * keds_knowledge_f16.h -- extension header of libkeds_hip.so: the knowledge stream on the fp16 matrix instruction.
 *
 * set_precision("fp16") is the reference's --precision fp16, and the reference converts the knowledge modules with CLIP
 * (convert_weights on img2text, retrieval_fuse and text_condition: src/eval_retrieval.py:122-126,149-153,
 * src/model/model.py:927-948).  The entries below are the bf16 stream of keds_hip.h section 4 with the element type changed:
 * every GEMM operand and every 16-bit intermediate is fp16 (v_mfma_f32_16x16x32_f16), accumulation, softmax statistics and
 * biases stay fp32, inputs and outputs are fp32.  The same launches in the same order, in the fused and in the per-layer weight
 * form; one query over 1 <= K <= 32 neighbours.  EVERY weight pointer of the params is an fp16 array: the fp32 masters rounded
 * to nearest even (keds_cast_f16), which is what convert_weights stores.
 *
 * An extension header like keds_select.h: it adds entry points to the same library and the same KEDS_ABI_VERSION without touching
 * keds_hip.h, is written in the C subset of keds_hip.h, includes only "keds_hip.h", is parsed by the same parser
 * (keds_amd/_abi.py, KNOWLEDGE_F16_HEADERS) into a table of its own and locked by tests/golden/abi_knowledge_f16_v1.json.
 * Whoever next moves KEDS_ABI_VERSION folds it into keds_hip.h.  The conventions of keds_hip.h hold: device pointers,
 * caller-owned buffers, stream-ordered, no allocation, KEDS_OK or a negative KEDS_E_* with keds_last_error().
 *
 * range_flag (nullable): a device int32 the caller zeroed.  It is set non-zero when any fp16 value the call stores -- a packed
 * or cast input row, a GEMM output -- lies beyond +-65504 or is not finite; the value stored is then inf or NaN, and the caller
 * re-runs on another precision.  (The attention core stores a convex combination of fp16 values and needs no check.)  Inside a
 * call that takes range_flag the flag stands in for the calling thread's tower guard (keds_numerics_guard_set), whose device flag
 * is neither read nor written and which is the thread's guard again when the call returns.  The entries WITHOUT a range_flag
 * argument -- the GEMM ids and keds_knowledge_pack_rows_h -- raise the thread's guard, as every fp16-storing kernel of
 * keds_hip.h does.
 */
#ifndef KEDS_KNOWLEDGE_F16_H
#define KEDS_KNOWLEDGE_F16_H

#include "keds_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* GEMM epilogues of keds_gemm_bt* with fp16 A and W, like ids 16-22.  All three carry the fp16 range guard.  They run on the
 * 128 x 128 kernel forms only (split-K included), whatever the shape; ids 23-31 stay refused. */
#define KEDS_EPI_BIAS_F16_H 32          /* out fp16 = acc + bias                  (the store KEDS_EPI_LN_BIAS_F16_H ends in) */
#define KEDS_EPI_BIAS_RELU_F16_H 33     /* out fp16 = relu(acc + bias)            (IM2TEXT, model.py:112-116) */
#define KEDS_EPI_BIAS_F16_H_HEADF32 34  /* id 32, and rows m < aux_i also as fp32 to ((float*)aux)[m*3N + n]: the fp16 twin of
                                           KEDS_EPI_BIAS_BF16_HEADF32 */

/* The stream's kernels one at a time (keds_cross_attn_core / keds_knowledge_pack_rows with fp16 rows; the same limits: K in
 * [1, 32], kv_ld >= 64 heads, dim % 8 == 0; KEDS_E_ARG before any launch). */
int keds_cross_attn_core_h(const void* Q, const void* Kp, const void* Vp, void* out, int B, int K, int heads, int kv_ld, void* stream);
int keds_knowledge_pack_rows_h(const float* q, const float* nbr_img, const float* nbr_txt, void* rows, int B, int K, int dim,
                               void* stream);

/* keds_crossformer_fuse on fp16 weights into fp16 arrays: wkv is a copy, wqn[l] = Wq_l . Wo_{l-1} is the fp32 sum of the fp16
 * weights rounded once to fp16.  The buffer size is keds_crossformer_fused_bytes(p). */
int keds_crossformer_fuse_f16(const keds_crossformer_params* p, void* buffer, size_t buffer_bytes, keds_crossformer_fused* out,
                              void* stream);

/* keds_im2text_forward / keds_crossformer_forward in fp16; workspaces of keds_im2text_workspace_bytes /
 * keds_crossformer_workspace_bytes (the element size is the same).  x, q, k, v 16-byte aligned. */
int keds_im2text_forward_f16(const keds_im2text_params* p, const float* x, int rows, float* out, void* workspace,
                             size_t workspace_bytes, int32_t* range_flag, void* stream);
int keds_crossformer_forward_f16(const keds_crossformer_params* p, const float* q, const float* k, const float* v, int B, int K,
                                 float* out, void* workspace, size_t workspace_bytes, int32_t* range_flag, void* stream);

/* keds_knowledge_run in fp16: tokens_out [B,3,dim] fp32 = [fuse(m, I, I), cond(m, T, T), m].  Argument refusals are KEDS_E_ARG
 * before any launch; a workspace below keds_knowledge_f16_workspace_bytes is KEDS_E_WORKSPACE with nothing written. */
size_t keds_knowledge_f16_workspace_bytes(const keds_knowledge_params* p, int B, int K);
int keds_knowledge_run_f16(const keds_knowledge_params* p, const float* q, const float* nbr_img, const float* nbr_txt, int B, int K,
                           float* tokens_out, void* workspace, size_t workspace_bytes, int32_t* range_flag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KEDS_KNOWLEDGE_F16_H */
