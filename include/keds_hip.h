/*
 * keds_hip.h -- C ABI of libkeds_hip.so: the MI355X (gfx950) retrieval hot path of KEDs.
 *
 * The reference (suoych/KEDs) has no FFI seam: its seam is the Python object API
 * (SURVEY.md section 8b).  The Python facade in keds_amd/ keeps that API and binds the
 * functions below with ctypes; each entry point names the reference code it replaces
 * (paths relative to the reference checkout).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - the caller owns every buffer (inputs, outputs, workspaces); the library never
 *     allocates, frees or synchronises, so every call is capturable in a hipGraph;
 *   - all launches go to the `stream` argument (a hipStream_t passed as void*);
 *   - return 0 on success, a negative KEDS_E_* code otherwise; keds_last_error()
 *     returns a thread-local message for the last failure;
 *   - bf16 tensors are raw 16-bit patterns (uint16_t), row-major, innermost dim contiguous.
 */
#ifndef KEDS_HIP_H
#define KEDS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KEDS_OK 0
#define KEDS_E_ARG (-1)      /* bad argument / unsupported shape */
#define KEDS_E_LAUNCH (-2)   /* HIP launch or runtime error */
#define KEDS_E_WORKSPACE (-3)/* workspace too small */

#define KEDS_ABI_VERSION 15       /* 15: keds_tower_plan_query (every tower pass is planned by one pure host function and run from its steps, as the
                                     GEMM and attention launches are);
                                     (still 15: keds_cross_attn_seq, keds_cross_seq_plan_query, keds_cross_seq_last_launch,
                                     keds_crossformer_seq_workspace_bytes and keds_crossformer_forward_seq were added; no earlier entry changed)
                                     (still 15: keds_pass_plan_query and keds_text_runs_packed were added; the step record keeps its 24 ints -- [23], always
                                     0 before, is now the read-out LayerNorm's flag -- and keds_tower_plan_query its 18 buffer rows)
                                     14: keds_attention_f32_packed, keds_attention_x3_packed (the fp32 and split-fp16 attention on packed rows, one call at a
                                     time; the tower passes launch through the same helpers);
                                     13: keds_cross_attn_core, keds_cross_core_f32, keds_knowledge_pack_rows, keds_place_token (the knowledge stream's
                                     kernels one at a time; the module paths launch through the same helpers);
                                     12: keds_attention_plan_query, keds_attention_last_launch and keds_gemm_mxfp8_plan_query (every 16-bit attention and
                                     MXFP8 GEMM launch is planned by one pure host function, as the bf16 GEMMs are);
                                     11: keds_merge_stamp_buffer, keds_attention_stamp_buffer and keds_tower_fill_enable left the library; the debug
                                     hooks refuse the timing-only variants they no longer offer (last at 14f64ac);
                                     10: keds_block_source, keds_block_pack_bytes, keds_block_pack (one weight-packing routine for both loaders);
                                     9: the "fp16" operating point -- keds_tower_params.f16, KEDS_EPI_*_F16_H / *_F32_H epilogues, keds_attention_h /
                                     keds_attention_packed_h, keds_im2col_ex, keds_layernorm_ex, keds_cast_f16;
                                     8 (round 6): keds_gemm_x3 takes w_exp, keds_split_f16_weight, keds_block_params.x3_exp, keds_text_run_packed / keds_attention_packed; keds_gemm_duo_enable left the product */

int keds_abi_version(void);
/* compiler flags of this build beyond the Makefile's defaults ("" for the product build; `make EXTRA="-D..."` variants of the
 * A/B scripts record theirs here, and the evidence digest of keds_amd/_lib.py includes it) */
const char* keds_build_flags(void);
const char* keds_last_error(void);

/* ---- numerics guard of the fast tower flow ---------------------------------------------------------------------
 * The default tower flow keeps the residual stream in fp16 and evaluates LayerNorm inside the GEMMs on un-centred rows: accurate while |row mean| /
 * row std stays small (CLIP: a few) and the stream stays inside the fp16 range.  While a device flag is registered for the calling thread, every
 * LayerNorm-consuming GEMM it enqueues sets *flag = 1 at a row of the call (not behind M, not a zero row of a packed text pass) with |mean| / std > 32,
 * and every writer of the fp16 stream (KEDS_EPI_RESID_STATS_F16 / _F16_H in every kernel form, keds_rowstats_cast_ex with out_f16) sets it at a stored
 * value beyond +-65504 or not finite -- or when a 64-column partial sum of squares reaches 65504^2 (the statistics, fixed-point sums of the fp32
 * values, cannot show it).  keds_amd.CLIP then re-runs the pass on the fp32-stream flow.  nullptr unregisters.  The library only ever sets the flag. */
int keds_numerics_guard_set(int32_t* device_flag);

/* ---- profiling of kernel classes with hipEvents on the launch stream -------------
 * bench.py switches this on over its timed region to get the dominant kernel's average
 * launch duration (roofline.achieved).  Classes: see KEDS_PROF_*. */
#define KEDS_PROF_GEMM 0
#define KEDS_PROF_ATTN 1
#define KEDS_PROF_SCAN 2
#define KEDS_PROF_LN 3
#define KEDS_PROF_OTHER 4
#define KEDS_PROF_NCLASS 5
int keds_prof_enable(int on);                 /* 0 off; 1: event pair around every launch; else bit (k+1) = class k */
int keds_prof_reset(void);
int keds_prof_read(int klass, double* total_ms, int64_t* launches);  /* synchronises the events */
/* algorithmic work of the launches that carried event pairs since the last reset: 2*M*N*K flops per GEMM launch
 * (KEDS_PROF_GEMM; a patch-embedding GEMM counts its zero-padded K), scan-image bytes per scan launch (KEDS_PROF_SCAN) */
int keds_prof_read_work(int klass, double* units);

/* =====================================================================================
 * 1. Similarity + top-k  (replaces faiss.IndexFlatL2 + index_cpu_to_all_gpus + .add/.search,
 *    src/eval_retrieval.py:289-298, src/eval_utils.py:169,177; brute-force twin
 *    src/trainer.py:246-257)
 * ===================================================================================== */
#define KEDS_METRIC_L2 0   /* D = ||q - x||^2 ascending (IndexFlatL2) */
#define KEDS_METRIC_IP 1   /* D = q . x descending (trainer.py:246-249) */

#define KEDS_SCAN_STAGE_KEYS 32     /* keys per packed stage */
#define KEDS_SCAN_MAX_QUERIES 128   /* queries per scan launch (one query block) */
#define KEDS_SCAN_LIST 16           /* per-lane exact list depth */
#define KEDS_SCAN_CAND 64           /* candidates re-ranked in fp32 per query for k <= 16 (256 for larger k) */
#define KEDS_SCAN_MAX_K 128         /* largest k of keds_index_search_packed */

/* test / A/B hook of the search, process-wide (0 = product path); every form it selects is exact: bit 4 single-phase scan,
 * bit 5 every query through the exact pass, bit 6 default-policy key stream, bits 7-9 threshold-pass list depth 1 or 4.
 * Bits 0-3 (timing-only scan ablations) and bit 10 (the fused search tail) last existed at 14f64ac: KEDS_E_ARG, state unchanged. */
int keds_scan_debug(int variant);

/* bytes of the packed bf16 scan image for n rows of dimension dim (dim % 128 == 0); the image ends with a 128-byte
 * trailer holding max ||bf16(x)||, max ||x - bf16(x)||, max ||x|| over the rows (the search certificate's bounds) */
size_t keds_index_packed_bytes(int64_t n, int dim);

/* `.add`: build the scan image from fp32 rows [n, dim] (device).  The image is the exact
 * LDS layout the scan kernel streams: per stage of 32 keys, XOR-swizzled bf16 rows followed
 * by 32 fp32 bias terms (-0.5*||x||^2 for L2, 0 for IP; -inf for rows >= n). */
int keds_index_pack(const float* db, int64_t n, int dim, int metric, void* packed, void* stream);   /* n <= 2,048 * 16,384 rows per shard */
/* chunked `.add`: `packed` already holds the image of rows [0, old_n) of `db` (same buffer, sized for n rows); pack rows
 * [old_n, n) only (the stage that old_n falls into is rewritten), keeping the bounds of the earlier rows. */
int keds_index_pack_append(const float* db, int64_t old_n, int64_t n, int dim, int metric, void* packed, void* stream);

/* workspace bytes for keds_index_search_packed(_ex): nq queries against n rows, top-k.  The two-argument form is sized
 * for k <= 16 over at most 4 M rows. */
size_t keds_index_search_workspace_bytes_ex(int nq, int dim, int64_t n, int k);
size_t keds_index_search_workspace_bytes(int nq, int dim);

/* `.search`: exact top-k (k <= KEDS_SCAN_MAX_K) of nq fp32 queries [nq, dim] against the index.
 *   normalize_q != 0 : L2-normalise the queries first (src/eval_utils.py:162)
 *   D [nq,k] fp32, I [nq,k] int64 (row ids offset by id_base, -1 if fewer than k rows)
 *   rows_out (nullable) [nq,k,dim] fp32 : gathered rows db[I]  (src/eval_utils.py:171-172,179-180)
 * Pipeline: bf16 MFMA scan with per-lane exact top-16 lists -> merge to 64 (k > 16: 256) candidates -> exact fp32
 * re-rank from `db` -> top-k -> CERTIFICATE per query: the k-th candidate's exact score minus a rigorous bound on the bf16
 * scan error must beat the best score any non-candidate row can have; queries that fail it (near-duplicate clusters
 * wider than the candidate list) are answered by an exact fp32 pass over all rows (IndexFlatL2 semantics in every case).
 * `db` is the fp32 matrix given to keds_index_pack.  status (nullable, device int32[2]): += {queries certified from the
 * candidates, queries answered by the exact pass}. */
int keds_index_search_packed_ex(const void* packed, const float* db, int64_t n, int dim, int metric,
                      const float* queries, int nq, int normalize_q, int k, int64_t id_base,
                      float* D, int64_t* I, float* rows_out,
                      void* workspace, size_t workspace_bytes, int32_t* status, void* stream);
int keds_index_search_packed(const void* packed, const float* db, int64_t n, int dim, int metric,
                      const float* queries, int nq, int normalize_q, int k, int64_t id_base,
                      float* D, int64_t* I, float* rows_out,
                      void* workspace, size_t workspace_bytes, void* stream);

/* The shape arithmetic of one launch set of keds_index_search_packed_ex (at most 1,024 queries), as pure host code that the
 * search itself launches from: out[KEDS_SEARCH_PLAN_FIELDS] = {two_phase, stagesA (stages of the threshold pass), nqb (query
 * blocks of 128), nwgA, nwgB (scan workgroups per query block of the threshold / candidate pass), depthA (list depth of the
 * threshold pass), ncand, chunk_rows, nchunks (exact pass), total_stages}.  `cus` above 256 counts as 256.  keds_scan_debug bits
 * 4 and 7-9 are honoured.  -1 where the search would be refused (exact-pass budget, a 2 GiB key stream). */
#define KEDS_SEARCH_PLAN_FIELDS 10
int keds_index_search_plan_query(int nq_set, int dim, int64_t n, int k, int cus, int32_t* out);

/* The stages of the search one at a time on caller-owned device buffers: the kernels and launch helpers of
 * keds_index_search_packed_ex (tests/test_gpu_search_kernels_edges.py).  A bad argument returns -1 before any launch.
 *   qprep  : queries [nq, dim] (nq <= 1024) -> qn [nq, dim] fp32 (normalised if asked), qb [ceil(nq/128)*128, dim] bf16 (rows >= nq
 *            zero), qstat [nq][4] = {||qn||^2, ||qn - qb|| rounded up, ||qb|| rounded up, 0}; clears counters[0].
 *   scan   : stages [0, stages) of the image of n rows, nqb query blocks of qb, thr [nqb*128] or NULL, depth 1 / 4 / 16, nwg in
 *            [1, min(stages, 256)] -> pairs [nqb*128][nwg][4*depth] (ord_key(score) << 32 | row), meta [nqb*128][nwg][2] = {entries,
 *            largest last-slot key of the segment's full lists or 0}.  Slots at or behind the count are not written.
 *   merge  : pairs / meta of nq queries (nwg <= 256 segments of `slots` = 4 / 16 / 64) -> cand_idx / cand_val [nq, ncand] (ncand 64 /
 *            256; fillers -1 / -inf), thr_out [nq] (nullable), sbound [nq] (nullable); thr_in [nq] nullable.
 *   rerank : cand_d [nq, ncand] = exact fp32 distance of qn[q] to db[cand_idx] (id < 0: +inf L2 / -inf IP).
 *   certify: top-k by (distance, id) of the candidates -> D, I (+ id_base) [nq, k], and the certificate from qstat, sbound and
 *            the image's trailer: fslot [nq] (-1 certified, else the query's place in fail_ids), dk [nq] of the failed,
 *            counters[0] += failed (counters: int32 [8 + nq], [8 + f] = 0 per failed slot), status[0 / 1] += certified / failed
 *            (nullable).  force_fail != 0 fails every query.
 *   exact  : the exact pass over all n rows in chunks of chunk_rows in [1, 16384] (at most 2,048 chunks) for the counters[0]
 *            queries of fail_ids, pruned by dk: plist uint64 [failed][nchunks][k], pcnt int32 [failed][nchunks]; rows of D / I
 *            of other queries are untouched. */
int keds_search_qprep(const float* queries, int nq, int dim, int normalize, float* qn, void* qb, float* qstat, int32_t* counters,
                      void* stream);
int keds_search_scan(const void* packed, int64_t n, int dim, int stages, const void* qb, int nqb, const float* thr /* nullable */,
                     int depth, int nwg, uint64_t* pairs, uint32_t* meta, void* stream);
int keds_search_merge(const uint64_t* pairs, const uint32_t* meta, int nq, int nwg, int slots, int ncand,
                      const float* thr_in /* nullable */, int32_t* cand_idx, float* cand_val, float* thr_out /* nullable */,
                      float* sbound /* nullable */, void* stream);
int keds_search_rerank(const float* db, int dim, int metric, const float* qn, const int32_t* cand_idx, int nq, int ncand,
                       float* cand_d, void* stream);
int keds_search_certify(const void* packed, int64_t n, int dim, const int32_t* cand_idx, const float* cand_d, int nq, int ncand,
                        int metric, int k, int64_t id_base, const float* qstat, const float* sbound, float* D, int64_t* I,
                        int32_t* counters, int32_t* fail_ids, int32_t* fslot, float* dk, int32_t* status /* nullable */,
                        int force_fail, void* stream);
int keds_search_exact(const float* db, int64_t n, int dim, int metric, const float* qn, int32_t* counters, const int32_t* fail_ids,
                      const float* dk, int chunk_rows, int k, int64_t id_base, uint64_t* plist, int32_t* pcnt, float* D, int64_t* I,
                      void* stream);

/* merge `parts` partial results [parts, nq, k] (each sorted) into the global top-k
 * (multi-GPU: after the all-gather of per-shard results).  Keyed on (D, I). */
int keds_topk_merge_parts(const float* D_parts, const int64_t* I_parts, int parts, int nq, int k,
                          int metric, float* D, int64_t* I, void* stream);

/* Packed exchange of a data-parallel, row-sharded search (replaces the replicated Faiss index of
 * src/eval_retrieval.py:289-298 and the two searches of src/eval_utils.py:169-183): every rank searched ITS shard for
 * the B queries of EVERY rank and holds D_p / I_p [world*B, k] (+ rows_p [world*B, k, dim], the rows of its partial
 * winners, when the caller needs the neighbours themselves).  keds_exchange_pack writes one message per peer,
 *   send[w][b][j][E] int32,  E = 3: distance bits | id low | id high;  with rows E = 4 + dim: those, a pad word, the row
 * (part w at send + w * w_stride words; w_stride >= B*k*E, a multiple of 4 with rows -- several databases share one
 * buffer by interleaving their parts).  After ONE all-to-all (block w to rank w) keds_exchange_merge turns the received
 * recv[w][b][j][E] (part w = what shard w found for MY query b) into this rank's D / I [B, k] keyed on (distance, id) --
 * the order of a single-GPU search of the whole database -- and, with rows != NULL, the winners' rows [B, k, dim].
 * world <= 64, world * k <= 4096, k <= KEDS_SCAN_MAX_K. */
int keds_exchange_pack(const float* D_p, const int64_t* I_p, const float* rows_p /* nullable */, int world, int B, int k,
                       int dim, int64_t w_stride, int32_t* send, void* stream);
int keds_exchange_merge(const int32_t* recv, int world, int B, int k, int dim, int64_t w_stride, int metric,
                        float* D, int64_t* I, float* rows /* nullable */, void* stream);

/* out[i,:] = db[idx[i],:]  (idx < 0 gives zeros) */
int keds_gather_rows(const float* db, int dim, const int64_t* idx, int64_t count, float* out, void* stream);

/* full gallery ranking for the recall metric (src/eval_utils.py:1040-1067):
 * order[q,:] = stable argsort of (1 - ref[q] . gallery[g]) ascending.  Up to 8192 gallery rows sort in LDS; larger
 * galleries (ImageNet domain-conversion targets) sort 8192-row chunks and merge the runs in global memory.
 * The call leaves dist fp32 [nq, ng] (the distances it sorted) in the first nq * ng floats of `workspace`; order[q,:] is the
 * ascending order of the 64-bit keys (orderable(bits of dist[q,g]) << 32 | g), orderable(u) = ~u for a set sign bit and
 * u | 0x80000000 otherwise: -0 before +0, ties by the smaller g, a NaN where its sign bit puts it (beyond +-inf). */
size_t keds_rank_gallery_workspace_bytes(int nq, int ng);
int keds_rank_gallery(const float* ref, int nq, const float* gallery, int ng, int dim,
                      int32_t* order, void* workspace, size_t workspace_bytes, void* stream);

/* recall hits from a ranking with the reference image removed (eval_utils.py:1050-1065):
 * names are integer ids (basename-interned on the host).  rank_out[q] = position of target
 * id in order[q] after removing ref_id[q]; -1 if absent. */
int keds_cirr_target_rank(const int32_t* order, int nq, int ng, const int32_t* gallery_ids,
                          const int32_t* ref_ids, const int32_t* target_ids, int32_t* rank_out,
                          int32_t* counts_out /* nullable [nq,2]: reference matches, target matches */,
                          void* stream);

/* get_metrics_imgnet (src/eval_utils.py:1090-1134): hits_out[q,j] = number of gallery items among the first
 * ks[j] of order[q,:] whose label equals query_labels[q]; total_out[q] = that count over the whole gallery.
 * ks is a HOST array of nk <= 8 cut-offs. */
int keds_label_hits(const int32_t* order, int nq, int ng, const int32_t* gallery_labels,
                    const int32_t* query_labels, const int32_t* ks, int nk, int32_t* hits_out,
                    int32_t* total_out, void* stream);

/* =====================================================================================
 * 2. Encoder primitives (src/model/model.py:291-326).  bf16 GEMM inputs, fp32 accumulate,
 *    fp32 residual stream, fp32 LayerNorm / softmax statistics.
 * ===================================================================================== */
#define KEDS_EPI_BIAS_BF16 0        /* out bf16 = acc + bias */
#define KEDS_EPI_BIAS_QGELU_BF16 1  /* out bf16 = qgelu(acc + bias)          (model.py:300-302,311-315) */
#define KEDS_EPI_BIAS_RELU_BF16 2   /* out bf16 = relu(acc + bias)           (IM2TEXT, model.py:112-116) */
#define KEDS_EPI_BIAS_RESID_F32 3   /* out f32 += acc + bias (in place)      (model.py:324-325) */
#define KEDS_EPI_BIAS_F32 4         /* out f32 = acc + bias */
#define KEDS_EPI_PATCH_F32 5        /* out f32 row (m/G)*(G+1)+1+m%G = acc + aux[1+m%G]  (model.py:394-398) */
/* LayerNorm folded into the neighbouring GEMMs (ln_1 -> in_proj, ln_2 -> c_fc, model.py:305-326): the producer of the
 * residual stream also emits a bf16 copy of it and per-row {sum, sum of squares}; the consumer multiplies the UN-normalised
 * rows with W.diag(gamma) and finishes LayerNorm per output element:
 *     LN(x) W^T + b = rstd (x W'^T - mean colsum(W')) + (b + W beta),   W' = bf16(W diag(gamma))
 * so the 2 x layers LayerNorm passes over the residual stream disappear (keds_fold_layernorm builds W', colsum, b'). */
#define KEDS_EPI_LN_BIAS_BF16 6     /* out bf16 = rstd[m] (acc - mean[m] csum[n]) + bias'[n];  bias = [bias'(N) | csum(N)],
                                       aux = row statistics [M,2] of A's rows (LayerNorm width = K): {sum, sum of squares} as
                                       64-bit fixed point (value * 2^28; integer atomics: order independent, deterministic),
                                       aux2 (nullable) = statistics buffer that is ZEROED for this launch's rows */
#define KEDS_EPI_LN_QGELU_BF16 7    /* same, then QuickGELU */
#define KEDS_EPI_RESID_STATS_F32 8  /* out f32 += acc + bias (in place); aux2 = bf16 copy [M,N] of the new rows;
                                       aux = statistics [M,2] (64-bit fixed point) += {sum, sum sq} of the new rows (zeroed before) */
#define KEDS_EPI_RESID_STATS_F16 9  /* out f16 += acc + bias (in place, fp32 sum rounded once): the residual stream kept in
                                       the reference's own storage type (convert_weights, model.py:531-548), one copy that is
                                       also the next GEMM's operand; aux = statistics as above (of the fp32 sums) or NULL */
#define KEDS_EPI_LN_BIAS_BF16_H 10  /* KEDS_EPI_LN_BIAS_BF16 with fp16 operands: A = the fp16 residual stream, W' fp16 */
#define KEDS_EPI_LN_QGELU_BF16_H 11 /* KEDS_EPI_LN_QGELU_BF16 with fp16 operands */
#define KEDS_EPI_BIAS_BF16_HEADF32 12 /* out bf16 = acc + bias, and rows m < aux_i also as fp32 to ((float*)aux)[m*3N + n]: IM2TEXT's
                                       * last layer writes the bf16 rows the CrossFormers read AND token slot 2 of [B,3,N] */
/* Split-operand GEMMs of the "fp32x3" operating point (round 5): BOTH operands are pairs of fp16 planes, x = hi + lo with
 * hi = fp16(x), lo = fp16(x - hi) (|x| < 65504; 22 significant bits while lo is a normal fp16 number, i.e. |x| >= 2^-3 -- below
 * that an absolute 2^-25), and the product is  hi.hi + hi.lo + lo.hi  on the fp16 MFMA with fp32 accumulation -- three times
 * the matrix work of a bf16 GEMM, ~1/5 of the time of the f32-input MFMA (157 TF), and fp32-grade results (the dropped lo.lo term
 * is 2^-22 relative).  A = planes [2][rows][K] (keds_split_f16_pair: activations are O(1)), W = planes [2][N][K] of W 2^e
 * (keds_split_f16_weight: an exact per-matrix power of two that lifts small weights out of the subnormal range; the epilogue
 * takes it out again); called through keds_gemm_x3. */
#define KEDS_EPI_X3_BIAS_F32 13     /* out f32 = acc + bias */
#define KEDS_EPI_X3_RESID_F32 14    /* out f32 += acc + bias (in place) */
#define KEDS_EPI_X3_QGELU_PAIR 15   /* out = fp16 planes [2][rows][N] of qgelu(acc + bias) (full-precision expf / division): the
                                       next split-operand GEMM's A operand; aux_i = elements between the two planes */
/* The "fp16" operating point (keds_tower_params.f16; the reference's --precision fp16, convert_weights model.py:927-948): BOTH
 * operands fp16 (v_mfma_f32_16x16x32_f16, fp32 accumulate, the bf16 rate), and every 16-bit output fp16.  Epilogues that STORE fp16
 * values (qkv, the MLP hidden layer) raise the numerics-guard flag (keds_numerics_guard_set) on any |v| > 65504 or non-finite v
 * instead of letting inf through; the host then re-runs the pass on another operating point. */
#define KEDS_EPI_LN_BIAS_F16_H 16     /* KEDS_EPI_LN_BIAS_BF16_H with an fp16 output (+ range guard) */
#define KEDS_EPI_LN_QGELU_F16_H 17    /* KEDS_EPI_LN_QGELU_BF16_H with an fp16 output (+ range guard) */
#define KEDS_EPI_RESID_STATS_F16_H 18 /* KEDS_EPI_RESID_STATS_F16 with an fp16 A operand and fp16 W */
#define KEDS_EPI_BIAS_RESID_F32_H 19  /* KEDS_EPI_BIAS_RESID_F32 on fp16 operands */
#define KEDS_EPI_BIAS_QGELU_F16_H 20  /* out fp16 = qgelu(acc + bias) on fp16 operands (+ range guard) */
#define KEDS_EPI_PATCH_F32_H 21       /* KEDS_EPI_PATCH_F32 on fp16 operands */
#define KEDS_EPI_BIAS_F32_H 22        /* KEDS_EPI_BIAS_F32 on fp16 operands (the read-out projections) */

/* out[M,N] = epilogue(A[M,K] . W[N,K]^T + bias[N]).  A, W bf16 row-major (W is the nn.Linear
 * weight as stored).  N % 128 == 0, K % 64 == 0; rows of A / out up to the next multiple of
 * 128 above M must be addressable (workspaces are allocated padded).  `bias` may be NULL.
 * aux: EPI_PATCH: fp32 positional embedding [G+1, N], aux_i = G (patches per image). */
int keds_gemm_bt(const void* A, const void* W, const float* bias, void* out, int M, int N, int K,
                 int epilogue, const float* aux, int aux_i, void* stream);
/* same with row strides (elements) of A and out: rows need not be contiguous (CLS-row-only last layer); A rows
 * past M are never read */
int keds_gemm_bt_ex(const void* A, int64_t lda, const void* W, const float* bias, void* out, int64_t ldc,
                    int M, int N, int K, int epilogue, const float* aux, int aux_i, void* stream);

/* same with the second auxiliary pointer the KEDS_EPI_LN_* / KEDS_EPI_RESID_STATS_F32 epilogues use */
int keds_gemm_bt_ex2(const void* A, int64_t lda, const void* W, const float* bias, void* out, int64_t ldc,
                     int M, int N, int K, int epilogue, const float* aux, int aux_i, void* aux2, void* stream);

/* Fold a LayerNorm (gamma, beta over K) into the nn.Linear that consumes it: W fp32 [N,K], bias fp32 [N] (nullable) ->
 * w_folded bf16 [N,K] = W diag(gamma), bias_csum fp32 [2N] = [bias + W beta | row sums of w_folded (as rounded)]. */
int keds_fold_layernorm(const float* W, const float* bias, const float* gamma, const float* beta, int N, int K,
                        void* w_folded, float* bias_csum, void* stream);
/* out_f16 != 0: w_folded in fp16 (operand of the KEDS_EPI_LN_*_H GEMMs, which read the fp16 residual stream) */
int keds_fold_layernorm_ex(const float* W, const float* bias, const float* gamma, const float* beta, int N, int K,
                           void* w_folded, int out_f16, float* bias_csum, void* stream);

/* Row statistics + bf16 copy of a residual stream (what KEDS_EPI_RESID_STATS_F32 emits, for the first block):
 * x fp32 [rows, dim] dense -> xb bf16 [rows, dim], stats [rows,2] = {sum, sum of squares} as 64-bit fixed point (* 2^28). */
int keds_rowstats_cast(const float* x, void* xb, float* stats, int rows, int dim, void* stream);
int keds_rowstats_cast_ex(const float* x, void* xb, int out_f16, float* stats, int rows, int dim, void* stream);  /* xb fp16 */

/* ---- MXFP8 (BASELINE config 5: fp8 encoders).  OCP e4m3 elements, one e8m0 scale per 32 consecutive K (OCP MX),
 * multiplied by v_mfma_scale_f32_16x16x128_f8f6f4 (block scales applied in hardware, 2x the bf16 MFMA rate).
 * Scales are stored as [K/128][rows_pad] dwords: byte b of dword (t, r) scales elements 128 t + 32 b .. + 31 of row r. */
size_t keds_mxfp8_scale_bytes(int rows_pad, int K);
int keds_mxfp8_debug(int variant);          /* test hook: 16 = every shape on the 8-wave kernel, 0 = product path; any other value
                                               (the timing-only ablations 1-4, last at 14f64ac) is KEDS_E_ARG, state unchanged */
/* x fp32 or bf16 [rows, K] dense -> q fp8 [rows, K], scales as above.  K % 128 == 0. */
int keds_quantize_mxfp8(const void* x, int x_is_bf16, int rows, int K, int rows_pad, void* q, void* scales, void* stream);
/* out bf16 [M,N] = A . W^T + bias with A [M,K], W [N,K] in MXFP8 (m_pad / n_pad: row counts of the scale arrays).
 * M % 256 == 0, N % 256 == 0, K % 128 == 0, K >= 256. */
int keds_gemm_mxfp8(const void* Aq, const void* As, int m_pad, const void* Wq, const void* Ws, int n_pad,
                    const float* bias, void* out, int M, int N, int K, void* stream);
/* the same with the fused epilogues of the fp8 tower (cf. KEDS_EPI_LN_* / KEDS_EPI_RESID_STATS_F32 above):
 *   LN_BIAS_BF16   out bf16 = rstd (acc - mean csum) + bias';  bias = [bias' | csum], aux = row statistics [M,2],
 *                  aux2 (nullable) = statistics buffer cleared for these rows
 *   LN_QGELU_MX    the same, then QuickGELU, emitted as MXFP8 to qout [M,N] / qscale ([N/128][q_pad] dwords)
 *   RESID_STATS_MX out fp32 += acc + bias; MXFP8 copy of the new rows to qout / qscale; aux += {sum, sum sq} per row */
#define KEDS_FP8_EPI_BIAS_BF16 0
#define KEDS_FP8_EPI_LN_BIAS_BF16 1
#define KEDS_FP8_EPI_LN_QGELU_MX 2
#define KEDS_FP8_EPI_RESID_STATS_MX 3
#define KEDS_FP8_EPI_RESID_STATS_MX_H 4   /* the same on an fp16 residual stream: out fp16 += acc + bias */
int keds_gemm_mxfp8_ex(const void* Aq, const void* As, int m_pad, const void* Wq, const void* Ws, int n_pad,
                       const float* bias, void* out, int M, int N, int K, int epilogue, float* aux, float* aux2,
                       void* qout, void* qscale, int q_pad, void* stream);
/* What the last keds_gemm_mxfp8 / keds_gemm_mxfp8_ex call of this thread launched (thread-local, written at the launch sites; all
 * zero after a call that launched nothing): info[4] = {form, grid size, 256 x 256 tiles, persistent (grid < tiles)}. */
#define KEDS_FP8_FORM_PAIR 1    /* gemm_mxfp8_kernel: 8 waves, one tile per workgroup */
#define KEDS_FP8_FORM_QUAD 2    /* gemm_mxfp8_quad_kernel: 4 waves, one tile per workgroup or persistent */
int keds_gemm_mxfp8_last_launch(int* info);
/* The plan of that call on a device of `cus` compute units under keds_mxfp8_debug's value (mxfp8_plan, csrc/gemm_plan.h: the
 * function the call launches from; a launch that differs from it fails with KEDS_E_LAUNCH): info[4] as above.  Touches no device;
 * the shape rules of keds_gemm_mxfp8_ex apply. */
int keds_gemm_mxfp8_plan_query(int epilogue, int M, int N, int K, int cus, int* info);
/* Weight preparation for the fp8 tower: W fp32 [N,K] (times diag(gamma) when a LayerNorm is folded in) -> MXFP8 wq / wscale,
 * bias_csum fp32 [2N] = [bias + W beta | row sums of the dequantised weight].  gamma = beta = NULL: plain quantisation. */
int keds_fold_layernorm_mxfp8(const float* W, const float* bias, const float* gamma, const float* beta, int N, int K,
                              int n_pad, void* wq, void* wscale, float* bias_csum, void* stream);

/* Optional split-K scratch (fp32, 32 MiB is enough for every shape of the path).  Launches with fewer than ~64 output
 * tiles (remainder rows, M <= 256) then split K over up to 16 workgroups per tile and reduce in a second tiny kernel;
 * without it they run unsplit.  The buffer must stay valid until it is replaced; pass NULL to unregister. */
int keds_gemm_set_workspace(void* ptr, size_t bytes);

/* out = epilogue(A . W^T 2^-w_exp + bias) on split fp16 operands (KEDS_EPI_X3_*): A_hi = a, A_lo = a + a_plane elements (rows of
 * lda elements), W_hi = w, W_lo = w + w_plane (dense [N, K]); the W planes hold W 2^w_exp (keds_split_f16_weight; 0 for planes
 * of the matrix as stored).  M, N, K as keds_gemm_bt_ex2; ldc in elements of the output type. */
int keds_gemm_x3(const void* a, int64_t a_plane, int64_t lda, const void* w, int64_t w_plane, const float* bias, void* out,
                 int64_t ldc, int M, int N, int K, int epilogue, int aux_i, int w_exp, void* stream);
/* x fp32 [rows, cols] (row stride ld elements) -> fp16 planes hi = out, lo = out + plane (dense rows of `cols`): the A operand
 * of keds_gemm_x3.  x = hi + lo to 22 significant bits for |x| >= 2^-3; below that the low plane is an fp16 subnormal and the pair
 * carries x to an ABSOLUTE 2^-25 (activations are O(1): LayerNorm outputs, attention outputs, QuickGELU values).  Values beyond
 * the fp16 range raise *overflow (device int32, nullable) instead of going through as inf. */
int keds_split_f16_pair(const float* x, int64_t ld, int64_t rows, int cols, void* out, int64_t plane, int* overflow, void* stream);
/* A WEIGHT matrix w fp32 dense [n, k] -> the planes of w 2^e, with e = *w_exp (host int, written) chosen so that max |w| 2^e lies
 * in [2^13, 2^14): small weights (|w| ~ 1e-2 .. 1e-3 in real checkpoints) then keep 22 bits -- split as stored their low plane
 * falls into the fp16 subnormals and keeps 14-17.  Pass *w_exp to keds_gemm_x3.  Packing-time call: waits for the stream once. */
int keds_split_f16_weight(const float* w, int64_t n, int k, void* out, int64_t plane, int* w_exp, void* stream);
/* Which kernel form a keds_gemm_bt* / keds_gemm_x3 call gets is decided in one host function (csrc/gemm_plan.h: the rules;
 * docs/kernels.md: the table of forms).  The three entries below steer it, report what it led to, and ask it without a GPU.
 *
 * test/bench hook, process-wide, `on` replaces the previous call's bits: bit 0 routes every GEMM through the 128x128 kernel,
 * bit 9 disables split-K; A/B switches of the 256x256 kernels: bit 10 residual tile as the accumulators' initial value,
 * bits 11-12 kernel form (1 = 4 waves, 2 = 4 waves persistent, 3 = 8 waves; 0 = by shape), bit 16 no three-deep A ring,
 * bit 17 no deferred epilogue stores in the persistent kernel.  Every form computes the same GEMM.  Bit 8 (no remainder-row
 * launch) and bits 13-15 (stamped builds) were timing-only and last existed at 14f64ac: KEDS_E_ARG, previous bits kept. */
int keds_gemm_force_small(int on);
/* test hook: what the last keds_gemm_bt* / keds_gemm_x3 call of the calling thread launched -- written where each kernel is
 * launched, not copied from the plan; a call whose launches differ from its plan fails with KEDS_E_LAUNCH.  info[8] (host ints, written):
 * [0] kernel form of the main launch, [1] of the remainder-row launch behind a 256 x 256 main launch (KEDS_GEMM_FORM_NONE: there
 * was none), [2] / [3] their LDS ring depths (K-tiles of the A operand in flight: 2, 3 or 4), [4] / [5] their split-K slice counts
 * (1 = no split, no reduce kernel), [6] 1 = the main launch was persistent (one workgroup per CU walks the tiles),
 * [7] KEDS_GEMM_FLAG_* of the main launch. */
#define KEDS_GEMM_FORM_NONE 0
#define KEDS_GEMM_FORM_SMALL 1   /* 128 x 128 tiles, 4 waves */
#define KEDS_GEMM_FORM_PAIR 2    /* 256 x 256 tiles, 8 waves */
#define KEDS_GEMM_FORM_QUAD 3    /* 256 x 256 tiles, 4 waves */
#define KEDS_GEMM_FORM_QUAD3 4   /* 256 x 256 tiles, 4 waves, three-deep A ring (fp16-residual epilogues) */
#define KEDS_GEMM_FLAG_DEFER 1           /* persistent LayerNorm form: part of a tile's stores leave inside the next tile's K-loop */
#define KEDS_GEMM_FLAG_RESID_PROLOGUE 2  /* residual tile + bias as the accumulators' initial value (bit 10 of the hook above) */
int keds_gemm_last_launch(int* info);
/* The plan of the call keds_gemm_bt_ex2 / keds_gemm_x3 (epilogue, M, N, K, lda, ldc) on a device of `cus` compute units, with
 * `splitk_bytes` of split-K scratch registered (0: none) and, small_lds != 0, with the 64 KiB-LDS
 * form of the 128 x 128 kernel; under the switches keds_gemm_force_small set.  info[8] as keds_gemm_last_launch.  Touches no
 * device.  The shape rules of keds_gemm_bt_ex2 apply (N % 128, K % 64, row strides, a dense EPI_PATCH output). */
int keds_gemm_plan_query(int epilogue, int M, int N, int K, int64_t lda, int64_t ldc, int cus, size_t splitk_bytes, int small_lds,
                         int* info);
/* the same for n calls at once (a sweep from Python costs its ctypes calls otherwise): cases [n][9] host int64 = {epilogue, M, N,
 * K, lda, ldc, cus, splitk_bytes, small_lds}, info [n][8].  Stops at the first case keds_gemm_plan_query rejects. */
int keds_gemm_plan_query_many(int64_t n, const int64_t* cases, int* info);

/* y = LayerNorm(x) * gamma + beta over the last dim (fp32 statistics, eps 1e-5).
 * x fp32 [rows, dim] with row stride x_stride (elements); out bf16 (out_f32 == 0) or fp32,
 * dense [rows, dim].  dim % 256 == 0 or dim == 128; dim <= 2048. */
int keds_layernorm(const float* x, int64_t x_stride, const float* gamma, const float* beta,
                   void* out, int out_f32, int rows, int dim, void* stream);
/* out_type: 0 bf16, 1 fp32, 2 fp16 */
int keds_layernorm_ex(const float* x, int64_t x_stride, const float* gamma, const float* beta,
                      void* out, int out_type, int rows, int dim, void* stream);

/* Every form of the LayerNorm kernel: output row r reads source row r * row_mul + row_map[r] (row_map int32 [rows], NULL: r * row_mul
 * -- row_mul = S reads the CLS row of every sample), rows x_stride elements apart; out dense [rows, dim], out_type as above.  A row
 * whose map entry is outside [0, row_mul) comes out as NaN in every element. */
int keds_layernorm_rows(const float* x, int64_t x_stride, const int32_t* row_map, int row_mul, const float* gamma, const float* beta,
                        void* out, int out_type, int rows, int dim, void* stream);
/* LayerNorm into a PAIR of fp16 planes, y = hi + lo to 22 bits (the A operand of a split-operand GEMM): hi dense [rows, dim] at out,
 * lo at out + plane elements; plane % 4 == 0, plane >= rows * dim, x_stride % 4 == 0.  form 0: the library's choice (a wave walks
 * several rows at dim 512 / 1024, rows >= 2048, plane % 8 == 0), 1: one row per wave at any row count. */
int keds_layernorm_pair(const float* x, int64_t x_stride, const float* gamma, const float* beta, void* out, int64_t plane, int rows,
                        int dim, int form, void* stream);
/* what this thread's last pair LayerNorm launched: 0 one row per wave, 1 a wave walks several rows; -1 before the first */
int keds_layernorm_pair_last_form(void);

/* rows of a [rows, stride] buffer into another of the same shape and another type: types as out_type above, the source fp32 or
 * fp16; dim % 8 == 0, stride >= dim (columns >= dim are neither read nor written); nt != 0: non-temporal stores */
int keds_cast_rows(const void* src, int src_type, void* dst, int dst_type, int rows, int dim, int64_t stride, int nt, void* stream);
/* one row per sample: dst[b] = src[b * S + row[b]] (global_rows != 0: src[row[b]], S = the rows src holds); mode 0: 16-bit elements
 * copied, 1: fp16 -> fp32, 2: fp32 copied; dim % 8 == 0.  A row outside [0, S) comes out as NaN.  (The name without `token` is the
 * index's gather.) */
int keds_gather_token_rows(const void* src, void* dst, const int32_t* row, int S, int B, int dim, int mode, int global_rows,
                           void* stream);
/* x[b * S, :] = cls + pos[0]: the class-token rows of a [B, S, d] stream; every other row is left alone */
int keds_cls_rows(float* x, const float* cls, const float* pos, int B, int S, int d, void* stream);

/* test / A/B hook of the S = 257 attention, process-wide (0 = product path): bit 4 the generic (padded) kernel, bit 5 the 4-wave
 * tail kernel.  Bits 0-3 and 6 (timing-only ablations) last existed at 14f64ac: KEDS_E_ARG, state unchanged. */
int keds_attention_debug(int variant);

/* multi-head self attention core on a packed qkv buffer (nn.MultiheadAttention,
 * model.py:309,319-321): qkv bf16 [B*S, 3*d] (q | k | v, head h at columns h*64),
 * out bf16 [B*S, d] = softmax(q k^T / 8 [+ causal mask, model.py:543-549]) v.  dh = 64,
 * S <= 288. */
int keds_attention(const void* qkv, void* out, int B, int S, int heads, int causal, void* stream);
/* same, computing and storing only the first q_limit query rows of every sample (keys/values: all S rows) */
int keds_attention_ex(const void* qkv, void* out, int B, int S, int heads, int causal, int q_limit, void* stream);
/* fp8 towers: rows < q8_rows of the output are written as MXFP8 (q8 [q8_rows, d] e4m3, s8 scale dwords [d/128][q8_rows])
 * INSTEAD of bf16; the remaining rows go to `out` as usual */
int keds_attention_mx(const void* qkv, void* out, int B, int S, int heads, int causal, int q_limit, void* q8, void* s8,
                      int q8_rows, void* stream);
/* PACKED rows (round 6): sample b is rows [seq_off[b], seq_off[b + 1]) of qkv / out (device int32 [B + 1]; lengths 1 .. s_max
 * <= 288) instead of [b S, (b + 1) S): sequences of different lengths without padding rows (the text tower, keds_text_run_packed) */
int keds_attention_packed(const void* qkv, void* out, int B, int s_max, const int32_t* seq_off, int heads, int causal, void* stream);
/* fp16 forms of keds_attention_ex / keds_attention_packed (keds_tower_params.f16): qkv and out fp16, both products on the fp16
 * matrix instruction, the probabilities rounded to fp16.  The output is a convex combination of V and cannot overflow. */
int keds_attention_h(const void* qkv, void* out, int B, int S, int heads, int causal, int q_limit, void* stream);
int keds_attention_packed_h(const void* qkv, void* out, int B, int s_max, const int32_t* seq_off, int heads, int causal, void* stream);
/* Which kernel form the six entries above get is decided in one host function (csrc/attention_plan.h: the rules; docs/kernels.md: the
 * table of forms) under keds_attention_debug's switches.  info[8] (host ints, written): [0] KEDS_ATTN_FORM_*, [1] 16-key tiles held
 * (2, 6, 18; 16 + the rank-1 last key for the two S = 257 forms), [2] leading key tiles left unmasked (0 or 16), [3] KEDS_ATTN_FLAG_*,
 * [4] grid, [5] block, [6] LDS bytes, [7] the effective q_limit. */
#define KEDS_ATTN_FORM_NONE 0
#define KEDS_ATTN_FORM_GENERIC 1    /* attention_kernel<nkt, causal, nfull>: 4 waves, keys padded to whole tiles */
#define KEDS_ATTN_FORM_TAIL1 2      /* attention_tail1_kernel<16>: 4 waves, S = 257 as 16 tiles + one key / query */
#define KEDS_ATTN_FORM_S257 3       /* attention_s257_kernel: 8 waves, S = 257 (the ViT-L/14 tower) */
#define KEDS_ATTN_FLAG_CAUSAL 1
#define KEDS_ATTN_FLAG_F16 2        /* fp16 qkv / out */
#define KEDS_ATTN_FLAG_Q8 4         /* MXFP8 output rows */
#define KEDS_ATTN_FLAG_PACKED 8     /* per-sample row offsets */
#define KEDS_ATTN_FLAG_STOP_EVENT 16 /* the form whose launch can record a (library-internal) caller's event as its stop event */
/* the plan of a call (packed != 0: S = s_max, q_limit ignored; q8 != 0: MXFP8 output rows); touches no device; B, heads > 0 and
 * 1 <= S <= 288, else KEDS_E_ARG with info untouched */
int keds_attention_plan_query(int B, int S, int heads, int causal, int q_limit, int f16, int q8, int packed, int* info);
/* test hook: what the calling thread's last such call launched -- written where the kernel is launched, not copied from the plan; a
 * call whose launch differs from its plan fails with KEDS_E_LAUNCH */
int keds_attention_last_launch(int* info);

/* patch im2col for conv1 (model.py:381,394-396): image fp32 [B,3,R,R] -> bf16 [B*G, Kpad],
 * column c*P*P + ky*P + kx, zero padded to Kpad (a multiple of 64). */
int keds_im2col(const float* image, void* out, int B, int R, int P, int Kpad, void* stream);
int keds_im2col_ex(const float* image, void* out, int out_f16, int B, int R, int P, int Kpad, void* stream);   /* out fp16 */

/* token embedding + optional pseudo-token splice + positional embedding
 * (model.py:579-581, 817-837): x fp32 [B, L, d].
 *   tokens int32 [B,L]; table bf16/fp32?  -> fp32 table [vocab, d]
 *   img_tokens (nullable) fp32 [B, n_tok, d] replaces column `insert_col`, the tail is shifted
 *   right by n_tok-1 and truncated to L. */
int keds_embed_tokens(const int32_t* tokens, const float* table, const float* pos,
                      const float* img_tokens, int n_tok, int insert_col,
                      float* x, int B, int L, int d, void* stream);

/* the same with only the first Lx <= L columns written (x [B, Lx, d]; a splice that reaches beyond Lx is cut there) and, seq_off
 * int32 [B + 1] not NULL, packed rows: sample b writes its first seq_off[b + 1] - seq_off[b] columns to rows seq_off[b] ... of x */
int keds_embed_tokens_ex(const int32_t* tokens, const float* table, const float* pos, const float* img_tokens, int n_tok,
                         int insert_col, float* x, int B, int L, int Lx, int d, const int32_t* seq_off, void* stream);

/* read-out: out[b,:] = LayerNorm(x[b*S + row[b], :]) . proj  (+ optional L2 normalisation)
 * (model.py:412-414, 586-589, 841-849).  proj_t bf16 [E, d] (the projection transposed),
 * row int32 [B] (NULL: row 0, the CLS token).  out fp32 [B, E]. */
int keds_readout(const float* x, int S, const int32_t* row, const float* gamma, const float* beta,
                 const void* proj_t, float* out, int B, int d, int E, int normalize,
                 void* workspace, size_t workspace_bytes, void* stream);
size_t keds_readout_workspace_bytes(int B, int d);

/* rows /= ||row||  (eval_utils.py:162,704-710);  out may alias x */
int keds_l2_normalize(const float* x, float* out, int rows, int dim, void* stream);
/* out = normalize(wa * normalize(a) + wb * normalize(b))  (eval_utils.py:704-710) */
int keds_mix_normalize(const float* a, const float* b, float wa, float wb,
                       float* a_n, float* b_n, float* mix, int rows, int dim, void* stream);
/* fp32 -> bf16 cast (weight packing, model.py:927-948 stand-in) */
int keds_cast_bf16(const float* x, void* out, int64_t count, void* stream);
int keds_cast_f16(const float* x, void* out, int64_t count, void* stream);    /* fp32 -> fp16 (round to nearest even) */

/* =====================================================================================
 * 3. Whole towers
 * ===================================================================================== */
typedef struct {
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;     /* fp32 [d] */
    const void *qkv_w, *out_w, *fc_w, *proj_w;      /* bf16 [3d,d] [d,d] [4d,d] [d,4d] */
    const float *qkv_b, *out_b, *fc_b, *proj_b;     /* fp32 */
    /* optional (all four or none): ln_1 folded into in_proj and ln_2 into c_fc by keds_fold_layernorm_ex(out_f16 = 1).
     * When present the tower runs without LayerNorm passes on an fp16 residual stream (KEDS_EPI_LN_*_H /
     * KEDS_EPI_RESID_STATS_F16); qkv_w / fc_w and the ln parameters are still needed (CLS-only last block). */
    const void *qkv_wf, *fc_wf;                     /* fp16 [3d,d], [4d,d] */
    const float *qkv_bc, *fc_bc;                    /* fp32 [2*3d], [2*4d]: folded bias | column sums */
    /* optional (all or none; needs the folded set above): MXFP8 copies for keds_tower_params.fp8
     * (keds_fold_layernorm_mxfp8: in_proj / c_fc with their LayerNorm folded in, out_proj / c_proj plain);
     * scales in the [K/128][N] dword layout */
    const void *qkv_q8, *out_q8, *fc_q8, *proj_q8;
    const void *qkv_s8, *out_s8, *fc_s8, *proj_s8;
    const float *qkv_bc8, *fc_bc8;                  /* fp32 [2*3d], [2*4d] for the MXFP8 weights */
    /* keds_tower_params.f32 == 2 only: the exponents keds_split_f16_weight returned for qkv_w, out_w, fc_w, proj_w */
    int x3_exp[4];
} keds_block_params;

/* the twelve tensors of one ResidualAttentionBlock: fp32, device, dense, as stored in the checkpoint */
typedef struct {
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    const float *qkv_w, *qkv_b, *out_w, *out_b, *fc_w, *fc_b, *proj_w, *proj_b;
} keds_block_source;

/* Weight preparation of one block, the same for every loader (ABI 10): builds every array keds_block_params points to from
 * `src` into the caller-owned device buffer `buf` (256-byte aligned, keds_block_pack_bytes bytes) and fills `out` completely --
 * fields the mode does not use are null, x3_exp is zero unless f32 == 2.  All arrays are copies (out never aliases src) and
 * start on 256-byte boundaries.  fp8 / f32 / f16 as in keds_tower_params; folded: LayerNorm folded into in_proj / c_fc (ignored
 * when f32 != 0).  With d = width and the GEMMs (N, K) = qkv (3d, d), out (d, d), fc (4d, d), proj (d, 4d), the buffer holds, in
 * this order, each rounded up to 256 bytes:
 *   ln1_g, ln1_b, ln2_g, ln2_b    4 d bytes each (fp32)
 *   qkv_b, out_b, fc_b, proj_b    4 N (fp32)
 *   qkv_w, out_w, fc_w, proj_w    2 N K (bf16; fp16 as keds_cast_f16 rounds when f16), 4 N K when f32 == 1 (fp32 as stored) or
 *                                 f32 == 2 (two fp16 planes of keds_split_f16_weight, exponents in x3_exp)
 *   folded and f32 == 0:          qkv_wf, fc_wf 2 N K (fp16), then qkv_bc, fc_bc 8 N (keds_fold_layernorm_ex, out_f16 = 1)
 *   fp8:                          the four *_q8 N K, the four *_s8 keds_mxfp8_scale_bytes(N, K), qkv_bc8, fc_bc8 8 N
 *                                 (keds_fold_layernorm_mxfp8), and 8 d bytes of scratch for the {bias, column sums} of out-proj /
 *                                 c_proj, which no kernel reads
 * Rules (KEDS_E_ARG from keds_block_pack, 0 from keds_block_pack_bytes, with a message): width % 128 == 0; fp8 needs folded and
 * width % 256 == 0; f16 needs folded and excludes fp8 and f32; fp8 excludes f32.
 * Asynchronous on `stream`, except that f32 == 2 waits for it (keds_split_f16_weight); `src` stays alive until the caller has
 * synchronised. */
size_t keds_block_pack_bytes(int width, int fp8, int f32, int f16, int folded);
int keds_block_pack(const keds_block_source* src, int width, int fp8, int f32, int f16, int folded,
                    void* buf, size_t buf_bytes, keds_block_params* out, void* stream);

typedef struct {
    int width, layers, heads, seq;                  /* seq = tokens per sample (257 / 77) */
    int causal;
    const keds_block_params* blocks;                /* HOST array [layers] of device pointers */
    int fp8;                                        /* 1: BASELINE config 5 -- the four GEMMs of every block run on MXFP8
                                                       operands (full 256-row tiles; remainder rows stay bf16); needs the
                                                       *_q8 block fields and width % 256 == 0 */
    int last_cls_only;                              /* 1: after the LAST block only token 0 of every sample is
                                                       defined (ViT read-out): its attention queries, out-proj, ln_2
                                                       and MLP run on B rows instead of B*seq */
    int f32;                                        /* 1: the fp32-ACCURATE flow (section 10; the reference's own eval
                                                       arithmetic, eval_retrieval.py:108-109): qkv_w / out_w / fc_w / proj_w of
                                                       every block -- and conv_w / proj_t of the enclosing vit / text struct --
                                                       point to FP32 arrays of the same shapes; the folded / MXFP8 fields are
                                                       unused; fp8 must be 0 */
    int f16;                                        /* 1: the "fp16" operating point -- EVERY 16-bit operand of the tower is fp16:
                                                       qkv_w / out_w / fc_w / proj_w (and the folded qkv_wf / fc_wf) of every
                                                       block, conv_w / proj_t of the enclosing vit / text struct; qkv, the
                                                       attention output and the MLP hidden layer are fp16 too (KEDS_EPI_*_F16_H,
                                                       keds_attention_h).  Folded flow only; fp8 and f32 must be 0 */
} keds_tower_params;

typedef struct {
    keds_tower_params tower;
    int resolution, patch, kpad, embed_dim;
    const void* conv_w;                             /* bf16 [width, kpad] (im2col order, zero padded) */
    const float *class_emb, *pos_emb;               /* fp32 [width], [G+1, width] */
    const float *ln_pre_g, *ln_pre_b, *ln_post_g, *ln_post_b;
    const void* proj_t;                             /* bf16 [embed_dim, width] */
} keds_vit_params;

typedef struct {
    keds_tower_params tower;
    int vocab, embed_dim;
    const float *token_emb, *pos_emb;               /* fp32 [vocab,d], [L,d] */
    const float *ln_final_g, *ln_final_b;
    const void* proj_t;                             /* bf16 [embed_dim, d] */
} keds_text_params;

size_t keds_tower_workspace_bytes(int width, int seq, int B);
size_t keds_tower_workspace_bytes_ex(const keds_tower_params* p, int B);   /* knows the fp32-accurate flow (p->f32) */
/* Rows (B*seq mod 256) that a tower pass of keds_vit_run / keds_text_run runs as their own chain on a second, high-priority
 * stream beside the full 256-row tiles (0: one stream; always 0 with KEDS_SIDE_STREAM=0, and 0 with KEDS_TOWER_FILL=1, an
 * experiment that runs the ragged last row tile as a full tile on filler rows -- measured slower, off by default).
 * Side-lane launches carry no profiling events: keds_prof_read(KEDS_PROF_GEMM) then covers the
 * full-tile launches only (bench.py scales the flops to match). */
int keds_tower_side_rows(int width, int seq, int B, int fp8);
int keds_side_lane_enable(int on);            /* run-time override of KEDS_SIDE_STREAM (default: on); results are identical */

/* What a tower pass launches, answered without a GPU from the function the passes themselves run from (csrc/tower_plan.h; ABI 15).
 *   flow         KEDS_TOWER_FLOW_*; width, heads, seq, causal, layers, B as in keds_tower_params
 *   tail         KEDS_TOWER_TAIL_*: what is read after the last block -- every row, the CLS rows (last_cls_only), or one read-out
 *                row per sample (keds_text_run_ex's default flow, keds_text_run_packed)
 *   packed_rows / packed_valid   packed rows (keds_text_run_packed): the rows the pass runs (rows_total rounded up to 256 where the
 *                workspace allows) and rows_total; 0, 0: rectangular rows
 *   taps         the per-block taps of keds_vit_run_tokens
 *   split        -1: the library's own rule (what keds_tower_side_rows reports) decides whether the remainder rows behind the last
 *                full 256-row tile are a span of their own; 0 / 1: as given (an MXFP8 tower splits by its row count alone)
 *   lane         -1: keds_side_lane_enable's setting; 0 / 1: without / with the side lane.  A bf16 / fp16 / fp32x3 pass has a
 *                remainder span only with the lane
 * steps (nullable): int32 [max_steps][KEDS_TOWER_STEP_INTS], the first min(*n_steps, max_steps) steps in enqueue order; *n_steps:
 * the count.  buffers (nullable): int64 [KEDS_TOWER_BUF_COUNT][4] = {id, byte offset in the tower scratch (-1: x, the caller's
 * stream), bytes (0: not a buffer of this flow), alias-of id}; *workspace_bytes (nullable): keds_tower_workspace_bytes_ex.
 * A step record: [0] op  [1] layer (-1: none)  [2] weight (0 none, 1 in_proj, 2 out_proj, 3 c_fc, 4 c_proj, 5 / 6 in_proj / c_fc with
 * their LayerNorm folded in, 7 ln_1, 8 ln_2)  [3] epi: the public epilogue id of a GEMM (KEDS_EPI_* / KEDS_FP8_EPI_* / KEDS_F32_EPI_*),
 * the output type of a LayerNorm / statistics cast (keds_layernorm_ex), the mode of a gather (0 16-bit rows, 1 fp16 -> fp32, 2 fp32
 * rows), the source type of a tap (1 fp32, 2 fp16), 1 for a copy that is a 2-D copy  [4] in  [5] its first row  [6] its row step
 * [7] out  [8] first row  [9] row step  [10] rows  [11] out2: the MXFP8 copy written beside out (its scale buffer: the next id)
 * [12] fp32x3: rows of one fp16 plane of in / out  [13] statistics buffer read  [14] added into (statistics cast: written)
 * [15] cleared  [16] their first row  [17] attention: q_limit  [18] rows written as MXFP8  [19] packed rows  [20] gather: rows
 * outside [0, bound) give NaN; the residual GEMM of a packed folded pass: rows >= bound of out and of [14] are zeroed behind it  [21] global (packed) row indices  [22] lane (0 the caller's stream, 1 the side lane)  [23] a LayerNorm
 * of the read-out rows: 1 when sample b's row is row b * [6] + its read-out column (the device array of keds_text_run_ex).
 * A whole pass (keds_pass_plan_query) adds the weights 9 conv1 (the patch embedding; its GEMM spreads row i of col to row
 * i / G * (G + 1) + 1 + i % G of x and adds the positional embedding), 10 ln_pre, 11 ln_post / ln_final, 12 the projection; the ops
 * KEDS_TOWER_OP_IM2COL ([3]: the output type), _CLS (B rows [9] apart), _EMBED ([10] = B x the columns that run; [19] packed rows)
 * and _L2NORM ([3] 1: the fp32 flows' kernel); and the buffers KEDS_PASS_BUF_*.
 * KEDS_E_ARG for an unknown flow, bad geometry, or packed rows on an MXFP8 / non-causal tower or without a read-out row. */
#define KEDS_TOWER_FLOW_UNFOLDED 0   /* stand-alone LayerNorm launches (no folded weights) */
#define KEDS_TOWER_FLOW_BF16 1
#define KEDS_TOWER_FLOW_FP16 2       /* keds_tower_params.f16 */
#define KEDS_TOWER_FLOW_FP8 3        /* keds_tower_params.fp8 */
#define KEDS_TOWER_FLOW_F32 4        /* keds_tower_params.f32 == 1 */
#define KEDS_TOWER_FLOW_X3 5         /* keds_tower_params.f32 == 2 */
#define KEDS_TOWER_TAIL_ALL 0
#define KEDS_TOWER_TAIL_CLS 1
#define KEDS_TOWER_TAIL_READOUT 2
#define KEDS_TOWER_OP_ZERO 1         /* memset of rows */
#define KEDS_TOWER_OP_STATS_CAST 2   /* keds_rowstats_cast_ex */
#define KEDS_TOWER_OP_QUANT 3        /* keds_quantize_mxfp8 */
#define KEDS_TOWER_OP_CAST 4         /* fp16 rows -> fp32 rows */
#define KEDS_TOWER_OP_COPY 5         /* strided rows, device to device */
#define KEDS_TOWER_OP_SPLIT 6        /* keds_split_f16_pair */
#define KEDS_TOWER_OP_GATHER 7       /* keds_gather_rows */
#define KEDS_TOWER_OP_LN 8           /* keds_layernorm_ex */
#define KEDS_TOWER_OP_LN_PAIR 9      /* keds_layernorm_pair */
#define KEDS_TOWER_OP_ATTN 10        /* the flow's attention */
#define KEDS_TOWER_OP_ATTN_FORK 11   /* the same with the side lane forked behind it (the launch's stop event where the form takes one) */
#define KEDS_TOWER_OP_GEMM16 12      /* keds_gemm_bt_ex2 */
#define KEDS_TOWER_OP_GEMM_MX 13     /* keds_gemm_mxfp8_ex */
#define KEDS_TOWER_OP_GEMM_F32 14    /* keds_gemm_f32 */
#define KEDS_TOWER_OP_GEMM_X3 15     /* keds_gemm_x3 */
#define KEDS_TOWER_OP_TAP 16         /* a span of the stream written out (keds_vit_run_tokens) */
#define KEDS_TOWER_OP_FORK 17        /* the side lane waits for the caller's stream */
#define KEDS_TOWER_OP_JOIN 18        /* the caller's stream waits for the side lane */
#define KEDS_TOWER_OP_IM2COL 19      /* keds_im2col_ex / keds_im2col_f32 */
#define KEDS_TOWER_OP_CLS 20         /* keds_cls_rows */
#define KEDS_TOWER_OP_EMBED 21       /* keds_embed_tokens_ex */
#define KEDS_TOWER_OP_L2NORM 22      /* keds_l2_normalize in place; the fp32 flows' own rows kernel */
enum { KEDS_TOWER_BUF_NONE = 0, KEDS_TOWER_BUF_X, KEDS_TOWER_BUF_H, KEDS_TOWER_BUF_QKV, KEDS_TOWER_BUF_ATT, KEDS_TOWER_BUF_HID,
       KEDS_TOWER_BUF_ST1, KEDS_TOWER_BUF_ST2, KEDS_TOWER_BUF_XQ, KEDS_TOWER_BUF_XS, KEDS_TOWER_BUF_AQ, KEDS_TOWER_BUF_AS,
       KEDS_TOWER_BUF_HQ, KEDS_TOWER_BUF_HS, KEDS_TOWER_BUF_SPLITK, KEDS_TOWER_BUF_LN, KEDS_TOWER_BUF_ATT_C, KEDS_TOWER_BUF_X_C,
       KEDS_TOWER_BUF_COUNT,
       /* a whole pass: col, the im2col matrix (an alias: it starts where the tower scratch starts); ro, the LayerNorm of the read-out
          rows; and the caller's: out [B, embed_dim], the token output of keds_text_run_tokens, the images / token ids */
       KEDS_PASS_BUF_COL = KEDS_TOWER_BUF_COUNT, KEDS_PASS_BUF_RO, KEDS_PASS_BUF_OUT, KEDS_PASS_BUF_TOK, KEDS_PASS_BUF_SRC,
       KEDS_PASS_BUF_COUNT };
#define KEDS_TOWER_STEP_INTS 24
int keds_tower_plan_query(int flow, int width, int heads, int seq, int causal, int layers, int B, int tail, int packed_rows,
                          int packed_valid, int taps, int split, int lane, int32_t* steps, int max_steps, int* n_steps,
                          int64_t* buffers, size_t* workspace_bytes);


/* The same for a WHOLE pass -- front end, blocks, read-out -- of keds_vit_run (KEDS_PASS_VIT), keds_vit_run_tokens with taps or
 * tokens (_VIT_TOKENS), keds_text_run_ex (_TEXT), keds_text_run_packed (_TEXT_PACKED) and keds_text_run_tokens (_TEXT_TOKENS);
 * KEDS_PASS_TOWER is keds_tower_plan_query.  The entries themselves run from these steps.  The steps are the record above; buffers:
 * int64 [KEDS_PASS_BUF_COUNT][4], byte offsets in the PASS workspace (-1: the caller's own buffer); *workspace_bytes:
 * keds_vit_workspace_bytes / keds_text_workspace_bytes for the shape (for a text kind: of the columns that run). */
#define KEDS_PASS_TOWER 0
#define KEDS_PASS_VIT 1
#define KEDS_PASS_VIT_TOKENS 2
#define KEDS_PASS_TEXT 3
#define KEDS_PASS_TEXT_PACKED 4
#define KEDS_PASS_TEXT_TOKENS 5
typedef struct {
    int kind, flow, width, heads, layers, B, causal;
    int seq;                                   /* tower and ViT kinds: rows per sample; text kinds: derived (the columns that run) */
    int resolution, patch, kpad, embed_dim;    /* ViT kinds; embed_dim: every kind with a read-out */
    int context;                               /* text kinds: L */
    int seq_used;                              /* _TEXT: the host's cut (0: unknown); _TEXT_PACKED: seq_max */
    int trim;                                  /* keds_text_trim_mode: 0 - 3 */
    int rows_total;                            /* _TEXT_PACKED */
    int n_tok, insert_col;                     /* the splice of pseudo tokens (n_tok 0: none) */
    int cls_only;                              /* keds_tower_params.last_cls_only */
    int readout;                               /* _VIT_TOKENS: 0 without `out` */
    int normalize, out_type;
    int split, lane;                           /* as keds_tower_plan_query's */
} keds_pass_shape;
int keds_pass_plan_query(const keds_pass_shape* shape, int32_t* steps, int max_steps, int* n_steps, int64_t* buffers,
                         size_t* workspace_bytes);
/* 1 when keds_text_forward_packed runs a batch of B captions with rows_total = sum of (read-out column + 1) and seq_used = the longest
 * on packed rows: a causal tower that is not the MXFP8 one, trim mode 1, and rows_total * 8 <= B * seq_used * 7.  No GPU needed. */
int keds_text_runs_packed(int causal, int fp8, int trim, int64_t rows_total, int B, int seq_used);

/* x fp32 [B*seq (padded to 128), width] in place through all residual blocks (model.py:372-373); workspace: rows padded to 256 */
int keds_tower_forward(const keds_tower_params* p, float* x, int B,
                       void* workspace, size_t workspace_bytes, void* stream);

/* _transform of src/model/clip.py:107-123 (eval branch) on the device: raw uint8 images [B,H,W,3] of one size (device) ->
 * fp32 [B,3,n_px,n_px]: bicubic Resize of the shorter side to n_px (PIL semantics: two antialiased passes with a uint8
 * intermediate), CenterCrop, /255, (x - mean) / std.  mean3 / std3: HOST arrays of 3 floats. */
/* bit-exact form: PIL's integer resampling (22-bit fixed-point weights computed by the host exactly as PIL's Resample.c
 * does, horizontal pass first, uint8 intermediate).  need_h / need_v: the axis is resampled at all (PIL skips a pass that
 * keeps the size); xb/yb [n_px][2] = {first source index, taps} of every output column/row of the crop, xk/yk
 * [n_px][ksx|ksy] their int32 weights; left/top: crop offset when an axis is NOT resampled (>= 0, and the window
 * [left, left + n_px) / [top, top + n_px) must lie inside the image, or the call is refused).  out_u8 (nullable)
 * [B,n_px,n_px,3]: the uint8 image PIL would hand to ToTensor.
 * keds_preprocess: the same two passes with fp32 weights computed on the device; one 8-bit step from PIL on rare pixels. */
int keds_preprocess_pil(const unsigned char* images, int B, int H, int W, int n_px, int need_h, int need_v, int left, int top,
                        const int32_t* xb, const int32_t* xk, int ksx, const int32_t* yb, const int32_t* yk, int ksy,
                        const float* mean3, const float* std3, float* out, unsigned char* out_u8, void* stream);
int keds_preprocess(const unsigned char* images, int B, int H, int W, int n_px, const float* mean3, const float* std3,
                    float* out, void* stream);

/* CLIP.encode_image (model.py:569-575,393-415): image fp32 [B,3,R,R] -> out fp32 [B, embed_dim] */
size_t keds_vit_workspace_bytes(const keds_vit_params* p, int B);
int keds_vit_run(const keds_vit_params* p, const float* image, int B, float* out, int normalize,
                     void* workspace, size_t workspace_bytes, void* stream);

/* CLIP.encode_image(mid_feature=True) / VisualTransformer.get_tokens (model.py:393-427, 337-342): the same pass as
 * keds_vit_run with the residual stream written out as out_type (0 bf16, 1 fp32, 2 fp16, as keds_layernorm_ex):
 *   taps    nullable [layers, B, S, width]: after block l, rows [0, B*S) of the stream at taps + l*B*S*width (sample-major: the
 *           reference's NLD order), the state before ln_post
 *   tokens  nullable [B, S, width]: after the last block only
 *   out     nullable fp32 [B, embed_dim]: the features of the same pass (as keds_vit_run, normalize as there)
 * At least one of the three.  With taps or tokens the last block runs on every row (keds_tower_params.last_cls_only is ignored)
 * and the read-out takes the CLS rows of the full stream.  Workspace: keds_vit_workspace_bytes.  The taps are written with
 * plain stores; keds_tap_store_nt(1) makes them non-temporal (an A/B: measured no faster, tools/bench_tokens.py). */
int keds_vit_run_tokens(const keds_vit_params* p, const float* image, int B, float* out, int normalize, void* taps, void* tokens,
                        int out_type, void* workspace, size_t workspace_bytes, void* stream);
int keds_tap_store_nt(int on);      /* 1: non-temporal tap stores; 0 (default): plain stores */

/* CLIP.encode_text / encode_text_img_retrieval (model.py:577-590, 808-851):
 * tokens int32 [B,L]; readout_row int32 [B]; img_tokens nullable fp32 [B,n_tok,d]. */
size_t keds_text_workspace_bytes(const keds_text_params* p, int B);
int keds_text_run(const keds_text_params* p, const int32_t* tokens, const int32_t* readout_row,
                      const float* img_tokens, int n_tok, int insert_col, int B, float* out, int normalize,
                      void* workspace, size_t workspace_bytes, void* stream);
/* The same with the host's knowledge of the read-out columns (ABI 7).  The mask is causal (model.py:543-549) and only the
 * read-out row of every sample is read (model.py:587-589, 847-849), so columns >= seq_used = max(readout_row) + 1 cannot
 * change the result: they are neither embedded nor run through the blocks (the sequence is cut there), and the last block's
 * out-proj / ln_2 / MLP run on the B read-out rows only.  seq_used = 0: unknown (all L columns; keds_text_run).  CONTRACT: every readout_row[b] < seq_used -- the rows live on
 * the device and are not checked.  keds_text_trim_enable(0) restores the all-columns / all-rows flow (A/B, bisecting), 2 =
 * the column cut only, 3 = the read-out-row tail only; -1 = the KEDS_TEXT_TRIM environment variable decides (default: on).
 * Numerics: the column cut changes no arithmetic (rows only land in other tiles); the tail runs the last block's out-proj /
 * ln_2 / MLP in the fp32-stream form (stand-alone LayerNorm, fp32 residual, as the ViT's CLS tail does) where the all-rows
 * flow uses the folded form on the fp16 stream: both are roundings of the same fp32 reference, 2-3e-3 apart. */
int keds_text_run_ex(const keds_text_params* p, const int32_t* tokens, const int32_t* readout_row,
                     const float* img_tokens, int n_tok, int insert_col, int B, int seq_used, float* out, int normalize,
                     void* workspace, size_t workspace_bytes, void* stream);
int keds_text_trim_enable(int on);
int keds_text_trim_mode(void);      /* the flow in force (0 .. 3 as above) */
/* CLIP.get_text_tokens (model.py:592-605): out [B, L, width] = ln_final(residual stream after the last block) over ALL L columns,
 * as out_type (0 bf16, 1 fp32, 2 fp16); no projection.  The rectangular flow whatever keds_text_trim_enable says: no column
 * cut, no read-out-row tail, no packed rows.  tokens int32 [B, L]; workspace: keds_text_workspace_bytes. */
int keds_text_run_tokens(const keds_text_params* p, const int32_t* tokens, int B, void* out, int out_type, void* workspace,
                         size_t workspace_bytes, void* stream);
/* The text tower on PACKED rows (round 6, ABI 8): captions end at different columns, and under the causal mask sample b needs its
 * columns [0, len_b) only (len_b = its read-out column + 1) -- keds_text_run_ex cuts every sample at the LONGEST caption of the
 * batch, here sample b owns rows [seq_off[b], seq_off[b + 1]) of every activation buffer and the tower runs sum(len_b) rows.
 *   seq_off         device int32 [B + 1], seq_off[0] = 0, seq_off[B] = rows_total, 1 <= len_b <= seq_max <= tower.seq
 *   readout_global  device int32 [B]: seq_off[b] + the read-out column of sample b (a row outside [0, rows_total) gives NaN)
 * Same arithmetic per row as keds_text_run_ex's default flow (rows only land in other tiles); causal bf16 towers only -- fp8 /
 * fp32 towers and the A/B flows of keds_text_trim_enable go through keds_text_run_ex.  Workspace: keds_text_workspace_bytes. */
int keds_text_run_packed(const keds_text_params* p, const int32_t* tokens, const int32_t* seq_off, const int32_t* readout_global,
                         int rows_total, int seq_max, const float* img_tokens, int n_tok, int insert_col, int B, float* out,
                         int normalize, void* workspace, size_t workspace_bytes, void* stream);

/* =====================================================================================
 * 4. Knowledge injection (IM2TEXT + 2 x CrossFormer, model.py:37-123, eval_utils.py:661-672)
 * ===================================================================================== */
typedef struct {
    const void *wq, *wk, *wv, *wo;                  /* bf16 [inner,dim] x3, [dim,inner] */
    const float *bq, *bk, *bv, *bo;
} keds_cross_layer_params;

typedef struct {                                    /* IM2TEXT: dim_in -> middle (x n_layer, ReLU) -> dim_out */
    int dim_in, middle, dim_out, n_layer;
    const void* w[4]; const float* b[4];            /* bf16 [middle, in] / fp32 [middle] per hidden layer */
    const void* out_w; const float* out_b;          /* bf16 [dim_out, middle] */
} keds_im2text_params;

/* Launch-saving re-arrangement of a CrossFormer's weights (built once by keds_crossformer_fuse from the per-layer ones):
 *  - k and v never change between the layers (model.py:98-101), so ALL layers' k / v projections are one GEMM:
 *    wkv [layers*2*inner, dim] = rows {Wk_0, Wv_0, Wk_1, Wv_1, ...}, bkv likewise;
 *  - layer l's output projection feeds only layer l+1's query projection (no residual, no norm, model.py:56-79), so the
 *    two are one matrix: wqn[l] = Wq_l . Wo_{l-1} [inner, inner], bqn[l] = Wq_l bo_{l-1} + bq_l   (l >= 1). */
typedef struct {
    const void* wkv; const float* bkv;
    const void* wqn[8]; const float* bqn[8];
} keds_crossformer_fused;

typedef struct {                                    /* CrossFormer: `layers` chained CrossAttention layers */
    int dim, heads, layers;                         /* dim_head = 64, inner = heads*64 */
    const keds_cross_layer_params* layer;           /* HOST array [layers] of device pointers */
    const keds_crossformer_fused* fused;            /* HOST struct of device pointers, or NULL (layer-by-layer launches) */
} keds_crossformer_params;

typedef struct {
    keds_im2text_params i2t;
    keds_crossformer_params fuse, cond;             /* retrieval_fuse, text_condition */
} keds_knowledge_params;

/* IM2TEXT.forward (model.py:120-123): x fp32 [rows, dim_in] -> out fp32 [rows, dim_out] */
size_t keds_im2text_workspace_bytes(const keds_im2text_params* p, int rows);
int keds_im2text_forward(const keds_im2text_params* p, const float* x, int rows, float* out,
                         void* workspace, size_t workspace_bytes, void* stream);

/* CrossFormer.forward (model.py:98-101) for single-query attention: q fp32 [B,dim],
 * k, v fp32 [B,K,dim] (K <= 32; v may alias k) -> out fp32 [B,dim] */
size_t keds_crossformer_workspace_bytes(const keds_crossformer_params* p, int B, int K);
int keds_crossformer_forward(const keds_crossformer_params* p, const float* q, const float* k, const float* v,
                             int B, int K, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* build `fused` (above) into a caller-owned device buffer of keds_crossformer_fused_bytes(p) bytes; layers <= 8 */
size_t keds_crossformer_fused_bytes(const keds_crossformer_params* p);
int keds_crossformer_fuse(const keds_crossformer_params* p, void* buffer, size_t buffer_bytes, keds_crossformer_fused* out,
                          void* stream);

/* The kernels of the stream one at a time (what keds_crossformer_forward and keds_knowledge_run launch, through the same
 * helpers); bad arguments return KEDS_E_ARG before any launch.
 * keds_cross_attn_core: single-query attention, dim_head 64: Q bf16 [B, 64 heads], Kp / Vp bf16 rows [B K] of stride kv_ld
 *   elements (kv_ld >= 64 heads: the fused form keeps every layer's k | v side by side), out bf16 [B, 64 heads]; K in [1, 32].
 * keds_knowledge_pack_rows: rows bf16 [B (1 + 2 K), dim] = [q; nbr_img; nbr_txt] (fp32, 16-byte aligned), dim % 8 == 0.
 * keds_place_token: tokens[b, slot, :] = src[b, :] for tokens fp32 [B, nslots, dim], 0 <= slot < nslots. */
int keds_cross_attn_core(const void* Q, const void* Kp, const void* Vp, void* out, int B, int K, int heads, int kv_ld, void* stream);
int keds_knowledge_pack_rows(const float* q, const float* nbr_img, const float* nbr_txt, void* rows, int B, int K, int dim,
                             void* stream);
int keds_place_token(const float* src, float* tokens, int B, int dim, int slot, int nslots, void* stream);

/* Multi-query cross-attention core (CrossAttention.forward, model.py:56-79, for any number of queries and keys), dim_head 64, no mask:
 *   out[b, i, h] = softmax(Q[b, i, h] . K[b, :, h]^T / 8) . V[b, :, h]
 * Q bf16 rows [B Lq] of stride q_ld elements, head h at columns 64 h .. 64 h + 63; Kp / Vp bf16 rows [B Lk] of stride kv_ld (two
 * pointers: K and V may be two column ranges of one wide buffer, and only the 64 heads columns behind each pointer are ever read);
 * out bf16 rows [B Lq] of stride o_ld, of which only the 64 heads leading columns are written.  1 <= Lk <= KEDS_CROSS_SEQ_MAX_KEYS;
 * Lq >= 1 has no limit of its own.  KEDS_E_ARG before any launch for a null pointer, B, Lq or heads < 1, Lk outside the range, a
 * stride below 64 heads or not a multiple of 8, or a pointer that is not 16-byte aligned.  The arithmetic is keds_attention's
 * (bf16 operands and probabilities on the matrix instruction, fp32 statistics).  keds_cross_attn_core keeps its own limits. */
#define KEDS_CROSS_SEQ_MAX_KEYS 288
int keds_cross_attn_seq(const void* Q, const void* Kp, const void* Vp, void* out, int B, int Lq, int Lk, int heads, int q_ld, int kv_ld,
                        int o_ld, void* stream);
/* Which launch the call above gets is decided in one host function (csrc/cross_seq_plan.h: the rules; docs/kernels.md: the table).
 * info[8] (host ints, written): [0] KEDS_CROSS_SEQ_FORM_*, [1] 16-key tiles held in LDS (2, 6, 18), [2] leading key tiles left
 * unmasked (0 or 16), [3] query rows per workgroup, [4] grid, [5] block, [6] LDS bytes, [7] workgroups per (sample, head). */
#define KEDS_CROSS_SEQ_FORM_NONE 0
#define KEDS_CROSS_SEQ_FORM_TILE 1  /* cross_attn_seq_kernel<nkt, nfull>: 4 waves, keys padded to whole tiles, K and V^T in LDS */
/* the plan of a call; touches no device; B, Lq, heads >= 1 and 1 <= Lk <= 288, else KEDS_E_ARG with info untouched */
int keds_cross_seq_plan_query(int B, int Lq, int Lk, int heads, int* info);
/* test hook: what the calling thread's last keds_cross_attn_seq call launched -- written where the kernel is launched, not copied
 * from the plan; a call whose launch differs from its plan fails with KEDS_E_LAUNCH */
int keds_cross_seq_last_launch(int* info);

/* CrossFormer.forward (model.py:98-101) on sequences: q fp32 [B,Lq,dim], k, v fp32 [B,Lk,dim] (Lk <= KEDS_CROSS_SEQ_MAX_KEYS; v may
 * alias k, which skips its cast) -> out fp32 [B,Lq,dim].  The per-layer chain of keds_crossformer_forward on B Lq query rows, made
 * of public pieces: keds_cast_bf16 of the inputs; per layer the q / k / v projections (keds_gemm_bt, KEDS_EPI_BIAS_BF16),
 * keds_cross_attn_seq, and the output projection (bf16 between layers, KEDS_EPI_BIAS_F32 for the last).  p->fused is not used.
 * KEDS_E_ARG before any launch; a workspace below keds_crossformer_seq_workspace_bytes is KEDS_E_WORKSPACE with nothing written. */
size_t keds_crossformer_seq_workspace_bytes(const keds_crossformer_params* p, int B, int Lq, int Lk);
int keds_crossformer_forward_seq(const keds_crossformer_params* p, const float* q, const float* k, const float* v, int B, int Lq, int Lk,
                                 float* out, void* workspace, size_t workspace_bytes, void* stream);

size_t keds_knowledge_workspace_bytes(const keds_knowledge_params* p, int B, int K);
/* one stream of eval_utils.py:661-672: q [B,dim] fp32, nbr_img / nbr_txt [B,K,dim] fp32 ->
 * tokens_out [B,3,dim] fp32 = [retrieval_fuse(m, I, I), text_condition(m, T, T), m], m = img2text(q),
 * I = img2text(nbr_img), T = img2text(nbr_txt) */
int keds_knowledge_run(const keds_knowledge_params* p, const float* q, const float* nbr_img,
                           const float* nbr_txt, int B, int K, float* tokens_out,
                           void* workspace, size_t workspace_bytes, void* stream);

/* =====================================================================================
 * 9. Training step of the knowledge-injection modules: building blocks of the forward in training
 *    mode, of the backward through IM2TEXT / CrossFormer / the FROZEN text tower, of the symmetric contrastive loss and
 *    of AdamW (src/trainer.py:44-165, src/main.py:215-237).  The matrix products run on keds_gemm_bt* (dX = dY.W with
 *    W^T as the operand, dW = dY^T.X with both operands transposed: keds_transpose_to_bf16); the host (keds_amd/train.py)
 *    sequences the step, as the reference's Python does.  Gradients that feed a GEMM are bf16, the residual-stream
 *    gradient, LayerNorm, softmax, loss and optimizer arithmetic fp32.
 * ===================================================================================== */
/* out bf16 [cols, ld_out] = transpose of src [rows, cols] (fp32 or bf16, row stride ld_src), columns rows..ld_out-1 zero */
int keds_transpose_to_bf16(const void* src, int src_is_f32, int64_t ld_src, int rows, int cols, void* out, int ld_out, void* stream);
/* out[c] (+)= sum_r x[r][c]: bias gradients (fixed summation order: reproducible) */
int keds_colsum(const void* x, int x_is_f32, int64_t ld, int rows, int cols, float* out, int accumulate, void* stream);
/* IM2TEXT hidden layer y = relu(dropout(z)) (model.py:112-116); mask uint8 (1 = keep; NULL = no dropout), scale = 1/(1-p) */
int keds_dropout_mask(uint8_t* mask, int64_t n, uint64_t seed, float p, void* stream);
int keds_dropout_relu_fwd(const void* z_bf16, const uint8_t* mask, float scale, void* y_bf16, int64_t n, void* stream);
int keds_dropout_relu_bwd(const void* dy, int dy_is_f32, const void* z_bf16, const uint8_t* mask, float scale, void* dz_bf16,
                          int64_t n, void* stream);
/* QuickGELU with the pre-activation kept (model.py:300-302) */
int keds_qgelu_fwd(const void* u_bf16, void* y_bf16, int64_t n, void* stream);
int keds_qgelu_bwd(const void* dy_bf16, const void* u_bf16, void* du_bf16, int64_t n, void* stream);
/* LayerNorm with saved statistics {mean, rstd} per row; rowmap (nullable): row r reads x[rowmap[r]] */
int keds_ln_fwd_stats(const float* x, int64_t ld, const int32_t* rowmap, const float* gamma, const float* beta, void* y_bf16,
                      float* stats, int rows, int dim, void* stream);
/* dx[rowmap[r]] += dLN/dx (dy [rows, dim] compact fp32; gamma frozen: no parameter gradients); dx_bf16 (nullable): bf16 copy */
int keds_ln_bwd(const float* dy, const float* x, int64_t ld, const int32_t* rowmap, const float* stats, const float* gamma,
                float* dx, void* dx_bf16, int rows, int dim, void* stream);
/* self-attention backward on the packed qkv buffer of keds_attention (S <= 80): dout bf16 [B*S, d] -> dqkv bf16 [B*S, 3d] */
int keds_attention_bwd(const void* qkv, const void* dout, void* dqkv, int B, int S, int heads, int causal, void* stream);
/* single-query cross-attention core (model.py:56-79) on projected bf16 rows Q [B, inner], K / V [B*K, inner], and backward */
int keds_cross_core_fwd(const void* Q, const void* Kp, const void* Vp, void* out, int B, int K, int heads, void* stream);
int keds_cross_core_bwd(const void* Q, const void* Kp, const void* Vp, const void* dout, void* dQ, void* dK, void* dV, int B,
                        int K, int heads, void* stream);
/* trainer.py:78-127: logits = scale * img_n . txt_n^T over N gathered rows (this rank's B_local first), loss = (CE rows + CE
 * columns) / 2 -> loss[0] (device), dtxt_n [B_local, dim] = dloss / d txt_n of this rank's rows (remote rows carry no grad) */
size_t keds_clip_loss_workspace_bytes(int N);
int keds_clip_loss(const float* img_n, const float* txt_n, int N, int B_local, int dim, float scale, float* loss, float* dtxt_n,
                   void* workspace, size_t workspace_bytes, void* stream);
/* y = x / ||x||:  dx = (dy - y (y . dy)) / ||x|| */
int keds_l2norm_bwd(const float* x, const float* dy, float* dx, int rows, int dim, void* stream);
/* torch.optim.AdamW update of one flat parameter buffer (step counts from 1); the gradient is read as g * grad_scale
 * (1 / world size after a SUM all-reduce) */
int keds_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int step, float grad_scale, void* stream);
/* dst[map[r]] (+)= src[r]  /  dst[r] = src[map[r]]   (read-out rows, spliced token rows) */
int keds_rows_scatter(const float* src, const int32_t* map, float* dst, int64_t ld_dst, int rows, int dim, int accumulate,
                      void* stream);
int keds_rows_gather(const float* src, int64_t ld_src, const int32_t* map, float* dst, int rows, int dim, void* stream);

/* =====================================================================================
 * 10. The fp32-accurate operating point (csrc/f32path.hip)
 * =====================================================================================
 * The reference evaluates in fp32 (src/eval_retrieval.py:108-109, flag src/params.py:227-232).  These kernels run the same
 * path WITHOUT rounding any operand: products on the f32-input matrix instruction (exact fp32 products, fp32 accumulate),
 * fp32 residual stream / LayerNorm output / q, k, v / probabilities / MLP hidden layer.  keds_vit_run / keds_text_run /
 * keds_tower_forward take this flow when keds_tower_params.f32 = 1 (CLIP.set_precision("fp32"), KEDS_F32 compute of
 * keds_vit_create / keds_text_create).  About 1/10 of the default flow's throughput: an accuracy reference, not the headline. */
#define KEDS_F32_EPI_BIAS 0      /* out = acc + bias                                   */
#define KEDS_F32_EPI_QGELU 1     /* out = quick_gelu(acc + bias)   (model.py:300-302)  */
#define KEDS_F32_EPI_RESID 2     /* out += acc + bias                                  */
#define KEDS_F32_EPI_RELU 3      /* out = max(acc + bias, 0)                           */
#define KEDS_F32_EPI_PATCH 4     /* patch embedding: row remap + positional embedding (aux = pos_emb [G+1, N], aux_i = G) */
/* out[M,N] (row stride ldc) = epilogue(A[M,K] (row stride lda) . W[N,K]^T + bias); all fp32; N % 128 == 0, K % 16 == 0,
 * strides multiples of 4; bias nullable */
int keds_gemm_f32(const float* A, int64_t lda, const float* W, const float* bias, float* out, int64_t ldc, int M, int N, int K,
                  int epilogue, const float* aux, int aux_i, void* stream);
/* keds_attention_ex on fp32 qkv [B*S, 3*d] -> out fp32 [B*S, d]; q_limit <= 0: all rows; S <= 288 */
int keds_attention_f32(const float* qkv, float* out, int B, int S, int heads, int causal, int q_limit, void* stream);
/* keds_attention_f32 at fp32 grade on the fp16 matrix instruction (the fp32x3 operating point, csrc/attention_x3.hip): q, k, v
 * and the probabilities as two fp16 planes each, three products per product, fp32 softmax.  out: fp32 [B*S, d] (nullable);
 * pair: fp16 planes [2][plane] of the same rows (nullable; what keds_gemm_x3 reads as its A operand); at least one of them.
 * overflow (nullable int on the device): raised when |q / 8|, |k| or |v| >= 65504.  Reference: src/model/model.py:319-321 */
int keds_attention_x3(const float* qkv, float* out, void* pair, int64_t plane, int B, int S, int heads, int causal, int q_limit,
                      int* overflow, void* stream);
/* the two on PACKED rows (keds_attention_packed): sample b is rows [seq_off[b], seq_off[b + 1]) of qkv / out (device int32 [B + 1],
 * lengths 1 .. s_max <= 288), every query row of every sample; what keds_text_run_packed launches in the fp32 and fp32x3 flows.
 * x3: `plane` is the distance of the two planes in elements and must hold every packed row (the caller's to size: the row count
 * lives on the device). */
int keds_attention_f32_packed(const float* qkv, float* out, int B, int s_max, const int32_t* seq_off, int heads, int causal, void* stream);
int keds_attention_x3_packed(const float* qkv, float* out, void* pair, int64_t plane, int B, int s_max, const int32_t* seq_off, int heads,
                             int causal, int* overflow, void* stream);
/* keds_im2col with an fp32 patch matrix [B*G, Kpad] (Kpad % 16 == 0) */
int keds_im2col_f32(const float* image, float* out, int B, int R, int P, int Kpad, void* stream);
/* keds_knowledge_run with EVERY weight pointer of the params an FP32 array (per-layer weights; `fused` unused): one stream
 * of the knowledge injection, tokens_out fp32 [B,3,dim]; K <= 64 */
size_t keds_knowledge_f32_workspace_bytes(const keds_knowledge_params* p, int B, int K);
int keds_knowledge_run_f32(const keds_knowledge_params* p, const float* q, const float* nbr_img, const float* nbr_txt, int B,
                           int K, float* tokens_out, void* workspace, size_t workspace_bytes, void* stream);

/* the fp32 stream's single-query attention core alone: Q fp32 [B, 64 heads], Kp / Vp fp32 [B K, 64 heads] -> out fp32
 * [B, 64 heads]; K in [1, 64] */
int keds_cross_core_f32(const float* Q, const float* Kp, const float* Vp, float* out, int B, int K, int heads, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KEDS_HIP_H */
