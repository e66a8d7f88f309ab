/*
 * keds_select.h -- extension header of libkeds_hip.so: filtered exact search over a resident index.
 *
 * The counterpart of faiss.SearchParameters(sel=IDSelector...): one index, searched over a SUBSET of its rows, with a short
 * per-query list of ids to leave out on top (the reference removes "the reference image" from a top-101 after the search,
 * src/eval_utils.py get_metrics_cirr_topk; the knowledge path's own-row neighbour, src/trainer.py:198-230).
 *
 * An extension header: it adds entry points to the same library and the same KEDS_ABI_VERSION without touching keds_hip.h.
 * It is written in the C subset of keds_hip.h, includes only "keds_hip.h", is parsed by the same parser (keds_amd/_abi.py,
 * EXT_HEADERS) and locked by tests/golden/abi_select_v1.json.  Whoever next moves KEDS_ABI_VERSION folds it into keds_hip.h.
 * The conventions of keds_hip.h hold: device pointers, caller-owned buffers, stream-ordered, no allocation, capturable,
 * KEDS_OK or a negative KEDS_E_* with keds_last_error().
 *
 * Selector `sel` (nullable: every row): uint32 words, ceil(n/32) of them -- one per 32-key stage of the scan image.  Bit
 *   (r & 31), least significant first, of word (r >> 5) is set when LOCAL row r is eligible.  Bits at or beyond n are ignored.
 * Exclusions `exclude` (nullable with n_exclude == 0: none): int64 [nq, n_exclude], 0 <= n_exclude <= KEDS_SEL_MAX_EXCLUDE,
 *   GLOBAL ids in the numbering of I (local row + id_base).  Entries that are -1, outside [id_base, id_base + n), duplicated
 *   or ineligible are ignored.
 * Result: the exact top-k by (distance, id) over the rows that are eligible and not excluded for that query, in the order --
 *   and with the bits of D -- that the unfiltered search gives on those rows.  Fewer than k such rows: the usual fillers
 *   (+inf | -inf, -1, zero rows from the gather).
 * The certificate is unchanged: the image's bounds are maxima over ALL rows, so they bound the eligible ones too.
 * The plan does not depend on the selector: keds_index_search_plan_query and the workspace size of
 *   keds_index_search_workspace_bytes_ex describe the filtered search as well.
 * keds_index_search_packed_ex, keds_search_scan, keds_search_certify and keds_search_exact are the null-argument calls of
 *   the entries below; with sel == NULL the scan launches the same kernels as ever.
 * Every argument is checked before any launch: n_exclude outside [0, 16], exclude == NULL with n_exclude > 0, count < 0 and
 *   ids == NULL with count > 0 return KEDS_E_ARG.
 */
#ifndef KEDS_SELECT_H
#define KEDS_SELECT_H

#include "keds_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KEDS_SEL_MAX_EXCLUDE 16

/* sel[ceil(n/32)]: drop == 0: zero, then set the bits of ids; drop != 0: all ones, then clear them.
 * ids: global ids (int64, count >= 0, nullable when 0); ids outside [id_base, id_base + n) are ignored.
 * One fill launch and one scatter launch (none when count == 0). */
int keds_sel_build(uint32_t* sel, int64_t n, const int64_t* ids, int64_t count, int64_t id_base, int drop, void* stream);

/* keds_index_search_packed_ex + sel (nullable) + exclude (nullable) / n_exclude; same workspace size as _ex */
int keds_index_search_packed_sel(const void* packed, const float* db, int64_t n, int dim, int metric,
                      const float* queries, int nq, int normalize_q, int k, int64_t id_base,
                      float* D, int64_t* I, float* rows_out,
                      void* workspace, size_t workspace_bytes, int32_t* status,
                      const uint32_t* sel, const int64_t* exclude, int n_exclude, void* stream);

/* the stage entries of keds_hip.h with the new arguments (tests/test_gpu_search_select_edges.py); sel is indexed by the
 * ABSOLUTE stage / row, exclude is [nq, n_exclude] */
int keds_search_scan_sel(const void* packed, int64_t n, int dim, int stages, const void* qb, int nqb, const float* thr /* nullable */,
                         int depth, int nwg, uint64_t* pairs, uint32_t* meta, const uint32_t* sel /* nullable */, void* stream);
int keds_search_certify_sel(const void* packed, int64_t n, int dim, const int32_t* cand_idx, const float* cand_d, int nq, int ncand,
                            int metric, int k, int64_t id_base, const float* qstat, const float* sbound, float* D, int64_t* I,
                            int32_t* counters, int32_t* fail_ids, int32_t* fslot, float* dk, int32_t* status /* nullable */,
                            int force_fail, const int64_t* exclude /* nullable */, int n_exclude, void* stream);
int keds_search_exact_sel(const float* db, int64_t n, int dim, int metric, const float* qn, int32_t* counters, const int32_t* fail_ids,
                          const float* dk, int chunk_rows, int k, int64_t id_base, uint64_t* plist, int32_t* pcnt, float* D, int64_t* I,
                          const uint32_t* sel /* nullable */, const int64_t* exclude /* nullable */, int n_exclude, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KEDS_SELECT_H */
