// Dual-stream knowledge injection (one stream per keds_knowledge_run call):
//   m      = IM2TEXT(q)                                   (src/model/model.py:105-123)
//   I', T' = IM2TEXT(neighbour image rows), IM2TEXT(neighbour text rows)
//   fused  = CrossFormer_fuse(m, I', I');  cond = CrossFormer_cond(m, T', T')   (model.py:37-101)
//   tokens = [fused, cond, m]                              (src/eval_utils.py:661-672)
// IM2TEXT runs ONCE over the stacked rows [q; I; T] (B*(1+2K) rows) through the MFMA GEMM with
// fused bias+ReLU; the cross-attention core (1 query x K keys x heads) is one wave per
// (sample, head) with the head dimension (64) on the lanes.  keds_im2text_forward and
// keds_crossformer_forward expose the two modules on their own (IM2TEXT.forward /
// CrossFormer.forward of the reference API).
// Every host chain of the stream lives here, written once over its numeric form (bf16 with one query, bf16 on sequences, fp32):
// xf_chain is the CrossFormer layer chain (xf_run_fused: the fused weight form) and i2t_hidden the IM2TEXT hidden layers.  The
// kernels of the other two forms are in cross_seq.hip and f32path.hip.  The fp16 stream (keds_knowledge_f16.h) is a fourth form,
// F16One: the kernels below are templates on the 16-bit element type, the entries on the form.
#include "keds_common.h"
#include "gemm_shared.h"         // f16_range_max / f16_range_flag: the fp16 range guard
#include "cross_seq_plan.h"      // DH, cross_seq_grid_fits: the argument rules of keds_crossformer_forward_seq
#include <math.h>
#include <cstring>
#include <type_traits>

namespace {

// one wave per (b, head): lane = head-dim element (dim_head = 64)
// (Kp / Vp rows have stride `kv_ld` elements: the fused form keeps every layer's projections side by side in one buffer)
template <typename T>      // bf16_t or f16_t
__global__ __launch_bounds__(256) void cross_attn_core_kernel(const T* __restrict__ Q, const T* __restrict__ Kp,
                                                              const T* __restrict__ Vp, T* __restrict__ out,
                                                              int B, int K, int heads, int kv_ld) {
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= B * heads) return;
    const int b = w / heads, h = w % heads;
    const int inner = heads * 64;
    const float q = (float)Q[(size_t)b * inner + h * 64 + lane];
    float sc[32];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        if (j < K) {
            const float kv = (float)Kp[((size_t)b * K + j) * kv_ld + h * 64 + lane];
            sc[j] = wave_sum(q * kv) * 0.125f;
            mx = fmaxf(mx, sc[j]);
        } else {
            sc[j] = -INFINITY;
        }
    }
    float sum = 0.f, o = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        if (j < K) {
            const float p = __expf(sc[j] - mx);
            sum += p;
            o += p * (float)Vp[((size_t)b * K + j) * kv_ld + h * 64 + lane];
        }
    }
    out[(size_t)b * inner + h * 64 + lane] = (T)(o / sum);
}

// tokens[b, slot, :] = src[b, :]
__global__ void place_token_kernel(const float* __restrict__ src, float* __restrict__ tokens, int B, int dim, int slot,
                                   int nslots) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * dim) return;
    const int b = i / dim, j = i % dim;
    tokens[((size_t)b * nslots + slot) * dim + j] = src[i];
}

// rows [q; nbr_img; nbr_txt] (fp32) -> one 16-bit matrix [B(1+2K), dim]: one launch instead of three casts
// (fp16 rows: a value beyond the fp16 range, or a non-finite one, raises `guard`; nn == 0: a guarded cast of q alone)
template <typename T>
__global__ __launch_bounds__(256) void pack_rows_kernel(const float* __restrict__ q, const float* __restrict__ ni,
                                                        const float* __restrict__ nt, T* __restrict__ rows, long long nq,
                                                        long long nn, int* __restrict__ guard) {
    typedef __attribute__((ext_vector_type(8))) T t8;
    const long long i = (blockIdx.x * 256LL + threadIdx.x) * 8;
    if (i >= nq + 2 * nn) return;
    const float* src = i < nq ? q + i : (i < nq + nn ? ni + (i - nq) : nt + (i - nq - nn));
    const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
    *reinterpret_cast<t8*>(rows + i) = t8{(T)a[0], (T)a[1], (T)a[2], (T)a[3], (T)b[0], (T)b[1], (T)b[2], (T)b[3]};
    if constexpr (std::is_same<T, f16_t>::value) f16_range_flag(guard, f16_range_max(0u, a, b));
}

// ---- fused CrossFormer weights (keds_hip.h, keds_crossformer_fused) -------------------------------------------------
template <typename T>
__global__ void concat_rows_kernel(const T* __restrict__ src, const float* __restrict__ bsrc, T* __restrict__ dst,
                                   float* __restrict__ bdst, int rows, int cols) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i < (long long)rows * cols) dst[i] = src[i];
    if (i < rows) bdst[i] = bsrc[i];
}
// W'[i][j] = sum_d Wq[i][d] Wo[d][j]  (fp32 sum of the 16-bit weights, rounded once); b'[i] = sum_d Wq[i][d] bo[d] + bq[i]
template <typename T>
__global__ __launch_bounds__(256) void fold_qo_kernel(const T* __restrict__ wq, const float* __restrict__ bq,
                                                      const T* __restrict__ wo, const float* __restrict__ bo, int inner,
                                                      int dim, T* __restrict__ wout, float* __restrict__ bout) {
    const int i = blockIdx.x, j0 = threadIdx.x;
    for (int j = j0; j < inner; j += 256) {
        float a = 0.f;
        for (int d = 0; d < dim; ++d) a += (float)wq[(size_t)i * dim + d] * (float)wo[(size_t)d * inner + j];
        wout[(size_t)i * inner + j] = (T)a;
    }
    if (j0 < 64) {
        float a = 0.f;
        for (int d = j0; d < dim; d += 64) a += (float)wq[(size_t)i * dim + d] * bo[d];
        a = wave_sum(a);
        if (j0 == 0) bout[i] = a + bq[i];
    }
}

// the launches of the three kernels above: the module paths and the stand-alone entries share them
template <typename T>
int launch_core(const void* Q, const void* Kp, const void* Vp, void* out, int B, int K, int heads, int kv_ld, hipStream_t st) {
    KedsProfScope prof(KEDS_PROF_OTHER, st);
    cross_attn_core_kernel<T><<<(B * heads + 3) / 4, 256, 0, st>>>((const T*)Q, (const T*)Kp, (const T*)Vp, (T*)out, B, K, heads, kv_ld);
    return keds_check_launch("cross_attn_core_kernel");
}
int launch_place(const float* src, float* tokens, int B, int dim, int slot, int nslots, hipStream_t st) {
    place_token_kernel<<<(B * dim + 255) / 256, 256, 0, st>>>(src, tokens, B, dim, slot, nslots);
    return keds_check_launch("place_token_kernel");
}
// nq elements of q, then nn of ni and of nt (multiples of 8)
template <typename T>
int launch_pack(const float* q, const float* ni, const float* nt, void* rows, long long nq, long long nn, int* guard, hipStream_t st) {
    KedsProfScope prof(KEDS_PROF_OTHER, st);
    pack_rows_kernel<T><<<(unsigned)(((nq + 2 * nn) / 8 + 255) / 256), 256, 0, st>>>(q, ni, nt, (T*)rows, nq, nn, guard);
    return keds_check_launch("pack_rows_kernel");
}

int check_i2t(const keds_im2text_params* p, const char* who) {
    if (!p || p->n_layer < 1 || p->n_layer > 4 || !p->out_w) {
        keds_set_error("%s: bad IM2TEXT parameters", who);
        return KEDS_E_ARG;
    }
    if (p->dim_in % 128 || p->middle % 128 || p->dim_out % 128) {
        keds_set_error("%s: IM2TEXT dims (%d,%d,%d) must be multiples of 128", who, p->dim_in, p->middle, p->dim_out);
        return KEDS_E_ARG;
    }
    return KEDS_OK;
}

int check_xf(const keds_crossformer_params* p, const char* who) {
    if (!p || !p->layer || p->layers < 1 || p->heads < 1 || (p->heads * 64) % 128 || p->dim % 128) {
        keds_set_error("%s: bad CrossFormer parameters", who);
        return KEDS_E_ARG;
    }
    return KEDS_OK;
}

// ---- the numeric forms of the host chains -----------------------------------------------------------------------------
// What a chain asks of a GEMM: rows of the form's own element type, the same after ReLU (IM2TEXT's hidden layers), the fp32
// rows a CrossFormer's last layer hands back, or rows of which the first `head_rows` also land as fp32 in a token slot (the
// stream's last IM2TEXT layer).  A form supplies its element size, the GEMM with row strides, the attention core on projected rows
// of stride `ld`, and how fp32 inputs become its rows (pack: [q; nbr_img; nbr_txt] in one launch; cast: n elements); the chains
// below are written once over it.
enum ChainEpi { CE_ROWS, CE_RELU, CE_OUT_F32, CE_ROWS_HEAD };

struct Bf16One {      // bf16 operands on the MFMA GEMM, one query per sample over K <= 32 keys
    static constexpr size_t esize = 2;
    static int gemm(const void* A, long long lda, const void* W, const float* bias, void* out, long long ldc, int M, int N, int K,
                    ChainEpi e, hipStream_t st, const float* head = nullptr, int head_rows = 0) {
        const int epi = e == CE_ROWS ? KEDS_EPI_BIAS_BF16 : e == CE_RELU ? KEDS_EPI_BIAS_RELU_BF16 : e == CE_OUT_F32 ? KEDS_EPI_BIAS_F32
                                                                                                    : KEDS_EPI_BIAS_BF16_HEADF32;
        return keds_gemm_bt_ex(A, lda, W, bias, out, ldc, M, N, K, epi, head, head_rows, st);
    }
    static int core(const void* Q, const void* Kp, const void* Vp, void* out, int B, int, int Lk, int heads, int ld, hipStream_t st) {
        return launch_core<bf16_t>(Q, Kp, Vp, out, B, Lk, heads, ld, st);
    }
    static int pack(const float* q, const float* ni, const float* nt, void* rows, int B, int K, int dim, hipStream_t st) {
        return launch_pack<bf16_t>(q, ni, nt, rows, (long long)B * dim, (long long)B * K * dim, nullptr, st);
    }
    static int cast(const float* x, void* out, int64_t n, hipStream_t st) { return keds_cast_bf16(x, out, n, st); }
};
// fp16 operands on the same GEMM kernels (ids 32-34 of keds_knowledge_f16.h and KEDS_EPI_BIAS_F32_H), one query over K <= 32 keys.
// Every kernel that stores fp16 checks the range against the thread's guard, which the entries point at their range_flag
// (KedsGuardScope); the cast is the pack kernel on one input, for that check.
struct F16One {
    static constexpr size_t esize = 2;
    static int gemm(const void* A, long long lda, const void* W, const float* bias, void* out, long long ldc, int M, int N, int K,
                    ChainEpi e, hipStream_t st, const float* head = nullptr, int head_rows = 0) {
        const int epi = e == CE_ROWS ? KEDS_EPI_BIAS_F16_H : e == CE_RELU ? KEDS_EPI_BIAS_RELU_F16_H : e == CE_OUT_F32 ? KEDS_EPI_BIAS_F32_H
                                                                                                      : KEDS_EPI_BIAS_F16_H_HEADF32;
        return keds_gemm_bt_ex(A, lda, W, bias, out, ldc, M, N, K, epi, head, head_rows, st);
    }
    static int core(const void* Q, const void* Kp, const void* Vp, void* out, int B, int, int Lk, int heads, int ld, hipStream_t st) {
        return launch_core<f16_t>(Q, Kp, Vp, out, B, Lk, heads, ld, st);
    }
    static int pack(const float* q, const float* ni, const float* nt, void* rows, int B, int K, int dim, hipStream_t st) {
        return launch_pack<f16_t>(q, ni, nt, rows, (long long)B * dim, (long long)B * K * dim, keds_numerics_guard(), st);
    }
    static int cast(const float* x, void* out, int64_t n, hipStream_t st) {
        return launch_pack<f16_t>(x, nullptr, nullptr, out, n, 0, keds_numerics_guard(), st);
    }
};
struct Bf16Seq : Bf16One {      // ... Lq queries per sample over Lk <= 288 keys (cross_seq.hip: its plan and its record check)
    static int core(const void* Q, const void* Kp, const void* Vp, void* out, int B, int Lq, int Lk, int heads, int ld, hipStream_t st) {
        return keds_cross_attn_seq(Q, Kp, Vp, out, B, Lq, Lk, heads, ld, ld, ld, st);
    }
};
struct F32One {       // every weight an fp32 array, every product on the f32-input MFMA (f32path.hip), one query over K <= 64 keys
    static constexpr size_t esize = 4;
    static int gemm(const void* A, long long lda, const void* W, const float* bias, void* out, long long ldc, int M, int N, int K,
                    ChainEpi e, hipStream_t st, const float* = nullptr, int = 0) {
        return keds_gemm_f32((const float*)A, lda, (const float*)W, bias, (float*)out, ldc, M, N, K,
                             e == CE_RELU ? KEDS_F32_EPI_RELU : KEDS_F32_EPI_BIAS, nullptr, 0, st);
    }
    static int core(const void* Q, const void* Kp, const void* Vp, void* out, int B, int, int Lk, int heads, int, hipStream_t st) {
        return keds_cross_core_f32_impl((const float*)Q, (const float*)Kp, (const float*)Vp, (float*)out, B, Lk, heads, st);
    }
};

// ---- IM2TEXT: (Linear, Dropout = identity, ReLU) x n_layer on rows [R, dim_in] through the two buffers h in turn; *last: the
// buffer the last layer wrote, [R, middle].  What follows (fc_out) differs between the flows and stays with the callers.
template <class P>
int i2t_hidden(const keds_im2text_params* p, const void* rows, int R, char* const (&h)[2], const void** last, hipStream_t st) {
    const void* cur = rows;
    int cur_dim = p->dim_in;
    for (int l = 0; l < p->n_layer; ++l) {
        if (int rc = P::gemm(cur, cur_dim, p->w[l], p->b[l], h[l & 1], p->middle, R, p->middle, cur_dim, CE_RELU, st)) return rc;
        cur = h[l & 1];
        cur_dim = p->middle;
    }
    *last = cur;
    return KEDS_OK;
}

// the two hidden buffers, [R, middle] each (the bf16 flows pad R: every operand of the MFMA GEMM is addressable up to the next
// multiple of 128 rows; keds_gemm_f32 clamps the rows of a ragged last tile instead)
template <class P>
void carve_i2t(KedsCarver& c, const keds_im2text_params* p, size_t R, char* (&h)[2]) {
    for (char*& b : h) b = c.take(R * p->middle * P::esize);
}

// IM2TEXT on 16-bit rows [R, dim_in] -> fp32 [R, dim_out]
template <class P>
int i2t_run(const keds_im2text_params* p, const void* rows16, int R, float* out_f, char* const (&h)[2], hipStream_t st) {
    const void* cur;
    if (int rc = i2t_hidden<P>(p, rows16, R, h, &cur, st)) return rc;
    return P::gemm(cur, p->middle, p->out_w, p->out_b, out_f, p->dim_out, R, p->dim_out, p->middle, CE_OUT_F32, st);
}

// ---- CrossFormer: q chained through the layers, k and v fixed (model.py:98-101).  Per layer the three projections, the core and
// the output projection; q rows [B Lq, dim] with stride ldq, k / v rows [B Lk, dim] with stride ld_kv, all of the form's element
// type; the last layer's output lands in `out` as fp32 rows of stride ldo.
struct XfBufs {
    char *qcur, *Qp, *Kp, *Vp, *att;      // [Rq, dim], [Rq, inner], [Rk, inner] x 2, [Rq, inner]
};

template <class P>
int xf_chain(const keds_crossformer_params* p, const void* q, long long ldq, const void* k, const void* v, long long ld_kv, int B, int Lq,
             int Lk, float* out, long long ldo, const XfBufs& s, hipStream_t st) {
    const int dim = p->dim, inner = p->heads * 64, Rq = B * Lq, Rk = B * Lk;
    int rc;
    for (int l = 0; l < p->layers; ++l) {
        const keds_cross_layer_params& c = p->layer[l];
        const bool last = l == p->layers - 1;
        if ((rc = P::gemm(q, ldq, c.wq, c.bq, s.Qp, inner, Rq, inner, dim, CE_ROWS, st))) return rc;
        if ((rc = P::gemm(k, ld_kv, c.wk, c.bk, s.Kp, inner, Rk, inner, dim, CE_ROWS, st))) return rc;
        if ((rc = P::gemm(v, ld_kv, c.wv, c.bv, s.Vp, inner, Rk, inner, dim, CE_ROWS, st))) return rc;
        if ((rc = P::core(s.Qp, s.Kp, s.Vp, s.att, B, Lq, Lk, p->heads, inner, st))) return rc;
        if ((rc = P::gemm(s.att, inner, c.wo, c.bo, last ? (void*)out : s.qcur, last ? ldo : dim, Rq, dim, inner, last ? CE_OUT_F32 : CE_ROWS, st)))
            return rc;
        q = s.qcur;
        ldq = dim;
    }
    return KEDS_OK;
}

// the five buffers for Rq query rows and Rk key rows (padded by the callers of the bf16 forms, as above)
template <class P>
XfBufs carve_xf_bufs(KedsCarver& c, const keds_crossformer_params* p, size_t Rq, size_t Rk) {
    const size_t dim = (size_t)p->dim, inner = (size_t)p->heads * 64;
    XfBufs s;
    s.qcur = c.take(Rq * dim * P::esize);
    s.Qp = c.take(Rq * inner * P::esize);
    s.Kp = c.take(Rk * inner * P::esize);
    s.Vp = c.take(Rk * inner * P::esize);
    s.att = c.take(Rq * inner * P::esize);
    return s;
}

// 16-bit inputs, one query: q [B,dim], k rows [B*K,dim], v rows [B*K,dim] -> fp32 [B,dim]  (the buffers of the two 16-bit forms
// have one size)
size_t xf_bytes(const keds_crossformer_params* p, int B, int K) {
    KedsCarver c{nullptr};
    carve_xf_bufs<Bf16One>(c, p, rpad(B), rpad((size_t)B * K));
    return c.bytes();
}
template <class P>
int xf_run(const keds_crossformer_params* p, const void* q16, const void* k16, const void* v16, int B, int K, float* out_f,
           char* scratch, hipStream_t st) {
    KedsCarver c{scratch};
    const XfBufs s = carve_xf_bufs<P>(c, p, rpad(B), rpad((size_t)B * K));
    return xf_chain<P>(p, q16, p->dim, k16, v16, p->dim, B, 1, K, out_f, p->dim, s, st);
}

// Fused form (p->fused): ONE GEMM projects the neighbour rows for all layers' k and v, each later layer's query comes
// straight from the previous layer's attention output (folded Wq.Wo), and the last output projection writes fp32 rows with
// stride `ld_out` (e.g. a token slot of [B,3,dim]).  2 + 2*layers launches instead of 5*layers.
struct XfFusedScratch {
    char *KV, *Qp, *att;
    size_t bytes;
};
XfFusedScratch carve_xf_fused(const keds_crossformer_params* p, int B, int K, char* base) {
    XfFusedScratch s;
    KedsCarver c{base};
    const int inner = p->heads * 64;
    s.KV = c.take(rpad((size_t)B * K) * (size_t)p->layers * 2 * inner * 2);
    s.Qp = c.take(rpad(B) * inner * 2);
    s.att = c.take(rpad(B) * inner * 2);
    s.bytes = c.bytes();
    return s;
}

template <class P>
int xf_run_fused(const keds_crossformer_params* p, const void* q16, const void* kv16, int B, int K, float* out_f,
                 long long ld_out, char* scratch, hipStream_t st) {
    static_assert(P::esize == 2, "carve_xf_fused sizes 16-bit rows");
    const keds_crossformer_fused* f = p->fused;
    XfFusedScratch s = carve_xf_fused(p, B, K, scratch);
    const int dim = p->dim, inner = p->heads * 64, BK = B * K, kv_ld = p->layers * 2 * inner;
    int rc;
    if ((rc = P::gemm(kv16, dim, f->wkv, f->bkv, s.KV, kv_ld, BK, kv_ld, dim, CE_ROWS, st))) return rc;
    for (int l = 0; l < p->layers; ++l) {
        if (l == 0) {
            if ((rc = P::gemm(q16, dim, p->layer[0].wq, p->layer[0].bq, s.Qp, inner, B, inner, dim, CE_ROWS, st))) return rc;
        } else if ((rc = P::gemm(s.att, inner, f->wqn[l], f->bqn[l], s.Qp, inner, B, inner, inner, CE_ROWS, st)))
            return rc;
        const char* kp = s.KV + (size_t)l * 2 * inner * P::esize;
        if ((rc = P::core(s.Qp, kp, kp + inner * P::esize, s.att, B, 1, K, p->heads, kv_ld, st))) return rc;
    }
    const keds_cross_layer_params& last = p->layer[p->layers - 1];
    return P::gemm(s.att, inner, last.wo, last.bo, out_f, ld_out, B, dim, inner, CE_OUT_F32, st);
}

}  // namespace

extern "C" size_t keds_crossformer_fused_bytes(const keds_crossformer_params* p) {
    if (!p || p->layers < 1 || p->layers > 8) return 0;
    const size_t inner = (size_t)p->heads * 64;
    size_t b = keds_align_up((size_t)p->layers * 2 * inner * p->dim * 2, 256) + keds_align_up((size_t)p->layers * 2 * inner * 4, 256);
    b += (size_t)(p->layers - 1) * (keds_align_up(inner * inner * 2, 256) + keds_align_up(inner * 4, 256));
    return b;
}

namespace {
template <typename T>      // the weights' element type: bf16_t or f16_t
int xf_fuse(const keds_crossformer_params* p, void* buffer, size_t buffer_bytes, keds_crossformer_fused* out, void* stream,
            const char* who) {
    int rc = check_xf(p, who);
    if (rc) return rc;
    KEDS_REQUIRE(buffer && out && p->layers <= 8, "%s: bad argument (at most 8 layers)", who);
    KEDS_REQUIRE(buffer_bytes >= keds_crossformer_fused_bytes(p), "%s: buffer too small", who);
    hipStream_t st = (hipStream_t)stream;
    const int inner = p->heads * 64, dim = p->dim;
    KedsCarver arrays{(char*)buffer};
    T* wkv = (T*)arrays.take((size_t)p->layers * 2 * inner * dim * 2);
    float* bkv = (float*)arrays.take((size_t)p->layers * 2 * inner * 4);
    memset(out, 0, sizeof(*out));
    out->wkv = wkv;
    out->bkv = bkv;
    const unsigned blocks = (unsigned)(((size_t)inner * dim + 255) / 256);
    for (int l = 0; l < p->layers; ++l) {
        const keds_cross_layer_params& c = p->layer[l];
        concat_rows_kernel<T><<<blocks, 256, 0, st>>>((const T*)c.wk, c.bk, wkv + (size_t)(2 * l) * inner * dim, bkv + (2 * l) * inner,
                                                      inner, dim);
        concat_rows_kernel<T><<<blocks, 256, 0, st>>>((const T*)c.wv, c.bv, wkv + (size_t)(2 * l + 1) * inner * dim,
                                                      bkv + (2 * l + 1) * inner, inner, dim);
        if (l >= 1) {
            T* w = (T*)arrays.take((size_t)inner * inner * 2);
            float* b = (float*)arrays.take((size_t)inner * 4);
            const keds_cross_layer_params& prev = p->layer[l - 1];
            fold_qo_kernel<T><<<inner, 256, 0, st>>>((const T*)c.wq, c.bq, (const T*)prev.wo, prev.bo, inner, dim, w, b);
            out->wqn[l] = w;
            out->bqn[l] = b;
        }
    }
    return keds_check_launch(who);
}
}  // namespace

extern "C" int keds_crossformer_fuse(const keds_crossformer_params* p, void* buffer, size_t buffer_bytes,
                                     keds_crossformer_fused* out, void* stream) {
    return xf_fuse<bf16_t>(p, buffer, buffer_bytes, out, stream, "keds_crossformer_fuse");
}
extern "C" int keds_crossformer_fuse_f16(const keds_crossformer_params* p, void* buffer, size_t buffer_bytes,
                                         keds_crossformer_fused* out, void* stream) {
    return xf_fuse<f16_t>(p, buffer, buffer_bytes, out, stream, "keds_crossformer_fuse_f16");
}

// ---- the stream's kernels one at a time (keds_hip.h) ---------------------------------------------
namespace {
template <class P>
int cross_core_entry(const void* Q, const void* Kp, const void* Vp, void* out, int B, int K, int heads, int kv_ld, void* stream,
                     const char* who) {
    KEDS_REQUIRE(Q && Kp && Vp && out && B > 0 && heads >= 1, "%s: bad argument", who);
    KEDS_REQUIRE(K >= 1 && K <= 32, "%s: K=%d must be in [1,32]", who, K);
    KEDS_REQUIRE(kv_ld >= 64 * heads, "%s: kv_ld=%d is less than 64 heads", who, kv_ld);
    return P::core(Q, Kp, Vp, out, B, 1, K, heads, kv_ld, (hipStream_t)stream);
}
template <class P>
int pack_rows_entry(const float* q, const float* nbr_img, const float* nbr_txt, void* rows, int B, int K, int dim, void* stream,
                    const char* who) {
    KEDS_REQUIRE(q && nbr_img && nbr_txt && rows && B > 0 && K >= 1 && dim > 0, "%s: bad argument", who);
    KEDS_REQUIRE(dim % 8 == 0, "%s: dim=%d must be a multiple of 8", who, dim);
    return P::pack(q, nbr_img, nbr_txt, rows, B, K, dim, (hipStream_t)stream);
}
}  // namespace

extern "C" int keds_cross_attn_core(const void* Q, const void* Kp, const void* Vp, void* out, int B, int K, int heads, int kv_ld,
                                    void* stream) {
    return cross_core_entry<Bf16One>(Q, Kp, Vp, out, B, K, heads, kv_ld, stream, "keds_cross_attn_core");
}
extern "C" int keds_cross_attn_core_h(const void* Q, const void* Kp, const void* Vp, void* out, int B, int K, int heads, int kv_ld,
                                      void* stream) {
    return cross_core_entry<F16One>(Q, Kp, Vp, out, B, K, heads, kv_ld, stream, "keds_cross_attn_core_h");
}

extern "C" int keds_knowledge_pack_rows(const float* q, const float* nbr_img, const float* nbr_txt, void* rows, int B, int K, int dim,
                                        void* stream) {
    return pack_rows_entry<Bf16One>(q, nbr_img, nbr_txt, rows, B, K, dim, stream, "keds_knowledge_pack_rows");
}
extern "C" int keds_knowledge_pack_rows_h(const float* q, const float* nbr_img, const float* nbr_txt, void* rows, int B, int K, int dim,
                                          void* stream) {
    return pack_rows_entry<F16One>(q, nbr_img, nbr_txt, rows, B, K, dim, stream, "keds_knowledge_pack_rows_h");
}

extern "C" int keds_place_token(const float* src, float* tokens, int B, int dim, int slot, int nslots, void* stream) {
    KEDS_REQUIRE(src && tokens && B > 0 && dim > 0 && nslots >= 1 && slot >= 0 && slot < nslots, "keds_place_token: bad argument");
    return launch_place(src, tokens, B, dim, slot, nslots, (hipStream_t)stream);
}

// ---- standalone IM2TEXT ------------------------------------------------------------------------
namespace {
struct I2tWs {
    char* x_bf;      // [Rp, dim_in] bf16
    char* h[2];
    size_t bytes;
};
I2tWs carve_i2t_ws(const keds_im2text_params* p, int rows, void* ws) {
    I2tWs w;
    KedsCarver c{(char*)ws};
    w.x_bf = c.take(rpad(rows) * p->dim_in * 2);       // (16-bit rows: the bf16 and the fp16 form share every layout below)
    carve_i2t<Bf16One>(c, p, rpad(rows), w.h);
    w.bytes = c.bytes();
    return w;
}
}  // namespace

extern "C" size_t keds_im2text_workspace_bytes(const keds_im2text_params* p, int rows) {
    if (!p || rows <= 0) return 0;
    return carve_i2t_ws(p, rows, nullptr).bytes;
}

namespace {
template <class P>
int i2t_forward(const keds_im2text_params* p, const float* x, int rows, float* out, void* workspace, size_t workspace_bytes,
                void* stream, const char* who) {
    int rc = check_i2t(p, who);
    if (rc) return rc;
    KEDS_REQUIRE(x && out && workspace && rows > 0, "%s: bad argument", who);
    const I2tWs w = carve_i2t_ws(p, rows, workspace);
    if (workspace_bytes < w.bytes) {
        keds_set_error("%s: workspace too small", who);
        return KEDS_E_WORKSPACE;
    }
    if ((rc = P::cast(x, w.x_bf, (int64_t)rows * p->dim_in, (hipStream_t)stream))) return rc;
    return i2t_run<P>(p, w.x_bf, rows, out, w.h, (hipStream_t)stream);
}
}  // namespace

extern "C" int keds_im2text_forward(const keds_im2text_params* p, const float* x, int rows, float* out, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    return i2t_forward<Bf16One>(p, x, rows, out, workspace, workspace_bytes, stream, "keds_im2text_forward");
}
extern "C" int keds_im2text_forward_f16(const keds_im2text_params* p, const float* x, int rows, float* out, void* workspace,
                                        size_t workspace_bytes, int32_t* range_flag, void* stream) {
    KedsGuardScope guard(range_flag);
    return i2t_forward<F16One>(p, x, rows, out, workspace, workspace_bytes, stream, "keds_im2text_forward_f16");
}

// ---- standalone CrossFormer: one query per sample, and sequences ---------------------------------------------------
namespace {
// scratch of xf_run, or of xf_run_fused where the parameters carry the fused weights and it is larger
size_t xf_scratch_bytes(const keds_crossformer_params* p, int B, int K) {
    const size_t sc = xf_bytes(p, B, K), fb = p->fused ? carve_xf_fused(p, B, K, nullptr).bytes : 0;
    return fb > sc ? fb : sc;
}

// the head of both entries' workspace: the fp32 inputs as bf16 rows
struct XfIn {
    char *q, *k, *v;
};
XfIn carve_xf_in(KedsCarver& c, const keds_crossformer_params* p, size_t Rq, size_t Rk) {
    XfIn in;
    in.q = c.take(Rq * p->dim * 2);
    in.k = c.take(Rk * p->dim * 2);
    in.v = c.take(Rk * p->dim * 2);
    return in;
}
// q, k, v -> the form's 16-bit rows (nq and nk elements); v == k is cast once and in.v becomes in.k
template <class P>
int cast_qkv(const float* q, const float* k, const float* v, int64_t nq, int64_t nk, XfIn& in, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = P::cast(q, in.q, nq, st))) return rc;
    if ((rc = P::cast(k, in.k, nk, st))) return rc;
    if (v == k) in.v = in.k;
    else if ((rc = P::cast(v, in.v, nk, st))) return rc;
    return KEDS_OK;
}

struct XfWs {
    XfIn in;
    char* scratch;
    size_t bytes;
};
XfWs carve_xf_ws(const keds_crossformer_params* p, int B, int K, void* ws) {
    XfWs w;
    KedsCarver c{(char*)ws};
    w.in = carve_xf_in(c, p, rpad(B), rpad((size_t)B * K));
    w.scratch = c.take(xf_scratch_bytes(p, B, K));
    w.bytes = c.bytes();
    return w;
}

struct XfSeqWs {
    XfIn in;
    XfBufs s;
    size_t bytes;
};
XfSeqWs carve_xf_seq(const keds_crossformer_params* p, int B, int Lq, int Lk, void* ws) {
    XfSeqWs w;
    KedsCarver c{(char*)ws};
    const size_t Rq = rpad((size_t)B * Lq), Rk = rpad((size_t)B * Lk);
    w.in = carve_xf_in(c, p, Rq, Rk);
    w.s = carve_xf_bufs<Bf16Seq>(c, p, Rq, Rk);
    w.bytes = c.bytes();
    return w;
}

int check_xf_seq(const keds_crossformer_params* p, int B, int Lq, int Lk, const char* who) {
    KEDS_REQUIRE(p && p->layer && p->layers >= 1 && p->heads >= 1 && (p->heads * DH) % 128 == 0 && p->dim >= 128 && p->dim % 128 == 0,
                 "%s: bad CrossFormer parameters (dim and 64 heads must be multiples of 128)", who);
    KEDS_REQUIRE(B >= 1 && Lq >= 1, "%s: B=%d and Lq=%d must be at least 1", who, B, Lq);
    KEDS_REQUIRE(Lk >= 1 && Lk <= KEDS_CROSS_SEQ_MAX_KEYS, "%s: Lk=%d must be in [1,%d]", who, Lk, KEDS_CROSS_SEQ_MAX_KEYS);
    KEDS_REQUIRE((long long)B * Lq <= 0x7FFFFFFFLL && (long long)B * Lk <= 0x7FFFFFFFLL && cross_seq_grid_fits(B, Lq, p->heads),
                 "%s: B=%d x Lq=%d (Lk=%d) rows are too many for one call", who, B, Lq, Lk);
    return KEDS_OK;
}
}  // namespace

extern "C" size_t keds_crossformer_workspace_bytes(const keds_crossformer_params* p, int B, int K) {
    if (!p || B <= 0 || K <= 0) return 0;
    return carve_xf_ws(p, B, K, nullptr).bytes;
}

namespace {
template <class P>
int xf_forward(const keds_crossformer_params* p, const float* q, const float* k, const float* v, int B, int K, float* out,
               void* workspace, size_t workspace_bytes, void* stream, const char* who) {
    int rc = check_xf(p, who);
    if (rc) return rc;
    KEDS_REQUIRE(q && k && v && out && workspace && B > 0, "%s: bad argument", who);
    KEDS_REQUIRE(K >= 1 && K <= 32, "%s: K=%d must be in [1,32]", who, K);
    XfWs w = carve_xf_ws(p, B, K, workspace);
    if (workspace_bytes < w.bytes) {
        keds_set_error("%s: workspace too small", who);
        return KEDS_E_WORKSPACE;
    }
    if ((rc = cast_qkv<P>(q, k, v, (int64_t)B * p->dim, (int64_t)B * K * p->dim, w.in, stream))) return rc;
    if (v == k && p->fused) return xf_run_fused<P>(p, w.in.q, w.in.k, B, K, out, p->dim, w.scratch, (hipStream_t)stream);
    return xf_run<P>(p, w.in.q, w.in.k, w.in.v, B, K, out, w.scratch, (hipStream_t)stream);
}
}  // namespace

extern "C" int keds_crossformer_forward(const keds_crossformer_params* p, const float* q, const float* k, const float* v,
                                        int B, int K, float* out, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    return xf_forward<Bf16One>(p, q, k, v, B, K, out, workspace, workspace_bytes, stream, "keds_crossformer_forward");
}
extern "C" int keds_crossformer_forward_f16(const keds_crossformer_params* p, const float* q, const float* k, const float* v, int B,
                                            int K, float* out, void* workspace, size_t workspace_bytes, int32_t* range_flag,
                                            void* stream) {
    KedsGuardScope guard(range_flag);
    return xf_forward<F16One>(p, q, k, v, B, K, out, workspace, workspace_bytes, stream, "keds_crossformer_forward_f16");
}

extern "C" size_t keds_crossformer_seq_workspace_bytes(const keds_crossformer_params* p, int B, int Lq, int Lk) {
    if (!p || B <= 0 || Lq <= 0 || Lk <= 0 || p->dim <= 0 || p->heads <= 0) return 0;
    return carve_xf_seq(p, B, Lq, Lk, nullptr).bytes;
}

// B Lq query rows over B Lk key rows (keds_hip.h); the core is keds_cross_attn_seq (cross_seq.hip)
extern "C" int keds_crossformer_forward_seq(const keds_crossformer_params* p, const float* q, const float* k, const float* v, int B, int Lq,
                                            int Lk, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_xf_seq(p, B, Lq, Lk, "keds_crossformer_forward_seq")) return rc;
    KEDS_REQUIRE(q && k && v && out && workspace, "keds_crossformer_forward_seq: null pointer");
    XfSeqWs w = carve_xf_seq(p, B, Lq, Lk, workspace);
    if (workspace_bytes < w.bytes) {
        keds_set_error("keds_crossformer_forward_seq: workspace %zu < %zu", workspace_bytes, w.bytes);
        return KEDS_E_WORKSPACE;
    }
    // (the fused weight form, p->fused, is not used here: with B Lq query rows the GEMMs carry the work)
    const int dim = p->dim;
    if (int rc = cast_qkv<Bf16Seq>(q, k, v, (int64_t)B * Lq * dim, (int64_t)B * Lk * dim, w.in, stream)) return rc;
    return xf_chain<Bf16Seq>(p, w.in.q, dim, w.in.k, w.in.v, dim, B, Lq, Lk, out, dim, w.s, (hipStream_t)stream);
}

// ---- one full stream ---------------------------------------------------------------------------
namespace {
struct KnWs {
    char* rows_bf;   // [R, dim] bf16 stacked q | nbr_img | nbr_txt (R = B(1+2K))
    float* map_f;    // [R, dim] fp32 IM2TEXT output
    char* map_bf;    // [R + 128, dim] bf16
    float* outf;     // [Bp, dim] fp32 CrossFormer output
    char* h[2];      // IM2TEXT hidden layers
    char* xf;        // CrossFormer scratch (retrieval_fuse)
    char* xf2;       // ... of text_condition: the two chains run side by side on two lanes
    size_t bytes;
};
KnWs carve_kn(const keds_knowledge_params* p, int B, int K, void* ws) {
    KnWs w;
    KedsCarver c{(char*)ws};
    const size_t R = (size_t)B * (1 + 2 * K);
    const int dim = p->i2t.dim_out;
    w.rows_bf = c.take(rpad(R) * p->i2t.dim_in * 2);
    w.map_f = (float*)c.take(rpad(R) * dim * 4);
    w.map_bf = c.take((rpad(R) + 128) * dim * 2);   // GEMMs on sub-ranges may read up to 127 rows past R
    w.outf = (float*)c.take(rpad(B) * dim * 4);
    carve_i2t<Bf16One>(c, &p->i2t, rpad(R), w.h);
    const size_t xb = xf_scratch_bytes(&p->fuse, B, K);
    w.xf = c.take(xb);
    w.xf2 = c.take(xb);
    w.bytes = c.bytes();
    return w;
}

// the fp32 stream: unpadded rows (keds_gemm_f32 clamps the rows of a ragged last tile), one CrossFormer at a time
struct KnowF32Ws {
    float *x, *y;    // [R, dim_in] stacked inputs; [2 B K, dim] mapped neighbours
    char* h[2];      // IM2TEXT hidden layers [R, middle]
    XfBufs s;
    size_t bytes;
};
KnowF32Ws carve_know_f32(const keds_knowledge_params* p, int B, int K, void* ws) {
    const size_t R = (size_t)B + 2 * (size_t)B * K;
    KnowF32Ws w;
    KedsCarver c{(char*)ws};
    w.x = (float*)c.take(R * p->i2t.dim_in * 4);
    carve_i2t<F32One>(c, &p->i2t, R, w.h);
    w.y = (float*)c.take(R * p->i2t.dim_out * 4);
    w.s = carve_xf_bufs<F32One>(c, &p->fuse, B, (size_t)B * K);
    w.bytes = c.bytes();
    return w;
}
}  // namespace

extern "C" size_t keds_knowledge_workspace_bytes(const keds_knowledge_params* p, int B, int K) {
    if (!p || B <= 0 || K <= 0) return 0;
    return carve_kn(p, B, K, nullptr).bytes;
}

namespace {
// one stream on a 16-bit form (Bf16One: keds_knowledge_run; F16One: keds_knowledge_run_f16)
template <class P>
int knowledge_run(const keds_knowledge_params* p, const float* q, const float* nbr_img, const float* nbr_txt, int B, int K,
                  float* tokens_out, void* workspace, size_t workspace_bytes, void* stream, const char* who) {
    static_assert(P::esize == 2, "carve_kn sizes 16-bit rows");
    KEDS_REQUIRE(p && q && nbr_img && nbr_txt && tokens_out && workspace, "%s: null pointer", who);
    KEDS_REQUIRE(B > 0 && K >= 1 && K <= 32, "%s: K must be in [1,32]", who);
    int rc;
    if ((rc = check_i2t(&p->i2t, who))) return rc;
    if ((rc = check_xf(&p->fuse, who))) return rc;
    if ((rc = check_xf(&p->cond, who))) return rc;
    const int dim = p->i2t.dim_out;
    KEDS_REQUIRE(p->i2t.dim_in == dim && p->fuse.dim == dim && p->cond.dim == dim && p->fuse.heads == p->cond.heads,
                 "%s: IM2TEXT and CrossFormer dims must agree", who);
    KnWs w = carve_kn(p, B, K, workspace);
    KedsSplitKScope no_split(nullptr, 0);     // the two CrossFormer chains run on two streams at once: no GEMM here may split K
    if (workspace_bytes < w.bytes) {
        keds_set_error("%s: workspace %zu < %zu", who, workspace_bytes, w.bytes);
        return KEDS_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int R = B * (1 + 2 * K), BK = B * K;
    char* rows = w.rows_bf;
    const size_t row = (size_t)dim * P::esize;      // bytes of one 16-bit row
    const bool fused = p->fuse.fused && p->cond.fused && p->fuse.layers == p->cond.layers;
    if (fused) {
        // 20 launches per stream instead of ~40 (x2 with the remainder-row splits of the GEMMs): one pack of the three
        // inputs, three IM2TEXT GEMMs (the last one writes the bf16 rows AND token slot 2), and per CrossFormer one k/v
        // GEMM for all layers + (query GEMM, attention core) per layer + the output GEMM straight into its token slot.
        // The two CrossFormer chains are independent: text_condition runs on the side lane beside retrieval_fuse.
        if ((rc = P::pack(q, nbr_img, nbr_txt, rows, B, K, dim, st))) return rc;
        const void* cur;
        if ((rc = i2t_hidden<P>(&p->i2t, rows, R, w.h, &cur, st))) return rc;
        if ((rc = P::gemm(cur, p->i2t.middle, p->i2t.out_w, p->i2t.out_b, w.map_bf, dim, R, dim, p->i2t.middle, CE_ROWS_HEAD, st,
                          tokens_out + 2 * dim, B)))
            return rc;
        const char* map_bf = w.map_bf;
        KedsSideLane* lane = keds_side_lane();
        hipStream_t s2 = st;
        if (lane) {
            s2 = lane->s;
            if ((rc = keds_stream_order(st, lane->fork, s2))) return rc;
        }
        rc = xf_run_fused<P>(&p->cond, map_bf, map_bf + (size_t)(B + BK) * row, B, K, tokens_out + dim, 3LL * dim, w.xf2, s2);
        if (!rc) rc = xf_run_fused<P>(&p->fuse, map_bf, map_bf + (size_t)B * row, B, K, tokens_out, 3LL * dim, w.xf, st);
        if (!rc && s2 != st) rc = keds_stream_order(s2, lane->join, st);
        return rc;
    }
    if ((rc = P::cast(q, rows, (int64_t)B * dim, st))) return rc;
    if ((rc = P::cast(nbr_img, rows + (size_t)B * row, (int64_t)BK * dim, st))) return rc;
    if ((rc = P::cast(nbr_txt, rows + (size_t)(B + BK) * row, (int64_t)BK * dim, st))) return rc;
    if ((rc = i2t_run<P>(&p->i2t, rows, R, w.map_f, w.h, st))) return rc;
    if ((rc = P::cast(w.map_f, w.map_bf, (int64_t)R * dim, st))) return rc;
    if ((rc = launch_place(w.map_f, tokens_out, B, dim, 2, 3, st))) return rc;
    const char* map_bf = w.map_bf;
    for (int which = 0; which < 2; ++which) {
        const keds_crossformer_params* xf = which == 0 ? &p->fuse : &p->cond;
        const char* nb = map_bf + (size_t)(B + which * BK) * row;
        if ((rc = xf_run<P>(xf, map_bf, nb, nb, B, K, w.outf, w.xf, st))) return rc;
        if ((rc = launch_place(w.outf, tokens_out, B, dim, which, 3, st))) return rc;
    }
    return KEDS_OK;
}
}  // namespace

extern "C" int keds_knowledge_run(const keds_knowledge_params* p, const float* q, const float* nbr_img,
                                      const float* nbr_txt, int B, int K, float* tokens_out, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    return knowledge_run<Bf16One>(p, q, nbr_img, nbr_txt, B, K, tokens_out, workspace, workspace_bytes, stream, "keds_knowledge_run");
}

// ---- one full stream in fp16 (keds_knowledge_f16.h): the same workspace layout, the same launches -------------------------------
extern "C" size_t keds_knowledge_f16_workspace_bytes(const keds_knowledge_params* p, int B, int K) {
    return keds_knowledge_workspace_bytes(p, B, K);
}

extern "C" int keds_knowledge_run_f16(const keds_knowledge_params* p, const float* q, const float* nbr_img, const float* nbr_txt, int B,
                                      int K, float* tokens_out, void* workspace, size_t workspace_bytes, int32_t* range_flag,
                                      void* stream) {
    KedsGuardScope guard(range_flag);
    return knowledge_run<F16One>(p, q, nbr_img, nbr_txt, B, K, tokens_out, workspace, workspace_bytes, stream, "keds_knowledge_run_f16");
}

// ---- one full stream in fp32 (f32path.hip: the kernels) -------------------------------------------------------------
extern "C" size_t keds_knowledge_f32_workspace_bytes(const keds_knowledge_params* p, int B, int K) {
    if (!p || B <= 0 || K <= 0) return 0;
    return carve_know_f32(p, B, K, nullptr).bytes;
}

// One stream of the knowledge injection with EVERY weight pointer of the params an fp32 array (unfused per-layer weights):
// tokens_out [B,3,dim] = [fuse(m, I, I), cond(m, T, T), m] with m = img2text(q), I / T = img2text(neighbours)
extern "C" int keds_knowledge_run_f32(const keds_knowledge_params* p, const float* q, const float* nbr_img, const float* nbr_txt,
                                      int B, int K, float* tokens_out, void* workspace, size_t workspace_bytes, void* stream) {
    KEDS_REQUIRE(p && q && nbr_img && nbr_txt && tokens_out && workspace && B > 0, "keds_knowledge_run_f32: bad argument");
    KEDS_REQUIRE(K >= 1 && K <= 64, "keds_knowledge_run_f32: K must be in [1, 64]");
    const keds_im2text_params& m = p->i2t;
    const int dim = p->fuse.dim;
    KEDS_REQUIRE(m.dim_in == dim && m.dim_out == dim && p->cond.dim == dim && p->cond.heads == p->fuse.heads && m.n_layer >= 1 &&
                     m.n_layer <= 4 && p->fuse.layer && p->cond.layer,
                 "keds_knowledge_run_f32: inconsistent module shapes");
    KnowF32Ws w = carve_know_f32(p, B, K, workspace);
    if (workspace_bytes < w.bytes) {
        keds_set_error("keds_knowledge_run_f32: workspace %zu < %zu", workspace_bytes, w.bytes);
        return KEDS_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t BK = (size_t)B * K, R = B + 2 * BK;
    if (hipMemcpyAsync(w.x, q, (size_t)B * dim * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(w.x + (size_t)B * dim, nbr_img, BK * dim * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(w.x + ((size_t)B + BK) * dim, nbr_txt, BK * dim * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        keds_set_error("keds_knowledge_run_f32: %s", hipGetErrorString(hipGetLastError()));
        return KEDS_E_LAUNCH;
    }
    int rc;
    const void* last;
    if ((rc = i2t_hidden<F32One>(&m, w.x, (int)R, w.h, &last, st))) return rc;
    const float* cur = (const float*)last;
    // fc_out: the mapped query rows go straight to token slot 2 (row stride 3 dim), the neighbours to y
    float* mapped = tokens_out + 2 * (size_t)dim;
    if ((rc = keds_gemm_f32(cur, m.middle, (const float*)m.out_w, m.out_b, mapped, 3LL * dim, B, dim, m.middle, KEDS_F32_EPI_BIAS, nullptr, 0, st)))
        return rc;
    if ((rc = keds_gemm_f32(cur + (size_t)B * m.middle, m.middle, (const float*)m.out_w, m.out_b, w.y, dim, (int)(2 * BK), dim, m.middle,
                            KEDS_F32_EPI_BIAS, nullptr, 0, st)))
        return rc;
    if ((rc = xf_chain<F32One>(&p->fuse, mapped, 3LL * dim, w.y, w.y, dim, B, 1, K, tokens_out, 3LL * dim, w.s, st))) return rc;
    return xf_chain<F32One>(&p->cond, mapped, 3LL * dim, w.y + BK * dim, w.y + BK * dim, dim, B, 1, K, tokens_out + dim, 3LL * dim, w.s, st);
}
