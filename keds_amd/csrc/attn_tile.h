// The tile routine and the K / V^T staging of the 4-wave attention kernels: attention_kernel and attention_tail1_kernel
// (attention.hip) and cross_attn_seq_kernel (cross_seq.hip) instantiate them, and this is the one place where the LDS image of
// AttnCfg<NKT> (attention_plan.h) is written (attn_stage_kv) and read (attn_tiles): K as swizzled 128-byte rows, V^T with its keys
// permuted to the MFMA k-slot order (attention_tail1_kernel's last query row, one row of VALU work, reads the same image in place).
// Device code only; what each kernel instantiates is decided by its plan header.
#pragma once
#include "keds_common.h"
#include "attention_plan.h"      // DH, AttnCfg
#include <math.h>

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) {
    f32x2 d;
    asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

// element type of the kernels: bf16 (default flow) or fp16 (the "fp16" operating point, keds_attention_h) -- the
// same code; only the matrix instructions, the dot products and the roundings of P / the output follow the type
template <typename T> struct Ev;
template <> struct Ev<bf16_t> { using v8 = bf16x8; using v4 = bf16x4; };
template <> struct Ev<f16_t> { using v8 = f16x8; using v4 = __attribute__((ext_vector_type(4))) _Float16; };
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c, int, int, int) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16(f16x8 a, f16x8 b, f32x4 c, int, int, int) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// ---- stage K (swizzled rows) and V^T (permuted key order) of one (sample, head): key i's 64 elements at k + i ld and v + i ld;
// keys >= nkeys are zero in LDS (a NaN there would survive a zero probability).  ALL: every one of the 16 NKT keys is valid (nkeys is
// not read).  Work item = (4 consecutive keys, one 8-wide dh chunk): all global loads of a thread are issued before the first LDS
// write (one HBM round trip instead of one per item), K goes in with ds_write_b128, and the four keys of an item are adjacent in the
// permuted V^T row, so V^T goes in with 8-byte stores.  The caller's __syncthreads() follows.
template <typename T, int NKT, bool ALL>
__device__ __forceinline__ void attn_stage_kv(const T* k, const T* v, int ld, int nkeys, char* k_lds, char* vt_lds, int tid) {
    using C = AttnCfg<NKT>;
    using V8 = typename Ev<T>::v8;
    using V4 = typename Ev<T>::v4;
    constexpr int ITEMS = (C::KEYS / 4) * 8;
    constexpr int PER = (ITEMS + 255) / 256;
    constexpr bool RAGGED = ITEMS % 256 != 0;
    static_assert(!ALL || !RAGGED, "staging items must divide over the workgroup");
    V8 kreg[PER][4], vreg[PER][4];
#pragma unroll
    for (int it = 0; it < PER; ++it) {
        const int id = tid + it * 256;
        const int quad = id >> 3, ch = id & 7;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int key = quad * 4 + e;
            if constexpr (!ALL) {
                kreg[it][e] = V8{0, 0, 0, 0, 0, 0, 0, 0};
                vreg[it][e] = kreg[it][e];
            }
            if (ALL || ((!RAGGED || id < ITEMS) && key < nkeys)) {
                const size_t off = (size_t)key * (size_t)ld + ch * 8;
                kreg[it][e] = *reinterpret_cast<const V8*>(k + off);
                vreg[it][e] = *reinterpret_cast<const V8*>(v + off);
            }
        }
    }
#pragma unroll
    for (int it = 0; it < PER; ++it) {
        const int id = tid + it * 256;
        if (RAGGED && id >= ITEMS) continue;
        const int quad = id >> 3, ch = id & 7;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int key = quad * 4 + e;
            *reinterpret_cast<V8*>(k_lds + key * 128 + ((ch ^ ((key >> 1) & 7)) << 4)) = kreg[it][e];
        }
        // keys 4*quad .. 4*quad+3: u = key>>5, w = key&31, chunk (4u + ((w&15)>>2)), element 4*(w>>4) + (w&3)
        const int k0 = quad * 4;
        const int u = k0 >> 5, w = k0 & 31;
        const int pos = (4 * u + ((w & 15) >> 2)) * 16 + ((w >> 4) << 2) * 2;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            *reinterpret_cast<V4*>(vt_lds + (ch * 8 + j) * C::VT_ROW + pos) =
                V4{vreg[it][0][j], vreg[it][1][j], vreg[it][2][j], vreg[it][3][j]};
    }
}

template <typename T>
struct AttnCtx {
    const T* q;          // Q of (b, h): row stride q_ld
    T* out;              // out of (b, h): row stride o_ld
    const char* k_lds;
    const char* vt_lds;
    size_t q_ld, o_ld;
    int nq;              // query rows of the sample: a partly filled tile loads row nq - 1 instead (never stored)
    int nk;              // keys of the sample: keys >= nk are masked
    int q_limit;         // rows [.., q_limit) of the sample are stored
    int g, c;
    // MX kernels (fp8 towers): rows < q8_rows of the [B*S, o_ld] output go out as MXFP8 (e4m3 + e8m0 per 32 columns) INSTEAD of T
    unsigned char* q8;    // element (row, col) at q8[row*o_ld + col]; nullptr = T everywhere
    unsigned char* s8;    // scale dwords [o_ld/128][q8_rows]
    int q8_rows, row0, col0;   // first global row of this sample, first column of this head
    const char* tail;          // TAIL kernels: [K row of the last key: 64 elements, unswizzled][its V row: 64 elements]
};

// NQ consecutive 16-query tiles whose first query row (inside the sample) is q0, for one wave.
// CAUSAL: key <= query.  NFULL: key tiles [0, NFULL) are known to lie entirely below nk and need no mask (non-causal only).
// TAIL: the sequence is 16*NKT + 1 keys; the MFMA tiles cover the first 16*NKT and the last key is a rank-1 VALU update
// (its score from the lane's 16 query dims + a reduction over the four lanes of the query, its P.V term 16 FMAs per tile)
// instead of two more key tiles of which 31 of 32 columns would be padding.
// MX: the store tests cx.q8 at run time; without it the q8 / s8 / q8_rows / row0 / col0 fields are never read.
template <typename T, int NKT, bool CAUSAL, int NFULL, int NQ, bool TAIL, bool MX>
__device__ __forceinline__ void attn_tiles(const AttnCtx<T>& cx, int q0) {
    using C = AttnCfg<NKT>;
    using V8 = typename Ev<T>::v8;
    using V4 = typename Ev<T>::v4;
    const int g = cx.g, c = cx.c;
    const float sl2 = 0.125f * 1.4426950408889634f;  // 1/sqrt(64) * log2(e)
    int qidx[NQ];
    V8 qf[NQ][2];
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
        qidx[t] = q0 + t * 16 + c;
        const int qrow = qidx[t] < cx.nq ? qidx[t] : cx.nq - 1;
        const T* qp = cx.q + (size_t)qrow * cx.q_ld + 8 * g;
        qf[t][0] = *reinterpret_cast<const V8*>(qp);
        qf[t][1] = *reinterpret_cast<const V8*>(qp + 32);
    }
    // ---- S^T tiles
    f32x4 sc[NQ][NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
        const int key = kt * 16 + c;
        const char* kr = cx.k_lds + key * 128;
        const int f = (key >> 1) & 7;
        const V8 a0 = *reinterpret_cast<const V8*>(kr + ((g ^ f) << 4));
        const V8 a1 = *reinterpret_cast<const V8*>(kr + (((4 + g) ^ f) << 4));
#pragma unroll
        for (int t = 0; t < NQ; ++t) {
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
            acc = mfma16(a0, qf[t][0], acc, 0, 0, 0);
            acc = mfma16(a1, qf[t][1], acc, 0, 0, 0);
            sc[t][kt] = acc;
        }
        if (kt % 3 == 2) __builtin_amdgcn_sched_barrier(0);   // bound how far LDS reads are hoisted (VGPR pressure)
    }
    // ---- TAIL: score of the last key for the lane's query (replicated over the four g lanes after the reduction)
    [[maybe_unused]] float tsc[NQ];
    if constexpr (TAIL) {
        const V8 k0 = *reinterpret_cast<const V8*>(cx.tail + g * 16);
        const V8 k1 = *reinterpret_cast<const V8*>(cx.tail + (4 + g) * 16);
#pragma unroll
        for (int t = 0; t < NQ; ++t) {
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) a += (float)qf[t][0][j] * (float)k0[j] + (float)qf[t][1][j] * (float)k1[j];
            tsc[t] = rows_sum(a);
        }
    }
    // ---- mask, row max, exp, row sum (lane holds query qidx[t], keys kt*16 + 4g + r)
    float inv[NQ];
    [[maybe_unused]] float tp[NQ];
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = sc[t][kt][r];
                if (CAUSAL || kt >= NFULL) {      // resolved at compile time once the kt loop is unrolled
                    const int kidx = kt * 16 + 4 * g + r;
                    const bool ok = kidx < cx.nk && (!CAUSAL || kidx <= qidx[t]);
                    v = ok ? v : -INFINITY;
                    sc[t][kt][r] = v;
                }
                mx = fmaxf(mx, v);
            }
        mx = rows_max(mx);                        // key 0 is always below nk and never above the query: finite
        if constexpr (TAIL) mx = fmaxf(mx, tsc[t]);
        const float nmx = -mx * sl2;
        // packed fp32 math (v_pk_fma_f32 / v_pk_add_f32: two elements per VALU issue); v_exp_f32 stays per element
        const f32x2 vs = f32x2{sl2, sl2}, vn = f32x2{nmx, nmx};
        f32x2 vsum = f32x2{0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                f32x2 e = f32x2{sc[t][kt][2 * hh], sc[t][kt][2 * hh + 1]};
                e = pk_fma(e, vs, vn);
                e[0] = __builtin_amdgcn_exp2f(e[0]);   // exp2(-inf) = 0
                e[1] = __builtin_amdgcn_exp2f(e[1]);
                sc[t][kt][2 * hh] = e[0];
                sc[t][kt][2 * hh + 1] = e[1];
                vsum += e;
            }
        }
        float sum = vsum[0] + vsum[1];
        sum = rows_sum(sum);
        if constexpr (TAIL) {
            const float e = __builtin_amdgcn_exp2f(tsc[t] * sl2 + nmx);
            sum += e;
            tp[t] = (float)(T)e;             // rounded to T like the probabilities the MFMA path multiplies
        }
        inv[t] = 1.0f / sum;
    }
    // ---- O^T = V^T . P^T
    f32x4 o[NQ][4];
#pragma unroll
    for (int t = 0; t < NQ; ++t)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < NKT / 2; ++u) {
        V8 pf[NQ];
#pragma unroll
        for (int t = 0; t < NQ; ++t) {
            const f32x4 p0 = sc[t][2 * u], p1 = sc[t][2 * u + 1];
            pf[t] = V8{(T)p0[0], (T)p0[1], (T)p0[2], (T)p0[3],
                           (T)p1[0], (T)p1[1], (T)p1[2], (T)p1[3]};
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const V8 a = *reinterpret_cast<const V8*>(cx.vt_lds + (dt * 16 + c) * C::VT_ROW + (4 * u + g) * 16);
#pragma unroll
            for (int t = 0; t < NQ; ++t) o[t][dt] = mfma16(a, pf[t], o[t][dt], 0, 0, 0);
        }
        if (u % 3 == 2) __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (TAIL) {      // + p_last * V[last key][16 dt + 4 g + r]
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const V4 v = *reinterpret_cast<const V4*>(cx.tail + 128 + (16 * dt + 4 * g) * 2);
#pragma unroll
            for (int t = 0; t < NQ; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[t][dt][r] += tp[t] * (float)v[r];
        }
    }
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
        if (qidx[t] < cx.q_limit) {
            [[maybe_unused]] const int row = cx.row0 + qidx[t];
            if (MX && cx.q8 && row < cx.q8_rows) {
                // lane (g, c): head columns 16*dt + 4g + r; a 32-column MX block = dt in {2b, 2b+1} over the four g lanes
#pragma unroll
                for (int b2 = 0; b2 < 2; ++b2) {
                    const f32x4 v0 = o[t][2 * b2] * inv[t], v1 = o[t][2 * b2 + 1] * inv[t];
                    const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                    float amax = 0.f;
#pragma unroll
                    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
                    amax = rows_max(amax);
                    const int e = mx_block_exp(amax);
                    const uint2 pk = mx_pack8(v, e);
                    unsigned char* qp = cx.q8 + (size_t)row * cx.o_ld + cx.col0 + 32 * b2 + 4 * g;
                    *reinterpret_cast<unsigned*>(qp) = pk.x;
                    *reinterpret_cast<unsigned*>(qp + 16) = pk.y;
                    if (g == 0) cx.s8[mx_scale_index((cx.col0 >> 5) + b2, row, cx.q8_rows)] = (unsigned char)(e + 127);
                }
            } else {
                T* op = cx.out + (size_t)qidx[t] * cx.o_ld + 4 * g;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const f32x4 v = o[t][dt] * inv[t];
                    *reinterpret_cast<V4*>(op + dt * 16) = V4{(T)v[0], (T)v[1], (T)v[2], (T)v[3]};
                }
            }
        }
    }
}

}  // namespace
