// The fp32-ACCURATE operating point of the encoder path (CLIP.set_precision("fp32"), keds_tower_params.f32 = 1).
//
// The reference evaluates in fp32 (src/eval_retrieval.py:108-109, `--precision` src/params.py:227-232: the default `amp`
// converts the model to fp32 and no autocast is entered in eval), and north_star asks for Recall@k EQUAL to that path.  The
// default flow of this library rounds GEMM operands to bf16 / fp16 and differs from the reference by a
// few 1e-3 in the embeddings -- enough to flip a (query, k) outcome the reference itself decides by a margin below 5e-4.  This
// file is the flow without operand rounding: every product runs on the f32-input matrix instruction
// (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate = an fmaf chain, cdna_hip_programming.md section 3), the
// residual stream, the LayerNorm output, q / k / v, the attention probabilities and the MLP hidden layer all stay fp32.
// Throughput is secondary here (the f32 matrix rate is 1/16 of the bf16 one): simple tiles, no side lane, no fused LayerNorm.
// The tower passes of this flow and of the fp32x3 one (f32 = 2) are planned in tower_plan.h and run by towers.hip like every other.
//
//   gemm_f32_kernel       out[M,N] = epilogue(X[M,K] . W[N,K]^T + bias)      model.py:309-326 (in/out projections, MLP), :381 (conv1)
//   attention_f32_kernel  softmax(q k^T / 8 [+ causal mask]) v per (sample, head) model.py:319-321, nn.MultiheadAttention
//   im2col_f32            patch rows of the conv1-as-GEMM                     model.py:394-398
#include "keds_common.h"
#include <math.h>

namespace {

namespace g32 {
constexpr int TM = 128, TN = 128, TK = 16;
constexpr int LD = TM + 4;            // k-major LDS image [TK][LD]: fragment reads are consecutive dwords (conflict free)
}  // namespace g32

enum { F32_EPI_BIAS = 0, F32_EPI_QGELU = 1, F32_EPI_RESID = 2, F32_EPI_RELU = 3, F32_EPI_PATCH = 4 };

// 128 x 128 x 16 tile, 4 waves (2 x 2), each wave 64 (n) x 64 (m) = 2 x 2 tiles of v_mfma_f32_32x32x2_f32.  W is the MFMA A
// operand and X the B operand (as in gemm.hip): the accumulator then holds, per lane, ONE output row m and runs of four
// consecutive n -> 16-byte stores.  Operand tiles go HBM -> registers -> LDS transposed to k-major ([k][row]: lane l of an
// MFMA reads element (k = 2 kk + (l >> 5), row = l & 31), i.e. 32 consecutive dwords per half wave), register-prefetched
// one K-tile ahead, two LDS buffers, one barrier per K-tile.
template <int EPI>
__global__ __launch_bounds__(256) void gemm_f32_kernel(const float* __restrict__ X, long long lda, const float* __restrict__ W,
                                                       const float* __restrict__ bias, float* __restrict__ out, long long ldc,
                                                       int M, int N, int K, const float* __restrict__ aux, int aux_i) {
    using namespace g32;
    __shared__ float sX[2][TK * LD];
    __shared__ float sW[2][TK * LD];
    const int n_tiles = N / TN;
    const int tm = blockIdx.x / n_tiles, tn = blockIdx.x - tm * n_tiles;       // n fastest: neighbours share their X rows
    const int m0 = tm * TM, n0 = tn * TN;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int r = t >> 2, kq = t & 3;                                           // staging: rows r, r + 64; k quarter kq
    const float* xp[2];
    const float* wp[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int m = m0 + r + 64 * i;
        m = m < M ? m : M - 1;                                                  // ragged last row tile: rows clamped, not stored
        xp[i] = X + (size_t)m * lda + 4 * kq;
        wp[i] = W + (size_t)(n0 + r + 64 * i) * K + 4 * kq;
    }
    f32x4 xr[2], wr[2];
    auto load = [&](int kt) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            xr[i] = *reinterpret_cast<const f32x4*>(xp[i] + kt * TK);
            wr[i] = *reinterpret_cast<const f32x4*>(wp[i] + kt * TK);
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sX[buf][(4 * kq + j) * LD + r + 64 * i] = xr[i][j];
                sW[buf][(4 * kq + j) * LD + r + 64 * i] = wr[i][j];
            }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const int nk = K / TK;
    const int h = lane >> 5, c = lane & 31;
    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load(kt + 1);
#pragma unroll
        for (int kk = 0; kk < TK / 2; ++kk) {
            const float* ws = sW[buf] + (2 * kk + h) * LD + 64 * wn + c;
            const float* xs = sX[buf] + (2 * kk + h) * LD + 64 * wm + c;
            const float a0 = ws[0], a1 = ws[32], b0 = xs[0], b1 = xs[32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (kt + 1 < nk) store(buf ^ 1);
        __syncthreads();
    }
    // C/D map of the 32 x 32 forms: column (here: m) = lane & 31, row (here: n) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int m = m0 + 64 * wm + 32 * j + c;
        if (m >= M) continue;
        size_t orow = (size_t)m;
        const float* pos = nullptr;
        if constexpr (EPI == F32_EPI_PATCH) {                                    // token row (m / G) (G + 1) + 1 + m % G, + positional embedding
            const int G = aux_i, b = m / G, pidx = m - b * G;
            orow = (size_t)b * (G + 1) + 1 + pidx;
            pos = aux + (size_t)(1 + pidx) * N;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = n0 + 64 * wn + 32 * i + 8 * g + 4 * h;
                f32x4 v = f32x4{acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                if (bias) v = v + *reinterpret_cast<const f32x4*>(bias + n);
                float* o = out + orow * ldc + n;
                if constexpr (EPI == F32_EPI_QGELU) {                            // x * sigmoid(1.702 x), model.py:300-302
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = v[e] / (1.0f + expf(-1.702f * v[e]));
                }
                if constexpr (EPI == F32_EPI_RELU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                if constexpr (EPI == F32_EPI_RESID) v = v + *reinterpret_cast<const f32x4*>(o);
                if constexpr (EPI == F32_EPI_PATCH) v = v + *reinterpret_cast<const f32x4*>(pos + n);
                *reinterpret_cast<f32x4*>(o) = v;
            }
    }
}

// One workgroup (9 waves) per (sample, head), both products on the f32-input matrix instruction.  K (row stride 65 floats:
// lane i reads key row i conflict free) and V live in LDS as fp32, zero padded to whole 32-key tiles; a wave owns 32-query
// tiles qt = wave, wave + 9, ... (S = 257: nine tiles, one per wave) and walks the key tiles with an online softmax:
//   S^T tile  = K tile . Q^T   32 MFMAs 32x32x2: A[i = key][k] = K[key][2 kk + h], B[k][j = query] = q[query][2 kk + h] / 8
//               (the lane's 32 q values sit in registers); result: lane = query j, register r = key (r & 3) + 8 (r >> 2) + 4 h
//   p = exp(s - m_new), running maximum m (combined over the two lane halves), running sum l (per half, combined at the end),
//               O rescaled by exp(m - m_new)
//   O^T tile += V^T tile . P^T  16 + 16 MFMAs: step r takes the key PAIR {key_0(r), key_1(r)} the two lane halves hold in
//               register r -- B[k = h][j] is the lane's own p[r], A[i = dim][k = h] = V[key_h(r)][dim] -- so the probabilities
//               go from the score accumulator into the next product without leaving their registers
// expf / division in full precision.  (The first version kept the scores of one key per lane and broadcast with v_readlane:
// 4.4 ms per ViT-L/14 layer at B = 128, 37 % of the fp32 step; this one ~0.4 ms.)  S <= 288.
constexpr int A32_WAVES = 9;
__global__ __launch_bounds__(64 * A32_WAVES) void attention_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out, int S,
                                                                        int heads, int causal, int q_limit,
                                                                        const int* __restrict__ seq_off) {
    extern __shared__ __attribute__((aligned(16))) float a32_lds[];
    // packed rows (towers.hip PackedRows): sample b owns rows [seq_off[b], seq_off[b + 1]); S (the longest sample: it sized the LDS)
    // becomes the sample's own length
    long long row_base = (long long)(blockIdx.x / heads) * S;
    if (seq_off) {
        row_base = seq_off[blockIdx.x / heads];
        S = seq_off[blockIdx.x / heads + 1] - (int)row_base;
        q_limit = q_limit < S ? q_limit : S;
    }
    const int nkt = (S + 31) >> 5, SP = nkt * 32;
    float* Ks = a32_lds;                           // [SP][65]
    float* Vs = a32_lds + (size_t)SP * 65;         // [SP][64]
    const int b = blockIdx.x / heads, hd = blockIdx.x - b * heads;
    const int d = heads * 64, ld = 3 * d;
    const float* base = qkv + (size_t)row_base * ld + hd * 64;
    for (int idx = threadIdx.x; idx < SP * 16; idx += 64 * A32_WAVES) {
        const int row = idx >> 4, c4 = idx & 15;
        f32x4 kv = f32x4{0.f, 0.f, 0.f, 0.f}, vv = kv;
        if (row < S) {
            kv = *reinterpret_cast<const f32x4*>(base + (size_t)row * ld + d + 4 * c4);
            vv = *reinterpret_cast<const f32x4*>(base + (size_t)row * ld + 2 * d + 4 * c4);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            Ks[row * 65 + 4 * c4 + e] = kv[e];
            Vs[row * 64 + 4 * c4 + e] = vv[e];
        }
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = lane & 31, hh = lane >> 5;
    const int nq = q_limit < S ? q_limit : S;
    const int nqt = (nq + 31) >> 5;
    for (int qt = wave; qt < nqt; qt += A32_WAVES) {
        const int q = qt * 32 + j;
        const float* qrow = base + (size_t)(q < S ? q : S - 1) * ld + hh;
        float qreg[32];
#pragma unroll
        for (int kk = 0; kk < 32; ++kk) qreg[kk] = qrow[2 * kk] * 0.125f;          // 1 / sqrt(64): exact scaling
        float m = -INFINITY, l = 0.f;
        f32x16 o0, o1;
#pragma unroll
        for (int e = 0; e < 16; ++e) o0[e] = 0.f, o1[e] = 0.f;
        int kt_end = nkt;
        if (causal) {                                                            // key tiles that hold a key <= the tile's last query
            const int lastq = qt * 32 + 31;
            kt_end = (lastq >> 5) + 1 < nkt ? (lastq >> 5) + 1 : nkt;
        }
        for (int kt = 0; kt < kt_end; ++kt) {
            f32x16 sc;
#pragma unroll
            for (int e = 0; e < 16; ++e) sc[e] = 0.f;
            const float* kr = Ks + (size_t)(kt * 32 + j) * 65 + hh;
#pragma unroll
            for (int kk = 0; kk < 32; ++kk) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[2 * kk], qreg[kk], sc, 0, 0, 0);
            float tmax = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                const bool valid = key < S && (!causal || key <= q);
                sc[r] = valid ? sc[r] : -INFINITY;
                tmax = fmaxf(tmax, sc[r]);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float mnew = fmaxf(m, tmax);
            const float resc = m == -INFINITY ? 0.f : expf(m - mnew);           // (first tile, or nothing valid so far)
            float psum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sc[r] = mnew == -INFINITY ? 0.f : expf(sc[r] - mnew);           // masked keys: exp(-inf) = 0
                psum += sc[r];
            }
            l = l * resc + psum;
#pragma unroll
            for (int e = 0; e < 16; ++e) o0[e] *= resc, o1[e] *= resc;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* vr = Vs + (size_t)(kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh) * 64 + j;
                o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[0], sc[r], o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[32], sc[r], o1, 0, 0, 0);
            }
            m = mnew;
        }
        const float ltot = l + __shfl_xor(l, 32, 64);
        if (q < nq) {                                                            // lane = query q; register r = dim (r & 3) + 8 (r >> 2) + 4 h
            float* orow = out + ((size_t)row_base + q) * d + hd * 64 + 4 * hh;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                *reinterpret_cast<f32x4*>(orow + 8 * g) = f32x4{o0[4 * g] / ltot, o0[4 * g + 1] / ltot, o0[4 * g + 2] / ltot, o0[4 * g + 3] / ltot};
                *reinterpret_cast<f32x4*>(orow + 32 + 8 * g) = f32x4{o1[4 * g] / ltot, o1[4 * g + 1] / ltot, o1[4 * g + 2] / ltot, o1[4 * g + 3] / ltot};
            }
        }
    }
}

// one block per output row (b, patch); columns c*P*P + ky*P + kx, zero padded to Kpad (elementwise.hip's im2col in fp32)
__global__ __launch_bounds__(256) void im2col_f32_kernel(const float* __restrict__ img, float* __restrict__ out, int R, int P,
                                                         int Kpad) {
    const int g = R / P;
    const int row = blockIdx.x;
    const int b = row / (g * g), pi = row % (g * g);
    const int py = pi / g, px = pi % g;
    const int kreal = 3 * P * P;
    const float* base = img + (size_t)b * 3 * R * R;
    for (int k = threadIdx.x; k < Kpad; k += 256) {
        float v = 0.f;
        if (k < kreal) {
            const int ch = k / (P * P), rem = k % (P * P);
            const int ky = rem / P, kx = rem % P;
            v = base[(size_t)ch * R * R + (size_t)(py * P + ky) * R + px * P + kx];
        }
        out[(size_t)row * Kpad + k] = v;
    }
}

__global__ void l2norm_rows_f32_kernel(float* __restrict__ x, int rows, int dim) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= rows) return;
    float* p = x + (size_t)r * dim;
    float s = 0.f;
    for (int i = lane; i < dim; i += 64) s = fmaf(p[i], p[i], s);
    s = wave_sum(s);
    const float nrm = sqrtf(s);                   // x / x.norm(dim=-1, keepdim=True), eval_utils.py:162,704-710
    for (int i = lane; i < dim; i += 64) p[i] = p[i] / nrm;
}

template <int EPI>
int launch_gemm_f32(const float* A, long long lda, const float* W, const float* bias, float* out, long long ldc, int M, int N,
                    int K, const float* aux, int aux_i, hipStream_t st) {
    const int tiles = ((M + g32::TM - 1) / g32::TM) * (N / g32::TN);
    KedsProfScope prof(KEDS_PROF_GEMM, st);
    prof.work(2.0 * M * N * (double)K);
    gemm_f32_kernel<EPI><<<tiles, 256, 0, st>>>(A, lda, W, bias, out, ldc, M, N, K, aux, aux_i);
    return keds_check_launch("gemm_f32_kernel");
}

}  // namespace

extern "C" int keds_gemm_f32(const float* A, int64_t lda, const float* W, const float* bias, float* out, int64_t ldc, int M,
                             int N, int K, int epilogue, const float* aux, int aux_i, void* stream) {
    KEDS_REQUIRE(A && W && out && M > 0, "keds_gemm_f32: bad argument");
    KEDS_REQUIRE(N > 0 && N % 128 == 0 && K > 0 && K % 16 == 0, "keds_gemm_f32: N must be a multiple of 128 and K of 16 (got N=%d K=%d)", N, K);
    KEDS_REQUIRE(lda >= K && lda % 4 == 0 && ldc % 4 == 0, "keds_gemm_f32: row strides must be multiples of 4 floats");
    KEDS_REQUIRE(epilogue != F32_EPI_PATCH || (aux && aux_i > 0), "keds_gemm_f32: the patch epilogue needs the positional embedding and G");
    hipStream_t st = (hipStream_t)stream;
    switch (epilogue) {
        case F32_EPI_BIAS: return launch_gemm_f32<F32_EPI_BIAS>(A, lda, W, bias, out, ldc, M, N, K, aux, aux_i, st);
        case F32_EPI_QGELU: return launch_gemm_f32<F32_EPI_QGELU>(A, lda, W, bias, out, ldc, M, N, K, aux, aux_i, st);
        case F32_EPI_RESID: return launch_gemm_f32<F32_EPI_RESID>(A, lda, W, bias, out, ldc, M, N, K, aux, aux_i, st);
        case F32_EPI_RELU: return launch_gemm_f32<F32_EPI_RELU>(A, lda, W, bias, out, ldc, M, N, K, aux, aux_i, st);
        case F32_EPI_PATCH: return launch_gemm_f32<F32_EPI_PATCH>(A, lda, W, bias, out, ldc, M, N, K, aux, aux_i, st);
    }
    keds_set_error("keds_gemm_f32: unknown epilogue %d", epilogue);
    return KEDS_E_ARG;
}

// (seq_off: packed rows or null; what the tower passes launch, towers.hip)
extern "C" int keds_attention_f32(const float* qkv, float* out, int B, int S, int heads, int causal, int q_limit, void* stream) {
    return attention_f32_impl(qkv, out, B, S, heads, causal, q_limit, nullptr, stream);
}
int attention_f32_impl(const float* qkv, float* out, int B, int S, int heads, int causal, int q_limit, const int32_t* seq_off, void* stream) {
    KEDS_REQUIRE(qkv && out && B > 0 && heads > 0, "keds_attention_f32: bad argument");
    KEDS_REQUIRE(S >= 1 && S <= 288, "keds_attention_f32: S must be in [1, 288] (got %d)", S);
    const int lds = ((S + 31) / 32 * 32) * (65 + 64) * (int)sizeof(float);           // K and V padded to whole 32-key tiles
    int rc = keds_func_lds_once((const void*)attention_f32_kernel, lds, "attention_f32_kernel");
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    KedsProfScope prof(KEDS_PROF_ATTN, st);
    attention_f32_kernel<<<B * heads, 64 * A32_WAVES, lds, st>>>(qkv, out, S, heads, causal, q_limit > 0 ? q_limit : S, seq_off);
    return keds_check_launch("attention_f32_kernel");
}

// packed rows one call at a time (tests/test_gpu_tower_compositions.py): the launch helper the fp32 tower pass uses
extern "C" int keds_attention_f32_packed(const float* qkv, float* out, int B, int s_max, const int32_t* seq_off, int heads, int causal,
                                         void* stream) {
    KEDS_REQUIRE(qkv && out && seq_off && B > 0 && heads > 0, "keds_attention_f32_packed: bad argument");
    KEDS_REQUIRE(s_max >= 1 && s_max <= 288, "keds_attention_f32_packed: s_max=%d unsupported (1..288)", s_max);
    return attention_f32_impl(qkv, out, B, s_max, heads, causal, s_max, seq_off, stream);
}

extern "C" int keds_im2col_f32(const float* image, float* out, int B, int R, int P, int Kpad, void* stream) {
    KEDS_REQUIRE(image && out && B > 0 && P > 0 && R % P == 0, "keds_im2col_f32: bad argument");
    KEDS_REQUIRE(Kpad >= 3 * P * P && Kpad % 16 == 0, "keds_im2col_f32: Kpad must cover 3*P*P and be a multiple of 16");
    const int g = R / P;
    KedsProfScope prof(KEDS_PROF_OTHER, (hipStream_t)stream);
    im2col_f32_kernel<<<B * g * g, 256, 0, (hipStream_t)stream>>>(image, out, R, P, Kpad);
    return keds_check_launch("im2col_f32_kernel");
}

// ---- read-out (tower_plan.h says what the passes launch, towers.hip runs it): the L2 normalisation of the fp32 flows, in place
int keds_l2norm_rows_f32_impl(float* x, int rows, int dim, hipStream_t st) {
    l2norm_rows_f32_kernel<<<(rows + 3) / 4, 256, 0, st>>>(x, rows, dim);
    return keds_check_launch("l2norm_rows_f32_kernel");
}

// ---- knowledge injection in fp32 (IM2TEXT + 2 x CrossFormer, model.py:37-123, eval_utils.py:661-672): the core; the host chain
// that runs it and keds_gemm_f32 is keds_knowledge_run_f32 (knowledge.hip) ----------------------------------------------------
namespace {
// single-query cross-attention core (model.py:56-79) on projected fp32 rows: one wave per (sample, head), lane = dim of the
// 64-wide head; Q [B, inner], Kp / Vp [B*K, inner] -> out [B, inner]; K <= 64
__global__ __launch_bounds__(256) void cross_core_f32_kernel(const float* __restrict__ Q, const float* __restrict__ Kp,
                                                             const float* __restrict__ Vp, float* __restrict__ out, int B, int K,
                                                             int heads) {
    const int wid = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wid >= B * heads) return;
    const int b = wid / heads, h = wid - b * heads, inner = heads * 64;
    const float q = Q[(size_t)b * inner + h * 64 + lane] * 0.125f;           // dim_head ** -0.5, exact
    // one pass with a running maximum (K <= 64 keys: the rescales are exact to rounding, results within 1e-7 of the two-pass form)
    float mx = -INFINITY, sum = 0.f, o = 0.f;
    for (int j = 0; j < K; ++j) {
        const float sj = wave_sum(q * Kp[((size_t)b * K + j) * inner + h * 64 + lane]);
        if (sj > mx) {                                                       // (wave-uniform)
            const float sc = expf(mx - sj);                                  // 0 on the first key
            sum *= sc;
            o *= sc;
            mx = sj;
        }
        const float e = expf(sj - mx);
        sum += e;
        o = fmaf(e, Vp[((size_t)b * K + j) * inner + h * 64 + lane], o);
    }
    out[(size_t)b * inner + h * 64 + lane] = o / sum;
}

}  // namespace

int keds_cross_core_f32_impl(const float* Q, const float* Kp, const float* Vp, float* out, int B, int K, int heads, hipStream_t st) {
    cross_core_f32_kernel<<<(B * heads + 3) / 4, 256, 0, st>>>(Q, Kp, Vp, out, B, K, heads);
    return keds_check_launch("cross_core_f32_kernel");
}

extern "C" int keds_cross_core_f32(const float* Q, const float* Kp, const float* Vp, float* out, int B, int K, int heads, void* stream) {
    KEDS_REQUIRE(Q && Kp && Vp && out && B > 0 && heads >= 1, "keds_cross_core_f32: bad argument");
    KEDS_REQUIRE(K >= 1 && K <= 64, "keds_cross_core_f32: K=%d must be in [1,64]", K);
    return keds_cross_core_f32_impl(Q, Kp, Vp, out, B, K, heads, (hipStream_t)stream);
}
