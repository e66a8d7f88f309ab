// How exactly does ONE v_mfma_scale_f32_16x16x128_f8f6f4 (fp8 x fp8) add its 128 block-scaled products and the accumulator?
// Every product e4m3 x e4m3 x 2^(sa + sb) is exact in fp32; the question is the multi-term adder.  Against a float64 sum on the host:
//   part 1, cut-off series: a term of 1.0 beside smaller terms of 2^-j -- one product in another 32-block; the accumulator; 96 products
//           in the other three blocks; the same beside an accumulator of 1 -- printed as the share of the small terms that arrives;
//   part 2, random data: Gaussian e4m3 operands under equal / ramped / jumping block scales, with a zero, a comparable and a dominant
//           accumulator: the largest |D - ref| in units of 2^-24 S (S = sum of |products| + |C|: what tests/gemm_check.py's e_acc is
//           written in, C_ACC * 128 per instruction), of 2^-24 max|term| and of 2^-24 |ref|.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// case cs: A, B bytes [16][128], sA, sB scale bytes [16][4] (block b of row r), C, D fp32 [16][16] (D[i][j] = sum_k A[i][k] B[j][k] + C[i][j])
__global__ void probe(const unsigned char* A, const unsigned char* B, const unsigned char* sA, const unsigned char* sB, const float* C, float* D) {
    const int cs = blockIdx.x, l = threadIdx.x, r = l & 15, g = l >> 4;
    A += cs * 2048; B += cs * 2048; sA += cs * 64; sB += cs * 64; C += cs * 256; D += cs * 256;
    union { i32x8 v; unsigned char b[32]; } a, b;
    for (int j = 0; j < 16; ++j) {
        a.b[j] = A[r * 128 + 16 * g + j]; a.b[16 + j] = A[r * 128 + 64 + 16 * g + j];
        b.b[j] = B[r * 128 + 16 * g + j]; b.b[16 + j] = B[r * 128 + 64 + 16 * g + j];
    }
    const int sa = sA[r * 4 + g], sb = sB[r * 4 + g];          // from memory: a literal scale operand is mis-read
    f32x4 c;
    for (int i = 0; i < 4; ++i) c[i] = C[(4 * g + i) * 16 + r];
    c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a.v, b.v, c, 0, 0, 0, sa, 0, sb);
    for (int i = 0; i < 4; ++i) D[(4 * g + i) * 16 + r] = c[i];
}

static double dec(unsigned char q) {
    const int s = q >> 7, e = (q >> 3) & 15, m = q & 7;
    const double v = e == 0 ? m * std::ldexp(1.0, -9) : (1.0 + m / 8.0) * std::ldexp(1.0, e - 7);
    return s ? -v : v;
}
static unsigned char enc(double x) {                              // nearest e4m3 (ties to even), saturating; for building data only
    unsigned char best = 0;
    double bd = 1e300;
    for (int q = 0; q < 256; ++q) {
        if ((q & 0x7F) == 0x7F) continue;
        const double d = std::fabs(dec((unsigned char)q) - x);
        if (d < bd || (d == bd && !(q & 1))) { bd = d; best = (unsigned char)q; }
    }
    return best;
}

struct Batch {
    std::vector<unsigned char> A, B, sA, sB;
    std::vector<float> C, D;
    int n = 0;
    int add() {
        A.resize((n + 1) * 2048, 0); B.resize((n + 1) * 2048, 0); sA.resize((n + 1) * 64, 127); sB.resize((n + 1) * 64, 127);
        C.resize((n + 1) * 256, 0.f);
        return n++;
    }
    void run() {
        unsigned char *dA, *dB, *dsA, *dsB; float *dC, *dD;
        D.assign(n * 256, 0.f);
        hipMalloc(&dA, A.size()); hipMalloc(&dB, B.size()); hipMalloc(&dsA, sA.size()); hipMalloc(&dsB, sB.size());
        hipMalloc(&dC, C.size() * 4); hipMalloc(&dD, D.size() * 4);
        hipMemcpy(dA, A.data(), A.size(), hipMemcpyHostToDevice); hipMemcpy(dB, B.data(), B.size(), hipMemcpyHostToDevice);
        hipMemcpy(dsA, sA.data(), sA.size(), hipMemcpyHostToDevice); hipMemcpy(dsB, sB.data(), sB.size(), hipMemcpyHostToDevice);
        hipMemcpy(dC, C.data(), C.size() * 4, hipMemcpyHostToDevice);
        probe<<<n, 64>>>(dA, dB, dsA, dsB, dC, dD);
        if (hipMemcpy(D.data(), dD, D.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("device error\n"); std::exit(2); }
        hipFree(dA); hipFree(dB); hipFree(dsA); hipFree(dsB); hipFree(dC); hipFree(dD);
    }
    // float64 reference of D[i][j] of case cs, with S = sum |terms| + |C| and the largest |term|
    void ref(int cs, int i, int j, double& sum, double& S, double& mx) const {
        sum = C[cs * 256 + i * 16 + j]; S = std::fabs(sum); mx = S;
        for (int k = 0; k < 128; ++k) {
            const double t = dec(A[cs * 2048 + i * 128 + k]) * dec(B[cs * 2048 + j * 128 + k]) *
                             std::ldexp(1.0, (int)sA[cs * 64 + i * 4 + k / 32] + (int)sB[cs * 64 + j * 4 + k / 32] - 254);
            sum += t; S += std::fabs(t); mx = std::fmax(mx, std::fabs(t));
        }
    }
};

int main() {
    const unsigned char ONE = 0x38;
    // ---- part 1: output (0, 0) of each case; rows / columns other than 0 stay zero
    const int JMAX = 40;
    Batch b1;
    for (int kind = 0; kind < 5; ++kind)
        for (int j = 0; j <= JMAX; ++j) {
            const int cs = b1.add();
            unsigned char* A = &b1.A[cs * 2048]; unsigned char* B = &b1.B[cs * 2048];
            auto small_blocks = [&](int first_k, int count) {       // `count` products of 2^-j from k = first_k on (blocks 1..3: scale 2^-j on A)
                for (int k = first_k; k < first_k + count; ++k) { A[k] = ONE; B[k] = ONE; }
                for (int blk = 1; blk < 4; ++blk) b1.sA[cs * 64 + blk] = (unsigned char)(127 - j);
            };
            if (kind == 0) { A[0] = ONE; B[0] = ONE; small_blocks(32, 1); }                       // 1 + one product of 2^-j in block 1
            if (kind == 1) { b1.C[cs * 256] = 1.f; small_blocks(32, 1); }                          // C = 1 + one product of 2^-j
            if (kind == 2) { b1.C[cs * 256] = std::ldexp(1.f, -j); A[0] = ONE; B[0] = ONE; }        // C = 2^-j + a product of 1
            if (kind == 3) { A[0] = ONE; B[0] = ONE; small_blocks(32, 96); }                      // 1 + 96 products of 2^-j
            if (kind == 4) { b1.C[cs * 256] = 1.f; small_blocks(32, 96); }                         // C = 1 + 96 products of 2^-j
        }
    b1.run();
    const char* names[5] = {"product 1 + ONE product 2^-j (another block)", "C = 1 + ONE product 2^-j", "C = 2^-j + a product of 1",
                            "product 1 + 96 products 2^-j (three blocks)", "C = 1 + 96 products 2^-j"};
    for (int kind = 0; kind < 5; ++kind) {
        printf("%s: (D - 1) / (small terms), j = 0 .. %d; a correctly rounded sum of the exact terms gives 1 while the small terms reach 2^-24\n ", names[kind], JMAX);
        for (int j = 0; j <= JMAX; ++j) {
            const double small = (kind >= 3 ? 96.0 : 1.0) * std::ldexp(1.0, -j);
            printf(" %d:%.4g", j, ((double)b1.D[(kind * (JMAX + 1) + j) * 256] - 1.0) / small);
        }
        printf("\n");
    }
    // ---- part 1b: the same inside ONE scale: a product of 2^16 (256 x 256) at k = 0 beside products of 2^(16 - j) made of the ELEMENTS'
    // own exponents (all scales 2^0), at k = 1 (the same dword) | k = 16 (the same block, another lane) | k = 64 (the same lane's
    // second half, block 2) | k = 1 .. 31 (the rest of the block) | k = 1 .. 127 | k = 1 with a negative sign
    auto pow2_byte = [](int x) { return (unsigned char)(x >= -6 ? (x + 7) << 3 : 1 << (x + 9)); };       // 2^x, x in [-9, 8]
    const int J2 = 34;
    Batch b2;
    for (int kind = 0; kind < 6; ++kind)
        for (int j = 0; j <= J2; ++j) {
            const int cs = b2.add();
            unsigned char* A = &b2.A[cs * 2048]; unsigned char* B = &b2.B[cs * 2048];
            A[0] = B[0] = pow2_byte(8);
            const int x = 16 - j, xa = x >= 0 ? (x + 1) / 2 : -((-x) / 2), xb = x - xa;
            const int k0 = kind == 1 ? 16 : kind == 2 ? 64 : 1, k1 = kind == 3 ? 32 : kind == 4 ? 128 : k0 + 1;
            for (int k = k0; k < k1; ++k) { A[k] = pow2_byte(xa); B[k] = (unsigned char)(pow2_byte(xb) | (kind == 5 ? 0x80 : 0)); }
        }
    b2.run();
    const char* names2[6] = {"k = 1", "k = 16", "k = 64", "k = 1 .. 31", "k = 1 .. 127", "k = 1, negative"};
    for (int kind = 0; kind < 6; ++kind) {
        printf("product 2^16 + products 2^(16 - j) at %s, one scale: (D - 2^16) / (small terms), j = 0 .. %d\n ", names2[kind], J2);
        for (int j = 0; j <= J2; ++j) {
            const double small = (kind == 3 ? 31.0 : kind == 4 ? 127.0 : kind == 5 ? -1.0 : 1.0) * std::ldexp(1.0, 16 - j);
            printf(" %d:%.4g", j, ((double)b2.D[(kind * (J2 + 1) + j) * 256] - 65536.0) / small);
        }
        printf("\n");
    }
    // ---- part 2: random data
    std::mt19937 rng(12345);
    std::normal_distribution<double> gauss(0.0, 1.0);
    std::vector<unsigned char> pool(1 << 14);                     // Gaussian e4m3 values (sigma 96: the largest near 448)
    for (auto& q : pool) q = enc(gauss(rng) * 96.0);
    const char* scale_names[3] = {"equal scales", "ramped scales (blocks 0, +2, +3, +5 on A)", "jumping scales (A 0,7,0,7; B 7,0,0,7 by row parity)"};
    const char* c_names[3] = {"C = 0", "C comparable", "C dominant (x 2^10)"};
    for (int sk = 0; sk < 3; ++sk)
        for (int ck = 0; ck < 3; ++ck) {
            Batch b;
            const int NC = 256;
            for (int n = 0; n < NC; ++n) {
                const int cs = b.add();
                for (int i = 0; i < 2048; ++i) {
                    b.A[cs * 2048 + i] = pool[rng() & (pool.size() - 1)];
                    b.B[cs * 2048 + i] = pool[rng() & (pool.size() - 1)];
                }
                for (int r = 0; r < 16; ++r)
                    for (int blk = 0; blk < 4; ++blk) {
                        int ea = 0, eb = 0;
                        if (sk == 1) ea = (blk == 0 ? 0 : blk == 1 ? 2 : blk == 2 ? 3 : 5);
                        if (sk == 2) { ea = ((blk + r) & 1) ? 7 : 0; eb = ((blk + r) & 1) ? 0 : 7; if (blk == 2) eb = 0; }
                        b.sA[cs * 64 + r * 4 + blk] = (unsigned char)(127 - 12 + ea);
                        b.sB[cs * 64 + r * 4 + blk] = (unsigned char)(127 - 12 + eb);
                    }
                if (ck > 0) {
                    for (int i = 0; i < 16; ++i)
                        for (int j = 0; j < 16; ++j) {
                            double s, S, mx;
                            b.ref(cs, i, j, s, S, mx);
                            b.C[cs * 256 + i * 16 + j] = (float)(gauss(rng) * std::sqrt(S * mx) * (ck == 2 ? 1024.0 : 1.0));
                        }
                }
            }
            b.run();
            double rS = 0, rM = 0, rR = 0;
            for (int cs = 0; cs < NC; ++cs)
                for (int i = 0; i < 16; ++i)
                    for (int j = 0; j < 16; ++j) {
                        double s, S, mx;
                        b.ref(cs, i, j, s, S, mx);
                        const double err = std::fabs((double)b.D[cs * 256 + i * 16 + j] - s) * 16777216.0;
                        rS = std::fmax(rS, err / S); rM = std::fmax(rM, err / mx);
                        if (s != 0) rR = std::fmax(rR, err / std::fabs(s));
                    }
            printf("%-52s %-20s max |D - ref| / 2^-24:  %.4g S   %.4g max|term|   %.4g |ref|   (%d outputs)\n", scale_names[sk], c_names[ck], rS, rM, rR,
                   NC * 256);
        }
    return 0;
}
