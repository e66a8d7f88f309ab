// Weight preparation of one transformer block (keds_hip.h, keds_block_pack): the one recipe behind both loaders -- the torch
// facade's _pack_tower (keds_amd/model.py) and the handle ABI's load_blocks (session.hip) -- so that the two hold the same bits
// by construction.  Load time only; built from the primitives of elementwise.hip / gemm_fp8.hip and device-to-device copies.
#include "keds_common.h"

namespace {

// nullptr, or why (fp8, f32, f16, folded) at this width cannot be packed
const char* mode_error(int width, int fp8, int f32, int f16, int folded) {
    if (width <= 0 || width % 128) return "width must be a positive multiple of 128";
    if (f32 < 0 || f32 > 2) return "f32 must be 0, 1 (fp32 weights) or 2 (split fp16 planes)";
    if (fp8 && f32) return "fp8 excludes f32";
    if (f16 && (fp8 || f32)) return "f16 excludes fp8 and f32";
    if (fp8 && !folded) return "fp8 needs the folded LayerNorm path";
    if (fp8 && width % 256) return "fp8 needs a width that is a multiple of 256";
    if (f16 && !folded) return "fp16 needs the folded LayerNorm path";
    return nullptr;
}

struct Gemm {
    int n, k;
};

// The arrays of a VALID mode, in buffer order (documented at keds_block_pack in keds_hip.h).  Fills every field of `out`;
// returns the scratch {bias, column sums} vector of the out-proj / c_proj MXFP8 calls (fp8 only), which no kernel reads.
float* layout(KedsCarver& c, int d, int fp8, int f32, int folded, keds_block_params* out) {
    const Gemm g[4] = {{3 * d, d}, {d, d}, {4 * d, d}, {d, 4 * d}};                  // qkv, out, fc, proj
    const size_t wsize = f32 ? 4 : 2;                                              // (f32 == 2: two fp16 planes)
    *out = keds_block_params{};
    const float** ln[4] = {&out->ln1_g, &out->ln1_b, &out->ln2_g, &out->ln2_b};
    const float** bias[4] = {&out->qkv_b, &out->out_b, &out->fc_b, &out->proj_b};
    const void** w[4] = {&out->qkv_w, &out->out_w, &out->fc_w, &out->proj_w};
    for (int j = 0; j < 4; ++j) *ln[j] = (const float*)c.take((size_t)d * 4);
    for (int j = 0; j < 4; ++j) *bias[j] = (const float*)c.take((size_t)g[j].n * 4);
    for (int j = 0; j < 4; ++j) *w[j] = c.take((size_t)g[j].n * g[j].k * wsize);
    if (f32 || !folded) return nullptr;
    out->qkv_wf = c.take((size_t)g[0].n * g[0].k * 2);
    out->fc_wf = c.take((size_t)g[2].n * g[2].k * 2);
    out->qkv_bc = (const float*)c.take((size_t)2 * g[0].n * 4);
    out->fc_bc = (const float*)c.take((size_t)2 * g[2].n * 4);
    if (!fp8) return nullptr;
    const void** q8[4] = {&out->qkv_q8, &out->out_q8, &out->fc_q8, &out->proj_q8};
    const void** s8[4] = {&out->qkv_s8, &out->out_s8, &out->fc_s8, &out->proj_s8};
    for (int j = 0; j < 4; ++j) *q8[j] = c.take((size_t)g[j].n * g[j].k);
    for (int j = 0; j < 4; ++j) *s8[j] = c.take(keds_mxfp8_scale_bytes(g[j].n, g[j].k));
    out->qkv_bc8 = (const float*)c.take((size_t)2 * g[0].n * 4);
    out->fc_bc8 = (const float*)c.take((size_t)2 * g[2].n * 4);
    return (float*)c.take((size_t)2 * d * 4);
}

}  // namespace

extern "C" size_t keds_block_pack_bytes(int width, int fp8, int f32, int f16, int folded) {
    if (const char* why = mode_error(width, fp8, f32, f16, folded)) {
        keds_set_error("keds_block_pack_bytes: %s", why);
        return 0;
    }
    KedsCarver c{nullptr};
    keds_block_params p;
    layout(c, width, fp8, f32, folded, &p);
    return c.bytes();
}

extern "C" int keds_block_pack(const keds_block_source* src, int width, int fp8, int f32, int f16, int folded, void* buf,
                               size_t buf_bytes, keds_block_params* out, void* stream) {
    const char* what = "keds_block_pack";
    const char* why = mode_error(width, fp8, f32, f16, folded);
    KEDS_REQUIRE(why == nullptr, "%s: %s", what, why);
    KEDS_REQUIRE(src && buf && out && (uintptr_t)buf % 256 == 0, "%s: bad argument (buf is 256-byte aligned)", what);
    const float* sv[8] = {src->ln1_g, src->ln1_b, src->ln2_g, src->ln2_b, src->qkv_b, src->out_b, src->fc_b, src->proj_b};
    const float* sw[4] = {src->qkv_w, src->out_w, src->fc_w, src->proj_w};
    for (const float* p : sv) KEDS_REQUIRE(p != nullptr, "%s: a source tensor is null", what);
    for (const float* p : sw) KEDS_REQUIRE(p != nullptr, "%s: a source tensor is null", what);
    KEDS_REQUIRE(buf_bytes >= keds_block_pack_bytes(width, fp8, f32, f16, folded), "%s: buffer too small", what);
    hipStream_t st = (hipStream_t)stream;
    const int d = width;
    const Gemm g[4] = {{3 * d, d}, {d, d}, {4 * d, d}, {d, 4 * d}};
    KedsCarver c{(char*)buf};
    keds_block_params p;
    float* scratch_bc8 = layout(c, d, fp8, f32, folded, &p);
    auto copy = [&](const void* dst, const float* from, size_t count) {
        if (hipMemcpyAsync((void*)dst, from, count * 4, hipMemcpyDeviceToDevice, st) == hipSuccess) return KEDS_OK;
        keds_set_error("%s: device-to-device copy failed", what);
        return KEDS_E_LAUNCH;
    };
    const float* dv[8] = {p.ln1_g, p.ln1_b, p.ln2_g, p.ln2_b, p.qkv_b, p.out_b, p.fc_b, p.proj_b};
    const size_t nv[8] = {(size_t)d, (size_t)d, (size_t)d, (size_t)d, (size_t)g[0].n, (size_t)g[1].n, (size_t)g[2].n, (size_t)g[3].n};
    int rc = KEDS_OK;
    for (int j = 0; j < 8; ++j)
        if ((rc = copy(dv[j], sv[j], nv[j]))) return rc;
    // the four GEMM weights in the operand type of the operating point
    const void* dw[4] = {p.qkv_w, p.out_w, p.fc_w, p.proj_w};
    for (int j = 0; j < 4; ++j) {
        const int64_t count = (int64_t)g[j].n * g[j].k;
        if (f32 == 2) rc = keds_split_f16_weight(sw[j], g[j].n, g[j].k, (void*)dw[j], count, &p.x3_exp[j], stream);
        else if (f32) rc = copy(dw[j], sw[j], (size_t)count);
        else if (f16) rc = keds_cast_f16(sw[j], (void*)dw[j], count, stream);
        else rc = keds_cast_bf16(sw[j], (void*)dw[j], count, stream);
        if (rc) return rc;
    }
    if (p.qkv_wf) {     // ln_1 folded into in_proj, ln_2 into c_fc: fp16, they multiply the fp16 residual stream
        if ((rc = keds_fold_layernorm_ex(sw[0], src->qkv_b, src->ln1_g, src->ln1_b, g[0].n, g[0].k, (void*)p.qkv_wf, 1,
                                         (float*)p.qkv_bc, stream)) ||
            (rc = keds_fold_layernorm_ex(sw[2], src->fc_b, src->ln2_g, src->ln2_b, g[2].n, g[2].k, (void*)p.fc_wf, 1,
                                         (float*)p.fc_bc, stream)))
            return rc;
    }
    if (p.qkv_q8) {     // MXFP8 copies of the four weights: in_proj / c_fc with their LayerNorm folded in, out_proj / c_proj plain
        const void* q8[4] = {p.qkv_q8, p.out_q8, p.fc_q8, p.proj_q8};
        const void* s8[4] = {p.qkv_s8, p.out_s8, p.fc_s8, p.proj_s8};
        const float* gamma[4] = {src->ln1_g, nullptr, src->ln2_g, nullptr};
        const float* beta[4] = {src->ln1_b, nullptr, src->ln2_b, nullptr};
        float* bc8[4] = {(float*)p.qkv_bc8, scratch_bc8, (float*)p.fc_bc8, scratch_bc8};
        for (int j = 0; j < 4; ++j)
            if ((rc = keds_fold_layernorm_mxfp8(sw[j], sv[4 + j], gamma[j], beta[j], g[j].n, g[j].k, g[j].n, (void*)q8[j],
                                                (void*)s8[j], bc8[j], stream)))
                return rc;
    }
    *out = p;
    return KEDS_OK;
}
