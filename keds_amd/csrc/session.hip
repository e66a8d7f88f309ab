// Handle-based C ABI (include/keds_session.h): the library owns packed weights, the database,
// workspaces and the RCCL communicator; every forward calls the stateless entry points of
// keds_hip.h, so results are bit-identical to the torch-hosted path.  Architecture inference
// follows build_model (src/model/model.py:951-991): everything is read off the tensor shapes.
#include "keds_common.h"
#include "tower_plan.h"      // text_runs_packed
#include "../../include/keds_session.h"
#include <dlfcn.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>


#define HIP_TRY(call, what)                                                    \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            keds_set_error("%s: %s", what, hipGetErrorString(e_));             \
            return KEDS_E_LAUNCH;                                              \
        }                                                                      \
    } while (0)

namespace {

// dst[r, c] = src[r*rs + c*cs] for c < cols, 0 for cols <= c < dcols   (cast / transpose / zero-pad in one pass)
template <typename DST>
__global__ void pack2d_kernel(const void* __restrict__ src, int sdt, long long rs, long long cs, int rows, int cols,
                              int dcols, DST* __restrict__ dst) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)rows * dcols) return;
    const int r = (int)(i / dcols), c = (int)(i % dcols);
    float v = 0.f;
    if (c < cols) {
        const long long s = r * rs + c * cs;
        if (sdt == KEDS_F32) v = ((const float*)src)[s];
        else if (sdt == KEDS_BF16) v = bf16_bits_to_f32(((const unsigned short*)src)[s]);
        else v = (float)((const _Float16*)src)[s];
    }
    dst[i] = (DST)v;
}

size_t dtype_size(int dt) { return dt == KEDS_F32 ? 4 : 2; }

// device allocations owned by one handle
struct Arena {
    std::vector<void*> blocks;
    void* alloc(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return nullptr;
        blocks.push_back(p);
        return p;
    }
    ~Arena() {
        for (void* p : blocks) (void)hipFree(p);
    }
};

struct GrowBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int reserve(size_t need, hipStream_t st, const char* what) {
        if (need <= bytes) return KEDS_OK;
        if (p) {
            HIP_TRY(hipStreamSynchronize(st), what);
            HIP_TRY(hipFree(p), what);
            p = nullptr;
            bytes = 0;
        }
        HIP_TRY(hipMalloc(&p, need), what);
        bytes = need;
        return KEDS_OK;
    }
    ~GrowBuf() {
        if (p) (void)hipFree(p);
    }
};

struct Weights {
    std::map<std::string, const keds_tensor*> by_name;
    Weights(const keds_tensor* t, int n) {
        for (int i = 0; i < n; ++i)
            if (t[i].name) by_name[t[i].name] = &t[i];
    }
    const keds_tensor* find(const std::string& k) const {
        auto it = by_name.find(k);
        return it == by_name.end() ? nullptr : it->second;
    }
    int count_layers(const std::string& prefix, const std::string& suffix) const {
        int n = 0;
        while (find(prefix + std::to_string(n) + suffix)) ++n;
        return n;
    }
};

int64_t numel(const keds_tensor* t) {
    int64_t n = 1;
    for (int i = 0; i < t->ndim; ++i) n *= t->shape[i];
    return n;
}

// Upload (host or device source) and convert one tensor viewed as [rows, cols] with element strides (rs, cs)
// into a dense [rows, dcols] device matrix of DST.  Synchronous: load-time only.
template <typename DST>
int pack_tensor(Arena& mem, const keds_tensor* t, int rows, int cols, long long rs, long long cs, int dcols, DST** out,
                const char* what) {
    KEDS_REQUIRE(t->dtype == KEDS_F32 || t->dtype == KEDS_BF16 || t->dtype == KEDS_F16, "%s: %s has an unknown dtype",
                 what, t->name);
    const size_t raw = (size_t)numel(t) * dtype_size(t->dtype);
    void* stage = nullptr;
    HIP_TRY(hipMalloc(&stage, raw ? raw : 16), what);
    hipError_t e = hipMemcpy(stage, t->data, raw, hipMemcpyDefault);
    if (e != hipSuccess) {
        (void)hipFree(stage);
        keds_set_error("%s: copying %s: %s", what, t->name, hipGetErrorString(e));
        return KEDS_E_LAUNCH;
    }
    DST* dst = (DST*)mem.alloc((size_t)rows * dcols * sizeof(DST));
    if (!dst) {
        (void)hipFree(stage);
        keds_set_error("%s: out of device memory for %s", what, t->name);
        return KEDS_E_LAUNCH;
    }
    const long long total = (long long)rows * dcols;
    pack2d_kernel<DST><<<(unsigned)((total + 255) / 256), 256, 0, 0>>>(stage, t->dtype, rs, cs, rows, cols, dcols, dst);
    e = hipDeviceSynchronize();
    (void)hipFree(stage);
    if (e != hipSuccess) {
        keds_set_error("%s: packing %s: %s", what, t->name, hipGetErrorString(e));
        return KEDS_E_LAUNCH;
    }
    *out = dst;
    return KEDS_OK;
}

// operating point of a tower: the fp8 / f32 / f16 fields of keds_tower_params
struct Mode {
    int fp8, f32, f16;
};

struct Loader {
    const Weights& w;
    Arena& mem;
    const char* what;
    int need(const std::string& key, int ndim, const keds_tensor** out) const {
        const keds_tensor* t = w.find(key);
        KEDS_REQUIRE(t != nullptr, "%s: missing weight '%s'", what, key.c_str());
        KEDS_REQUIRE(t->ndim == ndim && t->data, "%s: '%s' must be a %d-d tensor", what, key.c_str(), ndim);
        *out = t;
        return KEDS_OK;
    }
    // [n] fp32 vector
    int vec(const std::string& key, int64_t n, const float** out) const {
        const keds_tensor* t;
        int rc = need(key, 1, &t);
        if (rc) return rc;
        KEDS_REQUIRE(t->shape[0] == n, "%s: '%s' has %lld elements, expected %lld", what, key.c_str(),
                     (long long)t->shape[0], (long long)n);
        float* d;
        if ((rc = pack_tensor<float>(mem, t, 1, (int)n, 0, 1, (int)n, &d, what))) return rc;
        *out = d;
        return KEDS_OK;
    }
    // [rows, cols] matrix as stored -> bf16 (GEMM operand, K contiguous) or fp32
    template <typename DST>
    int mat(const std::string& key, int64_t rows, int64_t cols, const DST** out, bool transpose = false) const {
        const keds_tensor* t;
        int rc = need(key, 2, &t);
        if (rc) return rc;
        const int64_t sr = transpose ? cols : rows, sc = transpose ? rows : cols;
        KEDS_REQUIRE(t->shape[0] == sr && t->shape[1] == sc, "%s: '%s' is [%lld,%lld], expected [%lld,%lld]", what,
                     key.c_str(), (long long)t->shape[0], (long long)t->shape[1], (long long)sr, (long long)sc);
        DST* d;
        if (transpose) rc = pack_tensor<DST>(mem, t, (int)rows, (int)cols, 1, rows, (int)cols, &d, what);
        else rc = pack_tensor<DST>(mem, t, (int)rows, (int)cols, cols, 1, (int)cols, &d, what);
        if (rc) return rc;
        *out = d;
        return KEDS_OK;
    }
    // t viewed as [rows, cols] (transpose: stored as [cols, rows]) -> dense [rows, dcols], zero padded, in the GEMM operand
    // type of the operating point: fp32, fp16 or bf16.  The caller has checked the shape.
    int operand(const keds_tensor* t, const Mode& m, int rows, int cols, bool transpose, int dcols, const void** out) const {
        const long long rs = transpose ? 1 : cols, cs = transpose ? rows : 1;
        return m.f32   ? typed<float>(t, rows, cols, rs, cs, dcols, out)
               : m.f16 ? typed<f16_t>(t, rows, cols, rs, cs, dcols, out)
                       : typed<bf16_t>(t, rows, cols, rs, cs, dcols, out);
    }
    template <typename DST>
    int typed(const keds_tensor* t, int rows, int cols, long long rs, long long cs, int dcols, const void** out) const {
        DST* d;
        const int rc = pack_tensor<DST>(mem, t, rows, cols, rs, cs, dcols, &d, what);
        if (!rc) *out = d;
        return rc;
    }
};

int decode_compute(int compute, const char* what, Mode* m) {
    KEDS_REQUIRE(compute == KEDS_BF16 || compute == KEDS_F16 || compute == KEDS_FP8 || compute == KEDS_F32 || compute == KEDS_F32X3,
                 "%s: compute dtype must be KEDS_BF16, KEDS_F16, KEDS_FP8, KEDS_F32 or KEDS_F32X3", what);
    *m = Mode{compute == KEDS_FP8, compute == KEDS_F32 ? 1 : compute == KEDS_F32X3 ? 2 : 0, compute == KEDS_F16};
    return KEDS_OK;
}

// KEDS_DETERMINISTIC=1 keeps the separate LayerNorm kernels (A/B reference; the folded path is reproducible too)
int folded_flow(const Mode& m, const char* what, bool* folded) {
    const char* det = getenv("KEDS_DETERMINISTIC");
    *folded = !(det && det[0] == '1');
    KEDS_REQUIRE(!m.f16 || *folded, "%s: KEDS_F16 needs the folded LayerNorm path (KEDS_DETERMINISTIC=1 is set)", what);
    return KEDS_OK;
}

// resblocks of one tower (model.py:305-326): keys <prefix>transformer.resblocks.<i>.*, packed by keds_block_pack (keds_hip.h) --
// the routine the torch facade calls too -- from fp32 copies of a block's twelve tensors that live until the block is packed
int load_blocks(const Loader& L, const std::string& prefix, int width, int layers, std::vector<keds_block_params>& blocks,
                const Mode& m, bool folded) {
    const size_t bytes = keds_block_pack_bytes(width, m.fp8, m.f32, m.f16, folded);
    if (!bytes) return KEDS_E_ARG;                              // (the message is keds_block_pack_bytes' own)
    blocks.assign(layers, keds_block_params{});
    for (int i = 0; i < layers; ++i) {
        const std::string b = prefix + "transformer.resblocks." + std::to_string(i) + ".";
        Arena tmp;
        Loader T{L.w, tmp, L.what};
        keds_block_source s;
        int rc;
        if ((rc = T.vec(b + "ln_1.weight", width, &s.ln1_g)) || (rc = T.vec(b + "ln_1.bias", width, &s.ln1_b)) ||
            (rc = T.vec(b + "ln_2.weight", width, &s.ln2_g)) || (rc = T.vec(b + "ln_2.bias", width, &s.ln2_b)) ||
            (rc = T.mat<float>(b + "attn.in_proj_weight", 3 * width, width, &s.qkv_w)) ||
            (rc = T.vec(b + "attn.in_proj_bias", 3 * width, &s.qkv_b)) ||
            (rc = T.mat<float>(b + "attn.out_proj.weight", width, width, &s.out_w)) ||
            (rc = T.vec(b + "attn.out_proj.bias", width, &s.out_b)) ||
            (rc = T.mat<float>(b + "mlp.c_fc.weight", 4 * width, width, &s.fc_w)) ||
            (rc = T.vec(b + "mlp.c_fc.bias", 4 * width, &s.fc_b)) ||
            (rc = T.mat<float>(b + "mlp.c_proj.weight", width, 4 * width, &s.proj_w)) ||
            (rc = T.vec(b + "mlp.c_proj.bias", width, &s.proj_b)))
            return rc;
        void* buf = L.mem.alloc(bytes);
        KEDS_REQUIRE(buf, "%s: out of device memory", L.what);
        if ((rc = keds_block_pack(&s, width, m.fp8, m.f32, m.f16, folded, buf, bytes, &blocks[i], nullptr))) return rc;
        HIP_TRY(hipDeviceSynchronize(), L.what);               // (the pack has read the sources before tmp frees them)
    }
    return KEDS_OK;
}

// ---- RCCL, bound at run time so the library has no link-time dependency on it ------------------
struct CommId {
    char bytes[KEDS_COMM_ID_BYTES];
};
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(CommId*) = nullptr;
    int (*CommInitRank)(void**, int, CommId, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*AllToAll)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;      // RCCL extension (optional)
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;

int rccl_load() {
    if (g_rccl.lib) return KEDS_OK;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    for (const char* n : names)          // an already loaded copy (e.g. the host framework's) wins
        if ((h = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;
    if (!h)
        for (const char* n : names)
            if ((h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    KEDS_REQUIRE(h != nullptr, "keds_comm: cannot load librccl (%s)", dlerror());
    Rccl r;
    r.lib = h;
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(h, "ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(h, "ncclCommDestroy");
    r.AllGather = (decltype(r.AllGather))dlsym(h, "ncclAllGather");
    r.AllToAll = (decltype(r.AllToAll))dlsym(h, "ncclAllToAll");
    r.Send = (decltype(r.Send))dlsym(h, "ncclSend");
    r.Recv = (decltype(r.Recv))dlsym(h, "ncclRecv");
    r.GroupStart = (decltype(r.GroupStart))dlsym(h, "ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))dlsym(h, "ncclGroupEnd");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "ncclGetErrorString");
    KEDS_REQUIRE(r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.AllGather, "keds_comm: librccl lacks a symbol");
    KEDS_REQUIRE(r.AllToAll || (r.Send && r.Recv && r.GroupStart && r.GroupEnd),
                 "keds_comm: librccl has neither ncclAllToAll nor ncclSend / ncclRecv");
    g_rccl = r;
    return KEDS_OK;
}

int rccl_check(int rc, const char* what) {
    if (rc == 0) return KEDS_OK;
    keds_set_error("%s: RCCL error %d (%s)", what, rc, g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "?");
    return KEDS_E_LAUNCH;
}

}  // namespace

// ---- handles ----------------------------------------------------------------------------------------
struct keds_ctx {
    int device = 0;
    void* comm = nullptr;
    int rank = 0, world = 1;
};

struct keds_vit {
    keds_ctx* ctx;
    int device = 0;            // copied from the context: destroy must not touch a context that may already be gone
    Arena mem;
    std::vector<keds_block_params> blocks;
    keds_vit_params p;
    GrowBuf ws, img;
};

struct keds_text {
    keds_ctx* ctx;
    int device = 0;            // copied from the context: destroy must not touch a context that may already be gone
    Arena mem;
    std::vector<keds_block_params> blocks;
    keds_text_params p;
    GrowBuf ws, tok;
};

struct keds_knowledge {
    keds_ctx* ctx;
    int device = 0;            // copied from the context: destroy must not touch a context that may already be gone
    Arena mem;
    std::vector<keds_cross_layer_params> fuse, cond;
    keds_crossformer_fused fuse_f, cond_f;     // launch-saving weight re-arrangement (keds_hip.h)
    keds_knowledge_params p;
    GrowBuf ws;
};

struct keds_index {
    keds_ctx* ctx;
    int device = 0;            // copied from the context: destroy must not touch a context that may already be gone
    int dim, metric;
    int64_t n = 0, row0 = 0, cap = 0;     // cap: rows the two buffers below are sized for (grows geometrically)
    float* rows = nullptr;
    void* packed = nullptr;
    GrowBuf ws, xws;
};

static int use_device(const keds_ctx* ctx, const char* what) {
    KEDS_REQUIRE(ctx != nullptr, "%s: null context", what);
    HIP_TRY(hipSetDevice(ctx->device), what);
    return KEDS_OK;
}

extern "C" int keds_ctx_create(int device, keds_ctx** out) {
    KEDS_REQUIRE(out != nullptr, "keds_ctx_create: null out");
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count), "keds_ctx_create");
    KEDS_REQUIRE(device >= 0 && device < count, "keds_ctx_create: device %d of %d", device, count);
    HIP_TRY(hipSetDevice(device), "keds_ctx_create");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device), "keds_ctx_create");
    KEDS_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0, "keds_ctx_create: device %d is %s, this library is gfx950 only",
                 device, prop.gcnArchName);
    keds_ctx* c = new keds_ctx();
    c->device = device;
    // (split-K scratch of the small-M GEMMs lives inside every handle's own workspace: keds_common.h, KedsSplitKScope)
    *out = c;
    return KEDS_OK;
}

extern "C" int keds_ctx_destroy(keds_ctx* ctx) {
    if (!ctx) return KEDS_OK;
    if (ctx->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(ctx->comm);
    delete ctx;
    return KEDS_OK;
}

// ---- image tower ------------------------------------------------------------------------------------
extern "C" int keds_vit_create(keds_ctx* ctx, const keds_tensor* weights, int n, int compute, keds_vit** out) {
    const char* what = "keds_vit_create";
    KEDS_REQUIRE(weights && n > 0 && out, "%s: bad argument", what);
    Mode m;
    bool folded;
    int rc;
    if ((rc = decode_compute(compute, what, &m)) || (rc = folded_flow(m, what, &folded)) || (rc = use_device(ctx, what))) return rc;
    Weights W(weights, n);
    const keds_tensor *conv, *pos, *proj;
    keds_vit* v = new keds_vit();
    v->ctx = ctx;
    v->device = ctx->device;
    Loader L{W, v->mem, what};
    auto fail = [&](int code) {
        delete v;
        return code;
    };
    if ((rc = L.need("visual.conv1.weight", 4, &conv)) || (rc = L.need("visual.positional_embedding", 2, &pos)) ||
        (rc = L.need("visual.proj", 2, &proj)))
        return fail(rc);
    // model.py:955-961: width = conv1.shape[0], patch = conv1.shape[-1], grid = round(sqrt(pos.shape[0]-1))
    const int width = (int)conv->shape[0], patch = (int)conv->shape[3];
    const int grid = (int)std::lround(std::sqrt((double)(pos->shape[0] - 1)));
    const int layers = W.count_layers("visual.transformer.resblocks.", ".attn.in_proj_weight");
    const int embed = (int)proj->shape[1];
    if (conv->shape[1] != 3 || conv->shape[2] != patch || grid * grid + 1 != pos->shape[0] || pos->shape[1] != width ||
        proj->shape[0] != width || layers < 1 || width % 128 != 0) {
        keds_set_error("%s: inconsistent visual.* shapes (width %d, patch %d, grid %d, layers %d)", what, width, patch, grid,
                       layers);
        return fail(KEDS_E_ARG);
    }
    if ((rc = load_blocks(L, "visual.", width, layers, v->blocks, m, folded))) return fail(rc);
    keds_vit_params& p = v->p;
    memset(&p, 0, sizeof(p));
    p.tower.width = width;
    p.tower.layers = layers;
    p.tower.heads = width / 64;
    p.tower.seq = grid * grid + 1;
    p.tower.causal = 0;
    p.tower.blocks = v->blocks.data();
    p.tower.last_cls_only = 1;
    p.tower.fp8 = m.fp8;
    p.tower.f32 = m.f32;
    p.tower.f16 = m.f16;
    p.resolution = grid * patch;
    p.patch = patch;
    const int kreal = 3 * patch * patch;
    p.kpad = (kreal + 63) / 64 * 64;
    p.embed_dim = embed;
    // [width, 3*P*P] zero padded to kpad columns (im2col order == the conv weight's own order)
    if ((rc = L.operand(conv, m, width, kreal, false, p.kpad, &p.conv_w))) return fail(rc);
    if ((rc = L.vec("visual.class_embedding", width, &p.class_emb)) ||
        (rc = L.mat<float>("visual.positional_embedding", p.tower.seq, width, &p.pos_emb)) ||
        (rc = L.vec("visual.ln_pre.weight", width, &p.ln_pre_g)) || (rc = L.vec("visual.ln_pre.bias", width, &p.ln_pre_b)) ||
        (rc = L.vec("visual.ln_post.weight", width, &p.ln_post_g)) ||
        (rc = L.vec("visual.ln_post.bias", width, &p.ln_post_b)) ||
        (rc = L.operand(proj, m, embed, width, /*transpose=*/true, width, &p.proj_t)))
        return fail(rc);
    *out = v;
    return KEDS_OK;
}

extern "C" int keds_vit_destroy(keds_vit* vit) {
    if (vit) {
        (void)hipSetDevice(vit->device);
        delete vit;
    }
    return KEDS_OK;
}

extern "C" int keds_vit_info(const keds_vit* vit, int* width, int* layers, int* resolution, int* patch, int* embed_dim) {
    KEDS_REQUIRE(vit != nullptr, "keds_vit_info: null handle");
    if (width) *width = vit->p.tower.width;
    if (layers) *layers = vit->p.tower.layers;
    if (resolution) *resolution = vit->p.resolution;
    if (patch) *patch = vit->p.patch;
    if (embed_dim) *embed_dim = vit->p.embed_dim;
    return KEDS_OK;
}

// the image as fp32 (a converted copy in the handle's buffer for bf16 / fp16 images) and a workspace for B images
static int vit_prepare(keds_vit* vit, const void* image, int img_dtype, int B, hipStream_t st, const char* what, const float** img) {
    int rc;
    *img = (const float*)image;
    if (img_dtype != KEDS_F32) {
        KEDS_REQUIRE(img_dtype == KEDS_BF16 || img_dtype == KEDS_F16, "%s: unknown image dtype", what);
        const long long count = (long long)B * 3 * vit->p.resolution * vit->p.resolution;
        if ((rc = vit->img.reserve((size_t)count * 4, st, what))) return rc;
        pack2d_kernel<float><<<(unsigned)((count + 255) / 256), 256, 0, st>>>(image, img_dtype, 0, 1, 1, (int)count,
                                                                                (int)count, (float*)vit->img.p);
        if ((rc = keds_check_launch(what))) return rc;
        *img = (const float*)vit->img.p;
    }
    const size_t need = keds_vit_workspace_bytes(&vit->p, B);
    return vit->ws.reserve(need, st, what);
}

extern "C" int keds_vit_forward(keds_vit* vit, const void* image, int img_dtype, int B, void* out, void* stream) {
    const char* what = "keds_vit_forward";
    KEDS_REQUIRE(vit && image && out && B > 0, "%s: bad argument", what);
    const float* img;
    int rc = vit_prepare(vit, image, img_dtype, B, (hipStream_t)stream, what, &img);
    if (rc) return rc;
    return keds_vit_run(&vit->p, img, B, (float*)out, 0, vit->ws.p, vit->ws.bytes, stream);
}

extern "C" int keds_vit_forward_tokens(keds_vit* vit, const void* image, int img_dtype, int B, void* out, void* taps, void* tokens,
                                       int out_type, void* stream) {
    const char* what = "keds_vit_forward_tokens";
    KEDS_REQUIRE(B >= 1, "%s: B = %d, at least 1 image", what, B);
    KEDS_REQUIRE(out || taps || tokens, "%s: no output requested (out, taps and tokens are all null)", what);
    KEDS_REQUIRE(out_type >= 0 && out_type <= 2, "%s: out_type %d (0 bf16, 1 fp32, 2 fp16)", what, out_type);
    KEDS_REQUIRE(vit && image, "%s: bad argument", what);
    const float* img;
    int rc = vit_prepare(vit, image, img_dtype, B, (hipStream_t)stream, what, &img);
    if (rc) return rc;
    return keds_vit_run_tokens(&vit->p, img, B, (float*)out, 0, taps, tokens, out_type, vit->ws.p, vit->ws.bytes, stream);
}

// ---- text tower -------------------------------------------------------------------------------------
extern "C" int keds_text_create(keds_ctx* ctx, const keds_tensor* weights, int n, int compute, keds_text** out) {
    const char* what = "keds_text_create";
    KEDS_REQUIRE(weights && n > 0 && out, "%s: bad argument", what);
    Mode m;
    bool folded;
    int rc;
    if ((rc = decode_compute(compute, what, &m)) || (rc = folded_flow(m, what, &folded)) || (rc = use_device(ctx, what))) return rc;
    Weights W(weights, n);
    keds_text* t = new keds_text();
    t->ctx = ctx;
    t->device = ctx->device;
    Loader L{W, t->mem, what};
    auto fail = [&](int code) {
        delete t;
        return code;
    };
    const keds_tensor *emb, *pos, *proj;
    if ((rc = L.need("token_embedding.weight", 2, &emb)) || (rc = L.need("positional_embedding", 2, &pos)) ||
        (rc = L.need("text_projection", 2, &proj)))
        return fail(rc);
    // model.py:977-982: embed_dim = text_projection.shape[1], context = positional_embedding.shape[0],
    // vocab = token_embedding.shape[0], width = ln_final.shape[0], heads = width // 64
    const int vocab = (int)emb->shape[0], width = (int)emb->shape[1], context = (int)pos->shape[0];
    const int embed = (int)proj->shape[1];
    const int layers = W.count_layers("transformer.resblocks.", ".attn.in_proj_weight");
    if (pos->shape[1] != width || proj->shape[0] != width || layers < 1 || width % 128 != 0) {
        keds_set_error("%s: inconsistent text tower shapes (width %d, context %d, layers %d)", what, width, context, layers);
        return fail(KEDS_E_ARG);
    }
    m.fp8 = m.fp8 && width % 256 == 0;      // (a text tower of another width stays bf16 next to an fp8 image tower)
    if ((rc = load_blocks(L, "", width, layers, t->blocks, m, folded))) return fail(rc);
    keds_text_params& p = t->p;
    memset(&p, 0, sizeof(p));
    p.tower.width = width;
    p.tower.layers = layers;
    p.tower.heads = width / 64;
    p.tower.seq = context;
    p.tower.causal = 1;
    p.tower.blocks = t->blocks.data();
    p.tower.last_cls_only = 0;
    p.tower.fp8 = m.fp8;
    p.tower.f32 = m.f32;
    p.tower.f16 = m.f16;
    p.vocab = vocab;
    p.embed_dim = embed;
    if ((rc = L.mat<float>("token_embedding.weight", vocab, width, &p.token_emb)) ||
        (rc = L.mat<float>("positional_embedding", context, width, &p.pos_emb)) ||
        (rc = L.vec("ln_final.weight", width, &p.ln_final_g)) || (rc = L.vec("ln_final.bias", width, &p.ln_final_b)) ||
        (rc = L.operand(proj, m, embed, width, /*transpose=*/true, width, &p.proj_t)))
        return fail(rc);
    *out = t;
    return KEDS_OK;
}

extern "C" int keds_text_destroy(keds_text* txt) {
    if (txt) {
        (void)hipSetDevice(txt->device);
        delete txt;
    }
    return KEDS_OK;
}

extern "C" int keds_text_info(const keds_text* txt, int* width, int* layers, int* context, int* vocab, int* embed_dim) {
    KEDS_REQUIRE(txt != nullptr, "keds_text_info: null handle");
    if (width) *width = txt->p.tower.width;
    if (layers) *layers = txt->p.tower.layers;
    if (context) *context = txt->p.tower.seq;
    if (vocab) *vocab = txt->p.vocab;
    if (embed_dim) *embed_dim = txt->p.embed_dim;
    return KEDS_OK;
}

extern "C" int keds_text_forward(keds_text* txt, const int32_t* tokens, const void* img_tokens, int n_img_tok,
                                 int insert_idx, const int32_t* readout_idx, int B, void* out, void* stream) {
    return keds_text_forward_used(txt, tokens, img_tokens, n_img_tok, insert_idx, readout_idx, 0, B, out, stream);
}

extern "C" int keds_text_forward_used(keds_text* txt, const int32_t* tokens, const void* img_tokens, int n_img_tok,
                                      int insert_idx, const int32_t* readout_idx, int seq_used, int B, void* out, void* stream) {
    const char* what = "keds_text_forward";
    KEDS_REQUIRE(txt && tokens && readout_idx && out && B > 0, "%s: bad argument", what);
    KEDS_REQUIRE((img_tokens == nullptr) == (n_img_tok == 0), "%s: img_tokens and n_img_tok disagree", what);
    KEDS_REQUIRE(n_img_tok == 0 || n_img_tok == 2 || n_img_tok == 3, "%s: 2 or 3 pseudo tokens (model.py:831-834)", what);
    KEDS_REQUIRE(n_img_tok == 0 || (insert_idx >= 0 && insert_idx + n_img_tok <= txt->p.tower.seq),
                 "%s: insert_idx out of range", what);
    int rc;
    const size_t need = keds_text_workspace_bytes(&txt->p, B);
    if ((rc = txt->ws.reserve(need, (hipStream_t)stream, what))) return rc;
    return keds_text_run_ex(&txt->p, tokens, readout_idx, (const float*)img_tokens, n_img_tok, insert_idx, B, seq_used, (float*)out,
                            0, txt->ws.p, txt->ws.bytes, stream);
}

// The same with the read-out columns on the HOST (round 6): a caption needs its own columns [0, read-out column] only, so the
// tower runs on packed rows -- sum of the captions' lengths instead of B x the longest (keds_text_run_packed, keds_hip.h) -- when
// that saves an eighth of the rows and the tower is a bf16 one on its default flow; the rectangular cut of keds_text_forward_used
// otherwise.  readout_host: host int32 [B].
extern "C" int keds_text_forward_packed(keds_text* txt, const int32_t* tokens, const void* img_tokens, int n_img_tok,
                                        int insert_idx, const int32_t* readout_host, int B, void* out, void* stream) {
    const char* what = "keds_text_forward_packed";
    KEDS_REQUIRE(txt && tokens && readout_host && out && B > 0, "%s: bad argument", what);
    const int L = txt->p.tower.seq;
    std::vector<int32_t> host(2 * (size_t)B + 1);        // [0, B]: offsets; [B + 1, 2B]: global read-out rows
    long long rows = 0;
    int seq_used = 0;
    for (int b = 0; b < B; ++b) {
        KEDS_REQUIRE(readout_host[b] >= 0 && readout_host[b] < L, "%s: read-out column %d of sample %d outside [0, %d)", what, readout_host[b], b, L);
        host[b] = (int32_t)rows;
        host[B + 1 + b] = (int32_t)(rows + readout_host[b]);
        rows += readout_host[b] + 1;
        seq_used = readout_host[b] + 1 > seq_used ? readout_host[b] + 1 : seq_used;
    }
    host[B] = (int32_t)rows;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = txt->tok.reserve(host.size() * sizeof(int32_t), st, what))) return rc;
    // (pageable source: the copy has left `host` when the call returns)
    HIP_TRY(hipMemcpyAsync(txt->tok.p, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice, st), what);
    const int32_t* dev = (const int32_t*)txt->tok.p;
    const bool packed = text_runs_packed(txt->p.tower.causal != 0, txt->p.tower.fp8 != 0, keds_text_trim_mode(), rows, B, seq_used);
    KEDS_REQUIRE((img_tokens == nullptr) == (n_img_tok == 0), "%s: img_tokens and n_img_tok disagree", what);
    KEDS_REQUIRE(n_img_tok == 0 || n_img_tok == 2 || n_img_tok == 3, "%s: 2 or 3 pseudo tokens (model.py:831-834)", what);
    KEDS_REQUIRE(n_img_tok == 0 || (insert_idx >= 0 && insert_idx + n_img_tok <= L), "%s: insert_idx out of range", what);
    const size_t need = keds_text_workspace_bytes(&txt->p, B);
    if ((rc = txt->ws.reserve(need, st, what))) return rc;
    if (packed)
        return keds_text_run_packed(&txt->p, tokens, dev, dev + B + 1, (int)rows, seq_used, (const float*)img_tokens, n_img_tok, insert_idx,
                                    B, (float*)out, 0, txt->ws.p, txt->ws.bytes, stream);
    // rectangular: the device copy of the columns themselves
    for (int b = 0; b < B; ++b) host[b] = readout_host[b];
    HIP_TRY(hipMemcpyAsync(txt->tok.p, host.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st), what);
    return keds_text_run_ex(&txt->p, tokens, dev, (const float*)img_tokens, n_img_tok, insert_idx, B, seq_used, (float*)out, 0,
                            txt->ws.p, txt->ws.bytes, stream);
}

extern "C" int keds_text_forward_tokens(keds_text* txt, const int32_t* tokens, int B, void* out, int out_type, void* stream) {
    const char* what = "keds_text_forward_tokens";
    KEDS_REQUIRE(B >= 1, "%s: B = %d, at least 1 sequence", what, B);
    KEDS_REQUIRE(out, "%s: no output requested (out is null)", what);
    KEDS_REQUIRE(out_type >= 0 && out_type <= 2, "%s: out_type %d (0 bf16, 1 fp32, 2 fp16)", what, out_type);
    KEDS_REQUIRE(txt && tokens, "%s: bad argument", what);
    const size_t need = keds_text_workspace_bytes(&txt->p, B);
    int rc = txt->ws.reserve(need, (hipStream_t)stream, what);
    if (rc) return rc;
    return keds_text_run_tokens(&txt->p, tokens, B, out, out_type, txt->ws.p, txt->ws.bytes, stream);
}

// ---- knowledge injection ------------------------------------------------------------------------------
namespace {
int load_crossformer(const Loader& L, const Weights& W, std::vector<keds_cross_layer_params>& layers,
                     keds_crossformer_params* out) {
    const int n = W.count_layers("cross_layers.", ".to_q.weight");
    KEDS_REQUIRE(n >= 1, "%s: no cross_layers.*.to_q.weight", L.what);
    const keds_tensor* q0;
    int rc = L.need("cross_layers.0.to_q.weight", 2, &q0);
    if (rc) return rc;
    const int inner = (int)q0->shape[0], dim = (int)q0->shape[1];     // model.py:41-47: inner = heads * dim_head(64)
    KEDS_REQUIRE(inner % 64 == 0, "%s: inner dim %d is not heads x 64", L.what, inner);
    layers.assign(n, keds_cross_layer_params{});
    for (int i = 0; i < n; ++i) {
        const std::string b = "cross_layers." + std::to_string(i) + ".";
        keds_cross_layer_params& c = layers[i];
        const bf16_t* m;
        if ((rc = L.mat<bf16_t>(b + "to_q.weight", inner, dim, &m))) return rc;
        c.wq = m;
        if ((rc = L.mat<bf16_t>(b + "to_k.weight", inner, dim, &m))) return rc;
        c.wk = m;
        if ((rc = L.mat<bf16_t>(b + "to_v.weight", inner, dim, &m))) return rc;
        c.wv = m;
        if ((rc = L.mat<bf16_t>(b + "to_out.0.weight", dim, inner, &m))) return rc;
        c.wo = m;
        if ((rc = L.vec(b + "to_q.bias", inner, &c.bq)) || (rc = L.vec(b + "to_k.bias", inner, &c.bk)) ||
            (rc = L.vec(b + "to_v.bias", inner, &c.bv)) || (rc = L.vec(b + "to_out.0.bias", dim, &c.bo)))
            return rc;
    }
    out->dim = dim;
    out->heads = inner / 64;
    out->layers = n;
    out->layer = layers.data();
    out->fused = nullptr;
    return KEDS_OK;
}
}  // namespace

extern "C" int keds_knowledge_create(keds_ctx* ctx, const keds_tensor* im2text, int n_im2text, const keds_tensor* fuse,
                                     int n_fuse, const keds_tensor* cond, int n_cond, keds_knowledge** out) {
    const char* what = "keds_knowledge_create";
    KEDS_REQUIRE(im2text && fuse && cond && n_im2text > 0 && n_fuse > 0 && n_cond > 0 && out, "%s: bad argument", what);
    int rc = use_device(ctx, what);
    if (rc) return rc;
    keds_knowledge* k = new keds_knowledge();
    k->ctx = ctx;
    k->device = ctx->device;
    memset(&k->p, 0, sizeof(k->p));
    auto fail = [&](int code) {
        delete k;
        return code;
    };
    {   // IM2TEXT (model.py:105-123): layers.{i}.0 = Linear, fc_out
        Weights W(im2text, n_im2text);
        Loader L{W, k->mem, what};
        const int nl = W.count_layers("layers.", ".0.weight");
        const keds_tensor *w0, *wo;
        if (nl < 1 || nl > 4) {
            keds_set_error("%s: IM2TEXT with %d hidden layers (1..4 supported)", what, nl);
            return fail(KEDS_E_ARG);
        }
        if ((rc = L.need("layers.0.0.weight", 2, &w0)) || (rc = L.need("fc_out.weight", 2, &wo))) return fail(rc);
        keds_im2text_params& p = k->p.i2t;
        p.dim_in = (int)w0->shape[1];
        p.middle = (int)w0->shape[0];
        p.dim_out = (int)wo->shape[0];
        p.n_layer = nl;
        for (int i = 0; i < nl; ++i) {
            const std::string b = "layers." + std::to_string(i) + ".0.";
            const bf16_t* m;
            if ((rc = L.mat<bf16_t>(b + "weight", p.middle, i == 0 ? p.dim_in : p.middle, &m)) ||
                (rc = L.vec(b + "bias", p.middle, &p.b[i])))
                return fail(rc);
            p.w[i] = m;
        }
        const bf16_t* m;
        if ((rc = L.mat<bf16_t>("fc_out.weight", p.dim_out, p.middle, &m)) || (rc = L.vec("fc_out.bias", p.dim_out, &p.out_b)))
            return fail(rc);
        p.out_w = m;
    }
    {
        Weights W(fuse, n_fuse);
        Loader L{W, k->mem, what};
        if ((rc = load_crossformer(L, W, k->fuse, &k->p.fuse))) return fail(rc);
    }
    {
        Weights W(cond, n_cond);
        Loader L{W, k->mem, what};
        if ((rc = load_crossformer(L, W, k->cond, &k->p.cond))) return fail(rc);
    }
    // same re-arrangement as the torch facade builds (keds_amd.CrossFormer.params): both then launch the same kernels on
    // the same bits
    for (int which = 0; which < 2; ++which) {
        keds_crossformer_params* xp = which == 0 ? &k->p.fuse : &k->p.cond;
        keds_crossformer_fused* xf = which == 0 ? &k->fuse_f : &k->cond_f;
        if (xp->layers > 8) continue;
        const size_t bytes = keds_crossformer_fused_bytes(xp);
        void* buf = k->mem.alloc(bytes);
        if (!buf) {
            keds_set_error("%s: out of device memory", what);
            return fail(KEDS_E_LAUNCH);
        }
        if ((rc = keds_crossformer_fuse(xp, buf, bytes, xf, nullptr))) return fail(rc);
        xp->fused = xf;
    }
    HIP_TRY(hipStreamSynchronize(nullptr), what);
    *out = k;
    return KEDS_OK;
}

extern "C" int keds_knowledge_destroy(keds_knowledge* kn) {
    if (kn) {
        (void)hipSetDevice(kn->device);
        delete kn;
    }
    return KEDS_OK;
}

extern "C" int keds_knowledge_forward(keds_knowledge* kn, const float* q, const float* nbr_img, const float* nbr_txt, int B,
                                      int K, void* tokens_out, void* stream) {
    const char* what = "keds_knowledge_forward";
    KEDS_REQUIRE(kn && q && nbr_img && nbr_txt && tokens_out && B > 0 && K > 0, "%s: bad argument", what);
    int rc;
    const size_t need = keds_knowledge_workspace_bytes(&kn->p, B, K);
    KEDS_REQUIRE(need > 0, "%s: unsupported shape (B %d, K %d)", what, B, K);
    if ((rc = kn->ws.reserve(need, (hipStream_t)stream, what))) return rc;
    return keds_knowledge_run(&kn->p, q, nbr_img, nbr_txt, B, K, (float*)tokens_out, kn->ws.p, kn->ws.bytes, stream);
}

// ---- index ----------------------------------------------------------------------------------------------
extern "C" int keds_index_create(keds_ctx* ctx, int dim, int metric, int storage, keds_index** out) {
    const char* what = "keds_index_create";
    KEDS_REQUIRE(out != nullptr, "%s: null out", what);
    KEDS_REQUIRE(metric == KEDS_METRIC_L2 || metric == KEDS_METRIC_IP, "%s: unknown metric", what);
    KEDS_REQUIRE(storage == KEDS_BF16, "%s: the scan image is bf16 (KEDS_BF16)", what);
    KEDS_REQUIRE(keds_index_packed_bytes(32, dim) > 0, "%s: unsupported dimension %d", what, dim);
    int rc = use_device(ctx, what);
    if (rc) return rc;
    keds_index* idx = new keds_index();
    idx->ctx = ctx;
    idx->device = ctx->device;
    idx->dim = dim;
    idx->metric = metric;
    *out = idx;
    return KEDS_OK;
}

extern "C" int keds_index_destroy(keds_index* idx) {
    if (idx) {
        (void)hipSetDevice(idx->device);
        if (idx->rows) (void)hipFree(idx->rows);
        if (idx->packed) (void)hipFree(idx->packed);
        delete idx;
    }
    return KEDS_OK;
}

extern "C" int64_t keds_index_ntotal(const keds_index* idx) { return idx ? idx->n : -1; }

extern "C" int keds_index_set_base(keds_index* idx, int64_t row0) {
    KEDS_REQUIRE(idx && row0 >= 0, "keds_index_set_base: bad argument");
    idx->row0 = row0;
    return KEDS_OK;
}

extern "C" int keds_index_add(keds_index* idx, const float* rows, int64_t n) {
    // Appends in place (the Python facade's FlatIndex.add does the same): the fp32 rows and the scan image live in buffers
    // that grow geometrically, only the new rows are copied and only the new 32-row stages are packed
    // (keds_index_pack_append) -- amortised O(rows added), where round 2 re-allocated, re-copied and re-packed the whole
    // database and synchronised the device twice on every call (O(N^2) over a chunked build).  Work is enqueued on the
    // null stream; the call returns once the caller's `rows` have been consumed (pageable host copies are synchronous,
    // device sources are waited for with one stream synchronisation).
    const char* what = "keds_index_add";
    KEDS_REQUIRE(idx && rows && n > 0, "%s: bad argument", what);
    int rc = use_device(idx->ctx, what);
    if (rc) return rc;
    const int64_t total = idx->n + n;
    const size_t row_bytes = (size_t)idx->dim * sizeof(float);
    if (total > idx->cap) {
        // growth (log N times over a build): new buffers, the old rows and image stages copied across; hipFree of the old
        // pair waits for the searches still reading them
        const int64_t cap = total > 2 * idx->cap ? total : 2 * idx->cap;
        float* grown = nullptr;
        void* packed = nullptr;
        HIP_TRY(hipMalloc((void**)&grown, (size_t)cap * row_bytes), what);
        hipError_t e = hipMalloc(&packed, keds_index_packed_bytes(cap, idx->dim));
        if (e == hipSuccess && idx->n)
            e = hipMemcpyAsync(grown, idx->rows, (size_t)idx->n * row_bytes, hipMemcpyDeviceToDevice, nullptr);
        if (e == hipSuccess && idx->n)       // whole stages of the old image; the stage idx->n falls into is rewritten below
            e = hipMemcpyAsync(packed, idx->packed, keds_index_packed_bytes(idx->n, idx->dim), hipMemcpyDeviceToDevice, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) {
            (void)hipFree(grown);
            if (packed) (void)hipFree(packed);
            keds_set_error("%s: %s", what, hipGetErrorString(e));
            return KEDS_E_LAUNCH;
        }
        if (idx->rows) (void)hipFree(idx->rows);
        if (idx->packed) (void)hipFree(idx->packed);
        idx->rows = grown;
        idx->packed = packed;
        idx->cap = cap;
    }
    {   // a DEVICE source may still be being written on a non-blocking stream of the caller (every torch.cuda.Stream is one;
        // the null stream does not order behind those): the API has no stream argument, so wait for the device once
        // (keds_session.h states the contract).  Host sources need nothing.
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, rows) == hipSuccess && at.type == hipMemoryTypeDevice)
            HIP_TRY(hipDeviceSynchronize(), what);
        else
            (void)hipGetLastError();                              // (an unregistered host pointer reports an error: cleared)
    }
    HIP_TRY(hipMemcpyAsync(idx->rows + (size_t)idx->n * idx->dim, rows, (size_t)n * row_bytes, hipMemcpyDefault, nullptr), what);
    if ((rc = keds_index_pack_append(idx->rows, idx->n, total, idx->dim, idx->metric, idx->packed, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr), what);       // `rows` may be reused by the caller; the image is complete
    idx->n = total;
    return KEDS_OK;
}

extern "C" int keds_index_image(const keds_index* idx, void* packed_out, size_t bytes) {
    const char* what = "keds_index_image";
    KEDS_REQUIRE(idx && packed_out, "%s: bad argument", what);
    KEDS_REQUIRE(idx->n > 0, "%s: the index is empty", what);
    KEDS_REQUIRE(bytes >= keds_index_packed_bytes(idx->n, idx->dim), "%s: buffer smaller than keds_index_packed_bytes(ntotal, dim)", what);
    int prev = -1;                                                // the caller's current device is left as it was
    (void)hipGetDevice(&prev);
    HIP_TRY(hipSetDevice(idx->device), what);
    const hipError_t e = hipMemcpy(packed_out, idx->packed, keds_index_packed_bytes(idx->n, idx->dim), hipMemcpyDefault);
    if (prev >= 0 && prev != idx->device) (void)hipSetDevice(prev);
    HIP_TRY(e, what);
    return KEDS_OK;
}

static int index_search_local(keds_index* idx, const float* q, int nq, int k, float* D, int64_t* I, float* rows_out,
                              hipStream_t st, const char* what) {
    KEDS_REQUIRE(idx->n > 0, "%s: the index is empty", what);
    KEDS_REQUIRE(k >= 1 && k <= KEDS_SCAN_MAX_K, "%s: k must be in [1,%d] (got %d)", what, KEDS_SCAN_MAX_K, k);
    const size_t need = keds_index_search_workspace_bytes_ex(nq, idx->dim, idx->n, k);
    int rc = idx->ws.reserve(need, st, what);
    if (rc) return rc;
    return keds_index_search_packed(idx->packed, idx->rows, idx->n, idx->dim, idx->metric, q, nq, 0, k, idx->row0, D, I,
                                    rows_out, idx->ws.p, idx->ws.bytes, st);
}

extern "C" int keds_index_search(keds_index* idx, const void* q, int B, int k, float* D, int64_t* I, void* rows_out,
                                 void* stream) {
    const char* what = "keds_index_search";
    KEDS_REQUIRE(idx && q && D && I && B > 0, "%s: bad argument", what);
    return index_search_local(idx, (const float*)q, B, k, D, I, (float*)rows_out, (hipStream_t)stream, what);
}

// ---- communicator ---------------------------------------------------------------------------------------
extern "C" int keds_comm_unique_id(void* id_out) {
    KEDS_REQUIRE(id_out != nullptr, "keds_comm_unique_id: null out");
    int rc = rccl_load();
    if (rc) return rc;
    CommId id;
    if ((rc = rccl_check(g_rccl.GetUniqueId(&id), "keds_comm_unique_id"))) return rc;
    memcpy(id_out, id.bytes, KEDS_COMM_ID_BYTES);
    return KEDS_OK;
}

extern "C" int keds_comm_init(keds_ctx* ctx, int rank, int world, const void* unique_id) {
    const char* what = "keds_comm_init";
    KEDS_REQUIRE(ctx && unique_id && world >= 1 && rank >= 0 && rank < world, "%s: bad argument", what);
    KEDS_REQUIRE(ctx->comm == nullptr, "%s: the context already has a communicator", what);
    int rc = use_device(ctx, what);
    if (rc) return rc;
    if ((rc = rccl_load())) return rc;
    CommId id;
    memcpy(id.bytes, unique_id, KEDS_COMM_ID_BYTES);
    void* comm = nullptr;
    if ((rc = rccl_check(g_rccl.CommInitRank(&comm, world, id, rank), what))) return rc;
    ctx->comm = comm;
    ctx->rank = rank;
    ctx->world = world;
    return KEDS_OK;
}

extern "C" int keds_index_search_sharded(keds_index* idx, const void* q, int B, int k, float* D, int64_t* I, void* rows_out,
                                         void* stream) {
    // all-gather of the queries -> local exact search (+ row gather) of all B*world queries -> ONE all-to-all of the packed
    // partial lists (keds_exchange_pack: block w = what this shard found for rank w's queries, with the winners' rows when
    // rows_out is given: SURVEY 8e option B) -> merge of this rank's B queries keyed on (distance, id) (keds_exchange_merge).
    // Two collectives and k <= KEDS_SCAN_MAX_K, like the torch-hosted PackedExchange (round 2: three all-gathers, every
    // rank merged every query, k <= 16, no rows).
    const char* what = "keds_index_search_sharded";
    KEDS_REQUIRE(idx && q && D && I && B > 0 && k >= 1 && k <= KEDS_SCAN_MAX_K, "%s: bad argument", what);
    keds_ctx* ctx = idx->ctx;
    hipStream_t st = (hipStream_t)stream;
    const int W = ctx->world;
    if (W == 1 && !ctx->comm) return index_search_local(idx, (const float*)q, B, k, D, I, (float*)rows_out, st, what);
    KEDS_REQUIRE(ctx->comm != nullptr, "%s: call keds_comm_init first", what);
    KEDS_REQUIRE((long)W * k <= 4096, "%s: world * k = %ld exceeds 4096", what, (long)W * k);
    const int nq = B * W, dim = idx->dim;
    const int E = rows_out ? dim + 4 : 3;
    const size_t part = (size_t)B * k * E;                                   // int32 words per peer
    // exchange buffers: q_all [nq,dim] f32 | Dp [nq,k] f32 | Ip [nq,k] i64 | Rp [nq,k,dim] f32 | send [W][part] | recv [W][part]
    const size_t qb = keds_align_up((size_t)nq * dim * 4, 256), db = keds_align_up((size_t)nq * k * 4, 256),
                 ib = keds_align_up((size_t)nq * k * 8, 256), rb = rows_out ? keds_align_up((size_t)nq * k * dim * 4, 256) : 0,
                 xb = keds_align_up((size_t)W * part * 4, 256);
    int rc = idx->xws.reserve(qb + db + ib + rb + 2 * xb, st, what);
    if (rc) return rc;
    char* p = (char*)idx->xws.p;
    float* q_all = (float*)p;
    float* Dp = (float*)(p + qb);
    int64_t* Ip = (int64_t*)(p + qb + db);
    float* Rp = rows_out ? (float*)(p + qb + db + ib) : nullptr;
    int32_t* send = (int32_t*)(p + qb + db + ib + rb);
    int32_t* recv = (int32_t*)(p + qb + db + ib + rb + xb);
    if ((rc = rccl_check(g_rccl.AllGather(q, q_all, (size_t)B * dim * 4, /*ncclInt8*/ 0, ctx->comm, st), what))) return rc;
    if ((rc = index_search_local(idx, q_all, nq, k, Dp, Ip, Rp, st, what))) return rc;
    if ((rc = keds_exchange_pack(Dp, Ip, Rp, W, B, k, dim, (int64_t)part, send, stream))) return rc;
    if (g_rccl.AllToAll) {
        if ((rc = rccl_check(g_rccl.AllToAll(send, recv, part, /*ncclInt32*/ 2, ctx->comm, st), what))) return rc;
    } else {
        if ((rc = rccl_check(g_rccl.GroupStart(), what))) return rc;
        for (int w = 0; w < W; ++w) {
            int e1 = g_rccl.Send(send + (size_t)w * part, part, 2, w, ctx->comm, st);
            int e2 = g_rccl.Recv(recv + (size_t)w * part, part, 2, w, ctx->comm, st);
            if (e1 || e2) {
                (void)g_rccl.GroupEnd();
                return rccl_check(e1 ? e1 : e2, what);
            }
        }
        if ((rc = rccl_check(g_rccl.GroupEnd(), what))) return rc;
    }
    return keds_exchange_merge(recv, W, B, k, dim, (int64_t)part, idx->metric, D, I, (float*)rows_out, stream);
}
