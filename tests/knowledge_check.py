"""Checks of the knowledge-stream kernels (keds_amd/csrc/knowledge.hip and cross_core_f32_kernel of f32path.hip) and of the ranking
kernels (keds_amd/csrc/metrics.hip), each alone: seeded cases at the kernels' edges, a float64 or integer reference on the inputs as the
kernel receives them, a bound per element derived from the kernel's own fp32 operations, and float32 / integer CPU models of the
kernels with deliberate mutations (tests/test_host_knowledge_check.py proves that the checks pass the models and catch every mutation).
The shape of tests/train_check.py, whose helpers it uses.  Plain torch and numpy; imports without a GPU.  No constant here was tuned on
a kernel's output.  u = 2^-24; `held` is train_check's  |got - ref| <= e (1 + 2 u_out) + u_out |ref| + 2^-126 (1 + m).

cross_attn_core_kernel (bf16; one query, K <= 32 keys, head dim 64 on the lanes): the operation of train.hip's cross_core_fwd, so
    train_check.core_reference(...)["out"]:  e = (P rho) |v| + (K + 1) u P |v|,  m = sum |v|, output bf16.
    Kp / Vp rows have stride kv_ld; in the wide buffer of the fused form (kv_ld = 6 inner) K sits at column 2 l inner and V at
    (2 l + 1) inner, every other column NaN.
cross_core_f32_kernel (fp32; K <= 64; ONE pass with a running maximum): the same reference with u_out = 2^-24, and rho grows by what
    the rescales add.  A row rescales at most K - 1 times, each by expf(old max - new max) (relative error 2^-20 + 2 u |argument|, one
    multiplication each for sum and o: u twice); the arguments telescope to m_i - s_i0.  So
        rho += (K - 1) (2^-20 + 2 u) + 2 u (m_i - s_i0).
    `ramp` makes (nearly) K - 1 rescales; `ramp_down` (the keys of `ramp` reversed) none.
fold_qo_kernel: W' = Wq_l Wo_{l-1} against the float64 sum over the bf16 weights: e = (dim + 1) u sum |wq| |wo| (dim products, dim
    additions, sequential), output bf16;  b' = Wq_l bo_{l-1} + bq_l: e = (dim / 64 + 9) u (sum |wq bo| + |bq|) (a lane's chain in
    strides of 64, six butterfly steps, the product's rounding, one more addition), output fp32.  `integer` regime (weights in
    {-2 ... 2}, integer biases, every sum below 2^24): W' the bf16 rounding of the exact sum and b' the exact sum, to the bit.
dist_kernel: against 1 - ref gal^T in float64: e = (dim + 1) u sum |ref| |gal| + u |1 - acc| (an fma chain over dim, one
    subtraction); `integer` regime (entries in {-2 ... 2}) to the bit.
To the bit: pack_rows (torch.cat([q, ni, nt]).bfloat16(), row_check's cast specials among the data), place_token, concat_rows (rows
    {Wk_0, Wv_0, Wk_1, ...}, biases likewise), the ordering (argsort of the uint64 keys orderable(stored dist bits) << 32 | column:
    -0 before +0, a NaN where its sign bit puts it), cirr_rank and its counts (drop every ranked entry whose id is the reference id,
    then the index of the first entry with the target id, or -1), label_hits / total (numpy sums)."""
import math

import numpy as np
import torch

from tests import attention_check as ac
from tests import row_check as rc
from tests import train_check as tc
from tests.train_check import _butterfly, _chain, _collect, _exp32, _gen, _seq, held, same_bits  # noqa: F401  (re-exported)

U, U_FN, SENT = tc.U, tc.U_FN, tc.SENT
BF, F32, F64 = tc.BF, tc.F32, tc.F64
FLUSH = tc.FLUSH

CORE_K = (1, 2, 15, 16, 17, 31, 32)
CORE_F32_K = (1, 2, 31, 32, 33, 63, 64)
CORE_BH = ((1, 1), (3, 3), (5, 8))
CORE_REGIMES = ac.REGIMES
CORE_F32_REGIMES = ac.REGIMES + ("ramp_down",)
WIDE_LAYERS, WIDE_L = 3, (0, 2)                      # kv_ld = 6 inner; the layers whose columns a case reads
CORE_MUTATIONS = ("droplast", "kv_ld_inner", "v_at_k", "no_scale", "unnormalised", "drop_store")
CORE_F32_MUTATIONS = ("droplast", "v_at_k", "no_scale", "unnormalised", "drop_store", "o_not_rescaled")

PACK_B, PACK_K, PACK_DIMS = (1, 3, 33), (1, 16), (128, 768)
# (B, K, dim) beside the table: a workgroup packs 2048 elements; B (1 + 2 K) dim = 2056 (one 8-group into a second workgroup), 2040
# (one short of a full one) and 3 x 2048 + 24
PACK_EXTRA = ((1, 128, 8), (17, 7, 8), (1, 128, 24))
FUSE_SHAPES = ((128, 128), (128, 256), (256, 128), (768, 768))     # (dim, inner)
FUSE_LAYERS = (1, 2, 3, 8)
FUSE_REGIMES = ("random", "integer")
FUSE_MUTATIONS = ("wo_transposed", "no_bq", "bo_i", "cols_256_unwritten", "wk_wv_swapped", "bias_slot_plus1")
PACK_MUTATIONS = ("blocks_swapped", "last_group_unwritten", "stride_dim")

RANK_NG = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 8191, 8192, 8193, 16384, 16385, 24577)
RANK_NQ = (1, 3, 63, 64, 65)
RANK_DIMS = (1, 15, 16, 17, 64, 100)
RANK_REGIMES = ("random", "integer", "duplicates", "specials")
SORT_CHUNK = 8192
SORT_MUTATIONS = ("ties_larger_index", "neg_zero_is_zero", "pad_listed", "lone_run_dropped", "lone_run_duplicated")
CIRR_NG = (1, 63, 64, 65, 129, 200)
CIRR_NQ = (1, 3, 4, 5)
CIRR_MUTATIONS = ("earlier_refs_kept", "later_refs_subtracted", "target_eq_ref_counted")
LABEL_NK = (1, 3, 8)
LABEL_MUTATIONS = ("i_le_k", "butterfly_short")


def rank_pairs():
    """(ng, nq, dim) pairwise, not the full cross: every ng with every nq it may meet (nq <= 3 above 8192), every dim with every
    nq, and every dim on both sides of the 8192-column chunk"""
    out = []
    for i, ng in enumerate(RANK_NG):
        nqs = [n for n in RANK_NQ if ng <= SORT_CHUNK or n <= 3]
        for j, nq in enumerate(nqs):
            out.append((ng, nq, RANK_DIMS[(i + j) % len(RANK_DIMS)]))
    for k, dim in enumerate(RANK_DIMS):                   # every dim with nq around the 64-row tile
        for j, nq in enumerate((63, 64, 65)):
            t = ((64, 65, 257)[(k + j) % 3], nq, dim)
            if t not in out:
                out.append(t)
    out.append((16385, 1, 64))                            # (the one dim the cycle above leaves out beyond 8192)
    return out


# ---- the cross-attention cores ------------------------------------------------------------------------------------------------------
def core_inputs(B, K, H, regime, dtype, seed):
    """Q [B, d], Kp, Vp [B K, d] of `dtype` in attention_check's regimes; ramp_down: the keys (and values) of ramp reversed"""
    qkv = ac.make_qkv(B, K, H, "ramp" if regime == "ramp_down" else regime, dtype, seed)
    d = 64 * H
    Q, Kp, Vp = qkv[::K, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    if regime == "ramp_down":
        Kp, Vp = (t.reshape(B, K, d).flip(1).reshape(B * K, d) for t in (Kp, Vp))
    return Q.contiguous(), Kp.contiguous(), Vp.contiguous()


def wide(Kp, Vp, layer, layers=WIDE_LAYERS):
    """-> (buffer [B K, layers 2 inner] NaN but for layer `layer`'s k | v, column of K, column of V)"""
    rows, inner = Kp.shape
    buf = torch.full((rows, layers * 2 * inner), float("nan"), dtype=Kp.dtype)
    ko, vo = 2 * layer * inner, (2 * layer + 1) * inner
    buf[:, ko:ko + inner] = Kp
    buf[:, vo:vo + inner] = Vp
    return buf, ko, vo


def core_reference(Q, Kp, Vp, B, K, H, f32=False):
    """-> (ref, e, m) float64 [B, d]"""
    q, k, v = tc._split_heads(Q, B, 1, H), tc._split_heads(Kp, B, K, H), tc._split_heads(Vp, B, K, H)
    ref, e, m = tc.core_reference(q, k, v, torch.zeros_like(q))["out"]
    if f32:
        s = q @ k.transpose(-1, -2) / 8
        P = torch.softmax(s, -1)
        extra = (K - 1) * (U_FN + 2 * U) + 2 * U * (s.amax(-1, keepdim=True) - s[..., :1])
        e = e + extra * (P @ v.abs())
    return tuple(tc._merge_heads(t) for t in (ref, e, m))


def core_failures(R, out, what=""):
    f = held(out, R[0], R[1], out.dtype, what, R[2])
    return ([f] if f else []), f.worst


def core_applicable(mutation, K, kv_ld, inner):
    if mutation == "kv_ld_inner":
        return kv_ld != inner
    if mutation in ("droplast", "no_scale", "unnormalised", "o_not_rescaled"):
        return K >= 2
    return True


def core_model(Q, buf, ko, vo, B, K, H, f32=False, order="forward", mutation=None, at=(0, 0)):
    """cross_attn_core_kernel / cross_core_f32_kernel in float32 on the kernel's own indexing of the row buffer `buf` [B K, kv_ld]"""
    inner, ld = 64 * H, buf.shape[1]
    flat = buf.float().reshape(-1)
    stride = inner if mutation == "kv_ld_inner" else ld
    b, h, lane = torch.arange(B).view(B, 1, 1), torch.arange(H).view(1, H, 1), torch.arange(64).view(1, 1, 64)

    def row(off, j):
        return flat[(b * K + j) * stride + off + h * 64 + lane]

    if mutation == "v_at_k":
        vo = ko
    q = Q.float().reshape(B, H, 64)
    Kn = K - 1 if mutation == "droplast" else K
    scale = 1.0 if mutation == "no_scale" else 0.125
    if not f32:
        sc = [_butterfly(q * row(ko, j), order) * scale for j in range(Kn)]
        mx = torch.stack(sc).amax(0)
        p = [_exp32(s - mx) for s in sc]
        sm, o = _seq(p), _seq([p[j] * row(vo, j) for j in range(Kn)])
    else:
        q = q * scale
        mx, sm, o = torch.full((B, H, 1), float("-inf")), torch.zeros(B, H, 1), torch.zeros(B, H, 64)
        for j in range(Kn):
            sj = _butterfly(q * row(ko, j), order)
            new = sj > mx
            f = torch.where(new, torch.exp(mx - sj), torch.ones_like(sj))
            sm = sm * f
            if mutation != "o_not_rescaled":
                o = o * f
            mx = torch.where(new, sj, mx)
            e = torch.exp(sj - mx)
            sm = sm + e
            o = (e.double() * row(vo, j).double() + o.double()).float()             # fmaf
    out = (o if mutation == "unnormalised" else o / sm).reshape(B, inner).to(F32 if f32 else BF)
    if mutation == "drop_store":
        out[at] = SENT
    return out


# ---- pack_rows, place_token -----------------------------------------------------------------------------------------------------------
def pack_inputs(B, K, dim, seed):
    """q [B, dim], nbr_img, nbr_txt [B K, dim] fp32 with the cast specials at the head and the tail of each"""
    g = _gen(seed, B, K, dim, 11)
    sp = rc.cast_specials(F32)
    outs = []
    for rows in (B, B * K, B * K):
        x = torch.randn(rows * dim, generator=g)
        n = min(sp.numel(), x.numel() // 2)
        x[:n] = sp[:n]
        x[x.numel() - n:] = sp[:n].flip(0)
        outs.append(x.reshape(rows, dim))
    return outs


def pack_model(q, ni, nt, mutation=None):
    out = torch.cat([q, nt, ni] if mutation == "blocks_swapped" else [q, ni, nt]).bfloat16().reshape(-1)
    if mutation == "last_group_unwritten":
        out[-8:] = SENT
    return out.reshape(-1, q.shape[1])


def place_model(src, tokens, slot, nslots, mutation=None):
    """tokens [B, nslots, dim] (prefilled) with src [B, dim] in `slot`"""
    B, dim = src.shape
    out = tokens.clone().reshape(-1)
    b, j = torch.arange(B).view(B, 1), torch.arange(dim).view(1, dim)
    out[((b + slot) if mutation == "stride_dim" else (b * nslots + slot)) * dim + j] = src
    return out.reshape(B, nslots, dim)


# ---- keds_crossformer_fuse: concat_rows, fold_qo ------------------------------------------------------------------------------------------
def fuse_inputs(dim, inner, layers, regime, seed):
    """per layer: wq, wk, wv bf16 [inner, dim], wo bf16 [dim, inner], bq, bk, bv fp32 [inner], bo fp32 [dim]"""
    g = _gen(seed, dim, inner, layers, regime)
    out = []
    for _ in range(layers):
        L = {}
        for n, shape in (("wq", (inner, dim)), ("wk", (inner, dim)), ("wv", (inner, dim)), ("wo", (dim, inner))):
            w = torch.randint(-2, 3, shape, generator=g).float() if regime == "integer" else torch.randn(shape, generator=g) / math.sqrt(shape[1])
            L[n] = w.bfloat16()
        for n, k in (("bq", inner), ("bk", inner), ("bv", inner), ("bo", dim)):
            L[n] = torch.randint(-8, 9, (k,), generator=g).float() if regime == "integer" else 0.1 * torch.randn(k, generator=g)
        out.append(L)
    return out


def _al(n):
    return (n + 255) // 256 * 256


def fuse_layout(dim, inner, layers):
    """byte offsets of the buffer keds_crossformer_fuse fills -> dict(wkv, bkv, wqn {l}, bqn {l}, total) of (offset, bytes)"""
    off, lay = 0, {"wqn": {}, "bqn": {}}

    def take(nbytes):
        nonlocal off
        r = (off, nbytes)
        off += _al(nbytes)
        return r
    lay["wkv"] = take(layers * 2 * inner * dim * 2)
    lay["bkv"] = take(layers * 2 * inner * 4)
    for l in range(1, layers):
        lay["wqn"][l] = take(inner * inner * 2)
        lay["bqn"][l] = take(inner * 4)
    lay["total"] = off
    return lay


def fuse_reference(Ls):
    """-> dict(wkv bf16, bkv fp32 (both to the bit), wqn {l: (ref, e)}, bqn {l: (ref, e)}) float64"""
    dim = Ls[0]["wq"].shape[1]
    R = {"wkv": torch.cat([t for L in Ls for t in (L["wk"], L["wv"])]), "bkv": torch.cat([t for L in Ls for t in (L["bk"], L["bv"])]),
         "wqn": {}, "bqn": {}}
    for l in range(1, len(Ls)):
        wq, wo, bo, bq = Ls[l]["wq"].double(), Ls[l - 1]["wo"].double(), Ls[l - 1]["bo"].double(), Ls[l]["bq"].double()
        R["wqn"][l] = (wq @ wo, (dim + 1) * U * (wq.abs() @ wo.abs()))
        R["bqn"][l] = (wq @ bo + bq, (dim / 64 + 9) * U * ((wq * bo).abs().sum(1) + bq.abs()))
    return R


def fuse_failures(R, got, exact, what=""):
    """got: dict like fuse_model's.  exact (`integer`): W' is the bf16 rounding of the exact sum and b' the exact sum, to the bit"""
    fs = [same_bits(got["wkv"], R["wkv"], what + " wkv"), same_bits(got["bkv"], R["bkv"], what + " bkv")]
    for l in R["wqn"]:
        (w, ew), (b, eb) = R["wqn"][l], R["bqn"][l]
        if exact:
            assert float(w.abs().max()) < 2 ** 24 and float(b.abs().max()) < 2 ** 24
            fs += [same_bits(got["wqn"][l], w.bfloat16(), f"{what} wqn[{l}]"), same_bits(got["bqn"][l], b.float(), f"{what} bqn[{l}]")]
        else:
            fs += [held(got["wqn"][l], w, ew, BF, f"{what} wqn[{l}]"), held(got["bqn"][l], b, eb, F32, f"{what} bqn[{l}]")]
    return [f for f in fs if f], max(f.worst for f in fs)


def fuse_applicable(mutation, dim, inner, layers):
    if mutation == "cols_256_unwritten":
        return layers >= 2 and inner > 256
    if mutation == "wk_wv_swapped":
        return True
    return layers >= 2


def fuse_model(Ls, order="forward", mutation=None):
    inner, dim = Ls[0]["wq"].shape
    kv = [(L["wv"], L["wk"]) if mutation == "wk_wv_swapped" else (L["wk"], L["wv"]) for L in Ls]
    bias = [t for L in Ls for t in (L["bk"], L["bv"])]
    if mutation == "bias_slot_plus1":
        bias = bias[-2:] + bias[:-2]
    got = {"wkv": torch.cat([t for p in kv for t in p]), "bkv": torch.cat(bias), "wqn": {}, "bqn": {}}
    for l in range(1, len(Ls)):
        wq, wo, bo, bq = Ls[l]["wq"].float(), Ls[l - 1]["wo"].float(), Ls[l - 1]["bo"], Ls[l]["bq"]
        if mutation == "wo_transposed":
            wo = wo.reshape(inner, dim).t()
        a = torch.zeros(inner, inner)
        for d in (range(dim) if order == "forward" else reversed(range(dim))):
            a = a + wq[:, d, None] * wo[d]
        w = a.bfloat16()
        if mutation == "cols_256_unwritten":
            w[:, 256:] = SENT
        bsel = bo[torch.arange(inner) % dim].view(inner, 1).expand(inner, dim) if mutation == "bo_i" else bo
        b = _chain(wq * bsel, order)[:, 0]
        got["wqn"][l] = w
        got["bqn"][l] = b if mutation == "no_bq" else b + bq
    return got


# ---- dist ---------------------------------------------------------------------------------------------------------------------------------
def _unit(x):
    return torch.nn.functional.normalize(x, dim=1)


def rank_inputs(nq, ng, dim, regime, seed):
    """ref [nq, dim], gal [ng, dim] fp32"""
    g = _gen(seed, nq, ng, dim, regime)
    if regime == "integer":
        return torch.randint(-2, 3, (nq, dim), generator=g).float(), torch.randint(-2, 3, (ng, dim), generator=g).float()
    ref, gal = _unit(torch.randn(nq, dim, generator=g)), _unit(torch.randn(ng, dim, generator=g))
    if regime == "duplicates":
        gal = _unit(torch.randn(7, dim, generator=g))[torch.randint(0, 7, (ng,), generator=g)]
    elif regime == "specials":
        # rows cycled over the gallery (the last ones win where it is short): +-3e38 along query 0's signs (its dot overflows for
        # dim > 1: -inf / +inf; other queries may see inf - inf = NaN), a NaN row, query 0 itself (distance +0 or an ulp)
        big = 3e38 * torch.where(ref[0] < 0, -1.0, 1.0)
        rows = [big, -big, torch.full((dim,), float("nan")), ref[0].clone()]
        for i, r in enumerate(rows):
            gal[(ng // 2 + i) % ng] = r
    elif regime != "random":
        raise ValueError(regime)
    return ref, gal


def dist_reference(ref, gal):
    """-> (1 - ref gal^T, e) float64"""
    acc = ref.double() @ gal.double().t()
    return 1 - acc, (ref.shape[1] + 1) * U * (ref.double().abs() @ gal.double().abs().t()) + U * (1 - acc).abs()


def dist_failures(ref, gal, dist, exact, what=""):
    """dist fp32 [nq, ng] as the launch stored it.  A gallery row with a NaN must give NaN.  A row with an entry beyond 2^100 (the
    +-3e38 rows of `specials`) has no fp32 value to be held to -- a partial sum may overflow where the float64 sum does not, and
    inf - inf is NaN -- so any bits pass there; the ordering is held to the stored bits whatever they are."""
    want, e = dist_reference(ref, gal)
    if exact:
        return same_bits(dist, want.float(), what + " dist")
    ratio = (dist.double() - want).abs() / (e + FLUSH)
    nan = torch.isnan(gal).any(1)[None, :].expand_as(ratio)
    big = (gal.abs().nan_to_num(0.0).amax(1) >= 2.0 ** 100)[None, :].expand_as(ratio)
    ratio = torch.where(big, torch.zeros_like(ratio), ratio)
    ratio = torch.where(nan, torch.where(torch.isnan(dist), 0.0, float("inf")).double(), ratio)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return _collect(ratio, what + " dist")


def dist_model(ref, gal, order="forward", mutation=None):
    """dist_kernel's fma chain over dim (tiles of 16 in turn), then 1 - acc"""
    dim = ref.shape[1]
    n = dim - dim % 16 if mutation == "tail_dropped" else dim
    acc = torch.zeros(ref.shape[0], gal.shape[0])
    for k in (range(n) if order == "forward" else reversed(range(n))):
        acc = (ref[:, k, None].double() * gal[None, :, k].double() + acc.double()).float()
    return 1.0 - acc


# ---- the ordering -------------------------------------------------------------------------------------------------------------------------
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)


def orderable(bits):
    bits = bits.astype(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def sort_keys(dist, mutation=None):
    """dist: numpy float32 [nq, ng] -> uint64 keys"""
    bits = np.ascontiguousarray(dist).view(np.uint32)
    if mutation == "neg_zero_is_zero":
        bits = np.where(bits == np.uint32(0x80000000), np.uint32(0), bits)
    col = np.arange(dist.shape[1], dtype=np.uint64)[None, :]
    if mutation == "ties_larger_index":
        col = np.uint64(0xFFFFFFFF) - col
    return (orderable(bits).astype(np.uint64) << np.uint64(32)) | col


def order_reference(dist):
    """numpy float32 [nq, ng] (the stored distances) -> int32 [nq, ng]"""
    return np.argsort(sort_keys(dist), axis=1, kind="stable").astype(np.int32)


def order_failures(dist, order, what=""):
    return same_bits(torch.from_numpy(np.ascontiguousarray(order)), torch.from_numpy(order_reference(dist)), what + " order")


def _bitonic(keys):
    """the compare-exchange network of sort_rows_kernel / sort_chunk_keys_kernel on [rows, P] (P a power of two), in place"""
    P = keys.shape[1]
    i = np.arange(P)
    k = 2
    while k <= P:
        j = k >> 1
        while j > 0:
            l = i ^ j
            m = l > i
            lo, hi, up = i[m], l[m], (i[m] & k) == 0
            a, b = keys[:, lo], keys[:, hi]
            swap = (a > b) == up[None, :]
            keys[:, lo], keys[:, hi] = np.where(swap, b, a), np.where(swap, a, b)
            j >>= 1
        k <<= 1
    return keys


def sort_model(dist, mutation=None, chunk=SORT_CHUNK):
    """keds_rank_gallery behind dist_kernel: a bitonic sort in a padded power of two up to `chunk` columns; beyond, bitonic sorts of
    `chunk`-column runs and pairwise merges by rank (own offset + number of smaller keys in the other run), the last run alone
    where the runs are odd in number.  -> int32 [nq, ng]"""
    nq, ng = dist.shape
    keys = sort_keys(dist, mutation)
    pad = np.uint64(0) if mutation == "pad_listed" else PAD
    low = np.uint64(0xFFFFFFFF)

    def cols(k):
        c = k & low
        return (low - c if mutation == "ties_larger_index" else c).astype(np.int64).astype(np.int32)

    if ng <= chunk:
        P = 1
        while P < ng:
            P <<= 1
        buf = np.full((nq, P), pad, dtype=np.uint64)
        buf[:, :ng] = keys
        return cols(_bitonic(buf)[:, :ng])
    a = np.zeros_like(keys)
    for c0 in range(0, ng, chunk):
        n = min(chunk, ng - c0)
        buf = np.full((nq, chunk), pad, dtype=np.uint64)
        buf[:, :n] = keys[:, c0:c0 + n]
        a[:, c0:c0 + n] = _bitonic(buf)[:, :n]
    run = chunk
    while run < ng:
        out = np.zeros_like(a)
        for p0 in range(0, ng, 2 * run):
            al = min(run, ng - p0)
            b0 = p0 + al
            bl = max(0, min(run, ng - b0))
            if bl == 0 and mutation == "lone_run_dropped":
                continue
            if bl == 0 and mutation == "lone_run_duplicated":
                out[:, p0:p0 + al] = a[:, p0 - run:p0 - run + al]
                continue
            for q in range(nq):
                A, Bv = a[q, p0:b0], a[q, b0:b0 + bl]
                out[q, p0 + np.arange(al) + np.searchsorted(Bv, A, side="left")] = A
                out[q, p0 + np.arange(bl) + np.searchsorted(A, Bv, side="left")] = Bv
        a = out
        run *= 2
    return cols(a)


def sort_applicable(mutation, ng, chunk=SORT_CHUNK):
    if mutation == "pad_listed":
        return (ng & (ng - 1)) != 0 if ng <= chunk else ng % chunk != 0
    if mutation in ("lone_run_dropped", "lone_run_duplicated"):
        runs, lone = -(-ng // chunk), False
        while runs > 1:
            lone |= runs % 2 == 1
            runs = -(-runs // 2)
        return lone
    return ng >= 2


def sort_dist(nq, ng, regime, seed):
    """stored distances for the sort's own host test: `ties` (few distinct values), `zeros` (+-0 in plenty), `specials` (+-inf, NaNs
    of both signs, +-0 among random values)"""
    g = np.random.RandomState(seed % (2 ** 31))
    if regime == "ties":
        d = g.randint(-3, 4, (nq, ng)).astype(np.float32) / 4
        d[:, 0] = d[:, -1]                                                      # a tie of the first column with the last
        return d
    d = g.standard_normal((nq, ng)).astype(np.float32)
    if regime == "zeros":
        d = np.where(g.rand(nq, ng) < 0.5, np.float32(0.0), d)
        d = np.where(g.rand(nq, ng) < 0.5, -d, d).astype(np.float32)
        d[:, 0], d[:, -1] = 0.0, -0.0                                           # (-0 in the last column comes before +0 in the first)
        return d
    sp = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0xFFFFFFFF, 0, 0x80000000], dtype=np.uint32).view(np.float32)
    where = g.rand(nq, ng) < 0.3
    return np.where(where, sp[g.randint(0, 8, (nq, ng))], d).astype(np.float32)


# ---- cirr_rank ------------------------------------------------------------------------------------------------------------------------------
class CirrCase:
    """One launch: order int32 [nq, ng] (a permutation per query), gallery_ids [ng], ref_ids, target_ids [nq].
    Gallery items 0, 1, 2 share id 7 (three references at once), item 3 has id 8 (one reference), the rest distinct ids from 100.
    Scenarios, one per query, in turn: the target at rank 0, 63, 64 and ng - 1 (where the gallery has them) x 0, 1 or 3 references x
    placed before the target inside its 64-step, in an earlier step, behind it, or one of each (`mixed`) -- whatever fits; then the
    target id equal to the reference id, and the target absent."""

    def __init__(self, ng, nq=None, seed=0):
        g = np.random.RandomState(seed * 1000 + ng)
        self.ng = ng
        self.gallery_ids = np.array([7, 7, 7, 8][:ng] + list(range(100, 100 + max(0, ng - 4))), dtype=np.int32)
        scen = []
        for tpos in sorted({0, 63, 64, ng - 2, ng - 1} & set(range(ng))):            # (ng - 2: room for `mixed`)
            for nref in (0, 1, 3):
                for place in ("before", "earlier", "behind", "mixed"):
                    s = self._scenario(tpos, nref, place, g)
                    if s is not None and (nref or place == "before"):
                        scen.append(s + ((tpos, nref, place),))
        if ng >= 5:
            o = g.permutation(ng).astype(np.int32)
            scen.append((o, 8, 8, ("eq", 1, "")))                          # target id == reference id
            scen.append((o, 7, 7, ("eq", 3, "")))
            scen.append((o, 8, -9, ("absent", 1, "")))                      # target absent
            scen.append((o, -5, -9, ("absent", 0, "")))
        else:
            o = g.permutation(ng).astype(np.int32)
            scen.append((o, int(self.gallery_ids[0]), int(self.gallery_ids[0]), ("eq", 1, "")))
            scen.append((o, -5, -9, ("absent", 0, "")))
            scen.append((o, -5, int(self.gallery_ids[ng - 1]), ("plain", 0, "")))
        if nq is not None:
            scen = [scen[i % len(scen)] for i in range(nq)]
        self.nq = len(scen)
        self.order = np.stack([s[0] for s in scen]).astype(np.int32)
        self.ref_ids = np.array([s[1] for s in scen], dtype=np.int32)
        self.target_ids = np.array([s[2] for s in scen], dtype=np.int32)
        self.names = [s[3] for s in scen]

    def _scenario(self, tpos, nref, place, g):
        ng = self.ng
        if ng < 5 + nref:
            return None
        step0 = tpos // 64 * 64
        zones = {"before": list(range(step0, tpos)), "earlier": list(range(0, step0)), "behind": list(range(tpos + 1, ng))}
        if place == "mixed":
            if nref != 3 or not all(zones.values()):
                return None
            pos = [zones[z][g.randint(len(zones[z]))] for z in ("before", "earlier", "behind")]
        else:
            if len(zones[place]) < nref:
                return None
            pos = list(g.choice(zones[place], nref, replace=False)) if nref else []
        refs = {3: [0, 1, 2], 1: [3], 0: []}[nref]
        target = 4                                                          # id 100
        slots = np.full(ng, -1, dtype=np.int64)
        slots[tpos] = target
        for p, r in zip(pos, refs):
            slots[p] = r
        rest = [i for i in g.permutation(ng) if i != target and i not in refs]
        slots[slots < 0] = rest
        assert sorted(slots.tolist()) == list(range(ng))
        return slots.astype(np.int32), {3: 7, 1: 8, 0: -5}[nref], 100


def cirr_reference(order, gallery_ids, ref_ids, target_ids):
    """-> rank int32 [nq], counts int32 [nq, 2] (reference matches, target matches that are no reference matches)"""
    nq = order.shape[0]
    rank, counts = np.full(nq, -1, dtype=np.int32), np.zeros((nq, 2), dtype=np.int32)
    for q in range(nq):
        ids = gallery_ids[order[q]]
        kept = ids[ids != ref_ids[q]]
        hit = np.nonzero(kept == target_ids[q])[0]
        rank[q] = hit[0] if hit.size else -1
        counts[q] = ((ids == ref_ids[q]).sum(), (kept == target_ids[q]).sum())
    return rank, counts


def cirr_model(order, gallery_ids, ref_ids, target_ids, mutation=None):
    """cirr_rank_kernel: 64 ranked entries per step, ballots, the first target of a step minus the references before it"""
    nq, ng = order.shape
    rank, counts = np.full(nq, -1, dtype=np.int32), np.zeros((nq, 2), dtype=np.int32)
    for q in range(nq):
        removed = 0
        for base in range(0, ng, 64):
            ids = gallery_ids[order[q, base:base + 64]]
            is_ref = ids == ref_ids[q]
            is_tgt = (ids == target_ids[q]) & (True if mutation == "target_eq_ref_counted" else ~is_ref)
            if is_tgt.any() and rank[q] < 0:
                first = int(np.argmax(is_tgt))
                before = int(is_ref.sum() if mutation == "later_refs_subtracted" else is_ref[:first].sum())
                rank[q] = base + first - (0 if mutation == "earlier_refs_kept" else removed) - before
            removed += int(is_ref.sum())
            counts[q] += (int(is_ref.sum()), int(is_tgt.sum()))
    return rank, counts


# ---- label_hits -------------------------------------------------------------------------------------------------------------------------------
def label_inputs(nq, ng, seed):
    """order (a permutation per query), gallery labels in [0, 5), query labels in [0, 5) but the last query's, which no item has
    (with one query that one wins)"""
    g = np.random.RandomState(seed * 7919 + nq * 31 + ng)
    order = np.stack([g.permutation(ng) for _ in range(nq)]).astype(np.int32)
    ql, labels = g.randint(0, 5, nq).astype(np.int32), g.randint(0, 5, ng).astype(np.int32)
    ql[0] = labels[order[0, min(1, ng - 1)]]                                    # query 0 matches the item just behind cut-off 1
    ql[-1] = 77
    return order, labels, ql


def label_cutoffs(ng, nk):
    ks = [0, 1, 63, 64, 65, ng, ng + 7, 2][:nk] if nk == 8 else {1: [ng], 3: [0, 64, ng + 7]}[nk]
    return np.array(ks, dtype=np.int32)


def label_reference(order, labels, ql, ks):
    m = labels[order] == ql[:, None]
    hits = np.stack([m[:, :max(0, min(int(k), order.shape[1]))].sum(1) for k in ks], 1).astype(np.int32)
    return hits, m.sum(1).astype(np.int32)


def label_model(order, labels, ql, ks, mutation=None):
    """label_hits_kernel: lane l counts i = l, l + 64, ..., then the xor butterfly"""
    nq, ng = order.shape
    m = (labels[order] == ql[:, None]).astype(np.int64)
    i = np.arange(ng)
    steps = (32, 16, 8, 4, 2) if mutation == "butterfly_short" else (32, 16, 8, 4, 2, 1)

    def wave(x):                                       # [nq, ng] -> lane 0's value after the butterfly
        lanes = np.zeros((nq, 64), dtype=np.int64)
        np.add.at(lanes, (slice(None), i % 64), x)
        for o in steps:
            lanes = lanes + lanes[:, np.arange(64) ^ o]
        return lanes[:, 0]
    hits = np.stack([wave(m * ((i <= k) if mutation == "i_le_k" else (i < k))[None, :]) for k in ks], 1).astype(np.int32)
    return hits, wave(m).astype(np.int32)


def bits_np(got, want, what):
    return same_bits(torch.from_numpy(np.ascontiguousarray(got)), torch.from_numpy(np.ascontiguousarray(want)), what)
