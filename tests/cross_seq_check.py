"""Checks of the multi-query cross-attention core (cross_attn_seq_kernel, keds_amd/csrc/cross_seq.hip) alone: seeded cases at the
kernel's edges, a float64 reference on the rounded operands, a bound per element derived from the number formats, and a float32 CPU
model of the kernel's rounding ON THE KERNEL'S OWN INDEXING of its four buffers, with deliberate mutations
(tests/test_host_cross_seq_check.py proves that the bound passes the model and catches every mutation).  The shape of
tests/knowledge_check.py.  Plain torch; imports without a GPU.  No constant here was tuned on a kernel's output.

Operation (include/keds_hip.h, keds_cross_attn_seq): out[b, i, h] = softmax(Q[b, i, h] . K[b, :, h]^T / 8) . V[b, :, h], no mask,
dim_head 64, bf16.  Q rows [B Lq] of stride q_ld, Kp / Vp rows [B Lk] of stride kv_ld behind two pointers, out rows [B Lq] of stride
o_ld; head h at columns 64 h.

Cases: q is the q part of an attention_check.make_qkv draw over (B, Lq) rows, k and v the k and v parts of a second draw over (B, Lk)
rows, in attention_check's four regimes.  `ramp` (score grows with the key index: a zero pad key or a missing last key dominates the
row) and `flat` (every key weighs 1 / Lk and |o| ~ 2: a missing or extra key moves the row) are the regimes that expose pad and
missing keys; see attention_check.

Bound per element: attention_check's bound of the 16-bit kernels for bf16 (t = 0) with n_vis = Lk,
    |got - o| <= 1.05 * 2^-8 * (A + |o|) + 2^-20 * vmax,
o = softmax(s) v and A = softmax(s) |v| in float64 on the rounded operands, vmax = max |v| of the (sample, head): the probabilities
are rounded to bf16 (2^-8 A, the sum being taken over the unrounded ones), the output is rounded to bf16 (2^-8 |o|); 1.05 and 2^-20
cover second-order terms, fp32 accumulation and v_exp_f32.

Layout of a launch (layout()): K and V are two column ranges of one wide buffer [B Lk, 6 inner] (the fused CrossFormer layout at
layer 1: K at column 2 inner, V at 3 inner) whose other columns are NaN; Q sits at column 0 of a buffer of stride inner + 24 and out
of stride inner + 8 (so q_ld != o_ld != 64 heads), the columns beyond inner NaN (Q) / sentinel (out)."""
import torch

from keds_amd import _lib
from tests import attention_check as ac

DH = 64
BF = torch.bfloat16
SENT = -768.0                     # exact in bf16; an output is a convex combination of v, |v| < 6 * 8 in every regime: never the sentinel
REGIMES = ac.REGIMES
LK_EDGES = (1, 2, 15, 16, 17, 31, 32, 33, 95, 96, 97, 128, 257, 287, 288)
LQ_EDGES = (1, 15, 16, 17, 31, 32, 33, 77, 129, 257)
BH = ((1, 1), (3, 2), (2, 8))
MUTATIONS = ("pad", "droplast", "q_offset_lk", "kv_ld_inner", "v_at_k", "no_scale", "unnormalised", "drop_last_q_tile")
WIDE = 6                          # the wide K / V buffer holds 6 inner columns; K at 2 inner, V at 3 inner
Q_EXTRA, O_EXTRA = 24, 8          # q_ld = inner + 24, o_ld = inner + 8


def pairs():
    """(Lq, Lk) pairwise, not the full cross: every Lk with Lq in {1, 17}, every Lq with Lk in {33, 257}"""
    out = []
    for lk in LK_EDGES:
        out += [(1, lk), (17, lk)]
    for lq in LQ_EDGES:
        for lk in (33, 257):
            if (lq, lk) not in out:
                out.append((lq, lk))
    return out


def key_tiles(Lk):
    """16-key tiles cross_attn_seq_kernel holds (cross_seq_plan.h): the keys up to 16 * key_tiles exist as zero rows in LDS"""
    return 2 if Lk <= 32 else 6 if Lk <= 96 else 18


def inputs(B, Lq, Lk, H, regime, seed):
    """Q [B Lq, d], K, V [B Lk, d] bf16"""
    d = DH * H
    Q = ac.make_qkv(B, Lq, H, regime, BF, seed)[:, :d].contiguous()
    kv = ac.make_qkv(B, Lk, H, regime, BF, seed + 1000)
    return Q, kv[:, d:2 * d].contiguous(), kv[:, 2 * d:].contiguous()


def _heads(x, B, L, H, ft):
    return x.to(ft).reshape(B, L, H, DH).transpose(1, 2)                   # [B, H, L, 64]


def reference(Q, K, V, B, Lq, Lk, H):
    """-> (o, A, vmax) float64 [B Lq, d]"""
    q, k, v = _heads(Q, B, Lq, H, torch.float64), _heads(K, B, Lk, H, torch.float64), _heads(V, B, Lk, H, torch.float64)
    p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1)
    merge = lambda t: t.transpose(1, 2).reshape(B * Lq, H * DH)           # noqa: E731
    vmax = v.abs().amax(dim=(2, 3), keepdim=True).expand(B, H, Lq, DH)
    return merge(p @ v), merge(p @ v.abs()), merge(vmax)


def bound(R):
    o, A, vmax = R
    return 1.05 * ac.UNIT[BF] * (A + o.abs()) + 2.0 ** -20 * vmax


def failures(got, R, B, Lq, H, what=""):
    """got [B Lq, d] -> ([messages], worst ratio); a non-finite or sentinel output counts as infinite"""
    ratio = (got.double() - R[0]).abs() / bound(R)
    bad_val = ~torch.isfinite(got.double()) | (got.double() == SENT)
    ratio = torch.where(torch.isfinite(ratio) & ~bad_val, ratio, torch.full_like(ratio, float("inf")))
    per = ratio.reshape(B, Lq, H, DH).amax(-1)                              # [B, Lq, H]
    worst = float(per.max())
    bad = (per > 1.0).nonzero().tolist()
    if not bad:
        return [], worst
    head = f"{what}: {len(bad)} (sample, row, head) beyond the bound (worst ratio {worst:.3g}): "
    return [head + ", ".join(f"(b{b} row{i} h{h}: {float(per[b, i, h]):.3g})" for b, i, h in bad[:12])], worst


class Layout:
    """The four buffers of one launch as flat-indexable CPU tensors (see the module docstring)"""

    def __init__(self, Q, K, V, B, Lq, Lk, H):
        inner = DH * H
        self.B, self.Lq, self.Lk, self.H, self.inner = B, Lq, Lk, H, inner
        self.q_ld, self.kv_ld, self.o_ld = inner + Q_EXTRA, WIDE * inner, inner + O_EXTRA
        self.ko, self.vo = 2 * inner, 3 * inner
        self.qbuf = torch.full((B * Lq, self.q_ld), float("nan"), dtype=BF)
        self.qbuf[:, :inner] = Q
        self.kvbuf = torch.full((B * Lk, self.kv_ld), float("nan"), dtype=BF)
        self.kvbuf[:, self.ko:self.ko + inner] = K
        self.kvbuf[:, self.vo:self.vo + inner] = V

    def out_window(self, obuf):
        """the B Lq x inner window of an out buffer [B Lq, o_ld]"""
        return obuf[:, :self.inner]


def applicable(mutation, B, Lq, Lk):
    """Is the mutation a defect at all for this case?"""
    if mutation == "pad":
        return Lk != 16 * key_tiles(Lk)
    if mutation in ("droplast", "no_scale", "unnormalised"):
        return Lk >= 2
    if mutation == "q_offset_lk":
        return B >= 2 and Lq != Lk
    if mutation == "kv_ld_inner":
        return B * Lk >= 2
    return True


def model(lay, mutation=None):
    """cross_attn_seq_kernel in float32 on the kernel's own indexing of the buffers of `lay` -> out buffer [B Lq, o_ld] bf16 (sentinel
    where nothing is stored).  fp32 scores (products of bf16 operands are exact), p = exp2((s - m) / 8 log2 e) in fp32, the row sum over
    the UNROUNDED p, p rounded to bf16 for the second product (fp32 accumulate), the quotient rounded to bf16.
    Mutations: pad (the zero pad keys up to the tile count are not masked), droplast (the last key is not seen), q_offset_lk (a
    sample's query rows are taken to start at b Lk), kv_ld_inner (the K / V row stride is taken as 64 heads), v_at_k (V read at K's
    column), no_scale (no 1 / 8), unnormalised (no division by the row sum), drop_last_q_tile (the last 16-query tile is not stored)."""
    B, Lq, Lk, H, inner = lay.B, lay.Lq, lay.Lk, lay.H, lay.inner
    nan = torch.full((1,), float("nan"))
    qflat, kvflat = torch.cat([lay.qbuf.float().reshape(-1), nan]), torch.cat([lay.kvbuf.float().reshape(-1), nan])
    qn, kvn = qflat.numel() - 1, kvflat.numel() - 1
    b = torch.arange(B).view(B, 1, 1, 1)
    h = torch.arange(H).view(1, H, 1, 1)
    col = torch.arange(DH).view(1, 1, 1, DH)
    i = torch.arange(Lq).view(1, 1, Lq, 1)
    nk = Lk - 1 if mutation == "droplast" else Lk
    j = torch.arange(nk).view(1, 1, nk, 1)
    q_row0 = b * (Lk if mutation == "q_offset_lk" else Lq)
    stride = inner if mutation == "kv_ld_inner" else lay.kv_ld
    vo = lay.ko if mutation == "v_at_k" else lay.vo
    # (a mutated index may leave the buffer: it reads NaN there, as the NaN rows around the operands of the GPU test would give)
    q = qflat[((q_row0 + i) * lay.q_ld + h * DH + col).clamp_max(qn)]                        # [B, H, Lq, 64]
    k = kvflat[((b * Lk + j) * stride + lay.ko + h * DH + col).clamp_max(kvn)]               # [B, H, nk, 64]
    v = kvflat[((b * Lk + j) * stride + vo + h * DH + col).clamp_max(kvn)]
    if mutation == "pad":
        z = torch.zeros(B, H, 16 * key_tiles(Lk) - nk, DH)
        k, v = torch.cat([k, z], 2), torch.cat([v, z], 2)
    s = q @ k.transpose(-1, -2)
    sl2 = 1.4426950408889634 if mutation == "no_scale" else ac.SL2
    m = s.amax(-1, keepdim=True)
    p = torch.exp2(s * sl2 - m * sl2)
    o = (p.to(BF).double() @ v.double()).float()
    if mutation != "unnormalised":
        o = o * (1.0 / p.sum(-1, keepdim=True))
    o = o.to(BF).transpose(1, 2).reshape(B * Lq, inner)
    obuf = torch.full((B * Lq, lay.o_ld), SENT, dtype=BF)
    obuf[:, :inner] = o
    if mutation == "drop_last_q_tile":
        t0 = (Lq - 1) // 16 * 16
        for bb in range(B):
            obuf[bb * Lq + t0:(bb + 1) * Lq, :inner] = SENT
    return obuf


# ---- the plan (cross_seq_plan.h) as a Python model: tests/test_host_cross_seq_plan.py holds the library against it ----------------
FORM_TILE = _lib.CROSS_SEQ_FORM_TILE
ONE_WG_MAX, CHUNK = 288, 256


def lds_bytes(nkt):
    keys = 16 * nkt
    return keys * DH * 2 + DH * (keys * 2 + 16)


def plan(B, Lq, Lk, heads):
    """info[8] of keds_cross_seq_plan_query"""
    nkt = key_tiles(Lk)
    one = Lq <= ONE_WG_MAX
    chunks = 1 if one else (Lq + CHUNK - 1) // CHUNK
    return [FORM_TILE, nkt, 16 if Lk >= 256 else 0, Lq if one else CHUNK, B * heads * chunks, 256, lds_bytes(nkt), chunks]
