"""The training step as DATA: the ordered chain of public calls one KnowledgeTrainer.loss_and_grads (keds_amd/train.py) has to make, written
from the model's arithmetic (oracle.keds_oracle.training_loss: IM2TEXT in training mode, two CrossFormers, the frozen text tower with the
evaluation splice, the symmetric contrastive loss) and the documented contracts of the entry points (include/keds_hip.h sections 1 and 9)
-- and a float64 executor of such a chain that models the BUFFERS as state.  The shape of tests/tower_check.py, for the step.

plan(geom, dropout, masks_given, remote, adamw) -> Plan: links (dicts) + the named buffers (valid rows, cols, type).  A link names its op,
its inputs and outputs as (buffer, rows) with rows a `range` (first row, count, step) or, behind a row map, a list; the outputs it ADDS
into (`adds`: the BIAS_RESID_F32 epilogue, ln_bwd into dx) -- every other output is overwritten; the public epilogue id; head counts, K,
the causal flag; the dropout scale and seed.  Views are explicit: the key / value gradients of `fuse` and `cond` are the rows [B, B + BK)
and [B + BK, R) of `dmap`, the gradient of the IM2TEXT output; the three token gradients are the rows 3 b + slot of `dtok`.

run64(plan, params, inputs) executes the links in float64 with no rounding.  Every buffer starts as NaN, pad rows (up to the next
multiple of 128) included; adding links add; a transpose zeroes its own pad columns; `zero` links are the only other source of zeros.  A
chain that relies on memory nobody wrote, or on zeroed pad rows, therefore comes out NaN.  It also names the buffers whose pad rows were
written (`dirty`).

walk(plan) checks the dataflow: every row a link reads was written before, no link touches a pad row, no adding link meets rows nobody
initialised, and no store lands on rows that were written and not read since.

MUTATIONS / mutate(plan, name): wiring defects of a step, as edits of the plan.  tests/test_host_step_check.py holds run64 to a float64
autograd model of the step and shows that every mutation is visible; tests/test_gpu_train_step_chain.py runs the same links one public
call at a time beside the trainer and compares by bits."""
import copy

import torch

from tests import train_check as tk

F64 = torch.float64
LN_EPS = 1e-5
QA = 1.702
EPI_BIAS_BF16, EPI_BIAS_RESID_F32, EPI_BIAS_F32 = 0, 3, 4          # the public ids of include/keds_hip.h
BLOCK_W = (("qkv", "attn.in_proj_weight", "attn.in_proj_bias"), ("out", "attn.out_proj.weight", "attn.out_proj.bias"),
           ("fc", "mlp.c_fc.weight", "mlp.c_fc.bias"), ("proj", "mlp.c_proj.weight", "mlp.c_proj.bias"))
MUTATIONS = ("bias_grad_pad_rows", "dw_rows_B_for_BK", "cond_dkv_row_minus1", "dq0_overwrites", "slots_swapped", "drop_scale_missing_bwd",
             "ln_stats_swapped", "token_rows_plus1", "readout_eot_plus1", "wT_next_layer", "dx_bf_stale", "local_rows_all_N", "adamw_wd_on_bias")


def pad(n):
    return (n + 127) // 128 * 128


class Geom:
    """B samples, K neighbours; D the feature width (IM2TEXT in, text embedding), d the token width (IM2TEXT out, text tower), middle the
    IM2TEXT hidden width, xheads CrossFormer heads of 64, theads text heads of 64; eot [B]: the EOT column of every prompt row; ins: the
    column of the `*`; n_remote: rows of remote negatives behind the local ones"""

    def __init__(self, B, K, eot, ins=4, D=128, d=256, middle=384, xheads=8, Lc=77, tlayers=2, xlayers=3, ilayers=2, n_remote=0):
        self.__dict__.update(B=B, K=K, eot=list(eot), ins=ins, D=D, d=d, middle=middle, xheads=xheads, inner=64 * xheads, Lc=Lc,
                             theads=d // 64, tlayers=tlayers, xlayers=xlayers, ilayers=ilayers, n_remote=n_remote)
        self.BK, self.R, self.M, self.N = B * K, B * (1 + 2 * K), B * Lc, B + n_remote
        assert len(self.eot) == B and max(self.eot) + 2 < Lc


def trainable(g):
    """name -> (N, K) of every trainable Linear, in the trainer's naming"""
    out = {}
    k = g.D
    for i in range(g.ilayers):
        out[f"i2t.layers.{i}.0"] = (g.middle, k)
        k = g.middle
    out["i2t.fc_out"] = (g.d, g.middle)
    for tag in ("fuse", "cond"):
        for l in range(g.xlayers):
            for nm in ("to_q", "to_k", "to_v"):
                out[f"{tag}.cross_layers.{l}.{nm}"] = (g.inner, g.d)
            out[f"{tag}.cross_layers.{l}.to_out.0"] = (g.d, g.inner)
    return out


class Plan:
    def __init__(self, geom, **kw):
        self.g = geom
        self.__dict__.update(kw)
        self.links, self.buffers, self.given = [], {}, set()

    def buf(self, name, rows, cols, t="fp32", given=False):
        assert name not in self.buffers, name
        self.buffers[name] = (rows, cols, t)
        if given:
            self.given.add(name)
        return name

    def add(self, op, ins, outs, adds=(), **kw):
        link = dict(op=op, ins=dict(ins), outs=dict(outs), adds=tuple(adds), **kw)
        self.links.append(link)
        return link

    def clone(self):
        p = copy.copy(self)
        p.links, p.buffers, p.given = copy.deepcopy(self.links), dict(self.buffers), set(self.given)
        return p

    def find(self, **match):
        return [s for s in self.links if all(s.get(k) == v for k, v in match.items())]

    def grads(self):
        return sorted(n for n in self.buffers if n.startswith("g:"))


def R_(buf, n, r0=0, step=1):
    return (buf, range(r0, r0 + n * step, step))


def plan(geom, dropout=0.1, masks_given=True, remote=False, adamw=False, seed=0, steps=0, hp=None):
    g = geom
    assert remote == (g.n_remote > 0)
    p = Plan(g, dropout=dropout, masks_given=masks_given, remote=remote, seed=seed, steps=steps)
    B, K, BK, R, M, N, D, d, mid, inner, Lc = g.B, g.K, g.BK, g.R, g.M, g.N, g.D, g.d, g.middle, g.inner, g.Lc
    lin = trainable(g)

    def gemm(a, w, bias, epi, out, M_, what, add=False):
        """out[M_, N] (+)= a[M_, K] . w[N, K]^T + bias: every row of the weight buffer, every column of both operands"""
        Nw = p.buffers[w][0]
        ins = {"a": (a[0], range(a[1], a[1] + M_)), "w": R_(w, Nw)}
        if bias is not None:
            ins["bias"] = R_(bias, 1)
        assert add == (epi == EPI_BIAS_RESID_F32)
        return p.add("gemm", ins, {"out": (out[0], range(out[1], out[1] + M_))}, adds=("out",) if add else (), epi=epi, M=M_, N=Nw,
                     K=p.buffers[w][1], what=what)

    # ---- operands of this step: bf16 copies of the fp32 masters, and their transposes for dX
    for nm, (n_, k_) in lin.items():
        p.buf(f"p:{nm}.weight", n_, k_, given=True)
        p.buf(f"p:{nm}.bias", 1, n_, given=True)
        p.buf(f"w:{nm}", n_, k_, "bf16")
        p.buf(f"wT:{nm}", k_, n_, "bf16")
        p.add("cast", {"x": R_(f"p:{nm}.weight", n_)}, {"y": R_(f"w:{nm}", n_)})
        p.add("transpose", {"x": R_(f"p:{nm}.weight", n_)}, {"y": R_(f"wT:{nm}", k_)}, rows=n_, cols=k_, ld_out=n_)
    for t in range(g.tlayers):
        for nm, n_, k_ in (("qkv", 3 * d, d), ("out", d, d), ("fc", 4 * d, d), ("proj", d, 4 * d)):
            p.buf(f"f:{t}.{nm}_w", n_, k_, given=True)
            p.buf(f"f:{t}.{nm}_b", 1, n_, given=True)
            p.buf(f"w:{t}.{nm}", n_, k_, "bf16")
            p.buf(f"wT:{t}.{nm}", k_, n_, "bf16")
            p.add("cast", {"x": R_(f"f:{t}.{nm}_w", n_)}, {"y": R_(f"w:{t}.{nm}", n_)}, frozen=True)
            p.add("transpose", {"x": R_(f"f:{t}.{nm}_w", n_)}, {"y": R_(f"wT:{t}.{nm}", k_)}, rows=n_, cols=k_, ld_out=n_, frozen=True)
        for nm in ("ln1", "ln2"):
            p.buf(f"f:{t}.{nm}_g", 1, d, given=True)
            p.buf(f"f:{t}.{nm}_b", 1, d, given=True)
    for nm, r_, c_ in (("lnf_g", 1, d), ("lnf_b", 1, d), ("P", d, D), ("pos", Lc, d)):
        p.buf("f:" + nm, r_, c_, given=True)
    p.buf("f:tok", geom_vocab(g), d, given=True)
    p.buf("w:P", d, D, "bf16")                       # [d, D]: the dX operand of the read-out projection
    p.buf("wT:P", D, d, "bf16")                      # [D, d]: its forward operand
    p.add("cast", {"x": R_("f:P", d)}, {"y": R_("w:P", d)}, frozen=True)
    p.add("transpose", {"x": R_("f:P", d)}, {"y": R_("wT:P", D)}, rows=d, cols=D, ld_out=d, frozen=True)

    # ---- the rows [q; I; T] through IM2TEXT in training mode
    for nm, r_ in (("feats", B), ("nbr_img", BK), ("nbr_txt", BK)):
        p.buf(nm, r_, D, given=True)
    p.buf("text", B, Lc, "i32", given=True)
    p.buf("rows", R, D)
    p.add("copy", {"x": R_("feats", B)}, {"y": R_("rows", B)})
    p.add("copy", {"x": R_("nbr_img", BK)}, {"y": R_("rows", BK, B)})
    p.add("copy", {"x": R_("nbr_txt", BK)}, {"y": R_("rows", BK, B + BK)})
    p.buf("rows_bf", R, D, "bf16")
    p.add("cast", {"x": R_("rows", R)}, {"y": R_("rows_bf", R)})
    scale = 1.0 / (1.0 - dropout) if dropout > 0 else 1.0
    cur = "rows_bf"
    for i in range(g.ilayers):
        nm = f"i2t.layers.{i}.0"
        p.buf(f"z{i}", R, mid, "bf16")
        p.buf(f"y{i}", R, mid, "bf16")
        gemm((cur, 0), "w:" + nm, f"p:{nm}.bias", EPI_BIAS_BF16, (f"z{i}", 0), R, nm)
        ins = {"z": R_(f"z{i}", R)}
        if dropout > 0:
            if masks_given:
                p.buf(f"mask{i}", R, mid, "u8", given=True)
            else:
                p.buf(f"mask{i}", R, mid, "u8")
                p.add("mask", {}, {"mask": R_(f"mask{i}", R)}, seed=(seed << 32) + steps * 16 + i, p=dropout)
            ins["mask"] = R_(f"mask{i}", R)
        p.add("drelu_fwd", ins, {"y": R_(f"y{i}", R)}, scale=scale)
        cur = f"y{i}"
    y_last = cur
    p.buf("mapped", R, d)
    gemm((y_last, 0), "w:i2t.fc_out", "p:i2t.fc_out.bias", EPI_BIAS_F32, ("mapped", 0), R, "i2t.fc_out")
    p.buf("q_bf", B, d, "bf16")
    p.add("cast", {"x": R_("mapped", B)}, {"y": R_("q_bf", B)})
    kv = {}
    for s, tag in enumerate(("fuse", "cond")):
        kv[tag] = p.buf(f"kv_{tag}", BK, d, "bf16")
        p.add("cast", {"x": R_("mapped", BK, B + s * BK)}, {"y": R_(kv[tag], BK)})

    # ---- two CrossFormers: the query chained through the layers, keys and values fixed
    p.buf("tokens", 3 * B, d)
    for s, tag in enumerate(("fuse", "cond")):
        q_in = "q_bf"
        for l in range(g.xlayers):
            L = f"{tag}.cross_layers.{l}."
            X = f"{tag}{l}."
            p.buf(X + "Q", B, inner, "bf16"), p.buf(X + "K", BK, inner, "bf16"), p.buf(X + "V", BK, inner, "bf16")
            p.buf(X + "att", B, inner, "bf16"), p.buf(X + "qn", B, d)
            gemm((q_in, 0), "w:" + L + "to_q", "p:" + L + "to_q.bias", EPI_BIAS_BF16, (X + "Q", 0), B, L + "to_q")
            gemm((kv[tag], 0), "w:" + L + "to_k", "p:" + L + "to_k.bias", EPI_BIAS_BF16, (X + "K", 0), BK, L + "to_k")
            gemm((kv[tag], 0), "w:" + L + "to_v", "p:" + L + "to_v.bias", EPI_BIAS_BF16, (X + "V", 0), BK, L + "to_v")
            p.add("cross_fwd", {"Q": R_(X + "Q", B), "K": R_(X + "K", BK), "V": R_(X + "V", BK)}, {"out": R_(X + "att", B)}, B=B, Kn=K, heads=g.xheads)
            gemm((X + "att", 0), "w:" + L + "to_out.0", "p:" + L + "to_out.0.bias", EPI_BIAS_F32, (X + "qn", 0), B, L + "to_out.0")
            if l + 1 < g.xlayers:
                p.buf(X + "qn_bf", B, d, "bf16")
                p.add("cast", {"x": R_(X + "qn", B)}, {"y": R_(X + "qn_bf", B)})
            q_in = X + "qn_bf"
        p.add("copy", {"x": R_(f"{tag}{g.xlayers - 1}.qn", B)}, {"y": R_("tokens", B, s, 3)})
    p.add("copy", {"x": R_("mapped", B)}, {"y": R_("tokens", B, 2, 3)})

    # ---- the frozen text tower on the prompt with the three tokens at the *, saved activations
    readout = [b * Lc + g.eot[b] + 2 for b in range(B)]
    token_rows = [b * Lc + g.ins + j for b in range(B) for j in range(3)]
    p.buf("x0", M, d)
    p.add("embed", {"text": R_("text", B), "table": R_("f:tok", geom_vocab(g)), "pos": R_("f:pos", Lc), "tokens": R_("tokens", 3 * B)},
          {"x": R_("x0", M)}, B=B, Lc=Lc, n_tok=3, col=g.ins)
    for t in range(g.tlayers):
        T = f"t{t}."
        for nm, c_, ty in (("ln1", d, "bf16"), ("st1", 2, "fp32"), ("qkv", 3 * d, "bf16"), ("att", d, "bf16"), ("xm", d, "fp32"), ("ln2", d, "bf16"),
                           ("st2", 2, "fp32"), ("u", 4 * d, "bf16"), ("hid", 4 * d, "bf16")):
            p.buf(T + nm, M, c_, ty)
        p.buf(f"x{t + 1}", M, d)
        x = f"x{t}"
        p.add("ln_fwd", {"x": R_(x, M), "gamma": R_(f"f:{t}.ln1_g", 1), "beta": R_(f"f:{t}.ln1_b", 1)}, {"y": R_(T + "ln1", M), "stats": R_(T + "st1", M)})
        gemm((T + "ln1", 0), f"w:{t}.qkv", f"f:{t}.qkv_b", EPI_BIAS_BF16, (T + "qkv", 0), M, f"{t}.qkv")
        p.add("attn", {"qkv": R_(T + "qkv", M)}, {"out": R_(T + "att", M)}, B=B, S=Lc, heads=g.theads, causal=1)
        p.add("copy", {"x": R_(x, M)}, {"y": R_(T + "xm", M)})
        gemm((T + "att", 0), f"w:{t}.out", f"f:{t}.out_b", EPI_BIAS_RESID_F32, (T + "xm", 0), M, f"{t}.out", add=True)
        p.add("ln_fwd", {"x": R_(T + "xm", M), "gamma": R_(f"f:{t}.ln2_g", 1), "beta": R_(f"f:{t}.ln2_b", 1)}, {"y": R_(T + "ln2", M), "stats": R_(T + "st2", M)})
        gemm((T + "ln2", 0), f"w:{t}.fc", f"f:{t}.fc_b", EPI_BIAS_BF16, (T + "u", 0), M, f"{t}.fc")
        p.add("qgelu_fwd", {"u": R_(T + "u", M)}, {"y": R_(T + "hid", M)})
        p.add("copy", {"x": R_(T + "xm", M)}, {"y": R_(f"x{t + 1}", M)})
        gemm((T + "hid", 0), f"w:{t}.proj", f"f:{t}.proj_b", EPI_BIAS_RESID_F32, (f"x{t + 1}", 0), M, f"{t}.proj", add=True)
    xl = f"x{g.tlayers}"
    p.buf("lnf", B, d, "bf16"), p.buf("stf", B, 2), p.buf("feat", B, D)
    p.add("ln_fwd", {"x": (xl, list(readout)), "gamma": R_("f:lnf_g", 1), "beta": R_("f:lnf_b", 1)}, {"y": R_("lnf", B), "stats": R_("stf", B)}, mapped=True,
          what="readout")
    gemm(("lnf", 0), "wT:P", None, EPI_BIAS_F32, ("feat", 0), B, "text_projection")

    # ---- the loss over N rows, this rank's B first, and its gradient on the local text rows
    for nm in ("txt_n", "img_n"):
        p.buf(nm, B, D)
    p.add("l2n", {"x": R_("feat", B)}, {"y": R_("txt_n", B)})
    p.add("l2n", {"x": R_("feats", B)}, {"y": R_("img_n", B)})
    p.buf("all_img", N, D), p.buf("all_txt", N, D)
    p.add("copy", {"x": R_("img_n", B)}, {"y": R_("all_img", B)})
    p.add("copy", {"x": R_("txt_n", B)}, {"y": R_("all_txt", B)})
    if remote:
        p.buf("other_img_n", g.n_remote, D, given=True), p.buf("other_txt_n", g.n_remote, D, given=True)
        p.add("copy", {"x": R_("other_img_n", g.n_remote)}, {"y": R_("all_img", g.n_remote, B)})
        p.add("copy", {"x": R_("other_txt_n", g.n_remote)}, {"y": R_("all_txt", g.n_remote, B)})
    p.buf("loss", 1, 1), p.buf("dtxt_n", B, D), p.buf("dfeat", B, D), p.buf("dfeat_bf", B, D, "bf16"), p.buf("dlnf", B, d)
    p.add("loss", {"img": R_("all_img", N), "txt": R_("all_txt", N)}, {"loss": R_("loss", 1), "dtxt": R_("dtxt_n", B)}, N=N, B_local=B)
    p.add("l2n_bwd", {"x": R_("feat", B), "dy": R_("dtxt_n", B)}, {"dx": R_("dfeat", B)})

    # ---- backward through the frozen tower to the three token rows
    p.add("cast", {"x": R_("dfeat", B)}, {"y": R_("dfeat_bf", B)})
    gemm(("dfeat_bf", 0), "w:P", None, EPI_BIAS_F32, ("dlnf", 0), B, "text_projection^T")
    p.buf("dx", M, d), p.buf("dx_bf", M, d, "bf16")
    p.add("zero", {}, {"y": R_("dx", M)})
    p.add("ln_bwd", {"dy": R_("dlnf", B), "x": (xl, list(readout)), "stats": R_("stf", B), "gamma": R_("f:lnf_g", 1)}, {"dx": ("dx", list(readout))},
          adds=("dx",), mapped=True, what="readout")
    p.add("cast", {"x": R_("dx", M)}, {"y": R_("dx_bf", M)})
    for t in reversed(range(g.tlayers)):
        T = f"t{t}."
        for nm, c_, ty in (("dhid", 4 * d, "bf16"), ("du", 4 * d, "bf16"), ("dln2", d, "fp32"), ("datt", d, "bf16"), ("dqkv", 3 * d, "bf16"), ("dln1", d, "fp32")):
            p.buf(T + nm, M, c_, ty)
        gemm(("dx_bf", 0), f"wT:{t}.proj", None, EPI_BIAS_BF16, (T + "dhid", 0), M, f"{t}.proj^T")
        p.add("qgelu_bwd", {"dy": R_(T + "dhid", M), "u": R_(T + "u", M)}, {"du": R_(T + "du", M)})
        gemm((T + "du", 0), f"wT:{t}.fc", None, EPI_BIAS_F32, (T + "dln2", 0), M, f"{t}.fc^T")
        p.add("ln_bwd", {"dy": R_(T + "dln2", M), "x": R_(T + "xm", M), "stats": R_(T + "st2", M), "gamma": R_(f"f:{t}.ln2_g", 1)},
              {"dx": R_("dx", M), "dx_bf": R_("dx_bf", M)}, adds=("dx",), what=f"{t}.ln2", layer=t)
        gemm(("dx_bf", 0), f"wT:{t}.out", None, EPI_BIAS_BF16, (T + "datt", 0), M, f"{t}.out^T")
        p.add("attn_bwd", {"qkv": R_(T + "qkv", M), "dout": R_(T + "datt", M)}, {"dqkv": R_(T + "dqkv", M)}, B=B, S=Lc, heads=g.theads, causal=1)
        gemm((T + "dqkv", 0), f"wT:{t}.qkv", None, EPI_BIAS_F32, (T + "dln1", 0), M, f"{t}.qkv^T")
        p.add("ln_bwd", {"dy": R_(T + "dln1", M), "x": R_(f"x{t}", M), "stats": R_(T + "st1", M), "gamma": R_(f"f:{t}.ln1_g", 1)},
              {"dx": R_("dx", M), "dx_bf": R_("dx_bf", M)}, adds=("dx",), what=f"{t}.ln1", layer=t)
    p.buf("dtok", 3 * B, d)
    p.add("gather", {"x": ("dx", list(token_rows))}, {"y": R_("dtok", 3 * B)})

    # ---- backward of the three modules
    def grad_w(nm, dy, x, rows, n_, k_):
        """g:nm.weight [n_, k_] = dy[:rows]^T . x[:rows]: both operands transposed with `rows` padded to 128 by zeros"""
        a, b = p.buf(f"T:{nm}.dy", n_, pad(rows), "bf16"), p.buf(f"T:{nm}.x", k_, pad(rows), "bf16")
        p.add("transpose", {"x": (dy[0], range(dy[1], dy[1] + rows))}, {"y": R_(a, n_)}, rows=rows, cols=n_, ld_out=pad(rows), grad=nm)
        p.add("transpose", {"x": (x[0], range(x[1], x[1] + rows))}, {"y": R_(b, k_)}, rows=rows, cols=k_, ld_out=pad(rows), grad=nm)
        p.buf(f"g:{nm}.weight", n_, k_)
        gemm((a, 0), b, None, EPI_BIAS_F32, (f"g:{nm}.weight", 0), n_, f"dW {nm}")

    def grad_b(nm, x, rows, n_):
        p.buf(f"g:{nm}.bias", 1, n_)
        p.add("colsum", {"x": (x[0], range(x[1], x[1] + rows))}, {"y": R_(f"g:{nm}.bias", 1)}, grad=nm)

    p.buf("dmap", R, d)
    p.add("zero", {}, {"y": R_("dmap", R - B, B)})
    p.add("copy", {"x": R_("dtok", B, 2, 3)}, {"y": R_("dmap", B)}, slot=2)
    for s, tag in enumerate(("fuse", "cond")):
        dq = p.buf(f"{tag}.dq{g.xlayers - 1}", B, d)
        p.add("copy", {"x": R_("dtok", B, s, 3)}, {"y": R_(dq, B)}, slot=s, tag=tag)
        lo = B + s * BK
        for l in reversed(range(g.xlayers)):
            L = f"{tag}.cross_layers.{l}."
            X = f"{tag}{l}."
            q_in = "q_bf" if l == 0 else f"{tag}{l - 1}.qn_bf"
            p.buf(X + "dy", B, d, "bf16")
            p.buf(X + "datt", B, inner, "bf16"), p.buf(X + "dQ", B, inner, "bf16"), p.buf(X + "dK", BK, inner, "bf16"), p.buf(X + "dV", BK, inner, "bf16")
            p.add("cast", {"x": R_(dq, B)}, {"y": R_(X + "dy", B)})
            grad_w(L + "to_out.0", (X + "dy", 0), (X + "att", 0), B, d, inner)
            grad_b(L + "to_out.0", (dq, 0), B, d)
            gemm((X + "dy", 0), "wT:" + L + "to_out.0", None, EPI_BIAS_BF16, (X + "datt", 0), B, L + "to_out.0^T")
            p.add("cross_bwd", {"Q": R_(X + "Q", B), "K": R_(X + "K", BK), "V": R_(X + "V", BK), "dout": R_(X + "datt", B)},
                  {"dQ": R_(X + "dQ", B), "dK": R_(X + "dK", BK), "dV": R_(X + "dV", BK)}, B=B, Kn=K, heads=g.xheads)
            for nm, gb, xb, rows in (("to_q", X + "dQ", q_in, B), ("to_k", X + "dK", kv[tag], BK), ("to_v", X + "dV", kv[tag], BK)):
                grad_w(L + nm, (gb, 0), (xb, 0), rows, inner, d)
                grad_b(L + nm, (gb, 0), rows, inner)
            gemm((X + "dK", 0), "wT:" + L + "to_k", None, EPI_BIAS_RESID_F32, ("dmap", lo), BK, L + "to_k^T", add=True)
            gemm((X + "dV", 0), "wT:" + L + "to_v", None, EPI_BIAS_RESID_F32, ("dmap", lo), BK, L + "to_v^T", add=True)
            if l > 0:
                dq = p.buf(f"{tag}.dq{l - 1}", B, d)
                gemm((X + "dQ", 0), "wT:" + L + "to_q", None, EPI_BIAS_F32, (dq, 0), B, L + "to_q^T")
            else:
                gemm((X + "dQ", 0), "wT:" + L + "to_q", None, EPI_BIAS_RESID_F32, ("dmap", 0), B, L + "to_q^T", add=True)
    p.buf("dmap_bf", R, d, "bf16")
    p.add("cast", {"x": R_("dmap", R)}, {"y": R_("dmap_bf", R)})
    grad_w("i2t.fc_out", ("dmap_bf", 0), (y_last, 0), R, d, mid)
    grad_b("i2t.fc_out", ("dmap", 0), R, d)
    p.buf(f"dcur{g.ilayers - 1}", R, mid, "bf16")
    gemm(("dmap_bf", 0), "wT:i2t.fc_out", None, EPI_BIAS_BF16, (f"dcur{g.ilayers - 1}", 0), R, "i2t.fc_out^T")
    for i in reversed(range(g.ilayers)):
        nm = f"i2t.layers.{i}.0"
        p.buf(f"dz{i}", R, mid, "bf16")
        ins = {"dy": R_(f"dcur{i}", R), "z": R_(f"z{i}", R)}
        if dropout > 0:
            ins["mask"] = R_(f"mask{i}", R)
        p.add("drelu_bwd", ins, {"dz": R_(f"dz{i}", R)}, scale=scale, layer=i)
        x_in = "rows_bf" if i == 0 else f"y{i - 1}"
        grad_w(nm, (f"dz{i}", 0), (x_in, 0), R, mid, lin[nm][1])
        grad_b(nm, (f"dz{i}", 0), R, mid)
        if i > 0:
            p.buf(f"dcur{i - 1}", R, mid, "bf16")
            gemm((f"dz{i}", 0), "wT:" + nm, None, EPI_BIAS_BF16, (f"dcur{i - 1}", 0), R, nm + "^T")
    if adamw:
        hp = dict(lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, wd=0.1) if hp is None else hp
        p.hp = hp
        for n in p.grads():
            name = n[2:]
            r_, c_, _ = p.buffers[n]
            p.buf("m:" + name, r_, c_, given=True), p.buf("v:" + name, r_, c_, given=True)
            io = {"p": R_("p:" + name, r_), "m": R_("m:" + name, r_), "v": R_("v:" + name, r_)}
            p.add("adamw", dict(io, g=R_(n, r_)), io, wd=0.0 if name.endswith(".bias") else hp["wd"], step=steps + 1, name=name)
    return p


# ---- mutations -------------------------------------------------------------------------------------------------------------------------
def _shift(ref, by):
    buf, rows = ref
    return (buf, range(rows.start + by, rows.stop + by, rows.step)) if isinstance(rows, range) else (buf, [r + by for r in rows])


def mutate(plan_, name):
    """-> the mutated copy, or None where the geometry gives the defect nothing to change"""
    p = plan_.clone()
    g = p.g
    if name == "bias_grad_pad_rows":
        s = [x for x in p.find(op="colsum") if x["grad"] == "i2t.layers.1.0"][0]
        buf, rows = s["ins"]["x"]
        s["ins"]["x"] = (buf, range(0, pad(len(rows))))
        return p if pad(len(rows)) != len(rows) else None
    if name == "dw_rows_B_for_BK":
        if g.B == g.BK:
            return None
        for s in p.find(op="transpose"):
            if s.get("grad", "").endswith(".to_k") or s.get("grad", "").endswith(".to_v"):
                buf, rows = s["ins"]["x"]
                s["ins"]["x"], s["rows"] = (buf, range(0, g.B)), g.B
        return p
    if name == "cond_dkv_row_minus1":
        for s in p.find(op="gemm"):
            if s["what"].startswith("cond.") and s["what"].endswith(("to_k^T", "to_v^T")):
                s["outs"]["out"] = _shift(s["outs"]["out"], -1)
        return p
    if name == "dq0_overwrites":
        s = p.find(op="gemm", what="fuse.cross_layers.0.to_q^T")[0]
        s["adds"], s["epi"] = (), EPI_BIAS_F32
        return p
    if name == "slots_swapped":
        a, b = p.find(op="copy", tag="fuse")[0], p.find(op="copy", tag="cond")[0]
        a["ins"], b["ins"] = b["ins"], a["ins"]
        return p
    if name == "drop_scale_missing_bwd":
        if p.dropout == 0:
            return None
        for s in p.find(op="drelu_bwd"):
            s["scale"] = 1.0
        return p
    if name == "ln_stats_swapped":
        a, b = p.find(op="ln_bwd", what="1.ln2")[0], p.find(op="ln_bwd", what="1.ln1")[0]
        a["ins"]["stats"], b["ins"]["stats"] = b["ins"]["stats"], a["ins"]["stats"]
        return p
    if name == "token_rows_plus1":
        s = p.find(op="gather")[0]
        s["ins"]["x"] = _shift(s["ins"]["x"], 1)
        return p
    if name == "readout_eot_plus1":
        for s in p.find(what="readout"):
            s["ins"]["x"] = _shift(s["ins"]["x"], -1)
            if s["op"] == "ln_bwd":
                s["outs"]["dx"] = _shift(s["outs"]["dx"], -1)
        return p
    if name == "wT_next_layer":
        s = p.find(op="gemm", what="fuse.cross_layers.1.to_k^T")[0]
        s["ins"]["w"] = (s["ins"]["w"][0].replace("layers.1.", "layers.2."), s["ins"]["w"][1])
        return p
    if name == "dx_bf_stale":
        i = p.links.index(p.find(op="ln_bwd", what="1.ln2")[0])
        M = g.M
        p.buf("dx_bf_stale", M, g.d, "bf16")
        p.links.insert(i, dict(op="copy", ins={"x": R_("dx_bf", M)}, outs={"y": R_("dx_bf_stale", M)}, adds=()))
        p.find(op="gemm", what="1.out^T")[0]["ins"]["a"] = R_("dx_bf_stale", M)
        return p
    if name == "local_rows_all_N":
        if g.N == g.B:
            return None
        s = p.find(op="loss")[0]
        s["B_local"] = g.N
        s["outs"]["dtxt"] = R_("dtxt_n", g.N)
        return p
    if name == "adamw_wd_on_bias":
        hit = [s for s in p.find(op="adamw") if s["name"].endswith(".bias")]
        for s in hit:
            s["wd"] = p.hp["wd"]
        return p if hit else None
    raise KeyError(name)


# ---- the float64 executor ----------------------------------------------------------------------------------------------------------
def _ln_stats(x):
    mu = x.mean(1, keepdim=True)
    r = ((x - mu).square().mean(1, keepdim=True) + LN_EPS).rsqrt()
    return mu, r


def _heads(t, B, S, H):
    return t.reshape(B, S, H, 64).transpose(1, 2)


def _unheads(t):
    B, H, S, _ = t.shape
    return t.transpose(1, 2).reshape(B * S, H * 64)


def _core64(q, k, v, go, causal):
    """softmax(q k^T / 8) v and, given go, its backward (docs/kernels.md, training): -> out, dQ, dK, dV"""
    s = q @ k.transpose(-1, -2) / 8
    if causal:
        s = s.masked_fill(torch.ones(s.shape[-2:], dtype=torch.bool).triu(1), float("-inf"))
    P = torch.softmax(s, -1)
    out = P @ v
    if go is None:
        return out, None, None, None
    dP = go @ v.transpose(-1, -2)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True)) / 8
    return out, dS @ k, dS.transpose(-1, -2) @ q, P.transpose(-1, -2) @ go


def run64(p, params, inputs):
    """params: name -> tensor of every `given` buffer starting with p: / f: / m: / v:; inputs: the other given buffers.
    -> dict(loss, grads: name -> [N, K] or [N], state: every buffer with its pad rows, dirty: buffers whose pad rows were written)"""
    st = {}
    for name, (r, c, t) in p.buffers.items():
        st[name] = torch.full((pad(r), c), float("nan"), dtype=F64)
        if name in p.given:
            src = params[name] if name in params else inputs[name]
            st[name][:r] = src.reshape(r, c).double()

    def rd(ref):
        return st[ref[0]][list(ref[1])]

    def wr(link, role, val):
        buf, rows = link["outs"][role]
        rows = list(rows)
        st[buf][rows] = st[buf][rows] + val if role in link["adds"] else val

    for s in p.links:
        op, i = s["op"], s["ins"]
        if op in ("copy", "cast"):
            wr(s, "y", rd(i["x"]))
        elif op == "zero":
            wr(s, "y", 0.0)
        elif op == "transpose":
            x = rd(i["x"])
            out = torch.zeros(s["cols"], s["ld_out"], dtype=F64)
            out[:, :s["rows"]] = x.t()
            wr(s, "y", out)
        elif op == "gemm":
            acc = rd(i["a"]) @ rd(i["w"]).t()
            wr(s, "out", acc + rd(i["bias"]) if "bias" in i else acc)
        elif op == "mask":
            n = len(s["outs"]["mask"][1]) * st[s["outs"]["mask"][0]].shape[1]
            wr(s, "mask", tk.dropout_mask_ref(n, s["seed"], s["p"]).double().reshape(len(s["outs"]["mask"][1]), -1))
        elif op == "drelu_fwd":
            z = rd(i["z"])
            keep = (z > 0) & (rd(i["mask"]) != 0 if "mask" in i else True)
            wr(s, "y", torch.where(keep, z * s["scale"], torch.zeros_like(z)) + 0.0 * z)
        elif op == "drelu_bwd":
            z, dy = rd(i["z"]), rd(i["dy"])
            keep = (z > 0) & (rd(i["mask"]) != 0 if "mask" in i else True)
            wr(s, "dz", torch.where(keep, dy * (s["scale"] if "mask" in i else 1.0), torch.zeros_like(z)) + 0.0 * (z + dy))
        elif op in ("cross_fwd", "cross_bwd"):
            B, K, H = s["B"], s["Kn"], s["heads"]
            go = _heads(rd(i["dout"]), B, 1, H) if op == "cross_bwd" else None
            out, dQ, dK, dV = _core64(_heads(rd(i["Q"]), B, 1, H), _heads(rd(i["K"]), B, K, H), _heads(rd(i["V"]), B, K, H), go, False)
            if go is None:
                wr(s, "out", _unheads(out))
            else:
                wr(s, "dQ", _unheads(dQ)), wr(s, "dK", _unheads(dK)), wr(s, "dV", _unheads(dV))
        elif op in ("attn", "attn_bwd"):
            B, S, H = s["B"], s["S"], s["heads"]
            q, k, v = (_heads(t, B, S, H) for t in rd(i["qkv"]).split(64 * H, dim=1))
            go = _heads(rd(i["dout"]), B, S, H) if op == "attn_bwd" else None
            out, dQ, dK, dV = _core64(q, k, v, go, s["causal"])
            wr(s, "out", _unheads(out)) if go is None else wr(s, "dqkv", torch.cat([_unheads(t) for t in (dQ, dK, dV)], 1))
        elif op == "embed":
            text = rd(i["text"]).long()
            emb = rd(i["table"])[text]                                   # [B, Lc, d]
            tok = rd(i["tokens"]).reshape(s["B"], s["n_tok"], -1)
            c0, n = s["col"], s["n_tok"]
            x = torch.cat([emb[:, :c0], tok, emb[:, c0 + 1:s["Lc"] - (n - 1)]], 1) + rd(i["pos"])
            wr(s, "x", x.reshape(s["B"] * s["Lc"], -1))
        elif op == "ln_fwd":
            x = rd(i["x"])
            mu, r = _ln_stats(x)
            wr(s, "y", (x - mu) * r * rd(i["gamma"]) + rd(i["beta"]))
            wr(s, "stats", torch.cat([mu, r], 1))
        elif op == "ln_bwd":
            x, stats = rd(i["x"]), rd(i["stats"])
            mu, r = stats[:, :1], stats[:, 1:]
            gi = rd(i["dy"]) * rd(i["gamma"])
            xh = (x - mu) * r
            wr(s, "dx", r * (gi - gi.mean(1, keepdim=True) - xh * (gi * xh).mean(1, keepdim=True)))
            if "dx_bf" in s["outs"]:
                wr(s, "dx_bf", rd(s["outs"]["dx"]))
        elif op == "qgelu_fwd":
            u = rd(i["u"])
            wr(s, "y", u * torch.sigmoid(QA * u))
        elif op == "qgelu_bwd":
            u = rd(i["u"])
            sg = torch.sigmoid(QA * u)
            wr(s, "du", rd(i["dy"]) * (sg + QA * u * sg * (1 - sg)))
        elif op == "l2n":
            x = rd(i["x"])
            wr(s, "y", x / x.norm(dim=1, keepdim=True))
        elif op == "l2n_bwd":
            x, dy = rd(i["x"]), rd(i["dy"])
            nrm = x.norm(dim=1, keepdim=True)
            y = x / nrm
            wr(s, "dx", (dy - y * (y * dy).sum(1, keepdim=True)) / nrm)
        elif op == "loss":
            img, txt, N = rd(i["img"]), rd(i["txt"]), s["N"]
            lg = inputs["logit_scale"] * (img @ txt.t())
            lr_, lc_ = torch.logsumexp(lg, 1, keepdim=True), torch.logsumexp(lg, 0, keepdim=True)
            dg = lg.diagonal()
            wr(s, "loss", ((lr_.reshape(-1) - dg) + (lc_.reshape(-1) - dg)).sum().reshape(1, 1) / (2 * N))
            G = (torch.exp(lg - lr_) + torch.exp(lg - lc_) - 2 * torch.eye(N, dtype=F64)) * inputs["logit_scale"] / (2 * N)
            wr(s, "dtxt", (G.t() @ img)[:s["B_local"]])
        elif op == "gather":
            wr(s, "y", rd(i["x"]))
        elif op == "colsum":
            wr(s, "y", rd(i["x"]).sum(0, keepdim=True))
        elif op == "adamw":
            hp, t = p.hp, s["step"]
            pp, gg, m, v = rd(i["p"]), rd(i["g"]), rd(i["m"]), rd(i["v"])
            m1 = hp["b1"] * m + (1 - hp["b1"]) * gg
            v1 = hp["b2"] * v + (1 - hp["b2"]) * gg * gg
            upd = hp["lr"] * (m1 / (1 - hp["b1"] ** t)) / ((v1 / (1 - hp["b2"] ** t)).sqrt() + hp["eps"])
            wr(s, "p", pp - hp["lr"] * s["wd"] * pp - upd), wr(s, "m", m1), wr(s, "v", v1)
        else:
            raise KeyError(op)
    dirty = [n for n, (r, c, t) in p.buffers.items() if not bool(torch.isnan(st[n][r:]).all())]
    grads = {n[2:]: st[n][:p.buffers[n][0]] for n in p.grads()}
    return dict(loss=st["loss"][0, 0], grads=grads, state=st, dirty=dirty)


# ---- the dataflow of a plan ----------------------------------------------------------------------------------------------------------
def walk(p):
    """-> list of findings (empty: clean).  Every row a link reads was written before (or given); no link touches a buffer's pad rows;
    an adding output meets rows that were initialised; an overwriting output never lands on rows that were written (or added into)
    and not read since: a lost store, or a sum mistaken for a first write."""
    written = {n: set(range(r)) if n in p.given else set() for n, (r, c, t) in p.buffers.items()}
    unread = {n: set() for n in p.buffers}            # rows written and not read since
    bad = []
    for k, s in enumerate(p.links):
        tag = f"link {k} {s['op']} {s.get('what', '')}"
        for role, (buf, rows) in s["ins"].items():
            rows = set(rows)
            if max(rows) >= p.buffers[buf][0] or min(rows) < 0:
                bad.append(f"{tag}: reads rows of {buf} outside its {p.buffers[buf][0]} valid rows ({role})")
            if not rows <= written[buf]:
                bad.append(f"{tag}: reads {len(rows - written[buf])} rows of {buf} nobody wrote ({role})")
            unread[buf] -= rows
        for role, (buf, rows) in s["outs"].items():
            rl = list(rows)
            rows = set(rl)
            if len(rl) != len(rows):
                bad.append(f"{tag}: writes a row of {buf} twice ({role})")
            if max(rows) >= p.buffers[buf][0] or min(rows) < 0:
                bad.append(f"{tag}: writes rows of {buf} outside its {p.buffers[buf][0]} valid rows ({role})")
            if role in s["adds"]:
                if not rows <= written[buf]:
                    bad.append(f"{tag}: adds into {len(rows - written[buf])} rows of {buf} nobody initialised ({role})")
            elif rows & unread[buf]:
                bad.append(f"{tag}: overwrites {len(rows & unread[buf])} rows of {buf} that nobody read since they were written ({role})")
            unread[buf] |= rows
            written[buf] |= rows
    return bad


# ---- today's whole-tensor limits (tests/test_gpu_train.py), for the report column ------------------------------------------------------
def passes_todays_limits(loss, grads, ref_loss, ref_grads):
    """would these gradients pass cosine 0.999 / rel-L2 3e-2 (IM2TEXT hidden layers 0.998 / 6e-2) and the loss 2e-3 against the reference?
    -> (bool, worst cosine, worst rel-L2)"""
    ok = bool(torch.isfinite(loss)) and abs(float(loss) - float(ref_loss)) <= 2e-3 * max(1.0, abs(float(ref_loss)))
    wc, wr = 1.0, 0.0
    for n, w in ref_grads.items():
        gq = grads[n].reshape(-1)
        w = w.reshape(-1)
        if n.endswith("to_k.bias"):
            scale = float(ref_grads[n.replace(".bias", ".weight")].norm())
            ok = ok and bool(torch.isfinite(gq).all()) and float(gq.norm()) <= 2e-2 * scale
            continue
        if not bool(torch.isfinite(gq).all()):
            return False, float("nan"), float("nan")
        cs = float((gq * w).sum() / (gq.norm() * w.norm() + 1e-300))
        rl = float((gq - w).norm() / max(float(w.norm()), 1e-300))
        c_lim, r_lim = (0.998, 6e-2) if n.startswith("i2t.layers.") else (0.999, 3e-2)
        ok = ok and cs >= c_lim and rl <= r_lim
        wc, wr = min(wc, cs), max(wr, rl)
    return ok, wc, wr



# ---- seeded cases: the state dicts, the batch, the prompt, the masks -------------------------------------------------------------------
VOCAB, STAR = 512, 265
GEOMS = ((1, 1), (3, 5), (8, 16), (5, 32))
HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.1)
# (B, K, prompt form, dropout, masks given, remote rows): every geometry with the shared prompt, with a read-out row of its own per
# sample and with the last row's read-out in the last row of the context; dropout 0.1 with given masks, with device-drawn masks, and 0
CASES = ((1, 1, "shared", 0.1, True, 0), (1, 1, "rows", 0.0, True, 0), (3, 5, "shared", 0.1, True, 0), (3, 5, "rows", 0.1, False, 0),
         (3, 5, "last74", 0.0, True, 0), (3, 5, "rows", 0.1, True, 4), (8, 16, "shared", 0.1, False, 0), (8, 16, "rows", 0.1, True, 0),
         (8, 16, "last74", 0.0, True, 0), (5, 32, "shared", 0.0, True, 0), (5, 32, "rows", 0.1, True, 0), (5, 32, "last74", 0.1, False, 0))
MUT_CASE = (3, 5, "rows", 0.1, True, 4)          # nothing aligned, a read-out row per sample, remote negatives: every mutation applies


def geom_vocab(g):
    return VOCAB


def prompt(B, form):
    """-> (tokens int64 [77] or [B, 77], EOT column per row).  shared: '<sot> a photo of * <eot>'; rows: the * in column 4 and b filler
    words behind it in row b, so every row has its own EOT column and read-out row; last74: the same with the last row's EOT in column
    74 (its read-out in the last row of the context)"""
    head = [VOCAB - 2, 20, 21, 22, STAR]
    if form == "shared":
        t = torch.zeros(77, dtype=torch.int64)
        t[:6] = torch.tensor(head + [VOCAB - 1])
        return t, [5] * B
    t = torch.zeros(B, 77, dtype=torch.int64)
    eot = []
    for b in range(B):
        fill = 69 if (form == "last74" and b == B - 1) else b
        row = head + [30 + (7 * b + j) % 200 for j in range(fill)] + [VOCAB - 1]
        t[b, :len(row)] = torch.tensor(row)
        eot.append(len(row) - 1)
    return t, eot


class Case:
    """one seeded step: geometry, state dicts (oracle naming), inputs, plan parameters"""

    def __init__(self, B, K, form="shared", dropout=0.1, masks_given=True, n_remote=0, seed=31, steps=0):
        from oracle import keds_oracle as O
        import numpy as np
        self.text, eot = prompt(B, form)
        g = self.g = Geom(B, K, eot, n_remote=n_remote)
        self.dropout, self.masks_given, self.form, self.steps = dropout, masks_given, form, steps
        self.trainer_seed = 5                            # KnowledgeTrainer(seed=...): with `steps`, what the device draws its masks from
        self.name = f"B{B}.K{K}.{form}.p{dropout}.{'given' if masks_given else 'drawn'}" + (f".remote{n_remote}" if n_remote else "")
        self.sd = O.synth_clip_state_dict(embed_dim=g.D, image_resolution=56, vision_layers=1, vision_width=128, vision_patch_size=14, context_length=g.Lc,
                                          vocab_size=VOCAB, transformer_width=g.d, transformer_layers=g.tlayers, seed=7)
        self.sds = dict(i2t=O.synth_im2text_state_dict(g.D, g.middle, g.d, g.ilayers, seed=seed, tag="i2t"),
                        fuse=O.synth_crossformer_state_dict(g.d, g.xlayers, heads=g.xheads, seed=seed, tag="fuse"),
                        cond=O.synth_crossformer_state_dict(g.d, g.xlayers, heads=g.xheads, seed=seed, tag="cond"))
        rs = np.random.RandomState(seed + 1000 * B + K)
        nrm = lambda t: t / t.norm(dim=-1, keepdim=True)   # noqa: E731
        rnd = lambda *sh: torch.from_numpy(rs.standard_normal(sh).astype(np.float32))   # noqa: E731
        self.feats = nrm(rnd(B, g.D)) * 3.0
        self.nbr_img, self.nbr_txt = nrm(rnd(B, K, g.D)), nrm(rnd(B, K, g.D))
        self.other_img_n, self.other_txt_n = (nrm(rnd(n_remote, g.D)), nrm(rnd(n_remote, g.D))) if n_remote else (None, None)
        self.masks = None
        if dropout > 0:
            if masks_given:
                self.masks = [torch.from_numpy((rs.uniform(size=(g.R, g.middle)) >= dropout).astype(np.uint8)) for _ in range(g.ilayers)]
            else:           # what the device draws from (seed, step): the counter hash over the flat index
                self.masks = [tk.dropout_mask_ref(g.R * g.middle, (self.trainer_seed << 32) + steps * 16 + i, dropout).reshape(g.R, g.middle) for i in range(g.ilayers)]
        self.logit_scale = float(self.sd["logit_scale"].float().exp())

    def plan(self, adamw=False):
        return plan(self.g, self.dropout, self.masks_given, self.g.n_remote > 0, adamw=adamw, seed=self.trainer_seed, steps=self.steps, hp=HP)

    def params(self):
        """the given parameter buffers of the plan, from the state dicts"""
        out = {}
        for tag, sd in self.sds.items():
            for k, v in sd.items():
                out[f"p:{tag}.{k}"] = v
        for t in range(self.g.tlayers):
            pf = f"transformer.resblocks.{t}."
            for nm, wk, bk in BLOCK_W:
                out[f"f:{t}.{nm}_w"], out[f"f:{t}.{nm}_b"] = self.sd[pf + wk], self.sd[pf + bk]
            for nm, k in (("ln1", "ln_1"), ("ln2", "ln_2")):
                out[f"f:{t}.{nm}_g"], out[f"f:{t}.{nm}_b"] = self.sd[pf + k + ".weight"], self.sd[pf + k + ".bias"]
        out["f:lnf_g"], out["f:lnf_b"] = self.sd["ln_final.weight"], self.sd["ln_final.bias"]
        out["f:P"], out["f:pos"], out["f:tok"] = self.sd["text_projection"], self.sd["positional_embedding"], self.sd["token_embedding.weight"]
        return out

    def inputs(self):
        g = self.g
        text = self.text if self.text.dim() == 2 else self.text[None].repeat(g.B, 1)
        out = dict(feats=self.feats, nbr_img=self.nbr_img.reshape(g.BK, g.D), nbr_txt=self.nbr_txt.reshape(g.BK, g.D), text=text, logit_scale=self.logit_scale)
        if self.masks is not None and self.masks_given:
            for i, m in enumerate(self.masks):
                out[f"mask{i}"] = m
        if g.n_remote:
            out["other_img_n"], out["other_txt_n"] = self.other_img_n, self.other_txt_n
        return out
