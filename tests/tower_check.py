"""A tower pass as DATA: the ordered chain of kernel launches a pass of keds_amd/csrc/towers.hip (planned in tower_plan.h) has to make, written
from the model's arithmetic (a pre-LN residual block, a CLS or read-out row after the last block, a causal mask) and the documented
properties of the epilogues (include/keds_hip.h) -- and a float64 executor of such a chain that models the BUFFERS as state.

plan(flow, kind, ...) -> Plan: steps (dicts) + the named buffers with their shapes and storage types + the rows of `x` the pass
is specified to produce.  A step names its op, its row span (first row, row count, row step), its input and output buffers and, for
the LayerNorm-folded flows, the statistics buffer it reads, the one it adds into and the one it clears.

run64(plan, weights, inputs) executes the steps in float64 with no rounding.  Every buffer starts as NaN (pad rows included), the
statistics buffers too; a RESID_STATS step ADDS into its buffer, an LN consumer reads one buffer and clears the other, rowstats_cast
writes.  A chain that relies on a buffer being zero, or on rows nobody wrote, therefore comes out NaN.

tests/test_host_tower_check.py holds the plans to a directly written float64 model and shows that the mutations of a plan are caught;
tests/test_gpu_tower_compositions.py runs the same steps one public call at a time beside the pass itself and compares by bits."""
import copy
import math

import torch

FLOWS = ("bf16", "unfolded", "fp16", "fp8", "f32", "x3")
KINDS = ("tower", "readout", "packed")      # keds_tower_forward's rectangular rows; a read-out row per sample; the same on packed rows
TAILS = ("all", "cls", "readout")
LN_EPS = 1e-5
SPLITK_BYTES = 8 << 20
F64 = torch.float64


def pad256(n):
    return (n + 255) // 256 * 256


class Plan:
    """steps: list of dicts; buffers: name -> (rows, cols, type) with type in bf16 / fp16 / fp32 / e4m3 / scale / stat / pair (two fp16
    planes); outputs: name -> list of x rows (or None: every row of that output); geometry as attributes"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.steps, self.buffers = [], {}

    def add(self, op, **kw):
        kw["op"] = op
        self.steps.append(kw)
        return kw

    def clone(self):
        p = copy.copy(self)
        p.steps = copy.deepcopy(self.steps)
        p.buffers = dict(self.buffers)
        return p

    def find(self, **match):
        return [s for s in self.steps if all(s.get(k) == v for k, v in match.items())]


def _spans(flow, M, split):
    """row spans of the block GEMMs: (first row, rows, kernel family, lane)"""
    Mm = M // 256 * 256
    if flow == "fp8":
        return [(0, Mm, "mx", "main")] + ([(Mm, M - Mm, "16", "side")] if M > Mm else [])
    if split and flow in ("bf16", "fp16", "x3") and 0 < Mm < M:
        return [(0, Mm, _kern(flow), "main"), (Mm, M - Mm, _kern(flow), "side")]
    return [(0, M, _kern(flow), "main")]


def _kern(flow):
    return {"f32": "f32", "x3": "x3"}.get(flow, "16")


def tower_buffers(flow, w, seq, B):
    """the carving of one tower's scratch for B x seq rows, in order: name -> (rows, cols, type); its bytes are the sum of the
    buffers' 256-aligned sizes"""
    Mp = pad256(B * seq)
    if flow in ("f32", "x3"):
        t = "pair" if flow == "x3" else "fp32"
        return {"ln": (Mp, w, t), "qkv": (Mp, 3 * w, "fp32"), "att": (Mp, w, "fp32"), "hid": (Mp, 4 * w, t)}
    Mm = B * seq // 256 * 256
    hs = "bf16" if flow == "unfolded" else "fp16"            # the folded flows keep the residual stream in fp16 there
    act = "fp16" if flow == "fp16" else "bf16"
    return {"h": (Mp, w, hs), "qkv": (Mp, 3 * w, act), "att": (Mp, w, act), "hid": (Mp, 4 * w, act), "st1": (Mp, 2, "stat"),
            "st2": (Mp, 2, "stat"), "xq": (Mm, w, "e4m3"), "xs": (Mm, w // 32, "scale"), "aq": (Mm, w, "e4m3"),
            "as": (Mm, w // 32, "scale"), "hq": (Mm, 4 * w, "e4m3"), "hs": (Mm, 4 * w // 32, "scale"),
            "splitk": (1, SPLITK_BYTES, "scale")}


ESIZE = {"bf16": 2, "fp16": 2, "fp32": 4, "e4m3": 1, "scale": 1, "stat": 8, "pair": 4}


def buffers_bytes(bufs):
    return sum(pad256(r * c * ESIZE[t]) for r, c, t in bufs.values())


def plan(flow, kind, layers, B, S=None, lens=None, tail="all", width=256, heads=4, causal=None, split=False, rows=None, taps=False):
    """The chain of one tower pass over the fp32 stream `x` [rows, width].
    kind "tower": B x S rectangular rows, tail "all" or "cls" (keds_tower_forward, last_cls_only).
    kind "readout": the same with one read-out row per sample (rows: local columns; tail "readout"; x[b] = that row on return).
    kind "packed": sample b owns lens[b] rows, S = seq_max, rows GLOBAL; the pass runs whole 256-row tiles of zero rows behind them.
    split: the remainder rows behind the last full 256-row tile as their own span (the side lane), where the flow has one."""
    assert flow in FLOWS and kind in KINDS and tail in TAILS
    w = width
    causal = (kind != "tower") if causal is None else causal
    off = None
    if kind != "tower":
        tail = "readout"
    if kind == "packed":
        assert flow != "fp8" and causal
        off = [0]
        for n in lens:
            off.append(off[-1] + n)
        valid = off[-1]
        M = pad256(valid) if pad256(valid) <= pad256(B * S) else valid
    else:
        valid = M = B * S
    p = Plan(flow=flow, kind=kind, layers=layers, B=B, S=S, w=w, heads=heads, causal=causal, tail=tail, M=M, valid=valid, off=off,
             rows=rows, split=split)
    eff = flow
    if flow == "fp8" and M < 256:
        eff = "bf16"                     # fewer than 256 rows: no full tile, every row is a remainder row of the 16-bit kernels
    p.eff = eff
    p.buffers = {"x": (pad256(B * S), w, "fp32"), **tower_buffers(flow, w, S, B)}
    spans = _spans(eff, M, split)
    p.spans = spans
    folded = eff in ("bf16", "fp16", "fp8")
    k16 = eff in ("bf16", "fp16", "fp8", "unfolded")
    stream = "h" if folded else "x"      # where the residual stream lives between the blocks
    lnbuf = "h" if k16 else "ln"
    one = tail != "all"
    if kind == "packed" and M > valid:
        p.add("zero", buf="x", r0=valid, n=M - valid)        # zero rows up to the next 256-row tile: they belong to no sample
        if eff != "x3":                                      # (x3: the out-proj reads ln_1's output there, which is finite)
            p.add("zero", buf="att", r0=valid, n=M - valid)  # nobody's queries: their attention output is cleared once
    if folded:
        p.add("stats_cast", src="x", dst="h", st="st1", r0=0, n=M)
        if eff == "fp8":
            p.add("quant", src="x", dst="xq", r0=0, n=spans[0][1])

    def gemm(l, wname, epi, a, out, sp, **kw):
        r0, n, kern, lane = sp
        return p.add("gemm", layer=l, w=wname, epi=epi, a=(a, r0, 1), out=(out, r0, 1), n=n, kern=kern, lane=lane, st_r0=r0, **kw)

    def pre(l, sp):                      # ln_1 + in_proj
        if folded:
            a = "xq" if sp[2] == "mx" else "h"
            gemm(l, "qkv", "ln_bias", a, "qkv", sp, st_read="st1", st_clear="st2")
        else:
            p.add("ln", layer=l, g="ln1", src=("x", sp[0], 1), dst=(lnbuf, sp[0], 1), n=sp[1], lane=sp[3])
            gemm(l, "qkv", "bias", lnbuf, "qkv", sp)

    def post(l, sp, last):               # out-proj + ln_2 + MLP
        mx = sp[2] == "mx"
        if folded:
            gemm(l, "out", "resid_stats", "aq" if mx else "att", "h", sp, st_add="st2", qout="xq" if mx else None)
            gemm(l, "fc", "ln_qgelu", "xq" if mx else "h", "hq" if mx else "hid", sp, st_read="st2", st_clear="st1")
            # (the last block's output feeds no further ln_1: no statistics; the MXFP8 epilogue always adds them)
            gemm(l, "proj", "resid_stats", "hq" if mx else "hid", "h", sp, st_add=None if last and not mx else "st1",
                 qout="xq" if mx else None)
        else:
            gemm(l, "out", "resid", "ln" if eff == "x3" else "att", "x", sp)
            p.add("ln", layer=l, g="ln2", src=("x", sp[0], 1), dst=(lnbuf, sp[0], 1), n=sp[1], lane=sp[3])
            gemm(l, "fc", "qgelu", lnbuf, "hid", sp)
            gemm(l, "proj", "resid", "hid", "x", sp)
        if taps:
            p.add("tap", layer=l, src=(stream, sp[0], 1), n=sp[1], lane=sp[3])

    def attention(q_limit, out):
        q8 = spans[0][1] if eff == "fp8" and q_limit == S else 0
        p.add("attn", qkv="qkv", out=out, B=B, S=S, off=off, causal=causal, q_limit=q_limit, q8_rows=q8, out_q="aq" if q8 else None)

    for l in range(layers):
        last = l == layers - 1
        if eff != "x3" or l == 0:
            for sp in spans:
                pre(l, sp)
        if last and one:
            break
        attention(S, "ln" if eff == "x3" else "att")
        for sp in spans:
            post(l, sp, last)
            if eff == "x3" and not last:
                pre(l + 1, sp)           # the next block's ln_1 and in_proj ride on the span's lane
    if one:
        _tail(p, layers - 1, eff, stream, lnbuf, k16, folded)
    elif folded:
        p.add("cast", src=("h", 0, 1), dst=("x", 0, 1), n=M)
    # what the pass is specified to produce
    if tail == "all":
        p.out_rows = list(range(M))
    elif tail == "cls":
        p.out_rows = [b * S for b in range(B)]
    else:
        p.out_rows = list(range(B))
    return p


def _tail(p, l, eff, stream, lnbuf, k16, folded):
    """after the last block one row per sample is read: its attention, out-proj, ln_2 and MLP run on those B rows"""
    B, S, w = p.B, p.S, p.w
    kern = _kern(eff)
    compact = p.tail == "readout" or eff == "x3"          # B rows gathered into dense [B, w] buffers; else CLS rows in place (stride S)
    if compact:
        p.buffers["att_c"] = (pad256(B), w, p.buffers["att"][2])
        p.buffers["x_c"] = (pad256(B), w, "fp32")
    if p.tail == "cls":
        if folded:
            p.add("cast", src=("h", 0, S), dst=("x", 0, S), n=B)
        p.add("attn", qkv="qkv", out="att", B=B, S=S, off=None, causal=p.causal, q_limit=1, q8_rows=0, out_q=None)
        if compact:
            p.add("copy", src=("att", 0, S), dst=("att_c", 0, 1), n=B)
            p.add("copy", src=("x", 0, S), dst=("x_c", 0, 1), n=B)
    else:
        p.add("attn", qkv="qkv", out="att", B=B, S=S, off=p.off, causal=p.causal, q_limit=S, q8_rows=0, out_q=None)
        bound = p.valid if p.off is not None else S
        glob = p.off is not None
        p.add("gather", src="att", dst="att_c", rows="rows", bound=bound, S=S, glob=glob, n=B)
        p.add("gather", src=stream, dst="x_c", rows="rows", bound=bound, S=S, glob=glob, n=B)
    xa, rs = ("x_c", 1) if compact else ("x", S)
    aa = "att_c" if compact else "att"
    if eff == "x3":
        p.add("split", src=("att_c", 0, 1), dst=("ln", 0, 1), n=B, plane=pad256(B) * w)
        aa = "ln"
    g = dict(layer=l, n=B, kern=kern, lane="main", st_r0=0, tail=True)
    p.add("gemm", w="out", epi="resid", a=(aa, 0, rs if aa == "att" else 1), out=(xa, 0, rs), **g)
    p.add("ln", layer=l, g="ln2", src=(xa, 0, rs), dst=(lnbuf, 0, 1), n=B, lane="main", tail=True)
    p.add("gemm", w="fc", epi="qgelu", a=(lnbuf, 0, 1), out=("hid", 0, 1), **g)
    p.add("gemm", w="proj", epi="resid", a=("hid", 0, 1), out=(xa, 0, rs), **g)
    if compact:
        p.add("copy", src=("x_c", 0, 1), dst=("x", 0, 1 if p.tail == "readout" else S), n=B)


# ---- the float64 executor ---------------------------------------------------------------------------------------------------------
def _idx(ref, n):
    _, r0, rs = ref
    return torch.arange(n) * rs + r0


def qgelu(y):
    return y * torch.sigmoid(1.702 * y)


def layernorm64(x, g, b):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + LN_EPS) * g + b


def attention64(qkv, spans, heads, causal, q_limit):
    """qkv [rows, 3 w] -> {row: output row} for the first q_limit rows of every (first row, length) span"""
    w = qkv.shape[1] // 3
    out = {}
    for r0, n in spans:
        t = qkv[r0:r0 + n]
        nq = min(q_limit, n)
        o = torch.empty(nq, w, dtype=F64)
        for h in range(heads):
            q, k, v = (t[:, i * w + h * 64:i * w + h * 64 + 64] for i in range(3))
            s = q[:nq] @ k.T / 8.0
            if causal:
                s = s + torch.full((nq, n), float("-inf"), dtype=F64).triu(1)
            o[:, h * 64:h * 64 + 64] = torch.softmax(s, -1) @ v
        out[r0] = o
    return out


def run64(p, weights, x, rows=None, inputs=None):
    """x: the fp32 stream the blocks start from (None for a whole pass of plan_pass, which builds it from `inputs`: img / tokens /
    img_tokens) -> dict: "x" (the stream buffer after the pass, [pad rows, w]), "taps" ({layer: [M, w]}), "bufs" (every buffer)"""
    bufs = {n: torch.full((r, c), float("nan"), dtype=F64) for n, (r, c, _) in p.buffers.items() if n != "splitk"}
    if x is not None:
        bufs["x"][:x.shape[0]] = x.double()
    taps = {}
    blocks = weights["blocks"]
    for s in p.steps:
        op = s["op"]
        if op in ("im2col", "patch", "cls", "embed", "readout"):
            _run_front(p, s, weights, inputs, bufs, rows)
        elif op == "zero":
            bufs[s["buf"]][s["r0"]:s["r0"] + s["n"]] = 0.0
        elif op == "stats_cast":
            r = slice(s["r0"], s["r0"] + s["n"])
            v = bufs[s["src"]][r]
            bufs[s["dst"]][r] = v
            bufs[s["st"]][r] = torch.stack([v.sum(1), (v * v).sum(1)], 1)
        elif op == "quant":
            r = slice(s["r0"], s["r0"] + s["n"])
            bufs[s["dst"]][r] = bufs[s["src"]][r]
        elif op in ("cast", "copy", "split"):
            bufs[s["dst"][0]][_idx(s["dst"], s["n"])] = bufs[s["src"][0]][_idx(s["src"], s["n"])]
        elif op == "tap":
            taps.setdefault(s["layer"], torch.full((p.M, p.w), float("nan"), dtype=F64))[_idx(s["src"], s["n"])] = \
                bufs[s["src"][0]][_idx(s["src"], s["n"])]
        elif op == "gather":
            for b in range(s["n"]):
                r = int(rows[b])
                ok = 0 <= r < s["bound"]
                src = r if s["glob"] else b * s["S"] + r
                bufs[s["dst"]][b] = bufs[s["src"]][src] if ok else float("nan")
        elif op == "ln":
            k = weights["front"] if s["layer"] is None else blocks[s["layer"]]
            v = bufs[s["src"][0]][_idx(s["src"], s["n"])]
            bufs[s["dst"][0]][_idx(s["dst"], s["n"])] = layernorm64(v, k[s["g"] + "_g"], k[s["g"] + "_b"])
        elif op == "attn":
            spans = [(b * s["S"], s["S"]) for b in range(s["B"])] if s["off"] is None else \
                [(s["off"][b], s["off"][b + 1] - s["off"][b]) for b in range(s["B"])]
            for r0, o in attention64(bufs[s["qkv"]], spans, p.heads, s["causal"], s["q_limit"]).items():
                for i in range(o.shape[0]):
                    dst = s["out_q"] if r0 + i < s["q8_rows"] else s["out"]
                    bufs[dst][r0 + i] = o[i]
        elif op == "gemm":
            k = blocks[s["layer"]]
            n = s["n"]
            A = bufs[s["a"][0]][_idx(s["a"], n)]
            W, b = k[s["w"] + "_w"], k[s["w"] + "_b"]
            oi = _idx(s["out"], n)
            if s["epi"].startswith("ln"):
                ln = "ln1" if s["w"] == "qkv" else "ln2"
                K = W.shape[1]
                st = bufs[s["st_read"]][s["st_r0"]:s["st_r0"] + n]
                mean = st[:, :1] / K
                rstd = 1.0 / torch.sqrt(st[:, 1:] / K - mean * mean + LN_EPS)
                Wf = W * k[ln + "_g"]
                y = rstd * (A @ Wf.T - mean * Wf.sum(1)) + (b + W @ k[ln + "_b"])
                if s.get("st_clear"):
                    bufs[s["st_clear"]][s["st_r0"]:s["st_r0"] + n] = 0.0
            else:
                y = A @ W.T + b
            if "qgelu" in s["epi"]:
                y = qgelu(y)
            if s["epi"].startswith("resid"):
                y = bufs[s["out"][0]][oi] + y
                if s.get("st_add"):
                    bufs[s["st_add"]][s["st_r0"]:s["st_r0"] + n] += torch.stack([y.sum(1), (y * y).sum(1)], 1)
                if s.get("qout"):
                    bufs[s["qout"]][oi] = y
            bufs[s["out"][0]][oi] = y
        else:
            raise ValueError(op)
    return {"x": bufs["x"], "taps": taps, "bufs": bufs}


def synth_weights(layers, w, seed=0):
    """float64 block weights of O(1) activations: gamma near 1, weights ~ N(0, 1/K)"""
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    blocks = []
    for _ in range(layers):
        k = {}
        for ln in ("ln1", "ln2"):
            k[ln + "_g"], k[ln + "_b"] = 1.0 + 0.2 * r(w), 0.2 * r(w)
        for name, n, kk in (("qkv", 3 * w, w), ("out", w, w), ("fc", 4 * w, w), ("proj", w, 4 * w)):
            k[name + "_w"], k[name + "_b"] = r(n, kk) * (1.5 / math.sqrt(kk)), 0.1 * r(n)
        blocks.append(k)
    return {"blocks": blocks}


# ---- mutations of a plan: each is a defect the glue could have ----------------------------------------------------------------------
MUTATIONS = ("fc_stats_swapped", "no_clear", "rem_stats_row0", "cls_ln_gamma", "cls_row_mul1", "cls_out_ldc_w", "gather_local_packed",
             "gather_bound_S", "q_limit_early", "rem_mlp_skipped", "zero_rows_not_zeroed", "taps_before_proj")


def mutate(p, name):
    """-> a copy of the plan with the defect; raises LookupError when the plan has no step the defect applies to"""
    q = p.clone()
    L = p.layers - 1
    hit = []
    if name == "fc_stats_swapped":
        hit = [s for s in q.find(op="gemm", w="fc") if s.get("st_read")]
        for s in hit:
            s["st_read"], s["st_clear"] = s["st_clear"], s["st_read"]
    elif name == "no_clear":
        hit = [s for s in q.find(op="gemm", w="qkv") if s.get("st_clear")]
        for s in hit:
            s["st_clear"] = None
    elif name == "rem_stats_row0":
        hit = [s for s in q.find(op="gemm") if s["st_r0"] > 0 and (s.get("st_read") or s.get("st_add"))]
        for s in hit:
            s["st_r0"] = 0
    elif name == "cls_ln_gamma":
        hit = [s for s in q.find(op="ln", tail=True)] if p.tail == "cls" else []
        for s in hit:
            s["g"] = "ln1"
    elif name == "cls_row_mul1":
        hit = [s for s in q.find(op="ln", tail=True) if s["src"][2] > 1]
        for s in hit:
            s["src"] = (s["src"][0], 0, 1)
    elif name == "cls_out_ldc_w":
        hit = [s for s in q.find(op="gemm", w="out", tail=True) if s["out"][2] > 1]
        for s in hit:
            s["out"] = (s["out"][0], 0, 1)
    elif name == "gather_local_packed":
        hit = [s for s in q.find(op="gather") if s["glob"]]
        for s in hit:
            s["glob"] = False
    elif name == "gather_bound_S":
        hit = [s for s in q.find(op="gather") if s["glob"]]
        for s in hit:
            s["bound"] = p.S
    elif name == "q_limit_early":
        hit = [s for s in q.find(op="attn") if s["q_limit"] > 1][-1:] if p.tail == "cls" and p.layers > 1 else []
        for s in hit:
            s["q_limit"], s["q8_rows"], s["out_q"] = 1, 0, None
    elif name == "rem_mlp_skipped":
        hit = [s for s in q.find(op="gemm", layer=L) if s["st_r0"] > 0 and s["w"] in ("fc", "proj")]
        q.steps = [s for s in q.steps if not any(s is h for h in hit)]
    elif name == "zero_rows_not_zeroed":
        hit = q.find(op="zero")
        q.steps = [s for s in q.steps if s["op"] != "zero"]
    elif name == "taps_before_proj":
        hit = q.find(op="tap")
        for t in hit:
            q.steps.remove(t)
            proj = [s for s in q.find(op="gemm", layer=t["layer"], w="proj") if s["out"][1] == t["src"][1]][0]
            q.steps.insert(q.steps.index(proj), t)
    else:
        raise ValueError(name)
    if not hit:
        raise LookupError(f"{name}: no such step in this plan")
    return q


# ---- whole passes: a front end in front of the blocks, a read-out behind them --------------------------------------------------------
PASSES = ("vit", "vit_tokens", "text", "text_packed", "text_tokens")


def plan_pass(flow, kind, layers, B, width=256, heads=4, embed_dim=128, res=56, patch=14, L=77, rows=None, seq_used=0, trim=1, lens=None,
              seq_max=None, splice=None, normalize=0, cls_only=True, split=False):
    """The chain of keds_vit_run ("vit"), keds_vit_run_tokens, keds_text_run_ex ("text": seq_used and the trim mode 0 - 3 of
    keds_text_trim_enable), keds_text_run_packed and keds_text_run_tokens.  splice: (n_tok, insert_col) of spliced img_tokens."""
    assert kind in PASSES
    w = width
    if kind in ("vit", "vit_tokens"):
        g = res // patch
        S, Gp = g * g + 1, g * g
        kpad = (3 * patch * patch + 63) // 64 * 64
        tail = "cls" if kind == "vit" and cls_only else "all"
        p = plan(flow, "tower", layers, B, S=S, tail=tail, width=w, heads=heads, causal=False, split=split, taps=kind == "vit_tokens")
        ct = "fp32" if flow in ("f32", "x3") else "fp16" if flow == "fp16" else "bf16"
        p.buffers["col"] = (pad256(B * Gp), kpad, ct)
        front = [dict(op="im2col", res=res, patch=patch, kpad=kpad), dict(op="patch", G=Gp, kpad=kpad), dict(op="cls"),
                 dict(op="ln", layer=None, g="ln_pre", src=("x", 0, 1), dst=("x", 0, 1), n=B * S, lane="main")]
        p.steps = front + p.steps
        p.readout = dict(op="readout", S=S, rows=None, g="ln_post", normalize=normalize)
        p.steps.append(p.readout)
        p.res, p.patch, p.kpad = res, patch, kpad
    elif kind == "text_tokens":
        p = plan(flow, "tower", layers, B, S=L, tail="all", width=w, heads=heads, causal=True, split=split)
        p.steps.insert(0, dict(op="embed", L=L, Lx=L, splice=None, packed=False))
        p.buffers["tokens_out"] = (B * L, w, "fp32")
        p.steps.append(dict(op="ln", layer=None, g="ln_final", src=("x", 0, 1), dst=("tokens_out", 0, 1), n=B * L, lane="main"))
    elif kind == "text":
        cut, tr = trim in (1, 2), trim in (1, 3)
        Lx = seq_used if cut and 0 < seq_used < L else L
        if tr:
            p = plan(flow, "readout", layers, B, S=Lx, width=w, heads=heads, split=split)
            p.readout = dict(op="readout", S=1, rows=None, g="ln_final", normalize=normalize)
        else:
            p = plan(flow, "tower", layers, B, S=Lx, tail="all", width=w, heads=heads, causal=True, split=split)
            p.readout = dict(op="readout", S=Lx, rows="rows", g="ln_final", normalize=normalize)
        p.steps.insert(0, dict(op="embed", L=L, Lx=Lx, splice=splice, packed=False))
        p.steps.append(p.readout)
    else:
        p = plan(flow, "packed", layers, B, S=seq_max, lens=lens, width=w, heads=heads)
        zero_x = [s for s in p.steps if s["op"] == "zero" and s["buf"] == "x"]
        for s in zero_x:                     # (the zero rows are cleared in front of the embedding)
            p.steps.remove(s)
        p.steps = zero_x + [dict(op="embed", L=L, Lx=seq_max, splice=splice, packed=True)] + p.steps
        p.readout = dict(op="readout", S=1, rows=None, g="ln_final", normalize=normalize)
        p.steps.append(p.readout)
    p.pass_kind, p.E, p.L = kind, embed_dim, L
    # the LayerNorm of the read-out rows is a GEMM operand: addressable up to the next multiple of 128 rows
    p.buffers["ro"] = ((B + 127) // 128 * 128, w, "fp32" if flow in ("f32", "x3") else "fp16" if flow == "fp16" else "bf16")
    p.buffers["out"] = (B, embed_dim, "fp32")
    return p


# ---- mutations of a whole pass ---------------------------------------------------------------------------------------------------
# (embed_before_zero changes the order only: the embedding writes the samples' own rows, the zero steps the rows behind them, so the
# float64 executor, which runs the steps one after the other, computes the same; it shows in the comparison of the plans)
PASS_MUTATIONS = ("cls_dropped", "embed_before_zero", "no_ln_pre", "readout_stride_plus1", "no_l2norm")


def mutate_pass(p, name):
    """-> a copy of a plan_pass() plan with the defect; LookupError when the plan has no step the defect applies to"""
    q = p.clone()
    if name == "cls_dropped":
        hit = q.find(op="cls")
        q.steps = [s for s in q.steps if s["op"] != "cls"]
    elif name == "embed_before_zero":
        hit = [s for s in q.find(op="zero") if q.steps.index(s) < q.steps.index(q.find(op="embed")[0])] if q.find(op="embed") else []
        if hit:
            e = q.find(op="embed")[0]
            q.steps.remove(e)
            q.steps.insert(0, e)
    elif name == "no_ln_pre":
        hit = q.find(op="ln", g="ln_pre")
        q.steps = [s for s in q.steps if not (s["op"] == "ln" and s.get("g") == "ln_pre")]
    elif name == "readout_stride_plus1":
        hit = q.find(op="readout")
        for s in hit:
            s["S"] += 1
    elif name == "no_l2norm":
        hit = [s for s in q.find(op="readout") if s["normalize"]]
        for s in hit:
            s["normalize"] = 0
    else:
        raise ValueError(name)
    if not hit:
        raise LookupError(f"{name}: no such step in this plan")
    q.readout = (q.find(op="readout") or [None])[0]
    return q


def synth_front(w, E, kreal, kpad, S, L, vocab, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    conv = torch.zeros(w, kpad, dtype=F64)
    conv[:, :kreal] = r(w, kreal) / math.sqrt(kreal)
    f = {"conv_w": conv, "class_emb": r(w), "vit_pos": 0.3 * r(S, w), "proj": r(E, w) / math.sqrt(w), "token_emb": r(vocab, w),
         "text_pos": 0.3 * r(L, w)}
    for ln in ("ln_pre", "ln_post", "ln_final"):
        f[ln + "_g"], f[ln + "_b"] = 1.0 + 0.2 * r(w), 0.2 * r(w)
    return f


def im2col64(img, P, kpad):
    B, _, R, _ = img.shape
    g = R // P
    t = img.double().reshape(B, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, 3 * P * P)
    return torch.nn.functional.pad(t, (0, kpad - 3 * P * P))


def embed64(p, s, f, inputs, x):
    """token embedding + splice + positional embedding into the rows of x (packed: sample b's first lens[b] columns at off[b])"""
    B, Lx = p.B, s["Lx"]
    tok, img = inputs["tokens"], inputs.get("img_tokens")
    n_tok, col0 = s["splice"] if s["splice"] else (0, 0)
    for b in range(B):
        r0, n = (p.off[b], min(Lx, p.off[b + 1] - p.off[b])) if s["packed"] else (b * Lx, Lx)
        for t in range(n):
            if img is not None and col0 <= t < col0 + n_tok:
                v = img[b, t - col0].double()
            else:
                src = t - (n_tok - 1) if img is not None and t >= col0 + n_tok else t
                v = f["token_emb"][int(tok[b, src])]
            x[r0 + t] = v + f["text_pos"][t]


def _run_front(p, s, weights, inputs, bufs, rows):
    """the steps of plan_pass that run64 does not know -> True when `s` was one of them"""
    f = weights["front"]
    op = s["op"]
    if op == "im2col":
        c = im2col64(inputs["img"], s["patch"], s["kpad"])
        bufs["col"][:c.shape[0]] = c
    elif op == "patch":
        G, S = s["G"], p.S
        for b in range(p.B):
            bufs["x"][b * S + 1:b * S + 1 + G] = bufs["col"][b * G:(b + 1) * G] @ f["conv_w"].T + f["vit_pos"][1:]
    elif op == "cls":
        bufs["x"][torch.arange(p.B) * p.S] = f["class_emb"] + f["vit_pos"][0]
    elif op == "embed":
        embed64(p, s, f, inputs, bufs["x"])
    elif op == "readout":
        out = torch.full((p.B, p.E), float("nan"), dtype=F64)
        for b in range(p.B):
            r = int(rows[b]) if s["rows"] else 0
            if 0 <= r < s["S"]:
                out[b] = layernorm64(bufs["x"][b * s["S"] + r], f[s["g"] + "_g"], f[s["g"] + "_b"]) @ f["proj"].T
        if s["normalize"]:
            out = out / out.norm(dim=1, keepdim=True)
        bufs["out"] = out
    else:
        return False
    return True
