"""Legs B and C of the training step's bar (docs/kernels.md, "The bar the training step has to pass").

B. KnowledgeTrainer.loss_and_grads / apply_gradients equal, BY BITS, the chain of public calls of tests/step_check.plan: the loss, all 54
gradients and, over two consecutive steps, every parameter and both AdamW moments.  The chain makes one C call per link straight through
the library on buffers of its own -- none of keds_amd/train.py's helpers -- with 16-bit and fp32 buffers filled with NaN (pad rows up to
the next multiple of 128 included), byte masks with 0x7F, eight guard rows behind every buffer and the loss workspace of exactly the
reported bytes.  Every launch is told the VALID rows only, so pad and guard rows must keep their fill.

C. Every link is held, on the inputs it actually received (read back from the chain's buffers; an adding link's output cloned before the
launch), to its kernel's existing bar: GEMMs to gemm_check.expected on Case.from_operands, LayerNorm / attention backward / cross core /
loss / l2norm_bwd / QuickGELU / AdamW / colsum to train_check's references, the forward attention to attention_check.check, l2_normalize
to row_check.l2_expected; casts, transposes, gathers, the dropout ReLU pair, the mask and embed_tokens to the bit.

Four mutated chains must DIFFER from the trainer, so the comparison can fail."""
import time
import types

import pytest
import torch

import keds_amd
from keds_amd import _lib
from keds_amd.train import KnowledgeTrainer
from oracle import keds_oracle as O
from tests import attention_check as ac
from tests import gemm_check as gc
from tests import row_check as rc
from tests import step_check as sc
from tests import train_check as tk
from tests.gpu_util import report

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = 8                                            # guard rows behind every chain buffer
NAN = float("nan")
TYPES = {"bf16": torch.bfloat16, "fp32": torch.float32, "u8": torch.uint8, "i32": torch.int32}
FILL = {"bf16": NAN, "fp32": NAN, "u8": 0x7F, "i32": -1}
P = _lib.ptr


def _stop(what, e):
    """a failed launch or a device fault: nothing more of this session may run on the card"""
    pytest.exit(f"{what}: {e}", returncode=3)


class Chain:
    """the plan's links, one public call each, on buffers of its own"""

    def __init__(self, plan, given, logit_scale, links=False):
        """given: name -> tensor of every given buffer of the plan (any device); links: hold every link to its kernel's bar"""
        self.p, self.lib, self.scale = plan, _lib.load(), logit_scale
        self.bufs = {}
        for name, (r, c, t) in plan.buffers.items():
            b = torch.full((sc.pad(r) + G, c), FILL[t], dtype=TYPES[t], device=DEV)
            if name in plan.given:
                b[:r] = given[name].reshape(r, c).to(DEV, TYPES[t])
            self.bufs[name] = b
        self.maps = {}
        self.check = links
        self.worst, self.fails, self.ws_ok = {}, [], True

    # ---- buffers
    def untouched(self):
        """-> names of the buffers whose pad or guard rows lost their fill"""
        bad = []
        for name, (r, c, t) in self.p.buffers.items():
            tail = self.bufs[name][r:]
            ok = torch.isnan(tail).all() if t in ("bf16", "fp32") else (tail == FILL[t]).all()
            if not bool(ok):
                bad.append(name)
        return bad

    def rows(self, ref):
        buf, rows = ref
        if isinstance(rows, range) and rows.step == 1:
            return self.bufs[buf][rows.start:rows.stop]
        return self.bufs[buf][torch.tensor(list(rows), device=DEV)]

    def at(self, ref):
        """device address of the first row of a contiguous view"""
        buf, rows = ref
        assert isinstance(rows, range) and rows.step == 1
        return P(self.bufs[buf][rows.start:])

    def map(self, rows):
        key = tuple(rows)
        if key not in self.maps:
            self.maps[key] = torch.tensor(list(rows), dtype=torch.int32, device=DEV)
        return self.maps[key]

    def valid(self, name):
        return self.bufs[name][:self.p.buffers[name][0]]

    # ---- the launches
    def run(self):
        _lib.ensure_gemm_workspace()
        try:
            for k, s in enumerate(self.p.links):
                pre = {role: self.bufs[ref[0]].clone() for role, ref in s["outs"].items()} if self.check and (s["adds"] or s["op"] in ("ln_bwd", "adamw")) else None
                if self.check and s["op"] == "adamw":
                    pre = {role: self.rows(ref).clone() for role, ref in s["ins"].items()}
                rc_ = getattr(self, "_" + s["op"])(s)
                if rc_ is not None:
                    _lib.check(rc_, f"link {k} {s['op']} {s.get('what', '')}")
                if self.check:
                    getattr(self, "_c_" + s["op"])(s, pre)
            torch.cuda.synchronize()
        except RuntimeError as e:
            _stop("chain", e)
        return self

    def _cols(self, ref):
        return self.p.buffers[ref[0]][1]

    def _copy(self, s):
        (sb, sr), (db, dr) = s["ins"]["x"], s["outs"]["y"]
        self.bufs[db][torch.tensor(list(dr), device=DEV)] = self.bufs[sb][torch.tensor(list(sr), device=DEV)]

    def _zero(self, s):
        self.rows(s["outs"]["y"]).zero_()

    def _cast(self, s):
        x = s["ins"]["x"]
        return self.lib.keds_cast_bf16(self.at(x), self.at(s["outs"]["y"]), len(x[1]) * self._cols(x), _lib.stream())

    def _transpose(self, s):
        x = s["ins"]["x"]
        f32 = 1 if self.p.buffers[x[0]][2] == "fp32" else 0
        return self.lib.keds_transpose_to_bf16(self.at(x), f32, self._cols(x), s["rows"], s["cols"], self.at(s["outs"]["y"]), s["ld_out"], _lib.stream())

    def _gemm(self, s):
        i = s["ins"]
        return self.lib.keds_gemm_bt(self.at(i["a"]), self.at(i["w"]), self.at(i["bias"]) if "bias" in i else None, self.at(s["outs"]["out"]), s["M"], s["N"],
                                     s["K"], s["epi"], None, 0, _lib.stream())

    def _mask(self, s):
        m = s["outs"]["mask"]
        return self.lib.keds_dropout_mask(self.at(m), len(m[1]) * self._cols(m), s["seed"], s["p"], _lib.stream())

    def _drelu_fwd(self, s):
        i = s["ins"]
        return self.lib.keds_dropout_relu_fwd(self.at(i["z"]), self.at(i["mask"]) if "mask" in i else None, s["scale"], self.at(s["outs"]["y"]),
                                              len(i["z"][1]) * self._cols(i["z"]), _lib.stream())

    def _drelu_bwd(self, s):
        i = s["ins"]
        return self.lib.keds_dropout_relu_bwd(self.at(i["dy"]), 0, self.at(i["z"]), self.at(i["mask"]) if "mask" in i else None, s["scale"],
                                              self.at(s["outs"]["dz"]), len(i["z"][1]) * self._cols(i["z"]), _lib.stream())

    def _cross_fwd(self, s):
        i = s["ins"]
        return self.lib.keds_cross_core_fwd(self.at(i["Q"]), self.at(i["K"]), self.at(i["V"]), self.at(s["outs"]["out"]), s["B"], s["Kn"], s["heads"], _lib.stream())

    def _cross_bwd(self, s):
        i, o = s["ins"], s["outs"]
        return self.lib.keds_cross_core_bwd(self.at(i["Q"]), self.at(i["K"]), self.at(i["V"]), self.at(i["dout"]), self.at(o["dQ"]), self.at(o["dK"]),
                                            self.at(o["dV"]), s["B"], s["Kn"], s["heads"], _lib.stream())

    def _embed(self, s):
        i = s["ins"]
        return self.lib.keds_embed_tokens(self.at(i["text"]), self.at(i["table"]), self.at(i["pos"]), self.at(i["tokens"]), s["n_tok"], s["col"],
                                          self.at(s["outs"]["x"]), s["B"], s["Lc"], self._cols(i["table"]), _lib.stream())

    def _rowmap(self, ref):
        """-> (base address, row map or None, rows)"""
        buf, rows = ref
        if isinstance(rows, range):
            return self.at(ref), None, len(rows)
        return P(self.bufs[buf]), P(self.map(rows)), len(rows)

    def _ln_fwd(self, s):
        i, o = s["ins"], s["outs"]
        base, m, n = self._rowmap(i["x"])
        return self.lib.keds_ln_fwd_stats(base, self._cols(i["x"]), m, self.at(i["gamma"]), self.at(i["beta"]), self.at(o["y"]), self.at(o["stats"]), n,
                                          self._cols(i["x"]), _lib.stream())

    def _ln_bwd(self, s):
        i, o = s["ins"], s["outs"]
        assert list(i["x"][1]) == list(o["dx"][1])                      # one row map serves x and dx
        base, m, n = self._rowmap(i["x"])
        dbase, _, _ = self._rowmap(o["dx"])
        return self.lib.keds_ln_bwd(self.at(i["dy"]), base, self._cols(i["x"]), m, self.at(i["stats"]), self.at(i["gamma"]), dbase,
                                    self.at(o["dx_bf"]) if "dx_bf" in o else None, n, self._cols(i["x"]), _lib.stream())

    def _attn(self, s):
        return self.lib.keds_attention(self.at(s["ins"]["qkv"]), self.at(s["outs"]["out"]), s["B"], s["S"], s["heads"], s["causal"], _lib.stream())

    def _attn_bwd(self, s):
        i = s["ins"]
        return self.lib.keds_attention_bwd(self.at(i["qkv"]), self.at(i["dout"]), self.at(s["outs"]["dqkv"]), s["B"], s["S"], s["heads"], s["causal"], _lib.stream())

    def _qgelu_fwd(self, s):
        u = s["ins"]["u"]
        return self.lib.keds_qgelu_fwd(self.at(u), self.at(s["outs"]["y"]), len(u[1]) * self._cols(u), _lib.stream())

    def _qgelu_bwd(self, s):
        i = s["ins"]
        return self.lib.keds_qgelu_bwd(self.at(i["dy"]), self.at(i["u"]), self.at(s["outs"]["du"]), len(i["u"][1]) * self._cols(i["u"]), _lib.stream())

    def _l2n(self, s):
        x = s["ins"]["x"]
        return self.lib.keds_l2_normalize(self.at(x), self.at(s["outs"]["y"]), len(x[1]), self._cols(x), _lib.stream())

    def _l2n_bwd(self, s):
        i = s["ins"]
        return self.lib.keds_l2norm_bwd(self.at(i["x"]), self.at(i["dy"]), self.at(s["outs"]["dx"]), len(i["x"][1]), self._cols(i["x"]), _lib.stream())

    def _loss(self, s):
        i, o = s["ins"], s["outs"]
        nb = int(self.lib.keds_clip_loss_workspace_bytes(s["N"]))
        ws = torch.full((nb + 256,), 0x7F, dtype=torch.uint8, device=DEV)           # exactly the reported bytes; 256 guard bytes behind
        r = self.lib.keds_clip_loss(self.at(i["img"]), self.at(i["txt"]), s["N"], s["B_local"], self._cols(i["img"]), self.scale, self.at(o["loss"]),
                                    self.at(o["dtxt"]), P(ws), nb, _lib.stream())
        self.ws_ok = self.ws_ok and bool((ws[nb:] == 0x7F).all())
        return r

    def _gather(self, s):
        buf, rows = s["ins"]["x"]
        return self.lib.keds_rows_gather(P(self.bufs[buf]), self._cols(s["ins"]["x"]), P(self.map(rows)), self.at(s["outs"]["y"]), len(rows),
                                         self._cols(s["ins"]["x"]), _lib.stream())

    def _colsum(self, s):
        x = s["ins"]["x"]
        f32 = 1 if self.p.buffers[x[0]][2] == "fp32" else 0
        return self.lib.keds_colsum(self.at(x), f32, self._cols(x), len(x[1]), self._cols(x), self.at(s["outs"]["y"]), 0, _lib.stream())

    def _adamw(self, s):
        i, hp = s["ins"], self.p.hp
        n = len(i["p"][1]) * self._cols(i["p"])
        return self.lib.keds_adamw_step(self.at(i["p"]), self.at(i["g"]), self.at(i["m"]), self.at(i["v"]), n, hp["lr"], hp["b1"], hp["b2"], hp["eps"], s["wd"],
                                        s["step"], 1.0, _lib.stream())

    # ---- leg C: every link on its actual inputs
    def _note(self, family, fails, worst, s):
        self.worst[family] = max(self.worst.get(family, 0.0), float(worst))
        for f in fails:
            self.fails.append(f"{s['op']} {s.get('what', s.get('grad', ''))}: {f}")

    def _bits(self, family, got, want, s, by_value=False):
        f = tk.same_value(got, want, family) if by_value else tk.same_bits(got, want, family)
        self._note("bits." + family, [f] if f else [], f.worst, s)

    def _c_copy(self, s, pre):
        self._bits("copy", self.rows(s["outs"]["y"]), self.rows(s["ins"]["x"]), s)

    def _c_zero(self, s, pre):
        y = self.rows(s["outs"]["y"])
        self._bits("zero", y, torch.zeros_like(y), s)

    def _c_cast(self, s, pre):
        self._bits("cast", self.rows(s["outs"]["y"]), self.rows(s["ins"]["x"]).bfloat16(), s)

    def _c_transpose(self, s, pre):
        self._bits("transpose", self.rows(s["outs"]["y"]), tk.transpose_ref(self.rows(s["ins"]["x"]), s["ld_out"]), s)

    def _c_gemm(self, s, pre):
        i = s["ins"]
        buf, rows = s["outs"]["out"]
        resid = pre["out"][rows.start:rows.stop] if s["adds"] else None
        case = gc.Case.from_operands(self.rows(i["a"]), self.rows(i["w"]), self.rows(i["bias"])[0] if "bias" in i else None, resid=resid)
        f = gc.check(self.rows(s["outs"]["out"]), gc.expected(case, s["epi"]), s["what"])
        self._note("gemm." + gc.NAMES[s["epi"]], [f] if f else [], f.worst, s)

    def _c_mask(self, s, pre):
        m = self.rows(s["outs"]["mask"])
        self._bits("dropout_mask", m.reshape(-1).cpu(), tk.dropout_mask_ref(m.numel(), s["seed"], s["p"]), s)

    def _c_drelu_fwd(self, s, pre):
        i = s["ins"]
        want = tk.dropout_fwd_ref(self.rows(i["z"]), self.rows(i["mask"]) if "mask" in i else None, s["scale"])
        self._bits("dropout_relu_fwd", self.rows(s["outs"]["y"]), want, s, by_value=True)

    def _c_drelu_bwd(self, s, pre):
        i = s["ins"]
        want = tk.dropout_bwd_ref(self.rows(i["dy"]), self.rows(i["z"]), self.rows(i["mask"]) if "mask" in i else None, s["scale"])
        self._bits("dropout_relu_bwd", self.rows(s["outs"]["dz"]), want, s, by_value=True)

    def _c_cross_fwd(self, s, pre):
        i = s["ins"]
        Q = self.rows(i["Q"])
        R = tk.cross_reference(Q, self.rows(i["K"]), self.rows(i["V"]), torch.zeros_like(Q), s["B"], s["Kn"], s["heads"])
        self._note("cross_core_fwd", *tk.cross_failures(R, {"out": self.rows(s["outs"]["out"])}), s)

    def _c_cross_bwd(self, s, pre):
        i = s["ins"]
        R = tk.cross_reference(self.rows(i["Q"]), self.rows(i["K"]), self.rows(i["V"]), self.rows(i["dout"]), s["B"], s["Kn"], s["heads"])
        self._note("cross_core_bwd", *tk.cross_failures(R, {n: self.rows(s["outs"][n]) for n in ("dQ", "dK", "dV")}), s)

    def _c_embed(self, s, pre):
        i = s["ins"]
        emb = self.rows(i["table"])[self.rows(i["text"]).long()]
        tok = self.rows(i["tokens"]).reshape(s["B"], s["n_tok"], -1)
        c0, n = s["col"], s["n_tok"]
        want = torch.cat([emb[:, :c0], tok, emb[:, c0 + 1:s["Lc"] - (n - 1)]], 1) + self.rows(i["pos"])      # one fp32 addition
        self._bits("embed_tokens", self.rows(s["outs"]["x"]), want.reshape(s["B"] * s["Lc"], -1), s)

    def _c_ln_fwd(self, s, pre):
        i, o = s["ins"], s["outs"]
        self._note("ln_fwd_stats", *tk.ln_fwd_failures(self.rows(i["x"]), self.rows(i["gamma"])[0], self.rows(i["beta"])[0], self.rows(o["y"]), self.rows(o["stats"]),
                                                       s.get("what", "")), s)

    def _c_ln_bwd(self, s, pre):
        i, o = s["ins"], s["outs"]
        buf, rows = o["dx"]
        r = self.p.buffers[buf][0]
        src = torch.tensor(list(rows), device=DEV)
        case = types.SimpleNamespace(x=self.bufs[i["x"][0]][:r], dx0=pre["dx"][:r], src=src, dy=self.rows(i["dy"]), gamma=self.rows(i["gamma"])[0],
                                     dim=self._cols(o["dx"]), name=s["what"])
        ref, e = tk.ln_bwd_reference(case, self.rows(i["stats"]))
        dx = self.bufs[buf][:r]
        fs = [tk.held(dx[src], ref, e, torch.float32, s["what"] + " dx")]
        worst = fs[0].worst
        rest = torch.ones(r, dtype=torch.bool, device=DEV)
        rest[src] = False
        fs.append(tk.same_bits(dx[rest], pre["dx"][:r][rest], s["what"] + " dx outside the written rows") if bool(rest.any()) else [])
        if "dx_bf" in o:
            fs.append(tk.same_bits(self.rows(o["dx_bf"]), dx[src].bfloat16(), s["what"] + " dx_bf16 is not the rounding of the stored dx"))
        self._note("ln_bwd", [f for f in fs if f], worst, s)

    def _c_attn(self, s, pre):
        f = ac.check(self.rows(s["outs"]["out"]), ac.Case(self.rows(s["ins"]["qkv"]), s["B"], s["S"], s["heads"], s["causal"]))
        self._note("attention", [f] if len(f) else [], f.worst, s)

    def _c_attn_bwd(self, s, pre):
        i = s["ins"]
        ref3 = tk.att_reference(self.rows(i["qkv"]), self.rows(i["dout"]), s["B"], s["S"], s["heads"], s["causal"])
        self._note("attention_bwd", *tk.att_failures(ref3, self.rows(s["outs"]["dqkv"])), s)

    def _c_qgelu_fwd(self, s, pre):
        self._note("qgelu_fwd", *tk.qgelu_failures(self.rows(s["ins"]["u"]), y=self.rows(s["outs"]["y"])), s)

    def _c_qgelu_bwd(self, s, pre):
        i = s["ins"]
        self._note("qgelu_bwd", *tk.qgelu_failures(self.rows(i["u"]), dy=self.rows(i["dy"]), du=self.rows(s["outs"]["du"])), s)

    def _c_l2n(self, s, pre):
        self._note("l2_normalize", *rc.norm_failures(self.rows(s["outs"]["y"]), rc.l2_expected(self.rows(s["ins"]["x"])), "l2_normalize"), s)

    def _c_l2n_bwd(self, s, pre):
        i = s["ins"]
        self._note("l2norm_bwd", *tk.l2b_failures(self.rows(i["x"]), self.rows(i["dy"]), self.rows(s["outs"]["dx"])), s)

    def _c_loss(self, s, pre):
        i, o = s["ins"], s["outs"]
        R = tk.loss_reference(self.rows(i["img"]), self.rows(i["txt"]), s["B_local"], self.scale)
        self._note("clip_loss", *tk.loss_failures(R, self.rows(o["loss"]).reshape(1), self.rows(o["dtxt"])), s)

    def _c_gather(self, s, pre):
        self._bits("rows_gather", self.rows(s["outs"]["y"]), self.rows(s["ins"]["x"]), s)

    def _c_colsum(self, s, pre):
        self._note("colsum", *tk.colsum_failures(self.rows(s["ins"]["x"]), None, self.rows(s["outs"]["y"])[0], False, s["grad"]), s)

    def _c_adamw(self, s, pre):
        hp = dict(self.p.hp, wd=s["wd"])
        R = tk.adamw_reference(pre["p"], pre["g"], pre["m"], pre["v"], s["step"], 1.0, hp)
        o = s["outs"]
        self._note("adamw", *tk.adamw_failures(R, self.rows(o["p"]), self.rows(o["m"]), self.rows(o["v"]), s["name"]), s)


# ---- the trainer beside it -----------------------------------------------------------------------------------------------------------
_CLIP = {}


def _trainer(case):
    g = case.g
    if "m" not in _CLIP:
        _CLIP["m"] = keds_amd.build_model(dict(case.sd), fp16=False).cuda()
    mods = (keds_amd.IM2TEXT(g.D, g.middle, g.d, g.ilayers), keds_amd.CrossFormer(g.d, g.d, g.d, num_layers=g.xlayers),
            keds_amd.CrossFormer(g.d, g.d, g.d, num_layers=g.xlayers))
    for m, tag in zip(mods, ("i2t", "fuse", "cond")):
        m.load_state_dict(case.sds[tag])
    mods = tuple(m.cuda() for m in mods)
    other = (case.other_img_n, case.other_txt_n)

    class Remote(KnowledgeTrainer):
        """4 fixed unit rows of another rank behind the local ones (N > B local)"""

        def _gather_negatives(self, img_n, txt_n):
            if other[0] is None:
                return super()._gather_negatives(img_n, txt_n)
            return torch.cat([img_n, other[0].to(img_n.device)]).contiguous(), torch.cat([txt_n, other[1].to(txt_n.device)]).contiguous()
    return Remote(_CLIP["m"], *mods, lr=sc.HP["lr"], beta1=sc.HP["b1"], beta2=sc.HP["b2"], eps=sc.HP["eps"], wd=sc.HP["wd"], dropout=case.dropout, topk=g.K,
                  seed=case.trainer_seed)


def _given(case, plan, state=None):
    """the given buffers of a plan: parameters (or the previous step's), zero moments (or the previous step's), the inputs"""
    out = dict(case.params())
    out.update(case.inputs())
    for n in plan.buffers:
        if n[:2] in ("m:", "v:"):
            out[n] = torch.zeros(plan.buffers[n][0], plan.buffers[n][1])
    if state is not None:
        out.update(state)
    return out


def _loss_and_grads(tr, case, nbrs=None):
    ni, nt = (case.nbr_img.cuda(), case.nbr_txt.cuda()) if nbrs is None else nbrs
    try:
        out = tr.loss_and_grads(case.feats.cuda(), ni, nt, case.text, sc.STAR, case.masks if case.masks_given else None)
        torch.cuda.synchronize()
    except RuntimeError as e:
        _stop("trainer", e)
    return out


def _differences(tr, chain, loss, grads, after_apply):
    """names of what differs by bits between the trainer and the chain"""
    p = chain.p
    bad = [] if torch.equal(loss.reshape(1), chain.valid("loss").reshape(1)) else ["loss"]
    assert sorted(grads) == [n[2:] for n in p.grads()] and len(grads) == 54
    for n, gt in grads.items():
        if not torch.equal(gt.reshape(-1), chain.valid("g:" + n).reshape(-1)):
            bad.append("g:" + n)
    if after_apply:
        for n in grads:
            lin = tr.lin[n.rsplit(".", 1)[0]].lin
            prm = lin.weight if n.endswith(".weight") else lin.bias
            for what, got in (("p:", prm.detach()), ("m:", tr._opt[n][0]), ("v:", tr._opt[n][1])):
                if not torch.equal(got.reshape(-1), chain.valid(what + n).reshape(-1)):
                    bad.append(what + n)
    return bad


@pytest.mark.parametrize("key", sc.CASES, ids=lambda k: "-".join(map(str, k)))
def test_trainer_equals_chain_and_every_link_holds(key):
    t0 = time.time()
    case = sc.Case(*key)
    tr = _trainer(case)
    state = None
    for step in range(2):
        case.steps = step
        plan = case.plan(adamw=True)
        assert plan.steps == tr.steps == step
        loss, grads = _loss_and_grads(tr, case)
        grads = {n: g.clone() for n, g in grads.items()}
        tr.apply_gradients(dict(grads))
        chain = Chain(plan, _given(case, plan, state), case.logit_scale, links=True).run()
        assert chain.untouched() == [] and chain.ws_ok
        bad = _differences(tr, chain, loss, grads, True)
        assert bad == [], f"step {step}: the trainer and the chain differ by bits in {bad[:8]} ({len(bad)})"
        assert bool(torch.isfinite(chain.valid("loss")).all()) and all(bool(torch.isfinite(chain.valid(n)).all()) for n in plan.grads())
        assert chain.fails == [], "\n".join(chain.fails[:12])
        report("train_step_chain.links", case=case.name, step=step, links=len(plan.links), **{k: round(v, 4) for k, v in sorted(chain.worst.items())})
        state = {n: chain.valid(n).clone() for n in plan.buffers if n[:2] in ("m:", "v:") or (n[:2] == "p:")}
    dt = time.time() - t0
    report("train_step_chain.time", case=case.name, seconds=round(dt, 2))
    print(f"[time] {case.name}: {dt:.2f} s")


@pytest.mark.parametrize("name", ["bias_grad_pad_rows", "cond_dkv_row_minus1", "dx_bf_stale", "local_rows_all_N"])
def test_mutated_chain_differs(name):
    """the comparison can fail: a chain with one wiring defect differs from the trainer by bits (local_rows_all_N: the remote rows'
    gradient lands behind the B local rows of dtxt_n, which the clean chain leaves as filled)"""
    case = sc.Case(*sc.MUT_CASE)
    tr = _trainer(case)
    loss, grads = _loss_and_grads(tr, case)
    plan = case.plan()
    clean = Chain(plan, _given(case, plan), case.logit_scale).run()
    assert _differences(tr, clean, loss, grads, False) == [] and clean.untouched() == []
    mut = sc.mutate(plan, name)
    assert mut is not None
    chain = Chain(mut, _given(case, mut), case.logit_scale).run()
    bad = _differences(tr, chain, loss, grads, False)
    print(f"[mutated chain] {name}: differs in {len(bad)} tensors, pad rows written in {chain.untouched()}")
    assert bad or chain.untouched()


def test_step_on_a_database():
    """step() = retrieval on the device + loss_and_grads + apply_gradients: the parameters after one step equal, by bits, the chain run
    on get_retrieved_features' own output"""
    case = sc.Case(8, 16, "shared", 0.1, False)
    tr = _trainer(case)
    ib, tb = O.synth_database(3000, case.g.D, seed=2002), O.synth_database(3000, case.g.D, seed=2003)
    database = keds_amd.build_database(ib, tb, None, device="cuda")
    ni, nt = keds_amd.get_retrieved_features(case.feats.cuda(), database, None, topk=case.g.K)
    case.nbr_img, case.nbr_txt = ni.float().cpu(), nt.float().cpu()
    plan = case.plan(adamw=True)
    chain = Chain(plan, _given(case, plan), case.logit_scale).run()
    try:
        loss = tr.step(case.feats.cuda(), database, case.text, sc.STAR)
        torch.cuda.synchronize()
    except RuntimeError as e:
        _stop("step", e)
    assert torch.equal(loss.reshape(1), chain.valid("loss").reshape(1))
    for n, L in tr.lin.items():
        for kind, prm in (("weight", L.lin.weight), ("bias", L.lin.bias)):
            assert torch.equal(prm.detach().reshape(-1), chain.valid(f"p:{n}.{kind}").reshape(-1)), f"{n}.{kind}"
    assert chain.untouched() == []
