"""Leg A of the training step's bar (docs/kernels.md, "The bar the training step has to pass"), on the CPU: run64 of the written-down plan
(tests/step_check.py) equals a float64 autograd model of the step written here on torch primitives -- which shares nothing with run64
and is itself pinned to oracle.keds_oracle.training_loss in float32 -- every mutation of the plan is visible, and the plan's dataflow
is clean."""
import pytest
import torch
import torch.nn.functional as Fn

from oracle import keds_oracle as O
from tests import step_check as sc

F64 = torch.float64
RUN64_TOL = 1e-9                 # of max |reference| per tensor: the precedent of tests/test_host_tower_check.py
U32 = 2.0 ** -24


# ---- a float64 autograd model of the step --------------------------------------------------------------------------------------------
def model64(case, leaves, dtype=F64):
    """the loss of one step from the state dicts: leaves = {tag: {key: tensor requiring grad}}; everything in `dtype`"""
    g, sd = case.g, {k: v.to(dtype) for k, v in case.sd.items()}
    B, K = g.B, g.K
    x = torch.cat([case.feats, case.nbr_img.reshape(g.BK, g.D), case.nbr_txt.reshape(g.BK, g.D)]).to(dtype)
    i2t = leaves["i2t"]
    for i in range(g.ilayers):
        z = Fn.linear(x, i2t[f"layers.{i}.0.weight"], i2t[f"layers.{i}.0.bias"])
        if case.dropout > 0:
            z = z * case.masks[i].to(dtype) / (1.0 - case.dropout)
        x = torch.relu(z)
    mapped_all = Fn.linear(x, i2t["fc_out.weight"], i2t["fc_out.bias"])
    mapped = mapped_all[:B]

    def xformer(w, kv):
        q = mapped.unsqueeze(1)                                                   # [B, 1, d]
        kv = kv.reshape(B, K, g.d)
        for l in range(g.xlayers):
            pf = f"cross_layers.{l}."
            sp = lambda t, n: t.reshape(B, n, g.xheads, 64).permute(0, 2, 1, 3)   # noqa: E731
            Q = sp(Fn.linear(q, w[pf + "to_q.weight"], w[pf + "to_q.bias"]), 1)
            Kp = sp(Fn.linear(kv, w[pf + "to_k.weight"], w[pf + "to_k.bias"]), K)
            Vp = sp(Fn.linear(kv, w[pf + "to_v.weight"], w[pf + "to_v.bias"]), K)
            o = torch.softmax(Q @ Kp.transpose(-1, -2) * 0.125, -1) @ Vp
            q = Fn.linear(o.permute(0, 2, 1, 3).reshape(B, 1, g.inner), w[pf + "to_out.0.weight"], w[pf + "to_out.0.bias"])
        return q
    tokens = torch.cat([xformer(leaves["fuse"], mapped_all[B:B + g.BK]), xformer(leaves["cond"], mapped_all[B + g.BK:]), mapped.unsqueeze(1)], 1)
    text = case.text if case.text.dim() == 2 else case.text[None].repeat(B, 1)
    emb = sd["token_embedding.weight"][text]
    c0 = g.ins
    h = torch.cat([emb[:, :c0], tokens, emb[:, c0 + 1:g.Lc - 2]], 1) + sd["positional_embedding"]
    causal = torch.full((g.Lc, g.Lc), float("-inf"), dtype=dtype).triu(1)
    for t in range(g.tlayers):
        pf = f"transformer.resblocks.{t}."
        a = Fn.layer_norm(h, (g.d,), sd[pf + "ln_1.weight"], sd[pf + "ln_1.bias"], 1e-5)
        a, _ = Fn.multi_head_attention_forward(a.transpose(0, 1), a.transpose(0, 1), a.transpose(0, 1), g.d, g.theads, sd[pf + "attn.in_proj_weight"],
                                               sd[pf + "attn.in_proj_bias"], None, None, False, 0.0, sd[pf + "attn.out_proj.weight"],
                                               sd[pf + "attn.out_proj.bias"], need_weights=False, attn_mask=causal)
        h = h + a.transpose(0, 1)
        m = Fn.linear(Fn.layer_norm(h, (g.d,), sd[pf + "ln_2.weight"], sd[pf + "ln_2.bias"], 1e-5), sd[pf + "mlp.c_fc.weight"], sd[pf + "mlp.c_fc.bias"])
        h = h + Fn.linear(m * torch.sigmoid(1.702 * m), sd[pf + "mlp.c_proj.weight"], sd[pf + "mlp.c_proj.bias"])
    h = Fn.layer_norm(h, (g.d,), sd["ln_final.weight"], sd["ln_final.bias"], 1e-5)
    tf = h[torch.arange(B), torch.tensor(g.eot) + 2] @ sd["text_projection"]
    img_n, txt_n = Fn.normalize(case.feats.to(dtype), dim=-1, eps=0.0), Fn.normalize(tf, dim=-1, eps=0.0)
    if g.n_remote:
        img_n, txt_n = torch.cat([img_n, case.other_img_n.to(dtype)]), torch.cat([txt_n, case.other_txt_n.to(dtype)])
    logits = case.logit_scale * img_n @ txt_n.t()
    gt = torch.arange(g.N)
    return (Fn.cross_entropy(logits, gt) + Fn.cross_entropy(logits.t(), gt)) / 2


def model_grads(case, dtype=F64):
    leaves = {tag: {k: v.to(dtype).clone().requires_grad_() for k, v in sd.items()} for tag, sd in case.sds.items()}
    loss = model64(case, leaves, dtype)
    loss.backward()
    return loss.detach(), {f"{tag}.{k}": v.grad for tag, lf in leaves.items() for k, v in lf.items()}


def oracle_grads(case):
    leaves = {tag: {k: v.clone().requires_grad_() for k, v in sd.items()} for tag, sd in case.sds.items()}
    loss = O.training_loss(case.sd, leaves["i2t"], leaves["fuse"], leaves["cond"], case.feats, case.nbr_img, case.nbr_txt, case.text, sc.STAR,
                           case.masks, case.dropout, case.other_img_n, case.other_txt_n)
    loss.backward()
    return loss.detach(), {f"{tag}.{k}": v.grad for tag, lf in leaves.items() for k, v in lf.items()}


def _depth(g):
    """the float32 operations one value of the step passes through, forward and backward: the lengths of the sums on the longest path
    (every GEMM's K, every softmax, every LayerNorm), twice -- the first-order worst case of a float32 evaluation is that many unit
    roundoffs of the magnitudes"""
    i2t = g.D + g.middle * (g.ilayers - 1) + g.middle
    xf = g.xlayers * (g.d + g.d + 64 + g.K + g.inner)
    tower = g.tlayers * (g.d + g.d + 64 + g.Lc + g.d + g.d + g.d + 4 * g.d) + g.d + g.d
    return 2 * (i2t + xf + tower + g.D + g.N)


def _off(got, ref, names):
    """worst |got - ref| / max |ref| over the tensors; to_k.bias (zero in exact arithmetic) against the same layer's weight gradient"""
    worst, at = 0.0, None
    for n in names:
        scale = float(ref[n.replace(".bias", ".weight")].abs().max()) if n.endswith("to_k.bias") else float(ref[n].abs().max())
        diff = float((got[n].reshape(ref[n].shape).double() - ref[n].double()).abs().max())
        r = (0.0 if diff == 0 else float("inf")) if scale == 0 else diff / scale       # (one key: the score gradients are zero exactly)
        r = r if r == r else float("inf")
        if r > worst:
            worst, at = r, n
    return worst, at


CASES = sc.CASES
_REF = {}


def _ref(key):
    if key not in _REF:
        case = sc.Case(*key)
        _REF[key] = (case,) + model_grads(case)
    return _REF[key]


@pytest.mark.parametrize("key", CASES, ids=lambda k: "-".join(map(str, k)))
def test_model_is_the_oracle_in_float32(key):
    """the float64 model against O.training_loss (float32 whatever it is handed): the loss and every gradient tensor within
    depth x 2^-24 of the tensor's largest magnitude -- a modelling difference (a wrong splice column, a missing scale) is of order one"""
    case, loss64, g64 = _ref(key)
    loss32, g32 = oracle_grads(case)
    assert loss32.dtype == torch.float32 and set(g32) == set(g64) and len(g64) == 54
    lim = _depth(case.g) * U32
    assert abs(float(loss32) - float(loss64)) <= lim * max(1.0, abs(float(loss64)))
    worst, at = _off(g32, g64, sorted(g64))
    print(f"[model vs oracle] {case.name}: worst {worst:.3g} at {at}, limit {lim:.3g}")
    assert worst <= lim, (at, worst, lim)


@pytest.mark.parametrize("key", CASES, ids=lambda k: "-".join(map(str, k)))
def test_run64_is_the_model(key):
    case, loss, grads = _ref(key)
    p = case.plan()
    assert sc.walk(p) == []
    r = sc.run64(p, case.params(), case.inputs())
    assert r["dirty"] == []
    assert set(r["grads"]) == set(grads) and len(grads) == 54
    assert abs(float(r["loss"]) - float(loss)) <= RUN64_TOL * abs(float(loss))
    worst, at = _off(r["grads"], grads, sorted(grads))
    print(f"[run64 vs model] {case.name}: worst {worst:.3g} at {at}")
    assert worst <= RUN64_TOL, (at, worst)


def _adamw_state(case, p):
    g = torch.Generator().manual_seed(3)
    out = {}
    for n in p.grads():
        r, c, _ = p.buffers[n]
        out["m:" + n[2:]] = 0.01 * torch.randn(r, c, generator=g, dtype=F64)
        out["v:" + n[2:]] = 1e-4 * torch.rand(r, c, generator=g, dtype=F64)
    return out


MUT_KEY = sc.MUT_CASE


def mutation_table():
    """name -> (visible, how, passes today's limits, worst cosine, worst rel-L2) on MUT_KEY"""
    case = sc.Case(*MUT_KEY)
    p = case.plan(adamw=True)
    params = dict(case.params(), **_adamw_state(case, p))
    clean = sc.run64(p, params, case.inputs())
    rows = {}
    for name in sc.MUTATIONS:
        q = sc.mutate(p, name)
        assert q is not None, name
        r = sc.run64(q, params, case.inputs())
        outs = dict(r["grads"])
        ref = dict(clean["grads"])
        if name.startswith("adamw"):
            outs = {n: r["state"][n][:p.buffers[n][0]] for n in p.buffers if n[:2] in ("p:", "m:", "v:")}
            ref = {n: clean["state"][n][:p.buffers[n][0]] for n in outs}
        nan = any(not bool(torch.isfinite(t).all()) for t in outs.values()) or not bool(torch.isfinite(r["loss"]))
        worst = 0.0 if nan else max(float((outs[n] - ref[n]).abs().max()) / max(float(ref[n].abs().max()), 1e-300) for n in ref)
        how = "NaN" if nan else "pad rows written" if r["dirty"] and worst <= RUN64_TOL else f"{worst:.2e}"
        ok, wc, wr = sc.passes_todays_limits(r["loss"], r["grads"], clean["loss"], clean["grads"])
        rows[name] = (nan or worst > RUN64_TOL or bool(r["dirty"]), how, ok, wc, wr, sc.walk(q) != [])
    return rows


def test_every_mutation_is_visible():
    """every mutation changes a run64 output beyond the limit, produces NaN, or writes rows behind a buffer's valid rows; the last
    columns are a REPORT: would the mutated float64 gradients pass today's whole-tensor limits, and does the dataflow walk see it"""
    rows = mutation_table()
    print("| mutation | run64 | passes today's limits | worst cosine | worst rel-L2 | dataflow walk |")
    for name, (vis, how, ok, wc, wr, walked) in rows.items():
        print(f"| `{name}` | {how} | {'yes' if ok else 'no'} | {wc:.5f} | {wr:.2e} | {'finding' if walked else 'clean'} |")
    assert all(v[0] for v in rows.values()), [n for n, v in rows.items() if not v[0]]


def test_mutations_apply_where_the_geometry_allows():
    case = sc.Case(1, 1, "shared", 0.0)
    p = case.plan()
    assert sc.mutate(p, "dw_rows_B_for_BK") is None and sc.mutate(p, "drop_scale_missing_bwd") is None and sc.mutate(p, "local_rows_all_N") is None


def test_walk_sees_missing_initialisation():
    p = sc.Case(3, 5).plan()
    q = p.clone()
    q.links.remove(q.find(op="zero")[0])
    assert any("nobody initialised" in f for f in sc.walk(q))
    q = p.clone()
    q.links.remove([s for s in q.find(op="copy") if s["outs"]["y"][0] == "t0.xm"][0])
    assert any("nobody initialised" in f for f in sc.walk(q))
    r = sc.run64(q, sc.Case(3, 5).params(), sc.Case(3, 5).inputs())
    assert not bool(torch.isfinite(r["loss"]))
