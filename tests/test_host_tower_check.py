"""tests/tower_check.py on the CPU: the plans ARE the model (run64 of every plan equals a directly written float64 implementation of the
blocks on every row the pass specifies, and NaN exactly where a read-out row lies outside its sequence), every mutation of a plan is
caught by NaN or by >= 1e-3 relative, and the layout queries of keds_amd/csrc/towers.hip that need no GPU hold."""
import ctypes as C

import pytest
import torch

from keds_amd import _lib
from tests import tower_check as tc

LAYERS, W, HEADS = 3, 256, 4
LENS_256 = [1, 77, 5, 20, 33, 77, 43]
LENS_257 = [1, 77, 5, 20, 33, 77, 44]              # 257 rows: 255 zero rows run behind them
LENS_MAX60 = [60, 1, 17, 60, 32]                   # seq_max < L


# ---- the model, written here independently of tower_check's executor (no shared primitive: an error in either shows) ----------------
def _ln(x, g, b):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), g, b, 1e-5)


def _gelu(x):
    return x / (1.0 + torch.exp(-1.702 * x))


def _mha(qkv, causal):
    """nn.MultiheadAttention's core on one sample: qkv [n, 3 w] -> [n, w], heads of 64 columns"""
    n, w = qkv.shape[0], qkv.shape[1] // 3
    q, k, v = (t.reshape(n, w // 64, 64).permute(1, 0, 2) for t in qkv.split(w, dim=1))
    s = torch.einsum("hid,hjd->hij", q, k) * 64 ** -0.5
    if causal:
        s = s.masked_fill(torch.ones(n, n, dtype=torch.bool).tril().logical_not(), float("-inf"))
    return torch.einsum("hij,hjd->ihd", s.softmax(-1), v).reshape(n, w)


def _blocks64(x, seqs, blocks, causal, taps=None):
    """N pre-LN residual blocks over the samples `seqs` = [(first row, rows)]; rows of no sample get no attention"""
    y = x.clone()
    for k in blocks:
        qkv = _ln(y, k["ln1_g"], k["ln1_b"]) @ k["qkv_w"].T + k["qkv_b"]
        att = torch.zeros_like(y)
        for r0, n in seqs:
            att[r0:r0 + n] = _mha(qkv[r0:r0 + n], causal)
        y = y + att @ k["out_w"].T + k["out_b"]
        y = y + _gelu(_ln(y, k["ln2_g"], k["ln2_b"]) @ k["fc_w"].T + k["fc_b"]) @ k["proj_w"].T + k["proj_b"]
        if taps is not None:
            taps.append(y.clone())
    return y


def _direct(p, weights, x, rows=None, layers=None):
    """the rows the pass specifies: all, the CLS rows, or the read-out row of every sample (NaN outside its sequence)"""
    seqs = [(b * p.S, p.S) for b in range(p.B)] if p.off is None else [(p.off[b], p.off[b + 1] - p.off[b]) for b in range(p.B)]
    y = _blocks64(x.double(), seqs, weights["blocks"][:layers], p.causal)
    if p.tail != "readout":
        return y[p.out_rows]
    out = torch.full((p.B, p.w), float("nan"), dtype=torch.float64)
    for b, (r0, n) in enumerate(seqs):
        r = int(rows[b]) if p.off is None else int(rows[b]) - r0
        if 0 <= r < n and (p.off is None or int(rows[b]) < p.valid):
            out[b] = y[r0 + r]
    return out


@pytest.fixture(scope="module")
def weights():
    return tc.synth_weights(LAYERS, W, seed=3)


def _x(rows, seed=0):
    return torch.randn(rows, W, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _rel(got, want):
    """worst per-element relative difference, inf where exactly one side is NaN"""
    nan_g, nan_w = torch.isnan(got), torch.isnan(want)
    if bool((nan_g != nan_w).any()):
        return float("inf")
    ok = ~nan_w
    return float(((got[ok] - want[ok]).abs() / want[ok].abs().clamp_min(1e-2)).max()) if bool(ok.any()) else 0.0


def _cases():
    out = []
    for flow in tc.FLOWS:
        for B in (1, 15, 16, 31):
            for tail in ("all", "cls"):
                out.append((flow, "tower", dict(B=B, S=17, tail=tail)))
        for B in (16, 31):                          # the remainder rows as a span of their own
            if flow in ("bf16", "fp16", "x3"):
                out.append((flow, "tower", dict(B=B, S=17, tail="cls", split=True)))
                out.append((flow, "tower", dict(B=B, S=17, tail="all", split=True)))
        for B in (1, 3, 7):
            out.append((flow, "readout", dict(B=B, S=77)))
        if flow != "fp8":                           # (the MXFP8 tower refuses packed rows)
            out.append((flow, "packed", dict(B=7, S=77, lens=LENS_256)))
            out.append((flow, "packed", dict(B=7, S=77, lens=LENS_257)))
            out.append((flow, "packed", dict(B=5, S=60, lens=LENS_MAX60)))
    return out


def _rows(kind, kw):
    """read-out columns spread over the sequence, the first and the last column among them, and one row outside"""
    B, S = kw["B"], kw["S"]
    if kind == "tower":
        return None
    if kind == "readout":
        r = [(b * 19) % S for b in range(B)]
        r[-1] = S - 1
        if B > 1:
            r[0] = 0
        if B > 2:
            r[1] = S                                # outside: a NaN row
        return r
    off = [0]
    for n in kw["lens"]:
        off.append(off[-1] + n)
    r = [off[b + 1] - 1 for b in range(B)]
    r[2] = off[-1] + 3                              # outside [0, rows_total): a NaN row
    return r


@pytest.mark.parametrize("flow,kind,kw", _cases(), ids=lambda v: v if isinstance(v, str) else "-".join(f"{k}{x if not isinstance(x, list) else sum(x)}" for k, x in v.items()))
def test_plan_is_the_model(weights, flow, kind, kw):
    p = tc.plan(flow, kind, LAYERS, width=W, heads=HEADS, **kw)
    rows = _rows(kind, kw)
    x = _x(p.valid, seed=p.valid)
    res = tc.run64(p, weights, x, rows)
    got = res["x"][p.out_rows]
    want = _direct(p, weights, x, rows)
    nan_rows = torch.isnan(want).all(1)
    assert torch.isnan(got[nan_rows]).all() and not torch.isnan(got[~nan_rows]).any()
    if kind == "tower":
        assert not bool(nan_rows.any())
    else:
        outside = [not (0 <= r < (p.valid if kind == "packed" else p.S)) for r in rows]
        assert nan_rows.tolist() == outside         # a read-out row outside its sequence, and nothing else
    assert _rel(got, want) <= 1e-9
    if kind == "packed" and p.M > p.valid:          # the zero rows stay finite through the blocks
        stream = "h" if flow in ("bf16", "fp16") else "x"
        assert torch.isfinite(res["bufs"][stream][p.valid:p.M]).all()


def _taps_direct(p, weights, x):
    return [_direct(p, weights, x, layers=l) for l in range(1, p.layers + 1)]


@pytest.mark.parametrize("flow", tc.FLOWS)
@pytest.mark.parametrize("B", (1, 16))
def test_taps_are_the_stream_after_each_block(weights, flow, B):
    p = tc.plan(flow, "tower", LAYERS, B, S=17, tail="all", width=W, heads=HEADS, taps=True)
    x = _x(p.M, seed=9)
    res = tc.run64(p, weights, x)
    for l, want in enumerate(_taps_direct(p, weights, x)):
        assert _rel(res["taps"][l], want) <= 1e-9


# which plan shows each mutation (flow, kind, arguments); every flow that has the step is listed
def _mutation_cases():
    cls31 = dict(B=31, S=17, tail="cls")
    all31 = dict(B=31, S=17, tail="all")
    out = []
    for flow in ("bf16", "fp16", "fp8"):
        out += [("fc_stats_swapped", flow, "tower", all31), ("no_clear", flow, "tower", all31)]
    for flow in ("bf16", "fp16"):
        out += [("rem_stats_row0", flow, "tower", dict(all31, split=True)), ("rem_mlp_skipped", flow, "tower", dict(all31, split=True))]
    out += [("rem_stats_row0", "fp8", "tower", all31), ("rem_mlp_skipped", "fp8", "tower", all31)]
    for flow in ("bf16", "unfolded", "fp16", "fp8", "f32"):
        out += [("cls_ln_gamma", flow, "tower", cls31), ("cls_row_mul1", flow, "tower", cls31), ("cls_out_ldc_w", flow, "tower", cls31)]
    for flow in tc.FLOWS:
        out.append(("q_limit_early", flow, "tower", cls31))
        out.append(("taps_before_proj", flow, "tower", dict(all31, taps=True)))
    for flow in ("bf16", "unfolded", "fp16", "f32", "x3"):
        out.append(("gather_local_packed", flow, "packed", dict(B=7, S=77, lens=LENS_257)))
        out.append(("gather_bound_S", flow, "packed", dict(B=7, S=77, lens=LENS_257)))
    for flow in ("bf16", "unfolded", "fp16", "f32", "x3"):
        out.append(("zero_rows_not_zeroed", flow, "packed", dict(B=7, S=77, lens=LENS_257)))
    return out


def mutation_effect(weights, name, flow, kind, kw):
    """-> (worst relative difference of a specified output between the mutated and the clean plan -- inf for NaN --, rel-L2 and minimum
    row cosine of the mutated output against the clean one over the specified rows)"""
    p = tc.plan(flow, kind, LAYERS, width=W, heads=HEADS, **kw)
    rows = _rows(kind, kw)
    if kind == "packed":
        rows[2] = sum(kw["lens"][:3]) - 1           # every read-out row inside: the clean output has no NaN row
    x = _x(p.valid, seed=11)
    clean, bad = tc.run64(p, weights, x, rows), tc.run64(tc.mutate(p, name), weights, x, rows)

    def outs(r):
        o = [r["x"][p.out_rows]] + [r["taps"][l] for l in sorted(r["taps"])]
        if kind == "packed":
            o.append(r["bufs"]["h" if flow in ("bf16", "fp16") else "x"][p.valid:p.M])      # the zero rows are specified: finite
        return torch.cat([t.reshape(-1, W) for t in o])
    c, b = outs(clean), outs(bad)
    assert torch.isfinite(c).all()
    worst = _rel(b, c)
    if not torch.isfinite(b).all():
        return float("inf"), float("nan"), float("nan")
    l2 = float((b - c).norm() / c.norm())
    cos = float(((b * c).sum(1) / (b.norm(dim=1) * c.norm(dim=1))).min())
    return worst, l2, cos


@pytest.mark.parametrize("name,flow,kind,kw", _mutation_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_mutations_of_a_plan_are_caught(weights, name, flow, kind, kw):
    worst, l2, cos = mutation_effect(weights, name, flow, kind, kw)
    print(f"[mutation] {name} {flow}: worst element {worst:.3g}, rel-L2 {l2:.3g}, min cosine {cos:.6f}")
    assert worst >= 1e-3


def test_every_mutation_has_a_case():
    assert {c[0] for c in _mutation_cases()} == set(tc.MUTATIONS)


# ---- layout queries that need no GPU ------------------------------------------------------------------------------------------------
@pytest.fixture()
def lane():
    lib = _lib.load()
    lib.keds_side_lane_enable(1)
    yield lib
    lib.keds_side_lane_enable(1)


def test_side_rows(lane):
    lib = lane
    for B in range(1, 55):
        assert lib.keds_tower_side_rows(1024, 257, B, 0) == 0, B
    assert lib.keds_tower_side_rows(1024, 257, 55, 0) == 55
    assert lib.keds_tower_side_rows(1024, 17, 829, 0) == 13
    assert [lib.keds_tower_side_rows(256, 17, B, 1) for B in (15, 16, 31)] == [0, 16, 15]
    assert all(lib.keds_tower_side_rows(256, 17, B, 0) == 0 for B in range(1, 200))
    lib.keds_side_lane_enable(0)
    assert lib.keds_tower_side_rows(1024, 257, 55, 0) == 0 and lib.keds_tower_side_rows(256, 17, 16, 1) == 0


@pytest.mark.parametrize("w,S,B", [(256, 17, 1), (256, 17, 15), (256, 17, 16), (256, 17, 31), (256, 77, 7), (512, 17, 4), (1024, 257, 55)])
def test_tower_workspace_is_the_sum_of_the_plan_buffers(lane, w, S, B):
    lib = lane
    assert lib.keds_tower_workspace_bytes(w, S, B) == tc.buffers_bytes(tc.tower_buffers("bf16", w, S, B))
    for flow, f32 in (("f32", 1), ("x3", 2)):
        tp = _lib.TowerParams(w, 1, w // 64, S, 0, None, 0, 0, f32, 0)
        assert lib.keds_tower_workspace_bytes_ex(C.byref(tp), B) == tc.buffers_bytes(tc.tower_buffers(flow, w, S, B))


# ---- whole passes: front end + blocks + read-out ------------------------------------------------------------------------------------
E, VOCAB, L = 128, 512, 77


@pytest.fixture(scope="module")
def full(weights):
    return dict(weights, front=tc.synth_front(W, E, 588, 640, 17, L, VOCAB, seed=4))


def _text_direct(full, tokens, img, splice, cols, normalize, lens=None):
    """encode_text: embedding (+ splice) + positions, causal blocks over each caption's columns, ln_final of the read-out column, proj"""
    f = full["front"]
    out = torch.full((tokens.shape[0], E), float("nan"), dtype=torch.float64)
    for b in range(tokens.shape[0]):
        n = L if lens is None else lens[b]
        if not 0 <= cols[b] < n:
            continue
        e = f["token_emb"][tokens[b]]
        if splice:
            nt, c0 = splice
            e = torch.cat([e[:c0], img[b].double(), e[c0 + 1:]])[:L]
        y = _blocks64((e + f["text_pos"])[:n], [(0, n)], full["blocks"], True)
        out[b] = _ln(y[cols[b]], f["ln_final_g"], f["ln_final_b"]) @ f["proj"].T
    return out / out.norm(dim=1, keepdim=True) if normalize else out


@pytest.mark.parametrize("flow", tc.FLOWS)
@pytest.mark.parametrize("B", (1, 16))
def test_vit_passes_are_the_model(full, flow, B):
    f = full["front"]
    img = torch.randn(B, 3, 56, 56, generator=torch.Generator().manual_seed(B), dtype=torch.float64)
    x = torch.empty(B, 17, W, dtype=torch.float64)
    x[:, 1:] = (tc.im2col64(img, 14, 640) @ f["conv_w"].T).reshape(B, 16, W) + f["vit_pos"][1:]
    x[:, 0] = f["class_emb"] + f["vit_pos"][0]
    taps = []
    y = _blocks64(_ln(x.reshape(B * 17, W), f["ln_pre_g"], f["ln_pre_b"]), [(b * 17, 17) for b in range(B)], full["blocks"], False, taps)
    want = _ln(y[::17], f["ln_post_g"], f["ln_post_b"]) @ f["proj"].T
    for kind, norm in (("vit", 0), ("vit", 1), ("vit_tokens", 0)):
        p = tc.plan_pass(flow, kind, LAYERS, B, normalize=norm)
        res = tc.run64(p, full, None, inputs={"img": img})
        assert _rel(res["bufs"]["out"], want / want.norm(dim=1, keepdim=True) if norm else want) <= 1e-9
        if kind == "vit_tokens":
            for l in range(LAYERS):
                assert _rel(res["taps"][l], taps[l]) <= 1e-9


@pytest.mark.parametrize("flow", tc.FLOWS)
@pytest.mark.parametrize("trim", (0, 1, 2, 3))
@pytest.mark.parametrize("splice", (None, (1, 1), (3, 1), (3, 18)))      # (n_tok, column): at column 1, and ending at a read-out column
def test_text_passes_are_the_model(full, flow, trim, splice):
    B = 3
    g = torch.Generator().manual_seed(5)
    tokens = torch.randint(0, VOCAB, (B, L), generator=g)
    img = torch.randn(B, 3, W, generator=g)[:, :splice[0]] if splice else None
    cols = [0, 20, 76]
    for seq_used, cols in ((0, [0, 20, 76]), (21, [0, 20, 9]), (21, [0, 20, 21]), (77, [76, 20, 0])):
        p = tc.plan_pass(flow, "text", LAYERS, B, rows=cols, seq_used=seq_used, trim=trim, splice=splice, normalize=1)
        res = tc.run64(p, full, None, rows=cols, inputs={"tokens": tokens, "img_tokens": img})
        cut = p.S                                                        # a read-out column outside the cut is a NaN row
        want = _text_direct(full, tokens, img, splice, [c if c < cut else -1 for c in cols], 1)
        assert torch.isnan(res["bufs"]["out"]).all(1).tolist() == [not c < cut for c in cols]
        assert _rel(res["bufs"]["out"], want) <= 1e-9


@pytest.mark.parametrize("flow", ("bf16", "unfolded", "fp16", "f32", "x3"))
@pytest.mark.parametrize("lens,seq_max", [(LENS_256, 77), (LENS_257, 77), (LENS_MAX60, 60)])
def test_packed_text_is_the_model(full, flow, lens, seq_max):
    B = len(lens)
    tokens = torch.randint(0, VOCAB, (B, L), generator=torch.Generator().manual_seed(6))
    off = [sum(lens[:b]) for b in range(B + 1)]
    rows = [off[b + 1] - 1 for b in range(B)]
    rows[1] = off[-1] + 2                                                # outside [0, rows_total): a NaN row
    p = tc.plan_pass(flow, "text_packed", LAYERS, B, lens=lens, seq_max=seq_max)
    res = tc.run64(p, full, None, rows=rows, inputs={"tokens": tokens})
    cols = [lens[b] - 1 for b in range(B)]
    cols[1] = -1
    want = _text_direct(full, tokens, None, None, cols, 0, lens=lens)
    assert torch.isnan(res["bufs"]["out"]).all(1).tolist() == [c < 0 for c in cols]
    assert _rel(res["bufs"]["out"], want) <= 1e-9
    stream = "h" if flow in ("bf16", "fp16") else "x"
    assert torch.isfinite(res["bufs"][stream][max(p.valid, B):p.M]).all()  # the zero rows stay finite


@pytest.mark.parametrize("flow", tc.FLOWS)
def test_text_tokens_are_the_model(full, flow):
    B = 3
    f = full["front"]
    tokens = torch.randint(0, VOCAB, (B, L), generator=torch.Generator().manual_seed(8))
    p = tc.plan_pass(flow, "text_tokens", LAYERS, B)
    res = tc.run64(p, full, None, inputs={"tokens": tokens})
    y = _blocks64((f["token_emb"][tokens] + f["text_pos"]).reshape(B * L, W), [(b * L, L) for b in range(B)], full["blocks"], True)
    assert _rel(res["bufs"]["tokens_out"], _ln(y, f["ln_final_g"], f["ln_final_b"])) <= 1e-9


def test_seq_used_cut_one_short_is_caught(full):
    """the cut at seq_used - 1: the longest caption's read-out column falls outside and its row is NaN"""
    tokens = torch.randint(0, VOCAB, (3, L), generator=torch.Generator().manual_seed(9))
    cols = [3, 20, 9]
    outs = [tc.run64(tc.plan_pass("bf16", "text", LAYERS, 3, rows=cols, seq_used=u, trim=1), full, None, rows=cols,
                     inputs={"tokens": tokens})["bufs"]["out"] for u in (21, 20)]
    assert torch.isfinite(outs[0]).all() and torch.isnan(outs[1][1]).all()


@pytest.mark.parametrize("flow,f32", (("bf16", 0), ("f32", 1), ("x3", 2)))
@pytest.mark.parametrize("B", (1, 16, 31))
def test_pass_workspaces_are_the_sums_of_the_plan_buffers(lane, flow, f32, B):
    """x | max(tower scratch, im2col matrix: it aliases the scratch's head) | read-out rows"""
    lib = lane
    al = lambda n: (n + 255) // 256 * 256
    ro = (B + 127) // 128 * 128 * W * (4 if f32 else 2)
    for S, kind in ((17, "vit"), (L, "text")):
        tower = tc.buffers_bytes(tc.tower_buffers(flow, W, S, B))
        x = al(tc.pad256(B * S) * W * 4)
        tp = _lib.TowerParams(W, LAYERS, HEADS, S, int(kind == "text"), None, 0, 0, f32, 0)
        if kind == "vit":
            p = tc.plan_pass(flow, "vit", LAYERS, B)
            r, c, t = p.buffers["col"]
            col = al(r * c * tc.ESIZE[t])
            vp = _lib.VitParams(tp, 56, 14, 640, E)
            assert lib.keds_vit_workspace_bytes(C.byref(vp), B) == x + max(tower, col) + al(ro)
        else:
            xp = _lib.TextParams(tp, VOCAB, E)
            assert lib.keds_text_workspace_bytes(C.byref(xp), B) == x + tower + al(ro)


# ---- mutations of a whole pass (tower_check.PASS_MUTATIONS) -------------------------------------------------------------------------
def _pass_mutation_cases():
    out = []
    for flow in tc.FLOWS:
        out += [("cls_dropped", flow, "vit", {}), ("no_ln_pre", flow, "vit", {}), ("readout_stride_plus1", flow, "vit", {}),
                ("no_l2norm", flow, "vit", dict(normalize=1)), ("readout_stride_plus1", flow, "text", dict(trim=0)),
                ("readout_stride_plus1", flow, "text", dict(trim=1, seq_used=21)), ("no_l2norm", flow, "text", dict(trim=1, normalize=1))]
    return out


@pytest.mark.parametrize("name,flow,kind,kw", _pass_mutation_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_mutations_of_a_pass_are_caught(full, name, flow, kind, kw):
    """a dropped CLS row, a missing ln_pre, a read-out stride wrong by one and a missing L2 normalisation change the embeddings by
    NaN or >= 1e-3 relative.  (embed_before_zero changes the enqueue order only -- the two steps write disjoint rows --, so this executor
    computes the same; tests/test_host_tower_plan.py holds it to the order)"""
    B, cols = 3, [3, 20, 9]
    g = torch.Generator().manual_seed(12)
    inputs = {"img": torch.randn(B, 3, 56, 56, generator=g, dtype=torch.float64), "tokens": torch.randint(0, VOCAB, (B, L), generator=g)}
    p = tc.plan_pass(flow, kind, LAYERS, B, rows=cols, **kw) if kind == "text" else tc.plan_pass(flow, kind, LAYERS, B, **kw)
    clean = tc.run64(p, full, None, rows=cols, inputs=inputs)["bufs"]["out"]
    bad = tc.run64(tc.mutate_pass(p, name), full, None, rows=cols, inputs=inputs)["bufs"]["out"]
    assert torch.isfinite(clean).all()
    worst = _rel(bad, clean)
    print(f"[pass mutation] {name} {flow} {kind}: worst element {worst:.3g}")
    assert worst >= 1e-3


def test_every_pass_mutation_has_a_case():
    assert {c[0] for c in _pass_mutation_cases()} | {"embed_before_zero"} == set(tc.PASS_MUTATIONS)
