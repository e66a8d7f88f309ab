"""-m gpu: the knowledge stream in fp16 (include/keds_knowledge_f16.h; KnowledgeStream(..., precision="fp16"),
compose_query_features(..., knowledge_precision="fp16")).

Chain equality: keds_im2text_forward_f16, keds_crossformer_forward_f16 (both weight forms) and keds_knowledge_run_f16 (both forms,
side lane on and off) equal their chain of public calls -- keds_cast_f16 / keds_knowledge_pack_rows_h, keds_gemm_bt with the ids
32 - 34 and KEDS_EPI_BIAS_F32_H, keds_cross_attn_core_h, keds_place_token -- bit for bit; the chain's buffers are NaN behind the rows
in use, the entries' workspaces 0xFF bytes (fp16 NaN).

Parity, against the reference-minted module fixtures knowledge_d128.npz / knowledge_d768.npz: the fp16 modules' rel-L2 to the
reference is at most HALF the bf16 modules' on the same inputs -- the rule of test_gpu_fp16.py: the unit roundoff is 8 x smaller,
which leaves 4 x for the fp32 terms both share.  Both numbers are in tests/golden/parity_knowledge_f16.json, and so is the error of
the full-size dual row (dual_vitl14_full.npz under fp16 towers, knowledge_precision="fp16"), which is asserted at 2 x its measured
value: the project's parity-baseline convention.  `python -m tests.test_gpu_knowledge_f16_stream` rewrites that file on a GPU."""
import ctypes as C
import json
import sys
import warnings

import numpy as np
import pytest
import torch

import keds_amd
from keds_amd import _lib
from oracle import keds_oracle as O
from tests import knowledge_check as kc
from tests import test_gpu_knowledge_metric_kernels_edges as ke
from tests.conftest import golden_path
from tests.gpu_util import min_cosine, parity_limits, rel_l2, report
from tests.test_gpu_fp16 import TINY, VITL
from tests.test_gpu_knowledge_f16_edges import _params_h

pytestmark = pytest.mark.gpu

HF, F32 = torch.float16, torch.float32
DEV, P = "cuda", _lib.ptr
PARITY = golden_path("parity_knowledge_f16.json")
_done, _same, _twice, _guarded = ke._done, ke._same, ke._twice, ke._guarded


# ---- the chains of public calls ------------------------------------------------------------------------------------------------------------
def _rows(rows, cols, dtype=HF):
    """a chain buffer: addressable up to the next multiple of 128 rows (and 128 more for sub-ranges), NaN everywhere"""
    return torch.full(((rows + 127) // 128 * 128 + 128, cols), float("nan"), dtype=dtype, device=DEV)


def _gemm(lib, A, W, bias, out, M, N, K, epi, aux=None, aux_i=0, lda=None, ldc=None):
    _done(lib.keds_gemm_bt_ex(A, lda or K, W, bias, out, ldc or N, M, N, K, epi, aux, aux_i, _lib.stream()), f"keds_gemm_bt_ex({epi})")


def _cast(lib, src, rows, cols):
    out = _rows(rows, cols)
    _done(lib.keds_cast_f16(P(src), P(out), rows * cols, _lib.stream()), "keds_cast_f16")
    return out


def _chain_xf(lib, S, T, which, q16, k16, v16, B, K, out):
    dim, inner, BK = S.dim, S.inner, B * K
    Qp, Kp, Vp, att, qcur = (_rows(r, c) for r, c in ((B, inner), (BK, inner), (BK, inner), (B, inner), (B, dim)))
    qin = q16
    for l in range(S.layers):
        w = lambda n: T[f"x{which}.{l}.{n}"].data_ptr()   # noqa: E731
        _gemm(lib, qin, w("wq"), w("bq"), P(Qp), B, inner, dim, _lib.EPI_BIAS_F16_H)
        _gemm(lib, k16, w("wk"), w("bk"), P(Kp), BK, inner, dim, _lib.EPI_BIAS_F16_H)
        _gemm(lib, v16, w("wv"), w("bv"), P(Vp), BK, inner, dim, _lib.EPI_BIAS_F16_H)
        _done(lib.keds_cross_attn_core_h(P(Qp), P(Kp), P(Vp), P(att), B, K, S.heads, inner, _lib.stream()), "keds_cross_attn_core_h")
        if l == S.layers - 1:
            _gemm(lib, P(att), w("wo"), w("bo"), out, B, dim, inner, _lib.EPI_BIAS_F32_H)
        else:
            _gemm(lib, P(att), w("wo"), w("bo"), P(qcur), B, dim, inner, _lib.EPI_BIAS_F16_H)
            qin = P(qcur)


def _chain_xf_fused(lib, S, T, which, q16, kv16, B, K, out, ld_out):
    dim, inner, BK, kv_ld = S.dim, S.inner, B * K, S.layers * 2 * S.inner
    fz = T[f"x{which}.fused"]
    KV, Qp, att = _rows(BK, kv_ld), _rows(B, inner), _rows(B, inner)
    _gemm(lib, kv16, fz.wkv, fz.bkv, P(KV), BK, kv_ld, dim, _lib.EPI_BIAS_F16_H)
    for l in range(S.layers):
        if l == 0:
            _gemm(lib, q16, T[f"x{which}.0.wq"].data_ptr(), T[f"x{which}.0.bq"].data_ptr(), P(Qp), B, inner, dim, _lib.EPI_BIAS_F16_H)
        else:
            _gemm(lib, P(att), fz.wqn[l], fz.bqn[l], P(Qp), B, inner, inner, _lib.EPI_BIAS_F16_H)
        kp = P(KV) + 2 * l * 2 * inner
        _done(lib.keds_cross_attn_core_h(P(Qp), kp, kp + 2 * inner, P(att), B, K, S.heads, kv_ld, _lib.stream()), "keds_cross_attn_core_h")
    last = S.layers - 1
    _gemm(lib, P(att), T[f"x{which}.{last}.wo"].data_ptr(), T[f"x{which}.{last}.bo"].data_ptr(), out, B, dim, inner, _lib.EPI_BIAS_F32_H,
          ldc=ld_out)


def _chain_knowledge(lib, S, T, q, ni, nt, B, K, tokens, fused):
    dim, mid, BK = S.dim, S.middle, B * K
    R = B * (1 + 2 * K)
    rows, h0, h1, m16 = _rows(R, dim), _rows(R, mid), _rows(R, mid), _rows(R + 128, dim)
    st = _lib.stream()
    if fused:
        _done(lib.keds_knowledge_pack_rows_h(P(q), P(ni), P(nt), P(rows), B, K, dim, st), "keds_knowledge_pack_rows_h")
    else:
        for src, r0, n in ((q, 0, B), (ni, B, BK), (nt, B + BK, BK)):
            _done(lib.keds_cast_f16(P(src), P(rows) + 2 * r0 * dim, n * dim, st), "keds_cast_f16")
    _gemm(lib, P(rows), T["w0"].data_ptr(), T["b0"].data_ptr(), P(h0), R, mid, dim, _lib.EPI_BIAS_RELU_F16_H)
    _gemm(lib, P(h0), T["w1"].data_ptr(), T["b1"].data_ptr(), P(h1), R, mid, mid, _lib.EPI_BIAS_RELU_F16_H)
    tok, mb = tokens.data_ptr(), P(m16)
    if fused:
        _gemm(lib, P(h1), T["ow"].data_ptr(), T["ob"].data_ptr(), mb, R, dim, mid, _lib.EPI_BIAS_F16_H_HEADF32, tok + 4 * 2 * dim, B)
        _chain_xf_fused(lib, S, T, 1, mb, mb + 2 * (B + BK) * dim, B, K, tok + 4 * dim, 3 * dim)
        _chain_xf_fused(lib, S, T, 0, mb, mb + 2 * B * dim, B, K, tok, 3 * dim)
        return
    map_f, outf = _rows(R, dim, F32), _rows(B, dim, F32)
    _gemm(lib, P(h1), T["ow"].data_ptr(), T["ob"].data_ptr(), P(map_f), R, dim, mid, _lib.EPI_BIAS_F32_H)
    _done(lib.keds_cast_f16(P(map_f), mb, R * dim, st), "keds_cast_f16")
    _done(lib.keds_place_token(P(map_f), tok, B, dim, 2, 3, st), "keds_place_token")
    for which in range(2):
        nb = mb + 2 * (B + which * BK) * dim
        _chain_xf(lib, S, T, which, mb, nb, nb, B, K, P(outf))
        _done(lib.keds_place_token(P(outf), tok, B, dim, which, 3, st), "keds_place_token")


SHAPES = [(B, K) for B in (1, 3, 33) for K in (1, 16, 32)]
DIM, HEADS, LAYERS, MIDDLE = 128, 2, 3, 128


no_splitk = ke.no_splitk          # keds_knowledge_run_f16 never splits K: the chain of direct GEMM calls must plan the same way


@pytest.mark.parametrize("B,K", SHAPES)
def test_crossformer_forward_f16_equals_its_chain(no_splitk, B, K):
    lib = no_splitk
    S = ke.Stream(DIM, HEADS, LAYERS, MIDDLE, seed=B * 100 + K)
    q, k, _ = ke._inputs(S, B, K, seed=1)
    v = k.clone()
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    for fused in (False, True):
        kp, T = _params_h(S, lib, fused)
        p = kp.fuse
        nbytes = lib.keds_crossformer_workspace_bytes(C.byref(p), B, K)
        q16, k16 = _cast(lib, q, B, DIM), _cast(lib, k, B * K, DIM)
        want_u = _rows(B, DIM, F32)[:B]
        _chain_xf(lib, S, T, 0, P(q16), P(k16), P(k16), B, K, P(want_u))
        run = lambda vv: (lambda ws, n, out: _done(lib.keds_crossformer_forward_f16(C.byref(p), P(q), P(k), P(vv), B, K, out, ws, n, P(flag),   # noqa: E731
                                                                                    _lib.stream()), "keds_crossformer_forward_f16"))
        # a separate v with equal contents takes the layer-by-layer path, `fused` set or not
        assert _same(_twice(run(v), nbytes, B, DIM), want_u), f"fused={fused}: v separate"
        got = _twice(run(k), nbytes, B, DIM)
        if fused:
            want_f = _rows(B, DIM, F32)[:B]
            _chain_xf_fused(lib, S, T, 0, P(q16), P(k16), B, K, P(want_f), DIM)
            torch.cuda.synchronize()
            assert _same(got, want_f), "fused form against its chain"
        else:
            assert _same(got, want_u), "v == k without `fused`"
        assert lib.keds_crossformer_forward_f16(C.byref(p), P(q), P(k), P(k), B, K, P(want_u), P(q16), nbytes - 1, P(flag), _lib.stream()) == -3
    assert int(flag.item()) == 0


@pytest.mark.parametrize("B,K", SHAPES)
def test_knowledge_run_f16_equals_its_chain(no_splitk, B, K):
    """fused and unfused, every token slot of a sentinel-filled [B, 3, dim]; side lane on and off"""
    lib = no_splitk
    S = ke.Stream(DIM, HEADS, LAYERS, MIDDLE, seed=B * 100 + K)
    q, ni, nt = ke._inputs(S, B, K, seed=2)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    for fused in (False, True):
        kp, T = _params_h(S, lib, fused)
        nbytes = lib.keds_knowledge_f16_workspace_bytes(C.byref(kp), B, K)
        cbuf, want = _guarded(B, 3 * DIM, F32)
        _chain_knowledge(lib, S, T, q, ni, nt, B, K, want, fused)
        torch.cuda.synchronize()
        want = want.clone()
        cbuf.fill_(kc.SENT)
        assert bool(torch.isfinite(want).all()) and not bool((want == kc.SENT).any())
        run = lambda ws, n, out: _done(lib.keds_knowledge_run_f16(C.byref(kp), P(q), P(ni), P(nt), B, K, out, ws, n, P(flag), _lib.stream()),   # noqa: E731
                                       "keds_knowledge_run_f16")
        try:
            for lane in (1, 0):
                _lib.check(lib.keds_side_lane_enable(lane), "keds_side_lane_enable")
                got = _twice(run, nbytes, B, 3 * DIM)
                for slot in range(3):
                    sl = slice(slot * DIM, (slot + 1) * DIM)
                    assert _same(got[:, sl], want[:, sl]), f"fused={fused} side lane {lane}: token slot {slot}"
        finally:
            _lib.check(lib.keds_side_lane_enable(1), "keds_side_lane_enable")
        assert lib.keds_knowledge_run_f16(C.byref(kp), P(q), P(ni), P(nt), B, K, P(cbuf), P(cbuf), nbytes - 1, P(flag), _lib.stream()) == -3
        torch.cuda.synchronize()
        assert bool((cbuf == kc.SENT).all())                                        # a short workspace: nothing written
    assert int(flag.item()) == 0


@pytest.mark.parametrize("middle,n_layer", [(128, 1), (256, 2), (128, 3)])
def test_im2text_forward_f16_equals_its_chain(middle, n_layer):
    """the cast, n_layer x (Linear, ReLU) through two buffers in turn, the output Linear; rows on both sides of the 128-row padding"""
    lib = _lib.load()
    dim = DIM
    g = kc._gen(7, dim, middle, n_layer)
    rnd = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    dims = [dim] + [middle] * n_layer
    W = [(rnd(middle, k) / k ** 0.5).to(HF).to(DEV) for k in dims[:-1]] + [(rnd(dim, middle) / middle ** 0.5).to(HF).to(DEV)]
    bias = [(0.1 * rnd(middle)).to(DEV) for _ in range(n_layer)] + [(0.1 * rnd(dim)).to(DEV)]
    p = _lib.Im2TextParams()
    p.dim_in, p.middle, p.dim_out, p.n_layer = dim, middle, dim, n_layer
    for i in range(n_layer):
        p.w[i], p.b[i] = W[i].data_ptr(), bias[i].data_ptr()
    p.out_w, p.out_b = W[-1].data_ptr(), bias[-1].data_ptr()
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    for rows in (1, 129):
        x = rnd(rows, dim).to(DEV)
        cur, h = _cast(lib, x, rows, dim), [_rows(rows, middle), _rows(rows, middle)]
        for i in range(n_layer):
            _gemm(lib, P(cur), P(W[i]), P(bias[i]), P(h[i & 1]), rows, middle, dims[i], _lib.EPI_BIAS_RELU_F16_H)
            cur = h[i & 1]
        want = _rows(rows, dim, F32)[:rows]
        _gemm(lib, P(cur), P(W[-1]), P(bias[-1]), P(want), rows, dim, middle, _lib.EPI_BIAS_F32_H)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(want).all())
        nbytes = lib.keds_im2text_workspace_bytes(C.byref(p), rows)
        run = lambda ws, n, out: _done(lib.keds_im2text_forward_f16(C.byref(p), P(x), rows, out, ws, n, P(flag), _lib.stream()),   # noqa: E731
                                       "keds_im2text_forward_f16")
        assert _same(_twice(run, nbytes, rows, dim), want), f"rows={rows}"
        assert lib.keds_im2text_forward_f16(C.byref(p), P(x), rows, P(want), P(cur), nbytes - 1, P(flag), _lib.stream()) == -3
    assert int(flag.item()) == 0


# ---- parity against the reference-minted fixtures ----------------------------------------------------------------------------------------
def _modules(dim, middle):
    a = keds_amd.IM2TEXT(dim, middle, dim, 2).eval()
    b = keds_amd.CrossFormer(dim, dim, dim, num_layers=3).eval()
    a.load_state_dict(O.synth_im2text_state_dict(dim, middle, dim, 2, seed=11, tag="i2t"))
    b.load_state_dict(O.synth_crossformer_state_dict(dim, 3, seed=12, tag="fuse"))
    return a.cuda(), b.cuda()


def _module_parity(dim, middle):
    """-> {output: (rel-L2 of the fp16 modules, of the bf16 modules, min cosine of the fp16 modules)} against knowledge_d<dim>.npz; the
    CrossFormer of both precisions reads the REFERENCE's IM2TEXT outputs: the same inputs"""
    g = dict(np.load(golden_path(f"knowledge_d{dim}.npz")))
    i2t, xf = _modules(dim, middle)
    x, nb = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["nb"]).cuda()
    y, ynb = torch.from_numpy(g["im2text_x"]).cuda(), torch.from_numpy(g["im2text_nb"]).cuda()
    assert nb.shape[1] <= 32
    got = {}
    for prec in ("bf16", "fp16"):
        got[prec] = {"im2text_x": i2t(x, precision=prec), "im2text_nb": i2t(nb, precision=prec),
                     "crossformer": xf(y[:, None, :], ynb, ynb, precision=prec)}
    assert not i2t.range_tripped() and not xf.range_tripped()
    return {k: (rel_l2(got["fp16"][k], g[k]), rel_l2(got["bf16"][k], g[k]), min_cosine(got["fp16"][k], g[k])) for k in got["fp16"]}


def _recorded():
    with open(PARITY) as f:
        return json.load(f)


@pytest.mark.parametrize("dim,middle", [(128, 128), (768, 512)])
def test_fp16_modules_are_at_most_half_the_bf16_error_from_the_reference(dim, middle):
    rec = _recorded()["modules"][f"d{dim}"]
    for name, (rh, rb, ch) in _module_parity(dim, middle).items():
        c_lim, _ = parity_limits(f"fp16.knowledge_d{dim}.{name}")
        report(f"knowledge_f16.parity.d{dim}.{name}", rel_l2=rh, rel_l2_bf16=rb, ratio=rh / max(rb, 1e-30), min_cosine=ch,
               recorded_rel_l2=rec[name]["rel_l2_fp16"], recorded_rel_l2_bf16=rec[name]["rel_l2_bf16"])
        assert rh <= 0.5 * rb, f"d{dim} {name}: fp16 rel-L2 {rh} > 0.5 x bf16's {rb}"
        assert ch >= c_lim, f"d{dim} {name}: cosine {ch} < {c_lim}"


# ---- compose_query_features ------------------------------------------------------------------------------------------------------------------
def _streams(dim, middle, seed):
    a = keds_amd.IM2TEXT(dim, middle, dim, 2).eval()
    b = keds_amd.CrossFormer(dim, dim, dim, num_layers=3).eval()
    c = keds_amd.CrossFormer(dim, dim, dim, num_layers=3).eval()
    a.load_state_dict(O.synth_im2text_state_dict(dim, middle, dim, 2, seed=seed, tag="i2t"))
    b.load_state_dict(O.synth_crossformer_state_dict(dim, 3, seed=seed, tag="fuse"))
    c.load_state_dict(O.synth_crossformer_state_dict(dim, 3, seed=seed, tag="cond"))
    return keds_amd.KnowledgeStream(a.cuda(), b.cuda(), c.cuda())


def _dual_full():
    """dual_vitl14_full.npz under fp16 towers with knowledge_precision="fp16" -> (identical neighbour sets per database, B, rel-L2 of
    'composed' to the golden, the same with the fp32 streams of the default route)"""
    g = dict(np.load(golden_path("dual_vitl14_full.npz")))
    B, n_db, dim, middle = int(g["batch"]), int(g["n_db"]), 768, 512
    m = keds_amd.build_model(O.synth_clip_state_dict(**VITL, seed=7), fp16=False).cuda().set_precision("fp16")
    database = keds_amd.build_database(O.synth_database(n_db, dim, seed=2002), O.synth_database(n_db, dim, seed=2003, clustered=True),
                                       None, device="cuda")
    img = torch.from_numpy(np.random.RandomState(1001).standard_normal((B, 3, 224, 224)).astype(np.float32)).cuda()
    txt = O.synth_tokens(B, seed=4004).cuda()
    sa, sb = _streams(dim, middle, 21), _streams(dim, middle, 22)
    base = keds_amd.compose_query_features(m, sa, sb, img, txt, database, id_split=265)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                               # no range trip, no tower-guard trip
        out = keds_amd.compose_query_features(m, sa, sb, img, txt, database, id_split=265, knowledge_precision="fp16")
    assert m.precision == "fp16" and not sa.range_tripped() and not sb.range_tripped()
    assert torch.equal(out["query_image_features"], base["query_image_features"])   # the image pass does not depend on the streams
    same = {}
    for name, index, Iref in (("image", database[3], g["I_image"]), ("text", database[4], g["I_text"])):
        _, I0, _ = index.search_gather(base["query_image_features"], 16, normalize=True)
        _, I1, _ = index.search_gather(out["query_image_features"], 16, normalize=True)
        assert torch.equal(I0, I1)                                                   # the neighbour sets are kept
        same[name] = sum(set(I1[r].tolist()) == set(Iref[r, :16].tolist()) for r in range(B))
    return same, B, rel_l2(out["composed"], g["composed"]), rel_l2(base["composed"], g["composed"]), out, g


def test_dual_full_size_row_under_fp16_towers_with_fp16_streams():
    rec = _recorded()["dual_full"]
    same, B, r16, r32, out, g = _dual_full()
    report("knowledge_f16.dual_full", composed_rel_l2=r16, composed_rel_l2_fp32_streams=r32, recorded=rec["composed_rel_l2"],
           neighbour_sets_image=same["image"], neighbour_sets_text=same["text"], of=B)
    assert same["image"] >= B - 2 and same["text"] >= B - 2                        # (test_gpu_fp16.py's rule for the fp16 towers)
    assert torch.isfinite(out["composed"]).all()
    assert r16 <= 2.0 * rec["composed_rel_l2"], f"composed: rel-L2 {r16} > 2 x the recorded {rec['composed_rel_l2']}"


@pytest.fixture
def tiny_batch():
    gt = dict(np.load(golden_path("clip_tiny.npz")))
    g = dict(np.load(golden_path("cirr_batch_tiny.npz")))
    n_db = int(g["n_db"])
    m = keds_amd.build_model(O.synth_clip_state_dict(**TINY, seed=7), fp16=False).cuda().set_precision("fp16")
    database = keds_amd.build_database(O.synth_database(n_db, 128, seed=2002), O.synth_database(n_db, 128, seed=2003), [str(i) for i in range(n_db)])
    return m, database, torch.from_numpy(gt["image"]).cuda(), torch.from_numpy(gt["text"]).cuda()


KEYS = ("tokens_image_stream", "tokens_text_stream", "composed", "image", "mixture", "query_image_features")


def test_the_default_route_of_an_fp16_model_is_unchanged(tiny_batch, monkeypatch):
    """knowledge_precision=None without the environment switch: the streams run keds_knowledge_run_f32 as before -- the tokens are the
    bits of KnowledgeStream(..., precision="fp32") on the retrieved rows, and the features those of the text passes over them.  With
    KEDS_KNOWLEDGE_PRECISION=fp16, or the argument, they are the fp16 stream's."""
    m, database, img, txt = tiny_batch
    monkeypatch.delenv("KEDS_KNOWLEDGE_PRECISION", raising=False)
    sa, sb = _streams(128, 128, 21), _streams(128, 128, 22)
    out = keds_amd.compose_query_features(m, sa, sb, img, txt, database, id_split=265)
    q = out["query_image_features"]
    ti, tt = keds_amd.get_retrieved_features(q, database)
    for prec, kw, env in (("fp32", {}, None), ("fp16", dict(knowledge_precision="fp16"), None), ("fp16", {}, "fp16"), ("fp32", {}, "bf16")):
        if env is None:
            monkeypatch.delenv("KEDS_KNOWLEDGE_PRECISION", raising=False)
        else:
            monkeypatch.setenv("KEDS_KNOWLEDGE_PRECISION", env)
        got = keds_amd.compose_query_features(m, sa, sb, img, txt, database, id_split=265, **kw)
        tok_a, tok_b = sa(q, ti, tt, precision=prec), sb(q, ti, tt, precision=prec)
        assert torch.equal(got["tokens_image_stream"], tok_a) and torch.equal(got["tokens_text_stream"], tok_b), (prec, kw, env)
        both = m.encode_text_img_retrieval(torch.cat([txt, txt]), torch.cat([tok_a, tok_b]), split_ind=265, repeat=False)
        b_n, a_n, mix = keds_amd.ops.mix_normalize(both[len(txt):].float(), both[:len(txt)].float(), 0.5, 0.5)
        assert torch.equal(got["composed"], a_n) and torch.equal(got["image"], b_n) and torch.equal(got["mixture"], mix)
        assert sorted(got) == sorted(KEYS)
        if prec == "fp32":
            assert all(torch.equal(got[k], out[k]) for k in KEYS)
    assert not torch.equal(sa(q, ti, tt, precision="fp16"), sa(q, ti, tt, precision="fp32"))
    assert m.precision == "fp16" and not sa.range_tripped() and not sb.range_tripped()
    with pytest.raises(ValueError):
        keds_amd.compose_query_features(m, sa, sb, img, txt, database, id_split=265, knowledge_precision="fp8")


def test_an_overflowing_hidden_layer_raises_the_flag_and_verify_falls_back(tiny_batch, monkeypatch):
    """One hidden unit of the image stream's IM2TEXT gets a bias of 1e5 and a zero column in the next layer (the same function in
    exact arithmetic, and in fp32): the fp16 hidden layer stores a value beyond 65504 and the stream's flag goes up; verify=True
    returns what the fp32 streams return, with one RuntimeWarning; without it the question is range_tripped()'s."""
    m, database, img, txt = tiny_batch
    monkeypatch.delenv("KEDS_KNOWLEDGE_PRECISION", raising=False)
    sa, sb = _streams(128, 128, 21), _streams(128, 128, 22)
    with torch.no_grad():
        sa.img2text.layers[0][0].bias[5] = 1.0e5
        sa.img2text.layers[1][0].weight[:, 5] = 0.0
    sa.img2text._packed = None
    want = keds_amd.compose_query_features(m, sa, sb, img, txt, database, id_split=265)
    assert all(bool(torch.isfinite(want[k]).all()) for k in KEYS)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = keds_amd.compose_query_features(m, sa, sb, img, txt, database, id_split=265, knowledge_precision="fp16")
    rw = [w for w in rec if issubclass(w.category, RuntimeWarning)]
    assert len(rw) == 1 and "fp16 knowledge stream" in str(rw[0].message), [str(w.message) for w in rw]
    assert all(torch.equal(got[k], want[k]) for k in KEYS) and sorted(got) == sorted(KEYS)
    assert m.precision == "fp16" and not sa.range_tripped() and not sb.range_tripped()          # read and cleared by the call
    # what a verify=False caller sees: the streams themselves, and their flags afterwards
    q = want["query_image_features"]
    ti, tt = keds_amd.get_retrieved_features(q, database)
    tok_a, tok_b = sa(q, ti, tt, precision="fp16"), sb(q, ti, tt, precision="fp16")
    assert sa.range_tripped() is True and sb.range_tripped() is False and sa.range_tripped() is False
    # (the flag is the signal: the overflowed unit meets a zero weight, and what inf x 0 leaves in tok_a is not specified)
    assert tok_a.shape == tok_b.shape and bool(torch.isfinite(tok_b).all())


if __name__ == "__main__":                                     # python -m tests.test_gpu_knowledge_f16_stream: measure, rewrite the json
    doc = {"note": "rel-L2 to the reference-minted goldens, measured on an MI355X; rewritten by python -m tests.test_gpu_knowledge_f16_stream",
           "csrc_sha16": _lib.source_digest(), "modules": {}}
    for d_, mid_ in ((128, 128), (768, 512)):
        doc["modules"][f"d{d_}"] = {k: {"rel_l2_fp16": rh, "rel_l2_bf16": rb, "ratio": rh / rb} for k, (rh, rb, _) in _module_parity(d_, mid_).items()}
    same_, B_, r16_, r32_, _, _ = _dual_full()
    doc["dual_full"] = {"composed_rel_l2": r16_, "composed_rel_l2_fp32_streams": r32_, "neighbour_sets_identical": same_, "batch": B_}
    with open(PARITY, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc), file=sys.stderr)
