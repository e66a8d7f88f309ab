"""The multi-query cross-attention core (keds_amd/csrc/cross_seq.hip, keds_cross_attn_seq) alone at its edges (tests/cross_seq_check.py:
the reference, the bound, the cases; tests/test_host_cross_seq_check.py: proof that the bound passes a CPU model of the kernel and
catches its mutations), and keds_crossformer_forward_seq against the chain of its public pieces, to the bit.

Every launch: K and V as two column ranges of one wide buffer whose other columns are NaN, Q and out under strides of their own
(q_ld != o_ld != 64 heads), NaN rows before and behind every operand, 8 sentinel rows before and behind the output and sentinels in the
columns between its rows.  Every element of every launch is compared with the bound; nothing outside the B Lq x 64 heads window may
change; the same launch twice gives equal bits; what the launch site recorded equals the plan.  Only arguments the entry points accept
are passed to a launch; the argument errors asserted are those returned before any launch."""
import ctypes as C

import pytest
import torch

from keds_amd import _lib
from tests import cross_seq_check as cs
from tests import knowledge_check as kc
from tests.gpu_util import report
from tests.test_gpu_knowledge_metric_kernels_edges import (_around, _bytes, _cast, _done, _gemm, _pad_rows, _same, _twice, _xf_params)

pytestmark = pytest.mark.gpu

GR = 8
SENT, BF, F32 = cs.SENT, cs.BF, torch.float32
P = _lib.ptr
DEV = "cuda"
NAN = float("nan")
E_ARG, E_WORKSPACE = -1, -3


def _operand(buf):
    """a CPU buffer [rows, ld] on the device with NaN rows before and behind it"""
    dev = torch.full((buf.shape[0] + 2 * GR, buf.shape[1]), NAN, dtype=buf.dtype, device=DEV)
    dev[GR:GR + buf.shape[0]] = buf.to(DEV)
    return dev[GR:GR + buf.shape[0]]


def _out(rows, ld):
    buf = torch.full((rows + 2 * GR, ld), SENT, dtype=BF, device=DEV)
    return buf, buf[GR:GR + rows]


def _launch(lib, lay, q, kv, out):
    B, Lq, Lk, H = lay.B, lay.Lq, lay.Lk, lay.H
    rc = lib.keds_cross_attn_seq(q.data_ptr(), kv.data_ptr() + 2 * lay.ko, kv.data_ptr() + 2 * lay.vo, out.data_ptr(), B, Lq, Lk, H, lay.q_ld,
                                 lay.kv_ld, lay.o_ld, _lib.stream())
    _done(rc, f"keds_cross_attn_seq B{B}.Lq{Lq}.Lk{Lk}.H{H}")
    info = (C.c_int * 8)()
    assert lib.keds_cross_seq_last_launch(info) == 0
    return list(info)


@pytest.mark.parametrize("Lq,Lk", cs.pairs())
def test_cross_attn_seq(Lq, Lk):
    lib = _lib.load()
    msgs, worst, launches = [], {}, 0
    for B, H in cs.BH:
        for regime in cs.REGIMES:
            what = f"Lq{Lq}.Lk{Lk}.B{B}.H{H}.{regime}"
            Q, K, V = cs.inputs(B, Lq, Lk, H, regime, seed=Lq * 1000 + Lk)
            lay = cs.Layout(Q, K, V, B, Lq, Lk, H)
            R = cs.reference(Q, K, V, B, Lq, Lk, H)
            q, kv = _operand(lay.qbuf), _operand(lay.kvbuf)
            obuf, out = _out(B * Lq, lay.o_ld)
            obuf2, out2 = _out(B * Lq, lay.o_ld)
            rec = _launch(lib, lay, q, kv, out)
            rec2 = _launch(lib, lay, q, kv, out2)
            launches += 2
            if not (rec == rec2 == cs.plan(B, Lq, Lk, H)):
                msgs.append(f"{what}: launched {rec}, planned {cs.plan(B, Lq, Lk, H)}")
            if not _same(obuf, obuf2):
                msgs.append(f"{what}: two launches differ")
            got = obuf.cpu()
            f, w = cs.failures(got[GR:GR + B * Lq, :lay.inner], R, B, Lq, H, what)
            msgs += f
            worst[regime] = max(worst.get(regime, 0.0), w)
            got[GR:GR + B * Lq, :lay.inner] = SENT
            if not bool((got == SENT).all()):
                msgs.append(f"{what}: written outside the {B * Lq} x {lay.inner} window")
    for regime, w in sorted(worst.items()):
        report(f"cross_seq_edges.Lq{Lq}.Lk{Lk}.{regime}", worst_ratio=w)
    assert launches == 2 * len(cs.BH) * len(cs.REGIMES)
    assert not msgs, f"{len(msgs)} failures:\n" + "\n".join(msgs[:30])


def test_query_chunks_beyond_288_queries():
    """Lq = 600: three workgroups of 256 / 256 / 88 queries per (sample, head), each staging K and V again"""
    lib = _lib.load()
    B, H, Lq = 2, 2, 600
    for Lk, regime in ((33, "ramp"), (257, "flat")):
        Q, K, V = cs.inputs(B, Lq, Lk, H, regime, seed=Lk)
        lay = cs.Layout(Q, K, V, B, Lq, Lk, H)
        obuf, out = _out(B * Lq, lay.o_ld)
        rec = _launch(lib, lay, _operand(lay.qbuf), _operand(lay.kvbuf), out)
        assert rec == cs.plan(B, Lq, Lk, H) and rec[7] == 3 and rec[4] == B * H * 3
        got = obuf.cpu()
        f, w = cs.failures(got[GR:GR + B * Lq, :lay.inner], cs.reference(Q, K, V, B, Lq, Lk, H), B, Lq, H, f"Lq600.Lk{Lk}.{regime}")
        report(f"cross_seq_edges.Lq600.Lk{Lk}.{regime}", worst_ratio=w)
        assert not f, "\n".join(f)
        got[GR:GR + B * Lq, :lay.inner] = SENT
        assert bool((got == SENT).all())


# ---- argument errors ----------------------------------------------------------------------------------------------------------------
def _xf(dim, heads, layers, seed):
    Ls = kc.fuse_inputs(dim, 64 * heads, layers, "random", seed)
    p, keep = _xf_params(Ls, dim, heads)
    T = {f"{l}.{n}": t for l in range(layers) for n, t in zip(Ls[l], keep[1][l * 8:(l + 1) * 8])}
    return p, T, keep


def test_argument_errors_return_before_any_launch():
    lib = _lib.load()
    st = _lib.stream()
    bbuf = torch.full((64 + 2 * GR, 256), SENT, dtype=BF, device=DEV)
    x = bbuf[GR:GR + 64].data_ptr()
    ok = dict(B=1, Lq=4, Lk=4, heads=2, q_ld=128, kv_ld=128, o_ld=128)

    def call(ptrs=(x, x, x, x), **kw):
        a = dict(ok, **kw)
        return lib.keds_cross_attn_seq(*ptrs, a["B"], a["Lq"], a["Lk"], a["heads"], a["q_ld"], a["kv_ld"], a["o_ld"], st)

    for i in range(4):
        ptrs = [x] * 4
        ptrs[i] = None
        assert call(tuple(ptrs)) == E_ARG
        ptrs[i] = x + 2                                   # not 16-byte aligned
        assert call(tuple(ptrs)) == E_ARG
    for Lk in (0, 289, -1, 1 << 20):
        assert call(Lk=Lk) == E_ARG
        assert "Lk=" in _lib.last_error() and "[1,288]" in _lib.last_error()
    for kw in (dict(Lq=0), dict(Lq=-3), dict(B=0), dict(B=-1), dict(heads=0), dict(heads=-2)):
        assert call(**kw) == E_ARG, kw
    for name in ("q_ld", "kv_ld", "o_ld"):
        assert call(**{name: 127}) == E_ARG               # below 64 heads
        assert call(**{name: 120}) == E_ARG
        assert call(**{name: 132}) == E_ARG               # not a multiple of 8
        assert call(**{name: 129}) == E_ARG
    # the CrossFormer on sequences: the same limits, bad parameters, and the short workspace
    p, T, keep = _xf(128, 2, 1, seed=3)
    fbuf = torch.full((80, 128), SENT, dtype=F32, device=DEV)
    f = fbuf[GR:GR + 64]
    y = f.data_ptr()
    B, Lq, Lk = 2, 3, 5
    nbytes = lib.keds_crossformer_seq_workspace_bytes(C.byref(p), B, Lq, Lk)
    assert nbytes > 0 and nbytes % 256 == 0
    wbuf, ws = _bytes(nbytes)
    fwd = lambda q=y, k=y, v=y, o=y, w=ws.data_ptr(), n=nbytes, B=B, Lq=Lq, Lk=Lk, p=p: lib.keds_crossformer_forward_seq(   # noqa: E731
        C.byref(p) if p is not None else None, q, k, v, B, Lq, Lk, o, w, n, st)
    assert fwd(n=nbytes - 1) == E_WORKSPACE
    assert fwd(n=0) == E_WORKSPACE
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(o=None), dict(w=None), dict(p=None)):
        assert fwd(**kw) == E_ARG, kw
    for kw in (dict(Lk=0), dict(Lk=289), dict(Lq=0), dict(B=0), dict(B=-1)):
        assert fwd(**kw) == E_ARG, kw
    bad = _lib.CrossFormerParams(128, 0, 1, p.layer, None)
    assert fwd(p=bad) == E_ARG
    bad = _lib.CrossFormerParams(96, 2, 1, p.layer, None)
    assert fwd(p=bad) == E_ARG
    assert lib.keds_crossformer_seq_workspace_bytes(None, B, Lq, Lk) == 0
    assert lib.keds_crossformer_seq_workspace_bytes(C.byref(p), 0, Lq, Lk) == 0
    torch.cuda.synchronize()
    assert bool((bbuf == SENT).all()) and bool((fbuf == SENT).all())
    assert _around(wbuf, nbytes) and bool((ws == 0xA5).all()), "a refused call wrote to its workspace"
    # the single-query core keeps its own limit
    assert lib.keds_cross_attn_core(x, x, x, x, 1, 33, 1, 64, st) == E_ARG


# ---- composition, to the bit ----------------------------------------------------------------------------------------------------------
def _chain(lib, T, dim, heads, layers, q_bf, k_bf, v_bf, B, Lq, Lk, out):
    """keds_crossformer_forward_seq's chain from its public pieces; q_bf / k_bf / v_bf: device pointers of bf16 rows"""
    inner, Rq, Rk = 64 * heads, B * Lq, B * Lk
    Qp, Kp, Vp, att, qcur = (_pad_rows(r, c, BF) for r, c in ((Rq, inner), (Rk, inner), (Rk, inner), (Rq, inner), (Rq, dim)))
    qin = q_bf
    for l in range(layers):
        w = lambda n: T[f"{l}.{n}"].data_ptr()   # noqa: E731
        _gemm(lib, qin, w("wq"), w("bq"), P(Qp), Rq, inner, dim, _lib.EPI_BIAS_BF16)
        _gemm(lib, k_bf, w("wk"), w("bk"), P(Kp), Rk, inner, dim, _lib.EPI_BIAS_BF16)
        _gemm(lib, v_bf, w("wv"), w("bv"), P(Vp), Rk, inner, dim, _lib.EPI_BIAS_BF16)
        _done(lib.keds_cross_attn_seq(P(Qp), P(Kp), P(Vp), P(att), B, Lq, Lk, heads, inner, inner, inner, _lib.stream()), "keds_cross_attn_seq")
        if l == layers - 1:
            _gemm(lib, P(att), w("wo"), w("bo"), out, Rq, dim, inner, _lib.EPI_BIAS_F32)
        else:
            _gemm(lib, P(att), w("wo"), w("bo"), P(qcur), Rq, dim, inner, _lib.EPI_BIAS_BF16)
            qin = P(qcur)


@pytest.mark.parametrize("B,Lq,Lk", ((3, 1, 33), (2, 5, 77), (1, 17, 257)))
@pytest.mark.parametrize("dim,heads", ((128, 2), (768, 8)))
@pytest.mark.parametrize("layers", (1, 3))
def test_crossformer_forward_seq_equals_its_chain(layers, dim, heads, B, Lq, Lk):
    lib = _lib.load()
    _lib.ensure_gemm_workspace()
    p, T, keep = _xf(dim, heads, layers, seed=B * 100 + Lk)
    g = kc._gen(7, B, Lq, Lk, dim)
    q, k, v = (torch.randn(n, dim, generator=g).to(DEV) for n in (B * Lq, B * Lk, B * Lk))
    nbytes = lib.keds_crossformer_seq_workspace_bytes(C.byref(p), B, Lq, Lk)
    q_bf, k_bf, v_bf = _cast(lib, q, B * Lq, dim), _cast(lib, k, B * Lk, dim), _cast(lib, v, B * Lk, dim)
    want = {}
    for name, vb in (("v_is_k", k_bf), ("v_separate", v_bf)):
        want[name] = _pad_rows(B * Lq, dim, F32)[:B * Lq]
        _chain(lib, T, dim, heads, layers, P(q_bf), P(k_bf), P(vb), B, Lq, Lk, P(want[name]))
    torch.cuda.synchronize()
    assert not _same(want["v_is_k"], want["v_separate"])
    run = lambda vv: (lambda ws, n, out: _done(lib.keds_crossformer_forward_seq(C.byref(p), P(q), P(k), P(vv), B, Lq, Lk, out, ws, n, _lib.stream()),   # noqa: E731
                                               "keds_crossformer_forward_seq"))
    assert _same(_twice(run(k), nbytes, B * Lq, dim), want["v_is_k"]), "v is k"
    assert _same(_twice(run(v), nbytes, B * Lq, dim), want["v_separate"]), "v separate"
    assert lib.keds_crossformer_forward_seq(C.byref(p), P(q), P(k), P(k), B, Lq, Lk, P(want["v_is_k"]), P(q_bf), nbytes - 1, _lib.stream()) == E_WORKSPACE


# ---- the shared tile routine: cross-attention on a packed qkv buffer is self-attention, to the bit ----------------------------------
def test_cross_attn_seq_equals_self_attention_bit_for_bit():
    """keds_attention (full mask) on a packed bf16 qkv [B S, 3 x 64 H] against keds_cross_attn_seq with Q, Kp, Vp pointing at the three
    column ranges of the same buffer (q_ld = kv_ld = 3 x 64 H, o_ld = 64 H, Lq = Lk = S): both kernels instantiate one tile routine and
    one K / V^T staging (attn_tile.h), so every output bit is equal.  S over every tile count, both nfull values, a lone odd tile and
    the pair loop; S = 257 through the generic form (keds_attention_debug 16).  Before each comparison the two launch records name the
    generic / tile form with equal nkt and nfull.  Then q_limit rows of S = 273 against Lq = q_limit queries over Lk = 273 keys."""
    from tests import attention_check as ac
    lib = _lib.load()
    st = _lib.stream()
    GENERIC, TILE = _lib.ATTN_FORM_GENERIC, _lib.CROSS_SEQ_FORM_TILE
    H = 2
    d = 64 * H

    def both(qkv, B, S, q_limit, hook):
        """(self-attention rows [B S, d] over sentinels, cross rows [B q_limit, d]); q_limit < S only with B = 1"""
        out_s = torch.full((B * S, d), SENT, dtype=BF, device=DEV)
        out_c = torch.full((B * q_limit, d), SENT, dtype=BF, device=DEV)
        a, c = (C.c_int * 8)(), (C.c_int * 8)()
        try:
            assert lib.keds_attention_debug(hook) == 0
            if q_limit == S:
                _done(lib.keds_attention(P(qkv), P(out_s), B, S, H, 0, st), f"keds_attention S{S}")
            else:
                _done(lib.keds_attention_ex(P(qkv), P(out_s), B, S, H, 0, q_limit, st), f"keds_attention_ex S{S}.q{q_limit}")
            assert lib.keds_attention_last_launch(a) == 0
        finally:
            lib.keds_attention_debug(0)
        _done(lib.keds_cross_attn_seq(P(qkv), P(qkv) + 2 * d, P(qkv) + 4 * d, P(out_c), B, q_limit, S, H, 3 * d, 3 * d, d, st),
              f"keds_cross_attn_seq Lq{q_limit}.Lk{S}")
        assert lib.keds_cross_seq_last_launch(c) == 0
        a, c = list(a), list(c)
        assert a[0] == GENERIC and c[0] == TILE and a[1:3] == c[1:3], f"S{S}.q{q_limit}: attention launched {a}, cross {c}"
        return out_s, out_c

    msgs, launches = [], 0
    B = 2
    for S, hook in [(S, 0) for S in (1, 16, 17, 32, 33, 96, 97, 255, 256, 258, 272, 273, 288)] + [(257, 16)]:
        for regime in ("random", "ramp"):
            qkv = ac.make_qkv(B, S, H, regime, BF, seed=S, device=DEV)
            assert qkv.shape == (B * S, 3 * d) and qkv.dtype == BF
            out_s, out_c = both(qkv, B, S, S, hook)
            launches += 2
            if not torch.equal(out_s, out_c):
                bad = (out_s != out_c).any(1).nonzero().flatten().tolist()
                msgs.append(f"S{S}.{regime}: {len(bad)} rows differ, first {bad[:8]}")
    S = 273
    qkv = ac.make_qkv(1, S, H, "random", BF, seed=S, device=DEV)
    for q_limit in (1, 17, 257):
        out_s, out_c = both(qkv, 1, S, q_limit, 0)
        launches += 2
        if not torch.equal(out_s[:q_limit], out_c):
            msgs.append(f"S{S}.q_limit{q_limit}: stored rows differ")
        if not bool((out_s[q_limit:] == SENT).all()):
            msgs.append(f"S{S}.q_limit{q_limit}: self-attention wrote rows >= q_limit")
    assert launches == 2 * (14 * 2 + 3)
    assert not msgs, f"{len(msgs)} failures:\n" + "\n".join(msgs)
