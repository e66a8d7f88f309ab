"""Every training kernel of keds_amd/csrc/train.hip per ELEMENT at its edges (tests/train_check.py: the float64 references, the bounds,
the regimes; tests/test_host_train_check.py: proof that the checks pass float32 models of the kernels and catch their mutations):
the self-attention backward on both sides of its 64-lane softmax stride with and without the causal mask, the cross-attention core and
its backward from 1 to 32 keys, LayerNorm with statistics and its backward (strided rows, a row map, the bf16 plane), the contrastive
loss and its text gradient, the backward of the l2 normalisation, QuickGELU over every bf16 value in [-32, 32], the dropout ReLU pair
at its gates, AdamW, the dropout mask, the transpose, the column sums and the row gather / scatter.

Outputs sit in sentinel-filled buffers: 8 guard rows on both sides, guard columns where a stride exceeds the width, 256 elements around
flat arrays; everything outside the specified output must survive.  Every element of every launch is compared; the worst ratio to the
bound per kernel goes to the metrics log.  Only arguments the entry points accept are passed (S <= 80, K <= 32, row maps in range with
distinct entries, dim % 4 == 0 for the loss); the argument errors asserted are those KEDS_REQUIRE returns before any launch."""
import math

import numpy as np
import pytest
import torch

from keds_amd import _lib
from tests import train_check as tc
from tests.gpu_util import report

pytestmark = pytest.mark.gpu

GR, GAP = 8, 256
SENT = tc.SENT
BF, F32 = tc.BF, tc.F32
P = _lib.ptr
DEV = "cuda"


def _done(rc_, what):
    """a failed launch or a device fault: nothing more of this session may run on the card"""
    try:
        _lib.check(rc_, what)
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what}: {e}", returncode=3)


def _guarded(rows, cols, dtype, fill=SENT):
    """-> (buffer [rows + 2 GR, cols] filled with the sentinel, view of rows [GR, GR + rows))"""
    buf = torch.full((rows + 2 * GR, cols), fill, dtype=dtype, device=DEV)
    return buf, buf[GR:GR + rows]


def _flat(n, dtype, fill=SENT):
    buf = torch.full((n + 2 * GAP,), fill, dtype=dtype, device=DEV)
    return buf, buf[GAP:GAP + n]


def _untouched(buf, view, fill=SENT):
    """call AFTER the results were copied out: the written region is reset and the whole buffer must be the sentinel"""
    view.fill_(fill)
    return bool((buf == fill).all())


class Tally:
    """failures of a whole test and the worst ratio per key"""

    def __init__(self, label):
        self.label, self.msgs, self.worst, self.launches = label, [], {}, 0

    def add(self, key, fails, worst, guards_ok=True, what=""):
        self.launches += 1
        self.msgs += [str(f) for f in fails]
        if not guards_ok:
            self.msgs.append(f"{what}: written outside its output region (guard rows, guard columns or the elements around a flat array)")
        self.worst[key] = max(self.worst.get(key, 0.0), worst)

    def finish(self):
        for key, w in sorted(self.worst.items()):
            report(f"train_edges.{self.label}.{key}", worst_ratio=w)
        assert self.launches > 0
        assert not self.msgs, f"{len(self.msgs)} failures:\n" + "\n".join(self.msgs[:30])


def _one(f):
    return [f] if f else []


# ---- attention backward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", tc.ATT_S)
def test_attention_bwd(S):
    """dQ | dK | dV per element, causal and not, one workgroup and six, the four regimes of attention_check"""
    lib = _lib.load()
    t = Tally(f"attention_bwd.S{S}")
    for causal in (0, 1):
        for B, H in tc.ATT_BH:
            for regime in tc.ac.REGIMES:
                qkv, go = (x.to(DEV) for x in tc.att_inputs(B, S, H, regime, seed=S))
                buf, out = _guarded(B * S, 3 * 64 * H, BF)
                what = f"S{S}.B{B}.H{H}.causal{causal}.{regime}"
                _done(lib.keds_attention_bwd(P(qkv), P(go), out.data_ptr(), B, S, H, causal, _lib.stream()), "keds_attention_bwd " + what)
                fails, worst = tc.att_failures(tc.att_reference(qkv, go, B, S, H, causal), out.clone(), what)
                t.add(f"causal{causal}.{regime}", fails, worst, _untouched(buf, out), what)
    t.finish()


# ---- cross-attention core ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", tc.CROSS_K)
def test_cross_core_fwd_and_bwd(K):
    """B heads = 1, 9 and 40: a workgroup's four waves partly used, and ten workgroups"""
    lib = _lib.load()
    t = Tally(f"cross_core.K{K}")
    for B, H in tc.CROSS_BH:
        for regime in tc.ac.REGIMES:
            Q, Kp, Vp, go = (x.to(DEV) for x in tc.cross_inputs(B, K, H, regime, seed=K))
            R = tc.cross_reference(Q, Kp, Vp, go, B, K, H)
            d = 64 * H
            what = f"K{K}.B{B}.H{H}.{regime}"
            obuf, out = _guarded(B, d, BF)
            _done(lib.keds_cross_core_fwd(P(Q), P(Kp), P(Vp), out.data_ptr(), B, K, H, _lib.stream()), "keds_cross_core_fwd " + what)
            fails, worst = tc.cross_failures(R, {"out": out.clone()}, what)
            t.add(f"fwd.{regime}", fails, worst, _untouched(obuf, out), what + " fwd")
            bufs = {"dQ": _guarded(B, d, BF), "dK": _guarded(B * K, d, BF), "dV": _guarded(B * K, d, BF)}
            _done(lib.keds_cross_core_bwd(P(Q), P(Kp), P(Vp), P(go), bufs["dQ"][1].data_ptr(), bufs["dK"][1].data_ptr(), bufs["dV"][1].data_ptr(), B, K, H,
                                          _lib.stream()), "keds_cross_core_bwd " + what)
            fails, worst = tc.cross_failures(R, {n: v.clone() for n, (_, v) in bufs.items()}, what)
            t.add(f"bwd.{regime}", fails, worst, all(_untouched(b, v) for b, v in bufs.values()), what + " bwd")
    t.finish()


# ---- LayerNorm with statistics, and its backward -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", tc.LN_DIMS)
def test_layernorm_fwd_stats_and_bwd(dim):
    """rows over the four-rows-per-workgroup edge, ld = dim and dim + 4 (NaN / the sentinel behind dim), no map and a permuted map
    with gaps, the bf16 plane and NULL; the backward with the float64-exact statistics and with the forward launch's"""
    lib = _lib.load()
    t = Tally(f"layernorm_train.{dim}")
    for rows in tc.LN_ROWS:
        for regime in tc.LN_REGIMES:
            for ld in (dim, dim + 4):
                for mapped in (False, True):
                    for dyr in (tc.LN_DY if regime == "random" else ("random",)):
                        case = tc.LnBwdCase(rows, dim, ld, mapped, regime, dyr, seed=rows).to(DEV)
                        x = case.x.contiguous()
                        ybuf, y = _guarded(rows, dim, BF)
                        sbuf, st = _guarded(rows, 2, F32)
                        _done(lib.keds_ln_fwd_stats(P(x), ld, P(case.map), P(case.gamma), P(case.beta), y.data_ptr(), st.data_ptr(), rows, dim, _lib.stream()),
                              "keds_ln_fwd_stats " + case.name)
                        stats_fwd = st.clone()
                        fails, worst = tc.ln_fwd_failures(x[case.src, :dim], case.gamma, case.beta, y.clone(), stats_fwd, case.name)
                        t.add(f"fwd.{regime}", fails, worst, _untouched(ybuf, y) and _untouched(sbuf, st), case.name + " fwd")
                        if not torch.isfinite(stats_fwd).all():
                            continue                                  # (reported above; the backward below would only repeat it)
                        for which, stats in (("exact", case.stats_exact), ("fwd", stats_fwd)):
                            for with_bf in (True, False):
                                dbuf, dx = _guarded(case.n_src, ld, F32)
                                dx.copy_(case.dx0)
                                bbuf, dxb = _guarded(case.n_src, ld, BF)
                                stc = stats.contiguous()
                                _done(lib.keds_ln_bwd(P(case.dy), P(x), ld, P(case.map), P(stc), P(case.gamma), dx.data_ptr(), dxb.data_ptr() if with_bf else None,
                                                      rows, dim, _lib.stream()), "keds_ln_bwd " + case.name)
                                fails, worst = tc.ln_bwd_failures(case, stc, dx.clone(), dxb.clone() if with_bf else None, f"stats {which}. ")
                                ok = _untouched(dbuf, dx) and _untouched(bbuf, dxb)          # (without the plane nothing may be written to it)
                                t.add(f"bwd.{regime}.{dyr}", fails, worst, ok, case.name + " bwd")
    t.finish()


# ---- the loss ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", tc.LOSS_N)
def test_clip_loss(N):
    """loss and dtxt per element; rows behind B_local of dtxt are guard rows; N = 1: both are zero"""
    lib = _lib.load()
    t = Tally(f"clip_loss.N{N}")
    nbytes = int(lib.keds_clip_loss_workspace_bytes(N))
    for dim in tc.LOSS_DIMS:
        for regime in tc.LOSS_REGIMES:
            img, txt = (x.to(DEV) for x in tc.loss_inputs(N, dim, regime, seed=N))
            for scale in tc.LOSS_SCALES:
                full = tc.loss_reference(img, txt, N, scale)
                for B in sorted({1, math.ceil(N / 3), N}):
                    R = dict(full, dtxt=full["dtxt"][:B], e_dtxt=full["e_dtxt"][:B], m_dtxt=full["m_dtxt"][:B])
                    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=DEV)
                    lbuf, loss = _flat(1, F32)
                    dbuf, dt = _guarded(B, dim, F32)
                    what = f"N{N}.B{B}.d{dim}.{regime}.s{scale}"
                    _done(lib.keds_clip_loss(P(img), P(txt), N, B, dim, scale, loss.data_ptr(), dt.data_ptr(), P(ws), nbytes, _lib.stream()), "keds_clip_loss " + what)
                    fails, worst = tc.loss_failures(R, loss.clone(), dt.clone(), what)
                    t.add(f"{regime}.s{scale}", fails, worst, _untouched(lbuf, loss) and _untouched(dbuf, dt), what)
    t.finish()


@pytest.mark.parametrize("dim", tc.L2_DIMS)
def test_l2norm_bwd(dim):
    lib = _lib.load()
    t = Tally(f"l2norm_bwd.{dim}")
    for rows in tc.L2_ROWS:
        for regime in tc.L2_REGIMES:
            x, dy = (v.to(DEV) for v in tc.l2b_inputs(rows, dim, regime, seed=rows))
            buf, dx = _guarded(rows, dim, F32)
            _done(lib.keds_l2norm_bwd(P(x), P(dy), dx.data_ptr(), rows, dim, _lib.stream()), "keds_l2norm_bwd")
            fails, worst = tc.l2b_failures(x, dy, dx.clone(), f"{rows}x{dim}.{regime}")
            t.add(regime, fails, worst, _untouched(buf, dx), f"{rows}x{dim}.{regime}")
    t.finish()


# ---- element kernels -----------------------------------------------------------------------------------------------------------------
def test_qgelu_fwd_and_bwd():
    """every bf16 value in [-32, 32], +-100 and +-0; then n on both sides of the 256-thread workgroup"""
    lib = _lib.load()
    t = Tally("qgelu")
    vals = tc.qgelu_values()
    sets = [vals] + [vals[torch.randperm(vals.numel(), generator=torch.Generator().manual_seed(n))[:n]] for n in tc.FLAT_N]
    for u in sets:
        n = u.numel()
        u = u.to(DEV)
        dy = torch.randn(n, generator=torch.Generator().manual_seed(n)).bfloat16().to(DEV)
        ybuf, y = _flat(n, BF)
        dbuf, du = _flat(n, BF)
        _done(lib.keds_qgelu_fwd(P(u), y.data_ptr(), n, _lib.stream()), "keds_qgelu_fwd")
        _done(lib.keds_qgelu_bwd(P(dy), P(u), du.data_ptr(), n, _lib.stream()), "keds_qgelu_bwd")
        fails, worst = tc.qgelu_failures(u, y.clone(), None, None, f"n{n}")
        t.add("fwd", fails, worst, _untouched(ybuf, y), f"fwd n {n}")
        fails, worst = tc.qgelu_failures(u, None, dy, du.clone(), f"n{n}")
        t.add("bwd", fails, worst, _untouched(dbuf, du), f"bwd n {n}")
    t.finish()


@pytest.mark.parametrize("n", tc.FLAT_N + (1000,))
def test_dropout_relu_fwd_and_bwd(n):
    """to the bit (zeros by value): mask and no mask, dy fp32 and bf16, the gates at +-0, +-2^-126 and the smallest bf16 subnormal"""
    lib = _lib.load()
    t = Tally(f"dropout_relu.n{n}")
    z, mask, dy = (v.to(DEV) for v in tc.dropout_inputs(n, seed=n))
    scale = float(np.float32(1.0 / 0.7))
    for mk in (mask, None):
        buf, y = _flat(n, BF)
        _done(lib.keds_dropout_relu_fwd(P(z), P(mk), scale, y.data_ptr(), n, _lib.stream()), "keds_dropout_relu_fwd")
        f = tc.same_value(y.clone(), tc.dropout_fwd_ref(z, mk, scale), f"fwd n{n} mask {mk is not None}")
        t.add("fwd", _one(f), f.worst, _untouched(buf, y), f"fwd n {n}")
        for g in (dy, dy.bfloat16()):
            buf, dz = _flat(n, BF)
            _done(lib.keds_dropout_relu_bwd(P(g), int(g.dtype == F32), P(z), P(mk), scale, dz.data_ptr(), n, _lib.stream()), "keds_dropout_relu_bwd")
            f = tc.same_value(dz.clone(), tc.dropout_bwd_ref(g, z, mk, scale), f"bwd n{n} mask {mk is not None} dy {g.dtype}")
            t.add("bwd", _one(f), f.worst, _untouched(buf, dz), f"bwd n {n}")
    t.finish()


@pytest.mark.parametrize("step", (1, 2, 1000))
def test_adamw(step):
    """one step from given (p, g, m, v): p, m, v per element; v = g = 0; grad_scale 1 and 0.5"""
    lib = _lib.load()
    t = Tally(f"adamw.step{step}")
    hp = tc.ADAMW_HP
    for n in tc.FLAT_N:
        for regime in ("random", "zero_vg"):
            for gs in (1.0, 0.5):
                p0, g, m0, v0 = tc.adamw_inputs(n, regime, seed=step)
                R = tc.adamw_reference(p0.to(DEV), g.to(DEV), m0.to(DEV), v0.to(DEV), step, gs)
                bufs = [_flat(n, F32) for _ in range(3)]
                for (_, view), src in zip(bufs, (p0, m0, v0)):
                    view.copy_(src)
                gd = g.to(DEV)
                _done(lib.keds_adamw_step(bufs[0][1].data_ptr(), P(gd), bufs[1][1].data_ptr(), bufs[2][1].data_ptr(), n, hp["lr"], hp["b1"], hp["b2"], hp["eps"],
                                          hp["wd"], step, gs, _lib.stream()), "keds_adamw_step")
                fails, worst = tc.adamw_failures(R, *(v.clone() for _, v in bufs), f"n{n}.{regime}.gs{gs}")
                t.add(regime, fails, worst, all(_untouched(b, v) for b, v in bufs), f"n {n} {regime}")
    t.finish()


def test_dropout_mask():
    """against the uint64 model of the counter hash, to the byte; two launches agree; the keep rate within 5 binomial standard deviations"""
    lib = _lib.load()
    t = Tally("dropout_mask")
    for n in tc.FLAT_N + (2 ** 20 + 1,):
        for p in (0.0, 0.1, 0.5, 0.999):
            runs = []
            for _ in range(2):
                buf, mk = _flat(n, torch.uint8, fill=77)
                _done(lib.keds_dropout_mask(mk.data_ptr(), n, 1234 + n, p, _lib.stream()), "keds_dropout_mask")
                runs.append(mk.clone())
                ok = _untouched(buf, mk, 77)
            f = tc.same_bits(runs[0].cpu(), tc.dropout_mask_ref(n, 1234 + n, p), f"n{n}.p{p}")
            fails = _one(f) + ([] if torch.equal(runs[0], runs[1]) else [f"n{n}.p{p}: two launches differ"])
            rate = tc.keep_rate_ratio(runs[0], float(np.float32(p))) if n > 2 ** 20 else 0.0
            if rate > 1.0:
                fails.append(f"n{n}.p{p}: the keep rate is {rate:.3g} x 5 standard deviations off")
            t.add("bits", fails, rate, ok, f"n {n} p {p}")
    t.finish()


# ---- transpose, column sums, gather / scatter --------------------------------------------------------------------------------------------
def _ld_outs(rows):
    return sorted({rows, rows + 1, -(-rows // 64) * 64})


@pytest.mark.parametrize("src_dtype", (F32, BF), ids=("fp32", "bf16"))
def test_transpose_to_bf16(src_dtype):
    """to the bit against src.t().bfloat16() with the special values of a cast among the data; pad rows [rows, ld_out) are +0; the
    source's guard columns (NaN) are not read"""
    lib = _lib.load()
    t = Tally(f"transpose.{'fp32' if src_dtype == F32 else 'bf16'}")
    for rows in tc.T_ROWS:
        for cols in tc.T_COLS:
            x = tc.matrix_data(rows, cols, "specials", src_dtype, seed=rows).to(DEV)
            for ld_src in (cols, cols + 3):
                xs = tc.strided(x, ld_src)
                for ld_out in _ld_outs(rows):
                    buf, out = _guarded(cols, ld_out, BF)
                    what = f"{rows}x{cols}.ld_src{ld_src}.ld_out{ld_out}"
                    _done(lib.keds_transpose_to_bf16(P(xs), int(src_dtype == F32), ld_src, rows, cols, out.data_ptr(), ld_out, _lib.stream()), "keds_transpose_to_bf16 " + what)
                    f = tc.same_bits(out.clone(), tc.transpose_ref(x, ld_out), what)
                    t.add("bits", _one(f), f.worst, _untouched(buf, out), what)
    t.finish()


@pytest.mark.parametrize("src_dtype", (F32, BF), ids=("fp32", "bf16"))
def test_colsum(src_dtype):
    """against float64, exact in `integer`, the same bits over two launches, `accumulate` adds once to what the output held"""
    lib = _lib.load()
    t = Tally(f"colsum.{'fp32' if src_dtype == F32 else 'bf16'}")
    for rows in tc.T_ROWS:
        for cols in tc.T_COLS:
            for regime in ("integer", "random"):
                x = tc.matrix_data(rows, cols, regime, src_dtype, seed=rows).to(DEV)
                prev = (torch.randint(-4, 5, (cols,), generator=torch.Generator().manual_seed(cols)).float() + 16.0).to(DEV)
                for ld in (cols, cols + 3):
                    xs = tc.strided(x, ld)
                    for acc in (0, 1):
                        runs = []
                        for _ in range(2):
                            buf, out = _flat(cols, F32)
                            if acc:
                                out.copy_(prev)
                            _done(lib.keds_colsum(P(xs), int(src_dtype == F32), ld, rows, cols, out.data_ptr(), acc, _lib.stream()), "keds_colsum")
                            runs.append(out.clone())
                            ok = _untouched(buf, out)
                        what = f"{rows}x{cols}.{regime}.ld{ld}.acc{acc}"
                        fails, worst = tc.colsum_failures(x, prev if acc else None, runs[0], regime == "integer", what)
                        fails = fails + _one(tc.same_bits(runs[1], runs[0], what + " two launches"))
                        t.add(f"{regime}.acc{acc}", fails, worst, ok, what)
    t.finish()


def test_rows_gather_and_scatter():
    """to the bit; stride = dim and dim + 8; maps touch row 0 and the last row; scatter plain and accumulating (one fp32 addition);
    rows the map does not name and the columns behind dim keep the sentinel / their values"""
    lib = _lib.load()
    t = Tally("rows_gather_scatter")
    for rows in tc.G_ROWS:
        for dim in tc.G_DIMS:
            for stride in (dim, dim + 8):
                n_src = 2 * rows + 1
                g = torch.Generator().manual_seed(rows * 1000 + dim)
                m = tc.gather_map(rows, n_src, seed=dim).to(DEV)
                src = tc.strided(torch.randn(n_src, dim, generator=g).to(DEV), stride)
                what = f"{rows}x{dim}.stride{stride}"
                buf, out = _guarded(rows, dim, F32)
                _done(lib.keds_rows_gather(P(src), stride, P(m), out.data_ptr(), rows, dim, _lib.stream()), "keds_rows_gather " + what)
                f = tc.same_bits(out.clone(), src[m.long(), :dim], what + " gather")
                t.add("gather", _one(f), f.worst, _untouched(buf, out), what + " gather")
                dense = torch.randn(rows, dim, generator=g).to(DEV)
                for acc in (0, 1):
                    dst0 = torch.full((n_src, stride), SENT, device=DEV)
                    dst0[:, :dim] = torch.randn(n_src, dim, generator=g).to(DEV)
                    buf, dst = _guarded(n_src, stride, F32)
                    dst.copy_(dst0)
                    _done(lib.keds_rows_scatter(P(dense), P(m), dst.data_ptr(), stride, rows, dim, acc, _lib.stream()), "keds_rows_scatter " + what)
                    f = tc.same_bits(dst.clone(), tc.scatter_ref(dense, m, dst0, dim, acc), what + f" scatter acc{acc}")
                    t.add(f"scatter.acc{acc}", _one(f), f.worst, _untouched(buf, dst), what + " scatter")
    t.finish()


# ---- argument errors -------------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_before_any_launch():
    """S = 81, K = 33, N = 8193, a loss dim of 6, B_local > N, ld_out < rows: -1, and every output keeps the sentinel"""
    lib = _lib.load()
    bufs = []

    def out(n, dtype=BF):
        b = torch.full((n,), SENT, dtype=dtype, device=DEV)
        bufs.append(b)
        return b
    st = _lib.stream()
    qkv, go = torch.zeros(81, 192, dtype=BF, device=DEV), torch.zeros(81, 64, dtype=BF, device=DEV)
    assert lib.keds_attention_bwd(P(qkv), P(go), P(out(81 * 192)), 1, 81, 1, 1, st) == -1
    Q, KV = torch.zeros(1, 64, dtype=BF, device=DEV), torch.zeros(33, 64, dtype=BF, device=DEV)
    assert lib.keds_cross_core_fwd(P(Q), P(KV), P(KV), P(out(64)), 1, 33, 1, st) == -1
    assert lib.keds_cross_core_bwd(P(Q), P(KV), P(KV), P(Q), P(out(64)), P(out(33 * 64)), P(out(33 * 64)), 1, 33, 1, st) == -1
    big = torch.zeros(8193, 8, device=DEV)
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    assert lib.keds_clip_loss(P(big), P(big), 8193, 1, 4, 14.3, P(out(1, F32)), P(out(8, F32)), P(ws), ws.numel(), st) == -1
    small = torch.zeros(8, 8, device=DEV)
    ws8 = torch.zeros(int(lib.keds_clip_loss_workspace_bytes(8)), dtype=torch.uint8, device=DEV)
    assert lib.keds_clip_loss(P(small), P(small), 8, 4, 6, 14.3, P(out(1, F32)), P(out(64, F32)), P(ws8), ws8.numel(), st) == -1
    assert lib.keds_clip_loss(P(small), P(small), 8, 9, 8, 14.3, P(out(1, F32)), P(out(128, F32)), P(ws8), ws8.numel(), st) == -1
    assert lib.keds_transpose_to_bf16(P(small), 1, 8, 8, 8, P(out(64)), 7, st) == -1
    torch.cuda.synchronize()
    assert all(bool((b == SENT).all()) for b in bufs)
