"""Every row kernel of keds_amd/csrc/elementwise.hip per ELEMENT at its edges (tests/row_check.py: the float64 references, the bounds,
the regimes; tests/test_host_row_check.py: proof that the checks pass float32 models of the kernels and catch their mutations):
LayerNorm in every form (dense, strided, gathered, CLS rows; bf16 / fp32 / fp16 / fp16-pair output; NV = 1 - 4 and the generic
instantiation; the stream form a wave walks several rows in), row statistics, the LayerNorm fold, cast_rows, the token-row gather,
cast16 through its grid-stride loop, im2col, cls_rows, embed_tokens with the cut at Lx and packed rows, l2 / mixture normalisation, and
the read-out as the composition of its three kernels.

Outputs and planes sit in sentinel-filled buffers: 8 guard rows on both sides, 256 elements between and behind the planes of a pair,
guard columns where a stride exceeds dim (NaN in the SOURCE's guard columns); everything outside the written region must survive.
Every element of every launch is compared; the worst ratio to the bound per kernel and output type goes to the metrics log."""

import pytest
import torch

from keds_amd import _lib
from tests import gemm_check as gc
from tests import row_check as rc
from tests.gpu_util import report

pytestmark = pytest.mark.gpu

GR, GAP = 8, 256                               # guard rows on both sides; elements between and behind planes
SENT = rc.SENT
BF, HF, F32 = rc.BF, rc.HF, rc.F32
P = _lib.ptr
DEV = "cuda"


def _done(rc_, what):
    """a failed launch or a device fault: nothing more of this session may run on the card"""
    try:
        _lib.check(rc_, what)
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what}: {e}", returncode=3)


def _guarded(rows, cols, dtype, ld=None, fill=SENT):
    """-> (buffer [rows + 2 GR, ld] filled with the sentinel, view of rows [GR, GR + rows))"""
    buf = torch.full((rows + 2 * GR, ld or cols), fill, dtype=dtype, device=DEV)
    return buf, buf[GR:GR + rows]


def _untouched(buf, view, fill=SENT):
    """call AFTER the results were copied out: the written region is reset and the whole buffer must be the sentinel"""
    view.fill_(fill)
    return bool((buf == fill).all())


def _strided(x, stride):
    """x [rows, dim] with row stride `stride`, NaN in the guard columns"""
    if stride == x.shape[1]:
        return x.contiguous()
    s = torch.full((x.shape[0], stride), float("nan"), dtype=x.dtype, device=x.device)
    s[:, :x.shape[1]] = x
    return s


class Tally:
    """failures of a whole test and the worst ratio per key"""

    def __init__(self, label):
        self.label, self.msgs, self.worst, self.launches = label, [], {}, 0

    def add(self, key, fails, worst, guards_ok=True, what=""):
        self.launches += 1
        self.msgs += [str(f) for f in fails]
        if not guards_ok:
            self.msgs.append(f"{what}: written outside its output region (guard rows, guard columns or the gap behind a plane)")
        self.worst[key] = max(self.worst.get(key, 0.0), worst)

    def finish(self):
        for key, w in sorted(self.worst.items()):
            report(f"row_edges.{self.label}.{key}", worst_ratio=w)
        assert self.launches > 0
        assert not self.msgs, f"{len(self.msgs)} failures:\n" + "\n".join(self.msgs[:30])


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------
OUTS = (BF, F32, HF, "pair")


def _out_name(out):
    return out if out == "pair" else rc.TYPE_NAME[out]


def _run_ln(x_buf, x_stride, row_map, row_mul, case, out, rows, form=0):
    """one LayerNorm launch of `rows` output rows -> (res of row_check.ln_failures, guards intact, recorded pair form or None)"""
    lib = _lib.load()
    dim = case.dim
    if out == "pair":
        plane = rows * dim + GAP
        buf = torch.full((2 * GR * dim + 2 * plane,), SENT, dtype=HF, device=DEV)
        o = buf[GR * dim:]
        _done(lib.keds_layernorm_pair(P(x_buf), x_stride, P(case.gamma), P(case.beta), o.data_ptr(), plane, rows, dim, form, _lib.stream()),
              f"keds_layernorm_pair {case.name}")
        rec = lib.keds_layernorm_pair_last_form()
        views = [o[i * plane:i * plane + rows * dim].view(rows, dim) for i in (0, 1)]
        res = {"hi": views[0].clone(), "lo": views[1].clone()}
        for v in views:
            v.fill_(SENT)
        return res, bool((buf == SENT).all()), rec
    buf, view = _guarded(rows, dim, out)
    _done(lib.keds_layernorm_rows(P(x_buf), x_stride, P(row_map), row_mul, P(case.gamma), P(case.beta), view.data_ptr(), rc.OUT_CODE[out], rows, dim,
                                  _lib.stream()), f"keds_layernorm_rows {case.name}")
    res = {"out": view.clone()}
    return res, _untouched(buf, view), None


@pytest.mark.parametrize("dim", rc.LN_DIMS)
def test_layernorm_dense_and_strided(dim):
    """rows over the four-rows-per-workgroup edge, every regime, every output type, x_stride = dim and dim + 4"""
    t = Tally(f"layernorm.{dim}")
    for rows in (1, 3, 4, 5, 9):
        for regime in rc.LN_REGIMES:
            case = rc.LnCase(rows, dim, regime, seed=dim, device=DEV)
            for stride in (dim, dim + 4):
                xs = _strided(case.x, stride)
                for out in OUTS:
                    res, ok, rec = _run_ln(xs, stride, None, 1, case, out, rows)
                    fails, worst = rc.ln_failures(case, res, HF if out == "pair" else out, what=f"stride{stride}.")
                    if out == "pair" and rec != 0:
                        fails = fails + [f"{case.name}: recorded pair form {rec}, wanted the one-row form"]
                    t.add(f"{_out_name(out)}.{regime}", fails, worst, ok, f"{case.name} {_out_name(out)} stride {stride}")
    t.finish()


@pytest.mark.parametrize("dim", rc.LN_DIMS)
def test_layernorm_gathered(dim):
    """row_map / row_mul (the text read-out): a map that hits 0, row_mul - 1, row_mul and -1 -- rows outside [0, row_mul) are NaN in
    every element, no other row changes -- over a source whose groups of row_mul rows alternate in scale by 2^6; the CLS form
    (row_map = NULL, row_mul = S)"""
    t = Tally(f"layernorm_gathered.{dim}")
    rows = 9
    for row_mul in (1, 77):
        case = rc.LnCase(rows * row_mul, dim, "rowscale", seed=dim + 1, group=row_mul, device=DEV)
        row_map = torch.tensor([0, row_mul - 1, row_mul, -1, row_mul // 2, 0, row_mul - 1, 3 * row_mul, (row_mul + 1) // 3], dtype=torch.int32, device=DEV)
        src, bad = rc.gather_sources(rows, row_map, row_mul)
        assert int(bad.sum()) == 3
        for stride in (dim, dim + 4):
            xs = _strided(case.x, stride)
            for out in (BF, F32, HF):
                res, ok, _ = _run_ln(xs, stride, row_map, row_mul, case, out, rows)
                fails, worst = rc.ln_failures(case, res, out, src, bad, what=f"mul{row_mul}.stride{stride}.")
                t.add(f"{_out_name(out)}.map", fails, worst, ok, f"{case.name} mul {row_mul}")
    S = 5
    case = rc.LnCase(rows * S, dim, "rowscale", seed=dim + 2, group=1, device=DEV)
    src, bad = rc.gather_sources(rows, None, S)
    src = src.to(DEV)
    for out in (BF, F32, HF):
        res, ok, _ = _run_ln(case.x, dim, None, S, case, out, rows)
        fails, worst = rc.ln_failures(case, res, out, src, None, what="cls.")
        t.add(f"{_out_name(out)}.cls", fails, worst, ok, f"{case.name} cls")
    t.finish()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


STREAM_ROWS = ("2047", "2048", "2049", "nw-1", "nw+1", "2nw+7")


def _stream_rows(which):
    nw = 20 * _cus()
    return {"2047": 2047, "2048": 2048, "2049": 2049, "nw-1": nw - 1, "nw+1": nw + 1, "2nw+7": 2 * nw + 7}[which]


@pytest.mark.parametrize("dim", (512, 1024))
@pytest.mark.parametrize("which", STREAM_ROWS)
def test_layernorm_pair_stream_form(which, dim):
    """The stream form (rows >= 2048, dim 512 / 1024: 20 waves per CU walk rows r, r + nw, ... with the next row's loads in flight) at
    its row-count edges -- 2047 must record the one-row form, nw + 1 has one wave walk two rows, 2 nw + 7 three -- with rows x 2^6 on
    every other group of nw (a stale or a neighbour's row is gross).  The same inputs through form = 1: both hold the bound and differ by
    at most the sum of the two bounds (another summation order, so not to the bit)."""
    rows = _stream_rows(which)
    nw = 20 * _cus()
    assert nw > 2049, "the row counts of this test assume more than 2,049 resident waves"
    want = 0 if rows < 2048 else 1
    t = Tally(f"layernorm_stream.{dim}")
    for regime in ("rowscale", "offset1k", "constant_exact", "tiny"):
        case = rc.LnCase(rows, dim, regime, seed=rows, group=nw, device=DEV)
        ref, e = case.ref()
        both = 2 * gc.Expected(ref, e, HF, False, pair=True).bound
        for stride in (dim, dim + 4):
            xs = _strided(case.x, stride)
            sums = []
            for form in (0, 1):
                res, ok, rec = _run_ln(xs, stride, None, 1, case, "pair", rows, form=form)
                fails, worst = rc.ln_failures(case, res, HF, what=f"form{form}.stride{stride}.")
                if rec != (want if form == 0 else 0):
                    fails = fails + [f"{case.name} form {form}: recorded form {rec}"]
                t.add(f"pair.form{rec}.{regime}", fails, worst, ok, f"{case.name} form {form} stride {stride}")
                sums.append(res["hi"].double() + res["lo"].double())
            f = gc._collect((sums[0] - sums[1]).abs() / both, f"{case.name}: the two forms differ by more than the sum of their bounds")
            t.add(f"pair.forms_differ.{regime}", [f] if f else [], f.worst)
    t.finish()


def test_layernorm_pair_form_choice():
    """dim = 768 and a plane with plane % 8 == 4 must take the one-row form at 2,048 rows"""
    lib = _lib.load()
    t = Tally("layernorm_pair_choice")
    for dim, extra in ((768, 256), (1024, 260), (512, 260)):
        rows = 2048
        case = rc.LnCase(rows, dim, "random", seed=dim, device=DEV)
        plane = rows * dim + extra
        buf = torch.full((2 * plane,), SENT, dtype=HF, device=DEV)
        _done(lib.keds_layernorm_pair(P(case.x), dim, P(case.gamma), P(case.beta), P(buf), plane, rows, dim, 0, _lib.stream()), "keds_layernorm_pair")
        assert lib.keds_layernorm_pair_last_form() == 0, (dim, extra)
        views = [buf[i * plane:i * plane + rows * dim].view(rows, dim) for i in (0, 1)]
        res = {"hi": views[0].clone(), "lo": views[1].clone()}
        for v in views:
            v.fill_(SENT)
        fails, worst = rc.ln_failures(case, res, HF)
        t.add(f"pair.{dim}", fails, worst, bool((buf == SENT).all()), f"{dim} plane + {extra}")
    x = torch.zeros(8, 512, device=DEV)
    o = torch.zeros(2 * 8 * 512, dtype=HF, device=DEV)
    g = torch.ones(512, device=DEV)
    assert lib.keds_layernorm_pair(P(x), 512, P(g), P(g), P(o), 8 * 512 + 2, 8, 512, 0, _lib.stream()) == -1      # plane % 4
    assert lib.keds_layernorm_pair(P(x), 512, P(g), P(g), P(o), 8 * 512 - 4, 8, 512, 0, _lib.stream()) == -1     # plane < rows dim
    assert lib.keds_layernorm_pair(P(x), 510, P(g), P(g), P(o), 8 * 512, 8, 512, 0, _lib.stream()) == -1         # x_stride % 4
    assert lib.keds_layernorm_pair(P(x), 512, P(g), P(g), P(o), 8 * 512, 8, 640, 0, _lib.stream()) == -1         # dim
    assert lib.keds_layernorm_rows(P(x), 512, None, 1, P(g), P(g), P(o), 3, 8, 512, _lib.stream()) == -1         # out_type
    t.finish()


# ---- row statistics --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (BF, HF), ids=("bf16", "fp16"))
def test_rowstats_cast(dtype):
    """the 16-bit copy to the bit, {sum x, sum x^2} against float64 (exact in `integer`), the same bits over two launches"""
    lib = _lib.load()
    t = Tally(f"rowstats.{rc.TYPE_NAME[dtype]}")
    for rows in (1, 4, 5):
        for dim in (4, 252, 256, 260, 1024, 2044, 2048):
            for regime in ("random", "integer"):
                x = rc.stats_data(rows, dim, regime, seed=rows, device=DEV)
                runs = []
                for _ in range(2):
                    cbuf, copy = _guarded(rows, dim, dtype)
                    sbuf, st = _guarded(rows, 2, torch.int64, fill=-777)
                    _done(lib.keds_rowstats_cast_ex(P(x), copy.data_ptr(), int(dtype == HF), st.data_ptr(), rows, dim, _lib.stream()), "keds_rowstats_cast_ex")
                    runs.append((copy.clone(), st.clone()))
                    ok = _untouched(cbuf, copy) and _untouched(sbuf, st, -777)
                fails, worst = rc.stats_failures(x, runs[0][0], runs[0][1], dtype, regime == "integer", f"{rows}x{dim}.{regime}")
                if not torch.equal(runs[0][1], runs[1][1]):
                    fails = fails + [f"{rows}x{dim}.{regime}: the statistics of two launches differ"]
                t.add(regime, fails, worst, ok, f"{rows}x{dim}")
    t.finish()


# ---- LayerNorm fold --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (BF, HF), ids=("bf16", "fp16"))
def test_fold_layernorm(dtype):
    """W' = T(W gamma) per element (rounded once or twice: both counted), the column sums of the STORED W', b + W beta; with and
    without a bias; `integer` to the bit"""
    lib = _lib.load()
    t = Tally(f"fold.{rc.TYPE_NAME[dtype]}")
    twice = once = differ = 0
    for N in (1, 3, 4, 5):
        for K in (1, 63, 64, 65, 640, 1000):
            for regime in ("random", "integer"):
                case = rc.FoldCase(N, K, regime, seed=N, device=DEV)
                for with_bias in (True, False):
                    wbuf = torch.full((N * K + 2 * GAP,), SENT, dtype=dtype, device=DEV)
                    wf = wbuf[GAP:GAP + N * K].view(N, K)
                    bbuf = torch.full((2 * N + 2 * GAP,), SENT, dtype=F32, device=DEV)
                    bc = bbuf[GAP:GAP + 2 * N]
                    _done(lib.keds_fold_layernorm_ex(P(case.W), P(case.bias) if with_bias else None, P(case.gamma), P(case.beta), N, K, wf.data_ptr(),
                                                     int(dtype == HF), bc.data_ptr(), _lib.stream()), "keds_fold_layernorm_ex")
                    fails, worst, cnt = rc.fold_failures(case, wf.clone(), bc.clone(), dtype, with_bias)
                    twice, once, differ = twice + cnt[0], once + cnt[1], differ + cnt[2]
                    ok = _untouched(wbuf, wf) and _untouched(bbuf, bc)
                    t.add(regime, fails, worst, ok, case.name)
    report(f"row_edges.fold.{rc.TYPE_NAME[dtype]}.roundings", rounded_twice=twice, rounded_once=once, where_they_differ=differ)
    t.finish()


# ---- bit-for-bit kernels ---------------------------------------------------------------------------------------------------------
def _wide(n, seed, dtype=F32):
    """random magnitudes over many binades with the special values of the type scattered in"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    top = 10 if dtype == HF else 24
    x = torch.randn(n, generator=g, device=DEV) * torch.exp2(torch.randint(-top, top, (n,), generator=g, device=DEV).float())
    x = x.to(dtype)
    sp = rc.cast_specials(dtype).to(DEV)
    k = min(n, len(sp))
    x[torch.randperm(n, generator=g, device=DEV)[:k]] = sp[torch.randperm(len(sp), generator=g, device=DEV)[:k]]
    return x


@pytest.mark.parametrize("nt", (0, 1))
def test_cast_rows(nt):
    """all six type pairs, plain and non-temporal stores, stride = dim and dim + 8 (guard columns neither read nor written)"""
    lib = _lib.load()
    t = Tally(f"cast_rows.nt{nt}")
    for st in (F32, HF):
        for dt in (F32, HF, BF):
            for rows in (1, 33):
                for dim in (8, 64, 1000):
                    for stride in (dim, dim + 8):
                        x = _wide(rows * dim, rows + dim, st).view(rows, dim)
                        xs = _strided(x, stride)
                        buf, view = _guarded(rows, stride, dt, ld=stride)
                        _done(lib.keds_cast_rows(P(xs), rc.OUT_CODE[st], view.data_ptr(), rc.OUT_CODE[dt], rows, dim, stride, nt, _lib.stream()), "keds_cast_rows")
                        f = rc.bits_failures(view[:, :dim].clone(), rc.cast_ref(x, dt), f"{rc.TYPE_NAME[st]}->{rc.TYPE_NAME[dt]} {rows}x{dim} stride {stride}")
                        view[:, :dim] = SENT
                        t.add(f"{rc.TYPE_NAME[st]}_{rc.TYPE_NAME[dt]}", [f] if f else [], f.worst, bool((buf == SENT).all()), f"{rows}x{dim} stride {stride}")
    t.finish()


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_gather_token_rows(mode):
    """dst[b] = src[b S + row[b]] (global rows: src[row[b]]); rows 0, S - 1, S and -1 present: a row outside its sequence is NaN"""
    lib = _lib.load()
    S = 7
    t = Tally(f"gather_token_rows.mode{mode}")
    sd, dd = ((HF, HF), (HF, F32), (F32, F32))[mode]
    for glob in (0, 1):
        for B in (1, 3, 33):
            row_sets = [[0], [6], [7], [-1]] if B == 1 else [[0, 6, 7], [-1, 3, 6]] if B == 3 else [[0, 6, 7, -1] + [(5 * i) % 9 - 1 for i in range(29)]]
            for dim in (8, 128, 768):
                n_src = S if glob else B * S
                src = _wide(n_src * dim, B + dim, sd).view(n_src, dim)
                for rows in row_sets:
                    row = torch.tensor(rows, dtype=torch.int32, device=DEV)
                    buf, view = _guarded(B, dim, dd)
                    _done(lib.keds_gather_token_rows(P(src), view.data_ptr(), P(row), S, B, dim, mode, glob, _lib.stream()), "keds_gather_token_rows")
                    bad = (row < 0) | (row >= S)
                    idx = torch.where(bad, torch.zeros_like(row), row).long() + (0 if glob else torch.arange(B, device=DEV) * S)
                    want = src[idx].to(dd)
                    want[bad] = float("nan")
                    f = rc.bits_failures(view.clone(), want, f"mode {mode} global {glob} B {B} dim {dim} rows {rows[:4]}")
                    t.add(f"global{glob}", [f] if f else [], f.worst, _untouched(buf, view), f"B {B} dim {dim}")
    t.finish()


CAST16_COUNTS = (1, 2, 3, 4, 5, 1023, 3 * 1024 + 1, 3 * 1024 + 2, 3 * 1024 + 3, 2 * 4096 * 1024 + 3)


@pytest.mark.parametrize("dtype", (BF, HF), ids=("bf16", "fp16"))
def test_cast16_tail_and_grid_stride_loop(dtype):
    """counts whose tail is taken by the first thread, by a thread that came round the loop (3 x 1024 + r) and behind three trips of a
    capped grid (2 x 4096 x 1024 + 3); the sentinel behind `count` survives"""
    lib = _lib.load()
    fn = lib.keds_cast_bf16 if dtype == BF else lib.keds_cast_f16
    t = Tally(f"cast16.{rc.TYPE_NAME[dtype]}")
    for count in CAST16_COUNTS:
        x = _wide(count + GAP, count % 1000)
        out = torch.full((count + GAP,), SENT, dtype=dtype, device=DEV)
        _done(fn(P(x), P(out), count, _lib.stream()), "keds_cast16")
        f = rc.bits_failures(out[:count], rc.cast_ref(x[:count], dtype), f"count {count}")
        t.add("bits", [f] if f else [], f.worst, bool((out[count:] == SENT).all()), f"count {count}")
    t.finish()


@pytest.mark.parametrize("R,Pp,Kpad", [(28, 14, 640), (56, 14, 640), (32, 16, 768), (224, 14, 640)])
def test_im2col(R, Pp, Kpad):
    """rows (b, py, px), columns c P P + ky P + kx, zero pad columns (none at 32 / 16 / 768), rows >= B g^2 untouched; both types"""
    lib = _lib.load()
    t = Tally(f"im2col.{R}.{Pp}")
    g = R // Pp
    for B in (1, 3):
        img = _wide(B * 3 * R * R, R + B).view(B, 3, R, R)
        img = torch.where(torch.isfinite(img), img, torch.ones_like(img))
        for dtype in (BF, HF):
            buf, view = _guarded(B * g * g, Kpad, dtype)
            _done(lib.keds_im2col_ex(P(img), view.data_ptr(), int(dtype == HF), B, R, Pp, Kpad, _lib.stream()), "keds_im2col_ex")
            f = rc.bits_failures(view.clone(), rc.im2col_ref(img, Pp, Kpad, dtype), f"B {B} {rc.TYPE_NAME[dtype]}")
            t.add(rc.TYPE_NAME[dtype], [f] if f else [], f.worst, _untouched(buf, view), f"B {B}")
    t.finish()


def test_cls_rows():
    """x[b S] = cls + pos[0]; every other row is untouched"""
    lib = _lib.load()
    t = Tally("cls_rows")
    for B in (1, 3):
        for S in (1, 5):
            for d in (4, 128, 1028):
                g = torch.Generator(device=DEV).manual_seed(B * 100 + S * 10 + d)
                cls, pos = torch.randn(d, generator=g, device=DEV), torch.randn(S, d, generator=g, device=DEV)
                buf, view = _guarded(B * S, d, F32)
                _done(lib.keds_cls_rows(view.data_ptr(), P(cls), P(pos), B, S, d, _lib.stream()), "keds_cls_rows")
                want = torch.full((B * S, d), SENT, device=DEV)
                want[::S] = cls + pos[0]
                f = rc.bits_failures(view.clone(), want, f"B {B} S {S} d {d}")
                t.add("bits", [f] if f else [], f.worst, _untouched(buf, view), f"B {B} S {S} d {d}")
    t.finish()


@pytest.mark.parametrize("d", (4, 128, 1028))
def test_embed_tokens_cut_and_packed_rows(d):
    """token ids 0 and vocab - 1; Lx = L, 9, 1; splices at column 0, ending at L, of one token, straddling Lx, and none; dense rows and
    packed rows with lengths 0, 1, Lx and 5 (rows a sample does not own keep the sentinel); d = 1028: a second trip of the column loop"""
    lib = _lib.load()
    t = Tally(f"embed_tokens.{d}")
    B, L, vocab = 4, 12, 50
    g = torch.Generator().manual_seed(d)
    tokens = torch.randint(0, vocab, (B, L), generator=g, dtype=torch.int32)
    tokens[0, 0], tokens[1, 3], tokens[B - 1, L - 1], tokens[2, 0] = 0, vocab - 1, vocab - 1, vocab - 1
    table, pos = torch.randn(vocab, d, generator=g), torch.randn(L, d, generator=g)
    tok_d, table_d, pos_d = tokens.to(DEV), table.to(DEV), pos.to(DEV)
    for Lx in (L, 9, 1):
        for insert_col, n_tok in ((None, 0), (0, 3), (L - 3, 3), (4, 1)) + (((Lx - 2, 3),) if 2 < Lx < L else ()):      # (the last straddles Lx)
            img = None if insert_col is None else torch.randn(B, n_tok, d, generator=g)
            img_d = None if img is None else img.to(DEV)
            for packed in (False, True):
                lens = [0, 1, Lx, 5]
                seq_off = [0]
                for n in lens:
                    seq_off.append(seq_off[-1] + n)
                rows = seq_off[-1] if packed else B * Lx
                so_d = torch.tensor(seq_off, dtype=torch.int32, device=DEV) if packed else None
                buf, view = _guarded(rows, d, F32)
                _done(lib.keds_embed_tokens_ex(P(tok_d), P(table_d), P(pos_d), P(img_d), n_tok, insert_col or 0, view.data_ptr(), B, L, Lx, d, P(so_d), _lib.stream()),
                      "keds_embed_tokens_ex")
                want = rc.embed_ref(tokens, table, pos, img, n_tok, insert_col or 0, torch.full((rows, d), SENT), B, L, Lx, d, seq_off if packed else None)
                what = f"Lx {Lx} splice ({insert_col}, {n_tok}) packed {packed}"
                f = rc.bits_failures(view.cpu(), want, what)
                t.add("packed" if packed else "dense", [f] if f else [], f.worst, _untouched(buf, view), what)
    t.finish()


# ---- l2_normalize / mix_normalize ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", rc.NORM_DIMS)
def test_l2_and_mix_normalize(dim):
    """per element against float64, out of place and in place (out = x); an all-zero row gives a NaN row and leaves its neighbours"""
    lib = _lib.load()
    t = Tally(f"normalise.{dim}")
    for rows in (1, 4, 5):
        for regime in rc.L2_REGIMES + ("zero_row",):
            a = rc.norm_data(rows, dim, "random" if regime == "zero_row" else regime, seed=rows, device=DEV)[0]
            if regime == "zero_row":
                a[rows // 2] = 0.0
            exp = rc.l2_expected(a)
            buf, view = _guarded(rows, dim, F32)
            _done(lib.keds_l2_normalize(P(a), view.data_ptr(), rows, dim, _lib.stream()), "keds_l2_normalize")
            fails, worst = rc.norm_failures(view.clone(), exp, f"l2 {rows}x{dim}.{regime}")
            t.add(f"l2.{regime}", fails, worst, _untouched(buf, view), f"l2 {rows}x{dim}")
            view.copy_(a)
            _done(lib.keds_l2_normalize(view.data_ptr(), view.data_ptr(), rows, dim, _lib.stream()), "keds_l2_normalize in place")
            fails, worst = rc.norm_failures(view.clone(), exp, f"l2 in place {rows}x{dim}.{regime}")
            t.add(f"l2.{regime}", fails, worst, _untouched(buf, view), f"l2 in place {rows}x{dim}")
        for regime in (rc.MIX_REGIMES if dim > 1 else ()):
            a, b, wa, wb = rc.norm_data(rows, dim, regime, seed=rows, device=DEV)
            exps = rc.mix_expected(a, b, wa, wb)
            bufs = [_guarded(rows, dim, F32) for _ in range(3)]
            _done(lib.keds_mix_normalize(P(a), P(b), wa, wb, bufs[0][1].data_ptr(), bufs[1][1].data_ptr(), bufs[2][1].data_ptr(), rows, dim, _lib.stream()),
                  "keds_mix_normalize")
            for (buf, view), exp, nm in zip(bufs, exps, ("an", "bn", "mix")):
                fails, worst = rc.norm_failures(view.clone(), exp, f"mix.{nm} {rows}x{dim}.{regime}")
                t.add(f"mix.{regime}", fails, worst, _untouched(buf, view), f"mix.{nm} {rows}x{dim}")
    t.finish()


# ---- the read-out as the composition of its kernels ------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", (0, 1))
def test_readout_equals_its_three_kernels(normalize):
    """keds_readout = keds_layernorm_rows (gathered, bf16) -> keds_gemm_bt -> out-of-place keds_l2_normalize, bit for bit: pins the
    gathered LayerNorm and the in-place normalisation inside it.  With a row map (one row outside its sequence: a NaN row) and
    without one (the CLS rows)."""
    lib = _lib.load()
    B, S, E = 5, 7, 128
    for d in (256, 768):
        g = torch.Generator(device=DEV).manual_seed(d)
        x = torch.randn(B * S, d, generator=g, device=DEV) * 3.0 + 0.5
        gamma, beta = 1.0 + 0.5 * torch.randn(d, generator=g, device=DEV), 0.5 * torch.randn(d, generator=g, device=DEV)
        proj = (torch.randn(E, d, generator=g, device=DEV) * d ** -0.5).bfloat16()
        for row in (torch.tensor([0, 6, 3, 7, 2], dtype=torch.int32, device=DEV), None):
            nbytes = lib.keds_readout_workspace_bytes(B, d)
            ws1, ws2 = (torch.zeros(nbytes, dtype=torch.uint8, device=DEV) for _ in range(2))
            buf, out = _guarded(128, E, F32)
            _done(lib.keds_readout(P(x), S, P(row), P(gamma), P(beta), P(proj), out.data_ptr(), B, d, E, normalize, P(ws1), nbytes, _lib.stream()), "keds_readout")
            got = out[:B].clone()
            out[:B] = SENT
            assert bool((buf == SENT).all()), "keds_readout wrote outside its [B, E] output"
            _done(lib.keds_layernorm_rows(P(x), d, P(row), S, P(gamma), P(beta), P(ws2), 0, B, d, _lib.stream()), "keds_layernorm_rows")
            assert torch.equal(ws1, ws2), "the LayerNorm rows inside keds_readout differ from keds_layernorm_rows"
            y = torch.full((128, E), SENT, dtype=F32, device=DEV)
            _done(lib.keds_gemm_bt(P(ws2), P(proj), None, P(y), B, E, d, _lib.EPI_BIAS_F32, None, 0, _lib.stream()), "keds_gemm_bt")
            want = y[:B]
            if normalize:
                want = torch.empty_like(y[:B])
                _done(lib.keds_l2_normalize(P(y), P(want), B, E, _lib.stream()), "keds_l2_normalize")
            f = rc.bits_failures(got, want, f"readout d {d} normalize {normalize} map {row is not None}")
            assert not f, str(f)
            if row is not None:
                assert bool(torch.isnan(got[3]).all()) and bool(torch.isfinite(got[[0, 1, 2, 4]]).all())
