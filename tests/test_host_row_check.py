"""Proof, on the CPU, that the per-element checks of the row kernels (tests/row_check.py) pass float32 models of the kernels -- adding
in the kernels' own orders, forwards and reversed, with and without contracted multiply-adds -- in every regime at every dim the
device tests use, and catch every mutation of row_check by >= 4 x the bound or by inequality of bits; and which of those mutations
the whole-tensor limits the suite had (rel-L2 <= 1e-5 fp32, 5e-3 bf16) let through."""
import functools

import pytest
import torch

from tests import gemm_check as gc
from tests import row_check as rc

FACTOR = 4.0
ROWS = 24
VARIANTS = [(o, f) for o in ("forward", "reverse") for f in (False, True)]
OUTS = (rc.BF, rc.F32, rc.HF, "pair")
NW = 8                                  # the stream model's wave count: 19 rows = waves of three and of two trips
STREAM_ROWS = 19
FACTORS = {}                            # mutation -> the smallest factor over the dims (printed; docs/kernels.md quotes them)


@functools.lru_cache(maxsize=None)
def _ln(rows, dim, regime, group=1):
    return rc.LnCase(rows, dim, regime, seed=1, group=group)


def _res_dtype(out):
    return rc.HF if out == "pair" else out


def _note(mutation, worst):
    FACTORS[mutation] = min(FACTORS.get(mutation, float("inf")), worst)
    print(f"[factor] {mutation}: {worst:.3g}")


def _caught(mutation, fails, worst, name):
    top = max([worst] + [f.worst for f in fails])
    assert fails, f"{mutation} on {name}: not caught (worst ratio {worst:.3g})"
    assert top >= FACTOR, f"{mutation} on {name}: caught by only {top:.3g} x the bound"
    return top


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", rc.LN_DIMS)
@pytest.mark.parametrize("regime", rc.LN_REGIMES + ("rowscale",))
def test_layernorm_models_pass_in_every_order(regime, dim):
    """the one-row form at every dim and output type, the stream form at 512 / 1024, chains and butterflies forwards and reversed, with
    and without fused multiply-adds"""
    case = _ln(ROWS, dim, regime)
    msgs, top = [], 0.0
    forms = ("row", "stream") if dim in (512, 1024) else ("row",)
    for form in forms:
        for out in (OUTS if form == "row" else ("pair",)):
            for order, fma in VARIANTS:
                res = rc.ln_model(case.x, case.gamma, case.beta, out, form=form, order=order, fma=fma, nw=NW)
                fails, worst = rc.ln_failures(case, res, _res_dtype(out), what=f"{form}.{order}.fma{int(fma)}.")
                msgs += [str(f) for f in fails]
                top = max(top, worst)
    print(f"[model] layernorm {regime} dim {dim}: worst ratio {top:.3g}")
    assert not msgs, "\n".join(msgs[:10])
    assert top <= 1.0


def test_plain_sequential_sum_does_not_fit_the_bound():
    """why the model adds in the kernels' orders: the bound's L = dim / 64 + 8 is a lane's chain, not a chain of dim additions -- one
    thread adding 2,048 columns in turn leaves it in `constant`"""
    case = _ln(ROWS, 2048, "constant")
    x = case.x
    s = torch.zeros(ROWS, 1)
    for c in range(2048):
        s = s + x[:, c:c + 1]
    mean = s / 2048.0
    d = x - mean
    q = torch.zeros(ROWS, 1)
    for c in range(2048):
        q = q + d[:, c:c + 1] * d[:, c:c + 1]
    rstd = ((q / 2048.0).double() + 1e-5).rsqrt().float()
    out = d * rstd * case.gamma + case.beta
    fails, worst = rc.ln_failures(case, {"out": out}, rc.F32)
    print(f"[model] sequential sum, constant, dim 2048: {worst:.3g} x the bound")
    assert fails and worst > 1.0


# mutation -> (regime, output types)
LN_PLAN = {
    "gamma_chunk": ("random", OUTS),
    "stats_short": ("offset1k", OUTS),
    "one_pass_var": ("offset1k", OUTS),
    "rstd_row_plus1": ("rowscale", OUTS),
    "drop_store": ("random", OUTS),
    "lo_zero": ("random", ("pair",)),
    "lo_of_rounded": ("random", ("pair",)),
}


@pytest.mark.parametrize("dim", rc.LN_DIMS)
@pytest.mark.parametrize("mutation", tuple(LN_PLAN))
def test_each_layernorm_mutation_misses_the_bound_by_a_factor(mutation, dim):
    regime, outs = LN_PLAN[mutation]
    case = _ln(ROWS, dim, regime)
    low = float("inf")
    for out in outs:
        for form in (("row", "stream") if out == "pair" and dim in (512, 1024) else ("row",)):
            res = rc.ln_model(case.x, case.gamma, case.beta, out, form=form, mutation=mutation, at=dict(row=13, col=dim - 5), nw=NW)
            fails, worst = rc.ln_failures(case, res, _res_dtype(out))
            low = min(low, _caught(mutation, fails, worst, f"{case.name} {out} {form}"))
            if mutation == "drop_store":                                        # it fails WHERE the defect is
                assert {f[0] for fl in fails for f in fl} == {13}
    _note(mutation, low)


def _gather_setup(dim, row_mul):
    """9 output rows over a [9 row_mul, dim] source; the map hits 0, row_mul - 1, row_mul and -1"""
    rows = 9
    case = _ln(rows * row_mul, dim, "rowscale", group=row_mul)
    row_map = torch.tensor([0, row_mul - 1, row_mul, -1, row_mul // 2, 0, row_mul - 1, 3 * row_mul, (row_mul + 1) // 3], dtype=torch.int32)
    return case, rows, row_map


@pytest.mark.parametrize("dim", rc.LN_DIMS)
@pytest.mark.parametrize("row_mul", (1, 77))
def test_gathered_layernorm_model_and_its_mutations(row_mul, dim):
    """the gathered form: rows outside [0, row_mul) are NaN, the others pass; the map of row r + 1 and a row taken modulo are caught"""
    case, rows, row_map = _gather_setup(dim, row_mul)
    src, bad = rc.gather_sources(rows, row_map, row_mul)
    assert int(bad.sum()) == 3
    for out in (rc.F32, rc.BF):
        res = rc.ln_model(case.x[src], case.gamma, case.beta, out, bad=bad)
        fails, worst = rc.ln_failures(case, res, out, src, bad)
        assert not fails and worst <= 1.0, [str(f) for f in fails]
        for mutation in rc.GATHER_MUTATIONS:
            msrc, mbad = rc.gather_sources(rows, row_map, row_mul, mutation)
            res = rc.ln_model(case.x[msrc], case.gamma, case.beta, out, bad=mbad)
            fails, worst = rc.ln_failures(case, res, out, src, bad)
            _note(mutation, _caught(mutation, fails, worst, f"{case.name} mul {row_mul}"))
    # the CLS form: no map, every row_mul-th row
    src, bad = rc.gather_sources(rows, None, row_mul)
    res = rc.ln_model(case.x[src], case.gamma, case.beta, rc.F32)
    assert not rc.ln_failures(case, res, rc.F32, src, bad)[0]


@pytest.mark.parametrize("dim", (512, 1024))
@pytest.mark.parametrize("mutation", rc.STREAM_MUTATIONS)
def test_each_stream_mutation_misses_the_bound_by_a_factor(mutation, dim):
    """19 rows on 8 waves: rows x 2^6 on every other group of nw make the registers of row r + nw gross; a wave that skips its last trip
    leaves the sentinel"""
    case = _ln(STREAM_ROWS, dim, "rowscale", group=NW)
    clean = rc.ln_model(case.x, case.gamma, case.beta, "pair", form="stream", nw=NW)
    assert not rc.ln_failures(case, clean, rc.HF)[0]
    res = rc.ln_model(case.x, case.gamma, case.beta, "pair", form="stream", mutation=mutation, nw=NW)
    fails, worst = rc.ln_failures(case, res, rc.HF)
    _note(mutation, _caught(mutation, fails, worst, case.name))


# ---- row statistics --------------------------------------------------------------------------------------------------------------
STATS_DIMS = (4, 252, 256, 260, 1024, 2044, 2048)


@pytest.mark.parametrize("dim", STATS_DIMS)
@pytest.mark.parametrize("dtype", (rc.BF, rc.HF), ids=("bf16", "fp16"))
def test_rowstats_model_and_mutation(dtype, dim):
    """the model passes in `random` and is exact in `integer`; sum x^2 taken of the rounded copy differs in bits in `integer`"""
    for regime in ("random", "integer"):
        x = rc.stats_data(5, dim, regime, seed=2)
        for order, fma in VARIANTS:
            copy, st = rc.stats_model(x, dtype, order, fma)
            fails, worst = rc.stats_failures(x, copy, st, dtype, regime == "integer", f"{dim}.{regime}")
            assert not fails and worst <= 1.0, [str(f) for f in fails]
    x = rc.stats_data(5, dim, "integer", seed=2)
    copy, st = rc.stats_model(x, dtype, mutation="sq_of_rounded")
    fails, worst = rc.stats_failures(x, copy, st, dtype, True, "sq_of_rounded")
    _note("sq_of_rounded", _caught("sq_of_rounded", fails, worst, f"{dim}"))


# ---- LayerNorm fold --------------------------------------------------------------------------------------------------------------
FOLD_K = (1, 63, 64, 65, 640, 1000)


@pytest.mark.parametrize("K", FOLD_K)
@pytest.mark.parametrize("dtype", (rc.BF, rc.HF), ids=("bf16", "fp16"))
def test_fold_model_and_mutations(dtype, K):
    """csum of the unrounded products: another integer in `integer` (bits); beta of column k + 1: gross in `random`, bits in `integer`"""
    for regime in ("random", "integer"):
        case = rc.FoldCase(5, K, regime, seed=3)
        for with_bias in (True, False):
            for order, fma in VARIANTS:
                wf, bc = rc.fold_model(case, dtype, with_bias, order, fma)
                fails, worst, _ = rc.fold_failures(case, wf, bc, dtype, with_bias)
                assert not fails and worst <= 1.0, [str(f) for f in fails]
    case = rc.FoldCase(5, K, "integer", seed=3)
    assert bool(((case.W * case.gamma).to(dtype).float() != case.W * case.gamma).any()), "no product of the integer regime is rounded"
    wf, bc = rc.fold_model(case, dtype, mutation="csum_unrounded")
    fails, worst, _ = rc.fold_failures(case, wf, bc, dtype)
    _note("csum_unrounded", _caught("csum_unrounded", fails, worst, case.name))
    for regime in ("random", "integer"):
        if K == 1:                                   # one column: its neighbour is itself
            continue
        case = rc.FoldCase(5, K, regime, seed=3)
        wf, bc = rc.fold_model(case, dtype, mutation="beta_plus1")
        fails, worst, _ = rc.fold_failures(case, wf, bc, dtype)
        _note("beta_plus1", _caught("beta_plus1", fails, worst, case.name))


def test_round_once_is_one_rounding():
    """1 + 2^-11 + 2^-30 lies above the fp16 tie: fp32 first rounds it onto the tie and then to even (1), one rounding gives 1 + 2^-10"""
    p = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -30, 1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -11], dtype=torch.float64)
    assert rc.round_once(p, rc.HF).tolist() == [1.0 + 2.0 ** -10, 1.0 + 2.0 ** -8, 1.0]
    assert p.float().half().tolist()[0] == 1.0
    assert rc.round_once(p, rc.BF).tolist()[1] == 1.0 + 2.0 ** -7 and p.float().bfloat16().tolist()[1] == 1.0


# ---- embed_tokens, cast16 --------------------------------------------------------------------------------------------------------
def _embed_inputs(d, B=3, L=12, vocab=50, n_tok=3):
    g = torch.Generator().manual_seed(d)
    tokens = torch.randint(0, vocab, (B, L), generator=g, dtype=torch.int32)
    tokens[0, 0], tokens[B - 1, L - 1] = 0, vocab - 1
    return tokens, torch.randn(vocab, d, generator=g), torch.randn(L, d, generator=g), torch.randn(B, n_tok, d, generator=g)


@pytest.mark.parametrize("d", (4, 128, 1028))
def test_embed_tokens_mutations_differ_in_bits(d):
    B, L, n_tok = 3, 12, 3
    tokens, table, pos, img = _embed_inputs(d)
    for Lx, insert_col, seq_off in [(12, 2, None), (9, 7, None), (9, 2, [0, 1, 10, 15])]:
        rows = (seq_off[-1] if seq_off else B * Lx) + 16
        x0 = torch.full((rows, d), rc.SENT)
        want = rc.embed_ref(tokens, table, pos, img, n_tok, insert_col, x0, B, L, Lx, d, seq_off)
        assert bool((want[rows - 16:] == rc.SENT).all())
        for mutation in ("shift_off_by_one", "pos_by_source", "packed_full"):
            if (mutation == "packed_full") != (seq_off is not None):
                continue
            if mutation != "packed_full" and insert_col + n_tok >= Lx:
                continue                              # nothing behind the splice inside the cut
            got = rc.embed_ref(tokens, table, pos, img, n_tok, insert_col, x0, B, L, Lx, d, seq_off, mutation)
            f = rc.bits_failures(got, want, mutation)
            assert f and f.worst == float("inf"), mutation
            _note(mutation, f.worst)


@pytest.mark.parametrize("count", (1, 2, 3, 5, 1023, 3 * 1024 + 1, 3 * 1024 + 2, 3 * 1024 + 3))
def test_cast16_tail_left_unwritten_differs_in_bits(count):
    x = torch.randn(count + 8, generator=torch.Generator().manual_seed(count))
    for dtype in (rc.BF, rc.HF):
        want = rc.cast16_model(x, dtype, count)
        assert bool((want[count:] == rc.SENT).all()) and not rc.bits_failures(want[:count], rc.cast_ref(x[:count], dtype))
        f = rc.bits_failures(rc.cast16_model(x, dtype, count, "tail_unwritten"), want)
        assert f and f.count == count % 4
        _note("tail_unwritten", f.worst)


def test_cast_specials_cover_what_a_cast_can_get_wrong():
    f = rc.cast_specials(rc.F32)
    h, b = f.half(), f.bfloat16()
    assert float(h[f == 65504.0][0]) == 65504.0 and bool(torch.isinf(h[f == 65520.0]).all()) and bool(torch.isinf(h[f == 7e4]).all())
    assert bool(torch.isinf(b[f == 3.4028234663852886e38]).all())
    assert float(h[f == 1.0 + 2.0 ** -11][0]) == 1.0 and float(h[f == 1.0 + 3 * 2.0 ** -11][0]) == 1.0 + 2.0 ** -9       # ties to even
    assert float(b[f == 1.0 + 2.0 ** -8][0]) == 1.0 and float(b[f == 1.0 + 3 * 2.0 ** -8][0]) == 1.0 + 2.0 ** -6
    s = rc.cast_specials(rc.HF)
    assert int(((s.float().abs() < 2.0 ** -14) & (s != 0)).sum()) >= 4           # fp16 subnormals as source


# ---- l2_normalize / mix_normalize ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", rc.NORM_DIMS)
def test_normalise_models_pass(dim):
    top_l2, top_mix = 0.0, 0.0
    for order, fma in VARIANTS:
        for regime in rc.L2_REGIMES:
            a, _, _, _ = rc.norm_data(5, dim, regime, seed=4)
            fails, worst = rc.norm_failures(rc.l2_model(a, order, fma), rc.l2_expected(a), f"l2.{regime}.{dim}")
            assert not fails, [str(f) for f in fails]
            top_l2 = max(top_l2, worst)
        for regime in (rc.MIX_REGIMES if dim > 1 else ()):
            a, b, wa, wb = rc.norm_data(5, dim, regime, seed=4)
            exps = rc.mix_expected(a, b, wa, wb)
            for got, exp, nm in zip(rc.mix_model(a, b, wa, wb, order, fma), exps, ("an", "bn", "mix")):
                fails, worst = rc.norm_failures(got, exp, f"mix.{regime}.{dim}.{nm}")
                assert not fails, [str(f) for f in fails]
                top_mix = max(top_mix, worst)
    print(f"[model] normalise dim {dim}: l2 {top_l2:.3g}, mixture {top_mix:.3g}")
    a = rc.norm_data(5, dim, "random", seed=4)[0]
    a[2] = 0.0
    got = rc.l2_model(a)
    assert bool(torch.isnan(got[2]).all()) and not rc.norm_failures(got, rc.l2_expected(a))[0]
    assert rc.norm_failures(torch.where(torch.isnan(got), torch.zeros_like(got), got), rc.l2_expected(a))[0]


# ---- what the whole-tensor limits let through -----------------------------------------------------------------------------------
def test_whole_tensor_limits_against_the_mutations():
    """514 x 1024, `random`, the limits test_layernorm asserts (rel-L2 <= 1e-5 for fp32 output, 5e-3 for bf16): every mutation below is
    caught per element by >= 4 x; the whole-tensor number lets the listed ones through"""
    case = rc.LnCase(514, 1024, "random", seed=5)
    ref, _ = case.ref()
    passed = {}
    for out, limit in ((rc.F32, 1e-5), (rc.BF, 5e-3)):
        clean = rc.ln_model(case.x, case.gamma, case.beta, out)["out"]
        assert gc.rel_l2(clean, ref) <= limit
        for mutation in ("gamma_chunk", "stats_short", "one_pass_var", "rstd_row_plus1", "drop_store"):
            full = rc.ln_model(case.x, case.gamma, case.beta, out, mutation=mutation, at=dict(row=300, col=500))["out"]
            got = full
            if mutation in ("gamma_chunk", "rstd_row_plus1"):                   # in ONE workgroup's four rows
                got = clean.clone()
                got[300:304] = full[300:304]
            if mutation == "drop_store":                                        # into a zeroed buffer, as the suite's tests allocate
                got = torch.where(got == rc.SENT, torch.zeros_like(got), got)
            r = gc.rel_l2(got, ref)
            fails, worst = rc.ln_failures(case, {"out": got}, out)
            top = max([worst] + [f.worst for f in fails])
            print(f"[whole-tensor] {mutation} {rc.TYPE_NAME[out]}: rel_l2 {r:.3e} (limit {limit:g}), per element {top:.3g} x the bound")
            passed[(mutation, out)] = r <= limit
            if mutation != "one_pass_var":                                      # (harmless on this regime: that is offset1k's job)
                assert fails and top >= FACTOR, (mutation, out, top)
    assert passed[("stats_short", rc.BF)] and passed[("drop_store", rc.BF)] and passed[("one_pass_var", rc.BF)] and passed[("one_pass_var", rc.F32)]
