"""Proof, on the CPU, that the per-element GEMM check (tests/gemm_check.py) passes a faithful model of the kernels' rounding in every
order the kernels may add in, and catches each defect class of gemm_check.MUTATIONS with room to spare -- while today's whole-tensor
rel-L2 does not see the single-piece ones."""
import functools

import pytest
import torch

from tests import gemm_check as gc

KS = (64, 512, 1024, 4096)
M, N = 24, 512                         # three 8-row pieces, two 256-column tile columns, four 128-column ones
FACTOR = 4.0                           # a mutation must miss the bound by this much (or differ in bits in the integer regime)
ORDERS = (("forward", 1), ("reverse", 1), ("forward", 2), ("forward", 4), ("reverse", 16))


@functools.lru_cache(maxsize=None)
def _case(K, regime, dtype, m=M, n=N):
    return gc.Case(m, n, K, regime, dtype, seed=K)


def _worst(case, code, **kw):
    fails, worst = gc.model_failures(case, code, gc.emulate(case, code, **kw))
    return fails, worst


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("regime", gc.REGIMES)
def test_model_passes_every_epilogue_in_every_order(regime, K):
    """The unmutated model is inside the bound (equal to the bit where the bits are known) for every epilogue code, K-tiles forwards
    and backwards and in 2 / 4 / 16 split-K slices."""
    msgs, top = [], 0.0
    for code, (op, _, fam) in gc.EPILOGUES.items():
        case = _case(K, regime, op)
        for order, splits in ORDERS:
            if (K // gc.TILE_K) % splits:
                continue
            fails, worst = _worst(case, code, order=order, splits=splits)
            top = max(top, worst)
            msgs += [f"{order} x{splits}: {f}" for f in fails]
    assert not msgs, "\n".join(msgs[:20])
    assert top <= 1.0


def test_integer_cases_have_exact_statistics():
    """the property the bit comparison of the row statistics rests on, asserted on the cases themselves"""
    for K in KS:
        for dt in (gc.BF, gc.HF):
            case = _case(K, "integer", dt)
            assert gc.stats_exact(gc.expected(case, 9 if dt == gc.BF else 18).ref), case.name


# mutation -> (regimes, epilogue codes, model arguments)
PLAN = {
    "drop_ktile": (("tail", "head", "integer"), (0, 4, 6, 9, 20), {}),
    "stale_ktile": (("tail", "integer"), (0, 4, 16, 18), {}),
    "swap_rows": (("random", "integer"), (0, 4, 7), {}),
    "shift_side": (("random", "integer", "offset"), (0, 1, 4, 6, 17), {}),
    "bias_per_slice": (("random", "integer"), (0, 4, 8, 6), {"splits": 2}),
    "drop_store": (("random", "integer"), (0, 4, 5, 16), {}),
    "resid_twice": (("random", "integer"), (3, 8, 9, 19), {}),
    "ln_row_plus1": (("offset",), (6, 7, 10, 16), {}),
    "stats_miss16": (("random", "integer"), (8, 9, 18), {}),
    "stats_twice": (("random", "integer"), (8, 9, 18), {}),
}


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("mutation", gc.MUTATIONS)
def test_each_mutation_misses_the_bound_by_a_factor(mutation, K):
    """Each defect, placed in ONE 8-row piece / row / store of the launch, fails in the regime made for it at every K: by >= 4 x the
    bound, or by inequality of bits in the integer regime.  (A bound that only just catches a defect misses its milder cousin.)
    drop / stale K-tile: the last K-tile in `tail`, the first in `head` (at K = 64 there is one tile, and a stale buffer is an empty
    one).  shift_side on the LayerNorm forms shifts the column sums and is judged on `offset`; on the others the bias.
    bias_per_slice needs two K-tiles to split: not at K = 64."""
    regimes, codes, kw = PLAN[mutation]
    nk = K // gc.TILE_K
    if mutation == "bias_per_slice" and nk < 2:
        return
    ran = 0
    for regime in regimes:
        for code in codes:
            op, _, fam = gc.EPILOGUES[code]
            ln = fam in ("ln", "ln_qgelu")
            if mutation == "shift_side" and ((regime == "offset") != ln):
                continue
            case = _case(K, regime, op)
            at = dict(row=13, col=300, kt=0 if regime == "head" else nk - 1)
            fails, worst = _worst(case, code, mutation=mutation, at=at, **kw)
            assert fails, f"{mutation} on {case.name} code {code}: not caught (worst ratio {worst:.3g})"
            assert worst >= FACTOR, f"{mutation} on {case.name} code {code}: caught by only {worst:.3g} x the bound"
            # and it fails WHERE the defect is: nothing outside the piece's rows
            rows = {f[0] for fl in fails for f in fl}
            if mutation not in ("shift_side", "bias_per_slice"):          # (those two are defects of a whole column group)
                assert all(8 <= r_ < 16 for r_ in rows), (mutation, case.name, code, rows)
            ran += 1
    assert ran >= 2


def test_whole_tensor_rel_l2_misses_the_single_piece_mutations():
    """The gap this module closes: in a 4352 x 4096 x 1024 launch one 8-row piece that drops, or reads stale, one K-tile passes
    rel_l2 <= 4e-3 -- the only GEMM assertion the suite had -- while the per-element check fails it by orders of magnitude."""
    case = gc.Case(4352, 4096, 1024, "random", gc.BF, seed=1)
    exp = gc.expected(case, 0)
    clean = gc.emulate(case, 0)["out"]
    base = gc.rel_l2(clean, exp.ref)
    assert not gc.check(clean, exp) and base <= 4e-3
    for mutation in ("drop_ktile", "stale_ktile"):
        got = gc.emulate(case, 0, mutation=mutation, at=dict(row=1000, col=2000, kt=7))["out"]
        r = gc.rel_l2(got, exp.ref)
        f = gc.check(got, exp, mutation)
        print(f"{mutation}: rel_l2 {r:.3e} (clean {base:.3e}); per element: {f.count} beyond the bound, worst {f.worst:.3g}")
        assert r <= 4e-3, "the whole-tensor number saw it"
        assert f.count >= 0.9 * 8 * 256 and f.worst >= 10 * FACTOR
        assert all(1000 <= m < 1008 and 1792 <= n < 2048 for m, n, _ in f)


def test_failure_report_names_tiles_and_groups():
    case = _case(512, "random", gc.BF)
    f = gc.check(gc.emulate(case, 0, mutation="drop_store", at=dict(row=13, col=300))["out"], gc.expected(case, 0), "x")
    assert f.count == 8 and [(m, n) for m, n, _ in f][:2] == [(13, 296), (13, 297)]
    s = str(f)
    assert "8 elements" in s and "tile256 (0, 1) row 13 col 40" in s and "tile128 (0, 2)" in s and "group8 37" in s
