"""Proof, on the CPU, that the per-element MXFP8 GEMM checks (tests/mx_check.py) pass a faithful model of the kernels' rounding in both
K orders and catch each defect class of mx_check.MUTATIONS with room to spare -- while the whole-tensor limits the MXFP8 GEMMs were
held to before (tests/test_gpu_fp8.py) do not see them."""
import functools

import pytest
import torch

from tests import gemm_check as gc
from tests import mx_check as mc

KS = (256, 384, 512, 1024, 4096)
M, N = 288, 512                        # a second 256-row tile (ln_prev_tile), two 256-column tile columns, eight 64-column pairs
ROW, COL = 269, 300                    # piece 264 .. 271, row group 256 .. 271; tile column 1, 64-column pair 4, block 9
FACTOR = 4.0                           # a mutation must miss the bound by this much (or differ in bits in the integer regimes)


@functools.lru_cache(maxsize=None)
def _case(K, regime):
    return mc.MxCase(M, N, K, regime, seed=K)


def _worst(case, epi, **kw):
    return mc.model_failures(case, epi, mc.emulate_mx(case, epi, **kw))


def test_e4m3_helpers_agree_with_torch_on_every_byte_and_on_ties():
    """mx_check decodes with an explicit table and encodes with explicit arithmetic; this torch build converts float8_e4m3fn on the
    CPU, so both are compared with it: all 256 bytes, every midpoint between neighbours (ties to even), saturation, signed zeros"""
    b = torch.arange(256, dtype=torch.uint8)
    want = b.view(torch.float8_e4m3fn).double()
    got = mc.e4m3_decode(b)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got.nan_to_num(9e9), want.nan_to_num(9e9))
    fin = ~torch.isnan(got)
    assert torch.equal(mc.e4m3_encode(got[fin]), b[fin])                       # (-0 keeps its sign bit)
    pos = got[:0x7F]                                                           # 0 .. 448, ascending
    mid = (pos[:-1] + pos[1:]) / 2                                             # exact in float32
    x = torch.cat([mid, -mid, mid * (1 + 2.0 ** -20), mid * (1 - 2.0 ** -20), torch.tensor([449.0, 463.9, 1e6, -1e6, 2.0 ** -11, -2.0 ** -12, 0.0])])
    x = x.float().double()
    ref = x.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(mc.e4m3_encode(x), ref)
    assert int(mc.e4m3_encode(mid)[0]) == 0 and int(mc.e4m3_encode(mid)[1]) == 2      # ties to even
    assert int(mc.e4m3_encode(torch.tensor([float("nan")]))[0]) == mc.NAN_BYTE


def test_block_exponent_comes_from_the_exponent_field():
    one_below_two = torch.tensor([2.0 - 2.0 ** -23, 2.0, 1.0, 2.0 ** -140, 0.0, 3e38], dtype=torch.float32)
    assert mc.block_exp(one_below_two).tolist() == [-8, -7, -8, -127, -127, 119]
    s = mc.pack_scales(torch.tensor([[1, 2, 3, 4, 5, 6, 7, 8]]), 4)
    assert s.shape == (2, 4, 4) and s[1, 0].tolist() == [132, 133, 134, 135] and bool((s[:, 1:] == mc.PAD_SCALE).all())
    assert mc.unpack_scales(s, 1).tolist() == [[1, 2, 3, 4, 5, 6, 7, 8]]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("regime", mc.REGIMES)
def test_model_passes_every_epilogue_in_both_orders(regime, K):
    msgs, top = [], 0.0
    case = _case(K, regime)
    for epi in mc.NAMES:
        if regime not in mc.regimes_of(epi):
            continue
        for order in ("forward", "reverse"):
            fails, worst = _worst(case, epi, order=order)
            top = max(top, worst)
            msgs += [f"{order}: {f}" for f in fails]
    print(f"{case.name}: worst ratio of the clean model {top:.3g}")
    assert not msgs, "\n".join(msgs[:20])
    assert top <= 1.0


def test_model_without_bias_passes():
    case = _case(512, "random").without_bias()
    fails, worst = _worst(case, mc.EPI_BIAS)
    assert not fails and worst <= 1.0


def test_integer_cases_are_exact():
    """the properties the bit comparisons rest on, on the cases themselves: the magnitude sum (asserted by MxCase) and, where all
    scales are 2^0, the row statistics"""
    for K in KS:
        for regime in ("integer", "integer_pow2"):
            case = _case(K, regime)
            assert float(case.S.max()) + 32 < 2.0 ** 24
            assert bool((case.acc == case.acc.round()).all())
        assert gc.stats_exact(mc.expected(_case(K, "integer"), mc.EPI_RESID_MX_H).ref), K


RAMPS = ("blockramp_up", "blockramp_down")
ALL_EPIS = tuple(mc.NAMES)
# mutation -> (regimes, epilogues)
PLAN = {
    "drop_ktile": (RAMPS + ("integer", "integer_pow2"), ALL_EPIS),
    "stale_ktile": (("blockramp_up", "integer_pow2"), ALL_EPIS),
    "scale_next_block": (("blockjump", "integer_pow2"), ALL_EPIS),
    "scale_next_row": (("blockjump", "integer_pow2"), ALL_EPIS),
    "scale_pad_row": (("blockjump", "integer", "random"), ALL_EPIS),
    "shift_side": (("random", "integer", "offset"), ALL_EPIS),
    "ln_prev_tile": (("offset",), mc.LN_EPIS),
    "swap_mx_blocks": (("random", "integer", "blockjump"), mc.MX_EPIS),
    "swap_scale_pair": (("blockjump",), mc.MX_EPIS),
    "exp_minus1": (("random", "integer", "blockjump"), mc.MX_EPIS),
    "drop_store": (("random", "integer"), ALL_EPIS),
    "resid_twice": (("random", "integer"), (mc.EPI_RESID_MX, mc.EPI_RESID_MX_H)),
    "stats_miss16": (("random", "integer"), (mc.EPI_RESID_MX, mc.EPI_RESID_MX_H)),
    "stats_twice": (("random", "integer"), (mc.EPI_RESID_MX, mc.EPI_RESID_MX_H)),
}
WHOLE_COLUMNS = ("shift_side",)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("mutation", mc.MUTATIONS)
def test_each_mutation_misses_the_bound_by_a_factor(mutation, K):
    """Each defect, placed in ONE 8-row piece / 16-row group / row / block / store of the launch, fails in every regime made for it at
    every K: by >= 4 x the bound, or by inequality of bits in the integer regimes -- and nowhere but in the rows it touched.  drop / stale
    K-tile: the last K-tile (the first in blockramp_down; at two K-tiles a stale buffer is an empty one).  shift_side shifts the column
    sums on the LayerNorm epilogues (judged on `offset`) and the bias on the others.  The MX copy's own store is dropped once more
    on the residual epilogues (at=copy)."""
    regimes, epis = PLAN[mutation]
    nk = K // mc.TILE_K
    ran = 0
    for regime in regimes:
        for epi in epis:
            ln = epi in mc.LN_EPIS
            if regime not in mc.regimes_of(epi) or (mutation == "shift_side" and (regime == "offset") != ln):
                continue
            if ln and regime.startswith("integer") and mutation in ("swap_mx_blocks", "exp_minus1", "scale_pad_row"):
                continue                                   # (the LayerNorm forms are judged by the bound in the regimes made for them)
            case = _case(K, regime)
            ats = [dict(row=ROW, col=COL, kt=0 if regime == "blockramp_down" else nk - 1)]
            if mutation == "drop_store" and epi in (mc.EPI_RESID_MX, mc.EPI_RESID_MX_H):
                ats.append(ats[0] | dict(copy=True))
            for at in ats:
                fails, worst = _worst(case, epi, mutation=mutation, at=at)
                what = f"{mutation} on {case.name} {mc.NAMES[epi]} {at}"
                assert fails, f"{what}: not caught (worst ratio {worst:.3g})"
                assert worst >= FACTOR, f"{what}: caught by only {worst:.3g} x the bound"
                rows = {f[0] for fl in fails for f in fl}
                if mutation not in WHOLE_COLUMNS:
                    assert all(256 <= r_ < 272 for r_ in rows), (what, rows)
                ran += 1
    print(f"{mutation} K={K}: caught in {ran} (regime, epilogue) placements")
    assert ran >= 2


def test_whole_tensor_limits_miss_the_single_piece_mutations():
    """The gap this module closes.  In a 2048 x 1024 x 4096 launch on `random` data -- what tests/test_gpu_fp8.py runs -- one 8-row
    piece without a K-tile, one row group with its neighbouring block's scales in one K-tile and two interchanged MX blocks of one row
    pass the whole-tensor limits the suite had: rel-L2 <= 4e-3 (bf16 output), <= 5e-2 (MX output), <= 4e-4 (fp16 stream) and >= 99.9 %
    equal copy bytes.  The per-element checks fail each of them.  Placed in the 8-row piece of the smallest rows (the per-row factor
    of `random` spreads the rows' weight in the norm).  Left out, because the fp16 stream's tight 4e-4 does see them at this size: a K-tile missing
    from 8 x 256 outputs (2.3e-3 sigma_row of the norm) and a row group's wrong block scales (measured 1.1e-3); the interchanged blocks
    of its MX copy pass it, and its 99.9 % of equal bytes."""
    case = mc.MxCase(2048, 1024, 4096, "random", seed=1)
    energy = mc.dequantize(case.aq, case.a_exp).square().sum(1).reshape(-1, 8).sum(1)
    row = int(energy.argmin()) * 8
    at = dict(row=row, col=600, kt=7)
    g0 = row // 16 * 16
    for epi, limit in ((mc.EPI_BIAS, 4e-3), (mc.EPI_LN_QGELU_MX, 5e-2), (mc.EPI_RESID_MX_H, 4e-4)):
        exp = mc.expected(case, epi)
        clean = mc.emulate_mx(case, epi)
        assert not mc.model_failures(case, epi, clean)[0]
        for mutation in ("drop_ktile", "scale_next_block", "swap_mx_blocks"):
            if (mutation == "swap_mx_blocks" and epi not in mc.MX_EPIS) or (mutation != "swap_mx_blocks" and epi == mc.EPI_RESID_MX_H):
                continue
            res = mc.emulate_mx(case, epi, mutation=mutation, at=at)
            got = res["out"] if "out" in res else mc.dequantize(res["q"], res["qexp"])
            r = gc.rel_l2(got, exp.ref)
            same = float((res["q"] == clean["q"]).double().mean()) if "q" in res else 1.0
            fails, worst = mc.model_failures(case, epi, res)
            print(f"{mc.NAMES[epi]} {mutation}: rel_l2 {r:.3e} (limit {limit:g}), copy bytes equal {same:.5f}; per element: worst {worst:.3g}")
            assert r <= limit and same >= 0.999, "the whole-tensor numbers saw it"
            assert fails and worst >= FACTOR
            assert all(g0 <= m < g0 + 16 for fl in fails for m, _, _ in fl)
