"""The attention checker checked (tests/attention_check.py; no GPU): a CPU model of the kernels' rounding passes the per-element
bound in every regime, and the same model with one mask defect -- a pad key let in, the causal diagonal off by one either way, the
last key dropped, two rows exchanged -- fails it in the `ramp` regime at every sequence length, by a factor of at least 4.  A bound
four times looser, or a suite without `ramp`, would not pass this file."""
import functools

import pytest
import torch

from tests import attention_check as ac

B, H = 3, 3                       # the shape of the GPU cases (tests/test_gpu_attention_edges.py)
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]


@functools.lru_cache(maxsize=None)
def _case(S, regime, dtype, causal):
    qkv = ac.make_qkv(B, S, H, regime, dtype, seed=S)
    return qkv, ac.Case(qkv, B, S, H, causal, name=f"S{S}.{regime}")


@pytest.mark.parametrize("regime", ac.REGIMES)
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rounding_model_passes_the_bound(dtype, causal, regime):
    """fp32 scores, P rounded to the type, fp32 sum of the unrounded P, output rounded: inside the bound (measured peak 0.81)."""
    bad, worst = [], 0.0
    for S in ac.S_EDGES:
        qkv, case = _case(S, regime, dtype, causal)
        f = ac.check(ac.emulate(qkv, B, S, H, causal), case)
        worst = max(worst, f.worst)
        if f:
            bad.append(f"S={S}: {f}")
    print(f"[host] emulate {IDS[DTYPES.index(dtype)]} causal={causal} {regime}: worst ratio {worst:.3f}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_first_tile_reference_passes_where_it_cannot_overflow(dtype, causal):
    """Probabilities taken relative to the maximum of the first 32 keys (the first pass of the S = 257 kernel) are as good as those
    relative to the row maximum -- bf16 and fp32 keep their relative precision at any exponent -- as long as nothing overflows."""
    bad = []
    for regime in ("random", "flat") + (("ramp",) if dtype == torch.bfloat16 else ()):
        for S in ac.S_EDGES:
            qkv, case = _case(S, regime, dtype, causal)
            f = ac.check(ac.emulate(qkv, B, S, H, causal, first_tile=32), case)
            if f:
                bad.append(f"{regime} S={S}: {f}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("regime", ["ramp", "peaked"])
def test_first_tile_reference_overflows_fp16(regime):
    """Why the fp16 form of the S = 257 kernel recomputes: in `ramp` the later key tiles sit ~20 log2 units above the first, in
    `peaked` far more, and exp2 of that leaves fp16's range when P is packed -- the one-pass result is not finite."""
    S = 257
    qkv, case = _case(S, regime, torch.float16, False)
    got = ac.emulate(qkv, B, S, H, False, first_tile=32)
    assert not torch.isfinite(got.float()).all()
    assert ac.check(got, case)
    assert not ac.check(ac.emulate(qkv, B, S, H, False), case)          # with the true maximum: fine


# (causal_* without the mask and pad under it are no defects: ac.applicable)
DEFECTS = [(c, m) for c in (False, True) for m in ac.MUTATIONS if any(ac.applicable(m, S, c) for S in ac.S_EDGES)]


@pytest.mark.parametrize("causal,mutation", DEFECTS, ids=[("causal-" if c else "full-") + m for c, m in DEFECTS])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_mask_defect_fails_the_bound_in_ramp(dtype, causal, mutation):
    """Worst ratio >= 4 at EVERY sequence length where the mutation is a defect at all (ac.applicable).  `flat` alone would not do:
    it misses `pad` at S = 255 and 287 in bf16 (test_flat_alone_misses_a_pad_key below), and `random` misses much more."""
    lens = [S for S in ac.S_EDGES if ac.applicable(mutation, S, causal)]
    missed, low = [], float("inf")
    for S in lens:
        qkv, case = _case(S, "ramp", dtype, causal)
        f = ac.check(ac.emulate(qkv, B, S, H, causal, mutation=mutation), case)
        low = min(low, f.worst)
        if not f or f.worst < 4.0:
            missed.append((S, f.worst))
    print(f"[host] {mutation} {IDS[DTYPES.index(dtype)]} causal={causal}: smallest worst ratio {low:.3g} over {len(lens)} lengths")
    assert not missed, missed


def test_flat_alone_misses_a_pad_key():
    """One zero pad key among 255 or 287 nearly equal weights dilutes the row by less than one bf16 ulp: inside the bound in
    `flat`, far outside it in `ramp` (where the pad key's score 0 lies above every real score)."""
    for S in (255, 287):
        qkv, case = _case(S, "flat", torch.bfloat16, False)
        assert not ac.check(ac.emulate(qkv, B, S, H, False, mutation="pad"), case)
        qkv, case = _case(S, "ramp", torch.bfloat16, False)
        assert ac.check(ac.emulate(qkv, B, S, H, False, mutation="pad"), case).worst >= 4.0


def test_packed_cases_and_q_limit():
    """The packed layout: every sample is checked against its own keys only, a key of the neighbour let in fails, and q_limit
    confines the check to the rows a launch computes."""
    lens = [5, 31, 1, 32]
    regimes = ["ramp", "random", "ramp", "random"]
    for dtype in DTYPES:
        qkv = ac.make_qkv(len(lens), lens, H, regimes, dtype, seed=7)
        for causal in (False, True):
            case = ac.Case(qkv, len(lens), lens, H, causal)
            got = ac.emulate(qkv, len(lens), lens, H, causal)
            assert not ac.check(got, case)
            if not causal:
                # samples 0 and 1 attended as ONE sequence of 36 rows: the rows of sample 0 (ramp) see the keys of sample 1
                merged = ac.emulate(qkv[:36], 1, 36, H, causal)
                f = ac.check(torch.cat([merged, got[36:]]), case)
                assert 0 in {b for b, _, _, _ in f} and f.worst >= 4.0
                assert not {b for b, _, _, _ in f} - {0, 1}
            spoiled = got.clone()
            spoiled[3] = 100.0                                           # row 3 of sample 0
            assert [(b, r) for b, _, r, _ in ac.check(spoiled, case)] == [(0, 3)] * H
            assert not ac.check(spoiled, case, q_limit=3)


def test_f32_grade_check_against_torch32():
    """check_f32: a float32 evaluation passes against itself by construction; an error of 2^-12 of (A + |o|) on one row does not."""
    S = 33
    for regime in ac.REGIMES:
        qkv = ac.make_qkv(B, S, H, regime, torch.float32, seed=S)
        case = ac.Case(qkv, B, S, H, True)
        ref32 = ac.torch32(case)
        f = ac.check_f32(ref32, case)
        assert not f and f.limit >= ac.F32_FLOOR and f.worst <= f.limit / ac.F32_MARGIN + 1e-12
        off = ref32.clone().double()
        off[S + 4] += 2.0 ** -12 * (case.A + case.o.abs())[S + 4]
        f = ac.check_f32(off, case)
        assert sorted({(b, r) for b, _, r, _ in f}) == [(1, 4)], (regime, f.limit, str(f))
