"""Proof, on the CPU, that the per-element checks of the training kernels (tests/train_check.py) pass float32 models of the kernels --
adding in the kernels' own orders, lane chains and butterflies forwards and reversed -- in every regime at every shape the device
tests use, and catch every mutation of train_check by >= 4 x the bound or by inequality of bits in at least one regime at every shape
where it applies; and which of those mutations the whole-tensor limits of tests/test_gpu_train.py::test_building_blocks_against_torch
let through at that test's own shapes."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import gemm_check as gc
from tests import train_check as tc

FACTOR = 4.0
ORDERS = ("forward", "reverse")
FACTORS = {}                            # mutation -> the smallest factor over the shapes (printed; docs/kernels.md quotes them)


def _note(mutation, top):
    FACTORS[mutation] = min(FACTORS.get(mutation, float("inf")), top)
    print(f"[factor] {mutation}: {top:.3g}")


def _inside(fails, worst, name):
    assert not fails, f"{name}: the model leaves the bound: " + "; ".join(str(f) for f in fails[:4])
    assert worst <= 1.0, (name, worst)
    return worst


def _best(mutation, tops, name):
    """tops: the factor by which each regime catches the mutation (0: not caught) -> the mutation fails in at least one regime"""
    top = max(tops)
    assert top >= FACTOR, f"{mutation} on {name}: caught by only {top:.3g} x the bound in its best regime"
    _note(mutation, top)


def _factor(fails, worst):
    return tc._top(fails, worst) if fails else 0.0


# ---- attention backward --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _att(B, S, H, regime, causal):
    qkv, go = tc.att_inputs(B, S, H, regime, seed=S)
    return qkv, go, tc.att_reference(qkv, go, B, S, H, causal)


@pytest.mark.parametrize("S", tc.ATT_S)
@pytest.mark.parametrize("causal", (0, 1))
def test_attention_bwd_model_passes(causal, S):
    top = 0.0
    for B, H in tc.ATT_BH:
        for regime in tc.ac.REGIMES:
            qkv, go, R = _att(B, S, H, regime, causal)
            for order in ORDERS:
                fails, worst = tc.att_failures(R, tc.att_model(qkv, go, B, S, H, causal, order), f"S{S}.c{causal}.{regime}.{order}")
                top = max(top, _inside(fails, worst, f"attention_bwd S {S} causal {causal} {regime}"))
    print(f"[model] attention_bwd S {S} causal {causal}: worst ratio {top:.3g}")


ATT_PLAN = [(m, c, S) for m in tc.ATT_MUTATIONS + ("drop_store_dQ", "drop_store_dK", "drop_store_dV") for c in (0, 1) for S in tc.ATT_S
            if tc.att_applicable(m, S, c)]                     # (where the mutation changes something)


@pytest.mark.parametrize("mutation,causal,S", ATT_PLAN)
def test_each_attention_bwd_mutation_misses_the_bound(mutation, causal, S):
    B, H = 2, 3
    tops = []
    for regime in tc.ac.REGIMES:
        qkv, go, R = _att(B, S, H, regime, causal)
        got = tc.att_model(qkv, go, B, S, H, causal, mutation=mutation, at=(B * S - 1, 5))
        tops.append(_factor(*tc.att_failures(R, got)))
    _best(mutation, tops, f"S {S} causal {causal}")


# ---- cross-attention core --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cross(B, K, H, regime):
    a = tc.cross_inputs(B, K, H, regime, seed=K)
    return a, tc.cross_reference(*a, B, K, H)


@pytest.mark.parametrize("K", tc.CROSS_K)
def test_cross_core_models_pass(K):
    top = 0.0
    for B, H in tc.CROSS_BH:
        for regime in tc.ac.REGIMES:
            a, R = _cross(B, K, H, regime)
            for order in ORDERS:
                fails, worst = tc.cross_failures(R, tc.cross_model(*a, B, K, H, order), f"K{K}.{regime}.{order}")
                top = max(top, _inside(fails, worst, f"cross_core K {K} {regime}"))
    print(f"[model] cross_core K {K}: worst ratio {top:.3g}")


# (one key: nothing to drop, and its neighbour is itself)
CROSS_PLAN = [(m, K) for m in tc.CROSS_MUTATIONS + tuple(f"drop_store_{n}" for n in ("out", "dQ", "dK", "dV")) for K in tc.CROSS_K
              if K > 1 or m not in tc.CROSS_MUTATIONS]


@pytest.mark.parametrize("mutation,K", CROSS_PLAN)
def test_each_cross_core_mutation_misses_the_bound(mutation, K):
    B, H = 3, 3
    tops = []
    for regime in tc.ac.REGIMES:
        a, R = _cross(B, K, H, regime)
        tops.append(_factor(*tc.cross_failures(R, tc.cross_model(*a, B, K, H, mutation=mutation, at=(B * (K if mutation[-2:] in ("dK", "dV") else 1) - 1, 7)))))
    _best(mutation, tops, f"K {K}")


# ---- LayerNorm with statistics and its backward ------------------------------------------------------------------------------------------
def _ln_cases(dim, rows_set=tc.LN_ROWS, regimes=tc.LN_REGIMES):
    for rows in rows_set:
        for regime in regimes:
            for ld in (dim, dim + 4):
                for mapped in (False, True):
                    for dyr in (tc.LN_DY if regime == "random" else ("random",)):
                        yield tc.LnBwdCase(rows, dim, ld, mapped, regime, dyr, seed=rows)


@pytest.mark.parametrize("dim", tc.LN_DIMS)
def test_layernorm_train_models_pass(dim):
    """forward (y and the statistics) and backward with the float64-exact statistics and with the forward model's, with and without
    the bf16 plane"""
    tf = tb = 0.0
    for case in _ln_cases(dim):
        xr = case.x[case.src, :dim]
        for order in ORDERS:
            y, st = tc.ln_fwd_model(xr, case.gamma, case.beta, order)
            tf = max(tf, _inside(*tc.ln_fwd_failures(xr, case.gamma, case.beta, y, st, case.name), "ln_fwd_stats " + case.name))
            for stats in (case.stats_exact, st):
                for with_bf in (True, False):
                    dx, dxb = tc.ln_bwd_model(case, stats, with_bf, order)
                    tb = max(tb, _inside(*tc.ln_bwd_failures(case, stats, dx, dxb), "ln_bwd " + case.name))
    print(f"[model] ln_fwd_stats dim {dim}: worst ratio {tf:.3g}; ln_bwd: {tb:.3g}")


def _lnb_applicable(mutation, rows, dim, ld, mapped):
    if mutation == "stats_row_plus1":
        return rows > 1
    if mutation in ("b_short", "drop_store_dx"):
        return dim > 1                                 # one column: xhat, b and the whole term are zero, dx keeps its value
    if mutation == "dx_dense":
        return ld > dim and (rows > 1 or mapped)
    return True


@pytest.mark.parametrize("dim", tc.LN_DIMS)
@pytest.mark.parametrize("mutation", tc.LNB_MUTATIONS + ("drop_store_dx", "drop_store_bf", "drop_store_y", "drop_store_stats"))
def test_each_layernorm_train_mutation_misses_the_bound(mutation, dim):
    for rows in tc.LN_ROWS:
        for ld in (dim, dim + 4):
            for mapped in (False, True):
                if not _lnb_applicable(mutation, rows, dim, ld, mapped):
                    continue
                tops = []
                for regime, dyr in (("random", "random"), ("rowscale", "random"), ("offset6", "random"), ("random", "parallel")):
                    case = tc.LnBwdCase(rows, dim, ld, mapped, regime, dyr, seed=rows)
                    at = (rows - 1, dim - 1)
                    if mutation in ("drop_store_y", "drop_store_stats"):
                        xr = case.x[case.src, :dim]
                        y, st = tc.ln_fwd_model(xr, case.gamma, case.beta, mutation=mutation, at=at)
                        tops.append(_factor(*tc.ln_fwd_failures(xr, case.gamma, case.beta, y, st)))
                    else:
                        dx, dxb = tc.ln_bwd_model(case, case.stats_exact, True, mutation=mutation, at=at)
                        tops.append(_factor(*tc.ln_bwd_failures(case, case.stats_exact, dx, dxb)))
                _best(mutation, tops, f"{rows}x{dim} ld {ld} map {mapped}")


# ---- the loss ------------------------------------------------------------------------------------------------------------------------
def _blocals(N):
    return sorted({1, math.ceil(N / 3), N})


@functools.lru_cache(maxsize=None)
def _loss(N, dim, regime, scale):
    img, txt = tc.loss_inputs(N, dim, regime, seed=N)
    return img, txt, tc.loss_reference(img, txt, N, scale)


def _loss_rows(R, B):
    return dict(R, dtxt=R["dtxt"][:B], e_dtxt=R["e_dtxt"][:B], m_dtxt=R["m_dtxt"][:B])


@pytest.mark.parametrize("N", tc.LOSS_N)
@pytest.mark.parametrize("dim", tc.LOSS_DIMS)
def test_clip_loss_model_passes(dim, N):
    """the model computes the gradient of all N rows once; every B_local of the table is a prefix of it"""
    top = 0.0
    for scale in tc.LOSS_SCALES:
        for regime in tc.LOSS_REGIMES:
            img, txt, R = _loss(N, dim, regime, scale)
            for order in ORDERS:
                loss, dt = tc.loss_model(img, txt, N, scale, order)
                for B in _blocals(N):
                    top = max(top, _inside(*tc.loss_failures(_loss_rows(R, B), loss, dt[:B], f"N{N}.B{B}.d{dim}.{regime}.s{scale}"), f"clip_loss N {N} dim {dim}"))
    print(f"[model] clip_loss N {N} dim {dim}: worst ratio {top:.3g}")


# (one row: its column is its row and the gradient is zero)
LOSS_PLAN = [(m, N) for m in tc.LOSS_MUTATIONS + ("drop_store_loss", "drop_store_dtxt") for N in tc.LOSS_N if N > 1 or m not in tc.LOSS_MUTATIONS]


@pytest.mark.parametrize("mutation,N", LOSS_PLAN)
def test_each_clip_loss_mutation_misses_the_bound(mutation, N):
    for dim in (4, 128):
        for B in _blocals(N):
            if mutation == "grad_over_blocal" and B == N:
                continue
            tops = []
            for scale in tc.LOSS_SCALES:
                for regime in tc.LOSS_REGIMES:
                    img, txt, R = _loss(N, dim, regime, scale)
                    loss, dt = tc.loss_model(img, txt, B, scale, mutation=mutation, at=(B - 1, dim - 1))
                    tops.append(_factor(*tc.loss_failures(_loss_rows(R, B), loss, dt)))
            _best(mutation, tops, f"N {N} B_local {B} dim {dim}")


# ---- l2norm_bwd, QuickGELU, AdamW ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", tc.L2_DIMS)
def test_l2norm_bwd_model_and_lost_store(dim):
    top = 0.0
    for rows in tc.L2_ROWS:
        tops = []
        for regime in tc.L2_REGIMES:
            x, dy = tc.l2b_inputs(rows, dim, regime, seed=rows)
            for order in ORDERS:
                top = max(top, _inside(*tc.l2b_failures(x, dy, tc.l2b_model(x, dy, order), f"{rows}x{dim}.{regime}"), f"l2norm_bwd {rows}x{dim} {regime}"))
            tops.append(_factor(*tc.l2b_failures(x, dy, tc.l2b_model(x, dy, mutation="drop_store", at=(rows - 1, dim - 1)))))
        _best("l2norm_bwd.drop_store", tops, f"{rows}x{dim}")
    print(f"[model] l2norm_bwd dim {dim}: worst ratio {top:.3g}")


def test_qgelu_models_and_lost_stores():
    u = tc.qgelu_values()
    assert u.numel() == 2 * (0x4200 + 1) + 2 and float(u.float().abs().max()) == 100.0
    dy = torch.randn(u.numel(), generator=torch.Generator().manual_seed(3)).bfloat16()
    y, du = tc.qgelu_model(u, dy)
    top = _inside(*tc.qgelu_failures(u, y, dy, du), "qgelu")
    print(f"[model] qgelu over every bf16 value in [-32, 32]: worst ratio {top:.3g}")
    at = int((u.float() == 1.0).nonzero()[0])
    for mutation in ("drop_store_y", "drop_store_du"):
        y, du = tc.qgelu_model(u, dy, mutation=mutation, at=at)
        _best("qgelu." + mutation, [_factor(*tc.qgelu_failures(u, y, dy, du))], "qgelu")


@pytest.mark.parametrize("step", (1, 2, 1000))
def test_adamw_model_and_mutations(step):
    top = 0.0
    for n in tc.FLAT_N:
        for gs in (1.0, 0.5):
            tops = {m: [] for m in tc.ADAMW_MUTATIONS + ("drop_store_p", "drop_store_m", "drop_store_v")}
            for regime in ("random", "zero_vg"):
                a = tc.adamw_inputs(n, regime, seed=step)
                R = tc.adamw_reference(*a, step, gs)
                top = max(top, _inside(*tc.adamw_failures(R, *tc.adamw_model(*a, step, gs), f"n{n}.{regime}.step{step}"), f"adamw n {n} {regime}"))
                for m in tops:
                    tops[m].append(_factor(*tc.adamw_failures(R, *tc.adamw_model(*a, step, gs, mutation=m, at=n - 1))))
            for m, t in tops.items():
                if m == "bc2_outside_root" and step == 1000:          # 1 - 0.98^1000 rounds to 1: inside or outside the root is the same
                    continue
                _best("adamw." + m, t, f"n {n} step {step}")
    print(f"[model] adamw step {step}: worst ratio {top:.3g}")


# ---- column sums, transpose, gather / scatter, dropout ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", tc.T_ROWS)
def test_colsum_model_and_mutations(rows):
    top = 0.0
    for cols in tc.T_COLS:
        for dt in (tc.F32, tc.BF):
            tops = {m: [] for m in tc.COLSUM_MUTATIONS + ("drop_store",)}
            for regime in ("integer", "random"):
                x = tc.matrix_data(rows, cols, regime, dt, seed=rows)
                prev = torch.randint(-4, 5, (cols,), generator=torch.Generator().manual_seed(cols)).float() + 16.0
                for pv in (None, prev):
                    for order in ORDERS:
                        top = max(top, _inside(*tc.colsum_failures(x, pv, tc.colsum_model(x, pv, order), regime == "integer", f"{rows}x{cols}.{regime}"), "colsum"))
                    for m in tops:
                        if (m == "accumulate_ignored" and pv is None) or (m == "wave3_missing" and rows < 4):
                            continue
                        tops[m].append(_factor(*tc.colsum_failures(x, pv, tc.colsum_model(x, pv, mutation=m, at=cols - 1), regime == "integer")))
            for m, t in tops.items():
                if t:
                    _best("colsum." + m, t, f"{rows}x{cols}")
    print(f"[model] colsum rows {rows}: worst ratio {top:.3g}")


def test_transpose_scatter_and_dropout_mutations_differ_in_bits():
    for rows in tc.T_ROWS:
        for cols in tc.T_COLS:
            x = tc.matrix_data(rows, cols, "specials", tc.F32, seed=rows)
            for ld_out in sorted({rows, rows + 1, -(-rows // 64) * 64}):
                want = tc.transpose_ref(x, ld_out)
                assert not tc.same_bits(tc.transpose_model(x, ld_out), want, "")
                for m in ("pad_not_zeroed", "drop_store"):
                    if m == "pad_not_zeroed" and ld_out == rows:
                        continue
                    f = tc.same_bits(tc.transpose_model(x, ld_out, m, at=(cols - 1, rows - 1)), want, m)
                    assert f and f.worst == float("inf"), (m, rows, cols, ld_out)
                    _note("transpose." + m, f.worst)
    src = torch.randn(3, 5)
    dst0 = torch.randn(8, 9)
    m = tc.gather_map(3, 8, 1)
    assert sorted(m.tolist())[0] == 0 and sorted(m.tolist())[-1] == 7 and len(set(m.tolist())) == 3
    plain, acc = tc.scatter_ref(src, m, dst0, 5, 0), tc.scatter_ref(src, m, dst0, 5, 1)
    assert tc.same_bits(plain, acc, "accumulate ignored") and torch.equal(plain[:, 5:], dst0[:, 5:]) and torch.equal(plain[m.long(), :5], src)
    # one lost store leaves the sentinel (or, accumulating, the old value): bits
    lost = acc.clone()
    lost[m.long()[0], 4] = dst0[m.long()[0], 4]
    assert tc.same_bits(lost, acc, "a lost scatter store")
    gathered = dst0[m.long(), :5].clone()
    lost = gathered.clone()
    lost[2, 4] = tc.SENT
    assert tc.same_bits(lost, gathered, "a lost gather store")
    z, mask, dy = tc.dropout_inputs(257, 1)
    for want in (tc.dropout_fwd_ref(z, mask, 1.25), tc.dropout_bwd_ref(dy, z, mask, 1.25), tc.dropout_bwd_ref(dy.bfloat16(), z, None, 1.0)):
        lost = want.clone()
        lost[256] = tc.SENT
        assert tc.same_value(lost, want, "a lost dropout_relu store")
    mk = tc.dropout_mask_ref(257, 7, 0.5)
    lost = mk.clone()
    lost[256] = 77
    assert tc.same_bits(lost, mk, "a lost mask store")
    assert {float(v) for v in tc.gate_values().float()} <= {float(v) for v in z.float()}
    assert tc.same_value(tc.dropout_bwd_ref(dy, z, mask, 1.25, mutation="gate_ge"), tc.dropout_bwd_ref(dy, z, mask, 1.25), "gate z >= 0")
    assert float(tc.dropout_fwd_ref(tc.gate_values(), None, 1.0).float()[4]) == 2.0 ** -133      # a subnormal pre-activation passes the gate


def test_dropout_mask_model():
    """the uint64 model: deterministic, seed-dependent, keep rates inside 5 binomial standard deviations, p = 0 keeps everything"""
    n = 2 ** 20 + 1
    for p in (0.0, 0.1, 0.5, 0.999):
        m = tc.dropout_mask_ref(n, 1234, p)
        assert tc.keep_rate_ratio(m, float(np.float32(p))) <= 1.0, p
    assert bool(tc.dropout_mask_ref(n, 1234, 0.0).all())
    assert not torch.equal(tc.dropout_mask_ref(4096, 1, 0.5), tc.dropout_mask_ref(4096, 2, 0.5))
    assert tc.keep_rate_ratio(tc.dropout_mask_ref(n, 1234, 0.1), 0.2) > 1.0


# ---- what the whole-tensor limits let through ----------------------------------------------------------------------------------------
def test_whole_tensor_limits_against_the_mutations():
    """the shapes and limits of test_building_blocks_against_torch: attention backward B = 2, S = 77, 2 heads, causal, rel-L2 < 1e-2;
    cross core K = 16, 5 x 8 heads, rel-L2 < 1e-2; LayerNorm backward 37 x 128, rel-L2 < 1e-4 of dx - 1; column sums 300 x 192,
    max-abs < 1e-4.  Every mutation below is caught per element; the whole-tensor number lets the listed ones through."""
    passed = {}
    B, S, H = 2, 77, 2
    qkv, go = tc.att_inputs(B, S, H, "random", seed=6)
    R = tc.att_reference(qkv, go, B, S, H, 1)
    for m in ("droplast", "delta_row_plus1", "drop_store_dQ", "drop_store_dV", "softmax_first64"):
        got = tc.att_model(qkv, go, B, S, H, 1, mutation=m, at=(100, 5))
        got = torch.where(got == tc.SENT, torch.zeros_like(got), got)                   # into a zeroed buffer
        r = gc.rel_l2(got, R[0])
        top = _factor(*tc.att_failures(R, got))
        print(f"[whole-tensor] attention_bwd {m}: rel_l2 {r:.3e} (limit 1e-2), per element {top:.3g} x the bound")
        passed[m] = r < 1e-2
        assert top >= FACTOR, m
    assert passed["droplast"] and passed["drop_store_dQ"] and passed["drop_store_dV"]
    Bq, K, Hh = 5, 16, 8
    a = tc.cross_inputs(Bq, K, Hh, "random", seed=8)
    Rc = tc.cross_reference(*a, Bq, K, Hh)
    for m in ("droplast", "drop_store_dK", "drop_store_out"):
        got = tc.cross_model(*a, Bq, K, Hh, mutation=m, at=(3, 7))
        got = {n: torch.where(t == tc.SENT, torch.zeros_like(t), t) for n, t in got.items()}
        r = max(gc.rel_l2(got[n], Rc[n][0]) for n in got)
        top = _factor(*tc.cross_failures(Rc, got))
        print(f"[whole-tensor] cross_core {m}: rel_l2 {r:.3e} (limit 1e-2), per element {top:.3g} x the bound")
        passed["cross." + m] = r < 1e-2
        assert top >= FACTOR, m
    assert passed["cross.drop_store_dK"]
    case = tc.LnBwdCase(37, 128, 128, False, "random", "random", seed=2)
    case.dx0 = torch.ones_like(case.dx0)
    ref, _ = tc.ln_bwd_reference(case, case.stats_exact)
    for m in ("b_short", "drop_store_dx"):
        dx, _ = tc.ln_bwd_model(case, case.stats_exact, False, mutation=m, at=(20, 100))
        r = gc.rel_l2(dx - 1.0, ref - 1.0)
        top = _factor(*tc.ln_bwd_failures(case, case.stats_exact, dx, None))
        print(f"[whole-tensor] ln_bwd {m}: rel_l2 {r:.3e} (limit 1e-4), per element {top:.3g} x the bound")
        passed["ln." + m] = r < 1e-4
        assert top >= FACTOR, m
    x = tc.matrix_data(300, 192, "random", tc.F32, seed=1)
    got = tc.colsum_model(x, None, mutation="wave3_missing")
    d = float((got.double() - x.double().sum(0)).abs().max())
    print(f"[whole-tensor] colsum wave3_missing: max_abs {d:.3e} (limit 1e-4)")
    assert d > 1e-4                                                                     # (this one the old limit does catch)
