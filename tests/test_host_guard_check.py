"""Proof, on the CPU, that the guard sweeps (tests/guard_check.py) decide what they claim to decide: the grey zones hold the kernel's
own fp32 evaluation, the planted targets land on their side, every defect family of every kernel form skips at least one planted
position (and which pairing alone would still do so, should a sweep have to be trimmed to one) -- and that the single positions the
suite planted before (the last row, column 5 or 3) miss most of them, listed in the report."""
import numpy as np
import pytest
import torch

from oracle import keds_oracle as O
from tests import gemm_check as gc
from tests import guard_check as gd
from tests.conftest import golden_path
from tests.gpu_util import report

TINY = dict(embed_dim=128, image_resolution=56, vision_layers=2, vision_width=128, vision_patch_size=14,
            context_length=77, vocab_size=512, transformer_width=128, transformer_layers=2)
KS = (128, 512, 2048)


def _kernel_rho32(stats, K, order):
    """the kernel's fp32 evaluation (ln_row_coeff) of |nmr| in three orders a compiler may pick: as written, with the subtraction
    contracted into an fma, with 1 / K folded into a division"""
    s = (stats[:, 0].double() / gc.STAT_SCALE).float()
    ss = (stats[:, 1].double() / gc.STAT_SCALE).float()
    invk = torch.tensor(1.0 / K, dtype=torch.float32)
    if order == "division":
        mean, q = s / K, ss / K
    else:
        mean, q = s * invk, ss * invk
    if order == "fma":
        var = (q.double() - mean.double() * mean.double()).float().clamp_min(0.0)      # one rounding
    else:
        var = (q - mean * mean).clamp_min(0.0)
    rstd = torch.rsqrt(var + torch.tensor(gc.LN_EPS, dtype=torch.float32))
    return (-mean * rstd).abs()


@pytest.mark.parametrize("K", KS)
def test_ratio_zone_holds_the_kernels_fp32_evaluation(K):
    """rho swept densely through [31, 33] at variances from 1e-4 to 1e4: outside the grey zone the fp32 evaluation, in every order,
    decides as the float64 model does; the move of the fp32 rho stays below the derived worst case."""
    msgs, worst = [], 0.0
    for var in (1e-4, 1.0, 37.0, 1e4):
        rhos = torch.linspace(31.0, 33.0, 4001, dtype=torch.float64).tolist()
        stats = torch.tensor([gd.plant_stats(K, r, sign=-1 if i % 2 else 1, var=var) for i, r in enumerate(rhos)], dtype=torch.int64)
        want = gd.ratio_rows(stats, K)
        rho64 = gd.rho_of(stats, K)
        for order in ("written", "fma", "division"):
            got = _kernel_rho32(stats, K, order)
            raised = ~(got <= gd.RATIO_LIMIT)
            bad = ((want == 1) & ~raised) | ((want == -1) & raised)
            if bool(bad.any()):
                msgs.append(f"var {var} {order}: {int(bad.sum())} rows outside the zone decided otherwise")
            worst = max(worst, float(((got.double() - rho64).abs() / rho64).max()))
        assert int((want == 0).sum()) > 0 and int((want == 1).sum()) > 1000 and int((want == -1).sum()) > 1000
    report(f"guard_check.ratio_zone.K{K}", worst_relative_move=worst, derived_worst=gd.ratio_rounding_worst(), zone=gd.RATIO_ZONE)
    assert not msgs, "\n".join(msgs)
    assert worst <= gd.ratio_rounding_worst()


@pytest.mark.parametrize("K", KS)
def test_planted_ratio_targets_land_on_their_side(K):
    for var in (1.0, 0.01):
        for sign in (1, -1):
            assert gd.ratio_expect(torch.tensor([gd.plant_stats(K, 33.0, sign, var)]), K) == gd.MUST
            assert gd.ratio_expect(torch.tensor([gd.plant_stats(K, 31.0, sign, var)]), K) == gd.MUST_NOT
            assert gd.ratio_expect(torch.tensor([gd.plant_stats(K, 1000.0, sign, var)]), K) == gd.MUST
    assert gd.ratio_expect(torch.tensor([gd.plant_stats(K, 32.0)]), K) == gd.EITHER
    # extreme fixed-point values, by the same formula: a negative sum of squares is variance 0
    one = int(gc.STAT_SCALE)
    assert gd.ratio_expect(torch.tensor([[0, -5 * K * one]]), K) == gd.MUST_NOT                  # mean 0: rho 0
    assert gd.ratio_expect(torch.tensor([[K * one, -5 * K * one]]), K) == gd.MUST                # mean 1, var 0: rho 316
    assert gd.ratio_expect(torch.tensor([[gd.INT64_MAX, 0]]), K) == gd.MUST
    assert gd.ratio_expect(torch.tensor([[gd.INT64_MIN, gd.INT64_MAX]]), K) == gd.MUST
    assert gd.ratio_expect(torch.tensor([[0, gd.INT64_MAX]]), K) == gd.MUST_NOT
    # the launch is the combination of its rows
    rows = torch.tensor([gd.plant_stats(K, 31.0), gd.plant_stats(K, 32.0), gd.plant_stats(K, 2.0)])
    assert gd.ratio_expect(rows, K) == gd.EITHER and gd.ratio_expect(rows[[0, 2]], K) == gd.MUST_NOT
    assert gd.ratio_expect(torch.cat([rows, torch.tensor([gd.plant_stats(K, 33.0)])]), K) == gd.MUST
    # nmr_stats: the coefficient the range sweep asks for
    s = torch.tensor([gd.nmr_stats(K, -20.0)], dtype=torch.int64)
    c = gd.stack_case(gc.Case(1, 128, K, "random", gc.HF, seed=3), [0], stats=s)
    assert abs(float(-c.mean[0, 0] * c.rstd[0, 0]) + 20.0) < 1e-6


def test_planted_range_targets_land_on_their_side():
    """the side-input planting of the LayerNorm forms (nmr = -20, csum = +-3500 / +-3000) and the operand planting of the plain ones:
    7e4 MUST, 6e4 MUST_NOT, 65510 EITHER, by the float64 reference and gemm_check's bound"""
    K, N = 128, 256
    case = gc.Case(4, N, K, "random", gc.HF, seed=5)
    flat = torch.tensor([[0, K * int(gc.STAT_SCALE)]] * 4, dtype=torch.int64)                      # mean exactly 0, variance 1
    base = gd.stack_case(case, [0, 1, 2, 3], stats=flat)
    for code in (16, 17):
        assert gd.range_expect(gc.expected(base, code)) == gd.MUST_NOT
        for target, want in ((3500.0, gd.MUST), (-3500.0, gd.MUST if code == 16 else gd.MUST_NOT), (3000.0, gd.MUST_NOT),
                             (-3000.0, gd.MUST_NOT), (65510.0 / 20.0, gd.EITHER)):
            csum = case.csum.clone().repeat(1, 1)
            csum[0, 77] = -target                                                                  # v = nmr csum = +20 target
            st = torch.tensor([gd.nmr_stats(K, -20.0)], dtype=torch.int64)
            exp = gc.expected(gd.stack_case(case, [2], stats=st, csum=csum), code)
            assert abs(float(exp.ref[0, 77]) - (20 * target if code == 16 or target > 0 else 0.0)) < 40.0
            assert float(exp.bound.max()) < 50.0
            assert gd.range_expect(exp) == want, (code, target)
    W = case.W
    for target, want in ((7e4, gd.MUST), (6e4, gd.MUST_NOT)):
        scale = target / float(W[9].double().abs().sum())
        A = (torch.sign(W[9].float()) * scale).half().unsqueeze(0)
        exp = gc.expected(gd.stack_case(case, [1], A=A), 20)
        assert abs(float(exp.ref[0, 9]) - target) < 100.0
        assert gd.range_expect(exp) == want
    assert gd.combine([gd.MUST_NOT, gd.EITHER]) == gd.EITHER and gd.combine([gd.EITHER, gd.MUST]) == gd.MUST
    assert gd.combine([gd.MUST_NOT, gd.MUST_NOT]) == gd.MUST_NOT


def test_x3_and_split_expectations():
    B, S, d = 2, 33, 128
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(B * S, 3 * d, generator=g)
    assert gd.x3_expect(qkv, B, S, d) == gd.MUST_NOT
    for col, val, want in ((3, 4.0e5, gd.MUST_NOT), (3, 5.3e5, gd.MUST), (d + 3, 6.5e4, gd.MUST_NOT), (d + 3, 7e4, gd.MUST),
                           (2 * d + 63, -7e4, gd.MUST), (2 * d, float("nan"), gd.MUST), (0, float("-inf"), gd.MUST),
                           (d, 65504.0, gd.MUST), (0, 8 * 65504.0, gd.MUST), (0, 8 * 65503.0, gd.MUST_NOT)):
        x = qkv.clone()
        x[S + 5, col] = val
        assert gd.x3_expect(x, B, S, d) == want, (col, val)
    x = qkv.clone()
    x[S + 5, 3] = 5.3e5                                      # a q row the launch does not compute: no claim; k and v are read whatever
    assert gd.x3_expect(x, B, S, d, q_limit=1) == gd.EITHER
    x[S, 3] = 5.3e5
    assert gd.x3_expect(x, B, S, d, q_limit=1) == gd.MUST
    x = qkv.clone()
    x[S + 5, d + 3] = 7e4
    assert gd.x3_expect(x, B, S, d, q_limit=1) == gd.MUST
    off = torch.tensor([0, 20, 53])
    x = torch.cat([qkv[:53], torch.full((8, 3 * d), float("nan"))])
    assert gd.x3_expect(x, 2, 33, d, seq_off=off) == gd.MUST_NOT                 # guard rows behind the packed rows are not the operand
    x[52, 2 * d + 4] = float("inf")
    assert gd.x3_expect(x, 2, 33, d, seq_off=off) == gd.MUST
    y = torch.randn(7, 16, generator=g)
    assert gd.split_expect(y) == gd.MUST_NOT
    for val, want in ((65504.0, gd.MUST), (-65504.0, gd.MUST), (65503.99609375, gd.MUST_NOT), (7e4, gd.MUST), (float("nan"), gd.MUST)):
        z = y.clone()
        z[6, 15] = val
        assert gd.split_expect(z) == want, val


def test_tile_walk_covers_every_tile_once():
    for mt, nt, wg in ((96, 4, 256), (257, 1, 256), (32, 16, 256), (65, 8, 256), (36, 4, 96), (9, 3, 8)):
        walk = gd.tile_walk(mt, nt, wg)
        assert sorted(w[:2] for w in walk) == [(m, n) for m in range(mt) for n in range(nt)]
        assert sum(w[3] for w in walk) == min(wg, mt * nt)                      # every workgroup has exactly one last tile
        assert max(w[2] for w in walk) == (mt * nt - 1) // wg


def test_every_defect_family_skips_a_planted_position():
    """for every kernel form and both guards: no defect instance survives the sweep (the ratio sweep plants every row of its tiles
    and has no pairing).  One pairing alone ties row bits to column bits -- c = 5 r + 3 never meets 8 of the 32 (H, p, mi) stores of
    a lane -- so what each pairing alone would let through is reported: a sweep is only ever trimmed to a pairing that lets nothing
    through.  The positions planted before this module (the last row of the
    launch, column 5 for the LayerNorm forms, column 3 for the plain ones) are held against the same families and what they miss is
    reported."""
    total, old_missed, lines = 0, 0, []
    for name, form in gd.FORMS.items():
        M, N, K, row0 = gd.sweep_shape(name)
        for guard in ("ratio", "range"):
            fams = gd.families_of(guard, form)
            assert fams, (name, guard)
            planted = gd.sweep_positions(name, guard)
            assert gd.missed(guard, form, planted) == [], (name, guard)
            assert all(row0 <= o.m < M and 0 <= o.n < N for o in planted)
            if guard == "range":
                alone = [len(gd.missed(guard, form, gd.sweep_positions(name, guard, pairings=(w,)))) for w in (0, 1)]
                lines.append(f"{name}.{guard}: defect instances let through by pairing 0 alone: {alone[0]}, by pairing 1 alone: {alone[1]}")
                assert min(alone) == 0, (name, alone)
            n_inst = sum(len(list(f[2])) for f in fams.values())
            # the ratio guard had no planted position at kernel level at all; the range guard one per launch
            old = [] if guard == "ratio" else [gd.owner(form, M - 1, c, 0, row0) for c in (5, 3)]
            miss = gd.missed(guard, form, old)
            total += n_inst
            old_missed += len(miss)
            lines.append(f"{name}.{guard}: {len(miss)} of {n_inst} defect instances missed by the single positions: "
                         + ", ".join(sorted({m[0] for m in miss})))
    report("guard_check.coverage", defect_instances=total, missed_by_single_positions=old_missed, per_form=lines)
    assert old_missed > total // 2, "the single positions were expected to miss most defect instances"


def test_sweep_tiles_reach_the_second_round_and_the_last_tile_of_a_walk():
    for name in ("quad4.persistent", "quad4.persistent.defer"):
        for guard in ("ratio", "range"):
            tiles = gd.sweep_tiles(name, guard)
            M, N, K, _ = gd.sweep_shape(name)
            assert tiles[0] == (0, 0, 0) and any(t[2] == 1 for t in tiles) and len(tiles) >= 3
            assert (M // 256 - 1, 0 if guard == "ratio" else N // 256 - 1) in [t[:2] for t in tiles]
            assert guard != "ratio" or all(t[1] == 0 for t in tiles)
    deferred = [o for o in gd.sweep_positions("quad4.persistent.defer", "range") if o.deferred]
    assert deferred and all(16 * o.half + 8 * o.p + o.mi >= 14 for o in deferred)
    # every one of a lane's 32 stores s = 16 H + 8 p + mi is planted, the 14 issued ones and the 18 kept ones
    stores = {16 * o.half + 8 * o.p + o.mi for o in gd.sweep_positions("quad4.persistent.defer", "range")}
    assert stores == set(range(32)) and len({s for s in stores if s >= 32 - gd.ND}) == gd.ND


# ---- the float64 tower model against the oracle ----------------------------------------------------------------------------------
def test_tower64_is_the_oracles_tower():
    """guard_check.Tower64 (the pass-level tests' float64 model, which also sees pad rows) computes what the oracle's towers compute"""
    g = dict(np.load(golden_path("clip_tiny.npz")))
    sd = O.synth_clip_state_dict(**TINY, seed=7)
    img = torch.from_numpy(g["image"])
    x, bounds = gd.image_rows64(sd, img)
    tw = gd.Tower64(sd, "visual.transformer.", heads=2)
    y = tw.run(x, gd.attend_samples(bounds, 2, causal=False))
    S = bounds[0][1]
    cls = y.reshape(len(bounds), S, -1)[:, 0]
    feats = gd._ln64(cls, sd["visual.ln_post.weight"].double(), sd["visual.ln_post.bias"].double()) @ sd["visual.proj"].double()
    want = O.encode_image(sd, img)
    assert float((feats - want.double()).norm() / want.double().norm()) < 1e-5
    assert len(tw.ratios) == 4 and max(float(r.max()) for r in tw.ratios) < 4.0
    text = torch.from_numpy(g["text"])
    x, bounds = gd.text_rows64(sd, text)
    tt = gd.Tower64(sd, "transformer.", heads=2)
    stream = tt.run(x, gd.attend_samples(bounds, 2, causal=True))
    y = gd._ln64(stream, sd["ln_final.weight"].double(), sd["ln_final.bias"].double()).reshape(text.shape[0], text.shape[1], -1)
    eot = (text == TINY["vocab_size"] - 1).to(torch.int32).argmax(dim=1)
    feats = y[torch.arange(text.shape[0]), eot] @ sd["text_projection"].double()
    want = O.encode_text(sd, text)
    assert float((feats - want.double()).norm() / want.double().norm()) < 1e-5
    # packed rows: the same valid rows (causal attention never looks behind a sample's read-out row), pad rows carried along
    lengths = (eot + 1).tolist()
    xp, bp = gd.text_rows64(sd, text, lengths, pad_rows=5)
    yp = tt.run(xp, gd.attend_samples(bp, 2, causal=True))
    assert yp.shape[0] == sum(lengths) + 5
    for (a, e), (ra, _) in zip(bp, bounds):
        assert torch.allclose(yp[a:e], stream[ra:ra + e - a], atol=1e-9, rtol=0)


# ---- the packed pass keeps its zero rows away from the guard ---------------------------------------------------------------------
@pytest.mark.parametrize("flow", ("bf16", "fp16"))
def test_packed_plan_rezeroes_the_zero_rows_behind_every_residual_gemm(flow):
    """keds_tower_plan_query: in a packed folded pass with zero rows behind the captions, every residual GEMM that adds statistics
    carries bound = packed_valid ([20] of its record: the rows of its output and of those statistics from there on are zeroed behind
    the launch), so that every LayerNorm-folded GEMM reads statistics whose zero rows are zero.  No other step carries it, and no
    step of a pass without zero rows, of a rectangular pass or of the fp32 / fp32x3 flows."""
    from tests.test_host_tower_plan import BUF, OPNAME, query
    M, valid, layers = 512, 257, 3
    steps = query(flow, 256, 4, 77, True, layers, 7, "readout", packed=(M, valid), lane=1)[0]
    marked = [s for s in steps if s["bound"] and OPNAME[s["op"]] != "gather"]
    assert [(s["layer"], s["weight"]) for s in marked] == [(0, 2), (0, 4), (1, 2), (1, 4)]          # out_proj and c_proj of blocks 0, 1
    for s in marked:
        assert OPNAME[s["op"]] == "gemm" and s["bound"] == valid and BUF[s["out"]] == "h" and s["out_r0"] + s["n"] == M
        assert BUF[s["st_add"]] in ("st1", "st2")
    dirty = set()                                       # statistics buffers whose zero rows a residual GEMM has written
    reads = 0
    for s in steps:
        name = OPNAME[s["op"]]
        if name == "stats_cast":
            dirty.discard(BUF[s["st_add"]])             # written from x, whose zero rows are zero
        elif name == "gemm":
            if s["st_read"] and s["in_r0"] + s["n"] > valid:
                assert BUF[s["st_read"]] not in dirty, f"layer {s['layer']} weight {s['weight']} judges rows no caption owns"
                reads += 1
            if s["st_clear"]:
                dirty.discard(BUF[s["st_clear"]])
            if s["st_add"] and s["out_r0"] + s["n"] > valid and s["bound"] != valid:
                dirty.add(BUF[s["st_add"]])
    assert reads == 2 * layers - 1
    others = [query(flow, 256, 4, 77, True, layers, 7, "readout", packed=(512, 512), lane=1)[0],
              query(flow, 256, 4, 77, True, layers, 7, "readout", lane=1)[0],
              query("x3", 256, 4, 77, True, layers, 7, "readout", packed=(M, valid), lane=1)[0],
              query("f32", 256, 4, 77, True, layers, 7, "readout", packed=(M, valid), lane=1)[0]]
    for plan in others:
        assert not [s for s in plan if s["bound"] and OPNAME[s["op"]] != "gather"]
