"""What each numerics guard MUST, MUST NOT or MAY do for a launch, per row and per element (keds_hip.h: keds_numerics_guard_set, the
fp16 range guard of the *_F16_H epilogues, the overflow flags of keds_attention_x3 and keds_split_f16_pair); where to plant a
trigger so that every lane, wave, store and launch that has to look is made to look at least once; and the defect families those
positions are chosen against (tests/test_host_guard_check.py proves the coverage on the CPU, tests/test_gpu_guard_edges.py runs
the launches).  Plain torch; imports without a GPU.

Expectations are computed in float64 from what the kernel READS, never from what it returns.

Ratio guard (guard_check / ln_row_coeff / ln_coeff_from in csrc/gemm_shared.h, gemm.hip).  From the int64 statistics {s, ss} of a row
(fixed point, 2^28) and the GEMM's K:
    mean = s / 2^28 / K,   var = max(ss / 2^28 / K - mean^2, 0),   rho = |mean| / sqrt(var + 1e-5);   the flag rises when rho > 32.
The kernel evaluates this in fp32 (gemm_check's LayerNorm paragraph, u32 = 2^-24): mean carries 3 u32 relative, q = ss / K 3 u32,
mean^2 7 u32, the subtraction one more, so |d var| <= E = (3 q + 7 mean^2 + var) u32.  With var = q - mean^2 and rho^2 ~ mean^2 / var
that is d var / var <= (4 + 10 rho^2) u32; rsqrt adds U_FN = 2^-20 and two roundings, the product -mean rstd 4 u32:
    d rho / rho <= (2 + 5 rho^2) u32 + 2^-20 + 6 u32  =  3.1e-4 at rho = 32
(the typical figure -- the two roundings of q and mean^2 alone -- is 1.5 u32 (1 + rho^2) = 0.9e-4).  The grey zone is
RATIO_ZONE = 2^-10 = 9.8e-4 relative on either side of 32, three times the worst case: MUST at rho >= 32 (1 + 2^-10), MUST_NOT at
rho <= 32 (1 - 2^-10), EITHER between.  The planted targets, rho = 33 and rho = 31, are 3 % away.

Range guard (f16_range_flag).  From gemm_check's float64 reference v of every output and its per-element bound e (accumulation,
epilogue and output rounding: |stored - v| <= e): MUST when some |v| - e >= 65520 -- the fp32 value is then beyond 65504 whatever
the kernel's rounding, and fp16 stores inf; MUST_NOT when every |v| + e <= 65504; EITHER between.  Planted targets: +-7e4 and +-6e4
(e is below 50 there, asserted per launch).

keds_attention_x3 (keds_hip.h): MUST when an element the launch reads has |q / 8|, |k| or |v| >= 65504 or is not finite (the / 8 is
exact); MUST_NOT when every element of the [rows, 3 d] operand is inside.  A q row at or behind q_limit is EITHER: the header does
not say whether the kernel looks at queries it does not compute.  keds_split_f16_pair: MUST at |x| >= 65504 or non-finite inside
[rows, cols], MUST_NOT otherwise (the stride gap is not read).

Positions.  Two pairings of the rows and columns of a tile, c = (5 r + 3) mod T and c = (93 r + 128) mod T (T = 256, or 128 on the
128^2 forms: both are bijections, every row and every column of the tile is hit once per pairing), applied in the first tile, the
last tile and, on the persistent kernel, in the first tile of the second round and in the last tile a workgroup walks (tile_walk
models xcd_remap and quad_tile_coords of keds_common.h).

Defect families (FAMILIES): predicates over the owner of a position -- the lane map gemm.hip documents, lane (g, c) of wave
(wm, wn) owns rows 64 / 128 wm + 16 mi + c and columns 64 wn + 32 p + 8 g + j -- that say `a guard with this defect does not look
here`.  A one-hot launch planted at a position a defect skips comes back with the flag down where the model says MUST.

Pass level (tests/test_gpu_guard_passes.py): Tower64 walks a tower of the oracle's state dict in float64 and records the
|mean| / std of every row at every LayerNorm input and the largest |x| of the residual stream; text_rows64 lays the text tower's
rows out rectangular or packed, zero rows included, for the conditions the pad-row test asserts before anything runs on the GPU."""
import collections

import torch

from tests import gemm_check as gc

MUST, MUST_NOT, EITHER = "MUST", "MUST_NOT", "EITHER"
RATIO_LIMIT = 32.0
RATIO_ZONE = 2.0 ** -10
F16_MAX = 65504.0
F16_INF_FROM = 65520.0                  # the first fp32 value fp16 rounds to inf (65504 + half an ulp of 32)
INT64_MAX, INT64_MIN = 2 ** 63 - 1, -2 ** 63
ND = 18                                 # quad_nd(): deferred stores per lane of the persistent LayerNorm epilogue


def ratio_rounding_worst(rho=RATIO_LIMIT):
    """the derived worst relative move of the kernel's fp32 rho (module docstring)"""
    return (2 + 5 * rho * rho) * gc.U32 + gc.U_FN + 6 * gc.U32


assert 3 * ratio_rounding_worst() < RATIO_ZONE


def combine(expectations):
    """a launch of several rows / elements / guards: one MUST raises it, it stays down only if everything MUST_NOT"""
    expectations = list(expectations)
    if MUST in expectations:
        return MUST
    return MUST_NOT if all(e == MUST_NOT for e in expectations) else EITHER


# ---- ratio guard -----------------------------------------------------------------------------------------------------------------
def rho_of(stats, K):
    """stats int64 [..., 2] -> rho float64 [...]: the formula of the module docstring on the integers the kernel reads"""
    sf = stats.double() / gc.STAT_SCALE
    mean = sf[..., 0] / K
    var = (sf[..., 1] / K - mean.square()).clamp_min(0.0)
    return mean.abs() / (var + gc.LN_EPS).sqrt()


def ratio_rows(stats, K):
    """per row: +1 MUST, -1 MUST_NOT, 0 EITHER (int8 tensor)"""
    rho = rho_of(stats, K)
    out = torch.zeros(rho.shape, dtype=torch.int8, device=rho.device)
    out[rho >= RATIO_LIMIT * (1 + RATIO_ZONE)] = 1
    out[rho <= RATIO_LIMIT * (1 - RATIO_ZONE)] = -1
    out[~torch.isfinite(rho)] = 1                                   # (cannot happen from int64 input; kept for completeness)
    return out


def ratio_expect(stats, K):
    rows = ratio_rows(stats, K)
    return MUST if bool((rows == 1).any()) else MUST_NOT if bool((rows == -1).all()) else EITHER


def plant_stats(K, rho, sign=1, var=1.0):
    """(s, ss) fixed-point integers of a row with variance `var` and |mean| / sqrt(var + eps) = rho"""
    mean = sign * rho * (var + gc.LN_EPS) ** 0.5
    return int(round(mean * K * gc.STAT_SCALE)), int(round((var + mean * mean) * K * gc.STAT_SCALE))


def nmr_stats(K, nmr, var=1.0):
    """(s, ss) of a row whose LayerNorm coefficient -mean rstd is `nmr` at variance `var` (the range guard's side-input planting)"""
    return plant_stats(K, abs(nmr), sign=-1 if nmr > 0 else 1, var=var)


# ---- range guard -----------------------------------------------------------------------------------------------------------------
def range_rows(exp):
    """gemm_check.Expected -> per row: +1 MUST, -1 MUST_NOT, 0 EITHER"""
    a = exp.ref.abs()
    bad = ~torch.isfinite(exp.ref)
    must = (((a - exp.bound) >= F16_INF_FROM) | bad).any(dim=1)
    safe = (((a + exp.bound) <= F16_MAX) & ~bad).all(dim=1)
    out = torch.zeros(a.shape[0], dtype=torch.int8, device=a.device)
    out[safe] = -1
    out[must] = 1
    return out


def range_expect(exp):
    rows = range_rows(exp)
    return MUST if bool((rows == 1).any()) else MUST_NOT if bool((rows == -1).all()) else EITHER


# ---- the fp16 stream's own check (keds_f16_stream_bad) -----------------------------------------------------------------------------
# The writers of the fp16 residual stream test a partial sum of squares of the fp32 values they store against 65504^2: 64 aligned
# columns of a row in the GEMM epilogues (8 in the split-K reduce kernel, a lane's values in keds_rowstats_cast_ex -- subsets of
# them).  MUST: some stored value has |v| - e >= 65520 or is not finite (its square alone is beyond the limit).  MUST_NOT: every
# aligned 64-column partial of (|v| + e)^2 stays below 65504^2 (1 - 2^-16) -- the fp32 sum of 64 squares is within 65 2^-24 of the
# exact one.  EITHER between: the widened contract of keds_hip.h, a partial at the limit without a value beyond the range.
STREAM_LIMIT = F16_MAX * F16_MAX
STREAM_SAFE = STREAM_LIMIT * (1 - 2.0 ** -16)


def stream_partials(exp, group=64):
    """gemm_check.Expected -> the largest aligned `group`-column partial of (|v| + e)^2 per row, float64 [rows]"""
    hi = (exp.ref.abs() + exp.bound).square()
    hi = torch.where(torch.isfinite(hi), hi, torch.full_like(hi, float("inf")))
    pad = (-hi.shape[1]) % group
    return torch.nn.functional.pad(hi, (0, pad)).reshape(hi.shape[0], -1, group).sum(-1).max(dim=1).values


def stream_rows(exp, group=64):
    """per row: +1 MUST, -1 MUST_NOT, 0 EITHER"""
    bad = ~torch.isfinite(exp.ref)
    must = (((exp.ref.abs() - exp.bound) >= F16_INF_FROM) | bad).any(dim=1)
    safe = stream_partials(exp, group) < STREAM_SAFE
    out = torch.zeros(exp.ref.shape[0], dtype=torch.int8, device=exp.ref.device)
    out[safe & ~must] = -1
    out[must] = 1
    return out


def stream_expect_values(x, group):
    """x fp32 [rows, dim] read exactly (keds_rowstats_cast_ex: no arithmetic before the square); group: the columns one lane holds,
    as index lists -- conservatively, MUST_NOT asks the whole ROW's sum of squares below the limit"""
    v = x.double()
    if bool((~torch.isfinite(v) | (v.abs() > F16_MAX)).any()):
        return MUST
    return MUST_NOT if bool((v.square().sum(1) < STREAM_SAFE).all()) else EITHER


def code_of(v):
    return {1: MUST, -1: MUST_NOT, 0: EITHER}[int(v)]


def stack_case(case, rows, stats=None, csum=None, A=None):
    """A gemm_check case whose row i is row rows[i] of launch i: the planted row of each of P one-hot launches, judged in one pass.
    stats int64 [P, 2]: that launch's statistics of the row; csum fp32 [P, N] or [N]: that launch's column sums; A [P, K]: that
    launch's operand row (the accumulators are then recomputed).  Shares nothing it writes with `case`."""
    c = gc.Case.__new__(gc.Case)
    idx = torch.as_tensor(rows, device=case.device)
    c.dtype, c.device, c.regime, c.tile_k = case.dtype, case.device, "operands", case.tile_k
    c.M, c.N, c.K = len(rows), case.N, case.K
    c.name = f"{case.name}.stack{len(rows)}"
    c.W, c.bias, c.pos = case.W, case.bias, None
    if A is None:
        c.A, c.acc, c.S = case.A[idx], case.acc[idx], case.S[idx]
    else:
        c.A = A
        c.acc = A.double() @ case.W.double().t()
        c.S = A.double().abs() @ case.W.double().abs().t()
    c.resid = None if case.resid is None else case.resid[idx]
    st = case.stats[idx] if stats is None else stats
    c.stats = st
    c.csum = case.csum if csum is None else csum
    sf = st.double() / gc.STAT_SCALE
    c.mean = sf[:, :1] / c.K
    c.q = (sf[:, 1:] / c.K).abs()                              # (a negative sum of squares: the error terms by its size)
    c.var = (sf[:, 1:] / c.K - c.mean.square()).clamp_min(0.0)
    c.rstd = (c.var + gc.LN_EPS).rsqrt()
    c._e_acc = None
    return c


# ---- keds_attention_x3 / keds_split_f16_pair -------------------------------------------------------------------------------------
def _outside(x, limit=F16_MAX):
    return ~(x.abs() < limit)                                    # NaN and inf are outside


def x3_expect(qkv, B, S, d, q_limit=0, seq_off=None):
    """qkv fp32 [rows, 3 d] (rows = B S, or the packed rows of seq_off) -> MUST / MUST_NOT / EITHER.  q rows at or behind q_limit
    (q_limit > 0) make no claim."""
    rows = B * S if seq_off is None else int(seq_off[-1])
    x = qkv[:rows].double()
    q, kv = x[:, :d] / 8.0, x[:, d:]
    if bool(_outside(kv).any()):
        return MUST
    qbad = _outside(q).any(dim=1)
    if q_limit > 0 and seq_off is None:
        computed = (torch.arange(rows, device=x.device) % S) < q_limit
        if bool((qbad & computed).any()):
            return MUST
        return EITHER if bool(qbad.any()) else MUST_NOT
    return MUST if bool(qbad.any()) else MUST_NOT


def split_expect(x):
    """x fp32 [rows, cols] (the part keds_split_f16_pair is told to read)"""
    return MUST if bool(_outside(x.double()).any()) else MUST_NOT


# ---- kernel forms, owners, positions ---------------------------------------------------------------------------------------------
# kernel: which epilogue code runs -- "small" (128^2, tile_epilogue<4>), "reduce" (split-K: one thread per 8 outputs of a row),
# "pair" (8 waves, 2 x 4, pair_ln_epilogue / tile_epilogue<8>), "quad" (4 waves, 2 x 2, each wave two 64-column halves h)
Form = collections.namedtuple("Form", "name tile kernel persistent defer remainder")
FORMS = {f.name: f for f in (
    Form("small4", 128, "small", False, False, False),
    Form("small4.strided", 128, "small", False, False, False),
    Form("small2", 128, "small", False, False, False),
    Form("splitk", 128, "reduce", False, False, False),
    Form("pair8", 256, "pair", False, False, False),
    Form("quad4", 256, "quad", False, False, False),
    Form("quad4.persistent", 256, "quad", True, False, False),
    Form("quad4.persistent.defer", 256, "quad", True, True, False),
    Form("remainder", 128, "small", False, False, True),
    # the fp16-residual epilogues' own forms (codes 9 / 18): residual tile + bias as the accumulators' initial value; three-deep A ring
    Form("pair8.prologue", 256, "pair", False, False, False),
    Form("quad3", 256, "quad", False, False, False),
)}
LN_FORMS = tuple(n for n in FORMS if n not in ("pair8.prologue", "quad3"))                      # what a LayerNorm-folded epilogue reaches
STREAM_FORMS = tuple(n for n in FORMS if not FORMS[n].persistent)                               # what an fp16-residual epilogue reaches

# a planted position and who owns it.  m, n: output element; tile = (tm, tn) and r, col inside it; round: which tile of its
# workgroup's walk (0 unless persistent); wm, wn: wave row / column; mi, c, p, g, j: the lane map; half: the 128-column half of the
# 8-wave kernel's tile (wn >> 1) or the wave's 64-column half H of the 4-wave kernel; deferred: a store the persistent kernel keeps for
# the next K-loop; rwave: the wave whose thread r computes row r's coefficients in the 256^2 prologues (r >> 6)
Owner = collections.namedtuple("Owner", "m n tile r col round wm wn mi c p g j half deferred rwave remainder reduce")


def owner(form, m, n, round_=0, row0=0):
    """row0: the first row of the launch the position is in (the remainder launch numbers its tiles from there)"""
    T = form.tile
    r, col = (m - row0) % T, n % T
    tile = ((m - row0) // T, n // T)
    rows_per_wave = 64 if T == 128 else 128
    wm, mi, c = r // rows_per_wave, (r % rows_per_wave) // 16, r % 16
    p, g, j = (col % 64) // 32, (col % 32) // 8, col % 8
    if form.kernel == "quad":
        wn, half = col // 128, (col % 128) // 64
    else:
        wn, half = col // 64, col // 128
    deferred = bool(form.defer and 16 * half + 8 * p + mi >= 32 - ND)
    return Owner(m, n, tile, r, col, round_, wm, wn, mi, c, p, g, j, half, deferred, r // 64, form.remainder, form.kernel == "reduce")


def pairing(which, T):
    """row -> column of pairing 0 / 1 inside a tile of T"""
    a, b = ((5, 3), (93, 128))[which]
    return [(a * r + b) % T for r in range(T)]


def xcd_remap(bid, nwg):
    q, r, x = nwg >> 3, nwg & 7, bid & 7
    base = x * (q + 1) if x < r else r * (q + 1) + (x - r) * q
    return base + (bid >> 3)


def quad_tile_coords(bid, m_tiles, n_tiles):
    m8 = m_tiles & ~7
    if m8 and n_tiles % 4 == 0 and bid < m8 * n_tiles:
        grp, within = bid >> 5, bid & 31
        grows = m8 >> 3
        gn = grp // grows
        gm = grp - gn * grows
        return gm * 8 + (within & 7), gn * 4 + (within >> 3)
    if m8 and n_tiles % 4 == 0:
        r = bid - m8 * n_tiles
        tm = m8 + r // n_tiles
        return tm, r - (tm - m8) * n_tiles
    return bid // n_tiles, bid % n_tiles


def tile_walk(m_tiles, n_tiles, workgroups):
    """persistent 4-wave kernel: id -> (tm, tn, round, last of its workgroup's walk)"""
    nt = m_tiles * n_tiles
    return [quad_tile_coords(xcd_remap(i, nt), m_tiles, n_tiles) + (i // workgroups, i + workgroups >= nt) for i in range(nt)]


def tiles_to_plant(form, M, N, workgroups=None, col0_only=False):
    """[(tm, tn, round)]: the first tile, the last tile and, persistent, the first tile of the second round and the last tile of
    all (the last one its workgroup walks, behind at least one other).  col0_only (the ratio guard: the tile column that checks):
    tn = 0 throughout."""
    T = form.tile
    mt, nt = (M + T - 1) // T, N // T
    if not form.persistent:
        tiles = [(0, 0, 0), (mt - 1, 0 if col0_only else nt - 1, 0)]
    else:
        walk = tile_walk(mt, nt, workgroups)
        ok = [w for w in walk if w[1] == 0] if col0_only else walk
        first = next(w for w in ok if w[2] == 0)
        second = next(w for w in ok if w[2] == 1)
        last = next(w for w in reversed(ok) if w[2] >= 1 and w[3])
        corner = next(w for w in ok if w[0] == mt - 1 and (col0_only or w[1] == nt - 1))
        tiles = [first[:3], corner[:3], second[:3], last[:3]]
    out = []
    for t in tiles:
        if t not in out:
            out.append(t)
    return out


def positions(form, M, N, tiles, pairings=(0, 1), row0=0):
    """the Owners of both pairings in the given tiles (rows of a ragged last tile that do not exist are left out)"""
    T = form.tile
    out = []
    for tm, tn, rnd in tiles:
        for which in pairings:
            cols = pairing(which, T)
            for r in range(T):
                m = row0 + tm * T + r
                if m < M:
                    out.append(owner(form, m, tn * T + cols[r], rnd, row0))
    return out


def row_positions(form, M, tiles, row0=0):
    """the ratio guard: every row of the given tiles, judged where the checking lane sits (column 0 of the launch)"""
    T = form.tile
    return [owner(form, row0 + tm * T + r, 0, rnd, row0) for tm, tn, rnd in tiles for r in range(T) if row0 + tm * T + r < M]


def sweep_shape(name, threshold=256):
    """(M, N, K, row0) of the guard sweeps of form `name`: the smallest launch whose forced form is that form (gemm_plan.h: 256^2
    tiles need 128 of them, 218 with remainder rows behind; split-K needs K >= 2048 on at most 64 tiles; the two-deep ring more than
    256 tiles; deferral eight K-tiles).  threshold: tiles beyond which the 4-wave kernel goes persistent (min(CUs, 256) & ~7).
    row0: the first row of the launch under test (the remainder launch's)."""
    ragged = (threshold + threshold // 2) // 4 * 256                 # test_gpu_gemm_edges: a ragged second round, supertiles of 8 x 4
    return {"small4": (256, 256, 128, 0), "small4.strided": (256, 256, 128, 0), "small2": (2176, 2048, 128, 0),
            "splitk": (256, 256, 2048, 0), "pair8": (2048, 4096, 128, 0), "quad4": (2048, 4096, 128, 0),
            "quad4.persistent": (ragged, 1024, 128, 0), "quad4.persistent.defer": (ragged, 1024, 512, 0),
            "remainder": (3584 + 129, 4096, 128, 3584), "pair8.prologue": (2048, 4096, 128, 0), "quad3": (2048, 4096, 1024, 0)}[name]


def sweep_tiles(name, guard, threshold=256):
    """the tiles the sweep of (form, guard) plants in -- in the remainder form: of the remainder launch"""
    form = FORMS[name]
    M, N, K, row0 = sweep_shape(name, threshold)
    return tiles_to_plant(form, M - row0, N, threshold, col0_only=guard == "ratio")


def sweep_positions(name, guard, threshold=256, pairings=(0, 1)):
    form = FORMS[name]
    M, N, K, row0 = sweep_shape(name, threshold)
    tiles = sweep_tiles(name, guard, threshold)
    return row_positions(form, M, tiles, row0) if guard == "ratio" else positions(form, M, N, tiles, pairings, row0)


# ---- defect families -------------------------------------------------------------------------------------------------------------
# name -> (guards it applies to, forms it applies to (kernel kinds, or a predicate over the Form), the instances k, predicate(owner, k))
def _all(_form):
    return True


def _is(*kinds):
    return lambda form: form.kernel in kinds


FAMILIES = {
    # the ratio guard's lane per row: tile_epilogue (small) checks per (wm, mi, c); the 256^2 prologues per thread r of wave r >> 6
    "ratio.wave_row": (("ratio",), _is("small"), (0, 1), lambda o, k: o.wm == k),
    "ratio.mi": (("ratio",), _is("small"), range(4), lambda o, k: o.mi == k),
    "ratio.c": (("ratio",), _is("small"), range(16), lambda o, k: o.c == k),
    "ratio.prologue_wave": (("ratio",), _is("pair", "quad"), range(4), lambda o, k: o.rwave == k),
    "ratio.prologue_lane": (("ratio",), _is("pair", "quad"), range(64), lambda o, k: o.r % 64 == k),
    "ratio.reduce_n0_lane": (("ratio",), _is("reduce"), (0,), lambda o, k: o.reduce),
    # the range guard looks at every stored element
    "range.wave_row": (("range",), _is("small", "pair", "quad"), (0, 1), lambda o, k: o.wm == k),
    "range.wave_col": (("range",), _is("small", "quad"), (0, 1), lambda o, k: o.wn == k),
    "range.wave_col8": (("range",), _is("pair"), range(4), lambda o, k: o.wn == k),
    "range.half_of_8_wave_tile": (("range",), _is("pair"), (0, 1), lambda o, k: o.half == k),
    "range.half_of_4_wave_wave": (("range",), _is("quad"), (0, 1), lambda o, k: o.half == k),
    "range.mi": (("range",), _is("small"), range(4), lambda o, k: o.mi == k),
    "range.mi8": (("range",), _is("pair", "quad"), range(8), lambda o, k: o.mi == k),
    "range.c": (("range",), _is("small", "pair", "quad"), range(16), lambda o, k: o.c == k),
    "range.p": (("range",), _is("small", "pair", "quad"), (0, 1), lambda o, k: o.p == k),
    "range.g": (("range",), _is("small", "pair", "quad"), range(4), lambda o, k: o.g == k),
    "range.j": (("range",), _all, range(8), lambda o, k: o.j == k),
    "range.rmax_reset_between_p": (("range",), lambda f: f.kernel in ("pair", "quad") and not f.persistent, (0,), lambda o, k: o.p == 0),
    "range.deferred_stores": (("range",), lambda f: f.defer, (0,), lambda o, k: o.deferred),
    "range.issued_stores": (("range",), lambda f: f.defer, (0,), lambda o, k: not o.deferred),
    "range.store_index": (("range",), lambda f: f.defer, range(32), lambda o, k: 16 * o.half + 8 * o.p + o.mi == k),
    # both
    "rows_ge_128": (("ratio", "range"), _is("pair", "quad"), (0,), lambda o, k: o.r >= 128),
    "rows_lt_128": (("ratio", "range"), _is("pair", "quad"), (0,), lambda o, k: o.r < 128),
    "not_the_first_tile_of_a_workgroup": (("ratio", "range"), lambda f: f.persistent, (0,), lambda o, k: o.round > 0),
    "not_the_first_tile_of_the_launch": (("ratio", "range"), _all, (0,), lambda o, k: o.tile != (0, 0)),
    "remainder_launch": (("ratio", "range"), lambda f: f.remainder, (0,), lambda o, k: o.remainder),
}


def families_of(guard, form):
    return {name: f for name, f in FAMILIES.items() if guard in f[0] and f[1](form)}


def missed(guard, form, planted):
    """[(family, k)] of every defect instance that skips NONE of the planted positions: a guard with that defect passes the sweep"""
    out = []
    for name, (_, _, ks, pred) in families_of(guard, form).items():
        for k in ks:
            if not any(pred(o, k) for o in planted):
                out.append((name, k))
    return out


# ---- pass level: the oracle's towers in float64 ----------------------------------------------------------------------------------
def _ln64(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = (x - mu).square().mean(-1, keepdim=True)
    return (x - mu) / (var + gc.LN_EPS).sqrt() * w + b


def _ratio64(x):
    mu = x.mean(-1)
    var = (x - mu.unsqueeze(-1)).square().mean(-1)
    return mu.abs() / (var + gc.LN_EPS).sqrt()


class Tower64:
    """float64 model of one transformer tower of the state dict `sd` (prefix "visual.transformer." or "transformer."): the residual
    stream x [rows, width] through every block, `attend(q, k, v) -> o` supplied by the caller (it knows which rows form a sample).
    Records, per LayerNorm input (two per block, in order), the |mean| / std of every row, and the largest |x| of the stream."""

    def __init__(self, sd, prefix, heads):
        self.p = {k[len(prefix):]: v.double() for k, v in sd.items() if k.startswith(prefix)}
        self.layers = 1 + max(int(k.split(".")[1]) for k in self.p if k.startswith("resblocks."))
        self.heads = heads
        self.ratios, self.max_abs = [], 0.0

    def run(self, x, attend):
        self.ratios, self.max_abs = [], float(x.abs().max())
        for i in range(self.layers):
            g = lambda name: self.p[f"resblocks.{i}.{name}"]                   # noqa: E731
            self.ratios.append(_ratio64(x))
            h = _ln64(x, g("ln_1.weight"), g("ln_1.bias"))
            qkv = h @ g("attn.in_proj_weight").t() + g("attn.in_proj_bias")
            q, k, v = qkv.chunk(3, dim=-1)
            x = x + attend(q, k, v) @ g("attn.out_proj.weight").t() + g("attn.out_proj.bias")
            self.max_abs = max(self.max_abs, float(x.abs().max()))
            self.ratios.append(_ratio64(x))
            h = _ln64(x, g("ln_2.weight"), g("ln_2.bias"))
            h = h @ g("mlp.c_fc.weight").t() + g("mlp.c_fc.bias")
            h = h * torch.sigmoid(1.702 * h)
            x = x + h @ g("mlp.c_proj.weight").t() + g("mlp.c_proj.bias")
            self.max_abs = max(self.max_abs, float(x.abs().max()))
        return x


def attend_samples(bounds, heads, causal):
    """attention over samples given as row ranges [(a, b)]; rows outside every range (pad rows) attend to nothing: their output is 0,
    as the packed pass leaves its zeroed attention buffer"""
    def attend(q, k, v):
        o = torch.zeros_like(q)
        hd = q.shape[-1] // heads
        for a, b in bounds:
            L = b - a
            qh, kh, vh = (t[a:b].reshape(L, heads, hd).transpose(0, 1) for t in (q, k, v))
            s = qh @ kh.transpose(-1, -2) / hd ** 0.5
            if causal:
                s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float("-inf"))
            o[a:b] = (torch.softmax(s, -1) @ vh).transpose(0, 1).reshape(L, heads * hd)
        return o
    return attend


def text_rows64(sd, tokens, lengths=None, pad_rows=0):
    """the text tower's input rows in float64: token + positional embedding.  lengths None: rectangular, [B * ctx, width] and the
    sample bounds; else packed, sample b's first lengths[b] rows back to back, followed by `pad_rows` rows of zeros."""
    emb, pos = sd["token_embedding.weight"].double(), sd["positional_embedding"].double()
    B, ctx = tokens.shape
    x = emb[tokens.long()] + pos[:ctx]
    if lengths is None:
        return x.reshape(B * ctx, -1), [(b * ctx, (b + 1) * ctx) for b in range(B)]
    rows, bounds, at = [], [], 0
    for b in range(B):
        L = int(lengths[b])
        rows.append(x[b, :L])
        bounds.append((at, at + L))
        at += L
    rows.append(torch.zeros(pad_rows, x.shape[-1], dtype=torch.float64))
    return torch.cat(rows), bounds


def image_rows64(sd, image):
    """the image tower's rows behind ln_pre in float64 -> ([B * S, width], sample bounds)"""
    w = sd["visual.conv1.weight"].double()
    x = torch.nn.functional.conv2d(image.double(), w, stride=w.shape[-1])
    B, C = x.shape[:2]
    x = x.reshape(B, C, -1).transpose(1, 2)
    cls = sd["visual.class_embedding"].double().expand(B, 1, C)
    x = torch.cat([cls, x], 1) + sd["visual.positional_embedding"].double()
    x = _ln64(x, sd["visual.ln_pre.weight"].double(), sd["visual.ln_pre.bias"].double())
    S = x.shape[1]
    return x.reshape(B * S, C), [(b * S, (b + 1) * S) for b in range(B)]
