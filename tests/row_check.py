"""Per-ELEMENT checks of the row kernels of keds_amd/csrc/elementwise.hip -- what sits between the GEMMs and the attention in every
tower pass: LayerNorm in all its forms, row statistics, the LayerNorm fold, casts, gathers, token embedding, normalisation.  The shape
of tests/gemm_check.py: seeded cases in regimes made for the defects these kernels can have, a float64 reference on the fp32 inputs,
a bound per element derived from the arithmetic, and float32 CPU models of the kernels with deliberate mutations
(tests/test_host_row_check.py proves that the checks pass the models and catch every mutation).  Plain torch; imports without a GPU;
every function works on the device its inputs are on.  No constant here was tuned on a kernel's output.

u = 2^-24.  Output rounding as in gemm_check: bound = e (1 + 2 u_out) + u_out |ref| + t + 2^-126 (u_out 2^-8 bf16, 2^-11 fp16 with
t = 2^-25, 2^-24 fp32); a pair of fp16 planes is held as X3_QGELU_PAIR is: hi + lo within e (1 + 2 u_out) + 2^-22 |ref| + 2^-25 + 2^-126
and |lo| <= ulp_fp16(hi) / 2 per element.

LayerNorm (layernorm_kernel<OUT, NV>, layernorm_pair_stream_kernel<NJ>), per row, L = dim / 64 + 8 (a lane's addition chain, the six
butterfly steps, the division and the subtraction):
    mu = mean x, d = x - mu, var = mean d^2, r = (var + 1e-5)^-1/2,    ref = d r gamma + beta
    dmu = L u mean |x|
    dd  = dmu + u |d|
    dv  = 2 mean(|d| dd) + mean(dd^2) + (L + 4) u var
    dr  = dv / (2 (var + 1e-5)) + 2^-20                  (relative; 2^-20: the project's allowance for v_rsq_f32)
    e   = |gamma| r (dd + |d| (dr + 3 u)) + u |beta|
A row whose map entry lies outside [0, row_mul) must be NaN in every element.
Regimes (LN_REGIMES): random N(0, 1) 3 + 0.5;  offset6 N(0, 1) +- 6 (sign per row);  offset1k N(0, 1) + 1024 (a one-pass variance is
gross);  constant_exact 3.0 with small-integer gamma, beta (the output IS beta: torch.equal);  constant 3.3 (held to the bound);  spike
random with one column x 4096;  tiny random x 2^-20 (var << eps);  huge N(0, 1) 2^20 + 2^22;  rowscale random with row r x 2^6 when
(r / g) % 2 == 1, g the gather group or the stream kernel's wave count (a neighbour's or a stale row's statistics are gross).

Row statistics (rowstats_cast_kernel): the 16-bit copy equals x.to(dtype) bit for bit; {sum x, sum x^2} through gemm_check.check_stats
against the float64 sums of the fp32 input; exact in the `integer` regime (small integers and, in every row, one 2049 -- no 16-bit
type holds it, so the squares of the rounded copy are another integer).

LayerNorm fold (fold_layernorm_kernel): the float64 product of two fp32 values is exact, so per element wf is T(fl32(w gamma)) or
T(w gamma) -- one or two roundings, both are the specification (fold_check counts which occurs); csum against the float64 sum of the wf
the launch STORED within (K / 64 + 8) u sum |wf|; bias' against bias + sum w beta within (K / 64 + 9) u (sum |w beta| + |bias|).
`integer` regime: torch.equal (gamma holds 683 in places: 3 x 683 = 2049, so the unrounded products sum to another integer).

Casts, gathers, cls_rows, embed_tokens, im2col: bit for bit against torch casts and indexing (a copy, one rounding or one addition).

l2_normalize / mix_normalize, L = ceil(dim / 64) + 8:   e_l2 = |ref| (L / 2 + 3) u;   mixture m = wa a^ + wb b^:
    e_m = |wa| e_l2(a) + |wb| e_l2(b) + 2 u (|wa a^| + |wb b^|),     e = e_m / |m| + |ref| (<|m|, e_m> / |m|^2 + (L / 2 + 3) u)
An all-zero row gives a NaN row."""
import math

import torch

from tests import gemm_check as gc
from tests.gemm_check import Expected, Failures, _collect, check, check_bits, check_stats, fp16_ulp  # noqa: F401  (re-exported)

U = gc.U32
U_RSQ = gc.U_FN
LN_EPS = gc.LN_EPS
BF, HF, F32 = gc.BF, gc.HF, gc.F32
SENT = gc.SENTINEL
LN_DIMS = (128, 256, 512, 768, 1024, 1280, 2048)
LN_REGIMES = ("random", "offset6", "offset1k", "constant_exact", "constant", "spike", "tiny", "huge")
NORM_DIMS = (1, 4, 63, 64, 65, 128, 640, 768, 1000)
L2_REGIMES = ("random", "small", "large")                      # x 1, x 2^-40, x 2^40
MIX_REGIMES = ("random", "opposed", "weighted")
LN_MUTATIONS = ("gamma_chunk", "stats_short", "one_pass_var", "rstd_row_plus1", "drop_store")
GATHER_MUTATIONS = ("row_map_plus1", "gather_modulo")
STREAM_MUTATIONS = ("stale_regs", "skip_last_trip")
PAIR_MUTATIONS = ("lo_zero", "lo_of_rounded")
TYPE_NAME = {BF: "bf16", HF: "fp16", F32: "fp32"}
OUT_CODE = {BF: 0, F32: 1, HF: 2}                              # out_type / src_type / dst_type of the C entry points


def _gen(*key, device="cpu"):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator(device=device).manual_seed(s)


def _str_seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------
class LnCase:
    """x fp32 [rows, dim], gamma, beta fp32 [dim] (drawn on `device`); exact: the output is beta to the bit"""

    def __init__(self, rows, dim, regime, seed=0, group=1, device="cpu"):
        assert regime in LN_REGIMES + ("rowscale",)
        kw = dict(generator=_gen(seed, rows, dim, _str_seed(regime), group, device=device), device=device)      # (seeded per device type)
        n = torch.randn(rows, dim, dtype=torch.float64, **kw)
        if regime in ("random", "spike", "tiny", "rowscale"):
            x = n * 3.0 + 0.5
            if regime == "spike":
                x[:, int(torch.randint(0, dim, (1,), **kw))] *= 4096.0
            elif regime == "tiny":
                x = x * 2.0 ** -20
            elif regime == "rowscale":
                x = torch.where(((torch.arange(rows, device=device) // group) % 2 == 1).unsqueeze(1), x * 64.0, x)
        elif regime == "offset6":
            x = n + torch.where(torch.rand(rows, 1, dtype=torch.float64, **kw) < 0.5, -6.0, 6.0)
        elif regime == "offset1k":
            x = n + 1024.0
        elif regime == "huge":
            x = n * 2.0 ** 20 + 2.0 ** 22
        else:
            x = torch.full((rows, dim), 3.0 if regime == "constant_exact" else 3.3, dtype=torch.float64, device=device)
        if regime == "constant_exact":
            gamma = torch.randint(-3, 4, (dim,), **kw).double()
            beta = torch.randint(-4, 5, (dim,), **kw).double()
        else:
            gamma = 1.0 + 0.5 * torch.randn(dim, dtype=torch.float64, **kw)
            beta = 0.5 * torch.randn(dim, dtype=torch.float64, **kw)
        self.rows, self.dim, self.regime, self.group = rows, dim, regime, group
        self.exact = regime == "constant_exact"
        self.x, self.gamma, self.beta = x.float(), gamma.float(), beta.float()
        self.name = f"{rows}x{dim}.{regime}" + (f".g{group}" if regime == "rowscale" else "")
        self._ref = None

    def ref(self):
        """(ref, e) float64 [rows, dim] of every SOURCE row, computed once"""
        if self._ref is None:
            self._ref = ln_reference(self.x, self.gamma, self.beta)
        return self._ref


def ln_reference(x, gamma, beta):
    """-> (ref, e) float64: the reference and the error bound before the output rounding (module docstring)"""
    dim = x.shape[1]
    L = dim / 64 + 8
    x, g, b = x.double(), gamma.double(), beta.double()
    mu = x.mean(1, keepdim=True)
    d = x - mu
    var = d.square().mean(1, keepdim=True)
    r = (var + LN_EPS).rsqrt()
    dmu = L * U * x.abs().mean(1, keepdim=True)
    dd = dmu + U * d.abs()
    dv = 2 * (d.abs() * dd).mean(1, keepdim=True) + dd.square().mean(1, keepdim=True) + (L + 4) * U * var
    dr = 0.5 * dv / (var + LN_EPS) + U_RSQ
    e = g.abs() * r * (dd + d.abs() * (dr + 3 * U)) + U * b.abs()
    return d * r * g + b, e


def gather_sources(rows, row_map, row_mul, mutation=None):
    """-> (src int64 [rows]: the source row of output row r; bad bool [rows]: rows that must be NaN).  row_map: int tensor or None."""
    r = torch.arange(rows, device=row_map.device if row_map is not None else "cpu")
    if row_map is None:
        return r * row_mul, torch.zeros(rows, dtype=torch.bool, device=r.device)
    rm = row_map.long()
    if mutation == "row_map_plus1":
        rm = torch.roll(rm, -1)
    if mutation == "gather_modulo":
        rm = rm % row_mul
    bad = (rm < 0) | (rm >= row_mul)
    return r * row_mul + torch.where(bad, torch.zeros_like(rm), rm), bad


def ln_failures(case, res, out_dtype, src=None, bad=None, what=""):
    """every check of one LayerNorm launch: res = dict(out=[rows, dim]) or dict(hi=, lo=) for the pair form -> (failing Failures, worst
    ratio to the bound over the rows that hold numbers)"""
    ref, e = case.ref()
    if src is not None:
        ref, e = ref[src], e[src]
    pair = "hi" in res
    tag = f"{what}{case.name}.{'pair' if pair else TYPE_NAME[out_dtype]}"
    good = torch.ones(ref.shape[0], dtype=torch.bool, device=ref.device) if bad is None else ~bad
    exp = Expected(ref[good], e[good], HF if pair else out_dtype, False, pair=pair)
    if pair:
        hi, lo = res["hi"].double(), res["lo"].double()
        got = hi + lo
        fs = [check(got[good], exp, tag + " hi + lo"), _collect(lo[good].abs() / (0.5 * fp16_ulp(hi[good])), tag + " |lo| against ulp(hi) / 2")]
    else:
        got = res["out"].double()
        fs = [check(got[good], exp, tag)]
    worst = fs[0].worst
    if case.exact:
        want = case.beta.double().expand_as(ref)[good]
        fs.append(_collect(torch.where(got[good] == want, 0.0, float("inf")).double(), tag + " (bits: the output is beta)"))
        if pair:
            fs.append(_collect(torch.where(lo[good] == 0, 0.0, float("inf")).double(), tag + " (bits: lo is zero)"))
    if bad is not None and bool(bad.any()):
        fs.append(_collect(torch.where(torch.isnan(got[bad]), 0.0, float("inf")).double(), tag + " (rows outside their sequence must be NaN)"))
    return [f for f in fs if f], worst


# float32 models of the two kernels ------------------------------------------------------------------------------------------------
def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def _fma(a, b, c):
    """fl32(a b + c) for fp32 tensors: the product is exact in float64, the sum rounded to 53 bits and then to 24"""
    return (a.double() * b.double() + c.double()).float()


def _lanes(t, width):
    """[rows, dim] -> [rows, J, 64, width], zero padded: lane l of trip j holds columns j 64 width + l width ..."""
    rows, dim = t.shape
    per = 64 * width
    pad = (-dim) % per
    return torch.nn.functional.pad(t, (0, pad)).reshape(rows, -1, 64, width)


def _lane_sum(t, order, sq=False, fma=False):
    """a lane's chain: s += (t0 + t1) + (t2 + t3) per group of four (of squares: sq), trips forwards or reversed -> [rows, 64]"""
    rows, J, _, W = t.shape
    s = torch.zeros(rows, 64)
    groups = [(j, h) for j in range(J) for h in range(W // 4)]
    for j, h in (groups if order == "forward" else reversed(groups)):
        c = t[:, j, :, 4 * h:4 * h + 4]
        if not sq:
            s = s + ((c[..., 0] + c[..., 1]) + (c[..., 2] + c[..., 3]))
        elif fma:
            s = s + (_fma(c[..., 0], c[..., 0], c[..., 1] * c[..., 1]) + _fma(c[..., 2], c[..., 2], c[..., 3] * c[..., 3]))
        else:
            s = s + ((c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + (c[..., 2] * c[..., 2] + c[..., 3] * c[..., 3]))
    return s


def _butterfly(s, steps):
    """xor butterfly over the 64 lanes (every lane ends with the same sum) -> [rows, 1]"""
    lane = torch.arange(64)
    for o in steps:
        s = s + s[:, lane ^ o]
    return s[:, :1]


def ln_model(x, gamma, beta, out, form="row", order="forward", fma=False, bad=None, mutation=None, at=None, nw=None):
    """The kernels in float32 (CPU).  x [rows, dim]: the SOURCE rows already gathered; out: a torch dtype or "pair"; form "row"
    (layernorm_kernel: 4-column chunks per lane, butterfly 32 .. 1, mean by division) or "stream" (layernorm_pair_stream_kernel: runs of
    8 columns, butterfly 1 .. 32, mean by multiplication with fl(1 / dim), a wave walks rows r, r + nw, ...); order: the lane's chain
    and the butterfly forwards or reversed; fma: the compiler may contract a multiply and the addition behind it; rsqrt is correctly
    rounded.  mutation: one of LN_MUTATIONS / STREAM_MUTATIONS / PAIR_MUTATIONS, at = dict(row=, col=) for drop_store."""
    rows, dim = x.shape
    width = 4 if form == "row" else 8
    steps = (32, 16, 8, 4, 2, 1) if form == "row" else (1, 2, 4, 8, 16, 32)
    steps = steps if order == "forward" else steps[::-1]
    x = x.float()
    if mutation == "stale_regs":                      # row r is normalised and written from the registers that hold row r + nw
        r = torch.arange(rows)
        x = x[torch.where(r + nw < rows, r + nw, r)]
    keep = torch.ones(dim, dtype=torch.bool)
    if mutation == "stats_short":
        keep[dim - 4:] = False
    xs = torch.where(keep, x, torch.zeros_like(x))
    dimf = _f32(float(dim))
    total = _butterfly(_lane_sum(_lanes(xs, width), order), steps)
    mean = total / dimf if form == "row" else total * (_f32(1.0) / dimf)
    d = x - mean
    if mutation == "one_pass_var":
        q = _butterfly(_lane_sum(_lanes(xs, width), order, sq=True, fma=fma), steps)
        var = q / dimf - mean * mean
    else:
        q = _butterfly(_lane_sum(_lanes(torch.where(keep, d, torch.zeros_like(d)), width), order, sq=True, fma=fma), steps)
        var = q / dimf if form == "row" else q * (_f32(1.0) / dimf)
    rstd = (var.double() + float(_f32(LN_EPS))).float()
    rstd = rstd.double().rsqrt().float()
    if mutation == "rstd_row_plus1":
        rstd = torch.roll(rstd, -1, 0)
    if bad is not None:
        rstd = torch.where(bad.unsqueeze(1), torch.full_like(rstd, float("nan")), rstd)
    g, b = gamma.float(), beta.float()
    if mutation == "gamma_chunk":                     # the 16-byte chunk behind
        g, b = torch.roll(g, -4), torch.roll(b, -4)
    t = d * rstd
    y = _fma(t, g.expand_as(t), b.expand_as(t)) if fma else t * g + b
    skip = None
    if mutation == "skip_last_trip":                  # a wave that walks several rows leaves without its last one
        r = torch.arange(rows)
        skip = (r + nw >= rows) & (r >= nw)
    at = dict(row=0, col=0) | (at or {})
    if out == "pair":
        hi = y.half()
        lo = (y - hi.float()).half()
        if mutation == "lo_zero":
            lo = torch.zeros_like(lo)
        if mutation == "lo_of_rounded":               # the remainder taken on the ROUNDED y
            lo = (y.half().float() - hi.float()).half()
        if mutation == "drop_store":
            c = at["col"] // 8 * 8
            hi[at["row"], c:c + 8] = SENT
        if skip is not None:
            hi[skip], lo[skip] = SENT, SENT
        return {"hi": hi, "lo": lo}
    o = y.to(out)
    if mutation == "drop_store":
        n = 16 // o.element_size()
        c = at["col"] // n * n
        o[at["row"], c:c + n] = SENT
    if skip is not None:
        o[skip] = SENT
    return {"out": o}


# ---- row statistics --------------------------------------------------------------------------------------------------------------
def stats_data(rows, dim, regime, seed=0, device="cpu"):
    """x fp32 [rows, dim]: `random`, or `integer`: values in [-3, 3] and one 2049 per row (sums and squares exact in fp32 in any order)"""
    g = _gen(seed, rows, dim, _str_seed(regime), 7)
    if regime == "integer":
        x = torch.randint(-3, 4, (rows, dim), generator=g).float()
        x[torch.arange(rows), torch.randint(0, dim, (rows,), generator=g)] = 2049.0
        assert float(x.square().sum(1).max()) < 2.0 ** 24
    else:
        x = (torch.randn(rows, dim, generator=g, dtype=torch.float64) * 3.0 + 0.5).float()
    return x.to(device)


def stats_failures(x, copy, stats, dtype, exact, what=""):
    """copy [rows, dim] of `dtype` and stats int64 [rows, 2] of one rowstats launch on x"""
    want = x.to(dtype)
    same = (copy == want) | (torch.isnan(copy) & torch.isnan(want))
    fs = [_collect(torch.where(same, 0.0, float("inf")).double(), what + " copy != x.to(dtype)"), check_stats(stats, x.double(), None, exact, what)]
    return [f for f in fs if f], fs[1].worst


def stats_model(x, dtype, order="forward", fma=False, mutation=None):
    """rowstats_cast_kernel in float32: eight chunks of four columns per lane (zeros behind dim), butterfly 32 .. 1"""
    x = x.float()
    copy = x.to(dtype)
    steps = (32, 16, 8, 4, 2, 1) if order == "forward" else (1, 2, 4, 8, 16, 32)
    s = _butterfly(_lane_sum(_lanes(x, 4), order), steps)
    xq = copy.float() if mutation == "sq_of_rounded" else x
    q = _butterfly(_lane_sum(_lanes(xq, 4), order, sq=True, fma=fma), steps)
    return copy, torch.cat([gc._fixed(s), gc._fixed(q)], 1)


# ---- LayerNorm fold --------------------------------------------------------------------------------------------------------------
class FoldCase:
    """W fp32 [N, K], bias fp32 [N], gamma, beta fp32 [K]"""

    def __init__(self, N, K, regime, seed=0, device="cpu"):
        g = _gen(seed, N, K, _str_seed(regime), 11)
        if regime == "integer":
            W = torch.randint(-3, 4, (N, K), generator=g).float()
            gamma = torch.randint(1, 4, (K,), generator=g).float()
            gamma[::5] = 683.0                        # 3 x 683 = 2049: no 16-bit type holds it
            beta = torch.randint(-4, 5, (K,), generator=g).float()
            bias = torch.randint(-8, 9, (N,), generator=g).float()
            assert 3 * 683 * K < 2 ** 24
        else:
            W = (torch.randn(N, K, generator=g, dtype=torch.float64) * K ** -0.5).float()
            gamma = (1.0 + 0.5 * torch.randn(K, generator=g, dtype=torch.float64)).float()
            beta = (0.5 * torch.randn(K, generator=g, dtype=torch.float64)).float()
            bias = (0.5 * torch.randn(N, generator=g, dtype=torch.float64)).float()
        self.N, self.K, self.regime, self.exact = N, K, regime, regime == "integer"
        self.W, self.bias, self.gamma, self.beta = W.to(device), bias.to(device), gamma.to(device), beta.to(device)
        self.name = f"{N}x{K}.{regime}"


def round_once(p64, dtype):
    """float64 -> a 16-bit type in ONE rounding: through fp32 rounded to odd (13 and 16 bits to spare), so that the second rounding
    cannot see a false tie"""
    f = p64.float()
    err = p64 - f.double()
    nb = torch.nextafter(f, torch.where(err > 0, torch.full_like(f, float("inf")), torch.full_like(f, float("-inf"))))
    odd = (f.view(torch.int32) & 1) == 1
    return torch.where((err == 0) | odd, f, nb).to(dtype)


def fold_failures(case, wf, bias_csum, dtype, with_bias=True, what=""):
    """wf [N, K] of dtype, bias_csum fp32 [2 N] of one fold launch -> (failing Failures, worst ratio, (twice, once, ambiguous): how many
    elements were rounded twice / once where the two differ)"""
    N, K = case.N, case.K
    tag = f"{what}{case.name}.{TYPE_NAME[dtype]}" + ("" if with_bias else ".nobias")
    W, g, b = case.W.double(), case.gamma.double(), case.beta.double()
    p = W * g                                         # exact: 48 bits
    twice, once = p.float().to(dtype), round_once(p, dtype)
    ok = (wf == twice) | (wf == once)
    differ = twice != once
    counts = (int((differ & (wf == twice)).sum()), int((differ & (wf == once)).sum()), int(differ.sum()))
    fs = [_collect(torch.where(ok, 0.0, float("inf")).double(), tag + " wf is neither T(fl32(w gamma)) nor T(w gamma)")]
    stored = wf.double()
    bias = case.bias.double() if with_bias else torch.zeros(N, dtype=torch.float64, device=wf.device)
    want_b = bias + (W * b).sum(1)
    want_c = stored.sum(1)
    got_b, got_c = bias_csum[:N].double(), bias_csum[N:].double()
    if case.exact:
        fs.append(_collect(torch.where(got_c == want_c, 0.0, float("inf")).double().unsqueeze(1), tag + " csum (bits)"))
        fs.append(_collect(torch.where(got_b == want_b, 0.0, float("inf")).double().unsqueeze(1), tag + " bias' (bits)"))
        worst = 0.0
    else:
        bc = (K / 64 + 8) * U * stored.abs().sum(1) + gc.FLUSH
        bb = (K / 64 + 9) * U * ((W * b).abs().sum(1) + bias.abs()) + gc.FLUSH
        fs.append(_collect(((got_c - want_c).abs() / bc).unsqueeze(1), tag + " csum"))
        fs.append(_collect(((got_b - want_b).abs() / bb).unsqueeze(1), tag + " bias'"))
        worst = max(fs[1].worst, fs[2].worst)
    return [f for f in fs if f], worst, counts


def fold_model(case, dtype, with_bias=True, order="forward", fma=False, mutation=None):
    """fold_layernorm_kernel in float32: lane l adds columns l, l + 64, ...; butterfly 32 .. 1 -> (wf, bias_csum)"""
    W, g, b = case.W.float(), case.gamma.float(), case.beta.float()
    if mutation == "beta_plus1":
        b = torch.roll(b, -1)
    N, K = W.shape
    prod = W * g
    wf = prod.to(dtype)
    add_c = prod if mutation == "csum_unrounded" else wf.float()
    pad = (-K) % 64
    lanes = lambda t: torch.nn.functional.pad(t, (0, pad)).reshape(N, -1, 64)   # noqa: E731
    c3, w3, b3 = lanes(add_c), lanes(W), lanes(b.expand(N, K))
    cs, bb = torch.zeros(N, 64), torch.zeros(N, 64)
    trips = range(c3.shape[1])
    for t in (trips if order == "forward" else reversed(trips)):
        cs = cs + c3[:, t]
        bb = _fma(w3[:, t], b3[:, t], bb) if fma else bb + w3[:, t] * b3[:, t]
    steps = (32, 16, 8, 4, 2, 1) if order == "forward" else (1, 2, 4, 8, 16, 32)
    cs, bb = _butterfly(cs, steps)[:, 0], _butterfly(bb, steps)[:, 0]
    bias = case.bias.float() if with_bias else torch.zeros(N)
    return wf, torch.cat([bias + bb, cs])


# ---- bit-for-bit kernels ---------------------------------------------------------------------------------------------------------
def bits_failures(got, want, what=""):
    """tensors of one type equal to the bit (any NaN equals any NaN; +0 and -0 differ)"""
    g2, w2 = (t.reshape(t.shape[0], -1) if t.dim() > 1 else t.reshape(1, -1) for t in (got, want))
    it = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[g2.element_size()]
    same = (g2.contiguous().view(it) == w2.contiguous().view(it))
    if g2.is_floating_point():
        same = same | (torch.isnan(g2) & torch.isnan(w2))
    return _collect(torch.where(same, 0.0, float("inf")).double(), what + " (bits)")


def cast_specials(src_dtype):
    """special values of a cast's source type: +-0, NaN, +-inf, fp16 subnormals, fp32 ties to even for both 16-bit types, the edge of
    the fp16 range (65504, 65520 -> inf, 7e4), the largest finite fp32 (-> bf16 inf)"""
    if src_dtype == HF:
        v = [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 2.0 ** -24, -(2.0 ** -24), 3 * 2.0 ** -24, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -14, 65504.0, -65504.0,
             1.0 + 2.0 ** -10, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -10, 1.0 + 2.0 ** -7, 0.333251953125]
        return torch.tensor(v, dtype=torch.float32).half()
    v = [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, 6e-8, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -126,
         1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -23, -(2048.0 + 1.0), 2048.0 + 3.0,           # fp16 ties, and just above one
         1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, -(256.0 + 1.0), 256.0 + 3.0,                 # bf16 ties
         65504.0, 65519.99, 65520.0, -65520.0, 7e4, -7e4, 3.4028234663852886e38, -3.4028234663852886e38, 3.3895313892515355e38, 1e-3, -0.1]
    return torch.tensor(v, dtype=torch.float32)


def cast_ref(src, dst_dtype):
    """what every cast kernel must give: one rounding to nearest even; fp16 -> bf16 through fp32 (exact)"""
    return src.float().to(dst_dtype)


def cast16_model(x, dtype, count, mutation=None):
    """cast16_kernel's output buffer [count + 8] (sentinel behind count)"""
    out = torch.full((count + 8,), SENT, dtype=dtype)
    out[:count] = x[:count].to(dtype)
    if mutation == "tail_unwritten":
        out[count // 4 * 4:count] = SENT
    return out


def embed_ref(tokens, table, pos, img, n_tok, insert_col, x, B, L, Lx, d, seq_off=None, mutation=None):
    """embed_tokens_kernel on the sentinel-filled x [rows, d] (a copy is returned): column t < Lx of sample b is img[b, t - insert_col]
    inside the splice, table[tokens[b, t]] before it and table[tokens[b, t - (n_tok - 1)]] behind it, + pos[t] in fp32; packed rows
    (seq_off [B + 1]): sample b writes its first seq_off[b + 1] - seq_off[b] columns to rows seq_off[b] ...
    mutations: shift_off_by_one, pos_by_source, packed_full"""
    x = x.clone()
    for b in range(B):
        n = Lx
        r0 = b * Lx
        if seq_off is not None:
            r0 = int(seq_off[b])
            n = Lx if mutation == "packed_full" else min(Lx, int(seq_off[b + 1]) - r0)
        for t in range(n):
            col = t
            if img is not None and insert_col <= t < insert_col + n_tok:
                src = img[b, t - insert_col]
            else:
                if img is not None and t >= insert_col + n_tok:
                    col = t - (n_tok if mutation == "shift_off_by_one" else n_tok - 1)
                src = table[int(tokens[b, col])]
            if r0 + t < x.shape[0]:
                x[r0 + t] = src + pos[col if mutation == "pos_by_source" else t]
    return x


def im2col_ref(img, P, Kpad, dtype):
    """[B, 3, R, R] fp32 -> [B g g, Kpad]: row (b, py, px), column c P P + ky P + kx, zero behind 3 P P"""
    B, _, R, _ = img.shape
    g = R // P
    t = img.reshape(B, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, 3 * P * P)
    return torch.nn.functional.pad(t, (0, Kpad - 3 * P * P)).to(dtype)


# ---- l2_normalize / mix_normalize ------------------------------------------------------------------------------------------------
def norm_data(rows, dim, regime, seed=0, device="cpu"):
    """-> (a, b, wa, wb); l2 uses a alone.  L2_REGIMES scale a by 1, 2^-40, 2^40; MIX_REGIMES: random (weights 0.6 / 0.4), opposed
    (b = -3 a + 2^-8 noise, weights 1/2, 1/2: the sum cancels), weighted (0.9 / 0.1 with b x 5)"""
    g = _gen(seed, rows, dim, _str_seed(regime), 13)
    a = torch.randn(rows, dim, generator=g, dtype=torch.float64)
    b = torch.randn(rows, dim, generator=g, dtype=torch.float64)
    wa, wb = 0.6, 0.4
    if regime == "small":
        a = a * 2.0 ** -40
    elif regime == "large":
        a = a * 2.0 ** 40
    elif regime == "opposed":
        b, wa, wb = -3.0 * a + 2.0 ** -8 * b, 0.5, 0.5
    elif regime == "weighted":
        b, wa, wb = b * 5.0, 0.9, 0.1
    return a.float().to(device), b.float().to(device), wa, wb


def _norm_L(dim):
    return math.ceil(dim / 64) + 8


def l2_expected(x):
    x = x.double()
    ref = x / x.norm(dim=1, keepdim=True)
    return Expected(ref, ref.abs() * (_norm_L(x.shape[1]) / 2 + 3) * U, F32, False)


def mix_expected(a, b, wa, wb):
    """-> (Expected of a^, of b^, of the mixture); wa, wb as the kernel gets them: fp32"""
    c = (_norm_L(a.shape[1]) / 2 + 3) * U
    wa, wb = float(_f32(wa)), float(_f32(wb))
    ea, eb = l2_expected(a), l2_expected(b)
    ta, tb = wa * ea.ref, wb * eb.ref
    m = ta + tb
    e_m = abs(wa) * ea.pre_bound + abs(wb) * eb.pre_bound + 2 * U * (ta.abs() + tb.abs())
    nm = m.norm(dim=1, keepdim=True)
    ref = m / nm
    e = e_m / nm + ref.abs() * ((m.abs() * e_m).sum(1, keepdim=True) / nm.square() + c)
    return ea, eb, Expected(ref, e, F32, False)


def norm_failures(got, exp, what=""):
    """rows whose reference is NaN (an all-zero input row) must be NaN; the others are held to the bound"""
    nan_row = torch.isnan(exp.ref).any(1)
    good = ~nan_row
    fs = [_collect((got[good].double() - exp.ref[good]).abs() / exp.bound[good], what)]
    if bool(nan_row.any()):
        fs.append(_collect(torch.where(torch.isnan(got[nan_row]), 0.0, float("inf")).double(), what + " (an all-zero row must be NaN)"))
    return [f for f in fs if f], fs[0].worst


def _strided_sumsq(x, order, fma):
    """lane l adds x[l]^2, x[l + 64]^2, ... then the butterfly 32 .. 1 -> [rows, 1]"""
    rows, dim = x.shape
    t = torch.nn.functional.pad(x, (0, (-dim) % 64)).reshape(rows, -1, 64)
    s = torch.zeros(rows, 64)
    trips = range(t.shape[1])
    for i in (trips if order == "forward" else reversed(trips)):
        s = _fma(t[:, i], t[:, i], s) if fma else s + t[:, i] * t[:, i]
    return _butterfly(s, (32, 16, 8, 4, 2, 1) if order == "forward" else (1, 2, 4, 8, 16, 32))


def l2_model(x, order="forward", fma=False):
    x = x.float()
    return x / _strided_sumsq(x, order, fma).sqrt()


def mix_model(a, b, wa, wb, order="forward", fma=False):
    a, b = a.float(), b.float()
    wa, wb = _f32(wa), _f32(wb)
    va, vb = a / _strided_sumsq(a, order, fma).sqrt(), b / _strided_sumsq(b, order, fma).sqrt()
    m = _fma(wa.expand_as(va), va, wb * vb) if fma else wa * va + wb * vb
    return va, vb, m / _strided_sumsq(m, order, fma).sqrt()
