"""Per-ELEMENT checks of the training kernels of keds_amd/csrc/train.hip: LayerNorm with saved statistics and its backward, the
self-attention backward, the single-query cross-attention core and its backward, the contrastive loss and its text gradient, the
backward of the l2 normalisation, QuickGELU and its backward, AdamW, the column sums, and -- to the bit -- the transpose, the dropout
ReLU pair, the row gather / scatter and the counter-based dropout mask.  The shape of tests/row_check.py: seeded cases in regimes made
for the defects these kernels can have, a float64 reference on the inputs as the kernel receives them, a bound per element derived
from the kernel's own fp32 operations, and float32 CPU models of the kernels with deliberate mutations
(tests/test_host_train_check.py proves that the checks pass the models and catch every mutation).  Plain torch; imports without a GPU;
every reference works on the device its inputs are on.  No constant here was tuned on a kernel's output.

u = 2^-24.  Every bounded output is held to
    |got - ref| <= e (1 + 2 u_out) + u_out |ref| + 2^-126 (1 + m)
u_out the unit roundoff of the output type (2^-8 bf16, 2^-24 fp32), e the bound of the fp32 value before the output rounding, m the
magnitude sum a flushed probability multiplies (__expf gives 0 below 2^-126, and a product below it may be flushed as well).
eps(a) = 2^-20 + 2 |a| u is the relative error of __expf(a): 2^-20 the project's allowance for v_exp_f32, |a| u the rounding of the
argument and as much again for the constant folded into it.  L(n) = ceil(n / 64) + 8: a lane's chain over n elements in strides of 64,
the six butterfly steps, one division and one more operation.

ln_fwd_stats, per row, L = L(dim): row_check's LayerNorm bound
    mu = mean x, d = x - mu, var = mean d^2, r = (var + 1e-5)^-1/2, ref = d r gamma + beta
    dmu = L u mean |x|;  dd = dmu + u |d|;  dv = 2 mean(|d| dd) + mean(dd^2) + (L + 4) u var;  dr = dv / (2 (var + 1e-5)) + 2^-20
    e = |gamma| r (dd + |d| (dr + 3 u)) + u |beta|;       stats = {mean, rstd} within dmu and r dr
ln_bwd, inputs dy, x, the GIVEN stats {mu, r}, gamma and the previous dx; g = dy gamma, xh = (x - mu) r, a = mean g, b = mean(g xh),
t = g - a - xh b:
    ref = dx + r t
    dxh = 2 u |xh|;  da = L u mean |g|;  db = (L + 4) u mean |g xh|
    dt = u |g| + da + |xh| db + |b| dxh + 3 u (|g| + |a| + |xh b|)          (the cancellation of t is in the magnitudes)
    e = r dt + 2 u (|dx| + r |t|)
dx_bf16 is the bf16 rounding of the stored fp32 dx to the bit; rows the map does not name, and the columns behind dim of a strided
row, keep their bits.

attention_bwd per (sample, head), S keys; cross_core_* with one query and K keys (S = K below):
    s = q k^T / 8, P = softmax s (m_i the row maximum), dP = go v^T, delta = sum_j P dP, dS = P (dP - delta) / 8
    out = P v (cross_core_fwd), dV = P^T go, dQ = dS k, dK = dS^T q
    ds = 66 u |q| |k|^T / 8                                     (64 products, 63 additions, the scale)
    rho_ij = 2 max_l ds_il + eps(s_ij - m_i) + sum_l P_il eps(s_il - m_i) + (ceil(S / 64) + 10) u          (relative, of P_ij)
    ddP = 66 u |go| |v|^T
    ddelta_i = sum_j P (rho |dP| + ddP) + (ceil(S / 64) + 8) u sum_j P |dP|
    ddS = [P (rho |dP - delta| + ddP + ddelta) + 3 u P (|dP| + |delta|)] / 8
    e_out = (P rho) |v| + (S + 1) u P |v|;  e_dV = (P rho)^T |go| + (S + 1) u P^T |go|
    e_dQ = ddS |k| + (S + 1) u |dS| |k|;    e_dK = ddS^T |q| + (S + 1) u |dS|^T |q|
    m: sum |v| (out), sum |go| (dV), W_i sum_j |k_j| (dQ), sum_i W_i |q_i| (dK) with W_i = 1 + 2 sum_l |dP_il|: a flushed P_ij moves
    dS_ij by at most 2^-126 (|dP_ij| + |delta_i|) / 8 and delta_i by 2^-126 |dP_ij|, and the product dS_ij itself may be flushed.

keds_clip_loss (outputs loss and dtxt), l = scale img txt^T over N rows, lse the row and the column log-sum-exp, z = sum exp(l - m):
    dl = (dim + 2) u scale |img| |txt|^T
    dlse = max dl + sum p eps(l - m) + L(N) u + 2^-20 (1 + |log z|) + u |lse|
    loss = mean_i ((lse_row_i - l_ii) + (lse_col_i - l_ii)) / 2 within mean dlse + (ceil(N / 256) + 8) u mean |lse - l_ii|
    G_ij = (p_row + p_col - 2 delta_ij) scale / 2N,  dtxt_j = sum_i G_ij img_i for j < B_local
    dG = [p_row (dl + dlse_i + eps(l - lse_i)) + p_col (dl + dlse_j + eps(l - lse_j)) + 3 u (p_row + p_col + 2 delta_ij)] scale / 2N
    e_dtxt = dG^T |img| + (N + 1) u |G|^T |img|,   m = scale sum_i |img_i|
    N = 1: the loss and the gradient are zero to the bit.

l2norm_bwd, nn = |x|^2, dot = x . dy, q = x dot / nn, t = dy - q, ref = t / |x|, L = L(dim):
    dnn = (L + 1) u (relative: a sum of squares);  ddot = (L + 1) u sum |x dy|
    dq = |x| ddot / nn + |q| (dnn + 2 u);  dt = dq + u (|dy| + |q|)
    e = (dt + |t| (dnn / 2 + 2^-20 + u)) / |x|

qgelu_fwd: gemm_check's QuickGELU term with e_in = 0, sg = sigmoid(1.702 x):
    e = |x| (sg (1 - sg) eps(1.702 x) + sg (2^-20 + 2 u)) + u |y|   (+ |y| where exp overflows: the kernel's y is -0)
qgelu_bwd, f' = s + 1.702 x s (1 - s):
    dsg = s (1 - s) eps(1.702 x) + 2 u s
    e = |dy| (dsg (1 + 1.702 |x| |1 - 2 s|) + 4 u (s + 1.702 |x| s (1 - s))) + u |dy f'|

adamw, one step from (p, g, m, v); the hyper-parameters are the float32 values the kernel receives; grad_scale a power of two (exact):
    bc1 = 1 - b1^t, bc2 = 1 - b2^t (powf: 2 ulps): rel1 = 2 u b1^t / bc1, rel2 = u b2^t / bc2 (half through the root)
    m' = b1 m + (1 - b1) g within e_m = 3 u (|b1 m| + |(1 - b1) g|);  v' = b2 v + (1 - b2) g^2 within 3 u of its terms
    D = lr (m' / bc1) / (sqrt(v' / bc2) + eps);  p' = p - lr wd p - D
    e_p = 3 u |p| + 12 u |D| + lr e_m / bc1 / (sqrt(v' / bc2) + eps) + (rel1 + rel2) |D|

colsum: (ceil(rows / 4) + 3) u sum |x|; equal to the bit in the `integer` regime and over two launches; `accumulate` adds once.
Bit for bit: transpose_to_bf16 against src.t().bfloat16() with pad rows [rows, ld_out) +0; dropout_relu_* (one fp32 multiply, the gate
z > 0 in fp32; zeros compared by value); rows_gather; rows_scatter (accumulate: one fp32 addition); dropout_mask against a uint64
model of the counter hash."""
import math

import numpy as np
import torch

from tests import attention_check as ac
from tests import gemm_check as gc
from tests import row_check as rc
from tests.gemm_check import Failures, _collect  # noqa: F401  (re-exported)
from tests.row_check import bits_failures  # noqa: F401

U = gc.U32
U_FN = gc.U_FN
UNIT, TINY, FLUSH = gc.UNIT, gc.TINY, gc.FLUSH      # (TINY is 0 for both output types here: bf16 and fp32)
SENT = gc.SENTINEL
LN_EPS = gc.LN_EPS
BF, F32 = torch.bfloat16, torch.float32
QA = float(np.float32(1.702))                   # the constant as the kernels hold it
F64 = torch.float64

ATT_S = (1, 2, 3, 63, 64, 65, 77, 79, 80)
ATT_BH = ((1, 1), (2, 3))
CROSS_K = (1, 2, 15, 16, 17, 31, 32)
CROSS_BH = ((1, 1), (3, 3), (5, 8))
LN_ROWS = (1, 3, 4, 5, 9)
LN_DIMS = (1, 63, 64, 65, 128, 768, 1000)
LN_REGIMES = ("random", "offset6", "offset1k", "constant", "spike", "tiny", "rowscale")
LN_DY = ("random", "parallel", "constant_g")    # dy gamma random / proportional to xhat (t cancels whole) / constant
LOSS_N = (1, 2, 63, 64, 65, 255, 256, 257, 600)
LOSS_DIMS = (4, 128, 768)
LOSS_SCALES = (14.3, 100.0)
LOSS_REGIMES = ("random", "matched")
L2_ROWS = (1, 4, 5)
L2_DIMS = (1, 4, 63, 64, 65, 768, 1000)
L2_REGIMES = ("random", "small", "large", "parallel")
FLAT_N = (1, 255, 256, 257, 3 * 256 + 1)
T_ROWS = (1, 31, 32, 33, 300)
T_COLS = (1, 63, 64, 65, 192)
G_ROWS = (1, 3, 33)
G_DIMS = (1, 85, 256)
ATT_MUTATIONS = ("softmax_first64", "droplast", "causal_ge", "delta_row_plus1", "dk_untransposed", "ds_unscaled", "dv_unnormalised")
CROSS_MUTATIONS = ("droplast", "dkv_key_plus1")
LNB_MUTATIONS = ("b_short", "stats_row_plus1", "dx_dense", "bf_unaccumulated")
LOSS_MUTATIONS = ("col_lse_as_row", "no_diag", "grad_over_blocal")
COLSUM_MUTATIONS = ("wave3_missing", "accumulate_ignored")
ADAMW_MUTATIONS = ("wd_after", "bc2_outside_root")


def L(n):
    return math.ceil(n / 64) + 8


def eps_exp(a):
    return U_FN + 2 * a.abs() * U


def bound(ref, e, dtype, m=0.0):
    u = UNIT[dtype]
    return e * (1 + 2 * u) + u * ref.abs() + FLUSH * (1 + m)


def _2d(t):
    return t.reshape(1, -1) if t.dim() < 2 else t


def held(got, ref, e, dtype, what, m=0.0):
    """every element of got against the bound"""
    return _collect(_2d((got.double() - ref).abs() / bound(ref, e, dtype, m)), what)


def same_bits(got, want, what):
    return rc.bits_failures(_2d(got), _2d(want), what)


def same_value(got, want, what):
    """equal as numbers: +0 == -0, any NaN equals any NaN"""
    same = (got == want) | (torch.isnan(got.float()) & torch.isnan(want.float()))
    return _collect(_2d(torch.where(same, 0.0, float("inf")).double()), what + " (values)")


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + (rc._str_seed(k) if isinstance(k, str) else int(k))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _top(fails, worst):
    return max([worst] + [f.worst for f in fails])


# ---- the float32 lane chain --------------------------------------------------------------------------------------------------------
def _steps(order):
    return (32, 16, 8, 4, 2, 1) if order == "forward" else (1, 2, 4, 8, 16, 32)


def _butterfly(s, order):
    lane = torch.arange(64)
    for o in _steps(order):
        s = s + s[..., lane ^ o]
    return s[..., :1]


def _chain(t, order="forward", trips=None):
    """lane l adds t[l], t[l + 64], ... (forwards or reversed; `trips`: only the first so many), then the xor butterfly -> [..., 1]"""
    n = t.shape[-1]
    t = torch.nn.functional.pad(t, (0, (-n) % 64)).reshape(*t.shape[:-1], -1, 64)
    s = torch.zeros(*t.shape[:-2], 64)
    idx = list(range(t.shape[-2] if trips is None else trips))
    for i in (idx if order == "forward" else reversed(idx)):
        s = s + t[..., i, :]
    return _butterfly(s, order)


def _seq(terms, order="forward"):
    """one thread adding terms[0], terms[1], ... in turn (or reversed), from 0"""
    s = torch.zeros_like(terms[0])
    for t in (terms if order == "forward" else reversed(terms)):
        s = s + t
    return s


def _exp32(a):
    """__expf in float32: correctly rounded, results below 2^-126 flushed"""
    p = torch.exp(a.float())
    return torch.where(p < FLUSH, torch.zeros_like(p), p)


# ---- LayerNorm with statistics, and its backward -------------------------------------------------------------------------------------
def ln_map(rows, which):
    """-> (map int32 [rows] or None, source rows): `map`: a permutation with gaps that touches row 0 and the last source row"""
    if which is None:
        return None, rows
    n_src = 2 * rows + 1
    m = torch.arange(rows) * 2
    m = m.flip(0).clone()
    m[0] = n_src - 1
    if rows > 1:
        m[-1] = 0
    assert len(set(m.tolist())) == rows
    return m.to(torch.int32), n_src


def ln_fwd_reference(x, gamma, beta):
    """x [rows, dim] the rows as the kernel reads them -> dict(y, e_y, mean, e_mean, rstd, e_rstd) float64"""
    dim = x.shape[1]
    Ld = L(dim)
    x, g, b = x.double(), gamma.double(), beta.double()
    mu = x.mean(1, keepdim=True)
    d = x - mu
    var = d.square().mean(1, keepdim=True)
    r = (var + LN_EPS).rsqrt()
    dmu = Ld * U * x.abs().mean(1, keepdim=True)
    dd = dmu + U * d.abs()
    dv = 2 * (d.abs() * dd).mean(1, keepdim=True) + dd.square().mean(1, keepdim=True) + (Ld + 4) * U * var
    dr = 0.5 * dv / (var + LN_EPS) + U_FN
    e = g.abs() * r * (dd + d.abs() * (dr + 3 * U)) + U * b.abs()
    return dict(y=d * r * g + b, e_y=e, mean=mu, e_mean=dmu, rstd=r, e_rstd=r * dr)


def ln_fwd_failures(x_rows, gamma, beta, y, stats, what=""):
    """y bf16 [rows, dim], stats fp32 [rows, 2] of one launch; x_rows: the source rows already gathered"""
    R = ln_fwd_reference(x_rows, gamma, beta)
    fs = [held(y, R["y"], R["e_y"], BF, what + " y"),
          held(stats[:, :1], R["mean"], R["e_mean"], F32, what + " mean"),
          held(stats[:, 1:], R["rstd"], R["e_rstd"], F32, what + " rstd")]
    return [f for f in fs if f], max(f.worst for f in fs)


def ln_fwd_model(x_rows, gamma, beta, order="forward", mutation=None, at=(0, 0)):
    x = x_rows.float()
    dim = x.shape[1]
    dimf = torch.tensor(float(dim))
    mean = _chain(x, order) / dimf
    d = x - mean
    var = _chain(d * d, order) / dimf
    rstd = (var + torch.tensor(1e-5)).double().rsqrt().float()
    y = (d * rstd * gamma.float() + beta.float()).bfloat16()
    stats = torch.cat([mean, rstd], 1)
    if mutation == "drop_store_y":
        y[at] = SENT
    if mutation == "drop_store_stats":
        stats[at[0], 1] = SENT
    return y, stats


class LnBwdCase:
    """dy [rows, dim] dense, x and dx0 [n_src, ld] (NaN / the sentinel in the columns behind dim), map, gamma; stats as given"""

    def __init__(self, rows, dim, ld, mapped, regime, dy_regime="random", seed=0):
        base = rc.LnCase(rows, dim, regime, seed=seed + 17 * (ld - dim), group=1)
        self.map, self.n_src = ln_map(rows, "map" if mapped else None)
        g = _gen(seed, rows, dim, regime, dy_regime, 5)
        src = self.map.long() if mapped else torch.arange(rows)
        self.src = src
        xs = torch.randn(self.n_src, dim, generator=g) * 7.0 + 100.0          # rows no map entry names: gross if read
        xs[src] = base.x
        self.x = torch.full((self.n_src, ld), float("nan"))
        self.x[:, :dim] = xs
        self.gamma, self.beta = base.gamma, base.beta
        x64 = base.x.double()
        mu = x64.mean(1, keepdim=True)
        r = ((x64 - mu).square().mean(1, keepdim=True) + LN_EPS).rsqrt()
        self.stats_exact = torch.cat([mu, r], 1).float()
        xh = (x64 - mu) * r
        n = torch.randn(rows, dim, generator=g, dtype=F64)
        if dy_regime == "random":
            dy = n
        elif dy_regime == "parallel":
            dy = 0.75 * xh / self.gamma.double()
        else:
            dy = 1.25 / self.gamma.double().expand(rows, dim)
        self.dy = dy.float()
        self.dx0 = torch.full((self.n_src, ld), SENT)
        self.dx0[:, :dim] = torch.randn(self.n_src, dim, generator=g)
        self.rows, self.dim, self.ld, self.regime, self.dy_regime = rows, dim, ld, regime, dy_regime
        self.name = f"{rows}x{dim}.ld{ld}.{'map' if mapped else 'nomap'}.{regime}.{dy_regime}"

    def to(self, device):
        for k in ("x", "gamma", "beta", "stats_exact", "dy", "dx0", "src"):
            setattr(self, k, getattr(self, k).to(device))
        if self.map is not None:
            self.map = self.map.to(device)
        return self


def ln_bwd_reference(case, stats):
    """-> (ref, e) float64 [rows, dim] of the rows the launch writes"""
    dim = case.dim
    Ld = L(dim)
    x = case.x[case.src, :dim].double()
    dx = case.dx0[case.src, :dim].double()
    mu, r = stats[:, :1].double(), stats[:, 1:].double()
    g = case.dy.double() * case.gamma.double()
    xh = (x - mu) * r
    a = g.mean(1, keepdim=True)
    b = (g * xh).mean(1, keepdim=True)
    t = g - a - xh * b
    dxh = 2 * U * xh.abs()
    da = Ld * U * g.abs().mean(1, keepdim=True)
    db = (Ld + 4) * U * (g * xh).abs().mean(1, keepdim=True)
    dt = U * g.abs() + da + xh.abs() * db + b.abs() * dxh + 3 * U * (g.abs() + a.abs() + (xh * b).abs())
    e = r.abs() * dt + 2 * U * (dx.abs() + (r * t).abs())
    return dx + r * t, e


def ln_bwd_failures(case, stats, dx, dx_bf, what=""):
    """dx fp32 [n_src, ld] and dx_bf bf16 [n_src, ld] (or None; it started as the sentinel) AFTER the launch, whole buffers: the rows
    the map names are held to the bound in their first dim columns; everything else keeps its bits"""
    ref, e = ln_bwd_reference(case, stats)
    tag = what + case.name
    dim = case.dim
    fs = [held(dx[case.src, :dim], ref, e, F32, tag + " dx")]
    worst = fs[0].worst
    rest = torch.ones_like(dx, dtype=torch.bool)
    rest[case.src, :dim] = False
    fs.append(same_bits(dx[rest], case.dx0[rest], tag + " dx outside the written rows"))
    if dx_bf is not None:
        fs.append(same_bits(dx_bf[case.src, :dim], dx[case.src, :dim].bfloat16(), tag + " dx_bf16 is not the rounding of the stored dx"))
        fs.append(same_bits(dx_bf[rest], torch.full_like(dx_bf[rest], SENT), tag + " dx_bf16 outside the written rows"))
    return [f for f in fs if f], worst


def ln_bwd_model(case, stats, with_bf, order="forward", mutation=None, at=(0, 0)):
    """-> (dx, dx_bf or None): the whole buffers after the launch"""
    dim, ld, rows = case.dim, case.ld, case.rows
    st = torch.roll(stats, -1, 0) if mutation == "stats_row_plus1" else stats
    mean, rstd = st[:, :1].float(), st[:, 1:].float()
    p = case.x[case.src, :dim].float()
    gi = case.dy.float() * case.gamma.float()
    xh = (p - mean) * rstd
    dimf = torch.tensor(float(dim))
    a = _chain(gi, order) / dimf
    trips = math.ceil(dim / 64)
    b = _chain(gi * (p - mean) * rstd, order, trips=trips - 1 if mutation == "b_short" else None) / dimf
    term = rstd * (gi - a - xh * b)
    v = case.dx0[case.src, :dim] + term
    dx = case.dx0.clone()
    dx_bf = torch.full(case.dx0.shape, SENT, dtype=BF) if with_bf else None
    vb = (term if mutation == "bf_unaccumulated" else v).bfloat16()
    if mutation == "dx_dense":
        flat = dx.reshape(-1)
        idx = (case.src.unsqueeze(1) * dim + torch.arange(dim)).reshape(-1)
        flat[idx] = flat[idx] + term.reshape(-1)
        if with_bf:
            dx_bf.reshape(-1)[idx] = flat[idx].bfloat16()
        return dx, dx_bf
    if mutation == "drop_store_dx":
        v = v.clone()
        v[at] = case.dx0[case.src[at[0]], at[1]]
    dx[case.src, :dim] = v
    if with_bf:
        if mutation == "drop_store_bf":
            vb[at] = SENT
        dx_bf[case.src, :dim] = vb
    return dx, dx_bf


# ---- attention backward, cross-attention core ------------------------------------------------------------------------------------------
def att_inputs(B, S, H, regime, seed):
    """qkv bf16 [B S, 3 d] in attention_check's regimes, dout bf16 [B S, d]: N(0, 1), one-hot rows in `peaked`"""
    qkv = ac.make_qkv(B, S, H, regime, BF, seed)
    g = _gen(seed, B, S, H, regime, 3)
    d = 64 * H
    if regime == "peaked":
        go = torch.zeros(B * S, d)
        go[torch.arange(B * S), torch.randint(0, d, (B * S,), generator=g)] = 1.0
    else:
        go = torch.randn(B * S, d, generator=g)
    return qkv, go.bfloat16()


def _split_heads(t, B, S, H, ft=F64):
    return t.to(ft).reshape(B, S, H, 64).transpose(1, 2)


def _merge_heads(t):
    B, H, S, _ = t.shape
    return t.transpose(1, 2).reshape(B * S, H * 64)


def core_reference(q, k, v, go, causal=False):
    """q, go [..., Sq, 64], k, v [..., Sk, 64] float64 -> dict name -> (ref, e, m) (module docstring)"""
    Sq, Sk = q.shape[-2], k.shape[-2]
    T = lambda t: t.transpose(-1, -2)   # noqa: E731
    s = q @ T(k) / 8
    ds = 66 * U * (q.abs() @ T(k.abs())) / 8
    vis = torch.ones(Sq, Sk, dtype=torch.bool, device=q.device)
    if causal:
        vis = vis.tril()
    sm = s.masked_fill(~vis, float("-inf"))
    mx = sm.amax(-1, keepdim=True)
    P = torch.softmax(sm, -1)
    ep = eps_exp((s - mx).masked_fill(~vis, 0.0))
    rho = 2 * ds.masked_fill(~vis, 0.0).amax(-1, keepdim=True) + ep + (P * ep).sum(-1, keepdim=True) + (math.ceil(Sk / 64) + 10) * U
    dP = go @ T(v)
    ddP = 66 * U * (go.abs() @ T(v.abs()))
    delta = (P * dP).sum(-1, keepdim=True)
    ddelta = (P * (rho * dP.abs() + ddP)).sum(-1, keepdim=True) + (math.ceil(Sk / 64) + 8) * U * (P * dP.abs()).sum(-1, keepdim=True)
    dS = P * (dP - delta) / 8
    ddS = (P * (rho * (dP - delta).abs() + ddP + ddelta) + 3 * U * P * (dP.abs() + delta.abs())) / 8
    c = (Sk + 1) * U
    W = 1 + 2 * dP.abs().sum(-1, keepdim=True)
    return {
        "out": (P @ v, (P * rho) @ v.abs() + c * (P @ v.abs()), v.abs().sum(-2, keepdim=True).expand(*q.shape)),
        "dV": (T(P) @ go, T(P * rho) @ go.abs() + c * (T(P) @ go.abs()), go.abs().sum(-2, keepdim=True).expand(*k.shape)),
        "dQ": (dS @ k, ddS @ k.abs() + c * (dS.abs() @ k.abs()), W * k.abs().sum(-2, keepdim=True)),
        "dK": (T(dS) @ q, T(ddS) @ q.abs() + c * (T(dS.abs()) @ q.abs()), (W * q.abs()).sum(-2, keepdim=True).expand(*k.shape)),
    }


def att_reference(qkv, go, B, S, H, causal):
    """-> (ref, e, m) float64 [B S, 3 d]: dQ | dK | dV"""
    q, k, v = (_split_heads(t, B, S, H) for t in qkv.split(64 * H, dim=1))
    R = core_reference(q, k, v, _split_heads(go, B, S, H), causal)
    return tuple(torch.cat([_merge_heads(R[n][i]) for n in ("dQ", "dK", "dV")], 1) for i in range(3))


def att_failures(ref3, dqkv, what=""):
    ref, e, m = ref3
    d = ref.shape[1] // 3
    fs = [held(dqkv[:, i * d:(i + 1) * d], ref[:, i * d:(i + 1) * d], e[:, i * d:(i + 1) * d], BF, f"{what} {n}", m[:, i * d:(i + 1) * d])
          for i, n in enumerate(("dQ", "dK", "dV"))]
    return [f for f in fs if f], max(f.worst for f in fs)


def att_applicable(mutation, S, causal):
    if mutation == "softmax_first64":
        return S > 64
    if mutation == "causal_ge":
        return bool(causal)
    if mutation == "ds_unscaled":
        return S >= 2
    return S >= 2 if mutation in ("droplast", "delta_row_plus1", "dk_untransposed", "dv_unnormalised") else True


def att_model(qkv, go, B, S, H, causal, order="forward", mutation=None, at=(0, 0)):
    """attention_bwd_kernel in float32 -> dqkv bf16 [B S, 3 d]"""
    q, k, v = (_split_heads(t, B, S, H, F32) for t in qkv.split(64 * H, dim=1))
    g = _split_heads(go, B, S, H, F32)
    T = lambda t: t.transpose(-1, -2)   # noqa: E731
    s = _seq([q[..., :, None, c] * k[..., None, :, c] for c in range(64)], order)
    dP = _seq([g[..., :, None, c] * v[..., None, :, c] for c in range(64)], order)
    i, j = torch.arange(S).view(S, 1), torch.arange(S).view(1, S)
    vis = torch.ones(S, S, dtype=torch.bool)
    if causal:
        vis = (j < i) if mutation == "causal_ge" else (j <= i)
    if mutation == "droplast":
        vis = vis & (j != S - 1)
    if mutation == "softmax_first64":
        vis = vis & (j < 64)
    sc = (s * 0.125).masked_fill(~vis, float("-inf"))
    p = _exp32(sc - sc.amax(-1, keepdim=True))
    zinv = 1.0 / _chain(p, order)
    P = p * zinv
    delta = _chain(P * dP, order)
    if mutation == "delta_row_plus1":
        delta = torch.roll(delta, -1, -2)
    Pv = p if mutation == "dv_unnormalised" else P
    dV = _seq([Pv[..., r, :, None] * g[..., r, None, :] for r in range(S)], order)
    dS = P * (dP - delta) * (1.0 if mutation == "ds_unscaled" else 0.125)
    dQ = _seq([dS[..., :, r, None] * k[..., r, None, :] for r in range(S)], order)
    dSk = dS if mutation == "dk_untransposed" else T(dS)
    dK = _seq([dSk[..., :, r, None] * q[..., r, None, :] for r in range(S)], order)
    out = torch.cat([_merge_heads(t) for t in (dQ, dK, dV)], 1).bfloat16()
    if mutation in ("drop_store_dQ", "drop_store_dK", "drop_store_dV"):
        out[at[0], ("dQ", "dK", "dV").index(mutation[-2:]) * 64 * H + at[1]] = SENT
    return out


def cross_inputs(B, K, H, regime, seed):
    """Q bf16 [B, d], Kp, Vp bf16 [B K, d], dout bf16 [B, d]"""
    qkv = ac.make_qkv(B, K, H, regime, BF, seed)
    d = 64 * H
    Q = qkv[::K, :d].contiguous()
    g = _gen(seed, B, K, H, regime, 4)
    return Q, qkv[:, d:2 * d].contiguous(), qkv[:, 2 * d:].contiguous(), torch.randn(B, d, generator=g).bfloat16()


def cross_reference(Q, Kp, Vp, go, B, K, H):
    """-> dict name -> (ref, e, m) float64 in the layouts of the entry points"""
    q, g = _split_heads(Q, B, 1, H), _split_heads(go, B, 1, H)
    k, v = _split_heads(Kp, B, K, H), _split_heads(Vp, B, K, H)
    R = core_reference(q, k, v, g)
    return {n: tuple(_merge_heads(t) for t in R[n]) for n in R}


def cross_failures(R, got, what=""):
    """got: dict of the outputs present (out; or dQ, dK, dV)"""
    fs = [held(got[n], R[n][0], R[n][1], BF, f"{what} {n}", R[n][2]) for n in got]
    return [f for f in fs if f], max(f.worst for f in fs)


def cross_model(Q, Kp, Vp, go, B, K, H, order="forward", mutation=None, at=(0, 0)):
    """cross_core_fwd_kernel and cross_core_bwd_kernel in float32 -> dict(out, dQ, dK, dV) bf16"""
    q, g = _split_heads(Q, B, 1, H, F32)[..., 0, :], _split_heads(go, B, 1, H, F32)[..., 0, :]      # [B, H, 64]
    k, v = _split_heads(Kp, B, K, H, F32), _split_heads(Vp, B, K, H, F32)                                # [B, H, K, 64]
    Kn = K - 1 if mutation == "droplast" else K
    sc = [_butterfly(q * k[..., j, :], order) * 0.125 for j in range(Kn)]
    dp = [_butterfly(g * v[..., j, :], order) for j in range(Kn)]
    mx = torch.stack(sc).amax(0)
    p = [_exp32(s - mx) for s in sc]
    sm = _seq(p)
    o = _seq([p[j] * v[..., j, :] for j in range(Kn)])
    out = o / sm
    inv = 1.0 / sm
    pn = [x * inv for x in p]
    delta = _seq([pn[j] * dp[j] for j in range(Kn)])
    ds = [pn[j] * (dp[j] - delta) * 0.125 for j in range(Kn)]
    dq = _seq([ds[j] * k[..., j, :] for j in range(Kn)])
    dK = torch.full((B, H, K, 64), SENT)
    dV = torch.full((B, H, K, 64), SENT)
    for j in range(Kn):
        jj = (j + 1) % Kn if mutation == "dkv_key_plus1" else j
        dK[..., j, :] = ds[jj] * q
        dV[..., j, :] = pn[jj] * g
    res = {"out": out.reshape(B, H * 64), "dQ": dq.reshape(B, H * 64), "dK": _merge_heads(dK), "dV": _merge_heads(dV)}
    res = {n: t.bfloat16() for n, t in res.items()}
    if mutation and mutation.startswith("drop_store_"):
        res[mutation[11:]][at] = SENT
    return res


# ---- the contrastive loss ----------------------------------------------------------------------------------------------------------
def loss_inputs(N, dim, regime, seed):
    """img, txt fp32 [N, dim] with unit rows; `matched`: txt = img + 2^-6 noise, normalised (p_row + p_col - 2 cancels)"""
    g = _gen(seed, N, dim, regime, 6)
    nrm = lambda t: t / t.norm(dim=1, keepdim=True)   # noqa: E731
    img = nrm(torch.randn(N, dim, generator=g, dtype=F64))
    noise = torch.randn(N, dim, generator=g, dtype=F64)
    txt = nrm(noise) if regime == "random" else nrm(img + 2.0 ** -6 * noise)
    return img.float(), txt.float()


def loss_reference(img, txt, B_local, scale):
    """-> dict(loss, e_loss, dtxt [B_local, dim], e_dtxt, m_dtxt) float64; scale as the kernel receives it"""
    N, dim = img.shape
    sc = float(np.float32(scale))
    I, Tt = img.double(), txt.double()
    l = sc * (I @ Tt.t())
    dl = (dim + 2) * U * sc * (I.abs() @ Tt.abs().t())

    def lse_of(lg, dlg):                                # over the last dim
        m = lg.amax(1, keepdim=True)
        z = torch.exp(lg - m).sum(1, keepdim=True)
        lse = m + z.log()
        p = torch.exp(lg - lse)
        d = dlg.amax(1, keepdim=True) + (p * eps_exp(lg - m)).sum(1, keepdim=True) + L(N) * U + U_FN * (1 + z.log().abs()) + U * lse.abs()
        return lse, d, p
    lr_, dlr, pr = lse_of(l, dl)
    lc_, dlc, pc = lse_of(l.t(), dl.t())
    pc, diag = pc.t(), l.diagonal().unsqueeze(1)
    loss = ((lr_ - diag) + (lc_ - diag)).sum() / (2 * N)
    e_loss = (dlr + dlc).sum() / (2 * N) + (math.ceil(N / 256) + 8) * U * ((lr_ - diag).abs() + (lc_ - diag).abs()).sum() / (2 * N)
    eye = torch.eye(N, dtype=F64, device=img.device)
    G = (pr + pc - 2 * eye) * sc / (2 * N)
    dG = (pr * (dl + dlr + eps_exp(l - lr_)) + pc * (dl + dlc.t() + eps_exp(l - lc_.t())) + 3 * U * (pr + pc + 2 * eye)) * sc / (2 * N)
    dtxt = G.t() @ I
    e_dtxt = dG.t() @ I.abs() + (N + 1) * U * (G.abs().t() @ I.abs())
    m = sc * I.abs().sum(0, keepdim=True).expand(N, dim)
    return dict(N=N, loss=loss.reshape(1, 1), e_loss=e_loss.reshape(1, 1), dtxt=dtxt[:B_local], e_dtxt=e_dtxt[:B_local], m_dtxt=m[:B_local])


def loss_failures(R, loss, dtxt, what=""):
    """loss [1], dtxt [B_local, dim] of one launch; N = 1: both are zero"""
    if R["N"] == 1:
        fs = [same_value(loss.reshape(1, 1), torch.zeros(1, 1, device=loss.device), what + " loss at N = 1"),
              same_value(dtxt, torch.zeros_like(dtxt), what + " dtxt at N = 1")]
        return [f for f in fs if f], 0.0
    fs = [held(loss.reshape(1, 1), R["loss"], R["e_loss"], F32, what + " loss"), held(dtxt, R["dtxt"], R["e_dtxt"], F32, what + " dtxt", R["m_dtxt"])]
    return [f for f in fs if f], max(f.worst for f in fs)


def loss_model(img, txt, B_local, scale, order="forward", mutation=None, at=(0, 0)):
    """logits_kernel, lse_kernel, loss_reduce_kernel and loss_grad_text_kernel in float32 -> (loss [1], dtxt [B_local, dim])"""
    N, dim = img.shape
    sc = torch.tensor(scale, dtype=F32)
    a, b = img.float(), txt.float()
    pr = a[:, None, :] * b[None, :, :] if N * N * dim <= 2 ** 24 else None
    groups = []
    for c in range(0, dim, 4):
        x = pr[..., c:c + 4] if pr is not None else a[:, None, c:c + 4] * b[None, :, c:c + 4]
        groups.append(((x[..., 0] + x[..., 1]) + x[..., 2]) + x[..., 3])
    lg = _seq(groups, order) * sc

    def lse_of(t):
        m = t.amax(1, keepdim=True)
        return m + torch.log(_chain(_exp32(t - m), order))
    lr_, lc_ = lse_of(lg), lse_of(lg.t().contiguous())
    diag = lg.diagonal().unsqueeze(1)
    per = ((lr_ - diag) + (lc_ - diag)).reshape(1, N)
    per = torch.nn.functional.pad(per, (0, (-N) % 256)).reshape(-1, 4, 64)          # thread t = 64 w + lane adds i = t, t + 256, ...
    parts = [_butterfly(_seq(list(per[:, w:w + 1, :]), order), order)[0, 0] for w in range(4)]
    loss = ((parts[0] + parts[1]) + (parts[2] + parts[3])) / torch.tensor(2.0 * N)
    colse = lr_.t() if mutation == "col_lse_as_row" else lc_.t()
    eye2 = torch.zeros(N, N) if mutation == "no_diag" else 2.0 * torch.eye(N)
    G = (_exp32(lg - lr_) + _exp32(lg - colse) - eye2) * torch.tensor(0.5 / N, dtype=F32) * sc
    rows = B_local if mutation == "grad_over_blocal" else N
    dt = _seq([G[i, :B_local, None] * a[i, None, :] for i in range(rows)], order)
    loss = loss.reshape(1)
    if mutation == "drop_store_loss":
        loss = torch.full((1,), SENT)
    if mutation == "drop_store_dtxt":
        dt[at] = SENT
    return loss, dt


# ---- backward of the l2 normalisation ------------------------------------------------------------------------------------------------
def l2b_inputs(rows, dim, regime, seed):
    g = _gen(seed, rows, dim, regime, 8)
    x = torch.randn(rows, dim, generator=g, dtype=F64)
    dy = torch.randn(rows, dim, generator=g, dtype=F64)
    if regime == "small":
        x = x * 2.0 ** -40
    elif regime == "large":
        x = x * 2.0 ** 40
    elif regime == "parallel":
        dy = 1.5 * x
    return x.float(), dy.float()


def l2b_reference(x, dy):
    dim = x.shape[1]
    Ld = L(dim)
    x, dy = x.double(), dy.double()
    nn = x.square().sum(1, keepdim=True)
    dot = (x * dy).sum(1, keepdim=True)
    q = x * dot / nn
    t = dy - q
    nrm = nn.sqrt()
    dnn = (Ld + 1) * U
    ddot = (Ld + 1) * U * (x * dy).abs().sum(1, keepdim=True)
    dq = x.abs() * ddot / nn + q.abs() * (dnn + 2 * U)
    dt = dq + U * (dy.abs() + q.abs())
    return t / nrm, (dt + t.abs() * (dnn / 2 + U_FN + U)) / nrm


def l2b_failures(x, dy, dx, what=""):
    ref, e = l2b_reference(x, dy)
    f = held(dx, ref, e, F32, what + " dx")
    return ([f] if f else []), f.worst


def l2b_model(x, dy, order="forward", mutation=None, at=(0, 0)):
    p, g = x.float(), dy.float()
    nn, dot = _chain(p * p, order), _chain(p * g, order)
    inv = nn.double().rsqrt().float()
    dx = (g - p * dot / nn) * inv
    if mutation == "drop_store":
        dx[at] = SENT
    return dx


# ---- QuickGELU -----------------------------------------------------------------------------------------------------------------------
def qgelu_values():
    """every bf16 value in [-32, 32] (subnormals and both zeros included) and +-100"""
    bits = torch.arange(0, 0x4200 + 1, dtype=torch.int32)                      # 0x4200 = 32.0
    pos = bits.to(torch.int16).view(BF)
    return torch.cat([pos, -pos, torch.tensor([100.0, -100.0], dtype=BF)])


def qgelu_fwd_reference(u):
    x = u.double()
    sg = torch.sigmoid(QA * x)
    y = x * sg
    e = x.abs() * (sg * (1 - sg) * eps_exp(QA * x) + sg * (U_FN + 2 * U)) + U * y.abs()
    return y, e + torch.where(-QA * x * math.log2(math.e) >= 126.0, y.abs(), torch.zeros_like(y))


def qgelu_bwd_reference(dy, u):
    x, d = u.double(), dy.double()
    s = torch.sigmoid(QA * x)
    f = s + QA * x * s * (1 - s)
    dsg = s * (1 - s) * eps_exp(QA * x) + 2 * U * s
    e = d.abs() * (dsg * (1 + QA * x.abs() * (1 - 2 * s).abs()) + 4 * U * (s + QA * x.abs() * s * (1 - s))) + U * (d * f).abs()
    return d * f, e


def qgelu_failures(u, y=None, dy=None, du=None, what=""):
    fs = []
    if y is not None:
        fs.append(held(y, *qgelu_fwd_reference(u), BF, what + " qgelu_fwd"))
    if du is not None:
        fs.append(held(du, *qgelu_bwd_reference(dy, u), BF, what + " qgelu_bwd"))
    return [f for f in fs if f], max(f.worst for f in fs)


def qgelu_model(u, dy=None, mutation=None, at=0):
    """-> (y, du or None) bf16; exp correctly rounded, inf where it overflows"""
    x = u.float()
    a = torch.tensor(QA, dtype=F32)
    ex = _exp32(-a * x)
    y = (x / (1.0 + ex)).bfloat16()
    du = None
    if dy is not None:
        s = 1.0 / (1.0 + ex)
        du = (dy.float() * (s + a * x * s * (1.0 - s))).bfloat16()
    if mutation == "drop_store_y":
        y[at] = SENT
    if mutation == "drop_store_du":
        du[at] = SENT
    return y, du


# ---- dropout + ReLU (bits) -------------------------------------------------------------------------------------------------------------
def gate_values():
    """+-0, +-2^-126, the smallest positive bf16 subnormal (2^-133) and its negative"""
    return torch.tensor([0.0, -0.0, 2.0 ** -126, -(2.0 ** -126), 2.0 ** -133, -(2.0 ** -133)], dtype=F32).bfloat16()


def dropout_inputs(n, seed):
    g = _gen(seed, n, 9)
    z = torch.randn(n, generator=g).bfloat16()
    gv = gate_values()
    k = min(n, len(gv))
    z[torch.randperm(n, generator=g)[:k]] = gv[torch.randperm(len(gv), generator=g)[:k]]
    mask = (torch.rand(n, generator=g) >= 0.3).to(torch.uint8)
    if n >= len(gv):
        mask[(z.float().abs() < 1e-30)] = 1                                   # the gates at the zero crossing stay open to the mask
    return z, mask, torch.randn(n, generator=g)


def dropout_fwd_ref(z, mask, scale):
    v = z.float()
    if mask is not None:
        v = torch.where(mask != 0, v * torch.tensor(scale, dtype=F32), torch.zeros_like(v))
    return torch.where(v > 0, v, torch.zeros_like(v)).bfloat16()


def dropout_bwd_ref(dy, z, mask, scale, mutation=None):
    on = z.float() > 0
    if mutation == "gate_ge":
        on = z.float() >= 0
    if mask is not None:
        on = on & (mask != 0)
    v = dy.float() * torch.tensor(scale if mask is not None else 1.0, dtype=F32)
    return torch.where(on, v, torch.zeros_like(v)).bfloat16()


# ---- dropout mask ----------------------------------------------------------------------------------------------------------------------
def dropout_mask_ref(n, seed, p):
    """the counter hash in uint64 and its float32 comparison -> uint8 [n]"""
    with np.errstate(over="ignore"):
        i = np.arange(1, n + 1, dtype=np.uint64)
        x = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * i
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    r = (x >> np.uint64(32)).astype(np.uint32).astype(np.float32) * np.float32(2.0 ** -32)
    return torch.from_numpy((r >= np.float32(p)).astype(np.uint8))


def keep_rate_ratio(mask, p):
    """|kept - n (1 - p)| in units of 5 binomial standard deviations (r = fl32(hash / 2^32) >= p keeps: p = 0 keeps everything)"""
    n = mask.numel()
    sd = math.sqrt(n * p * (1 - p))
    dev = abs(float(mask.double().sum()) - n * (1 - p))
    return 0.0 if dev == 0 else dev / (5 * sd + 1) if sd > 0 else float("inf")


# ---- AdamW ---------------------------------------------------------------------------------------------------------------------------
ADAMW_HP = dict(lr=1e-2, b1=0.9, b2=0.98, eps=1e-6, wd=0.2)


def adamw_inputs(n, regime, seed):
    g = _gen(seed, n, regime, 10)
    p, gr, m = torch.randn(n, generator=g), torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g)
    v = 0.01 * torch.rand(n, generator=g)
    if regime == "zero_vg":
        gr, v = torch.zeros(n), torch.zeros(n)
    return p, gr, m, v


def adamw_reference(p, g, m, v, step, gscale, hp=ADAMW_HP):
    """-> dict(p, e_p, m, e_m, v, e_v) float64"""
    lr, b1, b2, eps, wd = (float(np.float32(hp[k])) for k in ("lr", "b1", "b2", "eps", "wd"))
    p, g, m, v = p.double(), g.double() * gscale, m.double(), v.double()
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    rel1, rel2 = 2 * U * b1 ** step / bc1, U * b2 ** step / bc2
    m1 = b1 * m + (1 - b1) * g
    e_m = 3 * U * ((b1 * m).abs() + ((1 - b1) * g).abs())
    v1 = b2 * v + (1 - b2) * g * g
    e_v = 3 * U * ((b2 * v).abs() + (1 - b2) * g * g)
    den = (v1 / bc2).sqrt() + eps
    D = lr * (m1 / bc1) / den
    e_p = 3 * U * p.abs() + 12 * U * D.abs() + lr * e_m / bc1 / den + (rel1 + rel2) * D.abs()
    return dict(p=p - lr * wd * p - D, e_p=e_p, m=m1, e_m=e_m, v=v1, e_v=e_v)


def adamw_failures(R, p, m, v, what=""):
    fs = [held(p, R["p"], R["e_p"], F32, what + " p"), held(m, R["m"], R["e_m"], F32, what + " m"), held(v, R["v"], R["e_v"], F32, what + " v")]
    return [f for f in fs if f], max(f.worst for f in fs)


def adamw_model(p, g, m, v, step, gscale, hp=ADAMW_HP, mutation=None, at=0):
    f = lambda x: torch.tensor(x, dtype=F32)   # noqa: E731
    lr, b1, b2, eps, wd = (f(hp[k]) for k in ("lr", "b1", "b2", "eps", "wd"))
    bc1 = f(1.0) - f(float(np.float32(float(b1) ** step)))
    bc2 = f(1.0) - f(float(np.float32(float(b2) ** step)))
    w = p.float()
    if mutation != "wd_after":
        w = w - lr * wd * w
    gi = g.float() * f(gscale)
    mi = b1 * m.float() + (f(1.0) - b1) * gi
    vi = b2 * v.float() + (f(1.0) - b2) * gi * gi
    root = torch.sqrt(vi) / bc2 if mutation == "bc2_outside_root" else torch.sqrt(vi / bc2)
    w = w - lr * (mi / bc1) / (root + eps)
    if mutation == "wd_after":
        w = w - lr * wd * w
    if mutation == "drop_store_p":
        w[at] = p[at]
    if mutation == "drop_store_m":
        mi[at] = m[at]
    if mutation == "drop_store_v":
        vi[at] = v[at]
    return w, mi, vi


# ---- column sums, transpose, gather / scatter ---------------------------------------------------------------------------------------
def matrix_data(rows, cols, regime, src_dtype, seed):
    """[rows, cols] of src_dtype: `integer` (small integers: every sum is exact in any order), `random`, `specials` (random with
    row_check.cast_specials scattered in: for the transpose)"""
    g = _gen(seed, rows, cols, regime, 11)
    if regime == "integer":
        return torch.randint(-8, 9, (rows, cols), generator=g).to(src_dtype)
    x = (torch.randn(rows, cols, generator=g) * 3.0 + 0.5)
    if regime == "specials":
        sp = rc.cast_specials(F32)
        k = min(rows * cols, len(sp))
        x.reshape(-1)[torch.randperm(rows * cols, generator=g)[:k]] = sp[torch.randperm(len(sp), generator=g)[:k]]
    return x.to(src_dtype)


def strided(x, ld, fill=float("nan")):
    if ld == x.shape[1]:
        return x.contiguous()
    s = torch.full((x.shape[0], ld), fill, dtype=x.dtype, device=x.device)
    s[:, :x.shape[1]] = x
    return s


def colsum_failures(x, prev, got, exact, what=""):
    """got fp32 [cols] = (prev or 0) + sum_r x"""
    rows = x.shape[0]
    ref = x.double().sum(0) + (0 if prev is None else prev.double())
    if exact:
        f = same_bits(got, ref.float(), what + " colsum")
        return ([f] if f else []), 0.0
    f = held(got, ref, (math.ceil(rows / 4) + 3) * U * x.double().abs().sum(0), F32, what + " colsum")
    return ([f] if f else []), f.worst


def colsum_model(x, prev, order="forward", mutation=None, at=0):
    xf = x.float()
    rows = xf.shape[0]
    parts = []
    for w in range(4):
        rs = list(range(w, rows, 4))
        parts.append(_seq([xf[r] for r in rs], order) if rs and not (w == 3 and mutation == "wave3_missing") else torch.zeros(xf.shape[1]))
    t = (parts[0] + parts[1]) + (parts[2] + parts[3])
    out = t if prev is None or mutation == "accumulate_ignored" else prev.float() + t
    if mutation == "drop_store":
        out[at] = SENT if prev is None else prev[at]
    return out


def transpose_ref(x, ld_out):
    """-> bf16 [cols, ld_out]: x^T, +0 in columns [rows, ld_out)"""
    rows, cols = x.shape
    out = torch.zeros(cols, ld_out, dtype=BF, device=x.device)
    out[:, :rows] = x.t().to(BF)
    return out


def transpose_model(x, ld_out, mutation=None, at=(0, 0)):
    out = transpose_ref(x, ld_out)
    if mutation == "pad_not_zeroed" and ld_out > x.shape[0]:
        out[:, ld_out - 1] = SENT
    if mutation == "drop_store":
        out[at] = SENT
    return out


def gather_map(rows, n_src, seed):
    """distinct rows of [0, n_src) in a shuffled order that touch the last row and (rows > 1) row 0"""
    assert n_src >= rows + 1
    g = _gen(seed, rows, n_src, 12)
    mid = 1 + torch.randperm(n_src - 2, generator=g)[:max(rows - 2, 0)]
    m = torch.cat([torch.tensor([n_src - 1]), torch.tensor([0])[:rows - 1], mid])
    return m[torch.randperm(rows, generator=g)].to(torch.int32)


def scatter_ref(src, map_, dst0, dim, accumulate):
    """dst0 [n, ld] -> the buffer after dst[map[r], :dim] (+)= src[r]"""
    out = dst0.clone()
    idx = map_.long()
    out[idx, :dim] = out[idx, :dim] + src if accumulate else src
    return out
