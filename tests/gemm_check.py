"""Per-ELEMENT checks of the GEMM kernels (keds_amd/csrc/gemm.hip): seeded cases whose outputs are dominated by the defects these
kernels can have, a float64 reference on the rounded operands, a per-element bound derived from the number formats, and a CPU model
of the kernels' rounding with deliberate mutations (tests/test_host_gemm_check.py proves with it that the bound catches them).
Plain torch; imports without a GPU.  Nothing is sampled: every element of a launch is compared.

out[M, N] = epilogue(A[M, K] . W[N, K]^T + bias[N]); A and W of one 16-bit operand type (bf16 or fp16; EPILOGUES maps every public
epilogue code to its operand type, output type and family -- further operand types would be further rows of that table).

Regimes (make_case), all seeded and already rounded to the operand type:
  integer  small-integer A, W, bias, residual and positional embedding, amplitudes by K (_INT_AMP) so that every product and every
           partial sum, in ANY order, is an integer below 2^24: the fp32 accumulator is exact and order independent, and every linear
           epilogue's output is known to the bit (the exact sum rounded once to the output type): torch.equal.  Row statistics are
           exact too while the squares of any 512 outputs of a row (the largest group a kernel sums in fp32 before its integer
           atomic) stay below 2^24; Case.stats_exact asserts that on the case itself, and where it does not hold the sum of
           squares is checked by the bound.  LayerNorm / QuickGELU epilogues: bound without the accumulation term.
  random   A ~ N(0, 1), W ~ N(0, 1 / K): what the whole-tensor tests use.
  tail     random, with A's column k scaled by 2^(6 (k + 1) / K): the LAST 64-wide K-tile carries the largest share of every output
  head     ... by 2^(-6 k / K): the FIRST one does (both normalised to unit mean square).  A dropped or stale edge K-tile, the first or
           last split-K slice, the ring's wrap.
  offset   random plus a row constant of +-(3 .. 6): |row mean| several times the row's standard deviation.  The folded LayerNorm
           form rstd (acc - mean colsum) cancels on such rows: a coefficient of the wrong row or a column sum of the wrong column is
           gross.  (|mean| / std stays far below the numerics guard's 32.)

Reference: float64 on the rounded operands, acc = A W^T, and beside it the magnitude sum S = |A| |W|^T.

Bound per element, |got - ref| <= bound, u32 = 2^-24, u = unit roundoff of the OUTPUT type (2^-8 bf16, 2^-11 fp16, 2^-24 fp32):
  accumulation   e_acc = C_ACC (K + 16) u32 S, C_ACC = 2.  Products of two 16-bit operands are exact in fp32 (at most 22 significant
                 bits).  A sum of K terms in fp32 in ANY order, every addition rounded to nearest, is within gamma_K = K u32 / (1 -
                 K u32) of S (Higham, Accuracy and Stability, section 4.2); + 16 for the additions of up to 16 split-K slices.  The factor
                 2: the matrix unit adds its 32 products and the accumulator in one multi-term adder whose internal alignment is not
                 documented to be a chain of correctly rounded binary additions -- an aligned-and-truncated addend loses up to one
                 ulp = 2 u32, not u32.  ZERO in the integer regime.
  linear forms   e_pre = e_acc + 2 u32 (S + |bias| + |resid or pos|): the two fp32 additions of the epilogue.  Zero in `integer`.
  LayerNorm      v = rstd acc + (nmr colsum + bias'), rstd = rsqrt(var + eps), nmr = -mean rstd, all fp32 (ln_coeff_from):
                 mean = fl(fl(s) fl(1 / K)): 3 u32;  q = fl(fl(ss) fl(1 / K)): 3 u32;  mean^2: 7 u32;  var = fl(q - mean^2): u32, so
                 |d var| <= (3 q + 7 mean^2 + var) u32 =: E;  var + eps: u32;  rsqrt: U_FN;  d rstd / rstd <= 0.5 E / (var + eps) + u32 +
                 U_FN =: dr;  nmr: dn = dr + 4 u32.  Epilogue: three products / sums more.  With T = rstd (|acc| + |mean colsum|) +
                 |bias'|:   e_pre = rstd e_acc + (dn + 3 u32) T.
  ReLU           1-Lipschitz: e = e_pre.
  QuickGELU      y = x sigma(1.702 x) as x rcp(1 + exp2(z)), z = fl(-1.702 log2(e)) x.  e = L e_pre + |x| (sigma (1 - sigma) (U_FN + 2 |z|
                 ln 2 u32) + sigma (U_FN + 2 u32)) + u32 |y|, L = sup |y'| (QGELU_LIPSCHITZ, evaluated on a grid below).  U_FN = 2^-20 is
                 the relative accuracy allowed to v_exp_f32, v_rcp_f32 and v_rsq_f32 (their documented accuracy is about one ulp
                 = 2^-23; 2^-20 is negligible beside u).  Where z >= 126 (x below -51) exp2 may overflow and the kernel's y is -0:
                 |y| itself (below 2^-120) is allowed there.
  output         bound = e (1 + 2 u) + u |ref| + t + 2^-126, t = 2^-25 for fp16 outputs (below 2^-14 fp16 rounds absolutely), 2^-126:
                 fp32 values below the normal range may be flushed.
No constant here was tuned on a kernel's output.

Row statistics {sum x, sum x^2} (64-bit fixed point, value 2^28): check_stats() compares them with the float64 sums of given values
the kernel STORED (themselves checked per element) within (N + 8) u32 sum |x| (fp32 sums of N values in any order; the squares carry
one rounding more) + (N / 8) 2^-29 (one fixed-point rounding per partial sum added).  The fp16 stream stores the ROUNDED fp32 sums
the statistics were taken of: every value may then differ by u |x| (+ 2^-25), which is added.

CPU model: emulate() accumulates per 64-wide K-tile in fp32, forwards or backwards, in 1 .. 16 split-K slices summed in fp32, and
applies the epilogue's fp32 operations as the kernels order them.  MUTATIONS are deliberate defects of it.

fp32 operands (keds_gemm_f32, gemm_f32_kernel of f32path.hip): Case(..., torch.float32) with the epilogue table F32_EPILOGUES (the
KEDS_F32_EPI_* codes 0 - 4 collide with the bf16 codes; epilogues(case) picks the table).  K-tiles of 16.  The bound is the one above:
C_ACC (K + 16) u32 S covers a chain of K multiply-adds, fused or not.  Regimes integer (exact), random, tail, head.

Split operands (keds_gemm_x3, epilogues 13 - 15 = X3_EPILOGUES): X3Case is built directly in the kernel's format, four fp16 planes
ah, al [M, K], wh, wl [N, K] and an exponent w_exp; what the kernel is specified to compute is
    acc = (ah wh^T + ah wl^T + al wh^T) 2^-w_exp,     S = (|ah| |wh|^T + |ah| |wl|^T + |al| |wh|^T) 2^-w_exp
in a K-loop of 3 K / 64 tiles (segment 0 hi.hi, 1 hi.lo, 2 lo.hi).  fp16 x fp16 products are exact in fp32, so the bound carries over
with e_acc = C_ACC (3 K + 16) u32 S.  The kernel cannot know whether its planes are a true split, so the planes are drawn
INDEPENDENTLY in every regime but `split`: each segment then weighs the same and a wrong plane, a wrong K offset at a seam or a
fourth lo.lo segment is gross.
  integer  all four planes, bias and residual small integers (_int_amp), S 2^w_exp + 32 < 2^24 asserted; 2^-w_exp is an exact
           scaling: epilogues 13 and 14 to the bit, for any w_exp
  random   independent N(0, 1) / N(0, 1 / K) 2^w_exp planes
  spike    random, with K-tile p of the 3 K / 64 carrying the output (about half of S up to K = 1024; spike_share): p in segment 0
           scales that tile's columns of both hi planes by 2^3, in segment 1 wl's by 2^6, in segment 2 al's by 2^6
  split    true splits of fp32 data (A ~ 2 N(0, 1) with every 97th column x 30, W ~ std N(0, 1)) made by `splitter` -- the
           library's own split kernels on the GPU, their torch evaluation split_ref / weight_exp_ref here.  The reference is the
           FULL product (ah + al) (wh + wl)^T 2^-w_exp and the bound gets the dropped term |al| |wl|^T 2^-w_exp added: the
           fp32-grade claim, per element.
  rowscale (any regime but integer) A's rows x 2^6 on every other 256-row tile: a prefetched K-tile of the wrong tile is gross.
X3_QGELU_PAIR: hi + lo against the reference within e (1 + 2 u) + 2^-22 |ref| + 2^-25 + 2^-126 (hi rounded to 11 bits, the
remainder to 11 more, a subnormal lo absolutely), and |lo| <= ulp_fp16(hi) / 2 per element: the planes are a split, not two numbers
that happen to sum right.  X3_MUTATIONS are the defects of the split-operand loop."""
import math

import torch

TILE_K = 64
U32 = 2.0 ** -24
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
TINY = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25, torch.float32: 0.0}
FLUSH = 2.0 ** -126
C_ACC = 2.0
U_FN = 2.0 ** -20
LN_EPS = 1e-5
STAT_SCALE = 2.0 ** 28
QGELU_A = 1.702
QGELU_Z = -2.4554669595930157                  # -1.702 log2(e), as the kernels write it
PATCH_G = 7                                    # patches per image of the PATCH epilogues' cases
REGIMES = ("integer", "random", "tail", "head", "offset")
SENTINEL = -777.0
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32


def _qgelu64(x):
    return x * torch.sigmoid(QGELU_A * x)


def _lipschitz():
    x = torch.linspace(-12.0, 12.0, 480001, dtype=torch.float64)
    s = torch.sigmoid(QGELU_A * x)
    return float((s + QGELU_A * x * s * (1 - s)).abs().max()) * 1.001


QGELU_LIPSCHITZ = _lipschitz()                 # ~1.10

# public epilogue code -> (operand type, output type, family)
EPILOGUES = {
    0: (BF, BF, "bias"), 1: (BF, BF, "qgelu"), 2: (BF, BF, "relu"), 3: (BF, F32, "resid"), 4: (BF, F32, "bias"), 5: (BF, F32, "patch"),
    6: (BF, BF, "ln"), 7: (BF, BF, "ln_qgelu"), 8: (BF, F32, "resid_stats"), 9: (BF, HF, "resid_stats"), 10: (HF, BF, "ln"),
    11: (HF, BF, "ln_qgelu"), 12: (BF, BF, "headf32"), 16: (HF, HF, "ln"), 17: (HF, HF, "ln_qgelu"), 18: (HF, HF, "resid_stats"),
    19: (HF, F32, "resid"), 20: (HF, HF, "qgelu"), 21: (HF, F32, "patch"), 22: (HF, F32, "bias"),
}
NAMES = {0: "BIAS_BF16", 1: "BIAS_QGELU_BF16", 2: "BIAS_RELU_BF16", 3: "BIAS_RESID_F32", 4: "BIAS_F32", 5: "PATCH_F32", 6: "LN_BIAS_BF16",
         7: "LN_QGELU_BF16", 8: "RESID_STATS_F32", 9: "RESID_STATS_F16", 10: "LN_BIAS_BF16_H", 11: "LN_QGELU_BF16_H", 12: "BIAS_BF16_HEADF32",
         16: "LN_BIAS_F16_H", 17: "LN_QGELU_F16_H", 18: "RESID_STATS_F16_H", 19: "BIAS_RESID_F32_H", 20: "BIAS_QGELU_F16_H",
         21: "PATCH_F32_H", 22: "BIAS_F32_H"}
LINEAR = ("bias", "relu", "resid", "patch", "headf32", "resid_stats")       # exact in the integer regime
# the fp32-operand kernel's own codes (KEDS_F32_EPI_*) and the split-operand ones (keds_gemm_x3)
F32_EPILOGUES = {0: (F32, F32, "bias"), 1: (F32, F32, "qgelu"), 2: (F32, F32, "resid"), 3: (F32, F32, "relu"), 4: (F32, F32, "patch")}
F32_NAMES = {0: "F32_BIAS", 1: "F32_QGELU", 2: "F32_RESID", 3: "F32_RELU", 4: "F32_PATCH"}
F32_REGIMES = ("integer", "random", "tail", "head")
X3_EPILOGUES = {13: (HF, F32, "bias"), 14: (HF, F32, "resid"), 15: (HF, HF, "qgelu_pair")}
X3_NAMES = {13: "X3_BIAS_F32", 14: "X3_RESID_F32", 15: "X3_QGELU_PAIR"}
X3_REGIMES = ("integer", "random", "spike", "split")
X3_MUTATIONS = ("x3_drop_lo", "x3_stale_lo", "x3_hi_for_lo", "x3_koff_runs_on", "x3_lo_lo", "x3_scale_after_bias", "x3_lo_zero", "drop_store")
MUTATIONS = ("drop_ktile", "stale_ktile", "swap_rows", "shift_side", "bias_per_slice", "drop_store", "resid_twice", "ln_row_plus1",
             "stats_miss16", "stats_twice")


def _int_amp(K):
    """(|A| max, |W| max) of the integer regime: K a^2 w^2 < 2^24 with a wide margin, and outputs of ~sqrt(K) a w / 1.5 whose squares
    sum below 2^24 over 512 of them"""
    return (3, 3) if K <= 256 else (2, 2) if K <= 1024 else (1, 2)


class Case:
    """One problem's operands and its float64 reference.  A [M, K], W [N, K] (operand type), bias fp32 [N], resid fp32 [M, N] (values
    an fp16 holds exactly, so one tensor serves the fp32 and the fp16 stream), pos fp32 [PATCH_G + 1, N]; acc, S float64 [M, N];
    LayerNorm side data of A's rows: stats int64 [M, 2] (fixed point), csum fp32 [N] (row sums of W), mean, var, rstd float64 [M, 1]."""

    def __init__(self, M, N, K, regime, dtype, seed=0, device="cpu"):
        self.tile_k = 16 if dtype == F32 else TILE_K               # gemm_f32_kernel walks K in tiles of 16
        assert K % self.tile_k == 0 and N % 8 == 0 and regime in REGIMES
        self.M, self.N, self.K, self.regime, self.dtype, self.device = M, N, K, regime, dtype, device
        self.name = f"{M}x{N}x{K}.{regime}.{ {BF: 'bf16', HF: 'fp16', F32: 'fp32'}[dtype]}"
        g = torch.Generator(device=device).manual_seed(seed * 1000003 + M * 7919 + N * 31 + K)      # (drawn on `device`: seeded per device type)
        kw = dict(generator=g, device=device)
        if regime == "integer":
            a, w = _int_amp(K)
            A = torch.randint(-a, a + 1, (M, K), **kw).double()
            W = torch.randint(-w, w + 1, (N, K), **kw).double()
            bias = torch.randint(-4, 5, (N,), **kw).double()
            resid = torch.randint(-8, 9, (M, N), **kw).double()
            pos = torch.randint(-8, 9, (PATCH_G + 1, N), **kw).double()
        else:
            kw["dtype"] = torch.float64
            A = torch.randn(M, K, **kw)
            W = torch.randn(N, K, **kw) * K ** -0.5
            bias = torch.randn(N, **kw) * 0.5
            resid = torch.randn(M, N, **kw) * 2.0
            pos = torch.randn(PATCH_G + 1, N, **kw)
            if regime in ("tail", "head"):
                k = torch.arange(K, dtype=torch.float64, device=device)
                s = torch.exp2(6.0 * (k + 1) / K) if regime == "tail" else torch.exp2(-6.0 * k / K)
                A = A * (s / s.square().mean().sqrt())
            elif regime == "offset":
                sign = torch.where(torch.rand(M, 1, **kw) < 0.5, -1.0, 1.0)
                A = A + sign * (3.0 + 3.0 * torch.rand(M, 1, **kw))
        self.A, self.W = A.to(dtype), W.to(dtype)
        self.bias = bias.float()
        self.resid = resid.half().float()
        self.pos = pos.float()
        A64, W64 = self.A.double(), self.W.double()
        self.acc = A64 @ W64.t()
        self.S = A64.abs() @ W64.abs().t()
        if regime == "integer":
            assert float(self.S.max()) + 32 < 2.0 ** 24, "integer regime: a partial sum could leave the exact range"
        s, ss = A64.sum(1, keepdim=True), A64.square().sum(1, keepdim=True)
        self.stats = torch.cat([s, ss], 1).mul(STAT_SCALE).round().to(torch.int64)
        self.csum = W64.sum(1).float()
        sf = self.stats.double() / STAT_SCALE                      # what the kernel reads
        self.mean = sf[:, :1] / K
        self.q = sf[:, 1:] / K
        self.var = (self.q - self.mean.square()).clamp_min(0.0)
        self.rstd = (self.var + LN_EPS).rsqrt()
        self._e_acc = None

    @classmethod
    def from_operands(cls, A, W, bias, resid=None, stats=None, csum=None):
        """The case of GIVEN operands (a link of a tower pass, read back from its buffers): A [M, K], W [N, K] of one operand type, bias
        fp32 [N] or None, resid [M, N] (what the output held before the launch), stats int64 [M, 2] (the fixed-point pairs the launch
        read) and csum fp32 [N] for the LayerNorm-folded epilogues.  Never `exact`: every check is by the bound."""
        c = cls.__new__(cls)
        c.dtype, c.device, c.regime = A.dtype, A.device, "operands"
        c.tile_k = 16 if c.dtype == F32 else TILE_K
        (c.M, c.K), c.N = A.shape, W.shape[0]
        c.name = f"{c.M}x{c.N}x{c.K}.operands"
        c.A, c.W = A, W
        c.bias = torch.zeros(c.N, device=A.device) if bias is None else bias.float()
        c.resid = None if resid is None else resid.float()
        c.pos = None
        A64, W64 = A.double(), W.double()
        c.acc = A64 @ W64.t()
        c.S = A64.abs() @ W64.abs().t()
        if stats is not None:
            c.stats, c.csum = stats, csum.float()
            sf = stats.double() / STAT_SCALE
            c.mean = sf[:, :1] / c.K
            c.q = sf[:, 1:] / c.K
            c.var = (c.q - c.mean.square()).clamp_min(0.0)
            c.rstd = (c.var + LN_EPS).rsqrt()
        c._e_acc = None
        return c

    @property
    def exact(self):
        return self.regime == "integer"

    def e_acc(self):
        if self._e_acc is None:
            self._e_acc = torch.zeros_like(self.S) if self.exact else C_ACC * (self.K + 16) * U32 * self.S
        return self._e_acc

    def rows(self, m):
        return torch.arange(m, device=self.device)

    def patch_rows(self):
        """output row of GEMM row m in the PATCH epilogues: image b = m // G keeps row b (G + 1) for its class token"""
        m = self.rows(self.M)
        return (m // PATCH_G) * (PATCH_G + 1) + 1 + m % PATCH_G

    def patch_out_rows(self):
        return (self.M + PATCH_G - 1) // PATCH_G * (PATCH_G + 1)

    def without_bias(self):
        """the same case for a launch with bias = NULL (fp32-operand kernel): shares every tensor but the bias"""
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.bias, c.name = torch.zeros_like(self.bias), self.name + ".nobias"
        c.__dict__.pop("_model_acc", None)
        return c


def split_ref(x, e=0):
    """what keds_split_f16_pair (e = 0) / keds_split_f16_weight compute, in IEEE arithmetic: hi = fp16(x 2^e), lo = fp16(x 2^e - hi)"""
    s = x.float() * torch.tensor(2.0 ** e, dtype=torch.float32, device=x.device)
    hi = s.half()
    return hi, (s - hi.float()).half()


def weight_exp_ref(w):
    """keds_split_f16_weight's exponent: max |w| 2^e in [2^13, 2^14), clamped to [-100, 40]; 0 for an all-zero matrix"""
    mx = float(w.abs().max())
    return 0 if mx == 0.0 else max(-100, min(40, 13 - (math.frexp(mx)[1] - 1)))


def _split_ref_pair(a, w):
    e = weight_exp_ref(w)
    return split_ref(a), split_ref(w, e), e


def x3_seg(p, np1):
    """K-tile p of 3 np1 -> (K-tile inside the plane, A reads its lo plane, W reads its lo plane): x3_seg of gemm_shared.h"""
    seg = p // np1
    return p - seg * np1, seg == 2, seg == 1


class X3Case:
    """One split-operand problem in the kernel's format and its float64 reference (module docstring).  regime `spike`: p = the K-tile
    of 3 K / 64 that carries the output; `split`: std = the weights' standard deviation, splitter(a fp32, w fp32) -> ((ah, al), (wh, wl),
    w_exp); rowscale: A's rows x 2^6 on every other 256-row tile."""

    def __init__(self, M, N, K, regime, w_exp=0, p=None, std=1.0, rowscale=False, seed=0, device="cpu", splitter=_split_ref_pair):
        assert K % TILE_K == 0 and N % 8 == 0 and regime in X3_REGIMES and not (rowscale and regime == "integer")
        self.M, self.N, self.K, self.regime, self.device, self.dtype = M, N, K, regime, device, HF
        np1 = K // TILE_K
        g = torch.Generator(device=device).manual_seed(seed * 1000003 + M * 7919 + N * 31 + K + 17 * (p or 0))
        kw = dict(generator=g, device=device)
        self.extra = None
        if regime == "integer":
            a, w = _int_amp(K)
            ah, al = (torch.randint(-a, a + 1, (M, K), **kw).half() for _ in range(2))
            wh, wl = (torch.randint(-w, w + 1, (N, K), **kw).half() for _ in range(2))
            bias = torch.randint(-4, 5, (N,), **kw).float()
            resid = torch.randint(-8, 9, (M, N), **kw).float()
        elif regime == "split":
            a = torch.randn(M, K, dtype=torch.float32, **kw) * 2.0
            a[:, ::97] *= 30.0
            w = torch.randn(N, K, dtype=torch.float32, **kw) * std
            (ah, al), (wh, wl), w_exp = splitter(a, w)
            bias = torch.randn(N, dtype=torch.float32, **kw) * (0.5 * std * K ** 0.5)
            resid = torch.randn(M, N, dtype=torch.float32, **kw) * (2.0 * std * K ** 0.5)
        else:
            ah, al = (torch.randn(M, K, dtype=torch.float64, **kw) for _ in range(2))
            wh, wl = (torch.randn(N, K, dtype=torch.float64, **kw) * (K ** -0.5 * 2.0 ** w_exp) for _ in range(2))
            bias = (torch.randn(N, dtype=torch.float64, **kw) * 0.5).float()
            resid = (torch.randn(M, N, dtype=torch.float64, **kw) * 2.0).float()
            if regime == "spike":
                assert 0 <= p < 3 * np1
                kt, a_lo, w_lo = x3_seg(p, np1)
                ks = slice(kt * TILE_K, (kt + 1) * TILE_K)
                if w_lo:
                    wl[:, ks] *= 64.0
                elif a_lo:
                    al[:, ks] *= 64.0
                else:
                    ah[:, ks] *= 8.0
                    wh[:, ks] *= 8.0
            ah, al, wh, wl = ah.half(), al.half(), wh.half(), wl.half()
        if rowscale:
            up = ((torch.arange(M, device=device) // 256) % 2 == 1).unsqueeze(1)
            ah, al = (torch.where(up, t * 64.0, t) for t in (ah, al))
        self.ah, self.al, self.wh, self.wl, self.w_exp, self.p, self.np1 = ah, al, wh, wl, int(w_exp), p, np1
        self.bias, self.resid = bias, resid
        tag = {"spike": f"spike{p}", "split": f"split{std:g}"}.get(regime, regime)
        self.name = f"{M}x{N}x{K}.x3.{tag}.e{self.w_exp}" + (".rowscale" if rowscale else "")
        sc = 2.0 ** -self.w_exp
        AH, AL, WH, WL = ah.double(), al.double(), wh.double(), wl.double()
        self.S = (AH.abs() @ (WH.abs() + WL.abs()).t() + AL.abs() @ WH.abs().t()) * sc
        if regime == "split":
            self.acc = ((AH + AL) @ (WH + WL).t()) * sc
            self.extra = (AL.abs() @ WL.abs().t()) * sc                    # the dropped lo.lo term, exactly bounded
        else:
            self.acc = (AH @ (WH + WL).t() + AL @ WH.t()) * sc
        if regime == "integer":
            raw = float(self.S.max()) / sc                                 # what the accumulators hold
            assert raw + 32 < 2.0 ** 24, "integer regime: a partial sum could leave the exact range"
            assert (raw * sc + 32) * max(1.0, 1.0 / sc) < 2.0 ** 24, "integer regime: the scaled sum + bias + residual is not exact in fp32"
        self._e_acc = None

    @property
    def exact(self):
        return self.regime == "integer"

    def e_acc(self):
        if self._e_acc is None:
            self._e_acc = torch.zeros_like(self.S) if self.exact else C_ACC * (3 * self.K + 16) * U32 * self.S
            if self.extra is not None:
                self._e_acc = self._e_acc + self.extra
        return self._e_acc

    @classmethod
    def from_operands(cls, ah, al, wh, wl, w_exp, bias, resid=None):
        """The case of GIVEN planes (a link of a tower pass): A planes [M, K], W planes [N, K] of W 2^w_exp (fp16), bias fp32 [N] or None,
        resid fp32 [M, N].  The reference is the three products of the planes themselves; never `exact`."""
        c = cls.__new__(cls)
        (c.M, c.K), c.N = ah.shape, wh.shape[0]
        c.regime, c.device, c.dtype, c.extra, c.p, c.np1 = "operands", ah.device, HF, None, None, c.K // TILE_K
        c.ah, c.al, c.wh, c.wl, c.w_exp = ah, al, wh, wl, int(w_exp)
        c.bias = torch.zeros(c.N, device=ah.device) if bias is None else bias.float()
        c.resid = None if resid is None else resid.float()
        c.name = f"{c.M}x{c.N}x{c.K}.x3.operands.e{c.w_exp}"
        sc = 2.0 ** -c.w_exp
        AH, AL, WH, WL = ah.double(), al.double(), wh.double(), wl.double()
        c.S = (AH.abs() @ (WH.abs() + WL.abs()).t() + AL.abs() @ WH.abs().t()) * sc
        c.acc = (AH @ (WH + WL).t() + AL @ WH.t()) * sc
        c._e_acc = None
        return c

    def spike_share(self):
        """the share of S that K-tile p carries, averaged over the outputs"""
        kt, a_lo, w_lo = x3_seg(self.p, self.np1)
        ks = slice(kt * TILE_K, (kt + 1) * TILE_K)
        a, w = (self.al if a_lo else self.ah)[:, ks].double().abs(), (self.wl if w_lo else self.wh)[:, ks].double().abs()
        return float(((a @ w.t()) * 2.0 ** -self.w_exp / self.S).mean())

    def rows(self, m):
        return torch.arange(m, device=self.device)


def epilogues(case):
    """the epilogue table of a case's kernel"""
    return X3_EPILOGUES if isinstance(case, X3Case) else F32_EPILOGUES if case.dtype == F32 else EPILOGUES


def epilogue_name(case, code):
    return (X3_NAMES if isinstance(case, X3Case) else F32_NAMES if case.dtype == F32 else NAMES)[code]


class Expected:
    """ref float64 [M, N] (before the output rounding), bound float64 [M, N], pre_bound (the bound without the output rounding: what
    the fp32 value the statistics see may be off by), bits: the output to the bit (integer regime, linear families) or None"""

    def __init__(self, ref, e, out_dtype, exact_bits, pair=False):
        u = UNIT[out_dtype]
        self.ref, self.pre_bound, self.out_dtype = ref, e, out_dtype
        # (pair: two fp16 planes, hi rounded to 11 bits and the remainder to 11 more; a subnormal lo rounds absolutely)
        self.bound = e * (1 + 2 * u) + (2.0 ** -22 if pair else u) * ref.abs() + TINY[out_dtype] + FLUSH
        self.bits = ref.to(out_dtype) if exact_bits else None      # float64 -> type: one rounding of the exact sum

    def first_rows(self, h):
        e = Expected.__new__(Expected)
        e.ref, e.pre_bound, e.out_dtype, e.bound = self.ref[:h], self.pre_bound[:h], self.out_dtype, self.bound[:h]
        e.bits = None if self.bits is None else self.bits[:h]
        return e


def expected(case, code, out_dtype=None):
    """what epilogue `code` must give on `case`.  out_dtype: override (the fp32 head rows of BIAS_BF16_HEADF32)"""
    op, od, fam = epilogues(case)[code]
    assert op == case.dtype, f"epilogue {code} takes {op} operands"
    od = od if out_dtype is None else out_dtype
    pair = fam == "qgelu_pair"
    fam = "qgelu" if pair else fam
    acc, S, bias = case.acc, case.S, case.bias.double()
    if fam in ("ln", "ln_qgelu"):
        mean, rstd, csum = case.mean, case.rstd, case.csum.double()
        pre = rstd * (acc - mean * csum) + bias
        E = (3 * case.q + 7 * mean.square() + case.var) * U32
        dn = 0.5 * E / (case.var + LN_EPS) + U32 + U_FN + 4 * U32
        T = rstd * (acc.abs() + (mean * csum).abs()) + bias.abs()
        e = rstd * case.e_acc() + (dn + 3 * U32) * T
    else:
        extra = case.resid.double() if fam in ("resid", "resid_stats") else \
            case.pos.double()[1 + case.rows(case.M) % PATCH_G] if fam == "patch" else None
        pre = acc + bias if extra is None else acc + bias + extra
        e = case.e_acc() if case.exact else case.e_acc() + 2 * U32 * (S + bias.abs() + (0 if extra is None else extra.abs()))
    if fam == "relu":
        return Expected(pre.clamp_min(0.0), e, od, case.exact)
    if fam in ("qgelu", "ln_qgelu"):
        sg = torch.sigmoid(QGELU_A * pre)
        z = (QGELU_Z * pre).abs()
        y = pre * sg
        e = QGELU_LIPSCHITZ * e + pre.abs() * (sg * (1 - sg) * (U_FN + 2 * z * math.log(2.0) * U32) + sg * (U_FN + 2 * U32)) + U32 * y.abs()
        e = e + torch.where(QGELU_Z * pre >= 126.0, y.abs(), torch.zeros_like(y))       # exp2 overflows: the kernel's y is -0
        return Expected(y, e, od, False, pair=pair)
    return Expected(pre, e, od, case.exact and fam in LINEAR)


# ---- comparison ------------------------------------------------------------------------------------------------------------------
class Failures(list):
    """(m, n, ratio) of the first failing elements; .count: how many failed; .worst: the largest |err| / bound of the elements that
    were checked (inf: a non-finite output or, in a bit comparison, any difference)"""
    count = 0
    worst = 0.0
    what = ""

    def __bool__(self):
        return self.count > 0

    def __str__(self):
        def where(m, n, x):
            return (f"(m{m} n{n}: {x:.3g}; tile256 ({m // 256}, {n // 256}) row {m % 256} col {n % 256}; tile128 ({m // 128}, {n // 128}) "
                    f"row {m % 128}; group8 {n // 8})")
        return f"{self.what}: {self.count} elements beyond the bound (worst ratio {self.worst:.3g}): " + ", ".join(where(*f) for f in self)


def _collect(ratio, what, show=6):
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    out = Failures()
    out.what = what
    out.worst = float(ratio.max()) if ratio.numel() else 0.0
    bad = ratio > 1.0
    out.count = int(bad.sum())
    if out.count:
        idx = bad.nonzero()[:show].cpu().tolist()
        vals = ratio.cpu()
        for i in idx:
            m, n = (i + [0])[:2]
            out.append((m, n, float(vals[tuple(i)])))
    return out


def check(got, exp, what=""):
    """every element of got [M, N] against the bound"""
    return _collect((got.double() - exp.ref).abs() / exp.bound, what)


def check_bits(got, exp, what=""):
    """integer regime, linear families: the output to the bit (a difference counts as an infinite ratio)"""
    assert exp.bits is not None
    same = (got == exp.bits) | (torch.isnan(got) & torch.isnan(exp.bits))
    return _collect(torch.where(same, 0.0, float("inf")).double(), what + " (bits)")


def verify(got, exp, what=""):
    """the strictest comparison the case allows: bits where they are known, else the bound"""
    return check_bits(got, exp, what) if exp.bits is not None else check(got, exp, what)


def stats_exact(values64):
    """are the fp32 partial sums of squares of a row exact whatever their order?  (sum x^2 of any aligned 512 outputs < 2^24, integer
    values)"""
    M, N = values64.shape
    if not bool((values64 == values64.round()).all()):
        return False
    pad = (-N) % 512
    sq = torch.nn.functional.pad(values64.square(), (0, pad)).reshape(M, -1, 512).sum(-1)
    return float(sq.max()) < 2.0 ** 24 and float(values64.abs().sum(1).max()) < 2.0 ** 24


def check_stats(stats, values64, extra=None, exact=False, what="", squares_only_by_bound=False):
    """stats int64 [M, 2] against the float64 {sum, sum sq} of values64 [M, N].  extra [M, N]: what each value the kernel summed may
    differ from values64 by.  exact: both must be equal to the bit (squares_only_by_bound: the sum only)."""
    M, N = values64.shape
    got = stats.double() / STAT_SCALE
    want = torch.stack([values64.sum(1), values64.square().sum(1)], 1)
    a1, a2 = values64.abs().sum(1), values64.square().sum(1)
    fix = (N / 8) * 2.0 ** -29 + 2.0 ** -28
    b = torch.stack([(N + 8) * U32 * a1 + fix, (N + 9) * U32 * a2 + fix], 1)
    if extra is not None:
        b = b + torch.stack([extra.sum(1), (2 * values64.abs() * extra + extra.square()).sum(1)], 1) * (1 + (N + 9) * U32)
    ratio = (got - want).abs() / b
    if exact:
        wrong = (stats != want.mul(STAT_SCALE).round().to(torch.int64))
        inf = torch.where(wrong, float("inf"), 0.0).double()
        ratio = torch.stack([inf[:, 0], ratio[:, 1] if squares_only_by_bound else inf[:, 1]], 1)
    return _collect(ratio, what + " (row statistics {sum, sum sq}: n = 0 / 1)")


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ---- CPU model of the kernels' rounding, and its mutations -----------------------------------------------------------------------
def _fixed(v32):
    return (v32.double() * STAT_SCALE).round().to(torch.int64)


def emulate(case, code, order="forward", splits=1, mutation=None, at=None):
    """-> dict(out [M, N] of the output type; for PATCH [patch_out_rows, N] with the class-token rows = SENTINEL), stats int64 [M, 2]
    for the RESID_STATS families, copy bf16 for RESID_STATS_F32, head fp32 for HEADF32).  fp32 throughout, as the kernels: per
    64-wide K-tile, `order` forward / reverse, `splits` slices summed in fp32 by a second pass that then applies the epilogue.
    mutation: one of MUTATIONS, placed by `at` = dict(row=, col=, kt=): the 8-row piece that contains `row`, K-tile kt."""
    if isinstance(case, X3Case):
        assert splits == 1
        return _emulate_x3(case, code, order, mutation, at)
    op, od, fam = epilogues(case)[code]
    assert str(case.device) == "cpu" and op == case.dtype
    M, N, K = case.M, case.N, case.K
    TILE_K = case.tile_k                                                      # 64; 16 for fp32 operands
    nk = K // TILE_K
    at = dict(row=0, col=0, kt=nk - 1) | (at or {})
    r, c, ktm = at["row"], at["col"], at["kt"]
    piece = slice(r // 8 * 8, min(r // 8 * 8 + 8, M))
    cols = slice(c // 256 * 256, min(c // 256 * 256 + 256, N))
    A, W = case.A.float(), case.W.float()
    assert nk % splits == 0
    per = nk // splits
    ktile_mut = mutation in ("drop_ktile", "stale_ktile")
    cache = case.__dict__.setdefault("_model_acc", {})
    acc = None if ktile_mut else cache.get((order, splits))
    for s in (() if acc is not None else range(splits) if order == "forward" else reversed(range(splits))):
        acc = torch.zeros(M, N) if acc is None else acc
        part = torch.zeros(M, N)
        kts = range(s * per, (s + 1) * per)
        for kt in (kts if order == "forward" else reversed(kts)):
            ks = slice(kt * TILE_K, (kt + 1) * TILE_K)
            p = A[:, ks] @ W[:, ks].t()
            if mutation in ("drop_ktile", "stale_ktile") and kt == ktm:
                a = torch.zeros(piece.stop - piece.start, TILE_K)
                if mutation == "stale_ktile" and kt >= 2:                      # the ring buffer still holds the K-tile two back
                    a = A[piece, (kt - 2) * TILE_K:(kt - 1) * TILE_K]
                p[piece, cols] = a @ W[cols, ks].t()
            part += p
        acc += part
    if not ktile_mut:
        cache[(order, splits)] = acc
    bias = case.bias.clone()
    csum = case.csum.clone()
    if mutation == "shift_side":                                              # the slice of the neighbouring 8-column group
        if fam in ("ln", "ln_qgelu"):
            csum = torch.roll(csum, -8)
        else:
            bias = torch.roll(bias, -8)
    b_eff = bias * float(splits) if mutation == "bias_per_slice" else bias
    res = {}
    if fam in ("ln", "ln_qgelu"):
        sf = (case.stats.double() / STAT_SCALE).float()
        if mutation == "ln_row_plus1":
            sf = sf.clone()
            sf[r] = sf[(r + 1) % M]
        invk = torch.tensor(1.0 / K, dtype=torch.float32)
        mean = sf[:, :1] * invk
        var = (sf[:, 1:] * invk - mean * mean).clamp_min(0.0)
        rstd = torch.rsqrt(var + torch.tensor(LN_EPS, dtype=torch.float32))
        nmr = -mean * rstd
        v = acc * rstd + (csum * nmr + b_eff)
    else:
        v = acc + b_eff
        if fam in ("resid", "resid_stats"):
            v = case.resid + v
            if mutation == "resid_twice":
                v[r] = case.resid[r] + v[r]
        elif fam == "patch":
            v = v + case.pos[1 + case.rows(M) % PATCH_G]
    if fam == "relu":
        v = v.clamp_min(0.0)
    if fam in ("qgelu", "ln_qgelu"):
        if op == F32:                                                         # gemm_f32_kernel: expf and a division
            v = v / (1.0 + torch.exp(-1.702 * v))
        else:
            v = v * (1.0 / (1.0 + torch.exp2(torch.tensor(QGELU_Z, dtype=torch.float32) * v)))
    if mutation == "swap_rows" and M >= 2:
        r2 = r + 1 if r + 1 < M else r - 1
        v = v.clone()
        v[[r, r2]] = v[[r2, r]]
    if fam == "resid_stats":
        sv, sq = v, v * v
        if mutation == "stats_miss16":
            keep = torch.ones(N, dtype=torch.bool)
            keep[c // 16 * 16:c // 16 * 16 + 16] = False
            row = torch.zeros(M, 1, dtype=torch.bool)
            row[r] = True
            sv, sq = torch.where(row & ~keep, 0.0, sv), torch.where(row & ~keep, 0.0, sq)
        parts = [(_fixed(sv[:, i:i + 64].sum(1)), _fixed(sq[:, i:i + 64].sum(1))) for i in range(0, N, 64)]   # one atomic per 64 columns
        st = torch.stack([sum(p[0] for p in parts), sum(p[1] for p in parts)], 1)
        if mutation == "stats_twice":
            st[r] = 2 * st[r]
        res["stats"] = st
    out = v.to(od)
    if mutation == "drop_store":                                              # one 16-byte store never leaves
        n8 = 16 // out.element_size()
        out[r, c // n8 * n8:c // n8 * n8 + n8] = SENTINEL
    if code == 8:
        res["copy"] = v.to(BF)
    if fam == "headf32":
        res["head"] = v.clone()
    if fam == "patch":
        full = torch.full((case.patch_out_rows(), N), SENTINEL, dtype=od)
        full[case.patch_rows()] = out
        out = full
    res["out"] = out
    return res


def _x3_acc(case, rows, order, mutation, at):
    """the fp32 accumulators of rows `rows` (a slice) of a split-operand launch: 3 K / 64 K-tiles, segment by segment"""
    np1, K = case.np1, case.K
    A = (case.ah[rows].float(), case.al[rows].float())
    W = (case.wh.float(), case.wl.float())
    acc = torch.zeros(A[0].shape[0], case.N)
    tile = lambda t, kt: t[:, kt * TILE_K:(kt + 1) * TILE_K]                   # noqa: E731
    ps = list(range(3 * np1)) + ([3 * np1 + i for i in range(np1)] if mutation == "x3_lo_lo" else [])
    for p in (ps if order == "forward" else reversed(ps)):
        kt, a_lo, w_lo = x3_seg(p, np1) if p < 3 * np1 else (p - 3 * np1, True, True)
        a, w = tile(A[a_lo], kt), tile(W[w_lo], kt)
        if p == np1 and mutation == "x3_hi_for_lo":                            # the seam's first tile still reads W's hi plane
            w = tile(W[0], kt)
        if p == np1 and mutation == "x3_koff_runs_on":                         # ... or counts its K offset on from segment 0: K-tile np1
            nxt = lambda t: torch.cat([t[1:], torch.zeros_like(t[:1])]).contiguous()   # noqa: E731  (dense rows: the next row's first tile)
            full_a = case.ah.float()
            a = tile(nxt(full_a), 0)[rows]
            w = tile(nxt(W[1]), 0)
        if mutation == "x3_drop_lo" and p == np1 + at["kt"]:
            continue
        if mutation == "x3_stale_lo" and p == 2 * np1 + at["kt"]:              # the ring still holds A of the K-tile two back
            if p < 2:
                continue
            k2, a2_lo, _ = x3_seg(p - 2, np1)
            a = tile(A[a2_lo], k2)
        acc += a @ w.t()
    return acc


def _emulate_x3(case, code, order, mutation, at):
    """emulate() for an X3Case -> dict(out fp32 [M, N]) or dict(hi, lo fp16 [M, N]) for X3_QGELU_PAIR"""
    assert str(case.device) == "cpu" and mutation in (None,) + X3_MUTATIONS
    _, od, fam = X3_EPILOGUES[code]
    M, N = case.M, case.N
    at = dict(row=0, col=0, kt=case.np1 - 1) | (at or {})
    r, c = at["row"], at["col"]
    piece = slice(r // 8 * 8, min(r // 8 * 8 + 8, M))
    cols = slice(c // 256 * 256, min(c // 256 * 256 + 256, N))
    cache = case.__dict__.setdefault("_model_acc", {})
    whole = mutation in ("x3_hi_for_lo", "x3_koff_runs_on", "x3_lo_lo")
    if whole:
        acc = _x3_acc(case, slice(0, M), order, mutation, at)
    else:
        if order not in cache:
            cache[order] = _x3_acc(case, slice(0, M), order, None, at)
        acc = cache[order]
        if mutation in ("x3_drop_lo", "x3_stale_lo"):
            acc = acc.clone()
            acc[piece, cols] = _x3_acc(case, piece, order, mutation, at)[:, cols]
    ws = torch.tensor(2.0 ** -case.w_exp, dtype=torch.float32)
    v = (acc + case.bias) * ws if mutation == "x3_scale_after_bias" else acc * ws + case.bias
    if fam == "resid":
        v = case.resid + v
    if fam != "qgelu_pair":
        out = v.clone()
        if mutation == "drop_store":
            out[r, c // 4 * 4:c // 4 * 4 + 4] = SENTINEL
        return {"out": out}
    v = v / (1.0 + torch.exp(-1.702 * v))
    hi = v.half()
    lo = (v - hi.float()).half()
    if mutation == "x3_lo_zero":
        lo = torch.zeros_like(lo)
    if mutation == "drop_store":
        hi[r, c // 8 * 8:c // 8 * 8 + 8] = SENTINEL
    return {"hi": hi, "lo": lo}


def fp16_ulp(h):
    """the spacing of fp16 at |h| (float64): 2^(floor(log2 |h|) - 10), 2^-24 below 2^-14"""
    _, ex = torch.frexp(h.double().abs())
    return torch.exp2((ex - 1).clamp_min(-14).double() - 10.0)


def _x3_failures(case, code, res):
    exp = expected(case, code)
    tag = f"{case.name}.{X3_NAMES[code]}"
    if code != 15:
        fs = [verify(res["out"][:case.M], exp, tag)]
    else:
        hi, lo = res["hi"][:case.M].double(), res["lo"][:case.M].double()
        fs = [check(hi + lo, exp, tag + " hi + lo"),
              _collect(lo.abs() / (0.5 * fp16_ulp(hi)), tag + " |lo| against ulp(hi) / 2")]
    # (the ratio reported is the bound's; |lo| reaches ulp(hi) / 2 exactly at every tie and says nothing more than pass or fail)
    return [f for f in fs if f], max(f.worst for f in fs if f or f is fs[0])


def model_failures(case, code, res):
    """every check of one launch's results `res` (emulate's dict, or the same built from a kernel's buffers) -> list of Failures,
    the failing ones only, and the worst ratio of all"""
    if isinstance(case, X3Case):
        return _x3_failures(case, code, res)
    op, od, fam = epilogues(case)[code]
    exp = expected(case, code)
    tag = f"{case.name}.{epilogue_name(case, code)}"
    out = res["out"][case.patch_rows()] if fam == "patch" else res["out"][:case.M]
    fs = [verify(out, exp, tag)]
    if fam == "headf32":
        fs.append(verify(res["head"], expected(case, code, F32).first_rows(res["head"].shape[0]), tag + " fp32 head"))
    if code == 8:
        same = res["copy"][:case.M] == out.to(BF)
        fs.append(_collect(torch.where(same, 0.0, float("inf")).double(), tag + " bf16 copy != bf16(out)"))
    if "stats" in res and res["stats"] is not None:
        st = res["stats"][:case.M]
        if case.exact:
            ok = stats_exact(exp.ref)
            fs.append(check_stats(st, exp.ref, None, True, tag, squares_only_by_bound=not ok))
        elif od == F32:
            fs.append(check_stats(st, out.double(), None, False, tag))            # of the values it stored
        else:                                                                     # of the fp32 sums whose fp16 roundings it stored
            o64 = out.double()
            fs.append(check_stats(st, o64, UNIT[od] * (1 + 2 * UNIT[od]) * o64.abs() + TINY[od], False, tag))
    worst = max(f.worst for f in fs)
    return [f for f in fs if f], worst
