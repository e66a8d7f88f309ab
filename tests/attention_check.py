"""Per-row checks of the attention kernels: cases whose rows are dominated by a mask error, a float64 reference on the rounded
operands, a per-element bound derived from the number formats, and a CPU model of the kernels' rounding with deliberate mask
mutations (tests/test_host_attention_check.py proves with it that the bound catches them).  Plain torch; imports without a GPU.

Layout (include/keds_hip.h): qkv [rows, 3 d] = q | k | v, head h at columns 64 h, d = 64 H; rectangular (B samples of S rows) or
packed (sample b = rows [offs[b], offs[b + 1])).

Regimes (make_qkv):
  random  N(0, 1.5^2) everywhere: what the whole-tensor tests use.  Softmax weights are spread unevenly; a single wrong key moves
          a row by less than the rounding error of the 16-bit forms.
  flat    q / 16, v + 2: attention is nearly uniform, every visible key weighs 1 / n and |o| ~ A ~ 2, so a missing or extra key
          with a non-zero value moves the row.  (It MISSES an unmasked zero pad key at S = 255 and 287 in bf16: the pad key dilutes
          the row by 1 / 256 = one bf16 ulp.  That is why `ramp` exists.)
  peaked  everything x 4: scores in the hundreds, softmax nearly one-hot: the maximum handling, and at S = 257 the recompute path.
  ramp    q = N(0, 0.5^2) + 1 and k_j = N(0, 0.5^2) - (3 - 2 j / S) on every dim: score / 8 grows with the key index from about -24
          to -8.  A zero pad key (score 0) or any later key that should be masked dominates the row, the last visible key is
          always among the heaviest, and at S = 257 the later key tiles sit ~23 log2 units above the first.

Bound of the 16-bit kernels, per element (bound()):
    |got - o| <= 1.05 u (A + |o|) + n_vis t vmax + t + 2^-20 vmax
with o = softmax(s) v and A = softmax(s) |v| in float64, u the unit roundoff of the type (P is rounded to it: u A, the sum being
taken over the unrounded P; the output is rounded to it: u |o|), t = 2^-25 for fp16 (P below 2^-14 rounds absolutely; every kernel
form has a row sum >= 1) and 0 for bf16, n_vis the keys the row may see, vmax = max |v| of the (sample, head); 1.05 and 2^-20 cover
second-order terms, fp32 accumulation and v_exp_f32.

Bound of the fp32-grade kernels (check_f32()): rho = max |err| / (A + |o|) of the kernel against rho of a plain float32 torch
evaluation of the same case on the CPU: rho_kernel <= max(4 rho_torch32, 2^-22).
"""
import math

import torch

DH = 64
S_EDGES = (1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 95, 96, 97, 128, 129, 255, 256, 257, 258, 272, 273, 287, 288)
REGIMES = ("random", "flat", "peaked", "ramp")
MUTATIONS = ("pad", "causal_lt", "causal_plus", "droplast", "swaprow")
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
F32_MARGIN, F32_FLOOR = 4.0, 2.0 ** -22
SL2 = 0.125 * 1.4426950408889634             # 1 / sqrt(64) * log2(e), as the kernels fold it


def offsets(B, S_or_lens):
    lens = [int(S_or_lens)] * B if isinstance(S_or_lens, int) else [int(n) for n in S_or_lens]
    assert len(lens) == B
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    return offs


def make_qkv(B, S_or_lens, H, regime, dtype, seed, device="cpu"):
    """qkv [rows, 3 * 64 H] already rounded to `dtype` (and of that dtype).  `regime`: one name, or one per sample."""
    offs = offsets(B, S_or_lens)
    regimes = [regime] * B if isinstance(regime, str) else list(regime)
    g = torch.Generator().manual_seed(seed)
    parts = []
    for b in range(B):
        n = offs[b + 1] - offs[b]
        x = torch.randn(n, 3, H, DH, generator=g, dtype=torch.float64)
        r = regimes[b]
        if r == "random":
            x *= 1.5
        elif r == "flat":
            x *= 1.5
            x[:, 0] /= 16.0
            x[:, 2] += 2.0
        elif r == "peaked":
            x *= 6.0
        elif r == "ramp":
            j = torch.arange(n, dtype=torch.float64).view(n, 1, 1)
            x[:, 0] = 0.5 * x[:, 0] + 1.0
            x[:, 1] = 0.5 * x[:, 1] - (3.0 - 2.0 * j / n)
            x[:, 2] *= 1.5
        else:
            raise ValueError(r)
        parts.append(x.reshape(n, 3 * H * DH))
    return torch.cat(parts).to(dtype).to(device)


def _heads(qkv, r0, r1, H, ft):
    """q, k, v of rows [r0, r1) as [H, n, 64] of type ft"""
    d = DH * H
    return tuple(t.to(ft).reshape(r1 - r0, H, DH).transpose(0, 1) for t in qkv[r0:r1].split(d, dim=1))


def _visible(n, causal, device, nk=None, mutation=None):
    """[n, nk] bool: may query i see key j"""
    nk = n if nk is None else nk
    i = torch.arange(n, device=device).view(n, 1)
    j = torch.arange(nk, device=device).view(1, nk)
    vis = (j < n) if mutation != "pad" else (j < nk)
    vis = vis.expand(n, nk).clone()
    if causal:
        vis &= (j < i) if mutation == "causal_lt" else (j <= i + 1) if mutation == "causal_plus" else (j <= i)
    if mutation == "droplast":
        vis &= j != n - 1
    return vis


class Case:
    """One launch's inputs and its float64 reference: o, A [rows, d]; vmax [rows, d] (max |v| of the row's (sample, head));
    nvis [rows, 1]; sample [rows] (index of the row's sample), local [rows] (row index inside its sample)."""

    def __init__(self, qkv, B, S_or_lens, H, causal, name=""):
        self.qkv, self.B, self.H, self.causal, self.name = qkv, B, H, bool(causal), name
        self.offs = offsets(B, S_or_lens)
        self.S = S_or_lens if isinstance(S_or_lens, int) else None
        self.dtype = qkv.dtype
        self.rows, self.d = self.offs[-1], DH * H
        assert qkv.shape == (self.rows, 3 * self.d)
        dev = qkv.device
        o, A, vmax, nvis, sample, local = [], [], [], [], [], []
        for b in range(B):
            r0, r1 = self.offs[b], self.offs[b + 1]
            n = r1 - r0
            q, k, v = _heads(qkv, r0, r1, H, torch.float64)
            s = q @ k.transpose(-1, -2) / 8.0
            vis = _visible(n, causal, dev)
            p = torch.softmax(s.masked_fill(~vis, float("-inf")), -1)
            o.append((p @ v).transpose(0, 1).reshape(n, self.d))
            A.append((p @ v.abs()).transpose(0, 1).reshape(n, self.d))
            vmax.append(v.abs().amax(dim=(1, 2)).repeat_interleave(DH).expand(n, self.d))
            nvis.append(vis.sum(1, keepdim=True).double())
            sample.append(torch.full((n,), b, dtype=torch.long, device=dev))
            local.append(torch.arange(n, device=dev))
        self.o, self.A, self.vmax, self.nvis = torch.cat(o), torch.cat(A), torch.cat(vmax), torch.cat(nvis)
        self.sample, self.local = torch.cat(sample), torch.cat(local)

    def bound(self):
        u, t = UNIT[self.dtype], TINY[self.dtype]
        return 1.05 * u * (self.A + self.o.abs()) + self.nvis * t * self.vmax + t + 2.0 ** -20 * self.vmax

    def row_mask(self, q_limit=None):
        """rows a launch with this q_limit computes"""
        return self.local < q_limit if q_limit else torch.ones_like(self.local, dtype=torch.bool)


class Failures(list):
    """(sample, head, row, ratio) of every failing row; .worst: the largest ratio of the rows that were checked; .limit: what a
    ratio may reach"""
    worst = 0.0
    limit = 1.0

    def __str__(self):
        head = f"{len(self)} rows beyond {self.limit:.3g} (worst ratio {self.worst:.3g}): "
        return head + ", ".join(f"(b{b} h{h} row{r}: {x:.3g})" for b, h, r, x in self[:40]) + (" ..." if len(self) > 40 else "")


def _collect(ratio, case, rows, limit):
    """ratio [rows, d] -> Failures over (row, head); a non-finite ratio (non-finite output) counts as infinite"""
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    per = ratio.reshape(case.rows, case.H, DH).amax(-1)                   # [rows, H]
    per = torch.where(rows.view(-1, 1), per, torch.zeros_like(per))
    out = Failures()
    out.limit = float(limit)
    out.worst = float(per.max()) if per.numel() else 0.0
    bad = (per > limit).nonzero().cpu().tolist()
    vals, smp, loc = per.cpu(), case.sample.cpu(), case.local.cpu()
    for r, h in bad:
        out.append((int(smp[r]), h, int(loc[r]), float(vals[r, h])))
    return out


def check(got, case, q_limit=None):
    """16-bit kernels: every (sample, head, row) of the first q_limit rows per sample whose worst |got - o| / bound exceeds 1."""
    ratio = (got[:case.rows].double() - case.o).abs() / case.bound()
    return _collect(ratio, case, case.row_mask(q_limit), 1.0)


def rel_err(got, case):
    """|got - o| / (A + |o|) per element (the scale of the fp32-grade check)"""
    return (got[:case.rows].double() - case.o).abs() / (case.A + case.o.abs())


def torch32(case):
    """The case in plain float32 torch on the CPU (float32 matmul, softmax, matmul): the yardstick of the fp32-grade kernels."""
    qkv = case.qkv.detach().cpu().float()
    outs = []
    for b in range(case.B):
        r0, r1 = case.offs[b], case.offs[b + 1]
        n = r1 - r0
        q, k, v = _heads(qkv, r0, r1, case.H, torch.float32)
        s = (q @ k.transpose(-1, -2)) / 8.0
        s = s.masked_fill(~_visible(n, case.causal, "cpu"), float("-inf"))
        outs.append((torch.softmax(s, -1) @ v).transpose(0, 1).reshape(n, case.d))
    return torch.cat(outs).to(case.qkv.device)


def rho_torch32(case, q_limit=None):
    r = rel_err(torch32(case), case)
    return float(r[case.row_mask(q_limit)].max())


def check_f32(got, case, q_limit=None, rho_ref=None, abs_floor=0.0):
    """fp32-grade kernels: rows whose rho = max |err| / (A + |o|) exceeds max(4 rho_torch32, 2^-22); .worst is rho_kernel and
    .limit the allowed value (rho_ref: rho_torch32 of the case when the caller has it already).
    abs_floor: an ABSOLUTE error that the number format of an operand or of the output implies and that no kernel can avoid; it is
    taken off |err| first.  0 for fp32 in, fp32 out.  The split-fp16 form carries a value below 2^-3 to an absolute 2^-25 (the
    low plane is an fp16 subnormal there, include/keds_hip.h): 2^-25 for its V operand (sum p = 1), another 2^-25 where the
    output itself is read from the planes.  It matters where A is tiny: a row that sees one or two keys whose v is near zero."""
    rho_ref = rho_torch32(case, q_limit) if rho_ref is None else rho_ref
    err = ((got[:case.rows].double() - case.o).abs() - abs_floor).clamp_min(0.0)
    return _collect(err / (case.A + case.o.abs()), case, case.row_mask(q_limit), max(F32_MARGIN * rho_ref, F32_FLOOR))


def emulate(qkv, B, S_or_lens, H, causal, mutation=None, first_tile=0):
    """The kernels' rounding on the CPU: fp32 scores, p = exp2((s - m) / 8 log2 e) in fp32, the row sum over the UNROUNDED p in
    fp32, p rounded to the operand type for the second product (fp32 accumulate), the quotient rounded to the type.
    first_tile = k > 0: m is the maximum over the first k keys only (the S = 257 kernel's first pass; it recomputes with the true
    maximum when that overflows).  mutation: a deliberate defect, see MUTATIONS."""
    dtype = qkv.dtype
    offs = offsets(B, S_or_lens)
    d = DH * H
    outs = []
    for b in range(B):
        r0, r1 = offs[b], offs[b + 1]
        n = r1 - r0
        q, k, v = _heads(qkv, r0, r1, H, torch.float32)
        nk = n
        if mutation == "pad":                       # the keys up to the next multiple of 16 exist as zero rows and are not masked
            nk = (n + 15) // 16 * 16
            z = torch.zeros(H, nk - n, DH)
            k, v = torch.cat([k, z], 1), torch.cat([v, z], 1)
        s = q @ k.transpose(-1, -2)                                         # fp32; products of 16-bit operands are exact
        vis = _visible(n, causal, "cpu", nk, mutation)
        s = s.masked_fill(~vis, float("-inf"))
        m = (s[..., :first_tile] if first_tile else s).amax(-1, keepdim=True)
        p = torch.exp2(s * SL2 - m * SL2)
        inv = 1.0 / p.sum(-1, keepdim=True)
        o = ((p.to(dtype).double() @ v.double()).float() * inv).to(dtype)
        o = o.transpose(0, 1).reshape(n, d)
        if mutation == "swaprow":
            o = torch.cat([o[:-2], o[-1:], o[-2:-1]])
        outs.append(o)
    return torch.cat(outs)


def applicable(mutation, S, causal):
    """Is the mutation a defect at all for this case?  causal_* need the mask, pad keys are hidden by the causal mask (and do not
    exist when S is a multiple of 16), and at S = 1 there is no second row or key to get wrong."""
    if mutation in ("causal_lt", "causal_plus"):
        return causal and S >= 2
    if mutation == "pad":
        return not causal and S % 16 != 0
    return S >= 2
