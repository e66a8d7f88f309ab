"""Every numerics guard per ROW and per ELEMENT, at kernel level (tests/guard_check.py: what each launch MUST, MUST NOT or MAY do, the
positions and the defect families they are chosen against; tests/test_host_guard_check.py: proof of the coverage).

One int32 slot per launch in one zeroed device array: keds_numerics_guard_set(slot i) before launch i (host state of the calling
thread), one synchronise per sweep, then every slot against the model; all mismatches of a sweep are collected before it asserts.
A failed launch ends the session (pytest.exit), as in test_gpu_gemm_edges.py, whose cases, force bits and recorded-form check are
reused: every launch of every sweep asserts the form keds_gemm_last_launch recorded.  The time of every sweep goes to the metrics
log, with the share of launches the model leaves open (EITHER) -- none of a planted target's."""
import ctypes
import functools
import time

import pytest
import torch

from keds_amd import _lib
from tests import gemm_check as gc
from tests import guard_check as gd
from tests.gpu_util import report
from tests.test_gpu_gemm_edges import (DEFER, F_NODEFER, F_PAIR, F_PERSIST, F_PROLOGUE, F_QUAD, F_SMALL, GUARD, PAIR, PROLOGUE, QUAD, QUAD3,
                                       SMALL, WS_BYTES, _expected_splits, _threshold)

pytestmark = pytest.mark.gpu

LN_CODES = (6, 7, 10, 11, 16, 17)
RESID_CODES = (9, 18)                                                # the fp16 residual stream: KEDS_EPI_RESID_STATS_F16 / _F16_H
F16_OUT = (16, 17, 20, 32, 33, 34)
KF16 = {32: "bias", 33: "relu", 34: "headf32"}                       # keds_knowledge_f16.h: 128^2 forms only
NAMES = dict(gc.NAMES) | {32: "BIAS_F16_H", 33: "BIAS_RELU_F16_H", 34: "BIAS_F16_H_HEADF32"}
ONE = int(gc.STAT_SCALE)
SENT = gc.SENTINEL


@pytest.fixture(scope="module", autouse=True)
def _workspace():
    """the 32 MiB split-K workspace of test_gpu_gemm_edges.py; the process-wide one and an empty guard come back afterwards"""
    lib = _lib.load()
    ws = torch.empty(WS_BYTES, dtype=torch.uint8, device="cuda")
    _lib.check(lib.keds_gemm_set_workspace(ws.data_ptr(), ws.numel()), "keds_gemm_set_workspace")
    try:
        yield
    finally:
        lib.keds_gemm_force_small(0)
        lib.keds_numerics_guard_set(None)
        old = _lib._gemm_ws.get(torch.cuda.current_device())
        lib.keds_gemm_set_workspace(old.data_ptr() if old is not None else None, old.numel() if old is not None else 0)
        _case.cache_clear()


@functools.lru_cache(maxsize=4)
def _case(M, N, K, dtype):
    return gc.Case(M, N, K, "random", dtype, seed=2, device="cuda")


def _dt(code):
    return gc.HF if code in KF16 else gc.EPILOGUES[code][0]


def _expected(case, code):
    """gemm_check.expected, and for ids 32 - 34 (its table has no rows for them) the plain form of test_gpu_knowledge_f16_edges.py"""
    if code not in KF16:
        return gc.expected(case, code)
    pre = case.acc + case.bias.double()
    e = case.e_acc() + 2 * gc.U32 * (case.S + case.bias.double().abs())
    return gc.Expected(pre.clamp_min(0.0) if KF16[code] == "relu" else pre, e, gc.HF, False)


class Slots:
    """one guard flag per launch, read once"""

    def __init__(self, label, capacity):
        self.label, self.flags = label, torch.zeros(capacity, dtype=torch.int32, device="cuda")
        self.names, self.expect, self.msgs, self.t0 = [], [], [], time.perf_counter()

    def next(self, name, expect):
        assert len(self.names) < self.flags.numel()
        self.names.append(name)
        self.expect.append(expect)
        return self.flags.data_ptr() + 4 * (len(self.names) - 1)

    def settle(self, planted_target=True):
        """-> number of launches; planted_target: no launch of this sweep may be EITHER"""
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:                 # a device fault: nothing more of this session may run on the card
            pytest.exit(f"{self.label}: {e}", returncode=3)
        got = self.flags[:len(self.names)].cpu().tolist()
        either = 0
        for name, want, g in zip(self.names, self.expect, got):
            if want == gd.EITHER:
                either += 1
                if planted_target:
                    self.msgs.append(f"{name}: the model leaves a planted target open")
            elif (g != 0) != (want == gd.MUST):
                self.msgs.append(f"{name}: flag {'raised' if g else 'down'}, the model says {want}")
        report(f"guard_edges.{self.label}", launches=len(got), either=either, seconds=time.perf_counter() - self.t0,
               mismatches=len(self.msgs))
        assert got, self.label
        assert not self.msgs, f"{self.label}: {len(self.msgs)} mismatches of {len(got)} launches:\n" + "\n".join(self.msgs[:30])
        return len(got)


# ---- the GEMM forms --------------------------------------------------------------------------------------------------------------
def _form_setup(name, code):
    """(force bits, recorded form to assert) of form `name` for epilogue `code`"""
    th = _threshold()
    M, N, K, row0 = gd.sweep_shape(name, th)
    plain = dict(tail=0, persistent=0, flags=0)
    if name in ("small4", "small4.strided"):
        return 0, dict(main=SMALL, ring=4, splits=1, **plain)
    if name == "small2":
        return F_SMALL, dict(main=SMALL, ring=2, splits=1, **plain)
    if name == "splitk":
        assert _expected_splits(M, N, K) == 16
        return 0, dict(main=SMALL, ring=4, splits=16, **plain)
    if name == "pair8":
        return F_PAIR, dict(main=PAIR, ring=2, splits=1, **plain)
    if name == "quad4":
        assert M // 256 * (N // 256) <= th
        return F_QUAD, dict(main=QUAD, ring=2, splits=1, **plain)
    if name == "quad4.persistent":
        assert M // 256 * (N // 256) > th
        return F_PERSIST | F_NODEFER, dict(main=QUAD, tail=0, ring=2, splits=1, persistent=1, flags=0)
    if name == "quad4.persistent.defer":
        assert M // 256 * (N // 256) > th and K // 64 >= 8 and code in (6, 10, 16)
        return F_PERSIST, dict(main=QUAD, tail=0, ring=2, splits=1, persistent=1, flags=DEFER)
    if name == "pair8.prologue":
        assert code in RESID_CODES
        return F_PROLOGUE | F_PAIR, dict(main=PAIR, tail=0, ring=2, splits=1, persistent=0, flags=PROLOGUE)
    if name == "quad3":
        assert code in RESID_CODES and K >= 1024
        return 0, dict(main=QUAD3, tail=0, ring=3, splits=1, persistent=0, flags=0)
    assert name == "remainder"
    return 0, dict(main=PAIR, tail=SMALL, tail_ring=4, tail_splits=1, splits=1, persistent=0)


def _codes_of(name, codes):
    if name == "quad4.persistent.defer":
        return tuple(c for c in codes if c in (6, 10, 16))           # what the plan defers: the LayerNorm-bias forms
    if name not in ("small4", "splitk"):
        return tuple(c for c in codes if c not in KF16)
    return codes


class Launcher:
    """the buffers of one (case, epilogue, form) and its launches.  A carries NaN rows behind M (and NaN columns behind K in the
    strided form); the statistics are allocated to whole 256-row tiles plus guard rows, all of them benign until planted."""

    def __init__(self, name, case, code, slots, M=None):
        self.name, self.case, self.code, self.slots = name, case, code, slots
        self.M, self.N, self.K = M or case.M, case.N, case.K
        M, N, K = self.M, self.N, self.K
        self.force, self.want = _form_setup(name, code)
        self.lda, self.ldc = (K + 72, N + 40) if name == "small4.strided" else (K, N)
        dt = _dt(code)
        od = gc.HF if code in KF16 else gc.EPILOGUES[code][1]
        self.A = torch.full((M + GUARD, self.lda), float("nan"), dtype=dt, device="cuda")
        self.A[:M, :K] = case.A[:M]
        self.out = torch.full((M + GUARD, self.ldc), SENT, dtype=od, device="cuda")
        self.ln = code in LN_CODES
        self.bias = torch.cat([case.bias, case.csum]) if self.ln else case.bias.clone()
        rows = (M + 255) // 256 * 256 + GUARD
        self.flat = torch.tensor([0, K * ONE], dtype=torch.int64, device="cuda")          # mean exactly 0, variance 1
        self.stats = self.flat.repeat(rows, 1) if self.ln else None
        self.other = torch.zeros(rows, 2, dtype=torch.int64, device="cuda") if self.ln else None
        self.aux, self.aux_i = self.stats, 0
        if code in RESID_CODES:                                       # the stream is read, added to and written in place
            self.resid = case.resid[:M].to(od)
            self.out[:M, :N] = self.resid
            self.aux = torch.zeros(rows, 2, dtype=torch.int64, device="cuda")
        if code == 34:
            self.aux_i = min(M, 130)
            self.aux = torch.full((self.aux_i + GUARD, 3, N), SENT, dtype=torch.float32, device="cuda")
        self.lib = _lib.load()
        P = _lib.ptr
        self.args = (P(self.A), self.lda, P(case.W), P(self.bias), P(self.out), self.ldc, M, N, K, code, P(self.aux), self.aux_i,
                     P(self.other), _lib.stream())
        self.info = (ctypes.c_int * 8)()
        self.label = f"{name}.{NAMES[code]}"

    def __enter__(self):
        _lib.check(self.lib.keds_gemm_force_small(self.force), "keds_gemm_force_small")
        return self

    def __exit__(self, *exc):
        self.lib.keds_gemm_force_small(0)
        self.lib.keds_numerics_guard_set(None)

    def go(self, tag, expect):
        lib = self.lib
        lib.keds_numerics_guard_set(self.slots.next(f"{self.label}.{tag}", expect))
        rc = lib.keds_gemm_bt_ex2(*self.args)
        if rc != 0:
            pytest.exit(f"{self.label}.{tag}: keds_gemm_bt_ex2 failed ({rc}): {_lib.last_error()}", returncode=3)
        lib.keds_gemm_last_launch(self.info)
        i = self.info
        got = dict(main=i[0], tail=i[1], ring=i[2], tail_ring=i[3], splits=i[4], tail_splits=i[5], persistent=i[6], flags=i[7])
        wrong = {k: (got[k], v) for k, v in self.want.items() if got[k] != v}
        if wrong:
            self.slots.msgs.append(f"{self.label}.{tag}: recorded kernel form differs (got, wanted): {wrong}")

    # -- models --
    def rows_case(self, rows, stats=None, csum=None, A=None, bias=None):
        c = gd.stack_case(self.case, rows, stats=stats, csum=csum, A=A)
        if bias is not None:
            c.bias = bias
        return c

    def range_of(self, case):
        """per row of `case`: MUST / MUST_NOT / EITHER of the range guard; MUST_NOT where the epilogue stores no fp16"""
        if self.code not in F16_OUT:
            return [gd.MUST_NOT] * case.M
        return [gd.code_of(v) for v in gd.range_rows(_expected(case, self.code)).cpu().tolist()]

    def base_range(self, stats=None):
        """the whole launch on its unplanted operands (statistics `stats`, default: flat)"""
        if self.code not in F16_OUT:
            return gd.MUST_NOT
        st = None
        if self.ln:
            st = (self.flat.repeat(self.M, 1) if stats is None else stats)
        return gd.combine(self.range_of(self.rows_case(list(range(self.M)), stats=st)))


def _signs(n):
    return [1 if i % 2 == 0 else -1 for i in range(n)]


# ---- 1. the ratio guard ----------------------------------------------------------------------------------------------------------
RATIO_FORMS = gd.LN_FORMS


@pytest.mark.parametrize("name", RATIO_FORMS)
def test_ratio_guard_every_row_of_every_form(name):
    """|row mean| / row std > 32, raised by one lane per row.  The statistics are an input of their own: planting is two int64 per
    row, A is untouched.  Per epilogue: every row of the form's tiles in turn at rho = 33 (MUST); every row at rho = 31 in one
    launch (MUST_NOT); the rows behind M, inside the tile-padded allocation, at rho = 1000 and INT64_MIN / INT64_MAX (MUST_NOT:
    the filler test_gpu_gemm_edges.py uses there is benign and cannot show a kernel that checks pad rows); extreme fixed-point
    values on a valid row, judged by the same float64 formula."""
    th = _threshold()
    M, N, K, row0 = gd.sweep_shape(name, th)
    pos = gd.sweep_positions(name, "ratio", th)
    codes = _codes_of(name, LN_CODES)
    slots = Slots(f"ratio.{name}", len(codes) * (len(pos) + 16))
    for code in codes:
        case = _case(M, N, K, _dt(code))
        with Launcher(name, case, code, slots) as L:
            base = L.base_range()
            assert base == gd.MUST_NOT, "the unplanted launch must be inside the fp16 range"
            sg = _signs(len(pos))
            plant = torch.tensor([gd.plant_stats(K, 33.0, s) for s in sg], dtype=torch.int64, device="cuda")
            rows = [o.m for o in pos]
            ratio = gd.ratio_rows(plant, K).cpu().tolist()
            rng = L.range_of(L.rows_case(rows, stats=plant))
            for i, o in enumerate(pos):
                L.stats[o.m].copy_(plant[i])
                L.go(f"rho33.m{o.m}.tile{o.tile}.r{o.r}", gd.combine([gd.code_of(ratio[i]), rng[i], base]))
                L.stats[o.m].copy_(L.flat)
            # every row at rho = 31
            all31 = torch.tensor([gd.plant_stats(K, 31.0, s) for s in _signs(M)], dtype=torch.int64, device="cuda")
            L.stats[:M].copy_(all31)
            L.go("rho31.everywhere", gd.combine([gd.ratio_expect(all31, K), L.base_range(all31)]))
            L.stats[:M].copy_(L.flat)
            # rows behind M
            pad = L.stats[M:]
            pad.copy_(torch.tensor(gd.plant_stats(K, 1000.0), dtype=torch.int64, device="cuda"))
            pad[1::3] = torch.tensor([gd.INT64_MIN, gd.INT64_MAX], dtype=torch.int64, device="cuda")
            pad[2::3] = torch.tensor([gd.INT64_MAX, gd.INT64_MIN], dtype=torch.int64, device="cuda")
            L.go("pad_rows.rho1000", gd.combine([gd.ratio_expect(L.stats[:M], K), base]))
            pad.copy_(L.flat)
            # extreme fixed-point values on a valid row
            for j, (s, ss) in enumerate(((0, -5 * K * ONE), (K * ONE, -5 * K * ONE), (gd.INT64_MAX, 0), (gd.INT64_MIN, gd.INT64_MAX),
                                         (0, gd.INT64_MAX), (-K * ONE, 0))):
                m = (row0, M - 1)[j % 2]
                row = torch.tensor([[s, ss]], dtype=torch.int64, device="cuda")
                L.stats[m].copy_(row[0])
                L.go(f"extreme.s{s}.ss{ss}.m{m}", gd.combine([gd.ratio_expect(row, K), L.range_of(L.rows_case([m], stats=row))[0], base]))
                L.stats[m].copy_(L.flat)
    slots.settle()


@pytest.mark.parametrize("name", ("small4", "small4.strided", "splitk"))
def test_ratio_guard_pad_rows_inside_a_ragged_tile(name):
    """M = 129: the second row tile has one valid row and 127 rows the kernel computes on but must not judge (it reads row M - 1's
    statistics for them); those rows hold rho = 1000 and INT64_MIN / INT64_MAX.  The last valid row at rho = 33 still raises."""
    th = _threshold()
    _, N, K, _ = gd.sweep_shape(name, th)
    M = 129
    slots = Slots(f"ratio.ragged.{name}", 4 * len(LN_CODES))
    for code in LN_CODES:
        case = _case(M, N, K, _dt(code))
        with Launcher(name, case, code, slots) as L:
            base = L.base_range()
            pad = L.stats[M:]
            pad.copy_(torch.tensor(gd.plant_stats(K, 1000.0, -1), dtype=torch.int64, device="cuda"))
            pad[1::2] = torch.tensor([gd.INT64_MAX, gd.INT64_MIN], dtype=torch.int64, device="cuda")
            L.go("pad_rows", gd.combine([gd.ratio_expect(L.stats[:M], K), base]))
            row = torch.tensor([gd.plant_stats(K, 33.0)], dtype=torch.int64, device="cuda")
            for m in (127, 128):
                L.stats[m].copy_(row[0])
                L.go(f"pad_rows.rho33.m{m}", gd.combine([gd.ratio_expect(L.stats[:M], K), L.range_of(L.rows_case([m], stats=row))[0], base]))
                L.stats[m].copy_(L.flat)
    slots.settle()


# ---- 2. the fp16 range guard -----------------------------------------------------------------------------------------------------
RANGE_CODES = (16, 17, 20, 32, 33, 34)
HOT, COOL = 7.0e4, 6.0e4


@pytest.mark.parametrize("name", RATIO_FORMS)
def test_range_guard_every_position_of_every_form(name):
    """One output of the launch beyond 65504, at both pairings of the form's tiles (guard_check.sweep_positions).  LayerNorm forms:
    planted through the side inputs only -- row m's statistics give nmr[m] = -20, every other row has mean exactly 0 (nmr = 0), and
    csum[c] = -+3500: v[m, c] = +-7e4, the rest of row m stays small (the reference proves it per launch).  Plain forms: row m of A
    becomes scale sign(W[c]) (test_gpu_fp16.py, _one_big_output).  Then every output near 6e4 in one launch (MUST_NOT), with NaN
    behind row M of A in every launch and behind column K in the strided form."""
    th = _threshold()
    M, N, K, row0 = gd.sweep_shape(name, th)
    pos = gd.sweep_positions(name, "range", th)
    codes = _codes_of(name, RANGE_CODES)
    slots = Slots(f"range.{name}", len(codes) * (len(pos) + 8))
    P = len(pos)
    rows = [o.m for o in pos]
    cols = torch.tensor([o.n for o in pos], device="cuda")
    ar = torch.arange(P, device="cuda")
    for code in codes:
        case = _case(M, N, K, _dt(code))
        post = code in (17, 20, 33)                                  # an activation in front of the store: a negative target is no target
        sg = torch.tensor([1 if post else s for s in _signs(P)], device="cuda", dtype=torch.float64)
        with Launcher(name, case, code, slots) as L:
            base = L.base_range()
            assert base == gd.MUST_NOT
            L.go("unplanted", base)
            if L.ln:
                hot = torch.tensor(gd.nmr_stats(K, -20.0), dtype=torch.int64, device="cuda")
                assert gd.ratio_expect(hot.unsqueeze(0), K) == gd.MUST_NOT
                csum = case.csum.repeat(P, 1)
                csum[ar, cols] = (-sg * (HOT / 20.0)).float()            # v = nmr csum = +-7e4
                model = L.rows_case(rows, stats=hot.repeat(P, 1), csum=csum)
                rng = L.range_of(model)
                planted_csum = csum[ar, cols].clone()
                keep = case.csum[cols].clone()
                cs = L.bias[N:]
                for i, o in enumerate(pos):
                    L.stats[o.m].copy_(hot)
                    cs[o.n].copy_(planted_csum[i])
                    L.go(f"hot.m{o.m}.n{o.n}.tile{o.tile}", gd.combine([rng[i], base]))
                    L.stats[o.m].copy_(L.flat)
                    cs[o.n].copy_(keep[i])
                # every output near 6e4
                cool = (torch.tensor(_signs(N), device="cuda") * (-COOL / 20.0)).float()
                allhot = hot.repeat(M, 1)
                cs.copy_(cool)
                L.stats[:M].copy_(allhot)
                e = gd.combine(L.range_of(L.rows_case(list(range(M)), stats=allhot, csum=cool)))
                L.go("cool.everywhere", gd.combine([e, gd.ratio_expect(allhot, K)]))
                cs.copy_(case.csum)
                L.stats[:M].copy_(L.flat)
            else:
                W = case.W
                scale = (sg * HOT / W[cols].double().abs().sum(1)).unsqueeze(1)
                Arows = (torch.sign(W[cols].double()) * scale).to(W.dtype)
                rng = L.range_of(L.rows_case(rows, A=Arows))
                keep = case.A[rows].clone()
                for i, o in enumerate(pos):
                    L.A[o.m, :K].copy_(Arows[i])
                    L.go(f"hot.m{o.m}.n{o.n}.tile{o.tile}", gd.combine([rng[i], base]))
                    L.A[o.m, :K].copy_(keep[i])
                # every output near 6e4: through the bias
                cool = (torch.tensor(_signs(N), device="cuda") * COOL).float()
                L.bias.copy_(cool)
                L.go("cool.everywhere", gd.combine(L.range_of(L.rows_case(list(range(M)), bias=cool))))
                L.bias.copy_(case.bias)
    n = slots.settle()
    assert n == len(codes) * (P + 2)


# ---- 3. keds_attention_x3 / keds_attention_x3_packed -----------------------------------------------------------------------------
X3_S = (1, 31, 32, 33, 257, 288)
X3_B, X3_H, X3_D = 2, 2, 128
X3_GUARD = 40                                 # rows in front of and behind the operand: 7e4 and NaN, never to be read


def _x3_positions(lengths, offsets):
    """(operand row, column) of every planted element: q, k, v x first / last sample x first / last head x rows 0, 31, 32, L - 1 x
    dims 0, 3, 4, 31, 32, 63"""
    out = []
    for t in range(3):
        for b in sorted({0, len(lengths) - 1}):
            for h in (0, X3_H - 1):
                for r in sorted({r for r in (0, 31, 32, lengths[b] - 1) if r < lengths[b]}):
                    for dim in (0, 3, 4, 31, 32, 63):
                        out.append((t, b, r, offsets[b] + r, t * X3_D + h * 64 + dim))
    return out


def _x3_sweep(label, lengths, launch, S, q_limit, packed):
    """plants one element per launch: a MUST value (rotating through the big value, +inf, -inf, NaN) and a MUST_NOT value"""
    offsets = [sum(lengths[:b]) for b in range(len(lengths))]
    rows = sum(lengths)
    g = torch.Generator(device="cuda").manual_seed(S * 7 + rows)
    buf = torch.randn(rows + 2 * X3_GUARD, 3 * X3_D, generator=g, device="cuda") * 1.5
    buf[:X3_GUARD] = 7.0e4
    buf[rows + X3_GUARD:] = float("nan")
    buf[rows + X3_GUARD + 1::2] = -7.0e4
    qkv = buf[X3_GUARD:X3_GUARD + rows]
    host = qkv.cpu()                                                  # the model judges this copy: no device read per launch
    model = host.clone()
    off_host = offsets + [rows] if packed else None
    seq_off = torch.tensor(offsets + [rows], dtype=torch.int32, device="cuda") if packed else None
    pos = _x3_positions(lengths, offsets)
    slots = Slots(label, 2 * len(pos) + 1)
    claim_free = 0
    launch(qkv, seq_off, slots.next("unplanted", gd.x3_expect(model, len(lengths), S, X3_D, q_limit, off_host)))
    for i, (t, b, r, row, col) in enumerate(pos):
        hot = ((5.3e5, 7.0e4, 7.0e4)[t], float("inf"), float("-inf"), float("nan"), -(5.3e5, 7.0e4, 7.0e4)[t])[i % 5]
        cool = (4.0e5, 6.5e4, 6.5e4)[t] * (1 if i % 2 else -1)
        for tag, val in (("hot", hot), ("cool", cool)):
            qkv[row, col] = val
            model[row, col] = val
            want = gd.x3_expect(model, len(lengths), S, X3_D, q_limit, off_host)
            if want == gd.EITHER:                                    # a q row the launch does not compute: the header makes no claim
                assert t == 0 and q_limit > 0 and r >= q_limit
                claim_free += 1
            else:
                assert want == (gd.MUST if tag == "hot" else gd.MUST_NOT)
            launch(qkv, seq_off, slots.next(f"{'qkv'[t]}.b{b}.row{r}.col{col}.{tag}{val:g}", want))
            qkv[row, col] = float(host[row, col])
            model[row, col] = host[row, col]
    n = slots.settle(planted_target=False)
    either = sum(e == gd.EITHER for e in slots.expect)
    assert either == claim_free
    report(f"guard_edges.{label}.either_share", share=either / n)


@pytest.mark.parametrize("q_limit", (0, 1))
@pytest.mark.parametrize("causal", (0, 1))
@pytest.mark.parametrize("S", X3_S)
def test_attention_x3_overflow_flag_every_operand_position(S, causal, q_limit):
    """one element of q, k or v beyond what an fp16 hi plane holds -- |q / 8|, |k|, |v| >= 65504, +-inf, NaN -- raises the flag
    wherever it sits; 4e5 in q (inside after the exact / 8) and 6.5e4 in k or v do not; rows in front of and behind the operand hold
    7e4 and NaN and are never read (keys S .. SP of the last sample would be)."""
    lib = _lib.load()
    out = torch.zeros(X3_B * S, X3_D, device="cuda")

    def launch(qkv, seq_off, flag):
        rc = lib.keds_attention_x3(qkv.data_ptr(), _lib.ptr(out), None, 0, X3_B, S, X3_H, causal, q_limit, flag, _lib.stream())
        if rc != 0:
            pytest.exit(f"keds_attention_x3 S{S}: {_lib.last_error()}", returncode=3)
    _x3_sweep(f"x3.S{S}.causal{causal}.q{q_limit}", [S] * X3_B, launch, S, q_limit, False)


@pytest.mark.parametrize("causal", (0, 1))
@pytest.mark.parametrize("S", X3_S)
def test_attention_x3_packed_overflow_flag_every_operand_position(S, causal):
    """the same on packed rows: two ragged samples (S and S // 2 + 1 rows), every query row of every sample"""
    lib = _lib.load()
    lengths = [S // 2 + 1, S]
    out = torch.zeros(sum(lengths), X3_D, device="cuda")

    def launch(qkv, seq_off, flag):
        rc = lib.keds_attention_x3_packed(qkv.data_ptr(), _lib.ptr(out), None, 0, len(lengths), S, _lib.ptr(seq_off), X3_H, causal, flag,
                                          _lib.stream())
        if rc != 0:
            pytest.exit(f"keds_attention_x3_packed S{S}: {_lib.last_error()}", returncode=3)
    _x3_sweep(f"x3_packed.S{S}.causal{causal}", lengths, launch, S, 0, True)


# ---- 4. keds_split_f16_pair ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", (8, 128, 136))
@pytest.mark.parametrize("rows", (1, 255, 256, 257))
def test_split_f16_pair_overflow_flag_every_position(rows, cols):
    """+-65504, 7e4, +-inf or NaN at every (row class, column class) -- first, middle and last row, the rows on either side of a
    256-thread block edge, the first and last element of the first and last 8-element group -- raises the flag; the largest value
    below 65504 there does not; the stride gap (ld = cols + 4) holds NaN and is not read."""
    lib = _lib.load()
    ld = cols + 4
    g = torch.Generator(device="cuda").manual_seed(rows * 131 + cols)
    src = torch.full((rows, ld), float("nan"), device="cuda")
    src[:, :cols] = torch.randn(rows, cols, generator=g, device="cuda") * 3.0
    host = src.cpu()
    model = host.clone()
    plane = rows * cols + 64
    out = torch.zeros(2 * plane, dtype=torch.float16, device="cuda")
    per_row = cols // 8
    edge = {(256 * k) // per_row for k in range(1, 1 + rows * per_row // 256)}            # rows that hold a block's first thread
    rws = sorted(r for r in {0, rows // 2, rows - 1} | edge | {e - 1 for e in edge} if 0 <= r < rows)
    cls = sorted({0, 7, 8, cols // 2, cols - 8, cols - 1} & set(range(cols)))
    hot = (65504.0, -65504.0, 7.0e4, float("inf"), float("-inf"), float("nan"), -7.0e4)
    slots = Slots(f"split.{rows}x{cols}", 2 * len(rws) * len(cls) + 1)

    def launch(name):
        want = gd.split_expect(model[:, :cols])
        rc = lib.keds_split_f16_pair(_lib.ptr(src), ld, rows, cols, _lib.ptr(out), plane, slots.next(name, want), _lib.stream())
        if rc != 0:
            pytest.exit(f"keds_split_f16_pair {rows} x {cols}: {_lib.last_error()}", returncode=3)
        return want
    assert launch("unplanted.nan_in_the_stride_gap") == gd.MUST_NOT
    i = 0
    for r in rws:
        for c in cls:
            for tag, val, want in (("hot", hot[i % len(hot)], gd.MUST), ("cool", 65503.99609375 * (1 if i % 2 else -1), gd.MUST_NOT)):
                src[r, c] = val
                model[r, c] = val
                assert launch(f"r{r}.c{c}.{tag}{val:g}") == want
                src[r, c] = float(host[r, c])
                model[r, c] = host[r, c]
            i += 1
    slots.settle()


# ---- 5. the fp16 residual stream's own check: KEDS_EPI_RESID_STATS_F16 / _F16_H in every form, keds_rowstats_cast_ex ------------
@pytest.mark.parametrize("name", gd.STREAM_FORMS)
def test_stream_guard_every_position_of_every_form(name):
    """keds_f16_stream_bad: the lane that holds a 64-column partial sum of squares of the values a residual epilogue stores raises the
    flag at 65504^2.  One stored value beyond the range per launch, at both pairings of the form's tiles, planted through the residual
    tile and the bias so that A stays untouched and the launch stays one-hot: resid[m, c] = +-60000 with bias[c] = +-10000 (v = +-7e4;
    every other row gets 1e4 in that column, far inside), or resid[m, c] = +-inf / NaN.  Then one value of 6e4 per 64-column group of
    every row (partial 3.6e9 < 65504^2: MUST_NOT), and two per group (7.2e9, no value beyond the range: the widened contract, EITHER,
    reported).  The stream is restored in front of every launch (it is updated in place); rows behind M of A hold NaN."""
    th = _threshold()
    M, N, K, row0 = gd.sweep_shape(name, th)
    pos = gd.sweep_positions(name, "range", th)
    P = len(pos)
    slots = Slots(f"stream.{name}", len(RESID_CODES) * (P + 4))
    grey = Slots(f"stream.{name}.grey", len(RESID_CODES))
    rows = [o.m for o in pos]
    idx = torch.tensor(rows, device="cuda")
    cols = torch.tensor([o.n for o in pos], device="cuda")
    ar = torch.arange(P, device="cuda")
    kind = ar % 4                                                    # +7e4, -7e4, +-inf, NaN
    sg = torch.where((ar // 4) % 2 == 0, 1.0, -1.0)
    inf = torch.tensor(float("inf"), device="cuda")
    nan = torch.tensor(float("nan"), device="cuda")
    plant_r = torch.where(kind == 0, 60000.0, torch.where(kind == 1, -60000.0, torch.where(kind == 2, sg * inf, nan))).float()
    plant_b = torch.where(kind == 0, 10000.0, torch.where(kind == 1, -10000.0, 0.0)).float()
    for code in RESID_CODES:
        case = _case(M, N, K, _dt(code))
        with Launcher(name, case, code, slots) as L:
            base = _expected(L.rows_case(list(range(M))), code)
            assert bool((gd.stream_rows(base) == -1).all()), "the unplanted launch must be far inside"
            p0, v0 = float(gd.stream_partials(base).max()), float((base.ref.abs() + base.bound).max())
            assert p0 + (1.0e4 + v0) ** 2 < gd.STREAM_SAFE            # the rows that only see the planted bias column
            L.go("unplanted", gd.MUST_NOT)
            model = L.rows_case(rows)
            model.resid = case.resid[idx].clone()
            model.resid[ar, cols] = plant_r
            model.bias = case.bias.repeat(P, 1)
            model.bias[ar, cols] = torch.where(kind < 2, plant_b, case.bias[cols])
            want = [gd.code_of(v) for v in gd.stream_rows(_expected(model, code)).cpu().tolist()]
            r16, pb, keep = plant_r.to(L.out.dtype), model.bias[ar, cols].clone(), case.bias[cols].clone()
            live = L.out[:M, :N]
            for i, o in enumerate(pos):
                live.copy_(L.resid)
                L.out[o.m, o.n].copy_(r16[i])
                L.bias[o.n].copy_(pb[i])
                L.go(f"hot{int(kind[i])}.m{o.m}.n{o.n}.tile{o.tile}", want[i])
                L.bias[o.n].copy_(keep[i])
            # one 6e4 per 64-column group of every row; then two
            for tag, cols6, sl in (("cool", (5,), slots), ("grey", (5, 37), grey)):
                b = case.bias.clone()
                for c6 in cols6:
                    b[c6::64] = torch.tensor(_signs(len(b[c6::64])), device="cuda") * COOL
                e = gd.stream_rows(_expected(L.rows_case(list(range(M)), bias=b), code))
                exp = gd.MUST_NOT if bool((e == -1).all()) else gd.MUST if bool((e == 1).any()) else gd.EITHER
                assert exp == (gd.MUST_NOT if tag == "cool" else gd.EITHER)
                live.copy_(L.resid)
                L.bias.copy_(b)
                L.slots = sl
                L.go(f"{tag}.every_row", exp)
                L.slots = slots
                L.bias.copy_(case.bias)
    assert slots.settle() == len(RESID_CODES) * (P + 2)
    grey.settle(planted_target=False)
    report(f"guard_edges.stream.{name}.grey_raised", raised=int(grey.flags[:len(grey.names)].sum()), of=len(grey.names))


@pytest.mark.parametrize("dim", (128, 768, 1024))
def test_rowstats_cast_stream_guard_every_lane(dim):
    """keds_rowstats_cast_ex with out_f16: one wave per row, lane l holds the 4-element chunks l, l + 64, ...; a value beyond +-65504,
    +-inf or NaN in any chunk of the first row, of both sides of a 4-row block edge and of the last row raises the thread's flag; 6e4
    there does not; two 6e4 in one chunk are the widened contract (EITHER, reported).  The bf16 instantiation never raises."""
    lib = _lib.load()
    rows = 9
    g = torch.Generator(device="cuda").manual_seed(dim)
    x = torch.randn(rows, dim, generator=g, device="cuda") * 2.0
    host = x.cpu()
    model = host.clone()
    xb = torch.zeros(rows + 8, dim, dtype=torch.float16, device="cuda")
    stats = torch.zeros(rows + 8, 2, dtype=torch.int64, device="cuda")
    chunks = dim // 4
    pos = [(r, q) for r in (0, 3, 4, rows - 1) for q in range(chunks)]
    slots = Slots(f"rowstats.{dim}", 3 * len(pos) + 2)
    grey = Slots(f"rowstats.{dim}.grey", 4)
    hot = (7.0e4, float("inf"), -7.0e4, float("nan"), float("-inf"), 65536.0)

    def launch(sl, name, f16, want):
        lib.keds_numerics_guard_set(sl.next(name, want))
        rc = lib.keds_rowstats_cast_ex(_lib.ptr(x), _lib.ptr(xb), int(f16), _lib.ptr(stats), rows, dim, _lib.stream())
        if rc != 0:
            pytest.exit(f"keds_rowstats_cast_ex {rows} x {dim}: {_lib.last_error()}", returncode=3)
    try:
        launch(slots, "unplanted", True, gd.stream_expect_values(model, 4))
        for i, (r, q) in enumerate(pos):
            c = 4 * q + i % 4
            for tag, val, want in (("hot", hot[i % len(hot)], gd.MUST), ("cool", COOL * (1 if i % 2 else -1), gd.MUST_NOT)):
                x[r, c] = val
                model[r, c] = val
                assert gd.stream_expect_values(model, 4) == want
                launch(slots, f"r{r}.chunk{q}.lane{q % 64}.{tag}{val:g}", True, want)
                if tag == "hot":
                    launch(slots, f"r{r}.chunk{q}.bf16.{val:g}", False, gd.MUST_NOT)
                x[r, c] = float(host[r, c])
                model[r, c] = host[r, c]
        for r, q in ((0, 0), (rows - 1, chunks - 1)):
            x[r, 4 * q:4 * q + 2] = COOL
            model[r, 4 * q:4 * q + 2] = COOL
            assert gd.stream_expect_values(model, 4) == gd.EITHER
            launch(grey, f"r{r}.chunk{q}.two_6e4", True, gd.EITHER)
            x[r, 4 * q:4 * q + 2] = host[r, 4 * q:4 * q + 2].cuda()
            model[r, 4 * q:4 * q + 2] = host[r, 4 * q:4 * q + 2]
    finally:
        lib.keds_numerics_guard_set(None)
    slots.settle()
    grey.settle(planted_target=False)
    report(f"guard_edges.rowstats.{dim}.grey_raised", raised=int(grey.flags[:len(grey.names)].sum()), of=len(grey.names))
