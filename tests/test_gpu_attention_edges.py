"""Every attention kernel form per ROW, at its tile and mask edges (tests/attention_check.py: the cases, the float64 reference and
the bounds; tests/test_host_attention_check.py: proof that the bound catches one wrong key in one row).

B = 3, H = 3 everywhere: nine workgroups hit every value of the odd-tile wave rotation, an odd head count catches a head-stride
error.  Each test loops the sequence lengths and collects the failing rows of the whole loop before it asserts."""
import ctypes
import functools

import pytest
import torch

from keds_amd import _lib
from tests import attention_check as ac
from tests.gpu_util import report

pytestmark = pytest.mark.gpu

B, H = 3, 3
D = ac.DH * H
GUARD = 64                                   # rows behind the last sample that no launch may touch
SENTINEL = -777.0
DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32, "x3": torch.float32}
ENTRIES = ("bf16", "fp16", "f32", "x3")      # keds_attention_ex, keds_attention_h, keds_attention_f32, keds_attention_x3
MASKS = pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
X3_OUT_FLOOR, X3_PLANE_FLOOR = 2.0 ** -25, 2.0 ** -24     # attention_check.check_f32: what the split-fp16 format itself implies
GENERIC, TAIL1, S257 = _lib.ATTN_FORM_GENERIC, _lib.ATTN_FORM_TAIL1, _lib.ATTN_FORM_S257
F_CAUSAL, F_F16, F_Q8, F_PACKED, F_STOP = (_lib.ATTN_FLAG_CAUSAL, _lib.ATTN_FLAG_F16, _lib.ATTN_FLAG_Q8, _lib.ATTN_FLAG_PACKED,
                                            _lib.ATTN_FLAG_STOP_EVENT)


@functools.lru_cache(maxsize=None)
def _case(S, regime, dtype, causal):
    """one reference per (S, regime, type, mask), shared by every test of this module and never written to"""
    qkv = ac.make_qkv(B, S, H, regime, dtype, seed=S, device="cuda")
    return ac.Case(qkv, B, S, H, causal, name=f"S{S}.{regime}")


@functools.lru_cache(maxsize=None)
def _rho32(S, regime, causal, q_limit=None):
    return ac.rho_torch32(_case(S, regime, torch.float32, causal), q_limit)


def _buffer(rows, dtype):
    return torch.full((rows + GUARD, D), SENTINEL, dtype=dtype, device="cuda")


def _untouched(t):
    return bool((t == torch.tensor(SENTINEL, dtype=t.dtype, device=t.device)).all())


def _recorded(lib):
    """keds_attention_last_launch -> [form, nkt, nfull, flags, grid, block, lds, q_limit]: what the launch site wrote"""
    info = (ctypes.c_int * 8)()
    _lib.check(lib.keds_attention_last_launch(info), "keds_attention_last_launch")
    return list(info)


def _recorded_is_planned(lib, Bn, S, heads, causal, q_limit, f16=0, q8=0, packed=0):
    """the record of the launch just made equals keds_attention_plan_query under the hook in force, all eight ints -> the record"""
    plan = (ctypes.c_int * 8)()
    _lib.check(lib.keds_attention_plan_query(Bn, S, heads, int(causal), q_limit, f16, q8, packed, plan), "keds_attention_plan_query")
    got = _recorded(lib)
    assert got == list(plan), f"S{S} causal={causal} q_limit={q_limit} f16={f16} q8={q8} packed={packed}: recorded {got}, planned {list(plan)}"
    return got


def _run(entry, case, q_limit=0):
    """-> (out buffer with guard rows, planes [2, rows + GUARD, D] or None)"""
    lib = _lib.load()
    S, c = case.S, int(case.causal)
    out = _buffer(case.rows, DTYPE[entry])
    P, st = _lib.ptr, _lib.stream()
    if entry == "bf16":
        _lib.check(lib.keds_attention_ex(P(case.qkv), P(out), B, S, H, c, q_limit, st), "keds_attention_ex")
        _recorded_is_planned(lib, B, S, H, c, q_limit)
    elif entry == "fp16":
        _lib.check(lib.keds_attention_h(P(case.qkv), P(out), B, S, H, c, q_limit, st), "keds_attention_h")
        _recorded_is_planned(lib, B, S, H, c, q_limit, f16=1)
    elif entry == "f32":
        _lib.check(lib.keds_attention_f32(P(case.qkv), P(out), B, S, H, c, q_limit, st), "keds_attention_f32")
    else:
        plane = (case.rows + GUARD) * D
        pair = torch.full((2, case.rows + GUARD, D), SENTINEL, dtype=torch.float16, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        _lib.check(lib.keds_attention_x3(P(case.qkv), P(out), P(pair), plane, B, S, H, c, q_limit, P(flag), st), "keds_attention_x3")
        only = torch.full_like(pair, SENTINEL)                        # planes only: the whole-line store path; the same bits
        _lib.check(lib.keds_attention_x3(P(case.qkv), None, P(only), plane, B, S, H, c, q_limit, P(flag), st), "keds_attention_x3 (planes)")
        assert int(flag.item()) == 0, f"{case.name}: range flag raised"
        assert torch.equal(only, pair), f"{case.name}: planes-only launch differs from the out + planes launch"
        return out, pair
    return out, None


def _verify(entry, case, regime, out, planes, q_limit=None, tag=""):
    """-> (list of messages, worst ratio).  16-bit: ratio against the bound; fp32 grade: rho against max(4 rho_torch32, 2^-22)"""
    msgs = []
    name = f"{case.name}{tag}" + (f".q{q_limit}" if q_limit else "")
    if entry in ("bf16", "fp16"):
        f = ac.check(out, case, q_limit)
        report(f"attention_edges.{entry}.{'causal' if case.causal else 'full'}.{name}", worst_ratio=f.worst)
        if f:
            msgs.append(f"{name}: {f}")
        return msgs, f.worst
    rho_t = _rho32(case.S, regime, case.causal, q_limit)
    floor = X3_OUT_FLOOR if entry == "x3" else 0.0
    f = ac.check_f32(out, case, q_limit, rho_t, abs_floor=floor)
    raw = ac.check_f32(out, case, q_limit, rho_t).worst
    rec = dict(rho_kernel=f.worst, rho_kernel_no_floor=raw, rho_torch32=rho_t, limit=f.limit)
    if f:
        msgs.append(f"{name}: out {f}")
    worst = f.worst / f.limit
    if planes is not None:
        rows = case.row_mask(q_limit)
        o = out[:case.rows][rows]
        hi = o.half()
        lo = (o - hi.float()).half()
        if not (torch.equal(planes[0, :case.rows][rows], hi) and torch.equal(planes[1, :case.rows][rows], lo)):
            msgs.append(f"{name}: the planes are not the fp16 split (hi, lo) of the fp32 output")
        fp = ac.check_f32(planes[0].double() + planes[1].double(), case, q_limit, rho_t, abs_floor=X3_PLANE_FLOOR)
        rec["rho_planes"] = fp.worst
        if fp:
            msgs.append(f"{name}: planes {fp}")
        worst = max(worst, fp.worst / fp.limit)
    report(f"attention_edges.{entry}.{'causal' if case.causal else 'full'}.{name}", **rec)
    return msgs, worst


# ---- rectangular ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ac.REGIMES)
@MASKS
@pytest.mark.parametrize("entry", ENTRIES)
def test_attention_rows_at_every_edge_length(entry, causal, regime):
    """S over every tile edge of every kernel form (1, 2, 16 k +- 1, the dispatch thresholds 32 | 33, 96 | 97, 255 .. 258, 288), all
    rows against float64 per element; 64 guard rows behind the output stay untouched.  At S = 257 the 4-wave tail kernel and the
    generic kernel (keds_attention_debug 32 / 16) run on the same case.  The 16-bit entries' launch record equals the plan at every
    length (_run), and at S = 257 it names the form each hook asks for: a hook that stopped routing fails here, not only in the numerics."""
    lib = _lib.load()
    msgs, worst, worst_at = [], 0.0, None
    for S in ac.S_EDGES:
        case = _case(S, regime, DTYPE[entry], causal)
        forms = [("", 0)]
        if S == 257 and not causal and entry in ("bf16", "fp16"):
            forms += [(".tail4", 32), (".generic", 16)]
        for tag, hook in forms:
            try:
                lib.keds_attention_debug(hook)
                out, planes = _run(entry, case)
                rec = _recorded(lib)
            finally:
                lib.keds_attention_debug(0)
            if S == 257 and not causal and entry in ("bf16", "fp16"):
                want = {0: [S257, 16, 16], 32: [TAIL1, 16, 16], 16: [GENERIC, 18, 16]}[hook]
                if rec[:3] != want:
                    msgs.append(f"S257{tag}: hook {hook} recorded (form, nkt, nfull) {rec[:3]}, wanted {want}")
            m, w = _verify(entry, case, regime, out, planes, tag=tag)
            msgs += m
            if w > worst:
                worst, worst_at = w, f"S{S}{tag}"
            if not _untouched(out[case.rows:]) or (planes is not None and not _untouched(planes[:, case.rows:])):
                msgs.append(f"S{S}{tag}: guard rows written")
    report(f"attention_edges.{entry}.{'causal' if causal else 'full'}.{regime}", worst_ratio=worst, at=worst_at, lengths=len(ac.S_EDGES))
    assert not msgs, "\n".join(msgs)


# ---- q_limit -------------------------------------------------------------------------------------------------------------------
@MASKS
@pytest.mark.parametrize("entry", ENTRIES)
def test_attention_q_limit_rows_and_guards(entry, causal):
    """Only the first q_limit rows of every sample are computed and stored: those pass the per-row check (16-bit forms: the same
    bits as the full launch), every other row and the guard rows keep the sentinel -- the planes of the split form too."""
    msgs, worst = [], 0.0
    for regime in ("ramp", "random"):
        for S in (33, 97, 257, 288):
            case = _case(S, regime, DTYPE[entry], causal)
            full, _ = _run(entry, case)
            for ql in sorted({min(q, S) for q in (1, 15, 16, 17, 33, S - 1)}):
                out, planes = _run(entry, case, ql)
                m, w = _verify(entry, case, regime, out, planes, q_limit=ql)
                msgs += m
                worst = max(worst, w)
                computed = torch.cat([case.row_mask(ql), torch.zeros(GUARD, dtype=torch.bool, device="cuda")])
                if not _untouched(out[~computed]) or (planes is not None and not _untouched(planes[:, ~computed])):
                    msgs.append(f"{case.name}.q{ql}: a row at or beyond q_limit, or a guard row, was written")
                if entry in ("bf16", "fp16") and not torch.equal(out[computed], full[computed]):
                    msgs.append(f"{case.name}.q{ql}: rows differ from the full launch")
    report(f"attention_edges.q_limit.{entry}.{'causal' if causal else 'full'}", worst_ratio=worst)
    assert not msgs, "\n".join(msgs)


# ---- packed rows ---------------------------------------------------------------------------------------------------------------
LENS = [1, 15, 16, 17, 32, 33, 77, 2, 96, 97]
PACKED = [("s97", LENS, 97), ("s288", LENS, 288), ("s32", [5, 31, 1, 32], 32)]     # the three instantiation classes: 18, 6 and 2 key tiles


@pytest.mark.parametrize("name,lens,s_max", PACKED, ids=[p[0] for p in PACKED])
@MASKS
@pytest.mark.parametrize("entry", ["bf16", "fp16"])
def test_attention_packed_rows(entry, causal, name, lens, s_max):
    """keds_attention_packed / _packed_h with per-sample offsets, both masks, s_max equal to and far above the longest sample.  Even
    samples are `ramp`, odd ones `random`: a key read from a neighbour into a ramp sample dominates its rows."""
    lib = _lib.load()
    n = len(lens)
    qkv = ac.make_qkv(n, lens, H, ["ramp" if b % 2 == 0 else "random" for b in range(n)], DTYPE[entry], seed=1000 + s_max, device="cuda")
    case = ac.Case(qkv, n, lens, H, causal, name=f"packed.{name}")
    offs = torch.tensor(case.offs, dtype=torch.int32, device="cuda")
    out = _buffer(case.rows, DTYPE[entry])
    fn = lib.keds_attention_packed if entry == "bf16" else lib.keds_attention_packed_h
    _lib.check(fn(_lib.ptr(qkv), _lib.ptr(out), n, s_max, _lib.ptr(offs), H, int(causal), _lib.stream()), "keds_attention_packed")
    rec = _recorded_is_planned(lib, n, s_max, H, causal, s_max, f16=int(entry == "fp16"), packed=1)
    assert rec[:4] == [GENERIC, {32: 2, 97: 18, 288: 18}[s_max], 0, F_CAUSAL * causal | F_F16 * (entry == "fp16") | F_PACKED], rec
    f = ac.check(out, case)
    report(f"attention_edges.packed.{entry}.{'causal' if causal else 'full'}.{name}", worst_ratio=f.worst)
    assert not f, str(f)
    assert _untouched(out[case.rows:]), "guard rows written"


# ---- MXFP8 output --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,causal,rows8", [(77, True, 100), (257, False, 300), (33, False, 16)])
def test_attention_mx_boundary_inside_a_sample_and_a_tile(S, causal, rows8):
    """keds_attention_mx with q8_rows falling inside a sample and inside a 16-query tile, by the method of
    test_attention_mxfp8_output_equals_quantised_bf16_path: bf16 rows bit-equal to the plain launch, MX rows decode to within its
    4e-2 and re-quantise to themselves, `out` rows below q8_rows untouched."""
    from tests.gpu_util import rel_l2
    from tests.test_gpu_fp8 import _dequantize, _torch_mx
    lib = _lib.load()
    Hm = 4                                                              # width 256: a multiple of 128
    d = Hm * 64
    g = torch.Generator(device="cuda").manual_seed(9 + S)
    qkv = (torch.randn(B * S, 3 * d, generator=g, device="cuda") * 1.2).to(torch.bfloat16)
    ref = torch.zeros((B * S, d), dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.keds_attention_ex(_lib.ptr(qkv), _lib.ptr(ref), B, S, Hm, int(causal), S, _lib.stream()), "keds_attention_ex")
    out = torch.full((B * S + GUARD, d), SENTINEL, dtype=torch.bfloat16, device="cuda")
    q8 = torch.zeros((rows8, d), dtype=torch.uint8, device="cuda")
    s8 = torch.full((d // 128, rows8, 4), 127, dtype=torch.uint8, device="cuda")
    _lib.check(lib.keds_attention_mx(_lib.ptr(qkv), _lib.ptr(out), B, S, Hm, int(causal), S, _lib.ptr(q8), _lib.ptr(s8), rows8,
                                     _lib.stream()), "keds_attention_mx")
    rec = _recorded_is_planned(lib, B, S, Hm, causal, S, q8=1)
    assert rec[3] & F_Q8 and rec[0] == (S257 if S == 257 else GENERIC), rec
    if S == 257:                        # hook 32 with MXFP8 rows: no tail kernel for them, the generic kernel with 16 unmasked tiles
        out32, q32, s32 = torch.full_like(out, SENTINEL), torch.zeros_like(q8), torch.full_like(s8, 127)
        try:
            lib.keds_attention_debug(32)
            _lib.check(lib.keds_attention_mx(_lib.ptr(qkv), _lib.ptr(out32), B, S, Hm, int(causal), S, _lib.ptr(q32), _lib.ptr(s32), rows8,
                                             _lib.stream()), "keds_attention_mx (hook 32)")
            rec32 = _recorded_is_planned(lib, B, S, Hm, causal, S, q8=1)
        finally:
            lib.keds_attention_debug(0)
        assert rec32[:4] == [GENERIC, 18, 16, F_Q8], rec32
        assert _untouched(out32[:rows8]) and _untouched(out32[B * S:])
        assert rel_l2(_dequantize(q32, s32), ref[:rows8].float()) <= 4e-2
    assert torch.equal(out[rows8:B * S], ref[rows8:])
    assert _untouched(out[:rows8]) and _untouched(out[B * S:])
    got = _dequantize(q8, s8)
    r = rel_l2(got, ref[:rows8].float())
    report(f"attention_edges.mx.S{S}.rows{rows8}", rel_l2=r)
    assert r <= 4e-2
    qt, _ = _torch_mx(got)
    assert torch.equal(qt, q8)
