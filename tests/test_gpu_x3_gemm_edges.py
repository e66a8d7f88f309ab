"""The split-operand GEMM (keds_gemm_x3, epilogues 13 - 15) per ELEMENT on every kernel form of gemm.hip, at its tile, K and
segment-seam edges, and the two split kernels bit for bit (tests/gemm_check.py: X3Case, the float64 reference, the bound;
tests/test_host_gemm_check.py: proof that the bound catches a dropped or stale lo K-tile in one 8-row piece, a wrong plane or K offset
at a seam, a fourth lo.lo segment, a misplaced 2^-e, a zero lo output plane, one lost store).

Every launch goes through keds_gemm_x3 and asserts what keds_gemm_last_launch recorded.  Operand planes sit in NaN-filled buffers: 256
guard rows behind M, a gap of 256 elements between (and behind) the hi and lo planes, NaN behind column K where lda > K -- a read
outside the operands poisons the output.  Outputs and output planes sit in sentinel-filled buffers with 256 guard rows, guard columns
where ldc > N and the same gap between the planes; everything outside [M, N] must survive (epilogue 14: rows >= M untouched).
One float64 reference per (shape, regime), computed on the GPU, serves the three epilogues and every form.  Every element of every
launch is compared; the worst ratio per (form, epilogue, regime) goes to the metrics log."""
import ctypes
import functools
import math

import pytest
import torch

from keds_amd import _lib
from tests import gemm_check as gc
from tests.gpu_util import report

pytestmark = pytest.mark.gpu

GUARD, GAP = 256, 256
SENT = gc.SENTINEL
SMALL, PAIR, QUAD = _lib.GEMM_FORM_SMALL, _lib.GEMM_FORM_PAIR, _lib.GEMM_FORM_QUAD
F_SMALL, F_PAIR = 1, 3 << 11                  # keds_gemm_force_small: bit 0, bits 11-12 = 3
CODES = tuple(gc.X3_EPILOGUES)
IDS = [gc.X3_NAMES[c] for c in CODES]


def _threshold():
    """tiles beyond which the 4-wave kernel goes persistent: min(CUs, 256) & ~7"""
    return min(torch.cuda.get_device_properties(0).multi_processor_count, 256) & ~7


def _lib_splitter(a, w):
    """the planes of a true split, made by the library's own kernels (each held to gemm_check.split_ref bit for bit below)"""
    lib = _lib.load()
    M, K = a.shape
    N = w.shape[0]
    a2 = torch.zeros((2, M, K), dtype=torch.float16, device="cuda")
    w2 = torch.zeros((2, N, K), dtype=torch.float16, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    e = ctypes.c_int32(0)
    _lib.check(lib.keds_split_f16_pair(_lib.ptr(a), K, M, K, _lib.ptr(a2), M * K, _lib.ptr(flag), _lib.stream()), "keds_split_f16_pair")
    _lib.check(lib.keds_split_f16_weight(_lib.ptr(w), N, K, _lib.ptr(w2), N * K, ctypes.byref(e), _lib.stream()), "keds_split_f16_weight")
    assert int(flag.item()) == 0
    return (a2[0], a2[1]), (w2[0], w2[1]), int(e.value)


def _make(M, N, K, regime, w_exp, p, std, rowscale):
    return gc.X3Case(M, N, K, regime, w_exp=w_exp, p=p, std=std, rowscale=rowscale, seed=1, device="cuda", splitter=_lib_splitter)


@functools.lru_cache(maxsize=4096)
def _case(M, N, K, regime, w_exp=0, p=None, std=1.0, rowscale=False):
    """one reference per (shape, regime), shared by every epilogue and form, never written to"""
    return _make(M, N, K, regime, w_exp, p, std, rowscale)


@functools.lru_cache(maxsize=1)
def _big_case(M, N, K, regime, w_exp=0, p=None, std=1.0, rowscale=False):
    return _make(M, N, K, regime, w_exp, p, std, rowscale)


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    try:
        yield
    finally:
        _lib.load().keds_gemm_force_small(0)
        _case.cache_clear()
        _big_case.cache_clear()


def _planes(hi, lo, rows, ld):
    """two [rows, ld] planes in ONE NaN-filled buffer -> (buffer, elements between the planes): guard rows behind hi.shape[0], NaN
    behind column hi.shape[1], a NaN gap behind each plane"""
    r, c = hi.shape
    stride = rows * ld + GAP
    buf = torch.full((2 * stride,), float("nan"), dtype=torch.float16, device="cuda")
    for i, t in enumerate((hi, lo)):
        buf[i * stride:i * stride + rows * ld].view(rows, ld)[:r, :c] = t
    return buf, stride


def _operands(case, lda):
    """the case's operand buffers, built once per row stride (no kernel writes them)"""
    cache = case.__dict__.setdefault("_operands", {})
    if lda not in cache:
        cache[lda] = _planes(case.ah, case.al, case.M + GUARD, lda) + _planes(case.wh, case.wl, case.N, case.K)
    return cache[lda]


def _is_sent(t):
    return bool((t == SENT).all())


def _launch(case, code, force=0, lda=None, ldc=None):
    """-> (res for gemm_check.model_failures, info of keds_gemm_last_launch, list of guard violations)"""
    lib = _lib.load()
    M, N, K = case.M, case.N, case.K
    lda, ldc = lda or K, ldc or N
    P = _lib.ptr
    a, a_plane, w, w_plane = _operands(case, lda)
    rows = M + GUARD
    pair = code == 15
    o_plane = rows * ldc + GAP
    out = torch.full((2 * o_plane,), SENT, dtype=torch.float16, device="cuda") if pair else torch.full((rows, ldc), SENT, dtype=torch.float32, device="cuda")
    if code == 14:
        out[:M, :N] = case.resid
    lib.keds_gemm_force_small(force)
    try:
        rc = lib.keds_gemm_x3(P(a), a_plane, lda, P(w), w_plane, P(case.bias), P(out), ldc, M, N, K, code, o_plane if pair else 0, case.w_exp, _lib.stream())
        info = (ctypes.c_int * 8)()
        _lib.check(lib.keds_gemm_last_launch(info), "keds_gemm_last_launch")
    finally:
        lib.keds_gemm_force_small(0)
    try:
        _lib.check(rc, f"keds_gemm_x3({gc.X3_NAMES[code]})")
        torch.cuda.synchronize()
    except RuntimeError as e:             # a failed launch or a device fault: nothing more of this session may run on the card
        pytest.exit(f"{case.name} {gc.X3_NAMES[code]} force={force:#x}: {e}", returncode=3)
    bad = []
    if pair:
        views = [out[i * o_plane:i * o_plane + rows * ldc].view(rows, ldc) for i in (0, 1)]
        res = {"hi": views[0][:M, :N].clone(), "lo": views[1][:M, :N].clone()}
        for v in views:
            v[:M, :N] = SENT
        if not _is_sent(out):
            bad.append("an output plane written outside [M, N]: guard rows, guard columns or the gap behind a plane")
    else:
        res = {"out": out[:, :N]}
        if not _is_sent(out[M:]):
            bad.append("output rows >= M written")
        if ldc > N and not _is_sent(out[:, N:]):
            bad.append("guard columns n >= N written")
    return res, tuple(info), bad


class Tally:
    """failures of a whole test, and the worst ratio per (form label, epilogue, regime)"""

    def __init__(self, label):
        self.label, self.msgs, self.worst, self.launches = label, [], {}, 0

    def run(self, case, code, want, tag="", **kw):
        """launch, assert the recorded form (`want`: the given ones of main, tail, ring, tail_ring, splits, tail_splits, persistent,
        flags), check every output element"""
        res, info, bad = _launch(case, code, **kw)
        self.launches += 1
        name = f"{self.label}{tag}.{case.name}.{gc.X3_NAMES[code]}"
        got = dict(main=info[0], tail=info[1], ring=info[2], tail_ring=info[3], splits=info[4], tail_splits=info[5], persistent=info[6], flags=info[7])
        wrong = {k: (got[k], v) for k, v in want.items() if got[k] != v}
        if wrong:
            self.msgs.append(f"{name}: recorded kernel form differs (got, wanted): {wrong}")
        self.msgs += [f"{name}: {b}" for b in bad]
        fails, worst = gc.model_failures(case, code, res)
        self.msgs += [str(f) for f in fails]
        key = (gc.X3_NAMES[code], case.regime + (".rowscale" if ".rowscale" in case.name else ""))
        self.worst[key] = max(self.worst.get(key, 0.0), worst)

    def finish(self):
        for (epi, regime), w in sorted(self.worst.items()):
            report(f"x3_edges.{self.label}.{epi}.{regime}", worst_ratio=w)
        assert self.launches > 0
        assert not self.msgs, f"{len(self.msgs)} failures:\n" + "\n".join(self.msgs[:30])


def _spikes(K):
    n = K // gc.TILE_K
    return sorted({0, n - 1, n, 2 * n - 1, 2 * n, 3 * n - 1})          # the first and last K-tile and both sides of both seams


def _all_regimes(K):
    """arguments of _case behind (M, N, K): integer at three exponents, random, every spike"""
    return ([("integer", e) for e in (0, 5, -3)] + [("random", 7)] + [("spike", 0, p) for p in _spikes(K)])


def _big_regimes(K, persistent=False, split=False):
    n = K // gc.TILE_K
    regs = [("integer", 5), ("spike", 0, n), ("spike", 0, 2 * n)]
    if persistent:
        regs.append(("random", 7, None, 1.0, True))                      # rows x 2^6 on every other 256-row tile
    if split:
        regs.append(("split", 0, None, 1e-2))
    return regs


# ---- 128 x 128 kernel ------------------------------------------------------------------------------------------------------------
SMALL_M = (1, 7, 127, 128, 129, 255, 256, 257)
SMALL_K = (64, 128, 192, 320)                      # 3, 6, 9 and 15 K-tiles against a ring of four
SMALL_WANT = dict(main=SMALL, tail=0, ring=4, splits=1, persistent=0, flags=0)


@pytest.mark.parametrize("code", CODES, ids=IDS)
def test_small_kernel_four_stage_ring(code):
    """M over every row-tile edge, N = 128 and 384, one to five K-tiles per segment; every regime and every spike at every shape,
    true splits of weights at three magnitudes at 257 x 384 x 320"""
    t = Tally("small4")
    for N in (128, 384):
        for M in SMALL_M:
            for K in SMALL_K:
                for args in _all_regimes(K):
                    t.run(_case(M, N, K, *args), code, SMALL_WANT)
    for std in (1.0, 1e-2, 3e-5):
        t.run(_case(257, 384, 320, "split", 0, None, std), code, SMALL_WANT)
    t.finish()


@pytest.mark.parametrize("code", CODES, ids=IDS)
def test_small_kernel_strided_rows(code):
    """lda = K + 72 (NaN behind column K) and ldc = N + 40 (guard columns, for the output planes too)"""
    t = Tally("small4.strided")
    for M, N, K in [(1, 128, 64), (129, 384, 192), (257, 128, 320), (255, 384, 128)]:
        for args in _all_regimes(K):
            t.run(_case(M, N, K, *args), code, SMALL_WANT, lda=K + 72, ldc=N + 40)
    t.run(_case(257, 384, 320, "split", 0, None, 1e-2), code, SMALL_WANT, lda=320 + 72, ldc=384 + 40)
    t.finish()


def test_small_kernel_two_stage_ring():
    """more than 256 tiles on the 128 x 128 path (bit 0 at 2170 x 2048: 272 tiles, a ragged last row tile)"""
    t = Tally("small2")
    for K in (64, 128):
        for args in _all_regimes(K):
            case = _big_case(2170, 2048, K, *args)
            for code in CODES:
                t.run(case, code, dict(main=SMALL, tail=0, ring=2, splits=1, persistent=0), force=F_SMALL)
    t.finish()


def test_long_k_never_splits():
    """129 x 1024 x 2048: 16 tiles and K >= 2048 split K for every other epilogue; gemm_may_split excludes the split-operand ones
    (96 K-tiles through the ring of four)"""
    t = Tally("nosplit")
    _lib.ensure_gemm_workspace("cuda")
    for args in _all_regimes(2048):
        case = _big_case(129, 1024, 2048, *args)
        for code in CODES:
            t.run(case, code, SMALL_WANT)
    t.finish()


# ---- 256 x 256 kernels -----------------------------------------------------------------------------------------------------------
BIG_M, BIG_N = 2048, 4096                      # 128 tiles
BIG_K = (128, 192, 1024)                       # 2, 3 and 16 K-tiles per segment


def test_eight_wave_and_four_wave_kernel_one_tile_per_workgroup():
    """2048 x 4096: the 4-wave kernel by shape (128 tiles <= T: one tile per workgroup), the 8-wave kernel with bits 11-12 = 3; the
    same reference serves both"""
    assert BIG_M // 256 * (BIG_N // 256) <= _threshold()
    t8, t4 = Tally("pair8"), Tally("quad4")
    for K in BIG_K:
        for args in _big_regimes(K, split=K == 1024):
            case = _big_case(BIG_M, BIG_N, K, *args)
            for code in CODES:
                t8.run(case, code, dict(main=PAIR, tail=0, ring=2, splits=1, persistent=0, flags=0), force=F_PAIR)
                t4.run(case, code, dict(main=QUAD, tail=0, ring=2, splits=1, persistent=0, flags=0))
    t8.msgs += t4.msgs
    t8.launches += t4.launches
    for (epi, regime), w in sorted(t4.worst.items()):
        report(f"x3_edges.quad4.{epi}.{regime}", worst_ratio=w)
    t8.finish()


def _persistent_shapes():
    """threshold + 1 tiles in one tile column (one workgroup walks two tiles), 1.5 T tiles (supertiles, a ragged second round),
    2 T + 8 tiles in one tile column"""
    th = _threshold()
    return [("plus1", (th + 1) * 256, 256), ("ragged", 3 * th // 8 * 256, 1024), ("two_rounds_plus8", (2 * th + 8) * 256, 256)]


@pytest.mark.parametrize("which", range(3), ids=["plus1", "ragged", "two_rounds_plus8"])
def test_four_wave_persistent_kernel(which):
    """More tiles than T: epilogues 13 and 15 walk their tiles in one workgroup per CU -- the next tile's first K-tiles are requested
    behind this tile's LAST segment -- and epilogue 14 must record one tile per workgroup.  K-tiles per segment 2, 3, 9, 16; rows
    x 2^6 on every other 256-row tile make a prefetched K-tile of the wrong tile gross; true splits at 1.5 T tiles."""
    label, M, N = _persistent_shapes()[which]
    assert (M // 256) * (N // 256) > _threshold(), "not a persistent launch on this device"
    t = Tally(f"quad4.persistent.{label}")
    for K in (128, 192, 576, 1024):
        for args in _big_regimes(K, persistent=True, split=which == 1 and K == 1024):
            case = _big_case(M, N, K, *args)
            for code in CODES:
                t.run(case, code, dict(main=QUAD, tail=0, ring=2, splits=1, persistent=int(code != 14), flags=0))
    t.finish()


@pytest.mark.parametrize("r", (1, 127, 129, 255))
def test_remainder_rows_behind_big_tiles(r):
    """(3584 + r) x 4096: 224 tiles of 256 x 256 on the 4-wave kernel and a 128 x 128 remainder launch of one or two row tiles, whose
    operand and output planes start 3584 rows in"""
    M, N = 3584 + r, 4096
    t = Tally(f"remainder.r{r}")
    pers = int(224 > _threshold())
    for K in (256, 1024):
        for args in _big_regimes(K):
            case = _big_case(M, N, K, *args)
            for code in CODES:
                t.run(case, code, dict(main=QUAD, tail=SMALL, ring=2, tail_ring=4, splits=1, tail_splits=1, persistent=pers if code != 14 else 0))
    t.finish()


# ---- the split kernels, bit for bit ----------------------------------------------------------------------------------------------
def _bits_equal(got, want):
    """fp16 tensors equal to the bit (any NaN equals any NaN)"""
    return bool(((got.view(torch.int16) == want.view(torch.int16)) | (torch.isnan(got) & torch.isnan(want))).all())


def _specials():
    """values in the SCALED domain (what the planes hold): lo an fp16 subnormal, exact fp16 values (lo = +-0), ties of hi and of a
    subnormal lo, the edge of the fp16 range (65504 - 2^-8 rounds to 65504 and is no overflow)"""
    return torch.tensor([0.1, -0.01, 1e-3, 1.0 + 2.0 ** -20, 2.0 ** -14 + 2.0 ** -26, 2.0 ** -3 + 2.0 ** -25, -(2.0 ** -3 + 3 * 2.0 ** -25), 6e-8, 2.0 ** -24,
                         1.0, -2.5, 1024.0, 2.0 ** -14, 0.0, -0.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(2048.0 + 1.0), 2048.0 + 3.0, 4096.0 + 2.0 ** -11,
                         65503.99609375, -65503.99609375, 65472.0, 30000.0 + 2.0 ** -8], dtype=torch.float32, device="cuda")


def _split_data(rows, cols, seed, top=60000.0):
    """random magnitudes over 24 binades (|x| <= top, zero or >= 2^-60) with the special values that fit below `top` scattered in"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(rows * cols, generator=g, device="cuda") * torch.exp2(torch.randint(-12, 12, (rows * cols,), generator=g, device="cuda").float())
    x = torch.where(x.abs() > top, x * float(top) * 2.0 ** -17, x)
    x = torch.where(x.abs() < 2.0 ** -60, torch.zeros_like(x), x)
    sp = _specials()
    sp = sp[sp.abs() <= top]
    idx = torch.randperm(rows * cols, generator=g, device="cuda")[:len(sp)]
    x[idx] = sp[:len(idx)]
    return x.view(rows, cols)


def _run_pair(x, rows, cols, ld):
    """keds_split_f16_pair on x [rows, cols] laid out with row stride ld -> (hi, lo, flag, untouched): planes rows cols + 256 apart in
    a sentinel-filled buffer; the source rows are padded with NaN behind column cols"""
    lib = _lib.load()
    src = torch.full((rows, ld), float("nan"), dtype=torch.float32, device="cuda")
    src[:, :cols] = x
    plane = rows * cols + GAP
    out = torch.full((2 * plane,), SENT, dtype=torch.float16, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = lib.keds_split_f16_pair(_lib.ptr(src), ld, rows, cols, _lib.ptr(out), plane, _lib.ptr(flag), _lib.stream())
    try:
        _lib.check(rc, "keds_split_f16_pair")
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"keds_split_f16_pair {rows} x {cols}: {e}", returncode=3)
    hi, lo = (out[i * plane:i * plane + rows * cols].view(rows, cols) for i in (0, 1))
    untouched = _is_sent(out[rows * cols:plane]) and _is_sent(out[plane + rows * cols:])
    return hi, lo, int(flag.item()), untouched


SPLIT_SHAPES = [(r, c) for r in (1, 7, 300) for c in (8, 72, 1024)]


@pytest.mark.parametrize("rows,cols", SPLIT_SHAPES)
def test_split_f16_pair_bit_for_bit(rows, cols):
    """hi = fp16(x), lo = fp16(x - hi) to the bit, fp16 subnormals kept (the absolute 2^-25 the kernel's comment promises); source
    row stride cols + 4; the gap and tail of the planes untouched; the overflow flag stays down just under 65504 and goes up at
    65504, 7e4, inf and NaN"""
    x = _split_data(rows, cols, rows * 131 + cols)
    hi, lo, flag, untouched = _run_pair(x, rows, cols, cols + 4)
    want_hi, want_lo = gc.split_ref(x)
    assert untouched and flag == 0
    assert _bits_equal(hi, want_hi) and _bits_equal(lo, want_lo)
    s = x.double()
    assert bool(((hi.double() + lo.double() - s).abs() <= 2.0 ** -22 * s.abs() + 2.0 ** -25).all())
    for i, big in enumerate((65504.0, -7e4, float("inf"), float("nan"))):
        y = x.clone()
        y.view(-1)[(i * 37 + rows * cols // 2) % (rows * cols)] = big
        hi, lo, flag, untouched = _run_pair(y, rows, cols, cols + 4)
        want_hi, want_lo = gc.split_ref(y)
        assert untouched and flag == 1, big
        assert _bits_equal(hi, want_hi) and _bits_equal(lo, want_lo), big


@pytest.mark.parametrize("rows,cols", SPLIT_SHAPES)
def test_split_f16_weight_bit_for_bit(rows, cols):
    """max |W| from 2^-30 to 2^20 (and 2^115): the exponent puts max |W| 2^e in [2^13, 2^14) unless it is clamped to 40 or -100, the
    planes are the torch evaluation of the split of W 2^e to the bit, the gap and tail behind the planes stay untouched; an
    all-zero matrix gives exponent 0 and zero planes.  (|w 2^e| of the non-zero values stays far above 2^-100: no fp32 subnormal.)"""
    lib = _lib.load()
    plane = rows * cols + GAP
    for lg, frac in [(-30, 1.0), (-27, 1.3), (-26, 1.99), (-15, 1.5), (-7, 1.1), (0, 1.0), (0, 1.9999999), (13, 1.0), (20, 1.7), (115, 1.5), (None, 0.0)]:
        if lg is None:
            w, want_e = torch.zeros(rows, cols, device="cuda"), 0
        else:
            want_e = max(-100, min(40, 13 - lg))
            top = float(torch.tensor(frac * 2.0 ** (lg + want_e), dtype=torch.float32))   # max |W| 2^e: in [2^13, 2^14) unless clamped
            s = _split_data(rows, cols, rows * 17 + cols + lg + 50, top=top)       # the planes' domain
            s.view(-1)[(rows * cols) // 3] = -top
            w = s * 2.0 ** -want_e                                                 # exact: a power of two, no fp32 under- or overflow
            assert float(w.abs().max()) == top * 2.0 ** -want_e and math.frexp(float(w.abs().max()))[1] - 1 == lg
        out = torch.full((2 * plane,), SENT, dtype=torch.float16, device="cuda")
        e = ctypes.c_int32(-999)
        rc = lib.keds_split_f16_weight(_lib.ptr(w), rows, cols, _lib.ptr(out), plane, ctypes.byref(e), _lib.stream())
        try:
            _lib.check(rc, "keds_split_f16_weight")
            torch.cuda.synchronize()
        except RuntimeError as err:
            pytest.exit(f"keds_split_f16_weight {rows} x {cols} max 2^{lg}: {err}", returncode=3)
        assert int(e.value) == want_e == gc.weight_exp_ref(w), (lg, frac, e.value)
        if lg is not None and -27 <= lg <= 20:
            assert 2.0 ** 13 <= float(w.abs().max()) * 2.0 ** want_e < 2.0 ** 14
        hi, lo = (out[i * plane:i * plane + rows * cols].view(rows, cols) for i in (0, 1))
        want_hi, want_lo = gc.split_ref(w, want_e)
        assert _is_sent(out[rows * cols:plane]) and _is_sent(out[plane + rows * cols:]), lg
        assert _bits_equal(hi, want_hi) and _bits_equal(lo, want_lo), (lg, frac)
        sc = w.double() * 2.0 ** want_e
        assert bool(((hi.double() + lo.double() - sc).abs() <= 2.0 ** -22 * sc.abs() + 2.0 ** -25).all()), lg
