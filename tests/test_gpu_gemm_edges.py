"""Every GEMM kernel form per ELEMENT, at its tile and K edges (tests/gemm_check.py: the cases, the float64 reference and the bound;
tests/test_host_gemm_check.py: proof that the bound catches one stale K-tile in one 8-row piece, one lost store, one shifted slice).

All calls go through keds_gemm_bt_ex2 (keds_gemm_bt_ex where the test is about it); every case asserts the kernel form that
keds_gemm_last_launch recorded, so a shape the dispatcher sends elsewhere fails instead of testing the wrong kernel.  Outputs and
side buffers are filled with a sentinel and carry guard rows (and guard columns where ldc > N) that must survive.  One reference
per (shape, regime, operand type) is shared by all epilogues and forms.  Each test loops its shapes and collects every failure
before it asserts; the worst bound ratio per (form, epilogue, regime) goes to the metrics log."""
import ctypes
import functools

import pytest
import torch

from keds_amd import _lib
from tests import gemm_check as gc
from tests.gpu_util import report

pytestmark = pytest.mark.gpu

GUARD = 256                                   # rows behind M that no launch may touch (the library wants 128 addressable)
SENT = gc.SENTINEL
STAT_BASE = (3 << 28, 11 << 28)               # what the statistics a launch ADDS INTO hold before it
STAT_GUARD = 7
SMALL, PAIR, QUAD, QUAD3 = _lib.GEMM_FORM_SMALL, _lib.GEMM_FORM_PAIR, _lib.GEMM_FORM_QUAD, _lib.GEMM_FORM_QUAD3
DEFER, PROLOGUE = _lib.GEMM_FLAG_DEFER, _lib.GEMM_FLAG_RESID_PROLOGUE
F_SMALL, F_NOSPLIT, F_PROLOGUE, F_QUAD, F_PERSIST, F_PAIR, F_NOQUAD3, F_NODEFER = 1, 1 << 9, 1 << 10, 1 << 11, 2 << 11, 3 << 11, 1 << 16, 1 << 17
WS_BYTES = 32 << 20
ALL_CODES = tuple(gc.EPILOGUES)
BIG_CODES = tuple(c for c in ALL_CODES if c != 12)      # BIAS_BF16_HEADF32 never takes 256^2 tiles (its head rows count from row 0)
LN_CODES = (6, 7, 10, 11, 16, 17)
ROW_SIDE_CODES = (6, 7, 10, 16, 17, 8, 9, 18, 5, 21)    # side buffers that move with the rows of a remainder launch


def _regimes(code):
    fam = gc.EPILOGUES[code][2]
    return gc.REGIMES if fam in ("ln", "ln_qgelu") else gc.REGIMES[:4]


@pytest.fixture(scope="module", autouse=True)
def _workspace_and_guard():
    """a 32 MiB split-K workspace (what keds_hip.h names as enough for every shape) and a registered numerics-guard flag for the
    module; the process-wide workspace of keds_amd._lib comes back afterwards"""
    lib = _lib.load()
    ws = torch.empty(WS_BYTES, dtype=torch.uint8, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(lib.keds_gemm_set_workspace(ws.data_ptr(), ws.numel()), "keds_gemm_set_workspace")
    _lib.check(lib.keds_numerics_guard_set(flag.data_ptr()), "keds_numerics_guard_set")
    _STATE["flag"] = flag
    try:
        yield
    finally:
        lib.keds_gemm_force_small(0)
        lib.keds_numerics_guard_set(None)
        old = _lib._gemm_ws.get(torch.cuda.current_device())
        lib.keds_gemm_set_workspace(old.data_ptr() if old is not None else None, old.numel() if old is not None else 0)
        _STATE.clear()
        _case.cache_clear()
        _big_case.cache_clear()


_STATE = {}


@functools.lru_cache(maxsize=1024)
def _case(M, N, K, regime, dtype):
    """one reference per (shape, regime, operand type), shared by every epilogue and form, never written to"""
    return gc.Case(M, N, K, regime, dtype, seed=1, device="cuda")


@functools.lru_cache(maxsize=2)
def _big_case(M, N, K, regime, dtype):
    return gc.Case(M, N, K, regime, dtype, seed=1, device="cuda")


def _threshold():
    """tiles beyond which the 4-wave kernel goes persistent: min(CUs, 256) & ~7"""
    return min(torch.cuda.get_device_properties(0).multi_processor_count, 256) & ~7


def _expected_splits(M, N, K):
    """launch_small's rule (gemm.hip)"""
    mt = (M + 127) // 128
    tiles = mt * (N // 128)
    if tiles > 64 or K < 2048:
        return 1
    s = 1
    while s < 16 and tiles * s * 2 <= 256 and K % (s * 2 * 64) == 0 and K // (s * 2) >= 128:
        s *= 2
    return s if s > 1 and s * mt * 128 * N * 4 <= WS_BYTES else 1


def _sent(t, value=SENT):
    return bool((t == torch.tensor(value, dtype=t.dtype, device=t.device)).all())       # (bf16 holds the sentinel rounded)


def _launch(case, code, force=0, lda=None, ldc=None, via_ex=False):
    """-> (res for gemm_check.model_failures, info of keds_gemm_last_launch, list of guard violations)"""
    lib = _lib.load()
    M, N, K = case.M, case.N, case.K
    op, od, fam = gc.EPILOGUES[code]
    lda, ldc = lda or K, ldc or N
    P = _lib.ptr
    A = torch.full((M + GUARD, lda), float("nan"), dtype=op, device="cuda")          # a read behind row M or column K poisons the output
    A[:M, :K] = case.A
    orows = (case.patch_out_rows() if fam == "patch" else M) + GUARD
    out = torch.full((orows, ldc), SENT, dtype=od, device="cuda")
    if fam in ("resid", "resid_stats"):
        out[:M, :N] = case.resid.to(od)
    bias, aux, aux_i, aux2 = case.bias, None, 0, None
    stats_in = other = stats = copy = head = None
    if fam in ("ln", "ln_qgelu"):
        bias = torch.cat([case.bias, case.csum])
        stats_in = torch.full((M + GUARD, 2), STAT_GUARD, dtype=torch.int64, device="cuda")
        stats_in[:M] = case.stats
        other = torch.full((M + GUARD, 2), STAT_GUARD, dtype=torch.int64, device="cuda")
        keep = stats_in.clone()
        aux, aux2 = stats_in, other
    elif fam == "resid_stats":
        stats = torch.tensor(STAT_BASE, dtype=torch.int64, device="cuda").repeat(M + GUARD, 1)
        aux = stats
        if code == 8:
            copy = torch.full((M + GUARD, N), SENT, dtype=torch.bfloat16, device="cuda")
            aux2 = copy
    elif fam == "patch":
        aux, aux_i = case.pos, gc.PATCH_G
    elif fam == "headf32":
        aux_i = min(M, 130)                                                        # head rows: across a 128-row tile edge
        head = torch.full((aux_i + GUARD, 3, N), SENT, dtype=torch.float32, device="cuda")
        aux = head
    lib.keds_gemm_force_small(force)
    try:
        if via_ex:
            rc = lib.keds_gemm_bt_ex(P(A), lda, P(case.W), P(bias), P(out), ldc, M, N, K, code, P(aux), aux_i, _lib.stream())
        else:
            rc = lib.keds_gemm_bt_ex2(P(A), lda, P(case.W), P(bias), P(out), ldc, M, N, K, code, P(aux), aux_i, P(aux2), _lib.stream())
        info = (ctypes.c_int * 8)()
        _lib.check(lib.keds_gemm_last_launch(info), "keds_gemm_last_launch")
    finally:
        lib.keds_gemm_force_small(0)
    try:
        _lib.check(rc, f"keds_gemm_bt_ex2({gc.NAMES[code]})")
        torch.cuda.synchronize()
    except RuntimeError as e:             # a failed launch or a device fault: nothing more of this session may run on the card
        pytest.exit(f"{case.name} {gc.NAMES[code]} force={force:#x}: {e}", returncode=3)
    bad = []
    res = {"out": out[:, :N]}
    if fam == "patch":
        written = torch.zeros(orows, dtype=torch.bool, device="cuda")
        written[case.patch_rows()] = True
        if not _sent(out[~written]):
            bad.append("a class-token row or a guard row of the PATCH output was written")
    else:
        if not _sent(out[M:]):
            bad.append("output rows >= M written")
    if ldc > N and not _sent(out[:, N:]):
        bad.append("guard columns n >= N written")
    if other is not None:
        if not (_sent(other[:M], 0) and _sent(other[M:], STAT_GUARD)):
            bad.append("the statistics buffer to clear: not exactly rows < M cleared")
        if not torch.equal(stats_in, keep):
            bad.append("the statistics a LayerNorm epilogue reads were written")
    if stats is not None:
        base = torch.tensor(STAT_BASE, dtype=torch.int64, device="cuda")
        if not bool((stats[M:] == base).all()):
            bad.append("statistics of rows >= M added to")
        res["stats"] = stats[:M] - base
    if copy is not None:
        if not _sent(copy[M:]):
            bad.append("bf16 copy rows >= M written")
        res["copy"] = copy
    if head is not None:
        if not (_sent(head[:, 1:]) and _sent(head[aux_i:])):
            bad.append("fp32 head: a slot other than [m < aux_i][0] written")
        res["head"] = head[:aux_i, 0]
    if int(_STATE["flag"].item()) != 0:
        bad.append("numerics guard raised")
        _STATE["flag"].zero_()
    return res, tuple(info), bad


class Tally:
    """failures of a whole test, and the worst ratio per (form label, epilogue, regime)"""

    def __init__(self, label):
        self.label, self.msgs, self.worst, self.launches, self.inexact_stats = label, [], {}, 0, set()

    def run(self, case, code, want, tag="", twice=False, **kw):
        """launch, assert the recorded form (`want`: dict of main, tail, ring, tail_ring, splits, tail_splits, persistent, flags --
        the given ones), check every output"""
        res, info, bad = _launch(case, code, **kw)
        self.launches += 1
        name = f"{self.label}{tag}.{case.name}.{gc.NAMES[code]}"
        got = dict(main=info[0], tail=info[1], ring=info[2], tail_ring=info[3], splits=info[4], tail_splits=info[5], persistent=info[6],
                   flags=info[7])
        wrong = {k: (got[k], v) for k, v in want.items() if got[k] != v}
        if wrong:
            self.msgs.append(f"{name}: recorded kernel form differs (got, wanted): {wrong}")
        self.msgs += [f"{name}: {b}" for b in bad]
        fails, worst = gc.model_failures(case, code, res)
        self.msgs += [str(f) for f in fails]
        if "stats" in res and case.exact and not gc.stats_exact(gc.expected(case, code).ref):
            self.inexact_stats.add(case.name)
        key = (gc.NAMES[code], case.regime)
        self.worst[key] = max(self.worst.get(key, 0.0), worst)
        if twice:                                                           # integer atomics: the same bits on a second run
            res2, _, _ = _launch(case, code, **kw)
            for k in res:
                if not torch.equal(res[k], res2[k]):
                    self.msgs.append(f"{name}: `{k}` differs between two runs")
        return res

    def finish(self):
        for (epi, regime), w in sorted(self.worst.items()):
            report(f"gemm_edges.{self.label}.{epi}.{regime}", worst_ratio=w)
        if self.inexact_stats:                                             # sum of squares by the bound only (gemm_check: stats_exact)
            report(f"gemm_edges.{self.label}.inexact_integer_statistics", cases=sorted(self.inexact_stats))
        assert self.launches > 0
        assert not self.msgs, f"{len(self.msgs)} failures:\n" + "\n".join(self.msgs[:30])


def _dt(code):
    return gc.EPILOGUES[code][0]


def _is_stats(code):
    return gc.EPILOGUES[code][2] == "resid_stats"


# ---- 128 x 128 kernel ------------------------------------------------------------------------------------------------------------
SMALL_M = (1, 7, 127, 128, 129, 255, 256, 257)
SMALL_K = (64, 128, 192, 256, 320)                    # one to five K-tiles against a ring of four


@pytest.mark.parametrize("code", ALL_CODES, ids=[gc.NAMES[c] for c in ALL_CODES])
def test_small_kernel_four_stage_ring(code):
    """<= 256 tiles, no split: M over every row-tile edge, N = 128 and 384 (one and three column tiles: never the 256-wide path),
    one to five K-tiles, every regime at every shape."""
    t = Tally("small4")
    for N in (128, 384):
        for M in SMALL_M:
            for K in SMALL_K:
                for regime in _regimes(code):
                    t.run(_case(M, N, K, regime, _dt(code)), code, dict(main=SMALL, tail=0, ring=4, splits=1, persistent=0),
                          twice=_is_stats(code) and M in (129, 257))
    t.finish()


@pytest.mark.parametrize("code", ALL_CODES, ids=[gc.NAMES[c] for c in ALL_CODES])
def test_small_kernel_strided_rows(code):
    """keds_gemm_bt_ex with lda > K and ldc > N (the PATCH forms want a dense output: lda only): the guard columns survive, the
    NaN columns behind K are not read"""
    t = Tally("small4.strided")
    patch = gc.EPILOGUES[code][2] == "patch"
    needs_ex2 = gc.EPILOGUES[code][2] in ("ln", "ln_qgelu") or code == 8
    for M, N, K in [(1, 128, 64), (129, 384, 192), (257, 128, 320), (255, 384, 128)]:
        for regime in _regimes(code):
            t.run(_case(M, N, K, regime, _dt(code)), code, dict(main=SMALL, ring=4, splits=1), lda=K + 72,
                  ldc=None if patch else N + 40, via_ex=not needs_ex2)
    t.finish()


@pytest.mark.parametrize("code", ALL_CODES, ids=[gc.NAMES[c] for c in ALL_CODES])
def test_small_kernel_two_stage_ring(code):
    """more than 256 tiles on the 128 x 128 path (bit 0 at 2176 x 2048: 272 tiles, M = 2170: a ragged last row tile)"""
    t = Tally("small2")
    for K in (64, 128, 192):
        for regime in _regimes(code):
            t.run(_big_case(2170, 2048, K, regime, _dt(code)), code, dict(main=SMALL, tail=0, ring=2, splits=1), force=F_SMALL)
    t.finish()


# ---- split-K + reduce ------------------------------------------------------------------------------------------------------------
SPLIT_SHAPES = [(1, 1024, 2048, 16), (1, 1024, 2176, 2), (129, 1024, 2304, 4), (129, 1024, 4096, 16), (129, 1024, 2560, 8), (1024, 1024, 2048, 4), (1024, 1024, 2304, 4),
                (1025, 1024, 2048, 1), (129, 384, 2176, 2), (7, 128, 4096, 16)]


@pytest.mark.parametrize("code", ALL_CODES, ids=[gc.NAMES[c] for c in ALL_CODES])
def test_split_k_and_reduce(code):
    """<= 64 tiles and K >= 2048 with the workspace registered: 2, 4, 8 and 16 slices, every epilogue through the reduce kernel,
    the first (`head`) and the last (`tail`) slice carrying the output; 1025 rows are 72 tiles and must NOT split; bit 9 switches
    the split off."""
    t = Tally("splitk")
    regs = ("tail", "head", "integer") + (("offset",) if code in LN_CODES else ("random",))
    for M, N, K, splits in SPLIT_SHAPES:
        assert _expected_splits(M, N, K) == splits, (M, N, K)
        for regime in regs:
            t.run(_case(M, N, K, regime, _dt(code)), code, dict(main=SMALL, tail=0, ring=4, splits=splits), twice=_is_stats(code) and M == 129)
    t.run(_case(129, 1024, 2304, "tail", _dt(code)), code, dict(main=SMALL, ring=4, splits=1), tag=".nosplit", force=F_NOSPLIT)
    t.finish()


# ---- 256 x 256 kernels -----------------------------------------------------------------------------------------------------------
BIG_M, BIG_N = 2048, 4096                      # 128 tiles: the smallest launch that takes 256^2 tiles (M % 256 == 0, K <= 1024)


def _big_loop(t, codes, Ks, want, force, regs_of=_regimes, shape=(BIG_M, BIG_N), tag=""):
    """every K x every regime of the epilogue x both operand types; one reference at a time serves all its epilogues"""
    M, N = shape
    for K in Ks:
        for regime in gc.REGIMES:
            for dt in (gc.BF, gc.HF):
                for code in (c for c in codes if _dt(c) == dt and regime in regs_of(c)):
                    w = want(code, K) if callable(want) else want
                    f = force(code, K) if callable(force) else force
                    t.run(_big_case(M, N, K, regime, dt), code, w, force=f, tag=tag, twice=_is_stats(code) and regime == "tail")


def test_eight_wave_kernel():
    """the 8-wave 256 x 256 kernel (bits 11-12 = 3), every epilogue that takes big tiles, two to sixteen K-tiles"""
    t = Tally("pair8")
    _big_loop(t, BIG_CODES, (128, 192, 256, 1024), dict(main=PAIR, tail=0, ring=2, splits=1, persistent=0, flags=0), F_PAIR)
    t.finish()


def test_eight_wave_kernel_is_the_default_of_the_plain_epilogues():
    t = Tally("pair8.default")
    _big_loop(t, (0, 1, 2, 3, 4, 5, 8, 19, 20, 21, 22), (128, 1024), dict(main=PAIR, tail=0, ring=2, persistent=0), 0)
    t.finish()


def test_eight_wave_kernel_residual_prologue_variant():
    """bit 10: residual tile + bias as the accumulators' initial value -- another order of the fp32 additions, the same bound"""
    t = Tally("pair8.prologue")
    _big_loop(t, (9, 18), (128, 256, 1024), dict(main=PAIR, tail=0, ring=2, flags=PROLOGUE), F_PROLOGUE | F_PAIR)
    t.finish()


def test_four_wave_kernel_one_tile_per_workgroup():
    """bits 11-12 = 1 at 128 tiles, K-tiles 2, 3, 4, 7, 8"""
    t = Tally("quad4")
    _big_loop(t, BIG_CODES, (128, 192, 256, 448, 512), dict(main=QUAD, tail=0, ring=2, splits=1, persistent=0), F_QUAD)
    t.finish()


def test_four_wave_kernel_is_the_default_of_the_layernorm_epilogues():
    """K >= 512 and no more tiles than the persistent threshold: one tile per workgroup, by shape"""
    assert BIG_M // 256 * (BIG_N // 256) <= _threshold()
    t = Tally("quad4.default")
    _big_loop(t, LN_CODES, (512, 1024), dict(main=QUAD, tail=0, ring=2, persistent=0), 0)
    t.finish()


def _persistent_shapes():
    """(label, M, N): threshold + 1 tiles (one workgroup walks two tiles; a single tile column, no supertiles), a ragged second
    round (supertiles of 8 x 4), exactly two rounds, two rounds + 8 (65 row tiles: the row tile behind the supertiles)"""
    th = _threshold()
    return [("plus1", (th + 1) * 256, 256), ("ragged", (th + th // 2) // 4 * 256, 1024), ("two_rounds", 2 * th // 16 * 256, 4096),
            ("two_rounds_plus8", (2 * th + 8) // 8 * 256, 2048)]


PERSIST_K = (128, 192, 448, 512, 576, 1024)    # K-tiles 2, 3, 7 | 8, 9, 16: deferral off | just on, odd, long


@pytest.mark.parametrize("which", range(4), ids=["plus1", "ragged", "two_rounds", "two_rounds_plus8"])
def test_four_wave_persistent_kernel(which):
    """Both LayerNorm forms, their fp16-output forms and a plain epilogue forced onto the persistent kernel (bits 11-12 = 2), with the
    deferred stores (on from 8 K-tiles, LayerNorm-bias forms only) and with bit 17 (never deferred)."""
    label, M, N = _persistent_shapes()[which]
    tiles = (M // 256) * (N // 256)
    assert tiles > _threshold(), "not a persistent launch on this device"
    codes = LN_CODES + (0, 22)

    def want(defer_on):
        def w(code, K):
            d = DEFER if defer_on and code in (6, 10, 16) and K >= 512 else 0
            return dict(main=QUAD, tail=0, ring=2, splits=1, persistent=1, flags=d)
        return w
    t = Tally(f"quad4.persistent.{label}")
    _big_loop(t, codes, PERSIST_K, want(True), F_PERSIST, shape=(M, N))
    t2 = Tally(f"quad4.persistent.{label}.nodefer")
    _big_loop(t2, (6, 10, 16), (512, 576, 1024), want(False), F_PERSIST | F_NODEFER, shape=(M, N))
    t.msgs += t2.msgs
    t.worst.update({(e + ".nodefer", r): w for (e, r), w in t2.worst.items()})
    t.finish()


def test_four_wave_persistent_kernel_is_the_default_beyond_the_threshold():
    label, M, N = _persistent_shapes()[1]
    t = Tally("quad4.persistent.default")
    _big_loop(t, (6, 16, 17), (512, 1024), lambda code, K: dict(main=QUAD, persistent=1, flags=DEFER if code in (6, 16) else 0), 0, shape=(M, N))
    t.finish()


def test_three_deep_a_ring():
    """RESID_STATS_F16 / _F16_H at 16, 17, 18 K-tiles (K-tiles mod 3 = 1, 2, 0) on 256 tiles, by shape; with bit 16 the same shapes
    on the two-deep 4-wave kernel"""
    t = Tally("quad3")
    regs = lambda code: ("tail", "head", "integer", "random")              # noqa: E731
    _big_loop(t, (9, 18), (1024, 1088, 1152), dict(main=QUAD3, tail=0, ring=3, splits=1, persistent=0), 0, regs_of=regs, shape=(4096, 4096))
    t2 = Tally("quad3.off")
    _big_loop(t2, (9, 18), (1024, 1088, 1152), dict(main=QUAD, tail=0, ring=2, splits=1, persistent=0), F_NOQUAD3, regs_of=regs, shape=(4096, 4096))
    t.msgs += t2.msgs
    t.worst.update({(e + ".bit16", r): w for (e, r), w in t2.worst.items()})
    t.finish()


# ---- remainder rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", (1, 127, 128, 129, 255))
def test_remainder_rows_behind_big_tiles(r):
    """3584 + r rows x 4096 (224 big tiles + a remainder launch of one or two row tiles numbered from 0): the epilogues whose side
    buffers move with the rows -- statistics read (LayerNorm), cleared, added into, the bf16 copy, the fp16 stream.  K = 2048 sends
    the remainder rows through split-K.  The PATCH forms leave the big tiles altogether when M % 256 != 0."""
    M, N = 3584 + r, 4096
    t = Tally(f"remainder.r{r}")

    def want(code, K):
        fam = gc.EPILOGUES[code][2]
        if fam == "patch":
            return dict(main=SMALL, tail=0, ring=2, splits=1)
        ts = _expected_splits(r, N, K)
        main = QUAD if (fam in ("ln", "ln_qgelu") and K >= 512) else PAIR
        if fam == "resid_stats" and code != 8 and K >= 1024:
            main = QUAD3
        return dict(main=main, tail=SMALL, tail_ring=4, tail_splits=ts, splits=1, persistent=0)
    _big_loop(t, ROW_SIDE_CODES, (256, 1024, 2048), want, 0, shape=(M, N))
    t.finish()
