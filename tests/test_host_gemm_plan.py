"""The GEMM dispatcher without a GPU: keds_gemm_plan_query (csrc/gemm_plan.h, the function every keds_gemm_bt* / keds_gemm_x3
call launches from) against a Python model of the rules, against the form table of docs/kernels.md row by row, and
keds_gemm_splits_rows against the same model.  The document, the model and the library are three statements that must agree."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from keds_amd import _lib
from tests.conftest import ROOT

NONE, SMALL, PAIR, QUAD, QUAD3 = (_lib.GEMM_FORM_NONE, _lib.GEMM_FORM_SMALL, _lib.GEMM_FORM_PAIR, _lib.GEMM_FORM_QUAD,
                                   _lib.GEMM_FORM_QUAD3)
DEFER, PROLOGUE = _lib.GEMM_FLAG_DEFER, _lib.GEMM_FLAG_RESID_PROLOGUE
F_SMALL, F_NOSPLIT, F_PROLOGUE, F_QUAD, F_PERSIST, F_PAIR, F_NOQUAD3, F_NODEFER = (
    1, 1 << 9, 1 << 10, 1 << 11, 2 << 11, 3 << 11, 1 << 16, 1 << 17)
F_REFUSED = (1 << 8, 1 << 13, 1 << 14, 1 << 15)           # timing-only forms the library no longer has: keds_gemm_force_small refuses them
PUBLIC = tuple(range(13)) + tuple(range(16, 23))          # the epilogue ids of keds_gemm_bt_ex2
X3 = (13, 14, 15)                                         # ... and of keds_gemm_x3
BIG = tuple(c for c in PUBLIC if c != 12)                 # BIAS_BF16_HEADF32 never takes 256^2 tiles
LN, LN_QGELU, RESID16, PATCH = (6, 7, 10, 11, 16, 17), (7, 11, 17), (9, 18), (5, 21)
MIB = 1 << 20
FIELDS = ("main", "tail", "ring", "tail_ring", "splits", "tail_splits", "persistent", "flags")    # keds_gemm_last_launch's layout


def model(epi, M, N, K, lda, ldc, cus, ws, small_lds, force):
    """The dispatcher of keds_gemm_bt* / keds_gemm_x3 on numpy arrays (or scalars), `force` = the one keds_gemm_force_small
    argument they share -> int64 [..., 8].  Written from launch_gemm / big_tiles_ok / launch_big / quad_by_shape / launch_small
    of gemm.hip as they stood before the decision moved to gemm_plan.h."""
    epi, M, N, K, lda, ldc, cus, ws, small_lds = np.broadcast_arrays(*(np.asarray(v, np.int64) for v in (epi, M, N, K, lda, ldc, cus, ws, small_lds)))
    bit = lambda b: bool((force >> b) & 1)                                              # noqa: E731
    forced = {0: -1, 1: 1, 2: 2, 3: 0}[(force >> 11) & 3]
    ln, ln_qgelu, resid16, x3, patch = (np.isin(epi, ids) for ids in (LN, LN_QGELU, RESID16, X3, PATCH))
    small_lds = small_lds != 0

    def small(rows):                                                                    # launch_small: (ring, splits)
        mt = (rows + 127) // 128
        tiles = mt * (N // 128)
        may = (tiles <= 64) & (K >= 2048) & (not bit(9)) & ~x3
        s = np.ones_like(K)
        for _ in range(4):                                                              # 1 -> 2 -> 4 -> 8 -> 16
            s = np.where(may & (s < 16) & (tiles * s * 2 <= 256) & (K % (s * 2 * 64) == 0) & (K // (s * 2) >= 128), s * 2, s)
        split = may & (s > 1) & (s * mt * 128 * N * 4 <= ws)
        return np.where(split, np.where(small_lds, 2, 4), np.where((tiles <= 256) & ~small_lds, 4, 2)), np.where(split, s, 1)

    bt = (M // 256) * (N // 256)                                                        # big_tiles_ok + launch_gemm's big_ok
    pct = np.where((M % 256 == 0) & (K <= 1024), 50, 85)
    big = ((not bit(0)) & (N % 256 == 0) & (K % 64 == 0) & (K >= 128) & (bt > 0) & (bt * 100 >= (bt + 255) // 256 * 256 * pct) &
           (lda == K) & (ldc == N) & (~patch | (M % 256 == 0)) & (epi != 12))
    by_shape = np.where(ln, K >= 512, np.where(resid16, K >= 1024, x3))                 # quad_by_shape
    quad = np.where(by_shape, 2, 0) if forced < 0 else np.full_like(K, forced)
    T = np.minimum(cus, 256) & ~7                                                       # launch_big
    persistent = (quad == 2) & (bt > T) & (T >= 8) & ~resid16 & (epi != 14)
    ring3 = (quad != 0) & ~persistent & resid16 & (not bit(16)) & (K >= 1024) & (K // 64 >= 4)
    form = np.where(persistent | ((quad != 0) & ~ring3), QUAD, np.where(ring3, QUAD3, PAIR))
    flags = np.where(persistent & ln & ~ln_qgelu & (not bit(17)) & (K // 64 >= 8), DEFER,
                     np.where((form == PAIR) & resid16 & bit(10), PROLOGUE, 0))
    tail = big & (M % 256 != 0)
    ring_all, splits_all = small(M)
    ring_tail, splits_tail = small(M % 256)
    z = np.zeros_like(K)
    return np.stack([np.where(big, form, SMALL), np.where(tail, SMALL, NONE), np.where(big, np.where(ring3, 3, 2), ring_all),
                     np.where(tail, ring_tail, z), np.where(big, 1, splits_all), np.where(tail, splits_tail, z),
                     np.where(big, persistent, z), np.where(big, flags, z)], axis=-1)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    yield lib
    lib.keds_gemm_force_small(0)


def query_many(lib, force, epi, M, N, K, lda, ldc, cus, ws, small_lds):
    """keds_gemm_plan_query for every element of the broadcast arguments -> int64 [n, 8]"""
    cases = np.ascontiguousarray(np.stack([a.ravel() for a in np.broadcast_arrays(
        *(np.asarray(v, np.int64) for v in (epi, M, N, K, lda, ldc, cus, ws, small_lds)))], axis=-1))
    info = np.empty((len(cases), 8), dtype=np.int32)
    lib.keds_gemm_force_small(force)
    try:
        _lib.check(lib.keds_gemm_plan_query_many(len(cases), cases.ctypes.data, info.ctypes.data), "keds_gemm_plan_query_many")
    finally:
        lib.keds_gemm_force_small(0)
    return info.astype(np.int64)


def query(lib, epi, M, N, K, force=0, cus=256, ws=32 * MIB, small_lds=0, lda=None, ldc=None):
    """one keds_gemm_plan_query call -> dict of FIELDS"""
    info = (ctypes.c_int * 8)()
    lib.keds_gemm_force_small(force)
    try:
        _lib.check(lib.keds_gemm_plan_query(epi, M, N, K, lda or K, ldc or N, cus, ws, small_lds, info), "keds_gemm_plan_query")
    finally:
        lib.keds_gemm_force_small(0)
    assert list(info) == [int(v) for v in model(epi, M, N, K, lda or K, ldc or N, cus, ws, small_lds, force)], (epi, M, N, K, force, cus)
    return dict(zip(FIELDS, info))


# ---- the model, everywhere ---------------------------------------------------------------------------------------------------------
SWEEP_M = (1, 7, 127, 128, 129, 255, 256, 257, 1024, 1025, 2048, 2170, 3584, 3585, 3584 + 127, 3584 + 128, 3584 + 129, 3584 + 255,
           4096, 11008, 19712, 32768, 32896)
SWEEP_N = (128, 256, 384, 768, 1024, 2048, 3072, 4096)
SWEEP_K = (64, 128, 192, 448, 512, 576, 1024, 1088, 2048, 2176, 2304, 2560, 3072, 4096)
SWEEP_FORCE = (0, F_SMALL, F_NOSPLIT, F_PROLOGUE, F_NOQUAD3, F_NODEFER, F_QUAD, F_PERSIST, F_PAIR)
SWEEP_CUS = (8, 64, 256, 304)
SWEEP_WS = (0, MIB, 32 * MIB)


def test_library_plans_what_the_model_plans_over_the_full_product(lib):
    """M x N x K x epilogue x force x cus x scratch x small-LDS x {dense, padded strides}: 25.6 M plans, all eight ints equal.
    (The PATCH epilogues want a dense output, as in keds_gemm_bt_ex2: their padded case pads lda only.)"""
    M, N, K, cus, ws, small_lds, padded = (a.ravel() for a in np.meshgrid(SWEEP_M, SWEEP_N, SWEEP_K, SWEEP_CUS, SWEEP_WS, (0, 1), (0, 1),
                                                                          indexing="ij"))
    lda = K + 72 * padded
    n = 0
    for epi in PUBLIC + X3:
        ldc = N + (0 if epi in PATCH else 40) * padded
        for force in SWEEP_FORCE:
            got = query_many(lib, force, epi, M, N, K, lda, ldc, cus, ws, small_lds)
            want = model(epi, M, N, K, lda, ldc, cus, ws, small_lds, force)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (f"{bad.size} plans differ, first: epilogue {epi} force {force:#x} M {M[bad[0]]} N {N[bad[0]]} K {K[bad[0]]} "
                                   f"lda {lda[bad[0]]} ldc {ldc[bad[0]]} cus {cus[bad[0]]} ws {ws[bad[0]]} small_lds {small_lds[bad[0]]}: "
                                   f"library {got[bad[0]].tolist()}, model {want[bad[0]].tolist()}")
            n += len(got)
    assert n == 23 * 8 * 14 * 23 * len(SWEEP_FORCE) * 4 * 3 * 2 * 2 and len(SWEEP_FORCE) == 9


def test_refused_force_bits_leave_the_switches_as_they_were(lib):
    """Bit 8 and bits 13-15 selected timing-only launches that are gone: the hook says so, names the bit, and the plans stay those
    of the bits set before -- here F_PAIR, then none."""
    cases = [(code, M, 1024, K) for code in (6, 9, 10) for M in (2048, 32896) for K in (1024, 4096)]
    info = (ctypes.c_int * 8)()
    try:
        for base in (F_PAIR, 0):
            for bad in F_REFUSED + (F_PAIR | 1 << 8, 7 << 13):
                assert lib.keds_gemm_force_small(base) == 0
                assert lib.keds_gemm_force_small(bad) == -1                               # KEDS_E_ARG
                err = _lib.last_error()
                assert err.startswith("keds_gemm_force_small: bit ") and re.search(r"bit (8|13|14|15)\b", err), err
                for epi, M, N, K in cases:
                    _lib.check(lib.keds_gemm_plan_query(epi, M, N, K, K, N, 256, 32 * MIB, 0, info), "keds_gemm_plan_query")
                    assert list(info) == [int(v) for v in model(epi, M, N, K, K, N, 256, 32 * MIB, 0, base)], (base, bad, epi, M, K)
    finally:
        lib.keds_gemm_force_small(0)


def test_query_applies_the_shape_rules_of_the_gemm_entry(lib):
    info = (ctypes.c_int * 8)()
    for epi, M, N, K, lda, ldc in [(0, 256, 192, 64, 64, 192), (0, 256, 128, 96, 96, 128), (0, 256, 128, 64, 60, 128), (0, 256, 128, 64, 64, 132),
                                   (0, 0, 128, 64, 64, 128), (5, 257, 128, 64, 64, 168), (21, 257, 128, 64, 64, 168), (23, 256, 128, 64, 64, 128),
                                   (-1, 256, 128, 64, 64, 128)]:
        assert lib.keds_gemm_plan_query(epi, M, N, K, lda, ldc, 256, 0, 0, info) == -1, (epi, M, N, K, lda, ldc)      # KEDS_E_ARG
        assert _lib.last_error().startswith("keds_gemm_plan_query: ")
    assert lib.keds_gemm_plan_query(0, 256, 128, 64, 64, 128, 256, 0, 0, None) == -1


# ---- docs/kernels.md: the form table, one test per row ---------------------------------------------------------------------------
ROWS = ("128², ring 4", "128², ring 2", "128², ring 4, split-K 2 / 4 / 8 / 16 + reduce", "256², 8 waves", "256², 4 waves, one tile per workgroup",
        "256², 4 waves, persistent", "256², 4 waves, three-deep A ring", "big tiles + 128² remainder launch (ring 4; split-K at K = 2048)")
CUS_T = ((128, 128), (256, 256), (304, 256))              # (CUs, T = min(CUs, 256) & ~7); below 128 CUs the shapes leave the 256² tiles
BIG_M, BIG_N = 2048, 4096                                 # 128 tiles


def _has(got, **want):
    assert {k: got[k] for k in want} == want, got


def test_the_document_has_exactly_these_rows():
    text = open(os.path.join(ROOT, "docs", "kernels.md"), encoding="utf-8").read()
    table = text[text.index("| form (recorded) | reached by |"):]
    table = table[:table.index("\n\n")]
    assert tuple(re.findall(r"^\| ([^|]+?) \|", table, flags=re.M)[1:]) == ROWS


def test_row_small_kernel_ring_4(lib):
    for M, N, K, code in itertools.product((1, 7, 127, 128, 129, 255, 256, 257), (128, 384), (64, 128, 192, 256, 320), PUBLIC):
        _has(query(lib, code, M, N, K), main=SMALL, tail=NONE, ring=4, splits=1, persistent=0, flags=0)
        _has(query(lib, code, M, N, K, lda=K + 72, ldc=None if code in PATCH else N + 40), main=SMALL, tail=NONE, ring=4, splits=1)


def test_row_small_kernel_ring_2(lib):
    for K, code in itertools.product((64, 128, 192), PUBLIC):
        _has(query(lib, code, 2170, 2048, K, force=F_SMALL), main=SMALL, tail=NONE, ring=2, splits=1, persistent=0, flags=0)


def test_row_split_k(lib):
    for code in PUBLIC:
        for M, N, K in itertools.product((1, 7, 129, 1024), (128, 384, 1024), (2048, 2176, 2304, 2560, 4096)):
            got = query(lib, code, M, N, K)
            _has(got, main=SMALL, tail=NONE, ring=4, persistent=0)
            assert got["splits"] in (2, 4, 8, 16), (M, N, K, got)
        for M, N, K, splits in [(1, 1024, 2048, 16), (1, 1024, 2176, 2), (129, 1024, 2304, 4), (129, 1024, 4096, 16), (129, 1024, 2560, 8),
                                (1024, 1024, 2048, 4), (1024, 1024, 2304, 4), (129, 384, 2176, 2), (7, 128, 4096, 16)]:
            _has(query(lib, code, M, N, K), main=SMALL, ring=4, splits=splits)
        _has(query(lib, code, 1025, 1024, 2048), main=SMALL, ring=4, splits=1)                       # 72 tiles
        _has(query(lib, code, 129, 1024, 2304, force=F_NOSPLIT), main=SMALL, ring=4, splits=1)       # bit 9
        _has(query(lib, code, 129, 1024, 2304, ws=0), main=SMALL, ring=4, splits=1)                  # no workspace


def test_row_eight_wave_kernel(lib):
    for cus, _ in CUS_T:
        for K, code in itertools.product((128, 192, 256, 1024), BIG):
            _has(query(lib, code, BIG_M, BIG_N, K, force=F_PAIR, cus=cus), main=PAIR, tail=NONE, ring=2, splits=1, persistent=0, flags=0)
        for K, code in itertools.product((128, 192, 256, 1024), (0, 1, 2, 3, 4, 5, 8, 19, 20, 21, 22)):      # the plain epilogues, by shape
            _has(query(lib, code, BIG_M, BIG_N, K, cus=cus), main=PAIR, tail=NONE, ring=2, splits=1, persistent=0, flags=0)
        for K, code in itertools.product((128, 192, 256, 1024), RESID16):
            _has(query(lib, code, BIG_M, BIG_N, K, force=F_PROLOGUE | F_PAIR, cus=cus), main=PAIR, tail=NONE, ring=2, splits=1, flags=PROLOGUE)
    _has(query(lib, 12, BIG_M, BIG_N, 1024, force=F_PAIR), main=SMALL)


def test_row_four_wave_kernel_one_tile_per_workgroup(lib):
    for cus, T in CUS_T:
        for K, code in itertools.product((128, 192, 256, 448, 512), BIG):
            _has(query(lib, code, BIG_M, BIG_N, K, force=F_QUAD, cus=cus), main=QUAD, tail=NONE, ring=2, splits=1, persistent=0, flags=0)
        if BIG_M // 256 * (BIG_N // 256) <= T:
            for K, code in itertools.product((512, 1024), LN):
                _has(query(lib, code, BIG_M, BIG_N, K, cus=cus), main=QUAD, tail=NONE, ring=2, splits=1, persistent=0, flags=0)
            for code in LN:
                _has(query(lib, code, BIG_M, BIG_N, 448, cus=cus), main=PAIR)


def test_row_four_wave_kernel_persistent(lib):
    for cus, T in CUS_T:
        for M, N in [((T + 1) * 256, 256), ((T + T // 2) // 4 * 256, 1024), (2 * T // 16 * 256, 4096), ((2 * T + 8) // 8 * 256, 2048)]:
            assert (M // 256) * (N // 256) > T
            for kt, code in itertools.product((2, 3, 7, 8, 9, 16), LN + (0, 22)):
                defer = DEFER if code in (6, 10, 16) and kt >= 8 else 0
                _has(query(lib, code, M, N, kt * 64, force=F_PERSIST, cus=cus), main=QUAD, tail=NONE, ring=2, splits=1, persistent=1, flags=defer)
                _has(query(lib, code, M, N, kt * 64, force=F_PERSIST | F_NODEFER, cus=cus), main=QUAD, ring=2, persistent=1, flags=0)
                if code in LN and kt >= 8:                                                           # by shape
                    _has(query(lib, code, M, N, kt * 64, cus=cus), main=QUAD, tail=NONE, ring=2, splits=1, persistent=1, flags=defer)
        _has(query(lib, 6, T * 256, 256, 512, force=F_PERSIST, cus=cus), main=QUAD, persistent=0)    # T tiles: one each
    for code in RESID16:                                                                             # the residual epilogue never
        _has(query(lib, code, 4096, 4096, 512, force=F_PERSIST, cus=128), main=QUAD, ring=2, persistent=0)


def test_row_three_deep_a_ring(lib):
    for (cus, _), kt, code in itertools.product(CUS_T, (16, 17, 18), RESID16):
        _has(query(lib, code, 4096, 4096, kt * 64, cus=cus), main=QUAD3, tail=NONE, ring=3, splits=1, persistent=0, flags=0)
        _has(query(lib, code, 4096, 4096, kt * 64, force=F_NOQUAD3, cus=cus), main=QUAD, tail=NONE, ring=2, splits=1, persistent=0, flags=0)
    for code in RESID16:
        _has(query(lib, code, 4096, 4096, 960), main=PAIR, ring=2)                                   # K < 1024: the 8-wave kernel


def test_row_remainder_launch_behind_big_tiles(lib):
    for r, K in itertools.product((1, 127, 128, 129, 255), (256, 1024, 2048)):
        M, N = 3584 + r, 4096
        for code in (6, 7, 10, 16, 17, 8, 9, 18):
            got = query(lib, code, M, N, K)
            main = QUAD if code in LN and K >= 512 else QUAD3 if code in RESID16 and K >= 1024 else PAIR
            _has(got, main=main, tail=SMALL, tail_ring=4, splits=1, persistent=0)
            assert (got["tail_splits"] > 1) == (K == 2048), got
        for code in PATCH:
            _has(query(lib, code, M, N, K), main=SMALL, tail=NONE, ring=2, splits=1)


# ---- docs/kernels.md: the split-operand table (keds_gemm_x3, epilogues 13 - 15), one test per row ----------------------------------
X3_ROWS = ("128², ring 4", "128², ring 2", "no split-K", "256², 8 waves", "256², 4 waves, one tile per workgroup", "256², 4 waves, persistent",
           "big tiles + remainder")
X3_BIG_K = (128, 192, 1024)


def test_the_document_has_exactly_these_split_operand_rows():
    text = open(os.path.join(ROOT, "docs", "kernels.md"), encoding="utf-8").read()
    assert text.index("| form (recorded) | reached by |") < text.index("| form of `keds_gemm_x3` (recorded) | reached by |")
    table = text[text.index("| form of `keds_gemm_x3` (recorded) | reached by |"):]
    table = table[:table.index("\n\n")]
    assert tuple(re.findall(r"^\| ([^|]+?) \|", table, flags=re.M)[1:]) == X3_ROWS


def test_x3_row_small_kernel_ring_4(lib):
    for cus, _ in CUS_T:
        for M, N, K, code in itertools.product((1, 7, 127, 128, 129, 255, 256, 257), (128, 384), (64, 128, 192, 320), X3):
            _has(query(lib, code, M, N, K, cus=cus), main=SMALL, tail=NONE, ring=4, splits=1, persistent=0, flags=0)
            _has(query(lib, code, M, N, K, cus=cus, lda=K + 72, ldc=N + 40), main=SMALL, tail=NONE, ring=4, splits=1, persistent=0, flags=0)


def test_x3_row_small_kernel_ring_2(lib):
    for (cus, _), K, code in itertools.product(CUS_T, (64, 128), X3):
        _has(query(lib, code, 2170, 2048, K, force=F_SMALL, cus=cus), main=SMALL, tail=NONE, ring=2, splits=1, persistent=0, flags=0)


def test_x3_row_no_split_k(lib):
    """16 tiles at K = 2048 with the workspace registered: every other epilogue splits, gemm_may_split excludes these"""
    for (cus, _), code in itertools.product(CUS_T, X3):
        _has(query(lib, code, 129, 1024, 2048, cus=cus), main=SMALL, tail=NONE, ring=4, splits=1, persistent=0, flags=0)
    assert query(lib, 19, 129, 1024, 2048)["splits"] > 1


def test_x3_row_eight_wave_kernel(lib):
    for (cus, _), K, code in itertools.product(CUS_T, X3_BIG_K, X3):
        _has(query(lib, code, BIG_M, BIG_N, K, force=F_PAIR, cus=cus), main=PAIR, tail=NONE, ring=2, splits=1, persistent=0, flags=0)


def test_x3_row_four_wave_kernel_one_tile_per_workgroup(lib):
    for (cus, T), K, code in itertools.product(CUS_T, X3_BIG_K, X3):
        assert BIG_M // 256 * (BIG_N // 256) <= T
        _has(query(lib, code, BIG_M, BIG_N, K, cus=cus), main=QUAD, tail=NONE, ring=2, splits=1, persistent=0, flags=0)


def test_x3_row_four_wave_kernel_persistent(lib):
    for cus, T in CUS_T:
        for M, N in [((T + 1) * 256, 256), (3 * T // 8 * 256, 1024), ((2 * T + 8) * 256, 256)]:
            assert (M // 256) * (N // 256) > T
            for K, code in itertools.product((128, 192, 576, 1024), X3):
                _has(query(lib, code, M, N, K, cus=cus), main=QUAD, tail=NONE, ring=2, splits=1, persistent=int(code != 14), flags=0)
        for code in X3:                                                                              # T tiles: one each
            _has(query(lib, code, T * 256, 256, 576, cus=cus), main=QUAD, persistent=0)


def test_x3_row_remainder_launch_behind_big_tiles(lib):
    for (cus, T), r, K, code in itertools.product(CUS_T, (1, 127, 129, 255), (256, 1024), X3):
        _has(query(lib, code, 3584 + r, 4096, K, cus=cus), main=QUAD, tail=SMALL, ring=2, tail_ring=4, splits=1, tail_splits=1,
             persistent=int(224 > T and code != 14), flags=0)


# ---- keds_gemm_splits_rows: whether a tower runs two lanes (tower_plan.h, tower_splits_rows) -----------------------------------------
def test_splits_rows_is_the_models_remainder_launch(lib):
    splits_rows = getattr(lib, "_Z21keds_gemm_splits_rowsiii")      # bool keds_gemm_splits_rows(int, int, int): library-internal, C++
    splits_rows.restype, splits_rows.argtypes = ctypes.c_bool, [ctypes.c_int] * 3
    seen = set()
    for w in (128, 768, 1024):
        for M in [B * 257 for B in (1, 2, 127, 128)] + [B * 77 for B in (1, 128, 256)]:
            for N, K in [(3 * w, w), (w, w), (4 * w, w), (w, 4 * w)]:
                want = bool(model(0, M, N, K, K, N, 256, 0, 0, 0)[1] != NONE)
                assert splits_rows(M, N, K) == want, (M, N, K)
                seen.add(want)
    assert seen == {False, True}
