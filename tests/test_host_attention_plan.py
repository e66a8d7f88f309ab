"""The attention and MXFP8-GEMM dispatchers without a GPU: keds_attention_plan_query (csrc/attention_plan.h, the function every 16-bit
attention call launches from) and keds_gemm_mxfp8_plan_query (mxfp8_plan in csrc/gemm_plan.h) against Python models of the rules, and
the attention one against the form table of docs/kernels.md row by row.  The document, the model and the library are three statements
that must agree."""
import ctypes
import itertools
import os
import re

import pytest

from keds_amd import _lib
from tests.conftest import ROOT

NONE, GENERIC, TAIL1, S257 = _lib.ATTN_FORM_NONE, _lib.ATTN_FORM_GENERIC, _lib.ATTN_FORM_TAIL1, _lib.ATTN_FORM_S257
CAUSAL, F16, Q8, PACKED, STOP = (_lib.ATTN_FLAG_CAUSAL, _lib.ATTN_FLAG_F16, _lib.ATTN_FLAG_Q8, _lib.ATTN_FLAG_PACKED,
                                 _lib.ATTN_FLAG_STOP_EVENT)
FIELDS = ("form", "nkt", "nfull", "flags", "grid", "block", "lds", "q_limit")      # keds_attention_last_launch's layout
HOOKS = (0, 16, 32, 48)                                     # keds_attention_debug: bit 4 no S = 257 form at all, bit 5 the 4-wave tail kernel
REFUSED_BITS = (0, 1, 2, 3, 6)
E_ARG = -1


# ---- the model: the four ladders of attention.hip at 8ac08b6 ----------------------------------------------------------------------
def _lds_generic(nkt):                                      # attention.hip:22-30, AttnCfg<NKT>::LDS
    keys = 16 * nkt
    return keys * 64 * 2 + 64 * (keys * 2 + 16)


LDS_TAIL1 = _lds_generic(16) + 256 + 2 * 1056               # :330 TAIL_LDS, :923
LDS_S257 = 65536 + 384 + 264 * 4 + 8 * 72 * 4 + 16 + 256    # :478-482


def _generic(nkt, causal, nfull, f16, q8, packed, grid, q_limit):        # launch_attn<NKT, CAUSAL, NFULL, T>, :975-993: 256 threads
    flags = CAUSAL * causal | F16 * f16 | Q8 * q8 | PACKED * packed
    return [GENERIC, nkt, nfull, flags, grid, 256, _lds_generic(nkt), q_limit]


def _rect(B, S, heads, causal, q_limit, f16, q8, hook):
    """keds_attention_mx (:1020-1041) and keds_attention_h (:1044-1060: the same ladder without q8)"""
    tail, s257 = not hook & 16, not hook & 32               # g_attn_tail, g_attn_s257: :1010-1011
    grid = B * heads
    if q_limit <= 0 or q_limit > S:                         # :1026, :1047
        q_limit = S
    if causal:                                              # :1028-1032, :1049-1053
        return _generic(2 if S <= 32 else 6 if S <= 96 else 18, 1, 0, f16, q8, 0, grid, q_limit)
    if S <= 32:                                             # :1033, :1054
        return _generic(2, 0, 0, f16, q8, 0, grid, q_limit)
    if S <= 96:                                             # :1034, :1055
        return _generic(6, 0, 0, f16, q8, 0, grid, q_limit)
    if S == 257 and tail and s257:                          # :1035-1037, :1056; launch_attn_s257(_q8), :951-973: 512 threads, takes the stop event (:938-949)
        return [S257, 16, 16, F16 * f16 | Q8 * q8 | STOP, grid, 512, LDS_S257, q_limit]
    if S == 257 and not q8 and tail:                        # :1038, :1057; launch_attn_tail1, :920-928
        return [TAIL1, 16, 16, F16 * f16, grid, 256, LDS_TAIL1, q_limit]
    if S >= 256:                                            # :1039, :1058
        return _generic(18, 0, 16, f16, q8, 0, grid, q_limit)
    return _generic(18, 0, 0, f16, q8, 0, grid, q_limit)    # :1040, :1059


def _packed(B, s_max, heads, causal, f16):
    """keds_attention_packed (:1080-1093) and keds_attention_packed_h (:1062-1075): NFULL = 0 at every length, q_limit = s_max, no q8"""
    return _generic(2 if s_max <= 32 else 6 if s_max <= 96 else 18, causal, 0, f16, 0, 1, B * heads, s_max)


def model(B, S, heads, causal, q_limit, f16, q8, packed, hook):
    q8 = q8 and not f16                                     # the fp16 entries have no q8 arguments
    return _packed(B, S, heads, causal, f16) if packed else _rect(B, S, heads, causal, q_limit, f16, q8, hook)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    yield lib
    assert lib.keds_attention_debug(0) == 0
    assert lib.keds_mxfp8_debug(0) == 0


def query(lib, S, causal=0, f16=0, q8=0, packed=0, q_limit=0, hook=0, B=3, heads=2):
    """one keds_attention_plan_query call, checked against the model -> dict of FIELDS"""
    info = (ctypes.c_int * 8)()
    assert lib.keds_attention_debug(hook) == 0
    try:
        _lib.check(lib.keds_attention_plan_query(B, S, heads, causal, q_limit, f16, q8, packed, info), "keds_attention_plan_query")
    finally:
        lib.keds_attention_debug(0)
    assert list(info) == model(B, S, heads, causal, q_limit, f16, q8, packed, hook), (S, causal, f16, q8, packed, q_limit, hook)
    return dict(zip(FIELDS, info))


def test_library_plans_what_the_model_plans_over_the_full_product(lib):
    """S in 1 .. 288 x mask x {bf16, bf16 + MXFP8 rows, fp16} x packed x q_limit in {0, 1, 16, S, S + 1} x hook x (B, heads): 207,360
    plans, all eight ints equal"""
    info = (ctypes.c_int * 8)()
    n, bad = 0, []
    try:
        for hook in HOOKS:
            assert lib.keds_attention_debug(hook) == 0
            for S, causal, (f16, q8), packed, (B, heads) in itertools.product(range(1, 289), (0, 1), ((0, 0), (0, 1), (1, 0)), (0, 1),
                                                                               ((1, 1), (3, 2), (128, 16))):
                for q_limit in (0, 1, 16, S, S + 1):
                    assert lib.keds_attention_plan_query(B, S, heads, causal, q_limit, f16, q8, packed, info) == 0
                    want = model(B, S, heads, causal, q_limit, f16, q8, packed, hook)
                    n += 1
                    if list(info) != want:
                        bad.append((hook, S, causal, f16, q8, packed, B, heads, q_limit, list(info), want))
    finally:
        lib.keds_attention_debug(0)
    assert not bad, f"{len(bad)} plans differ, first (hook, S, causal, f16, q8, packed, B, heads, q_limit, library, model): {bad[0]}"
    assert n == 288 * 2 * 3 * 2 * 5 * 4 * 3


# ---- docs/kernels.md: the attention form table, one test per row ------------------------------------------------------------------
ROWS = ("generic, 2 key tiles", "generic, 6 key tiles", "generic, 18 key tiles, every tile masked", "generic, 18 key tiles, 16 unmasked",
        "4-wave tail kernel", "8-wave S = 257 kernel")
TYPES = ((0, 0), (0, 1), (1, 0))                            # (f16, q8)


def _has(got, **want):
    assert {k: got[k] for k in want} == want, got


def test_the_document_has_exactly_these_attention_rows():
    text = open(os.path.join(ROOT, "docs", "kernels.md"), encoding="utf-8").read()
    table = text[text.index("| form of the 16-bit attention (recorded) | reached by |"):]
    table = table[:table.index("\n\n")]
    assert tuple(re.findall(r"^\| ([^|]+?) \|", table, flags=re.M)[1:]) == ROWS


def test_row_generic_2_and_6_key_tiles(lib):
    for (lo, hi, nkt), causal, (f16, q8), packed, hook in itertools.product(((1, 32, 2), (33, 96, 6)), (0, 1), TYPES, (0, 1), HOOKS):
        for S in (lo, lo + 1, hi - 1, hi):
            got = query(lib, S, causal, f16, q8, packed, hook=hook)
            _has(got, form=GENERIC, nkt=nkt, nfull=0, grid=6, block=256, lds=_lds_generic(nkt), q_limit=S)
            assert got["flags"] == CAUSAL * causal | F16 * f16 | Q8 * (q8 and not packed) | PACKED * packed


def test_row_generic_18_key_tiles_every_tile_masked(lib):
    for S, (f16, q8), hook in itertools.product((97, 255, 256, 257, 258, 288), TYPES, HOOKS):
        _has(query(lib, S, 1, f16, q8, hook=hook), form=GENERIC, nkt=18, nfull=0, block=256, lds=_lds_generic(18))       # causal: at every S
        for causal in (0, 1):                                                                                           # packed: at every s_max
            _has(query(lib, S, causal, f16, q8, packed=1, hook=hook), form=GENERIC, nkt=18, nfull=0, flags=CAUSAL * causal | F16 * f16 | PACKED)
        if S < 256:
            _has(query(lib, S, 0, f16, q8, hook=hook), form=GENERIC, nkt=18, nfull=0)


def test_row_generic_18_key_tiles_16_unmasked(lib):
    for S, (f16, q8), hook in itertools.product((256, 258, 272, 288), TYPES, HOOKS):
        _has(query(lib, S, 0, f16, q8, hook=hook), form=GENERIC, nkt=18, nfull=16, flags=F16 * f16 | Q8 * q8, block=256, lds=_lds_generic(18))
    for (f16, q8), hook in itertools.product(TYPES, (16, 48)):                                       # S = 257: bit 4
        _has(query(lib, 257, 0, f16, q8, hook=hook), form=GENERIC, nkt=18, nfull=16, flags=F16 * f16 | Q8 * q8)
    _has(query(lib, 257, 0, 0, 1, hook=32), form=GENERIC, nkt=18, nfull=16, flags=Q8)               # bit 5 with MXFP8 rows: no tail kernel for them


def test_row_four_wave_tail_kernel(lib):
    for f16, q_limit in itertools.product((0, 1), (0, 1, 256, 257, 300)):
        _has(query(lib, 257, 0, f16, 0, q_limit=q_limit, hook=32), form=TAIL1, nkt=16, nfull=16, flags=F16 * f16, block=256, lds=LDS_TAIL1,
             q_limit=q_limit if 1 <= q_limit <= 257 else 257)
    for S in (256, 258):
        _has(query(lib, S, 0, hook=32), form=GENERIC)


def test_row_eight_wave_s257_kernel(lib):
    for (f16, q8), q_limit in itertools.product(TYPES, (0, 1, 256, 257, 300)):
        _has(query(lib, 257, 0, f16, q8, q_limit=q_limit), form=S257, nkt=16, nfull=16, flags=F16 * f16 | Q8 * q8 | STOP, block=512, lds=LDS_S257,
             q_limit=q_limit if 1 <= q_limit <= 257 else 257)
    _has(query(lib, 257, 0, B=128, heads=16), form=S257, grid=2048)
    for S, causal, packed in ((256, 0, 0), (258, 0, 0), (257, 1, 0), (257, 0, 1), (257, 1, 1)):      # the only form that takes a stop event
        got = query(lib, S, causal, packed=packed)
        assert got["form"] == GENERIC and not got["flags"] & STOP, got


# ---- hook and failure behaviour ---------------------------------------------------------------------------------------------------
def _plans(lib):
    info = (ctypes.c_int * 8)()
    out = []
    for q8 in (0, 1):
        assert lib.keds_attention_plan_query(3, 257, 2, 0, 0, 0, q8, 0, info) == 0
        out.append(list(info))
    return out


def test_refused_hook_bits_leave_the_switches_as_they_were(lib):
    try:
        for base in HOOKS:
            assert lib.keds_attention_debug(base) == 0
            want = _plans(lib)
            assert want == [model(3, 257, 2, 0, 0, 0, q8, 0, base) for q8 in (0, 1)]
            for bit in REFUSED_BITS:
                for other in (0, 16, 32):
                    assert lib.keds_attention_debug(other | 1 << bit) == E_ARG
                    err = _lib.last_error()
                    assert err.startswith("keds_attention_debug: bit ") and re.search(r"bit (0|1|2|3|6)\b", err), err
                    assert _plans(lib) == want, (base, other, bit)
    finally:
        lib.keds_attention_debug(0)


def test_query_with_a_bad_argument_returns_e_arg_and_leaves_info_untouched(lib):
    info = (ctypes.c_int * 8)(*range(100, 108))
    for B, S, heads in [(0, 77, 12), (-1, 77, 12), (3, 0, 12), (3, -5, 12), (3, 289, 12), (3, 77, 0), (3, 77, -2)]:
        assert lib.keds_attention_plan_query(B, S, heads, 0, 0, 0, 0, 0, info) == E_ARG, (B, S, heads)
        assert _lib.last_error().startswith("keds_attention_plan_query: ")
        assert list(info) == list(range(100, 108))
    assert lib.keds_attention_plan_query(3, 77, 12, 0, 0, 0, 0, 0, None) == E_ARG
    assert lib.keds_attention_last_launch(None) == E_ARG


# ---- the MXFP8 GEMM: keds_gemm_mxfp8_ex's decision at 8ac08b6 (gemm_fp8.hip:951-956, launch_mxfp8_quad :921-928) ------------------------
FP8_PAIR, FP8_QUAD = _lib.FP8_FORM_PAIR, _lib.FP8_FORM_QUAD


def mxfp8_model(epilogue, M, N, K, cus, debug):
    tiles = (M // 256) * (N // 256)
    quad = debug == 0 and K % 256 == 0 and K >= 512 and epilogue != 3        # :951, and `if constexpr ((E) != 3)` :954
    if not quad:
        return [FP8_PAIR, tiles, tiles, 0]                  # launch_mxfp8, :908-909
    T = min(cus, 256) & ~7                                  # :922-924
    grid = T if T >= 8 and tiles > T else tiles             # :928
    return [FP8_QUAD, grid, tiles, int(grid < tiles)]


def test_mxfp8_library_plans_what_the_model_plans(lib):
    info = (ctypes.c_int * 4)()
    n, seen = 0, set()
    try:
        for debug in (0, 16):
            assert lib.keds_mxfp8_debug(debug) == 0
            for cus in (8, 64, 256, 304):
                T = min(cus, 256) & ~7
                for epi, K, tiles in itertools.product(range(5), (256, 384, 512, 640, 768, 1024, 4096), (1, T, T + 1, 2 * T + 8)):
                    for M, N in ((tiles * 256, 256), (256, tiles * 256)):
                        _lib.check(lib.keds_gemm_mxfp8_plan_query(epi, M, N, K, cus, info), "keds_gemm_mxfp8_plan_query")
                        assert list(info) == mxfp8_model(epi, M, N, K, cus, debug), (debug, cus, epi, M, N, K)
                        seen.add((info[0], info[3]))
                        n += 1
    finally:
        lib.keds_mxfp8_debug(0)
    assert n == 2 * 4 * 5 * 7 * 4 * 2 and seen == {(FP8_PAIR, 0), (FP8_QUAD, 0), (FP8_QUAD, 1)}


def test_mxfp8_query_applies_the_shape_rules_of_the_gemm_entry(lib):
    info = (ctypes.c_int * 4)(7, 7, 7, 7)
    for epi, M, N, K in [(0, 0, 256, 512), (0, 128, 256, 512), (0, 256, 384, 512), (0, 256, 256, 128), (0, 256, 256, 320), (5, 256, 256, 512),
                         (-1, 256, 256, 512)]:
        assert lib.keds_gemm_mxfp8_plan_query(epi, M, N, K, 256, info) == E_ARG, (epi, M, N, K)
        assert _lib.last_error().startswith("keds_gemm_mxfp8_plan_query: ")
        assert list(info) == [7, 7, 7, 7]
    assert lib.keds_gemm_mxfp8_plan_query(0, 256, 256, 512, 256, None) == E_ARG
