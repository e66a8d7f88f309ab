"""The test / A/B hooks of the library without a GPU: every form they still select computes correct results, and the values that
selected a timing-only kernel (last at 14f64ac) are refused -- KEDS_E_ARG, an error that names the hook and the bit, the previous
state kept -- instead of silently ignored."""
import ctypes
import os

import pytest

from keds_amd import _lib

E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    yield lib
    for hook in (lib.keds_attention_debug, lib.keds_scan_debug, lib.keds_mxfp8_debug, lib.keds_gemm_force_small):
        assert hook(0) == 0


def _refused(lib, hook, value, *bits):
    assert getattr(lib, hook)(value) == E_ARG, (hook, value)
    err = _lib.last_error()
    assert err.startswith(hook + ": "), err
    assert any(f"bit {b} " in err for b in bits) or f"value {value} " in err, err


def test_attention_debug_accepts_the_two_routing_bits_and_refuses_the_ablations(lib):
    for ok in (0, 16, 32, 48, 0):
        assert lib.keds_attention_debug(ok) == 0, ok
    for bit in (0, 1, 2, 3, 6):
        for base in (0, 16, 48):
            _refused(lib, "keds_attention_debug", base | 1 << bit, bit)
    _refused(lib, "keds_attention_debug", 64 + 8, 3, 6)          # what the stamped S = 257 build was asked for with
    _refused(lib, "keds_attention_debug", 5, 0, 2)


def _search_plan(lib):
    out = (ctypes.c_int32 * 10)()
    _lib.check(lib.keds_index_search_plan_query(128, 768, 500000, 10, 256, out), "keds_index_search_plan_query")
    return list(out)


def test_scan_debug_accepts_bits_4_to_9_and_refuses_the_ablations_and_the_fused_tail(lib):
    for ok in (0, 1 << 4, 1 << 5, 1 << 6, 1 << 7, 4 << 7, 7 << 7, 0x3F0, 0):
        assert lib.keds_scan_debug(ok) == 0, ok
    by_shape = _search_plan(lib)
    assert by_shape[0] == 1                                      # two phases at 0.5 M rows
    assert lib.keds_scan_debug(1 << 4 | 4 << 7) == 0             # single phase, threshold depth 4: both show in the plan
    forced = _search_plan(lib)
    assert forced[0] == 0 and forced[5] == 4 and forced != by_shape
    for bit in (0, 1, 2, 3, 10):
        for base in (0, 1 << 5, 0x3F0):
            _refused(lib, "keds_scan_debug", base | 1 << bit, bit)
            assert _search_plan(lib) == forced                   # the state of the last accepted call
    assert lib.keds_scan_debug(0) == 0
    assert _search_plan(lib) == by_shape


def test_mxfp8_debug_accepts_0_and_16_only(lib):
    for ok in (0, 16, 0):
        assert lib.keds_mxfp8_debug(ok) == 0, ok
    for bad in (1, 2, 3, 4, 5, 8, 15, 17, 32, 16 + 1, -1):
        _refused(lib, "keds_mxfp8_debug", bad)


def _gemm_plans(lib):
    plans = []
    info = (ctypes.c_int * 8)()
    for epi, M, K in ((6, 32896, 1024), (9, 32896, 4096), (10, 2048, 1024), (0, 300, 4096)):
        _lib.check(lib.keds_gemm_plan_query(epi, M, 1024, K, K, 1024, 256, 32 << 20, 0, info), "keds_gemm_plan_query")
        plans.append(list(info))
    return plans


def test_gemm_force_small_refuses_bit_8_and_bits_13_to_15(lib):
    accepted = (1, 1 << 9, 1 << 10, 1 << 11, 2 << 11, 3 << 11, 1 << 16, 1 << 17, 1 | 1 << 9 | 1 << 10 | 3 << 11 | 1 << 16 | 1 << 17, 0)
    for ok in accepted:
        assert lib.keds_gemm_force_small(ok) == 0, ok
    by_shape = _gemm_plans(lib)
    assert by_shape[0][1] == 1 and by_shape[0][6] == 1           # full tiles persistent + a remainder launch
    for bit in (8, 13, 14, 15):
        for base in (0, 3 << 11, 1 << 17):
            _refused(lib, "keds_gemm_force_small", base | 1 << bit, bit)
            assert _gemm_plans(lib) == by_shape                  # keds_gemm_plan_query answers as with 0
    _refused(lib, "keds_gemm_force_small", 7 << 13, 13, 14, 15)
    assert lib.keds_gemm_force_small(3 << 11) == 0
    forced = _gemm_plans(lib)
    assert forced != by_shape
    _refused(lib, "keds_gemm_force_small", 1 << 8, 8)
    assert _gemm_plans(lib) == forced                            # ... and otherwise as with the last accepted bits
    assert lib.keds_gemm_force_small(0) == 0


def test_the_stamp_buffers_and_the_filler_switch_left_the_library(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "keds_scan_debug")                       # (the probe finds what is there)
    for name in ("keds_merge_stamp_buffer", "keds_attention_stamp_buffer", "keds_tower_fill_enable"):
        assert not hasattr(raw, name), name
        assert name not in _lib.SIGNATURES


def test_the_attention_stop_event_protocol_left_the_library_and_the_plan_entries_arrived(lib):
    """keds_attention_stop_event / keds_attention_stop_event_taken were C++ symbols (mangled: no dlsym by their plain names), so the
    library's bytes are searched: its symbol and string tables must not name them.  The event is an argument of keds_attention16 now."""
    raw = ctypes.CDLL(_lib.LIB_PATH)
    image = open(_lib.LIB_PATH, "rb").read()
    assert b"keds_attention16" in image                          # (the probe finds what is there)
    for gone in (b"keds_attention_stop_event_taken", b"keds_attention_stop_event"):
        assert gone not in image, gone
    for name in ("keds_attention_plan_query", "keds_attention_last_launch", "keds_gemm_mxfp8_plan_query"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES


def test_the_knowledge_stream_kernels_have_entries_of_their_own(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("keds_cross_attn_core", "keds_cross_core_f32", "keds_knowledge_pack_rows", "keds_place_token"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
