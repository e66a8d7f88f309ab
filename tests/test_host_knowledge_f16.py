"""No GPU: the extension header include/keds_knowledge_f16.h (the knowledge stream on the fp16 matrix instruction) parses with the
project's parser into a table of its own, leaves the select extension's table what it was, every function it declares is exported
and bound, its table equals tests/golden/abi_knowledge_f16_v1.json, the refusals it promises come back as KEDS_E_ARG with a message
before anything is launched, and the planner sends the three new epilogue ids to the 128 x 128 kernel forms only."""
import ctypes as C
import json
import os
import re
import sys

import pytest

from keds_amd import _abi, _lib
from tests.conftest import ROOT, golden_path
from tests.test_host_abi import _lock_table

LOCK = golden_path("abi_knowledge_f16_v1.json")
HEADER = os.path.join(ROOT, "include", "keds_knowledge_f16.h")
FUNCTIONS = ["keds_cross_attn_core_h", "keds_knowledge_pack_rows_h", "keds_crossformer_fuse_f16", "keds_im2text_forward_f16",
             "keds_crossformer_forward_f16", "keds_knowledge_f16_workspace_bytes", "keds_knowledge_run_f16"]
CONSTANTS = {"KEDS_EPI_BIAS_F16_H": 32, "KEDS_EPI_BIAS_RELU_F16_H": 33, "KEDS_EPI_BIAS_F16_H_HEADF32": 34}
A = 0x7F0000001000                                                # a non-null address: every refusal comes before any access


def _table():
    return _lock_table(dict(_lib.STRUCTS), _lib.KF16_SIGNATURES)


def test_the_header_parses_into_a_third_table():
    assert _abi.KNOWLEDGE_F16_HEADERS == ("keds_knowledge_f16.h",)
    text = open(HEADER).read()
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.findall(r'#\s*include\s+(\S+)', bare) == ['"keds_hip.h"']           # the core header and nothing else
    k = _lib.KF16_ABI
    assert list(k.functions) == FUNCTIONS == re.findall(r"\b(keds_[a-z0-9_]+)\s*\(", bare)
    assert k.constants == CONSTANTS and k.structs == {} and k.handles == []
    assert (_lib.EPI_BIAS_F16_H, _lib.EPI_BIAS_RELU_F16_H, _lib.EPI_BIAS_F16_H_HEADF32) == (32, 33, 34)
    assert k == _abi.parse_ext_headers(_abi.KNOWLEDGE_F16_HEADERS)
    core = [(f"include/{h}", open(os.path.join(ROOT, "include", h)).read()) for h in _abi.HEADERS]
    whole = _abi.parse(core + [("include/keds_knowledge_f16.h", text)])
    assert {n: whole.functions[n] for n in FUNCTIONS} == k.functions
    assert not set(FUNCTIONS) & (set(_lib.ABI.functions) | set(_lib.EXT_ABI.functions))
    # each entry is the bf16 entry's parameter list, with range_flag in front of the stream where the header says so
    f, flag = {**_lib.ABI.functions, **k.functions}, _abi.Type("int32_t", 1)
    for new, old, added in (("keds_cross_attn_core_h", "keds_cross_attn_core", []), ("keds_knowledge_pack_rows_h", "keds_knowledge_pack_rows", []),
                            ("keds_crossformer_fuse_f16", "keds_crossformer_fuse", []), ("keds_im2text_forward_f16", "keds_im2text_forward", [flag]),
                            ("keds_crossformer_forward_f16", "keds_crossformer_forward", [flag]),
                            ("keds_knowledge_run_f16", "keds_knowledge_run", [flag])):
        assert f[new][0] == f[old][0] and f[new][1] == f[old][1][:-1] + added + f[old][1][-1:], new
    assert f["keds_knowledge_f16_workspace_bytes"] == f["keds_knowledge_workspace_bytes"]


def test_the_select_extension_and_the_core_are_what_they_were():
    assert _abi.EXT_HEADERS == ("keds_select.h",) and _abi.HEADERS == ("keds_hip.h", "keds_session.h")
    ext = _lib.EXT_ABI
    assert ext == _abi.parse_ext_headers() == _abi.parse_ext_headers(_abi.EXT_HEADERS)
    assert list(ext.functions) == ["keds_sel_build", "keds_index_search_packed_sel", "keds_search_scan_sel", "keds_search_certify_sel",
                                   "keds_search_exact_sel"]
    assert ext.constants == {"KEDS_SEL_MAX_EXCLUDE": 16} and ext.structs == {} and ext.handles == []
    assert _lib.ABI_VERSION == 15 and not set(CONSTANTS) & set(_lib.ABI.constants)
    with open(golden_path("abi_select_v1.json")) as fh:
        assert sorted(json.load(fh)) == sorted(_lib.EXT_SIGNATURES)


def test_every_declared_function_is_exported_and_bound():
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in FUNCTIONS:
        assert hasattr(raw, name), f"{name} is not exported"
        res, args = _lib.KF16_SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args and len(args) == len(_lib.KF16_ABI.functions[name][1])
        assert res is (C.c_size_t if name.endswith("workspace_bytes") else C.c_int)


def test_function_table_equals_the_lock():
    """python -m tests.test_host_knowledge_f16 rewrites the lock; its diff is then the change of the extension's ABI"""
    with open(LOCK) as f:
        lock = json.load(f)
    table = _table()
    assert sorted(table) == sorted(lock) == sorted(FUNCTIONS)
    assert {n: table[n] for n in table if table[n] != lock[n]} == {}
    assert lock["keds_cross_attn_core_h"] == ["int32", ["pointer"] * 4 + ["int32"] * 4 + ["pointer"]]


def _refused(rc_, *words):
    msg = _lib.last_error()
    assert rc_ == _lib.E_ARG, (rc_, msg)
    assert all(w in msg for w in words), msg


def _i2t(dim_in=128, middle=128, dim_out=128, n_layer=2, out_w=A):
    p = _lib.Im2TextParams()
    p.dim_in, p.middle, p.dim_out, p.n_layer = dim_in, middle, dim_out, n_layer
    for i in range(4):
        p.w[i], p.b[i] = A, A
    p.out_w, p.out_b = out_w, A
    return p


def _xf(dim=128, heads=2, layers=2, with_layers=True):
    arr = (_lib.CrossLayerParams * max(layers, 1))()
    p = _lib.CrossFormerParams(dim, heads, layers, arr if with_layers else None, None)
    p._keep = arr
    return p


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    core = lambda *a: lib.keds_cross_attn_core_h(*a, None)                        # noqa: E731
    for K in (0, 33, -1):
        _refused(core(A, A, A, A, 1, K, 1, 64), "keds_cross_attn_core_h", "[1,32]")
    _refused(core(A, A, A, A, 1, 4, 2, 127), "keds_cross_attn_core_h", "kv_ld=127", "64 heads")
    _refused(core(A, A, A, A, 1, 4, 0, 64), "keds_cross_attn_core_h", "bad argument")
    _refused(core(A, A, A, A, 0, 4, 1, 64), "keds_cross_attn_core_h", "bad argument")
    for i in range(4):
        a = [A] * 4
        a[i] = None
        _refused(core(*a, 1, 4, 1, 64), "keds_cross_attn_core_h", "bad argument")
        _refused(lib.keds_knowledge_pack_rows_h(*a, 1, 1, 8, None), "keds_knowledge_pack_rows_h", "bad argument")
    for dim in (4, 12, 129):
        _refused(lib.keds_knowledge_pack_rows_h(A, A, A, A, 1, 1, dim, None), "keds_knowledge_pack_rows_h", "multiple of 8")
    _refused(lib.keds_knowledge_pack_rows_h(A, A, A, A, 1, 0, 8, None), "keds_knowledge_pack_rows_h", "bad argument")
    # fuse: nine layers, a short buffer, bad module shapes
    fz = _lib.CrossFormerFused()
    p9 = _xf(layers=9)
    assert lib.keds_crossformer_fused_bytes(C.byref(p9)) == 0
    _refused(lib.keds_crossformer_fuse_f16(C.byref(p9), A, 1 << 30, C.byref(fz), None), "keds_crossformer_fuse_f16", "8 layers")
    p2 = _xf()
    _refused(lib.keds_crossformer_fuse_f16(C.byref(p2), A, lib.keds_crossformer_fused_bytes(C.byref(p2)) - 1, C.byref(fz), None),
             "keds_crossformer_fuse_f16", "too small")
    _refused(lib.keds_crossformer_fuse_f16(C.byref(p2), None, 1 << 30, C.byref(fz), None), "keds_crossformer_fuse_f16", "bad argument")
    for bad in (_xf(dim=130), _xf(heads=1), _xf(heads=0), _xf(layers=0), _xf(with_layers=False)):
        _refused(lib.keds_crossformer_fuse_f16(C.byref(bad), A, 1 << 30, C.byref(fz), None), "keds_crossformer_fuse_f16", "CrossFormer parameters")
        _refused(lib.keds_crossformer_forward_f16(C.byref(bad), A, A, A, 1, 4, A, A, 1 << 30, None, None), "keds_crossformer_forward_f16",
                 "CrossFormer parameters")
    # IM2TEXT
    i2t = lambda p, x=A, rows=1, out=A, ws=A: lib.keds_im2text_forward_f16(C.byref(p), x, rows, out, ws, 1 << 30, A, None)   # noqa: E731
    for bad in (_i2t(n_layer=0), _i2t(n_layer=5), _i2t(out_w=None)):
        _refused(i2t(bad), "keds_im2text_forward_f16", "IM2TEXT parameters")
    for bad in (_i2t(dim_in=100), _i2t(middle=192), _i2t(dim_out=64)):
        _refused(i2t(bad), "keds_im2text_forward_f16", "multiples of 128")
    good = _i2t()
    for kw in (dict(x=None), dict(out=None), dict(ws=None), dict(rows=0)):
        _refused(i2t(good, **kw), "keds_im2text_forward_f16", "bad argument")
    # CrossFormer
    xf = lambda K=4, q=A, k=A, v=A, out=A, ws=A, B=1: lib.keds_crossformer_forward_f16(C.byref(p2), q, k, v, B, K, out, ws, 1 << 30, A, None)   # noqa: E731
    for K in (0, 33, -1):
        _refused(xf(K), "keds_crossformer_forward_f16", "[1,32]")
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(ws=None), dict(B=0)):
        _refused(xf(**kw), "keds_crossformer_forward_f16", "bad argument")
    # the stream
    kp = _lib.KnowledgeParams(_i2t(), _xf(), _xf())
    run = lambda p, K=4, B=1, q=A, ni=A, nt=A, out=A, ws=A: lib.keds_knowledge_run_f16(C.byref(p), q, ni, nt, B, K, out, ws, 1 << 30, A, None)   # noqa: E731
    for K in (0, 33, -1):
        _refused(run(kp, K), "keds_knowledge_run_f16", "[1,32]")
    _refused(run(kp, B=0), "keds_knowledge_run_f16", "[1,32]")
    for kw in (dict(q=None), dict(ni=None), dict(nt=None), dict(out=None), dict(ws=None)):
        _refused(run(kp, **kw), "keds_knowledge_run_f16", "null pointer")
    _refused(lib.keds_knowledge_run_f16(None, A, A, A, 1, 4, A, A, 1 << 30, A, None), "keds_knowledge_run_f16", "null pointer")
    _refused(run(_lib.KnowledgeParams(_i2t(n_layer=0), _xf(), _xf())), "keds_knowledge_run_f16", "IM2TEXT parameters")
    _refused(run(_lib.KnowledgeParams(_i2t(), _xf(heads=1), _xf())), "keds_knowledge_run_f16", "CrossFormer parameters")
    _refused(run(_lib.KnowledgeParams(_i2t(), _xf(), _xf(dim=100))), "keds_knowledge_run_f16", "CrossFormer parameters")
    _refused(run(_lib.KnowledgeParams(_i2t(), _xf(dim=256), _xf())), "keds_knowledge_run_f16", "dims must agree")
    _refused(run(_lib.KnowledgeParams(_i2t(), _xf(), _xf(heads=4))), "keds_knowledge_run_f16", "dims must agree")
    _refused(run(_lib.KnowledgeParams(_i2t(dim_in=256), _xf(), _xf())), "keds_knowledge_run_f16", "dims must agree")
    assert lib.keds_knowledge_f16_workspace_bytes(None, 1, 4) == 0 and lib.keds_knowledge_f16_workspace_bytes(C.byref(kp), 0, 4) == 0
    assert lib.keds_knowledge_f16_workspace_bytes(C.byref(kp), 3, 16) == lib.keds_knowledge_workspace_bytes(C.byref(kp), 3, 16) > 0
    # the GEMM refusals of the new ids: the head buffer of id 34, and the ids between the tables
    gemm = lambda epi, aux=None, aux_i=0: lib.keds_gemm_bt(A, A, A, A, 128, 128, 64, epi, aux, aux_i, None)   # noqa: E731
    _refused(gemm(34), "EPI_BIAS_F16_H_HEADF32", "head buffer")
    _refused(gemm(34, A, -1), "EPI_BIAS_F16_H_HEADF32", "head buffer")
    for epi in (23, 31, 35, 100):
        _refused(gemm(epi), "unknown epilogue")


SHAPES = [(M, N, K) for M in (1, 127, 128, 129, 257) for N in (128, 384) for K in (64, 192, 768)] + \
         [(4224, 768, 768), (2048, 3072, 768), (4224, 1536, 768), (32768, 1024, 1024), (256, 256, 128), (128, 128, 2048), (128, 128, 4096)]


@pytest.mark.parametrize("epi", (32, 33, 34))
def test_the_plan_keeps_the_new_ids_on_the_128_forms(epi):
    """whatever the shape, the device, the split-K scratch or the LDS wish: KEDS_GEMM_FORM_SMALL with no remainder launch -- also where
    the same shape sends KEDS_EPI_BIAS_F32_H (same operands) to a 256 x 256 kernel; a split-K plan only where the scratch allows it"""
    lib = _lib.load()
    info, other = (C.c_int * 8)(), (C.c_int * 8)()
    big_elsewhere = 0
    for M, N, K in SHAPES:
        for cus in (0, 64, 256, 304):
            for scratch in (0, 8 << 20):
                for small_lds in (0, 1):
                    assert lib.keds_gemm_plan_query(epi, M, N, K, K, N, cus, scratch, small_lds, info) == 0, _lib.last_error()
                    form, tail, ring, _, splits, tail_splits, persistent, flags = list(info)
                    assert form == _lib.GEMM_FORM_SMALL and tail == _lib.GEMM_FORM_NONE and ring in (2, 4), (M, N, K, list(info))
                    assert persistent == 0 and flags == 0 and tail_splits == 0 and splits >= 1
                    assert splits == 1 or (scratch and K >= 2048), (M, N, K, list(info))
                    assert lib.keds_gemm_plan_query(_lib.EPI_BIAS_F32_H, M, N, K, K, N, cus, scratch, small_lds, other) == 0
                    big_elsewhere += other[0] != _lib.GEMM_FORM_SMALL
    assert big_elsewhere > 0                                                       # (the comparison above is not vacuous)
    assert lib.keds_gemm_plan_query(epi, 128, 128, 4096, 4096, 128, 256, 8 << 20, 0, info) == 0 and info[4] > 1
    for bad in (23, 24, 31, 35, 99, 100, -1):
        assert lib.keds_gemm_plan_query(bad, 128, 128, 64, 64, 128, 256, 0, 0, info) == -1
        assert "unknown epilogue" in _lib.last_error()
    assert lib.keds_gemm_plan_query(23, 4224, 768, 768, 768, 768, 256, 0, 0, info) == -1        # (what test_host_gemm_plan pins)


if __name__ == "__main__":                                                              # python -m tests.test_host_knowledge_f16: rewrite the lock
    rows = _table()
    with open(LOCK, "w") as out:
        out.write("{\n" + ",\n".join(f" {json.dumps(n)}: {json.dumps(rows[n])}" for n in sorted(rows)) + "\n}\n")
    print(f"{LOCK}: {len(rows)} functions", file=sys.stderr)
