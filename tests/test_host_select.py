"""No GPU: the extension header include/keds_select.h (filtered search: a row selector and per-query exclusions) parses with the
project's parser, every function it declares is exported and bound, its table equals tests/golden/abi_select_v1.json, the refusals it
promises come back as KEDS_E_ARG with a message before anything is launched, and Selector.from_mask packs like a numpy model."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

from keds_amd import _abi, _lib
from keds_amd.index import Selector
from tests.conftest import ROOT, golden_path
from tests.test_host_abi import _lock_table

LOCK = golden_path("abi_select_v1.json")
HEADER = os.path.join(ROOT, "include", "keds_select.h")
FUNCTIONS = ["keds_sel_build", "keds_index_search_packed_sel", "keds_search_scan_sel", "keds_search_certify_sel", "keds_search_exact_sel"]
A = 0x7F0000001000                                                # a non-null address: every refusal comes before any access


def _table():
    classes = dict(_lib.STRUCTS)
    return _lock_table(classes, _lib.EXT_SIGNATURES)


def test_the_extension_header_parses_with_the_projects_parser():
    assert _abi.EXT_HEADERS == ("keds_select.h",)
    text = open(HEADER).read()
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.findall(r'#\s*include\s+(\S+)', bare) == ['"keds_hip.h"']           # the core header and nothing else
    ext = _lib.EXT_ABI
    assert list(ext.functions) == FUNCTIONS == re.findall(r"\b(keds_[a-z0-9_]+)\s*\(", bare)
    assert ext.constants == {"KEDS_SEL_MAX_EXCLUDE": 16} and ext.structs == {} and ext.handles == []
    assert _lib.SEL_MAX_EXCLUDE == 16
    # on its own, behind the core headers, through the public parse(): the same rows
    core = [(f"include/{h}", open(os.path.join(ROOT, "include", h)).read()) for h in _abi.HEADERS]
    whole = _abi.parse(core + [("include/keds_select.h", text)])
    assert {n: whole.functions[n] for n in FUNCTIONS} == ext.functions
    assert not set(FUNCTIONS) & set(_lib.ABI.functions)          # the core tables are what they were
    # the filtered entries are the unfiltered ones plus the new arguments in front of the stream
    f, T = {**_lib.ABI.functions, **ext.functions}, _abi.Type
    sel, ex, ne = T("uint32_t", 1), T("int64_t", 1), T("int")
    for new, old, added in (("keds_index_search_packed_sel", "keds_index_search_packed_ex", [sel, ex, ne]),
                            ("keds_search_scan_sel", "keds_search_scan", [sel]),
                            ("keds_search_certify_sel", "keds_search_certify", [ex, ne]),
                            ("keds_search_exact_sel", "keds_search_exact", [sel, ex, ne])):
        assert f[new][0] == f[old][0] and f[new][1] == f[old][1][:-1] + added + f[old][1][-1:], new


def test_a_declaration_outside_the_vocabulary_fails_in_the_extension_header_too():
    core = [(f"include/{h}", open(os.path.join(ROOT, "include", h)).read()) for h in _abi.HEADERS]
    text = open(HEADER).read()
    assert text.count("int n_exclude, void* stream);") == 3
    with pytest.raises(_abi.HeaderError, match=r"include/keds_select\.h:\d+: unknown type token 'long'"):
        _abi.parse(core + [("include/keds_select.h", text.replace("int drop, void* stream);", "long drop, void* stream);"))])
    with pytest.raises(_abi.HeaderError, match=r"include/keds_select\.h:\d+: keds_search_scan: declared twice"):
        _abi.parse(core + [("include/keds_select.h", text.replace("int keds_search_scan_sel(", "int keds_search_scan("))])


def test_every_declared_function_is_exported_and_bound():
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in FUNCTIONS:
        assert hasattr(raw, name), f"{name} is not exported"
        res, args = _lib.EXT_SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.restype is res is C.c_int and list(fn.argtypes) == args and len(args) == len(_lib.EXT_ABI.functions[name][1])


def test_function_table_equals_the_lock():
    """python -m tests.test_host_select rewrites the lock; its diff is then the change of the extension's ABI"""
    with open(LOCK) as f:
        lock = json.load(f)
    table = _table()
    assert sorted(table) == sorted(lock) == sorted(FUNCTIONS)
    assert {n: table[n] for n in table if table[n] != lock[n]} == {}
    assert lock["keds_sel_build"] == ["int32", ["pointer", "int64", "pointer", "int64", "int64", "int32", "pointer"]]


def _refused(rc_, *words):
    msg = _lib.last_error()
    assert rc_ == _lib.E_ARG, (rc_, msg)
    assert all(w in msg for w in words), msg


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    search = lambda sel, ex, ne: lib.keds_index_search_packed_sel(A, A, 100, 128, 0, A, 4, 0, 1, 0, A, A, None, A, 1 << 30, None, sel, ex, ne, None)
    certify = lambda ex, ne: lib.keds_search_certify_sel(A, 100, 128, A, A, 4, 64, 0, 1, 0, A, A, A, A, A, A, A, A, None, 0, ex, ne, None)
    exact = lambda ex, ne: lib.keds_search_exact_sel(A, 100, 128, 0, A, A, A, A, 2048, 1, 0, A, A, A, A, None, ex, ne, None)
    for name, call in (("keds_index_search_packed_sel", lambda ex, ne: search(None, ex, ne)), ("keds_search_certify_sel", certify),
                       ("keds_search_exact_sel", exact)):
        for ne in (-1, 17, 1 << 20):
            _refused(call(A, ne), name, "n_exclude", "[0,16]")
        for ne in (1, 16):
            _refused(call(None, ne), name, "exclude is null")
    _refused(lib.keds_sel_build(A, 100, A, -1, 0, 0, None), "keds_sel_build", "count")
    _refused(lib.keds_sel_build(A, 100, None, 1, 0, 0, None), "keds_sel_build", "ids is null")
    _refused(lib.keds_sel_build(A, 100, None, 5, 7, 1, None), "keds_sel_build", "ids is null")
    _refused(lib.keds_sel_build(None, 100, None, 0, 0, 0, None), "keds_sel_build", "null selector")
    _refused(lib.keds_sel_build(A, 0, None, 0, 0, 0, None), "keds_sel_build", "n must be")


def _model_words(mask):
    """bit (r & 31) of word (r >> 5), least significant first; the bits behind n are zero"""
    n = len(mask)
    words = np.zeros((n + 31) // 32, np.uint64)
    for r in np.nonzero(mask)[0]:
        words[r >> 5] |= np.uint64(1) << np.uint64(r & 31)
    return words.astype(np.uint32)


@pytest.mark.parametrize("n", (1, 31, 32, 33, 1000))
def test_from_mask_matches_the_numpy_model(n):
    rs = np.random.RandomState(n)
    for mask in (np.ones(n, bool), np.zeros(n, bool), rs.rand(n) < 0.5, rs.rand(n) < 0.02, np.arange(n) == n - 1, np.arange(n) == 0):
        s = Selector.from_mask(mask)
        got = s.words.numpy().view(np.uint32)
        assert s.n == n and s.words.dtype.is_signed and got.shape == ((n + 31) // 32,)
        assert np.array_equal(got, _model_words(mask))
        tail = n % 32
        assert tail == 0 or int(got[-1]) >> tail == 0            # the ignored tail bits come out zero
        assert np.array_equal(s.to_mask(), mask) and s.count() == int(mask.sum())
        # tail bits that ARE set are ignored by to_mask / count
        if tail:
            dirty = s.words.clone()
            dirty[-1] |= -(1 << tail)
            d = Selector(n, dirty)
            assert np.array_equal(d.to_mask(), mask) and d.count() == int(mask.sum())
    import torch
    assert np.array_equal(Selector.from_mask(torch.from_numpy(mask)).words.numpy(), Selector.from_mask(mask).words.numpy())


def test_shard_is_a_view_of_whole_words():
    from keds_amd.index import shard_bounds
    n = 1000 + 13
    mask = np.random.RandomState(3).rand(n) < 0.3
    s = Selector.from_mask(mask)
    seen = 0
    for rank in range(3):
        lo, hi = shard_bounds(n, 3, rank)
        part = s.shard(lo, hi)
        assert part.n == hi - lo and part.words.data_ptr() == s.words.data_ptr() + 4 * (lo // 32)
        assert np.array_equal(part.to_mask(), mask[lo:hi])
        seen += part.count()
    assert seen == int(mask.sum())
    for lo, hi in ((1, 64), (0, n + 1), (64, 64), (-32, 32)):
        with pytest.raises(ValueError):
            s.shard(lo, hi)
    with pytest.raises(ValueError):
        Selector(33, s.words[:1])


if __name__ == "__main__":                                                              # python -m tests.test_host_select: rewrite the lock
    rows = _table()
    with open(LOCK, "w") as out:
        out.write("{\n" + ",\n".join(f" {json.dumps(n)}: {json.dumps(rows[n])}" for n in sorted(rows)) + "\n}\n")
    print(f"{LOCK}: {len(rows)} functions", file=sys.stderr)
