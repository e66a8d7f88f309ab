"""No GPU: the Python binding is what include/keds_hip.h and include/keds_session.h declare (keds_amd/_abi.py parses them,
keds_amd/_lib.py binds the library from the result).  Four statements are held against each other: the parser's tables, independent
regexes over the header text (nothing skipped), the host C compiler's sizeof / offsetof / values (layouts and constants), and
tests/golden/abi_v15.json, minted from the hand-written table this binding replaced (argument widths)."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

from keds_amd import _abi, _lib
from tests.conftest import ROOT, golden_path

SOURCES = [(f"include/{h}", open(os.path.join(ROOT, "include", h)).read()) for h in _abi.HEADERS]
BARE = "\n".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S) for _, text in SOURCES)        # the headers without their comments
LOCK = golden_path(f"abi_v{_lib.ABI_VERSION}.json")


def _mutated(old, new):
    """the parse of the headers with `old` replaced by `new` once, in the text only"""
    assert sum(text.count(old) for _, text in SOURCES) == 1, old
    return _abi.parse([(label, text.replace(old, new)) for label, text in SOURCES])


# ---- nothing skipped -----------------------------------------------------------------------------------------------------------------
def test_every_declaration_of_the_headers_is_in_the_tables():
    abi = _lib.ABI
    assert sorted(abi.functions) == sorted(set(re.findall(r"\b(keds_[a-z0-9_]+)\s*\(", BARE))) and len(abi.functions) >= 178
    assert list(abi.structs) == re.findall(r"typedef\s+struct\s*\{[^}]*\}\s*(\w+)\s*;", BARE) and len(abi.structs) >= 12
    assert abi.handles == re.findall(r"typedef\s+struct\s+(\w+)\s+\w+\s*;", BARE)
    defines = re.findall(r"#define[ \t]+(KEDS_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", BARE, flags=re.M)
    assert len(defines) == len(re.findall(r"#define[ \t]+KEDS_\w+[ \t]+\S", BARE)) >= 112        # every define with a value is an integer
    enumerators = [e.split("=")[0].strip() for body in re.findall(r"enum\s*\{([^}]*)\}", BARE) for e in body.split(",")]
    assert len(enumerators) == 5 + 25
    assert sorted(abi.constants) == sorted([n for n, _ in defines] + enumerators)
    for name, value in defines:
        assert abi.constants[name] == int(value), name
    assert [abi.constants[k] for k in ("KEDS_TOWER_BUF_COUNT", "KEDS_PASS_BUF_COL", "KEDS_PASS_BUF_COUNT", "KEDS_F32X3")] == [18, 18, 23, 4]


def test_lib_exposes_every_constant_and_struct_under_its_python_name():
    assert _lib.SIGNATURES.keys() == _lib.ABI.functions.keys()
    for name, value in _lib.ABI.constants.items():
        assert getattr(_lib, name[len("KEDS_"):]) == value, name
    for typedef, cls in _lib.STRUCTS.items():
        assert getattr(_lib, _lib.CLASS_NAMES[typedef]) is cls and issubclass(cls, C.Structure)
        assert [f for f, _ in cls._fields_] == [m for m, _ in _lib.ABI.structs[typedef]]
    assert (_lib.DT_F32, _lib.DT_BF16, _lib.DT_F16, _lib.DT_FP8, _lib.DT_F32X3) == (0, 1, 2, 3, 4)
    assert _lib.ABI_VERSION == 15 and _lib.COMM_ID_BYTES == 128 and _lib.SCAN_MAX_K == 128 and _lib.E_WORKSPACE == -3
    t = _lib.TowerParams(512, 2, 8, 77, 1, None, 0, 1, 2, 0)                         # positional construction in header order
    assert (t.width, t.layers, t.heads, t.seq, t.causal, t.fp8, t.last_cls_only, t.f32, t.f16) == (512, 2, 8, 77, 1, 0, 1, 2, 0)


# ---- the C compiler as oracle for layouts and values ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{("S", struct): size, ("F", struct, member): (offset, size), ("K", constant): value} as the host C compiler sees the headers"""
    cc = os.environ.get("CC") or next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    assert cc, "no host C compiler ($CC, cc, gcc, clang): the layout check cannot run"
    abi, lines = _lib.ABI, []
    for s, members in abi.structs.items():
        lines.append(f'printf("S {s} %zu\\n", sizeof({s}));')
        lines += [f'printf("F {s} {m} %zu %zu\\n", offsetof({s}, {m}), sizeof((({s}*)0)->{m}));' for m, _ in members]
    lines += [f'printf("K {k} %lld\\n", (long long)({k}));' for k in abi.constants]
    d = tmp_path_factory.mktemp("abi")
    (d / "abi.c").write_text('#include <stdio.h>\n#include "keds_hip.h"\n#include "keds_session.h"\nint main(void) {\n'
                             + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run(cc.split() + ["-std=c99", "-I", os.path.join(ROOT, "include"), str(d / "abi.c"), "-o", str(d / "abi")], check=True)
    out = {}
    for row in subprocess.run([str(d / "abi")], check=True, capture_output=True, text=True).stdout.splitlines():
        kind, *rest = row.split()
        if kind == "F":
            out["F", rest[0], rest[1]] = (int(rest[2]), int(rest[3]))
        else:
            out[kind, rest[0]] = int(rest[1])
    assert len(out) == len(lines)
    return out


def _layout_mismatches(abi, compiled):
    """what ctypes and the parsed constants say against the compiler, item by item; [] when they agree everywhere"""
    classes, _ = _abi.bind(abi)
    got = {("K", k): v for k, v in abi.constants.items()}
    for s, cls in classes.items():
        got[("S", s)] = C.sizeof(cls)
        got.update({("F", s, m): (getattr(cls, m).offset, getattr(cls, m).size) for m, _ in cls._fields_})
    return [f"{key}: binding {got.get(key)}, compiler {compiled.get(key)}" for key in sorted(got.keys() | compiled.keys(), key=str)
            if got.get(key) != compiled.get(key)]


def test_layouts_and_constants_equal_the_c_compilers(compiled):
    assert len([k for k in compiled if k[0] == "S"]) == 12 and len([k for k in compiled if k[0] == "F"]) >= 117
    assert _layout_mismatches(_lib.ABI, compiled) == []
    assert compiled["S", "keds_block_params"] == 224 and compiled["F", "keds_block_params", "x3_exp"] == (208, 16)
    assert compiled["F", "keds_tower_params", "blocks"] == (24, 8) and compiled["F", "keds_tensor", "shape"] == (24, 32)


def test_swapped_struct_members_fail_the_compiler_comparison(compiled):
    bad = _layout_mismatches(_mutated("*qkv_w, *out_w, *fc_w, *proj_w;", "*out_w, *qkv_w, *fc_w, *proj_w;"), compiled)
    assert len(bad) == 2 and "qkv_w" in bad[1] and "out_w" in bad[0], bad
    bad = _layout_mismatches(_mutated("int fp8;  ", "int64_t fp8;  "), compiled)            # a widened member moves every later one
    assert any("keds_vit_params" in b for b in bad) and any("'fp8'" in b for b in bad), bad


# ---- the lock on the function table --------------------------------------------------------------------------------------------------
KINDS = {None: "void", C.c_int: "int32", C.c_int64: "int64", C.c_uint32: "uint32", C.c_uint64: "uint64", C.c_float: "float",
         C.c_double: "double", C.c_char_p: "char*", C.POINTER(C.c_char_p): "char**", C.c_void_p: "pointer"}


def _lock_table(classes, signatures):
    """name -> [return kind, [parameter kinds]] of the ctypes types the library is bound with (size_t is uint64 here)"""
    typedef = {cls: name for name, cls in classes.items()}

    def kind(ct):
        if ct in KINDS:
            return KINDS[ct]
        return "pointer" if issubclass(ct, C.c_void_p) else f"struct-pointer({typedef[ct._type_]})"

    return {name: [kind(res), [kind(a) for a in args]] for name, (res, args) in signatures.items()}


def test_function_table_equals_the_lock():
    """Every function's return kind and parameter kinds, as bound, equal tests/golden/abi_v<KEDS_ABI_VERSION>.json.  The file for ABI 15
    was minted from the last hand-written ctypes table, so this holds the derived widths to the ones every caller ran on.  When the ABI
    moves, rewrite it with

        python -m tests.test_host_abi

    (and drop the old version's file): the change of the table is then a diff to review."""
    with open(LOCK) as f:
        lock = json.load(f)
    table = _lock_table(_lib.STRUCTS, _lib.SIGNATURES)
    assert sorted(table) == sorted(lock)
    assert {n: table[n] for n in table if table[n] != lock[n]} == {}


def test_a_narrowed_stride_fails_the_lock():
    with open(LOCK) as f:
        lock = json.load(f)
    abi = _mutated("int keds_gemm_bt_ex(const void* A, int64_t lda,", "int keds_gemm_bt_ex(const void* A, int lda,")
    table = _lock_table(*_abi.bind(abi))
    assert [n for n in table if table[n] != lock[n]] == ["keds_gemm_bt_ex"]
    assert (table["keds_gemm_bt_ex"][1][1], lock["keds_gemm_bt_ex"][1][1]) == ("int32", "int64")


# ---- the parser fails loudly ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("old, new, message", [
    ("int keds_prof_enable(int on);", "int keds_prof_enable(long on);", r"include/keds_hip\.h:76: unknown type token 'long'"),
    ("int x3_exp[4];", "short x3_exp[4];", r"include/keds_hip\.h:529: unknown type token 'short'"),
    ("} keds_block_source;", "", r"include/keds_hip\.h:533: no complete declaration"),               # an unterminated struct
    ("} keds_tensor;", "", r"include/keds_session\.h:39: no complete declaration"),
    ("int keds_prof_reset(void);", "int keds_prof_reset(void)", r"include/keds_hip\.h:77: cannot classify"),
    ("int keds_prof_reset(void);", "int keds_prof_reset();", r"include/keds_hip\.h:77: keds_prof_reset: empty parameter"),
    ("int keds_prof_reset(void);", "static int one(void) { return 1; }", r"include/keds_hip\.h:77: cannot classify"),
    ("#define KEDS_PROF_NCLASS 5", "#define KEDS_PROF_NCLASS (KEDS_PROF_OTHER + 1)", r"include/keds_hip\.h:75: unknown preprocessor line"),
    ("#define KEDS_PROF_NCLASS 5", "#define KEDS_PROF_LN 5", r"include/keds_hip\.h:75: KEDS_PROF_LN defined twice"),
    ("#define KEDS_PROF_NCLASS 5", "#if 0", r"include/keds_hip\.h:75: unknown preprocessor line"),
    ("KEDS_PASS_BUF_COL = KEDS_TOWER_BUF_COUNT,", "KEDS_PASS_BUF_COL = KEDS_LATER,", r"include/keds_hip\.h:674: 'KEDS_LATER' is neither"),
    ("keds_tower_params tower;\n    int vocab", "keds_ctx tower;\n    int vocab", r"include/keds_hip\.h:592: unknown type token 'keds_ctx'"),
    ("int64_t shape[4];", "void shape[4];", r"include/keds_session\.h:44: void by value"),
    ("const char* name; ", "const char* name  ", r"include/keds_session\.h:40: cannot read a member of keds_tensor"),
])
def test_parser_raises_on_what_it_does_not_know(old, new, message):
    with pytest.raises(_abi.HeaderError, match=message):
        _mutated(old, new)


# ---- call sites ----------------------------------------------------------------------------------------------------------------------
def test_every_pointer_parameter_accepts_what_call_sites_pass():
    """Plain pointers (arrays, handles, out-parameters) take None, an address, a ctypes array and byref / pointer of an element; where the
    header names the element (int*, float*, size_t*, a handle out-parameter) a bare element goes by reference too, as it did under the
    hand-written POINTER(c_int) rows.  A pointer to a public struct takes None, an array of the struct, byref of one and -- by reference,
    automatically -- the struct itself; const char* takes bytes; const char* const* an array of them.  (ctypes' own struct and char
    pointers refuse a bare address, as the hand-written rows did.)"""
    abi, checked, bare = _lib.ABI, 0, 0
    for name, (_, params) in abi.functions.items():
        argtypes = _lib.SIGNATURES[name][1]
        assert len(argtypes) == len(params)
        for t, at in zip(params, argtypes):
            if t.ptr == 0:
                assert at is _abi.SCALARS[t.base]
                continue
            if t.ptr == 1 and t.base in _lib.STRUCTS:
                cls = _lib.STRUCTS[t.base]
                assert at is C.POINTER(cls)
                accepted = [None, (cls * 2)(), C.byref(cls()), cls()]
            elif t.base == "char":
                elem = C.c_char if t.ptr == 1 else C.c_char_p
                assert at is (C.c_char_p if t.ptr == 1 else C.POINTER(C.c_char_p))
                accepted = [None, (elem * 4)(), C.byref(elem())] + ([b"bpe.txt"] if t.ptr == 1 else [])
            else:
                typed = t.ptr == 2 or t.base in _abi.SCALARS                             # the header names what the pointer points to
                elem = _abi.SCALARS[t.base] if t.ptr == 1 and typed else C.c_void_p if typed or t.base in ("void", *abi.handles) else C.c_ubyte
                assert at is (_abi.pointer_to(elem) if typed else C.c_void_p) and issubclass(at, C.c_void_p)
                accepted = [None, 0x7F0000001000, (elem * 4)(), C.byref(elem()), C.pointer(elem()), C.c_void_p(0x1000)]
                if typed:
                    one = elem(7)
                    assert at.from_param(one)._obj is one                               # by reference, not by value
                    accepted.append(one)
                    bare += 1
            for value in accepted:
                at.from_param(value)                                                    # raises TypeError / ArgumentError if refused
            checked += 1
    assert checked >= 600 and bare >= 200


def test_a_bare_out_parameter_is_written_through():
    """keds_tower_plan_query's n_steps and workspace_bytes handed over without byref come back filled, as with byref"""
    lib, shape = _lib.load(), (_lib.TOWER_FLOW_BF16, 256, 4, 17, 0, 2, 4, _lib.TOWER_TAIL_ALL, 0, 0, 0, -1, -1)
    n, ws, n_ref, ws_ref = C.c_int(0), C.c_size_t(0), C.c_int(0), C.c_size_t(0)
    assert lib.keds_tower_plan_query(*shape, None, 0, C.byref(n_ref), None, C.byref(ws_ref)) == 0
    assert lib.keds_tower_plan_query(*shape, None, 0, n, None, ws) == 0
    assert (n.value, ws.value) == (n_ref.value, ws_ref.value) and n.value > 0 and ws.value > 0


if __name__ == "__main__":                                                              # python -m tests.test_host_abi: rewrite the lock
    rows = _lock_table(_lib.STRUCTS, _lib.SIGNATURES)
    with open(LOCK, "w") as out:
        out.write("{\n" + ",\n".join(f" {json.dumps(n)}: {json.dumps(rows[n])}" for n in sorted(rows)) + "\n}\n")
    print(f"{LOCK}: {len(rows)} functions", file=sys.stderr)
