"""The C ABI of libkeds_hip.so as its headers declare it: include/keds_hip.h and include/keds_session.h parsed into ordered tables of
constants, structs and functions, and those turned into ctypes Structures and (restype, argtypes) rows.  _lib.py binds the library
from them, so an ABI change is an edit of the header alone.  Pure Python, no compiler; the headers are read once per process.

The parser knows exactly the C subset the two headers are written in (see parse) and raises HeaderError, naming the header line, on
anything else: it never skips a declaration."""
from __future__ import annotations

import ctypes as C
import functools
import os
import re
from typing import NamedTuple, Optional

HEADERS = ("keds_hip.h", "keds_session.h")          # in include order: the second includes the first
# Extension headers: entry points added to the same library between two moves of KEDS_ABI_VERSION.  Each is written in the same C
# subset, includes "keds_hip.h" only, is parsed by the same parser on top of the core tables and has a lock of its own under
# tests/golden (keds_select.h: abi_select_v1.json); the next ABI version folds them into the core header.
EXT_HEADERS = ("keds_select.h",)
# ... and the knowledge stream in fp16, in a table and under a lock of its own (abi_knowledge_f16_v1.json): EXT_HEADERS and what
# parse_ext_headers() returns for it stay what the select lock describes
KNOWLEDGE_F16_HEADERS = ("keds_knowledge_f16.h",)
INCLUDE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
SCALARS = {"int": C.c_int, "int32_t": C.c_int, "uint32_t": C.c_uint32, "uint8_t": C.c_uint8, "int64_t": C.c_int64,
           "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
POINTEES = ("void", "char", "unsigned char")        # only ever behind a pointer (void also as a return type)

_INT = r"-?\s*(?:0[xX][0-9a-fA-F]+|\d+)"
_IGNORED = re.compile(r'#\s*(ifndef\s+KEDS_\w+_H|define\s+KEDS_\w+_H|endif|include\s+(<stddef\.h>|<stdint\.h>|"keds_hip\.h"))')
_DEFINE = re.compile(rf"#\s*define\s+(KEDS_\w+)\s+(?:\(\s*({_INT})\s*\)|({_INT}))")
_STATEMENT = re.compile(r"\s*([^;{}]*?(?:\{[^{}]*\}[^;{}]*?)?)\s*;")
_DECL = re.compile(r"\s*(?:const\s+)?(unsigned\s+char|\w+)((?:\s|\*|\bconst\b)*)(\w+)?\s*(?:\[\s*(\w*)\s*\])?\s*")
_ENUMERATOR = re.compile(rf"\s*(KEDS_\w+)\s*(?:=\s*({_INT}|KEDS_\w+))?\s*")


class HeaderError(ValueError):
    """A header holds something outside the parser's vocabulary; the message starts with header:line."""


class Type(NamedTuple):
    base: str                       # a key of SCALARS, one of POINTEES, or a typedef of the headers (public struct or opaque handle)
    ptr: int = 0                    # pointer depth (an array parameter counts as one)
    array: Optional[int] = None     # struct members only: element count


class Abi(NamedTuple):
    constants: dict                 # KEDS_* name -> int: every #define and every enumerator, in header order
    structs: dict                   # typedef name -> [(member, Type)], in header order
    functions: dict                 # keds_* name -> (return Type, [parameter Type])
    handles: list                   # the opaque `typedef struct keds_x keds_x;` names


def _parse_header(label, text, abi):
    consts = {}                     # this header's: name -> (offset, value)

    def fail(pos, msg):
        raise HeaderError(f"{label}:{text.count(chr(10), 0, pos) + 1}: {msg}")

    def blank(m):
        return re.sub(r"[^\n]", " ", m.group(0))

    def integer(tok, pos):
        if re.fullmatch(_INT, tok):
            return int(tok.replace(" ", ""), 0)
        if tok in consts or tok in abi.constants:
            return consts[tok][1] if tok in consts else abi.constants[tok]
        fail(pos, f"{tok!r} is neither an integer nor an earlier constant")

    def constant(name, value, pos):
        if name in consts or name in abi.constants:
            fail(pos, f"{name} defined twice")
        consts[name] = (pos, value)

    def decl(s, pos, where, param=False):
        """`[const] type [*...] [name] [[N]]` -> (Type, name)"""
        m = _DECL.fullmatch(s)
        if not m:
            fail(pos, f"cannot read {where} {' '.join(s.split())!r}")
        base, name, count = " ".join(m.group(1).split()), m.group(3), m.group(4)
        if base not in SCALARS and base not in POINTEES and base not in abi.structs and base not in abi.handles:
            fail(pos, f"unknown type token {base!r} in {where}")
        if count is not None and not (param or count):
            fail(pos, f"array {name} without a length in {where}")
        t = Type(base, m.group(2).count("*") + (param and count is not None), None if param or count is None else integer(count, pos))
        if t.ptr == 0 and (base in POINTEES or base in abi.handles) and where != "the return type":
            fail(pos, f"{base} by value in {where}")
        return t, name

    def pieces(m, group, sep, at):
        """the non-blank `sep`-separated pieces of a group of m, a match inside the statement at offset `at`: (text, its offset)"""
        for piece in re.finditer(f"[^{sep}]+", m.group(group)):
            if piece.group(0).strip():
                yield piece.group(0), at + m.start(group) + piece.start() + len(piece.group(0)) - len(piece.group(0).lstrip())

    text = re.sub(r"/\*.*?\*/", blank, text, flags=re.S)
    if "/*" in text:
        fail(text.index("/*"), "unterminated comment")
    text = re.sub(r"^#ifdef __cplusplus\n.*?^#endif$", blank, text, flags=re.S | re.M)         # extern "C" { and its }
    for m in re.finditer(r"^[ \t]*(#.*)$", text, flags=re.M):
        d = _DEFINE.fullmatch(m.group(1).strip())
        if d:
            constant(d.group(1), integer(d.group(2) or d.group(3), m.start()), m.start())
        elif not _IGNORED.fullmatch(m.group(1).strip()):
            fail(m.start(), f"unknown preprocessor line {m.group(1).strip()!r} (a constant is `#define KEDS_NAME <integer>`)")
    text = re.sub(r"^[ \t]*#.*$", blank, text, flags=re.M)

    pos = 0
    while text[pos:].strip():
        st = _STATEMENT.match(text, pos)
        if not st:
            fail(pos + len(text[pos:]) - len(text[pos:].lstrip()), "no complete declaration from here on (an unterminated struct, enum or prototype?)")
        s, at, pos = st.group(1), st.start(1), st.end()
        if m := re.fullmatch(r"typedef\s+struct\s*\{(.*)\}\s*(keds_\w+)", s, flags=re.S):
            members, where = [], f"a member of {m.group(2)}"
            if m.group(2) in abi.structs:
                fail(at, f"struct {m.group(2)} declared twice")
            for line, p in pieces(m, 1, ";", at):                       # `type a, *b, c[4]`: the declarators share the base type
                first, *rest = line.split(",")
                t0, name = decl(first, p, where)
                for t, name in [(t0, name)] + [decl(f"{t0.base} {r}", p, where) for r in rest]:
                    if not name or name in dict(members):
                        fail(p, f"{where} without a name, or {name} twice")
                    members.append((name, t))
            abi.structs[m.group(2)] = members
        elif m := re.fullmatch(r"typedef\s+struct\s+(keds_\w+)\s+\1", s):
            abi.handles.append(m.group(1))
        elif m := re.fullmatch(r"(?:typedef\s+)?enum\s*\{(.*)\}\s*(?:keds_\w+)?", s, flags=re.S):
            value = -1
            for item, p in pieces(m, 1, ",", at):
                e = _ENUMERATOR.fullmatch(item)
                if not e:
                    fail(p, f"cannot read enumerator {item.strip()!r}")
                value = value + 1 if e.group(2) is None else integer(e.group(2), p)
                constant(e.group(1), value, p)
        elif m := re.fullmatch(r"([^()]*?)\b(keds_\w+)\s*\(([^()]*)\)", s, flags=re.S):
            ret, junk = decl(m.group(1), at, "the return type")
            if junk or m.group(2) in abi.functions or not (ret == Type("void") or ret == Type("char", 1) or ret.ptr == 0 and ret.base in SCALARS):
                fail(at, f"{m.group(2)}: declared twice, or its return type is not void, const char* or a scalar")
            params = []
            if m.group(3).strip() != "void":
                params = [decl(item, p, f"a parameter of {m.group(2)}", param=True)[0] for item, p in pieces(m, 3, ",", at)]
                if len(params) != m.group(3).count(",") + 1:
                    fail(at, f"{m.group(2)}: empty parameter")
            abi.functions[m.group(2)] = (ret, params)
        else:
            fail(at, f"cannot classify declaration {' '.join(s.split())[:80]!r}")
    abi.constants.update((name, v) for name, (_, v) in sorted(consts.items(), key=lambda kv: kv[1][0]))


def parse(sources) -> Abi:
    """sources: (label, text) of each header in include order -> Abi.  The vocabulary, with /* comments */ anywhere:
      the include guard, #include of <stddef.h>, <stdint.h> or "keds_hip.h", #ifdef __cplusplus blocks (dropped);
      #define KEDS_X <integer | (integer) | (-integer)>;
      typedef struct { [const] type [*]a, [*]b[N]; ... } keds_x;   members: scalars, pointers, earlier public structs by value;
      typedef struct keds_x keds_x;                                an opaque handle: only pointers to it appear;
      [typedef] enum { KEDS_A [= integer | earlier constant], ... } [keds_x];
      type keds_name(parameters | void);                           over any number of lines; an array parameter is a pointer."""
    abi = Abi({}, {}, {}, [])
    for label, text in sources:
        _parse_header(label, text, abi)
    return abi


@functools.lru_cache(maxsize=None)
def parse_headers() -> Abi:
    """The two headers of this checkout, parsed once per process."""
    sources = []
    for h in HEADERS:
        with open(os.path.join(INCLUDE_DIR, h)) as f:
            sources.append((f"include/{h}", f.read()))
    return parse(sources)


@functools.lru_cache(maxsize=None)
def parse_ext_headers(headers=EXT_HEADERS) -> Abi:
    """What the extension headers `headers` (EXT_HEADERS, or another tuple such as KNOWLEDGE_F16_HEADERS) add to the core tables: an
    Abi holding only their constants, structs, functions and handles (their declarations may use every type and constant of the
    core headers; a name declared twice is a HeaderError)."""
    core = parse_headers()
    abi = Abi(dict(core.constants), dict(core.structs), dict(core.functions), list(core.handles))
    for h in headers:
        with open(os.path.join(INCLUDE_DIR, h)) as f:
            _parse_header(f"include/{h}", f.read(), abi)
    return Abi({k: v for k, v in abi.constants.items() if k not in core.constants},
               {k: v for k, v in abi.structs.items() if k not in core.structs},
               {k: v for k, v in abi.functions.items() if k not in core.functions},
               [h for h in abi.handles if h not in core.handles])


@functools.lru_cache(maxsize=None)
def pointer_to(elem):
    """The argtype of a `elem*` parameter: c_void_p -- None, an address, a ctypes array or pointer, byref(...) -- that, like
    POINTER(elem), also takes a bare `elem` instance by reference (an out-parameter handed over without byref)."""
    def from_param(cls, value):
        return C.byref(value) if type(value) is elem else C.c_void_p.from_param(value)
    return type(f"pointer_to_{elem.__name__}", (C.c_void_p,), {"from_param": classmethod(from_param)})


def _ctype(t: Type, classes, param=False):
    if t.ptr == 0:
        ct = classes[t.base] if t.base in classes else SCALARS[t.base]
    elif t.base == "char" and t.ptr <= 2:
        ct = C.c_char_p if t.ptr == 1 else C.POINTER(C.c_char_p)
    elif t.ptr == 1 and t.base in classes:
        ct = C.POINTER(classes[t.base])         # a Structure instance is then passed by reference
    elif param and (t.ptr == 2 or t.base in SCALARS):
        ct = pointer_to(SCALARS[t.base] if t.ptr == 1 else C.c_void_p)      # arrays, out-parameters, handle out-parameters
    else:
        ct = C.c_void_p                         # untyped arrays, handles, every pointer member
    return ct * t.array if t.array else ct


def bind(abi: Abi, class_names=None, classes=None):
    """-> (classes: typedef name -> ctypes.Structure subclass with the header's members in the header's order,
           signatures: function name -> (restype, argtypes)).  class_names: typedef name -> Python class name (default: the typedef).
    classes: Structure classes an earlier bind() made, kept for their typedefs (an extension's functions then take the very structs
    the core table is bound with)."""
    classes = dict(classes or {})
    for typedef, members in abi.structs.items():
        if typedef in classes:
            continue
        classes[typedef] = type((class_names or {}).get(typedef, typedef), (C.Structure,),
                                {"_fields_": [(m, _ctype(t, classes)) for m, t in members], "__doc__": f"{typedef} of include/*.h"})
    signatures = {name: (None if ret == Type("void") else _ctype(ret, classes), [_ctype(p, classes, param=True) for p in params])
                  for name, (ret, params) in abi.functions.items()}
    return classes, signatures
