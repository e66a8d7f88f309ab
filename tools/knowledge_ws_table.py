#!/usr/bin/env python3
"""Every *_workspace_bytes function of the knowledge stream over a grid of shapes, as a table with its SHA-256: two builds of the library
size their workspaces alike exactly when the digests agree.  Pure host code, no GPU.

    python tools/knowledge_ws_table.py [path/to/libkeds_hip.so] [--table]
"""
import ctypes as C
import hashlib
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keds_amd import _lib  # noqa: E402

DIMS, HEADS, LAYERS, MIDDLES = (128, 512, 768), (2, 8, 12), (1, 2, 3, 8), (128, 512)
BS, KS, KS_F32 = (1, 3, 127, 128, 129, 1000), (1, 5, 16, 32), (1, 5, 16, 32, 64)
SEQ = ((1, 77), (77, 257), (257, 288), (600, 32))


def rows(lib):
    sz, i32 = C.c_size_t, C.c_int32
    for name, args in (("keds_im2text_workspace_bytes", [C.POINTER(_lib.Im2TextParams), i32]),
                       ("keds_crossformer_workspace_bytes", [C.POINTER(_lib.CrossFormerParams), i32, i32]),
                       ("keds_crossformer_seq_workspace_bytes", [C.POINTER(_lib.CrossFormerParams), i32, i32, i32]),
                       ("keds_knowledge_workspace_bytes", [C.POINTER(_lib.KnowledgeParams), i32, i32]),
                       ("keds_knowledge_f32_workspace_bytes", [C.POINTER(_lib.KnowledgeParams), i32, i32])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = sz, args
    fz = _lib.CrossFormerFused()
    for dim, middle, n_layer in itertools.product(DIMS, MIDDLES, (1, 2, 3, 4)):
        i2t = _lib.Im2TextParams(dim, middle, dim, n_layer)
        for r in BS + (1000 * 65,):
            yield f"im2text d{dim} m{middle} n{n_layer} rows{r}", lib.keds_im2text_workspace_bytes(C.byref(i2t), r)
    for dim, heads, layers in itertools.product(DIMS, HEADS, LAYERS):
        arr = (_lib.CrossLayerParams * layers)()
        for fused in (0, 1):
            xf = _lib.CrossFormerParams(dim, heads, layers, arr, C.pointer(fz) if fused else None)
            for B, K in itertools.product(BS, KS):
                yield f"crossformer d{dim} h{heads} l{layers} fused{fused} B{B} K{K}", lib.keds_crossformer_workspace_bytes(C.byref(xf), B, K)
            for B, (Lq, Lk) in itertools.product(BS, SEQ):
                yield (f"crossformer_seq d{dim} h{heads} l{layers} fused{fused} B{B} Lq{Lq} Lk{Lk}",
                       lib.keds_crossformer_seq_workspace_bytes(C.byref(xf), B, Lq, Lk))
            for middle in MIDDLES:
                kp = _lib.KnowledgeParams(_lib.Im2TextParams(dim, middle, dim, 2), xf, xf)
                for B, K in itertools.product(BS, KS_F32):
                    tag = f"d{dim} h{heads} l{layers} m{middle} fused{fused} B{B} K{K}"
                    if K <= 32:
                        yield "knowledge " + tag, lib.keds_knowledge_workspace_bytes(C.byref(kp), B, K)
                    yield "knowledge_f32 " + tag, lib.keds_knowledge_f32_workspace_bytes(C.byref(kp), B, K)


def main():
    paths = [a for a in sys.argv[1:] if not a.startswith("--")]
    lib = C.CDLL(paths[0] if paths else _lib.LIB_PATH)
    table = [f"{what} {nbytes}" for what, nbytes in rows(lib)]
    assert all(int(t.rsplit(" ", 1)[1]) > 0 for t in table)
    if "--table" in sys.argv:
        print("\n".join(table))
    print(f"{len(table)} rows, sha256 {hashlib.sha256(chr(10).join(table).encode()).hexdigest()}")


if __name__ == "__main__":
    main()
