"""ctypes binding of libkeds_hip.so (the C ABI declared in include/keds_hip.h and include/keds_session.h).

Signatures, parameter structs and constants are not written here: _abi.py parses them out of the two headers at import, so the
headers are the one place the ABI is edited.  Extension headers (_abi.EXT_HEADERS: include/keds_select.h) are parsed the same way
into a second table, EXT_SIGNATURES, and bound into the same CDLL; include/keds_knowledge_f16.h (_abi.KNOWLEDGE_F16_HEADERS) likewise
into a third, KF16_SIGNATURES.

There is no CPU fallback anywhere in this package: if the shared library is missing
or a call fails, a RuntimeError is raised.  Torch is used only for device memory,
streams and torch.distributed.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

import torch

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libkeds_hip.so")

# ---- the ABI, derived from the headers (keds_amd/_abi.py) ---------------------------------------------------------------------
vp, i32, i64, f32, sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t

# Python class name of every parameter struct (a typedef without a row keeps its C name).  Members, their order and their types are
# the header's, so positional construction follows the header.
CLASS_NAMES = {"keds_block_params": "BlockParams", "keds_block_source": "BlockSource", "keds_tower_params": "TowerParams",
               "keds_vit_params": "VitParams", "keds_text_params": "TextParams", "keds_pass_shape": "PassShape",
               "keds_cross_layer_params": "CrossLayerParams", "keds_im2text_params": "Im2TextParams",
               "keds_crossformer_fused": "CrossFormerFused", "keds_crossformer_params": "CrossFormerParams",
               "keds_knowledge_params": "KnowledgeParams", "keds_tensor": "Tensor"}

ABI = _abi.parse_headers()
# STRUCTS: typedef name -> ctypes.Structure;  SIGNATURES: function name -> (restype, argtypes), every prototype of the two headers
STRUCTS, SIGNATURES = _abi.bind(ABI, CLASS_NAMES)
_derived = {cls.__name__: cls for cls in STRUCTS.values()}                                   # _lib.BlockParams, _lib.Tensor, ...
_derived.update((name[len("KEDS_"):], value) for name, value in ABI.constants.items())      # _lib.EPI_BIAS_BF16, _lib.ABI_VERSION, ...
assert not set(_derived) & set(globals()), sorted(set(_derived) & set(globals()))
globals().update(_derived)
# the extension headers (_abi.EXT_HEADERS: keds_select.h) in a second table, bound into the same CDLL by load()
EXT_ABI = _abi.parse_ext_headers()
EXT_SIGNATURES = _abi.bind(_abi.Abi({**ABI.constants, **EXT_ABI.constants}, {**ABI.structs, **EXT_ABI.structs}, EXT_ABI.functions,
                                    ABI.handles + EXT_ABI.handles), CLASS_NAMES)[1]
_derived = {name[len("KEDS_"):]: value for name, value in EXT_ABI.constants.items()}        # _lib.SEL_MAX_EXCLUDE
assert not set(_derived) & set(globals()), sorted(set(_derived) & set(globals()))
globals().update(_derived)
# the knowledge stream in fp16 (_abi.KNOWLEDGE_F16_HEADERS: keds_knowledge_f16.h) in a third table
KF16_ABI = _abi.parse_ext_headers(_abi.KNOWLEDGE_F16_HEADERS)
KF16_SIGNATURES = _abi.bind(_abi.Abi({**ABI.constants, **KF16_ABI.constants}, {**ABI.structs, **KF16_ABI.structs}, KF16_ABI.functions,
                                     ABI.handles + KF16_ABI.handles), CLASS_NAMES, classes=STRUCTS)[1]    # (its entries take the core's structs)
_derived = {name[len("KEDS_"):]: value for name, value in KF16_ABI.constants.items()}       # _lib.EPI_BIAS_F16_H, ...
assert not set(_derived) & set(globals()), sorted(set(_derived) & set(globals()))
globals().update(_derived)
DT_F32, DT_BF16, DT_F16, DT_FP8, DT_F32X3 = (ABI.constants["KEDS_" + k] for k in ("F32", "BF16", "F16", "FP8", "F32X3"))    # keds_dtype

_lib: Optional[C.CDLL] = None


def build(verbose: bool = False) -> str:
    """Compile libkeds_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building libkeds_hip.so failed:\n" + res.stdout[-4000:] + res.stderr[-4000:])
    if verbose:
        print(res.stdout[-2000:])
    return LIB_PATH


def load() -> C.CDLL:
    """Load the HIP library.  Raises RuntimeError if it is missing (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(or `make -C keds_amd/csrc`).  keds_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(SIGNATURES.items()) + list(EXT_SIGNATURES.items()) + list(KF16_SIGNATURES.items()):
        fn = getattr(lib, name)          # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    got = lib.keds_abi_version()
    if got != ABI_VERSION:
        raise RuntimeError(f"libkeds_hip.so ABI {got} != expected {ABI_VERSION}")
    _lib = lib
    return lib


def source_digest() -> str:
    """First 16 hex digits of the SHA-256 over the kernel sources (csrc/*.hip, *.h, *.cpp, Makefile and include/*.h, in name
    order).  Measurement files under profiles/ carry the digest of the sources they were taken on; bench.py quotes a
    committed PMC / parity number only while this digest still matches (no .git travels to the GPU box)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = []
    for pat in ("csrc/*.hip", "csrc/*.h", "csrc/*.cpp", "csrc/Makefile"):
        files += glob.glob(os.path.join(_HERE, pat))
    files += glob.glob(os.path.join(os.path.dirname(_HERE), "include", "*.h"))
    for f in sorted(files, key=lambda x: os.path.relpath(x, os.path.dirname(_HERE))):
        h.update(os.path.relpath(f, os.path.dirname(_HERE)).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    # a variant build (make EXTRA="-D...": A/B and timing-only scripts) is a different build of the same sources
    try:
        extra = (load().keds_build_flags() or b"").decode().strip()
    except Exception:                                                 # noqa: BLE001  (no library: the sources alone)
        extra = ""
    if extra:
        h.update(b"EXTRA " + extra.encode())
    return h.hexdigest()[:16]


def build_flags() -> str:
    """The EXTRA flags the loaded library was built with ("" for the product build; "-DKEDS_ST_LN=1 ..." for an A/B variant)."""
    return (load().keds_build_flags() or b"").decode().strip()


def last_error() -> str:
    return (load().keds_last_error() or b"").decode()


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {last_error()}")


def require_gpu() -> None:
    if not torch.cuda.is_available():
        raise RuntimeError("keds_amd needs an MI355X (ROCm device); there is no CPU fallback")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device pointer of a contiguous CUDA tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("keds_amd: tensor is not on the GPU")
    if not t.is_contiguous():
        raise RuntimeError("keds_amd: tensor must be contiguous")
    return t.data_ptr()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class Workspace:
    """Grow-only device scratch buffer (one per owner object)."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None

    def get(self, nbytes: int, device) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != torch.device(device):
            self.buf = torch.zeros(int(nbytes) + 256, dtype=torch.uint8, device=device)
        return self.buf


_gemm_ws = {}


def ensure_gemm_workspace(device=None) -> None:
    """Register an 8 MiB split-K scratch buffer for `device` (idempotent; one registration per device).  Only direct
    `ops.gemm_bt` calls use it (one stream at a time per device): towers and handles split K into their own workspace."""
    require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _gemm_ws:
        buf = torch.empty(8 << 20, dtype=torch.uint8, device=dev)
        _gemm_ws[key] = buf
        with torch.cuda.device(key):
            check(load().keds_gemm_set_workspace(buf.data_ptr(), buf.numel()), "keds_gemm_set_workspace")


def prof_enable(on, classes=None) -> None:
    """on: False/True, or pass `classes` (iterable of PROF_* ids) to record only those kernel classes."""
    code = 0
    if classes is not None:
        for k in classes:
            code |= 1 << (k + 1)
    elif on:
        code = 1
    check(load().keds_prof_enable(code), "keds_prof_enable")


def prof_reset() -> None:
    check(load().keds_prof_reset(), "keds_prof_reset")


def prof_read_work(klass: int) -> float:
    """Algorithmic flops (PROF_GEMM) / scan-image bytes (PROF_SCAN) of the launches that carried event pairs."""
    u = C.c_double(0)
    check(load().keds_prof_read_work(klass, C.byref(u)), "keds_prof_read_work")
    return u.value


def prof_read(klass: int):
    ms, n = C.c_double(0), i64(0)
    check(load().keds_prof_read(klass, C.byref(ms), C.byref(n)), "keds_prof_read")
    return ms.value, n.value
