"""No GPU: the host side of keds_block_pack (include/keds_hip.h), the one weight-packing routine behind the torch facade's
_pack_tower and the handle ABI's load_blocks -- the buffer size of every mode and the argument rules."""
import itertools
import os
import re

import pytest

from keds_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _up(n):
    return (n + 255) // 256 * 256


def _valid(width, fp8, f32, f16, folded):
    if fp8 and (f32 or not folded or width % 256):
        return False
    if f16 and (fp8 or f32 or not folded):
        return False
    return True


def _documented_bytes(lib, d, fp8, f32, f16, folded):
    """The arrays the header lists at keds_block_pack, each rounded up to 256 bytes."""
    gemms = [(3 * d, d), (d, d), (4 * d, d), (d, 4 * d)]                   # (N, K) of qkv, out, fc, proj
    total = 4 * _up(4 * d) + sum(_up(4 * n) for n, _ in gemms)              # LayerNorm vectors, biases (fp32)
    total += sum(_up((4 if f32 else 2) * n * k) for n, k in gemms)          # fp32 as stored / two fp16 planes; else 16-bit
    if folded and not f32:
        total += sum(_up(2 * n * k) + _up(8 * n) for n, k in (gemms[0], gemms[2]))
    if fp8:
        total += sum(_up(n * k) + _up(lib.keds_mxfp8_scale_bytes(n, k)) for n, k in gemms)
        total += _up(8 * 3 * d) + _up(8 * 4 * d) + _up(8 * d)               # qkv_bc8, fc_bc8, scratch of out-proj / c_proj
    return total


@pytest.mark.parametrize("width", [128, 256, 1024])
def test_block_pack_bytes_is_the_sum_of_the_documented_arrays(width):
    lib = _lib.load()
    seen = 0
    for fp8, f32, f16, folded in itertools.product((0, 1), (0, 1, 2), (0, 1), (0, 1)):
        got = lib.keds_block_pack_bytes(width, fp8, f32, f16, folded)
        if _valid(width, fp8, f32, f16, folded):
            assert got == _documented_bytes(lib, width, fp8, f32, f16, folded), (width, fp8, f32, f16, folded)
            seen += 1
        else:
            assert got == 0, (width, fp8, f32, f16, folded)
    # bf16 folded / unfolded, fp32 and fp32x3 (folded ignored: 2 each), fp16, and fp8 from width 256 on
    assert seen == (8 if width % 256 == 0 else 7)


def test_block_pack_bytes_is_zero_with_a_message_for_each_invalid_combination():
    lib = _lib.load()
    for args, word in (((128, 1, 0, 0, 1), "256"),            # fp8 at width 128
                       ((256, 1, 0, 0, 0), "folded"),         # fp8 unfolded
                       ((128, 0, 0, 1, 0), "folded"),         # f16 unfolded
                       ((128, 0, 1, 1, 1), "excludes"),       # f16 with f32
                       ((256, 1, 1, 0, 1), "excludes"),       # fp8 with f32
                       ((256, 1, 2, 0, 1), "excludes"),
                       ((192, 0, 0, 0, 1), "128")):           # width % 128
        assert lib.keds_block_pack_bytes(*args) == 0
        assert word in _lib.last_error(), (args, _lib.last_error())


def test_block_source_mirrors_the_header_and_only_the_packing_routine_calls_the_fold_primitives():
    hdr = open(os.path.join(ROOT, "include", "keds_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} keds_block_source;", hdr).group(1)
    assert re.findall(r"\*(\w+)", body) == [f[0] for f in _lib.BlockSource._fields_]
    for path in ("keds_amd/model.py", "keds_amd/csrc/session.hip"):
        src = open(os.path.join(ROOT, path)).read()
        for prim in ("keds_fold_layernorm_ex", "keds_fold_layernorm_mxfp8", "keds_split_f16_weight"):
            assert prim + "(" not in src, (path, prim)
        assert "keds_block_pack(" in src
