"""No GPU: the "fp16" operating point's host side -- CLIP.set_precision("fp16") / KEDS_PRECISION=fp16, its exclusion of the
unfolded LayerNorm path (set_numerics("safe")), and the ABI-9 struct field keds_tower_params.f16."""
import ctypes as C
import os
import re

import pytest

import keds_amd
from keds_amd import _lib
from oracle import keds_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(embed_dim=128, image_resolution=56, vision_layers=2, vision_width=128, vision_patch_size=14,
            context_length=77, vocab_size=512, transformer_width=128, transformer_layers=2)


def _model():
    return keds_amd.build_model(O.synth_clip_state_dict(**TINY, seed=7), fp16=False)


def test_set_precision_fp16_sets_precision():
    m = _model()
    assert m.set_precision("fp16") is m
    assert m.precision == "fp16"
    m.set_precision("bf16")
    assert m.precision == "bf16"


def test_keds_precision_environment_selects_fp16(monkeypatch):
    monkeypatch.setenv("KEDS_PRECISION", "fp16")
    assert _model().precision == "fp16"


def test_fp16_and_safe_numerics_exclude_each_other_in_both_orders():
    m = _model().set_precision("fp16")
    with pytest.raises(ValueError):
        m.set_numerics("safe")
    assert m.numerics == "auto" and m.precision == "fp16"
    m = _model()
    m.set_numerics("safe")
    with pytest.raises(ValueError):
        m.set_precision("fp16")
    assert m.precision == "bf16" and m.numerics == "safe"
    m.set_numerics("fast").set_precision("fp16")          # the folded path without the guard is allowed
    assert m.precision == "fp16"


def test_tower_params_carry_the_f16_field_and_header_and_library_agree_on_abi_9():
    names = [f[0] for f in _lib.TowerParams._fields_]
    assert names[-1] == "f16" and names[-2] == "f32"
    assert _lib.TowerParams.f16.offset == _lib.TowerParams.f32.offset + C.sizeof(C.c_int)
    p = _lib.TowerParams(768, 12, 12, 77, 1, None, 0, 0, 0, 1)
    assert p.f16 == 1 and p.f32 == 0
    hdr = open(os.path.join(ROOT, "include", "keds_hip.h")).read()
    assert int(re.search(r"#define KEDS_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 15
    assert re.search(r"int f16;", hdr)
    for name, val in (("KEDS_EPI_LN_BIAS_F16_H", 16), ("KEDS_EPI_LN_QGELU_F16_H", 17), ("KEDS_EPI_RESID_STATS_F16_H", 18),
                      ("KEDS_EPI_BIAS_RESID_F32_H", 19), ("KEDS_EPI_BIAS_QGELU_F16_H", 20), ("KEDS_EPI_PATCH_F32_H", 21),
                      ("KEDS_EPI_BIAS_F32_H", 22)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == val == getattr(_lib, name[5:])
    lib = _lib.load()
    assert lib.keds_abi_version() == 15
    for sym in ("keds_attention_h", "keds_attention_packed_h", "keds_im2col_ex", "keds_layernorm_ex", "keds_cast_f16"):
        assert hasattr(lib, sym)


class _DoneEvent:
    def query(self):
        return True

    def synchronize(self):
        pass


def test_pending_guard_trip_is_settled_at_the_precision_its_pass_ran_at():
    """A lazily checked bf16 pass whose flag copy says "tripped" is settled by set_precision() BEFORE the switch: it counts as a
    bf16 trip (the fp32-stream flow), not as an fp16 range trip -- and a model on the fp32-stream flow refuses "fp16"."""
    import torch
    m = _model()
    m._guard = torch.zeros(1, dtype=torch.int32)
    m._guard_host = torch.ones(1, dtype=torch.int32)
    m._guard_event = _DoneEvent()
    with pytest.warns(RuntimeWarning):
        with pytest.raises(ValueError):
            m.set_precision("fp16")
    assert m.numerics_tripped and m.numerics_late_trip and m.precision == "bf16"
    assert getattr(m, "fp16_range_trips", 0) == 0 and m.numerics_sync()
    m.set_numerics("auto").set_precision("fp16")             # set_numerics resets the trip: the folded flow again
    assert m.precision == "fp16" and not m.numerics_sync()
