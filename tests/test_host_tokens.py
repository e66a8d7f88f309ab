"""Token-level tower outputs without a GPU: the new entry points are declared, exported and bound, reject bad arguments
before touching a device, and the façade methods raise the library's "no CPU" error instead of NotImplementedError."""
import ctypes as C
import os

import pytest
import torch

import keds_amd
from keds_amd import _lib
from oracle import keds_oracle as O

NEW = ("keds_vit_run_tokens", "keds_text_run_tokens", "keds_tap_store_nt", "keds_vit_forward_tokens", "keds_text_forward_tokens")
TINY = dict(embed_dim=128, image_resolution=56, vision_layers=2, vision_width=128, vision_patch_size=14,
            context_length=77, vocab_size=512, transformer_width=128, transformer_layers=2)


def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_token_entry_points_are_declared_exported_and_bound():
    lib = _lib_loaded()
    for name in NEW:
        assert name in _lib.ABI.functions, f"{name} not declared in include/*.h"
        assert name in _lib.SIGNATURES, f"{name} missing from keds_amd._lib.SIGNATURES"
        assert hasattr(lib, name), f"{name} not exported"
    assert lib.keds_abi_version() == 15 == _lib.ABI_VERSION


def test_token_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib_loaded()
    vp, tp = _lib.VitParams(), _lib.TextParams()
    fake = C.c_void_p(0x1000)              # never dereferenced: the argument checks come first
    out = C.c_void_p(0x2000)

    def vit(B, out_, taps, toks, ot):
        return lib.keds_vit_run_tokens(C.byref(vp), fake, B, out_, 0, taps, toks, ot, fake, 1 << 20, None)

    assert vit(2, None, None, None, 1) == -1 and "no output requested" in _lib.last_error()
    assert vit(2, None, out, None, 3) == -1 and "out_type 3" in _lib.last_error()
    assert vit(0, out, out, None, 1) == -1 and "B = 0" in _lib.last_error()
    assert lib.keds_vit_run_tokens(None, fake, 2, out, 0, None, None, 1, fake, 1 << 20, None) == -1
    assert "bad argument" in _lib.last_error()
    assert lib.keds_text_run_tokens(C.byref(tp), fake, 2, None, 1, fake, 1 << 20, None) == -1
    assert "no output requested" in _lib.last_error()
    assert lib.keds_text_run_tokens(C.byref(tp), fake, 2, out, -1, fake, 1 << 20, None) == -1 and "out_type -1" in _lib.last_error()
    assert lib.keds_text_run_tokens(C.byref(tp), fake, -3, out, 1, fake, 1 << 20, None) == -1 and "B = -3" in _lib.last_error()
    assert lib.keds_vit_forward_tokens(None, fake, 0, 2, None, None, None, 1, None) == -1
    assert "no output requested" in _lib.last_error()
    assert lib.keds_vit_forward_tokens(None, fake, 0, 2, out, None, None, 1, None) == -1 and "bad argument" in _lib.last_error()
    assert lib.keds_text_forward_tokens(None, fake, 2, out, 7, None) == -1 and "out_type 7" in _lib.last_error()
    assert lib.keds_text_forward_tokens(None, fake, 2, out, 1, None) == -1 and "bad argument" in _lib.last_error()
    assert lib.keds_tap_store_nt(1) == 0


def test_token_methods_raise_the_no_cpu_error(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # (the same path on a GPU machine)
    m = keds_amd.build_model(dict(O.synth_clip_state_dict(**TINY, seed=7)), fp16=False)
    img = torch.zeros((1, 3, 56, 56))
    calls = (lambda: m.encode_image(img, mid_feature=True), lambda: m.visual(img), lambda: m.visual(img, mid_feature=True),
             lambda: m.visual.get_tokens(img), lambda: m.get_text_tokens(torch.zeros((1, 77), dtype=torch.long)))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_visual_reaches_its_model_without_a_state_dict_change():
    m = keds_amd.build_model(dict(O.synth_clip_state_dict(**TINY, seed=7)), fp16=False)
    assert m.visual._owner() is m
    assert not any("clip" in k for k in m.state_dict())
    assert not any("clip" in n for n, _ in m.named_modules())
    import copy
    import pickle
    c = copy.deepcopy(m)
    assert c.visual._owner() is c
    p = pickle.loads(pickle.dumps(m))
    assert p.visual._owner() is p
