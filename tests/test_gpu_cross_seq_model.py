"""CrossFormer.forward on sequences (keds_crossformer_forward_seq behind it): any number of queries over up to 288 keys against the
oracle's crossformer at the project's class ceiling for knowledge-module outputs (tests/gpu_util.CLASS_LIMITS: cosine >= 0.99994,
rel-L2 <= 1.3e-2), against the reference-minted fixture tests/golden/crossformer_seq.npz, and the late fusion of
eval_utils.py:244-254 end to end on the tiny model.  One query over at most 32 keys stays the single-query call, to the bit.

A float32 emulation of the chain on exactly the cases below (bf16 inputs, weights, projections, probabilities and layer outputs) lies
at rel-L2 1.6-2.3e-3 and 1 - cosine 1.4-2.9e-6 from the oracle: the ceiling has about 6x room and is not a number to loosen."""
import ctypes as C

import numpy as np
import pytest
import torch

import keds_amd
from keds_amd import _lib
from oracle import keds_oracle as O
from tests.conftest import golden_path
from tests.gpu_util import assert_parity
from tests.test_gpu_model import TINY

pytestmark = pytest.mark.gpu

SHAPES = ((4, 1, 33), (4, 1, 77), (4, 1, 128), (3, 5, 77), (2, 77, 257), (2, 257, 77), (2, 257, 288))


def _xf(dim):
    sd = O.synth_crossformer_state_dict(dim, 3, seed=5)
    xf = keds_amd.CrossFormer(dim, dim, dim, num_layers=3).eval()
    xf.load_state_dict(sd)
    return sd, xf.cuda()


@pytest.fixture(scope="module", params=(128, 768))
def module(request):
    return (request.param,) + _xf(request.param)


def _inputs(dim, B, Lq, Lk):
    q = O.synth_database(B * Lq, dim, seed=100 + Lq).reshape(B, Lq, dim)
    k = O.synth_database(B * Lk, dim, seed=200 + Lk).reshape(B, Lk, dim)
    v = O.synth_database(B * Lk, dim, seed=300 + Lk).reshape(B, Lk, dim)
    return q, k, v


@pytest.mark.parametrize("B,Lq,Lk", SHAPES)
def test_crossformer_sequences_match_the_oracle(module, B, Lq, Lk):
    dim, sd, xf = module
    q, k, v = _inputs(dim, B, Lq, Lk)
    got = xf(q.cuda(), k.cuda(), v.cuda())
    assert got.shape == (B, Lq, dim) and got.dtype == torch.float32
    assert_parity(f"crossformer_seq.d{dim}.B{B}.Lq{Lq}.Lk{Lk}", got, O.crossformer(sd, q, k, v))
    if (B, Lq, Lk) in ((4, 1, 77), (3, 5, 77)):                      # k passed as v: the aliasing path
        kd = k.cuda()
        assert_parity(f"crossformer_seq.d{dim}.B{B}.Lq{Lq}.Lk{Lk}.v_is_k", xf(q.cuda(), kd, kd), O.crossformer(sd, q, k, k))


@pytest.mark.parametrize("K", (16, 32))
def test_one_query_over_at_most_32_keys_is_the_single_query_call_to_the_bit(module, K):
    dim, sd, xf = module
    B = 4
    q, k, v = (t.cuda() for t in _inputs(dim, B, 1, K))
    lib = _lib.load()
    p = xf.params()
    for vv in (k, v):
        got = xf(q, k, vv)
        ws = torch.zeros(int(lib.keds_crossformer_workspace_bytes(C.byref(p), B, K)) + 256, dtype=torch.uint8, device="cuda")
        want = torch.empty((B, dim), dtype=torch.float32, device="cuda")
        _lib.check(lib.keds_crossformer_forward(C.byref(p), _lib.ptr(q.reshape(B, dim).contiguous()), _lib.ptr(k), _lib.ptr(vv), B, K,
                                                _lib.ptr(want), _lib.ptr(ws), ws.numel(), _lib.stream()), "keds_crossformer_forward")
        assert got.shape == (B, 1, dim) and torch.equal(got.reshape(B, dim), want)


def test_more_than_288_keys_raise_value_error(module):
    dim, sd, xf = module
    q, k, _ = _inputs(dim, 2, 1, 289)
    with pytest.raises(ValueError, match="288"):
        xf(q.cuda(), k.cuda(), k.cuda())


def test_half_precision_inputs_return_half(module):
    dim, sd, xf = module
    q, k, v = _inputs(dim, 3, 5, 77)
    for dt in (torch.float16, torch.bfloat16):
        got = xf(q.cuda().to(dt), k.cuda().to(dt), v.cuda().to(dt))
        assert got.dtype == dt and got.shape == (3, 5, dim)
        want = O.crossformer(sd, q.to(dt).float(), k.to(dt).float(), v.to(dt).float())
        assert_parity(f"crossformer_seq.d{dim}.{str(dt).split('.')[-1]}_inputs", got.float(), want.to(dt).float())


def test_reference_fixture():
    g = dict(np.load(golden_path("crossformer_seq.npz")))
    sd, xf = _xf(128)
    t = {k: torch.from_numpy(v).cuda() for k, v in g.items() if v.ndim >= 2}
    for name, q, k, v in (("out_1_77", "q1", "k77", "k77"), ("out_5_77", "q5", "k77", "v77"), ("out_17_257", "q17", "k257", "k257")):
        assert_parity(f"crossformer_seq.golden.{name}", xf(t[q], t[k], t[v]), g[name])
    assert_parity("crossformer_seq.golden.late_inputs", xf(t["late_q"].unsqueeze(1), t["late_k"], t["late_k"]), g["late_out"])


def test_late_fusion_end_to_end_on_the_tiny_model():
    """eval_utils.py:244-254 as written: the image feature as the one query over the 77 text tokens"""
    g = dict(np.load(golden_path("crossformer_seq.npz")))
    gt = dict(np.load(golden_path("clip_tiny.npz")))
    sd_clip = O.synth_clip_state_dict(**TINY, seed=7)
    m = keds_amd.build_model({k: v for k, v in sd_clip.items()}, fp16=False).cuda()
    sd, xf = _xf(128)
    img, text = torch.from_numpy(gt["image"][:2]).cuda(), torch.from_numpy(gt["text"][:2]).cuda()
    tokens = m.get_text_tokens(text)[0]
    got = xf(m.encode_image(img).unsqueeze(1), tokens, tokens)
    assert got.shape == (2, 1, 128)
    assert_parity("crossformer_seq.late_fusion.tiny", got, g["late_out"])
