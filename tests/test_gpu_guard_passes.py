"""The numerics guard at PASS level, on the tiny fixture model: what keds_hip.h promises of a whole tower pass under
numerics = "auto" (tests/test_gpu_guard_edges.py holds the kernels' flags per row and per element).

5. A residual stream that leaves the fp16 range.  One bias element of block 0 raised to 1e5: the fp32 reference is finite and the
   largest |row mean| / row std at any LayerNorm input is far below 1 -- no ratio can have fired -- but the fp16 stream of the fast
   flow stores inf.  The pass must come back finite, with the guard tripped, equal to the bit to a model put on the destination flow
   beforehand, and a following pass of an unmodified model on the same thread must not trip.
6. Pad rows of a packed text pass.  The rows between the last caption and the next 256-row tile belong to no sample; behind block 0
   they hold out_proj.bias alone, a row of mean 0.2 and deviation 0.001.  They must not reach the guard: the same captions do not
   trip it when they run rectangular."""
import warnings

import numpy as np
import pytest
import torch

import keds_amd
from keds_amd import _lib, session
from keds_amd import model as keds_model
from oracle import keds_oracle as O
from tests import guard_check as gd
from tests.conftest import golden_path
from tests.gpu_util import report

pytestmark = pytest.mark.gpu

TINY = dict(embed_dim=128, image_resolution=56, vision_layers=2, vision_width=128, vision_patch_size=14,
            context_length=77, vocab_size=512, transformer_width=128, transformer_layers=2)
BIG = 1.0e5


def _captions():
    """the ragged 24-caption batch of test_gpu_session.py (without its pseudo-token splice): lengths 7 .. 60"""
    rs = np.random.RandomState(4)
    B, L = 24, 77
    rag = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        e = int(rs.randint(6, 60))
        rag[b, :e] = rs.randint(1, 500, size=e)
        rag[b, 0], rag[b, e] = 510, 511
    return torch.from_numpy(rag)


def _packs(text):
    """(rows_total, packed rows) if the library runs this batch on packed rows, read from the library's own plan of the pass
    (keds_text_runs_packed: its rule; keds_pass_plan_query: the zero step on x covers rows [rows_total, packed rows)), else None"""
    from tests.test_host_tower_plan import BUF, OPNAME, pass_query
    eot = (text == TINY["vocab_size"] - 1).int().argmax(dim=1)
    lens = eot + 1
    rows_total, B, seq_used = int(lens.sum()), text.shape[0], int(lens.max())
    lib = _lib.load()
    if not lib.keds_text_runs_packed(1, 0, lib.keds_text_trim_mode(), rows_total, B, seq_used):
        return None
    steps = pass_query("bf16", "text_packed", B, width=TINY["transformer_width"], heads=2, layers=TINY["transformer_layers"],
                       embed_dim=TINY["embed_dim"], lens=lens.tolist(), seq_max=seq_used)[0]
    zero = [s for s in steps if OPNAME[s["op"]] == "zero" and BUF[s["out"]] == "x"]
    if not zero:
        return rows_total, rows_total
    assert zero[0]["out_r0"] == rows_total
    return rows_total, zero[0]["out_r0"] + zero[0]["n"]


# ---- 5. stream overflow ----------------------------------------------------------------------------------------------------------
OVERFLOW = [("image", "visual.transformer.resblocks.0.mlp.c_proj.bias"), ("image", "visual.transformer.resblocks.0.attn.out_proj.bias"),
            ("text_rectangular", "transformer.resblocks.0.mlp.c_proj.bias"), ("text_packed", "transformer.resblocks.0.mlp.c_proj.bias")]


def _reference_is_tame(sd, tower, inp):
    """on the CPU: the oracle's output is finite, the stream reaches 1e5, and no row at any LayerNorm input has |mean| / std >= 1"""
    if tower == "image":
        want = O.encode_image(sd, inp)
        x, bounds = gd.image_rows64(sd, inp)
        t = gd.Tower64(sd, "visual.transformer.", 2)
        t.run(x, gd.attend_samples(bounds, 2, causal=False))
    else:
        want = O.encode_text(sd, inp)
        x, bounds = gd.text_rows64(sd, inp)
        t = gd.Tower64(sd, "transformer.", 2)
        t.run(x, gd.attend_samples(bounds, 2, causal=True))
    worst = max(float(r.max()) for r in t.ratios)
    assert bool(torch.isfinite(want).all()) and worst < 1.0 and t.max_abs >= 0.99 * BIG, (worst, t.max_abs)
    return worst


@pytest.mark.parametrize("precision", ("bf16", "fp16"))
@pytest.mark.parametrize("tower,key", OVERFLOW, ids=[f"{t}.{k.split('.')[-2]}" for t, k in OVERFLOW])
def test_a_stream_beyond_the_fp16_range_trips_the_guard(tower, key, precision, monkeypatch):
    sd = O.synth_clip_state_dict(**TINY, seed=7)
    clean = dict(sd)
    sd[key] = sd[key].clone()
    sd[key][7] = BIG
    if tower == "image":
        inp = torch.from_numpy(dict(np.load(golden_path("clip_tiny.npz")))["image"])
    else:
        inp = _captions()
        monkeypatch.setattr(keds_model, "TEXT_PACKED", tower == "text_packed")
        assert _packs(inp) is not None
    worst = _reference_is_tame(sd, tower, inp)

    def encode(m):
        return m.encode_image(inp.cuda()) if tower == "image" else m.encode_text(inp.cuda())
    dest = keds_amd.build_model(dict(sd), fp16=False).cuda()
    dest = dest.set_precision("fp32x3") if precision == "fp16" else dest.set_numerics("safe")
    want = encode(dest)
    assert torch.isfinite(want).all()
    m = keds_amd.build_model(dict(sd), fp16=False).cuda().set_precision(precision)
    assert m.numerics == "auto"
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = encode(m)
    rw = [w for w in rec if issubclass(w.category, RuntimeWarning)]
    report(f"guard_passes.overflow.{tower}.{key.split('.')[-2]}.{precision}", finite=bool(torch.isfinite(out).all()),
           tripped=bool(m.numerics_tripped), precision_after=m.precision, warnings=len(rw), worst_ratio_of_the_reference=worst)
    assert torch.isfinite(out).all(), "non-finite features returned"
    if precision == "fp16":
        assert len(rw) == 1 and getattr(m, "fp16_range_trips", 0) == 1 and m.precision == "fp32x3"
        assert m.numerics_sync() is True
    else:
        assert m.numerics_tripped and len(rw) == 1 and m.precision == "bf16"
    assert torch.equal(out, want)
    # the thread's flag is the tripped model's own: an unmodified model that follows does not trip
    after = keds_amd.build_model(clean, fp16=False).cuda().set_precision(precision)
    out2 = encode(after)
    assert torch.isfinite(out2).all() and not after.numerics_tripped and after.precision == precision and after.numerics_sync() is False


# ---- 6. pad rows of a packed text pass -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = session.Context(0)
    yield c
    c.close()


def _ratios64(sd, text, packed_rows):
    """float64 model of the packed pass -> (largest ratio of a valid row, of a pad row) over every LayerNorm input of every block"""
    eot = (text == TINY["vocab_size"] - 1).int().argmax(dim=1)
    lens = (eot + 1).tolist()
    total = sum(lens)
    x, bounds = gd.text_rows64(sd, text, lens, pad_rows=packed_rows - total)
    t = gd.Tower64(sd, "transformer.", 2)
    t.run(x, gd.attend_samples(bounds, 2, causal=True))
    return max(float(r[:total].max()) for r in t.ratios), max(float(r[total:].max()) for r in t.ratios)


def _both_layouts(ctx, sd, text, compute):
    """-> (packed output, its flag, rectangular output, its flag) of the handle calls under a guard flag of their own"""
    lib = _lib.load()
    txt = session.Text(ctx, {k: v.numpy() for k, v in sd.items()}, compute=compute)
    eot = (text == TINY["vocab_size"] - 1).int().argmax(dim=1)
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    try:
        _lib.check(lib.keds_numerics_guard_set(flags.data_ptr()), "keds_numerics_guard_set")
        packed = txt.forward(text.cuda(), eot)                      # read-out columns on the host: packed rows
        _lib.check(lib.keds_numerics_guard_set(flags.data_ptr() + 4), "keds_numerics_guard_set")
        rect = txt.forward(text.cuda(), eot.cuda())                 # on the device: the rectangular cut
    finally:
        lib.keds_numerics_guard_set(None)
    torch.cuda.synchronize()
    f = flags.cpu().tolist()
    txt.close()
    return packed, f[0], rect, f[1]


@pytest.mark.parametrize("compute", (_lib.DT_BF16, _lib.DT_F16), ids=("bf16", "fp16"))
def test_pad_rows_of_a_packed_text_pass_do_not_reach_the_guard(ctx, compute):
    """Block 0's attn.out_proj.bias = 0.2 + 0.001 randn.  Asserted on the CPU first, by the float64 model: no valid row exceeds 4 at
    any LayerNorm input, a pad row reaches 40.  The control adds an offset to the token embedding until VALID rows reach 40 (asserted
    as well): the flag must then rise in both layouts.  (The offset of the control is 1.0, not the bias's 0.2: on this fixture's
    embeddings -- deviation 0.02 + 0.01 -- 0.2 gives valid rows a ratio of 11, which is no trip.)"""
    text = _captions()
    pk = _packs(text)
    assert pk is not None and pk[1] > pk[0], "the batch must run packed, with zero rows behind the captions"
    sd = O.synth_clip_state_dict(**TINY, seed=7)
    g = torch.Generator().manual_seed(11)
    sd["transformer.resblocks.0.attn.out_proj.bias"] = (0.2 + 0.001 * torch.randn(128, generator=g)).float()
    valid, pad = _ratios64(sd, text, pk[1])
    assert valid <= 4.0 and pad >= 40.0, (valid, pad)
    packed, f_packed, rect, f_rect = _both_layouts(ctx, sd, text, compute)
    report(f"guard_passes.pad_rows.compute{compute}", rows_total=pk[0], packed_rows=pk[1], valid_ratio=valid, pad_ratio=pad,
           flag_packed=f_packed, flag_rectangular=f_rect)
    assert torch.isfinite(packed).all()
    assert f_rect == 0, "the rectangular pass tripped: the premise of the test does not hold"
    assert f_packed == 0, "rows that belong to no caption tripped the numerics guard"
    assert torch.equal(packed, rect)
    # control: valid rows off centre trip both layouts
    sd2 = dict(sd)
    sd2["token_embedding.weight"] = sd["token_embedding.weight"] + 1.0
    valid2, _ = _ratios64(sd2, text, pk[1])
    assert valid2 >= 40.0, valid2
    _, c_packed, _, c_rect = _both_layouts(ctx, sd2, text, compute)
    assert c_packed == 1 and c_rect == 1, (c_packed, c_rect)


@pytest.mark.parametrize("compute", (_lib.DT_F32, _lib.DT_F32X3), ids=("fp32", "fp32x3"))
def test_pad_rows_of_a_packed_text_pass_in_the_fp32_flows(ctx, compute):
    """The fp32 and fp32x3 flows have no ratio guard, and their zero rows reach the split kernels (fp32x3: the thread's flag is their
    overflow flag) only as LayerNorm outputs and attention outputs of zero rows.  The same planted bias: the flag stays down in both
    layouts and the features are finite."""
    text = _captions()
    pk = _packs(text)
    assert pk is not None and pk[1] > pk[0]
    sd = O.synth_clip_state_dict(**TINY, seed=7)
    g = torch.Generator().manual_seed(11)
    sd["transformer.resblocks.0.attn.out_proj.bias"] = (0.2 + 0.001 * torch.randn(128, generator=g)).float()
    packed, f_packed, rect, f_rect = _both_layouts(ctx, sd, text, compute)
    report(f"guard_passes.pad_rows.compute{compute}", flag_packed=f_packed, flag_rectangular=f_rect,
           equal_bits=bool(torch.equal(packed, rect)))
    assert torch.isfinite(packed).all() and torch.isfinite(rect).all()
    assert f_packed == 0 and f_rect == 0, (f_packed, f_rect)
