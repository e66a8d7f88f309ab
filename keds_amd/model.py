"""Drop-in model API of the KEDs retrieval path on MI355X.

Same class names, constructor arguments, method signatures and ``state_dict`` keys as the
reference's ``src/model/model.py`` (CLIP :431-911, IM2TEXT :105-123, CrossFormer :81-101,
build_model :951, convert_weights :927), so reference checkpoints load unchanged
(``main.py:330-341`` layout) and reference call sites (``eval_utils.py:610,652-695``,
``eval_retrieval.py:96-101``) run as written.  The modules here only HOLD parameters
(torch.nn containers); every forward runs hand-written gfx950 kernels through
``libkeds_hip.so`` -- bf16 / fp16 MFMA GEMMs with fp32 accumulation, the residual stream of a tower kept in
fp16 with LayerNorm folded into the GEMMs (fp32 stream + stand-alone LayerNorm in numerics mode "safe",
selected automatically by the numerics guard), fp32 LayerNorm / softmax statistics.  There is no PyTorch compute path and no CPU fallback:
calling a forward without the library or without a GPU raises RuntimeError.

Token-level outputs run in the library as well: ``encode_image(mid_feature=True)`` (the residual stream after
every block), ``VisualTransformer.forward`` / ``get_tokens`` and ``get_text_tokens``.

Out of scope: ModifiedResNet towers, `encode_text_img_vis`, the
training-only splice variants and `forward(extra=True)` (undefined in the reference itself, App. B).
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from collections import OrderedDict
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch
from torch import nn

from . import _lib
from ._lib import check, load, ptr, stream


def _bf16(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.bfloat16).contiguous()


def _f16(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float16).contiguous()


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


# ---------------------------------------------------------------------------------------------------
# parameter containers (key names are the checkpoint contract)
# ---------------------------------------------------------------------------------------------------
class LayerNorm(nn.LayerNorm):
    """Parameter holder; the statistics run in fp32 inside the HIP kernels (model.py:291-297)."""


class QuickGELU(nn.Module):
    """x * sigmoid(1.702 x), fused into the c_fc GEMM epilogue (model.py:300-302)."""


class ResidualAttentionBlock(nn.Module):
    def __init__(self, d_model: int, n_head: int, attn_mask: Optional[torch.Tensor] = None):
        super().__init__()
        self.attn = nn.MultiheadAttention(d_model, n_head)     # holds in_proj_weight/bias, out_proj.*
        self.ln_1 = LayerNorm(d_model)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(d_model, d_model * 4)), ("gelu", QuickGELU()),
                                              ("c_proj", nn.Linear(d_model * 4, d_model))]))
        self.ln_2 = LayerNorm(d_model)
        self.causal = attn_mask is not None


class Transformer(nn.Module):
    def __init__(self, width: int, layers: int, heads: int, attn_mask: Optional[torch.Tensor] = None):
        super().__init__()
        self.width, self.layers, self.heads = width, layers, heads
        self.resblocks = nn.Sequential(*[ResidualAttentionBlock(width, heads, attn_mask) for _ in range(layers)])


class VisualTransformer(nn.Module):
    def __init__(self, input_resolution: int, patch_size: int, width: int, layers: int, heads: int, output_dim: int):
        super().__init__()
        self.input_resolution, self.output_dim, self.patch_size = input_resolution, output_dim, patch_size
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=False)
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn((input_resolution // patch_size) ** 2 + 1, width))
        self.ln_pre = LayerNorm(width)
        self.transformer = Transformer(width, layers, heads)
        self.ln_post = LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))

    # The tower runs through the engine of the CLIP model that owns it: CLIP.__init__ leaves a weak reference here (no
    # submodule, no state_dict key).
    def _owner(self) -> "CLIP":
        ref = self.__dict__.get("_clip_ref")
        clip = ref() if ref is not None else None
        if clip is None:
            raise RuntimeError("keds_amd.VisualTransformer runs through the CLIP model that owns it (model.visual)")
        return clip

    def __getstate__(self):
        state = super().__getstate__()
        state.pop("_clip_ref", None)             # (a weak reference does not pickle; CLIP.__setstate__ sets it again)
        return state

    def forward(self, x, mid_feature=False):
        """model.py:393-415: [B, embed_dim], or with mid_feature (features, [residual stream after each block [B, S, width]]
        x layers) -- CLIP.encode_image."""
        return self._owner().encode_image(x, mid_feature=mid_feature)

    def get_tokens(self, x):
        """model.py:418-427: all S tokens after the last block, before ln_post: [B, S, width] in the model's dtype."""
        return self._owner()._image_pass(x, False, "tokens")


def _pack_tower(tr: Transformer, seq: int, causal: bool, keep: list, cls_only: bool = False,
                fp8: bool = False, folded: bool = True, f32: bool = False, f16: bool = False) -> _lib.TowerParams:
    """Every block's weights in the layout and operand types of the operating point, built by the library's
    keds_block_pack (include/keds_hip.h) -- the routine the handle ABI's loader calls too -- into one device buffer per block."""
    lib = load()
    blocks = (_lib.BlockParams * tr.layers)()
    mode = (tr.width, 1 if fp8 else 0, int(f32), 1 if f16 else 0, 1 if folded else 0)
    nbytes = lib.keds_block_pack_bytes(*mode)
    if not nbytes:
        raise ValueError(_lib.last_error())
    for i, blk in enumerate(tr.resblocks):
        src = dict(
            ln1_g=_f32(blk.ln_1.weight), ln1_b=_f32(blk.ln_1.bias), ln2_g=_f32(blk.ln_2.weight), ln2_b=_f32(blk.ln_2.bias),
            qkv_w=_f32(blk.attn.in_proj_weight), qkv_b=_f32(blk.attn.in_proj_bias),
            out_w=_f32(blk.attn.out_proj.weight), out_b=_f32(blk.attn.out_proj.bias),
            fc_w=_f32(blk.mlp.c_fc.weight), fc_b=_f32(blk.mlp.c_fc.bias),
            proj_w=_f32(blk.mlp.c_proj.weight), proj_b=_f32(blk.mlp.c_proj.bias))
        buf = torch.empty(nbytes, dtype=torch.uint8, device=src["qkv_w"].device)
        check(lib.keds_block_pack(C.byref(_lib.BlockSource(**{k: ptr(v) for k, v in src.items()})), *mode, ptr(buf), nbytes,
                                  C.byref(blocks[i]), stream()), "keds_block_pack")
        torch.cuda.current_stream().synchronize()          # the fp32 views of a 16-bit checkpoint die here
        keep.append(buf)
    keep.append(blocks)
    return _lib.TowerParams(tr.width, tr.layers, tr.heads, seq, 1 if causal else 0, blocks, 1 if fp8 else 0,
                            1 if cls_only else 0, int(f32), 1 if f16 else 0)


class _Packed:
    """bf16/fp16/fp32 device copies of the weights in the layout the kernels want + the ABI structs."""

    def __init__(self, clip: "CLIP", folded: bool = True):
        self.keep: list = []
        self.folded = folded
        v = clip.visual
        width = v.conv1.weight.shape[0]
        P = v.patch_size
        kreal = 3 * P * P
        self.kpad = (kreal + 63) // 64 * 64
        prec = getattr(clip, "precision", "bf16")
        f32 = 2 if prec == "fp32x3" else 1 if prec == "fp32" else 0      # (2: the block GEMMs on split fp16 operands, the rest as 1)
        f16 = prec == "fp16"                                            # every 16-bit operand fp16, conv / projections included
        wdt = torch.float32 if f32 else torch.float16 if f16 else torch.bfloat16
        wcast = _f32 if f32 else _f16 if f16 else _bf16
        self.f32, self.f16 = f32, f16
        conv = torch.zeros((width, self.kpad), dtype=wdt, device=v.conv1.weight.device)
        conv[:, :kreal] = v.conv1.weight.detach().reshape(width, kreal).to(wdt)
        g = v.input_resolution // P
        t = dict(conv_w=conv, class_emb=_f32(v.class_embedding), pos_emb=_f32(v.positional_embedding),
                 ln_pre_g=_f32(v.ln_pre.weight), ln_pre_b=_f32(v.ln_pre.bias), ln_post_g=_f32(v.ln_post.weight),
                 ln_post_b=_f32(v.ln_post.bias), proj_t=wcast(v.proj.detach().t()))
        self.keep.append(t)
        fp8 = getattr(clip, "precision", "bf16") == "fp8"
        self.vit = _lib.VitParams(_pack_tower(v.transformer, g * g + 1, False, self.keep, cls_only=True, fp8=fp8, folded=folded,
                                              f32=f32, f16=f16),
                                  v.input_resolution, P,
                                  self.kpad, v.output_dim, *[ptr(t[k]) for k in (
                                      "conv_w", "class_emb", "pos_emb", "ln_pre_g", "ln_pre_b", "ln_post_g",
                                      "ln_post_b", "proj_t")])
        tt = dict(token_emb=_f32(clip.token_embedding.weight), pos_emb=_f32(clip.positional_embedding),
                  ln_final_g=_f32(clip.ln_final.weight), ln_final_b=_f32(clip.ln_final.bias),
                  proj_t=wcast(clip.text_projection.detach().t()))
        self.keep.append(tt)
        self.text = _lib.TextParams(_pack_tower(clip.transformer, clip.context_length, True, self.keep,
                                                fp8=fp8 and clip.transformer.width % 256 == 0, folded=folded, f32=f32,
                                                f16=f16),
                                    clip.vocab_size, clip.embed_dim,
                                    *[ptr(tt[k]) for k in ("token_emb", "pos_emb", "ln_final_g", "ln_final_b", "proj_t")])
        self.device = conv.device


_OUT_TYPE = {torch.bfloat16: 0, torch.float32: 1, torch.float16: 2}     # out_type of the token entry points (keds_hip.h)
TEXT_PACKED = True          # the text tower on packed rows when captions end at different columns (tests switch it off for an A/B)
GUARD_EAGER_PASSES = 8      # numerics = "auto": tower passes whose guard flag is read back at once (see CLIP.__init__)


def x3_chunk(width, rows_per_sample):
    """samples per call of an "fp32x3" tower pass: the split-operand GEMMs address their planes with 32-bit byte offsets
    (keds_gemm_x3), so the MLP hidden planes of one call -- rows * 4 * width * 2 bytes -- stay below 2 GiB, less a margin of 512 rows"""
    return max(1, ((1 << 31) // (8 * width) - 512) // rows_per_sample)


class CLIP(nn.Module):
    def __init__(self, embed_dim: int, image_resolution: int, vision_layers: Union[Tuple[int, int, int, int], int],
                 vision_width: int, vision_patch_size: int, context_length: int, vocab_size: int,
                 transformer_width: int, transformer_heads: int, transformer_layers: int,
                 extra_transformer_layers: int = 0, share_projection_layer: bool = True):
        super().__init__()
        if isinstance(vision_layers, (tuple, list)):
            raise NotImplementedError("ModifiedResNet visual towers are out of scope (ViT only)")
        if extra_transformer_layers:
            raise NotImplementedError("extra_transformer_layers is unused by the retrieval path")
        self.embed_dim, self.context_length = embed_dim, context_length
        self.share_projection_layer, self.has_extra = share_projection_layer, False
        self.visual = VisualTransformer(image_resolution, vision_patch_size, vision_width, vision_layers,
                                        vision_width // 64, embed_dim)
        object.__setattr__(self.visual, "_clip_ref", weakref.ref(self))
        self.transformer_width = transformer_width
        self.transformer = Transformer(transformer_width, transformer_layers, transformer_heads,
                                       attn_mask=self.build_attention_mask())
        self.vocab_size = vocab_size
        self.end_id = vocab_size - 1
        self.token_embedding = nn.Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, transformer_width))
        self.ln_final = LayerNorm(transformer_width)
        self.text_projection = nn.Parameter(torch.empty(transformer_width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
        self.initialize_parameters()
        self._packed: Optional[_Packed] = None
        self._ws = _lib.Workspace()
        self.precision = os.environ.get("KEDS_PRECISION", "bf16")
        # "auto": the fast tower flow (fp16 residual stream, LayerNorm folded into the GEMMs) guarded by a device flag --
        # a row with |mean|/std > 32, or a value the fp16 stream cannot hold, re-runs the pass on the fp32-stream flow with stand-alone
        # LayerNorm and keeps the model there (keds_hip.h, keds_numerics_guard_set); "fast": no guard; "safe": always the
        # fp32-stream flow (what KEDS_DETERMINISTIC=1 selected before).
        self.numerics = "safe" if os.environ.get("KEDS_DETERMINISTIC", "0") == "1" else "auto"      # (set_numerics() changes it)
        self.numerics_tripped = False
        self._guard: Optional[torch.Tensor] = None
        # "auto" reads the guard flag back EAGERLY (one host-device sync per pass, the pass is re-run on the safe flow when it
        # tripped) for the first GUARD_EAGER_PASSES passes after the weights were packed -- what trips the guard is a property
        # of the weights far more than of one batch -- and LAZILY afterwards: the flag travels to pinned host memory behind
        # the pass, is looked at when the next pass is enqueued (or by numerics_sync()), and a late trip warns, switches the
        # model to the safe flow for every later pass and sets `numerics_late_trip` (the passes since the last check ran on
        # the fast flow: re-run them if their accuracy matters).  The host then never waits for a tower: the search of batch
        # i and the tower of batch i+1 are enqueued while batch i is still running (round-2 advisor finding).
        self.numerics_late_trip = False
        self._guard_eager_left = GUARD_EAGER_PASSES
        self._guard_host: Optional[torch.Tensor] = None
        self._guard_event = None

    # ---- init (same distributions as model.py:511-541) ------------------------------------------
    def initialize_parameters(self):
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        w, L = self.transformer.width, self.transformer.layers
        for blk in self.transformer.resblocks:
            nn.init.normal_(blk.attn.in_proj_weight, std=w ** -0.5)
            nn.init.normal_(blk.attn.out_proj.weight, std=w ** -0.5 * (2 * L) ** -0.5)
            nn.init.normal_(blk.mlp.c_fc.weight, std=(2 * w) ** -0.5)
            nn.init.normal_(blk.mlp.c_proj.weight, std=w ** -0.5 * (2 * L) ** -0.5)
        nn.init.normal_(self.text_projection, std=w ** -0.5)

    def build_attention_mask(self):
        m = torch.full((self.context_length, self.context_length), float("-inf"))
        return m.triu_(1)           # kept for API parity; the kernel applies the causal mask itself

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    def __setstate__(self, state):
        super().__setstate__(state)
        if "visual" in self._modules:                # (unpickled / deep-copied: the tower's link to THIS model)
            object.__setattr__(self.visual, "_clip_ref", weakref.ref(self))

    # ---- weight packing -------------------------------------------------------------------------
    def _apply(self, fn, *a, **k):
        self._packed = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        self._packed = None
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def repack(self):
        """Re-read the parameters (call after mutating weights in place)."""
        self._packed = None

    def set_precision(self, precision: str = "bf16"):
        """"bf16" (default: bf16 / fp16 GEMM operands, fp32 accumulate), "fp8" (BASELINE config 5: the image tower's GEMMs on
        MXFP8 operands -- OCP e4m3 with an e8m0 scale per 32 elements; needs vision width % 256 == 0; the text tower follows
        when its width is a multiple of 256 too, e.g. 768), or "fp32": the reference's own evaluation arithmetic
        (eval_retrieval.py:108-109, `--precision` params.py:227-232) -- no operand is rounded, every product runs on the
        f32-input matrix instruction, residual stream / LayerNorm / attention stay fp32 (csrc/f32path.hip).  About a tenth
        of the default flow's throughput; embeddings agree with the fp32 reference to ~1e-6 and Recall@k is equal.
        "fp32x3" (round 5): the same fp32 flow with the four GEMMs of every block on SPLIT fp16 operands -- x = hi + lo
        (22 significant bits), hi.hi + hi.lo + lo.hi on the fp16 matrix instruction, fp32 accumulate: fp32-grade embeddings
        (Recall@k equal) at more than twice "fp32"'s throughput; values beyond the fp16 range (|x| >= 65504) send the model
        back to "fp32" by themselves.
        "fp16": the reference's `--precision fp16` (convert_weights, model.py:927-948): EVERY GEMM operand of both towers is
        fp16 -- weights rounded as stored, qkv, attention probabilities and output, MLP hidden layer, patches and read-out rows --
        on the fp16 matrix instruction (the bf16 rate), fp32 accumulate, LayerNorm folded as in "bf16".  Needs the folded path
        (not with set_numerics("safe")).  Under numerics "auto" a value beyond the fp16 range (or a statistics trip) moves the
        model to "fp32x3" -- a RuntimeWarning, `fp16_range_trips` += 1 -- and the pass runs again there.  The knowledge
        modules run their exact fp32 path (compose_query_features)."""
        if precision not in ("bf16", "fp16", "fp8", "fp32", "fp32x3"):
            raise ValueError("precision must be 'bf16', 'fp16', 'fp8', 'fp32' or 'fp32x3'")
        if precision == "fp8" and (self.visual.transformer.width % 256 != 0 or self.numerics == "safe"):
            raise ValueError("fp8 needs a vision width that is a multiple of 256 and the folded LayerNorm path")
        if precision == "fp16" and self.numerics == "safe":
            raise ValueError("fp16 needs the folded LayerNorm path (numerics 'auto' or 'fast')")
        # a pass still waiting for its lazy guard check ran at the CURRENT precision: settle it there before switching
        self._guard_poll(wait=True)
        if precision == "fp16" and self.numerics_tripped:
            raise ValueError("fp16 needs the folded LayerNorm path; the numerics guard has moved this model to the fp32-stream "
                             "flow (set_numerics() resets it)")
        self.precision = precision
        self._packed = None
        return self

    def _engine(self) -> _Packed:
        _lib.require_gpu()
        load()
        if not self.visual.conv1.weight.is_cuda:
            raise RuntimeError("keds_amd.CLIP: move the model to the GPU first (model.cuda()); no CPU path exists")
        folded = self.numerics != "safe" and not self.numerics_tripped
        if self._packed is None or self._packed.folded != folded:
            self._packed = _Packed(self, folded=folded)
            self._guard_eager_left = GUARD_EAGER_PASSES
        _lib.ensure_gemm_workspace(self._packed.device)
        return self._packed

    def set_numerics(self, mode: str = "auto"):
        if mode not in ("auto", "fast", "safe"):
            raise ValueError("numerics must be 'auto', 'fast' or 'safe'")
        if mode == "safe" and self.precision in ("fp8", "fp16"):
            raise ValueError(f"{self.precision} needs the folded LayerNorm path")
        self._guard_poll(wait=True)
        self.numerics, self.numerics_tripped, self.numerics_late_trip = mode, False, False
        self._fp16_trip_seen = False
        self._guard_eager_left = GUARD_EAGER_PASSES
        return self

    def _guard_trip(self, late: bool):
        import warnings
        if self.precision == "fp16":
            # an fp16 operand left the fp16 range (|v| > 65504 / non-finite) or the folded LayerNorm's statistics tripped: the
            # model moves to "fp32x3" (Recall-equal, no fp16 storage of qkv / hidden values) -- as fp32x3 moves to fp32 on its own trip
            warnings.warn("keds_amd.CLIP: fp16 tower values left the fp16 range (or |row mean|/std > 32); " +
                          ("the passes since the last check ran in fp16 (numerics_late_trip); later passes run" if late else
                           "re-running") + " on precision 'fp32x3' and staying there", RuntimeWarning)
            self._guard.zero_()
            self.fp16_range_trips = getattr(self, "fp16_range_trips", 0) + 1
            self._fp16_trip_seen = True
            self.numerics_late_trip = self.numerics_late_trip or late
            self.set_precision("fp32x3")
            return
        warnings.warn("keds_amd.CLIP: activations left the range the fast tower flow is accurate in (|row mean|/std > 32 or a "
                      "non-finite fp16 residual); " + ("the passes since the last check ran on the fast flow (numerics_late_trip); "
                      "later passes run" if late else "re-running") + " on the fp32-stream flow and staying there", RuntimeWarning)
        self._guard.zero_()
        self.numerics_tripped = True
        self.numerics_late_trip = self.numerics_late_trip or late

    def _guard_poll(self, wait: bool) -> None:
        """Look at the flag copy that travelled behind the last lazily checked pass (blocking only when `wait`)."""
        ev = self._guard_event
        if ev is None or not (wait or ev.query()):
            return
        if wait:
            ev.synchronize()
        self._guard_event = None
        if int(self._guard_host[0]) != 0 and not self.numerics_tripped:
            self._guard_trip(late=True)

    def numerics_sync(self) -> bool:
        """Block until every lazily checked pass has been verified; True when the guard tripped at any point (the model is
        then on the safe flow -- or, after an fp16 trip, on precision "fp32x3"; `numerics_late_trip` says whether passes had
        already been returned from the fast flow)."""
        self._guard_poll(wait=True)
        return self.numerics_tripped or getattr(self, "_fp16_trip_seen", False)

    def numerics_checked(self, fn):
        """Run `fn()` (any number of encoder passes whose outputs the caller KEEPS: a feature-extraction or evaluation loop)
        and return its result only after every pass in it has been verified: the lazily checked guard is synchronised
        behind the loop, and when it tripped while passes of this loop had already been returned from the fast flow
        (`numerics_late_trip`), the loop is run again -- the model is on the fp32-stream flow by then, so the second run is
        clean.  Loops that collect features must not end on an unverified pass (retrieval.py uses this everywhere)."""
        before = self.numerics_late_trip
        out = fn()
        self.numerics_sync()
        if self.numerics_late_trip and not before:
            out = fn()
            self.numerics_sync()
        return out

    def _guarded(self, run):
        """Run one tower pass (`run(engine)` enqueues it and returns the output tensor) under the numerics guard."""
        # (a stream that is being captured into a hipGraph can be neither synchronised nor queried -- an event query inside a
        # global-mode capture invalidates it: no flag read there; call numerics_sync() before the capture, or capture a
        # model on set_numerics("safe"))
        if torch.cuda.is_current_stream_capturing():
            return run(self._engine())
        self._guard_poll(wait=False)
        eng = self._engine()
        if self.precision == "fp32x3":
            # split fp16 operands hold |x| < 65504 only: the split / LayerNorm kernels raise the guard flag beyond that, and a
            # non-finite output says the MLP hidden layer went there -- either way this pass and all later ones run on the
            # f32-input matrix instruction instead ("fp32": slower, no range limit).  Checked at once: a pass takes ~80 ms.
            if self._guard is None or self._guard.device != eng.device:
                self._guard = torch.zeros(1, dtype=torch.int32, device=eng.device)
            lib = load()
            check(lib.keds_numerics_guard_set(ptr(self._guard)), "keds_numerics_guard_set")
            try:
                out = run(eng)
            finally:
                check(lib.keds_numerics_guard_set(None), "keds_numerics_guard_set")
            first = out[0] if isinstance(out, tuple) else out       # (token passes: the features, or the tokens)
            if int(self._guard.item()) == 0 and bool(torch.isfinite(first).all()):
                return out
            self._guard.zero_()
            self.x3_range_trips = getattr(self, "x3_range_trips", 0) + 1
            self.set_precision("fp32")
            return run(self._engine())
        if self.numerics != "auto" or not eng.folded or self.precision in ("fp8", "fp32"):
            return run(eng)
        if self._guard is None or self._guard.device != eng.device:
            self._guard = torch.zeros(1, dtype=torch.int32, device=eng.device)
        lib = load()
        check(lib.keds_numerics_guard_set(ptr(self._guard)), "keds_numerics_guard_set")
        try:
            out = run(eng)
        finally:
            check(lib.keds_numerics_guard_set(None), "keds_numerics_guard_set")
        if self._guard_eager_left <= 0:                      # lazy: the flag follows the pass to pinned host memory
            if self._guard_host is None:
                self._guard_host = torch.zeros(1, dtype=torch.int32).pin_memory()
                self._guard_event_obj = torch.cuda.Event()
            if self._guard_event is not None:                # at most one copy in flight: the flag is sticky, nothing is lost
                self._guard_poll(wait=True)
            self._guard_host.copy_(self._guard, non_blocking=True)
            self._guard_event_obj.record()
            self._guard_event = self._guard_event_obj
            return out
        self._guard_eager_left -= 1
        if int(self._guard.item()) == 0:
            return out
        self._guard_trip(late=False)
        return self._guarded(run)           # (the safe flow -- or, after an fp16 trip, the fp32x3 branch above)

    # ---- encoders ------------------------------------------------------------------------------------
    def encode_image(self, image, mid_feature=False, mask_token=False, normalize: bool = False):
        """model.py:569-575 -> VisualTransformer.forward :393-415.  image [B,3,R,R] -> [B, embed_dim].
        mid_feature=True (:337-342, 393-410): (features [B, embed_dim], [the residual stream after each block, [B, S, width]]
        x layers) from ONE pass, all in the model's dtype; the list holds views of one [layers, B, S, width] tensor."""
        return self._image_pass(image, normalize, "mid" if mid_feature else "features")

    def _image_pass(self, image, normalize, mode):
        """mode "features": encode_image; "mid": features + per-block taps; "tokens": the last block's tokens only."""
        eng = self._engine()
        if image.dim() != 4 or image.shape[1] != 3 or image.shape[2] != self.visual.input_resolution \
                or image.shape[3] != self.visual.input_resolution:
            raise RuntimeError(f"expected images [B,3,{self.visual.input_resolution},{self.visual.input_resolution}], "
                               f"got {tuple(image.shape)}")
        img = image.to(eng.device, dtype=torch.float32).contiguous()
        B = img.shape[0]
        tr = self.visual.transformer
        S = (self.visual.input_resolution // self.visual.patch_size) ** 2 + 1
        dt = self.dtype
        if B == 0:                                    # an empty last batch of a loader: the reference returns [0, embed_dim]
            feats = torch.empty((0, self.embed_dim), dtype=dt, device=eng.device)
            if mode == "features":
                return feats
            if mode == "tokens":
                return torch.empty((0, S, tr.width), dtype=dt, device=eng.device)
            return feats, list(torch.empty((tr.layers, 0, S, tr.width), dtype=dt, device=eng.device).unbind(0))
        if self.precision == "fp32x3":
            # the split-operand GEMMs address their planes with 32-bit byte offsets (keds_gemm_x3): the MLP hidden planes of one call
            # must stay below 2 GiB -- rows * 4 * width * 2 bytes.  Larger batches run in chunks (rows are independent between samples).
            chunk = x3_chunk(self.visual.transformer.width, (self.visual.input_resolution // self.visual.conv1.kernel_size[0]) ** 2 + 1)
            if B > chunk:
                parts = [self._image_pass(img[i:i + chunk], normalize, mode) for i in range(0, B, chunk)]
                if mode == "mid":
                    return (torch.cat([p[0] for p in parts]),
                            [torch.cat([p[1][l] for p in parts]) for l in range(tr.layers)])
                return torch.cat(parts)
        lib = load()
        if mode != "features" and dt not in _OUT_TYPE:
            raise RuntimeError(f"token outputs come as fp32, fp16 or bf16, not {dt}")

        def run(eng):
            nbytes = lib.keds_vit_workspace_bytes(C.byref(eng.vit), B)
            ws = self._ws.get(nbytes, eng.device)
            if mode == "features":
                out = torch.empty((B, self.embed_dim), dtype=torch.float32, device=eng.device)
                check(lib.keds_vit_run(C.byref(eng.vit), ptr(img), B, ptr(out), 1 if normalize else 0, ptr(ws), ws.numel(),
                                       stream()), "keds_vit_run")
                return out
            out = torch.empty((B, self.embed_dim), dtype=torch.float32, device=eng.device) if mode == "mid" else None
            taps = torch.empty((tr.layers, B, S, tr.width), dtype=dt, device=eng.device) if mode == "mid" else None
            toks = torch.empty((B, S, tr.width), dtype=dt, device=eng.device) if mode == "tokens" else None
            check(lib.keds_vit_run_tokens(C.byref(eng.vit), ptr(img), B, ptr(out), 1 if normalize else 0, ptr(taps), ptr(toks),
                                          _OUT_TYPE[dt], ptr(ws), ws.numel(), stream()), "keds_vit_run_tokens")
            return (out, taps) if mode == "mid" else toks
        res = self._guarded(run)
        if mode == "features":
            return res.to(self.dtype)
        if mode == "tokens":
            return res
        return res[0].to(self.dtype), list(res[1].unbind(0))

    def _host_tokens(self, text: torch.Tensor) -> torch.Tensor:
        """The token rows on the HOST for the argument checks the reference's own indexing performs (one EOT per row, ids
        inside the table, the split token, the read-out column): one device-to-host copy per call when the caller passed
        device tokens (none for the CPU tokens a DataLoader yields) instead of five blocking reductions on the device."""
        th = text.cpu() if text.is_cuda else text
        # nn.Embedding raises IndexError on an id outside the table (model.py:579); the gather kernel does not check
        if th.numel() and (int(th.min()) < 0 or int(th.max()) >= self.vocab_size):
            raise IndexError(f"token id outside [0, {self.vocab_size})")
        return th

    def _eot_columns(self, text: torch.Tensor) -> torch.Tensor:
        hits = text == self.end_id
        if not bool((hits.sum(dim=1) == 1).all()):
            # the reference indexes nonzero()[:,1] with arange(B): anything but one EOT per row fails there
            raise IndexError("every token row must contain exactly one EOT token")
        return hits.to(torch.int32).argmax(dim=1)

    def _run_text(self, text, readout, img_tokens, insert_col, normalize):
        eng = self._engine()
        lib = load()
        B = text.shape[0]
        if B == 0:
            return torch.empty((0, self.embed_dim), dtype=self.dtype, device=eng.device)
        tok = text.to(eng.device, dtype=torch.int32).contiguous()           # (ids were range-checked on the host: _host_tokens)
        ro = readout.to(torch.int32).to(eng.device, non_blocking=True).contiguous()
        it = None if img_tokens is None else img_tokens.to(eng.device, dtype=torch.float32).contiguous()
        n_tok = 0 if it is None else it.shape[1]
        # columns to the right of the last read-out column cannot reach any read-out under the causal mask
        # (model.py:543-549): the host knows the read-out columns (they were derived from the host copy of the tokens), so
        # the library cuts the sequence there (keds_text_run_ex)
        seq_used = int(readout.max()) + 1
        # ... and columns to the right of a caption's OWN read-out column cannot reach that caption's read-out: when the captions of
        # a batch end at different columns the tower runs on PACKED rows, sample b owning len_b = read-out column + 1 of them
        # (keds_text_run_packed, round 6) -- sum(len_b) rows instead of B * max(len_b).  Worth it from an eighth fewer rows; the
        # MXFP8 tower and KEDS_TEXT_TRIM=0 keep the rectangular layout.
        if self.precision == "fp32x3":                       # (see encode_image: the planes of one call stay below 2 GiB)
            chunk = x3_chunk(self.transformer.width, self.context_length)
            if B > chunk:
                return torch.cat([self._run_text(text[i:i + chunk], readout[i:i + chunk], None if img_tokens is None else img_tokens[i:i + chunk],
                                                 insert_col, normalize) for i in range(0, B, chunk)])
        lens = readout.to(torch.int64).cpu() + 1
        rows_total = int(lens.sum())
        packed = None
        if TEXT_PACKED and lib.keds_text_runs_packed(1, int(self.precision == "fp8"), lib.keds_text_trim_mode(), rows_total, B, seq_used):
            off = torch.zeros(B + 1, dtype=torch.int64)
            off[1:] = torch.cumsum(lens, 0)
            both = torch.cat([off, off[:-1] + readout.to(torch.int64).cpu()]).to(torch.int32)
            both = both.to(eng.device, non_blocking=True)
            packed = (both[:B + 1], both[B + 1:])

        def run(eng):
            nbytes = lib.keds_text_workspace_bytes(C.byref(eng.text), B)
            ws = self._ws.get(nbytes, eng.device)
            out = torch.empty((B, self.embed_dim), dtype=torch.float32, device=eng.device)
            if packed is not None and self.precision != "fp8":
                check(lib.keds_text_run_packed(C.byref(eng.text), ptr(tok), ptr(packed[0]), ptr(packed[1]), rows_total, seq_used,
                                               ptr(it), n_tok, int(insert_col), B, ptr(out), 1 if normalize else 0, ptr(ws),
                                               ws.numel(), stream()), "keds_text_run_packed")
                return out
            check(lib.keds_text_run_ex(C.byref(eng.text), ptr(tok), ptr(ro), ptr(it), n_tok, int(insert_col), B, seq_used,
                                       ptr(out), 1 if normalize else 0, ptr(ws), ws.numel(), stream()), "keds_text_run")
            return out
        return self._guarded(run).to(self.dtype)

    def encode_text(self, text, normalize: bool = False):
        """model.py:577-590.  text int [B, L] -> [B, embed_dim]; read-out at the EOT column."""
        if text.dim() != 2 or text.shape[1] != self.context_length:
            raise RuntimeError(f"expected tokens [B,{self.context_length}], got {tuple(text.shape)}")
        if text.shape[0] == 0:
            return self._run_text(text, text.new_zeros(0), None, 0, normalize)
        return self._run_text(text, self._eot_columns(self._host_tokens(text)), None, 0, normalize)

    def encode_text_img_retrieval(self, text, img_tokens, split_ind=4, repeat=True, normalize: bool = False):
        """model.py:808-851.  The first `split_ind` token of ROW 0 is replaced by the 2 or 3 pseudo tokens of
        every row, the tail shifts right, read-out at EOT column + n_tok - 1."""
        if isinstance(img_tokens, tuple):
            raise NotImplementedError("tuple img_tokens (multi-insert) is not used by the retrieval path")
        b_size = img_tokens.shape[0]
        if repeat:
            text = text.repeat(b_size, 1)
        if text.shape[0] != b_size or text.shape[1] != self.context_length:
            raise RuntimeError(f"token rows {tuple(text.shape)} do not match {b_size} pseudo-token rows")
        n_tok = img_tokens.shape[1]
        if n_tok not in (2, 3):
            raise RuntimeError("img_tokens must carry 2 or 3 pseudo tokens per row (sequence length would not be "
                               f"{self.context_length})")
        if img_tokens.shape[2] != self.transformer_width:
            raise RuntimeError("pseudo-token width does not match the text transformer")
        th = self._host_tokens(text)
        where = (th[0] == int(split_ind)).nonzero()
        if where.numel() == 0:
            raise IndexError("split token not present in text[0]")
        ins = int(where[0])
        readout = self._eot_columns(th) + (n_tok - 1)
        if int(readout.max()) >= self.context_length:
            raise IndexError("read-out row beyond the context length")
        return self._run_text(text, readout, img_tokens, ins, normalize)

    def encode_text_img_train(self, text, img_tokens, split_ind=4, repeat=True, normalize: bool = False):
        """model.py:853-892 (the splice evaluate_fashion calls, eval_utils.py:957,969): the THREE token positions
        starting at the first `split_ind` of row 0 are overwritten by the pseudo tokens, nothing shifts, read-out at
        the EOT column.  Identical to the retrieval splice of a token row with positions ins+1, ins+2 deleted, which
        is how it runs here (integer column shuffling on the host side, same kernels).  `repeat` is ignored, as in
        the reference."""
        if img_tokens.dim() != 3 or img_tokens.shape[1] != 3:
            raise RuntimeError("encode_text_img_train needs exactly 3 pseudo tokens per row (sequence length would not "
                               f"be {self.context_length})")               # reference: size mismatch at model.py:883
        if text.dim() != 2 or text.shape[0] != img_tokens.shape[0] or text.shape[1] != self.context_length:
            raise RuntimeError(f"token rows {tuple(text.shape)} do not match {img_tokens.shape[0]} pseudo-token rows")
        th = self._host_tokens(text)
        where = (th[0] == int(split_ind)).nonzero()
        if where.numel() == 0:
            raise IndexError("split token not present in text[0]")
        ins = int(where[0])
        if ins + 3 > self.context_length:
            raise RuntimeError("no room for 3 pseudo tokens after the split token")
        eot = self._eot_columns(th)
        if bool(((eot >= ins) & (eot < ins + 3)).any()):
            raise IndexError("the EOT token lies inside the overwritten span")
        L = self.context_length
        squeezed = torch.zeros_like(text)
        squeezed[:, :ins + 1] = text[:, :ins + 1]
        squeezed[:, ins + 1:L - 2] = text[:, ins + 3:]
        return self._run_text(squeezed, eot, img_tokens, ins, normalize)

    def get_text_tokens(self, text):
        """model.py:592-605.  text int [B, L] -> (ln_final(tokens after the last block) [B, L, width] over ALL L columns, in the
        model's dtype; collect_ind int64 = (text == end_id).nonzero()[:, 1], the column of every EOT token).  No projection."""
        eng = self._engine()
        if text.dim() != 2 or text.shape[1] != self.context_length:
            raise RuntimeError(f"expected tokens [B,{self.context_length}], got {tuple(text.shape)}")
        th = self._host_tokens(text)
        collect_ind = (th == self.end_id).nonzero()[:, 1].to(eng.device)
        B, L, W = text.shape[0], self.context_length, self.transformer_width
        dt = self.dtype
        if dt not in _OUT_TYPE:
            raise RuntimeError(f"token outputs come as fp32, fp16 or bf16, not {dt}")
        if B == 0:
            return torch.empty((0, L, W), dtype=dt, device=eng.device), collect_ind
        return self._text_tokens(text, eng), collect_ind

    def _text_tokens(self, text, eng):
        B, L, W = text.shape[0], self.context_length, self.transformer_width
        if self.precision == "fp32x3":                       # (see encode_image: the planes of one call stay below 2 GiB)
            chunk = x3_chunk(W, L)
            if B > chunk:
                return torch.cat([self._text_tokens(text[i:i + chunk], eng) for i in range(0, B, chunk)])
        lib = load()
        tok = text.to(eng.device, dtype=torch.int32).contiguous()           # (ids were range-checked on the host: _host_tokens)

        def run(eng):
            nbytes = lib.keds_text_workspace_bytes(C.byref(eng.text), B)
            ws = self._ws.get(nbytes, eng.device)
            out = torch.empty((B, L, W), dtype=self.dtype, device=eng.device)
            check(lib.keds_text_run_tokens(C.byref(eng.text), ptr(tok), B, ptr(out), _OUT_TYPE[self.dtype], ptr(ws), ws.numel(),
                                           stream()), "keds_text_run_tokens")
            return out
        return self._guarded(run)

    def forward(self, image, text, extra=False):
        """model.py:894-911 (extra=True is broken in the reference: undefined encode_text_extra)."""
        if extra:
            raise NotImplementedError("extra text tower is not part of the retrieval path")
        if image is None:
            return self.encode_text(text)
        if text is None:
            return self.encode_image(image)
        return self.encode_image(image, normalize=True), self.encode_text(text, normalize=True), self.logit_scale.exp()


# ---------------------------------------------------------------------------------------------------
# knowledge-injection modules
# ---------------------------------------------------------------------------------------------------
class _RangeFlag:
    """The device int32 an fp16 knowledge call raises when a value it stores as fp16 lies beyond +-65504 or is not finite
    (keds_knowledge_f16.h, range_flag); one per owner, made on first use."""

    def __init__(self):
        self.flag: Optional[torch.Tensor] = None

    def get(self, device) -> torch.Tensor:
        if self.flag is None or self.flag.device != torch.device(device):
            self.flag = torch.zeros(1, dtype=torch.int32, device=device)
        return self.flag

    def tripped(self) -> bool:
        """Read and clear (synchronises with the device)."""
        if self.flag is None:
            return False
        hit = bool(self.flag.item())
        if hit:
            self.flag.zero_()
        return hit


def _check_module_precision(precision):
    if precision not in (None, "bf16", "fp16"):
        raise ValueError("precision must be None, 'bf16' or 'fp16'")
    return precision == "fp16"


class IM2TEXT(nn.Module):
    """model.py:105-123: (Linear, Dropout, ReLU) x n_layer then fc_out; eval-mode forward on HIP."""

    def __init__(self, embed_dim=512, middle_dim=512, output_dim=512, n_layer=2, dropout=0.1):
        super().__init__()
        if not 1 <= n_layer <= 4:
            raise ValueError("n_layer must be in [1,4]")
        self.fc_out = nn.Linear(middle_dim, output_dim)
        layers, dim = [], embed_dim
        for _ in range(n_layer):
            layers.append(nn.Sequential(nn.Linear(dim, middle_dim), nn.Dropout(dropout), nn.ReLU()))
            dim = middle_dim
        self.layers = nn.Sequential(*layers)
        self.embed_dim, self.middle_dim, self.output_dim, self.n_layer = embed_dim, middle_dim, output_dim, n_layer
        self._packed = None
        self._ws = _lib.Workspace()
        self._range = _RangeFlag()

    def _apply(self, fn, *a, **k):
        self._packed = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        self._packed = None
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def params(self, f32: bool = False, f16: bool = False) -> _lib.Im2TextParams:
        """f32: the weights as fp32 arrays (the fp32-accurate flow, keds_knowledge_run_f32); f16: as fp16 arrays, the fp32 masters
        rounded as convert_weights rounds them (keds_knowledge_run_f16); default bf16 GEMM operands."""
        _lib.require_gpu()
        if not self.fc_out.weight.is_cuda:
            raise RuntimeError("keds_amd.IM2TEXT: move the module to the GPU first; no CPU path exists")
        if self._packed is None:
            self._packed = {}
        if f16:
            f32 = "fp16"                                                      # the third weight set's key
        if f32 not in self._packed:
            keep = []
            wcast = _f16 if f16 else _f32 if f32 else _bf16
            p = _lib.Im2TextParams()
            p.dim_in, p.middle, p.dim_out, p.n_layer = self.embed_dim, self.middle_dim, self.output_dim, self.n_layer
            for i, blk in enumerate(self.layers):
                w, b = wcast(blk[0].weight), _f32(blk[0].bias)
                keep += [w, b]
                p.w[i], p.b[i] = ptr(w), ptr(b)
            ow, ob = wcast(self.fc_out.weight), _f32(self.fc_out.bias)
            keep += [ow, ob]
            p.out_w, p.out_b = ptr(ow), ptr(ob)
            self._packed[f32] = (p, keep)
        _lib.ensure_gemm_workspace(self.fc_out.weight.device)
        return self._packed[f32][0]

    def range_tripped(self) -> bool:
        """True when an fp16 forward since the last call stored a value beyond the fp16 range; reads and clears (synchronises)."""
        return self._range.tripped()

    def forward(self, x: torch.Tensor, precision: Optional[str] = None):
        """precision "fp16": every GEMM operand and the hidden rows in fp16 (keds_im2text_forward_f16; range_tripped() tells whether a
        value left the fp16 range); None or "bf16": the bf16 forward."""
        if self.training:
            raise RuntimeError("keds_amd.IM2TEXT runs the eval-mode forward only (dropout = identity); call .eval()")
        f16 = _check_module_precision(precision)
        p = self.params(f16=f16)
        lib = load()
        shape = x.shape
        x2 = x.reshape(-1, shape[-1]).to(dtype=torch.float32).contiguous()
        rows = x2.shape[0]
        nbytes = lib.keds_im2text_workspace_bytes(C.byref(p), rows)
        ws = self._ws.get(nbytes, x2.device)
        out = torch.empty((rows, self.output_dim), dtype=torch.float32, device=x2.device)
        if f16:
            check(lib.keds_im2text_forward_f16(C.byref(p), ptr(x2), rows, ptr(out), ptr(ws), ws.numel(), ptr(self._range.get(x2.device)),
                                               stream()), "keds_im2text_forward_f16")
        else:
            check(lib.keds_im2text_forward(C.byref(p), ptr(x2), rows, ptr(out), ptr(ws), ws.numel(), stream()),
                  "keds_im2text_forward")
        return out.reshape(*shape[:-1], self.output_dim).to(x.dtype)


class CrossAttention(nn.Module):
    """Parameter holder for one layer (model.py:37-54)."""

    def __init__(self, q_dim, k_dim, v_dim, heads=8, dim_head=64, dropout=0.):
        super().__init__()
        if dim_head != 64:
            raise ValueError("the HIP cross-attention core is built for dim_head = 64")
        inner = dim_head * heads
        self.heads = heads
        self.to_q = nn.Linear(q_dim, inner, bias=True)
        self.to_k = nn.Linear(k_dim, inner, bias=True)
        self.to_v = nn.Linear(v_dim, inner, bias=True)
        self.to_out = nn.Sequential(nn.Linear(inner, q_dim), nn.Dropout(dropout))


class CrossFormer(nn.Module):
    """model.py:81-101: q chained through `num_layers` CrossAttention layers, k and v fixed.  q may hold any number of query rows per
    sample and k, v up to MAX_KEYS = 288 rows (KEDS_CROSS_SEQ_MAX_KEYS); dim_head = 64 and q_dim == k_dim == v_dim."""

    MAX_KEYS = 288

    def __init__(self, q_dim, k_dim, v_dim, num_layers=1, heads=8, dim_head=64, dropout=0.):
        super().__init__()
        if not (q_dim == k_dim == v_dim):
            raise ValueError("the HIP path needs q_dim == k_dim == v_dim")
        self._num_layers, self.dim, self.heads = num_layers, q_dim, heads
        self.cross_layers = nn.ModuleList([CrossAttention(q_dim, k_dim, v_dim, heads, dim_head, dropout)
                                           for _ in range(num_layers)])
        self._packed = self._packed32 = self._packed16 = None
        self._ws = _lib.Workspace()
        self._range = _RangeFlag()

    def _apply(self, fn, *a, **k):
        self._packed = self._packed32 = self._packed16 = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        self._packed = self._packed32 = self._packed16 = None
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def params(self, f32: bool = False, f16: bool = False) -> _lib.CrossFormerParams:
        """f32: the per-layer weights as fp32 arrays, nothing fused (keds_knowledge_run_f32); f16: fp16 arrays, fused by
        keds_crossformer_fuse_f16 (keds_knowledge_run_f16); default bf16 GEMM operands."""
        _lib.require_gpu()
        if not self.cross_layers[0].to_q.weight.is_cuda:
            raise RuntimeError("keds_amd.CrossFormer: move the module to the GPU first; no CPU path exists")
        slot, cast = ("_packed16", _f16) if f16 else ("_packed32", _f32) if f32 else ("_packed", _bf16)
        f32 = f32 and not f16
        if getattr(self, slot, None) is None:
            keep = []
            arr = (_lib.CrossLayerParams * self._num_layers)()
            for i, l in enumerate(self.cross_layers):
                t = dict(wq=cast(l.to_q.weight), wk=cast(l.to_k.weight), wv=cast(l.to_v.weight), wo=cast(l.to_out[0].weight),
                         bq=_f32(l.to_q.bias), bk=_f32(l.to_k.bias), bv=_f32(l.to_v.bias), bo=_f32(l.to_out[0].bias))
                for k, v in t.items():
                    setattr(arr[i], k, ptr(v))
                keep.append(t)
            p = _lib.CrossFormerParams(self.dim, self.heads, self._num_layers, arr, None)
            # launch-saving re-arrangement of the 16-bit weights (keds_hip.h, keds_crossformer_fused): one k/v GEMM for all layers,
            # and every later layer's query projection folded with the previous output projection
            if not f32 and self._num_layers <= 8:
                lib = load()
                dev = self.cross_layers[0].to_q.weight.device
                buf = torch.empty(int(lib.keds_crossformer_fused_bytes(C.byref(p))), dtype=torch.uint8, device=dev)
                fused = _lib.CrossFormerFused()
                fuse = "keds_crossformer_fuse_f16" if f16 else "keds_crossformer_fuse"
                check(getattr(lib, fuse)(C.byref(p), ptr(buf), buf.numel(), C.byref(fused), stream()), fuse)
                torch.cuda.current_stream().synchronize()
                p.fused = C.pointer(fused)
                keep += [buf, fused]
            setattr(self, slot, (p, keep, arr))
        if not f32:
            _lib.ensure_gemm_workspace(self.cross_layers[0].to_q.weight.device)
        return getattr(self, slot)[0]

    def range_tripped(self) -> bool:
        """True when an fp16 forward since the last call stored a value beyond the fp16 range; reads and clears (synchronises)."""
        return self._range.tripped()

    def forward(self, q, k, v, precision: Optional[str] = None):
        """q [B,Lq,D], k [B,Lk,D], v [B,Lk,D] -> [B,Lq,D] in q's dtype; 1 <= Lk <= 288 (MAX_KEYS), dim_head = 64.
        precision "fp16": the single-query shape (Lq == 1, Lk <= 32) with fp16 operands and intermediates
        (keds_crossformer_forward_f16); the sequence form is built in bf16 only and refuses it.

        One query over at most 32 keys (the neighbour streams of eval_utils.py:661-672) is the single-query call,
        keds_crossformer_forward; every other shape -- one query over the 77 text tokens (the late fusion of eval_utils.py:249), a
        token sequence as queries (model.py:343-371) -- is keds_crossformer_forward_seq, whose attention runs on the matrix
        instruction.  There is no CPU path."""
        f16 = _check_module_precision(precision)
        if f16 and not (q.dim() == 3 and q.shape[1] == 1 and k.dim() == 3 and k.shape[1] <= 32):
            raise ValueError("precision 'fp16' is built for one query over at most 32 keys; the sequence form is bf16")
        p = self.params(f16=f16)
        if q.dim() != 3 or q.shape[1] < 1 or q.shape[2] != self.dim:
            raise RuntimeError("q must be [B,Lq,D] with Lq >= 1")
        if k.dim() != 3 or k.shape != v.shape or k.shape[0] != q.shape[0] or k.shape[2] != self.dim or k.shape[1] < 1:
            raise RuntimeError("k and v must both be [B,Lk,D] with Lk >= 1")
        B, Lq, K = q.shape[0], q.shape[1], k.shape[1]
        if K > self.MAX_KEYS:
            raise ValueError(f"the HIP CrossFormer attends over at most {self.MAX_KEYS} keys per sample, got {K}")
        lib = load()
        qf = q.to(dtype=torch.float32).contiguous()
        kf = k.to(dtype=torch.float32).contiguous()
        vf = kf if v is k else v.to(dtype=torch.float32).contiguous()
        out = torch.empty((B, Lq, self.dim), dtype=torch.float32, device=qf.device)
        if f16:
            nbytes = lib.keds_crossformer_workspace_bytes(C.byref(p), B, K)
            ws = self._ws.get(nbytes, qf.device)
            check(lib.keds_crossformer_forward_f16(C.byref(p), ptr(qf), ptr(kf), ptr(vf), B, K, ptr(out), ptr(ws), ws.numel(),
                                                   ptr(self._range.get(qf.device)), stream()), "keds_crossformer_forward_f16")
        elif Lq == 1 and K <= 32:
            nbytes = lib.keds_crossformer_workspace_bytes(C.byref(p), B, K)
            ws = self._ws.get(nbytes, qf.device)
            check(lib.keds_crossformer_forward(C.byref(p), ptr(qf), ptr(kf), ptr(vf), B, K, ptr(out), ptr(ws), ws.numel(),
                                               stream()), "keds_crossformer_forward")
        else:
            nbytes = lib.keds_crossformer_seq_workspace_bytes(C.byref(p), B, Lq, K)
            ws = self._ws.get(nbytes, qf.device)
            check(lib.keds_crossformer_forward_seq(C.byref(p), ptr(qf), ptr(kf), ptr(vf), B, Lq, K, ptr(out), ptr(ws), ws.numel(),
                                                   stream()), "keds_crossformer_forward_seq")
        return out.to(q.dtype)


class KnowledgeStream:
    """One stream (img2text + retrieval_fuse + text_condition) fused into a single library call
    (eval_utils.py:661-672): tokens = [fuse(m,I,I), cond(m,T,T), m]."""

    def __init__(self, img2text: IM2TEXT, retrieval_fuse: CrossFormer, text_condition: CrossFormer):
        self.img2text, self.retrieval_fuse, self.text_condition = img2text, retrieval_fuse, text_condition
        self._ws = _lib.Workspace()
        self._range = _RangeFlag()

    def range_tripped(self) -> bool:
        """True when a precision="fp16" call since the last look stored an fp16 value beyond +-65504 or a non-finite one (its tokens
        then hold inf or NaN: re-run on "fp32").  Reads and clears the stream's device flag; synchronises."""
        return self._range.tripped()

    def __call__(self, q: torch.Tensor, nbr_img: torch.Tensor, nbr_txt: torch.Tensor, precision: str = "bf16") -> torch.Tensor:
        """precision "fp32": the fp32-accurate flow (no operand rounding, keds_knowledge_run_f32) -- what
        compose_query_features passes when the CLIP model is on set_precision("fp32").  "fp16": every GEMM operand and 16-bit
        intermediate in fp16 (keds_knowledge_run_f16), the reference's converted modules; see range_tripped()."""
        f32, f16 = precision in ("fp32", "fp32x3"), precision == "fp16"
        kp = _lib.KnowledgeParams(self.img2text.params(f32, f16), self.retrieval_fuse.params(f32, f16),
                                  self.text_condition.params(f32, f16))
        lib = load()
        B, K, dim = nbr_img.shape
        qf = q.to(dtype=torch.float32).contiguous()
        ni = nbr_img.to(dtype=torch.float32).contiguous()
        nt = nbr_txt.to(dtype=torch.float32).contiguous()
        size, run = (("keds_knowledge_f32_workspace_bytes", "keds_knowledge_run_f32") if f32 else
                     ("keds_knowledge_f16_workspace_bytes", "keds_knowledge_run_f16") if f16 else
                     ("keds_knowledge_workspace_bytes", "keds_knowledge_run"))
        ws = self._ws.get(getattr(lib, size)(C.byref(kp), B, K), qf.device)
        out = torch.empty((B, 3, dim), dtype=torch.float32, device=qf.device)
        flag = (ptr(self._range.get(qf.device)),) if f16 else ()             # the fp16 entry takes range_flag in front of the stream
        check(getattr(lib, run)(C.byref(kp), ptr(qf), ptr(ni), ptr(nt), B, K, ptr(out), ptr(ws), ws.numel(), *flag, stream()), run)
        return out


# ---------------------------------------------------------------------------------------------------
# builders (model.py:927-991)
# ---------------------------------------------------------------------------------------------------
def convert_weights(model: nn.Module):
    """fp16 cast of Linear/Conv/MHA/projection weights (model.py:927-948).  Kept for API parity: it
    changes the checkpoint dtype (`model.dtype`) and rounds the stored weights to fp16; the GEMM operand types are those of
    the operating point (`CLIP.set_precision`), not of the checkpoint."""
    def _cast(l):
        if isinstance(l, (nn.Conv1d, nn.Conv2d, nn.Linear)):
            l.weight.data = l.weight.data.half()
            if l.bias is not None:
                l.bias.data = l.bias.data.half()
        if isinstance(l, nn.MultiheadAttention):
            for attr in ["in_proj_weight", "q_proj_weight", "k_proj_weight", "v_proj_weight", "in_proj_bias",
                         "bias_k", "bias_v"]:
                t = getattr(l, attr, None)
                if t is not None:
                    t.data = t.data.half()
        for name in ("text_projection", "proj"):
            t = getattr(l, name, None)
            if isinstance(t, torch.Tensor):
                t.data = t.data.half()
    model.apply(_cast)
    if hasattr(model, "repack"):
        model.repack()


def clip_config_from_state_dict(state_dict: Dict[str, torch.Tensor]) -> Dict[str, int]:
    if "visual.proj" not in state_dict:
        raise NotImplementedError("only ViT visual towers are supported")
    vw = state_dict["visual.conv1.weight"].shape[0]
    patch = state_dict["visual.conv1.weight"].shape[-1]
    grid = round((state_dict["visual.positional_embedding"].shape[0] - 1) ** 0.5)
    tw = state_dict["ln_final.weight"].shape[0]
    return dict(
        embed_dim=state_dict["text_projection"].shape[1], image_resolution=patch * grid,
        vision_layers=len([k for k in state_dict if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")]),
        vision_width=vw, vision_patch_size=patch, context_length=state_dict["positional_embedding"].shape[0],
        vocab_size=state_dict["token_embedding.weight"].shape[0], transformer_width=tw, transformer_heads=tw // 64,
        transformer_layers=len(set(k.split(".")[2] for k in state_dict if k.startswith("transformer.resblocks"))))


def build_model(state_dict: dict, fp16: bool = True) -> CLIP:
    """Infer the architecture from checkpoint shapes and load it (model.py:951-991)."""
    cfg = clip_config_from_state_dict(state_dict)
    model = CLIP(**cfg)
    sd = {k: v for k, v in state_dict.items() if k not in ("input_resolution", "context_length", "vocab_size")}
    if fp16:
        convert_weights(model)
    model.load_state_dict(sd)
    return model.eval()


def convert_models_to_fp32(model: nn.Module):
    """utils.py:44-48 (`--precision amp|fp32`)."""
    for p in model.parameters():
        p.data = p.data.float()
    if hasattr(model, "repack"):
        model.repack()
