"""Cost of the token-level tower outputs at B = 128, ViT-L/14 (seed-7 synthetic weights), precision "bf16".

Times with device events (warm-up, then --iters timed calls, median per call):
  encode_image                         the pooled features only (keds_vit_run: CLS-only last block)
  mid_feature fp32 / fp16 taps         encode_image(mid_feature=True): 24 taps [128, 257, 1024] + features, plain and
                                       non-temporal tap stores (keds_tap_store_nt: the A/B the store policy was chosen by)
  get_tokens                           VisualTransformer.get_tokens: the last block's tokens only
  encode_text / get_text_tokens        B = 128 captions (77 columns)
Prints one JSON line per measurement and a summary with the ratios.  For the tap kernel's own time and bytes/s run
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/bench_tokens.py --only taps
and divide the bytes of one tap (128 x 257 x 1024 x (2 read + 4 or 2 written)) by the cast_rows_kernel rows of the stats.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import keds_amd  # noqa: E402
from keds_amd import _lib  # noqa: E402
from oracle import keds_oracle as O  # noqa: E402

VITL = dict(embed_dim=768, image_resolution=224, vision_layers=24, vision_width=1024, vision_patch_size=14,
            context_length=77, vocab_size=49408, transformer_width=768, transformer_layers=12)


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", choices=["all", "taps"], default="all", help="taps: the fp32 / fp16 tap passes only (profiler runs)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    sd = O.synth_clip_state_dict(**VITL, seed=7)
    m = keds_amd.build_model(dict(sd), fp16=False).cuda()
    B = args.batch
    img = torch.from_numpy(np.random.RandomState(0).standard_normal((B, 3, 224, 224)).astype(np.float32)).cuda()
    text = O.synth_tokens(B, seed=4004).cuda()
    lib = _lib.load()
    m.encode_image(img)
    m.numerics_sync()
    res = {}

    def put(name, fn):
        med, best = timed(fn, args.warmup, args.iters)
        res[name] = med
        print(json.dumps({"case": name, "B": B, "median_ms": round(med, 4), "min_ms": round(best, 4), "iters": args.iters}), flush=True)

    def taps_f16():
        # the same pass with fp16 taps (the façade returns the model's dtype: the library call directly)
        eng = m._engine()
        ws = m._ws.get(lib.keds_vit_workspace_bytes(eng.vit, B), eng.device)
        _lib.check(lib.keds_vit_run_tokens(eng.vit, _lib.ptr(img), B, _lib.ptr(out), 0, _lib.ptr(t16), None, 2, _lib.ptr(ws),
                                           ws.numel(), _lib.stream()), "keds_vit_run_tokens")

    out = torch.empty((B, 768), device="cuda")
    t16 = torch.empty((24, B, 257, 1024), dtype=torch.float16, device="cuda")
    if args.only == "taps":
        put("mid_feature.fp32_taps.plain", lambda: m.encode_image(img, mid_feature=True))
        put("mid_feature.fp16_taps.plain", taps_f16)
        lib.keds_tap_store_nt(1)
        put("mid_feature.fp32_taps.nt", lambda: m.encode_image(img, mid_feature=True))
        put("mid_feature.fp16_taps.nt", taps_f16)
        lib.keds_tap_store_nt(0)
        return
    put("encode_image", lambda: m.encode_image(img))
    for nt in (0, 1):
        lib.keds_tap_store_nt(nt)
        tag = "nt" if nt else "plain"
        put(f"mid_feature.fp32_taps.{tag}", lambda: m.encode_image(img, mid_feature=True))
        put(f"mid_feature.fp16_taps.{tag}", taps_f16)
    lib.keds_tap_store_nt(0)
    put("encode_image.again", lambda: m.encode_image(img))
    put("get_tokens", lambda: m.visual.get_tokens(img))
    put("encode_text", lambda: m.encode_text(text))
    put("get_text_tokens", lambda: m.get_text_tokens(text))
    enc = min(res["encode_image"], res["encode_image.again"])
    summary = {"summary": "ratios to encode_image (min of the two encode_image runs)", "encode_image_ms": round(enc, 4)}
    for k in ("mid_feature.fp32_taps.nt", "mid_feature.fp32_taps.plain", "mid_feature.fp16_taps.nt", "mid_feature.fp16_taps.plain",
              "get_tokens"):
        summary[k] = round(res[k] / enc, 4)
    summary["get_text_tokens_over_encode_text"] = round(res["get_text_tokens"] / res["encode_text"], 4)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
