#!/usr/bin/env python3
"""Time the knowledge stream's entries alone on one MI355X: what their host chains cost per call.

    python tools/bench_knowledge.py [--out profiles/knowledge_bench.txt] [--calls 200] [--repeats 5]

Method: wall clock over `--calls` back-to-back calls with ONE synchronisation at the end, divided by their number; the median, minimum
and maximum of `--repeats` such runs after two warm-up runs.  These passes are launch-latency bound, so the wall clock of the enqueue
loop is the quantity of interest: host overhead in a chain shows here and nowhere else.

Rows: KnowledgeStream on the bf16 fused path and on the fp32 path at B = 128, K = 16, dim 768, middle 512, two hidden layers, three
CrossFormer layers of 12 heads; CrossFormer.forward (three layers, 12 heads, dim 768, B = 128) at (Lq, Lk) = (1, 16), (1, 77), (257, 77).
Nothing here is a gate."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import keds_amd  # noqa: E402
from keds_amd import _lib  # noqa: E402

B, K, DIM, MIDDLE, HEADS, LAYERS = 128, 16, 768, 512, 12, 3
SEQ = ((1, 16), (1, 77), (257, 77))


def measure(fn, calls, repeats):
    runs = []
    for i in range(repeats + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        runs.append(1e6 * (time.perf_counter() - t0) / calls)
    runs = runs[2:]
    return dict(median_us=round(statistics.median(runs), 2), min_us=round(min(runs), 2), max_us=round(max(runs), 2), calls=calls, repeats=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knowledge_bench.txt"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    i2t = keds_amd.IM2TEXT(embed_dim=DIM, middle_dim=MIDDLE, output_dim=DIM, n_layer=2).eval().to(dev)
    fuse, cond = (keds_amd.CrossFormer(DIM, DIM, DIM, num_layers=LAYERS, heads=HEADS).eval().to(dev) for _ in range(2))
    stream = keds_amd.KnowledgeStream(i2t, fuse, cond)
    g = torch.Generator(device=dev).manual_seed(2)
    q, ni, nt = (torch.randn(*s, generator=g, device=dev) for s in ((B, DIM), (B, K, DIM), (B, K, DIM)))
    lines = [f"# tools/bench_knowledge.py on one MI355X (device name '{torch.cuda.get_device_name(0)}'): microseconds per call, wall clock over "
             f"{args.calls} back-to-back calls with one synchronisation at the end; median, min and max of {args.repeats} runs after two warm-up runs",
             f"# csrc_sha16 {_lib.source_digest()}   build flags '{_lib.build_flags()}'"]
    cases = [("KnowledgeStream bf16 fused", lambda: stream(q, ni, nt)), ("KnowledgeStream fp32", lambda: stream(q, ni, nt, precision="fp32"))]
    for Lq, Lk in SEQ:
        qs, ks = torch.randn(B, Lq, DIM, generator=g, device=dev), torch.randn(B, Lk, DIM, generator=g, device=dev)
        cases.append((f"CrossFormer.forward Lq={Lq} Lk={Lk}", lambda qs=qs, ks=ks: fuse(qs, ks, ks)))
    for name, fn in cases:
        lines.append(json.dumps(dict(case=name, **measure(fn, args.calls, args.repeats))))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
