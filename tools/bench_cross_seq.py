#!/usr/bin/env python3
"""Time keds_cross_attn_seq alone on one MI355X and write profiles/cross_seq_bench.txt.

    python tools/bench_cross_seq.py [--out profiles/cross_seq_bench.txt] [--iters 100]

Method: one device event pair (hipEvent, recorded on the launch stream) around every launch; warm-up runs in rounds of 20 timed
launches until the medians of two consecutive rounds agree within 5 % (at most 50 rounds, else the case is marked "unsettled"); then
the median of `--iters` launches.  An event pair is two marker packets on the stream, which a launch of a few microseconds feels,
so every case also reports "b2b": the same `--iters` launches back to back between ONE pair, divided by their number.
Bytes are the algorithmic ones: Q + out (B Lq 64 heads) and K + V (B Lk 64 heads), bf16, each touched once.

Shapes: B = 128, 8 heads, (Lq, Lk) in the table below.  For orientation only, at Lk <= 32 and Lq = 1 the single-query core
keds_cross_attn_core is timed in the same run on the same operands.  Nothing here is a gate."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keds_amd import _lib  # noqa: E402

SHAPES = ((1, 16), (1, 32), (1, 77), (1, 128), (77, 257), (257, 77), (257, 257))
B, HEADS = 128, 8
ROUND = 20


def _pairs(fn, n):
    """n launches, each inside its own event pair -> microseconds per launch"""
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [1e3 * a.elapsed_time(b) for a, b in evs]


def _b2b(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / n


def measure(fn, iters):
    prev, rounds, settled = None, 0, False
    while rounds < 50 and not settled:
        med = statistics.median(_pairs(fn, ROUND))
        settled = prev is not None and abs(med - prev) <= 0.05 * max(med, prev)
        prev = med
        rounds += 1
    t = _pairs(fn, iters)
    return dict(median_us=round(statistics.median(t), 2), min_us=round(min(t), 2), b2b_us=round(_b2b(fn, iters), 2), warm_rounds=rounds,
                settled=settled, iters=iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_seq_bench.txt"))
    ap.add_argument("--iters", type=int, default=100)
    args = ap.parse_args()
    _lib.require_gpu()
    lib = _lib.load()
    inner = 64 * HEADS
    g = torch.Generator().manual_seed(1)
    lines = [f"# tools/bench_cross_seq.py on one MI355X (device name '{torch.cuda.get_device_name(0)}'): keds_cross_attn_seq alone, B = {B}, {HEADS} heads, bf16; one device "
             f"event pair per launch, warm-up until two {ROUND}-launch medians agree within 5 %, median of {args.iters} launches; b2b = "
             f"{args.iters} launches between one pair / {args.iters}",
             f"# csrc_sha16 {_lib.source_digest()}   build flags '{_lib.build_flags()}'",
             "# bytes = (2 B Lq + 2 B Lk) x 64 heads x 2 (Q, out, K, V once each); GB/s over the median"]
    for Lq, Lk in SHAPES:
        q = (1.5 * torch.randn(B * Lq, inner, generator=g)).bfloat16().cuda()
        k = (1.5 * torch.randn(B * Lk, inner, generator=g)).bfloat16().cuda()
        v = (1.5 * torch.randn(B * Lk, inner, generator=g)).bfloat16().cuda()
        out = torch.empty(B * Lq, inner, dtype=torch.bfloat16, device="cuda")
        st = _lib.stream()

        def seq():
            rc = lib.keds_cross_attn_seq(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, Lq, Lk, HEADS, inner, inner, inner, st)
            if rc:
                raise RuntimeError(f"keds_cross_attn_seq failed ({rc}): {_lib.last_error()}")

        nbytes = (2 * B * Lq + 2 * B * Lk) * inner * 2
        rec = dict(case="cross_attn_seq", Lq=Lq, Lk=Lk, **measure(seq, args.iters))
        rec["MB"] = round(nbytes / 1e6, 3)
        rec["GBps"] = round(nbytes / rec["median_us"] / 1e3, 1)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if Lq == 1 and Lk <= 32:
            def core():
                rc = lib.keds_cross_attn_core(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, Lk, HEADS, inner, st)
                if rc:
                    raise RuntimeError(f"keds_cross_attn_core failed ({rc}): {_lib.last_error()}")

            rec = dict(case="cross_attn_core (yardstick)", Lq=Lq, Lk=Lk, **measure(core, args.iters))
            rec["MB"] = round(nbytes / 1e6, 3)
            rec["GBps"] = round(nbytes / rec["median_us"] / 1e3, 1)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
