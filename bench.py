#!/usr/bin/env python3
"""Headline benchmark: query-images/sec for (CLIP ViT-L/14 encode_image of B=128 synthetic 224x224
images) + (top-10 over a synthetic 0.5 M x 768 database), BASELINE.json `metric`, `configs[1]`.

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One process per GPU.  A "step" is one pass of the hot path over one batch: every rank encodes its own
128 images (data parallel, weights replicated), the query embeddings are all-gathered, every rank scans
ITS shard of the database rows for all 128*N queries, and the [B,k] partial results are all-gathered
and merged keyed on (distance, id) (weak scaling: per-GPU encoder work is fixed and every rank streams
one full database's worth of bytes per step).  Inputs are resident in HBM before the
timed region.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times --steps steps, writes the last step's outputs (--dump-outputs DIR) and
prints the headline line.  --full adds everything else this file measures and checks: per-kernel-class
hipEvents in the timed steps (roofline figures), the self-verification against the oracle, the legs of the
other BASELINE configurations and operating points, the measured Recall@k parity and the CPU baseline.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

VITL = dict(embed_dim=768, image_resolution=224, vision_layers=24, vision_width=1024, vision_patch_size=14,
            context_length=77, vocab_size=49408, transformer_width=768, transformer_heads=12, transformer_layers=12)

# GEMM work EXECUTED per ViT-L/14 image (SURVEY.md App. A shapes): patch embed + 24 x qkv + 23 x (out, fc, proj) on all
# 257 tokens + the last block's (out, fc, proj) on the CLS token only (nothing else is read after the last block,
# model.py:412; the reference computes those 256 unused rows) + read-out.  The reference-equivalent count
# (all 24 blocks on 257 tokens) is 77.77 GMAC; executed: 75.35 GMAC.
_PER_TOKEN_TAIL = 1024 * 1024 + 2 * 1024 * 4096                     # out-proj + fc + proj MACs per token
GEMM_MAC_PER_IMAGE = (256 * 588 * 1024 + 24 * 257 * 1024 * 3072 + 23 * 257 * _PER_TOKEN_TAIL + 1 * _PER_TOKEN_TAIL
                      + 1024 * 768)
PEAK_BF16_TFLOPS = 2500.0     # dense bf16 MFMA, MI355X_MICROARCH.md
PEAK_FP8_TFLOPS = 5000.0      # dense MX-fp8 MFMA (--precision fp8 only; the headline is bf16 / fp16)
PEAK_FP8_MEASURED_TFLOPS = 3400.0    # register-only v_mfma_scale_f32_16x16x128_f8f6f4 loop (profiles/r01_microbench.txt)
PEAK_BF16_MEASURED_TFLOPS = 2060.0   # tools/micro/mfma_peak.hip on the gpurun MI355X
PEAK_F32_TFLOPS = 157.3       # f32-input MFMA (--precision fp32 only), MI355X_MICROARCH.md
PEAK_F32_MEASURED_TFLOPS = 155.0     # MI355X_MICROARCH.md, Matrix cores table
PEAK_HBM_MEASURED_GBPS = 7150.0      # tools/micro/hbm_stream.hip (read-only)
PEAK_HBM_GBPS = 8000.0        # HBM3E spec, MI355X_MICROARCH.md


def evidence(kind):
    """Newest committed measurement file profiles/r<NN>_<kind>.json (by round number) -- only while it still describes THIS
    build: the file carries the digest of the kernel sources it was measured on (keds_amd._lib.source_digest, written by
    tools/parse_pmc.py / tools/update_parity_baseline.py) and is dropped when csrc/ or include/ changed since.  Returns
    (dict or None, note) where `note` names the file, its digest and -- when a .git is present -- the commit that last
    touched it.  (No .git travels to the GPU box, so staleness is decided by the digest, not by `git diff`.)"""
    import glob
    import re
    import subprocess
    from keds_amd import _lib
    best = None
    for f in glob.glob(os.path.join(ROOT, "profiles", f"r*_{kind}.json")):
        m = re.match(r"r(\d+)_" + re.escape(kind) + r"\.json$", os.path.basename(f))
        if m and (best is None or int(m.group(1)) > best[0]):
            best = (int(m.group(1)), f)
    if best is None:
        return None, f"no profiles/r*_{kind}.json committed"
    f = best[1]
    try:
        d = json.load(open(f))
    except Exception as e:                                            # noqa: BLE001
        return None, f"{os.path.basename(f)} unreadable ({e})"
    now = _lib.source_digest()
    name = "profiles/" + os.path.basename(f)
    commit = ""
    try:
        r = subprocess.run(["git", "-C", ROOT, "log", "-1", "--format=%h", "--", f], capture_output=True, text=True, timeout=10)
        if r.returncode == 0 and r.stdout.strip():
            commit = f", commit {r.stdout.strip()}"
    except Exception:                                                 # noqa: BLE001  (no git on the GPU box)
        pass
    if d.get("csrc_sha16") != now:
        return None, f"{name} is stale: measured on sources {d.get('csrc_sha16')}, this build is {now}{commit}"
    return d, f"{name} (sources {now}{commit})"


def pmc_traffic(kernel_key, batch, rows, world):
    """HBM bytes per launch of `kernel_key` from the committed PMC passes (tools/pmc_step.py + tools/parse_pmc.py:
    separate --pmc FETCH_SIZE and --pmc WRITE_SIZE runs of this same workload, FETCH_SIZE doubled per the gfx950
    rule of MI355X_MICROARCH.md).  Only valid for the configuration and the sources they were taken on; otherwise None.
    Returns (bytes or None, note)."""
    if batch != 128 or rows != 500000 or world != 1:
        return None, "PMC passes are of the 1-GPU B=128, 0.5 M-row configuration only"
    d, note = evidence("pmc_traffic")
    e = (d or {}).get(kernel_key)
    if not e:
        return None, note
    return e.get("hbm_read_bytes_per_launch", 0.0) + e.get("hbm_write_bytes_per_launch", 0.0), note


def recall_parity():
    """Recall@k parity with the reference's CPU path on identical inputs, from the newest committed parity file (measured by
    tests/test_gpu_fullsize.py on the reference-minted ViT-L/14 1k-gallery fixture); None when that file does not describe
    this build."""
    d, note = evidence("parity")
    if d is None:
        return None, note
    out = {}
    for key, label in (("recall_vitl14", "default (bf16/fp16 operands)"), ("recall_vitl14.fp32", "set_precision('fp32')")):
        r = d.get("other_metrics", {}).get(key)
        if r:
            ks = sorted(int(k[2:]) for k in r if k.startswith("R@"))
            out[label] = {"outcomes_flipped_of_%d" % (256 * len(ks)): r.get("outcomes_flipped_inside_tolerance"),
                          "recall": {f"R@{k}": r[f"R@{k}"] for k in ks}, "reference": {f"R@{k}": r[f"ref_R@{k}"] for k in ks}}
    return (out or None), note


def random_clip(device):
    """Random-init ViT-L/14 CLIP of the reference architecture (there are no checkpoints offline)."""
    import keds_amd
    torch.manual_seed(1234)
    with torch.device(device):
        model = keds_amd.CLIP(**VITL)
    with torch.no_grad():
        for blk in model.visual.transformer.resblocks:        # visual tower: same stds as the text tower init
            w, L = 1024, 24
            blk.attn.in_proj_weight.normal_(std=w ** -0.5)
            blk.attn.out_proj.weight.normal_(std=w ** -0.5 * (2 * L) ** -0.5)
            blk.mlp.c_fc.weight.normal_(std=(2 * w) ** -0.5)
            blk.mlp.c_proj.weight.normal_(std=w ** -0.5 * (2 * L) ** -0.5)
    return model.eval()


def cpu_threads():
    """Fixed thread count of the CPU baseline: one thread per physical core (half the logical CPUs of an SMT-2 host), at most
    128 -- oversubscribing a many-core host makes torch's CPU GEMMs slower, and a per-run pilot made the number wander
    (1.1-3.7 query-images/s over three driver runs of round 3)."""
    ncpu = os.cpu_count() or 1
    return max(1, min(ncpu // 2 if ncpu >= 16 else ncpu, 128))


def pin_host_threads(n):
    """Best effort: confine this process (and the oracle's OpenMP pool with it) to `n` hardware threads of ONE NUMA node, one per
    physical core, for the duration of the CPU leg -- on a two-socket host shared with other jobs most of the run-to-run spread of
    the oracle is threads migrating between sockets and onto busy SMT siblings.  Returns (previous affinity or None, the CPUs
    chosen or None); restore with os.sched_setaffinity(0, previous)."""
    try:
        allowed = sorted(os.sched_getaffinity(0))

        def cpulist(path):
            out = []
            for part in open(path).read().strip().split(","):
                a, _, b = part.partition("-")
                out += list(range(int(a), int(b or a) + 1))
            return out
        best = None
        import glob
        for node in sorted(glob.glob("/sys/devices/system/node/node[0-9]*")):
            cpus = [c for c in cpulist(node + "/cpulist") if c in allowed]
            cores, seen = [], set()
            for c in cpus:                                   # one hardware thread per physical core
                sib = tuple(cpulist(f"/sys/devices/system/cpu/cpu{c}/topology/thread_siblings_list"))
                if sib not in seen:
                    seen.add(sib)
                    cores.append(c)
            if best is None or len(cores) > len(best):
                best = cores
            if len(cores) >= n:
                best = cores
                break
        if not best or len(best) < max(2, n // 2):
            return None, None
        chosen = best[:n]
        os.sched_setaffinity(0, chosen)
        return allowed, chosen
    except Exception:                                         # noqa: BLE001  (no sysfs, no permission: run unpinned)
        return None, None


def _vit_sd(model):
    sd = {k_: v.detach().float().cpu() for k_, v in model.state_dict().items() if k_.startswith("visual.")}
    for k_ in ("text_projection", "positional_embedding", "token_embedding.weight", "ln_final.weight"):
        sd[k_] = model.state_dict()[k_].detach().float().cpu()   # arch inference reads their shapes only
    return sd


CPU_WARMUP_CAP = 5
CPU_SAMPLE_SEED, CPU_SAMPLE_IMAGES = 1, 8     # the images the CPU leg encodes; the GPU path encodes the SAME ones for `verification`


def cpu_baseline(model, n_db, dim, k):
    """Oracle (CPU restatement, fp32 torch) timed on this host's cores on a bounded sample, per BASELINE.md section 2.
    The setting is the one that MAXIMISES the oracle's throughput on this box: a pilot times ONE ViT-L/14 block (1/24 of an
    image's encoder work) at batch in {8, 32} x threads in {32, 64, one per physical core}, the best (batch, threads) is kept
    and reported, and the whole encoder is timed at it.  The timed runs start only when the host has SETTLED: warm-up
    passes repeat until two consecutive ones agree within 5 % (at most CPU_WARMUP_CAP; round 5's single warm-up left a
    monotone 0.49 -> 0.39 s/image drift in the timed runs: thread pool, page faults of the 1.2 GB of weights and the clock
    governor were still moving), then the median of 7 runs (of 3 when a run takes more than 8 s).  Plus 128 queries against a
    65,536-row slice scaled to n_db rows.  Returns (record, oracle embeddings of the first CPU_SAMPLE_IMAGES images, unit
    norm) -- the latter feed the bench line's self-verification.

    Why a fraction of the host threads wins: the oracle's GEMMs are [B*257, 1024] x [1024, 1024..4096] -- at batch 8 that is
    2,056 rows, a few hundred 2-D blocks of the CPU BLAS; past ~32 threads the per-thread block is too small to amortise the
    fork/join and the cross-socket traffic of a 2-socket host (the pilot table in `setting` shows it: the per-image time of
    one block RISES with the thread count).  `cores` is the thread count actually used."""
    import statistics
    from oracle import keds_oracle as O
    ncpu = os.cpu_count() or 1
    phys = cpu_threads()
    sd = _vit_sd(model)
    gen = torch.Generator().manual_seed(CPU_SAMPLE_SEED)
    img_all = torch.randn(32, 3, 224, 224, generator=gen)        # the first CPU_SAMPLE_IMAGES rows are the verification sample
    pilot = {}
    with torch.no_grad():
        for threads in sorted({min(32, phys), min(64, phys), phys}):
            torch.set_num_threads(threads)
            for nb in (8, 32):
                x = torch.randn(nb, 257, 1024, generator=torch.Generator().manual_seed(5))
                O.residual_block(x, sd, "visual.transformer.resblocks.0.", 16, False)        # warm-up of this shape / pool
                ts = []
                for _ in range(2):
                    t0 = time.perf_counter()
                    O.residual_block(x, sd, "visual.transformer.resblocks.0.", 16, False)
                    ts.append((time.perf_counter() - t0) / nb)
                pilot[(nb, threads)] = min(ts)
        (nb, threads), _ = min(pilot.items(), key=lambda kv: kv[1])
        torch.set_num_threads(threads)
        prev_aff, pinned = pin_host_threads(threads)
        img = img_all[:nb]

        def one():
            t0 = time.perf_counter()
            r = O.encode_image(sd, img)
            return (time.perf_counter() - t0) / nb, r
        warm = []
        w, ref = one()                                            # also the verification reference
        warm.append(w)
        while len(warm) < CPU_WARMUP_CAP:
            w, _ = one()
            warm.append(w)
            if abs(warm[-1] - warm[-2]) <= 0.05 * min(warm[-1], warm[-2]):
                break
        settled = len(warm) >= 2 and abs(warm[-1] - warm[-2]) <= 0.05 * min(warm[-1], warm[-2])
        # 7 timed runs (3 when a run takes more than 8 s); the median is the value, and the spread is quoted over the middle five:
        # the host is shared with other jobs of the pool and a single run caught by a neighbour's burst says nothing about this code
        ts = [one()[0] for _ in range(7 if warm[-1] * nb <= 8.0 else 3)]
        t_img = statistics.median(ts)
        rows = 65536
        db = torch.nn.functional.normalize(torch.randn(rows, dim, generator=torch.Generator().manual_seed(2)), dim=1)
        q = torch.nn.functional.normalize(torch.randn(128, dim, generator=torch.Generator().manual_seed(3)), dim=1)
        O.flat_l2_search_f32(db, q, k)
        tq = []
        for _ in range(5):
            t0 = time.perf_counter()
            O.flat_l2_search_f32(db, q, k)
            tq.append((time.perf_counter() - t0) / q.shape[0] * (n_db / rows))
        t_q = statistics.median(tq)
        if prev_aff is not None:
            os.sched_setaffinity(0, prev_aff)
    mid = sorted(ts)[1:-1] if len(ts) >= 7 else ts
    spread = (max(mid) - min(mid)) / t_img
    spread_all = (max(ts) - min(ts)) / t_img
    rec = {"value": 1.0 / (t_img + t_q), "unit": "query-images/sec", "cores": threads, "kind": "port",
           "setting": {"batch": nb, "threads": threads, "host_threads": ncpu, "physical_cores_assumed": phys,
                       "pinned_to_cpus": (f"{pinned[0]}..{pinned[-1]} ({len(pinned)} hardware threads of one NUMA node, one per core)" if pinned else None),
                       "pilot_ms_per_image_of_one_block": {f"B{b}xT{t}": round(v * 1e3, 2) for (b, t), v in sorted(pilot.items())}},
           "warmup_s_per_image": [round(t, 3) for t in warm], "settled_within_5pct": bool(settled),
           "runs_s_per_image": [round(t, 3) for t in ts], "spread_over_median": round(spread, 3),
           "spread_is": "(max - min) / median over the middle five of seven runs" if len(ts) >= 7 else "(max - min) / median",
           "spread_all_runs_over_median": round(spread_all, 3),
           "sample": f"oracle fp32 at the fastest of six (batch, threads) settings (pilot: one ViT-L/14 block each): batch {nb}, "
                     f"{threads} of {ncpu} host threads ({phys} physical cores assumed; more threads are slower on this shape, see "
                     f"setting.pilot), {len(warm)} warm-up passes (until two agree within 5 %) + median of {len(ts)}: {nb} images "
                     f"through ViT-L/14 ({t_img:.2f} s/image; runs {', '.join(f'{t:.2f}' for t in ts)}) "
                     f"+ 128 queries x {rows}-row slice scaled to {n_db} rows ({t_q * 1e3:.2f} ms/query, median of 5)"}
    return rec, (img_all[:CPU_SAMPLE_IMAGES], torch.nn.functional.normalize(ref[:CPU_SAMPLE_IMAGES], dim=1))


def synth_tokens(batch, context_length=77, seed=4004, sot=49406, eot=49407, star=265):
    """'a photo of * , <filler>' token rows: SOT 320 1125 539 * 267 filler... EOT 0..., the EOT column
    varying per row in [8, 40]."""
    import numpy as np
    rs = np.random.RandomState(seed)
    out = np.zeros((batch, context_length), dtype=np.int64)
    for b in range(batch):
        e = 8 + int(rs.randint(0, 33))
        row = [sot, 320, 1125, 539, star, 267] + list(rs.randint(300, 40000, size=e - 6)) + [eot]
        out[b, :len(row)] = row
    return torch.from_numpy(out)


def cpu_baseline_dual(model, s_img, s_txt, n_db, dim):
    """Oracle (CPU restatement, fp32 torch) of the dual-stream composed query on a bounded sample: 2 queries through
    compose_query (ViT-L/14 + two knowledge streams + two text passes) against two 65,536-row database slices; the
    two scans are scaled to n_db rows, the rest is per query."""
    from oracle import keds_oracle as O
    ncpu = os.cpu_count() or 1
    threads = cpu_threads()
    torch.set_num_threads(threads)
    sd = {k_: v.detach().float().cpu() for k_, v in model.state_dict().items()}
    streams = []
    for st in (s_img, s_txt):
        streams.append(tuple({k_: v.detach().float().cpu() for k_, v in m.state_dict().items()}
                             for m in (st.img2text, st.retrieval_fuse, st.text_condition)))
    rows = 65536
    g = torch.Generator().manual_seed(2)
    ib = torch.nn.functional.normalize(torch.randn(rows, dim, generator=g), dim=1)
    tb = torch.nn.functional.normalize(torch.randn(rows, dim, generator=g), dim=1)
    img = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(1))
    tok = synth_tokens(2)
    with torch.no_grad():
        t0 = time.perf_counter()
        ref = O.compose_query(sd, streams[0], streams[1], img, tok, ib, tb)
        t_all = (time.perf_counter() - t0) / 2
        q = torch.nn.functional.normalize(torch.randn(128, dim, generator=torch.Generator().manual_seed(3)), dim=1)
        t0 = time.perf_counter()
        O.flat_l2_search_f32(ib, q, 16)
        t_scan = (time.perf_counter() - t0) / 128                  # one database slice, per query
    t_query = t_all + 2.0 * t_scan * (n_db / rows - 1.0)
    # the SAME two queries against the SAME two slices through the timed path: neighbours equal, composed features within the
    # operating point's stated tolerance (the dual line's self-verification; `ref` is the oracle's)
    import keds_amd
    dev = next(model.parameters()).device
    dbs = []
    for base in (ib, tb):
        ix = keds_amd.FlatIndex(dim, "l2", device=dev)
        ix.add(base.to(dev))
        dbs.append(ix)
    got = keds_amd.compose_query_features(model, s_img, s_txt, img.to(dev), tok.to(dev), [None, None, None, dbs[0], dbs[1]],
                                          id_split=265, verify=True)
    # (i) the search is exact for the query the timed path itself produced: its neighbours against the oracle's exact search with
    # THAT query (the oracle's own fp32 query may rank near-tied rows of a random database differently: reported, not asserted);
    # (ii) the composed features against the oracle's
    feat = torch.nn.functional.normalize(got["query_image_features"].float(), dim=1)
    _, ii, _ = dbs[0].search_gather(feat, 16, normalize=False)
    _, it, _ = dbs[1].search_gather(feat, 16, normalize=False)
    _, oi = O.flat_l2_search(ib, feat.cpu(), 16)
    _, ot = O.flat_l2_search(tb, feat.cpu(), 16)
    cos, rel = _cos_rel(got["mixture"].float().cpu(), ref["mixture"].float())
    check = {"queries": 2, "rows_per_database": rows,
             "neighbour_id_mismatches": int((ii.cpu() != torch.as_tensor(oi)).sum() + (it.cpu() != torch.as_tensor(ot)).sum()),
             "neighbours_differing_from_the_oracles_own_query": int((ii.cpu() != ref["topk_image_indices"]).sum() + (it.cpu() != ref["topk_text_indices"]).sum()),
             "mixture_min_cosine": cos, "mixture_rel_l2": rel,
             "checker": "oracle compose_query (fp32 torch CPU): the cpu_baseline leg's two queries and database slices through the timed path"}
    return {"value": 1.0 / t_query, "unit": "queries/sec", "cores": threads, "kind": "port",
            "sample": f"oracle fp32, {threads} of {ncpu} host threads: 2 composed queries against two {rows}-row slices "
                      f"({t_all:.2f} s/query), the two scans scaled to {n_db} rows (+{2.0 * t_scan * (n_db / rows - 1.0) * 1e3:.1f} ms/query)"}, check


def self_launch(gpus, argv):
    """`python bench.py --gpus N` (N > 1) outside torch.distributed.run: start the N ranks as a CHILD process
    (`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py
    <same arguments>`), relay its output and return its exit code.  Nothing in this parent has touched the GPU (no
    torch.cuda call, no library load), it never execs, and rank 0's JSON line is printed as the LAST stdout line
    whatever the ranks or RCCL print after it."""
    import socket
    import subprocess
    with socket.socket() as s:                                  # a free rendezvous port on the loopback interface
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC only on this pool (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    if os.environ.get("KEDS_BENCH_LAUNCH_DRYRUN") == "1":       # tests: show what would be started, start nothing
        print(json.dumps({"launch": cmd, "HSA_ENABLE_IPC_MODE_LEGACY": env["HSA_ENABLE_IPC_MODE_LEGACY"]}), flush=True)
        return 0
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, bufsize=1)
    result = None
    for line in proc.stdout:
        s = line.strip()
        if s.startswith("{") and '"metric"' in s:
            result = s                                          # held back: it must be the last line on stdout
        else:
            sys.stdout.write(line)
            sys.stdout.flush()
    rc = proc.wait()
    if result is not None:
        print(result, flush=True)
    return rc


# text-tower GEMM work per token row (12 blocks of width 768 on every row; the read-out projection is per sequence)
TEXT_MAC_PER_ROW = 12 * (768 * 2304 + 768 * 768 + 2 * 768 * 3072)


def build_database(keds_amd, shard_bounds, N, D, world, rank, dev, seed, sharded):
    """Seeded unit-norm rows, the same global stream on every rank; this rank keeps rows shard_bounds(N, world, rank)."""
    lo, hi = shard_bounds(N, world, rank)
    gen = torch.Generator(device=dev).manual_seed(seed)
    parts = []
    for s in range(0, N, 65536):
        blk = torch.randn(min(65536, N - s), D, generator=gen, device=dev)
        a, b = max(lo, s), min(hi, s + blk.shape[0])
        if a < b:
            parts.append(torch.nn.functional.normalize(blk[a - s:b - s], dim=1))
    rows = torch.cat(parts)
    del parts
    if sharded:
        from keds_amd.index import ShardedFlatIndex
        idx = ShardedFlatIndex(D, "l2", device=dev)
        idx.n_global = N
        idx.local = keds_amd.FlatIndex(D, "l2", device=dev, row0=lo)
        idx.local.add(rows)
        return idx, idx.local, lo, hi
    idx = keds_amd.FlatIndex(D, "l2", device=dev, row0=lo)
    idx.add(rows)
    return idx, idx, lo, hi


# ---- KEDS_BENCH_CPU_DRYRUN=1: the whole N-rank FLOW of this file on CPU tensors over gloo (tests/test_host_cpu.py runs it with 8
# ranks: launch, pilot, packed exchange, per-rank report, verification, exit codes).  The encoder and the shard scan are stand-ins
# (seeded unit-norm queries; the oracle's exact search over a small shard) -- nothing it prints is a measurement.
class _DryEvent:
    def __init__(self, enable_timing=False):
        self.t = 0.0

    def record(self):
        self.t = time.perf_counter()

    def elapsed_time(self, other):
        return (other.t - self.t) * 1e3


class _DryModel:
    numerics = "dry-run"

    def __init__(self, batch, rank):
        self.q = torch.nn.functional.normalize(torch.randn(batch, 768, generator=torch.Generator().manual_seed(1001 + rank)), dim=1)
        fail = os.environ.get("KEDS_BENCH_DRYRUN_FAIL_RANK", "")
        self.fail = fail != "" and int(fail) == rank
        self.calls = 0

    def encode_image(self, images, normalize=True):
        self.calls += 1
        if self.fail and self.calls >= 3:
            raise RuntimeError(f"KEDS_BENCH_DRYRUN_FAIL_RANK: rank {os.environ.get('RANK', '0')} fails on purpose")
        return self.q[: (images.shape[0] if images is not None else self.q.shape[0])].clone()

    def set_precision(self, p):
        return self

    def numerics_sync(self):
        return False


class _DryIndex:
    """Stand-in for FlatIndex on CPU tensors: exact search of this rank's rows (the oracle's), global ids."""
    def __init__(self, rows, lo):
        from keds_amd import _lib
        self.rows, self.row0, self.metric = rows, lo, _lib.METRIC_L2

    def search_device(self, q, k, normalize=False):
        from oracle import keds_oracle as O
        d, i = O.flat_l2_search(self.rows, q, k)
        return d, i + self.row0, None


def _cos_rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    cos = float((torch.nn.functional.normalize(a, dim=1) * torch.nn.functional.normalize(b, dim=1)).sum(1).min())
    return cos, float((a - b).norm() / b.norm())


# composed dual-stream features: the tolerance of the text tower's pass on top of the image tower's, and -- for the rounded
# operating points -- room for a near-tied neighbour of the random database to change (it changes a knowledge token)
EMBED_LIMITS_DUAL = {"bf16": (0.999, 5.0e-2), "fp8": (0.98, 2.0e-1), "fp32": (0.99999, 1.0e-4), "fp32x3": (0.99999, 1.0e-4)}
EMBED_LIMITS = {"bf16": (0.9999, 6.0e-3), "fp8": (0.995, 1.0e-1), "fp32": (0.999999, 1.0e-5), "fp32x3": (0.999999, 2.0e-5)}     # (min cosine, max rel-L2): tests/gpu_util.py


def verify_topk(index_rows, lo, q_dev, Dk, Ik, k, world, dist, n_check=8):
    """The timed path's top-k of this rank-0's first `n_check` queries against the oracle's exact search
    (oracle/keds_oracle.py flat_l2_search: fp64 distances, ties to the lower id) over ALL database rows: every rank searches ITS
    rows on its host cores, rank 0 merges the partial lists keyed on (distance, id).  Returns a dict on rank 0, None elsewhere."""
    from oracle import keds_oracle as O
    q = q_dev[:n_check].float().cpu().contiguous()
    if world > 1:
        dist.broadcast_object_list(obj := [q], src=0)
        q = obj[0]
    t0 = time.perf_counter()
    d, i = O.flat_l2_search(index_rows.float().cpu(), q, k)
    part = (d.double(), i + lo)
    parts = [part]
    if world > 1:
        parts = [None] * world
        dist.all_gather_object(parts, part)
    if (int(os.environ.get("RANK", "0")) if world > 1 else 0) != 0:
        return None
    d_all, i_all = torch.cat([p_[0] for p_ in parts], dim=1), torch.cat([p_[1] for p_ in parts], dim=1)
    key = torch.argsort(i_all, dim=1, stable=True)                       # (distance, id) order: sort by id, then stably by distance
    d_all, i_all = torch.gather(d_all, 1, key), torch.gather(i_all, 1, key)
    key = torch.argsort(d_all, dim=1, stable=True)[:, :k]
    d_ref, i_ref = torch.gather(d_all, 1, key), torch.gather(i_all, 1, key)
    got_i, got_d = Ik[:n_check].cpu().long(), Dk[:n_check].cpu().double()
    mism = int((got_i != i_ref).sum())
    return {"queries": int(q.shape[0]), "k": k, "rows_searched": None, "id_mismatches": mism,
            "max_abs_distance_error": float((got_d - d_ref).abs().max()), "cpu_seconds": round(time.perf_counter() - t0, 2),
            "checker": "oracle flat_l2_search (fp64, exact) over all database rows on the host cores"}



RECALL_KS = (1, 5, 10, 50, 100)
RECALL_MARGIN = 5e-4      # tests/test_gpu_fullsize.py: an outcome may differ only where the reference's own gap at the cut is below this


def _synth_parallel(fn, n, chunk=25):
    """oracle image generators are per-image seeded (any slice reproducible on its own): run slices on a few host threads."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        parts = list(ex.map(lambda s: fn(s, min(chunk, n - s)), range(0, n, chunk)))
    return torch.cat(parts)


def recall_leg(keds_amd, dev, precisions=("bf16", "fp32x3")):
    """Recall@k parity MEASURED IN THIS RUN (BASELINE config 1 at ViT-L/14 on the GPU): the 1,000 gallery + 256 query images of
    tests/golden/recall_vitl14.npz (seeded generators of the oracle; sharpened seed-7 weights) through the timed path's
    encode_image at the headline operating point and at the Recall-equal one, ranked by get_metrics_cirr, against the features
    and Recall@k the REFERENCE produced for the same inputs (minted by tools/mint_golden.py from /root/reference;
    metric: src/eval_utils.py:1040-1067).  An outcome (query, k) counts as flipped when the target is inside the top-k in one
    ranking and not in the other; the headline point may flip at most 3 of 1,280, each inside the reference's own 5e-4 gap."""
    import numpy as np
    from oracle import keds_oracle as O
    t_start = time.perf_counter()
    path = os.path.join(ROOT, "tests", "golden", "recall_vitl14.npz")
    g = dict(np.load(path))
    cfg = {k_: v for k_, v in VITL.items() if k_ != "transformer_heads"}
    sd = O.sharpen_clip(O.synth_clip_state_dict(**cfg, seed=7, visual_only=True))
    m = keds_amd.build_model(sd, fp16=False).to(dev)
    del sd
    G, Q = g["gallery"].shape[0], g["query"].shape[0]
    tgt, ref, sigma = O.synth_recall_plan(G, Q)
    if not (np.array_equal(tgt, g["tgt_idx"]) and np.array_equal(ref, g["ref_idx"])):
        return {"ok": False, "error": "the recall plan of the oracle differs from the fixture's"}
    gal_img = _synth_parallel(lambda s_, n_: O.synth_gallery_images(n_, start=s_), G).to(dev)
    q_img = _synth_parallel(lambda s_, n_: O.synth_recall_queries(tgt, sigma, start=s_, count=n_), Q).to(dev)
    t_synth = time.perf_counter() - t_start
    index_names = [f"/data/cirr/dev/img_{i:05d}.png" for i in range(G)]
    ref_names = [os.path.basename(index_names[i]) for i in ref]
    tgt_names = [os.path.basename(index_names[i]) for i in tgt]
    rows, tg, rf = torch.arange(Q), torch.from_numpy(tgt), torch.from_numpy(ref)
    dr = 1.0 - torch.from_numpy(g["query"]) @ torch.from_numpy(g["gallery"]).T
    dr[rows, rf] = float("inf")
    rank_r = (dr < dr[rows, tg][:, None]).sum(1)
    others = dr.clone()
    others[rows, tg] = float("inf")
    sorted_others = others.sort(dim=1).values
    want = {k_: float(g[f"recall_R_at_{k_}"]) for k_ in RECALL_KS}
    out = {"gallery": G, "queries": Q, "ks": list(RECALL_KS), "reference": {f"R@{k_}": want[k_] for k_ in RECALL_KS}, "points": {}}
    ok = True
    for prec in precisions:
        m.set_precision(prec)
        m.encode_image(gal_img[:125], normalize=True)             # packing + first-launch costs outside the clock
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gal = torch.cat([m.encode_image(gal_img[i:i + 125], normalize=True) for i in range(0, G, 125)]).float()
        qf = torch.cat([m.encode_image(q_img[i:i + 128], normalize=True) for i in range(0, Q, 128)]).float()
        tripped = bool(m.numerics_sync())
        torch.cuda.synchronize()
        t_enc = time.perf_counter() - t0
        got = keds_amd.get_metrics_cirr(gal, qf, ref_names, index_names, tgt_names)
        dg = (1.0 - qf @ gal.T).cpu()
        dg[rows, rf] = float("inf")
        rank_g = (dg < dg[rows, tg][:, None]).sum(1)
        flips, outside = 0, 0
        for k_ in RECALL_KS:
            flip = (rank_r < k_) != (rank_g < k_)
            gap = (dr[rows, tg] - sorted_others[:, k_ - 1]).abs()
            flips += int(flip.sum())
            outside += int((gap[flip] >= RECALL_MARGIN).sum())
        cg, rg = _cos_rel(gal, torch.from_numpy(g["gallery"]))
        cq, rq = _cos_rel(qf, torch.from_numpy(g["query"]))
        rec = {f"R@{k_}": got[f"recall_R@{k_}"] for k_ in RECALL_KS}
        equal = all(abs(rec[f"R@{k_}"] - want[k_]) < 1e-9 for k_ in RECALL_KS)
        limit = 0 if prec in ("fp32", "fp32x3") else 3
        p_ok = flips <= limit and outside == 0 and not tripped and (equal or prec == "bf16") and (getattr(m, "precision", prec) == prec)
        out["points"][prec] = {"recall": rec, "recall_equals_reference": bool(equal), "outcomes_flipped_of_%d" % (Q * len(RECALL_KS)): flips,
                               "flips_outside_the_references_own_margin": outside, "target_rank_changes": int((rank_r != rank_g).sum()),
                               "gallery_features_vs_reference": {"min_cosine": cg, "rel_l2": rg},
                               "query_features_vs_reference": {"min_cosine": cq, "rel_l2": rq},
                               "encode_seconds": round(t_enc, 3), "images_per_sec": round((G + Q) / t_enc, 1),
                               "numerics_guard_tripped": tripped, "ok": bool(p_ok)}
        ok = ok and p_ok
    out["ok"] = bool(ok)
    out["host_seconds_generating_inputs_and_weights"] = round(t_synth, 1)
    out["checker"] = ("tests/golden/recall_vitl14.npz: features and Recall@k the reference produced for these inputs "
                      "(tools/mint_golden.py); inputs regenerated by the oracle's seeded generators")
    del m, gal_img, q_img
    torch.cuda.empty_cache()
    return out


def headline(args, dual, world, B, N, D, k, elapsed, shared_gpu, dry):
    """The head of the result line, the same in a plain run and in --full: the measured figure, its unit and its setting."""
    fp8, f32, x3 = args.precision == "fp8", args.precision == "fp32", args.precision == "fp32x3"
    steps = args.steps
    if dual:
        metric = "composed dual-stream queries/sec (ViT-L/14 encode + 2 x top-16 with rows + knowledge streams + 2 text passes)"
        workload = ("dual-stream composed query, BASELINE config 4: ViT-L/14 encode_image (224x224 synthetic, random-init "
                    "weights) + exact top-16 with row gather over TWO synthetic unit-norm %.1fM x 768 databases + 2 knowledge "
                    "streams (IM2TEXT + 2 x CrossFormer) + 2 text-tower passes with pseudo-token splice + normalise / "
                    "mixture" % (N / 1e6))
        par = f"dp{world} encoders + knowledge path, {world}-way row-sharded scans, rows shipped with the partial lists"
    else:
        metric = "query-images/sec (encode+0.5M top-10) ViT-L/14"
        workload = ("ViT-L/14 encode_image (224x224 synthetic, random-init weights) + exact top-%d over a synthetic "
                    "unit-norm %.1fM x 768 database" % (k, N / 1e6))
        par = f"dp{world} encoders + {world}-way row-sharded scan"
    return {
        "metric": metric,
        "value": world * B * steps / elapsed,
        "unit": "queries/sec" if dual else "query-images/sec",
        "n_gpus": world, "steps": steps, "warmup": args.warmup,
        "ms_per_step": elapsed / steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": ("fp8 (MXFP8 e4m3 operands, fp32 accumulate; config 5)" if fp8 else
                  "f32 (f32-input MFMA, no operand rounding: the accuracy operating point)" if f32 else
                  "fp32x3 (fp32 flow, block GEMMs on split fp16 operands: 3 fp16 MFMA products per product, fp32 accumulate)" if x3 else
                  "bf16/fp16 operands, fp32 accumulate"), "data": "synthetic",
        **({"diagnostic": "KEDS_BENCH_SHARED_GPU=1: all ranks share ONE GPU over a host-staged gloo transport -- a test of the "
                          "N > 1 flow, not a scaling measurement"} if shared_gpu else {}),
        **({"diagnostic": "KEDS_BENCH_CPU_DRYRUN=1: CPU tensors over gloo with stand-ins for the encoder and the shard scan -- "
                          "a test of this file's N-rank flow; NOTHING here is a measurement"} if dry else {}),
        "config": {"workload": workload,
                   "batch_per_gpu": B, "global_batch": B * world, "db_rows": N, "dim": D, "k": k,
                   "db_shards": world, "parallelism": par},
    }


def search_overlap_note(dual, xchg, on):
    return ("n/a (dual: the knowledge path consumes the neighbours at once)" if dual else
            "none (one GPU: no collective to hide)" if xchg is None else
            ("search of batch i on a second stream beside the encoder pass of batch i+1" if on
             else "serial: search on the encoder's stream"))


def emit(out):
    try:                                   # RCCL writes its version banner through C stdio, which flushes at exit:
        import ctypes                      # push it out now so that the JSON line is the last line on stdout
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    print(json.dumps(out), flush=True)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(directory, arrays, seed=0):
    """--dump-outputs: each array the timed path returned in its last step as <directory>/<name>.npy, floating outputs in float32,
    integer ones in float64 (exact below 2**53).  Beyond DUMP_LIMIT_BYTES in all, every array keeps the same fixed, seeded sample of
    its rows, and <name>.rows.npy holds the row numbers kept."""
    import numpy as np
    host = {}
    for name, t in arrays.items():
        if isinstance(t, torch.Tensor):
            t = t.detach().cpu()
            host[name] = (t.float() if t.is_floating_point() else t.double()).numpy()
    total = sum(a.nbytes for a in host.values())
    os.makedirs(directory, exist_ok=True)
    for name, a in host.items():
        if total > DUMP_LIMIT_BYTES and a.ndim and a.shape[0] > 1:
            keep = max(1, int(a.shape[0] * (DUMP_LIMIT_BYTES // 2) / total))
            rows = np.sort(np.random.RandomState(seed).permutation(a.shape[0])[:keep])
            a = a[rows]
            np.save(os.path.join(directory, name + ".rows.npy"), rows.astype(np.float64))
        np.save(os.path.join(directory, name + ".npy"), a)
    print(f"bench: wrote {len(host)} output arrays to {directory}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128, help="images per GPU per step")
    ap.add_argument("--db-rows", type=int, default=500000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-verify", action="store_true", help="skip the self-verification behind the timed region (A/B scripts)")
    ap.add_argument("--workload", choices=["encode_search", "dual"], default="encode_search",
                    help="encode_search = BASELINE configs 1-3, the headline (ViT-L/14 encode + top-10); dual = config 4: the "
                         "dual-stream composed query (encode + 2 x top-16 with rows over two databases + 2 knowledge streams + "
                         "2 text-tower passes + normalise / mixture)")
    ap.add_argument("--precision", choices=["bf16", "fp8", "fp32", "fp32x3"], default="bf16",
                    help="fp8 = BASELINE config 5 (MXFP8 GEMM operands in the towers; use with --db-rows 2000000); fp32 = the "
                         "reference's own evaluation arithmetic (no operand rounding, f32-input MFMA: the accuracy operating "
                         "point, Recall@k equal to the reference); fp32x3 = the same flow with the block GEMMs on split fp16 operands "
                         "(three fp16 MFMA products per product, fp32-grade results); the headline metric is bf16")
    ap.add_argument("--search-overlap", choices=["auto", "on", "off"], default=os.environ.get("KEDS_BENCH_OVERLAP", "auto"),
                    help="N > 1, encode_search: run the search of batch i (its two collectives and short launches) on a second "
                         "stream beside the encoder pass of batch i+1 (on), behind it on the encoder's stream (off), or time "
                         "both in a pilot before the timed region and keep the faster (auto)")
    ap.add_argument("--no-legs", action="store_true", help="skip the 3-step legs of the other BASELINE configurations behind the timed "
                    "region (safe_point, fp8_point, dual_point, recall_parity_measured)")
    ap.add_argument("--fp8-db-rows", type=int, default=2000000, help="keys of the fp8_point leg's database (config 5: 2 M)")
    ap.add_argument("--prof-every", type=int, default=4, help="record the per-launch hipEvents on every N-th timed step")
    ap.add_argument("--prof-all", action="store_true", help="hipEvent pairs around every kernel class (default: only the "
                    "dominant GEMM class and the scan; the full breakdown costs ~1-2 %% of the step)")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline: per-kernel-class hipEvents in the timed "
                    "steps (roofline, stage times), the self-verification, the legs of the other configurations, the measured "
                    "Recall@k parity and the CPU baseline (--no-verify / --no-legs / --no-cpu-baseline / --prof-* apply here)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the timed path returned in its last step "
                    "as DIR/<name>.npy (float32 / float64; at most 64 MB in all)")
    args = ap.parse_args()
    args.prof_every = max(1, args.prof_every)
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: start the ranks as a child process before anything here touches the GPU
        raise SystemExit(self_launch(args.gpus, sys.argv[1:]))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # KEDS_BENCH_SHARED_GPU=1 (diagnostic, never a measurement of scaling): all ranks of `--gpus N` share cuda:0 and talk over
    # gloo with host-staged collectives (keds_amd.index.install_host_staged_transport) -- the whole N > 1 flow of this file
    # (packed exchange, overlap pilot, per-rank report) on a box with one GPU
    shared_gpu = os.environ.get("KEDS_BENCH_SHARED_GPU") == "1"
    dry = os.environ.get("KEDS_BENCH_CPU_DRYRUN") == "1"       # flow test on CPU tensors over gloo (see _DryModel): no measurement
    if shared_gpu:
        local = 0
    if dry:
        dev = torch.device("cpu")
    else:
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
    import torch.distributed as dist
    use_dist = world > 1 or os.environ.get("KEDS_BENCH_FORCE_DIST") == "1"   # the latter: 1-rank test of the RCCL path
    if use_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if world == 1:                                         # forced 1-rank group outside torch.distributed.run
            for key, val in (("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0"), ("MASTER_ADDR", "127.0.0.1"),
                             ("MASTER_PORT", str(29500 + os.getpid() % 2000))):
                os.environ.setdefault(key, val)
        if dry:
            os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
            dist.init_process_group("gloo")
        elif shared_gpu:
            dist.init_process_group("gloo")
            from keds_amd.index import install_host_staged_transport
            install_host_staged_transport(dist)
        else:
            dist.init_process_group("nccl", device_id=dev)     # "nccl" is RCCL on ROCm

    import keds_amd
    from keds_amd import _lib
    from keds_amd.index import PackedExchange, shard_bounds
    _lib.load()                                                # fail loudly if the HIP library is missing

    dual = args.workload == "dual"
    if os.environ.get("KEDS_BENCH_TEXT_RECT") == "1":           # A/B only: the text tower on the rectangular [B, max len] layout
        import keds_amd.model as _km
        _km.TEXT_PACKED = False
    B, N, D = args.batch, args.db_rows, 768
    k = 16 if dual else args.k                                 # the knowledge path takes the 16 nearest rows of each database
    model = _DryModel(B, rank) if dry else random_clip(dev)
    if args.precision != "bf16":
        model.set_precision(args.precision)
    fault = os.environ.get("KEDS_BENCH_INJECT_FAULT", "")       # tests only: the self-verification must catch both
    if fault == "1":                                            # 1: an encoder that writes garbage into a seventh of its outputs
        _enc = model.encode_image

        def _bad_encode(*a, **kw):
            o = _enc(*a, **kw)
            o[:, ::7] = 0.0
            return o
        model.encode_image = _bad_encode
    if dry:
        if dual:
            raise SystemExit("KEDS_BENCH_CPU_DRYRUN covers the encode_search workload")
        lo, hi = shard_bounds(N, world, rank)
        rows_all = torch.nn.functional.normalize(torch.randn(N, D, generator=torch.Generator().manual_seed(2002)), dim=1)
        index = local_index = _DryIndex(rows_all[lo:hi].clone(), lo)
        images = torch.zeros(B, 1)
    else:
        index, local_index, lo, hi = build_database(keds_amd, shard_bounds, N, D, world, rank, dev, 2002, dual and use_dist)
        images = torch.randn(B, 3, 224, 224, generator=torch.Generator(device=dev).manual_seed(1001 + rank), device=dev)
    if dual:
        index_t, _, _, _ = build_database(keds_amd, shard_bounds, N, D, world, rank, dev, 2003, use_dist)
        database = [None, None, None, index, index_t]

        def stream_modules(seed):
            torch.manual_seed(seed)
            a, b, c = keds_amd.make_stream_modules(model, middle_dim=512, n_layer=2, device=dev)
            return keds_amd.KnowledgeStream(a, b, c)
        s_img, s_txt = stream_modules(1), stream_modules(2)
        tokens = synth_tokens(B).to(dev)

    # encode_search, N > 1: the search of batch i can run on its own stream behind batch i's encoder pass, beside batch
    # i+1's: its two KB-sized, latency-bound collectives (one packed all-gather of the queries, one packed all-to-all of the
    # partial lists; preallocated buffers, keds_amd.index.PackedExchange) and its short merge / re-rank launches then hide
    # under the next encoder pass instead of standing between two of them -- but a scan that shares the CUs with the next
    # encoder pass reads at a lower rate and slows that pass down.  Which wins depends on the world size (collective
    # latency) and is measured, not assumed: --search-overlap auto times both before the timed region.
    # (With one GPU there is no collective to hide: the search stays on the encoder's stream.)
    xchg = PackedExchange() if (use_dist and not dual) else None
    import contextlib
    Event = _DryEvent if dry else torch.cuda.Event
    main_stream = None if dry else torch.cuda.current_stream()
    side_stream = torch.cuda.Stream(device=dev) if (xchg is not None and not dry) else None
    overlap = {"on": False}
    comm_events = []                                            # (gather, scan, return) hipEvent quadruples of profiled steps
    search_events = []                                          # hipEvent pairs around the whole local search of profiled steps

    cur = {"index": index}                                   # (a leg behind the timed region swaps the database: fp8_point)
    last = {}                                                # what the latest step returned to its caller (--dump-outputs)

    def step_encode_search(timed=False):
        q = model.encode_image(images, normalize=True)          # [B,768] on device
        last["query_embeddings"] = q
        ovl = overlap["on"] and not dry
        search_stream = side_stream if ovl else main_stream
        if ovl:
            search_stream.wait_stream(main_stream)
        with (contextlib.nullcontext() if dry else torch.cuda.stream(search_stream)):
            if ovl:
                q.record_stream(search_stream)
            ev = [Event(enable_timing=True) for _ in range(4)] if (timed and xchg is not None) else None
            if ev:
                ev[0].record()
            allq = xchg.gather_queries(q) if xchg is not None else q
            if ev:
                ev[1].record()
            sev = [Event(enable_timing=True) for _ in range(2)] if timed else None
            if sev:
                sev[0].record()
            Dk, Ik, _ = cur["index"].search_device(allq, k)
            if sev:
                sev[1].record()
                search_events.append(sev)
            if ev:
                ev[2].record()
            if xchg is not None:
                Dk, Ik = xchg.return_partials(Dk, Ik, index.metric)
            if ev:
                ev[3].record()
                comm_events.append(ev)
        return Dk, Ik

    def step_dual(timed=False):
        out = keds_amd.compose_query_features(model, s_img, s_txt, images, tokens, database, id_split=265, verify=False)
        last.update(out)
        return out["mixture"], None

    step = step_dual if dual else step_encode_search

    def fence():
        if not dry:
            torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        if not dry:
            torch.cuda.synchronize()

    red_dev = torch.device("cpu") if (shared_gpu or dry) else dev       # (gloo reduces host tensors)

    def timed_run(n):
        fence()
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        fence()
        t = torch.tensor([time.perf_counter() - t0], device=red_dev, dtype=torch.float64)
        if use_dist:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item()) / n * 1e3

    for _ in range(args.warmup):
        step()
    pilot = None
    if xchg is not None:
        if args.search_overlap == "auto":                       # untimed pilot: both placements, max over ranks, keep the faster
            pilot = {}
            for name, on in (("off", False), ("on", True), ("off2", False), ("on2", True)):
                overlap["on"] = on
                step()
                pilot[name] = timed_run(6)
            t_off, t_on = min(pilot["off"], pilot["off2"]), min(pilot["on"], pilot["on2"])
            overlap["on"] = t_on < t_off
            pilot = {"serial_ms_per_step": t_off, "overlapped_ms_per_step": t_on}
        else:
            overlap["on"] = args.search_overlap == "on"
        step()
    fence()
    if dry:                                                     # no launches: no per-launch events
        _lib.prof_reset = _lib.prof_enable = lambda *a, **k: None
        _lib.prof_read = lambda klass: (0.0, 0)
        _lib.prof_read_work = lambda klass: 0.0
    _lib.prof_reset()
    # hipEvent pair around every launch of the dominant kernel class (GEMM) and of the scan, on the launch stream, inside
    # the timed region -- on every `--prof-every`-th timed step (default 4: steps 0, 4, 8, ...).  An event pair costs ~3.5 us
    # of stream time; around all 100 launches of every step that is 2.7 % of the step, sampled it is 0.7 %.
    # A plain run carries no event pairs: they feed the per-kernel figures of --full only.
    classes = None if args.prof_all else (_lib.PROF_GEMM, _lib.PROF_SCAN)
    events = args.full and os.environ.get("KEDS_BENCH_NO_EVENTS") != "1"      # (the latter: A/B of the event overhead only)
    prof_steps = 0
    t0 = time.perf_counter()
    for i in range(args.steps):
        on = events and i % args.prof_every == 0
        if on:
            _lib.prof_enable(True, classes)
            prof_steps += 1
        Dk, Ik = step(timed=on)
        if on:
            _lib.prof_enable(False)
    fence()
    elapsed = time.perf_counter() - t0
    guard_tripped = bool(model.numerics_sync())                 # the lazily checked numerics guard of the timed passes
    if fault == "2" and Ik is not None:                          # 2: a search that returns two neighbours in the wrong order
        Ik = Ik.clone()
        Ik[0, [0, 1]] = Ik[0, [1, 0]]
    t = torch.tensor([elapsed], device=red_dev, dtype=torch.float64)
    if use_dist:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, dict(last) if dual else
                     {"query_embeddings": last["query_embeddings"], "topk_distances": Dk, "topk_ids": Ik})

    if not args.full:
        if rank == 0:
            out = headline(args, dual, world, B, N, D, k, elapsed, shared_gpu, dry)
            out["numerics_guard"] = {"mode": model.numerics, "tripped": guard_tripped}
            out["search_overlap"] = search_overlap_note(dual, xchg, overlap["on"])
            out["search_overlap_pilot"] = pilot
            emit(out)
        if use_dist:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ---- self-verification, OUTSIDE the timed region: the line must not be able to report a speed for wrong results
    # (round 4, finding 1: a "10 % gain" was a kernel writing garbage).  (a) the LAST timed step's top-k of rank 0's first 8
    # queries against the oracle's exact search over all rows (every rank checks its shard on its host cores);
    # (b) an fp32-mode leg of 3 steps: the Recall-equal operating point, timed by the same clock; (c) -- with the cpu_baseline
    # leg, rank 0, N = 1 -- the embeddings of the SAME 8 images the oracle encodes (below, where the oracle's are available).
    verification = None
    fp32_point = fp32x3_point = emb32 = None
    if not dual and not args.no_verify:
        q_chk = model.encode_image(images, normalize=True)       # the same bits as the last step's queries (deterministic kernels)
        verification = verify_topk(local_index.rows, lo, q_chk, Dk, Ik, k, world if use_dist else 1, dist)
        if args.precision == "bf16" and not dry:
            model.set_precision("fp32")
            step()
            ms32 = timed_run(3)
            emb32 = model.encode_image(images[:8], normalize=True).float().cpu()
            model.set_precision("bf16")
            emb16 = model.encode_image(images[:8], normalize=True).float().cpu()
            c32, r32 = _cos_rel(emb16, emb32)
            model.set_precision("fp32x3")
            step()
            msx3 = timed_run(3)
            embx3 = model.encode_image(images[:8], normalize=True).float().cpu()
            model.set_precision("bf16")
            cx3, rx3 = _cos_rel(embx3, emb32)
            fp32x3_point = {"value": world * B / (msx3 * 1e-3), "unit": "query-images/sec", "ms_per_step": msx3, "steps": 3,
                            "what": "the same step with set_precision('fp32x3'): the fp32 flow with the block GEMMs on split fp16 operands "
                                    "(hi.hi + hi.lo + lo.hi on the fp16 MFMA) -- fp32-grade embeddings, Recall@k equal (tests/test_gpu_fp32.py)",
                            "vs_fp32_embeddings": {"min_cosine": cx3, "rel_l2": rx3, "images": 8},
                            "fell_back_to_fp32": bool(getattr(model, "x3_range_trips", 0))}
            fp32_point = {"value": world * B / (ms32 * 1e-3), "unit": "query-images/sec", "ms_per_step": ms32, "steps": 3,
                          "what": "the same step with set_precision('fp32'): f32-input MFMA, no operand rounding -- the operating "
                                  "point whose Recall@k equals the reference's (tests/test_gpu_fp32.py)",
                          "headline_vs_fp32_embeddings": {"min_cosine": c32, "rel_l2": r32, "images": 8}}

    failed = False
    per_rank = None
    if xchg is not None:                                        # what each rank's search costs, so a scaling run explains itself
        mine = [sum(e[i].elapsed_time(e[i + 1]) for e in comm_events) / max(len(comm_events), 1) * 1e3 for i in range(3)]
        gathered = [None] * world
        dist.all_gather_object(gathered, mine)
        per_rank = {"query_allgather_us": [round(g[0], 1) for g in gathered],
                    "local_search_us": [round(g[1], 1) for g in gathered],
                    "partials_alltoall_merge_us": [round(g[2], 1) for g in gathered]}
    gemm_ms, gemm_n = _lib.prof_read(_lib.PROF_GEMM)
    scan_ms, scan_n = _lib.prof_read(_lib.PROF_SCAN)
    attn_ms, attn_n = _lib.prof_read(_lib.PROF_ATTN)
    ln_ms, ln_n = _lib.prof_read(_lib.PROF_LN)
    other_ms, other_n = _lib.prof_read(_lib.PROF_OTHER)
    gemm_work = _lib.prof_read_work(_lib.PROF_GEMM)            # 2*M*N*K summed over the launches that carried event pairs

    # ---- the other BASELINE configurations' 1-GPU forms, timed by the same clock behind the timed region (3 steps each, like
    # fp32_point) and each checked against the oracle / the reference-minted fixture: `safe_point` (the fp32-stream flow a
    # checkpoint that trips the numerics guard runs on), `fp8_point` (config 5: MXFP8 towers + 2 M keys), `dual_point`
    # (config 4: the dual-stream composed query) and `recall_parity` measured in this run (config 1 at ViT-L/14).
    legs, legs_failed = {}, False
    if fp32_point is not None and world == 1 and not use_dist and not args.no_legs:
        def embed_check(prec_key):
            e = model.encode_image(images[:8], normalize=True).float().cpu()
            c_, r_ = _cos_rel(e, emb32)
            lim_ = EMBED_LIMITS[prec_key]
            return {"min_cosine": c_, "rel_l2": r_, "limit_min_cosine": lim_[0], "limit_rel_l2": lim_[1], "images": 8,
                    "against": "the fp32 leg's embeddings of the same images (themselves 1e-6 from the oracle's)"}, bool(c_ >= lim_[0] and r_ <= lim_[1])

        # safe_point
        model.set_numerics("safe")
        step()
        ms = timed_run(3)
        chk, ok_ = embed_check("bf16")
        legs["safe_point"] = {"value": B / (ms * 1e-3), "unit": "query-images/sec", "ms_per_step": ms, "steps": 3,
                              "what": "the same step with set_numerics('safe'): fp32 residual stream + stand-alone LayerNorm, the flow a "
                                      "checkpoint runs on after the numerics guard tripped (keds_amd/model.py _guarded)",
                              "embeddings": chk, "ok": ok_}
        model.set_numerics("auto")
        legs_failed |= not ok_

        # fp8_point (config 5 on one GPU): MXFP8 towers, 2 M keys
        n8 = args.fp8_db_rows
        idx8, _, _, _ = build_database(keds_amd, shard_bounds, n8, D, 1, 0, dev, 2004, False)
        model.set_precision("fp8")
        cur["index"] = idx8
        step()
        ms = timed_run(3)
        torch.cuda.synchronize()
        _lib.prof_reset()
        _lib.prof_enable(True, (_lib.PROF_GEMM,))
        Dk8, Ik8 = step()
        _lib.prof_enable(False)
        torch.cuda.synchronize()
        g8_ms, g8_n = _lib.prof_read(_lib.PROF_GEMM)
        g8_work = _lib.prof_read_work(_lib.PROF_GEMM)
        q8 = model.encode_image(images, normalize=True)
        v8 = verify_topk(idx8.rows, 0, q8, Dk8, Ik8, k, 1, dist)
        chk, ok_ = embed_check("fp8")
        ok_ = bool(ok_ and v8["id_mismatches"] == 0 and v8["max_abs_distance_error"] <= 4e-6)
        v8["rows_searched"] = n8
        ach8 = g8_work / (g8_ms * 1e-3) / 1e12 if g8_ms > 0 else 0.0
        legs["fp8_point"] = {"value": B / (ms * 1e-3), "unit": "query-images/sec", "ms_per_step": ms, "steps": 3, "db_rows": n8,
                             "what": "BASELINE config 5 on one GPU: set_precision('fp8') (the block GEMMs on OCP-MX e4m3 operands, "
                                     "v_mfma_scale_f32_16x16x128_f8f6f4) + exact top-%d over %.1f M keys (bf16 scan + fp32 re-rank)" % (k, n8 / 1e6),
                             "roofline": {"kernel": "gemm_mxfp8_quad_kernel / gemm_mxfp8_kernel (all GEMM launches of one profiled step that carried event pairs)",
                                          "bound": "mfma", "achieved": ach8, "peak": PEAK_FP8_TFLOPS, "unit": "TFLOP/s",
                                          "frac": ach8 / PEAK_FP8_TFLOPS, "launches": g8_n, "gemm_ms_per_step": g8_ms},
                             "embeddings": chk, "topk": v8, "ok": ok_}
        model.set_precision("bf16")
        cur["index"] = index
        del idx8, q8, Dk8, Ik8
        torch.cuda.empty_cache()
        legs_failed |= not ok_

        # dual_point (config 4 on one GPU)
        index_t2, _, _, _ = build_database(keds_amd, shard_bounds, N, D, 1, 0, dev, 2003, False)
        database2 = [None, None, None, index, index_t2]

        def stream_modules2(seed):
            torch.manual_seed(seed)
            a, b, c = keds_amd.make_stream_modules(model, middle_dim=512, n_layer=2, device=dev)
            return keds_amd.KnowledgeStream(a, b, c)
        s_img2, s_txt2 = stream_modules2(1), stream_modules2(2)
        tokens2 = synth_tokens(B).to(dev)

        def step_dual2():
            return keds_amd.compose_query_features(model, s_img2, s_txt2, images, tokens2, database2, id_split=265, verify=False)["mixture"]
        for _ in range(2):
            step_dual2()
        fence()
        t0 = time.perf_counter()
        for _ in range(3):
            step_dual2()
        fence()
        ms = (time.perf_counter() - t0) / 3 * 1e3
        tripped2 = bool(model.numerics_sync())
        cpu_dual, chk = (None, None)
        if not args.no_cpu_baseline:
            cpu_dual, chk = cpu_baseline_dual(model, s_img2, s_txt2, N, D)
            lim = EMBED_LIMITS_DUAL["bf16"]
            chk["limit_min_cosine"], chk["limit_rel_l2"] = lim
            chk["ok"] = bool(chk["mixture_min_cosine"] >= lim[0] and chk["mixture_rel_l2"] <= lim[1] and chk["neighbour_id_mismatches"] == 0)
        ok_ = bool((chk is None or chk["ok"]) and not tripped2)
        legs["dual_point"] = {"value": B / (ms * 1e-3), "unit": "queries/sec", "ms_per_step": ms, "steps": 3,
                              "what": "BASELINE config 4 on one GPU: compose_query_features (ViT-L/14 encode + 2 x exact top-16 with rows over "
                                      "two %.1f M x 768 databases + 2 knowledge streams + one 2B-row text-tower pass + normalise / mixture; "
                                      "src/eval_utils.py:652-714)" % (N / 1e6),
                              "verification": chk, "cpu_baseline": cpu_dual, "ok": ok_}
        del index_t2, database2, s_img2, s_txt2
        torch.cuda.empty_cache()
        legs_failed |= not ok_

        # recall parity, measured
        try:
            legs["recall_parity_measured"] = recall_leg(keds_amd, dev)
        except FileNotFoundError as e:                          # (a checkout without tests/golden)
            legs["recall_parity_measured"] = {"ok": None, "skipped": str(e)}
        legs_failed |= legs["recall_parity_measured"]["ok"] is False

    if rank == 0:
        psteps = max(prof_steps, 1)                              # timed steps whose launches carried event pairs
        fp8, f32, x3 = args.precision == "fp8", args.precision == "fp32", args.precision == "fp32x3"
        side_rows = 0 if (f32 or x3 or dry) else _lib.load().keds_tower_side_rows(VITL["vision_width"], 257, B, int(fp8))
        if dual:
            # every GEMM launch of the step that carried an event pair (image tower, the 2B-row text-tower pass, IM2TEXT /
            # CrossFormer GEMMs, read-outs) with its own 2*M*N*K, counted by the library at launch (keds_prof_read_work);
            # side-lane launches carry neither events nor work
            gemm_flops = gemm_work
        else:
            gemm_flops = 2.0 * GEMM_MAC_PER_IMAGE * B * psteps     # this rank's GEMM launches on those steps
            # rows the towers run on the side lane (B*257 mod 256 = 128 of 32,896): those launches overlap the main stream
            # and carry no event pairs, so their flops leave the numerator as well
            if side_rows:
                tower_mac = 24 * 257 * 1024 * 3072 + 23 * 257 * _PER_TOKEN_TAIL
                gemm_flops -= 2.0 * tower_mac * B * psteps * side_rows / (B * 257.0)
        ach = gemm_flops / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
        # dense MFMA peak of the operand type; fp32x3: three fp16 MFMA products per algorithmic product (hi.hi + hi.lo + lo.hi)
        peak_tf = PEAK_FP8_TFLOPS if fp8 else PEAK_F32_TFLOPS if f32 else PEAK_BF16_TFLOPS / 3 if x3 else PEAK_BF16_TFLOPS
        peak_meas_tf = (PEAK_FP8_MEASURED_TFLOPS if fp8 else PEAK_F32_MEASURED_TFLOPS if f32 else
                        PEAK_BF16_MEASURED_TFLOPS / 3 if x3 else PEAK_BF16_MEASURED_TFLOPS)
        # algorithmic bytes of one search = one pass over this rank's bf16 rows (N_local*D*2 B), charged with the time of
        # every scan launch the search issues
        n_search = psteps * world * (2 if dual else 1)            # query blocks of 128 searched by this rank (profiled steps)
        scan_bytes = (hi - lo) * D * 2.0 * n_search
        scan_ach = scan_bytes / (scan_ms * 1e-3) / 1e9 if scan_ms > 0 else 0.0
        # the WHOLE local search (query preparation, scan, merges, re-rank, certificate + select, the exact-pass launches)
        # against the same algorithmic bytes: what a caller of index.search pays per query block
        whole = None
        if search_events:
            whole_ms = sum(a.elapsed_time(b2) for a, b2 in search_events) / len(search_events)
            whole_ach = (hi - lo) * D * 2.0 * world / (whole_ms * 1e-3) / 1e9 if whole_ms > 0 else 0.0
            whole = {"ms": whole_ms, "query_blocks": world, "achieved": whole_ach, "frac": whole_ach / PEAK_HBM_GBPS}
        gemm_traffic, gemm_traffic_note = (None, "PMC passes are of the bf16 encode_search workload only") if (fp8 or f32 or x3 or dual) \
            else pmc_traffic("gemm_256x256_all", B, N, world)
        scan_traffic, scan_traffic_note = (None, "n/a") if dual else pmc_traffic("scan_topk_kernel<768, 16", B, N, world)
        parity, parity_note = recall_parity()
        out = {
            **headline(args, dual, world, B, N, D, k, elapsed, shared_gpu, dry),
            "roofline": {"kernel": ("gemm_f32_kernel (128x128 tiles, v_mfma_f32_32x32x2_f32)" if f32 else
                                    "gemm_bt_pair_kernel<KEDS_EPI_X3_*> (256x256 tiles, three K segments over split fp16 planes; achieved = algorithmic 2MNK flops, peak = fp16 MFMA / 3)" if x3 else
                                    ("gemm_mxfp8_kernel" if fp8 else "gemm_bt_quad_kernel / gemm_bt_quad3_kernel / gemm_bt_pair_kernel") + " (256x256 tiles; all main-lane GEMM launches of the step incl. the few 128x128-tile ones)"), "bound": "mfma",
                         "achieved": ach, "peak": peak_tf, "unit": "TFLOP/s", "frac": ach / peak_tf,
                         "traffic": gemm_traffic, "traffic_unit": "bytes/launch (PMC, mean over the 256x256 GEMM launches; committed "
                         "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this workload; null when they are not of this build)",
                         "traffic_source": gemm_traffic_note,
                         "launches": gemm_n, "avg_launch_ms": gemm_ms / max(gemm_n, 1),
                         "flops_counted_at_launch": gemm_work,
                         # practical ceiling of this chip, measured (profiles/r01_microbench.txt): a register-only
                         # v_mfma_f32_16x16x32_bf16 loop sustains 2.06 PFLOP/s (clock ~2.0 GHz under MFMA load)
                         "peak_measured": peak_meas_tf, "frac_of_measured": ach / peak_meas_tf},
            "roofline_scan": {"kernel": "scan_topk_kernel", "bound": "hbm", "achieved": scan_ach,
                              "peak": PEAK_HBM_GBPS, "unit": "GB/s", "frac": scan_ach / PEAK_HBM_GBPS,
                              "traffic": scan_traffic, "traffic_source": scan_traffic_note,
                              "algorithmic_bytes_per_search": (hi - lo) * D * 2.0,
                              "launches": scan_n, "searches": n_search, "ms_per_search": scan_ms / max(n_search, 1),
                              "whole_search": whole,
                              # read-only stream over 4 GiB on this box: 7.15 TB/s (profiles/r01_microbench.txt)
                              "peak_measured": PEAK_HBM_MEASURED_GBPS, "frac_of_measured": scan_ach / PEAK_HBM_MEASURED_GBPS},
            "profiled_steps": prof_steps, "side_lane_rows": side_rows,
            "numerics_guard": {"mode": model.numerics, "tripped": guard_tripped,
                               "checked": "eagerly on the first passes, then lazily (flag copied to pinned memory behind every pass, "
                                          "verified after the timed region)"},
            "search_overlap": search_overlap_note(dual, xchg, overlap["on"]),
            "search_overlap_pilot": pilot,
            "per_rank_search": per_rank,
            # (classes whose launches carried no event pairs -- everything but GEMM and scan unless --prof-all -- read null)
            "stage_ms_per_step": {"gemm": gemm_ms / psteps if gemm_n else None, "attention": attn_ms / psteps if attn_n else None,
                                  "layernorm": ln_ms / psteps if ln_n else None, "scan": scan_ms / psteps if scan_n else None,
                                  "other": other_ms / psteps if other_n else None},
            # Recall@k parity with the reference's CPU path on identical inputs (tests/test_gpu_fullsize.py, fixture
            # recall_vitl14.npz: ViT-L/14, 1 k gallery, 256 queries x k in {1,5,10,50,100}); see profiles/r03_parity.json
            "recall_parity": parity, "recall_parity_source": parity_note,
            "recall_parity_measured_in_this_run": bool(legs.get("recall_parity_measured", {}).get("ok") is not None
                                                       and "recall_parity_measured" in legs),
        }
        for name in ("safe_point", "fp8_point", "dual_point"):
            if name in legs:
                out[name] = legs[name]
        if "recall_parity_measured" in legs:
            out["recall_parity_measured"] = legs["recall_parity_measured"]
        failed_dual = False
        if fp32_point is not None:
            out["fp32_point"] = fp32_point
            out["fp32x3_point"] = fp32x3_point
        if world == 1 and not args.no_cpu_baseline and not dual and not dry:
            out["cpu_baseline"], (s_img8, s_ref8) = cpu_baseline(model, N, D, k)
            if verification is not None:                       # the SAME images through the timed path
                got = model.encode_image(s_img8.to(dev), normalize=True).float().cpu()
                cos, rel = _cos_rel(got, s_ref8)
                lim = EMBED_LIMITS[args.precision]
                verification["embedding"] = {"images": int(s_img8.shape[0]), "min_cosine": cos, "rel_l2": rel,
                                             "limit_min_cosine": lim[0], "limit_rel_l2": lim[1],
                                             "checker": "oracle encode_image (fp32 torch CPU) on the images of the cpu_baseline leg"}
        elif world == 1 and not args.no_cpu_baseline and not dry:
            out["cpu_baseline"], chk = cpu_baseline_dual(model, s_img, s_txt, N, D)
            lim = EMBED_LIMITS_DUAL[args.precision]
            # (a neighbour may legitimately differ where the oracle's own fp32 query sits within rounding of a tie: reported, and
            # bounded -- the features decide)
            chk["limit_min_cosine"], chk["limit_rel_l2"] = lim
            chk["ok"] = bool(chk["mixture_min_cosine"] >= lim[0] and chk["mixture_rel_l2"] <= lim[1] and chk["neighbour_id_mismatches"] == 0
                             and not guard_tripped)
            out["verification"] = chk
            if not chk["ok"]:
                failed_dual = True
        if verification is not None:
            emb = verification.get("embedding")
            if emb is None:                                    # said, not implied: this line vouches for the search only
                verification["embedding"] = None
                verification["embedding_not_checked"] = ("no oracle embeddings in this run (--no-cpu-baseline, the dual workload, N > 1 "
                                                         "or the dry run): the top-k check above does not see a wrong ENCODER")
            verification["ok"] = bool(verification["id_mismatches"] == 0 and verification["max_abs_distance_error"] <= 4e-6 and
                                      (emb is None or (emb["min_cosine"] >= emb["limit_min_cosine"] and emb["rel_l2"] <= emb["limit_rel_l2"]))
                                      and not guard_tripped)
            verification["rows_searched"] = N
            out["verification"] = verification
        emit(out)
        if (verification is not None and not verification["ok"]) or failed_dual or legs_failed:
            failed = True
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if failed:
        raise SystemExit(3)                                    # a speed for wrong results is not a result


if __name__ == "__main__":
    main()
