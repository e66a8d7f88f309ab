"""keds_amd/csrc/tower_plan.h on the CPU, through keds_tower_plan_query: the steps a tower pass of the library runs from are the steps
tests/tower_check.py writes down (a), the comparison can fail (b), no two steps that share rows of a buffer are left unordered by the
lanes (c), the buffer table is the carving of tower_check.tower_buffers (d), and bad arguments are refused (e).  (f), at the end: the
same for WHOLE passes -- front end, blocks, read-out -- through keds_pass_plan_query against tower_check.plan_pass, with the workspace
sizes of the passes as literals, the packed-rows rule at its edge and the fp32x3 chunk helper.

The field mapping of (a), Python step -> int32 record of the library (include/keds_hip.h documents the record):
  op        zero / stats_cast / quant / cast / copy / split / gather / ln / attn / gemm / tap -> [0]; ln is LN_PAIR in the x3 flow, attn is
            ATTN or ATTN_FORK (the library's fork / join steps have no Python counterpart: they are what (c) checks), gemm is one of
            the four families by `kern`
  layer     [1];  w / g -> [2] (the LayerNorm-folded in_proj / c_fc of the 16-bit kernels are weights 5 / 6)
  epi       the class (bias, qgelu, resid, ln_bias, ln_qgelu, resid_stats) -> [3], the public id of that class in the flow's family and type
  a, src    (buffer, first row, row step) -> [4..6];  out, dst -> [7..9];  n -> [10];  qout / out_q -> [11];  plane -> [12] * width
  st_read / st_add / st_clear / st_r0 -> [13..16] (stats_cast's `st` is [14]: the buffer it writes)
  q_limit, q8_rows, off is not None -> [17..19];  bound, glob -> [20], [21];  lane -> [22] (side = 1 only where a side lane exists)"""
import ctypes as C

import numpy as np
import pytest

from keds_amd import _lib
from tests import tower_check as tc
from tests.test_host_tower_check import HEADS, LAYERS, LENS_256, LENS_257, LENS_MAX60, W, _cases, _mutation_cases

FLOW_ID = {"unfolded": 0, "bf16": 1, "fp16": 2, "fp8": 3, "f32": 4, "x3": 5}
TAIL_ID = {"all": 0, "cls": 1, "readout": 2}
TOWER_BUFS = 18                           # keds_tower_plan_query's table; a whole pass adds col, ro, out, tok, src
BUF = ["", "x", "h", "qkv", "att", "hid", "st1", "st2", "xq", "xs", "aq", "as", "hq", "hs", "splitk", "ln", "att_c", "x_c", "col", "ro", "out",
       "tok", "src"]
(ZERO, STATS_CAST, QUANT, CAST, COPY, SPLIT, GATHER, LN, LN_PAIR, ATTN, ATTN_FORK, GEMM16, GEMM_MX, GEMM_F32, GEMM_X3, TAP, FORK,
 JOIN, IM2COL, CLS, EMBED, L2NORM) = range(1, 23)
OPNAME = {ZERO: "zero", STATS_CAST: "stats_cast", QUANT: "quant", CAST: "cast", COPY: "copy", SPLIT: "split", GATHER: "gather", LN: "ln",
          LN_PAIR: "ln", ATTN: "attn", ATTN_FORK: "attn", GEMM16: "gemm", GEMM_MX: "gemm", GEMM_F32: "gemm", GEMM_X3: "gemm", TAP: "tap",
          FORK: "fork", JOIN: "join", IM2COL: "im2col", CLS: "cls", EMBED: "embed", L2NORM: "l2norm"}
KERN = {GEMM16: "16", GEMM_MX: "mx", GEMM_F32: "f32", GEMM_X3: "x3"}
WEIGHT = {1: "qkv", 2: "out", 3: "fc", 4: "proj", 5: "qkv", 6: "fc", 7: "ln1", 8: "ln2", 9: "conv", 10: "ln_pre", 11: "ln_out", 12: "proj_t"}
FIELDS = ("op", "layer", "weight", "epi", "in", "in_r0", "in_step", "out", "out_r0", "out_step", "n", "out2", "plane_rows", "st_read",
          "st_add", "st_clear", "st_r0", "q_limit", "q8_rows", "packed", "bound", "global", "lane", "rows")


def _epi_id(kern, cls, fp16):
    """the public epilogue id of a class in a kernel family (include/keds_hip.h)"""
    L = _lib
    if kern == "mx":
        return {"ln_bias": L.FP8_EPI_LN_BIAS_BF16, "ln_qgelu": L.FP8_EPI_LN_QGELU_MX, "resid_stats": L.FP8_EPI_RESID_STATS_MX_H}[cls]
    if kern == "f32":
        return {"bias": L.F32_EPI_BIAS, "qgelu": L.F32_EPI_QGELU, "resid": L.F32_EPI_RESID}[cls]
    if kern == "x3":
        return {"bias": L.EPI_X3_BIAS_F32, "qgelu": L.EPI_X3_QGELU_PAIR, "resid": L.EPI_X3_RESID_F32}[cls]
    if fp16:
        return {"ln_bias": L.EPI_LN_BIAS_F16_H, "ln_qgelu": L.EPI_LN_QGELU_F16_H, "resid_stats": L.EPI_RESID_STATS_F16_H,
                "resid": L.EPI_BIAS_RESID_F32_H, "qgelu": L.EPI_BIAS_QGELU_F16_H}[cls]
    return {"ln_bias": L.EPI_LN_BIAS_BF16_H, "ln_qgelu": L.EPI_LN_QGELU_BF16_H, "resid_stats": L.EPI_RESID_STATS_F16,
            "resid": L.EPI_BIAS_RESID_F32, "qgelu": L.EPI_BIAS_QGELU_BF16, "bias": L.EPI_BIAS_BF16}[cls]


def query(flow, width, heads, S, causal, layers, B, tail, packed=(0, 0), taps=False, split=-1, lane=-1, expect=0):
    """-> (steps as dicts, buffers {name: (offset, bytes, alias-of name)}, workspace bytes)"""
    lib = _lib.load()
    cap = 4096
    rec = np.zeros((cap, len(FIELDS)), dtype=np.int32)
    bufs = np.zeros((TOWER_BUFS, 4), dtype=np.int64)
    n, ws = C.c_int(0), C.c_size_t(0)
    rc = lib.keds_tower_plan_query(FLOW_ID.get(flow, flow), width, heads, S, int(causal), layers, B, TAIL_ID[tail], packed[0], packed[1],
                                   int(taps), split, lane, rec.ctypes.data, cap, C.byref(n), bufs.ctypes.data, C.byref(ws))
    assert rc == expect, _lib.last_error() if hasattr(_lib, "last_error") else rc
    if rc:
        return None
    assert 0 < n.value <= cap
    steps = [dict(zip(FIELDS, (int(v) for v in r))) for r in rec[:n.value]]
    table = {BUF[int(i)]: (int(o), int(b), BUF[int(al)]) for i, o, b, al in bufs if i}
    return steps, table, ws.value


def _stats(read, add, clear, r0):
    return (read or "", add or "", clear or "", r0) if (read or add or clear) else None


def canon_lib(s):
    """a record of the library in the canonical form both sides are compared in"""
    op = s["op"]
    ref_in, ref_out = (BUF[s["in"]], s["in_r0"], s["in_step"]), (BUF[s["out"]], s["out_r0"], s["out_step"])
    name = OPNAME[op]
    if name == "zero":
        return (name, BUF[s["out"]], s["out_r0"], s["n"])
    if name in ("stats_cast", "quant"):
        return (name, ref_in, ref_out, s["n"], BUF[s["st_add"]])
    if name in ("cast", "copy"):
        return (name, ref_in, ref_out, s["n"])
    if name == "split":
        return (name, ref_in, ref_out, s["n"], s["plane_rows"])
    if name == "gather":
        return (name, BUF[s["in"]], BUF[s["out"]], s["n"], s["bound"], bool(s["global"]))
    if name == "ln":
        return (name, s["layer"], WEIGHT[s["weight"]], ref_in, ref_out, s["n"], s["lane"], "pair" if op == LN_PAIR else "rows", s["rows"],
                s["epi"] if s["layer"] < 0 else None)
    if name == "im2col":
        return (name, BUF[s["in"]], BUF[s["out"]], s["n"], s["epi"])
    if name == "cls":
        return (name, ref_out, s["n"])
    if name == "embed":
        return (name, BUF[s["in"]], BUF[s["out"]], s["n"], bool(s["packed"]))
    if name == "l2norm":
        return (name, BUF[s["in"]], BUF[s["out"]], s["n"], s["epi"])
    if name == "attn":
        return (name, BUF[s["in"]], BUF[s["out"]], s["q_limit"], s["q8_rows"], BUF[s["out2"]], bool(s["packed"]))
    if name == "tap":
        return (name, s["layer"], ref_in, s["n"], s["lane"])
    if name == "gemm":
        return (name, s["layer"], WEIGHT[s["weight"]], s["weight"] in (5, 6), KERN[op], s["epi"], ref_in, ref_out, s["n"], BUF[s["out2"]],
                _stats(BUF[s["st_read"]], BUF[s["st_add"]], BUF[s["st_clear"]], s["st_r0"]), s["lane"])
    return (name,)


def canon_py(s, p, lane_on):
    name = s["op"]
    lane = int(lane_on and s.get("lane") == "side")
    if name == "zero":
        return (name, s["buf"], s["r0"], s["n"])
    if name in ("stats_cast", "quant"):
        return (name, (s["src"], s["r0"], 1), (s["dst"], s["r0"], 1), s["n"], s.get("st", ""))
    if name in ("cast", "copy"):
        return (name, s["src"], s["dst"], s["n"])
    if name == "split":
        assert s["plane"] % p.w == 0
        return (name, s["src"], s["dst"], s["n"], s["plane"] // p.w)
    if name == "gather":
        return (name, s["src"], s["dst"], s["n"], s["bound"], s["glob"])
    if name == "ln":
        return (name, s["layer"], s["g"], s["src"], s["dst"], s["n"], lane, "pair" if p.eff == "x3" else "rows", 0, None)
    if name == "attn":
        return (name, s["qkv"], s["out"], s["q_limit"], s["q8_rows"], s["out_q"] or "", s["off"] is not None)
    if name == "tap":
        return (name, s["layer"], s["src"], s["n"], lane)
    if name == "gemm":
        folded_w = s["kern"] == "16" and s["epi"].startswith("ln_")
        return (name, s["layer"], s["w"], folded_w, s["kern"], _epi_id(s["kern"], s["epi"], p.eff == "fp16"), s["a"], s["out"], s["n"],
                s.get("qout") or "", _stats(s.get("st_read"), s.get("st_add"), s.get("st_clear"), s["st_r0"]), lane)
    raise ValueError(name)


SPAN_OPS = ("gemm", "ln", "tap")      # confined to one span of rows; every other step is a cut


def segments(canon):
    """[(cut step or None, {first row of the span: [steps]})]: independent spans may interleave differently in the two orders"""
    segs = [(None, {})]
    for c in canon:
        if c[0] in ("fork", "join"):
            continue
        if c[0] in SPAN_OPS:
            r0 = c[3][1] if c[0] == "ln" else c[2][1] if c[0] == "tap" else c[7][1]
            segs[-1][1].setdefault(r0, []).append(c)
        else:
            segs.append((c, {}))
    return segs


def lib_args(flow, kind, kw):
    """the case of tower_check.plan(flow, kind, ...) as the arguments of the query"""
    p = tc.plan(flow, kind, LAYERS, width=kw.get("width", W), heads=kw.get("heads", HEADS), **{k: v for k, v in kw.items() if k not in ("width", "heads")})
    packed = (p.M, p.valid) if kind == "packed" else (0, 0)
    return p, dict(flow=flow, width=p.w, heads=p.heads, S=p.S, causal=p.causal, layers=LAYERS, B=p.B, tail=p.tail, packed=packed)


def compare(flow, kind, kw, lane, mutation=None):
    """-> None when the library's plan equals tower_check.plan (mutated: that plan with the defect), else the first difference"""
    split = bool(kw.get("split")) and flow in ("bf16", "fp16", "x3")
    pkw = dict(kw, split=split and lane)                           # a remainder span of the bf16 / fp16 / x3 flows needs the lane
    p, args = lib_args(flow, kind, pkw)
    steps, _, _ = query(**args, taps=bool(kw.get("taps")), split=int(split), lane=int(lane))
    if mutation:
        p = tc.mutate(p, mutation)
    if not lane:
        assert all(s["lane"] == 0 and s["op"] not in (FORK, JOIN, ATTN_FORK) for s in steps)
    a, b = segments([canon_lib(s) for s in steps]), segments([canon_py(s, p, lane) for s in p.steps])
    if len(a) != len(b):
        return f"{len(a)} segments, {len(b)} in the model"
    for i, ((ca, sa), (cb, sb)) in enumerate(zip(a, b)):
        if ca != cb:
            return f"segment {i}: cut {ca} != {cb}"
        if sa != sb:
            return f"segment {i}: {sa} != {sb}"
    return None


def _plan_cases():
    out = []
    for flow, kind, kw in _cases():
        for taps in (False, True):
            if taps and (kind != "tower" or kw.get("tail") != "all"):
                continue                                           # (taps: the all-rows pass of keds_vit_run_tokens)
            has_rem = flow == "fp8" or kw.get("split")
            for lane in ((True, False) if has_rem else (True,)):
                out.append((flow, kind, dict(kw, taps=taps), lane))
    return out


_ID = lambda v: v if isinstance(v, str) else str(v) if isinstance(v, bool) else "-".join(
    f"{k}{x if not isinstance(x, list) else sum(x)}" for k, x in v.items())


@pytest.mark.parametrize("flow,kind,kw,lane", _plan_cases(), ids=_ID)
def test_plan_is_tower_check_plan(flow, kind, kw, lane):
    assert compare(flow, kind, kw, lane) is None


def _gemm_splits_rows():
    f = getattr(_lib.load(), "_Z21keds_gemm_splits_rowsiii")      # bool keds_gemm_splits_rows(int, int, int): library-internal, C++
    f.restype, f.argtypes = C.c_bool, [C.c_int] * 3
    return f


def _real_cases():
    return [(flow, 257, B) for flow in ("bf16", "fp16", "fp8", "x3") for B in (54, 55)] + [("bf16", 17, 829)]


@pytest.mark.parametrize("flow,S,B", _real_cases())
@pytest.mark.parametrize("tail", ("all", "cls"))
def test_plan_at_the_geometry_that_splits(flow, S, B, tail):
    """width 1024: the library's own rule (split = -1) decides; the three rules of tower_splits_rows restated here"""
    w, M = 1024, B * S
    gs = _gemm_splits_rows()
    if flow == "x3":
        split = 0 < M // 256 * 256 < M and gs(M, 3 * w, w)
    elif flow == "fp8":
        split = M >= 256 and M % 256 != 0
    else:
        split = all(gs(M, n, k) for n, k in ((3 * w, w), (w, w), (4 * w, w), (w, 4 * w)))
    if flow in ("bf16", "fp16"):
        assert split == (B != 54)                                  # (tests/test_host_tower_check.py, test_side_rows)
    for lane in (True, False):
        p = tc.plan(flow, "tower", LAYERS, B, S=S, tail=tail, width=w, heads=16, split=split and lane, taps=tail == "all")
        steps, _, _ = query(flow, w, 16, S, False, LAYERS, B, tail, taps=tail == "all", split=-1, lane=int(lane))
        a, b = segments([canon_lib(s) for s in steps]), segments([canon_py(s, p, lane) for s in p.steps])
        assert a == b
        assert (len({s["lane"] for s in steps}) == 2) == bool(split and lane)


# ---- the library's own total order, written out from the passes' code as it stood before the plan existed ---------------------------
def _order(steps):
    out = []
    for s in steps:
        name = {ATTN_FORK: "attn+fork"}.get(s["op"], OPNAME[s["op"]])
        if name in SPAN_OPS:
            name = f"{WEIGHT.get(s['weight'], 'tap')}{s['layer']}@{'side' if s['lane'] else 'main'}"
        out.append(name)
    return out


def _block16(l):
    return [f"out{l}@main", f"out{l}@side", f"fc{l}@main", f"fc{l}@side", f"proj{l}@main", f"tap{l}@main", f"proj{l}@side", f"tap{l}@side"]


def test_enqueue_order_folded():
    steps, _, _ = query("bf16", 1024, 16, 257, False, 2, 55, "all", taps=True, lane=1)
    assert _order(steps) == ["stats_cast", "fork", "qkv0@main", "qkv0@side", "join", "attn+fork"] + _block16(0) + \
        ["qkv1@main", "qkv1@side", "join", "attn+fork"] + _block16(1) + ["join", "cast"]
    steps, _, _ = query("fp16", 1024, 16, 257, False, 2, 55, "cls", lane=1)
    assert _order(steps) == ["stats_cast", "fork", "qkv0@main", "qkv0@side", "join", "attn+fork"] + \
        [s for s in _block16(0) if "tap" not in s] + ["qkv1@main", "qkv1@side", "join", "cast", "attn", "out1@main", "ln21@main",
                                                      "fc1@main", "proj1@main"]


def test_enqueue_order_fp8():
    steps, _, _ = query("fp8", 1024, 16, 257, False, 2, 55, "all", taps=True, lane=1)
    assert _order(steps) == ["stats_cast", "quant", "fork", "qkv0@main", "qkv0@side", "join", "attn+fork"] + _block16(0) + \
        ["qkv1@main", "qkv1@side", "join", "attn+fork"] + _block16(1) + ["join", "cast"]
    assert [s["op"] for s in steps if OPNAME[s["op"]] == "gemm"][:2] == [GEMM_MX, GEMM16]
    steps, _, _ = query("fp8", 256, 4, 77, True, 2, 7, "readout", lane=1)      # 539 rows: 512 on the MXFP8 kernels, 27 on the side lane
    assert _order(steps) == ["stats_cast", "quant", "fork", "qkv0@main", "qkv0@side", "join", "attn+fork"] + \
        [s for s in _block16(0) if "tap" not in s] + ["qkv1@main", "qkv1@side", "join", "attn", "gather", "gather", "out1@main", "ln21@main",
                                                      "fc1@main", "proj1@main", "copy"]


def test_enqueue_order_x3():
    def chain(l, lane, nxt):
        c = [f"out{l}@{lane}", f"ln2{l}@{lane}", f"fc{l}@{lane}", f"proj{l}@{lane}", f"tap{l}@{lane}"]
        return c + ([f"ln1{nxt}@{lane}", f"qkv{nxt}@{lane}"] if nxt is not None else [])
    steps, _, _ = query("x3", 256, 4, 17, False, 2, 16, "all", taps=True, split=1, lane=1)
    assert _order(steps) == ["fork", "ln10@main", "qkv0@main", "ln10@side", "qkv0@side", "join", "attn", "fork"] + chain(0, "main", 1) + \
        chain(0, "side", 1) + ["join", "attn", "fork"] + chain(1, "main", None) + chain(1, "side", None) + ["join"]
    steps, _, _ = query("x3", 256, 4, 17, False, 2, 16, "cls", split=1, lane=1)
    assert _order(steps) == ["fork", "ln10@main", "qkv0@main", "ln10@side", "qkv0@side", "join", "attn", "fork"] + \
        [s for s in chain(0, "main", 1) + chain(0, "side", 1) if "tap" not in s] + \
        ["join", "attn", "copy", "copy", "split", "out1@main", "ln21@main", "fc1@main", "proj1@main", "copy"]
    packed, _, _ = query("x3", 256, 4, 77, True, 1, 7, "readout", packed=(512, 257), lane=1)
    assert _order(packed) == ["zero", "ln10@main", "qkv0@main", "attn", "gather", "gather", "split", "out0@main", "ln20@main", "fc0@main",
                              "proj0@main", "copy"]


# ---- (b) the comparison can fail ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,flow,kind,kw", _mutation_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_mutated_plans_compare_unequal(name, flow, kind, kw):
    assert compare(flow, kind, kw, True) is None
    assert compare(flow, kind, kw, True, mutation=name) is not None


# ---- (c) no race in the plan --------------------------------------------------------------------------------------------------------
def _accesses(s, table, M, Mp):
    """[(buffer, first row, last row, writes)] of a step; aliases resolve to rows of the buffer they live in, statistics included;
    strided and plane accesses are widened to the range they span (conservative)"""
    op = s["op"]
    acc = []

    def touch(buf, r0, n, step, write):
        if not buf:
            return
        name = BUF[buf]
        lo, hi = r0, r0 + (n - 1) * step
        off, nbytes, alias = table[name]
        if alias:
            aoff, abytes, _ = table[alias]
            row_bytes = abytes // Mp
            lo, hi, name = (off - aoff) // row_bytes, (off + nbytes - 1 - aoff) // row_bytes, alias
            for other, (ooff, obytes, oalias) in table.items():      # an alias that runs on over the buffers behind: all of each
                if other != alias and not oalias and ooff >= 0 and obytes and max(off, ooff) < min(off + nbytes, ooff + obytes):
                    acc.append((other, 0, 1 << 40, write))
        elif s["plane_rows"] and s["plane_rows"] != Mp and name in ("ln", "hid"):
            lo, hi = 0, Mp - 1                   # planes of another stride: anywhere in the buffer
        acc.append((name, lo, hi, write))
    n = s["n"]
    if op in (GEMM16, GEMM_F32) and s["weight"] == 9:      # the patch GEMM spreads its rows over every sample's patch rows of x
        touch(s["in"], 0, n, 1, False)
        touch(s["out"], 0, M, 1, True)
    elif op == LN and s["rows"]:                             # a read-out column somewhere in each sample's in_step rows
        touch(s["in"], 0, n * s["in_step"], 1, False)
        touch(s["out"], 0, n, 1, True)
    elif op in (ATTN, ATTN_FORK):
        touch(s["in"], 0, M, 1, False)
        touch(s["out"], 0, M, 1, True)
        touch(s["out2"], 0, max(s["q8_rows"], 1), 1, True)
    elif op == GATHER:
        touch(s["in"], 0, M, 1, False)
        touch(s["out"], 0, n, 1, True)
    elif op not in (FORK, JOIN):
        touch(s["in"], s["in_r0"], n, s["in_step"], False)
        if op != TAP:
            touch(s["out"], s["out_r0"], n, s["out_step"], True)
            touch(s["out2"], s["out_r0"], n, 1, True)
        touch(s["st_read"], s["st_r0"], n, 1, False)
        touch(s["st_add"], s["st_r0"], n, 1, True)
        touch(s["st_clear"], s["st_r0"], n, 1, True)
    return acc



def races(steps, table, M, width):
    """pairs of steps that touch overlapping rows of one buffer, at least one writing, and that the lanes leave unordered.
    Happens-before: the order of each lane; fork: the side lane waits for the main lane's steps so far; join: the reverse;
    attention + fork: the attention on the main lane, then a fork."""
    Mp = table["x"][1] // (4 * width)                             # the rows every buffer is carved for
    seen = {0: [0, 0], 1: [0, 0]}       # per lane: how many steps of (main, side) are known to have happened
    clock, info = [], []
    for s in steps:
        op, lane = s["op"], s["lane"]
        if op not in (FORK, JOIN):
            seen[lane][lane] += 1
            clock.append((lane, seen[lane][lane], tuple(seen[lane])))
            info.append((s, _accesses(s, table, M, Mp)))
        if op in (FORK, ATTN_FORK):
            seen[1][0] = max(seen[1][0], seen[0][0])
        if op == JOIN:
            seen[0][1] = max(seen[0][1], seen[1][1])
    bad = []
    for j in range(len(info)):
        for i in range(j):
            (la, ia, _), (_, _, vb) = clock[i], clock[j]
            if vb[la] >= ia:
                continue                                           # step i happened before step j
            for ba, lo_a, hi_a, wa in info[i][1]:
                for bb, lo_b, hi_b, wb in info[j][1]:
                    if ba == bb and (wa or wb) and lo_a <= hi_b and lo_b <= hi_a:
                        bad.append((i, j, ba))
    return bad


def _race_cases():
    seen, out = set(), []
    for flow, kind, kw, _ in _plan_cases():
        key = (flow, kind, str(kw))
        if key not in seen:
            seen.add(key)
            out.append((flow, kind, kw))
    return out


@pytest.mark.parametrize("flow,kind,kw", _race_cases(), ids=_ID)
def test_no_two_steps_race(flow, kind, kw):
    split = bool(kw.get("split")) and flow in ("bf16", "fp16", "x3")
    p, args = lib_args(flow, kind, dict(kw, split=split))
    steps, table, _ = query(**args, taps=bool(kw.get("taps")), split=int(split), lane=1)
    assert races(steps, table, p.M, p.w) == []


@pytest.mark.parametrize("flow,S,B", _real_cases())
def test_no_two_steps_race_at_the_geometry_that_splits(flow, S, B):
    steps, table, _ = query(flow, 1024, 16, S, False, 2, B, "all", taps=True, lane=1)
    assert races(steps, table, B * S, 1024) == []


@pytest.mark.parametrize("flow", ("bf16", "fp8", "x3"))
def test_a_missing_join_or_fork_is_a_race(flow):
    steps, table, _ = query(flow, 256, 4, 17, False, 2, 31, "all", taps=True, split=1, lane=1)
    assert races(steps, table, 31 * 17, 256) == []
    joins = [i for i, s in enumerate(steps) if s["op"] == JOIN and i + 1 < len(steps) and steps[i + 1]["op"] in (ATTN, ATTN_FORK)]
    assert len(joins) == 2
    for i in joins:                                                # the attention reads the side lane's q, k, v rows
        bad = races(steps[:i] + steps[i + 1:], table, 31 * 17, 256)
        assert bad and {b for _, _, b in bad} & {"qkv"}
    forks = [i for i, s in enumerate(steps) if s["op"] == ATTN_FORK or (s["op"] == FORK and steps[i - 1]["op"] == ATTN)]
    assert len(forks) == 2
    for i in forks:                                                # the side lane's out-proj reads the attention's output
        cut = steps[:i] + ([dict(steps[i], op=ATTN)] if steps[i]["op"] == ATTN_FORK else []) + steps[i + 1:]
        bad = races(cut, table, 31 * 17, 256)
        assert bad and {b for _, _, b in bad} & {"att", "ln"}


# ---- (d) the buffer table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flow", tc.FLOWS)
@pytest.mark.parametrize("w,S,B", [(256, 17, 1), (256, 17, 31), (256, 77, 7), (512, 17, 4), (1024, 257, 55)])
def test_buffer_table_is_the_carving(flow, w, S, B):
    _, table, ws = query(flow, w, w // 64, S, False, 1, B, "all")
    want = tc.tower_buffers(flow, w, S, B)
    off = 0
    for name, (r, c, t) in want.items():
        assert table[name] == (off, r * c * tc.ESIZE[t], ""), name
        off += tc.pad256(r * c * tc.ESIZE[t])
    assert ws == off == tc.buffers_bytes(want)
    assert {n for n, (_, b, a) in table.items() if b and not a and n != "x"} == {n for n, (r, c, _) in want.items() if r * c}      # nothing else
    assert table["x"] == (-1, tc.pad256(B * S) * w * 4, "")
    # the compact tail buffers: declared aliases inside qkv, 6 B w (16-bit) / 8 B w (fp32) bytes from its start
    q0, qb, _ = table["qkv"]
    e = 4 if flow in ("f32", "x3") else 2
    assert table["att_c"] == (q0, B * w * e, "qkv") and table["x_c"] == (q0 + B * w * e, B * w * 4, "qkv")
    assert q0 + (e + 4) * B * w <= q0 + qb


# ---- (e) arguments ------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    ok = dict(flow="bf16", width=256, heads=4, S=77, causal=True, layers=2, B=7, tail="readout")
    query(**ok, packed=(512, 257))
    query(**dict(ok, flow=6), expect=-1)                           # KEDS_E_ARG: unknown flow
    query(**dict(ok, flow=-1), expect=-1)
    query(**dict(ok, flow="fp8"), packed=(512, 257), expect=-1)    # packed rows on the MXFP8 tower
    query(**dict(ok, causal=False), packed=(512, 257), expect=-1)  # ... on a non-causal tower
    query(**dict(ok, tail="all"), packed=(512, 257), expect=-1)    # ... without a read-out row per sample
    query(**dict(ok, heads=3), expect=-1)
    # fp16 with fp8: the pass itself refuses the parameters before it touches a device
    lib = _lib.load()
    blocks = (_lib.BlockParams * 2)()
    tp = _lib.TowerParams(256, 2, 4, 77, 1, blocks, 1, 0, 0, 1)
    assert lib.keds_tower_forward(C.byref(tp), C.c_void_p(256), 1, C.c_void_p(256), C.c_size_t(1 << 40), None) == -1


# ---- (f) whole passes: keds_pass_plan_query against tower_check.plan_pass -------------------------------------------------------------
# The front end and the read-out of the model, step -> record:
#   im2col  -> IM2COL (src -> col, B x patches rows, [3] the operand type 0 bf16 / 1 fp32 / 2 fp16);  patch -> a GEMM of weight 9 (conv1)
#   cls     -> CLS (B rows of x, S apart);  ln with layer None -> LN of weight 10 (ln_pre, in place, fp32) or 11 (ln_final into tok)
#   embed   -> EMBED (src -> x, B x the columns that run, [19] packed)
#   readout -> LN of weight 11 into ro ([6] the row step, [23] the read-out columns), a GEMM of weight 12 into out, L2NORM where asked
PASS_ID = {"tower": 0, "vit": 1, "vit_tokens": 2, "text": 3, "text_packed": 4, "text_tokens": 5}
TYPE = {"bf16": 0, "fp32": 1, "fp16": 2}
E, L = 128, 77
NAME = {"tokens_out": "tok"}


def pass_query(flow, kind, B, width=W, heads=HEADS, layers=LAYERS, res=56, patch=14, embed_dim=E, seq_used=0, trim=1, lens=None, seq_max=None,
               splice=None, normalize=0, cls_only=True, out_type=1, readout=1, split=-1, lane=-1, expect=0):
    """-> (steps as dicts, buffers {name: (offset, bytes, alias-of name)}, workspace bytes) of a whole pass"""
    lib = _lib.load()
    vit = kind in ("vit", "vit_tokens")
    q = _lib.PassShape(kind=PASS_ID[kind], flow=FLOW_ID[flow], width=width, heads=heads, layers=layers, B=B, causal=int(not vit),
                       seq=(res // patch) ** 2 + 1 if vit else 0, resolution=res, patch=patch, kpad=(3 * patch * patch + 63) // 64 * 64,
                       embed_dim=embed_dim, context=0 if vit else L, seq_used=seq_max if kind == "text_packed" else seq_used, trim=trim,
                       rows_total=sum(lens) if lens else 0, n_tok=splice[0] if splice else 0, insert_col=splice[1] if splice else 0,
                       cls_only=int(cls_only and kind == "vit"), readout=readout, normalize=normalize, out_type=out_type, split=split, lane=lane)
    cap = 4096
    rec = np.zeros((cap, len(FIELDS)), dtype=np.int32)
    bufs = np.zeros((len(BUF), 4), dtype=np.int64)
    n, ws = C.c_int(0), C.c_size_t(0)
    rc = lib.keds_pass_plan_query(C.byref(q), rec.ctypes.data, cap, C.byref(n), bufs.ctypes.data, C.byref(ws))
    assert rc == expect, rc
    if rc:
        return None
    assert 0 < n.value <= cap
    steps = [dict(zip(FIELDS, (int(v) for v in r))) for r in rec[:n.value]]
    return steps, {BUF[int(i)]: (int(o), int(b), BUF[int(al)]) for i, o, b, al in bufs if i}, ws.value


def canon_pass_py(s, p, lane_on, out_type):
    """-> the canonical forms of one step of plan_pass (the read-out is up to three launches)"""
    name, f32, h = s["op"], p.flow in ("f32", "x3"), p.flow == "fp16"
    kern = "f32" if f32 else "16"
    if name == "im2col":
        return [(name, "src", "col", p.B * (p.S - 1), TYPE[p.buffers["col"][2]])]
    if name == "patch":
        epi = _lib.F32_EPI_PATCH if f32 else _lib.EPI_PATCH_F32_H if h else _lib.EPI_PATCH_F32
        return [("gemm", -1, "conv", False, kern, epi, ("col", 0, 1), ("x", 0, 1), p.B * s["G"], "", None, 0)]
    if name == "cls":
        return [(name, ("x", 0, p.S), p.B)]
    if name == "embed":
        return [(name, "src", "x", p.B * s["Lx"], s["packed"])]
    if name == "ln" and s["layer"] is None:
        dst = (NAME.get(s["dst"][0], s["dst"][0]),) + tuple(s["dst"][1:])
        pre = s["g"] == "ln_pre"
        return [("ln", -1, "ln_pre" if pre else "ln_out", s["src"], dst, s["n"], 0, "rows", 0, 1 if pre else out_type)]
    if name == "readout":
        t = 1 if f32 else 2 if h else 0
        epi = _lib.F32_EPI_BIAS if f32 else _lib.EPI_BIAS_F32_H if h else _lib.EPI_BIAS_F32
        out = [("ln", -1, "ln_out", ("x", 0, s["S"]), ("ro", 0, 1), p.B, 0, "rows", int(bool(s["rows"])), t),
               ("gemm", -1, "proj_t", False, kern, epi, ("ro", 0, 1), ("out", 0, 1), p.B, "", None, 0)]
        return out + ([("l2norm", "out", "out", p.B, int(f32))] if s["normalize"] else [])
    return [canon_py(s, p, lane_on)]


def model_split(flow, M, w):
    """the three rules of tower_splits_rows restated (test_plan_at_the_geometry_that_splits)"""
    gs = _gemm_splits_rows()
    if flow == "x3":
        return bool(0 < M // 256 * 256 < M and gs(M, 3 * w, w))
    if flow == "fp8":
        return M >= 256 and M % 256 != 0
    return flow in ("bf16", "fp16") and all(gs(M, n, k) for n, k in ((3 * w, w), (w, w), (4 * w, w), (w, 4 * w)))


def pass_pair(flow, kind, B, lane, out_type=1, mutation=None, **kw):
    """-> (the library's steps, its table, its bytes, the model plan) of one pass; the model's split is the restated rule"""
    vit = kind in ("vit", "vit_tokens")
    geo = {k: kw[k] for k in ("width", "heads", "res") if k in kw}
    w = geo.get("width", W)
    if vit:
        S = (geo.get("res", 56) // 14) ** 2 + 1
        M = B * S
    elif kind == "text_packed":
        M = None                                                   # (bf16 / fp16 / x3 at width 256 and < 256 x 4 rows: never split)
    else:
        tr, su = kw.get("trim", 1), kw.get("seq_used", 0)
        M = B * (su if kind == "text" and tr in (1, 2) and 0 < su < L else L)
    split = bool(lane) and M is not None and model_split(flow, M, w)
    mkw = {k: v for k, v in kw.items() if k in ("seq_used", "trim", "lens", "seq_max", "splice", "normalize", "cls_only", "rows")}
    p = tc.plan_pass(flow, kind, kw.get("layers", LAYERS), B, embed_dim=kw.get("embed_dim", E), split=split, **geo, **mkw)
    if mutation:
        p = tc.mutate_pass(p, mutation)
    qkw = {k: v for k, v in kw.items() if k != "rows"}
    steps, table, ws = pass_query(flow, kind, B, lane=int(lane), out_type=out_type, **qkw)
    return steps, table, ws, p


def compare_pass(flow, kind, B, lane, out_type=1, mutation=None, **kw):
    steps, _, _, p = pass_pair(flow, kind, B, lane, out_type, mutation, **kw)
    if not lane:
        assert all(s["lane"] == 0 and s["op"] not in (FORK, JOIN, ATTN_FORK) for s in steps)
    a = segments([canon_lib(s) for s in steps])
    b = segments([c for s in p.steps for c in canon_pass_py(s, p, lane, out_type)])
    if len(a) != len(b):
        return f"{len(a)} segments, {len(b)} in the model"
    for i, ((ca, sa), (cb, sb)) in enumerate(zip(a, b)):
        if ca != cb:
            return f"segment {i}: cut {ca} != {cb}"
        if sa != sb:
            return f"segment {i}: {sa} != {sb}"
    return None


def expected_table(p, kind, flow, out_type=1, res=56):
    """the pass workspace written from the model's buffers: x | the tower scratch (col aliases its head) | ro, 256-byte aligned"""
    al = tc.pad256
    B, S, w = p.B, p.S, p.w
    x_bytes = al(B * S) * w * 4
    exp, off = {"x": (0, x_bytes, "")}, al(x_bytes)
    first = None
    for name, (r, c, t) in tc.tower_buffers(flow, w, S, B).items():
        first = first or name
        if r * c:
            exp[name] = (off, r * c * tc.ESIZE[t], "")
        off += al(r * c * tc.ESIZE[t])
    e = 4 if flow in ("f32", "x3") else 2
    q0 = exp["qkv"][0]
    exp["att_c"], exp["x_c"] = (q0, B * w * e, "qkv"), (q0 + B * w * e, B * w * 4, "qkv")
    if kind in ("vit", "vit_tokens"):
        r, c, t = p.buffers["col"]
        exp["col"] = (al(x_bytes), r * c * tc.ESIZE[t], first)
        off = max(off, al(x_bytes) + al(r * c * tc.ESIZE[t]))
        exp["src"] = (-1, B * 3 * res * res * 4, "")
    else:
        exp["src"] = (-1, B * p.L * 4, "")
    r, c, t = p.buffers["ro"]
    exp["ro"] = (off, r * c * tc.ESIZE[t], "")
    if kind == "text_tokens":
        exp["tok"] = (-1, B * p.L * w * (4 if out_type == 1 else 2), "")
    else:
        exp["out"] = (-1, B * p.E * 4, "")
    return exp, off + al(r * c * tc.ESIZE[t])


def check_pass(flow, kind, B, out_type=1, **kw):
    """steps, buffers and races of one pass, with and without the side lane"""
    for lane in (True, False):
        assert compare_pass(flow, kind, B, lane, out_type, **kw) is None, (flow, kind, B, lane, kw)
    steps, table, ws, p = pass_pair(flow, kind, B, True, out_type, **kw)
    exp, total = expected_table(p, kind, flow, out_type, kw.get("res", 56))
    assert {n: v for n, v in table.items() if v[1]} == exp and ws == total, (flow, kind, B, kw)
    assert races(steps, table, p.M, p.w) == [], (flow, kind, B, kw)
    return steps, table, p


@pytest.mark.parametrize("flow", tc.FLOWS)
@pytest.mark.parametrize("B", (1, 15, 16, 31))
def test_vit_pass_plans_are_the_model(flow, B):
    for normalize in (0, 1):
        for cls_only in (True, False):
            check_pass(flow, "vit", B, normalize=normalize, cls_only=cls_only)
        for out_type in (0, 1, 2):
            check_pass(flow, "vit_tokens", B, out_type, normalize=normalize)


@pytest.mark.parametrize("flow", tc.FLOWS)
@pytest.mark.parametrize("B", (1, 15, 16, 31))
def test_text_pass_plans_are_the_model(flow, B):
    for trim in (0, 1, 2, 3):
        for seq_used in (0, 1, 43, 77):
            for splice in (None, (2, 1), (3, 1)):
                check_pass(flow, "text", B, trim=trim, seq_used=seq_used, splice=splice, normalize=int(splice is None))
    for out_type in (0, 1, 2):
        check_pass(flow, "text_tokens", B, out_type)


@pytest.mark.parametrize("flow", ("bf16", "unfolded", "fp16", "f32", "x3"))
@pytest.mark.parametrize("lens,seq_max", [(LENS_256, 77), (LENS_257, 77), (LENS_MAX60, 60)], ids=("256", "257", "max60"))
def test_packed_text_pass_plans_are_the_model(flow, lens, seq_max):
    for splice in (None, (2, 1), (3, 1)):
        for normalize in (0, 1):
            steps, _, _ = check_pass(flow, "text_packed", len(lens), lens=lens, seq_max=seq_max, splice=splice, normalize=normalize)
            names = [OPNAME[s["op"]] for s in steps]
            if sum(lens) % 256:                                    # the zero rows of x are cleared in front of the embedding
                assert names.index("zero") < names.index("embed") and BUF[steps[names.index("zero")]["out"]] == "x"
    pass_query(flow, "text_packed", len(lens), lens=lens, seq_max=seq_max, trim=0, expect=-1)
    pass_query("fp8", "text_packed", len(lens), lens=lens, seq_max=seq_max, expect=-1)


@pytest.mark.parametrize("flow", ("bf16", "fp16", "fp8", "x3"))
def test_vit_pass_plans_at_the_geometry_that_splits(flow):
    """ViT-L/14, B = 128: 32,896 rows = 128 full tiles + 128 remainder rows on the side lane"""
    geo = dict(width=1024, heads=16, res=224, embed_dim=768, layers=2)
    assert model_split(flow, 128 * 257, 1024)
    for kind, kw in (("vit", dict(cls_only=True, normalize=1)), ("vit", dict(cls_only=False)), ("vit_tokens", {})):
        steps, _, _ = check_pass(flow, kind, 128, **geo, **kw)
        assert {s["lane"] for s in steps} == {0, 1}
        assert all(s["lane"] == 0 for s in steps if s["layer"] < 0)              # the front end and the read-out: the caller's stream


VITL = dict(width=1024, heads=16, res=224, embed_dim=768, layers=1)


# ---- the enqueue order of a whole pass, and what keeps its aliases and lanes apart ---------------------------------------------------
def test_enqueue_order_of_whole_passes():
    steps, _, _ = pass_query("bf16", "vit", 3, layers=1, normalize=1, lane=1)
    assert _order(steps) == ["im2col", "conv-1@main", "cls", "ln_pre-1@main", "stats_cast", "qkv0@main", "cast", "attn", "out0@main", "ln20@main",
                             "fc0@main", "proj0@main", "ln_out-1@main", "proj_t-1@main", "l2norm"]
    steps, _, _ = pass_query("f32", "text_packed", 7, layers=1, lens=LENS_257, seq_max=77, lane=1)
    assert _order(steps) == ["zero", "embed", "zero", "ln10@main", "qkv0@main", "attn", "gather", "gather", "out0@main", "ln20@main", "fc0@main",
                             "proj0@main", "copy", "ln_out-1@main", "proj_t-1@main"]
    steps, _, _ = pass_query("unfolded", "text_tokens", 2, layers=1, lane=1)
    assert _order(steps) == ["embed", "ln10@main", "qkv0@main", "attn", "out0@main", "ln20@main", "fc0@main", "proj0@main", "ln_out-1@main"]
    steps, _, _ = pass_query("bf16", "vit_tokens", 2, layers=1, readout=0, lane=1)
    assert _order(steps)[-3:] == ["proj0@main", "tap0@main", "cast"]


@pytest.mark.parametrize("flow", tc.FLOWS)
@pytest.mark.parametrize("geo", (dict(), VITL), ids=("w256", "vitl"))
def test_col_is_dead_before_the_scratch_it_aliases_is_written(flow, geo):
    """the im2col matrix starts where the tower scratch starts: its last reader (the patch GEMM) is enqueued on the caller's stream in
    front of the first step that writes a scratch buffer it overlaps, and no step on the side lane comes before that"""
    steps, table, _ = pass_query(flow, "vit", 16, lane=1, **geo)
    c0, cb, alias = table["col"]
    assert alias == ("ln" if flow in ("f32", "x3") else "h") and c0 == table[alias][0] and cb > 0
    over = {n for n, (o, b, a) in table.items() if n != "col" and not a and o >= 0 and b and max(o, c0) < min(o + b, c0 + cb)}
    assert alias in over and "x" not in over and "ro" not in over
    uses = [i for i, s in enumerate(steps) if "col" in (BUF[s["in"]], BUF[s["out"]])]
    writes = [i for i, s in enumerate(steps) if {BUF[s[k]] for k in ("out", "out2", "st_add", "st_clear")} & over
              or (s["out2"] and BUF[s["out2"] + 1] in over)]
    assert len(uses) == 2 and writes and max(uses) < min(writes)
    assert all(s["lane"] == 0 and s["op"] not in (FORK, ATTN_FORK) for s in steps[:min(writes)])


@pytest.mark.parametrize("flow,kind,kw", [("fp8", "vit_tokens", {}), ("fp8", "vit", dict(cls_only=False)), ("fp8", "text", dict(trim=0)),
                                          ("fp8", "text_tokens", {}), ("bf16", "vit", dict(VITL, cls_only=False)),
                                          ("fp16", "vit_tokens", VITL)], ids=lambda v: v if isinstance(v, str) else "")
def test_the_read_out_waits_for_the_side_lane(flow, kind, kw):
    """every row of the stream is written before the read-out's LayerNorm reads its rows: without the join behind the last block the
    side lane's c_proj and the read-out (16-bit flows: the cast in front of it) are unordered"""
    B = 128 if "width" in kw else 31 if kind.startswith("vit") else 7
    steps, table, _, p = pass_pair(flow, kind, B, True, **kw)
    assert {s["lane"] for s in steps} == {0, 1} and races(steps, table, p.M, p.w) == []
    last = max(i for i, s in enumerate(steps) if s["op"] == JOIN)
    tail = [OPNAME[s["op"]] for s in steps[last + 1:]]
    assert set(tail) <= {"cast", "ln", "gemm", "l2norm"} and "ln" in tail
    bad = races(steps[:last] + steps[last + 1:], table, p.M, p.w)
    assert bad and {b for _, _, b in bad} <= {"x", "h"}


@pytest.mark.parametrize("name,flow,kind,kw", [
    ("cls_dropped", "bf16", "vit", {}), ("cls_dropped", "x3", "vit_tokens", {}), ("no_ln_pre", "fp16", "vit", {}), ("no_ln_pre", "f32", "vit", {}),
    ("embed_before_zero", "bf16", "text_packed", dict(lens=LENS_257, seq_max=77)),
    ("embed_before_zero", "x3", "text_packed", dict(lens=LENS_MAX60, seq_max=60)),
    ("readout_stride_plus1", "bf16", "vit", {}), ("readout_stride_plus1", "fp8", "text", dict(trim=0)),
    ("readout_stride_plus1", "f32", "text", dict(trim=1, seq_used=43)), ("no_l2norm", "bf16", "vit", dict(normalize=1)),
    ("no_l2norm", "x3", "text", dict(normalize=1))], ids=lambda v: v if isinstance(v, str) else "")
def test_mutated_pass_plans_compare_unequal(name, flow, kind, kw):
    B = len(kw["lens"]) if "lens" in kw else 7
    assert compare_pass(flow, kind, B, True, **kw) is None
    assert compare_pass(flow, kind, B, True, mutation=name, **kw) is not None


# ---- the workspaces of the passes: the sizes of the commit before the pass plan existed, as literals ---------------------------------
WS_BEFORE = {   # (kind, f32, width, B) -> bytes; width 256: 3 layers, 56 / 14 px (S = 17), L = 77, embed_dim 128; ViT-L/14 and its text tower at B = 128
    ("vit", 0, 256, 1): 9904128, ("text", 0, 256, 1): 9904128, ("vit", 0, 256, 15): 9904128, ("text", 0, 256, 15): 17326080,
    ("vit", 0, 256, 16): 11759616, ("text", 0, 256, 16): 17326080, ("vit", 0, 256, 31): 13615104, ("text", 0, 256, 31): 26603520,
    ("vit", 0, 1024, 128): 961290240, ("text", 0, 768, 128): 223821824,
    ("vit", 1, 256, 1): 2752512, ("text", 1, 256, 1): 2752512, ("vit", 1, 256, 15): 2752512, ("text", 1, 256, 15): 13238272,
    ("vit", 1, 256, 16): 5373952, ("text", 1, 256, 16): 13238272, ("vit", 1, 256, 31): 7995392, ("text", 1, 256, 31): 26345472,
    ("vit", 1, 1024, 128): 1353187328, ("text", 1, 768, 128): 307101696,
    ("vit", 2, 256, 1): 2752512, ("text", 2, 256, 1): 2752512, ("vit", 2, 256, 15): 2752512, ("text", 2, 256, 15): 13238272,
    ("vit", 2, 256, 16): 5373952, ("text", 2, 256, 16): 13238272, ("vit", 2, 256, 31): 7995392, ("text", 2, 256, 31): 26345472,
    ("vit", 2, 1024, 128): 1353187328, ("text", 2, 768, 128): 307101696}


@pytest.mark.parametrize("key", sorted(WS_BEFORE), ids=lambda k: "-".join(str(v) for v in k))
def test_pass_workspaces_are_what_they_were(key):
    kind, f32, w, B = key
    lib = _lib.load()
    small = w == 256
    heads, res, emb = w // 64, 56 if small else 224, E if small else 768
    flows = {0: ("bf16", "unfolded", "fp16", "fp8"), 1: ("f32",), 2: ("x3",)}[f32]
    if kind == "vit":
        tp = _lib.TowerParams(w, 3, heads, (res // 14) ** 2 + 1, 0, None, 0, 0, f32, 0)
        assert lib.keds_vit_workspace_bytes(C.byref(_lib.VitParams(tp, res, 14, 640, emb)), B) == WS_BEFORE[key]
        for flow in flows:
            _, table, ws = pass_query(flow, "vit", B, width=w, heads=heads, res=res, embed_dim=emb)
            assert ws == WS_BEFORE[key]
            assert sum(tc.pad256(b) for n, (o, b, a) in table.items() if o >= 0 and not a) + \
                max(0, tc.pad256(table["col"][1]) - (table["ro"][0] - table["col"][0])) == WS_BEFORE[key]
    else:
        tp = _lib.TowerParams(w, 3, heads, L, 1, None, 0, 0, f32, 0)
        assert lib.keds_text_workspace_bytes(C.byref(_lib.TextParams(tp, 512, emb)), B) == WS_BEFORE[key]
        for flow in flows:
            for kind_, kw in (("text", dict(trim=0)), ("text", dict(trim=1, seq_used=0)), ("text_tokens", {})):
                _, table, ws = pass_query(flow, kind_, B, width=w, heads=heads, embed_dim=emb, **kw)
                assert ws == WS_BEFORE[key] == sum(tc.pad256(b) for n, (o, b, a) in table.items() if o >= 0 and not a)


# ---- the packed-rows rule at its edge -----------------------------------------------------------------------------------------------
def test_packed_rows_rule_at_its_edge():
    """B = 8 captions, the longest 40 columns: packed rows from an eighth fewer rows, 8 x 40 x 7 / 8 = 280"""
    f = _lib.load().keds_text_runs_packed
    assert f(1, 0, 1, 280, 8, 40) == 1 and f(1, 0, 1, 281, 8, 40) == 0
    assert f(1, 1, 1, 280, 8, 40) == 0                             # the MXFP8 tower
    assert [f(1, 0, trim, 280, 8, 40) for trim in (0, 2, 3)] == [0, 0, 0]
    assert f(0, 0, 1, 280, 8, 40) == 0                             # not causal
    assert f(1, 0, 1, 8, 8, 40) == 1 and f(1, 0, 1, 7 * (1 << 31) // 8, 1 << 16, 1 << 15) == 1      # 64-bit products


def test_x3_chunk_is_the_old_expression():
    from keds_amd.model import x3_chunk
    for width in range(256, 1281, 64):
        for rows in (17, 50, 77, 197, 257, 577, 1 << 20):
            assert x3_chunk(width, rows) == max(1, ((1 << 31) // (8 * width) - 512) // rows)
