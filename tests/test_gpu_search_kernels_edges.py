"""Every kernel of keds_amd/csrc/search.hip alone at its list, cut and certificate edges, through the stage entries (keds_search_*):
tests/search_check.py holds the float64 references, the bounds and the regimes; tests/test_host_search_check.py shows that the checks
pass CPU models of the stages and catch their mutations.

Every output sits in a sentinel-filled buffer with 256 guard elements on both sides; what a kernel is not meant to write must survive.
The worst ratio to the bound per kernel and regime goes to the metrics log.  Two compositions close the file: the stage entries chained
by keds_index_search_plan_query reproduce keds_index_search_packed_ex bit for bit, and on those runs the certificate's premise
(|scan score - exact score| <= eps), its claim (a certified query has no better row outside its candidates) and the result hold
against float64 on the original rows."""
import ctypes as C

import numpy as np
import pytest
import torch

from keds_amd import _lib
from tests import search_check as sc
from tests.gpu_util import report

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = 256
SENT64 = 0x5EA5C0DE5EA5C0DE
SENT32 = 0x5EA5C0DE
SENTF = 7.25
P = _lib.ptr


def _done(rc_, what):
    """a failed launch or a device fault: nothing more of this session may run on the card"""
    try:
        _lib.check(rc_, what)
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what}: {e}", returncode=3)


def _buf(numel, dtype, fill):
    """-> (whole 1-D buffer with G guard elements on both sides, view of the `numel` elements between them)"""
    whole = torch.full((numel + 2 * G,), fill, dtype=dtype, device=DEV)
    return whole, whole[G:G + numel]


def _guards_ok(whole, fill):
    return bool((whole[:G] == fill).all()) and bool((whole[-G:] == fill).all())


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev(a, keep=None):
    """a host array on the device; `keep` (a list) holds the tensor until the caller is done with the launch that reads it"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    if keep is not None:
        keep.append(t)
    return t


class Tally:
    def __init__(self, label):
        self.label, self.msgs, self.worst, self.launches = label, [], {}, 0

    def add(self, key, msgs, worst=0.0, guards=True, what=""):
        self.launches += 1
        self.msgs += [f"{what}{m}" for m in msgs]
        if not guards:
            self.msgs.append(f"{what}written outside the output buffer")
        self.worst[key] = max(self.worst.get(key, 0.0), worst)

    def finish(self):
        for key, w in sorted(self.worst.items()):
            report(f"search_edges.{self.label}.{key}", worst_ratio=w)
        assert self.launches > 0
        assert not self.msgs, f"{len(self.msgs)} failures:\n" + "\n".join(self.msgs[:30])


def _pack(x, metric, append_from=0):
    """-> (rows on the device, the image as a device uint8 tensor, its bytes on the host, guards intact)"""
    lib = _lib.load()
    n, dim = x.shape
    nbytes = sc.packed_bytes(n, dim)
    assert nbytes == lib.keds_index_packed_bytes(n, dim)
    whole, img = _buf(nbytes, torch.uint8, 0xA5)
    rows = _dev(x)
    if append_from:
        _done(lib.keds_index_pack(P(rows), append_from, dim, metric, img.data_ptr(), _lib.stream()), "keds_index_pack (first part)")
        old = sc.packed_bytes(append_from, dim)
        assert bool((img[old:] == 0xA5).all()), "the first pack wrote behind its image"
        _done(lib.keds_index_pack_append(P(rows), append_from, n, dim, metric, img.data_ptr(), _lib.stream()), "keds_index_pack_append")
    else:
        _done(lib.keds_index_pack(P(rows), n, dim, metric, img.data_ptr(), _lib.stream()), "keds_index_pack")
    return rows, img, img.cpu().numpy(), _guards_ok(whole, 0xA5), whole


# ---- pack ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", sc.DIMS)
def test_pack_and_append(dim):
    t = Tally(f"pack.{dim}")
    for n in (1, 31, 32, 33, 1025):
        for metric in (sc.L2, sc.IP):
            for regime in ("integer", "random", "bignorm"):
                x, _ = sc.make_inputs(regime, n, dim, 1)
                _, _, host, ok, _ = _pack(x, metric)
                msgs, worst = sc.pack_failures(x, metric, host)
                t.add(regime, msgs, worst, ok, f"n {n} metric {metric} {regime}: ")
    # appends: no new stage; a new stage (the trailer moves); the extreme row in the old part / in the new part
    for old_n, n, big in ((33, 40, None), (33, 70, None), (33, 70, 3), (33, 70, 69), (31, 32, 0), (32, 33, 32)):
        x, _ = sc.make_inputs("random", n, dim, 1, seed=n)
        if big is not None:
            x[big] *= 50.0
        one = _pack(x, sc.L2)
        two = _pack(x, sc.L2, append_from=old_n)
        same = np.array_equal(one[2], two[2])
        t.add("append", [] if same else [f"append {old_n} -> {n} (extreme row {big}) differs from one pack in {int((one[2] != two[2]).sum())} bytes"],
              0.0, two[3])
        msgs, worst = sc.pack_failures(x, sc.L2, two[2])
        t.add("append", msgs, worst, True, f"append {old_n} -> {n}: ")
    t.finish()


# ---- qprep --------------------------------------------------------------------------------------------------------------------------
def _qprep(q, normalize):
    lib = _lib.load()
    nq, dim = q.shape
    rows = -(-nq // 128) * 128
    wqn, qn = _buf(nq * dim, torch.float32, SENTF)
    wqb, qb = _buf(rows * dim, torch.int16, 0x5EA5)
    wqs, qs = _buf(nq * 4, torch.float32, SENTF)
    wc, cnt = _buf(8, torch.int32, SENT32)
    keep = []
    _done(lib.keds_search_qprep(P(_dev(q, keep)), nq, dim, normalize, qn.data_ptr(), qb.data_ptr(), qs.data_ptr(), cnt.data_ptr(), _lib.stream()),
          "keds_search_qprep")
    ok = all(_guards_ok(w, f) for w, f in ((wqn, SENTF), (wqb, 0x5EA5), (wqs, SENTF), (wc, SENT32)))
    c = cnt.cpu().numpy()
    ok = ok and c[0] == 0 and (c[1:] == SENT32).all()
    return (qn.cpu().numpy().reshape(nq, dim), qb.cpu().numpy().view(np.uint16).reshape(rows, dim), qs.cpu().numpy().reshape(nq, 4), ok,
            (qn, qb, qs))


@pytest.mark.parametrize("dim", sc.DIMS)
def test_qprep(dim):
    t = Tally(f"qprep.{dim}")
    for nq in (1, 127, 128, 129):
        for normalize in (0, 1):
            for regime in ("integer", "random", "bignorm"):
                if regime == "integer" and normalize:
                    continue
                _, q = sc.make_inputs(regime, 4, dim, nq)
                qn, qb, qs, ok, _ = _qprep(q, normalize)
                msgs, worst = sc.qprep_failures(q, normalize, qn, qb, qs)
                t.add(f"{regime}.norm{normalize}", msgs, worst, ok, f"nq {nq} {regime} normalize {normalize}: ")
    # a zero row with normalise: 0 / 0 -- the row is NaN in qn, qb and qstat; its neighbours are untouched by it
    _, q = sc.make_inputs("random", 4, dim, 5)
    q[2] = 0.0
    qn, qb, qs, ok, _ = _qprep(q, 1)
    keep = [0, 1, 3, 4]
    msgs, worst = sc.qprep_failures(q[keep], 1, qn[keep], np.concatenate([qb[keep], qb[5:9]]), qs[keep])
    t.add("zero_row", msgs, worst, ok, "rows beside a zero row: ")
    report(f"search_edges.qprep.{dim}.zero_row", qn_nan=bool(np.isnan(qn[2]).all()), qstat=[float(v) for v in qs[2]])
    t.add("zero_row", [] if np.isnan(qn[2]).all() and np.isnan(qs[2, :3]).all() else ["a zero row normalised is not NaN throughout"])
    t.finish()


# ---- scan ---------------------------------------------------------------------------------------------------------------------------
class ScanData:
    """rows of one regime packed, and the float64 scores of `nq` queries (padded to whole blocks with zero rows) on the stored operands"""

    def __init__(self, regime, n, dim, nq, stages_for_placed=None, nwg_for_placed=1, seed=0):
        keys = sc.placed_keys(n, stages_for_placed or -(-n // 32), nwg_for_placed, dim) if regime == "placed" else ()
        self.x, q = sc.make_inputs(regime, n, dim, nq, seed=seed, placed_keys=tuple(keys))
        self.n, self.dim, self.nq, self.regime = n, dim, nq, regime
        self.nqb = -(-nq // 128)
        qpad = np.zeros((self.nqb * 128, dim), np.float32)
        qpad[:nq] = q
        self.qb = _dev(qpad).bfloat16()
        self.qb_bits = self.qb.view(torch.int16).cpu().numpy().view(np.uint16)
        self.rows, self.img, host, self.pack_ok, self._keep = _pack(self.x, sc.L2)
        d = sc.decode_image(host, n, dim)
        self.keys, self.bias = d["keys"], d["bias"]
        self.s64, self.e64 = sc.scan_scores64(self.keys, self.bias, self.qb_bits)
        self.model_scores = sc.scan_scores_model(self.keys, self.bias, self.qb_bits) if regime == "integer" else None

    def thr(self, kind):
        if kind == "none":
            return None
        nqp = self.nqb * 128
        if kind in ("-inf", "+inf"):
            return np.full(nqp, -np.inf if kind == "-inf" else np.inf, np.float32)
        s = np.where(np.isfinite(self.s64[:, :self.n]), self.s64[:, :self.n], -3e38)
        if kind == "median":
            return np.median(s, axis=1).astype(np.float32)
        return s.max(1).astype(np.float32)                       # "exact": an existing score (integer: exact in fp32), the best one


def _scan(data, stages, nwg, depth, thr):
    lib = _lib.load()
    nqp = data.nqb * 128
    wp, pairs = _buf(nqp * nwg * 4 * depth, torch.int64, SENT64)
    wm, meta = _buf(nqp * nwg * 2, torch.int32, SENT32)
    thr_d = None if thr is None else _dev(thr)
    _done(lib.keds_search_scan(data.img.data_ptr(), data.n, data.dim, stages, P(data.qb), data.nqb, P(thr_d), depth, nwg, pairs.data_ptr(),
                               meta.data_ptr(), _lib.stream()), f"keds_search_scan dim {data.dim} stages {stages} nwg {nwg} depth {depth}")
    ok = _guards_ok(wp, SENT64) and _guards_ok(wm, SENT32)
    return _u64(pairs).reshape(nqp, nwg, 4 * depth), meta.cpu().numpy().view(np.uint32).reshape(nqp, nwg, 2), ok, (pairs, meta)


def _scan_and_check(t, data, stages, nwg, depth, kind, what):
    thr = data.thr(kind)
    pairs, meta, ok, _ = _scan(data, stages, nwg, depth, thr)
    msgs, worst = sc.scan_failures(data.s64, data.e64, data.n, stages, nwg, depth, thr, pairs, meta, SENT64)
    if data.regime == "integer":
        mp, mm = sc.scan_lists_model(data.model_scores, data.n, stages, nwg, depth, thr, SENT64)
        if not (np.array_equal(mp, pairs) and np.array_equal(mm, meta)):
            msgs.append(f"differs from the integer model in {int((mp != pairs).sum())} pairs, {int((mm != meta).sum())} meta words")
    t.add(data.regime, msgs, worst, ok and data.pack_ok, what)
    return pairs, meta


THR_KINDS = ("none", "-inf", "median", "exact", "+inf")


@pytest.mark.parametrize("dim", sc.DIMS)
def test_scan_ring_lists_and_output(dim):
    """stages per workgroup around the ring depth, uneven splits, every list depth, every threshold kind, every regime"""
    t = Tally(f"scan.{dim}")
    nst = sc.ring_depth(dim)
    spw = sorted({1, max(nst - 1, 1), nst, nst + 1, 2 * nst + 1})
    shapes = [(s * nwg, nwg) for s in spw for nwg in (1, 2, 7)] + [(3 * nwg + 1, nwg) for nwg in (2, 7)] + [(256, 256), (8192 // 32, 7)]
    i = 0
    for stages, nwg in shapes:
        n = stages * 32 - (0, 31, 1)[i % 3]                       # n mod 32 = 0, 1, 31 in turn
        regime = sc.REGIMES[i % len(sc.REGIMES)]
        data = ScanData(regime, n, dim, 8, stages_for_placed=stages, nwg_for_placed=nwg, seed=i)
        for depth in (1, 4, 16):
            kind = THR_KINDS[(i + depth) % len(THR_KINDS)] if regime != "integer" or depth != 16 else "exact"
            _scan_and_check(t, data, stages, nwg, depth, kind, f"{regime} stages {stages} nwg {nwg} n {n} depth {depth} thr {kind}: ")
        i += 1
    # every regime x every threshold kind at depth 16 over 2 NST + 1 stages per workgroup, a partial last stage
    stages, nwg = 2 * (2 * nst + 1), 2
    for regime in sc.REGIMES:
        data = ScanData(regime, stages * 32 - 31, dim, 8, stages_for_placed=stages, nwg_for_placed=nwg)
        for kind in THR_KINDS:
            for depth in ((16,) if kind != "none" else (1, 4, 16)):
                _scan_and_check(t, data, stages, nwg, depth, kind, f"{regime} depth {depth} thr {kind}: ")
    # a prefix of the image only (the threshold pass scans stages [0, stagesA))
    data = ScanData("random", 40 * 32 - 5, dim, 129)
    _scan_and_check(t, data, 13, 2, 4, "none", "prefix of 13 stages, two query blocks: ")
    _scan_and_check(t, data, 40, 7, 16, "median", "two query blocks: ")
    if dim == 128:
        data = ScanData("random", 700, dim, 1024)
        _scan_and_check(t, data, 22, 2, 16, "median", "eight query blocks: ")
        _scan_and_check(t, data, 22, 3, 1, "none", "eight query blocks, depth 1: ")
    if dim == 768:                                                # both cache policies of the candidate pass's key stream
        lib = _lib.load()
        data = ScanData("random", 21 * 32 - 31, dim, 1)
        a = _scan_and_check(t, data, 21, 3, 16, "none", "non-temporal key stream: ")
        try:
            lib.keds_scan_debug(1 << 6)
            b = _scan_and_check(t, data, 21, 3, 16, "none", "default-policy key stream: ")
        finally:
            lib.keds_scan_debug(0)
        t.add("random", [] if np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) else ["the two cache policies give different lists"])
    t.finish()


def test_scan_refuses_bad_arguments():
    lib = _lib.load()
    data = ScanData("random", 64, 128, 1)
    _, pairs = _buf(128 * 2 * 64, torch.int64, SENT64)
    _, meta = _buf(128 * 2 * 2, torch.int32, SENT32)
    good = dict(n=64, dim=128, stages=2, nqb=1, depth=16, nwg=2)
    for bad in (dict(stages=3), dict(stages=0), dict(nwg=3), dict(nwg=0), dict(nwg=257), dict(depth=8), dict(nqb=0), dict(nqb=9), dict(dim=192),
                dict(n=0)):
        a = dict(good, **bad)
        rc_ = lib.keds_search_scan(data.img.data_ptr(), a["n"], a["dim"], a["stages"], P(data.qb), a["nqb"], None, a["depth"], a["nwg"],
                                   pairs.data_ptr(), meta.data_ptr(), _lib.stream())
        assert rc_ != 0, bad
    # the 2 GiB span: 1024-wide stages of 65,664 bytes, 32,704 or more per workgroup (the arguments alone decide; nothing is launched)
    assert lib.keds_search_scan(data.img.data_ptr(), 2048 * 16384, 1024, 1048576, P(data.qb), 1, None, 16, 32, pairs.data_ptr(),
                                meta.data_ptr(), _lib.stream()) != 0
    assert "2 GiB" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((pairs == SENT64).all()) and bool((meta == SENT32).all())
    one = torch.zeros(64, dtype=torch.int32, device=DEV)
    onef = torch.zeros(64, dtype=torch.float32, device=DEV)
    assert lib.keds_search_merge(pairs.data_ptr(), meta.data_ptr(), 1, 257, 64, 64, None, P(one), P(onef), None, None, _lib.stream()) != 0
    assert lib.keds_search_merge(pairs.data_ptr(), meta.data_ptr(), 1, 2, 32, 64, None, P(one), P(onef), None, None, _lib.stream()) != 0
    assert lib.keds_search_merge(pairs.data_ptr(), meta.data_ptr(), 1, 2, 64, 128, None, P(one), P(onef), None, None, _lib.stream()) != 0
    assert lib.keds_search_exact(P(data.rows), 64, 128, 0, P(data.rows), P(one), P(one), P(onef), 0, 1, 0, pairs.data_ptr(), P(one), P(onef),
                                 pairs.data_ptr(), _lib.stream()) != 0
    assert lib.keds_search_exact(P(data.rows), 5000, 128, 0, P(data.rows), P(one), P(one), P(onef), 2, 1, 0, pairs.data_ptr(), P(one), P(onef),
                                 pairs.data_ptr(), _lib.stream()) != 0                      # 2,500 chunks
    torch.cuda.synchronize()


# ---- merge --------------------------------------------------------------------------------------------------------------------------
def _merge(pairs, meta, ncand, thr_in, want_thr=True, want_sb=True):
    lib = _lib.load()
    nq, nwg, slots = pairs.shape
    wi, ci = _buf(nq * ncand, torch.int32, SENT32)
    wv, cv = _buf(nq * ncand, torch.float32, SENTF)
    wt, to = _buf(nq, torch.float32, SENTF)
    ws, sb = _buf(nq, torch.float32, SENTF)
    dp, dm = _dev(pairs.view(np.int64)), _dev(meta.view(np.int32))
    ti = None if thr_in is None else _dev(thr_in)
    _done(lib.keds_search_merge(dp.data_ptr(), dm.data_ptr(), nq, nwg, slots, ncand, P(ti), ci.data_ptr(), cv.data_ptr(),
                                to.data_ptr() if want_thr else None, sb.data_ptr() if want_sb else None, _lib.stream()),
          f"keds_search_merge nwg {nwg} slots {slots} ncand {ncand}")
    ok = all(_guards_ok(w, f) for w, f in ((wi, SENT32), (wv, SENTF), (wt, SENTF), (ws, SENTF)))
    if not want_thr:
        ok = ok and bool((to == SENTF).all())
    return (ci.cpu().numpy().reshape(nq, ncand), cv.cpu().numpy().reshape(nq, ncand), to.cpu().numpy() if want_thr else None,
            sb.cpu().numpy() if want_sb else None, ok, (ci, cv))


KEYSETS = ("equal", "random", "straddle", ("bit", 0), ("bit", 7), ("bit", 8), ("bit", 15), ("bit", 16), ("bit", 23), ("bit", 24), ("bit", 31),
           ("ties", 2, 1), ("ties", 256, 3), ("ties", 257, 3), ("ties", 300, 40))


@pytest.mark.parametrize("slots", (4, 16, 64))
@pytest.mark.parametrize("ncand", (64, 256))
def test_merge_cuts_ties_and_bounds(ncand, slots):
    """synthetic segments: every query of a launch is another (V, key set, meta.y) case; garbage of larger keys lies behind every count"""
    t = Tally(f"merge.c{ncand}.s{slots}")
    T = 0xC0000000
    for nwg in (1, 63, 64, 65, 255, 256):
        rs = np.random.RandomState(nwg * 100 + slots)
        cap = nwg * slots
        P_, M_, thr_rows, names = [], [], [], []
        j = 0
        for V in (0, ncand - 1, ncand, ncand + 1, 4096, 4097, 16384):
            if V > cap:
                continue
            for kind in KEYSETS:
                if isinstance(kind, tuple) and kind[0] == "ties" and V < ncand - kind[2] + kind[1]:
                    continue
                keys = sc.key_set(kind, V, ncand, rs)
                pattern = (0, 1, 16, 17, 64) if V < cap else (slots,)
                cnts = sc.spread_counts(len(keys), nwg, slots, rs, pattern)
                metay = (0, T - 5, 0xFF000000)[j % 3]
                p, m = sc.synth_segments(cnts, slots, keys, rs, metay=metay)
                P_.append(p)
                M_.append(m)
                thr_rows.append((-3.0e38, 3.0e38)[(j // 3) % 2])
                names.append(f"V {V} {kind} meta.y {metay:#x}")
                j += 1
        pairs, meta = np.stack(P_), np.stack(M_)
        for thr_in in (None, np.array(thr_rows, np.float32)):
            ci, cv, to, sb, ok, _ = _merge(pairs, meta, ncand, thr_in)
            msgs = sc.merge_failures(pairs, meta, ncand, thr_in, ci, cv, to, sb)
            msgs = [m + " [" + names[int(m.split("query ")[1].split(" ")[0])] + "]" for m in msgs]
            t.add(f"nwg{nwg}", msgs, 0.0, ok, f"nwg {nwg} thr_in {'none' if thr_in is None else 'given'}: ")
        ci, cv, to, sb, ok, _ = _merge(pairs[:3], meta[:3], ncand, None, want_thr=False, want_sb=False)
        t.add(f"nwg{nwg}", sc.merge_failures(pairs[:3], meta[:3], ncand, None, ci, cv, None, None), 0.0, ok, "no thr_out, no sbound: ")
    t.finish()


# ---- rerank, certify ----------------------------------------------------------------------------------------------------------------
def _rerank(rows_d, qn_d, dim, metric, ci):
    lib = _lib.load()
    nq, ncand = ci.shape
    wd, cd = _buf(nq * ncand, torch.float32, SENTF)
    keep = []
    _done(lib.keds_search_rerank(P(rows_d), dim, metric, P(qn_d), P(_dev(ci, keep)), nq, ncand, cd.data_ptr(), _lib.stream()), "keds_search_rerank")
    return cd.cpu().numpy().reshape(nq, ncand), _guards_ok(wd, SENTF)


@pytest.mark.parametrize("dim", sc.DIMS)
def test_rerank(dim):
    t = Tally(f"rerank.{dim}")
    for regime in ("integer", "random", "bignorm", "offset"):
        x, q = sc.make_inputs(regime, 600, dim, 9)
        rows_d, qn_d = _dev(x), _dev(q)
        for ncand in (64, 256):
            rs = np.random.RandomState(ncand)
            ci = np.stack([rs.permutation(600)[:ncand] for _ in range(9)]).astype(np.int32)
            ci[1, :] = -1
            ci[2, 5:] = -1
            ci[3, ::3] = -1
            for metric in (sc.L2, sc.IP):
                cd, ok = _rerank(rows_d, qn_d, dim, metric, ci)
                msgs, worst = sc.rerank_failures(q, x, metric, ci, cd)
                t.add(f"{regime}.m{metric}", msgs, worst, ok, f"{regime} ncand {ncand} metric {metric}: ")
    t.finish()


def _certify(img_d, n, dim, ci, cd, metric, k, id_base, qstat, sbound, force, status0=True):
    lib = _lib.load()
    nq, ncand = ci.shape
    bufs = dict(D=_buf(nq * k, torch.float32, SENTF), I=_buf(nq * k, torch.int64, SENT64), counters=_buf(8 + nq, torch.int32, 9),
                fail_ids=_buf(nq, torch.int32, SENT32), fslot=_buf(nq, torch.int32, SENT32), dk=_buf(nq, torch.float32, SENTF),
                status=_buf(2, torch.int32, 0))
    bufs["counters"][1][0] = 0
    v = {name: b[1] for name, b in bufs.items()}
    keep = []
    _done(lib.keds_search_certify(img_d.data_ptr(), n, dim, P(_dev(ci, keep)), P(_dev(cd, keep)), nq, ncand, metric, k, id_base, P(_dev(qstat, keep)),
                                  P(_dev(sbound, keep)),
                                  v["D"].data_ptr(), v["I"].data_ptr(), v["counters"].data_ptr(), v["fail_ids"].data_ptr(), v["fslot"].data_ptr(),
                                  v["dk"].data_ptr(), v["status"].data_ptr(), force, _lib.stream()), f"keds_search_certify k {k} ncand {ncand}")
    fills = dict(D=SENTF, I=SENT64, counters=9, fail_ids=SENT32, fslot=SENT32, dk=SENTF, status=0)
    ok = all(_guards_ok(bufs[name][0], fills[name]) for name in bufs)
    res = {name: v[name].cpu().numpy() for name in v}
    res["D"], res["I"] = res["D"].reshape(nq, k), res["I"].reshape(nq, k)
    return res, ok


@pytest.mark.parametrize("dim", sc.DIMS)
@pytest.mark.parametrize("metric", (sc.L2, sc.IP))
def test_certify(metric, dim):
    """k and ncand at their edges, valid candidates 0 / k - 1 / k / ncand, duplicate distances, id_base 2^33, verdict margins of +-4 delta and
    +-0.1 eps, sbound = -inf, force_fail; the DbBounds are read from the trailer of an image of `dim`"""
    t = Tally(f"certify.{dim}.m{metric}")
    n = 33
    img = np.zeros(sc.packed_bytes(n, dim), np.uint8)
    for k, ncand in ((1, 64), (16, 64), (17, 256), (128, 256), (1, 256), (64, 64)):
        ci, cd, qstat, sbound, bounds = sc.cert_case(metric, k, ncand, seed=k + dim, dim=dim)
        img[-128:-112] = bounds.view(np.uint8)
        img_d = _dev(img)
        for force in (0, 1):
            res, ok = _certify(img_d, n, dim, ci, cd, metric, k, 1 << 33, qstat, sbound, force)
            msgs, closest = sc.certify_failures(ci, cd, metric, k, 1 << 33, qstat, sbound, bounds, force, res, SENTF, dim)
            t.add(f"k{k}", msgs, 0.0, ok, f"k {k} ncand {ncand} force {force}: ")
    t.finish()


# ---- exact pass ---------------------------------------------------------------------------------------------------------------------
def _all_distances(rows_d, x, qn, dim, metric):
    """fp32 distances of every query to every row as the rerank entry returns them"""
    nq, n = qn.shape[0], x.shape[0]
    blocks = -(-n // 256)
    ids = np.full((nq, blocks * 256), -1, np.int32)
    ids[:, :n] = np.arange(n, dtype=np.int32)
    out = np.zeros((nq, blocks * 256), np.float32)
    per = max(1024 // blocks, 1)
    for q0 in range(0, nq, per):
        qq = _dev(np.repeat(qn[q0:q0 + per], blocks, axis=0))
        cd, ok = _rerank(rows_d, qq, dim, metric, ids[q0:q0 + per].reshape(-1, 256))
        assert ok
        out[q0:q0 + per] = cd.reshape(-1, blocks * 256)
    return out[:, :n]


def _exact(rows_d, n, dim, metric, qn, fail_ids, dk, chunk_rows, k, id_base):
    lib = _lib.load()
    nq, nfail = qn.shape[0], len(fail_ids)
    nchunks = -(-n // chunk_rows)
    bufs = dict(D=_buf(nq * k, torch.float32, SENTF), I=_buf(nq * k, torch.int64, SENT64), plist=_buf(max(nfail, 1) * nchunks * k, torch.int64, SENT64),
                pcnt=_buf(max(nfail, 1) * nchunks, torch.int32, SENT32), counters=_buf(8 + nq, torch.int32, 9))
    v = {name: b[1] for name, b in bufs.items()}
    v["counters"][0] = nfail
    v["counters"][8:8 + nfail] = 0
    fi = np.full(nq, -1, np.int32)
    fi[:nfail] = fail_ids
    keep = []
    _done(lib.keds_search_exact(P(rows_d), n, dim, metric, P(_dev(qn, keep)), v["counters"].data_ptr(), P(_dev(fi, keep)), P(_dev(dk, keep)), chunk_rows, k, id_base,
                                v["plist"].data_ptr(), v["pcnt"].data_ptr(), v["D"].data_ptr(), v["I"].data_ptr(), _lib.stream()),
          f"keds_search_exact n {n} chunk_rows {chunk_rows} k {k}")
    fills = dict(D=SENTF, I=SENT64, plist=SENT64, pcnt=SENT32, counters=9)
    ok = all(_guards_ok(bufs[name][0], fills[name]) for name in bufs)
    c = v["counters"].cpu().numpy()
    ok = ok and c[0] == nfail and (c[8:8 + nfail] == nchunks).all() and (c[8 + nfail:] == 9).all()
    return v["D"].cpu().numpy().reshape(nq, k), v["I"].cpu().numpy().reshape(nq, k), ok


@pytest.mark.parametrize("metric", (sc.L2, sc.IP))
@pytest.mark.parametrize("n", (1, 2056, 5000))
def test_exact_pass(n, metric):
    """1, 257, 625 and 2 ... 3 chunks (1, 2 and 3 lists per merging thread), a partial last chunk, dk = +inf / the k-th distance / one ulp
    tighter than a duplicate pair, 0 / 1 / 5 failed queries of 8"""
    t = Tally(f"exact.n{n}.m{metric}")
    dim, nq = 128, 8
    for regime in ("integer", "random"):
        x, q = sc.make_inputs(regime, n, dim, nq, seed=n)
        if n > 40:
            x[n - 1] = x[17]                                      # a duplicate pair, one of them in the last (partial) chunk
            x[n // 2] = x[17]
        rows_d = _dev(x)
        dist = _all_distances(rows_d, x, q, dim, metric)
        worse = np.float32(np.inf if metric == sc.L2 else -np.inf)
        for chunk_rows in (8, 64, 2048):
            if -(-n // chunk_rows) > 2048:
                continue
            for k in (1, 16, 128):
                for fail_ids in ((), (5,), (6, 1, 3, 0, 5)):
                    key = dist if metric == sc.L2 else -dist
                    kth = np.sort(key, 1)[:, min(k, n) - 1] * (1 if metric == sc.L2 else -1)
                    dup = dist[:, 17] if n > 40 else kth
                    tight = np.nextafter(dup, -worse).astype(np.float32)           # both rows of the pair fall to the prune
                    dk = np.stack([np.full(nq, worse), kth, tight])[np.arange(nq) % 3, np.arange(nq)].astype(np.float32)
                    D, I, ok = _exact(rows_d, n, dim, metric, q, fail_ids, dk, chunk_rows, k, 1 << 33)
                    before_D, before_I = np.full((nq, k), SENTF, np.float32), np.full((nq, k), SENT64, np.int64)
                    msgs = sc.exact_failures(dist[list(fail_ids)].reshape(len(fail_ids), n), dk[list(fail_ids)], k, metric, 1 << 33, list(fail_ids),
                                             D, I, before_D, before_I)
                    t.add(regime, msgs, 0.0, ok, f"{regime} chunk_rows {chunk_rows} k {k} failed {fail_ids}: ")
    t.finish()


# ---- the two compositions -----------------------------------------------------------------------------------------------------------
def _plan(nq, dim, n, k):
    lib = _lib.load()
    out = (C.c_int32 * len(sc.PLAN_FIELDS))()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _lib.check(lib.keds_index_search_plan_query(nq, dim, n, k, cus, out), "keds_index_search_plan_query")
    return dict(zip(sc.PLAN_FIELDS, list(out)))


def _search_whole(rows_d, img_d, n, dim, metric, q, k, id_base, normalize):
    lib = _lib.load()
    nq = q.shape[0]
    wsb = lib.keds_index_search_workspace_bytes_ex(nq, dim, n, k)
    ws = torch.zeros(wsb + 256, dtype=torch.uint8, device=DEV)
    D = torch.full((nq, k), SENTF, dtype=torch.float32, device=DEV)
    I = torch.full((nq, k), SENT64, dtype=torch.int64, device=DEV)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    q_d = _dev(q)
    _done(lib.keds_index_search_packed_ex(img_d.data_ptr(), P(rows_d), n, dim, metric, P(q_d), nq, normalize, k, id_base, P(D), P(I), None,
                                          ws.data_ptr(), wsb, P(status), _lib.stream()), "keds_index_search_packed_ex")
    return D.cpu().numpy(), I.cpu().numpy(), status.cpu().numpy()


def _search_by_stages(t, rows_d, img_d, x, n, dim, metric, q, k, id_base, normalize, what):
    """the stage entries chained as the plan says -> everything the compositions look at"""
    nq = q.shape[0]
    p = _plan(nq, dim, n, k)
    qn, qb_bits, qstat, ok, (qn_d, qb_d, qs_d) = _qprep(q, normalize)
    t.add("chain", sc.qprep_failures(q, normalize, qn, qb_bits, qstat)[0], 0.0, ok, what + "qprep: ")

    class Q:                                                      # what _scan reads of a ScanData
        pass
    data = Q()
    data.img, data.n, data.dim, data.qb, data.nqb = img_d, n, dim, qb_d, p["nqb"]
    thr = None
    if p["two_phase"]:
        pa, ma, ok, _ = _scan(data, p["stagesA"], p["nwgA"], p["depthA"], None)
        _, _, thr, _, ok2, _ = _merge(pa[:nq], ma[:nq], p["ncand"], None, want_sb=False)
        t.add("chain", [], 0.0, ok and ok2, what + "threshold pass: ")
        thr_pad = np.zeros(p["nqb"] * 128, np.float32)
        thr_pad[:nq] = thr
        thr = thr_pad
    pairs, meta, ok, _ = _scan(data, p["total_stages"], p["nwgB"], 16, thr)
    pairs, meta = pairs[:nq], meta[:nq]
    thr_q = None if thr is None else thr[:nq]
    ci, cv, _, sbound, ok2, _ = _merge(pairs, meta, p["ncand"], thr_q, want_thr=False)
    t.add("chain", sc.merge_failures(pairs, meta, p["ncand"], thr_q, ci, cv, None, sbound), 0.0, ok and ok2, what + "merge of the scan's own output: ")
    cd, ok = _rerank(rows_d, qn_d.view(nq, dim), dim, metric, ci)
    msgs, worst = sc.rerank_failures(qn, x, metric, ci, cd)
    t.add("chain.rerank", msgs, worst, ok, what + "rerank: ")
    res, ok = _certify(img_d, n, dim, ci, cd, metric, k, id_base, qstat, sbound, 0)
    bounds = sc.decode_image(img_d.cpu().numpy(), n, dim)["bounds"]
    t.add("chain", sc.certify_failures(ci, cd, metric, k, id_base, qstat, sbound, bounds, 0, res, SENTF, dim)[0], 0.0, ok, what + "certify: ")
    nfail = int(res["counters"][0])
    D, I = res["D"].copy(), res["I"].copy()
    if nfail:
        lib = _lib.load()
        Dd, Id = _dev(D), _dev(I)
        cnt = _dev(res["counters"])
        nchunks = p["nchunks"]
        plist = torch.zeros(nfail * nchunks * k, dtype=torch.int64, device=DEV)
        pcnt = torch.zeros(nfail * nchunks, dtype=torch.int32, device=DEV)
        keep = []
        _done(lib.keds_search_exact(P(rows_d), n, dim, metric, qn_d.data_ptr(), P(cnt), P(_dev(res["fail_ids"], keep)), P(_dev(res["dk"], keep)), p["chunk_rows"], k,
                                    id_base, P(plist), P(pcnt), P(Dd), P(Id), _lib.stream()), "keds_search_exact")
        D, I = Dd.cpu().numpy(), Id.cpu().numpy()
    return dict(D=D, I=I, status=res["status"], qn=qn, qstat=qstat, bounds=bounds, pairs=pairs, meta=meta, ci=ci, cd=cd, sbound=sbound,
                certified=res["fslot"] < 0, plan=p)


def _compose(t, name, x, q, k, metric=sc.L2, normalize=0, id_base=0):
    n, dim = x.shape
    nq = q.shape[0]
    rows_d, img_d, _, ok, _keep = _pack(x, metric)
    r = _search_by_stages(t, rows_d, img_d, x, n, dim, metric, q, k, id_base, normalize, f"{name}: ")
    D, I, status = _search_whole(rows_d, img_d, n, dim, metric, q, k, id_base, normalize)
    same = sc.same_bits(D, r["D"]) and np.array_equal(I, r["I"]) and np.array_equal(status, r["status"])
    t.add("chain", [] if same else [f"{name}: the chained stages differ from keds_index_search_packed_ex (D {int((sc.f32_bits(D) != sc.f32_bits(r['D'])).sum())}, "
                                    f"I {int((I != r['I']).sum())} places; status {status.tolist()} vs {r['status'].tolist()})"], 0.0, ok)
    # premise, claim, result: float64 on the original rows and the stored qn
    t64 = sc.t64(r["qn"], x, metric)
    dkq = sc.ref_dk(r["ci"], r["cd"], metric, k)
    tk = np.where(metric == sc.L2, 0.5 * (r["qstat"][:, 0].astype(np.float64) - dkq), dkq)
    tk = np.where(np.isnan(tk), 0.0, tk)
    prem = sc.premise_ratio(r["pairs"], r["meta"], t64, r["qstat"], r["bounds"], tk, dim, metric)
    frac = float(r["certified"].mean())
    report(f"search_edges.composition.{name}", premise_ratio=prem, certified_fraction=frac, two_phase=r["plan"]["two_phase"], nq=nq, n=n, dim=dim, k=k)
    t.add(f"premise.{name}", [] if prem <= 1.0 else [f"{name}: a listed pair's score is {prem:.3g} x eps from its exact score"], prem)
    t.add("claim", sc.claim_failures(t64, r["ci"], r["certified"], k, f"{name}: "))
    t.add("result", sc.result_failures(r["qn"], x, metric, k, D, I, id_base, f"{name}: "))
    return frac, r


def test_stages_chained_equal_the_search_and_the_certificate_holds():
    t = Tally("composition")
    x, q = sc.make_inputs("random", 4129, 768, 37, seed=1)
    frac, r = _compose(t, "single_phase", x, q, 16)
    assert not r["plan"]["two_phase"]
    t.add("claim", [] if frac >= 0.25 else [f"single_phase: only {frac:.3g} of the queries certified"])
    x, q = sc.make_inputs("random", 32768 + 33, 128, 130, seed=2)
    frac, r = _compose(t, "two_phase", x, q, 16, normalize=1, id_base=1 << 33)
    assert r["plan"]["two_phase"]
    t.add("claim", [] if frac >= 0.25 else [f"two_phase: only {frac:.3g} of the queries certified"])
    x, q = sc.make_inputs("random", 3000, 256, 9, seed=3)
    _compose(t, "k101", x, q, 101)
    _compose(t, "k101_ip", x, q, 101, metric=sc.IP)
    for regime in ("random", "bignorm", "offset", "placed"):
        x, q, k = sc.composition_inputs(regime, 4096 + 33, 128, 16, seed=3)
        frac, r = _compose(t, regime, x, q, k)
        if regime in ("random", "bignorm"):
            t.add("claim", [] if frac >= 0.25 else [f"{regime}: only {frac:.3g} of the queries certified: the claim is checked on too few"])
        if regime == "offset":
            t.add("claim", [] if frac == 0.0 else [f"offset: {frac:.3g} of the queries certified where bf16 cannot rank the rows"])
    t.finish()


# ---- merge_parts, exchange, gather_rows: bit for bit against a sort keyed on (key, id) --------------------------------------------------
@pytest.mark.parametrize("metric", (sc.L2, sc.IP))
def test_merge_parts(metric):
    lib = _lib.load()
    t = Tally(f"merge_parts.m{metric}")
    for parts in (1, 2, 64):
        for k in (1, 16, 128):
            for nq in (5, 70):
                D, I = sc.partial_lists(parts, nq, k, metric, seed=nq)
                wD, oD = _buf(nq * k, torch.float32, SENTF)
                wI, oI = _buf(nq * k, torch.int64, SENT64)
                dD, dI = _dev(D), _dev(I)
                _done(lib.keds_topk_merge_parts(P(dD), P(dI), parts, nq, k, metric, oD.data_ptr(), oI.data_ptr(), _lib.stream()), "keds_topk_merge_parts")
                wantD, wantI, _ = sc.merged_topk(D, I, metric)
                same = sc.same_bits(oD.cpu().numpy().reshape(nq, k), wantD) and np.array_equal(oI.cpu().numpy().reshape(nq, k), wantI)
                t.add("bits", [] if same else [f"parts {parts} k {k} nq {nq}: differs from the sort by (key, id)"], 0.0,
                      _guards_ok(wD, SENTF) and _guards_ok(wI, SENT64))
    t.finish()


@pytest.mark.parametrize("with_rows", (False, True))
@pytest.mark.parametrize("metric", (sc.L2, sc.IP))
def test_exchange_pack_and_merge(metric, with_rows):
    lib = _lib.load()
    t = Tally(f"exchange.m{metric}.rows{int(with_rows)}")
    dim = 8
    for world, k in ((1, 1), (2, 16), (64, 16), (32, 128), (64, 1)):          # 32 x 128 = 4096 entries of one query
        B = 3
        D, I = sc.partial_lists(world, B, k, metric, seed=world)
        rows = np.random.RandomState(world).standard_normal((world, B, k, dim)).astype(np.float32) if with_rows else None
        E = dim + 4 if with_rows else 3
        stride = B * k * E + 4                                    # a gap behind every part
        ws, send = _buf(world * stride, torch.int32, SENT32)
        dD, dI = _dev(D.reshape(world * B, k)), _dev(I.reshape(world * B, k))
        dR = _dev(rows.reshape(world * B, k, dim)) if with_rows else None
        _done(lib.keds_exchange_pack(P(dD), P(dI), P(dR), world, B, k, dim, stride, send.data_ptr(), _lib.stream()), "keds_exchange_pack")
        got = send.cpu().numpy().reshape(world, stride)
        want = np.full((world, stride), SENT32, np.int32)
        body = np.zeros((world, B, k, E), np.int32)
        body[..., 0] = D.view(np.int32)
        body[..., 1] = (I & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        body[..., 2] = (I >> 32).astype(np.int32)
        if with_rows:
            body[..., 4:] = rows.view(np.int32)
        want[:, :B * k * E] = body.reshape(world, -1)
        t.add("pack", [] if np.array_equal(got, want) else [f"world {world} k {k}: the packed message differs in {int((got != want).sum())} words"],
              0.0, _guards_ok(ws, SENT32))
        wD, oD = _buf(B * k, torch.float32, SENTF)
        wI, oI = _buf(B * k, torch.int64, SENT64)
        wR, oR = _buf(B * k * dim, torch.float32, SENTF)
        _done(lib.keds_exchange_merge(send.data_ptr(), world, B, k, dim, stride, metric, oD.data_ptr(), oI.data_ptr(),
                                      oR.data_ptr() if with_rows else None, _lib.stream()), "keds_exchange_merge")
        wantD, wantI, src = sc.merged_topk(D, I, metric)
        msgs = []
        if not (sc.same_bits(oD.cpu().numpy().reshape(B, k), wantD) and np.array_equal(oI.cpu().numpy().reshape(B, k), wantI)):
            msgs.append(f"world {world} k {k}: (D, I) differ from the sort by (key, id)")
        if with_rows:
            wantR = np.where((src[..., 0] >= 0)[..., None], rows[src[..., 0], np.arange(B)[:, None], src[..., 1]], np.float32(0.0))
            if not sc.same_bits(oR.cpu().numpy().reshape(B, k, dim), wantR.astype(np.float32)):
                msgs.append(f"world {world} k {k}: the winners' rows differ")
        elif not bool((oR == SENTF).all()):
            msgs.append("rows written without a rows buffer")
        t.add("merge", msgs, 0.0, _guards_ok(wD, SENTF) and _guards_ok(wI, SENT64) and _guards_ok(wR, SENTF))
    t.finish()


def test_gather_rows():
    lib = _lib.load()
    t = Tally("gather_rows")
    for dim in (4, 128, 768, 1024):
        for count in (1, 3, 4, 5, 131):
            rs = np.random.RandomState(dim + count)
            db = rs.standard_normal((50, dim)).astype(np.float32)
            idx = rs.randint(0, 50, count).astype(np.int64)
            idx[::3] = -1
            idx[-1] = 49
            wO, out = _buf(count * dim, torch.float32, SENTF)
            d_db, d_idx = _dev(db), _dev(idx)
            _done(lib.keds_gather_rows(P(d_db), dim, P(d_idx), count, out.data_ptr(), _lib.stream()), "keds_gather_rows")
            want = np.where((idx >= 0)[:, None], db[np.maximum(idx, 0)], np.float32(0.0))
            same = sc.same_bits(out.cpu().numpy().reshape(count, dim), want)
            t.add("bits", [] if same else [f"dim {dim} count {count}: differs"], 0.0, _guards_ok(wO, SENTF))
    t.finish()
