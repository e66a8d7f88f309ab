"""The filtered search (include/keds_select.h: a row selector of one 32-bit word per scan stage, per-query exclusion lists) at its
edges, kernel by kernel through the *_sel stage entries and then whole.

The scan's SEL form is held to two references at once: the unfiltered scan on a copy of the image whose ineligible rows' bias words
were overwritten with -inf (bit for bit in pairs and meta: a masked key IS a key with a -inf bias) and tests/search_check.py's
float64 check of the lists on scores with those rows at -inf.  Certify and the exact pass are held to search_check's models on the
candidates / rows that remain.  The whole search is held to an index built from the eligible rows alone, to the unfiltered search
with k + E, and to a top-k by (distance, id) of the rerank entry's own fp32 distances over the allowed rows.

Every output sits in a sentinel-filled buffer with guard elements on both sides (the helpers of test_gpu_search_kernels_edges.py)."""
import numpy as np
import pytest
import torch

import keds_amd
from keds_amd import _lib, ops
from keds_amd.index import FlatIndex, Selector, shard_bounds
from tests import search_check as sc
from tests.test_gpu_search_kernels_edges import (DEV, SENT32, SENT64, SENTF, P, ScanData, Tally, _all_distances, _buf, _dev, _done, _guards_ok,
                                                 _u64)

pytestmark = pytest.mark.gpu

BIG_BASE = (1 << 33) + 5
SELFILL = 0x2AAAAAAA                                              # guard words around a selector: alternating bits, were they ever read


def _hit(I, ex):
    """does a query's result hold one of ITS excluded ids (-1 entries and fillers aside)"""
    return bool(((I[:, :, None] == ex[:, None, :]) & (ex[:, None, :] >= 0)).any())


# ---- selectors ------------------------------------------------------------------------------------------------------------------------
def _words(elig):
    """bool [S * 32] -> uint32 [S], bit (r & 31) of word (r >> 5)"""
    return Selector.pack_mask(elig)


def _sel_dev(words):
    """-> (whole guarded buffer, device int32 view of the words)"""
    whole, view = _buf(len(words), torch.int32, SELFILL)
    view.copy_(torch.from_numpy(words.view(np.int32).copy()))
    return whole, view


def _selector_cases(n, S, rs):
    """name -> bool [S * 32] (bits at or behind n are set in some and clear in others: they are ignored)"""
    rows = S * 32
    r = np.arange(rows)
    out = {"ones": np.ones(rows, bool), "zero": np.zeros(rows, bool), "rows31_32": (r == 31) | (r == 32), "last_stage": r >= (S - 1) * 32,
           "half": rs.rand(rows) < 0.5, "percent": rs.rand(rows) < 0.01}
    return out


def _bit_cases():
    """one-hot bit p of every stage and its complement"""
    for p in range(32):
        yield f"bit{p}", lambda rows, p=p: (np.arange(rows) % 32) == p
        yield f"notbit{p}", lambda rows, p=p: (np.arange(rows) % 32) != p


# ---- keds_sel_build -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 31, 32, 33, 1000))
def test_sel_build(n):
    lib = _lib.load()
    t = Tally(f"sel_build.n{n}")
    rs = np.random.RandomState(n)
    nw = (n + 31) // 32
    for id_base in (0, BIG_BASE):
        inside = rs.randint(0, n, max(n // 3, 1)).astype(np.int64) + id_base
        lists = {"some": inside,
                 "duplicates": np.concatenate([inside, inside, inside[:1].repeat(5)]),
                 "out_of_range": np.concatenate([inside, [id_base - 1, id_base + n, id_base + n + 31, -1, id_base + (1 << 32), -(1 << 40),
                                                          np.iinfo(np.int64).max]]).astype(np.int64),
                 "edges": np.array([id_base, id_base + n - 1], np.int64),
                 "empty": np.zeros(0, np.int64)}
        for name, ids in lists.items():
            for drop in (0, 1):
                whole, sel = _buf(nw, torch.int32, SENT32)
                keep = []
                d_ids = _dev(ids, keep) if len(ids) else None
                _done(lib.keds_sel_build(sel.data_ptr(), n, P(d_ids), len(ids), id_base, drop, _lib.stream()), f"keds_sel_build n {n} {name}")
                local = ids - id_base
                hit = np.zeros(nw * 32, bool)
                hit[local[(ids >= id_base) & (local < n) & (local >= 0)]] = True
                want = _words(~hit if drop else hit)
                got = sel.cpu().numpy().view(np.uint32)
                t.add("bits", [] if np.array_equal(got, want) else [f"{int((got != want).sum())} words differ from numpy"], 0.0,
                      _guards_ok(whole, SENT32), f"id_base {id_base} {name} drop {drop}: ")
                s = Selector.from_ids(n, ids, keep=not drop, id_base=id_base, device=DEV)
                same = np.array_equal(s.to_mask(), (~hit if drop else hit)[:n]) and s.count() == int((~hit if drop else hit)[:n].sum())
                t.add("from_ids", [] if same else ["Selector.from_ids differs from the numpy mask"], 0.0, True, f"id_base {id_base} {name} drop {drop}: ")
    m = rs.rand(n) < 0.5
    t.add("from_mask", [] if np.array_equal(Selector.from_mask(m, device=DEV).to_mask(), m) else ["from_mask on the device does not round-trip"])
    t.finish()


# ---- scan -----------------------------------------------------------------------------------------------------------------------------
def _scan_sel(data, img, stages, nwg, depth, thr, sel):
    """sel: device int32 words or None (then the unfiltered entry on `img`)"""
    lib = _lib.load()
    nqp = data.nqb * 128
    wp, pairs = _buf(nqp * nwg * 4 * depth, torch.int64, SENT64)
    wm, meta = _buf(nqp * nwg * 2, torch.int32, SENT32)
    thr_d = None if thr is None else _dev(thr)
    what = f"dim {data.dim} stages {stages} nwg {nwg} depth {depth}"
    if sel is None:
        _done(lib.keds_search_scan(img.data_ptr(), data.n, data.dim, stages, P(data.qb), data.nqb, P(thr_d), depth, nwg, pairs.data_ptr(),
                                   meta.data_ptr(), _lib.stream()), "keds_search_scan " + what)
    else:
        _done(lib.keds_search_scan_sel(img.data_ptr(), data.n, data.dim, stages, P(data.qb), data.nqb, P(thr_d), depth, nwg, pairs.data_ptr(),
                                       meta.data_ptr(), sel.data_ptr(), _lib.stream()), "keds_search_scan_sel " + what)
    ok = _guards_ok(wp, SENT64) and _guards_ok(wm, SENT32)
    return _u64(pairs).reshape(nqp, nwg, 4 * depth), meta.cpu().numpy().view(np.uint32).reshape(nqp, nwg, 2), ok


def _masked_image(data, elig):
    """a copy of the image whose ineligible rows' bias words are -inf"""
    img = data.img.clone()
    f = img.view(torch.float32)
    rows = np.nonzero(~elig)[0]
    sb = sc.stage_bytes(data.dim)
    idx = (rows // 32) * (sb // 4) + (32 * data.dim * 2) // 4 + rows % 32
    f[torch.from_numpy(idx).to(DEV)] = float("-inf")
    return img


def _check_selector(t, data, name, elig, stages, nwg, depth, kind, plain=None):
    """the SEL scan against the unfiltered scan of the masked image (bits) and against float64 on the masked scores"""
    what = f"{data.regime} sel {name} stages {stages} nwg {nwg} n {data.n} depth {depth} thr {kind}: "
    thr = data.thr(kind)
    wsel, sel = _sel_dev(_words(elig))
    pa, ma, ok_a = _scan_sel(data, data.img, stages, nwg, depth, thr, sel)
    pb, mb, ok_b = _scan_sel(data, _masked_image(data, elig), stages, nwg, depth, thr, None)
    msgs = []
    if not (np.array_equal(pa, pb) and np.array_equal(ma, mb)):
        msgs.append(f"differs from the unfiltered scan of the masked image in {int((pa != pb).sum())} pairs, {int((ma != mb).sum())} meta words")
    s64 = data.s64.copy()
    s64[:, ~elig[:s64.shape[1]]] = -np.inf
    more, worst = sc.scan_failures(s64, data.e64, data.n, stages, nwg, depth, thr, pa, ma, SENT64)
    msgs += more
    if name == "ones":
        if plain is None:
            plain = _scan_sel(data, data.img, stages, nwg, depth, thr, None)
        if not (np.array_equal(pa, plain[0]) and np.array_equal(ma, plain[1])):
            msgs.append("the all-ones selector differs from the unfiltered scan of the untouched image")
    if name == "zero" and not ((ma == 0).all() and (pa == np.uint64(SENT64)).all()):
        msgs.append(f"the all-zero selector left {int((ma[..., 0] != 0).sum())} nonzero counts, {int((pa != np.uint64(SENT64)).sum())} written pairs")
    t.add(name.rstrip("0123456789"), msgs, worst, ok_a and ok_b and data.pack_ok and _guards_ok(wsel, SELFILL), what)
    return pa, ma


DEPTHS = (1, 4, 16)
KINDS = ("none", "median", "+inf")
SCAN_REGIMES = ("random", "integer", "ramp_up")


@pytest.mark.parametrize("dim", sc.DIMS)
def test_scan_selector(dim):
    """stages per workgroup around the ring depth with 1, 2 and 7 workgroups (s0 != 0), n mod 32 = 0, 1, 31, every list depth and
    threshold kind, every selector: the six named ones on every shape with depth and threshold in turn and in full cross on one shape;
    the 64 one-hot / complement selectors on a one-workgroup and a seven-workgroup shape"""
    t = Tally(f"scan_sel.{dim}")
    nst = sc.ring_depth(dim)
    spw = sorted({max(nst - 1, 1), nst, nst + 1, 2 * nst + 1})
    shapes = [(s * nwg, nwg) for s in spw for nwg in (1, 2, 7)]
    for i, (stages, nwg) in enumerate(shapes):
        n = stages * 32 - (0, 31, 1)[i % 3]                       # n mod 32 = 0, 1, 31 in turn
        data = ScanData(SCAN_REGIMES[i % 3], n, dim, 8, seed=i)
        rs = np.random.RandomState(1000 * dim + i)
        for j, (name, elig) in enumerate(_selector_cases(n, stages, rs).items()):
            _check_selector(t, data, name, elig, stages, nwg, DEPTHS[(i + j) % 3], KINDS[(i + j // 3) % 3])
    # full cross of depth x threshold x named selector: 2 NST + 1 stages per workgroup, seven workgroups, a partial last stage
    stages, nwg = 7 * (2 * nst + 1), 7
    data = ScanData("random", stages * 32 - 31, dim, 8, seed=77)
    cases = _selector_cases(data.n, stages, np.random.RandomState(dim))
    for depth in DEPTHS:
        for kind in KINDS:
            for name, elig in cases.items():
                _check_selector(t, data, name, elig, stages, nwg, depth, kind)
    # the lane that owns each bit: one-hot bit p of every stage, and the complements
    for stages, nwg, regime in ((nst + 1, 1, "integer"), (7 * nst + 3, 7, "random")):
        data = ScanData(regime, stages * 32 - 1, dim, 8, seed=5)
        for j, (name, make) in enumerate(_bit_cases()):
            _check_selector(t, data, name, make(stages * 32), stages, nwg, DEPTHS[j % 3], KINDS[(j // 2) % 2])
    # a prefix of the image (the threshold pass): the word of stage t is sel[t] of the whole index; two query blocks
    data = ScanData("random", 40 * 32 - 5, dim, 129, seed=9)
    cases = _selector_cases(data.n, 40, np.random.RandomState(dim + 1))
    _check_selector(t, data, "half", cases["half"], 13, 2, 4, "none")
    _check_selector(t, data, "half", cases["half"], 13, 7, 1, "none")
    _check_selector(t, data, "percent", cases["percent"], 40, 7, 16, "median")
    _check_selector(t, data, "rows31_32", cases["rows31_32"], 40, 2, 16, "none")
    if dim == 128:                                                # eight query blocks
        data = ScanData("random", 700, dim, 1024, seed=11)
        cases = _selector_cases(700, 22, np.random.RandomState(4))
        _check_selector(t, data, "half", cases["half"], 22, 2, 16, "median")
        _check_selector(t, data, "last_stage", cases["last_stage"], 22, 3, 1, "none")
        _check_selector(t, data, "ones", cases["ones"], 22, 3, 4, "none")
    if dim == 768:                                                # both cache policies of the candidate pass's key stream
        lib = _lib.load()
        data = ScanData("random", 21 * 32 - 31, dim, 1, seed=13)
        elig = np.random.RandomState(6).rand(21 * 32) < 0.5
        a = _check_selector(t, data, "half", elig, 21, 3, 16, "none")
        try:
            lib.keds_scan_debug(1 << 6)
            b = _check_selector(t, data, "half", elig, 21, 3, 16, "none")
        finally:
            lib.keds_scan_debug(0)
        t.add("half", [] if np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) else ["the two cache policies give different lists"])
    t.finish()


# ---- certify --------------------------------------------------------------------------------------------------------------------------
def _certify_sel(img_d, n, dim, ci, cd, metric, k, id_base, qstat, sbound, force, exclude):
    """exclude: int64 [nq, E] host array, or None for the unfiltered entry"""
    lib = _lib.load()
    nq, ncand = ci.shape
    bufs = dict(D=_buf(nq * k, torch.float32, SENTF), I=_buf(nq * k, torch.int64, SENT64), counters=_buf(8 + nq, torch.int32, 9),
                fail_ids=_buf(nq, torch.int32, SENT32), fslot=_buf(nq, torch.int32, SENT32), dk=_buf(nq, torch.float32, SENTF),
                status=_buf(2, torch.int32, 0))
    bufs["counters"][1][0] = 0
    v = {name: b[1] for name, b in bufs.items()}
    keep = []
    head = (img_d.data_ptr(), n, dim, P(_dev(ci, keep)), P(_dev(cd, keep)), nq, ncand, metric, k, id_base, P(_dev(qstat, keep)), P(_dev(sbound, keep)),
            v["D"].data_ptr(), v["I"].data_ptr(), v["counters"].data_ptr(), v["fail_ids"].data_ptr(), v["fslot"].data_ptr(), v["dk"].data_ptr(),
            v["status"].data_ptr(), force)
    if exclude is None:
        _done(lib.keds_search_certify(*head, _lib.stream()), f"keds_search_certify k {k} ncand {ncand}")
    else:
        ex = _dev(exclude, keep) if exclude.size else None
        _done(lib.keds_search_certify_sel(*head, P(ex), exclude.shape[1], _lib.stream()), f"keds_search_certify_sel k {k} ncand {ncand}")
    fills = dict(D=SENTF, I=SENT64, counters=9, fail_ids=SENT32, fslot=SENT32, dk=SENTF, status=0)
    ok = all(_guards_ok(bufs[name][0], fills[name]) for name in bufs)
    res = {name: v[name].cpu().numpy() for name in v}
    res["D"], res["I"] = res["D"].reshape(nq, k), res["I"].reshape(nq, k)
    return res, ok


EXCLUDE_KINDS = ("rank0", "rank_k-1", "rank_k", "top16", "absent_dup_minus1", "only_minus1")


def _exclude_lists(ci, cd, metric, k, id_base, E, rs):
    """per query (kind by groups of four queries, so that every kind meets 0 / k - 1 / k / ncand valid candidates): int64 [nq, E] global ids"""
    nq = ci.shape[0]
    ex = np.full((nq, 16), -1, np.int64)
    for q in range(nq):
        ok = np.nonzero(ci[q] >= 0)[0]
        key = cd[q, ok] if metric == sc.L2 else -cd[q, ok]
        ranked = ci[q, ok[np.lexsort((ci[q, ok], key))]].astype(np.int64) + id_base      # the valid candidates, best first, as global ids
        kind = EXCLUDE_KINDS[(q // 4) % len(EXCLUDE_KINDS)]
        absent = np.array([id_base + 6000 + q, id_base - 1 if id_base else 7000, (ranked[0] if len(ranked) else 5) + (1 << 32)], np.int64)
        if kind == "rank0" and len(ranked) > 0:
            ex[q, 0] = ranked[0]
        elif kind == "rank_k-1" and len(ranked) > k - 1:
            ex[q, :3] = [absent[0], ranked[k - 1], -1]
        elif kind == "rank_k" and len(ranked) > k:
            ex[q, :2] = [-1, ranked[k]]
        elif kind == "top16":
            top = ranked[:16]
            ex[q, :len(top)] = top[rs.permutation(len(top))]
        elif kind == "absent_dup_minus1":
            first = ranked[:2]
            row = np.concatenate([absent, first, first, [-1], first[:1]])
            ex[q, :len(row)] = row
    return np.ascontiguousarray(ex[:, :E])


@pytest.mark.parametrize("id_base", (0, BIG_BASE))
@pytest.mark.parametrize("metric", (sc.L2, sc.IP))
def test_certify_exclusions(metric, id_base):
    """an excluded id at rank 0, k - 1 and k, the whole top 16 excluded (k = 16 of 64 candidates: the next 16 are returned), absent,
    duplicate and -1 entries, an entry 2^32 above a candidate: the kernel against search_check's model on the candidates that remain"""
    t = Tally(f"certify_sel.m{metric}.b{int(id_base != 0)}")
    dim, n = 128, 33
    img = np.zeros(sc.packed_bytes(n, dim), np.uint8)
    for (k, ncand), E in (((1, 64), 16), ((16, 64), 16), ((17, 256), 3), ((128, 256), 16), ((64, 64), 1)):
        ci, cd, qstat, sbound, bounds = sc.cert_case(metric, k, ncand, seed=k + 3, dim=dim)
        img[-128:-112] = bounds.view(np.uint8)
        img_d = _dev(img)
        ex = _exclude_lists(ci, cd, metric, k, id_base, E, np.random.RandomState(k))
        gone = ((ci.astype(np.int64) + id_base)[:, :, None] == ex[:, None, :]).any(2) & (ci >= 0)
        left = np.where(gone, -1, ci).astype(np.int32)
        if (k, ncand) == (16, 64):
            assert any(gone[q].sum() == 16 and (ci[q] >= 0).sum() == 64 for q in range(ci.shape[0]))
        for force in (0, 1):
            res, ok = _certify_sel(img_d, n, dim, ci, cd, metric, k, id_base, qstat, sbound, force, ex)
            msgs, _ = sc.certify_failures(left, cd, metric, k, id_base, qstat, sbound, bounds, force, res, SENTF, dim)
            if _hit(res["I"], ex):
                msgs.append("an excluded id was returned")
            t.add(f"k{k}", msgs, 0.0, ok, f"k {k} ncand {ncand} E {E} force {force}: ")
        # null arguments: the unfiltered entry, n_exclude = 0 and a list of -1 alone give the same bits
        base, ok0 = _certify_sel(img_d, n, dim, ci, cd, metric, k, id_base, qstat, sbound, 0, None)
        for name, arg in (("n_exclude 0", np.zeros((ci.shape[0], 0), np.int64)), ("all -1", np.full((ci.shape[0], E), -1, np.int64))):
            res, ok = _certify_sel(img_d, n, dim, ci, cd, metric, k, id_base, qstat, sbound, 0, arg)
            same = all(np.array_equal(res[f].view(np.uint8), base[f].view(np.uint8)) for f in ("D", "I", "dk", "status"))     # (fail slots: atomic order)
            nf = int(base["counters"][0])
            same = same and np.array_equal(res["fslot"] >= 0, base["fslot"] >= 0) and np.array_equal(res["counters"][[0]], base["counters"][[0]])
            same = same and sorted(res["fail_ids"][:nf].tolist()) == sorted(base["fail_ids"][:nf].tolist())
            t.add(f"k{k}", [] if same else [f"{name}: differs from keds_search_certify"], 0.0, ok and ok0, f"k {k} ncand {ncand}: ")
    t.finish()


# ---- exact pass -----------------------------------------------------------------------------------------------------------------------
def _exact_sel(rows_d, n, dim, metric, qn, fail_ids, dk, chunk_rows, k, id_base, sel, exclude):
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
    ex = _dev(exclude, keep) if exclude is not None else None
    _done(lib.keds_search_exact_sel(P(rows_d), n, dim, metric, P(_dev(qn, keep)), v["counters"].data_ptr(), P(_dev(fi, keep)), P(_dev(dk, keep)), chunk_rows, k,
                                    id_base, v["plist"].data_ptr(), v["pcnt"].data_ptr(), v["D"].data_ptr(), v["I"].data_ptr(),
                                    None if sel is None else sel.data_ptr(), P(ex), 0 if exclude is None else exclude.shape[1], _lib.stream()),
          f"keds_search_exact_sel n {n} chunk_rows {chunk_rows} k {k}")
    fills = dict(D=SENTF, I=SENT64, plist=SENT64, pcnt=SENT32, counters=9)
    ok = all(_guards_ok(bufs[name][0], fills[name]) for name in bufs)
    c = v["counters"].cpu().numpy()
    ok = ok and c[0] == nfail and (c[8:8 + nfail] == nchunks).all() and (c[8 + nfail:] == 9).all()
    return v["D"].cpu().numpy().reshape(nq, k), v["I"].cpu().numpy().reshape(nq, k), ok


def _allowed(n, nq, elig, exclude, id_base):
    """bool [nq, n]: row r may be returned to query q"""
    a = np.broadcast_to(elig[:n][None, :], (nq, n)).copy()
    if exclude is not None:
        for q in range(nq):
            loc = exclude[q] - id_base
            loc = loc[(exclude[q] >= id_base) & (loc < n) & (loc >= 0)]
            a[q, loc] = False
    return a


def _best_allowed(dist, allowed, metric, count):
    """[nq, count] local ids of each query's best allowed rows by (distance, id); -1 where there are fewer"""
    nq, n = dist.shape
    out = np.full((nq, count), -1, np.int64)
    key = dist if metric == sc.L2 else -dist
    for q in range(nq):
        rows = np.nonzero(allowed[q])[0]
        best = rows[np.lexsort((rows, key[q, rows]))][:count]
        out[q, :len(best)] = best
    return out


@pytest.mark.parametrize("metric", (sc.L2, sc.IP))
@pytest.mark.parametrize("n", (1, 2056, 5000))
def test_exact_pass_selector_and_exclusions(n, metric):
    """selector and exclusions together against search_check's model of the pass on the rerank entry's fp32 distances, the rows that are not
    allowed taken out (a NaN distance is within no bound); id_base 2^33 + 5; 1 / 5 failed queries of 8; the counters as ever"""
    t = Tally(f"exact_sel.n{n}.m{metric}")
    dim, nq, id_base = 128, 8, BIG_BASE
    rs = np.random.RandomState(n)
    for regime in ("integer", "random"):
        x, q = sc.make_inputs(regime, n, dim, nq, seed=n)
        if n > 40:
            x[n - 1] = x[17]
            x[n // 2] = x[17]
        rows_d = _dev(x)
        dist = _all_distances(rows_d, x, q, dim, metric)
        worse = np.float32(np.inf if metric == sc.L2 else -np.inf)
        S = -(-n // 32)
        selectors = {"half": rs.rand(S * 32) < 0.5, "ones": np.ones(S * 32, bool), "zero": np.zeros(S * 32, bool), "none": None}
        if n > 40:
            selectors["half"][[17, n - 1]] = True                 # the duplicate pair stays in play
        for sname, elig in selectors.items():
            el = np.ones(S * 32, bool) if elig is None else elig
            wsel, sel = (None, None) if elig is None else _sel_dev(_words(elig))
            best = _best_allowed(dist, _allowed(n, nq, el, None, id_base), metric, 20)
            ex = np.full((nq, 16), -1, np.int64)
            for qi in range(nq):                                  # the query's best rows, an ineligible row, duplicates, absent ids, -1
                b = best[qi][best[qi] >= 0] + id_base
                inel = np.nonzero(~el[:n])[0]
                row = np.concatenate([b[:(0, 1, 3, 16)[qi % 4]], b[:1], inel[:1] + id_base, [id_base + n, id_base - 1, -1, qi + (1 << 32) + id_base]])
                ex[qi, :min(len(row), 16)] = row[:16]
            for E in (16, 2, None):
                exq = None if E is None else np.ascontiguousarray(ex[:, :E])
                allowed = _allowed(n, nq, el, exq, id_base)
                dmask = np.where(allowed, dist, np.float32(np.nan))
                for chunk_rows in ((8, 64, 2048) if sname == "half" else (64,)):
                    if -(-n // chunk_rows) > 2048:
                        continue
                    for k in (1, 16, 128):
                        for fail_ids in ((5,), (6, 1, 3, 0, 5)):
                            key = dmask if metric == sc.L2 else -dmask
                            srt = np.sort(key, 1)                # NaN last
                            kth = srt[:, min(k, n) - 1] * (1 if metric == sc.L2 else -1)
                            kth = np.where(np.isnan(kth), worse, kth)
                            dup = dist[:, 17] if n > 40 else kth
                            tight = np.nextafter(dup, -worse).astype(np.float32)
                            dk = np.stack([np.full(nq, worse), kth, tight])[np.arange(nq) % 3, np.arange(nq)].astype(np.float32)
                            D, I, ok = _exact_sel(rows_d, n, dim, metric, q, fail_ids, dk, chunk_rows, k, id_base, sel, exq)
                            before_D, before_I = np.full((nq, k), SENTF, np.float32), np.full((nq, k), SENT64, np.int64)
                            msgs = sc.exact_failures(dmask[list(fail_ids)].reshape(len(fail_ids), n), dk[list(fail_ids)], k, metric, id_base, list(fail_ids),
                                                     D, I, before_D, before_I)
                            t.add(regime, msgs, 0.0, ok and (wsel is None or _guards_ok(wsel, SELFILL)),
                                  f"{regime} sel {sname} E {E} chunk_rows {chunk_rows} k {k} failed {fail_ids}: ")
    t.finish()


# ---- the whole search -----------------------------------------------------------------------------------------------------------------
def _expect(dist, best, k, metric, id_base):
    """best: _best_allowed(dist, allowed, metric, >= k) -> the top-k by (fp32 distance, id) over the allowed rows, fillers behind:
    (D [nq, k], I [nq, k])"""
    ids = best[:, :k]
    nq = dist.shape[0]
    D = np.where(ids >= 0, dist[np.arange(nq)[:, None], np.maximum(ids, 0)], np.float32(np.inf if metric == sc.L2 else -np.inf)).astype(np.float32)
    return D, np.where(ids >= 0, ids + id_base, -1)


class WholeCase:
    """one database in one FlatIndex, the fp32 distances of the queries to every row as the rerank entry computes them"""

    def __init__(self, dim, n, metric, row0, nq=24):
        self.dim, self.n, self.metric, self.row0, self.nq = dim, n, metric, row0, nq
        self.x, q = sc.make_inputs("random", n, dim, nq, seed=dim + n)
        self.own = np.arange(nq // 2) * 37 % n                   # the first half of the queries ARE database rows
        q[:nq // 2] = self.x[self.own]
        self.q = q
        self.index = FlatIndex(dim, "l2" if metric == sc.L2 else "ip", device=DEV, row0=row0)
        self.index.add(self.x)
        self.q_d = _dev(q)
        self.dist = _all_distances(self.index.rows, self.x, q, dim, metric)
        self.cache = {}                                           # what the plain and the forced-exact run share: selectors, references

    def once(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def search(self, k, sel=None, exclude=None, gather=False):
        self.index.certificate_counts(reset=True)
        D, I, rows = self.index.search_device(self.q_d, k, sel=sel, exclude=exclude, gather=gather)
        torch.cuda.synchronize()
        counts = self.index.certificate_counts(reset=True)
        return D.cpu().numpy(), I.cpu().numpy(), counts, rows


def _whole_selector_cases(c, rs):
    """name -> bool [n]: densities 100 %, 50 %, 1 % and eligible-row counts between k and ncand, below k, 0"""
    n = c.n
    pick = lambda m: np.isin(np.arange(n), rs.permutation(n)[:m])
    return {"all": np.ones(n, bool), "half": rs.rand(n) < 0.5, "percent": rs.rand(n) < 0.01, "count40": pick(40), "count200": pick(200),
            "count5": pick(5), "count0": np.zeros(n, bool)}


def _run_whole(t, c, ks, force):
    """every selector case x every k, then the exclusions; -> {case: (D, I)} for the comparison of the two runs"""
    out = {}
    rs = np.random.RandomState(c.dim + c.n)
    L2 = c.metric == sc.L2

    def sub_index(rows):
        sub = FlatIndex(c.dim, "l2" if L2 else "ip", device=DEV)
        sub.add(c.x[rows])
        return sub

    for name, mask in c.once("selectors", lambda: _whole_selector_cases(c, rs)).items():
        sel = Selector.from_mask(mask, device=DEV)
        rows = np.nonzero(mask)[0]
        sub = c.once(("sub", name), lambda: sub_index(rows)) if len(rows) else None
        best = c.once(("best", name), lambda: _best_allowed(c.dist, np.broadcast_to(mask[None, :], (c.nq, c.n)), c.metric, max(ks)))
        for k in ks:
            what = f"dim {c.dim} n {c.n} metric {c.metric} sel {name} k {k} force {force}: "
            D, I, counts, _ = c.search(k, sel=sel)
            msgs = []
            if sub is not None:                                   # an index of the eligible rows alone
                Ds, Is, _ = sub.search_device(c.q_d, k)
                Ds, Is = Ds.cpu().numpy(), Is.cpu().numpy()
                Is = np.where(Is >= 0, rows[np.maximum(Is, 0)] + c.row0, -1)
            else:
                Ds, Is = np.full((c.nq, k), np.inf if L2 else -np.inf, np.float32), np.full((c.nq, k), -1, np.int64)
            if not (sc.same_bits(D, Ds) and np.array_equal(I, Is)):
                msgs.append(f"differs from the index of the eligible rows (D {int((sc.f32_bits(D) != sc.f32_bits(Ds)).sum())}, I {int((I != Is).sum())} places)")
            De, Ie = _expect(c.dist, best, k, c.metric, c.row0)
            if not (sc.same_bits(D, De) and np.array_equal(I, Ie)):
                msgs.append(f"differs from the top-k of the fp32 distances (D {int((sc.f32_bits(D) != sc.f32_bits(De)).sum())}, I {int((I != Ie).sum())} places)")
            if sum(counts) != c.nq or (force and counts[0] != 0):
                msgs.append(f"certified + fallback = {counts} of {c.nq} queries")
            t.add("selector", msgs, 0.0, True, what)
            out[name, k] = (D, I)
    # exclusions: own row (the first half of the queries are database rows), the query's best rows, absent ids, duplicates, -1
    best = c.once(("best", "all"), lambda: None)[:, :16]
    half = c.once("exclude_half", lambda: rs.rand(c.n) < 0.5)
    for E in (1, 5, 16):
        ex = np.full((c.nq, E), -1, np.int64)
        ex[:c.nq // 2, 0] = c.own + c.row0
        if E > 1:
            for q in range(c.nq):
                row = np.concatenate([best[q, :(E - 2, 1, 0)[q % 3]] + c.row0, [c.row0 + c.n, -1, best[q, 0] + c.row0, best[q, 0] + c.row0 + (1 << 32)]])
                m = min(len(row), E - 1)
                ex[q, 1:1 + m] = row[:m]
        for sname, mask in (("none", None), ("half", half)):
            sel = None if mask is None else Selector.from_mask(mask, device=DEV)
            best_ex = c.once(("best_ex", E, sname), lambda: _best_allowed(
                c.dist, _allowed(c.n, c.nq, np.ones(c.n, bool) if mask is None else mask, ex, c.row0), c.metric, max(ks)))
            for k in ks:
                what = f"dim {c.dim} n {c.n} metric {c.metric} exclude E {E} sel {sname} k {k} force {force}: "
                D, I, counts, rows_g = c.search(k, sel=sel, exclude=ex if E > 1 else ex[:, 0], gather=True)
                msgs = []
                De, Ie = _expect(c.dist, best_ex, k, c.metric, c.row0)
                if not (sc.same_bits(D, De) and np.array_equal(I, Ie)):
                    msgs.append(f"differs from the top-k of the fp32 distances (D {int((sc.f32_bits(D) != sc.f32_bits(De)).sum())}, I {int((I != Ie).sum())} places)")
                if _hit(I, ex):
                    msgs.append("an excluded id was returned")
                if (I[:c.nq // 2] == (c.own + c.row0)[:, None]).any():
                    msgs.append("a query that is a database row got its own row back")
                want_rows = np.where((I >= 0)[..., None], c.x[np.maximum(I - c.row0, 0)], np.float32(0))
                if not sc.same_bits(rows_g.cpu().numpy(), want_rows):
                    msgs.append("the gathered rows are not the rows of I")
                if mask is None:                                  # the unfiltered search with k + E, the excluded ids removed, cut at k
                    kk = min(k + E, _lib.SCAN_MAX_K)
                    Du, Iu, _, _ = c.search(kk)
                    for q in range(c.nq):
                        keep = ~np.isin(Iu[q], ex[q][ex[q] >= 0])
                        m = min(int(keep.sum()), k)               # k = 128: the search returns no more than 128, the first 128 - E places
                        if not (sc.same_bits(D[q, :m], Du[q][keep][:m]) and np.array_equal(I[q, :m], Iu[q][keep][:m])) or (kk == k + E and m < k):
                            msgs.append(f"query {q}: differs from the unfiltered top-{kk} without the excluded ids")
                            break
                if sum(counts) != c.nq:
                    msgs.append(f"certified + fallback = {counts} of {c.nq} queries")
                t.add("exclude", msgs, 0.0, True, what)
                out["ex", E, sname, k] = (D, I)
    return out


@pytest.mark.parametrize("metric", (sc.L2, sc.IP))
@pytest.mark.parametrize("dim,n", ((128, 5000), (128, 40000), (768, 5000), (768, 40000)))
def test_whole_search(dim, n, metric):
    """one phase (5,000 rows) and two phases (40,000), both metrics, k = 1, 16, 17, 128, every density and eligible-row count, the exclusions;
    then everything once more with every query sent through the exact pass: the same bits"""
    lib = _lib.load()
    t = Tally(f"whole_sel.{dim}.n{n}.m{metric}")
    c = WholeCase(dim, n, metric, row0=BIG_BASE if n == 5000 else 0)
    ks = (1, 16, 17, 128)
    first = _run_whole(t, c, ks, force=0)
    try:
        lib.keds_scan_debug(1 << 5)
        second = _run_whole(t, c, ks, force=1)
    finally:
        lib.keds_scan_debug(0)
    differ = [key for key in first if not (sc.same_bits(first[key][0], second[key][0]) and np.array_equal(first[key][1], second[key][1]))]
    t.add("exact_rerun", [f"{len(differ)} cases differ when every query takes the exact pass (first: {differ[0]})"] if differ else [])
    assert first.keys() == second.keys() and len(first) == 7 * 4 + 3 * 2 * 4
    t.finish()


def test_selector_of_another_size_is_refused():
    c = WholeCase(128, 100, sc.L2, 0, nq=2)
    with pytest.raises(ValueError):
        c.index.search_device(c.q_d, 1, sel=Selector.from_mask(np.ones(99, bool), device=DEV))
    with pytest.raises(ValueError):
        c.index.search_device(c.q_d, 1, exclude=np.zeros((2, 17), np.int64))
    with pytest.raises(ValueError):
        c.index.search_device(c.q_d, 1, exclude=np.zeros((3, 1), np.int64))
    D, I = c.index.search(c.q, 3, sel=Selector.from_mask(np.arange(100) % 2 == 0), exclude=np.array([0, -1]))      # numpy in, host selector
    assert isinstance(D, np.ndarray) and (I % 2 == 0).all() and 0 not in I[0]


# ---- shards ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", (sc.L2, sc.IP))
def test_three_shards_equal_the_single_filtered_index(metric):
    """three FlatIndex shards on shard_bounds, each with Selector.shard of one global selector, merged by topk_merge_parts: the single
    filtered index bit for bit.  n is no multiple of 32; the shards' densities are 50 %, 0 (no eligible row) and 1 %"""
    t = Tally(f"shards_sel.m{metric}")
    dim, n, nq = 128, 5000 + 13, 24
    name = "l2" if metric == sc.L2 else "ip"
    x, q = sc.make_inputs("random", n, dim, nq, seed=3)
    q[:4] = x[[0, 1700, 3400, n - 1]]
    rs = np.random.RandomState(8)
    bounds = [shard_bounds(n, 3, r) for r in range(3)]
    assert bounds[0][0] == 0 and bounds[2][1] == n and all(lo % 32 == 0 for lo, _ in bounds) and n % 32
    mask = np.zeros(n, bool)
    mask[bounds[0][0]:bounds[0][1]] = rs.rand(bounds[0][1] - bounds[0][0]) < 0.5
    mask[bounds[2][0]:bounds[2][1]] = rs.rand(bounds[2][1] - bounds[2][0]) < 0.01
    mask[n - 1] = True
    sel = Selector.from_mask(mask, device=DEV)
    whole = FlatIndex(dim, name, device=DEV)
    whole.add(x)
    shards = []
    for lo, hi in bounds:
        ix = FlatIndex(dim, name, device=DEV, row0=lo)
        ix.add(x[lo:hi])
        shards.append(ix)
    q_d = _dev(q)
    ex = np.full((nq, 2), -1, np.int64)
    ex[:4, 0] = [0, 1700, 3400, n - 1]
    ex[:, 1] = np.nonzero(mask)[0][np.arange(nq) % mask.sum()]
    for k in (1, 16, 128):
        for exclude in (None, ex):
            D, I, _ = whole.search_device(q_d, k, sel=sel, exclude=exclude)
            parts = [ix.search_device(q_d, k, sel=sel.shard(lo, hi), exclude=exclude) for ix, (lo, hi) in zip(shards, bounds)]
            empty = parts[1][1].cpu().numpy()
            Dm, Im = ops.topk_merge_parts(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), shards[0].metric)
            msgs = []
            if not (sc.same_bits(D.cpu().numpy(), Dm.cpu().numpy()) and np.array_equal(I.cpu().numpy(), Im.cpu().numpy())):
                msgs.append("the merged shards differ from the single filtered index")
            if not (empty == -1).all():
                msgs.append("the shard without an eligible row returned a row")
            got = I.cpu().numpy()
            if not mask[got[got >= 0]].all() or (exclude is not None and _hit(got, ex)):
                msgs.append("an ineligible or excluded row was returned")
            t.add("bits", msgs, 0.0, True, f"k {k} exclude {'given' if exclude is not None else 'none'}: ")
    t.finish()


# ---- get_retrieved_features -----------------------------------------------------------------------------------------------------------
def test_get_retrieved_features_leaves_the_excluded_rows_out():
    dim, n, B, k = 128, 300, 6, 16
    x_img, feat = sc.make_inputs("random", n, dim, B, seed=1)
    x_txt, _ = sc.make_inputs("random", n, dim, B, seed=2)
    own = np.array([5, 77, 123, 200, 31, 299])
    feat = (3.0 * x_img[own]).astype(np.float32)                  # any norm: the features of database images
    x_txt[own] = x_img[own]
    image_index, text_index = FlatIndex(dim, "l2", device=DEV), FlatIndex(dim, "l2", device=DEV)
    image_index.add(x_img)
    text_index.add(x_txt)
    database = (None, None, None, image_index, text_index)
    f_d = _dev(feat)
    ti0, tt0 = keds_amd.get_retrieved_features(f_d, database, None, topk=k)
    assert sc.same_bits(ti0[:, 0].cpu().numpy(), x_img[own]) and sc.same_bits(tt0[:, 0].cpu().numpy(), x_txt[own])     # neighbour 0 is the image itself
    for exclude in (own.astype(np.int64), np.stack([own, (own + 1) % n, np.full(B, -1)], 1).astype(np.int64), torch.from_numpy(own).to(DEV)):
        ti, tt = keds_amd.get_retrieved_features(f_d, database, None, topk=k, exclude=exclude)
        ex = exclude.cpu().numpy() if isinstance(exclude, torch.Tensor) else exclude
        ex = ex[:, None] if ex.ndim == 1 else ex
        for index, got, x in ((image_index, ti, x_img), (text_index, tt, x_txt)):
            _, I, _ = index.search_device(f_d, k, normalize=True, exclude=exclude)
            I = I.cpu().numpy()
            assert not _hit(I, ex) and (I >= 0).all()
            assert sc.same_bits(got.cpu().numpy(), x[I])                                  # the gather of the filtered ids
            _, Iu, _ = index.search_device(f_d, k + ex.shape[1], normalize=True)
            Iu = Iu.cpu().numpy()
            for b in range(B):
                assert np.array_equal(I[b], Iu[b][~np.isin(Iu[b], ex[b])][:k])
    ti1, tt1 = keds_amd.get_retrieved_features(f_d, database, None, topk=k, exclude=None)
    assert sc.same_bits(ti1.cpu().numpy(), ti0.cpu().numpy()) and sc.same_bits(tt1.cpu().numpy(), tt0.cpu().numpy())
