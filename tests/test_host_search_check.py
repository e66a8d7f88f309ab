"""Proof, on the CPU, that the checks of the search kernels (tests/search_check.py) pass models of the stages -- the scan's scores
accumulated in fp32 in 32-wide steps from the bias, forwards and reversed; everything else integer algorithms -- in every regime, and
catch every mutation of the models by >= 4 x the bound or by bits; which of the mutations today's end-to-end assertions
(test_gpu_search._check on iid rows, 20000 x 128) let through; and that a Python model of the launch plan's rules equals
keds_index_search_plan_query everywhere while the plan's invariants hold."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import search_check as sc

FACTOR = 4.0
SENT = 0x5EA5C0DE5EA5C0DE
NQ = 12


def _bits_of(rows):
    return sc.bf16_bits(rows)


@functools.lru_cache(maxsize=None)
def _scan_case(regime, dim, nwg=2, extra=1, seed=0):
    """rows of 2 NST + 1 stages per workgroup (+ a partial last stage), their image operands and float64 scores"""
    nst = sc.ring_depth(dim)
    stages = nwg * (2 * nst + 1) + extra
    n = stages * 32 - 31                                         # the last stage holds one real key
    keys = sc.placed_keys(n, stages, nwg, dim) if regime == "placed" else ()
    x, q = sc.make_inputs(regime, n, dim, NQ, seed=seed, placed_keys=tuple(keys))
    xb = np.zeros((stages * 32, dim), np.uint16)
    xb[:n] = _bits_of(x)
    bias = np.full(stages * 32, -np.inf, np.float32)
    bias[:n] = (-0.5 * (x.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    qb = _bits_of(q)
    s64, e64 = sc.scan_scores64(xb, bias, qb)
    return dict(n=n, stages=stages, nwg=nwg, dim=dim, xb=xb, bias=bias, qb=qb, s64=s64, e64=e64, x=x, q=q)


def _thr_for(case, kind):
    if kind == "none":
        return None
    if kind == "-inf":
        return np.full(NQ, -np.inf, np.float32)
    if kind == "+inf":
        return np.full(NQ, np.inf, np.float32)
    s = sc.scan_scores_model(case["xb"], case["bias"], case["qb"])[:, :case["n"]]
    if kind == "p97":                                            # most lists hold a few entries, none is full at depth 16
        return np.percentile(s, 97, axis=1).astype(np.float32)
    return np.median(s, axis=1).astype(np.float32) if kind == "median" else s.max(1)          # "exact": an existing score, the best


def _run_scan(case, depth, thr, order="forward", mutation=None, **score_mut):
    scores = sc.scan_scores_model(case["xb"], case["bias"], case["qb"], order=order, **score_mut)
    pairs, meta = sc.scan_lists_model(scores, case["n"], case["stages"], case["nwg"], depth, thr, SENT, mutation=mutation,
                                      ring=sc.ring_depth(case["dim"]))
    return pairs, meta


def _scan_check(case, depth, thr, pairs, meta, what=""):
    return sc.scan_failures(case["s64"], case["e64"], case["n"], case["stages"], case["nwg"], depth, thr, pairs, meta, SENT, what)


# ---- formats and the image ----------------------------------------------------------------------------------------------------------
def test_formats_agree_with_torch():
    import torch
    rs = np.random.RandomState(0)
    x = np.concatenate([rs.standard_normal(4096) * 10.0 ** rs.randint(-20, 20, 4096), [0.0, -0.0, 1.0, 1.00390625, 1.01171875]]).astype(np.float32)
    assert np.array_equal(sc.bf16_round(x), torch.from_numpy(x).bfloat16().float().numpy())
    f = np.concatenate([x, [np.inf, -np.inf]]).astype(np.float32)
    k = sc.ord_key(f)
    assert sc.same_bits(sc.key_float(k), f)
    nz = f != 0                                                   # (-0 sorts below +0 as a key, equal as a float)
    o = np.argsort(f[nz], kind="stable")
    assert (np.diff(k[nz][o].astype(np.int64)) >= 0).all()
    assert sc.ord_key(np.float32(-0.0)) < sc.ord_key(np.float32(0.0)) and sc.ord_key(np.float32(-np.inf)) == sc.NEG_INF_KEY
    assert [sc.ring_depth(d) for d in sc.DIMS] == [8, 8, 4, 3, 2]


def _pack_model(x, metric):
    """the image as pack_kernel writes it (bias and bounds in float64 rounded once: inside every bound)"""
    n, dim = x.shape
    S = -(-n // 32)
    img = np.zeros(sc.packed_bytes(n, dim), np.uint8)
    keys = np.zeros((S * 32, dim), np.uint16)
    keys[:n] = sc.bf16_bits(x)
    chunks = dim // 8
    body = img[:S * sc.stage_bytes(dim)].reshape(S, sc.stage_bytes(dim))
    raw = np.zeros((S, 32, chunks, 8), np.uint16)
    row, ch = np.arange(32)[:, None], np.arange(chunks)[None, :]
    raw[:, row, sc.swz_chunk(ch, row), :] = keys.reshape(S, 32, chunks, 8)
    body[:, :32 * dim * 2] = raw.reshape(S, -1).view(np.uint8)
    bias = np.full(S * 32, -np.inf, np.float32)
    x64 = x.astype(np.float64)
    bias[:n] = -0.5 * (x64 ** 2).sum(1) if metric == sc.L2 else 0.0
    body[:, 32 * dim * 2:] = bias.reshape(S, 32).view(np.uint8)
    xt = sc.bf16_round(x).astype(np.float64)
    b = np.array([np.sqrt((xt ** 2).sum(1)).max(), np.sqrt(((x64 - xt) ** 2).sum(1)).max(), np.sqrt((x64 ** 2).sum(1)).max(), 0.0])
    b32 = (b * (1 + 5e-7)).astype(np.float32)
    img[S * sc.stage_bytes(dim):][:16] = b32.view(np.uint8)
    return img


@pytest.mark.parametrize("dim", sc.DIMS)
def test_pack_model_passes_and_mutations_fail(dim):
    for regime in ("integer", "random", "bignorm"):
        for metric in (sc.L2, sc.IP):
            x, _ = sc.make_inputs(regime, 33, dim, 1)
            img = _pack_model(x, metric)
            msgs, worst = sc.pack_failures(x, metric, img)
            assert not msgs and worst <= 1.0, msgs
            d = sc.decode_image(img, 33, dim)
            assert np.array_equal(d["keys"][:33], sc.bf16_bits(x))
    x, _ = sc.make_inputs("random", 33, dim, 1)
    img = _pack_model(x, sc.L2)
    sb = sc.stage_bytes(dim)
    for name, edit in (("key_byte", lambda a: a.__setitem__(dim * 2 * 3 + 2, a[dim * 2 * 3 + 2] ^ 1)),
                       ("pad_bias", lambda a: a[sb + 32 * dim * 2 + 4 * 5:sb + 32 * dim * 2 + 4 * 6].__setitem__(slice(None), 0)),
                       ("bound_low", lambda a: a[2 * sb:2 * sb + 4].__setitem__(slice(None), np.array([0.5], np.float32).view(np.uint8))),
                       ("bias_next_row", lambda a: a[32 * dim * 2:32 * dim * 2 + 4].__setitem__(slice(None), np.array([-0.6], np.float32).view(np.uint8)))):
        bad = img.copy()
        edit(bad)
        msgs, _ = sc.pack_failures(x, sc.L2, bad)
        assert msgs, name


# ---- scan ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", sc.DIMS)
@pytest.mark.parametrize("regime", sc.REGIMES)
def test_scan_models_pass_in_every_regime(regime, dim):
    case = _scan_case(regime, dim)
    top = 0.0
    for depth in (1, 4, 16):
        for kind in ("none", "-inf", "median", "p97", "exact", "+inf"):
            thr = _thr_for(case, kind)
            for order in ("forward", "reverse"):
                pairs, meta = _run_scan(case, depth, thr, order)
                msgs, worst = _scan_check(case, depth, thr, pairs, meta, f"{regime}.{dim}.L{depth}.{kind}.{order}: ")
                assert not msgs, "\n".join(msgs[:5])
                top = max(top, worst)
    print(f"[model] scan {regime} dim {dim}: worst |score - s| / e = {top:.3g}")
    assert top <= 1.0
    if regime == "integer":
        assert top == 0.0                                        # exact in bf16 and fp32: everything by bits


# mutation -> (regime, depth, thr kind, caught by "bound" (>= FACTOR x e) or "bits")
SCAN_MUTATIONS = {
    "ring_early": ("random", 16, "none", "bound"),
    "bias_next_row": ("bignorm", 16, "none", "bound"),
    "swizzle_no_mask": ("random", 16, "none", "bound"),
    "tie_displaces": ("integer", 4, "none", "bits"),
    "short5": ("ramp_up", 16, "none", "bits"),
    "thr_ge": ("integer", 16, "exact", "bits"),
    "pad_listed": ("random", 16, "none", "bits"),
    "metay_unfilled": ("random", 16, "p97", "bits"),
    "metay_missing": ("ramp_down", 4, "none", "bits"),
    "quarters_reversed": ("random", 4, "none", "bits"),
}
SCAN_FACTORS = {}


def _mutated_scan(case, name, depth, thr):
    if name == "bias_next_row":
        return _run_scan(case, depth, thr, bias_shift=1)
    if name == "swizzle_no_mask":
        return _run_scan(case, depth, thr, swz_mask=False)
    return _run_scan(case, depth, thr, mutation=name)


@pytest.mark.parametrize("dim", sc.DIMS)
@pytest.mark.parametrize("name", sorted(SCAN_MUTATIONS))
def test_scan_mutations_are_caught(name, dim):
    regime, depth, kind, how = SCAN_MUTATIONS[name]
    case = _scan_case(regime, dim)
    thr = _thr_for(case, kind)
    pairs, meta = _mutated_scan(case, name, depth, thr)
    msgs, worst = _scan_check(case, depth, thr, pairs, meta)
    if regime == "integer":                                      # the device test compares with the model by bits there
        good = _run_scan(case, depth, thr)
        differs = not (np.array_equal(pairs, good[0]) and np.array_equal(meta, good[1]))
        assert differs, f"{name}: the mutation changes nothing at dim {dim}"
        msgs = msgs or ["differs from the model by bits"]
    assert msgs, f"{name} at dim {dim}: not caught"
    if how == "bound":
        assert worst >= FACTOR, f"{name} at dim {dim}: only {worst:.3g} x e"
        SCAN_FACTORS[name] = min(SCAN_FACTORS.get(name, np.inf), worst)
        print(f"[factor] scan {name} dim {dim}: {worst:.3g}")


def test_stale_lmin_changes_no_result():
    """`lmin` left stale after an insert only admits scores the sorted insert then drops again (it never rises above the true
    threshold): a cost, not a wrong list.  No check of results can see it, and none has to."""
    for regime in ("integer", "ramp_up", "random"):
        case = _scan_case(regime, 128)
        for depth in (1, 4, 16):
            a = _run_scan(case, depth, None)
            b = _run_scan(case, depth, None, mutation="lmin_stale")
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- merge --------------------------------------------------------------------------------------------------------------------------
def _merge_case(kind, V, nwg, slots, ncand, seed=0, metay=0, nq=3):
    rs = np.random.RandomState(seed + V + nwg)
    P, M = [], []
    for _ in range(nq):
        keys = sc.key_set(kind, V, ncand, rs)
        cnts = sc.spread_counts(len(keys), nwg, slots, rs)
        p, m = sc.synth_segments(cnts, slots, keys, rs, metay=metay)
        P.append(p)
        M.append(m)
    return np.stack(P), np.stack(M)


MERGE_KEYSETS = ("equal", "random", "straddle", ("bit", 0), ("bit", 7), ("bit", 8), ("bit", 15), ("bit", 16), ("bit", 23), ("bit", 24), ("bit", 31),
                 ("ties", 2, 1), ("ties", 256, 3), ("ties", 257, 3), ("ties", 300, 40))


@pytest.mark.parametrize("ncand", (64, 256))
def test_merge_model_passes_every_key_set(ncand):
    T = 0xC0000000
    for kind in MERGE_KEYSETS:
        for V in (0, ncand - 1, ncand, ncand + 1, 4096, 4097):
            if isinstance(kind, tuple) and kind[0] == "ties" and V < ncand + kind[1]:
                continue
            for metay, thr_in in ((0, None), (T - 5, 3.0e38), (0xFF000000, -3.0e38), (0, 3.0e38)):
                pairs, meta = _merge_case(kind, V, 128, 64, ncand, metay=metay)
                ti = None if thr_in is None else np.full(3, thr_in, np.float32)
                ci, cv, to, sb = sc.merge_model(pairs, meta, ncand, ti)
                msgs = sc.merge_failures(pairs, meta, ncand, ti, ci, cv, to, sb, f"{kind}.V{V}: ")
                assert not msgs, msgs[:3]


MERGE_MUTATIONS = {
    "cut_high": ("random", 1000), "cut_low": ("random", 1000), "ties_largest": (("ties", 256, 3), 1000), "stale_counted": ("random", 40),
    "drop_last_segment": ("random", 40), "sbound_no_metay": ("random", 1000), "sbound_no_thr": ("random", 40), "no_fillers": ("random", 40),
    ("dropbit", 7): (("bit", 7), 1000), ("dropbit", 8): (("bit", 8), 1000), ("dropbit", 23): (("bit", 23), 1000),
    ("dropbit", 24): (("bit", 24), 1000), ("dropbit", 31): (("bit", 31), 1000),
}


@pytest.mark.parametrize("ncand", (64, 256))
@pytest.mark.parametrize("name", list(MERGE_MUTATIONS), ids=str)
def test_merge_mutations_are_caught(name, ncand):
    kind, V = MERGE_MUTATIONS[name]
    V = V if V > 100 else ncand - 24
    rs = np.random.RandomState(5)
    P, M = [], []
    for _ in range(3):
        keys = sc.key_set(kind, V, ncand, rs)
        cnts = sc.spread_counts(V, 128, 64, rs)
        cnts[127] = max(cnts[127], 1) if name == "drop_last_segment" else cnts[127]
        if cnts.sum() != V:
            cnts[int(np.argmax(cnts[:127]))] -= cnts.sum() - V
        p, m = sc.synth_segments(cnts, 64, keys, rs, metay=0xFF000000 if name == "sbound_no_metay" else 0)
        P.append(p)
        M.append(m)
    pairs, meta = np.stack(P), np.stack(M)
    ti = np.full(3, 3.0e38, np.float32)
    ci, cv, to, sb = sc.merge_model(pairs, meta, ncand, ti, mutation=name)
    assert sc.merge_failures(pairs, meta, ncand, ti, ci, cv, to, sb), f"{name}: not caught"


# ---- rerank / certify / exact -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", sc.DIMS)
def test_distance_model_fits_the_bound(dim):
    for regime in ("integer", "random", "bignorm", "offset"):
        x, q = sc.make_inputs(regime, 200, dim, 8)
        for metric in (sc.L2, sc.IP):
            for order in ("forward", "reverse"):
                idx = np.tile(np.arange(64, dtype=np.int32), (8, 1))
                idx[:, 60:] = -1
                d = sc.dist_model(q[:, None, :], x[np.maximum(idx, 0)], metric, order).astype(np.float32)
                d[idx < 0] = np.inf if metric == sc.L2 else -np.inf
                msgs, worst = sc.rerank_failures(q, x, metric, idx, d)
                assert not msgs and worst <= 1.0, (regime, metric, order, worst)
                # a distance to row id + 1 fails by far more than the bound
                bad = sc.dist_model(q[:, None, :], x[np.maximum(idx, 0) + 1], metric, order).astype(np.float32)
                bad[idx < 0] = d[idx < 0]
                msgs, worst = sc.rerank_failures(q, x, metric, idx, bad)
                assert msgs and worst >= FACTOR


CERT_MUTATIONS = ("ties_larger_id", "dk_rank_k", "certify_short", "eps_no_qr", "no_id_base")


@pytest.mark.parametrize("metric", (sc.L2, sc.IP))
@pytest.mark.parametrize("k,ncand", [(1, 64), (16, 64), (17, 256), (128, 256)])
def test_certify_model_passes_and_mutations_fail(k, ncand, metric):
    ci, cd, qstat, sbound, bounds = sc.cert_case(metric, k, ncand)
    nq = ci.shape[0]
    id_base = 1 << 33

    def run(mutation=None, force=0):
        m = sc.certify_model(ci, cd, metric, k, id_base, qstat, sbound, bounds, force, 7.0, 128, mutation=mutation)
        failed = np.nonzero(~m["verdict"])[0]
        fslot = np.full(nq, -1, np.int32)
        fslot[failed] = np.arange(len(failed))[::-1]              # any order of arrival
        fail_ids = np.full(nq, -5, np.int32)
        fail_ids[fslot[failed]] = failed
        counters = np.full(8 + nq, 9, np.int32)
        counters[0] = len(failed)
        counters[8:8 + len(failed)] = 0
        res = dict(D=m["D"], I=m["I"], fslot=fslot, fail_ids=fail_ids, counters=counters, dk=m["dk"],
                   status=np.array([nq - len(failed), len(failed)], np.int32))
        return sc.certify_failures(ci, cd, metric, k, id_base, qstat, sbound, bounds, force, res, 7.0, 128)[0]

    assert not run(), run()[:3]
    assert not run(force=1)
    for mutation in CERT_MUTATIONS:
        if mutation == "dk_rank_k" and k == ncand:
            continue
        assert run(mutation), f"{mutation}: not caught (k {k}, ncand {ncand}, metric {metric})"


EXACT_MUTATIONS = ("prune_strict", "skip_last_chunk", "lists_256_unread", "pop_twice")


@pytest.mark.parametrize("metric", (sc.L2, sc.IP))
@pytest.mark.parametrize("k", (1, 16, 128))
def test_exact_model_passes_and_mutations_fail(k, metric):
    rs = np.random.RandomState(k)
    n, nf, chunk = 2053, 3, 8                                     # 257 chunks, the last of 5 rows
    dist = rs.randint(0, 400, (nf, n)).astype(np.float32)         # duplicates in plenty
    for f, pos in enumerate((n - 1, 2050, 300)):                  # a best row where each mutation loses it
        dist[f, pos] = -1.0 if metric == sc.L2 else 500.0
    key = dist if metric == sc.L2 else -dist
    kth = np.sort(key, 1)[:, min(k, n) - 1]
    dk = np.stack([np.inf, kth[1], kth[2]]).astype(np.float32) * (1 if metric == sc.L2 else -1)
    before_D, before_I = np.full((5, k), 3.0, np.float32), np.full((5, k), -9, np.int64)
    fail_ids = [4, 0, 2]

    def run(mutation=None):
        D, I = before_D.copy(), before_I.copy()
        d, i = sc.exact_model(dist, dk, k, metric, 1 << 33, chunk, mutation=mutation)
        D[fail_ids], I[fail_ids] = d, i
        return sc.exact_failures(dist, dk, k, metric, 1 << 33, fail_ids, D, I, before_D, before_I)

    assert not run(), run()[:3]
    for mutation in EXACT_MUTATIONS:
        if mutation == "pop_twice" and k == 1:
            continue
        assert run(mutation), f"{mutation}: not caught (k {k})"


# ---- what today's end-to-end assertions let through -----------------------------------------------------------------------------------
def test_which_mutations_the_end_to_end_check_misses():
    """test_gpu_search._check's assertions on iid unit rows, 20000 x 128, nq 37, k 16, applied to a model pipeline (single phase: 625 stages)
    whose scan or merge is mutated while the stages behind it stay right: the final (D, I) equal the float64 top-k for every one of
    these, because 64 candidates per query leave a margin of 48 and the rows are iid.  The per-stage checks above catch them all."""
    n, dim, nq, k, nwg = 20000, 128, 37, 16, 8
    rs = np.random.RandomState(2002)
    x = rs.standard_normal((n, dim))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    q = rs.standard_normal((nq, dim))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    stages = -(-n // 32)
    xb = np.zeros((stages * 32, dim), np.uint16)
    xb[:n] = sc.bf16_bits(x)
    bias = np.full(stages * 32, -np.inf, np.float32)
    bias[:n] = (-0.5 * (x.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    scores = sc.scan_scores_model(xb, bias, sc.bf16_bits(q))
    d64 = -2.0 * sc.t64(q, x, sc.L2)                              # ||q - x||^2 - ||q||^2: the same order per query
    want = np.argsort(d64, 1, kind="stable")[:, :k]
    missed = []
    for scan_mut, merge_mut in [(m, None) for m in ("tie_displaces", "short5", "thr_ge", "metay_unfilled", "metay_missing", "quarters_reversed")] + \
                               [(None, m) for m in ("cut_high", "cut_low", "ties_largest", "sbound_no_metay", "sbound_no_thr")]:
        pairs, meta = sc.scan_lists_model(scores, n, stages, nwg, 16, None, SENT, mutation=scan_mut)
        ci, cv, to, sb = sc.merge_model(pairs, meta, 64, None, mutation=merge_mut)
        d = sc.dist_model(q[:, None, :], x[np.maximum(ci, 0)], sc.L2)
        got = np.take_along_axis(ci, np.lexsort((ci, d), axis=1)[:, :k], 1)
        if np.array_equal(got, want):
            missed.append(scan_mut or merge_mut)
    print("[end-to-end] mutations that pass _check:", missed)
    assert set(missed) >= {"tie_displaces", "thr_ge", "metay_unfilled", "metay_missing", "cut_low", "ties_largest", "sbound_no_metay",
                           "sbound_no_thr"}


# ---- the certificate's premise and claim on the models ---------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ("random", "bignorm"))
def test_model_certificate_is_not_vacuous(regime):
    """the inputs of the device composition: the float64 model of the certificate certifies at least half the queries"""
    n, dim, nq, k = 4096 + 33, 128, 16, 16
    x, q, k = sc.composition_inputs(regime, n, dim, nq, seed=3)
    frac, prem = sc.certificate_model_fraction(x, q, k)
    print(f"[model] {regime}: certified fraction {frac:.3g}, premise ratio {prem:.3g}")
    assert frac >= 0.5 and prem <= 1.0


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
def test_plan_model_equals_the_library_and_invariants_hold():
    from keds_amd import _lib
    lib = _lib.load()
    out = (C.c_int32 * len(sc.PLAN_FIELDS))()
    rs = np.random.RandomState(1)
    ns = [1, 31, 32, 33, 1023 * 32, 1024 * 32, 1024 * 32 + 1, 16384 * 32, 2048 * 16384, 2048 * 16384 - 1] + \
         [int(v) for v in np.exp(rs.uniform(0, np.log(2048 * 16384), 60))]
    cases = refused = 0
    for n in ns:
        for dim in sc.DIMS:
            for cus in (8, 64, 255, 256, 304):
                for nq_set in (1, 128, 129, 1024, int(rs.randint(1, 1025))):
                    for k in (1, 16, 17, 128, int(rs.randint(1, 129))):
                        want = sc.plan_model(nq_set, dim, n, k, cus)
                        rc = lib.keds_index_search_plan_query(nq_set, dim, n, k, cus, out)
                        cases += 1
                        if want is None:
                            refused += 1
                            assert rc != 0, (nq_set, dim, n, k, cus)
                            continue
                        assert rc == 0, (_lib.last_error(), nq_set, dim, n, k, cus)
                        got = dict(zip(sc.PLAN_FIELDS, list(out)))
                        assert got == want, (nq_set, dim, n, k, cus, got, want)
                        msgs = sc.plan_invariant_failures(got, nq_set, dim, n, k)
                        assert not msgs, (msgs, nq_set, dim, n, k, cus)
    print(f"[plan] {cases} cases, {refused} refused")
    assert refused > 0 and refused < cases // 2
    try:                                                          # keds_scan_debug bit 4 (single phase) and bits 7-9 (depth forced)
        for variant, kw in ((16, dict(force_single=True)), (1 << 7, dict(thr_depth=1)), (4 << 7, dict(thr_depth=4))):
            lib.keds_scan_debug(variant)
            for n, nq_set, cus in ((500000, 1024, 256), (500000, 100, 256), (40000, 300, 64)):
                assert lib.keds_index_search_plan_query(nq_set, 768, n, 16, cus, out) == 0
                assert dict(zip(sc.PLAN_FIELDS, list(out))) == sc.plan_model(nq_set, 768, n, 16, cus, **kw)
    finally:
        lib.keds_scan_debug(0)
    for bad in ((0, 128, 10, 1, 8), (1025, 128, 10, 1, 8), (1, 100, 10, 1, 8), (1, 128, 0, 1, 8), (1, 128, 10, 129, 8), (1, 128, 10, 1, 0)):
        assert lib.keds_index_search_plan_query(*bad, out) != 0
