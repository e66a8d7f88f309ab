"""Proof, on the CPU, that the checks of the sharded-search merge (tests/exchange_check.py) pass line-by-line integer models of
exchange_pack_kernel, exchange_merge_kernel and merge_parts_kernel at every table shape and in every regime, that the host twin
keds_amd.index.merge_partials gives the same answer, that every mutation of the models fails by bits wherever it changes anything, and
which of the mutations the earlier end-to-end assertions (iid rows, 3,000 x 128, k = 16, three shards, one duplicate pair) let through."""
import numpy as np
import pytest
import torch

from keds_amd.index import merge_partials, shard_bounds
from tests import exchange_check as xc

SENTF = np.float32(7.25)
SENT64 = 0x5EA5C0DE5EA5C0DE
G = 64


def _guarded(numel, dtype, fill):
    whole = np.full(numel + 2 * G, fill, dtype)
    return whole, whole[G:G + numel]


def _intact(whole, fill):
    return bool((whole[:G] == fill).all() and (whole[-G:] == fill).all())


def _pipeline(D, I, rows, stride, metric, pack_mut=None, merge_mut=None, zero_send=False):
    """pack -> (the all-to-all of one rank's view: part w of the message is list w) -> merge, on guarded sentinel-filled buffers
    -> (send words [world * stride], D, I, rows or None, every guard intact)"""
    world, B, k = D.shape
    dim = 0 if rows is None else rows.shape[3]
    ws, send = _guarded(world * stride, np.uint32, 0 if zero_send else xc.SENT32)
    xc.pack_model(D, I, rows, stride, send.view(np.int32), mutation=pack_mut)
    wD, oD = _guarded(B * k, np.float32, SENTF)
    wI, oI = _guarded(B * k, np.int64, SENT64)
    wR, oR = _guarded(B * k * max(dim, 1), np.float32, SENTF)
    xc.exchange_merge_model(send.view(np.int32), world, B, k, dim, stride, metric, oD, oI, oR if dim else None, mutation=merge_mut)
    ok = _intact(ws, 0 if zero_send else xc.SENT32) and _intact(wD, SENTF) and _intact(wI, SENT64) and _intact(wR, SENTF)
    if not dim:
        ok = ok and bool((oR == SENTF).all())
    return send, oD, oI, (oR if dim else None), ok


def _failures(D, I, rows, stride, metric, run):
    send, oD, oI, oR, ok = run
    msgs = xc.pack_failures(D, I, rows, stride, send.view(np.int32)) + xc.merge_failures(D, I, metric, oD, oI, rows, oR)
    return msgs + ([] if ok else ["written outside a buffer"])


# ---- the regimes are what they say ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,k", xc.MERGE_SHAPES)
def test_lists_are_sorted_and_the_regimes_hold_what_they_name(world, k):
    for metric in xc.METRICS:
        for regime in xc.REGIMES:
            for B in xc.BATCHES:
                D, I = xc.make_lists(regime, world, B, k, metric, seed=B)
                assert xc.lists_sorted(D, I, metric), (regime, metric, B)
                assert (I[I >= 0] % world == np.broadcast_to(np.arange(world)[:, None, None], I.shape)[I >= 0]).all() or regime == "bigid"
        D, I = xc.make_lists("zeros", world, 3, k, metric)
        if world * k >= 16:
            assert (xc.f32_bits(D[I >= 0]) == 0x80000000).any() and (xc.f32_bits(D[I >= 0]) == 0).any()
        totals = set()
        for seed in range(3):
            _, I = xc.make_lists("short", world, 3, k, metric, seed=seed)
            totals |= {int(np.sign((I[:, b] >= 0).sum() - k)) for b in range(3)}
        assert totals == ({-1, 0, 1} if world >= 3 else {-1, 0}), totals        # below, at and above k within one launch of 3
        _, I = xc.make_lists("few", world, 3, k, metric)
        assert ((I >= 0).sum(axis=(0, 2)) == 1).all() and (I[-1, :, 0] >= 0).all()
        _, I = xc.make_lists("bigid", world, 3, k, metric)
        v = I[I >= 0]
        assert (v == 0).any()
        if world * k >= 16:
            assert ((v & 0xFFFFFFFF) >= (1 << 31)).any() and (v >= (1 << 32)).any() and (v >= (1 << 33)).any()
        D, I = xc.make_lists("inf", world, 3, k, metric)
        assert (np.isinf(D) & (I >= 0)).any() and (k == 1 or ((I < 0).any() == (k > 5)))
        if world > 1:
            D, I = xc.make_lists("onesided", world, 2, k, metric)
            _, wI, _ = xc.merged_reference(D, I, metric)
            assert set(wI[0]) <= set(I[0, 0]) and set(wI[1]) <= set(I[-1, 1])


def test_the_shapes_reach_the_kernel_limits():
    """world * k entries of one query in LDS, nvalid[64], src[128]: at the limit, one below in both factors, and a single list / entry"""
    prod = [w * k for w, k in xc.MERGE_SHAPES]
    assert max(prod) == xc.MAX_ENTRIES and prod.count(xc.MAX_ENTRIES) == 2 and xc.MAX_ENTRIES - 63 * 65 == 1
    assert max(w for w, _ in xc.MERGE_SHAPES) == xc.MAX_WORLD and max(k for _, k in xc.MERGE_SHAPES) == xc.MAX_K
    assert (1, 1) in xc.MERGE_SHAPES and max(xc.PARTS) == 64 and max(xc.PARTS_K) > xc.MAX_K
    for B in xc.BATCHES:
        for dim in (0,) + xc.ROW_DIMS:
            assert xc.wide_stride(B, 17, dim) >= xc.dense_stride(B, 17, dim) and (not dim or xc.wide_stride(B, 17, dim) % 4 == 0)


def test_reference_equals_a_python_sort_of_tuples():
    for metric in xc.METRICS:
        for regime in xc.REGIMES:
            D, I = xc.make_lists(regime, 3, 3, 17, metric)
            wD, wI, _ = xc.merged_reference(D, I, metric)
            for b in range(3):
                ent = []
                for s in range(3):
                    for j in range(17):
                        if I[s, b, j] >= 0:
                            d = float(D[s, b, j]) if metric == xc.L2 else -float(D[s, b, j])
                            ent.append((d + 0.0, int(I[s, b, j]), int(xc.f32_bits(D[s, b, j:j + 1])[0])))     # python: -0.0 == 0.0, inf == inf
                ent.sort(key=lambda t: (t[0], t[1]))
                ent = ent[:17]
                assert [t[1] for t in ent] == [int(i) for i in wI[b, :len(ent)]]
                assert [t[2] for t in ent] == [int(x) for x in xc.f32_bits(wD[b, :len(ent)])]
                assert (wI[b, len(ent):] == -1).all() and (wD[b, len(ent):] == xc.filler_of(metric)).all()


# ---- the models pass ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,k", xc.MERGE_SHAPES)
def test_models_of_pack_and_merge_pass_in_every_regime(world, k):
    runs = 0
    for B in xc.BATCHES:
        for ri, regime in enumerate(xc.REGIMES):
            for metric in xc.METRICS:
                D, I = xc.make_lists(regime, world, B, k, metric, seed=B)
                big = world * k > 1024
                # every regime with and without rows; the three row widths and the two strides rotate (all of them on the small shapes)
                dims = (0, xc.ROW_DIMS[(ri + metric) % 3]) if big else (0,) + xc.ROW_DIMS
                for dim in dims:
                    rows = xc.make_rows(world, B, k, dim) if dim else None
                    strides = (xc.dense_stride(B, k, dim), xc.wide_stride(B, k, dim))
                    for stride in (strides[(ri + B) % 2],) if big else strides:
                        msgs = _failures(D, I, rows, stride, metric, _pipeline(D, I, rows, stride, metric))
                        assert not msgs, (regime, metric, B, dim, stride, msgs)
                        runs += 1
    assert runs >= 72


def test_model_of_merge_parts_passes_at_every_table_shape():
    i = 0
    for parts in xc.PARTS:
        for nq in xc.PARTS_NQ:
            for k in xc.PARTS_K:
                regimes = xc.REGIMES if (parts, nq) == (3, 65) else (xc.REGIMES[i % len(xc.REGIMES)],)
                for regime in regimes:
                    for metric in xc.METRICS if len(regimes) > 1 else (xc.METRICS[i % 2],):
                        D, I = xc.make_lists(regime, parts, nq, k, metric, seed=i)
                        wD, oD = _guarded(nq * k, np.float32, SENTF)
                        wI, oI = _guarded(nq * k, np.int64, SENT64)
                        xc.merge_parts_model(D, I, metric, oD.reshape(nq, k), oI.reshape(nq, k))
                        msgs = xc.merge_failures(D, I, metric, oD, oI)
                        assert not msgs and _intact(wD, SENTF) and _intact(wI, SENT64), (parts, nq, k, regime, metric, msgs)
                i += 1


@pytest.mark.parametrize("world,k", xc.MERGE_SHAPES)
def test_three_implementations_one_answer_on_the_cpu(world, k):
    """the exchange pipeline's model, merge_parts' model and merge_partials (the host twin the gloo tests run): the reference's bits.
    The `inf` regime is the test of merge_partials' order on (filler, key, id): keyed on (key, id) with fillers at +inf it lost every
    valid entry whose distance is infinite."""
    B = 3
    for regime in xc.REGIMES:
        for metric in xc.METRICS:
            D, I = xc.make_lists(regime, world, B, k, metric, seed=1)
            wD, wI, _ = xc.merged_reference(D, I, metric)
            hD, hI = merge_partials(torch.from_numpy(D), torch.from_numpy(I), metric)
            assert xc.same_bits(hD.numpy(), wD) and np.array_equal(hI.numpy(), wI), (regime, metric, "merge_partials")
            pD, pI = np.empty((B, k), np.float32), np.empty((B, k), np.int64)
            xc.merge_parts_model(D, I, metric, pD, pI)
            assert xc.same_bits(pD, wD) and np.array_equal(pI, wI), (regime, metric, "merge_parts")
            if world * k <= 1024:
                _, oD, oI, _, _ = _pipeline(D, I, None, xc.dense_stride(B, k, 0), metric)
                assert xc.same_bits(oD.reshape(B, k), wD) and np.array_equal(oI.reshape(B, k), wI), (regime, metric, "exchange")


def test_merge_partials_keeps_valid_infinite_entries():
    """the case of the issue: three lists of one finite entry, four valid infinite ones and three fillers -> eight valid ids"""
    for metric in xc.METRICS:
        D, I = xc.make_lists("inf", 3, 1, 8, metric)
        assert ((I >= 0).sum(axis=2) == 5).all() and (np.isinf(D) & (I >= 0)).sum() == 12
        hD, hI = merge_partials(torch.from_numpy(D), torch.from_numpy(I), metric)
        assert (hI.numpy() >= 0).all() and np.isfinite(hD.numpy()).sum() == 3
        wD, wI, _ = xc.merged_reference(D, I, metric)
        assert xc.same_bits(hD.numpy(), wD) and np.array_equal(hI.numpy(), wI)


def test_gather_reference():
    db = np.arange(40, dtype=np.float32).reshape(10, 4)
    got = xc.gather_reference(db, np.array([0, 9, -1, 9]))
    assert np.array_equal(got, np.stack([db[0], db[9], np.zeros(4, np.float32), db[9]]))
    assert np.array_equal(xc.gather_reference(db, np.array([(1 << 33) + 3, -1]), id_base=1 << 33), np.stack([db[3], np.zeros(4, np.float32)]))


# ---- the mutations fail -----------------------------------------------------------------------------------------------------------------
# the regime that shows a mutation soonest goes first; the rest follow
FIRST = {"ties_larger_id": "ties", "neg_zero_first": "zeros", "fillers_valid": "short", "no_own_position": "random", "drop_high": "bigid",
         "sign_extend_low": "bigid", "no_fillers": "few", "row_neighbour": "random", "drop_last_list": "few", "dense_stride": "random",
         "no_ip_sign": "random", "le_on_key": "ties", "drop_high@pack": "bigid", "pad_unwritten": "random", "dense_stride@pack": "random"}


def _must_change(mutation, world, k):
    """the shapes at which a mutation has something to change (B = 3, rows, the wide stride)"""
    if mutation in ("ties_larger_id", "neg_zero_first", "le_on_key", "row_neighbour", "drop_last_list", "dense_stride", "dense_stride@pack",
                    "no_ip_sign"):
        return world >= 2                                       # an order across lists / another list / a part behind the first
    if mutation == "no_own_position":
        return k >= 2                                           # the first entry's own position is zero
    return True                                                 # fillers and ids: `short`, `few` and `bigid` reach every shape at B = 3


def _regimes_from(first):
    return (first,) + tuple(r for r in xc.REGIMES if r != first)


@pytest.mark.parametrize("world,k", xc.MERGE_SHAPES)
@pytest.mark.parametrize("mutation", xc.MERGE_MUTATIONS + xc.PACK_MUTATIONS)
def test_mutations_of_pack_and_merge_fail_by_bits(mutation, world, k):
    B, dim = 3, 4
    stride = xc.wide_stride(B, k, dim)
    pm, mm = (mutation, None) if mutation in xc.PACK_MUTATIONS else (None, mutation)
    must = _must_change(mutation, world, k)
    changed = caught = False
    for regime in _regimes_from(FIRST[mutation]):
        for metric in (xc.IP, xc.L2) if mutation == "no_ip_sign" else xc.METRICS:
            D, I = xc.make_lists(regime, world, B, k, metric, seed=2)
            rows = xc.make_rows(world, B, k, dim)
            base = _pipeline(D, I, rows, stride, metric)
            mut = _pipeline(D, I, rows, stride, metric, pm, mm)
            differs = any(not np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(base[:4], mut[:4])) or base[4] != mut[4]
            fails = bool(_failures(D, I, rows, stride, metric, mut))
            assert fails == differs, (regime, metric, "a change the check does not see" if differs else "a failure without a change")
            changed, caught = changed or differs, caught or fails
            if caught and must:
                break
        if caught and must:
            break
    assert changed == must and caught == must, (mutation, world, k, changed, caught)


@pytest.mark.parametrize("mutation", xc.PARTS_MUTATIONS)
def test_mutations_of_merge_parts_fail_by_bits(mutation):
    for parts, nq, k in ((1, 3, 1), (2, 63, 16), (3, 65, 128), (64, 64, 16), (63, 1, 200)):
        must = parts >= 2 if mutation in ("ties_larger_id", "neg_zero_first", "drop_last_list", "no_ip_sign") else True
        caught = False
        for regime in _regimes_from(FIRST[mutation]):
            for metric in (xc.IP, xc.L2) if mutation == "no_ip_sign" else xc.METRICS:
                D, I = xc.make_lists(regime, parts, nq, k, metric, seed=3)
                oD, oI = np.full((nq, k), SENTF, np.float32), np.full((nq, k), SENT64, np.int64)
                xc.merge_parts_model(D, I, metric, oD, oI, mutation=mutation)
                caught = caught or bool(xc.merge_failures(D, I, metric, oD, oI))
                if caught:
                    break
            if caught:
                break
        assert caught == must, (mutation, parts, nq, k)


@pytest.mark.parametrize("world,k", xc.MERGE_SHAPES)
def test_le_on_the_pair_is_no_defect(world, k):
    """a binary search with `<=` on the (key, id) pair finds the same place, since no other list holds the entry's id: recorded as an
    equivalent form, as the search bar records count_less; `<=` on the key alone is the mutation le_on_key above"""
    for regime in xc.REGIMES:
        D, I = xc.make_lists(regime, world, 1, k, xc.L2, seed=4)
        run = _pipeline(D, I, None, xc.dense_stride(1, k, 0), xc.L2, None, "le_on_pair")
        assert not _failures(D, I, None, xc.dense_stride(1, k, 0), xc.L2, run), regime


# ---- what the earlier end-to-end assertions let through ---------------------------------------------------------------------------------
LET_THROUGH = ("neg_zero_first", "fillers_valid", "drop_high", "sign_extend_low", "no_fillers", "dense_stride", "no_ip_sign",
               "drop_high@pack", "pad_unwritten", "dense_stride@pack")


def _searched_lists(db, q, world, k):
    """fp32 L2 lists of a row-sharded exact search, each sorted by (distance, id), invalid entries (+inf, -1) at the tail"""
    d = ((q[:, None, :].astype(np.float32) - db[None, :, :]) ** 2).sum(axis=2, dtype=np.float32)
    D = np.full((world, len(q), k), np.inf, np.float32)
    I = np.full((world, len(q), k), -1, np.int64)
    for s in range(world):
        lo, hi = shard_bounds(len(db), world, s)
        for b in range(len(q)):
            o = np.lexsort((np.arange(lo, hi), d[b, lo:hi]))[:k]
            D[s, b, :len(o)], I[s, b, :len(o)] = d[b, lo:hi][o], o + lo
    return D, I, db[np.maximum(I, 0)] * (I >= 0)[..., None]


def test_which_mutations_the_end_to_end_assertions_let_through():
    """test_exchange_pack_merge_kernels_emulate_three_shards in the models' terms: iid rows 3,000 x 128 with one duplicate pair across
    shards, k = 16, three shards, L2, the dense stride in a zero-filled message; then 40 rows over two shards (a list with fillers, more
    than k valid entries in all).  It asserts (D, I, rows) against a search of the whole.  Ten of the fifteen mutations pass it."""
    rs = np.random.RandomState(21)
    db = rs.standard_normal((3000, 128)).astype(np.float32)
    db /= np.linalg.norm(db, axis=1, keepdims=True)
    db[1500] = db[7]
    q = rs.standard_normal((15, 128)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[0] = db[7]
    cases = [_searched_lists(db, q, 3, 16), _searched_lists(db[:40], q[:5], 2, 16)]
    passed = []
    for mutation in xc.MERGE_MUTATIONS + xc.PACK_MUTATIONS:
        pm, mm = (mutation, None) if mutation in xc.PACK_MUTATIONS else (None, mutation)
        ok = True
        for D, I, rows in cases:
            B, k = D.shape[1:]
            run = _pipeline(D, I, rows, xc.dense_stride(B, k, 128), xc.L2, pm, mm, zero_send=True)
            ok = ok and not xc.merge_failures(D, I, xc.L2, run[1], run[2], rows, run[3])
        if ok:
            passed.append(mutation)
    print("let through by the end-to-end assertions:", passed)
    assert tuple(passed) == LET_THROUGH
