"""References, regimes and checks of the merge end of a row-sharded search (keds_amd/csrc/search.hip: exchange_pack_kernel,
exchange_merge_kernel, merge_parts_kernel, gather_rows_kernel; their host twin keds_amd.index.merge_partials).  Plain numpy, no GPU.

tests/test_host_exchange_check.py shows that line-by-line integer models of the kernels pass these checks and that mutations of them
fail; tests/test_gpu_exchange_kernels_edges.py holds the kernels to them.

Everything here is integer work and compared by bits; there is no tolerance anywhere.  The reference of a merge: of a query's `world`
lists take every entry with id >= 0, order them by (key, id) -- key = D for L2, -D for IP, -0 folded into +0 -- keep k, then fillers
(+inf for L2, -inf for IP, id -1).  A merged entry keeps the distance bits it arrived with (a -0 stays a -0), its id as int64 and, with
rows, its row by bits; a filler's row is zero.

Lists are built directly, not by searching: each sorted by (key, id) with its invalid entries (id -1) at the tail, ids unique across
shards (shard s holds the ids = s mod world; `bigid` adds offsets around 2^31, 2^32 and 2^33).  An invalid entry carries either the
filler distance of its metric or a finite distance that would WIN if it were counted (key -7), so that counting one shows.
"""
import numpy as np

from keds_amd import _lib

L2, IP = _lib.METRIC_L2, _lib.METRIC_IP
METRICS = (L2, IP)
MAX_ENTRIES, MAX_WORLD, MAX_K = 4096, 64, 128                   # exchange_merge_kernel: world * k entries in LDS, nvalid[64], src[MAX_K]
REGIMES = ("random", "ties", "equal", "zeros", "short", "few", "onesided", "bigid", "inf")
BIG_OFFSETS = (0, (1 << 31) - 3, (1 << 32) - 2, 1 << 33)
SENT32 = 0x5EA5C0DE

# (world, k) of keds_exchange_merge / keds_exchange_pack: one list of one entry; one list at the largest k; a full 64 x 64 and 32 x 128
# (both 4,096 entries, the LDS limit); 63 x 65 just under it with neither a power of two; small odd ones
MERGE_SHAPES = ((1, 1), (1, 128), (2, 16), (3, 17), (5, 1), (63, 65), (64, 64), (32, 128))
BATCHES = (1, 3)
ROW_DIMS = (4, 128, 260)
# keds_topk_merge_parts: one thread per query, 64 per workgroup; pos[64]
PARTS, PARTS_NQ, PARTS_K = (1, 2, 3, 63, 64), (1, 63, 64, 65), (1, 16, 128, 200)


def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(f32_bits(a), f32_bits(b))


def ordered_key(v):
    """ordered_key() of search.hip on fp32 values: unsigned order == float order, -0 folded into +0 (as uint64 values)"""
    u = f32_bits(np.asarray(v, np.float32) + np.float32(0.0)).astype(np.uint64)
    return np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)


def merge_key(D, metric):
    return ordered_key(np.asarray(D, np.float32) if metric == L2 else -np.asarray(D, np.float32))


def filler_of(metric):
    return np.float32(np.inf if metric == L2 else -np.inf)


def dense_stride(B, k, dim):
    """int32 words of one part: E = 3 (distance bits | id low | id high) or, with rows, 4 + dim (... | pad | the row)"""
    return B * k * (dim + 4 if dim else 3)


def wide_stride(B, k, dim):
    return 2 * dense_stride(B, k, dim) + 4


# ---- lists ------------------------------------------------------------------------------------------------------------------------------
def make_lists(regime, world, B, k, metric, seed=0):
    """-> (D f32 [world, B, k], I int64 [world, B, k]): list [s, b] = what shard s found for query b"""
    rs = np.random.RandomState(seed * 7919 + world * 131 + k * 17 + B + REGIMES.index(regime) * 1009 + metric)
    n = world * k
    s_of = np.arange(world)[:, None, None]
    q_of = np.arange(B)[None, :, None]
    j_of = np.arange(k)[None, None, :]
    m = np.argsort(rs.rand(world, B, 2 * k + 2), axis=2)[:, :, :k].astype(np.int64)      # distinct within a list
    ids = s_of + world * m
    nvalid = np.full((world, B), k, np.int64)
    tie_set = np.array([0.0, 1.0, 2.0] if metric == L2 else [-1.0, 0.0, 1.0], np.float32)

    def distinct():
        perm = np.stack([rs.permutation(2 * n) for _ in range(B)])[:, :n].reshape(B, world, k).transpose(1, 0, 2)
        v = ((perm + 0.5) * (4.0 / (2 * n))).astype(np.float32)                            # [0, 4), all different in fp32
        return v if metric == L2 else v - np.float32(2.0)                                  # IP: both signs

    if regime == "random":
        key = distinct()
    elif regime in ("ties", "bigid"):
        key = tie_set[rs.randint(0, 3, (world, B, k))]
    elif regime == "equal":
        key = np.full((world, B, k), 1.0, np.float32)
    elif regime == "zeros":
        key = np.where(rs.randint(0, 2, (world, B, k)) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    elif regime == "short":
        cyc = np.array([0, 1, max(k - 1, 0), k])
        nvalid = np.zeros((world, B), np.int64)
        for b in range(B):
            which = (b + seed) % 3
            if which == 0:                                       # every count of the cycle, the first list full: k (world 1) or more
                nvalid[:, b] = cyc[(np.arange(world) + 3) % 4]
            elif which == 1:                                     # exactly k over two lists (k - 1 + 1), or k - 1 in one
                nvalid[0, b] = k - 1
                if world > 1:
                    nvalid[-1, b] = 1
            else:                                                # below k: one entry in every second list, at most k - 1 in all
                nvalid[::2, b] = 1
                nvalid[:, b] = np.where(np.cumsum(nvalid[:, b]) <= max(k - 1, 0), nvalid[:, b], 0)
        key = np.where(rs.randint(0, 2, (world, B, k)) == 1, tie_set[rs.randint(0, 3, (world, B, k))], distinct())
    elif regime == "few":
        nvalid = np.zeros((world, B), np.int64)
        nvalid[-1] = 1
        key = distinct()
    elif regime == "onesided":
        key = distinct() * np.float32(0.25) + np.float32(2.0)                              # [1.5, 3)
        for b in range(B):
            key[0 if (b + seed) % 2 == 0 else -1, b] -= np.float32(4.0)                    # below every other list
    elif regime == "inf":
        n_fin = np.where((k > 1) | (np.arange(world) % 2 == 1), 1, 0)[:, None, None]   # k = 1: every second list is one infinite entry
        n_inf = np.minimum(k - n_fin, 4)
        nvalid = np.broadcast_to((n_fin + n_inf)[:, :, 0], (world, B)).copy()
        key = np.where(j_of < n_fin, distinct(), np.float32(np.inf)).astype(np.float32)
    else:
        raise ValueError(regime)
    if regime == "bigid":                                        # three queries in a row hold every kind of id at every place of a list
        turn = (s_of + q_of + j_of + seed) % 3                   # 0: small ids; 1: the low word's top bit; 2: a high word
        high = np.where((s_of + j_of) % 2 == 0, BIG_OFFSETS[2], BIG_OFFSETS[3])
        ids = np.where(turn == 0, ids + world, ids + 3 * world + np.where(turn == 1, BIG_OFFSETS[1], high))   # + 3 world: 2^31 - 3 + id >= 2^31
        ids[0, :, 0] = np.where(turn[0, :, 0] == 0, 0, ids[0, :, 0])                      # id 0 itself (shard 0 holds the ids = 0 mod world)
    key = np.ascontiguousarray(key, np.float32)
    valid = j_of < nvalid[:, :, None]
    D = key if metric == L2 else -key                            # -(+0) = -0: the IP lists of `zeros` are mixed as well
    o = np.lexsort((ids, ordered_key(key), ~valid), axis=2)      # valid first, each list by (key, id)
    D, ids, valid = (np.take_along_axis(a, o, axis=2) for a in (D, ids, valid))
    winning = np.float32(-7.0) if metric == L2 else np.float32(7.0)
    production = regime == "inf" or ((s_of + q_of) % 2 == 1)
    junk = np.where(production, filler_of(metric), winning).astype(np.float32)
    D = np.where(valid, D, junk).astype(np.float32)
    I = np.where(valid, ids, -1).astype(np.int64)
    return np.ascontiguousarray(D), np.ascontiguousarray(I)


def make_rows(world, B, k, dim, seed=0):
    """fp32 rows [world, B, k, dim] with every bit pattern class among them: finite, -0, inf, NaN payloads travel as words"""
    rs = np.random.RandomState(seed + world * 3 + k * 5 + dim)
    r = rs.standard_normal((world, B, k, dim)).astype(np.float32)
    w = r.view(np.uint32)
    w[..., 0] = (np.arange(world)[:, None, None] << 20) | (np.arange(B)[None, :, None] << 12) | np.arange(k)[None, None, :]   # who am I
    if dim > 1:
        w[..., 1] = 0x80000000
        w[..., dim - 1] = 0x7FC00001 + np.arange(k, dtype=np.uint32)[None, None, :]
    return r


def lists_sorted(D, I, metric):
    """what the merges take for granted: every list sorted by (key, id), invalid entries at the tail, ids unique per query"""
    valid = I >= 0
    if (valid[..., 1:] & ~valid[..., :-1]).any():
        return False
    key = merge_key(D, metric)
    a_k, b_k, a_i, b_i = key[..., :-1], key[..., 1:], I[..., :-1], I[..., 1:]
    both = valid[..., 1:]
    if (both & ~((a_k < b_k) | ((a_k == b_k) & (a_i < b_i)))).any():
        return False
    for b in range(I.shape[1]):
        v = I[:, b][I[:, b] >= 0]
        if len(np.unique(v)) != len(v):
            return False
    return True


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
def merged_reference(D, I, metric, rows=None):
    """-> (D [B, k] f32, I [B, k] int64, rows [B, k, dim] or None): a plain sort of the valid entries by (key, id)"""
    world, B, k = D.shape
    oD = np.full((B, k), filler_of(metric), np.float32)
    oI = np.full((B, k), -1, np.int64)
    oR = None if rows is None else np.zeros((B, k, rows.shape[3]), np.float32)
    key = merge_key(D, metric)
    for b in range(B):
        s, j = np.nonzero(I[:, b, :] >= 0)
        o = np.lexsort((I[s, b, j], key[s, b, j]))[:k]
        oD[b, :len(o)], oI[b, :len(o)] = D[s[o], b, j[o]], I[s[o], b, j[o]]
        if rows is not None:
            oR[b, :len(o)] = rows[s[o], b, j[o]]
    return oD, oI, oR


def message_reference(D, I, rows, w_stride, fill=SENT32):
    """the int32 words keds_exchange_pack must leave in a `fill`-filled send buffer -> int32 [world, w_stride]"""
    world, B, k = D.shape
    E = 3 if rows is None else rows.shape[3] + 4
    body = np.zeros((world, B, k, E), np.uint32)
    body[..., 0] = f32_bits(D)
    body[..., 1] = (I & 0xFFFFFFFF).astype(np.uint32)
    body[..., 2] = ((I >> 32) & 0xFFFFFFFF).astype(np.uint32)
    if rows is not None:
        body[..., 4:] = f32_bits(rows)                           # word 3: the pad, zero
    out = np.full((world, w_stride), fill, np.uint32)
    out[:, :B * k * E] = body.reshape(world, -1)
    return out.view(np.int32)


def merge_failures(D, I, metric, gotD, gotI, rows=None, gotR=None, what=""):
    wD, wI, wR = merged_reference(D, I, metric, rows)
    msgs = []
    gotD, gotI = np.asarray(gotD).reshape(wD.shape), np.asarray(gotI).reshape(wI.shape)
    if not same_bits(gotD, wD):
        bad = np.argwhere(f32_bits(gotD) != f32_bits(wD))
        msgs.append(f"{what}D differs from the sort by (key, id) at {len(bad)} places, first (query, rank) {tuple(bad[0])}")
    if not np.array_equal(gotI.astype(np.int64), wI):
        bad = np.argwhere(gotI != wI)
        msgs.append(f"{what}I differs at {len(bad)} places, first (query, rank) {tuple(bad[0])}: {gotI[tuple(bad[0])]} for {wI[tuple(bad[0])]}")
    if rows is not None:
        gotR = np.asarray(gotR).reshape(wR.shape)
        if not same_bits(gotR, wR):
            bad = np.argwhere((f32_bits(gotR) != f32_bits(wR)).any(axis=2))
            msgs.append(f"{what}the winners' rows differ at {len(bad)} places, first (query, rank) {tuple(bad[0])}")
    return msgs


def pack_failures(D, I, rows, w_stride, got, what=""):
    want = message_reference(D, I, rows, w_stride)
    got = np.asarray(got).reshape(want.shape)
    if np.array_equal(got, want):
        return []
    bad = np.argwhere(got != want)
    E = 3 if rows is None else rows.shape[3] + 4
    s, o = bad[0]
    where = f"word {o % E} of entry {o // E}" if o < dense_stride(D.shape[1], D.shape[2], 0 if rows is None else rows.shape[3]) else "the gap"
    return [f"{what}the message differs in {len(bad)} words, first part {s} {where}"]


def gather_reference(db, idx, id_base=0):
    idx = np.asarray(idx, np.int64)
    return np.where((idx >= 0)[:, None], db[np.maximum(idx - id_base, 0)], np.float32(0.0)).astype(np.float32)


# ---- line-by-line models of the kernels -------------------------------------------------------------------------------------------------
PACK_MUTATIONS = ("drop_high@pack", "pad_unwritten", "dense_stride@pack")
MERGE_MUTATIONS = ("ties_larger_id", "neg_zero_first", "fillers_valid", "no_own_position", "drop_high", "sign_extend_low", "no_fillers",
                   "row_neighbour", "drop_last_list", "dense_stride", "no_ip_sign", "le_on_key")
PARTS_MUTATIONS = ("ties_larger_id", "neg_zero_first", "fillers_valid", "no_fillers", "drop_last_list", "no_ip_sign")
EQUIVALENT = ("le_on_pair",)                                     # ids are unique, so `<=` on the (key, id) pair finds the same place


def pack_model(D, I, rows, w_stride, send, mutation=None):
    """exchange_pack_kernel on a flat int32 `send` (modified in place): D, I [world, B, k], rows [world, B, k, dim] or None"""
    world, B, k = D.shape
    dim = 0 if rows is None else rows.shape[3]
    E = dim + 4 if dim else 3
    stride = B * k * E if mutation == "dense_stride@pack" else w_stride
    u = send.view(np.uint32)
    for lst in range(world * B):
        w, b = divmod(lst, B)
        dst = w * stride + b * k * E
        at = dst + np.arange(k) * E
        ids = I[w, b]
        u[at + 0] = f32_bits(D[w, b])
        u[at + 1] = (ids & 0xFFFFFFFF).astype(np.uint32)
        u[at + 2] = 0 if mutation == "drop_high@pack" else ((ids >> 32) & 0xFFFFFFFF).astype(np.uint32)
        if dim:
            u[(at + 4)[:, None] + np.arange(dim)[None, :]] = f32_bits(rows[w, b])
            if mutation != "pad_unwritten":
                u[at + 3] = 0
    return send


def _ordered_key_words(d, metric, mutation):
    kf = d if (metric == L2 or mutation == "no_ip_sign") else -d
    if mutation == "neg_zero_first":
        u = f32_bits(kf).astype(np.uint64)
    else:
        u = f32_bits(kf + np.float32(0.0)).astype(np.uint64)
    return np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)


def exchange_merge_model(recv, world, B, k, dim, w_stride, metric, D, I, R, mutation=None):
    """exchange_merge_kernel on flat buffers (outputs written in place, what the kernel does not write is left alone): the loads, the
    per-list valid counts, the rank = own position + one binary search per other list, the scatter, the fillers, the rows"""
    E = dim + 4 if dim else 3
    stride = B * k * E if mutation == "dense_stride" else w_stride
    lists = world - 1 if (mutation == "drop_last_list" and world > 1) else world
    n = lists * k
    e = np.arange(n)
    w_e, j_e = e // k, e % k
    words = recv.view(np.uint32)
    Du = D.view(np.uint32)
    Ru = None if R is None else R.view(np.uint32)
    for b in range(B):
        p = w_e * stride + (b * k + j_e) * E
        dbits = words[p]
        lo_w, hi_w = words[p + 1].astype(np.int64), words[p + 2].view(np.int32).astype(np.int64)
        if mutation == "drop_high":
            ids = lo_w
        elif mutation == "sign_extend_low":
            ids = (hi_w << 32) | words[p + 1].view(np.int32).astype(np.int64)
        else:
            ids = (hi_w << 32) | lo_w
        keys = _ordered_key_words(dbits.view(np.float32), metric, mutation)
        valid = np.ones(n, bool) if mutation == "fillers_valid" else ids >= 0
        nvalid = np.bincount(w_e[valid], minlength=lists)
        live = j_e < nvalid[w_e]
        rank = np.zeros(n, np.int64) if mutation == "no_own_position" else j_e.astype(np.int64).copy()
        keys2, ids2, oi = keys.reshape(lists, k), ids.reshape(lists, k), np.arange(lists)[None, :]
        lo, hi = np.zeros((n, lists), np.int64), np.broadcast_to(nvalid[None, :], (n, lists)).astype(np.int64)
        act = live[:, None] & (w_e[:, None] != oi)               # one binary search per OTHER list, all of them in step
        key_e, id_e = keys[:, None], ids[:, None]
        while True:
            go = act & (lo < hi)
            if not go.any():
                break
            mid = (lo + hi) >> 1
            at = np.minimum(mid, k - 1)
            km, im = keys2[oi, at], ids2[oi, at]
            if mutation == "ties_larger_id":
                less = (km < key_e) | ((km == key_e) & (im > id_e))
            elif mutation == "le_on_key":
                less = km <= key_e
            elif mutation == "le_on_pair":
                less = (km < key_e) | ((km == key_e) & (im <= id_e))
            else:
                less = (km < key_e) | ((km == key_e) & (im < id_e))
            lo = np.where(go & less, mid + 1, lo)
            hi = np.where(go & ~less, mid, hi)
        rank += np.where(act, lo, 0).sum(axis=1)
        src = np.full(k, -1, np.int64)
        for x in np.nonzero(live & (rank < k))[0]:              # colliding ranks (a mutation's): the later entry wins the slot
            Du[b * k + rank[x]] = dbits[x]
            I[b * k + rank[x]] = ids[x]
            src[rank[x]] = x
        total = int(nvalid.sum())
        if mutation != "no_fillers":
            D[b * k + total:(b + 1) * k] = filler_of(metric)
            I[b * k + total:(b + 1) * k] = -1
        if Ru is not None:
            for r in range(k):
                x = src[r]
                if x < 0:
                    Ru[(b * k + r) * dim:(b * k + r + 1) * dim] = 0
                    continue
                w = w_e[x] if mutation != "row_neighbour" else (w_e[x] + 1) % world
                at = w * stride + (b * k + j_e[x]) * E + 4
                Ru[(b * k + r) * dim:(b * k + r + 1) * dim] = words[at:at + dim]


def merge_parts_model(Dp, Ip, metric, D, I, mutation=None):
    """merge_parts_kernel: k selection steps over the heads of the lists, fp32 comparisons (so -0 == +0 by itself); outputs in place"""
    parts, nq, k = Dp.shape
    lists = parts - 1 if (mutation == "drop_last_list" and parts > 1) else parts
    neg = metric != L2 and mutation != "no_ip_sign"
    key = (-Dp if neg else Dp)[:lists]                           # [lists, nq, k]
    cmp_key = _ordered_key_words(key, L2, "neg_zero_first").astype(np.int64) if mutation == "neg_zero_first" else key
    ids = Ip[:lists]
    q = np.arange(nq)
    pos = np.zeros((lists, nq), np.int64)
    for r in range(k):
        head = np.minimum(pos, k - 1)
        hk = np.take_along_axis(cmp_key, head[:, :, None], axis=2)[:, :, 0]
        hi = np.take_along_axis(ids, head[:, :, None], axis=2)[:, :, 0]
        ok = pos < k
        if mutation != "fillers_valid":
            ok &= hi >= 0
        bp = np.full(nq, -1, np.int64)
        bk = np.zeros(nq, cmp_key.dtype)
        bi = np.zeros(nq, np.int64)
        for p in range(lists):
            tie = (hi[p] > bi) if mutation == "ties_larger_id" else (hi[p] < bi)
            take = ok[p] & ((bp < 0) | (hk[p] < bk) | ((hk[p] == bk) & tie))
            bp, bk, bi = np.where(take, p, bp), np.where(take, hk[p], bk), np.where(take, hi[p], bi)
        none = bp < 0
        sel = np.maximum(bp, 0)
        kept = key[sel, q, np.minimum(pos[sel, q], k - 1)]       # the kernel stores bk (the key) back with its sign undone
        out = np.where(none, filler_of(metric), -kept if neg else kept).astype(np.float32)
        if mutation == "no_fillers":
            D[~none, r], I[~none, r] = out[~none], bi[~none]
        else:
            D[:, r], I[:, r] = out, np.where(none, -1, bi)
        pos[sel[~none], q[~none]] += 1
