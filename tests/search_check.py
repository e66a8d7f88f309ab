"""References and checks of the search kernels (keds_amd/csrc/search.hip), one stage at a time.  Plain numpy float64, no GPU.

tests/test_host_search_check.py shows that CPU models of the stages pass these checks and that mutations of them fail;
tests/test_gpu_search_kernels_edges.py holds the kernels to them through the stage entries (keds_search_*).

Bounds, with u = 2^-24 (none is tuned on a kernel):
  pack    key bytes = bf16(x) to the bit at swz_chunk positions; pad rows zero keys, bias -inf; L2 bias within (D/64 + 8) u * 0.5||x||^2 of
          -0.5||x||^2 (a lane adds D/64 squares, the butterfly 6 more, the square and the halving round once each), IP bias 0; each
          DbBounds entry >= its float64 maximum and <= it * (1 + 1e-6 + (D/64 + 8) u).
  qprep   qn = q to the bit, or within 3u |q/||q||| per element (the norm's sum and root, the division); qb = bf16(stored qn) to the bit;
          qstat[1], [2] >= float64 ||qn - qb||, ||qb|| and within 1e-6 + (dim/64 + 8) u above; qstat[0] within (dim/64 + 8) u.
  scan    s = q~.x~ + bias in float64 on the stored operands; |score - s| <= e = 2 (D + 16) u (|q~|.|x~| + |bias|).
  rerank  L2: (4 ceil(dim/256) + 9) u sum (q - x)^2 (the subtraction twice through the square, the square, a lane's 4 ceil(dim/256)
          additions, 6 butterfly steps); IP: (4 ceil(dim/256) + 7) u sum |q||x|.
  certify eps(q) = (||q - q~|| xt + ||q~|| r + ||q - q~|| r + 2e-4 ||q~|| xt + bias_err) 1.01 + 1e-6 (|t_k| + ||q||^2 + 1), bias_err =
          (3 dim/64 + 8) u 0.5 max||x||^2 for L2 (see bias_err below); verdict margin m = t_k - eps - sbound in float64 from the stored inputs; decided outside |m| <= delta = 8u (|t_k| + eps + |sbound|)
          (the kernel evaluates eight fp32 operations on these magnitudes).
Everything else (lists, cuts, ties, ranks, fillers, counters) is integer work and compared by bits.
"""
import numpy as np

from keds_amd import _lib

U = 2.0 ** -24
STAGE_KEYS, QBLOCK, LISTK = 32, 128, 16
DIMS = (128, 256, 512, 768, 1024)
L2, IP = _lib.METRIC_L2, _lib.METRIC_IP
NEG_INF_KEY = 0x007FFFFF                    # ord_key(-inf)
PLAN_FIELDS = ("two_phase", "stagesA", "nqb", "nwgA", "nwgB", "depthA", "ncand", "chunk_rows", "nchunks", "total_stages")
EXACT_BUDGET = 256 << 20


def ring_depth(dim):
    """stages of the scan's LDS ring: 8, 8, 4, 3, 2 for dim 128 ... 1024"""
    return min(8, (160 * 1024) // (STAGE_KEYS * dim * 2 + 8 * 128))


# ---- number formats ---------------------------------------------------------------------------------------------------------------
def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def bits_f32(b):
    return np.ascontiguousarray(b, dtype=np.uint32).view(np.float32)


def bf16_bits(x):
    """round-to-nearest-even bf16 of finite fp32 values, as uint16"""
    b = f32_bits(x).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_f32(bits16):
    return (np.asarray(bits16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_f32(bf16_bits(x))


def ord_key(f):
    """order-preserving uint32 image of an fp32 score (as uint64 values): a > b <=> ord_key(a) > ord_key(b); -0 < +0"""
    b = f32_bits(f).astype(np.uint64)
    return np.where(b & 0x80000000, (~b) & 0xFFFFFFFF, b | 0x80000000)


def key_float(k):
    k = np.asarray(k, dtype=np.uint64)
    return bits_f32(np.where(k & 0x80000000, k & 0x7FFFFFFF, (~k) & 0xFFFFFFFF).astype(np.uint32))


def same_bits(a, b):
    return np.array_equal(f32_bits(a), f32_bits(b))


# ---- the packed image -------------------------------------------------------------------------------------------------------------
def stage_bytes(dim):
    return STAGE_KEYS * dim * 2 + 128


def packed_bytes(n, dim):
    return ((n + STAGE_KEYS - 1) // STAGE_KEYS) * stage_bytes(dim) + 128


def swz_chunk(ch, row, mask15=True):
    return (ch & ~15) | ((ch ^ row) & 15) if mask15 else (ch & ~15) | (ch ^ row)


def decode_image(img, n, dim):
    """img: uint8 array of packed_bytes(n, dim) -> dict(keys uint16 [S*32, dim] bf16 bits, bias f32 [S*32], bounds f32 [4] = xt, r, x, pad,
    trailer uint8 [128])"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    S = (n + STAGE_KEYS - 1) // STAGE_KEYS
    sb, chunks = stage_bytes(dim), dim // 8
    assert img.size == S * sb + 128, "image size"
    body = img[:S * sb].reshape(S, sb)
    raw = body[:, :STAGE_KEYS * dim * 2].copy().view(np.uint16).reshape(S, STAGE_KEYS, chunks, 8)
    row = np.arange(STAGE_KEYS)[:, None]
    ch = np.arange(chunks)[None, :]
    keys = raw[:, row, swz_chunk(ch, row), :].reshape(S * STAGE_KEYS, dim)
    bias = body[:, STAGE_KEYS * dim * 2:].copy().view(np.float32).reshape(S * STAGE_KEYS)
    trailer = img[S * sb:].copy()
    return dict(keys=keys, bias=bias, bounds=trailer[:16].view(np.float32).copy(), trailer=trailer, stages=S)


def chain_len(dim):
    return dim / 64 + 8


def pack_failures(x, metric, img, what=""):
    """x: fp32 rows [n, dim] as given to the pack -> (messages, worst ratio to a bound)"""
    n, dim = x.shape
    d = decode_image(img, n, dim)
    msgs, worst = [], 0.0
    want = bf16_bits(x)
    if not np.array_equal(d["keys"][:n], want):
        msgs.append(f"{what}key bytes differ from bf16(x) in {int((d['keys'][:n] != want).any(1).sum())} rows")
    if d["keys"][n:].any():
        msgs.append(f"{what}pad rows hold nonzero keys")
    if not (np.isneginf(d["bias"][n:])).all():
        msgs.append(f"{what}pad rows' bias is not -inf")
    x64 = x.astype(np.float64)
    sq = (x64 ** 2).sum(1)
    if metric == L2:
        err = np.abs(d["bias"][:n].astype(np.float64) + 0.5 * sq)
        bound = chain_len(dim) * U * 0.5 * sq
        ratio = float((err / np.maximum(bound, 1e-300)).max()) if n else 0.0
        ratio = 0.0 if (err == 0).all() else ratio
        worst = max(worst, ratio)
        if ratio > 1.0:
            msgs.append(f"{what}bias off by {ratio:.3g} x the bound")
    elif (f32_bits(d["bias"][:n]) != 0).any():
        msgs.append(f"{what}IP bias is not +0")
    xt = bf16_f32(want).astype(np.float64)
    maxima = (np.sqrt((xt ** 2).sum(1)).max(), np.sqrt(((x64 - xt) ** 2).sum(1)).max(), np.sqrt(sq).max())
    slack = 1e-6 + chain_len(dim) * U
    for name, got, m in zip(("xt", "r", "x"), d["bounds"][:3].astype(np.float64), maxima):
        if got < m:
            msgs.append(f"{what}bound {name} = {got!r} below the float64 maximum {m!r}")
        elif got > m * (1 + slack):
            msgs.append(f"{what}bound {name} = {got!r} above {m!r} (1 + {slack:.3g})")
        if m > 0:
            worst = max(worst, (got / m - 1) / slack)
    if d["bounds"][3] != 0 or d["trailer"][16:].any():
        msgs.append(f"{what}trailer bytes behind the three bounds are not zero")
    return msgs, worst


# ---- qprep ------------------------------------------------------------------------------------------------------------------------
def qprep_failures(q, normalize, qn, qb_bits, qstat, what=""):
    """q fp32 [nq, dim]; qn fp32 [nq, dim]; qb_bits uint16 [ceil(nq/128)*128, dim]; qstat fp32 [nq, 4]"""
    nq, dim = q.shape
    msgs, worst = [], 0.0
    if not normalize:
        if not same_bits(qn, q):
            msgs.append(f"{what}qn differs from q")
    else:
        q64 = q.astype(np.float64)
        ref = q64 / np.sqrt((q64 ** 2).sum(1, keepdims=True))
        err = np.abs(qn.astype(np.float64) - ref)
        bound = 3 * U * np.abs(ref)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = float(np.nanmax(np.where(err == 0, 0.0, err / bound)))
        worst = max(worst, ratio)
        if not ratio <= 1.0:
            msgs.append(f"{what}normalised qn off by {ratio:.3g} x 3u")
    if not np.array_equal(qb_bits[:nq], bf16_bits(qn)):
        msgs.append(f"{what}qb is not bf16 of the stored qn")
    if qb_bits[nq:].any():
        msgs.append(f"{what}rows >= nq of the bf16 block are not +0")
    qn64, qb64 = qn.astype(np.float64), bf16_f32(qb_bits[:nq]).astype(np.float64)
    slack = 1e-6 + chain_len(dim) * U
    for col, name, ref in ((1, "||qn - qb||", np.sqrt(((qn64 - qb64) ** 2).sum(1))), (2, "||qb||", np.sqrt((qb64 ** 2).sum(1)))):
        got = qstat[:, col].astype(np.float64)
        if (got < ref).any():
            msgs.append(f"{what}qstat[{col}] below {name} in {int((got < ref).sum())} rows")
        if (got > ref * (1 + slack)).any():
            msgs.append(f"{what}qstat[{col}] above {name} (1 + {slack:.3g})")
        pos = ref > 0
        if pos.any():
            worst = max(worst, float(((got[pos] / ref[pos] - 1) / slack).max()))
    s = (qn64 ** 2).sum(1)
    err = np.abs(qstat[:, 0].astype(np.float64) - s)
    ratio = float((err / np.maximum(chain_len(dim) * U * s, 1e-300)).max()) if (err > 0).any() else 0.0
    worst = max(worst, ratio)
    if ratio > 1.0:
        msgs.append(f"{what}qstat[0] off by {ratio:.3g} x the bound")
    if (f32_bits(qstat[:, 3]) != 0).any():
        msgs.append(f"{what}qstat[3] is not +0")
    return msgs, worst


# ---- scan -------------------------------------------------------------------------------------------------------------------------
def wg_ranges(stages, nwg):
    """stage range [s0, s1) of every scan workgroup"""
    w = np.arange(nwg + 1, dtype=np.int64)
    b = (w * stages) // nwg
    return b[:-1], b[1:]


def scan_scores64(keys_bits, bias, qb_bits):
    """(s [nq, nkeys] float64 = q~.x~ + bias, e [nq, nkeys] the error bound) from the stored operands"""
    x = bf16_f32(keys_bits).astype(np.float64)
    q = bf16_f32(qb_bits).astype(np.float64)
    dim = x.shape[1]
    b = bias.astype(np.float64)
    with np.errstate(invalid="ignore"):
        s = q @ x.T + b[None, :]
        e = 2 * (dim + 16) * U * (np.abs(q) @ np.abs(x).T + np.abs(b)[None, :])
    return s, e


def scan_scores_model(keys_bits, bias, qb_bits, order="forward", bias_shift=0, swz_mask=True):
    """fp32 scores as the MFMA chain gives them: C-in = bias, one 32-wide step at a time (the step's dot product exact, the addition
    rounded to nearest).  Mutations: bias_shift = 1 takes the bias of the next row; swz_mask = False reads the chunks a swizzle
    without `& 15` would address (for rows >= 16 a chunk of the NEXT rows' bytes)."""
    x = bf16_f32(keys_bits).astype(np.float64)
    q = bf16_f32(qb_bits).astype(np.float64)
    nk, dim = x.shape
    if not swz_mask:                                              # chunk ch of row r is read from slot (ch ^ r) instead of (ch ^ r) & 15
        raw = np.zeros((nk // STAGE_KEYS, STAGE_KEYS * dim + 16 * 8 * STAGE_KEYS), np.float64)      # the stage as stored, + what lies behind
        chunks = dim // 8
        r = np.arange(STAGE_KEYS)[:, None]
        c = np.arange(chunks)[None, :]
        xs = x.reshape(-1, STAGE_KEYS, chunks, 8)
        dst = (r * chunks + swz_chunk(c, r)) * 8
        src = (r * chunks + swz_chunk(c, r, mask15=False)) * 8
        for e8 in range(8):
            raw[:, (dst + e8).ravel()] = xs[:, :, :, e8].reshape(len(raw), -1)
        x = np.stack([raw[:, (src + e8).ravel()] for e8 in range(8)], -1).reshape(-1, STAGE_KEYS, chunks, 8).reshape(nk, dim)
    b = np.roll(bias, -bias_shift) if bias_shift else bias
    acc = np.broadcast_to(b.astype(np.float32)[None, :], (q.shape[0], nk)).copy()
    steps = range(dim // 32) if order == "forward" else range(dim // 32 - 1, -1, -1)
    with np.errstate(invalid="ignore"):
        for s in steps:
            acc = (acc.astype(np.float64) + q[:, 32 * s:32 * s + 32] @ x[:, 32 * s:32 * s + 32].T).astype(np.float32)
    return acc


def scan_lists_model(scores, n, stages, nwg, depth, thr, sentinel, mutation=None, ring=None):
    """The list logic of scan_topk_kernel on given fp32 scores [nq_pad, >= stages*32]: every lane (query, workgroup, key quarter g)
    walks its keys in order and inserts.  -> (pairs uint64 [nq_pad, nwg, 4*depth], meta uint32 [nq_pad, nwg, 2]).
    Mutations: tie_displaces, lmin_stale, short5, thr_ge, pad_listed, metay_unfilled, metay_missing, quarters_reversed, ring_early."""
    nq = scores.shape[0]
    L = depth
    s0, s1 = wg_ranges(stages, nwg)
    thr0 = np.full(nq, -np.inf, np.float32) if thr is None else thr.astype(np.float32)
    lv = np.full((nq, nwg, 4, L), -np.inf, np.float32)
    li = np.full((nq, nwg, 4, L), -1, np.int64)
    lmin = np.broadcast_to(thr0[:, None, None], (nq, nwg, 4)).copy()
    span = int((s1 - s0).max())
    g = np.arange(4)
    sc_all = scores
    if mutation == "pad_listed":
        sc_all = scores.copy()
        sc_all[:, n:] = np.float32(3.0e38)                        # a pad key's -inf bias ignored
    for t in range(span):
        live = (s0 + t < s1)                                      # [nwg]
        st = np.minimum(s0 + t, stages - 1)
        if mutation == "ring_early" and ring is not None:
            # stage `ring` of a workgroup is read before its DMA landed: the slot still holds the stage loaded a lap earlier
            st_read = np.where(t == ring, st - ring, st)
        else:
            st_read = st
        for tt in range(2):
            for r in range(4):
                ci = st[:, None] * STAGE_KEYS + tt * 16 + g[None, :] * 4 + r                 # [nwg, 4] the id that is recorded
                cr = st_read[:, None] * STAGE_KEYS + tt * 16 + g[None, :] * 4 + r            # ... the key bytes that are read
                sc = sc_all[:, cr]                                                            # [nq, nwg, 4]
                with np.errstate(invalid="ignore"):
                    ins = (sc >= lmin) if mutation == "thr_ge" else (sc > lmin)
                ins &= live[None, :, None]
                if not ins.any():
                    continue
                nocc = (li >= 0).sum(-1)
                gt = (sc[..., None] >= lv) if mutation == "tie_displaces" else (sc[..., None] > lv)   # [nq, nwg, 4, L]
                pos = L - gt.sum(-1)                              # first slot the new score beats
                j = np.arange(L)
                newv = np.where(j < pos[..., None], lv, np.where(j == pos[..., None], sc[..., None], np.roll(lv, 1, -1)))
                newi = np.where(j < pos[..., None], li, np.where(j == pos[..., None], ci[None, :, :, None], np.roll(li, 1, -1)))
                if mutation == "short5" and L > 4:
                    short = nocc <= 4                             # one entry too many: the shift out of slot 3 is lost
                    keep_tail = short[..., None] & (j >= 4)
                    newv = np.where(keep_tail, lv, newv)
                    newi = np.where(keep_tail, li, newi)
                lv = np.where(ins[..., None], newv, lv)
                li = np.where(ins[..., None], newi, li)
                if mutation == "lmin_stale":
                    pass                                          # the threshold of the first insert stays
                else:
                    lmin = np.where(ins, np.maximum(np.broadcast_to(thr0[:, None, None], lmin.shape), lv[..., L - 1]), lmin)
    cnt = (li >= 0).sum(-1)                                       # [nq, nwg, 4]
    pairs = np.full((nq, nwg, 4 * L), sentinel, np.uint64)
    keys = ord_key(lv.ravel()).reshape(lv.shape)
    val = (keys << np.uint64(32)) | (li & 0xFFFFFFFF).astype(np.uint64)
    order = g[::-1] if mutation == "quarters_reversed" else g
    base = np.zeros((nq, nwg), np.int64)
    qi, wi = np.meshgrid(np.arange(nq), np.arange(nwg), indexing="ij")
    for gg in order:
        for jj in range(L):
            m = jj < cnt[:, :, gg]
            pairs[qi[m], wi[m], (base + jj)[m]] = val[:, :, gg, jj][m]
        base = base + cnt[:, :, gg]
    full = cnt == L
    if mutation == "metay_unfilled":
        full = cnt >= 1
        lastk = np.where(cnt >= 1, np.take_along_axis(keys, np.maximum(cnt - 1, 0)[..., None], -1)[..., 0], 0)
    else:
        lastk = keys[..., L - 1]
    lk = np.where(full, lastk, 0).max(-1)
    if mutation == "metay_missing":
        lk = np.zeros_like(lk)
    meta = np.stack([cnt.sum(-1).astype(np.uint32), lk.astype(np.uint32)], -1)
    return pairs, meta


def scan_failures(s64, e64, n, stages, nwg, depth, thr, pairs, meta, sentinel, what=""):
    """s64, e64 [nq_pad, >= stages*32]: float64 scores of the stored operands and their bound; pairs [nq_pad, nwg, 4*depth] uint64 as
    the kernel left them in a buffer filled with `sentinel`; meta [nq_pad, nwg, 2].  -> (messages, worst ratio |score - s| / e)"""
    nq = pairs.shape[0]
    L = depth
    msgs = []
    s0, s1 = wg_ranges(stages, nwg)
    thr64 = np.full(nq, -np.inf) if thr is None else thr.astype(np.float64)
    cnt = meta[:, :, 0].astype(np.int64)
    if (cnt > 4 * L).any():
        return [f"{what}meta.x above 4 * depth"], float("inf")
    slot = np.arange(4 * L)[None, None, :]
    valid = slot < cnt[..., None]
    if (pairs[~valid] != np.uint64(sentinel)).any():
        msgs.append(f"{what}{int((pairs[~valid] != np.uint64(sentinel)).sum())} slots at or behind the count were written")
    ids = (pairs & np.uint64(0xFFFFFFFF)).astype(np.int64)
    keys = (pairs >> np.uint64(32)).astype(np.int64)
    qi, wi, _ = np.nonzero(valid)
    vid, vkey = ids[valid], keys[valid]
    stage_of = vid // STAGE_KEYS
    bad_dom = (vid >= n) | (stage_of < s0[wi]) | (stage_of >= s1[wi])
    if bad_dom.any():
        msgs.append(f"{what}{int(bad_dom.sum())} listed ids outside their workgroup's keys < n (first: query {qi[bad_dom][0]}, wg {wi[bad_dom][0]}, "
                    f"id {vid[bad_dom][0]})")
        return msgs, float("inf")
    gq = (ids % 16) // 4
    both = valid[..., 1:] & valid[..., :-1]
    if (both & (gq[..., 1:] < gq[..., :-1])).any():
        msgs.append(f"{what}the four lanes' entries are not in the order g = 0 ... 3")
    same = both & (gq[..., 1:] == gq[..., :-1])
    kp, kn, ip_, in_ = keys[..., :-1], keys[..., 1:], ids[..., :-1], ids[..., 1:]
    if (same & (kn > kp)).any():
        msgs.append(f"{what}a list's scores increase")
    if (same & (kn == kp) & (in_ <= ip_)).any():
        msgs.append(f"{what}equal scores of a list are not in ascending id order (or an id is listed twice)")
    score = key_float(vkey).astype(np.float64)
    sv, ev = s64[qi, vid], e64[qi, vid]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(score == sv, 0.0, np.abs(score - sv) / ev)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        i = int(ratio.argmax())
        msgs.append(f"{what}score of query {qi[i]} id {vid[i]} off by {worst:.3g} x e (got {score[i]!r}, float64 {sv[i]!r})")
    low = sv < thr64[qi] - ev
    if low.any():
        msgs.append(f"{what}{int(low.sum())} listed keys lie below thr - e")
    # per lane (query, wg, g): entries, last score of a full list
    lane_n = np.stack([(valid & (gq == g)).sum(-1) for g in range(4)], -1)                      # [nq, nwg, 4]
    big = np.int64(1) << 40
    lane_last = np.stack([np.where(valid & (gq == g), keys, big).min(-1) for g in range(4)], -1)
    full = lane_n == L
    if (lane_n > L).any():
        msgs.append(f"{what}a lane lists more than its depth")
    want_y = np.where(full, lane_last, 0).max(-1)
    if not np.array_equal(want_y, meta[:, :, 1].astype(np.int64)):
        b = np.argwhere(want_y != meta[:, :, 1].astype(np.int64))[0]
        msgs.append(f"{what}meta.y of query {b[0]} wg {b[1]} is {int(meta[b[0], b[1], 1]):#x}, the largest last-slot key of its full lists "
                    f"is {int(want_y[b[0], b[1]]):#x}")
    # every unlisted key of the domain: s <= max(thr, last score of a full list) + e
    nk = stages * STAGE_KEYS
    listed = np.zeros((nq, nk), bool)
    listed[qi, vid] = True
    key_id = np.arange(nk)
    wg_of = np.searchsorted(s1, key_id // STAGE_KEYS, side="right")
    g_of = (key_id % 16) // 4
    lane_bound = np.where(full, key_float(np.where(full, lane_last, 0).ravel()).reshape(full.shape).astype(np.float64), -np.inf)
    bound = np.maximum(thr64[:, None], lane_bound[:, wg_of, g_of])                             # [nq, nk]
    with np.errstate(invalid="ignore"):
        missed = (~listed) & (key_id[None, :] < n) & (s64[:, :nk] > bound + e64[:, :nk])
    if missed.any():
        b = np.argwhere(missed)[0]
        msgs.append(f"{what}{int(missed.sum())} unlisted keys beat their list's bound by more than e (first: query {b[0]} key {b[1]}: "
                    f"s = {s64[b[0], b[1]]!r}, bound {bound[b[0], b[1]]!r})")
    return msgs, worst


# ---- merge ------------------------------------------------------------------------------------------------------------------------
def merge_entries(pairs, meta, q):
    cnt = meta[q, :, 0].astype(np.int64)
    return np.concatenate([pairs[q, w, :cnt[w]] for w in range(pairs.shape[1])]) if cnt.sum() else np.zeros(0, np.uint64)


def merge_sbound(T_key, V, ncand, thr_in_q, metay, use_metay=True, use_thr=True):
    b = key_float(np.array([T_key]))[0] if V > ncand else (np.float32(thr_in_q) if (thr_in_q is not None and use_thr) else np.float32(-np.inf))
    if metay and use_metay:
        b = np.maximum(b, key_float(np.array([metay]))[0])
    return np.float32(b)


def merge_model(pairs, meta, ncand, thr_in, mutation=None):
    """merge_pairs_kernel as integer arithmetic -> (cand_idx int32 [nq, ncand], cand_val f32, thr_out f32 [nq], sbound f32 [nq]).
    Mutations: cut_high, cut_low, ties_largest, stale_counted, drop_last_segment, sbound_no_metay, sbound_no_thr, no_fillers,
    ("dropbit", b): the digit walk does not see bit b of the keys."""
    nq, nwg, slots = pairs.shape
    ci = np.full((nq, ncand), -7, np.int32)
    cv = np.full((nq, ncand), np.float32(7.0))
    to = np.zeros(nq, np.float32)
    sb = np.zeros(nq, np.float32)
    for q in range(nq):
        m = meta.copy()
        if mutation == "stale_counted":
            m[q, :, 0] = np.minimum(m[q, :, 0] + 1, slots)
        if mutation == "drop_last_segment":
            m[q, nwg - 1, 0] = 0
        ent = merge_entries(pairs, m, q)
        V = len(ent)
        k = (ent >> np.uint64(32)).astype(np.int64)
        i = (ent & np.uint64(0xFFFFFFFF)).astype(np.int64)
        want = min(V, ncand)
        T = 0
        if V > ncand:
            kk = k
            if isinstance(mutation, tuple):
                kk = k & ~(np.int64(1) << mutation[1])
            place = ncand + (-1 if mutation == "cut_high" else 1 if mutation == "cut_low" else 0)
            T = int(np.sort(kk)[::-1][min(place, V) - 1])
            above = kk > T
            eq = np.nonzero(kk == T)[0]
            rem = want - int(above.sum())
            eq_sorted = eq[np.argsort(i[eq], kind="stable")]
            take = eq_sorted[::-1][:max(rem, 0)] if mutation == "ties_largest" else eq_sorted[:max(rem, 0)]
            sel = np.concatenate([np.nonzero(above)[0], take])[:ncand]
        else:
            sel = np.arange(V)
        ci[q, :len(sel)] = i[sel].astype(np.uint32).view(np.int32)
        cv[q, :len(sel)] = key_float(k[sel])
        if mutation != "no_fillers":
            ci[q, len(sel):] = -1
            cv[q, len(sel):] = -np.inf
        to[q] = key_float(np.array([T]))[0] if V > ncand else -np.inf
        sb[q] = merge_sbound(T, V, ncand, None if thr_in is None else thr_in[q], int(meta[q, :, 1].max()),
                             use_metay=mutation != "sbound_no_metay", use_thr=mutation != "sbound_no_thr")
    return ci, cv, to, sb


def merge_failures(pairs, meta, ncand, thr_in, cand_idx, cand_val, thr_out, sbound, what=""):
    """the kernel's result against the specification (sets of (id, value) pairs per row; a free choice only among more than 256 ties)"""
    nq = pairs.shape[0]
    msgs = []
    for q in range(nq):
        ent = merge_entries(pairs, meta, q)
        V = len(ent)
        k = (ent >> np.uint64(32)).astype(np.int64)
        i = (ent & np.uint64(0xFFFFFFFF)).astype(np.int64)
        got = (ord_key(cand_val[q]).astype(np.uint64) << np.uint64(32)) | cand_idx[q].view(np.uint32).astype(np.uint64)
        filler = (np.uint64(NEG_INF_KEY) << np.uint64(32)) | np.uint64(0xFFFFFFFF)
        tag = f"{what}query {q} (V = {V}): "
        if V <= ncand:
            if not np.array_equal(np.sort(got[:V]), np.sort(ent)):
                msgs.append(tag + "the candidates are not the union's entries")
            if (got[V:] != filler).any():
                msgs.append(tag + "fillers (-1, -inf) missing behind the entries")
            T = 0
        else:
            T = int(np.sort(k)[::-1][ncand - 1])
            must = ent[k > T]
            rem = ncand - len(must)
            eq = ent[k == T]
            gs = np.sort(got)
            if len(np.unique(gs)) != ncand:
                msgs.append(tag + "a candidate is listed twice")
            if len(eq) <= 256:
                want = np.sort(np.concatenate([must, np.sort(eq)[:rem]]))        # equal keys: the pair orders by id
                if not np.array_equal(gs, want):
                    msgs.append(tag + f"candidates differ from the {ncand} largest keys with ties to the smallest ids "
                                f"({int((~np.isin(want, gs)).sum())} missing)")
            else:
                if not np.isin(must, gs).all():
                    msgs.append(tag + "a key above the cut is missing")
                rest = gs[~np.isin(gs, must)]
                if len(rest) != rem or not np.isin(rest, eq).all():
                    msgs.append(tag + "the remaining candidates are not ties at the cut")
        if thr_out is not None:
            want_t = key_float(np.array([T]))[0] if V > ncand else np.float32(-np.inf)
            if f32_bits(thr_out[q:q + 1])[0] != f32_bits(np.array([want_t]))[0]:
                msgs.append(tag + f"thr_out {thr_out[q]!r}, want {want_t!r}")
        if sbound is not None:
            want_b = merge_sbound(T, V, ncand, None if thr_in is None else thr_in[q], int(meta[q, :, 1].max()))
            if not (sbound[q] == want_b and (want_b != 0 or same_bits(sbound[q:q + 1], np.array([want_b])))):
                msgs.append(tag + f"sbound {sbound[q]!r}, want {want_b!r}")
    return msgs


# ---- exact distances --------------------------------------------------------------------------------------------------------------
def dist64(q, x, metric):
    """float64 distance and its fp32 bound, row by row (q, x broadcastable [.., dim])"""
    q, x = q.astype(np.float64), x.astype(np.float64)
    dim = q.shape[-1]
    c = 4 * -(-dim // 256)
    if metric == L2:
        d = ((q - x) ** 2).sum(-1)
        return d, (c + 9) * U * d
    return (q * x).sum(-1), (c + 7) * U * (np.abs(q) * np.abs(x)).sum(-1)


def dist_model(q, x, metric, order="forward"):
    """fp32 distance in rerank_kernel's order: lane l owns columns 256 i + 4 l .. + 3, then a butterfly over the 64 lanes"""
    q, x = q.astype(np.float32), x.astype(np.float32)
    dim = q.shape[-1]
    lead = np.broadcast_shapes(q.shape[:-1], x.shape[:-1])
    s = np.zeros(lead + (64,), np.float32)
    for i in range(0, dim, 256):
        w = min(256, dim - i)
        a = np.broadcast_to(q[..., i:i + w], lead + (w,)).reshape(lead + (w // 4, 4))
        b = np.broadcast_to(x[..., i:i + w], lead + (w,)).reshape(lead + (w // 4, 4))
        p = (a - b) * (a - b) if metric == L2 else a * b
        t = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]
        s[..., :w // 4] = s[..., :w // 4] + t
    if order == "reverse":
        s = s[..., ::-1]
    width = 64
    while width > 1:
        width //= 2
        s = s[..., :width] + s[..., width:2 * width]
    return s[..., 0]


def rerank_failures(qn, db, metric, cand_idx, cand_d, what=""):
    nq, ncand = cand_idx.shape
    ok = cand_idx >= 0
    msgs = []
    inval = np.float32(np.inf if metric == L2 else -np.inf)
    if not (cand_d[~ok] == inval).all():
        msgs.append(f"{what}invalid ids do not give {inval}")
    d, b = dist64(qn[:, None, :], db[np.where(ok, cand_idx, 0)], metric)
    err = np.abs(cand_d.astype(np.float64) - d)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(ok & (err > 0), err / b, 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    if not worst <= 1.0:
        msgs.append(f"{what}distance off by {worst:.3g} x the bound")
    return msgs, worst


# ---- certify ----------------------------------------------------------------------------------------------------------------------
def bias_err(dim, metric, xmax):
    """what the L2 bias -0.5||x||^2 costs a scan score: its own fp32 sum, (dim/64 + 8) u, and dim/32 additions onto it as the MFMA chain's
    C-in, each rounding at its magnitude: (3 dim/64 + 8) u 0.5 max||x||^2; 0 for IP"""
    return (3 * dim // 64 + 8) * U * 0.5 * xmax * xmax if metric == L2 else 0.0


def cert_eps64(qstat, bounds, tk, dim, metric, with_qr=True):
    """eps(q) of the certificate in float64 from the stored qstat [.., 4] and DbBounds (xt, r, x)"""
    qs = qstat.astype(np.float64)
    xt, rm, xm = float(bounds[0]), float(bounds[1]), float(bounds[2])
    core = qs[..., 1] * xt + (qs[..., 2] * rm if with_qr else 0.0) + qs[..., 1] * rm + 2e-4 * qs[..., 2] * xt + bias_err(dim, metric, xm)
    return core * 1.01 + 1e-6 * (np.abs(tk) + qs[..., 0] + 1.0)


def certify_model(cand_idx, cand_d, metric, k, id_base, qstat, sbound, bounds, force_fail, sentinel_dk, dim, mutation=None):
    """certify_select_kernel in float32 / integers.  -> dict(D, I, verdict bool [nq] (True certified), dk f32 [nq] (sentinel where
    certified)).  Mutations: ties_larger_id, dk_rank_k, certify_short, eps_no_qr, no_id_base."""
    nq, ncand = cand_idx.shape
    D = np.zeros((nq, k), np.float32)
    I = np.zeros((nq, k), np.int64)
    verdict = np.zeros(nq, bool)
    dk_out = np.full(nq, sentinel_dk, np.float32)
    bad = np.float32(np.inf if metric == L2 else -np.inf)
    f = np.float32
    for q in range(nq):
        ids, d = cand_idx[q].astype(np.int64), cand_d[q]
        ok = np.nonzero(ids >= 0)[0]
        key = d[ok] if metric == L2 else -d[ok]
        tie = -ids[ok] if mutation == "ties_larger_id" else ids[ok]
        order = ok[np.lexsort((tie, key))]
        nvalid = len(order)
        top = order[:k]
        D[q, :len(top)] = d[top]
        I[q, :len(top)] = ids[top] + (0 if mutation == "no_id_base" else id_base)
        D[q, len(top):] = bad
        I[q, len(top):] = -1
        kth = k if mutation == "dk_rank_k" else k - 1
        s_dk = d[order[kth]] if nvalid > kth else bad
        okv = bool(np.isneginf(sbound[q]))
        if force_fail:
            okv = False
        elif not okv and (nvalid >= k or mutation == "certify_short"):
            qs = qstat[q].astype(np.float32)
            xt, rm = f(bounds[0]), f(bounds[1])
            tk = f(0.5) * (qs[0] - s_dk) if metric == L2 else s_dk
            with np.errstate(invalid="ignore", over="ignore"):
                be = f(3 * dim // 64 + 8) * f(5.9604645e-8) * f(0.5) * f(bounds[2]) * f(bounds[2]) if metric == L2 else f(0)
                core = qs[1] * xt + (qs[2] * rm if mutation != "eps_no_qr" else f(0)) + qs[1] * rm + f(2e-4) * qs[2] * xt + be
                eps = core * f(1.01) + f(1e-6) * (np.abs(tk) + qs[0] + f(1.0))
                okv = bool(tk - eps > sbound[q]) if nvalid >= k else True
        verdict[q] = okv
        if not okv:
            dk_out[q] = s_dk if nvalid >= k else bad
    return dict(D=D, I=I, verdict=verdict, dk=dk_out)


def certify_failures(cand_idx, cand_d, metric, k, id_base, qstat, sbound, bounds, force_fail, res, sentinel_dk, dim, what=""):
    """res: dict(D, I, fslot int32 [nq], fail_ids int32 [>= nq], counters int32 [8 + nq] (counters[0] was 0, [8:] nonzero before),
    dk f32 [nq] (was sentinel_dk), status int32 [2] (was 0)) -> (messages, smallest |m| / delta over the decided queries)"""
    nq, ncand = cand_idx.shape
    msgs = []
    ref = certify_model(cand_idx, cand_d, metric, k, id_base, qstat, sbound, bounds, force_fail, sentinel_dk, dim)
    if not same_bits(res["D"], ref["D"]):
        msgs.append(f"{what}D differs from the top-k by (distance, id) in {int((f32_bits(res['D']) != f32_bits(ref['D'])).any(1).sum())} queries")
    if not np.array_equal(res["I"], ref["I"]):
        msgs.append(f"{what}I differs in {int((res['I'] != ref['I']).any(1).sum())} queries")
    fslot = res["fslot"].astype(np.int64)
    failed = fslot >= 0
    nfail = int(failed.sum())
    if (fslot < -1).any() or (fslot >= nq).any():
        return msgs + [f"{what}fslot out of range"], 0.0
    if int(res["counters"][0]) != nfail:
        msgs.append(f"{what}counters[0] = {int(res['counters'][0])}, {nfail} queries have a fail slot")
    if sorted(fslot[failed].tolist()) != list(range(nfail)):
        msgs.append(f"{what}fail slots are not 0 .. nfail - 1 once each")
    elif not np.array_equal(res["fail_ids"][fslot[failed]], np.nonzero(failed)[0]):
        msgs.append(f"{what}fail_ids[fslot[q]] != q")
    if (res["counters"][8:8 + nfail] != 0).any():
        msgs.append(f"{what}counters[8 + f] not cleared for a failed slot")
    if (res["counters"][8 + nfail:] == 0).any():
        msgs.append(f"{what}counters[8 + f] cleared behind the failed slots")
    if res.get("status") is not None and (int(res["status"][0]), int(res["status"][1])) != (nq - nfail, nfail):
        msgs.append(f"{what}status {res['status'].tolist()} != (certified {nq - nfail}, failed {nfail})")
    # the verdict, in float64 from the stored inputs
    nvalid = (cand_idx >= 0).sum(1)
    dkq = ref_dk(cand_idx, cand_d, metric, k)
    tk = np.where(metric == L2, 0.5 * (qstat[:, 0].astype(np.float64) - dkq), dkq)
    eps = cert_eps64(qstat, bounds, tk, dim, metric)
    sb = sbound.astype(np.float64)
    with np.errstate(invalid="ignore"):
        m = tk - eps - sb
        delta = 8 * U * (np.abs(tk) + eps + np.abs(sb))
    closest = float("inf")
    for q in range(nq):
        if force_fail:
            must = False
        elif np.isneginf(sb[q]):
            must = True
        elif nvalid[q] < k:
            must = False
        elif m[q] > delta[q]:
            must = True
        elif m[q] < -delta[q]:
            must = False
        else:
            must = None
        if must is not None and np.isfinite(m[q]) and delta[q] > 0 and not force_fail and nvalid[q] >= k:
            closest = min(closest, abs(m[q]) / delta[q])
        if must is not None and bool(failed[q]) == must:
            msgs.append(f"{what}query {q}: {'failed' if failed[q] else 'certified'} at margin {m[q]!r} (delta {delta[q]!r}, nvalid {nvalid[q]}, "
                        f"sbound {sb[q]!r})")
        want_dk = np.float32(sentinel_dk) if not failed[q] else (np.float32(dkq[q]) if nvalid[q] >= k else np.float32(np.inf if metric == L2 else -np.inf))
        if f32_bits(res["dk"][q:q + 1])[0] != f32_bits(np.array([want_dk]))[0]:
            msgs.append(f"{what}query {q}: dk {res['dk'][q]!r}, want {want_dk!r}")
    return msgs, closest


def ref_dk(cand_idx, cand_d, metric, k):
    """the k-th distance by (distance, id) of the valid candidates as float64 (nan where fewer than k)"""
    out = np.full(cand_idx.shape[0], np.nan)
    for q in range(cand_idx.shape[0]):
        ok = np.nonzero(cand_idx[q] >= 0)[0]
        if len(ok) >= k:
            key = cand_d[q, ok] if metric == L2 else -cand_d[q, ok]
            out[q] = cand_d[q, ok[np.lexsort((cand_idx[q, ok], key))[k - 1]]]
    return out


def cert_case(metric, k, ncand, seed=0, dup=True, dim=128):
    """24 queries for the certificate: valid candidates 0 / k - 1 / k / ncand, duplicate distances, verdict margins +4 delta, -4 delta,
    +0.1 eps, -0.1 eps by groups of four queries, sbound = -inf for the last four -> (cand_idx, cand_d, qstat, sbound, bounds)"""
    rs = np.random.RandomState(seed)
    nq = 24
    ci = np.stack([rs.permutation(5000)[:ncand] for _ in range(nq)]).astype(np.int32)
    cd = (1.0 + rs.rand(nq, ncand)).astype(np.float32)
    if dup:
        cd[:, 1::2] = cd[:, 0::2]                                 # duplicate distances: the id decides
    nvalid = [0, k - 1, k, ncand]
    for q in range(nq):
        nv = nvalid[q % 4]
        drop = rs.permutation(ncand)[:ncand - nv]
        ci[q, drop] = -1
        cd[q, drop] = np.inf if metric == L2 else -np.inf
    qstat = np.stack([np.full(nq, 1.0), np.full(nq, 2e-3), np.full(nq, 1.0), np.zeros(nq)], 1).astype(np.float32)
    bounds = np.array([1.0, 2e-3, 1.0, 0.0], np.float32)
    dk = ref_dk(ci, cd, metric, k)
    tk = np.where(metric == L2, 0.5 * (1.0 - dk), dk)
    eps = cert_eps64(qstat, bounds, tk, dim, metric)
    delta = 8 * U * (np.abs(tk) + eps + np.abs(tk - eps))
    margins = np.array([4 * 1.0, -4 * 1.0, 0.0, 0.0])[(np.arange(nq) // 4) % 4] * delta + np.array([0, 0, 0.1, -0.1])[(np.arange(nq) // 4) % 4] * eps
    sbound = np.where(np.isnan(tk), 0.0, tk - eps - margins).astype(np.float32)
    sbound[20:] = -np.inf
    return ci, cd, qstat, sbound, bounds


# ---- exact pass -------------------------------------------------------------------------------------------------------------------
def exact_model(dist, dk, k, metric, id_base, chunk_rows, mutation=None):
    """exact_chunk_kernel + exact_merge_query on given fp32 distances dist [nfail, n]: per chunk the survivors' best k by (key, id), then a
    k-way merge of the chunk lists.  Mutations: prune_strict, skip_last_chunk, lists_256_unread, pop_twice."""
    nf, n = dist.shape
    nchunks = -(-n // chunk_rows)
    D = np.zeros((nf, k), np.float32)
    I = np.zeros((nf, k), np.int64)
    for f in range(nf):
        d = dist[f]
        kf = d if metric == L2 else -d
        with np.errstate(invalid="ignore"):
            if mutation == "prune_strict":
                keep = d < dk[f] if metric == L2 else d > dk[f]
            else:
                keep = d <= dk[f] if metric == L2 else d >= dk[f]
        full = (ord_key(kf) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
        lists = []
        for c in range(nchunks):
            r0, r1 = c * chunk_rows, min(n, (c + 1) * chunk_rows)
            if mutation == "skip_last_chunk" and c == nchunks - 1 and n % chunk_rows:
                lists.append(np.zeros(0, np.uint64))
                continue
            if mutation == "lists_256_unread" and c >= 256:
                lists.append(np.zeros(0, np.uint64))
                continue
            lists.append(np.sort(full[r0:r1][keep[r0:r1]])[:k])
        if mutation == "pop_twice":
            # the owner of the popped head advances by two: the entry behind every winner is lost
            pos = [0] * nchunks
            out = []
            while len(out) < k:
                heads = [(lists[c][pos[c]], c) for c in range(nchunks) if pos[c] < len(lists[c])]
                if not heads:
                    break
                h, c = min(heads)
                out.append(h)
                pos[c] += 2
            merged = np.array(out, np.uint64)
        else:
            merged = np.sort(np.concatenate(lists))[:k] if lists else np.zeros(0, np.uint64)
        m = len(merged)
        kfo = key_float(merged >> np.uint64(32))
        D[f, :m] = kfo if metric == L2 else -kfo
        I[f, :m] = (merged & np.uint64(0xFFFFFFFF)).astype(np.int64) + id_base
        D[f, m:] = np.inf if metric == L2 else -np.inf
        I[f, m:] = -1
    return D, I


def exact_failures(dist, dk, k, metric, id_base, fail_ids, D, I, D_before, I_before, what=""):
    """dist [nfail, n]: the fp32 distances the rerank entry returns for the failed queries' rows; D, I [nq, k] after the pass, *_before the
    buffers' contents before it"""
    msgs = []
    wantD, wantI = exact_model(dist, dk, k, metric, id_base, chunk_rows=max(dist.shape[1], 1))
    for f, q in enumerate(fail_ids):
        if not (same_bits(D[q], wantD[f]) and np.array_equal(I[q], wantI[f])):
            msgs.append(f"{what}failed query {q}: (D, I) differ from the top-k by (fp32 distance, id) of the rows within dk in "
                        f"{int(((f32_bits(D[q]) != f32_bits(wantD[f])) | (I[q] != wantI[f])).sum())} places")
    others = np.setdiff1d(np.arange(D.shape[0]), np.asarray(fail_ids, dtype=np.int64))
    if not (same_bits(D[others], D_before[others]) and np.array_equal(I[others], I_before[others])):
        msgs.append(f"{what}rows of queries that did not fail were written")
    return msgs


# ---- the launch plan --------------------------------------------------------------------------------------------------------------
def exact_chunk_rows(n, nq_set, k):
    rows = 2048
    while rows <= 16384:
        chunks = -(-n // rows)
        if chunks <= 2048 and chunks * nq_set * k * 8 <= EXACT_BUDGET:
            return rows
        rows *= 2
    return 0


def span_ok(stages, nwg, dim):
    return nwg > 0 and ((stages + nwg - 1) // nwg + 1) * stage_bytes(dim) < (1 << 31)


def plan_model(nq_set, dim, n, k, cus, force_single=False, thr_depth=0):
    """the rules of keds_index_search_packed_ex's shape arithmetic -> dict of PLAN_FIELDS, or None where the search is refused"""
    total = -(-n // STAGE_KEYS)
    ncand = 256 if k > LISTK else 64
    cus = min(cus, 256)
    two_phase = int(not force_single and total >= 16 * 64)
    stagesA = total // 16
    if stagesA < 512:
        stagesA = min(total // 4, 512)
    nqb = -(-nq_set // QBLOCK)
    per = max(cus // nqb, 1)
    nwgA = max(stagesA, 1) if stagesA < per else per
    nwgB = min(total, per)
    depthA = thr_depth if thr_depth in (1, 4) else (1 if nwgA * 4 >= 4 * ncand else 4)
    chunk_rows = exact_chunk_rows(n, nq_set, k)
    if not chunk_rows or not span_ok(total, nwgB, dim) or (two_phase and not span_ok(stagesA, nwgA, dim)):
        return None
    vals = (two_phase, stagesA, nqb, nwgA, nwgB, depthA, ncand, chunk_rows, -(-n // chunk_rows), total)
    return dict(zip(PLAN_FIELDS, vals))


def plan_invariant_failures(p, nq_set, dim, n, k):
    """what every plan must satisfy whatever the rules are"""
    msgs = []
    for name, nwg, stages in (("A", p["nwgA"], p["stagesA"]), ("B", p["nwgB"], p["total_stages"])):
        if name == "A" and not p["two_phase"]:
            continue
        if p["nqb"] * QBLOCK * nwg > QBLOCK * 256:
            msgs.append(f"pass {name}: {p['nqb']} blocks x {nwg} workgroups exceed lpairs")
        if nwg > 256:
            msgs.append(f"pass {name}: nwg {nwg} > 256")
        if nwg > max(stages, 1):
            msgs.append(f"pass {name}: nwg {nwg} > stages {stages}")
        if not span_ok(stages, nwg, dim):
            msgs.append(f"pass {name}: a workgroup's stage span reaches 2 GiB")
    if p["depthA"] == 1 and p["two_phase"] and not 4 * p["nwgA"] >= 4 * p["ncand"]:
        msgs.append("depth 1 with fewer than 4 ncand lane maxima")
    if p["nchunks"] > 2048 or p["nchunks"] != -(-n // p["chunk_rows"]):
        msgs.append(f"nchunks {p['nchunks']}")
    if p["nchunks"] * nq_set * k * 8 > EXACT_BUDGET:
        msgs.append("chunk lists exceed the 256 MiB budget")
    if p["chunk_rows"] > 16384:
        msgs.append("chunk_rows above the LDS survivor list")
    return msgs


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
REGIMES = ("integer", "random", "bignorm", "offset", "ramp_up", "ramp_down", "placed")


def make_inputs(regime, n, dim, nq, seed=0, placed_keys=()):
    """-> (rows fp32 [n, dim], queries fp32 [nq, dim]).  `placed`: query j's best row (a copy of the query) sits at placed_keys[j]."""
    rs = np.random.RandomState(seed * 7919 + n * 31 + dim + nq)
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)
    if regime == "integer":
        return rs.randint(-2, 3, (n, dim)).astype(np.float32), rs.randint(-2, 3, (nq, dim)).astype(np.float32)
    x = unit(rs.standard_normal((n, dim)))
    q = unit(rs.standard_normal((nq, dim)))
    if regime == "bignorm":
        x = x * (2.0 ** (np.arange(n) % 8))[:, None]
        q = q * np.where(np.arange(nq) % 2 == 0, 2.0 ** -7, 1.0)[:, None]
    elif regime == "offset":
        c = unit(rs.standard_normal((1, dim)))
        x, q = c + 0.02 * x, c + 0.02 * q
    elif regime in ("ramp_up", "ramp_down"):
        c = unit(rs.standard_normal((1, dim)))
        t = np.linspace(0.1, 0.9, n) if regime == "ramp_up" else np.linspace(0.9, 0.1, n)
        x = t[:, None] * c + 1e-3 * x
        q = np.broadcast_to(c, (nq, dim)) + 1e-3 * q
    elif regime == "placed":
        for j, key in enumerate(placed_keys):
            if j < nq and key < n:
                x[key] = q[j]
    return x.astype(np.float32), q.astype(np.float32)


def placed_keys(n, stages, nwg, dim):
    """first and last key of a middle workgroup's range, the stages at the ring's wrap, the last real key of a partial stage"""
    s0, s1 = wg_ranges(stages, nwg)
    w = nwg // 2
    nst = ring_depth(dim)
    keys = [int(s0[w]) * 32, min(int(s1[w]) * 32 - 1, n - 1), n - 1]
    for st in (nst - 1, nst, nst + 1):
        if s0[w] + st < s1[w]:
            keys.append(min((int(s0[w]) + st) * 32 + 5, n - 1))
    return keys


# ---- synthetic scan output for the merge ------------------------------------------------------------------------------------------
def key_set(kind, V, ncand, rs):
    """V uint32 keys (as int64): "equal", ("bit", b) = the top differing bit is b, "straddle" = scores around +-0,
    ("ties", t, rem) = t keys equal to the cut of which rem are taken, "random" """
    if V == 0:
        return np.zeros(0, np.int64)
    if kind == "equal":
        return np.full(V, 0xC1234567, np.int64)
    if kind == "random":
        return ord_key(rs.standard_normal(V).astype(np.float32)).astype(np.int64)
    if kind == "straddle":
        v = np.concatenate([[0.0, -0.0, 1e-45, -1e-45], rs.standard_normal(max(V - 4, 0)) * 1e-3]).astype(np.float32)[:V]
        return ord_key(rs.permutation(v)).astype(np.int64)
    if kind[0] == "bit":
        b = kind[1]
        base = 0 if b == 31 else (0xC0000000 if b < 30 else 0x80000000)
        low = rs.randint(0, 1 << b, V).astype(np.int64) if b > 0 else np.zeros(V, np.int64)
        hi = (np.arange(V) % 2).astype(np.int64)                                  # bit b itself: both values occur (V >= 2)
        k = (base & ~((1 << (b + 1)) - 1)) | (hi << b) | low
        return np.maximum(rs.permutation(k), 1)
    if kind[0] == "ties":
        t, rem = kind[1], kind[2]
        T = 0xC0000000
        above = T + 1 + rs.permutation(1 << 15)[:ncand - rem]
        below = T - 1 - rs.permutation(1 << 15)[:max(V - t - (ncand - rem), 0)]
        return rs.permutation(np.concatenate([above, np.full(t, T), below]).astype(np.int64))[:V]
    raise ValueError(kind)


def synth_segments(cnts, slots, keys, rs, metay=0, id_hi=1 << 15, sentinel_garbage=True):
    """one query's scan output: segment w holds cnts[w] entries of `keys` (sum(cnts) == len(keys)) with distinct ids, and behind them
    garbage of LARGER keys.  -> (pairs uint64 [nwg, slots], meta uint32 [nwg, 2]); meta.y = metay on segment 0"""
    nwg = len(cnts)
    ids = rs.permutation(max(id_hi, nwg * slots))[:nwg * slots].astype(np.uint64)
    pairs = (np.uint64(0xFFFFFFF0) << np.uint64(32)) | ids.reshape(nwg, slots)            # garbage: larger than every key
    if not sentinel_garbage:
        pairs = ids.reshape(nwg, slots).copy()
    pos = 0
    for w, c in enumerate(cnts):
        pairs[w, :c] = (keys[pos:pos + c].astype(np.uint64) << np.uint64(32)) | ids.reshape(nwg, slots)[w, :c]
        pos += c
    meta = np.zeros((nwg, 2), np.uint32)
    meta[:, 0] = cnts
    meta[0, 1] = metay
    return pairs, meta


def spread_counts(V, nwg, slots, rs, pattern=(0, 1, 16, 17, 64)):
    """nwg counts from `pattern` (clipped to slots) adjusted to sum to V (V <= nwg * slots)"""
    c = np.minimum(np.array([pattern[i % len(pattern)] for i in range(nwg)]), slots)
    order = rs.permutation(nwg)
    while c.sum() > V:
        w = order[int(np.argmax(c[order]))]
        c[w] -= min(c[w], c.sum() - V)
    i = 0
    while c.sum() < V:
        w = order[i % nwg]
        add = min(slots - c[w], V - c.sum())
        c[w] += add
        i += 1
    return c


# ---- the two compositions ---------------------------------------------------------------------------------------------------------
def composition_inputs(regime, n, dim, nq, seed=0):
    """-> (rows, queries, k) of the certificate's composition test.  `bignorm`: the queries are copies (every third x 2^-7, the others x 2^0) of norm-1
    rows and k = 1 -- with k = 16 the top of a bignorm database is closer together than eps (~ ||q|| max||x~|| 2^-9) allows and nothing
    would be certified; the x 2^-7 queries fail even so (the bias term of eps, 0.5 max||x||^2 14 u, is as large as their scores' gap); `random` certifies at k = 16; `offset` must not certify anything."""
    x, q = make_inputs(regime, n, dim, nq, seed=seed, placed_keys=tuple(range(5, n, max(n // max(nq, 1), 1)))[:nq])
    if regime == "bignorm":
        rows = (np.arange(nq) * 8 * max(n // (8 * nq), 1)) % n                    # norm 2^0 rows
        q = (x[rows] * np.where(np.arange(nq) % 3 == 0, 2.0 ** -7, 1.0)[:, None]).astype(np.float32)
        return x, q, 1
    return x, q, 16


def t64(qn, x, metric):
    """exact score [nq, n] in float64 on the original rows: q.x - 0.5||x||^2 (L2) or q.x"""
    q64, x64 = qn.astype(np.float64), x.astype(np.float64)
    s = q64 @ x64.T
    return s - 0.5 * (x64 ** 2).sum(1)[None, :] if metric == L2 else s


def premise_ratio(pairs, meta, t, qstat, bounds, tk, dim, metric):
    """worst |score - t64| / eps64(q) over every pair the scan listed (eps from the stored qstat, DbBounds and t_k)"""
    cnt = meta[:, :, 0].astype(np.int64)
    valid = np.arange(pairs.shape[2])[None, None, :] < cnt[..., None]
    qi = np.nonzero(valid)[0]
    ids = (pairs[valid] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    score = key_float(pairs[valid] >> np.uint64(32)).astype(np.float64)
    eps = cert_eps64(qstat, bounds, tk, dim, metric)
    return float((np.abs(score - t[qi, ids]) / eps[qi]).max()) if len(qi) else 0.0


def claim_failures(t, cand_idx, certified, k, what=""):
    """for every certified query no row outside the candidate set has t64 above the k-th candidate's t64"""
    msgs = []
    for q in np.nonzero(certified)[0]:
        c = cand_idx[q][cand_idx[q] >= 0]
        kth = np.sort(t[q, c])[::-1][k - 1]
        out = np.ones(t.shape[1], bool)
        out[c] = False
        if (t[q, out] > kth).any():
            msgs.append(f"{what}certified query {q}: {int((t[q, out] > kth).sum())} outside rows beat the k-th candidate")
    return msgs


def result_failures(qn, x, metric, k, D, I, id_base=0, what=""):
    """(D, I) against the float64 top-k; two rows may swap only where their float64 distances differ by at most the sum of their rerank
    bounds, and every returned distance is within its bound.  (The float64 distances are taken row by row as sum (q - x)^2 for the
    returned rows and the best k + 32 of a matrix-product ranking: no [nq, n, dim] array.)"""
    msgs = []
    n = x.shape[0]
    kk = min(k, n)
    rough = -t64(qn, x, metric)                                   # ascending = better (L2: half the distance up to ||q||^2)
    short = np.argsort(rough, 1, kind="stable")[:, :min(kk + 32, n)]
    for q in range(D.shape[0]):
        got = I[q] - id_base
        if (I[q, kk:] != -1).any() or set(got[:kk].tolist()) - set(range(n)) or len(set(got[:kk].tolist())) != kk:
            msgs.append(f"{what}query {q}: ids invalid or repeated")
            continue
        pool = np.union1d(short[q], got[:kk])
        d, b = dist64(qn[q][None, :], x[pool], metric)
        key = d if metric == L2 else -d
        o = np.lexsort((pool, key))
        want = pool[o][:kk]
        at = {int(r): i for i, r in enumerate(pool)}
        gi = np.array([at[int(r)] for r in got[:kk]])
        wi = o[:kk]
        if (np.abs(D[q, :kk].astype(np.float64) - d[gi]) > b[gi]).any():
            msgs.append(f"{what}query {q}: a distance is outside its rerank bound")
        for r in np.nonzero(got[:kk] != want)[0]:
            if abs(d[gi[r]] - d[wi[r]]) > b[gi[r]] + b[wi[r]]:
                msgs.append(f"{what}query {q} rank {r}: row {got[r]} for {want[r]}, float64 distances {d[gi[r]]!r} / {d[wi[r]]!r} differ by more "
                            f"than their bounds")
                break
    return msgs


def certificate_model_fraction(x, q, k, metric=L2, nwg=8):
    """the model pipeline (single phase) on rows x and queries q -> (fraction of queries the float64 certificate certifies, premise ratio)"""
    n, dim = x.shape
    stages = -(-n // STAGE_KEYS)
    xb = np.zeros((stages * STAGE_KEYS, dim), np.uint16)
    xb[:n] = bf16_bits(x)
    bias = np.full(stages * STAGE_KEYS, -np.inf, np.float32)
    x64 = x.astype(np.float64)
    bias[:n] = (-0.5 * (x64 ** 2).sum(1)).astype(np.float32) if metric == L2 else 0.0
    qb = bf16_bits(q)
    scores = scan_scores_model(xb, bias, qb)
    pairs, meta = scan_lists_model(scores, n, stages, nwg, LISTK, None, 0)
    ncand = 256 if k > LISTK else 64
    ci, cv, to, sb = merge_model(pairs, meta, ncand, None)
    cd = dist_model(q[:, None, :], x[np.maximum(ci, 0)], metric).astype(np.float32)
    cd[ci < 0] = np.inf if metric == L2 else -np.inf
    up = 1 + 5e-7
    q64, qt, xt = q.astype(np.float64), bf16_f32(qb).astype(np.float64), bf16_f32(xb[:n]).astype(np.float64)
    qstat = np.stack([(q64 ** 2).sum(1), np.sqrt(((q64 - qt) ** 2).sum(1)) * up, np.sqrt((qt ** 2).sum(1)) * up, np.zeros(len(q))], 1).astype(np.float32)
    bounds = np.array([np.sqrt((xt ** 2).sum(1)).max() * up, np.sqrt(((x64 - xt) ** 2).sum(1)).max() * up,
                       np.sqrt((x64 ** 2).sum(1)).max() * up, 0], np.float32)
    dk = ref_dk(ci, cd, metric, k)
    tk = np.where(metric == L2, 0.5 * (qstat[:, 0].astype(np.float64) - dk), dk)
    eps = cert_eps64(qstat, bounds, tk, dim, metric)
    with np.errstate(invalid="ignore"):
        cert = (tk - eps > sb.astype(np.float64)) | np.isneginf(sb)
    t = t64(q, x, metric)
    return float(cert.mean()), premise_ratio(pairs, meta, t, qstat, bounds, tk, dim, metric)


# ---- merge_parts / exchange / gather_rows: a sort keyed on (key, id) ----------------------------------------------------------------
def folded_key(d, metric):
    """the order both merges use: the distance (negated for IP) with -0 folded into +0"""
    kf = np.asarray(d, np.float32) if metric == L2 else -np.asarray(d, np.float32)
    return ord_key(kf + np.float32(0.0))


def partial_lists(parts, nq, k, metric, seed=0, big_ids=True):
    """[parts, nq, k] lists as a shard returns them: sorted by (key, id), invalid entries (id -1, any distance) at the tail; distances from a
    small set with +-0 among them (ties across parts in plenty), ids unique across the parts of a query, some >= 2^32; some queries have fewer
    than k valid entries in all parts together"""
    rs = np.random.RandomState(seed + parts * 1000 + k)
    D = np.zeros((parts, nq, k), np.float32)
    I = np.full((parts, nq, k), -1, np.int64)
    values = np.array([0.0, -0.0, 0.25, 0.5, 0.5, 1.0, 3.0, -1.0, -2.5], np.float32)
    for q in range(nq):
        ids = rs.permutation(parts * k * 2).astype(np.int64)
        if big_ids:
            ids = np.where(ids % 3 == 0, ids + (1 << 32), ids)
        sparse = q % 3 == 2                                       # fewer than k valid entries altogether
        for p in range(parts):
            nv = int(rs.randint(0, k + 1)) if not sparse else int(rs.randint(0, 2) if p < max(k // 2, 1) else 0)
            d = values[rs.randint(0, len(values), nv)]
            i = ids[p * k:p * k + nv]
            o = np.lexsort((i, folded_key(d, metric)))
            D[p, q, :nv], I[p, q, :nv] = d[o], i[o]
            D[p, q, nv:] = rs.standard_normal(k - nv)
    return D, I


def merged_topk(D, I, metric):
    """-> (D [nq, k], I [nq, k], source (part, slot) [nq, k, 2], -1 for fillers): the k best of all valid entries by (folded key, id)"""
    parts, nq, k = D.shape
    oD = np.full((nq, k), np.inf if metric == L2 else -np.inf, np.float32)
    oI = np.full((nq, k), -1, np.int64)
    src = np.full((nq, k, 2), -1, np.int64)
    for q in range(nq):
        p, j = np.nonzero(I[:, q, :] >= 0)
        o = np.lexsort((I[p, q, j], folded_key(D[p, q, j], metric)))[:k]
        oD[q, :len(o)], oI[q, :len(o)] = D[p[o], q, j[o]], I[p[o], q, j[o]]
        src[q, :len(o), 0], src[q, :len(o), 1] = p[o], j[o]
    return oD, oI, src
