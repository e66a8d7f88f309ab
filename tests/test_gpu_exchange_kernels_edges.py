"""The merge end of a row-sharded search alone at its edges: keds_exchange_pack, keds_exchange_merge, keds_topk_merge_parts and
keds_gather_rows (keds_amd/csrc/search.hip) against tests/exchange_check.py -- a plain sort by (key, id), compared by bits, no tolerance.
tests/test_host_exchange_check.py shows that the checks pass line-by-line models of the kernels and catch their mutations.

Every output sits in a sentinel-filled buffer with 256 guard elements on both sides; the gap behind every part of a wide-strided message
is sentinel-filled and must survive the pack; a refused call leaves every buffer as it was."""
import numpy as np
import pytest
import torch

import keds_amd
from keds_amd import _lib
from keds_amd.index import merge_partials
from tests import exchange_check as xc
from tests.gpu_util import report

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = 256
SENT64 = 0x5EA5C0DE5EA5C0DE
SENT32 = xc.SENT32
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
    whole = torch.full((numel + 2 * G,), fill, dtype=dtype, device=DEV)
    return whole, whole[G:G + numel]


def _guards_ok(whole, fill):
    return bool((whole[:G] == fill).all()) and bool((whole[-G:] == fill).all())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Tally:
    def __init__(self, label):
        self.label, self.msgs, self.launches, self.words = label, [], 0, 0

    def add(self, msgs, guards=True, what="", words=0):
        self.launches += 1
        self.words += words
        self.msgs += [f"{what}{m}" for m in msgs]
        if not guards:
            self.msgs.append(f"{what}written outside the output buffer")

    def finish(self):
        report(f"exchange_edges.{self.label}", launches=self.launches, compared_by_bits=self.words, failures=len(self.msgs))
        assert self.launches > 0
        assert not self.msgs, f"{len(self.msgs)} failures:\n" + "\n".join(self.msgs[:30])


def _pack(lib, D, I, rows, stride):
    """keds_exchange_pack of [world, B, k] lists into a guarded sentinel-filled message -> (whole, send view, failures, guards intact)"""
    world, B, k = D.shape
    dim = 0 if rows is None else rows.shape[3]
    ws, send = _buf(world * stride, torch.int32, SENT32)
    dD, dI = _dev(D.reshape(world * B, k)), _dev(I.reshape(world * B, k))
    dR = _dev(rows.reshape(world * B, k, dim)) if dim else None
    _done(lib.keds_exchange_pack(P(dD), P(dI), P(dR), world, B, k, dim, stride, send.data_ptr(), _lib.stream()), "keds_exchange_pack")
    return ws, send, xc.pack_failures(D, I, rows, stride, send.cpu().numpy()), _guards_ok(ws, SENT32)


def _merge(lib, recv, world, B, k, dim, stride, metric):
    """keds_exchange_merge into guarded buffers -> (D, I, rows or None as numpy, guards intact and no rows written without a rows buffer)"""
    wD, oD = _buf(B * k, torch.float32, SENTF)
    wI, oI = _buf(B * k, torch.int64, SENT64)
    wR, oR = _buf(B * k * max(dim, 1), torch.float32, SENTF)
    _done(lib.keds_exchange_merge(recv.data_ptr(), world, B, k, dim, stride, metric, oD.data_ptr(), oI.data_ptr(),
                                  oR.data_ptr() if dim else None, _lib.stream()), "keds_exchange_merge")
    ok = _guards_ok(wD, SENTF) and _guards_ok(wI, SENT64) and _guards_ok(wR, SENTF) and (bool(dim) or bool((oR == SENTF).all()))
    return oD.cpu().numpy(), oI.cpu().numpy(), (oR.cpu().numpy() if dim else None), ok


def _merge_parts(lib, D, I, metric):
    parts, nq, k = D.shape
    wD, oD = _buf(nq * k, torch.float32, SENTF)
    wI, oI = _buf(nq * k, torch.int64, SENT64)
    dD, dI = _dev(D), _dev(I)
    _done(lib.keds_topk_merge_parts(P(dD), P(dI), parts, nq, k, metric, oD.data_ptr(), oI.data_ptr(), _lib.stream()), "keds_topk_merge_parts")
    return oD.cpu().numpy(), oI.cpu().numpy(), _guards_ok(wD, SENTF) and _guards_ok(wI, SENT64)


# ---- pack and merge at every table shape ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,k", xc.MERGE_SHAPES)
def test_exchange_pack_and_merge(world, k):
    """every regime in both metrics at B = 1 and 3, with rows and without, the dense stride and 2 x dense + 4: the message by words (pad
    zero, gap and guards intact), the merge by bits; and on the same lists keds_topk_merge_parts and merge_partials: one answer"""
    lib = _lib.load()
    t = Tally(f"pack_merge.w{world}.k{k}")
    big = world * k > 1024
    for B in xc.BATCHES:
        for ri, regime in enumerate(xc.REGIMES):
            for metric in xc.METRICS:
                D, I = xc.make_lists(regime, world, B, k, metric, seed=B + ri)
                want = xc.merged_reference(D, I, metric)
                what = f"{regime} metric {metric} B {B}: "
                gD, gI, ok = _merge_parts(lib, D, I, metric)
                t.add(xc.merge_failures(D, I, metric, gD, gI, what="merge_parts "), ok, what, 2 * B * k)
                hD, hI = merge_partials(torch.from_numpy(D), torch.from_numpy(I), metric)
                same = xc.same_bits(hD.numpy(), want[0]) and np.array_equal(hI.numpy(), want[1])
                t.add([] if same else ["merge_partials differs from the reference"], True, what)
                # the three row widths and the two strides: all of them on the small shapes, in rotation on the 4,096-entry ones
                dims = (0, xc.ROW_DIMS[(ri + metric) % 3]) if big else (0,) + xc.ROW_DIMS
                for dim in dims:
                    rows = xc.make_rows(world, B, k, dim) if dim else None
                    strides = (xc.dense_stride(B, k, dim), xc.wide_stride(B, k, dim))
                    for stride in (strides[(ri + B) % 2],) if big else strides:
                        w2 = f"{what}dim {dim} stride {stride}: "
                        ws, send, msgs, ok = _pack(lib, D, I, rows, stride)
                        t.add(msgs, ok, w2, world * stride)
                        before = ws.clone()
                        gD, gI, gR, ok = _merge(lib, send, world, B, k, dim, stride, metric)
                        t.add(xc.merge_failures(D, I, metric, gD, gI, rows, gR), ok and torch.equal(ws, before), w2, B * k * (2 + dim))
                        if not xc.same_bits(gD.reshape(B, k), hD.numpy()) or not np.array_equal(gI.reshape(B, k), hI.numpy()):
                            t.add(["the exchange and merge_partials differ"], True, w2)
    t.finish()


@pytest.mark.parametrize("world,k", ((2, 16), (3, 17), (5, 1)))
def test_all_to_all_of_every_rank(world, k):
    """`world` ranks, each with its shard's lists for ALL world x B queries: every rank packs, block w of every message goes to rank w as
    the all-to-all delivers it, every rank merges its own B queries.  Against the reference, keds_topk_merge_parts and merge_partials."""
    lib = _lib.load()
    t = Tally(f"all_to_all.w{world}.k{k}")
    B = 3
    for ri, regime in enumerate(xc.REGIMES):
        for metric in xc.METRICS:
            dim = (0,) + xc.ROW_DIMS
            dim = dim[(ri + metric) % 4]
            stride = xc.wide_stride(B, k, dim) if ri % 2 else xc.dense_stride(B, k, dim)
            D, I = xc.make_lists(regime, world, world * B, k, metric, seed=ri)          # [shard, query of any rank, k]
            rows = xc.make_rows(world, world * B, k, dim) if dim else None
            sends = []
            for s in range(world):                              # rank s: part w of its message = its lists for rank w's queries
                Ds, Is = D[s].reshape(world, B, k), I[s].reshape(world, B, k)
                Rs = rows[s].reshape(world, B, k, dim) if dim else None
                ws, send, msgs, ok = _pack(lib, Ds, Is, Rs, stride)
                t.add(msgs, ok, f"{regime} metric {metric} rank {s} pack: ", world * stride)
                sends.append(send.reshape(world, stride))
            for w in range(world):
                recv = torch.stack([sends[s][w] for s in range(world)]).contiguous()
                Dq, Iq = np.ascontiguousarray(D[:, w * B:(w + 1) * B]), np.ascontiguousarray(I[:, w * B:(w + 1) * B])
                Rq = np.ascontiguousarray(rows[:, w * B:(w + 1) * B]) if dim else None
                what = f"{regime} metric {metric} rank {w}: "
                gD, gI, gR, ok = _merge(lib, recv, world, B, k, dim, stride, metric)
                t.add(xc.merge_failures(Dq, Iq, metric, gD, gI, Rq, gR), ok, what, B * k * (2 + dim))
                pD, pI, ok = _merge_parts(lib, Dq, Iq, metric)
                hD, hI = merge_partials(torch.from_numpy(Dq), torch.from_numpy(Iq), metric)
                same = (xc.same_bits(pD, gD) and np.array_equal(pI, gI) and xc.same_bits(hD.numpy().reshape(-1), gD)
                        and np.array_equal(hI.numpy().reshape(-1), gI))
                t.add([] if same else ["the three merges differ"], ok, what, 4 * B * k)
    t.finish()


@pytest.mark.parametrize("dim", (0, 4))
def test_exchange_pack_more_entries_than_threads(dim):
    lib = _lib.load()
    t = Tally(f"pack.k300.dim{dim}")
    world, B, k = 2, 3, 300
    for regime in ("random", "bigid", "short"):
        D, I = xc.make_lists(regime, world, B, k, xc.L2)
        rows = xc.make_rows(world, B, k, dim) if dim else None
        for stride in (xc.dense_stride(B, k, dim), xc.wide_stride(B, k, dim)):
            _, _, msgs, ok = _pack(lib, D, I, rows, stride)
            t.add(msgs, ok, f"{regime} stride {stride}: ", world * stride)
    t.finish()


def test_exchange_refusals_leave_every_buffer_intact():
    lib = _lib.load()
    cases = (("world * k = 4160", 52, 80, 4, 0), ("k = 129", 1, 129, 4, 0), ("world = 65", 65, 1, 4, 0), ("w_stride one short", 3, 17, 4, -1),
             ("w_stride one short, no rows", 3, 17, 0, -1), ("dim % 4 != 0 with rows", 3, 17, 6, 0), ("w_stride % 4 != 0 with rows", 3, 17, 4, 2))
    B = 3
    for name, world, k, dim, dstride in cases:
        stride = xc.dense_stride(B, k, dim) + dstride
        ws, send = _buf(world * (stride + 8), torch.int32, SENT32)
        wD, oD = _buf(B * k, torch.float32, SENTF)
        wI, oI = _buf(B * k, torch.int64, SENT64)
        wR, oR = _buf(B * k * max(dim, 1), torch.float32, SENTF)
        rc = lib.keds_exchange_merge(send.data_ptr(), world, B, k, dim, stride, xc.L2, oD.data_ptr(), oI.data_ptr(),
                                     oR.data_ptr() if dim else None, _lib.stream())
        torch.cuda.synchronize()
        assert rc != 0, f"keds_exchange_merge accepted {name}"
        for whole, fill in ((ws, SENT32), (wD, SENTF), (wI, SENT64), (wR, SENTF)):
            assert bool((whole == fill).all()), f"keds_exchange_merge wrote after refusing {name}"
        if dstride or dim % 4:                                   # the pack has no limit on world or k
            dD = torch.zeros((world * B, k), dtype=torch.float32, device=DEV)
            dI = torch.zeros((world * B, k), dtype=torch.int64, device=DEV)
            dR = torch.zeros((world * B, k, max(dim, 1)), dtype=torch.float32, device=DEV)
            rc = lib.keds_exchange_pack(P(dD), P(dI), P(dR) if dim else None, world, B, k, dim, stride, send.data_ptr(), _lib.stream())
            torch.cuda.synchronize()
            assert rc != 0, f"keds_exchange_pack accepted {name}"
            assert bool((ws == SENT32).all()), f"keds_exchange_pack wrote after refusing {name}"


# ---- keds_topk_merge_parts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", xc.PARTS)
def test_merge_parts(parts):
    """parts x nq (below, at and above one 64-thread workgroup) x k (200: above the scan's largest k): the regimes in rotation, every one of
    them in both metrics at nq = 65"""
    lib = _lib.load()
    t = Tally(f"merge_parts.p{parts}")
    i = parts
    for nq in xc.PARTS_NQ:
        for k in xc.PARTS_K:
            full = nq == 65 and k in (16, 128)
            for regime in xc.REGIMES if full else (xc.REGIMES[i % len(xc.REGIMES)],):
                for metric in xc.METRICS if full else (xc.METRICS[i % 2],):
                    D, I = xc.make_lists(regime, parts, nq, k, metric, seed=i)
                    gD, gI, ok = _merge_parts(lib, D, I, metric)
                    t.add(xc.merge_failures(D, I, metric, gD, gI), ok, f"nq {nq} k {k} {regime} metric {metric}: ", 2 * nq * k)
            i += 1
    t.finish()


def test_merge_parts_refuses_65_parts():
    lib = _lib.load()
    wP, dD = _buf(65 * 2 * 4, torch.float32, 1.0)
    dI = torch.zeros(65 * 2 * 4, dtype=torch.int64, device=DEV)
    wD, oD = _buf(8, torch.float32, SENTF)
    wI, oI = _buf(8, torch.int64, SENT64)
    rc = lib.keds_topk_merge_parts(dD.data_ptr(), dI.data_ptr(), 65, 2, 4, xc.L2, oD.data_ptr(), oI.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert bool((wD == SENTF).all()) and bool((wI == SENT64).all()) and bool((wP == 1.0).all())


# ---- keds_gather_rows -------------------------------------------------------------------------------------------------------------------
def test_gather_rows():
    """count around the 4 rows of a workgroup x dim around the 256 floats of a wave's pass: the first row, the last, -1 (a zero row), an id
    twice"""
    lib = _lib.load()
    t = Tally("gather_rows")
    n = 50
    for dim in (4, 8, 252, 256, 260, 768, 1028):
        db = xc.make_rows(1, 1, n, dim, seed=dim)[0, 0]
        wdb, d_db = _buf(n * dim, torch.float32, SENTF)
        d_db.copy_(_dev(db).reshape(-1))
        for count in (1, 3, 4, 5):
            seqs = [[0, n - 1, -1, 0, n - 1][:count], [n - 1, -1, -1, 7, 7][:count], [-1, 0, n - 1, n - 1, 0][:count]]
            for idx in seqs:
                idx = np.array(idx, np.int64)
                wO, out = _buf(count * dim, torch.float32, SENTF)
                widx, d_idx = _buf(count, torch.int64, -1)
                d_idx.copy_(_dev(idx))
                _done(lib.keds_gather_rows(d_db.data_ptr(), dim, d_idx.data_ptr(), count, out.data_ptr(), _lib.stream()), "keds_gather_rows")
                same = xc.same_bits(out.cpu().numpy().reshape(count, dim), xc.gather_reference(db, idx))
                t.add([] if same else [f"dim {dim} ids {idx.tolist()}: differs"], _guards_ok(wO, SENTF), words=count * dim)
    wO, out = _buf(8, torch.float32, SENTF)
    d_idx = torch.zeros(2, dtype=torch.int64, device=DEV)
    rc = lib.keds_gather_rows(d_db.data_ptr(), 6, d_idx.data_ptr(), 1, out.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert rc != 0 and bool((wO == SENTF).all()), "dim 6 accepted, or written after the refusal"
    t.finish()


@pytest.mark.parametrize("metric", ("l2", "ip"))
def test_gather_rows_of_a_shard_with_a_large_row0(metric):
    """the id_base path of the same kernel: a shard whose first row is global row 2^33, 40 rows, k = 64: every winner's row is
    db[I - row0] by bits and the 24 fillers' rows are zero"""
    dim, n, k, row0 = 128, 40, 64, 1 << 33
    rs = np.random.RandomState(5)
    db = rs.standard_normal((n, dim)).astype(np.float32)
    q = rs.standard_normal((3, dim)).astype(np.float32)
    ix = keds_amd.FlatIndex(dim, metric, row0=row0)
    ix.add(torch.from_numpy(db))
    D, I, R = ix.search_gather(torch.from_numpy(q).to(DEV), k)
    torch.cuda.synchronize()
    I, R, D = I.cpu().numpy(), R.cpu().numpy(), D.cpu().numpy()
    assert (I[:, :n] >= row0).all() and (I[:, :n] < row0 + n).all() and (I[:, n:] == -1).all()
    assert all(len(set(r[:n])) == n for r in I.tolist())
    assert (D[:, n:] == (np.inf if metric == "l2" else -np.inf)).all()
    assert xc.same_bits(R.reshape(-1, dim), xc.gather_reference(db, I.reshape(-1), id_base=row0))
    assert not R[:, n:].any() and xc.same_bits(R[:, :n], db[I[:, :n] - row0])
    report(f"exchange_edges.gather_row0.{metric}", compared_by_bits=int(R.size))
