"""GPU parity: similarity + top-k (FlatIndex) against the oracle's exact fp64 L2 search.

Bar: indices bit-exact (integer work), distances within 2e-6 absolute (fp32 evaluation of
sum (q-x)^2 on unit-norm data vs the oracle's fp64).  Full-size (0.5 M x 768) checks use
size-independent properties plus an oracle cross-check on a query subset.
"""
import os

import numpy as np
import pytest
import torch

import keds_amd
from keds_amd import _lib, ops
from keds_amd.index import merge_partials, shard_bounds
from oracle import keds_oracle as O
from tests.conftest import golden_path
from tests.gpu_util import max_abs, report

pytestmark = pytest.mark.gpu
D_ATOL = 2e-6


def _check(index, db, q, k, name, normalize=False, max_swap_rows=None):
    """Indices equal to the oracle's, except that two rows whose exact (fp64) distances agree within 1e-6 may swap
    ranks: the GPU orders the final candidates by fp32 distances (error ~1e-7), the oracle by fp64."""
    D, I, rows = index.search_gather(q.cuda(), k, normalize=normalize)
    qq = O.l2_normalize(q) if normalize else q
    Do, Io = O.flat_l2_search(db, qq, k)
    I, D = I.cpu(), D.cpu()
    mism = int((I != Io).sum())
    report(name, n=db.shape[0], dim=db.shape[1], nq=q.shape[0], k=k, index_mismatches=mism, d_maxabs=max_abs(D, Do))
    assert max_abs(D, Do) <= D_ATOL
    if mism:
        bad_rows = torch.nonzero((I != Io).any(dim=1)).flatten()
        limit = max(1, q.shape[0] // 200) if max_swap_rows is None else max_swap_rows
        assert len(bad_rows) <= limit, f"{len(bad_rows)} rows differ"
        for r in bad_rows.tolist():
            exact = ((qq[r].double()[None, :] - db[I[r]].double()) ** 2).sum(1)      # fp64 distances of OUR ids
            assert float((exact - Do[r].double()).abs().max()) <= 1e-6, "not a near-tie swap"
            assert len(set(I[r].tolist())) == k
    assert torch.equal(rows.cpu(), db[I.reshape(-1)].reshape(q.shape[0], k, -1)), "gathered rows differ"
    return D, I


@pytest.mark.parametrize("n,dim,nq,k", [(20000, 768, 37, 16), (20000, 768, 128, 10), (4099, 128, 5, 16),
                                        (50001, 256, 130, 1), (3000, 512, 9, 7), (2500, 1024, 3, 16),
                                        (62500, 768, 1024, 10),      # one 8-GPU shard searched for 8 ranks' queries
                                        (40000, 768, 1300, 16)])     # more than one launch set (> 1024 queries)
def test_search_matches_oracle(n, dim, nq, k):
    db = O.synth_database(n, dim, seed=2002)
    q = O.synth_database(nq, dim, seed=3003)
    idx = keds_amd.FlatIndex(dim, "l2")
    idx.add(db.numpy())
    assert idx.ntotal == n
    _check(idx, db, q, k, "search_iid")


def test_search_clustered_and_unnormalised_queries():
    db = O.synth_database(30000, 768, seed=2002, clustered=True, n_centroids=256)
    q = 3.0 * db[torch.arange(0, 30000, 997)] + 0.02 * O.synth_tensor("qnoise", [31, 768], 1.0)
    idx = keds_amd.IndexFlatL2(768)
    idx.add(db)
    _check(idx, db, q, 16, "search_clustered_normalize", normalize=True)     # eval_utils.py:162


def test_search_non_unit_database_uses_l2_not_cosine():
    """IndexFlatL2 ranks by L2 on the DB as stored (SURVEY 'L2 vs cosine'): scale rows so cosine != L2."""
    db = O.synth_database(6000, 128, seed=5) * (0.5 + torch.rand(6000, 1, generator=torch.Generator().manual_seed(1)))
    q = O.synth_database(17, 128, seed=6)
    idx = keds_amd.IndexFlatL2(128)
    idx.add(db)
    _check(idx, db, q, 16, "search_nonunit")
    _, Iip = O.flat_ip_search(db, q, 16)
    _, Il2 = O.flat_l2_search(db, q, 16)
    assert not torch.equal(Iip, Il2)                              # the case really distinguishes the metrics


def test_search_faiss_call_shape_numpy():
    g = dict(np.load(golden_path("search_small.npz")))              # minted from trainer.py:246-257
    # the golden DB is 64-d; pad to the smallest supported width with zeros (distances unchanged)
    db = torch.zeros(3000, 128)
    db[:, :64] = O.synth_database(3000, 64, seed=31)
    q = np.zeros((9, 128), np.float32)
    q[:, :64] = g["q"]
    idx = keds_amd.index_cpu_to_all_gpus(keds_amd.IndexFlatL2(128))
    idx.add(db.numpy())
    D, I = idx.search(q, 16)
    assert isinstance(D, np.ndarray) and D.dtype == np.float32 and I.dtype == np.int64
    np.testing.assert_array_equal(I, g["I_image"])
    np.testing.assert_allclose(D, g["D_image"], atol=D_ATOL)


def test_search_edge_cases():
    db = O.synth_database(40, 128, seed=7)
    q = O.synth_database(3, 128, seed=8)
    idx = keds_amd.IndexFlatL2(128)
    idx.add(db[:5])                                                # fewer rows than k: -1 / inf padding
    D, I, _ = idx.search_device(q.cuda(), 16)
    Do, Io = O.flat_l2_search(db[:5], q, 5)
    assert torch.equal(I.cpu()[:, :5], Io) and bool((I.cpu()[:, 5:] == -1).all())
    assert bool(torch.isinf(D.cpu()[:, 5:]).all())
    idx.add(db[5:])                                                # incremental add re-packs
    _check(idx, db, q, 16, "search_incremental_add")
    dup = torch.cat([db, db[:7]])                                  # exact duplicates: lower id first
    idx2 = keds_amd.IndexFlatL2(128)
    idx2.add(dup)
    D, I, _ = idx2.search_device(db[:7].cuda(), 2)
    assert torch.equal(I.cpu()[:, 0], torch.arange(7)) and torch.equal(I.cpu()[:, 1], torch.arange(40, 47))
    with pytest.raises(ValueError):
        idx.search_device(q.cuda(), 129)
    with pytest.raises(ValueError):
        keds_amd.IndexFlatL2(100)
    with pytest.raises(RuntimeError):
        keds_amd.IndexFlatL2(128).search_device(q.cuda(), 1)       # empty index


def test_inner_product_metric():
    db = O.synth_database(9000, 256, seed=11) * 1.7
    q = O.synth_database(20, 256, seed=12)
    idx = keds_amd.IndexFlatIP(256)
    idx.add(db)
    D, I, _ = idx.search_device(q.cuda(), 16)
    So, Io = O.flat_ip_search(db, q, 16)
    assert torch.equal(I.cpu(), Io)
    assert max_abs(D, So) <= 5e-6


def test_sharded_merge_bit_identical_to_single():
    """Row shards searched separately then merged keyed on (D, id) == one search."""
    n, dim = 30000, 768
    db = O.synth_database(n, dim, seed=2002)
    q = O.synth_database(64, dim, seed=3003).cuda()
    full = keds_amd.FlatIndex(dim)
    full.add(db)
    D1, I1, _ = full.search_device(q, 10)
    for world in (2, 4, 8):
        Dp, Ip = [], []
        for r in range(world):
            lo, hi = shard_bounds(n, world, r)
            sh = keds_amd.FlatIndex(dim, row0=lo)
            sh.add(db[lo:hi])
            d, i, _ = sh.search_device(q, 10)
            Dp.append(d)
            Ip.append(i)
        Dm, Im = ops.topk_merge_parts(torch.stack(Dp), torch.stack(Ip), _lib.METRIC_L2)
        assert torch.equal(Im, I1) and torch.equal(Dm, D1)
        Dh, Ih = merge_partials(torch.stack(Dp).cpu(), torch.stack(Ip).cpu())      # host twin used by gloo tests
        assert torch.equal(Ih, I1.cpu()) and torch.equal(Dh, D1.cpu())


def test_two_phase_thresholds_equal_single_phase():
    """The thresholded two-phase scan (>= 32768 rows) and the single-phase scan are both exact: identical results,
    on iid data, on clustered data, and on a database SORTED by similarity to the queries (worst case for a
    threshold taken from the first rows)."""
    lib = _lib.load()
    n, dim = 70000, 768
    dbs = {"iid": O.synth_database(n, dim, seed=41),
           "clustered": O.synth_database(n, dim, seed=42, clustered=True, n_centroids=64)}
    q = O.synth_database(40, dim, seed=43)
    order = torch.argsort(dbs["iid"] @ q[0])                     # ascending similarity to query 0: best rows LAST
    dbs["sorted_adversarial"] = dbs["iid"][order].contiguous()
    for name, db in dbs.items():
        idx = keds_amd.FlatIndex(dim)
        idx.add(db)
        D2, I2, _ = idx.search_device(q.cuda(), 16)
        lib.keds_scan_debug(0x10)
        try:
            D1, I1, _ = idx.search_device(q.cuda(), 16)
        finally:
            lib.keds_scan_debug(0)
        assert torch.equal(I1, I2) and torch.equal(D1, D2), name
        Do, Io = O.flat_l2_search(db, q, 16)
        assert torch.equal(I2.cpu(), Io), name


def test_full_size_half_million_properties():
    """BASELINE size: 0.5 M x 768.  Self-retrieval, sortedness, top-10 prefix of top-16, oracle on a subset."""
    n, dim = 500000, 768
    db = O.synth_database(n, dim, seed=2002)
    idx = keds_amd.FlatIndex(dim)
    idx.add(db)
    rows = torch.arange(0, n, n // 128)[:128]
    q = db[rows].cuda()
    D, I, _ = idx.search_device(q, 16)
    assert torch.equal(I[:, 0].cpu(), rows), "a database row must retrieve itself first"
    assert float(D[:, 0].abs().max()) <= 1e-6
    assert bool((D[:, 1:] >= D[:, :-1]).all())
    D10, I10, _ = idx.search_device(q, 10)
    assert torch.equal(I10, I[:, :10])
    qq = O.synth_database(8, dim, seed=3003)
    Dq, Iq, _ = idx.search_device(qq.cuda(), 16)
    Do, Io = O.flat_l2_search(db, qq, 16)
    mism = int((Iq.cpu() != Io).sum())
    report("search_full_size", n=n, index_mismatches=mism, d_maxabs=max_abs(Dq, Do))
    assert mism == 0 and max_abs(Dq, Do) <= D_ATOL


def test_two_million_keys_sharded_like_config5():
    """BASELINE config 5 size: 2 M x 768 keys.  Built from four 0.5 M chunks (incremental add), searched whole on one
    GPU and as 8 row shards with the 8 ranks' queries batched (1,024 queries per shard search) + (D, id) merge:
    both exact against the oracle on a query subset, self-retrieval on all."""
    dim, chunk = 768, 500000
    parts = [O.synth_database(chunk, dim, seed=2002 + i) for i in range(4)]
    idx = keds_amd.FlatIndex(dim)
    for p in parts:
        idx.add(p)
    n = idx.ntotal
    assert n == 4 * chunk
    rows = torch.arange(0, n, n // 1024)[:1024]
    q = torch.stack([parts[int(r) // chunk][int(r) % chunk] for r in rows]).cuda()
    D, I, _ = idx.search_device(q, 10)
    assert torch.equal(I[:, 0].cpu(), rows) and float(D[:, 0].abs().max()) <= 1e-6
    assert bool((D[:, 1:] >= D[:, :-1]).all())
    # 8 shards, each searched for all 1,024 queries, merged
    Dp, Ip = [], []
    for r in range(8):
        lo, hi = shard_bounds(n, 8, r)
        sh = keds_amd.FlatIndex(dim, row0=lo)
        sh.add(idx.rows[lo:hi])
        d, i, _ = sh.search_device(q, 10)
        Dp.append(d)
        Ip.append(i)
        del sh
    Dm, Im = ops.topk_merge_parts(torch.stack(Dp), torch.stack(Ip), _lib.METRIC_L2)
    assert torch.equal(Im, I) and torch.equal(Dm, D)
    # oracle on 4 fresh queries (fp64 brute force over 2 M rows, ~10 s of CPU)
    qq = O.synth_database(4, dim, seed=3003)
    Dq, Iq, _ = idx.search_device(qq.cuda(), 10)
    Do, Io = O.flat_l2_search(torch.cat(parts), qq, 10)
    report("search_2M", n=n, index_mismatches=int((Iq.cpu() != Io).sum()), d_maxabs=max_abs(Dq, Do))
    assert torch.equal(Iq.cpu(), Io) and max_abs(Dq, Do) <= D_ATOL


def test_search_random_sizes_against_oracle():
    """Seeded sweep over database sizes (ragged stage tails, below / above the two-phase threshold), dimensions, query
    counts (partial and multiple query blocks) and k."""
    rs = np.random.RandomState(77)
    for case in range(10):
        dim = int(rs.choice([128, 256, 512, 768, 1024]))
        n = int(rs.choice([1, 31, 33, 1000, 4097, 32767, 32769, 70001]))
        nq = int(rs.choice([1, 2, 127, 128, 129, 300]))
        k = int(rs.randint(1, 17))
        db = O.synth_database(n, dim, seed=500 + case, clustered=bool(case % 2), n_centroids=16)
        q = O.synth_database(nq, dim, seed=900 + case)
        idx = keds_amd.FlatIndex(dim)
        idx.add(db)
        kk = min(k, n)
        D, I, _ = idx.search_device(q.cuda(), k)
        Do, Io = O.flat_l2_search(db, q, kk)
        I, D = I.cpu(), D.cpu()
        if not torch.equal(I[:, :kk], Io):               # only exact-tie / fp32-vs-fp64 near-tie swaps are tolerated
            bad = torch.nonzero((I[:, :kk] != Io).any(dim=1)).flatten()
            assert len(bad) <= max(1, nq // 100), (n, dim, nq, k)
            for r in bad.tolist():
                exact = ((q[r].double()[None, :] - db[I[r, :kk]].double()) ** 2).sum(1)
                assert float((exact - Do[r].double()).abs().max()) <= 1e-6
        assert max_abs(D[:, :kk], Do) <= D_ATOL
        assert bool((I[:, kk:] == -1).all())


def test_exchange_merge_gather_over_rccl_single_rank():
    """The sharded search-with-rows exchange (all-to-all of partial lists and their rows, merge, row selection) on
    device tensors over a 1-rank RCCL group; the 2-rank logic runs under gloo in tests/test_host_cpu.py."""
    import os
    import torch.distributed as dist
    from keds_amd.index import exchange_merge_gather
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29611", rank=0, world_size=1,
                                device_id=torch.device("cuda", 0))
    try:
        n, dim = 9000, 256
        db = O.synth_database(n, dim, seed=21)
        q = O.synth_database(12, dim, seed=22).cuda()
        idx = keds_amd.FlatIndex(dim)
        idx.add(db)
        Dp, Ip, Rp = idx.search_gather(q, 16)
        D, I, R = exchange_merge_gather(Dp, Ip, Rp, 12, _lib.METRIC_L2)
        assert torch.equal(D, Dp) and torch.equal(I, Ip) and torch.equal(R, Rp)
        sh = keds_amd.ShardedFlatIndex(dim)
        sh.add_global(db)
        D2, I2, R2 = sh.search_gather(q, 16)
        assert torch.equal(I2, Ip) and torch.equal(R2, Rp)
    finally:
        if created:
            dist.destroy_process_group()


def test_index_save_load_and_database_extraction(tmp_path):
    """On-disk forms: FlatIndex.save/load round trip (no re-pack, identical results), loading the
    reference's plain [N, d] tensor files, and the device-side database builder."""
    db = O.synth_database(5000, 256, seed=31)
    q = O.synth_database(9, 256, seed=32).cuda()
    idx = keds_amd.FlatIndex(256, row0=640)
    idx.add(db)
    D, I, R = idx.search_gather(q, 16)
    path = str(tmp_path / "idx.pt")
    idx.save(path)
    back = keds_amd.FlatIndex.load(path)
    assert back.ntotal == 5000 and back.row0 == 640 and torch.equal(back.packed, idx.packed)
    D2, I2, R2 = back.search_gather(q, 16)
    assert torch.equal(D, D2) and torch.equal(I, I2) and torch.equal(R, R2)
    plain = str(tmp_path / "cc_image_databases.pt")
    torch.save(db, plain)                                            # the reference's own format (eval_retrieval.py:281)
    ref = keds_amd.FlatIndex.load(plain)
    _, I3, _ = ref.search_device(q, 16)
    assert torch.equal(I3 + 640, I)
    with pytest.raises(RuntimeError):
        torch.save({"x": 1}, str(tmp_path / "bad.pt"))
        keds_amd.FlatIndex.load(str(tmp_path / "bad.pt"))
    # database extraction with the tiny model: rows are unit norm and equal to encode(...) of the same batches
    from tests.test_gpu_model import TINY
    sd = O.synth_clip_state_dict(**TINY, seed=7)
    m = keds_amd.build_model(dict(sd), fp16=False).cuda()
    rs = np.random.RandomState(1)
    imgs = [torch.from_numpy(rs.standard_normal((3, 3, 56, 56)).astype(np.float32)).cuda() for _ in range(2)]
    g = dict(np.load(golden_path("clip_tiny.npz")))
    toks = [torch.from_numpy(g["text"][:3]).cuda(), torch.from_numpy(g["text"][1:4]).cuda()]
    ib, tb = keds_amd.extract_feature_database(m, imgs, toks, out_dir=str(tmp_path / "db"))
    assert ib.shape == (6, 128) and tb.shape == (6, 128)
    assert torch.allclose(ib.norm(dim=1), torch.ones(6, device="cuda"), atol=1e-5)
    assert torch.equal(ib[:3], m.encode_image(imgs[0], normalize=True))
    assert torch.equal(torch.load(str(tmp_path / "db" / "cc_text_databases.pt")), tb.cpu())
    li = keds_amd.FlatIndex.load(str(tmp_path / "db" / "cc_image_index.pt"))
    _, Iq, _ = li.search_device(ib[:2], 1)
    assert Iq[:, 0].tolist() == [0, 1]


def test_database_extraction_against_oracle_and_sharded_build(tmp_path):
    """f2 (README.md:8, eval_retrieval.py:253-286): the device-side database builder against the ORACLE --
    rows equal to the oracle's normalised encode_image / encode_text of the same inputs within the embedding tolerance,
    and a search over the built index returns the oracle's neighbours of the oracle's database -- then the per-rank
    sharded build: two 'ranks' each encode their own row range, write shard files, and the shards loaded back answer a
    query exactly like the single index (bit-identical distances and ids after the (distance, id) merge)."""
    from tests.test_gpu_model import TINY
    from keds_amd.index import merge_partials, shard_bounds
    sd = O.synth_clip_state_dict(**TINY, seed=7)
    m = keds_amd.build_model(dict(sd), fp16=False).cuda()
    rs = np.random.RandomState(3)
    n = 200
    images = torch.from_numpy(rs.standard_normal((n, 3, 56, 56)).astype(np.float32))
    tokens = torch.from_numpy(np.stack([np.concatenate([[510], rs.randint(30, 200, size=5 + i % 20), [511], np.zeros(70 - i % 20)])
                                        for i in range(n)]).astype(np.int64))
    ib, tb = keds_amd.extract_feature_database(m, [images[i:i + 64].cuda() for i in range(0, n, 64)],
                                               [tokens[i:i + 64].cuda() for i in range(0, n, 64)], out_dir=str(tmp_path / "one"))
    want_i = O.l2_normalize(O.encode_image(sd, images))
    want_t = O.l2_normalize(O.encode_text(sd, tokens))
    for name, got, want in (("image", ib, want_i), ("text", tb, want_t)):
        c = float((got.cpu() * want).sum(1).min())
        r = float((got.cpu() - want).norm() / want.norm())
        report(f"extract_feature_database.{name}", min_cosine=c, rel_l2=r)
        assert c >= 0.9999 and r <= 1.5e-2
    # (rows of the oracle's database are >= 0.16 apart; a perturbation of norm 0.02 keeps each query's neighbour decided)
    q = O.l2_normalize(want_i[:7] + 0.002 * torch.from_numpy(rs.standard_normal((7, 128)).astype(np.float32)))
    idx = keds_amd.FlatIndex.load(str(tmp_path / "one" / "cc_image_index.pt"))
    _, I, _ = idx.search_device(q.cuda(), 1)
    assert I[:, 0].tolist() == list(range(7))                     # the oracle's nearest row of every perturbed row is itself
    # ---- two ranks build their shards independently
    world = 2
    shards = []
    for r in range(world):
        ii, ti = keds_amd.extract_feature_database_sharded(m, n, lambda a, b: images[a:b].cuda(), lambda a, b: tokens[a:b].cuda(),
                                                           str(tmp_path / "sh"), rank=r, world=world, batch=48)
        lo, hi = shard_bounds(n, world, r)
        assert ii.row0 == lo and ii.ntotal == hi - lo and ti.ntotal == hi - lo
        assert torch.equal(ii.rows, ib[lo:hi]) and torch.equal(ti.rows, tb[lo:hi])      # same kernels, batch independent
    assert sorted(os.listdir(str(tmp_path / "sh"))) == ["cc_database_shards.json", "cc_image_index.shard0-of-2.pt",
                                                         "cc_image_index.shard1-of-2.pt", "cc_text_index.shard0-of-2.pt",
                                                         "cc_text_index.shard1-of-2.pt"]
    parts = [keds_amd.load_database_shard(str(tmp_path / "sh"), r, world) for r in range(world)]
    full = keds_amd.FlatIndex(128, "l2")
    full.add(tb)
    Df, If, _ = full.search_device(q.cuda(), 16)
    Dp, Ip = zip(*[p[4].search_device(q.cuda(), 16)[:2] for p in parts])
    Dm, Im = merge_partials(torch.stack(Dp).cpu(), torch.stack(Ip).cpu())
    assert torch.equal(Im, If.cpu()) and torch.equal(Dm, Df.cpu())
    with pytest.raises(RuntimeError):
        keds_amd.load_database_shard(str(tmp_path / "sh"), 0, 4)


def test_exact_ties_larger_than_k():
    """Groups of identical rows around the best match.  Up to the 64 re-ranked candidates the (distance, id) order is exact
    (lowest ids first, like the oracle's stable sort); beyond that the distances are still exact and the ids are members of
    the tied group (which of > 64 identical rows are reported is not defined by the reference either: Faiss does not order ties)."""
    dim = 256
    db = O.synth_database(20000, dim, seed=77)
    q = O.synth_database(3, dim, seed=78)
    for group, start in ((40, 5000), (200, 9000)):
        d2 = db.clone()
        d2[start:start + group] = q[0]                              # `group` exact copies of query 0
        idx = keds_amd.FlatIndex(dim)
        idx.add(d2)
        D, I, _ = idx.search_device(q.cuda(), 16)
        Do, Io = O.flat_l2_search(d2, q, 16)
        assert max_abs(D, Do) <= D_ATOL
        assert torch.equal(I.cpu()[1:], Io[1:])                     # the other queries are untouched
        got = I.cpu()[0]
        assert bool(((got >= start) & (got < start + group)).all()) and len(set(got.tolist())) == 16
        if group <= 64:
            assert torch.equal(got, Io[0])
