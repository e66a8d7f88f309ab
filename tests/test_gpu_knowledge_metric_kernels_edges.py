"""The knowledge-stream kernels (keds_amd/csrc/knowledge.hip, cross_core_f32_kernel) and the ranking kernels (keds_amd/csrc/metrics.hip)
each alone at their edges (tests/knowledge_check.py: the references, the bounds, the cases; tests/test_host_knowledge_check.py: proof
that the checks pass CPU models of the kernels and catch their mutations), and the compositions built from them -- the two forms of
keds_crossformer_forward, keds_knowledge_run fused and unfused, keds_knowledge_run_f32 -- against the chain of their public pieces, to
the bit.

Outputs sit in sentinel-filled buffers with 8 guard rows on both sides (guard columns under a stride, 1 KiB around byte buffers);
operand buffers are NaN outside the operands; workspaces and the fused-weight buffer are EXACTLY the reported bytes inside a
sentinel buffer.  Every element of every launch is compared; the worst ratio to the bound per kernel and regime goes to the metrics log.
Only arguments the entry points accept are passed to a launch; the argument errors asserted are those returned before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from keds_amd import _lib
from tests import knowledge_check as kc
from tests.gpu_util import report

pytestmark = pytest.mark.gpu

GR, GAPB, BYTE = 8, 1024, 0xA5
SENT = kc.SENT
BF, F32 = kc.BF, kc.F32
P = _lib.ptr
DEV = "cuda"
NAN = float("nan")


def _done(rc_, what):
    """a failed launch or a device fault: nothing more of this session may run on the card"""
    try:
        _lib.check(rc_, what)
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what}: {e}", returncode=3)


def _guarded(rows, cols, dtype, fill=SENT):
    buf = torch.full((rows + 2 * GR, cols), fill, dtype=dtype, device=DEV)
    return buf, buf[GR:GR + rows]


def _untouched(buf, view, fill=SENT):
    """call AFTER the results were copied out: the written region is reset and the whole buffer must be the fill"""
    view.fill_(fill)
    return bool((buf == fill).all())


def _operand(t):
    """the operand on the device with NaN rows before and behind it"""
    t2 = t.reshape(t.shape[0], -1)
    buf = torch.full((t2.shape[0] + 2 * GR, t2.shape[1]), NAN, dtype=t.dtype, device=DEV)
    buf[GR:GR + t2.shape[0]] = t2.to(DEV)
    return buf[GR:GR + t2.shape[0]]


def _bytes(n, fill=BYTE):
    """-> (buffer of n + 2 KiB bytes, the n bytes in its middle), 256-byte aligned"""
    buf = torch.full((n + 2 * GAPB,), fill, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    return buf, buf[GAPB:GAPB + n]


def _around(buf, n, fill=BYTE):
    return bool((buf[:GAPB] == fill).all()) and bool((buf[GAPB + n:] == fill).all())


def _same(a, b):
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and bool((a.contiguous().view(it) == b.contiguous().view(it)).all())


class Tally:
    def __init__(self, label):
        self.label, self.msgs, self.worst, self.launches = label, [], {}, 0

    def add(self, key, fails, worst, guards_ok=True, what=""):
        self.launches += 1
        self.msgs += [str(f) for f in fails]
        if not guards_ok:
            self.msgs.append(f"{what}: written outside its output region")
        self.worst[key] = max(self.worst.get(key, 0.0), worst)

    def finish(self):
        for key, w in sorted(self.worst.items()):
            report(f"knowledge_edges.{self.label}.{key}", worst_ratio=w)
        assert self.launches > 0
        assert not self.msgs, f"{len(self.msgs)} failures:\n" + "\n".join(self.msgs[:30])


def _one(f):
    return ([f] if f else []), f.worst


# ---- the cross-attention cores -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", kc.CORE_K)
def test_cross_attn_core(K):
    """kv_ld = inner with K and V in two buffers, and the fused form's wide buffer (kv_ld = 6 inner) at layers 0 and 2"""
    lib = _lib.load()
    t = Tally(f"core_bf16.K{K}")
    for B, H in kc.CORE_BH:
        inner = 64 * H
        for regime in kc.CORE_REGIMES:
            Q, Kp, Vp = kc.core_inputs(B, K, H, regime, BF, seed=K)
            R = kc.core_reference(Q, Kp, Vp, B, K, H)
            Qd, Kd, Vd = _operand(Q), _operand(Kp), _operand(Vp)
            layouts = [("ld_inner", Kd.data_ptr(), Vd.data_ptr(), inner, None)]
            for l in kc.WIDE_L:
                wbuf, ko, vo = kc.wide(Kp, Vp, l)
                wd = _operand(wbuf)
                layouts.append((f"wide_l{l}", wd.data_ptr() + 2 * ko, wd.data_ptr() + 2 * vo, wbuf.shape[1], wd))
            for name, kptr, vptr, ld, _keep in layouts:
                what = f"K{K}.B{B}.H{H}.{regime}.{name}"
                obuf, out = _guarded(B, inner, BF)
                _done(lib.keds_cross_attn_core(Qd.data_ptr(), kptr, vptr, out.data_ptr(), B, K, H, ld, _lib.stream()), "keds_cross_attn_core " + what)
                fails, worst = kc.core_failures(R, out.cpu(), what)
                t.add(f"{regime}.{'wide' if _keep is not None else 'ld_inner'}", fails, worst, _untouched(obuf, out), what)
    t.finish()


@pytest.mark.parametrize("K", kc.CORE_F32_K)
def test_cross_core_f32(K):
    lib = _lib.load()
    t = Tally(f"core_f32.K{K}")
    for B, H in kc.CORE_BH:
        for regime in kc.CORE_F32_REGIMES:
            Q, Kp, Vp = kc.core_inputs(B, K, H, regime, F32, seed=K)
            R = kc.core_reference(Q, Kp, Vp, B, K, H, f32=True)
            what = f"K{K}.B{B}.H{H}.{regime}"
            obuf, out = _guarded(B, 64 * H, F32)
            Qd, Kd, Vd = _operand(Q), _operand(Kp), _operand(Vp)
            _done(lib.keds_cross_core_f32(Qd.data_ptr(), Kd.data_ptr(), Vd.data_ptr(), out.data_ptr(), B, K, H, _lib.stream()), "keds_cross_core_f32 " + what)
            fails, worst = kc.core_failures(R, out.cpu(), what)
            t.add(regime, fails, worst, _untouched(obuf, out), what)
    t.finish()


# ---- pack_rows, place_token ------------------------------------------------------------------------------------------------------------------
PACK_SHAPES = [(B, K, d) for B in kc.PACK_B for K in kc.PACK_K for d in kc.PACK_DIMS] + list(kc.PACK_EXTRA)


@pytest.mark.parametrize("B,K,dim", PACK_SHAPES)
def test_pack_rows_and_place_token(B, K, dim):
    lib = _lib.load()
    t = Tally(f"pack_place.B{B}.K{K}.d{dim}")
    q, ni, nt = kc.pack_inputs(B, K, dim, seed=1)
    R = B * (1 + 2 * K)
    obuf, out = _guarded(R, dim, BF)
    qd, nid, ntd = _operand(q), _operand(ni), _operand(nt)
    _done(lib.keds_knowledge_pack_rows(qd.data_ptr(), nid.data_ptr(), ntd.data_ptr(), out.data_ptr(), B, K, dim, _lib.stream()), "keds_knowledge_pack_rows")
    t.add("pack", *_one(kc.same_bits(out.cpu(), torch.cat([q, ni, nt]).bfloat16(), "pack")), _untouched(obuf, out), "pack")
    for slot in range(3):
        tbuf, tok = _guarded(B, 3 * dim, F32)
        _done(lib.keds_place_token(qd.data_ptr(), tok.data_ptr(), B, dim, slot, 3, _lib.stream()), "keds_place_token")
        want = torch.full((B, 3, dim), SENT)
        want[:, slot] = q
        t.add("place", *_one(kc.same_bits(tok.cpu(), want.reshape(B, 3 * dim), f"place slot {slot}")), _untouched(tbuf, tok), f"place slot {slot}")
    t.finish()


# ---- keds_crossformer_fuse ---------------------------------------------------------------------------------------------------------------------
def _xf_params(Ls, dim, heads, f32=False):
    """per-layer weights (dicts of CPU tensors) -> (CrossFormerParams, what must stay alive)"""
    arr = (_lib.CrossLayerParams * len(Ls))()
    keep = []
    for i, L in enumerate(Ls):
        for n, v in L.items():
            d = (v.float() if f32 else v).to(DEV).contiguous()
            keep.append(d)
            setattr(arr[i], n, d.data_ptr())
    return _lib.CrossFormerParams(dim, heads, len(Ls), arr, None), (arr, keep)


def _fuse(lib, p, total):
    """keds_crossformer_fuse into exactly `total` bytes -> (fused struct, buffer, view)"""
    buf, view = _bytes(total)
    fused = _lib.CrossFormerFused()
    _done(lib.keds_crossformer_fuse(C.byref(p), view.data_ptr(), total, C.byref(fused), _lib.stream()), "keds_crossformer_fuse")
    return fused, buf, view


@pytest.mark.parametrize("dim,inner", kc.FUSE_SHAPES)
def test_crossformer_fuse(dim, inner):
    lib = _lib.load()
    t = Tally(f"fuse.d{dim}.i{inner}")
    for layers in kc.FUSE_LAYERS:
        lay = kc.fuse_layout(dim, inner, layers)
        for regime in kc.FUSE_REGIMES:
            what = f"dim{dim}.inner{inner}.L{layers}.{regime}"
            Ls = kc.fuse_inputs(dim, inner, layers, regime, seed=3)
            p, keep = _xf_params(Ls, dim, inner // 64)
            assert lib.keds_crossformer_fused_bytes(C.byref(p)) == lay["total"], what
            fused, buf, view = _fuse(lib, p, lay["total"])
            base = view.data_ptr()
            cpu = view.cpu()
            gaps = torch.ones(lay["total"], dtype=torch.bool)

            def part(off_n, dtype, shape):
                off, n = off_n
                gaps[off:off + n] = False
                return cpu[off:off + n].view(dtype).reshape(shape)
            got = {"wkv": part(lay["wkv"], BF, (layers * 2 * inner, dim)), "bkv": part(lay["bkv"], F32, (layers * 2 * inner,)),
                   "wqn": {l: part(lay["wqn"][l], BF, (inner, inner)) for l in range(1, layers)},
                   "bqn": {l: part(lay["bqn"][l], F32, (inner,)) for l in range(1, layers)}}
            fails, worst = kc.fuse_failures(kc.fuse_reference(Ls), got, regime == "integer", what)
            ptrs_ok = fused.wkv == base + lay["wkv"][0] and fused.bkv == base + lay["bkv"][0] and fused.wqn[0] is None and fused.bqn[0] is None
            for l in range(1, 8):
                ptrs_ok &= fused.wqn[l] == (base + lay["wqn"][l][0] if l < layers else None)
                ptrs_ok &= fused.bqn[l] == (base + lay["bqn"][l][0] if l < layers else None)
            t.add(regime, fails, worst, _around(buf, lay["total"]) and bool((cpu[gaps] == BYTE).all()) and bool(ptrs_ok), what)
    # refused before any launch, the buffer intact: nine layers; a buffer one byte short
    Ls = kc.fuse_inputs(dim, inner, 9, "random", seed=3)
    p9, keep9 = _xf_params(Ls, dim, inner // 64)
    assert lib.keds_crossformer_fused_bytes(C.byref(p9)) == 0
    buf, view = _bytes(kc.fuse_layout(dim, inner, 9)["total"])
    fused = _lib.CrossFormerFused()
    assert lib.keds_crossformer_fuse(C.byref(p9), view.data_ptr(), view.numel(), C.byref(fused), _lib.stream()) == -1
    p2, keep2 = _xf_params(Ls[:2], dim, inner // 64)
    total = kc.fuse_layout(dim, inner, 2)["total"]
    assert lib.keds_crossformer_fuse(C.byref(p2), view.data_ptr(), total - 1, C.byref(fused), _lib.stream()) == -1
    torch.cuda.synchronize()
    assert bool((buf == BYTE).all())
    t.finish()


# ---- keds_rank_gallery ---------------------------------------------------------------------------------------------------------------------------
def _rank(lib, ref, gal, short=0):
    """-> (rc, dist numpy [nq, ng] as the launch left it in the workspace, order numpy, guards intact)"""
    nq, ng, dim = ref.shape[0], gal.shape[0], ref.shape[1]
    nbytes = lib.keds_rank_gallery_workspace_bytes(nq, ng)
    wbuf, ws = _bytes(nbytes)
    obuf = torch.full((nq + 2 * GR, ng), -777, dtype=torch.int32, device=DEV)
    out = obuf[GR:GR + nq]
    refd, gald = _operand(ref), _operand(gal)
    rc_ = lib.keds_rank_gallery(refd.data_ptr(), nq, gald.data_ptr(), ng, dim, out.data_ptr(), ws.data_ptr(), nbytes - short, _lib.stream())
    if short:
        torch.cuda.synchronize()
        return rc_, None, None, bool((obuf == -777).all()) and bool((wbuf == BYTE).all())
    _done(rc_, f"keds_rank_gallery nq {nq} ng {ng} dim {dim}")
    dist = ws[:nq * ng * 4].view(torch.float32).reshape(nq, ng).cpu().numpy()
    order = out.cpu().numpy()
    return rc_, dist, order, _untouched(obuf, out, -777) and _around(wbuf, nbytes)


@pytest.mark.parametrize("ng", kc.RANK_NG)
def test_rank_gallery(ng):
    """dist per element (to the bit in `integer`), and the ordering to the bit as a function of the distances the launch stored"""
    lib = _lib.load()
    t = Tally(f"rank.ng{ng}")
    cases = [c for c in kc.rank_pairs() if c[0] == ng]
    assert cases
    for _, nq, dim in cases:
        for regime in kc.RANK_REGIMES:
            what = f"ng{ng}.nq{nq}.dim{dim}.{regime}"
            ref, gal = kc.rank_inputs(nq, ng, dim, regime, seed=ng)
            _, dist, order, ok = _rank(lib, ref, gal)
            f = kc.dist_failures(ref, gal, torch.from_numpy(dist), regime == "integer", what)
            t.add(f"dist.{regime}", *_one(f), ok, what)
            t.add(f"order.{regime}", *_one(kc.order_failures(dist, order, what)), True, what)
    _, nq, dim = cases[0]
    ref, gal = kc.rank_inputs(nq, ng, dim, "random", seed=ng)
    rc_, _, _, intact = _rank(lib, ref, gal, short=1)
    assert rc_ == -3 and intact                                                  # KEDS_E_WORKSPACE, nothing written
    t.finish()


# ---- keds_cirr_target_rank, keds_label_hits ----------------------------------------------------------------------------------------------------
def _ints(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("ng", kc.CIRR_NG)
def test_cirr_target_rank(ng):
    lib = _lib.load()
    t = Tally(f"cirr.ng{ng}")
    for nq in (None,) + kc.CIRR_NQ:
        c = kc.CirrCase(ng, nq)
        want_rank, want_counts = kc.cirr_reference(c.order, c.gallery_ids, c.ref_ids, c.target_ids)
        order, gid, rid, tid = _ints(c.order), _ints(c.gallery_ids), _ints(c.ref_ids), _ints(c.target_ids)
        for with_counts in (True, False):
            rbuf = torch.full((c.nq + 2 * GR,), -777, dtype=torch.int32, device=DEV)
            cbuf = torch.full((c.nq + 2 * GR, 2), -777, dtype=torch.int32, device=DEV)
            rank, counts = rbuf[GR:GR + c.nq], cbuf[GR:GR + c.nq]
            what = f"ng{ng}.nq{c.nq}.counts{int(with_counts)}"
            _done(lib.keds_cirr_target_rank(P(order), c.nq, ng, P(gid), P(rid), P(tid), rank.data_ptr(), counts.data_ptr() if with_counts else None,
                                            _lib.stream()), "keds_cirr_target_rank " + what)
            fs = [kc.bits_np(rank.cpu().numpy(), want_rank, what + " rank")]
            if with_counts:
                fs.append(kc.bits_np(counts.cpu().numpy(), want_counts, what + " counts"))
            ok = _untouched(rbuf, rank, -777) and (_untouched(cbuf, counts, -777) if with_counts else bool((cbuf == -777).all()))
            t.add("rank", [f for f in fs if f], max(f.worst for f in fs), ok, what)
    t.finish()


@pytest.mark.parametrize("ng", kc.CIRR_NG)
def test_label_hits(ng):
    lib = _lib.load()
    t = Tally(f"label_hits.ng{ng}")
    for nq in kc.CIRR_NQ:
        order, labels, ql = kc.label_inputs(nq, ng, seed=2)
        od, ld, qd = _ints(order), _ints(labels), _ints(ql)
        for nk in kc.LABEL_NK:
            ks = kc.label_cutoffs(ng, nk)
            want_hits, want_total = kc.label_reference(order, labels, ql, ks)
            hbuf = torch.full((nq + 2 * GR, nk), -777, dtype=torch.int32, device=DEV)
            tbuf = torch.full((nq + 2 * GR,), -777, dtype=torch.int32, device=DEV)
            hits, total = hbuf[GR:GR + nq], tbuf[GR:GR + nq]
            what = f"ng{ng}.nq{nq}.nk{nk}"
            cks = (C.c_int * nk)(*[int(k) for k in ks])
            _done(lib.keds_label_hits(P(od), nq, ng, P(ld), P(qd), cks, nk, hits.data_ptr(), total.data_ptr(), _lib.stream()), "keds_label_hits " + what)
            fs = [kc.bits_np(hits.cpu().numpy(), want_hits, what + " hits"), kc.bits_np(total.cpu().numpy(), want_total, what + " total")]
            t.add("hits", [f for f in fs if f], max(f.worst for f in fs), _untouched(hbuf, hits, -777) and _untouched(tbuf, total, -777), what)
        for nk in (0, 9):
            cks = (C.c_int * 9)(*range(9))
            assert lib.keds_label_hits(P(od), nq, ng, P(ld), P(qd), cks, nk, hits.data_ptr(), total.data_ptr(), _lib.stream()) == -1
    t.finish()


def test_argument_errors_return_before_any_launch():
    lib = _lib.load()
    st = _lib.stream()
    bbuf, b = _guarded(64, 256, BF)
    fbuf, f = _guarded(64, 256, F32)
    x, y = b.data_ptr(), f.data_ptr()
    for K in (0, 33, -1):
        assert lib.keds_cross_attn_core(x, x, x, x, 1, K, 1, 64, st) == -1
    for K in (0, 65, -1):
        assert lib.keds_cross_core_f32(y, y, y, y, 1, K, 1, st) == -1
    assert lib.keds_cross_attn_core(x, x, x, x, 1, 4, 0, 64, st) == -1             # heads < 1
    assert lib.keds_cross_attn_core(x, x, x, x, 1, 4, 2, 127, st) == -1            # kv_ld < 64 heads
    assert lib.keds_cross_attn_core(x, x, x, x, 0, 4, 1, 64, st) == -1
    assert lib.keds_cross_core_f32(y, y, y, y, 1, 4, 0, st) == -1
    for i in range(4):
        a = [x] * 4
        a[i] = None
        assert lib.keds_cross_attn_core(*a, 1, 4, 1, 64, st) == -1
        a = [y] * 4
        a[i] = None
        assert lib.keds_cross_core_f32(*a, 1, 4, 1, st) == -1
        a = [y, y, y, x]
        a[i] = None
        assert lib.keds_knowledge_pack_rows(*a, 1, 1, 8, st) == -1
    for dim in (4, 12, 129, 0):
        assert lib.keds_knowledge_pack_rows(y, y, y, x, 1, 1, dim, st) == -1
    assert lib.keds_knowledge_pack_rows(y, y, y, x, 1, 0, 8, st) == -1
    for slot, nslots in ((3, 3), (-1, 3), (0, 0)):
        assert lib.keds_place_token(y, y, 1, 8, slot, nslots, st) == -1
    assert lib.keds_place_token(None, y, 1, 8, 0, 3, st) == -1 and lib.keds_place_token(y, None, 1, 8, 0, 3, st) == -1
    torch.cuda.synchronize()
    assert bool((bbuf == SENT).all()) and bool((fbuf == SENT).all())


# ---- compositions, to the bit -------------------------------------------------------------------------------------------------------------------
def _pad_rows(rows, cols, dtype):
    """a chain buffer: GEMM operands and outputs are addressable up to the next multiple of 128 rows (and 128 more for sub-ranges)"""
    return torch.zeros(((rows + 127) // 128 * 128 + 128, cols), dtype=dtype, device=DEV)


class Stream:
    """random weights of one knowledge stream: IM2TEXT (two hidden layers) and the two CrossFormers, as bf16 and as fp32 parameters"""

    def __init__(self, dim, heads, layers, middle, seed):
        g = kc._gen(seed, dim, heads, layers, middle)
        self.dim, self.heads, self.layers, self.middle, self.inner = dim, heads, layers, middle, 64 * heads
        rnd = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
        self.i2t = [(rnd(middle, dim) / dim ** 0.5, 0.1 * rnd(middle)), (rnd(middle, middle) / middle ** 0.5, 0.1 * rnd(middle))]
        self.i2t_out = (rnd(dim, middle) / middle ** 0.5, 0.1 * rnd(dim))
        self.xf = [kc.fuse_inputs(dim, self.inner, layers, "random", seed + i) for i in range(2)]        # retrieval_fuse, text_condition
        self.keep = []

    def _dev(self, t, dtype):
        d = t.to(dtype).to(DEV).contiguous()
        self.keep.append(d)
        return d

    def params(self, lib, f32=False, fused=False):
        """-> (KnowledgeParams, dict of the device tensors by name)"""
        wt = F32 if f32 else BF
        T = {}
        i2t = _lib.Im2TextParams()
        i2t.dim_in, i2t.middle, i2t.dim_out, i2t.n_layer = self.dim, self.middle, self.dim, 2
        for i, (w, b) in enumerate(self.i2t):
            T[f"w{i}"], T[f"b{i}"] = self._dev(w, wt), self._dev(b, F32)
            i2t.w[i], i2t.b[i] = T[f"w{i}"].data_ptr(), T[f"b{i}"].data_ptr()
        T["ow"], T["ob"] = self._dev(self.i2t_out[0], wt), self._dev(self.i2t_out[1], F32)
        i2t.out_w, i2t.out_b = T["ow"].data_ptr(), T["ob"].data_ptr()
        xfs = []
        for which, Ls in enumerate(self.xf):
            arr = (_lib.CrossLayerParams * self.layers)()
            for l, L in enumerate(Ls):
                for n, v in L.items():
                    T[f"x{which}.{l}.{n}"] = self._dev(v, wt if n[0] == "w" else F32)
                    setattr(arr[l], n, T[f"x{which}.{l}.{n}"].data_ptr())
            p = _lib.CrossFormerParams(self.dim, self.heads, self.layers, arr, None)
            self.keep.append(arr)
            if fused:
                total = lib.keds_crossformer_fused_bytes(C.byref(p))
                fz, buf, view = _fuse(lib, p, total)
                self.keep += [fz, buf]
                p.fused = C.pointer(fz)
                T[f"x{which}.fused"] = fz
            xfs.append(p)
        return _lib.KnowledgeParams(i2t, xfs[0], xfs[1]), T


def _gemm(lib, A, W, bias, out, M, N, K, epi, aux=None, aux_i=0):
    _done(lib.keds_gemm_bt(A, W, bias, out, M, N, K, epi, aux, aux_i, _lib.stream()), "keds_gemm_bt")


def _chain_xf(lib, S, T, which, q_bf, k_bf, v_bf, B, K, out, ld_out):
    """xf_run: per layer three projections, the core, the output projection; q_bf / k_bf / v_bf: device pointers of bf16 rows"""
    dim, inner, BK = S.dim, S.inner, B * K
    Qp, Kp, Vp, att, qcur = (_pad_rows(r, c, BF) for r, c in ((B, inner), (BK, inner), (BK, inner), (B, inner), (B, dim)))
    qin = q_bf
    for l in range(S.layers):
        w = lambda n: T[f"x{which}.{l}.{n}"].data_ptr()   # noqa: E731
        _gemm(lib, qin, w("wq"), w("bq"), P(Qp), B, inner, dim, _lib.EPI_BIAS_BF16)
        _gemm(lib, k_bf, w("wk"), w("bk"), P(Kp), BK, inner, dim, _lib.EPI_BIAS_BF16)
        _gemm(lib, v_bf, w("wv"), w("bv"), P(Vp), BK, inner, dim, _lib.EPI_BIAS_BF16)
        _done(lib.keds_cross_attn_core(P(Qp), P(Kp), P(Vp), P(att), B, K, S.heads, inner, _lib.stream()), "keds_cross_attn_core")
        if l == S.layers - 1:
            assert ld_out == dim
            _gemm(lib, P(att), w("wo"), w("bo"), out, B, dim, inner, _lib.EPI_BIAS_F32)
        else:
            _gemm(lib, P(att), w("wo"), w("bo"), P(qcur), B, dim, inner, _lib.EPI_BIAS_BF16)
            qin = P(qcur)


def _chain_xf_fused(lib, S, T, which, q_bf, kv_bf, B, K, out, ld_out):
    """xf_run_fused: ONE k | v GEMM with N = layers 2 inner, the first query GEMM, the core with kv_ld, the folded query GEMMs, and the
    output projection with ldc"""
    dim, inner, BK, kv_ld = S.dim, S.inner, B * K, S.layers * 2 * S.inner
    fz = T[f"x{which}.fused"]
    KV, Qp, att = _pad_rows(BK, kv_ld, BF), _pad_rows(B, inner, BF), _pad_rows(B, inner, BF)
    _gemm(lib, kv_bf, fz.wkv, fz.bkv, P(KV), BK, kv_ld, dim, _lib.EPI_BIAS_BF16)
    for l in range(S.layers):
        if l == 0:
            _gemm(lib, q_bf, T[f"x{which}.0.wq"].data_ptr(), T[f"x{which}.0.bq"].data_ptr(), P(Qp), B, inner, dim, _lib.EPI_BIAS_BF16)
        else:
            _gemm(lib, P(att), fz.wqn[l], fz.bqn[l], P(Qp), B, inner, inner, _lib.EPI_BIAS_BF16)
        kp = P(KV) + 2 * l * 2 * inner
        _done(lib.keds_cross_attn_core(P(Qp), kp, kp + 2 * inner, P(att), B, K, S.heads, kv_ld, _lib.stream()), "keds_cross_attn_core")
    last = S.layers - 1
    _done(lib.keds_gemm_bt_ex(P(att), inner, T[f"x{which}.{last}.wo"].data_ptr(), T[f"x{which}.{last}.bo"].data_ptr(), out, ld_out, B, dim, inner,
                              _lib.EPI_BIAS_F32, None, 0, _lib.stream()), "keds_gemm_bt_ex")


def _cast(lib, src, rows, cols):
    out = _pad_rows(rows, cols, BF)
    _done(lib.keds_cast_bf16(P(src), P(out), rows * cols, _lib.stream()), "keds_cast_bf16")
    return out


def _twice(run, nbytes, out_rows, out_cols):
    """run(workspace pointer, nbytes, out pointer) with the workspace prefilled with 0xFF bytes, then with zeros, each exactly
    `nbytes` inside a sentinel buffer -> the output (equal bits both times, finite, guards intact)"""
    outs = []
    for fill in (0xFF, 0x00):
        wbuf, ws = _bytes(nbytes)
        ws.fill_(fill)
        obuf, out = _guarded(out_rows, out_cols, F32)
        run(ws.data_ptr(), nbytes, out.data_ptr())
        torch.cuda.synchronize()
        outs.append(out.clone())
        assert _around(wbuf, nbytes), "bytes around the workspace changed"
        assert _untouched(obuf, out), "written outside the output rows"
    assert _same(outs[0], outs[1]), "the result depends on scratch the call did not write"
    assert bool(torch.isfinite(outs[0]).all())
    return outs[0]


@pytest.fixture
def no_splitk():
    """keds_knowledge_run never splits K (its two chains share no scratch); a chain of direct GEMM calls must plan the same way"""
    lib = _lib.load()
    _lib.check(lib.keds_gemm_set_workspace(None, 0), "keds_gemm_set_workspace")
    yield lib
    buf = _lib._gemm_ws.get(torch.cuda.current_device())
    if buf is not None:
        _lib.check(lib.keds_gemm_set_workspace(buf.data_ptr(), buf.numel()), "keds_gemm_set_workspace")


COMPOSE = [(128, 2, 3, 128, B, K) for B, K in ((1, 1), (3, 5), (9, 16), (9, 32))] + [(768, 12, 3, 256, 3, 16)]


def _inputs(S, B, K, seed):
    g = kc._gen(seed, B, K)
    return [torch.randn(n, S.dim, generator=g).to(DEV) for n in (B, B * K, B * K)]


@pytest.mark.parametrize("dim,heads,layers,middle,B,K", COMPOSE)
def test_crossformer_forward_equals_its_chain(no_splitk, dim, heads, layers, middle, B, K):
    lib = no_splitk
    S = Stream(dim, heads, layers, middle, seed=B * 100 + K)
    q, k, _ = _inputs(S, B, K, seed=1)
    v = k.clone()
    dist = {}
    for fused in (False, True):
        kp, T = S.params(lib, fused=fused)
        p = kp.fuse
        nbytes = lib.keds_crossformer_workspace_bytes(C.byref(p), B, K)
        q_bf, k_bf, v_bf = _cast(lib, q, B, dim), _cast(lib, k, B * K, dim), _cast(lib, v, B * K, dim)
        want_u = _pad_rows(B, dim, F32)[:B]
        _chain_xf(lib, S, T, 0, P(q_bf), P(k_bf), P(v_bf), B, K, P(want_u), dim)
        want_a = _pad_rows(B, dim, F32)[:B]                                       # v aliasing k
        _chain_xf(lib, S, T, 0, P(q_bf), P(k_bf), P(k_bf), B, K, P(want_a), dim)
        assert _same(want_u, want_a)
        run = lambda vv: (lambda ws, n, out: _done(lib.keds_crossformer_forward(C.byref(p), P(q), P(k), P(vv), B, K, out, ws, n, _lib.stream()),   # noqa: E731
                                                   "keds_crossformer_forward"))
        # a separate v with equal contents takes the layer-by-layer path, `fused` set or not
        assert _same(_twice(run(v), nbytes, B, dim), want_u), f"fused={fused}: v separate"
        got = _twice(run(k), nbytes, B, dim)
        if fused:
            want_f = _pad_rows(B, dim, F32)[:B]
            _chain_xf_fused(lib, S, T, 0, P(q_bf), P(k_bf), B, K, P(want_f), dim)
            torch.cuda.synchronize()
            assert _same(got, want_f), "fused form against its chain"
            dist["fused_vs_unfused"] = float((want_f.double() - want_u.double()).abs().max() / want_u.double().abs().max())
        else:
            assert _same(got, want_u), "v == k without `fused`"
        assert lib.keds_crossformer_forward(C.byref(p), P(q), P(k), P(k), B, K, P(want_a), P(q_bf), nbytes - 1, _lib.stream()) == -3
    report(f"knowledge_edges.compose.crossformer.d{dim}.B{B}.K{K}", **dist)


def _chain_knowledge(lib, S, T, q, ni, nt, B, K, tokens, fused):
    dim, mid, BK = S.dim, S.middle, B * K
    R = B * (1 + 2 * K)
    rows, h0, h1, map_bf = _pad_rows(R, dim, BF), _pad_rows(R, mid, BF), _pad_rows(R, mid, BF), _pad_rows(R + 128, dim, BF)
    st = _lib.stream()
    if fused:
        _done(lib.keds_knowledge_pack_rows(P(q), P(ni), P(nt), P(rows), B, K, dim, st), "keds_knowledge_pack_rows")
    else:
        for src, r0, n in ((q, 0, B), (ni, B, BK), (nt, B + BK, BK)):
            _done(lib.keds_cast_bf16(P(src), P(rows) + 2 * r0 * dim, n * dim, st), "keds_cast_bf16")
    _gemm(lib, P(rows), T["w0"].data_ptr(), T["b0"].data_ptr(), P(h0), R, mid, dim, _lib.EPI_BIAS_RELU_BF16)
    _gemm(lib, P(h0), T["w1"].data_ptr(), T["b1"].data_ptr(), P(h1), R, mid, mid, _lib.EPI_BIAS_RELU_BF16)
    tok = tokens.data_ptr()
    mb = P(map_bf)
    if fused:
        _gemm(lib, P(h1), T["ow"].data_ptr(), T["ob"].data_ptr(), mb, R, dim, mid, _lib.EPI_BIAS_BF16_HEADF32, tok + 4 * 2 * dim, B)
        _chain_xf_fused(lib, S, T, 1, mb, mb + 2 * (B + BK) * dim, B, K, tok + 4 * dim, 3 * dim)
        _chain_xf_fused(lib, S, T, 0, mb, mb + 2 * B * dim, B, K, tok, 3 * dim)
        return
    map_f, outf = _pad_rows(R, dim, F32), _pad_rows(B, dim, F32)
    _gemm(lib, P(h1), T["ow"].data_ptr(), T["ob"].data_ptr(), P(map_f), R, dim, mid, _lib.EPI_BIAS_F32)
    _done(lib.keds_cast_bf16(P(map_f), mb, R * dim, st), "keds_cast_bf16")
    _done(lib.keds_place_token(P(map_f), tok, B, dim, 2, 3, st), "keds_place_token")
    for which in range(2):
        nb = mb + 2 * (B + which * BK) * dim
        _chain_xf(lib, S, T, which, mb, nb, nb, B, K, P(outf), dim)
        _done(lib.keds_place_token(P(outf), tok, B, dim, which, 3, st), "keds_place_token")


@pytest.mark.parametrize("dim,heads,layers,middle,B,K", COMPOSE)
def test_knowledge_run_equals_its_chain(no_splitk, dim, heads, layers, middle, B, K):
    """fused and unfused, every token slot of a sentinel-filled [B, 3, dim]; side lane on and off; and how far the two forms differ"""
    lib = no_splitk
    S = Stream(dim, heads, layers, middle, seed=B * 100 + K)
    q, ni, nt = _inputs(S, B, K, seed=2)
    res = {}
    for fused in (False, True):
        kp, T = S.params(lib, fused=fused)
        nbytes = lib.keds_knowledge_workspace_bytes(C.byref(kp), B, K)
        cbuf, want = _guarded(B, 3 * dim, F32)
        _chain_knowledge(lib, S, T, q, ni, nt, B, K, want, fused)
        torch.cuda.synchronize()
        want = want.clone()
        assert bool(torch.isfinite(want).all()) and not bool((want == SENT).any())
        run = lambda ws, n, out: _done(lib.keds_knowledge_run(C.byref(kp), P(q), P(ni), P(nt), B, K, out, ws, n, _lib.stream()), "keds_knowledge_run")   # noqa: E731
        try:
            for lane in (1, 0):
                _lib.check(lib.keds_side_lane_enable(lane), "keds_side_lane_enable")
                got = _twice(run, nbytes, B, 3 * dim)
                for slot in range(3):
                    assert _same(got[:, slot * dim:(slot + 1) * dim], want[:, slot * dim:(slot + 1) * dim]), f"fused={fused} side lane {lane}: token slot {slot}"
        finally:
            _lib.check(lib.keds_side_lane_enable(1), "keds_side_lane_enable")
        res[fused] = want.double()
        assert lib.keds_knowledge_run(C.byref(kp), P(q), P(ni), P(nt), B, K, P(cbuf), P(cbuf), nbytes - 1, _lib.stream()) == -3
    d = {f"slot{s}": float((res[True] - res[False])[:, s * dim:(s + 1) * dim].abs().max() / res[False][:, s * dim:(s + 1) * dim].abs().max()) for s in range(3)}
    report(f"knowledge_edges.compose.knowledge_run.d{dim}.B{B}.K{K}", **{"fused_vs_unfused_" + k: v for k, v in d.items()})


I2T = [(128, middle, n_layer) for middle in (128, 256) for n_layer in (1, 2, 3)]


@pytest.mark.parametrize("dim,middle,n_layer", I2T)
def test_im2text_forward_equals_its_chain(dim, middle, n_layer):
    """the cast, n_layer x (Linear, ReLU) through two buffers in turn (at n_layer = 3 the third layer writes the buffer the second one
    read), the output Linear; rows on both sides of the 128-row padding"""
    lib = _lib.load()
    g = kc._gen(7, dim, middle, n_layer)
    rnd = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    dims = [dim] + [middle] * n_layer
    W = [(rnd(middle, k) / k ** 0.5).to(BF).to(DEV) for k in dims[:-1]] + [(rnd(dim, middle) / middle ** 0.5).to(BF).to(DEV)]
    bias = [(0.1 * rnd(middle)).to(DEV) for _ in range(n_layer)] + [(0.1 * rnd(dim)).to(DEV)]
    p = _lib.Im2TextParams()
    p.dim_in, p.middle, p.dim_out, p.n_layer = dim, middle, dim, n_layer
    for i in range(n_layer):
        p.w[i], p.b[i] = W[i].data_ptr(), bias[i].data_ptr()
    p.out_w, p.out_b = W[-1].data_ptr(), bias[-1].data_ptr()
    for rows in (1, 129):
        x = rnd(rows, dim).to(DEV)
        cur, h = _cast(lib, x, rows, dim), [_pad_rows(rows, middle, BF), _pad_rows(rows, middle, BF)]
        for i in range(n_layer):
            _gemm(lib, P(cur), P(W[i]), P(bias[i]), P(h[i & 1]), rows, middle, dims[i], _lib.EPI_BIAS_RELU_BF16)
            cur = h[i & 1]
        want = _pad_rows(rows, dim, F32)[:rows]
        _gemm(lib, P(cur), P(W[-1]), P(bias[-1]), P(want), rows, dim, middle, _lib.EPI_BIAS_F32)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(want).all())
        nbytes = lib.keds_im2text_workspace_bytes(C.byref(p), rows)
        run = lambda ws, n, out: _done(lib.keds_im2text_forward(C.byref(p), P(x), rows, out, ws, n, _lib.stream()), "keds_im2text_forward")   # noqa: E731
        assert _same(_twice(run, nbytes, rows, dim), want), f"rows={rows}"
        assert lib.keds_im2text_forward(C.byref(p), P(x), rows, P(want), P(cur), nbytes - 1, _lib.stream()) == -3


def _gemm32(lib, A, lda, W, bias, out, ldc, M, N, K, epi):
    _done(lib.keds_gemm_f32(A, lda, W, bias, out, ldc, M, N, K, epi, None, 0, _lib.stream()), "keds_gemm_f32")


# keds_knowledge_run_f32 takes up to 64 neighbours (keds_cross_core_f32's own limit), twice what the bf16 entries take
COMPOSE_F32 = COMPOSE + [(128, 2, 3, 128, 2, 64)]


@pytest.mark.parametrize("dim,heads,layers,middle,B,K", COMPOSE_F32)
def test_knowledge_run_f32_equals_its_chain(dim, heads, layers, middle, B, K):
    lib = _lib.load()
    S = Stream(dim, heads, layers, middle, seed=B * 100 + K)
    q, ni, nt = _inputs(S, B, K, seed=3)
    kp, T = S.params(lib, f32=True)
    mid, inner, BK = S.middle, S.inner, B * K
    R = B + 2 * BK
    cbuf, want = _guarded(B, 3 * dim, F32)
    tok = want.data_ptr()
    x = _pad_rows(R, dim, F32)
    x[:R] = torch.cat([q, ni, nt])
    h0, h1, y = _pad_rows(R, mid, F32), _pad_rows(R, mid, F32), _pad_rows(2 * BK, dim, F32)
    _gemm32(lib, P(x), dim, T["w0"].data_ptr(), T["b0"].data_ptr(), P(h0), mid, R, mid, dim, _lib.F32_EPI_RELU)
    _gemm32(lib, P(h0), mid, T["w1"].data_ptr(), T["b1"].data_ptr(), P(h1), mid, R, mid, mid, _lib.F32_EPI_RELU)
    _gemm32(lib, P(h1), mid, T["ow"].data_ptr(), T["ob"].data_ptr(), tok + 4 * 2 * dim, 3 * dim, B, dim, mid, _lib.F32_EPI_BIAS)
    _gemm32(lib, P(h1) + 4 * B * mid, mid, T["ow"].data_ptr(), T["ob"].data_ptr(), P(y), dim, 2 * BK, dim, mid, _lib.F32_EPI_BIAS)
    qp, kpj, vpj, core, qt = (_pad_rows(r, c, F32) for r, c in ((B, inner), (BK, inner), (BK, inner), (B, inner), (B, dim)))
    for which in range(2):
        qin, ldq, kv = tok + 4 * 2 * dim, 3 * dim, P(y) + 4 * which * BK * dim
        for l in range(layers):
            w = lambda n: T[f"x{which}.{l}.{n}"].data_ptr()   # noqa: E731
            _gemm32(lib, qin, ldq, w("wq"), w("bq"), P(qp), inner, B, inner, dim, _lib.F32_EPI_BIAS)
            _gemm32(lib, kv, dim, w("wk"), w("bk"), P(kpj), inner, BK, inner, dim, _lib.F32_EPI_BIAS)
            _gemm32(lib, kv, dim, w("wv"), w("bv"), P(vpj), inner, BK, inner, dim, _lib.F32_EPI_BIAS)
            _done(lib.keds_cross_core_f32(P(qp), P(kpj), P(vpj), P(core), B, K, heads, _lib.stream()), "keds_cross_core_f32")
            last = l == layers - 1
            _gemm32(lib, P(core), inner, w("wo"), w("bo"), tok + 4 * which * dim if last else P(qt), 3 * dim if last else dim, B, dim, inner, _lib.F32_EPI_BIAS)
            qin, ldq = P(qt), dim
    torch.cuda.synchronize()
    want = want.clone()
    assert bool(torch.isfinite(want).all()) and not bool((want == SENT).any())
    nbytes = lib.keds_knowledge_f32_workspace_bytes(C.byref(kp), B, K)
    run = lambda ws, n, out: _done(lib.keds_knowledge_run_f32(C.byref(kp), P(q), P(ni), P(nt), B, K, out, ws, n, _lib.stream()), "keds_knowledge_run_f32")   # noqa: E731
    got = _twice(run, nbytes, B, 3 * dim)
    for slot in range(3):
        assert _same(got[:, slot * dim:(slot + 1) * dim], want[:, slot * dim:(slot + 1) * dim]), f"token slot {slot}"
    assert lib.keds_knowledge_run_f32(C.byref(kp), P(q), P(ni), P(nt), B, K, P(cbuf), P(cbuf), nbytes - 1, _lib.stream()) == -3
