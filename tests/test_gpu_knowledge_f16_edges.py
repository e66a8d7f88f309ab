"""The kernels of the fp16 knowledge stream (include/keds_knowledge_f16.h) each alone at their edges: the fp16 instantiations of
cross_attn_core_kernel, pack_rows_kernel, concat_rows_kernel and fold_qo_kernel (keds_amd/csrc/knowledge.hip) and the GEMM epilogues
32 - 34 (keds_amd/csrc/gemm.hip), per element against float64 on the inputs as the kernel receives them.

The cases, references and bounds are those of the bf16 kernels (tests/knowledge_check.py, tests/train_check.py, tests/gemm_check.py)
with the output's unit roundoff 2^-11 in place of 2^-8 -- the helpers take the type; nothing here was tuned on an output.  The GEMM
bound is gemm_check's: C_ACC (K + 16) u32 S for the accumulation, 2 u32 (S + |bias|) for the epilogue's additions, and for the fp16
output e (1 + 2 u) + u |ref| + 2^-25 + 2^-126; `integer` cases to the bit.  Outputs sit in sentinel-filled buffers with guard rows
on both sides, operands in NaN-filled ones.  The range flag: a value of 70,000 raises the flag of the call that stores it and leaves
the calling thread's tower guard untouched."""
import ctypes as C
import functools

import pytest
import torch

from keds_amd import _lib
from tests import gemm_check as gc
from tests import knowledge_check as kc
from tests import test_gpu_knowledge_metric_kernels_edges as ke
from tests.gpu_util import report

pytestmark = pytest.mark.gpu

HF, F32, BF = torch.float16, torch.float32, torch.bfloat16
SENT, DEV, GR = kc.SENT, "cuda", ke.GR
P = _lib.ptr
_done, _guarded, _untouched, _operand, _one = ke._done, ke._guarded, ke._untouched, ke._operand, ke._one


class Tally(ke.Tally):
    def finish(self):
        for key, w in sorted(self.worst.items()):
            report(f"knowledge_f16_edges.{self.label}.{key}", worst_ratio=w)
        assert self.launches > 0
        assert not self.msgs, f"{len(self.msgs)} failures:\n" + "\n".join(self.msgs[:30])


# ---- the cross-attention core ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", kc.CORE_K)
def test_cross_attn_core_h(K):
    """kv_ld = inner with K and V in two buffers, and the fused form's wide buffer (kv_ld = 6 inner, NaN elsewhere) at layers 0 and 2"""
    lib = _lib.load()
    t = Tally(f"core_f16.K{K}")
    for B, H in kc.CORE_BH:
        inner = 64 * H
        for regime in kc.CORE_REGIMES:
            Q, Kp, Vp = kc.core_inputs(B, K, H, regime, HF, seed=K)
            R = kc.core_reference(Q, Kp, Vp, B, K, H)
            Qd, Kd, Vd = _operand(Q), _operand(Kp), _operand(Vp)
            layouts = [("ld_inner", Kd.data_ptr(), Vd.data_ptr(), inner, None)]
            for l in kc.WIDE_L:
                wbuf, ko, vo = kc.wide(Kp, Vp, l)
                wd = _operand(wbuf)
                layouts.append((f"wide_l{l}", wd.data_ptr() + 2 * ko, wd.data_ptr() + 2 * vo, wbuf.shape[1], wd))
            for name, kptr, vptr, ld, _keep in layouts:
                what = f"K{K}.B{B}.H{H}.{regime}.{name}"
                obuf, out = _guarded(B, inner, HF)
                _done(lib.keds_cross_attn_core_h(Qd.data_ptr(), kptr, vptr, out.data_ptr(), B, K, H, ld, _lib.stream()), "keds_cross_attn_core_h " + what)
                got = out.cpu()
                assert got.dtype == HF
                fails, worst = kc.core_failures(R, got, what)                       # (held() takes u_out from the output's type: 2^-11)
                t.add(f"{regime}.{'wide' if _keep is not None else 'ld_inner'}", fails, worst, _untouched(obuf, out), what)
    t.finish()


# ---- pack_rows ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,dim", ke.PACK_SHAPES)
def test_pack_rows_h(B, K, dim):
    """to the bit against torch.cat(...).half(), the cast specials (inf, NaN, values beyond 65504, subnormals) among the data"""
    lib = _lib.load()
    t = Tally(f"pack.B{B}.K{K}.d{dim}")
    q, ni, nt = kc.pack_inputs(B, K, dim, seed=1)
    R = B * (1 + 2 * K)
    obuf, out = _guarded(R, dim, HF)
    qd, nid, ntd = _operand(q), _operand(ni), _operand(nt)
    _done(lib.keds_knowledge_pack_rows_h(qd.data_ptr(), nid.data_ptr(), ntd.data_ptr(), out.data_ptr(), B, K, dim, _lib.stream()), "keds_knowledge_pack_rows_h")
    t.add("pack", *_one(kc.same_bits(out.cpu(), torch.cat([q, ni, nt]).half(), "pack")), _untouched(obuf, out), "pack")
    t.finish()


# ---- keds_crossformer_fuse_f16: concat_rows, fold_qo ----------------------------------------------------------------------------------------------
def _fuse_inputs_h(dim, inner, layers, regime, seed):
    """knowledge_check's cases with the weights as fp16 arrays"""
    return [{n: (v.half() if n[0] == "w" else v) for n, v in L.items()} for L in kc.fuse_inputs(dim, inner, layers, regime, seed)]


def _fuse_failures_h(R, got, exact, what):
    """knowledge_check.fuse_failures with fp16 in the place of bf16"""
    fs = [kc.same_bits(got["wkv"], R["wkv"], what + " wkv"), kc.same_bits(got["bkv"], R["bkv"], what + " bkv")]
    for l in R["wqn"]:
        (w, ew), (b, eb) = R["wqn"][l], R["bqn"][l]
        if exact:
            assert float(w.abs().max()) < 2048 and float(b.abs().max()) < 2 ** 24         # (integers an fp16 holds exactly)
            fs += [kc.same_bits(got["wqn"][l], w.half(), f"{what} wqn[{l}]"), kc.same_bits(got["bqn"][l], b.float(), f"{what} bqn[{l}]")]
        else:
            fs += [kc.held(got["wqn"][l], w, ew, HF, f"{what} wqn[{l}]"), kc.held(got["bqn"][l], b, eb, F32, f"{what} bqn[{l}]")]
    return [f for f in fs if f], max(f.worst for f in fs)


@pytest.mark.parametrize("dim,inner", kc.FUSE_SHAPES)
def test_crossformer_fuse_f16(dim, inner):
    lib = _lib.load()
    t = Tally(f"fuse.d{dim}.i{inner}")
    for layers in kc.FUSE_LAYERS:
        lay = kc.fuse_layout(dim, inner, layers)
        for regime in kc.FUSE_REGIMES:
            what = f"dim{dim}.inner{inner}.L{layers}.{regime}"
            Ls = _fuse_inputs_h(dim, inner, layers, regime, seed=3)
            p, keep = ke._xf_params(Ls, dim, inner // 64)
            assert lib.keds_crossformer_fused_bytes(C.byref(p)) == lay["total"], what
            buf, view = ke._bytes(lay["total"])
            fused = _lib.CrossFormerFused()
            _done(lib.keds_crossformer_fuse_f16(C.byref(p), view.data_ptr(), lay["total"], C.byref(fused), _lib.stream()), "keds_crossformer_fuse_f16")
            base, cpu = view.data_ptr(), view.cpu()
            gaps = torch.ones(lay["total"], dtype=torch.bool)

            def part(off_n, dtype, shape):
                off, n = off_n
                gaps[off:off + n] = False
                return cpu[off:off + n].view(dtype).reshape(shape)
            got = {"wkv": part(lay["wkv"], HF, (layers * 2 * inner, dim)), "bkv": part(lay["bkv"], F32, (layers * 2 * inner,)),
                   "wqn": {l: part(lay["wqn"][l], HF, (inner, inner)) for l in range(1, layers)},
                   "bqn": {l: part(lay["bqn"][l], F32, (inner,)) for l in range(1, layers)}}
            fails, worst = _fuse_failures_h(kc.fuse_reference(Ls), got, regime == "integer", what)
            ptrs_ok = fused.wkv == base + lay["wkv"][0] and fused.bkv == base + lay["bkv"][0] and fused.wqn[0] is None and fused.bqn[0] is None
            for l in range(1, 8):
                ptrs_ok &= fused.wqn[l] == (base + lay["wqn"][l][0] if l < layers else None)
                ptrs_ok &= fused.bqn[l] == (base + lay["bqn"][l][0] if l < layers else None)
            t.add(regime, fails, worst, ke._around(buf, lay["total"]) and bool((cpu[gaps] == ke.BYTE).all()) and bool(ptrs_ok), what)
    t.finish()


# ---- GEMM epilogues 32 - 34 ------------------------------------------------------------------------------------------------------------------
EPI = {32: "bias", 33: "relu", 34: "headf32"}
GEMM_M, GEMM_N, GEMM_K = (1, 127, 128, 129, 257), (128, 384), (64, 192, 768)
GEMM_REGIMES = gc.REGIMES[:4]                                   # (`offset` is for the LayerNorm-folded epilogues)
WS_BYTES = 32 << 20


@pytest.fixture(scope="module")
def gemm_state():
    """a split-K workspace and a registered guard flag (the thread's tower guard) for the GEMM tests; both restored afterwards"""
    lib = _lib.load()
    ws = torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(lib.keds_gemm_set_workspace(ws.data_ptr(), ws.numel()), "keds_gemm_set_workspace")
    _lib.check(lib.keds_numerics_guard_set(flag.data_ptr()), "keds_numerics_guard_set")
    try:
        yield flag
    finally:
        lib.keds_numerics_guard_set(None)
        old = _lib._gemm_ws.get(torch.cuda.current_device())
        lib.keds_gemm_set_workspace(old.data_ptr() if old is not None else None, old.numel() if old is not None else 0)
        _case.cache_clear()


@functools.lru_cache(maxsize=256)
def _case(M, N, K, regime):
    """one reference per (shape, regime), shared by the three epilogues, never written to"""
    return gc.Case(M, N, K, regime, HF, seed=1, device=DEV)


def _expected(case, fam, out_dtype=HF):
    """gemm_check.expected for the families of ids 32 - 34 (its table has no rows for them): pre = acc + bias, e = e_acc + 2 u32 (S +
    |bias|), zero in `integer`; ReLU is 1-Lipschitz"""
    pre = case.acc + case.bias.double()
    e = case.e_acc() if case.exact else case.e_acc() + 2 * gc.U32 * (case.S + case.bias.double().abs())
    return gc.Expected(pre.clamp_min(0.0) if fam == "relu" else pre, e, out_dtype, case.exact)


def _gemm(case, code, flag, plan_args):
    """-> (failures, worst ratio, guard violations, info of keds_gemm_last_launch)"""
    lib = _lib.load()
    M, N, K, fam = case.M, case.N, case.K, EPI[code]
    A = torch.full((M + GR, K), float("nan"), dtype=HF, device=DEV)            # a read behind row M poisons the output
    A[:M] = case.A
    obuf, out = _guarded(M, N, HF)
    head, aux, aux_i = None, None, 0
    if fam == "headf32":
        aux_i = min(M, 130)                                                     # head rows: across a 128-row tile edge
        head = torch.full((aux_i + GR, 3, N), SENT, dtype=F32, device=DEV)
        aux = head
    rc_ = lib.keds_gemm_bt_ex(P(A), K, P(case.W), P(case.bias), out.data_ptr(), N, M, N, K, code, P(aux), aux_i, _lib.stream())
    info, plan = (C.c_int * 8)(), (C.c_int * 8)()
    _lib.check(lib.keds_gemm_last_launch(info), "keds_gemm_last_launch")
    _done(rc_, f"keds_gemm_bt_ex({code}) {case.name}")
    _lib.check(lib.keds_gemm_plan_query(code, M, N, K, K, N, *plan_args, 0, plan), "keds_gemm_plan_query")
    bad = []
    if list(info) != list(plan):
        bad.append(f"launched {list(info)}, planned {list(plan)}")
    if info[0] != _lib.GEMM_FORM_SMALL or info[1] != _lib.GEMM_FORM_NONE:
        bad.append(f"not on the 128 x 128 form: {list(info)}")
    got = out.clone()
    fs = [gc.verify(got, _expected(case, fam), f"{case.name}.{code}")]
    if head is not None:
        if not (bool((head[:, 1:] == SENT).all()) and bool((head[aux_i:] == SENT).all())):
            bad.append("fp32 head: a slot other than [m < aux_i][0] written")
        fs.append(gc.verify(head[:aux_i, 0], _expected(case, fam, F32).first_rows(aux_i), f"{case.name}.{code}.head"))
    if not _untouched(obuf, out):
        bad.append("written outside the output rows")
    if int(flag.item()) != 0:
        bad.append("range guard raised on in-range values")
        flag.zero_()
    return [f for f in fs if f], max(f.worst for f in fs), bad, tuple(info)


@pytest.mark.parametrize("N", GEMM_N)
@pytest.mark.parametrize("M", GEMM_M)
def test_gemm_epilogues_32_to_34(gemm_state, M, N):
    """every id at every K and regime; the launch recorded by keds_gemm_last_launch is the plan's, on the 128 x 128 form"""
    t = Tally(f"gemm.M{M}.N{N}")
    forms = set()
    for K in GEMM_K:
        for regime in GEMM_REGIMES:
            case = _case(M, N, K, regime)
            for code in EPI:
                fails, worst, bad, info = _gemm(case, code, gemm_state, (0, WS_BYTES))
                forms.add(info[:6])
                t.add(f"{EPI[code]}.{regime}", fails, worst, not bad, f"{case.name}.{code}: {bad}")
    assert forms == {(_lib.GEMM_FORM_SMALL, 0, 4, 0, 1, 0)}, forms               # the one (form, ring, splits) the plan has at these shapes
    t.finish()


@pytest.mark.parametrize("M,N,K,ring,splits", [(128, 128, 2048, 4, 16), (257, 384, 2304, 4, 4), (128 * 86, 384, 64, 2, 1)])
def test_gemm_epilogues_32_to_34_on_the_plans_other_forms(gemm_state, M, N, K, ring, splits):
    """what the plan returns beyond those shapes: split-K through the reduce kernel (K >= 2048, few tiles) and the two-deep ring
    (more than 256 tiles)"""
    t = Tally(f"gemm_forms.M{M}.N{N}.K{K}")
    for regime in ("integer", "tail"):
        case = gc.Case(M, N, K, regime, HF, seed=2, device=DEV)
        for code in EPI:
            fails, worst, bad, info = _gemm(case, code, gemm_state, (0, WS_BYTES))
            if info[:6] != (_lib.GEMM_FORM_SMALL, 0, ring, 0, splits, 0):
                bad.append(f"form {info}")
            t.add(f"{EPI[code]}.{regime}", fails, worst, not bad, f"{case.name}.{code}: {bad}")
    t.finish()


# ---- the range flag --------------------------------------------------------------------------------------------------------------------------
def _flags():
    return torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)


def test_gemm_ids_raise_the_threads_guard_on_a_value_beyond_fp16(gemm_state):
    """like every fp16-storing epilogue of keds_hip.h: ONE output of 512 x 137 = 70,144 (or inf) raises the registered flag and is
    stored as inf; 512 x 117 = 59,904 does not"""
    lib = _lib.load()
    M = N = 128
    K = 64
    A = torch.zeros(M + GR, K, dtype=HF, device=DEV)
    A[77, 0] = 512.0
    for code in EPI:
        for w, want in ((117.0, 0), (137.0, 1), (float("inf"), 1)):
            W = torch.zeros(N, K, dtype=HF, device=DEV)
            W[5, 0] = w
            bias = torch.zeros(N, device=DEV)
            obuf, out = _guarded(M, N, HF)
            head = torch.zeros(M, 3, N, device=DEV)
            _done(lib.keds_gemm_bt(P(A), P(W), P(bias), out.data_ptr(), M, N, K, code, P(head) if code == 34 else None, M if code == 34 else 0,
                                   _lib.stream()), f"keds_gemm_bt({code})")
            assert int(gemm_state.item()) == want, (code, w)
            gemm_state.zero_()
            assert float(out[77, 5]) == (float("inf") if want else 59904.0)
            if w == 137.0:
                got = out.clone()
                got[77, 5] = 0
                assert not bool(got.any())                                          # every other output is the zero it should be
            assert _untouched(obuf, out)


def _tiny_stream(lib, fused):
    S = ke.Stream(128, 2, 2, 128, seed=5)
    kp, T = _params_h(S, lib, fused)
    return S, kp, T


def _params_h(S, lib, fused):
    """ke.Stream.params with the weights as fp16 arrays, fused by keds_crossformer_fuse_f16"""
    i2t = _lib.Im2TextParams()
    i2t.dim_in, i2t.middle, i2t.dim_out, i2t.n_layer = S.dim, S.middle, S.dim, 2
    T = {}
    for i, (w, b) in enumerate(S.i2t):
        T[f"w{i}"], T[f"b{i}"] = S._dev(w, HF), S._dev(b, F32)
        i2t.w[i], i2t.b[i] = T[f"w{i}"].data_ptr(), T[f"b{i}"].data_ptr()
    T["ow"], T["ob"] = S._dev(S.i2t_out[0], HF), S._dev(S.i2t_out[1], F32)
    i2t.out_w, i2t.out_b = T["ow"].data_ptr(), T["ob"].data_ptr()
    xfs = []
    for which, Ls in enumerate(S.xf):
        arr = (_lib.CrossLayerParams * S.layers)()
        for l, L in enumerate(Ls):
            for n, v in L.items():
                T[f"x{which}.{l}.{n}"] = S._dev(v.float(), HF if n[0] == "w" else F32)
                setattr(arr[l], n, T[f"x{which}.{l}.{n}"].data_ptr())
        p = _lib.CrossFormerParams(S.dim, S.heads, S.layers, arr, None)
        S.keep.append(arr)
        if fused:
            total = lib.keds_crossformer_fused_bytes(C.byref(p))
            buf, view = ke._bytes(total)
            fz = _lib.CrossFormerFused()
            _done(lib.keds_crossformer_fuse_f16(C.byref(p), view.data_ptr(), total, C.byref(fz), _lib.stream()), "keds_crossformer_fuse_f16")
            S.keep += [fz, buf]
            p.fused = C.pointer(fz)
            T[f"x{which}.fused"] = fz
        xfs.append(p)
    return _lib.KnowledgeParams(i2t, xfs[0], xfs[1]), T


@pytest.mark.parametrize("fused", (True, False))
def test_a_value_of_70000_raises_range_flag_and_leaves_the_tower_guard(fused):
    """in each entry that takes range_flag: an input of 70,000 is stored as fp16 inf by the pack (or the cast) -- the call's flag goes
    up, the registered tower guard's flag stays 0 and is still the thread's guard afterwards (a GEMM that stores an fp16 inf then
    raises IT); in-range inputs leave both flags at 0; a null range_flag is accepted"""
    lib = _lib.load()
    S, kp, T = _tiny_stream(lib, fused)
    B, K, dim = 3, 4, S.dim
    tower, flag = _flags()
    _lib.check(lib.keds_numerics_guard_set(tower.data_ptr()), "keds_numerics_guard_set")
    try:
        ws = torch.zeros(lib.keds_knowledge_f16_workspace_bytes(C.byref(kp), B, K) + 256, dtype=torch.uint8, device=DEV)
        xws = torch.zeros(lib.keds_crossformer_workspace_bytes(C.byref(kp.fuse), B, K) + 256, dtype=torch.uint8, device=DEV)
        iws = torch.zeros(lib.keds_im2text_workspace_bytes(C.byref(kp.i2t), B) + 256, dtype=torch.uint8, device=DEV)
        out, xo = torch.zeros(B, 3, dim, device=DEV), torch.zeros(B, dim, device=DEV)
        for big in (False, True):
            q, ni, nt = ke._inputs(S, B, K, seed=4)
            if big:
                ni[5, 17] = 70000.0
                q[1, 3] = 70000.0
            calls = (
                ("keds_knowledge_run_f16", lambda f: lib.keds_knowledge_run_f16(C.byref(kp), P(q), P(ni), P(nt), B, K, P(out), P(ws), ws.numel(), f, _lib.stream())),
                ("keds_crossformer_forward_f16", lambda f: lib.keds_crossformer_forward_f16(C.byref(kp.fuse), P(q), P(ni), P(ni), B, K, P(xo), P(xws), xws.numel(), f, _lib.stream())),
                ("keds_im2text_forward_f16", lambda f: lib.keds_im2text_forward_f16(C.byref(kp.i2t), P(q), B, P(xo), P(iws), iws.numel(), f, _lib.stream())))
            for name, call in calls:
                _done(call(flag.data_ptr()), name)
                assert int(flag.item()) == int(big), (name, big)
                assert int(tower.item()) == 0, f"{name}: the tower guard's flag was written"
                flag.zero_()
                _done(call(None), name + " (null range_flag)")
                assert int(flag.item()) == 0 and int(tower.item()) == 0, name
        # the thread's guard is the tower's again: an fp16-storing GEMM outside the stream raises it
        W = torch.zeros(128, 64, dtype=HF, device=DEV)
        A = torch.zeros(128 + GR, 64, dtype=HF, device=DEV)
        bias = torch.full((128,), 70000.0, device=DEV)
        o = torch.zeros(128 + GR, 128, dtype=HF, device=DEV)
        _done(lib.keds_gemm_bt(P(A), P(W), P(bias), P(o), 128, 128, 64, _lib.EPI_BIAS_F16_H, None, 0, _lib.stream()), "keds_gemm_bt")
        assert int(tower.item()) == 1 and int(flag.item()) == 0
    finally:
        lib.keds_numerics_guard_set(None)


def test_pack_rows_h_raises_the_threads_guard():
    """the stand-alone pack has no range_flag argument: like the GEMM ids it reports to the thread's guard, and to nobody without one"""
    lib = _lib.load()
    B, K, dim = 2, 3, 128
    q, ni, nt = (torch.randn(n, dim, device=DEV) for n in (B, B * K, B * K))
    rows = torch.zeros(B * (1 + 2 * K), dim, dtype=HF, device=DEV)
    tower = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(lib.keds_numerics_guard_set(tower.data_ptr()), "keds_numerics_guard_set")
    try:
        _done(lib.keds_knowledge_pack_rows_h(P(q), P(ni), P(nt), P(rows), B, K, dim, _lib.stream()), "keds_knowledge_pack_rows_h")
        assert int(tower.item()) == 0
        nt[-1, -1] = -70000.0
        _done(lib.keds_knowledge_pack_rows_h(P(q), P(ni), P(nt), P(rows), B, K, dim, _lib.stream()), "keds_knowledge_pack_rows_h")
        assert int(tower.item()) == 1 and float(rows[-1, -1]) == float("-inf")
    finally:
        lib.keds_numerics_guard_set(None)
    _done(lib.keds_knowledge_pack_rows_h(P(q), P(ni), P(nt), P(rows), B, K, dim, _lib.stream()), "keds_knowledge_pack_rows_h")
