"""Both MXFP8 GEMM kernels per ELEMENT, at their tile, K and block-scale edges (tests/mx_check.py: the cases, the float64 reference, the
bound and the MX-output checks; tests/test_host_mx_check.py: proof that they catch a stale K-tile in one 8-row piece, a scale byte of
the neighbouring block or row, side data of the previous tile, two interchanged MX blocks, a block exponent one too small, ...).

All calls go through keds_gemm_mxfp8_ex on operands built directly in the kernels' format; every case asserts the kernel form, grid
and tile count that keds_gemm_mxfp8_last_launch recorded (and that keds_gemm_mxfp8_plan_query plans the same for this device), so a shape
the dispatcher sends elsewhere fails instead of testing the wrong kernel.  Outputs, the MX copy [q_pad = M + 256, N], its scale bytes, the statistics and the statistics buffer to clear sit in
sentinel-filled buffers with 256 guard rows that must survive; the operands' scale slabs carry pad rows with a gross scale (every
regime but `random`), the operands themselves NaN guard rows.  One reference per (shape, regime) is shared by all epilogues and
forms.  Each test collects every failure before it asserts; the worst bound ratio per (form, epilogue, regime) goes to the metrics log."""
import ctypes
import functools

import pytest
import torch

from keds_amd import _lib
from tests import gemm_check as gc
from tests import mx_check as mc
from tests.gpu_util import report

pytestmark = pytest.mark.gpu

GUARD = 256
SENT = gc.SENTINEL
STAT_BASE = (3 << 28, 11 << 28)               # what the statistics a launch ADDS INTO hold before it
STAT_GUARD = 7
PAIR, QUAD = _lib.FP8_FORM_PAIR, _lib.FP8_FORM_QUAD
QUAD_EPIS = (mc.EPI_BIAS, mc.EPI_LN, mc.EPI_LN_QGELU_MX, mc.EPI_RESID_MX_H)      # the fp32-residual epilogue stays on 8 waves
ALL_EPIS = tuple(mc.NAMES)
SHAPES = [(256, 256), (768, 256), (256, 768), (2304, 256), (512, 1024)]          # 1, 3, 3, 9 (no multiple of 8: the XCD remap) and 8 tiles
SHAPE_IDS = [f"{m}x{n}" for m, n in SHAPES]


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    try:
        yield
    finally:
        _lib.load().keds_mxfp8_debug(0)
        _case.cache_clear()
        _big_case.cache_clear()


@functools.lru_cache(maxsize=256)
def _case(M, N, K, regime):
    """one reference per (shape, regime), shared by every epilogue and form, never written to"""
    return mc.MxCase(M, N, K, regime, seed=1, device="cuda")


@functools.lru_cache(maxsize=2)
def _big_case(M, N, K, regime, alt):
    return mc.MxCase(M, N, K, regime, seed=1, device="cuda", row_alt=alt)


def _threshold():
    """tiles beyond which the 4-wave kernel goes persistent: min(CUs, 256) & ~7"""
    return min(torch.cuda.get_device_properties(0).multi_processor_count, 256) & ~7


def _sent(t, value):
    return bool((t == torch.tensor(value, dtype=t.dtype, device=t.device)).all())


def _operands(case):
    """the case's operands in device buffers (cached on the case; no launch writes them): bytes with NaN guard rows, scale slabs with
    pad rows (PAD_SCALE) in every regime but `random`"""
    ops = case.__dict__.get("_gpu_ops")
    if ops is None:
        pad = 0 if case.regime == "random" else 1
        m_pad, n_pad = case.M + 8 * pad, case.N + 12 * pad
        aq = torch.full((case.M + GUARD, case.K), mc.NAN_BYTE, dtype=torch.uint8, device="cuda")
        aq[:case.M] = case.aq
        wq = torch.full((case.N + GUARD, case.K), mc.NAN_BYTE, dtype=torch.uint8, device="cuda")
        wq[:case.N] = case.wq
        ops = case.__dict__["_gpu_ops"] = (aq, case.a_scales(m_pad), m_pad, wq, case.w_scales(n_pad), n_pad)
    return ops


def _launch(case, epi, debug=0):
    """-> (res for mx_check.model_failures, info of keds_gemm_mxfp8_last_launch, list of guard violations)"""
    lib = _lib.load()
    M, N = case.M, case.N
    P = _lib.ptr
    aq, as_, m_pad, wq, ws, n_pad = _operands(case)
    od = {mc.EPI_BIAS: gc.BF, mc.EPI_LN: gc.BF, mc.EPI_RESID_MX: gc.F32, mc.EPI_RESID_MX_H: gc.HF}.get(epi)
    out = q = qs = stats_in = other = stats = keep = None
    q_pad = 0
    if od is not None:
        out = torch.full((M + GUARD, N), SENT, dtype=od, device="cuda")
        if epi in (mc.EPI_RESID_MX, mc.EPI_RESID_MX_H):
            out[:M] = case.resid.to(od)
    if epi in mc.MX_EPIS:
        q_pad = M + GUARD
        q = torch.full((q_pad, N), mc.NAN_BYTE, dtype=torch.uint8, device="cuda")
        qs = torch.full((N // 128, q_pad, 4), mc.PAD_SCALE, dtype=torch.uint8, device="cuda")
    bias = None if case.name.endswith(".nobias") else case.bias
    aux = aux2 = None
    if epi in mc.LN_EPIS:
        bias = torch.cat([case.bias, case.csum])
        stats_in = torch.full((M + GUARD, 2), STAT_GUARD, dtype=torch.int64, device="cuda")
        stats_in[:M] = case.stats
        other = torch.full((M + GUARD, 2), STAT_GUARD, dtype=torch.int64, device="cuda")
        keep = stats_in.clone()
        aux, aux2 = stats_in, other
    elif epi in (mc.EPI_RESID_MX, mc.EPI_RESID_MX_H):
        stats = torch.tensor(STAT_BASE, dtype=torch.int64, device="cuda").repeat(M + GUARD, 1)
        aux = stats
    info = (ctypes.c_int * 4)()
    lib.keds_mxfp8_debug(debug)
    try:
        rc = lib.keds_gemm_mxfp8_ex(P(aq), P(as_), m_pad, P(wq), P(ws), n_pad, P(bias), P(out), M, N, case.K, epi, P(aux), P(aux2), P(q), P(qs),
                                    q_pad, _lib.stream())
        _lib.check(lib.keds_gemm_mxfp8_last_launch(info), "keds_gemm_mxfp8_last_launch")
        plan = (ctypes.c_int * 4)()            # ... and what the planner says of this call on this device, under the same debug value
        _lib.check(lib.keds_gemm_mxfp8_plan_query(epi, M, N, case.K, torch.cuda.get_device_properties(0).multi_processor_count, plan),
                   "keds_gemm_mxfp8_plan_query")
    finally:
        lib.keds_mxfp8_debug(0)
    try:
        _lib.check(rc, f"keds_gemm_mxfp8_ex({mc.NAMES[epi]})")
        torch.cuda.synchronize()
    except RuntimeError as e:             # a failed launch or a device fault: nothing more of this session may run on the card
        pytest.exit(f"{case.name} {mc.NAMES[epi]} debug={debug}: {e}", returncode=3)
    bad, res = [], {}
    if tuple(info) != tuple(plan):
        bad.append(f"recorded (form, grid, tiles, persistent) {tuple(info)} is not the plan {tuple(plan)}")
    if out is not None:
        if not _sent(out[M:], SENT):
            bad.append("output rows >= M written")
        res["out"] = out
    if q is not None:
        if not _sent(q[M:], mc.NAN_BYTE):
            bad.append("MX copy rows >= M written")
        if not _sent(qs[:, M:, :], mc.PAD_SCALE):
            bad.append("MX scale bytes of rows >= M (the slabs' padding) written")
        res["q"], res["qexp"] = q, mc.unpack_scales(qs, M)
    if other is not None:
        if not (_sent(other[:M], 0) and _sent(other[M:], STAT_GUARD)):
            bad.append("the statistics buffer to clear: not exactly rows < M cleared")
        if not torch.equal(stats_in, keep):
            bad.append("the statistics a LayerNorm epilogue reads were written")
    if stats is not None:
        base = torch.tensor(STAT_BASE, dtype=torch.int64, device="cuda")
        if not bool((stats[M:] == base).all()):
            bad.append("statistics of rows >= M added to")
        res["stats"] = stats[:M] - base
    return res, tuple(info), bad


class Tally:
    """failures of a whole test, and the worst ratio per (epilogue, regime)"""

    def __init__(self, label):
        self.label, self.msgs, self.worst, self.launches = label, [], {}, 0

    def run(self, case, epi, form, persistent=False, debug=0, twice=False):
        res, info, bad = _launch(case, epi, debug)
        self.launches += 1
        name = f"{self.label}.{case.name}.{mc.NAMES[epi]}"
        tiles = (case.M // 256) * (case.N // 256)
        want = (form, _threshold() if persistent else tiles, tiles, int(persistent))
        if info != want:
            self.msgs.append(f"{name}: recorded (form, grid, tiles, persistent) {info}, wanted {want}")
        self.msgs += [f"{name}: {b}" for b in bad]
        fails, worst = mc.model_failures(case, epi, res)
        self.msgs += [str(f) for f in fails]
        key = (mc.NAMES[epi], case.regime)
        self.worst[key] = max(self.worst.get(key, 0.0), worst)
        if twice:                                                           # integer atomics: the same bits on a second run
            res2, _, _ = _launch(case, epi, debug)
            for k in res:
                if not torch.equal(res[k], res2[k]):
                    self.msgs.append(f"{name}: `{k}` differs between two runs")

    def sweep(self, case_of, epis, Ks, form, persistent=False, debug=0, regimes=None):
        """every K x every regime of the epilogue; one reference at a time serves all its epilogues.  `random` also runs BIAS_BF16
        without a bias; the residual epilogues run `random` twice"""
        for K in Ks:
            for regime in (regimes or mc.REGIMES):
                for epi in (e for e in epis if regime in mc.regimes_of(e)):
                    case = case_of(K, regime)
                    self.run(case, epi, form, persistent, debug, twice=regime == "random" and epi in (mc.EPI_RESID_MX, mc.EPI_RESID_MX_H))
                    if regime == "random" and epi == mc.EPI_BIAS:
                        self.run(case.without_bias(), epi, form, persistent, debug)

    def finish(self):
        for (epi, regime), w in sorted(self.worst.items()):
            report(f"mx_gemm_edges.{self.label}.{epi}.{regime}", worst_ratio=w)
        assert self.launches > 0
        assert not self.msgs, f"{len(self.msgs)} failures:\n" + "\n".join(self.msgs[:30])


# ---- 8 waves ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", SHAPES, ids=SHAPE_IDS)
def test_eight_wave_kernel_by_shape(M, N):
    """K < 512 or K % 256 != 0 (two, three and five K-tiles) for every epilogue; the fp32-residual epilogue at any K (four and eight
    K-tiles too)"""
    t = Tally("pair8")
    t.sweep(lambda K, regime: _case(M, N, K, regime), ALL_EPIS, (256, 384, 640), PAIR)
    t.sweep(lambda K, regime: _case(M, N, K, regime), (mc.EPI_RESID_MX,), (512, 1024), PAIR)
    t.finish()


@pytest.mark.parametrize("M,N", [(768, 256), (512, 1024)], ids=["768x256", "512x1024"])
def test_eight_wave_kernel_forced_at_the_four_wave_shapes(M, N):
    """keds_mxfp8_debug(16): four, six and 32 K-tiles on the 8-wave kernel (the reference of the bit-identity test)"""
    t = Tally("pair8.forced")
    t.sweep(lambda K, regime: _case(M, N, K, regime), ALL_EPIS, (512, 768, 4096), PAIR, debug=16)
    t.finish()


# ---- 4 waves ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", SHAPES, ids=SHAPE_IDS)
def test_four_wave_kernel_one_tile_per_workgroup(M, N):
    """by shape, tiles <= T: four (the shortest K-loop: two opening and two closing steps), six, eight and ten K-tiles; 32 once"""
    assert (M // 256) * (N // 256) <= _threshold()
    t = Tally("quad4")
    t.sweep(lambda K, regime: _case(M, N, K, regime), QUAD_EPIS, (512, 768, 1024, 1280), QUAD)
    if (M, N) == (512, 1024):
        t.sweep(lambda K, regime: _case(M, N, K, regime), QUAD_EPIS, (4096,), QUAD)
    t.finish()


def _persistent_shapes():
    """(label, M, N): T + 1 tiles (one workgroup walks two tiles; a single tile column), 1.5 T (a ragged second round, supertiles of
    8 x 4), 2 T + 8 (a third round of 8 tiles)"""
    th = _threshold()
    return [("plus1", (th + 1) * 256, 256), ("ragged", 3 * th // 8 * 256, 1024), ("two_rounds_plus8", (2 * th + 8) * 256, 256)]


PERSIST_REGIMES = ("integer_pow2", "random", "blockramp_up", "blockramp_down", "blockjump", "offset")
ALT = ("blockramp_up", "blockramp_down", "offset")       # with the row scale that alternates by 2^6 every 256 rows


@pytest.mark.parametrize("which", range(3), ids=["plus1", "ragged", "two_rounds_plus8"])
def test_four_wave_persistent_kernel(which):
    """by shape, tiles > T.  blockramp and offset carry a row scale that alternates by 2^6 from one 256-row tile to the next: a tile
    that starts from its predecessor's K-tiles 0 / 1 or side data fails grossly.  Four and six K-tiles; eight once, on the LayerNorm
    and fp16-residual epilogues."""
    label, M, N = _persistent_shapes()[which]
    assert (M // 256) * (N // 256) > _threshold() >= 8, "not a persistent launch on this device"
    t = Tally(f"quad4.persistent.{label}")
    t.sweep(lambda K, regime: _big_case(M, N, K, regime, regime in ALT), QUAD_EPIS, (512, 768), QUAD, persistent=True, regimes=PERSIST_REGIMES)
    if label == "ragged":
        t.sweep(lambda K, regime: _big_case(M, N, K, regime, regime in ALT), (mc.EPI_LN, mc.EPI_LN_QGELU_MX, mc.EPI_RESID_MX_H), (1024,), QUAD,
                persistent=True, regimes=("blockramp_down", "offset", "integer_pow2"))
    t.finish()
