"""keds_gemm_f32 (gemm_f32_kernel of f32path.hip: the f32-input matrix instruction, 128 x 128 x 16 tiles through registers and a
k-major LDS image) per ELEMENT at its tile and K edges (tests/gemm_check.py: Case with fp32 operands, F32_EPILOGUES, the float64
reference and the bound; tests/test_host_gemm_check.py: the CPU model with K-tiles of 16 and its mutations).

A sits in a NaN-filled buffer with 256 guard rows and, where lda > K, NaN behind column K; the output in a sentinel-filled buffer with
256 guard rows and, where ldc > N, guard columns: all of it must survive.  K = 16 is a single K-tile (no prefetch, no second LDS
buffer); M runs over the 32-, 64- and 128-row edges of the wave and workgroup tiles.  All five epilogues, with a bias and with
bias = NULL; `integer` cases of the linear epilogues with torch.equal.  One float64 reference per (shape, regime) is computed on the
GPU and shared; every element of every launch is compared."""
import functools

import pytest
import torch

from keds_amd import _lib
from tests import gemm_check as gc
from tests.gpu_util import report

pytestmark = pytest.mark.gpu

GUARD = 256
SENT = gc.SENTINEL
CODES = tuple(gc.F32_EPILOGUES)
SHAPE_M = (1, 7, 63, 64, 65, 127, 128, 129, 257)
SHAPE_N = (128, 384)
SHAPE_K = (16, 32, 48, 64, 1024)
STRIDES = ((0, 0), (8, 12), (8, 0), (0, 12))          # (lda - K, ldc - N)


@functools.lru_cache(maxsize=4096)
def _case(M, N, K, regime):
    """one reference per (shape, regime), shared by every epilogue, never written to"""
    return gc.Case(M, N, K, regime, gc.F32, seed=1, device="cuda")


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    try:
        yield
    finally:
        _case.cache_clear()


def _is_sent(t):
    return bool((t == SENT).all())


def _launch(case, code, bias, lda, ldc):
    """-> (res for gemm_check.model_failures, list of guard violations)"""
    lib = _lib.load()
    M, N, K = case.M, case.N, case.K
    fam = gc.F32_EPILOGUES[code][2]
    P = _lib.ptr
    A = torch.full((M + GUARD, lda), float("nan"), dtype=torch.float32, device="cuda")       # a read behind row M or column K poisons the output
    A[:M, :K] = case.A
    orows = (case.patch_out_rows() if fam == "patch" else M) + GUARD
    out = torch.full((orows, ldc), SENT, dtype=torch.float32, device="cuda")
    if fam == "resid":
        out[:M, :N] = case.resid
    aux, aux_i = (case.pos, gc.PATCH_G) if fam == "patch" else (None, 0)
    rc = lib.keds_gemm_f32(P(A), lda, P(case.W), P(case.bias) if bias else None, P(out), ldc, M, N, K, code, P(aux), aux_i, _lib.stream())
    try:
        _lib.check(rc, f"keds_gemm_f32({gc.F32_NAMES[code]})")
        torch.cuda.synchronize()
    except RuntimeError as e:             # a failed launch or a device fault: nothing more of this session may run on the card
        pytest.exit(f"{case.name} {gc.F32_NAMES[code]} lda={lda} ldc={ldc}: {e}", returncode=3)
    bad = []
    if fam == "patch":
        written = torch.zeros(orows, dtype=torch.bool, device="cuda")
        written[case.patch_rows()] = True
        if not _is_sent(out[~written]):
            bad.append("a class-token row or a guard row of the PATCH output was written")
    elif not _is_sent(out[M:]):
        bad.append("output rows >= M written")
    if ldc > N and not _is_sent(out[:, N:]):
        bad.append("guard columns n >= N written")
    return {"out": out[:, :N]}, bad


@pytest.mark.parametrize("bias", (True, False), ids=["bias", "null_bias"])
@pytest.mark.parametrize("code", CODES, ids=[gc.F32_NAMES[c] for c in CODES])
def test_gemm_f32_every_shape_regime_and_stride(code, bias):
    """M over the 32- / 64- / 128-row edges x N = 128, 384 x K = one, two, three, four and sixty-four K-tiles, every regime, dense and
    padded strides (lda in {K, K + 8} x ldc in {N, N + 12}).
    PATCH: G = 7 (images straddle the 32-, 64- and 128-row edges; class-token rows and guard rows keep the sentinel; pos is read
    with stride N whatever ldc).  RESID runs in place and leaves rows >= M untouched."""
    msgs, worst, n = [], {}, 0
    for N in SHAPE_N:
        for M in SHAPE_M:
            for K in SHAPE_K:
                for regime in gc.F32_REGIMES:
                    base = _case(M, N, K, regime)
                    case = base if bias else base.without_bias()
                    for da, dc in STRIDES:
                        res, bad = _launch(case, code, bias, K + da, N + dc)
                        name = f"{case.name}.{gc.F32_NAMES[code]}.lda+{da}.ldc+{dc}"
                        msgs += [f"{name}: {b}" for b in bad]
                        fails, w = gc.model_failures(case, code, res)
                        msgs += [f"{name}: {f}" for f in fails]
                        worst[regime] = max(worst.get(regime, 0.0), w)
                    n += 1
    for regime, w in sorted(worst.items()):
        report(f"f32_edges.{gc.F32_NAMES[code]}.{'bias' if bias else 'null_bias'}.{regime}", worst_ratio=w)
    assert n == len(SHAPE_N) * len(SHAPE_M) * len(SHAPE_K) * len(gc.F32_REGIMES)
    assert not msgs, f"{len(msgs)} failures:\n" + "\n".join(msgs[:30])
