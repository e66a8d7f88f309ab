"""The image preprocessing kernels alone at their edges (keds_amd/csrc/elementwise.hip): keds_preprocess_pil against PIL itself, byte for
byte on the uint8 image and bit for bit on the normalised floats; keds_preprocess against the float64 set of its own definition.
tests/preprocess_check.py holds the references, the regimes and the derivation of the set; tests/test_host_preprocess_check.py shows that
the checks pass models of the kernels and catch their mutations.

Every output -- the u8 image too -- sits in a sentinel-filled buffer with 256 guard elements on both sides; a refused call leaves every
buffer as it was."""
import ctypes as C

import numpy as np
import pytest
import torch

from keds_amd import _lib, ops
from tests import preprocess_check as pc
from tests.gpu_util import report

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = 256
SENTF = 7.25
SENT8 = 0xA5


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
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _f3(v):
    return (C.c_float * 3)(*v)


def _call_pil(img, n_px, a, with_u8=True, out=None, u8=None):
    """keds_preprocess_pil with the arguments `a` (preprocess_check.pil_args / one_pass_args) -> the return code"""
    B, H, W, _ = img.shape
    t = {k: _dev(a[k]) for k in ("xb", "xk", "yb", "yk")}
    d_img = _dev(img)
    ksx = 0 if a["xk"] is None else a["xk"].shape[1]
    ksy = 0 if a["yk"] is None else a["yk"].shape[1]
    rc = _lib.load().keds_preprocess_pil(_lib.ptr(d_img), B, H, W, n_px, int(a["need_h"]), int(a["need_v"]), a["left"], a["top"],
                                         _lib.ptr(t["xb"]), _lib.ptr(t["xk"]), ksx, _lib.ptr(t["yb"]), _lib.ptr(t["yk"]), ksy, _f3(pc.MEAN),
                                         _f3(pc.STD), out.data_ptr(), u8.data_ptr() if with_u8 else None, _lib.stream())
    torch.cuda.synchronize()
    return rc


def _run_pil(img, n_px, a, want, what):
    """both forms of the call (with and without the u8 output) in guarded buffers -> (failures, outputs compared by bits)"""
    B = img.shape[0]
    msgs, words = [], 0
    for with_u8 in (True, False):
        wO, out = _buf(B * 3 * n_px * n_px, torch.float32, SENTF)
        wU, u8 = _buf(B * n_px * n_px * 3, torch.uint8, SENT8)
        _done(_call_pil(img, n_px, a, with_u8, out, u8), "keds_preprocess_pil")
        msgs += pc.pil_failures(want, out.cpu().numpy(), u8.cpu().numpy() if with_u8 else None, what=f"{what}u8 {with_u8}: ")
        words += int(want.size) * (2 if with_u8 else 1)
        if not (_guards_ok(wO, SENTF) and _guards_ok(wU, SENT8)):
            msgs.append(f"{what}written outside an output buffer")
        if not with_u8 and not bool((wU == SENT8).all()):
            msgs.append(f"{what}the u8 buffer was written without being passed")
    return msgs, words


@pytest.mark.parametrize("H,W,n_px", pc.OPS_CASES)
def test_preprocess_pil_equals_pil(H, W, n_px):
    """the five regimes as one batch of five different images, then batches of 1 and 3 (and 4 at n_px = 8: 192 and 256 threads, below and
    exactly one workgroup), with the arguments ops.preprocess builds; ops.preprocess itself returns the same bits"""
    img = pc.batch(H, W)
    want = np.stack([pc.pil_reference(x, n_px) for x in img])
    a = pc.pil_args(H, W, n_px)
    msgs, words = [], 3 * int(want.size)
    for idx in ([0, 1, 2, 3, 4], [0], [4, 0, 3]) + (([3, 0, 4, 1],) if n_px == 8 else ()):
        m, w = _run_pil(img[idx], n_px, a, want[idx], f"images {idx}: ")
        msgs, words = msgs + m, words + w
    got, got_u8 = ops.preprocess(torch.from_numpy(img).to(DEV), n_px, return_u8=True)
    msgs += pc.pil_failures(want, got.cpu().numpy(), got_u8.cpu().numpy(), what="ops.preprocess: ")
    only = ops.preprocess(torch.from_numpy(img).to(DEV), n_px)
    msgs += pc.pil_failures(want, only.cpu().numpy(), None, what="ops.preprocess without u8: ")
    report(f"preprocess_edges.pil.{H}x{W}.{n_px}", compared_by_bits=words, failures=len(msgs))
    assert not msgs, "\n".join(msgs[:20])


@pytest.mark.parametrize("axis,offset", pc.ONE_PASS_CASES)
def test_preprocess_pil_one_pass_and_squash(axis, offset):
    """what only a C host reaches: one pass resampled, the other axis cropped at `offset` (0, and the last window that fits); and the
    300 x 37 image squashed to 28 x 28 (45 taps)"""
    args, size, box = pc.one_pass_args(axis, offset)
    img = pc.batch(*pc.one_pass_image_size(axis))
    want = np.stack([pc.pil_resize_crop(x, size, box) for x in img])
    msgs, words = _run_pil(img, pc.ONE_PASS_N, args, want, f"{axis} {offset}: ")
    report(f"preprocess_edges.pil_one_pass.{axis}.{offset}", compared_by_bits=words, failures=len(msgs))
    assert not msgs, "\n".join(msgs[:20])


def test_preprocess_pil_refusals_leave_the_outputs_intact():
    H, W, n = pc.ONE_PASS_H, pc.ONE_PASS_W, pc.ONE_PASS_N
    img = pc.batch(H, W)[:2]
    both = pc.pil_args(H, W, n)
    h_only, v_only = pc.one_pass_args("h", 0)[0], pc.one_pass_args("v", 0)[0]
    cases = [("the horizontal pass without its tables", dict(both, xb=None, xk=None)),
             ("the vertical pass without its weights", dict(both, yk=None)),
             ("a negative left", dict(v_only, left=-1)), ("a negative top", dict(h_only, top=-1)),
             ("a skipped horizontal pass whose window leaves the image", dict(v_only, left=W - n + 1)),
             ("a skipped vertical pass whose window leaves the image", dict(h_only, top=H - n + 1)),
             ("no pass and a window outside", dict(need_h=False, need_v=False, left=0, top=H - n + 1, xb=None, xk=None, yb=None, yk=None))]
    for name, a in cases:
        wO, out = _buf(2 * 3 * n * n, torch.float32, SENTF)
        wU, u8 = _buf(2 * n * n * 3, torch.uint8, SENT8)
        rc = _call_pil(img, n, a, True, out, u8)
        assert rc != 0, f"keds_preprocess_pil accepted {name}"
        assert bool((wO == SENTF).all()) and bool((wU == SENT8).all()), f"written after refusing {name}"
    for a in (dict(v_only, left=W - n), dict(h_only, top=H - n)):  # the last windows that fit are accepted
        wO, out = _buf(2 * 3 * n * n, torch.float32, SENTF)
        wU, u8 = _buf(2 * n * n * 3, torch.uint8, SENT8)
        _done(_call_pil(img, n, a, True, out, u8), "keds_preprocess_pil")
        assert _guards_ok(wO, SENTF) and _guards_ok(wU, SENT8)


@pytest.mark.parametrize("H,W,n_px,regimes", pc.F32_CASES)
def test_preprocess_f32_weights_within_the_set_of_its_definition(H, W, n_px, regimes):
    """keds_preprocess: the value recovered from every output lies in the set the float64 evaluation of the kernel's definition allows, the
    float within 4 u (v / 255 + |m|) / |s| of that value's normalisation; the share of outputs that differ from PIL's is reported"""
    img = pc.batch(H, W, regimes)
    allowed = pc.f32_allowed(img, n_px)
    want = np.stack([pc.pil_reference(x, n_px) for x in img])
    msgs = []
    for idx in (list(range(len(regimes))), [0]):
        B = len(idx)
        wO, out = _buf(B * 3 * n_px * n_px, torch.float32, SENTF)
        d_img = _dev(img[idx])
        _done(_lib.load().keds_preprocess(_lib.ptr(d_img), B, H, W, n_px, _f3(pc.MEAN), _f3(pc.STD), out.data_ptr(), _lib.stream()),
              "keds_preprocess")
        got = out.cpu().numpy().reshape(B, 3, n_px, n_px)
        m, share, v = pc.f32_failures(img[idx], n_px, got, allowed=(allowed[0][idx], allowed[1][idx]), what=f"images {idx}: ")
        msgs += m + ([] if _guards_ok(wO, SENTF) else [f"images {idx}: written outside the output buffer"])
        if B > 1:
            differs = v != want[idx]
            report(f"preprocess_edges.f32.{H}x{W}.{n_px}", ambiguous_share=share, differs_from_pil=float(differs.mean()),
                   largest_step=int(np.abs(v - want[idx].astype(np.int64)).max()), outputs=int(v.size))
    assert not msgs, "\n".join(msgs[:20])
