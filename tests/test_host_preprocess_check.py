"""Proof, on the CPU, that the checks of the image preprocessing (tests/preprocess_check.py) pass models of the two kernels -- an integer
model of preprocess_pil_kernel, which must equal PIL byte for byte, and a float32 model of preprocess_kernel, held to the float64 set of its
own definition -- on every case and in every regime, that every mutation of the models fails wherever it changes anything, and what the
earlier test's regime (smooth content + noise at 224) shows of the clip8 and shift mutations."""
import functools

import numpy as np
import pytest

from keds_amd import clip as kclip
from keds_amd import ops
from tests import preprocess_check as pc


@functools.lru_cache(maxsize=None)
def _ops_case(H, W, n_px):
    img = pc.batch(H, W)
    return img, pc.pil_args(H, W, n_px), np.stack([pc.pil_reference(x, n_px) for x in img])


@functools.lru_cache(maxsize=None)
def _one_pass_case(axis, offset):
    args, size, box = pc.one_pass_args(axis, offset)
    img = pc.batch(*pc.one_pass_image_size(axis))
    return img, args, np.stack([pc.pil_resize_crop(x, size, box) for x in img])


def _all_pil_cases():
    for H, W, n in pc.OPS_CASES:
        yield f"{H}x{W}->{n}", n, _ops_case(H, W, n)
    for axis, offset in pc.ONE_PASS_CASES:
        yield f"{axis} only, offset {offset}", pc.ONE_PASS_N, _one_pass_case(axis, offset)


# ---- the reference and the regimes ------------------------------------------------------------------------------------------------------
def test_reference_is_the_transform_of_the_evaluation():
    """Image.resize + crop with the geometry of ops.resize_crop_geometry is what keds_amd.clip's eval transform does, on every case"""
    from PIL import Image
    for H, W, n in pc.OPS_CASES:
        arr = pc.make_image("noise", H, W)
        want = np.asarray(kclip._center_crop(kclip._resize_shorter_side(Image.fromarray(arr), n), n))
        assert np.array_equal(pc.pil_reference(arr, n), want), (H, W, n)
        t = kclip._transform(n, is_train=False)(Image.fromarray(arr)).numpy()
        assert np.array_equal(pc.normalized(want).view(np.uint32), t.view(np.uint32)), (H, W, n)


def test_the_cases_reach_what_they_name():
    assert ops.resize_crop_geometry(300, 37, 28) == (28, 227, 0, 100) and ops.resize_crop_geometry(37, 300, 28) == (227, 28, 100, 0)
    assert pc.one_pass_args("hv", 0)[0]["yk"].shape[1] == 45    # the 10.7 x downscale
    a = pc.pil_args(33, 32, 32)
    assert not a["need_h"] and not a["need_v"]                  # no pass at all
    a = pc.pil_args(1, 40, 8)
    assert a["need_v"] and a["need_h"] and a["left"] == 156
    # white and black: the 22-bit weights of a table row sum to one within a few units (each is rounded on its own), near enough for
    # 255 x the sum to round to 255 steps
    for H, W, n in pc.OPS_CASES:
        _, a, want = _ops_case(H, W, n)
        for k in (a["xk"], a["yk"]):
            assert k is None or (np.abs(k.sum(axis=1) - (1 << 22)) * 255 < 1 << 21).all(), (H, W, n)
        assert (want[pc.REGIMES.index("white")] == 255).all() and (want[pc.REGIMES.index("black")] == 0).all()


def test_checker_and_stripes_overshoot_where_smooth_content_does_not():
    """accumulators below zero / above 255 per image: thousands for the 0 / 255 patterns under upscaling, none for a smooth ramp"""
    H, W, n = 20, 23, 28
    _, neg, over = pc.pil_two_pass(pc.make_image("checker", H, W), n)
    assert neg >= 500 and over >= 500, (neg, over)
    _, neg, over = pc.pil_two_pass(pc.make_image("stripes", H, W), n)
    assert neg >= 100, (neg, over)
    y, x = np.mgrid[0:H, 0:W]
    ramp = np.stack([20 + x * 9, 20 + y * 10, 20 + x * 5 + y * 5], axis=2).astype(np.uint8)
    assert pc.pil_two_pass(ramp, n)[1:] == (0, 0)


# ---- the integer model equals PIL ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,n_px", pc.OPS_CASES)
def test_integer_model_equals_pil(H, W, n_px):
    img, a, want = _ops_case(H, W, n_px)
    f, u8 = pc.pil_kernel_model(img, n_px, **a)
    assert not pc.pil_failures(want, f, u8)
    for b in range(len(img)):                                    # the image-wise form of the same arithmetic
        assert np.array_equal(pc.pil_two_pass(img[b], n_px)[0], want[b])


@pytest.mark.parametrize("axis,offset", pc.ONE_PASS_CASES)
def test_integer_model_equals_pil_one_pass(axis, offset):
    img, a, want = _one_pass_case(axis, offset)
    f, u8 = pc.pil_kernel_model(img, pc.ONE_PASS_N, **a)
    assert not pc.pil_failures(want, f, u8)


# where a mutation must show, at the least
MUST_CATCH = {
    "h_unrounded": ("45x61->28", "20x23->28"), "vertical_first": ("45x61->28", "20x23->28"), "no_round_const": ("45x61->28", "1x40->8", "hv only, offset 0"),
    "no_lower_clamp": ("20x23->28", "9x8->28", "300x37->28", "h only, offset 0", "v only, offset 0"),
    "logical_shift": ("20x23->28", "9x8->28", "300x37->28", "h only, offset 0", "v only, offset 0"),
    "table_row_next": ("45x61->28", "h only, offset 17"), "last_tap_dropped": ("45x61->28", "v only, offset 33", "h only, offset 0"),
    "left_ignored": ("v only, offset 33",), "neighbour_channel": ("33x32->32", "3x3->28"), "stride_hw": ("33x32->32", "17x9->8"),
    "u8_plane_major": ("33x32->32", "1x40->8"),
}
NO_CHANGE = {"left_ignored": tuple(f"{H}x{W}->{n}" for H, W, n in pc.OPS_CASES if (H, W) != (33, 32)) + ("h only, offset 0", "h only, offset 17",
                              "v only, offset 0", "hv only, offset 0")}


@pytest.mark.parametrize("mutation", pc.PIL_MUTATIONS)
def test_mutations_of_the_integer_model_fail_by_bits(mutation):
    caught = set()
    for name, n, (img, a, want) in _all_pil_cases():
        base = pc.pil_kernel_model(img, n, **a)
        f, u8 = pc.pil_kernel_model(img, n, **a, mutation=mutation)
        changed = not (np.array_equal(f.view(np.uint32), base[0].view(np.uint32)) and np.array_equal(u8, base[1]))
        fails = bool(pc.pil_failures(want, f, u8))
        assert fails == changed, (mutation, name)
        if fails:
            caught.add(name)
    assert set(MUST_CATCH[mutation]) <= caught, (mutation, sorted(caught))
    assert not (set(NO_CHANGE.get(mutation, ())) & caught), (mutation, sorted(caught))


def test_what_the_earlier_regime_shows_of_the_clip_mutations():
    """test_gpu_preprocess_equals_pil_transform_bit_for_bit: smooth content + noise of +-20 at n_px = 224, seven sizes.  Three of them resample
    nothing or clamp nothing; the other four catch `no_lower_clamp` and `logical_shift` on 6 to 52 negative accumulators of an image (23 to 157
    bytes of 150,528).  The checker of this bar gives thousands.  The one-pass branches and `left_ignored` it cannot reach at all."""
    from PIL import Image
    shown = {}
    for H, W in [(480, 640), (640, 427), (224, 224), (500, 224), (231, 1000), (150, 180), (224, 300)]:
        rs = np.random.RandomState(H + W)
        base = rs.randint(0, 256, (H // 8 + 1, W // 8 + 1, 3)).astype(np.uint8)
        arr = np.asarray(Image.fromarray(base).resize((W, H), Image.BILINEAR), dtype=np.int16) + rs.randint(-20, 21, (H, W, 3))
        arr = np.clip(arr, 0, 255).astype(np.uint8)
        ref, neg, over = pc.pil_two_pass(arr, 224)
        assert np.array_equal(ref, pc.pil_reference(arr, 224))
        differ = {m: int((pc.pil_two_pass(arr, 224, m)[0] != ref).sum()) for m in ("no_lower_clamp", "logical_shift")}
        assert (differ["no_lower_clamp"] > 0) == (neg > 0) == (differ["logical_shift"] > 0)
        shown[(H, W)] = neg
        a = pc.pil_args(H, W, 224)
        assert a["need_h"] == a["need_v"], "a one-pass call through ops.preprocess"
    print("negative accumulators per image of the earlier test:", shown)
    assert {k for k, v in shown.items() if v == 0} == {(224, 224), (500, 224), (224, 300)}
    assert max(shown.values()) < 100


# ---- keds_preprocess ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _f32_case(H, W, n_px, regimes):
    img = pc.batch(H, W, regimes)
    return img, pc.f32_allowed(img, n_px), pc.f32_kernel_model(img, n_px)


def test_f32_geometry_rounds_half_to_even():
    assert pc.f32_geometry(33, 32, 32) == (32, 33, 0, 0) and pc.f32_geometry(35, 32, 32)[3] == 2 and pc.f32_geometry(37, 32, 32)[3] == 2
    for H, W, n in pc.OPS_CASES:
        assert pc.f32_geometry(H, W, n) == ops.resize_crop_geometry(H, W, n)


@pytest.mark.parametrize("H,W,n_px,regimes", pc.F32_CASES)
def test_float32_model_passes_its_check(H, W, n_px, regimes):
    img, allowed, got = _f32_case(H, W, n_px, regimes)
    msgs, share, v = pc.f32_failures(img, n_px, got, allowed=allowed)
    want = np.stack([pc.pil_reference(x, n_px) for x in img])
    print(f"keds_preprocess model {H}x{W}->{n_px}: ambiguous share {share:.4f}, differs from PIL on {float((v != want).mean()):.4f} of the outputs "
          f"by at most {int(np.abs(v - want.astype(np.int64)).max())}")
    assert not msgs, msgs
    assert share <= pc.AMBIGUOUS_CAP


def test_the_exact_two_times_downscale_of_checker_is_ambiguous():
    """28 % and more of its outputs sit exactly on a tie: the case cannot show a failure and is left out of the table"""
    img = pc.batch(64, 64, ("checker", "stripes"))
    lo, hi = pc.f32_allowed(img, 32)
    assert (hi > lo).mean(axis=(1, 2, 3)).min() > pc.AMBIGUOUS_CAP


@pytest.mark.parametrize("mutation", pc.F32_MUTATIONS)
def test_mutations_of_the_float32_model_fall_outside_the_set(mutation):
    both = [c for c in pc.F32_CASES if pc.f32_geometry(*c[:3])[0] != c[1] and pc.f32_geometry(*c[:3])[1] != c[0]]
    must = {"h_unrounded": both[:3], "vertical_first": both[:3], "last_tap_dropped": both, "truncate": both,
            "neighbour_channel": list(pc.F32_CASES), "stride_hw": list(pc.F32_CASES)}[mutation]
    for case in pc.F32_CASES:
        H, W, n, regimes = case
        img, allowed, base = _f32_case(*case)
        got = pc.f32_kernel_model(img, n, mutation=mutation)
        msgs, _, v = pc.f32_failures(img, n, got, allowed=allowed)
        _, _, v0 = pc.f32_failures(img, n, base, allowed=allowed)
        single = allowed[0] == allowed[1]
        if ((v != v0) & single).any():                          # a changed value where the definition allows one: outside the set
            assert msgs, (mutation, case)
        if case in must:
            assert msgs, (mutation, case, "not caught")
