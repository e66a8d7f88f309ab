"""References, regimes and checks of the image preprocessing (keds_amd/csrc/elementwise.hip: preprocess_pil_kernel behind
keds_preprocess_pil / ops.preprocess, preprocess_kernel behind keds_preprocess).  numpy + PIL, no GPU.

tests/test_host_preprocess_check.py shows that an integer model of preprocess_pil_kernel equals PIL, that a float32 model of
preprocess_kernel passes its check and that mutations of both fail; tests/test_gpu_preprocess_edges.py holds the kernels to the same.

keds_preprocess_pil: the reference is PIL itself -- Image.resize(BICUBIC) then crop -- and the uint8 image must equal it byte for byte;
the float output must equal (r.float() / 255 - m) / s in fp32.  No tolerance.

keds_preprocess computes the same two passes with fp32 weights and rounds floor(x + 0.5) after each, so PIL's bytes are not its
specification.  It is held to a float64 evaluation of its own definition that carries, per output, the set of 8-bit values the definition
allows: a pass whose float64 value lies within e of a tie allows both neighbours, and the vertical pass is evaluated over the interval
the horizontal sets span.  e is derived from the kernel's fp32 operations (pass_error below), not tuned on the kernel; at most
AMBIGUOUS_CAP of a case's outputs may allow more than one value.  The float must lie within 4 u (v / 255 + |m|) / |s| of the float64
normalisation of the value recovered from it.
"""
import numpy as np

from keds_amd import ops

U = 2.0 ** -24
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
REGIMES = ("noise", "white", "black", "checker", "stripes")
AMBIGUOUS_CAP = 0.20

# (H, W, n_px) through ops.preprocess: down- and upscaling both ways; the extreme aspect ratios (crop offset 100 on either axis); a 2 x
# downscale with its exact ties; no pass at all; a one-row image upscaled 8 x vertically
OPS_CASES = ((45, 61, 28), (61, 45, 28), (20, 23, 28), (9, 8, 28), (3, 3, 28), (300, 37, 28), (37, 300, 28), (64, 64, 32), (33, 32, 32),
             (17, 9, 8), (1, 40, 8))
# one pass only, which ops.preprocess cannot reach: (axis, offset of the crop on the other axis); "hv": both passes of a 300 x 37 image
# squashed to 28 x 28, a 10.7 x downscale with 45 taps, which the aspect-preserving geometry of ops.preprocess cannot reach either
ONE_PASS_CASES = (("h", 0), ("h", 17), ("v", 0), ("v", 33), ("hv", 0))
ONE_PASS_H, ONE_PASS_W, ONE_PASS_N = 45, 61, 28
SQUASH_H, SQUASH_W = 300, 37
# keds_preprocess: sides of at most 64 pixels (the centre term of e grows with the coordinate)
# (the exact 2 x downscale puts 28 % and more of the outputs of `checker` and `stripes` on a tie: it runs on the other regimes)
F32_CASES = tuple((H, W, n, REGIMES) for H, W, n in ((45, 61, 28), (61, 45, 28), (20, 23, 28), (9, 8, 28), (3, 3, 28), (33, 32, 32), (17, 9, 8),
                                                     (1, 40, 8))) + ((64, 64, 32, ("noise", "white", "black")),)


def make_image(regime, H, W, seed=0):
    """uint8 [H, W, 3]"""
    y, x = np.mgrid[0:H, 0:W]
    if regime == "noise":
        return np.random.RandomState(seed * 1000 + H * 31 + W).randint(0, 256, (H, W, 3)).astype(np.uint8)
    if regime == "white":
        return np.full((H, W, 3), 255, np.uint8)
    if regime == "black":
        return np.zeros((H, W, 3), np.uint8)
    if regime == "checker":                                      # 0 / 255 cells of 3 x 2 pixels: overshoots on both sides under upscaling
        c = (((x // 3) + (y // 2)) % 2 * 255).astype(np.uint8)
        return np.stack([c, c, 255 - c], axis=2)
    if regime == "stripes":                                      # alternating columns in R, rows in G, every third diagonal in B
        return np.stack([(x % 2) * 255, (y % 2) * 255, ((x + y) % 3 == 0) * 255], axis=2).astype(np.uint8)
    raise ValueError(regime)


def one_pass_image_size(axis):
    return (SQUASH_H, SQUASH_W) if axis == "hv" else (ONE_PASS_H, ONE_PASS_W)


def batch(H, W, regimes=REGIMES, seed=0):
    return np.stack([make_image(r, H, W, seed) for r in regimes])


# ---- PIL ----------------------------------------------------------------------------------------------------------------------------------
def pil_resize_crop(arr, size, box):
    """PIL itself: resize to size = (RW, RH) with BICUBIC, then crop box = (left, top, right, bottom) -> uint8 [h, w, 3]"""
    from PIL import Image
    return np.asarray(Image.fromarray(arr).resize(size, Image.BICUBIC).crop(box), dtype=np.uint8)


def pil_reference(arr, n_px):
    RW, RH, left, top = ops.resize_crop_geometry(arr.shape[0], arr.shape[1], n_px)
    return pil_resize_crop(arr, (RW, RH), (left, top, left + n_px, top + n_px))


def normalized(u8, mean=MEAN, std=STD):
    """(r.float() / 255 - m) / s in torch fp32 on a uint8 [..., n, n, 3] -> float32 [..., 3, n, n]"""
    import torch
    t = torch.from_numpy(np.array(u8, dtype=np.uint8)).movedim(-1, -3).float()
    m = torch.tensor(mean, dtype=torch.float32)[:, None, None]
    s = torch.tensor(std, dtype=torch.float32)[:, None, None]
    return ((t / 255 - m) / s).numpy()


def pil_args(H, W, n_px):
    """the arguments ops.preprocess hands keds_preprocess_pil: dict(need_h, need_v, left, top, xb, xk, yb, yk), tables sliced to the crop"""
    RW, RH, left, top = ops.resize_crop_geometry(H, W, n_px)
    a = dict(need_h=RW != W, need_v=RH != H, left=left, top=top, xb=None, xk=None, yb=None, yk=None)
    if a["need_h"]:
        b, k = ops.pil_bicubic_coeffs(W, RW)
        a["xb"], a["xk"] = b[left:left + n_px].copy(), k[left:left + n_px].copy()
    if a["need_v"]:
        b, k = ops.pil_bicubic_coeffs(H, RH)
        a["yb"], a["yk"] = b[top:top + n_px].copy(), k[top:top + n_px].copy()
    return a


def one_pass_args(axis, offset):
    """-> (the arguments, PIL's size, PIL's crop box) of a call that resamples one axis of the 45 x 61 image to 28 and crops the other"""
    H, W, n = ONE_PASS_H, ONE_PASS_W, ONE_PASS_N
    if axis == "hv":
        (xb, xk), (yb, yk) = ops.pil_bicubic_coeffs(SQUASH_W, n), ops.pil_bicubic_coeffs(SQUASH_H, n)
        return (dict(need_h=True, need_v=True, left=0, top=0, xb=xb.copy(), xk=xk.copy(), yb=yb.copy(), yk=yk.copy()), (n, n), (0, 0, n, n))
    if axis == "h":
        b, k = ops.pil_bicubic_coeffs(W, n)
        return (dict(need_h=True, need_v=False, left=0, top=offset, xb=b.copy(), xk=k.copy(), yb=None, yk=None), (n, H),
                (0, offset, n, offset + n))
    b, k = ops.pil_bicubic_coeffs(H, n)
    return (dict(need_h=False, need_v=True, left=offset, top=0, xb=None, xk=None, yb=b.copy(), yk=k.copy()), (W, n),
            (offset, 0, offset + n, n))


# ---- the integer model of preprocess_pil_kernel -----------------------------------------------------------------------------------------
PIL_MUTATIONS = ("h_unrounded", "vertical_first", "no_round_const", "no_lower_clamp", "logical_shift", "table_row_next", "last_tap_dropped",
                 "left_ignored", "neighbour_channel", "stride_hw", "u8_plane_major")


def _clip8(v, mutation):
    """clip8(acc >> 22) on int64 values that fit int32"""
    assert (np.abs(v) < (1 << 31)).all(), "an accumulator leaves int32"
    if mutation == "logical_shift":
        s = (v & 0xFFFFFFFF) >> 22
    else:
        s = v >> 22
    if mutation == "no_lower_clamp":                             # stored through an unsigned char
        return np.where(s > 255, 255, s & 0xFF)
    return np.clip(s, 0, 255)


def pil_kernel_model(img, n_px, need_h, need_v, left, top, xb, xk, yb, yk, mean=MEAN, std=STD, mutation=None):
    """preprocess_pil_kernel, one output pixel at a time as the kernel does it: the horizontal pass recomputed for every vertical tap, the
    table rows indexed by the crop's column / row -> (float32 [B, 3, n, n], the bytes of the u8 output [B * n * n * 3])"""
    B, H, W, _ = img.shape
    flat = np.ascontiguousarray(img).reshape(-1).astype(np.int64)
    ch = np.arange(3)
    half = 0 if mutation == "no_round_const" else 1 << 21
    r = np.zeros((B, n_px, n_px, 3), np.int64)
    for b in range(B):
        base = b * H * W * (1 if mutation == "stride_hw" else 3)
        for oy in range(n_px):
            y0, yn = (int(yb[oy, 0]), int(yb[oy, 1])) if need_v else (oy + top, 1)
            ky = yk[oy, :yn].astype(np.int64) if need_v else None
            for ox in range(n_px):
                if need_h:
                    x0, xn = int(xb[ox, 0]), int(xb[ox, 1])
                    kx = xk[min(ox + 1, n_px - 1) if mutation == "table_row_next" else ox].astype(np.int64)
                    if mutation == "last_tap_dropped":
                        xn -= 1
                    kx = kx[:xn]
                else:
                    x0, xn = (ox if mutation == "left_ignored" else ox + left), 1
                yy, xx = np.arange(y0, y0 + yn)[:, None, None], np.arange(x0, x0 + xn)[None, :, None]
                px = flat[base + (yy * W + xx) * 3 + ch]       # [yn, xn, 3]
                if mutation == "vertical_first" and need_h and need_v:
                    v = _clip8(half + (ky[:, None, None] * px).sum(axis=0), None)
                    r[b, oy, ox] = _clip8(half + (kx[:, None] * v).sum(axis=0), None)
                    continue
                if need_h:
                    acc = half + (kx[None, :, None] * px).sum(axis=1)
                    h = (acc - half) / float(1 << 22) if mutation == "h_unrounded" else _clip8(acc, mutation)
                else:
                    h = px[:, 0, :]
                if need_v:
                    if mutation == "last_tap_dropped" and not need_h:
                        ky, h = ky[:yn - 1], h[:yn - 1]
                    a = half + (ky[:, None] * h).sum(axis=0)
                    r[b, oy, ox] = _clip8(np.floor(a).astype(np.int64), mutation)
                else:
                    r[b, oy, ox] = np.floor(h[0]).astype(np.int64) if mutation == "h_unrounded" else h[0]
    m, s = np.array(mean, np.float32), np.array(std, np.float32)
    if mutation == "neighbour_channel":
        m, s = np.roll(m, -1), np.roll(s, -1)
    f = ((r.astype(np.float32) / np.float32(255.0) - m) / s).astype(np.float32).transpose(0, 3, 1, 2)
    u8 = (r & 0xFF).astype(np.uint8)
    if mutation == "u8_plane_major":
        u8 = u8.transpose(0, 3, 1, 2)
    return np.ascontiguousarray(f), np.ascontiguousarray(u8).reshape(-1)


def pil_two_pass(arr, n_px, clip=None):
    """the same arithmetic image-wise (the horizontal pass of every source row, then the vertical one) for one image through the geometry
    of ops.preprocess -> (uint8 [n, n, 3], accumulators below zero, accumulators above 255 after the shift); clip: None or a clip8
    mutation"""
    H, W, _ = arr.shape
    a = pil_args(H, W, n_px)
    src = arr.astype(np.int64)
    neg = over = 0
    if a["need_h"]:
        cols = []
        for ox in range(n_px):
            x0, xn = int(a["xb"][ox, 0]), int(a["xb"][ox, 1])
            acc = (1 << 21) + (a["xk"][ox, :xn].astype(np.int64)[None, :, None] * src[:, x0:x0 + xn]).sum(axis=1)
            neg, over = neg + int((acc < 0).sum()), over + int(((acc >> 22) > 255).sum())
            cols.append(_clip8(acc, clip))
        src = np.stack(cols, axis=1)
    else:
        src = src[:, a["left"]:a["left"] + n_px]
    if a["need_v"]:
        rows = []
        for oy in range(n_px):
            y0, yn = int(a["yb"][oy, 0]), int(a["yb"][oy, 1])
            acc = (1 << 21) + (a["yk"][oy, :yn].astype(np.int64)[:, None, None] * src[y0:y0 + yn]).sum(axis=0)
            neg, over = neg + int((acc < 0).sum()), over + int(((acc >> 22) > 255).sum())
            rows.append(_clip8(acc, clip))
        src = np.stack(rows, axis=0)
    else:
        src = src[a["top"]:a["top"] + n_px]
    return (src & 0xFF).astype(np.uint8), neg, over


def pil_failures(want_u8, got_f, got_u8, mean=MEAN, std=STD, what=""):
    """want_u8: PIL's [B, n, n, 3]; got_f float32 [B, 3, n, n]; got_u8: the bytes of the u8 output, or None"""
    msgs = []
    if got_u8 is not None:
        got_u8 = np.asarray(got_u8).reshape(-1)
        if got_u8.size != want_u8.size or not np.array_equal(got_u8, want_u8.reshape(-1)):
            bad = np.argwhere(got_u8.reshape(want_u8.shape) != want_u8)
            first = tuple(bad[0])
            msgs.append(f"{what}the uint8 image differs from PIL's at {len(bad)} of {want_u8.size} bytes, first (b, y, x, c) {first}: "
                        f"{got_u8.reshape(want_u8.shape)[first]} for {want_u8[first]}")
    want_f = normalized(want_u8, mean, std)
    got_f = np.asarray(got_f, np.float32).reshape(want_f.shape)
    if not np.array_equal(got_f.view(np.uint32), want_f.view(np.uint32)):
        bad = np.argwhere(got_f.view(np.uint32) != want_f.view(np.uint32))
        first = tuple(bad[0])
        msgs.append(f"{what}the float output differs from (r / 255 - m) / s at {len(bad)} of {want_f.size} places, first (b, c, y, x) {first}: "
                    f"{got_f[first]!r} for {want_f[first]!r}")
    return msgs


# ---- keds_preprocess: the fp32-weight form -----------------------------------------------------------------------------------------------
def f32_geometry(H, W, n_px):
    """RW, RH, left, top of keds_preprocess: torchvision's Resize(int) and CenterCrop offsets rounded half to even (lrintf)"""
    if W <= H:
        RW, RH = n_px, n_px * H // W
    else:
        RW, RH = n_px * W // H, n_px
    return RW, RH, int(round((RW - n_px) / 2.0)), int(round((RH - n_px) / 2.0))


def _cubic(x):
    x = np.abs(x)
    return np.where(x < 1.0, ((1.5 * x - 2.5) * x) * x + 1.0, np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5, 0.0))


def _window(i, scale, in_size, dt):
    """pil_window of elementwise.hip in the arithmetic of dtype dt -> lo, hi, centre, 1 / filterscale"""
    one, half = dt(1.0), dt(0.5)
    fs = max(dt(scale), one)
    support = dt(2.0) * fs
    center = dt(dt(i) + half) * dt(scale)
    lo, hi = int(dt(dt(center - support) + half)), int(dt(dt(center + support) + half))
    return max(lo, 0), min(hi, in_size), center, dt(one / fs)


def pass_error(n, S, A, Q, P, center, ss, vmax=255.0):
    """|fp32 pass - float64 pass| before the rounding, for one output of one pass with n taps; S = sum w, A = sum |w| (unnormalised cubic
    weights), Q = sum p, P = sum |w| p / S over the taps (p: the 8-bit inputs).  With u = 2^-24 and every fp32 operation within u of exact:
      the centre (i + 1/2) scale: scale = fl(in / out) and the product round once each: |dc| <= 2 u c;
      the argument t = fl(fl(fl(x - c) + 0.5) ss): dc, two additions on magnitudes <= 2 fs + 1.5, ss = fl(1 / fs) and the product:
        |dt| <= ss (2 u c + 2 u (2 fs + 1.5)) + 3 u |t| <= u (2 c ss + 16)             (ss fs = 1, ss <= 1, |t| <= 2.5);
      the cubic, |slope| <= 1.4, its Horner steps on magnitudes <= 8: <= 26 u of evaluation error (the 1 <= |t| < 2 branch; 10 u below 1):
        dw = u (26 + 1.4 (2 c ss + 16));
      the weight sum over n taps: |dS| <= n dw + n u A, so every normalised weight w / S is off by dw / S + (|w| / S)(dS / S + u);
      the accumulation: every product and every addition rounds once on a partial sum <= P:
        e = dw Q / S + P (dS / S + (n + 2) u)
      and floorf(x + 0.5f) adds one more rounding on a magnitude <= 256."""
    dw = U * (26.0 + 1.4 * (2.0 * abs(center) * ss + 16.0))
    dS = n * dw + n * U * A
    return dw * Q / S + P * (dS / S + (n + 2) * U) + (vmax + 1.0) * U


def _round_set(x, e):
    """the integers floor(v + 0.5), clamped to [0, 255], over v in [x_lo - e, x_hi + e]; x = (x_lo, x_hi) arrays"""
    lo = np.clip(np.floor(x[0] - e + 0.5), 0, 255).astype(np.int64)
    hi = np.clip(np.floor(x[1] + e + 0.5), 0, 255).astype(np.int64)
    return lo, hi


def f32_allowed(img, n_px):
    """the 8-bit values keds_preprocess's definition allows per output, as an inclusive interval -> (lo, hi) int64 [B, n, n, 3]"""
    B, H, W, _ = img.shape
    RW, RH, left, top = f32_geometry(H, W, n_px)
    p = img.astype(np.float64)
    # the horizontal pass of every source row for the n_px columns of the crop: an interval [B, H, n, 3]
    if RW == W:
        h_lo = h_hi = p[:, :, left:left + n_px, :]
    else:
        h_lo, h_hi = np.zeros((B, H, n_px, 3)), np.zeros((B, H, n_px, 3))
        for ox in range(n_px):
            lo, hi, c, ss = _window(ox + left, W / RW, W, float)
            w = _cubic((np.arange(lo, hi) - c + 0.5) * ss)
            S, A = w.sum(), np.abs(w).sum()
            taps = p[:, :, lo:hi, :]
            val = (taps * w[None, None, :, None]).sum(axis=2) / S
            e = pass_error(hi - lo, S, A, taps.sum(axis=2), (taps * np.abs(w)[None, None, :, None]).sum(axis=2) / S, c, ss)
            h_lo[:, :, ox], h_hi[:, :, ox] = _round_set((val, val), e)
    if RH == H:
        return (h_lo[:, top:top + n_px].astype(np.int64), h_hi[:, top:top + n_px].astype(np.int64))
    out_lo, out_hi = np.zeros((B, n_px, n_px, 3), np.int64), np.zeros((B, n_px, n_px, 3), np.int64)
    for oy in range(n_px):
        lo, hi, c, ss = _window(oy + top, H / RH, H, float)
        w = _cubic((np.arange(lo, hi) - c + 0.5) * ss)
        S, A = w.sum(), np.abs(w).sum()
        wn = (w / S)[None, :, None, None]
        a, b = h_lo[:, lo:hi], h_hi[:, lo:hi]
        v_lo = (np.where(wn >= 0, a, b) * wn).sum(axis=1)       # the vertical pass over everything the horizontal sets allow
        v_hi = (np.where(wn >= 0, b, a) * wn).sum(axis=1)
        e = pass_error(hi - lo, S, A, b.sum(axis=1), (b * np.abs(w)[None, :, None, None]).sum(axis=1) / S, c, ss)
        out_lo[:, oy], out_hi[:, oy] = _round_set((v_lo, v_hi), e)
    return out_lo, out_hi


# (`left_ignored` has nothing to change here: keds_preprocess skips the horizontal pass only when W == n_px, and then left = 0)
F32_MUTATIONS = ("h_unrounded", "vertical_first", "last_tap_dropped", "neighbour_channel", "stride_hw", "truncate")


def f32_kernel_model(img, n_px, mean=MEAN, std=STD, mutation=None):
    """preprocess_kernel in numpy float32, one output pixel at a time, every operation rounded to fp32 in the kernel's order (no
    contraction) -> float32 [B, 3, n, n]"""
    f = np.float32
    B, H, W, _ = img.shape
    RW, RH, left, top = f32_geometry(H, W, n_px)
    flat = np.ascontiguousarray(img).reshape(-1)
    sx, sy = f(f(W) / f(RW)), f(f(H) / f(RH))
    out = np.zeros((B, 3, n_px, n_px), f)
    m, s = np.array(mean, f), np.array(std, f)
    if mutation == "neighbour_channel":
        m, s = np.roll(m, -1), np.roll(s, -1)

    def cubic(x):
        x = np.abs(x).astype(f)
        a = f(-0.5)
        lt1 = ((a + f(2.0)) * x - (a + f(3.0))) * x * x + f(1.0)
        lt2 = (((x - f(5.0)) * x + f(8.0)) * x - f(4.0)) * a
        return np.where(x < 1, lt1, np.where(x < 2, lt2, f(0.0))).astype(f)

    def clip8(v):
        v = np.floor(v if mutation == "truncate" else v + f(0.5)).astype(f)
        return np.minimum(np.maximum(v, f(0.0)), f(255.0))

    def weights(i, scale, size):
        lo, hi, c, ss = _window(i, scale, size, f)
        w = cubic(((np.arange(lo, hi).astype(f) - c).astype(f) + f(0.5)) * ss)
        tot = f(0.0)
        for v in w:
            tot = f(tot + v)
        return lo, hi, (w / tot).astype(f)

    for b in range(B):
        base = b * H * W * (1 if mutation == "stride_hw" else 3)
        src = flat[base:base + H * W * 3].reshape(H, W, 3).astype(f)
        for oy in range(n_px):
            ylo, yhi, wy = weights(oy + top, sy, H)
            for ox in range(n_px):
                xlo, xhi, wx = weights(ox + left, sx, W)
                if mutation == "last_tap_dropped" and RW != W:
                    xhi, wx = xhi - 1, wx[:-1]
                rows = src[ylo:yhi]
                if mutation == "vertical_first" and RW != W and RH != H:
                    v = np.zeros((xhi - xlo, 3), f)
                    for j in range(yhi - ylo):
                        v = (v + wy[j] * rows[j, xlo:xhi]).astype(f)
                    v = clip8(v)
                    acc = np.zeros(3, f)
                    for j in range(xhi - xlo):
                        acc = (acc + wx[j] * v[j]).astype(f)
                    acc = clip8(acc)
                else:
                    if RW == W:
                        h = rows[:, (ox if mutation == "left_ignored" else ox + left)]
                    else:
                        h = np.zeros((yhi - ylo, 3), f)
                        for j in range(xhi - xlo):
                            h = (h + wx[j] * rows[:, xlo + j]).astype(f)
                        if mutation != "h_unrounded":
                            h = clip8(h)
                    if RH == H:
                        acc = h[oy + top - ylo]
                    else:
                        acc = np.zeros(3, f)
                        for j in range(yhi - ylo):
                            acc = (acc + wy[j] * h[j]).astype(f)
                        acc = clip8(acc)
                out[b, :, oy, ox] = ((acc * f(f(1.0) / f(255.0))).astype(f) - m) / s
    return out


def f32_failures(img, n_px, got, mean=MEAN, std=STD, what="", allowed=None):
    """-> (failures, ambiguous share, values recovered from the output [B, n, n, 3])"""
    lo, hi = allowed if allowed is not None else f32_allowed(img, n_px)
    m, s = np.array(mean, np.float32).astype(np.float64), np.array(std, np.float32).astype(np.float64)
    g = np.asarray(got, np.float32).astype(np.float64).transpose(0, 2, 3, 1)          # [B, n, n, 3]
    v = np.rint((g * s + m) * 255.0)
    msgs = []
    if not np.isfinite(g).all():
        msgs.append(f"{what}non-finite output")
        v = np.nan_to_num(v, nan=-1.0, posinf=-1.0, neginf=-1.0)
    v = v.astype(np.int64)
    outside = (v < lo) | (v > hi)
    if outside.any():
        first = tuple(np.argwhere(outside)[0])
        msgs.append(f"{what}{int(outside.sum())} of {v.size} outputs hold a value the definition does not allow, first (b, y, x, c) {first}: "
                    f"{v[first]} outside [{lo[first]}, {hi[first]}]")
    bound = 4.0 * U * (np.abs(v) / 255.0 + np.abs(m)) / np.abs(s)
    off = np.abs(g - (v / 255.0 - m) / s)
    if (off > bound).any():
        first = tuple(np.argwhere(off > bound)[0])
        msgs.append(f"{what}{int((off > bound).sum())} floats lie further from the normalisation of their value than 4 u (v / 255 + |m|) / |s|, "
                    f"first (b, y, x, c) {first}: {off[first]:.3g} > {bound[first]:.3g}")
    share = float((hi > lo).mean())
    if share > AMBIGUOUS_CAP:
        msgs.append(f"{what}{share:.3f} of the outputs allow more than one value: the case cannot show a failure (cap {AMBIGUOUS_CAP})")
    return msgs, share, v

