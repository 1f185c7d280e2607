"""GPU parity of the resampling / packing kernels (csrc/resample.hip), one kernel at a time, against the references of
oracle/resample.py: float64 where the operation rounds, bit-exact where it only moves or truncates values.

House rules (as in test_decoder_kernels_gpu.py): every output buffer is filled with NaN (0xA5 bytes for integer buffers) before the
call, so an element a kernel leaves unwritten fails; bounds are c x 2^-23 x magnitude element-wise, the magnitude coming from the
reference (tests/test_resample_reference_cpu.py shows the same bounds hold for ATen's own fp32 kernels); no flat tolerances. Every
call goes through protosam_amd.ops (one NULL-pointer rejection in the argument test excepted: ops cannot express it).

Worst ratios measured on an MI355X (profiles/resample_kernel_tests.txt, 158 tests in 11 s) are quoted in the docstrings.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import resample as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
NAN = float("nan")
HALF_FLOOR = 2.0 ** -25        # half the spacing of the subnormal halves
PIXEL_MEAN, PIXEL_STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def _a5(shape, dev, dtype=torch.uint8):
    """An integer buffer of 0xA5 bytes."""
    fill = {torch.uint8: 0xA5, torch.int32: -1515870811}[dtype]           # 0xA5A5A5A5 as int32
    return torch.full(shape, fill, dtype=dtype, device=dev)


def _within(out, ref, mag, c, what, floor=0.0):
    """|out - ref| <= c 2^-23 mag (+ floor) element-wise; returns the worst |out - ref| / (2^-23 mag) for the report."""
    out = out.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(out).all()), f"{what}: {int((~torch.isfinite(out)).sum())} non-finite (unwritten?) elements"
    err = (out - ref).abs()
    worst = ((err - floor).clamp_min(0) / mag.clamp_min(1e-300)).max().item() / U
    bad = err > c * U * mag + floor
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements off by more than {c} x 2^-23 x magnitude (worst {worst:.2f})"
    print(f"{what}: worst |err| = {worst:.2f} x 2^-23 x magnitude (bound {c})")
    return worst


def _planes(P, IH, IW, seed):
    """P planes of 5 * randn; with P >= 3 the last two are 1e4 + randn (cancellation in the weights shows here) and a plane that is
    zero except its last row and last column (a wrong i1 clamp shows here)."""
    x = _rand((P, IH, IW), seed, 5.0)
    if P >= 3:
        x[-2] = 1e4 + _rand((IH, IW), seed + 1)
        edge = torch.zeros((IH, IW))
        edge[-1, :] = 3.0 + torch.arange(IW, dtype=torch.float32)
        edge[:, -1] = -2.0 - torch.arange(IH, dtype=torch.float32)
        x[-1] = edge
    return x


# ---- 1. the plane kernels: psam_bilinear_nchw, psam_resize2d ------------------------------------------------------------
# (planes, IH, IW, OH, OW): the ten shapes of the CPU test; OW on and around the 256-wide block edge; OH = 1, OW = 1 and IH = 1
# (scale 0 with align_corners); 1, 7 and 70 planes
PLANE_CASES = [(3, 36, 36, 512, 512), (3, 512, 512, 1024, 1024), (3, 73, 73, 1024, 1024), (3, 300, 517, 1024, 1024),
               (3, 1024, 1024, 256, 256), (3, 640, 480, 37, 53), (3, 7, 5, 3, 2), (3, 1, 1, 9, 9), (3, 64, 64, 64, 64),
               (3, 256, 256, 1001, 999),
               (7, 40, 100, 5, 1), (7, 40, 100, 5, 3), (7, 40, 100, 5, 255), (7, 40, 100, 5, 256), (7, 40, 100, 5, 257),
               (7, 40, 100, 5, 1001), (1, 40, 100, 1, 300), (1, 1, 50, 4, 120), (3, 1, 1, 1, 1), (70, 20, 30, 45, 64)]


@pytest.mark.parametrize("P,IH,IW,OH,OW", PLANE_CASES)
def test_plane_resize_modes(dev, P, IH, IW, OH, OW):
    """psam_bilinear_nchw and psam_resize2d modes 0 (the same kernel: torch.equal), 1 (align_corners) and 2 (nearest: exact).
    Bilinear bound: 4 x 2^-23 x (blend + weights); ATen's own fp32 kernel on the CPU needs under 2 of these units. Measured worst: 1.51 (mode 0), 3.37 (mode 1, at
    1024 -> 256 on the 1e4 + randn plane: five roundings of 1e4-sized terms and the rounding of scale * dst, which the float64
    reference does not make; 2.88 at 256 -> 1001 x 999, under 1.9 elsewhere)."""
    from protosam_amd import ops
    x = _planes(P, IH, IW, 100 * IH + OW + P)
    xd = x.to(dev)
    what = f"{P}x{IH}x{IW}->{OH}x{OW}"
    out0 = _nan((P, OH, OW), dev)
    ops.bilinear_nchw(xd, OH, OW, out=out0)
    ref, blend, weights = R.bilinear(x, OH, OW)
    _within(out0, ref, blend + weights, 4, f"bilinear_nchw {what}")
    out = _nan((P, OH, OW), dev)
    ops.resize2d(xd, OH, OW, 0, out=out)
    assert torch.equal(out, out0)
    out = _nan((P, OH, OW), dev)
    ops.resize2d(xd, OH, OW, 1, out=out)
    ref, blend, weights = R.bilinear(x, OH, OW, align_corners=True)
    _within(out, ref, blend + weights, 4, f"resize2d align_corners {what}")
    out = _nan((P, OH, OW), dev)
    ops.resize2d(xd, OH, OW, 2, out=out)
    assert torch.equal(out.cpu(), R.nearest(x, OH, OW)), f"resize2d nearest {what}"


# ---- 2. psam_bilinear_tokens --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 100, 768])
@pytest.mark.parametrize("ih,iw,oh,ow", [(18, 18, 32, 32), (36, 36, 32, 32), (9, 13, 32, 32), (32, 32, 32, 32)])
def test_bilinear_tokens(dev, ih, iw, oh, ow, C):
    """Token-major resize with a row stride ld > C and a batch stride beyond the map; the padding holds NaN and must not reach the
    result. Bound as for the plane kernels; measured worst 1.56."""
    from protosam_amd import ops
    B, ld = 3, C + 5
    bstride = ih * iw * ld + 11
    data = _rand((B, ih * iw, C), ih + 7 * C, 5.0)
    data[1] += 1e4
    buf = torch.full((B, bstride), NAN)
    buf[:, :ih * iw * ld].view(B, ih * iw, ld)[:, :, :C] = data
    out = _nan((B, oh * ow, C), dev)
    ops.bilinear_tokens(buf.to(dev), bstride, ld, B, ih, iw, C, oh, ow, out=out)
    ref, blend, weights = R.bilinear(data.view(B, ih, iw, C).permute(0, 3, 1, 2).reshape(B * C, ih, iw), oh, ow)
    tok = lambda t: t.view(B, C, oh * ow).permute(0, 2, 1)  # noqa: E731
    _within(out, tok(ref), tok(blend + weights), 4, f"bilinear_tokens {ih}x{iw}->{oh}x{ow} C={C}")


# ---- 3. psam_patchify_bilinear ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", ["same", (512, 512), (300, 517)])
@pytest.mark.parametrize("S,P,Kpad", [(504, 14, 640), (1024, 16, 768), (28, 14, 640), (32, 16, 768)])
def test_patchify_bilinear(dev, S, P, Kpad, HW):
    """H == S and W == S: half(img) in patch order, exactly. Otherwise the fp16 rounding of an fp32 value that is itself within the
    bilinear bound: |out - ref| <= 2^-11 |ref| + 4 x 2^-23 (blend + weights) + 2^-25. Columns >= 3*P*P are exactly zero.
    Measured: 0.45 of the bilinear units beyond the fp16 rounding."""
    from protosam_amd import ops
    B, C = 2, 3
    H, W = (S, S) if HW == "same" else HW
    img = _rand((B, C, H, W), S + H + W, 5.0)
    img[1, 1] = 1e3 + _rand((H, W), S)
    n = B * (S // P) ** 2
    out = _nan((n, Kpad), dev, torch.float16)
    ops.patchify_bilinear(img.to(dev), S, P, Kpad, out=out)
    K = C * P * P
    assert bool((out[:, K:] == 0).all()), "K padding not zero"
    if HW == "same":
        assert torch.equal(out.cpu(), R.patchify(img.half(), P, Kpad))
        return
    ref, blend, weights = R.bilinear(img.view(B * C, H, W), S, S)
    pat = lambda t: R.patchify(t.view(B, C, S, S), P, K)  # noqa: E731
    ref = pat(ref)
    _within(out[:, :K], ref, pat(blend + weights), 4, f"patchify_bilinear {H}x{W}->{S} P={P}",
            floor=2.0 ** -11 * ref.abs() + HALF_FLOOR)


# ---- 4. psam_prob_argmax ------------------------------------------------------------------------------------------------
PROB_CASES = [(64, 64, 64, 64), (5, 7, 5, 7), (36, 36, 512, 512), (512, 512, 1024, 1024), (300, 517, 1024, 1024),
              (73, 73, 1001, 999)] + [(9, 40, 3, ow) for ow in (1, 2, 3, 4, 5, 1023, 1025)]
SATURATED = 110.0   # exp(-110) = 1.7e-48 lies below half the smallest fp32 subnormal (7e-46): the small probability is exactly 0


def _logits(B, IH, IW, seed):
    """2 * randn (|l1 - l0| stays below 16: see test_prob_argmax), with a block of (80, -80), a block of (-1e4, 1e4), on image 0 a
    block of exact ties, and as image 1 (B = 3) two identical planes. From 128 rows on the field is smooth (coarse noise, upsampled,
    plus a little fine noise): the error band of the argmax grows with the source coordinate times the difference of neighbouring
    samples, and with white noise at 512 x 512 the float64 reference alone would leave 4.6e-4 of the pixels inside it."""
    l = _rand((B, 2, IH, IW), seed, 2.0)
    if IH >= 128:
        l = F.interpolate(_rand((B, 2, IH // 16 + 2, IW // 16 + 2), seed, 2.0), size=(IH, IW), mode="bilinear") + 0.02 * l
    l[:, 0, 0:2, 0:2], l[:, 1, 0:2, 0:2] = 80.0, -80.0
    l[:, 0, 0:2, 3:5], l[:, 1, 0:2, 3:5] = -1e4, 1e4
    l[0, 1, 3:5, 0:4] = l[0, 0, 3:5, 0:4]
    if B > 1:
        l[1, 1] = l[1, 0]
    return l


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("IH,IW,OH,OW", PROB_CASES)
def test_prob_argmax(dev, IH, IW, OH, OW, B):
    """[bilinear] -> softmax -> argmax, with the foreground count.

    Probabilities: 8 x 2^-23 x p (1 + M0 + M1), M = blend + weights of each logit plane (its error magnitude, first order through
    the softmax; zero on the same-size path) - plus 2^-126, below which fp32 has no relative accuracy left. The random logits are
    2 * randn, so |l1 - l0| < 16: the fp32 rounding of l - max alone is |l1 - l0| 2^-24 relative to the small probability, which the
    magnitude of the same-size path does not carry; below 16 it is at most 4 of the 8 units.
    Argmax: equal to the float64 argmax wherever the float64 margin exceeds the logit error bound 4 x 2^-23 (M0 + M1); 0 where the
    margin is exactly 0 (ties: the first maximum); the pixels in between are left out, and are at most 1e-4 of the case.
    fg_sum accumulates onto its seed exactly pred.sum() per image.
    Measured: probabilities 4.50 (64 x 64 same-size, B = 3), under 0.5 on the resized paths; at most 7.1e-5 of the pixels inside the
    band (73 -> 1001 x 999)."""
    from protosam_amd import ops
    l = _logits(B, IH, IW, 1000 * IH + 7 * OW + B)
    same = (IH, IW) == (OH, OW)
    if same:
        v = l.double()
        M = torch.zeros((B, OH, OW), dtype=torch.float64)
    else:
        v, blend, weights = R.bilinear(l.view(B * 2, IH, IW), OH, OW)
        v, m = v.view(B, 2, OH, OW), (blend + weights).view(B, 2, OH, OW)
        M = m[:, 0] + m[:, 1]
    p0, p1, am, margin = R.softmax2_argmax(v[:, 0], v[:, 1])
    prob, pred = _nan((B, 2, OH, OW), dev), _a5((B, OH, OW), dev)
    seed = torch.tensor([1000 + 37 * b for b in range(B)], dtype=torch.int32)
    fg = seed.clone().to(dev)
    ops.prob_argmax(l.to(dev), OH, OW, prob=prob, pred=pred, fg_sum=fg)
    what = f"prob_argmax B={B} {IH}x{IW}->{OH}x{OW}"
    pref = torch.stack([p0, p1], 1)
    _within(prob, pref, pref * (1.0 + M[:, None]), 8, what, floor=2.0 ** -126)
    pc, predc = prob.double().cpu(), pred.cpu()
    assert bool(((pc[:, 0] + pc[:, 1] - 1.0).abs() <= 2 * U).all()), f"{what}: p0 + p1 not within 2 x 2^-23 of 1"
    band = 4 * U * M
    sat = margin > SATURATED + band
    assert int(sat.sum()) > 0 or OW < 7, "no saturated pixel in the case"      # a few output columns can miss the two blocks
    big = torch.where(v[:, 1] > v[:, 0], pc[:, 1], pc[:, 0])
    small = torch.where(v[:, 1] > v[:, 0], pc[:, 0], pc[:, 1])
    assert bool((big[sat] == 1.0).all()) and bool((small[sat] == 0.0).all()), f"{what}: saturated logits not exactly 0 / 1"
    tie, sure = margin == 0, margin > band
    share = (margin.numel() - int(tie.sum()) - int(sure.sum())) / max(margin.numel() - int(tie.sum()), 1)
    print(f"{what}: {margin.numel() - int(tie.sum()) - int(sure.sum())} pixels inside the error band ({share:.1e}), "
          f"{int(tie.sum())} exact ties")
    assert share <= 1e-4, f"{what}: {share:.2e} of the pixels inside the error band - the inputs do not test the argmax"
    assert int(tie.sum()) >= (8 if same else 0) + (OH * OW if B > 1 else 0)
    assert bool((predc <= 1).all())
    assert torch.equal(predc[sure], am[sure]), f"{what}: {int((predc[sure] != am[sure]).sum())} labels differ outside the band"
    assert int(predc[tie].sum()) == 0, f"{what}: a tie went to class 1"
    assert torch.equal(fg.cpu() - seed, predc.view(B, -1).sum(1, dtype=torch.int32)), f"{what}: fg_sum"


# ---- 5. psam_minmax -----------------------------------------------------------------------------------------------------
TRIP = 128 * 256 * 4     # floats one trip of minmax_kernel's grid-stride loop covers (128 workgroups at most, 16 bytes per lane)


def _plant(x, n, b, where):
    """(index of the minimum, index of the maximum) for image b of n elements."""
    tail0 = (n // 4) * 4 if n % 4 else n - 1          # first element after the 16-byte body (of an aligned image)
    return {"first-last": (0, n - 1), "last-first": (n - 1, 0), "tail": (tail0, min(tail0 + 1, n - 1) if n > 1 else 0),
            "deep": (min(5 * TRIP + 17 + b, n - 1), min(3 * TRIP + 4099 - b, n - 1))}[where]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4097, 3 * 37 * 53, 3 * 1024 * 1024])
def test_minmax_exact(dev, n, B):
    """Exact extremes per image, planted at the first / last element, at the first elements after the 16-byte body and (largest size)
    where a workgroup arrives only on a later trip of its grid-stride loop; with n % 4 != 0 images 1 and 2 start off a 16-byte
    boundary (the scalar path). Then all-negative images, images whose extreme is a zero of either sign, and +-inf."""
    from protosam_amd import ops

    def run(x, what):
        mm = _a5((2 * B,), dev, torch.int32)
        ops.minmax(x.to(dev), B, mm=mm)
        got = torch.from_numpy(R.ord_decode(mm.cpu().numpy())).view(B, 2)
        want = torch.stack([x.view(B, -1).min(1).values, x.view(B, -1).max(1).values], 1)
        assert torch.equal(got, want), f"minmax n={n} B={B} {what}: got {got.tolist()}, want {want.tolist()}"
        return got

    for where in ("first-last", "last-first", "tail") + (("deep",) if n > 6 * TRIP else ()):
        x = torch.rand((B, n), generator=torch.Generator().manual_seed(n % 1000 + B)) * 2.0 - 1.0
        for b in range(B):
            imin, imax = _plant(x, n, b, where)
            x[b, imax] = 9.0 + b
            x[b, imin] = -7.0 - 2 * b            # n == 1: one element, both extremes
        run(x, where)
    x = torch.rand((B, n), generator=torch.Generator().manual_seed(5)) * -50.0 - 100.0 * (1 + torch.arange(B).view(B, 1))
    run(x, "all negative")
    x = torch.rand((B, n), generator=torch.Generator().manual_seed(6))
    x[:, n // 2], x[:, 0] = -0.0, 0.0
    got = run(x, "zeros, non-negative")           # torch.equal compares values: -0 == +0
    assert bool((got[:, 0] == 0).all())
    got = run(-x, "zeros, non-positive")
    assert bool((got[:, 1] == 0).all())
    x = _rand((B, n), 7)
    x[:, n - 1], x[:, n // 3] = float("inf"), float("-inf")
    run(x, "infinities")


# ---- 6. psam_sam_patchify -----------------------------------------------------------------------------------------------
def _image(kind, S, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        return torch.randn((3, S, S), generator=g) * (3.0 + seed % 7) + seed % 5
    if kind == "k":          # lo 0, range 255
        return (torch.arange(3 * S * S) % 256).float().view(3, S, S)
    if kind == "k255":       # lo 0, range 1: q * 255 falls just below or on k
        return ((torch.arange(3 * S * S) * 7 % 256).float() / 255.0).view(3, S, S)
    if kind == "narrow":     # a range of 1e-3 around 1e3 (some 16 distinct fp32 values)
        return 1e3 + 1e-3 * torch.rand((3, S, S), generator=g)
    if kind == "constant":
        return torch.full((3, S, S), 0.25)
    raise ValueError(kind)


def _check_sam_patchify(dev, S, P, kinds, seed, skip=()):
    from protosam_amd import ops
    B = len(kinds)
    img = torch.stack([_image(k, S, seed + 11 * b) for b, k in enumerate(kinds)])      # made on the CPU: both sides see these bits
    imgd = img.to(dev)
    mm = _a5((2 * B,), dev, torch.int32)
    ops.minmax(imgd, B, mm=mm)
    lohi = R.ord_decode(mm.cpu().numpy()).reshape(B, 2)
    n, K = (S // P) ** 2, 3 * P * P
    keep = [b for b in range(B) if b not in skip]
    for b in keep:
        assert lohi[b, 0] == img[b].min().item() and lohi[b, 1] == img[b].max().item()
    u8ref = torch.stack([torch.from_numpy(R.quantise(img[b].numpy(), lohi[b, 0], lohi[b, 1])) if b in keep
                         else torch.zeros((3, S, S), dtype=torch.uint8) for b in range(B)])
    sd = torch.tensor(PIXEL_STD, dtype=torch.float64).view(1, 3, 1, 1)
    mean = torch.tensor(PIXEL_MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    ref = R.patchify(R.normalise(u8ref, PIXEL_MEAN, PIXEL_STD), P, K).view(B, n, K)
    mag = R.patchify((u8ref.double() + mean) / sd, P, K).view(B, n, K)
    what = f"sam_patchify S={S} {'/'.join(kinds)}"
    for with_u8 in (True, False):
        out = _nan((B * n, K), dev, torch.float16)
        u8 = _a5((B, 3, S, S), dev) if with_u8 else None
        ops.sam_patchify(imgd, mm, S, P, PIXEL_MEAN, PIXEL_STD, quantise=True, out=out, u8out=u8)      # returns: status 0
        if with_u8:
            for b in keep:      # no share of the pixels is exempt
                diff = int((u8[b].cpu() != u8ref[b]).sum())
                assert diff == 0, f"{what}: image {b} ({kinds[b]}): {diff} uint8 pixels differ from numpy float32"
        o = out.view(B, n, K)
        _within(o[keep], ref[keep], mag[keep], 4, f"{what} quantised{'' if with_u8 else ' (no u8out)'}",
                floor=2.0 ** -11 * ref[keep].abs() + HALF_FLOOR)
    # quantise = 0 (ProtoMedSAM): (v - lo) / (hi - lo), mean 0 / std 1
    lo = torch.from_numpy(lohi[:, 0].astype(np.float64)).view(B, 1, 1, 1)
    hi = torch.from_numpy(lohi[:, 1].astype(np.float64)).view(B, 1, 1, 1)
    with np.errstate(all="ignore"):
        q = (img.double() - lo) / (hi - lo)
    for b in skip:
        q[b] = 0.0
    ref = R.patchify(q, P, K).view(B, n, K)
    out = _nan((B * n, K), dev, torch.float16)
    ops.sam_patchify(imgd, mm, S, P, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], quantise=False, out=out)
    _within(out.view(B, n, K)[keep], ref[keep], ref[keep].abs(), 4, f"{what} unquantised",
            floor=2.0 ** -11 * ref[keep].abs() + HALF_FLOOR)


@pytest.mark.parametrize("kinds", [("random", "k", "k255"), ("narrow", "random", "k"), ("k255", "narrow", "random")])
@pytest.mark.parametrize("S,P", [(1024, 16), (512, 16), (32, 16)])
def test_sam_patchify(dev, S, P, kinds):
    """u8out equals numpy float32's ((x - lo) / (hi - lo) * 255).astype(uint8) at every pixel (both sides read the same fp32 bits and
    the same min / max). Patches: |out - ref| <= 2^-11 |ref| + 4 x 2^-23 (|q| + |mean|) / sd + 2^-25 against the float64
    normalisation of the same uint8 values; quantise = 0 likewise against float64 (v - lo) / (hi - lo). B = 3, a different range
    per image. Measured: no uint8 pixel differs; the patches stay inside the fp16 rounding term alone."""
    _check_sam_patchify(dev, S, P, kinds, S + len(kinds[0]))


@pytest.mark.parametrize("S", [32, 512])
def test_sam_patchify_constant_image_leaves_the_others_alone(dev, S):
    """A constant image (range 0) as image 1 of 3: the call returns 0, images 0 and 2 are written in full and within bounds. What
    image 1 holds is not asserted (the reference divides by zero there too)."""
    _check_sam_patchify(dev, S, 16, ("random", "constant", "k255"), S, skip=(1,))


# ---- 7. psam_normalize_chw ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 255), (257, 1), (37, 53), (1024, 1024)])
def test_normalize_chw(dev, H, W, B, u8):
    """(x - mean[c]) / std[c]: 2 x 2^-23 x (|x| + |mean|) / std (one subtraction, one division). Measured worst 0.95."""
    from protosam_amd import ops
    g = torch.Generator().manual_seed(H + W + B)
    x = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8) if u8 else _rand((B, 3, H, W), H + B, 80.0) + 100.0
    out = _nan((B, 3, H, W), dev)
    ops.normalize_chw(x.to(dev), PIXEL_MEAN, PIXEL_STD, out=out)
    # the kernel receives the constants as fp32
    mean = torch.tensor(PIXEL_MEAN, dtype=torch.float32).double()
    std = torch.tensor(PIXEL_STD, dtype=torch.float32).double()
    ref = R.normalise(x, mean, std)
    mag = (x.double().abs() + mean.view(3, 1, 1)) / std.view(3, 1, 1)
    _within(out, ref, mag, 2, f"normalize_chw {'u8' if u8 else 'f32'} B={B} {H}x{W}")


# ---- 8. psam_im2col3x3 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C", [8, 256])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (5, 7), (32, 32), (64, 64)])
def test_im2col3x3(dev, H, W, C, B):
    """Exact. The input holds no zeros, so every zero of the output is a padding tap."""
    from protosam_amd import ops
    x = _rand((B, H * W, C), H * W + C).half()
    x[x == 0] = 1.0
    out = _nan((B * H * W, 9 * C), dev, torch.float16)
    ops.im2col3x3(x.to(dev), B, H, W, C, out=out)
    ref = R.im2col3x3(x, B, H, W, C)
    assert torch.equal(out.cpu().view(torch.int16), ref.view(torch.int16))
    assert int((ref == 0).sum()) == B * C * (9 * H * W - (3 * H - 2) * (3 * W - 2))


# ---- 9. element-wise passes ---------------------------------------------------------------------------------------------
SIZES = [8, 8 * 256, 8 * 257, 1000 * 64]     # one lane, one full workgroup, a partly filled last one, many


def _halves():
    """Every finite half as fp32, by bit pattern."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32)
    bits = bits[(bits & 0x7C00) != 0x7C00]
    assert bits.numel() == 63488
    return bits.to(torch.int16).view(torch.float16)


def _cast_pool(seed):
    h = _halves().float()
    nxt = (_halves().view(torch.int16) + 1).view(torch.float16).float()       # next half away from zero (inf after 65504: dropped)
    mid = ((h + nxt) / 2)[torch.isfinite(nxt)]                                 # exactly halfway: round to even, both ways
    special = torch.tensor([0.0, -0.0, 65504.0, 65519.996, 65520.0, 65536.0, 1e5, -65520.0, -1e5, 3.4e38, 2.0 ** -25,
                            2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -26, -2.0 ** -25, 2.0 ** -24, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24,
                            2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12)])
    g = torch.Generator().manual_seed(seed)
    rest = torch.cat([mid, torch.nextafter(mid, torch.zeros_like(mid)), torch.nextafter(mid, torch.full_like(mid, 1e30)),
                      torch.randn(20000, generator=g) * 10.0, torch.randn(5000, generator=g) * 1e-6])
    return torch.cat([special, rest[torch.randperm(rest.numel(), generator=g)]])


@pytest.mark.parametrize("n", SIZES + [0])
def test_cast_f16_bits(dev, n):
    """fp32 -> half, bit-equal to x.half(): both zeros, overflow to inf, half subnormals (the first elements of every size), then in
    random order every exact halfway case between two halves (round to even, both ways) with its two fp32 neighbours, and random
    values. n = 0: the whole pool."""
    from protosam_amd import ops
    pool = _cast_pool(n)
    n = n or pool.numel() // 8 * 8
    x = pool[:n]
    out = _nan((n,), dev, torch.float16)
    ops.cast_f16(x.to(dev), out=out)
    assert torch.equal(out.cpu().view(torch.int16), x.half().view(torch.int16))


@pytest.mark.parametrize("n", SIZES[:3] + [63488])
def test_cast_f32_bits(dev, n):
    """half -> fp32, bit-equal to h.float(); 63 488 elements: every finite half bit pattern."""
    from protosam_amd import ops
    h = _halves()
    h = h[:n] if n == 63488 else h[torch.randperm(h.numel(), generator=torch.Generator().manual_seed(n))[:n]]
    out = _nan((n,), dev)
    ops.cast_f32(h.to(dev), out=out)
    assert torch.equal(out.cpu().view(torch.int32), h.float().view(torch.int32))


@pytest.mark.parametrize("n", SIZES)
def test_split_f16(dev, n):
    """hi bit-equal to x.half(), lo bit-equal to half(x - float(hi)). With write_hi = False and a hi that is the neighbouring half
    of x, hi comes back unchanged and lo is relative to it. float(hi) + float(lo) carries x to 2^-22 |x| for |x| in [2^-10, 6e4] -
    plus 2^-25, half the spacing of the subnormal halves, which lo is for |x| < 2^-3 (the exact reference needs that term too:
    test_resample_reference_cpu.py::test_split_f16)."""
    from protosam_amd import ops
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 10.0 ** torch.randint(-3, 5, (n,), generator=g).float()
    x = x.clamp(-6e4, 6e4)
    x[:4] = torch.tensor([0.0, -0.0, 1.0, -2.0 ** -10])
    xd = x.to(dev)
    hi, lo = _nan((n,), dev, torch.float16), _nan((n,), dev, torch.float16)
    ops.split_f16(xd, hi=hi, lo=lo)
    rhi, rlo = R.split_f16(x)
    assert torch.equal(hi.cpu().view(torch.int16), rhi.view(torch.int16))
    assert torch.equal(lo.cpu().view(torch.int16), rlo.view(torch.int16))
    inr = (x.abs() >= 2.0 ** -10) & (x.abs() <= 6e4)
    err = (hi.cpu().double() + lo.cpu().double() - x.double()).abs()
    assert bool((err <= 2.0 ** -22 * x.double().abs() + HALF_FLOOR)[inr].all())
    assert bool((err <= 2.0 ** -22 * x.double().abs())[inr & (rlo.float().abs() >= 2.0 ** -14)].all())
    nb = (rhi.view(torch.int16) + 1).view(torch.float16)          # the neighbouring half (away from zero)
    hi2, lo2 = nb.to(dev), _nan((n,), dev, torch.float16)
    ops.split_f16(xd, hi=hi2, lo=lo2, write_hi=False)
    assert torch.equal(hi2.cpu().view(torch.int16), nb.view(torch.int16)), "write_hi = False wrote hi"
    assert torch.equal(lo2.cpu().view(torch.int16), R.split_f16(x, hi=nb)[1].view(torch.int16))
    assert not torch.equal(lo2.cpu().view(torch.int16), rlo.view(torch.int16))


@pytest.mark.parametrize("n", SIZES)
def test_gelu_f32(dev, n):
    """0.5 x (1 + erf(x / sqrt 2)) in place: c x 2^-23 x |x| against float64, c = 8 (three roundings and an erff of a few ulp).
    Measured on an MI355X: 0.95 at worst; fp32 F.gelu on the CPU needs 2.64 on the same data (printed beside it)."""
    from protosam_amd import ops
    x = torch.cat([torch.linspace(-12.0, 12.0, n // 2), _rand((n - n // 2,), n, 3.0)])
    ref = R.gelu_erf(x)
    cpu = ((F.gelu(x).double() - ref).abs() / x.double().abs().clamp_min(1e-300)).max().item() / U
    xd = x.clone().to(dev)
    ops.gelu_f32_(xd)
    w = _within(xd, ref, x.double().abs(), 8, f"gelu_f32 n={n}")
    print(f"gelu_f32 n={n}: fp32 F.gelu on the CPU needs {cpu:.2f} of the same units (kernel {w:.2f})")


@pytest.mark.parametrize("D", [1, 255, 768, 1000])
def test_broadcast_rows(dev, D):
    """The D elements of each row equal the source; every other element of `out` still holds its NaN."""
    from protosam_amd import ops
    B, stride, off = 3, D + 37, 5
    row = _rand((D,), D)
    out = _nan((B * stride,), dev)
    ops.broadcast_rows(row.to(dev), out, B, stride, off)
    o = out.cpu().view(B, stride)
    assert torch.equal(o[:, off:off + D], row.expand(B, D))
    assert bool(o[:, :off].isnan().all()) and bool(o[:, off + D:].isnan().all())


# ---- 10. arguments ------------------------------------------------------------------------------------------------------
def test_rejections_return_status_1_before_any_launch(dev):
    """Every rejection of the header returns status 1 and leaves the NaN-filled outputs untouched. Only rejections that return before
    a launch are here; nothing launches with bad sizes."""
    import ctypes
    from protosam_amd import _lib, ops
    f32 = lambda *s: torch.ones(s, dtype=torch.float32, device=dev)  # noqa: E731
    f16 = lambda *s: torch.ones(s, dtype=torch.float16, device=dev)  # noqa: E731
    N = lambda *s, dt=torch.float32: _nan(s, dev, dt)  # noqa: E731
    H = torch.float16
    cases = []

    def case(name, fn, *outs):
        cases.append((name, fn, outs))

    o = N(16, dt=H); case("cast_f16 n % 8", lambda o=o: ops.cast_f16(f32(12), out=o), o)
    o = N(16); case("cast_f32 n % 8", lambda o=o: ops.cast_f32(f16(12), out=o), o)
    o1, o2 = N(16, dt=H), N(16, dt=H); case("split_f16 n % 8", lambda a=o1, b=o2: ops.split_f16(f32(12), hi=a, lo=b), o1, o2)
    o = N(8); case("gelu_f32 n % 4", lambda o=o: ops.gelu_f32_(o[:6]), o)
    o = N(8, 640, dt=H)
    case("patchify_bilinear S % P", lambda o=o: ops.patchify_bilinear(f32(1, 3, 28, 28), 30, 14, 640, out=o), o)
    case("patchify_bilinear Kpad < C*P*P", lambda o=o: ops.patchify_bilinear(f32(1, 3, 28, 28), 28, 14, 584, out=o), o)
    case("patchify_bilinear B = 0", lambda o=o: ops.patchify_bilinear(f32(0, 3, 28, 28), 28, 14, 640, out=o), o)
    case("patchify_bilinear H = 0", lambda o=o: ops.patchify_bilinear(f32(1, 3, 0, 28), 28, 14, 640, out=o), o)
    case("patchify_bilinear W = 0", lambda o=o: ops.patchify_bilinear(f32(1, 3, 28, 0), 28, 14, 640, out=o), o)
    case("patchify_bilinear S = 0", lambda o=o: ops.patchify_bilinear(f32(1, 3, 28, 28), 0, 14, 640, out=o), o)
    case("patchify_bilinear P = 0", lambda o=o: ops.patchify_bilinear(f32(1, 3, 28, 28), 28, 0, 640, out=o), o)
    o = N(2, 8, 8)
    case("resize2d mode = 3", lambda o=o: ops.resize2d(f32(2, 4, 4), 8, 8, 3, out=o), o)
    case("resize2d mode = -1", lambda o=o: ops.resize2d(f32(2, 4, 4), 8, 8, -1, out=o), o)
    case("resize2d planes = 0", lambda o=o: ops.resize2d(f32(0, 4, 4), 8, 8, 1, out=o), o)
    case("resize2d OH = 0", lambda o=o: ops.resize2d(f32(2, 4, 4), 0, 8, 2, out=o), o)
    case("bilinear_nchw planes = 0", lambda o=o: ops.bilinear_nchw(f32(0, 4, 4), 8, 8, out=o), o)
    case("bilinear_nchw OW = 0", lambda o=o: ops.bilinear_nchw(f32(2, 4, 4), 8, 0, out=o), o)
    p, q = N(1, 2, 8, 8), _a5((1, 8, 8), dev)
    for name, lg, oh, ow in (("B = 0", (0, 2, 4, 4), 8, 8), ("IH = 0", (1, 2, 0, 4), 8, 8), ("IW = 0", (1, 2, 4, 0), 8, 8),
                             ("OH = 0", (1, 2, 4, 4), 0, 8), ("OW = 0", (1, 2, 4, 4), 8, 0)):
        case(f"prob_argmax {name}", lambda lg=lg, oh=oh, ow=ow, p=p, q=q: ops.prob_argmax(f32(*lg), oh, ow, prob=p, pred=q), p, q)
    o = N(4, 72, dt=H)
    case("im2col3x3 C % 8", lambda o=o: ops.im2col3x3(f16(1, 4, 4), 1, 2, 2, 4, out=o), o)
    case("im2col3x3 C = 0", lambda o=o: ops.im2col3x3(f16(1, 4, 8), 1, 2, 2, 0, out=o), o)
    case("im2col3x3 B = 0", lambda o=o: ops.im2col3x3(f16(1, 4, 8), 0, 2, 2, 8, out=o), o)
    case("im2col3x3 H = 0", lambda o=o: ops.im2col3x3(f16(1, 4, 8), 1, 0, 2, 8, out=o), o)
    case("im2col3x3 W = 0", lambda o=o: ops.im2col3x3(f16(1, 4, 8), 1, 2, 0, 8, out=o), o)
    mm = ops.minmax(f32(1, 3, 32, 32) * torch.arange(32, device=dev), 1)
    o, u = N(4, 768, dt=H), _a5((1, 3, 40, 40), dev)
    case("sam_patchify S % P", lambda o=o, u=u: ops.sam_patchify(f32(1, 3, 40, 40), mm, 40, 16, PIXEL_MEAN, PIXEL_STD, out=o, u8out=u), o, u)
    case("sam_patchify P = 0", lambda o=o, u=u: ops.sam_patchify(f32(1, 3, 32, 32), mm, 32, 0, PIXEL_MEAN, PIXEL_STD, out=o, u8out=u), o, u)
    case("sam_patchify S = 0", lambda o=o, u=u: ops.sam_patchify(f32(1, 3, 0, 0), mm, 0, 16, PIXEL_MEAN, PIXEL_STD, out=o, u8out=u), o, u)
    case("sam_patchify B = 0", lambda o=o, u=u: ops.sam_patchify(f32(0, 3, 32, 32), mm, 32, 16, PIXEL_MEAN, PIXEL_STD, out=o, u8out=u), o, u)
    img = f32(1, 3, 32, 32)
    three = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    for name, m, s in (("mean3 NULL", None, three), ("std3 NULL", three, None)):       # ops always passes both: straight to the library
        def direct(m=m, s=s, o=o, u=u):
            st = _lib.lib().psam_sam_patchify(img.data_ptr(), mm.data_ptr(), 1, 32, 16, m, s, 1, o.data_ptr(), u.data_ptr(), None)
            _lib.check(st, "psam_sam_patchify")
        case(f"sam_patchify {name}", direct, o, u)
    o = N(2)
    case("minmax n_per_img = 0", lambda: ops.minmax(f32(0), 1, mm=_a5((2,), dev, torch.int32)))
    o = N(64)
    case("broadcast_rows B = 0", lambda o=o: ops.broadcast_rows(f32(8), o, 0, 16, 0), o)
    case("broadcast_rows D = 0", lambda o=o: ops.broadcast_rows(f32(0), o, 2, 16, 0), o)
    o = N(1, 3, 4, 4)
    case("normalize_chw B = 0", lambda o=o: ops.normalize_chw(f32(0, 3, 4, 4), PIXEL_MEAN, PIXEL_STD, out=o), o)
    case("normalize_chw plane = 0", lambda o=o: ops.normalize_chw(f32(1, 3, 0, 4), PIXEL_MEAN, PIXEL_STD, out=o), o)
    o = N(2, 16, 8)
    tok = f32(2, 9, 8)
    for name, a in (("B = 0", (0, 3, 3, 8, 4, 4)), ("C = 0", (2, 3, 3, 0, 4, 4)), ("ih = 0", (2, 0, 3, 8, 4, 4)),
                    ("iw = 0", (2, 3, 0, 8, 4, 4)), ("oh = 0", (2, 3, 3, 8, 0, 4)), ("ow = 0", (2, 3, 3, 8, 4, 0))):
        case(f"bilinear_tokens {name}", lambda a=a, o=o: ops.bilinear_tokens(tok, 72, 8, *a, out=o), o)
    for name, fn, outs in cases:
        with pytest.raises(RuntimeError, match="status 1"):
            fn()
        torch.cuda.synchronize()
        for t in outs:
            if t.dtype.is_floating_point:
                assert bool(t.isnan().all()), f"{name}: output written"
            else:
                assert bool((t == 0xA5).all()), f"{name}: output written"
    print(f"{len(cases)} rejections, each status 1 with its outputs untouched")


def test_misaligned_views_are_refused_on_the_host(dev):
    """The 16-byte passes and the vector store path of prob_argmax need aligned base pointers: a contiguous view that starts 4 (or,
    for halves, 2) bytes into a storage raises before any call into the library. Where the kernel has no such need (prob_argmax with
    OW % 4 != 0, minmax on any 4-byte boundary) the same view is accepted and right."""
    from protosam_amd import ops
    x = torch.arange(33, dtype=torch.float32, device=dev)
    h = torch.arange(34, dtype=torch.float16, device=dev)
    o16, o32 = _nan((34,), dev, torch.float16), _nan((33,), dev)
    bad = [lambda: ops.cast_f16(x[1:17], out=o16[:16]), lambda: ops.cast_f16(x[:16], out=o16[1:17]),
           lambda: ops.cast_f32(h[1:17], out=o32[:16]), lambda: ops.cast_f32(h[:16], out=o32[1:17]),
           lambda: ops.gelu_f32_(o32[1:17]),
           lambda: ops.split_f16(x[1:17], hi=o16[:16], lo=o16[16:32]), lambda: ops.split_f16(x[:16], hi=o16[1:17], lo=o16[16:32]),
           lambda: ops.split_f16(x[:16], hi=o16[:16], lo=o16[17:33])]
    for fn in bad:
        with pytest.raises(ValueError, match="aligned"):
            fn()
    l = _rand((1, 2, 4, 8), 3).to(dev)
    pbuf, qbuf = _nan((2 * 4 * 8 + 1,), dev), _a5((4 * 8 + 1,), dev)
    with pytest.raises(ValueError, match="aligned"):
        ops.prob_argmax(l, 4, 8, prob=pbuf[1:].view(1, 2, 4, 8), pred=qbuf[:32].view(1, 4, 8))
    with pytest.raises(ValueError, match="aligned"):
        ops.prob_argmax(l, 4, 8, prob=pbuf[:64].view(1, 2, 4, 8), pred=qbuf[1:].view(1, 4, 8))
    torch.cuda.synchronize()
    assert bool(o16.isnan().all()) and bool(o32.isnan().all()) and bool(pbuf.isnan().all()) and bool((qbuf == 0xA5).all())
    # OW % 4 != 0: per-pixel stores, any alignment
    l = _rand((1, 2, 4, 7), 4).to(dev)
    pbuf, qbuf = _nan((2 * 4 * 7 + 1,), dev), _a5((4 * 7 + 1,), dev)
    prob, pred = ops.prob_argmax(l, 4, 7, prob=pbuf[1:].view(1, 2, 4, 7), pred=qbuf[1:].view(1, 4, 7))
    prob_a, pred_a = ops.prob_argmax(l, 4, 7)
    assert torch.equal(prob, prob_a) and torch.equal(pred, pred_a) and bool(pbuf[0].isnan()) and int(qbuf[0]) == 0xA5
    # minmax: the kernel takes the scalar path
    mm = ops.minmax(x[1:], 1)
    assert R.ord_decode(mm.cpu().numpy()).tolist() == [1.0, 32.0]
