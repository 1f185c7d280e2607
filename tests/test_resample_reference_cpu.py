"""oracle/resample.py against stock torch on the CPU. The GPU tests of the resampling kernels (test_resample_kernels_gpu.py) bound a
kernel's error by multiples of 2^-23 times the magnitudes these references return; here the same bounds are shown to hold for ATen's
own fp32 implementation, so they are bounds of the arithmetic and not of our kernels, and the exact references are shown to be exact.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import resample as R

U = 2.0 ** -23

# (IH, IW, OH, OW)
BILINEAR_SHAPES = [(36, 36, 512, 512), (512, 512, 1024, 1024), (73, 73, 1024, 1024), (300, 517, 1024, 1024),
                   (1024, 1024, 256, 256), (640, 480, 37, 53), (7, 5, 3, 2), (1, 1, 9, 9), (64, 64, 64, 64),
                   (256, 256, 1001, 999)]


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("IH,IW,OH,OW", BILINEAR_SHAPES)
def test_bilinear_bounds_hold_for_aten_fp32(IH, IW, OH, OW, align):
    """fp32 F.interpolate lies within 2 x 2^-23 x (blend + weights) of the float64 restatement (measured worst over these shapes and seeds:
    0.78). With `blend` alone as the magnitude the strongly non-integer ratios need thousands of units, which is why `weights`
    exists."""
    x = _rand((2, IH, IW), IH * 7 + OW + int(align), 5.0)
    ref, blend, weights = R.bilinear(x, OH, OW, align)
    got = F.interpolate(x[None], size=(OH, OW), mode="bilinear", align_corners=align)[0].double()
    ratio = ((got - ref).abs() / (blend + weights).clamp_min(1e-300)).max().item() / U
    print(f"ATen fp32 bilinear {IH}x{IW}->{OH}x{OW} align={align}: worst {ratio:.2f} x 2^-23 x (blend + weights)")
    assert ratio <= 2.0
    # float64 ATen takes the scale in float64, not as the fp32 quotient: half an fp32 ulp of the coordinate, nothing else, apart
    ref64 = F.interpolate(x.double()[None], size=(OH, OW), mode="bilinear", align_corners=align)[0]
    assert ((ref64 - ref).abs() <= U * weights + 1e-12 * blend).all()


@pytest.mark.parametrize("I,O", [(256, 1001), (3, 7), (1024, 640), (64, 1024), (5, 4099), (64, 64), (1, 9)])
def test_nearest_is_aten_nearest(I, O):
    x = _rand((2, I, I), I + O)
    assert torch.equal(R.nearest(x, O, O), F.interpolate(x[None], size=(O, O), mode="nearest")[0])
    y = _rand((1, I, 5), I)
    assert torch.equal(R.nearest(y, 3, O), F.interpolate(y[None], size=(3, O), mode="nearest")[0])


def test_softmax2_argmax():
    l = _rand((2, 50, 60), 3, 4.0)
    l[1, :10] = l[0, :10]                       # ties
    p0, p1, am, margin = R.softmax2_argmax(l[0], l[1])
    sm = torch.softmax(l.double(), 0)
    assert torch.allclose(p0, sm[0], rtol=1e-14, atol=0) and torch.allclose(p1, sm[1], rtol=1e-14, atol=0)
    assert torch.equal(am.long(), l.double().argmax(0)) and int(am[:10].sum()) == 0
    assert torch.equal(margin, (l[1].double() - l[0].double()).abs())
    p0, p1, am, _ = R.softmax2_argmax(torch.tensor([80.0, -1e4]), torch.tensor([-80.0, 1e4]))
    assert p0.tolist() == [1.0, 0.0] and p1[1].item() == 1.0 and am.tolist() == [0, 1]


@pytest.mark.parametrize("H,W,C,B", [(1, 1, 8, 1), (1, 9, 8, 2), (5, 7, 16, 2), (32, 32, 8, 1)])
def test_im2col3x3_is_unfold(H, W, C, B):
    x = _rand((B, H * W, C), H + W)
    ref = F.unfold(x.view(B, H, W, C).permute(0, 3, 1, 2), 3, padding=1)            # [B, C*9, H*W], row c*9 + tap
    ref = ref.view(B, C, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9 * C)
    assert torch.equal(R.im2col3x3(x, B, H, W, C), ref)


@pytest.mark.parametrize("S,P,Kpad,C", [(28, 14, 640, 3), (32, 16, 768, 3), (64, 16, 800, 3), (28, 14, 196, 1)])
def test_patchify_is_unfold(S, P, Kpad, C):
    x = _rand((2, C, S, S), S + P)
    ref = F.unfold(x, P, stride=P).transpose(1, 2).reshape(-1, C * P * P)
    out = R.patchify(x, P, Kpad)
    assert out.shape == (2 * (S // P) ** 2, Kpad)
    assert torch.equal(out[:, :C * P * P], ref) and bool((out[:, C * P * P:] == 0).all())


def test_quantise_is_glue_quantise_image():
    from oracle import glue
    for seed, scale, shift in ((1, 1.0, 0.0), (2, 40.0, -3.0), (3, 1e-3, 1e3)):
        img = _rand((1, 3, 64, 48), seed, scale) + shift
        ref = glue.quantise_image(img)                                            # HWC uint8
        out = R.quantise(img[0].numpy(), img.min().item(), img.max().item())
        assert out.dtype == np.uint8 and np.array_equal(out.transpose(1, 2, 0), ref)
        assert out.min() == 0 and out.max() == 255


def test_normalise_and_gelu():
    x = _rand((2, 3, 5, 7), 4, 50.0)
    mean, std = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
    ref = (x.double() - torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    assert torch.equal(R.normalise(x, mean, std), ref)
    v = torch.cat([torch.linspace(-12, 12, 4001), _rand((4000,), 5, 3.0)]).double()
    assert ((R.gelu_erf(v) - F.gelu(v)).abs() <= 1e-15 * v.abs()).all()      # 1 + erf cancels in the negative tail: absolute in |x|


def test_split_f16():
    x = _rand((4096,), 6, 10.0)
    hi, lo = R.split_f16(x)
    assert torch.equal(hi, x.half()) and torch.equal(lo, (x - x.half().float()).half())
    # hi + lo carries x to 2^-22 |x|, plus half the spacing of the subnormal halves (2^-25) where lo is one (|x| below 2^-3)
    err = (hi.double() + lo.double() - x.double()).abs()
    assert (err <= 2.0 ** -22 * x.double().abs() + 2.0 ** -25).all()
    assert (err <= 2.0 ** -22 * x.double().abs())[lo.float().abs() >= 2.0 ** -14].all()
    up = (hi.view(torch.int16) + 1).view(torch.float16)                       # the neighbouring half, away from zero
    hi2, lo2 = R.split_f16(x, hi=up)
    assert hi2 is up and torch.equal(lo2, (x - up.float()).half())


def test_ord_code_round_trips_and_orders():
    """ord_decode(f2ord(x)) == x bit for bit, with f2ord restated here from its definition (sign bit set -> complement, else set the
    sign bit); the code is monotone, which is what lets atomicMin / atomicMax on it find the float extremes."""
    vals = np.array([-np.inf, -3.4e38, -1.5, -1e-40, -0.0, 0.0, 1e-45, 1e-40, 1.17549435e-38, 1.0, 65504.0, 3.4e38, np.inf],
                    dtype=np.float32)
    u = vals.view(np.uint32)
    enc = np.where(u >> 31 == 1, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    assert np.array_equal(enc, R.ord_encode(vals))
    dec = R.ord_decode(enc)
    assert dec.dtype == np.float32 and np.array_equal(dec.view(np.uint32), u)
    assert np.array_equal(R.ord_decode(enc.view(np.int32)).view(np.uint32), u)    # the int32 tensor ops.minmax returns
    assert bool((np.diff(enc.astype(np.int64)) > 0).all())                        # vals ascend (-0 < +0 in the code)
