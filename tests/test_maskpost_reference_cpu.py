"""oracle/maskpost.py against stock torch on the CPU. The GPU tests of the mask post-processing kernels (test_mask_kernels_gpu.py)
hold each kernel to these references: the values within multiples of 2^-23 times the magnitudes returned here, the thresholded bits
wherever the float64 value is further from the threshold than that bound. Here the same bounds are shown to hold for ATen's own fp32
kernels, the exact parts are shown to be exact, and every input of the GPU tests is built and shown to leave at most 1e-4 of its
pixels inside the error band - otherwise a GPU test would pass without testing anything.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import maskpost as M
from oracle import resample as R

U = 2.0 ** -23
SHAPES = sorted({c[:2] for c in M.CASES}) + [(16, 128)]


def _aten(x, MID, variant, dtype):
    x = x.to(dtype)
    if variant == 2:
        return F.interpolate(x[None], size=(MID, MID), mode="nearest")[0]
    if variant == 3:
        x = torch.sigmoid(x)
    return F.interpolate(x[None], size=(MID, MID), mode="bilinear", align_corners=(variant == 1))[0]


@pytest.mark.parametrize("variant", [0, 1, 3])
@pytest.mark.parametrize("IN,MID", SHAPES)
def test_up_sample_is_aten(IN, MID, variant):
    """float64 F.interpolate (after torch.sigmoid for variant 3) equals the reference to 1e-12 of the magnitude where the fp32 scale
    the kernels use is the exact quotient; elsewhere float64 ATen takes the quotient in float64, which moves the source coordinate by
    up to half an fp32 ulp: one unit of `weights` more. fp32 ATen stays inside the bound of the GPU test, 4 x 2^-23 x magnitude
    (+ 2^-126 for variant 3); measured worst 1.33 (variants 0, 1), 0.73 (variant 3)."""
    thr, off = M.THRESHOLDS[variant][0]
    x, ref, mag = M.case_reference(IN, MID, variant, thr, off) if (IN, MID) != (16, 128) else \
        (M.planes(IN, variant),) + M.up_sample(M.planes(IN, variant), MID, variant)
    a, b = (IN - 1, max(MID - 1, 1)) if variant == 1 else (IN, MID)
    exact_scale = float(np.float32(a) / np.float32(b)) == a / b
    got64 = _aten(x, MID, variant, torch.float64)
    slack = 0.0 if exact_scale else U
    assert bool(((got64 - ref).abs() <= (1e-12 + slack) * mag + 1e-300).all())
    if exact_scale:
        assert bool(((got64 - ref).abs() <= 1e-12 * ref.abs().clamp_min(1.0)).all())
    got32 = _aten(x, MID, variant, torch.float32).double()
    floor = 2.0 ** -126 if variant == 3 else 0.0
    ratio = (((got32 - ref).abs() - floor).clamp_min(0) / mag.clamp_min(1e-300)).max().item() / U
    print(f"ATen fp32 variant {variant} {IN}->{MID}: worst {ratio:.2f} x 2^-23 x magnitude")
    assert ratio <= M.C_BOUND


@pytest.mark.parametrize("IN,MID", SHAPES)
def test_up_sample_nearest_is_aten(IN, MID):
    x = M.planes(IN, 2)
    v, mag = M.up_sample(x, MID, 2)
    assert torch.equal(v, _aten(x, MID, 2, torch.float64)) and not bool(mag.any())


@pytest.mark.parametrize("IN,MID", [(16, 128), (64, 256)])
def test_integer_planes_are_exact_in_fp32(IN, MID):
    """Integer logits at a power-of-two ratio: ATen's fp32 result equals the float64 reference bit for bit (so there is no band),
    and the planes hold pixels exactly equal to 0."""
    x = M.integer_planes(IN)
    for variant in (0, 2):
        ref, _ = M.up_sample(x, MID, variant)
        assert torch.equal(_aten(x, MID, variant, torch.float32).double(), ref)
        assert int((ref == 0).sum()) > 50


def test_threshold_band_logic_by_hand():
    """A 4 x 4 case with a known answer: c = 4, t = 1; magnitude 2^20 makes the half-width of the band 0.5."""
    big = 2.0 ** 20
    value = torch.tensor([[1.0, 1.0, 1.6, 0.4], [1.5, 0.5, 1.0 + 2.0 ** -40, 1.0 - 2.0 ** -40], [3.0, -3.0, 1.2, 0.8], [1.0, 1.0, 1.0, 1.0]],
                         dtype=torch.float64)
    mag = torch.tensor([[0.0, big, big, big], [big, big, 0.0, 0.0], [big, big, big, big], [0.0, 0.0, big, 0.0]], dtype=torch.float64)
    s1, s0, band = M.threshold(value, mag, 1.0, 4)
    want1 = torch.tensor([[0, 0, 1, 0], [0, 0, 1, 0], [1, 0, 0, 0], [0, 0, 0, 0]], dtype=torch.bool)
    want0 = torch.tensor([[1, 0, 0, 1], [0, 0, 0, 1], [0, 1, 0, 0], [1, 1, 0, 1]], dtype=torch.bool)
    assert torch.equal(s1, want1) and torch.equal(s0, want0) and torch.equal(band, ~(want1 | want0))
    assert int(band.sum()) == 6                                   # the tie with a magnitude, both edges 1.5 / 0.5, 1.2, 0.8, and the tie in row 3
    lo, hi, inner, outer = M.counts_and_boxes(s1, band)
    assert (int(lo), int(hi)) == (3, 9)
    assert inner.tolist() == [0, 0, 2, 2] and outer.tolist() == [0, 0, 3, 3]
    e_lo, e_hi, e_in, e_out = M.counts_and_boxes(torch.zeros(2, 3, 3, dtype=torch.bool), torch.zeros(2, 3, 3, dtype=torch.bool))
    assert e_lo.tolist() == [0, 0] and e_hi.tolist() == [0, 0]
    assert e_in.tolist() == [[M.INT_MAX, M.INT_MAX, -1, -1]] * 2 and e_out.tolist() == e_in.tolist()
    b = torch.tensor([0, 0, 2, 3])                                # a box between the two
    assert bool(M.box_between(b, inner, outer)) and not bool(M.box_between(torch.tensor([1, 0, 2, 2]), inner, outer))
    assert not bool(M.box_between(torch.tensor([0, 0, 2, 4]), inner, outer))
    assert M.thr32(0.3) == float(np.float32(0.3)) != 0.3
    assert M.thr32(0.3, 1.0, -1) == float(np.float32(0.3) - np.float32(1.0)) and M.thr32(0.3, 1.0, 1) == float(np.float32(1.3))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("IN,MID", [(16, 64), (20, 77), (3, 1)])
def test_union_is_the_reference_lines(IN, MID, B):
    """models/ProtoSAM.py:669-676 with torch ops - pred = sum(masks) > 0, as float, F.interpolate(..., 'nearest') to the output
    size - on exactly known masks (variant 2 copies samples, so nothing is in the band)."""
    x = M.planes(IN, 2, 0.3, 1.0)[list(M.UNION_PROMPTS[B])]
    v, mag = M.up_sample(x, MID, 2)
    s1, s0, band = M.threshold(v, mag, M.thr32(0.3), M.C_BOUND)
    assert not bool(band.any())
    masks = [F.interpolate(x[b][None, None], size=(MID, MID), mode="nearest")[0, 0] > np.float32(0.3) for b in range(B)]
    pred = (sum(m.long() for m in masks) > 0).float()
    for OUT in M.union_outs(MID):
        want = F.interpolate(pred[None, None], size=(OUT, OUT), mode="nearest")[0, 0]
        u1, u0, ub = M.union_fold(s1, s0, OUT)
        assert torch.equal(u1, want == 1) and torch.equal(u0, want == 0) and not bool(ub.any())


def test_softmax2_twice():
    l = M.class_scores(3, 40, 50, 5)
    p0, p1, am, margin, q1 = M.softmax2_twice(l[:, 0], l[:, 1])
    sm = torch.softmax(l.double(), 1)
    sm2 = torch.softmax(sm, 1)
    assert torch.allclose(p0, sm[:, 0], rtol=1e-14, atol=0) and torch.allclose(p1, sm[:, 1], rtol=1e-14, atol=0)
    assert torch.allclose(q1, sm2[:, 1], rtol=1e-14, atol=0)
    assert torch.equal(am.long(), l.double().argmax(1)) and int(am[1].sum()) == 0 and int(am[2].sum()) == 0


def test_composed_resize_is_two_interpolates():
    x = M.class_scores(2, 16, 12, 3)[:, 0]
    v, mag = M.composed_resize(x, 64, 48, 251, 333)
    two = F.interpolate(F.interpolate(x.double()[None], size=(64, 48), mode="bilinear"), size=(251, 333), mode="bilinear")[0]
    assert bool(((v - two).abs() <= 2 * U * mag).all())              # float64 ATen: the float64 quotient as the scale, twice
    got = F.interpolate(F.interpolate(x[None], size=(64, 48), mode="bilinear"), size=(251, 333), mode="bilinear")[0].double()
    ratio = ((got - v).abs() / mag.clamp_min(1e-300)).max().item() / U
    print(f"ATen fp32 resize twice: worst {ratio:.2f} x 2^-23 x magnitude")
    assert ratio <= M.C_BOUND
    v1, m1 = M.composed_resize(x, 64, 48, 64, 48)
    r, b, w = R.bilinear(x, 64, 48)
    assert torch.equal(v1, r) and torch.equal(m1, b + w)


def test_pb_grid_straddles():
    assert M.pb_grid(5) == (5, 1) and M.pb_grid(2048) == (2048, 1) and M.pb_grid(2049) == (1025, 2)
    assert M.pb_grid(9 * 602) == (1806, 3) and M.pb_straddlers(301, 1100, 9) >= 4      # 602 items per plane in runs of three
    assert M.pb_straddlers(1025, 1025, 5) >= 1                                          # mask_union_seg: OUT = 1025, 5 segments
    assert M.pb_straddlers(251, 333, 3) == 0                                            # one item per workgroup: nothing to straddle


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("IN,MID,H,W", M.CASES)
def test_gpu_inputs_leave_the_band_almost_empty(IN, MID, H, W, variant):
    """Per case, variant and threshold used on the GPU: at most 1e-4 of the pixels of the float64 reference lie inside the band of
    c = 4 (measured worst 2.3e-5, none at all below IN = 64); the empty / full / island planes are what they are called; and the
    unions of mask_union / mask_union_seg inherit it."""
    for thr, off in M.THRESHOLDS[variant]:
        x, v, mag = M.case_reference(IN, MID, variant, thr, off)
        v, mag = v[:, :H, :W], mag[:, :H, :W]
        for sign in ((0,) if off == 0 else (-1, 0, 1)):
            s1, s0, band = M.threshold(v, mag, M.thr32(thr, off, sign), M.C_BOUND)
            share = int(band.sum()) / band.numel()
            print(f"{IN}->{MID} [{H}x{W}] variant {variant} t = {M.thr32(thr, off, sign):+.2f}: band share {share:.1e}")
            assert share <= 1e-4
            assert not bool(s1[M.EMPTY].any()) and bool(s1[M.FULL].all()) and not bool(band[[M.EMPTY, M.FULL, M.ISLAND]].any())
            assert 0 < int(s1[M.ISLAND].sum()) < H * W or IN < 3 or MID < 5
        s1, s0, _ = M.threshold(*M.case_reference(IN, MID, variant, thr, off)[1:], M.thr32(thr), M.C_BOUND)
        nb = n = 0                                   # pooled over B and OUT, as the GPU test asserts it: OUT = 1 is one pixel
        for B, prompts in M.UNION_PROMPTS.items():
            for OUT in M.union_outs(MID):
                ub = M.union_fold(s1[list(prompts)], s0[list(prompts)], OUT)[2]
                nb, n = nb + int(ub.sum()), n + ub.numel()
        assert nb / n <= 1e-4 and (nb == 0 or MID > 5)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_gpu_70_planes_leave_the_band_almost_empty(variant):
    v, mag = M.up_sample(M.planes70(variant), 64, variant)
    for sign in (-1, 0, 1):
        band = M.threshold(v[:, :50], mag[:, :50], M.thr32(0.3, 1.0, sign), M.C_BOUND)[2]
        assert int(band.sum()) / band.numel() <= 1e-4
        assert int((band.flatten(1).sum(1) == 0).sum()) >= 35


@pytest.mark.parametrize("case", M.PROB2_CASES + M.SCORES_CASES)
def test_gpu_class_scores_leave_the_band_almost_empty(case):
    """The argmax of every psam_prob2_argmax / psam_scores_prob_argmax case: at most 1e-4 of the untied pixels have a float64 margin
    inside 4 x 2^-23 (M0 + M1)."""
    P, OH, OW = case[0], case[-2], case[-1]
    l = M.case_scores(case)
    if len(case) == 5:
        same = case[1:3] == case[3:5]
        v, mag = (l.view(2 * P, *case[1:3]).double(), torch.zeros((2 * P, OH, OW), dtype=torch.float64)) if same else \
            (lambda r: (r[0], r[1] + r[2]))(R.bilinear(l.view(2 * P, *case[1:3]), OH, OW))
    else:
        v, mag = M.composed_resize(l.view(2 * P, *case[1:3]), *case[3:])
    v, mag = v.view(P, 2, OH, OW), mag.view(P, 2, OH, OW)
    margin = (v[:, 1] - v[:, 0]).abs()
    tie, sure, share = M.argmax_band(margin, mag[:, 0] + mag[:, 1])
    print(f"{case}: band share {share:.1e}, {int(tie.sum())} ties")
    assert share <= 1e-4 and int(tie.sum()) >= OH * OW
