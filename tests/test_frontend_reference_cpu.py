"""The references of oracle/frontend.py, pinned on the CPU: each one against stock code (oracle/slice_io.py's cv2 restatement,
F.unfold / F.max_pool2d / F.conv2d, oracle/rotate.py's torchvision restatement, F.interpolate(antialias=True)), and each stated
bound shown to hold for fp32 numpy / torch on the very inputs tests/test_frontend_kernels_gpu.py feeds the kernels. The rotation
inputs are also held to their band cap here: a condition on the inputs, not a tolerance (the GPU comparison is exact).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import frontend as FE
from oracle import rotate as orot
from oracle import slice_io

U = FE.U


def _ratio(err, bound):
    return float((np.asarray(err) / np.maximum(np.asarray(bound), 1e-300)).max())


# ---- psam_volume_stats ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0, 1, 2, 3])
@pytest.mark.parametrize("n", FE.STATS_SIZES[:4] + [100003])
def test_volume_stats_reference(dt, n):
    """slope 1 / intercept 0: both candidates coincide and equal the exact integer sums (Python ints) up to the one rounding of
    the pairwise sum; a sequential float64 sum (cumsum) of the fp32 values is within n 2^-53 x magnitude. slope 0.37 / intercept -12.5: numpy
    float32 (unfused) lies in the interval by construction, the interval is not empty, and its ends differ by at most one fp32
    rounding per voxel."""
    v = FE.stats_volume(dt, n, 10 * n + dt)
    if dt == 0 and n > 1:
        assert v.min() == -32768 and v.max() == 32767
    if dt == 3 and n > 4:
        assert int(np.abs(v.astype(np.int64)).max()) == 2 ** 31 and (np.abs(v.astype(np.int64)) > 2 ** 24).sum() >= 5
    r = FE.volume_stats64(v)
    assert r["unfused"] == r["fused"] == r["lo"] == r["hi"]
    es, eq = FE.exact_integer_sums(v)
    assert abs(r["lo"][0] - es) <= FE.SUM_SLACK * 2.0 ** -53 * r["mag"][0] and abs(r["lo"][1] - eq) <= FE.SUM_SLACK * 2.0 ** -53 * eq
    x = v.astype(np.float32).astype(np.float64)
    for k, got in enumerate((np.cumsum(x.ravel())[-1], np.cumsum((x * x).ravel())[-1])):
        assert abs(got - (es, eq)[k]) <= n * 2.0 ** -53 * r["mag"][k]
    r = FE.volume_stats64(v, 0.37, -12.5)
    x32 = v.astype(np.float32) * np.float32(0.37) + np.float32(-12.5)
    assert x32.dtype == np.float32
    x = x32.astype(np.float64).ravel()
    for k, got in enumerate((x.sum(), (x * x).sum())):
        tol = (n + FE.SUM_SLACK) * 2.0 ** -53 * r["mag"][k]
        assert r["lo"][k] - tol <= got <= r["hi"][k] + tol
    assert r["hi"][0] - r["lo"][0] <= 2 * U * r["mag"][0] and r["hi"][1] - r["lo"][1] <= 4 * U * r["mag"][1] * (1 + U)


# ---- psam_volume_slices --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0, 1, 2, 3])
@pytest.mark.parametrize("H,W,S", FE.SLICE_SHAPES)
def test_volume_slices_reference_vs_slice_io(H, W, S, dt):
    """Mode 1 equals oracle/slice_io.resize_nearest per slice; mode 0 holds oracle/slice_io.resize_linear (numpy float32) of the
    float32 normalisation inside its bound, with and without slope / intercept; the identity size returns the normalised input."""
    Z = 2
    lab = FE.label_volume(dt, Z, H, W, H + W + dt)
    assert lab.min() == 0 and lab.max() == 255
    ref = FE.volume_slices_ref(lab, 1.0, 0.0, 0.0, 1.0, S, 1)
    assert ref.dtype == np.float32
    for z in range(Z):
        assert np.array_equal(ref[z], slice_io.resize_nearest(lab[z], S).astype(np.float32))
    assert np.array_equal(FE.volume_slices_ref(lab, 2.0, 3.0, 0.0, 1.0, S, 1), 2 * ref + 3)      # the scaling is part of mode 1
    vol = FE.slice_volume(dt, Z, H, W, H * W + S + dt)
    for norm in (FE.SLICE_NORM, dict(slope=1.0, inter=0.0, mean=41.3, inv_std=1.0 / 57.9)):
        val, bound = FE.volume_slices_ref(vol, S=S, mode=0, **norm)
        n32 = FE.normalise32(vol, **norm)
        got = np.stack([slice_io.resize_linear(n32[z], S) for z in range(Z)])
        err = np.abs(got.astype(np.float64) - val)
        assert (err <= bound).all(), f"numpy float32 needs {_ratio(err, bound):.2f} of the bound"
        if norm["slope"] == 1.0 and (H, W) == (S, S):
            assert np.array_equal(got, n32)      # (bit for bit the fp32 normalisation; `val` is its float64 form, within the bound)


def test_volume_slices_exact_arithmetic_case():
    """Integer voxels, mean 0, 1 / std 1, S = 4 H = 2 W: every weight is a multiple of 1/8, every product and sum exact in fp32:
    the reference value is an fp32 number and numpy float32 reproduces it bit for bit."""
    H, W, S = 6, 12, 24
    vol = FE.slice_volume(0, 2, H, W, 5)
    for n_in in (H, W):
        w = FE.linear_taps(n_in, S)[2]
        assert np.array_equal(w * 8, np.round(w * 8)) and (w > 0).any()
    val, _ = FE.volume_slices_ref(vol, 1.0, 0.0, 0.0, 1.0, S, 0)
    assert np.array_equal(val.astype(np.float32).astype(np.float64), val)
    got = np.stack([slice_io.resize_linear(vol[z].astype(np.float32), S) for z in range(2)])
    assert np.array_equal(got.astype(np.float64), val)


# ---- the gathers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kh,kw,stride,dil,pad,H,W", FE.im2col_cases())
def test_im2col_ref_equals_unfold(kh, kw, stride, dil, pad, H, W):
    B, C = 2, 8
    for enc in (0, 1):
        x = FE.coded_map(B, H, W, C, enc)
        assert int((x == 0).sum()) == 0 and bool((x.float() == x.float().round()).all())
        ref = FE.im2col_ref(x, B, H, W, C, kh, kw, stride, dil, pad, kh * kw * C + 8)
        nchw = x.reshape(B, H, W, C).permute(0, 3, 1, 2).float()
        un = F.unfold(nchw, (kh, kw), dilation=dil, padding=pad, stride=stride)          # [B, C*kh*kw, L], (c, ky, kx) order
        L = un.shape[-1]
        un = un.view(B, C, kh * kw, L).permute(0, 3, 2, 1).reshape(B * L, kh * kw * C)
        assert ref.shape[0] == B * L and torch.equal(ref[:, :kh * kw * C].float(), un) and bool((ref[:, kh * kw * C:] == 0).all())


def test_coded_maps_name_their_pixels():
    """Inside one image every (y, x) pixel of the 19 x 23 map has its own 8-channel vector under either encoding, the two encodings
    differ, and the images of a batch differ."""
    for enc in (0, 1):
        x = FE.coded_map(3, 19, 23, 8, enc)
        for b in range(3):
            assert len({tuple(r.tolist()) for r in x[b]}) == 19 * 23
        assert not torch.equal(x[0], x[1])
    assert not torch.equal(FE.coded_map(1, 19, 23, 8, 0), FE.coded_map(1, 19, 23, 8, 1))


@pytest.mark.parametrize("H,W", FE.STEM_IMAGES)
def test_stem_ref_equals_unfold(H, W):
    B = 2
    img = FE.stem_image(B, H, W, H + W)
    ref = FE.im2col_stem_ref(img, 152)
    un = F.unfold(img, 7, padding=3, stride=2).permute(0, 2, 1).reshape(ref.shape[0], 147).half()
    assert torch.equal(ref[:, :147].view(torch.int16), un.view(torch.int16)) and bool((ref[:, 147:] == 0).all())
    if H * W * 3 * B >= 9:
        h = img.half().view(-1)[-9:]
        assert h[0] == 1.0 and h[1] == 1.0 + 2.0 ** -9 and torch.isinf(h[2]) and h[3] == 65504.0 and h[4] == 2.0 ** -24
        assert 0 < h[5] < 2.0 ** -14 and h[6] == 0 and torch.isinf(h[7]) and h[8] == -1.0
        assert bool(torch.isinf(ref).any())


@pytest.mark.parametrize("kind", ["negative", "inf", "ties"])
@pytest.mark.parametrize("H,W", FE.POOL_MAPS)
def test_maxpool_ref_equals_max_pool2d(H, W, kind):
    B, C = 2, 8
    x = FE.pool_map(B, H, W, C, kind, H + W)
    assert not bool(torch.isnan(x).any())
    ref = FE.maxpool_ref(x, B, H, W, C)
    mp = F.max_pool2d(x.reshape(B, H, W, C).permute(0, 3, 1, 2).float(), 3, 2, 1).permute(0, 2, 3, 1).reshape(ref.shape)
    assert torch.equal(ref.float(), mp)
    if kind == "negative":
        assert bool((ref < 0).all())
    if kind == "inf" and H >= 3:
        assert bool(torch.isinf(ref).any()) and bool((ref[0] == float("-inf")).all())


# ---- epilogue 3 ----------------------------------------------------------------------------------------------------------
def test_conv_epilogue_ref_equals_conv2d_float64():
    """relu(conv2d(x, w, bias, dilation 2, padding 2) + identity) in float64 against im2col_ref -> conv_epilogue_ref."""
    g = torch.Generator().manual_seed(1)
    B, C, H, W, N = 2, 8, 7, 9, 16
    x = torch.randn((B, C, H, W), generator=g).half()
    w = (torch.randn((N, C, 3, 3), generator=g) / 8).half()
    bias = torch.randn(N, generator=g)
    idn = torch.randn((B, N, H, W), generator=g).half()
    want = F.relu(F.conv2d(x.double(), w.double(), bias.double(), dilation=2, padding=2) + idn.double())
    tok = x.permute(0, 2, 3, 1).reshape(B, H * W, C)
    cols = FE.im2col_ref(tok, B, H, W, C, 3, 3, 1, 2, 2)
    ref, bound = FE.conv_epilogue_ref(cols, w.permute(0, 2, 3, 1).reshape(N, 9 * C), bias, idn.permute(0, 2, 3, 1).reshape(-1, N))
    want = want.permute(0, 2, 3, 1).reshape(-1, N)
    assert float((ref - want).abs().max()) <= 1e-13 * float(want.abs().max())
    assert bool((bound >= FE.HALF_FLOOR).all())


@pytest.mark.parametrize("K", FE.GEMM_K)
def test_fp32_torch_sits_inside_the_epilogue_bound(K):
    M, N = 300, 384
    a, w, bias, resid = FE.gemm_operands(M, N, K, K)
    for r in (None, resid):
        ref, bound = FE.conv_epilogue_ref(a, w, bias, r)
        v = a.float() @ w.float().t() + bias
        got = F.relu(v + r.float() if r is not None else v).half().double()
        err = (got - ref).abs()
        assert bool((err <= bound).all()), f"fp32 torch needs {_ratio(err, bound):.2f} of the bound"
    a, w, bias, resid = FE.gemm_operands(M, N, K, K + 1, integers=True)
    ref, _ = FE.conv_epilogue_ref(a, w, bias, resid)
    pre = a.double() @ w.double().t() + bias.double() + resid.double()
    assert torch.equal(ref, ref.round()) and float(pre.abs().max()) < 2048 and float(ref.max()) > 0
    assert torch.equal(ref.half().double(), ref)


# ---- psam_rotate_nearest -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,angle,expand", FE.ROTATE_CASES)
def test_rotate_replica_vs_tv_rotate_and_band_cap(H, W, angle, expand):
    """The fp32 replica names the pixel oracle/rotate.py's tv_rotate (affine grid + grid_sample, NEAREST) samples, everywhere
    outside the band; it agrees with the float64 chain outside the band; and at most 1 % of the in-image pixels lie in the band."""
    xg, yg, rt, ow, oh = FE.rotate_setup(H, W, angle, expand)
    r = FE.rotate_nearest_ref(H, W, xg.numpy(), yg.numpy(), rt.numpy(), 0, 0, oh, ow)
    src = np.arange(1, H * W + 1, dtype=np.float32).reshape(1, H, W)
    got = FE.rotate_gather(src, r)
    tv = orot.tv_rotate(torch.from_numpy(src)[None], angle, expand)[0].numpy()
    assert tv.shape == got.shape
    diff = got != tv
    assert not (diff[0] & ~r["band"]).any(), f"{int((diff[0] & ~r['band']).sum())} pixels differ from tv_rotate outside the band"
    d64 = (r["inside"] != r["inside64"]) | (r["inside"] & ((r["sx"] != r["sx64"]) | (r["sy"] != r["sy64"])))
    assert not (d64 & ~r["band"]).any()
    inside = r["inside"] | r["inside64"]
    share = int((r["band"] & inside).sum()) / max(int(inside.sum()), 1)
    print(f"rotate {H}x{W} {angle} expand={expand}: canvas {oh}x{ow}, {int(inside.sum())} in-image pixels, band share {share:.2e}, "
          f"{int(diff.sum())} differ from tv_rotate, {int(d64.sum())} from float64")
    assert share <= FE.ROTATE_BAND_CAP
    assert int(r["inside"].sum()) >= min(H, W) ** 2 // 2 + 1


def test_rotate_tie_case_is_decided_exactly():
    """The structural-tie input: no operation of the fp32 chain rounds (it equals the float64 chain bit for bit), every source
    coordinate is an exact half-integer, and round-half-to-even goes down at even and up at odd indices - floor(x + 0.5) would
    differ on half of them."""
    H, W, xg, yg, rt, ow, oh = FE.tie_case()
    r = FE.rotate_nearest_ref(H, W, xg.numpy(), yg.numpy(), rt.numpy(), 0, 0, oh, ow)
    assert r["exact"]
    assert np.array_equal(r["ix"], np.broadcast_to(np.arange(ow, dtype=np.float32) - 0.5, (oh, ow)))
    assert np.array_equal(r["iy"], np.broadcast_to((np.arange(oh, dtype=np.float32) - 0.5)[:, None], (oh, ow)))
    up = np.floor(r["ix"] + np.float32(0.5)).astype(np.int64)
    assert int((up != r["sx"]).sum()) == oh * (ow // 2) and int((up == r["sx"]).sum()) > 0
    # -0.5 rounds to -0, which is inside; 63.5 rounds to 64, which is not
    assert r["inside"][:H, :W].all() and not r["inside"][H].any() and not r["inside"][:, W].any()


@pytest.mark.parametrize("H,W,OH,OW", FE.AA_RANGE_CASES)
def test_aa_tap_ranges_hold_for_aten(H, W, OH, OW):
    """fp32 ATen reads no tap outside [xmin, xmax): with an input column (row) at +inf every output whose range does not hold it
    stays finite (the same check holds the kernel's ranges on the GPU)."""
    x = FE.aa_planes(1, H, W, H + OW)
    for axis, n_in, n_out in ((2, W, OW), (1, H, OH)):
        for pos in range(0, n_in, max(1, n_in // 12)):
            dirty = x.clone()
            dirty.select(axis, pos).fill_(float("inf"))
            if W == 1 and OW == 1:       # (ATen misreads a one-column image: see test_resize_aa_ref_vs_interpolate)
                got = F.interpolate(dirty.expand(1, H, 2).contiguous()[None], size=(OH, 2), mode="bilinear", antialias=True)[0, :, :, :1]
            else:
                got = F.interpolate(dirty[None], size=(OH, OW), mode="bilinear", antialias=True)[0]
            keep = torch.from_numpy(FE.aa_outside_range(n_in, n_out, pos))
            g = got[:, :, keep] if axis == 2 else got[:, keep, :]
            assert bool(torch.isfinite(g).all()), (axis, pos)


# ---- psam_resize_aa ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W,OH,OW", FE.AA_CASES)
def test_resize_aa_ref_vs_interpolate(H, W, OH, OW, C):
    """fp32 F.interpolate(bilinear, antialias=True) - the kernel restates its index and weight rule - lies inside the float64
    bound; the identity size returns the input; a constant image stays constant within the bound."""
    x = FE.aa_planes(C, H, W, H + OW)
    ref, bound = FE.resize_aa_ref(x.numpy(), OH, OW)
    if W == 1 and OW == 1:
        # ATen's CPU kernel misreads a [1, C, H, 1] tensor (its strides also pass for channels-last: output row 1 comes back as a
        # copy of row 0). Two identical columns resized to two columns are the same operation (the width pass is the identity).
        got = F.interpolate(x.expand(C, H, 2).contiguous()[None], size=(OH, 2), mode="bilinear", align_corners=False,
                            antialias=True)[0, :, :, :1].double().numpy()
    else:
        got = F.interpolate(x[None], size=(OH, OW), mode="bilinear", align_corners=False, antialias=True)[0].double().numpy()
    err = np.abs(got - ref)
    print(f"resize_aa {C}x{H}x{W}->{OH}x{OW}: fp32 ATen needs {_ratio(err, bound):.3f} of the bound")
    assert (err <= bound).all(), f"fp32 ATen needs {_ratio(err, bound):.2f} of the bound"
    if (H, W) == (OH, OW):
        assert np.array_equal(ref, x.double().numpy())
    c = np.full((1, H, W), 3.7, dtype=np.float32)
    ref, bound = FE.resize_aa_ref(c, OH, OW)
    assert np.abs(ref - np.float64(np.float32(3.7))).max() <= 4 * 2.0 ** -53 * 3.7
    assert np.isfinite(bound).all() and bound.min() > 0
