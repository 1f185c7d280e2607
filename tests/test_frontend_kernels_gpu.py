"""GPU parity of the second half of csrc/resample.hip - the scan hand-off (psam_volume_stats, psam_volume_slices), the ResNet front
end (psam_im2col, psam_im2col_stem, psam_maxpool3x3s2), the rotation kernels (psam_rotate_nearest, psam_resize_aa) - and of the
conv epilogue of csrc/gemm.hip (epilogue 3), one kernel at a time, against the references of oracle/frontend.py.

House rules (as in test_resample_kernels_gpu.py): every output buffer is filled with NaN before the call and is larger than what
the kernel must write, so an element left unwritten fails and so does one written past the end; gathers, nearest resampling and
the rotation indices are compared exactly; where a kernel rounds, the bound is the element-wise one the reference states, counted
from the kernel's roundings (tests/test_frontend_reference_cpu.py shows fp32 numpy / torch inside the same bounds on the same
inputs); no flat tolerances. Every call goes through protosam_amd.ops.

Worst ratios measured on an MI355X are in profiles/frontend_kernel_tests.txt.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import frontend as FE

pytestmark = pytest.mark.gpu

NAN = float("nan")
TAIL = 64          # elements (or one row) of NaN after every output


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def _out(n, dev, dtype=torch.float32):
    """(flat NaN buffer of n + TAIL elements, its first n elements)."""
    buf = _nan((n + TAIL,), dev, dtype)
    return buf, buf[:n]


def _tail_untouched(buf, n, what):
    assert bool(buf[n:].isnan().all()), f"{what}: wrote past the end of its output"


def _within(out, ref, bound, what):
    """|out - ref| <= bound element-wise (float64 on the CPU); returns the worst |out - ref| / bound."""
    out = torch.as_tensor(out).detach().double().cpu().reshape(ref.shape)
    ref, bound = torch.as_tensor(ref), torch.as_tensor(bound)
    assert bool(torch.isfinite(out).all()), f"{what}: {int((~torch.isfinite(out)).sum())} non-finite (unwritten?) elements"
    err = (out - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"RATIO {what}: worst |err| / bound = {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements outside the bound (worst {worst:.2f} of it)"
    return worst


# ---- 1. psam_volume_stats -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0, 1, 2, 3])
@pytest.mark.parametrize("n", FE.STATS_SIZES)
def test_volume_stats(dev, n, dt):
    """Case A (slope 1, intercept 0, integer voxels): sum and sum of squares against the exact integer sums, relative n 2^-53 (an
    fp64 accumulation of n terms in any order; x and x * x are exact). Case B (slope 0.37, intercept -12.5): inside the interval
    of the fused and the unfused fp32 scaling, widened by the same accumulation term (and the reference's own summation slack)."""
    from protosam_amd import ops
    v = FE.stats_volume(dt, n, 10 * n + dt)
    vd = torch.from_numpy(v).to(dev)
    got = ops.volume_stats(vd, dt).cpu().tolist()
    es, eq = FE.exact_integer_sums(v)
    mag = (float(np.abs(v.astype(np.float32).astype(np.float64)).sum()), float(eq))
    for k, (g, e) in enumerate(zip(got, (es, eq))):
        tol = n * 2.0 ** -53 * mag[k]
        print(f"RATIO volume_stats A dt={dt} n={n} {'sum' if k == 0 else 'sumsq'}: {abs(g - e) / max(tol, 1e-300):.3f}")
        assert abs(g - e) <= tol, f"volume_stats dt={dt} n={n} [{k}]: got {g!r}, exact {e}"
    r = FE.volume_stats64(v, 0.37, -12.5)
    got = ops.volume_stats(vd, dt, 0.37, -12.5).cpu().tolist()
    for k, g in enumerate(got):
        tol = (n + FE.SUM_SLACK) * 2.0 ** -53 * r["mag"][k]
        off = max(r["lo"][k] - g, g - r["hi"][k], 0.0)
        print(f"RATIO volume_stats B dt={dt} n={n} [{k}]: {off / max(tol, 1e-300):.3f} outside [fused, unfused]")
        assert off <= tol, f"volume_stats dt={dt} n={n} [{k}]: {g!r} outside [{r['lo'][k]!r}, {r['hi'][k]!r}]"


# ---- 2. psam_volume_slices ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0, 1, 2, 3])
@pytest.mark.parametrize("H,W,S", FE.SLICE_SHAPES)
def test_volume_slices(dev, H, W, S, dt):
    """Z and tile in {1, 3}. Mode 1 (labels with 0 and 255): exactly the reference, every tile copy equal to copy 0, also with an
    exact slope / intercept (2, 3). Mode 0 with
    slope / intercept / mean / 1/std all non-trivial: inside the reference's bound (12 chained fp32 roundings of the blend
    magnitude). The identity size with slope 1: bit for bit the fp32 normalisation of the input. A 1-pixel axis: constant along
    it, bit for bit."""
    from protosam_amd import ops
    worst = 0.0
    for Z in (1, 3):
        lab = FE.label_volume(dt, Z, H, W, H + W + dt)
        vol = FE.slice_volume(dt, Z, H, W, H * W + S + dt)
        labd, vold = torch.from_numpy(lab).to(dev), torch.from_numpy(vol).to(dev)
        lref = torch.from_numpy(FE.volume_slices_ref(lab, 1.0, 0.0, 0.0, 1.0, S, 1))
        val, bound = FE.volume_slices_ref(vol, S=S, mode=0, **FE.SLICE_NORM)
        for tile in (1, 3):
            what = f"volume_slices dt={dt} {Z}x{H}x{W}->{S} tile={tile}"
            n = Z * tile * S * S
            buf, o = _out(n, dev)
            ops.volume_slices(labd, dt, Z, H, W, 1.0, 0.0, 0.0, 1.0, S, tile, 1, out=o.view(Z, tile, S, S))
            _tail_untouched(buf, n, what)
            oc = o.view(Z, tile, S, S).cpu()
            for c in range(tile):
                assert torch.equal(oc[:, c], lref), f"{what} mode 1: tile copy {c} differs from the reference"
            # mode 1 scales too: slope 2, intercept 3 are exact on label values, fused or not
            buf, o = _out(n, dev)
            ops.volume_slices(labd, dt, Z, H, W, 2.0, 3.0, 0.0, 1.0, S, tile, 1, out=o.view(Z, tile, S, S))
            _tail_untouched(buf, n, what)
            assert torch.equal(o.view(Z, tile, S, S).cpu(), (2.0 * lref + 3.0)[:, None].expand(Z, tile, S, S)), f"{what} mode 1 scaled"
            buf, o = _out(n, dev)
            ops.volume_slices(vold, dt, Z, H, W, S=S, tile=tile, mode=0, out=o.view(Z, tile, S, S), **FE.SLICE_NORM)
            _tail_untouched(buf, n, what)
            oc = o.view(Z, tile, S, S).cpu()
            for c in range(1, tile):
                assert torch.equal(oc[:, c], oc[:, 0]), f"{what} mode 0: tile copy {c} differs from copy 0"
            worst = max(worst, _within(oc[:, 0], torch.from_numpy(val), torch.from_numpy(bound), what))
            # a 1-pixel axis: both clamps collapse the weight onto the one pixel, so the blend along it is exact and the
            # result is constant along it, bit for bit (a clamp that keeps its weight blends the pixel with itself, and rounds)
            if W == 1:
                assert torch.equal(oc, oc[..., :1].expand_as(oc)), f"{what}: not constant along x on a 1-pixel axis"
            if H == 1:
                assert torch.equal(oc, oc[..., :1, :].expand_as(oc)), f"{what}: not constant along y on a 1-pixel axis"
            if (H, W) == (S, S):
                buf, o = _out(n, dev)
                ops.volume_slices(vold, dt, Z, H, W, 1.0, 0.0, 41.3, 1.0 / 57.9, S, tile, 0, out=o.view(Z, tile, S, S))
                n32 = torch.from_numpy(FE.normalise32(vol, 1.0, 0.0, 41.3, 1.0 / 57.9))
                assert torch.equal(o.view(Z, tile, S, S).cpu(), n32[:, None].expand(Z, tile, S, S)), f"{what}: identity not bit-equal"


@pytest.mark.parametrize("dt", [0, 3])
def test_volume_slices_exact_arithmetic(dev, dt):
    """Integer voxels, mean 0, 1 / std 1, S = 4 H = 2 W: every weight is a multiple of 1/8 and every product and sum is exact, fused
    or not: bit-equal to the float64 reference."""
    from protosam_amd import ops
    Z, H, W, S = 2, 6, 12, 24
    vol = FE.slice_volume(0, Z, H, W, 5).astype(FE.NP_DT[dt])
    val, _ = FE.volume_slices_ref(vol, 1.0, 0.0, 0.0, 1.0, S, 0)
    buf, o = _out(Z * S * S, dev)
    ops.volume_slices(torch.from_numpy(vol).to(dev), dt, Z, H, W, 1.0, 0.0, 0.0, 1.0, S, 1, 0, out=o.view(Z, 1, S, S))
    assert torch.equal(o.view(Z, S, S).cpu().double(), torch.from_numpy(val))


# ---- 3. psam_im2col -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", FE.IM2COL_C)
@pytest.mark.parametrize("kh,kw,stride,dil,pad,H,W", FE.im2col_cases())
def test_im2col(dev, kh, kw, stride, dil, pad, H, W, C):
    """Exactly the reference for B in {1, 3}, ldo = kh kw C (+ 8, + 64; the pad columns zero) and both position encodings; the row
    after the last one keeps its NaN."""
    from protosam_amd import ops
    K = kh * kw * C
    for B in (1, 3):
        for enc in (0, 1):
            x = FE.coded_map(B, H, W, C, enc)
            ref = FE.im2col_ref(x, B, H, W, C, kh, kw, stride, dil, pad)
            xd = x.to(dev)
            for ldo in (K, K + 8, K + 64):
                rows = ref.shape[0]
                out = _nan((rows + 1, ldo), dev, torch.float16)
                _, Ho, Wo = ops.im2col(xd, B, H, W, C, kh, kw, stride, dil, pad, ldo=ldo, out=out[:rows])
                assert B * Ho * Wo == rows
                oc = out.cpu()
                what = f"im2col {kh}x{kw} s{stride} d{dil} p{pad} {B}x{H}x{W}x{C} ldo={ldo} enc={enc}"
                assert torch.equal(oc[:rows, :K].view(torch.int16), ref.view(torch.int16)), what
                assert bool((oc[:rows, K:] == 0).all()), f"{what}: K padding not zero"
                assert bool(oc[rows].isnan().all()), f"{what}: wrote past the last row"


# ---- 4. psam_im2col_stem ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("ldo", FE.STEM_LDO)
@pytest.mark.parametrize("H,W", FE.STEM_IMAGES)
def test_im2col_stem(dev, H, W, ldo, B):
    """Bit-equal to the half rounding of the gathered fp32 values (ties to even, overflow to inf, subnormals), zero beyond 147."""
    from protosam_amd import ops
    img = FE.stem_image(B, H, W, H + W)
    ref = FE.im2col_stem_ref(img, ldo)
    rows = ref.shape[0]
    out = _nan((rows + 1, ldo), dev, torch.float16)
    _, Ho, Wo = ops.im2col_stem(img.to(dev), ldo, out=out[:rows])
    assert B * Ho * Wo == rows
    oc = out.cpu()
    assert torch.equal(oc[:rows].view(torch.int16), ref.view(torch.int16)), f"im2col_stem {B}x{H}x{W} ldo={ldo}"
    assert bool(oc[rows].isnan().all())


# ---- 5. psam_maxpool3x3s2 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", FE.POOL_C)
@pytest.mark.parametrize("H,W", FE.POOL_MAPS)
def test_maxpool3x3s2(dev, H, W, C):
    """Exact on all-negative maps (the -inf start), maps with -inf / +inf entries and maps of ties."""
    from protosam_amd import ops
    B = 2
    for kind in ("negative", "inf", "ties"):
        x = FE.pool_map(B, H, W, C, kind, H + W + C)
        ref = FE.maxpool_ref(x, B, H, W, C)
        rows = ref.shape[0]
        out = _nan((rows + 1, C), dev, torch.float16)
        ops.maxpool3x3s2(x.to(dev), B, H, W, C, out=out[:rows])
        oc = out.cpu()
        assert not bool(oc[:rows].isnan().any()), f"maxpool {kind} {H}x{W}x{C}: unwritten elements"
        assert torch.equal(oc[:rows].float(), ref.float()), f"maxpool {kind} {H}x{W}x{C}"
        assert bool(oc[rows].isnan().all())


# ---- 6. epilogue 3 of psam_gemm_f16 -------------------------------------------------------------------------------------
def _gemm3(dev, a, w, bias, resid, strided):
    """ops.gemm(epilogue 3); strided: `a` lives inside a wider buffer (lda = K + 64, as inside an im2col output), the residual in
    one of N + 4 columns, the output in one of N + 8 columns with a row after it. Returns (out [M, N] on the CPU, the whole output
    buffer on the CPU)."""
    from protosam_amd import ops
    M, K = a.shape
    N = w.shape[0]
    if strided:
        ab = _nan((M, K + 64), dev, torch.float16)
        ab[:, :K] = a.to(dev)
        ad = ab[:, :K]
        rd = None
        if resid is not None:
            rb = _nan((M, N + 4), dev, torch.float16)
            rb[:, :N] = resid.to(dev)
            rd = rb[:, :N]
        ob = _nan((M + 1, N + 8), dev, torch.float16)
    else:
        ad, rd = a.to(dev), None if resid is None else resid.to(dev)
        ob = _nan((M + 1, N), dev, torch.float16)
    ops.gemm(ad, w.to(dev), bias.to(dev), out=ob[:M, :N], epilogue=ops.EPI_RELU_F16, resid=rd)
    oc = ob.cpu()
    assert bool(oc[M].isnan().all()) and bool(oc[:, N:].isnan().all()), "rows past M / columns past N were written"
    return oc[:M, :N], oc


@pytest.mark.parametrize("K", FE.GEMM_K)
@pytest.mark.parametrize("N", FE.GEMM_N)
@pytest.mark.parametrize("M", FE.GEMM_M)
def test_conv_epilogue(dev, M, N, K):
    """relu(a @ w^T + bias [+ resid]) within conv_epilogue_ref's bound, contiguous and strided (lda > K, ldr > N, ldo > N), with and
    without the half residual; rows past M and columns past N keep their NaN. Then small-integer operands: every partial sum is
    exact, so the result equals the reference in value."""
    a, w, bias, resid = FE.gemm_operands(M, N, K, M + N + K)
    for r in (None, resid):
        ref, bound = FE.conv_epilogue_ref(a, w, bias, r)
        for strided in (False, True):
            out, _ = _gemm3(dev, a, w, bias, r, strided)
            _within(out, ref, bound, f"epilogue3 {M}x{N}x{K} resid={r is not None} strided={strided}")
    a, w, bias, resid = FE.gemm_operands(M, N, K, M + N + K + 1, integers=True)
    for r in (None, resid):
        ref, _ = FE.conv_epilogue_ref(a, w, bias, r)
        assert float(ref.max()) < 2048 and torch.equal(ref, ref.round())          # exact in half
        out, _ = _gemm3(dev, a, w, bias, r, True)
        assert torch.equal(out.double(), ref), f"epilogue3 integers {M}x{N}x{K} resid={r is not None}"


def test_conv_epilogue_ignores_the_forced_tile(dev):
    """Whatever psam_gemm_set_tile forces, epilogue 3 runs on the 128-tile kernel: bit-identical results."""
    from protosam_amd import ops
    M, N, K = 300, 384, 192
    a, w, bias, resid = FE.gemm_operands(M, N, K, 7)
    base, _ = _gemm3(dev, a, w, bias, resid, True)
    try:
        for t in (11, 12, 13, 15, 16):
            ops.gemm_set_tile(t)
            out, _ = _gemm3(dev, a, w, bias, resid, True)
            assert torch.equal(out.view(torch.int16), base.view(torch.int16)), f"tile {t}"
    finally:
        ops.gemm_set_tile(0)


@pytest.mark.parametrize("stride,dil", [(2, 1), (1, 2)])
def test_bottleneck_end_to_end(dev, stride, dil):
    """One ResNet bottleneck with a downsample branch, as protosam_amd/backbone.py runs it (1x1 conv + ReLU, im2col 3x3 -> GEMM +
    ReLU, 1x1 downsample (epilogue 0) on the strided map, 1x1 conv + identity + ReLU), B = 2, 9 x 11, 128 -> 128 -> 512, against
    F.conv2d in float64 on the same half weights. The bound is conv_epilogue_ref's, propagated: each stage's bound (its half
    rounding included) is the input error of the next, through |w|."""
    from protosam_amd import ops
    g = torch.Generator().manual_seed(stride * 10 + dil)
    B, H, W, Cin, Wd, Cout = 2, 9, 11, 128, 128, 512
    x = torch.randn((B, Cin, H, W), generator=g).relu().half()
    w1 = (torch.randn((Wd, Cin), generator=g) / Cin ** 0.5).half()
    w2 = (torch.randn((Wd, Wd, 3, 3), generator=g) / (9 * Wd) ** 0.5).half()
    w3 = (torch.randn((Cout, Wd), generator=g) / Wd ** 0.5).half()
    wd = (torch.randn((Cout, Cin), generator=g) / Cin ** 0.5).half()
    b1, b2, b3, bd = (torch.randn(n, generator=g) * 0.1 for n in (Wd, Wd, Cout, Cout))
    tok = x.permute(0, 2, 3, 1).reshape(B * H * W, Cin).contiguous()
    w2m = w2.permute(0, 2, 3, 1).reshape(Wd, 9 * Wd).contiguous()
    # the product path
    xd = tok.to(dev)
    y = ops.gemm(xd, w1.to(dev), b1.to(dev), epilogue=ops.EPI_RELU_F16)
    cols, Ho, Wo = ops.im2col(y, B, H, W, Wd, 3, 3, stride, dil, dil)
    y = ops.gemm(cols, w2m.to(dev), b2.to(dev), epilogue=ops.EPI_RELU_F16)
    idn = xd
    if stride != 1:
        idn, _, _ = ops.im2col(xd, B, H, W, Cin, 1, 1, stride, 1, 0)
    idn = ops.gemm(idn, wd.to(dev), bd.to(dev), epilogue=ops.EPI_F16)
    out = ops.gemm(y, w3.to(dev), b3.to(dev), epilogue=ops.EPI_RELU_F16, resid=idn)
    # float64, no intermediate rounding
    x64 = x.double()
    r = F.relu(F.conv2d(x64, w1.double()[:, :, None, None], b1.double()))
    r = F.relu(F.conv2d(r, w2.double(), b2.double(), stride=stride, dilation=dil, padding=dil))
    want = F.relu(F.conv2d(r, w3.double()[:, :, None, None], b3.double())
                  + F.conv2d(x64, wd.double()[:, :, None, None], bd.double(), stride=stride))
    assert want.shape[-2:] == (Ho, Wo)
    want = want.permute(0, 2, 3, 1).reshape(B * Ho * Wo, Cout)
    # the same chain through the references, carrying the bound
    v1, e1 = FE.conv_epilogue_ref(tok, w1, b1)
    c1 = FE.im2col_ref(v1, B, H, W, Wd, 3, 3, stride, dil, dil)
    ce1 = FE.im2col_ref(e1, B, H, W, Wd, 3, 3, stride, dil, dil)
    v2, e2 = FE.conv_epilogue_ref(c1, w2m, b2, in_err=ce1)
    xs = FE.im2col_ref(tok, B, H, W, Cin, 1, 1, stride, 1, 0)
    vi, ei = FE.conv_epilogue_ref(xs, wd, bd, relu=False)
    v3, e3 = FE.conv_epilogue_ref(v2, w3, b3, resid=vi, in_err=e2)
    assert float((v3 - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # the residual the kernel adds is within ei of vi: one more input error of the last stage (its fp32 add and half rounding
    # are already counted on |v|; ei moves |v| by at most ei)
    bound = e3 + ei * (1.0 + FE.U + FE.HALF_U)
    _within(out, want, bound, f"bottleneck stride={stride} dil={dil}")


# ---- 7. psam_rotate_nearest ---------------------------------------------------------------------------------------------
def _arange_planes(C, H, W):
    return torch.arange(1, C * H * W + 1, dtype=torch.float32).view(1, C, H, W)       # 0 names "outside"


@pytest.mark.parametrize("H,W,angle,expand", FE.ROTATE_CASES)
def test_rotate_nearest_equals_the_fp32_replica(dev, H, W, angle, expand):
    """Through protosam_amd.rotate._rotate (with and without reverse_tensor's centre crop) and straight through
    ops.rotate_nearest: every output pixel names the source pixel the fp32 replica names, or 0 outside. No allowance."""
    from protosam_amd import ops
    from protosam_amd.rotate import _rotate
    C = 2
    src = _arange_planes(C, H, W)
    srcd = src.to(dev)
    xg, yg, rt, ow, oh = FE.rotate_setup(H, W, angle, expand)
    crops = [(0, 0)] + ([(1, 2)] if oh > 2 and ow > 4 else [])
    for cy, cx in crops:
        outH, outW = oh - 2 * cy, ow - 2 * cx
        ref = FE.rotate_nearest_ref(H, W, xg.numpy(), yg.numpy(), rt.numpy(), cy, cx, outH, outW)
        want = torch.from_numpy(FE.rotate_gather(src[0].numpy(), ref))
        what = f"rotate {H}x{W} {angle} expand={expand} crop=({cy},{cx})"
        got = _rotate(srcd, angle, expand, crop=(cy, cx)).cpu()
        assert got.shape == (1, C, outH, outW)
        assert torch.equal(got[0], want), f"{what} via _rotate: {int((got[0] != want).sum())} pixels differ from the fp32 replica"
        n = C * outH * outW
        buf, o = _out(n, dev)
        ops.rotate_nearest(srcd, xg.to(dev), yg.to(dev), rt, cy, cx, outH, outW, out=o.view(1, C, outH, outW))
        _tail_untouched(buf, n, what)
        assert torch.equal(o.view(C, outH, outW).cpu(), want), f"{what} via ops.rotate_nearest"
        assert int(ref["inside"].sum()) > 0


def test_rotate_nearest_ties_round_to_even(dev):
    """The structural-tie input (every source coordinate an exact half-integer): round half to even, down at even and up at odd
    indices, exactly as the replica."""
    from protosam_amd import ops
    H, W, xg, yg, rt, ow, oh = FE.tie_case()
    src = _arange_planes(1, H, W)
    ref = FE.rotate_nearest_ref(H, W, xg.numpy(), yg.numpy(), rt.numpy(), 0, 0, oh, ow)
    want = torch.from_numpy(FE.rotate_gather(src[0].numpy(), ref))
    buf, o = _out(oh * ow, dev)
    ops.rotate_nearest(src.to(dev), xg.to(dev), yg.to(dev), rt, 0, 0, oh, ow, out=o.view(1, 1, oh, ow))
    _tail_untouched(buf, oh * ow, "rotate ties")
    assert torch.equal(o.view(1, oh, ow).cpu(), want)


@pytest.mark.parametrize("outW", [255, 256, 257])
def test_rotate_nearest_block_edge(dev, outW):
    """Output widths around the 256-wide block: a 17 x 23 source sampled on a (outW + 6)-wide canvas with a crop of 3 columns."""
    from protosam_amd import ops
    from oracle import rotate as orot
    H, W, C, cy, cx, outH = 17, 23, 2, 1, 3, 5
    _, _, rt, _, _ = FE.rotate_setup(H, W, 33.0, False)
    rt = (rt * 0.1).contiguous()                   # the wide canvas mapped onto the source: most columns sample inside
    xg, yg = orot.base_grid_axes(outW + 2 * cx, outH + 2 * cy)
    src = _arange_planes(C, H, W)
    ref = FE.rotate_nearest_ref(H, W, xg.numpy(), yg.numpy(), rt.numpy(), cy, cx, outH, outW)
    assert int(ref["inside"][:, -3:].sum()) > 0 and int(ref["inside"].sum()) > outW
    want = torch.from_numpy(FE.rotate_gather(src[0].numpy(), ref))
    n = C * outH * outW
    buf, o = _out(n, dev)
    ops.rotate_nearest(src.to(dev), xg.to(dev), yg.to(dev), rt, cy, cx, outH, outW, out=o.view(1, C, outH, outW))
    _tail_untouched(buf, n, f"rotate outW={outW}")
    assert torch.equal(o.view(C, outH, outW).cpu(), want)


# ---- 8. psam_resize_aa --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W,OH,OW", FE.AA_CASES)
def test_resize_aa(dev, H, W, OH, OW, C):
    """Inside the float64 bound of resize_aa_ref (tap ranges reproduced exactly; weight, normalisation and multiply-add roundings
    counted); the identity size bit-equal to the input; a constant image constant within the same bound."""
    from protosam_amd import ops
    x = FE.aa_planes(C, H, W, H + OW)
    ref, bound = FE.resize_aa_ref(x.numpy(), OH, OW)
    n = C * OH * OW
    buf, o = _out(n, dev)
    ops.resize_aa(x[None].to(dev), OH, OW, out=o.view(1, C, OH, OW))
    _tail_untouched(buf, n, "resize_aa")
    _within(o.view(C, OH, OW), torch.from_numpy(ref), torch.from_numpy(bound), f"resize_aa {C}x{H}x{W}->{OH}x{OW}")
    if (H, W) == (OH, OW):
        assert torch.equal(o.view(C, OH, OW).cpu(), x), "identity size not bit-equal"
    c = torch.full((1, 1, H, W), 3.7)
    ref, bound = FE.resize_aa_ref(c[0].numpy(), OH, OW)
    buf, o = _out(OH * OW, dev)
    ops.resize_aa(c.to(dev), OH, OW, out=o.view(1, 1, OH, OW))
    _within(o.view(1, OH, OW), torch.from_numpy(ref), torch.from_numpy(bound), f"resize_aa constant {H}x{W}->{OH}x{OW}")


@pytest.mark.parametrize("H,W,OH,OW", FE.AA_RANGE_CASES)
def test_resize_aa_tap_ranges(dev, H, W, OH, OW):
    """The taps of an output are [xmin, xmax) and nothing else: with one input column (then one input row) set to +inf, every output
    whose range does not hold it is finite and inside the bound of the same image with that column zeroed. A range widened by one
    tap would only add a zero weight - and 0 x inf is NaN. The outputs whose range holds the column are not compared (their last
    tap may itself weigh zero)."""
    from protosam_amd import ops
    x = FE.aa_planes(1, H, W, H + OW)
    for axis, n_in, n_out in ((2, W, OW), (1, H, OH)):
        for pos in range(0, n_in, max(1, n_in // 12)):
            clean, dirty = x.clone(), x.clone()
            clean.select(axis, pos).zero_()
            dirty.select(axis, pos).fill_(float("inf"))
            ref, bound = FE.resize_aa_ref(clean.numpy(), OH, OW)
            keep = torch.from_numpy(FE.aa_outside_range(n_in, n_out, pos))
            buf, o = _out(OH * OW, dev)
            ops.resize_aa(dirty[None].to(dev), OH, OW, out=o.view(1, 1, OH, OW))
            got = o.view(1, OH, OW).cpu().double()
            sel = (lambda t: t[:, :, keep]) if axis == 2 else (lambda t: t[:, keep, :])
            g, r, b = sel(got), sel(torch.from_numpy(ref)), sel(torch.from_numpy(bound))
            what = f"resize_aa {H}x{W}->{OH}x{OW} inf at {'column' if axis == 2 else 'row'} {pos}"
            assert bool(torch.isfinite(g).all()), f"{what}: {int((~torch.isfinite(g)).sum())} outputs outside its range are not finite"
            assert bool(((g - r).abs() <= b).all()), what


# ---- 9. arguments -------------------------------------------------------------------------------------------------------
def test_rejections_return_status_1_before_any_launch(dev):
    """Every rejection of the header returns status 1 and leaves the NaN-filled outputs untouched; where ops sizes a default output
    from the same formulas it raises ValueError before the allocation."""
    from protosam_amd import ops
    H16, f32, f16 = torch.float16, torch.float32, torch.float16
    ones = lambda *s, dt=f32: torch.ones(s, dtype=dt, device=dev)  # noqa: E731
    cases = []

    def case(name, fn, *outs):
        cases.append((name, fn, outs))

    case("volume_stats n = 0", lambda: ops.volume_stats(ones(0), 1))
    o = _nan((1, 1, 4, 4), dev)
    vol = ones(1, 4, 4)
    for name, a in (("Z = 0", (0, 4, 4, 4, 1, 0, 1)), ("H = 0", (1, 0, 4, 4, 1, 0, 1)), ("W = 0", (1, 4, 0, 4, 1, 0, 1)),
                    ("S = 0", (1, 4, 4, 0, 1, 0, 1)), ("S = -1", (1, 4, 4, -1, 1, 0, 1)), ("tile = 0", (1, 4, 4, 4, 0, 0, 1)),
                    ("mode = 2", (1, 4, 4, 4, 1, 2, 1)), ("vol_dtype = 4", (1, 4, 4, 4, 1, 0, 4))):
        Z, H, W, S, tile, mode, dt = a
        case(f"volume_slices {name}", lambda Z=Z, H=H, W=W, S=S, tile=tile, mode=mode, dt=dt, o=o:
             ops.volume_slices(vol, dt, Z, H, W, 1.0, 0.0, 0.0, 1.0, S, tile, mode, out=o), o)
    x = ones(2, 6, 8, dt=f16)                      # B = 2, 2 x 3, C = 8
    o = _nan((64, 144), dev, H16)
    #                      B  H  W  C  kh kw s  d  p  ldo
    for name, a in (("C % 8", (2, 2, 3, 4, 3, 3, 1, 1, 1, 72)), ("ldo % 8", (2, 2, 3, 8, 3, 3, 1, 1, 1, 76)),
                    ("ldo < kh kw C", (2, 2, 3, 8, 3, 3, 1, 1, 1, 64)), ("stride = 0", (2, 2, 3, 8, 3, 3, 0, 1, 1, 72)),
                    ("dil = 0", (2, 2, 3, 8, 3, 3, 1, 0, 1, 72)), ("dil = -1", (2, 2, 3, 8, 3, 3, 1, -1, 1, 72)),
                    ("kh = 0", (2, 2, 3, 8, 0, 3, 1, 1, 1, 72)), ("kw = 0", (2, 2, 3, 8, 3, 0, 1, 1, 1, 72)),
                    ("kh = -1", (2, 2, 3, 8, -1, 3, 1, 1, 1, 72)), ("H = 0", (2, 0, 3, 8, 3, 3, 1, 1, 1, 72)),
                    ("W = 0", (2, 2, 0, 8, 3, 3, 1, 1, 1, 72)), ("B = 0", (0, 2, 3, 8, 3, 3, 1, 1, 1, 72)),
                    ("C = 0", (2, 2, 3, 0, 3, 3, 1, 1, 1, 72)), ("pad = -1", (1, 4, 3, 8, 1, 1, 1, 1, -1, 8))):
        case(f"im2col {name}", lambda a=a, o=o: ops.im2col(x, *a[:9], ldo=a[9], out=o), o)
    for kh, kw, stride, dil, pad, H, W in FE.im2col_cases(valid=False):      # the map is smaller than the dilated kernel: Ho <= 0
        case(f"im2col {kh}x{kw} d{dil} p{pad} on {H}x{W}", lambda kh=kh, kw=kw, stride=stride, dil=dil, pad=pad, H=H, W=W, o=o:
             ops.im2col(x, 1, H, W, 8, kh, kw, stride, dil, pad, ldo=kh * kw * 8, out=o), o)
    o = _nan((16, 192), dev, H16)
    case("im2col_stem ldo = 144", lambda o=o: ops.im2col_stem(ones(1, 3, 4, 4), 144, out=o), o)
    case("im2col_stem ldo % 8", lambda o=o: ops.im2col_stem(ones(1, 3, 4, 4), 148, out=o), o)
    case("im2col_stem H = 0", lambda o=o: ops.im2col_stem(ones(1, 3, 0, 4), 152, out=o), o)
    case("im2col_stem W = 0", lambda o=o: ops.im2col_stem(ones(1, 3, 4, 0), 152, out=o), o)
    case("im2col_stem B = 0", lambda o=o: ops.im2col_stem(ones(0, 3, 4, 4), 152, out=o), o)
    o = _nan((16, 8), dev, H16)
    for name, a in (("H = 0", (2, 0, 3, 8)), ("W = 0", (2, 2, 0, 8)), ("C = 0", (2, 2, 3, 0)), ("B = 0", (0, 2, 3, 8)),
                    ("H = -1", (2, -1, 3, 8))):
        case(f"maxpool3x3s2 {name}", lambda a=a, o=o: ops.maxpool3x3s2(x, *a, out=o), o)
    ga, gw, gb, gr = (t.to(dev) for t in FE.gemm_operands(8, 128, 64, 1))
    o = _nan((8, 128), dev, H16)
    case("gemm epilogue 3 with resid_mod", lambda ga=ga, gw=gw, gb=gb, gr=gr, o=o:
         ops.gemm(ga, gw, gb, out=o, epilogue=ops.EPI_RELU_F16, resid=gr, resid_mod=4), o)
    for N in FE.GEMM_N_REJECTED:                   # N % 128 != 0 is outside the GEMM's contract
        a2, w2, b2, _ = (t.to(dev) for t in FE.gemm_operands(8, N, 64, 2))
        o2 = _nan((8, N), dev, H16)
        case(f"gemm epilogue 3 N = {N}", lambda a2=a2, w2=w2, b2=b2, o2=o2: ops.gemm(a2, w2, b2, out=o2, epilogue=ops.EPI_RELU_F16), o2)
    img = ones(1, 1, 4, 4)
    xg, yg, rt = ones(4), ones(4), torch.zeros((3, 2))
    o = _nan((1, 1, 4, 4), dev)
    for name, a in (("xg NULL", (None, yg, 0, 0, 4, 4)), ("yg NULL", (xg, None, 0, 0, 4, 4)), ("outH = 0", (xg, yg, 0, 0, 0, 4)),
                    ("outW = 0", (xg, yg, 0, 0, 4, 0)), ("crop_y < 0", (xg, yg, -1, 0, 4, 4)), ("crop_x < 0", (xg, yg, 0, -1, 4, 4))):
        case(f"rotate_nearest {name}", lambda a=a, o=o: ops.rotate_nearest(img, a[0], a[1], rt, *a[2:], out=o), o)
    case("rotate_nearest H = 0", lambda o=o: ops.rotate_nearest(ones(1, 1, 0, 4), xg, yg, rt, 0, 0, 4, 4, out=o), o)
    case("resize_aa OH = 0", lambda o=o: ops.resize_aa(img, 0, 4, out=o), o)
    case("resize_aa OW = 0", lambda o=o: ops.resize_aa(img, 4, 0, out=o), o)
    case("resize_aa W = 0", lambda o=o: ops.resize_aa(ones(1, 1, 4, 0), 4, 4, out=o), o)
    for name, fn, outs in cases:
        with pytest.raises(RuntimeError, match="status 1"):
            fn()
        torch.cuda.synchronize()
        for t in outs:
            assert bool(t.isnan().all()), f"{name}: output written"
    # default outputs: nothing is allocated from sizes the library would reject
    for fn in (lambda: ops.im2col(x, 1, 2, 3, 8, 3, 3, 1, 4, 0), lambda: ops.im2col(x, 2, 0, 3, 8, 3, 3, 1, 1, 1),
               lambda: ops.im2col(x, 2, 2, 3, 8, 0, 3, 1, 1, 1), lambda: ops.im2col(x, 2, 2, 3, 8, 3, 3, 1, 1, -1),
               lambda: ops.maxpool3x3s2(x, 2, 0, 3, 8), lambda: ops.maxpool3x3s2(x, 2, 2, -1, 8)):
        with pytest.raises(ValueError, match="no output"):
            fn()
    print(f"{len(cases)} rejections, each status 1 with its outputs untouched")
