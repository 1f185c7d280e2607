"""References for the second half of csrc/resample.hip - the scan hand-off (psam_volume_stats, psam_volume_slices), the ResNet
front end (psam_im2col, psam_im2col_stem, psam_maxpool3x3s2), the rotation kernels (psam_rotate_nearest, psam_resize_aa) - and for
the conv epilogue of csrc/gemm.hip (EPI_RELU_F16, epilogue 3). Plain restatements on the CPU in numpy / torch, written from the
header comments and the kernel comments:

  * where a kernel only moves values (the gathers, nearest resampling) the reference is exact;
  * where a kernel takes a decision in fp32 (tap indices, rounded source pixels) the reference repeats that fp32 arithmetic
    operation by operation in numpy float32, so the decision is reproduced, not bounded;
  * where a kernel rounds, the reference is float64 and comes with an element-wise bound counted from the kernel's roundings in
    units of u = 2^-24 (the unit round-off of fp32), never a flat tolerance.

tests/test_frontend_reference_cpu.py pins every reference to stock code and shows that the bounds hold for fp32 torch / numpy on
the inputs of the GPU test; tests/test_frontend_kernels_gpu.py holds the kernels to them. The input builders of both files are at
the end.
"""
import numpy as np
import torch

U = 2.0 ** -24                    # unit round-off of fp32
HALF_U = 2.0 ** -11               # unit round-off of half
HALF_FLOOR = 2.0 ** -25           # half the spacing of the subnormal halves
SUM_SLACK = 64                    # see volume_stats64
NP_DT = {0: np.int16, 1: np.float32, 2: np.uint8, 3: np.int32}        # the vol_dtype codes of psam_volume_*
TORCH_DT = {0: torch.int16, 1: torch.float32, 2: torch.uint8, 3: torch.int32}


def gamma(n):
    """n u / (1 - n u): the relative error of n chained fp32 roundings (Higham, Accuracy and Stability, lemma 3.1)."""
    return n * U / (1.0 - n * U)


# ---- psam_volume_stats ---------------------------------------------------------------------------------------------------
def _scaled_candidates(vol, slope, inter):
    """x = fl(voxel * slope + inter) both ways a compiler may emit it: (unfused, fused), float32 arrays. The voxel is converted to
    fp32 first (round to nearest even: part of the contract, an int32 above 2^24 loses its low bits here). The fused value rounds
    the exact product-sum once; the product of two fp32 numbers is exact in float64."""
    v = np.asarray(vol).astype(np.float32).ravel()
    s, i = np.float32(slope), np.float32(inter)
    unfused = (v * s + i).astype(np.float32)
    fused = (v.astype(np.float64) * np.float64(s) + np.float64(i)).astype(np.float32)
    return unfused, fused


def volume_stats64(vol, slope=1.0, inter=0.0):
    """-> dict(unfused=(sum, sumsq), fused=(sum, sumsq), lo=(.., ..), hi=(.., ..), mag=(sum |x|, sum x^2), n).
    The sums are numpy's float64 pairwise sums (blocks of 128 summed 8 abreast, then a binary tree: fewer than 64 chained
    roundings at any size used here, so within SUM_SLACK x 2^-53 x mag of the exact sum); [lo, hi] is the interval the two
    candidates span. An fp64 accumulation of n terms in any order is within (n - 1) 2^-53 x mag of the exact sum (x * x is exact
    in fp64 for an fp32 x): a kernel is held to [lo, hi] widened by (n + SUM_SLACK) 2^-53 x mag."""
    out = {}
    for name, x in zip(("unfused", "fused"), _scaled_candidates(vol, slope, inter)):
        x = x.astype(np.float64)
        out[name] = (float(x.sum()), float((x * x).sum()))
        out["mag_" + name] = (float(np.abs(x).sum()), out[name][1])
    out["lo"] = tuple(min(out["unfused"][k], out["fused"][k]) for k in range(2))
    out["hi"] = tuple(max(out["unfused"][k], out["fused"][k]) for k in range(2))
    out["mag"] = tuple(max(out["mag_unfused"][k], out["mag_fused"][k]) for k in range(2))
    out["n"] = int(np.asarray(vol).size)
    return out


def exact_integer_sums(vol):
    """(sum, sum of squares) of the fp32-converted voxels of an integer-valued volume as Python ints (exact at any size)."""
    x = np.asarray(vol).astype(np.float32).ravel().astype(np.int64)
    assert np.array_equal(x.astype(np.float32), np.asarray(vol).astype(np.float32).ravel()), "voxels are not integers"
    sq = x * x                                   # |x| <= 2^31: fits int64
    lo, hi = sq & ((1 << 31) - 1), sq >> 31      # n < 2^32 terms below 2^31 each: the partial sums fit int64
    return int(x.sum(dtype=np.int64)), (int(hi.sum(dtype=np.int64)) << 31) + int(lo.sum(dtype=np.int64))


# ---- psam_volume_slices --------------------------------------------------------------------------------------------------
def linear_taps(n_in, S):
    """The kernel's own rule for one axis: the double coordinate (d + 0.5) * (n_in / S) - 0.5 cast to fp32, floorf, the fp32
    remainder as the weight of the upper tap, then the two clamps that collapse the weight onto the edge pixel.
    -> (i0, i1, w) with w float32: exactly what the kernel decides."""
    f = ((np.arange(S, dtype=np.float64) + 0.5) * (np.float64(n_in) / np.float64(S)) - 0.5).astype(np.float32)
    i0 = np.floor(f).astype(np.int64)
    w = (f - i0.astype(np.float32)).astype(np.float32)
    i1 = i0 + 1
    lo, hi = i0 < 0, i0 >= n_in - 1
    i0[lo], i1[lo], w[lo] = 0, 0, 0
    i0[hi], i1[hi], w[hi] = n_in - 1, n_in - 1, 0
    return i0, i1, w


def nearest_taps(n_in, S):
    """min(floor(d * (n_in / S)), n_in - 1) in float64: exact."""
    i = np.floor(np.arange(S, dtype=np.float64) * (np.float64(n_in) / np.float64(S))).astype(np.int64)
    return np.minimum(i, n_in - 1)


def normalise32(vol, slope, inter, mean, inv_std):
    """((voxel * slope + inter) - mean) * inv_std in numpy float32, unfused: bit-exact whenever voxel * slope + inter is exact
    (slope 1, intercept 0), because the subtraction and the product that follow cannot be contracted."""
    v = np.asarray(vol).astype(np.float32)
    x = v * np.float32(slope) + np.float32(inter)
    return ((x - np.float32(mean)) * np.float32(inv_std)).astype(np.float32)


def volume_slices_ref(vol, slope, inter, mean, inv_std, S, mode):
    """vol [Z, H, W] (any of the four dtypes) -> mode 1: fl(voxel * slope + inter) gathered at `nearest_taps`, float32 [Z, S, S]
    (exact for slope 1 / intercept 0); mode 0: (value, bound), float64 [Z, S, S].

    Mode 0: the taps and weights are the kernel's (`linear_taps`: decisions, reproduced exactly); the value is the float64 blend
    of the float64 normalisation of the fp32 voxels. The bound counts the kernel's roundings: 4 in the normalisation (product, sum,
    difference, product - one fewer when the compiler fuses the first two), 4 per blend (1 - f, two products, one sum - fewer when
    fused), a horizontal blend feeding the vertical one: 12 chained roundings at most, gamma(12) x magnitude, the magnitude
    being the same blend (the `blend` of oracle/resample.py) of (|voxel * slope| + |inter| + |mean|) |inv_std|. The coordinate term
    (`weights` there) is zero here: the weights are reproduced, not approximated."""
    v = np.asarray(vol).astype(np.float32)
    Z, H, W = v.shape
    if mode == 1:
        x = (v * np.float32(slope) + np.float32(inter)).astype(np.float32)
        return x[:, nearest_taps(H, S)][:, :, nearest_taps(W, S)]
    s, i, m, r = (np.float64(np.float32(t)) for t in (slope, inter, mean, inv_std))
    v = v.astype(np.float64)
    n = ((v * s + i) - m) * r
    mag = (np.abs(v * s) + abs(i) + abs(m)) * abs(r)
    x0, x1, wx = linear_taps(W, S)
    y0, y1, wy = linear_taps(H, S)
    wx1, wy1 = wx.astype(np.float64), wy.astype(np.float64)[:, None]
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1              # exact; the kernel's fl(1 - f) is one of the counted roundings

    def blend(a):
        rows = a[:, :, x0] * wx0 + a[:, :, x1] * wx1
        return rows[:, y0] * wy0 + rows[:, y1] * wy1

    return blend(n), gamma(12) * blend(mag)


# ---- the gathers ---------------------------------------------------------------------------------------------------------
def conv_out(n, k, stride, dil, pad):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def im2col_ref(x, B, H, W, C, kh, kw, stride, dil, pad, ldo=None):
    """token-major half map [B, H*W, C] -> [B*Ho*Wo, ldo], column (ky*kw + kx)*C + c = x[b, y*stride - pad + ky*dil,
    x*stride - pad + kx*dil, c], zero outside the map and in columns kh*kw*C .. ldo - 1. Explicit loops over the taps."""
    x = torch.as_tensor(x).reshape(B, H, W, C)
    Ho, Wo = conv_out(H, kh, stride, dil, pad), conv_out(W, kw, stride, dil, pad)
    assert Ho > 0 and Wo > 0
    ldo = kh * kw * C if ldo is None else ldo
    out = torch.zeros((B, Ho, Wo, ldo), dtype=x.dtype)
    for ky in range(kh):
        for kx in range(kw):
            for y in range(Ho):
                yy = y * stride - pad + ky * dil
                if not 0 <= yy < H:
                    continue
                for xo in range(Wo):
                    xx = xo * stride - pad + kx * dil
                    if 0 <= xx < W:
                        out[:, y, xo, (ky * kw + kx) * C:(ky * kw + kx + 1) * C] = x[:, yy, xx]
    return out.reshape(B * Ho * Wo, ldo)


def im2col_stem_ref(img, ldo):
    """fp32 [B, 3, H, W] -> half [B*Ho*Wo, ldo] of the 7x7 / stride 2 / pad 3 conv, column (c*7 + ky)*7 + kx, zero beyond 147;
    each value rounded to half (round to nearest even; beyond the half range: inf)."""
    img = torch.as_tensor(img).float()
    B, _, H, W = img.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pad = torch.zeros((B, 3, H + 6, W + 6))
    pad[:, :, 3:H + 3, 3:W + 3] = img
    out = torch.zeros((B, Ho, Wo, ldo))
    for c in range(3):
        for ky in range(7):
            for kx in range(7):
                out[..., (c * 7 + ky) * 7 + kx] = pad[:, c, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2]
    return out.reshape(B * Ho * Wo, ldo).half()


def maxpool_ref(x, B, H, W, C):
    """MaxPool2d(3, 2, 1) on a token-major half map [B, H*W, C] -> [B*Ho*Wo, C]: the maximum over the taps inside the map (a window
    always holds its centre row / column, so -inf never survives unless the map holds it). NaN inputs are outside the contract:
    the kernel's fmaxf drops them where F.max_pool2d propagates them; the input is a post-ReLU half map."""
    x = torch.as_tensor(x).reshape(B, H, W, C)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.full((B, Ho, Wo, C), float("-inf"), dtype=torch.float32)
    for y in range(Ho):
        for xo in range(Wo):
            for ky in range(3):
                for kx in range(3):
                    yy, xx = 2 * y - 1 + ky, 2 * xo - 1 + kx
                    if 0 <= yy < H and 0 <= xx < W:
                        out[:, y, xo] = torch.maximum(out[:, y, xo], x[:, yy, xx].float())
    return out.reshape(B * Ho * Wo, C).to(x.dtype)


# ---- epilogue 3 of psam_gemm_f16 -----------------------------------------------------------------------------------------
def conv_epilogue_ref(a, w, bias=None, resid=None, in_err=None, relu=True):
    """relu(a @ w^T + bias + resid) in float64 from the half operands -> (value, bound), [M, N].

    Bound, element-wise: products of two halves are exact in fp32 (22 significant bits), so the dot product costs the K - 1 sums
    only, in whatever order the MFMAs take them: gamma(K) sum_k |a_k w_k|. Each of the two fp32 adds (bias, residual) adds
    u x |its own result| on top of what it inherits; the half rounding of the result adds 2^-11 |v| + 2^-25 (v within the
    inherited error of the exact value). ReLU is 1-Lipschitz and commutes with the (monotone) half rounding, so the bound on the
    pre-activation carries over. `in_err` (same shape as `a`, optional) is an error already present in `a`: it enters as
    in_err @ |w|^T. relu = False: epilogue 0 (the downsample conv), the same bound."""
    a64, w64 = torch.as_tensor(a).double(), torch.as_tensor(w).double()
    K = a64.shape[1]
    acc = a64 @ w64.t()
    if in_err is None:
        e = gamma(K) * (a64.abs() @ w64.abs().t())
    else:       # the kernel multiplies the operand it was given, within in_err of `a`
        ie = torch.as_tensor(in_err).double()
        e = ie @ w64.abs().t() + gamma(K) * ((a64.abs() + ie) @ w64.abs().t())
    if not relu and bias is not None:
        # epilogue 0 may run on a kernel that starts its accumulators from the bias (the half-tile assembly kernels): the bias
        # then takes part in every sum of the dot product
        e = e + gamma(K) * torch.as_tensor(bias).double().abs()
    v = acc
    if bias is not None:
        v = v + torch.as_tensor(bias).double()
        e = e + U * (v.abs() + e)
    if resid is not None:
        v = v + torch.as_tensor(resid).double()
        e = e + U * (v.abs() + e)
    e = e + HALF_U * (v.abs() + e) + HALF_FLOOR
    return (v.clamp_min(0.0) if relu else v), e


# ---- psam_rotate_nearest -------------------------------------------------------------------------------------------------
def rotate_nearest_ref(H, W, xg, yg, rt, crop_y, crop_x, outH, outW):
    """The kernel's index arithmetic, three ways, for a source of H x W and an output of outH x outW:

      fp32 replica: one numpy float32 operation per _rn intrinsic, in the kernel's order -
        g  = (b_x r0k + b_y r1k) + r2k           (b = the base-grid values xg[x + crop_x], yg[y + crop_y]; rt row-major [3, 2])
        i  = (((g + 1) n) + -1) / 2              (grid_sample's un-normalisation, align_corners = False)
        then np.rint (round half to even, as nearbyintf) and the inside test 0 <= f <= n - 1;
      float64: the same chain in float64 from the same fp32 inputs;
      band: |i64 - nearest half-integer| <= the fp32 chain's error bound (u x the magnitude of every rounded intermediate,
        propagated), on either axis: where the float64 chain cannot say which pixel the fp32 chain must pick.

    -> dict(sy, sx int64 [outH, outW] (valid where `inside`), inside bool, sy64, sx64, inside64, band bool, exact bool (the fp32
    chain made no rounding error anywhere: ix, iy equal their float64 values))."""
    xg, yg = np.asarray(xg, dtype=np.float32), np.asarray(yg, dtype=np.float32)
    r = np.asarray(rt, dtype=np.float32).reshape(6)
    bx = np.broadcast_to(xg[crop_x:crop_x + outW][None, :], (outH, outW))
    by = np.broadcast_to(yg[crop_y:crop_y + outH][:, None], (outH, outW))

    def chain(bx, by, ra, rb, rc, n, f):
        g = (bx * f(ra) + by * f(rb)) + f(rc)
        return g, (((g + f(1)) * f(n)) + f(-1)) / f(2)

    res = {}
    err = {}
    for name, ra, rb, rc, n in (("x", r[0], r[2], r[4], W), ("y", r[1], r[3], r[5], H)):
        g32, i32 = chain(bx, by, ra, rb, rc, n, np.float32)
        assert g32.dtype == np.float32 and i32.dtype == np.float32
        g64, i64 = chain(bx.astype(np.float64), by.astype(np.float64), ra, rb, rc, n, np.float64)
        # error of the fp32 chain: two products and two sums in g, then g + 1, x n, - 1 (the halving is exact)
        p, q = np.abs(bx.astype(np.float64) * ra), np.abs(by.astype(np.float64) * rb)
        eg = U * (p + q) + U * (p + q) + U * (np.abs(g64) + 2 * U * (p + q))
        e1 = eg + U * (np.abs(g64 + 1) + eg)
        e2 = e1 * n + U * (np.abs((g64 + 1) * n) + e1 * n)
        e3 = e2 + U * (np.abs((g64 + 1) * n - 1) + e2)
        err[name] = e3 / 2
        res["i" + name], res["i" + name + "64"] = i32, i64
    fx, fy = np.rint(res["ix"]), np.rint(res["iy"])
    res["inside"] = (fx >= 0) & (fx <= np.float32(W - 1)) & (fy >= 0) & (fy <= np.float32(H - 1))
    res["sx"], res["sy"] = fx.astype(np.int64), fy.astype(np.int64)
    fx64, fy64 = np.rint(res["ix64"]), np.rint(res["iy64"])
    res["inside64"] = (fx64 >= 0) & (fx64 <= W - 1) & (fy64 >= 0) & (fy64 <= H - 1)
    res["sx64"], res["sy64"] = fx64.astype(np.int64), fy64.astype(np.int64)
    half = lambda i: np.abs(i - (np.floor(i) + 0.5))  # noqa: E731
    res["band"] = (half(res["ix64"]) <= err["x"]) | (half(res["iy64"]) <= err["y"])
    res["exact"] = bool(np.array_equal(res["ix"].astype(np.float64), res["ix64"])
                        and np.array_equal(res["iy"].astype(np.float64), res["iy64"]))
    return res


def rotate_gather(src, ref):
    """What the kernel writes for planes src [C, H, W]: the source pixel the fp32 replica names, 0 outside."""
    src = np.asarray(src)
    sy, sx = np.where(ref["inside"], ref["sy"], 0), np.where(ref["inside"], ref["sx"], 0)
    return np.where(ref["inside"][None], src[:, sy, sx], np.zeros((), dtype=src.dtype))


def rotate_setup(H, W, angle, expand):
    """What protosam_amd.rotate._rotate computes on the host, restated from torchvision's rotate (oracle/rotate.py):
    -> (xg, yg, rt [3, 2] fp32, ow, oh)."""
    from oracle import rotate as orot
    matrix = orot.inverse_rotation_matrix(-angle)
    ow, oh = orot.affine_output_size(matrix, W, H) if expand else (W, H)
    xg, yg = orot.base_grid_axes(ow, oh)
    rt = orot.rescaled_theta(matrix, W, H)[0].contiguous()
    return xg, yg, rt, ow, oh


# ---- psam_resize_aa ------------------------------------------------------------------------------------------------------
def aa_axis(n_in, n_out):
    """One axis of the separable anti-aliased resize -> (xmin [n_out], xsize [n_out], Wn [n_out, n_in], EW [n_out, n_in],
    gam [n_out]).

    xmin / xsize: the kernel's fp32 rule, reproduced exactly in numpy float32 (scale = in / out, support = max(scale, 1),
    centre = scale (i + 0.5), taps [int(centre - support + 0.5), int(centre + support + 0.5)) clipped to the input).
    Wn: the triangle weights 1 - |(j - centre + 0.5) invscale| (zero beyond 1) normalised to sum 1, in float64 from the fp32
    centre and invscale. EW: a bound on the absolute error of the kernel's fp32 normalised weight - the four roundings of a weight
    (difference, + 0.5, product, 1 - a: u x each result), the xsize sums of the total (gamma(xsize) x total), the normalising
    divide (u). gam = gamma(xsize): the xsize multiply-adds of the pass (fused or not: at most two roundings per tap, the product
    being relative to its own term)."""
    f = np.float32
    scale = f(n_in) / f(n_out)
    support = scale if scale >= 1 else f(1)
    invscale = f(1) / scale if scale >= 1 else f(1)
    center = (scale * (np.arange(n_out, dtype=np.float32) + f(0.5))).astype(np.float32)
    xmin = np.maximum(((center - support) + f(0.5)).astype(np.float32).astype(np.int64), 0)      # (int) truncates toward zero
    xmax = np.minimum(((center + support) + f(0.5)).astype(np.float32).astype(np.int64), n_in)
    xsize = xmax - xmin
    j = np.arange(n_in, dtype=np.float64)[None, :]
    c64, inv64 = center.astype(np.float64)[:, None], np.float64(invscale)
    taken = (j >= xmin[:, None]) & (j < xmax[:, None])
    t = j - c64
    a = np.abs((t + 0.5) * inv64)
    w = np.where(taken & (a < 1.0), 1.0 - a, 0.0)
    ew = np.where(taken, U * ((np.abs(t) + np.abs(t + 0.5)) * inv64 + a + np.abs(1.0 - a)), 0.0)
    total = w.sum(1, keepdims=True)
    etotal = ew.sum(1, keepdims=True) + gamma(np.maximum(xsize, 1))[:, None] * total
    nz = total != 0
    tot = np.where(nz, total, 1.0)
    wn = w / tot
    ewn = np.where(taken, (ew + wn * etotal) / tot * (1.0 + 4 * U) + U * wn, 0.0)
    return xmin, xsize, wn, ewn, gamma(2 * np.maximum(xsize, 1))


def resize_aa_ref(x, OH, OW):
    """planes [C, H, W] -> (value, bound) float64 [C, OH, OW]: width pass, then height pass on its result, as the kernel. The
    width pass's bound is an input error of the height pass (its weights sum to 1 within their own error) and the intermediate is
    stored as the fp32 the accumulator already is (no further rounding)."""
    x = np.asarray(x, dtype=np.float64)
    C, H, W = x.shape
    _, _, wx, ewx, gx = aa_axis(W, OW)
    _, _, wy, ewy, gy = aa_axis(H, OH)
    t = x @ wx.T                                                           # [C, H, OW]
    bt = np.abs(x) @ ewx.T + gx[None, None, :] * (np.abs(x) @ wx.T)
    v = np.einsum("oh,chw->cow", wy, t)
    at = np.abs(t) + bt
    b = np.einsum("oh,chw->cow", wy + ewy, bt) + np.einsum("oh,chw->cow", ewy, at) + gy[None, :, None] * np.einsum("oh,chw->cow", wy, at)
    return v, b


# ---- input builders (shared by the CPU and the GPU test) -----------------------------------------------------------------
def _gen(seed):
    return np.random.default_rng(seed)


STATS_SIZES = [1, 255, 256, 257, 256 * 16 * 2048 + 4097]      # one voxel; one block, just under / over; the grid-stride loop wraps


def stats_volume(dt, n, seed, integers=True):
    """A flat volume of n voxels of dtype code dt. Integer-valued (exactly summable); int16 holds both extremes, int32 values
    above 2^24 (odd ones: the fp32 conversion rounds them) and both extremes, uint8 0 and 255, float32 integers up to 2^20."""
    g = _gen(seed)
    if dt == 0:
        v = g.integers(-2000, 3000, n).astype(np.int16)
        sp = [-32768, 32767]
    elif dt == 2:
        v = g.integers(0, 256, n).astype(np.uint8)
        sp = [0, 255]
    elif dt == 3:
        v = g.integers(-5000, 5000, n).astype(np.int32)
        sp = [2 ** 24 + 1, -(2 ** 24) - 3, 2 ** 31 - 1, -(2 ** 31), 2 ** 25 + 2]
    else:
        v = g.integers(-1000, 1000, n).astype(np.float32)
        sp = [2.0 ** 20, -(2.0 ** 20) + 1]
    for k, s in enumerate(sp):                      # spread through the volume, the first at element 0 (n = 1 keeps sp[0])
        if k < n:
            v[(k * (n // len(sp))) % n if k else 0] = s
    return v


SLICE_SHAPES = [(1, 1, 4), (1, 7, 5), (5, 1, 3), (8, 8, 8), (97, 131, 64), (30, 26, 257), (300, 260, 256)]   # (H, W, S)
SLICE_NORM = dict(slope=0.37, inter=-12.5, mean=41.3, inv_std=1.0 / 57.9)


def slice_volume(dt, Z, H, W, seed):
    g = _gen(seed)
    if dt == 0:
        return g.integers(-1024, 3072, (Z, H, W)).astype(np.int16)
    if dt == 2:
        return g.integers(0, 256, (Z, H, W)).astype(np.uint8)
    if dt == 3:
        v = g.integers(-100000, 100000, (Z, H, W)).astype(np.int32)
        v.flat[0] = 2 ** 24 + 1
        return v
    return (g.standard_normal((Z, H, W)) * 300.0 + 100.0).astype(np.float32)


def label_volume(dt, Z, H, W, seed):
    """Label values 0 .. 4 with 0 and 255 planted (255 as far as the dtype goes: all four hold it)."""
    v = _gen(seed).integers(0, 5, (Z, H, W))
    v.flat[0], v.flat[-1] = 255, 0
    if v.size > 2:
        v.flat[v.size // 2] = 255
    return v.astype(NP_DT[dt])


IM2COL_KERNELS = [(3, 3, 1, 1, 1), (3, 3, 2, 1, 1), (3, 3, 1, 2, 2), (3, 3, 1, 4, 4), (1, 1, 2, 1, 0), (1, 3, 1, 1, 0),
                  (3, 2, 1, 1, 1), (3, 3, 1, 1, 0)]                       # (kh, kw, stride, dil, pad)
IM2COL_MAPS = [(1, 1), (1, 5), (2, 3), (19, 23)]
IM2COL_C = [8, 64, 264]


def im2col_cases(valid=True):
    """(kh, kw, stride, dil, pad, H, W) over IM2COL_KERNELS x IM2COL_MAPS with an output (valid) or without one (the map is smaller
    than the dilated kernel: psam_im2col rejects it)."""
    return [k + m for k in IM2COL_KERNELS for m in IM2COL_MAPS
            if (conv_out(m[0], k[0], k[2], k[3], k[4]) > 0 and conv_out(m[1], k[1], k[2], k[3], k[4]) > 0) == valid]


def coded_map(B, H, W, C, encoding):
    """A token-major half map [B, H*W, C] whose values name their position, as far as halves allow (integers up to 2048 are exact
    in half). Encoding 0: 1 + (7 b + 13 y + 29 x + 3 c) mod 2039; encoding 1: 1 + (11 b + 31 y + 17 x + 5 c + 977) mod 2029 (two
    primes: a transposed, shifted or channel-rotated gather cannot satisfy both). Never zero: every zero of an im2col output is
    padding."""
    b, y, x, c = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    if encoding == 0:
        v = 1 + (7 * b + 13 * y + 29 * x + 3 * c) % 2039
    else:
        v = 1 + (11 * b + 31 * y + 17 * x + 5 * c + 977) % 2029
    return torch.from_numpy(v.astype(np.float32)).half().reshape(B, H * W, C)


STEM_IMAGES = [(1, 1), (2, 2), (7, 9), (37, 41)]
STEM_LDO = [152, 192, 256]


def stem_image(B, H, W, seed):
    """fp32 [B, 3, H, W]: values that need rounding to half, with (first elements, as far as the image goes) a tie that rounds to
    even downwards and one upwards, a value that overflows half to inf, the largest value that still rounds to 65504, a half
    subnormal, a value that rounds to a subnormal, and one below half the smallest subnormal (rounds to 0)."""
    x = torch.randn((B, 3, H, W), generator=torch.Generator().manual_seed(seed)) * 3.0
    special = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 70000.0, 65519.0, 2.0 ** -24, 1.3 * 2.0 ** -20, 2.0 ** -26,
                            -65520.0, -(1.0 + 2.0 ** -11)])
    flat = x.view(-1)
    k = min(flat.numel(), special.numel())
    flat[flat.numel() - k:] = special[:k]          # the last pixels of the last plane: inside the map at every size
    return x


POOL_MAPS = [(1, 1), (2, 2), (3, 4), (19, 23), (16, 16)]
POOL_C = [1, 8, 128, 136]


def pool_map(B, H, W, C, kind, seed):
    """Token-major half map [B, H*W, C]: "negative" (all below zero: the -inf start matters), "inf" (random with -inf and +inf
    entries, one window all -inf where the map is large enough), "ties" (three values only: equal maxima everywhere)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "negative":
        x = -(torch.rand((B, H, W, C), generator=g) * 100.0 + 0.5)
    elif kind == "ties":
        x = torch.randint(-1, 2, (B, H, W, C), generator=g).float()
    else:
        x = torch.randn((B, H, W, C), generator=g) * 10.0
        m = torch.rand((B, H, W, C), generator=g)
        x[m < 0.1] = float("-inf")
        x[m > 0.93] = float("inf")
        x[:, :3, :3] = float("-inf")               # the first window (rows / columns -1 .. 1) holds nothing else
    return x.half().reshape(B, H * W, C)


GEMM_M = [1, 127, 128, 129, 300]
GEMM_N = [128, 384]           # the GEMM's contract is N % 128 == 0: one tile column, and an odd number of them
GEMM_N_REJECTED = [64, 320]
GEMM_K = [64, 192, 4608]


def gemm_operands(M, N, K, seed, integers=False):
    """(a [M, K], w [N, K], bias [N] fp32, resid [M, N]) halves. Random: a ~ randn, w ~ randn / sqrt(K), resid ~ randn.
    integers: a, w in {-2 .. 2}, bias and resid small integers: every partial sum is an integer below 2^24 (|sum| <= 4 K <= 18432)
    and the result an integer below 2048 (the CPU test checks it):
    exact in fp32 and in half, in any summation order."""
    g = torch.Generator().manual_seed(seed)
    if integers:
        a = torch.randint(-2, 3, (M, K), generator=g).half()
        w = torch.randint(-2, 3, (N, K), generator=g).half()
        bias = torch.randint(-8, 9, (N,), generator=g).float()
        resid = torch.randint(-16, 17, (M, N), generator=g).half()
        return a, w, bias, resid
    a = torch.randn((M, K), generator=g).half()
    w = (torch.randn((N, K), generator=g) / K ** 0.5).half()
    return a, w, torch.randn(N, generator=g), torch.randn((M, N), generator=g).half()


# rotation inputs: (H, W, angle, expand). tests/test_frontend_reference_cpu.py checks the band cap on each of them.
# 45 degrees on the square map and -30 / 60 degrees at 17 x 23 put 2 to 6 % of the pixels on structural ties that the fp32 chain
# reaches only approximately (above the cap: left out); the structural tie that is kept is `tie_case`, which the replica decides
# exactly.
ROTATE_CASES = [(1, 1, 30.0, True), (1, 1, 30.0, False), (2, 3, 20.0, True), (2, 3, 20.0, False), (17, 23, 33.0, True),
                (17, 23, -77.0, False), (64, 64, -30.0, True), (64, 64, 10.0, False), (64, 64, -77.0, False),
                (96, 130, -30.0, True), (96, 130, 123.0, False), (96, 130, 7.5, True)]
ROTATE_BAND_CAP = 0.01


def tie_case(n=64):
    """A structural-tie input the replica decides unambiguously: the identity matrix on an n x n source (n a power of two: 2 / n
    is exact) sampled on the base grid of an (n + 1)-wide canvas, whose values are integers: every i = j - 0.5 is an exact
    half-integer in fp32 and in float64 alike (no operation of the chain rounds), so round-half-to-even alone decides, down at
    even j, up at odd j. -> (H, W, xg, yg, rt, ow, oh)."""
    from oracle import rotate as orot
    xg, yg = orot.base_grid_axes(n + 1, n + 1)
    rt = torch.tensor([[2.0 / n, 0.0], [0.0, 2.0 / n], [0.0, 0.0]], dtype=torch.float32)
    return n, n, xg, yg, rt, n + 1, n + 1


AA_CASES = [(1, 1, 3, 3), (1, 9, 1, 4), (7, 1, 2, 1), (33, 47, 33, 47), (50, 70, 20, 31), (40, 40, 100, 90), (64, 64, 3, 5),
            (5, 5, 129, 130)]       # (H, W, OH, OW)


AA_RANGE_CASES = [(1, 9, 1, 4), (7, 1, 2, 1), (50, 70, 20, 31)]


def aa_outside_range(n_in, n_out, pos):
    """bool [n_out]: the outputs of one axis whose tap range [xmin, xmin + xsize) does not hold input index `pos`."""
    xmin, xsize = aa_axis(n_in, n_out)[:2]
    return (pos < xmin) | (pos >= xmin + xsize)


def aa_planes(C, H, W, seed):
    """C planes of 5 * randn; the last (C = 3) is 1e3 + randn: cancellation in the weights shows there."""
    x = torch.randn((C, H, W), generator=torch.Generator().manual_seed(seed)) * 5.0
    if C >= 3:
        x[-1] += 1e3
    return x
