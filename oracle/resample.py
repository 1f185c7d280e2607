"""References for the resampling / packing kernels of csrc/resample.hip: plain restatements on the CPU, float64 where the operation
rounds (with the magnitudes an fp32 implementation's error is measured against), bit-exact where it only moves or truncates values.

Written from the header comments of csrc/resample.hip and csrc/interp.h and from ATen's published rules (UpSample.h:
area_pixel_compute_scale / area_pixel_compute_source_index / nearest_idx). tests/test_resample_reference_cpu.py pins them to stock
torch on the CPU; tests/test_resample_kernels_gpu.py holds the kernels to them.
"""
import math

import numpy as np
import torch


# ---- resizing ------------------------------------------------------------------------------------------------------------
def _scale(in_size, out_size, align_corners):
    """The scale as the fp32 quotient the kernels and ATen use."""
    if align_corners:
        return float(np.float32(in_size - 1) / np.float32(out_size - 1)) if out_size > 1 else 0.0
    return float(np.float32(in_size) / np.float32(out_size))


def source_index(in_size, out_size, align_corners=False):
    """Per output index: (src, i0, i1, l1) - the source coordinate in float64 from the fp32 scale, clamped at 0, its integer part
    (never past the last sample), the neighbour i1 = i0 + (i0 < in - 1) and the weight of i1."""
    dst = torch.arange(out_size, dtype=torch.float64)
    s = _scale(in_size, out_size, align_corners)
    src = s * dst if align_corners else (s * (dst + 0.5) - 0.5).clamp_min(0.0)
    i0 = src.floor().long().clamp_max(in_size - 1)
    i1 = i0 + (i0 < in_size - 1).long()
    l1 = (src - i0.double()).clamp(0.0, 1.0)
    return src, i0, i1, l1


def bilinear(x, OH, OW, align_corners=False):
    """F.interpolate(x, (OH, OW), 'bilinear') of planes [P, IH, IW] in float64 -> (value, blend, weights), each [P, OH, OW].

    blend   = the same four-term blend of |p|: what the roundings of the products and sums cost (in units of 2^-23).
    weights = max(src_y, 1) * (blend over x of |p10 - p00|, |p11 - p01|) + max(src_x, 1) * (blend over y of |p01 - p00|,
              |p11 - p10|): what one fp32 ulp of the source coordinate costs. An implementation may or may not contract
              scale * (dst + 0.5) - 0.5 into an FMA; bilinear is continuous in the coordinate, so this term also covers i0 landing on
              the other side of an integer."""
    x = torch.as_tensor(x).double()
    assert x.dim() == 3
    IH, IW = x.shape[-2:]
    sy, y0, y1, ly1 = source_index(IH, OH, align_corners)
    sx, x0, x1, lx1 = source_index(IW, OW, align_corners)
    ly1, lx1 = ly1[None, :, None], lx1[None, None, :]
    ly0, lx0 = 1.0 - ly1, 1.0 - lx1
    r0, r1 = x[:, y0], x[:, y1]
    p00, p01, p10, p11 = r0[:, :, x0], r0[:, :, x1], r1[:, :, x0], r1[:, :, x1]
    val = ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11)
    blend = ly0 * (lx0 * p00.abs() + lx1 * p01.abs()) + ly1 * (lx0 * p10.abs() + lx1 * p11.abs())
    dy = lx0 * (p10 - p00).abs() + lx1 * (p11 - p01).abs()
    dx = ly0 * (p01 - p00).abs() + ly1 * (p11 - p10).abs()
    weights = sy.clamp_min(1.0)[None, :, None] * dy + sx.clamp_min(1.0)[None, None, :] * dx
    return val, blend, weights


def nearest_index(in_size, out_size):
    """min(floor(fp32(dst) * fp32(in / out)), in - 1), evaluated in numpy float32."""
    s = np.float32(in_size) / np.float32(out_size)
    i = np.floor(np.arange(out_size, dtype=np.float32) * s).astype(np.int64)
    return torch.from_numpy(np.minimum(i, in_size - 1))


def nearest(x, OH, OW):
    """F.interpolate(x, (OH, OW), 'nearest') of [..., IH, IW]: copies values, so it is exact in any dtype."""
    x = torch.as_tensor(x)
    return x[..., nearest_index(x.shape[-2], OH), :][..., nearest_index(x.shape[-1], OW)]


# ---- two-class softmax ---------------------------------------------------------------------------------------------------
def softmax2_argmax(l0, l1):
    """softmax over (l0, l1) in float64 -> (p0, p1, argmax with "first maximum on a tie", margin |l1 - l0|)."""
    l0, l1 = torch.as_tensor(l0).double(), torch.as_tensor(l1).double()
    m = torch.maximum(l0, l1)
    e0, e1 = (l0 - m).exp(), (l1 - m).exp()
    s = e0 + e1
    return e0 / s, e1 / s, (l1 > l0).to(torch.uint8), (l1 - l0).abs()


# ---- image hand-off ------------------------------------------------------------------------------------------------------
def quantise(img, lo, hi):
    """((x - lo) / (hi - lo) * 255).astype(uint8) in numpy float32, operation by operation: a bit-exact reference."""
    x = np.asarray(img, dtype=np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    return ((x - lo) / (hi - lo) * np.float32(255.0)).astype(np.uint8)


def normalise(x, mean, std):
    """(x - mean[c]) / std[c] on [..., 3, H, W] in float64."""
    x = torch.as_tensor(x).double()
    mean = torch.as_tensor(mean, dtype=torch.float64).view(3, 1, 1)
    std = torch.as_tensor(std, dtype=torch.float64).view(3, 1, 1)
    return (x - mean) / std


def ord_encode(x):
    """The order-preserving uint32 code psam_minmax keeps its extremes in: negative floats complemented, the others with the sign
    bit set, so unsigned order equals float order."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def ord_decode(u):
    """Inverse of `ord_encode`: uint32 (or the int32 view of it) -> float32."""
    u = np.ascontiguousarray(u)
    u = u.view(np.uint32) if u.dtype == np.int32 else u.astype(np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7fffffff), ~u).astype(np.uint32).view(np.float32)


# ---- packing -------------------------------------------------------------------------------------------------------------
def patchify(img, P, Kpad):
    """im2col of a P x P / stride P conv: [B, C, S, S'] -> [B * (S/P) * (S'/P), Kpad], column c*P*P + ky*P + kx, zero tail."""
    img = torch.as_tensor(img)
    B, C, H, W = img.shape
    assert H % P == 0 and W % P == 0 and Kpad >= C * P * P
    rows = img.reshape(B, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // P) * (W // P), C * P * P)
    out = torch.zeros((rows.shape[0], Kpad), dtype=img.dtype)
    out[:, :C * P * P] = rows
    return out


def im2col3x3(x, B, H, W, C):
    """im2col of a 3x3 / pad 1 conv on a token-major map: [B, H*W, C] -> [B*H*W, 9*C], column (ky*3 + kx)*C + c =
    x[b, (y + ky - 1)*W + (x + kx - 1), c], zero outside the map."""
    x = torch.as_tensor(x).reshape(B, H, W, C)
    pad = torch.zeros((B, H + 2, W + 2, C), dtype=x.dtype)
    pad[:, 1:H + 1, 1:W + 1] = x
    taps = [pad[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)]
    return torch.stack(taps, dim=3).reshape(B * H * W, 9 * C)


# ---- element-wise --------------------------------------------------------------------------------------------------------
def split_f16(x, hi=None):
    """fp32 -> (hi, lo) halves: hi = half(x) (or the one given), lo = half(x - float(hi)) with the difference in float32."""
    x = torch.as_tensor(x).float()
    hi = x.half() if hi is None else hi
    return hi, (x - hi.float()).half()


def gelu_erf(x):
    """nn.GELU in its erf form, float64."""
    x = torch.as_tensor(x).double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
