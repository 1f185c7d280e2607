"""Host restatements that the image-intake tests compare against (no GPU, no project code).

`pillow_u8`  Pillow's 8-bit BILINEAR resampling (src/libImaging/Resample.c) in numpy: float64 triangle weights, 22-bit fixed point,
             width pass first with a uint8 intermediate, an unchanged axis skipped. Checked against Pillow itself in
             test_image_intake_cpu.py; the GPU tests then compare the kernel with Pillow directly.
`aten_f64`   the antialiased bilinear resize of aten `_upsample_bilinear2d_aa` (what F.interpolate(..., antialias=True) computes) in
             float64, with a bound on what an fp32 implementation of the same formulas may differ from it.
"""
import numpy as np

SIZES = [((37, 53), 64), ((100, 75), 64), ((64, 64), 64), ((33, 128), 64), ((50, 20), 128), ((288, 384), 128), ((13, 64), 128),
         ((700, 90), 64), ((1, 40), 64)]


def preprocess_shape(h, w, S):
    """ResizeLongestSide.get_preprocess_shape, restated"""
    scale = S * 1.0 / max(h, w)
    return (int(h * scale + 0.5), int(w * scale + 0.5))


def taps(insz, outsz):
    """per output index: (first source index, float64 weights summing to 1) of the triangle filter with support max(in/out, 1)"""
    scale = insz / outsz
    fs = max(scale, 1.0)
    out = []
    for i in range(outsz):
        center = (i + 0.5) * scale
        xmin = max(0, int(center - fs + 0.5))
        xmax = min(insz, int(center + fs + 0.5))
        x = np.arange(xmin, xmax)
        w = np.clip(1.0 - np.abs((x - center + 0.5) * (1.0 / fs)), 0, None)
        out.append((xmin, w / w.sum()))
    return out


def _q(w):
    return np.floor(0.5 + w * (1 << 22)).astype(np.int64)


def pillow_u8(img, oh, ow):
    """np.array(Image.fromarray(img).resize((ow, oh), Image.BILINEAR)) for uint8 img [H, W] or [H, W, C]"""
    a = np.asarray(img)
    flat = a.ndim == 2
    a = (a[:, :, None] if flat else a).astype(np.int64)
    H, W, C = a.shape
    if ow != W:
        b = np.empty((H, ow, C), np.int64)
        for i, (x0, w) in enumerate(taps(W, ow)):
            b[:, i] = np.clip(((1 << 21) + (a[:, x0:x0 + len(w)] * _q(w)[None, :, None]).sum(1)) >> 22, 0, 255)
        a = b
    if oh != H:
        b = np.empty((oh, a.shape[1], C), np.int64)
        for i, (y0, w) in enumerate(taps(H, oh)):
            b[i] = np.clip(((1 << 21) + (a[y0:y0 + len(w)] * _q(w)[:, None, None]).sum(0)) >> 22, 0, 255)
        a = b
    a = a.astype(np.uint8)
    return a[:, :, 0] if flat else a


U32 = 2.0 ** -24          # unit roundoff of fp32


def _axis_error(n_in, n_out):
    """(sum over the taps of |fp32 weight - exact weight|, taps) for one axis: see `aten_f64`"""
    scale = n_in / n_out
    sup = max(scale, 1.0)
    K = int(2 * sup) + 2
    da = (4 * U32 * n_in + 4 * U32 * (sup + 1)) / sup + 2 * U32
    dt = da + U32
    T = 0.5 * sup
    return (2 * K * dt + K * U32) / T + K * U32, K


def aten_f64(x, oh, ow, mean=None, std=None):
    """x [C, H, W] -> (ref float64 [C, oh, ow], budget float64 [C, oh, ow]).

    ref: width pass then height pass with the float64 weights of `taps`, then (v - mean[c]) / std[c] when mean is given.

    budget: a bound on |fp32 result - ref| for an implementation that evaluates the same formulas in fp32 with one rounding
    (unit roundoff u = 2^-24) per operation, M = max |x|:
      * coordinate: centre = scale * (i + 0.5) carries the rounding of scale and of the product, at most 2 u n_in (centre < n_in);
        (j - centre + 0.5) * invscale adds two roundings of a value below support + 1, the rounding of invscale and of the product:
        the filter argument is off by da <= (4 u n_in + 4 u (support + 1)) / support + 2 u, the un-normalised weight t = 1 - |a| by
        dt = da + u. The triangle is continuous, so a tap that fp32 takes or leaves at the end of the support changes t by no more.
      * weight: w = t / T with T = sum t >= support / 2 (at least half of the triangle lies inside the image) over at most
        K = floor(2 support) + 2 taps: sum |dw| <= (K dt) / T + (K dt + K u) / T + K u =: Ew (numerators, the sum, the divisions).
      * multiply-adds: K fused steps, each rounding a partial sum of magnitude at most M (1 + Ew).
      A pass therefore maps an input error e to e (1 + Ew) + M (Ew + K u) (1 + Ew); the two passes are chained, width first.
      * normalisation: the subtraction and the division round once each: e / std + 2 u (M + |mean|) / std.
    The bound is the same for every pixel of a channel (it uses M, not the local values)."""
    x = np.asarray(x, dtype=np.float64)
    C, H, W = x.shape
    tx, ty = taps(W, ow), taps(H, oh)
    b = np.stack([(x[:, :, x0:x0 + len(w)] * w).sum(-1) for x0, w in tx], -1)
    ref = np.stack([(b[:, y0:y0 + len(w)] * w[None, :, None]).sum(1) for y0, w in ty], 1)
    M = float(np.abs(x).max()) if x.size else 0.0
    e = 0.0
    for n_in, n_out in ((W, ow), (H, oh)):
        Ew, K = _axis_error(n_in, n_out)
        e = e * (1 + Ew) + M * (Ew + K * U32) * (1 + Ew)
    budget = np.full(ref.shape, e)
    if mean is not None:
        m = np.asarray(mean, dtype=np.float64).reshape(-1, 1, 1)
        s = np.asarray(std, dtype=np.float64).reshape(-1, 1, 1)
        ref = (ref - m) / s
        budget = budget / s + 2 * U32 * (M + np.abs(m)) / s
    return ref, budget


def random_image(h, w, c, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, c) if c else (h, w), dtype=np.uint8)


def single_pixel_image(h, w, c):
    a = np.zeros((h, w, c) if c else (h, w), np.uint8)
    a[h // 2, w // 3] = 255
    return a


def rect_mask(h, w, rects):
    m = np.zeros((h, w), np.uint8)
    for (y0, y1, x0, x1) in rects:
        m[y0:y1, x0:x1] = 1
    return m
