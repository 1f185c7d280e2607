"""References for the mask post-processing kernels (psam_mask_upsample / _union / _stats / _binarize, psam_plane_stats in
csrc/decoder.hip; psam_prob2_argmax, psam_scores_prob_argmax, psam_mask_union_seg in csrc/coarse_batch.hip): plain float64
restatements on the CPU with the magnitudes an fp32 implementation's error is measured against, and - because these kernels
threshold what they compute - the three-way split of every pixel into "surely set", "surely clear" and "inside the error band".

Written from the header comments of include/protosam_hip.h and csrc/interp.h on top of oracle/resample.py.
tests/test_maskpost_reference_cpu.py pins them to stock torch on the CPU; tests/test_mask_kernels_gpu.py holds the kernels to them.
The last section builds the inputs both test files use, so that the CPU file can show that the inputs leave (almost) no pixel
inside the band before a GPU test relies on that.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import resample as R

U = 2.0 ** -23
INT_MAX = 0x7fffffff


# ---- the first resize of postprocess_masks -------------------------------------------------------------------------------
def up_sample(low, MID, variant):
    """interpolate(low [P, IN, IN] fp32 -> [P, MID, MID]) in float64 -> (value, magnitude) per output pixel.

    variant 0 / 1: bilinear, align_corners False / True; magnitude = blend + weights of R.bilinear.
    variant 2: nearest: copies values, magnitude 0.
    variant 3: float64 sigmoid of the fp32 logits, then the variant-0 blend; magnitude = 2 blend + weights of the sigmoid planes
               (the second blend carries the fp32 sigmoid: expf, one add, one divide - a few ulps of a value <= 1)."""
    low = torch.as_tensor(low)
    assert low.dim() == 3 and low.shape[-1] == low.shape[-2]
    if variant in (0, 1):
        v, blend, weights = R.bilinear(low, MID, MID, align_corners=(variant == 1))
        return v, blend + weights
    if variant == 2:
        v = R.nearest(low.double(), MID, MID)
        return v, torch.zeros_like(v)
    if variant == 3:
        v, blend, weights = R.bilinear(torch.sigmoid(low.double()), MID, MID)
        return v, 2.0 * blend + weights
    raise ValueError(variant)


def thr32(thr, off=0.0, sign=0):
    """The fp32 number a kernel compares with: float(thr), or float(thr) +- float(off) added in fp32 - as a Python float."""
    t, o = np.float32(thr), np.float32(off)
    return float(t if sign == 0 else (t + o if sign > 0 else t - o))


def threshold(value, magnitude, t, c):
    """`x > t` for an fp32 x within c 2^-23 magnitude of `value` -> (sure1, sure0, band), three bool maps that partition the pixels.
    sure1: value > t + c U magnitude. sure0: value < t - c U magnitude, or value == t with magnitude 0 (an exact tie is not set:
    the comparison is strict). band: the rest - either answer is consistent with the bound."""
    e = c * U * magnitude
    sure1 = value > t + e
    sure0 = (value < t - e) | ((value == t) & (magnitude == 0))
    return sure1, sure0, ~(sure1 | sure0)


def union_fold(sure1, sure0, OUT):
    """OR over the prompts (dim 0 of [B, MID, MID]) and F.interpolate(..., 'nearest') MID -> OUT: a pixel is surely 1 if any prompt
    is surely 1 there, surely 0 if every prompt is surely 0 -> (sure1, sure0, band), each [OUT, OUT]."""
    idx = R.nearest_index(sure1.shape[-1], OUT)
    s1 = sure1.any(0)[idx][:, idx]
    s0 = sure0.all(0)[idx][:, idx]
    return s1, s0, ~(s1 | s0)


def box(mask):
    """(min_x, min_y, max_x, max_y) of the set pixels of [..., H, W], inclusive; INT_MAX, INT_MAX, -1, -1 for an empty set."""
    ys, xs = mask.any(-1), mask.any(-2)                      # [..., H], [..., W]
    H, W = mask.shape[-2:]
    ay, ax = torch.arange(H), torch.arange(W)
    big = torch.tensor(INT_MAX)
    mny = torch.where(ys, ay, big).amin(-1)
    mnx = torch.where(xs, ax, big).amin(-1)
    mxy = torch.where(ys, ay, torch.tensor(-1)).amax(-1)
    mxx = torch.where(xs, ax, torch.tensor(-1)).amax(-1)
    return torch.stack([mnx, mny, mxx, mxy], -1)


def counts_and_boxes(sure1, band):
    """From [..., H, W] maps -> (lo, hi, inner, outer): every count of `x > t` lies in [lo, hi] = [n(sure1), n(sure1) + n(band)];
    the box of `x > t` lies between inner = box(sure1) and outer = box(sure1 | band)."""
    lo = sure1.flatten(-2).sum(-1)
    return lo, lo + band.flatten(-2).sum(-1), box(sure1), box(sure1 | band)


def box_between(b, inner, outer):
    """outer.min <= b.min <= inner.min and inner.max <= b.max <= outer.max (an empty inner box allows everything inside outer)."""
    b, inner, outer = b.long(), inner.long(), outer.long()
    return ((outer[..., :2] <= b[..., :2]) & (b[..., :2] <= inner[..., :2]) &
            (inner[..., 2:] <= b[..., 2:]) & (b[..., 2:] <= outer[..., 2:])).all(-1)


# ---- the coarse model's class scores -------------------------------------------------------------------------------------
def softmax2_twice(l0, l1):
    """softmax over (l0, l1), then softmax over the two probabilities (util/utils.py:485 re-applies it) -> (p0, p1, argmax with
    ties to class 0, margin |l1 - l0|, q1 = foreground channel of the second softmax), float64."""
    p0, p1, am, margin = R.softmax2_argmax(l0, l1)
    _, q1, _, _ = R.softmax2_argmax(p0, p1)
    return p0, p1, am, margin, q1


def composed_resize(scores, IH, IW, OH, OW):
    """bilinear [P, GH, GW] -> (IH, IW), then bilinear of that float64 result -> (OH, OW) (skipped when equal) -> (value, magnitude).
    magnitude = the second stage's own blend + weights, plus its blend (the same four weights) of the first stage's magnitude map."""
    v1, b1, w1 = R.bilinear(scores, IH, IW)
    m1 = b1 + w1
    if (IH, IW) == (OH, OW):
        return v1, m1
    v2, b2, w2 = R.bilinear(v1, OH, OW)
    m1_through = R.bilinear(m1, OH, OW)[0]                  # m1 >= 0: its value is its blend
    return v2, b2 + w2 + m1_through


# ---- work distribution of coarse_batch.hip, restated from its header comment ---------------------------------------------
PB_ROW, PB_MAX_BLOCKS = 1024, 2048


def pb_grid(items):
    """(workgroups, items per workgroup): at most PB_MAX_BLOCKS workgroups, each walking a contiguous run of items."""
    g = min(items, PB_MAX_BLOCKS)
    per = -(-items // g)
    return -(-items // per), per


def pb_straddlers(rows_per_unit, OW, units):
    """Number of workgroups whose run of items holds the last item of one unit (plane / segment) and the first of the next."""
    per_unit = rows_per_unit * (-(-OW // PB_ROW))
    grid, per = pb_grid(per_unit * units)
    return sum(1 for b in range(grid) if (b * per) // per_unit != (min((b + 1) * per, per_unit * units) - 1) // per_unit)


# ---- inputs of the tests -------------------------------------------------------------------------------------------------
# (IN, MID, H, W): the smallest shapes at which each structure of the kernels has an edge (see tests/test_mask_kernels_gpu.py)
CASES = [(16, 64, 64, 64), (20, 77, 50, 77), (64, 250, 250, 250), (64, 300, 289, 300), (64, 256, 256, 256), (1, 5, 5, 5),
         (3, 1, 1, 1), (256, 1024, 1024, 1024), (256, 1024, 683, 1024)]
C_BOUND = 4                                   # |fp32 - float64| <= 4 x 2^-23 x magnitude: the bound of mask_upsample
NPLANES = 8
RANDOM, BIG, EDGE, EMPTY, FULL, ISLAND = (0, 1, 7), 2, 3, 4, 5, 6


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def noise(P, IN, seed):
    """P planes of 3 * randn; from IN >= 128 smooth (coarse noise up-sampled plus 0.02 x fine noise): the error band grows with the
    source coordinate times the difference of neighbouring samples, and white noise at 256 -> 1024 leaves 1.6e-4 of the pixels in
    it."""
    x = _rand((P, IN, IN), seed, 3.0)
    if IN >= 128:
        x = F.interpolate(_rand((1, P, IN // 16 + 2, IN // 16 + 2), seed, 3.0), size=(IN, IN), mode="bilinear")[0] + 0.02 * x
    return x.contiguous()


def levels(variant, thr, off):
    """(a value every up-sampled pixel of a plane filled with it keeps below thr - off, one above thr + off), as logits."""
    if variant == 3:
        return -5.0, 5.0                      # sigmoid: 0.0067 / 0.9933 against the threshold 0.5
    return thr - off - 1.5, thr + off + 2.25  # not symmetric about thr: a blend with weights 1/2, 1/2 must not land on it


def planes(IN, variant, thr=0.0, off=1.0):
    """The NPLANES logit planes of a case: 0, 1, 7 random (plane 0 with patches of +-100 and +-1e4 for variant 3, where the sigmoid
    saturates); 2 = 1e4 + randn (cancellation in the weights); 3 = zero (variant 3: -5) except its last row and last column (a wrong
    i1 clamp); 4 =
    everywhere below thr - off (empty); 5 = everywhere above thr + off (full); 6 = empty with one island of 3 x 1 samples."""
    seed = 1000 * IN + 10 * variant + int(round(10 * thr)) + 1
    x = noise(NPLANES, IN, seed)
    lo, hi = levels(variant, thr, off)
    x[BIG] = 1e4 + _rand((IN, IN), seed + 1)
    edge = torch.full((IN, IN), lo if variant == 3 else 0.0)       # sigmoid(0) is variant 3's threshold itself
    edge[-1, :] = 3.0 + torch.arange(IN, dtype=torch.float32)
    edge[:, -1] = -2.0 - torch.arange(IN, dtype=torch.float32)
    x[EDGE] = edge
    x[EMPTY] = lo - torch.rand((IN, IN), generator=torch.Generator().manual_seed(seed + 2))
    x[FULL] = hi + torch.rand((IN, IN), generator=torch.Generator().manual_seed(seed + 3))
    x[ISLAND] = lo
    r, c = IN // 3, (2 * IN) // 3
    x[ISLAND, r:min(r + 3, IN), c] = hi
    if variant == 3 and IN >= 16:
        x[0, 0:2, 0:2], x[0, 0:2, 3:5] = 100.0, -100.0
        x[0, 4:6, 0:2], x[0, 4:6, 3:5] = 1e4, -1e4
    return x.contiguous()


@functools.lru_cache(maxsize=None)
def case_reference(IN, MID, variant, thr=0.0, off=1.0):
    """(planes fp32 [NPLANES, IN, IN], value, magnitude [NPLANES, MID, MID] float64) of a case; computed once, never modified."""
    x = planes(IN, variant, thr, off)
    v, m = up_sample(x, MID, variant)
    return x, v, m


def planes70(variant, thr=0.3, off=1.0):
    """70 white-noise planes of 16 x 16 for one psam_mask_stats call; plane 13 is empty, plane 69 full."""
    x = noise(70, 16, 70 + variant)
    x[13], x[69] = thr - off - 2.0, thr + off + 2.0
    return x


def integer_planes(IN, P=4, seed=0):
    """Integer-valued logits in [-8, 8]: at a power-of-two ratio every weight is dyadic and every product and sum exact in fp32."""
    return torch.randint(-8, 9, (P, IN, IN), generator=torch.Generator().manual_seed(IN + seed)).float()


def class_scores(P, IH, IW, seed, smooth_from=40, tie_block=True):
    """[P, 2, IH, IW] two-class scores, 2 * randn (|l1 - l0| < 16), smooth from `smooth_from` rows on (the band of the argmax grows
    with the source coordinate times the difference of neighbouring samples: 73 -> 3 rows of white noise leaves 2e-3 of the pixels
    in it, and a grid that is resized twice carries the first resize's magnitude through the second); a block of (80, -80), a block of
    (-1e4, 1e4), on plane 0 a block of exact ties, plane 1 (P > 1) two identical channels, the last plane (P > 2) without
    foreground."""
    l = _rand((P, 2, IH, IW), seed, 2.0)
    if IH >= smooth_from:
        l = F.interpolate(_rand((P, 2, IH // 16 + 2, IW // 16 + 2), seed, 2.0), size=(IH, IW), mode="bilinear") + 0.02 * l
    if IH >= 2 and IW >= 5:
        l[:, 0, 0:2, 0:2], l[:, 1, 0:2, 0:2] = 80.0, -80.0
        l[:, 0, 0:2, 3:5], l[:, 1, 0:2, 3:5] = -1e4, 1e4
    if tie_block and IH >= 5 and IW >= 4:      # (only where nothing is resized: its rim is all band otherwise)
        l[0, 1, 3:5, 0:4] = l[0, 0, 3:5, 0:4]
    if P > 1:
        l[1, 1] = l[1, 0]
    if P > 2:
        l[-1, 0], l[-1, 1] = 3.0, -3.0
    return l.contiguous()


# (thr, off) per variant of the general cases. Not thr = 0: a zero sample next to a non-zero one gives pixels whose float64 value is
# exactly 0 with a non-zero magnitude wherever a source coordinate is an integer (align_corners at 20 -> 77 has the scale 1/4), and
# all of those are band. Exact ties at thr = 0 are what the exact-arithmetic cases are for. 0.3 is not representable in fp32.
THRESHOLDS = {0: ((0.3, 1.0), (0.3, 0.0)), 1: ((0.3, 1.0), (0.3, 0.0)), 2: ((0.3, 1.0), (0.3, 0.0)), 3: ((0.5, 0.0),)}
UNION_PROMPTS = {1: (0,), 3: (1, EDGE, ISLAND)}       # the planes of a case that act as the B prompts of a union


def union_outs(MID):
    """OUT in {MID, MID / 2, an odd size above MID, 1}."""
    return sorted({MID, max(MID // 2, 1), (MID + MID // 3) | 1, 1})


# (P, IH, IW, OH, OW) of psam_prob2_argmax: the tuples of test_prob2_argmax_equals_chain (odd OW, non-square, same-size with an odd
# and a multiple-of-four width), then 602 items per plane in runs of three, so that workgroups straddle plane boundaries
PROB2_CASES = [(3, 41, 53, 251, 333), (3, 73, 61, 3, 1023), (3, 47, 51, 47, 51), (3, 64, 52, 64, 52), (9, 40, 50, 301, 1100)]
# (P, GH, GW, IH, IW, OH, OW) of psam_scores_prob_argmax: IH, IW == OH, OW and the second-resize path, non-square, odd OW
SCORES_CASES = [(3, 9, 13, 60, 76, 60, 76), (3, 9, 13, 61, 75, 61, 75), (3, 16, 12, 64, 48, 251, 333), (3, 32, 32, 448, 448, 512, 512),
                (9, 10, 14, 40, 50, 301, 1100), (9, 10, 14, 301, 1100, 301, 1100)]


def argmax_band(margin, M, c=4):
    """(tie, sure, share): margin == 0; margin > c U M; the share of the untied pixels that are neither."""
    tie, sure = margin == 0, margin > c * U * M
    rest = margin.numel() - int(tie.sum())
    return tie, sure, (rest - int(sure.sum())) / max(rest, 1)


def case_scores(case):
    """The scores of a PROB2_CASES / SCORES_CASES entry."""
    return class_scores(case[0], case[1], case[2], sum(case), smooth_from=40 if len(case) == 5 else 8,
                        tie_block=len(case) == 5 and case[1:3] == case[3:5])
