"""Float64 reference of the two-stage value behind psam_mask_stats_resized / psam_mask_binarize_resized (csrc/amg_resize.hip), the
cases and input planes of tests/test_amg_resize_cpu.py and tests/test_amg_resize_gpu.py, and the checks the GPU file applies - kept
here so that the CPU file can show, without a GPU, that the inputs leave almost no pixel inside the error band and that each
injected fault fails those checks.

The value of pixel (y, x) of the OH x OW image is Sam.postprocess_masks' second resize - source size ih x iw, the un-padded corner
of the first-stage map - of the first resize IN -> MID (oracle.maskpost.up_sample); bilinear with align_corners False / True for
variants 0 / 1 (oracle.resample.bilinear), nearest for variant 2 (oracle.resample.nearest). The magnitude an fp32 implementation's
error is measured against is the second stage's own blend + weights plus its blend of the first stage's magnitude map, as
oracle.maskpost.composed_resize carries it; a second stage that changes nothing (ih x iw == OH x OW) is skipped, as
postprocess_masks skips it.
"""
import functools

import torch

from oracle import maskpost as M
from oracle import resample as R

U = M.U
C_BOUND = M.C_BOUND                 # each stage is a four-tap blend held to 4 x 2^-23 x its magnitude (oracle.maskpost.C_BOUND)
THR, OFF = 0.3, 1.0                 # the generator's offset; 0.3 is not representable in fp32 (oracle.maskpost.THRESHOLDS)
FILL = 0xAB                         # what the frames hold before a call
POISON = M.NPLANES                  # index of the added plane

# (IN, MID, ih, iw, OH, OW): the smallest shapes at which each thing can go wrong
CASES = [(16, 64, 64, 47, 37, 27),          # down-scaling; one wave's worth of columns
         (32, 128, 96, 128, 225, 300),      # up-scaling; OW > 256: the column loop strides; OH not a multiple of 32
         (64, 256, 256, 171, 600, 401),     # many row blocks
         (64, 256, 200, 256, 50, 64),       # 4x down
         (32, 128, 128, 77, 333, 200),      # narrow crop
         (32, 128, 128, 128, 128, 128)]     # identity second stage: must equal psam_mask_stats / psam_mask_binarize exactly
VARIANTS = (0, 1, 2)
# faults of test_amg_resize_cpu.py::test_injected_faults
FAULTS = ("clamp_mid", "swap_ih_iw", "drop_align_stage1", "drop_align_stage2", "nearest_off_by_one")


def reach(IN, MID, n, variant):
    """Number of low-resolution rows (columns) the first-stage taps of up-sampled rows 0 .. n - 1 can read."""
    if variant == 2:
        return int(R.nearest_index(IN, MID)[:n].max()) + 1
    return int(R.source_index(IN, MID, variant == 1)[2][:n].max()) + 1


def poison_plane(IN, MID, ih, iw, variant):
    """Zero on the low-resolution rows and columns that the taps of the ih x iw corner can reach, +1e4 on the rows and -1e4 on the
    columns beyond them: the true value is 0 everywhere, and a tap that reads the padding moves a count by thousands."""
    p = torch.zeros((IN, IN))
    p[reach(IN, MID, ih, variant):, :] = 1e4
    p[:, reach(IN, MID, iw, variant):] = -1e4
    return p


def tie_plane(IN):
    """Every sample exactly fp32(THR): nearest copies it, `>` leaves the mask empty, `>=` would fill it."""
    return torch.full((IN, IN), M.thr32(THR))


def inputs(case, variant):
    """fp32 [NPLANES + 1, IN, IN]: oracle.maskpost.planes (random, large-offset, edge, empty, full, island) + the poison plane."""
    IN, MID, ih, iw = case[:4]
    return torch.cat([M.planes(IN, variant, THR, OFF), poison_plane(IN, MID, ih, iw, variant)[None]]).contiguous()


def two_stage(low, MID, ih, iw, OH, OW, variant, fault=None):
    """(value, magnitude) float64 [P, OH, OW] of planes `low` fp32 [P, IN, IN]. `fault` injects one of FAULTS."""
    a1 = variant == 1 and fault != "drop_align_stage1"
    a2 = variant == 1 and fault != "drop_align_stage2"
    v1, m1 = M.up_sample(low, MID, variant if variant == 2 else (1 if a1 else 0))
    if fault == "swap_ih_iw":
        ih, iw = iw, ih
    if fault == "clamp_mid":                # the second stage's neighbour taps run on into the padding
        ch, cw = min(ih + 1, MID), min(iw + 1, MID)
    else:
        ch, cw = ih, iw
    v1, m1 = v1[:, :ch, :cw], m1[:, :ch, :cw]
    if variant == 2:
        first = R.nearest_index(low.shape[-1], MID)             # the two index maps composed: a copy of one input sample
        fy, fx = first[R.nearest_index(ih, OH)], first[R.nearest_index(iw, OW)]
        if fault == "nearest_off_by_one":
            fy = (fy + 1).clamp_max(low.shape[-1] - 1)
        v = torch.as_tensor(low).double()[:, fy][:, :, fx]
        assert fault is not None or torch.equal(v, R.nearest(v1, OH, OW))
        return v, torch.zeros_like(v)
    if (ih, iw) == (OH, OW) and fault is None:
        return v1, m1
    if fault == "clamp_mid":
        return _bilinear_open(v1, m1, ih, iw, OH, OW, a2)
    v2, b2, w2 = R.bilinear(v1, OH, OW, a2)
    return v2, b2 + w2 + R.bilinear(m1, OH, OW, a2)[0]       # m1 >= 0: its value is its blend


def _bilinear_open(v1, m1, ih, iw, OH, OW, align):
    """the clamp_mid fault: source coordinates of an ih x iw source, neighbour taps i0 + 1 allowed up to the array's end"""
    sy, y0, _, ly1 = R.source_index(ih, OH, align)
    sx, x0, _, lx1 = R.source_index(iw, OW, align)
    y1, x1 = (y0 + 1).clamp_max(v1.shape[-2] - 1), (x0 + 1).clamp_max(v1.shape[-1] - 1)
    ly1, lx1 = ly1[None, :, None], lx1[None, None, :]

    def blend(p):
        r0, r1 = p[:, y0], p[:, y1]
        return (1 - ly1) * ((1 - lx1) * r0[:, :, x0] + lx1 * r0[:, :, x1]) + ly1 * ((1 - lx1) * r1[:, :, x0] + lx1 * r1[:, :, x1])
    return blend(v1), blend(v1.abs()) + blend(m1)


@functools.lru_cache(maxsize=None)
def case_reference(case, variant):
    """(planes fp32, value, magnitude float64 [NPLANES + 1, OH, OW]) of a case; computed once, shared, never modified."""
    x = inputs(case, variant)
    v, m = two_stage(x, *case[1:], variant)
    return x, v, m


@functools.lru_cache(maxsize=None)
def sure_maps(case, variant):
    """[(sure1, sure0, band)] at thr + off, thr - off, thr - the order of the statistics columns."""
    _, v, m = case_reference(case, variant)
    return [M.threshold(v, m, M.thr32(THR, OFF, sign), C_BOUND) for sign in (1, -1, 0)]


def band_share(case, variant):
    """the largest share of a case's pixels inside the error band over the three thresholds"""
    return max(int(b.sum()) for _, _, b in sure_maps(case, variant)) / sure_maps(case, variant)[0][0].numel()


# ---- what the kernels are modelled as on the CPU, and the checks of the GPU file ------------------------------------------------
def model_outputs(v, y0=0, x0=0, FH=None, FW=None, ge=False, place=True):
    """What a kernel computing exactly the float64 value `v` [P, OH, OW] returns: (stats int64 [P, 8], frames uint8 [P, FH, FW]
    pre-filled with FILL, mask at (y0, x0)). `ge` compares with >=, `place=False` ignores the offset: two more injected faults."""
    P, OH, OW = v.shape
    FH, FW = FH or y0 + OH, FW or x0 + OW
    cmp = (lambda a, t: a >= t) if ge else (lambda a, t: a > t)
    m = [cmp(v, M.thr32(THR, OFF, sign)) for sign in (1, -1, 0)]
    stats = torch.cat([torch.stack([k.flatten(1).sum(1) for k in m], 1), M.box(m[2]), torch.zeros((P, 1), dtype=torch.long)], 1)
    frames = torch.full((P, FH, FW), FILL, dtype=torch.uint8)
    oy, ox = (y0, x0) if place else (0, 0)
    frames[:, oy:oy + OH, ox:ox + OW] = m[2].to(torch.uint8)
    return stats, frames


def check_stats(stats, maps, what):
    """stats [P, 8] against [(sure1, sure0, band)] at thr + off, thr - off, thr: every count inside [lo, hi], the box between the
    inner and the outer box, an empty mask INT_MAX, INT_MAX, -1, -1, column 7 zero. -> the number of planes that had to be exact."""
    st = stats.cpu().long()
    assert bool((st[:, 7] == 0).all()), f"{what}: column 7"
    exact = 0
    for col, (s1, s0, band) in enumerate(maps):
        lo, hi, inner, outer = M.counts_and_boxes(s1, band)
        ok = (lo <= st[:, col]) & (st[:, col] <= hi)
        assert bool(ok.all()), (f"{what}: count {col} of planes {(~ok).nonzero().flatten().tolist()} outside "
                                f"[{lo.tolist()}, {hi.tolist()}]: {st[:, col].tolist()}")
        if col == 2:
            okb = M.box_between(st[:, 3:7], inner, outer)
            assert bool(okb.all()), (f"{what}: box of planes {(~okb).nonzero().flatten().tolist()}: {st[:, 3:7].tolist()} not "
                                     f"between {inner.tolist()} and {outer.tolist()}")
            empty = hi == 0
            assert torch.equal(st[empty, 2:7], torch.tensor([0, M.INT_MAX, M.INT_MAX, -1, -1]).expand(int(empty.sum()), 5)), what
            exact = int((lo == hi).sum())
    return exact


def check_frames(frames, sure1, sure0, y0, x0, what, fill=FILL):
    """frames uint8 [n, FH, FW]: inside the rectangle at (y0, x0) 1 on sure1 and 0 on sure0, outside it still `fill`."""
    f = frames.cpu()
    n, OH, OW = sure1.shape
    inside = f[:, y0:y0 + OH, x0:x0 + OW]
    assert bool(((inside == 0) | (inside == 1)).all()), f"{what}: values other than 0 / 1 inside the rectangle (unwritten?)"
    n1, n0 = int((inside[sure1] != 1).sum()), int((inside[sure0] != 0).sum())
    assert n1 == 0 and n0 == 0, f"{what}: {n1} surely-set pixels clear, {n0} surely-clear pixels set"
    outside = torch.ones(f.shape[1:], dtype=torch.bool)
    outside[y0:y0 + OH, x0:x0 + OW] = False
    assert bool((f[:, outside] == fill).all()), f"{what}: bytes outside the rectangle written"


def check_counts(counts, label_rect, sure1, sure0, what):
    """counts int64 [n, 3] = {tp, fp, fn} against label_rect bool [OH, OW] (the label inside the rectangle): each between what the
    sure maps allow."""
    c = counts.cpu().long()
    band = ~(sure1 | sure0)
    lab = label_rect[None]
    for col, (sure, maybe) in enumerate([(sure1 & lab, band & lab), (sure1 & ~lab, band & ~lab), (sure0 & lab, band & lab)]):
        lo = sure.flatten(1).sum(1)
        hi = lo + maybe.flatten(1).sum(1)
        ok = (lo <= c[:, col]) & (c[:, col] <= hi)
        assert bool(ok.all()), f"{what}: count {col} {c[:, col].tolist()} outside [{lo.tolist()}, {hi.tolist()}]"
