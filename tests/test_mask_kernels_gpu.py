"""GPU parity of the mask post-processing kernels - psam_mask_upsample / _union / _stats / _binarize and psam_plane_stats
(csrc/decoder.hip), psam_prob2_argmax, psam_scores_prob_argmax and psam_mask_union_seg (csrc/coarse_batch.hip), with their shared
up_sample / lin2 (csrc/interp.h) - one kernel at a time, against the float64 references of oracle/maskpost.py.

House rules (as in test_resample_kernels_gpu.py): every call goes through protosam_amd.ops; every output buffer is filled with NaN
(0xA5 bytes for integer buffers) before the call; bounds are c x 2^-23 x magnitude element-wise with the magnitude from the
reference; no flat tolerances. A kernel that thresholds is held to the float64 value wherever that value is further from the
threshold than the bound of the value ("surely 1" / "surely 0"); the pixels in between (the band) may go either way, and every case
asserts that they are at most 1e-4 of its pixels - tests/test_maskpost_reference_cpu.py shows on the CPU that the inputs allow it.
Counts must lie in [n(sure1), n(sure1) + n(band)], boxes between the box of sure1 and the box of sure1 | band; where the band is
empty, which is most planes, everything is exact.

The general cases threshold at 0.3 (0.5 for variant 3), not 0: see oracle/maskpost.py THRESHOLDS. Exact ties at thr = 0 are held by
the exact-arithmetic cases (integer logits at a power-of-two ratio), where every number of every kernel is exactly the reference's.

Shapes (IN, MID, H, W) = oracle.maskpost.CASES: the smallest at which each structure has an edge - odd sizes, H not a multiple of
the 32-row blocks, W below / above the 256-lane stride, a 1-row tail block (H = 289), dyadic and non-dyadic ratios, one input
sample, MID = 1 (align_corners scale 0) - and the production size 256 -> 1024, whole and cropped.

Worst ratios measured on an MI355X (profiles/mask_kernel_tests.txt, 163 tests in 11 s) are quoted in the docstrings.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import maskpost as M
from oracle import resample as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
NAN = float("nan")
FLOOR = 2.0 ** -126
C = M.C_BOUND
SIZES = sorted({c[:2] for c in M.CASES})
EXACT = [(16, 128), (64, 256)]
IDX = [6, 0, 3, 3, 7, 1, 5, 4, 2, 0]          # mask_binarize's candidates: repeats, out of order


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def _a5(shape, dev, dtype=torch.uint8):
    fill = {torch.uint8: 0xA5, torch.int32: -1515870811, torch.int64: -6510615555426900571}[dtype]
    return torch.full(shape, fill, dtype=dtype, device=dev)


def _within(out, ref, mag, c, what, floor=0.0):
    """|out - ref| <= c 2^-23 mag (+ floor) element-wise; returns the worst |out - ref| / (2^-23 mag)."""
    out = out.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(out).all()), f"{what}: {int((~torch.isfinite(out)).sum())} non-finite (unwritten?) elements"
    err = (out - ref).abs()
    ratio = (err - floor).clamp_min(0) / mag.clamp_min(1e-300)
    worst = ratio.max().item() / U
    bad = err > c * U * mag + floor
    if bool(bad.any()):
        i = tuple(int(k) for k in np.unravel_index(int(ratio.argmax()), ratio.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} elements off by more than {c} x 2^-23 x magnitude; worst {worst:.2f} at {i}: "
                             f"got {out[i].item():.9g}, reference {ref[i].item():.17g}, magnitude {mag[i].item():.6g}")
    print(f"RATIO {what}: worst |err| = {worst:.2f} x 2^-23 x magnitude (bound {c})")
    return worst


def _bits(out, sure1, sure0, what):
    """out is {0, 1}, 1 on sure1 and 0 on sure0; returns the number of band pixels."""
    o = out.detach().cpu().reshape(sure1.shape)
    assert bool(((o == 0) | (o == 1)).all()), f"{what}: values other than 0 / 1 (unwritten?)"
    n1, n0 = int((o[sure1] != 1).sum()), int((o[sure0] != 0).sum())
    assert n1 == 0 and n0 == 0, f"{what}: {n1} surely-set pixels clear, {n0} surely-clear pixels set"
    return sure1.numel() - int(sure1.sum()) - int(sure0.sum())


def _share(nband, n, what):
    print(f"BAND {what}: {nband} of {n} pixels inside the error band ({nband / n:.1e})")
    assert nband / n <= 1e-4, f"{what}: {nband / n:.2e} of the pixels inside the error band - the inputs do not test the kernel"


@functools.lru_cache(maxsize=None)
def _sure(IN, MID, variant, thr, off, sign):
    """(sure1, sure0, band) [NPLANES, MID, MID] of a case at one of its thresholds; computed once, shared, never modified."""
    _, v, mag = M.case_reference(IN, MID, variant, thr, off)
    return M.threshold(v, mag, M.thr32(thr, off, sign), C)


def _low4(x, B, nsel, first, Cn, dev, filler=77.0):
    """planes [B * nsel, IN, IN] as channels first .. first + nsel - 1 of low [B, Cn, IN, IN]; the other channels hold `filler`."""
    IN = x.shape[-1]
    low = torch.full((B, Cn, IN, IN), filler)
    low[:, first:first + nsel] = x.view(B, nsel, IN, IN)
    return low.contiguous().to(dev)


# ---- 1. psam_mask_upsample ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("IN,MID", SIZES)
def test_mask_upsample(dev, IN, MID, variant):
    """Variants 0, 1: |out - ref| <= 4 x 2^-23 x (blend + weights), the bound of the plane kernels. Variant 2: exact. Variant 3:
    4 x 2^-23 x (2 blend + weights) + 2^-126 on the sigmoid planes, with patches of +-100 and +-1e4 where the sigmoid saturates.
    Measured worst: 1.60 (variant 0), 1.50 (variant 1), 0.75 (variant 3), each at 64 -> 256; ATen's fp32 kernels on the CPU need 1.33 /
    0.73 of the same units on the same inputs."""
    from protosam_amd import ops
    thr, off = M.THRESHOLDS[variant][0]
    x, ref, mag = M.case_reference(IN, MID, variant, thr, off)
    out = _nan((M.NPLANES, MID, MID), dev)
    ops.mask_upsample(x.to(dev), MID, variant, out=out)
    what = f"mask_upsample variant {variant} {IN}->{MID}"
    if variant == 2:
        assert torch.equal(out.cpu().double(), ref), what
    else:
        _within(out, ref, mag, C, what, floor=FLOOR if variant == 3 else 0.0)


# ---- 2. exact arithmetic: every number of every kernel ------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("IN,MID", EXACT)
def test_exact_arithmetic_cases(dev, IN, MID, variant):
    """Integer logits in [-8, 8] at a power-of-two ratio: every weight is dyadic, every product and sum exact in fp32, so there is no
    band. mask_upsample is torch.equal to the reference; every mask, count and box of mask_stats, mask_binarize, mask_union and
    mask_union_seg at thr = 0, off = 1 is exactly the reference's, and the (many) pixels equal to thr are not set. Fails on any
    wrong index, weight, strict / non-strict comparison or reduction."""
    from protosam_amd import ops
    x = M.integer_planes(IN)
    P = x.shape[0]
    ref, _ = M.up_sample(x, MID, variant)
    zero = torch.zeros_like(ref)
    assert int((ref == 0).sum()) > 50
    xd = x.to(dev)
    out = _nan((P, MID, MID), dev)
    ops.mask_upsample(xd, MID, variant, out=out)
    assert torch.equal(out.cpu().double(), ref)
    H, W = MID - 3, MID - 1
    maps = [M.threshold(ref[:, :H, :W], zero[:, :H, :W], t, C) for t in (1.0, -1.0, 0.0)]
    assert not any(bool(m[2].any()) for m in maps)
    # mask_stats: planes as channels 1, 2 of [2, 4, IN, IN]
    stats = _a5((P, 8), dev, torch.int32)
    ops.mask_stats(_low4(x, 2, 2, 1, 4, dev), 1, 2, MID, H, W, variant, 0.0, 1.0, stats=stats)
    want = torch.cat([torch.stack([m[0].flatten(1).sum(1) for m in maps], 1), M.box(maps[2][0]), torch.zeros((P, 1), dtype=torch.long)], 1)
    assert torch.equal(stats.cpu().long(), want), f"mask_stats: {stats.cpu().tolist()} != {want.tolist()}"
    # mask_binarize
    idx = torch.tensor([3, 0, 2, 2, 1], dtype=torch.int32)
    label = (torch.rand((H, W), generator=torch.Generator().manual_seed(IN)) < 0.4).to(torch.uint8) * 255
    m = _a5((5, H, W), dev)
    m, counts = ops.mask_binarize(xd, idx.to(dev), MID, H, W, variant, 0.0, label=label.to(dev), out=m)
    wm = maps[2][0][idx.long()]
    assert torch.equal(m.cpu().bool(), wm) and int(m.max()) == 1
    lb = label.bool()
    wc = torch.stack([(wm & lb).flatten(1).sum(1), (wm & ~lb).flatten(1).sum(1), (~wm & lb).flatten(1).sum(1)], 1)
    assert torch.equal(counts.cpu(), wc)
    # mask_union / mask_union_seg: prompts 1..3 as channel 1 of [3, 2, IN, IN]
    s1, s0, _ = M.threshold(ref, zero, 0.0, C)
    low = _low4(x[1:4], 3, 1, 1, 2, dev)
    for OUT in M.union_outs(MID):
        u1 = M.union_fold(s1[1:4], s0[1:4], OUT)[0]
        pred = _nan((OUT, OUT), dev)
        ops.mask_union(low, 1, MID, OUT, variant, 0.0, pred=pred)
        assert torch.equal(pred.cpu(), u1.float()), f"mask_union OUT={OUT}"
        segs = torch.tensor([[0, 3, 1], [1, 1, 0]], dtype=torch.int32, device=dev)
        o = _a5((2, OUT, OUT), dev)
        ops.mask_union_seg(low, 1, segs, 2, MID, OUT, variant, 0.0, out=o)
        assert torch.equal(o[1].cpu().bool(), u1) and torch.equal(o[0].cpu().bool(), M.union_fold(s1[2:3], s0[2:3], OUT)[0])
        assert int(o.max()) <= 1


# ---- 3. psam_mask_binarize ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("IN,MID,H,W", M.CASES)
def test_mask_binarize(dev, IN, MID, H, W, variant):
    """out == 1 on sure1, == 0 on sure0, band share <= 1e-4; counts are exactly the {tp, fp, fn} of the mask the same call wrote
    against a label with the values 0, 1 and 255 (the kernel tests label != 0); idx has repeats and is out of order; without a
    label counts is None and the mask is the same bits. Measured: at most 5.2e-5 of the pixels inside the band (variant 1, 20 -> 77),
    none for variant 2."""
    from protosam_amd import ops
    thr, off = M.THRESHOLDS[variant][0]
    x = M.case_reference(IN, MID, variant, thr, off)[0]
    s1, s0, _ = _sure(IN, MID, variant, thr, off, 0)
    idx = torch.tensor(IDX, dtype=torch.int32)
    n = idx.numel()
    label = torch.tensor([0, 1, 255], dtype=torch.uint8)[torch.randint(0, 3, (H, W), generator=torch.Generator().manual_seed(H + W))]
    xd = x.to(dev)
    out = _a5((n, H, W), dev)
    out, counts = ops.mask_binarize(xd, idx.to(dev), MID, H, W, variant, thr, label=label.contiguous().to(dev), out=out)
    what = f"mask_binarize variant {variant} {IN}->{MID} [{H}x{W}]"
    nband = _bits(out, s1[idx.long(), :H, :W], s0[idx.long(), :H, :W], what)
    _share(nband, n * H * W, what)
    o, lb = out.cpu().bool(), label.bool()
    want = torch.stack([(o & lb).flatten(1).sum(1), (o & ~lb).flatten(1).sum(1), (~o & lb).flatten(1).sum(1)], 1)
    assert counts.dtype == torch.int64 and torch.equal(counts.cpu(), want), f"{what}: counts"
    assert torch.equal(out[1], out[9]) and torch.equal(out[2], out[3])
    out2 = _a5((n, H, W), dev)
    out2, none = ops.mask_binarize(xd, idx.to(dev), MID, H, W, variant, thr, out=out2)
    assert none is None and torch.equal(out2, out)


# ---- 4. psam_mask_stats -------------------------------------------------------------------------------------------------
def _check_stats(stats, maps, what):
    """stats int32 [P, 8] against (sure1, sure0, band) [P, H, W] at thr + off, thr - off, thr; returns the band pixels at thr."""
    st = stats.cpu().long()
    assert bool((st[:, 7] == 0).all()), f"{what}: column 7"
    exact = 0
    for col, (s1, s0, band) in enumerate(maps):
        lo, hi, inner, outer = M.counts_and_boxes(s1, band)
        ok = (lo <= st[:, col]) & (st[:, col] <= hi)
        assert bool(ok.all()), f"{what}: count {col} of planes {(~ok).nonzero().flatten().tolist()} outside [{lo.tolist()}, {hi.tolist()}]: {st[:, col].tolist()}"
        if col == 2:
            okb = M.box_between(st[:, 3:7], inner, outer)
            assert bool(okb.all()), f"{what}: box of planes {(~okb).nonzero().flatten().tolist()}: {st[:, 3:7].tolist()} not between {inner.tolist()} and {outer.tolist()}"
            empty = hi == 0
            assert torch.equal(st[empty, 2:7], torch.tensor([0, M.INT_MAX, M.INT_MAX, -1, -1]).expand(int(empty.sum()), 5))
            exact = int((lo == hi).sum())
    return exact


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("IN,MID,H,W", M.CASES)
def test_mask_stats(dev, IN, MID, H, W, variant):
    """Each of the three counts inside its interval, the box between the inner and the outer box, empty planes INT_MAX, INT_MAX, -1,
    -1 and three zeros, column 7 zero; first = 1 and nsel = 2 of C = 4 channels (the other channels hold 77, which would count).
    Once with off = 1 and once with off = 0, where the three counts must be equal. Most planes have no band pixel: there all seven
    numbers are exact. Measured: at most 3.2e-5 of the pixels inside the band (20 -> 77)."""
    from protosam_amd import ops
    for thr, off in M.THRESHOLDS[variant]:
        x = M.case_reference(IN, MID, variant, thr, off)[0]
        maps = [tuple(m[:, :H, :W] for m in _sure(IN, MID, variant, thr, off, sign)) for sign in (1, -1, 0)]
        stats = _a5((M.NPLANES, 8), dev, torch.int32)
        ops.mask_stats(_low4(x, 4, 2, 1, 4, dev), 1, 2, MID, H, W, variant, thr, off, stats=stats)
        what = f"mask_stats variant {variant} {IN}->{MID} [{H}x{W}] thr {thr} off {off}"
        exact = _check_stats(stats, maps, what)
        _share(max(int(m[2].sum()) for m in maps), M.NPLANES * H * W, what)
        assert exact >= M.NPLANES - 4, f"{what}: only {exact} planes without a band pixel"
        st = stats.cpu()
        assert st[M.EMPTY].tolist() == [0, 0, 0, M.INT_MAX, M.INT_MAX, -1, -1, 0]
        assert st[M.FULL].tolist() == [H * W, H * W, H * W, 0, 0, W - 1, H - 1, 0]
        if off == 0:
            assert torch.equal(st[:, 0], st[:, 1]) and torch.equal(st[:, 1], st[:, 2])


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_mask_stats_70_planes(dev, variant):
    """70 planes in one call (B = 10 prompts x nsel = 7 of C = 9 channels from first = 2) at 16 -> 64, H = 50, W = 64."""
    from protosam_amd import ops
    IN, MID, H, W, thr, off = 16, 64, 50, 64, 0.3, 1.0
    x = M.planes70(variant, thr, off)
    v, mag = M.up_sample(x, MID, variant)
    maps = [M.threshold(v[:, :H, :W], mag[:, :H, :W], M.thr32(thr, off, sign), C) for sign in (1, -1, 0)]
    stats = _a5((70, 8), dev, torch.int32)
    ops.mask_stats(_low4(x, 10, 7, 2, 9, dev), 2, 7, MID, H, W, variant, thr, off, stats=stats)
    what = f"mask_stats 70 planes variant {variant}"
    exact = _check_stats(stats, maps, what)
    _share(max(int(m[2].sum()) for m in maps), 70 * H * W, what)
    assert exact >= 35
    assert stats[13].tolist() == [0, 0, 0, M.INT_MAX, M.INT_MAX, -1, -1, 0] and stats[69].tolist() == [H * W] * 3 + [0, 0, W - 1, H - 1, 0]


# ---- 5. psam_plane_stats ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr,off", [(0.0, 1.0), (0.3, 0.25), (0.3, 0.0)])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 257), (31, 33), (32, 32), (33, 31), (257, 1), (33, 257), (257, 32)])
def test_plane_stats(dev, H, W, thr, off):
    """Materialised planes: everything is exactly the fp32 comparison, with or without the uint8 output. Non-square planes with H,
    W in {1, 31, 32, 33, 257}; values planted exactly at thr, thr + off and thr - off (none of them counts: the comparisons are
    strict) and one fp32 step above each; +-inf; a NaN plane (all counts 0, box empty); 0.3 is not representable."""
    from protosam_amd import ops
    g = torch.Generator().manual_seed(H * 1000 + W)
    t = [np.float32(M.thr32(thr, off, s)) for s in (1, -1, 0)]
    n = 6
    x = torch.randn((n, H, W), generator=g) * 1.5
    planted = torch.tensor([float(v) for tk in t for v in (tk, np.nextafter(tk, np.float32(9)), np.nextafter(tk, np.float32(-9)))] +
                           [float("inf"), float("-inf")], dtype=torch.float32)
    flat = x[0].view(-1)
    pos = torch.randperm(H * W, generator=g)[:planted.numel()]
    flat[pos] = planted[:pos.numel()]
    x[1] = torch.from_numpy(np.full((H, W), t[2]))                     # everywhere exactly thr: nothing above thr
    x[2] = NAN
    x[3] = float("-inf")
    x[3, H - 1, W - 1] = float("inf")
    x[4] = torch.from_numpy(np.full((H, W), t[0]))                     # exactly thr + off: above thr (off > 0), not above thr + off
    want = []
    for p in range(n):
        m = [x[p] > float(tk) for tk in t]
        want.append([int(m[0].sum()), int(m[1].sum()), int(m[2].sum())] + M.box(m[2]).tolist() + [0])
    want = torch.tensor(want)
    assert want[2].tolist() == [0, 0, 0, M.INT_MAX, M.INT_MAX, -1, -1, 0] and want[1, 2] == 0 and want[4, 0] == 0
    assert want[3].tolist() == [1, 1, 1, W - 1, H - 1, W - 1, H - 1, 0]
    xd = x.to(dev)
    stats, out = _a5((n, 8), dev, torch.int32), _a5((n, H, W), dev)
    ops.plane_stats(xd, thr, off, stats=stats, out=out)
    assert torch.equal(stats.cpu().long(), want), f"plane_stats {H}x{W}: {stats.cpu().tolist()} != {want.tolist()}"
    assert torch.equal(out.cpu(), (x > float(t[2])).to(torch.uint8))
    stats2 = _a5((n, 8), dev, torch.int32)
    _, none = ops.plane_stats(xd, thr, off, binarize=False, stats=stats2)
    assert none is None and torch.equal(stats2, stats)


# ---- 6. psam_mask_union, psam_mask_union_seg ----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("IN,MID", SIZES)
def test_mask_union_and_seg(dev, IN, MID, variant):
    """B in {1, 3} prompts (sel = 1 of C = 3 channels; the other channels hold 77), OUT in {MID, MID / 2, an odd size above MID, 1},
    all four variants (threshold 0.5 for variant 3): surely-1 and surely-0 pixels exact, for mask_union (fp32 {0, 1}) and for
    mask_union_seg (uint8, one table with the B = 1 and the B = 3 segment; the outputs at OUT % 4 == 0 once more through a view
    that starts one byte into its storage: the per-pixel store path). The band share, pooled over B and OUT, is <= 1e-4 (measured: at
    most 5.6e-5, variant 1 at 20 -> 77)."""
    from protosam_amd import ops
    thr, off = M.THRESHOLDS[variant][0]
    x = M.case_reference(IN, MID, variant, thr, off)[0]
    s1, s0, _ = _sure(IN, MID, variant, thr, off, 0)
    p1, p3 = list(M.UNION_PROMPTS[1]), list(M.UNION_PROMPTS[3])
    low = _low4(x[p1 + p3], 4, 1, 1, 3, dev)                          # prompts 0 | 1 2 3
    segs = torch.tensor([[1, 3, 0], [0, 1, 2]], dtype=torch.int32, device=dev)
    nband = npix = 0
    for OUT in M.union_outs(MID):
        what = f"variant {variant} {IN}->{MID}->{OUT}"
        refs = {1: M.union_fold(s1[p1], s0[p1], OUT), 3: M.union_fold(s1[p3], s0[p3], OUT)}
        for B, lo4 in ((1, low[:1]), (3, low[1:])):
            pred = _nan((OUT, OUT), dev)
            ops.mask_union(lo4.contiguous(), 1, MID, OUT, variant, thr, pred=pred)
            nband += _bits(pred, refs[B][0], refs[B][1], f"mask_union B={B} {what}")
            npix += OUT * OUT
        for shift in ((0, 1) if OUT % 4 == 0 else (0,)):
            buf = _a5((3 * OUT * OUT + shift,), dev)
            o = buf[shift:].view(3, OUT, OUT)
            ops.mask_union_seg(low, 1, segs, 3, MID, OUT, variant, thr, out=o)
            _bits(o[0], refs[3][0], refs[3][1], f"mask_union_seg B=3 shift {shift} {what}")
            _bits(o[2], refs[1][0], refs[1][1], f"mask_union_seg B=1 shift {shift} {what}")
            assert bool((o[1] == 0xA5).all()) and bool((buf[:shift] == 0xA5).all()), f"mask_union_seg {what}: wrote an output no segment names"
    _share(nband, npix, f"mask_union variant {variant} {IN}->{MID}")


def test_mask_union_seg_table(dev):
    """The segment table, with the output pre-filled with 0xA5: a count of 0 writes zeros; rows with first < 0, first + count > Pm,
    o < 0 or o >= nout are skipped and leave their target untouched; an output no row names stays 0xA5; a row that ends exactly at
    Pm is not skipped; Pm = 0 with low = None. OUT is odd."""
    from protosam_amd import ops
    IN, MID, OUT, variant, thr = 16, 64, 37, 0, 0.3
    x = M.case_reference(IN, MID, variant, thr, 1.0)[0]
    s1, s0, _ = _sure(IN, MID, variant, thr, 1.0, 0)
    order = [0, 1, 7, M.ISLAND]
    low = _low4(x[order], 4, 1, 1, 2, dev)                            # Pm = 4
    ref = lambda a, b: M.union_fold(s1[order[a:b]], s0[order[a:b]], OUT)  # noqa: E731
    #        zeros      first<0     past Pm     o<0         o>=nout    ends at Pm  plain       count<0
    table = [(2, 0, 0), (-1, 2, 1), (3, 2, 2), (0, 1, -1), (0, 1, 8), (2, 2, 3), (0, 2, 4), (1, -1, 5)]
    nout = 8
    out = _a5((nout, OUT, OUT), dev)
    ops.mask_union_seg(low, 1, torch.tensor(table, dtype=torch.int32, device=dev), nout, MID, OUT, variant, thr, out=out)
    assert int(out[0].count_nonzero()) == 0, "a count of 0 must write zeros"
    for o in (1, 2, 5, 6, 7):
        assert bool((out[o] == 0xA5).all()), f"output {o} was written"
    assert _bits(out[3], *ref(2, 4)[:2], "segment ending at Pm") == 0 and _bits(out[4], *ref(0, 2)[:2], "plain segment") == 0
    assert 0 < int(out[3].sum()) < OUT * OUT
    out = _a5((2, OUT, OUT), dev)
    ops.mask_union_seg(None, 0, torch.tensor([(0, 0, 1), (0, 1, 0)], dtype=torch.int32, device=dev), 2, MID, OUT, variant, thr, out=out)
    assert int(out[1].count_nonzero()) == 0 and bool((out[0] == 0xA5).all())


def test_mask_union_seg_workgroups_straddle_segments(dev):
    """OUT = 1025 with 5 segments: a row is two work items, 10250 items go to 2048 workgroups in runs of six (pb_grid, restated in
    oracle/maskpost.py), so workgroups walk across segment boundaries - between written, skipped and zero-count segments."""
    from protosam_amd import ops
    IN, MID, OUT, variant, thr = 16, 64, 1025, 0, 0.3
    assert M.pb_grid(5 * OUT * 2) == (1709, 6) and M.pb_straddlers(OUT, OUT, 5) >= 1
    x = M.case_reference(IN, MID, variant, thr, 1.0)[0]
    s1, s0, _ = _sure(IN, MID, variant, thr, 1.0, 0)
    order = [0, 1, 7, M.ISLAND]
    low = _low4(x[order], 4, 1, 1, 2, dev)
    table = [(0, 2, 4), (3, 2, 1), (1, 3, 0), (0, 0, 2), (3, 1, 5)]
    out = _a5((6, OUT, OUT), dev)
    ops.mask_union_seg(low, 1, torch.tensor(table, dtype=torch.int32, device=dev), 6, MID, OUT, variant, thr, out=out)
    nband = 0
    for a, b, o in ((0, 2, 4), (1, 4, 0), (3, 4, 5)):
        r = M.union_fold(s1[order[a:b]], s0[order[a:b]], OUT)
        nband += _bits(out[o], r[0], r[1], f"segment {a}:{b}")
    _share(nband, 3 * OUT * OUT, "mask_union_seg OUT=1025")
    assert int(out[2].count_nonzero()) == 0 and bool((out[1] == 0xA5).all()) and bool((out[3] == 0xA5).all())


# ---- 7. psam_prob2_argmax, psam_scores_prob_argmax ----------------------------------------------------------------------
def _check_classes(case, v, mag, prob, pred, fg, seed, pfg2, what):
    """prob as in test_prob_argmax: 8 x 2^-23 x p (1 + M0 + M1) + 2^-126. pred: the float64 argmax wherever the float64 margin exceeds
    4 x 2^-23 (M0 + M1), class 0 on exact ties, band share <= 1e-4. pfg2: 8 x 2^-23 x q1 (1 + (1 - q1)(1 + M)): the derivative of
    sigma(p1 - p0), q1 (1 - q1), times prob's bound, plus the roundings of the second softmax itself. fg_sum: onto its seed,
    exactly pred.sum() per plane."""
    P, OH, OW = case[0], case[-2], case[-1]
    v, mag = v.view(P, 2, OH, OW), mag.view(P, 2, OH, OW)
    Mm = mag[:, 0] + mag[:, 1]
    p0, p1, am, margin, q1 = M.softmax2_twice(v[:, 0], v[:, 1])
    if prob is not None:
        pref = torch.stack([p0, p1], 1)
        _within(prob, pref, pref * (1.0 + Mm[:, None]), 8, f"{what} prob", floor=FLOOR)
    if pfg2 is not None:
        _within(pfg2, q1, q1 * (1.0 + (1.0 - q1) * (1.0 + Mm)), 8, f"{what} pfg2", floor=FLOOR)
    predc = pred.cpu()
    assert bool((predc <= 1).all()), f"{what}: labels other than 0 / 1 (unwritten?)"
    tie, sure, share = M.argmax_band(margin, Mm)
    print(f"BAND {what}: {share:.1e} of the untied pixels inside the error band, {int(tie.sum())} exact ties")
    assert share <= 1e-4 and int(tie.sum()) >= OH * OW
    assert torch.equal(predc[sure], am[sure]), f"{what}: {int((predc[sure] != am[sure]).sum())} labels differ outside the band"
    assert int(predc[tie].sum()) == 0, f"{what}: a tie went to class 1"
    assert torch.equal(fg.cpu() - seed, predc.view(P, -1).sum(1, dtype=torch.int32)), f"{what}: fg_sum"
    assert int(fg[-1].cpu() - seed[-1]) == 0 or P < 3


@pytest.mark.parametrize("case", M.PROB2_CASES, ids=lambda c: "-".join(map(str, c)))
def test_prob2_argmax(dev, case):
    """psam_prob2_argmax against float64: see _check_classes. The tuples of test_prob2_argmax_equals_chain, plus P = 9 planes of 301 x
    1100 from 40 x 50: two items per row, 602 per plane, three per workgroup, so workgroups straddle plane boundaries (asserted from
    the restated pb_grid). With and without `prob`: the other outputs are the same bits. Measured worst: prob 2.85 (64 x 52
    same-size), pfg2 0.80; at most 7.6e-7 of the pixels inside the band."""
    from protosam_amd import ops
    P, IH, IW, OH, OW = case
    if P == 9:
        assert M.pb_grid(P * OH * 2) == (1806, 3) and M.pb_straddlers(OH, OW, P) >= 4
    l = M.case_scores(case)
    if (IH, IW) == (OH, OW):
        v, mag = l.view(2 * P, IH, IW).double(), torch.zeros((2 * P, OH, OW), dtype=torch.float64)
    else:
        v, blend, weights = R.bilinear(l.view(2 * P, IH, IW), OH, OW)
        mag = blend + weights
    ld = l.to(dev)
    seed = torch.tensor([1000 + 37 * p for p in range(P)], dtype=torch.int32)
    pred, pfg2, prob, fg = _a5((P, OH, OW), dev), _nan((P, OH, OW), dev), _nan((P, 2, OH, OW), dev), seed.clone().to(dev)
    ops.prob2_argmax(ld, OH, OW, pred=pred, pfg2=pfg2, fg_sum=fg, prob=prob)
    _check_classes(case, v, mag, prob, pred, fg, seed, pfg2, f"prob2_argmax {case}")
    pred2, pfg22, fg2 = _a5((P, OH, OW), dev), _nan((P, OH, OW), dev), seed.clone().to(dev)
    ops.prob2_argmax(ld, OH, OW, pred=pred2, pfg2=pfg22, fg_sum=fg2)
    assert torch.equal(pred2, pred) and torch.equal(pfg22, pfg2) and torch.equal(fg2, fg)


@pytest.mark.parametrize("case", M.SCORES_CASES, ids=lambda c: "-".join(map(str, c)))
def test_scores_prob_argmax(dev, case):
    """psam_scores_prob_argmax against the composed-resize reference (grid -> image size -> output, float64 throughout): non-square
    grids and images, the (IH, IW) == (OH, OW) path and the second-resize path, odd OW, and the plane-straddling shape on both
    paths. Measured worst: prob 1.24; at most 3.4e-6 of the pixels inside the band."""
    from protosam_amd import ops
    P, GH, GW, IH, IW, OH, OW = case
    if P == 9:
        assert M.pb_straddlers(OH, OW, P) >= 4
    l = M.case_scores(case)
    v, mag = M.composed_resize(l.view(2 * P, GH, GW), IH, IW, OH, OW)
    seed = torch.tensor([5 + 3 * p for p in range(P)], dtype=torch.int32)
    prob, pred, fg = _nan((P, 2, OH, OW), dev), _a5((P, OH, OW), dev), seed.clone().to(dev)
    ops.scores_prob_argmax(l.to(dev), IH, IW, OH, OW, prob=prob, pred=pred, fg_sum=fg)
    _check_classes(case, v, mag, prob, pred, fg, seed, None, f"scores_prob_argmax {case}")


# ---- 8. arguments -------------------------------------------------------------------------------------------------------
def test_rejections_return_status_1_before_any_launch(dev):
    """Each status-1 condition of the kernels' argument checks comes back before any launch, with the output still holding its
    pre-fill: variant out of range, first + nsel > C, H > MID (and W > MID), off < 0, sel >= C (and sel < 0). A label without counts
    cannot be expressed through ops, which allocates the counts itself."""
    from protosam_amd import ops
    f32 = lambda *s: torch.ones(s, dtype=torch.float32, device=dev)  # noqa: E731
    low, idx = f32(2, 3, 8, 8), torch.zeros(2, dtype=torch.int32, device=dev)
    segs = torch.tensor([[0, 1, 0]], dtype=torch.int32, device=dev)
    cases = []

    def case(name, fn, *outs):
        cases.append((name, fn, outs))

    o = _nan((6, 16, 16), dev)
    case("mask_upsample variant 4", lambda o=o: ops.mask_upsample(low, 16, 4, out=o), o)
    case("mask_upsample variant -1", lambda o=o: ops.mask_upsample(low, 16, -1, out=o), o)
    o = _nan((16, 16), dev)
    case("mask_union variant 4", lambda o=o: ops.mask_union(low, 1, 16, 16, 4, pred=o), o)
    case("mask_union sel = C", lambda o=o: ops.mask_union(low, 3, 16, 16, 0, pred=o), o)
    case("mask_union sel < 0", lambda o=o: ops.mask_union(low, -1, 16, 16, 0, pred=o), o)
    o = _a5((1, 16, 16), dev)
    case("mask_union_seg variant 4", lambda o=o: ops.mask_union_seg(low, 1, segs, 1, 16, 16, 4, 0.0, out=o), o)
    case("mask_union_seg sel = C", lambda o=o: ops.mask_union_seg(low, 3, segs, 1, 16, 16, 0, 0.0, out=o), o)
    o = _a5((4, 8), dev, torch.int32)
    case("mask_stats variant 3", lambda o=o: ops.mask_stats(low, 0, 2, 16, 16, 16, 3, stats=o), o)
    case("mask_stats first + nsel > C", lambda o=o: ops.mask_stats(low, 2, 2, 16, 16, 16, 0, stats=o), o)
    case("mask_stats first < 0", lambda o=o: ops.mask_stats(low, -1, 2, 16, 16, 16, 0, stats=o), o)
    case("mask_stats H > MID", lambda o=o: ops.mask_stats(low, 0, 2, 16, 17, 16, 0, stats=o), o)
    case("mask_stats W > MID", lambda o=o: ops.mask_stats(low, 0, 2, 16, 16, 17, 0, stats=o), o)
    case("mask_stats off < 0", lambda o=o: ops.mask_stats(low, 0, 2, 16, 16, 16, 0, 0.0, -0.5, stats=o), o)
    o = _a5((2, 17, 17), dev)
    case("mask_binarize variant 3", lambda o=o: ops.mask_binarize(low, idx, 16, 16, 16, 3, out=o), o)
    case("mask_binarize H > MID", lambda o=o: ops.mask_binarize(low, idx, 16, 17, 16, 0, out=o), o)
    case("mask_binarize W > MID", lambda o=o: ops.mask_binarize(low, idx, 16, 16, 17, 0, out=o), o)
    s, o = _a5((6, 8), dev, torch.int32), _a5((6, 8, 8), dev)
    case("plane_stats off < 0", lambda s=s, o=o: ops.plane_stats(low.view(6, 8, 8), 0.0, -1.0, stats=s, out=o), s, o)
    for name, fn, outs in cases:
        with pytest.raises(RuntimeError, match="status 1"):
            fn()
        torch.cuda.synchronize()
        for t in outs:
            if t.dtype.is_floating_point:
                assert bool(t.isnan().all()), f"{name}: output written"
            else:
                assert bool((t.view(torch.uint8) == 0xA5).all()), f"{name}: output written"
    print(f"{len(cases)} rejections, each status 1 with its outputs untouched")
