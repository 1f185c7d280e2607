"""CPU: tests/amg_resize_reference.py, what tests/test_amg_resize_gpu.py holds psam_mask_stats_resized / psam_mask_binarize_resized
to. (1) the float64 two-stage reference against stock F.interpolate applied twice in fp32; (2) the inputs leave at most 1e-4 of a
case's pixels inside the error band at the thresholds the kernels compare with; (3) each injected fault fails the checks the GPU
file applies; plus the generator's PSAM_AMG_RESIZE switch and path choice, which need no GPU.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import amg_resize_reference as rr
from oracle import maskpost as M

MODES = {0: dict(mode="bilinear", align_corners=False), 1: dict(mode="bilinear", align_corners=True), 2: dict(mode="nearest")}


@pytest.mark.parametrize("variant", rr.VARIANTS)
@pytest.mark.parametrize("case", rr.CASES)
def test_reference_vs_torch_twice(case, variant):
    """F.interpolate IN -> MID, crop to ih x iw, F.interpolate -> OH x OW, both fp32 in the variant's mode (the second skipped when it
    changes nothing, as postprocess_masks skips it): within C_BOUND x 2^-23 x magnitude of the reference at every pixel; nearest
    copies values, so there the two are equal."""
    IN, MID, ih, iw, OH, OW = case
    x, v, m = rr.case_reference(case, variant)
    t = F.interpolate(x[None], size=(MID, MID), **MODES[variant])[..., :ih, :iw]
    if (ih, iw) != (OH, OW):
        t = F.interpolate(t, size=(OH, OW), **MODES[variant])
    t = t[0].double()
    err = (t - v).abs()
    bad = err > rr.C_BOUND * rr.U * m
    worst = float((err / m.clamp_min(1e-300)).max()) / rr.U if variant != 2 else 0.0
    print(f"RATIO two-stage reference vs torch, case {case} variant {variant}: worst {worst:.2f} x 2^-23 x magnitude")
    assert not bool(bad.any()), f"{int(bad.sum())} pixels off by more than {rr.C_BOUND} x 2^-23 x magnitude, worst {worst:.2f}"
    if variant == 2:
        assert torch.equal(t, v) and not bool(m.any())
    # the poison plane: nothing of the padding arrives
    assert not bool(v[rr.POISON].any()) and not bool(t[rr.POISON].any())


@pytest.mark.parametrize("variant", rr.VARIANTS)
@pytest.mark.parametrize("case", rr.CASES)
def test_band_share(case, variant):
    """At thr32(0.3, 1.0, +1 / -1 / 0) at most 1e-4 of the pixels lie inside the error band; the empty plane is surely empty and the
    full plane surely full; nearest has no band at all. Measured: worst 6.9e-5, (64, 256, 200, 256, 50, 64) at variant 0."""
    share = rr.band_share(case, variant)
    print(f"BAND case {case} variant {variant}: {share:.1e} of the pixels inside the error band")
    assert share <= 1e-4
    if variant == 2:
        assert share == 0.0
    for s1, s0, _ in rr.sure_maps(case, variant):
        assert bool(s0[M.EMPTY].all()) and bool(s1[M.FULL].all())
    s1, s0, _ = rr.sure_maps(case, variant)[2]
    assert bool(s0[rr.POISON].all())                                   # the poison plane is surely empty at thr


def _run_checks(case, variant, stats, frames, y0, x0):
    maps = rr.sure_maps(case, variant)
    rr.check_stats(stats, maps, "model")
    rr.check_frames(frames, maps[2][0], maps[2][1], y0, x0, "model")


@pytest.mark.parametrize("variant", rr.VARIANTS)
@pytest.mark.parametrize("case", rr.CASES)
def test_unfaulted_model_passes(case, variant):
    """A kernel that computes exactly the float64 value passes the GPU file's checks (so a failure below is the fault's)."""
    _, v, _ = rr.case_reference(case, variant)
    stats, frames = rr.model_outputs(v, 3, 5, v.shape[1] + 7, v.shape[2] + 9)
    _run_checks(case, variant, stats, frames, 3, 5)


def _fails(case, variant, fault):
    x = rr.inputs(case, variant)
    v, _ = rr.two_stage(x, *case[1:], variant, fault=fault)
    stats, frames = rr.model_outputs(v, 3, 5, v.shape[1] + 7, v.shape[2] + 9)
    try:
        _run_checks(case, variant, stats, frames, 3, 5)
    except AssertionError:
        return True
    return False


def test_injected_faults():
    """Each fault, injected into the float64 model of the kernels, fails the checks of the GPU file on the cases where it can show:
    a second-stage clamp at MID instead of ih / iw (variant 0, the three up-scaling cases with padding); ih and iw swapped (every
    case with ih != iw); align_corners dropped from one stage (variant 1); a nearest index off by one (variant 2); the placement offset ignored;
    `>=` for `>` on a plane of exact ties (nearest, where the value is a copy)."""
    padded = [c for c in rr.CASES if c[2] < c[1] or c[3] < c[1]]
    assert len(padded) == 5
    # the neighbour tap past ih - 1 / iw - 1 carries weight only where a source coordinate exceeds ih - 1 / iw - 1: variant 0
    # (align_corners=True ends exactly on the last sample) when that axis is up-scaled and has padding behind it
    shows = [c for c in padded if (c[2] < c[1] and c[4] > c[2]) or (c[3] < c[1] and c[5] > c[3])]
    assert len(shows) == 3
    for case in shows:
        assert _fails(case, 0, "clamp_mid"), (case, "clamp_mid")
    for case in padded:
        for variant in rr.VARIANTS:
            assert _fails(case, variant, "swap_ih_iw"), (case, variant, "swap_ih_iw")
    for case in rr.CASES:
        assert _fails(case, 1, "drop_align_stage1"), (case, "drop_align_stage1")
        assert _fails(case, 2, "nearest_off_by_one"), (case, "nearest_off_by_one")
        if case[2:4] != case[4:6]:
            assert _fails(case, 1, "drop_align_stage2"), (case, "drop_align_stage2")
    for case in rr.CASES:
        for variant in rr.VARIANTS:
            _, v, _ = rr.case_reference(case, variant)
            maps = rr.sure_maps(case, variant)
            _, frames = rr.model_outputs(v, 3, 5, v.shape[1] + 7, v.shape[2] + 9, place=False)
            with pytest.raises(AssertionError):
                rr.check_frames(frames, maps[2][0], maps[2][1], 3, 5, "placement ignored")
    for case in rr.CASES:
        IN, MID, ih, iw, OH, OW = case
        tie = rr.tie_plane(IN)[None]
        v, m = rr.two_stage(tie, MID, ih, iw, OH, OW, 2)
        maps = [M.threshold(v, m, M.thr32(rr.THR, rr.OFF, sign), rr.C_BOUND) for sign in (1, -1, 0)]
        assert bool(maps[2][1].all())                                  # an exact tie with magnitude 0 is surely clear
        rr.check_stats(rr.model_outputs(v)[0], maps, "tie plane")
        with pytest.raises(AssertionError):
            rr.check_stats(rr.model_outputs(v, ge=True)[0], maps, "tie plane, >=")


def test_switch_and_paths(monkeypatch):
    """PSAM_AMG_RESIZE is read in the constructor: `fused` (default) takes every image without crop layers and small-region removal
    on the fused path, `materialise` only those at the model's size; anything else is a ValueError. `_fast_path` keeps its meaning
    (at the model's size: what SamWrapper.forward_batch chains its kernels behind)."""
    from protosam_amd.segment_anything import SamAutomaticMaskGenerator, sam_model_registry
    sam = sam_model_registry["vit_b"](encoder_depth=1)
    small, big = np.zeros((48, 44, 3), np.uint8), np.zeros((1024, 768, 3), np.uint8)
    monkeypatch.delenv("PSAM_AMG_RESIZE", raising=False)
    g = SamAutomaticMaskGenerator(sam, points_per_side=4)
    assert g.amg_resize == "fused" and g._fused_path(small) and g._fused_path(big)
    assert g._fast_path(big) and not g._fast_path(small)
    assert g._input_size(48, 44) == (1024, 939) and g._input_size(1024, 768) == (1024, 768) and g._input_size(700, 1100) == (652, 1024)
    for kw in (dict(crop_n_layers=1), dict(min_mask_region_area=6)):
        assert not SamAutomaticMaskGenerator(sam, points_per_side=4, **kw)._fused_path(small)
    monkeypatch.setenv("PSAM_AMG_RESIZE", "materialise")
    g = SamAutomaticMaskGenerator(sam, points_per_side=4)
    assert g.amg_resize == "materialise" and not g._fused_path(small) and g._fused_path(big)
    monkeypatch.setenv("PSAM_AMG_RESIZE", "fuse")
    with pytest.raises(ValueError, match="PSAM_AMG_RESIZE"):
        SamAutomaticMaskGenerator(sam, points_per_side=4)
    assert os.environ["PSAM_AMG_RESIZE"] == "fuse"
