"""GPU: the device RLE codec (`psam_rle_count` / `_write` / `_decode` behind `ops.rle_encode` / `ops.rle_decode`), the helpers on
top of it (`mask_to_rle_pytorch`, `rle_to_mask_device`) and the generator's RLE output, against the host
`utils.amg.mask_to_rle` / `rle_to_mask` (pinned by tests/test_amg_cpu.py). Every comparison is exact: each count list and each
decoded pixel.

Shapes are the smallest at which each mechanism can go wrong: one pixel / one row / one column; W % 4 != 0 (byte loads) and
W % 4 == 0 (32-bit loads, four columns per lane); H odd and past one 64-row cell; more columns than one strip of the
workgroup holds (64 lanes x 1 or 4 columns) with a ragged last strip, on both load paths; one realistic 1024 x 1024 batch."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from protosam_amd.segment_anything.utils import amg

pytestmark = pytest.mark.gpu

SEG = 64                                                            # rows of a cell (RLE_SEG of csrc/rle.hip)
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 3),
          (64, 65), (48, 44),                                       # byte path
          (63, 64), (257, 132), (129, 4),                           # 32-bit path, H odd, H across cells
          (300, 1030),                                              # byte path, 17 strips, the last one 6 columns
          (70, 520)]                                                # 32-bit path, 3 strips, the last one 2 lanes


def _patterns(H, W, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    b = SEG if H > SEG + 1 else max(1, H // 2)                      # a cell boundary where the shape has one
    out = {
        "zeros": np.zeros((H, W), bool),
        "ones": np.ones((H, W), bool),
        "rand_0.02": rng.random((H, W)) < 0.02,
        "rand_0.5": rng.random((H, W)) < 0.5,
        "first_pixel": (y == 0) & (x == 0),
        "last_pixel": (y == H - 1) & (x == W - 1),
        "vertical_stripes": x % 2 == 1,                             # every transition at y == 0: the column-boundary rule
        "vertical_stripes_set_first": x % 2 == 0,
        "vertical_stripes_3": (x // 3) % 2 == 1,
        "horizontal_stripes": y % 2 == 1,
        "horizontal_stripes_5": (y // 5) % 2 == 0,
        "checkerboard": (x + y) % 2 == 0,                           # first pixel set; H odd: H * W + 1 counts
        "step_on_boundary": y >= b,
        "step_below_boundary": y >= b + 1,
        "step_above_boundary": y >= b - 1,
        "band_to_boundary": (y >= b // 2) & (y < b),
    }
    return out


def _host_counts(m):
    return amg.mask_to_rle(np.asarray(m, dtype=bool))["counts"]


def _split(counts, offsets):
    c, o = counts.cpu().numpy(), offsets.cpu().numpy()
    return [c[o[i]:o[i + 1]].tolist() for i in range(len(o) - 1)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_encode_decode_patterns(dev, H, W):
    from protosam_amd import ops
    pats = _patterns(H, W, seed=H * 1000 + W)
    names = list(pats)
    host = np.stack([pats[k] for k in names])
    ref = [_host_counts(m) for m in host]
    masks = torch.from_numpy(host.astype(np.uint8)).to(dev)
    counts, offsets = ops.rle_encode(masks)
    assert counts.dtype == torch.int32 and offsets.dtype == torch.int64 and counts.is_cuda and offsets.is_cuda
    assert offsets.cpu().tolist() == np.concatenate([[0], np.cumsum([len(r) for r in ref])]).tolist()
    got = _split(counts, offsets)
    for k, g, r in zip(names, got, ref):
        assert g == r, (k, H, W, len(g), len(r))
    assert got[names.index("ones")] == [0, H * W] and got[names.index("zeros")] == [H * W]
    if H % 2 == 1:
        assert len(got[names.index("checkerboard")]) == H * W + 1   # the longest list a mask can have
    dec = ops.rle_decode(counts, offsets, H, W)
    assert dec.dtype == torch.uint8 and tuple(dec.shape) == (len(names), H, W)
    assert torch.equal(dec, masks)
    # one mask at a time (n = 1, [H, W] input) gives the same lists
    for k in ("rand_0.5", "checkerboard"):
        i = names.index(k)
        c1, o1 = ops.rle_encode(masks[i])
        assert o1.cpu().tolist() == [0, len(ref[i])] and c1.cpu().tolist() == ref[i]


def test_batch_offsets_and_empty_mask_in_the_middle(dev):
    from protosam_amd import ops
    rng = np.random.default_rng(2)
    H, W = 130, 68
    host = np.stack([rng.random((H, W)) < 0.5, np.zeros((H, W), bool), (np.arange(H)[:, None] >= 100) & np.ones((1, W), bool)])
    ref = [_host_counts(m) for m in host]
    assert len(ref[0]) > 1000 and ref[1] == [H * W] and len(ref[2]) == 2 * W
    counts, offsets = ops.rle_encode(torch.from_numpy(host).to(dev))
    assert offsets.cpu().tolist() == np.concatenate([[0], np.cumsum([len(r) for r in ref])]).tolist()
    assert _split(counts, offsets) == ref
    assert torch.equal(ops.rle_decode(counts, offsets, H, W).bool().cpu(), torch.from_numpy(host))


def test_input_forms(dev):
    """bool input; uint8 input whose set pixels are 2 and 255; a non-contiguous slice."""
    from protosam_amd import ops
    rng = np.random.default_rng(3)
    for H, W in ((37, 52), (37, 51)):                               # both load paths
        m = rng.random((3, H, W)) < 0.4
        ref = [_host_counts(v) for v in m]
        b = torch.tensor(m).to(dev)
        assert _split(*ops.rle_encode(b)) == ref
        u = torch.from_numpy(m.astype(np.uint8) * np.where(rng.random((3, H, W)) < 0.5, 2, 255).astype(np.uint8)).to(dev)
        assert set(u.unique().cpu().tolist()) == {0, 2, 255}
        assert _split(*ops.rle_encode(u)) == ref
        big = torch.zeros((3, H + 5, 2 * W + 3), dtype=torch.uint8, device=dev)
        big[:, 2:2 + H, 3:3 + 2 * W:2] = u
        view = big[:, 2:2 + H, 3:3 + 2 * W:2]
        assert not view.is_contiguous()
        assert _split(*ops.rle_encode(view)) == ref
        off1 = big.view(-1)[1:1 + 3 * H * W].view(3, H, W)          # contiguous, but its base is 1 byte off a word
        off1.copy_(u)
        assert _split(*ops.rle_encode(off1)) == ref
    with pytest.raises(TypeError):
        ops.rle_encode(torch.zeros((1, 4, 4), dtype=torch.float32, device=dev))
    c, o = ops.rle_encode(torch.zeros((0, 4, 4), dtype=torch.uint8, device=dev))
    assert c.numel() == 0 and o.cpu().tolist() == [0]


def test_encode_is_deterministic(dev):
    from protosam_amd import ops
    rng = np.random.default_rng(4)
    masks = torch.from_numpy(rng.random((5, 257, 132)) < 0.3).to(dev)
    c1, o1 = ops.rle_encode(masks)
    c2, o2 = ops.rle_encode(masks)
    assert torch.equal(c1, c2) and torch.equal(o1, o2)


@pytest.fixture(scope="module")
def blobs():
    """Four blob-shaped 1024 x 1024 masks (the first with its first pixel set) and their host run lengths."""
    g = torch.Generator().manual_seed(6)
    x = F.avg_pool2d(torch.randn((4, 1, 1024, 1024), generator=g), 31, 1, 15)[:, 0]
    m = (x > 0.02).numpy()
    m[0, :9, :7] = True
    m.setflags(write=False)
    return m, [_host_counts(v) for v in m]


def test_realistic_1024(dev, blobs):
    from protosam_amd import ops
    m, ref = blobs
    masks = torch.tensor(m).to(dev)
    counts, offsets = ops.rle_encode(masks)
    assert _split(counts, offsets) == ref
    assert ref[0][0] == 0 and all(len(r) > 100 for r in ref)
    assert torch.equal(ops.rle_decode(counts, offsets, 1024, 1024).bool(), masks)


def test_mask_to_rle_pytorch(dev, blobs):
    m, ref = blobs
    got = amg.mask_to_rle_pytorch(torch.tensor(m).to(dev))
    assert got == [{"size": [1024, 1024], "counts": r} for r in ref]
    assert all(type(v) is int for v in got[0]["counts"][:8])
    small = np.random.default_rng(8).random((6, 48, 44)) < 0.5
    assert amg.mask_to_rle_pytorch(torch.from_numpy(small.astype(np.uint8)).to(dev)) == [amg.mask_to_rle(v) for v in small]
    assert amg.mask_to_rle_pytorch(torch.zeros((0, 48, 44), dtype=torch.uint8, device=dev)) == []


def test_rle_to_mask_device(dev):
    rng = np.random.default_rng(9)
    for H, W in ((5, 3), (64, 65), (257, 132)):
        m = rng.random((4, H, W)) < 0.3
        m[1, 0, 0] = True                                           # a zero-length first run
        m[2] = True
        m[3] = False
        rles = [amg.mask_to_rle(v) for v in m]
        assert rles[1]["counts"][0] == 0 and rles[2]["counts"] == [0, H * W]
        rles.append({"size": [H, W], "counts": [3, 0, 0, 2, H * W - 5]})    # zero-length runs inside a hand-made list
        out = amg.rle_to_mask_device(rles, dev)
        assert out.dtype == torch.uint8 and out.is_cuda and tuple(out.shape) == (5, H, W)
        for i, r in enumerate(rles):
            np.testing.assert_array_equal(out[i].cpu().numpy().astype(bool), amg.rle_to_mask(r))
    with pytest.raises(ValueError):
        amg.rle_to_mask_device([{"size": [4, 4], "counts": [3, -1, 14]}], dev)
    with pytest.raises(ValueError):
        amg.rle_to_mask_device([{"size": [4, 4], "counts": [3, 12]}], dev)


# ---- the generator: RLE records without a full-size download --------------------------------------------------------------
@pytest.fixture(scope="module")
def sam_small(dev):
    """SAM vit_b with two encoder blocks and synthetic weights: the configuration the generator's own GPU tests use."""
    from protosam_amd import synth_cases as gi
    from protosam_amd.sam_wrapper import SamWrapper
    torch.set_num_threads(min(32, os.cpu_count() or 8))
    w = SamWrapper({"model_type": "vit_b", "sam_checkpoint": f"random:{gi.AMG_SEED}:{gi.AMG_ENCODER_DEPTH}",
                    "generator_args": dict(gi.AMG_ARGS)}).to(dev)
    return w.sam


def _compare_modes(sam, image, args, min_records):
    from protosam_amd.segment_anything import SamAutomaticMaskGenerator
    binary = SamAutomaticMaskGenerator(sam, **dict(args, output_mode="binary_mask")).generate(image)
    rle = SamAutomaticMaskGenerator(sam, **dict(args, output_mode="uncompressed_rle")).generate(image)
    assert len(binary) == len(rle) >= min_records
    for a, b in zip(binary, rle):
        assert set(a) == set(b) == {"segmentation", "area", "bbox", "predicted_iou", "point_coords", "stability_score", "crop_box"}
        assert b["segmentation"] == amg.mask_to_rle(a["segmentation"])
        assert all(type(v) is int for v in b["segmentation"]["counts"][:4]) and type(b["segmentation"]["size"][0]) is int
        for k in a:
            if k != "segmentation":
                assert a[k] == b[k], k
        assert amg.area_from_rle(b["segmentation"]) == a["area"]
        coco = amg.coco_encode_rle(b["segmentation"])
        assert isinstance(coco["counts"], str) and coco["size"] == b["segmentation"]["size"]
        assert amg.coco_decode_rle(coco) == b["segmentation"]
    return len(rle)


def test_generate_rle_fast_path(dev, sam_small):
    from protosam_amd import synth_cases as gi
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_outputs.npz"))
    t_iou, t_stab = (float(v) for v in gold["amg_thresholds"])
    img, _ = gi.amg_case()
    n = _compare_modes(sam_small, img, dict(gi.AMG_ARGS, pred_iou_thresh=t_iou, stability_score_thresh=t_stab), 10)
    print(f"fast path: {n} records of 1024 x 1024")


def test_generate_rle_general_path(dev, sam_small):
    from protosam_amd import synth_cases as gi
    n = _compare_modes(sam_small, gi.amg_small_case(), dict(gi.AMG_CROP_ARGS, crop_nms_thresh=1.0), 100)
    print(f"general path (crop_n_layers = 1): {n} records of 48 x 44")
