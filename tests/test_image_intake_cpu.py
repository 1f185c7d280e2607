"""CPU: the host side of the image-set path - the two restatements the GPU intake tests compare against (checked here against Pillow and
stock torch), `ResizeLongestSide` at sizes other than the model's, the listing rules of `ImageSet`, and `eval_detection`."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import intake_reference as ir

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


@pytest.mark.parametrize("hw,S", ir.SIZES)
def test_pillow_restatement_equals_pillow(hw, S):
    from PIL import Image
    h, w = hw
    oh, ow = ir.preprocess_shape(h, w, S)
    for img in (ir.random_image(h, w, 3, 1), ir.single_pixel_image(h, w, 3), ir.random_image(h, w, 0, 2)):
        ref = np.array(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
        got = ir.pillow_u8(img, oh, ow)
        assert got.shape == ref.shape and got.dtype == np.uint8
        assert np.array_equal(got, ref), int((got != ref).sum())


@pytest.mark.parametrize("hw,S", [c for c in ir.SIZES if min(c[0]) > 1])      # ATen misreads one-column images (test_frontend_reference_cpu.py)
def test_float64_restatement_bounds_stock_torch(hw, S):
    h, w = hw
    oh, ow = ir.preprocess_shape(h, w, S)
    x = torch.from_numpy(ir.random_image(h, w, 3, 3)).permute(2, 0, 1).float()
    got = F.interpolate(x[None], (oh, ow), mode="bilinear", align_corners=False, antialias=True)[0]
    ref, budget = ir.aten_f64(x.numpy(), oh, ow)
    err = np.abs(got.numpy().astype(np.float64) - ref)
    share = float((err / budget).max())
    print(f"{hw} -> {(oh, ow)}: max error {err.max():.3e}, budget {budget.max():.3e}, largest share used {share:.4f}")
    assert share <= 1.0
    got_n = (got - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)
    ref_n, budget_n = ir.aten_f64(x.numpy(), oh, ow, np.float32(MEAN), np.float32(STD))
    assert (np.abs(got_n.numpy().astype(np.float64) - ref_n) <= budget_n).all()


def test_apply_image_torch_equals_stock_interpolate_on_cpu():
    from protosam_amd.segment_anything.utils.transforms import ResizeLongestSide
    t = ResizeLongestSide(64)
    g = torch.Generator().manual_seed(4)
    for shape in ((37, 53), (3, 100, 75), (2, 3, 50, 20)):
        x = torch.rand(shape, generator=g) * 255
        target = t.get_preprocess_shape(shape[-2], shape[-1], 64)
        ref = F.interpolate(x[(None,) * (4 - x.dim())], target, mode="bilinear", align_corners=False, antialias=True)
        got = t.apply_image_torch(x)
        assert tuple(got.shape) == tuple(shape[:-2]) + target
        assert torch.equal(got, ref.reshape(got.shape))
    same = torch.rand((3, 64, 48), generator=g)
    assert t.apply_image_torch(same) is same        # already at the target: the identity, as before


def test_preprocess_pads_bottom_and_right_with_zeros():
    from protosam_amd.segment_anything.utils.transforms import ResizeLongestSide
    t = ResizeLongestSide(64)
    x = torch.full((3, 40, 64), 200.0)
    y = t.preprocess(x)
    assert tuple(y.shape) == (3, 64, 64)
    assert torch.equal(y[:, :40], (x - t.pixel_mean) / t.pixel_std)
    assert (y[:, 40:].view(torch.int32) == 0).all()                 # +0.0: the pad follows the normalisation
    m = torch.ones((40, 64))
    pm = t.preprocess(m)
    assert tuple(pm.shape) == (64, 64) and torch.equal(pm[:40], m) and (pm[40:] == 0).all()
    w = t.preprocess(torch.ones((64, 30)))
    assert tuple(w.shape) == (64, 64) and (w[:, 30:] == 0).all() and (w[:, :30] == 1).all()


def _png(path, hw, value=0, mode="RGB"):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    a = np.full(tuple(hw) + ((3,) if mode == "RGB" else ()), value, np.uint8)
    Image.fromarray(a).save(path)


def test_image_set_listing_rules(tmp_path):
    from protosam_amd import image_io
    ir_, gr = str(tmp_path / "images"), str(tmp_path / "masks")
    _png(f"{ir_}/b.png", (20, 30)); _png(f"{gr}/b.png", (20, 30), 255, "L")
    _png(f"{ir_}/a.jpg", (24, 16)); _png(f"{gr}/a.png", (24, 16), 255, "L")                    # a .jpg image with a .png mask
    _png(f"{ir_}/c.png", (20, 30)); _png(f"{gr}/c.png", (21, 30), 255, "L")                    # sizes differ: dropped
    _png(f"{ir_}/Kvasir/k.png", (10, 12)); _png(f"{gr}/Kvasir/k.png", (10, 12), 255, "L")      # one level of sub-directories
    _png(f"{ir_}/CVC-300/x.png", (10, 12)); _png(f"{gr}/CVC-300/x.png", (10, 12), 255, "L")    # excluded dataset name
    _png(f"{ir_}/Kvasir/deep/d.png", (10, 12)); _png(f"{gr}/Kvasir/deep/d.png", (10, 12), 255, "L")   # two levels: not listed
    (tmp_path / "images" / "notes.txt").write_text("not an image")
    pairs = image_io.list_pairs(ir_, gr)
    rel = [(os.path.relpath(a, ir_), os.path.relpath(b, gr)) for a, b in pairs]
    assert rel == [("Kvasir/k.png", "Kvasir/k.png"), ("a.jpg", "a.png"), ("b.png", "b.png")]
    s = image_io.ImageSet.__new__(image_io.ImageSet)                                           # (no device needed for the names)
    s.pairs, s.datasets = pairs, image_io.DATASETS
    assert [s.case(k) for k in range(3)] == ["Kvasir", "", ""]
    img, mask = image_io.decode_pair(*pairs[2])
    assert img.shape == (20, 30, 3) and img.dtype == np.uint8 and mask.shape == (20, 30) and set(np.unique(mask)) == {1}
    _png(f"{gr}/extra.png", (5, 5), 0, "L")
    with pytest.raises(ValueError):
        image_io.list_pairs(ir_, gr)                                                           # lists of different length cannot be paired


def test_eval_detection_counts():
    from protosam_amd import metrics
    gt = (10, 10, 100, 100)

    def pred_with_iou(frac):                       # same corner and width, height frac * 100: IoU = frac
        return {"pred_bbox": (10, 10, 100, int(round(100 * frac))), "gt_bbox": gt, "score": 0.5}
    ious = [1.0, 0.9, 0.72, 0.55, 0.3]
    rows = metrics.eval_detection([pred_with_iou(f) for f in ious], as_frame=False)
    thr = np.round(np.arange(0.5, 1.0, 0.05), 2)
    assert [r["iou_threshold"] for r in rows] == list(thr) and len(rows) == 10
    for r, t in zip(rows, thr):
        tp = sum(1 for f in ious if f >= t)
        assert (r["tp"], r["fp"], r["n_gt"]) == (tp, 5 - tp, 5)
        assert r["precision"] == tp / 5 and r["recall"] == tp / 5
        assert r["f1"] == 2 * (tp / 5) * (tp / 5) / (2 * tp / 5)
    assert [r["tp"] for r in rows] == [4, 4, 3, 3, 3, 2, 2, 2, 2, 1]
    miss = metrics.eval_detection([{"pred_bbox": (0, 0, 5, 5), "gt_bbox": (50, 50, 5, 5), "score": 0.1}] * 3, as_frame=False)
    assert all(r["tp"] == 0 and r["fp"] == 3 and r["precision"] == 0 and r["recall"] == 0 and math.isnan(r["f1"]) for r in miss)
    with pytest.raises(ZeroDivisionError):
        metrics.eval_detection([{"pred_bbox": (0, 0, 0, 0), "gt_bbox": (0, 0, 0, 0), "score": 0.0}], as_frame=False)
    try:
        import pandas  # noqa: F401
    except ImportError:
        assert metrics.eval_detection([pred_with_iou(1.0)]) == metrics.eval_detection([pred_with_iou(1.0)], as_frame=False)
    else:
        df = metrics.eval_detection([pred_with_iou(f) for f in ious])
        assert list(df.columns) == ["iou_threshold", "tp", "fp", "n_gt", "f1", "precision", "recall"] and list(df["tp"]) == [r["tp"] for r in rows]


def test_intake_size_range():
    from protosam_amd import ops
    assert ops.intake_shape(600, 900, 512) == (341, 512) and ops.intake_supported(600, 900, 512)
    assert ops.intake_supported(8192, 8192, 512) and not ops.intake_supported(8193, 100, 1024)
    assert ops.intake_supported(1024, 40, 64) and not ops.intake_supported(1100, 40, 64)    # 16 source rows per resized row is the limit
    assert not ops.intake_supported(0, 10, 64) and not ops.intake_supported(2000, 1, 64)        # a side that resizes to 0
    with pytest.raises(RuntimeError):
        ops.image_intake([torch.zeros((8, 8, 3), dtype=torch.uint8)], 64, 1, MEAN, STD)          # CPU tensors are rejected
