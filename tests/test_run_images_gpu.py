"""GPU: the image-set driver - `runner.run_images` / `evaluate_images` over an `image_io.ImageSet` of PNG pairs of different sizes,
with the reduced-depth ProtoSAM of tests/test_protosam_gpu.py, against `forward_batch` called by hand and scores computed on the host."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S = 512


def _numpy_box(m):
    ys, xs = np.nonzero(m)
    if ys.size == 0:
        return (0, 0, 0, 0)
    return (int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1))


def test_run_and_evaluate_images(dev, tmp_path):
    from test_protosam_gpu import _build
    from protosam_amd import metrics, runner
    from protosam_amd.image_io import ImageSet
    from protosam_amd.protosam import InputFactory, TYPE_ALPNET
    from protosam_amd.synth import IMAGE_PAIR_SIZES, write_image_pairs
    image_root, gt_root = write_image_pairs(str(tmp_path), 7, seed=3)
    images = ImageSet(image_root, gt_root, dev, S=S)
    assert len(images) == 7 and len(set(IMAGE_PAIR_SIZES[:6])) == 6
    sup_i, sup_m, _ = images.get_support(1, indices=[0])
    assert tuple(sup_i[0].shape) == (1, 3, S, S) and tuple(sup_m[0].shape) == (1, S, S)
    queries = list(range(1, 7))                                   # six images: a batch of four and a short one of two
    model, _ = _build(dev, "random:vit_b:1234:2", 2, use_bbox=True, use_points=True, point_mode="both")

    masks, prompts, scores = runner.run_images(model, images, (sup_i, sup_m), queries, batch=4)
    assert tuple(masks.shape) == (6, S, S) and masks.dtype == torch.uint8 and len(prompts) == len(scores) == 6

    want, want_scores, labels, sizes = [], [], [], []
    for part in (queries[:4], queries[4:]):
        q, lab, orig, cases = images.load(part)
        assert tuple(q.shape) == (len(part), 3, S, S) and tuple(lab.shape) == (len(part), S, S) and cases == [""] * len(part)
        inp = InputFactory.create_input(TYPE_ALPNET, q, support_images=sup_i, support_labels=sup_m, isval=True, val_wsize=2)
        for pred, sc in model.forward_batch(q, inp):
            want.append(pred.to(torch.uint8) if pred.shape[-1] == S else torch.zeros((S, S), dtype=torch.uint8, device=dev))
            want_scores.append(sc)
        labels.append(lab)
        sizes += orig
    assert sizes == [IMAGE_PAIR_SIZES[k % 6] for k in queries]
    assert torch.equal(masks, torch.stack(want))
    assert [list(map(float, s)) for s in scores] == [list(map(float, s)) for s in want_scores]
    labels = torch.cat(labels)
    assert int(masks.sum()) > 0 and set(torch.unique(labels).tolist()) == {0.0, 1.0}

    keep = torch.zeros((6, S, S), dtype=torch.uint8, device=dev)
    res = runner.evaluate_images(model, images, (sup_i, sup_m), queries, batch=4, keep=keep)
    assert torch.equal(keep, masks)
    host_m, host_l = masks.cpu(), labels.cpu()
    assert res["rows"] == list(range(6))                          # every synthetic mask has foreground
    for k in range(6):
        d = metrics.get_dice_iou_precision_recall(host_m[k].double(), host_l[k].double())
        for name in ("dice", "iou", "precision", "recall"):
            assert res[name][k] == float(d[name]), (k, name)
        box = res["bboxes_w_scores"][k]
        assert box["pred_bbox"] == _numpy_box(host_m[k].numpy()) and box["gt_bbox"] == _numpy_box(host_l[k].numpy())
        assert box["score"] == float(np.mean(want_scores[k]))
    assert res["mean_dice"] == float(np.mean(res["dice"])) and res["dice_cases"] == {"": float(np.mean(res["dice"]))}

    boxes = [b for b in res["bboxes_w_scores"] if b["pred_bbox"][2] > 0]
    table = metrics.eval_detection(boxes, as_frame=False)
    for row in table:
        tp = sum(1 for b in boxes if metrics.calc_iou(_numpy_box_of(b, "pred_bbox"), _numpy_box_of(b, "gt_bbox")) >= row["iou_threshold"])
        assert (row["tp"], row["fp"], row["n_gt"]) == (tp, len(boxes) - tp, len(boxes))
        assert row["precision"] == tp / len(boxes) and row["recall"] == tp / len(boxes)
        assert (np.isnan(row["f1"]) and tp == 0) or row["f1"] == 2 * row["precision"] * row["recall"] / (row["precision"] + row["recall"])


def _numpy_box_of(b, key):
    return tuple(int(v) for v in b[key])
