"""Scores a set of image files end to end on the GPU, as the polyp branch of the reference's validation does
(validation_protosam.py:307-449): ImageSet -> get_support -> evaluate_images -> score_slices and eval_detection.

  python tools/eval_images.py --synthetic 8                       (eight seeded PNG pairs of mixed sizes in a temporary directory)
  python tools/eval_images.py --images TestDataset/images --masks TestDataset/masks [--support-file support.txt]

Weights are the seeded synthetic ones of `runner.build_protosam` (`--sam-depth` / `--dino-depth` cut the encoders for a quick
run). The first image pair is the support unless --support-file names one. Prints one JSON line: the per-image means of
`score_slices`, the per-case means, the detection table of `eval_detection` (an undefined f1 as null) and images per second.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images")
    ap.add_argument("--masks")
    ap.add_argument("--support-file", help="rows of 'image_path mask_path'; the first --n-support are the support set")
    ap.add_argument("--n-support", type=int, default=1)
    ap.add_argument("--synthetic", type=int, default=0, metavar="N")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--sam-type", default="vit_b")
    ap.add_argument("--sam-depth", type=int, default=None)
    ap.add_argument("--dino-depth", type=int, default=None)
    args = ap.parse_args()
    if bool(args.synthetic) == bool(args.images and args.masks):
        raise SystemExit("give either --images and --masks, or --synthetic N")
    import torch
    from protosam_amd import metrics, runner
    from protosam_amd.image_io import ImageSet
    from protosam_amd.synth import write_image_pairs
    if not torch.cuda.is_available():
        raise SystemExit("eval_images.py runs the GPU pipeline: no device found")
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        image_root, gt_root = write_image_pairs(tmp, args.synthetic) if args.synthetic else (args.images, args.masks)
        images = ImageSet(image_root, gt_root, dev, S=args.size)
        if len(images) < 2:
            raise SystemExit(f"{len(images)} usable image pairs under {image_root}: need a support and at least one query")
        if args.support_file:
            sup_i, sup_m, _ = images.get_support(args.n_support, text_file=args.support_file)
            queries = list(range(len(images)))
        else:
            sup_i, sup_m, _ = images.get_support(args.n_support, indices=list(range(args.n_support)))
            queries = list(range(args.n_support, len(images)))
        model, _ = runner.build_protosam(dev, sam_type=args.sam_type, image_size=args.size, dino_depth=args.dino_depth,
                                         sam_depth=args.sam_depth)
        runner.evaluate_images(model, images, (sup_i, sup_m), queries[:args.batch], batch=args.batch)      # warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = runner.evaluate_images(model, images, (sup_i, sup_m), queries, batch=args.batch)
        dt = time.perf_counter() - t0
    boxes = [b for b in res["bboxes_w_scores"] if b["pred_bbox"][2] * b["pred_bbox"][3] + b["gt_bbox"][2] * b["gt_bbox"][3] > 0]
    table = metrics.eval_detection(boxes, as_frame=False) if boxes else []
    print(json.dumps({"images": len(queries), "rows_scored": len(res["rows"]), "mean_dice": res["mean_dice"], "mean_iou": res["mean_iou"],
                      "mean_precision": res["mean_precision"], "mean_recall": res["mean_recall"], "dice_cases": res["dice_cases"],
                      "iou_cases": res["iou_cases"], "prompted": int(sum(res["n_prompts"])),
                      "detection": [{k: (None if v != v else float(v)) for k, v in r.items()} for r in table], "images_per_s": len(queries) / dt}))


if __name__ == "__main__":
    main()
