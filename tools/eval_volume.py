"""Scores one scan end to end on the GPU, as the reference's per-organ validation does, without moving a mask to the host:
ScanSlices -> class_part_table / class_support_slices -> evaluate_slices_class_supports -> Metric and score_slices.

  python tools/eval_volume.py                                   (two synthetic scans: query seed 0, support seed 1, organs 1 and 2)
  python tools/eval_volume.py --image q.nii.gz --label q_seg.nii.gz --support-image s.nii.gz --support-label s_seg.nii.gz --classes 1 6

Weights are the seeded synthetic ones of `runner.build_protosam` (`--sam-depth` / `--dino-depth` cut the encoders for a quick
run). Prints one JSON line: per-class scan-level Dice (`Metric.get_mDice`), the per-slice means of `score_slices`, slices per second.
`--surface` adds the boundary measures per organ beside Dice: scan-level HD95 and ASSD in 3-D (`runner.score_scan_surfaces` on the
kept masks) and their per-slice means, in the units of the NIfTI header's voxel spacing (`ScanSlices.info`; 1 for synthetic scans).
`--clean largest|min` (`--connectivity`, `--min-voxels`) also scores the scan after the 3-D connected-component clean-up of
`runner.clean_scan`: `scan_dice_per_class_clean`, `components_per_class`, `voxels_dropped_per_class` and, with `--surface`, the
`scan_*_per_class_clean` boundary measures.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def synthetic_scan(Z, S, seed):
    """image volume and a label volume with organ 1 (the synthetic organ) and organ 2 (an ellipse beside it)"""
    import numpy as np
    from protosam_amd.synth import ellipse_mask, synth_volume
    vol, lab = synth_volume(Z, S, seed=seed)
    lab = (lab.numpy() > 0).astype(np.uint8)
    lab[(lab == 0) & (ellipse_mask(S, 0.3, 0.7, 0.1, 0.12) > 0)[None]] = 2
    return vol.numpy().astype(np.float32), lab


def main():
    ap = argparse.ArgumentParser()
    for name in ("--image", "--label", "--support-image", "--support-label"):
        ap.add_argument(name)
    ap.add_argument("--classes", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--slices", type=int, default=12, help="depth of the synthetic scans")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--n-parts", type=int, default=3)
    ap.add_argument("--sam-type", default="vit_b")
    ap.add_argument("--sam-depth", type=int, default=None)
    ap.add_argument("--dino-depth", type=int, default=None)
    ap.add_argument("--surface", action="store_true", help="also HD95 and ASSD per organ (spacing from the NIfTI header)")
    ap.add_argument("--clean", choices=("largest", "min"), default=None,
                    help="also score the scan after a 3-D connected-component clean-up per organ: keep the largest component, or "
                         "drop the components below --min-voxels")
    ap.add_argument("--connectivity", type=int, choices=(6, 18, 26), default=26)
    ap.add_argument("--min-voxels", type=int, default=0, help="components below this many voxels are dropped (with either --clean)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from protosam_amd import metrics, runner
    from protosam_amd.protosam import InputFactory, TYPE_ALPNET
    from protosam_amd.slice_io import ScanSlices, slice_spacing
    if not torch.cuda.is_available():
        raise SystemExit("eval_volume.py runs the GPU pipeline: no device found")
    dev = torch.device("cuda:0")
    S, classes = args.size, args.classes
    if args.image:
        qry = ScanSlices.from_nifti(args.image, dev, S, label_path=args.label)
        sup = ScanSlices.from_nifti(args.support_image, dev, S, label_path=args.support_label)
    else:
        (qv, ql), (sv, sl) = synthetic_scan(args.slices, S, 0), synthetic_scan(args.slices, S, 1)
        qry = ScanSlices.from_volume(qv, dev, S, labels_zyx=ql)
        sup = ScanSlices.from_volume(sv, dev, S, labels_zyx=sl)
    model, _ = runner.build_protosam(dev, sam_type=args.sam_type, image_size=S, dino_depth=args.dino_depth, sam_depth=args.sam_depth)
    vol, labels = qry.images[:, 0].contiguous(), qry.labels
    part_table = runner.class_part_table(labels, classes, args.n_parts)
    sup_z = runner.class_support_slices(sup.labels, classes, args.n_parts)
    q0 = qry.images[:1]
    supports = []
    for c, cls in enumerate(classes):
        per_part = []
        for z in sup_z[c]:
            inp = InputFactory.create_input(TYPE_ALPNET, q0, support_images=[sup.images[z][None].contiguous()],
                                            support_labels=[(sup.labels[z] == cls).float()[None].contiguous()], isval=True, val_wsize=2)
            inp.to(dev)
            per_part.append(inp)
        supports.append(per_part)
    zs = list(range(vol.shape[0]))
    runner.evaluate_slices_class_supports(model, vol, labels, supports, part_table, zs[:args.batch], classes, batch=args.batch)   # warm
    torch.cuda.synchronize()
    C = len(classes)
    spacing = slice_spacing(qry.info, S)
    keep = torch.empty((len(zs), C, S, S), dtype=torch.uint8, device=dev) if args.surface or args.clean else None
    t0 = time.perf_counter()
    res = runner.evaluate_slices_class_supports(model, vol, labels, supports, part_table, zs, classes, batch=args.batch, keep=keep,
                                                surface=dict(spacing=spacing) if args.surface else None)
    table, prompted = res[0], res[1]
    host = table.cpu().numpy()                                    # the one copy of the scan: 96 bytes per (slice, class)
    dt = time.perf_counter() - t0
    extra = {}
    nan_to_none = lambda v: None if v != v else float(v)          # noqa: E731  (JSON has no NaN)
    if args.surface:
        per_slice = metrics.score_surfaces(metrics.surface_table(keep, labels, metrics.surface_rows(len(zs), classes).tolist(),
                                                                 spacing, table=res[2]),
                                           cases=[f"class{classes[r % C]}" for r in range(len(host))])
        scan = runner.score_scan_surfaces(keep, labels, classes, spacing)
        extra = {"spacing_zyx": list(spacing), "scan_hd95_per_class": [nan_to_none(v) for v in scan[:, metrics.HD95]],
                 "scan_assd_per_class": [nan_to_none(v) for v in scan[:, metrics.ASSD]],
                 "scan_hd_per_class": [nan_to_none(v) for v in scan[:, metrics.HD]],
                 "slice_mean_hd95_per_class": per_slice["hd95_cases"], "slice_mean_assd_per_class": per_slice["assd_cases"],
                 "surface_rows_scored": len(per_slice["rows"]), "surface_rows_empty_pred": len(per_slice["empty_pred"]),
                 "surface_rows_empty_gt": len(per_slice["empty_gt"])}
    if args.clean:
        # the kept masks cleaned where they lie, then one counts table and (with --surface) one surface table per organ
        from protosam_amd import ops
        cleaned, info = runner.clean_scan(keep, classes, connectivity=args.connectivity, min_voxels=args.min_voxels,
                                          keep_largest=args.clean == "largest", out=keep)
        scan_counts = runner.score_scan(cleaned, labels, classes).cpu().numpy()
        mc = metrics.Metric(max_label=max(classes))
        for c, cls in enumerate(classes):
            tp, fp, fn, tn = scan_counts[c, :4]
            mc.record_table(np.array([[tn, fn, fp], [tp, fp, fn]]), labels=[cls])
        with np.errstate(all="ignore"):
            dice_clean, _, _ = mc.get_mDice(labels=classes, n_scan=0)
        regions = ops.volume_regions_table(info)
        extra.update({"scan_dice_per_class_clean": [nan_to_none(v) for v in dice_clean],
                      "components_per_class": [r["components"] for r in regions],
                      "voxels_dropped_per_class": [r["voxels_dropped"] for r in regions]})
        if args.surface:
            scan = runner.score_scan_surfaces(cleaned, labels, classes, spacing)
            extra.update({"scan_hd95_per_class_clean": [nan_to_none(v) for v in scan[:, metrics.HD95]],
                          "scan_assd_per_class_clean": [nan_to_none(v) for v in scan[:, metrics.ASSD]],
                          "scan_hd_per_class_clean": [nan_to_none(v) for v in scan[:, metrics.HD]]})
    m = metrics.Metric(max_label=max(classes))
    for k in range(len(zs)):
        for c, cls in enumerate(classes):
            tp, fp, fn, tn = host[k * C + c, :4]
            m.record_table(np.array([[tn, fn, fp], [tp, fp, fn]]), labels=[cls])      # (background, organ): validation.py:304's call
    with np.errstate(all="ignore"):
        dice_cls, dice_mean, _ = m.get_mDice(labels=classes, n_scan=0)
    sc = metrics.score_slices(host, cases=[f"class{classes[r % C]}" for r in range(len(host))])
    print(json.dumps({"classes": classes, "scan_dice_per_class": [float(v) for v in dice_cls], "scan_dice_mean": float(dice_mean),
                      "slices": len(zs), "rows_scored": len(sc["rows"]), "slice_mean_dice": sc["mean_dice"], "slice_mean_iou": sc["mean_iou"],
                      "slice_mean_dice_per_class": sc["dice_cases"], "prompted_pairs": int(sum(prompted)),
                      "slices_per_s": len(zs) / dt, **extra}))


if __name__ == "__main__":
    main()
