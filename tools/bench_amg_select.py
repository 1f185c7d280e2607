"""Times the mask generator's candidate selection on the device against the host lines, and the batch entry points against the
single-image ones. Needs the GPU; every timed window ends in a device synchronise or a blocking copy.

  python tools/bench_amg_select.py [--sam vit_h] [--depth N] [--points 32] [--images 8] [--reps 7] [--skip-models]

(a) the selection stage alone, on fabricated tables of 3 * points^2 candidates (3072) in `clusters` tight clusters, so that about
    `clusters` survive the NMS: `_select_host` (two downloads, numpy filters, nms_xyxy, one upload of the plane indices) against
    `psam_amg_select` + the one copy of its record table + the same candidate dict. The statistics table and the predicted IoUs
    are on the device before either leg starts, as they are in the generator.
(b) SamWrapper.forward_batch of `images` images against that many forward calls, and generate_batch against generate calls, with
    the two settings of tools/bench_amg.py (the generator's defaults; everything kept but the 64 best predicted IoUs).
The legs alternate inside every repetition after one warm-up of each; medians with the minimum and maximum are reported.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def _alternate(legs, reps):
    """legs: name -> callable. One warm-up each, then `reps` rounds of every leg in turn -> name -> (median, min, max) ms."""
    for fn in legs.values():
        fn()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(_ms(fn))
    return {k: (round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)) for k, v in times.items()}


def _clustered_table(n, clusters, seed):
    """stats int32 [n,8] and iou4 fp32 [n/3,4]: boxes in tight clusters (IoU > 0.9 inside, 0 between), every row passes the
    default score filters"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, clusters, n)
    x0, y0 = (c % 40) * 25 + rng.integers(0, 2, n), (c // 40) * 25 + rng.integers(0, 2, n)
    stats = np.zeros((n, 8), np.int32)
    stats[:, 0], stats[:, 1], stats[:, 2] = 99, 100, 400
    stats[:, 3], stats[:, 4], stats[:, 5], stats[:, 6] = x0, y0, x0 + 20, y0 + 20
    iou4 = np.zeros((n // 3, 4), np.float32)
    iou4[:, 1:] = (0.9 + 0.1 * rng.random(n, dtype=np.float32)).reshape(-1, 3)
    return stats, iou4


def selection_stage(points, reps, dev):
    from protosam_amd.segment_anything import SamAutomaticMaskGenerator
    n = points * points
    g = SamAutomaticMaskGenerator.__new__(SamAutomaticMaskGenerator)
    g.pred_iou_thresh, g.stability_score_thresh, g.box_nms_thresh = 0.88, 0.95, 0.7
    out = []
    for clusters in (8, 100, 1000):
        stats, iou4 = _clustered_table(3 * n, clusters, seed=clusters)
        ctx = dict(pts=np.zeros((n, 2)), n=n, size=(1024, 1024), low=torch.zeros(1, device=dev),
                   stats=torch.from_numpy(stats).to(dev), iou=torch.from_numpy(iou4).to(dev))
        sel_out = torch.empty((3 * n * 9 + 1,), dtype=torch.int32, device=dev)

        def device():
            o, rec, _ = g._select_enqueue(ctx, out=sel_out)
            return g._cand_from_records(ctx, o.cpu().numpy(), rec)

        a, b = g._select_host(ctx), device()
        for k in ("iou_preds", "boxes", "area"):
            assert np.array_equal(a[k], b[k]), k
        assert torch.equal(a["plane"], b["plane"])
        t = _alternate({"host": lambda: g._select_host(ctx), "device": device}, reps)
        out.append(dict(stage="selection", candidates=3 * n, survivors=len(a["boxes"]), host_ms=t["host"], device_ms=t["device"]))
        print(json.dumps(out[-1]), flush=True)
    return out


def pipelines(a, dev):
    from protosam_amd.sam_wrapper import SamWrapper
    from protosam_amd.synth import synth_pair
    ck = "random:7" + (f":{a.depth}" if a.depth else "")
    images, labels = [], []
    for seed in range(3, 3 + a.images):
        _, _, q, gt = synth_pair(1024, seed=seed)
        q = q[0].permute(1, 2, 0).numpy()
        images.append(((q - q.min()) / (q.max() - q.min()) * 255).astype(np.uint8))
        labels.append(gt[0].numpy().astype(np.uint8))
    out = []
    for name, gargs in (("defaults", {}), ("keep_top64", dict(pred_iou_thresh=0.0, stability_score_thresh=0.0, box_nms_thresh=1.0))):
        w = SamWrapper({"model_type": a.sam, "sam_checkpoint": ck,
                        "generator_args": dict(points_per_side=a.points, **gargs)}).cuda()
        g = w.mask_generator
        if name == "keep_top64":
            thr = float(np.sort(g._candidates(images[0])["iou_preds"])[-64])
            g.pred_iou_thresh = thr if thr > 0 else 1e-9

        def quiet(fn):                      # with synthetic weights the defaults keep no proposal: forward's TypeError, after the work
            def run():
                try:
                    return fn()
                except TypeError:
                    return None
            return run

        def one():                          # every image does its work, whether or not it ends in the TypeError
            return [quiet(lambda: w(im, lb))() for im, lb in zip(images, labels)]

        batch = quiet(lambda: w.forward_batch(images, labels))
        r1, r2 = one(), batch()
        if r2 is None:
            assert any(m is None for m in r1)
        else:
            assert np.array_equal(np.stack(r1), r2)
        t = _alternate({"forward": one, "forward_batch": batch}, a.reps)
        n_masks = [s["n_masks"] for s in w.last_stats] if isinstance(w.last_stats, list) and r2 is not None else None
        out.append(dict(stage="wrapper", setting=name, images=a.images, forward_ms=t["forward"], forward_batch_ms=t["forward_batch"],
                        n_masks=n_masks))
        print(json.dumps(out[-1]), flush=True)
        gen = lambda: [g.generate(im) for im in images]          # noqa: E731
        genb = lambda: g.generate_batch(images)                   # noqa: E731
        r1, r2 = gen(), genb()
        assert [len(x) for x in r1] == [len(x) for x in r2]
        t = _alternate({"generate": gen, "generate_batch": genb}, a.reps)
        out.append(dict(stage="generate", setting=name, images=a.images, generate_ms=t["generate"], generate_batch_ms=t["generate_batch"],
                        records=[len(x) for x in r2]))
        print(json.dumps(out[-1]), flush=True)
        del w, g
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sam", default="vit_h")
    ap.add_argument("--depth", type=int, default=None)
    ap.add_argument("--points", type=int, default=32)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-models", action="store_true", help="part (a) only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_amg_select.py measures on the GPU; there is no CPU figure"
    dev = torch.device("cuda:0")
    print(json.dumps(dict(sam=a.sam, depth=a.depth, points=a.points ** 2, images=a.images, reps=a.reps,
                          times="[median, min, max] ms per leg; (b) per batch of `images` images")), flush=True)
    selection_stage(a.points, max(a.reps, 15), dev)
    if not a.skip_models:
        pipelines(a, dev)


if __name__ == "__main__":
    main()
