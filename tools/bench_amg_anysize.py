"""Times the mask generator on images that are not at the model's input size: the fused route (psam_mask_stats_resized /
psam_mask_binarize_resized, PSAM_AMG_RESIZE=fused) against the materialising one (PSAM_AMG_RESIZE=materialise). Needs the GPU;
every timed window ends in a device synchronise.

  python tools/bench_amg_anysize.py [--sam vit_b] [--depth N] [--points 32] [--reps 7] [--sizes 480x640,1080x1920,352x352]
                                    [--tree DIR] [--skip-kernels] [--skip-batch]

(a) `generate` per image, fused against materialise, per size and per setting. Both routes work only on the candidates that pass
    the predicted-IoU filter (the materialising one writes them at full size, the fused one skips the others in the statistics
    kernel), so the share that passes scales both; with synthetic weights the default threshold passes none. Settings: `defaults`
    (the generator's), `half` (predicted-IoU threshold at the image's median predicted IoU, stability filter off), `all` (both
    score filters off).
(b) `generate_batch` over 8 images of mixed sizes against 8 `generate` calls (setting `half` of the first image).
(c) the kernels alone, HIP events, 3 * points^2 planes: psam_mask_stats_resized against the chain it replaces, psam_mask_upsample
    -> crop -> psam_resize2d -> psam_plane_stats in chunks of 64 planes (all planes), the scored form with half and with none of
    the planes passing, and psam_mask_binarize_resized of 64 planes.
`--tree DIR` imports the package from another checkout (the parent commit: one leg, whatever `generate` does there).
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


def _ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def _stat(v):
    return (round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3))


def _alternate(legs, reps):
    """legs: name -> callable. One warm-up each, then `reps` rounds of every leg in turn -> name -> (median, min, max) ms."""
    for fn in legs.values():
        fn()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(_ms(fn))
    return {k: _stat(v) for k, v in times.items()}


def _events(fn, reps):
    """(median, min, max) ms of fn's device work between two HIP events, after one warm-up"""
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return _stat(out)


def _image(h, w, seed):
    g = np.random.RandomState(seed)
    coarse = torch.from_numpy(g.rand(1, 3, h // 32 + 2, w // 32 + 2).astype(np.float32))
    img = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear")[0].permute(1, 2, 0).numpy() * 255.0
    return np.ascontiguousarray(img.clip(0, 255).astype(np.uint8))


def _generators(sam, **kw):
    """name -> generator: fused and materialise where the checkout has the switch, else the one route it has"""
    from protosam_amd.segment_anything import SamAutomaticMaskGenerator
    probe = SamAutomaticMaskGenerator(sam, **kw)
    if not hasattr(probe, "amg_resize"):
        return {"parent": probe}
    out = {}
    old = os.environ.get("PSAM_AMG_RESIZE")
    for name in ("fused", "materialise"):
        os.environ["PSAM_AMG_RESIZE"] = name
        out[name] = SamAutomaticMaskGenerator(sam, **kw)
    if old is None:
        del os.environ["PSAM_AMG_RESIZE"]
    else:
        os.environ["PSAM_AMG_RESIZE"] = old
    return out


def _settings(sam, points, image):
    """name -> generator arguments; `half` needs the image's predicted IoUs"""
    from protosam_amd.segment_anything import SamAutomaticMaskGenerator
    g = SamAutomaticMaskGenerator(sam, points_per_side=points)
    g.generate(image)
    med = float(np.median(g._iou[:, 1:].cpu().numpy()))
    return {"defaults": dict(points_per_side=points),
            "half": dict(points_per_side=points, pred_iou_thresh=med if med > 0 else 1e-9, stability_score_thresh=0.0),
            "all": dict(points_per_side=points, pred_iou_thresh=0.0, stability_score_thresh=0.0)}


def per_image(a, sam, sizes):
    for h, w in sizes:
        image = _image(h, w, h + w)
        for name, kw in _settings(sam, a.points, image).items():
            gens = _generators(sam, **kw)
            recs = {k: g.generate(image) for k, g in gens.items()}
            first = next(iter(recs.values()))
            for r in recs.values():
                assert [x["area"] for x in r] == [x["area"] for x in first] and [x["bbox"] for x in r] == [x["bbox"] for x in first]
            thr = kw.get("pred_iou_thresh", 0.88)                              # (a threshold of 0 switches the filter off)
            passed = int((gens[next(iter(gens))]._iou[:, 1:] > thr).sum()) if thr > 0 else 3 * a.points ** 2
            t = _alternate({k: (lambda g=g: g.generate(image)) for k, g in gens.items()}, a.reps)
            print(json.dumps(dict(stage="generate", size=[h, w], setting=name, candidates=3 * a.points ** 2, pass_pred_iou=passed,
                                  records=len(first), **{k + "_ms": v for k, v in t.items()})), flush=True)


def batch(a, sam, sizes):
    images = [_image(h, w, i) for i, (h, w) in enumerate((sizes * 8)[:7])] + [_image(1024, 1024, 99)]
    kw = _settings(sam, a.points, images[0])["half"]
    g = next(iter(_generators(sam, **kw).values()))
    one = lambda: [g.generate(im) for im in images]          # noqa: E731
    many = lambda: g.generate_batch(images)                   # noqa: E731
    r1, r2 = one(), many()
    assert [[x["area"] for x in r] for r in r1] == [[x["area"] for x in r] for r in r2]
    t = _alternate({"generate": one, "generate_batch": many}, a.reps)
    print(json.dumps(dict(stage="batch", images=[list(im.shape[:2]) for im in images], route=getattr(g, "amg_resize", "parent"),
                          records=[len(r) for r in r2], generate_ms=t["generate"], generate_batch_ms=t["generate_batch"])), flush=True)


def kernels(a, sam, sizes, dev):
    from protosam_amd import ops
    from protosam_amd.segment_anything.utils.transforms import ResizeLongestSide
    n, S, variant = a.points ** 2, sam.image_encoder.img_size, sam.variant_id()
    low = torch.randn((n, 4, 256, 256), device=dev)
    flat = low.view(-1, 256, 256)
    planes = torch.tensor([(c // 3) * 4 + 1 + c % 3 for c in range(3 * n)], device=dev)
    idx = planes[:64].to(torch.int32)
    for h, w in sizes:
        ih, iw = (int(v) for v in ResizeLongestSide.get_preprocess_shape(h, w, S))
        if (ih, iw) == (h, w):
            continue

        def chain():
            for lo in range(0, 3 * n, 64):
                up = ops.mask_upsample(flat[planes[lo:lo + 64]].contiguous(), S, variant)[:, :ih, :iw].contiguous()
                ops.plane_stats(ops.resize2d(up, h, w, variant), 0.0, 1.0)

        row = dict(stage="kernels", size=[h, w], input_size=[ih, iw], planes=3 * n, variant=variant, chain_ms=_events(chain, a.reps))
        if hasattr(ops, "mask_stats_resized"):
            frames = torch.zeros((64, h, w), dtype=torch.uint8, device=dev)
            row["stats_resized_ms"] = _events(lambda: ops.mask_stats_resized(low, 1, 3, S, (ih, iw), (h, w), variant, 0.0, 1.0), a.reps)
            score = torch.rand((n, 4), device=dev)                                   # half of the planes pass 0.5, none passes 2
            for name, t in (("half", 0.5), ("none", 2.0)):
                row[f"stats_resized_{name}_pass_ms"] = _events(
                    lambda: ops.mask_stats_resized(low, 1, 3, S, (ih, iw), (h, w), variant, 0.0, 1.0, score=score, score_thresh=t), a.reps)
            row["binarize_resized_64_ms"] = _events(
                lambda: ops.mask_binarize_resized(low, idx, S, (ih, iw), (h, w), variant, 0.0, out=frames), a.reps)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sam", default="vit_b")
    ap.add_argument("--depth", type=int, default=None)
    ap.add_argument("--points", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="480x640,1080x1920,352x352")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-batch", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    assert torch.cuda.is_available(), "bench_amg_anysize.py measures on the GPU; there is no CPU figure"
    dev = torch.device("cuda:0")
    from protosam_amd.sam_wrapper import SamWrapper
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    ck = "random:7" + (f":{a.depth}" if a.depth else "")
    sam = SamWrapper({"model_type": a.sam, "sam_checkpoint": ck, "generator_args": dict(points_per_side=a.points)}).cuda().sam
    print(json.dumps(dict(sam=a.sam, depth=a.depth, points=a.points ** 2, reps=a.reps, tree=os.path.abspath(a.tree),
                          times="[median, min, max] ms per leg")), flush=True)
    per_image(a, sam, sizes)
    if not a.skip_batch:
        batch(a, sam, sizes)
    if not a.skip_kernels:
        kernels(a, sam, sizes, dev)


if __name__ == "__main__":
    main()
