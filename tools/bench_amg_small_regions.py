"""Times the mask generator's small-region stage (min_mask_region_area > 0): the per-mask host loop (PSAM_AMG_REGIONS=host: two
psam_ccl calls and two downloads per mask, then statistics and nms_xyxy on the host) against the device chain
(PSAM_AMG_REGIONS=device: ops.small_regions_select and one download). Needs the GPU; every timed window ends in a device
synchronise.

  python tools/bench_amg_small_regions.py [--sam vit_b] [--depth N] [--points 32] [--reps 5] [--tree DIR] [--skip-stage]
                                          [--skip-generate] [--stage-cases 64x512,256x512,64x1024,256x1024]
                                          [--generate-cases 32:0.7,16:1.0]

(a) the stage alone on synthetic blob-plus-speckle masks, m masks of S x S per case: wall time per call and per mask and the
    number of host synchronisations (device-to-host copies and scalar reads) per call, for each route.
(b) `generate` on a 1024 x 1024 image with min_mask_region_area = 100, crop_n_layers 0 and 1, random-weight SAM, predicted-IoU
    threshold at the image's median predicted IoU (with synthetic weights the default passes nothing), per case "points per side :
    box_nms_thresh" (noise-like masks span the image, so the default NMS at 0.7 leaves one mask for the stage; at 1.0 every
    candidate that passes the filter reaches it): wall time per call for each route, host synchronisations per call, and the
    share of the call the stage takes - the stage alone, timed on the very masks that enter it, over the call.
`--tree DIR` imports the package from another checkout; one without the switch (the parent commit) reports its only route as
`parent`, the host loop. The legs alternate inside every repetition after one warm-up of each; medians with minimum and maximum.
"""
import argparse
import contextlib
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


@contextlib.contextmanager
def _count_syncs(out):
    """counts the calls that make the host wait for the device: .cpu(), .item(), .tolist() and bool() of a device tensor"""
    T = torch.Tensor
    saved = {n: getattr(T, n) for n in ("cpu", "item", "tolist", "__bool__")}

    def wrap(name):
        inner = saved[name]

        def f(self, *a, **k):
            if self.is_cuda:
                out[0] += 1
            return inner(self, *a, **k)
        return f

    for n in saved:
        setattr(T, n, wrap(n))
    try:
        yield
    finally:
        for n, v in saved.items():
            setattr(T, n, v)


def _syncs(fn):
    n = [0]
    with _count_syncs(n):
        fn()
    return n[0]


def synthetic_masks(m, S, dev, seed=0):
    """m masks of S x S: an ellipse of random place and size, flipped on 0.2 % of the pixels (speckle inside and outside) and with
    a few holes of 30 to 300 pixels - what a binarised SAM mask looks like before the stage"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    out = torch.empty((m, S, S), dtype=torch.uint8)
    for i in range(m):
        cy, cx, ry, rx = (torch.rand(4, generator=g) * torch.tensor([S, S, S / 3, S / 3]) + torch.tensor([0, 0, S / 16, S / 16])).tolist()
        blob = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1
        for _ in range(3):
            hy, hx, hr = (torch.rand(3, generator=g) * torch.tensor([2 * ry, 2 * rx, 7.0]) + torch.tensor([cy - ry, cx - rx, 3.0])).tolist()
            blob &= ~((yy - hy) ** 2 + (xx - hx) ** 2 < hr * hr)
        out[i] = (blob ^ (torch.rand((S, S), generator=g) < 0.002)).to(torch.uint8)
    return out.to(dev)


def host_stage(g, masks, area, nms_thresh):
    """the host route's stage as `_generate_general` runs it, on masks uint8 [m,H,W] -> (kept indices, new masks of the kept)"""
    from protosam_amd import ops
    from protosam_amd.segment_anything.utils.amg import nms_xyxy
    m, H, W = masks.shape
    cw = ops.CclWorkspace(H, W, 4096, masks.device)
    new_masks, scores = [], []
    for i in range(m):
        x, c1 = g._remove_small_regions(masks[i], area, "holes", cw)
        x, c2 = g._remove_small_regions(x, area, "islands", cw)
        new_masks.append(x)
        scores.append(float(not c1 and not c2))
    nm = torch.stack(new_masks)
    st, _ = ops.plane_stats(nm.float().contiguous(), 0.5, 0.0, binarize=False)
    st = st.cpu().numpy()
    nb = st[:, 3:7].astype(np.int64)
    nb[st[:, 2] == 0] = 0
    keep = nms_xyxy(nb, np.asarray(scores, dtype=np.float32), nms_thresh)
    return keep, nm[torch.from_numpy(keep).to(masks.device)], nb, st[:, 2]


def device_stage(masks, area, nms_thresh):
    from protosam_amd import ops
    nm, table = ops.small_regions_select(masks, area, nms_thresh)
    keep, info, nb = ops.small_regions_table(table.cpu().numpy(), len(masks))
    return keep, nm[torch.from_numpy(keep).to(masks.device)], nb, info[:, 2]


def _stage_legs(g, masks, area, nms_thresh):
    from protosam_amd import ops
    legs = {"host": lambda: host_stage(g, masks, area, nms_thresh)}
    if hasattr(ops, "small_regions_select"):
        legs["device"] = lambda: device_stage(masks, area, nms_thresh)
        a, b = legs["host"](), legs["device"]()
        assert np.array_equal(a[0], b[0]) and torch.equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    else:
        legs = {"parent": legs["host"]}
    return legs


def stage(a, dev):
    from protosam_amd.segment_anything import SamAutomaticMaskGenerator
    g = SamAutomaticMaskGenerator.__new__(SamAutomaticMaskGenerator)      # (`_remove_small_regions` needs no model)
    for case in a.stage_cases.split(","):
        m, S = (int(v) for v in case.split("x"))
        masks = synthetic_masks(m, S, dev, seed=m + S)
        legs = _stage_legs(g, masks, 100, 0.7)
        t = _alternate(legs, a.reps)
        row = dict(stage="stage_alone", masks=m, size=[S, S], area_thresh=100, kept=len(next(iter(legs.values()))()[0]))
        for k, fn in legs.items():
            row[k + "_ms"] = t[k]
            row[k + "_ms_per_mask"] = round(t[k][0] / m, 4)
            row[k + "_host_syncs"] = _syncs(fn)
        print(json.dumps(row), flush=True)
        del masks
        torch.cuda.empty_cache()


def _image(h, w, seed):
    g = np.random.RandomState(seed)
    coarse = torch.from_numpy(g.rand(1, 3, h // 32 + 2, w // 32 + 2).astype(np.float32))
    img = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear")[0].permute(1, 2, 0).numpy() * 255.0
    return np.ascontiguousarray(img.clip(0, 255).astype(np.uint8))


def _generators(sam, **kw):
    """name -> generator: host and device where the checkout has the switch, else the one route it has"""
    from protosam_amd.segment_anything import SamAutomaticMaskGenerator
    if not hasattr(SamAutomaticMaskGenerator(sam, **kw), "amg_regions"):
        return {"parent": SamAutomaticMaskGenerator(sam, **kw)}
    out = {}
    old = os.environ.get("PSAM_AMG_REGIONS")
    for name in ("host", "device"):
        os.environ["PSAM_AMG_REGIONS"] = name
        out[name] = SamAutomaticMaskGenerator(sam, **kw)
    if old is None:
        del os.environ["PSAM_AMG_REGIONS"]
    else:
        os.environ["PSAM_AMG_REGIONS"] = old
    return out


def generate(a, sam):
    from protosam_amd import ops
    from protosam_amd.segment_anything import SamAutomaticMaskGenerator
    image = _image(1024, 1024, 2048)
    cases = [(int(c.split(":")[0]), float(c.split(":")[1]), layers) for c in a.generate_cases.split(",") for layers in (0, 1)]
    for points, nms, layers in cases:
        probe = SamAutomaticMaskGenerator(sam, points_per_side=points)
        probe.generate(image)
        med = float(np.median(probe._iou[:, 1:].cpu().numpy()))
        kw = dict(points_per_side=points, pred_iou_thresh=med if med > 0 else 1e-9, stability_score_thresh=0.0, crop_n_layers=layers,
                  crop_n_points_downscale_factor=2, min_mask_region_area=100, box_nms_thresh=nms)
        gens = _generators(sam, **kw)
        recs = {k: g.generate(image) for k, g in gens.items()}
        first = next(iter(recs.values()))
        for r in recs.values():
            assert [x["area"] for x in r] == [x["area"] for x in first] and [x["bbox"] for x in r] == [x["bbox"] for x in first]
            assert all(np.array_equal(x["segmentation"], y["segmentation"]) for x, y in zip(r, first))
        t = _alternate({k: (lambda g=g: g.generate(image)) for k, g in gens.items()}, a.reps)
        row = dict(stage="generate", size=[1024, 1024], points=points ** 2, box_nms_thresh=nms, crop_n_layers=layers,
                   min_mask_region_area=100, records=len(first),
                   **{k + "_ms": v for k, v in t.items()}, **{k + "_host_syncs": _syncs(lambda g=g: g.generate(image)) for k, g in gens.items()})
        # the masks that enter the stage, taken from the host loop's first argument, and the stage alone on them
        g0 = next(iter(gens.values())) if "host" not in gens else gens["host"]
        seen = []
        inner = g0._remove_small_regions
        g0._remove_small_regions = lambda mk, *x: (seen.append(mk.clone()) if x[1] == "holes" else None, inner(mk, *x))[1]
        g0.generate(image)
        g0._remove_small_regions = inner
        row["masks_into_stage"] = len(seen)
        if seen:
            masks = torch.stack(seen)
            ts = _alternate(_stage_legs(g0, masks, 100, max(g0.box_nms_thresh, g0.crop_nms_thresh)), a.reps)
            for k, v in ts.items():
                row[k + "_stage_ms"] = v
                row[k + "_stage_share"] = round(v[0] / t[k][0], 4)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sam", default="vit_b")
    ap.add_argument("--depth", type=int, default=None)
    ap.add_argument("--points", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stage-cases", default="64x512,256x512,64x1024,256x1024")
    ap.add_argument("--generate-cases", default="32:0.7,16:1.0", help="points per side : box_nms_thresh, comma separated")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--skip-stage", action="store_true")
    ap.add_argument("--skip-generate", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    assert torch.cuda.is_available(), "bench_amg_small_regions.py measures on the GPU; there is no CPU figure"
    dev = torch.device("cuda:0")
    from protosam_amd.sam_wrapper import SamWrapper
    print(json.dumps(dict(sam=a.sam, depth=a.depth, points=a.points ** 2, reps=a.reps, tree=os.path.abspath(a.tree),
                          times="[median, min, max] ms per leg")), flush=True)
    if not a.skip_stage:
        stage(a, dev)
    if not a.skip_generate:
        ck = "random:7" + (f":{a.depth}" if a.depth else "")
        sam = SamWrapper({"model_type": a.sam, "sam_checkpoint": ck, "generator_args": dict(points_per_side=a.points)}).cuda().sam
        generate(a, sam)


if __name__ == "__main__":
    main()
