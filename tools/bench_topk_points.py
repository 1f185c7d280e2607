"""Times the device top-k points (psam_topk_points_batch) and what they change in forward_batch (profiles/topk_points_bench.txt).

  python tools/bench_topk_points.py

(a) `ops.topk_points_batch` alone: 16 planes of 1024^2 `blobs` (oracle-free: the generator is restated here), labelled by
    ops.ccl_batch, for k = 3, 16, 251 with and without only_best. Clock: HIP events around `iters` back-to-back calls on the
    current stream, divided by `iters`. The six configurations take turns inside every repeat.
(b) `ProtoSAM.forward_batch`, B = 16, SAM ViT-B with synthetic weights (full depth), num_points_for_sam = 8, use_bbox=True,
    given coarse logits (a smooth field with several blobs per slice, rolled per slice; the coarse model is not part of either
    leg). One leg is PSAM_TOPK_POINTS "host" - the default, the code path before the switch existed - the other "device"; the
    same model object, the legs alternate inside every repeat. Clock: time.perf_counter around the call with a device
    synchronisation on both sides.
Every repeat is printed; the summary is the median and the spread (max - min) / median of the repeats.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def blobs(S, seed, thr=0.15):
    """thresholded bilinear upsampling of a coarse Gaussian field -> (mask uint8 [S,S], p_fg fp32 [S,S] in eighths)"""
    import numpy as np
    import torch
    g = np.random.RandomState(seed)
    pfg = (g.randint(0, 9, size=(S, S)) / 8.0).astype(np.float32)
    f = torch.from_numpy(np.random.RandomState(seed).randn(1, 1, S // 64, S // 64).astype(np.float32))
    m = (torch.nn.functional.interpolate(f, size=(S, S), mode="bilinear")[0, 0].numpy() > thr).astype(np.uint8)
    return m, pfg


def summary(name, vals, unit="ms"):
    med = statistics.median(vals)
    print(f"{name}: {' '.join(f'{v:.3f}' for v in vals)} {unit} | median {med:.3f} {unit}, spread {100 * (max(vals) - min(vals)) / med:.1f} %",
          flush=True)
    return med


class FixedCoarse:
    def __init__(self, logits):
        self.logits = logits

    def __call__(self, inp):
        return self.logits.clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--planes", type=int, default=16)
    a = ap.parse_args()
    import numpy as np
    import torch
    from protosam_amd import ops, synth_cases as gi
    from protosam_amd.protosam import InputFactory, ProtoSAM, TYPE_ALPNET
    if not torch.cuda.is_available():
        raise SystemExit("bench_topk_points.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    S, P = 1024, a.planes

    # ---- (a) the kernel chain alone ---------------------------------------------------------------------------------------
    made = [blobs(S, 100 + p) for p in range(P)]
    pred = torch.from_numpy(np.stack([m for m, _ in made])).to(dev)
    prob = torch.from_numpy(np.stack([np.stack([1.0 - p, p]) for _, p in made]).astype(np.float32)).to(dev)
    cw = ops.CclWorkspace(S, S, 256, dev, slots=P)
    ops.ccl_batch(pred, prob, cw)
    ns = [int(t[1]) for t in cw.tabs.cpu().numpy()]
    print(f"(a) topk_points_batch, {P} planes of {S}^2 blobs, {min(ns)}-{max(ns)} components per plane, "
          f"{float(pred.float().mean()) * 100:.1f} % foreground, max_comp 64; HIP events over {a.iters} calls")
    configs = [(k, ob) for k in (3, 16, 251) for ob in (False, True)]
    keys = {c: torch.empty((P, 1 if c[1] else 64, c[0]), dtype=torch.int64, device=dev) for c in configs}

    def run(c):
        ops.topk_points_batch(cw.labels_b[:P], prob[:, 1], cw.tabs[:P], c[0], 64, only_best=c[1], keys=keys[c])

    for c in configs:                                           # warm-up: code objects, the scratch of each shape
        run(c); run(c)
    torch.cuda.synchronize()
    times = {c: [] for c in configs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.repeats):
        for c in configs:
            e0.record()
            for _ in range(a.iters):
                run(c)
            e1.record()
            e1.synchronize()
            times[c].append(e0.elapsed_time(e1) / a.iters)
    for c in configs:
        summary(f"  k = {c[0]:3d}, only_best = {int(c[1])}", times[c])

    # ---- (b) forward_batch, host leg against device leg ---------------------------------------------------------------------
    B, k = 16, 8
    logits = gi.orch_coarse_logits()
    batch_logits = torch.cat([torch.roll(logits, (13 * b, -9 * b), (-2, -1)) for b in range(B)]).to(dev)
    q = gi.orch_query()
    q = torch.cat([torch.roll(q, (13 * b, -9 * b), (-2, -1)) for b in range(B)]).contiguous().to(dev)
    model = ProtoSAM((1024, 1024), FixedCoarse(batch_logits), "random:vit_b", num_points_for_sam=k, use_bbox=True,
                     use_points=True, point_mode="both", use_cca=False, use_sam_trans=True).to(dev).eval()
    inp = InputFactory.create_input(TYPE_ALPNET, q, support_images=[q[:1]], support_labels=[torch.zeros(1, 512, 512)],
                                    isval=True, val_wsize=2)

    def leg(mode):
        model.topk_points = mode
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = model.forward_batch(q, inp)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, res

    for mode in ("host", "device", "host", "device"):           # warm-up of both legs
        _, res = leg(mode)
    n_sets = sum(len(r[1]) for r in res)
    print(f"(b) forward_batch, B = {B}, SAM ViT-B synthetic weights, num_points_for_sam = {k}, use_bbox=True, {n_sets} prompt sets; "
          f"time.perf_counter around the call, synchronised")
    host, device = [], []
    for _ in range(a.repeats):
        host.append(leg("host")[0])
        device.append(leg("device")[0])
    mh = summary("  host   (default)", host)
    md = summary("  device          ", device)
    print(f"  host / device = {mh / md:.3f} ({'device mode is faster' if md < mh else 'device mode is NOT faster'}; "
          f"{mh / B:.2f} -> {md / B:.2f} ms per slice)")


if __name__ == "__main__":
    main()
