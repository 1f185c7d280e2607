"""Times the surface-distance chain (ops.surface_distances: HD, HD95, ASSD on the device) on the project's synthetic volumes, and
beside it the route a user had before: download of the kept masks and a host distance transform per row.

  python tools/bench_surface_metrics.py [--size 512] [--batch 16] [--slices 32] [--out FILE]

Cases (4 classes: the synthetic organ of `synth_volume` and three ellipses whose cross-section follows it; the "prediction" is the
same construction from the next seed, moved by a few pixels, with a stray island on class 1):
  slices  one batch of `--batch` slices x 4 classes at size^2, a row per (slice, class), depth 1
  scan    the whole scan of `--slices` slices, one 3-D row per class
Device times are HIP events around work already warmed up, the median of 7: the whole chain, and each stage on its own (points =
count + scan + fill, dist, sort = torch.sort of the keys, stats). Pairs = sum over rows of 2 |S(P)| |S(G)| from the counts the
kernels report; a pair costs 8 (depth 1) or 12 (3-D) separately rounded fp32 operations (no FMA by definition), so the bound named
beside the rate is half the fp32 vector peak of MI355X_MICROARCH (157.3 TFLOP/s counts an FMA as two). Peak workspace is
torch.cuda.max_memory_allocated over the chain minus what was allocated before it.
The host route: `.cpu()` of masks and labels, then per row scipy's binary_erosion and distance_transform_edt(sampling=) in both
directions, numpy.percentile and the means; where scipy is missing, tests/surface_reference.py on a case cut down (stated)."""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP32_VECTOR_PEAK = 157.3e12       # FLOP/s, an FMA counted as two (MI355X_MICROARCH.md, chip-level parameters)


def four_class_volume(Z, S, seed, shift=(0, 0), island=False):
    """uint8 masks [Z, 4, S, S]: class 0 the organ of synth_volume(seed), classes 1..3 ellipses scaled with z like it"""
    import numpy as np
    from protosam_amd.synth import MULTI_ORGANS, ellipse_mask, synth_volume
    _, lab = synth_volume(Z, S, seed=seed)
    out = np.zeros((Z, 4, S, S), dtype=np.uint8)
    out[:, 0] = lab.numpy() > 0
    for z in range(Z):
        t = (z + 0.5) / Z
        r = math.sqrt(max(1e-3, 1.0 - (2 * t - 1) ** 2 * 0.8))
        for c, (cy, cx, ry, rx, _) in enumerate(MULTI_ORGANS[1:]):
            out[z, 1 + c] = ellipse_mask(S, cy + 0.01 * seed, cx, 0.8 * ry * r, 0.8 * rx * r) > 0
    out[:, 1:] &= (out[:, :1] == 0)
    if island and Z > 2:
        out[Z // 2, 0, S // 16:S // 16 + 6, S - S // 8:S - S // 8 + 9] = 1           # a stray component far from the organ
    return np.roll(out, shift, axis=(2, 3))


def device_times(fn, reps=7):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def host_route(pred_dev, label_dev, rows, spacing, ndi):
    """what a user ran before: masks to the host, then a distance transform per row and direction -> (seconds for the copy, seconds
    for the computation, table [n, 8])"""
    import numpy as np
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pred = pred_dev.cpu().numpy().reshape((-1,) + tuple(pred_dev.shape[-2:]))
    label = label_dev.cpu().numpy()
    t1 = time.perf_counter()
    table = np.full((len(rows), 8), np.nan)
    for k, (pp, pv, lp, lv, D) in enumerate(rows):
        P, G = pred[pp:pp + D] == pv, label[lp:lp + D] == lv
        if D == 1:
            P, G, samp = P[0], G[0], spacing[1:]
        else:
            samp = spacing
        cross = ndi.generate_binary_structure(P.ndim, 1)
        sp, sg = P ^ ndi.binary_erosion(P, cross), G ^ ndi.binary_erosion(G, cross)
        table[k, 0], table[k, 1], table[k, 7] = sp.sum(), sg.sum(), 0
        if table[k, 0] == 0 or table[k, 1] == 0:
            continue
        a = ndi.distance_transform_edt(~sg, sampling=samp)[sp]
        b = ndi.distance_transform_edt(~sp, sampling=samp)[sg]
        table[k, 2:7] = (max(a.max(), b.max()), np.percentile(np.concatenate([a, b]), 95), (a.mean() + b.mean()) / 2, a.mean(), b.mean())
    return t1 - t0, time.perf_counter() - t1, table


def reference_route(pred_dev, label_dev, rows, spacing):
    """without scipy: tests/surface_reference.py (all pairs in numpy) on the rows given"""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import surface_reference as sr
    t0 = time.perf_counter()
    pred = pred_dev.cpu().numpy().reshape((-1,) + tuple(pred_dev.shape[-2:]))
    label = label_dev.cpu().numpy()
    t1 = time.perf_counter()
    table = np.stack([sr.reference(pred[pp:pp + D] == pv, label[lp:lp + D] == lv, spacing)["row"] for pp, pv, lp, lv, D in rows])
    return t1 - t0, time.perf_counter() - t1, table


def run_case(name, pred, label, rows, spacing, say, ndi):
    import numpy as np
    import torch
    from protosam_amd import ops
    depth = max(r[4] for r in rows)
    covered = sum(r[4] for r in rows) * pred.shape[-2] * pred.shape[-1]
    cap = ops.surface_default_cap(covered)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    table = ops.surface_distances(pred, label, rows, spacing)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    host = table.cpu().numpy()
    assert (host[:, 7] == 0).all(), "a row overflowed the default pool"
    pairs = float((2 * host[:, 0] * host[:, 1]).sum())
    ops_per_pair = 12 if depth > 1 else 8
    say(f"== {name}: {len(rows)} rows of depth {depth} at {pred.shape[-2]} x {pred.shape[-1]}, spacing {spacing}")
    say(f"   surface voxels {int(host[:, :2].sum())} (largest row {int(host[:, :2].sum(axis=1).max())}), default pool {cap} points, "
        f"pairs {pairs:.4g}")
    whole = device_times(lambda: ops.surface_distances(pred, label, rows, spacing))
    work = ops.surface_points(pred, label, rows, cap)
    ops.surface_dist(work, spacing, keys=True)
    sorted_keys = torch.sort(work["keys"])[0]
    stages = {"points": device_times(lambda: ops.surface_points(pred, label, rows, cap)),
              "dist": device_times(lambda: ops.surface_dist(work, spacing, keys=True)),
              "sort": device_times(lambda: torch.sort(work["keys"])),
              "stats": device_times(lambda: ops.surface_stats(sorted_keys, work))}
    say(f"   device chain    {whole[0]:9.3f} ms (median of 7; min {whole[1]:.3f}, max {whole[2]:.3f})")
    for stage, t in stages.items():
        say(f"     {stage:<7}       {t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})")
    rate = pairs / (stages["dist"][0] * 1e-3)
    say(f"   psam_surface_dist: {rate:.4g} pairs/s = {rate * ops_per_pair / 1e12:.2f} T fp32 operations/s at {ops_per_pair} per pair; "
        f"the bound is {FP32_VECTOR_PEAK / 2e12:.1f} T non-FMA operations/s (half the {FP32_VECTOR_PEAK / 1e12:.1f} TFLOP/s vector peak): "
        f"{100 * rate * ops_per_pair / (FP32_VECTOR_PEAK / 2):.1f} % (the dist stage also fills d2 and the keys: two torch fills)")
    say(f"   peak workspace  {peak / 2 ** 20:9.1f} MiB (ops.surface_workspace: {ops.surface_workspace(len(rows), cap) / 2 ** 20:.1f} MiB + the sort's temporaries)")
    if ndi is not None:
        copy_s, comp_s, ref = host_route(pred, label, rows, spacing, ndi)
        what = "scipy binary_erosion + distance_transform_edt"
        sub = list(range(len(rows)))
    else:
        sub = list(range(min(len(rows), 4))) if depth == 1 else []
        what = f"tests/surface_reference.py on {len(sub)} of {len(rows)} rows (no scipy on this machine; cut down)"
        if not sub:
            say("   host route: not measured (no scipy, and the numpy all-pairs reference does not finish a scan in seconds)")
            return
        copy_s, comp_s, ref = reference_route(pred, label, [rows[k] for k in sub], spacing)
    say(f"   host route      {1e3 * (copy_s + comp_s):9.1f} ms = download {1e3 * copy_s:.1f} ms + {what} {1e3 * comp_s:.1f} ms")
    if len(sub) == len(rows):
        say(f"   ratio host / device: {1e3 * (copy_s + comp_s) / whole[0]:.1f}")
    ok = np.isfinite(ref[:, 2])
    rel = np.abs(host[sub][ok][:, 2:7] - ref[ok][:, 2:7]) / np.maximum(np.abs(ref[ok][:, 2:7]), 1e-30)
    assert np.array_equal(host[sub][:, :2], ref[:, :2]), "surface sizes differ from the host route"
    say(f"   largest relative difference to the host route over hd, hd95, assd, asd: {float(rel.max()) if rel.size else 0.0:.2e}")
    say(f"   mean hd {np.nanmean(host[:, 2]):.3f}, hd95 {np.nanmean(host[:, 3]):.3f}, assd {np.nanmean(host[:, 4]):.3f} "
        f"({int(np.isfinite(host[:, 2]).sum())} rows with both surfaces)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--slices", type=int, default=32)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    import torch
    from protosam_amd.metrics import surface_rows
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface_metrics.py times the GPU chain: no device found")
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    S, Z, B = args.size, args.slices, min(args.batch, args.slices)
    spacing = (2.5, 0.78125, 0.78125)
    gt = four_class_volume(Z, S, 0)
    label = torch.from_numpy((gt * (1 + torch.arange(4).numpy())[None, :, None, None]).sum(axis=1).astype("uint8")).to(dev)
    pred = torch.from_numpy(four_class_volume(Z, S, 1, shift=(5, -7), island=True)).to(dev)
    say(f"surface metrics on {torch.cuda.get_device_name(0)}; synthetic scan {Z} x {S} x {S}, 4 classes")
    z0 = (Z - B) // 2                                                # the middle of the scan, where the organs are largest
    run_case("slices", pred[z0:z0 + B], label, surface_rows(B, [1, 2, 3, 4], label_planes=list(range(z0, z0 + B))).tolist(), spacing,
             say, ndi)
    vol = pred.permute(1, 0, 2, 3).contiguous()
    run_case("scan", vol, label, surface_rows(1, [1, 2, 3, 4], depth=Z).tolist(), spacing, say, ndi)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
