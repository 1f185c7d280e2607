"""Times the 3-D connected-component clean-up (ops.volume_regions: label, filter, keep the largest, per class on the device) on the
synthetic 4-class scan of tools/bench_surface_metrics.py, and beside it the route a user had before: download of the kept masks,
scipy.ndimage.label + numpy.bincount per class, upload of the result.

  python tools/bench_volume_regions.py [--size 512] [--slices 32] [--big] [--out FILE]

Cases: the kept masks [Z, 4, S, S] of `four_class_volume(Z, S, 1, island=True)`, cleaned where they lie (layout "zchw",
keep_largest, connectivity 26), without and with the label volume; `--big` adds 64 x 4 x 1024 x 1024 if its scratch fits the device.
Device times are HIP events around work already warmed up, the median of 7 (min .. max beside it). The time per stage is the sum
of each kernel's durations over one call, from one torch.profiler trace of a call of its own (not the timed ones). Peak scratch is
torch.cuda.max_memory_allocated over a call minus what was allocated before it. Bytes: what every pass has to move if each array
is read or written once per pass - init 1 + 8, merge 4, flatten + sizes 4 + 4 per set voxel, roots 4, rewrite 4 + 1 + 4 per set
voxel (26 bytes per voxel + 8 per set voxel; with labels the ranks read 4 and the rewrite writes 4 + reads 4 per set voxel more) -
divided by the chain time, against the HBM peak DESIGN.md quotes (8.0 TB/s)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK = 8.0e12                 # bytes / s
STAGES = ("vr_clear", "vr_init", "vr_merge", "vr_flatten_size", "vr_roots", "vr_scan", "vr_rank", "vr_rewrite", "vr_finalize")


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


def stage_times(fn):
    """microseconds per stage of one call, from one profiler trace; None where the profiler gives no kernel records"""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            for s in STAGES:
                if ev.name.startswith(s + "_kernel") or (s + "_kernel") in ev.name:
                    out[s] = out.get(s, 0.0) + float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0))
        return out or None
    except Exception as e:        # noqa: BLE001  (a missing tracer must not lose the timings above)
        print(f"  (no per-stage times: {type(e).__name__}: {e})")
        return None


def host_route(keep, conn_rank, ndi):
    """download, label + bincount + largest per class, upload -> (seconds copy down, seconds compute, seconds copy up, cleaned)"""
    import numpy as np
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = keep.cpu().numpy()
    t1 = time.perf_counter()
    st = ndi.generate_binary_structure(3, conn_rank)
    out = np.zeros_like(host)
    comps = []
    for c in range(host.shape[1]):
        lab, n = ndi.label(host[:, c] != 0, structure=st)
        comps.append(n)
        if n:
            sizes = np.bincount(lab.reshape(-1), minlength=n + 1)[1:]
            out[:, c] = lab == 1 + int(np.argmax(sizes))
    t2 = time.perf_counter()
    dev = torch.from_numpy(out).to(keep.device)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return t1 - t0, t2 - t1, t3 - t2, dev, comps


def run_case(name, keep, say, ndi, host=True):
    import torch
    from protosam_amd import ops
    Z, C, S, _ = keep.shape
    n = Z * S * S
    out = torch.empty_like(keep)
    chunk = ops.volume_regions_chunk(C, Z, S, S)
    say(f"[{name}] kept masks {Z} x {C} x {S} x {S} uint8 ({keep.numel() / 1e6:.1f} MB), connectivity 26, keep_largest, "
        f"{chunk} volume(s) in flight")
    set_voxels = int((keep != 0).sum())
    for with_labels in (False, True):
        lab = torch.empty((C, Z, S, S), dtype=torch.int32, device=keep.device) if with_labels else False
        fn = lambda: ops.volume_regions(keep, 26, 0, True, labels=lab, out=out, layout="zchw")     # noqa: E731
        fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        info = fn()[1]
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        scratch = ops.volume_regions_workspace(Z, S, S, chunk, labels=with_labels)
        med, lo, hi = device_times(fn)
        table = ops.volume_regions_table(info)
        nbytes = 26 * n * C + 8 * set_voxels + (8 * n * C + 4 * set_voxels if with_labels else 0)
        say(f"  {'with labels' if with_labels else 'no labels  '}: chain {med:8.3f} ms (min {lo:.3f} .. max {hi:.3f}), scratch "
            f"{scratch / 2**20:.1f} MiB held between calls (+ {peak / 2**20:.1f} MiB allocated during one), must-move "
            f"{nbytes / 1e6:.0f} MB -> {nbytes / (med * 1e-3) / 1e12:.3f} TB/s = {100 * nbytes / (med * 1e-3) / HBM_PEAK:.1f} % of "
            f"{HBM_PEAK / 1e12:.1f} TB/s")
        st = stage_times(fn)
        if st:
            tot = sum(st.values())
            say("    stages (us, one call): " + ", ".join(f"{s[3:]} {st[s]:.0f}" for s in STAGES if s in st) +
                f"; sum {tot:.0f} of {med * 1e3:.0f}")
        else:
            say("    stages: not measured (no kernel records from the profiler)")
    say(f"  components per class {[t['components'] for t in table]}, voxels in {[t['voxels_in'] for t in table]}, dropped "
        f"{[t['voxels_dropped'] for t in table]}, largest {[t['largest_size'] for t in table]}")
    if ndi is None or not host:
        say("  host route (download, scipy.ndimage.label + bincount per class, upload): not measured" +
            (" (scipy is not installed here)" if ndi is None else ""))
        return
    down, comp, up, ref, comps = host_route(keep, 3, ndi)
    same = bool(torch.equal(ref, out))
    say(f"  host route: download {down * 1e3:.1f} ms + label / bincount / select {comp * 1e3:.1f} ms + upload {up * 1e3:.1f} ms = "
        f"{(down + comp + up) * 1e3:.1f} ms (one run); components {comps}; result equal to the device's: {same}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--slices", type=int, default=32)
    ap.add_argument("--big", action="store_true", help="also 64 x 4 x 1024 x 1024, if the scratch fits")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    import torch
    from bench_surface_metrics import four_class_volume
    from protosam_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_volume_regions.py times the GPU chain: no device found")
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"volume regions on {torch.cuda.get_device_name(0)}; synthetic 4-class scans with a stray island on class 1")
    keep = torch.from_numpy(four_class_volume(args.slices, args.size, 1, shift=(5, -7), island=True)).to(dev)
    run_case("scan", keep, say, ndi)
    if args.big:
        Z, S = 64, 1024
        need = ops.volume_regions_workspace(Z, S, S, ops.volume_regions_chunk(4, Z, S, S), labels=True) + 6 * 4 * Z * S * S
        free = torch.cuda.mem_get_info()[0]
        if need > free:
            say(f"[big] 64 x 4 x 1024 x 1024: not measured, {need / 2**30:.1f} GiB needed and {free / 2**30:.1f} GiB free")
        else:
            del keep
            keep = torch.from_numpy(four_class_volume(Z, S, 1, shift=(5, -7), island=True)).to(dev)
            run_case("big", keep, say, ndi)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
