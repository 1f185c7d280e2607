"""BASELINE config 5 (DINOv2 ViT-B/14 at 1022^2 + a 4-class prototype bank + MedSAM ViT-B, 1024x1024 slices, full depth, seed 1234)
one slice per call (`ProtoMedSAM.forward_classes`, what bench.py's config5 leg times) against many slices per call
(`ProtoMedSAM.forward_classes_batch`), in one process on the same 32 distinct slices.

  python tools/config5_batched.py [--batches 8 16 32] [--repeats 3] [--out results/config5_batched.json]
  python tools/config5_batched.py --only-batched 16          (one batched leg only: the command to run under rocprofv3)

Slices: small rolls and mirror images of synth_cases.cfg5_inputs()'s query (every organ stays in the slice), so no call sees the
query of the previous one. Every shape is run once before timing; each timed pass is all 32 slices, between two device events,
ending in a synchronise; the legs alternate, `--repeats` passes each. Then the batched results are compared with the per-slice ones
on the same inputs: max |d sigmoid(low_res)|, max |d conf| and the number of differing mask pixels.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def slices(q, n):
    """n distinct variants of q [1,3,S,S]: rolls by up to 21 px and their mirror images"""
    import torch
    out = []
    for i in range(n):
        dy, dx = (i * 7) % 43 - 21, (i * 11) % 37 - 18
        v = torch.roll(q, (dy, dx), (-2, -1))
        out.append(torch.flip(v, (-1,)) if i % 2 else v)
    return torch.cat(out).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=32)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 16, 32])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only-batched", type=int, default=0, help="time forward_classes_batch at this B only (for a kernel trace)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from protosam_amd.grid_proto_fewshot import FewShotSeg
    from protosam_amd.protomedsam import ProtoMedSAM
    from protosam_amd.protosam import ALPNetWrapper
    from protosam_amd.runner import ALP_CFG
    from protosam_amd.synth import synth_state_dict
    from protosam_amd.synth_cases import cfg5_inputs
    if not torch.cuda.is_available():
        raise SystemExit("config5_batched.py measures the GPU: no device found")
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    alp = FewShotSeg(1024, None, dict(ALP_CFG))
    alp.load_state_dict(synth_state_dict(alp, 1234))
    alp = alp.to(dev).eval()
    model = ProtoMedSAM((1024, 1024), ALPNetWrapper(alp), "random:vit_b:1234", use_cca=True).to(dev).eval()
    s_img, s_masks, q_img = cfg5_inputs()
    s_img, s_masks = s_img.to(dev), [m.to(dev) for m in s_masks]
    N = args.slices
    qs = slices(q_img, N).to(dev)

    def per_slice():
        return [model.forward_classes(qs[i:i + 1], s_img, s_masks) for i in range(N)]

    def batched(B):
        out = []
        for i in range(0, N, B):
            out += model.forward_classes_batch(qs[i:i + B], s_img, s_masks)
        return out

    legs = [(f"batched B={args.only_batched}", lambda: batched(args.only_batched))] if args.only_batched else \
        [("per-slice", per_slice)] + [(f"batched B={B}", (lambda B=B: batched(B))) for B in args.batches]
    t0 = time.time()
    for _, fn in legs:                                       # warm every shape (and the support-bank cache)
        fn()
    torch.cuda.synchronize()
    print(f"warm-up {time.time() - t0:.1f} s")
    rates = {name: [] for name, _ in legs}
    peak = {}
    for r in range(args.repeats):
        for name, fn in legs:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            rates[name].append(N / (e0.elapsed_time(e1) / 1e3))
            hi = torch.cuda.max_memory_allocated(dev)
            old = peak.get(name, (0, 0))
            peak[name] = (max(old[0], hi - base), max(old[1], hi))
    result = dict(slices=N, classes=len(s_masks), repeats=args.repeats, legs={})
    for name, _ in legs:
        v = sorted(rates[name])
        result["legs"][name] = dict(slices_per_s=v, median=v[len(v) // 2], transient_mib=peak[name][0] / 2 ** 20,
                                    peak_allocated_mib=peak[name][1] / 2 ** 20)
        print(f"{name:>14}: {v[len(v) // 2]:7.1f} slices/s (min {v[0]:.1f}, max {v[-1]:.1f}), peak allocated "
              f"{peak[name][1] / 2 ** 20:.0f} MiB ({peak[name][0] / 2 ** 20:.0f} MiB above the warmed-up state)")
    if not args.only_batched:
        ref = result["legs"]["per-slice"]["median"]
        for B in args.batches:
            result["legs"][f"batched B={B}"]["speedup"] = result["legs"][f"batched B={B}"]["median"] / ref
            print(f"batched B={B}: {result['legs'][f'batched B={B}']['speedup']:.2f}x the per-slice rate")
        # batched vs per-slice on the same inputs
        lows, confs, segs = [], [], []
        for i in range(N):
            r1 = model.forward_classes(qs[i:i + 1], s_img, s_masks)
            lows.append(model.last_stats.get("low_res").clone() if model.last_stats.get("low_res") is not None else None)
            confs.append([c for _, c in r1])
            segs.append([m.to(torch.uint8).clone() for m, _ in r1])
        comp = {}
        for B in args.batches:
            dp = dc = 0.0
            dpx = 0
            n_cls = []
            for i0 in range(0, N, B):
                res = model.forward_classes_batch(qs[i0:i0 + B], s_img, s_masks)
                st = model.last_stats
                for b in range(len(res)):
                    i, k1 = i0 + b, 0
                    n_cls.append(sum(1 for c in range(len(s_masks)) if (b, c) in st["prompt"]))
                    for c in range(len(s_masks)):
                        dpx = max(dpx, int((res[b][c][0].to(torch.uint8) != segs[i][c]).sum()))
                        if (b, c) not in st["prompt"]:
                            continue
                        k = st["prompt"][(b, c)]
                        dp = max(dp, (torch.sigmoid(st["low_res"][k, 0]) - torch.sigmoid(lows[i][k1, 0])).abs().max().item())
                        dc = max(dc, float(np.abs(np.asarray(res[b][c][1][0]) - np.asarray(confs[i][c][0])).max()))
                        k1 += 1
            comp[B] = dict(max_dsigmoid_low_res=dp, max_dconf=dc, max_differing_px=dpx, min_classes_with_component=min(n_cls))
            print(f"batched B={B} vs per-slice on the same {N} slices: max |d sigmoid(low_res)| {dp:.2e}, max |d conf| {dc:.2e}, "
                  f"max differing px {dpx}, classes with a component per slice >= {min(n_cls)}")
        result["vs_per_slice"] = comp
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
