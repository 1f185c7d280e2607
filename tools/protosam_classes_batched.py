"""ProtoSAM over four classes: `forward_batch` once per class (every slice through the SAM encoder four times) against
`forward_classes_batch` (one encoder pass per slice for all classes), in one process on the same 32 distinct slices. Config 4's
model: DINOv2 ViT-B/14 + SAM ViT-H, 512^2 slices, full depth, seed 1234; four classes of synth.synth_pair_multi(512).

  python tools/protosam_classes_batched.py [--batches 16 32] [--repeats 3] [--out results/protosam_classes.json]
  python tools/protosam_classes_batched.py --only-classes 32     (one leg only: the command to run under rocprofv3)

Each timed pass is all 32 slices x 4 classes between two device events, ending in a synchronise, after a warm-up of every shape;
the legs alternate, `--repeats` passes each. Rates are (slice, class) pairs per second. Then both legs are compared on the same
inputs: max |d sigmoid(low_res)|, max |d score| and the number of differing mask pixels.
"""
import argparse
import json
import os
import sys

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
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only-classes", type=int, default=0, help="time forward_classes_batch at this B only (for a kernel trace)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from protosam_amd.protosam import InputFactory, TYPE_ALPNET
    from protosam_amd.runner import build_protosam
    from protosam_amd.synth import synth_pair_multi
    if not torch.cuda.is_available():
        raise SystemExit("protosam_classes_batched.py measures the GPU: no device found")
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    model, _ = build_protosam(dev, "vit_h", 512)
    s_img, s_masks, q_img, _ = synth_pair_multi(512, seed=0)
    s_img, s_masks = s_img.to(dev), [m.to(dev) for m in s_masks]
    N, C = args.slices, len(s_masks)
    qs = slices(q_img, N).to(dev)
    inputs = [InputFactory.create_input(TYPE_ALPNET, qs[:1], support_images=[s_img], support_labels=[m], isval=True, val_wsize=2)
              for m in s_masks]
    for i in inputs:
        i.to(dev)

    def per_class(B, keep=None):
        for i in range(0, N, B):
            for c in range(C):
                r = model.forward_batch(qs[i:i + B], inputs[c])
                if keep is not None:
                    st = model.last_stats
                    spans = st.get("spans") or ([(0, 0, st["n_prompts"])] if st.get("n_prompts") else [])
                    for (b, start, cnt) in spans:
                        keep[(i + b, c)] = (torch.sigmoid(st["low_res"][start:start + cnt, st["sel"]]).clone(),
                                            np.asarray(r[b][1], dtype=np.float64), r[b][0].to(torch.uint8).clone())
                    for b in range(len(r)):
                        keep.setdefault((i + b, c), (None, np.zeros(1), r[b][0].to(torch.uint8).clone()))

    def classes(B, keep=None):
        for i in range(0, N, B):
            r = model.forward_classes_batch(qs[i:i + B], s_img, s_masks)
            if keep is not None:
                st = model.last_stats
                for b in range(len(r)):
                    for c in range(C):
                        low = None
                        if (b, c) in st["spans"]:
                            f, n = st["spans"][(b, c)]
                            low = torch.sigmoid(st["low_res"][f:f + n, st["sel"]]).clone()
                        keep[(i + b, c)] = (low, np.asarray(r[b][c][1], dtype=np.float64), r[b][c][0].clone())

    if args.only_classes:
        legs = [(f"classes B={args.only_classes}", lambda: classes(args.only_classes))]
    else:
        legs = []
        for B in args.batches:
            legs += [(f"per-class B={B}", (lambda B=B: per_class(B))), (f"classes B={B}", (lambda B=B: classes(B)))]
    for _, fn in legs:                                       # warm every shape (and the support-bank caches)
        fn()
    torch.cuda.synchronize()
    rates = {name: [] for name, _ in legs}
    for _ in range(args.repeats):
        for name, fn in legs:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            rates[name].append(N * C / (e0.elapsed_time(e1) / 1e3))
    result = dict(slices=N, classes=C, repeats=args.repeats, legs={})
    for name, _ in legs:
        v = sorted(rates[name])
        result["legs"][name] = dict(pairs_per_s=v, median=v[len(v) // 2])
        print(f"{name:>16}: {v[len(v) // 2]:7.1f} (slice, class) pairs/s (min {v[0]:.1f}, max {v[-1]:.1f})")
    if not args.only_classes:
        comp = {}
        for B in args.batches:
            ratio = result["legs"][f"classes B={B}"]["median"] / result["legs"][f"per-class B={B}"]["median"]
            a, b = {}, {}
            per_class(B, a)
            classes(B, b)
            dp = ds = 0.0
            dpx = 0
            for key, (low_a, sc_a, m_a) in a.items():
                low_b, sc_b, m_b = b[key]
                dpx = max(dpx, int((m_a != m_b).sum()))
                if low_a is None or low_b is None:
                    continue
                dp = max(dp, (low_a - low_b).abs().max().item())
                ds = max(ds, float(np.abs(sc_a - sc_b).max()))
            comp[B] = dict(ratio=ratio, max_dsigmoid_low_res=dp, max_dscore=ds, max_differing_px=dpx)
            print(f"B={B}: forward_classes_batch {ratio:.2f}x forward_batch per class; max |d sigmoid(low_res)| {dp:.2e}, "
                  f"max |d score| {ds:.2e}, max differing px {dpx}")
        result["classes_vs_per_class"] = comp
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
