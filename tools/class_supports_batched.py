"""Multi-class batches with a support set of their own per class and z-part, as the reference evaluates (one 1-way episode per
organ): `forward_batch` once per class with that class's mixed supports (leg 1) against `forward_classes_batch(supports=...)`
(leg 2), in one process on the same synthetic 64-slice volume. Config 4's model (DINOv2 ViT-B/14 + SAM ViT-H, 512^2 slices, full
depth, seed 1234), or config 5's (DINOv2 at 1022^2 + MedSAM ViT-B, 1024^2 slices) with --medsam.

  python tools/class_supports_batched.py [--batch 16] [--repeats 3] [--medsam] [--out results/class_supports.json]
  python tools/class_supports_batched.py --only-new          (leg 2 only: the command to run under rocprofv3 --kernel-trace --stats)

The volume: rolls and mirror images of synth.synth_pair_multi's query, four classes with unequal z-extents (so each class has a part
table of its own, runner.class_part_table), and a 24-slice support scan whose (class, part) support slices come from
runner.class_support_slices; class 1 has two shots per part. Each timed pass is all 64 slices x 4 classes between two device events,
ending in a synchronise, after a warm-up pass of each leg; the legs alternate, `--repeats` passes each, and the median is reported
in (slice, class) pairs per second. Then both legs are compared on the same inputs: max |d sigmoid(low_res)|, max |d score| and the
number of differing mask pixels.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EXTENTS = ((0, 63), (8, 40), (20, 63), (4, 30))      # z range of each class in the query scan
SUP_EXTENTS = ((0, 23), (3, 17), (6, 23), (1, 12))    # ... and in the 24-slice support scan


def volume(img, n):
    """n distinct variants of img [1,3,S,S]: rolls by up to 21 px and their mirror images"""
    import torch
    out = []
    for i in range(n):
        dy, dx = (i * 7) % 43 - 21, (i * 11) % 37 - 18
        v = torch.roll(img, (dy, dx), (-2, -1))
        out.append(torch.flip(v, (-1,)) if i % 2 else v)
    return torch.cat(out).contiguous()


def labels(extents, Z):
    import numpy as np
    lab = np.zeros((Z, 2, 2), dtype=np.int64)
    for c, (lo, hi) in enumerate(extents):
        lab[lo:hi + 1, c // 2, c % 2] = c + 1
    return lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--medsam", action="store_true", help="config 5's model (ProtoMedSAM, 1024^2) instead of config 4's")
    ap.add_argument("--only-new", action="store_true", help="time forward_classes_batch(supports=) only (for a kernel trace)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from protosam_amd.protosam import InputFactory, TYPE_ALPNET
    from protosam_amd.runner import build_protosam, class_part_table, class_support_slices, class_support_specs
    from protosam_amd.synth import synth_pair_multi
    if not torch.cuda.is_available():
        raise SystemExit("class_supports_batched.py measures the GPU: no device found")
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    if args.medsam:
        from protosam_amd.grid_proto_fewshot import FewShotSeg
        from protosam_amd.protomedsam import ProtoMedSAM
        from protosam_amd.protosam import ALPNetWrapper
        from protosam_amd.runner import ALP_CFG
        from protosam_amd.synth import synth_state_dict
        S = 1024
        alp = FewShotSeg(S, None, dict(ALP_CFG))
        alp.load_state_dict(synth_state_dict(alp, 1234))
        model = ProtoMedSAM((1024, 1024), ALPNetWrapper(alp.to(dev).eval()), "random:vit_b:1234", use_cca=True).to(dev).eval()
    else:
        S = 512
        model, _ = build_protosam(dev, "vit_h", S)
    s_img, s_masks, q_img, _ = synth_pair_multi(S, seed=0)
    N, B, C = args.slices, args.batch, len(EXTENTS)
    qs = volume(q_img, N).to(dev)
    part_table = class_part_table(labels(EXTENTS, N), list(range(1, C + 1)))
    sup_z = class_support_slices(labels(SUP_EXTENTS, 24), list(range(1, C + 1)))
    sup_vol = volume(s_img, 24).to(dev)
    sup_lab = [volume(m[None].expand(1, 3, S, S), 24)[:, 0].to(dev) for m in s_masks]

    def inp(c, z):
        zz = [z, (z + 5) % 24] if c == 1 else [z]                            # class 1: two shots
        i = InputFactory.create_input(TYPE_ALPNET, qs[:1], support_images=[sup_vol[k:k + 1] for k in zz],
                                      support_labels=[sup_lab[c][k:k + 1] for k in zz], isval=True, val_wsize=2)
        i.to(dev)
        return i
    supports = [[inp(c, sup_z[c][p]) for p in range(3)] for c in range(C)]
    specs = [class_support_specs(supports, part_table, range(i, min(i + B, N))) for i in range(0, N, B)]

    def keep_batch(keep, i, c, r, low, score_of):
        for b in range(len(r)):
            keep[(i + b, c)] = (low(b), score_of(r[b]), r[b][0].to(torch.uint8).clone())

    def per_class(keep=None):
        for k, i in enumerate(range(0, N, B)):
            for c in range(C):
                r = model.forward_batch(qs[i:i + B], specs[k][c])
                if keep is not None:
                    keep_batch(keep, i, c, r, lambda b: leg1_low(b, len(r)), score)

    def classes(keep=None):
        for k, i in enumerate(range(0, N, B)):
            r = model.forward_classes_batch(qs[i:i + B], supports=specs[k])
            if keep is not None:
                for c in range(C):
                    keep_batch(keep, i, c, [row[c] for row in r], lambda b: leg2_low(b, c), score)

    def score(res):
        return np.asarray([np.asarray(v, dtype=np.float64).ravel()[0] for v in res[1]], dtype=np.float64)

    def leg1_low(b, n):
        st = model.last_stats
        if args.medsam:
            ps = st.get("per_slice", [st])[b] if n > 1 else st
            return None if ps.get("prompt") is None else torch.sigmoid(st["low_res"][ps["prompt"], 0]).clone()
        for (bb, start, cnt) in st.get("spans") or []:
            if bb == b:
                return torch.sigmoid(st["low_res"][start:start + cnt, st["sel"]]).clone()
        return None

    def leg2_low(b, c):
        st = model.last_stats
        if args.medsam:
            k = st["prompt"].get((b, c))
            return None if k is None else torch.sigmoid(st["low_res"][k, 0]).clone()
        if (b, c) not in st["spans"]:
            return None
        f, n = st["spans"][(b, c)]
        return torch.sigmoid(st["low_res"][f:f + n, st["sel"]]).clone()

    legs = [("new: forward_classes_batch(supports=)", classes)]
    if not args.only_new:
        legs = [("forward_batch per class", per_class)] + legs
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
    result = dict(model="config5 (ProtoMedSAM)" if args.medsam else "config4 (ProtoSAM)", slices=N, classes=C, batch=B,
                  repeats=args.repeats, legs={})
    for name, _ in legs:
        v = sorted(rates[name])
        result["legs"][name] = dict(pairs_per_s=v, median=v[len(v) // 2])
        print(f"{name:>40}: {v[len(v) // 2]:7.1f} (slice, class) pairs/s (min {v[0]:.1f}, max {v[-1]:.1f})")
    if not args.only_new:
        a, b = {}, {}
        per_class(a)
        classes(b)
        dp = ds = 0.0
        dpx = 0
        for key, (low_a, sc_a, m_a) in a.items():
            low_b, sc_b, m_b = b[key]
            dpx = max(dpx, int((m_a != m_b).sum()) if m_a.shape == m_b.shape else int(m_a.sum()) + int(m_b.sum()))
            if low_a is None or low_b is None or sc_a.shape != sc_b.shape:
                continue
            dp = max(dp, (low_a - low_b).abs().max().item())
            ds = max(ds, float(np.abs(sc_a - sc_b).max()) if sc_a.size else 0.0)
        ratio = result["legs"]["new: forward_classes_batch(supports=)"]["median"] / result["legs"]["forward_batch per class"]["median"]
        result["new_vs_per_class"] = dict(ratio=ratio, max_dsigmoid_low_res=dp, max_dscore=ds, max_differing_px=dpx)
        print(f"B={B}: new path {ratio:.2f}x forward_batch per class; max |d sigmoid(low_res)| {dp:.2e}, max |d score| {ds:.2e}, "
              f"max differing px {dpx}")
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
