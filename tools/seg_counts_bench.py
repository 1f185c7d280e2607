"""Times the scoring kernel (`ops.seg_counts`, one launch per call) against what the package offered before it
(`metrics.get_dice_iou_precision_recall` once per (slice, class) plane on the device tensors), and `runner.evaluate_slices_classes`
against `runner.run_slices_classes` on BASELINE config 5's model (tools/config5_batched.py).

  python tools/seg_counts_bench.py [--repeats 3] [--skip-model] [--out profiles/seg_counts_bench.txt]

Every leg is warmed, then timed between two device events in a window that ends in a synchronise; the two variants of a comparison
alternate in one process, `--repeats` windows each. Bytes of a seg_counts call = the mask planes once + the label planes once;
the share of peak is that over the time over the HBM rate of 8.0 TB/s (spec) and 6.29 TB/s (measured copy rate). Fails without a GPU.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def window(fn, calls):
    import torch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-model", action="store_true", help="only the kernel legs")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from protosam_amd import metrics, ops
    if not torch.cuda.is_available():
        raise SystemExit("seg_counts_bench.py measures the GPU: no device found")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for (n, C, S) in ((16, 4, 1024), (32, 4, 512)):
        g = torch.Generator().manual_seed(S)
        label = torch.randint(0, C + 1, (n, S // 8, S // 8), generator=g).to(torch.uint8)
        label = label.repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous().to(dev)                  # blocky organs
        pred = torch.stack([(label == c + 1) ^ (torch.rand((n, S, S), generator=g) < 0.02).to(dev) for c in range(C)], 1)
        pred = pred.to(torch.uint8).contiguous()
        rows = torch.from_numpy(metrics.class_rows(n, list(range(1, C + 1)))).to(dev)
        table = torch.empty((n * C, 12), dtype=torch.int64, device=dev)
        nbytes = pred.numel() + label.numel()

        def new():
            ops.seg_counts(pred, label, rows, out=table)

        def old():
            out = []
            for k in range(n):
                for c in range(C):
                    out.append(metrics.get_dice_iou_precision_recall(pred[k, c].float(), (label[k] == c + 1).float()))
            return out

        new(); old()
        window(new, 20); window(old, 1)
        ref = old()
        sc = metrics.score_slices(table)
        dd = max(abs(float(ref[k]["dice"]) - sc["dice"][i]) for i, k in enumerate(sc["rows"]))
        t_new, t_old = [], []
        for _ in range(args.repeats):
            t_new.append(window(new, 200))
            t_old.append(window(old, 2))
        for r in range(args.repeats):
            say(f"seg_counts {n}x{C} planes {S}x{S} u8/u8 repeat {r}: new {t_new[r] * 1e6:.1f} us/call, per-plane torch loop "
                f"{t_old[r] * 1e6:.1f} us/call")
        tn, to = sorted(t_new)[len(t_new) // 2], sorted(t_old)[len(t_old) // 2]
        say(f"seg_counts {n}x{C} planes {S}x{S}: median {tn * 1e6:.1f} us for {nbytes / 2 ** 20:.0f} MiB = {nbytes / tn / 1e12:.2f} TB/s "
            f"= {100 * nbytes / tn / HBM_SPEC:.0f} % of 8.0 TB/s (spec), {100 * nbytes / tn / HBM_COPY:.0f} % of 6.29 TB/s (copy rate); "
            f"torch loop {to * 1e6:.0f} us -> {to / tn:.0f}x; max |d dice| against it {dd:.1e}")

    if not args.skip_model:
        from protosam_amd.grid_proto_fewshot import FewShotSeg
        from protosam_amd.protomedsam import ProtoMedSAM
        from protosam_amd.protosam import ALPNetWrapper
        from protosam_amd.runner import ALP_CFG, evaluate_slices_classes, run_slices_classes
        from protosam_amd.synth import synth_state_dict
        from protosam_amd.synth_cases import cfg5_inputs
        from config5_batched import slices
        torch.manual_seed(1234)
        alp = FewShotSeg(1024, None, dict(ALP_CFG))
        alp.load_state_dict(synth_state_dict(alp, 1234))
        alp = alp.to(dev).eval()
        model = ProtoMedSAM((1024, 1024), ALPNetWrapper(alp), "random:vit_b:1234", use_cca=True).to(dev).eval()
        s_img, s_masks, q_img = cfg5_inputs()
        s_img, s_masks = s_img.to(dev), [m.to(dev) for m in s_masks]
        N, B, C = 32, 16, len(s_masks)
        vol = slices(q_img, N).to(dev)[:, 0].contiguous()
        labels = torch.zeros((N, 1024, 1024), dtype=torch.uint8, device=dev)
        for c, m in enumerate(s_masks):
            labels[:, m.reshape(1024, 1024) > 0] = c + 1
        sup_imgs, per_part, zs, classes = [s_img] * 3, [s_masks] * 3, list(range(N)), list(range(1, C + 1))
        out = torch.zeros((N, C, 1024, 1024), dtype=torch.uint8, device=dev)

        def run():
            run_slices_classes(model, vol, sup_imgs, per_part, zs, dev, batch=B, out=out)

        def evaluate():
            evaluate_slices_classes(model, vol, labels, sup_imgs, per_part, zs, classes, dev, batch=B)

        run(); evaluate()
        r_run, r_eval = [], []
        for _ in range(args.repeats):
            r_run.append(N / window(run, 1))
            r_eval.append(N / window(evaluate, 1))
        say(f"config 5, {N} slices x {C} classes, {B} per call: run_slices_classes {' / '.join(f'{v:.1f}' for v in r_run)} slices/s, "
            f"evaluate_slices_classes {' / '.join(f'{v:.1f}' for v in r_eval)} slices/s "
            f"(medians {sorted(r_run)[len(r_run) // 2]:.1f} / {sorted(r_eval)[len(r_eval) // 2]:.1f}; spread of the repeats "
            f"{100 * (max(r_run) - min(r_run)) / min(r_run):.1f} % / {100 * (max(r_eval) - min(r_eval)) / min(r_eval):.1f} %)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
