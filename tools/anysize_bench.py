"""Times global rel-pos attention on token maps other than 64 x 64 (`gattn_any_kernel`) beside the 64-wide kernels at equal N^2
work, and the SAM image encoder at 512 pixels against the same model at 1024.

  python tools/anysize_bench.py [--repeats 5] [--skip-encoder] [--out profiles/anysize_bench.txt]

Kernel legs (FLOPs = 4 B H N^2 hd): g = 32, B = 32 (32 x 1024^2) against g = 64, B = 2 (2 x 4096^2), for H = 12 / hd 64 and
H = 16 / hd 80. At g = 64: the DMA-fed HIP kernel (variant 17) and the default dispatch (the assembly kernel), both fed by
`psam_relpos` (timed on its own: the any-size kernel computes those terms itself), and the any-size kernel (variant bit 5).
Encoder legs: images/s of ViT-B and ViT-H `ImageEncoderViT` at 512 and 1024, four images per call, default-initialised weights.
Every leg is warmed, then timed between two device events in a window that ends in a synchronise; the legs of a comparison
alternate in one process, `--repeats` windows each; medians and the spread of the repeats are printed. Fails without a GPU.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


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


def med(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return 100.0 * (max(v) - min(v)) / min(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-encoder", action="store_true", help="only the kernel legs")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from protosam_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("anysize_bench.py measures the GPU: no device found")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def rnd(shape, std, seed):
        return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * std).to(dev)

    for H, hd in ((12, 64), (16, 80)):
        scale = hd ** -0.5
        legs = {}

        def setup(g, B):
            N = g * g
            qkv = rnd((B, N, 3, H, hd), 1.0, g).half()
            rp = ops.pack_rel_tables(rnd((2 * g - 1, hd), 0.3, 1), rnd((2 * g - 1, hd), 0.3, 2), False, hd)
            out = torch.empty((B, N, H * hd), dtype=torch.float16, device=dev)
            return N, qkv, rp, out

        N32, q32, rp32, o32 = setup(32, 32)
        N64, q64, rp64, o64 = setup(64, 2)
        relh = torch.empty((2, H, N64, 64), dtype=torch.float32, device=dev)
        relw = torch.empty_like(relh)
        flops = 4.0 * 32 * H * N32 * N32 * hd
        assert flops == 4.0 * 2 * H * N64 * N64 * hd

        def with_variant(v, fn):
            def run():
                fn()
            run.variant = v
            return run

        legs["any-size g=32 B=32"] = with_variant(5, lambda: ops.attention(q32, 32, N32, H, hd, scale, out=o32, mode=1, rpack=rp32, gh=32, gw=32))
        legs["any-size g=64 B=2"] = with_variant(5 | 32, lambda: ops.attention(q64, 2, N64, H, hd, scale, out=o64, mode=1, rpack=rp64, gh=64, gw=64))
        legs["64-wide HIP (gattn_kernel) g=64 B=2"] = with_variant(
            17, lambda: ops.attention(q64, 2, N64, H, hd, scale, out=o64, mode=1, rel_h=relh, rel_w=relw, gh=64, gw=64))
        legs["64-wide default (assembly) g=64 B=2"] = with_variant(
            5, lambda: ops.attention(q64, 2, N64, H, hd, scale, out=o64, mode=1, rel_h=relh, rel_w=relw, gh=64, gw=64))
        legs["psam_relpos g=64 B=2 (feeds the two 64-wide legs)"] = with_variant(
            5, lambda: ops.relpos(q64, rp64, 2, N64, H, hd, 64, 64, False, scale, rel_h=relh, rel_w=relw))
        times = {k: [] for k in legs}
        ops.relpos(q64, rp64, 2, N64, H, hd, 64, 64, False, scale, rel_h=relh, rel_w=relw)
        try:
            for name, fn in legs.items():           # warm-up
                ops.attention_set_variant(fn.variant)
                window(fn, 10)
            for _ in range(args.repeats):           # alternated repeats
                for name, fn in legs.items():
                    ops.attention_set_variant(fn.variant)
                    times[name].append(window(fn, 50))
        finally:
            ops.attention_set_variant(5)
        for name, t in times.items():
            m = med(t)
            rate = "" if name.startswith("psam_relpos") else f" = {flops / m / 1e12:.1f} TFLOP/s"
            say(f"H={H} hd={hd} {name}: median {m * 1e6:.1f} us{rate} (repeats {' / '.join(f'{v * 1e6:.1f}' for v in t)} us, "
                f"spread {spread(t):.1f} %)")
        a, b = med(times["any-size g=32 B=32"]), med(times["64-wide HIP (gattn_kernel) g=64 B=2"])
        say(f"H={H} hd={hd}: any-size kernel at g=32 runs at {100 * b / a:.0f} % of the 64-wide HIP kernel's rate at equal N^2 work "
            f"({100 * (b + med(times['psam_relpos g=64 B=2 (feeds the two 64-wide legs)'])) / a:.0f} % with that kernel's psam_relpos pass counted)")

    if not args.skip_encoder:
        from protosam_amd.segment_anything import sam_model_registry
        B = 4
        for name in ("vit_b", "vit_h"):
            encs, xs = {}, {}
            for size in (512, 1024):
                encs[size] = sam_model_registry[name](image_size=size).image_encoder.to(dev).eval()
                xs[size] = rnd((B, 3, size, size), 1.0, size)
            rates = {512: [], 1024: []}
            with torch.no_grad():
                for size in (512, 1024):
                    for _ in range(2):
                        encs[size].forward_tokens(xs[size])
                for _ in range(args.repeats):
                    for size in (512, 1024):
                        rates[size].append(B / window(lambda: encs[size].forward_tokens(xs[size]), 3))
            for size in (512, 1024):
                say(f"{name} ImageEncoderViT at {size}: median {med(rates[size]):.1f} images/s, {B} per call "
                    f"(repeats {' / '.join(f'{v:.1f}' for v in rates[size])}, spread {spread(rates[size]):.1f} %)")
            say(f"{name}: 512 over 1024 = {med(rates[512]) / med(rates[1024]):.2f}x images/s")
            del encs, xs
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
