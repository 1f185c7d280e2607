"""Times one MaskDecoder.predict_masks_tokens call by the number of tokens per prompt set (profiles/decoder_many_tokens_bench.txt).

  python tools/bench_decoder_tokens.py                  (1 and 27 prompt sets at T = 9, 16, 17, 32, 64, 128, Nk = 4096; medians)
  PSAM_T2I_ALL=0 python tools/bench_decoder_tokens.py --tokens 32      (the one-workgroup-per-token token-to-image kernel, for A/B:
                                                        the switch is read once per process)
  python tools/bench_decoder_tokens.py --launches-only  (a few calls per shape: the program to put under a kernel trace)

Up to 16 tokens the decoder runs the launches it ran before the token kernels (psam_small_attention, one token group): T = 9 and 16
are the figures to hold against the parent commit. Past 16, psam_token_attention and ceil(T / 16) token groups of the token-to-image
kernel take over; only the token side grows with T, so time(32) <= 2 time(16) and time(17) <= time(32) are expected.
With PSAM_T2I_ALL=0 the decoder's K / V projections are written token-major (the round-1 kernel reads nothing else), no key split.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, iters):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--tokens", type=int, nargs="*", default=[9, 16, 17, 32, 64, 128])
    ap.add_argument("--sets", type=int, nargs="*", default=[1, 27])
    ap.add_argument("--launches-only", action="store_true")
    a = ap.parse_args()
    import torch
    from protosam_amd.segment_anything.modeling import transformer as tr
    from protosam_amd.segment_anything.modeling.mask_decoder import MaskDecoder
    from protosam_amd.synth import synth_state_dict
    if not torch.cuda.is_available():
        raise SystemExit("bench_decoder_tokens.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    round1 = os.environ.get("PSAM_T2I_ALL", "1") == "0"
    if round1:          # the round-1 kernel: token-major K / V, one key range (what `_Run` chose past 16 tokens before the token groups)
        init = tr._Run.__init__

        def plain(self, *args, **kw):
            init(self, *args, **kw)
            self.hm, self.t2i_s = False, 1
        tr._Run.__init__ = plain
    md = MaskDecoder(transformer_dim=256, transformer=tr.TwoWayTransformer(depth=2, embedding_dim=256, mlp_dim=2048, num_heads=8))
    md.load_state_dict(synth_state_dict(md, 1234), strict=True)
    md = md.to(dev).eval()
    g = torch.Generator().manual_seed(0)
    Nk = 4096
    feat = torch.randn((Nk, 256), generator=g).to(dev)
    pe = torch.randn((Nk, 256), generator=g).to(dev)
    dense = (torch.randn((256,), generator=g) * 0.5).to(dev)
    print(f"predict_masks_tokens, Nk = {Nk}, token-to-image kernel: {'round 1 (PSAM_T2I_ALL=0)' if round1 else 'one wave per token'}; "
          f"{a.iters} calls per timing, {a.repeats} timings", flush=True)
    for B in a.sets:
        for T in a.tokens:
            tokens = md.build_tokens(torch.randn((B, T - 5, 256), generator=g).to(dev))

            def call():
                return md.predict_masks_tokens(feat, pe, tokens, dense)
            call()
            if a.launches_only:
                timed(call, 3)
                continue
            timed(call, 3)
            ms = [timed(call, a.iters) for _ in range(a.repeats)]
            med = statistics.median(ms)
            print(f"B={B:3d} T={T:4d}: median {med * 1e3:8.1f} us  (min {min(ms) * 1e3:.1f}, max {max(ms) * 1e3:.1f}, spread "
                  f"{100 * (max(ms) - min(ms)) / med:.1f} %)", flush=True)


if __name__ == "__main__":
    main()
