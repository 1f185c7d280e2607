"""A/B of the two MFMA shapes of the 256x256x64 assembly tile: tile 15 (v_mfma_f32_32x32x16_f16) against tile 17 (16x16x32), on the
eight Linear layers of the two encoders as the pipeline runs them at 32 slices (folded-LayerNorm consumers / producers):
  SAM ViT-H, M = 131072 : qkv (fp16 + LN consumer), fc1 (GELU + LN consumer), proj and fc2 (fp32 residual + LN producer)
  DINOv2-B,  M = 41504  : the same four
Random data, both tiles alternating in one process on one device, ROUNDS rounds each; per shape: wall TFLOP/s median (min-max) of
both and whether tile 17's median beats tile 15's by more than the min-max spread of tile 15's rounds (the rule csrc/gemm.hip
mfma16_auto is written from).
  python tools/gemm_mfma_ab.py [rounds] [plain]         -> the table (stdout); "plain": the same shapes without the LayerNorm fold
Each shape warms both tiles up (20 calls each, not measured) before its first round.
With a library built with GENFLAGS=--trace and PSAM_GEMM_ASM_TRACE=1 it instead runs the plain (not LayerNorm-folded) forms of the
same shapes once per tile on the traced variant 1: cycles per K-tile and per epilogue on stderr. A candidate build is compared as a
second library: one run per library, PSAM_LIB_PATH naming it."""
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from protosam_amd import ops

dev = torch.device("cuda:0")
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
TRACE = os.environ.get("PSAM_GEMM_ASM_TRACE") is not None
PLAIN = "plain" in sys.argv[2:]
SHAPES = []
for model, M, D in (("SAM-H", 131072, 1280), ("DINOv2-B", 41504, 768)):
    SHAPES += [(model, "qkv", M, 3 * D, D, 0), (model, "fc1", M, 4 * D, D, 1), (model, "proj", M, D, D, 2), (model, "fc2", M, D, 4 * D, 2)]


def timeit(fn, n, w):
    for _ in range(w):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3


def make_call(M, N, K, epi, fold):
    a = torch.randn(M, K, device=dev).half()
    w = (torch.randn(N, K, device=dev) * 0.05).half()
    bias = torch.randn(N, device=dev)
    if epi == 2:
        x = torch.randn(M, N, device=dev)
        gamma = torch.rand(N, device=dev) + 0.5
        if not fold:
            return lambda: ops.gemm(a, w, bias, out=x, epilogue=ops.EPI_F32, resid=x, gamma=gamma)
        x16 = torch.empty(M, N, device=dev, dtype=torch.float16)
        stats = torch.empty(M, N // 64, 2, device=dev)
        return lambda: ops.gemm(a, w, bias, out=x, epilogue=ops.EPI_F32, resid=x, gamma=gamma, out16=x16, stats=stats)
    e = (ops.EPI_F16, ops.EPI_GELU_F16)[epi]
    out = torch.empty(M, N, device=dev, dtype=torch.float16)
    if not fold:
        return lambda: ops.gemm(a, w, bias, out=out, epilogue=e)
    # consumer: (mean, rstd) of a random fp32 x whose fp16 copy is `a`, LayerNorm-folded weights
    xg = a.float().view(M, K // 64, 64)
    stats = torch.stack([xg.sum(2), (xg * xg).sum(2)], 2).contiguous()
    mr = ops.ln_finalize(stats, M, K, 1e-6)
    wf, s_ext, t = ops.fold_layernorm(torch.randn(N, K, device=dev) * 0.05, bias, torch.rand(K, device=dev) + 0.5, torch.randn(K, device=dev) * 0.1)
    return lambda: ops.gemm(a, wf, t, out=out, epilogue=e, ln_mr=mr, ln_s=s_ext)


print(f"# tile 15 (32x32x16) against tile 17 (16x16x32), {ROUNDS} alternating rounds, wall TFLOP/s: median (min-max)")
for model, name, M, N, K, epi in SHAPES:
    fn = make_call(M, N, K, epi, not (TRACE or PLAIN))
    flop = 2.0 * M * N * K
    res = {15: [], 17: []}
    try:
        if TRACE:
            os.environ["PSAM_TRACE_QUIET"] = "1"
            ops.gemm_asm_variant(1)
        for tile in (() if TRACE else (15, 17)):
            ops.gemm_set_tile(tile)
            timeit(fn, 20, 0)
        for rnd in range(1 if TRACE else ROUNDS):
            for tile in (15, 17):
                ops.gemm_set_tile(tile)
                t = timeit(fn, 1 if TRACE else 20, 1 if TRACE else 3)
                assert ops.gemm_last_tile() == tile, (ops.gemm_last_tile(), tile)
                res[tile].append(flop / t / 1e12)
    finally:
        ops.gemm_set_tile(0)
        ops.gemm_asm_variant(0)
    if TRACE:
        continue
    m15, m17 = statistics.median(res[15]), statistics.median(res[17])
    spread = max(res[15]) - min(res[15])
    verdict = "17 wins" if m17 - m15 > spread else "15 stays"
    kind = (("fp16", "GELU", "fp32 residual") if PLAIN else ("fp16 + LN consumer", "GELU + LN consumer", "fp32 residual + LN producer"))[epi]
    print(f"{model:9s} {name:4s} {M}x{N}x{K} {kind:28s} t15 {m15:6.0f} ({min(res[15]):.0f}-{max(res[15]):.0f})  t17 {m17:6.0f} ({min(res[17]):.0f}-{max(res[17]):.0f})  "
          f"ratio {m17 / m15:.3f}  {verdict}", flush=True)
    del fn
    torch.cuda.empty_cache()
