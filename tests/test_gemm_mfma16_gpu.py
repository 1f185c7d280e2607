"""Tile 17 of psam_gemm_f16: the 256x256x64 assembly tile with its k-loop on v_mfma_f32_16x16x32_f16 (csrc/gemm_asm_gen.py sched
"mfma"), forced with gemm_set_tile(17), against float64 on the fp16-rounded operands.

The bound is derived, not tuned (u = 2^-24, the unit roundoff of fp32):
  * accumulation of K products in fp32, in any order:  E_acc = gamma_K * sum_k |a_k w_k|,  gamma_K = K u / (1 - K u);
  * epilogue 0 (bias -> fp16):           E_acc + 2^-11 |y|                    (the fp16 rounding of the result)
  * epilogue 1 (bias -> GELU -> fp16):   1.13 E_acc + 3.4e-6 + 2^-11 |y|      (|gelu'| <= 1.13; 3.4e-6: the shipped GELU form against erf)
  * epilogue 2 (resid + gamma (acc + bias), fp32):  |gamma| E_acc + 3 u (|resid| + |gamma| |acc + bias|)   (three fp32 roundings)
  * statistics of the folded-LayerNorm producer: an fp32 sum of 64 terms on the kernel's own x: gamma_64 sum |x| (and sum x^2);
  * folded-LayerNorm consumer, y = act(rstd (acc - mean s) + t) on the kernel's own (x16, mean, rstd): the rank-1 term is three more
    products of the same accumulation (hi hi + lo hi + hi lo of the fp16 splits of s and -mean), so
    E_c = gamma_(K+3) (sum |x w| + |mean s|) + 3 * 2^-22 |mean s| + 2^-25 (|mean| + |s|): a two-term fp16 split represents its value to
    2^-22 (relative) or 2^-25 (absolute, once the low part is subnormal), the dropped lo lo product is below 2^-22 |mean s|; then one
    fused multiply-add (u |v|) and the epilogue terms above with rstd E_c in the place of E_acc.
Tile 17 against tile 15 on the same inputs: within twice the bound (both are inside it; they are not bit-identical - the two MFMA
shapes sum in different orders). A test without a GPU evaluates the same expressions in fp32 on the CPU through the same assertions.
Run with -s for the worst error / bound ratio of every case."""
import pytest
import torch

from oracle.gemm import Case, _gamma, _ln_reference, _rand      # the float64 references and bounds, shared with tests/test_gemm_exact_gpu.py


def _within_twice(o17, o15, case, what):
    d = (o17.double().cpu() - o15.double().cpu()).abs()
    ratio = (d / (2.0 * case.bound)).max().item()
    print(f"{what}: tile 17 against tile 15: worst |difference| / (2 bound) = {ratio:.3f} (max |difference| {d.max().item():.3e})")
    assert ratio <= 1.0, (what, ratio)


def _inputs(M, N, K, dev, seed):
    a = _rand((M, K), dev, 1.0, seed).half()
    w = _rand((N, K), dev, 0.05, seed + 1).half()
    bias = _rand((N,), dev, 0.5, seed + 2)
    resid = _rand((M, N), dev, 1.0, seed + 3)
    gamma = (_rand((N,), dev, 0.3, seed + 4) + 1.0).contiguous()
    return a, w, bias, resid, gamma


def _run(ops, tile, a, w, bias, epi, resid, gamma):
    """epilogue 2 in place with gamma, as the encoder blocks call it; returns (out, tile dispatched to)"""
    e = (ops.EPI_F16, ops.EPI_GELU_F16, ops.EPI_F32)[epi]
    ops.gemm_set_tile(tile)
    try:
        if epi == 2:
            x = resid.clone()
            out = ops.gemm(a, w, bias, out=x, epilogue=e, resid=x, gamma=gamma)
        else:
            out = ops.gemm(a, w, bias, epilogue=e)
        torch.cuda.synchronize()
        return out, ops.gemm_last_tile()
    finally:
        ops.gemm_set_tile(0)


# (M, N, K, the tile a forced 17 must end on): one tile and one K-tile (below tile 15's minimum K: falls back like 15); two and three
# K-tiles (buffer parity, address toggles, even / odd count); ragged M and two column tiles; N no multiple of 256 (falls back)
SHAPES = [(256, 256, 64, 11), (256, 256, 128, 17), (256, 256, 192, 17), (300, 512, 320, 17), (256, 384, 128, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,lands", SHAPES)
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_tile17_against_float64(dev, M, N, K, lands, epi):
    from protosam_amd import ops
    a, w, bias, resid, gamma = _inputs(M, N, K, dev, 100 + epi)
    case = Case(a, w, bias, epi, resid, gamma)
    o17, t17 = _run(ops, 17, a, w, bias, epi, resid, gamma)
    assert t17 == lands, (t17, lands)
    case.check(o17, f"tile 17 {M}x{N}x{K} epilogue {epi}")
    o15, t15 = _run(ops, 15, a, w, bias, epi, resid, gamma)
    assert t15 == (15 if lands == 17 else lands)
    _within_twice(o17, o15, case, f"{M}x{N}x{K} epilogue {epi}")


@pytest.mark.gpu
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_tile17_one_workgroup_walks_three_tiles(dev, epi):
    """max_wgs = 1: the K-tile stream runs across two tile seams, an epilogue runs with the next tile's DMA in flight"""
    from protosam_amd import ops
    M, N, K = 768, 256, 192
    a, w, bias, resid, gamma = _inputs(M, N, K, dev, 200 + epi)
    case = Case(a, w, bias, epi, resid, gamma)
    ops.gemm_set_option("max_wgs", 1)
    try:
        o17, t17 = _run(ops, 17, a, w, bias, epi, resid, gamma)
        o15, _ = _run(ops, 15, a, w, bias, epi, resid, gamma)
    finally:
        ops.gemm_set_option("max_wgs", 0)
    assert t17 == 17
    case.check(o17, f"tile 17 one workgroup, three tiles, epilogue {epi}")
    _within_twice(o17, o15, case, f"one workgroup epilogue {epi}")


@pytest.mark.gpu
def test_tile17_residual_table(dev):
    """resid_mod = 256: a [256, N] table as the residual of every 256-row image (out of place)"""
    from protosam_amd import ops
    M, N, K = 512, 256, 128
    a, w, bias, _, gamma = _inputs(M, N, K, dev, 300)
    table = _rand((256, N), dev, 1.0, 305)
    case = Case(a, w, bias, 2, table, gamma, resid_mod=256)
    outs = []
    for tile in (17, 15):
        ops.gemm_set_tile(tile)
        try:
            outs.append(ops.gemm(a, w, bias, epilogue=ops.EPI_F32, resid=table, gamma=gamma, resid_mod=256))
            torch.cuda.synchronize()
            assert ops.gemm_last_tile() == tile
        finally:
            ops.gemm_set_tile(0)
    case.check(outs[0], "tile 17 resid_mod 256")
    _within_twice(outs[0], outs[1], case, "resid_mod 256")


@pytest.mark.gpu
@pytest.mark.parametrize("act", [0, 1])
def test_tile17_folded_layernorm(dev, act):
    """the smallest parameter set of test_gemm_folded_layernorm (M = 777, D = 256, N2 = 256): the producer (fp32 residual epilogue + fp16
    copy + per-row statistics over 64-column groups) and the consumer (rank-1 -mean s, rstd, bias, (GELU)) on tile 17"""
    from protosam_amd import ops
    M, D, N2, K1 = 777, 256, 256, 256
    a, w1, b1, resid, gamma = _inputs(M, D, K1, dev, 400)
    resid = (resid + 0.7).contiguous()
    ln_w = (_rand((D,), dev, 0.1, 406) + 1.0).contiguous()
    ln_b = _rand((D,), dev, 0.1, 407)
    w2 = _rand((N2, D), dev, 0.03, 408)
    b2 = _rand((N2,), dev, 0.2, 409)
    prod = Case(a, w1, b1, 2, resid, gamma)
    wf, s_ext, t_ = ops.fold_layernorm(w2, b2, ln_w, ln_b)
    res = {}
    for tile in (17, 15):
        ops.gemm_set_tile(tile)
        try:
            x = resid.clone()
            x16 = torch.empty((M, D), dtype=torch.float16, device=dev)
            stats = torch.full((M, D // 64, 2), float("nan"), device=dev)
            ops.gemm(a, w1, b1, out=x, epilogue=ops.EPI_F32, resid=x, gamma=gamma, out16=x16, stats=stats)
            torch.cuda.synchronize()
            assert ops.gemm_last_tile() == tile
            mr = ops.ln_finalize(stats, M, D, 1e-6)
            y = ops.gemm(x16, wf, t_, epilogue=ops.EPI_GELU_F16 if act else ops.EPI_F16, ln_mr=mr, ln_s=s_ext)
            torch.cuda.synchronize()
            assert ops.gemm_last_tile() == tile
            res[tile] = (x, x16, stats, mr, y)
        finally:
            ops.gemm_set_tile(0)
    x, x16, stats, mr, y = res[17]
    prod.check(x, "tile 17 producer x")
    assert torch.equal(x16, x.half())
    xg = x.double().cpu().view(M, D // 64, 64)
    for j, (ref, mag) in enumerate(((xg.sum(2), xg.abs().sum(2)), ((xg * xg).sum(2), (xg * xg).sum(2)))):
        d = (stats[..., j].double().cpu() - ref).abs()
        ratio = (d / (_gamma(64) * mag)).max().item()
        print(f"tile 17 producer statistics {('sum', 'sum of squares')[j]}: worst |error| / bound = {ratio:.3f}")
        assert ratio <= 1.0
    ref, bound = _ln_reference(x16, wf, t_, mr[:2 * M].view(M, 2), s_ext[:N2], act)
    d = (y.double().cpu() - ref).abs()
    ratio = (d / bound).max().item()
    print(f"tile 17 consumer act {act}: worst |error| / bound = {ratio:.3f} (max |error| {d.max().item():.3e})")
    assert torch.isfinite(y).all() and ratio <= 1.0
    # against tile 15 on the same inputs (its own producer's x16 / statistics are within rounding of these, so compare the consumers
    # through their own references: each inside its bound, and the producers within twice theirs)
    _within_twice(x, res[15][0], prod, "producer")
    ref15, bound15 = _ln_reference(res[15][1], wf, t_, res[15][3][:2 * M].view(M, 2), s_ext[:N2], act)
    assert ((res[15][4].double().cpu() - ref15).abs() <= bound15).all()
    ops.gemm_set_tile(15)
    try:
        y15_on_17 = ops.gemm(x16, wf, t_, epilogue=ops.EPI_GELU_F16 if act else ops.EPI_F16, ln_mr=mr, ln_s=s_ext)
        torch.cuda.synchronize()
    finally:
        ops.gemm_set_tile(0)
    dd = (y.double().cpu() - y15_on_17.double().cpu()).abs()
    print(f"consumer act {act}: tile 17 against tile 15 on the same inputs: worst |difference| / (2 bound) = {(dd / (2 * bound)).max().item():.3f} "
          f"(max |difference| {dd.max().item():.3e})")
    assert (dd <= 2 * bound).all()


@pytest.mark.parametrize("epi", [0, 1, 2])
def test_bound_holds_for_fp32_on_the_cpu(epi):
    """the same expressions in fp32 torch on the CPU pass the same assertions: the float64 reference and the bound are consistent"""
    cpu = torch.device("cpu")
    for (M, N, K) in [(256, 256, 128), (300, 512, 320)]:
        a, w, bias, resid, gamma = _inputs(M, N, K, cpu, 100 + epi)
        case = Case(a, w, bias, epi, resid, gamma)
        v = a.float() @ w.float().t() + bias
        if epi == 0:
            out = v.half()
        elif epi == 1:
            out = torch.nn.functional.gelu(v).half()
        else:
            out = resid + gamma * v
        case.check(out, f"fp32 on the CPU {M}x{N}x{K} epilogue {epi}")


@pytest.mark.parametrize("act", [0, 1])
def test_layernorm_bound_holds_for_fp32_on_the_cpu(act):
    cpu = torch.device("cpu")
    M, D, N2 = 300, 256, 256
    x = _rand((M, D), cpu, 1.0, 500) + 0.7
    x16 = x.half()
    w2 = _rand((N2, D), cpu, 0.03, 508)
    b2 = _rand((N2,), cpu, 0.2, 509)
    ln_w = _rand((D,), cpu, 0.1, 506) + 1.0
    ln_b = _rand((D,), cpu, 0.1, 507)
    wf = (w2 * ln_w[None, :]).half()
    s = wf.float().sum(1)
    t = b2 + w2 @ ln_b
    mean = x.mean(1)
    rstd = torch.rsqrt(x.var(1, unbiased=False) + 1e-6)
    mr2 = torch.stack([mean, rstd], 1)
    # the kernel's arithmetic in fp32: the fp16 hi / lo splits of s and -mean, three products added to the accumulation
    s_hi = s.half().float(); s_lo = (s - s_hi).half().float()
    m_hi = (-mean).half().float(); m_lo = (-mean - m_hi).half().float()
    acc = x16.float() @ wf.float().t() + (s_hi[None, :] * m_hi[:, None] + s_lo[None, :] * m_hi[:, None] + s_hi[None, :] * m_lo[:, None])
    v = (rstd.double()[:, None] * acc.double() + t.double()[None, :]).float()      # one rounding: the fused multiply-add
    out = (torch.nn.functional.gelu(v) if act else v).half()
    ref, bound = _ln_reference(x16, wf, t, mr2, s, act)
    ratio = ((out.double() - ref).abs() / bound).max().item()
    print(f"fp32 on the CPU, folded-LayerNorm consumer act {act}: worst |error| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    # statistics: an fp32 sum of 64 terms
    xg = x.view(M, D // 64, 64)
    for got, ref64, mag in ((xg.sum(2), xg.double().sum(2), xg.double().abs().sum(2)), ((xg * xg).sum(2), (xg.double() ** 2).sum(2), (xg.double() ** 2).sum(2))):
        assert ((got.double() - ref64).abs() <= _gamma(64) * mag).all()
