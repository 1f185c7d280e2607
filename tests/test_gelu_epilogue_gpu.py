"""GPU: the three hand-written GELUs behind EPI_GELU_F16 (common.h gelu_erf on tiles 1 / 11 / 12 / 13, gelu_quad of csrc/gemm_asm_gen.py
on tiles 15 / 17, gelu_scalar of csrc/gemm_asm2_gen.py on tile 16) and the folded-LayerNorm consumers (tiles 1, 11, 15, 17) run on the
device over the whole line: the uniform sweep of [-32, 32.25) at step 2^-10 and the tail sets of oracle/pointwise.py (|x| up to 60000,
fp16-subnormal results, fp32-subnormal and signed-zero pre-activations), where the other GPU tests stop at |x| of about 4.5.

The pre-activation of every element is exact (one non-zero product plus the bias), so the bound is the epilogue's alone:
3.4e-6 + 2^-11 |y| against 0.5 x erfc(-x / sqrt 2) in float64, plus the structural checks (finite; the sign of x; y = x to an fp16
rounding from 8 on; |y| <= 3.4e-6 below -8). tests/test_pointwise_reference_cpu.py shows fp32 emulations of the shipped sequences inside
all of it and seven wrong GELUs outside. Every launch: the tile's minimum K, poisoned K padding, the tile asserted with gemm_last_tile(),
a guarded output (NaN where a value is owed, a sentinel elsewhere; nothing outside M x N may change). Run with -s for the worst
|error| / bound and its x per tile, set and range of the line; measured: profiles/pointwise_tests.txt."""
import pytest
import torch

from oracle import gemm as G
from oracle import pointwise as P

pytestmark = pytest.mark.gpu

HIP_TILES = (1, 11, 12, 13)
RESULTS = {}        # (tile, folded, set) -> the M x N outputs on the CPU


def _on(dev, buf, view):
    b = buf.to(dev)
    return torch.as_strided(b, view.shape, view.stride(), view.storage_offset())


def _result(dev, tile, folded, name):
    """one guarded launch of set `name` on `tile` (cached): the tile and the guards are asserted here"""
    key = (tile, folded, name)
    if key in RESULTS:
        return RESULTS[key]
    from protosam_amd import ops
    c, d = P.gelu_sets()[name]
    (a_buf, a), (w_buf, w), bias = P.gelu_operands(c, d, P.gelu_min_k(tile))
    lay = G.Layout("out", torch.float16, P.GELU_M, P.GELU_N, P.GELU_N + 8)
    buf = lay.alloc().to(dev)
    kw = {}
    if folded:
        mr, s_ext = P.gelu_ln_operands(P.GELU_M, P.GELU_N)
        kw = dict(ln_mr=mr.to(dev), ln_s=s_ext.to(dev))
    ops.gemm_set_tile(tile)
    try:
        ops.gemm(_on(dev, a_buf, a), _on(dev, w_buf, w), bias.to(dev), out=lay.view(buf), epilogue=ops.EPI_GELU_F16, **kw)
        torch.cuda.synchronize()
        landed = ops.gemm_last_tile()
    finally:
        ops.gemm_set_tile(0)
    assert landed == tile, f"forced tile {tile} ran on tile {landed}"
    buf = buf.cpu()
    owed = torch.zeros(lay.total, dtype=torch.bool)
    owed[lay.index.reshape(-1)] = True
    guards = G._sentinel(lay.total, torch.float16).view(torch.int16)
    changed = (buf.view(torch.int16) != guards) & ~owed
    assert not bool(changed.any()), f"tile {tile} {name}: {int(changed.sum())} elements outside the {P.GELU_M} x {P.GELU_N} block were written"
    RESULTS[key] = lay.view(buf).clone()
    return RESULTS[key]


@pytest.mark.parametrize("name", list(P.gelu_sets()))
@pytest.mark.parametrize("tile", P.GELU_TILES)
def test_gelu_epilogue_over_the_whole_line(dev, tile, name):
    c, d = P.gelu_sets()[name]
    P.gelu_check(_result(dev, tile, False, name), P.gelu_x(c, d), f"tile {tile} {name}")


@pytest.mark.parametrize("name", list(P.gelu_sets()))
@pytest.mark.parametrize("tile", P.GELU_LN_TILES)
def test_gelu_folded_layernorm_consumer_over_the_whole_line(dev, tile, name):
    """ln_mr written by hand for mean 0, rstd 1: rstd (acc - mean s) + t = acc + t exactly, whatever ln_s holds"""
    c, d = P.gelu_sets()[name]
    P.gelu_check(_result(dev, tile, True, name), P.gelu_x(c, d), f"tile {tile} folded-LayerNorm consumer {name}")


def test_gelu_forms_against_each_other(dev):
    """on the grid: the HIP tiles (one gelu_erf) agree bit for bit, plain and folded; tile 15 is within one fp16 ulp + 5e-6 of them (what
    test_gemm_persistent_tile_walks_many_tiles allows); tiles 16 and 17 are reported"""
    hip = _result(dev, 1, False, "grid")
    for tile in HIP_TILES[1:]:
        assert torch.equal(_result(dev, tile, False, "grid").view(torch.int16), hip.view(torch.int16)), f"tile {tile} against tile 1"
    for tile in (1, 11):
        assert torch.equal(_result(dev, tile, True, "grid").view(torch.int16), hip.view(torch.int16)), f"folded tile {tile} against tile 1"
    h = hip.double()
    ulp = torch.maximum(torch.exp2(torch.floor(torch.log2(h.abs().clamp_min(2.0 ** -14))) - 10), torch.tensor(2.0 ** -24, dtype=torch.float64))
    for tile, folded in ((15, False), (15, True), (16, False), (17, False), (17, True)):
        diff = (_result(dev, tile, folded, "grid").double() - h).abs()
        r = (diff / (ulp + 5e-6)).max().item()
        print(f"tile {tile}{' folded' if folded else ''} against the HIP tiles on the grid: {int((diff > 0).sum())} of {diff.numel()} differ, worst "
              f"|difference| / (ulp + 5e-6) = {r:.3f}")
        if tile == 15:
            assert r <= 1.0, (tile, folded, r)
