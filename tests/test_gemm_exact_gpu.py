"""GPU: every path behind psam_gemm_f16 / psam_gemm_f16_ln / psam_gemm_f16_heads / psam_gemm_f16_splitk_ln (csrc/gemm.hip: the 128x128
kernel, its four-deep ring form, the 64x64 kernel, the persistent 256x256 kernel, the assembly tiles 15 / 16 / 17, both split-K forms
and the column split) held to oracle/gemm.py instead of the rtol = atol = 2e-3 the other GEMM tests inherit - at a typical product of
0.04 that passes a dropped 8-element chunk, a K-tile read from the wrong ring buffer on one parity and the bias of the neighbouring
column group (tests/test_gemm_reference_cpu.py injects those and thirteen more, and shows that the checks used here catch each one at
every case below).

Exact layer (`test_exact`, `test_hip_splitk_*`, `test_splitk_ln_exact`): operands on which every partial sum is exact in any order, so the
output is ONE bit pattern. Every case has: guarded outputs (sentinel rows before row 0, 256 rows behind row M - 1, padding columns, the
owed elements prefilled with NaN; the whole buffer is compared as integers), poisoned K padding (lda = K + 64, ldw = K + 8), the tile
`gemm_last_tile()` must report, and a failure message that names the first wrong element, its tile and its place inside the tile.
The case table is `oracle.gemm.cases()`; its comments say which loop state each shape is the smallest witness of.

Bound layer: real operands against float64 with the derived bounds of the oracle's docstring (epilogues 0 / 1 / 2 on tiles 1, 11, 12, 13,
15, 16; the folded-LayerNorm consumer on tiles 1, 11, 15; ln_finalize; the LayerNorm of gemm_splitk_ln). Run with -s for every ratio.

Rows of the issue's table that read differently here, because the code decides:
  * tile 15's map sweep runs on 256-tiles (N = 256 ntn): N = 128 ntn with an odd ntn is no multiple of 256 and falls back to tile 1;
  * gemm_last_tile() reports the second launch of the column split: 256 columns left of 4352, 64 tiles of 128 for 256 CUs, tile 13;
  * a forced tile 12 below four K-tiles and a forced tile 13 with a head-major output run on tile 1, and gemm_last_tile() must say 1
    (the report is taken after these two fall-backs as well: docs/history/KERNEL_NOTES.md);
  * PSAM_GEMM_MAP is read once per process, so the maps cannot be switched per case: the HIP tiles run the 2-D region map at every grid
    of the sweep, the assembly tiles the map pick_map_mode takes for the grid - the region map at the nine grids of the table, so a
    tenth, 85 x 3 tiles, is there for the contiguous map (tests/test_gemm_reference_cpu.py walks both maps on the host);
  * measured results: profiles/gemm_exact_tests.txt."""
import pytest
import torch

from oracle import gemm as G

pytestmark = pytest.mark.gpu

DEFAULTS = {"max_wgs": 0, "nsplit": 1, "half_tiles": 1}
TALLY = {}      # path -> [cases, elements compared, elements not bit-equal]


def _on(dev, buf, view):
    b = buf.to(dev)
    return torch.as_strided(b, view.shape, view.stride(), view.storage_offset())


def _launch(ops, dev, c, inp, tile=None):
    """one launch of the case on prefilled device buffers -> (buffers, gemm_last_tile()); options and the override are restored"""
    a, w = _on(dev, inp.a_buf, inp.a), _on(dev, inp.w_buf, inp.w)
    bias = inp.bias64.float().to(dev)
    gamma = inp.gamma64.float().to(dev) if c.gamma else None
    bufs = {k: v.to(dev) for k, v in inp.buffers().items()}
    out = inp.out.view(bufs["out"])
    resid = None
    if c.resid == "in":
        resid = out
    elif c.resid == "out":
        resid = _on(dev, inp.resid_buf, inp.resid)
    kw = {}
    if c.fold:
        kw = dict(out16=inp.out16.view(bufs["out16"]), stats=inp.stats.view(bufs["stats"]))
    if c.seg:
        kw.update(out_seg=c.seg[0], out_seg_stride=c.seg[1], out_seg_off=c.seg[2])
    for k, v in c.opts:
        ops.gemm_set_option(k, v)
    ops.gemm_set_tile(c.tile if tile is None else tile)
    try:
        if c.hd:
            ops.gemm_heads(a, w, bias, c.hd, out=out)
        else:
            ops.gemm(a, w, bias, out=out, epilogue=(ops.EPI_F16, None, ops.EPI_F32, ops.EPI_RELU_F16)[c.epi], resid=resid, gamma=gamma,
                     resid_mod=c.resid_mod, **kw)
        torch.cuda.synchronize()
        return bufs, ops.gemm_last_tile()
    finally:
        ops.gemm_set_tile(0)
        for k, _ in c.opts:
            ops.gemm_set_option(k, DEFAULTS[k])


def _checked(c, inp, bufs):
    """tally, then the located check"""
    t = TALLY.setdefault(c.path, [0, 0, 0])
    bad = inp.count_bad(bufs)
    t[0] += 1; t[1] += sum(b.numel() for b in bufs.values()); t[2] += bad
    if bad:
        inp.check(bufs)


def _exact(ops, dev, c, tile=None):
    inp = G.inputs(c)
    bufs, landed = _launch(ops, dev, c, inp, tile)
    if tile is None:
        assert landed == c.lands, f"{c.id}: ran on tile {landed}, the case is meant for tile {c.lands} ({c.why or 'forced'})"
    _checked(c, inp, bufs)
    return inp, bufs


SPECIAL = ("splitk",)


@pytest.mark.parametrize("case", [c for c in G.cases() if c.path not in SPECIAL], ids=lambda c: c.id)
def test_exact(dev, case):
    from protosam_amd import ops
    _exact(ops, dev, case)


@pytest.mark.parametrize("case", [c for c in G.cases() if c.path == "splitk"], ids=lambda c: c.id)
def test_hip_splitk_exact_and_ran(dev, case):
    """launch8kp_splitk + its reduce pass: the registered workspace is NaN-filled first and its first ks M N floats are finite afterwards
    (the path ran, with `ks` ranges and every partial sum written); bit-equal to the reference, hence to the forced tile 1, which is run too"""
    from protosam_amd import ops
    ops._ensure_gemm_workspace(dev)
    ws = ops._GEMM_WS[dev.index].view(torch.float32)
    n = case.ks * case.M * case.N
    assert torch.cuda.get_device_properties(dev).multi_processor_count == 256 and ws.numel() >= n
    ws.fill_(float("nan"))
    inp, bufs = _exact(ops, dev, case)
    assert torch.isfinite(ws[:n]).all(), "the split-K workspace was not written: another path ran"
    assert torch.isnan(ws[n:n + case.M * case.N]).all(), "more than ks planes were written"
    ws.fill_(float("nan"))
    _, bufs1 = _exact(ops, dev, case, tile=1)
    assert torch.isnan(ws[:n]).all() and torch.equal(bufs1["out"].view(torch.int32), bufs["out"].view(torch.int32))


def _splitk_ln(ops, dev, c, ln=None):
    """gemm_splitk_ln on the exact case under its max_wgs: -> (inputs, buffers, workspace with a guarded tail)"""
    inp = G.inputs(c)
    a, w = _on(dev, inp.a_buf, inp.a), _on(dev, inp.w_buf, inp.w)
    bufs = {k: v.to(dev) for k, v in inp.buffers().items()}
    x, o16 = inp.out.view(bufs["out"]), inp.out16.view(bufs["out16"])
    n = c.ks * ops.splitk_rows(c.M) * c.N
    ws = torch.full((n + 4096,), float("nan"), device=dev)
    ws[n:] = 12345.0
    for k, v in c.opts:
        ops.gemm_set_option(k, v)
    try:
        assert ops.gemm_splitk_ranges(c.M, c.N, c.K) == c.ks
        ops.gemm_splitk_ln(a, w, inp.bias64.float().to(dev), x, c.ks, ws[:n], *(ln or (None, None)), 1e-6, out16=o16)
        torch.cuda.synchronize()
    finally:
        for k, _ in c.opts:
            ops.gemm_set_option(k, DEFAULTS[k])
    assert bool((ws[n:] == 12345.0).all()), "the workspace was written beyond ks planes"
    for r in range(c.ks):         # every row a reduce pass reads was written by the launch
        assert torch.isfinite(ws[:n].view(c.ks, -1, c.N)[r, :c.M]).all(), f"range {r} of {c.ks} left rows unwritten"
    return inp, bufs


@pytest.mark.parametrize("case", G.splitk_ln_cases(), ids=lambda c: c.id)
def test_splitk_ln_exact(dev, case):
    """psam_gemm_asm_f32_sk + splitk_reduce_ln_kernel, ln_w None: x and out16 = half(x) exact, ldx and ld16 padded and guarded"""
    from protosam_amd import ops
    inp, bufs = _splitk_ln(ops, dev, case)
    _checked(case, inp, bufs)


@pytest.mark.parametrize("case", G.splitk_ln_cases(), ids=lambda c: c.id)
def test_splitk_ln_layernorm_bound(dev, case):
    """the same with ln_w, ln_b: x stays exact, out16 against the float64 LayerNorm of that x within the two-pass fp32 bound"""
    from protosam_amd import ops
    ln_w, ln_b = G.ln_params(case.N)
    inp, bufs = _splitk_ln(ops, dev, case, (ln_w.to(dev), ln_b.to(dev)))
    inp.out.check(bufs["out"], inp.ref, case)
    o16 = inp.out16.view(bufs["out16"])
    y, bound = G.layernorm16_bound(inp.ref.float(), ln_w, ln_b, 1e-6)
    ratio = ((o16.double().cpu() - y).abs() / bound).max().item()
    print(f"gemm_splitk_ln {case.M}x{case.N}x{case.K}, {case.ks} ranges, LayerNorm: worst |error| / bound = {ratio:.3f}")
    assert torch.isfinite(o16).all() and ratio <= 1.0
    exp = inp.out16.expected(y)                       # the guards of out16: everything the kernel does not owe is untouched
    owed = torch.zeros(inp.out16.total, dtype=torch.bool)
    owed[inp.out16.index.reshape(-1)] = True
    assert torch.equal(bufs["out16"].cpu().view(torch.int16)[~owed], exp.view(torch.int16)[~owed])


def test_splitk_ln_declines(dev):
    from protosam_amd import ops
    for M, N, K, wgs in G.SPLITK_LN_DECLINED:
        ops.gemm_set_option("max_wgs", wgs)
        try:
            assert ops.gemm_splitk_ranges(M, N, K) == 0, (M, N, K, wgs)
        finally:
            ops.gemm_set_option("max_wgs", 0)


# ------------------------------------------------------------------------------------------------ bound layer
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


@pytest.mark.parametrize("tile", [1, 11, 12, 13, 15, 16])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_epilogues_against_float64(dev, tile, epi):
    """tile 16 starts its accumulators from the bias: its bound has the bias inside the accumulation, gamma_(K+1) (sum |a w| + |bias|)"""
    from protosam_amd import ops
    M, N, K = G.bound_shape(tile, epi)
    a, w, bias, resid, gamma = G.real_inputs(M, N, K, dev, 100 + epi)
    case = G.Case(a, w, bias, epi, resid, gamma, bias_inside=tile == 16)
    out, landed = _run(ops, tile, a, w, bias, epi, resid, gamma)
    assert landed == tile, (landed, tile)
    case.check(out, f"tile {tile} {M}x{N}x{K} epilogue {epi}")


@pytest.mark.parametrize("tile", [1, 11, 15])
@pytest.mark.parametrize("act", [0, 1])
def test_folded_layernorm_consumer(dev, tile, act):
    """producer (x, half(x), statistics) -> ln_finalize -> consumer, all on `tile`; the consumer against float64 on its own
    (x16, mean, rstd): the HIP bound for tiles 1 and 11, the assembly bound for tile 15"""
    from protosam_amd import ops
    M, D, N2 = G.LN_CONSUMER
    K1 = 128
    a, w1, b1, resid, gamma = G.real_inputs(M, D, K1, dev, 400)
    resid = (resid + 0.7).contiguous()
    ln_w = (G._rand((D,), dev, 0.1, 406) + 1.0).contiguous()
    ln_b = G._rand((D,), dev, 0.1, 407)
    w2, b2 = G._rand((N2, D), dev, 0.03, 408), G._rand((N2,), dev, 0.2, 409)
    prod = G.Case(a, w1, b1, 2, resid, gamma)
    wf, s_ext, t_ = ops.fold_layernorm(w2, b2, ln_w, ln_b)
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
    finally:
        ops.gemm_set_tile(0)
    prod.check(x, f"tile {tile} producer x")
    assert torch.equal(x16, x.half())
    xg = x.double().cpu().view(M, D // 64, 64)
    for j, (ref, mag) in enumerate(((xg.sum(2), xg.abs().sum(2)), ((xg * xg).sum(2), (xg * xg).sum(2)))):
        ratio = ((stats[..., j].double().cpu() - ref).abs() / (G._gamma(64) * mag)).max().item()
        print(f"tile {tile} producer statistics {('sum', 'sum of squares')[j]}: worst |error| / bound = {ratio:.3f}")
        assert ratio <= 1.0
    reference = G._ln_reference if tile == 15 else G.ln_reference_hip
    ref, bound = reference(x16, wf, t_, mr[:2 * M].view(M, 2), s_ext[:N2], act)
    d = (y.double().cpu() - ref).abs()
    ratio = (d / bound).max().item()
    print(f"tile {tile} consumer act {act}: worst |error| / bound = {ratio:.3f} (max |error| {d.max().item():.3e})")
    assert torch.isfinite(y).all() and ratio <= 1.0


@pytest.mark.parametrize("D", G.LN_FINALIZE_D)
def test_ln_finalize_on_exact_statistics(dev, D):
    """mean within two fp32 roundings of float64, rstd within the bound of the oracle's docstring; the fp16 fragments of -mean"""
    from protosam_amd import ops
    M = 300
    stats, _ = G.exact_stats(M, D)
    mr = ops.ln_finalize(stats.to(dev), M, D, 1e-6)
    torch.cuda.synchronize()
    mr2 = mr[:2 * M].view(M, 2).double().cpu()
    m64, dm, r64, dr = G.ln_finalize_bounds(stats, D, 1e-6)
    em, er = (mr2[:, 0] - m64).abs(), (mr2[:, 1] - r64).abs()
    assert (em <= dm).all() and (er <= dr).all(), ((em - dm).max().item(), (er / dr).max().item())
    print(f"ln_finalize D = {D}: worst |error| / bound: mean {(em / dm.clamp_min(1e-300)).max().item():.3f}, rstd {(er / dr).max().item():.3f}")
    frag = mr[2 * M:].view(torch.float16).view(M, 8).float()
    assert torch.equal(frag[:, 0], frag[:, 1]) and int(frag[:, 3:].abs().sum()) == 0
    torch.testing.assert_close(frag[:, 0] + frag[:, 2], -mr[:2 * M].view(M, 2)[:, 0], rtol=1e-6, atol=1e-7)


def test_zz_tally(dev):
    """the digest of the exact layer (printed with -s): cases, elements compared and elements not bit-equal per path"""
    for path, (n, elems, bad) in sorted(TALLY.items()):
        print(f"exact {path}: {n} cases, {elems} buffer elements compared (guards included), {bad} not bit-equal")
    assert all(t[2] == 0 for t in TALLY.values())
