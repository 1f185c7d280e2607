"""GPU: every attention kernel path of csrc/attention.hip (`attn_kernel`, `wattn_kernel`, `wattn_p_kernel`, `gattn_kernel`,
`gattn_any_kernel` and the assembly kernels psam_gattn_asm_{80,64}_{rel,fused}, psam_gattn_asm_64_norel, psam_wattn_asm_80) held to
oracle/attention.py, with tolerances that are derived instead of the 2e-3 the other attention tests inherit - at unit-variance
inputs 2e-3 is 2 to 10 % of the output and passes a dropped key, the unmasked tail tile and swapped weights
(tests/test_attention_reference_cpu.py shows that, and that the checks used here catch them at every shape below).

Three families per shape and path, each blind to something the others see:
  (a) selector inputs - every query's softmax is one-hot on its own key, the targets a permutation: the output must be that key's
      v row to within one fp16 ulp (QK selector: every key and value; rel-pos selector: every (query row, key row) of both table
      gathers). The margin (>= 32 nats) is asserted on the float64 reference before the kernel output is looked at.
  (b) constant V - any correct softmax returns c: |out - c| <= (2^-10 + N_k 2^-24) |c|, diffuse and with the spike pattern (the
      lazy-rescale branch). A mask error or a rescale applied to O but not to l shows at full size.
  (c) the float64 error budget on diffuse inputs: the derived elementwise bound, and rms(out - o) <= 3 rms(rounding model - o) per
      (image, head). docs/ATTENTION_ACCURACY.md records the measured ratios.

Every path = (name, variant, kind, id) also names the kernel it is meant to land on, as `ops.attention_last_kernel()` reports it after
the launch (family | FULL | STAGE64 | V2; the `ops.relpos` launch of the two-kernel paths: relpos | QT4): `launch_attn` falls back
silently wherever an eligibility rule says no, and a label is worth what that report says.
"""
import pytest
import torch

from oracle import attention as A
from protosam_amd import ops as K          # (the ids only: nothing here loads the library)

pytestmark = pytest.mark.gpu


def _full(N):
    """the flag of the HIP global kernels' full-tile instance"""
    return K.ATTN_KERNEL_FULL if N % 64 == 0 else 0


def _relpos_id(N):
    return K.ATTN_KERNEL_RELPOS | (K.ATTN_KERNEL_QT4 if N % 256 == 0 else 0)


def _landed(want, what):
    """the kernel the launch just made went to, against the path's id."""
    got = K.attention_last_kernel()
    assert got == want, (f"{what} ran {K.attention_kernel_name(got)} ({got:#x}), the path names "
                         f"{K.attention_kernel_name(want)} ({want:#x})")


def _head_major(qkv):
    """[B,N,3,H,hd] -> [3,H,B*N,hd] (what psam_gemm_f16_heads writes; as tests/test_anysize_gpu.py::_head_major)."""
    B, N, _, H, hd = qkv.shape
    return qkv.permute(2, 3, 0, 1, 4).reshape(3, H, B * N, hd).contiguous()


def _embed(R, g, K=64):
    """(2 g - 1, hd) table -> the (2 K - 1, hd) table psam_relpos indexes with pos - k + K - 1: the rows moved up by K - g."""
    full = R.new_zeros((2 * K - 1, R.shape[1]))
    full[K - g:K + g - 1] = R
    return full


def _run(case, kind, head_major=False, out=None):
    """one launch (two for the paths that take psam_relpos' output, whose kernel id is asserted here) of the kernel the current
    variant selects, into a NaN-filled buffer (or `out`, which the caller filled)."""
    from protosam_amd import ops
    c = case
    src = _head_major(c.qkv) if head_major else c.qkv
    args = (src, c.B, c.N, c.H, c.hd, c.scale)
    if out is None:
        out = torch.full((c.B, c.N, c.H * c.hd), float("nan"), device=c.qkv.device, dtype=torch.float16)
    if kind == "plain":
        return ops.attention(*args, out=out, head_major=head_major)
    if kind == "terms":                     # gw == 64: rel_h / rel_w from psam_relpos
        rp = ops.pack_rel_tables(_embed(c.Rh, c.gh), c.Rw, False, c.hd)
        rel_h, rel_w = ops.relpos(src, rp, c.B, c.N, c.H, c.hd, 64, 64, False, c.scale, head_major=head_major)
        _landed(_relpos_id(c.N), "ops.relpos (global)")
        return ops.attention(*args, out=out, mode=1, rel_h=rel_h, rel_w=rel_w, gh=c.gh, gw=c.gw, head_major=head_major)
    if kind == "tables":                    # the packed tables alone: the fused assembly kernels / gattn_any_kernel
        rp = ops.pack_rel_tables(c.Rh, c.Rw, False, c.hd)
        return ops.attention(*args, out=out, mode=1, rpack=rp, gh=c.gh, gw=c.gw, head_major=head_major)
    rp = ops.pack_rel_tables(c.Rh, c.Rw, True, c.hd)
    kw = dict(out=out, mode=2, pad_row=c.pad_row, gh=c.gh, gw=c.gw, ws=A.WS, head_major=head_major)
    if kind == "relq":                      # the two-kernel window path
        relq = ops.relpos(src, rp, c.B, c.N, c.H, c.hd, c.gw, A.WS, True, c.scale, head_major=head_major)
        _landed(_relpos_id(c.N), "ops.relpos (windowed)")
        return ops.attention(*args, relq=relq, **kw)
    assert kind == "window"
    return ops.attention(*args, rpack=rp, **kw)


def _exact(dev, label, mode, B, H, hd, paths, N=0, gh=0, gw=0, head_major=False, seed=0):
    """Families (a), (b), (c) at one shape on every path = (name, variant, kind, kernel id). Every reference is computed once and
    shared by the paths; every failure of every path is collected, so one run shows the whole picture."""
    from protosam_amd import ops
    geo = dict(N=N, gh=gh, gw=gw, device=dev)
    cases = [("qk-selector", A.selector_qk(mode, B, H, hd, seed=seed + 1, **geo))]
    if mode:
        cases.append(("relpos-selector", A.selector_relpos(mode, B, H, hd, gh, gw, seed=seed + 2, device=dev)))
    cases += [("constant-v", A.constant_v(mode, B, H, hd, seed=seed + 3, **geo)),
              ("constant-v-spiky", A.constant_v(mode, B, H, hd, seed=seed + 4, spiky=True, **geo)),
              ("diffuse-0.5", A.diffuse(mode, B, H, hd, std=0.5, seed=seed + 5, **geo)),
              ("diffuse-1.0", A.diffuse(mode, B, H, hd, std=1.0, seed=seed + 6, **geo))]
    errors = []
    shape = f"{label} B{B} H{H} hd{hd} " + (f"N{N}" if mode == 0 else f"{gh}x{gw}") + (" head-major" if head_major else "")
    for fam, case in cases:
        budget = fam.startswith("diffuse")
        ref = None
        if fam.endswith("selector") or budget:
            ref = A.reference(case.qkv, mode, budget=budget, model=budget, targets=case.targets, **A.ref_kwargs(case))
        if fam.endswith("selector"):
            margin = A.check_margin(case, ref)              # the condition, before any kernel output
            print(f"EXACT | {shape} | {fam} | least margin {margin:.1f} nats")
        for name, variant, kind, kid in paths:
            ops.attention_set_variant(variant)
            try:
                out = _run(case, kind, head_major)
                landed = ops.attention_last_kernel()
            finally:
                ops.attention_set_variant(5)
            try:
                assert landed == kid, (f"ran {ops.attention_kernel_name(landed)} ({landed:#x}), the path names "
                                       f"{ops.attention_kernel_name(kid)} ({kid:#x})")
                if fam.endswith("selector"):
                    res = f"not bit-equal {A.check_selector(out, case)}"
                elif budget:
                    res = "max/bound {:.3f} rms/model {:.2f}".format(*A.check_budget(out, case, ref))
                else:
                    res = f"max/bound {A.check_constant_v(out, case):.3f}"
                print(f"EXACT | {shape} | {fam} | {name} | {ops.attention_kernel_name(landed)} | {res}")
            except AssertionError as e:
                print(f"EXACT | {shape} | {fam} | {name} | FAILED {e}")
                errors.append(f"{shape}, {fam}, {name}: {e}")
    assert not errors, f"{len(errors)} failures:\n" + "\n".join(errors)


# ---- mode 0 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", [(1, 2), (3, 3)])
@pytest.mark.parametrize("N", A.MODE0_ASM_N)
def test_global_default_dispatch(dev, N, B, H):
    """hd = 64 on the default dispatch: psam_gattn_asm_64_norel from N >= 128 - two tiles and no loop (128), three (192), ONE key in
    the last tile (449), 17 valid keys in it (1297, 1301); B * H = 9 is no multiple of eight."""
    _exact(dev, "mode0", 0, B, H, 64, [("default: psam_gattn_asm_64_norel", 5, "plain", K.ATTN_KERNEL_ASM_NOREL)], N=N, seed=N)


@pytest.mark.parametrize("hd,N", A.MODE0_HIP)
def test_global_hip_kernels(dev, hd, N):
    """the HIP kernels behind the variants: 5 | 16 gattn_kernel (DMA-fed), 9 attn_kernel with the V2 softmax, 8 attn_kernel with the
    serial softmax, and 0 as the other tests select it (the serial softmax where no assembly kernel applies, else the assembly
    kernel); one tile (64), ragged (200, 1297), full tiles at hd = 80 (320)."""
    asm = hd == 64 and N >= 128
    f = _full(N)
    paths = [("variant 21: gattn_kernel", 5 | 16, "plain", K.ATTN_KERNEL_GATTN | f),
             ("variant 9: attn_kernel V2", 9, "plain", K.ATTN_KERNEL_ATTN | f | K.ATTN_KERNEL_V2),
             ("variant 8: attn_kernel serial", 8, "plain", K.ATTN_KERNEL_ATTN | f),
             ("variant 0: " + ("psam_gattn_asm_64_norel" if asm else "attn_kernel serial"), 0, "plain",
              K.ATTN_KERNEL_ASM_NOREL if asm else K.ATTN_KERNEL_ATTN | f)]
    _exact(dev, "mode0", 0, 1, 2, hd, paths, N=N, seed=N + hd)


# ---- mode 1 -----------------------------------------------------------------------------------------------------------------------
# (gw = 64 and gh in {4, 16, 64}: N is a multiple of 256 - the assembly kernel applies, the HIP kernels run their full-tile instance)
REL_PATHS = [("default: psam_gattn_asm_rel", 5, "terms", K.ATTN_KERNEL_ASM_REL),
             ("variant 17: gattn_kernel", 17, "terms", K.ATTN_KERNEL_GATTN | K.ATTN_KERNEL_FULL),
             ("variant 9: attn_kernel V2", 9, "terms", K.ATTN_KERNEL_ATTN | K.ATTN_KERNEL_FULL | K.ATTN_KERNEL_V2),
             ("variant 8: attn_kernel serial", 8, "terms", K.ATTN_KERNEL_ATTN | K.ATTN_KERNEL_FULL),
             ("variant 0: psam_gattn_asm_rel", 0, "terms", K.ATTN_KERNEL_ASM_REL)]   # (0 leaves the assembly kernel on where it applies)


@pytest.mark.parametrize("B,H", [(1, 2), (1, 3)])
@pytest.mark.parametrize("hd", A.HEAD_DIMS)
@pytest.mark.parametrize("gh", A.MODE1_GH_AT_GW64)
def test_global_relpos_terms_from_relpos(dev, gh, hd, B, H):
    """gw = 64 with rel_h / rel_w from `ops.relpos`: gh = 4 (N = 256, the smallest the assembly kernel takes), 16 and 64."""
    _exact(dev, "mode1 psam_relpos", 1, B, H, hd, REL_PATHS, gh=gh, gw=64, seed=gh + hd)


def _any_id(gh, gw):
    """gattn_any_kernel: ragged unless the map is whole key tiles, the 64-float stage from a side above 32."""
    return K.ATTN_KERNEL_GATTN_ANY | _full(gh * gw) | (K.ATTN_KERNEL_STAGE64 if max(gh, gw) > 32 else 0)


@pytest.mark.parametrize("hd", A.HEAD_DIMS)
def test_global_relpos_fused(dev, hd):
    """the packed tables alone at 64 x 64: the fused assembly kernels, and with bit 5 set gattn_any_kernel at gw = 64."""
    from protosam_amd import ops
    assert ops.attention_fused_relpos(1, 4096, 2, hd, 64, 64)
    paths = [(f"default: psam_gattn_asm_{hd}_fused", 5, "tables", K.ATTN_KERNEL_ASM_FUSED),
             ("variant 37: gattn_any_kernel", 5 | 32, "tables", _any_id(64, 64))]
    _exact(dev, "mode1 tables", 1, 1, 2, hd, paths, gh=64, gw=64, seed=hd)


@pytest.mark.parametrize("hd", A.HEAD_DIMS)
@pytest.mark.parametrize("gh,gw", A.ANY_MAPS)
def test_global_relpos_any_map(dev, gh, gw, hd):
    """gattn_any_kernel: maps smaller than one key tile (5 x 7, 3 x 1), key tiles that straddle rows with a ragged last tile
    (20 x 28), full tiles (32 x 32, 40 x 40), the 64-float stages (64 x 33)."""
    _exact(dev, "mode1 tables", 1, 1, 2, hd, [("gattn_any_kernel", 5, "tables", _any_id(gh, gw))], gh=gh, gw=gw,
           seed=gh * 64 + gw + hd)


# ---- mode 2 -----------------------------------------------------------------------------------------------------------------------
def _window_paths(g, hd, head_major=False):
    """the assembly window kernel takes hd = 80 on the 64 x 64 map from a token-major qkv with the packed tables; everything else
    of the default dispatch is wattn_p_kernel, and with relq in place of the tables attn_kernel."""
    asm = g == 64 and hd == 80 and not head_major
    paths = [("variant 1: attn_kernel", 1, "window", K.ATTN_KERNEL_ATTN), ("variant 3: wattn_kernel", 3, "window", K.ATTN_KERNEL_WATTN),
             ("variant 5: " + ("psam_wattn_asm_80" if asm else "wattn_p_kernel"), 5, "window",
              K.ATTN_KERNEL_ASM_WINDOW if asm else K.ATTN_KERNEL_WATTN_P),
             ("variant 7: wattn_p_kernel", 7, "window", K.ATTN_KERNEL_WATTN_P)]
    if (g * g) % 64 == 0:
        paths.append(("relq: psam_relpos + attn_kernel", 5, "relq", K.ATTN_KERNEL_ATTN))
    return paths


@pytest.mark.parametrize("B,H", [(1, 1), (1, 2), (3, 4)])
@pytest.mark.parametrize("g,hd", [(64, 80), (64, 64), (32, 64), (32, 80), (20, 64), (20, 80)])
def test_window_relpos(dev, g, hd, B, H):
    """14 x 14 windows: the 64 x 64 map (25 windows, nine of them ragged; 300 items at B = 3, H = 4 - more than one per CU, the
    persistent kernels walk their lists), 32 x 32 (nine windows), 20 x 20 (four, three of them ragged)."""
    _exact(dev, "mode2", 2, B, H, hd, _window_paths(g, hd), gh=g, gw=g, seed=g + hd)


# ---- head-major qkv: one case per mode --------------------------------------------------------------------------------------------
def test_head_major_global(dev):
    _exact(dev, "mode0", 0, 2, 3, 64, [("default: psam_gattn_asm_64_norel", 5, "plain", K.ATTN_KERNEL_ASM_NOREL),
                                       ("variant 21: gattn_kernel", 21, "plain", K.ATTN_KERNEL_GATTN),
                                       ("variant 9: attn_kernel V2", 9, "plain", K.ATTN_KERNEL_ATTN | K.ATTN_KERNEL_V2)],
           N=449, head_major=True, seed=71)


def test_head_major_global_relpos(dev):
    _exact(dev, "mode1 psam_relpos", 1, 2, 2, 80, REL_PATHS, gh=16, gw=64, head_major=True, seed=72)
    _exact(dev, "mode1 tables", 1, 2, 2, 80, [("gattn_any_kernel", 5, "tables", _any_id(20, 28))], gh=20, gw=28, head_major=True,
           seed=73)


def test_head_major_window(dev):
    _exact(dev, "mode2", 2, 2, 2, 80, _window_paths(32, 80, True), gh=32, gw=32, head_major=True, seed=74)
