"""GPU: SAM at any input size - global attention with decomposed rel-pos on a gh x gw token map with gw != 64 (`gattn_any_kernel`
behind `ops.attention(mode=1, rpack=..., gh=, gw=)`), and the modules built on it (`ImageEncoderViT(img_size=...)`, `Block` /
`Attention` on a g x g map, `Sam` / `SamPredictor` at 512 pixels) against what the REFERENCE's same-named modules returned for the
same seeded weights and inputs (tests/golden/reference_anysize.npz, written by tools/make_anysize_goldens.py).

Bounds are the project's own for the same quantities: rtol = atol = 2e-3 on the fp16 attention output of unit-variance inputs
(test_kernels_core_gpu.py), max err / rms < 4e-3 for `Block` / `Attention`, max < 5e-2 and mean < 3e-3 for the encoder embedding
(test_sam_gpu.py::test_image_encoder), 1e-3 on sigmoid(low_res) and on the IoU predictions (test_predictor_vs_reference).
"""
import os
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_anysize.npz")
TOL_PROB = 1e-3


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _rand(shape, dev, std, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * std).to(dev)


def _head_major(qkv):
    """[B,N,3,H,hd] -> [3,H,B*N,hd] (what psam_gemm_f16_heads writes)."""
    B, N, _, H, hd = qkv.shape
    return qkv.permute(2, 3, 0, 1, 4).reshape(3, H, B * N, hd).contiguous()


def _ref_relpos_attention(qkv, Rh, Rw, gh, gw, scale):
    """float64: softmax_k(scale q.k + q.Rh[qh - kh + gh - 1] + q.Rw[qw - kw + gw - 1]) v, the rel-pos terms from the UNSCALED q
    (add_decomposed_rel_pos); qkv fp16 [B,N,3,H,hd] -> float64 [B,N,H*hd]."""
    B, N, _, H, hd = qkv.shape
    dev = qkv.device
    ih = torch.arange(gh, device=dev)[:, None] - torch.arange(gh, device=dev)[None, :] + gh - 1       # [qh, kh]
    iw = torch.arange(gw, device=dev)[:, None] - torch.arange(gw, device=dev)[None, :] + gw - 1
    Rhh, Rww = Rh.double()[ih], Rw.double()[iw]                                                         # [gh, gh, hd], [gw, gw, hd]
    out = torch.empty((B, N, H * hd), dtype=torch.float64, device=dev)
    for b in range(B):
        q, k, v = qkv[b].double().permute(1, 2, 0, 3)                                                   # [H, N, hd]
        r_q = q.reshape(H, gh, gw, hd)
        rel_h = torch.einsum("bhwc,hkc->bhwk", r_q, Rhh)                                                # [H, gh, gw, kh]
        rel_w = torch.einsum("bhwc,wkc->bhwk", r_q, Rww)                                                # [H, gh, gw, kw]
        att = (q * scale) @ k.transpose(-2, -1)
        att = (att.view(H, gh, gw, gh, gw) + rel_h[..., :, None] + rel_w[..., None, :]).view(H, N, N)
        out[b] = (att.softmax(-1) @ v).permute(1, 0, 2).reshape(N, H * hd)
    return out


MAPS = [(16, 16), (24, 24), (32, 32), (40, 40), (48, 48), (20, 28), (28, 20), (64, 33), (5, 7), (3, 1)]


@pytest.mark.parametrize("head_major", [False, True], ids=["token_major", "head_major"])
@pytest.mark.parametrize("H,B", [(2, 1), (12, 3), (16, 1)])
@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("gh,gw", MAPS)
def test_attention_relpos_any_map(dev, gh, gw, hd, H, B, head_major):
    """The kernel against float64. Maps: multiples of 16 and not (20 x 28: 560 tokens, key tiles straddle rows, ragged last tile);
    gw > 32 with gh = 64 (the 64-float stages); maps smaller than one key tile (5 x 7, 3 x 1)."""
    from protosam_amd import ops
    N = gh * gw
    qkv = _rand((B, N, 3, H, hd), dev, 1.0, 100 + gh * 64 + gw).half()
    Rh = _rand((2 * gh - 1, hd), dev, 0.3, 12)
    Rw = _rand((2 * gw - 1, hd), dev, 0.3, 13)
    scale = hd ** -0.5
    rp = ops.pack_rel_tables(Rh, Rw, False, hd)
    src = _head_major(qkv) if head_major else qkv
    out = ops.attention(src, B, N, H, hd, scale, mode=1, rpack=rp, gh=gh, gw=gw, head_major=head_major)
    ref = _ref_relpos_attention(qkv, Rh, Rw, gh, gw, scale)
    err = (out.double() - ref).abs().max().item()
    print(f"{gh}x{gw} hd{hd} H{H} B{B} {'head' if head_major else 'token'}-major: max abs err {err:.2e}")
    assert out.shape == (B, N, H * hd) and torch.isfinite(out.float()).all()
    torch.testing.assert_close(out.double(), ref, rtol=2e-3, atol=2e-3)


@pytest.mark.parametrize("gh,gw,hd", [(32, 32, 64), (20, 28, 80), (40, 40, 80)])
def test_attention_relpos_any_map_spiky_rows(dev, gh, gw, hd):
    """Rows whose maximum jumps late in the key order, far beyond the 2^8 lazy-rescale threshold: a key aligned with a query in a
    middle tile, one in the (ragged, for 20 x 28) last tile, one that hits only one of a wave's two query tiles."""
    from protosam_amd import ops
    B, H = 1, 2
    N = gh * gw
    qkv = _rand((B, N, 3, H, hd), dev, 0.4, 9)
    for (qi, ki, gain) in ((17, N - 3, 40.0), (40, N // 2 + 5, 25.0), (N - 2, 130, 60.0)):
        qkv[0, ki, 1, 0] = qkv[0, qi, 0, 0] * gain
    qkv = qkv.half()
    Rh = _rand((2 * gh - 1, hd), dev, 0.3, 14)
    Rw = _rand((2 * gw - 1, hd), dev, 0.3, 15)
    scale = hd ** -0.5
    out = ops.attention(qkv, B, N, H, hd, scale, mode=1, rpack=ops.pack_rel_tables(Rh, Rw, False, hd), gh=gh, gw=gw)
    ref = _ref_relpos_attention(qkv, Rh, Rw, gh, gw, scale)
    print(f"spiky {gh}x{gw} hd{hd}: max abs err {(out.double() - ref).abs().max().item():.2e}")
    assert torch.isfinite(out.float()).all()
    torch.testing.assert_close(out.double(), ref, rtol=2e-3, atol=2e-3)


@pytest.mark.parametrize("H,hd,B", [(2, 64, 1), (12, 64, 2), (16, 80, 1), (3, 80, 3)])
def test_nothing_moves_at_64(dev, H, hd, B):
    """gw == 64: `ops.attention(mode=1, rel_h=, rel_w=)` on the default dispatch agrees with the HIP mode-1 kernels selected through
    `attention_set_variant` (9: register-staged, 17: DMA-fed) within 2e-3, as test_attention_softmax_variants_agree checks; the
    any-size kernel, reached at gw == 64 through variant bit 5 with the packed tables alone, is held to the same bound against them
    and against float64."""
    from protosam_amd import ops
    g = 64
    N = g * g
    qkv = _rand((B, N, 3, H, hd), dev, 1.0, 51).half()
    Rh = _rand((2 * g - 1, hd), dev, 0.3, 52)
    Rw = _rand((2 * g - 1, hd), dev, 0.3, 53)
    scale = hd ** -0.5
    rp = ops.pack_rel_tables(Rh, Rw, False, hd)
    rel_h, rel_w = ops.relpos(qkv, rp, B, N, H, hd, g, g, False, scale)
    assert ops.attention_last_kernel() == ops.ATTN_KERNEL_RELPOS | ops.ATTN_KERNEL_QT4
    kw = dict(mode=1, rel_h=rel_h, rel_w=rel_w, gh=g, gw=g)
    default = ops.attention(qkv, B, N, H, hd, scale, **kw).float()
    assert ops.attention_last_kernel() == ops.ATTN_KERNEL_ASM_REL                    # the default dispatch: the assembly kernel
    outs = {}
    lands = {9: ops.ATTN_KERNEL_ATTN | ops.ATTN_KERNEL_FULL | ops.ATTN_KERNEL_V2, 17: ops.ATTN_KERNEL_GATTN | ops.ATTN_KERNEL_FULL}
    for v in (9, 17):
        ops.attention_set_variant(v)
        try:
            outs[v] = ops.attention(qkv, B, N, H, hd, scale, **kw).float()
            got = ops.attention_last_kernel()
        finally:
            ops.attention_set_variant(5)
        assert got == lands[v], (v, ops.attention_kernel_name(got))
    ops.attention_set_variant(5 | 32)
    try:
        anyk = ops.attention(qkv, B, N, H, hd, scale, mode=1, rpack=rp, gh=g, gw=g).float()
        got = ops.attention_last_kernel()
    finally:
        ops.attention_set_variant(5)
    assert got == ops.ATTN_KERNEL_GATTN_ANY | ops.ATTN_KERNEL_FULL | ops.ATTN_KERNEL_STAGE64, ops.attention_kernel_name(got)
    ref = _ref_relpos_attention(qkv, Rh, Rw, g, g, scale)
    print(f"H{H} hd{hd} B{B} at 64 x 64: default vs variants 9 / 17 "
          + " / ".join(f"{(default - outs[v]).abs().max().item():.2e}" for v in (9, 17))
          + f"; any-size kernel vs 9 / 17 / float64 {(anyk - outs[9]).abs().max().item():.2e} / "
          f"{(anyk - outs[17]).abs().max().item():.2e} / {(anyk.double() - ref).abs().max().item():.2e}")
    for v in (9, 17):
        torch.testing.assert_close(default, outs[v], rtol=2e-3, atol=2e-3)
        torch.testing.assert_close(anyk, outs[v], rtol=2e-3, atol=2e-3)
    torch.testing.assert_close(anyk.double(), ref, rtol=2e-3, atol=2e-3)
    assert torch.equal(ops.attention(qkv, B, N, H, hd, scale, **kw).float(), default)    # bit 5 cleared: the default dispatch again
    assert ops.attention_last_kernel() == ops.ATTN_KERNEL_ASM_REL


def test_larger_maps_stay_an_argument_error(dev):
    from protosam_amd import ops
    H, hd = 2, 64
    for gh, gw in ((65, 65), (64, 65), (65, 32)):
        N = gh * gw
        qkv = torch.zeros((1, N, 3, H, hd), dtype=torch.float16, device=dev)
        rp = ops.pack_rel_tables(torch.zeros((127, hd), device=dev), torch.zeros((127, hd), device=dev), False, hd)
        with pytest.raises(RuntimeError):
            ops.attention(qkv, 1, N, H, hd, hd ** -0.5, mode=1, rpack=rp, gh=gh, gw=gw)
    assert not ops.attention_fused_relpos(1, 1024, 12, 64, 32, 32)           # (answers for the 64 x 64 map only)


# ---- modules against the reference's record -------------------------------------------------------------------------------


def _load(mod, dev, seed=None):
    from protosam_amd import synth_cases as gi
    from protosam_amd.synth import synth_state_dict
    mod.load_state_dict(synth_state_dict(mod, gi.MODULE_SEED if seed is None else seed))
    return mod.to(dev).eval()


def _rel(got, ref):
    ref = torch.as_tensor(ref)
    return float((got.detach().float().cpu() - ref).abs().max() / ref.pow(2).mean().sqrt())


@pytest.mark.parametrize("name,ws", [("window", 14), ("global", 0)])
def test_block_forward_g32(dev, gold, name, ws):
    from protosam_amd import anysize_cases as ac
    from protosam_amd.segment_anything.modeling.image_encoder import Block
    blk = _load(Block(ac.DIM, ac.HEADS, 4.0, True, partial(torch.nn.LayerNorm, eps=1e-6), torch.nn.GELU, True, True, ws, (32, 32)), dev)
    x = ac.block_input().to(dev)
    y = blk(x)
    e = _rel(y[0, 3::8, 5::8], gold[f"block_{name}_g32"])
    print(f"Block.forward at 32 x 32 ({name}): max err / rms {e:.2e}")
    assert y.shape == x.shape and y.dtype == torch.float32
    assert e < 4e-3


def test_attention_forward_g32_and_mismatches(dev, gold):
    from protosam_amd import anysize_cases as ac
    from protosam_amd.segment_anything.modeling.image_encoder import Attention, Block, ImageEncoderViT
    att = _load(Attention(ac.DIM, num_heads=ac.HEADS, qkv_bias=True, use_rel_pos=True, input_size=(32, 32)), dev)
    y = att(ac.block_input().to(dev))
    e = _rel(y[0, 3::8, 5::8], gold["enc_attention_g32"])
    print(f"image_encoder.Attention.forward at 32 x 32: max err / rms {e:.2e}")
    assert y.shape == (1, 32, 32, ac.DIM) and e < 4e-3
    # a map whose side does not match the module's own tables keeps raising
    with pytest.raises(NotImplementedError):
        att(torch.zeros((1, 64, 64, ac.DIM), device=dev))
    with pytest.raises(NotImplementedError):
        att(torch.zeros((25, 14, 14, ac.DIM), device=dev))
    with pytest.raises(NotImplementedError):
        att(torch.zeros((1, 32, 24, ac.DIM), device=dev))
    blk = _load(Block(ac.DIM, ac.HEADS, 4.0, True, partial(torch.nn.LayerNorm, eps=1e-6), torch.nn.GELU, True, True, 0, (32, 32)), dev)
    with pytest.raises(NotImplementedError):
        blk(torch.zeros((1, 48, 48, ac.DIM), device=dev))
    with pytest.raises(NotImplementedError):
        ImageEncoderViT(img_size=65 * 16, embed_dim=ac.DIM, depth=2, num_heads=ac.HEADS, use_rel_pos=True, window_size=14,
                        global_attn_indexes=(1,))
    big = _load(Attention(ac.DIM, num_heads=ac.HEADS, qkv_bias=True, use_rel_pos=True, input_size=(65, 65)), dev)
    with pytest.raises(NotImplementedError):
        big(torch.zeros((1, 65, 65, ac.DIM), device=dev))


@pytest.mark.parametrize("case", ["vitb_512", "vitb_384", "vith_512"])
def test_image_encoder_any_size(dev, gold, case):
    """`ImageEncoderViT(img_size=...)`, depth 2 (one windowed + one global block): ViT-B width (12 heads of 64) at 512 and 384
    pixels (32 x 32 and 24 x 24 maps), ViT-H width (16 heads of 80) at 512."""
    from protosam_amd import anysize_cases as ac
    enc = _load(ac.build_encoder(case), dev, ac.ENCODER_SEED)
    x = ac.encoder_input(case).to(dev)
    y = enc(x)
    g = enc.grid
    ref = torch.from_numpy(gold[f"encoder_{case}"])
    assert y.shape == (1, 256, g, g)
    d = (y[0, :, 3::8, 5::8].float().cpu() - ref).abs()
    print(f"ImageEncoderViT {case}: {g} x {g} map, max err {d.max().item():.2e}, mean {d.mean().item():.2e} "
          f"(embedding rms {ref.pow(2).mean().sqrt().item():.2f})")
    assert d.max().item() < 5e-2 and d.mean().item() < 3e-3


def test_image_encoder_512_graph_replay_bit_exact(dev, monkeypatch):
    """A graph-captured 512-pixel encoder replays to the same bits as the eager run."""
    from protosam_amd import anysize_cases as ac
    from protosam_amd import ops
    enc = _load(ac.build_encoder("vitb_512"), dev, ac.ENCODER_SEED)
    x = ac.encoder_input("vitb_512").to(dev)
    P = enc.patch_size
    patches = ops.patchify_bilinear(x.float().contiguous(), enc.img_size, P, 3 * P * P)
    eager = enc._encode_patches(patches, 1).clone()
    monkeypatch.setenv("PSAM_HIPGRAPH", "auto")         # (the default: one or two images go through a captured graph)
    assert ops.graph_wanted(patches, 2 * enc.grid * enc.grid)
    a = enc.encode_patches(patches, 1).clone()          # captures
    b = enc.encode_patches(patches, 1).clone()          # replays
    assert "_graphs" in enc.__dict__
    assert torch.equal(a, eager) and torch.equal(b, eager)


def test_predictor_512(dev, gold):
    """`SamPredictor.set_image / predict` on a 512-pixel `Sam` (ViT-B width, two blocks): points + box, multimask on and off, one
    non-square image."""
    from protosam_amd import anysize_cases as ac
    from protosam_amd.segment_anything import SamPredictor
    sam = _load(ac.build_sam_512(), dev, ac.SAM_SEED)
    assert sam.image_encoder.img_size == 512 and sam.prompt_encoder.image_embedding_size == (32, 32)
    pred = SamPredictor(sam)
    for name, img, prompts in ac.predictor_cases():
        pred.set_image(img)
        for mm in (True, False):
            masks, iou, low = pred.predict(multimask_output=mm, return_logits=False, **prompts)
            pre = f"pred_{name}_mm{int(mm)}"
            ref_low, ref_iou = torch.from_numpy(gold[pre + "_low"]), gold[pre + "_iou"]
            assert masks.shape == ((3 if mm else 1),) + img.shape[:2] and low.shape[-2:] == (128, 128)
            perr = (torch.sigmoid(torch.as_tensor(low)[..., ::2, ::2].float()) - torch.sigmoid(ref_low)).abs().max().item()
            ierr = float(np.abs(np.asarray(iou) - ref_iou).max())
            print(f"{pre}: max |dprob(low_res)| {perr:.2e}, iou {ierr:.2e}")
            assert perr < TOL_PROB and ierr < 1e-3
