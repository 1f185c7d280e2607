"""GPU parity of the SAM stage (image encoder, prompt encoder, mask decoder, post-processing, predictor API)
against the CPU oracle (which is pinned to the vendored reference modules, see tests/test_oracle_golden.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _sam(dev, model_type, depth, seed=1234):
    from protosam_amd.segment_anything import sam_model_registry
    from protosam_amd.synth import synth_state_dict
    sam = sam_model_registry[model_type](encoder_depth=depth)
    sd = synth_state_dict(sam, seed)
    sam.load_state_dict(sd, strict=True)
    return sam.to(dev).eval(), sd


def _image(seed=0):
    from protosam_amd.synth import synth_pair
    _, _, q, _ = synth_pair(1024, seed=seed)
    q = (q - q.min()) / (q.max() - q.min()) * 255
    return q.to(torch.uint8)  # [1,3,1024,1024]


def _normalised(img):
    return (img.float() - torch.tensor([123.675, 116.28, 103.53]).view(1, 3, 1, 1)) / torch.tensor([58.395, 57.12, 57.375]).view(1, 3, 1, 1)


@pytest.fixture(scope="module")
def oracle_embedding():
    """(model_type, depth, image seed) -> the fp32 CPU oracle's embedding [1,256,64,64] of _image(seed) under _sam's default weights
    (seed 1234), computed once per module (one ViT-L image of 6 blocks: a few seconds on the CPU)."""
    from oracle import sam_image_encoder as oenc
    from protosam_amd.synth import synth_state_dict
    from protosam_amd.segment_anything import sam_model_registry
    cache = {}

    def get(model_type, depth, seed):
        if (model_type, depth, seed) not in cache:
            sd = synth_state_dict(sam_model_registry[model_type](encoder_depth=depth), 1234)
            cache[(model_type, depth, seed)] = oenc.image_encoder(_normalised(_image(seed)), sd, model_type=model_type, depth=depth)
        return cache[(model_type, depth, seed)]
    return get


@pytest.mark.parametrize("model_type,depth", [("vit_b", 3), ("vit_h", 8),
                                              ("vit_l", 6)])    # ViT-L: windowed blocks 0-4 and the global block 5, 16 heads of 64
def test_image_encoder(dev, oracle_embedding, model_type, depth):
    sam, sd = _sam(dev, model_type, depth)
    img = _image(1)
    x = _normalised(img)
    ref = oracle_embedding(model_type, depth, 1)
    xin = sam.preprocess(img.to(dev))
    torch.testing.assert_close(xin.cpu(), x, rtol=1e-6, atol=1e-6)
    out = sam.image_encoder(xin)
    assert out.shape == (1, 256, 64, 64)
    err = (out.cpu() - ref).abs()
    print(f"{model_type} depth {depth}: max abs err {err.max():.3e} mean {err.mean():.3e} ref rms {ref.pow(2).mean().sqrt():.3f}")
    assert err.max() < 5e-2 and err.mean() < 3e-3


def _cases():
    from protosam_amd import synth_cases as gi
    return gi.decoder_cases()


@pytest.mark.parametrize("name", ["pts_box", "pts_only", "box_only"])
def test_prompt_encoder_and_mask_decoder(dev, name):
    from oracle import sam_prompt_decoder as odec
    from protosam_amd import synth_cases as gi
    sam, sd = _sam(dev, "vit_b", 0)
    feats = gi.decoder_features()
    pc, pl, bx = _cases()[name]
    pts = (pc, pl) if pc is not None else None
    sp_r, de_r = odec.prompt_encoder(sd, pts, bx)
    pe_r = odec.dense_pe(sd)
    dpts = (pc.to(dev), pl.to(dev)) if pc is not None else None
    sp, de = sam.prompt_encoder(points=dpts, boxes=None if bx is None else bx.to(dev), masks=None)
    torch.testing.assert_close(sp.cpu(), sp_r, rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(de.cpu(), de_r, rtol=0, atol=0)
    pe = sam.prompt_encoder.get_dense_pe()
    torch.testing.assert_close(pe.cpu(), pe_r, rtol=1e-4, atol=2e-5)
    for mm in (True, False):
        taps = {}
        low_r, iou_r = odec.mask_decoder(sd, feats, pe_r, sp_r, de_r, mm, taps=taps)
        low, iou = sam.mask_decoder(image_embeddings=feats.to(dev), image_pe=pe, sparse_prompt_embeddings=sp,
                                    dense_prompt_embeddings=de, multimask_output=mm)
        assert low.shape == low_r.shape and iou.shape == iou_r.shape
        lerr = (low.cpu() - low_r).abs().max().item()
        perr = (torch.sigmoid(low.cpu()) - torch.sigmoid(low_r)).abs().max().item()
        ierr = (iou.cpu() - iou_r).abs().max().item()
        print(f"{name} multimask={mm}: |dlogit| {lerr:.3e} (|logit| max {low_r.abs().max():.2f}), |dprob| {perr:.3e}, |diou| {ierr:.3e}")
        # the decoder's 4096-token projections run at fp32 accuracy (psam_gemm_f32x3 / psam_gemm_f32); the decoder and each of its
        # kernels are bounded much tighter against float64 in tests/test_decoder_kernels_gpu.py (<= 1.7e-6 on sigmoid(low_res) there)
        assert perr < 1e-3 and ierr < 1e-3


@pytest.mark.parametrize("variant", ["upstream", "batched", "nearest"])
def test_postprocess_variants(dev, variant):
    from oracle import sam_prompt_decoder as odec
    from protosam_amd import ops
    sam, _ = _sam(dev, "vit_b", 0)
    sam.postprocess_variant = variant
    g = torch.Generator().manual_seed(4)
    low = torch.randn((2, 3, 256, 256), generator=g) * 4
    ref = odec.postprocess_masks(low, (1024, 1024), (1024, 1024), variant)
    out = sam.postprocess_masks(low.to(dev), (1024, 1024), (1024, 1024))
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-5, atol=1e-5)
    # fused union + nearest to 512 (ProtoSAM.py:669-676)
    pred = ops.mask_union(low.to(dev), 1, 1024, 512, sam.variant_id())
    refu = ((ref[:, 1] > 0).sum(0) > 0).float()
    refu = torch.nn.functional.interpolate(refu[None, None], size=512, mode="nearest")[0, 0]
    assert (pred.cpu() != refu).sum().item() <= 2


def test_predictor_api(dev):
    from oracle import glue, sam_image_encoder as oenc, sam_prompt_decoder as odec
    from protosam_amd.segment_anything import SamPredictor
    sam, sd = _sam(dev, "vit_b", 2)
    pred = SamPredictor(sam)
    with pytest.raises(RuntimeError):
        pred.predict(point_coords=np.array([[1.0, 2.0]]), point_labels=np.array([1]))
    img = _image(2)[0].permute(1, 2, 0).numpy()  # HWC uint8
    pred.set_image(img)
    feats_ref = oenc.image_encoder(glue.sam_preprocess(img), sd, model_type="vit_b", depth=2)
    emb = pred.get_image_embedding()
    assert (emb.cpu() - feats_ref).abs().max() < 5e-2
    pts, lbl, box = np.array([[400.0, 500.0], [520.5, 480.0]]), np.array([1, 1]), np.array([300, 350, 700, 800])
    masks, iou, low = pred.predict(point_coords=pts, point_labels=lbl, box=box, multimask_output=True)
    m_r, iou_r, low_r = odec.predict(sd, emb.cpu().contiguous(), pts, lbl, box, True, (1024, 1024))
    assert masks.shape == (3, 1024, 1024) and masks.dtype == np.bool_ and low.shape == (3, 256, 256)
    assert (torch.sigmoid(torch.from_numpy(low)) - torch.sigmoid(low_r)).abs().max() < 1e-3
    assert np.abs(iou - iou_r.numpy()).max() < 1e-3
    assert (masks != m_r.numpy()).mean() < 1e-3  # sign flips of near-zero logits only


def test_mask_prompt_embedding_and_predict(dev):
    """PromptEncoder.mask_downscaling (one HIP kernel) and the decoder fed with per-prompt dense maps, against the
    REFERENCE's recorded outputs (dec_mask_* in tests/golden/reference_outputs.npz) and the oracle."""
    import os
    from oracle import sam_prompt_decoder as odec
    from protosam_amd import synth_cases as gi
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_outputs.npz"))
    sam, sd = _sam(dev, "vit_b", 1, seed=gi.DECODER_SEED)
    mk = gi.mask_prompt_case()
    sparse, dense = sam.prompt_encoder(points=None, boxes=None, masks=mk.to(dev))
    assert sparse.shape == (2, 0, 256) and dense.shape == (2, 256, 64, 64)
    ref = odec.embed_masks(sd, mk)
    err = (dense.cpu() - ref).abs().max().item()
    print(f"mask_downscaling: max abs err {err:.3e} (|ref| max {ref.abs().max():.1f})")
    assert err < 1e-3 * max(1.0, ref.abs().max().item())
    np.testing.assert_allclose(dense.cpu()[:, :, ::8, ::8].numpy(), gold["dec_mask_dense"], atol=2e-3, rtol=1e-4)
    feats = gi.decoder_features().to(dev)
    low, iou = sam.mask_decoder(image_embeddings=feats, image_pe=sam.prompt_encoder.get_dense_pe(),
                                sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense, multimask_output=True)
    e_low = (torch.sigmoid(low.cpu()) - torch.sigmoid(torch.from_numpy(gold["dec_mask_low_res"]))).abs().max().item()
    e_iou = np.abs(iou.cpu().numpy() - gold["dec_mask_iou"]).max()
    print(f"decoder with mask prompts vs reference: max |dprob| {e_low:.3e}, iou {e_iou:.3e}")
    assert e_low < 1e-3 and e_iou < 1e-3
    with pytest.raises(ValueError):
        sam.prompt_encoder(points=None, boxes=None, masks=torch.zeros((1, 1, 128, 128), device=dev))


@pytest.mark.parametrize("hw", [(600, 900), (1024, 768), (300, 300)])
def test_predictor_arbitrary_image_size(dev, hw):
    """SamPredictor on images that are not 1024x1024: PIL resize of the long side, zero padding after normalisation, prompt
    coordinates scaled by ResizeLongestSide, mask logits cropped and resized back (predictor.py:34-90,92-241; sam.py:132-173)."""
    from oracle import glue, sam_image_encoder as oenc, sam_prompt_decoder as odec
    from protosam_amd.segment_anything import SamPredictor
    sam, sd = _sam(dev, "vit_b", 2)
    rng = np.random.RandomState(hw[0])
    import scipy.ndimage as ndi
    img = np.stack([ndi.gaussian_filter(rng.rand(*hw), 6 + c) for c in range(3)], -1)
    img = ((img - img.min()) / (img.max() - img.min()) * 255).astype(np.uint8)
    pred = SamPredictor(sam)
    pred.set_image(img)
    pts = np.array([[hw[1] * 0.4, hw[0] * 0.5], [hw[1] * 0.6, hw[0] * 0.3]])
    lab = np.array([1, 0])
    box = np.array([hw[1] * 0.2, hw[0] * 0.1, hw[1] * 0.8, hw[0] * 0.9])
    masks, iou, low = pred.predict(point_coords=pts, point_labels=lab, box=box, multimask_output=True)
    assert masks.shape == (3,) + hw and masks.dtype == bool and low.shape == (3, 256, 256)
    # oracle
    rz = glue.apply_image(img)
    assert tuple(rz.shape[:2]) == tuple(pred.input_size) and max(rz.shape[:2]) == 1024
    feats = oenc.image_encoder(glue.sam_preprocess(rz), sd, model_type="vit_b", depth=2)
    m_ref, iou_ref, low_ref = odec.predict(sd, feats, pts, lab, box, True, hw, input_size=tuple(rz.shape[:2]))
    perr = (torch.sigmoid(torch.from_numpy(low)) - torch.sigmoid(low_ref)).abs().max().item()
    d = min(2.0 * (masks[c] & m_ref[c].numpy()).sum() / max(masks[c].sum() + m_ref[c].numpy().sum(), 1) for c in range(3)
            if m_ref[c].any())
    print(f"{hw}: input {pred.input_size}, max |dprob(low_res)| {perr:.2e}, iou err {np.abs(iou - iou_ref.numpy()).max():.2e}, "
          f"min Dice {d:.5f}")
    assert perr < 1e-3 and np.abs(iou - iou_ref.numpy()).max() < 1e-3 and d > 0.99


def test_image_encoder_rel_pos_table_resize(dev):
    """`get_rel_pos` (image_encoder.py:303-334): a rel-pos table whose length is not 2K - 1 is linearly resized. Block 0
    (windowed, K = 14) gets 63-row tables, block 2 (global, K = 64) 41-row ones; the oracle takes the reference's resize path."""
    from oracle import sam_image_encoder as oenc
    from protosam_amd.synth import synth_tensor
    sam, sd = _sam(dev, "vit_b", 3)
    enc = sam.image_encoder
    hd = enc.embed_dim // enc.num_heads
    for bi, L in ((0, 63), (2, 41)):
        for nm in ("rel_pos_h", "rel_pos_w"):
            t = synth_tensor(f"resized.{bi}.{nm}", (L, hd), 99)
            sd[f"image_encoder.blocks.{bi}.attn.{nm}"] = t
            setattr(enc.blocks[bi].attn, nm, torch.nn.Parameter(t.to(dev)))
    enc._packed = None
    img = _image(3)
    x = (img.float() - torch.tensor([123.675, 116.28, 103.53]).view(1, 3, 1, 1)) / torch.tensor(
        [58.395, 57.12, 57.375]).view(1, 3, 1, 1)
    ref = oenc.image_encoder(x, sd, model_type="vit_b", depth=3)
    out = sam.image_encoder(sam.preprocess(img.to(dev)))
    err = (out.cpu() - ref).abs()
    print(f"resized rel-pos tables: max abs err {err.max():.3e} mean {err.mean():.3e}")
    assert err.max() < 5e-2 and err.mean() < 3e-3


@pytest.mark.parametrize("model_type,depth", [("vit_b", 3), ("vit_l", 6)])
def test_image_encoder_folded_layernorm_path(dev, oracle_embedding, model_type, depth):
    """`fold_ln = True` (LayerNorm folded into the GEMMs either side of it, psam_gemm_f16_ln) against the oracle and against
    the default path with the separate LayerNorm passes."""
    sam, sd = _sam(dev, model_type, depth)
    img = _image(4)
    ref = oracle_embedding(model_type, depth, 4)
    xin = sam.preprocess(img.to(dev))
    outs = {}
    default = sam.image_encoder.fold_ln
    sam.image_encoder.fold_min_fill = 0.0          # (one image is below the size where the fold is switched on by itself)
    for fold in (False, True):
        sam.image_encoder.fold_ln = fold
        outs[fold] = sam.image_encoder(xin).cpu().clone()
    sam.image_encoder.fold_ln = default
    sam.image_encoder.fold_min_fill = 0.8
    for fold, o in outs.items():
        err = (o - ref).abs()
        print(f"{model_type} depth {depth} fold_ln={fold}: max abs err {err.max():.3e} mean {err.mean():.3e}")
        assert err.max() < 5e-2 and err.mean() < 3e-3
    assert (outs[True] - outs[False]).abs().max() < 5e-2


def test_image_encoder_split_fp16_neck_and_patch_embedding(dev):
    """Round 5 (`split_fp16`): the neck's two GEMMs on (hi, lo) fp16 pairs of activations and weights, the patch embedding on the exact
    uint8 pixel values against split weights with Sam.preprocess' normalisation folded in (image_encoder.py:90-122, sam.py:163-168).
    On a 0-block encoder (patch embedding + neck only) the embedding has to match the fp32 oracle far below the plain fp16-operand path;
    with blocks in between it must not be worse; the [0 ... 255] hand-off equals the normalised-pixel route up to that rounding."""
    from oracle import sam_image_encoder as oenc
    from protosam_amd import ops
    for depth, bound in ((0, 5e-4), (3, 5e-2)):
        sam, sd = _sam(dev, "vit_b", depth)
        enc = sam.image_encoder
        img = _image(5)                                                     # uint8-valued [1,3,1024,1024]
        x = (img.float() - torch.tensor([123.675, 116.28, 103.53]).view(1, 3, 1, 1)) / torch.tensor(
            [58.395, 57.12, 57.375]).view(1, 3, 1, 1)
        ref = oenc.image_encoder(x, sd, model_type="vit_b", depth=depth)    # [1,256,64,64]
        errs = {}
        for split in (False, True):
            enc.split_fp16 = split
            if split:      # raw pixel values, normalisation inside the weights (what ProtoSAM._sam_features hands over)
                patches = ops.patchify_bilinear(img.float().to(dev).contiguous(), 1024, 16, 768)
                tok = enc.encode_patches(patches, 1, raw_norm=(sam._mean_host, sam._std_host))
            else:
                tok = enc.forward_tokens(sam.preprocess(img.to(dev)))
            out = tok.view(1, 64, 64, 256).permute(0, 3, 1, 2).cpu()
            errs[split] = (out - ref).abs()
        enc.split_fp16 = True
        print(f"depth {depth}: plain fp16 operands max {errs[False].max():.3e} mean {errs[False].mean():.3e}; "
              f"split neck + exact-pixel patch embedding max {errs[True].max():.3e} mean {errs[True].mean():.3e}")
        assert errs[True].max() < bound
        assert errs[True].mean() <= errs[False].mean() * (0.25 if depth == 0 else 1.02)


@pytest.mark.parametrize("model_type,depth", [("vit_b", 3), ("vit_h", 4), ("vit_l", 6)])
def test_image_encoder_reference_width_mode(dev, model_type, depth):
    """Round 6 (`gemm_x3`, PSAM_ENCODER_X3=1): every Linear of the blocks at fp32 accuracy (fp32 operands and results, psam_gemm_f32x3),
    LayerNorm / GELU as fp32 passes, split neck + exact-pixel patch embedding; only QK^T / PV keep fp16 operands. Against the fp32 oracle
    the embedding error has to drop well below the fp16-operand default's (what remains is the attention's operand rounding)."""
    from oracle import sam_image_encoder as oenc
    from protosam_amd import ops
    sam, sd = _sam(dev, model_type, depth)
    enc = sam.image_encoder
    img = _image(6)
    x = (img.float() - torch.tensor([123.675, 116.28, 103.53]).view(1, 3, 1, 1)) / torch.tensor(
        [58.395, 57.12, 57.375]).view(1, 3, 1, 1)
    ref = oenc.image_encoder(x, sd, model_type=model_type, depth=depth)
    patches = ops.patchify_bilinear(img.float().to(dev).contiguous(), 1024, 16, 768)
    errs = {}
    for x3 in (False, True):
        enc.gemm_x3 = x3
        if x3:
            tok = enc.encode_patches(patches, 1, raw_norm=(sam._mean_host, sam._std_host))
        else:
            tok = enc.forward_tokens(sam.preprocess(img.to(dev)))
        errs[x3] = (tok.view(1, 64, 64, 256).permute(0, 3, 1, 2).cpu() - ref).abs()
    enc.gemm_x3 = False
    print(f"{model_type} depth {depth}: fp16 operands max {errs[False].max():.3e} mean {errs[False].mean():.3e}; reference-width GEMMs "
          f"max {errs[True].max():.3e} mean {errs[True].mean():.3e} (ref rms {ref.pow(2).mean().sqrt():.3f})")
    assert errs[True].mean() < 0.5 * errs[False].mean() and errs[True].max() < errs[False].max()
    h = torch.randn((1000, 64), generator=torch.Generator().manual_seed(1)).half().to(dev)
    assert torch.equal(ops.cast_f32(h), h.float())
    g = torch.randn((1000, 64), generator=torch.Generator().manual_seed(2)).to(dev) * 3
    torch.testing.assert_close(ops.gelu_f32_(g.clone()), torch.nn.functional.gelu(g), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("model_type,depth", [("vit_h", 3), ("vit_l", 6)])
def test_image_encoder_splitk_lin2_option(dev, oracle_embedding, model_type, depth):
    """`splitk_lin2` (PSAM_SPLITK_LIN2=1, round 6): one image with mlp.lin2 as K ranges of the assembly tile and the next block's norm1
    fused into the reduce pass (ops.gemm_splitk_ln) - same products in another summation order: the embedding agrees with the default path
    far inside the fp16-operand error, and with the oracle as well as the default does; eager and graph replay agree bit for bit."""
    from protosam_amd import ops
    sam, sd = _sam(dev, model_type, depth)
    enc = sam.image_encoder
    D = enc.embed_dim
    ks = ops.gemm_splitk_ranges(4096, D, 4 * D)
    print(f"{model_type}: mlp.lin2 of one image in {ks} K ranges")
    assert ks >= 2
    img = _image(7)
    ref = oracle_embedding(model_type, depth, 7)
    xin = sam.preprocess(img.to(dev))
    outs = {}
    for sk in (False, True):
        enc.splitk_lin2 = sk
        outs[sk] = enc(xin).cpu().clone()
    a = enc(xin).cpu().clone()                       # (second call: the captured graph of the split-K form, if graphs are on)
    enc.splitk_lin2 = False
    assert torch.equal(a, outs[True])
    d = (outs[True] - outs[False]).abs().max().item()
    e0, e1 = (outs[False] - ref).abs(), (outs[True] - ref).abs()
    print(f"{model_type} depth {depth} splitk_lin2: max |difference to the default path| {d:.2e}; vs oracle: default max {e0.max():.3e} mean {e0.mean():.3e}, split-K max {e1.max():.3e} mean {e1.mean():.3e}")
    # (another fp32 summation order flips fp16 roundings of the LayerNorm outputs downstream: the two paths differ from each other by what
    # either differs from the oracle - measured 2.1e-3 against 3.7e-3 / 3.6e-3)
    assert d < 5e-3 and e1.mean() < 1.05 * e0.mean() + 1e-6 and e1.max() < 5e-2


def test_image_encoder_two_images_vit_l(dev, oracle_embedding):
    """ViT-L (6 blocks) on a [2,3,1024,1024] batch: M = 8192 rows pick other GEMM kernels than one image does, so each image has to meet the
    oracle bounds on its own, and agree with its own one-image call to within the fp16-operand error (not bit for bit)."""
    sam, sd = _sam(dev, "vit_l", 6)
    enc = sam.image_encoder
    seeds = (1, 4)
    imgs = torch.cat([_image(s) for s in seeds]).to(dev)
    two = enc(sam.preprocess(imgs)).cpu().clone()
    assert two.shape == (2, 256, 64, 64)
    for i, s in enumerate(seeds):
        one = enc(sam.preprocess(imgs[i:i + 1])).cpu().clone()
        ref = oracle_embedding("vit_l", 6, s)[0]
        e2, e1, d = (two[i] - ref).abs(), (one[0] - ref).abs(), (two[i] - one[0]).abs()
        print(f"vit_l depth 6 image {i} of 2: max abs err {e2.max():.3e} mean {e2.mean():.3e}; alone: max {e1.max():.3e} mean {e1.mean():.3e}; "
              f"batch vs alone max {d.max():.3e} mean {d.mean():.3e}")
        assert e2.max() < 5e-2 and e2.mean() < 3e-3 and e1.max() < 5e-2 and e1.mean() < 3e-3
        assert d.max() < 5e-2 and d.mean() < 3e-3


def test_image_encoder_splitk_lin2_sub_batches_vit_l(dev, oracle_embedding):
    """Regression: with `splitk_lin2` on, ViT-L takes mlp.lin2 in split-K form at one image AND at two (more K ranges for one image), and the
    one-image workspace is built as views of the two-image one. A B = 2, B = 1, B = 2 sequence must give, call by call, bit for bit what a
    freshly built encoder with the same weights gives at that batch size alone (same kernels, same ks), and meet the oracle bounds. (The
    one-image call once inherited a truncated view of the two-image split-K scratch and failed gemm_splitk_ln's size check.)"""
    from protosam_amd import ops
    D, N = 1024, 4096
    ks = {B: ops.gemm_splitk_ranges(B * N, D, 4 * D) for B in (1, 2)}
    print(f"vit_l mlp.lin2 K ranges: {ks}")
    assert ks[1] >= 2 and ks[2] >= 2
    seeds = (1, 4)
    imgs = torch.cat([_image(s) for s in seeds])
    sam, sd = _sam(dev, "vit_l", 6)
    enc = sam.image_encoder
    enc.splitk_lin2 = True
    x = {2: sam.preprocess(imgs.to(dev)), 1: sam.preprocess(imgs[:1].to(dev))}
    got = [(B, enc(x[B]).cpu().clone()) for B in (2, 1, 2)]
    alone = {}
    for B in (2, 1):
        fresh, _ = _sam(dev, "vit_l", 6)
        fresh.image_encoder.splitk_lin2 = True
        alone[B] = fresh.image_encoder(x[B]).cpu().clone()
        del fresh
    for i, (B, out) in enumerate(got):
        assert torch.equal(out, alone[B]), (i, B, (out - alone[B]).abs().max().item())
        for b in range(B):
            e = (out[b] - oracle_embedding("vit_l", 6, seeds[b])[0]).abs()
            print(f"call {i} (B = {B}) image {b}: max abs err {e.max():.3e} mean {e.mean():.3e}")
            assert e.max() < 5e-2 and e.mean() < 3e-3
