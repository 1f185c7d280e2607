"""The cases of the encoder ladder tests (tests/test_encoder_ladder_cpu.py, tests/test_encoder_ladder_gpu.py): configurations, seeded
weights of two families, inputs, and the float64 reference / rounding-model outputs of oracle/encoder_model.py, each computed once per
process and shared (read-only) by every test that needs it. Test infrastructure only (see oracle/__init__.py).

A case runs at every depth d = 1 .. depth: weights are seeded by parameter name, so block i is the same in every one of those models,
and one forward of the deepest model yields what each shallower one returns (`all_depths`)."""
import functools

import torch

from . import encoder_model as EM

_DINO_B = dict(embed_dim=768, num_heads=12, num_register_tokens=0, interpolate_antialias=False, interpolate_offset=0.1)
_DINO_L_REG = dict(embed_dim=1024, num_heads=16, num_register_tokens=4, interpolate_antialias=True, interpolate_offset=0.0)


def _sam(D, H, grid, glob, oc=256):
    return dict(embed_dim=D, num_heads=H, grid=grid, window_size=14, global_attn_indexes=glob, patch_size=16, out_chans=oc)


# name -> kind, cfg, input side S, batch B, depth; `product`: what builds the HIP model (GPU ladder), None for the tiny CPU-only ones
CASES = {
    # 257 tokens = four 64-key tiles + ONE key; M = 514 = two 256-row tiles + 2
    "dino_b": dict(kind="dino", cfg=_DINO_B, S=224, B=2, depth=3, product="dinov2_vitb14"),
    # 261 tokens, 4 register rows
    "dino_l_reg": dict(kind="dino", cfg=_DINO_L_REG, S=224, B=1, depth=2, product="dinov2_vitl14_reg"),
    # 16 x 16 map: 2 x 2 padded windows, the any-map global kernel
    "sam_b16": dict(kind="sam", cfg=_sam(768, 12, 16, (2,)), S=256, B=2, depth=3, product="sam"),
    # ViT-H width, 64 x 64 map: the assembly window kernel, then the fused global assembly kernel
    "sam_h64": dict(kind="sam", cfg=_sam(1280, 16, 64, (1,)), S=1024, B=1, depth=2, product="sam"),
    # head dim 64 on the 64 x 64 map: wattn_p_kernel, psam_gattn_asm_64_fused
    "sam_b64": dict(kind="sam", cfg=_sam(768, 12, 64, (1,)), S=1024, B=1, depth=2, product="sam"),
    # tiny configurations (CPU file only): D = 128, two heads of 64, 5 x 5 and 16 x 16 maps
    "dino_tiny5": dict(kind="dino", cfg=dict(_DINO_B, embed_dim=128, num_heads=2), S=70, B=2, depth=2, product=None),
    "dino_tiny16_reg": dict(kind="dino", cfg=dict(_DINO_L_REG, embed_dim=128, num_heads=2), S=224, B=2, depth=2, product=None),
    "sam_tiny5": dict(kind="sam", cfg=_sam(128, 2, 5, (1,), 64), S=80, B=2, depth=2, product=None),
    "sam_tiny16": dict(kind="sam", cfg=_sam(128, 2, 16, (1,), 64), S=256, B=2, depth=2, product=None),
}
LADDER = tuple(k for k, c in CASES.items() if c["product"])
TINY = tuple(k for k, c in CASES.items() if not c["product"])
FAMILIES = ("plain", "heavy")
SAM_PRE = "image_encoder."


@functools.lru_cache(maxsize=None)
def state_dict(case, family):
    """fp32 state dict of the case's deepest model (hub names for DINOv2, `image_encoder.`-prefixed reference names for SAM)"""
    from protosam_amd import synth
    c = CASES[case]
    if c["kind"] == "dino":
        sd = EM.synth_sd(EM.dino_shapes(c["cfg"], c["depth"]))
        return synth.heavy_tail_dino_(sd) if family == "heavy" else sd
    sd = EM.synth_sd(EM.sam_shapes(c["cfg"], c["depth"], SAM_PRE))
    return synth.heavy_tail_sam_(sd) if family == "heavy" else sd


def state_dict_for_depth(case, family, d):
    """the deepest model's state dict without the blocks a model of d blocks does not have"""
    keep = tuple(f"blocks.{i}." for i in range(d, CASES[case]["depth"]))
    return {k: v for k, v in state_dict(case, family).items() if not any(s in k for s in keep)}


@functools.lru_cache(maxsize=None)
def image(case):
    """fp32 [B, 3, S, S]: z-scored synthetic slices (a smooth field with a bright organ)"""
    from protosam_amd.synth import synth_pair
    c = CASES[case]
    s_img, _, q_img, _ = synth_pair(c["S"], seed=11)
    return torch.cat([q_img, s_img], 0)[:c["B"]].contiguous()


def forward(case, family, d=None, **kw):
    """oracle/encoder_model.py's forward of the case (d: a model of d blocks; default the deepest)"""
    c = CASES[case]
    fn = EM.dino_forward if c["kind"] == "dino" else EM.sam_forward
    with torch.no_grad():
        return fn(image(case), state_dict(case, family), c["cfg"], c["depth"] if d is None else d, **kw)


@functools.lru_cache(maxsize=None)
def ref(case, family):
    """float64, un-rounded: a tuple, entry d - 1 the output of the model of d blocks"""
    return tuple(forward(case, family, all_depths=True))


@functools.lru_cache(maxsize=None)
def model(case, family, fold):
    """float64 with the product's fp16 roundings (`fold`: the LayerNorm placement) -> (outputs per depth, largest value handed to fp16)"""
    q = EM.Fp16()
    outs = tuple(forward(case, family, q=q, fold=fold, all_depths=True))
    return outs, q.peak
