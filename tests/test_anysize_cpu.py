"""CPU: `build_sam_vit_{h,l,b}(image_size=...)` builds the state-dict keys and shapes that follow from the constructor arguments
(pos_embed [1,g,g,D], 2g - 1 table rows in the global blocks, 27 in the windowed ones), the default call builds today's 1024-pixel
model, sizes beyond a 64 x 64 token map raise, and the C header and the ctypes signatures still agree."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARCH = {"vit_b": (768, 12, 12, (2, 5, 8, 11)), "vit_l": (1024, 24, 16, (5, 11, 17, 23)), "vit_h": (1280, 32, 16, (7, 15, 23, 31))}


def _expected_encoder_shapes(dim, depth, heads, global_idx, image_size, window=14, patch=16, out=256):
    g, hd = image_size // patch, dim // heads
    s = {"pos_embed": (1, g, g, dim), "patch_embed.proj.weight": (dim, 3, patch, patch), "patch_embed.proj.bias": (dim,)}
    for i in range(depth):
        K = g if i in global_idx else window
        p = f"blocks.{i}."
        s.update({p + "norm1.weight": (dim,), p + "norm1.bias": (dim,), p + "norm2.weight": (dim,), p + "norm2.bias": (dim,),
                  p + "attn.rel_pos_h": (2 * K - 1, hd), p + "attn.rel_pos_w": (2 * K - 1, hd),
                  p + "attn.qkv.weight": (3 * dim, dim), p + "attn.qkv.bias": (3 * dim,),
                  p + "attn.proj.weight": (dim, dim), p + "attn.proj.bias": (dim,),
                  p + "mlp.lin1.weight": (4 * dim, dim), p + "mlp.lin1.bias": (4 * dim,),
                  p + "mlp.lin2.weight": (dim, 4 * dim), p + "mlp.lin2.bias": (dim,)})
    s.update({"neck.0.weight": (out, dim, 1, 1), "neck.1.weight": (out,), "neck.1.bias": (out,),
              "neck.2.weight": (out, out, 3, 3), "neck.3.weight": (out,), "neck.3.bias": (out,)})
    return s


def _build(name, **kw):
    from protosam_amd.segment_anything import sam_model_registry
    with torch.device("meta"):           # shapes only: no parameter storage for the 32 blocks of ViT-H
        return sam_model_registry[name](**kw)


@pytest.mark.parametrize("name,size", [("vit_b", 512), ("vit_h", 256), ("vit_l", 384)])
def test_state_dict_follows_image_size(name, size):
    dim, depth, heads, gidx = ARCH[name]
    sam = _build(name, image_size=size)
    g = size // 16
    enc = {k: tuple(v.shape) for k, v in sam.image_encoder.state_dict().items()}
    assert enc == _expected_encoder_shapes(dim, depth, heads, gidx, size)
    assert sam.image_encoder.img_size == size and sam.image_encoder.grid == g
    assert sam.prompt_encoder.image_embedding_size == (g, g) and sam.prompt_encoder.input_image_size == (size, size)
    assert sam.prompt_encoder.mask_input_size == (4 * g, 4 * g)
    # the prompt encoder's and the mask decoder's parameters do not depend on the image size
    ref = _build(name, encoder_depth=1)
    for part in ("prompt_encoder", "mask_decoder"):
        a = {k: tuple(v.shape) for k, v in getattr(sam, part).state_dict().items()}
        b = {k: tuple(v.shape) for k, v in getattr(ref, part).state_dict().items()}
        assert a == b


def test_default_build_is_todays_1024_model():
    sam = _build("vit_b")
    dim, depth, heads, gidx = ARCH["vit_b"]
    enc = {k: tuple(v.shape) for k, v in sam.image_encoder.state_dict().items()}
    assert enc == _expected_encoder_shapes(dim, depth, heads, gidx, 1024)
    assert list(enc) == list(_build("vit_b", image_size=1024).image_encoder.state_dict())          # same keys, same order
    assert enc["pos_embed"] == (1, 64, 64, 768) and enc["blocks.2.attn.rel_pos_h"] == (127, 64) and enc["blocks.0.attn.rel_pos_h"] == (27, 64)
    assert sam.image_encoder.img_size == 1024 and sam.prompt_encoder.image_embedding_size == (64, 64)
    trimmed = _build("vit_b", encoder_depth=2)                                                       # the present call forms stay
    assert len(trimmed.image_encoder.blocks) == 2


def test_loading_another_size_fails_strictly():
    """No silent interpolation: a 1024-pixel state dict does not load into a 512-pixel model."""
    from protosam_amd.segment_anything import sam_model_registry
    big = sam_model_registry["vit_b"](encoder_depth=3)
    small = sam_model_registry["vit_b"](encoder_depth=3, image_size=512)
    with pytest.raises(RuntimeError, match="size mismatch"):
        small.load_state_dict(big.state_dict())


@pytest.mark.parametrize("size", [1040, 1000, 0])
def test_sizes_without_a_kernel_raise(size):
    """More than 64 x 64 tokens, or a side that is not a multiple of the patch size."""
    with pytest.raises(NotImplementedError):
        _build("vit_b", image_size=size, encoder_depth=1)


def test_header_and_signatures_still_agree():
    from protosam_amd import _lib
    src = open(os.path.join(ROOT, "include", "protosam_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = re.findall(r"\bint\s+(psam_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert set(n for n, _ in protos) == set(_lib.SIGNATURES)
    for name, args in protos:
        assert len([a for a in args.split(",") if a.strip()]) == len(_lib.SIGNATURES[name]), name
    assert len(_lib.SIGNATURES["psam_attention_f16"]) == 18          # mode 1 took the new maps without a new argument
