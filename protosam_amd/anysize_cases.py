"""Seeded cases of tests/golden/reference_anysize.npz (SAM at input sizes other than 1024): shared by tools/make_anysize_goldens.py,
which runs them through the reference's modules, and tests/test_anysize_gpu.py, which runs them through ours. The builders take the
`modeling` namespace to build from (ours by default), so both sides are constructed by the same lines."""
from functools import partial

import torch

from .synth_cases import _randn, predictor_image

DIM, HEADS = 768, 12            # SAM ViT-B's block width (heads of 64)
ENCODER_SEED = 707
SAM_SEED = 808

# name -> (img_size, embed_dim, num_heads): depth 2 = one 14 x 14 windowed block + one global block
ENCODERS = {"vitb_512": (512, 768, 12), "vitb_384": (384, 768, 12), "vith_512": (512, 1280, 16)}


def block_input():
    """[1,32,32,768]: what a 512-pixel `ImageEncoderViT` hands to a block."""
    return _randn((1, 32, 32, DIM), 41)


def _ours():
    from .segment_anything import modeling
    return modeling


def build_encoder(case, modeling=None):
    m = modeling or _ours()
    size, dim, heads = ENCODERS[case]
    return m.ImageEncoderViT(depth=2, embed_dim=dim, img_size=size, mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                             num_heads=heads, patch_size=16, qkv_bias=True, use_rel_pos=True, global_attn_indexes=(1,),
                             window_size=14, out_chans=256)


def encoder_input(case):
    size = ENCODERS[case][0]
    return _randn((1, 3, size, size), 42 + size)


def build_sam_512(modeling=None):
    """A 512-pixel `Sam`: ViT-B width, two blocks (windowed + global), 32 x 32 embedding, 128 x 128 low-res masks."""
    m = modeling or _ours()
    return m.Sam(image_encoder=build_encoder("vitb_512", m),
                 prompt_encoder=m.PromptEncoder(embed_dim=256, image_embedding_size=(32, 32), input_image_size=(512, 512),
                                                mask_in_chans=16),
                 mask_decoder=m.MaskDecoder(num_multimask_outputs=3,
                                            transformer=m.TwoWayTransformer(depth=2, embedding_dim=256, mlp_dim=2048, num_heads=8),
                                            transformer_dim=256, iou_head_depth=3, iou_head_hidden_dim=256),
                 pixel_mean=[123.675, 116.28, 103.53], pixel_std=[58.395, 57.12, 57.375]).eval()


def predictor_cases():
    """(name, uint8 HWC image, `SamPredictor.predict` prompt arguments): a square image at the model's size with points + box, a
    non-square one (resized to a long side of 512, zero-padded) with a positive and a negative point."""
    import numpy as np
    return [
        ("sq_pts_box", predictor_image((512, 512), seed=5),
         dict(point_coords=np.array([[200.0, 250.0], [260.5, 240.0]]), point_labels=np.array([1, 1]), box=np.array([150, 175, 350, 400]))),
        ("rect_pts_neg", predictor_image((600, 900), seed=6),
         dict(point_coords=np.array([[360.0, 300.0], [540.0, 180.0]]), point_labels=np.array([1, 0]))),
    ]
