"""`ResizeLongestSide` (models/segment_anything/utils/transforms.py:17-148): coordinate / box scaling, the target shape
rule and the image resizes. On the hot path every image is already 1024x1024 and resizing is the identity; `apply_image` sends
other sizes through PIL's bilinear resize on the host exactly as the reference does (`resize(to_pil_image(image), size)` is
`PIL.Image.resize(size[::-1], BILINEAR)`, :38; `SamPredictor.set_image` does the same on the device, ops.image_intake mode 1).
`apply_image_torch` is the antialiased torch resize (:62-92): device tensors go through `ops.resize_aa`, CPU tensors (host data
loading, as the reference's dataset code calls it) through stock `F.interpolate(antialias=True)`."""
from copy import deepcopy

import numpy as np
import torch
import torch.nn.functional as F


class ResizeLongestSide:
    def __init__(self, target_length, pixel_mean=(123.675, 116.28, 103.53), pixel_std=(58.395, 57.12, 57.375)):
        self.target_length = target_length
        self.pixel_mean = torch.Tensor(list(pixel_mean)).view(-1, 1, 1)
        self.pixel_std = torch.Tensor(list(pixel_std)).view(-1, 1, 1)

    @staticmethod
    def get_preprocess_shape(oldh, oldw, long_side_length):
        scale = long_side_length * 1.0 / max(oldh, oldw)
        newh, neww = oldh * scale, oldw * scale
        return (int(newh + 0.5), int(neww + 0.5))

    def apply_image(self, image):
        target = self.get_preprocess_shape(image.shape[0], image.shape[1], self.target_length)
        if target == tuple(image.shape[:2]):
            return np.array(image)
        from PIL import Image  # host-side, as in the reference (torchvision's PIL path)
        return np.array(Image.fromarray(image).resize((target[1], target[0]), Image.BILINEAR))

    def apply_image_torch(self, image):
        """transforms.py:62-92 for [H,W], [C,H,W] and [B,C,H,W] float tensors."""
        target = self.get_preprocess_shape(image.shape[-2], image.shape[-1], self.target_length)
        if target == tuple(image.shape[-2:]):
            return image
        if image.dim() not in (2, 3, 4):
            raise ValueError(f"apply_image_torch expects [H,W], [C,H,W] or [B,C,H,W], got {tuple(image.shape)}")
        x = image[(None,) * (4 - image.dim())]
        if image.is_cuda:
            from ... import ops
            y = ops.resize_aa(x.float().contiguous(), target[0], target[1])
        else:
            y = F.interpolate(x, target, mode="bilinear", align_corners=False, antialias=True)
        return y.reshape(tuple(image.shape[:-2]) + target)

    def apply_coords(self, coords, original_size):
        old_h, old_w = original_size
        new_h, new_w = self.get_preprocess_shape(original_size[0], original_size[1], self.target_length)
        coords = deepcopy(coords).astype(float)
        coords[..., 0] = coords[..., 0] * (new_w / old_w)
        coords[..., 1] = coords[..., 1] * (new_h / old_h)
        return coords

    def apply_boxes(self, boxes, original_size):
        return self.apply_coords(boxes.reshape(-1, 2, 2), original_size).reshape(-1, 4)

    def apply_coords_torch(self, coords, original_size):
        old_h, old_w = original_size
        new_h, new_w = self.get_preprocess_shape(original_size[0], original_size[1], self.target_length)
        coords = deepcopy(coords).to(torch.float)
        coords[..., 0] = coords[..., 0] * (new_w / old_w)
        coords[..., 1] = coords[..., 1] * (new_h / old_h)
        return coords

    def apply_boxes_torch(self, boxes, original_size):
        return self.apply_coords_torch(boxes.reshape(-1, 2, 2), original_size).reshape(-1, 4)

    def preprocess(self, x):
        """Normalise + zero-pad at the bottom and right (transforms.py:94-110); a 2-D input (a mask) is only padded."""
        if len(x.shape) != 2:
            dev = x.device
            x = (x - self.pixel_mean.to(dev)) / self.pixel_std.to(dev)
        h, w = x.shape[-2:]
        S = self.target_length
        if (h, w) == (S, S):
            return x
        if h > S or w > S:
            raise ValueError(f"preprocess expects inputs with sides <= {S}, got {(h, w)}")
        out = torch.zeros(tuple(x.shape[:-2]) + (S, S), dtype=x.dtype, device=x.device)    # F.pad(x, (0, padw, 0, padh))
        out[..., :h, :w] = x
        return out
