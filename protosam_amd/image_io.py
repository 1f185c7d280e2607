"""Image-file I/O in front of the hot path: a directory pair of images and masks of arbitrary sizes -> normalised, resized,
zero-padded batches on the device. The sibling of `slice_io.ScanSlices` for the reference's second kind of data.

Mirrors the inference side of `PolypDataset` (dataloaders/PolypDataset.py):
  * the listing of `__init__` (:116-155) and `filter_files_and_get_ds_mean_and_std` (:362-381): `.jpg` / `.png` images and `.png`
    masks of the two roots and of one level of sub-directories, each list sorted, paired by position; pairs whose image path holds
    an excluded dataset name, or whose image and mask differ in size, are dropped;
  * `cv2_loader` (:395-402) + `process_image_gt` with a `sam_trans` (:319-348, the only branch validation_protosam.py:306-308 uses):
    the [0, 255] float image and the {0, 1} mask go through `ResizeLongestSide.apply_image_torch` (antialiased bilinear), the mask
    is cut at 0.5, then `preprocess` normalises the image with the transform's mean / std and zero-pads both to S x S;
  * `get_support` (:268-317).

The files are decoded by Pillow on the host: `convert("RGB")` stands in for `cv2.imread` + BGR -> RGB and `convert("L")` then
`> 0` for `cv2.imread(path, 0)` then `img[img > 0] = 1`. PNG images and grey PNG masks decode to the same bytes in both libraries;
a JPEG decoder, and cv2's grey conversion of a colour mask, may differ from Pillow's by a rounding step. cv2 and torchvision are
not dependencies. Everything per pixel after the decode runs in `psam_image_intake` (mode 0): the uint8 bytes of a batch are
uploaded once, one launch makes the images and one the thresholded masks; no float image exists on the host.
"""
import os
import random

import numpy as np
import torch

from . import ops
from .segment_anything.utils.transforms import ResizeLongestSide

KVASIR, CLINIC_DB, COLON_DB, ETIS_DB, CVC300 = "Kvasir", "CVC-ClinicDB", "CVC-ColonDB", "ETIS-LaribPolypDB", "CVC-300"
DATASETS = (KVASIR, CLINIC_DB, COLON_DB, ETIS_DB)
EXCLUDE_DS = (CVC300,)


def _listed(root, exts):
    return [os.path.join(root, f) for f in os.listdir(root) if f.endswith(exts)]


def list_pairs(image_root, gt_root, exclude=EXCLUDE_DS):
    """-> [(image path, mask path)] by the reference's rules (see the module docstring)."""
    from PIL import Image
    images, gts = _listed(image_root, (".jpg", ".png")), _listed(gt_root, (".png",))
    for sub in os.listdir(image_root):
        if not os.path.isdir(os.path.join(image_root, sub)):
            continue
        images += _listed(os.path.join(image_root, sub), (".jpg", ".png"))
        gts += _listed(os.path.join(gt_root, sub), (".png",))
    images, gts = sorted(images), sorted(gts)
    if len(images) != len(gts):
        raise ValueError(f"{len(images)} images under {image_root} but {len(gts)} masks under {gt_root}")
    pairs = []
    for ip, gp in zip(images, gts):
        if any(ex in ip for ex in exclude):
            continue
        with Image.open(ip) as im, Image.open(gp) as gt:
            if im.size == gt.size:
                pairs.append((ip, gp))
    return pairs


def decode_pair(image_path, gt_path):
    """-> (uint8 [H, W, 3] RGB, uint8 [H, W] in {0, 1})"""
    from PIL import Image
    with Image.open(image_path) as im:
        img = np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))
    with Image.open(gt_path) as gt:
        mask = (np.asarray(gt.convert("L")) > 0).astype(np.uint8)
    if img.shape[:2] != mask.shape:
        raise ValueError(f"{image_path} is {img.shape[:2]} but {gt_path} is {mask.shape}")
    return img, mask


def intake_pairs(decoded, S, device, mean, std):
    """[(uint8 image [H, W, 3], uint8 mask [H, W])] as decoded -> images fp32 [B, 3, S, S], labels fp32 {0, 1} [B, S, S] on the device:
    two uploads of packed bytes, two launches of psam_image_intake (mode 0; the masks thresholded at 0.5)."""
    rows_i, rows_m, oi, om = [], [], 0, 0
    for img, mask in decoded:
        h, w = mask.shape
        if not ops.intake_supported(h, w, S):
            raise ValueError(f"an image of {h} x {w} is outside the intake kernel's range at S = {S} "
                             f"(sides 1..{ops.INTAKE_MAX_SIDE}, at most {ops.INTAKE_MAX_SCALE} source pixels per resized pixel)")
        oh, ow = ops.intake_shape(h, w, S)
        rows_i.append((oi, h, w, oh, ow))
        rows_m.append((om, h, w, oh, ow))
        oi += h * w * 3
        om += h * w
    ibuf = torch.from_numpy(np.concatenate([img.reshape(-1) for img, _ in decoded])).to(device)
    mbuf = torch.from_numpy(np.concatenate([mask.reshape(-1) for _, mask in decoded])).to(device)
    images = ops.image_intake_packed(ibuf, rows_i, 3, S, 0, mean, std)
    labels = ops.image_intake_packed(mbuf, rows_m, 1, S, 0, None, None, threshold=True)
    return images, labels[:, 0]


class ImageSet:
    """The image / mask pairs of a directory pair, loaded in batches onto `device` at model size S."""

    def __init__(self, image_root, gt_root, device, S=1024, transform=None, datasets=DATASETS, exclude=EXCLUDE_DS):
        self.device, self.S, self.datasets = device, int(S), tuple(datasets)
        self.transform = transform if transform is not None else ResizeLongestSide(self.S)
        assert self.transform.target_length == self.S
        self.mean = [float(v) for v in self.transform.pixel_mean.reshape(-1)]
        self.std = [float(v) for v in self.transform.pixel_std.reshape(-1)]
        self.pairs = list_pairs(image_root, gt_root, exclude)

    def __len__(self):
        return len(self.pairs)

    def case(self, index):
        """`get_dataset_name_from_path`: the first dataset name found in the image path, else ''"""
        for name in self.datasets:
            if name in self.pairs[index][0]:
                return name
        return ""

    def _intake(self, decoded):
        return intake_pairs(decoded, self.S, self.device, self.mean, self.std)

    def load(self, indices):
        """-> (images fp32 [B, 3, S, S], labels fp32 {0, 1} [B, S, S], [(H, W) of the files], [case]) on the device"""
        indices = [int(i) for i in indices]
        decoded = [decode_pair(*self.pairs[i]) for i in indices]
        images, labels = self._intake(decoded)
        return images, labels, [tuple(m.shape) for _, m in decoded], [self.case(i) for i in indices]

    def get_support(self, n_support=1, text_file=None, indices=None):
        """`PolypDataset.get_support`: the first n_support (image path, mask path) rows of `text_file`, or the pairs `indices` of
        this set, or (as the reference) n_support pairs drawn with `random.choices`. -> ([image [1, 3, S, S]], [mask [1, S, S]],
        case): the case is '' as the reference's `process_image_gt(image, mask)` leaves it."""
        if text_file is not None:
            with open(text_file) as f:
                paths = [tuple(line.strip().split()) for line in f if line.strip()]
            if n_support > len(paths):
                raise ValueError(f"n_support ({n_support}) is larger than the number of images in the text file ({len(paths)})")
            paths = paths[:n_support]
        else:
            if indices is None:
                indices = random.choices(range(len(self.pairs)), k=n_support)
            paths = [self.pairs[int(i)] for i in list(indices)[:n_support]]
        images, labels = self._intake([decode_pair(ip, gp) for ip, gp in paths])
        return [images[k:k + 1] for k in range(len(paths))], [labels[k:k + 1] for k in range(len(paths))], ""
