"""`SamWrapper` (models/SamWrapper.py:8-54): SAM's automatic mask generator as an oracle-guided coarse model - of all the
masks SAM proposes for an image, return the one with the best IoU against a given binary label.

Same constructor (`sam_args = {"model_type", "sam_checkpoint"}`) and `forward(image uint8 HWC, image_labels) -> bool
[H, W]` as the reference. The registry of the vendored package builds `SamBatched` (build_sam.py:66), whose
`postprocess_masks` interpolates with align_corners=True (modeling/sam.py:313-320), so that variant is selected here.

The reference downloads every proposed mask and scores it in numpy (:41-48). Here the masks are binarised on the device
together with their {tp, fp, fn} counts against the label; one mask crosses PCIe.

`sam_checkpoint = "random:<seed>[:<encoder_depth>]"` builds seeded synthetic weights (no checkpoints exist offline).
"""
import numpy as np
import torch
import torch.nn as nn

from .segment_anything import SamAutomaticMaskGenerator, sam_model_registry
from .segment_anything.utils.transforms import ResizeLongestSide


def get_iou(mask, label):
    """models/SamWrapper.py:8-13 (host version, for callers that hold numpy masks)."""
    tp = (mask * label).sum()
    fp = (mask * (1 - label)).sum()
    fn = ((1 - mask) * label).sum()
    return tp / (tp + fp + fn)


class SamWrapper(nn.Module):
    def __init__(self, sam_args):
        super().__init__()
        ckpt = sam_args["sam_checkpoint"]
        if isinstance(ckpt, str) and ckpt.startswith("random:"):
            from .synth import synth_state_dict
            parts = ckpt.split(":")
            depth = int(parts[2]) if len(parts) > 2 else None
            self.sam = sam_model_registry[sam_args["model_type"]](encoder_depth=depth)
            self.sam.load_state_dict(synth_state_dict(self.sam, int(parts[1])))
        else:
            self.sam = sam_model_registry[sam_args["model_type"]](checkpoint=ckpt)
        self.sam.postprocess_variant = "batched"
        self.sam.requires_grad_(False)
        self.mask_generator = SamAutomaticMaskGenerator(self.sam, **sam_args.get("generator_args", {}))
        self.transform = ResizeLongestSide(self.sam.image_encoder.img_size)
        self.last_stats = {}

    @torch.no_grad()
    def forward(self, image, image_labels, return_device=False):
        """image: HWC uint8; image_labels: binary [H, W] (numpy or tensor). -> bool numpy [H, W]: the proposal with the
        largest IoU against the label (the first one on ties, :44-46). `return_device=True` keeps it on the device as
        uint8 (used by `SamWrapperWrapper`)."""
        image = self.transform.apply_image(image)                               # :37
        dev = self.sam.device
        lab = self._check_label(image, image_labels).to(device=dev, dtype=torch.uint8).contiguous()
        cand, masks, counts = self.mask_generator.generate_device(image, lab)   # :38
        return self._best_mask(cand, masks, counts, return_device)

    def _best_mask(self, cand, masks, counts, return_device):
        """:40-48 over the proposals of `generate_device`: the mask with the largest IoU against the label; sets `last_stats`."""
        if masks.shape[0] == 0:
            raise TypeError("list indices must be integers or slices, not NoneType")   # masks[None], :48
        c = counts.cpu().numpy().astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = c[:, 0] / (c[:, 0] + c[:, 1] + c[:, 2])
        best, best_iou = None, 0                                                # :40-46
        for i, v in enumerate(iou):
            if best is None or v > best_iou:
                best, best_iou = i, v
        self.last_stats = dict(n_masks=int(masks.shape[0]), best_index=best, best_iou=float(best_iou), ious=iou,
                               candidates=cand)
        if return_device:
            return masks[best]
        return masks[best].cpu().numpy().astype(bool)

    @staticmethod
    def _check_label(image, image_labels):
        """`forward`'s label checks -> the label as a tensor (on whatever device it came)."""
        lab = torch.as_tensor(np.asarray(image_labels) if not torch.is_tensor(image_labels) else image_labels)
        if lab.numel() and (int(lab.min()) < 0 or int(lab.max()) > 1):
            raise ValueError("image_labels must be binary {0, 1} (models/ProtoSAM.py:124-125)")
        if tuple(lab.shape) != tuple(image.shape[:2]):
            raise ValueError(f"operands could not be broadcast together with shapes {tuple(image.shape[:2])} "
                             f"{tuple(lab.shape)}")                            # numpy's error in get_iou, :8-10
        return lab

    @torch.no_grad()
    def forward_batch(self, images, labels, return_device=False):
        """`forward` for B images of one size in one call: -> bool numpy [B, H, W] (uint8 on the device with `return_device`),
        equal to `forward(images[b], labels[b])` mask for mask. Labels are validated up front with `forward`'s messages. Per image
        one chain is enqueued with nothing read back - encode, decode, statistics, `psam_amg_select` (filters + box NMS),
        `psam_mask_counts` ({tp, fp, fn} of the survivors), `psam_best_iou`, and the binarisation of the one winning plane - and
        the decoder's output buffer is reused in stream order. The host waits once, after the last image; an image without a
        surviving proposal then raises `forward`'s TypeError. `last_stats` becomes a list with one `forward`-style dict per image.
        A generator that is off the fused path (crop layers, small-region removal) goes through `generate_device_batch`: the crops'
        device route per image, the host's wait for image i behind the crops of image i + 1, then `forward`'s choice."""
        from . import ops
        raw = list(images)
        images = [self.transform.apply_image(im) for im in raw]                 # :37
        labels = list(labels)
        if len(labels) != len(images):
            raise ValueError(f"{len(images)} images but {len(labels)} labels")
        if len(images) == 0:
            raise ValueError("forward_batch needs at least one image")
        dev = self.sam.device
        labs = [self._check_label(im, lb) for im, lb in zip(images, labels)]
        if any(im.shape[:2] != images[0].shape[:2] for im in images):
            raise ValueError("forward_batch: all images of a batch must have the same size")
        g = self.mask_generator
        if not all(g._fast_path(im) for im in images):
            # crop layers, small-region removal: `generate_device_batch` (the crops' device route, the host one image behind the
            # device), then `forward`'s choice per image
            labs_d = [lb.to(device=dev, dtype=torch.uint8).contiguous() for lb in labs]
            outs, stats = [], []
            for cand, masks, counts in g.generate_device_batch(images, labs_d):
                outs.append(self._best_mask(cand, masks, counts, return_device))
                stats.append(self.last_stats)
            self.last_stats = stats
            return torch.stack(outs) if return_device else np.stack(outs)
        B = len(images)
        h, w = images[0].shape[:2]
        sam = self.sam
        labs = [lb.to(device=dev, dtype=torch.uint8).contiguous() for lb in labs]
        masks = torch.empty((B, h, w), dtype=torch.uint8, device=dev)
        best = torch.empty((B, 4), dtype=torch.int32, device=dev)
        best_iou = torch.empty((B,), dtype=torch.float64, device=dev)
        tables, counts, ctxs = None, None, []
        for b, im in enumerate(images):
            ctx = g._enqueue(im)
            if tables is None:
                cap = 3 * ctx["n"]
                tables = torch.empty((B, cap * ops.AMG_REC + 1), dtype=torch.int32, device=dev)
                counts = torch.empty((B, cap, 3), dtype=torch.int64, device=dev)
            _, records, count = g._select_enqueue(ctx, out=tables[b])
            ops.mask_counts(ctx["low"], records, count, sam.image_encoder.img_size, h, w, sam.variant_id(), labs[b],
                            float(sam.mask_threshold), counts=counts[b])
            ops.best_iou(counts[b], records, count, best=best[b], iou=best_iou[b:b + 1])
            ops.mask_binarize(ctx["low"], best[b, :1], sam.image_encoder.img_size, h, w, sam.variant_id(),
                              float(sam.mask_threshold), out=masks[b:b + 1])
            ctxs.append(dict(pts=ctx["pts"], size=ctx["size"], n=ctx["n"]))
        best_h = best.cpu().numpy()                                             # the batch's one wait
        iou_h, tab_h, cnt_h = best_iou.cpu().numpy(), tables.cpu().numpy(), counts.cpu().numpy()
        stats = []
        for b in range(B):
            if best_h[b, 2]:
                raise TypeError("list indices must be integers or slices, not NoneType")   # masks[None], :48
            k = int(best_h[b, 3])
            c = cnt_h[b, :k].astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                ious = c[:, 0] / (c[:, 0] + c[:, 1] + c[:, 2])
            cand = g._cand_from_records(ctxs[b], tab_h[b], tables[b, :cap * ops.AMG_REC].view(cap, ops.AMG_REC))
            stats.append(dict(n_masks=k, best_index=int(best_h[b, 1]), best_iou=float(iou_h[b]), ious=ious, candidates=cand))
        self.last_stats = stats
        if return_device:
            return masks
        return masks.cpu().numpy().astype(bool)

    def to(self, device):
        self.sam.to(device)
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)
