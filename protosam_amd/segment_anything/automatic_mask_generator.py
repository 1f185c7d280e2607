"""`SamAutomaticMaskGenerator` (models/segment_anything/automatic_mask_generator.py:35-373) on the HIP path.

Same constructor arguments, record keys and filtering rules as the reference's generator; what differs is where the work
happens:
  * all grid points of a crop go through the two-way decoder in chunks of `decode_chunk` prompts (the reference: 64 per
    call, :255-259); the decoder is per-prompt independent, so chunking does not change results;
  * the reference up-samples every candidate to full resolution ([64*3, H, W] fp32) to take three counts and a box from
    it (:293-310). `psam_mask_stats` computes them straight from the 256x256 logits; nothing full-size is written;
  * box NMS (:262-268) runs on the host over the few hundred survivors of the score filters;
  * only the survivors of NMS are binarised (`psam_mask_binarize`), and they stay on the device until a caller asks
    for numpy (`generate`) - `SamWrapper` scores them against the label on the device and downloads one mask.
The intermediate uncompressed RLE (:312-313) only exists when `output_mode` asks for it, and then it is made on the device
(`mask_to_rle_pytorch` over `psam_rle_count` / `psam_rle_write`): the surviving masks are encoded in one call and only their
run lengths cross to the host - no full-size mask is downloaded.

`custom_points` keeps the reference's default, the *string* "false" (:52), and the reference's truthiness test (:280):
with the default, the second half of every `points_per_batch` batch is labelled as NEGATIVE points. `custom_points=False`
gives upstream SAM's behaviour.

An image whose long side is not the model's input size takes the same fused path, through every entry point (`generate`,
`generate_device`, `generate_batch`, `generate_device_batch`): its masks take the SECOND resize of `postprocess_masks`
(sam.py:132-160), which `psam_mask_stats_resized` / `psam_mask_binarize_resized` (csrc/amg_resize.hip) compute per output
pixel together with the first one - the bits of `psam_mask_upsample` -> crop -> `psam_resize2d`, nothing written in between.
The statistics kernel is given the predicted IoUs and skips the candidates that the first filter drops whatever their statistics
(`psam_mask_stats_resized_scored`): their rows hold the empty-mask values and are never read.
Images at the model's size run `psam_mask_stats` / `psam_mask_binarize` as before (`_fast_path`).

Crop layers (`crop_n_layers > 0`, :194-262) and `min_mask_region_area > 0` (:332-380) take the general path
(`_generate_general`): every crop is re-encoded; one statistics table for all 3n candidates of the crop comes straight from
its logits (`_crop_fused`), one download, then predicted-IoU, stability and edge filter and the per-crop NMS on the host in
the reference's order, and only the NMS survivors are binarised - into zeroed frames of the original image at the crop's
offset (uncrop_masks); cross-crop NMS on the host; holes / islands below the area threshold are found with the device
connected-components kernel (`psam_ccl`; the reference loops over masks with cv2, utils/amg.py:267-291), one mask at a time.

The small-region stage itself runs on the device for all masks at once (`PSAM_AMG_REGIONS=device`, read in the constructor, the
default): `ops.small_regions_select` (csrc/small_regions.hip: holes and islands of every mask in one kernel chain, areas counted per
union-find root, so no limit on the number of regions; new areas and boxes from the same passes; `psam_box_nms` behind it) and one
download of the decision; the masks are then one gather. `PSAM_AMG_REGIONS=host` keeps the per-mask loop described above. Both
return the same records; profiles/amg_small_regions_bench.txt has the timings behind the default.
With `PSAM_AMG_SELECT=device` a crop's candidates are selected on the device too (`psam_amg_select_crop`: `psam_amg_select` with
the crop-edge filter of :309-311): one copy of the records instead of the statistics table, and the binarisation reads its planes
from the record table. With the default, `host`, a crop is selected on the host as before.

`PSAM_AMG_CROPS=device` (read in the constructor; default `host` for the single-image entry points, and what the batch entry points
always do) takes the host out of the crop loop (csrc/amg_crops.hip): per crop encode, decode, statistics, `psam_amg_select_crop`
and `psam_amg_keep_planes` - the crop's kept records join the image's merged table, translated to the image's frame, and their
logit planes a plane pool, because the next crop overwrites the decoder's output - with nothing read back; behind the last crop
`psam_amg_crops_nms` (cross-crop NMS on the device, `psam_box_nms` with the float32 1 / crop area scores of :208-213), ONE copy of
the final records and one wait; then `psam_mask_binarize_crops` for the final records only, each with its own crop's geometry, and
the small-region stage as before. Device memory is the pool (`crop_pool_cap` planes of 256 KiB, default 256 per crop) instead of
(survivors of all crops) x H x W bytes; a pool overflow is reported in the final table and sends the image down the host route.
The records are the host route's, record for record.

`PSAM_AMG_RESIZE=materialise` (read in the constructor, default `fused`) selects the earlier route for any-size images and
crops: the candidates that pass the predicted-IoU filter are written at full size in chunks of 64 (`postprocess_masks`) and
reduced by `psam_plane_stats` (counts, box, binary mask in one pass). Both routes return the same records; the tests and
tools/bench_amg_anysize.py compare them.
output_mode "coco_rle" keeps the reference's contract: the constructor imports pycocotools and raises the same ImportError
without it (:116-117); with it, the segmentation is `coco_encode_rle` of the uncompressed RLE (:181-183), which is this
project's own restatement of the COCO string form. Without the package, `coco_encode_rle(rec["segmentation"])` on the
records of output_mode "uncompressed_rle" gives the same COCO record.
"""
import os

import numpy as np
import torch

from .. import ops
from .predictor import SamPredictor
from .utils.amg import (area_from_rle, box_xyxy_to_xywh, build_all_layer_point_grids, coco_encode_rle, generate_crop_boxes,
                        is_box_near_crop_edge, mask_to_rle_pytorch, nms_xyxy)


class SamAutomaticMaskGenerator:
    def __init__(self, model, points_per_side=32, points_per_batch=64, pred_iou_thresh=0.88,
                 stability_score_thresh=0.95, stability_score_offset=1.0, box_nms_thresh=0.7, crop_n_layers=0,
                 crop_nms_thresh=0.7, crop_overlap_ratio=512 / 1500, crop_n_points_downscale_factor=1,
                 point_grids=None, min_mask_region_area=0, output_mode="binary_mask", custom_points="false",
                 decode_chunk=256, crop_pool_cap=None):
        assert (points_per_side is None) != (point_grids is None), \
            "Exactly one of points_per_side or point_grid must be provided."
        if points_per_side is not None:
            self.point_grids = build_all_layer_point_grids(points_per_side, crop_n_layers,
                                                           crop_n_points_downscale_factor)
        else:
            self.point_grids = point_grids
        assert output_mode in ["binary_mask", "uncompressed_rle", "coco_rle"], f"Unknown output_mode {output_mode}."
        if output_mode == "coco_rle":
            from pycocotools import mask as mask_utils  # noqa: F401  (same ImportError as the reference, :116-117)
        self.predictor = SamPredictor(model)
        self.points_per_batch = points_per_batch
        self.pred_iou_thresh = pred_iou_thresh
        self.stability_score_thresh = stability_score_thresh
        self.stability_score_offset = stability_score_offset
        self.box_nms_thresh = box_nms_thresh
        self.crop_n_layers = crop_n_layers
        self.crop_nms_thresh = crop_nms_thresh
        self.crop_overlap_ratio = crop_overlap_ratio
        self.crop_n_points_downscale_factor = crop_n_points_downscale_factor
        self.min_mask_region_area = min_mask_region_area
        self.output_mode = output_mode
        self.custom_points = custom_points
        self.decode_chunk = decode_chunk
        # where the fused path filters and suppresses its candidates: "host" (numpy + nms_xyxy between two device stages, the
        # default) or "device" (psam_amg_select); the batch entry points always select on the device
        self.amg_select = os.environ.get("PSAM_AMG_SELECT", "host")
        if self.amg_select not in ("host", "device"):
            raise ValueError(f"PSAM_AMG_SELECT must be 'host' or 'device', got {self.amg_select!r}")
        # how images that are not at the model's input size, and crops, get their statistics and masks: "fused" (the default:
        # psam_mask_stats_resized / psam_mask_binarize_resized, both resizes of postprocess_masks per pixel, nothing written in
        # between) or "materialise" (postprocess_masks writes every filtered candidate at full size, psam_plane_stats reduces it)
        self.amg_resize = os.environ.get("PSAM_AMG_RESIZE", "fused")
        if self.amg_resize not in ("fused", "materialise"):
            raise ValueError(f"PSAM_AMG_RESIZE must be 'fused' or 'materialise', got {self.amg_resize!r}")
        # the small-region stage (min_mask_region_area > 0): "host" (a Python loop over the masks, two psam_ccl calls and two
        # downloads per mask, then statistics and nms_xyxy on the host) or "device" (the default: ops.small_regions_select, one
        # kernel chain for all masks, box NMS on the device, one download). Both give the same records.
        self.amg_regions = os.environ.get("PSAM_AMG_REGIONS", "device")
        if self.amg_regions not in ("host", "device"):
            raise ValueError(f"PSAM_AMG_REGIONS must be 'host' or 'device', got {self.amg_regions!r}")
        # the general path's crops (crop_n_layers > 0, or the one crop of min_mask_region_area > 0): "host" (the default of the
        # single-image entry points: the host waits for every crop, binarises every per-crop survivor into a full frame and runs
        # the cross-crop NMS) or "device" (`_crops_enqueue` / `_crops_finish`: no wait per crop, cross-crop NMS on the device, one
        # copy per image, only the final records binarised); the batch entry points always take the device route
        self.amg_crops = os.environ.get("PSAM_AMG_CROPS", "host")
        if self.amg_crops not in ("host", "device"):
            raise ValueError(f"PSAM_AMG_CROPS must be 'host' or 'device', got {self.amg_crops!r}")
        if crop_pool_cap is not None and not 1 <= int(crop_pool_cap) <= ops.NMS_MAX_GROUP:
            raise ValueError(f"crop_pool_cap must be in 1 .. {ops.NMS_MAX_GROUP}, got {crop_pool_cap}")
        self.crop_pool_cap = None if crop_pool_cap is None else int(crop_pool_cap)
        self._low = None

    def to(self, device):  # models/SamWrapper.py:52-54 calls this
        self.predictor.model.to(device)
        return self

    # ---- candidates ------------------------------------------------------------------------------------------------
    def _point_labels(self, n):
        """:277-283. Labels by position inside each `points_per_batch` batch."""
        out = np.ones(n, np.int32)
        if not self.custom_points:
            return out
        for lo in range(0, n, self.points_per_batch):
            m = min(self.points_per_batch, n - lo)
            if m % 2:
                raise ValueError(f"custom_points needs an even number of points per batch, got {m}")
            out[lo + m // 2: lo + m] = 0
        return out

    def _buffers(self, n, dev, slot=0):
        """The decoder's outputs for n prompts: (low [n,4,256,256], iou [n,4]) fp32 on the device. Slot 0 is `self._low` /
        `self._iou`, what the single-image entry points use; slot 1 is the second pair `generate_batch` alternates with."""
        names = ("_low", "_iou") if slot == 0 else ("_low_b", "_iou_b")
        low = getattr(self, names[0], None)
        if low is None or low.shape[0] != n or low.device != dev:
            setattr(self, names[0], torch.empty((n, 4, 256, 256), dtype=torch.float32, device=dev))
            setattr(self, names[1], torch.empty((n, 4), dtype=torch.float32, device=dev))
        return getattr(self, names[0]), getattr(self, names[1])

    @torch.no_grad()
    def _enqueue(self, image, slot=0):
        """Layer-0 crop (the whole image): encode, decode every grid point, reduce. Everything is enqueued, nothing is read back.
        -> dict(pts, size, n, low, iou, stats): the grid points (host), the decoder's outputs and the int32 [3n, 8] statistics
        table (device)."""
        pr = self.predictor
        sam = pr.model
        h, w = image.shape[:2]
        pr.set_image(image)                                                     # :239
        in_size = tuple(int(v) for v in pr.input_size)
        assert in_size == self._input_size(h, w)
        pts = self.point_grids[0] * np.array([[w, h]], dtype=np.float64)        # :241-243
        n = len(pts)
        labels = self._point_labels(n)
        dev = pr.device
        S = sam.image_encoder.img_size
        coords = np.zeros((n, 2, 2), np.float32)                                # point + the "not a point" pad token
        coords[:, 0] = pr.transform.apply_coords(pts, (h, w))                   # :274
        lab2 = np.stack([labels, np.full(n, -1, np.int32)], 1)
        pe = sam.prompt_encoder._packed()
        dpk = sam.mask_decoder._packed()
        coords_d = torch.from_numpy(coords).to(dev)
        lab_d = torch.from_numpy(np.ascontiguousarray(lab2)).to(dev)
        low, iou = self._buffers(n, dev, slot)
        feat_tok = pr.features_tokens[0]
        for lo in range(0, n, self.decode_chunk):                               # :255-259 / predictor.py:216-235
            hi = min(lo + self.decode_chunk, n)
            tokens = ops.prompt_tokens(coords_d[lo:hi], lab_d[lo:hi], pe["G"], pe["type_emb"], dpk["out_tok"], hi - lo, 2,
                                       float(S))
            sam.mask_decoder.predict_masks_tokens(feat_tok, pe["pe_tok"], tokens, pe["no_mask"],
                                                  masks_out=low[lo:hi], iou_out=iou[lo:hi])
        pr.reset_image()                                                        # :260
        thr = float(sam.mask_threshold)
        if in_size == (h, w):
            stats = ops.mask_stats(low, 1, 3, S, h, w, sam.variant_id(), thr, self.stability_score_offset)
        else:   # the second resize of postprocess_masks, on the fly; candidates the predicted-IoU filter drops anyway are skipped
            stats = ops.mask_stats_resized(low, 1, 3, S, in_size, (h, w), sam.variant_id(), thr, self.stability_score_offset,
                                           score=iou, score_thresh=self.pred_iou_thresh)
        return dict(pts=pts, size=(h, w), n=n, low=low, iou=iou, stats=stats)

    def _select_host(self, ctx):
        """The score filters and box NMS on the host: two downloads, numpy, one upload (the default, PSAM_AMG_SELECT=host)."""
        pts, n, dev = ctx["pts"], ctx["n"], ctx["low"].device
        stats = ctx["stats"].cpu().numpy()
        iou = ctx["iou"][:, 1:].reshape(-1).cpu().numpy()                       # multimask_output=True, flatten(0, 1)
        keep = np.arange(3 * n)
        if self.pred_iou_thresh > 0.0:                                          # :293-295
            keep = keep[iou[keep] > self.pred_iou_thresh]
        with np.errstate(divide="ignore", invalid="ignore"):                    # utils/amg.py:156-176 (int32 / int32)
            stab = stats[:, 0].astype(np.float32) / stats[:, 1].astype(np.float32)
        if self.stability_score_thresh > 0.0:                                   # :301-303
            keep = keep[stab[keep] >= self.stability_score_thresh]
        boxes = stats[:, 3:7].astype(np.int64)
        boxes[stats[:, 2] == 0] = 0                                             # empty mask -> [0,0,0,0] (amg.py:339-341)
        # is_box_near_crop_edge (:309-311) is vacuous for the layer-0 crop: the crop box IS the image box
        kept = keep[nms_xyxy(boxes[keep], iou[keep], self.box_nms_thresh)]      # :262-268
        plane = (kept // 3) * 4 + 1 + kept % 3                                  # index into low.view(-1,256,256)
        return dict(iou_preds=iou[kept], stability_score=stab[kept], boxes=boxes[kept], area=stats[kept, 2],
                    points=pts[kept // 3], plane=torch.from_numpy(plane.astype(np.int32)).to(dev), size=ctx["size"])

    def _select_enqueue(self, ctx, out=None):
        """The same selection on the device (`psam_amg_select`), enqueued behind the statistics: -> (out, records int32 [3n,9],
        count int32 [1]): `out` (given, or a new one) is the int32 device tensor of 3n * 9 + 1 words that holds the records and
        then the count, so one copy of it brings the whole selection to the host."""
        cap = 3 * ctx["n"]
        if out is None:
            out = torch.empty((cap * ops.AMG_REC + 1,), dtype=torch.int32, device=ctx["low"].device)
        records, count = ops.amg_select(ctx["stats"], ctx["iou"], (0, cap), self.pred_iou_thresh, self.stability_score_thresh,
                                        self.box_nms_thresh, cap=cap, out=out)
        return out, records[0], count

    @staticmethod
    def _cand_from_records(ctx, table, records_dev):
        """The candidate dict of `_select_host` from the record table alone: `table` = the host copy (numpy int32) of the tensor
        behind `records_dev` [3n, 9] (records, then the count)."""
        cap = 3 * ctx["n"]
        k = min(int(table[cap * ops.AMG_REC]), cap)
        r = table[:cap * ops.AMG_REC].reshape(cap, ops.AMG_REC)[:k].copy()     # (the caller may reuse `table`)
        kept = r[:, 0].astype(np.int64)
        # the plane column as a dense tensor (a new one: `.contiguous()` hands a one-row view back with its stride of 9)
        plane = torch.empty((k,), dtype=torch.int32, device=records_dev.device).copy_(records_dev[:k, 1])
        return dict(iou_preds=np.ascontiguousarray(r[:, 2]).view(np.float32), stability_score=np.ascontiguousarray(r[:, 3]).view(np.float32),
                    boxes=r[:, 5:9].astype(np.int64), area=np.ascontiguousarray(r[:, 4]), points=ctx["pts"][kept // 3],
                    plane=plane, size=ctx["size"])

    @torch.no_grad()
    def _candidates(self, image):
        """Layer-0 crop (the whole image): encode, decode every grid point, reduce, filter, NMS.
        -> dict of numpy arrays over the kept candidates (NMS order) + `plane` (int32 device indices into self._low)."""
        ctx = self._enqueue(image)
        if self.amg_select == "host":
            return self._select_host(ctx)
        out, records, _ = self._select_enqueue(ctx)
        return self._cand_from_records(ctx, out.cpu().numpy(), records)                 # the one copy

    def _binarize(self, cand, label=None, low=None):
        """uint8 device masks [n, H, W] of the kept candidates (+ {tp, fp, fn} vs `label` uint8 [H, W] on the device)."""
        sam = self.predictor.model
        low = self._low if low is None else low
        h, w = cand["size"]
        if cand["plane"].numel() == 0:
            return torch.empty((0, h, w), dtype=torch.uint8, device=low.device), None
        S = sam.image_encoder.img_size
        in_size = self._input_size(h, w)
        if in_size == (h, w):
            return ops.mask_binarize(low, cand["plane"], S, h, w, sam.variant_id(), float(sam.mask_threshold), label=label)
        return ops.mask_binarize_resized(low, cand["plane"], S, in_size, (h, w), sam.variant_id(), float(sam.mask_threshold),
                                         label=label)

    def _input_size(self, h, w):
        """`predictor.input_size` of an h x w image: its size once the long side is the model's (ResizeLongestSide)."""
        S = self.predictor.model.image_encoder.img_size
        return tuple(int(v) for v in self.predictor.transform.get_preprocess_shape(h, w, S))

    # ---- general path: crop layers, small-region removal, PSAM_AMG_RESIZE=materialise -----------------------------------------
    def _fast_path(self, image):
        """Layer-0 crop only, image already at the model's input size (what SamWrapper.forward produces): the fused path without a
        second resize, which is what `SamWrapper.forward_batch` chains its own kernels behind."""
        h, w = image.shape[:2]
        S = self.predictor.model.image_encoder.img_size
        return self.crop_n_layers == 0 and self.min_mask_region_area == 0 and max(h, w) == S

    def _fused_path(self, image):
        """Layer-0 crop only, no small-region stage: the fused path, at any image size unless PSAM_AMG_RESIZE=materialise keeps
        images that need the second resize on the general path."""
        if self.amg_resize == "fused":
            return self.crop_n_layers == 0 and self.min_mask_region_area == 0
        return self._fast_path(image)

    def _decode_points(self, pts, im_size):
        """All grid points of the image set on the predictor -> self._low [n,4,256,256], self._iou [n,4] (device)."""
        pr = self.predictor
        sam = pr.model
        n = len(pts)
        dev = pr.device
        S = sam.image_encoder.img_size
        labels = self._point_labels(n)
        coords = np.zeros((n, 2, 2), np.float32)
        coords[:, 0] = pr.transform.apply_coords(pts, im_size)
        lab2 = np.stack([labels, np.full(n, -1, np.int32)], 1)
        pe = sam.prompt_encoder._packed()
        dpk = sam.mask_decoder._packed()
        coords_d = torch.from_numpy(coords).to(dev)
        lab_d = torch.from_numpy(np.ascontiguousarray(lab2)).to(dev)
        if self._low is None or self._low.shape[0] != n or self._low.device != dev:
            self._low = torch.empty((n, 4, 256, 256), dtype=torch.float32, device=dev)
            self._iou = torch.empty((n, 4), dtype=torch.float32, device=dev)
        feat_tok = pr.features_tokens[0]
        for lo in range(0, n, self.decode_chunk):
            hi = min(lo + self.decode_chunk, n)
            tokens = ops.prompt_tokens(coords_d[lo:hi], lab_d[lo:hi], pe["G"], pe["type_emb"], dpk["out_tok"], hi - lo, 2,
                                       float(S))
            sam.mask_decoder.predict_masks_tokens(feat_tok, pe["pe_tok"], tokens, pe["no_mask"],
                                                  masks_out=self._low[lo:hi], iou_out=self._iou[lo:hi])

    def _process_crop(self, image, crop_box, layer_idx, orig_size, chunk=64):
        """:221-316 for one crop. -> dict of host arrays over the candidates kept after the per-crop NMS, in the ORIGINAL
        image's frame, + `masks` uint8 [k, H, W] on the device (uncropped)."""
        pr = self.predictor
        sam = pr.model
        H, W = orig_size
        x0, y0, x1, y1 = crop_box
        cropped = np.ascontiguousarray(image[y0:y1, x0:x1, :])
        ch, cw = cropped.shape[:2]
        pr.set_image(cropped)
        pts = self.point_grids[layer_idx] * np.array([[cw, ch]], dtype=np.float64)
        self._decode_points(pts, (ch, cw))
        in_size = tuple(pr.input_size)
        pr.reset_image()
        if self.amg_resize == "fused":
            return self._crop_fused(pts, crop_box, tuple(int(v) for v in in_size), orig_size)
        dev = self._low.device
        thr = float(sam.mask_threshold)
        n = len(pts)
        iou = self._iou[:, 1:].reshape(-1).cpu().numpy()
        cand = np.arange(3 * n)
        if self.pred_iou_thresh > 0.0:
            cand = cand[iou[cand] > self.pred_iou_thresh]
        planes = (cand // 3) * 4 + 1 + cand % 3
        low_flat = self._low.view(-1, 1, 256, 256)
        keep_l, stab_l, box_l, area_l, mask_l = [], [], [], [], []
        for lo in range(0, len(cand), chunk):                                   # bounded full-resolution working set
            sel = torch.from_numpy(planes[lo:lo + chunk].astype(np.int64)).to(dev)
            full = sam.postprocess_masks(low_flat[sel].contiguous(), in_size, (ch, cw))[:, 0].contiguous()   # [k, ch, cw] logits
            st, binm = ops.plane_stats(full, thr, self.stability_score_offset)
            st = st.cpu().numpy()
            with np.errstate(divide="ignore", invalid="ignore"):
                stab = st[:, 0].astype(np.float32) / st[:, 1].astype(np.float32)
            ok = np.ones(len(st), bool)
            if self.stability_score_thresh > 0.0:
                ok &= stab >= self.stability_score_thresh
            boxes = st[:, 3:7].astype(np.int64)
            boxes[st[:, 2] == 0] = 0
            ok &= ~is_box_near_crop_edge(boxes, crop_box, [0, 0, W, H])         # :309-311
            idx = np.flatnonzero(ok)
            keep_l.append(cand[lo:lo + chunk][idx]); stab_l.append(stab[idx]); box_l.append(boxes[idx]); area_l.append(st[idx, 2])
            mask_l.append(binm[torch.from_numpy(idx).to(dev)])
        kept = np.concatenate(keep_l) if keep_l else np.zeros(0, np.int64)
        stab = np.concatenate(stab_l) if stab_l else np.zeros(0, np.float32)
        boxes = np.concatenate(box_l) if box_l else np.zeros((0, 4), np.int64)
        area = np.concatenate(area_l) if area_l else np.zeros(0, np.int64)
        masks = torch.cat(mask_l) if mask_l else torch.empty((0, ch, cw), dtype=torch.uint8, device=dev)
        order = nms_xyxy(boxes, iou[kept], self.box_nms_thresh)                 # :244-250
        full_masks = torch.zeros((len(order), H, W), dtype=torch.uint8, device=dev)   # uncrop_masks
        if len(order):
            full_masks[:, y0:y1, x0:x1] = masks[torch.from_numpy(order).to(dev)]
        return dict(iou_preds=iou[kept][order], stability_score=stab[order], boxes=boxes[order] + np.array([[x0, y0, x0, y0]]),
                    area=area[order], points=pts[kept[order] // 3] + np.array([[x0, y0]], dtype=np.float64),
                    crop_boxes=np.tile(np.array([crop_box], dtype=np.int64), (len(order), 1)), masks=full_masks)

    def _crop_stats(self, in_size, crop_size):
        """The int32 [3n, 8] statistics table of the crop whose logits are in self._low, straight from them (device)."""
        sam = self.predictor.model
        S, variant, thr = sam.image_encoder.img_size, sam.variant_id(), float(sam.mask_threshold)
        if in_size == crop_size:
            return ops.mask_stats(self._low, 1, 3, S, crop_size[0], crop_size[1], variant, thr, self.stability_score_offset)
        return ops.mask_stats_resized(self._low, 1, 3, S, in_size, crop_size, variant, thr, self.stability_score_offset,
                                      score=self._iou, score_thresh=self.pred_iou_thresh)

    def _crop_fused(self, pts, crop_box, in_size, orig_size):
        """`_process_crop` after the decoder, without a full-resolution candidate: one statistics table for all 3n candidates
        straight from the logits, one download, the host filters and NMS in `_process_crop`'s order, and only the NMS survivors
        binarised - into zeroed frames of the ORIGINAL image at the crop's offset (uncrop_masks). The same dict."""
        sam = self.predictor.model
        H, W = orig_size
        x0, y0, x1, y1 = crop_box
        ch, cw = y1 - y0, x1 - x0
        dev = self._low.device
        S, variant, thr = sam.image_encoder.img_size, sam.variant_id(), float(sam.mask_threshold)
        n = len(pts)
        stats = self._crop_stats(in_size, (ch, cw))
        if self.amg_select == "device":
            return self._crop_select_device(stats, pts, crop_box, in_size, orig_size)
        host = torch.cat([stats.view(-1), self._iou.view(torch.int32).view(-1)]).cpu().numpy()   # the one download
        st = host[:3 * n * 8].reshape(3 * n, 8)
        iou = np.ascontiguousarray(host[3 * n * 8:].view(np.float32).reshape(n, 4)[:, 1:]).reshape(-1)
        cand = np.arange(3 * n)
        if self.pred_iou_thresh > 0.0:
            cand = cand[iou[cand] > self.pred_iou_thresh]
        st = st[cand]
        with np.errstate(divide="ignore", invalid="ignore"):
            stab = st[:, 0].astype(np.float32) / st[:, 1].astype(np.float32)
        ok = np.ones(len(st), bool)
        if self.stability_score_thresh > 0.0:
            ok &= stab >= self.stability_score_thresh
        boxes = st[:, 3:7].astype(np.int64)
        boxes[st[:, 2] == 0] = 0
        ok &= ~is_box_near_crop_edge(boxes, crop_box, [0, 0, W, H])             # :309-311
        idx = np.flatnonzero(ok)
        kept, stab, boxes, area = cand[idx], stab[idx], boxes[idx], st[idx, 2]
        order = nms_xyxy(boxes, iou[kept], self.box_nms_thresh)                 # :244-250
        full_masks = torch.zeros((len(order), H, W), dtype=torch.uint8, device=dev)   # uncrop_masks
        if len(order):
            planes = (kept[order] // 3) * 4 + 1 + kept[order] % 3
            ops.mask_binarize_resized(self._low, torch.from_numpy(planes.astype(np.int32)).to(dev), S, in_size, (ch, cw), variant,
                                      thr, out=full_masks, origin=(y0, x0))
        return dict(iou_preds=iou[kept][order], stability_score=stab[order], boxes=boxes[order] + np.array([[x0, y0, x0, y0]]),
                    area=area[order], points=pts[kept[order] // 3] + np.array([[x0, y0]], dtype=np.float64),
                    crop_boxes=np.tile(np.array([crop_box], dtype=np.int64), (len(order), 1)), masks=full_masks)

    def _crop_select_device(self, stats, pts, crop_box, in_size, orig_size):
        """`_crop_fused` behind the statistics with the selection on the device (PSAM_AMG_SELECT=device): the score filters, the
        crop-edge filter and the per-crop NMS are `psam_amg_select_crop`, one small copy brings the records and their count to the
        host, and the binarisation reads its planes from the record table. The same dict."""
        sam = self.predictor.model
        H, W = orig_size
        x0, y0, x1, y1 = crop_box
        ch, cw = y1 - y0, x1 - x0
        dev = self._low.device
        S, variant, thr = sam.image_encoder.img_size, sam.variant_id(), float(sam.mask_threshold)
        cap = 3 * len(pts)
        out = torch.empty((cap * ops.AMG_REC + 1,), dtype=torch.int32, device=dev)
        records, _ = ops.amg_select_crop(stats, self._iou, (0, cap), self.pred_iou_thresh, self.stability_score_thresh,
                                         self.box_nms_thresh, crop_box, [0, 0, W, H], cap=cap, out=out)
        cand = self._cand_from_records(dict(n=len(pts), pts=pts, size=(ch, cw)), out.cpu().numpy(), records[0])   # the one copy
        k = cand["plane"].numel()
        full_masks = torch.zeros((k, H, W), dtype=torch.uint8, device=dev)      # uncrop_masks
        if k:
            ops.mask_binarize_resized(self._low, cand["plane"], S, in_size, (ch, cw), variant, thr, out=full_masks, origin=(y0, x0))
        return dict(iou_preds=cand["iou_preds"], stability_score=cand["stability_score"],
                    boxes=cand["boxes"] + np.array([[x0, y0, x0, y0]]), area=cand["area"],
                    points=cand["points"] + np.array([[x0, y0]], dtype=np.float64),
                    crop_boxes=np.tile(np.array([crop_box], dtype=np.int64), (k, 1)), masks=full_masks)

    # ---- crops on the device (PSAM_AMG_CROPS=device, and always from the batch entry points) ----------------------------------
    CROP_POOL_PER_CROP = 256

    def _crops_device_ok(self):
        """whether the general path can take the device route whatever PSAM_AMG_CROPS says (the batch entry points ask this):
        PSAM_AMG_RESIZE=materialise and the per-mask host loop of PSAM_AMG_REGIONS=host keep today's route"""
        return self.amg_resize == "fused" and not (self.min_mask_region_area > 0 and self.amg_regions == "host")

    def _crop_pool_rows(self, caps):
        """Rows of the plane pool (and of the merged table) for an image whose crops have `caps` candidates each: the constructor's
        `crop_pool_cap`, or by default CROP_POOL_PER_CROP = 256 per crop (fewer where a crop has fewer candidates), shared by
        all crops of the image, at most ops.NMS_MAX_GROUP - the group limit of the cross-crop NMS. A row is one 256 x 256 fp32
        plane, 256 KiB: the default costs 64 MiB per crop - 320 MiB for the 5 crops of crop_n_layers=1, 1344 MiB for the 21 of
        crop_n_layers=2 - and the batch entry points hold two pools. An image whose per-crop survivors do not fit is reported
        by the device (`_crops_finish` returns None) and takes the host route."""
        if self.crop_pool_cap is not None:
            return self.crop_pool_cap
        return max(1, min(ops.NMS_MAX_GROUP, sum(min(c, self.CROP_POOL_PER_CROP) for c in caps)))

    def _crop_buffers(self, slot, pool_cap, ncrops, sel_words, dev):
        """The device buffers of buffer set `slot`: pool, merged table, counter, final table, per-crop record table."""
        sets = self.__dict__.setdefault("_crop_bufs", {})
        b = sets.get(slot)
        if b is None or b["key"][:3] != (pool_cap, ncrops, str(dev)) or b["key"][3] < sel_words:
            b = sets[slot] = None                                               # (release before the new pool is made)
            b = sets[slot] = dict(key=(pool_cap, ncrops, str(dev), sel_words),
                                  pool=torch.empty((pool_cap, 256, 256), dtype=torch.float32, device=dev),
                                  merged=torch.empty((pool_cap * ops.AMG_CREC,), dtype=torch.int32, device=dev),
                                  bases=torch.empty((ncrops + 1,), dtype=torch.int32, device=dev),
                                  out=torch.empty((pool_cap * ops.AMG_CREC + 2,), dtype=torch.int32, device=dev),
                                  sel=torch.empty((sel_words,), dtype=torch.int32, device=dev))
        return b

    @torch.no_grad()
    def _crops_enqueue(self, image, slot=0):
        """Every crop of the image, enqueued with nothing read back: encode and decode by `_process_crop`'s calls (the same logits),
        statistics, `psam_amg_select_crop`, `psam_amg_keep_planes` (the crop's records join the image's merged table, their planes
        the pool); behind the last crop the geometry table goes up and `psam_amg_crops_nms` leaves the final records and their count
        in ONE int32 device tensor, ctx["out"]. -> ctx for `_crops_finish`."""
        pr = self.predictor
        H, W = image.shape[:2]
        crop_boxes, layer_idxs = generate_crop_boxes((H, W), self.crop_n_layers, self.crop_overlap_ratio)
        ncrops = len(crop_boxes)
        grids = [self.point_grids[li] for li in layer_idxs]
        caps = [3 * len(g) for g in grids]
        pool_cap = self._crop_pool_rows(caps)
        dev = pr.device
        buf = self._crop_buffers(slot, pool_cap, ncrops, max(caps) * ops.AMG_REC + 1, dev)
        pts_all, in_sizes = [], []
        for c, (crop_box, grid) in enumerate(zip(crop_boxes, grids)):
            x0, y0, x1, y1 = crop_box
            cropped = np.ascontiguousarray(image[y0:y1, x0:x1, :])
            ch, cw = cropped.shape[:2]
            pr.set_image(cropped)
            pts = grid * np.array([[cw, ch]], dtype=np.float64)
            self._decode_points(pts, (ch, cw))
            in_size = tuple(int(v) for v in pr.input_size)
            pr.reset_image()
            stats = self._crop_stats(in_size, (ch, cw))
            cap = caps[c]
            records, count = ops.amg_select_crop(stats, self._iou, (0, cap), self.pred_iou_thresh, self.stability_score_thresh,
                                                 self.box_nms_thresh, crop_box, [0, 0, W, H], cap=cap, out=buf["sel"])
            ops.amg_keep_planes(self._low, records[0], count, c, ncrops, (x0, y0), buf["pool"], buf["merged"], buf["bases"])
            pts_all.append(pts)
            in_sizes.append(in_size)
        geom = torch.from_numpy(ops.amg_crop_geometry(crop_boxes, in_sizes)).to(dev)          # the one upload
        ops.amg_crops_nms(buf["merged"], buf["bases"], geom, ncrops, pool_cap, self.crop_nms_thresh, use_nms=ncrops > 1,   # :208
                          out=buf["out"])
        return dict(size=(H, W), crop_boxes=np.asarray(crop_boxes, dtype=np.int64), pts=pts_all, geom=geom, ncrops=ncrops,
                    pool_cap=pool_cap, pool=buf["pool"], out=buf["out"])

    @torch.no_grad()
    def _crops_finish(self, ctx, table):
        """`table`: the host copy (numpy int32) of ctx["out"]. -> (dict of host arrays, uint8 masks [m, H, W] on the device) over
        the records that the cross-crop NMS left, as `_generate_general` has them in front of its small-region stage - only these
        are binarised (`psam_mask_binarize_crops`, every record with its own crop's geometry). None where the pool overflowed."""
        sam = self.predictor.model
        H, W = ctx["size"]
        words = ctx["pool_cap"] * ops.AMG_CREC
        m = int(table[words])
        if m < 0:
            return None
        r = table[:m * ops.AMG_CREC].reshape(m, ops.AMG_CREC).copy()           # (the caller may reuse `table`)
        crop, cand = r[:, ops.AMG_REC].astype(np.int64), r[:, 0].astype(np.int64)
        cb = ctx["crop_boxes"]
        points = np.zeros((m, 2), np.float64)
        for c in np.unique(crop):
            sel = crop == c
            points[sel] = ctx["pts"][c][cand[sel] // 3] + np.array([[cb[c, 0], cb[c, 1]]], dtype=np.float64)
        data = dict(iou_preds=np.ascontiguousarray(r[:, 2]).view(np.float32), stability_score=np.ascontiguousarray(r[:, 3]).view(np.float32),
                    boxes=r[:, 5:9].astype(np.int64), area=np.ascontiguousarray(r[:, 4]), points=points, crop_boxes=cb[crop])
        dev = ctx["pool"].device
        if m == 0:
            return data, torch.empty((0, H, W), dtype=torch.uint8, device=dev)
        masks = ops.mask_binarize_crops(ctx["pool"], ctx["out"], m, ctx["geom"], ctx["ncrops"], sam.image_encoder.img_size, (H, W),
                                        sam.variant_id(), float(sam.mask_threshold))
        return data, masks

    def _zero_plane(self, H, W, dev):
        z = getattr(self, "_zero_planes", None)
        if z is None:
            z = self._zero_planes = {}
        key = (H, W, str(dev))
        if key not in z:
            z.clear()
            z[key] = torch.zeros((H, W), dtype=torch.float32, device=dev)
        return z[key]

    def _remove_small_regions(self, mask_u8, area_thresh, mode, cw):
        """utils/amg.py:267-291 on the device: connected components of the mask (islands) or of its complement (holes) with
        `psam_ccl`, areas from its table, relabelling through a small lookup table. -> (uint8 mask [H,W], changed)."""
        H, W = mask_u8.shape
        holes = mode == "holes"
        working = (1 - mask_u8) if holes else mask_u8
        ops.ccl(working.contiguous(), self._zero_plane(H, W, mask_u8.device), cw)
        tab = cw.tab.cpu().numpy()
        if int(tab[0]) > int(tab[1]):
            # more regions than the table has rows (speckled crop-resolution logits; cv2.connectedComponentsWithStats has no
            # limit): the union-find forest of the same labelling is complete - every foreground pixel of `working` holds its
            # region's root pixel - so the areas come from it; roots ascend like the table's rows, so ties break alike
            par = cw.parent.view(H, W)
            fgm = par >= 0
            _, inv, counts = torch.unique(par[fgm], return_inverse=True, return_counts=True)
            small_t = counts < area_thresh
            if not bool(small_t.any()):
                return mask_u8, False
            sel = torch.zeros((H, W), dtype=torch.uint8, device=mask_u8.device)
            if holes:
                sel[fgm] = small_t[inv].to(torch.uint8)
                return mask_u8 | sel, True
            keep = ~small_t
            if not bool(keep.any()):
                keep[int(counts.argmax())] = True
            sel[fgm] = keep[inv].to(torch.uint8)
            return sel, True
        n = int(tab[1])
        sizes = tab[ops.CC_HDR:ops.CC_HDR + ops.CC_STRIDE * n].reshape(n, ops.CC_STRIDE)[:, 0]
        small = [i + 1 for i, sz in enumerate(sizes) if sz < area_thresh]
        if len(small) == 0:
            return mask_u8, False
        fill = [0] + small
        if not holes:
            fill = [i for i in range(n + 1) if i not in fill]
            if len(fill) == 0:
                fill = [int(np.argmax(sizes)) + 1]
        lut = np.zeros(n + 1, np.uint8)
        lut[fill] = 1
        new = torch.from_numpy(lut).to(mask_u8.device)[cw.labels.view(H, W).long()]
        return new, True

    def _small_regions_device(self, data, masks):
        """The small-region stage (:332-380) of `_generate_general` on the device: holes and islands of all masks, their new areas
        and boxes and the stage's box NMS in one enqueued chain (`ops.small_regions_select`), one download of the decision. The
        kept records whose mask changed take the new box and area (:372-377); an unchanged mask equals its input, so the masks
        are one gather of the chain's output."""
        masks = masks.contiguous()
        nm, table = ops.small_regions_select(masks, self.min_mask_region_area, max(self.box_nms_thresh, self.crop_nms_thresh))
        keep, info, nb = ops.small_regions_table(table.cpu().numpy(), len(masks))   # the one download
        changed = keep[(info[keep, 0] | info[keep, 1]) != 0]
        data["boxes"][changed] = nb[changed]
        data["area"][changed] = info[changed, 2]
        return {k: v[keep] for k, v in data.items()}, nm[torch.from_numpy(keep).to(masks.device)]

    @torch.no_grad()
    def _generate_general(self, image):
        """-> (dict of host arrays, uint8 masks [m, H, W] on the device) over the final records."""
        if self.amg_crops == "device" and self.amg_resize == "fused":
            ctx = self._crops_enqueue(image)
            done = self._crops_finish(ctx, ctx["out"].cpu().numpy())           # the image's one copy and wait
            if done is not None:
                return self._small_region_stage(*done)
        return self._small_region_stage(*self._crops_host(image))              # PSAM_AMG_CROPS=host, or the pool overflowed

    def _crops_host(self, image):
        """The crops of the general path with the host between them (PSAM_AMG_CROPS=host): every crop waits for its statistics or
        its records, its survivors are binarised into full frames, and the cross-crop NMS runs on the host."""
        H, W = image.shape[:2]
        crop_boxes, layer_idxs = generate_crop_boxes((H, W), self.crop_n_layers, self.crop_overlap_ratio)
        parts = [self._process_crop(image, cb, li, (H, W)) for cb, li in zip(crop_boxes, layer_idxs)]
        data = {k: np.concatenate([p[k] for p in parts]) for k in parts[0] if k != "masks"}
        masks = torch.cat([p["masks"] for p in parts])
        dev = masks.device
        if len(crop_boxes) > 1:                                                 # :208-218 prefer masks from smaller crops
            cb = data["crop_boxes"].astype(np.float32)
            scores = 1.0 / ((cb[:, 2] - cb[:, 0]) * (cb[:, 3] - cb[:, 1]))
            keep = nms_xyxy(data["boxes"], scores, self.crop_nms_thresh)
            data = {k: v[keep] for k, v in data.items()}
            masks = masks[torch.from_numpy(keep).to(dev)]
        return data, masks

    def _small_region_stage(self, data, masks):
        """:332-380 behind the crops of either route; without min_mask_region_area > 0 it hands its arguments back."""
        H, W = masks.shape[1:]
        dev = masks.device
        if self.min_mask_region_area > 0 and len(masks) and self.amg_regions == "device":   # :332-380
            data, masks = self._small_regions_device(data, masks)
        elif self.min_mask_region_area > 0 and len(masks):
            cw = ops.CclWorkspace(H, W, 4096, dev)
            new_masks, scores = [], []
            for i in range(len(masks)):
                m, c1 = self._remove_small_regions(masks[i], self.min_mask_region_area, "holes", cw)
                m, c2 = self._remove_small_regions(m, self.min_mask_region_area, "islands", cw)
                new_masks.append(m)
                scores.append(float(not c1 and not c2))
            nm = torch.stack(new_masks)
            st, _ = ops.plane_stats(nm.float().contiguous(), 0.5, 0.0, binarize=False)
            st = st.cpu().numpy()
            nb = st[:, 3:7].astype(np.int64)
            nb[st[:, 2] == 0] = 0
            keep = nms_xyxy(nb, np.asarray(scores, dtype=np.float32), max(self.box_nms_thresh, self.crop_nms_thresh))
            for i in keep:
                if scores[i] == 0.0:
                    masks[i] = nm[i]
                    data["boxes"][i] = nb[i]
                    data["area"][i] = st[i, 2]
            data = {k: v[keep] for k, v in data.items()}
            masks = masks[torch.from_numpy(keep).to(dev)]
        return data, masks

    # ---- public API --------------------------------------------------------------------------------------------------
    def _segmentations(self, masks):
        """uint8 device masks [n, H, W] of the final records -> their `segmentation` values (:176-183): bool arrays (the one
        download of the masks), or RLEs encoded on the device in one call, of which only the run lengths are downloaded."""
        if self.output_mode == "binary_mask":
            return masks.cpu().numpy().astype(bool)
        rles = mask_to_rle_pytorch(masks)
        if self.output_mode == "coco_rle":
            rles = [coco_encode_rle(r) for r in rles]
        return rles

    @torch.no_grad()
    def generate(self, image):
        """image: HWC uint8 -> list of records {segmentation, area, bbox (XYWH), predicted_iou, point_coords,
        stability_score, crop_box} (:139-192). `segmentation` is a bool [H, W] array (output_mode "binary_mask"), the
        uncompressed RLE {"size", "counts": [ints]} ("uncompressed_rle") or its COCO string form ("coco_rle", needs
        pycocotools at construction as in the reference; `utils.amg.coco_encode_rle(rec["segmentation"])` on the
        "uncompressed_rle" records gives the same COCO record without the package)."""
        if not self._fused_path(image):
            return self._general_records(*self._generate_general(image))
        cand = self._candidates(image)
        masks, _ = self._binarize(cand)
        return self._fused_records(cand, masks)

    def _general_records(self, data, masks):
        """The records of the general path from `_generate_general`'s host arrays and uint8 device masks."""
        masks = self._segmentations(masks)
        anns = []
        for i in range(len(masks)):
            anns.append({
                "segmentation": masks[i],
                "area": int(data["area"][i]),
                "bbox": box_xyxy_to_xywh(data["boxes"][i]).tolist(),
                "predicted_iou": float(data["iou_preds"][i]),
                "point_coords": [data["points"][i].tolist()],
                "stability_score": float(data["stability_score"][i]),
                "crop_box": box_xyxy_to_xywh(data["crop_boxes"][i]).tolist(),
            })
        return anns

    @staticmethod
    def _general_device(data, masks, label, size):
        """`generate_device`'s triple for the general path: {tp, fp, fn} of every record against the label
        (models/SamWrapper.py:8-13), on the device."""
        counts = None
        if label is not None:
            lab = (label != 0)
            m = masks != 0
            counts = torch.stack([(m & lab).flatten(1).sum(1), (m & ~lab).flatten(1).sum(1), (~m & lab).flatten(1).sum(1)], 1)
        return dict(data, size=tuple(size)), masks, counts

    def _fused_records(self, cand, masks):
        """The records of the fused path from its candidate dict and the kept candidates' uint8 device masks."""
        masks = self._segmentations(masks)
        h, w = cand["size"]
        anns = []
        for i in range(len(masks)):
            anns.append({
                "segmentation": masks[i],
                "area": int(cand["area"][i]),
                "bbox": box_xyxy_to_xywh(cand["boxes"][i]).tolist(),
                "predicted_iou": float(cand["iou_preds"][i]),
                "point_coords": [cand["points"][i].tolist()],
                "stability_score": float(cand["stability_score"][i]),
                "crop_box": [0, 0, w, h],
            })
        return anns

    def _pipelined(self, images, finish, finish_general, fallback):
        """The fused path over several images with the host one image behind the device: image i's encode, decode, statistics and
        selection (`psam_amg_select`) are enqueued into buffer pair i % 2, its record table is copied to pinned memory behind an
        event, and the host waits for that event only after image i + 1 has been enqueued; then `finish(i, cand, low)` enqueues
        what works on the survivors. Every image is encoded and decoded by the calls `generate` makes, so its logits are the same
        bits. An image on the general path (crop layers, small-region removal) takes the crops' device route in the same way: all
        its crops are enqueued (`_crops_enqueue`, buffer set i % 2: the planes it needs later are in that set's pool, not in the
        decoder's output), its final table is copied to pinned memory behind an event, and after the wait
        `finish_general(i, data, masks)` gets what `_generate_general` returns. What that route does not cover
        (`_crops_device_ok`) goes to `fallback(i)`, one by one, after what is pending; an image whose plane pool overflowed takes
        the host route (`_crops_host`) after the last image."""
        out = [None] * len(images)
        pending = None

        def drain():
            nonlocal pending
            if pending is None:
                return
            i, ctx, records, host, ev = pending
            pending = None
            ev.synchronize()
            if records is not None:
                out[i] = finish(i, self._cand_from_records(ctx, host.numpy(), records), ctx["low"])
                return
            done = self._crops_finish(ctx, host.numpy())
            if done is None:
                overflowed.append(i)            # (after the loop: the host route writes self._low, which image i + 1 may still need)
            else:
                out[i] = finish_general(i, *self._small_region_stage(*done))

        overflowed = []

        k = 0
        for i, image in enumerate(images):
            if not self._fused_path(image):
                if not self._crops_device_ok():
                    drain()
                    out[i] = fallback(i)
                    continue
                if pending is not None and pending[2] is not None:
                    drain()                                                     # a pending fused image still needs self._low
                ctx = self._crops_enqueue(image, slot=k % 2)
                host = self._pinned(ctx["out"].numel(), k % 2)
                host.copy_(ctx["out"], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                drain()                                                         # image i - 1, while image i's crops run
                pending = (i, ctx, None, host, ev)
                k += 1
                continue
            ctx = self._enqueue(image, slot=k % 2)
            dev_out, records, _ = self._select_enqueue(ctx, out=self._select_out(ctx, k % 2))
            host = self._pinned(dev_out.numel(), k % 2)
            host.copy_(dev_out, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            drain()                                                             # image i - 1, while image i runs
            pending = (i, ctx, records, host, ev)
            k += 1
        drain()
        for i in overflowed:
            out[i] = finish_general(i, *self._small_region_stage(*self._crops_host(images[i])))
        return out

    def _select_out(self, ctx, slot):
        """the device tensor behind the records and count of buffer pair `slot`"""
        bufs = self.__dict__.setdefault("_sel_out", {})
        words = 3 * ctx["n"] * ops.AMG_REC + 1
        t = bufs.get(slot)
        if t is None or t.numel() != words or t.device != ctx["low"].device:
            t = bufs[slot] = torch.empty((words,), dtype=torch.int32, device=ctx["low"].device)
        return t

    def _pinned(self, words, slot):
        bufs = self.__dict__.setdefault("_sel_host", {})
        t = bufs.get(slot)
        if t is None or t.numel() != words:
            t = bufs[slot] = torch.empty((words,), dtype=torch.int32, pin_memory=True)
        return t

    @torch.no_grad()
    def generate_batch(self, images):
        """`[generate(im) for im in images]`, the same records, with the candidate selection on the device and the host's wait
        for image i behind the enqueue of image i + 1 (see `_pipelined`). Images on the general path (crop layers, small-region
        removal) take the crops' device route, whatever PSAM_AMG_CROPS says, with one wait per image behind the next image's crops;
        only PSAM_AMG_RESIZE=materialise, min_mask_region_area > 0 with PSAM_AMG_REGIONS=host, and an image whose plane pool
        overflowed are handled by the single-image host route, one by one."""
        images = list(images)
        return self._pipelined(images, lambda i, cand, low: self._fused_records(cand, self._binarize(cand, low=low)[0]),
                               lambda i, data, masks: self._general_records(data, masks), lambda i: self.generate(images[i]))

    @torch.no_grad()
    def generate_device_batch(self, images, labels=None):
        """`[generate_device(im, lab) for im, lab in zip(images, labels)]` in the same way: a list of (candidate dict, uint8 device
        masks [n,H,W], int64 [n,3] {tp, fp, fn} or None). `labels`: None, or one uint8 device label (or None) per image."""
        images = list(images)
        labels = [None] * len(images) if labels is None else list(labels)
        if len(labels) != len(images):
            raise ValueError(f"{len(images)} images but {len(labels)} labels")
        return self._pipelined(images, lambda i, cand, low: (cand,) + tuple(self._binarize(cand, labels[i], low=low)),
                               lambda i, data, masks: self._general_device(data, masks, labels[i], images[i].shape[:2]),
                               lambda i: self.generate_device(images[i], labels[i]))

    @torch.no_grad()
    def generate_device(self, image, label=None):
        """Device-resident variant for callers that reduce the masks further: -> (candidate dict, uint8 masks [n,H,W] on
        the device, int64 [n,3] {tp, fp, fn} against `label` or None)."""
        if not self._fused_path(image):
            return self._general_device(*self._generate_general(image), label, image.shape[:2])
        cand = self._candidates(image)
        masks, counts = self._binarize(cand, label)
        return cand, masks, counts


__all__ = ["SamAutomaticMaskGenerator", "area_from_rle"]
