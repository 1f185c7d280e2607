"""`ProtoMedSAM` on the HIP path (mirror of /root/reference/models/ProtoMedSAM.py:10-222).

Same constructor and `forward(query_image, coarse_model_input, degrees_rotate=0) -> (uint8 mask [H,W], [conf])` contract.
Differences from `ProtoSAM` that are reproduced: box prompts only; the image is min-max scaled to [0,1]
floats (no uint8 quantisation, no mean/std) before `medsam.image_encoder`; `mask_decoder(multimask_output=False)`;
`sigmoid` BEFORE the bilinear resize and a 0.5 threshold; the component confidences are computed from
`softmax(softmax(logits))` because `get_connected_components` re-applies softmax to the already-softmaxed tensor
(ProtoMedSAM.py:178-187, util/utils.py:485); an empty coarse mask returns the arg-max map at the ORIGINAL size (:194-197).
More than one connected component without `use_cca` is undefined in the reference (5-D nearest interpolate, SURVEY
Q16) and raises here.

`forward` is `forward_batch` of one slice and `forward_classes` is `forward_classes_batch` of one slice; both batched paths run
one pipeline, `_segment`: psam_prob2_argmax (resize, softmax, arg-max, softmax again) -> connected components -> MedSAM encoder
of the slices with foreground -> one box per (slice, class) -> decoder -> psam_mask_union_seg.
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops
from .protosam import CCL_SLOTS, DECODER_CHUNK, MAX_COMPONENTS, ModelWrapper, ProtoSAM, class_support_scores
from .segment_anything import sam_model_registry


class ProtoMedSAM(nn.Module):
    # ProtoSAM's: the rotation TTA around the coarse model (ProtoMedSAM.py:129-139), the coarse-only path (ProtoMedSAM.py:163-172
    # is ProtoSAM.py:580-590) and the large-table relabelling of a plane with many components
    _coarse_logits = ProtoSAM._coarse_logits
    _coarse_only_batch = ProtoSAM._coarse_only_batch
    _ccl_large = ProtoSAM._ccl_large

    def __init__(self, image_size, coarse_segmentation_model: ModelWrapper,
                 sam_pretrained_path="pretrained_model/medsam_vit_b.pth", debug=False, use_cca=False,
                 coarse_pred_only=False):
        super().__init__()
        if isinstance(image_size, int):
            image_size = (image_size, image_size)
        self.image_size = image_size
        self.coarse_segmentation_model = coarse_segmentation_model
        self.get_sam(sam_pretrained_path)
        self.coarse_pred_only = coarse_pred_only
        self.debug = debug
        self.use_cca = use_cca
        if debug:
            raise NotImplementedError("debug plots are outside the accelerated path")
        if tuple(self.image_size) != (1024, 1024):
            raise NotImplementedError("image_size must be (1024, 1024) as in validation_protosam.py:234")
        self.last_stats = {}

    def get_sam(self, checkpoint_path):
        model_type = "vit_b"
        if checkpoint_path is not None and "vit_h" in checkpoint_path:
            model_type = "vit_h"
        if checkpoint_path is not None and checkpoint_path.startswith("random:"):
            from .synth import synth_state_dict
            parts = checkpoint_path.split(":")
            model_type = parts[1]
            seed = int(parts[2]) if len(parts) > 2 else 1234
            depth = int(parts[3]) if len(parts) > 3 else None
            self.medsam = sam_model_registry[model_type](encoder_depth=depth)
            self.medsam.load_state_dict(synth_state_dict(self.medsam, seed))
            self.medsam.eval()
        else:
            self.medsam = sam_model_registry[model_type](checkpoint=checkpoint_path).eval()

    # ---- the reference's helper methods by name (ProtoMedSAM.py:31-120,224-249); `_segment` does their work inside fused kernels ----
    @torch.no_grad()
    def medsam_inference(self, img_embed, box_1024, H, W, query_label=None):
        """ProtoMedSAM.py:31-66: box prompts [B,4] (XYXY in the 1024 frame) on ONE image embedding [1,256,64,64] -> (uint8 masks as
        numpy - `squeeze()`d like the reference: [H,W] for one box - , conf numpy [B,C]); sigmoid BEFORE the bilinear resize, 0.5
        threshold. With `query_label` the decoder returns its three masks and the one with the best IoU against the label is kept
        (`get_best_mask`), as [1,H,W]."""
        sam = self.medsam
        box_torch = torch.as_tensor(box_1024, dtype=torch.float, device=img_embed.device)
        if len(box_torch.shape) == 2:
            box_torch = box_torch[:, None, :]                                           # (B, 1, 4)
        sparse, dense = sam.prompt_encoder(points=None, boxes=box_torch, masks=None)
        low, conf = sam.mask_decoder(image_embeddings=img_embed, image_pe=sam.prompt_encoder.get_dense_pe(),
                                     sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense,
                                     multimask_output=True if query_label is not None else False)
        if H != W:
            raise NotImplementedError("medsam_inference: square outputs (psam_mask_union)")
        low = low.contiguous()
        n, C = low.shape[:2]
        segs = torch.stack([ops.mask_union(low[i:i + 1], c, int(H), int(H), 3, 0.5) for i in range(n) for c in range(C)])
        medsam_seg = segs.view(n, C, H, W).squeeze().to(torch.uint8).cpu().numpy()
        if query_label is not None:
            medsam_seg = self.get_best_mask(medsam_seg, query_label)[None, :]
        return medsam_seg, conf.cpu().detach().numpy()

    def get_iou(self, pred, label):
        """ProtoMedSAM.py:68-77 (numpy uint8 [h,w] each)."""
        tp = np.logical_and(pred, label).sum()
        fp = np.logical_and(pred, 1 - label).sum()
        fn = np.logical_and(1 - pred, label).sum()
        return tp / (tp + fp + fn)

    def get_best_mask(self, masks, labels):
        """ProtoMedSAM.py:79-92: masks numpy [B,h,w], labels tensor [1,H,W] -> the mask with the largest IoU (None when every IoU is 0)."""
        np_labels = labels[0].clone().detach().cpu().numpy()
        best_iou, best_mask = 0, None
        for mask in masks:
            iou = self.get_iou(mask, np_labels)
            if iou > best_iou:
                best_iou, best_mask = iou, mask
        return best_mask

    def get_bbox(self, pred):
        """ProtoMedSAM.py:94-106: [xmin, ymin, xmax, ymax] of the non-zero pixels of pred [H,W] (tensor or numpy), None when empty."""
        if isinstance(pred, np.ndarray):
            pred = torch.from_numpy(pred)
        if pred.max() == 0:
            return None
        indices = torch.nonzero(pred)
        ymin, xmin = indices.min(dim=0)[0]
        ymax, xmax = indices.max(dim=0)[0]
        return np.array([int(xmin), int(ymin), int(xmax), int(ymax)])

    def get_bbox_per_cc(self, conn_components):
        """ProtoMedSAM.py:109-120: one XYXY box per label 1 ... n-1 of a cv2-style `(n, labels, stats, centroids)` tuple
        (protosam_amd.utils.cca / get_connected_components)."""
        return np.array([self.get_bbox(torch.as_tensor(np.asarray(conn_components[1]) == i).to(torch.uint8))
                         for i in range(1, conn_components[0])])

    @torch.no_grad()
    def segment_all(self, query_image, query_label):
        """ProtoMedSAM.py:224-249: the whole-image box [0,0,W,H] as the prompt, three masks, the one closest to `query_label` kept.
        query_image [1,3,1024,1024] on the device (the reference hands it to the image encoder as it is)."""
        H, W = query_image.shape[-2:]
        sam = self.medsam
        S = sam.image_encoder.img_size
        if (H, W) != (S, S):
            raise ValueError(f"segment_all: the image encoder takes {S} x {S} images, got {(H, W)}")      # (the reference's encoder asserts)
        bbox = np.array([[0, 0, W, H]])
        g = sam.image_encoder.grid
        emb = self._medsam_features(query_image, self._batch_bufs(query_image.device, 1, 1)).view(1, g, g, -1).permute(0, 3, 1, 2)
        medsam_seg, conf = self.medsam_inference(emb, bbox, H, W, query_label)
        medsam_seg = torch.tensor(medsam_seg, device=query_image.device)
        return medsam_seg.view(H, W), [conf]

    @torch.no_grad()
    def forward(self, query_image, coarse_model_input, degrees_rotate=0):
        """Reference contract (ProtoMedSAM.py:122-222): one query slice [1,3,H,W] -> (uint8 mask [H,W], [conf]), or int64 zeros
        and [0] for an empty coarse mask; `forward_batch` of one slice."""
        return self.forward_batch(query_image, coarse_model_input, degrees_rotate)[0]

    @torch.no_grad()
    def forward_classes(self, query_image, support_image, support_masks, val_wsize=2):
        """Throughput path of the multi-class loop (BASELINE config 5; /root/reference/validation.py:207 runs one 1-way episode per
        class on the same slice): `forward_classes_batch` of one slice. Returns a list of (uint8 mask [H,W], [conf]) per class,
        equal to `forward()` of each class alone; the masks are views of one uint8 [1,C,H,W] tensor."""
        return self.forward_classes_batch(query_image, support_image, support_masks, val_wsize)[0]

    # ---- the pipeline: B slices x C classes per call -------------------------------------------------------------------------
    def _batch_bufs(self, dev, P, B):
        """Buffers of the pipeline, grown to the largest P (planes) / B (slices) seen: per plane the uint8 arg-max map, the
        softmax(softmax) foreground plane, the foreground count and (pinned) the component table; per slice the encoder input."""
        S = self.medsam.image_encoder.img_size
        bb = self.__dict__.setdefault("_bbufs", {})
        if bb.get("P", 0) < P:
            bb.update(P=P, pred=None, pfg2=None)          # (drop the old planes before allocating the larger ones)
            bb.update(pred=torch.empty((P, S, S), dtype=torch.uint8, device=dev),
                      pfg2=torch.empty((P, S, S), dtype=torch.float32, device=dev),
                      fg=torch.zeros(P, dtype=torch.int32, device=dev), fg_host=torch.zeros(P, dtype=torch.int32).pin_memory(),
                      tabs_host=torch.empty((P, ops.CC_HDR + ops.CC_STRIDE * MAX_COMPONENTS), dtype=torch.float64).pin_memory(),
                      fg_event=torch.cuda.Event(), event=torch.cuda.Event())
        if bb.get("B", 0) < B:
            bb.update(B=B, q1024=None)
            bb.update(q1024=torch.empty((B, 3, S, S), dtype=torch.float32, device=dev),
                      mm=torch.empty(2 * B, dtype=torch.int32, device=dev),
                      patches=torch.empty((B * 4096, 768), dtype=torch.float16, device=dev))
        slots = min(P, CCL_SLOTS)
        if getattr(self, "_ccl_chunk", None) is None or self._ccl_chunk.slots < slots:
            self._ccl_chunk = None
            self._ccl_chunk = ops.CclWorkspace(S, S, MAX_COMPONENTS, dev, slots=slots)
        return bb

    def _coarse_to_components(self, scores, P, bb):
        """scores fp32 [P,2,h,w] -> one psam_prob2_argmax launch (bilinear to 1024 unless already there, softmax, arg-max, foreground
        count, softmax again: ProtoMedSAM.py:176-187, util/utils.py:485) -> connected components in chunks of CCL_SLOTS planes, every
        table on its way to pinned host memory. Nothing waits: bb["fg_event"] marks the foreground counts, bb["event"] the tables."""
        S = self.medsam.image_encoder.img_size
        pred, pfg2, fg = bb["pred"][:P], bb["pfg2"][:P], bb["fg"][:P]
        fg.zero_()
        ops.prob2_argmax(scores, S, S, pred=pred, pfg2=pfg2, fg_sum=fg)
        bb["fg_host"][:P].copy_(fg, non_blocking=True)
        bb["fg_event"].record()
        cw = self._ccl_chunk
        for c0 in range(0, P, cw.slots):
            c1 = min(c0 + cw.slots, P)
            ops.ccl_planes(pred[c0:c1], pfg2[c0:c1], cw, fg_sum=fg[c0:c1])
            bb["tabs_host"][c0:c1].copy_(cw.tabs[:c1 - c0], non_blocking=True)   # (stream order: copied before the next chunk)
        bb["event"].record()

    def _medsam_features(self, imgs, bb):
        """min-max to [0,1] -> im2col -> MedSAM image encoder for the slices `imgs` [B',3,H,W] (ProtoMedSAM.py:203-205)
        -> token-major embeddings [B', 4096, 256]."""
        sam = self.medsam
        S = sam.image_encoder.img_size
        n = imgs.shape[0]
        q = imgs.float().contiguous()
        if tuple(q.shape[-2:]) != (S, S):
            q = ops.bilinear_nchw(q, S, S, out=bb["q1024"][:n])
        mm, patches = bb["mm"][:2 * n], bb["patches"][:n * 4096]
        ops.minmax(q, n, mm=mm)
        ops.sam_patchify(q, mm, S, sam.image_encoder.patch_size, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), False, out=patches)
        return sam.image_encoder.encode_patches(patches, n)

    def _decode_boxes(self, feat_tok, boxes, img_idx):
        """One box prompt per row of `boxes` (XYXY in the 1024 frame) on image img_idx[i] of feat_tok, all through the decoder in
        chunks of DECODER_CHUNK prompt sets (multimask_output=False: mask 0). -> low-res masks [n,4,256,256], iou [n,4]."""
        sam = self.medsam
        S = sam.image_encoder.img_size
        dev = feat_tok.device
        n = len(boxes)
        coords = torch.from_numpy(np.stack(boxes).reshape(-1, 2, 2).astype(np.float32)).to(dev)
        labels = torch.from_numpy(np.tile(np.array([[2, 3]], dtype=np.int32), (n, 1))).to(dev)
        iop = torch.tensor(img_idx, dtype=torch.int32).to(dev)
        pe = sam.prompt_encoder._packed()
        dpk = sam.mask_decoder._packed()
        tokens = ops.prompt_tokens(coords, labels, pe["G"], pe["type_emb"], dpk["out_tok"], n, 2, float(S))
        masks = torch.empty((n, 4, 256, 256), dtype=torch.float32, device=dev)
        iou = torch.empty((n, 4), dtype=torch.float32, device=dev)
        for c0 in range(0, n, DECODER_CHUNK):
            c1 = min(c0 + DECODER_CHUNK, n)
            sam.mask_decoder.predict_masks_tokens(feat_tok, pe["pe_tok"], tokens[c0:c1].contiguous(), pe["no_mask"],
                                                  img_of_prompt=iop[c0:c1].contiguous(), masks_out=masks[c0:c1],
                                                  iou_out=iou[c0:c1])
        return masks, iou

    def _segment(self, query_images, scores, C, relabel, out=None):
        """The pipeline under `forward_batch` (C = 1) and `forward_classes_batch`: B query slices [B,3,H,W] and the coarse scores fp32
        [P,2,h,w] of their P = C*B class-major planes (plane c*B + b is class c of slice b) -> `_coarse_to_components` -> the
        MedSAM encoder on the slices where some plane has foreground, as one sub-batch (ProtoMedSAM.py:194-197 returns before it;
        it is enqueued before the host waits for the tables, so that wait overlaps it) -> one box per plane with a component, the
        most confident one with `use_cca` (ProtoMedSAM.py:201-202) -> one decoder call -> one psam_mask_union_seg into uint8
        [B,C,H,W] (`out` if given; zeros where a plane has no prompt).
        A plane with more components than the fast table is labelled again with the large table if `relabel`, else an error.
        Returns (results[b][c] = (mask view [H,W], [conf]) or (int64 zeros, [0]), components found per plane, stats)."""
        B, H = query_images.shape[0], query_images.shape[-2]
        P = C * B
        dev = query_images.device
        S = self.medsam.image_encoder.img_size
        bb = self._batch_bufs(dev, P, B)
        self._coarse_to_components(scores, P, bb)
        bb["fg_event"].synchronize()
        fgh = bb["fg_host"][:P].view(C, B)
        keep = [b for b in range(B) if int(fgh[:, b].max()) > 0]
        feat_row = [-1] * B
        feat_tok = None
        if keep:
            sub = query_images if len(keep) == B else query_images[torch.tensor(keep, device=dev)]
            feat_tok = self._medsam_features(sub, bb)
            for i, b in enumerate(keep):
                feat_row[b] = i
        bb["event"].synchronize()
        results = [[None] * C for _ in range(B)]
        found = [0] * P
        prompt, boxes, img_idx = {}, [], []
        for b in range(B):
            for c in range(C):
                p = c * B + b
                tab = bb["tabs_host"][p].numpy()
                # more components than the fast table holds (cca searches ALL of them, utils.py:496-541)
                if int(tab[0]) > int(tab[1]):
                    if not relabel:
                        raise RuntimeError(f"slice {b}, class {c}: {int(tab[0])} connected components exceed the fast table; use "
                                           "forward() for this slice")
                    _, tab = self._ccl_large(bb["pred"][p], bb["pfg2"][p], bb["fg"][p:p + 1])
                found[p], n = int(tab[0]), int(tab[1])
                if n == 0:                                                                          # :194-197
                    results[b][c] = (torch.zeros((H, H), dtype=torch.int64, device=dev), [0])
                    continue
                if not self.use_cca and n != 1:
                    raise NotImplementedError(f"slice {b} of the batch: ProtoMedSAM with several components is undefined in the "
                                              "reference (SURVEY Q16); use use_cca=True")
                k = int(tab[3]) if self.use_cca else 0
                row = tab[ops.CC_HDR + ops.CC_STRIDE * k:ops.CC_HDR + ops.CC_STRIDE * (k + 1)]
                prompt[(b, c)] = len(boxes)
                boxes.append(row[3:7] / np.array([S, S, S, S]) * max(self.image_size))                # :201-202
                img_idx.append(feat_row[b])
        if out is None:
            out = torch.empty((B, C, H, H), dtype=torch.uint8, device=dev)
        assert out.shape == (B, C, H, H) and out.dtype == torch.uint8 and out.is_contiguous()
        # one segment per (slice, class): its prompt, or none (zeros)
        segs = np.array([(prompt.get((b, c), 0), int((b, c) in prompt), b * C + c) for b in range(B) for c in range(C)],
                        dtype=np.int32)
        masks = iou = None
        if boxes:
            masks, iou = self._decode_boxes(feat_tok, boxes, img_idx)
        # sigmoid -> bilinear -> > 0.5
        ops.mask_union_seg(masks, 0, torch.from_numpy(segs).to(dev), P, S, H, 3, 0.5, out=out.view(P, H, H))
        stats = dict(n_slices=B, n_classes=C, n_prompted=len(prompt), prompt=prompt, n_encoded=len(keep))
        if boxes:
            iou_h = iou[:, 0:1].cpu().numpy()
            for (b, c), k in prompt.items():
                results[b][c] = (out[b, c], [iou_h[k:k + 1]])
            stats.update(low_res=masks, iou=iou)
        return results, found, stats

    @torch.no_grad()
    def forward_batch(self, query_images, coarse_model_input, degrees_rotate=0):
        """MI355X extension, `ProtoSAM.forward_batch`'s contract: B query slices [B,3,H,W] through every stage as one batch.
        `coarse_model_input`: one input (shared support set) or a list of (input, n) pairs in batch order. Returns a list of
        (mask, [conf]) per slice, each what `forward` gives for that slice (uint8 [H,W]; int64 zeros and [0] for an empty coarse
        mask). Pipeline: `_segment` with one class."""
        original_size = query_images.shape[-2]
        logits = self._coarse_logits(query_images, coarse_model_input, degrees_rotate)             # [B,2,H,W]
        if self.coarse_pred_only:                                                                   # ProtoMedSAM.py:163-172
            return self._coarse_only_batch(logits, original_size)
        results, found, st = self._segment(query_images, logits.float().contiguous(), 1, relabel=True)
        prompt = st["prompt"]
        stats = [dict(n_components=found[b], n_prompts=int((b, 0) in prompt), prompt=prompt.get((b, 0)))
                 for b in range(len(results))]
        self.last_stats = stats[0] if len(stats) == 1 else dict(per_slice=stats)
        if "low_res" in st:
            self.last_stats.update(low_res=st["low_res"], iou=st["iou"])
        return [r[0] for r in results]

    @torch.no_grad()
    def forward_classes_batch(self, query_images, support_image=None, support_masks=None, val_wsize=2, out=None, supports=None):
        """The config-5 throughput path: B query slices [B,3,H,W] x C classes (support_masks: C masks of `support_image`) in one
        call. Returns results[b][c] = (mask, [conf]), equal to `forward_classes(query_images[b:b+1], ...)[c]`: the masks of the
        classes with a component are views of one uint8 [B,C,H,W] tensor (`out` if given), the others int64 zeros and [0] (that
        tensor holds zeros there too). Only `use_cca=True`.
        Pipeline: ONE DINOv2 forward of the B slices matched against the C banks (FewShotSeg.class_scores: scores at grid
        resolution, class-major planes c*B + b), then `_segment`: ONE psam_prob2_argmax over the P = B*C planes, the connected
        components in chunks of CCL_SLOTS planes, ONE MedSAM encoder forward of the slices where some class has a component, ONE
        decoder call over every (slice, class) box (chunked by DECODER_CHUNK), ONE psam_mask_union_seg into [B,C,H,W].
        Extra device memory at B = 32, C = 4, 1024^2: 640 MiB of per-plane maps (uint8 arg-max + fp32 softmax(softmax)), ~260 MiB of
        CCL scratch (32 slots), 128 MiB of output masks, 128 MiB of low-res decoder masks, plus the encoder's 32-slice workspace
        and the decoder's per-prompt workspace (measured peak: see DESIGN.md section 6).
        `supports=` (instead of support_image / support_masks): one support spec per class - one ALPNetInput or a list of
        (ALPNetInput, n) runs in batch order, any number of shots (`ProtoSAM.forward_classes_batch`) - and then results[b][c] is
        what `forward_batch(query_images, supports[c])[b]` gives."""
        if not self.use_cca or self.coarse_pred_only:
            raise NotImplementedError("forward_classes_batch: use_cca=True, coarse_pred_only=False")
        alp = self.coarse_segmentation_model.model
        if supports is not None:
            sc, img_size = class_support_scores(alp, supports, support_image, support_masks, query_images)
        else:
            sc = alp.class_scores(support_image, support_masks, query_images, isval=True, val_wsize=val_wsize)   # [C,B,2,g,g]
            img_size = tuple(support_image.shape[-2:])
        C, B, g = sc.shape[0], sc.shape[1], sc.shape[-1]
        S = self.medsam.image_encoder.img_size
        sc = sc.view(C * B, 2, g, g)
        if img_size != (S, S):     # the coarse logits live at the image size (FewShotSeg.forward): resized there first, then to 1024
            sc = ops.bilinear_nchw(sc, img_size[0], img_size[1])
        results, _, self.last_stats = self._segment(query_images, sc, C, relabel=False, out=out)
        return results
