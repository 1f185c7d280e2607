"""`ProtoMedSAM` on the HIP path (mirror of /root/reference/models/ProtoMedSAM.py:10-222).

Same constructor and `forward(query_image, coarse_model_input, degrees_rotate=0) -> (uint8 mask [H,W], [conf])` contract.
Differences from `ProtoSAM` that are reproduced: box prompts only; the image is min-max scaled to [0,1]
floats (no uint8 quantisation, no mean/std) before `medsam.image_encoder`; `mask_decoder(multimask_output=False)`;
`sigmoid` BEFORE the bilinear resize and a 0.5 threshold; the component confidences are computed from
`softmax(softmax(logits))` because `get_connected_components` re-applies softmax to the already-softmaxed tensor
(ProtoMedSAM.py:178-187, util/utils.py:485); an empty coarse mask returns the arg-max map at the ORIGINAL size (:194-197).
More than one connected component without `use_cca` is undefined in the reference (5-D nearest interpolate, SURVEY
Q16) and raises here.
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops
from .protosam import DECODER_CHUNK, MAX_COMPONENTS, MAX_COMPONENTS_LARGE, ModelWrapper, ProtoSAM
from .segment_anything import sam_model_registry

CCL_SLOTS = 32   # planes per connected-components launch chain of the batched paths (~8 MB of CCL scratch per slot at 1024^2)


class ProtoMedSAM(nn.Module):
    # the coarse-only paths are ProtoSAM's (ProtoMedSAM.py:163-172 is ProtoSAM.py:580-590)
    _coarse_only = ProtoSAM._coarse_only
    _coarse_only_batch = ProtoSAM._coarse_only_batch

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
        self._ccl = None
        self._bufs = {}
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

    # ---- the reference's helper methods by name (ProtoMedSAM.py:31-120,224-249); `forward` does their work inside fused kernels ----
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
        bufs = self._work(query_image.device)
        q = query_image.float().contiguous()
        ops.minmax(q, 1, mm=bufs["mm"])                                                  # (x - min) / (max - min), :230
        ops.sam_patchify(q, bufs["mm"], S, sam.image_encoder.patch_size, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), False, out=bufs["patches"])
        g = sam.image_encoder.grid
        emb = sam.image_encoder.encode_patches(bufs["patches"], 1).view(1, g, g, -1).permute(0, 3, 1, 2)
        medsam_seg, conf = self.medsam_inference(emb, bbox, H, W, query_label)
        medsam_seg = torch.tensor(medsam_seg, device=query_image.device)
        return medsam_seg.view(H, W), [conf]

    def _work(self, dev):
        if not self._bufs:
            self._bufs = dict(fg_sum=torch.zeros(1, dtype=torch.int32, device=dev),
                              prob=torch.empty((1, 2, 1024, 1024), dtype=torch.float32, device=dev),
                              prob2=torch.empty((1, 2, 1024, 1024), dtype=torch.float32, device=dev),
                              pred=torch.empty((1, 1024, 1024), dtype=torch.uint8, device=dev),
                              pred2=torch.empty((1, 1024, 1024), dtype=torch.uint8, device=dev),
                              q1024=torch.empty((1, 3, 1024, 1024), dtype=torch.float32, device=dev),
                              mm=torch.empty(2, dtype=torch.int32, device=dev),
                              patches=torch.empty((4096, 768), dtype=torch.float16, device=dev),
                              event=torch.cuda.Event())
            self._ccl = ops.CclWorkspace(1024, 1024, MAX_COMPONENTS, dev)
        return self._bufs

    @torch.no_grad()
    def forward(self, query_image, coarse_model_input, degrees_rotate=0):
        from .protosam import ProtoSAM
        original_size = query_image.shape[-2]
        dev = query_image.device
        # ProtoMedSAM.py:129-139 (rotation TTA around the coarse model; identity at 0 degrees)
        output_logits = ProtoSAM._coarse_logits(self, query_image, coarse_model_input, degrees_rotate)   # [1,2,H,W] ALP logits
        if self.coarse_pred_only:                                                          # ProtoMedSAM.py:163-172
            return ProtoSAM._coarse_only(self, output_logits, original_size)
        bufs = self._work(dev)
        sam = self.medsam
        S = sam.image_encoder.img_size
        bufs["fg_sum"].zero_()
        # bilinear to 1024 -> softmax (need_softmax is True for ALP logits, :178-179) -> argmax
        output_p, pred = ops.prob_argmax(output_logits.float().contiguous(), S, S, prob=bufs["prob"], pred=bufs["pred"],
                                         fg_sum=bufs["fg_sum"])
        # get_connected_components softmaxes its `logits` argument again (util/utils.py:485)
        p2, _ = ops.prob_argmax(output_p, S, S, prob=bufs["prob2"], pred=bufs["pred2"])
        cw = ops.ccl(pred[0], p2[0, 1], self._ccl, fg_sum=bufs["fg_sum"])
        cw.tab_host.copy_(cw.tab, non_blocking=True)
        bufs["event"].record()
        q = query_image.float().contiguous()
        if tuple(q.shape[-2:]) != (S, S):
            q = ops.bilinear_nchw(q, S, S, out=bufs["q1024"])
        ops.minmax(q, 1, mm=bufs["mm"])
        ops.sam_patchify(q, bufs["mm"], S, sam.image_encoder.patch_size, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), False,
                         out=bufs["patches"])                                              # :203-205
        feat_tok = sam.image_encoder.encode_patches(bufs["patches"], 1)[0]
        bufs["event"].synchronize()
        tab = cw.tab_host.numpy()
        if int(tab[0]) > int(tab[1]):   # more components than the fast table holds (cca searches ALL of them, utils.py:496-541)
            if getattr(self, "_ccl_big", None) is None:
                self._ccl_big = ops.CclWorkspace(1024, 1024, MAX_COMPONENTS_LARGE, dev)
            tab = ops.ccl(pred[0], p2[0, 1], self._ccl_big, fg_sum=bufs["fg_sum"]).tab.cpu().numpy()
            if int(tab[0]) > int(tab[1]):
                raise RuntimeError(f"{int(tab[0])} connected components exceed the table capacity {MAX_COMPONENTS_LARGE}")
        n = int(tab[1])
        self.last_stats = dict(n_components=int(tab[0]))
        if n == 0:                                                                         # :194-197
            return torch.zeros((original_size, original_size), dtype=torch.int64, device=dev), [0]
        rows = tab[ops.CC_HDR:ops.CC_HDR + ops.CC_STRIDE * n].reshape(n, ops.CC_STRIDE)
        if self.use_cca:
            rows = rows[int(tab[3]):int(tab[3]) + 1]
        if rows.shape[0] != 1:
            raise NotImplementedError("ProtoMedSAM with several components is undefined in the reference (SURVEY Q16); "
                                      "use use_cca=True")
        boxes = rows[:, 3:7] / np.array([S, S, S, S]) * max(self.image_size)               # :201-202 (identity at 1024)
        coords = boxes.reshape(-1, 2, 2).astype(np.float32)
        labels = np.tile(np.array([[2, 3]], dtype=np.int32), (coords.shape[0], 1))
        pe = sam.prompt_encoder._packed()
        dpk = sam.mask_decoder._packed()
        tokens = ops.prompt_tokens(torch.from_numpy(coords).to(dev), torch.from_numpy(labels).to(dev), pe["G"],
                                   pe["type_emb"], dpk["out_tok"], coords.shape[0], 2, float(S))
        masks, iou, _ = sam.mask_decoder.predict_masks_tokens(feat_tok, pe["pe_tok"], tokens, pe["no_mask"])
        seg = ops.mask_union(masks, 0, S, original_size, 3, 0.5)                           # sigmoid -> bilinear -> > 0.5
        self.last_stats.update(low_res=masks, iou=iou)
        return seg.to(torch.uint8), [iou[:, 0:1].cpu().numpy()]

    @torch.no_grad()
    def forward_classes(self, query_image, support_image, support_masks, val_wsize=2):
        """Throughput path of the multi-class loop (BASELINE config 5; /root/reference/validation.py:207 runs one 1-way episode per
        class on the same slice): ONE DINOv2 forward of the query (and of the support) shared by all classes' prototype banks, ONE
        MedSAM image-encoder forward of the query, one batched box-prompt decoder call for all classes. Returns a list of
        (uint8 mask [H,W], [conf]) per class, equal to `forward()` of each class alone (same arithmetic; the decoder batches).
        Only `use_cca=True` (one component per class), as `forward()`."""
        if not self.use_cca or self.coarse_pred_only:
            raise NotImplementedError("forward_classes: use_cca=True, coarse_pred_only=False")
        original_size = query_image.shape[-2]
        dev = query_image.device
        alp = self.coarse_segmentation_model.model
        logits = alp.forward_classes(support_image, support_masks, query_image, isval=True, val_wsize=val_wsize)
        bufs = self._work(dev)
        sam = self.medsam
        S = sam.image_encoder.img_size
        nc = len(logits)
        if len(getattr(self, "_cls_ws", [])) < nc:
            self._cls_ws = [dict(ccl=ops.CclWorkspace(1024, 1024, MAX_COMPONENTS, dev), fg=torch.zeros(1, dtype=torch.int32, device=dev),
                                 prob=torch.empty((1, 2, 1024, 1024), dtype=torch.float32, device=dev),
                                 pred=torch.empty((1, 1024, 1024), dtype=torch.uint8, device=dev)) for _ in range(nc)]
        cws = []
        for c, lg in enumerate(logits):
            w = self._cls_ws[c]
            w["fg"].zero_()
            output_p, pred = ops.prob_argmax(lg.float().contiguous(), S, S, prob=w["prob"], pred=w["pred"], fg_sum=w["fg"])
            p2, _ = ops.prob_argmax(output_p, S, S, prob=bufs["prob2"], pred=bufs["pred2"])
            cw = ops.ccl(pred[0], p2[0, 1], w["ccl"], fg_sum=w["fg"])
            cw.tab_host.copy_(cw.tab, non_blocking=True)
            cws.append(cw)
        bufs["event"].record()
        q = query_image.float().contiguous()
        if tuple(q.shape[-2:]) != (S, S):
            q = ops.bilinear_nchw(q, S, S, out=bufs["q1024"])
        ops.minmax(q, 1, mm=bufs["mm"])
        ops.sam_patchify(q, bufs["mm"], S, sam.image_encoder.patch_size, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), False, out=bufs["patches"])
        feat_tok = sam.image_encoder.encode_patches(bufs["patches"], 1)[0]
        bufs["event"].synchronize()
        results = [None] * nc
        boxes, owners = [], []
        for c, cw in enumerate(cws):
            tab = cw.tab_host.numpy()
            if int(tab[0]) > int(tab[1]):
                raise RuntimeError(f"class {c}: {int(tab[0])} connected components exceed the fast table; use forward() for this slice")
            n = int(tab[1])
            if n == 0:
                results[c] = (torch.zeros((original_size, original_size), dtype=torch.int64, device=dev), [0])
                continue
            rows = tab[ops.CC_HDR:ops.CC_HDR + ops.CC_STRIDE * n].reshape(n, ops.CC_STRIDE)
            row = rows[int(tab[3])]
            boxes.append(row[3:7] / np.array([S, S, S, S]) * max(self.image_size))
            owners.append(c)
        self.last_stats = dict(n_classes=nc, n_prompted=len(owners))
        if owners:
            coords = np.stack(boxes).reshape(-1, 2, 2).astype(np.float32)
            labels = np.tile(np.array([[2, 3]], dtype=np.int32), (coords.shape[0], 1))
            pe = sam.prompt_encoder._packed()
            dpk = sam.mask_decoder._packed()
            tokens = ops.prompt_tokens(torch.from_numpy(coords).to(dev), torch.from_numpy(labels).to(dev), pe["G"], pe["type_emb"],
                                       dpk["out_tok"], coords.shape[0], 2, float(S))
            masks, iou, _ = sam.mask_decoder.predict_masks_tokens(feat_tok, pe["pe_tok"], tokens, pe["no_mask"])
            iou_h = iou[:, 0:1].cpu().numpy()
            for k, c in enumerate(owners):
                seg = ops.mask_union(masks[k:k + 1], 0, S, original_size, 3, 0.5)
                results[c] = (seg.to(torch.uint8).clone(), [iou_h[k:k + 1]])
            self.last_stats.update(low_res=masks, iou=iou)
        return results

    # ---- batched paths: B slices (x C classes) per call --------------------------------------------------------------------
    def _batch_bufs(self, dev, P, B):
        """Buffers of the batched paths, grown to the largest P (planes) / B (slices) seen: per plane the uint8 arg-max map, the
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

    def _plane_table(self, p, bb, what):
        """Component table of plane p (host numpy); a plane with more components than the fast table is labelled again with the large
        table, as `forward` does (synchronous, rare)."""
        tab = bb["tabs_host"][p].numpy()
        if int(tab[0]) > int(tab[1]):
            if getattr(self, "_ccl_big", None) is None:
                self._ccl_big = ops.CclWorkspace(1024, 1024, MAX_COMPONENTS_LARGE, bb["pred"].device)
            tab = ops.ccl(bb["pred"][p], bb["pfg2"][p], self._ccl_big, fg_sum=bb["fg"][p:p + 1]).tab.cpu().numpy()
            if int(tab[0]) > int(tab[1]):
                raise RuntimeError(f"{what}: {int(tab[0])} connected components exceed the table capacity {MAX_COMPONENTS_LARGE}")
        return tab

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

    @torch.no_grad()
    def forward_batch(self, query_images, coarse_model_input, degrees_rotate=0):
        """MI355X extension, `ProtoSAM.forward_batch`'s contract: B query slices [B,3,H,W] through every stage as one batch.
        `coarse_model_input`: one input (shared support set) or a list of (input, n) pairs in batch order. Returns a list of
        (mask, [conf]) per slice, each what `forward` gives for that slice (uint8 [H,W]; int64 zeros and [0] for an empty coarse
        mask). Pipeline: one psam_prob2_argmax over the B planes, one connected-components chain (per CCL_SLOTS planes), the
        MedSAM encoder on the slices with a component only (as one sub-batch), one box-prompted decoder call, one
        psam_mask_union_seg."""
        B = query_images.shape[0]
        original_size = query_images.shape[-2]
        dev = query_images.device
        logits = ProtoSAM._coarse_logits(self, query_images, coarse_model_input, degrees_rotate)    # [B,2,H,W]
        if self.coarse_pred_only:                                                                   # ProtoMedSAM.py:163-172
            return self._coarse_only_batch(logits, original_size)
        S = self.medsam.image_encoder.img_size
        bb = self._batch_bufs(dev, B, B)
        self._coarse_to_components(logits.float().contiguous(), B, bb)
        # the encoder runs on the slices with foreground only (ProtoMedSAM.py:194-197 returns before it); it is enqueued before the
        # host waits for the tables, so that wait overlaps it
        bb["fg_event"].synchronize()
        keep = [b for b in range(B) if int(bb["fg_host"][b]) > 0]
        feat_row = [-1] * B
        feat_tok = None
        if keep:
            sub = query_images if len(keep) == B else query_images[torch.tensor(keep, device=dev)]
            feat_tok = self._medsam_features(sub, bb)
            for i, b in enumerate(keep):
                feat_row[b] = i
        bb["event"].synchronize()
        results = [None] * B
        stats, boxes, img_idx, owners = [], [], [], []
        for b in range(B):
            tab = self._plane_table(b, bb, f"slice {b}")
            n = int(tab[1])
            stats.append(dict(n_components=int(tab[0]), n_prompts=0, prompt=None))
            if n == 0:                                                                              # :194-197
                results[b] = (torch.zeros((original_size, original_size), dtype=torch.int64, device=dev), [0])
                continue
            rows = tab[ops.CC_HDR:ops.CC_HDR + ops.CC_STRIDE * n].reshape(n, ops.CC_STRIDE)
            if self.use_cca:
                rows = rows[int(tab[3]):int(tab[3]) + 1]
            if rows.shape[0] != 1:
                raise NotImplementedError(f"slice {b} of the batch: ProtoMedSAM with several components is undefined in the "
                                          "reference (SURVEY Q16); use use_cca=True")
            stats[b].update(n_prompts=1, prompt=len(boxes))
            boxes.append(rows[0, 3:7] / np.array([S, S, S, S]) * max(self.image_size))              # :201-202
            img_idx.append(feat_row[b])
            owners.append(b)
        self.last_stats = stats[0] if B == 1 else dict(per_slice=stats)
        if owners:
            masks, iou = self._decode_boxes(feat_tok, boxes, img_idx)
            segs = torch.tensor([[k, 1, k] for k in range(len(owners))], dtype=torch.int32).to(dev)
            out = ops.mask_union_seg(masks, 0, segs, len(owners), S, original_size, 3, 0.5)       # sigmoid -> bilinear -> > 0.5
            iou_h = iou[:, 0:1].cpu().numpy()
            for k, b in enumerate(owners):
                results[b] = (out[k], [iou_h[k:k + 1]])
            self.last_stats.update(low_res=masks, iou=iou)
        return results

    @torch.no_grad()
    def forward_classes_batch(self, query_images, support_image, support_masks, val_wsize=2, out=None):
        """The config-5 throughput path: B query slices [B,3,H,W] x C classes (support_masks: C masks of `support_image`) in one
        call. Returns results[b][c] = (mask, [conf]), equal to `forward_classes(query_images[b:b+1], ...)[c]`: the masks of the
        classes with a component are views of one uint8 [B,C,H,W] tensor (`out` if given), the others int64 zeros and [0] (that
        tensor holds zeros there too). Only `use_cca=True`, as `forward_classes`.
        Pipeline: ONE DINOv2 forward of the B slices matched against the C banks (FewShotSeg.class_scores: scores at grid
        resolution, class-major planes c*B + b), ONE psam_prob2_argmax over the P = B*C planes, the connected components in chunks
        of CCL_SLOTS planes, ONE MedSAM encoder forward of the slices where some class has a component, ONE decoder call over every
        (slice, class) box (chunked by DECODER_CHUNK), ONE psam_mask_union_seg into [B,C,H,W].
        Extra device memory at B = 32, C = 4, 1024^2: 640 MiB of per-plane maps (uint8 arg-max + fp32 softmax(softmax)), ~260 MiB of
        CCL scratch (32 slots), 128 MiB of output masks, 128 MiB of low-res decoder masks, plus the encoder's 32-slice workspace
        and the decoder's per-prompt workspace (measured peak: see DESIGN.md section 6)."""
        if not self.use_cca or self.coarse_pred_only:
            raise NotImplementedError("forward_classes_batch: use_cca=True, coarse_pred_only=False")
        B, H = query_images.shape[0], query_images.shape[-2]
        dev = query_images.device
        alp = self.coarse_segmentation_model.model
        sc = alp.class_scores(support_image, support_masks, query_images, isval=True, val_wsize=val_wsize)   # [C,B,2,g,g]
        C, g = sc.shape[0], sc.shape[-1]
        P = C * B
        S = self.medsam.image_encoder.img_size
        sc = sc.view(P, 2, g, g)
        img_size = tuple(support_image.shape[-2:])
        if img_size != (S, S):     # forward_classes resizes to the image size first, then to 1024 (two resamplings)
            sc = ops.bilinear_nchw(sc, img_size[0], img_size[1])
        bb = self._batch_bufs(dev, P, B)
        self._coarse_to_components(sc, P, bb)
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
        boxes, img_idx, owners = [], [], []
        for b in range(B):
            for c in range(C):
                p = c * B + b
                tab = bb["tabs_host"][p].numpy()
                if int(tab[0]) > int(tab[1]):
                    raise RuntimeError(f"slice {b}, class {c}: {int(tab[0])} connected components exceed the fast table; use "
                                       "forward() for this slice")
                n = int(tab[1])
                if n == 0:
                    results[b][c] = (torch.zeros((H, H), dtype=torch.int64, device=dev), [0])
                    continue
                row = tab[ops.CC_HDR + ops.CC_STRIDE * int(tab[3]):ops.CC_HDR + ops.CC_STRIDE * (int(tab[3]) + 1)]
                boxes.append(row[3:7] / np.array([S, S, S, S]) * max(self.image_size))
                img_idx.append(feat_row[b])
                owners.append((b, c))
        if out is None:
            out = torch.empty((B, C, H, H), dtype=torch.uint8, device=dev)
        assert out.shape == (B, C, H, H) and out.dtype == torch.uint8 and out.is_contiguous()
        prompt = {bc: k for k, bc in enumerate(owners)}
        # one segment per (slice, class): its prompt, or none (zeros)
        segs = np.zeros((B * C, 3), dtype=np.int32)
        for b in range(B):
            for c in range(C):
                k = prompt.get((b, c))
                segs[b * C + c] = (k, 1, b * C + c) if k is not None else (0, 0, b * C + c)
        masks = iou = None
        if owners:
            masks, iou = self._decode_boxes(feat_tok, boxes, img_idx)
        ops.mask_union_seg(masks, 0, torch.from_numpy(segs).to(dev), B * C, S, H, 3, 0.5, out=out.view(B * C, H, H))
        self.last_stats = dict(n_slices=B, n_classes=C, n_prompted=len(owners), prompt=prompt, n_encoded=len(keep))
        if owners:
            iou_h = iou[:, 0:1].cpu().numpy()
            for k, (b, c) in enumerate(owners):
                results[b][c] = (out[b, c], [iou_h[k:k + 1]])
            self.last_stats.update(low_res=masks, iou=iou)
        return results
