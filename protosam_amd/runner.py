"""Volume-level driver: the per-slice loop of /root/reference/validation_protosam.py:346-388 (support per z-part,
one `ProtoSAM.forward` per query slice) plus data-parallel sharding of slices over ranks.

Slices are independent given the (replicated) support set, so rank r of W takes slices z = r (mod W) with no
data-path collective; the only exchange is one all-gather of the uint8 masks per volume / step.
"""
import math

import numpy as np
import torch
import torch.distributed as dist

from .grid_proto_fewshot import FewShotSeg
from .metrics import class_rows, surface_rows
from .protosam import ALPNetWrapper, InputFactory, ProtoSAM, TYPE_ALPNET
from .synth import synth_state_dict

ALP_CFG = {"which_model": "dinov2_b14", "cls_name": "grid_proto", "proto_grid_size": 8, "lora": 0, "align": False,
           "debug": False}


def build_protosam(device, sam_type="vit_h", image_size=512, seed=1234, dino_depth=None, sam_depth=None,
                   cache_support=True, heavy_tail=False, **protosam_kw):
    """Seeded synthetic-weight ProtoSAM as validation_protosam.get_model builds it (:188-232)."""
    cfg = dict(ALP_CFG)
    if dino_depth is not None:
        cfg["encoder_depth"] = dino_depth
    alp = FewShotSeg(image_size, None, cfg, cache_support=cache_support)
    alp_sd = synth_state_dict(alp, seed)
    alp.load_state_dict(alp_sd)
    alp = alp.to(device).eval()
    spec = ("random-heavy" if heavy_tail else "random") + f":{sam_type}:{seed}" + (f":{sam_depth}" if sam_depth is not None else "")
    kw = dict(use_bbox=True, use_points=True, point_mode="both", use_cca=False, num_points_for_sam=1,
              use_sam_trans=True)
    kw.update(protosam_kw)
    model = ProtoSAM(image_size=(1024, 1024), coarse_segmentation_model=ALPNetWrapper(alp), sam_pretrained_path=spec,
                     **kw).to(device).eval()
    return model, alp_sd


def part_assign(z, n_slices, n_parts=3):
    """dataloaders/common.py:241-249 style: equal z-chunks."""
    return min(int(z * n_parts / n_slices), n_parts - 1)


def support_set(vol, lab, n_parts=3):
    """Middle slice of each z-chunk of the support volume (ManualAnnoDatasetv2.py:457-462), tiled x3."""
    n = vol.shape[0]
    imgs, masks = [], []
    for p in range(n_parts):
        z = int((p + 0.5) * n / n_parts)
        imgs.append(vol[z][None, None].repeat(1, 3, 1, 1).contiguous())
        masks.append(lab[z][None].contiguous())
    return imgs, masks


def shard_slices(n_slices, rank, world):
    return list(range(rank, n_slices, world))


def _batch_dst(out, buf, i, j):
    """where the masks of slices i..j-1 go: their rows of the whole-run tensor `out`, or the front of the reused batch buffer"""
    return out[i:j] if out is not None else buf[:j - i]


@torch.no_grad()
def run_slices(model, vol, sup_imgs, sup_masks, zs, device, out=None, batch=1, mix_parts=True):
    """Runs ProtoSAM on slices `zs` of `vol` [n,S,S] (device tensor), `batch` slices at a time through `forward_batch`; returns uint8
    masks [len(zs),S,S] and the number of prompts per slice. A batch may span z-parts (different support sets: the batch then carries
    one (input, count) pair per part - only the prototype match is done per part); mix_parts=False cuts batches at part boundaries."""
    if out is None:
        out = torch.zeros((len(zs), vol.shape[-1], vol.shape[-1]), dtype=torch.uint8, device=device)
    return out, _slices_loop(model, vol, sup_imgs, sup_masks, zs, device, out, None, batch, mix_parts, None)


def _slices_loop(model, vol, sup_imgs, sup_masks, zs, device, out, buf, batch, mix_parts, sink):
    """The loop of `run_slices`. The masks of a batch go to `out[i:j]`, or to the batch buffer `buf` when out is None;
    sink(i, j, masks) is then called with them (`evaluate_slices` scores them there). -> prompts per slice."""
    n, S = vol.shape[0], vol.shape[-1]
    stats = [0] * len(zs)
    inputs = {}

    def part_input(part, q):
        if part not in inputs:
            inputs[part] = InputFactory.create_input(TYPE_ALPNET, q, support_images=[sup_imgs[part]],
                                                     support_labels=[sup_masks[part]], isval=True, val_wsize=2)
        return inputs[part]
    i = 0
    while i < len(zs):
        part = part_assign(zs[i], n)
        j = i
        while j < len(zs) and j - i < batch and (mix_parts and batch > 1 or part_assign(zs[j], n) == part):
            j += 1
        idx = torch.tensor(zs[i:j], device=device)
        q = vol[idx][:, None].expand(j - i, 3, S, S).contiguous()
        if batch == 1:
            res = [model(q, part_input(part, q), degrees_rotate=0)]
            st = [model.last_stats]
        else:
            runs = []                                   # consecutive slices of one part
            for z in zs[i:j]:
                pz = part_assign(z, n)
                if runs and runs[-1][0] == pz:
                    runs[-1][1] += 1
                else:
                    runs.append([pz, 1])
            cin = part_input(part, q) if len(runs) == 1 else [(part_input(pz, q), cnt) for pz, cnt in runs]
            res = model.forward_batch(q, cin)
            st = model.last_stats.get("per_slice", [model.last_stats])
        dst = _batch_dst(out, buf, i, j)
        for k, (pred, scores) in enumerate(res):
            if pred.shape[-1] == S:
                dst[k].copy_(pred)                # ({0., 1.} -> uint8 inside the one copy kernel)
            else:   # empty coarse mask: the reference hands back the all-zero 1024x1024 arg-max map (ProtoSAM.py:612-613)
                dst[k].zero_()
            stats[i + k] = st[k].get("n_prompts", 0) if k < len(st) else 0
        if sink is not None:
            sink(i, j, dst)
        i = j
    return stats


@torch.no_grad()
def run_slices_classes(model, vol, sup_imgs, sup_masks_per_part, zs, device, batch=16, out=None):
    """The multi-class form of `run_slices` (BASELINE config 5; the reference runs one 1-way episode per class, validation.py:207):
    slices `zs` of `vol` [n,S,S] against C classes, `batch` slices per `model.forward_classes_batch` call (a ProtoMedSAM or a
    ProtoSAM). Part p of the scan has its own support image sup_imgs[p] and C masks sup_masks_per_part[p]; batches are cut at part
    boundaries.
    Returns uint8 masks [len(zs), C, S, S] (the batch's output tensor is a slice of it) and the number of prompted classes per
    slice."""
    if out is None:
        out = torch.zeros((len(zs), len(sup_masks_per_part[0]), vol.shape[-1], vol.shape[-1]), dtype=torch.uint8, device=device)
    return out, _slices_classes_loop(model, vol, sup_imgs, sup_masks_per_part, zs, device, batch, out, None, None)


def _collect_classes(model, res, dst, stats, i):
    """after a forward_classes_batch(out=dst) call on the slices from i on: the masks it did not write into dst, and the counts"""
    for k, per_class in enumerate(res):
        for c, (mask, _) in enumerate(per_class):
            if mask.data_ptr() != dst[k, c].data_ptr():        # (an empty class: int64 zeros, and zeros in `dst` already)
                dst[k, c].copy_(mask)
    for (k, _) in model.last_stats.get("prompt", {}):          # (slice, class) pairs that went to the decoder
        stats[i + k] += 1


def _slices_classes_loop(model, vol, sup_imgs, sup_masks_per_part, zs, device, batch, out, buf, sink):
    """The loop of `run_slices_classes`; out / buf / sink as `_slices_loop`."""
    n, S = vol.shape[0], vol.shape[-1]
    stats = [0] * len(zs)
    i = 0
    while i < len(zs):
        part = part_assign(zs[i], n)
        j = i
        while j < len(zs) and j - i < batch and part_assign(zs[j], n) == part:
            j += 1
        idx = torch.tensor(zs[i:j], device=device)
        q = vol[idx][:, None].expand(j - i, 3, S, S).contiguous()
        dst = _batch_dst(out, buf, i, j)
        res = model.forward_classes_batch(q, sup_imgs[part], sup_masks_per_part[part], out=dst)
        _collect_classes(model, res, dst, stats, i)
        if sink is not None:
            sink(i, j, dst)
        i = j
    return stats


def _class_zlists(label_vol, classes):
    """per class: the sorted z indices of label_vol [Z,H,W] (tensor or array of integer labels) where the class has a pixel (the
    reference's per-scan `tp1_cls_map` lists); ValueError for a class the scan does not hold"""
    lab = label_vol.detach().cpu().numpy() if isinstance(label_vol, torch.Tensor) else np.asarray(label_vol)
    out = []
    for c in classes:
        zl = np.nonzero((lab == c).reshape(lab.shape[0], -1).any(axis=1))[0].tolist()
        if not zl:
            raise ValueError(f"class {c} is absent from the scan (the reference's min() of its empty z-list fails)")
        out.append(zl)
    return out


def class_part_table(label_vol, classes, n_parts=3):
    """The z-part of every query slice per class -> int64 [C, Z] (dataloaders/common.py:236-249): slice z belongs to part
    int((z - z_min) // ((z_max - z_min) / n_parts)) of class c, with z_min / z_max the class's own extent in this scan (float floor
    division), part 0 where z_max == z_min (the reference's `except`), clipped to [0, n_parts - 1]. The same slice can be in
    different parts for different classes."""
    zls = _class_zlists(label_vol, classes)
    Z = label_vol.shape[0]
    tab = np.zeros((len(classes), Z), dtype=np.int64)
    for c, zl in enumerate(zls):
        z_min, z_max = min(zl), max(zl)
        for z in range(Z):
            try:
                part = int((z - z_min) // ((z_max - z_min) / n_parts))
            except ZeroDivisionError:
                part = 0
            tab[c, z] = min(max(part, 0), n_parts - 1)
    return tab


def class_support_slices(sup_label_vol, classes, n_parts=3):
    """The support slice of every (class, part) -> [C][n_parts] z indices of the support scan (ManualAnnoDatasetv2.py:457-477): part p
    of class c takes zlist[int(pcts[p] * len(zlist))] of the class's own z-list, pcts = [0.5] for one part, else the centres
    1/(2 n) + p (1 - 1/n) / (n - 1). n_parts must be odd, as the reference asserts."""
    if n_parts % 2 != 1:
        raise ValueError(f"n_parts must be odd (the reference asserts npart % 2 == 1), got {n_parts}")
    if n_parts == 1:
        pcts = [0.5]
    else:
        half_part = 1 / (n_parts * 2)
        part_interval = (1.0 - 1.0 / n_parts) / (n_parts - 1)
        pcts = [half_part + part_interval * ii for ii in range(n_parts)]
    return [[zl[int(pcts[p] * len(zl))] for p in range(n_parts)] for zl in _class_zlists(sup_label_vol, classes)]


def class_support_specs(supports, part_table, zs):
    """The `supports=` argument of forward_classes_batch for the slices zs of one batch: per class c, supports[c][p] of the part p of
    every slice (part_table[c][z]), as one input when the batch lies in one part, else as (input, n) runs of equal part."""
    specs = []
    for c in range(len(supports)):
        runs = []                                   # consecutive slices of one part of class c
        for z in zs:
            p = int(part_table[c][z])
            if runs and runs[-1][0] == p:
                runs[-1][1] += 1
            else:
                runs.append([p, 1])
        specs.append(supports[c][runs[0][0]] if len(runs) == 1 else [(supports[c][p], n) for p, n in runs])
    return specs


@torch.no_grad()
def run_slices_class_supports(model, vol, supports, part_table, zs, batch=16, out=None):
    """`run_slices_classes` as the reference evaluates (one 1-way episode per organ): class c has a support input of its own per
    z-part, supports[c][p] (an ALPNetInput, one or more shots), and slice z is matched against supports[c][part_table[c][z]]
    (`class_part_table`). `batch` consecutive slices go to one `model.forward_classes_batch(..., supports=...)` call whatever
    their parts: each class's runs of equal part become its (input, n) list.
    Returns uint8 masks [len(zs), C, S, S] and the number of prompted classes per slice, as `run_slices_classes`."""
    if out is None:
        out = torch.zeros((len(zs), len(supports), vol.shape[-1], vol.shape[-1]), dtype=torch.uint8, device=vol.device)
    return out, _slices_class_supports_loop(model, vol, supports, part_table, zs, batch, out, None, None)


def _slices_class_supports_loop(model, vol, supports, part_table, zs, batch, out, buf, sink):
    """The loop of `run_slices_class_supports`; out / buf / sink as `_slices_loop`."""
    S, dev = vol.shape[-1], vol.device
    stats = [0] * len(zs)
    for i in range(0, len(zs), batch):
        zb = list(zs[i:i + batch])
        idx = torch.tensor(zb, device=dev)
        q = vol[idx][:, None].expand(len(zb), 3, S, S).contiguous()
        specs = class_support_specs(supports, part_table, zb)
        dst = _batch_dst(out, buf, i, i + len(zb))
        res = model.forward_classes_batch(q, supports=specs, out=dst)
        _collect_classes(model, res, dst, stats, i)
        if sink is not None:
            sink(i, i + len(zb), dst)
    return stats


# ---- evaluation: score every batch where it lies; only a [rows, 12] table is kept --------------------------
def _scoring(labels, zs, classes, keep, batch, shape, device, label_value=1, surface=None):
    """table, batch buffer and sink of the evaluate_* functions. shape: of one slice's masks ([C, S, S] or [S, S]).
    surface: None, or dict(spacing=(sy, sx) or (sz, sy, sx), cap=None): the sink also fills a per-slice surface table float64
    [rows, 8] (ops.SURF_COLS) with one `ops.surface_distances` per batch; it is the fourth value returned (None without)."""
    from . import ops
    per = 1 if classes is None else len(classes)
    table = torch.empty((len(zs) * per, 12), dtype=torch.int64, device=device)
    if keep is not None:
        assert tuple(keep.shape) == (len(zs),) + tuple(shape) and keep.dtype == torch.uint8 and keep.is_contiguous()
    buf = None if keep is not None else torch.empty((min(batch, len(zs)),) + tuple(shape), dtype=torch.uint8, device=device)
    surf = None
    if surface is not None:
        spacing, cap = ops._surface_spacing(surface["spacing"]), surface.get("cap")
        surf = torch.empty((len(zs) * per, 8), dtype=torch.float64, device=device)

    def sink(i, j, masks):
        rows = class_rows(j - i, classes, label_planes=zs[i:j], label_value=label_value)
        ops.seg_counts(masks, labels, rows.tolist(), out=table[i * per:j * per])
        if surf is not None:
            srows = surface_rows(j - i, classes, label_planes=zs[i:j], label_value=label_value)
            ops.surface_distances(masks, labels, srows.tolist(), spacing, cap=cap, out=surf[i * per:j * per])
    return table, buf, sink, surf


def _with_surface(table, stats, surf):
    """the return value of the evaluate_slices* functions: as it always was without surface=, the surface table appended with it"""
    return (table, stats) if surf is None else (table, stats, surf)


@torch.no_grad()
def evaluate_slices(model, vol, labels, sup_imgs, sup_masks, zs, device, batch=1, mix_parts=True, keep=None, label_value=1,
                    surface=None):
    """`run_slices` scored in place: the masks of each batch go to ONE reused batch-sized buffer and one `ops.seg_counts` compares
    them with `labels` [Z, S, S] (the scan's label volume on the device, true where == label_value). Returns the int64 table
    [len(zs), 12] (ops.SEG_COLS; still on the device, nothing synchronised) and the prompts per slice. keep= (uint8
    [len(zs), S, S]) also receives the masks, as `run_slices(..., out=keep)`.
    surface=dict(spacing=(sy, sx) or (sz, sy, sx)[, cap=]): a third value, the per-slice surface table float64 [len(zs), 8]
    (ops.SURF_COLS: HD, HD95, ASSD of every slice, `metrics.score_surfaces` reads it), filled batch by batch beside the counts; the
    default changes nothing."""
    S = vol.shape[-1]
    table, buf, sink, surf = _scoring(labels, list(zs), None, keep, batch, (S, S), device, label_value, surface)
    return _with_surface(table, _slices_loop(model, vol, sup_imgs, sup_masks, zs, device, keep, buf, batch, mix_parts, sink), surf)


@torch.no_grad()
def evaluate_slices_classes(model, vol, labels, sup_imgs, sup_masks_per_part, zs, classes, device, batch=16, keep=None,
                            surface=None):
    """`run_slices_classes` scored in place against the label volume `labels` [Z, S, S]: class c of the call is organ classes[c].
    One reused [batch, C, S, S] buffer, one `ops.seg_counts` per model call. Returns the int64 table [len(zs) * C, 12] (row
    k * C + c = slice zs[k], class c; on the device) and the prompted classes per slice. keep= (uint8 [len(zs), C, S, S]) also
    receives the masks. surface= as `evaluate_slices`: a third value, the surface table float64 [len(zs) * C, 8], rows as the counts."""
    S, C = vol.shape[-1], len(classes)
    assert C == len(sup_masks_per_part[0])
    table, buf, sink, surf = _scoring(labels, list(zs), classes, keep, batch, (C, S, S), device, surface=surface)
    return _with_surface(table, _slices_classes_loop(model, vol, sup_imgs, sup_masks_per_part, zs, device, batch, keep, buf, sink),
                         surf)


@torch.no_grad()
def evaluate_slices_class_supports(model, vol, labels, supports, part_table, zs, classes, batch=16, keep=None, surface=None):
    """`run_slices_class_supports` scored in place; table, counts, keep= and surface= as `evaluate_slices_classes`."""
    S, C = vol.shape[-1], len(classes)
    assert C == len(supports)
    table, buf, sink, surf = _scoring(labels, list(zs), classes, keep, batch, (C, S, S), vol.device, surface=surface)
    return _with_surface(table, _slices_class_supports_loop(model, vol, supports, part_table, zs, batch, keep, buf, sink), surf)


@torch.no_grad()
def score_scan_surfaces(keep, labels, classes, spacing, zs=None, cap=None):
    """The boundary measures of a whole scan in 3-D: keep uint8 [Z, C, S, S] (the masks evaluate_slices_classes(..., keep=) left; [Z,
    S, S] with classes = None: one class, true where labels == 1) against the label volume `labels` [Z', S, S]; slice k of keep is
    label plane zs[k] (default k). One row per class over the kept volume with depth Z (6-neighbour surfaces, the first and last
    kept slice count as the volume's faces), spacing (sz, sy, sx) as slice_io.read_nifti's header gives it. One launch chain for
    all classes; rows that overflow the default pool are recomputed (`metrics.surface_table`).
    -> float64 array [C, 8] on the host (ops.SURF_COLS; `metrics.score_surfaces` reads it). It synchronises."""
    from .metrics import surface_table
    Z = keep.shape[0]
    if keep.dim() != (3 if classes is None else 4) or (classes is not None and keep.shape[1] != len(classes)):
        raise ValueError(f"keep {tuple(keep.shape)} does not hold {None if classes is None else len(classes)} classes per slice")
    vol = (keep[None] if keep.dim() == 3 else keep.permute(1, 0, 2, 3)).contiguous()          # class-major volumes
    zs = list(range(Z)) if zs is None else [int(z) for z in zs]
    if len(zs) != Z:
        raise ValueError(f"zs has {len(zs)} entries for {Z} kept slices")
    if zs == list(range(zs[0], zs[0] + Z)):
        lab, first = labels, zs[0]
    else:
        lab, first = labels[torch.tensor(zs, device=labels.device)], 0
    rows = surface_rows(1, classes, label_planes=[first], depth=Z)
    return surface_table(vol.reshape((-1,) + tuple(vol.shape[-2:])), lab, rows.tolist(), spacing, cap=cap)


def _kept_classes(keep, classes):
    if keep.dim() != (3 if classes is None else 4) or (classes is not None and keep.shape[1] != len(classes)):
        raise ValueError(f"keep {tuple(keep.shape)} does not hold {None if classes is None else len(classes)} classes per slice")


@torch.no_grad()
def clean_scan(keep, classes=None, connectivity=26, min_voxels=0, keep_largest=True, out=None):
    """The connected-component clean-up of a kept scan in 3-D, per class, on the device (`ops.volume_regions`): keep uint8 [Z, C,
    S, S] as evaluate_slices_classes(..., keep=) left it (read where it lies, no class-major copy), or [Z, S, S] with classes =
    None. Every component (connectivity 6 / 18 / 26) below min_voxels voxels is dropped; keep_largest keeps only the largest
    survivor of each class, ties to the first in raster order. out=keep cleans in place.
    -> (cleaned uint8 shaped as keep, info int64 [C, 12] on the device: ops.VOLREG_COLS, `ops.volume_regions_table` reads it).
    Nothing is synchronised."""
    from . import ops
    _kept_classes(keep, classes)
    return ops.volume_regions(keep, connectivity=connectivity, min_voxels=min_voxels, keep_largest=keep_largest, out=out,
                              layout="rdhw" if keep.dim() == 3 else "zchw")


@torch.no_grad()
def score_scan(keep, labels, classes, zs=None):
    """The scan-level counts of kept (or cleaned) masks: keep uint8 [Z, C, S, S] ([Z, S, S] with classes = None: one class, true
    where labels == 1) against the label volume `labels` [Z', S, S]; slice k of keep is label plane zs[k] (default k). One
    `ops.seg_counts` over every (slice, class), reduced over the slices on the device: counts summed, boxes united.
    -> int64 [C, 12] (ops.SEG_COLS; an empty box is (INT32_MAX, INT32_MAX, -1, -1) as seg_counts leaves it), on the device,
    nothing synchronised."""
    from . import ops
    _kept_classes(keep, classes)
    Z = keep.shape[0]
    zs = list(range(Z)) if zs is None else [int(z) for z in zs]
    if len(zs) != Z:
        raise ValueError(f"zs has {len(zs)} entries for {Z} kept slices")
    per = ops.seg_counts(keep, labels, class_rows(Z, classes, label_planes=zs).tolist()).view(Z, -1, 12)
    lo, hi = per.amin(dim=0), per.amax(dim=0)
    return torch.cat([per[..., :4].sum(dim=0), lo[:, 4:6], hi[:, 6:8], lo[:, 8:10], hi[:, 10:12]], dim=1)


# ---- image sets (image_io.ImageSet): the polyp branch of validation_protosam.py:307-449 -----------------------------------------
@torch.no_grad()
def run_images(model, image_set, support, indices, batch=4, out=None):
    """Runs ProtoSAM on the images `indices` of `image_set`, `batch` at a time through `forward_batch` (a last short batch is
    allowed). support: (images, masks) lists of [1,3,S,S] / [1,S,S] as `ImageSet.get_support` returns them; the support input is
    built once, so its features stay cached as in `run_slices`. -> uint8 masks [len(indices), S, S], prompts per image and the
    confidence lists per image."""
    indices = list(indices)
    if out is None:
        out = torch.zeros((len(indices), image_set.S, image_set.S), dtype=torch.uint8, device=image_set.device)
    stats, scores, _ = _images_loop(model, image_set, support, indices, batch, out, None, None)
    return out, stats, scores


def _images_loop(model, image_set, support, indices, batch, out, buf, sink):
    """The loop of `run_images`; out / buf as `_slices_loop`; sink(i, j, masks, labels) gets each batch's masks and loaded labels.
    -> prompts per image, confidences per image, case per image."""
    S = image_set.S
    stats, scores, cases = [0] * len(indices), [None] * len(indices), [None] * len(indices)
    cin = None
    for i in range(0, len(indices), max(int(batch), 1)):
        j = min(i + max(int(batch), 1), len(indices))
        q, labels, _, cs = image_set.load(indices[i:j])
        if cin is None:
            cin = InputFactory.create_input(TYPE_ALPNET, q, support_images=list(support[0]), support_labels=list(support[1]),
                                            isval=True, val_wsize=2)
        res = model.forward_batch(q, cin)
        st = model.last_stats.get("per_slice", [model.last_stats])
        dst = _batch_dst(out, buf, i, j)
        for k, (pred, sc) in enumerate(res):
            if pred.shape[-1] == S:
                dst[k].copy_(pred)
            else:                                 # empty coarse mask: the all-zero 1024 x 1024 arg-max map (ProtoSAM.py:612-613)
                dst[k].zero_()
            stats[i + k] = st[k].get("n_prompts", 0) if k < len(st) else 0
            scores[i + k] = sc
            cases[i + k] = cs[k]
        if sink is not None:
            sink(i, j, dst, labels)
    return stats, scores, cases


@torch.no_grad()
def evaluate_images(model, image_set, support, indices, batch=4, keep=None, skip_no_organ_slices=True, surface=None):
    """`run_images` scored where each batch lies: one `ops.seg_counts` per batch against the batch's own labels, then
    `metrics.score_slices` on the table with the per-image confidences and cases. -> its dict (dice / iou / precision / recall, their
    means, per-case means, "bboxes_w_scores" for `metrics.eval_detection`) plus "table" (int64 [n, 12], host) and "n_prompts".
    keep= (uint8 [len(indices), S, S]) also receives the masks.
    surface=dict(spacing=(sy, sx)[, cap=]): also "surface_table" (float64 [n, 8], host, ops.SURF_COLS: HD, HD95, ASSD per image) and
    "surface" (`metrics.score_surfaces` of it with the cases); the default leaves the dict as it was."""
    from . import ops
    from .metrics import score_slices, score_surfaces
    indices = list(indices)
    S, dev = image_set.S, image_set.device
    table = torch.empty((len(indices), 12), dtype=torch.int64, device=dev)
    if keep is not None:
        assert tuple(keep.shape) == (len(indices), S, S) and keep.dtype == torch.uint8 and keep.is_contiguous()
    buf = None if keep is not None else torch.empty((min(max(int(batch), 1), len(indices)), S, S), dtype=torch.uint8, device=dev)

    surf = None
    if surface is not None:
        spacing, cap = ops._surface_spacing(surface["spacing"]), surface.get("cap")
        surf = torch.empty((len(indices), 8), dtype=torch.float64, device=dev)

    def sink(i, j, masks, labels):
        ops.seg_counts(masks, labels, class_rows(j - i).tolist(), out=table[i:j])
        if surf is not None:
            ops.surface_distances(masks, labels, surface_rows(j - i).tolist(), spacing, cap=cap, out=surf[i:j])
    stats, scores, cases = _images_loop(model, image_set, support, indices, batch, keep, buf, sink)
    host = table.cpu().numpy()
    res = score_slices(host, scores=scores, cases=cases, skip_no_organ_slices=skip_no_organ_slices)
    res["table"], res["n_prompts"] = host, stats
    if surf is not None:
        res["surface_table"] = surf.cpu().numpy()
        res["surface"] = score_surfaces(res["surface_table"], cases=cases)
    return res


def gather_counts(local, world):
    """One all-gather of the per-rank int64 counts tables [k, 12] -> [world*k, 12] (rank-major; `interleave_rank_major` puts the
    rows back in z order): 96 bytes per (slice, class) cross the link instead of an S*S mask."""
    if world == 1 or not dist.is_initialized():
        return local
    return all_gather_rows(local)


def gather_masks(local, world):
    """One all-gather of the per-rank uint8 masks (RCCL on GPUs, gloo on CPU). [k,S,S] -> [world*k,S,S] (rank-major)."""
    if world == 1 or not dist.is_initialized():
        return local
    return all_gather_rows(local)


def all_gather_rows(local):
    """dist.all_gather_into_tensor along dim 0. Device tensors go through RCCL as they are; under the gloo backend (the CPU tests, and
    the two-ranks-on-one-GPU test of the real pipeline, where RCCL refuses two ranks on one device) they are staged through the host."""
    world = dist.get_world_size()
    local = local.contiguous()
    if local.is_cuda and dist.get_backend() == "gloo":
        host = torch.empty((world * local.shape[0],) + tuple(local.shape[1:]), dtype=local.dtype)
        dist.all_gather_into_tensor(host, local.cpu())
        return host.to(local.device)
    full = torch.empty((world * local.shape[0],) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(full, local)
    return full


def interleave_rank_major(full, n_slices, world):
    """Undo the z = r (mod W) sharding: rank-major gathered masks -> z order (pads dropped)."""
    k = math.ceil(n_slices / world)
    idx = []
    for z in range(n_slices):
        idx.append((z % world) * k + z // world)
    return full[torch.tensor(idx, device=full.device)]
