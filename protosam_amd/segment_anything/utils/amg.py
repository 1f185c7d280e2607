"""Host-side helpers of the automatic mask generator (names of models/segment_anything/utils/amg.py).

Only the pieces that remain on the host once the per-candidate reductions run on the GPU (`psam_mask_stats`): the point
grids (:179-199), crop boxes of layer 0 (:202-237), XYXY->XYWH (:92-96), the uncompressed column-major RLE
(:108-153) and box NMS. The RLE also exists on the device (`mask_to_rle_pytorch`, `rle_to_mask_device` over `psam_rle_*`; the
host `mask_to_rle` / `rle_to_mask` stay as the reference the tests compare them with), and `coco_encode_rle` /
`coco_decode_rle` (:294-300) restate the COCO API's published string form, so no pycocotools is needed for it. `torchvision.ops.batched_nms` (a dependency absent from /root/reference; all categories are 0 in
the generator, so it is plain NMS) is restated from its published contract: visit boxes by decreasing score (stable),
drop every later box whose IoU with a kept box exceeds the threshold, areas = (x2-x1)*(y2-y1) in fp32.
"""
import numpy as np


def build_point_grid(n_per_side):
    """n x n points at the cell centres of the unit square, x fastest. [n*n, 2] float64 (x, y)."""
    half = 1 / (2 * n_per_side)
    side = np.linspace(half, 1 - half, n_per_side)
    xs, ys = np.meshgrid(side, side)
    return np.stack([xs, ys], axis=-1).reshape(-1, 2)


def build_all_layer_point_grids(n_per_side, n_layers, scale_per_layer):
    return [build_point_grid(int(n_per_side / (scale_per_layer ** i))) for i in range(n_layers + 1)]


def box_xyxy_to_xywh(box):
    b = np.array(box, copy=True)
    b[2] -= b[0]
    b[3] -= b[1]
    return b


def batch_iterator(batch_size, *args):
    n = len(args[0])
    assert all(len(a) == n for a in args), "Batched iteration must have inputs of all the same size."
    for lo in range(0, n, batch_size):
        yield [a[lo:lo + batch_size] for a in args]


def mask_to_rle(mask):
    """bool [H, W] -> {"size": [H, W], "counts": [...]}: run lengths in column-major (Fortran) order, starting with
    the number of leading zeros (0 if the first pixel is set) - the pycocotools uncompressed format."""
    h, w = mask.shape
    flat = np.asarray(mask, dtype=bool).T.reshape(-1)
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    edges = np.concatenate([[0], change, [h * w]])
    counts = np.diff(edges).tolist()
    if flat.size and flat[0]:
        counts = [0] + counts
    return {"size": [h, w], "counts": counts}


def rle_to_mask(rle):
    h, w = rle["size"]
    counts = np.asarray(rle["counts"], dtype=np.int64)
    vals = (np.arange(len(counts)) & 1).astype(bool)
    return np.repeat(vals, counts).reshape(w, h).T


def area_from_rle(rle):
    return sum(rle["counts"][1::2])


def mask_to_rle_pytorch(tensor):
    """utils/amg.py:107-135 on the HIP codec: device bool / uint8 [b, h, w] -> list of {"size": [h, w], "counts": [ints]}, equal
    to `mask_to_rle` of every mask. The masks stay on the device (`ops.rle_encode`); one download of the run lengths and
    their offsets serves the whole batch."""
    import torch
    from ... import ops
    if tensor.dim() != 3:
        raise ValueError(f"expected [b, h, w], got {tuple(tensor.shape)}")
    b, h, w = tensor.shape
    counts, offsets = ops.rle_encode(tensor)
    packed = torch.cat([offsets, counts.to(torch.int64)]).cpu().numpy()
    off, cnt = packed[:b + 1], packed[b + 1:]
    return [{"size": [h, w], "counts": cnt[off[i]:off[i + 1]].tolist()} for i in range(b)]


def rle_to_mask_device(rles, device):
    """utils/amg.py:138-149 for a list of uncompressed RLEs of one size -> uint8 {0, 1} [n, h, w] on `device`
    (`ops.rle_decode`). Every list is checked on the host first: a negative count, or counts that do not sum to h * w,
    raise ValueError before anything is uploaded."""
    import torch
    from ... import ops
    if len(rles) == 0:
        raise ValueError("rle_to_mask_device needs at least one RLE (the size comes from it)")
    h, w = (int(v) for v in rles[0]["size"])
    if h <= 0 or w <= 0:
        raise ValueError(f"bad size {rles[0]['size']}")
    lists = []
    for i, r in enumerate(rles):
        if [int(v) for v in r["size"]] != [h, w]:
            raise ValueError(f"rle {i}: size {r['size']} differs from {[h, w]}")
        c = np.asarray(r["counts"], dtype=np.int64).reshape(-1)
        if c.size and int(c.min()) < 0:
            raise ValueError(f"rle {i}: negative count")
        if int(c.sum()) != h * w:
            raise ValueError(f"rle {i}: counts sum to {int(c.sum())}, not {h} * {w}")
        lists.append(c)
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int64)
    counts = np.concatenate(lists).astype(np.int32)
    return ops.rle_decode(torch.from_numpy(counts).to(device), torch.from_numpy(offsets).to(device), h, w)


def coco_encode_rle(uncompressed_rle):
    """utils/amg.py:294-300 without pycocotools: {"size", "counts": [ints]} -> {"size", "counts": str}, the COCO API's
    compressed string (`rleToString`): each count from the third on is stored as its difference from the count two places
    back, then written 5 bits at a time, low bits first, as chr(48 + bits) with 0x20 marking "more follows" (the sign is
    carried by bit 0x10 of the last group)."""
    cnts = [int(v) for v in uncompressed_rle["counts"]]
    out = []
    for i, x in enumerate(cnts):
        if i > 2:
            x -= cnts[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    h, w = uncompressed_rle["size"]
    return {"size": [h, w], "counts": "".join(out)}


def coco_decode_rle(rle):
    """The inverse of `coco_encode_rle` (the COCO API's `rleFrString`): {"size", "counts": str or bytes} -> uncompressed."""
    s = rle["counts"]
    if isinstance(s, str):
        s = s.encode("ascii")
    cnts = []
    p = 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            if p >= len(s):
                raise ValueError("truncated COCO RLE string")
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    h, w = rle["size"]
    return {"size": [h, w], "counts": cnts}


def nms_xyxy(boxes, scores, iou_threshold):
    """-> indices kept, by decreasing score. boxes [n,4] (x0,y0,x1,y1), scores [n]."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    order = np.argsort(-np.asarray(scores, dtype=np.float32), kind="stable")
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    dead = np.zeros(len(b), bool)
    keep = []
    for pos, i in enumerate(order):
        if dead[i]:
            continue
        keep.append(int(i))
        rest = order[pos + 1:]
        rest = rest[~dead[rest]]
        if rest.size == 0:
            continue
        iw = np.maximum(np.float32(0), np.minimum(b[i, 2], b[rest, 2]) - np.maximum(b[i, 0], b[rest, 0]))
        ih = np.maximum(np.float32(0), np.minimum(b[i, 3], b[rest, 3]) - np.maximum(b[i, 1], b[rest, 1]))
        inter = iw * ih
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = inter / (area[i] + area[rest] - inter)
        dead[rest[iou.astype(np.float64) > iou_threshold]] = True
    return np.asarray(keep, dtype=np.int64)


def generate_crop_boxes(im_size, n_layers, overlap_ratio):
    """utils/amg.py:202-237: the image box, then (2**i)**2 overlapping crops for layer i. -> (boxes XYXY, layer per box)."""
    import math
    from itertools import product
    boxes, layers = [], []
    im_h, im_w = im_size
    short = min(im_h, im_w)
    boxes.append([0, 0, im_w, im_h])
    layers.append(0)
    for i_layer in range(n_layers):
        n = 2 ** (i_layer + 1)
        overlap = int(overlap_ratio * short * (2 / n))
        cw = int(math.ceil((overlap * (n - 1) + im_w) / n))
        ch = int(math.ceil((overlap * (n - 1) + im_h) / n))
        xs = [int((cw - overlap) * i) for i in range(n)]
        ys = [int((ch - overlap) * i) for i in range(n)]
        for x0, y0 in product(xs, ys):
            boxes.append([x0, y0, min(x0 + cw, im_w), min(y0 + ch, im_h)])
            layers.append(i_layer + 1)
    return boxes, layers


def is_box_near_crop_edge(boxes, crop_box, orig_box, atol=20.0):
    """utils/amg.py:78-88: a box edge within `atol` of the crop's edge but not of the image's. boxes int [n,4] in the crop's
    frame -> bool [n]. (torch.isclose with rtol = 0 is |a - b| <= atol.)"""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4) + np.array([[crop_box[0], crop_box[1], crop_box[0], crop_box[1]]],
                                                                      dtype=np.float32)
    near_crop = np.abs(b - np.asarray(crop_box, dtype=np.float32)[None, :]) <= atol
    near_img = np.abs(b - np.asarray(orig_box, dtype=np.float32)[None, :]) <= atol
    return np.any(near_crop & ~near_img, axis=1)
