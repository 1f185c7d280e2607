"""NumPy reference of the crops route's merge and cross-crop NMS (csrc/amg_crops.hip: psam_amg_keep_planes' merged table and
psam_amg_crops_nms' final table), the inputs the kernels are held to, and the comparison the GPU tests use.

The reference is the host code of SamAutomaticMaskGenerator._crops_host behind its per-crop stage: np.concatenate of the per-crop
records translated into the image's frame, then utils.amg.nms_xyxy with the float32 score 1 / crop area of every record's crop.
tests/test_amg_crops_cpu.py pins it against those lines, and shows that `same_final` tells every fault in FAULTS from it."""
import numpy as np

from protosam_amd.segment_anything.utils.amg import generate_crop_boxes, nms_xyxy

REC, CREC = 9, 11          # words of a psam_amg_select record / of a merged or final record (+ crop index, pool row)
FAULTS = ("dropped", "wrong_crop", "untranslated", "tie_order")


def crop_scores(crop_boxes):
    """float32 1 / crop area per crop, by the expression of `_crops_host`"""
    cb = np.asarray(crop_boxes, dtype=np.int64).reshape(-1, 4).astype(np.float32)
    return (1.0 / ((cb[:, 2] - cb[:, 0]) * (cb[:, 3] - cb[:, 1]))).astype(np.float32)


def merged_reference(per_crop, crop_boxes, fault=None):
    """per_crop: one int32 [k_c, REC] record table per crop, boxes in the crop's frame -> int32 [sum k_c, CREC]: the records of all
    crops in crop order, boxes in the image's frame, then the crop index and the row itself (the pool row)."""
    rows = []
    for c, (r, cb) in enumerate(zip(per_crop, crop_boxes)):
        r = np.asarray(r, dtype=np.int32).reshape(-1, REC)
        m = np.zeros((len(r), CREC), np.int32)
        m[:, :REC] = r
        if not (fault == "untranslated" and c >= 2):       # (crop 1 starts at the image's origin)
            m[:, 5:9] += np.array([[cb[0], cb[1], cb[0], cb[1]]], dtype=np.int32)
        m[:, REC] = c
        rows.append(m)
    out = np.concatenate(rows) if rows else np.zeros((0, CREC), np.int32)
    out[:, REC + 1] = np.arange(len(out))
    return out


def final_reference(per_crop, crop_boxes, thr, fault=None):
    """-> int32 [m, CREC]: the merged records that the cross-crop NMS keeps, in its order; with a single crop box no NMS runs
    (automatic_mask_generator.py:208). `fault`: one of FAULTS, a wrong implementation for the comparison to catch."""
    merged = merged_reference(per_crop, crop_boxes, fault)
    if len(crop_boxes) > 1:
        scores = crop_scores(crop_boxes)[merged[:, REC]]
        if fault == "tie_order":        # equal scores visited from the last row to the first
            order = np.argsort(-scores[::-1], kind="stable")
            keep = (len(merged) - 1 - order)[nms_xyxy(merged[::-1][order][:, 5:9].astype(np.int64), scores[::-1][order], thr)]
        else:
            keep = nms_xyxy(merged[:, 5:9].astype(np.int64), scores, thr)
        merged = merged[keep]
    if fault == "dropped" and len(merged):
        merged = np.delete(merged, len(merged) // 2, axis=0)
    if fault == "wrong_crop" and len(merged):
        merged = merged.copy()
        merged[0, REC] = (merged[0, REC] + 1) % max(len(crop_boxes), 2)
    return merged


def same_final(got, ref):
    """The comparison of the GPU tests: the final tables are equal word for word - count, order, candidate, plane, score bits,
    area, box in the image's frame, crop index and pool row."""
    got, ref = np.asarray(got).reshape(-1, CREC), np.asarray(ref).reshape(-1, CREC)
    assert len(got) == len(ref), f"{len(got)} final records, the reference has {len(ref)}"
    bad = np.flatnonzero((got != ref).any(1))
    assert len(bad) == 0, f"record {bad[0]}: {got[bad[0]].tolist()} != {ref[bad[0]].tolist()} ({len(bad)} records differ)"


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
IMAGE = (600, 800)     # crops of one layer: the image, then four 502 x 402 crops that all contain x 298 .. 502, y 198 .. 402


def layout(n_layers=1):
    return generate_crop_boxes(IMAGE, n_layers, 512 / 1500)[0]


def _records(rng, boxes_img, crop_box):
    """records of one crop from boxes given in the IMAGE's frame: random candidate, plane and score words"""
    k = len(boxes_img)
    r = np.zeros((k, REC), np.int32)
    r[:, 0] = rng.integers(0, 3000, k)
    r[:, 1] = (r[:, 0] // 3) * 4 + 1 + r[:, 0] % 3
    r[:, 2] = rng.random(k, dtype=np.float32).view(np.int32)
    r[:, 3] = rng.random(k, dtype=np.float32).view(np.int32)
    r[:, 4] = rng.integers(0, 5000, k)
    r[:, 5:9] = np.asarray(boxes_img, dtype=np.int64).reshape(k, 4) - np.array([[crop_box[0], crop_box[1]] * 2])
    return r


def _split(total, shares):
    """`total` records over the crops in proportion to `shares` (zeros stay zero)"""
    shares = np.asarray(shares, dtype=np.float64)
    k = np.floor(total * shares / shares.sum()).astype(np.int64)
    k[int(np.argmax(shares))] += total - k.sum()
    return k.tolist()


def case(kind, total, seed=0):
    """-> dict(per_crop, crop_boxes, thr): `total` records over the crops of `layout()`.
      clustered  : boxes of every crop jittered around 12 anchors in the region all crops share: most are suppressed, and the four
                   layer-1 crops have EQUAL scores (equal areas), so ties between crops and inside a crop decide the order
      exact      : pairs across crops whose IoU is exactly the threshold 1/2 (both stay), and one integer step to either side
      empty_crops: clustered, with crops 0, 2 and 4 empty - the first crop has zero survivors
      first_empty: clustered, only crop 0 empty
      single     : one crop box (crop_n_layers = 0): identical boxes, no NMS, every record stays
      identical_nms1: identical boxes in every crop at threshold 1.0: IoU == threshold, every record stays"""
    rng = np.random.default_rng(seed)
    boxes = layout()
    if kind == "single":
        boxes = boxes[:1]
        return dict(per_crop=[_records(rng, np.tile([[300, 200, 400, 300]], (total, 1)), boxes[0])], crop_boxes=boxes, thr=0.7)
    shares = {"clustered": [3, 1, 1, 1, 1], "exact": [1, 1, 0, 0, 0], "empty_crops": [0, 1, 0, 1, 0], "first_empty": [0, 2, 1, 1, 1],
              "identical_nms1": [1, 1, 1, 1, 1]}[kind]
    counts = _split(total, shares)
    per_crop = []
    if kind == "exact":
        units = [([300, 200, 320, 210], [300, 200, 310, 210]), ([340, 200, 360, 210], [340, 200, 351, 210]),
                 ([380, 200, 400, 210], [380, 200, 389, 210])]        # IoU 10/20 (stays), 11/20 (removed), 9/20 (stays)
        for c, k in enumerate(counts):
            j = np.arange(k)
            b = np.array([units[i % 3][1 if c == 0 else 0] for i in j], dtype=np.int64).reshape(k, 4)
            b[:, [1, 3]] += (j // 3 * 12)[:, None] % 190                # rows of non-overlapping triples (they repeat past 16 rows)
            per_crop.append(_records(rng, b, boxes[c]))
        return dict(per_crop=per_crop, crop_boxes=boxes, thr=0.5)
    anchors = np.array([[300 + 48 * (a % 4), 200 + 64 * (a // 4), 340 + 48 * (a % 4), 250 + 64 * (a // 4)] for a in range(12)])
    for c, k in enumerate(counts):
        if kind == "identical_nms1":
            b = np.tile([[310, 210, 400, 300]], (k, 1))
        else:
            b = anchors[rng.integers(0, 12, k)] + np.concatenate([rng.integers(0, 3, (k, 2)), rng.integers(0, 3, (k, 2))], 1)
        per_crop.append(_records(rng, b, boxes[c]))
    return dict(per_crop=per_crop, crop_boxes=boxes, thr=1.0 if kind == "identical_nms1" else 0.7)


KINDS = ("clustered", "exact", "empty_crops", "first_empty", "single", "identical_nms1")
# which inputs must tell each fault from the reference
SEPARATES = {"dropped": KINDS, "wrong_crop": KINDS, "untranslated": ("clustered", "empty_crops", "first_empty", "identical_nms1"),
             "tie_order": ("clustered", "first_empty", "empty_crops", "identical_nms1")}
