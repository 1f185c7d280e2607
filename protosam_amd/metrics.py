"""Per-slice overlap metrics of the caller (validation_protosam.py:169-185 `get_dice_iou_precision_recall`).

Evaluation bookkeeping on two [H, W] {0,1} maps, not a stage of the hot path: the reference computes it on the host
after `query_pred.cpu()` (validation_protosam.py:389,400). Same formulas, same 1e-8 guards, same all-background early
return (a dict WITHOUT the "iou" key, as the reference). Runs on whatever device the two tensors live on.
bench.py, __graft_entry__.smoke() and the parity tests use `dice` as the "Dice-equivalent" agreement measure.
"""
import numpy as np
import torch


def get_dice_iou_precision_recall(pred: torch.Tensor, gt: torch.Tensor):
    if gt.sum() == 0:
        print("gt is all background")
        return {"dice": 0, "precision": 0, "recall": 0}
    tp = (pred * gt).sum()
    fp = (pred * (1 - gt)).sum()
    fn = ((1 - pred) * gt).sum()
    dice = 2 * tp / (2 * tp + fp + fn + 1e-8)
    precision = tp / (tp + fp + 1e-8)
    recall = tp / (tp + fn + 1e-8)
    iou = tp / (tp + fp + fn + 1e-8)
    return {"dice": dice, "iou": iou, "precision": precision, "recall": recall}


def dice(pred, gt):
    """float Dice of two {0,1} maps (1.0 when both are empty: identical masks agree)."""
    pred, gt = torch.as_tensor(pred).float(), torch.as_tensor(gt).float()
    if gt.sum() == 0:
        return 1.0 if pred.sum() == 0 else 0.0
    return float(get_dice_iou_precision_recall(pred, gt)["dice"])


# ---- scoring from the counts table of ops.seg_counts ------------------------------------------------------------------------------
# Everything below works on integer counts {tp, fp, fn, tn} and boxes that psam_seg_counts left in an int64 [n, 12] table
# (ops.SEG_COLS); only `Metric.record` / `record_batch` touch the device, and they only enqueue.

TP, FP, FN, TN = 0, 1, 2, 3
_PRED_BOX, _GT_BOX = slice(4, 8), slice(8, 12)


def class_rows(n, classes=None, label_planes=None, pred_value=1, label_value=1):
    """The row table of ops.seg_counts for n slices -> int32 array [rows, 4] of (pred plane, pred value, label plane, label value).
    classes = [organ ids]: masks [n, C, H, W] against a label map, row k*C + c = (k*C + c, pred_value, label plane of slice k,
    classes[c]). classes = None: the one-class form for masks [n, H, W], row k = (k, pred_value, label plane of slice k, label_value).
    label_planes: the label plane of every slice (default k: a label map [n, H, W]; a list of z for a whole label volume)."""
    lp = list(range(n)) if label_planes is None else [int(z) for z in label_planes]
    if len(lp) != n:
        raise ValueError(f"label_planes has {len(lp)} entries for {n} slices")
    if classes is None:
        return np.array([(k, pred_value, lp[k], label_value) for k in range(n)], dtype=np.int32).reshape(-1, 4)
    C = len(classes)
    return np.array([(k * C + c, pred_value, lp[k], int(classes[c])) for k in range(n) for c in range(C)],
                    dtype=np.int32).reshape(-1, 4)


def _host_table(counts):
    if isinstance(counts, torch.Tensor):
        counts = counts.detach().cpu().numpy()
    return np.asarray(counts)


def box_xywh(x0, y0, x1, y1):
    """Inclusive extremes -> cv2.boundingRect's (x, y, w, h): w = x1 - x0 + 1, h = y1 - y0 + 1, and (0, 0, 0, 0) for an empty map
    (x1 < x0). cv2 is not a dependency: restated from boundingRect's definition for a mask (the up-right rectangle of the
    non-zero pixels), which validation_protosam.py:49-62 applies to the uint8 map."""
    if x1 < x0:
        return (0, 0, 0, 0)
    return (int(x0), int(y0), int(x1 - x0 + 1), int(y1 - y0 + 1))


def calc_iou(boxA, boxB):
    """IoU of two (x, y, w, h) boxes as validation_protosam.py:64-80 (continuous extents, no +1; 0/0 raises as there)."""
    ax0, ay0, ax1, ay1 = boxA[0], boxA[1], boxA[0] + boxA[2], boxA[1] + boxA[3]
    bx0, by0, bx1, by1 = boxB[0], boxB[1], boxB[0] + boxB[2], boxB[1] + boxB[3]
    inter = max(0, min(ax1, bx1) - max(ax0, bx0)) * max(0, min(ay1, by1) - max(ay0, by0))
    return inter / float(boxA[2] * boxA[3] + boxB[2] * boxB[3] - inter)


def eval_detection(pred_list, as_frame=None):
    """validation_protosam.py:81-122: the detection table of a list of {"pred_bbox", "gt_bbox", "score"} with (x, y, w, h) boxes (as
    `score_slices` returns under "bboxes_w_scores"). Per IoU threshold of np.round(np.arange(0.5, 1.0, 0.05), 2): a prediction is a
    true positive when calc_iou(pred_bbox, gt_bbox) >= threshold, else a false positive; precision = tp / (tp + fp), recall =
    tp / len(pred_list), f1 = 2 p r / (p + r) - nan where that expression is 0 / 0 (no true positive; the reference's Python floats raise there, and the rows
    of the other thresholds are still wanted).
    An empty list divides by zero and two empty boxes make calc_iou divide by zero, as in the reference: both raise.
    -> a pandas DataFrame (the reference's return) where pandas imports, else the list of row dicts; as_frame=False / True forces
    either."""
    rows = []
    for thr in np.round(np.arange(0.5, 1.0, 0.05), 2):
        tp = sum(1 for p in pred_list if calc_iou(p["pred_bbox"], p["gt_bbox"]) >= thr)
        fp = len(pred_list) - tp
        precision = tp / (tp + fp)
        recall = tp / len(pred_list)
        f1 = 2 * (precision * recall) / (precision + recall) if precision + recall > 0 else float("nan")
        rows.append({"iou_threshold": thr, "tp": tp, "fp": fp, "n_gt": len(pred_list), "f1": f1, "precision": precision,
                     "recall": recall})
    if as_frame is False:
        return rows
    try:
        import pandas as pd
    except ImportError:
        if as_frame:
            raise
        return rows
    return pd.DataFrame(rows)


def score_slices(counts, scores=None, cases=None, skip_no_organ_slices=True):
    """The numbers of the per-slice loop of validation_protosam.py:369-448 from a counts table [n, 12] (host side, float64).
    Per row dice / iou / precision / recall with the 1e-8 guards (:169-185). A row whose ground truth is empty (tp + fn == 0) is
    left out when skip_no_organ_slices (:369-370); otherwise KeyError naming the row, as the reference's loop fails there (its
    early-return dict has no "iou", :174-176,405).
    scores: per row the confidences of its prompt sets (their mean is the box score, :409); cases: per row the case it belongs to.
    -> dict: rows (indices kept), dice / iou / precision / recall (arrays over them), mean_dice / mean_precision / mean_recall /
    mean_iou (:436-439), dice_cases / iou_cases {case: mean} (:411-415,429-433), bboxes_w_scores [{pred_bbox, gt_bbox, score}]
    with boxes (x, y, w, h) as `box_xywh` (:407-409)."""
    t = _host_table(counts).astype(np.int64)
    kept, per = [], {"dice": [], "iou": [], "precision": [], "recall": []}
    boxes, by_case = [], {}
    for k in range(t.shape[0]):
        tp, fp, fn = (float(v) for v in t[k, :3])
        if tp + fn == 0:
            if skip_no_organ_slices:
                continue
            raise KeyError(f"iou (row {k}: the ground truth is all background, and the reference's dict then has no 'iou')")
        d = {"dice": 2 * tp / (2 * tp + fp + fn + 1e-8), "precision": tp / (tp + fp + 1e-8), "recall": tp / (tp + fn + 1e-8),
             "iou": tp / (tp + fp + fn + 1e-8)}
        kept.append(k)
        for name in per:
            per[name].append(d[name])
        boxes.append({"pred_bbox": box_xywh(*t[k, _PRED_BOX]), "gt_bbox": box_xywh(*t[k, _GT_BOX]),
                      "score": None if scores is None else float(np.mean(scores[k]))})
        if cases is not None:
            by_case.setdefault(cases[k], ([], []))
            by_case[cases[k]][0].append(d["dice"])
            by_case[cases[k]][1].append(d["iou"])
    out = {"rows": kept, "bboxes_w_scores": boxes}
    for name in per:
        out[name] = np.array(per[name], dtype=np.float64)
        out["mean_" + name] = float(np.mean(out[name])) if kept else float("nan")
    out["dice_cases"] = {c: float(np.mean(v[0])) for c, v in by_case.items()}
    out["iou_cases"] = {c: float(np.mean(v[1])) for c, v in by_case.items()}
    return out


class Metric:
    """util/metric.py's `Metric` (same constructor, methods, arguments and return tuples) on counts that psam_seg_counts leaves on
    the device: `record` / `record_batch` enqueue one launch and return; the tables come to the host in ONE copy at the first
    `get_*` (or `reset_scan`). `record_table` is the host half: it takes the counts of one `record` call as an array, so the
    bookkeeping and every `get_*` run without a device.
    Kept as the reference behaves, including what looks like a slip there (util/metric.py:72-98): with labels=[lb, ...] the loop
    compares pred == j and target == j for the POSITION j in [0, lb, ...] (0 and 1 for one label: binary maps, as
    validation.py:304 passes them) and stores under index 0 and lb; with labels=None position and label coincide. Labels that a
    call does not record stay NaN in its entry and are skipped by the nansums; a class with tp + fp + fn == 0 gives NaN (0/0).
    The one difference: get_mDice does not print."""

    def __init__(self, max_label=20, n_scans=None):
        self.labels = list(range(max_label + 1))
        self.n_scans = 1 if n_scans is None else n_scans
        self.slice_counter = [0 for _ in range(self.n_scans)]
        self._clear()

    def _clear(self):
        self.tp_lst = [[] for _ in range(self.n_scans)]
        self.fp_lst = [[] for _ in range(self.n_scans)]
        self.fn_lst = [[] for _ in range(self.n_scans)]
        self._pending = []          # (device table, [(scan, entry, label index, table row, background_from_tn)])

    def reset(self):
        self._clear()

    def reset_scan(self, n_scan, labels=None):
        self._flush()
        labels = self.labels if labels is None else labels
        for lst in (self.tp_lst, self.fp_lst, self.fn_lst):
            for entry in lst[n_scan]:
                for lb in labels:
                    entry[lb] = np.nan

    # ---- recording -------------------------------------------------------------------------------------------------------------
    def _positions(self, labels):
        """[(value compared in both maps, index stored under)] of one `record` call"""
        return list(enumerate(self.labels if labels is None else [0] + list(labels)))

    def _new_entry(self, n_scan):
        if self.n_scans == 1:
            n_scan = 0
        for lst in (self.tp_lst, self.fp_lst, self.fn_lst):
            lst[n_scan].append(np.full(len(self.labels), np.nan))
        self.slice_counter[n_scan] += 1
        return n_scan, len(self.tp_lst[n_scan]) - 1

    def _store(self, scan, entry, idx, tp, fp, fn):
        self.tp_lst[scan][entry][idx] = tp
        self.fp_lst[scan][entry][idx] = fp
        self.fn_lst[scan][entry][idx] = fn

    def record_rows(self, labels=None, pred_plane=0, label_plane=0):
        """the seg_counts rows of one `record(pred, target, labels)` call: (pred_plane, j, label_plane, j) per position j"""
        return np.array([(pred_plane, j, label_plane, j) for j, _ in self._positions(labels)], dtype=np.int32).reshape(-1, 4)

    def record_table(self, table, labels=None, n_scan=None):
        """Host half of `record`: table [len(record_rows(labels)), >= 3] holds {tp, fp, fn} of those rows, in their order."""
        t = _host_table(table)
        pos = self._positions(labels)
        assert t.shape[0] == len(pos), (t.shape, len(pos))
        scan, entry = self._new_entry(n_scan)
        for r, (_, idx) in enumerate(pos):
            self._store(scan, entry, idx, t[r, TP], t[r, FP], t[r, FN])

    def record(self, pred, target, labels=None, n_scan=None):
        """pred, target: device tensors [H, W] (label maps, or binary maps with labels=[lb]). One launch, no synchronise."""
        assert pred.shape == target.shape
        self.record_batch(pred[None], target[None], labels, n_scan)

    def record_batch(self, preds, targets, labels=None, n_scan=None):
        """Many slices in one launch. n_scan: one scan for all, or one per slice.
        preds [n, H, W], targets [n, H, W]: the loop `record(preds[k], targets[k], labels, n_scan)`.
        preds [n, C, H, W] {0, 1} masks, targets [n, H, W] label map, labels = the C organ ids: the loop over k, c of
        `record(preds[k, c], targets[k] == labels[c], labels=[labels[c]], n_scan)` as validation.py:304 calls it per organ - ONE
        row per (slice, class): with binary maps the background's {tp, fp, fn} are the organ's {tn, fn, fp}."""
        from . import ops
        n = preds.shape[0]
        scans = list(n_scan) if isinstance(n_scan, (list, tuple)) else [n_scan] * n
        assert len(scans) == n and tuple(preds.shape[-2:]) == tuple(targets.shape[-2:]) and targets.shape[0] == n
        fill = []
        if preds.dim() == 4:
            C = preds.shape[1]
            assert targets.dim() == 3 and labels is not None and len(labels) == C
            rows = class_rows(n, labels)
            for k in range(n):
                for c in range(C):
                    scan, entry = self._new_entry(scans[k])
                    fill.append((scan, entry, 0, k * C + c, True))
                    fill.append((scan, entry, int(labels[c]), k * C + c, False))      # (after index 0: the later store wins)
        else:
            assert preds.dim() == 3 and targets.dim() == 3
            pos = self._positions(labels)
            rows = np.concatenate([self.record_rows(labels, k, k) for k in range(n)])
            for k in range(n):
                scan, entry = self._new_entry(scans[k])
                fill += [(scan, entry, idx, k * len(pos) + r, False) for r, (_, idx) in enumerate(pos)]
        self._pending.append((ops.seg_counts(preds, targets, rows.tolist()), fill))

    def _flush(self):
        if not self._pending:
            return
        tables = [t for t, _ in self._pending]
        host = (tables[0] if len(tables) == 1 else torch.cat(tables)).cpu().numpy()          # the one copy (it synchronises)
        base = 0
        for t, fill in self._pending:
            for scan, entry, idx, r, from_tn in fill:
                row = host[base + r]
                if from_tn:
                    self._store(scan, entry, idx, row[TN], row[FN], row[FP])
                else:
                    self._store(scan, entry, idx, row[TP], row[FP], row[FN])
            base += t.shape[0]
        self._pending = []

    # ---- results ---------------------------------------------------------------------------------------------------------------
    def _sums(self, scan):
        """nansum over the slices of one scan -> tp, fp, fn over all label indices (ValueError for a scan without slices)"""
        return tuple(np.nansum(np.vstack(lst[scan]), axis=0) for lst in (self.tp_lst, self.fp_lst, self.fn_lst))

    def _per_scan(self, fn, n_scan):
        """fn(tp, fp, fn) per scan: stacked [n_scans, ...] for n_scan None, else that scan's alone"""
        self._flush()
        if n_scan is None:
            return np.vstack([fn(*self._sums(s)) for s in range(self.n_scans)])
        return fn(*self._sums(n_scan))

    @staticmethod
    def _spread(cls):
        m = cls.mean(axis=1)
        return cls.mean(axis=0), cls.std(axis=0), m.mean(axis=0), m.std(axis=0)

    def get_mIoU(self, labels=None, n_scan=None):
        labels = self.labels if labels is None else labels
        cls = self._per_scan(lambda tp, fp, fn: tp.take(labels) / (tp.take(labels) + fp.take(labels) + fn.take(labels)), n_scan)
        return self._spread(cls) if n_scan is None else (cls, cls.mean())

    def get_mDice(self, labels=None, n_scan=None, give_raw=False):
        labels = self.labels if labels is None else labels
        cls = self._per_scan(lambda tp, fp, fn: 2 * tp.take(labels) / (2 * tp.take(labels) + fp.take(labels) + fn.take(labels)),
                             n_scan)
        if n_scan is not None:
            return cls, cls.mean(), cls
        return self._spread(cls) + ((cls,) if give_raw else ())

    def get_mPrecRecall(self, labels=None, n_scan=None, give_raw=False):
        labels = self.labels if labels is None else labels
        prec = self._per_scan(lambda tp, fp, fn: tp.take(labels) / (tp.take(labels) + fp.take(labels)), n_scan)
        rec = self._per_scan(lambda tp, fp, fn: tp.take(labels) / (tp.take(labels) + fn.take(labels)), n_scan)
        if n_scan is not None:
            return prec, None, prec.mean(), None, rec, None, rec.mean(), None, prec, rec
        return self._spread(prec) + self._spread(rec) + ((prec, rec) if give_raw else ())

    def get_mIoU_binary(self, n_scan=None):
        """background and the sum of all foreground classes as two classes"""
        def two(v):
            return np.c_[v[0], np.nansum(v[1:])]

        cls = self._per_scan(lambda tp, fp, fn: two(tp) / (two(tp) + two(fp) + two(fn)), n_scan)
        return self._spread(cls) if n_scan is None else (cls, cls.mean())


# ---- boundary measures from the table of ops.surface_distances ----------------------------------------------------------------------
# HD, HD95 and ASSD as MedPy's hd / hd95 / asd / assd with connectivity=1 define them (restated in ops.surface_points /
# surface_dist / surface_stats and DESIGN.md section 4b): surfaces by face neighbours with the array's edge as background,
# Euclidean distances with voxel spacing, hd the larger directed maximum, hd95 numpy.percentile(., 95) of both directed sets
# together, assd the mean of the two directed means; NaN, with the counts saying which side, where a surface is empty.

N_PRED, N_GT, HD, HD95, ASSD, ASD_PG, ASD_GP, SURF_STATUS = range(8)


def surface_rows(n, classes=None, label_planes=None, depth=1, pred_value=1, label_value=1):
    """The row table of ops.surface_distances -> int32 array [rows, 5] of (first pred plane, pred value, first label plane, label
    value, depth). It mirrors `class_rows`.
    depth = 1, n slices: classes = [organ ids]: masks [n, C, H, W] against a label map, row k*C + c = (k*C + c, pred_value, label
    plane of slice k, classes[c], 1); classes = None: masks [n, H, W], row k = (k, pred_value, label plane of slice k, label_value,
    1). label_planes as in class_rows.
    depth = D > 1, n volumes of D consecutive planes each (a scan): classes = [organ ids]: masks [n * C, D, H, W] (class-major
    volumes), row k*C + c = ((k*C + c) * D, pred_value, first label plane of volume k, classes[c], D); classes = None: row k =
    (k * D, pred_value, first label plane of volume k, label_value, D). label_planes: the FIRST label plane of every volume
    (default k * D)."""
    D = int(depth)
    if D < 1:
        raise ValueError(f"depth must be at least 1, got {depth}")
    lp = [k * D for k in range(n)] if label_planes is None else [int(z) for z in label_planes]
    if len(lp) != n:
        raise ValueError(f"label_planes has {len(lp)} entries for {n} slices")
    if classes is None:
        return np.array([(k * D, pred_value, lp[k], label_value, D) for k in range(n)], dtype=np.int32).reshape(-1, 5)
    C = len(classes)
    return np.array([((k * C + c) * D, pred_value, lp[k], int(classes[c]), D) for k in range(n) for c in range(C)],
                    dtype=np.int32).reshape(-1, 5)


def score_surfaces(table, cases=None):
    """Host half of the boundary measures (float64, no device): table [n, 8] as ops.surface_distances leaves it (ops.SURF_COLS).
    A row counts when both of its surfaces are present and it was filled (status 0). -> dict: rows (indices that count), hd /
    hd95 / assd / asd_pg / asd_gp (arrays over them), mean_hd / mean_hd95 / mean_assd (NaN without rows), n_pred / n_gt (surface
    sizes of ALL rows), and the rows left out, each under a key of its own: empty_pred, empty_gt (a row with both surfaces empty
    is in both), overflowed (status 1: the pool was too small, see `surface_table`), bad_rows (status 2). cases: per row the case
    it belongs to -> hd95_cases / assd_cases {case: mean over its counted rows}."""
    t = np.asarray(_host_table(table), dtype=np.float64).reshape(-1, 8)
    status = t[:, SURF_STATUS].astype(np.int64)
    n_pred, n_gt = t[:, N_PRED].astype(np.int64), t[:, N_GT].astype(np.int64)
    ok = status == 0
    kept = [int(k) for k in np.nonzero(ok & (n_pred > 0) & (n_gt > 0))[0]]
    out = {"rows": kept, "n_pred": n_pred, "n_gt": n_gt,
           "empty_pred": [int(k) for k in np.nonzero(ok & (n_pred == 0))[0]],
           "empty_gt": [int(k) for k in np.nonzero(ok & (n_gt == 0))[0]],
           "overflowed": [int(k) for k in np.nonzero(status == 1)[0]],
           "bad_rows": [int(k) for k in np.nonzero(status > 1)[0]]}
    for name, col in (("hd", HD), ("hd95", HD95), ("assd", ASSD), ("asd_pg", ASD_PG), ("asd_gp", ASD_GP)):
        out[name] = t[kept, col] if kept else np.zeros(0, dtype=np.float64)
    for name in ("hd", "hd95", "assd"):
        out["mean_" + name] = float(np.mean(out[name])) if kept else float("nan")
    by_case = {}
    if cases is not None:
        for i, k in enumerate(kept):
            by_case.setdefault(cases[k], ([], []))
            by_case[cases[k]][0].append(out["hd95"][i])
            by_case[cases[k]][1].append(out["assd"][i])
    out["hd95_cases"] = {c: float(np.mean(v[0])) for c, v in by_case.items()}
    out["assd_cases"] = {c: float(np.mean(v[1])) for c, v in by_case.items()}
    return out


def surface_table(pred, label, rows, spacing=(1.0, 1.0, 1.0), cap=None, table=None):
    """The complete host table [n, 8] of ops.surface_distances(pred, label, rows, spacing, cap): rows flagged as overflowed
    (status 1) are computed again, only they, in one further call whose capacity is the sum of their true surface sizes (which
    the first pass counted whatever its cap), so every row is as an un-overflowed run gives it, bit for bit. table: a table
    already computed for these arguments (device or host) - then only the flagged rows run. rows: a list / array [n, 5]. It
    synchronises (one copy per pass)."""
    from . import ops
    r = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
    host = np.array(_host_table(ops.surface_distances(pred, label, r.tolist(), spacing, cap=cap) if table is None else table),
                    dtype=np.float64).reshape(-1, 8)
    if host.shape[0] != r.shape[0]:
        raise ValueError(f"table has {host.shape[0]} rows for {r.shape[0]} rows")
    again = np.nonzero(host[:, SURF_STATUS] == 1)[0]
    if again.size:
        need = int(host[again, N_PRED].sum() + host[again, N_GT].sum())
        host[again] = _host_table(ops.surface_distances(pred, label, r[again].tolist(), spacing, cap=max(need, 1)))
        assert (host[again, SURF_STATUS] == 0).all()
    return host
