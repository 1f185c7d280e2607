"""Reference for psam_box_nms / psam_amg_select (csrc/nms.hip) and the tables the CPU and GPU tests share.

The reference is the host code the device path replaces, run as it stands: `select_lines` restates the filter lines of
SamAutomaticMaskGenerator._select_host (automatic_mask_generator.py) in numpy and calls `utils.amg.nms_xyxy` itself (pinned in
tests/test_amg_cpu.py). `fault=` swaps in one deliberately wrong variant; tests/test_amg_select_cpu.py shows that the tables below
tell every such variant from the reference, so a device kernel with that mistake cannot pass the GPU tests on them.

A table is a dict: boxes int32 [n,4], scores fp32 [n] (the predicted IoUs), hi / lo / area int32 [n] (columns 0..2 of the
statistics table), thr = (pred_iou_thresh, stability_score_thresh, box_nms_thresh).
"""
import numpy as np

from protosam_amd.segment_anything.utils.amg import nms_xyxy

REC = 9
FAULTS = ("ge", "no_f64", "unstable", "no_empty_rule", "stab_f64", "dead_suppresses")
INT_MAX = 2 ** 31 - 1


# ---- the reference -------------------------------------------------------------------------------------------------------------
def nms_faulty(boxes, scores, iou_threshold, fault):
    """utils.amg.nms_xyxy with one injected fault (the loop restated; fault None must equal nms_xyxy - the CPU test checks it)."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    s = -np.asarray(scores, dtype=np.float32)
    order = np.argsort(s, kind="stable")
    if fault == "unstable":                                   # equal scores in descending index order
        order = np.lexsort((-np.arange(len(s)), s))
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    dead = np.zeros(len(b), bool)
    keep = []
    for pos, i in enumerate(order):
        if dead[i]:
            if fault != "dead_suppresses":
                continue
        else:
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
        if fault == "no_f64":
            over = iou > np.float32(iou_threshold)
        elif fault == "ge":
            over = iou.astype(np.float64) >= iou_threshold
        else:
            over = iou.astype(np.float64) > iou_threshold
        dead[rest[over]] = True
    return np.asarray(keep, dtype=np.int64)


def _nms(fault):
    if fault in ("ge", "no_f64", "unstable", "dead_suppresses"):
        return lambda b, s, t: nms_faulty(b, s, t, fault)
    return nms_xyxy


def select_lines(stats, iou, pred_iou_thresh, stability_score_thresh, box_nms_thresh, fault=None):
    """The host lines of SamAutomaticMaskGenerator._select_host on one group: stats int32 [m,8], iou fp32 [m] (flatten(0, 1) of
    the decoder's columns 1..3) -> int32 [k, 9] records {candidate, plane, IoU bits, stability bits, area, box} in NMS order."""
    stats = np.asarray(stats, dtype=np.int32).reshape(-1, 8)
    iou = np.asarray(iou, dtype=np.float32)
    keep = np.arange(len(stats))
    if pred_iou_thresh > 0.0:
        keep = keep[iou[keep] > pred_iou_thresh]
    with np.errstate(divide="ignore", invalid="ignore"):
        stab = stats[:, 0].astype(np.float32) / stats[:, 1].astype(np.float32)
    if stability_score_thresh > 0.0:
        if fault == "stab_f64":
            keep = keep[stab[keep].astype(np.float64) >= np.float64(stability_score_thresh)]
        else:
            keep = keep[stab[keep] >= stability_score_thresh]
    boxes = stats[:, 3:7].astype(np.int64)
    if fault != "no_empty_rule":
        boxes[stats[:, 2] == 0] = 0
    kept = keep[_nms(fault)(boxes[keep], iou[keep], box_nms_thresh)]
    plane = (kept // 3) * 4 + 1 + kept % 3
    rec = np.zeros((len(kept), REC), np.int32)
    rec[:, 0], rec[:, 1] = kept, plane
    rec[:, 2], rec[:, 3] = iou[kept].view(np.int32), stab[kept].view(np.int32)
    rec[:, 4] = stats[kept, 2]
    rec[:, 5:9] = boxes[kept]
    return rec


def select_groups(stats, iou4, offsets, thr, fault=None):
    """select_lines per group of rows offsets[g]:offsets[g+1]; candidate and plane count from the table's first row."""
    n = len(stats)
    iou = np.asarray(iou4, dtype=np.float32)[:, 1:].reshape(-1)[:n]
    out = []
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        rec = select_lines(stats[lo:hi], iou[lo:hi], *thr, fault=fault)
        c = rec[:, 0].astype(np.int64) + lo
        rec[:, 0], rec[:, 1] = c, (c // 3) * 4 + 1 + c % 3
        out.append(rec)
    return out


def nms_groups(boxes, scores, offsets, thr, fault=None):
    return [_nms(fault)(boxes[lo:hi], scores[lo:hi], thr) for lo, hi in zip(offsets[:-1], offsets[1:])]


# ---- tables --------------------------------------------------------------------------------------------------------------------
def make_stats(t):
    """-> (stats int32 [n,8] as psam_mask_stats writes it, iou4 fp32 [ceil(n/3),4] as the decoder writes it; column 0, the
    single-mask output, holds a value that would win every comparison if it were read)."""
    n = len(t["scores"])
    stats = np.zeros((n, 8), np.int32)
    stats[:, 0], stats[:, 1], stats[:, 2] = t["hi"], t["lo"], t["area"]
    stats[:, 3:7] = t["boxes"]
    stats[:, 7] = 0
    flat = np.full(3 * ((n + 2) // 3), -7.0, np.float32)
    flat[:n] = t["scores"]
    iou4 = np.full(((n + 2) // 3, 4), 9.0, np.float32)
    iou4[:, 1:] = flat.reshape(-1, 3)
    return stats, iou4


def _table(boxes, scores, thr, hi=None, lo=None, area=None):
    n = len(scores)
    boxes = np.asarray(boxes, dtype=np.int64).reshape(n, 4)
    return dict(boxes=boxes.astype(np.int32), scores=np.asarray(scores, dtype=np.float32),
                hi=np.full(n, 99, np.int32) if hi is None else np.asarray(hi, dtype=np.int32),
                lo=np.full(n, 100, np.int32) if lo is None else np.asarray(lo, dtype=np.int32),
                area=np.full(n, 50, np.int32) if area is None else np.asarray(area, dtype=np.int32), thr=thr)


def _rand_boxes(rng, n, span=1024, size=200):
    x0, y0 = rng.integers(0, span - 1, n), rng.integers(0, span - 1, n)
    return np.stack([x0, y0, x0 + rng.integers(1, size, n), y0 + rng.integers(1, size, n)], 1)


def _shift(units, n, pitch=400):
    """n rows from repeating `units` (a [u,4] pattern) translated so that copies never overlap"""
    u = len(units)
    reps = (n + u - 1) // u
    k = np.arange(reps)
    off = np.stack([(k % 64) * pitch, (k // 64) * pitch], 1)
    full = (np.asarray(units)[None, :, :] + np.concatenate([off, off], 1)[:, None, :]).reshape(-1, 4)
    return full[:n]


def _desc(n):
    """distinct scores in (0.9, 1), descending with the row"""
    return (1.0 - (np.arange(n) + 1) / (10.0 * (n + 1))).astype(np.float32)


T0 = (0.0, 0.0)    # both score filters off


def t_random(n, seed=0):
    rng = np.random.default_rng(seed)
    return _table(_rand_boxes(rng, n), rng.random(n, dtype=np.float32), T0 + (0.7,))


def t_big(n, seed=1):
    """crop-sized boxes of an 8192-pixel image: areas beyond 2^24, where a product fused into the union changes the quotient"""
    rng = np.random.default_rng(seed)
    x0, y0 = rng.integers(0, 3000, n), rng.integers(0, 3000, n)
    b = np.stack([x0, y0, x0 + rng.integers(4097, 5200, n), y0 + rng.integers(4097, 5200, n)], 1)
    return _table(b, rng.random(n, dtype=np.float32), T0 + (0.5,))


def t_identical(n, seed=2):
    rng = np.random.default_rng(seed)
    return _table(np.tile([[10, 20, 300, 400]], (n, 1)), rng.random(n, dtype=np.float32), T0 + (0.7,))


def t_chain(n):
    """A > B > C by score: A removes B (IoU 0.8) but not C (0.6); B, had it lived, would remove C (0.75)"""
    return _table(_shift([[0, 0, 100, 100], [0, 0, 100, 80], [0, 0, 100, 60]], n), _desc(n), T0 + (0.7,))


def t_exact(n, num, den):
    """pairs whose IoU is exactly num / den, compared with the threshold num / den (as a Python float): both are kept"""
    return _table(_shift([[0, 0, den, 10], [0, 0, num, 10]], n), _desc(n), T0 + (num / den,))


def t_steps(n, thr=0.5):
    """the exact pair at 1/2 and its two neighbours one integer step to either side: 11/20 is removed, 9/20 and 10/20 stay"""
    units = [[0, 0, 20, 10], [0, 0, 10, 10], [400, 0, 420, 10], [400, 0, 411, 10], [800, 0, 820, 10], [800, 0, 809, 10]]
    return _table(_shift(units, n, pitch=1200), _desc(n), T0 + (thr,))


def t_equal_scores(n, seed=3):
    rng = np.random.default_rng(seed)
    return _table(_rand_boxes(rng, n, span=300), np.full(n, 0.5, np.float32), T0 + (0.3,))


def t_signed(n, seed=4):
    """+0.0, -0.0, negative and positive scores, many of them equal"""
    rng = np.random.default_rng(seed)
    pool = np.array([0.0, -0.0, -1.5, -1e-30, 2.0, 1e-30, -3.25, 0.0, -0.0], np.float32)
    return _table(_rand_boxes(rng, n, span=300), pool[rng.integers(0, len(pool), n)], T0 + (0.3,))


def t_empty(n, seed=5):
    """empty boxes (zero width, height or both), some of them identical (0 / 0), among ordinary ones"""
    rng = np.random.default_rng(seed)
    b = _rand_boxes(rng, n, span=200)
    kind = rng.integers(0, 4, n)
    b[kind == 0, 2] = b[kind == 0, 0]
    b[kind == 1, 3] = b[kind == 1, 1]
    b[kind == 2] = [7, 7, 7, 7]
    return _table(b, rng.random(n, dtype=np.float32), T0 + (0.3,))


def t_filters(n, seed=6, thr=(0.88, 0.95, 0.7)):
    """rows on and around both filter thresholds: predicted IoU exactly float32(thr), one step above and below; stability 19/20
    (== float32(0.95): passes), 0/0 (NaN: fails), 5/0 (inf: passes), 94/100; area 0 with the statistics kernel's empty box"""
    rng = np.random.default_rng(seed)
    t32 = np.float32(thr[0])
    iou_pool = np.array([t32, np.nextafter(t32, np.float32(2)), np.nextafter(t32, np.float32(0)), 0.97, 0.5, 0.93], np.float32)
    frac = [(19, 20), (0, 0), (5, 0), (94, 100), (96, 100), (950001, 1000000), (1, 1), (18999999, 20000000)]
    pick = rng.integers(0, len(frac), n)
    hi, lo = np.array([frac[i][0] for i in pick]), np.array([frac[i][1] for i in pick])
    scores = iou_pool[rng.integers(0, len(iou_pool), n)]
    boxes = _rand_boxes(rng, n, span=400)
    area = rng.integers(1, 5000, n)
    empty = rng.random(n) < 0.2
    area[empty] = 0
    boxes[empty] = [INT_MAX, INT_MAX, -1, -1]
    return _table(boxes, scores, thr, hi, lo, area)


def t_clustered(n, seed=7, clusters=200):
    """n boxes in `clusters` tight clusters (IoU inside a cluster > 0.9, none between clusters): about `clusters` are kept"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, clusters, n)
    x0, y0 = (c % 16) * 300 + rng.integers(0, 3, n), (c // 16) * 300 + rng.integers(0, 3, n)
    b = np.stack([x0, y0, x0 + 200 + rng.integers(0, 3, n), y0 + 200 + rng.integers(0, 3, n)], 1)
    return _table(b, rng.random(n, dtype=np.float32), T0 + (0.7,))


def with_thr(t, **kw):
    """a copy of the table with some thresholds replaced: iou=, stab=, nms="""
    a, b, c = t["thr"]
    return dict(t, thr=(kw.get("iou", a), kw.get("stab", b), kw.get("nms", c)))


def tables(n):
    """name -> table of n rows: every kind the device kernels are held to at this size"""
    out = {
        "random": t_random(n), "big": t_big(n), "identical": t_identical(n), "chain": t_chain(n),
        "exact_7_10": t_exact(n, 7, 10), "exact_1_2": t_exact(n, 1, 2), "exact_1_3": t_exact(n, 1, 3), "exact_4_5": t_exact(n, 4, 5),
        "steps": t_steps(n), "equal_scores": t_equal_scores(n), "signed": t_signed(n), "empty": t_empty(n),
        "filters": t_filters(n), "filters_0_8": t_filters(n, thr=(0.8, 0.95, 0.7)),
        "filters_off": with_thr(t_filters(n), iou=0.0, stab=0.0),
        "filters_nms1": with_thr(t_filters(n), nms=1.0), "random_nms1": with_thr(t_random(n), nms=1.0),
        "identical_nms1": with_thr(t_identical(n), nms=1.0),                  # IoU == 1.0 == threshold: every box stays
        "all_nms1": with_thr(t_filters(n), iou=0.0, stab=0.0, nms=1.0),
    }
    return out


# which tables must tell each fault from the reference, from `min_n` rows on
SEPARATES = {
    "ge": (["exact_1_2", "steps", "identical_nms1"], 2),
    "no_f64": (["exact_1_3", "exact_4_5"], 2),
    "unstable": (["equal_scores", "signed"], 63),
    "no_empty_rule": (["filters", "filters_off"], 63),
    "stab_f64": (["filters", "filters_nms1"], 63),
    "dead_suppresses": (["chain"], 3),
}


def split_offsets(n, G):
    """G = 1: one group; G = 3: unequal groups with an empty one in the middle"""
    if G == 1:
        return [0, n]
    a = n // 3
    return [0, a, a, n]
