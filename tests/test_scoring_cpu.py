"""CPU: the host half of the scoring path - `metrics.Metric` on counts tables against the outputs recorded from the reference's own
`util.metric.Metric` (tests/golden/reference_metric.npz, tools/record_reference_metric.py), `score_slices` / `calc_iou` against a
transcription of validation_protosam.py:169-185,400-448, the row tables, the host range check of `ops.seg_counts`, and the
all-gather of a counts table at world 2 under gloo."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1
CALLS = [("get_mIoU", False), ("get_mDice", True), ("get_mPrecRecall", True), ("get_mIoU_binary", False)]
REL = 1e-12     # the same float64 expressions on integers below 2^53; the margin covers another numpy's summation order in mean / std


def load_fixture():
    f = np.load(os.path.join(ROOT, "tests", "golden", "reference_metric.npz"))
    res = {}
    off, vals = f["results.offsets"], f["results.values"]
    for i, (name, shape) in enumerate(zip(f["results.names"].tolist(), f["results.shapes"].tolist())):
        if shape == "none":
            res[name] = None
        else:
            res[name] = vals[off[i]:off[i + 1]].reshape([int(d) for d in shape.split(",")] if shape else [])
    return f, res


def np_counts(pred, label, rows):
    """psam_seg_counts in numpy: pred / label [planes, H, W], rows [n, 4] -> int64 [n, 12]; rows outside the planes keep the
    initial values."""
    out = np.zeros((len(rows), 12), dtype=np.int64)
    out[:, [4, 5, 8, 9]] = INT_MAX
    out[:, [6, 7, 10, 11]] = -1
    for k, (pp, pv, lp, lv) in enumerate(np.asarray(rows).tolist()):
        if not (0 <= pp < pred.shape[0] and 0 <= lp < label.shape[0]):
            continue
        p, g = pred[pp] == pv, label[lp] == lv
        out[k, :4] = [(p & g).sum(), (p & ~g).sum(), (~p & g).sum(), (~p & ~g).sum()]
        for col, m in ((4, p), (8, g)):
            if m.any():
                ys, xs = np.nonzero(m)
                out[k, col:col + 4] = [xs.min(), ys.min(), xs.max(), ys.max()]
    return out


def variants(n_scans):
    out = [("all", {}, False), ("all_raw", {"give_raw": True}, True)]
    for k in range(n_scans):
        out += [(f"scan{k}", {"n_scan": k}, False), (f"scan{k}_raw", {"n_scan": k, "give_raw": True}, True)]
    return out


def check_against_fixture(metric, name, n_scans, res, rel=REL):
    """every get_* of `metric`, in every recorded form, against the reference's recorded tuple"""
    n_checked = 0
    for method, has_raw in CALLS:
        for var, kw, raw in variants(n_scans):
            if raw and not has_raw:
                continue
            with np.errstate(all="ignore"):
                got = getattr(metric, method)(**kw)
            key = f"{name}.{method}.{var}"
            assert len(got) == int(res[key + ".len"]), key
            for i, v in enumerate(got):
                want = res[f"{key}.{i}"]
                if want is None:
                    assert v is None, (key, i)
                    continue
                v = np.asarray(v, dtype=np.float64)
                assert v.shape == want.shape, (key, i, v.shape, want.shape)
                assert np.array_equal(np.isnan(v), np.isnan(want)), (key, i, v, want)
                ok = ~np.isnan(want)
                assert np.all(np.abs(v[ok] - want[ok]) <= rel * np.abs(want[ok])), (key, i, v, want)
                n_checked += int(ok.sum())
    return n_checked


def feed(record_a, record_b, record_c, f):
    """the recorder's three record loops through the given record functions"""
    gt, pred, organs = f["gt"], f["pred"], f["organs"]
    for s in range(gt.shape[0]):
        for z in range(gt.shape[1]):
            for lb in range(1, organs.shape[1]):
                if organs[s, lb]:
                    record_a((pred[s, z] == lb).astype(np.uint8), (gt[s, z] == lb).astype(np.uint8), [lb], s)
            record_b(pred[s, z], gt[s, z], None, s)
            if s == 0:
                record_c(pred[s, z], gt[s, z], None, None)


def test_metric_on_numpy_counts_reproduces_the_reference():
    from protosam_amd.metrics import Metric
    f, res = load_fixture()
    S, L = f["gt"].shape[0], f["organs"].shape[1] - 1
    A, B, C = Metric(L, S), Metric(L, S), Metric(L)

    def via_table(m):
        return lambda p, g, labels, s: m.record_table(np_counts(p[None], g[None], m.record_rows(labels)), labels, s)
    feed(via_table(A), via_table(B), via_table(C), f)
    assert A.slice_counter == [32, 24, 32] and B.slice_counter == [8, 8, 8] and C.slice_counter == [8]
    n = check_against_fixture(A, "A", S, res) + check_against_fixture(B, "B", S, res) + check_against_fixture(C, "C", 1, res)
    assert n > 300
    # the NaN paths are in the fixture: scan 1 never records organ 3, organ 4 of scan 2 has tp + fp + fn == 0
    d = A.get_mDice(n_scan=1)[0]
    assert np.isnan(d[3]) and not np.isnan(d[2]) and np.isnan(A.get_mDice(n_scan=2)[0][4])
    # reset_scan / reset
    A.reset_scan(0, labels=[2])
    assert np.isnan(A.get_mDice(n_scan=0)[0][2]) and not np.isnan(A.get_mDice(n_scan=0)[0][1])
    A.reset()
    with pytest.raises(ValueError):
        A.get_mDice()


def _host_seg_counts(pred, label, rows, out=None):
    p = pred.reshape((-1,) + tuple(pred.shape[-2:])).numpy()
    g = label.reshape((-1,) + tuple(label.shape[-2:])).numpy()
    return torch.from_numpy(np_counts(p, g, rows))


def test_record_and_record_batch_bookkeeping(monkeypatch):
    """`record` / `record_batch` with the kernel replaced by its numpy statement: the deferred fill, the position-not-label rule, and
    the one-row-per-(slice, class) form of [n, C, H, W] masks equal the loop of `record` calls (the device test repeats this on the
    real kernel)."""
    from protosam_amd import metrics, ops
    monkeypatch.setattr(ops, "seg_counts", _host_seg_counts)
    f, res = load_fixture()
    gt, pred, organs = torch.from_numpy(f["gt"]), torch.from_numpy(f["pred"]), f["organs"]
    S, Z, L = gt.shape[0], gt.shape[1], organs.shape[1] - 1
    A, B = metrics.Metric(L, S), metrics.Metric(L, S)
    for s in range(S):
        for z in range(Z):
            for lb in range(1, L + 1):
                if organs[s, lb]:
                    A.record((pred[s, z] == lb).to(torch.uint8), (gt[s, z] == lb).to(torch.uint8), labels=[lb], n_scan=s)
        B.record_batch(pred[s], gt[s], None, s)
    assert len(A._pending) == 88 and len(B._pending) == 3
    assert check_against_fixture(A, "A", S, res) > 100 and check_against_fixture(B, "B", S, res) > 100
    assert not A._pending
    # [n, C, H, W] binary masks against the label map, one launch per scan
    A4 = metrics.Metric(L, S)
    for s in range(S):
        cls = [lb for lb in range(1, L + 1) if organs[s, lb]]
        masks = torch.stack([(pred[s] == lb).to(torch.uint8) for lb in cls], dim=1)
        A4.record_batch(masks, gt[s], cls, s)
    assert A4.slice_counter == [32, 24, 32]
    assert check_against_fixture(A4, "A", S, res) > 100
    # position, not label: labels=[3] compares the VALUE 1 in both maps and stores under 3
    M = metrics.Metric(4)
    p, g = torch.zeros((4, 4), dtype=torch.uint8), torch.zeros((4, 4), dtype=torch.uint8)
    p[0, :3], g[0, 1:] = 1, 1
    p[3, 3] = 3
    M.record(p, g, labels=[3])
    M._flush()
    assert M.tp_lst[0][0][3] == 2 and M.fp_lst[0][0][3] == 1 and M.fn_lst[0][0][3] == 1 and np.isnan(M.tp_lst[0][0][1])
    assert M.tp_lst[0][0][0] == 11 and M.fp_lst[0][0][0] == 1 and M.fn_lst[0][0][0] == 2


def _transcribed_loop(counts, scores, cases, skip):
    """validation_protosam.py:169-185,400-448 on counts, written out in the order of the reference's loop"""
    mean_dice, mean_prec, mean_rec, mean_iou, boxes, dice_cases, iou_cases = [], [], [], [], [], {}, {}
    for k, row in enumerate(counts):
        tp, fp, fn = float(row[0]), float(row[1]), float(row[2])
        if tp + fn == 0 and skip:
            continue
        if tp + fn == 0:
            metrics = {"dice": 0, "precision": 0, "recall": 0}
        else:
            metrics = {"dice": 2 * tp / (2 * tp + fp + fn + 1e-8), "precision": tp / (tp + fp + 1e-8), "recall": tp / (tp + fn + 1e-8),
                       "iou": tp / (tp + fp + fn + 1e-8)}
        mean_dice.append(metrics["dice"]); mean_prec.append(metrics["precision"]); mean_rec.append(metrics["recall"])
        mean_iou.append(metrics["iou"])

        def rect(b):
            return (0, 0, 0, 0) if b[2] < b[0] else (b[0], b[1], b[2] - b[0] + 1, b[3] - b[1] + 1)
        boxes.append({"pred_bbox": rect(row[4:8]), "gt_bbox": rect(row[8:12]), "score": np.mean(scores[k])})
        dice_cases.setdefault(cases[k], []).append(metrics["dice"])
        iou_cases.setdefault(cases[k], []).append(metrics["iou"])
    return (np.mean(mean_dice), np.mean(mean_prec), np.mean(mean_rec), np.mean(mean_iou), boxes,
            {c: np.mean(v) for c, v in dice_cases.items()}, {c: np.mean(v) for c, v in iou_cases.items()})


def test_score_slices_against_the_transcribed_loop():
    from protosam_amd.metrics import score_slices
    rng = np.random.default_rng(5)
    n, H, W = 40, 24, 31
    pred = (rng.random((n, H, W)) < 0.3).astype(np.uint8)
    gt = (rng.random((n, H, W)) < 0.3).astype(np.uint8)
    gt[[3, 17]] = 0                                  # empty ground truth: skipped, or the loop fails
    pred[5] = 0                                      # empty prediction: box (0, 0, 0, 0)
    counts = np_counts(pred, gt, [(k, 1, k, 1) for k in range(n)])
    scores = [rng.random(1 + k % 3).astype(np.float32) for k in range(n)]
    cases = [f"case{k // 9}" for k in range(n)]
    want = _transcribed_loop(counts, scores, cases, True)
    got = score_slices(torch.from_numpy(counts), scores, cases, skip_no_organ_slices=True)
    assert got["rows"] == [k for k in range(n) if k not in (3, 17)]
    for name, w in zip(("mean_dice", "mean_precision", "mean_recall", "mean_iou"), want[:4]):
        assert abs(got[name] - w) <= 1e-12 * abs(w), name
    assert [{k: (tuple(int(x) for x in v) if k != "score" else v) for k, v in b.items()} for b in want[4]] == \
        [dict(b) for b in got["bboxes_w_scores"]]
    assert got["bboxes_w_scores"][5 - 1]["pred_bbox"] == (0, 0, 0, 0)                    # (row 5 is entry 4: row 3 was skipped)
    assert got["dice_cases"].keys() == want[5].keys()
    for c in want[5]:
        assert abs(got["dice_cases"][c] - want[5][c]) <= 1e-12 and abs(got["iou_cases"][c] - want[6][c]) <= 1e-12
    with pytest.raises(KeyError, match="row 3"):
        score_slices(counts, scores, cases, skip_no_organ_slices=False)
    with pytest.raises(KeyError):
        _transcribed_loop(counts, scores, cases, False)
    # per-row values against the reference's own function on these maps (recorded in float32: a few ulps of a value <= 1)
    f, _ = load_fixture()
    tri = f["formula.triples"]
    rows = [(i, 1, i, 1) for i in range(len(tri))]
    p = np.stack([f["pred"][s, z] == lb for s, z, lb in tri]).astype(np.uint8)
    g = np.stack([f["gt"][s, z] == lb for s, z, lb in tri]).astype(np.uint8)
    sc = score_slices(np_counts(p, g, rows))
    assert len(tri) >= 20 and sc["rows"] == list(range(len(tri)))
    for col, name in enumerate(("dice", "iou", "precision", "recall")):
        assert np.abs(sc[name] - f["formula.values"][:, col]).max() < 1e-6


def test_calc_iou_and_boxes():
    from protosam_amd.metrics import box_xywh, calc_iou
    assert calc_iou((0, 0, 4, 4), (10, 10, 2, 2)) == 0.0                     # disjoint
    assert calc_iou((0, 0, 10, 10), (2, 3, 4, 5)) == 20 / 100                # nested
    assert calc_iou((3, 4, 5, 6), (3, 4, 5, 6)) == 1.0                       # equal
    assert calc_iou((0, 0, 4, 4), (2, 2, 4, 4)) == 4 / 28
    assert box_xywh(2, 3, 2, 3) == (2, 3, 1, 1) and box_xywh(INT_MAX, INT_MAX, -1, -1) == (0, 0, 0, 0)
    assert box_xywh(0, 5, 9, 7) == (0, 5, 10, 3)


def test_class_rows():
    from protosam_amd.metrics import class_rows
    r = class_rows(2, [1, 6, 3])
    assert r.dtype == np.int32 and r.tolist() == [[0, 1, 0, 1], [1, 1, 0, 6], [2, 1, 0, 3], [3, 1, 1, 1], [4, 1, 1, 6], [5, 1, 1, 3]]
    assert class_rows(3).tolist() == [[0, 1, 0, 1], [1, 1, 1, 1], [2, 1, 2, 1]]
    assert class_rows(2, [4], label_planes=[7, 9]).tolist() == [[0, 1, 7, 4], [1, 1, 9, 4]]
    assert class_rows(2, None, label_planes=[7, 9], label_value=5).tolist() == [[0, 1, 7, 5], [1, 1, 9, 5]]
    assert class_rows(0, [1]).shape == (0, 4)
    with pytest.raises(ValueError):
        class_rows(2, [1], label_planes=[0])


def test_seg_counts_checks_a_row_list_on_the_host():
    """a bad plane index in a Python row list is a ValueError before any device call (the tensors here are not even on a device)"""
    from protosam_amd import ops
    pred, label = torch.zeros((2, 3, 8, 8), dtype=torch.uint8), torch.zeros((2, 8, 8), dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"rows\[1\]: prediction plane 6"):
        ops.seg_counts(pred, label, [(0, 1, 0, 1), (6, 1, 0, 1)])
    with pytest.raises(ValueError, match="label plane 2"):
        ops.seg_counts(pred, label, [(5, 1, 2, 1)])
    with pytest.raises(ValueError, match="label plane -1"):
        ops.seg_counts(pred, label, [(5, 1, -1, 1)])
    with pytest.raises(ValueError, match="differ"):
        ops.seg_counts(pred, torch.zeros((2, 8, 9), dtype=torch.uint8), [(0, 1, 0, 1)])
    with pytest.raises(RuntimeError, match="device tensor"):                 # good rows: only now the missing device is noticed
        ops.seg_counts(pred, label, [(5, 1, 1, 1)])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fake_counts(z, C=3):
    g = torch.Generator().manual_seed(300 + z)
    return torch.randint(0, 2 ** 40, (C, 12), generator=g, dtype=torch.int64)


def _gather_worker(rank, world, port, n_slices, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from protosam_amd.runner import gather_counts, interleave_rank_major, shard_slices
    zs = shard_slices(n_slices, rank, world)
    k = -(-n_slices // world)
    local = torch.zeros((k, 3, 12), dtype=torch.int64)
    for i, z in enumerate(zs):
        local[i] = _fake_counts(z)
    full = gather_counts(local.view(k * 3, 12), world)                       # [world * k * C, 12], as the evaluate_* tables
    ok = full.shape == (world * k * 3, 12) and full.dtype == torch.int64
    table = interleave_rank_major(full.view(world * k, 3, 12), n_slices, world).reshape(n_slices * 3, 12)
    one_rank = torch.cat([_fake_counts(z) for z in range(n_slices)])
    q.put((rank, bool(ok and torch.equal(table, one_rank))))
    dist.destroy_process_group()


@pytest.mark.parametrize("n_slices", [8, 7])
def test_two_rank_gather_of_counts_matches_one_rank(n_slices):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, n_slices, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok in res)
    from protosam_amd.runner import gather_counts
    t = _fake_counts(0)
    assert gather_counts(t, 1) is t
