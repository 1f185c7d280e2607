"""CPU: tests/amg_select_reference.py (what the GPU tests of psam_box_nms / psam_amg_select compare against).

  the reference    its restated NMS loop without a fault equals utils.amg.nms_xyxy; `select_lines` equals the generator's own
                   host lines (`SamAutomaticMaskGenerator._select_host`) run on the same table
  the tables       hold what they claim: IoUs exactly on the threshold, stabilities exactly on theirs, areas beyond 2^24
  injected faults  `>=` for `>`, the float64 comparison dropped, an unstable tie order, the area == 0 box rule dropped, stability
                   compared in float64, a suppressed box allowed to suppress: at every size of the GPU test that can hold the
                   structure, the tables named in SEPARATES tell each of them from the reference
"""
import numpy as np
import pytest
import torch

import amg_select_reference as ar
from protosam_amd.segment_anything.utils.amg import nms_xyxy

SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 3072]


@pytest.mark.parametrize("n", SIZES[:-1])
def test_faultless_loop_equals_nms_xyxy(n):
    for name, t in ar.tables(n).items():
        got = ar.nms_faulty(t["boxes"], t["scores"], t["thr"][2], None)
        assert np.array_equal(got, nms_xyxy(t["boxes"], t["scores"], t["thr"][2])), name


@pytest.mark.parametrize("n", [0, 1, 65, 257])
def test_select_lines_equal_the_generators_host_lines(n):
    """`_select_host` fed with the table (CPU tensors stand in for the device's) gives the same candidates, field by field"""
    from protosam_amd.segment_anything import SamAutomaticMaskGenerator
    for name, t in ar.tables(n).items():
        m = 3 * ((n + 2) // 3)                                # the generator always holds whole prompts
        stats, iou4 = ar.make_stats(t)
        stats = np.concatenate([stats, np.zeros((m - n, 8), np.int32)])
        g = SamAutomaticMaskGenerator.__new__(SamAutomaticMaskGenerator)
        g.pred_iou_thresh, g.stability_score_thresh, g.box_nms_thresh = t["thr"]
        ctx = dict(pts=np.zeros((m // 3, 2)), n=m // 3, low=torch.zeros(1), stats=torch.from_numpy(stats), iou=torch.from_numpy(iou4),
                   size=(8, 8))
        cand = g._select_host(ctx)
        iou = iou4[:, 1:].reshape(-1)
        rec = ar.select_lines(stats, iou, *t["thr"])
        assert np.array_equal(cand["plane"].numpy(), rec[:, 1]), name
        assert np.array_equal(cand["iou_preds"].view(np.int32), rec[:, 2]) and np.array_equal(cand["area"], rec[:, 4]), name
        assert np.array_equal(cand["stability_score"].view(np.int32), rec[:, 3]) and np.array_equal(cand["boxes"], rec[:, 5:9]), name


def test_tables_hold_what_they_claim():
    f32 = np.float32
    for num, den in ((7, 10), (1, 2), (1, 3), (4, 5)):
        b = ar.t_exact(2, num, den)["boxes"].astype(f32)
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        assert area[1] / (area[0] + area[1] - area[1]) == f32(num) / f32(den)
    # the pairs that separate the comparison's width: fp32(1/3) and fp32(4/5) lie above the double, fp32(7/10) below
    assert float(f32(1) / f32(3)) > 1 / 3 and float(f32(4) / f32(5)) > 4 / 5 and float(f32(7) / f32(10)) < 7 / 10
    assert f32(19) / f32(20) == f32(0.95) and float(f32(19) / f32(20)) < 0.95
    t = ar.t_filters(257)
    assert (t["scores"] == f32(0.88)).any() and (t["area"] == 0).any() and ((t["hi"] == 0) & (t["lo"] == 0)).any()
    b = ar.t_big(64)["boxes"].astype(np.int64)
    assert ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) > 2 ** 24).all()
    t = ar.t_chain(3)
    assert ar.nms_faulty(t["boxes"], t["scores"], 0.7, None).tolist() == [0, 2]
    kept = nms_xyxy(ar.t_clustered(16384)["boxes"][:2048], ar.t_clustered(16384)["scores"][:2048], 0.7)
    assert 150 <= len(kept) <= 200
    for n in (63, 3072):
        for name in ("steps", "exact_1_2", "exact_7_10"):      # on the threshold and below it stays, above it goes
            t = ar.tables(n)[name]
            want = n - (n + 2) // 6 if name == "steps" else n  # (row 3 of every six is the 11/20 box)
            assert len(nms_xyxy(t["boxes"], t["scores"], t["thr"][2])) == want, (n, name)


def _records(t, offsets, fault=None):
    stats, iou4 = ar.make_stats(t)
    return ar.select_groups(stats, iou4, offsets, t["thr"], fault=fault)


@pytest.mark.parametrize("fault,n", [(f, n) for f in ar.FAULTS for n in SIZES if n >= ar.SEPARATES[f][1]])
def test_fault_is_separated_at_every_size(fault, n):
    """(sizes below SEPARATES' minimum cannot hold the structure: one or two rows have no tie to break, no chain of three)"""
    names, _ = ar.SEPARATES[fault]
    tabs = ar.tables(n)
    for name in names:
        t = tabs[name]
        ref, bad = _records(t, [0, n]), _records(t, [0, n], fault)
        assert not np.array_equal(ref[0], bad[0]), (fault, name, n)
        if fault not in ("no_empty_rule", "stab_f64"):         # the NMS faults also show in psam_box_nms's own output
            a, b = ar.nms_groups(t["boxes"], t["scores"], [0, n], t["thr"][2]), ar.nms_groups(t["boxes"], t["scores"], [0, n],
                                                                                             t["thr"][2], fault)
            assert not np.array_equal(a[0], b[0]), (fault, name, n)


def test_groups_are_independent():
    """three unequal groups, the middle one empty: each equals the reference on its slice alone"""
    n = 257
    off = ar.split_offsets(n, 3)
    assert off[1] == off[2] and off[1] - off[0] != off[3] - off[2]
    for name, t in ar.tables(n).items():
        stats, iou4 = ar.make_stats(t)
        iou = iou4[:, 1:].reshape(-1)[:n]
        got = ar.select_groups(stats, iou4, off, t["thr"])
        for g, (lo, hi) in enumerate(zip(off[:-1], off[1:])):
            one = ar.select_lines(stats[lo:hi], iou[lo:hi], *t["thr"])
            assert np.array_equal(got[g][:, 2:], one[:, 2:]) and np.array_equal(got[g][:, 0], one[:, 0] + lo), (name, g)
