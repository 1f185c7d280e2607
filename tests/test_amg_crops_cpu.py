"""CPU: tests/amg_crops_reference.py - what tests/test_amg_crops_gpu.py holds psam_amg_keep_planes / psam_amg_crops_nms to - is the
merge and cross-crop NMS of SamAutomaticMaskGenerator._crops_host, its inputs contain the cases they claim, and the comparison of
the GPU tests tells a dropped record, a record of the wrong crop, an untranslated box and a wrong tie order from the reference."""
import inspect

import numpy as np
import pytest

import amg_crops_reference as cr
from protosam_amd.segment_anything.utils.amg import nms_xyxy

TOTALS = (63, 64, 65, 255, 256, 257)


def _host_lines(per_crop, crop_boxes, thr):
    """`_crops_host` behind its per-crop stage, line for line, over the dicts `_process_crop` returns (boxes already translated)"""
    parts = []
    for r, cb in zip(per_crop, crop_boxes):
        x0, y0 = cb[0], cb[1]
        parts.append(dict(boxes=r[:, 5:9].astype(np.int64) + np.array([[x0, y0, x0, y0]]), rec=r[:, :5],
                          crop_boxes=np.tile(np.array([cb], dtype=np.int64), (len(r), 1))))
    data = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    rows = np.arange(len(data["boxes"]))
    if len(crop_boxes) > 1:
        cb = data["crop_boxes"].astype(np.float32)
        scores = 1.0 / ((cb[:, 2] - cb[:, 0]) * (cb[:, 3] - cb[:, 1]))
        keep = nms_xyxy(data["boxes"], scores, thr)
        data = {k: v[keep] for k, v in data.items()}
        rows = rows[keep]
    return data, rows


def test_host_lines_are_the_generators():
    """the lines `_host_lines` restates are in `_crops_host`, and the geometry table's score is their float32 expression"""
    from protosam_amd import ops
    from protosam_amd.segment_anything import SamAutomaticMaskGenerator
    src = inspect.getsource(SamAutomaticMaskGenerator._crops_host)
    for line in ('data = {k: np.concatenate([p[k] for p in parts]) for k in parts[0] if k != "masks"}', "if len(crop_boxes) > 1:",
                 'cb = data["crop_boxes"].astype(np.float32)', "scores = 1.0 / ((cb[:, 2] - cb[:, 0]) * (cb[:, 3] - cb[:, 1]))",
                 'keep = nms_xyxy(data["boxes"], scores, self.crop_nms_thresh)'):
        assert line in src, line
    boxes = cr.layout(2) + [[0, 0, 8192, 8192], [3, 5, 4, 6], [0, 0, 1500, 2250]]
    g = ops.amg_crop_geometry(boxes, [(1024, 768)] * len(boxes))
    cb = np.asarray(boxes, dtype=np.int64).astype(np.float32)
    want = 1.0 / ((cb[:, 2] - cb[:, 0]) * (cb[:, 3] - cb[:, 1]))
    assert want.dtype == np.float32 and np.array_equal(g[:, 6].view(np.float32), want) and np.array_equal(cr.crop_scores(boxes), want)
    assert g.dtype == np.int32 and g[:, :4].tolist() == [[b[0], b[1], b[2] - b[0], b[3] - b[1]] for b in boxes]
    assert (g[:, 4] == 1024).all() and (g[:, 5] == 768).all() and (g[:, 7] == 0).all()
    assert ops.AMG_CREC == cr.CREC and ops.AMG_REC == cr.REC


@pytest.mark.parametrize("total", TOTALS)
@pytest.mark.parametrize("kind", cr.KINDS)
def test_reference_is_the_host_code(kind, total):
    c = cr.case(kind, total, seed=total)
    assert sum(len(r) for r in c["per_crop"]) == total
    ref = cr.final_reference(c["per_crop"], c["crop_boxes"], c["thr"])
    data, rows = _host_lines(c["per_crop"], c["crop_boxes"], c["thr"])
    assert np.array_equal(ref[:, 5:9], data["boxes"]) and np.array_equal(ref[:, :5], data["rec"])
    assert np.array_equal(ref[:, cr.REC + 1], rows)
    assert np.array_equal(np.asarray(c["crop_boxes"])[ref[:, cr.REC]], data["crop_boxes"])
    cr.same_final(ref, cr.final_reference(c["per_crop"], c["crop_boxes"], c["thr"]))


def test_inputs_hold_what_they_claim():
    for total in TOTALS:
        sizes = {k: [len(r) for r in cr.case(k, total)["per_crop"]] for k in cr.KINDS}
        assert sizes["empty_crops"][0] == sizes["empty_crops"][2] == sizes["empty_crops"][4] == 0 and min(sizes["empty_crops"][1::2]) > 0
        assert sizes["first_empty"][0] == 0 and min(sizes["first_empty"][1:]) > 0
        assert len(sizes["single"]) == 1 and min(sizes["clustered"]) > 0
        # a single crop box: no NMS, although every box is the same one
        c = cr.case("single", total)
        assert len(cr.final_reference(c["per_crop"], c["crop_boxes"], c["thr"])) == total
        # IoU == threshold stays: all of identical_nms1; of "exact"'s triples the pairs at 10/20 and 9/20 stay whole
        c = cr.case("identical_nms1", total)
        assert len(cr.final_reference(c["per_crop"], c["crop_boxes"], c["thr"])) == total
        # equal scores inside a crop and between the four layer-1 crops, and suppression does happen
        c = cr.case("clustered", total)
        s = cr.crop_scores(c["crop_boxes"])
        assert s[1] == s[2] == s[3] == s[4] > s[0]
        assert 0 < len(cr.final_reference(c["per_crop"], c["crop_boxes"], c["thr"])) < total
    c = cr.case("exact", 6)
    ref = cr.final_reference(c["per_crop"], c["crop_boxes"], c["thr"])
    # crop 1's three wide boxes come first (smaller crop), then crop 0's narrow ones at IoU 1/2 (stays) and 9/20 (stays); 11/20 goes
    assert ref[:, cr.REC].tolist() == [1, 1, 1, 0, 0] and ref[3:, 5:9].tolist() == [[300, 200, 310, 210], [380, 200, 389, 210]]


@pytest.mark.parametrize("fault", cr.FAULTS)
def test_comparison_catches_fault(fault):
    for kind in cr.SEPARATES[fault]:
        for total in TOTALS:
            c = cr.case(kind, total, seed=total)
            ref = cr.final_reference(c["per_crop"], c["crop_boxes"], c["thr"])
            bad = cr.final_reference(c["per_crop"], c["crop_boxes"], c["thr"], fault=fault)
            with pytest.raises(AssertionError):
                cr.same_final(bad, ref)


def test_crops_switch_is_validated(monkeypatch):
    """PSAM_AMG_CROPS is read in the constructor and validated like the other three; crop_pool_cap is bounded by the NMS group"""
    from protosam_amd import ops, synth_cases as gi
    from protosam_amd.segment_anything import SamAutomaticMaskGenerator, sam_model_registry
    sam = sam_model_registry["vit_b"](encoder_depth=gi.AMG_ENCODER_DEPTH)
    monkeypatch.delenv("PSAM_AMG_CROPS", raising=False)
    g = SamAutomaticMaskGenerator(sam, **gi.AMG_CROP_ARGS)
    assert g.amg_crops == "host" and g.crop_pool_cap is None
    assert g._crop_pool_rows([192, 48, 48, 48, 48]) == 384 and g._crop_pool_rows([3072] * 5) == 5 * 256
    assert g._crop_pool_rows([3072] * 341) == ops.NMS_MAX_GROUP
    monkeypatch.setenv("PSAM_AMG_CROPS", "device")
    assert SamAutomaticMaskGenerator(sam, crop_pool_cap=7, **gi.AMG_CROP_ARGS)._crop_pool_rows([192]) == 7
    monkeypatch.setenv("PSAM_AMG_CROPS", "gpu")
    with pytest.raises(ValueError, match="PSAM_AMG_CROPS"):
        SamAutomaticMaskGenerator(sam)
    monkeypatch.setenv("PSAM_AMG_CROPS", "host")
    for cap in (0, ops.NMS_MAX_GROUP + 1):
        with pytest.raises(ValueError, match="crop_pool_cap"):
            SamAutomaticMaskGenerator(sam, crop_pool_cap=cap)
