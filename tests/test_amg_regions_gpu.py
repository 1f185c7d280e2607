"""GPU: the generator's small-region stage on the device (PSAM_AMG_REGIONS=device: ops.small_regions_select, one download) against
the per-mask host loop (PSAM_AMG_REGIONS=host), and a crop's candidate selection on the device (PSAM_AMG_SELECT=device:
psam_amg_select_crop) against the host filters - record for record and mask for mask, on the synthetic ViT-B of synth_cases."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ENV = ("PSAM_AMG_RESIZE", "PSAM_AMG_SELECT", "PSAM_AMG_REGIONS")


def _image(h, w, seed):
    """a smooth random uint8 image [h, w, 3] with a few rectangles (the 225 x 300 image of test_amg_resize_gpu.py: seed 1)"""
    g = np.random.RandomState(seed)
    coarse = torch.from_numpy(g.rand(1, 3, h // 16 + 2, w // 16 + 2).astype(np.float32))
    img = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear")[0].permute(1, 2, 0).numpy() * 200.0
    for _ in range(4):
        y, x = g.randint(0, h - h // 4), g.randint(0, w - w // 4)
        img[y:y + h // 4, x:x + w // 4] = g.rand(3) * 255.0
    return np.ascontiguousarray(img.clip(0, 255).astype(np.uint8))


@pytest.fixture(scope="module")
def setup(dev):
    from protosam_amd import synth_cases as gi
    from protosam_amd.sam_wrapper import SamWrapper
    w = SamWrapper({"model_type": "vit_b", "sam_checkpoint": f"random:{gi.AMG_SEED}:{gi.AMG_ENCODER_DEPTH}",
                    "generator_args": dict(gi.AMG_ARGS)}).to(dev)
    return dict(w=w, images={"48x44": gi.amg_small_case(), "225x300": _image(225, 300, 1)}, cache={})


def _generator(s, regions="host", select="host", **kw):
    """a generator over the shared model; the three switches are read when it is built"""
    from protosam_amd.segment_anything import SamAutomaticMaskGenerator
    old = {k: os.environ.get(k) for k in ENV}
    os.environ.update(PSAM_AMG_RESIZE="fused", PSAM_AMG_SELECT=select, PSAM_AMG_REGIONS=regions)
    try:
        g = SamAutomaticMaskGenerator(s["w"].sam, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    assert g.amg_regions == regions and g.amg_select == select
    return g


def _host_records(s, name, **kw):
    """the records of the host routes, once per (image, arguments)"""
    key = (name, tuple(sorted(kw.items())))
    if key not in s["cache"]:
        s["cache"][key] = _generator(s, **kw).generate(s["images"][name])
    return s["cache"][key]


def _same_records(a, b):
    """masks, boxes, areas, scores, points, crop boxes and order"""
    assert len(a) == len(b), (len(a), len(b))
    for x, y in zip(a, b):
        assert set(x) == set(y)
        for k in x:
            if k == "segmentation":
                assert x[k].dtype == y[k].dtype == bool and np.array_equal(x[k], y[k])
            else:
                assert x[k] == y[k] and type(x[k]) is type(y[k]), (k, x[k], y[k])


def _wrap(obj, name, calls):
    inner = getattr(obj, name)
    setattr(obj, name, lambda *a, **k: (calls.append(name), inner(*a, **k))[1])


# with and without cross-crop suppression; holes / islands below 6 pixels and a threshold above every region (keep-largest);
# the stage's own NMS with and without suppression (its threshold is max(box_nms_thresh, crop_nms_thresh))
REGION_SETTINGS = {"area6": dict(), "area6_no_crop_nms": dict(crop_nms_thresh=1.0),
                   "area6_nms07": dict(box_nms_thresh=0.7), "above_all": dict(min_mask_region_area=10 ** 6),
                   "above_all_nms07": dict(min_mask_region_area=10 ** 6, box_nms_thresh=0.7),
                   "area50.5_no_crop_nms": dict(min_mask_region_area=50.5, crop_nms_thresh=1.0)}


@pytest.mark.parametrize("setting", list(REGION_SETTINGS))
@pytest.mark.parametrize("name", ["48x44", "225x300"])
def test_device_regions_equal_host_regions(dev, setup, name, setting):
    """AMG_CROP_ARGS (crop_n_layers = 1, min_mask_region_area = 6) and its variants: PSAM_AMG_REGIONS=device returns the records
    of PSAM_AMG_REGIONS=host, and never enters `_remove_small_regions`."""
    from protosam_amd import synth_cases as gi
    kw = dict(gi.AMG_CROP_ARGS, **REGION_SETTINGS[setting])
    ref = _host_records(setup, name, **kw)
    g = _generator(setup, regions="device", **kw)
    calls = []
    _wrap(g, "_remove_small_regions", calls)
    got = g.generate(setup["images"][name])
    _same_records(got, ref)
    assert calls == [], f"_remove_small_regions entered {len(calls)} times"
    h, w = setup["images"][name].shape[:2]
    n_crop = sum(1 for a in got if a["crop_box"] != [0, 0, w, h])
    print(f"{name} {setting}: {len(got)} records, {n_crop} from layer-1 crops")
    assert len(got) > 0
    if setting.startswith("above_all"):            # every hole is filled, the outer background too: the masks are the whole image
        assert all(a["area"] == h * w and a["bbox"] == [0, 0, w - 1, h - 1] for a in got)
        assert len(got) == 1 or setting == "above_all"      # coinciding boxes: the stage's NMS at 0.7 leaves the first


def test_host_route_still_loops(dev, setup):
    """The wrapper counts: PSAM_AMG_REGIONS=host enters `_remove_small_regions` twice per mask of the stage."""
    from protosam_amd import synth_cases as gi
    g = _generator(setup, regions="host", **gi.AMG_CROP_ARGS)
    calls = []
    _wrap(g, "_remove_small_regions", calls)
    got = g.generate(setup["images"]["48x44"])
    assert len(calls) >= 2 * len(got) > 0 and len(calls) % 2 == 0


def test_regions_switch_is_validated(dev, setup):
    old = os.environ.get("PSAM_AMG_REGIONS")
    os.environ["PSAM_AMG_REGIONS"] = "gpu"
    try:
        from protosam_amd.segment_anything import SamAutomaticMaskGenerator
        with pytest.raises(ValueError, match="PSAM_AMG_REGIONS"):
            SamAutomaticMaskGenerator(setup["w"].sam)
    finally:
        if old is None:
            del os.environ["PSAM_AMG_REGIONS"]
        else:
            os.environ["PSAM_AMG_REGIONS"] = old


SELECT_SETTINGS = {"all": dict(min_mask_region_area=0), "all_no_crop_nms": dict(min_mask_region_area=0, crop_nms_thresh=1.0),
                   "filters_nms07": dict(min_mask_region_area=0, box_nms_thresh=0.7, crop_nms_thresh=1.0),
                   "regions_device": dict()}


@pytest.mark.parametrize("setting", list(SELECT_SETTINGS))
@pytest.mark.parametrize("name", ["48x44", "225x300"])
def test_device_crop_selection_equals_host(dev, setup, name, setting):
    """PSAM_AMG_SELECT=device with crop layers: the records of PSAM_AMG_SELECT=host exactly; every crop is selected by
    `amg_select_crop` (one call per crop) and the host's filters over a downloaded statistics table (they end in
    `is_box_near_crop_edge`) never run."""
    from protosam_amd import ops, synth_cases as gi
    from protosam_amd.segment_anything.utils.amg import generate_crop_boxes
    kw = dict(gi.AMG_CROP_ARGS, **SELECT_SETTINGS[setting])
    if setting == "filters_nms07":                 # thresholds that some, not all, of this image's candidates pass
        every = _host_records(setup, name, **dict(gi.AMG_CROP_ARGS, **SELECT_SETTINGS["all_no_crop_nms"]))
        pos = [r["predicted_iou"] for r in every if r["predicted_iou"] > 0]
        assert len(pos) >= 4                       # (a threshold <= 0 would switch the filter off)
        iou_t = float(np.median(pos))
        stab = [r["stability_score"] for r in every if r["predicted_iou"] > iou_t and r["stability_score"] > 0]
        assert len(stab) >= 2
        stab_t = float(np.median(stab))
        kw = dict(kw, pred_iou_thresh=iou_t, stability_score_thresh=stab_t)
    ref = _host_records(setup, name, **kw)
    g = _generator(setup, regions="device" if setting == "regions_device" else "host", select="device", **kw)
    import protosam_amd.segment_anything.automatic_mask_generator as amg_mod
    calls = []
    inner_sel, inner_edge = ops.amg_select_crop, amg_mod.is_box_near_crop_edge
    ops.amg_select_crop = lambda *a, **k: (calls.append("amg_select_crop"), inner_sel(*a, **k))[1]
    amg_mod.is_box_near_crop_edge = lambda *a, **k: (calls.append("host edge filter"), inner_edge(*a, **k))[1]
    try:
        got = g.generate(setup["images"][name])
    finally:
        ops.amg_select_crop, amg_mod.is_box_near_crop_edge = inner_sel, inner_edge
    _same_records(got, ref)
    h, w = setup["images"][name].shape[:2]
    n_crops = len(generate_crop_boxes((h, w), 1, g.crop_overlap_ratio)[0])
    assert calls == ["amg_select_crop"] * n_crops and n_crops == 5, calls
    assert len(got) > 0
