"""GPU: the generator's crop layers on the device (csrc/amg_crops.hip; PSAM_AMG_CROPS=device and the batch entry points).
Kernel level: psam_amg_keep_planes, psam_amg_crops_nms and psam_mask_binarize_crops in guarded, garbage-filled buffers against
tests/amg_crops_reference.py and psam_mask_binarize_resized. Route level: the records of PSAM_AMG_CROPS=host, record for record
and mask for mask, on the synthetic ViT-B of synth_cases, without a wait per crop, through every batch entry point, and after a
forced pool overflow."""
import os

import numpy as np
import pytest
import torch

import amg_crops_reference as cr

pytestmark = pytest.mark.gpu

ENV = ("PSAM_AMG_RESIZE", "PSAM_AMG_SELECT", "PSAM_AMG_REGIONS", "PSAM_AMG_CROPS")
GARBAGE = -1234567


# ---- kernel level -----------------------------------------------------------------------------------------------------------------
def _guarded(rows, row_words, dtype, fill, dev):
    """-> (whole, inner): `inner` = rows 1 .. rows of a tensor of rows + 2 rows filled with `fill`"""
    whole = torch.full(((rows + 2) * row_words,), fill, dtype=dtype, device=dev)
    return whole, whole[row_words:(rows + 1) * row_words]


def _records_dev(r, cap, dev):
    """a crop's device record table of `cap` rows: the records, then garbage rows"""
    t = np.full((cap, cr.REC), GARBAGE, np.int32)
    t[:len(r)] = r
    return torch.from_numpy(t).to(dev)


@pytest.mark.parametrize("count,crop", [(0, 1), (5, 1), (8, 1), (3, 0), (0, 0)])
def test_keep_planes_copies_the_first_records(dev, count, crop):
    """cap = 5 records of which the device count says 0, 5 (= cap) or 8 (> cap: only cap were stored): exactly the planes and
    records of the first min(count, cap) rows arrive, at the rows the counter names; every other row, the guards around the pool
    and the merged table, and the counter words of other crops keep their garbage. 256 x 256 planes as in the generator."""
    from protosam_amd import ops
    IN, cap, pool_cap, ncrops, base0 = 256, 5, 9, 3, 2
    g = torch.Generator(device="cpu").manual_seed(count * 7 + crop)
    low = torch.randn((3, 4, IN, IN), generator=g).to(dev)
    rng = np.random.default_rng(count)
    r = cr._records(rng, rng.integers(0, 200, (cap, 4)), [0, 0, 0, 0])
    r[:, 1] = rng.permutation(12)[:cap]
    records, cnt = _records_dev(r, cap, dev), torch.tensor([count], dtype=torch.int32, device=dev)
    pool_whole, pool = _guarded(pool_cap, IN * IN, torch.float32, -7.5, dev)
    merged_whole, merged = _guarded(pool_cap, cr.CREC, torch.int32, GARBAGE, dev)
    bases = torch.tensor([GARBAGE, base0, GARBAGE, GARBAGE, GARBAGE], dtype=torch.int32, device=dev)
    ops.amg_keep_planes(low, records, cnt, crop, ncrops, (17, 31), pool.view(pool_cap, IN, IN), merged, bases[:ncrops + 1])
    k, base = min(count, cap), (0 if crop == 0 else base0)
    want_pool = torch.full((pool_cap + 2, IN, IN), -7.5, device=dev)
    want_pool[1 + base:1 + base + k] = low.view(-1, IN, IN)[torch.from_numpy(r[:k, 1].astype(np.int64)).to(dev)]
    assert torch.equal(pool_whole.view(pool_cap + 2, IN, IN), want_pool)
    want = np.full((pool_cap + 2, cr.CREC), GARBAGE, np.int32)
    want[1 + base:1 + base + k, :cr.REC] = r[:k]
    want[1 + base:1 + base + k, 5:9] += np.array([[17, 31, 17, 31]], dtype=np.int32)
    want[1 + base:1 + base + k, cr.REC] = crop
    want[1 + base:1 + base + k, cr.REC + 1] = base + np.arange(k)
    assert np.array_equal(merged_whole.cpu().numpy().reshape(-1, cr.CREC), want)
    want_bases = [GARBAGE, base0, GARBAGE, GARBAGE, GARBAGE]
    want_bases[crop + 1] = base + k
    if crop == 0:
        want_bases[0] = 0
    assert bases.cpu().tolist() == want_bases


def _run_crops(dev, per_crop, crop_boxes, thr, pool_cap, IN=4, low_planes=16, spare=2):
    """keep_planes per crop, then crops_nms, all in guarded buffers -> (final table [m, CREC] or None on overflow, total, pool, low)"""
    from protosam_amd import ops
    ncrops = len(crop_boxes)
    low = torch.arange(low_planes * IN * IN, dtype=torch.float32, device=dev).view(low_planes // 4, 4, IN, IN)
    pool_whole, pool = _guarded(pool_cap, IN * IN, torch.float32, -7.5, dev)
    merged_whole, merged = _guarded(pool_cap, cr.CREC, torch.int32, GARBAGE, dev)
    out_whole = torch.full((pool_cap * cr.CREC + 2 + 8,), GARBAGE, dtype=torch.int32, device=dev)
    bases = torch.full((ncrops + 1 + 4,), GARBAGE, dtype=torch.int32, device=dev)
    for c, (r, cb) in enumerate(zip(per_crop, crop_boxes)):
        cap = len(r) + spare
        ops.amg_keep_planes(low, _records_dev(r, cap, dev), torch.tensor([len(r)], dtype=torch.int32, device=dev), c, ncrops,
                            (cb[0], cb[1]), pool.view(pool_cap, IN, IN), merged, bases[:ncrops + 1])
    geom = torch.from_numpy(ops.amg_crop_geometry(crop_boxes, [(8, 8)] * ncrops)).to(dev)
    ops.amg_crops_nms(merged, bases[:ncrops + 1], geom, ncrops, pool_cap, thr, use_nms=ncrops > 1, out=out_whole[4:4 + pool_cap * cr.CREC + 2])
    host = out_whole.cpu().numpy()
    assert (host[:4] == GARBAGE).all() and (host[-4:] == GARBAGE).all() and (bases[ncrops + 1:].cpu().numpy() == GARBAGE).all()
    pw = pool_whole.view(pool_cap + 2, IN * IN)
    mw = merged_whole.view(pool_cap + 2, cr.CREC)
    assert bool((pw[0] == -7.5).all()) and bool((pw[-1] == -7.5).all()) and bool((mw[0] == GARBAGE).all()) and bool((mw[-1] == GARBAGE).all())
    m, total = int(host[4 + pool_cap * cr.CREC]), int(host[4 + pool_cap * cr.CREC + 1])
    final = None if m < 0 else host[4:4 + m * cr.CREC].reshape(m, cr.CREC)
    return final, total, pw[1:-1], low.view(low_planes, IN * IN), mw[1:-1]


@pytest.mark.parametrize("total", [63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("kind", cr.KINDS)
def test_crops_nms_equals_reference(dev, kind, total):
    """The merged table behind keep_planes over all crops and the final table of crops_nms against the NumPy reference, word for
    word: equal scores inside a crop and between crops, IoU exactly at the threshold, empty crops, a first crop without records,
    a single crop box (no NMS), at merged sizes on both sides of 64 and 256. The pool holds each merged record's plane."""
    c = cr.case(kind, total, seed=total)
    for r in c["per_crop"]:
        r[:, 1] %= 16
    pool_cap = total if total % 2 else total + 3               # a pool that is exactly full, and one with room
    final, got_total, pool, low, merged = _run_crops(dev, c["per_crop"], c["crop_boxes"], c["thr"], pool_cap)
    assert got_total == total and final is not None
    ref_merged = cr.merged_reference(c["per_crop"], c["crop_boxes"])
    assert np.array_equal(merged[:total].cpu().numpy(), ref_merged)
    assert torch.equal(pool[:total], low[torch.from_numpy(ref_merged[:, 1].astype(np.int64)).to(dev)])
    assert bool((pool[total:] == -7.5).all())
    cr.same_final(final, cr.final_reference(c["per_crop"], c["crop_boxes"], c["thr"]))


def test_pool_overflow_is_reported_and_writes_nothing(dev):
    """Two crops of 3 records into a pool of 4 rows: rows 0 .. 3 are written, nothing past the pool or the merged table (the guards
    of `_run_crops`), the counter goes on to 6 and the final table says -1. One record too many does the same; a full pool is fine."""
    c = cr.case("clustered", 6, seed=1)
    per_crop = [np.concatenate(c["per_crop"][:3])[:3], np.concatenate(c["per_crop"][:3])[3:6]]
    for r in per_crop:
        r[:, 1] %= 16
    boxes = c["crop_boxes"][:2]
    for pool_cap, over in ((4, True), (5, True), (6, False)):
        final, total, pool, low, merged = _run_crops(dev, per_crop, boxes, 0.7, pool_cap)
        assert total == 6 and (final is None) == over
        ref = cr.merged_reference(per_crop, boxes)[:pool_cap]
        assert np.array_equal(merged.cpu().numpy()[:len(ref)], ref)
        assert torch.equal(pool[:len(ref)], low[torch.from_numpy(ref[:, 1].astype(np.int64)).to(dev)])
    from protosam_amd import ops
    with pytest.raises(ValueError, match="group limit"):
        ops.amg_crops_nms(merged, torch.zeros(3, dtype=torch.int32, device=dev), torch.zeros(16, dtype=torch.int32, device=dev), 2,
                          ops.NMS_MAX_GROUP + 1, 0.7)


# frame (H, W), IN, MID, geometries (x0, y0, cw, ch, ih, iw): the whole frame, crops at the origin and at the far edge, an odd one;
# in_size == crop size in one of them
BINARIZE = {
    "48x44": ((48, 44), 16, 64, [(0, 0, 44, 48, 48, 44), (14, 16, 30, 32, 64, 60), (0, 0, 30, 32, 64, 60), (7, 5, 21, 17, 52, 64)]),
    "225x300": ((225, 300), 256, 1024, [(0, 0, 300, 225, 768, 1024), (99, 75, 201, 150, 764, 1024), (0, 0, 120, 100, 100, 120),
                                        (0, 75, 201, 150, 764, 1024)]),
}


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("name", list(BINARIZE))
def test_binarize_crops_equals_binarize_resized(dev, name, variant):
    """ONE launch over records of four crop geometries (one with in_size == crop size, origins at 0 and at the far edge) equals
    mask_binarize_resized(origin=...) of every record into a zeroed frame, bit for bit; every byte of the garbage-filled output is
    written, the guard frames are not; a record whose crop index is out of range gives a zero frame."""
    from protosam_amd import ops
    (H, W), IN, MID, geoms = BINARIZE[name]
    pool_cap, ncrops = 8, len(geoms)
    g = torch.Generator(device="cpu").manual_seed(variant)
    pool = (torch.randn((pool_cap, IN, IN), generator=g) * 2.0).to(dev)
    geom = np.zeros((ncrops, ops.AMG_GEOM), np.int32)
    geom[:, :6] = geoms
    geom_d = torch.from_numpy(geom).to(dev)
    picks = [(0, 3), (1, 0), (2, 5), (3, 1), (1, 2), (0, 4), (-1, 0), (2, 0)]          # (crop, pool row) of the final records
    m = len(picks)
    final = np.full((m + 1, cr.CREC), GARBAGE, np.int32)
    final[:m, cr.REC:] = picks
    whole = torch.full((m + 2, H, W), 0xAB, dtype=torch.uint8, device=dev)
    ops.mask_binarize_crops(pool, torch.from_numpy(final).to(dev).view(-1), m, geom_d, ncrops, MID, (H, W), variant, thr=0.25, out=whole[1:-1])
    assert bool((whole[0] == 0xAB).all()) and bool((whole[-1] == 0xAB).all())
    n_set = 0
    for i, (c, row) in enumerate(picks):
        want = torch.zeros((1, H, W), dtype=torch.uint8, device=dev)
        if c >= 0:
            x0, y0, cw, ch, ih, iw = geoms[c]
            ops.mask_binarize_resized(pool, torch.tensor([row], dtype=torch.int32, device=dev), MID, (ih, iw), (ch, cw), variant, thr=0.25,
                                      out=want, origin=(y0, x0))
        assert torch.equal(whole[1 + i], want[0]), (i, c, row)
        n_set += int(want.sum())
    assert 0 < n_set < m * H * W


# ---- route level ------------------------------------------------------------------------------------------------------------------
def _image(h, w, seed):
    """a smooth random uint8 image [h, w, 3] with a few rectangles (the 225 x 300 image of test_amg_regions_gpu.py: seed 1)"""
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
    return dict(w=w, images={"48x44": gi.amg_small_case(), "225x300": _image(225, 300, 1), "57x51": _image(57, 51, 2)}, cache={})


def _generator(s, crops="host", **kw):
    """a generator over the shared model; the switches are read when it is built"""
    from protosam_amd.segment_anything import SamAutomaticMaskGenerator
    old = {k: os.environ.get(k) for k in ENV}
    os.environ.update(PSAM_AMG_RESIZE="fused", PSAM_AMG_SELECT="host", PSAM_AMG_REGIONS="device", PSAM_AMG_CROPS=crops)
    try:
        g = SamAutomaticMaskGenerator(s["w"].sam, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    assert g.amg_crops == crops and g.amg_regions == "device" and g.amg_resize == "fused"
    return g


def _host_records(s, name, **kw):
    """the records of PSAM_AMG_CROPS=host, once per (image, arguments)"""
    key = (name, tuple(sorted(kw.items())))
    if key not in s["cache"]:
        s["cache"][key] = _generator(s, **kw).generate(s["images"][name])
    return s["cache"][key]


def _same_records(a, b):
    """masks (or their RLEs), boxes, areas, scores, points, crop boxes and order"""
    assert len(a) == len(b), (len(a), len(b))
    for x, y in zip(a, b):
        assert set(x) == set(y)
        for k in x:
            if isinstance(x[k], np.ndarray):
                assert x[k].dtype == y[k].dtype == bool and np.array_equal(x[k], y[k])
            else:
                assert x[k] == y[k] and type(x[k]) is type(y[k]), (k, x[k], y[k])


def _wrap(obj, name, calls):
    inner = getattr(obj, name)
    setattr(obj, name, lambda *a, **k: (calls.append(name), inner(*a, **k))[1])


def _host_route_guards(g):
    """-> calls: filled when the generator enters the per-crop host code"""
    calls = []
    for name in ("_crops_host", "_process_crop", "_crop_fused", "_crop_select_device"):
        _wrap(g, name, calls)
    return calls


ROUTE_SETTINGS = {"crop_args": dict(), "no_crop_nms": dict(crop_nms_thresh=1.0), "area0": dict(min_mask_region_area=0),
                  "area0_no_crop_nms": dict(min_mask_region_area=0, crop_nms_thresh=1.0),
                  "rle": dict(output_mode="uncompressed_rle"), "rle_area0": dict(output_mode="uncompressed_rle", min_mask_region_area=0),
                  "layers2": dict(crop_n_layers=2)}


# (the 21 crops of two layers: on the small image only)
ROUTE_CASES = [(n, s) for n in ("48x44", "225x300") for s in ROUTE_SETTINGS if not (s == "layers2" and n != "48x44")]
ROUTE_CASES += [("57x51", "crop_args"), ("57x51", "area0_no_crop_nms")]


@pytest.mark.parametrize("name,setting", ROUTE_CASES)
def test_device_crops_equal_host_crops(dev, setup, name, setting):
    """AMG_CROP_ARGS and its variants: PSAM_AMG_CROPS=device returns the records of PSAM_AMG_CROPS=host and never enters the
    per-crop host code. With AMG_CROP_ARGS' thresholds (every candidate passes the score filters) the cross-crop NMS at 0.7
    removes records of every image, which the *_no_crop_nms settings show. Every case on the 48 x 44 and the 57 x 51 image has
    records of layer-1 crops. The 225 x 300 image has none, at any thresholds: the synthetic weights give noise-like masks that
    span their crop, so every candidate of its layer-1 crops has a box edge at a crop edge more than 20 pixels from the image's
    edge and the crop-edge filter drops it (the CPU oracle, oracle/amg.py, with the score filters off and no NMS: 192 records at
    8 points per side and 768 at 16, with crop_n_points_downscale_factor 1 or 2 and crop_overlap_ratio 512/1500 or 0.9, every one
    from the layer-0 crop). There the route runs four crops that end empty behind a full first one; the 57 x 51 image (layer-1
    crops of 37 x 34, every crop edge within 20 pixels of the image's) is here to have crop records at a second, odd size.
    output_mode "coco_rle" needs pycocotools at construction; its string is coco_encode_rle of the "uncompressed_rle" records."""
    from protosam_amd import synth_cases as gi
    kw = dict(gi.AMG_CROP_ARGS, **ROUTE_SETTINGS[setting])
    ref = _host_records(setup, name, **kw)
    g = _generator(setup, crops="device", **kw)
    calls = _host_route_guards(g)
    got = g.generate(setup["images"][name])
    _same_records(got, ref)
    assert calls == [], calls
    h, w = setup["images"][name].shape[:2]
    n_crop = sum(1 for a in got if a["crop_box"] != [0, 0, w, h])
    print(f"{name} {setting}: {len(got)} records, {n_crop} from crops of layer >= 1")
    assert len(got) >= 1
    if name != "225x300":
        assert n_crop >= 1
    if setting in ("crop_args", "area0"):                  # the cross-crop NMS removed something
        every = _host_records(setup, name, **dict(kw, crop_nms_thresh=1.0))
        assert len(ref) < len(every), (len(ref), len(every))
    if setting == "rle":
        from protosam_amd.segment_anything.utils.amg import coco_encode_rle
        assert [coco_encode_rle(a["segmentation"]) for a in got] == [coco_encode_rle(a["segmentation"]) for a in ref]


@pytest.mark.parametrize("regions", [6, 0])
def test_one_record_copy_per_image(dev, setup, regions):
    """Device-to-host copies of int32 tables (statistics, records, decisions) during `generate`: the device route makes ONE for
    the image's final table, plus one for the small-region stage; the host route makes at least one per crop."""
    from protosam_amd import synth_cases as gi
    kw = dict(gi.AMG_CROP_ARGS, min_mask_region_area=regions)
    seen = {}
    inner = torch.Tensor.cpu

    def counting(t, *a, **k):
        if t.is_cuda and t.dtype == torch.int32:
            seen["n"] = seen.get("n", 0) + 1
        return inner(t, *a, **k)

    counts = {}
    for crops in ("device", "host"):
        g = _generator(setup, crops=crops, **kw)
        seen.clear()
        torch.Tensor.cpu = counting
        try:
            got = g.generate(setup["images"]["48x44"])
        finally:
            torch.Tensor.cpu = inner
        counts[crops] = seen.get("n", 0)
        assert len(got) > 0
    print(f"int32 downloads, min_mask_region_area={regions}: {counts}")
    assert counts["device"] == 1 + (1 if regions else 0) and counts["host"] >= 5 + (1 if regions else 0)


def test_generate_batch_takes_the_device_route(dev, setup):
    """generate_batch([a, b, a]) with crop layers on and mixed sizes equals [generate(x) ...] of the host route; every image goes
    through `_crops_enqueue`, none through the fallback or the per-crop host code."""
    from protosam_amd import synth_cases as gi
    a, b = setup["images"]["48x44"], setup["images"]["225x300"]
    g = _generator(setup, crops="host", **gi.AMG_CROP_ARGS)           # the batch entry points take the device route whatever it says
    calls = _host_route_guards(g)
    enq = []
    _wrap(g, "_crops_enqueue", enq)
    _wrap(g, "generate", calls)
    got = g.generate_batch([a, b, a])
    assert calls == [] and len(enq) == 3, (calls, enq)
    refs = [_host_records(setup, n, **gi.AMG_CROP_ARGS) for n in ("48x44", "225x300", "48x44")]
    for x, y in zip(got, refs):
        _same_records(x, y)
    assert all(len(x) > 0 for x in got)


def test_generate_device_batch_with_labels(dev, setup):
    """generate_device_batch with labels: the candidates, masks and {tp, fp, fn} of generate_device on the host route."""
    from protosam_amd import synth_cases as gi
    names = ("225x300", "48x44", "48x44")
    images = [setup["images"][n] for n in names]
    rng = np.random.RandomState(3)
    labels = [torch.from_numpy((rng.rand(*im.shape[:2]) > 0.6).astype(np.uint8)).to(dev) for im in images]
    labels[1] = None
    host = _generator(setup, crops="host", **gi.AMG_CROP_ARGS)
    refs = [host.generate_device(im, lb) for im, lb in zip(images, labels)]
    g = _generator(setup, crops="host", **gi.AMG_CROP_ARGS)
    calls = _host_route_guards(g)
    _wrap(g, "generate_device", calls)
    got = g.generate_device_batch(images, labels)
    assert calls == [], calls
    for (cd, md, kd), (ch, mh, kh) in zip(got, refs):
        assert set(cd) == set(ch) and cd["size"] == ch["size"]
        for k in cd:
            if k != "size":
                assert np.array_equal(cd[k], ch[k]), k
        assert torch.equal(md, mh) and md.shape[0] > 0
        assert (kd is None and kh is None) or torch.equal(kd, kh)
    assert got[1][2] is None and got[0][2].shape == (got[0][1].shape[0], 3)


def test_forward_batch_picks_forwards_mask(dev, setup):
    """SamWrapper.forward_batch with crop layers goes through generate_device_batch (the device route) and picks the mask that
    forward picks on the host route."""
    from protosam_amd import synth_cases as gi
    w = setup["w"]
    a = setup["images"]["48x44"]
    images = [a, np.ascontiguousarray(a[:, ::-1])]
    rng = np.random.RandomState(5)
    labels = [(rng.rand(*w.transform.apply_image(im).shape[:2]) > 0.5).astype(np.uint8) for im in images]
    old = w.mask_generator
    try:
        w.mask_generator = _generator(setup, crops="host", **gi.AMG_CROP_ARGS)
        refs = []
        for im, lb in zip(images, labels):
            refs.append((w.forward(im, lb), w.last_stats["best_index"], w.last_stats["n_masks"]))
        w.mask_generator = g = _generator(setup, crops="host", **gi.AMG_CROP_ARGS)
        calls = _host_route_guards(g)
        _wrap(g, "generate_device", calls)
        enq = []
        _wrap(g, "_crops_enqueue", enq)
        got = w.forward_batch(images, labels)
        stats = w.last_stats
    finally:
        w.mask_generator = old
    assert calls == [] and len(enq) == 2, (calls, enq)
    for b, (mask, best, n) in enumerate(refs):
        assert got[b].dtype == bool and np.array_equal(got[b], mask)
        assert stats[b]["best_index"] == best and stats[b]["n_masks"] == n > 0


def test_forced_overflow_falls_back(dev, setup):
    """crop_pool_cap=7 (an argument) is far below the 384 per-crop survivors of AMG_CROP_ARGS: the device reports the overflow,
    `generate` and `generate_batch` take the host route for that image and return its records."""
    from protosam_amd import synth_cases as gi
    ref = _host_records(setup, "48x44", **gi.AMG_CROP_ARGS)
    g = _generator(setup, crops="device", crop_pool_cap=7, **gi.AMG_CROP_ARGS)
    calls = []
    _wrap(g, "_crops_host", calls)
    _wrap(g, "_crops_enqueue", calls)
    _same_records(g.generate(setup["images"]["48x44"]), ref)
    assert calls == ["_crops_enqueue", "_crops_host"], calls
    del calls[:]
    got = g.generate_batch([setup["images"]["48x44"]] * 2)
    assert calls == ["_crops_enqueue", "_crops_enqueue", "_crops_host", "_crops_host"], calls
    for x in got:
        _same_records(x, ref)
