"""CPU: tests/topk_reference.py (what the GPU tests of psam_topk_points compare against) and the host helpers of the device
top-k path, pinned against the reference's own lines.

  tie-free inputs   equal, in order, to `torch.topk(output_p_fg[mask], k)` + `torch.nonzero(mask)[indices]`
                    (models/ProtoSAM.py:266-289, restated in `_reference_lines`)
  tie-heavy inputs  the chosen probabilities equal torch.topk's values exactly; k = 1 is the component table's best pixel
  ops.decode_topk_keys and the dictionary ProtoSAM._topk_from_keys hands to _prompts_from_table
  injected faults   a wrong tie rule, a dropped pixel, a key of another component, a swap, a key beyond the area: none passes
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import topk_reference as tr
from oracle import ccl as occl

SHAPES = [(1, 1), (1, 300), (63, 65), (65, 257), (130, 190)]


def _tie_free(H, W, seed):
    """a seeded permutation of (i + 1) / (H*W + 1): distinct in fp32 for H*W < 2^24"""
    n = H * W
    v = (np.random.RandomState(seed).permutation(n).astype(np.float64) + 1.0) / (n + 1.0)
    p = v.astype(np.float32).reshape(H, W)
    assert np.unique(p).size == n
    return p


def _reference_lines(output_p_fg, mask, k):
    """ProtoSAM.get_most_conf_points' lines (models/ProtoSAM.py:281-283) -> (values, (y, x) locations)"""
    confidences, indices = torch.topk(output_p_fg[mask], k)
    locations = torch.nonzero(mask)[indices]
    return confidences, locations


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("pattern", ["full", "bars", "blobs", "noise41", "twins", "nested_uv"])
def test_tie_free_equals_reference_lines(pattern, H, W):
    pred, _, _ = occl.make_pattern(pattern, H, W, seed=1)
    pfg = _tie_free(H, W, seed=H * 1000 + W)
    n, lab = occl.label(pred)
    t_p, t_lab = torch.from_numpy(pfg), torch.from_numpy(lab)
    for k in (1, 3, 17):
        keys = tr.topk_keys(lab, pfg, n, k, max(n, 1))
        for c in range(n):
            mask = t_lab == c + 1
            area = int(mask.sum())
            pts = [tr.decode(v, W) for v in keys[c] if v]
            assert len(pts) == min(area, k) and not keys[c, len(pts):].any()
            if area >= k:
                conf, loc = _reference_lines(t_p, mask, k)
                assert [(x, y) for x, y, _ in pts] == [(int(x), int(y)) for y, x in loc.tolist()]
                assert [p for _, _, p in pts] == [float(v) for v in conf]


@pytest.mark.parametrize("pattern", occl.PATTERNS)
def test_tie_heavy_values_equal_topk(pattern):
    H, W = 65, 131
    pred, pfg, _ = occl.make_pattern(pattern, H, W, seed=2)
    n, lab, st = occl.ccl_reference(pred, pfg)
    t_p, t_lab = torch.from_numpy(pfg), torch.from_numpy(lab)
    k1 = tr.topk_keys(lab, pfg, n, 1, max(n, 1))
    for c in range(n):
        x, y, p = tr.decode(k1[c, 0], W)
        assert (x, y) == (int(st["best_x"][c]), int(st["best_y"][c])) and np.float32(p) == st["best_p"][c]
    for k in (3, 40):
        keys = tr.topk_keys(lab, pfg, n, k, max(n, 1))
        for c in range(n):
            vals = t_p[t_lab == c + 1]
            got = [tr.decode(v, W) for v in keys[c] if v]
            assert len(got) == min(k, vals.numel())
            want = torch.topk(vals, len(got)).values
            assert sorted((p for _, _, p in got), reverse=True) == [p for _, _, p in got] == [float(v) for v in want]
            # and the points belong to the component, each once
            assert len({(x, y) for x, y, _ in got}) == len(got) and all(lab[y, x] == c + 1 for x, y, _ in got)


def test_only_best_and_capacity_rows():
    H, W = 65, 131
    pred, pfg, _ = occl.make_pattern("noise20", H, W, seed=3)
    n, lab = occl.label(pred)
    assert n > 12
    full = tr.topk_keys(lab, pfg, n, 4, n)
    assert np.array_equal(tr.topk_keys(lab, pfg, n, 4, 5), full[:5])                 # n > max_comp: the first rows only
    cut = tr.topk_keys(np.where(lab > 7, 0, lab), pfg, 7, 4, 12)                    # a table of 7 components
    assert np.array_equal(cut[:7], full[:7]) and not cut[7:].any()
    assert np.array_equal(tr.topk_keys(lab, pfg, n, 4, 12, only_best=9), full[9:10])


def test_decode_topk_keys_and_prompt_dictionary():
    from protosam_amd import ops
    from protosam_amd.protosam import ProtoSAM
    S = 1024
    pts = [(5, 0, 1.0), (1023, 1023, 0.75), (0, 7, 0.75), (17, 300, 0.0)]      # p = 0 is a point, not an empty slot
    row = np.array([occl.point_key(p, y * S + x) for x, y, p in pts] + [0, 0], dtype=np.uint64)
    assert ops.decode_topk_keys(row.view(np.int64), S) == pts                  # the int64 view the device hands over
    assert ops.decode_topk_keys(row[:2], S) == pts[:2] and ops.decode_topk_keys(np.zeros(3, np.uint64), S) == []
    # the dictionary of _prompts_from_table: label -> float64 [k, 2] of (x, y), in the row's order
    tab = np.zeros(ops.CC_HDR + ops.CC_STRIDE * 4)
    tab[0] = tab[1] = 2
    tab[3] = 1
    tab[ops.CC_HDR:ops.CC_HDR + 12] = [9, 0, 0, 0, 0, 9, 9, 0.5, 5, 0, 1.0, 0]
    tab[ops.CC_HDR + 12:ops.CC_HDR + 24] = [2, 0, 0, 3, 4, 5, 6, 0.6, 17, 300, 0.5, 0]
    keys = np.stack([row[:4], np.roll(row[:4], 1)]).view(np.int64)
    me = SimpleNamespace(sam=SimpleNamespace(image_encoder=SimpleNamespace(img_size=S)), num_points_for_sam=4, use_cca=False,
                         use_points=True, use_neg_points=False, use_bbox=True, point_mode="conf")
    topk = ProtoSAM._topk_from_keys(me, keys, tab, [1, 2], plane=0)
    assert sorted(topk) == [1, 2] and topk[1].dtype == np.float64 and topk[1].shape == (4, 2)
    assert topk[1].tolist() == [[float(x), float(y)] for x, y, _ in pts] and topk[2][0].tolist() == [17.0, 300.0]
    coords, labels, rows = ProtoSAM._prompts_from_table(me, tab, None, topk)
    assert labels == [[1, 1, 1, 1, 2, 3]] * 2 and coords[0][:4] == topk[1].tolist() and coords[1][4:] == [[3.0, 4.0], [5.0, 6.0]]
    me.use_cca = True                                                           # one row: the kept component tab[3] = 1
    topk = ProtoSAM._topk_from_keys(me, keys[1:2], tab, [2], plane=0)
    coords, labels, rows = ProtoSAM._prompts_from_table(me, tab, None, topk)
    assert len(coords) == 1 and coords[0][:4] == topk[2].tolist()
    # a component of fewer than k pixels: the error names plane, component, area and k
    short = keys.copy()
    short[1, 2:] = 0
    me.use_cca = False
    with pytest.raises(RuntimeError, match=r"plane 7: component 1 has 2 pixels, fewer than num_points_for_sam = 4"):
        ProtoSAM._topk_from_keys(me, short, tab, [1, 2], plane=7)


# ---- injected faults: each one, put into a copy of the reference output, must fail the comparison helper ---------------------
def _fault_cases():
    """(name, labels, pfg, n, k): saturated and tie-heavy planes whose components are larger than k, and one with small ones"""
    out = []
    for pattern, (H, W), k in (("full", (67, 130), 5), ("bars", (65, 257), 7), ("blobs", (130, 190), 5), ("comb", (63, 65), 3),
                               ("twins", (65, 257), 4)):
        pred, pfg, _ = occl.make_pattern(pattern, H, W, seed=4)
        n, lab = occl.label(pred)
        out.append((pattern, lab, pfg, n, k))
        out.append((pattern + "-saturated", lab, np.ones_like(pfg), n, k))
    return out


FAULT_CASES = _fault_cases()
CASE_IDS = [c[0] for c in FAULT_CASES]


def _fails(bad, ref, W):
    assert tr.mismatches(ref.copy(), ref, W) == []            # (the helper passes the unchanged output)
    return bool(tr.mismatches(bad, ref, W))


@pytest.mark.parametrize("case", FAULT_CASES, ids=CASE_IDS)
def test_fault_tie_broken_by_last_index(case):
    _, lab, pfg, n, k = case
    ref = tr.topk_keys(lab, pfg, n, k, n)
    assert _fails(tr.topk_keys(lab, pfg, n, k, n, tie="last"), ref, lab.shape[1])


BOUNDARY_CASES = [c for c in FAULT_CASES if not c[0].startswith("twins")]    # (the twins' corners touch no 64-pixel boundary)


@pytest.mark.parametrize("case", BOUNDARY_CASES, ids=[c[0] for c in BOUNDARY_CASES])
def test_fault_pixel_dropped_at_lane_boundary(case):
    """a chosen pixel at a 64-pixel boundary of the raster (index % 64 in {63, 0}) is lost: its label reads 0. The probabilities
    are halved except on those boundaries, so that the chosen pixels lie there."""
    _, lab, pfg, n, k = case
    W = lab.shape[1]
    raster = np.arange(lab.size).reshape(lab.shape) % 64
    pfg = np.where((raster == 63) | (raster == 0), np.float32(1.0), pfg * np.float32(0.5)).astype(np.float32)
    ref = tr.topk_keys(lab, pfg, n, k, n)
    idx = (np.uint64(tr.U32) - (ref[ref != 0] & np.uint64(tr.U32))).astype(np.int64)
    edge = idx[(idx % 64 == 63) | (idx % 64 == 0)]
    assert edge.size, "the case has no chosen pixel on a 64-lane boundary"
    holed = lab.copy()
    holed.ravel()[edge[0]] = 0
    assert _fails(tr.topk_keys(holed, pfg, n, k, n), ref, W)


@pytest.mark.parametrize("case", [c for c in FAULT_CASES if c[3] >= 2], ids=[c[0] for c in FAULT_CASES if c[3] >= 2])
def test_fault_key_of_neighbouring_component(case):
    _, lab, pfg, n, k = case
    ref = tr.topk_keys(lab, pfg, n, k, n)
    bad = ref.copy()
    bad[0, k - 1] = ref[1, 0]
    bad[0] = np.sort(bad[0])[::-1]                             # (still in descending order)
    assert _fails(bad, ref, lab.shape[1])


@pytest.mark.parametrize("case", FAULT_CASES, ids=CASE_IDS)
def test_fault_adjacent_keys_swapped(case):
    _, lab, pfg, n, k = case
    ref = tr.topk_keys(lab, pfg, n, k, n)
    swapped = 0
    for c in range(n):
        filled = int((ref[c] != 0).sum())
        if filled < 2:                                         # (a one-pixel component has no pair)
            continue
        bad = ref.copy()
        bad[c, [filled - 2, filled - 1]] = ref[c, [filled - 1, filled - 2]]
        assert _fails(bad, ref, lab.shape[1])
        swapped += 1
    assert swapped


@pytest.mark.parametrize("case", FAULT_CASES, ids=CASE_IDS)
def test_fault_key_beyond_area(case):
    """asked for more keys than the smallest component has pixels: a non-zero key in a slot beyond `area`"""
    _, lab, pfg, n, _ = case
    area = np.bincount(lab.ravel())[1:]
    c = int(np.argmin(area))
    k = int(area[c]) + 2
    ref = tr.topk_keys(lab, pfg, n, k, n)
    assert ref[c, area[c] - 1] != 0 and not ref[c, area[c]:].any()
    bad = ref.copy()
    bad[c, area[c]] = ref[c, area[c] - 1] - np.uint64(1)       # the next raster index at the same probability
    assert _fails(bad, ref, lab.shape[1])
