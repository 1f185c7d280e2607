"""CPU: the numpy contract of psam_small_regions / ops.small_regions_select (tests/small_regions_reference.py) is the reference's
remove_small_regions twice, the integer crop-edge rule of psam_amg_select_crop is utils.amg.is_box_near_crop_edge, and the shared
patterns tell single injected mistakes from the contract. Host-side argument checks of the wrappers. No GPU."""
import numpy as np
import pytest
import torch

import small_regions_reference as sr


def _oracle(mask, t):
    """remove_small_regions(mask, t, "holes") then (., t, "islands") as oracle/amg.py:125-140 restates it"""
    from oracle.amg import remove_small_regions
    m, ch = remove_small_regions(np.asarray(mask) != 0, t, "holes")
    m, ci = remove_small_regions(m, t, "islands")
    return np.asarray(m).astype(np.uint8), bool(ch), bool(ci)


@pytest.mark.parametrize("shape", sr.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_is_the_oracle(shape):
    """Every pattern at every threshold: mask, both flags, and area / box / score as the generator derives them."""
    names, masks = sr.pattern_batch(*shape)
    assert {"empty", "full", "checker", "comb", "runs", "border_holes", "small_background", "random0.05", "random0.8"} <= set(names)
    changed = 0
    for t in sr.THRESHOLDS:
        out, boxes, scores, info = sr.batch(masks, t)
        for i, name in enumerate(names):
            want, ch, ci = _oracle(masks[i], t)
            what = f"{shape} {name} t={t}"
            assert np.array_equal(out[i], want), what
            assert info[i].tolist() == [int(ch), int(ci), int(want.sum()), 0], what
            assert scores[i] == float(not ch and not ci), what
            ys, xs = np.nonzero(want)
            assert boxes[i].tolist() == ([xs.min(), ys.min(), xs.max(), ys.max()] if len(ys) else [0, 0, 0, 0]), what
            if not (ch or ci):
                assert np.array_equal(out[i], (masks[i] != 0).astype(np.uint8)), what
            changed += ch or ci
    print(f"{shape}: {len(names)} patterns x {len(sr.THRESHOLDS)} thresholds, {changed} changed")
    if shape != (1, 1):
        assert changed > 0


def test_patterns_hold_what_they_promise():
    """The spiral is ONE region whose complement is one region too, under 4-connectivity as well; the checkerboard is one region
    under 8- and H * W / 2 under 4-connectivity; the rings' holes have exactly k pixels; the tie patterns have two equal largest."""
    s = sr.spiral(129) != 0
    for fg in (s, ~s):
        for conn4 in (False, True):
            assert len(np.unique(sr.label_roots(fg, conn4)[fg])) == 1
    assert 0.45 < s.mean() < 0.55
    assert int(sr.label_roots(s)[s].max()) == 0 and int((s.sum(0) == 1).sum() + (s.sum(1) == 1).sum()) <= 4
    P = sr.patterns(48, 44)
    c = P["checker"] != 0
    assert len(np.unique(sr.label_roots(c)[c])) == 1 and len(np.unique(sr.label_roots(~c)[~c])) == 1
    assert len(np.unique(sr.label_roots(c, True)[c])) == c.sum()
    for k in (1, 5, 6, 49, 50):
        m = P[f"ring{k}"] != 0
        roots = sr.label_roots(~m)
        _, counts = np.unique(roots[roots >= 0], return_counts=True)
        assert sorted(counts.tolist())[0] == k and len(counts) == 2
    for name, a in (("tie", 4), ("tie5", 5)):
        m = P[name] != 0
        _, counts = np.unique(sr.label_roots(m)[m], return_counts=True)
        assert sorted(counts.tolist())[-2:] == [a, a]
    x = sr.patterns(65, 257)["runs"]
    for xb in (64, 128, 256):
        assert bool((x[:, xb - 1] != 0).any() and ((x[:, xb - 1] != 0) & (x[:, xb] != 0)).any())


# where each mistake must show: (shape, pattern, threshold)
FAULT_CASES = {"conn4": ((48, 44), "checker", 6), "le": ((48, 44), "ring6", 6), "islands_on_unfilled": ((48, 44), "thin_ring", 50),
               "tie_last": ((48, 44), "tie", 6), "keep_largest_unflagged": ((48, 44), "tie", 6),
               "sentinel_box": ((48, 44), "empty", 6)}


@pytest.mark.parametrize("fault", sr.FAULTS)
def test_reference_catches_injected_faults(fault):
    """4-connectivity, <= at the threshold, islands of the unfilled mask, the last of two equal largest, changed_islands left clear
    in the keep-largest case, min / max sentinels as an empty mask's box: each changes the result of its pattern."""
    shape, name, t = FAULT_CASES[fault]
    P = sr.patterns(*shape)
    good = sr.batch(P[name][None], t)
    bad = sr.batch(P[name][None], t, frozenset([fault]))
    differ = [k for k, (a, b) in enumerate(zip(good, bad)) if not np.array_equal(a, b)]
    assert differ, f"{fault}: {name} at t={t} does not show it"
    # and across all patterns of the shape the fault shows in more than that one place or exactly there - never nowhere
    names, masks = sr.pattern_batch(*shape)
    hits = 0
    for tt in sr.THRESHOLDS:
        a, b = sr.batch(masks, tt), sr.batch(masks, tt, frozenset([fault]))
        hits += sum(1 for i in range(len(names)) if any(not np.array_equal(x[i], y[i]) for x, y in zip(a, b)))
    print(f"{fault}: outputs {differ} differ on {name}; {hits} (pattern, threshold) pairs of {shape} show it")
    assert hits >= 1


def test_ring_threshold_is_strict():
    """A hole of exactly t pixels stays, one of t - 1 is filled; with t = 5.5 the hole of 5 goes and the hole of 6 stays."""
    P = sr.patterns(48, 44)
    for t, stays, goes in ((6, "ring6", "ring5"), (50, "ring50", "ring49"), (5.5, "ring6", "ring5")):
        out, _, scores, info = sr.batch(np.stack([P[stays], P[goes]]), t)
        assert info[:, 0].tolist() == [0, 1] and scores.tolist() == [1.0, 0.0]
        assert np.array_equal(out[0], P[stays]) and int(out[1].sum()) == int(P[goes].sum()) + (t - 1 if t != 5.5 else 5)


def test_crop_edge_rule_is_the_host_rule():
    """Boxes with one edge at distance 19, 20 and 21 from each crop edge and each image edge, inside and outside, for crops in a
    corner, on an edge and in the middle of the image: the integer rule equals utils.amg.is_box_near_crop_edge. Empty masks use
    the [0, 0, 0, 0] box."""
    from protosam_amd.segment_anything.utils.amg import is_box_near_crop_edge
    W, H = 400, 300
    orig = [0, 0, W, H]
    n = 0
    for crop in ([0, 0, 250, 200], [150, 100, 400, 300], [100, 60, 330, 250], [0, 60, 400, 250], [0, 0, 400, 300], [10, 15, 390, 290],
                 [21, 20, 379, 281]):
        x0, y0, x1, y1 = crop
        cw, ch = x1 - x0, y1 - y0
        boxes = [[0, 0, 0, 0], [cw // 2 - 5, ch // 2 - 5, cw // 2 + 5, ch // 2 + 5]]
        for d in (19, 20, 21):
            for s in (-1, 1):
                for k in range(4):
                    # edge k at distance d (signed) from the crop's edge k, and from the image's edge k, in the crop's frame
                    for target in (crop[k] - crop[k % 2], orig[k] - crop[k % 2]):
                        b = [cw // 2 - 5, ch // 2 - 5, cw // 2 + 5, ch // 2 + 5]
                        b[k] = target + s * d
                        boxes.append(b)
        boxes = np.array(boxes, dtype=np.int64)
        want = is_box_near_crop_edge(boxes, crop, orig)
        got = sr.near_crop_edge(boxes, crop, orig)
        assert np.array_equal(got, want), (crop, boxes[got != want])
        assert crop == orig or (want.any() and not want.all())
        n += len(boxes)
    print(f"{n} boxes")


def test_select_reference_order():
    """Unchanged masks (score 1) are visited before changed ones (score 0), each group in index order; coinciding boxes leave the
    first."""
    P = sr.patterns(48, 44)
    masks = np.stack([P["ring5"], P["ring50"], P["ring5"], P["ring50"], P["blob_speckle"], P["empty"], P["empty"]])
    out, kept, info, boxes = sr.select(masks, 6, 0.7)
    assert info[:, 0].tolist()[:4] == [1, 0, 1, 0]
    assert kept.tolist()[:1] == [1] and 3 not in kept.tolist() and 2 not in kept.tolist()
    assert 5 in kept.tolist() and 6 in kept.tolist()            # two empty boxes: 0 / 0 suppresses nothing


def test_wrappers_check_their_arguments_on_the_host():
    from protosam_amd import ops
    with pytest.raises(RuntimeError):
        ops.small_regions(torch.zeros((1, 4, 4), dtype=torch.uint8), 6)
    with pytest.raises(RuntimeError):
        ops.small_regions_select(torch.zeros((1, 4, 4), dtype=torch.uint8), 6, 0.7)
    with pytest.raises(TypeError):
        ops.small_regions(None, 6)
    with pytest.raises(RuntimeError):
        ops.amg_select_crop(torch.zeros((3, 8), dtype=torch.int32), torch.zeros((1, 4)), (0, 3), 0.0, 0.0, 0.7, [0, 0, 4, 4], [0, 0, 8, 8])


def test_working_set_follows_the_byte_budget():
    """300 masks of 1024 x 1024 stay inside the 256 MiB budget (not 2.4 GB); at least one mask is always in flight; the library's
    workspace size is chunk * (8 * H * W + 64) and refuses what the entry refuses."""
    from protosam_amd import _lib, ops
    c = ops.small_regions_chunk(300, 1024, 1024)
    assert 1 <= c < 300 and ops.small_regions_workspace(1024, 1024, c) <= ops.SMALL_REGIONS_BUDGET == 256 << 20
    assert ops.small_regions_workspace(1024, 1024, c + 1) > ops.SMALL_REGIONS_BUDGET
    assert ops.small_regions_chunk(5, 48, 44) == 5 and ops.small_regions_chunk(0, 48, 44) == 1
    assert ops.small_regions_chunk(10, 8192, 8192) == 1
    assert ops.small_regions_workspace(33, 17, 4) == 4 * (8 * 33 * 17 + 64)
    b = _lib.c_longlong(-7)
    for H, W, chunk in ((0, 4, 1), (4, 0, 1), (-1, 4, 1), (4, 4, 0), (65536, 32768, 1)):
        assert _lib.lib().psam_small_regions_workspace(H, W, chunk, b) == 1 and b.value == -7
    assert _lib.lib().psam_small_regions_workspace(4, 4, 1, None) == 1
