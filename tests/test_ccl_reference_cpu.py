"""Pins the vectorised connected-components reference (oracle/ccl.py) to the loop oracles of oracle/glue.py on small
versions of every adversarial pattern: labels, statistics, most confident points, confidences and negative points."""
import numpy as np
import pytest
import torch

from oracle import ccl as oc
from oracle import glue

SHAPES = [(1, 1), (1, 9), (9, 1), (23, 37), (40, 70)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", oc.PATTERNS)
def test_table_matches_glue(name, shape):
    pred, pfg, _ = oc.make_pattern(name, *shape)
    n, lab, st = oc.ccl_reference(pred, pfg)
    n_g, lab_g, stats, cent = glue.connected_components_with_stats(pred)
    assert n == n_g - 1 and np.array_equal(lab, lab_g)
    s = stats[1:].astype(np.int64)
    assert np.array_equal(st["area"], s[:, 4])
    assert np.array_equal(st["min_x"], s[:, 0]) and np.array_equal(st["min_y"], s[:, 1])
    assert np.array_equal(st["max_x"], s[:, 0] + s[:, 2] - 1) and np.array_equal(st["max_y"], s[:, 1] + s[:, 3] - 1)
    assert np.array_equal(st["sum_x"] / st["area"], cent[1:, 0]) and np.array_equal(st["sum_y"] / st["area"], cent[1:, 1])
    for k in range(n):
        m = lab_g == k + 1
        pt, conf = glue.most_conf_point(pfg, m)
        assert (st["best_x"][k], st["best_y"][k]) == (pt[0, 0], pt[0, 1]) and st["best_p"][k] == np.float32(conf[0])
        assert st["first"][k] == np.flatnonzero(m)[0]
        # p_fg is a multiple of 1/8: both sums are exact, so the quotients agree to the last bit
        assert st["conf"][k] == (pfg.astype(np.float64) * m).sum() / (pred.sum() + 1e-6)
    rows = oc.table_rows(st)
    assert rows.shape == (n, 12) and np.array_equal(rows[:, 0], st["area"]) and np.array_equal(rows[:, 7], st["conf"])
    if n:
        assert np.all(np.diff(st["first"]) > 0)   # numbered by raster order of the first pixel


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", oc.PATTERNS)
def test_neg_points_match_glue(name, shape):
    """r = 10, thr = 0.95: the restated ProtoSAM ring and global negative points."""
    H, W = shape
    pred, pfg, pbg = oc.make_pattern(name, H, W)
    n, lab, st = oc.ccl_reference(pred, pfg)
    keys = oc.neg_point_keys(lab, st, pbg, 10, 0.95, n + 2)
    assert np.all(keys[n + 1:] == 0)
    ref = glue.sam_neg_points((n + 1, lab, None, None), torch.from_numpy(np.stack([pbg, pfg])[None]))
    assert len(ref) == n
    glob = oc.decode_key(keys[0], W)
    if glob is not None:
        assert glob[2] == pbg[glob[1], glob[0]] >= 0.95
    for k in range(n):
        got = [p for p in (oc.decode_key(keys[1 + k], W), glob) if p is not None]
        exp = [] if ref[k] is None else [tuple(int(v) for v in e) for e in ref[k]]
        assert [(g[0], g[1]) for g in got] == exp, (k, got, exp)
        for g in got:
            assert g[2] == pbg[g[1], g[0]]


@pytest.mark.parametrize("r", [0, 1, 3])
@pytest.mark.parametrize("name", ["blobs", "twins", "noise20", "spiral", "full"])
def test_neg_points_general_r_and_thr(name, r):
    """Other ring radii (r iterations of glue.dilate3x3) and thresholds met exactly (inclusive)."""
    H, W = 23, 37
    pred, pfg, pbg = oc.make_pattern(name, H, W, seed=3)
    n, lab, st = oc.ccl_reference(pred, pfg)
    for thr in (0.75, 1.0):
        keys = oc.neg_point_keys(lab, st, pbg, r, thr, n)
        exp = glue.first_argmax_point(pbg, pbg >= thr)
        glob = oc.decode_key(keys[0], W)
        assert (glob is None) == (exp is None) and (glob is None or glob[:2] == tuple(exp[0]))
        for k in range(n):
            comp = ((lab == k + 1) * 255).astype(np.uint8)
            ring = (glue.dilate3x3(comp, r) > 0) & (comp == 0)
            exp = glue.first_argmax_point(pbg, ring)
            got = oc.decode_key(keys[1 + k], W)
            assert (got is None) == (exp is None) and (got is None or got[:2] == tuple(exp[0])), (k, got, exp)


def test_pattern_properties():
    """The patterns are what their names say at the shapes the GPU tests use."""
    for H, W in ((1, 300), (64, 64), (300, 517)):
        n = lambda name: oc.label(oc.make_pattern(name, H, W)[0])[0]  # noqa: E731
        assert n("empty") == 0 and n("full") == 1 and n("lattice") == ((H + 1) // 2) * ((W + 1) // 2)
        assert n("checker") == (1 if H > 1 else (W + 1) // 2)
        assert n("comb") == 1 and n("spiral") == 1
    pred, pfg, _ = oc.make_pattern("twins", 63, 65)
    n, lab, st = oc.ccl_reference(pred, pfg)
    assert n == 2 and st["conf"][0] == st["conf"][1] and st["area"][0] == st["area"][1]
    pred = oc.make_pattern("bars", 48, 300)[0]
    assert pred[4, 63] and pred[5, 64] and not pred[4, 64] and not pred[5, 63]      # NW-only link across x = 63/64
    assert pred[7, 64] and pred[8, 63] and not pred[7, 63] and not pred[8, 64]      # NE-only link across x = 63/64
    assert oc.label(oc.make_pattern("nested_uv", 64, 64)[0])[0] > 4
    assert oc.decode_key(oc.point_key(0.625, 1234), 100) == (34, 12, 0.625)
