"""Oracle: the connected-components table and the negative point prompts of csrc/ccl.hip, vectorised (numpy / scipy).
Test infrastructure only (see oracle/__init__.py).

Restates the same operations as `glue.connected_components_with_stats`, `glue.most_conf_point` and `glue.sam_neg_points`
(util/utils.py:474-494, ProtoSAM.py:242-289, :361-372, :395-419), which loop over the components on the whole image; these
functions do one pass over the foreground (bincount, ufunc.at, one lexsort) and one crop per ring, so images with thousands of
components at 1024^2 stay cheap. Every output is an exact integer except the float64 confidence.

Conventions shared with the kernels:
  * labels 1..n in raster order of each component's first pixel (scipy.ndimage.label numbers components that way);
  * ties of the most confident pixel go to the first pixel in raster order;
  * a point key is (float bits of p) << 32 | (0xFFFFFFFF - pixel index), 0 = no pixel.

`make_pattern` builds the masks where lock-free union-find goes wrong (diagonal-only links, unions that meet only in the last
row, runs across the 64- and 256-lane segment boundaries, percolating noise), with probabilities quantised to multiples of 1/8.
"""
import numpy as np
import scipy.ndimage as ndi

EIGHT = np.ones((3, 3), dtype=bool)

# a table row (csrc/ccl.hip): area, sum_x, sum_y, min_x, min_y, max_x, max_y, conf, best_x, best_y, best_p, 0
ROW_NAMES = ("area", "sum_x", "sum_y", "min_x", "min_y", "max_x", "max_y", "conf", "best_x", "best_y", "best_p")
INT_COLS = (0, 1, 2, 3, 4, 5, 6, 8, 9)


def label(pred):
    """8-connected components of pred != 0 -> (n, labels int32 [H,W])."""
    lab, n = ndi.label(np.asarray(pred) != 0, structure=EIGHT)
    return int(n), lab.astype(np.int32)


def component_stats(labels, n, pfg, fg_total):
    """Per component k = 0..n-1 (label k+1): dict of arrays area, sum_x, sum_y, min_x, min_y, max_x, max_y, best_x, best_y,
    first (int64; first = raster index of the component's first pixel), best_p (float32) and
    conf = sum(p_fg [label = k+1]) / (fg_total + 1e-6) (float64)."""
    H, W = labels.shape
    flat = labels.ravel()
    idx = np.flatnonzero(flat).astype(np.int64)
    lab = flat[idx].astype(np.int64) - 1
    x, y = idx % W, idx // W
    p = np.asarray(pfg, dtype=np.float32).ravel()[idx]
    out = {"area": np.bincount(lab, minlength=n).astype(np.int64)}
    # float64 weights: sums of integers below 2^53 are exact
    out["sum_x"] = np.bincount(lab, weights=x, minlength=n).astype(np.int64)
    out["sum_y"] = np.bincount(lab, weights=y, minlength=n).astype(np.int64)
    for name, fn, init, v in (("min_x", np.minimum, W, x), ("min_y", np.minimum, H, y),
                              ("max_x", np.maximum, -1, x), ("max_y", np.maximum, -1, y), ("first", np.minimum, H * W, idx)):
        a = np.full(n, init, dtype=np.int64)
        fn.at(a, lab, v)
        out[name] = a
    # most confident pixel: sort by label, then p descending, then raster index ascending; each label's first entry wins
    order = np.lexsort((idx, -p.astype(np.float64), lab))
    starts = order[np.searchsorted(lab[order], np.arange(n))]
    out["best_x"], out["best_y"], out["best_p"] = x[starts], y[starts], p[starts]
    out["conf"] = np.bincount(lab, weights=p.astype(np.float64), minlength=n) / (float(fg_total) + 1e-6)
    return out


def ccl_reference(pred, pfg):
    """-> (n, labels int32 [H,W], component_stats with the denominator sum(pred != 0))."""
    n, lab = label(pred)
    return n, lab, component_stats(lab, n, pfg, int((np.asarray(pred) != 0).sum()))


def table_rows(st, ks=None):
    """Table rows (float64 [len(ks), 12], the csrc/ccl.hip layout) of components ks (default: all)."""
    ks = np.arange(len(st["area"])) if ks is None else np.asarray(ks, dtype=np.int64)
    rows = np.zeros((len(ks), 12), dtype=np.float64)
    for c, name in enumerate(ROW_NAMES):
        rows[:, c] = st[name][ks]
    return rows


def point_key(p, index):
    """(float bits of p) << 32 | (0xFFFFFFFF - index) as a python int (p >= 0)."""
    return (int(np.array(p, dtype=np.float32).view(np.uint32)) << 32) | (0xFFFFFFFF - int(index))


def _first_max_key(vals, region, index):
    """Key of the first (raster order) maximum of vals over region, or 0 when region is empty. A crop keeps the raster order
    of its pixels, so the first occurrence in the crop is the first in the image."""
    if not region.any():
        return 0
    i = int(np.argmax(np.where(region, vals.astype(np.float64), -np.inf)))
    return point_key(vals.ravel()[i], index.ravel()[i])


def neg_point_keys(labels, st, pbg, r, thr, max_comp):
    """psam_neg_points restated -> uint64 keys [max_comp + 1]:
    keys[0]     = the first pixel with the largest p_bg among p_bg >= thr (inclusive);
    keys[1 + k] = the first pixel with the largest p_bg in the ring of component k, k < min(n, max_comp): the (2r+1) x (2r+1)
                  box dilation of the component clipped to the image, minus the component, evaluated on the box +- r crop;
    every other key 0."""
    H, W = labels.shape
    pbg = np.asarray(pbg, dtype=np.float32)
    index = np.arange(H * W, dtype=np.int64).reshape(H, W)
    keys = np.zeros(max_comp + 1, dtype=np.uint64)
    keys[0] = _first_max_key(pbg, pbg >= np.float32(thr), index)
    for k in range(min(len(st["area"]), max_comp)):
        y0, y1 = max(int(st["min_y"][k]) - r, 0), min(int(st["max_y"][k]) + r, H - 1) + 1
        x0, x1 = max(int(st["min_x"][k]) - r, 0), min(int(st["max_x"][k]) + r, W - 1) + 1
        comp = labels[y0:y1, x0:x1] == k + 1
        dil = ndi.maximum_filter(comp, size=2 * r + 1, mode="constant", cval=False)
        keys[1 + k] = _first_max_key(pbg[y0:y1, x0:x1], dil & ~comp, index[y0:y1, x0:x1])
    return keys


def decode_key(key, W):
    """key (uint64 or python int) -> (x, y, p) or None."""
    key = int(key) & ((1 << 64) - 1)
    if key == 0:
        return None
    i = 0xFFFFFFFF - (key & 0xFFFFFFFF)
    return i % W, i // W, float(np.array(key >> 32, dtype=np.uint32).view(np.float32))


# ---- adversarial masks --------------------------------------------------------------------------------------------------
PATTERNS = ("empty", "full", "checker", "lattice", "diag", "antidiag", "spiral", "comb", "nested_uv", "bars", "noise20",
            "noise41", "noise60", "blobs", "twins")


def _spiral(H, W):
    """Concentric 1-pixel rectangle outlines two pixels apart, each cut just below its top-left corner and bridged to the
    corner of the next one inside: one long 1-pixel path."""
    m = np.zeros((H, W), np.uint8)
    d = 0
    while d <= (H - 1) // 2 and d <= (W - 1) // 2:
        x0, y0, x1, y1 = d, d, W - 1 - d, H - 1 - d
        m[y0, x0:x1 + 1] = m[y1, x0:x1 + 1] = 1
        m[y0:y1 + 1, x0] = m[y0:y1 + 1, x1] = 1
        d += 2
    d = 0
    while d + 2 <= (H - 1) // 2 and d + 2 <= (W - 1) // 2:
        m[d + 1, d] = 0            # the cut of outline d
        m[d + 2, d + 1] = 1        # the bridge to (d + 2, d + 2), the corner of outline d + 2
        d += 2
    return m


def _nested_uv(H, W):
    """Nested U shapes (left half) and V shapes (right half): the two arms of each start in row 0 and meet only at its
    bottom, which lies two rows above the bottom of the next outer one."""
    m = np.zeros((H, W), np.uint8)
    half = W // 2
    xc, ss = half // 2, list(range(1, half // 2, 2))
    for s in ss:                                        # U: arms at xc -+ s, bottom row at `depth`
        depth = H - 1 - (ss[-1] - s)
        if depth < 0:
            continue
        m[:depth + 1, xc - s] = m[:depth + 1, xc + s] = 1
        m[depth, xc - s:xc + s + 1] = 1
    xc = half + (W - half) // 2
    for s in range(1, (W - half) // 2, 3):              # V: arms x = xc -+ (s - y), y = 0..s
        ys = np.arange(0, min(s, H - 1) + 1)
        m[ys, xc - s + ys] = 1
        m[ys, xc + s - ys] = 1
    return m


def _bars(H, W):
    """Per 12-row band, for one segment boundary c (64, 256, 128, 512 in turn, whichever fit): bars that end at x = c - 1,
    start at x = c, touch across c only diagonally (both ways), and cross c."""
    m = np.zeros((H, W), np.uint8)
    cs = [c for c in (64, 256, 128, 512) if c < W]
    band = 0
    while cs and 12 * band + 11 < H:
        c, y = cs[band % len(cs)], 12 * band
        left, right = slice(max(c - 20, 0), c), slice(c, min(c + 21, W))
        m[y, left] = 1
        m[y + 2, right] = 1
        m[y + 4, left] = 1
        m[y + 5, right] = 1                               # (c, y+5) meets (c-1, y+4) only as its NW neighbour
        m[y + 7, right] = 1
        m[y + 8, left] = 1                                # (c-1, y+8) meets (c, y+7) only as its NE neighbour
        m[y + 10, max(c - 20, 0):min(c + 21, W)] = 1
        band += 1
    return m


def _blobs(H, W, seed, thr=0.15):
    """Thresholded bilinear upsampling of a coarse Gaussian field (the smooth blobs of test_protosam_gpu)."""
    import torch
    f = torch.from_numpy(np.random.RandomState(seed).randn(1, 1, max(1, H // 64), max(1, W // 64)).astype(np.float32))
    return (torch.nn.functional.interpolate(f, size=(H, W), mode="bilinear")[0, 0].numpy() > thr).astype(np.uint8)


def _twins(H, W, seed):
    """One random component at the top-left corner and a translated copy at the bottom-right one (when it fits apart)."""
    m = np.zeros((H, W), np.uint8)
    h, w = max(1, min(12, H // 3)), max(1, min(14, W // 3))
    shape = (np.random.RandomState(seed).random_sample((h, w)) < 0.7).astype(np.uint8)
    shape[h // 2, :] = 1
    shape[:, w // 2] = 1
    m[:h, :w] = shape
    dy, dx = H - h, W - w
    if dy > h or dx > w:
        m[dy:, dx:] = shape
    return m, (dy, dx, h, w)


def make_pattern(name, H, W, seed=0):
    """-> (pred uint8 [H,W] of 0/1, p_fg float32 [H,W], p_bg float32 [H,W]); the probabilities are multiples of 1/8 in [0, 1],
    so ties are common and every partial sum of p_fg below 2^21 is exact in fp32."""
    yy, xx = np.mgrid[0:H, 0:W]
    g = np.random.RandomState(seed)
    pfg = (g.randint(0, 9, size=(H, W)) / 8.0).astype(np.float32)
    pbg = (g.randint(0, 9, size=(H, W)) / 8.0).astype(np.float32)
    if name == "empty":
        m = np.zeros((H, W), np.uint8)
    elif name == "full":
        m = np.ones((H, W), np.uint8)
    elif name == "checker":
        m = (xx + yy) % 2 == 0
    elif name == "lattice":
        m = (xx % 2 == 0) & (yy % 2 == 0)
    elif name == "diag":
        m = (xx - yy) % 7 == 0
    elif name == "antidiag":
        m = (xx + yy) % 7 == 0
    elif name == "spiral":
        m = _spiral(H, W)
    elif name == "comb":
        m = (xx % 2 == 0) | (yy == H - 1)
    elif name == "nested_uv":
        m = _nested_uv(H, W)
    elif name == "bars":
        m = _bars(H, W)
    elif name.startswith("noise"):
        m = g.random_sample((H, W)) < int(name[5:]) / 100.0
    elif name == "blobs":
        m = _blobs(H, W, seed)
    elif name == "twins":
        m, (dy, dx, h, w) = _twins(H, W, seed)
        pfg[dy:, dx:] = pfg[:h, :w]                     # equal p_fg on both copies: equal confidences
    else:
        raise ValueError(name)
    return np.ascontiguousarray(m, dtype=np.uint8), pfg, pbg
