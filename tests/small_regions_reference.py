"""Numpy restatement of the batch contract of psam_small_regions (csrc/small_regions.hip) and of ops.small_regions_select, with
the test patterns shared by tests/test_small_regions_cpu.py and tests/test_small_regions_gpu.py.

Per mask: remove_small_regions(mask, t, "holes") then remove_small_regions(., t, "islands") (segment_anything/utils/amg.py:267-291)
-> out {0, 1}, info = {changed_holes, changed_islands, area, 0}, box = XYXY min / max or [0, 0, 0, 0] for an empty mask, score =
float(not changed). The labelling here is its own: minimum-index propagation over the 8 neighbours with pointer jumping, so a region
is named by its first pixel in raster order; test_small_regions_cpu.py pins the whole thing to oracle.amg.remove_small_regions.

`faults` switches single mistakes on, one name each; the CPU test shows that the patterns below tell every one of them from the
contract."""
import numpy as np

FAULTS = ("conn4", "le", "islands_on_unfilled", "tie_last", "keep_largest_unflagged", "sentinel_box")
SHAPES = ((1, 1), (1, 130), (130, 1), (33, 17), (40, 64), (48, 44), (65, 257), (129, 129))
THRESHOLDS = (1, 6, 5.5, 50, 10 ** 6)
INT_MAX = 0x7fffffff


def label_roots(fg, conn4=False):
    """bool [H, W] -> int64 [H, W]: the raster index of the first pixel of the pixel's 8-connected region, -1 on background."""
    H, W = fg.shape
    n = H * W
    lab = np.where(fg, np.arange(n, dtype=np.int64).reshape(H, W), n)
    shifts = [(0, 1), (1, 0), (1, 2), (2, 1)] if conn4 else [(dy, dx) for dy in range(3) for dx in range(3) if (dy, dx) != (1, 1)]
    while True:
        p = np.pad(lab, 1, constant_values=n)
        m = lab
        for dy, dx in shifts:
            m = np.minimum(m, p[dy:dy + H, dx:dx + W])
        flat = np.append(np.where(fg, m, n).ravel(), n)      # a pixel's value is a pixel of its region, at or before it
        while True:
            nxt = flat[flat]
            if np.array_equal(nxt, flat):
                break
            flat = nxt
        new = flat[:n].reshape(H, W)
        if np.array_equal(new, lab):
            return np.where(fg, lab, -1)
        lab = new


def _areas(roots):
    r, c = np.unique(roots[roots >= 0], return_counts=True)
    return r, c                                               # roots ascending = raster order of the regions' first pixels


def one_mask(mask, t, faults=frozenset()):
    """mask [H, W] (0 / non-0) -> (out uint8 {0,1}, changed_holes, changed_islands)."""
    conn4 = "conn4" in faults
    below = (lambda a: a <= t) if "le" in faults else (lambda a: a < t)
    m = np.asarray(mask) != 0
    roots = label_roots(~m, conn4)
    r, c = _areas(roots)
    small = r[below(c.astype(np.float64))]
    ch = len(small) > 0
    filled = m | np.isin(roots, small)
    src = m if "islands_on_unfilled" in faults else filled
    roots = label_roots(src, conn4)
    r, c = _areas(roots)
    sm = below(c.astype(np.float64))
    ci = bool(sm.any())
    out = filled
    if ci:
        keep = r[~sm]
        if len(keep) == 0:
            best = np.flatnonzero(c == c.max())
            keep = r[best[-1 if "tie_last" in faults else 0]:][:1]
            if "keep_largest_unflagged" in faults:
                ci = False
        out = np.isin(roots, keep)
        if "islands_on_unfilled" in faults:
            out = out | (filled & ~m)
    return out.astype(np.uint8), ch, ci


def batch(masks, t, faults=frozenset()):
    """masks [m, H, W] -> (out uint8 [m,H,W], boxes int32 [m,4], scores float32 [m], info int32 [m,4]): the contract of
    psam_small_regions."""
    masks = np.asarray(masks)
    m = len(masks)
    out = np.zeros(masks.shape, np.uint8)
    boxes, scores, info = np.zeros((m, 4), np.int32), np.zeros(m, np.float32), np.zeros((m, 4), np.int32)
    for i in range(m):
        out[i], ch, ci = one_mask(masks[i], t, faults)
        ys, xs = np.nonzero(out[i])
        info[i] = [ch, ci, len(ys), 0]
        scores[i] = float(not ch and not ci)
        if len(ys):
            boxes[i] = [xs.min(), ys.min(), xs.max(), ys.max()]
        elif "sentinel_box" in faults:
            boxes[i] = [INT_MAX, INT_MAX, -1, -1]
    return out, boxes, scores, info


def select(masks, t, nms_thresh):
    """The contract of ops.small_regions_select: batch() and utils.amg.nms_xyxy on its boxes and scores ->
    (out, kept int64 in suppression order, info, boxes)."""
    from protosam_amd.segment_anything.utils.amg import nms_xyxy
    out, boxes, scores, info = batch(masks, t)
    kept = nms_xyxy(boxes.astype(np.int64), scores, nms_thresh)
    return out, np.asarray(kept, dtype=np.int64), info, boxes


def near_crop_edge(boxes, crop_box, orig_box):
    """The integer edge rule of psam_amg_select_crop: boxes int [n, 4] in the crop's frame -> bool [n]."""
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4) + np.array([[crop_box[0], crop_box[1], crop_box[0], crop_box[1]]], dtype=np.int64)
    near_crop = np.abs(b - np.asarray(crop_box, dtype=np.int64)[None]) <= 20
    near_img = np.abs(b - np.asarray(orig_box, dtype=np.int64)[None]) <= 20
    return np.any(near_crop & ~near_img, axis=1)


# ---- patterns ----------------------------------------------------------------------------------------------------------------
def _ring(H, W, k):
    """a filled rectangle with a one-pixel border around a hole of exactly k pixels (the first k pixels of its inside in raster
    order), or None where the shape has no room"""
    wb = min(k, W - 4)
    if wb < 1:
        return None
    rows = -(-k // wb)
    if rows + 3 > H:
        return None
    m = np.zeros((H, W), np.uint8)
    m[1:rows + 3, 1:wb + 3] = 1
    inside = np.zeros(rows * wb, bool)
    inside[:k] = True
    m[2:rows + 2, 2:wb + 2][inside.reshape(rows, wb)] = 0
    return m


def spiral(n):
    """a one-pixel-wide square spiral in an n x n mask: one long 8-connected (and 4-connected) chain"""
    m = np.zeros((n, n), np.uint8)
    y0, x0, y1, x1 = 0, 0, n - 1, n - 1
    m[y0, x0:x1 + 1] = 1
    while True:
        m[y0:y1 + 1, x1] = 1                                  # down the right side
        if y1 - y0 < 2:
            break
        m[y1, x0:x1 + 1] = 1                                  # left along the bottom
        if x1 - x0 < 2:
            break
        y0 += 2
        m[y0:y1 + 1, x0] = 1                                  # up the left side
        x1 -= 2
        if x1 <= x0 or y0 > y1:
            break
        m[y0, x0:x1 + 1] = 1                                  # right along the next top
        y1 -= 2
        x0 += 2
        if y1 <= y0 or x0 > x1:
            break
    return m


def patterns(H, W):
    """name -> uint8 [H, W] mask (0 / non-0; some use 255 or 7 for "set") of everything the issue lists that fits the shape."""
    g = np.random.RandomState(H * 1000 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    P = {}
    P["empty"] = np.zeros((H, W), np.uint8)
    P["full"] = np.full((H, W), 255, np.uint8)
    P["checker"] = (((yy + xx) & 1) * 7).astype(np.uint8)      # one diagonal-connected region whose complement is one too
    P["checker_inv"] = ((yy + xx + 1) & 1).astype(np.uint8)
    if H == W and H >= 5:
        P["spiral"] = spiral(H)
        P["spiral_inv"] = (1 - spiral(H)).astype(np.uint8)
    comb = np.zeros((H, W), np.uint8)                          # a spine along the top, teeth in every other column
    comb[0, :] = 1
    comb[:, ::2] = 1
    P["comb"] = comb
    comb2 = np.zeros((H, W), np.uint8)                         # teeth hanging from the LAST row: roots found late
    comb2[H - 1, :] = 1
    comb2[:, 1::2] = 1
    P["comb_up"] = comb2
    runs = np.zeros((H, W), np.uint8)                          # horizontal runs crossing x = 64, 128 and 256
    for j, xb in enumerate((64, 128, 256)):
        if W > xb and H > 2 * j:
            runs[min(2 * j, H - 1), max(xb - 3 - j, 0):min(xb + 2 + j, W)] = 1
            if H > 2 * j + 8:
                runs[2 * j + 8, max(xb - 1, 0):xb + 1] = 255   # a two-pixel run right on the boundary
    P["runs"] = runs
    rows = np.zeros((H, W), np.uint8)                          # whole rows, every third: runs as long as the row
    rows[::3, :] = 1
    P["rows"] = rows
    holes = np.ones((H, W), np.uint8)                          # one-pixel holes on the border and in the corners
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H - 1, W // 2), (H // 2, W - 1),
                 (H // 2, W // 2)):
        holes[y, x] = 0
    P["border_holes"] = holes
    for k in (1, 5, 6, 49, 50):                                # a ring whose hole has exactly t and exactly t - 1 pixels
        r = _ring(H, W, k)
        if r is not None:
            P[f"ring{k}"] = r
    if H >= 10 and W >= 20:                                    # a thin ring: 28 pixels around a hole of 36, beside a block of 64 -
        thin = np.zeros((H, W), np.uint8)                      # at t = 50 an island only once its hole is filled
        thin[1:9, 1:9] = 1
        thin[2:8, 2:8] = 0
        thin[1:9, 11:19] = 1
        P["thin_ring"] = thin
    outer = np.ones((H, W), np.uint8)                          # an outer background smaller than t: it is filled
    outer[0, :min(3, W)] = 0
    outer[H - 1, W - 1] = 0
    P["small_background"] = outer
    if H >= 7 and W >= 9:                                      # all islands below t = 6, two equal largest: the tie
        tie = np.zeros((H, W), np.uint8)
        tie[H - 3:H - 1, 1:3] = 1
        tie[1:3, W - 3:W - 1] = 1
        tie[H // 2, W // 2] = 1
        P["tie"] = tie
        tie2 = np.zeros((H, W), np.uint8)                      # the same with areas of 5, and the later one listed first in x
        tie2[1:3, 5:7] = 1; tie2[3, 5] = 1
        tie2[H - 3:H - 1, 1:3] = 1; tie2[H - 1, 1] = 1
        P["tie5"] = tie2
    elif W >= 9 or H >= 9:                                     # single rows and columns: runs of 3, 1, 3
        tie = np.zeros((H, W), np.uint8)
        flat = tie.reshape(-1)
        flat[1:4] = 1; flat[5] = 1; flat[-4:-1] = 1
        P["tie"] = tie
    for d in (0.05, 0.3, 0.55, 0.8):
        P[f"random{d}"] = (g.rand(H, W) < d).astype(np.uint8)
    blob = ((yy - H / 2.0) ** 2 / max(H / 3.0, 1) ** 2 + (xx - W / 2.0) ** 2 / max(W / 3.0, 1) ** 2 < 1).astype(np.uint8)
    P["blob_speckle"] = (blob ^ (g.rand(H, W) < 0.04)).astype(np.uint8)    # what a generator's mask looks like
    return P


def pattern_batch(H, W):
    """-> (names, uint8 [m, H, W]) of patterns(H, W)"""
    P = patterns(H, W)
    return list(P), np.stack([P[k] for k in P])
