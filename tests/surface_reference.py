"""The surface-distance definitions restated in plain numpy, and the checks both surface test files apply.

MedPy's hd / hd95 / asd / assd with connectivity=1 (test_surface_cpu.py pins this file to scipy's binary_erosion and
distance_transform_edt):
  surface S(M)   the voxels of M [D, H, W] with a face neighbour that is background or outside the array - the 4 in-plane
                 neighbours when D == 1, the 6 neighbours when D > 1 - from shifted comparisons;
  d2(p)          min over the other surface, in float32 with every operation rounded separately:
                 ((dx*sx)*(dx*sx) + (dy*sy)*(dy*sy)) + (dz*sz)*(dz*sz), dx / dy / dz exact integer offsets;
  metrics        float64 functions of sqrt(d2): hd the larger directed maximum, hd95 numpy.percentile of both directed sets
                 together, asd_pg / asd_gp the directed means (math.fsum), assd their mean; NaN where a surface is empty.
`faults` switches on one deliberate mistake at a time; test_surface_cpu.py shows that each makes the checks below fail."""
import math

import numpy as np

COLS = ("n_pred", "n_gt", "hd", "hd95", "assd", "asd_pg", "asd_gp", "status")
FAULTS = ("eight_neighbours", "edge_not_surface", "hd_one_direction", "percentile_one_direction", "nearest_rank",
          "swap_sy_sz", "z_neighbours_at_depth_1", "fma")
REL = 1e-12        # hd95 / assd / asd: a few float64 roundings of the interpolation and the sums; two distinct float32
#                    neighbours differ by 6e-8, seven orders above it, so a wrong element cannot pass


def _shifted(m, axis, step, fill):
    out = np.full_like(m, fill)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if step > 0:
        src[axis], dst[axis] = slice(0, -1), slice(1, None)
    else:
        src[axis], dst[axis] = slice(1, None), slice(0, -1)
    out[tuple(dst)] = m[tuple(src)]
    return out


def surface_mask(m, faults=()):
    """S(m) for a boolean [D, H, W] array"""
    m = np.asarray(m, dtype=bool)
    assert m.ndim == 3
    outside = "edge_not_surface" in faults                      # what lies outside the array: background (False), or, wrongly, set
    axes = [1, 2] + ([0] if m.shape[0] > 1 or "z_neighbours_at_depth_1" in faults else [])
    interior = m.copy()
    for axis in axes:
        for step in (1, -1):
            interior &= _shifted(m, axis, step, outside)
    if "eight_neighbours" in faults:
        for sy in (1, -1):
            for sx in (1, -1):
                interior &= _shifted(_shifted(m, 1, sy, outside), 2, sx, outside)
    return m & ~interior


def surface_points(m, faults=()):
    """ascending linear indices (z * H + y) * W + x of S(m)"""
    return np.flatnonzero(surface_mask(m, faults)).astype(np.int64)


def min_d2(query, other, shape, spacing, faults=()):
    """float32 [len(query)]: per query index the minimum over `other` of the squared distance; +inf where `other` is empty"""
    sz, sy, sx = (np.float32(v) for v in spacing)
    if "swap_sy_sz" in faults:
        sy, sz = sz, sy
    out = np.full(len(query), np.inf, dtype=np.float32)
    if len(other) == 0 or len(query) == 0:
        return out
    qz, qy, qx = (v.astype(np.int64) for v in np.unravel_index(query, shape))
    oz, oy, ox = (v.astype(np.int64) for v in np.unravel_index(other, shape))
    step = max(1, (1 << 22) // len(other))
    for i in range(0, len(query), step):
        dx = (qx[i:i + step, None] - ox[None]).astype(np.float32) * sx
        dy = (qy[i:i + step, None] - oy[None]).astype(np.float32) * sy
        dz = (qz[i:i + step, None] - oz[None]).astype(np.float32) * sz
        if "fma" in faults:                                     # what a contracting compiler makes of it: fma(dz, dz, fma(dy, dy, dx*dx))
            t = (dy.astype(np.float64) * dy + (dx * dx).astype(np.float64)).astype(np.float32)
            d = (dz.astype(np.float64) * dz + t.astype(np.float64)).astype(np.float32)
        else:
            d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        out[i:i + step] = d.min(axis=1)
    return out


def table_row(d2_p, d2_g, faults=(), status=0):
    """the float64 row (COLS) of one pair from its two directed sets of squared distances"""
    row = np.full(8, np.nan, dtype=np.float64)
    row[0], row[1], row[7] = len(d2_p), len(d2_g), status
    if len(d2_p) == 0 or len(d2_g) == 0 or status != 0:
        return row
    a, b = np.sqrt(d2_p.astype(np.float64)), np.sqrt(d2_g.astype(np.float64))
    row[2] = a.max() if "hd_one_direction" in faults else max(a.max(), b.max())
    both = a if "percentile_one_direction" in faults else np.concatenate([a, b])
    if "nearest_rank" in faults:
        row[3] = np.sort(both)[max(int(math.ceil(0.95 * len(both))) - 1, 0)]
    else:
        row[3] = np.percentile(both, 95)
    row[5], row[6] = math.fsum(a) / len(a), math.fsum(b) / len(b)
    row[4] = (row[5] + row[6]) / 2
    return row


def reference(P, G, spacing=(1.0, 1.0, 1.0), faults=()):
    """everything the kernels produce for one row: P, G boolean [D, H, W] -> dict points_p / points_g (ascending linear indices),
    d2_p / d2_g (float32, in the order of the points), row (float64 [8])"""
    P, G = np.asarray(P, dtype=bool), np.asarray(G, dtype=bool)
    assert P.shape == G.shape and P.ndim == 3
    pp, pg = surface_points(P, faults), surface_points(G, faults)
    dp, dg = min_d2(pp, pg, P.shape, spacing, faults), min_d2(pg, pp, P.shape, spacing, faults)
    return {"points_p": pp, "points_g": pg, "d2_p": dp, "d2_g": dg, "row": table_row(dp, dg, faults)}


# ---- the checks (the GPU test applies them to the kernels, the CPU test to the reference with a fault switched on) ---------------
def check_points(got_p, got_g, ref):
    """the surface voxels as sets per segment, exactly"""
    for name, got, want in (("pred", got_p, ref["points_p"]), ("gt", got_g, ref["points_g"])):
        got = np.sort(np.asarray(got, dtype=np.int64))
        assert len(got) == len(want), (name, len(got), len(want))
        assert np.array_equal(got, want), (name, got[got != want][:5], want[got != want][:5])


def check_d2(points_p, d2_p, points_g, d2_g, ref):
    """d2 bit for bit, whatever order the points are in"""
    for name, pts, got, wp, want in (("pred", points_p, d2_p, ref["points_p"], ref["d2_p"]),
                                     ("gt", points_g, d2_g, ref["points_g"], ref["d2_g"])):
        order = np.argsort(np.asarray(pts, dtype=np.int64), kind="stable")
        got = np.asarray(got, dtype=np.float32)[order]
        assert np.array_equal(np.asarray(pts, dtype=np.int64)[order], wp), name
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        assert bad.size == 0, (name, bad[:5], got[bad[:5]], want[bad[:5]])


def check_row(got, want):
    """counts and status exact, the NaN pattern equal, hd bit-equal, hd95 / assd / asd_pg / asd_gp within REL"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == (8,) and want.shape == (8,)
    assert got[0] == want[0] and got[1] == want[1] and got[7] == want[7], (got, want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    if np.isnan(want[2]):
        return
    assert got[2:3].view(np.uint64)[0] == want[2:3].view(np.uint64)[0], ("hd", got[2], want[2])
    for c in (3, 4, 5, 6):
        assert abs(got[c] - want[c]) <= REL * abs(want[c]), (COLS[c], got[c], want[c])


# ---- shapes -----------------------------------------------------------------------------------------------------------------------
def blobs(shape, seed, n=4, fill=0.35):
    """a boolean [D, H, W] array of a few overlapping ellipsoids, some touching the array's faces"""
    rng = np.random.default_rng(seed)
    D, H, W = shape
    z, y, x = np.ogrid[:D, :H, :W]
    m = np.zeros(shape, dtype=bool)
    for _ in range(n):
        c = rng.uniform(0, 1, 3) * (D, H, W)
        r = np.maximum(rng.uniform(0.1, fill, 3) * (D, H, W), (min(2.6, D), 2.6, 2.6))   # thick enough for an interior
        m |= ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 <= 1.0
    return m
