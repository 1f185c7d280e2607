"""Plain-numpy reference of ops.volume_regions (csrc/volume_regions.hip): 3-D connected components with an explicit neighbour list
per connectivity, a sequential union-find whose root is a component's first voxel in raster order (z, y, x), the numbering of
scipy.ndimage.label (by first voxel), the filter rules (size < min_voxels dropped; keep_largest keeps the largest survivor, ties to
the first in raster order; nothing survives -> empty) and the info table. test_volume_regions_cpu.py pins it to scipy.ndimage.label
+ numpy.bincount and shows that every fault of FAULTS fails a case of `cases()`; test_volume_regions_gpu.py compares the device
with it, exactly.

`faults` switches on one deliberate mistake at a time."""
import numpy as np

FAULTS = ("18_as_26", "18_as_6", "z_edges_missing", "x_wrap", "y_wrap", "volume_link", "tie_later", "min_le", "number_by_size",
          "box_of_input")

COLS = ("components", "kept", "voxels_in", "voxels_out", "largest_size", "largest_root", "z0", "y0", "x0", "z1", "y1", "x1")

# the neighbours (dz, dy, dx) that come BEFORE a voxel in raster order; the other half is their mirror image
_FACES = [(0, 0, -1), (0, -1, 0), (-1, 0, 0)]
_EDGES = [(0, -1, -1), (0, -1, 1), (-1, 0, -1), (-1, 0, 1), (-1, -1, 0), (-1, 1, 0)]
_CORNERS = [(-1, -1, -1), (-1, -1, 1), (-1, 1, -1), (-1, 1, 1)]
EARLIER = {6: _FACES, 18: _FACES + _EDGES, 26: _FACES + _EDGES + _CORNERS}


def offsets(connectivity):
    """all neighbours (dz, dy, dx) of a connectivity: 6, 18 or 26 of them"""
    e = EARLIER[connectivity]
    return e + [(-a, -b, -c) for a, b, c in e]


def reference(vols, connectivity=26, min_voxels=0, keep_largest=False, faults=()):
    """vols [R, D, H, W] (or [D, H, W]), non-zero = set -> dict(out uint8 [R, D, H, W], info int64 [R, 12] (COLS), labels int32
    [R, D, H, W], sizes: per volume the int64 sizes of components 1..n)."""
    v = np.asarray(vols) != 0
    if v.ndim == 3:
        v = v[None]
    R, D, H, W = v.shape
    n = D * H * W
    if connectivity not in EARLIER:
        raise ValueError(f"connectivity {connectivity}")
    conn = connectivity
    if conn == 18 and "18_as_26" in faults:
        conn = 26
    if conn == 18 and "18_as_6" in faults:
        conn = 6
    offs = list(EARLIER[conn])
    if "z_edges_missing" in faults:
        offs = [o for o in offs if not (o[0] == -1 and abs(o[1]) + abs(o[2]) == 1)]
    flat = v.reshape(-1)
    fgl = flat.tolist()
    parent = list(range(R * n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)                      # the root is the component's first voxel

    fg = np.flatnonzero(flat)
    for gidx in fg.tolist():
        r, p = divmod(gidx, n)
        z, rem = divmod(p, H * W)
        y, x = divmod(rem, W)
        for dz, dy, dx in offs:
            if z + dz < 0:
                continue
            if "y_wrap" not in faults and not 0 <= y + dy < H:
                continue
            if "x_wrap" not in faults and not 0 <= x + dx < W:
                continue
            q = p + (dz * H + dy) * W + dx
            if 0 <= q < n and fgl[r * n + q]:
                union(gidx, r * n + q)
    if "volume_link" in faults:
        for r in range(R - 1):
            if fgl[r * n + n - 1] and fgl[(r + 1) * n]:
                union(r * n + n - 1, (r + 1) * n)
    root = np.full(R * n, -1, dtype=np.int64)
    root[fg] = [find(a) for a in fg.tolist()]
    size_of = np.bincount(root[fg], minlength=R * n) if fg.size else np.zeros(R * n, dtype=np.int64)
    out = np.zeros((R, D, H, W), dtype=np.uint8)
    labels = np.zeros((R, D, H, W), dtype=np.int32)
    info = np.full((R, 12), -1, dtype=np.int64)
    all_sizes = []
    for r in range(R):
        pos = np.flatnonzero(flat[r * n:(r + 1) * n])          # the volume's voxels in raster order
        rv = root[r * n + pos]
        uniq, first = np.unique(rv, return_index=True)         # first: a component's first voxel among `pos`
        sizes = size_of[uniq].astype(np.int64)
        order = np.argsort(first, kind="stable")               # components by first voxel: their raster order
        uniq, first, sizes = uniq[order], first[order], sizes[order]
        ncomp = len(uniq)
        number = np.arange(1, ncomp + 1)
        if "number_by_size" in faults:
            number = np.empty(ncomp, dtype=np.int64)
            number[np.lexsort((np.arange(ncomp), -sizes))] = np.arange(1, ncomp + 1)
        if ncomp:
            comp = _rank_of(uniq, rv)                          # every voxel's component, as an index into the ordered roots
            labels[r].reshape(-1)[pos] = number[comp]
        all_sizes.append(sizes)
        stay = sizes > min_voxels if "min_le" in faults else sizes >= min_voxels
        best = -1
        if ncomp:
            big = np.flatnonzero(sizes == sizes.max())
            best = int(big[-1] if "tie_later" in faults else big[0])
        if keep_largest:
            only = np.zeros(ncomp, dtype=bool)
            if ncomp and stay[best]:
                only[best] = True
            stay = only
        if ncomp:
            out[r].reshape(-1)[pos] = stay[comp]
        info[r, 0] = ncomp
        info[r, 1] = int(stay.sum())
        info[r, 2] = len(pos)
        info[r, 3] = int(out[r].sum())
        info[r, 4] = int(sizes[best]) if ncomp else 0
        info[r, 5] = int(pos[first[best]]) if ncomp else -1
        boxed = v[r] if "box_of_input" in faults else out[r]
        if boxed.any():
            zz, yy, xx = np.nonzero(boxed)
            info[r, 6:] = (zz.min(), yy.min(), xx.min(), zz.max(), yy.max(), xx.max())
    return {"out": out, "info": info, "labels": labels, "sizes": all_sizes}


def _rank_of(uniq, rv):
    """index into `uniq` (any order, distinct) of every entry of rv"""
    order = np.argsort(uniq)
    return order[np.searchsorted(uniq[order], rv)]


# ---- the case list shared by the CPU and the GPU tests ---------------------------------------------------------------------------
def pair_volume(shape, a, off):
    """two voxels: a and a + off (None if the second falls outside)"""
    b = tuple(i + j for i, j in zip(a, off))
    if not all(0 <= i < s for i, s in zip(b, shape)):
        return None
    v = np.zeros(shape, dtype=np.uint8)
    v[a] = v[b] = 1
    return v


def serpentine(D, rows, W):
    """[D, 2 * rows - 1, W], one voxel thick and ONE 6-connected path: every even plane is a snake (full rows 0, 2, 4, .. joined at
    alternating ends), every odd plane a single voxel that joins the snakes below and above it, by turns at their end and start"""
    H = 2 * rows - 1
    plane = np.zeros((H, W), dtype=np.uint8)
    for k in range(rows):
        plane[2 * k] = 1
        if k + 1 < rows:
            plane[2 * k + 1, W - 1 if k % 2 == 0 else 0] = 1
    start, end = (0, 0), (H - 1, W - 1 if (rows - 1) % 2 == 0 else 0)
    v = np.zeros((D, H, W), dtype=np.uint8)
    for z in range(D):
        if z % 2 == 0:
            v[z] = plane
        else:
            v[(z,) + (end if (z // 2) % 2 == 0 else start)] = 1
    return v


def checkerboard(D, H, W):
    z, y, x = np.indices((D, H, W))
    return ((z + y + x) % 2 == 0).astype(np.uint8)


def random_volume(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


SHAPES = [(1, 1, 1), (1, 1, 63), (1, 2, 64), (2, 1, 65), (2, 5, 64), (3, 2, 65), (3, 5, 63), (5, 2, 257), (5, 5, 1), (2, 2, 257)]
_cache = {}


def cases():
    """-> list of (name, vols uint8 [R, D, H, W], connectivity, min_voxels, keep_largest); built once"""
    if "cases" in _cache:
        return _cache["cases"]
    out = []
    # pairs at each of the 26 offsets under each connectivity, also across the 63 | 64 and 255 | 256 boundaries in x
    allo = offsets(26)
    for conn in (6, 18, 26):
        for shape, anchors in (((3, 5, 65), [(1, 2, 1), (1, 2, 63)]), ((3, 3, 257), [(1, 1, 255), (1, 1, 64)])):
            vols = [pair_volume(shape, a, o) for a in anchors for o in allo]
            out.append((f"pairs{shape[2]}_c{conn}", np.stack(vols), conn, 0, False))
    # row-end, plane-end and volume-end neighbours that must not link
    v = np.zeros((3, 3, 2, 5), dtype=np.uint8)
    v[0, 0, 0, 4] = v[0, 0, 1, 0] = 1                          # end of a row | start of the next
    v[0, 1, 1, 4] = v[0, 2, 0, 0] = 1                          # end of a plane | start of the next
    v[0, 2, 1, 4] = v[1, 0, 0, 0] = 1                          # end of a volume | start of the next
    v[1, 1, 0, 0] = v[1, 0, 1, 4] = 1                          # (0, y, x) | (z - 1, y - 1 wrapped, .)
    v[2, 0, 0, 4] = v[2, 0, 1, 0] = v[2, 0, 1, 1] = 1
    v[2, 2, 1, 4] = 1
    for conn in (6, 18, 26):
        out.append((f"ends_c{conn}", v, conn, 0, False))
        out.append((f"ends_largest_c{conn}", v, conn, 2, True))
    # random volumes over the shapes and densities
    k = 0
    for shape in SHAPES:
        for dens in (0.2, 0.35, 0.5, 0.7):
            conn = (6, 18, 26)[k % 3]
            R = 3 if k % 2 else 1
            vols = np.stack([random_volume(shape, dens, 100 + 7 * k + r) for r in range(R)])
            out.append((f"random{k}_{shape}_d{dens}_c{conn}", vols, conn, 0, False))
            out.append((f"random{k}_filtered", vols, conn, 3, bool(k % 4 < 2)))
            k += 1
    for conn in (6, 18, 26):
        out.append((f"random_mid_c{conn}", np.stack([random_volume((3, 5, 65), 0.35, 900 + r) for r in range(3)]), conn, 2, False))
    out.append(("serpentine_c6", serpentine(5, 3, 65)[None], 6, 0, True))
    out.append(("serpentine_c26", serpentine(3, 3, 257)[None], 26, 0, False))
    for conn in (6, 18, 26):
        out.append((f"checkerboard_c{conn}", checkerboard(3, 5, 65)[None], conn, 0, False))
        out.append((f"checkerboard_largest_c{conn}", checkerboard(2, 2, 64)[None], conn, 0, True))
    out.append(("empty", np.zeros((3, 2, 5, 65), dtype=np.uint8), 26, 0, True))
    out.append(("full", np.full((1, 3, 5, 65), 255, dtype=np.uint8), 6, 0, True))
    out.append(("full_d1", np.ones((3, 1, 2, 257), dtype=np.uint8), 18, 4, False))
    # two and three equally large components: the first in raster order stays
    t = np.zeros((2, 3, 5, 65), dtype=np.uint8)
    t[0, 2, 1, 60:64] = 1
    t[0, 0, 3, 2:6] = 1
    t[1, 0, 4, 62:65] = 1
    t[1, 1, 0:3, 64] = 1
    t[1, 2, 2, 0:3] = 1
    t[1, 2, 4, 10:12] = 1
    out.append(("ties", t, 6, 0, True))
    out.append(("ties_min", t, 26, 3, True))
    # min_voxels at size - 1, size and size + 1 of a known component (sizes 5 and 2), and one that empties the volume
    m = np.zeros((1, 3, 5, 65), dtype=np.uint8)
    m[0, 1, 2, 60:65] = 1
    m[0, 2, 4, 0:2] = 1
    for mv in (4, 5, 6):
        out.append((f"min{mv}", m, 18, mv, False))
        out.append((f"min{mv}_largest", m, 18, mv, True))
    for mv in (1, 2, 3):
        out.append((f"min{mv}_small", m, 6, mv, False))
    out.append(("min_empties", m, 26, 100, False))
    out.append(("min_empties_largest", m, 26, 100, True))
    _cache["cases"] = out
    return out


def expected(name):
    """the reference of case `name`, computed once"""
    key = ("ref", name)
    if key not in _cache:
        _, vols, conn, mv, kl = next(c for c in cases() if c[0] == name)
        _cache[key] = reference(vols, conn, mv, kl)
    return _cache[key]
