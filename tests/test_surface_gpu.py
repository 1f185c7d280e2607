"""GPU: psam_surface_points / psam_surface_dist / psam_surface_stats against tests/surface_reference.py - surface voxels as exact sets,
squared distances bit for bit, hd bit-equal and hd95 / assd / asd within 1e-12 relative (surface_reference.check_*, the checks whose
teeth test_surface_cpu.py shows); the capacity rule with poisoned guard regions; the evaluate_* drivers and score_scan_surfaces
against ops.surface_distances on the masks they keep."""
import numpy as np
import pytest
import torch

import surface_reference as sr

pytestmark = pytest.mark.gpu

ANISO = (2.5, 0.7, 0.9)
POISON32, POISON64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
GUARD = 64


def _volumes(t):
    return t.reshape((-1,) + tuple(t.shape[-2:])).cpu().numpy()


def _chain(pred, label, rows, spacing, cap, max_depth=None):
    """the three kernels and the sort between them -> (work with host copies, table on the host)"""
    from protosam_amd import ops
    work = ops.surface_points(pred, label, rows, cap, max_depth=max_depth)
    ops.surface_dist(work, spacing, keys=True)
    table = ops.surface_stats(torch.sort(work["keys"])[0], work)
    torch.cuda.synchronize()
    host = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in work.items()}
    return host, table.cpu().numpy()


def _row_volumes(pred_np, label_np, row):
    pp, pv, lp, lv, D = (int(v) for v in row)
    return pred_np[pp:pp + D] == pv, label_np[lp:lp + D] == lv


def _check_all(pred, label, rows, spacing, cap=None, refs=None):
    """every output of the chain for every row against the reference; -> (host work, table, references)"""
    rows = [tuple(int(v) for v in r) for r in rows]
    pred_np, label_np = _volumes(pred), _volumes(label)
    if refs is None:
        refs = [sr.reference(*_row_volumes(pred_np, label_np, r), spacing) for r in rows]
    if cap is None:
        cap = max(1, sum(len(r["points_p"]) + len(r["points_g"]) for r in refs))
    work, table = _chain(pred, label, rows, spacing, cap)
    off = work["offsets"]
    assert off[0] == 0 and (work["status"] == 0).all()
    for k, ref in enumerate(refs):
        assert work["counts"][k].tolist() == [len(ref["points_p"]), len(ref["points_g"])], (k, work["counts"][k])
        pp, pg = work["points"][off[2 * k]:off[2 * k + 1]], work["points"][off[2 * k + 1]:off[2 * k + 2]]
        sr.check_points(pp, pg, ref)
        sr.check_d2(pp, work["d2"][off[2 * k]:off[2 * k + 1]], pg, work["d2"][off[2 * k + 1]:off[2 * k + 2]], ref)
        sr.check_row(table[k], ref["row"])
    return work, table, refs


def _blob_rows(dev, H, W, D, seed, dtype=torch.uint8):
    """R volumes of D planes each: random blobs (some touching the faces), a full volume, an empty one, single voxels in a corner and
    inside, an object on every face"""
    vols_p, vols_g = [], []
    for k in range(3):
        vols_p.append(sr.blobs((D, H, W), seed + k))
        vols_g.append(sr.blobs((D, H, W), seed + 50 + k))
    full, empty = np.ones((D, H, W), dtype=bool), np.zeros((D, H, W), dtype=bool)
    corner, inner = empty.copy(), empty.copy()
    corner[D - 1, H - 1, W - 1] = True
    inner[0, H // 2, W // 3] = True
    faces = empty.copy()
    faces[:, 0, :] = faces[:, H - 1, :] = faces[:, :, 0] = faces[:, :, W - 1] = True
    faces[0, 2:5, 2:9] = faces[D - 1, 7:20, 5:8] = True
    vols_p += [full, empty, corner, inner, faces, full, vols_p[0]]
    vols_g += [vols_g[0], vols_g[1], inner, corner, vols_g[2], full, empty]
    R = len(vols_p)
    pred = torch.from_numpy(np.concatenate(vols_p).astype(np.uint8)).to(dtype).to(dev)
    label = torch.from_numpy(np.concatenate(vols_g).astype(np.uint8)).to(dtype).to(dev)
    return pred, label, [(r * D, 1, r * D, 1, D) for r in range(R)]


@pytest.mark.parametrize("D", [1, 2, 5])
@pytest.mark.parametrize("H,W", [(37, 53), (64, 64)])
def test_surfaces_distances_and_statistics_on_blobs(dev, H, W, D):
    pred, label, rows = _blob_rows(dev, H, W, D, seed=H + D)
    _, table, refs = _check_all(pred, label, rows, ANISO)
    assert np.isnan(table[4, 2]) and table[4, 0] == 0 and table[9, 1] == 0 and np.isnan(table[9, 3])      # an empty side: NaN
    assert sum(len(r["points_p"]) for r in refs) > 300
    _check_all(pred, label, rows, (1.0, 1.0, 1.0), refs=None)
    # P == G: every distance is zero
    work, table = _chain(pred, pred, rows, ANISO, 4 * pred.numel())
    filled = work["d2"][:work["offsets"][-1]]
    assert filled.size > 600 and (filled.view(np.uint32) == 0).all()
    assert (table[[0, 1, 2, 3, 5, 6, 7, 8, 9], 2:7] == 0).all() and np.isnan(table[4, 2:7]).all()


PRED_TYPES = [torch.uint8, torch.float32, torch.int16, torch.int32, torch.int64]


@pytest.mark.parametrize("pred_dtype", PRED_TYPES)
@pytest.mark.parametrize("label_dtype", PRED_TYPES)
def test_types(dev, pred_dtype, label_dtype):
    """every dtype pair seg_counts accepts: {0, 1} masks [n, C, H, W] against a label map, by class, for D = 1 and D = 2"""
    from protosam_amd.metrics import surface_rows
    H, W, C = 37, 53, 3
    lab = np.zeros((2, H, W), dtype=np.int64)
    masks = np.zeros((2, C, H, W), dtype=np.int64)
    for k in range(2):
        for c in range(C):
            lab[k][sr.blobs((1, H, W), 10 * k + c, n=2)[0]] = c + 1
            masks[k, c] = sr.blobs((1, H, W), 10 * k + c + 5, n=2)[0]
    pred, label = torch.from_numpy(masks).to(pred_dtype).to(dev), torch.from_numpy(lab).to(label_dtype).to(dev)
    _check_all(pred, label, surface_rows(2, [1, 2, 3]).tolist(), ANISO)
    vol = pred.permute(1, 0, 2, 3).contiguous()                   # class-major volumes of depth 2
    _check_all(vol, label, surface_rows(1, [1, 2, 3], depth=2).tolist(), ANISO)
    # a value a uint8 plane cannot hold matches nothing; -0. == 0 by value
    work, table = _chain(pred, label, [(0, 257, 0, 1, 1), (0, 1, 0, -255, 1), (0, 0, 0, 0, 1)], ANISO, 4 * H * W)
    assert work["counts"][0, 0] == 0 and work["counts"][1, 1] == 0 and (work["counts"][2] > 0).all()


def test_views_plane_strides_and_odd_offsets(dev):
    from protosam_amd.metrics import surface_rows
    n, C, H, W = 3, 4, 37, 53
    big = torch.from_numpy(np.stack([np.stack([sr.blobs((1, H, W), 7 * k + c)[0] for c in range(C)]) for k in range(n + 1)])
                           .astype(np.uint8)).to(dev)
    label = torch.from_numpy(np.stack([sr.blobs((1, H, W), 90 + k)[0] for k in range(n + 1)]).astype(np.uint8)).to(dev)
    view = big[1:]                                                 # a storage offset
    assert view.data_ptr() != big.data_ptr()
    _check_all(view, label, surface_rows(n, [1, 1, 1, 1], label_planes=[1, 2, 3]).tolist(), ANISO)
    _check_all(big[:, 1], label, surface_rows(n + 1).tolist(), ANISO)                     # plane stride C * H * W
    _check_all(big[:, 1], label, surface_rows(1, None, depth=n + 1).tolist(), ANISO)     # ... as one volume of 4 planes
    for shift_p, shift_l, dt in ((1, 0, torch.uint8), (0, 3, torch.uint8), (5, 2, torch.int16), (3, 1, torch.float32)):
        flat_p = torch.zeros(3 * H * W + 16, dtype=dt, device=dev)
        flat_l = torch.zeros(3 * H * W + 16, dtype=torch.uint8, device=dev)
        flat_p[shift_p:shift_p + 3 * H * W] = big[:3, 0].reshape(-1).to(dt)
        flat_l[shift_l:shift_l + 3 * H * W] = label[:3].reshape(-1)
        pred, lab = flat_p[shift_p:shift_p + 3 * H * W].view(3, H, W), flat_l[shift_l:shift_l + 3 * H * W].view(3, H, W)
        assert pred.storage_offset() == shift_p and lab.storage_offset() == shift_l
        _check_all(pred, lab, [(0, 1, 0, 1, 1), (1, 1, 2, 1, 1), (0, 1, 0, 1, 3), (1, 1, 1, 1, 2)], ANISO)


def _isolated(rng, H, W, count):
    """a plane with `count` isolated pixels (even coordinates: no two are face neighbours), each of which is a surface voxel"""
    cells = rng.permutation((H // 2) * (W // 2))[:count]
    m = np.zeros((H, W), dtype=bool)
    m[2 * (cells // (W // 2)), 2 * (cells % (W // 2))] = True
    return m


def test_segment_sizes_around_the_tile(dev):
    """1, T - 1, T, T + 1 and 2T + 1 points on either side (every pair of sizes, one row each): the query tiles and the LDS tiles of
    psam_surface_dist straddled both ways; unit and anisotropic spacing"""
    from protosam_amd import ops
    T, H, W = ops.SURFACE_TILE, 64, 64
    sizes = [1, T - 1, T, T + 1, 2 * T + 1]
    rng = np.random.default_rng(5)
    pairs = [(a, b) for a in sizes for b in sizes]
    pred = torch.from_numpy(np.stack([_isolated(rng, H, W, a) for a, _ in pairs]).astype(np.uint8)).to(dev)
    label = torch.from_numpy(np.stack([_isolated(rng, H, W, b) for _, b in pairs]).astype(np.uint8)).to(dev)
    rows = [(k, 1, k, 1, 1) for k in range(len(pairs))]
    for spacing in ((1.0, 1.0, 1.0), ANISO):
        work, _, _ = _check_all(pred, label, rows, spacing)
        assert work["counts"].tolist() == [list(p) for p in pairs]
    # the same planes as volumes of depth 5 (the three-term form), sizes 5 .. 5 (2T + 1) a side
    _check_all(pred, label, [(5 * k, 1, 5 * k, 1, 5) for k in range(5)], ANISO)


def test_statistics_positions(dev):
    """n = 1 and n = 2 a side, a position 0.95 (n - 1) that is an integer (21 values: 19) and ones that are not, and a 95th
    percentile that lies among the other direction's values (a far island on one side only)"""
    H, W = 64, 64
    rng = np.random.default_rng(8)
    counts = [(1, 1), (1, 2), (2, 1), (2, 2), (11, 10), (10, 11), (20, 1), (7, 30), (41, 40), (100, 101)]
    P = np.stack([_isolated(rng, H, W, a) for a, _ in counts])
    G = np.stack([_isolated(rng, H, W, b) for _, b in counts])
    far_p, far_g = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)      # P: a block; G: the block and an island far away
    far_p[4:14, 4:14] = True
    far_g[4:14, 4:14] = True
    far_g[50:60, 50:60] = True
    P, G = np.concatenate([P, far_p[None], far_g[None]]), np.concatenate([G, far_g[None], far_p[None]])
    pred, label = torch.from_numpy(P.astype(np.uint8)).to(dev), torch.from_numpy(G.astype(np.uint8)).to(dev)
    rows = [(k, 1, k, 1, 1) for k in range(len(P))]
    for spacing in ((1.0, 1.0, 1.0), (1.0, 0.7, 0.9)):
        _, table, refs = _check_all(pred, label, rows, spacing)
        assert (0.95 * (11 + 10 - 1)) == 19.0 and table[4, 3] == np.sort(np.sqrt(np.concatenate(
            [refs[4]["d2_p"], refs[4]["d2_g"]]).astype(np.float64)))[19]
        far = refs[10]
        assert far["d2_p"].max() == 0 and table[10, 3] > 0 and table[10, 5] == 0 and table[10, 6] > 0      # all of hd95 is G's
        assert table[10, 2] == table[11, 2] and table[10, 3] == table[11, 3] and table[10, 5] == table[11, 6]


def test_largest_offsets_ties_and_empty_sides(dev):
    from protosam_amd import ops
    H, W = 2250, 1500
    pred = torch.zeros((2, H, W), dtype=torch.uint8, device=dev)
    label = torch.zeros((2, H, W), dtype=torch.uint8, device=dev)
    pred[0, 0, 0] = 1
    label[0, H - 1, W - 1] = 1
    pred[1, 0, W - 1] = 1
    label[1, H - 1, 0] = 1
    rows = [(0, 1, 0, 1, 1), (1, 1, 1, 1, 1), (0, 1, 0, 1, 2)]
    for spacing in ((1.0, 1.0, 1.0), (3.0, 0.78125, 0.6), (1.0, 1000.0, 1e-3)):
        work, table, refs = _check_all(pred, label, rows, spacing)
        dx, dy = np.float32(W - 1) * np.float32(spacing[2]), np.float32(H - 1) * np.float32(spacing[1])
        assert work["d2"][0] == dx * dx + dy * dy and table[0, 2] == np.sqrt(np.float64(work["d2"][0]))
    # ties: four ground-truth voxels at the same distance from one predicted voxel, and the other way round
    p = torch.zeros((1, 33, 33), dtype=torch.uint8, device=dev)
    g = torch.zeros((1, 33, 33), dtype=torch.uint8, device=dev)
    p[0, 16, 16] = 1
    for y, x in ((16, 6), (16, 26), (6, 16), (26, 16)):
        g[0, y, x] = 1
    _, table, _ = _check_all(p, g, [(0, 1, 0, 1, 1)], (1.0, 1.0, 1.0))
    assert table[0, 2:7].tolist() == [10.0] * 5
    # an empty other side: +inf for every point of the side that is there, NaN in the table, and the counts say which side
    work, table = _chain(p, torch.zeros_like(g), [(0, 1, 0, 1, 1)], ANISO, 16)
    assert work["counts"].tolist() == [[1, 0]] and np.isposinf(work["d2"][0]) and np.isnan(table[0, 2:7]).all() and table[0, 7] == 0
    work, table = _chain(torch.zeros_like(p), g, [(0, 1, 0, 1, 1)], ANISO, 16)
    assert work["counts"].tolist() == [[0, 4]] and np.isposinf(work["d2"][:4]).all() and np.isnan(table[0, 2:7]).all()
    assert ops.SURFACE_BAD_ROW == 2
    dev_rows = torch.tensor([(0, 1, 0, 1, 1), (1, 1, 0, 1, 1), (0, 1, -1, 1, 1), (0, 1, 0, 1, 2), (0, 1, 0, 1, 0)], dtype=torch.int32, device=dev)
    work, table = _chain(p, g, dev_rows, ANISO, 64, max_depth=1)                 # device rows are checked by the kernel
    assert work["status"].tolist() == [0, 2, 2, 2, 2] and (work["counts"][1:] == 0).all()
    sr.check_row(table[0], sr.reference(p.cpu().numpy() == 1, g.cpu().numpy() == 1, ANISO)["row"])
    assert table[1:, 7].tolist() == [2.0] * 4 and np.isnan(table[1:, 2:7]).all()


# ---- capacity ---------------------------------------------------------------------------------------------------------------------
def _guarded(dev, n, dtype, poison):
    t = torch.full((n + 2 * GUARD,), poison, dtype=dtype, device=dev)
    return t, t[GUARD:GUARD + n]


def _guarded_chain(pred, label, rows, spacing, cap):
    """the chain through the C ABI on buffers of the test's own, each between two poisoned guard regions -> host work, table; the
    guards are checked here"""
    from protosam_amd import _lib, ops
    dev = pred.device
    n, (H, W) = len(rows), pred.shape[-2:]
    md = max(r[4] for r in rows)
    rows_t = torch.tensor(rows, dtype=torch.int32, device=dev)
    bufs = {}
    for name, size, dt, poison in (("counts", 2 * n, torch.int32, POISON32), ("offsets", 2 * n + 1, torch.int32, POISON32),
                                   ("tiles", 2 * n + 1, torch.int32, POISON32), ("status", n, torch.int32, POISON32),
                                   ("cursors", 2 * n, torch.int32, POISON32), ("points", cap, torch.int32, POISON32),
                                   ("d2", cap, torch.int32, POISON32), ("keys", cap, torch.int64, POISON64),
                                   ("table", 8 * n, torch.int64, POISON64)):
        bufs[name] = _guarded(dev, size, dt, poison)
    v = {k: b[1] for k, b in bufs.items()}
    L, s = _lib.lib(), torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()      # noqa: E731
    st = L.psam_surface_points(p(pred), 2, pred.shape[0], pred.stride(0), p(label), 2, label.shape[0], label.stride(0), H, W, md,
                               p(rows_t), n, p(v["counts"]), p(v["offsets"]), p(v["tiles"]), p(v["status"]), p(v["cursors"]),
                               p(v["points"]), cap, s)
    assert st == 0
    st = L.psam_surface_dist(p(v["points"]), p(v["offsets"]), p(v["tiles"]), n, H, W, md, spacing[0], spacing[1], spacing[2], cap,
                             p(v["d2"]), p(v["keys"]), s)
    assert st == 0
    filled = v["keys"] != POISON64                                  # what the kernel did not write sorts to the end
    keys = torch.where(filled, v["keys"], torch.full_like(v["keys"], 0x7fffffffffffffff))
    st = L.psam_surface_stats(p(torch.sort(keys)[0]), 2, p(v["counts"]), p(v["offsets"]), p(v["status"]), n, p(v["table"]), s)
    assert st == 0
    torch.cuda.synchronize()
    for name, (whole, view) in bufs.items():
        poison = POISON64 if whole.dtype == torch.int64 else POISON32
        assert bool((whole[:GUARD] == poison).all()) and bool((whole[GUARD + view.numel():] == poison).all()), name
    host = {k: t.cpu().numpy() for k, t in v.items()}
    host["d2"], host["counts"] = host["d2"].view(np.float32), host["counts"].reshape(n, 2)
    return host, host["table"].view(np.float64).reshape(n, 8), int(filled.sum())


def test_capacity_flags_guards_and_recompute(dev):
    from protosam_amd import ops
    from protosam_amd.metrics import surface_table
    pred, label, rows = _blob_rows(dev, 37, 53, 2, seed=3)
    roomy_work, roomy, refs = _check_all(pred, label, rows, ANISO)
    sizes = [len(r["points_p"]) + len(r["points_g"]) for r in refs]
    total = sum(sizes)
    ends = np.cumsum(sizes)
    for fit in (0, 1, 3, len(rows)):                              # a pool that ends inside row `fit`: rows 0 .. fit - 1 fit
        cap = total if fit == len(rows) else int(ends[fit]) - 1
        want_status = [0 if (k < fit or sizes[k] == 0) else 1 for k in range(len(rows))]
        work, table, written = _guarded_chain(pred, label, rows, ANISO, max(cap, 1))
        assert work["status"].tolist() == want_status, (fit, work["status"])
        assert work["counts"].tolist() == roomy_work["counts"].tolist()       # the true counts whatever the capacity
        assert written == (int(ends[fit - 1]) if fit else 0)                   # nothing of a flagged row is written
        assert (work["points"][written:] == POISON32).all() and (work["d2"][written:].view(np.uint32) == POISON32).all()
        for k in range(len(rows)):
            if want_status[k] == 0:
                assert np.array_equal(table[k].view(np.uint64), roomy[k].view(np.uint64)), (fit, k)
            else:
                assert table[k, :2].tolist() == roomy[k, :2].tolist() and np.isnan(table[k, 2:7]).all() and table[k, 7] == 1
        # the caller-facing table: only the flagged rows run again, and the result is the roomy one bit for bit
        full = surface_table(pred, label, rows, ANISO, cap=max(cap, 1))
        assert np.array_equal(full.view(np.uint64), roomy.view(np.uint64)), fit
        assert np.array_equal(surface_table(pred, label, rows, ANISO, table=table).view(np.uint64), roomy.view(np.uint64))
    # two runs and two other roomy capacities: the same bits
    for cap in (total, total, total + 1, 3 * total + 777):
        t = ops.surface_distances(pred, label, rows, ANISO, cap=cap)
        assert np.array_equal(t.cpu().numpy().view(np.uint64), roomy.view(np.uint64)), cap
    out = torch.zeros((len(rows) + 1, 8), dtype=torch.float64, device=dev)
    assert ops.surface_distances(pred, label, rows, ANISO, out=out[:len(rows)]).data_ptr() == out.data_ptr()       # default cap
    assert np.array_equal(out[:len(rows)].cpu().numpy().view(np.uint64), roomy.view(np.uint64)) and bool((out[-1] == 0).all())


def test_refused_arguments_raise_before_any_launch(dev):
    from protosam_amd import _lib, ops
    m = torch.zeros((4, 8, 8), dtype=torch.uint8, device=dev)
    ok = [(0, 1, 0, 1, 1)]
    for rows in ([(4, 1, 0, 1, 1)], [(0, 1, 4, 1, 1)], [(3, 1, 0, 1, 2)], [(0, 1, 2, 1, 3)], [(-1, 1, 0, 1, 1)], [(0, 1, 0, 1, 0)],
                 [(0, 1, 0, 1)], [], [(0, 1 << 40, 0, 1, 1)]):
        with pytest.raises(ValueError):
            ops.surface_distances(m, m, rows)
    with pytest.raises(ValueError):
        ops.surface_distances(m, m[:, :4], ok)
    with pytest.raises(ValueError):
        ops.surface_distances(m, m, ok, cap=0)
    with pytest.raises(ValueError):
        ops.surface_distances(m, m, ok, spacing=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError):
        ops.surface_distances(m, m, torch.tensor(ok, dtype=torch.int32, device=dev))           # device rows without max_depth
    with pytest.raises(TypeError):
        ops.surface_distances(m.double(), m, ok)
    huge = torch.zeros(1, dtype=torch.uint8, device=dev).expand(1, 65536, 32768)                # 2^31 voxels in a plane
    with pytest.raises(ValueError):
        ops.surface_distances(huge, huge, ok)
    with pytest.raises(ValueError):
        ops.surface_distances(huge[:, :4096], huge[:, :4096], [(0, 1, 0, 1, 1)], max_depth=16)  # depth * H * W outside int32
    L = _lib.lib()
    p = m.data_ptr()
    assert L.psam_surface_points(p, 2, 4, 64, p, 2, 4, 64, 8, 8, 1, p, 1, p, p, p, p, p, 0, 16, 0) == 1             # a null pointer
    assert L.psam_surface_points(p, 2, 4, 64, p, 2, 4, 64, 8, 8, 1, p, 1, p, p, p, p, p, p, 0, 0) == 1              # cap 0
    assert L.psam_surface_points(p, 7, 4, 64, p, 2, 4, 64, 8, 8, 1, p, 1, p, p, p, p, p, p, 16, 0) == 1             # dtype
    assert L.psam_surface_dist(p, p, p, 1, 8, 8, 1, 1.0, float("nan"), 1.0, 16, p, 0, 0) == 1
    assert L.psam_surface_dist(p, p, p, 1, 8, 8, 1, 1.0, 1.0, -1.0, 16, p, 0, 0) == 1
    assert L.psam_surface_stats(p, 3, p, p, p, 1, p, 0) == 1
    torch.cuda.synchronize()
    assert bool((m == 0).all())


# ---- callers ----------------------------------------------------------------------------------------------------------------------
def _three_organ_case(dev, Z=4, S=512):
    from protosam_amd.runner import support_set
    from protosam_amd.synth import ellipse_mask, synth_volume
    vol, qlab = synth_volume(Z, S, seed=0)
    svol, slab = synth_volume(Z, S, seed=1)
    sup_imgs, sup_masks = support_set(svol.to(dev), slab.to(dev))
    extras = [torch.from_numpy(ellipse_mask(S, 0.3, 0.7, 0.1, 0.12)[None]).to(dev),
              torch.from_numpy(ellipse_mask(S, 0.75, 0.3, 0.08, 0.1)[None]).to(dev)]
    labels = (qlab > 0).to(torch.uint8)
    for c, e in enumerate(extras):
        labels[(labels == 0) & (e.cpu()[0] > 0)[None]] = 2 + c
    return vol.to(dev), labels.to(dev), sup_imgs, sup_masks, extras


def test_evaluate_slices_classes_with_surfaces_and_scan_surfaces(dev):
    from test_protosam_gpu import _build
    from protosam_amd import ops
    from protosam_amd.metrics import score_surfaces, surface_rows, surface_table
    from protosam_amd.runner import evaluate_slices_classes, score_scan_surfaces
    S, Z, classes, spacing = 512, 4, [1, 2, 3], (2.5, 0.78125, 0.78125)
    model, _ = _build(dev, "random:vit_b:1234:2", 2, use_bbox=True, use_points=True, point_mode="both")
    vol, labels, sup_imgs, sup_masks, extras = _three_organ_case(dev, Z, S)
    per_part = [[m] + extras for m in sup_masks]
    zs = list(range(Z))
    keep0 = torch.full((Z, 3, S, S), 7, dtype=torch.uint8, device=dev)
    plain = evaluate_slices_classes(model, vol, labels, sup_imgs, per_part, zs, classes, dev, batch=3, keep=keep0)
    keep = torch.full((Z, 3, S, S), 7, dtype=torch.uint8, device=dev)
    roomy = 2 * 3 * 3 * S * S                                      # the masks of a seeded random model are ragged: room for every voxel
    got = evaluate_slices_classes(model, vol, labels, sup_imgs, per_part, zs, classes, dev, batch=3, keep=keep,
                                  surface=dict(spacing=spacing, cap=roomy))
    assert len(plain) == 2 and len(got) == 3
    table, st, surf = got
    assert torch.equal(table, plain[0]) and st == plain[1] and torch.equal(keep, keep0)          # nothing else changes
    assert surf.is_cuda and surf.dtype == torch.float64 and tuple(surf.shape) == (Z * 3, 8)
    rows = surface_rows(Z, classes, label_planes=zs).tolist()
    want = ops.surface_distances(keep, labels, rows, spacing, cap=2 * Z * 3 * S * S).cpu().numpy()
    assert np.array_equal(surf.cpu().numpy().view(np.uint64), want.view(np.uint64))
    sc = score_surfaces(surf)
    print(f"per-slice surfaces: {len(sc['rows'])} of {len(rows)} rows scored, mean HD95 {sc['mean_hd95']:.3f}, mean ASSD "
          f"{sc['mean_assd']:.3f}; empty pred {sc['empty_pred']}, empty gt {sc['empty_gt']}; largest surfaces "
          f"{int(sc['n_pred'].max())} / {int(sc['n_gt'].max())}")
    assert not sc["overflowed"] and not sc["bad_rows"] and len(sc["rows"]) >= 3
    # the default pool: rows that do not fit are flagged, and surface_table completes them to the same bits
    _, _, flagged = evaluate_slices_classes(model, vol, labels, sup_imgs, per_part, zs, classes, dev, batch=3, surface=dict(spacing=spacing))
    flagged = flagged.cpu().numpy()
    same = flagged[:, 7] == 0
    assert np.array_equal(flagged[same].view(np.uint64), want[same].view(np.uint64)) and (flagged[~same, 7] == 1).all()
    assert np.array_equal(flagged[:, :2], want[:, :2])
    assert np.array_equal(surface_table(keep, labels, rows, spacing, table=flagged).view(np.uint64), want.view(np.uint64))
    masks_np, labels_np = keep.cpu().numpy(), labels.cpu().numpy()
    cheapest = sorted(sc["rows"], key=lambda k: sc["n_pred"][k] * sc["n_gt"][k])[:3]
    for k in cheapest:                                            # against the reference on the kept masks
        pp, pv, lp, lv, _ = rows[k]
        ref = sr.reference(masks_np.reshape(-1, S, S)[pp:pp + 1] == pv, labels_np[lp:lp + 1] == lv, spacing)
        sr.check_row(want[k], ref["row"])
    # the scan form: one row per class, depth Z: surface sizes against numpy on the whole volume, every metric against the 3-D
    # reference on a 40 x 40 window at each organ's centre (the all-pairs reference in numpy does not finish the ragged whole in seconds)
    scan = score_scan_surfaces(keep, labels, classes, spacing)
    assert scan.shape == (3, 8) and (scan[:, 7] == 0).all() and np.isfinite(scan[:, 2]).any()
    for c, (cy, cx) in enumerate(((0.5, 0.48), (0.3, 0.7), (0.75, 0.3))):
        assert scan[c, 0] == sr.surface_mask(masks_np[:, c] == 1).sum() and scan[c, 1] == sr.surface_mask(labels_np == classes[c]).sum()
        y0, x0 = int(cy * S) - 20, int(cx * S) - 20
        window = score_scan_surfaces(keep[:, c:c + 1, y0:y0 + 40, x0:x0 + 40], labels[:, y0:y0 + 40, x0:x0 + 40], [classes[c]], spacing)
        ref = sr.reference(masks_np[:, c, y0:y0 + 40, x0:x0 + 40] == 1, labels_np[:, y0:y0 + 40, x0:x0 + 40] == classes[c], spacing)
        assert ref["row"][1] > 0
        sr.check_row(window[0], ref["row"])
    part = score_scan_surfaces(keep[1:3], labels, classes, spacing, zs=[1, 2])          # a range of slices against its label planes
    assert np.array_equal(part.view(np.uint64), score_scan_surfaces(keep[1:3], labels[1:3], classes, spacing).view(np.uint64))
