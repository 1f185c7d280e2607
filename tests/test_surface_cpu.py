"""CPU: tests/surface_reference.py is pinned to scipy (binary_erosion, distance_transform_edt); every injected fault fails the checks
the GPU test applies to the kernels; the host halves (metrics.surface_rows, metrics.score_surfaces, the argument checks of the ops
wrappers) on tables written by hand."""
import numpy as np
import pytest

import surface_reference as sr

CASES = [((1, 37, 53), (1.0, 0.7, 0.7)), ((5, 23, 29), (2.5, 0.7, 0.7)), ((2, 16, 16), (3.0, 0.78125, 0.78125))]


def _pair(shape, seed):
    return sr.blobs(shape, seed), sr.blobs(shape, seed + 100)


@pytest.mark.parametrize("shape,spacing", CASES)
def test_surfaces_are_scipys(shape, spacing):
    ndi = pytest.importorskip("scipy.ndimage")
    for seed in range(3):
        for m in _pair(shape, seed):
            vol = m[0] if shape[0] == 1 else m
            want = vol ^ ndi.binary_erosion(vol, ndi.generate_binary_structure(vol.ndim, 1))
            assert np.array_equal(sr.surface_mask(m).reshape(vol.shape), want)
            assert want.any() and ((want != vol).any() or shape[0] == 2)     # (two planes have no interior)
    full = np.ones(shape, dtype=bool)                            # a full array: the faces only; a single voxel: itself
    vol = full[0] if shape[0] == 1 else full
    assert np.array_equal(sr.surface_mask(full).reshape(vol.shape), vol ^ ndi.binary_erosion(vol, ndi.generate_binary_structure(vol.ndim, 1)))
    one = np.zeros(shape, dtype=bool)
    one[0, 3, 4] = True
    assert sr.surface_points(one).tolist() == [3 * shape[2] + 4] and sr.surface_points(~full).size == 0


@pytest.mark.parametrize("shape,spacing", CASES)
def test_distances_are_scipys(shape, spacing):
    """sqrt(d2) equals distance_transform_edt exactly at unit spacing (both are sqrt of an exact integer in float64) and stays
    within 2^-22 relative at anisotropic spacing: per term three float32 roundings (the product with the spacing, the square, and
    the spacing's own conversion counted twice) and the two additions, each 2^-24 relative on non-negative terms, so at most
    8 * 2^-24 on d2, halved by the square root: 2^-22. (Observed on these cases: 9.4e-8, below 2^-23.)"""
    ndi = pytest.importorskip("scipy.ndimage")
    worst = 0.0
    for seed in range(3):
        P, G = _pair(shape, seed)
        for sp in ((1.0, 1.0, 1.0), spacing):
            ref = sr.reference(P, G, sp)
            for mine, other, d2 in ((P, G, ref["d2_p"]), (G, P, ref["d2_g"])):
                so, sm = sr.surface_mask(other), sr.surface_mask(mine)
                vol, sampling = (so[0], sp[1:]) if shape[0] == 1 else (so, sp)
                edt = ndi.distance_transform_edt(~vol, sampling=sampling).reshape(shape)[sm]
                got = np.sqrt(d2.astype(np.float64))
                if sp == (1.0, 1.0, 1.0):
                    assert np.array_equal(got, edt)
                else:
                    nz = edt > 0
                    assert np.array_equal(got[~nz], edt[~nz])
                    rel = np.abs(got[nz] - edt[nz]) / edt[nz]
                    worst = max(worst, float(rel.max()) if rel.size else 0.0)
                    assert (rel <= 2.0 ** -22).all(), rel.max()
    print(f"{shape} {spacing}: worst relative difference to scipy's EDT {worst:.2e}")


def _apply_checks(got, ref):
    """what test_surface_gpu.py asks of the kernels' output for one row"""
    sr.check_points(got["points_p"], got["points_g"], ref)
    sr.check_d2(got["points_p"], got["d2_p"], got["points_g"], got["d2_g"], ref)
    sr.check_row(got["row"], ref["row"])


def _fault_case(fault):
    if fault == "z_neighbours_at_depth_1":
        shape, spacing = (1, 37, 53), (1.0, 0.7, 0.7)
    elif fault == "fma":
        shape, spacing = (5, 23, 29), FMA_SPACING
    else:
        shape, spacing = (5, 23, 29), (2.5, 0.7, 0.9)
    P, G = _pair(shape, 2)
    if fault == "hd_one_direction":                              # the far voxel is on the ground truth's side
        P = P & G
        G = G.copy()
        G[0, 0, 0] = True
    return P, G, spacing


FMA_SPACING = (2.5, 0.7, 0.7)   # a spacing at which fma(dz, dz, fma(dy, dy, dx*dx)) differs from the separately rounded sum (found by trial)


def test_checks_pass_on_the_reference_itself():
    for fault in sr.FAULTS:
        P, G, spacing = _fault_case(fault)
        ref = sr.reference(P, G, spacing)
        shuffled = dict(ref)                                      # the kernels give the points in any order
        for side in "pg":
            perm = np.random.default_rng(3).permutation(len(ref["points_" + side]))
            shuffled["points_" + side], shuffled["d2_" + side] = ref["points_" + side][perm], ref["d2_" + side][perm]
        _apply_checks(shuffled, ref)


@pytest.mark.parametrize("fault", sr.FAULTS)
def test_injected_fault_fails_the_checks(fault):
    P, G, spacing = _fault_case(fault)
    ref = sr.reference(P, G, spacing)
    bad = sr.reference(P, G, spacing, faults=(fault,))
    with pytest.raises(AssertionError):
        _apply_checks(bad, ref)
    # and the part of the output the fault is about is what differs
    if fault in ("eight_neighbours", "edge_not_surface", "z_neighbours_at_depth_1"):
        with pytest.raises(AssertionError):
            sr.check_points(bad["points_p"], bad["points_g"], ref)
    elif fault in ("swap_sy_sz", "fma"):
        sr.check_points(bad["points_p"], bad["points_g"], ref)
        with pytest.raises(AssertionError):
            sr.check_d2(bad["points_p"], bad["d2_p"], bad["points_g"], bad["d2_g"], ref)
    else:
        sr.check_d2(bad["points_p"], bad["d2_p"], bad["points_g"], bad["d2_g"], ref)
        with pytest.raises(AssertionError):
            sr.check_row(bad["row"], ref["row"])


def test_percentile_positions():
    """table_row on hand-made sets: n = 1, n = 2, an integer position 0.95 (n - 1), a fractional one, and a 95th percentile that
    falls among the other direction's values"""
    f = lambda *v: np.array(v, dtype=np.float32)   # noqa: E731
    r = sr.table_row(f(4.0), f(9.0))
    assert r[:2].tolist() == [1, 1] and r[2] == 3.0 and abs(r[3] - (2 + 0.95)) < 1e-15 and r[4] == 2.5
    r = sr.table_row(f(0.0, 1.0, 4.0, 9.0, 16.0, 25.0, 36.0, 49.0, 64.0, 81.0, 100.0), f(*[float(i * i) for i in range(11, 21)]))
    assert r[3] == 19.0                                          # 21 values 0 .. 20: position 0.95 * 20 = 19 exactly
    r = sr.table_row(f(1.0, 1.0, 1.0), f(400.0, 900.0))         # union 1, 1, 1, 20, 30: position 3.8 -> 20 + 0.8 * 10, all of G's
    assert abs(r[3] - 28.0) < 1e-13 and r[2] == 30.0 and r[5] == 1.0 and r[6] == 25.0
    e = sr.table_row(f(), f(1.0))
    assert e[:2].tolist() == [0, 1] and np.isnan(e[2:7]).all() and e[7] == 0


# ---- host halves ------------------------------------------------------------------------------------------------------------------
def test_surface_rows():
    from protosam_amd.metrics import class_rows, surface_rows
    assert surface_rows(3).tolist() == [[0, 1, 0, 1, 1], [1, 1, 1, 1, 1], [2, 1, 2, 1, 1]]
    for classes, lp in ((None, None), ([3, 5], None), ([3, 5], [7, 2, 4]), (None, [7, 2, 4])):
        got = surface_rows(3, classes, label_planes=lp)
        assert got.dtype == np.int32 and np.array_equal(got[:, :4], class_rows(3, classes, label_planes=lp)) and (got[:, 4] == 1).all()
    assert surface_rows(1, [1, 2, 6], depth=40).tolist() == [[0, 1, 0, 1, 40], [40, 1, 0, 2, 40], [80, 1, 0, 6, 40]]
    assert surface_rows(2, None, depth=4, label_value=9).tolist() == [[0, 1, 0, 9, 4], [4, 1, 4, 9, 4]]
    assert surface_rows(2, [2], label_planes=[10, 30], depth=4, pred_value=3).tolist() == [[0, 3, 10, 2, 4], [4, 3, 30, 2, 4]]
    with pytest.raises(ValueError):
        surface_rows(2, label_planes=[0])
    with pytest.raises(ValueError):
        surface_rows(2, depth=0)


def test_score_surfaces_on_a_hand_written_table():
    from protosam_amd.metrics import score_surfaces
    nan = float("nan")
    table = np.array([[10, 12, 5.0, 4.0, 1.5, 1.0, 2.0, 0],
                      [0, 7, nan, nan, nan, nan, nan, 0],           # empty prediction
                      [4, 0, nan, nan, nan, nan, nan, 0],           # empty ground truth
                      [0, 0, nan, nan, nan, nan, nan, 0],           # both
                      [900, 800, nan, nan, nan, nan, nan, 1],       # overflowed: true counts, no metrics
                      [6, 6, 3.0, 2.0, 0.5, 0.25, 0.75, 0],
                      [0, 0, nan, nan, nan, nan, nan, 2]])          # a row outside the planes
    s = score_surfaces(table, cases=["a", "a", "a", "b", "b", "b", "b"])
    assert s["rows"] == [0, 5] and s["empty_pred"] == [1, 3] and s["empty_gt"] == [2, 3]
    assert s["overflowed"] == [4] and s["bad_rows"] == [6]
    assert s["hd"].tolist() == [5.0, 3.0] and s["hd95"].tolist() == [4.0, 2.0] and s["assd"].tolist() == [1.5, 0.5]
    assert s["asd_pg"].tolist() == [1.0, 0.25] and s["asd_gp"].tolist() == [2.0, 0.75]
    assert s["mean_hd"] == 4.0 and s["mean_hd95"] == 3.0 and s["mean_assd"] == 1.0
    assert s["hd95_cases"] == {"a": 4.0, "b": 2.0} and s["assd_cases"] == {"a": 1.5, "b": 0.5}
    assert s["n_pred"].tolist() == [10, 0, 4, 0, 900, 6, 0] and s["n_gt"].tolist() == [12, 7, 0, 0, 800, 6, 0]
    every = sorted(s["rows"] + s["empty_pred"] + s["empty_gt"] + s["overflowed"] + s["bad_rows"])
    assert sorted(set(every)) == list(range(7))                   # no row is dropped silently
    none = score_surfaces(table[1:5])
    assert none["rows"] == [] and np.isnan(none["mean_hd95"]) and none["hd"].size == 0 and none["hd95_cases"] == {}
    import torch
    assert score_surfaces(torch.from_numpy(table))["rows"] == [0, 5]


def test_wrapper_argument_checks_need_no_device():
    import torch
    from protosam_amd import ops
    assert ops.SURF_COLS == sr.COLS and ops.SURFACE_TILE == 256
    m = torch.zeros((2, 8, 8), dtype=torch.uint8)
    for bad in ((1, 1, 0), (1, -1, 1), (float("nan"), 1, 1), (1, float("inf"), 1), (1, 1, 1e-60), (1, 1e60, 1), (1,), (1, 1, 1, 1)):
        with pytest.raises(ValueError):
            ops.surface_distances(m, m, [(0, 1, 0, 1, 1)], spacing=bad)
    with pytest.raises(RuntimeError):                            # CPU tensors are rejected as everywhere else
        ops.surface_distances(m, m, [(0, 1, 0, 1, 1)])
    with pytest.raises(RuntimeError):
        ops.surface_points(m, m, [(0, 1, 0, 1, 1)], 16)
    with pytest.raises(ValueError):
        ops.surface_points(m, m[:, :4], [(0, 1, 0, 1, 1)], 16)
    assert ops.surface_default_cap(0) == 65536 and ops.surface_default_cap(16 * 4 * 512 * 512) == 2 * 1024 * 1024
    assert ops.surface_default_cap(1 << 40) == 2 ** 31 - 2
    assert ops.surface_workspace(64, 1 << 20) == 4 * (9 * 64 + 2) + 32 * (1 << 20) + 64 * 64


def test_slice_spacing_from_the_header():
    from protosam_amd.slice_io import slice_spacing
    assert slice_spacing(None, 512) == (1.0, 1.0, 1.0)
    info = {"spacing": (0.75, 0.8, 2.5), "array_size": (40, 256, 320)}          # stored x, y, z; the array is [z, y, x]
    assert slice_spacing(info, 512) == (2.5, 0.8 * 256 / 512, 0.75 * 320 / 512)
    assert slice_spacing(info, 256) == (2.5, 0.8, 0.75 * 320 / 256)
