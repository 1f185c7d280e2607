"""CPU: tests/volume_regions_reference.py is pinned to scipy.ndimage.label + numpy.bincount over the case list the GPU test uses;
every injected fault fails at least one case of that list; ops.volume_regions refuses bad arguments before it needs a device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import volume_regions_reference as vr  # noqa: E402

CASES = vr.cases()
NAMES = [c[0] for c in CASES]


def _scipy_expected(vols, conn, min_voxels, keep_largest):
    """out, info and labels from scipy.ndimage.label + numpy.bincount, the route a user takes on the host"""
    import scipy.ndimage as ndi
    st = ndi.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn])
    R = vols.shape[0]
    out, labels, info = np.zeros(vols.shape, np.uint8), np.zeros(vols.shape, np.int32), np.full((R, 12), -1, np.int64)
    for r in range(R):
        lab, n = ndi.label(vols[r] != 0, structure=st)
        sizes = np.bincount(lab.reshape(-1), minlength=n + 1)[1:]
        stay = sizes >= min_voxels
        best = int(np.argmax(sizes)) if n else -1              # (argmax: the first of equal maxima = the lowest label)
        if keep_largest:
            only = np.zeros(n, dtype=bool)
            if n and stay[best]:
                only[best] = True
            stay = only
        keep = np.concatenate([[False], stay])[lab]
        out[r], labels[r] = keep, lab
        info[r, :6] = (n, stay.sum(), (lab > 0).sum(), keep.sum(), sizes[best] if n else 0,
                       np.flatnonzero(lab.reshape(-1) == best + 1)[0] if n else -1)
        if keep.any():
            zz, yy, xx = np.nonzero(keep)
            info[r, 6:] = (zz.min(), yy.min(), xx.min(), zz.max(), yy.max(), xx.max())
    return out, info, labels


def test_neighbour_lists_are_scipys_structures():
    ndi = pytest.importorskip("scipy.ndimage")
    for conn, rank in ((6, 1), (18, 2), (26, 3)):
        st = ndi.generate_binary_structure(3, rank)
        st[1, 1, 1] = False
        want = sorted(tuple(int(i) - 1 for i in p) for p in zip(*np.nonzero(st)))
        assert sorted(vr.offsets(conn)) == want and len(want) == conn
        assert all(o < (0, 0, 0) for o in vr.EARLIER[conn]) and len(vr.EARLIER[conn]) * 2 == conn


@pytest.mark.parametrize("name", NAMES)
def test_reference_is_scipys(name):
    pytest.importorskip("scipy.ndimage")
    _, vols, conn, mv, kl = CASES[NAMES.index(name)]
    got = vr.expected(name)
    out, info, labels = _scipy_expected(vols, conn, mv, kl)
    assert np.array_equal(got["labels"], labels)
    assert np.array_equal(got["out"], out)
    assert np.array_equal(got["info"], info), (got["info"], info)


def test_case_list_covers_the_shapes():
    ws = {c[1].shape[3] for c in CASES}
    hs = {c[1].shape[2] for c in CASES}
    ds = {c[1].shape[1] for c in CASES}
    rs = {c[1].shape[0] for c in CASES}
    assert {1, 63, 64, 65, 257} <= ws and {1, 2, 5} <= hs and {1, 2, 3, 5} <= ds and {1, 3} <= rs
    assert {c[2] for c in CASES} == {6, 18, 26}


def test_patterns_are_what_they_claim():
    for conn in (6, 18, 26):
        for w in (65, 257):
            info = vr.expected(f"pairs{w}_c{conn}")["info"]
            linked = [o in vr.offsets(conn) for _ in range(2) for o in vr.offsets(26)]
            assert (info[:, 0] == np.where(linked, 1, 2)).all()
    assert vr.expected("serpentine_c6")["info"][0, 0] == 1 and vr.expected("serpentine_c26")["info"][0, 0] == 1
    board = next(c[1] for c in CASES if c[0] == "checkerboard_c6")
    assert vr.expected("checkerboard_c6")["info"][0, 0] == board.sum()
    assert vr.expected("checkerboard_c18")["info"][0, 0] == 1 and vr.expected("checkerboard_c26")["info"][0, 0] == 1
    assert (vr.expected("empty")["info"][:, :6] == [0, 0, 0, 0, 0, -1]).all() and (vr.expected("empty")["info"][:, 6:] == -1).all()
    ties = vr.expected("ties")["info"]
    assert ties[0, 4] == 4 and ties[0, 5] == 3 * 65 + 2 and ties[1, 4] == 3 and ties[1, 5] == 4 * 65 + 62 and (ties[:, 1] == 1).all()
    assert [int(vr.expected(f"min{mv}")["info"][0, 3]) for mv in (4, 5, 6)] == [5, 5, 0]
    assert [int(vr.expected(f"min{mv}_small")["info"][0, 3]) for mv in (1, 2, 3)] == [7, 7, 5]
    for name in ("min_empties", "min_empties_largest"):
        e = vr.expected(name)
        assert not e["out"].any() and e["info"][0].tolist() == [2, 0, 7, 0, 5, (1 * 5 + 2) * 65 + 60] + [-1] * 6


@pytest.mark.parametrize("fault", vr.FAULTS)
def test_every_fault_fails_a_case(fault):
    caught = []
    for name, vols, conn, mv, kl in CASES:
        bad, good = vr.reference(vols, conn, mv, kl, faults=(fault,)), vr.expected(name)
        if any(not np.array_equal(bad[k], good[k]) for k in ("out", "info", "labels")):
            caught.append(name)
            break
    assert caught, f"fault {fault} passes every case"


def test_refused_arguments_without_a_device():
    import torch
    from protosam_amd import ops
    v = torch.zeros((2, 3, 4, 5), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        ops.volume_regions(v)                                   # a CPU tensor
    with pytest.raises(TypeError):
        ops.volume_regions(v.to(torch.int32))
    with pytest.raises(TypeError):
        ops.volume_regions(None)
    for kw in (dict(connectivity=8), dict(connectivity=4), dict(min_voxels=-1), dict(min_voxels=1.5), dict(keep_largest=2),
               dict(layout="czhw")):
        with pytest.raises(ValueError):
            ops.volume_regions(v, **kw)
    with pytest.raises(ValueError):
        ops.volume_regions(v[0, 0])                             # [H, W]
    with pytest.raises(ValueError):
        ops.volume_regions(v[0], layout="zchw")
    with pytest.raises(ValueError):
        ops.volume_regions(v[..., ::2])                         # planes that are not contiguous
    with pytest.raises(ValueError):
        ops.volume_regions(torch.zeros((0, 3, 4, 5), dtype=torch.uint8))


def test_workspace_and_chunk():
    from protosam_amd import ops
    n = 3 * 5 * 65
    assert ops.volume_regions_workspace(3, 5, 65, 2) == 2 * (8 * n + 64)
    assert ops.volume_regions_workspace(3, 5, 65, 2, labels=True) == 2 * (8 * n + 64 + 4 * ((n + 255) // 256))
    assert ops.volume_regions_chunk(4, 3, 5, 65) == 4 and ops.volume_regions_chunk(4, 3, 5, 65, budget=1) == 1
    assert ops.volume_regions_chunk(4, 3, 5, 65, budget=2 * ops.volume_regions_workspace(3, 5, 65, 1, labels=True)) == 2
    for bad in ((0, 5, 65), (1 << 11, 1 << 10, 1 << 10), (1 << 24, 1, 1)):
        with pytest.raises(ValueError):
            ops.volume_regions_workspace(*bad, 1)
    with pytest.raises(ValueError):
        ops.volume_regions_workspace(3, 5, 65, 0)
    assert len(ops.VOLREG_COLS) == 12 and ops.VOLREG_COLS == vr.COLS
    rows = ops.volume_regions_table(np.array([[2, 1, 7, 5, 5, 9, 1, 2, 60, 1, 2, 64], [0, 0, 0, 0, 0, -1] + [-1] * 6]))
    assert rows[0]["voxels_dropped"] == 2 and rows[0]["box"] == (1, 2, 60, 1, 2, 64) and rows[1]["box"] is None
