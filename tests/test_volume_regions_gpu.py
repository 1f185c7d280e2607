"""GPU: ops.volume_regions (csrc/volume_regions.hip) against tests/volume_regions_reference.py, exactly: out, info and labels of
every case of the shared case list, through the C ABI on poisoned buffers between guard regions and through the wrapper in both
layouts; in place, chunking, independence of the neighbouring volumes, refused arguments; runner.clean_scan / score_scan on a kept
scan with a stray island."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import volume_regions_reference as vr  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = vr.cases()
NAMES = [c[0] for c in CASES]
GUARD = 256
POISON8, POISON32, POISON64 = 0xA5, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


def _guarded(dev, n, dtype, poison):
    t = torch.full((n + 2 * GUARD,), poison, dtype=dtype, device=dev)
    return t, t[GUARD:GUARD + n]


def _cabi(dev, vols, conn, mv, kl, chunk, labels=True):
    """psam_volume_regions on buffers of the test's own: out, info, labels and scratch pre-filled with garbage, the first three
    between poisoned guard regions (checked here) -> host out, info, labels"""
    from protosam_amd import _lib, ops
    R, D, H, W = vols.shape
    n = D * H * W
    src = torch.from_numpy(vols).to(dev)
    need = ops.volume_regions_workspace(D, H, W, chunk, labels=labels)
    bufs = {"out": _guarded(dev, R * n, torch.uint8, POISON8), "info": _guarded(dev, R * 12, torch.int64, POISON64),
            "labels": _guarded(dev, R * n, torch.int32, POISON32), "scratch": _guarded(dev, (need + 7) // 8, torch.int64, POISON64)}
    v = {k: b[1] for k, b in bufs.items()}
    st = _lib.lib().psam_volume_regions(src.data_ptr(), R, D, H, W, n, H * W, conn, mv, int(kl), chunk, v["out"].data_ptr(),
                                        v["info"].data_ptr(), v["labels"].data_ptr() if labels else 0, v["scratch"].data_ptr(),
                                        need, torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    for name, (whole, view) in bufs.items():
        poison = {torch.uint8: POISON8, torch.int32: POISON32, torch.int64: POISON64}[whole.dtype]
        assert bool((whole[:GUARD] == poison).all()) and bool((whole[GUARD + view.numel():] == poison).all()), name
    if not labels:
        assert bool((v["labels"] == POISON32).all())
    assert torch.equal(src.cpu(), torch.from_numpy(vols))                      # the source is only read
    return (v["out"].cpu().numpy().reshape(vols.shape), v["info"].cpu().numpy().reshape(R, 12),
            v["labels"].cpu().numpy().reshape(vols.shape))


def _same(got, want, what=("out", "info", "labels")):
    for k, g in zip(("out", "info", "labels"), got):
        if k in what:
            assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), (k, g if k == "info" else None, want["info"])


@pytest.mark.parametrize("name", NAMES)
def test_cases_exact(dev, name):
    from protosam_amd import ops
    _, vols, conn, mv, kl = CASES[NAMES.index(name)]
    want = vr.expected(name)
    R = vols.shape[0]
    _same(_cabi(dev, vols, conn, mv, kl, chunk=R), want)
    # the slice-major layout [Z, C, H, W], read where it lies; labels come back class-major
    keep = torch.from_numpy(np.ascontiguousarray(vols.transpose(1, 0, 2, 3))).to(dev)
    out, info, labels = ops.volume_regions(keep, conn, mv, kl, labels=True, layout="zchw")
    assert out.shape == keep.shape and out.is_contiguous() and labels.shape == vols.shape and info.shape == (R, 12)
    _same((out.permute(1, 0, 2, 3).cpu().numpy(), info.cpu().numpy(), labels.cpu().numpy()), want)


def test_wrapper_forms_in_place_and_chunks(dev):
    from protosam_amd import ops
    name = "random_mid_c18"
    _, vols, conn, mv, kl = CASES[NAMES.index(name)]
    want = vr.expected(name)
    R, D, H, W = vols.shape
    src = torch.from_numpy(vols).to(dev)
    out, info = ops.volume_regions(src, conn, mv, kl)                          # class-major, no labels
    _same((out.cpu().numpy(), info.cpu().numpy(), None), want, ("out", "info"))
    for chunk in (1, 2, R):                                                    # chunk = 1 equals chunk = R, with and without labels
        _same(_cabi(dev, vols, conn, mv, kl, chunk=chunk), want)
        _same(_cabi(dev, vols, conn, mv, kl, chunk=chunk, labels=False), want, ("out", "info"))
        o, i, lab = ops.volume_regions(src, conn, mv, kl, labels=True, chunk=chunk)
        _same((o.cpu().numpy(), i.cpu().numpy(), lab.cpu().numpy()), want)
    one = ops.volume_regions(src[1], conn, mv, kl, labels=True)                # one volume [D, H, W]
    assert one[0].shape == (D, H, W) and one[2].shape == (D, H, W) and one[1].shape == (1, 12)
    _same((one[0].cpu().numpy()[None], one[1].cpu().numpy(), one[2].cpu().numpy()[None]),
          {k: want[k][1:2] for k in ("out", "info", "labels")})
    # in place equals out of place, in both layouts
    work = src.clone()
    o, i = ops.volume_regions(work, conn, mv, kl, out=work)
    assert o.data_ptr() == work.data_ptr()
    _same((work.cpu().numpy(), i.cpu().numpy(), None), want, ("out", "info"))
    keep = src.permute(1, 0, 2, 3).contiguous()
    o, i = ops.volume_regions(keep, conn, mv, kl, out=keep, layout="zchw", chunk=1)
    _same((keep.permute(1, 0, 2, 3).cpu().numpy(), i.cpu().numpy(), None), want, ("out", "info"))
    # a view with outer strides of its own: every second volume of a larger buffer
    big = torch.from_numpy(np.repeat(vols, 2, axis=0)).to(dev)
    big[1::2] = 1
    o, i = ops.volume_regions(big[0::2], conn, mv, kl)
    assert o.stride() == big[0::2].stride()
    _same((o.cpu().numpy(), i.cpu().numpy(), None), want, ("out", "info"))
    assert ops.volume_regions_table(i)[0]["voxels_dropped"] == int(want["info"][0, 2] - want["info"][0, 3])


def test_numbering_beyond_one_turn_of_the_scan(dev):
    """more than 4096 blocks of 256 voxels, so the scan of the block counts carries from turn to turn: sparse voxels (the reference
    walks set voxels only), a line through every plane and a component in the last block"""
    from protosam_amd import ops
    shape = (5, 460, 461)
    assert np.prod(shape) > 4096 * 256 + 256
    v = vr.random_volume(shape, 0.002, 77)
    v[:, 229, 230] = 1
    v[2, 100, 3:400] = 1
    v[-1, -1, -3:] = 1
    want = vr.reference(v, 18, 2, False)
    assert want["info"][0, 0] > 1500
    out, info, labels = ops.volume_regions(torch.from_numpy(v).to(dev), 18, 2, False, labels=True)
    _same((out.cpu().numpy()[None], info.cpu().numpy(), labels.cpu().numpy()[None]), want)


def test_a_volume_does_not_see_its_neighbours(dev):
    """volume 1 ends and starts with set voxels; its result is the same between empty, full and random neighbours"""
    mid = vr.random_volume((3, 5, 65), 0.5, 5)
    mid[0, 0, 0] = mid[-1, -1, -1] = 1
    want = vr.reference(mid[None], 26, 2, False)
    for fill in ("empty", "full", "random"):
        side = {"empty": np.zeros_like(mid), "full": np.ones_like(mid), "random": vr.random_volume(mid.shape, 0.5, 6)}[fill]
        got = _cabi(dev, np.stack([side, mid, side]), 26, 2, False, chunk=3)
        _same(tuple(g[1:2] for g in got), want)


def test_refused_arguments_leave_the_outputs_alone(dev):
    from protosam_amd import _lib, ops
    vols = vr.random_volume((2, 3, 5, 65), 0.4, 1)
    src = torch.from_numpy(vols).to(dev)
    out = torch.full(vols.shape, POISON8, dtype=torch.uint8, device=dev)
    lab = torch.full(vols.shape, POISON32, dtype=torch.int32, device=dev)
    for exc, args, kw in ((ValueError, (src,), dict(connectivity=8)), (ValueError, (src,), dict(min_voxels=-1)),
                          (ValueError, (src,), dict(keep_largest=2)), (RuntimeError, (src.cpu(),), {}),
                          (TypeError, (src.to(torch.int32),), {}), (ValueError, (src,), dict(chunk=0)),
                          (ValueError, (src,), dict(scratch=torch.zeros(8, dtype=torch.int64, device=dev)))):
        with pytest.raises(exc):
            ops.volume_regions(*args, out=out, labels=lab, **kw)
    for bad_out in (out.cpu(), out[:1], out.to(torch.int32)):
        with pytest.raises((RuntimeError, TypeError, ValueError)):
            ops.volume_regions(src, out=bad_out)
    # the C entry itself: non-zero and nothing launched
    R, D, H, W = vols.shape
    n = D * H * W
    need = ops.volume_regions_workspace(D, H, W, R, labels=True)
    scratch = torch.zeros((need + 7) // 8, dtype=torch.int64, device=dev)
    info = torch.full((R, 12), POISON64, dtype=torch.int64, device=dev)
    good = dict(R=R, D=D, H=H, W=W, sr=n, sz=H * W, conn=26, mv=0, kl=1, chunk=R, out=out.data_ptr(), info=info.data_ptr(),
                scratch=scratch.data_ptr(), nbytes=need)
    for change in (dict(conn=8), dict(conn=0), dict(mv=-1), dict(kl=2), dict(kl=-1), dict(chunk=0), dict(R=-1), dict(D=0), dict(W=0),
                   dict(sz=H * W - 1), dict(sr=H * W - 1), dict(out=0), dict(info=0), dict(scratch=0), dict(nbytes=need - 1),
                   dict(scratch=scratch.data_ptr() + 4), dict(D=1 << 11, H=1 << 10, W=1 << 10)):
        a = dict(good, **change)
        st = _lib.lib().psam_volume_regions(src.data_ptr(), a["R"], a["D"], a["H"], a["W"], a["sr"], a["sz"], a["conn"], a["mv"],
                                            a["kl"], a["chunk"], a["out"], a["info"], lab.data_ptr(), a["scratch"], a["nbytes"],
                                            torch.cuda.current_stream().cuda_stream)
        assert st != 0, change
    torch.cuda.synchronize()
    assert bool((out == POISON8).all()) and bool((lab == POISON32).all()) and bool((info == POISON64).all())
    assert not bool(scratch.any())


# ---- pipeline: a kept scan with a stray island ------------------------------------------------------------------------------------
def _ellipsoid(shape, centre, radii):
    z, y, x = np.indices(shape)
    return sum(((a - c) / r) ** 2 for a, c, r in zip((z, y, x), centre, radii)) <= 1.0


def test_clean_scan_and_scores(dev):
    from protosam_amd import metrics, ops, runner
    Z, C, S = 6, 2, 64
    classes = [1, 2]
    label = np.zeros((Z, S, S), dtype=np.uint8)
    label[_ellipsoid(label.shape, (2.5, 20, 22), (3.4, 11, 9))] = 1
    label[_ellipsoid(label.shape, (2.5, 44, 40), (3.4, 8, 12))] = 2
    clean = np.zeros((Z, C, S, S), dtype=np.uint8)                             # the island-free construction: the organs, moved
    clean[:, 0] = _ellipsoid(label.shape, (2.5, 21, 23), (3.4, 11, 9))
    clean[:, 1] = _ellipsoid(label.shape, (2.5, 43, 41), (3.4, 8, 12))
    kept = clean.copy()
    kept[0, 0, 60:62, 2:5] = 1                                                 # 6 voxels far from organ 1, on another slice's corner
    kept[5, 1, 1:3, 58:60] = 1                                                 # 4 voxels far from organ 2
    kept[5, 1, 3, 60] = 1                                                      # and a fifth, joined by a corner in the plane
    want = vr.reference(kept.transpose(1, 0, 2, 3), 26, 0, True)
    assert np.array_equal(want["out"].transpose(1, 0, 2, 3), clean) and want["info"][:, 0].tolist() == [2, 2]
    keep_d, lab_d = torch.from_numpy(kept).to(dev), torch.from_numpy(label).to(dev)
    cleaned, info = runner.clean_scan(keep_d, classes)
    assert cleaned.data_ptr() != keep_d.data_ptr() and torch.equal(keep_d.cpu(), torch.from_numpy(kept))
    assert np.array_equal(cleaned.cpu().numpy(), clean) and np.array_equal(info.cpu().numpy(), want["info"])
    table = ops.volume_regions_table(info)
    assert [t["voxels_dropped"] for t in table] == [6, 5] and [t["kept"] for t in table] == [1, 1]
    # min_voxels instead of the largest, one class [Z, S, S], in place
    one = keep_d[:, 1].contiguous()
    got, info1 = runner.clean_scan(one, None, connectivity=6, min_voxels=5, keep_largest=False, out=one)
    assert got.data_ptr() == one.data_ptr() and np.array_equal(one.cpu().numpy(), clean[:, 1])
    assert np.array_equal(info1.cpu().numpy(), vr.reference(kept[:, 1], 6, 5, False)["info"])
    with pytest.raises(ValueError):
        runner.clean_scan(keep_d, [1, 2, 3])
    with pytest.raises(ValueError):
        runner.clean_scan(keep_d, None)
    # scan-level counts: one seg_counts call, summed by hand
    scan = runner.score_scan(cleaned, lab_d, classes).cpu().numpy()
    per = ops.seg_counts(cleaned, lab_d, metrics.class_rows(Z, classes, label_planes=list(range(Z))).tolist()).cpu().numpy()
    per = per.reshape(Z, C, 12)
    assert scan.shape == (C, 12) and np.array_equal(scan[:, :4], per[:, :, :4].sum(axis=0))
    for cols, fn in (((4, 5, 8, 9), np.min), ((6, 7, 10, 11), np.max)):
        assert np.array_equal(scan[:, cols], fn(per[:, :, cols], axis=0))
    for c, cls in enumerate(classes):
        tp, fp, fn_ = (clean[:, c] & (label == cls)).sum(), (clean[:, c] & (label != cls)).sum(), ((clean[:, c] == 0) & (label == cls)).sum()
        assert scan[c, :4].tolist() == [tp, fp, fn_, Z * S * S - tp - fp - fn_]
    shifted = runner.score_scan(cleaned[1:4], lab_d, classes, zs=[1, 2, 3]).cpu().numpy()
    assert np.array_equal(shifted[:, :4], per[1:4, :, :4].sum(axis=0))
    # the boundary measures: the cleaned scan's HD is the island-free construction's, and below the uncleaned scan's
    spacing = (1.0, 1.0, 1.0)
    hd_clean = runner.score_scan_surfaces(cleaned, lab_d, classes, spacing)[:, metrics.HD]
    hd_free = runner.score_scan_surfaces(torch.from_numpy(clean).to(dev), lab_d, classes, spacing)[:, metrics.HD]
    hd_kept = runner.score_scan_surfaces(keep_d, lab_d, classes, spacing)[:, metrics.HD]
    assert np.array_equal(hd_clean, hd_free) and (hd_clean < hd_kept).all() and np.isfinite(hd_kept).all()
