"""GPU: psam_topk_points / psam_topk_points_batch (csrc/topk_points.hip) against tests/topk_reference.py, bit for bit.

Labels and tables come from ops.ccl / ops.ccl_batch on oracle.ccl.make_pattern masks; the reference labels come from
oracle.ccl.label (the same numbering). Before every call `keys` holds a garbage pattern, and `keys` and the scratch lie between
guard words: afterwards every key equals the reference (uint64 equality) and every guard word is intact.
"""
import numpy as np
import pytest
import torch

import topk_reference as tr
from oracle import ccl as occl

pytestmark = pytest.mark.gpu

GUARD, GARBAGE, NG = 0x5AFEC0DE5AFEC0DE, 0x7BADBADBADBADBAD, 64
SHAPES = [(1, 1), (1, 300), (300, 1), (63, 65), (64, 64), (65, 257), (257, 255), (300, 517), (1031, 97)]
CAP = 256


class Guarded:
    """an int64 device buffer of `numel` words between two runs of NG guard words"""

    def __init__(self, numel, dev, fill=None):
        self.buf = torch.full((numel + 2 * NG,), GUARD, dtype=torch.int64, device=dev)
        self.view = self.buf[NG:NG + numel]
        if fill is not None:
            self.view.fill_(fill)

    def intact(self):
        return bool((self.buf[:NG] == GUARD).all()) and bool((self.buf[-NG:] == GUARD).all())


def _call(ws, pfg, tab, k, max_comp, only_best=False, labels=None, P=None, tabs=None):
    """one guarded call of ops.topk_points (P None) or ops.topk_points_batch -> uint64 numpy keys"""
    from protosam_amd import ops
    dev = pfg.device
    R = 1 if only_best else max_comp
    planes = 1 if P is None else P
    keys = Guarded(planes * R * k, dev, GARBAGE)
    scratch = Guarded((ops.topk_points_workspace(planes, max_comp, only_best) + 7) // 8, dev, GARBAGE)
    if P is None:
        out = ops.topk_points(ws, pfg, tab, k, max_comp, only_best, keys=keys.view.view(R, k), labels=labels, scratch=scratch.view)
    else:
        out = ops.topk_points_batch(labels, pfg, tabs, k, max_comp, only_best, keys=keys.view.view(P, R, k), scratch=scratch.view)
    torch.cuda.synchronize()
    assert keys.intact() and scratch.intact(), "a guard word next to keys or scratch was overwritten"
    return tr.as_u64(out)


def _plane(dev, pattern, H, W, seed=0, pfg=None, cap=CAP):
    """-> (workspace after ops.ccl, device p_fg, host table, n kept, oracle labels, host p_fg)"""
    from protosam_amd import ops
    pred, p, _ = occl.make_pattern(pattern, H, W, seed=seed)
    p = p if pfg is None else pfg
    ws = ops.CclWorkspace(H, W, cap, dev)
    d_p = torch.from_numpy(p).to(dev)
    ops.ccl(torch.from_numpy(pred).to(dev), d_p, ws)
    tab = ws.tabs[0].cpu().numpy()
    n_found, lab = occl.label(pred)
    assert int(tab[0]) == n_found and int(tab[1]) == min(n_found, cap)
    d_lab = ws.labels.view(H, W).cpu().numpy()
    if n_found > cap:
        # which components an overflowing table keeps is up to the labelling (the others carry label 0): the kernel's own labels,
        # checked to be a renumbering of `cap` whole components
        kept = d_lab != 0
        assert np.unique(d_lab[kept]).size == cap and np.unique(lab[kept]).size == cap and not (d_lab[lab == 0]).any()
        assert all(np.unique(lab[d_lab == c + 1]).size == 1 for c in range(0, cap, 37))
        lab = d_lab
    else:
        assert np.array_equal(d_lab, lab)
    return ws, d_p, tab, int(tab[1]), lab, p


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("pattern", occl.PATTERNS)
def test_patterns_and_shapes(dev, pattern, H, W):
    from protosam_amd import ops
    ws, d_p, tab, n, lab, p = _plane(dev, pattern, H, W, seed=H + W)
    R = max(min(n, 64), 1)
    for k in (1, 3, 64, 251):
        got = _call(ws, d_p, ws.tabs[0], k, R)
        tr.assert_keys(got, tr.topk_keys(lab, p, n, k, R), W)
        if k == 1:                                          # the table's most confident pixel of every component
            rows = tab[ops.CC_HDR:ops.CC_HDR + ops.CC_STRIDE * n].reshape(n, ops.CC_STRIDE)
            for c in range(min(n, R)):
                x, y, v = tr.decode(got[c, 0], W)
                assert (x, y, v) == (rows[c, 8], rows[c, 9], rows[c, 10]), (c, (x, y, v), rows[c, 8:11])
    if n > 64:                                              # every component the table holds, and only the best one
        tr.assert_keys(_call(ws, d_p, ws.tabs[0], 3, n), tr.topk_keys(lab, p, n, 3, n), W)
    if n:
        best = int(tab[3])
        tr.assert_keys(_call(ws, d_p, ws.tabs[0], 5, R, only_best=True), tr.topk_keys(lab, p, n, 5, R, only_best=best), W)


@pytest.mark.parametrize("pattern", ["full", "bars", "blobs"])
def test_saturated(dev, pattern):
    """p_fg = 1.0 everywhere: a component's keys are its first pixels in raster order"""
    H, W, k = 257, 255, 251
    ws, d_p, tab, n, lab, p = _plane(dev, pattern, H, W, pfg=np.ones((H, W), np.float32))
    got = _call(ws, d_p, ws.tabs[0], k, max(n, 1))
    tr.assert_keys(got, tr.topk_keys(lab, p, n, k, max(n, 1)), W)
    for c in range(n):
        first = np.flatnonzero(lab.ravel() == c + 1)[:k]
        idx = tr.U32 - (got[c, :len(first)] & np.uint64(tr.U32)).astype(np.int64)
        assert np.array_equal(idx, first) and not got[c, len(first):].any()
    if pattern == "full":
        assert n == 1 and np.array_equal(tr.U32 - (got[0] & np.uint64(tr.U32)).astype(np.int64), np.arange(k))


@pytest.mark.parametrize("pattern,H,W", [("blobs", 300, 517), ("noise41", 65, 257), ("bars", 257, 255), ("full", 63, 65)])
def test_tie_free_equals_torch_topk(dev, pattern, H, W):
    """distinct probabilities: equal, in order, to the reference's own lines (models/ProtoSAM.py:281-283) run on the CPU"""
    nn = H * W
    p = ((np.random.RandomState(7).permutation(nn).astype(np.float64) + 1.0) / (nn + 1.0)).astype(np.float32).reshape(H, W)
    ws, d_p, tab, n, lab, _ = _plane(dev, pattern, H, W, pfg=p)
    k = 9
    got = _call(ws, d_p, ws.tabs[0], k, max(n, 1))
    t_p, t_lab = torch.from_numpy(p), torch.from_numpy(lab)
    checked = 0
    for c in range(n):
        mask = t_lab == c + 1
        if int(mask.sum()) < k:
            continue
        confidences, indices = torch.topk(t_p[mask], k)
        locations = torch.nonzero(mask)[indices]
        assert [tr.decode(v, W) for v in got[c]] == [(int(x), int(y), float(v)) for (y, x), v in zip(locations.tolist(), confidences)]
        checked += 1
    assert checked
    tr.assert_keys(got, tr.topk_keys(lab, p, n, k, max(n, 1)), W)


@pytest.fixture(scope="module")
def batch_planes(dev):
    """3 planes of 1024^2 blobs, p_fg as channel 1 of a [3,2,H,W] map, labelled by ops.ccl_batch; the reference keys' inputs"""
    from protosam_amd import ops
    S, P = 1024, 3
    made = [occl.make_pattern("blobs", S, S, seed=s) for s in (11, 12, 13)]
    pred = torch.from_numpy(np.stack([m[0] for m in made])).to(dev)
    prob = torch.from_numpy(np.stack([np.stack([m[2], m[1]]) for m in made])).to(dev)
    cw = ops.CclWorkspace(S, S, CAP, dev, slots=P)
    ops.ccl_batch(pred, prob, cw)
    tabs = cw.tabs.cpu().numpy()
    labs = [occl.label(m[0])[1] for m in made]
    return cw, prob, tabs, labs, [m[1] for m in made]


@pytest.mark.parametrize("only_best", [False, True])
def test_batch(dev, batch_planes, only_best):
    cw, prob, tabs, labs, pfgs = batch_planes
    S, P, k, R = 1024, 3, 12, 64
    got = _call(None, prob[:, 1], None, k, R, only_best, labels=cw.labels_b[:P], P=P, tabs=cw.tabs[:P])
    again = _call(None, prob[:, 1], None, k, R, only_best, labels=cw.labels_b[:P], P=P, tabs=cw.tabs[:P])
    assert np.array_equal(got, again)
    for p in range(P):
        n = int(tabs[p][1])
        assert n >= 2
        best = int(tabs[p][3]) if only_best else None
        tr.assert_keys(got[p], tr.topk_keys(labs[p], pfgs[p], n, k, R, only_best=best), S)
        one = _call(cw, prob[p, 1].contiguous(), cw.tabs[p], k, R, only_best, labels=cw.labels_b[p])
        assert np.array_equal(got[p], one), p


def test_more_components_than_rows(dev):
    H, W = 65, 257
    ws, d_p, tab, n, lab, p = _plane(dev, "noise20", H, W)
    assert n > 5
    got = _call(ws, d_p, ws.tabs[0], 4, 5)
    tr.assert_keys(got, tr.topk_keys(lab, p, n, 4, 5), W)
    assert got[:, 0].all()
    few = _plane(dev, "twins", H, W)                       # fewer components than rows: the other rows are zeros
    got = _call(few[0], few[1], few[0].tabs[0], 4, 7)
    tr.assert_keys(got, tr.topk_keys(few[4], few[5], few[3], 4, 7), W)
    assert few[3] == 2 and not got[2:].any()


def test_more_components_than_table(dev):
    """lattice on 257 x 255 has 16512 one-pixel components, the table 256 rows: pixels of the others carry label 0"""
    H, W = 257, 255
    ws, d_p, tab, n, lab, p = _plane(dev, "lattice", H, W)
    assert int(tab[0]) > n == CAP
    got = _call(ws, d_p, ws.tabs[0], 3, CAP)
    tr.assert_keys(got, tr.topk_keys(lab, p, n, 3, CAP), W)
    d_lab = ws.labels.cpu().numpy()
    idx = tr.U32 - (got[got != 0] & np.uint64(tr.U32)).astype(np.int64)
    assert idx.size == CAP and (d_lab[idx] != 0).all()
    assert got[:, 0].all() and not got[:, 1:].any()         # components of one pixel: one slot, then zeros


def test_components_smaller_than_k(dev):
    H, W, k = 63, 65, 40
    ws, d_p, tab, n, lab, p = _plane(dev, "noise20", H, W)
    got = _call(ws, d_p, ws.tabs[0], k, n)
    tr.assert_keys(got, tr.topk_keys(lab, p, n, k, n), W)
    area = np.bincount(lab.ravel(), minlength=n + 1)[1:n + 1]
    assert (area < k).any() and (area > 1).any()
    for c in range(n):
        a = min(int(area[c]), k)
        assert got[c, :a].all() and not got[c, a:].any()


def test_refused_arguments(dev):
    """status 1 through _lib.check, nothing launched: keys keep their garbage"""
    from protosam_amd import _lib, ops
    H, W = 65, 257
    ws, d_p, tab, n, lab, p = _plane(dev, "blobs", H, W)
    keys = Guarded(CAP * 252, dev, GARBAGE)
    scratch = Guarded((ops.topk_points_workspace(1, CAP) + 7) // 8, dev, GARBAGE)
    L = _lib.lib()

    def raw(labels=None, pfg=None, tabp=None, cap=CAP, H=H, W=W, k=3, max_comp=4, keysp=None, scr=None, nbytes=None, P=1):
        a = [ws.labels.data_ptr() if labels is None else labels, d_p.data_ptr() if pfg is None else pfg, H * W,
             ws.tabs.data_ptr() if tabp is None else tabp, cap, P, H, W, k, max_comp, 0,
             keys.view.data_ptr() if keysp is None else keysp, scratch.view.data_ptr() if scr is None else scr,
             scratch.view.numel() * 8 if nbytes is None else nbytes, ops._stream()]
        return L.psam_topk_points_batch(*a)

    assert raw() == 0                                                           # (the arguments the cases below vary are good)
    keys.view.fill_(GARBAGE)
    bad = [dict(k=0), dict(k=-1), dict(k=252), dict(max_comp=0), dict(max_comp=CAP + 1), dict(P=0), dict(P=-1), dict(H=0), dict(W=0),
           dict(H=-3), dict(H=65536, W=32768), dict(labels=0), dict(pfg=0), dict(tabp=0), dict(keysp=0), dict(scr=0),
           dict(nbytes=ops.topk_points_workspace(1, 4) - 1), dict(nbytes=0)]
    for kw in bad:
        st = raw(**kw)
        assert st == 1, kw
        with pytest.raises(RuntimeError, match="psam_topk_points_batch failed with status 1"):
            _lib.check(st, "psam_topk_points_batch")
    one = L.psam_topk_points(ws.labels.data_ptr(), d_p.data_ptr(), ws.tabs.data_ptr(), CAP, H, W, 252, 4, 0, keys.view.data_ptr(),
                             scratch.view.data_ptr(), scratch.view.numel() * 8, ops._stream())
    assert one == 1
    # and through the wrappers
    for kw in (dict(k=0), dict(k=252), dict(max_comp=0), dict(max_comp=CAP + 1)):
        a = dict(k=3, max_comp=4)
        a.update(kw)
        with pytest.raises(RuntimeError, match="failed with status 1"):
            ops.topk_points(ws, d_p, ws.tabs[0], a["k"], a["max_comp"], keys=keys.view, scratch=scratch.view)
        with pytest.raises(RuntimeError, match="failed with status 1"):
            ops.topk_points_batch(ws.labels.view(1, -1), d_p.view(1, H, W), ws.tabs[:1], a["k"], a["max_comp"], keys=keys.view,
                                  scratch=scratch.view)
    with pytest.raises(RuntimeError, match="failed with status 1"):             # scratch of a smaller call
        ops.topk_points(ws, d_p, ws.tabs[0], 3, CAP, keys=keys.view, scratch=scratch.view[:16])
    torch.cuda.synchronize()
    assert bool((keys.view == GARBAGE).all()) and keys.intact() and scratch.intact()
