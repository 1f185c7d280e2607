"""GPU parity of the connected-components kernels (csrc/ccl.hip: psam_ccl, psam_ccl_batch, psam_neg_points,
psam_neg_points_batch) against the exact reference oracle/ccl.py, on the masks where lock-free union-find goes wrong:
diagonal-only links, unions that meet only in the last row, runs across the 64- and 256-lane segment boundaries, shapes that are
not multiples of 64, 16 or 32, 1-pixel images, ties, percolating noise and tables at and beyond their capacity.

Every output starts as garbage (labels and parent -7, tables NaN), so an element a kernel leaves unwritten fails. Every output
is an exact integer except the fp32 confidence, whose bound follows from its arithmetic:

p_fg is a multiple of 1/8 in [0, 1] (oracle.ccl.make_pattern). ccl_stats_kernel sums one wave's p_fg in fp32 (at most 64 terms:
every partial sum is a multiple of 1/8 below 2^6, exact) and those partials in fp64 (multiples of 1/8 below 2^21, exact), so
the component's sum S is exact until ccl_finalize_kernel rounds it to fp32 (relative error <= u = 2^-24). The denominator
fl(T + 1e-6f), T = sum(pred) <= 2^21 exact in fp32, is rounded once (<= u) and differs from T + 1e-6 by |1e-6f - 1e-6| < 3e-14,
below 0.001 u relative to T >= 1; the IEEE division rounds once more (<= u). So |conf - S / (T + 1e-6)| <=
((1 + u)^2 / (1 - u) (1 + 0.001 u) - 1) conf < 3.01 u conf. The component tab[3] names holds the largest fp32 confidence,
so its float64 confidence is within 2 x 3.01 u of the float64 maximum.
"""
import types

import numpy as np
import pytest
import torch

from oracle import ccl as oc

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
CONF_BOUND = 3.01                 # x 2^-24 x conf, derived above
CAP = 4096                        # psam_ccl's largest table
HDR, STRIDE = 8, 12               # csrc/ccl.hip table layout
SHAPES = [(1, 1), (1, 300), (300, 1), (63, 65), (64, 64), (65, 257), (257, 255), (300, 517), (1031, 97)]
ADVERSARIAL = ("spiral", "comb", "checker", "noise41", "bars", "nested_uv", "diag", "antidiag")


def _ops():
    from protosam_amd import ops
    return ops


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _poison(ws):
    ws.labels_b.fill_(-7)
    ws.parent_b.fill_(-7)
    ws.tabs.fill_(float("nan"))


def _fg(preds, dev):
    return torch.tensor([int(p.sum()) for p in preds], dtype=torch.int32, device=dev)


def _run_ccl(ws, pred, pfg, dev, fg_sum, poison=True):
    """ops.ccl on one plane -> host (labels [H,W], table, parent [H,W])."""
    if poison:
        _poison(ws)
    _ops().ccl(_dev(pred, dev), _dev(pfg, dev), ws, fg_sum=_fg([pred], dev) if fg_sum else None)
    H, W = pred.shape
    return ws.labels.cpu().numpy().reshape(H, W), ws.tabs[0].cpu().numpy(), ws.parent.cpu().numpy().reshape(H, W)


def _kept_components(what, labels, lab, n, cap):
    """n > cap: every reference component carries one kernel label on all its pixels, 0 where it was not kept, and the kept ones
    carry 1..cap in the order of their first pixels. -> reference indices of the kept components (which ones is unspecified)."""
    fg = lab > 0
    assert np.all(labels[~fg] == 0), f"{what}: background pixels labelled"
    lo = np.full(n, np.iinfo(np.int64).max)
    hi = np.full(n, np.iinfo(np.int64).min)
    np.minimum.at(lo, lab[fg] - 1, labels[fg])
    np.maximum.at(hi, lab[fg] - 1, labels[fg])
    split = np.flatnonzero(lo != hi)
    assert not len(split), f"{what}: {len(split)} components carry several labels, first: reference component {split[0]}"
    ks = np.flatnonzero(lo > 0)
    assert len(ks) == cap and np.array_equal(lo[ks], np.arange(1, cap + 1)), f"{what}: kept labels are not 1..cap by first pixel"
    return ks


def _check_table(what, pred, pfg, ref, labels, tab, cap, parent=None):
    """One plane's labels / table (and union-find forest) against the reference -> worst conf error in units of 2^-24."""
    n, lab, st = ref
    kept = min(n, cap)
    assert (tab[0], tab[1]) == (n, kept), f"{what}: (n, kept) = ({tab[0]}, {tab[1]}), expected ({n}, {kept})"
    assert tab[2] == int(pred.sum()), f"{what}: sum(pred) {tab[2]}, expected {int(pred.sum())}"
    if n <= cap:
        bad = labels != lab
        assert not bad.any(), f"{what}: {int(bad.sum())} labels differ, first at (y, x) = {tuple(np.argwhere(bad)[0])}"
        ks = np.arange(n)
    else:
        ks = _kept_components(what, labels, lab, n, cap)
    rows = tab[HDR:HDR + STRIDE * kept].reshape(kept, STRIDE)
    assert np.isfinite(tab[:4]).all() and np.isfinite(rows).all(), f"{what}: unwritten table entries"
    exp = oc.table_rows(st, ks)
    for c in oc.INT_COLS:
        bad = np.flatnonzero(rows[:, c] != exp[:, c])
        assert not len(bad), (f"{what}: {oc.ROW_NAMES[c]} differs in {len(bad)} rows, first row {bad[0]}: "
                              f"{rows[bad[0], c]} != {exp[bad[0], c]}")
    assert np.all(rows[:, 11] == 0), f"{what}: pad column"
    bp = rows[:, 10].astype(np.float32)
    at = pfg[rows[:, 9].astype(np.int64), rows[:, 8].astype(np.int64)]
    assert np.array_equal(bp.astype(np.float64), rows[:, 10]) and np.array_equal(bp.view(np.uint32), at.view(np.uint32)), \
        f"{what}: best_p is not p_fg at the best point"
    c, cr = rows[:, 7], exp[:, 7]
    err = np.abs(c - cr)
    worst = float((err[cr > 0] / cr[cr > 0]).max() / U24) if (cr > 0).any() else 0.0
    assert np.all(err <= CONF_BOUND * U24 * cr), f"{what}: conf off by {worst:.2f} x 2^-24 (bound {CONF_BOUND})"
    t3 = int(tab[3])
    assert t3 == (int(np.argmax(c)) if kept else 0), f"{what}: tab[3] = {t3} is not the first most confident row"
    if kept:
        assert cr.max() - cr[t3] <= 2 * CONF_BOUND * U24 * cr.max(), f"{what}: tab[3] names a component far from the maximum"
    if parent is not None:   # the flattened forest (SamAutomaticMaskGenerator reads it): every pixel holds its root, the first
        fg = pred != 0
        assert np.all(parent[~fg] == -1) and np.array_equal(parent[fg], st["first"][lab[fg] - 1]), f"{what}: parent"
    return worst


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ccl_patterns(dev, shape):
    """Every pattern at every shape, with fg_sum given and without: labels, table and forest exact, conf within the bound."""
    H, W = shape
    ws = _ops().CclWorkspace(H, W, CAP, dev)
    worst = 0.0
    for i, name in enumerate(oc.PATTERNS):
        pred, pfg, _ = oc.make_pattern(name, H, W, seed=i)
        ref = oc.ccl_reference(pred, pfg)
        for fg_sum in (True, False):
            labels, tab, parent = _run_ccl(ws, pred, pfg, dev, fg_sum)
            worst = max(worst, _check_table(f"{name} {H}x{W} fg_sum={fg_sum}", pred, pfg, ref, labels, tab, CAP, parent))
    print(f"ccl {H}x{W}: {len(oc.PATTERNS)} patterns exact; worst conf error {worst:.3f} x 2^-24 (bound {CONF_BOUND})")


def test_ccl_1024_patterns_deterministic(dev):
    """Every pattern at 1024^2; the adversarial ones three times, with bit-identical integer outputs when the table holds every
    component (beyond the capacity, which components are kept is unspecified)."""
    ws = _ops().CclWorkspace(1024, 1024, CAP, dev)
    worst = 0.0
    for i, name in enumerate(oc.PATTERNS):
        pred, pfg, _ = oc.make_pattern(name, 1024, 1024, seed=i)
        ref = oc.ccl_reference(pred, pfg)
        first = None
        for run in range(3 if name in ADVERSARIAL else 1):
            labels, tab, parent = _run_ccl(ws, pred, pfg, dev, fg_sum=run != 1)
            worst = max(worst, _check_table(f"{name} 1024^2 run {run}", pred, pfg, ref, labels, tab, CAP, parent))
            kept = min(ref[0], CAP)
            ints = (labels, parent, tab[:4], tab[HDR:HDR + STRIDE * kept].reshape(kept, STRIDE)[:, list(oc.INT_COLS)])
            if first is None:
                first = ints
            elif ref[0] <= CAP:
                assert all(np.array_equal(a, b) for a, b in zip(first, ints)), f"{name}: run {run} differs from run 0"
    print(f"ccl 1024^2: {len(oc.PATTERNS)} patterns exact; worst conf error {worst:.3f} x 2^-24 (bound {CONF_BOUND})")


def test_ccl_adversarial_timing(dev):
    """psam_ccl time at 1024^2 (device events, no assertion): union chains on these masks can be far longer than on blobs."""
    ops = _ops()
    ws = ops.CclWorkspace(1024, 1024, CAP, dev)
    for name in ("blobs", "spiral", "comb", "checker", "noise41"):
        pred, pfg, _ = oc.make_pattern(name, 1024, 1024)
        pd, fd, fg = _dev(pred, dev), _dev(pfg, dev), _fg([pred], dev)
        ops.ccl(pd, fd, ws, fg_sum=fg)
        torch.cuda.synchronize()
        times = []
        for _ in range(10):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.ccl(pd, fd, ws, fg_sum=fg)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        print(f"ccl 1024^2 {name:8s}: {int(ws.tab[0].item()):6d} components, median {np.median(times):7.1f} us "
              f"(min {min(times):.1f}, max {max(times):.1f}, 10 calls)")


@pytest.mark.parametrize("name,shape", [("lattice", (20, 30)), ("noise20", (65, 257)), ("twins", (63, 65))])
def test_capacity_edges(dev, name, shape):
    """Tables one below, at and one above the number of components."""
    pred, pfg, _ = oc.make_pattern(name, *shape, seed=5)
    ref = oc.ccl_reference(pred, pfg)
    n = ref[0]
    assert 2 <= n < CAP
    for cap in (n - 1, n, n + 1):
        ws = _ops().CclWorkspace(*shape, cap, dev)
        for fg_sum in (True, False):
            labels, tab, parent = _run_ccl(ws, pred, pfg, dev, fg_sum)
            _check_table(f"{name} cap {cap} of {n} fg_sum={fg_sum}", pred, pfg, ref, labels, tab, cap, parent)


def test_ccl_large_fallback(dev):
    """ProtoSAM._ccl_large: more components than the fast table (MAX_COMPONENTS) are labelled again with the 4096-row table;
    more than that is a RuntimeError."""
    from protosam_amd.protosam import MAX_COMPONENTS, MAX_COMPONENTS_LARGE, ProtoSAM
    holder = types.SimpleNamespace()          # _ccl_large keeps its workspace in the caller's __dict__
    for name, H, W in (("lattice", 64, 100), ("noise41", 257, 255)):
        pred, pfg, _ = oc.make_pattern(name, H, W)
        ref = oc.ccl_reference(pred, pfg)
        assert MAX_COMPONENTS < ref[0] <= MAX_COMPONENTS_LARGE
        pd, fd, fg = _dev(pred, dev), _dev(pfg, dev), _fg([pred], dev)
        for call in range(2):                 # the second call on a poisoned workspace of the first
            ws, tab = ProtoSAM._ccl_large(holder, pd, fd, fg)
            if call == 0:
                _poison(ws)
        _check_table(f"_ccl_large {name}", pred, pfg, ref, ws.labels.cpu().numpy().reshape(H, W), tab, MAX_COMPONENTS_LARGE,
                     ws.parent.cpu().numpy().reshape(H, W))
    pred, pfg, _ = oc.make_pattern("lattice", 130, 130)
    assert oc.label(pred)[0] == 4225 > MAX_COMPONENTS_LARGE
    with pytest.raises(RuntimeError, match="exceed the table capacity"):
        ProtoSAM._ccl_large(holder, _dev(pred, dev), _dev(pfg, dev), _fg([pred], dev))


def _batch(names, H, W, dev, seed0=0):
    planes = [oc.make_pattern(nm, H, W, seed=seed0 + b) for b, nm in enumerate(names)]
    preds = [p[0] for p in planes]
    prob = np.stack([np.stack([p[2], p[1]]) for p in planes])        # [B,2,H,W]: channel 0 = p_bg, channel 1 = p_fg
    return planes, [oc.ccl_reference(p[0], p[1]) for p in planes], _dev(np.stack(preds), dev), _dev(prob, dev)


def _check_batch(what, ws, planes, refs, cap):
    H, W = planes[0][0].shape
    tabs, labels, parent = ws.tabs.cpu().numpy(), ws.labels_b.cpu().numpy(), ws.parent_b.cpu().numpy()
    for b, ((pred, pfg, _), ref) in enumerate(zip(planes, refs)):
        _check_table(f"{what} plane {b}", pred, pfg, ref, labels[b].reshape(H, W), tabs[b], cap, parent[b].reshape(H, W))


def test_ccl_batch_entries(dev):
    """psam_ccl_batch through ccl_batch (p_fg = channel 1 of [B,2,H,W]) and ccl_planes (p_fg [B,H,W]): five different planes."""
    ops = _ops()
    names = ("comb", "spiral", "bars", "twins", "nested_uv")
    H, W = 300, 517
    planes, refs, pd, probd = _batch(names, H, W, dev)
    pfgd = probd[:, 1].contiguous()
    ws = ops.CclWorkspace(H, W, 1024, dev, slots=len(names))
    fg = _fg([p[0] for p in planes], dev)
    for entry in ("ccl_batch", "ccl_planes"):
        for use_fg in (True, False):
            _poison(ws)
            if entry == "ccl_batch":
                ops.ccl_batch(pd, probd, ws, fg_sum=fg if use_fg else None)
            else:
                ops.ccl_planes(pd, pfgd, ws, fg_sum=fg if use_fg else None)
            _check_batch(f"{entry} fg_sum={use_fg}", ws, planes, refs, 1024)


def test_ccl_batch_slots_and_reuse(dev):
    """Empty planes next to full ones; then many-component planes (beyond the capacity) and few-component planes in the same
    workspace without clearing it in between, for the batched and the one-plane entry."""
    ops = _ops()
    H, W, cap = 257, 255, 512
    ws = ops.CclWorkspace(H, W, cap, dev, slots=4)
    _poison(ws)
    for i, names in enumerate((("empty", "full", "empty", "full"), ("noise41", "noise20", "lattice", "checker"),
                               ("twins", "blobs", "empty", "spiral"))):
        planes, refs, pd, probd = _batch(names, H, W, dev, seed0=10 * i)
        ops.ccl_batch(pd, probd, ws, fg_sum=_fg([p[0] for p in planes], dev))
        _check_batch(f"batch {names}", ws, planes, refs, cap)
    one = ops.CclWorkspace(H, W, cap, dev)
    for i, name in enumerate(("noise41", "twins")):
        pred, pfg, _ = oc.make_pattern(name, H, W, seed=i)
        labels, tab, parent = _run_ccl(one, pred, pfg, dev, fg_sum=False, poison=i == 0)
        _check_table(f"reused workspace {name}", pred, pfg, oc.ccl_reference(pred, pfg), labels, tab, cap, parent)


def _edge_scene(H, W, seed):
    """Components in the four corners and on the four edges (clipped rings), one across the whole width, and three close enough
    for each ring to cover the others."""
    _, pfg, pbg = oc.make_pattern("empty", H, W, seed)
    m = np.zeros((H, W), np.uint8)
    m[0:2, 0:3] = m[0:3, W - 2:] = m[H - 2:, 0:2] = m[H - 3:, W - 3:] = 1
    m[0, W // 2 - 2:W // 2 + 2] = m[H - 1, W // 3] = m[H // 2 - 1:H // 2 + 2, 0] = m[2 * H // 3, W - 1] = 1
    m[H // 3, :] = 1
    y, x = 3 * H // 4, W // 2
    m[y - 1:y + 2, x - 1:x + 2] = m[y, x + 4] = m[y + 5, x - 3] = 1
    return m, pfg, pbg


def _check_keys(what, keys, exp, W):
    bad = np.flatnonzero(keys != exp)
    assert not len(bad), (f"{what}: {len(bad)} keys differ, first [{bad[0]}]: {oc.decode_key(keys[bad[0]], W)} != "
                          f"{oc.decode_key(exp[bad[0]], W)}")


NEG_CASES = [("scene", 97, 131), ("blobs", 257, 255), ("twins", 63, 65), ("noise20", 64, 64), ("lattice", 1, 300),
             ("full", 300, 1), ("full", 1, 1), ("comb", 65, 257)]


@pytest.mark.parametrize("r", [0, 1, 3, 10])
def test_neg_points(dev, r):
    """psam_neg_points: ring and global keys exact, for thr = 0.95, thr equal to the largest p_bg (1.0) and to 0.75, and
    max_comp below, at and above n (keys beyond n are 0)."""
    ops = _ops()
    for i, (name, H, W) in enumerate(NEG_CASES):
        pred, pfg, pbg = _edge_scene(H, W, i) if name == "scene" else oc.make_pattern(name, H, W, seed=i)
        ref = oc.ccl_reference(pred, pfg)
        n, lab, st = ref
        ws = ops.CclWorkspace(H, W, 1024, dev)
        labels, tab, _ = _run_ccl(ws, pred, pfg, dev, fg_sum=True)
        _check_table(f"{name} {H}x{W}", pred, pfg, ref, labels, tab, 1024)
        pbgd = _dev(pbg, dev)
        for thr in (0.95, 1.0, 0.75):
            for max_comp in sorted({0, n // 2, n, n + 3}):
                keys = ops.neg_points(ws, pbgd, ws.tabs[0], max_comp, r=r, thr=thr).cpu().numpy().view(np.uint64)
                _check_keys(f"{name} {H}x{W} r={r} thr={thr} max_comp={max_comp}", keys,
                            oc.neg_point_keys(lab, st, pbg, r, thr, max_comp), W)


@pytest.mark.parametrize("r", [1, 10])
def test_neg_points_batch(dev, r):
    """psam_neg_points_batch on psam_ccl_batch's labels, p_bg = channel 0 of [P,2,H,W], max_comp above and below every n."""
    ops = _ops()
    H, W, cap = 97, 131, 1024
    names = ("noise20", "blobs", "twins", "empty", "bars")
    planes, refs, pd, probd = _batch(names, H, W, dev, seed0=20)
    planes[0] = _edge_scene(H, W, 20)
    refs[0] = oc.ccl_reference(planes[0][0], planes[0][1])
    pd[0] = _dev(planes[0][0], dev)
    probd[0, 0], probd[0, 1] = _dev(planes[0][2], dev), _dev(planes[0][1], dev)
    ws = ops.CclWorkspace(H, W, cap, dev, slots=len(names))
    ops.ccl_batch(pd, probd, ws, fg_sum=_fg([p[0] for p in planes], dev))
    _check_batch("neg batch", ws, planes, refs, cap)
    P = len(names)
    for max_comp in (max(ref[0] for ref in refs) + 2, 3):
        for thr in (0.95, 1.0):
            keys = ops.neg_points_batch(ws.labels_b[:P], probd[:, 0], ws.tabs[:P], max_comp, r=r, thr=thr)
            keys = keys.cpu().numpy().view(np.uint64)
            for p, ((_, _, pbg), (n, lab, st)) in enumerate(zip(planes, refs)):
                _check_keys(f"batch plane {p} r={r} thr={thr} max_comp={max_comp}", keys[p],
                            oc.neg_point_keys(lab, st, pbg, r, thr, max_comp), W)


def test_argument_rejections(dev):
    """Every entry point rejects out-of-range arguments before any launch (status 1). The buffers are real and large enough for
    the call even if a check were missing, and the tables hold 0 components."""
    from protosam_amd import _lib
    ops = _ops()
    L, P, s = _lib.lib(), ops._ptr, ops._stream()

    def rejected(st, name):
        assert st == 1, (name, st)
        with pytest.raises(RuntimeError, match="status 1"):
            _lib.check(st, name)

    H = W = 8
    pred = torch.ones((H, W), dtype=torch.uint8, device=dev)
    pfg = torch.zeros((H, W), dtype=torch.float32, device=dev)
    ws = ops.CclWorkspace(H, W, 4097, dev)

    def ccl(h=H, w=W, cap=16):
        return L.psam_ccl(P(pred), P(pfg), h, w, cap, P(ws.labels), P(ws.parent), P(ws.counters), P(ws.roots), P(ws.acc_i),
                          P(ws.acc_u), P(ws.acc_d), 0, P(ws.tabs[0]), s)

    for kw in (dict(cap=0), dict(cap=4097), dict(h=0), dict(w=0)):
        rejected(ccl(**kw), "psam_ccl")
    B = 65536
    wb = ops.CclWorkspace(1, 1, 1, dev, slots=B)
    pb = torch.ones(B, dtype=torch.uint8, device=dev)
    fb = torch.zeros(B, dtype=torch.float32, device=dev)
    for b in (0, B):
        rejected(L.psam_ccl_batch(P(pb), P(fb), 1, b, 1, 1, 1, P(wb.labels_b), P(wb.parent_b), P(wb.counters_b), P(wb.roots_b),
                                  P(wb.acc_i_b), P(wb.acc_u_b), P(wb.acc_d_b), 0, P(wb.tabs), s), "psam_ccl_batch")
    del wb
    tab = torch.zeros(HDR + STRIDE * 4, dtype=torch.float64, device=dev)
    keys = torch.zeros(16, dtype=torch.int64, device=dev)
    lab = torch.zeros((H, W), dtype=torch.int32, device=dev)
    for r, max_comp in ((-1, 2), (11, 2), (3, -1)):
        rejected(L.psam_neg_points(P(lab), P(pfg), P(tab), H, W, max_comp, r, 0.95, P(keys), s), "psam_neg_points")
    Pn, capn = 16, 4095
    tabs = torch.zeros((Pn, HDR + STRIDE * capn), dtype=torch.float64, device=dev)
    keysb = torch.zeros(Pn * (capn + 1), dtype=torch.int64, device=dev)
    labb = torch.zeros((Pn, H, W), dtype=torch.int32, device=dev)
    pbgb = torch.zeros((Pn, H, W), dtype=torch.float32, device=dev)
    for stride, cap, planes, max_comp in ((H * W, 2, 1, 3),            # max_comp > cap
                                          (H * W, capn, Pn, capn),      # P (max_comp + 1) = 65536 > 65535
                                          (-1, 4, 1, 2)):               # pbg_stride < 0
        rejected(L.psam_neg_points_batch(P(labb), P(pbgb), stride, P(tabs), cap, planes, H, W, max_comp, 10, 0.95, P(keysb), s),
                 "psam_neg_points_batch")
    # the same buffers with valid arguments run
    assert ccl() == 0
    assert L.psam_neg_points(P(lab), P(pfg), P(tab), H, W, 2, 10, 0.95, P(keys), s) == 0
    assert L.psam_neg_points_batch(P(labb), P(pbgb), H * W, P(tabs), capn, 4, H, W, 3, 10, 0.95, P(keysb), s) == 0
    torch.cuda.synchronize()
    assert int(ws.tabs[0][0].item()) == 1 and ws.labels.view(H, W).eq(1).all()
