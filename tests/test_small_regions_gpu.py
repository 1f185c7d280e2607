"""GPU: psam_small_regions (csrc/small_regions.hip), ops.small_regions and ops.small_regions_select against the numpy contract of
tests/small_regions_reference.py (pinned to the reference's remove_small_regions by tests/test_small_regions_cpu.py). Every
comparison is exact. The kernel cases call the C entry with every output and the scratch inside guarded buffers filled with
garbage: the guard bytes must be intact afterwards."""
import functools

import numpy as np
import pytest
import torch

import small_regions_reference as sr

pytestmark = pytest.mark.gpu

GUARD = 256          # bytes in front of and behind every payload (keeps the payload 16-byte aligned)
FILL = 0xA5


class _Guarded:
    """a payload of `nbytes` inside a uint8 device buffer of FILL, with GUARD bytes on either side"""

    def __init__(self, nbytes, dev):
        self.n = nbytes
        self.buf = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)

    def ptr(self):
        return self.buf.data_ptr() + GUARD

    def payload(self, dtype, shape):
        return self.buf[GUARD:GUARD + self.n].view(dtype).view(shape).cpu().numpy()

    def intact(self):
        return bool((self.buf[:GUARD] == FILL).all()) and bool((self.buf[GUARD + self.n:] == FILL).all())


def _call(masks, t, chunk, dev):
    """psam_small_regions on numpy masks [m,H,W] through the C entry, guarded -> (out, boxes, scores, info) as numpy"""
    from protosam_amd import _lib, ops
    m, H, W = masks.shape
    md = torch.from_numpy(np.ascontiguousarray(masks)).to(dev)
    need = ops.small_regions_workspace(H, W, chunk)
    g = dict(out=_Guarded(m * H * W, dev), boxes=_Guarded(m * 16, dev), scores=_Guarded(m * 4, dev), info=_Guarded(m * 16, dev),
             scratch=_Guarded(need, dev))
    st = _lib.lib().psam_small_regions(md.data_ptr(), m, H, W, float(t), chunk, g["out"].ptr(), g["boxes"].ptr(), g["scores"].ptr(),
                                       g["info"].ptr(), g["scratch"].ptr(), need, ops._stream())
    assert st == 0, st
    torch.cuda.synchronize()
    for k, v in g.items():
        assert v.intact(), f"guard bytes around {k} written ({m} x {H} x {W}, chunk {chunk})"
    assert torch.equal(md.cpu(), torch.from_numpy(masks)), "the input was written"
    return (g["out"].payload(torch.uint8, (m, H, W)), g["boxes"].payload(torch.int32, (m, 4)), g["scores"].payload(torch.float32, (m,)),
            g["info"].payload(torch.int32, (m, 4)))


@functools.lru_cache(maxsize=None)
def _want(shape, t):
    names, masks = sr.pattern_batch(*shape)
    return names, masks, sr.batch(masks, t)


def _compare(got, want, names, what):
    for k, field in enumerate(("out", "boxes", "scores", "info")):
        if not np.array_equal(got[k], want[k]):
            bad = [names[i] for i in range(len(names)) if not np.array_equal(got[k][i], want[k][i])]
            raise AssertionError(f"{what}: {field} differs for {bad}; first: got {got[k][names.index(bad[0])].tolist() if k else '(mask)'} "
                                 f"want {want[k][names.index(bad[0])].tolist() if k else '(mask)'}")
    assert got[2].dtype == np.float32 and got[0].dtype == np.uint8


@pytest.mark.parametrize("t", sr.THRESHOLDS)
@pytest.mark.parametrize("shape", sr.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_patterns_equal_the_contract(dev, shape, t):
    """Every pattern of the shape in one batch, at one threshold: masks, boxes, scores and info are exactly the contract's."""
    names, masks, want = _want(shape, t)
    got = _call(masks, t, len(names), dev)
    _compare(got, want, names, f"{shape} t={t}")
    if shape == (48, 44) and t == 6:                 # the cases the contract's mistakes show on are really in the batch
        i = names.index("tie")
        assert want[3][i].tolist()[:3] == [0, 1, 4] and want[2][i] == 0.0
        assert want[1][names.index("empty")].tolist() == [0, 0, 0, 0]
        assert want[3][names.index("ring5")][0] == 1 and want[3][names.index("ring6")][0] == 0


@functools.lru_cache(maxsize=None)
def _batch_case(m):
    """m masks of 33 x 17 - the patterns, then random fills (m = 3: a random fill, the tie, the border holes) - and the contract's
    result at t = 6, computed once per m"""
    H, W = 33, 17
    names, masks = sr.pattern_batch(H, W)
    if m == 3:
        allm = np.stack([masks[names.index("random0.3")], masks[names.index("tie")], masks[names.index("border_holes")]])
    else:
        g = np.random.RandomState(m)
        extra = [((g.rand(H, W) < g.choice([0.05, 0.3, 0.55, 0.8])) * g.choice([1, 255])).astype(np.uint8)
                 for _ in range(max(0, m - len(names)))]
        allm = np.concatenate([masks] + ([np.stack(extra)] if extra else []))[:m]
    allm = np.ascontiguousarray(allm)
    assert len(allm) == m
    return allm, sr.batch(allm, 6)


@pytest.mark.parametrize("chunk", [1, 4, 64])
@pytest.mark.parametrize("m", [1, 3, 67])
def test_batches_and_chunks(dev, m, chunk):
    """m masks with 1, 4 and 64 masks in flight: chunk boundaries, a ragged last chunk and a chunk larger than the batch give the
    result of the contract, mask for mask."""
    allm, want = _batch_case(m)
    got = _call(allm, 6, chunk, dev)
    _compare(got, want, [str(i) for i in range(m)], f"m={m} chunk={chunk}")


def test_wrapper_equals_the_entry(dev):
    """ops.small_regions: default chunk, a given `out` and `scratch`, a float threshold; m = 0 returns empty tensors."""
    from protosam_amd import ops
    names, masks, want = _want((48, 44), 5.5)
    md = torch.from_numpy(masks).to(dev)
    out, boxes, scores, info = ops.small_regions(md, 5.5)
    _compare((out.cpu().numpy(), boxes.cpu().numpy(), scores.cpu().numpy(), info.cpu().numpy()), want, names, "wrapper")
    mine = torch.full(masks.shape, FILL, dtype=torch.uint8, device=dev)
    scratch = torch.empty((ops.small_regions_workspace(48, 44, 5) + 7) // 8, dtype=torch.int64, device=dev)
    out2, boxes2, scores2, info2 = ops.small_regions(md, 5.5, out=mine, chunk=5, scratch=scratch)
    assert out2 is mine
    _compare((out2.cpu().numpy(), boxes2.cpu().numpy(), scores2.cpu().numpy(), info2.cpu().numpy()), want, names, "wrapper, chunk 5")
    e = ops.small_regions(torch.empty((0, 48, 44), dtype=torch.uint8, device=dev), 6)
    assert [tuple(x.shape) for x in e] == [(0, 48, 44), (0, 4), (0,), (0, 4)]


def _select(masks, t, thr, dev):
    from protosam_amd import ops
    out, table = ops.small_regions_select(torch.from_numpy(np.ascontiguousarray(masks)).to(dev), t, thr)
    assert table.dtype == torch.int32 and table.numel() == 1 + 9 * len(masks)
    kept, info, boxes = ops.small_regions_table(table.cpu().numpy(), len(masks))
    return out.cpu().numpy(), kept, info, boxes


def test_select_equals_the_contract(dev):
    """small_regions_select: kept order and count, info and boxes from ONE int32 tensor - on the patterns (changed and unchanged
    masks mixed), on a batch where every score is 0, and on one where boxes coincide; with and without suppression."""
    names, masks = sr.pattern_batch(48, 44)
    P = dict(zip(names, masks))
    all_changed = np.stack([P["ring5"], P["border_holes"], P["tie"], P["random0.3"], P["ring5"], P["small_background"]])
    coincide = np.stack([P["ring50"], P["ring50"], P["ring5"], P["ring5"], P["full"], P["full"], P["empty"], P["empty"], P["ring6"]])
    for what, batch_, t in (("patterns", masks, 6), ("patterns", masks, 50), ("all changed", all_changed, 6), ("coincide", coincide, 6)):
        for thr in (0.7, 1.0, 0.0):
            want_out, want_kept, want_info, want_boxes = sr.select(batch_, t, thr)
            out, kept, info, boxes = _select(batch_, t, thr, dev)
            assert kept.tolist() == want_kept.tolist(), f"{what} t={t} nms={thr}: kept {kept.tolist()} want {want_kept.tolist()}"
            assert np.array_equal(info, want_info) and np.array_equal(boxes, want_boxes) and np.array_equal(out, want_out), what
        if what == "all changed":
            assert want_info[:, :2].sum(1).min() > 0
        if what == "coincide":
            k = sr.select(batch_, t, 0.7)[1].tolist()
            assert 1 not in k and 3 not in k and 5 not in k and 6 in k and 7 in k
    from protosam_amd import ops
    out, table = ops.small_regions_select(torch.empty((0, 8, 8), dtype=torch.uint8, device=dev), 6, 0.7)
    assert table.cpu().tolist() == [0] and tuple(out.shape) == (0, 8, 8)


def test_refused_arguments(dev):
    """Each refusal raises (the wrapper on the host, the entry with status 1, outputs untouched), and a call after them all gives
    the contract's result."""
    from protosam_amd import _lib, ops
    names, masks, want = _want((33, 17), 6)
    md = torch.from_numpy(masks).to(dev)
    m, H, W = masks.shape
    nan = float("nan")
    with pytest.raises(ValueError):
        ops.small_regions(md, nan)
    with pytest.raises(ValueError):
        ops.small_regions(md, 6, chunk=0)
    with pytest.raises(ValueError):
        ops.small_regions(md[:, :, :5], 6)                                   # not contiguous
    with pytest.raises(ValueError):
        ops.small_regions(md[0], 6)
    with pytest.raises(TypeError):
        ops.small_regions(md.int(), 6)
    with pytest.raises(ValueError):
        ops.small_regions(md, 6, out=torch.empty((m, H, W + 1), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        ops.small_regions(md, 6, chunk=4, scratch=torch.empty(8, dtype=torch.int64, device=dev))
    with pytest.raises(TypeError):
        ops.small_regions(md, 6, scratch=torch.empty(1 << 16, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.small_regions_select(torch.zeros((ops.NMS_MAX_GROUP + 1, 1, 1), dtype=torch.uint8, device=dev), 6, 0.7)
    need = ops.small_regions_workspace(H, W, 4)
    o = torch.full((m, H, W), FILL, dtype=torch.uint8, device=dev)
    b = torch.full((m, 4), -7, dtype=torch.int32, device=dev)
    s = torch.full((m,), -7.0, dtype=torch.float32, device=dev)
    i = torch.full((m, 4), -7, dtype=torch.int32, device=dev)
    x = torch.full(((need + 7) // 8,), -7, dtype=torch.int64, device=dev)
    P = dict(masks=md.data_ptr(), m=m, H=H, W=W, t=6.0, chunk=4, out=o.data_ptr(), boxes=b.data_ptr(), scores=s.data_ptr(),
             info=i.data_ptr(), scratch=x.data_ptr(), bytes=need)
    cases = [dict(m=-1), dict(H=0), dict(W=0), dict(H=-3), dict(H=65536, W=32768), dict(chunk=0), dict(bytes=need - 1), dict(t=nan),
             dict(masks=None), dict(out=None), dict(boxes=None), dict(scores=None), dict(info=None), dict(scratch=None),
             dict(scratch=x.data_ptr() + 4)]
    for c in cases:
        a = dict(P, **c)
        st = _lib.lib().psam_small_regions(a["masks"], a["m"], a["H"], a["W"], a["t"], a["chunk"], a["out"], a["boxes"], a["scores"],
                                           a["info"], a["scratch"], a["bytes"], ops._stream())
        assert st == 1, (c, st)
    assert _lib.lib().psam_small_regions(None, 0, H, W, 6.0, 1, None, None, None, None, None, 0, ops._stream()) == 0   # m == 0: a no-op
    torch.cuda.synchronize()
    assert bool((o == FILL).all()) and bool((b == -7).all()) and bool((s == -7).all()) and bool((i == -7).all()) and bool((x == -7).all())
    got = ops.small_regions(md, 6)
    _compare(tuple(v.cpu().numpy() for v in got), want, names, "after the refusals")
    print(f"{len(cases)} refusals of the entry, 9 of the wrappers")


def test_crop_select_equals_host_filters(dev):
    """psam_amg_select_crop on a synthetic statistics table: boxes at distances 19, 20 and 21 from every crop and image edge, empty
    masks, score filters on - the records are those of the host's filters, edge rule and nms_xyxy, in order."""
    from protosam_amd import ops
    from protosam_amd.segment_anything.utils.amg import is_box_near_crop_edge, nms_xyxy
    crop, orig = [100, 60, 330, 250], [0, 0, 400, 300]
    cw, ch = crop[2] - crop[0], crop[3] - crop[1]
    boxes = [[0, 0, 0, 0]]
    for d in (19, 20, 21):
        for sgn in (-1, 1):
            for k in range(4):
                for target in (crop[k] - crop[k % 2], orig[k] - crop[k % 2]):
                    bx = [cw // 2 - 30 + 3 * len(boxes) % 20, ch // 2 - 30, cw // 2 + 30, ch // 2 + 30 - len(boxes) % 17]
                    bx[k] = target + sgn * d
                    boxes.append(bx)
    while len(boxes) % 3:
        boxes.append([5 + len(boxes), 40, 60, 90])
    boxes = np.array(boxes, dtype=np.int64)
    n = len(boxes)
    g = np.random.RandomState(3)
    stats = np.zeros((n, 8), np.int32)
    stats[:, 0] = g.randint(90, 101, n); stats[:, 1] = 100; stats[:, 2] = 50
    stats[:, 3:7] = boxes
    stats[0, 2] = 0; stats[0, 3:7] = [sr.INT_MAX, sr.INT_MAX, -1, -1]          # an empty mask: its box is [0, 0, 0, 0]
    iou4 = g.rand(n // 3, 4).astype(np.float32)
    for iou_t, stab_t, nms_t in ((0.0, 0.0, 1.0), (0.3, 0.93, 0.7), (0.0, 0.0, 0.5)):
        iou = iou4[:, 1:].reshape(-1)
        ok = np.ones(n, bool)
        if iou_t > 0:
            ok &= iou > iou_t
        if stab_t > 0:
            ok &= (stats[:, 0].astype(np.float32) / stats[:, 1].astype(np.float32)) >= stab_t
        ok &= ~is_box_near_crop_edge(boxes, crop, orig)
        idx = np.flatnonzero(ok)
        want = idx[nms_xyxy(boxes[idx], iou[idx], nms_t)]
        rec, cnt = ops.amg_select_crop(torch.from_numpy(stats).to(dev), torch.from_numpy(iou4).to(dev), (0, n), iou_t, stab_t, nms_t,
                                       crop, orig)
        k = int(cnt.cpu()[0])
        r = rec[0, :k].cpu().numpy()
        assert r[:, 0].tolist() == want.tolist(), (iou_t, stab_t, nms_t)
        assert np.array_equal(r[:, 5:9], boxes[want]) and 0 < k < n
        rec0, cnt0 = ops.amg_select(torch.from_numpy(stats).to(dev), torch.from_numpy(iou4).to(dev), (0, n), iou_t, stab_t, nms_t)
        assert int(cnt0.cpu()[0]) > k                                            # the edge filter dropped something
