"""GPU: psam_box_nms / psam_amg_select (csrc/nms.hip) against tests/amg_select_reference.py - the host lines the device path
replaces, run as they stand - bit for bit: kept indices, their order, the counts and every field of every record.

The pipeline tests cannot carry this: with synthetic weights every box of the generator is the whole image. The tables here are
fabricated (tests/test_amg_select_cpu.py shows which mistakes they catch). Outputs and scratch hold a garbage pattern before every
call and lie between guard words that must be intact afterwards; slots beyond the count must still hold the garbage.
"""
import functools

import numpy as np
import pytest
import torch

import amg_select_reference as ar

pytestmark = pytest.mark.gpu

GUARD, GARBAGE, NG = 0x5AFEC0DE, 0x7BADBAD1, 64
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 3072]


class Guarded:
    """a device buffer of `numel` words of `dtype` (int32 / int64) between two runs of NG guard words, filled with garbage"""

    def __init__(self, numel, dev, dtype=torch.int32, offset=0):
        self.buf = torch.full((numel + 2 * NG + offset,), GUARD, dtype=dtype, device=dev)
        self.view = self.buf[NG + offset:NG + offset + numel]
        self.view.fill_(GARBAGE)
        self.lo, self.hi = self.buf[:NG + offset], self.buf[NG + offset + numel:]

    def intact(self):
        return bool((self.lo == GUARD).all()) and bool((self.hi == GUARD).all())


def _scratch(G, maxg, dev):
    from protosam_amd import ops
    return Guarded((ops.nms_workspace(G, max(maxg, 1)) + 7) // 8, dev, torch.int64)


def _maxg(off):
    return max([b - a for a, b in zip(off[:-1], off[1:])] + [1])


def _box_nms(dev, boxes, scores, off, thr, cap=None):
    """one guarded call -> (kept [G, cap] numpy, count [G] numpy)"""
    from protosam_amd import ops
    G, cap = len(off) - 1, _maxg(off) if cap is None else cap
    kept, count, scr = Guarded(G * cap, dev), Guarded(G, dev), _scratch(G, _maxg(off), dev)
    k, c = ops.box_nms(torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), off, thr, cap=cap,
                       kept=kept.view.view(G, cap), count=count.view, scratch=scr.view)
    torch.cuda.synchronize()
    assert kept.intact() and count.intact() and scr.intact(), "a guard word next to kept, count or scratch was overwritten"
    return k.cpu().numpy(), c.cpu().numpy()


def _amg_select(dev, stats, iou4, off, thr, cap=None):
    """one guarded call -> (records [G, cap, 9] numpy, count [G] numpy)"""
    from protosam_amd import ops
    G, cap = len(off) - 1, _maxg(off) if cap is None else cap
    out, scr = Guarded(G * cap * ar.REC + G, dev), _scratch(G, _maxg(off), dev)
    r, c = ops.amg_select(torch.from_numpy(stats).to(dev), torch.from_numpy(iou4).to(dev), off, *thr, cap=cap, out=out.view,
                          scratch=scr.view)
    torch.cuda.synchronize()
    assert out.intact() and scr.intact(), "a guard word next to the records or the scratch was overwritten"
    assert r.data_ptr() == out.view.data_ptr() and c.data_ptr() == out.view.data_ptr() + 4 * G * cap * ar.REC   # one copy serves
    return r.cpu().numpy(), c.cpu().numpy()


def _check_kept(kept, count, ref, cap, what):
    for g, want in enumerate(ref):
        assert count[g] == len(want), (what, g, int(count[g]), len(want))
        k = min(len(want), cap)
        assert np.array_equal(kept[g, :k], want[:k]), (what, g)
        assert (kept[g, k:] == GARBAGE).all(), (what, g, "a slot beyond the count was written")


def _one_nan(rec):
    """the stability field of a 0 / 0 row: numpy's divider and the device's give NaNs of different sign; the header documents
    0x7fc00000, and the reference's NaN - any NaN - is brought to it"""
    rec = rec.copy()
    nan = np.isnan(np.ascontiguousarray(rec[:, 3]).view(np.float32))
    rec[nan, 3] = 0x7fc00000
    return rec


def _check_records(rec, count, ref, cap, what):
    for g, want in enumerate(ref):
        want = _one_nan(want)
        assert count[g] == len(want), (what, g, int(count[g]), len(want))
        k = min(len(want), cap)
        bad = np.argwhere(rec[g, :k] != want[:k])
        assert bad.size == 0, (what, g, "first differing (record, field)", bad[0].tolist(), rec[g, bad[0][0]], want[bad[0][0]])
        assert (rec[g, k:] == GARBAGE).all(), (what, g, "a record beyond the count was written")


@functools.lru_cache(maxsize=None)
def _reference(n, G):
    """name -> (table, stats, iou4, offsets, reference kept lists, reference records), computed once per size"""
    off = ar.split_offsets(n, G)
    out = {}
    for name, t in ar.tables(n).items():
        stats, iou4 = ar.make_stats(t)
        out[name] = (t, stats, iou4, off, ar.nms_groups(t["boxes"], t["scores"], off, t["thr"][2]),
                     ar.select_groups(stats, iou4, off, t["thr"]))
    return out


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_every_table_at_every_size(dev, n, G):
    for name, (t, stats, iou4, off, ref_kept, ref_rec) in _reference(n, G).items():
        cap = _maxg(off)
        kept, count = _box_nms(dev, t["boxes"], t["scores"], off, t["thr"][2])
        _check_kept(kept, count, ref_kept, cap, (name, n, G, "int32 boxes"))
        kept, count = _box_nms(dev, t["boxes"].astype(np.float32), t["scores"], off, t["thr"][2])
        _check_kept(kept, count, ref_kept, cap, (name, n, G, "fp32 boxes"))
        rec, count = _amg_select(dev, stats, iou4, off, t["thr"])
        _check_records(rec, count, ref_rec, cap, (name, n, G))


def test_fractional_fp32_boxes(dev):
    """the fp32 form with coordinates that are no integers (and so no int32 form): equal to nms_xyxy on the same floats"""
    rng = np.random.default_rng(11)
    n = 257
    x0, y0 = rng.random(n, dtype=np.float32) * 300, rng.random(n, dtype=np.float32) * 300
    b = np.stack([x0, y0, x0 + rng.random(n, dtype=np.float32) * 150, y0 + rng.random(n, dtype=np.float32) * 150], 1).astype(np.float32)
    s = rng.random(n, dtype=np.float32)
    for thr in (0.1, 0.5):
        ref = ar.nms_groups(b, s, [0, n], thr)
        assert 10 < len(ref[0]) < n
        _check_kept(*_box_nms(dev, b, s, [0, n], thr), ref, n, ("fractional", thr))


def test_capacity_16384_clustered(dev):
    """the largest group the kernels take: 16384 boxes in 200 tight clusters, about 200 kept"""
    n = 16384
    t = ar.t_clustered(n)
    ref = ar.nms_groups(t["boxes"], t["scores"], [0, n], 0.7)
    assert 150 <= len(ref[0]) <= 200
    _check_kept(*_box_nms(dev, t["boxes"], t["scores"], [0, n], 0.7), ref, n, "clustered")
    stats, iou4 = ar.make_stats(t)
    _check_records(*_amg_select(dev, stats, iou4, [0, n], t["thr"]), ar.select_groups(stats, iou4, [0, n], t["thr"]), n, "clustered")


def test_cap_below_the_kept_count(dev):
    """count reports every kept row; only the first cap are stored, and nothing is written behind them"""
    n = 257
    for G in (1, 3):
        t, stats, iou4, off, ref_kept, ref_rec = _reference(n, G)["random_nms1"]
        assert max(len(k) for k in ref_kept) > 5
        for cap in (1, 5):
            _check_kept(*_box_nms(dev, t["boxes"], t["scores"], off, 1.0, cap=cap), ref_kept, cap, ("cap", cap, G))
            _check_records(*_amg_select(dev, stats, iou4, off, t["thr"], cap=cap), ref_rec, cap, ("cap", cap, G))


def test_repeatable_and_scratch_shared_in_stream_order(dev):
    """two calls on different tables through the default (cached) scratch without a wait between them, then the first again"""
    from protosam_amd import ops
    n = 256
    ref = _reference(n, 1)
    outs = []
    for name in ("equal_scores", "chain", "equal_scores"):
        t = ref[name][0]
        outs.append(ops.box_nms(torch.from_numpy(t["boxes"]).to(dev), torch.from_numpy(t["scores"]).to(dev), [0, n], t["thr"][2]))
    torch.cuda.synchronize()
    for name, (kept, count) in zip(("equal_scores", "chain", "equal_scores"), outs):
        want = ref[name][4][0]
        assert int(count[0]) == len(want) and np.array_equal(kept[0, :len(want)].cpu().numpy(), want), name


def test_refused_arguments(dev):
    """refused on the host, nothing launched: outputs keep their garbage"""
    from protosam_amd import _lib, ops
    n = 64
    t, stats, iou4, off, _, _ = _reference(n, 1)["random"]
    boxes, scores = torch.from_numpy(t["boxes"]).to(dev), torch.from_numpy(t["scores"]).to(dev)
    d_stats, d_iou4 = torch.from_numpy(stats).to(dev), torch.from_numpy(iou4).to(dev)
    kept, count, out = Guarded(n, dev), Guarded(1, dev), Guarded(n * ar.REC + 1, dev)
    scr = _scratch(1, n, dev)
    kw = dict(kept=kept.view.view(1, n), count=count.view, scratch=scr.view)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.box_nms(boxes.cpu(), scores, off, 0.7, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.box_nms(boxes, scores.cpu(), off, 0.7, **kw)
    with pytest.raises(TypeError):
        ops.box_nms(boxes.long(), scores, off, 0.7, **kw)
    with pytest.raises(TypeError):
        ops.box_nms(boxes, scores.double(), off, 0.7, **kw)
    with pytest.raises(ValueError):
        ops.box_nms(boxes.view(-1), scores, off, 0.7, **kw)
    with pytest.raises(ValueError):
        ops.box_nms(boxes, scores[:-1], off, 0.7, **kw)
    for bad in ([0, n - 1], [1, n], [0, 40, 30, n], [0], [n]):
        with pytest.raises(ValueError, match="offsets"):
            ops.box_nms(boxes, scores, bad, 0.7, **kw)
    with pytest.raises(ValueError, match="cap"):
        ops.box_nms(boxes, scores, off, 0.7, cap=0, **kw)
    with pytest.raises(RuntimeError, match="psam_box_nms failed with status 1"):    # a NaN threshold; the scratch of a smaller call
        ops.box_nms(boxes, scores, off, float("nan"), **kw)
    with pytest.raises(RuntimeError, match="psam_box_nms failed with status 1"):
        ops.box_nms(boxes, scores, off, 0.7, kept=kept.view.view(1, n), count=count.view, scratch=scr.view[:16])
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.box_nms(boxes, scores, off, 0.7, kept=kept.view.view(1, n), count=count.view, scratch=scr.view[1:])
    # over capacity: one group of 16385
    big = ops.NMS_MAX_GROUP + 1
    bb, bs = torch.zeros((big, 4), dtype=torch.int32, device=dev), torch.zeros((big,), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="exceeds the capacity of 16384"):
        ops.box_nms(bb, bs, [0, big], 0.7)
    with pytest.raises(ValueError, match="exceeds the capacity of 16384"):
        ops.amg_select(torch.zeros((big, 8), dtype=torch.int32, device=dev), torch.zeros(((big + 2) // 3, 4), device=dev), [0, big],
                       0.0, 0.0, 0.7)
    ops.box_nms(bb, bs, [0, 1, big], 0.7, cap=4)                                   # (two groups of it are fine)
    with pytest.raises(RuntimeError):
        ops.nms_workspace(1, big)
    with pytest.raises(RuntimeError):
        ops.nms_workspace(0, 4)
    # psam_amg_select
    skw = dict(out=out.view, scratch=scr.view)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.amg_select(d_stats.cpu(), d_iou4, off, 0.88, 0.95, 0.7, **skw)
    with pytest.raises(TypeError):
        ops.amg_select(d_stats.float(), d_iou4, off, 0.88, 0.95, 0.7, **skw)
    with pytest.raises(TypeError):
        ops.amg_select(d_stats, d_iou4.double(), off, 0.88, 0.95, 0.7, **skw)
    with pytest.raises(ValueError):
        ops.amg_select(d_stats, d_iou4[:-1], off, 0.88, 0.95, 0.7, **skw)
    with pytest.raises(ValueError):
        ops.amg_select(d_stats[:, :7].contiguous(), d_iou4, off, 0.88, 0.95, 0.7, **skw)
    with pytest.raises(RuntimeError, match="psam_amg_select failed with status 1"):
        ops.amg_select(d_stats, d_iou4, off, 0.88, float("nan"), 0.7, **skw)
    # the C entry points themselves: null pointers, sizes out of range
    L = _lib.lib()

    def raw(**k):
        a = dict(boxes=boxes.data_ptr(), fp32=0, scores=scores.data_ptr(), off=ops._nms_groups(off, n, dev)[0].data_ptr(), n=n, G=1,
                 maxg=n, thr=0.7, kept=kept.view.data_ptr(), cap=n, count=count.view.data_ptr(), scr=scr.view.data_ptr(),
                 nbytes=scr.view.numel() * 8)
        a.update(k)
        return L.psam_box_nms(a["boxes"], a["fp32"], a["scores"], a["off"], a["n"], a["G"], a["maxg"], a["thr"], a["kept"], a["cap"],
                              a["count"], a["scr"], a["nbytes"], ops._stream())

    for k in (dict(boxes=0), dict(scores=0), dict(off=0), dict(kept=0), dict(count=0), dict(scr=0), dict(nbytes=0), dict(n=-1),
              dict(G=0), dict(G=65536), dict(maxg=0), dict(maxg=16385), dict(cap=0), dict(boxes=boxes.data_ptr() + 4),
              dict(scr=scr.view.data_ptr() + 8)):
        assert raw(**k) == 1, k
    torch.cuda.synchronize()
    for gb in (kept, count, out):
        assert bool((gb.view == GARBAGE).all()) and gb.intact()
    assert scr.intact() and bool((scr.view == GARBAGE).all())
    assert raw() == 0                                                              # (the arguments the cases above vary are good)
    torch.cuda.synchronize()
    assert int(count.view[0]) == len(_reference(n, 1)["random"][4][0])


def test_offsets_that_break_the_rules_on_the_device(dev):
    """the C entry point cannot see device offsets: a group that leaves [0, n], descends or exceeds max_group reports -1 and
    writes nothing else; the groups beside it are unaffected"""
    from protosam_amd import _lib, ops
    n = 64
    t, _, _, _, _, _ = _reference(n, 1)["random"]
    boxes, scores = torch.from_numpy(t["boxes"]).to(dev), torch.from_numpy(t["scores"]).to(dev)
    for off, bad_groups in (([0, 20, 80], [1]), ([0, 40, 30, 64], [1]), ([0, 10, 64], [1]), ([-1, 10, 20], [0])):
        G, maxg = len(off) - 1, 48
        kept, count, scr = Guarded(G * maxg, dev), Guarded(G, dev), _scratch(G, maxg, dev)
        d_off = torch.tensor(off, dtype=torch.int32, device=dev)
        st = _lib.lib().psam_box_nms(boxes.data_ptr(), 0, scores.data_ptr(), d_off.data_ptr(), n, G, maxg, 0.7, kept.view.data_ptr(),
                                     maxg, count.view.data_ptr(), scr.view.data_ptr(), scr.view.numel() * 8, ops._stream())
        torch.cuda.synchronize()
        assert st == 0 and kept.intact() and count.intact() and scr.intact()
        k, c = kept.view.view(G, maxg).cpu().numpy(), count.view.cpu().numpy()
        for g in range(G):
            if g in bad_groups:
                assert c[g] == -1 and (k[g] == GARBAGE).all(), (off, g)
            else:
                want = ar.nms_groups(t["boxes"][off[g]:off[g + 1]], t["scores"][off[g]:off[g + 1]], [0, off[g + 1] - off[g]], 0.7)[0]
                assert c[g] == len(want) and np.array_equal(k[g, :len(want)], want), (off, g)
