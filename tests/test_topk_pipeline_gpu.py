"""GPU: ProtoSAM with PSAM_TOPK_POINTS=device - the k most confident pixels of every component from psam_topk_points_batch
instead of the host's torch.topk.

Models as tests/test_reference_records_gpu.py builds them: given coarse logits (protosam_amd/synth_cases.py), SAM ViT-B with
synthetic weights and the orchestration depth. The points are checked against tests/topk_reference.py run on the model's own
probability and arg-max planes, labelled by oracle.ccl.label.
"""
import numpy as np
import pytest
import torch

import topk_reference as tr
from oracle import ccl as occl

pytestmark = pytest.mark.gpu


class FixedCoarse:
    """Coarse-model stand-in returning given logits; for a batch, slice b gets them rolled by (7 b, -5 b)"""

    def __init__(self, logits):
        self.logits = logits

    def __call__(self, inp):
        B = inp.qry_imgs[0].shape[0]
        if B == 1:
            return self.logits.clone()
        return torch.cat([torch.roll(self.logits, (7 * b, -5 * b), (-2, -1)) for b in range(B)])


def _model(dev, logits=None, mode="device", monkeypatch=None, **kw):
    from protosam_amd import synth_cases as gi
    from protosam_amd.protosam import ProtoSAM
    if monkeypatch is not None:
        monkeypatch.setenv("PSAM_TOPK_POINTS", mode)
    spec = f"random:vit_b:{gi.ORCH_SAM_SEED}:{gi.ORCH_SAM_DEPTH}"
    logits = gi.orch_coarse_logits() if logits is None else logits
    m = ProtoSAM((1024, 1024), FixedCoarse(logits.to(dev)), spec, use_sam_trans=True, **kw).to(dev).eval()
    m.sam.postprocess_variant = "batched"
    if monkeypatch is None:
        m.topk_points = mode
    return m


def _inputs(dev, B=1):
    from protosam_amd import synth_cases as gi
    from protosam_amd.protosam import InputFactory, TYPE_ALPNET
    q = gi.orch_query()
    q = torch.cat([torch.roll(q, (7 * b, -5 * b), (-2, -1)) for b in range(B)]).contiguous().to(dev)
    inp = InputFactory.create_input(TYPE_ALPNET, q, support_images=[q[:1]], support_labels=[torch.zeros(1, 512, 512)],
                                    isval=True, val_wsize=2)
    return q, inp


def _plane_reference(model, plane, k):
    """topk_reference on the model's own planes -> (n, labels, p_fg, keys [n, k])"""
    bb = model._bbufs
    pfg = bb["prob"][plane, 1].cpu().numpy()
    pred = bb["pred"][plane].cpu().numpy()
    n, lab = occl.label(pred)
    return n, lab, pfg, tr.topk_keys(lab, pfg, n, k, max(n, 1))


def test_switch_default_and_values(dev, monkeypatch):
    monkeypatch.delenv("PSAM_TOPK_POINTS", raising=False)
    from protosam_amd import synth_cases as gi
    from protosam_amd.protosam import ProtoSAM
    spec = f"random:vit_b:{gi.ORCH_SAM_SEED}:{gi.ORCH_SAM_DEPTH}"
    build = lambda: ProtoSAM((1024, 1024), FixedCoarse(gi.orch_coarse_logits()), spec, num_points_for_sam=3)   # noqa: E731
    assert build().topk_points == "host"
    monkeypatch.setenv("PSAM_TOPK_POINTS", "device")
    assert build().topk_points == "device"
    monkeypatch.setenv("PSAM_TOPK_POINTS", "gpu")
    with pytest.raises(ValueError, match="PSAM_TOPK_POINTS"):
        build()


CASES = [("default", 3, {}), ("conf_pts", 3, {}), ("cca", 2, {}), ("default", 12, {})]


@pytest.mark.parametrize("name,k,extra", CASES, ids=[f"{c[0]}-k{c[1]}" for c in CASES])
def test_device_points_equal_reference(dev, monkeypatch, name, k, extra):
    from protosam_amd import synth_cases as gi
    kw = dict(gi.ORCH_FLAGS[name], **extra)
    assert kw.get("use_bbox") or name != "default"
    model = _model(dev, mode="device", monkeypatch=monkeypatch, num_points_for_sam=k, **kw)
    assert model.topk_points == "device"
    q, inp = _inputs(dev)
    pred, scores = model(q, inp, degrees_rotate=0)
    st = model.last_stats
    n, lab, pfg, ref = _plane_reference(model, 0, k)
    tab = st["table"]
    rows = range(n)
    if kw["use_cca"]:                                           # the most confident component only (table row -> its index)
        stats = occl.component_stats(lab, n, pfg, int((lab != 0).sum()))
        best = [c for c in range(n) if (stats["best_x"][c], stats["best_y"][c]) == (tab[0][8], tab[0][9])]
        assert len(best) == 1
        rows = best
    assert len(st["prompts"][0]) == len(rows) == len(scores)
    for coords, c in zip(st["prompts"][0], rows):
        want = [tr.decode(v, 1024) for v in ref[c]]
        assert None not in want, f"component {c} has fewer than {k} pixels"
        assert [tuple(pt) for pt in coords[:k]] == [(float(x), float(y)) for x, y, _ in want], c
    assert pred.shape == (512, 512)


@pytest.mark.parametrize("name,k", [("default", 3), ("conf_pts", 3), ("cca", 2), ("default", 12)])
def test_host_and_device_choose_equal_probabilities(dev, name, k):
    """tied points may be other pixels; the number of prompt sets and each component's descending probabilities may not differ"""
    from protosam_amd import synth_cases as gi
    q, inp = _inputs(dev)
    lists = {}
    for mode in ("host", "device"):
        model = _model(dev, mode=mode, num_points_for_sam=k, **gi.ORCH_FLAGS[name])
        model(q, inp, degrees_rotate=0)
        pfg = model._bbufs["prob"][0, 1].cpu().numpy()
        lists[mode] = [[pfg[int(y), int(x)] for x, y in coords[:k]] for coords in model.last_stats["prompts"][0]]
        assert all(v == sorted(v, reverse=True) for v in lists[mode])
    assert len(lists["host"]) == len(lists["device"]) > 0 and lists["host"] == lists["device"]


@pytest.fixture
def same_kernels(monkeypatch):
    """Kernel choices that do not follow the size of a call, for comparing a batch with its parts bit for bit: by default the
    GEMM tile, the folded LayerNorm, the captured graphs of one- and two-slice encoder forwards and the key split of the
    token-to-image attention follow the number of rows / prompt sets, and a slice's mask then differs from the per-slice
    forward's in a few pixels on the threshold WHATEVER finds the points (measured on these inputs: 11 / 20 / 14 pixels with
    the host's torch.topk, 11 / 21 / 14 with the device keys; tests/test_protosam_gpu.py bounds that by 32 pixels). With these
    switches (the ones test_mixed_support_batch_equals_per_support_batches uses, and the environment's) the arithmetic of a
    slice is the same in both calls. The models are built inside the test, after the environment is set."""
    from protosam_amd import ops
    for name in ("PSAM_OVERLAP_STREAMS", "PSAM_HIPGRAPH", "PSAM_T2I_SPLIT", "PSAM_FOLD_LN"):
        monkeypatch.setenv(name, "0")
    ops.gemm_set_tile(1)
    yield
    ops.gemm_set_tile(0)


def test_forward_batch_equals_per_slice(dev, same_kernels):
    """forward_batch on 3 slices against the three forward calls, device mode: points, scores and masks bit for bit"""
    from protosam_amd import synth_cases as gi
    B, k = 3, 3
    model = _model(dev, mode="device", num_points_for_sam=k, **gi.ORCH_FLAGS["default"])
    q, inp = _inputs(dev, B)
    res = model.forward_batch(q, inp)
    per = [dict(prompts=s["prompts"]) for s in model.last_stats["per_slice"]]
    masks = [r[0].clone() for r in res]
    scores = [list(r[1]) for r in res]
    single = _model(dev, mode="device", num_points_for_sam=k, **gi.ORCH_FLAGS["default"])
    flips = []
    for b in range(B):
        single.coarse_segmentation_model.logits = torch.roll(model.coarse_segmentation_model.logits, (7 * b, -5 * b), (-2, -1))
        p1, s1 = single(q[b:b + 1], inp, degrees_rotate=0)
        flips.append(int((masks[b] != p1).sum()))
        print(f"slice {b}: {flips[-1]} mask pixels differ from the per-slice forward")
        assert single.last_stats["prompts"] == per[b]["prompts"] and [float(v) for v in s1] == [float(v) for v in scores[b]], b
        n, lab, pfg, ref = _plane_reference(single, 0, k)
        assert len(per[b]["prompts"][0]) == n
        for c, coords in enumerate(per[b]["prompts"][0]):
            assert [tuple(pt) for pt in coords[:k]] == [(float(x), float(y)) for x, y, _ in (tr.decode(v, 1024) for v in ref[c])]
    assert flips == [0] * B, flips


def _classes_against_batches(dev, B, mode="device"):
    """forward_classes_batch on B slices x C classes and forward_batch once per class, conf points with use_cca and k = 3, built the
    way tests/test_protosam_classes_gpu.py sets num_points_for_sam -> ({(b, c): differing mask pixels}, prompt sets per class);
    asserts the prompt sets themselves"""
    from test_protosam_classes_gpu import _build, _inp, _multi
    kw = dict(use_bbox=False, use_points=True, point_mode="conf", use_cca=True)
    model, _ = _build(dev, "random:vit_b:1234:2", 2, **kw)
    model.num_points_for_sam = 3
    model.topk_points = mode
    s_img, s_masks, qs = _multi(dev, B=B)
    C = len(s_masks)
    res = model.forward_classes_batch(qs, s_img, s_masks)
    st = model.last_stats
    got = {(b, c): (res[b][c][0].clone(), list(res[b][c][1]), st["prompts"].get((b, c))) for b in range(B) for c in range(C)}
    worst, sets = {}, [0] * C
    for c in range(C):
        per = model.forward_batch(qs, _inp(dev, qs, s_img, s_masks[c]))
        stats = model.last_stats["per_slice"] if B > 1 else [model.last_stats]
        for b in range(B):
            m, sc, prompts = got[(b, c)]
            if prompts is None:
                assert sc == [0] and "prompts" not in stats[b]
                continue
            sets[c] += 1
            worst[(b, c)] = int((m.to(per[b][0].dtype) != per[b][0]).sum())
            assert prompts == stats[b]["prompts"], (b, c)
            assert len(prompts[0]) == 1 and len(prompts[0][0]) == 3 + 1   # k points and the padding point
            assert [float(v) for v in sc] == [float(v) for v in per[b][1]] or worst[(b, c)], (b, c)
    print(f"{mode}, B = {B}: prompt sets per class {sets}, differing mask pixels {worst}")
    return worst, sets


def test_forward_classes_batch_equals_forward_batch_per_class(dev, same_kernels):
    """forward_classes_batch with k = 3 against forward_batch per class, device mode: prompt sets, scores and masks bit for bit.
    Four slices, so that every per-class call has four prompt sets of nine tokens: the decoder's token-side linears take their
    split-K form from 32 rows on (TwoWayAttentionBlock._run), and a per-class call of three sets (27 rows) would go through
    another kernel than the all-class call - measured there: every prompt set identical, one mask pixel of twelve pairs differs."""
    worst, sets = _classes_against_batches(dev, 4)
    assert min(sets) * 9 >= 32, sets
    assert not any(worst.values()), worst


@pytest.mark.parametrize("mode", ["host", "device"])
def test_small_component_raises(dev, mode):
    """a component of 2 pixels and k = 3: torch.topk's RuntimeError on the host (as the reference), a named one on the device"""
    from protosam_amd import synth_cases as gi
    logits = gi.orch_empty_logits(1024)                        # at the SAM input size: the softmax sees these pixels as they are
    logits[0, 1, 100:160, 200:300], logits[0, 0, 100:160, 200:300] = 3.0, -3.0
    logits[0, 1, 300, 40:42], logits[0, 0, 300, 40:42] = 3.0, -3.0
    model = _model(dev, logits=logits, mode=mode, num_points_for_sam=3, **gi.ORCH_FLAGS["conf_pts"])
    q, inp = _inputs(dev)
    with pytest.raises(RuntimeError) as err:
        model(q, inp, degrees_rotate=0)
    if mode == "device":
        assert "num_points_for_sam = 3" in str(err.value) and "component 1" in str(err.value)
