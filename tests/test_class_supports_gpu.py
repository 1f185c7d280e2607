"""Multi-class batches with a support set of their own per class, per z-part and per shot count.

  psam_alp_sim_pairs against psam_alp_sim per entry (+ torch.maximum over the shots), bit for bit
  FewShotSeg.class_scores_supports against forward_groups per class, bit for bit
  ProtoSAM / ProtoMedSAM forward_classes_batch(supports=...) against forward_batch(q, supports[c]) per class, the old argument form
  against supports= with the same support, runner.run_slices_class_supports against per-class run_slices, and the errors
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_protosam_gpu import _build   # noqa: E402


# ---- the kernel ----------------------------------------------------------------------------------------------------------------
def _bank(dev, g, pool_w, seed, C=768, shifted=0.0):
    from protosam_amd import ops
    gen = torch.Generator().manual_seed(seed)
    tok = torch.randn((g * g, C), generator=gen).to(dev)
    yy, xx = torch.meshgrid(torch.arange(64), torch.arange(64), indexing="ij")
    cy, cx = 20 + 7 * (seed % 4) + shifted, 24 + 5 * (seed % 3)
    mask = (((yy - cy) / 14.0) ** 2 + ((xx - cx) / 17.0) ** 2 <= 1.0).float().to(dev).contiguous()
    return ops.alp_bank(tok, C, g, g, C, mask, pool_w, 4, 0.95, 1e-4)


@pytest.mark.parametrize("g", [37, 73])
def test_alp_sim_pairs_bit_identical(dev, g):
    from protosam_amd import ops
    from protosam_amd.alpmodule import MultiProtoAsConv
    C, B = 768, 3
    gen = torch.Generator().manual_seed(g)
    qry = torch.randn((B, g * g, C), generator=gen).to(dev)
    small = g // 9                                  # pool so that (g // pool)^2 + 1 <= 96: a bank of one 96-prototype group
    banks = [_bank(dev, g, small, 1), _bank(dev, g, 2, 2), _bank(dev, g, 2, 3, shifted=3.0), _bank(dev, g, small, 4),
             _bank(dev, g, 2, 5)]
    assert (banks[0].cap + 95) // 96 == 1 and (banks[1].cap + 95) // 96 > 1
    merged = MultiProtoAsConv.merge_banks([banks[2], banks[3], banks[4]], 0)      # a 3-shot set's background bank
    banks.append(merged)
    # class 0: one single-group bank for all slices; class 1: slice 0 on a multi-group bank, slices 1-2 on the 3-shot set
    runs = [[(0, [0], B)], [(1, [1], 1), (5, [2, 3, 4], 2)]]
    entries, n_planes = ops.plan_alp_pairs(runs, B)
    out = ops.alp_sim_pairs(qry, g * g * C, C, B, g * g, C, banks, entries, n_planes)
    ref = torch.empty_like(out)
    for (k, b, which, plane) in entries:
        r = ops.alp_sim(qry[b:b + 1], g * g * C, C, 1, g * g, C, banks[k])[0, which]
        first = all(e[3] != plane for e in entries[:entries.index((k, b, which, plane))])
        ref[plane] = r if first else torch.maximum(ref[plane], r)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref)
    # the same bank against every slice: the planes of psam_alp_sim's own batched launch
    entries, n_planes = ops.plan_alp_pairs([[(1, [1], B)]], B)
    one = ops.alp_sim_pairs(qry, g * g * C, C, B, g * g, C, banks, entries, n_planes)
    assert torch.equal(one.view(B, 2, g * g), ops.alp_sim(qry, g * g * C, C, B, g * g, C, banks[1]))


# ---- the models ----------------------------------------------------------------------------------------------------------------
def _inp(dev, q, imgs, masks):
    from protosam_amd.protosam import InputFactory, TYPE_ALPNET
    inp = InputFactory.create_input(TYPE_ALPNET, q, support_images=list(imgs), support_labels=list(masks), isval=True, val_wsize=2)
    inp.to(dev)
    return inp


def _queries(q, B):
    qs = [q]
    for i in range(1, B):
        v = torch.roll(q, (7 * i, -5 * i), (-2, -1))
        qs.append(torch.flip(v, (-1,)) if i % 2 else v)
    return torch.cat(qs).contiguous()


def _class_supports(dev, S, B, C=3, splits=((3, 3), (2, 4), (4, 2)), two_shot=2):
    """B query slices and C classes; class c takes support image (c, p) for z-part p (its own support slice per part, synthetic
    images of different seeds), with run lengths splits[c]; class `two_shot` has two shots per part."""
    from protosam_amd.synth import synth_pair_multi
    pairs = {sd: synth_pair_multi(S, seed=sd) for sd in range(1, 8)}
    qs = _queries(pairs[1][2], B).to(dev)
    supports = []
    for c in range(C):
        runs = []
        for p, n in enumerate(splits[c]):
            sd = 1 + (2 * c + p) % 7
            imgs, masks = [pairs[sd][0].to(dev)], [pairs[sd][1][c].to(dev)]
            if c == two_shot:
                sd2 = 1 + (2 * c + p + 3) % 7
                imgs.append(pairs[sd2][0].to(dev))
                masks.append(pairs[sd2][1][c].to(dev))
            runs.append((_inp(dev, qs, imgs, masks), n))
        supports.append(runs)
    return qs, supports


def test_fewshot_class_scores_supports_equal_forward_groups(dev):
    from protosam_amd import ops
    model, _ = _build(dev, "random:vit_b:1234:1", 2)
    alp = model.coarse_segmentation_model.model
    qs, supports = _class_supports(dev, 512, 6)
    sc = alp.class_scores_supports(supports, qs)
    C, B, g = sc.shape[0], sc.shape[1], sc.shape[-1]
    assert sc.shape == (3, 6, 2, g, g)
    for c in range(C):
        ref = alp.forward_groups(qs, [(i.supp_imgs, i.fore_mask, i.back_mask, i.isval, i.val_wsize, n) for i, n in supports[c]])
        got = ops.bilinear_nchw(sc[c].contiguous(), 512, 512)
        assert torch.equal(got, ref), c
    # one input for all slices (no run list) is the single-run case
    sc1 = alp.class_scores_supports([supports[0][0][0]], qs)
    ref = alp.forward_groups(qs, [(supports[0][0][0].supp_imgs, supports[0][0][0].fore_mask, supports[0][0][0].back_mask, True, 2,
                                   6)])
    assert torch.equal(ops.bilinear_nchw(sc1[0].contiguous(), 512, 512), ref)


def _compare(res, ref, c, tol=2e-3):
    for b in range(len(ref)):
        m, s = res[b][c]
        p1, s1 = ref[b]
        d = int((m.to(p1.dtype) != p1).sum()) if m.shape == p1.shape else int(m.sum()) + int(p1.sum())
        assert d <= 32, (b, c, d)
        assert len(s) == len(s1) and np.allclose(np.array(s, dtype=np.float64), np.array(s1, dtype=np.float64), atol=tol), (b, c)


FLAGS = [dict(use_bbox=True, use_points=True, point_mode="both", use_cca=False),
         dict(use_bbox=False, use_points=True, point_mode="both", use_neg_points=True),
         dict(use_bbox=False, use_points=False, use_mask=True, use_cca=True)]


@pytest.mark.parametrize("kw", FLAGS, ids=[str(i) for i in range(len(FLAGS))])
def test_protosam_supports_equal_forward_batch_per_class(dev, kw):
    model, _ = _build(dev, "random:vit_b:1234:2", 2, **kw)
    qs, supports = _class_supports(dev, 512, 6)
    res = model.forward_classes_batch(qs, supports=supports)
    assert len(res) == 6 and len(res[0]) == 3
    assert res[0][0][0].dtype == torch.uint8 and res[0][0][0].shape == (512, 512)
    n_prompted = model.last_stats["n_prompted"]
    assert n_prompted > 0
    for c in range(3):
        _compare(res, model.forward_batch(qs, supports[c]), c)


def test_protosam_supports_coarse_pred_only(dev):
    model, _ = _build(dev, "random:vit_b:1234:1", 2, use_bbox=True, use_points=True, point_mode="both", coarse_pred_only=True)
    qs, supports = _class_supports(dev, 512, 6)
    res = model.forward_classes_batch(qs, supports=supports)
    for c in range(3):
        _compare(res, model.forward_batch(qs, supports[c]), c)


def test_old_form_equals_supports_form(dev):
    from protosam_amd.synth import synth_pair_multi
    model, _ = _build(dev, "random:vit_b:1234:2", 2, use_bbox=True, use_points=True, point_mode="both")
    s_img, s_masks, q, _ = synth_pair_multi(512, seed=0)
    s_img, s_masks = s_img.to(dev), [m.to(dev) for m in s_masks]
    qs = _queries(q, 3).to(dev)
    old = model.forward_classes_batch(qs, s_img, s_masks)
    st_old = model.last_stats
    old_masks = [[old[b][c][0].clone() for c in range(4)] for b in range(3)]
    old_scores = [[list(old[b][c][1]) for c in range(4)] for b in range(3)]
    low_old = st_old["low_res"].clone()
    new = model.forward_classes_batch(qs, supports=[_inp(dev, qs, [s_img], [m]) for m in s_masks])
    st_new = model.last_stats
    assert st_new["spans"] == st_old["spans"]
    assert torch.equal(st_new["low_res"], low_old)
    for b in range(3):
        for c in range(4):
            assert torch.equal(new[b][c][0], old_masks[b][c]) and list(new[b][c][1]) == old_scores[b][c]


def test_errors(dev):
    from protosam_amd.synth import synth_pair_multi
    model, _ = _build(dev, "random:vit_b:1234:1", 1, use_bbox=True, use_points=True, point_mode="both")
    qs, supports = _class_supports(dev, 512, 6)
    bad = [supports[0], [(supports[1][0][0], 2), (supports[1][1][0], 3)], supports[2]]
    with pytest.raises(ValueError, match="do not sum"):
        model.forward_classes_batch(qs, supports=bad)
    s2, m2, _, _ = synth_pair_multi(256, seed=0)
    other = _inp(dev, qs, [s2.to(dev)], [m2[0].to(dev)])
    with pytest.raises(ValueError, match="size"):
        model.forward_classes_batch(qs, supports=[supports[0], other, supports[2]])
    with pytest.raises(NotImplementedError):
        model.forward_classes_batch(qs, supports=supports, degrees_rotate=10)
    with pytest.raises(TypeError):
        model.forward_classes_batch(qs, supports[0][0][0].supp_imgs[0][0], [supports[0][0][0].fore_mask[0][0]], supports=supports)
    with pytest.raises(ValueError):
        model.forward_classes_batch(qs, supports=[])


def test_run_slices_class_supports_vs_run_slices(dev):
    from protosam_amd.runner import class_part_table, part_assign, run_slices, run_slices_class_supports, support_set
    from protosam_amd.synth import ellipse_mask, synth_volume
    S, Z = 512, 12
    model, _ = _build(dev, "random:vit_b:1234:2", 2, use_bbox=True, use_points=True, point_mode="both")
    vol, _ = synth_volume(Z, S, seed=0)
    svol, slab = synth_volume(Z, S, seed=1)
    vol = vol.to(dev)
    sup_imgs, sup_masks = support_set(svol.to(dev), slab.to(dev))
    extra = torch.from_numpy(ellipse_mask(S, 0.3, 0.7, 0.1, 0.12)[None]).to(dev)
    masks = [sup_masks, [extra] * 3]                      # class c, part p: sup_imgs[p] with masks[c][p]
    supports = [[_inp(dev, vol[:1], [sup_imgs[p]], [masks[c][p]]) for p in range(3)] for c in range(2)]
    # every class spans the whole scan: its part table is run_slices' equal z-chunks
    lab = np.ones((Z, 2, 2), dtype=np.int64)
    lab[:, 1] = 2
    table = class_part_table(lab, [1, 2])
    assert table.tolist() == [[part_assign(z, Z) for z in range(Z)]] * 2
    zs = list(range(Z))
    mc, stc = run_slices_class_supports(model, vol, supports, table, zs, batch=5)       # batches 0-4, 5-9, 10-11 straddle parts
    assert mc.shape == (Z, 2, S, S) and mc.dtype == torch.uint8 and int(mc.sum()) > 0
    for c in range(2):
        m1, _ = run_slices(model, vol, sup_imgs, masks[c], zs, dev, batch=5)
        diffs = [int((mc[z, c] != m1[z]).sum()) for z in zs]
        assert max(diffs) <= 32, (c, diffs)
    assert all(0 <= s <= 2 for s in stc)


# ---- ProtoMedSAM ---------------------------------------------------------------------------------------------------------------
def test_protomedsam_supports_equal_forward_batch_per_class(dev):
    from test_protomedsam_batch_gpu import _medsam_small
    model, _, _ = _medsam_small(dev)
    qs, supports = _class_supports(dev, 1024, 4, splits=((2, 2), (1, 3), (3, 1)))
    res = model.forward_classes_batch(qs, supports=supports)
    assert len(res) == 4 and len(res[0]) == 3
    for c in range(3):
        ref = model.forward_batch(qs, supports[c])
        for b in range(4):
            m, s = res[b][c]
            p1, s1 = ref[b]
            assert m.shape == p1.shape and int((m.to(p1.dtype) != p1).sum()) <= 32, (b, c)
            assert np.allclose(np.asarray(s[0], dtype=np.float64), np.asarray(s1[0], dtype=np.float64), atol=2e-3), (b, c)


# ---- full depth ----------------------------------------------------------------------------------------------------------------
def test_full_depth_config4_supports_vs_forward_batch_per_class(dev):
    """Config 4's model (DINOv2 ViT-B/14 + SAM ViT-H, 512^2, full depth): B = 4 slices straddling two parts x C = 4 classes, each
    (class, part) with its own support, one class with two shots, against forward_batch once per class."""
    from protosam_amd.runner import build_protosam
    model, _ = build_protosam(dev, "vit_h", 512)
    model.overlap_streams = "0"
    qs, supports = _class_supports(dev, 512, 4, C=4, splits=((2, 2), (1, 3), (3, 1), (2, 2)), two_shot=1)
    res = model.forward_classes_batch(qs, supports=supports)
    st = model.last_stats
    worst_p = worst_s = 0.0
    for c in range(4):
        ref = model.forward_batch(qs, supports[c])
        rst = model.last_stats
        for (b, start, cnt) in rst["spans"]:
            first, n = st["spans"][(b, c)]
            assert n == cnt
            a = torch.sigmoid(st["low_res"][first:first + n, st["sel"]])
            r = torch.sigmoid(rst["low_res"][start:start + cnt, rst["sel"]])
            worst_p = max(worst_p, (a - r).abs().max().item())
            worst_s = max(worst_s, float(np.abs(np.array(res[b][c][1], dtype=np.float64) -
                                                np.array(ref[b][1], dtype=np.float64)).max()))
            assert int((res[b][c][0].to(ref[b][0].dtype) != ref[b][0]).sum()) <= 32
    print(f"full depth supports B=4 x C=4: max |d sigmoid(low_res)| {worst_p:.2e}, max |d score| {worst_s:.2e}")
    assert worst_p <= 1e-3 and worst_s <= 1e-3
