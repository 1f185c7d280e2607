"""ProtoSAM.forward_classes_batch: B slices x C classes of one support image in one call (one SAM encoder pass per slice).

  psam_scores_prob_argmax against psam_bilinear_nchw + psam_prob_argmax, bit for bit
  psam_neg_points_batch against per-plane psam_neg_points, bit for bit
  forward_classes_batch against per-class forward (every prompt mode), the CPU oracle, an overflowing plane, coarse_pred_only,
  runner.run_slices_classes, and forward_batch per class at full depth (SAM ViT-H, 512^2)
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_many_components_gpu import _blob_logits   # noqa: E402
from test_protosam_gpu import _build, _dice           # noqa: E402


def _scores(P, g, seed, empty=()):
    gen = torch.Generator().manual_seed(seed)
    sc = torch.randn((P, 2, g, g), generator=gen) * 3.0
    for p in empty:
        sc[p, 0], sc[p, 1] = 5.0, -5.0
    return sc


# O: the output size, square, or (OH, OW). The last cases are the edges test_resample_kernels_gpu.py anchors the chain at: an odd
# output width (the per-pixel store path and a partly filled last group of four), a non-square output, and an output equal to the
# image size (no second resize) with an odd and with a multiple-of-four width.
@pytest.mark.parametrize("P,g,IH,IW,O", [(9, 37, 512, 512, 1024), (9, 73, 1024, 1024, 1024), (10, 37, 300, 517, 1024),
                                          (9, 20, 97, 131, 250),
                                          pytest.param(9, 37, 300, 517, (1001, 999), id="9-37-300-517-1001x999"),
                                          pytest.param(9, 20, 97, 131, (250, 333), id="9-20-97-131-250x333"),
                                          pytest.param(9, 37, 301, 517, (301, 517), id="9-37-301-517-same"),
                                          pytest.param(9, 20, 64, 48, (64, 48), id="9-20-64-48-same"),
                                          pytest.param(9, 20, 97, 131, (3, 1025), id="9-20-97-131-3x1025")])
def test_scores_prob_argmax_bit_identical(dev, P, g, IH, IW, O):
    from protosam_amd import ops
    OH, OW = O if isinstance(O, tuple) else (O, O)
    sc = _scores(P, g, P + g, empty=(1, 4, 7)).to(dev)
    fg_ref = torch.zeros(P, dtype=torch.int32, device=dev)
    prob_ref, pred_ref = ops.prob_argmax(ops.bilinear_nchw(sc, IH, IW), OH, OW, fg_sum=fg_ref)
    fg = torch.zeros(P, dtype=torch.int32, device=dev)
    prob, pred = ops.scores_prob_argmax(sc, IH, IW, OH, OW, fg_sum=fg)
    torch.cuda.synchronize()
    assert torch.equal(prob, prob_ref) and torch.equal(pred, pred_ref) and torch.equal(fg, fg_ref)
    assert int(fg[1]) == 0 and int(fg.max()) > 0


def _blob_planes(dev, S=512):
    """uint8 / logit planes: 0 components, 1 component, 80 > MAX_NEG_COMPONENTS components, 5 components."""
    logits = [torch.zeros((1, 2, S, S)) + torch.tensor([4.0, -4.0]).view(1, 2, 1, 1)]
    one = logits[0].clone()
    one[0, 1, 100:300, 150:400], one[0, 0, 100:300, 150:400] = 2.0, -1.0
    logits.append(one)
    many = logits[0].clone()
    for k in range(80):
        y, x = 10 + 55 * (k // 9), 10 + 55 * (k % 9)
        many[0, 1, y:y + 20, x:x + 20 + k % 4] = 1.0 + 0.05 * k
        many[0, 0, y:y + 20, x:x + 20 + k % 4] = -1.0
    logits.append(many)
    logits.append(_blob_logits(5, S))
    return torch.cat(logits).to(dev)


@pytest.mark.parametrize("max_comp", [64, 3])
def test_neg_points_batch_bit_identical(dev, max_comp):
    from protosam_amd import ops
    S = 512
    logits = _blob_planes(dev, S)
    P = logits.shape[0]
    prob, pred = ops.prob_argmax(logits, S, S)
    cw = ops.CclWorkspace(S, S, 256, dev, slots=P)
    ops.ccl_batch(pred, prob, cw)
    n = [int(t[1]) for t in cw.tabs.cpu().numpy()]
    assert n[0] == 0 and n[1] == 1 and n[2] == 80 > 64
    keys = ops.neg_points_batch(cw.labels_b[:P], prob[:, 0], cw.tabs[:P], max_comp)
    for p in range(P):
        ref = ops.neg_points(cw, prob[p, 0].contiguous(), cw.tabs[p], max_comp, labels=cw.labels_b[p])
        assert torch.equal(keys[p], ref), p
    assert int(keys[2, 1:].ne(0).sum()) == max_comp


# ---- the model -------------------------------------------------------------------------------------------------------------
EMPTY = {(0, 2)} | {(2, c) for c in range(4)}    # class 2 on slice 0, and every class on slice 2


def _multi(dev, B=3):
    from protosam_amd.synth import synth_pair_multi
    s_img, s_masks, q, _ = synth_pair_multi(512, seed=0)
    qs = [q]
    for i in range(1, B):
        v = torch.roll(q, (7 * i, -5 * i), (-2, -1))
        qs.append(torch.flip(v, (-1,)) if i % 2 else v)
    return s_img.to(dev), [m.to(dev) for m in s_masks], torch.cat(qs).contiguous().to(dev)


def _force_empty(model, empty):
    alp = model.coarse_segmentation_model.model
    orig = alp.class_scores

    def patched(*a, **k):
        sc = orig(*a, **k)
        for (b, c) in empty:
            if b < sc.shape[1]:
                sc[c, b, 0], sc[c, b, 1] = 5.0, -5.0
        return sc
    alp.class_scores = patched


def _inp(dev, q, s_img, m):
    from protosam_amd.protosam import InputFactory, TYPE_ALPNET
    inp = InputFactory.create_input(TYPE_ALPNET, q, support_images=[s_img], support_labels=[m], isval=True, val_wsize=2)
    inp.to(dev)
    return inp


FLAGS = [dict(use_bbox=False, use_points=True, point_mode="conf", use_cca=False),
         dict(use_bbox=True, use_points=True, point_mode="centroid", use_cca=False),
         dict(use_bbox=True, use_points=True, point_mode="both", use_cca=True),
         dict(use_bbox=False, use_points=True, point_mode="both", use_neg_points=True),
         dict(use_bbox=False, use_points=False, use_mask=True),
         dict(use_bbox=False, use_points=False, use_mask=True, use_cca=True),
         dict(use_bbox=True, use_points=True, point_mode="conf", use_mask=True),
         dict(use_bbox=False, use_points=True, point_mode="conf", use_cca=True, k=3)]


@pytest.mark.parametrize("kw", FLAGS, ids=[str(i) for i in range(len(FLAGS))])
def test_forward_classes_batch_equals_per_class_forward(dev, kw):
    kw = dict(kw)
    k = kw.pop("k", 1)
    model, _ = _build(dev, "random:vit_b:1234:2", 2, **kw)
    model.num_points_for_sam = k
    s_img, s_masks, qs = _multi(dev)
    B, C = qs.shape[0], len(s_masks)
    _force_empty(model, EMPTY)
    calls = []
    enc = model.sam.image_encoder
    orig = enc.encode_patches
    enc.encode_patches = lambda patches, n, **kk: (calls.append(n), orig(patches, n, **kk))[1]
    res = model.forward_classes_batch(qs, s_img, s_masks)
    st = model.last_stats
    enc.encode_patches = orig
    assert calls == [2] and st["n_encoded"] == 2                 # slice 2 is empty for every class
    out = res[0][0][0]
    assert out.dtype == torch.uint8 and out.shape == (512, 512)
    assert st["n_prompted"] == B * C - len(EMPTY) == len(st["prompt"])
    for b in range(B):
        for c in range(C):
            m, sc = res[b][c]
            assert m.dtype == torch.uint8 and m.shape == (512, 512)
            if (b, c) in EMPTY:
                assert int(m.sum()) == 0 and sc == [0] and (b, c) not in st["prompt"]
                continue
            p1, s1 = model(qs[b:b + 1], _inp(dev, qs[b:b + 1], s_img, s_masks[c]))
            d = int((m.to(p1.dtype) != p1).sum())
            assert p1.shape == m.shape and d <= 32, (b, c, d)
            assert len(sc) == len(s1) and np.allclose(np.array(sc, dtype=np.float64), np.array(s1, dtype=np.float64), atol=2e-3)
    # one slice: the prompt tables and coordinates are those of per-class forward
    res1 = model.forward_classes_batch(qs[:1], s_img, s_masks)
    st1 = model.last_stats
    for c in range(C):
        p1, s1 = model(qs[:1], _inp(dev, qs[:1], s_img, s_masks[c]))
        ref = model.last_stats
        if c == 2 and (0, 2) in EMPTY:
            continue
        assert st1["n_components"][0][c] == ref["n_components"]
        assert st1["spans"][(0, c)][1] == ref["n_prompts"]
        if not model._mask_only:
            cs, ls = st1["prompts"][(0, c)]
            assert ls == ref["prompts"][1] and np.array_equal(np.asarray(cs, dtype=np.float64),
                                                             np.asarray(ref["prompts"][0], dtype=np.float64))
        assert int((res1[0][c][0].to(p1.dtype) != p1).sum()) <= 32


def test_forward_classes_batch_vs_oracle(dev):
    """B = 1 slice x 4 classes against the CPU oracle of each class, with test_protosam_forward_vs_oracle's tolerances. On a class
    where per-class `forward` itself is farther than 1e-3 from the oracle on sigmoid(low_res), the bound is forward's error."""
    from oracle import alp as oalp, dinov2 as odino, glue
    from protosam_amd.synth import synth_state_dict
    kw = dict(use_bbox=True, use_points=True, point_mode="both", use_cca=False)
    sam_depth, dino_depth = 3, 4
    model, alp_sd = _build(dev, f"random:vit_b:1234:{sam_depth}", dino_depth, **kw)
    sam_sd = {k: v.cpu() for k, v in synth_state_dict(model.sam, 1234).items()}
    s_img, s_masks, qs = _multi(dev, B=1)
    res = model.forward_classes_batch(qs, s_img, s_masks)
    st = model.last_stats
    enc_sd = {k[len("encoder."):]: v for k, v in alp_sd.items() if k.startswith("encoder.")}
    enc = lambda im: odino.forward_features(im, enc_sd, "dinov2_b14", depth=dino_depth)["x_norm_patchtokens"]  # noqa
    q = qs.cpu()
    for c, m in enumerate(s_masks):
        logits_ref = oalp.fewshot_forward(enc, s_img.cpu(), m.cpu(), q, 512)
        taps = {}
        pred_ref, scores_ref = glue.protosam_forward(q, logits_ref, sam_sd, "vit_b", encoder_depth=sam_depth, taps=taps, **kw)
        first, cnt = st["spans"][(0, c)]
        assert cnt == taps["cc"][0] - 1 and len(res[0][c][1]) == len(scores_ref)
        low = st["low_res"][first:first + cnt, st["sel"]].cpu()
        low_ref = torch.stack([l[0] for l in taps["low_res"]])
        perr = (torch.sigmoid(low) - torch.sigmoid(low_ref)).abs().max().item()
        model(qs, _inp(dev, qs, s_img, m))
        fst = model.last_stats
        ferr = (torch.sigmoid(fst["low_res"][:, fst["sel"]].cpu()) - torch.sigmoid(low_ref)).abs().max().item()
        d = _dice(res[0][c][0].cpu(), pred_ref)
        print(f"class {c}: comps {cnt}, max |dprob(low_res)| {perr:.3e} (per-class forward {ferr:.3e}), Dice {d:.5f}")
        assert d >= 0.999 and perr < max(1e-3, 1.05 * ferr)
        assert np.abs(np.array(res[0][c][1], dtype=np.float64) - np.array(scores_ref)).max() < 1e-3


class _FixedClasses:
    """Stands in for the coarse model: grid-resolution class scores [C,B,2,g,g] (`class_scores`), and for per-class `forward`
    the logits FewShotSeg.forward would give for slice `b`, class `c` (the scores resized to the image size)."""

    def __init__(self, sc, size):
        self.sc, self.size, self.model, self.b, self.c = sc, size, self, 0, 0

    def class_scores(self, supp_img, fore_masks, qry_imgs, isval=True, val_wsize=None):
        return self.sc.clone()

    def __call__(self, cin):
        from protosam_amd import ops
        return ops.bilinear_nchw(self.sc[self.c, self.b:self.b + 1].contiguous(), self.size, self.size)


@pytest.mark.parametrize("kw", [dict(use_bbox=True, use_points=True, point_mode="both", use_neg_points=True),
                                dict(use_bbox=False, use_points=False, use_mask=True)])
def test_overflowing_class_plane_is_relabelled(dev, monkeypatch, kw):
    """A class plane with more components than the fast table holds (MAX_COMPONENTS lowered to 8, 12 blobs) is relabelled with
    the large table and agrees with per-class forward; 12 > MAX_NEG_COMPONENTS also takes the full ring search."""
    from protosam_amd import protosam as psmod
    monkeypatch.setattr(psmod, "MAX_COMPONENTS", 8)
    monkeypatch.setattr(psmod, "MAX_NEG_COMPONENTS", 3)
    model, _ = _build(dev, "random:vit_b:1234:1", 1, **kw)
    s_img, s_masks, qs = _multi(dev, B=2)
    g = 512
    sc = torch.stack([torch.cat([_blob_logits(12, g), _blob_logits(5, g)]), torch.cat([_blob_logits(3, g), _blob_logits(12, g)])])
    fixed = _FixedClasses(sc.to(dev).contiguous(), 512)
    model.coarse_segmentation_model = fixed
    res = model.forward_classes_batch(qs, s_img, s_masks[:2])
    st = model.last_stats
    assert st["n_components"] == [[12, 3], [5, 12]]
    assert st["spans"][(0, 0)][1] == 12 and st["spans"][(1, 1)][1] == 12
    for b in range(2):
        for c in range(2):
            fixed.b, fixed.c = b, c
            p1, s1 = model(qs[b:b + 1], _inp(dev, qs[b:b + 1], s_img, s_masks[c]))
            m, s = res[b][c]
            assert int((m.to(p1.dtype) != p1).sum()) <= 32
            assert len(s) == len(s1) and np.allclose(np.array(s, dtype=np.float64), np.array(s1, dtype=np.float64), atol=2e-3)


@pytest.mark.parametrize("use_cca", [False, True])
def test_coarse_pred_only_and_errors(dev, use_cca):
    model, _ = _build(dev, "random:vit_b:1234:1", 2, use_bbox=True, use_points=True, point_mode="both", use_cca=use_cca,
                      coarse_pred_only=True)
    s_img, s_masks, qs = _multi(dev)
    res = model.forward_classes_batch(qs, s_img, s_masks)
    for b in range(qs.shape[0]):
        for c in range(len(s_masks)):
            p1, s1 = model(qs[b:b + 1], _inp(dev, qs[b:b + 1], s_img, s_masks[c]))
            m, s = res[b][c]
            assert m.shape == p1.shape and int((m != p1).sum()) <= 32
            assert np.allclose(np.array(s, dtype=np.float64), np.array(s1, dtype=np.float64), atol=2e-3)
    with pytest.raises(NotImplementedError):
        model.forward_classes_batch(qs, s_img, s_masks, degrees_rotate=10)
    with pytest.raises(NotImplementedError):
        model.forward_classes_batch(qs, [s_img, s_img], s_masks)
    with pytest.raises(NotImplementedError):
        model.forward_classes_batch(qs, torch.cat([s_img, s_img]), s_masks)
    with pytest.raises(NotImplementedError):
        model.forward_classes_batch(qs, [(s_img, 1), (s_img, 2)], s_masks)
    with pytest.raises(NotImplementedError):
        model.forward_classes_batch(qs, s_img, [[m, m] for m in s_masks])


def test_run_slices_classes_drives_protosam(dev):
    from protosam_amd.runner import run_slices, run_slices_classes, support_set
    from protosam_amd.synth import ellipse_mask, synth_volume
    S = 512
    model, _ = _build(dev, "random:vit_b:1234:2", 2, use_bbox=True, use_points=True, point_mode="both")
    vol, _ = synth_volume(6, S, seed=0)
    svol, slab = synth_volume(6, S, seed=1)
    vol = vol.to(dev)
    sup_imgs, sup_masks = support_set(svol.to(dev), slab.to(dev))
    extra = torch.from_numpy(ellipse_mask(S, 0.3, 0.7, 0.1, 0.12)[None]).to(dev)
    per_part = [[m, extra] for m in sup_masks]
    zs = list(range(6))
    mc, stc = run_slices_classes(model, vol, sup_imgs, per_part, zs, dev, batch=4)
    assert mc.shape == (6, 2, S, S) and mc.dtype == torch.uint8 and int(mc.sum()) > 0
    for c in range(2):
        # per-class run_slices on the same batches (cut at the z-parts): the encoders see the same slices per call
        m1, _ = run_slices(model, vol, sup_imgs, [pp[c] for pp in per_part], zs, dev, batch=4, mix_parts=False)
        diffs = [int((mc[z, c] != m1[z]).sum()) for z in zs]
        assert max(diffs) <= 32, (c, diffs)
    assert all(0 <= s <= 2 for s in stc)


def test_full_depth_config4_vs_forward_batch_per_class(dev):
    """Config 4's model (DINOv2 ViT-B/14 + SAM ViT-H, 512^2, full depth): B = 4 x C = 4 against forward_batch once per class."""
    from protosam_amd.runner import build_protosam
    model, _ = build_protosam(dev, "vit_h", 512)
    model.overlap_streams = "0"
    s_img, s_masks, qs = _multi(dev, B=4)
    res = model.forward_classes_batch(qs, s_img, s_masks)
    st = model.last_stats
    worst_p = worst_s = 0.0
    for c, m in enumerate(s_masks):
        ref = model.forward_batch(qs, _inp(dev, qs, s_img, m))
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
    print(f"full depth B=4 x C=4: max |d sigmoid(low_res)| {worst_p:.2e}, max |d score| {worst_s:.2e}")
    assert worst_p <= 1e-3 and worst_s <= 1e-3
