"""GPU: the batched ProtoMedSAM paths (BASELINE config 5 with many slices per call) and their two kernels.

  psam_prob2_argmax   against the chain it replaces: bilinear_nchw -> prob_argmax -> prob_argmax
  psam_mask_union_seg against psam_mask_union + .to(torch.uint8), per segment
  ProtoMedSAM.forward_classes_batch against the CPU oracle (reduced depth), the full-depth record, and per-slice forward_classes
  ProtoMedSAM.forward_batch against per-slice forward (one support set, mixed supports, empty slices, use_cca=False, coarse only)
  runner.run_slices / run_slices_classes driving a ProtoMedSAM
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-3
CFG = {"which_model": "dinov2_b14", "cls_name": "grid_proto", "proto_grid_size": 8, "lora": 0, "align": False,
       "debug": False}


def _empty(conf):
    """`forward`'s result for an empty coarse mask carries the int 0 as its score list"""
    return len(conf) == 1 and isinstance(conf[0], int) and conf[0] == 0


def _dice(a, b):
    a, b = a.float(), b.float()
    return float(2 * (a * b).sum() / (a.sum() + b.sum() + 1e-8))


def _unpack(bits, S):
    return torch.from_numpy(np.unpackbits(bits)[:S * S].reshape(S, S).astype(np.float32))


# ---- kernels ----------------------------------------------------------------------------------------------------------------
# IH: the square input size of a 1024^2 output, or (IH, IW, OH, OW). The tuples are the edges test_resample_kernels_gpu.py anchors
# psam_prob_argmax at: an odd output width (the per-pixel store path, a partly filled last group of four), non-square maps, and
# the same-size path with an odd and with a multiple-of-four width.
@pytest.mark.parametrize("IH", [73, 1024,
                                pytest.param((41, 53, 251, 333), id="41x53-251x333"),
                                pytest.param((73, 61, 3, 1023), id="73x61-3x1023"),
                                pytest.param((47, 51, 47, 51), id="47x51-same"),
                                pytest.param((64, 52, 64, 52), id="64x52-same")])
def test_prob2_argmax_equals_chain(dev, IH):
    from protosam_amd import ops
    IH, IW, OH, OW = IH if isinstance(IH, tuple) else (IH, IH, 1024, 1024)
    g = torch.Generator().manual_seed(7 + IH)
    sc = torch.randn((12, 2, IH, IW), generator=g) * 4.0
    ties = torch.randn((2, 1, IH, IW), generator=g)
    sc = torch.cat([sc, ties.expand(2, 2, IH, IW),                          # exact ties everywhere: argmax -> class 0
                    torch.stack([torch.full((IH, IW), 3.0), torch.full((IH, IW), -3.0)])[None]])   # no foreground at all
    sc[3, :, 5:40, 7:50] = 0.25                                               # a tied patch inside a random plane
    P = sc.shape[0]
    sc = sc.contiguous().to(dev)
    # the chain it replaces: resize, softmax + arg-max, softmax again (ProtoMedSAM.py:176-187, util/utils.py:485)
    full = ops.bilinear_nchw(sc, OH, OW) if (IH, IW) != (OH, OW) else sc
    fg_ref = torch.zeros(P, dtype=torch.int32, device=dev)
    prob_ref, pred_ref = ops.prob_argmax(full.contiguous(), OH, OW, fg_sum=fg_ref)
    p2_ref, _ = ops.prob_argmax(prob_ref, OH, OW)
    fg = torch.zeros(P, dtype=torch.int32, device=dev)
    prob = torch.empty((P, 2, OH, OW), dtype=torch.float32, device=dev)
    pred, pfg2 = ops.prob2_argmax(sc, OH, OW, fg_sum=fg, prob=prob)
    assert torch.equal(pred, pred_ref)
    assert torch.equal(fg, fg_ref) and int(fg[-1]) == 0 and int(fg[-2]) == 0 and int(fg[0]) > 0
    d = (pfg2 - p2_ref[:, 1]).abs().max().item()
    print(f"prob2_argmax {IH}x{IW}->{OH}x{OW}: max |dpfg2| {d:.2e}")
    # pred and the counts are exact. The probabilities can differ from the chain in the last bit: bilinear_nchw_kernel resamples one
    # plane at a time, the fused kernels interpolate the two classes together (packed FMAs), so the compiler contracts the
    # interpolation's multiply-adds differently. prob_argmax with its own resize is the same arithmetic as the fused kernel.
    assert d <= 1e-6
    assert (prob - prob_ref).abs().max().item() <= 1e-6
    prob_direct, pred_direct = ops.prob_argmax(sc, OH, OW)
    assert torch.equal(prob, prob_direct) and torch.equal(pred, pred_direct)
    # without the optional outputs
    fg2 = torch.zeros(P, dtype=torch.int32, device=dev)
    pred2, pfg22 = ops.prob2_argmax(sc, OH, OW, fg_sum=fg2)
    assert torch.equal(pred2, pred) and torch.equal(pfg22, pfg2) and torch.equal(fg2, fg)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("MID,OUT", [(1024, 1024), (1024, 512), (512, 1001)])
def test_mask_union_seg_equals_mask_union(dev, variant, MID, OUT):
    from protosam_amd import ops
    g = torch.Generator().manual_seed(variant * 31 + OUT)
    Pm, C = 7, 3
    low = (torch.randn((Pm, C, 256, 256), generator=g) * 3.0).to(dev)
    thr = 0.5 if variant == 3 else 0.0
    sel = 1
    # segments of 1, 3, 0 and 3 prompts, written to outputs out of order
    table = [(0, 1, 2), (1, 3, 0), (4, 0, 3), (4, 3, 1)]
    segs = torch.tensor(table, dtype=torch.int32, device=dev)
    out = torch.full((4, OUT, OUT), 7, dtype=torch.uint8, device=dev)
    ops.mask_union_seg(low, sel, segs, 4, MID, OUT, variant, thr, out=out)
    for first, cnt, o in table:
        if cnt == 0:
            assert int(out[o].count_nonzero()) == 0
            continue
        ref = ops.mask_union(low[first:first + cnt].contiguous(), sel, MID, OUT, variant, thr).to(torch.uint8)
        assert torch.equal(out[o], ref), (variant, first, cnt)
        assert 0 < int(ref.sum()) < OUT * OUT


# ---- models -----------------------------------------------------------------------------------------------------------------
def _medsam_small(dev, S=1024, **kw):
    from protosam_amd.grid_proto_fewshot import FewShotSeg
    from protosam_amd.protomedsam import ProtoMedSAM
    from protosam_amd.protosam import ALPNetWrapper
    from protosam_amd.synth import synth_state_dict
    alp = FewShotSeg(S, None, dict(CFG, encoder_depth=2))
    alp_sd = synth_state_dict(alp, 1234)
    alp.load_state_dict(alp_sd)
    alp = alp.to(dev).eval()
    kw.setdefault("use_cca", True)
    model = ProtoMedSAM((1024, 1024), ALPNetWrapper(alp), "random:vit_b:1234:2", **kw).to(dev).eval()
    return model, alp, alp_sd


def _four_masks(S, s_m):
    from protosam_amd.synth import ellipse_mask
    return [s_m] + [torch.from_numpy(ellipse_mask(S, cy, cx, ry, rx)[None]) for cy, cx, ry, rx in
                    ((0.25, 0.3, 0.1, 0.12), (0.7, 0.72, 0.14, 0.09), (0.3, 0.75, 0.08, 0.15))]


def test_forward_classes_batch_vs_oracle(dev):
    """test_config5_medsam_1024_four_classes with three query slices in one call."""
    from oracle import alp as oalp, dinov2 as odino, glue
    from protosam_amd import ops
    from protosam_amd.synth import synth_pair, synth_state_dict
    S = 1024
    model, alp, alp_sd = _medsam_small(dev)
    sam_sd = {k: v.cpu() for k, v in synth_state_dict(model.medsam, 1234).items()}
    s_img, s_m, _, _ = synth_pair(S, seed=2)
    qs = torch.cat([synth_pair(S, seed=sd)[2] for sd in (2, 3, 5)])
    masks = _four_masks(S, s_m)
    s_d, m_d, q_d = s_img.to(dev), [m.to(dev) for m in masks], qs.to(dev)
    res = model.forward_classes_batch(q_d, s_d, m_d)
    # the coarse probabilities of the same call's class scores
    sc = alp.class_scores(s_d, m_d, q_d, isval=True, val_wsize=2)
    C, B = sc.shape[:2]
    assert (C, B) == (4, 3)
    prob = torch.empty((C * B, 2, S, S), dtype=torch.float32, device=dev)
    ops.prob2_argmax(sc.view(C * B, 2, sc.shape[-2], sc.shape[-1]), S, S, prob=prob)
    enc_sd = {k[len("encoder."):]: v for k, v in alp_sd.items() if k.startswith("encoder.")}
    enc = lambda im: odino.forward_features(im, enc_sd, "dinov2_b14", depth=2)["x_norm_patchtokens"]  # noqa: E731
    ran = 0
    for b in range(B):
        for c, m in enumerate(masks):
            logits_ref = oalp.fewshot_forward(enc, s_img, m, qs[b:b + 1], S)
            perr = (prob[c * B + b].cpu() - logits_ref[0].softmax(0)).abs().max().item()
            seg_ref, _ = glue.protomedsam_forward(qs[b:b + 1], logits_ref, sam_sd, "vit_b", use_cca=True, encoder_depth=2)
            seg, conf = res[b][c]
            assert seg.shape == (S, S) and perr < TOL, (b, c, perr)
            if int(seg_ref.sum()) == 0:
                assert int(seg.sum()) == 0 and _empty(conf)
                continue
            d = _dice(seg.cpu(), seg_ref)
            print(f"slice {b} class {c}: coarse prob err {perr:.2e}, Dice {d:.5f}")
            assert seg.dtype == torch.uint8 and int(seg.sum()) > 0 and d >= 0.999
            ran += 1
    assert ran >= 1


@pytest.fixture(scope="module")
def full_cfg5(dev):
    from protosam_amd.grid_proto_fewshot import FewShotSeg
    from protosam_amd.protomedsam import ProtoMedSAM
    from protosam_amd.protosam import ALPNetWrapper
    from protosam_amd.runner import ALP_CFG
    from protosam_amd.synth import synth_state_dict
    from protosam_amd.synth_cases import cfg5_inputs
    alp = FewShotSeg(1024, None, dict(ALP_CFG))
    alp.load_state_dict(synth_state_dict(alp, 1234))
    alp = alp.to(dev).eval()
    model = ProtoMedSAM((1024, 1024), ALPNetWrapper(alp), "random:vit_b:1234", use_cca=True).to(dev).eval()
    s_img, s_masks, q_img = cfg5_inputs()
    return model, alp, s_img.to(dev), [m.to(dev) for m in s_masks], q_img.to(dev)


def _rolls(q):
    """four distinct slices around the cfg5 query (every organ stays inside the slice)"""
    return torch.cat([q, torch.roll(q, (9, -13), (-2, -1)), torch.roll(q, (-17, 6), (-2, -1)), torch.flip(q, (-1,))])


def test_forward_classes_batch_vs_full_depth_record(dev, full_cfg5):
    from protosam_amd import ops
    from protosam_amd.metrics import dice
    model, alp, s_d, m_d, q_d = full_cfg5
    gold = np.load(os.path.join(GOLD, "fullsize_cfg5.npz"))
    S = 1024
    qs = _rolls(q_d)[[1, 0, 2, 3]].contiguous()                # the record's query at position 1
    res = model.forward_classes_batch(qs, s_d, m_d)
    st = model.last_stats
    low = st["low_res"].cpu()
    sc = alp.class_scores(s_d, m_d, qs, isval=True, val_wsize=2)
    C, B = sc.shape[:2]
    prob = torch.empty((C * B, 2, S, S), dtype=torch.float32, device=dev)
    ops.prob2_argmax(sc.view(C * B, 2, sc.shape[-2], sc.shape[-1]), S, S, prob=prob)
    ran = 0
    for ci in range(4):
        cp = prob[ci * B + 1, 1, ::4, ::4].cpu()
        cerr = (cp - torch.from_numpy(gold[f"class{ci}_coarse_p"].astype(np.float32) / 65535.0)).abs().max().item()
        seg, conf = res[1][ci]
        ref_mask = _unpack(gold[f"class{ci}_mask"], S)
        assert seg.shape == (S, S) and cerr <= TOL
        if f"class{ci}_prob" not in gold.files:
            assert int(seg.sum()) == 0
            continue
        ran += 1
        k = st["prompt"][(1, ci)]
        perr = (torch.sigmoid(low[k, 0]) - torch.from_numpy(gold[f"class{ci}_prob"].astype(np.float32) / 65535.0)).abs().max().item()
        ce = float(np.abs(np.asarray(conf[0]) - gold[f"class{ci}_conf"]).max())
        d = dice(seg.cpu().float(), ref_mask)
        flips = int((seg.cpu().float() != ref_mask).sum())
        print(f"batched config 5 class {ci}: coarse prob err {cerr:.2e}, max |dprob(low_res)| {perr:.2e}, conf err {ce:.2e}, "
              f"Dice {d:.5f} ({flips} px)")
        assert perr <= TOL and ce <= TOL and (d >= 0.998 or flips <= 8)
    assert ran == 4


def test_forward_classes_batch_equals_per_slice(dev, full_cfg5):
    model, alp, s_d, m_d, q_d = full_cfg5
    qs = _rolls(q_d)
    res = model.forward_classes_batch(qs, s_d, m_d)
    st = model.last_stats
    low_b = st["low_res"]
    worst = [0.0, 0.0, 0]
    for b in range(4):
        r1 = model.forward_classes(qs[b:b + 1], s_d, m_d)
        low1 = model.last_stats["low_res"]
        k1 = 0
        for c in range(4):
            seg, conf = res[b][c]
            seg1, conf1 = r1[c]
            assert seg.shape == seg1.shape
            diff = int((seg.cpu().to(torch.uint8) != seg1.cpu().to(torch.uint8)).sum())
            if _empty(conf1):
                assert _empty(conf) and int(seg.sum()) == 0
                continue
            k = st["prompt"][(b, c)]
            dp = (torch.sigmoid(low_b[k, 0]) - torch.sigmoid(low1[k1, 0])).abs().max().item()
            dc = float(np.abs(np.asarray(conf[0]) - np.asarray(conf1[0])).max())
            k1 += 1
            worst = [max(worst[0], dp), max(worst[1], dc), max(worst[2], diff)]
            assert dp <= TOL and dc <= TOL and diff <= 64, (b, c, dp, dc, diff)
    print(f"forward_classes_batch (B = 4) vs per-slice forward_classes: max |dsigmoid(low_res)| {worst[0]:.2e}, "
          f"max |dconf| {worst[1]:.2e}, max differing px {worst[2]}")
    assert st["n_prompted"] == 16 and st["n_encoded"] == 4


def _inp(q, s_img, m):
    from protosam_amd.protosam import InputFactory, TYPE_ALPNET
    inp = InputFactory.create_input(TYPE_ALPNET, q, support_images=[s_img], support_labels=[m], isval=True, val_wsize=2)
    inp.to(q.device)
    return inp


def _agree(a, b, what):
    (sa, ca), (sb, cb) = a, b
    assert sa.shape == sb.shape, what
    if _empty(cb):
        assert _empty(ca) and int(sa.sum()) == 0, what
        return 0, 0.0
    diff = int((sa.to(torch.uint8) != sb.to(torch.uint8)).sum())
    dc = float(np.abs(np.asarray(ca[0]) - np.asarray(cb[0])).max())
    assert sa.dtype == torch.uint8 and diff <= 64 and dc <= TOL, (what, diff, dc)
    return diff, dc


def test_forward_batch_equals_per_slice(dev):
    from protosam_amd.synth import synth_pair
    S = 1024
    model, alp, _ = _medsam_small(dev)
    s_img, s_m, _, _ = synth_pair(S, seed=2)
    s_img2, s_m2, _, _ = synth_pair(S, seed=3)
    qs = torch.cat([synth_pair(S, seed=sd)[2] for sd in (2, 3, 5)]).to(dev)
    inA = _inp(qs, s_img.to(dev), s_m.to(dev))
    inB = _inp(qs, s_img2.to(dev), s_m2.to(dev))
    batched = model.forward_batch(qs, inA)
    assert len(batched) == 3 and len(model.last_stats["per_slice"]) == 3
    low_b = model.last_stats["low_res"]
    per = model.last_stats["per_slice"]
    for b in range(3):
        one = model(qs[b:b + 1], _inp(qs[b:b + 1], s_img.to(dev), s_m.to(dev)))
        diff, dc = _agree(batched[b], one, f"slice {b}")
        if not _empty(one[1]):
            dp = (torch.sigmoid(low_b[per[b]["prompt"], 0]) - torch.sigmoid(model.last_stats["low_res"][0, 0])).abs().max().item()
            print(f"forward_batch slice {b}: {diff} px, |dconf| {dc:.2e}, |dsigmoid(low_res)| {dp:.2e}")
            assert dp <= TOL
    # mixed supports: the first two slices against support A, the third against support B
    mixed = model.forward_batch(qs, [(inA, 2), (inB, 1)])
    split = model.forward_batch(qs[:2], inA) + model.forward_batch(qs[2:], inB)
    for b in range(3):
        _agree(mixed[b], split[b], f"mixed slice {b}")


class _Forced:
    """Wraps the coarse model and overwrites chosen slices' logits: 'empty' = background everywhere, 'one' / 'two' = one / two
    separate squares of foreground."""

    def __init__(self, real, forced):
        self.real, self.forced, self.model = real, forced, real.model

    def __call__(self, inp):
        lg = self.real(inp).clone()
        for b, kind in self.forced.items():
            fg = torch.full(lg.shape[-2:], -10.0, device=lg.device)
            if kind in ("one", "two"):
                fg[100:200, 100:200] = 10.0
            if kind == "two":
                fg[600:700, 600:700] = 10.0
            lg[b, 1], lg[b, 0] = fg, -fg
        return lg


def test_forward_batch_empty_slice_and_errors(dev):
    from protosam_amd.synth import synth_pair
    S = 1024
    model, alp, _ = _medsam_small(dev)
    s_img, s_m, _, _ = synth_pair(S, seed=2)
    qs = torch.cat([synth_pair(S, seed=sd)[2] for sd in (2, 3, 5)]).to(dev)
    inp = _inp(qs, s_img.to(dev), s_m.to(dev))
    real = model.coarse_segmentation_model
    enc = model.medsam.image_encoder
    calls = []
    orig = enc.encode_patches
    enc.encode_patches = lambda patches, B, *a, **k: (calls.append(B), orig(patches, B, *a, **k))[1]
    try:
        ref = model.forward_batch(qs, inp)
        calls.clear()
        model.coarse_segmentation_model = _Forced(real, {1: "empty"})
        out = model.forward_batch(qs, inp)
        assert calls == [2]                                                   # only the two slices with a component
        assert _empty(out[1][1]) and out[1][0].dtype == torch.int64 and int(out[1][0].sum()) == 0 and out[1][0].shape == (S, S)
        for b in (0, 2):
            _agree(out[b], ref[b], f"slice {b} beside an empty one")
        model.use_cca = False
        model.coarse_segmentation_model = _Forced(real, {0: "one", 1: "one", 2: "two"})
        with pytest.raises(NotImplementedError, match="slice 2"):
            model.forward_batch(qs, inp)
    finally:
        enc.encode_patches = orig
        model.coarse_segmentation_model = real
        model.use_cca = True


def test_forward_batch_coarse_pred_only(dev):
    from protosam_amd.synth import synth_pair
    S = 1024
    for use_cca in (False, True):
        model, alp, _ = _medsam_small(dev, use_cca=use_cca, coarse_pred_only=True)
        s_img, s_m, _, _ = synth_pair(S, seed=2)
        qs = torch.cat([synth_pair(S, seed=sd)[2] for sd in (2, 3, 5)]).to(dev)
        batched = model.forward_batch(qs, _inp(qs, s_img.to(dev), s_m.to(dev)))
        for b in range(3):
            pred, conf = model(qs[b:b + 1], _inp(qs[b:b + 1], s_img.to(dev), s_m.to(dev)))
            pb, cb = batched[b]
            assert pb.shape == pred.shape and pb.dtype == pred.dtype
            assert int((pb != pred).sum()) <= 64 and abs(float(cb[0]) - float(conf[0])) <= TOL


def test_runner_drives_protomedsam(dev):
    from protosam_amd.runner import run_slices, run_slices_classes, support_set
    from protosam_amd.synth import ellipse_mask, synth_volume
    S = 1024
    model, alp, _ = _medsam_small(dev)
    vol, _ = synth_volume(6, S, seed=0)
    svol, slab = synth_volume(6, S, seed=1)
    vol = vol.to(dev)
    sup_imgs, sup_masks = support_set(svol.to(dev), slab.to(dev))
    zs = list(range(6))
    m1, st1 = run_slices(model, vol, sup_imgs, sup_masks, zs, dev, batch=1)
    m4, st4 = run_slices(model, vol, sup_imgs, sup_masks, zs, dev, batch=4)      # batches span z-parts (mixed supports)
    assert m4.shape == (6, S, S) and m4.dtype == torch.uint8
    diffs = [int((m4[z] != m1[z]).sum()) for z in zs]
    print(f"run_slices batch 4 vs 1: differing px per slice {diffs}, prompts {st4}")
    assert max(diffs) <= 64 and int(m1.sum()) > 0 and all(s in (0, 1) for s in st4)
    extra = torch.from_numpy(ellipse_mask(S, 0.3, 0.7, 0.1, 0.12)[None]).to(dev)
    per_part = [[m, extra] for m in sup_masks]
    mc, stc = run_slices_classes(model, vol, sup_imgs, per_part, zs, dev, batch=4)
    assert mc.shape == (6, 2, S, S) and mc.dtype == torch.uint8
    from protosam_amd.runner import part_assign
    # batches are cut at the z-parts (0-1, 2-3, 4-5): the same calls made directly give the same bits
    for z0 in (0, 2, 4):
        p = part_assign(z0, 6)
        q = vol[z0:z0 + 2][:, None].expand(2, 3, S, S).contiguous()
        res = model.forward_classes_batch(q, sup_imgs[p], per_part[p])
        for b in range(2):
            assert stc[z0 + b] == sum(1 for (bb, _) in model.last_stats["prompt"] if bb == b)
            for c in range(2):
                assert torch.equal(mc[z0 + b, c], res[b][c][0].to(torch.uint8)), (z0 + b, c)
    # and per-slice forward_classes (a 1-slice call runs other GEMM tiles: border pixels may flip)
    worst = 1.0
    for z in zs:
        p = part_assign(z, 6)
        q = vol[z][None, None].expand(1, 3, S, S).contiguous()
        r1 = model.forward_classes(q, sup_imgs[p], per_part[p])
        for c in range(2):
            ref = r1[c][0].to(torch.uint8)
            d = int((mc[z, c] != ref).sum())
            dc = _dice(mc[z, c].cpu(), ref.cpu()) if int(ref.sum()) else float(int(mc[z, c].sum()) == 0)
            worst = min(worst, dc)
            assert dc >= 0.995 and d <= 256, (z, c, d, dc)
    print(f"run_slices_classes vs per-slice forward_classes: worst Dice {worst:.5f}")
