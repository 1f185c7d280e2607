"""GPU: prompt sets of more than 16 tokens (more than 11 points or boxes) through the SAM mask decoder.

  1. psam_token_attention (token self-attention and image-to-token attention over 17 ... MAX_PROMPT_TOKENS keys) and the
     token-grouped psam_t2i_attention / psam_t2i_attention_split, each against float64 with the bounds DERIVED in
     tests/test_decoder_tokens_cpu.py from the kernels' summation order (that file shows the same checks refusing dropped, phantom
     and exchanged keys): random rows, selector rows, constant V, NaN guard rows after the last prompt set, refused arguments;
  2. MaskDecoder.predict_masks_tokens against oracle.sam_prompt_decoder.mask_decoder in float64, stage by stage;
  3. the callers that used to raise: SamPredictor.predict with 12 and 40 clicks, Sam.forward with a 20-point record,
     ProtoSAM.forward with twelve points, a box and negative points per component; and the cap at every layer.

The worst measured error of every case (what `_within` prints) is recorded in profiles/decoder_many_tokens_tests.txt.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_decoder_kernels_gpu import DECODER_BOUNDS, NAN, _attention_ref, _nan, _rand, _shape_rows, _within   # noqa: E402
from test_decoder_tokens_cpu import I2T_TK, SELF_T, T2I_NK, T2I_T, t2i_bound, token_bound                    # noqa: E402

GUARD = 3          # NaN rows after the last prompt set's K / V rows and after the last output row
LN2_24 = 24 * math.log(2.0)


def _guarded(x, dev, dtype=None):
    """x [rows, width] on the device with GUARD rows of NaN behind it (one allocation): (the view of the rows, the guard rows)"""
    buf = torch.full((x.shape[0] + GUARD, x.shape[1]), NAN, dtype=dtype or x.dtype, device=dev)
    buf[:x.shape[0]] = x.to(dev)
    return buf[:x.shape[0]], buf[x.shape[0]:]


def _out(rows, width, dev, dtype=torch.float32):
    buf = _nan((rows + GUARD, width), dev, dtype)
    return buf[:rows], buf[rows:]


def _run_token_attention(dev, q, kbuf, vbuf, B, Tq, Tk, NH, hd, width):
    """ops.token_attention with the decoder's strides: K / V the first `width` columns of 256-wide rows, q / out `width` wide;
    K, V and out carry NaN guard rows, which must stay NaN while the result is finite."""
    from protosam_amd import ops
    kd, kg = _guarded(kbuf, dev)
    vd, vg = _guarded(vbuf, dev)
    out, og = _out(B * Tq, width, dev, q.dtype)
    ops.token_attention(q.to(dev), kd[:, :width], vd[:, :width], out, B, Tq, Tk, NH, hd, width, 256, 256, width)
    assert bool(kg.isnan().all()) and bool(vg.isnan().all()) and bool(og.isnan().all()), "guard rows written"
    return out


def _selector_case(B, Tq, Tk, NH, hd, seed, pick=None):
    """(q, k, v, sel): the keys of every head at the same length, query row r a copy of key pick[r] (default r % Tk) scaled per head
    so that every other key's weight is below 2^-24 / Tk (scores s_j - s_i >= 24 ln 2 + ln Tk + 1): the output is v[pick[r]] (sel)."""
    W = NH * hd
    k = _rand((B, Tk, NH, hd), seed).double()
    k = k / k.norm(dim=-1, keepdim=True) * math.sqrt(hd)
    v = _rand((B * Tk, W), seed + 1)
    kh = k.permute(0, 2, 1, 3)                                                     # [B, NH, Tk, hd]
    j = torch.arange(Tq) % Tk if pick is None else pick
    kj = kh[:, :, j]                                                               # [B, NH, Tq, hd]
    dots = kj @ kh.transpose(-1, -2)                                               # [B, NH, Tq, Tk]
    dots.scatter_(-1, j.view(1, 1, Tq, 1).expand(B, NH, Tq, 1), -1e30)
    gap = hd - dots.amax(-1)                                                       # [B, NH, Tq] > 0: distinct directions
    assert bool((gap > 1e-3 * hd).all())
    scale = (LN2_24 + math.log(Tk) + 1.0) * math.sqrt(hd) / gap
    q = (scale[..., None] * kj).permute(0, 2, 1, 3).reshape(B * Tq, W).float()
    sel = v.view(B, Tk, W)[:, j].reshape(B * Tq, W).double()
    return q, k.reshape(B * Tk, W).float(), v, sel


# ---- 1a. token self-attention ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", SELF_T)
@pytest.mark.parametrize("B", [1, 3])
def test_token_attention_self(dev, B, T):
    """The two-way block's token self-attention past 16 tokens (transformer.py:218-240 at hd 32, fp32, Tq = Tk = T): random rows with
    dominant-key and all-zero queries (`_shape_rows`), selector rows for every key, and constant V, within token_bound(T, 32) -
    derived in test_decoder_tokens_cpu.py: 28.5 (T = 17) ... 63.5 (T = 256) x 2^-23 x magnitude. T spans one key past a chunk of 16,
    whole chunks, one past them, several workgroups per prompt set (T x 8 heads > 256 threads from T = 33) and the cap."""
    NH, hd, c = 8, 32, token_bound(T, 32)
    q, k, v = _rand((B * T, 256), 1), _rand((B * T, 256), 2), _rand((B * T, 256), 3)
    _shape_rows(q, k, B, T, T, 256, 1.0)
    ref, mag = _attention_ref(q.double(), k.double(), v.double(), B, T, T, NH, hd)
    out = _run_token_attention(dev, q, k, v, B, T, T, NH, hd, 256)
    _within(out, ref, mag, c, f"token_attention hd32 B={B} T={T}")
    # selector rows: query j picks key j
    qs, ks, vs, sel = _selector_case(B, T, T, NH, hd, 40 + T)
    ref, mag = _attention_ref(qs.double(), ks.double(), vs.double(), B, T, T, NH, hd)
    out = _run_token_attention(dev, qs, ks, vs, B, T, T, NH, hd, 256)
    _within(out, ref, mag, c, f"token_attention hd32 selectors B={B} T={T}")
    _within(out, sel, mag, c, f"token_attention hd32 selectors = v_j B={B} T={T}", floor=2.0 ** -24 * 2 * vs.abs().max().item())
    # constant V: the output is that row whatever the scores
    vc = _rand((1, 256), 5).expand(B * T, 256).contiguous()
    ref, mag = _attention_ref(q.double(), k.double(), vc.double(), B, T, T, NH, hd)
    assert float((ref - vc.double()).abs().max()) < 1e-14
    out = _run_token_attention(dev, q, k, vc, B, T, T, NH, hd, 256)
    _within(out, vc.double(), mag, c, f"token_attention hd32 constant V B={B} T={T}")


# ---- 1b. image-to-token attention -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tk", I2T_TK)
@pytest.mark.parametrize("Tq", [64, 4096])
@pytest.mark.parametrize("qdt", [torch.float32, torch.float16])
def test_token_attention_image_to_token(dev, Tq, Tk, qdt):
    """Image-to-token attention past 16 tokens (transformer.py:176-180): g^2 = 64 or 4096 image-token queries per prompt set over
    the Tk tokens, hd 16, the decoder's strides (q / out 128 wide, K / V the first 128 columns of 256-wide rows), q / out fp32 or
    fp16 (fp16 out: the fp32 result rounded once more, its half ulp allowed as a floor). Bound token_bound(Tk, 16): 20 ... 57."""
    B, NH, hd, c = 2, 8, 16, token_bound(Tk, 16)
    tag = f"hd16 {str(qdt)[6:]} Tq={Tq} Tk={Tk}"
    floor = (lambda r: 2.0 ** -11 * r.abs() + 2.0 ** -25) if qdt == torch.float16 else (lambda r: 0.0)
    q = _rand((B * Tq, 128), 11)
    kbuf, vbuf = _rand((B * Tk, 256), 12), _rand((B * Tk, 256), 13)
    k, v = kbuf[:, :128].contiguous(), vbuf[:, :128].contiguous()
    _shape_rows(q, k, B, Tq, Tk, 128, 1.5)
    qd = q.to(qdt)
    ref, mag = _attention_ref(qd.double(), k.double(), v.double(), B, Tq, Tk, NH, hd)
    out = _run_token_attention(dev, qd, kbuf, vbuf, B, Tq, Tk, NH, hd, 128)
    _within(out, ref, mag, c, f"token_attention {tag}", floor=floor(ref))
    # selector rows: image token r picks token r % Tk (every key where Tq >= Tk)
    qs, ks, vs, sel = _selector_case(B, Tq, Tk, NH, hd, 60 + Tk)
    qd = qs.to(qdt)
    kb, vb = _rand((B * Tk, 256), 14), _rand((B * Tk, 256), 15)
    kb[:, :128], vb[:, :128] = ks, vs
    ref, mag = _attention_ref(qd.double(), ks.double(), vs.double(), B, Tq, Tk, NH, hd)
    out = _run_token_attention(dev, qd, kb, vb, B, Tq, Tk, NH, hd, 128)
    _within(out, ref, mag, c, f"token_attention {tag} selectors", floor=floor(ref))
    _within(out, sel, mag, c, f"token_attention {tag} selectors = v_j", floor=floor(sel) + 2.0 ** -24 * 2 * vs.abs().max().item())
    # constant V
    vc = _rand((1, 256), 16).expand(B * Tk, 256).contiguous()
    want = vc[:1, :128].expand(B * Tq, 128).double()
    out = _run_token_attention(dev, q.to(qdt), kbuf, vc, B, Tq, Tk, NH, hd, 128)
    mag = _attention_ref(q.to(qdt).double(), k.double(), vc[:, :128].contiguous().double(), B, Tq, Tk, NH, hd)[1]
    _within(out, want, mag, c, f"token_attention {tag} constant V", floor=floor(want))


def test_token_attention_up_to_16_keys(dev):
    """One partial or whole chunk: psam_token_attention takes 1 ... 16 keys as well (the callers send those to psam_small_attention),
    within its own bound against float64."""
    for Tk in (1, 9, 16):
        B, NH, hd = 3, 8, 32
        q, k, v = (_rand((B * Tk, 256), s) for s in (31, 32, 33))
        ref, mag = _attention_ref(q.double(), k.double(), v.double(), B, Tk, Tk, NH, hd)
        out = _run_token_attention(dev, q, k, v, B, Tk, Tk, NH, hd, 256)
        _within(out, ref, mag, token_bound(Tk, hd), f"token_attention hd32 B={B} T={Tk}")


def test_token_attention_rejects_bad_arguments(dev):
    """No keys, more than MAX_PROMPT_TOKENS keys, hd 32 with fp16 q, a head size without a kernel, more than 8 heads, and K rows
    that are not 16-byte aligned are refused by the host before any launch: the output stays untouched."""
    from protosam_amd import ops
    cap = ops.MAX_PROMPT_TOKENS
    q = _rand((4, 256), 1).to(dev)
    k, v = _rand((cap + 2, 256), 2).to(dev), _rand((cap + 2, 256), 3).to(dev)
    cases = [(0, q, 8, 32, k, 256), (cap + 1, q, 8, 32, k, 256), (17, q.half(), 8, 32, k, 256), (17, q, 4, 64, k, 256),
             (17, q, 16, 16, k, 256), (17, q, 8, 32, k.view(-1)[1:1 + 17 * 256].view(17, 256), 256), (17, q, 8, 32, k, 258)]
    for Tk, qq, NH, hd, kk, ldk in cases:
        out = _nan((4, 256), dev, qq.dtype)
        with pytest.raises(RuntimeError, match="status 1"):
            ops.token_attention(qq, kk, v, out, 1, 4, Tk, NH, hd, 256, ldk, 256, 256)
        assert bool(out.isnan().all()), (Tk, NH, hd, ldk)
    out = _nan((4, 256), dev)                     # the cap itself runs
    ops.token_attention(q, k, v, out, 1, 4, cap, 8, 32, 256, 256, 256, 256)
    assert bool(torch.isfinite(out).all())


# ---- 1c. token-to-image attention ---------------------------------------------------------------------------------------------------
def _head_major(x, B, Nk):
    return x.view(B, Nk, 8, 16).permute(0, 2, 1, 3).contiguous().view(B * Nk, 128)


@pytest.mark.parametrize("kdt", [torch.float32, torch.float16])
@pytest.mark.parametrize("Nk", T2I_NK)
@pytest.mark.parametrize("T", T2I_T)
def test_t2i_attention_token_groups(dev, T, Nk, kdt):
    """Token-to-image attention past 16 tokens (transformer.py:163-167,98-103): 16 tokens (waves) per workgroup, ceil(T / 16) groups
    next to the key-split index in the grid. K / V fp32 or fp16, token-major and head-major, 1, 3 and 16 key ranges, against float64
    within t2i_bound(Nk, S) (derived in test_decoder_tokens_cpu.py: 186.5 unsplit at 4096 keys ... 29 at 64): random queries with a
    dominant key, selector queries (token t picks image key (37 t) % Nk) and constant V. NaN guard rows follow K, V, the output and
    the partial buffer; the split result is the same bits at every repeat."""
    from protosam_amd import ops
    B, NH, hd = 2, 8, 16
    q = _rand((B * T, 128), 81, 1.5)
    k, v = _rand((B * Nk, 128), 82), _rand((B * Nk, 128), 83)
    k[5] *= 6.0
    qs, ks, vs, sel = _selector_case(B, T, Nk, NH, hd, 90 + T, pick=torch.tensor([(37 * t) % Nk for t in range(T)]))
    vc = _rand((1, 128), 84).expand(B * Nk, 128).contiguous()
    cases = [("random", q, k, v, None), ("selectors", qs, ks, vs, sel), ("constant V", q, k, vc, vc[:1].expand(B * T, 128).double())]
    for name, qq, kk, vv, exact in cases:
        kq, vq = kk.to(kdt), vv.to(kdt)
        ref, mag = _attention_ref(qq.double(), kq.double(), vq.double(), B, T, Nk, NH, hd)
        if exact is not None and kdt == torch.float16:
            exact = None if name == "selectors" else vq[:1].double().expand(B * T, 128)     # (fp16 keys move the selectors' scores)
        for hm in (False, True):
            K, kg = _guarded(_head_major(kq, B, Nk) if hm else kq, dev)
            V, vg = _guarded(_head_major(vq, B, Nk) if hm else vq, dev)
            for S in (1, 3, 16):
                tag = f"t2i T={T} Nk={Nk} {str(kdt)[6:]} {'head' if hm else 'token'}-major S={S} {name}"
                part = _nan((B * NH * S * T * 18 + 18 * GUARD,), dev)
                outs = []
                for _ in range(2 if S > 1 else 1):
                    out, og = _out(B * T, 128, dev)
                    ops.t2i_attention(qq.to(dev), K, V, out, B, T, Nk, NH, head_major=hm, split=(S, part))
                    assert bool(og.isnan().all()) and bool(kg.isnan().all()) and bool(vg.isnan().all()), tag
                    outs.append(out)
                if S > 1:
                    assert bool(part[B * NH * S * T * 18:].isnan().all()), tag
                    assert torch.equal(outs[0], outs[1]), tag
                _within(outs[0], ref, mag, t2i_bound(Nk, S), tag)
                if exact is not None:
                    _within(outs[0], exact, mag, t2i_bound(Nk, S), tag + " = v", floor=2.0 ** -24 * 2 * vv.abs().max().item())


def test_t2i_attention_rejects_more_than_the_cap(dev):
    """psam_t2i_attention_split refuses T > MAX_PROMPT_TOKENS, S > 16 and a missing partial buffer; head-major K / V are refused past
    the cap as well (the one-workgroup-per-token kernel reads token-major rows only). The output stays untouched."""
    from protosam_amd import ops
    cap, Nk = ops.MAX_PROMPT_TOKENS, 64
    T = cap + 1
    q, k, v = _rand((T, 128), 1).to(dev), _rand((Nk, 128), 2).to(dev), _rand((Nk, 128), 3).to(dev)
    part = _nan((8 * 17 * T * 18,), dev)
    for kw in (dict(split=(2, part)), dict(head_major=True)):
        out = _nan((T, 128), dev)
        with pytest.raises(RuntimeError, match="status 1"):
            ops.t2i_attention(q, k, v, out, 1, T, Nk, 8, **kw)
        assert bool(out.isnan().all())
    out = _nan((cap, 128), dev)
    with pytest.raises(RuntimeError, match="status 1"):
        ops.t2i_attention(q[:cap], k, v, out, 1, cap, Nk, 8, split=(17, part))
    assert bool(out.isnan().all())


# ---- 2. the whole decoder against the oracle ---------------------------------------------------------------------------------------
DECODER_CASES = [(1, 17, 64), (2, 33, 64), (5, 20, 64), (2, 133, 64), (2, 17, 8)]       # (prompt sets, tokens, g: Nk = g^2)
N_IMG = 3
_DEC = {}


def _decoder(dev, g):
    """the decoder of test_decoder_sweep (synthetic weights, seed 1234) with three g x g embeddings"""
    if "md" not in _DEC:
        from protosam_amd.segment_anything.modeling.mask_decoder import MaskDecoder
        from protosam_amd.segment_anything.modeling.transformer import TwoWayTransformer
        from protosam_amd.synth import synth_state_dict
        md = MaskDecoder(transformer_dim=256, transformer=TwoWayTransformer(depth=2, embedding_dim=256, mlp_dim=2048, num_heads=8),
                         num_multimask_outputs=3, iou_head_depth=3, iou_head_hidden_dim=256)
        sd = synth_state_dict(md, 1234)
        md.load_state_dict(sd, strict=True)
        _DEC.update(md=md.to(dev).eval(), sd64={k: v.double() for k, v in sd.items()}, dense=_rand((256,), 113, 0.5))
    if ("grid", g) not in _DEC:
        from oracle import sam_prompt_decoder as odec
        y = ((torch.arange(g, dtype=torch.float32) + 0.5) / g)[:, None].expand(g, g)
        pe = odec.pe_encoding(torch.stack([y.t(), y], -1), _rand((2, 128), 111)).permute(2, 0, 1)[None].contiguous()
        _DEC[("grid", g)] = (_rand((N_IMG, 256, g, g), 112), pe)
    return _DEC


def _decoder_case(dev, B, T, g):
    """(sparse, img_of_prompt, float64 oracle taps) of B prompt sets of T tokens over N_IMG images, computed once per case"""
    from oracle import sam_prompt_decoder as odec
    D = _decoder(dev, g)
    if (B, T, g) not in _DEC:
        feats, pe = D[("grid", g)]
        sparse = _rand((B, T - 5, 256), 120 + B * 17 + T)
        iop = torch.tensor([(7 * i + 2) % N_IMG for i in range(B)], dtype=torch.int32)
        taps = {k: [None] * B for k in ("hs", "keys", "hyper", "masks_all", "iou_all")}
        for im in range(N_IMG):
            idx = [i for i in range(B) if int(iop[i]) == im]
            if not idx:
                continue
            t = {}
            dense = D["dense"].double().reshape(1, -1, 1, 1).expand(len(idx), -1, g, g)
            odec.mask_decoder(D["sd64"], feats[im:im + 1].double(), pe.double(), sparse[idx].double(), dense, True, pre="", taps=t)
            for k in taps:
                for j, i in enumerate(idx):
                    taps[k][i] = t[k][j]
        _DEC[(B, T, g)] = (sparse, iop, {k: torch.stack(v) for k, v in taps.items()})
    return _DEC[(B, T, g)]


@pytest.mark.parametrize("path", ["x3", "f32", "f16"])
@pytest.mark.parametrize("B,T,g", DECODER_CASES)
def test_decoder_sweep_many_tokens(dev, B, T, g, path):
    """MaskDecoder.predict_masks_tokens with 17 ... 133 tokens per prompt set (12 ... 128 sparse prompts) on three images, img_of_prompt
    not monotone, against oracle.mask_decoder in float64 stage by stage, as test_decoder_sweep does up to 16 tokens: the queries
    after the two-way transformer (hs), the keys, the hyper-network vectors, the low-res masks, and sigmoid(masks) / IoU absolute.
    The cases span token_attention with one and several chunks and workgroups, two to nine token groups of the token-to-image
    kernel with 16 ... 1 key ranges, head-major K / V (x3, f32) and token-major fp16 K / V (f16), and a 8 x 8 embedding (64 keys).
    Bounds: DECODER_BOUNDS of test_decoder_sweep unchanged (per stage relative to the stage's largest value; prob / iou 1e-3 at
    most); the measured worst per stage is in profiles/decoder_many_tokens_tests.txt."""
    D = _decoder(dev, g)
    md = D["md"]
    Nk = g * g
    sparse, iop, ref = _decoder_case(dev, B, T, g)
    feats, pe = D[("grid", g)]
    md.image_side_x3, md.image_side_fp16 = path == "x3", path == "f16"
    try:
        feat = feats.permute(0, 2, 3, 1).reshape(N_IMG, Nk, 256).contiguous().to(dev)
        pe_tok = pe[0].permute(1, 2, 0).reshape(Nk, 256).contiguous().to(dev)
        tokens = md.build_tokens(sparse.to(dev))
        assert tokens.shape == (B, T, 256)
        masks, iou = _nan((B, 4, 4 * g, 4 * g), dev), _nan((B, 4), dev)
        _, _, hs = md.predict_masks_tokens(feat, pe_tok, tokens, D["dense"].to(dev), img_of_prompt=iop.to(dev), masks_out=masks,
                                           iou_out=iou)
        keys = md.transformer._ws[(B, T, Nk, path == "f16")]["keys"]
        hyper = md._ws[(B, T, Nk)]["hyper"]
        got = dict(hs=hs, keys=keys.view(B, g, g, 256).permute(0, 3, 1, 2), hyper=hyper, masks=masks)
        want = dict(hs=ref["hs"], keys=ref["keys"], hyper=ref["hyper"], masks=ref["masks_all"])
        errs = {}
        for k in got:
            x = got[k].double().cpu()
            assert bool(torch.isfinite(x).all()), k
            errs[k] = (x - want[k]).abs().max().item() / want[k].abs().max().item()
        errs["prob"] = (torch.sigmoid(masks.double().cpu()) - torch.sigmoid(ref["masks_all"])).abs().max().item()
        assert bool(torch.isfinite(iou).all())
        errs["iou"] = (iou.double().cpu() - ref["iou_all"]).abs().max().item()
        print(f"decoder {path} B={B} T={T} Nk={Nk}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        bounds = DECODER_BOUNDS[path]
        for k, v in errs.items():
            assert v < bounds[k], (path, B, T, Nk, k, v, bounds[k])
    finally:
        md.image_side_x3, md.image_side_fp16 = True, False


# ---- 3. the callers ---------------------------------------------------------------------------------------------------------------
SIDE = 256         # a 256-pixel SAM: 16 x 16 embedding, 64 x 64 low-res masks


@pytest.fixture(scope="module")
def small_sam(dev):
    """ViT-B with one encoder block at a 256-pixel input, synthetic weights; the oracle's prompt encoder is written for the 1024-pixel
    model through two module constants, set to this model's for the module"""
    from oracle import sam_prompt_decoder as odec
    from protosam_amd.segment_anything import sam_model_registry
    from protosam_amd.synth import synth_state_dict
    sam = sam_model_registry["vit_b"](encoder_depth=1, image_size=SIDE)
    sd = synth_state_dict(sam, 1234)
    sam.load_state_dict(sd, strict=True)
    old = odec.IMG, odec.GRID
    odec.IMG, odec.GRID = SIDE, SIDE // 16
    yield sam.to(dev).eval(), {k: v.cpu().float() for k, v in sd.items()}
    odec.IMG, odec.GRID = old


def _small_image(seed):
    import scipy.ndimage as ndi
    rng = np.random.RandomState(seed)
    img = np.stack([ndi.gaussian_filter(rng.rand(SIDE, SIDE), 3 + c) for c in range(3)], -1)
    return ((img - img.min()) / (img.max() - img.min()) * 255).astype(np.uint8)


def _clicks(n, seed):
    rng = np.random.RandomState(seed)
    pts = np.round(rng.uniform(4, SIDE - 4, size=(n, 2)) * 4) / 4
    return pts, (np.arange(n) % 3 != 2).astype(np.int64)          # two positive clicks, one negative, ...


def _oracle_decode(sd, feats, pts, lab, box):
    from oracle import sam_prompt_decoder as odec
    pc = torch.as_tensor(pts, dtype=torch.float)
    pl = torch.as_tensor(lab, dtype=torch.int)
    if pc.dim() == 2:
        pc, pl = pc[None], pl[None]
    bx = None if box is None else torch.as_tensor(box, dtype=torch.float).reshape(-1, 4)
    sparse, dense = odec.prompt_encoder(sd, (pc, pl), bx)
    low, iou = odec.mask_decoder(sd, feats, odec.dense_pe(sd), sparse, dense, True)
    return sparse, low, iou


@pytest.mark.parametrize("with_box", [False, True])
@pytest.mark.parametrize("n", [12, 40])
def test_predictor_with_many_clicks(dev, small_sam, n, with_box):
    """SamPredictor.predict with 12 and 40 clicks of mixed labels, with and without a box (18 ... 47 tokens per prompt set; up to ten
    clicks ran before), against the oracle's prompt encoder + mask decoder on the predictor's own features: sigmoid(low_res) and
    IoU within the project's 1e-3, masks equal up to sign flips of near-zero logits."""
    from oracle import sam_prompt_decoder as odec
    from protosam_amd.segment_anything import SamPredictor
    sam, sd = small_sam
    pred = SamPredictor(sam)
    pred.set_image(_small_image(n))
    pts, lab = _clicks(n, n)
    box = np.array([30.0, 40.0, 200.0, 220.0]) if with_box else None
    masks, iou, low = pred.predict(point_coords=pts, point_labels=lab, box=box, multimask_output=True)
    feats = pred.features.float().cpu().contiguous()
    assert feats.shape == (1, 256, SIDE // 16, SIDE // 16)
    sparse, low_r, iou_r = _oracle_decode(sd, feats, pts, lab, box)
    assert sparse.shape[1] == n + (2 if with_box else 1) and low.shape == (3, SIDE // 4, SIDE // 4) == tuple(low_r.shape[1:])
    perr = (torch.sigmoid(torch.from_numpy(low)) - torch.sigmoid(low_r[0])).abs().max().item()
    ierr = np.abs(iou - iou_r[0].numpy()).max()
    m_r = (odec.postprocess_masks(low_r, (SIDE, SIDE), (SIDE, SIDE), sam.postprocess_variant) > 0)[0].numpy()
    flips = (masks != m_r).mean()
    print(f"predict {n} clicks box={with_box}: {sparse.shape[1] + 5} tokens, max |dprob(low_res)| {perr:.2e}, |diou| {ierr:.2e}, "
          f"flipped {flips:.2e}")
    assert masks.shape == (3, SIDE, SIDE) and masks.dtype == np.bool_
    assert perr < 1e-3 and ierr < 1e-3 and flips < 1e-3


def test_sam_forward_with_a_20_point_record(dev, small_sam):
    """Sam.forward (sam.py:54-131) with a record of two prompt sets of 20 points each (26 tokens) and one of 3 points, against the
    oracle on the model's own embedding."""
    sam, sd = small_sam
    img = torch.from_numpy(_small_image(7)).permute(2, 0, 1).contiguous().to(dev)
    p20 = np.stack([_clicks(20, 1)[0], _clicks(20, 2)[0]])
    l20 = np.stack([_clicks(20, 1)[1], _clicks(20, 2)[1]])
    recs = [dict(image=img, original_size=(SIDE, SIDE), image_size=(SIDE, SIDE),
                 point_coords=torch.as_tensor(p, dtype=torch.float32, device=dev), point_labels=torch.as_tensor(l, device=dev))
            for p, l in ((p20, l20), (p20[:1, :3], l20[:1, :3]))]
    outs = sam(recs, multimask_output=True)
    feats = sam.image_encoder(sam.preprocess(img[None])).float().cpu().contiguous()
    for (p, l), o in zip(((p20, l20), (p20[:1, :3], l20[:1, :3])), outs):
        _, low_r, iou_r = _oracle_decode(sd, feats, p, l, None)
        perr = (torch.sigmoid(o["low_res_logits"].cpu()) - torch.sigmoid(low_r)).abs().max().item()
        ierr = (o["iou_predictions"].cpu() - iou_r).abs().max().item()
        print(f"Sam.forward {p.shape[1]} points x {p.shape[0]} sets: max |dprob(low_res)| {perr:.2e}, |diou| {ierr:.2e}")
        assert o["masks"].shape == (p.shape[0], 3, SIDE, SIDE) and o["masks"].dtype == torch.bool
        assert perr < 1e-3 and ierr < 1e-3


def test_protosam_with_twelve_points_box_and_negative_points(dev, monkeypatch):
    """ProtoSAM.forward with num_points_for_sam = 12, use_bbox and use_neg_points: per component 12 most confident pixels + the
    centroid, up to two negative points and the box = 17 sparse tokens, 22 with the output tokens (it raised "more than 11 sparse
    prompt tokens" before). Against oracle.glue.protosam_forward on the same given coarse logits, with the Dice, probability and
    score bounds of the ProtoSAM-vs-oracle tests (test_protosam_gpu._forward_vs_oracle)."""
    from oracle import glue, sam_prompt_decoder as odec
    from protosam_amd import synth_cases as gi
    from protosam_amd.protosam import InputFactory, ProtoSAM, TYPE_ALPNET
    monkeypatch.setattr(odec, "IMG", 1024)          # (the module's small_sam fixture holds the 256-pixel model's values)
    monkeypatch.setattr(odec, "GRID", 64)
    from protosam_amd.synth import synth_state_dict
    from test_protosam_gpu import _dice
    from test_reference_records_gpu import FixedCoarse
    logits = gi.orch_coarse_logits()
    kw = dict(use_bbox=True, use_points=True, point_mode="both", use_cca=False, use_neg_points=True)
    model = ProtoSAM((1024, 1024), FixedCoarse(logits.to(dev)), f"random:vit_b:{gi.ORCH_SAM_SEED}:{gi.ORCH_SAM_DEPTH}",
                     num_points_for_sam=12, use_sam_trans=True, **kw).to(dev).eval()
    q = gi.orch_query()
    inp = InputFactory.create_input(TYPE_ALPNET, q.to(dev), support_images=[q.to(dev)], support_labels=[torch.zeros(1, 512, 512)],
                                    isval=True, val_wsize=2)
    pred, scores = model(q.to(dev), inp, degrees_rotate=0)
    st = model.last_stats
    sam_sd = {k: v.cpu() for k, v in synth_state_dict(model.sam, gi.ORCH_SAM_SEED).items()}
    taps = {}
    pred_ref, scores_ref = glue.protosam_forward(q, logits, sam_sd, "vit_b", encoder_depth=gi.ORCH_SAM_DEPTH, taps=taps,
                                                 postprocess=model.sam.postprocess_variant, num_points=12, **kw)
    coords, labels = st["prompts"]
    assert len(scores) == len(scores_ref) == len(coords) and max(len(l) for l in labels) >= 12 + 1 + 1 + 2
    low = st["low_res"][:, st["sel"]].cpu()
    low_ref = torch.stack([l[0] for l in taps["low_res"]])
    perr = (torch.sigmoid(low) - torch.sigmoid(low_ref)).abs().max().item()
    d = _dice(pred.cpu(), pred_ref)
    serr = np.abs(np.array(scores, dtype=np.float64) - np.array(scores_ref)).max()
    print(f"ProtoSAM 12 points + box + negatives: {len(coords)} prompt sets of {sorted(set(len(l) + 5 for l in labels))} tokens, "
          f"max |dprob(low_res)| {perr:.2e}, Dice {d:.5f}, scores {serr:.2e}")
    assert d >= 0.999 and perr < 1e-3 and serr < 1e-3


def test_cap_is_refused_at_every_layer(dev, small_sam):
    """MAX_PROMPT_TOKENS + 1 tokens per prompt set: NotImplementedError with the number from MaskDecoder.predict_masks_tokens,
    TwoWayTransformer (forward and run_tokens), TwoWayAttentionBlock.forward, MaskDecoder.forward, SamPredictor.predict_torch and
    Sam.forward; Attention.forward keeps refusing what has no kernel. The cap itself decodes."""
    from protosam_amd import ops
    from protosam_amd.segment_anything import SamPredictor
    sam, _ = small_sam
    cap, g = ops.MAX_PROMPT_TOKENS, SIDE // 16
    md, tr = sam.mask_decoder, sam.mask_decoder.transformer
    z = lambda *s: torch.zeros(s, device=dev)  # noqa: E731
    match = str(cap)
    with pytest.raises(NotImplementedError, match=match):
        md.predict_masks_tokens(z(g * g, 256), z(g * g, 256), z(1, cap + 1, 256), z(256))
    with pytest.raises(NotImplementedError, match=match):
        tr.run_tokens(z(g * g, 256), z(g * g, 256), z(1, cap + 1, 256), z(256))
    with pytest.raises(NotImplementedError, match=match):
        tr(z(1, 256, g, g), z(1, 256, g, g), z(1, cap + 1, 256))
    with pytest.raises(NotImplementedError, match=match):
        tr.layers[0](z(1, cap + 1, 256), z(1, g * g, 256), z(1, cap + 1, 256), z(1, g * g, 256))
    with pytest.raises(NotImplementedError, match=match):
        md(image_embeddings=z(1, 256, g, g), image_pe=z(1, 256, g, g), sparse_prompt_embeddings=z(1, cap - 4, 256),
           dense_prompt_embeddings=z(1, 256, 1, 1).expand(1, 256, g, g), multimask_output=True)
    n = cap - 5                                            # n points + the padding point = cap - 4 sparse tokens: cap + 1 tokens
    pts = torch.rand((1, n, 2), device=dev) * SIDE
    lab = torch.ones((1, n), dtype=torch.int64, device=dev)
    pred = SamPredictor(sam)
    pred.set_image(_small_image(3))
    with pytest.raises(NotImplementedError, match=match):
        pred.predict_torch(pts, lab)
    img = torch.from_numpy(_small_image(3)).permute(2, 0, 1).contiguous().to(dev)
    with pytest.raises(NotImplementedError, match=match):
        sam([dict(image=img, original_size=(SIDE, SIDE), image_size=(SIDE, SIDE), point_coords=pts, point_labels=lab)], True)
    masks, iou, low = pred.predict_torch(pts[:, :n - 1], lab[:, :n - 1])          # cap tokens
    assert bool(torch.isfinite(low).all()) and bool(torch.isfinite(iou).all())
    attn = tr.layers[0].self_attn
    with pytest.raises(NotImplementedError, match="no HIP kernel"):
        attn(z(1, cap + 1, 256), z(1, cap + 1, 256), z(1, cap + 1, 256))          # 32-wide heads over more than `cap` keys
    out = attn(torch.randn((2, 40, 256), device=dev), torch.randn((2, 40, 256), device=dev), torch.randn((2, 40, 256), device=dev))
    assert out.shape == (2, 40, 256) and bool(torch.isfinite(out).all())
