"""GPU parity of the SAM prompt-encoder and mask-decoder kernels (csrc/decoder.hip), one kernel at a time, against float64
restatements of the same operations, and of the whole decoder (`MaskDecoder.predict_masks_tokens`) against the oracle in float64.

Every output buffer is filled with NaN before the call, so an element a kernel leaves unwritten fails. Error bounds follow the
operation's arithmetic: a small multiple of 2^-23 times the sum of the magnitudes of the terms that make up each output (first-order
propagation through softmax, LayerNorm and GELU), not a flat tolerance. Bounds that could only be set by measurement (the whole
decoder) carry the measured figure in their docstring.
"""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -23          # fp32 unit in the last place at 1.0
NAN = float("nan")
GELU_SLOPE = 1.13       # max |d gelu(x) / dx|: how far an input error can grow through the erf GELU


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def _within(out, ref, mag, c, what, floor=0.0):
    """|out - ref| <= c 2^-23 mag (+ floor) element-wise; returns the worst |out - ref| / (2^-23 mag) for the report."""
    out = out.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(out).all()), f"{what}: {int((~torch.isfinite(out)).sum())} non-finite (unwritten?) elements"
    err = (out - ref).abs()
    worst = ((err - floor).clamp_min(0) / mag.clamp_min(1e-300)).max().item() / U
    bad = err > c * U * mag + floor
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements off by more than {c} x 2^-23 x magnitude (worst {worst:.2f})"
    print(f"{what}: worst |err| = {worst:.2f} x 2^-23 x magnitude (bound {c})")
    return worst


# ---- float64 references with their error magnitudes -------------------------------------------------------------------
def _attention_ref(q, k, v, B, Tq, Tk, NH, hd):
    """softmax(q k^T / sqrt(hd)) v per (batch, head): q [B*Tq, NH*hd], k / v [B*Tk, NH*hd] (float64) -> (out, magnitude).
    magnitude: |dout| <= sum_j p_j |v_j - out| |ds_j| + the rounding of the weighted sums, |ds_j| ~ u sum_d |q_d k_jd| / sqrt(hd)."""
    qh = q.view(B, Tq, NH, hd).permute(0, 2, 1, 3)
    kh = k.view(B, Tk, NH, hd).permute(0, 2, 1, 3)
    vh = v.view(B, Tk, NH, hd).permute(0, 2, 1, 3)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(hd)
    smag = qh.abs() @ kh.abs().transpose(-1, -2) / math.sqrt(hd)
    p = torch.softmax(s, -1)
    o = p @ vh
    ps = p * (1.0 + smag)
    mag = p @ vh.abs() + ps @ vh.abs() + o.abs() * ps.sum(-1, keepdim=True)
    flat = lambda x: x.permute(0, 2, 1, 3).reshape(B * Tq, NH * hd)  # noqa: E731
    return flat(o), flat(mag)


def _ln2d_mag(x, xmag, w, b, eps):
    """LayerNorm over dim 1 of NCHW (oracle _ln2d) and the magnitude of its output error given input errors of scale xmag:
    the mean's rounding, x - mean, and the relative error of 1 / sqrt(var + eps)."""
    mu = x.mean(1, keepdim=True)
    d = x - mu
    r = (d.pow(2).mean(1, keepdim=True) + eps).rsqrt()
    A = xmag + xmag.mean(1, keepdim=True)
    wa, ba = w.abs()[:, None, None], b.abs()[:, None, None]
    y = w[:, None, None] * d * r + b[:, None, None]
    return y, wa * r * A + wa * d.abs() * r.pow(3) * (d.abs() * A).mean(1, keepdim=True) + ba + y.abs()


# ---- 1. small_attention ------------------------------------------------------------------------------------------------
def _shape_rows(q, k, B, Tq, Tk, width, dominant=3.0):
    """Every third query row a scaled copy of one key (one dominant key: p ~ 1), every fifth all zeros (equal scores)."""
    qv, kv = q.view(B, Tq, width), k.view(B, Tk, width)
    for r in range(Tq):
        if r % 3 == 1:
            qv[:, r] = dominant * kv[:, r % Tk]
        elif r % 5 == 2:
            qv[:, r] = 0.0


@pytest.mark.parametrize("Tk", [1, 2, 5, 11, 16])
@pytest.mark.parametrize("B", [1, 3, 33])
def test_small_attention_token_self_attention(dev, B, Tk):
    """The two-way block's token self-attention (transformer.py:218-240 at hd 32, fp32): Tq = Tk tokens per prompt set, 8 heads."""
    from protosam_amd import ops
    NH, hd, T = 8, 32, Tk
    q, k, v = _rand((B * T, 256), 1), _rand((B * T, 256), 2), _rand((B * T, 256), 3)
    _shape_rows(q, k, B, T, T, 256, 1.0)
    ref, mag = _attention_ref(q.double(), k.double(), v.double(), B, T, T, NH, hd)
    out = _nan((B * T, 256), dev)
    ops.small_attention(q.to(dev), k.to(dev), v.to(dev), out, B, T, T, NH, hd, 256, 256, 256, 256)
    _within(out, ref, mag, 8, f"small_attention hd32 B={B} T={T}")


@pytest.mark.parametrize("Tk", [7, 16])
@pytest.mark.parametrize("qdt", [torch.float32, torch.float16])
def test_small_attention_image_to_token(dev, Tk, qdt):
    """Image-to-token attention (transformer.py:176-180): 4096 image-token queries per prompt set over the T tokens, hd 16, with the
    strides the decoder passes - q [B*4096,128] (ldq 128), K / V the first 128 columns of [B*T,256] buffers (ldk = ldv = 256),
    out ldo 128 - and q / out in fp32 (the default image side) or fp16. fp16 out: the fp32 result rounded once more."""
    from protosam_amd import ops
    B, Tq, NH, hd = 2, 4096, 8, 16
    q = _rand((B * Tq, 128), 11)
    kbuf, vbuf = _rand((B * Tk, 256), 12), _rand((B * Tk, 256), 13)
    k, v = kbuf[:, :128].contiguous(), vbuf[:, :128].contiguous()
    _shape_rows(q, k, B, Tq, Tk, 128, 1.5)
    qd = q.to(qdt)
    ref, mag = _attention_ref(qd.double(), k.double(), v.double(), B, Tq, Tk, NH, hd)
    out = _nan((B * Tq, 128), dev, qdt)
    kd, vd = kbuf.to(dev), vbuf.to(dev)
    ops.small_attention(qd.to(dev), kd[:, :128], vd[:, :128], out, B, Tq, Tk, NH, hd, 128, 256, 256, 128)
    if qdt == torch.float16:   # half ulp of the fp16 output, normal or subnormal
        _within(out, ref, mag, 8, f"small_attention hd16 fp16 T={Tk}", floor=2.0 ** -11 * ref.abs() + 2.0 ** -25)
    else:
        _within(out, ref, mag, 8, f"small_attention hd16 fp32 T={Tk}")


def test_small_attention_rejects_bad_shapes(dev):
    """No keys, more than 16 keys and hd 32 with fp16 q are refused by the host before any launch (the output stays untouched)."""
    from protosam_amd import ops
    q, k, v = _rand((4, 256), 1).to(dev), _rand((17, 256), 2).to(dev), _rand((17, 256), 3).to(dev)
    for Tk, qq in ((0, q), (17, q), (4, q.half())):
        out = _nan((4, 256), dev, qq.dtype)
        with pytest.raises(RuntimeError, match="status 1"):
            ops.small_attention(qq, k, v, out, 1, 4, Tk, 8, 32, 256, 256, 256, 256)
        assert bool(out.isnan().all())


# ---- 2. small_linear_splitk --------------------------------------------------------------------------------------------
def _linear_ref(x, W, b, resid):
    ref = x @ W.t() + b
    mag = x.abs() @ W.abs().t() + b.abs()
    if resid is not None:
        ref, mag = ref + resid, mag + resid.abs()
    return ref, mag


@pytest.mark.parametrize("M", [32, 33, 63, 243, 528])
@pytest.mark.parametrize("ks", [8, 4])
@pytest.mark.parametrize("with_resid", [True, False])
def test_small_linear_splitk(dev, M, ks, with_resid):
    """The two-way block's MLP output (transformer.py:170-171, 2048 -> 256 over B*T >= 32 token rows): ks K ranges as the groups of
    one MFMA launch into caller-owned planes, then a fixed-order sum with bias (+ residual). Bit-identical over repeated calls."""
    from protosam_amd import ops
    K, N = 2048, 256
    x, W, b = _rand((M, K), 21), _rand((N, K), 22, K ** -0.5), _rand((N,), 23, 0.1)
    resid = _rand((M, N), 24) if with_resid else None
    ref, mag = _linear_ref(x.double(), W.double(), b.double(), None if resid is None else resid.double())
    xd, Wd, bd, rd = x.to(dev), W.to(dev), b.to(dev), None if resid is None else resid.to(dev)
    outs = []
    for _ in range(3):
        parts = _nan((ks, M, N), dev)
        out = _nan((M, N), dev)
        ops.small_linear_splitk(xd, Wd, bd, rd, out, parts, ks)
        outs.append(out)
    _within(outs[0], ref, mag, 8, f"small_linear_splitk M={M} ks={ks} resid={with_resid}")
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


@pytest.mark.parametrize("form", ["parts_offset", "x_offset", "n70"])
def test_small_linear_splitk_element_wise_loads(dev, form):
    """The element-wise (non-VEC) form: `parts` or `x` one float into a larger allocation (not 16-byte aligned, in bounds), or
    N = 70 (planes of M * N % 4 != 0 floats)."""
    from protosam_amd import ops
    K, ks = 2048, 8
    M, N = (33, 70) if form == "n70" else (63, 256)
    x, W, b, resid = _rand((M, K), 31), _rand((N, K), 32, K ** -0.5), _rand((N,), 33, 0.1), _rand((M, N), 34)
    ref, mag = _linear_ref(x.double(), W.double(), b.double(), resid.double())
    if form == "x_offset":
        xb = _nan((M * K + 1,), dev)
        xb[1:] = x.reshape(-1).to(dev)
        xd = xb[1:].view(M, K)
    else:
        xd = x.to(dev)
    pb = _nan((ks * M * N + 1,), dev)
    parts = pb[1:] if form == "parts_offset" else pb[:-1]
    out = _nan((M, N), dev)
    ops.small_linear_splitk(xd, W.to(dev), b.to(dev), resid.to(dev), out, parts, ks)
    _within(out, ref, mag, 8, f"small_linear_splitk element-wise ({form})")


def test_small_linear_splitk_rejects_bad_ranges(dev):
    """K not a multiple of 64 ks, and fewer than two ranges, are refused by the host before any launch."""
    from protosam_amd import ops
    x, W, b = _rand((40, 2048), 1).to(dev), _rand((256, 2048), 2).to(dev), _rand((256,), 3).to(dev)
    parts = _nan((16 * 40 * 256,), dev)
    x2, W2 = _rand((40, 1984), 1).to(dev), _rand((256, 1984), 2).to(dev)
    for xx, WW, ks in ((x, W, 3), (x2, W2, 8), (x, W, 1), (x, W, 0)):
        out = _nan((40, 256), dev)
        with pytest.raises(RuntimeError, match="status 1"):
            ops.small_linear_splitk(xx, WW, b, None, out, parts, ks)
        assert bool(out.isnan().all()) and bool(parts.isnan().all())


# ---- 3. ln_pe ----------------------------------------------------------------------------------------------------------
def _ln_rows_ref(v, vmag, w, b, eps):
    """row LayerNorm of v [M,256] (float64) and its error magnitude (as _ln2d_mag on rows)."""
    y, ym = _ln2d_mag(v.t()[None, :, :, None], vmag.t()[None, :, :, None], w, b, eps)
    return y[0, :, :, 0].t(), ym[0, :, :, 0].t()


def _ln_pe_input(n_rows, seed):
    x = _rand((n_rows, 256), seed, 1.5) + 0.3
    x[1::7] = 100.0 + 0.01 * _rand((len(range(1, n_rows, 7)), 256), seed + 1)   # large mean, small spread
    x[3::11] *= 1e-3
    return x


@pytest.mark.parametrize("do_ln", [True, False])
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_ln_pe_images_of_prompts(dev, do_ln, eps):
    """`src = image_embeddings + dense` (mask_decoder.py:126-127) and `keys + key_pe` for the prompt sets of several images:
    in_mod = 4096 with img_of_prompt mapping 5 prompt sets onto 3 images out of order and repeated, add_vec, pe_mod; the fp16
    outputs are .half() of the fp32 result (y16) and of result + pe (ype16), bit for bit."""
    from protosam_amd import ops
    n_img, Nk, P = 3, 4096, 5
    iop = torch.tensor([2, 0, 2, 1, 0], dtype=torch.int32)
    x = _ln_pe_input(n_img * Nk, 41)
    add = _rand((256,), 42, 0.5)
    pe = _rand((Nk, 256), 43)
    w, b = 1.0 + _rand((256,), 44, 0.1), _rand((256,), 45, 0.1)
    xs = x.view(n_img, Nk, 256)[iop.long()].reshape(P * Nk, 256).double()
    v = xs + add.double()
    vmag = xs.abs() + add.double().abs()
    M = P * Nk
    y32, y16, ype16 = _nan((M, 256), dev), _nan((M, 256), dev, torch.float16), _nan((M, 256), dev, torch.float16)
    ops.ln_pe(x.to(dev), pe.to(dev), M, y32=y32, y16=y16, ype16=ype16, add_vec=add.to(dev), w=w.to(dev) if do_ln else None,
              b=b.to(dev) if do_ln else None, in_mod=Nk, pe_mod=Nk, eps=eps, img_of_prompt=iop.to(dev))
    if do_ln:
        ref, mag = _ln_rows_ref(v, vmag, w.double(), b.double(), eps)
        _within(y32, ref, mag, 8, f"ln_pe in_mod eps={eps}")
    else:   # one fp32 addition
        assert torch.equal(y32, (x.view(n_img, Nk, 256)[iop.long()].reshape(M, 256) + add).to(dev))
    assert torch.equal(y16, y32.half())
    assert torch.equal(ype16, (y32 + pe.to(dev).repeat(P, 1)).half())


def test_ln_pe_in_place_norm4(dev):
    """norm4 of the two-way block (transformer.py:180): the keys LayerNormed in place (y32 is x), their fp16 copy and fp16
    keys + pe with pe_mod = 4096 over 2 prompt sets; and a plain row op with a short pe_mod."""
    from protosam_amd import ops
    M, Nk = 2 * 4096, 4096
    x = _ln_pe_input(M, 51)
    pe = _rand((Nk, 256), 52)
    w, b = 1.0 + _rand((256,), 53, 0.1), _rand((256,), 54, 0.1)
    ref, mag = _ln_rows_ref(x.double(), x.double().abs(), w.double(), b.double(), 1e-5)
    keys = x.to(dev)
    y16, ype16 = _nan((M, 256), dev, torch.float16), _nan((M, 256), dev, torch.float16)
    ops.ln_pe(keys, pe.to(dev), M, y32=keys, y16=y16, ype16=ype16, w=w.to(dev), b=b.to(dev), pe_mod=Nk, eps=1e-5)
    _within(keys, ref, mag, 8, "ln_pe in place")
    assert torch.equal(y16, keys.half())
    assert torch.equal(ype16, (keys + pe.to(dev).repeat(2, 1)).half())
    # no LayerNorm, no in_mod, pe_mod 3: y32 = x exactly, ype16 = half(x + pe[row % 3])
    M2 = 37
    x2, pe2 = _rand((M2, 256), 55), _rand((3, 256), 56)
    y32, ype = _nan((M2, 256), dev), _nan((M2, 256), dev, torch.float16)
    ops.ln_pe(x2.to(dev), pe2.to(dev), M2, y32=y32, ype16=ype, pe_mod=3)
    assert torch.equal(y32, x2.to(dev))
    assert torch.equal(ype, (x2 + pe2[torch.arange(M2) % 3]).half().to(dev))


# ---- 4. prompt_tokens and dense_pe -------------------------------------------------------------------------------------
def _prompt_encoder(dev, seed=1234):
    from protosam_amd.segment_anything.modeling.prompt_encoder import PromptEncoder
    from protosam_amd.synth import synth_state_dict
    pe = PromptEncoder(embed_dim=256, image_embedding_size=(64, 64), input_image_size=(1024, 1024), mask_in_chans=16)
    sd = synth_state_dict(pe, seed)
    pe.load_state_dict(sd, strict=True)
    return pe.to(dev).eval(), sd


def _pe_ref(c01, G):
    """oracle pe_encoding in float64 and the magnitude of the fp32 error of its argument 2 pi ((2c - 1) @ G)."""
    from oracle import sam_prompt_decoder as odec
    ref = odec.pe_encoding(c01, G)
    arg = 2 * math.pi * ((2 * c01 - 1).abs() @ G.abs() + 2 * G.abs().sum(0))
    return ref, torch.cat([arg, arg], -1) + 1.0


@pytest.mark.parametrize("img_size", [1024, 512])
@pytest.mark.parametrize("Ns", [7, 0])
def test_prompt_tokens(dev, img_size, Ns):
    """Sparse prompt tokens (prompt_encoder.py:73-101, 186-214): tokens[b, :5] = the output tokens, tokens[b, 5 + j] =
    PE((coords + 0.5) / img_size) + the type embedding of label + 1; label -1 (not a point) has no PE. Labels -1 .. 3 mixed in one
    batch, coordinates at 0 and at the far edge."""
    from protosam_amd import ops
    pem, sd = _prompt_encoder(dev)
    pk = pem._packed()
    G = sd["pe_layer.positional_encoding_gaussian_matrix"].double()
    type_emb = pk["type_emb"].double().cpu()
    B = 4
    out_tok = _rand((5, 256), 61)
    labels = torch.tensor([[-1, 0, 1, 2, 3, 1, 0], [3, 2, 1, 0, -1, -1, 1], [1, 1, 1, 1, 1, 1, 1], [2, 3, 0, -1, 0, 2, 3]],
                          dtype=torch.int32)[:, :Ns].contiguous()
    coords = torch.rand((B, Ns, 2), generator=torch.Generator().manual_seed(62)) * img_size
    if Ns:
        coords[0, 1:3] = 0.0
        coords[1, 0:2] = img_size - 1.0
        coords[2, 3] = torch.tensor([0.0, img_size - 1.0])
    tok = _nan((B, 5 + Ns, 256), dev)
    ops.prompt_tokens(coords.to(dev), labels.to(dev), pk["G"], pk["type_emb"], out_tok.to(dev), B, Ns, img_size, tokens=tok)
    assert torch.equal(tok[:, :5].cpu(), out_tok.expand(B, -1, -1))
    if Ns == 0:
        return
    pe, mag = _pe_ref((coords.double() + 0.5) / img_size, G)
    lab = labels.long()
    pe[lab < 0] = 0.0
    mag[lab < 0] = 0.0
    ref = pe + type_emb[lab + 1]
    _within(tok[:, 5:], ref, mag + type_emb[lab + 1].abs(), 8, f"prompt_tokens img={img_size}")


@pytest.mark.parametrize("gh,gw", [(64, 64), (48, 80)])
def test_dense_pe(dev, gh, gw):
    """The dense positional grid (prompt_encoder.py:62-71,195-206), token-major [gh*gw, 256], square and not."""
    from protosam_amd import ops
    pem, sd = _prompt_encoder(dev)
    G = sd["pe_layer.positional_encoding_gaussian_matrix"].double()
    y = ((torch.arange(gh, dtype=torch.float64) + 0.5) / gh)[:, None].expand(gh, gw)
    x = ((torch.arange(gw, dtype=torch.float64) + 0.5) / gw)[None, :].expand(gh, gw)
    ref, mag = _pe_ref(torch.stack([x, y], -1).reshape(gh * gw, 2), G)
    _within(ops.dense_pe(pem._packed()["G"], gh, gw), ref, mag, 8, f"dense_pe {gh}x{gw}")


# ---- 5. upscale_tail ---------------------------------------------------------------------------------------------------
def _upscale_case(B, g, seed):
    u1 = _rand((B * g * g, 256), seed)
    u1[5::9, 64:128] *= 1e-3         # mid pixels whose 64 channels spread about as little as eps (1e-6): eps matters
    u1[2::13, 192:] = 0.7 + 1e-3 * u1[2::13, 192:]
    lnw, lnb = 1.0 + _rand((64,), seed + 1, 0.1), _rand((64,), seed + 2, 0.1)
    W2, b2 = _rand((64, 32, 2, 2), seed + 3, 0.125), _rand((32,), seed + 4, 0.1)
    hyper = _rand((B, 4, 32), seed + 5)
    return u1, lnw, lnb, W2, b2, hyper


def _upscale_ref(u1, lnw, lnb, W2, b2, hyper, B, g):
    """mask_decoder.py:137-144 after ConvT #1 in float64: u1 [B*g*g, (dy*2+dx)*64 + c] -> mid [B,64,2g,2g] -> LayerNorm2d(eps 1e-6)
    -> GELU -> ConvT(64->32, 2, 2) -> GELU -> hyper-network dot -> masks [B,4,4g,4g]; with the error magnitude of each stage."""
    from oracle import sam_prompt_decoder as odec
    mid = u1.view(B, g, g, 2, 2, 64).permute(0, 5, 1, 3, 2, 4).reshape(B, 64, 2 * g, 2 * g)
    ln = odec._ln2d(mid, lnw, lnb, 1e-6)
    _, lnm = _ln2d_mag(mid, mid.abs(), lnw, lnb, 1e-6)
    up = F.gelu(F.conv_transpose2d(F.gelu(ln), W2, b2, stride=2))
    upm = GELU_SLOPE * F.conv_transpose2d(GELU_SLOPE * lnm, W2.abs(), b2.abs(), stride=2) + up.abs()
    masks = (hyper @ up.view(B, 32, -1)).view(B, 4, 4 * g, 4 * g)
    mag = (hyper.abs() @ upm.view(B, 32, -1)).view(B, 4, 4 * g, 4 * g)
    return masks, mag


@pytest.mark.parametrize("B,g", [(1, 64), (3, 64), (3, 16)])
def test_upscale_tail(dev, B, g):
    """LayerNorm2d -> GELU -> ConvT(64->32) on the fp32 MFMA -> GELU -> hyper-network dot (psam_upscale_tail) with the packed
    ConvT weight of mask_decoder.py:79 ([c, (dy2*2+dx2)*32 + c2]), against float64."""
    from protosam_amd import ops
    u1, lnw, lnb, W2, b2, hyper = _upscale_case(B, g, 70 + B + g)
    ref, mag = _upscale_ref(*(t.double() for t in (u1, lnw, lnb, W2, b2, hyper)), B, g)
    W2r = W2.permute(0, 2, 3, 1).reshape(64, 4 * 32).contiguous()
    masks = _nan((B, 4, 4 * g, 4 * g), dev)
    ops.upscale_tail(u1.to(dev), lnw.to(dev), lnb.to(dev), W2r.to(dev), b2.to(dev), hyper.to(dev), B, g, masks=masks)
    _within(masks, ref, mag, 8, f"upscale_tail B={B} g={g}")


def test_upscale_tail_rejects_partial_blocks(dev):
    from protosam_amd import ops
    g = 12                           # g * g = 144: not a whole number of 64-pixel workgroups
    u1 = _rand((g * g, 256), 1).to(dev)
    masks = _nan((1, 4, 4 * g, 4 * g), dev)
    z = torch.zeros(64, device=dev)
    with pytest.raises(RuntimeError, match="status 1"):
        ops.upscale_tail(u1, z, z, torch.zeros((64, 128), device=dev), z[:32], torch.zeros((1, 4, 32), device=dev), 1, g, masks=masks)
    assert bool(masks.isnan().all())


# ---- 6. mask_downscale -------------------------------------------------------------------------------------------------
def _mask_prompts(n, g, seed):
    S = 4 * g
    m = F.interpolate(_rand((n, 1, S // 16, S // 16), seed, 4.0), size=(S, S), mode="bicubic", align_corners=False)[:, 0]
    m[0, S // 8:S // 2, S // 4:3 * S // 4] = 20.0
    m[-1, S // 2:, : S // 3] = -20.0
    m[:, -S // 8:, -S // 8:] = 20.0
    return m.contiguous()


@pytest.mark.parametrize("n,g", [(2, 64), (3, 16)])
def test_mask_downscale(dev, n, g):
    """Mask prompts (prompt_encoder.py:51-59,102-105: Conv 2x2 s2 -> LayerNorm2d -> GELU -> Conv 2x2 s2 -> LayerNorm2d -> GELU ->
    Conv 1x1) in one kernel against oracle.embed_masks in float64, on smooth logits and on +-20 regions."""
    from oracle import sam_prompt_decoder as odec
    from protosam_amd import ops
    pem, sd = _prompt_encoder(dev)
    pk = pem._packed()
    sd64 = {k: v.double() for k, v in sd.items()}
    masks = _mask_prompts(n, g, 80 + g)
    x = masks.double()[:, None]
    ref = odec.embed_masks(sd64, x, pre="")
    w = lambda i, part: sd64[f"mask_downscaling.{i}.{part}"]  # noqa: E731
    c1 = F.conv2d(x, w(0, "weight"), w(0, "bias"), stride=2)
    _, y1m = _ln2d_mag(c1, F.conv2d(x.abs(), w(0, "weight").abs(), w(0, "bias").abs(), stride=2), w(1, "weight"), w(1, "bias"), 1e-6)
    y1 = F.gelu(odec._ln2d(c1, w(1, "weight"), w(1, "bias")))
    c2 = F.conv2d(y1, w(3, "weight"), w(3, "bias"), stride=2)
    c2m = F.conv2d(GELU_SLOPE * y1m, w(3, "weight").abs(), w(3, "bias").abs(), stride=2)
    _, y2m = _ln2d_mag(c2, c2m, w(4, "weight"), w(4, "bias"), 1e-6)
    mag = F.conv2d(GELU_SLOPE * y2m, w(6, "weight").abs(), w(6, "bias").abs())
    out = _nan((n, g * g, 256), dev)
    ops.mask_downscale(masks.to(dev), pk["mask_w"], g, pk["mask_eps"], out=out)
    tm = lambda t: t.permute(0, 2, 3, 1).reshape(n, g * g, 256)  # noqa: E731
    _within(out, tm(ref), tm(mag), 8, f"mask_downscale n={n} g={g}")


# ---- 7. gemm_f32 / gemm_f32_heads --------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [4096, 16384, 16385, 5 * 4096 + 37])
@pytest.mark.parametrize("N", [64, 128, 256])
def test_gemm_f32_direct(dev, M, N):
    """The exact-fp32 MFMA GEMM of the decoder's image side (psam_gemm_f32: 64x64 tiles, 64x128 past 16384 rows when N % 128 == 0)
    against float64: plain; `keys + key_pe` as a2 with a2_mod and the in-place residual; head-major output."""
    from protosam_amd import ops
    K = 256
    a, w, bias = _rand((M, K), 91), _rand((N, K), 92, K ** -0.5), _rand((N,), 93, 0.1)
    a2, x = _rand((4096, K), 94), _rand((M, N), 95)
    ad, wd, bd = a.double(), w.double(), bias.double()
    rep = lambda t: t.repeat((M + 4095) // 4096, 1)[:M]  # noqa: E731
    A, W, Bi, A2 = a.to(dev), w.to(dev), bias.to(dev), a2.to(dev)
    ref, mag = _linear_ref(ad, wd, bd, None)
    out = _nan((M, N), dev)
    ops.gemm_f32(A, W, Bi, out=out)
    _within(out, ref, mag, 8, f"gemm_f32 M={M} N={N}")
    sa = ad + rep(a2.double())
    ref2, mag2 = sa @ wd.t() + bd + x.double(), (ad.abs() + rep(a2.double()).abs()) @ wd.abs().t() + bd.abs() + x.double().abs()
    y = x.to(dev)
    ops.gemm_f32(A, W, Bi, out=y, resid=y, a2=A2, a2_mod=4096)
    _within(y, ref2, mag2, 8, f"gemm_f32 a2 + in-place residual M={M} N={N}")
    if M % 4096 == 0:
        nk, hd = 4096, 16
        hm = _nan((M * N,), dev)
        ops.gemm_f32(A, W, Bi, out=hm, a2=A2, a2_mod=4096, heads=(nk, hd))
        ref3 = (sa @ wd.t() + bd).view(M // nk, nk, N // hd, hd).permute(0, 2, 1, 3)
        mag3 = (mag2 - x.double().abs()).view(M // nk, nk, N // hd, hd).permute(0, 2, 1, 3)
        _within(hm, ref3.reshape(-1), mag3.reshape(-1), 8, f"gemm_f32_heads M={M} N={N}")


# ---- 8. the round-1 token-to-image attention kernel (16 < Nk < 64) -----------------------------------------------------
@pytest.mark.parametrize("Nk", [17, 40, 63])
@pytest.mark.parametrize("T", [1, 9, 16])
@pytest.mark.parametrize("kdt", [torch.float32, torch.float16])
def test_t2i_round1_kernel(dev, Nk, T, kdt):
    """psam_t2i_attention below 64 keys (Attention.forward with 16 < Nk < 64) runs the one-workgroup-per-(token, head, prompt set)
    kernel: against the float64 softmax(q k^T / 4) v of test_t2i_attention_key_split, K / V token-major fp32 or fp16."""
    from protosam_amd import ops
    B, NH = 2, 8
    q = _rand((B * T, 128), 101, 1.5)
    k, v = _rand((B * Nk, 128), 102), _rand((B * Nk, 128), 103)
    k[5] *= 6.0
    kq, vq = k.to(kdt), v.to(kdt)
    ref, mag = _attention_ref(q.double(), kq.double(), vq.double(), B, T, Nk, NH, 16)
    out = _nan((B * T, 128), dev)
    ops.t2i_attention(q.to(dev), kq.to(dev), vq.to(dev), out, B, T, Nk, NH)
    _within(out, ref, mag, 8, f"t2i round-1 Nk={Nk} T={T} {kdt}")


# ---- 9. the whole decoder against the oracle ---------------------------------------------------------------------------
DECODER_CASES = [(1, 6), (2, 16), (5, 9), (6, 11), (33, 7)]
N_IMG = 3
_DEC = {}


def _decoder(dev):
    if "md" not in _DEC:
        from protosam_amd.segment_anything.modeling.mask_decoder import MaskDecoder
        from protosam_amd.segment_anything.modeling.transformer import TwoWayTransformer
        from protosam_amd.synth import synth_state_dict
        md = MaskDecoder(transformer_dim=256, transformer=TwoWayTransformer(depth=2, embedding_dim=256, mlp_dim=2048, num_heads=8),
                         num_multimask_outputs=3, iou_head_depth=3, iou_head_hidden_dim=256)
        sd = synth_state_dict(md, 1234)
        md.load_state_dict(sd, strict=True)
        from oracle import sam_prompt_decoder as odec
        G = _rand((2, 128), 111)
        y = ((torch.arange(64, dtype=torch.float32) + 0.5) / 64)[:, None].expand(64, 64)
        pe = odec.pe_encoding(torch.stack([y.t(), y], -1), G).permute(2, 0, 1)[None].contiguous()   # [1,256,64,64] fp32
        _DEC.update(md=md.to(dev).eval(), sd64={k: v.double() for k, v in sd.items()}, feats=_rand((N_IMG, 256, 64, 64), 112),
                    pe=pe, dense=_rand((256,), 113, 0.5))
    return _DEC


def _decoder_case(dev, B, T):
    """(inputs, float64 oracle taps) of B prompt sets of T tokens over N_IMG images, computed once per (B, T)."""
    from oracle import sam_prompt_decoder as odec
    D = _decoder(dev)
    if (B, T) not in _DEC:
        sparse = _rand((B, T - 5, 256), 120 + B * 17 + T)
        iop = torch.tensor([(7 * i + 2) % N_IMG for i in range(B)], dtype=torch.int32)
        taps = {k: [None] * B for k in ("hs", "keys", "hyper", "masks_all", "iou_all")}
        for im in range(N_IMG):
            idx = [i for i in range(B) if int(iop[i]) == im]
            if not idx:
                continue
            t = {}
            dense = D["dense"].double().reshape(1, -1, 1, 1).expand(len(idx), -1, 64, 64)
            odec.mask_decoder(D["sd64"], D["feats"][im:im + 1].double(), D["pe"].double(), sparse[idx].double(), dense, True, pre="",
                              taps=t)
            for k in taps:
                for j, i in enumerate(idx):
                    taps[k][i] = t[k][j]
        _DEC[(B, T)] = (sparse, iop, {k: torch.stack(v) for k, v in taps.items()})
    return _DEC[(B, T)]


# {tap: bound}; measured on MI355X, worst over DECODER_CASES: x3 hs 6.7e-7, keys 4.4e-7, hyper 8.5e-7, masks 1.1e-6, prob 1.3e-6,
# iou 1.6e-6; f32 hs 6.7e-7, keys 5.4e-7, hyper 9.6e-7, masks 1.3e-6, prob 1.7e-6, iou 1.3e-6; f16 hs 2.7e-4, keys 3.0e-4,
# hyper 4.4e-4, masks 6.4e-4, prob 7.8e-4, iou 2.8e-4. hs / keys / hyper / masks relative to the tap's largest |value|,
# sigmoid(masks) (prob) and iou absolute. About 5x headroom; the fp16 image side keeps the 1e-3 budget of its docstring.
_FP32_BOUNDS = dict(hs=4e-6, keys=3e-6, hyper=6e-6, masks=7e-6, prob=1e-5, iou=1e-5)
DECODER_BOUNDS = {"x3": _FP32_BOUNDS, "f32": _FP32_BOUNDS,
                  "f16": dict(hs=1.5e-3, keys=1.5e-3, hyper=2e-3, masks=3.5e-3, prob=1e-3, iou=1e-3)}


@pytest.mark.parametrize("path", ["x3", "f32", "f16"])
@pytest.mark.parametrize("B,T", DECODER_CASES)
def test_decoder_sweep(dev, B, T, path):
    """MaskDecoder.predict_masks_tokens (mask_decoder.py:112-149 for B prompt sets on 3 images, img_of_prompt not monotone) against
    oracle.mask_decoder in float64 per prompt set, stage by stage: the queries after the two-way transformer (hs), the keys, the
    hyper-network vectors, the low-res masks and IoU. The (B, T) cases span the B*T >= 32 split-K MLP, the M >= 32 MFMA form of the
    hyper-network linears, the token-to-image key split (16 ... 1 ranges) and, on the exact-fp32 path, the 64x128 gemm_f32 tile
    (B >= 5). Image side: `x3` = gemm_f32x3 (default), `f32` = exact-fp32 MFMA (image_side_x3 = False), `f16` = fp16 operands
    (image_side_fp16 = True, the 1e-3 budget of its docstring). Measured on MI355X, worst over the cases: sigmoid(low_res_masks)
    1.3e-6 (x3), 1.7e-6 (f32), 7.8e-4 (f16); IoU 1.6e-6, 1.3e-6, 2.8e-4. Bounds per stage in DECODER_BOUNDS."""
    D = _decoder(dev)
    md = D["md"]
    sparse, iop, ref = _decoder_case(dev, B, T)
    md.image_side_x3, md.image_side_fp16 = path == "x3", path == "f16"
    try:
        feat = D["feats"].permute(0, 2, 3, 1).reshape(N_IMG, 4096, 256).contiguous().to(dev)
        pe_tok = D["pe"][0].permute(1, 2, 0).reshape(4096, 256).contiguous().to(dev)
        tokens = md.build_tokens(sparse.to(dev))
        assert tokens.shape == (B, T, 256)
        masks, iou = _nan((B, 4, 256, 256), dev), _nan((B, 4), dev)
        _, _, hs = md.predict_masks_tokens(feat, pe_tok, tokens, D["dense"].to(dev), img_of_prompt=iop.to(dev), masks_out=masks,
                                           iou_out=iou)
        keys = md.transformer._ws[(B, T, 4096, path == "f16")]["keys"]
        hyper = md._ws[(B, T, 4096)]["hyper"]
        got = dict(hs=hs, keys=keys.view(B, 64, 64, 256).permute(0, 3, 1, 2), hyper=hyper, masks=masks)
        want = dict(hs=ref["hs"], keys=ref["keys"], hyper=ref["hyper"], masks=ref["masks_all"])
        errs = {}
        for k in got:
            g = got[k].double().cpu()
            assert bool(torch.isfinite(g).all()), k
            errs[k] = (g - want[k]).abs().max().item() / want[k].abs().max().item()
        errs["prob"] = (torch.sigmoid(masks.double().cpu()) - torch.sigmoid(ref["masks_all"])).abs().max().item()
        assert bool(torch.isfinite(iou).all())
        errs["iou"] = (iou.double().cpu() - ref["iou_all"]).abs().max().item()
        print(f"decoder {path} B={B} T={T}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        bounds = DECODER_BOUNDS[path]
        for k, v in errs.items():
            assert v < bounds[k], (path, B, T, k, v, bounds[k])
    finally:
        md.image_side_x3, md.image_side_fp16 = True, False


# ---- the once-per-process A/B switches ---------------------------------------------------------------------------------
def test_fallback_kernels_in_a_fresh_process(dev):
    """The A/B switches PSAM_UPSCALE_MFMA=0 (scalar ConvT #2), PSAM_GEMM_F32_SHAPE=0 (128x128 gemm_f32 tiles), PSAM_T2I_ALL=0 and
    PSAM_SMALL_LINEAR_VEC=0 are read once per process: checks 5, 7 and 8 repeated in a child process that sets them."""
    env = dict(os.environ, PSAM_UPSCALE_MFMA="0", PSAM_GEMM_F32_SHAPE="0", PSAM_T2I_ALL="0", PSAM_SMALL_LINEAR_VEC="0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "test_upscale_tail or test_gemm_f32_direct or test_t2i_round1_kernel"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "skipped" not in tail, tail
    print("child process:", tail.strip().splitlines()[-1])
