"""CPU: the yardstick of tests/test_decoder_tokens_gpu.py (prompt sets of more than 16 tokens: psam_token_attention and the
token-grouped psam_t2i_attention), checked without a GPU.

  - the float64 attention reference the GPU tests compare against (`_attention_ref` of test_decoder_kernels_gpu.py) is pinned to
    torch.nn.functional.scaled_dot_product_attention in float64;
  - the error bounds the GPU tests use (`token_bound`, `t2i_bound`: derived from the kernels' summation order, below) refuse the
    faults a chunked kernel can have - a key dropped at the first chunk boundary, the last key dropped, a phantom key after the
    last one, two keys (or two tokens) exchanged across a chunk / token-group boundary, a softmax sum that lacks one key - when
    these are applied to the reference's own output at every tested number of tokens;
  - the one constant MAX_PROMPT_TOKENS is the same number in the public header, the kernels' common.h and ops.py, and the
    Python layers refuse more with the number in the message.

The bounds, in units of 2^-23 x `mag` of `_attention_ref` (eps = 2^-24 is one rounding, so c = roundings / 2):

psam_token_attention (csrc/decoder.hip), one thread per (query row, head), keys in chunks of CHUNK = 16:
  weights   every unnormalised weight exp(s_j - m_chunk) exp(m_chunk - m) carries (hd + 3) eps smag_j from its score (a serial chain
            of hd fused multiply-adds, the product with 1 / sqrt(hd) and that constant's own rounding) and 22 eps from the two exponent
            differences (|x| eps each, together at most 24 ln 2 < 17 for a weight above 2^-24 of the largest), the two expf (2 eps
            each) and their product: at most max(hd + 3, 22) eps against the p_j (1 + smag_j) (|v_j| + |out|) terms of `mag`;
  chunk     the chunk's sums of p and p v are serial chains of min(Tk, 16) fused multiply-adds: 16 eps;
  merges    the running (l, o) take ceil(Tk / 16) - 1 merges o a1 + o_chunk a2 (the first is exact: a1 = 0, a2 = 1): two roundings
            and the 3 eps of the factor (an expf of a rounded difference) each: 5 eps per merge;
  division  1 eps.
  c = (max(hd + 3, 22) + 16 + 5 (ceil(Tk / 16) - 1) + 1) / 2: 28.5 at (17 keys, hd 32), 63.5 at (256, 32), 57 at (256, 16).

psam_t2i_attention[_split] (one wave per token, lane kl walks keys kl, kl + 64, ... of its key range with an online softmax):
  weights   as above with hd = 16 and q scaled by 1/4 first (exact): max(16 + 2, 22) = 22 eps;
  lane      n = ceil(range / 64) serial steps l = l sc + p, o = o sc + p v: two roundings and the 3 eps of sc each: 5 n eps, where
            range = Nk unsplit and ceil(Nk / (64 S)) 64 with S key ranges;
  merges    six butterfly levels over the wave's 64 lanes, and four more in t2i_combine_kernel when S > 1, 5 eps each;
  division  1 eps.
  c = (22 + 5 n + 30 + (20 if S > 1) + 1) / 2: 186.5 at (4096 keys, unsplit), 29 at 64 keys.
Both are worst cases over the rounding directions; the GPU tests record what they measure in profiles/decoder_many_tokens_tests.txt.
"""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from test_decoder_kernels_gpu import U, _attention_ref, _rand, _within   # noqa: E402  (torch-only helpers of a GPU test module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 16                                  # keys per LDS chunk of token_attention_kernel, tokens per workgroup of t2i_attention_all_kernel
SELF_T = [17, 32, 33, 64, 65, 256]          # token self-attention (hd 32)
I2T_TK = [17, 33, 64, 256]                  # image-to-token (hd 16)
T2I_T = [17, 32, 33, 100]                   # token-to-image tokens
T2I_NK = [64, 4096]


def token_bound(Tk, hd):
    return (max(hd + 3, 22) + min(Tk, CHUNK) + 5 * (math.ceil(Tk / CHUNK) - 1) + 1) / 2


def t2i_bound(Nk, S=1):
    rng = Nk if S <= 1 else math.ceil(Nk / (64 * S)) * 64
    return (22 + 5 * math.ceil(rng / 64) + 30 + (20 if S > 1 else 0) + 1) / 2


def test_bounds_are_the_documented_figures():
    assert token_bound(17, 32) == 28.5 and token_bound(256, 32) == 63.5 and token_bound(256, 16) == 57
    assert token_bound(16, 32) == 26 and token_bound(32, 16) == 22
    assert t2i_bound(4096) == 186.5 and t2i_bound(64) == 29 and t2i_bound(4096, 16) == 46.5 and t2i_bound(64, 3) == 39


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def _heads(x, B, T, NH, hd):
    return x.view(B, T, NH, hd).permute(0, 2, 1, 3)


def _flat(x, B, T, NH, hd):
    return x.permute(0, 2, 1, 3).reshape(B * T, NH * hd)


@pytest.mark.parametrize("B,Tq,Tk,hd", [(3, 17, 17, 32), (1, 256, 256, 32), (2, 64, 33, 16), (2, 100, 4096, 16)])
def test_reference_is_float64_sdpa(B, Tq, Tk, hd):
    NH = 8
    q, k, v = (_rand((B * t, NH * hd), s).double() for t, s in ((Tq, 1), (Tk, 2), (Tk, 3)))
    ref, mag = _attention_ref(q, k, v, B, Tq, Tk, NH, hd)
    sdpa = F.scaled_dot_product_attention(_heads(q, B, Tq, NH, hd), _heads(k, B, Tk, NH, hd), _heads(v, B, Tk, NH, hd))
    assert sdpa.dtype == torch.float64
    torch.testing.assert_close(ref, _flat(sdpa, B, Tq, NH, hd), rtol=1e-13, atol=1e-14)
    assert bool((mag > 0).all()) and bool((mag >= ref.abs()).all())


# ---- injected faults -------------------------------------------------------------------------------------------------------------
def _softmax_parts(q, k, B, Tq, Tk, NH, hd):
    s = _heads(q, B, Tq, NH, hd) @ _heads(k, B, Tk, NH, hd).transpose(-1, -2) / math.sqrt(hd)
    return torch.exp(s - s.amax(-1, keepdim=True))          # unnormalised weights [B, NH, Tq, Tk]


def faulty_outputs(q, k, v, B, Tq, Tk, NH, hd, boundary=CHUNK):
    """{fault: output} of the faults a chunked attention kernel can have, in float64 from the reference's own arithmetic.
    boundary: the first key of the second chunk (the kernel's chunk size, or 64 for a lane stride)."""
    vh = _heads(v, B, Tk, NH, hd)
    p = _softmax_parts(q, k, B, Tq, Tk, NH, hd)
    out = {}

    def without(j):
        keep = [i for i in range(Tk) if i != j]
        return _flat((p[..., keep] @ vh[:, :, keep]) / p[..., keep].sum(-1, keepdim=True), B, Tq, NH, hd)
    out["key at the chunk boundary dropped"] = without(boundary)
    out["last key dropped"] = without(Tk - 1)
    gk, gv = _rand((B, 1, NH * hd), 71).double(), _rand((B, 1, NH * hd), 72).double()
    k2 = torch.cat([k.view(B, Tk, -1), gk], 1).reshape(B * (Tk + 1), -1)
    v2 = torch.cat([v.view(B, Tk, -1), gv], 1).reshape(B * (Tk + 1), -1)
    out["phantom key after the last"] = _attention_ref(q, k2, v2, B, Tq, Tk + 1, NH, hd)[0]
    perm = list(range(Tk))
    perm[boundary - 1], perm[boundary] = perm[boundary], perm[boundary - 1]
    out["values of two keys exchanged across the boundary"] = _flat((p @ vh[:, :, perm]) / p.sum(-1, keepdim=True), B, Tq, NH, hd)
    less = p.sum(-1, keepdim=True) - p[..., boundary:boundary + 1]
    out["softmax sum without one key"] = _flat((p @ vh) / less, B, Tq, NH, hd)
    return out


def _assert_refused(bad, ref, mag, c, what):
    with pytest.raises(AssertionError, match="elements off by more than"):
        _within(bad, ref, mag, c, what)


@pytest.mark.parametrize("T", SELF_T)
def test_self_attention_checks_refuse_faults(T):
    B, NH, hd = 3, 8, 32
    q, k, v = (_rand((B * T, 256), s).double() for s in (1, 2, 3))
    ref, mag = _attention_ref(q, k, v, B, T, T, NH, hd)
    _within(ref.float(), ref, mag, token_bound(T, hd), f"fp32-rounded reference T={T}")
    for name, bad in faulty_outputs(q, k, v, B, T, T, NH, hd).items():
        _assert_refused(bad, ref, mag, token_bound(T, hd), name)
    swapped = ref.view(B, T, 256).clone()                       # two query rows exchanged across the 16-token boundary
    swapped[:, [15, 16]] = swapped[:, [16, 15]]
    _assert_refused(swapped.reshape(B * T, 256), ref, mag, token_bound(T, hd), "rows 15 / 16 exchanged")


@pytest.mark.parametrize("Tk", I2T_TK)
def test_image_to_token_checks_refuse_faults(Tk):
    B, Tq, NH, hd = 2, 64, 8, 16
    q, k, v = _rand((B * Tq, 128), 11).double(), _rand((B * Tk, 128), 12).double(), _rand((B * Tk, 128), 13).double()
    ref, mag = _attention_ref(q, k, v, B, Tq, Tk, NH, hd)
    floor16 = 2.0 ** -11 * ref.abs() + 2.0 ** -25               # the fp16 output's own rounding, as the GPU test allows it
    for name, bad in faulty_outputs(q, k, v, B, Tq, Tk, NH, hd).items():
        _assert_refused(bad, ref, mag, token_bound(Tk, hd), name)
        with pytest.raises(AssertionError, match="elements off by more than"):
            _within(bad, ref, mag, token_bound(Tk, hd), name + " (fp16 floor)", floor=floor16)


@pytest.mark.parametrize("Nk", T2I_NK)
@pytest.mark.parametrize("T", T2I_T)
def test_token_to_image_checks_refuse_faults(T, Nk):
    """the loosest bound any tested split count has at this Nk, against faults at the lane stride (key 64 would be lane 0's second
    key; at Nk = 64 the last lane's only key) and a token exchanged across the 16-token group boundary"""
    B, NH, hd = 2, 8, 16
    q, k, v = _rand((B * T, 128), 21, 1.5).double(), _rand((B * Nk, 128), 22).double(), _rand((B * Nk, 128), 23).double()
    ref, mag = _attention_ref(q, k, v, B, T, Nk, NH, hd)
    c = max(t2i_bound(Nk, S) for S in (1, 3, 16))
    _within(ref.float(), ref, mag, c, f"fp32-rounded reference T={T} Nk={Nk}")
    for name, bad in faulty_outputs(q, k, v, B, T, Nk, NH, hd, boundary=min(64, Nk - 1)).items():
        _assert_refused(bad, ref, mag, c, name)
    swapped = ref.view(B, T, 128).clone()
    swapped[:, [15, 16]] = swapped[:, [16, 15]]
    _assert_refused(swapped.reshape(B * T, 128), ref, mag, c, "tokens 15 / 16 exchanged")


# ---- the cap -----------------------------------------------------------------------------------------------------------------------
def test_one_cap_in_header_kernels_and_python():
    from protosam_amd import ops
    pat = re.compile(r"#define\s+PSAM_MAX_PROMPT_TOKENS\s+(\d+)")
    hdr = pat.findall(open(os.path.join(ROOT, "include", "protosam_hip.h")).read())
    com = pat.findall(open(os.path.join(ROOT, "protosam_amd", "csrc", "common.h")).read())
    assert hdr == com == [str(ops.MAX_PROMPT_TOKENS)] and ops.MAX_PROMPT_TOKENS >= 256


def test_python_layers_refuse_more_than_the_cap():
    """_check_shapes (TwoWayTransformer.run_tokens, TwoWayAttentionBlock.forward) and MaskDecoder.predict_masks_tokens name the cap;
    17 ... MAX_PROMPT_TOKENS tokens pass the shape check (they raised "more than 11 sparse prompt tokens" before)."""
    from protosam_amd import ops
    from protosam_amd.segment_anything.modeling import transformer as tr
    from protosam_amd.segment_anything.modeling.mask_decoder import MaskDecoder
    cap = ops.MAX_PROMPT_TOKENS
    for T in (17, 133, cap):
        tr._check_shapes(256, T, 4096, 8)
    with pytest.raises(NotImplementedError, match=str(cap)):
        tr._check_shapes(256, cap + 1, 4096, 8)
    md = MaskDecoder(transformer_dim=256, transformer=tr.TwoWayTransformer(depth=2, embedding_dim=256, mlp_dim=2048, num_heads=8))
    with pytest.raises(NotImplementedError, match=str(cap)):
        md.predict_masks_tokens(torch.zeros(64, 256), torch.zeros(64, 256), torch.zeros(1, cap + 1, 256), torch.zeros(256))


def test_t2i_split_counts_token_groups(monkeypatch):
    """the key split fills the chip with B x heads x token groups x ranges workgroups: 16 tokens per group"""
    from protosam_amd import ops
    monkeypatch.delenv("PSAM_T2I_SPLIT", raising=False)
    assert ops.t2i_split(1, 8, 16, 4096) == 16 and ops.t2i_split(1, 8, 17, 4096) == 16 and ops.t2i_split(1, 8, 33, 4096) == 10
    assert ops.t2i_split(2, 8, 133, 4096) == 1 and ops.t2i_split(1, 8, 256, 4096) == 2 and ops.t2i_split(1, 8, 17, 64) == 1
    monkeypatch.setenv("PSAM_T2I_SPLIT", "3")
    assert ops.t2i_split(27, 8, 40, 4096) == 3
