"""The two encoders on the HIP path, held per token row to the rounding model of oracle/encoder_model.py: with ref = the float64
forward and model = the same forward with a round-to-fp16 wherever the product stores fp16, every row r of every image must have

    rms_c(out[r] - model[r]) <= sqrt(2) * rms_c(model[r] - ref[r])

(tests/test_encoder_ladder_cpu.py shows what that catches and what it lets through). This is the layer above the kernel tests: which
LayerNorm placement runs (`fold_pays`), DINOv2's unfolded block 0, the cls / register rows beside a GEMM with `out_seg`, `resid_mod`
position tables, `pad_row`, window or global attention per block, the split-K lin2 hand-off, sub-batch workspace views, the neck.

Every case (oracle/encoder_ladder.py CASES) runs at each depth d = 1 .. D through a model BUILT with d blocks; weights are seeded by name,
so block i is the same in every one, and ref / model per (case, family, LayerNorm placement) come from one float64 forward each, computed
once per process. Every test names the kernel or tile it means to run and asserts it, restores every switch it touches, and prints one
line per (case, path, d): worst row ratio, rms and max of out - ref and of model - ref.

Not in the matrix: `gemm_x3` and `split_fp16` (fewer rounding places: they need a model of their own).
"""
import functools

import pytest
import torch

from oracle import encoder_ladder as L
from oracle import encoder_model as EM

pytestmark = pytest.mark.gpu

DINO_CASES = tuple(c for c in L.LADDER if L.CASES[c]["kind"] == "dino")
SAM_CASES = tuple(c for c in L.LADDER if L.CASES[c]["kind"] == "sam")
TILES = (15, 17, 11, 1)


@functools.lru_cache(maxsize=None)
def _module(case, family, d):
    """the product encoder with d blocks and the case's weights, on the GPU (one per process)"""
    c = L.CASES[case]
    sd = L.state_dict_for_depth(case, family, d)
    if c["kind"] == "dino":
        from protosam_amd.dinov2 import DinoVisionTransformer
        m = DinoVisionTransformer(c["product"], depth=d)
    else:
        from protosam_amd.segment_anything.modeling.image_encoder import ImageEncoderViT
        cfg = c["cfg"]
        m = ImageEncoderViT(img_size=c["S"], embed_dim=cfg["embed_dim"], depth=d, num_heads=cfg["num_heads"], use_rel_pos=True,
                            window_size=cfg["window_size"], global_attn_indexes=cfg["global_attn_indexes"])
        sd = {k[len(L.SAM_PRE):]: v for k, v in sd.items()}
    m.load_state_dict(sd, strict=True)
    return m.to("cuda:0").eval()


def _folds(m, rows):
    """the LayerNorm placement the product takes for `rows` token rows under its current switches (dinov2.py / image_encoder.py)"""
    from protosam_amd import ops
    return bool(m.fold_ln and not ops.QKV_HEAD_MAJOR and m.embed_dim % 64 == 0
                and ops.fold_pays(rows, m.embed_dim, torch.device("cuda:0"), m.fold_min_fill))


def _forward(case, m, x, eager):
    c = L.CASES[case]
    m.__dict__.pop("_graphs", None)                 # (a replayed graph dispatches nothing: capture again, so the kernels asserted are this call's)
    with torch.no_grad():
        if c["kind"] == "dino":
            if eager:
                return m._forward_tokens(x, c["S"]).cpu().double()
            f = m.forward_features(x)
            return torch.cat([f["x_norm_clstoken"][:, None], f["x_norm_regtokens"], f["x_norm_patchtokens"]], 1).cpu().double()
        if eager:
            from protosam_amd import ops
            P = m.patch_size
            return m._encode_patches(ops.patchify_bilinear(x.contiguous(), m.img_size, P, 3 * P * P), x.shape[0]).cpu().double()
        return m.forward_tokens(x).cpu().double()


def _expected_attention(case, d, variant=5, head_major=False):
    """the ATTN_KERNEL_* families the LAST block of a model of d blocks may land on"""
    from protosam_amd import ops
    c = L.CASES[case]
    if c["kind"] == "dino":                         # mode 0, hd 64, 257 / 261 tokens
        if variant & 16:
            return (ops.ATTN_KERNEL_GATTN,)
        return (ops.ATTN_KERNEL_ASM_NOREL, ops.ATTN_KERNEL_GATTN) if head_major else (ops.ATTN_KERNEL_ASM_NOREL,)
    cfg = c["cfg"]
    hd = cfg["embed_dim"] // cfg["num_heads"]
    if d - 1 in cfg["global_attn_indexes"]:
        return (ops.ATTN_KERNEL_ASM_FUSED,) if cfg["grid"] == 64 else (ops.ATTN_KERNEL_GATTN_ANY,)
    return (ops.ATTN_KERNEL_ASM_WINDOW,) if (cfg["grid"] == 64 and hd == 80) else (ops.ATTN_KERNEL_WATTN_P,)


def _ladder(case, family, path, fold_ln=None, fold_min_fill=None, tile=0, variant=5, head_major=False, eager=False, splitk=False,
            expect_fold=None, after=None):
    """the case at every depth under one set of switches: asserts the kernels that ran, prints a line per depth, checks every row"""
    from protosam_amd import ops
    c = L.CASES[case]
    x = L.image(case).to("cuda:0")
    rows = c["B"] * ((c["S"] // EM.DINO_PATCH) ** 2 + 1 + c["cfg"]["num_register_tokens"] if c["kind"] == "dino" else c["cfg"]["grid"] ** 2)
    ref = L.ref(case, family)
    failures = []
    for d in range(1, c["depth"] + 1):
        m = _module(case, family, d)
        saved = (m.fold_ln, m.fold_min_fill, getattr(m, "splitk_lin2", None))
        try:
            if fold_ln is not None:
                m.fold_ln = fold_ln
            if fold_min_fill is not None:
                m.fold_min_fill = fold_min_fill
            if splitk:
                m.splitk_lin2 = True
            ops.QKV_HEAD_MAJOR = head_major
            ops.gemm_set_tile(tile)
            ops.attention_set_variant(variant)
            fold = _folds(m, rows)
            assert expect_fold is None or fold == expect_fold, f"{case} {path}: LayerNorm folded = {fold}, the path means {expect_fold}"
            out = _forward(case, m, x, eager)
            landed_tile, landed_attn = ops.gemm_last_tile(), ops.attention_last_kernel()
            if after is not None:
                after(m, d)
        finally:
            m.fold_ln, m.fold_min_fill = saved[:2]
            if saved[2] is not None:
                m.splitk_lin2 = saved[2]
            ops.QKV_HEAD_MAJOR = False
            ops.gemm_set_tile(0)
            ops.attention_set_variant(5)
            m.__dict__.pop("_graphs", None)
        model, peak = L.model(case, family, fold)
        EM.preconditions(ref[d - 1], model[d - 1], peak)
        what = (f"{case} {family} {path} d={d} [LayerNorm {'folded' if fold else 'separate'}, last GEMM tile {landed_tile}, "
                f"last attention {ops.attention_kernel_name(landed_attn)}]")
        print(EM.report(what, out, model[d - 1], ref[d - 1]))
        assert landed_tile == tile if tile else landed_tile > 0, f"{what}: tile {tile} asked for"
        want = _expected_attention(case, d, variant, head_major)
        assert landed_attn & ops.ATTN_KERNEL_FAMILY in want, f"{what}: meant for {[ops.ATTN_KERNEL_NAMES[k] for k in want]}"
        try:
            EM.row_check(out, model[d - 1], ref[d - 1], what)
        except AssertionError as e:                 # (every depth is measured and printed before the test fails)
            failures.append(str(e))
    assert not failures, "\n".join(failures)


# ---- DINOv2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", L.FAMILIES)
@pytest.mark.parametrize("case", DINO_CASES)
class TestDino:
    def test_default_forward_features(self, dev, case, family):
        """as the pipeline calls it (graph replay where `graph_wanted`); a few hundred rows: `fold_pays` says no, separate LayerNorms"""
        _ladder(case, family, "default forward_features", expect_fold=False)

    def test_eager_forward_tokens(self, dev, case, family):
        _ladder(case, family, "eager _forward_tokens", eager=True, expect_fold=False)

    def test_fold_forced(self, dev, case, family):
        """fold_min_fill = 0: block 0's norm1 a pass of its own, every later LayerNorm folded, on the tile the picker chooses"""
        _ladder(case, family, "fold forced", fold_ln=True, fold_min_fill=0.0, eager=True, expect_fold=True)

    @pytest.mark.parametrize("tile", TILES)
    def test_fold_forced_on_tile(self, dev, case, family, tile):
        _ladder(case, family, f"fold forced tile {tile}", fold_ln=True, fold_min_fill=0.0, tile=tile, eager=True, expect_fold=True)

    def test_fold_off(self, dev, case, family):
        _ladder(case, family, "fold off", fold_ln=False, fold_min_fill=0.0, eager=True, expect_fold=False)

    def test_hip_global_attention_kernel(self, dev, case, family):
        """attention variant 5 | 16: the DMA-fed HIP kernel in place of the assembly one"""
        _ladder(case, family, "attention variant 5|16", variant=5 | 16, eager=True)

    def test_head_major_qkv(self, dev, case, family):
        """ops.QKV_HEAD_MAJOR: qkv written [3, H, B*N, hd] by gemm_heads; the fold is off on this layout. That the layout ran is read off
        the workspace: the last block's qkv buffer, viewed head-major, holds what the token-major run left viewed [B*N, 3, H, hd] (the same
        products on another tile: within two fp16 ulps of the largest value; a buffer in the other layout is off by the values themselves)."""
        c = L.CASES[case]
        H = c["cfg"]["num_heads"]
        hd = c["cfg"]["embed_dim"] // H
        qkv = {}

        def grab(tag):
            return lambda m, d: qkv.__setitem__((tag, d), next(iter(m._ws.values()))["qkv"].clone())
        _ladder(case, family, "head-major qkv", head_major=True, fold_min_fill=0.0, eager=True, expect_fold=False, after=grab("hm"))
        _ladder(case, family, "token-major qkv (layout reference)", fold_ln=False, eager=True, expect_fold=False, after=grab("tm"))
        for d in range(1, c["depth"] + 1):
            hm = qkv["hm", d].view(3, H, -1, hd).float()
            tm = qkv["tm", d].view(-1, 3, H, hd).permute(1, 2, 0, 3).float()
            assert float((hm - tm).abs().max()) <= 2.0 ** -8 * float(tm.abs().max()), f"{case} {family} d={d}: qkv is not head-major"
            assert float((qkv["hm", d].view(-1, 3, H, hd).float() - tm.permute(2, 0, 1, 3)).abs().max()) > 0.1 * float(tm.abs().max())


# ---- SAM -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", L.FAMILIES)
@pytest.mark.parametrize("case", SAM_CASES)
class TestSam:
    def test_default_forward_tokens(self, dev, case, family):
        """as `Sam` calls it (graph replay for one or two images); at most 16 row tiles: separate LayerNorms"""
        _ladder(case, family, "default forward_tokens", expect_fold=False)

    def test_fold_forced(self, dev, case, family):
        """every LayerNorm of the blocks folded, block 0's norm1 into the patch-embedding GEMM with its `resid_mod` position table"""
        _ladder(case, family, "fold forced", fold_ln=True, fold_min_fill=0.0, eager=True, expect_fold=True)

    @pytest.mark.parametrize("tile", TILES)
    def test_fold_forced_on_tile(self, dev, case, family, tile):
        _ladder(case, family, f"fold forced tile {tile}", fold_ln=True, fold_min_fill=0.0, tile=tile, eager=True, expect_fold=True)

    def test_fold_off(self, dev, case, family):
        _ladder(case, family, "fold off", fold_ln=False, fold_min_fill=0.0, eager=True, expect_fold=False)


@pytest.mark.parametrize("family", L.FAMILIES)
def test_sam_splitk_lin2_vit_h(dev, family):
    """`splitk_lin2` at ViT-H width, one image: mlp.lin2 as K ranges, the next block's norm1 (or the neck's fp16 copy) written by the
    reduce pass (`ln1_ready`). Its LayerNorm placement is the separate-pass model's."""
    from protosam_amd import ops
    cfg = L.CASES["sam_h64"]["cfg"]
    ks = ops.gemm_splitk_ranges(cfg["grid"] ** 2, cfg["embed_dim"], 4 * cfg["embed_dim"])
    print(f"sam_h64: mlp.lin2 of one image in {ks} K ranges")
    assert ks >= 2
    _ladder("sam_h64", family, f"splitk_lin2 ({ks} K ranges)", splitk=True, expect_fold=False)


@pytest.mark.parametrize("family", L.FAMILIES)
def test_sam_sub_batch_after_batch(dev, family):
    """B = 2, then B = 1 on the same module: the one-image call runs on views of the two-image workspace and must give image 0's rows"""
    from protosam_amd import ops
    case = "sam_b16"
    c = L.CASES[case]
    d = c["depth"]
    x = L.image(case).to("cuda:0")
    m = _module(case, family, d)
    m._ws.clear()
    m.__dict__.pop("_graphs", None)
    try:
        with torch.no_grad():
            two = m.forward_tokens(x).cpu().double()
            assert sorted(m._ws) == [2]
            one = m.forward_tokens(x[:1]).cpu().double()
        assert sorted(m._ws) == [1, 2] and m._ws[1]["x"].data_ptr() == m._ws[2]["x"].data_ptr(), "the sub-batch runs on views"
        landed = ops.attention_last_kernel()
    finally:
        m._ws.clear()
        m.__dict__.pop("_graphs", None)
    assert landed & ops.ATTN_KERNEL_FAMILY in _expected_attention(case, d)
    assert not _folds(m, 2 * c["cfg"]["grid"] ** 2)
    ref, (model, peak) = L.ref(case, family)[-1], L.model(case, family, False)
    EM.preconditions(ref, model[-1], peak)
    for name, out, sl in (("B=2", two, slice(0, 2)), ("B=1 on views of B=2", one, slice(0, 1))):
        what = f"{case} {family} {name} d={d} [last attention {ops.attention_kernel_name(landed)}]"
        print(EM.report(what, out, model[-1][sl], ref[sl]))
        EM.row_check(out, model[-1][sl], ref[sl], what)
