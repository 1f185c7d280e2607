"""The per-token-row rounding-model check of the encoder ladder (oracle/encoder_model.py `row_check`), held to account on the CPU:

  * with q = identity the new forwards ARE the float64 oracles of the two encoders (oracle/dinov2.py, oracle/sam_image_encoder.py, both
    pinned to the reference), and the parameter names / shapes they read are the product modules';
  * an fp32 torch emulation of the product (dtype float32, fp16 at the model's places; a second variant sums every K in two halves)
    passes the check at every ladder case, both weight families, folded and separate LayerNorm, every depth;
  * every fault of oracle/encoder_model.py FAULTS fails the check at every case it applies to - or is listed in INVISIBLE below, with
    its ratio, as one the check cannot see there.

Conditions asserted on the reference before anything is compared: finite, every row of the model at a distance > 0 from it, nothing
handed to fp16 beyond 65504.

Faults run on the tiny configurations (D = 128, two heads of 64, 5 x 5 and 16 x 16 maps) and on every ladder case.

INVISIBLE: the (fault, case, family, folded) the check does not catch, with the worst row ratio measured; also in
profiles/encoder_ladder_tests.txt. Such a pair is printed, not asserted either way. All three are ONE key of the 4096 of the global
block of sam_b64 (ViT-B width, 64 x 64 map) under the heavy-tailed weights: a key there weighs 1 / 4096 on average, and the Student-t
projections put the model's own error above what losing it moves. The same fault is caught with the plain weights (200 / 25 rows of 4096),
at ViT-H width with both families (12 to 427 rows), and the cls key of the separate-LayerNorm model by 3 rows (1.56); on the 196-key windows
and the 256- / 257- / 261-key cases it is caught everywhere.
"""
import pytest
import torch

from oracle import encoder_ladder as L
from oracle import encoder_model as EM

INVISIBLE = {
    ("mask_last_key", "sam_b64", "heavy", False): 1.01,
    ("mask_last_key", "sam_b64", "heavy", True): 1.05,
    ("mask_cls_key", "sam_b64", "heavy", True): 1.40,
}

FAULT_CASES = L.TINY + L.LADDER


def _assert_preconditions(case, family, fold):
    ref = L.ref(case, family)
    model, peak = L.model(case, family, fold)
    for r, m in zip(ref, model):
        EM.preconditions(r, m, peak)
    return ref, model


@pytest.mark.parametrize("case", ["dino_b", "dino_l_reg"])
def test_dino_shapes_are_the_product_modules(case):
    from protosam_amd.dinov2 import DINO_CFGS, DinoVisionTransformer
    c = L.CASES[case]
    assert {k: DINO_CFGS[c["product"]][k] for k in c["cfg"]} == c["cfg"]
    m = DinoVisionTransformer(c["product"], depth=c["depth"])
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == EM.dino_shapes(c["cfg"], c["depth"])


@pytest.mark.parametrize("case", ["sam_b16", "sam_h64", "sam_b64"])
def test_sam_shapes_are_the_product_modules(case):
    from protosam_amd.segment_anything.modeling.image_encoder import ImageEncoderViT
    c = L.CASES[case]
    cfg = c["cfg"]
    m = ImageEncoderViT(img_size=c["S"], embed_dim=cfg["embed_dim"], depth=c["depth"], num_heads=cfg["num_heads"], use_rel_pos=True,
                        window_size=cfg["window_size"], global_attn_indexes=cfg["global_attn_indexes"])
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == EM.sam_shapes(cfg, c["depth"], "")


@pytest.mark.parametrize("family", L.FAMILIES)
@pytest.mark.parametrize("case,which", [("dino_b", "dinov2_b14"), ("dino_l_reg", "dinov2_l14_reg")])
def test_identity_is_the_dinov2_oracle(case, which, family):
    from oracle import dinov2 as odino
    c = L.CASES[case]
    R = c["cfg"]["num_register_tokens"]
    sd64 = {k: v.double() for k, v in L.state_dict(case, family).items()}
    for d in range(1, c["depth"] + 1):
        want = odino.forward_features(L.image(case).double(), sd64, which, depth=d)
        got = L.ref(case, family)[d - 1]
        diff = max(float((got[:, 0] - want["x_norm_clstoken"]).abs().max()), float((got[:, 1 + R:] - want["x_norm_patchtokens"]).abs().max()))
        print(f"{case} {family} depth {d}: max |dino_forward - oracle.dinov2| = {diff:.3e}")
        assert diff < 1e-10


@pytest.mark.parametrize("family", L.FAMILIES)
def test_identity_is_the_sam_oracle(family):
    """sam_b16 is ViT-B's first three blocks (windows, windows, global: oracle VIT_CFGS["vit_b"]) on a 16 x 16 map"""
    from oracle import sam_image_encoder as oenc
    case = "sam_b16"
    c = L.CASES[case]
    sd64 = {k: v.double() for k, v in L.state_dict(case, family).items()}
    for d in range(1, c["depth"] + 1):
        want = oenc.image_encoder(L.image(case).double(), sd64, pre=L.SAM_PRE, model_type="vit_b", depth=d)
        got = L.ref(case, family)[d - 1]
        diff = float((got - want.flatten(2).transpose(1, 2)).abs().max())
        print(f"{case} {family} depth {d}: max |sam_forward - oracle.sam_image_encoder| = {diff:.3e}")
        assert diff < 1e-10


def test_all_depths_is_what_shallower_models_return():
    """entry d - 1 of `all_depths` equals a forward built with depth d from the state dict without the later blocks"""
    for case in ("dino_tiny16_reg", "sam_tiny16"):
        c = L.CASES[case]
        fn = EM.dino_forward if c["kind"] == "dino" else EM.sam_forward
        for d in range(1, c["depth"] + 1):
            one = fn(L.image(case), L.state_dict_for_depth(case, "heavy", d), c["cfg"], d, q=EM.Fp16(), fold=True)
            assert torch.equal(one, L.model(case, "heavy", True)[0][d - 1])


@pytest.mark.parametrize("fold", [False, True], ids=["separate", "folded"])
@pytest.mark.parametrize("family", L.FAMILIES)
@pytest.mark.parametrize("case", L.LADDER + L.TINY)
def test_fp32_emulation_is_under_the_limit(case, family, fold):
    ref, model = _assert_preconditions(case, family, fold)
    for khalves in (False, True):
        emu = L.forward(case, family, dtype=torch.float32, q=EM.Fp16(), fold=fold, khalves=khalves, all_depths=True)
        for d, out in enumerate(emu, 1):
            what = f"{case} {family} {'folded' if fold else 'separate'} fp32 emulation{' K in two halves' if khalves else ''} d={d}"
            print(EM.report(what, out, model[d - 1], ref[d - 1]))
            EM.row_check(out, model[d - 1], ref[d - 1], what)


@pytest.mark.parametrize("fold", [False, True], ids=["separate", "folded"])
@pytest.mark.parametrize("family", L.FAMILIES)
@pytest.mark.parametrize("case", ["dino_b", "sam_b16"])
def test_layernorm_on_the_other_side_stays_under_the_limit(case, family, fold):
    """the model of the OTHER LayerNorm placement as `out`: a different, equally legitimate set of roundings. It must not trip the check
    (the limit has room for roundings the model does not share), and it lands well above the emulation."""
    ref, model = _assert_preconditions(case, family, fold)
    other = L.model(case, family, not fold)[0]
    for d in range(len(ref)):
        what = f"{case} {family} model {'separate' if fold else 'folded'} against model {'folded' if fold else 'separate'} d={d + 1}"
        print(EM.report(what, other[d], model[d], ref[d]))
        EM.row_check(other[d], model[d], ref[d], what)


def _fault_params():
    out = []
    for case in FAULT_CASES:
        c = L.CASES[case]
        for fold in (False, True):
            for fault in EM.faults_for(c["kind"], c["cfg"], c["B"], c["depth"], fold):
                for family in L.FAMILIES:
                    out.append(pytest.param(case, family, fold, fault, id=f"{case}-{family}-{'folded' if fold else 'separate'}-{fault}"))
    return out


@pytest.mark.parametrize("case,family,fold,fault", _fault_params())
def test_fault_fails_the_check(case, family, fold, fault):
    ref, model = _assert_preconditions(case, family, fold)
    out = L.forward(case, family, q=EM.Fp16(), fold=fold, fault=fault)
    worst, nbad, first = EM.row_check(out, model[-1], ref[-1], raises=False)
    r = EM.row_ratios(out, model[-1], ref[-1])
    print(f"{case} {family} {'folded' if fold else 'separate'} {fault}: worst ratio {worst:.3g} median {float(r.median()):.3g}, "
          f"{nbad} of {r.numel()} rows over the limit, first {first}")
    if (fault, case, family, fold) in INVISIBLE:
        print(f"    (listed as invisible to the check at {INVISIBLE[fault, case, family, fold]:.2f})")
        return
    assert nbad > 0, f"{fault} passes the row check at {case} {family} fold={fold}: worst ratio {worst:.3f}"
    with pytest.raises(AssertionError, match=f"image {first[0]} row {first[1]}"):
        EM.row_check(out, model[-1], ref[-1], fault)


def test_every_fault_is_exercised():
    seen = {p.values[3] for p in _fault_params()}
    assert seen == set(EM.FAULTS)


def test_row_check_locates_one_bad_row():
    """one row of one image moved by 2 x its own model error, the rest exact: the whole-tensor rms ratio stays near zero, the row is named"""
    case = "dino_tiny5"
    ref, model = L.ref(case, "plain")[-1], L.model(case, "plain", False)[0][-1]
    out = model.clone()
    out[1, 7] += 2.0 * (model[1, 7] - ref[1, 7])
    assert float((out - model).pow(2).mean().sqrt() / (model - ref).pow(2).mean().sqrt()) < 0.5
    worst, nbad, first = EM.row_check(out, model, ref, raises=False)
    assert (nbad, first) == (1, (1, 7)) and abs(worst - 2.0) < 1e-9
    out[0, 3, 5] = float("nan")
    assert EM.row_check(out, model, ref, raises=False)[1:] == (2, (0, 3))
