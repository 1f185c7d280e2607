"""oracle/alp_kernels.py (the float64 references of tests/test_alp_kernels_gpu.py) against stock torch and oracle/alp.py, on the CPU.

  values     nearest_resize == F.interpolate(mode='nearest'); bank_ref / sim_ref / pairs_ref / merge_ref == oracle/alp.py evaluated in
             float64 (get_prototypes + cls_unit in all three modes, fewshot_scores, fewshot_scores_multishot) to 1e-11
  bounds     oracle/alp.py in fp32 - honest fp32 arithmetic - stays inside every derived bound on every input the GPU file uses
             (worst ratios printed; recorded in profiles/alp_kernel_tests.txt)
  decisions  every mask is binary and no coverage k / pw^2, k / ks^2 is within 1e-6 of float32(thresh) - except the tie cases, which
             hold exact ties and nothing else near the threshold: no cell of any GPU case is left out of the comparison
  tolerances the derived bounds against test_alp_bank_and_scores' rtol / atol at its four shapes (test_bounds_against_existing_tolerances)
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import alp as oalp
from oracle import alp_kernels as K

MODE_NAME = {0: "mask", 1: "gridconv+", 2: "gridconv"}


def _nchw(tok, h, w):
    return tok.t().reshape(1, -1, h, w)


def _oalp_bank(case, dtype):
    """(bg rows, fg rows, mode) of a bank case through oracle/alp.py's get_prototypes in `dtype`."""
    c = case
    h, w = c["h"], c["w"]
    sup = _nchw(c["sup"].to(dtype), h, w)
    fg = F.interpolate(c["mask"][None, None].to(dtype), size=(h, w), mode="nearest")
    bgm = 1 - c["mask"] if c["bmask"] is None else c["bmask"]
    bg = F.interpolate(bgm[None, None].to(dtype), size=(h, w), mode="nearest")
    kh = (h // c["kernel_size"]) * (w // c["kernel_size"])
    if c["force_mode"] >= 0:
        mode = c["force_mode"]
    elif c["thresh"] == 0.95:
        mode = 1 if kh and oalp.fg_mode_for(fg, c["kernel_size"]) == "gridconv+" else 0
    else:
        mode = 1 if kh and float(F.avg_pool2d(fg, c["kernel_size"]).max()) >= c["thresh"] else 0
    rb = oalp.get_prototypes(sup, bg, "gridconv", c["pool_w"], c["thresh"])
    rf = oalp.get_prototypes(sup, fg, MODE_NAME[mode], c["pool_w"], c["thresh"])
    if mode == 0:
        rf = oalp.safe_norm(rf)
    return rb, rf, mode


def test_nearest_resize_is_interpolate():
    sizes = {(c[7][0], c[0]) for c in K.BANK_CASES.values()} | {(c[7][1], c[1]) for c in K.BANK_CASES.values()}
    sizes |= {(512, 36), (512, 73), (1000, 37), (3, 7), (7, 3), (1023, 1022)} | set(K.SEARCHED)
    for MH, h in sorted(sizes):
        m = torch.arange(MH * 5, dtype=torch.float32).reshape(MH, 5)
        for dt in (torch.float32, torch.float64):
            ref = F.interpolate(m[None, None].to(dt), size=(h, 5), mode="nearest")[0, 0]
            assert torch.equal(K.nearest_resize(m.to(dt), h, 5), ref), (MH, h, dt)


def test_nearest_size_search():
    """Below 1024 there ARE sizes at which floor(dst * float32(MH / h)) in fp32 differs from floor(dst * MH / h): the first in ascending
    (h, MH) is (62, 14) (dst 7 reads row 30, exactly 31), the first with h >= 15 is (150, 18). Bank case 14x18_searched uses both, with
    the mask's edge between the two candidate rows / columns: ATen follows the fp32 rule, and so must the kernel."""
    assert K.search_nearest_pair(1024, 1) == (62, 14, 7)
    assert K.search_nearest_pair(1024, 15)[:2] == (150, 18)
    assert K.SEARCHED == ((62, 14), (150, 18))
    c = K.bank_case("14x18_searched")
    iy, ix = K.nearest_index_exact(14, 62), K.nearest_index_exact(18, 150)
    exact = c["mask"][torch.from_numpy(iy)][:, torch.from_numpy(ix)]
    got = K.nearest_resize(c["mask"], 14, 18)
    assert int((got != exact).sum()) == 9          # row 7 (two pixels) and column 15 (seven)
    assert torch.equal(got, F.interpolate(c["mask"][None, None], size=(14, 18), mode="nearest")[0, 0])


@pytest.mark.parametrize("name", sorted(K.BANK_CASES))
def test_bank_decisions_exact(name):
    c = K.bank_case(name)
    for m in (c["mask"], c["bmask"]):
        assert m is None or bool(((m == 0) | (m == 1)).all())
    r = K.bank_case_ref(c)
    margin, ties = K.decision_margin(r, c["thresh"])
    assert margin > 1e-6, (name, margin)
    assert (ties > 0) == (name in K.TIE_CASES), (name, ties)
    if name in K.TIE_CASES:
        # the tie is the point: fg cells at exactly 3/4 are NOT selected (strict), a 3/4 kernel cell DOES switch the mode (non-strict)
        assert float(np.float32(c["thresh"])) == 0.75 and (r["cover_fg"] == 0.75).sum() == 2 and (r["cover_bg"] == 0.75).sum() == 1
        assert r["cover_fg"].max() == 0.75 and r["meta"] == (13, 1, 1, 0) and (r["slot_fg"] == -1).all()


def test_bank_ref_is_oracle_alp_and_fp32_within_bounds():
    worst = {"cell": 0.0, "global": 0.0}
    for name in sorted(K.BANK_CASES):
        c = K.bank_case(name)
        r = K.bank_case_ref(c)
        rb, rf, mode = _oalp_bank(c, torch.float64)
        assert r["meta"][:3] == (rb.shape[0], rf.shape[0], mode), (name, r["meta"])
        assert (r["rows_bg"] - rb).abs().max().item() < 1e-11 if rb.numel() else True
        assert (r["rows_fg"] - rf).abs().max().item() < 1e-11, name
        rb32, rf32, mode32 = _oalp_bank(c, torch.float32)
        assert mode32 == mode and rb32.shape == rb.shape and rf32.shape == rf.shape
        for got, ref, bound, kinds in ((rb32, r["rows_bg"], r["bound_bg"], ["cell"] * rb.shape[0]), (rf32, r["rows_fg"], r["bound_fg"], r["kinds"])):
            if not got.numel():
                continue
            ratio = ((got.double() - ref).abs() / bound).max(dim=1)[0]
            assert ratio.max().item() <= 1.0, (name, ratio.max().item())
            for k, v in zip(kinds, ratio.tolist()):
                worst[k] = max(worst[k], v)
    print(f"RATIO fp32 torch / bound, bank: pooled rows {worst['cell']:.3f}, global row {worst['global']:.3f}")


def _sim_grid():
    for n in K.SIM_COUNTS:
        for C in K.SIM_C:
            for npix in K.SIM_NPIX:
                yield n, C, npix, "d2"
    for n in K.SIM_D_COUNTS:
        for C in K.SIM_D_C:
            for npix in K.SIM_D_NPIX:
                yield n, C, npix, "d"


def test_sim_ref_is_oracle_alp_and_fp32_within_bounds():
    worst = {"d2": 0.0, "d": 0.0}
    factor = 0.0                 # (sum_i s_i |d_i| + |S|) / (1 + |S|): sim_ref's magnitude for the exp / merge roundings over the issue's
    for n, C, npix, path in _sim_grid():
        nb, nf = K.SIM_BANKS[n]
        q, rb, rf = K.sim_case(nb, nf, C, npix)
        for b in range(q.shape[0]):
            for rows in (rb, rf):
                S, bound = K.sim_ref(q[b], rows, 1e-4, 20.0, path)
                ref64 = oalp.predict(rows.double(), _nchw(q[b].double(), 1, npix), "gridconv")[0, 0, 0]
                assert (S - ref64).abs().max().item() < 1e-11
                d = 20.0 * (q[b].double() @ rows.double().t()) / q[b].double().norm(dim=1).clamp_min(1e-4)[:, None]
                A = (torch.softmax(d, dim=1) * d.abs()).sum(dim=1)
                factor = max(factor, ((A + S.abs()) / (1 + S.abs())).max().item())
                got = oalp.predict(rows, _nchw(q[b], 1, npix), "gridconv")[0, 0, 0]
                ratio = ((got.double() - S).abs() / bound).max().item()
                assert ratio <= 1.0, (n, C, npix, path, ratio)
                worst[path] = max(worst[path], ratio)
    q, banks = K.structured_case()
    for name, rows in banks.items():
        S, bound = K.sim_ref(q[0], rows)
        got = K.sim_fp32(q[0], rows)
        ratio = ((got.double() - S).abs() / bound.clamp_min(1e-300))
        ratio[(got.double() == S)] = 0
        assert ratio.max().item() <= 1.0, (name, ratio)
        worst["d2"] = max(worst["d2"], ratio.max().item())
        assert S[2].item() == 0.0 and got[2].item() == 0.0                       # the all-zero query row
        if name == "same":
            d = 20.0 * (q[0].double() @ rows[0].double()) / q[0].double().norm(dim=1).clamp_min(1e-4)
            assert (S - d).abs().max().item() < 1e-12 and abs(d[3].item() - 0.2) < 1e-6     # row 3: the clamp, d = 20 * 1e-6 / 1e-4
        if name == "anti":
            assert abs(S[0].item() - 20.0) < 1e-6 and abs(S[1].item() - 20.0) < 1e-6
    print(f"RATIO fp32 torch / bound, sim: D2 structure {worst['d2']:.3f}, D + E structure {worst['d']:.3f}")
    print(f"FACTOR (sum s |d| + |S|) / (1 + |S|) over the GPU grid: at most {factor:.2f}")
    assert factor < 2.0
    assert torch.isnan(K.sim_ref(q[0], torch.zeros((0, 64)))[0]).all()


def test_mask_mode_is_one_prototype():
    """cls_unit(mode='mask') == the P = 1 case of the grid path on the normalised global row (csrc/alp.hip's 'mask' mode note)."""
    c = K.bank_case("8x8_pixel")
    r = K.bank_case_ref(c)
    assert r["meta"][2] == 0
    q = K.queries(1, 64, 32, r["rows_fg"].float(), 3)[0]
    fg = K.nearest_resize(c["mask"], 8, 8)[None, None].double()
    ref, _ = oalp.cls_unit(_nchw(q.double(), 8, 8), _nchw(c["sup"].double(), 8, 8), fg, "mask", 0.95, 2)
    S, _ = K.sim_ref(q, r["rows_fg"])
    assert (S - ref.reshape(-1)).abs().max().item() < 1e-11


@pytest.mark.parametrize("name", ["8x8_inside", "8x8_pixel", "7x9", "36x36_c96", "14x18_searched"])
def test_fewshot_scores_is_bank_then_sim(name):
    c = K.bank_case(name)
    assert c["thresh"] == 0.95 and c["bmask"] is None and c["force_mode"] == -1
    h, w, C = c["h"], c["w"], c["C"]
    r = K.bank_case_ref(c)
    q = K.queries(1, h * w, C, r["rows_bg"].float(), 5)[0]
    ref = oalp.fewshot_scores(_nchw(q.double(), h, w), _nchw(c["sup"].double(), h, w), c["mask"][None].double(), c["kernel_size"], c["pool_w"])
    for which, rows in ((0, r["rows_bg"]), (1, r["rows_fg"])):
        S, _ = K.sim_ref(q, rows)
        assert (S - ref[0, which].reshape(-1)).abs().max().item() < 1e-10


def test_multishot_is_merge_and_pairs():
    """Three shots at 8x8, C = 32, in the modes the rule gives them: gridconv+, mask, gridconv+."""
    cases = [K.bank_case(n) for n in ("8x8_inside", "8x8_pixel", "8x8_on_border")]
    refs = [K.bank_case_ref(c) for c in cases]
    assert [c["force_mode"] for c in cases] == [-1] * 3 and [r["meta"][2] for r in refs] == [1, 0, 1]
    q = K.queries(1, 64, 32, refs[0]["rows_bg"].float(), 9)
    sup = torch.cat([_nchw(c["sup"].double(), 8, 8) for c in cases])
    msk = torch.stack([c["mask"] for c in cases]).double()
    ref = oalp.fewshot_scores_multishot(_nchw(q[0].double(), 8, 8), sup, msk, 2, 2)
    bg = K.merge_ref([r["rows_bg"] for r in refs], [r["meta"][0] for r in refs])
    entries = [(bg, 0, 0)] + [(r["rows_fg"], 0, 1) for r in refs]
    S, _ = K.pairs_ref(q, entries, 3)
    assert (S[:2] - ref[0].reshape(2, -1)).abs().max().item() < 1e-10 and torch.isnan(S[2]).all()


def test_bounds_against_existing_tolerances():
    """At the four shapes of test_alp_bank_and_scores (36x36 / 73x73, C = 768, ellipse masks) that test allows rtol 1e-5 / atol 1e-6
    on bank rows and rtol 1e-4 / atol 2e-4 on scores. The derived bounds are WORST-CASE rounding counts:
      pooled rows   are inside that allowance everywhere (largest bound / allowance 0.08): asserted.
      global row    is not: a 16-chain sum of h*w products has a linear worst case, gamma(119) sum|x m| for 36x36 and gamma(435) for 73x73,
                    up to 44 times the allowance (printed); fp32 torch itself uses 0.06 of the bound or less.
      scores        are not: gamma(C + ..) = 8.2e-4 relative to sim_scale sum|q_k p_k| / |q| at C = 768 is up to 3.6 times the allowance
                    (printed). At C = 32 .. 96, where the GPU file does most of its work, the same formula is 10 to 25 times tighter.
    Both shortfalls are recorded here and in the commit; neither bound is narrowed to fit, and the existing test keeps its tolerances."""
    from protosam_amd.synth import ellipse_mask
    worst = {"cell": 0.0, "global": 0.0, "score": 0.0}
    for hw, cover in ((36, "big"), (36, "small"), (36, "tiny"), (73, "big")):
        C, S = 768, 512
        g = torch.Generator().manual_seed(hw)
        sup = torch.randn((hw * hw, C), generator=g)
        qry = torch.randn((2, hw * hw, C), generator=g) + 0.3 * sup[None]
        r = {"big": (0.25, 0.3), "small": (0.09, 0.1), "tiny": (0.03, 0.03)}[cover]
        fg = torch.from_numpy(ellipse_mask(S, 0.5, 0.45, *r)).float()
        ref = K.bank_ref(sup, hw, hw, fg, None, 2, hw // 8, 0.95, 1e-4, -1, (hw // 2) ** 2 + 1)
        margin, ties = K.decision_margin(ref, 0.95)
        assert margin > 1e-6 and ties == 0
        for rows, bound, kinds in ((ref["rows_bg"], ref["bound_bg"], ["cell"] * ref["meta"][0]), (ref["rows_fg"], ref["bound_fg"], ref["kinds"])):
            ratio = (bound / (1e-6 + 1e-5 * rows.abs())).max(dim=1)[0]
            for k, v in zip(kinds, ratio.tolist()):
                worst[k] = max(worst[k], v)
        step = 1 if hw == 36 else 9
        for rows in (ref["rows_bg"], ref["rows_fg"]):
            Sc, bd = K.sim_ref(qry[0, ::step], rows.float())
            worst["score"] = max(worst["score"], (bd / (2e-4 + 1e-4 * Sc.abs())).max().item())
    print(f"BOUND / existing tolerance: pooled rows {worst['cell']:.2f}, global row {worst['global']:.2f}, scores {worst['score']:.2f}")
    assert worst["cell"] <= 1.0
    assert worst["global"] > 1.0 and worst["score"] > 1.0      # the recorded shortfall; if a derivation improves, update the docstring
