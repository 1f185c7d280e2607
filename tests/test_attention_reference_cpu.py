"""CPU: pins oracle/attention.py - the float64 reference, the rounding model, the input constructors and the checks that
tests/test_attention_exact_gpu.py holds the attention kernels to.

  * `reference` against torch's own float64 softmax / matmul (mode 0) and against oracle.sam_image_encoder's
    decomposed_rel_pos_terms / window_partition / window_unpartition (modes 1 / 2), which are pinned to the reference project;
  * at every shape the GPU file uses: the selector margins (>= 32 nats), and the rounding model passing all three checks;
  * faults injected into the float64 arithmetic - a dropped key, the tail tile's phantom keys, swapped weights, a transposed or
    shifted rel-pos gather, rel-pos terms from the scaled q, a pad key read as zeros, a shifted un-partition - each failing its
    check at every shape. Nothing here touches a GPU; the faults never reach a kernel;
  * at the (image, head) counts of tests/test_attention_items_gpu.py (`A.item_shapes_cpu()`, H = 12 and H = 48 among them): the
    constructors' conditions again, and the faults of a wrong ITEM map - an item never run, two heads exchanged, an item computed from
    another image, an item written twice while its successor is skipped - each refused by at least one of the four things that
    file checks: the selectors, constant V, the NaN prefill (what `_finite` inside both checks reports) and the guard rows.
"""
import functools

import pytest
import torch

from oracle import attention as A
from oracle.sam_image_encoder import decomposed_rel_pos_terms, window_partition, window_unpartition

SHAPES = A.shapes()
IDS = [f"mode{m}-N{N}-{gh}x{gw}-hd{hd}" for m, N, gh, gw, hd in SHAPES]


def _rand(shape, std, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * std


# ---- the reference against stock arithmetic -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,H,hd", [(2, 70, 3, 64), (1, 449, 2, 80), (1, 1, 1, 64)])
def test_reference_mode0_matches_torch(B, N, H, hd):
    qkv = _rand((B, N, 3, H, hd), 1.0, 1).half()
    scale = hd ** -0.5
    r = A.reference(qkv, 0, scale=scale)
    q, k, v = qkv.double().permute(2, 0, 3, 1, 4)
    p = ((q * scale) @ k.transpose(-2, -1)).softmax(-1)
    torch.testing.assert_close(r.o, (p @ v).permute(0, 2, 1, 3).reshape(B, N, H * hd), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(r.A, (p @ v.abs()).permute(0, 2, 1, 3).reshape(B, N, H * hd), rtol=1e-12, atol=1e-14)
    ds = 2.0 ** -17 * scale * (q.abs() @ k.abs().transpose(-2, -1)).max(-1).values
    torch.testing.assert_close(r.ds, ds, rtol=1e-12, atol=0)


def _ref_regions(q, k, v, Rh, Rw, side, scale):
    """[Bh, n, hd] float64 regions -> attention with the pinned rel-pos terms."""
    rh, rw = decomposed_rel_pos_terms(q, Rh.double(), Rw.double(), side)
    att = (q * scale) @ k.transpose(-2, -1)
    n = side[0] * side[1]
    att = (att.view(-1, side[0], side[1], side[0], side[1]) + rh[..., :, None] + rw[..., None, :]).view(-1, n, n)
    return att.softmax(-1) @ v


@pytest.mark.parametrize("gh,gw", [(5, 7), (3, 1), (20, 28), (16, 64)])
@pytest.mark.parametrize("hd", [64, 80])
def test_reference_mode1_matches_pinned_relpos(gh, gw, hd):
    B, H, N = 2, 2, gh * gw
    qkv = _rand((B, N, 3, H, hd), 1.0, 2).half()
    Rh, Rw = _rand((2 * gh - 1, hd), 0.3, 3), _rand((2 * gw - 1, hd), 0.3, 4)
    scale = hd ** -0.5
    r = A.reference(qkv, 1, scale=scale, Rh=Rh, Rw=Rw, gh=gh, gw=gw, budget=False)
    q, k, v = qkv.double().permute(2, 0, 3, 1, 4).reshape(3, B * H, N, hd)
    ref = _ref_regions(q, k, v, Rh, Rw, (gh, gw), scale).view(B, H, N, hd).permute(0, 2, 1, 3).reshape(B, N, H * hd)
    torch.testing.assert_close(r.o, ref, rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("gh,gw", [(20, 28), (32, 32), (10, 9), (64, 64)])
def test_reference_mode2_matches_pinned_windows(gh, gw):
    """a ragged 20 x 28 map, 32 x 32 (nine windows, five of them ragged), a map smaller than
    one window, and the 64 x 64 map; the padding is zero in window_partition, so the pad row is subtracted before and added after."""
    B, H, hd, ws = 2, 2, 64, 14
    N, C = gh * gw, H * hd
    qkv = _rand((B, N, 3, H, hd), 1.0, 5).half()
    pad = _rand((3, H, hd), 1.0, 6).half()
    Rh, Rw = _rand((2 * ws - 1, hd), 0.3, 7), _rand((2 * ws - 1, hd), 0.3, 8)
    scale = hd ** -0.5
    r = A.reference(qkv, 2, scale=scale, Rh=Rh, Rw=Rw, pad_row=pad, gh=gh, gw=gw, budget=False)
    padv = pad.double().view(1, 1, 1, 3 * C)
    wins, pad_hw = window_partition(qkv.double().view(B, gh, gw, 3 * C) - padv, ws)
    wins = wins + padv
    nW = wins.shape[0]
    assert nW == B * A.window_tokens(gh, gw).shape[0]
    q, k, v = wins.view(nW, ws * ws, 3, H, hd).permute(2, 0, 3, 1, 4).reshape(3, nW * H, ws * ws, hd)
    o = _ref_regions(q, k, v, Rh, Rw, (ws, ws), scale).view(nW, H, ws, ws, hd).permute(0, 2, 3, 1, 4).reshape(nW, ws, ws, C)
    ref = window_unpartition(o, ws, pad_hw, (gh, gw)).reshape(B, N, C)
    torch.testing.assert_close(r.o, ref, rtol=1e-11, atol=1e-13)


def test_window_tokens_is_window_partition():
    for gh, gw in ((20, 28), (32, 32), (10, 9), (64, 64), (14, 15)):
        ids = torch.arange(gh * gw, dtype=torch.float32).view(1, gh, gw, 1) + 1.0
        wins, _ = window_partition(ids, 14)
        assert torch.equal(A.window_tokens(gh, gw), wins.reshape(-1, 196).long() - 1)


def test_ordinal_counts_fp16_values():
    x = torch.tensor([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 1.0, 1.0 + 2.0 ** -10, -1.0, 65504.0], dtype=torch.float16)
    assert A._ordinal(x).tolist() == [0, 0, 1, -1, 0x3c00, 0x3c01, -0x3c00, 0x7bff]


# ---- at every shape of the GPU file ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bundle(shape):
    """the six inputs of the three families at one image, one head, each with its float64 reference and rounding model."""
    mode, N, gh, gw, hd = shape
    geo = dict(N=N, gh=gh, gw=gw)
    b = {"qk": A.selector_qk(mode, 1, 1, hd, seed=11, **geo)}
    if mode:
        b["rel"] = A.selector_relpos(mode, 1, 1, hd, gh, gw, seed=12)
    b["const"] = A.constant_v(mode, 1, 1, hd, seed=13, **geo)
    b["const_spiky"] = A.constant_v(mode, 1, 1, hd, seed=14, spiky=True, **geo)
    b["diffuse_0.5"] = A.diffuse(mode, 1, 1, hd, std=0.5, seed=15, **geo)
    b["diffuse_1.0"] = A.diffuse(mode, 1, 1, hd, std=1.0, seed=16, **geo)
    for name, case in b.items():
        case.ref = A.reference(case.qkv, mode, budget=name.startswith("diffuse"), model=True, targets=case.targets,
                               **A.ref_kwargs(case))
    return b


def _faulty(case, fault, arg=None):
    """the float64 arithmetic with one fault, rounded to the fp16 a kernel would return."""
    return A.reference(case.qkv, case.mode, budget=False, fault=fault, fault_arg=arg, **A.ref_kwargs(case)).o.half()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_constructors_meet_their_conditions_and_the_model_passes(shape):
    b = _bundle(shape)
    line = []
    for name in ("qk", "rel"):
        if name in b:
            case = b[name]
            margin = A.check_margin(case, case.ref)
            assert A.check_selector(case.ref.model.half(), case) == 0            # the model is bit-equal to the target's v
            line.append(f"{name} margin {margin:.1f} nats")
    for name in ("const", "const_spiky"):
        case = b[name]
        c = case.c
        assert float(c.abs().min()) >= 0.5 and float(c.abs().max()) < 2.0 and bool((c > 0).any() and (c < 0).any())
        assert bool((case.qkv[:, :, 2] == c).all()) and (case.pad_row is None or bool((case.pad_row[2] == c).all()))
        line.append(f"{name} model / bound {A.check_constant_v(case.ref.model.half(), case):.3f}")
    for name in ("diffuse_0.5", "diffuse_1.0"):
        case = b[name]
        mx, rr = A.check_budget(case.ref.model.half(), case, case.ref)
        assert rr == 1.0
        assert torch.equal(A.rounding_model(case.qkv, case.mode, **A.ref_kwargs(case)), case.ref.model)
        line.append(f"{name} model / bound {mx:.3f}")
    print(f"{IDS[SHAPES.index(shape)]}: " + ", ".join(line))


def _must_fail(check, what, *args):
    try:
        check(*args)
    except AssertionError as e:
        return str(e).split(";")[0]
    raise AssertionError(f"{what}: the check passed a faulty result")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_fault_fails_its_check(shape):
    """Each fault against the check meant to see it. (phantom keys: only where the key count is no multiple of 64, i.e. where a
    masked tail tile exists.)"""
    mode, N, gh, gw, hd = shape
    b = _bundle(shape)
    nk = A.n_keys(mode, N)
    sid = IDS[SHAPES.index(shape)]
    caught = []

    def run(fault, arg, case_name, check, *extra):
        case = b[case_name]
        msg = _must_fail(check, f"{sid} {fault} {arg}", _faulty(case, fault, arg), case, *extra)
        caught.append(f"  {fault}{'' if arg is None else ' ' + str(arg)} [{case_name}]: {msg}")

    swap = (1 % nk, (nk // 2 + 1) % nk)
    if nk > 1:
        for j in sorted({0, nk // 2, nk - 1}):
            run("drop_key", j, "qk", A.check_selector)
        if swap[0] != swap[1]:
            run("swap_keys", swap, "qk", A.check_selector)
            run("swap_keys", swap, "diffuse_0.5", A.check_budget, b["diffuse_0.5"].ref)
        run("drop_key", nk - 1, "diffuse_0.5", A.check_budget, b["diffuse_0.5"].ref)
    if A.phantom_count(nk):
        run("phantom_tail", None, "const", A.check_constant_v)
        run("phantom_tail", None, "diffuse_0.5", A.check_budget, b["diffuse_0.5"].ref)
    if mode:
        run("relh_transposed", None, "rel", A.check_selector)
        run("rel_row_off_by_one", None, "rel", A.check_selector)
        run("rel_scaled_q", None, "diffuse_1.0", A.check_budget, b["diffuse_1.0"].ref)
    if mode == 2:
        run("pad_key_zero", None, "const", A.check_constant_v)
        run("unpartition_shift", None, "qk", A.check_selector)
    print(f"{sid}: {len(caught)} injected faults, every one caught\n" + "\n".join(caught))


@pytest.mark.parametrize("N,hd,std", [(1297, 64, 0.5), (1301, 64, 0.5)])
def test_faults_the_old_tolerance_passes(N, hd, std):
    """What rtol = atol = 2e-3 lets through and the rms criterion does not: the last key dropped, and the tail tile's phantoms, stay
    inside 2e-3 on (nearly) every element while their rms error is far more than 3 x the rounding model's."""
    case = A.diffuse(0, 1, 1, hd, N=N, std=std, seed=21)
    ref = A.reference(case.qkv, 0, model=True)
    mdl = float((ref.model - ref.o).pow(2).mean().sqrt())
    for fault, arg in (("drop_key", N - 1), ("phantom_tail", None)):
        bad = _faulty(case, fault, arg)
        err = (bad.double() - ref.o).abs()
        rms = float(err.pow(2).mean().sqrt())
        inside = float((err <= 2e-3 + 2e-3 * ref.o.abs()).double().mean())
        print(f"N={N} std {std} {fault}: rms {rms:.2e} = {rms / mdl:.0f} x the model's {mdl:.2e}; {100 * inside:.2f} % of the "
              f"elements inside 2e-3")
        assert inside > 0.98 and rms > 35 * mdl
        with pytest.raises(AssertionError):
            A.check_budget(bad, case, ref)


# ---- item maps: the sweeps of tests/test_attention_items_gpu.py -----------------------------------------------------------------
ITEM_SHAPES = A.item_shapes_cpu()
ITEM_IDS = [f"mode{m}-B{B}-H{H}-hd{hd}-N{N}-{gh}x{gw}" for m, B, H, hd, N, gh, gw, _ in ITEM_SHAPES]


@functools.lru_cache(maxsize=None)
def _item_bundle(shape):
    """the selector and constant-V inputs of the item sweep at the sweep's own (B, H), each with its float64 reference and model."""
    mode, B, H, hd, N, gh, gw, _ = shape
    geo = dict(N=N, gh=gh, gw=gw)
    b = {"qk": A.selector_qk(mode, B, H, hd, seed=31, **geo)}
    if mode:
        b["rel"] = A.selector_relpos(mode, B, H, hd, gh, gw, seed=32)
    b["const"] = A.constant_v(mode, B, H, hd, seed=33, **geo)
    for name, case in b.items():
        case.ref = A.reference(case.qkv, mode, budget=False, model=True, targets=case.targets, **A.ref_kwargs(case))
    return b


@pytest.mark.parametrize("shape", ITEM_SHAPES, ids=ITEM_IDS)
def test_item_sweep_constructors_meet_their_conditions_and_the_model_passes(shape):
    b = _item_bundle(shape)
    line = []
    for name in ("qk", "rel"):
        if name in b:
            margin = A.check_margin(b[name], b[name].ref)
            assert A.check_selector(b[name].ref.model.half(), b[name]) == 0
            line.append(f"{name} margin {margin:.1f} nats")
    line.append(f"const model / bound {A.check_constant_v(b['const'].ref.model.half(), b['const']):.3f}")
    c = b["const"].c
    assert c.shape[0] == 1 or len({tuple(r.tolist()) for r in c}) == c.shape[0]       # one c per head, no two alike
    print(f"{ITEM_IDS[ITEM_SHAPES.index(shape)]}: " + ", ".join(line))


def _refusals(buf, case, check, B):
    """which of the item tests' checks refuse this buffer: the family's own check (a NaN it meets is the prefill) and the guard."""
    seen = []
    try:
        check(buf[:B].contiguous(), case)
    except AssertionError as e:
        seen.append("NaN prefill" if "not finite" in str(e) else check.__name__)
    try:
        A.check_guard(buf, B)
    except AssertionError:
        seen.append("guard rows")
    return seen


@pytest.mark.parametrize("shape", ITEM_SHAPES, ids=ITEM_IDS)
def test_every_item_fault_is_refused(shape):
    """Each item fault at the first, a middle and the last item: the selector refuses every one of them (by the NaN it meets for
    a dropped item, by the guard rows too for the repeat of the very last item); constant V, whose c differs between heads only,
    refuses what moves a result to another head or leaves the prefill, and is blind to `wrong_image` and to a repeat inside one
    head - recorded below per fault, asserted for the selector."""
    mode, B, H, hd, N, gh, gw, rows = shape
    b = _item_bundle(shape)
    slots = A.item_slots(mode, N, gh, gw, rows or 256)
    R = slots.shape[0]
    sid = ITEM_IDS[ITEM_SHAPES.index(shape)]
    places = sorted({(0, 0, 0), (B // 2, H // 2, R // 2), (B - 1, H - 1, R - 1), (0, H - 1, R - 1)})
    faults = [("drop_item", p) for p in places] + [("repeat_item_skip_next", p) for p in places]
    if H > 1:
        faults += [("swap_heads", (B - 1, 0, H - 1)), ("swap_heads", (0, H // 2, H // 2 - 1))]
    if B > 1:
        faults += [("wrong_image", (0, H - 1, B - 1)), ("wrong_image", (B - 1, 0, B - 2))]
    lines = []
    for fault, arg in faults:
        seen = {}
        for name, check in (("qk", A.check_selector), ("rel", A.check_selector), ("const", A.check_constant_v)):
            if name not in b:
                continue
            case = b[name]
            clean = case.ref.model.half()
            buf = A.item_fault(clean, fault, arg, slots, mode, H, hd, 1)
            assert fault in ("drop_item", "repeat_item_skip_next") or not bool(buf[:B].isnan().any())   # (the others leave no prefill)
            seen[name] = _refusals(buf, case, check, B)
        assert seen["qk"], f"{sid} {fault} {arg}: the QK selector passed a misplaced item"
        assert "rel" not in seen or seen["rel"], f"{sid} {fault} {arg}: the rel-pos selector passed a misplaced item"
        if fault == "drop_item":
            assert all("NaN prefill" in v for v in seen.values()), (sid, fault, arg, seen)
        if fault == "swap_heads":
            assert seen["const"] == ["check_constant_v"], (sid, fault, arg, seen)
        if fault == "repeat_item_skip_next" and arg == (B - 1, H - 1, R - 1):
            assert all("guard rows" in v for v in seen.values()), (sid, fault, arg, seen)
        lines.append(f"  {fault} {arg}: " + "; ".join(f"{k}: {', '.join(v) or 'passes (blind)'}" for k, v in seen.items()))
    print(f"{sid}: {len(faults)} item faults, every one refused\n" + "\n".join(lines))


def test_item_faults_through_reference():
    """`reference(fault=...)` places the same faults: one small shape per mode, against `item_fault` on the sound result."""
    for mode, geo in ((0, dict(N=200)), (2, dict(gh=20, gw=20))):
        case = A.selector_qk(mode, 2, 3, 64, seed=41, **geo)
        kw = dict(budget=False, item_rows=128, **A.ref_kwargs(case))
        sound = A.reference(case.qkv, mode, **kw).o
        slots = A.item_slots(mode, case.N, case.gh, case.gw, 128)
        for fault, arg in (("drop_item", (1, 2, 1)), ("swap_heads", (0, 0, 2)), ("wrong_image", (1, 1, 0)),
                           ("repeat_item_skip_next", (1, 2, slots.shape[0] - 1))):
            got = A.reference(case.qkv, mode, fault=fault, fault_arg=arg, guard=1, **kw).o
            want = A.item_fault(sound, fault, arg, slots, mode, 3, 64, 1)
            assert got.shape == (3, case.N, 3 * 64) and torch.equal(got.isnan(), want.isnan())
            assert torch.equal(got.nan_to_num(0.0), want.nan_to_num(0.0))
            assert not torch.equal(got.nan_to_num(0.0), torch.cat([sound, torch.zeros_like(sound[:1])]))      # (the fault did something)
