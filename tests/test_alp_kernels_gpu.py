"""GPU parity of the ALP prototype kernels of csrc/alp.hip - psam_alp_bank, psam_alp_sim (kernel D2, D2 + E and the 64-prototype
fallback D + E), psam_alp_sim_pairs - and MultiProtoAsConv.merge_banks, one at a time, against the float64 references of
oracle/alp_kernels.py.

House rules (as in test_mask_kernels_gpu.py): every output (bank, meta, slots, pred, part) is filled with NaN or a sentinel before the
call; values are compared element-wise under the reference's own derived bound (rounding counts, oracle/alp_kernels.py), decisions
(counts, mode, slots) exactly - tests/test_alp_reference_cpu.py shows on the CPU that no input has a coverage within 1e-6 of its
threshold except the exact ties, and that fp32 torch stays inside every bound. Banks for the similarity kernels are filled by hand,
with 7.0 in the first row past each count, NaN in every later row and in every padding column of the queries, so a read past an edge
poisons the result. NaN rows alone would not: the kernels' softmax drops a NaN logit (fmaxf returns the other operand, `d > -inf` is
false), so a prototype-count bug that lets row n through is invisible when row n is NaN - hence the finite 7.0, whose logit cannot be
dropped. The same holds for the bank that merge_banks returns, which is zero, not NaN, past its total: a zero row gives a logit of 0,
which moves the score and is caught by the float64 comparison, not by a NaN.
Shapes are the smallest that reach each edge: prototype groups of 96 (n = 1 .. 193), K stages C = 32 / 64 / 96, pixel tiles of 32 / 128.

Every comparison prints a RATIO line; the module prints the worst ratio per kernel and path (PATH lines) when it ends. Both, as
measured on an MI355X, are in profiles/alp_kernel_tests.txt.
"""
import numpy as np
import pytest
import torch

from oracle import alp_kernels as K

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -1515870811
EPS, SCALE = 1e-4, 20.0
POISON = 7.0
_PATHS = {}                       # kernel and path -> worst |err| / bound over the module's comparisons


@pytest.fixture(scope="module", autouse=True)
def _print_paths():
    yield
    for key in sorted(_PATHS):
        print(f"\nPATH {key}: worst |err| / bound {_PATHS[key]:.3f}", end="")
    print()


def _within(out, ref, bound, what, path):
    """out == ref within bound element-wise, NaN exactly where ref is NaN; prints and returns the worst |err| / bound, and keeps the
    largest per `path` (the kernel and code path the comparison went through) for the module's PATH lines."""
    out = out.detach().double().cpu().reshape(ref.shape)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(out), nan), f"{what}: NaN at {int((torch.isnan(out) != nan).sum())} wrong places (unwritten / poisoned?)"
    err = (out - ref).abs()[~nan]
    bd = bound[~nan]
    if not err.numel():
        return 0.0
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bd.clamp_min(1e-300))
    worst = ratio.max().item()
    print(f"RATIO {what}: worst |err| / bound {worst:.3f}")
    _PATHS[path] = max(_PATHS.get(path, 0.0), worst)
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} elements outside the bound, worst {worst:.3f} (|err| {err[ratio.argmax()].item():.3e})"
    return worst


def _hand_bank(dev, cap, C, rows_bg, rows_fg, mode=1):
    from protosam_amd import ops
    bk = ops.AlpBank(cap - 1, C, dev)
    bk.bank.fill_(NAN)
    nb, nf = rows_bg.shape[0], rows_fg.shape[0]
    assert nb <= cap and nf <= cap
    bk.bank[:nb] = rows_bg.to(dev)
    bk.bank[cap:cap + nf] = rows_fg.to(dev)
    # the first row past each count is finite: the softmax skips a NaN logit (fmaxf, `d > -inf`), a logit of 20 * 7 * sum(q) / |q| it cannot
    if nb < cap:
        bk.bank[nb] = POISON
    if nf < cap:
        bk.bank[cap + nf] = POISON
    bk.meta.copy_(torch.tensor([nb, nf, mode, max(nf - 1, 0), SENT, SENT, SENT, SENT], dtype=torch.int32))
    return bk


def _strided(q, ld, extra, dev):
    """q [B, npix, C] -> (flat NaN-padded device buffer with row stride ld and batch stride npix * ld + extra, that batch stride)."""
    B, npix, C = q.shape
    bs = npix * ld + extra
    buf = torch.full((B * bs,), NAN)
    for b in range(B):
        buf[b * bs:b * bs + npix * ld].view(npix, ld)[:, :C] = q[b]
    return buf.to(dev), bs


def _sim(dev, q, bank, ld, extra, which_only=-1):
    """-> (pred [B, 2, npix], part [2B, ceil(cap / 64), npix_pad, 3]), both pre-filled with NaN."""
    from protosam_amd import ops
    B, npix, C = q.shape
    buf, bs = _strided(q, ld, extra, dev)
    npix_pad = (npix + 63) // 64 * 64
    part = torch.full((2 * B, (bank.cap + 63) // 64, npix_pad, 3), NAN, device=dev)
    pred = torch.full((B, 2, npix), NAN, device=dev)
    ops.alp_sim(buf, bs, ld, B, npix, C, bank, pred=pred, part=part, eps=EPS, sim_scale=SCALE, which_only=which_only)
    torch.cuda.synchronize()
    return pred, part


def _sim_path(path, cap):
    """The code path psam_alp_sim takes: kernel D + E when ld % 4 != 0, else kernel D2, alone for one group of 96, with E for more."""
    return "sim D + E" if path == "d" else "sim D2 direct" if cap <= 96 else "sim D2 + E"


def _sim_check(dev, q, rb, rf, cap, ld_extra, path, what, which_only=-1):
    B, npix, C = q.shape
    bank = _hand_bank(dev, cap, C, rb, rf)
    pred, part = _sim(dev, q, bank, C + ld_extra, 8, which_only)
    ref = torch.full((B, 2, npix), NAN, dtype=torch.float64)
    bound = torch.zeros((B, 2, npix), dtype=torch.float64)
    for b in range(B):
        for which, rows in ((0, rb), (1, rf)):
            if which_only in (-1, which):
                ref[b, which], bound[b, which] = K.sim_ref(q[b], rows, EPS, SCALE, path)
    worst = _within(pred, ref, bound, what, _sim_path(path, cap))
    # the padding columns of `part` (pixels npix .. npix_pad - 1) belong to no pixel: never written
    assert bool(torch.isnan(part[:, :, npix:]).all()), f"{what}: part written past pixel {npix}"
    return worst


# ---- 1. psam_alp_bank ---------------------------------------------------------------------------------------------------------
def _run_bank(dev, c, cap=None):
    from protosam_amd import ops
    h, w, C, ld = c["h"], c["w"], c["C"], c["ld"]
    npx = h * w
    ncell = (h // c["pool_w"]) * (w // c["pool_w"])
    bk = ops.AlpBank((cap or ncell + 1) - 1, C, dev)
    bk.bank.fill_(NAN)
    bk.meta.fill_(SENT)
    bk.slot_bg = torch.full((ncell,), SENT, dtype=torch.int32, device=dev)
    bk.slot_fg = torch.full((ncell,), SENT, dtype=torch.int32, device=dev)
    off = 1 if c["misaligned"] else 0
    flat = torch.full((npx * ld + 1,), NAN)
    flat[off:off + npx * ld].view(npx, ld)[:, :C] = c["sup"]
    flat = flat.to(dev)
    sup = flat[off:off + npx * ld].view(npx, ld)[:, :C]
    assert sup.data_ptr() % 16 == (4 if off else 0)
    bm = None if c["bmask"] is None else c["bmask"].to(dev).contiguous()
    ops.alp_bank(sup, ld, h, w, C, c["mask"].to(dev).contiguous(), c["pool_w"], c["kernel_size"], c["thresh"], c["eps"], bank=bk,
                 force_mode=c["force_mode"], bmask=bm)
    torch.cuda.synchronize()
    return bk


@pytest.mark.parametrize("name", sorted(K.BANK_CASES))
def test_alp_bank(dev, name):
    """meta[0..3] and both slot arrays exact, occupied rows within the derived bound (pooled rows: gamma(pw^2) and the normalisation;
    the global row: the 16-chain sum scaled by sum |x m|), every row at or past the count in both halves still NaN, meta[4..7]
    untouched. The cases (oracle.alp_kernels.BANK_CASES): h != w, trailing rows / columns, pool_w 2 / 4 / h, more than 256 cells
    (73x73: six cells per thread), C 32 .. 768, ld = C, C + 4, C + 1 (scalar global row), a 4-byte-offset view, masks of 8x8 .. 512x512
    and 100x130 and the sizes at which the fp32 nearest index differs from the exact one, all ones / zeros / one pixel, an explicit
    bmask, force_mode 0 / 1 / 2, and thresh = 0.75 against coverages of exactly 3/4 (cells not selected, mode switched)."""
    c = K.bank_case(name)
    r = K.bank_case_ref(c)
    bk = _run_bank(dev, c)
    cap = bk.cap
    meta = bk.meta.cpu().tolist()
    assert tuple(meta[:4]) == r["meta"], (meta, r["meta"])
    assert meta[4:] == [SENT] * 4
    assert np.array_equal(bk.slot_bg.cpu().numpy(), r["slot_bg"]) and np.array_equal(bk.slot_fg.cpu().numpy(), r["slot_fg"])
    nb, nf = r["meta"][:2]
    bank = bk.bank.cpu()
    assert bool(torch.isnan(bank[nb:cap]).all()) and bool(torch.isnan(bank[cap + nf:]).all()), "a row at or past the count was written"
    if nb:
        _within(bank[:nb], r["rows_bg"], r["bound_bg"], f"bank {name} bg pooled rows", "bank pooled rows")
    ncf = r["meta"][3]
    if ncf:
        _within(bank[cap:cap + ncf], r["rows_fg"][:ncf], r["bound_fg"][:ncf], f"bank {name} fg pooled rows", "bank pooled rows")
    if r["meta"][2] != 2:
        f4 = c["C"] % 256 == 0 and c["ld"] % 4 == 0 and not c["misaligned"]
        kind = f"global row ({'float4' if f4 else 'scalar'})"
        _within(bank[cap + ncf], r["rows_fg"][ncf], r["bound_fg"][ncf], f"bank {name} {kind}", f"bank {kind}")
    if name == "8x8_force0":
        assert nf == 1
    if name == "8x8_force2":
        assert nf == ncf == 4 and r["kinds"] == ["cell"] * 4
    if name in K.TIE_CASES:
        assert (nb, nf, meta[2]) == (13, 1, 1)


def test_alp_bank_spare_capacity(dev):
    """cap larger than ncell + 1: the fg half starts at row cap, and nothing else moves."""
    c = K.bank_case("8x8_on_border")
    r = K.bank_case_ref(c, cap=40)
    bk = _run_bank(dev, c, cap=40)
    nb, nf = r["meta"][:2]
    bank = bk.bank.cpu()
    assert bk.cap == 40 and tuple(bk.meta.cpu().tolist()[:4]) == r["meta"]
    assert bool(torch.isnan(bank[nb:40]).all()) and bool(torch.isnan(bank[40 + nf:]).all())
    _within(bank[:nb], r["rows_bg"], r["bound_bg"], "bank spare capacity bg", "bank pooled rows")
    ncf = r["meta"][3]
    assert r["kinds"] == ["cell"] * ncf + ["global"] and nf == ncf + 1
    _within(bank[40:40 + ncf], r["rows_fg"][:ncf], r["bound_fg"][:ncf], "bank spare capacity fg", "bank pooled rows")
    _within(bank[40 + ncf], r["rows_fg"][ncf], r["bound_fg"][ncf], "bank spare capacity global row", "bank global row (scalar)")


def test_alp_bank_rejections(dev):
    from protosam_amd import _lib
    L = _lib.lib()
    h = w = 8
    C, pw, ks = 32, 2, 2
    ncell, cap = 16, 17
    sup = torch.randn((h * w, C), device=dev)
    mask = torch.ones((h, w), device=dev)
    bank = torch.full((2 * cap, C), NAN, device=dev)
    meta = torch.full((8,), SENT, dtype=torch.int32, device=dev)
    sb = torch.full((ncell,), SENT, dtype=torch.int32, device=dev)
    sf = torch.full((ncell,), SENT, dtype=torch.int32, device=dev)
    mres = torch.full((2 * h * w,), NAN, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def call(h=h, w=w, C=C, pw=pw, ks=ks, cap=cap):
        return L.psam_alp_bank(sup.data_ptr(), C, h, w, C, mask.data_ptr(), 0, 8, 8, pw, ks, 0.95, 1e-4, bank.data_ptr(), cap,
                               meta.data_ptr(), sb.data_ptr(), sf.data_ptr(), mres.data_ptr(), -1, st)
    for kw in (dict(h=0), dict(h=-8), dict(w=0), dict(C=0), dict(C=-32), dict(pw=0), dict(pw=-2), dict(ks=0), dict(ks=-1), dict(cap=1),
               dict(cap=0), dict(cap=16)):
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(bank).all()) and bool(torch.isnan(mres).all())
    assert bool((meta == SENT).all()) and bool((sb == SENT).all()) and bool((sf == SENT).all())
    assert call() == 0                   # (the accepted call, so that the refusals above are refusals of their argument)
    torch.cuda.synchronize()
    assert int(meta[1]) == 17


# ---- 2. psam_alp_sim ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", K.SIM_COUNTS)
def test_alp_sim_groups(dev, n):
    """Kernel D2 (and E when cap > 96): count n in one half, another count in the other (oracle.alp_kernels.SIM_BANKS), cap = n + 1,
    C = 32 (one K stage) / 64 (two) / 96 (three: the odd tail of the loop unrolled by two) / 768, npix 1 .. 200 around the 32-pixel
    strips and 128-pixel tiles, B = 2, ld = C + 4, batch stride npix * ld + 8. n = 96 leaves the second launched group empty."""
    nb, nf = K.SIM_BANKS[n]
    worst = 0.0
    for C in K.SIM_C:
        for npix in K.SIM_NPIX:
            q, rb, rf = K.sim_case(nb, nf, C, npix)
            worst = max(worst, _sim_check(dev, q, rb, rf, n + 1, 4, "d2", f"sim {'D2' if n + 1 <= 96 else 'D2+E'} n={nb}/{nf} C={C} npix={npix}"))
    print(f"WORST sim {'D2 direct' if n + 1 <= 96 else 'D2 + E'} n={n}: {worst:.3f}")


def test_alp_sim_sparse_bank(dev):
    """cap = 300 with 5 / 3 prototypes: groups 1 .. 3 of the launch are empty."""
    for C, npix in ((32, 33), (96, 129)):
        q, rb, rf = K.sim_case(5, 3, C, npix)
        _sim_check(dev, q, rb, rf, 300, 4, "d2", f"sim D2+E cap=300 n=5/3 C={C} npix={npix}")


@pytest.mark.parametrize("path", ["d2", "d"])
@pytest.mark.parametrize("which_only", [0, 1])
def test_alp_sim_which_only(dev, path, which_only):
    for n in (33, 97):
        nb, nf = K.SIM_BANKS[n]
        q, rb, rf = K.sim_case(nb, nf, 64, 129)
        _sim_check(dev, q, rb, rf, n + 1, 4 if path == "d2" else 1, path, f"sim {path} which_only={which_only} n={n}", which_only)


@pytest.mark.parametrize("n", K.SIM_D_COUNTS)
def test_alp_sim_fallback(dev, n):
    """ld = C + 1: no float4 loads, so psam_alp_sim runs kernel D (prototype tiles of 64, pixel tiles of 64) and kernel E. The padding
    columns of `part` stay NaN (kernel D's `x0 + t < npix` guard)."""
    nb, nf = K.SIM_BANKS[n]
    worst = 0.0
    for C in K.SIM_D_C:
        for npix in K.SIM_D_NPIX:
            q, rb, rf = K.sim_case(nb, nf, C, npix)
            worst = max(worst, _sim_check(dev, q, rb, rf, n + 1, 1, "d", f"sim D+E n={nb}/{nf} C={C} npix={npix}"))
    print(f"WORST sim D + E n={n}: {worst:.3f}")


@pytest.mark.parametrize("path", ["d2", "d"])
def test_alp_sim_structured(dev, path):
    """Rows with known answers (oracle.alp_kernels.structured_case): identical prototypes (S = d), one prototype along the query among
    96 against it (S ~ 20, logits 20 and -20 in one softmax), duplicates, an all-zero query (S = 0 exactly), a query of norm 1e-6 (the
    eps clamp: d = sim_scale q.p / eps = 0.2), +-1 / +-1/2 entries (exact dot products)."""
    q, banks = K.structured_case(64)
    for name, rows in banks.items():
        n = rows.shape[0]
        bank = _hand_bank(dev, n + 1, 64, rows, rows[:1])
        pred, _ = _sim(dev, q, bank, 64 + (4 if path == "d2" else 1), 8)
        S, bound = K.sim_ref(q[0], rows, EPS, SCALE, path)
        _within(pred[0, 0], S, bound, f"sim {path} structured '{name}'", _sim_path(path, n + 1))
        out = pred[0, 0].double().cpu()
        assert out[2].item() == 0.0
        if name == "same":
            assert abs(out[3].item() - 0.2) < 1e-5 and abs(out[0].item() - 20.0) < 1e-4 and abs(out[1].item() + 20.0) < 1e-4
        if name == "anti":
            assert abs(out[0].item() - 20.0) < 1e-4 and abs(out[1].item() - 20.0) < 1e-4 and abs(out[6].item() - 20.0) < 1e-4
        if name == "pm":
            # row 4 = (1, -1, 1, 1, 0 ..), |q| = 2: d_i = 10 * (q.p_i), q.p_i in {-2, -1, 0, 1, 2}; the fp32 kernel has the d_i exactly
            d = 10.0 * (q[0, 4].double() @ rows.double().t())
            s = torch.softmax(d, 0)
            assert abs(out[4].item() - (s * d).sum().item()) < 2e-5


@pytest.mark.parametrize("path", ["d2", "d"])
@pytest.mark.parametrize("cap", [6, 200])
def test_alp_sim_empty_bank(dev, path, cap):
    """A bank half with no prototype: every pixel of its plane is NaN (0 / 0, as csrc/alp.hip's comment in kernel E says), the other
    plane is right; both halves in turn."""
    q, rb, rf = K.sim_case(5, 3, 32, 70)
    empty = torch.zeros((0, 32))
    for a, b in ((empty, rf), (rb, empty)):
        _sim_check(dev, q, a, b, cap, 4 if path == "d2" else 1, path, f"sim {path} empty half cap={cap} n={a.shape[0]}/{b.shape[0]}")


def test_alp_sim_rejections(dev):
    from protosam_amd import _lib
    L = _lib.lib()
    C, npix, cap = 32, 16, 4
    q = torch.randn((npix, C), device=dev)
    bank = _hand_bank(dev, cap, C, K.unit_rows(2, C, 0), K.unit_rows(2, C, 1))
    part = torch.full((2 * 64 * 3,), NAN, device=dev)
    pred = torch.full((2, npix), NAN, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def call(C=C, B=1, npix=npix, cap=cap):
        return L.psam_alp_sim(q.data_ptr(), npix * 32, 32, B, npix, C, bank.bank.data_ptr(), cap, bank.meta.data_ptr(), 1e-4, 20.0,
                              part.data_ptr(), pred.data_ptr(), -1, st)
    for kw in (dict(C=31), dict(C=16), dict(C=0 + 8), dict(B=0), dict(B=-1), dict(npix=0), dict(npix=-4), dict(cap=1), dict(cap=0)):
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(pred).all()) and bool(torch.isnan(part).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(pred).all())


# ---- 3. psam_alp_sim_pairs and merge_banks -------------------------------------------------------------------------------------
def _pairs_banks(dev, C):
    """Hand-filled banks: 0: cap 9 (7 / 5); 1: cap 200 (150 / 101); 2: cap 97 (96 / 40: its second group is empty); 3: cap 9 (3 / 8)."""
    spec = [(9, 7, 5), (200, 150, 101), (97, 96, 40), (9, 3, 8)]
    rows = [(K.unit_rows(nb, C, 10 + i), K.unit_rows(nf, C, 20 + i)) for i, (_, nb, nf) in enumerate(spec)]
    return [_hand_bank(dev, cap, C, rb, rf) for (cap, _, _), (rb, rf) in zip(spec, rows)], rows


@pytest.mark.parametrize("C,npix", [(96, 33), (32, 200)])
def test_alp_sim_pairs(dev, C, npix):
    """One table with a direct plane (one entry, cap 9), a merged plane (cap 200), a three-shot foreground plane over banks of
    capacities 9, 97 and 200 (max_groups = 3 is more than the first two need), a bank used by two slices and a merged plane whose bank
    holds cap - 1 = 96 prototypes (its second group is empty); planes 3 and 6 are not named and stay NaN. Against pairs_ref in float64 and, bit for bit, against psam_alp_sim per entry with fmax over the shots.
    Then a table whose entries are all direct (no `part`)."""
    from protosam_amd import ops
    B = 2
    banks, rows = _pairs_banks(dev, C)
    q = K.queries(B, npix, C, torch.cat([rows[1][0], rows[0][1], rows[2][1], rows[1][1]]), 77)
    buf, bs = _strided(q, C + 4, 8, dev)
    # (bank, slice, which, plane)
    entries = [(0, 0, 0, 0), (1, 0, 0, 1), (0, 1, 1, 2), (2, 1, 1, 2), (1, 1, 1, 2), (1, 1, 0, 4), (3, 0, 1, 5), (0, 1, 0, 7), (2, 0, 0, 8)]
    n_planes = 9
    pred = torch.full((n_planes, npix), NAN, device=dev)
    # `part` as the wrapper lays it out, [entry, group of max_groups, npix_pad, 3], NaN: a merge that reads a group its entry did not
    # write (only the cap-200 bank fills all max_groups = 3) gives NaN, where fresh memory could hold zeros, which leave W / Z alone
    ngmax = max((banks[k].cap + 95) // 96 for k, _, _, _ in entries)
    npix_pad = (npix + 63) // 64 * 64
    assert ngmax == 3
    part = torch.full((len(entries), ngmax, npix_pad, 3), NAN, device=dev)
    ops.alp_sim_pairs(buf, bs, C + 4, B, npix, C, banks, entries, n_planes, pred=pred, part=part, eps=EPS, sim_scale=SCALE)
    torch.cuda.synchronize()
    ref, bound = K.pairs_ref(q, [(rows[k][which], b, plane) for k, b, which, plane in entries], n_planes, EPS, SCALE)
    assert bool(torch.isnan(ref[3]).all()) and bool(torch.isnan(ref[6]).all())
    _within(pred, ref, bound, f"pairs mixed table C={C} npix={npix}", "pairs")
    # what of `part` was written: a direct entry (its plane's only one, cap <= 96) nothing, any other its max(1, ceil(n / 96)) groups
    # of pixels 0 .. npix - 1; the groups past that and the padding columns npix .. npix_pad - 1 are still NaN
    written = []
    for e, (k, b, which, plane) in enumerate(entries):
        direct = sum(pl == plane for _, _, _, pl in entries) == 1 and banks[k].cap <= 96
        ng = 0 if direct else max(1, (rows[k][which].shape[0] + 95) // 96)
        written.append(ng)
        assert bool(torch.isfinite(part[e, :ng, :npix]).all()), f"pairs entry {e}: a group it owns is not written"
        assert bool(torch.isnan(part[e, ng:]).all()), f"pairs entry {e}: part written past its {ng} groups"
        assert bool(torch.isnan(part[e, :, npix:]).all()), f"pairs entry {e}: part written past pixel {npix}"
    assert written == [0, 2, 1, 1, 2, 2, 0, 0, 1]
    # the three shots do not agree on the maximum everywhere: the shot maximum is exercised
    shots = torch.stack([K.sim_ref(q[1], rows[k][1], EPS, SCALE)[0] for k in (0, 2, 1)])
    assert len(set(shots.argmax(dim=0).tolist())) >= 2
    same = torch.full_like(pred, NAN)
    seen = set()
    for k, b, which, plane in entries:
        r = _sim(dev, q[b:b + 1], banks[k], C + 4, 8)[0][0, which]
        same[plane] = r if plane not in seen else torch.fmax(same[plane], r)
        seen.add(plane)
    assert torch.equal(torch.nan_to_num(pred, nan=-7.0), torch.nan_to_num(same, nan=-7.0)), "pairs is not bit-identical to psam_alp_sim"
    # every entry direct: part is NULL
    entries = [(0, 0, 0, 0), (3, 1, 1, 1), (0, 1, 1, 3), (3, 0, 0, 4)]
    pred = torch.full((5, npix), NAN, device=dev)
    ops.alp_sim_pairs(buf, bs, C + 4, B, npix, C, banks, entries, 5, pred=pred, eps=EPS, sim_scale=SCALE)
    torch.cuda.synchronize()
    ref, bound = K.pairs_ref(q, [(rows[k][which], b, plane) for k, b, which, plane in entries], 5, EPS, SCALE)
    _within(pred, ref, bound, f"pairs all-direct table C={C} npix={npix}", "pairs")


def test_alp_sim_pairs_rejections(dev):
    from protosam_amd import _lib
    L = _lib.lib()
    C, npix = 32, 16
    banks, _ = _pairs_banks(dev, C)
    q = torch.randn((npix * 36 + 4,), device=dev)
    tab = torch.tensor([[banks[0].bank.data_ptr(), banks[0].meta.data_ptr(), 9 | (0 << 32), (0 | 2) | (0 << 32)]], dtype=torch.int64).to(dev)
    pred = torch.full((1, npix), NAN, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def call(qp=q.data_ptr(), ld=36, tabp=tab.data_ptr(), ne=1, predp=pred.data_ptr(), C=C, bs=npix * 36, mg=1):
        return L.psam_alp_sim_pairs(qp, bs, ld, npix, C, tabp, ne, mg, 1e-4, 20.0, 0, predp, st)
    for kw in (dict(qp=q.data_ptr() + 4), dict(ld=33), dict(ld=34), dict(ne=0), dict(ne=65536), dict(tabp=0), dict(predp=0), dict(C=48),
               dict(bs=npix * 36 + 2), dict(mg=0)):
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(pred).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(pred).all())


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("counts", [(40, 56), (40, 57), (0, 96, 1)])
def test_merge_banks(dev, which, counts):
    """Counts summing to 96 (one full group) and 97: rows == the concatenation in bank order, meta == the sum, and the scores against the
    merged bank == sim_ref over the concatenated rows."""
    from protosam_amd import ops
    from protosam_amd.alpmodule import MultiProtoAsConv
    C, npix = 32, 70
    rows = [K.unit_rows(n, C, 30 + i, which) for i, n in enumerate(counts)]
    other = K.unit_rows(2, C, 40)
    banks = [_hand_bank(dev, n + 4, C, *((r, other) if which == 0 else (other, r))) for r, n in zip(rows, counts)]
    merged = MultiProtoAsConv.merge_banks(banks, which)
    tot = sum(counts)
    cat = K.merge_ref(rows, counts)
    assert merged.cap == tot + 1 and int(merged.meta[ops.META_NFG if which else ops.META_NBG]) == tot
    assert torch.equal(merged.bank[which * merged.cap:which * merged.cap + tot].cpu(), cat)
    q = K.queries(1, npix, C, cat, 50)
    pred, _ = _sim(dev, q, merged, C + 4, 8, which_only=which)
    S, bound = K.sim_ref(q[0], cat, EPS, SCALE)
    _within(pred[0, which], S, bound, f"merge_banks which={which} counts={counts}", "merge_banks + " + _sim_path("d2", merged.cap))
    assert bool(torch.isnan(pred[0, 1 - which]).all())


def test_merge_banks_empty(dev):
    from protosam_amd import ops
    from protosam_amd.alpmodule import MultiProtoAsConv
    empty = torch.zeros((0, 32))
    banks = [_hand_bank(dev, 5, 32, empty, K.unit_rows(2, 32, 1)) for _ in range(2)]
    merged = MultiProtoAsConv.merge_banks(banks, 0)
    assert int(merged.meta[ops.META_NBG]) == 0 and merged.cap >= 2
    q = K.queries(1, 33, 32, None, 1)
    pred, _ = _sim(dev, q, merged, 36, 8, which_only=0)
    assert bool(torch.isnan(pred[0, 0]).all())
