"""GPU: the item maps of the attention kernels - how each turns a workgroup id into (image, head, window or query block) - over
batch and head counts the arithmetic tests (tests/test_attention_exact_gpu.py, B * H <= 12) never reach: H = 12, 16, 32, 33, 48, 64,
odd H, fewer items than XCDs, more items than CUs, both branches of the window kernel's work list and the last (B, H) the global
assembly kernels' work table admits.

The maps (csrc/attention.hip; the two host-built tables csrc/work_tables.h), restated on the host - below, and the list-building parts
in oracle/attention.py, which tests/test_work_tables_cpu.py compares with the C++ - so that every case can say which of their branches
it exercises:
  * attn_kernel, wattn_kernel, gattn_kernel, gattn_any_kernel: blockIdx.x -> group g * 8 + (r & 7), index r >> 3 over
    ceil(groups / 8) * 8 * per workgroups; those of a group >= groups leave at once (`_arith`);
  * wattn_p_kernel: min(B * windows * H, CUs) workgroups; XCD x = wg & 7 owns the windows grp = q * 8 + x, its workgroups cut its
    (window, head) list into contiguous shares and walk them with item_at / item_next (`_wattn_p_lists`);
  * psam_wattn_asm_80: the host table wattn_work_list - where an XCD's workgroup count is a multiple of H a workgroup keeps ONE head and
    strides over the windows, elsewhere the contiguous shares of wattn_p_kernel (`_wattn_asm_lists`);
  * psam_gattn_asm_*: the host table gattn_work_table - B * H * query blocks items cut into eight equal runs, padded with -1, an entry
    (b * H + h) << 10 | query block, and b = ((b * H + h) * ceil(2^16 / H)) >> 16 inside the kernel (`_gattn_asm_table`).

That division: with M = ceil(2^16 / H) = (2^16 + e) / H, 0 <= e < H, and grp = b H + h, 0 <= h < H:
    grp M / 2^16 = b + h / H + grp e / (H 2^16),  which stays below b + 1 for every h <= H - 1 exactly when grp e < 2^16.
gattn_asm_eligible admits grp < floor(2^16 / H), so grp e < (2^16 / H) (H - 1) < 2^16: the guard is sufficient for every H (for
H = 48: M = 1366, e = 32, largest grp 1343, 1343 * 32 = 42976 < 65536). `test_table_division_is_exact_where_admitted` walks every
admitted grp of every H <= 64; the sweep runs the last admitted B for H = 48 and 64 (28 and 15) on the assembly kernel and the first
refused (29 and 16) on the HIP kernel it falls back to, and asserts which one ran.

Checks per case and path, all exact (oracle/attention.py; tests/test_attention_reference_cpu.py shows on the CPU that a dropped item, two
exchanged heads, an item computed from another image and an item written twice while its successor is skipped each fail at least
one of them - constant V, whose c differs between heads only, is blind to the wrong image; the selectors are not):
  * the kernel `ops.attention_last_kernel()` reports is the one the path names;
  * selector inputs (QK; rel-pos in modes 1 / 2): the target's v row to one fp16 ulp, the >= 32 nat margin asserted on the float64
    reference before any kernel output is looked at;
  * constant V: `constant_v_bound`;
  * the output buffer starts as NaN and has one image of NaN guard rows behind the last image, which must stay NaN.
Every case prints an `ITEMS |` line with the branches of its map; `test_every_branch_is_reached` recomputes them over the case lists
and fails when an edit of a list loses one. profiles/attention_item_tests.txt holds the lines of one full run.
"""
import pytest
import torch

from oracle import attention as A
from protosam_amd import ops as K          # (the ids only: nothing here loads the library)
from test_attention_exact_gpu import _any_id, _full, _relpos_id, _run   # noqa: E402  (one launch of a path, as the exact tests make it)

pytestmark = pytest.mark.gpu

XCDS = A.XCDS                              # as the kernels assume (blockIdx.x & 7)
NWIN64 = A.NWIN64                          # 14 x 14 windows of the 64 x 64 map
_shares = A.wattn_shares                   # per workgroup of wattn_p_kernel: (wg, x, sx, nwg_x, windows of the XCD, it0, it1)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- the maps on the host: which branch a case exercises -------------------------------------------------------------------------------
def _arith(groups, per):
    """the arithmetic map: (workgroups, branches); every (group, index) exactly once among the workgroups that stay."""
    nwg = -(-groups // 8) * 8 * per
    seen = set()
    for wg in range(nwg):
        g, r = divmod(wg, 8 * per)
        grp = g * 8 + (r & 7)
        if grp < groups:
            seen.add((grp, r >> 3))
    assert len(seen) == groups * per
    surplus = (-(-groups // 8) * 8 - groups) * per
    return {"arith: surplus workgroups leave (grp >= nshare)" if surplus else "arith: every workgroup has an item"}


def _walk_branches(lists, B, H, nwin, grid, cus, name):
    """branches common to both persistent window kernels from the per-workgroup lists of (b, h, win); every item exactly once."""
    flat = [it for l in lists for it in l]
    assert len(flat) == len(set(flat)) == B * H * nwin, (len(flat), len(set(flat)), B * H * nwin)
    out = set()
    nwg = {(grid + 7 - x) >> 3 for x in range(XCDS)}
    if grid == cus:
        out.add(f"{name}: grid == CUs (more items than CUs)")
    elif len(nwg) > 1:
        out.add(f"{name}: grid < CUs, unequal nwg_x across XCDs")
    else:
        out.add(f"{name}: grid < CUs, equal nwg_x")
    if B * H * nwin < XCDS:
        out.add(f"{name}: fewer items than XCDs")
    if any(not l for l in lists):
        out.add(f"{name}: a workgroup without items leaves at once")
    for l in lists:
        for (b0, h0, w0), (b1, h1, w1) in zip(l, l[1:]):
            if b1 == b0 + 1 and h0 == H - 1 and h1 in (0, h0):
                out.add(f"{name}: a list goes from the last head of image b's last window on this XCD to image b + 1")
    return out


def _wattn_p_lists(B, H, nwin, cus):
    """wattn_p_kernel: item_at at it0, item_next up to it1."""
    grid = min(B * nwin * H, cus)
    lists = []
    for wg, x, sx, nwg_x, nwin_x, it0, it1 in _shares(B, H, nwin, grid):
        l = []
        if it0 < it1:
            grpq, h = divmod(it0, H)
            for _ in range(it1 - it0):
                grp = grpq * 8 + x
                l.append((grp // nwin, h, grp % nwin))
                h += 1
                if h == H:
                    h, grpq = 0, grpq + 1
        lists.append(l)
    return _walk_branches(lists, B, H, nwin, grid, cus, "wattn_p")


def _wattn_asm_lists(B, H, cus):
    """wattn_work_list of psam_wattn_asm_80 (the 64 x 64 map: 25 windows)."""
    nwin = NWIN64
    grid = min(B * nwin * H, cus)
    lists, one_head = A.wattn_asm_lists(B, H, grid)
    out = set()
    for f in one_head:
        if f:
            out.add("wattn_asm: nwg_x % H == 0 (one head per workgroup)" + (", grid == CUs" if grid == cus else ", grid < CUs"))
        else:
            out.add("wattn_asm: nwg_x % H != 0 (contiguous shares)")
    return out | _walk_branches(lists, B, H, nwin, grid, cus, "wattn_asm")


def _gattn_asm_table(B, H, nqb):
    """gattn_work_table and the kernel's decode of its entries; every (b, h, query block) exactly once."""
    items = B * H * nqb
    tab = A.gattn_asm_table(B * H, nqb, XCDS)
    seen = set(A.gattn_asm_decode(tab, H))
    assert seen == {(b, h, q) for b in range(B) for h in range(H) for q in range(nqb)}, "the table or its decode loses an item"
    out = {"gattn_asm: padded table (-1 entries)" if -1 in tab else "gattn_asm: no padding"}
    if items < XCDS:
        out.add("gattn_asm: fewer items than XCDs")
    if nqb > 1:
        out.add("gattn_asm: more than one query block")
    if not A.gattn_asm_admits(B + 1, H):
        out.add(f"gattn_asm: the last B the table admits for H = {H}")
    return out


def _branches(kid, mode, B, H, N, gh, gw, cus):
    """the branches of the map of the kernel `kid` names at this shape."""
    fam = kid & K.ATTN_KERNEL_FAMILY
    nwin = -(-gh // A.WS) * -(-gw // A.WS) if mode == 2 else 0
    if fam == K.ATTN_KERNEL_ASM_WINDOW:
        return _wattn_asm_lists(B, H, cus)
    if fam == K.ATTN_KERNEL_WATTN_P:
        return _wattn_p_lists(B, H, nwin, cus)
    if fam in (K.ATTN_KERNEL_ASM_REL, K.ATTN_KERNEL_ASM_FUSED, K.ATTN_KERNEL_ASM_NOREL):
        return _gattn_asm_table(B, H, -(-N // 256))
    out = _arith(B * nwin, H) if mode == 2 else _arith(B * H, -(-N // 128))
    if mode != 2 and H in (48, 64) and not A.gattn_asm_admits(B, H) and A.gattn_asm_admits(B - 1, H):
        out.add(f"gattn_asm: the first B refused for H = {H} runs the HIP kernel")
    return out


REQUIRED = {
    "wattn_asm: nwg_x % H == 0 (one head per workgroup), grid == CUs", "wattn_asm: nwg_x % H != 0 (contiguous shares)",
    "wattn_asm: grid < CUs, unequal nwg_x across XCDs", "wattn_asm: grid == CUs (more items than CUs)",
    "wattn_asm: a list goes from the last head of image b's last window on this XCD to image b + 1",
    "wattn_p: grid == CUs (more items than CUs)", "wattn_p: grid < CUs, unequal nwg_x across XCDs", "wattn_p: fewer items than XCDs",
    "wattn_p: a workgroup without items leaves at once",
    "wattn_p: a list goes from the last head of image b's last window on this XCD to image b + 1",
    "gattn_asm: fewer items than XCDs", "gattn_asm: padded table (-1 entries)", "gattn_asm: no padding",
    "gattn_asm: more than one query block", "gattn_asm: the last B the table admits for H = 48",
    "gattn_asm: the last B the table admits for H = 64", "gattn_asm: the first B refused for H = 48 runs the HIP kernel",
    "gattn_asm: the first B refused for H = 64 runs the HIP kernel",
    "arith: surplus workgroups leave (grp >= nshare)", "arith: every workgroup has an item",
}


# ---- one case ------------------------------------------------------------------------------------------------------------------------
def _sweep(dev, label, mode, B, H, hd, paths, N=0, gh=0, gw=0, head_major=False, seed=0):
    """the selectors and constant V at one (B, H) on every path = (name, variant, kind, kernel id): id, values, NaN prefill, guard rows.
    Inputs and the float64 reference live on the device; the reference is computed once per family and shared by the paths."""
    from protosam_amd import ops
    geo = dict(N=N, gh=gh, gw=gw, device=dev)
    cases = [("qk-selector", A.selector_qk(mode, B, H, hd, seed=seed + 1, **geo))]
    if mode:
        cases.append(("relpos-selector", A.selector_relpos(mode, B, H, hd, gh, gw, seed=seed + 2, device=dev)))
    cases.append(("constant-v", A.constant_v(mode, B, H, hd, seed=seed + 3, **geo)))
    N = cases[0][1].N
    shape = f"{label} B{B} H{H} hd{hd} " + (f"N{N}" if mode == 0 else f"{gh}x{gw}") + (" head-major" if head_major else "")
    cus = _cus()
    for name, _, _, kid in paths:
        print(f"ITEMS | {shape} | {name} | {K.attention_kernel_name(kid)} | {B * H} heads, {cus} CUs | "
              + "; ".join(sorted(_branches(kid, mode, B, H, N, gh, gw, cus))))
    errors = []
    for fam, case in cases:
        if fam.endswith("selector"):
            ref = A.reference(case.qkv, mode, budget=False, targets=case.targets, **A.ref_kwargs(case))
            margin = A.check_margin(case, ref)               # the condition, before any kernel output
            print(f"ITEMS | {shape} | {fam} | least margin {margin:.1f} nats")
            del ref
        for name, variant, kind, kid in paths:
            buf = torch.full((B + 1, N, H * hd), float("nan"), device=dev, dtype=torch.float16)
            ops.attention_set_variant(variant)
            try:
                _run(case, kind, head_major, out=buf[:B])
                landed = ops.attention_last_kernel()
            finally:
                ops.attention_set_variant(5)
            try:
                assert landed == kid, (f"ran {ops.attention_kernel_name(landed)} ({landed:#x}), the path names "
                                       f"{ops.attention_kernel_name(kid)} ({kid:#x})")
                A.check_guard(buf, B)
                if fam.endswith("selector"):
                    res = f"not bit-equal {A.check_selector(buf[:B], case)}"
                else:
                    res = f"max/bound {A.check_constant_v(buf[:B], case):.3f}"
                print(f"ITEMS | {shape} | {fam} | {name} | {res}")
            except AssertionError as e:
                print(f"ITEMS | {shape} | {fam} | {name} | FAILED {e}")
                errors.append(f"{shape}, {fam}, {name}: {e}")
            del buf
    assert not errors, f"{len(errors)} failures:\n" + "\n".join(errors)


# ---- the case lists: (mode, B, H, hd, N, gh, gw, paths), shared with test_every_branch_is_reached ---------------------------------------
def _window64_paths():
    return [("default: psam_wattn_asm_80", 5, "window", K.ATTN_KERNEL_ASM_WINDOW),
            ("variant 7: wattn_p_kernel", 7, "window", K.ATTN_KERNEL_WATTN_P),
            ("variant 3: wattn_kernel", 3, "window", K.ATTN_KERNEL_WATTN), ("variant 1: attn_kernel", 1, "window", K.ATTN_KERNEL_ATTN)]


def _asm_or_hip(B, H, asm, N):
    """the default dispatch of the global kernels: the assembly kernel while its work table admits (B, H), else gattn_kernel."""
    if A.gattn_asm_admits(B, H):
        return ("default: " + K.ATTN_KERNEL_NAMES[asm], asm)
    return ("default: gattn_kernel (the assembly work table refuses B * H)", K.ATTN_KERNEL_GATTN | _full(N))


def _hip_paths(N):
    f = _full(N)
    return [("variant 21: gattn_kernel", 21, "plain", K.ATTN_KERNEL_GATTN | f),
            ("variant 9: attn_kernel V2", 9, "plain", K.ATTN_KERNEL_ATTN | f | K.ATTN_KERNEL_V2),
            ("variant 8: attn_kernel serial", 8, "plain", K.ATTN_KERNEL_ATTN | f)]


def _all_cases():
    """every (mode, B, H, N, gh, gw, kernel id) the sweeps below launch."""
    out = []
    for B, H in A.ITEMS_WINDOW64_BH:
        out += [(2, B, H, 4096, 64, 64, p[3]) for p in _window64_paths()]
    for g, hd, B, H in A.ITEMS_WINDOW_SMALL:
        out.append((2, B, H, g * g, g, g, K.ATTN_KERNEL_WATTN_P))
    for N in (128, 449):
        out += [(0, B, H, N, 0, 0, K.ATTN_KERNEL_ASM_NOREL) for B, H in A.ITEMS_ASM_BH]
    for B, H in A.ITEMS_ASM_EDGES:
        out.append((0, B, H, 128, 0, 0, _asm_or_hip(B, H, K.ATTN_KERNEL_ASM_NOREL, 128)[1]))
        out.append((1, B, H, 256, 4, 64, _asm_or_hip(B, H, K.ATTN_KERNEL_ASM_REL, 256)[1]))
    out += [(1, B, H, 256, 4, 64, K.ATTN_KERNEL_ASM_REL) for B, H in A.ITEMS_ASM_BH]
    out += [(1, B, H, 4096, 64, 64, K.ATTN_KERNEL_ASM_FUSED) for B, H in A.ITEMS_FUSED_BH]
    for B, H in A.ITEMS_HIP_BH:
        out += [(0, B, H, 200, 0, 0, p[3]) for p in _hip_paths(200)]
        out += [(1, B, H, gh * gw, gh, gw, _any_id(gh, gw)) for gh, gw in A.ITEMS_ANY_MAPS]
    return out


def test_table_division_is_exact_where_admitted():
    """b = (grp * ceil(2^16 / H)) >> 16 equals grp // H for every grp gattn_asm_eligible admits, for every H it admits (the derivation
    in the module docstring, walked); and it is the guard, not luck, that keeps it so: for H = 48 the first wrong grp lies beyond."""
    for H in range(1, 65):
        M = (65536 + H - 1) // H
        lim = 65536 // H
        assert A.gattn_asm_admits((lim - 1) // H, H) or lim - 1 < H
        assert all((grp * M) >> 16 == grp // H for grp in range(lim)), H
        assert (lim - 1) * M < 2 ** 32                                    # the kernel's 32-bit product, shifted right logically
    first_wrong = next(grp for grp in range(1 << 16) if (grp * 1366) >> 16 != grp // 48)
    assert first_wrong >= 65536 // 48 and A.gattn_asm_admits(28, 48) and not A.gattn_asm_admits(29, 48)
    assert A.gattn_asm_admits(15, 64) and not A.gattn_asm_admits(16, 64)


# ---- windows -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", A.ITEMS_WINDOW64_BH)
def test_window_64x64_hd80(dev, B, H):
    """the 64 x 64 map, hd = 80: psam_wattn_asm_80 on the default dispatch, wattn_p_kernel, wattn_kernel and attn_kernel forced. 25
    windows per image: (1, 1) 25 items, (1, 5) 125 (XCDs with 16 and 15 workgroups - both branches of the work list in ONE table),
    (11, 1) 275 windows, neither a multiple of 8 nor of 25 * 8; H = 16 and 32 divide the 32 workgroups an XCD has of 256, 3, 5, 7
    and 12 do not."""
    _sweep(dev, "mode2", 2, B, H, 80, _window64_paths(), gh=64, gw=64, seed=100 * B + H)


@pytest.mark.parametrize("g,hd,B,H", A.ITEMS_WINDOW_SMALL)
def test_window_smaller_maps(dev, g, hd, B, H):
    """maps the assembly kernel does not take: the default dispatch must say wattn_p_kernel. 32 x 32 (nine windows), 20 x 20 (four),
    14 x 14 (ONE window: B * H = 1, 2, 3 items for eight XCDs; with one window and two heads the second workgroup has nothing)."""
    _sweep(dev, "mode2", 2, B, H, hd, [("default: wattn_p_kernel", 5, "window", K.ATTN_KERNEL_WATTN_P)], gh=g, gw=g,
           seed=g + hd + 100 * B + H)


# ---- the global assembly kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", A.ITEMS_ASM_BH)
@pytest.mark.parametrize("N", [128, 449])
def test_global_asm_norel(dev, N, B, H):
    """psam_gattn_asm_64_norel: one query block (128) and two (449); (1, 1) at 128 tokens is ONE item in eight table slots."""
    _sweep(dev, "mode0", 0, B, H, 64, [("default: psam_gattn_asm_64_norel", 5, "plain", K.ATTN_KERNEL_ASM_NOREL)], N=N,
           seed=N + 100 * B + H)


@pytest.mark.parametrize("B,H", A.ITEMS_ASM_EDGES)
def test_global_asm_norel_at_the_table_limit(dev, B, H):
    """B * H < 65536 // H: (28, 48) and (15, 64) are the last the table admits and run the assembly kernel, (29, 48) and (16, 64)
    the first refused - the id must name gattn_kernel, and the same checks hold."""
    name, kid = _asm_or_hip(B, H, K.ATTN_KERNEL_ASM_NOREL, 128)
    assert (kid == K.ATTN_KERNEL_ASM_NOREL) == ((B, H) in ((28, 48), (15, 64)))
    _sweep(dev, "mode0", 0, B, H, 64, [(name, 5, "plain", kid)], N=128, seed=100 * B + H)


@pytest.mark.parametrize("B,H", A.ITEMS_ASM_BH + A.ITEMS_ASM_EDGES)
@pytest.mark.parametrize("hd", A.HEAD_DIMS)
def test_global_asm_rel(dev, hd, B, H):
    """psam_gattn_asm_{80,64}_rel at gh = 4, gw = 64 (N = 256, one query block), rel_h / rel_w from `ops.relpos` (whose own id is
    asserted: four query tiles per wave); at the table limit as above."""
    name, kid = _asm_or_hip(B, H, K.ATTN_KERNEL_ASM_REL, 256)
    _sweep(dev, "mode1 psam_relpos", 1, B, H, hd, [(name, 5, "terms", kid)], gh=4, gw=64, seed=hd + 100 * B + H)


@pytest.mark.parametrize("B,H", A.ITEMS_FUSED_BH)
@pytest.mark.parametrize("hd", A.HEAD_DIMS)
def test_global_asm_fused(dev, hd, B, H):
    """psam_gattn_asm_{80,64}_fused at 64 x 64: 16 query blocks per (image, head)."""
    _sweep(dev, "mode1 tables", 1, B, H, hd, [(f"default: psam_gattn_asm_{hd}_fused", 5, "tables", K.ATTN_KERNEL_ASM_FUSED)], gh=64, gw=64,
           seed=hd + 100 * B + H)


# ---- the HIP global kernels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", A.ITEMS_HIP_BH)
@pytest.mark.parametrize("hd", A.HEAD_DIMS)
def test_global_hip_kernels(dev, hd, B, H):
    """gattn_kernel (21), attn_kernel with the V2 (9) and the serial softmax (8) at N = 200, their ragged instances, two query blocks:
    1, 7, 60 and 32 groups for rows of eight - seven, one, four and no surplus groups whose workgroups leave."""
    _sweep(dev, "mode0", 0, B, H, hd, _hip_paths(200), N=200, seed=hd + 100 * B + H)


@pytest.mark.parametrize("B,H", A.ITEMS_HIP_BH)
@pytest.mark.parametrize("hd", A.HEAD_DIMS)
@pytest.mark.parametrize("gh,gw", A.ITEMS_ANY_MAPS)
def test_global_any_map(dev, gh, gw, hd, B, H):
    """gattn_any_kernel at 5 x 7 (one query block) and 20 x 28 (five)."""
    _sweep(dev, "mode1 tables", 1, B, H, hd, [("gattn_any_kernel", 5, "tables", _any_id(gh, gw))], gh=gh, gw=gw,
           seed=gh * 64 + gw + hd + 100 * B + H)


# ---- head-major qkv and psam_relpos at (5, 12) -------------------------------------------------------------------------------------------
def test_head_major_at_5x12(dev):
    """one case per mode: the strides of a head-major qkv grow with B (an image is B * N rows of ONE head apart from the next head)."""
    _sweep(dev, "mode0", 0, 5, 12, 64, [("default: psam_gattn_asm_64_norel", 5, "plain", K.ATTN_KERNEL_ASM_NOREL)], N=128, head_major=True,
           seed=81)
    _sweep(dev, "mode1 psam_relpos", 1, 5, 12, 80, [("default: psam_gattn_asm_rel", 5, "terms", K.ATTN_KERNEL_ASM_REL)], gh=4, gw=64,
           head_major=True, seed=82)
    _sweep(dev, "mode1 tables", 1, 5, 12, 64, [("gattn_any_kernel", 5, "tables", _any_id(20, 28))], gh=20, gw=28, head_major=True, seed=83)
    _sweep(dev, "mode2", 2, 5, 12, 80, [("default: wattn_p_kernel", 5, "window", K.ATTN_KERNEL_WATTN_P)], gh=32, gw=32, head_major=True,
           seed=84)


@pytest.mark.parametrize("hd", A.HEAD_DIMS)
def test_relpos_both_forms_at_5x12(dev, hd):
    """psam_relpos' grid is (query tiles, H, B): four query tiles per wave where N is a multiple of 256 (4 x 64 = 256, 32 x 32 = 1024)
    and one elsewhere (9 x 64 = 24 x 24 = 576), global (rel_h / rel_w for the mode-1 kernels) and windowed (relq for attn_kernel);
    `_run` asserts the relpos id (QT4 or not) from N. At N = 576 the global assembly kernel does not apply: gattn_kernel."""
    assert _relpos_id(256) != _relpos_id(576) == K.ATTN_KERNEL_RELPOS
    _sweep(dev, "mode1 psam_relpos", 1, 5, 12, hd, [("default: psam_gattn_asm_rel", 5, "terms", K.ATTN_KERNEL_ASM_REL)], gh=4, gw=64,
           seed=91 + hd)
    hip = [("default: gattn_kernel (N % 256 != 0)", 5, "terms", K.ATTN_KERNEL_GATTN | K.ATTN_KERNEL_FULL)]
    _sweep(dev, "mode1 psam_relpos", 1, 5, 12, hd, hip, gh=9, gw=64, seed=92 + hd)
    relq = [("relq: psam_relpos + attn_kernel", 5, "relq", K.ATTN_KERNEL_ATTN)]
    _sweep(dev, "mode2", 2, 5, 12, hd, relq, gh=32, gw=32, seed=93 + hd)
    _sweep(dev, "mode2", 2, 5, 12, hd, relq, gh=24, gw=24, seed=94 + hd)


# ---- last: the branch accounting -----------------------------------------------------------------------------------------------------
def test_every_branch_is_reached(dev):
    """the branches of the maps over the case lists of this file at this device's CU count: an edit of a list that loses one fails."""
    cus = _cus()
    hit = set()
    for mode, B, H, N, gh, gw, kid in _all_cases():
        hit |= _branches(kid, mode, B, H, N, gh, gw, cus)
    for b in sorted(hit):
        print(f"ITEMS | branch reached | {b}")
    assert REQUIRED <= hit, f"with {cus} CUs the case lists no longer reach: {sorted(REQUIRED - hit)}"
