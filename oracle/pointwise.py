"""Oracle of the two pointwise functions every transformer block runs: the GELU of the GEMM epilogues (EPI_GELU_F16: common.h gelu_erf,
csrc/gemm_asm_gen.py gelu_quad, csrc/gemm_asm2_gen.py gelu_scalar) and the row LayerNorm psam_layernorm (csrc/layernorm.hip).
CPU torch / numpy only. Used by tests/test_pointwise_reference_cpu.py (no GPU: the references alone pass, every injected fault fails) and
by tests/test_gelu_epilogue_gpu.py / tests/test_layernorm_gpu.py (the kernels, through the same checks).

GELU. The pre-activation x = acc + bias is made EXACT: a[m, m % K] = c_m and zeros elsewhere, w all ones, bias = d, so that
x[m, n] = c_m + d_n from one non-zero product, whatever the order of the summation and whether the accumulator starts at 0 or at the bias
(tile 16). Three sets of one shape (257 x 256: two row tiles of every kernel, one ragged):
  * "grid":      c_m = (m - 128) / 4, d_n = n 2^-10: the uniform sweep of [-32, 32.25) at step 2^-10, every x a multiple of 2^-10 below 2^6;
  * "tail-rows": c_m = +-{64 .. 32768 by powers of two, 59744}, d_n = n: integers below 2^24, |x| <= 59999 (fp16 holds 65504);
  * "tail-bias": c_m = 0, so x = d_n: +-{0, 2^-149, 1e-30, 2^-24, 2^-14, 1, 6, 8, 13, 13.5, 20, 60000} and a log-spaced sweep of
    +-[2^-20, 2^15]. (One bias vector serves a whole launch, so the rows of large c and the special biases are two launches.)
No infinity and no NaN goes in and nothing overflows fp16. Reference: 0.5 x erfc(-x / sqrt 2) in float64 (no cancellation in the negative
tail, where 1 + erf loses every digit). Bound: 3.4e-6 + 2^-11 |y|, the epilogue-1 bound of oracle/gemm.py with E_acc = 0: 3.4e-6 is the
project's figure for the shipped forms against erf, 2^-11 |y| the fp16 rounding. Structural checks, which no bound on |error| gives:
every output finite; y x >= 0 (a GELU never changes the sign; zeros of either sign pass); x >= 8: |y - x| <= 2^-11 |x| (gelu(x) = x to
1e-14 there: the fp16 rounding alone); x <= -8: |y| <= 3.4e-6. Nothing here is tuned on a kernel: the CPU test shows fp32 F.gelu and fp32
emulations of both shipped operation sequences inside every check (they reach 0.999 of the bound, at fp16 ties).

LayerNorm. `layernorm_bound` is oracle.gemm.layernorm16_bound (the derived bound of a two-pass fp32 LayerNorm); an fp32 output drops its
fp16-rounding term H |y|. `LNCase` / `ln_cases()` is the case table both test files share; `LNBuffers` holds x as a view with row stride
ldx into a buffer of NaN (more rows than M behind it, finite), and the output as a view with row stride ldy into a buffer of a sentinel
bit pattern: one guard row before row 0, the M owed rows prefilled with NaN, `zero_tail_rows` rows that must come back as +0, eight guard
rows behind, guard columns D .. ldy - 1. `ln_violations` compares everything that is not owed as integers, holds the owed elements to the
bound and all-zero rows to b exactly. Regimes (|x| <= 1e4): plain N(0, 3) + 0.7; offset N(0, 1) + c with c = `offset_c(D)`; outlier N(0, 1)
with two channels at +300 / -250; tinyvar 5 + 1e-3 N(0, 1); const (one value per row, another in the next row); zero; mixed = the six
interleaved row by row. offset_c: the bound's variance term grows as D u c / std and a one-pass variance E[x^2] - mean^2 errs by u c^2 /
std^2, so the fault shows only where c is large against D: 1000 up to D = 256, 4000 beyond, where u c^2 reaches the variance itself (the
CPU test asserts both sides at every D)."""
import functools
import importlib
import math
import os
import sys
from dataclasses import dataclass

import numpy as np
import torch

from oracle.gemm import E_ASM2, H, U, _padded, _rand, _sentinel, layernorm16_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------------------------------------ GELU
GELU_M, GELU_N = 257, 256
GELU_ABS = 3.4e-6
GELU_TILES = (1, 11, 12, 13, 15, 16, 17)
GELU_LN_TILES = (1, 11, 15, 17)
_BIG_C = (64.0, 128.0, 256.0, 512.0, 1024.0, 2048.0, 4096.0, 8192.0, 16384.0, 32768.0, 59744.0)
_SPECIAL = (0.0, 2.0 ** -149, 1e-30, 2.0 ** -24, 2.0 ** -14, 1.0, 6.0, 8.0, 13.0, 13.5, 20.0, 60000.0)


def _grid_cd():
    return (torch.arange(GELU_M, dtype=torch.float32) - 128.0) * 0.25, torch.arange(GELU_N, dtype=torch.float32) * 2.0 ** -10


def gelu_grid():
    """the exact fp32 pre-activations x[m, n] = c_m + d_n, c_m = (m - 128) / 4, d_n = n 2^-10: the uniform sweep of [-32, 32.25) at step 2^-10"""
    c, d = _grid_cd()
    return c[:, None] + d[None, :]


@functools.lru_cache(maxsize=None)
def gelu_sets():
    """name -> (c, d): the grid and the two halves of the tail set (module docstring)"""
    sign = torch.tensor([1.0, -1.0]).repeat(GELU_M)[:GELU_M]
    big = torch.tensor(_BIG_C)[(torch.arange(GELU_M) // 2) % len(_BIG_C)] * sign
    sp = torch.tensor(_SPECIAL, dtype=torch.float64)
    n = (GELU_N - 2 * len(_SPECIAL)) // 2
    sweep = torch.exp2(torch.linspace(-20.0, 15.0, n, dtype=torch.float64))
    d = torch.cat([sp, -sp, sweep, -sweep]).float()
    assert d.numel() == GELU_N and torch.isfinite(d).all()
    return {"grid": _grid_cd(), "tail-rows": (big, torch.arange(GELU_N, dtype=torch.float32)), "tail-bias": (torch.zeros(GELU_M), d)}


def gelu_x(c, d):
    """the exact pre-activations in float64; asserts what makes them exact in fp32 and fp16-safe"""
    x = c.double()[:, None] + d.double()[None, :]
    assert torch.equal(x.float().double(), x) and torch.equal(c.half().float(), c) and x.abs().max().item() <= 60000.0
    return x


def gelu_min_k(tile):
    """the tile's minimum K as oracle.gemm.bound_shape takes it"""
    return 64 * max(3, E_ASM2[1] + 1) if tile == 16 else 256 if tile == 12 else 192


def gelu_operands(c, d, K):
    """(a, w, bias) on the CPU: a and w are views with lda = K + 64, ldw = K + 8 into buffers of oracle.gemm's poison"""
    M = c.numel()
    a = torch.zeros((M, K), dtype=torch.float64)
    a[torch.arange(M), torch.arange(M) % K] = c.double()
    a_buf, av = _padded(a, K + 64, torch.float16)
    w_buf, wv = _padded(torch.ones((GELU_N, K), dtype=torch.float64), K + 8, torch.float16, rows_after=8)
    return (a_buf, av), (w_buf, wv), d.clone()


def gelu_ln_operands(M, N, seed=77):
    """(ln_mr, ln_s) of a folded-LayerNorm consumer with mean 0 and rstd 1, written by hand in the layout of the ops.gemm docstring: fp32
    (0, 1) per row, then the fp16 fragments of -mean, all zero; ln_s = any s in the s_ext layout of ops.fold_layernorm. Then
    rstd (acc - mean s) + t = acc + t exactly on every tile."""
    mr = torch.zeros(6 * M, dtype=torch.float32)
    mr[1:2 * M:2] = 1.0
    s = _rand((N,), torch.device("cpu"), 3.0, seed)
    hi = s.half()
    frag = torch.zeros((N, 8), dtype=torch.float16)
    frag[:, 0], frag[:, 1], frag[:, 2] = hi, (s - hi.float()).half(), hi
    return mr, torch.cat([s, frag.reshape(-1).view(torch.float32)]).contiguous()


def gelu_ref(x64):
    return 0.5 * x64 * torch.special.erfc(-x64 / math.sqrt(2.0))


RANGES = (("x < -8", -math.inf, -8.0), ("-8 <= x < -4.5", -8.0, -4.5), ("|x| <= 4.5", -4.5, 4.5), ("4.5 < x <= 8", 4.5, 8.0),
          ("x > 8", 8.0, math.inf))


def gelu_report(y, x64):
    """y: the fp16 outputs, x64: the exact pre-activations. -> (violations, {range: (worst |error| / bound, its x)})"""
    y64 = y.double().cpu() if torch.is_tensor(y) else torch.from_numpy(np.asarray(y, dtype=np.float64))
    ref = gelu_ref(x64)
    fin = torch.isfinite(y64)
    yz = torch.where(fin, y64, torch.zeros_like(y64))
    ratio = (yz - ref).abs() / (GELU_ABS + H * ref.abs())
    bad = []
    if not bool(fin.all()):
        bad.append(f"{int((~fin).sum())} outputs not finite; first at x = {x64[~fin][0].item()!r}")
    w = yz * x64 < 0
    if bool(w.any()):
        bad.append(f"{int(w.sum())} outputs with the sign against x; first at x = {x64[w][0].item()!r}: {yz[w][0].item()!r}")
    w = (x64 >= 8.0) & ((yz - x64).abs() > H * x64.abs())
    if bool(w.any()):
        bad.append(f"{int(w.sum())} outputs off x by more than 2^-11 |x| at x >= 8; first at x = {x64[w][0].item()!r}: {yz[w][0].item()!r}")
    w = (x64 <= -8.0) & (yz.abs() > GELU_ABS)
    if bool(w.any()):
        bad.append(f"{int(w.sum())} outputs above 3.4e-6 at x <= -8; first at x = {x64[w][0].item()!r}: {yz[w][0].item()!r}")
    per = {}
    for name, lo, hi in RANGES:
        sel = (x64 > lo) & (x64 <= hi) if lo >= 4.5 else (x64 >= lo) & (x64 < hi) if hi <= -4.5 else (x64 >= lo) & (x64 <= hi)
        if bool(sel.any()):
            r = torch.where(sel, ratio, torch.full_like(ratio, -1.0))
            i = int(r.argmax())
            per[name] = (r.reshape(-1)[i].item(), x64.reshape(-1)[i].item())
    worst = max(per.values())
    if worst[0] > 1.0:
        bad.append(f"|error| = {worst[0]:.3f} times the bound 3.4e-6 + 2^-11 |y| at x = {worst[1]!r}")
    return bad, per


def gelu_check(y, x64, what):
    bad, per = gelu_report(y, x64)
    for name, (r, at) in per.items():
        print(f"{what}, {name}: worst |error| / bound = {r:.4f} at x = {at!r}")
    assert not bad, (what, bad)
    return per


def sigpoly_constants():
    """(c4, c3, c2, c1, c0) of gelu_quad as fp32, from the names csrc/gemm_asm_gen.py emits them under: GELU_SGPR_CONSTS, the SGPR list
    [c4 c4 c2 c2 c1 c1 c0 c0], and GELU_C3, the constant of the two VGPRs"""
    csrc = os.path.join(ROOT, "protosam_amd", "csrc")
    sys.path.insert(0, csrc)                       # (the generator imports its neighbour asm_common by name)
    try:
        gen = importlib.import_module("gemm_asm_gen")
    finally:
        sys.path.remove(csrc)
    lst = list(gen.GELU_SGPR_CONSTS)
    assert len(lst) == 8 and lst[0::2] == lst[1::2], lst
    bits = np.array([lst[0], gen.GELU_C3, lst[2], lst[4], lst[6]], dtype=np.uint32)
    return bits.view(np.float32)


def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32)


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 is exact in float64"""
    return _f32(a.astype(np.float64) * b.astype(np.float64) + np.asarray(c, dtype=np.float32).astype(np.float64))


def _mul(a, b):
    return _f32(a.astype(np.float64) * np.asarray(b, dtype=np.float32).astype(np.float64))


def emulate_gelu_erf(x64):
    """the operation sequence of common.h gelu_erf in fp32 (exp2 and the reciprocal correctly rounded), rounded to fp16"""
    with np.errstate(all="ignore"):
        x = _f32(x64.numpy())
        ax = np.abs(x)
        t = _f32(1.0 / _fma(ax, np.float32(0.23164189), np.float32(1.0)).astype(np.float64))
        p = _fma(np.full_like(t, 1.061405429), t, np.float32(-1.453152027))
        p = _fma(p, t, np.float32(1.421413741))
        p = _fma(p, t, np.float32(-0.284496736))
        p = _fma(p, t, np.float32(0.254829592))
        e = _f32(np.exp2(_mul(_mul(x, x), np.float32(-0.72134752044448170)).astype(np.float64)))
        y = _fma(_mul(-p, t), e, np.float32(1.0))
        h = _mul(x, np.float32(0.5))
        return _fma(h, np.copysign(y, x), h).astype(np.float16)


def emulate_gelu_sigpoly(x64, consts=None):
    """gelu_quad in fp32: x / (1 + exp2(x Q(x^2))), Q by Horner with the generator's own constants, rounded to fp16"""
    c4, c3, c2, c1, c0 = sigpoly_constants() if consts is None else consts
    with np.errstate(all="ignore"):
        x = _f32(x64.numpy())
        u = _mul(x, x)
        q = _fma(u, np.full_like(u, c4), c3)
        for c in (c2, c1, c0):
            q = _fma(q, u, c)
        e = _f32(np.exp2(_mul(x, q).astype(np.float64)))
        r = _f32(1.0 / (e + np.float32(1.0)).astype(np.float32).astype(np.float64))
        return _mul(x, r).astype(np.float16)


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_REGIMES = ("plain", "offset", "outlier", "tinyvar", "const", "zero", "mixed")
LN_D = (4, 64, 252, 256, 260, 768, 1024, 1280, 2044, 2048)
LN_M = (1, 3, 4, 5, 37, 1297)
LN_PRE, LN_POST, LN_EXTRA = 1, 8, 5      # guard rows before / behind the output; rows of x behind row M - 1


def offset_c(D):
    return 1000.0 if D <= 256 else 4000.0


def layernorm_bound(x, w, b, eps, out16):
    """float64 LayerNorm of x and the bound of a two-pass fp32 LayerNorm: oracle.gemm.layernorm16_bound, without H |y| for an fp32 output"""
    y, bound = layernorm16_bound(x, w, b, eps)
    return (y, bound) if out16 else (y, bound - H * y.abs())


@dataclass(frozen=True)
class LNCase:
    D: int
    M: int
    regime: str
    eps: float
    out16: bool
    xpad: int = 0            # ldx = D + xpad
    ypad: int = 0            # ldy = D + ypad
    tail: int = 0            # zero_tail_rows
    out2: bool = False       # an fp32 second copy next to an fp16 out

    @property
    def id(self):
        return (f"D{self.D}-M{self.M}-{self.regime}-eps{self.eps:g}-{'f16' if self.out16 else 'f32'}-ldx+{self.xpad}-ldy+{self.ypad}"
                f"-tail{self.tail}{'-out2' if self.out2 else ''}")


@functools.lru_cache(maxsize=None)
def ln_cases():
    """A pruned product: every D with three regimes, every regime at D = 260 and D = 2048, the other parameters cycled with periods that
    are coprime where they must meet (tests/test_pointwise_reference_cpu.py asserts the coverage)"""
    C, i = [], 0
    small_m = (3, 4, 5, 37, 1)

    def add(D, regime, M=None):
        nonlocal i
        M = M or (37 if regime == "mixed" else small_m[i % 5])
        if regime == "offset" and M == 1:       # the one-pass fault is a rounding error: one row alone can come out anywhere below its maximum
            M = 5
        out16 = (i // 4) % 2 == 0
        C.append(LNCase(D, M, regime, (1e-6, 1e-5)[i % 2], out16, (0, 4, 64)[i % 3], (0, 8)[(i // 2) % 2], (0, 1, 3, 6)[i % 4],
                        out16 and i % 3 != 1))
        i += 1

    for D in LN_D:
        regs = LN_REGIMES if D in (260, 2048) else ("plain", "offset", "mixed") + (("tinyvar",) if D in (4, 768) else ())
        for r in regs:
            add(D, r)
    i += 5                                       # the regimes of D = 260 and D = 2048 again, with the other output type and other strides
    for D in (260, 2048):
        for r in ("plain", "outlier", "tinyvar", "const", "zero"):
            add(D, r)
    for D, r in ((768, "plain"), (2048, "mixed"), (1280, "outlier"), (260, "mixed")):
        add(D, r, 1297)
        add(D, r, 1297)
    return tuple(C)


def ln_rows(regime, M, D, seed):
    """fp32 rows [M, D] of one regime"""
    cpu = torch.device("cpu")
    if regime == "mixed":
        parts = {r: ln_rows(r, M, D, seed + 10 * k) for k, r in enumerate(LN_REGIMES[:6])}
        return torch.stack([parts[LN_REGIMES[m % 6]][m] for m in range(M)])
    if regime == "plain":
        return _rand((M, D), cpu, 3.0, seed) + 0.7
    if regime == "offset":
        return _rand((M, D), cpu, 1.0, seed) + offset_c(D)
    if regime == "outlier":
        x = _rand((M, D), cpu, 1.0, seed)
        x[:, D // 3], x[:, (2 * D) // 3] = 300.0, -250.0
        return x
    if regime == "tinyvar":
        return 5.0 + 1e-3 * _rand((M, D), cpu, 1.0, seed)
    if regime == "const":
        return ((0.7 * (1 + torch.arange(M) % 5) - 2.0).float()[:, None]).expand(M, D).contiguous()
    assert regime == "zero"
    return torch.zeros((M, D))


class LNBuffers:
    """inputs, guarded outputs and the float64 reference of one case, all on the CPU"""

    def __init__(self, c):
        self.case = c
        D, M = c.D, c.M
        self.ldx, self.ldy = D + c.xpad, D + c.ypad
        seed = 7000 + 13 * D + M
        self.rows = ln_rows(c.regime, M, D, seed)
        assert self.rows.abs().max().item() <= 1e4
        R = M + LN_EXTRA
        self.x_buf = torch.full((R * self.ldx,), float("nan"))
        self.x_all = torch.as_strided(self.x_buf, (R, D), (self.ldx, 1), 0)
        self.x_all[:M] = self.rows
        self.x_all[M:] = _rand((LN_EXTRA, D), torch.device("cpu"), 2.0, seed + 1) - 3.0     # behind row M - 1: finite, never to be read
        self.w, self.b = _rand((D,), torch.device("cpu"), 1.0, seed + 2), _rand((D,), torch.device("cpu"), 1.0, seed + 3)
        self.nrows = LN_PRE + M + c.tail + LN_POST
        r, col = torch.arange(self.nrows)[:, None], torch.arange(self.ldy)[None, :]
        self.owed = ((r >= LN_PRE) & (r < LN_PRE + M) & (col < D)).reshape(-1)
        self.zeros = ((r >= LN_PRE + M) & (r < LN_PRE + M + c.tail) & (col < D)).reshape(-1)

    @functools.cached_property
    def reference(self):
        return {o16: layernorm_bound(self.rows, self.w, self.b, self.case.eps, o16) for o16 in (True, False)}

    def x_view(self, buf):
        """x as the caller passes it: every row of the buffer, M given separately"""
        return torch.as_strided(buf, (self.case.M + LN_EXTRA, self.case.D), (self.ldx, 1), 0)

    def alloc(self, dtype):
        buf = _sentinel(self.nrows * self.ldy, dtype)
        buf[self.owed] = float("nan")
        return buf

    def out_view(self, buf):
        return torch.as_strided(buf, (self.case.M + self.case.tail, self.case.D), (self.ldy, 1), LN_PRE * self.ldy)

    def owed_view(self, buf):
        return torch.as_strided(buf, (self.case.M, self.case.D), (self.ldy, 1), LN_PRE * self.ldy)


@functools.lru_cache(maxsize=2)
def ln_buffers(case):
    return LNBuffers(case)


def ln_violations(lb, buf, out2=None, ref32=None):
    """buf: the output buffer after the call (any device). Everything not owed bit-equal to the prefill (zero-tail rows: +0), the owed
    elements finite and inside `layernorm_bound`, all-zero rows equal to b exactly; out2 (an fp32 buffer of the same layout, zero tail
    excepted) bit-equal to `ref32`, the owed part of the fp32 launch. -> (violations, worst |error| / bound)"""
    c = lb.case
    buf = buf.cpu()
    dt = buf.dtype
    it = torch.int16 if dt == torch.float16 else torch.int32
    exp = _sentinel(buf.numel(), dt)
    exp[lb.zeros] = 0.0
    rest = ~lb.owed
    bad = []
    ne = (buf.view(it) != exp.view(it)) & rest
    if bool(ne.any()):
        p = int(torch.nonzero(ne)[0])
        bad.append(f"{int(ne.sum())} elements outside the {c.M} x {c.D} owed block changed or zero-tail elements not +0; first: buffer row "
                   f"{p // lb.ldy - LN_PRE} (rows >= {c.M}: zero tail of {c.tail}, then guards), column {p % lb.ldy}: {buf[p].item()!r}")
    y, bound = lb.reference[dt == torch.float16]
    got = lb.owed_view(buf).double()
    fin = torch.isfinite(got)
    if not bool(fin.all()):
        m, n = (int(v) for v in torch.nonzero(~fin)[0])
        bad.append(f"{int((~fin).sum())} owed elements not finite (left unwritten, or the NaN padding of x read); first ({m}, {n})")
    err = torch.where(fin, (got - y).abs(), torch.zeros_like(y))
    over = err > bound
    tiny = bound.clamp_min(1e-300)
    ratio = (err / tiny).max().item()
    if bool(over.any()):
        m, n = (int(v) for v in torch.nonzero(over)[0])
        bad.append(f"{int(over.sum())} elements outside the bound, worst {ratio:.3f} times; first ({m}, {n}): got {got[m, n].item()!r}, "
                   f"float64 {y[m, n].item()!r}, bound {bound[m, n].item():.3e}")
    zr = (lb.rows == 0).all(1)
    if bool(zr.any()) and not torch.equal(lb.owed_view(buf)[zr], lb.b.to(dt)[None, :].expand(int(zr.sum()), c.D)):
        bad.append("an all-zero row is not b exactly")
    if out2 is not None:
        out2 = out2.cpu()
        e2 = _sentinel(out2.numel(), torch.float32)
        e2[lb.owed] = ref32.reshape(-1)
        n2 = out2.view(torch.int32) != e2.view(torch.int32)
        if bool(n2.any()):
            p = int(torch.nonzero(n2)[0])
            bad.append(f"out2: {int(n2.sum())} elements differ from the fp32 launch or from the prefill; first: row {p // lb.ldy - LN_PRE}, "
                       f"column {p % lb.ldy}")
    return bad, ratio


# the injected faults of tests/test_pointwise_reference_cpu.py; no fault ever reaches a kernel
LN_FAULTS = ("one_pass", "drop_last4", "eps_outside", "unbiased", "affine_shift4", "neighbour_mean", "tail_unwritten", "guard_column")


def ln_fault_applies(fault, c):
    """whether a correct check CAN see the fault at this case (the reasons: module docstring of tests/test_pointwise_reference_cpu.py)"""
    tight = c.regime in ("plain", "outlier")
    return {"one_pass": (c.regime == "offset" and c.M >= 3) or (c.regime == "mixed" and c.M >= 14),
            "drop_last4": c.regime != "zero",
            "eps_outside": (c.regime == "tinyvar" or (c.regime == "mixed" and c.M >= 4)) and (c.eps > 5e-6 or c.D <= 1024),
            "unbiased": (tight or (c.regime == "mixed" and c.M >= 3)) and (not c.out16 or c.D <= 256),
            "affine_shift4": c.D > 4,
            "neighbour_mean": c.M >= 2 and c.regime in ("plain", "outlier", "const", "mixed"),
            "tail_unwritten": c.tail > 0,
            "guard_column": c.ypad > 0}[fault]


def ln_emulate(lb, dtype, fault=None):
    """plain two-pass fp32 torch written into the case's guarded output buffer, with one fault on request"""
    c = lb.case
    x, w, b = lb.rows, lb.w, lb.b
    D = c.D
    xs = x[:, :D - 4] if fault == "drop_last4" else x
    mean = xs.sum(1, keepdim=True) / D
    if fault == "neighbour_mean":
        mean = torch.roll(mean, -1, 0)
    d = x - mean
    ds = d[:, :D - 4] if fault == "drop_last4" else d
    if fault == "one_pass":
        var = ((x * x).sum(1, keepdim=True) / D - mean * mean).clamp_min(0.0)
    else:
        var = (ds * ds).sum(1, keepdim=True) / (D - 1 if fault == "unbiased" else D)
    rstd = 1.0 / (torch.sqrt(var) + c.eps) if fault == "eps_outside" else 1.0 / torch.sqrt(var + c.eps)
    if fault == "affine_shift4":
        w, b = torch.roll(w, -4), torch.roll(b, -4)
    y = d * rstd * w + b
    buf = lb.alloc(dtype)
    lb.owed_view(buf).copy_(y.to(dtype))
    if c.tail and fault != "tail_unwritten":
        lb.out_view(buf)[c.M:] = 0.0
    if fault == "guard_column":
        buf[(LN_PRE + c.M - 1) * lb.ldy + D] = y[c.M - 1, 0].to(dtype)
    return buf
