"""No GPU: the checks of oracle/pointwise.py are not tuned on a kernel and cannot be passed by a wrong one.

GELU. fp32 F.gelu rounded to fp16 and fp32 numpy emulations of both shipped operation sequences (common.h gelu_erf; gelu_quad of
csrc/gemm_asm_gen.py, with the constants READ from the generator) stay inside 3.4e-6 + 2^-11 |y| and pass every structural check over the
whole grid and both tail sets; seven wrong GELUs fail, each on the set where it is wrong.

LayerNorm. Plain two-pass fp32 torch stays inside `layernorm_bound` at every case tests/test_layernorm_gpu.py runs, for both output types;
eight injected faults fail at every case where the fault exists and a bound derived for a correct two-pass kernel can see it
(`ln_fault_applies`):
  * one_pass: E[x^2] - mean^2 errs by u mean^2: visible where |mean| >> std (`offset`, and `mixed`, which holds such rows). It is a rounding
    error, so a single row can come out anywhere below that: the fault is asked of cases with at least three such rows;
  * drop_last4: not on all-zero rows;
  * eps_outside: 1 / (sqrt(var) + eps) differs from 1 / sqrt(var + eps) only where var is of the order of eps (`tinyvar`; `mixed`): by
    41 % at eps = 1e-6 and by a factor 3.3 at eps = 1e-5. The bound's worst-case error of the mean, gamma_(D+1) 5, grows to 0.6 of the
    std 1e-3 of such a row at D = 2048 and then allows 56 % on the variance term: the 41 % are asked for up to D = 1024 only;
  * unbiased: rstd off by 1 / 2D relative: against H = 2^-11 only up to D = 256, against the fp32 bound at every D - but only in the regimes
    whose bound is tight (`plain`, `outlier`): the bound of `offset`, `tinyvar` and `const` rows is dominated by the worst-case error of
    the mean and is wider than 1 / 2D;
  * affine_shift4: a rotation by four columns is the identity at D = 4;
  * neighbour_mean: needs a second row, and rows whose means differ by more than the bound allows (not `offset` / `tinyvar` / `zero`);
  * tail_unwritten / guard_column: where there is a zero tail / a guard column."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pointwise as P


def _sets():
    return [(name, P.gelu_x(c, d)) for name, (c, d) in P.gelu_sets().items()]


def test_gelu_sets_are_what_the_kernels_are_owed():
    sets = dict(_sets())
    assert P.gelu_grid().dtype == torch.float32 and torch.equal(P.gelu_grid().double(), sets["grid"])
    g = sets["grid"].reshape(-1).sort().values
    assert g[0].item() == -32.0 and g[-1].item() == 32.25 - 2.0 ** -10 and torch.equal(g[1:] - g[:-1], torch.full((g.numel() - 1,), 2.0 ** -10,
                                                                                                                 dtype=torch.float64))
    rows = sets["tail-rows"]
    for c in (64, 128, 512, 4096, 32768):
        for s in (1, -1):
            assert bool(((rows[:, 0] == s * c) & (rows[:, 255] == s * c + 255)).any())
    assert rows.abs().max().item() <= 60000
    b = sets["tail-bias"]
    assert torch.equal(b, b[:1].expand_as(b))
    for v in P._SPECIAL:
        v = float(np.float32(v))
        assert bool((b[0] == v).any()) and bool((b[0] == -v).any())
    assert bool(torch.signbit(P.gelu_sets()["tail-bias"][1][len(P._SPECIAL)]))      # -0 is there as a bit pattern
    for x in sets.values():
        assert x.shape == (P.GELU_M, P.GELU_N) and torch.isfinite(x).all() and P.gelu_ref(x).abs().max().item() < 65504


def test_gelu_operands_realise_the_sets():
    for tile in P.GELU_TILES:
        K = P.gelu_min_k(tile)
        for name, (c, d) in P.gelu_sets().items():
            (_, a), (_, w), bias = P.gelu_operands(c, d, K)
            assert a.stride(0) == K + 64 and w.stride(0) == K + 8 and int((a != 0).sum(1).max()) <= 1
            assert torch.equal(a.double() @ w.double().t() + bias.double()[None, :], P.gelu_x(c, d))
    mr, s_ext = P.gelu_ln_operands(P.GELU_M, P.GELU_N)
    assert mr.numel() == 6 * P.GELU_M and s_ext.numel() == 5 * P.GELU_N and int(mr[2 * P.GELU_M:].abs().sum()) == 0
    assert torch.equal(mr[:2 * P.GELU_M].view(-1, 2), torch.tensor([0.0, 1.0]).expand(P.GELU_M, 2))


def test_sigpoly_constants_are_read_from_the_generator():
    c = P.sigpoly_constants()
    assert c.dtype == np.float32 and c.shape == (5,) and c[0] < 0 and np.all(np.isfinite(c))      # the leading coefficient: saturates the right way
    assert abs(float(c[4]) + 2.3022) < 1e-3       # -log2(e) * 2 sqrt(2 / pi) = -2.30220...: the slope of the logit of Phi at 0


REFERENCES = {"F.gelu fp32": lambda x: F.gelu(x.float()).half(),
              "A&S 7.1.26 sequence of common.h, fp32": P.emulate_gelu_erf,
              "sigmoid-polynomial of gemm_asm_gen.py, fp32": P.emulate_gelu_sigpoly}


@pytest.mark.parametrize("form", list(REFERENCES))
def test_gelu_references_stay_inside(form):
    for name, x in _sets():
        per = P.gelu_check(REFERENCES[form](x), x, f"{form}, {name}")
        assert max(r for r, _ in per.values()) <= 1.0


def _gelu32(x):
    return F.gelu(x.float())


def _tanh(x):
    return F.gelu(x.float(), approximate="tanh").half()


def _dip(x):
    y = _gelu32(x)
    return torch.where((x >= 11.0) & (x < 11.0 + 2.0 ** -6), y * 0.995, y).half()


def _flush(x):
    y = _gelu32(x).half()
    return torch.where(y.abs() < 2.0 ** -14, torch.zeros_like(y), y)


def _overflow(x):
    return torch.where(x.abs() > 13.0, torch.full_like(x, float("nan")), _gelu32(x).double()).half()


def _sign(x):
    y = _gelu32(x).half()
    return torch.where(x.abs() < 2.0 ** -10, -y, y)


GELU_FAULTS = {"tanh form": (_tanh, "grid"),
               "x sigmoid(1.702 x)": (lambda x: (x.float() * torch.sigmoid(1.702 * x.float())).half(), "grid"),
               "zero below -4": (lambda x: torch.where(x < -4.0, torch.zeros_like(x), _gelu32(x).double()).half(), "grid"),
               "0.5 % dip in [11, 11 + 2^-6)": (_dip, "grid"),
               "fp16 subnormal results flushed": (_flush, "tail-bias"),
               "NaN beyond |x| = 13": (_overflow, "tail-rows"),
               "sign flipped at the zero crossing": (_sign, "tail-bias")}


@pytest.mark.parametrize("fault", list(GELU_FAULTS))
def test_gelu_faults_fail(fault):
    fn, where = GELU_FAULTS[fault]
    failed = []
    for name, x in _sets():
        bad, per = P.gelu_report(fn(x), x)
        print(f"{fault}, {name}: worst |error| / bound = {max(r for r, _ in per.values()):.2f}; {bad[:1]}")
        if bad:
            failed.append(name)
        with pytest.raises(AssertionError) if bad else _none():
            P.gelu_check(fn(x), x, fault)
    assert where in failed, (fault, failed)


class _none:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


# ------------------------------------------------------------------------------------------------ LayerNorm
def test_ln_case_table_covers_the_issue():
    C = P.ln_cases()
    assert 40 <= len(C) <= 70 and len({c.id for c in C}) == len(C)
    assert {c.D for c in C} == set(P.LN_D) and {c.M for c in C} == set(P.LN_M) and {c.eps for c in C} == {1e-6, 1e-5}
    assert {c.xpad for c in C} == {0, 4, 64} and {c.ypad for c in C} == {0, 8}
    assert {(c.tail, c.out16) for c in C} == {(t, o) for t in (0, 1, 3, 6) for o in (True, False)}
    for D in (260, 2048):
        assert {c.regime for c in C if c.D == D} == set(P.LN_REGIMES)
    assert any(c.out2 for c in C) and all(c.out16 for c in C if c.out2)
    assert any(c.tail and (c.M % 4) + c.tail > 4 for c in C)                 # a zero tail that crosses a workgroup of four rows
    assert max(c.M * c.D for c in C) == 1297 * 2048
    for f in P.LN_FAULTS:
        assert sum(P.ln_fault_applies(f, c) for c in C) >= 4, f
    for D in (260, 2044):
        assert any(c.D == D and P.ln_fault_applies("drop_last4", c) for c in C)


@pytest.mark.parametrize("case", P.ln_cases(), ids=lambda c: c.id)
def test_ln_two_pass_fp32_stays_inside_and_faults_fail(case):
    lb = P.ln_buffers(case)
    assert torch.isnan(lb.x_buf).sum().item() == (case.M + P.LN_EXTRA) * case.xpad
    for dt in (torch.float16, torch.float32):
        bad, ratio = P.ln_violations(lb, P.ln_emulate(lb, dt))
        print(f"{case.id} two-pass fp32 torch -> {dt}: worst |error| / bound = {ratio:.3f}")
        assert not bad, bad
    dt = torch.float16 if case.out16 else torch.float32
    for f in P.LN_FAULTS:
        if P.ln_fault_applies(f, case):
            bad, ratio = P.ln_violations(lb, P.ln_emulate(lb, dt, f))
            print(f"{case.id} {f}: worst |error| / bound = {ratio:.2f}")
            assert bad, f
    ref32 = lb.owed_view(P.ln_emulate(lb, torch.float32)).clone()
    good2 = P._sentinel(lb.nrows * lb.ldy, torch.float32)
    good2[lb.owed] = ref32.reshape(-1)
    assert not P.ln_violations(lb, P.ln_emulate(lb, dt), good2, ref32)[0]
    good2[lb.owed.nonzero()[-1]] += 1e-3                                      # one element of out2 off
    assert P.ln_violations(lb, P.ln_emulate(lb, dt), good2, ref32)[0]


@pytest.mark.parametrize("D", P.LN_D)
def test_offset_regime_separates_one_pass_from_two_pass(D):
    """the `offset` rows at this D's c: the one-pass variance is outside the bound, two-pass fp32 inside, for both output types"""
    for o16 in (True, False):
        lb = P.LNBuffers(P.LNCase(D, 5, "offset", 1e-6, o16))
        dt = torch.float16 if o16 else torch.float32
        r2, r1 = P.ln_violations(lb, P.ln_emulate(lb, dt))[1], P.ln_violations(lb, P.ln_emulate(lb, dt, "one_pass"))[1]
        print(f"D = {D}, c = {P.offset_c(D):g}, {dt}: two-pass {r2:.3f}, one-pass {r1:.2f} times the bound")
        assert r2 <= 1.0 < r1


# ------------------------------------------------------------------------------------------------ ops.layernorm refuses a bad out2
class _Fake:
    """stands in for a device tensor: ops.layernorm must refuse before it asks for a pointer or calls the library"""

    def __init__(self, shape, dtype, stride0=None):
        self.shape, self.dtype, self.is_cuda, self._s0 = torch.Size(shape), dtype, True, stride0 or shape[-1]

    def dim(self):
        return len(self.shape)

    def stride(self, i):
        return 1 if i in (-1, len(self.shape) - 1) else self._s0

    def element_size(self):
        return 2 if self.dtype == torch.float16 else 4

    def data_ptr(self):
        raise AssertionError("ops.layernorm went on to the launch")


@pytest.mark.parametrize("why,out,out2", [
    ("fp32 out", _Fake((8, 64), torch.float32), _Fake((8, 64), torch.float32)),
    ("out2 not fp32", _Fake((8, 64), torch.float16), _Fake((8, 64), torch.float16)),
    ("row stride", _Fake((8, 64), torch.float16, 72), _Fake((8, 64), torch.float32)),
    ("rows", _Fake((8, 64), torch.float16), _Fake((7, 64), torch.float32)),
    ("columns", _Fake((8, 64), torch.float16), _Fake((8, 60), torch.float32, 64))])
def test_layernorm_refuses_a_bad_out2_on_the_host(why, out, out2):
    from protosam_amd import ops
    x, w = _Fake((8, 64), torch.float32), _Fake((64,), torch.float32)
    with pytest.raises(ValueError) as e:
        ops.layernorm(x, w, w, 1e-6, out=out, out2=out2)
    assert "out2" in str(e.value), (why, str(e.value))
