"""GPU: psam_layernorm (csrc/layernorm.hip) through ops.layernorm against float64 with the derived bound of oracle/pointwise.py
(`layernorm_bound`: a two-pass fp32 LayerNorm, with or without the fp16 rounding of the result), at the case table `ln_cases()`:
D off the 256-column lane pattern (4, 252, 260, 2044, 2048), ldx != D with NaN padding, ldy != D with sentinel guard columns, M smaller than
the buffer, zero tails that cross a workgroup, both output types, out2, and rows with |mean| >> std, outlier channels, a variance near eps,
constant and all-zero rows, and all of these interleaved. Everything the kernel does not owe is compared as integers; an all-zero row must
give b exactly; out2 must equal the fp32 launch bit for bit. tests/test_pointwise_reference_cpu.py shows plain two-pass fp32 torch inside
the bound at these very cases and eight injected faults outside. The refusals are asked of the C entry point and must leave the output
untouched; nothing misaligned or out of range is ever launched. PSAM_LN_REVERSE=1 (read once per process) runs in a child process whose
digest of the output bits must equal this process's. Run with -s for every ratio; measured: profiles/pointwise_tests.txt."""
import hashlib
import os
import subprocess
import sys

import pytest
import torch

from oracle import pointwise as P

pytestmark = pytest.mark.gpu


def _launch(dev, lb, out16, out2=False, x_dev=None):
    """ops.layernorm on the case's buffers: x with every row of its buffer and M given, `out` the guarded view -> (buffer, out2 buffer)"""
    from protosam_amd import ops
    c = lb.case
    dt = torch.float16 if out16 else torch.float32
    x = lb.x_view(lb.x_buf.to(dev)) if x_dev is None else x_dev
    buf = lb.alloc(dt).to(dev)
    buf2 = lb.alloc(torch.float32).to(dev) if out2 else None
    ops.layernorm(x, lb.w.to(dev), lb.b.to(dev), c.eps, out=lb.out_view(buf), out2=None if buf2 is None else lb.out_view(buf2),
                  zero_tail_rows=c.tail, M=c.M)
    torch.cuda.synchronize()
    return buf, buf2


def _run_case(dev, case):
    """the case as the table has it -> the bits of everything it wrote (for the digest)"""
    lb = P.ln_buffers(case)
    x = lb.x_view(lb.x_buf.to(dev))
    ref32 = None
    if case.out2:
        b32, _ = _launch(dev, lb, False, x_dev=x)
        ref32 = lb.owed_view(b32.cpu()).clone()
    buf, buf2 = _launch(dev, lb, case.out16, case.out2, x_dev=x)
    bad, ratio = P.ln_violations(lb, buf, buf2, ref32)
    print(f"layernorm {case.id}: worst |error| / bound = {ratio:.3f}")
    assert not bad, (case.id, bad)
    return buf.cpu().view(torch.int16 if case.out16 else torch.int32).numpy().tobytes() + (b"" if buf2 is None else buf2.cpu().numpy().tobytes())


@pytest.mark.parametrize("case", P.ln_cases(), ids=lambda c: c.id)
def test_layernorm_case(dev, case):
    _run_case(dev, case)


def _refused(lib, dev, M, D, ldx, ldy, out_dtype):
    """-> the status of a call the entry point must refuse before it launches; the buffers are large enough for any reading of the
    arguments and the output must come back untouched"""
    x = torch.zeros(8 * 4096, device=dev)
    w = torch.ones(4096, device=dev)
    y = torch.full((8 * 4096,), 7.0, device=dev)
    st = lib.psam_layernorm(x.data_ptr(), w.data_ptr(), w.data_ptr(), y.data_ptr(), 0, M, D, ldx, ldy, 1e-6, out_dtype, 0, 0)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()), (M, D, ldx, ldy)
    return st


def test_layernorm_refusals(dev):
    from protosam_amd import _lib
    lib = _lib.lib()
    for what, (M, D, ldx, ldy) in {"D % 4": (4, 258, 260, 260), "D = 2052": (4, 2052, 2052, 2052), "ldx % 4": (4, 256, 258, 256),
                                   "ldy % 4": (4, 256, 256, 258), "M = 0": (0, 256, 256, 256)}.items():
        for out_dtype in (0, 1):
            assert _refused(lib, dev, M, D, ldx, ldy, out_dtype) == 1, what


# ---- PSAM_LN_REVERSE ---------------------------------------------------------------------------------------------------
REVERSE_SUBSET = tuple(c for c in P.ln_cases() if c.M >= 5 and (c.D in (260, 2048) or c.M == 1297))


def _digest(dev):
    h = hashlib.sha256()
    for c in REVERSE_SUBSET:
        h.update(_run_case(dev, c))
    return h.hexdigest()


def test_layernorm_digest(dev):
    """the fixed subset of the cases (more than one workgroup of four rows each), checked, and the digest of the bits it wrote"""
    print(f"layernorm digest {_digest(dev)} reverse {os.environ.get('PSAM_LN_REVERSE', '0')}")


def test_layernorm_reverse_row_order_in_a_fresh_process(dev):
    """PSAM_LN_REVERSE=1 walks the rows from the last workgroup to the first: the same checks pass and every bit written is the same"""
    assert len(REVERSE_SUBSET) >= 8
    mine = _digest(dev)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "test_layernorm_digest"], cwd=root, env=dict(os.environ, PSAM_LN_REVERSE="1"), capture_output=True, text=True,
                       timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and " passed" in tail and "skipped" not in tail, tail
    line = [ln for ln in r.stdout.splitlines() if "layernorm digest " in ln]
    assert line and line[-1].split("layernorm digest ")[1].split() == [mine, "reverse", "1"], (mine, line)
