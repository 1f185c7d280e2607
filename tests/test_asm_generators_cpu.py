"""No GPU: the text of the assembly kernels, pinned byte for byte.

protosam_amd/csrc/gemm_asm_gen.py (with gemm_asm2_gen.py, gattn_asm_gen.py and wattn_asm_gen.py behind it) writes the one assembly
module of the library. tests/golden/asm_kernels_sha256.json holds the SHA-256 of that module, of the header `--meta` writes and of
every kernel in it (its lines from the section directive in front of its entry label through the one behind its descriptor, plus
its entry of the metadata), recorded from the generators as they stood while they still carried their numbered ablation schedules:
the default run, `--meta`, and the `--experiments` run whose `_v1` kernels are today's `--trace` ones. So a change to a generator
that is meant to leave a kernel alone shows here, per kernel, before anything is built or run.

The generators are run the way the Makefile runs them, in a child process, and the result is hashed and assembled: nothing else.
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "protosam_amd", "csrc")
GOLDEN = json.load(open(os.path.join(HERE, "golden", "asm_kernels_sha256.json")))
CLANG = os.environ.get("CLANG") or "/opt/rocm/lib/llvm/bin/clang"        # the Makefile's

TRACED = tuple("psam_gemm_asm%s_%s%s_v1" % (two, epi, m16) for two, m16 in (("", ""), ("", "_m16"), ("2", "")) for epi in ("f16", "gelu", "f32"))
# what the generators once read from the build's environment, each at a value that changed their output
FORMER_SWITCHES = {"PSAM_GEN_GEMM_DMA": "nt,nt", "PSAM_GEN_GELU": "packed", "PSAM_GEN_GATTN_ABLATE": "nobar", "PSAM_GEN_GATTN_LAZYMAX": "0",
                   "PSAM_GEN_GATTN_RH_AT": "phase1", "PSAM_GEN_GATTN_DMA_AT": "decision", "PSAM_GEN_GATTN_LATE": "2,3",
                   "PSAM_GEN_WATTN_ABLATE": "nobar", "PSAM_GEN_WATTN_LAZYMAX": "0"}


def generate(*flags, csrc=CSRC, env=None):
    """stdout of `python gemm_asm_gen.py <flags>` run in `csrc`, in an environment that holds nothing but PATH and `env`"""
    r = subprocess.run([sys.executable, "-B", "gemm_asm_gen.py"] + list(flags), cwd=csrc, capture_output=True,
                       env=dict({"PATH": os.environ.get("PATH", "")}, **(env or {})))
    assert r.returncode == 0, r.stderr.decode()[-4000:]
    return r.stdout


def sha256(data):
    return hashlib.sha256(data).hexdigest()


def kernel_digests(module):
    """kernel name -> SHA-256 of its text: the lines `.text` ... `.end_amdhsa_kernel`, `.text` that asm_common.kernel_begin /
    kernel_end put around it, then its entry `  - .name: <kernel>` ... of the metadata; in the module's order"""
    lines = module.decode().split("\n")
    body, meta = {}, {}
    i = 0
    while i < len(lines):
        if lines[i] == ".text" and i + 1 < len(lines) and lines[i + 1].startswith(".protected "):
            name = lines[i + 1].split()[1]
            end = lines.index(".end_amdhsa_kernel", i)
            assert lines[end + 1] == ".text" and name not in body
            body[name] = lines[i:end + 2]
            i = end + 2
        elif lines[i].startswith("  - .name: "):
            name = lines[i].split()[-1]
            end = i + 1
            while not lines[end].startswith("  - .name: ") and lines[end] != "...":
                end += 1
            assert name not in meta
            meta[name] = lines[i:end]
            i = end
        else:
            i += 1
    assert list(body) == list(meta)
    return {k: sha256(("\n".join(body[k] + meta[k]) + "\n").encode()) for k in body}


@pytest.fixture(scope="module")
def default_module():
    return generate()


@pytest.fixture(scope="module")
def trace_module():
    return generate("--trace")


def test_default_module_is_the_recorded_one(default_module):
    assert sha256(default_module) == GOLDEN["module"]
    assert sha256(generate("--meta")) == GOLDEN["meta_header"]
    got = kernel_digests(default_module)
    assert len(GOLDEN["kernels"]) == 25 and got == GOLDEN["kernels"]


def test_trace_module_adds_the_nine_traced_kernels(trace_module):
    got = kernel_digests(trace_module)
    assert len(GOLDEN["traced"]) == 9 and sorted(GOLDEN["traced"]) == sorted(TRACED)
    assert set(got) == set(GOLDEN["kernels"]) | set(TRACED) and len(got) == 34
    assert {k: got[k] for k in GOLDEN["kernels"]} == GOLDEN["kernels"]
    assert {k: got[k] for k in TRACED} == GOLDEN["traced"]
    assert sha256(generate("--meta", "--trace")) == GOLDEN["meta_header"]


def test_build_environment_does_not_reach_the_text(default_module, trace_module):
    assert len(FORMER_SWITCHES) == 9
    assert generate(env=FORMER_SWITCHES) == default_module
    assert generate("--trace", env=FORMER_SWITCHES) == trace_module
    assert generate("--meta", env=FORMER_SWITCHES) == generate("--meta")


def test_two_runs_give_the_same_bytes(default_module, trace_module):
    assert generate() == default_module
    assert generate("--trace") == trace_module


@pytest.mark.skipif(shutil.which(CLANG) is None, reason="no AMDGPU assembler (%s)" % CLANG)
def test_both_modules_assemble(default_module, trace_module, tmp_path):
    for name, text in (("default", default_module), ("trace", trace_module)):
        src, obj = tmp_path / (name + ".s"), tmp_path / (name + ".o")
        src.write_bytes(text)
        r = subprocess.run([CLANG, "-x", "assembler", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950", "-c", str(src), "-o", str(obj)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        assert obj.stat().st_size > len(text) // 16
