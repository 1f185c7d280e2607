"""CPU: the C-ABI library loads and exports every symbol declared in include/protosam_hip.h (no compute calls)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "protosam_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.findall(r"\bint\s+(psam_\w+)\s*\(", src)


def test_header_symbols_exported():
    from protosam_amd import _lib
    names = _declared()
    assert len(names) >= 25
    L = _lib.lib()
    for n in names:
        assert getattr(L, n) is not None
    assert set(names) == set(_lib.SIGNATURES), set(names) ^ set(_lib.SIGNATURES)


def test_header_compiles_as_c(tmp_path):
    import subprocess
    c = tmp_path / "t.c"
    c.write_text('#include "protosam_hip.h"\nint main(void){return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o",
                           str(tmp_path / "t.o")])


def test_arity_matches_header():
    """ctypes argtypes in protosam_amd/_lib.py have the same arity as the C prototypes."""
    from protosam_amd import _lib
    src = open(os.path.join(ROOT, "include", "protosam_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, args in re.findall(r"\bint\s+(psam_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        n = len([a for a in args.split(",") if a.strip()])
        assert n == len(_lib.SIGNATURES[name]), (name, n, len(_lib.SIGNATURES[name]))


def test_attention_kernel_ids_agree():
    """The ids psam_attention_last_kernel reports: the header's PSAM_ATTN_KERNEL_* macros, the enum csrc/attention.hip stores and
    the ops.ATTN_KERNEL_* constants carry the same numbers; families are distinct and fit the mask, the flags are single bits above
    it; the report is 0 in a process that has launched nothing."""
    from protosam_amd import ops
    hdr = open(os.path.join(ROOT, "include", "protosam_hip.h")).read()
    head = dict((n, int(v, 0)) for n, v in re.findall(r"#define\s+PSAM_ATTN_KERNEL_(\w+)\s+(0x[0-9a-fA-F]+|\d+)", hdr))
    src = open(os.path.join(ROOT, "protosam_amd", "csrc", "attention.hip")).read()
    body = re.search(r"enum\s*\{([^}]*AK_ATTN[^}]*)\}", src).group(1)
    lib = dict((n, int(v, 0)) for n, v in re.findall(r"\bAK_(\w+)\s*=\s*(0x[0-9a-fA-F]+|\d+)", body))
    py = {n[len("ATTN_KERNEL_"):]: v for n, v in vars(ops).items() if n.startswith("ATTN_KERNEL_") and isinstance(v, int)}
    assert len(head) == 15 and lib == {n: v for n, v in head.items() if n != "FAMILY"} and py == head, (head, lib, py)
    flags = {n: head[n] for n in ("FULL", "STAGE64", "QT4", "V2")}
    fams = {n: v for n, v in head.items() if n not in flags and n != "FAMILY"}
    assert sorted(fams.values()) == list(range(1, 11)) and set(fams.values()) == set(ops.ATTN_KERNEL_NAMES)
    assert all(v & (v - 1) == 0 and v > head["FAMILY"] for v in flags.values()) and len(set(flags.values())) == 4
    assert ops.attention_kernel_name(5 | 0x100 | 0x200) == "gattn_any_kernel+full+stage64"
    import subprocess
    import sys
    out = subprocess.check_output([sys.executable, "-c", "from protosam_amd import ops; print(ops.attention_last_kernel())"],
                                  cwd=ROOT)
    assert out.split()[-1] == b"0"


def test_missing_library_is_loud(monkeypatch):
    import importlib
    from protosam_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libprotosam_hip.so")
    try:
        _lib.lib()
        raise AssertionError("expected HipExtensionMissing")
    except _lib.HipExtensionMissing:
        pass


def test_product_never_imports_oracle():
    import glob
    for f in glob.glob(os.path.join(ROOT, "protosam_amd", "**", "*.py"), recursive=True):
        txt = open(f).read()
        assert "import oracle" not in txt and "from oracle" not in txt, f


def test_cpu_tensor_is_rejected():
    import pytest
    import torch
    from protosam_amd import ops
    with pytest.raises(RuntimeError):
        ops.gemm(torch.zeros((128, 64), dtype=torch.float16), torch.zeros((128, 64), dtype=torch.float16))
