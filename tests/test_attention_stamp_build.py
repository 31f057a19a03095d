"""CPU: the decode attention stamps live in the measurement-only library alone.

libqz_diag.so (csrc/diag_stamps.hip, built with QZ_STAMPS) exports qz_diag_decode_attn_stamped, and its
kernel reads the clock at the head's seven points.  libquantizations.so contains no stamp code: no
decode attention kernel of it reads the clock, and each has the instruction count of layer_ops.hip
compiled on its own with the product's flags -- the build of the diag target beside it changes nothing
in it.  Read from the libraries' gfx950 code objects; no GPU needed."""
import os
import re
import subprocess
import tempfile

import pytest
from test_kernel_resources import LIB, LLVM, REPO, _tools_ok, code_objects

DIAG = os.path.join(REPO, "quantizations_amd", "libqz_diag.so")
CSRC = os.path.join(REPO, "quantizations_amd", "csrc")
OBJDUMP = os.path.join(LLVM, "llvm-objdump")
HIPCC = "/opt/rocm/bin/hipcc"


def _ok():
    return _tools_ok() and os.path.exists(DIAG) and os.path.exists(OBJDUMP)


def _kernels(co, want):
    """{symbol: [instruction mnemonics]} of the functions of code object `co` whose name contains `want`."""
    text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in text.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1) if want in m.group(1) else None
            if cur:
                out[cur] = []
            continue
        if cur and line.startswith("\t"):
            mnem = line.split("//")[0].split()
            if mnem and mnem[0] not in ("s_nop", "s_code_end"):      # padding behind s_endpgm
                out[cur].append(mnem[0])
    return out


def _lib_kernels(lib, want):
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in code_objects(lib, d):
            out.update(_kernels(co, want))
    return out


@pytest.mark.skipif(not _ok(), reason="the libraries or the ROCm LLVM tools are missing")
def test_diag_library_exports_the_stamped_attention():
    syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--dyn-syms", DIAG], capture_output=True, text=True,
                          check=True).stdout
    assert re.search(r"\bFUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+qz_diag_decode_attn_stamped\b", syms), "not exported"
    k = _lib_kernels(DIAG, "k_diag_decode_attn")
    assert len(k) == 1, sorted(k)
    clocks = [m for m in next(iter(k.values())) if m == "s_memrealtime"]
    # seven points in each of the head's two forms (caches up to / past the early-load length)
    assert len(clocks) == 14, len(clocks)


@pytest.mark.skipif(not _ok(), reason="the libraries or the ROCm LLVM tools are missing")
def test_product_attention_kernels_hold_no_stamp_code():
    prod = {n: v for n, v in _lib_kernels(LIB, "_attn").items()
            if any(s in n for s in ("k_decode_attn", "k_paged_attn", "k_kv8_attn"))}
    assert len(prod) >= 28, sorted(prod)    # shared, streams, verify, combine + paged / kv8 streams and verify, x4
    for name, ins in prod.items():
        assert "s_memrealtime" not in ins and "s_memtime" not in ins, name
    # layer_ops.hip compiled alone, with the Makefile's flags and no diag target anywhere near it
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS\s*:=\s*(.*?)(?<!\\)\n", mk, re.S | re.M).group(1).replace("\\\n", " ")
    flags = flags.replace("$(ARCH)", "gfx950").split()
    assert not any("QZ_STAMPS" in f for f in flags)
    with tempfile.TemporaryDirectory() as d:
        obj = os.path.join(d, "layer_ops.o")
        subprocess.run([HIPCC] + flags + ["--cuda-device-only", "--no-gpu-bundle-output", "-c",
                                          os.path.join(CSRC, "layer_ops.hip"), "-o", obj],
                       check=True, capture_output=True)
        alone = _kernels(obj, "k_decode_attn")
    assert len(alone) == 16, sorted(alone)
    for name, ins in alone.items():
        assert name in prod, name
        assert len(ins) == len(prod[name]), (name, len(ins), len(prod[name]))
