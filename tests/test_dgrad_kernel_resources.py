"""CPU: the fused dgrad kernel's instantiations (csrc/gemm_dgrad.hip), read from
libquantizations.so's gfx950 code objects: every (quant type, double quant, dtype, token tile) is in
the library, and none uses scratch or spills a register."""
import itertools

import pytest

from test_kernel_resources import _targs, _tools_ok, kernel_resources


@pytest.mark.skipif(not _tools_ok(), reason="libquantizations.so or the ROCm LLVM tools are missing")
def test_dgrad_kernels_present_without_scratch_or_spills():
    found = {}
    for name, res in kernel_resources().items():
        base = name.split("<")[0].replace("void ", "").strip()
        if base == "qz::k_gemm_4bit_dgrad":
            found[tuple(_targs(name))] = res
    # <QT (FP4 = 0, NF4 = 1), DQ, DT (F16 = 0, BF16 = 1), BT>
    want = {(qt, dq, dt, bt) for qt, dq, dt, bt in itertools.product("01", ("false", "true"), "01", ("64", "128"))}
    assert set(found) == want, sorted(set(found) ^ want)
    for targs, (vgpr, agpr, priv, ssp, vsp) in found.items():
        assert priv == 0 and ssp == 0 and vsp == 0, (targs, vgpr, agpr, priv, ssp, vsp)
        assert vgpr <= 256, (targs, vgpr)      # two workgroups (8 waves) per CU fit beside the 64 KiB of LDS
