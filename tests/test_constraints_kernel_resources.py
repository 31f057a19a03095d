"""CPU: the budget of the constrained-decoding kernels (csrc/constrain.hip), read from
libquantizations.so's gfx950 code-object metadata through test_kernel_resources.py's helpers:
k_constrain_logits for fp16 and bf16 and k_constraint_advance, no scratch, no spills, no AGPRs, and at
most 64 registers -- the siblings' cap: a thread of k_constrain_logits holds 8 classes, 8 logits and 8
bias entries."""
import pytest
from test_kernel_resources import _tools_ok, kernel_resources


@pytest.mark.skipif(not _tools_ok(), reason="libquantizations.so or the ROCm LLVM tools are missing")
def test_constraint_kernels_use_no_scratch():
    res = {n: r for n, r in kernel_resources().items() if "k_constrain_logits" in n or "k_constraint_advance" in n}
    print(res)
    assert len(res) == 3, sorted(res)
    assert sum("k_constrain_logits<" in n for n in res) == 2 and sum("k_constraint_advance" in n for n in res) == 1
    for name, (vgpr, agpr, priv, ssp, vsp) in res.items():
        assert priv == 0 and ssp == 0 and vsp == 0 and agpr == 0, (name, priv, ssp, vsp, agpr)
        assert vgpr <= 64, (name, vgpr)
