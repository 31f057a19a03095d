"""CPU: the budget of qz_logits_process' kernel (csrc/logits.hip), read from libquantizations.so's
gfx950 code-object metadata through test_kernel_resources.py's helpers: eight instantiations (fp16 /
bf16; the table in 16, 64 or 128 KiB of LDS, or in the workspace), no scratch, no spills, no AGPRs, and at most 64 registers:
a workgroup is 16 waves (the launch is latency-bound glue in front of the pick) and two must fit a CU."""
import pytest
from test_kernel_resources import _tools_ok, kernel_resources


@pytest.mark.skipif(not _tools_ok(), reason="libquantizations.so or the ROCm LLVM tools are missing")
def test_logits_process_kernels_use_no_scratch():
    res = {n: r for n, r in kernel_resources().items() if "k_logits_process<" in n}
    print(res)
    assert len(res) == 8, sorted(res)
    for name, (vgpr, agpr, priv, ssp, vsp) in res.items():
        assert priv == 0 and ssp == 0 and vsp == 0 and agpr == 0, (name, priv, ssp, vsp, agpr)
        assert vgpr <= 64, (name, vgpr)
