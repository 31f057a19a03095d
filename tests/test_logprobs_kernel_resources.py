"""CPU: the budget of the log-probability kernels (csrc/logprobs.hip), read from libquantizations.so's
gfx950 code-object metadata through test_kernel_resources.py's helpers: four instantiations
(k_logprobs_chunk and k_logprobs_final, fp16 / bf16), no scratch, no spills, no AGPRs, and at most 64
registers: both are 256-thread workgroups of small per-thread state (8 logits, 8 composites)."""
import pytest
from test_kernel_resources import _tools_ok, kernel_resources


@pytest.mark.skipif(not _tools_ok(), reason="libquantizations.so or the ROCm LLVM tools are missing")
def test_logprobs_kernels_use_no_scratch():
    res = {n: r for n, r in kernel_resources().items() if "k_logprobs" in n}
    print(res)
    assert len(res) == 4, sorted(res)
    assert sum("k_logprobs_chunk<" in n for n in res) == 2 and sum("k_logprobs_final<" in n for n in res) == 2
    for name, (vgpr, agpr, priv, ssp, vsp) in res.items():
        assert priv == 0 and ssp == 0 and vsp == 0 and agpr == 0, (name, priv, ssp, vsp, agpr)
        assert vgpr <= 64, (name, vgpr)
