"""CPU: the budget of qz_verify_sample_step_streams' own kernel (csrc/sample.hip), read from
libquantizations.so's gfx950 code-object metadata through test_kernel_resources' helpers: one
k_verify_sample_accept, no scratch, no spills, no AGPRs, at most 64 VGPRs.  The five kernels it shares
with qz_sample_step keep the budget of test_sample_kernel_resources.py, which counts their
instantiations: the rows-per-stream mapping is a run-time operand, not a template parameter."""
import pytest
from test_kernel_resources import _tools_ok, kernel_resources


@pytest.mark.skipif(not _tools_ok(), reason="libquantizations.so or the ROCm LLVM tools are missing")
def test_the_accept_kernel_uses_no_scratch_and_few_registers():
    res = kernel_resources()
    accept = {n: r for n, r in res.items() if "k_verify_sample_accept" in n}
    print(accept)
    assert len(accept) == 1, sorted(accept)
    for name, (vgpr, agpr, priv, ssp, vsp) in accept.items():
        assert priv == 0 and ssp == 0 and vsp == 0 and agpr == 0, (name, priv, ssp, vsp, agpr)
        assert vgpr <= 64, (name, vgpr)


@pytest.mark.skipif(not _tools_ok(), reason="libquantizations.so or the ROCm LLVM tools are missing")
def test_the_shared_kernels_gained_no_instantiation():
    res = kernel_resources()
    for k in ("k_sample_hist<", "k_sample_scan<", "k_sample_chunk<", "k_sample_final<"):
        found = [n for n in res if k in n]
        assert len(found) == 2, (k, found)
        for n in found:
            vgpr, agpr, priv, ssp, vsp = res[n]
            assert priv == 0 and ssp == 0 and vsp == 0 and agpr == 0, (n, priv, ssp, vsp, agpr)
