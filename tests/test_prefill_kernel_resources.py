"""CPU: the budget of the prefill attention's kernels (csrc/prefill_attn.hip), read from
libquantizations.so's gfx950 code-object metadata through test_kernel_resources.kernel_resources: four
instantiations of k_prefill_attn and of k_prefill_kv_write (fp16 / bf16, D = 64 / 128), no scratch, no
SGPR / VGPR spills, and the LDS of one workgroup within the 64 KiB a workgroup may declare statically
(160 KiB per CU: D = 128 leaves room for three workgroups).  AGPRs are allowed in the attention: the
fp32 accumulators may live there.  The counts are recorded in DESIGN."""
import os
import re
import subprocess
import tempfile

import pytest
from test_kernel_resources import LIB, LLVM, _tools_ok, code_objects, kernel_resources


def _lds():
    """{mangled name: group_segment_fixed_size} of the prefill kernels."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in code_objects(LIB, d):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True,
                                   text=True, check=True).stdout
            for ent in notes.split("  - .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", ent).group(1)
                if "k_prefill_attn" in name:
                    out[name] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", ent).group(1))
    return out


@pytest.mark.skipif(not _tools_ok(), reason="libquantizations.so or the ROCm LLVM tools are missing")
def test_prefill_kernels_use_no_scratch_and_fit_a_workgroups_lds():
    res = kernel_resources()
    attn = {n: r for n, r in res.items() if "k_prefill_attn<" in n}
    write = {n: r for n, r in res.items() if "k_prefill_kv_write<" in n}
    lds = _lds()
    print(attn, write, lds)
    assert len(attn) == 4 and len(write) == 4 and len(lds) == 4, (sorted(attn), sorted(write), sorted(lds))
    for name, (vgpr, agpr, priv, ssp, vsp) in attn.items():
        assert priv == 0 and ssp == 0 and vsp == 0, (name, priv, ssp, vsp)
        assert vgpr + agpr <= 256, (name, vgpr, agpr)          # two workgroups of 4 waves per CU at least
    for name, (vgpr, agpr, priv, ssp, vsp) in write.items():
        assert priv == 0 and ssp == 0 and vsp == 0 and agpr == 0, (name, priv, ssp, vsp, agpr)
        assert vgpr <= 64, (name, vgpr)
    for name, size in lds.items():
        assert 0 < size <= 64 * 1024, (name, size)
