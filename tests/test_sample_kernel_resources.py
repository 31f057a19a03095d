"""CPU: the budget of qz_sample_step's kernels (csrc/sample.hip), read from libquantizations.so's
gfx950 code-object metadata: no scratch, no spills, at most 64 KiB of LDS per workgroup, and the
1024-thread scan within the 128 VGPRs that let its 16 waves be resident."""
import os
import re
import subprocess
import tempfile

import pytest
from test_kernel_resources import LIB, LLVM, _tools_ok, code_objects

KERNELS = ("k_sample_hist", "k_sample_scan", "k_sample_chunk", "k_sample_final")


def _sample_kernels():
    """{demangled name: (vgpr, agpr, private bytes, LDS bytes, sgpr spills, vgpr spills)}"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in code_objects(LIB, d):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True,
                                   text=True, check=True).stdout
            for ent in notes.split("  - .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", ent).group(1)
                if "k_sample_" not in name:
                    continue

                def num(key, default=None):
                    m = re.search(rf"\.{key}:\s+(\d+)", ent)
                    return int(m.group(1)) if m else default
                out[name] = (num("vgpr_count"), int(ent.split("\n")[0].strip()), num("private_segment_fixed_size"),
                             num("group_segment_fixed_size"), num("sgpr_spill_count", 0), num("vgpr_spill_count", 0))
    dem = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True, check=True).stdout.split("\n")
    return {dm: out[n] for n, dm in zip(list(out), dem)}


@pytest.mark.skipif(not _tools_ok(), reason="libquantizations.so or the ROCm LLVM tools are missing")
def test_sample_kernels_use_no_scratch_and_little_lds():
    res = _sample_kernels()
    print(res)
    for k in KERNELS:
        found = [n for n in res if f"qz::{k}<" in n.replace("(anonymous namespace)::", "")]
        assert len(found) == 2, f"{k}: fp16 and bf16 instantiations, found {found}"
    for name, (vgpr, agpr, priv, lds, ssp, vsp) in res.items():
        assert priv == 0 and ssp == 0 and vsp == 0 and agpr == 0, (name, priv, ssp, vsp, agpr)
        assert lds is not None and lds <= 64 * 1024, (name, lds)
        assert vgpr <= (128 if "k_sample_scan" in name else 256), (name, vgpr)
