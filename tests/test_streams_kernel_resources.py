"""CPU: the budget of the per-stream decode attention (k_decode_attn_streams, csrc/layer_ops.hip),
read from libquantizations.so's gfx950 code-object metadata as test_sample_kernel_resources.py
reads the sampler's: four instantiations (fp16 / bf16, D = 64 / 128), no scratch, no spills, and no
more LDS than the shared-position kernel of the same dtype and head size.  The streams picks launch
the existing kernels, whose budget test_sample_kernel_resources.py already holds."""
import os
import re
import subprocess
import tempfile

import pytest
from test_kernel_resources import LIB, LLVM, _tools_ok, code_objects


def _attn_kernels():
    """{demangled name: (vgpr, agpr, private bytes, LDS bytes, sgpr spills, vgpr spills)}"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in code_objects(LIB, d):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True,
                                   text=True, check=True).stdout
            for ent in notes.split("  - .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", ent).group(1)
                if "k_decode_attn" not in name or "combine" in name:
                    continue

                def num(key, default=None):
                    m = re.search(rf"\.{key}:\s+(\d+)", ent)
                    return int(m.group(1)) if m else default
                out[name] = (num("vgpr_count"), int(ent.split("\n")[0].strip()), num("private_segment_fixed_size"),
                             num("group_segment_fixed_size"), num("sgpr_spill_count", 0), num("vgpr_spill_count", 0))
    dem = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True, check=True).stdout.split("\n")
    return {dm: out[n] for n, dm in zip(list(out), dem)}


@pytest.mark.skipif(not _tools_ok(), reason="libquantizations.so or the ROCm LLVM tools are missing")
def test_streams_attention_uses_no_scratch_and_no_more_lds():
    res = _attn_kernels()
    print(res)
    streams = {n: r for n, r in res.items() if "k_decode_attn_streams<" in n}
    shared = {n: r for n, r in res.items() if "k_decode_attn<" in n}
    assert len(streams) == 4 and len(shared) == 4, (sorted(streams), sorted(shared))
    for name, (vgpr, agpr, priv, lds, ssp, vsp) in streams.items():
        twin = name.replace("k_decode_attn_streams<", "k_decode_attn<")
        assert twin in shared, (name, sorted(shared))
        assert priv == 0 and ssp == 0 and vsp == 0 and agpr == 0, (name, priv, ssp, vsp, agpr)
        assert lds is not None and lds <= shared[twin][3], (name, lds, shared[twin][3])
        assert vgpr <= 256, (name, vgpr)
