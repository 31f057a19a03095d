"""CPU: the budget of the paged attention kernels (csrc/paged_attn.hip), read from
libquantizations.so's gfx950 code-object metadata: four instantiations of each (fp16 / bf16, D = 64 /
128), no scratch, no spills, no more LDS than the contiguous twin of the same dtype and head size, and
VGPR + AGPR <= 256 for the paged prefill kernel (two workgroups of 4 waves per CU, the contiguous
kernel's bar).  The counts are recorded in DESIGN."""
import os
import re
import subprocess
import tempfile

import pytest
from test_kernel_resources import LIB, LLVM, _tools_ok, code_objects

TWINS = {"k_paged_attn_streams<": "k_decode_attn_streams<", "k_paged_attn_verify<": "k_decode_attn_verify<",
         "k_paged_prefill_attn<": "k_prefill_attn<", "k_paged_kv_write<": "k_prefill_kv_write<"}


def _kernels():
    """{demangled name: (vgpr, agpr, private bytes, LDS bytes, sgpr spills, vgpr spills)}"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in code_objects(LIB, d):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True,
                                   text=True, check=True).stdout
            for ent in notes.split("  - .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", ent).group(1)

                def num(key, default=None):
                    m = re.search(rf"\.{key}:\s+(\d+)", ent)
                    return int(m.group(1)) if m else default
                out[name] = (num("vgpr_count"), int(ent.split("\n")[0].strip()), num("private_segment_fixed_size"),
                             num("group_segment_fixed_size"), num("sgpr_spill_count", 0), num("vgpr_spill_count", 0))
    dem = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True, check=True).stdout.split("\n")
    return {dm: out[n] for n, dm in zip(list(out), dem)}


def _targs(name):
    return re.search(r"<([^>]*)>", name.split("k_", 1)[1]).group(1)


@pytest.mark.skipif(not _tools_ok(), reason="libquantizations.so or the ROCm LLVM tools are missing")
def test_paged_kernels_fit_like_their_twins():
    res = _kernels()
    for paged, twin in TWINS.items():
        mine = {_targs(n): r for n, r in res.items() if paged in n}
        theirs = {_targs(n): r for n, r in res.items() if twin in n}
        print(paged, mine, twin, theirs)
        assert len(mine) == 4 and len(theirs) == 4, (paged, sorted(mine), sorted(theirs))
        assert sorted(mine) == sorted(theirs) == ["0, 128", "0, 64", "1, 128", "1, 64"]
        for ta, (vgpr, agpr, priv, lds, ssp, vsp) in mine.items():
            assert priv == 0 and ssp == 0 and vsp == 0, (paged, ta, priv, ssp, vsp)
            assert lds is not None and lds <= theirs[ta][3], (paged, ta, lds, theirs[ta][3])
            assert vgpr + agpr <= 256, (paged, ta, vgpr, agpr)
            if "prefill_attn" not in paged:
                assert agpr == 0, (paged, ta, agpr)
            if "kv_write" in paged:
                assert vgpr <= 64, (paged, ta, vgpr)
