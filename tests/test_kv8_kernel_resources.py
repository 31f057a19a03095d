"""CPU: the budget of the kv8 attention kernels (csrc/paged_attn.hip), read from
libquantizations.so's gfx950 code-object metadata in the manner of test_paged_kernel_resources.py:
four instantiations of each (fp16 / bf16, D = 64 / 128), no scratch, no spills, no more LDS than the
16-bit paged twin of the same dtype and head size, VGPR + AGPR <= 256, and no AGPRs outside the
prefill kernel.  The counts are recorded in DESIGN."""
import pytest
from test_kernel_resources import _tools_ok
from test_paged_kernel_resources import _kernels, _targs

TWINS = {"k_kv8_attn_streams<": "k_paged_attn_streams<", "k_kv8_attn_verify<": "k_paged_attn_verify<",
         "k_kv8_prefill_attn<": "k_paged_prefill_attn<", "k_kv8_kv_write<": "k_paged_kv_write<"}


@pytest.mark.skipif(not _tools_ok(), reason="libquantizations.so or the ROCm LLVM tools are missing")
def test_kv8_kernels_fit_like_their_twins():
    res = _kernels()
    for kv8, twin in TWINS.items():
        mine = {_targs(n): r for n, r in res.items() if kv8 in n}
        theirs = {_targs(n): r for n, r in res.items() if twin in n}
        print(kv8, mine, twin, theirs)
        assert len(mine) == 4 and len(theirs) == 4, (kv8, sorted(mine), sorted(theirs))
        assert sorted(mine) == sorted(theirs) == ["0, 128", "0, 64", "1, 128", "1, 64"]
        for ta, (vgpr, agpr, priv, lds, ssp, vsp) in mine.items():
            assert priv == 0 and ssp == 0 and vsp == 0, (kv8, ta, priv, ssp, vsp)
            assert lds is not None and lds <= theirs[ta][3], (kv8, ta, lds, theirs[ta][3])
            assert vgpr + agpr <= 256, (kv8, ta, vgpr, agpr)
            if "prefill_attn" not in kv8:
                assert agpr == 0, (kv8, ta, agpr)
            if "kv_write" in kv8:
                assert vgpr <= 64, (kv8, ta, vgpr)
