"""CPU: the budget of the verify window's kernels (csrc/layer_ops.hip), read from libquantizations.so's
gfx950 code-object metadata as test_streams_kernel_resources.py reads the streams kernel's: four
instantiations of k_decode_attn_verify and of k_verify_kv_write (fp16 / bf16, D = 64 / 128), the pick's
k_verify_final and the drafter's k_ngram_draft -- no scratch, no spills, no AGPRs, and for the
attention no more LDS than the streams kernel of the same dtype and head size (the same head, one
flag more)."""
import pytest
from test_kernel_resources import _tools_ok, kernel_resources
from test_streams_kernel_resources import _attn_kernels


@pytest.mark.skipif(not _tools_ok(), reason="libquantizations.so or the ROCm LLVM tools are missing")
def test_verify_attention_uses_no_scratch_and_no_more_lds_than_streams():
    res = _attn_kernels()
    print(res)
    verify = {n: r for n, r in res.items() if "k_decode_attn_verify<" in n}
    streams = {n: r for n, r in res.items() if "k_decode_attn_streams<" in n}
    assert len(verify) == 4 and len(streams) == 4, (sorted(verify), sorted(streams))
    for name, (vgpr, agpr, priv, lds, ssp, vsp) in verify.items():
        twin = name.replace("k_decode_attn_verify<", "k_decode_attn_streams<").replace("DecodeAttnArgs, int)", "DecodeAttnArgs)")
        assert twin in streams, (name, sorted(streams))
        assert priv == 0 and ssp == 0 and vsp == 0 and agpr == 0, (name, priv, ssp, vsp, agpr)
        assert lds is not None and lds <= streams[twin][3], (name, lds, streams[twin][3])
        assert vgpr <= streams[twin][0], (name, vgpr, streams[twin][0])   # it loads and rotates less


@pytest.mark.skipif(not _tools_ok(), reason="libquantizations.so or the ROCm LLVM tools are missing")
def test_the_small_verify_kernels_use_no_scratch():
    res = kernel_resources()
    small = {n: r for n, r in res.items() if any(k in n for k in ("k_verify_kv_write<", "k_verify_final", "k_ngram_draft"))}
    print(small)
    assert sum("k_verify_kv_write<" in n for n in small) == 4
    assert sum("k_verify_final" in n for n in small) == 1 and sum("k_ngram_draft" in n for n in small) == 1
    for name, (vgpr, agpr, priv, ssp, vsp) in small.items():
        assert priv == 0 and ssp == 0 and vsp == 0 and agpr == 0, (name, priv, ssp, vsp, agpr)
        assert vgpr <= 64, (name, vgpr)
