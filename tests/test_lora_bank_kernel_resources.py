"""CPU: the kernels of the adapter-bank route (k_gemv_4bit_mt_grouped_lora in gemm_mt.hip,
k_lora_shrink_mt in lora.hip), read from libquantizations.so's gfx950 code objects as
tests/test_kernel_resources.py reads the decode GEMVs: no scratch, no spills, no AGPR use, and each
multi-token kernel in the occupancy class of its plain twin k_gemv_4bit_mt_grouped<same arguments>
(the expand lives in the epilogue, after the accumulators are dead: it must not cost a wave)."""
import pytest
from test_kernel_resources import _targs, _tools_ok, kernel_resources


def _base(name):
    return name.split("<")[0].replace("void ", "").strip()


def _waves_per_simd(vgpr):
    """gfx950: 512 VGPRs per SIMD lane, allocated in blocks of 8, at most 8 waves."""
    return min(8, 512 // (8 * ((max(vgpr, 1) + 7) // 8)))


@pytest.mark.skipif(not _tools_ok(), reason="libquantizations.so or the ROCm LLVM tools are missing")
def test_bank_multi_token_kernels_match_their_plain_twins():
    res = kernel_resources()
    plain = {tuple(_targs(k)): v for k, v in res.items() if _base(k) == "qz::k_gemv_4bit_mt_grouped"}
    bank = {tuple(_targs(k)): v for k, v in res.items() if _base(k) == "qz::k_gemv_4bit_mt_grouped_lora"}
    # quant type x double quant x dtype x token bucket
    assert len(plain) == 32 and set(bank) == set(plain), (len(plain), len(bank))
    for args, (vgpr, agpr, priv, ssp, vsp) in bank.items():
        assert agpr == 0 and priv == 0 and ssp == 0 and vsp == 0, (args, vgpr, agpr, priv, ssp, vsp)
        assert _waves_per_simd(vgpr) >= _waves_per_simd(plain[args][0]), (args, vgpr, plain[args][0])


@pytest.mark.skipif(not _tools_ok(), reason="libquantizations.so or the ROCm LLVM tools are missing")
def test_shrink_mt_kernels_for_both_dtypes():
    res = kernel_resources()
    shrink = {tuple(_targs(k)): v for k, v in res.items() if _base(k) == "qz::k_lora_shrink_mt"}
    assert set(shrink) == {("0",), ("1",)}, sorted(shrink)               # QZ_DT_F16, QZ_DT_BF16
    for args, (vgpr, agpr, priv, ssp, vsp) in shrink.items():
        assert agpr == 0 and priv == 0 and ssp == 0 and vsp == 0 and vgpr <= 64, (args, vgpr, agpr, priv, ssp, vsp)


@pytest.mark.skipif(not _tools_ok(), reason="libquantizations.so or the ROCm LLVM tools are missing")
def test_previously_pinned_kernel_names_are_still_in_the_library():
    res = kernel_resources()
    picks = [
        "qz::k_gemv_4bit_pair<true, 0, 4, true, true, true, true, true>",
        "qz::k_gemv_4bit<true, 0, 2, 1, 8, true, true, true, false, 0>",
        "qz::k_gemv_4bit_grouped<true, 0, 2, 1, true, true, true, true>",
        "qz::k_gemv_4bit<true, 0, 2, 1, 4, true, true, false, true, 0>",
        "qz::k_gemv_4bit_grouped_lora<true, 0, 2, 1, true, true, true, true>",
        "qz::k_gemv_4bit_grouped_lora<true, 0, 4, 1, true, true, true, true>",
        "qz::k_gemv_4bit_lora<true, 0, 2, 1, 4, true, true, false, true>",
        "qz::k_gemv_4bit_lora<true, 0, 2, 1, 8, true, true, true, false>",
    ]
    for p in picks:
        assert any(p in k for k in res), f"{p} not in the library"
    bases = {_base(k) for k in res}
    for b in ("qz::k_gemv_4bit_mt", "qz::k_gemv_4bit_mt_grouped", "qz::k_lora_shrink"):
        assert b in bases, f"{b} not in the library"
    # the plain multi-token kernels keep their template arity (the adapter flag is mt_body's, not theirs)
    assert all(len(_targs(k)) == 5 for k in res if _base(k) == "qz::k_gemv_4bit_mt")
    assert all(len(_targs(k)) == 4 for k in res if _base(k) == "qz::k_gemv_4bit_mt_grouped")
