"""CPU: register budgets of the adapter-carrying decode kernels (lora.hip), read from
libquantizations.so's gfx950 code objects -- the budget tests/test_kernel_resources.py sets for the
plain decode GEMVs: 16-bit activations with up to 4 rows per wave fit the 256 architectural VGPRs
with no AGPR use, no scratch and no spills; the shrink kernel meets the same budget."""
import pytest
from test_kernel_resources import _targs, _tools_ok, kernel_resources


def _bad(vgpr, agpr, priv, ssp, vsp):
    return agpr > 0 or priv > 0 or vgpr > 256 or vsp or ssp


@pytest.mark.skipif(not _tools_ok(), reason="libquantizations.so or the ROCm LLVM tools are missing")
def test_lora_decode_kernels_fit_without_spills():
    res = kernel_resources()
    checked, bad, shrink = {"qz::k_gemv_4bit_lora": 0, "qz::k_gemv_4bit_grouped_lora": 0}, [], 0
    for name, r in res.items():
        base = name.split("<")[0].replace("void ", "").strip()
        a = _targs(name)
        if base == "qz::k_lora_shrink":
            shrink += 1
            if _bad(*r):
                bad.append(r + (name,))
            continue
        # the adapter-carrying decode kernels' templates start <DQ, DT, R, ...> like the plain ones
        if base not in checked or len(a) < 4:
            continue
        dt, rows = int(a[1]), int(a[2])
        assert dt in (0, 1), f"{name}: adapters take 16-bit activations only"
        if rows > 4:
            continue
        checked[base] += 1
        if _bad(*r):
            bad.append(r + (name,))
    assert shrink == 4, f"{shrink} shrink kernels (fp16 / bf16, with and without the norm) found"
    assert checked["qz::k_gemv_4bit_lora"] >= 40 and checked["qz::k_gemv_4bit_grouped_lora"] >= 40, checked
    assert not bad, "adapter kernels over the budget:\n" + "\n".join(map(str, sorted(bad, reverse=True)[:20]))


@pytest.mark.skipif(not _tools_ok(), reason="libquantizations.so or the ROCm LLVM tools are missing")
def test_lora_product_picks_keep_two_waves_per_simd():
    """The adapter forms of the four Llama-3-8B decode launches (the picks of
    test_kernel_resources.test_product_decode_picks_keep_two_waves_per_simd; gate/up takes the
    grouped launch when it carries adapters) are in the library and within the budget."""
    res = kernel_resources()
    picks = [
        "qz::k_gemv_4bit_grouped_lora<true, 0, 2, 1, true, true, true, true>",     # q/k/v + norm
        "qz::k_gemv_4bit_grouped_lora<true, 0, 4, 1, true, true, true, true>",     # gate/up + norm
        "qz::k_gemv_4bit_lora<true, 0, 2, 1, 4, true, true, false, true>",         # o_proj + residual
        "qz::k_gemv_4bit_lora<true, 0, 2, 1, 8, true, true, true, false>",         # down_proj + residual
    ]
    for p in picks:
        hits = [v for k, v in res.items() if p in k]
        assert hits, f"{p} not in the library"
        assert not _bad(*hits[0]), (p, hits[0])
