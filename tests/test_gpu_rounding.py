"""Rounding of fp32 -> fp16/bf16 stores on gfx950 (ties to even)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def test_dequant_store_tie_cases(orc, oracle_vectors):
    """The one halfway case that exposed the scalar fp16 convert.  The `ties` family
    (tests/weight_families.py, test_gpu_weight_range.test_dequantize_families_bit_exact) generalises
    it: >= 32 fp16 and >= 8 bf16 halfway cases per code and parity, and subnormal-range ones."""
    from quantizations_amd import _lib
    from quantizations_amd.core import dequantize_4bit, quantize_4bit

    V = oracle_vectors
    key = "nf4_40x2112"
    W = torch.from_numpy(V[f"{key}_W"].view(np.float16))
    packed, st = quantize_4bit(W.to(DEV), quant_type="nf4")
    w32 = dequantize_4bit(packed, st, out_dtype=torch.float32).t().contiguous().cpu().numpy()
    o = orc.quantize_4bit(W.float().numpy(), 64, "nf4")
    ref32 = orc.dequantize(o)
    diff32 = np.argwhere(w32.view(np.uint32) != ref32.view(np.uint32))
    # a single product, fp32 absmax (no DQ): 0.33791524 * 0.050958175 = 0x3c8d1000 (an fp16 tie)
    am = torch.tensor([0.050958175] * 2, dtype=torch.float32, device=DEV)
    pk = torch.full((64,), 0xBB, dtype=torch.uint8, device=DEV)   # nibble 11 everywhere
    out32 = torch.empty(128, dtype=torch.float32, device=DEV)
    out16 = torch.empty(128, dtype=torch.float16, device=DEV)
    for out, dt in ((out32, _lib.DT_F32), (out16, _lib.DT_F16)):
        _lib.check(_lib.lib.qz_dequantize_4bit(pk.data_ptr(), 128, _lib.NF4, 64, am.data_ptr(), 0, 0, 0, 0, 0,
                                               out.data_ptr(), dt, 0), "dq")
    v32 = out32.cpu().numpy()
    v16 = out16.cpu().numpy().view(np.uint16)
    info = dict(diff32=diff32[:4].tolist(), n32=len(diff32), prod=hex(int(v32[0].view(np.uint32))),
                f16=[hex(int(v)) for v in np.unique(v16)])
    print(info)
    assert len(diff32) == 0, info
    assert v32[0].view(np.uint32) == 0x3C8D1000, info
    assert np.all(v16 == 0x2468), info
