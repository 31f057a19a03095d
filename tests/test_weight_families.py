"""CPU: every family of tests/weight_families.py reaches the edge it was built for -- shown on the
oracle's outputs alone, so the GPU tests that consume the families (tests/test_gpu_weight_range.py)
cannot pass by never meeting the case.  These are conditions on the constructions, not
measurements of any kernel."""
import numpy as np
import pytest
import torch

import weight_families as wf


def _f16_subnormal(w32):
    h = torch.from_numpy(w32).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    return ((h & 0x7C00) == 0) & ((h & 0x03FF) != 0)


def _bf16_subnormal(w32):
    h = torch.from_numpy(w32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    return ((h & 0x7F80) == 0) & ((h & 0x007F) != 0)


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
def test_sweep_reaches_subnormals_underflow_overflow_and_a_zero_scale(orc, qt):
    st = orc.quantize_4bit(wf.sweep("fp16").float().numpy(), 64, qt, double_quant=False)
    w = orc.dequantize(st).ravel()
    assert int((st.absmax_raw == 0).sum()) == 1
    assert int(_f16_subnormal(w).sum()) >= 10_000
    # products that underflow: FP4's smallest code (1/192) under any scale below 2^-17.  NF4's smallest
    # (0.08) would need a scale below 6 * 2^-24, where a block holds only 0, +-1, ... +-5 times the
    # smallest fp16 subnormal and no input falls in that code's interval
    if qt == "fp4":
        assert int(((w != 0) & (torch.from_numpy(w).to(torch.float16).float().numpy() == 0)).sum()) >= 1_000
    assert np.isfinite(w).all() and torch.isfinite(torch.from_numpy(w).to(torch.float16)).all()
    for name in ("bf16", "fp32"):
        st = orc.quantize_4bit(wf.sweep(name).float().numpy(), 64, qt, double_quant=False)
        w = orc.dequantize(st).ravel()
        assert int((st.absmax_raw == 0).sum()) == 1, name
        assert int(torch.isinf(torch.from_numpy(w).to(torch.float16)).sum()) >= 1_000, name
        assert int(_bf16_subnormal(w).sum()) >= 1_000, name


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
@pytest.mark.parametrize("exp", [-14, -20])
def test_tiny_is_mostly_fp16_subnormal(orc, qt, exp):
    st = orc.quantize_4bit(wf.tiny(exp).float().numpy(), 64, qt, double_quant=True)
    w = orc.dequantize(st).ravel()
    assert np.isfinite(w).all()
    assert int(_f16_subnormal(w).sum()) >= 50_000


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
def test_outlier_decodes_negative_block_scales(orc, qt):
    st = orc.quantize_4bit(wf.outlier().float().numpy(), 64, qt, double_quant=True)
    am = st.absmax()
    assert int((am < 0).sum()) >= 10
    assert np.isfinite(orc.dequantize(st)).all()
    # a negative scale under a zero code (the all-zero blocks quantise to code 0, FP4's zero): the sign
    # of zero is part of the bit-exact claim
    if qt == "fp4":
        w = orc.dequantize(st).reshape(-1, 64)[am < 0]
        assert np.signbit(w[w == 0]).any()


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
def test_ties_are_exact_halfway_cases_of_both_parities(orc, qt):
    packed, absmax, meta = wf.ties(orc, qt)
    assert len(absmax) <= 2048 and len(meta) == len(absmax)
    codes = wf.dequant_codes(orc, qt)
    w = orc.dequantize_4bit(packed, absmax, 64 * len(absmax), 64, qt).reshape(-1, 64)
    count = {}
    for b, (c, fmt, odd) in enumerate(meta):
        col = (c - b) % 16                      # block b's nibbles are (j + b) % 16
        prod = w[b, col]
        assert prod == np.float32(codes[c]) * absmax[b]      # the oracle's product is numpy's
        half, isodd = wf.tie_kind(np.array([prod]), fmt)
        assert half[0] and bool(isodd[0]) == odd, (b, c, fmt, odd)
        lo, hi = {"fp16": (2.0 ** -14, 65504.0), "bf16": (2.0 ** -126, 3e38), "fp16sub": (0.0, 2.0 ** -14)}[fmt]
        assert lo <= abs(float(prod)) < hi
        count[c, fmt, odd] = count.get((c, fmt, odd), 0) + 1
    # torch's rounding (the reference the GPU tests use) takes every one of them to the even neighbour
    h = torch.from_numpy(w).to(torch.float16).view(torch.int16).numpy()
    bf = torch.from_numpy(w).to(torch.bfloat16).view(torch.int16).numpy()
    for b, (c, fmt, odd) in enumerate(meta):
        r = (bf if fmt == "bf16" else h)[b, (c - b) % 16]
        assert r & 1 == 0, (b, c, fmt)
    for c in range(16):
        if codes[c] == 0:
            continue
        for odd in (False, True):
            assert count.get((c, "fp16", odd), 0) >= 32, (c, odd)
            assert count.get((c, "bf16", odd), 0) >= 8, (c, odd)
        assert count.get((c, "fp16sub", False), 0) + count.get((c, "fp16sub", True), 0) >= 1, c


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_domain16_block_absmax_is_the_pivot_and_every_code_occurs(orc, name):
    w, piv = wf.domain16(name)
    if name == "fp16":
        assert w.numel() >= 152_320
    for qt in ("fp4", "nf4"):
        packed, absmax = orc.quantize_4bit_raw(w.float().numpy(), 64, qt)
        assert np.array_equal(absmax.view(np.uint32), piv.view(np.uint32))
        assert set(np.unique(np.concatenate([packed >> 4, packed & 15])).tolist()) == set(range(16))
    # exhaustive: every finite value of the format below the largest pivot is in the tensor
    allv = wf._all16(name)
    assert set(np.unique(allv.view(np.uint32)).tolist()) <= set(np.unique(w.float().numpy().view(np.uint32)).tolist())


def test_nonfinite16_blocks_hold_what_they_say():
    for name in ("fp16", "bf16"):
        w = wf.nonfinite16(name).float()
        assert torch.isposinf(w[0]).sum() == 1 and torch.isneginf(w[1]).sum() == 1 and torch.isnan(w[2]).sum() == 1
        assert torch.isnan(w[5]).all() and torch.isinf(w[6]).all() and torch.isfinite(w[7]).all()


def test_thresholds32_straddles_every_decision(orc):
    w, piv = wf.thresholds32(orc.nf4_thresholds())
    for qt, nthr in (("nf4", 15), ("fp4", 7)):
        packed, absmax = orc.quantize_4bit_raw(w.numpy(), 64, qt)
        assert np.array_equal(absmax.view(np.uint32), piv.view(np.uint32))
        assert set(np.unique(np.concatenate([packed >> 4, packed & 15])).tolist()) == set(range(16))
    # at pivot 1 the scaled input IS the stored value: both sides of every threshold occur
    x = w.numpy()[piv == 1.0].ravel()
    for t in np.concatenate([orc.nf4_thresholds(), wf.FP4_THRESHOLDS, -wf.FP4_THRESHOLDS]):
        assert (x == t).any() and (x == np.nextafter(t, np.float32(1))).any() \
            and (x == np.nextafter(t, np.float32(-1))).any(), t


def test_code8_hits_every_code_and_midpoint(orc):
    code = orc.create_dynamic_map()
    a = wf.code8(code)
    q, am = orc.quantize_blockwise_8bit(code, a.numpy(), 256)
    assert np.array_equal(am, np.ones(len(am), np.float32))
    assert len(np.unique(q)) == len(np.unique(code))
    x = a.numpy().ravel()
    mid = ((code[:-1] + code[1:]) * np.float32(0.5)).astype(np.float32)
    assert np.isin(code, x).all() and np.isin(mid, x).all()
    assert np.isin(np.nextafter(mid[mid < 1], np.float32(2)), x).all()
