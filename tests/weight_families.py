"""Test-only weight families that reach the edges N(0, 0.02^2) never does: fp16 / bf16 subnormal
weights, underflow to zero, overflow to inf, zero and negative block scales, exact halfway cases
of the fp32 -> fp16 / bf16 stores (normal and subnormal), and inputs that sit on the quantisers'
decision thresholds.  Everything is deterministic from a seed and built with numpy / torch on the
CPU; tests/test_weight_families.py proves on the oracle alone that each family reaches its edge,
tests/test_gpu_weight_range.py hands them to the HIP kernels.

  sweep(dtype)        block b of 64 = randn * 2^e_b, e_b cycling over the dtype's exponent range
                      in shuffled order, clamped to the finite maximum, one block all zero
                      (quantised WITHOUT double quant: the scales span the whole fp32 range)
  tiny(exp)           randn * 2^exp in fp16 (exp = -14, -20; double quant)
  outlier()           N(0, 0.02^2) fp16 with 2 % of the blocks holding one x10..x10^4 outlier and
                      2 % all zero (double quant: code2[q] * absmax2 + offset goes negative)
  ties(qt)            no quantiser: packed codes + an fp32 absmax per block, chosen so that the fp32
                      product code * absmax is an exact halfway case of fp16 / bf16 / fp16-subnormal
  domain16(dtype)     every finite 16-bit value below each pivot, 63 per block + the pivot itself
  nonfinite16(dtype)  blocks holding +inf, -inf and NaN
  thresholds32()      every NF4 / FP4 threshold x pivot, both signs, -2..+2 ulp (fp32 input)
  code8()             every dynamic-map code and tree midpoint at -1, 0, +1 ulp (8-bit quantiser)
"""
from __future__ import annotations

import functools

import numpy as np
import torch

BLOCK = 64
SHAPE = (128, 1024)            # 2048 blocks of 64: the largest tensor any family hands a kernel
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
EXP_RANGE = {"fp16": (-26, 15), "bf16": (-130, 127), "fp32": (-140, 127)}   # sweep's 2^e_b
# the FP4 quantiser's decision constants (reference kernels.cu:113-163)
FP4_THRESHOLDS = np.array([0.00260417, 0.0859375, 0.20833333, 0.29166667, 0.4166667, 0.583333, 0.8333333],
                          np.float32)
TIE_SCAN = 1 << 21             # consecutive fp32 absmax values scanned per code
TIE_KEEP = {"fp16": 32, "bf16": 12, "fp16sub": 4}   # kept per (code, parity of the lower neighbour)


def _to(a64: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    """float64 -> dtype, one rounding, clamped to the dtype's finite maximum first."""
    mx = torch.finfo(dtype).max
    return torch.from_numpy(np.clip(a64, -mx, mx)).to(dtype)


# ---------------------------------------------------------------------------
# quantiser inputs
# ---------------------------------------------------------------------------

# seeds for which rounding to fp16 leaves no block but the planted one all zero (a 2^-26 block
# rounds to zero wholly with probability ~5 %); test_weight_families asserts the count
SWEEP_SEED = {"fp16": 9, "bf16": 0, "fp32": 0}


def sweep(name: str, seed: int | None = None, shape=SHAPE) -> torch.Tensor:
    seed = SWEEP_SEED[name] if seed is None else seed
    rng = np.random.default_rng(seed)
    lo, hi = EXP_RANGE[name]
    exps = rng.permutation(np.arange(lo, hi + 1))
    n = shape[0] * shape[1]
    nb = n // BLOCK
    e = exps[np.arange(nb) % len(exps)].astype(np.float64)
    w = rng.standard_normal((nb, BLOCK)) * np.exp2(e)[:, None]
    w[nb // 3] = 0.0
    return _to(w.reshape(shape), DTYPES[name])


def tiny(exp: int = -14, seed: int = 3, shape=SHAPE) -> torch.Tensor:
    rng = np.random.default_rng(seed - exp)
    return _to(rng.standard_normal(shape) * 2.0 ** exp, torch.float16)


def outlier(seed: int = 4, shape=SHAPE) -> torch.Tensor:
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    nb = n // BLOCK
    w = rng.standard_normal((nb, BLOCK)) * 0.02
    k = max(1, nb * 2 // 100)
    pick = rng.permutation(nb)
    for b in pick[:k]:
        w[b, rng.integers(BLOCK)] *= 10.0 ** rng.uniform(1, 4)
    w[pick[k:2 * k]] = 0.0
    return _to(w.reshape(shape), torch.float16)


def _pivot_blocks(vals: np.ndarray, pivot, np_dtype) -> np.ndarray:
    """vals in blocks of 63 + the pivot (at a position that moves with the block); zero padded."""
    nb = -(-len(vals) // (BLOCK - 1))
    body = np.zeros(nb * (BLOCK - 1), np_dtype)
    body[:len(vals)] = vals
    body = body.reshape(nb, BLOCK - 1)
    out = np.empty((nb, BLOCK), np_dtype)
    for b in range(nb):
        p = (7 * b) % BLOCK
        out[b, :p], out[b, p], out[b, p + 1:] = body[b, :p], pivot, body[b, p:]
    return out


def _all16(name: str) -> np.ndarray:
    """Every finite 16-bit value of the format as float32 (exact), both signs and both zeros."""
    bits = np.arange(1 << 16, dtype=np.uint16)
    if name == "fp16":
        v = bits.view(np.float16).astype(np.float32)
    else:
        v = (bits.astype(np.uint32) << 16).view(np.float32)
    return v[np.isfinite(v)]


DOMAIN16_PIVOTS = {
    "fp16": [1.0, 0.75, 0.0999755859375, 65504.0, 2.0 ** -14, 3 * 2.0 ** -24],
    # the same roles in bf16: 1, 0.75, the bf16 next to 0.1, the finite maximum, the smallest
    # normal and three times the smallest subnormal
    "bf16": [1.0, 0.75, 0.10009765625, float(torch.finfo(torch.bfloat16).max), 2.0 ** -126, 3 * 2.0 ** -133],
}


@functools.lru_cache(maxsize=None)
def domain16(name: str):
    """(tensor [nb, 64] of the 16-bit dtype, pivot of every block as float32 [nb])."""
    allv = _all16(name)
    blocks, piv = [], []
    for A in DOMAIN16_PIVOTS[name]:
        a32 = np.float32(A)
        assert float(a32) == A
        b = _pivot_blocks(allv[np.abs(allv) <= a32], a32, np.float32)
        blocks.append(b)
        piv.append(np.full(len(b), a32, np.float32))
    w = torch.from_numpy(np.concatenate(blocks)).to(DTYPES[name])
    assert torch.equal(w.float(), torch.from_numpy(np.concatenate(blocks)))   # every value is exact in the dtype
    return w, np.concatenate(piv)


def nonfinite16(name: str, seed: int = 5) -> torch.Tensor:
    """[8, 64]: N(0, 0.02^2) blocks with +inf / -inf / NaN / NaN and inf / both infs planted, an
    all-NaN block, an all-inf block and an untouched one."""
    rng = np.random.default_rng(seed)
    w = torch.from_numpy(rng.standard_normal((8, BLOCK)) * 0.02).to(DTYPES[name])
    inf, nan = float("inf"), float("nan")
    w[0, 5] = inf
    w[1, 10] = -inf
    w[2, 63] = nan
    w[3, 0], w[3, 33] = nan, inf
    w[4, 1], w[4, 2] = inf, -inf
    w[5, :] = nan
    w[6, :] = inf
    w[6, 1::2] = -inf
    return w


def thresholds32(nf4_thresholds: np.ndarray):
    """(fp32 tensor [nb, 64], pivots [nb]): every threshold t of both quantisers as fl(t * A), both
    signs, at -2..+2 ulp, in blocks whose absmax is the pivot A."""
    ts = np.concatenate([np.asarray(nf4_thresholds, np.float32), FP4_THRESHOLDS])
    blocks, piv = [], []
    for A in (np.float32(1.0), np.float32(0.75)):
        base = np.abs(ts * A)
        vals = []
        for k in range(-2, 3):
            v = base.copy()
            for _ in range(abs(k)):
                v = np.nextafter(v, np.float32(np.inf if k > 0 else 0.0), dtype=np.float32)
            vals += [v, -v]
        vals = np.concatenate(vals)
        assert np.all(np.abs(vals) < A)
        b = _pivot_blocks(vals, A, np.float32)
        blocks.append(b)
        piv.append(np.full(len(b), A, np.float32))
    return torch.from_numpy(np.concatenate(blocks)), np.concatenate(piv)


def code8(code: np.ndarray) -> torch.Tensor:
    """fp32 [nb, 256], every block's absmax exactly 1.0: the 256 codes of the sorted dynamic map and
    the 255 midpoints fl(fl(c_i + c_{i+1}) * 0.5) its search tree compares against, each at -1, 0,
    +1 ulp (values beyond +-1 are left out)."""
    c = np.asarray(code, np.float32)
    mid = ((c[:-1] + c[1:]) * np.float32(0.5)).astype(np.float32)
    base = np.concatenate([c, mid])
    vals = np.concatenate([np.nextafter(base, np.float32(-np.inf), dtype=np.float32), base,
                           np.nextafter(base, np.float32(np.inf), dtype=np.float32)])
    vals = vals[np.abs(vals) <= 1.0]
    nb = -(-len(vals) // 255)
    body = np.zeros(nb * 255, np.float32)
    body[:len(vals)] = vals
    out = np.concatenate([np.ones((nb, 1), np.float32), body.reshape(nb, 255)], axis=1)
    return torch.from_numpy(out)


# ---------------------------------------------------------------------------
# ties: dequantiser inputs, no quantiser involved
# ---------------------------------------------------------------------------

def dequant_codes(orc, qt: str) -> np.ndarray:
    """The 16 fp32 values a code dequantises to at absmax 1 (FP4: the reference's tree, whose
    constants differ from the GEMV codebook's x / 12 in the last digit)."""
    one = np.ones(1, np.float32)
    return np.array([orc.dequantize_4bit(np.array([i << 4], np.uint8), one, 1, BLOCK, qt)[0] for i in range(16)],
                    np.float32)


def _scan(start: float) -> np.ndarray:
    return (np.arange(TIE_SCAN, dtype=np.uint32) + np.float32(start).view(np.uint32)).view(np.float32)


def tie_kind(prod32: np.ndarray, fmt: str):
    """(is an exact halfway case of `fmt`, lower neighbour is odd) for fp32 products."""
    prod32 = np.asarray(prod32, np.float32)
    bits = prod32.view(np.uint32)
    mag = np.abs(prod32)
    if fmt == "fp16":
        return ((bits & 0x1FFF) == 0x1000) & (mag >= 2.0 ** -14) & (mag < 65504.0), ((bits >> 13) & 1) == 1
    if fmt == "bf16":
        return ((bits & 0xFFFF) == 0x8000) & (mag >= 2.0 ** -126) & np.isfinite(prod32), ((bits >> 16) & 1) == 1
    q = mag.astype(np.float64) * 2.0 ** 25          # fp16 subnormal spacing 2^-24: halfway = odd multiple of 2^-25
    half = (mag < 2.0 ** -14) & (q == np.floor(q)) & (np.floor(q) % 2 == 1)
    return half, (np.floor(q) // 2) % 2 == 1


@functools.lru_cache(maxsize=None)
def _ties_cached(qt: str, codes_key: bytes):
    codes = np.frombuffer(codes_key, np.float32)
    am_norm, am_sub = _scan(0.05), _scan(2.0 ** -16)
    absmax, meta = [], []
    for c in range(16):
        if codes[c] == 0:
            continue
        for fmt, am in (("fp16", am_norm), ("bf16", am_norm), ("fp16sub", am_sub)):
            half, odd = tie_kind(codes[c] * am, fmt)
            for parity in (False, True):
                kept = am[half & (odd == parity)][:TIE_KEEP[fmt]]
                absmax.append(kept)
                meta += [(c, fmt, parity)] * len(kept)
    absmax = np.concatenate(absmax)
    order = np.random.default_rng(6).permutation(len(absmax))   # any slice of blocks holds every kind
    return absmax[order], [meta[i] for i in order]


def ties(orc, qt: str):
    """(packed u8 [nb * 32], absmax f32 [nb], meta [(code, format, lower neighbour odd)] per block).
    Every block's 64 nibbles cycle through the 16 codes (rotated by the block index)."""
    absmax, meta = _ties_cached(qt, dequant_codes(orc, qt).tobytes())
    nb = len(absmax)
    nib = ((np.arange(BLOCK)[None, :] + np.arange(nb)[:, None]) % 16).astype(np.uint8)
    packed = (nib[:, 0::2] << 4) | nib[:, 1::2]
    return packed.reshape(-1), absmax, meta


def ties_weight(orc, qt: str, M: int, K: int, first: int = 0):
    """M x K weight made of the ties blocks first, first + 1, ... (wrapping round)."""
    packed, absmax, _ = ties(orc, qt)
    nb = M * K // BLOCK
    idx = (first + np.arange(nb)) % len(absmax)
    return packed.reshape(-1, BLOCK // 2)[idx].reshape(-1), absmax[idx]
