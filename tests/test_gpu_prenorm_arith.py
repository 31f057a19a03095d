"""GPU: the RMSNorm arithmetic of qz_rmsnorm and of the fused pre-norm prologues, bit for bit.

The fused prologue (gemv_core.h norm_chunk_ss / norm_chunk_apply) forms x' = w * fp16(x * rs) with
one fused multiply-add per square, one packed conversion per pair and a packed fp16 weight product.
Each of those is the same value as torch's op-by-op rounding only because a product of two fp16
values is exact in fp32; a fusion that goes one step further (x * rs rounded straight to fp16) is
wrong on rounding ties.  So:

 1. qz_rmsnorm (k_rmsnorm_held, the form every aligned row of K <= 16384 takes) equals a torch
    restatement of LlamaRMSNorm -- x.float(), the mean of squares, rsqrt(var + eps), the
    product rounded to fp32 and then to the storage dtype, the weight product -- with `torch.equal`.
    torch leaves the order of the fp32 sum open; the restatement adds the squares in the order the
    kernels document (thread t of 256: 16-byte chunks t, t + 256, ... in element order; the xor
    butterfly of each wave; the four wave sums as (s0 + s1) + (s2 + s3)), every add a torch fp32 op.
    Inputs: randn x {1e-4, 1, 300}; a row whose weight products are fp16 subnormals; a row of +-0
    with one 65504; a row seeded with elements whose x * rs lands on an fp16 rounding tie after the
    fp32 rounding (searched for on the CPU; the test asserts that the reference itself tells double
    from single rounding on them).
 2. The fused grouped launch equals qz_rmsnorm + the plain grouped launch on every segment, on the
    same hostile inputs.
 3. The pair launch with the norm equals qz_rmsnorm + grouped + silu_mul where the grouped launch
    keeps whole rows per wave (the pair's summation order), and qz_rmsnorm + the plain pair launch
    at the small row counts where the grouped geometry splits K over waves; one workgroup per block
    and persistent workgroups through the QZ_PAIR_PS knob.
 4. The normed grouped launch on 8-wave workgroups (QZ_GROUPED_NORM_NW8, exact codes, at least 256
    workgroups) equals the 4-wave one.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
EPS = 1e-5
KS = (2048, 4096)


# ---- the reference: LlamaRMSNorm in torch ops, the fp32 sum in the kernels' documented order ----

def _ordered_sum_sq(xf):
    """sum(xf ** 2) for a 1-D fp32 tensor (len % 8 == 0) in k_rmsnorm's order; every add is a torch fp32 add."""
    sq = xf * xf
    n = sq.numel() // 8
    rounds = (n + 255) // 256
    pad = torch.zeros(rounds * 256 * 8, dtype=torch.float32, device=xf.device)
    pad[:sq.numel()] = sq                      # a thread without a chunk in the last round adds +0: no change
    pad = pad.view(rounds, 256, 8)
    ss = torch.zeros(256, dtype=torch.float32, device=xf.device)
    for r in range(rounds):
        for j in range(8):
            ss = ss + pad[r, :, j]
    lane = torch.arange(256, device=xf.device)
    for o in (32, 16, 8, 4, 2, 1):
        ss = ss + ss[lane ^ o]
    return (ss[0] + ss[64]) + (ss[128] + ss[192])


def _rs(x, eps=EPS):
    K = x.numel()
    tot = _ordered_sum_sq(x.float())
    inv = torch.tensor(1.0 / K, dtype=torch.float32, device=x.device)   # fp32(1 / K), as MeanOps
    return torch.rsqrt(tot * inv + eps)


def _llama_rmsnorm(x, w, eps=EPS):
    h = x.float() * _rs(x, eps)          # rounded to fp32 ...
    return w * h.to(x.dtype)             # ... then to the storage dtype; the weight product in it


# ---- inputs ----

def _f16_values():
    """every positive fp16 value below 2^-7, as fp16 numpy"""
    bits = np.arange(1, 0x2000, dtype=np.uint16)       # 0x2000 = 2^-7
    return bits.view(np.float16)


def _tie_candidates(rs32):
    """fp16 values v in (0, 2^-7) whose fp32 product v * rs lies within one fp32 ulp of the midpoint of two
    adjacent fp16 values, and among them those on which rounding the exact product to fp16 once differs
    from rounding it to fp32 first.  CPU only (numpy float64 holds the 35-bit product exactly)."""
    v = _f16_values()
    p64 = v.astype(np.float64) * np.float64(rs32)
    p32 = p64.astype(np.float32)                                   # the one rounding of __fmul_rn
    lo = p32.astype(np.float16)
    up = np.nextafter(lo, np.float16(np.inf))
    dn = np.nextafter(lo, np.float16(-np.inf))
    bits = p32.view(np.uint32).astype(np.int64)
    near = np.zeros(v.shape, dtype=bool)
    for nb in (up, dn):
        mid = ((lo.astype(np.float64) + nb.astype(np.float64)) * 0.5).astype(np.float32)   # exact in fp32
        near |= np.abs(bits - mid.view(np.uint32).astype(np.int64)) <= 1
    differs = p64.astype(np.float16) != lo
    return v[near], v[differs]


def _base_row(K, seed, scale):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(K, generator=g) * scale).half()


@functools.lru_cache(maxsize=None)
def _tie_row(K):
    """A randn x 32 row with tie candidates planted at elements 1..7 of 16-byte chunks.  Element 0 of every
    chunk is at least 32, so the thread's running sum is at least 1024 (half an ulp: 2^-14) when a planted
    square, below 2^-14, is added: every partial sum -- and so rs -- stays what the search assumed."""
    for seed in range(400):
        x = _base_row(K, 1000 + seed, 32.0)
        x[0::8] = torch.where(x[0::8].abs() < 32, torch.full_like(x[0::8], 40.0), x[0::8])
        slots = [c * 8 + j for c in range(K // 8) for j in range(1, 8)][:256]
        x[slots] = 0.0                                                 # reserved for the candidates
        rs = float(_rs(x.to(DEV)).cpu())
        near, differs = _tie_candidates(np.float32(rs))
        if len(differs) < 2:
            continue
        vals = np.concatenate([differs, -differs, near, -near])[:len(slots)]
        x[slots[:len(vals)]] = torch.from_numpy(vals.copy())
        assert float(_rs(x.to(DEV)).cpu()) == rs, "planting the candidates moved rs"
        return x, rs, len(differs)
    raise AssertionError("no row with two double-rounding elements in 400 seeds")


def _rows(K):
    """name -> (x, w) fp16 CPU tensors"""
    g = torch.Generator().manual_seed(K)
    w1 = (1.0 + 0.1 * torch.randn(K, generator=g)).half()
    rows = {f"randn*{s:g}": ((torch.randn(K, generator=g) * s).half(), w1) for s in (1e-4, 1.0, 300.0)}
    # |x * rs| ~ 2^-10 against w ~ 2^-12: products ~ 2^-22, fp16 subnormals (a unit of 2^-24)
    big = torch.zeros(K).half()
    big[:K // 64] = 1024.0 * (K ** 0.5) / ((K // 64) ** 0.5)        # carries the mean square: rs ~ 2^-10
    xs = torch.where(big != 0, big, (1.0 + 0.5 * torch.rand(K, generator=g)).half())
    ws = ((2.0 ** -12) * (1.0 + torch.rand(K, generator=g)) * torch.where(torch.rand(K, generator=g) < 0.5, -1.0, 1.0)).half()
    rows["subnormal products"] = (xs, ws)
    xz = torch.zeros(K).half()
    xz[1::2] = -0.0
    xz[K // 3] = 65504.0
    rows["zeros and 65504"] = (xz, w1)
    rows["ties"] = (_tie_row(K)[0], w1)
    return rows


@functools.lru_cache(maxsize=None)
def _cases(K, dtype):
    """name -> (x, w, reference) on the device; computed once"""
    out = {}
    for name, (x, w) in _rows(K).items():
        if dtype != torch.float16:
            if name == "ties":
                continue                                    # searched for fp16 roundings
            x, w = x.float().to(dtype), w.float().to(dtype)
        x, w = x.to(DEV), w.to(DEV)
        out[name] = (x, w, _llama_rmsnorm(x, w))
    return out


# ---- 1. qz_rmsnorm against the restatement ----

def test_tie_row_distinguishes_double_from_single_rounding():
    """The reference rounds x * rs to fp32 and then to fp16; on the planted elements a single rounding of
    the exact product gives another fp16 value, so a kernel that fuses the two cannot pass test 1."""
    for K in KS:
        x, rs, n = _tie_row(K)
        assert n >= 2
        xd = x.to(DEV)
        rs_t = _rs(xd)
        assert float(rs_t.cpu()) == rs
        twice = (xd.float() * rs_t).half().cpu().numpy()                                   # the reference's way
        once = (x.numpy().astype(np.float64) * np.float64(np.float32(rs))).astype(np.float16)
        diff = int((twice != once).sum())
        print(f"K={K}: rs={rs!r}, {diff} elements where single rounding differs")
        assert diff >= 1


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("K", KS)
def test_rmsnorm_equals_llama_rmsnorm_restatement(K, dtype):
    from quantizations_amd.layer_ops import rms_norm

    for name, (x, w, ref) in _cases(K, dtype).items():
        got = rms_norm(x, w, EPS)                           # K <= 16384, aligned: k_rmsnorm_held
        bad = int((got.view(torch.int16) != ref.view(torch.int16)).sum())
        print(f"K={K} {dtype} {name}: {bad} differing elements")
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), name


# ---- 2. / 3. the fused prologues against qz_rmsnorm + the plain launches ----

@functools.lru_cache(maxsize=None)
def _items(Ms, K, dtype, seed):
    from quantizations_amd.core import quantize_4bit

    g = torch.Generator(device="cuda").manual_seed(seed)
    items = []
    for M in Ms:
        W = (torch.randn(M, K, device=DEV, generator=g) * 0.02).to(dtype)
        packed, st = quantize_4bit(W, quant_type="nf4", compress_statistics=True)
        items.append((packed, st, None))
    return tuple(items)


def _inputs(K, dtype):
    """the hostile rows of test 1 at K = 2048 / 4096; at K = 6144 (the loop form) rows stitched from them"""
    if K in KS:
        return {n: (x, w) for n, (x, w, _) in _cases(K, dtype).items()}
    a, b = _cases(2048, dtype), _cases(4096, dtype)
    return {n: (torch.cat([b[n][0], a[n][0]]), torch.cat([b[n][1], a[n][1]])) for n in a}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("Ms,K", [(Ms, K) for K in (2048, 4096, 6144) for Ms in ((16, 8, 8), (40, 16, 16))] +
                         [((4096, 1024, 1024), 4096)])   # and the Llama-3-8B q/k/v geometry (R = 2, two-step form)
def test_fused_grouped_equals_norm_then_grouped(Ms, K, dtype):
    from quantizations_amd.core import LAST_FORM, gemv_4bit_grouped
    from quantizations_amd.layer_ops import rms_norm

    exact = True if dtype == torch.float16 else None
    items = _items(Ms, K, dtype, K + Ms[0])
    for name, (x, w) in _inputs(K, dtype).items():
        x = x.view(1, 1, K)
        ref = gemv_4bit_grouped(rms_norm(x, w, EPS), items, exact_codes=exact)
        got = gemv_4bit_grouped(x, items, exact_codes=exact, norm=(w, EPS))
        assert LAST_FORM["grouped"] == "grouped (norm fused)"
        for i, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{name}: segment {i}"


@pytest.fixture
def pair_ps():
    from quantizations_amd import _lib

    try:
        yield lambda v: _lib.set_gemv_knob("QZ_PAIR_PS", v)
    finally:
        _lib.set_gemv_knob("QZ_PAIR_PS", -1)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,K", [(16, 2048), (40, 2048), (16, 4096), (40, 4096), (16, 6144), (40, 6144),
                                 (1030, 4096), (1030, 6144)])
def test_fused_pair_equals_norm_then_plain_launches(pair_ps, M, K, dtype):
    """M = 16 / 40 at K = 2048 and M = 1030: the grouped launch keeps whole rows per wave, so the reference
    is qz_rmsnorm + grouped + silu_mul.  M = 16 / 40 at K = 4096 / 6144: the grouped geometry splits K over
    waves (another fp32 summation order than the pair's whole rows), so the reference is qz_rmsnorm + the
    plain pair launch.  QZ_PAIR_PS 0: one workgroup per block; 16 / 256: a persistent grid of that size."""
    from quantizations_amd.core import LAST_FORM, gemv_4bit_grouped, gemv_4bit_pair_silu
    from quantizations_amd.layer_ops import rms_norm, silu_mul

    exact = True if dtype == torch.float16 else None
    items = _items((M, M), K, dtype, K + M)
    whole_rows = K == 2048 or M >= 1024
    for name, (x, w) in _inputs(K, dtype).items():
        x = x.view(1, 1, K)
        xn = rms_norm(x, w, EPS)
        pair_ps(0)
        if whole_rows:
            ref = silu_mul(*gemv_4bit_grouped(xn, items, exact_codes=exact))
        else:
            ref = gemv_4bit_pair_silu(xn, items, exact_codes=exact)
        assert ref is not None
        for ps in (0, 16 if M < 1024 else 256):
            pair_ps(ps)
            h = gemv_4bit_pair_silu(x, items, exact_codes=exact, norm=(w, EPS))
            assert h is not None and LAST_FORM["pair"] == "pair (norm fused)"
            assert torch.equal(h.view(torch.int16), ref.view(torch.int16)), f"{name}: QZ_PAIR_PS={ps}"


# ---- 4. the 8-wave normed grouped launch against the 4-wave one ----

@pytest.mark.parametrize("K", [2048, 4096, 6144])
@pytest.mark.parametrize("tail", [16, 40])
def test_grouped_norm_8_waves_equals_4_waves(tail, K):
    """The 8-wave form is taken from 256 workgroups (of 16 rows) on: a first segment of 4096 rows, then
    segments of `tail` and 8 rows -- 40 leaves a ragged last block at 4 waves (8 rows) and at 8 (16 rows)."""
    from quantizations_amd import _lib
    from quantizations_amd.core import LAST_FORM, gemv_4bit_grouped

    items = _items((4096, tail, 8), K, torch.float16, K + tail)
    try:
        for name, (x, w) in _inputs(K, torch.float16).items():
            x = x.view(1, 1, K)
            _lib.set_gemv_knob("QZ_GROUPED_NORM_NW8", 0)
            ref = gemv_4bit_grouped(x, items, exact_codes=True, norm=(w, EPS))
            _lib.set_gemv_knob("QZ_GROUPED_NORM_NW8", 1)
            assert _lib.gemv_knobs()["QZ_GROUPED_NORM_NW8"] == 1
            got = gemv_4bit_grouped(x, items, exact_codes=True, norm=(w, EPS))
            assert LAST_FORM["grouped"] == "grouped (norm fused)"
            for i, (a, b) in enumerate(zip(got, ref)):
                assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{name}: segment {i}"
    finally:
        _lib.set_gemv_knob("QZ_GROUPED_NORM_NW8", 0)
