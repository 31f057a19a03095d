"""GPU: the 4-bit kernels on weights beyond N(0, 0.02^2) -- the families of tests/weight_families.py
(tests/test_weight_families.py shows on the oracle alone that each reaches its edge).

* Quantise: packed codes, raw absmax and the double-quant statistics bit-exact against the oracle on
  the exhaustive 16-bit domain, on the fp32 decision thresholds, on non-finite blocks, on scales over
  the whole exponent range, and the 8-bit quantiser on every code and tree midpoint.
* Dequantise: fp16 / bf16 / fp32 stores bit-exact (compared as integers: the sign of zero under a
  negative scale, infs, underflows and NaN payloads count) against the oracle's fp32 product rounded
  once by torch -- including the exact halfway cases of the `ties` family, which generalise the
  single example of tests/test_gpu_rounding.py.
* Fused decode: one-hot activations / gradients read EVERY weight of each family back through each
  MFMA kernel; it must be dequantize_4bit's value.
* GEMV and product routes on the project's existing bars (test_gpu_parity.assert_close).

The dequantise and fused-decode groups take their QuantState from the ORACLE's quantisation (built
by hand), so a quantiser mismatch cannot hide or cause a decode mismatch.
"""
import numpy as np
import pytest
import torch

import weight_families as wf
from test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DT_IDS = {F16: "fp16", BF16: "bf16", F32: "fp32"}

# family -> (builder(shape) of the weight tensor, double quant)
FAMILIES = {
    "sweep16": (lambda shape: wf.sweep("fp16", shape=shape), False),
    "sweepbf": (lambda shape: wf.sweep("bf16", shape=shape), False),
    "sweep32": (lambda shape: wf.sweep("fp32", shape=shape), False),
    "tiny14": (lambda shape: wf.tiny(-14, shape=shape), True),
    "tiny20": (lambda shape: wf.tiny(-20, shape=shape), True),
    "outlier": (lambda shape: wf.outlier(shape=shape), True),
}
FINITE16 = ["tiny14", "tiny20", "outlier", "ties", "sweep16"]   # every dequantised weight finite in fp16 and bf16

_cache = {}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _oracle_state(family, qt, shape, bs=64):
    """The oracle's quantisation of a family (cached); `ties` has no quantiser: codes + fp32 absmax."""
    import oracle

    key = (family, qt, shape, bs)
    if key not in _cache:
        if family == "ties":
            packed, absmax = wf.ties_weight(oracle, qt, *shape)
            _cache[key] = oracle.OracleState(packed, absmax, shape, bs, qt, oracle.codebook(qt), False)
        else:
            build, dq = FAMILIES[family]
            _cache[key] = oracle.quantize_4bit(build(shape).float().numpy(), bs, qt, double_quant=dq)
    return _cache[key]


def _gpu_state(o):
    """(packed, QuantState) on the GPU, built by hand from an OracleState."""
    from quantizations_amd.core import QuantState, get_4bit_type

    packed = torch.from_numpy(o.packed).reshape(-1, 1).to(DEV)
    code = get_4bit_type(o.quant_type, device=DEV)
    if not o.double_quant:
        return packed, QuantState(absmax=torch.from_numpy(o.absmax_raw).to(DEV), shape=torch.Size(o.shape), dtype=F16,
                                  blocksize=o.blocksize, code=code, quant_type=o.quant_type)
    st2 = QuantState(absmax=torch.from_numpy(o.absmax2).to(DEV), code=torch.from_numpy(o.code2).to(DEV),
                     blocksize=o.blocksize2, dtype=F32)
    return packed, QuantState(absmax=torch.from_numpy(o.qabsmax).to(DEV), shape=torch.Size(o.shape), dtype=F16,
                              blocksize=o.blocksize, code=code, quant_type=o.quant_type,
                              offset=torch.tensor(float(o.offset), dtype=F32, device=DEV), state2=st2)


def _weight(family, qt, shape, dt):
    """(packed, state, Wd [M, K] in dt = the ORACLE's dequantised weight rounded once by torch)."""
    import oracle

    o = _oracle_state(family, qt, shape)
    key = ("wd", family, qt, shape, dt)
    if key not in _cache:
        _cache[key] = torch.from_numpy(oracle.dequantize(o)).to(dt)
    packed, st = _gpu_state(o)
    return packed, st, _cache[key].to(DEV)


# ---------------------------------------------------------------------------
# quantise: bit-exact against the oracle
# ---------------------------------------------------------------------------


def _assert_quantised_like_oracle(orc, W, bs, qt, dq, what):
    from quantizations_amd.core import quantize_4bit

    o = orc.quantize_4bit(W.float().numpy(), bs, qt, double_quant=dq)
    packed, st = quantize_4bit(W.to(DEV), blocksize=bs, quant_type=qt, compress_statistics=False)
    got = packed.cpu().numpy().ravel()
    bad = np.flatnonzero(got != o.packed)
    assert bad.size == 0, (what, "codes", bad.size, [(int(i), hex(got[i]), hex(o.packed[i])) for i in bad[:4]],
                           W.reshape(-1)[torch.from_numpy(2 * bad[:4])].tolist())
    am = st.absmax.cpu().numpy()
    bad = np.flatnonzero(am.view(np.uint32) != o.absmax_raw.view(np.uint32))
    assert bad.size == 0, (what, "absmax", bad.size, am[bad[:4]].tolist(), o.absmax_raw[bad[:4]].tolist())
    if dq:
        packed, st = quantize_4bit(W.to(DEV), blocksize=bs, quant_type=qt, compress_statistics=True)
        assert np.array_equal(packed.cpu().numpy().ravel(), o.packed), (what, "codes (double quant)")
        off = st.offset.cpu().numpy().reshape(1)
        assert off.view(np.uint32)[0] == np.float32(o.offset).reshape(1).view(np.uint32)[0], (what, off, o.offset)
        q = st.absmax.cpu().numpy()
        bad = np.flatnonzero(q != o.qabsmax)
        assert bad.size == 0, (what, "qabsmax", bad.size, q[bad[:4]].tolist(), o.qabsmax[bad[:4]].tolist())
        a2 = st.state2.absmax.cpu().numpy()
        assert np.array_equal(a2.view(np.uint32), o.absmax2.view(np.uint32)), (what, "absmax2", a2, o.absmax2)


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_quantize_exhaustive_16bit_domain(orc, name, qt):
    """Every finite 16-bit input below each pivot, the block absmax being the pivot: every decision of
    both trees at every input the format can present, with and without double quant."""
    W, _ = wf.domain16(name)
    _assert_quantised_like_oracle(orc, W, 64, qt, True, f"domain16 {name} {qt}")


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
def test_quantize_fp32_thresholds(orc, qt):
    """fp32 inputs at -2..+2 ulp of every NF4 / FP4 threshold times the pivot: a constant wrong in
    its last digit, or >= written for >, changes a code."""
    W, _ = wf.thresholds32(orc.nf4_thresholds())
    _assert_quantised_like_oracle(orc, W, 64, qt, True, f"thresholds32 {qt}")


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
@pytest.mark.parametrize("bs", [64, 256])
@pytest.mark.parametrize("dt", [F16, BF16, F32], ids=DT_IDS.get)
@pytest.mark.parametrize("family", ["sweep", "tiny14", "tiny20", "outlier"])
def test_quantize_families(orc, family, dt, bs, qt):
    """Scales over the dtype's whole exponent range (an all-zero block, 1 / absmax overflowing to inf
    or denormal), tiny tensors and outlier / zero blocks under double quant."""
    if family == "sweep":
        W, dq = wf.sweep(DT_IDS[dt]), False
    else:
        W, dq = FAMILIES[family][0](wf.SHAPE).to(dt), True
    _assert_quantised_like_oracle(orc, W, bs, qt, dq, f"{family} {dt} bs={bs} {qt}")


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_quantize_nonfinite_blocks(orc, name, qt):
    """Blocks holding +inf, -inf, NaN, both, only NaN, only inf.  The oracle is the bar; it restates
    the reference kernel (kernels.cu:406-431, 340-478): the block maximum is an fmaxf chain seeded
    with -FLT_MAX, which ignores NaN (an all-NaN block keeps -FLT_MAX), an inf makes the scale
    1 / inf = 0, finite inputs then quantise as 0 and inf * 0 = NaN falls through every strict '>'
    to code 0 (sign bit from `x < 0`, false for NaN).  Without double quant: the statistics of an
    inf absmax are NaN by construction and say nothing about a kernel."""
    W = wf.nonfinite16(name)
    _assert_quantised_like_oracle(orc, W, 64, qt, False, f"nonfinite {name} {qt}")


def test_quantize_8bit_every_code_and_midpoint(orc):
    """The 8-bit double-quant quantiser (blocksize 256, block absmax exactly 1) on all 256 codes of the
    dynamic map and the 255 midpoints its search compares against, at -1, 0, +1 ulp."""
    from quantizations_amd.core import quantize_blockwise

    code = orc.create_dynamic_map()
    A = wf.code8(code)
    q, st = quantize_blockwise(A.to(DEV), blocksize=256)
    assert np.array_equal(st.code.cpu().numpy().view(np.uint32), code.view(np.uint32))
    oq, oam = orc.quantize_blockwise_8bit(code, A.numpy(), 256)
    got = q.cpu().numpy().ravel()
    bad = np.flatnonzero(got != oq)
    assert bad.size == 0, (bad.size, got[bad[:6]].tolist(), oq[bad[:6]].tolist(), A.reshape(-1)[bad[:6]].tolist())
    assert np.array_equal(st.absmax.cpu().numpy().view(np.uint32), oam.view(np.uint32))


# ---------------------------------------------------------------------------
# dequantise: bit-exact against the oracle
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
@pytest.mark.parametrize("dt", [F16, BF16, F32], ids=DT_IDS.get)
@pytest.mark.parametrize("family", ["sweep16", "sweepbf", "sweep32", "tiny14", "tiny20", "outlier", "ties"])
def test_dequantize_families_bit_exact(family, dt, qt):
    """Infs, underflows to +-0, subnormals, -0.0 from a zero code under a negative scale, and (ties)
    >= 32 fp16 and >= 8 bf16 exact halfway cases per code and parity plus subnormal-range ones: the
    stored bits are the oracle's fp32 product rounded once, ties to even."""
    from quantizations_amd.core import dequantize_4bit

    packed, st, want = _weight(family, qt, wf.SHAPE, dt)
    got = dequantize_4bit(packed, st, out_dtype=dt).t().contiguous()
    assert got.shape == want.shape and got.dtype == dt
    bad = (_bits(got) != _bits(want)).nonzero()
    assert bad.shape[0] == 0, (f"{family} {qt} {dt}: {bad.shape[0]} of {want.numel()} differ", bad[:4].tolist(),
                               [(got[tuple(i)].item(), want[tuple(i)].item()) for i in bad[:4]])


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS.get)
def test_dequantize_ties_unaligned_and_ragged(dt, qt):
    """The 16-codes-per-thread kernel (an output not 16-byte aligned) and the element-wise tail
    (n % 32 != 0) convert through store_f32 / cvt_pk / __float2bfloat16 instead of the block table:
    the same halfway cases through those conversions."""
    import oracle
    from quantizations_amd import _lib

    o = _oracle_state("ties", qt, wf.SHAPE)
    n = 64 * 40 - 21
    want = torch.from_numpy(oracle.dequantize_4bit(o.packed, o.absmax_raw, n, 64, qt)).to(dt)
    pk = torch.from_numpy(o.packed[:(n + 1) // 2].copy()).to(DEV)
    am = torch.from_numpy(o.absmax_raw[:40].copy()).to(DEV)
    for shift in (0, 4):        # elements: 0 = aligned (32 per thread + tail), 4 = 8 bytes off (16 per thread)
        buf = torch.zeros(n + 8, dtype=dt, device=DEV)
        out = buf[shift:shift + n]
        _lib.check(_lib.lib.qz_dequantize_4bit(pk.data_ptr(), n, _lib.QUANT_TYPES[qt], 64, am.data_ptr(), 0, 0, 0, 0,
                                               0, out.data_ptr(), _lib.dtype_code(dt), 0), "dequantize_4bit")
        torch.cuda.synchronize()
        bad = (_bits(out.cpu()) != _bits(want)).nonzero()
        assert bad.shape[0] == 0, (shift, bad.shape[0], bad[:4].tolist())
        assert not buf[:shift].any() and not buf[shift + n:].any()


# ---------------------------------------------------------------------------
# fused decode: the W operand of each MFMA kernel is the dequantised weight
# ---------------------------------------------------------------------------


def _assert_operand(Y, want, what):
    """Values (torch.equal: the MFMA's 1 * -0.0 + 0 reads back as +0.0)."""
    assert Y.shape == want.shape and Y.dtype == want.dtype, what
    if torch.equal(Y, want):
        return
    bad = Y != want
    tiny_ = torch.finfo(Y.dtype).tiny
    flushed = bad & (want.abs() < tiny_) & (Y == 0)
    raise AssertionError(f"{what}: {int(bad.sum())} of {want.numel()} differ ({int(flushed.sum())} of them subnormal "
                         f"weights read back as zero), first {bad.nonzero()[:3].tolist()}: got "
                         f"{Y[bad][:3].tolist()} want {want[bad][:3].tolist()}")


def _one_hot(T, K, cols, dt):
    X = torch.zeros(T, K, dtype=dt, device=DEV)
    X[torch.arange(T, device=DEV), cols] = 1
    return X


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS.get)
@pytest.mark.parametrize("family", FINITE16)
def test_gemm_tile128_w_operand(family, dt, qt):
    """gemm_4bit(route='fused') on the 128-row tile kernel, T = 256 per launch: four launches read all
    128 x 1024 weights."""
    from quantizations_amd.core import gemm_4bit

    M, K = wf.SHAPE
    packed, st, Wd = _weight(family, qt, (M, K), dt)
    for c0 in range(0, K, 256):
        cols = torch.arange(c0, c0 + 256, device=DEV)
        Y = gemm_4bit(_one_hot(256, K, cols, dt), packed, st, route="fused")
        _assert_operand(Y, Wd[:, cols].t(), f"{family} {qt} {dt} columns {c0}..")
        assert torch.isfinite(Y).all()


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS.get)
@pytest.mark.parametrize("family", FINITE16)
def test_gemm_tile256_w_operand(family, dt, qt):
    """The 256 x 256 tile kernel at its minimum (T = 4096, M = K = 256): every weight, 16 times."""
    from quantizations_amd.core import gemm_4bit

    packed, st, Wd = _weight(family, qt, (256, 256), dt)
    cols = (torch.arange(4096, device=DEV) * 37) % 256
    Y = gemm_4bit(_one_hot(4096, 256, cols, dt), packed, st, route="fused")
    _assert_operand(Y, Wd[:, cols].t(), f"{family} {qt} {dt}")


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS.get)
@pytest.mark.parametrize("family", FINITE16)
def test_multi_token_w_operand(family, dt, qt):
    """The multi-token kernel (K = 256): T = 16 in 16 launches reads all 512 x 256 weights; T = 2 reads
    two columns per launch."""
    from quantizations_amd.core import gemm_4bit

    packed, st, Wd = _weight(family, qt, (512, 256), dt)
    for c0 in range(0, 256, 16):
        cols = torch.arange(c0, c0 + 16, device=DEV)
        Y = gemm_4bit(_one_hot(16, 256, cols, dt), packed, st, route="fused")
        _assert_operand(Y, Wd[:, cols].t(), f"{family} {qt} {dt} T=16 columns {c0}..")
    for c0 in (0, 77, 254):
        cols = torch.tensor([c0, (c0 + 129) % 256], device=DEV)
        Y = gemm_4bit(_one_hot(2, 256, cols, dt), packed, st, route="fused")
        _assert_operand(Y, Wd[:, cols].t(), f"{family} {qt} {dt} T=2 columns {cols.tolist()}")


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS.get)
@pytest.mark.parametrize("pair", [("tiny14", "outlier"), ("outlier", "tiny20"), ("sweep16", "ties")], ids="+".join)
def test_grouped_multi_token_w_operand(pair, dt, qt):
    """gemm_4bit_grouped: two weights of different families (one scale format) in one launch."""
    from quantizations_amd.core import gemm_4bit_grouped

    ws = [_weight(f, qt, (512, 256), dt) for f in pair]
    items = [(p, st, None) for p, st, _ in ws]
    for c0 in (0, 64, 240):
        cols = torch.arange(c0, c0 + 16, device=DEV)
        ys = gemm_4bit_grouped(_one_hot(16, 256, cols, dt), items)
        for f, y, (_, _, Wd) in zip(pair, ys, ws):
            _assert_operand(y, Wd[:, cols].t(), f"{f} in {pair} {qt} {dt} columns {c0}..")


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS.get)
@pytest.mark.parametrize("family", FINITE16)
def test_dgrad_w_operand(family, dt, qt):
    """gemm_4bit_dgrad(route='fused'): one-hot gradients pick rows; T = 130 in four launches reads
    all 512 x 256 weights, T = 16 two more groups of rows."""
    from quantizations_amd.core import gemm_4bit_dgrad

    M, K = 512, 256
    packed, st, Wd = _weight(family, qt, (M, K), dt)
    for T, starts in ((130, range(0, M, 130)), (16, (0, 499))):
        for r0 in starts:
            rows = (torch.arange(r0, r0 + T, device=DEV)) % M
            dX = gemm_4bit_dgrad(_one_hot(T, M, rows, dt), packed, st, route="fused")
            _assert_operand(dX, Wd[rows], f"{family} {qt} {dt} T={T} rows {r0}..")


# ---------------------------------------------------------------------------
# GEMV and product routes on the existing bars
# ---------------------------------------------------------------------------


def _assert_on_bar(y, yref, dt, what):
    """assert_close on the GPU value -- after the reference itself, rounded once to the output dtype,
    has passed the same bar (else the case says nothing about the kernel)."""
    yref = np.asarray(yref, np.float64)
    assert_close(torch.from_numpy(yref).to(dt).double().numpy(), yref, dt, f"{what}: the rounded reference")
    assert torch.isfinite(y).all(), what
    assert_close(y.double().cpu().numpy(), yref, dt, what)


def _x(K, dt, seed):
    return torch.randn(K, generator=torch.Generator().manual_seed(seed)).to(dt)


GEMV_SHAPES = [(256, 2112), (64, 8192), (1024, 4096)]   # K split over waves (generic steps, few rows); full steps


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
@pytest.mark.parametrize("dt,exact", [(F16, None), (F16, True), (BF16, None), (F32, None)],
                         ids=["fp16", "fp16-exact", "bf16", "fp32"])
@pytest.mark.parametrize("shape", GEMV_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("family", ["tiny14", "outlier"])
def test_gemv_families(orc, family, shape, dt, exact, qt):
    from quantizations_amd.core import gemv_4bit

    o = _oracle_state(family, qt, shape)
    packed, st = _gpu_state(o)
    x = _x(shape[1], dt, seed=shape[0])
    y = gemv_4bit(x.to(DEV).reshape(1, -1), packed, state=st, exact_codes=exact)
    assert y.dtype == dt and y.shape == (1, shape[0])
    _assert_on_bar(y, orc.gemv(x.float().numpy(), o), dt, f"gemv {family} {shape} {dt} exact={exact} {qt}")


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "rmsnorm"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS.get)
@pytest.mark.parametrize("shape", [(64, 8192), (1024, 4096)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gemv_grouped_families(orc, shape, dt, norm):
    """tiny14 and outlier as two segments of one grouped launch, with and without the fused RMSNorm
    (the reference takes the norm kernel's output, which has its own bit-exact tests)."""
    from quantizations_amd.core import gemv_4bit_grouped
    from quantizations_amd.layer_ops import rms_norm

    K = shape[1]
    os_ = [_oracle_state(f, "nf4", shape) for f in ("tiny14", "outlier")]
    items = [(*_gpu_state(o), None) for o in os_]
    x = (_x(K, dt, seed=K) * 3).to(DEV).reshape(1, K)
    nw = (1 + 0.1 * _x(K, F32, seed=K + 1)).to(dt).to(DEV)
    ys = gemv_4bit_grouped(x, items, norm=(nw, 1e-5) if norm else None)
    xin = rms_norm(x, nw, 1e-5) if norm else x
    for f, o, y in zip(("tiny14", "outlier"), os_, ys):
        _assert_on_bar(y, orc.gemv(xin.float().cpu().numpy().ravel(), o), dt, f"grouped {f} {shape} {dt} norm={norm}")


@pytest.mark.parametrize("dt,exact", [(F16, None), (F16, True), (BF16, None)], ids=["fp16", "fp16-exact", "bf16"])
@pytest.mark.parametrize("families", [("tiny14", "outlier"), ("outlier", "tiny14")], ids="+".join)
def test_pair_silu_families(orc, families, dt, exact):
    """silu(gate) * up in one launch at the pair's minimum (full K-steps: K = 2048; 64 rows), tiny14 as
    gate and as up against outlier, against fp64 of the oracle's two GEMVs."""
    from quantizations_amd.core import gemv_4bit_pair_silu

    os_ = [_oracle_state(f, "nf4", (64, 2048)) for f in families]
    items = [(*_gpu_state(o), None) for o in os_]
    x = _x(2048, dt, seed=2)
    h = gemv_4bit_pair_silu(x.to(DEV).reshape(1, -1), items, exact_codes=exact)
    assert h is not None and h.dtype == dt
    g, u = (orc.gemv(x.float().numpy(), o) for o in os_)
    # the launch rounds gate and up to dt before the product (bit-identical to the grouped launch + silu_mul)
    g, u = (torch.from_numpy(v).to(dt).double().numpy() for v in (g, u))
    _assert_on_bar(h, g / (1 + np.exp(-g)) * u, dt, f"pair {families} {dt} exact={exact}")


@pytest.mark.parametrize("T", [1, 5, 40])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS.get)
@pytest.mark.parametrize("family", ["tiny14", "outlier"])
def test_linear4bit_forward_families(orc, family, dt, T):
    """Linear4bit.forward (its own GPU quantisation of the family) on the GEMV (T = 1), the multi-token
    kernel (5) and the fused tile kernel (40), against fp64 of the oracle's dequantised weight in the
    dtype the route multiplies (decode: the fp32 products; prefill: rounded to dt)."""
    import quantizations_amd as qa

    out_f, in_f = wf.SHAPE
    W = FAMILIES[family][0](wf.SHAPE)
    m = qa.Linear4bit(in_f, out_f, bias=False, quant_type="nf4", compute_dtype=dt)
    m.weight = qa.Params4bit(W, requires_grad=False, quant_type="nf4", module=m)
    m = m.to(DEV)
    o = _oracle_state(family, "nf4", wf.SHAPE)
    assert np.array_equal(m.weight.cpu().numpy().ravel(), o.packed)
    wref = torch.from_numpy(orc.dequantize(o))
    if T > 1:
        wref = wref.to(dt)
    X = torch.randn(1, T, in_f, generator=torch.Generator().manual_seed(T)).to(dt)
    y = m(X.to(DEV))
    assert y.shape == (1, T, out_f) and y.dtype == dt
    ref = X.double().reshape(T, in_f) @ wref.double().t()
    _assert_on_bar(y.reshape(T, out_f), ref.numpy(), dt, f"Linear4bit {family} {dt} T={T}")
