"""GPU: the memory footprint of every kernel, through the C ABI (tests/footprint.py is the harness,
tests/test_footprint.py shows that it notices).

Every case hands the library
  (a) inputs that are `guarded` views with poisoned guards (NaN / 0xFF / out-of-range ids), row strides
      above the row length and, where a route exists for it, a start that is not 16-B aligned;
  (b) outputs and scratch buffers of EXACTLY the size the header or the *_size function names, the
      payload and the guards pre-filled with the sentinel (scratch: NaN or 0xFF, never zero);
and asserts
  (c) every guard byte of every output and scratch buffer is untouched and no input changed;
  (d) the payload carries the bits of the same entry point called on plain packed clones (the same
      alignment mod 16, the same stride divisibility: the same kernel, the same summation order)
      with a zero-filled scratch;
  (e) the values against the oracle / an fp64 product of the bit-exact dequantised weight, on the
      bars the suite already has (test_gpu_parity.assert_close, integer equality for the codecs).
No address outside a live allocation is ever passed: a spill or a dependence shows by value.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import footprint as fp
import weight_families as wf
from footprint import assert_same_bits, assert_unchanged, assert_untouched, filled, guarded, same_bits
from test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
I32, I64, U8, F64 = torch.int32, torch.int64, torch.uint8, torch.float64
DT_IDS = {F16: "fp16", BF16: "bf16", F32: "fp32"}.get
QZ_ERR_SHAPE = -3


def P(t):
    return 0 if t is None else t.data_ptr()


def S():
    return torch.cuda.current_stream().cuda_stream


def L():
    from quantizations_amd import _lib

    return _lib


def _plain(t, offset_elems=0):
    """t's bits in an ordinary packed allocation, the same number of elements off the allocation's start."""
    buf = torch.empty(t.numel() + offset_elems, dtype=t.dtype, device=DEV)
    v = buf[offset_elems:].view(t.shape)
    fp.bits(v).copy_(fp.bits(t.to(DEV)))
    return v


class Bufs(dict):
    __getattr__ = dict.__getitem__


class Case:
    """The operands of one call, twice: `g` guarded (strided, offset, dirty scratch), `p` plain."""

    def __init__(self):
        self.g, self.p = Bufs(), Bufs()
        self.ins, self.outs, self.scr = [], [], []

    def inp(self, name, t, *, row_stride=None, offset_elems=0, fill="poison"):
        t = torch.as_tensor(t)
        t = (t.reshape(1) if t.dim() == 0 else t).to(DEV)
        self.g[name] = guarded(t, row_stride=row_stride, offset_elems=offset_elems, fill=fill, name=name)
        self.p[name] = _plain(t, offset_elems)
        self.ins.append(name)
        return self

    def out(self, name, shape, dtype, *, row_stride=None, offset_elems=0):
        self.g[name] = guarded(filled(shape, dtype, "sentinel", DEV), row_stride=row_stride,
                               offset_elems=offset_elems, fill="sentinel", name=name)
        self.p[name] = _plain(torch.zeros(shape, dtype=dtype), offset_elems)
        self.outs.append(name)
        return self

    def inout(self, name, t, *, row_stride=None, fill="sentinel"):
        """A buffer the call reads and updates (caches, pos, hist): given content, compared afterwards."""
        t = torch.as_tensor(t).to(DEV)
        self.g[name] = guarded(t, row_stride=row_stride, fill=fill, name=name)
        self.p[name] = _plain(t)
        self.outs.append(name)
        return self

    def scratch(self, name, numel, dtype, dirty="poison"):
        """Exactly numel elements; the guarded one dirty between sentinel guards, the plain one zeroed."""
        self.g[name] = guarded(filled(numel, dtype, dirty, DEV), fill="sentinel", name=name)
        self.p[name] = torch.zeros(numel, dtype=dtype, device=DEV)
        self.scr.append(name)
        return self

    def run(self, fn, rc=0):
        for b in (self.g, self.p):
            got = fn(b)
            assert got == rc, f"status {got}, expected {rc}"
        torch.cuda.synchronize()
        return self.check()

    def check(self):
        for n in self.ins:
            assert_unchanged(self.g[n], n)
        for n in self.outs + self.scr:
            assert_untouched(self.g[n], n)
        for n in self.outs:
            assert_same_bits(self.g[n], self.p[n], n)
        return self.g


def _randn(shape, dt, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dt)


# ---------------------------------------------------------------------------------------------
# quantise and dequantise
# ---------------------------------------------------------------------------------------------

def _np_bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.mark.parametrize("bs", [64, 4096])
@pytest.mark.parametrize("dt", [F16, BF16, F32], ids=DT_IDS)
def test_quantize_4bit_exact_size_outputs(orc, dt, bs):
    """out is exactly (n + 1) / 2 bytes and absmax exactly ceil(n / bs) floats; the input starts on a
    16-B boundary and one element past it.  Codes (the low nibble of an odd n's last byte included)
    and absmax are the oracle's."""
    lib, dtc = L().lib, L().dtype_code(dt)
    for i, n in enumerate((1, 63, 64, 65, 127, 4097, 2 * 4096 + 33)):
        for off in (0, 1):
            qt = ("nf4", "fp4")[(i + off) % 2]
            A = _randn(n, dt, 7 * n + off, 0.5)
            c = Case().inp("A", A, offset_elems=off).out("out", ((n + 1) // 2,), U8).out("absmax", (-(-n // bs),), F32)
            g = c.run(lambda b: lib.qz_quantize_4bit(P(b.A), dtc, n, bs, L().QUANT_TYPES[qt], P(b.absmax), P(b.out), S()))
            packed, am = orc.quantize_4bit_raw(A.float().numpy(), bs, qt)
            what = f"n={n} off={off} {qt}"
            assert np.array_equal(g.out.cpu().numpy(), packed), what
            assert np.array_equal(_np_bits(g.absmax.cpu().numpy()), _np_bits(am)), what


def test_blockwise_8bit_exact_size_outputs(orc):
    """qz_quantize_blockwise_8bit with `subtract` and qz_dequantize_blockwise_8bit with `offset`."""
    lib = L().lib
    code = orc.create_dynamic_map()
    for n in (1, 255, 256, 257, 4097):
        A = _randn(n, F32, n, 0.3) + 0.25
        sub = np.float32(0.25)
        c = (Case().inp("code", code).inp("A", A).inp("sub", torch.tensor([sub]))
             .out("absmax", (-(-n // 256),), F32).out("q", (n,), U8))
        g = c.run(lambda b: lib.qz_quantize_blockwise_8bit(P(b.code), P(b.A), n, 256, P(b.sub), P(b.absmax), P(b.q), S()))
        oq, oam = orc.quantize_blockwise_8bit(code, A.numpy(), 256, subtract=float(sub))
        assert np.array_equal(g.q.cpu().numpy(), oq), n
        assert np.array_equal(_np_bits(g.absmax.cpu().numpy()), _np_bits(oam)), n
        c = (Case().inp("code", code).inp("q", torch.from_numpy(oq)).inp("absmax", torch.from_numpy(oam))
             .inp("off", torch.tensor([sub])).out("out", (n,), F32))
        g = c.run(lambda b: lib.qz_dequantize_blockwise_8bit(P(b.code), P(b.q), P(b.absmax), n, 256, P(b.off), P(b.out), S()))
        want = orc.dequantize_blockwise_8bit(code, oq, oam, 256, offset=float(sub))
        assert np.array_equal(_np_bits(g.out.cpu().numpy()), _np_bits(want)), n


def test_absmax_mean_exact_dirty_workspace(orc):
    """The workspace is exactly qz_absmax_mean_workspace(n) doubles and holds the sentinel."""
    lib = L().lib
    for n in (1, 255, 257, 65537):
        am = _randn(n, F32, n).abs() + 0.01
        nws = int(lib.qz_absmax_mean_workspace(n))
        assert nws == -(-n // 1024)
        c = Case().inp("am", am).scratch("ws", nws, F64, dirty="sentinel").out("off", (1,), F32)
        g = c.run(lambda b: lib.qz_absmax_mean(P(b.am), n, P(b.ws), P(b.off), S()))
        want = np.array([orc.absmax_mean(am.numpy())], np.float32)
        assert np.array_equal(_np_bits(g.off.cpu().numpy()), _np_bits(want)), (n, g.off.item(), want)


@pytest.mark.parametrize("dq", [False, True], ids=["absmax", "dq"])
@pytest.mark.parametrize("dt", [F16, BF16, F32], ids=DT_IDS)
def test_dequantize_4bit_exact_size_output(orc, dt, dq):
    """out 16-B aligned (32 codes per thread) and one element off (16 per thread); with double quant
    qabsmax, absmax2, code2 and offset all lie inside poisoned bands.  Bits: the oracle's fp32 product
    rounded once."""
    lib, dtc = L().lib, L().dtype_code(dt)
    for i, n in enumerate((1, 31, 32, 33, 4096 + 17)):
        for off in (0, 1):
            qt = ("nf4", "fp4")[(i + off) % 2]
            o = orc.quantize_4bit(_randn(n, F32, 3 * n + off, 0.02).numpy(), 64, qt, double_quant=dq)
            c = Case().inp("A", torch.from_numpy(o.packed)).out("out", (n,), dt, offset_elems=off)
            if dq:
                c.inp("qam", torch.from_numpy(o.qabsmax)).inp("am2", torch.from_numpy(o.absmax2))
                c.inp("code2", torch.from_numpy(o.code2)).inp("offset", torch.tensor([o.offset], dtype=F32))
                sc = lambda b: (0, P(b.qam), P(b.am2), P(b.code2), P(b.offset), 256)
            else:
                c.inp("am", torch.from_numpy(o.absmax_raw))
                sc = lambda b: (P(b.am), 0, 0, 0, 0, 0)
            g = c.run(lambda b: lib.qz_dequantize_4bit(P(b.A), n, L().QUANT_TYPES[qt], 64, *sc(b), P(b.out), dtc, S()))
            assert fp.is_aligned(g.out) == (off == 0)
            want = torch.from_numpy(orc.dequantize(o)).to(dt)
            assert_same_bits(g.out.cpu(), want, f"n={n} off={off} {qt} vs the oracle")


def test_reference_abi_names(orc):
    """One call each of the five reference-ABI names, odd n and M = 3."""
    lib = L().lib
    n = 4097
    A = _randn(n, F16, 11, 0.5)
    c = Case().inp("A", A).out("absmax", (-(-n // 64),), F32).out("out", ((n + 1) // 2,), U8)
    g = c.run(lambda b: lib.cquantize_blockwise_fp16_fp4_stream(0, P(b.A), P(b.absmax), P(b.out), 64, n, S()))
    packed, am = orc.quantize_4bit_raw(A.float().numpy(), 64, "fp4")
    assert np.array_equal(g.out.cpu().numpy(), packed) and np.array_equal(_np_bits(g.absmax.cpu().numpy()), _np_bits(am))

    c = Case().inp("A", torch.from_numpy(packed)).inp("absmax", torch.from_numpy(am)).out("out", (n,), F16)
    g = c.run(lambda b: lib.cdequantize_blockwise_fp16_fp4_stream(0, P(b.A), P(b.absmax), P(b.out), 64, n, S()))
    want = torch.from_numpy(orc.dequantize_4bit(packed, am, n, 64, "fp4")).to(F16)
    assert_same_bits(g.out.cpu(), want, "cdequantize_blockwise_fp16_fp4")

    code = orc.create_dynamic_map()
    A32 = _randn(n, F32, 12, 0.3)
    c = Case().inp("code", code).inp("A", A32).out("absmax", (-(-n // 256),), F32).out("q", (n,), U8)
    g = c.run(lambda b: lib.cquantize_blockwise_fp32_stream(P(b.code), P(b.A), P(b.absmax), P(b.q), 256, n, S()))
    oq, oam = orc.quantize_blockwise_8bit(code, A32.numpy(), 256)
    assert np.array_equal(g.q.cpu().numpy(), oq) and np.array_equal(_np_bits(g.absmax.cpu().numpy()), _np_bits(oam))

    c = Case().inp("code", code).inp("q", torch.from_numpy(oq)).inp("absmax", torch.from_numpy(oam)).out("out", (n,), F32)
    g = c.run(lambda b: lib.cdequantize_blockwise_fp32_stream(P(b.code), P(b.q), P(b.absmax), P(b.out), 256, n, S()))
    assert np.array_equal(_np_bits(g.out.cpu().numpy()), _np_bits(orc.dequantize_blockwise_8bit(code, oq, oam, 256)))

    M, K = 3, 72          # K % 32 != 0: the per-element kernel
    o = orc.quantize_4bit(_randn((M, K), F32, 13, 0.02).numpy(), 64, "nf4", double_quant=False)
    x = _randn(K, F32, 14)
    c = (Case().inp("x", x).inp("B", torch.from_numpy(o.packed)).inp("absmax", torch.from_numpy(o.absmax_raw))
         .inp("lut", torch.from_numpy(orc.codebook("nf4"))).out("y", (M,), F32))
    g = c.run(lambda b: lib.cgemm_4bit_inference_naive_fp32_stream(M, 1, K, P(b.x), P(b.B), P(b.absmax), P(b.lut),
                                                                   P(b.y), M, (K + 1) // 2, M, 64, S()))
    yref = orc.gemv_4bit(x.numpy(), o.packed, o.absmax_raw, orc.codebook("nf4"), M, K, 64)
    assert_close(g.y.cpu().numpy(), yref, F32, "cgemm_4bit_inference_naive_fp32")


# ---------------------------------------------------------------------------------------------
# 4-bit weights shared by the GEMV and GEMM groups
# ---------------------------------------------------------------------------------------------

_weights = {}


class _W:
    """An [M, K] weight quantised on the GPU: packed codes, statistics, the dequantised values."""

    def __init__(self, M, K, dq, qt, seed):
        from quantizations_amd.core import quantize_4bit

        self.M, self.K, self.dq, self.qt = M, K, dq, qt
        vals = wf.outlier(seed=seed, shape=(M, K)) if (M * K) % 64 == 0 else _randn((M, K), F16, seed, 0.02)
        self.packed, self.st = quantize_4bit(vals.to(DEV), blocksize=64, quant_type=qt, compress_statistics=dq)
        self._wd = {}

    def wd(self, dt):
        """[M, K] float64 of the values qz_dequantize_4bit stores in dt (bit-exact: test_gpu_weight_range)."""
        from quantizations_amd.core import dequantize_4bit

        if dt not in self._wd:
            self._wd[dt] = dequantize_4bit(self.packed, self.st, out_dtype=dt).t().double()
        return self._wd[dt]

    def add(self, c, pre, rows=None):
        """The packed rows (all, or the slice `rows`) and the WHOLE statistics as guarded inputs."""
        B = self.packed.view(self.M, self.K // 2)
        c.inp(pre + "B", B if rows is None else B[rows])
        st = self.st
        if st.nested:
            c.inp(pre + "qam", st.absmax).inp(pre + "am2", st.state2.absmax).inp(pre + "code2", st.state2.code)
            c.inp(pre + "off", st.offset)
        else:
            c.inp(pre + "am", st.absmax)

    def scale(self, b, pre):
        """(absmax, qabsmax, absmax2, code2, offset, blocksize2) as the C ABI takes them."""
        if self.st.nested:
            return (0, P(b[pre + "qam"]), P(b[pre + "am2"]), P(b[pre + "code2"]), P(b[pre + "off"]), 256)
        return (P(b[pre + "am"]), 0, 0, 0, 0, 0)

    @property
    def bs2(self):
        return 256 if self.st.nested else 0


def weight(M, K, dq, qt="nf4", seed=0):
    key = (M, K, dq, qt, seed)
    if key not in _weights:
        _weights[key] = _W(M, K, dq, qt, seed + M + K)
    return _weights[key]


def _segments(b, ws, ys, biases=None):
    """qz_gemv_segment array of the weights ws (operands "w<i>..."), outputs b[ys[i]], biases b[biases[i]]."""
    segs = (L().GemvSegment * len(ws))()
    for i, w in enumerate(ws):
        am, qam, am2, c2, off, _ = w.scale(b, f"w{i}")
        segs[i] = L().GemvSegment(w.M, P(b[f"w{i}B"]), am, qam, am2, c2, off, 0, P(b[biases[i]]) if biases else 0,
                                  P(b[ys[i]]) if ys else 0)
    return segs


def _vp(arr):
    return ctypes.cast(arr, ctypes.c_void_p)


# ---------------------------------------------------------------------------------------------
# decode GEMV
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dq", [False, True], ids=["absmax", "dq"])
@pytest.mark.parametrize("dt", [F16, BF16, F32], ids=DT_IDS)
@pytest.mark.parametrize("K", [32, 96, 2048, 4096, 2080, 40])
def test_gemv_4bit_and_residual(dt, dq, K):
    """K = 32 / 96: part of one step; 2048 / 4096: full steps; 2080: the vector path with a ragged step;
    40: K % 32 != 0, the per-element kernel -- which an x 8 B off a 16-B boundary takes at every K.
    bias, residual and y are exactly M elements."""
    lib, dtc = L().lib, L().dtype_code(dt)
    for M in (1, 3, 7, 130):
        w = weight(M, K, dq)
        x, bias, res = _randn(K, dt, K + M), _randn(M, dt, M, 0.1), _randn(M, dt, M + 1)
        for xoff in (0, 8 // x.element_size()):
            c = Case()
            w.add(c, "w")
            c.inp("x", x, offset_elems=xoff).inp("bias", bias).inp("res", res).out("y", (M,), dt).out("y2", (M,), dt)

            def call(b):
                head = (M, K, P(b.x), dtc, P(b.wB), L().QUANT_TYPES["nf4"], 64, *w.scale(b, "w"), 0, 0, P(b.bias))
                return lib.qz_gemv_4bit(*head, P(b.y), S()) or lib.qz_gemv_4bit_residual(*head, P(b.res), P(b.y2), S())

            g = c.run(call)
            assert fp.is_aligned(g.x) == (xoff == 0)
            yref = w.wd(F32) @ x.double().to(DEV) + bias.double().to(DEV)
            assert_close(g.y.double().cpu().numpy(), yref.cpu().numpy(), dt, f"M={M} K={K} xoff={xoff}")
            assert_same_bits(g.y2, g.y + res.to(DEV), "residual epilogue")


@pytest.mark.parametrize("dq", [False, True], ids=["absmax", "dq"])
@pytest.mark.parametrize("K", [2048, 128])
def test_gemv_4bit_row_shard_unsliced_scales(dq, K):
    """Rows 5..11 of a 12-row layer: the shard's packed rows, the WHOLE scale arrays (guards around
    them) and block_base = 5 K / 64."""
    lib, dt = L().lib, F16
    Mf, r0, M = 12, 5, 7
    w = weight(Mf, K, dq)
    x = _randn(K, dt, K)
    c = Case()
    w.add(c, "w", rows=slice(r0, r0 + M))
    c.inp("x", x).out("y", (M,), dt)
    base = r0 * K // 64
    g = c.run(lambda b: lib.qz_gemv_4bit(M, K, P(b.x), 0, P(b.wB), 1, 64, *w.scale(b, "w"), base, 0, 0, P(b.y), S()))
    yref = w.wd(F32)[r0:r0 + M] @ x.double().to(DEV)
    assert_close(g.y.double().cpu().numpy(), yref.cpu().numpy(), dt, "row shard")


@pytest.mark.parametrize("dq", [False, True], ids=["absmax", "dq"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
@pytest.mark.parametrize("K", [2048, 96, 40])
def test_gemv_4bit_grouped_and_rmsnorm(dt, dq, K):
    """Three segments M = (5, 130, 2).  K = 2048: the plain and the fused-norm launch; K = 96: a partial
    step, the fused norm declines (QZ_ERR_SHAPE, nothing written); K = 40: K % 32 != 0, one launch per
    segment."""
    from quantizations_amd.layer_ops import rms_norm

    lib, dtc = L().lib, L().dtype_code(dt)
    Ms = (5, 130, 2)
    ws = [weight(M, K, dq, seed=i) for i, M in enumerate(Ms)]
    x, nw = _randn(K, dt, K, 2.0), (1.0 + 0.1 * _randn(K, F32, 1)).to(dt)
    c = Case().inp("x", x).inp("nw", nw)
    for i, (w, M) in enumerate(zip(ws, Ms)):
        w.add(c, f"w{i}")
        c.inp(f"bias{i}", _randn(M, dt, i, 0.1)).out(f"y{i}", (M,), dt)
        if K == 2048:
            c.out(f"z{i}", (M,), dt)
    eps = 1e-5

    def call(b):
        segs = _segments(b, ws, [f"y{i}" for i in range(3)], [f"bias{i}" for i in range(3)])
        rc = lib.qz_gemv_4bit_grouped(3, _vp(segs), K, P(b.x), dtc, 1, 64, ws[0].bs2, 0, S())
        zs = _segments(b, ws, [f"z{i}" if K == 2048 else f"y{i}" for i in range(3)], [f"bias{i}" for i in range(3)])
        rn = lib.qz_gemv_4bit_grouped_rmsnorm(3, _vp(zs), K, P(b.x), dtc, 1, 64, ws[0].bs2, 0, P(b.nw), eps, S())
        assert rn == (0 if K == 2048 else QZ_ERR_SHAPE)      # the route the shape was chosen for
        return rc

    g = c.run(call)
    xn = rms_norm(x.to(DEV).view(1, K), nw.to(DEV), eps).view(K)
    for i, w in enumerate(ws):
        bias = g[f"bias{i}"].double()
        assert_close(g[f"y{i}"].double().cpu().numpy(), (w.wd(F32) @ x.double().to(DEV) + bias).cpu().numpy(), dt, f"seg {i}")
        if K == 2048:
            assert_close(g[f"z{i}"].double().cpu().numpy(), (w.wd(F32) @ xn.double() + bias).cpu().numpy(), dt, f"norm seg {i}")


@pytest.mark.parametrize("dq", [False, True], ids=["absmax", "dq"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
@pytest.mark.parametrize("M,K,norm", [(6, 2048, False), (6, 2048, True), (130, 2048, False), (130, 2048, True),
                                      (64, 8192, False)])
def test_gemv_4bit_pair_silu(dt, dq, M, K, norm):
    """h is exactly M elements; K = 8192 is the geometry that splits K over waves in the grouped launch."""
    from quantizations_amd.core import gemv_4bit_grouped
    from quantizations_amd.layer_ops import silu_mul

    lib, dtc = L().lib, L().dtype_code(dt)
    ws = [weight(M, K, dq, seed=10), weight(M, K, dq, seed=11)]
    x, nw = _randn(K, dt, K + 1, 2.0), (1.0 + 0.1 * _randn(K, F32, 2)).to(dt)
    c = Case().inp("x", x).inp("nw", nw).out("h", (M,), dt)
    for i, w in enumerate(ws):
        w.add(c, f"w{i}")
    g = c.run(lambda b: lib.qz_gemv_4bit_pair_silu(_vp(_segments(b, ws, None)), K, P(b.x), dtc, 1, 64, ws[0].bs2, 0,
                                                   P(b.nw) if norm else 0, 1e-5, P(b.h), S()))
    if K == 2048:      # the header: the bits of the grouped launch + qz_silu_mul
        gu = gemv_4bit_grouped(x.to(DEV).view(1, K), [(w.packed, w.st, None) for w in ws],
                               norm=(nw.to(DEV), 1e-5) if norm else None)
        assert_same_bits(g.h, silu_mul(gu[0], gu[1]).view(M), "pair vs grouped + silu_mul")


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
def test_gemv_dense(dt):
    lib, dtc, K = L().lib, L().dtype_code(dt), 4096
    for M in (1, 5, 257):
        W, x = _randn((M, K), dt, M, 0.02), _randn(K, dt, M + 1)
        c = Case().inp("W", W).inp("x", x).out("y", (M,), dt)
        g = c.run(lambda b: lib.qz_gemv_dense(M, K, P(b.x), dtc, P(b.W), P(b.y), S()))
        assert_close(g.y.double().cpu().numpy(), (W.double() @ x.double()).numpy(), dt, f"gemv_dense M={M}")


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
@pytest.mark.parametrize("ranks", [(1, 5), (5, 64), (64, 1)])
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
def test_lora_shrink_and_adapter_gemvs(dt, ranks, norm):
    """t is exactly r0 + r1 floats and the second adapter's t_offset is r0; qz_gemv_4bit_lora reads the
    second adapter, qz_gemv_4bit_grouped_lora both (segments M = (5, 130))."""
    from quantizations_amd.layer_ops import rms_norm

    lib, dtc, K = L().lib, L().dtype_code(dt), 2048
    Ms, eps = (5, 130), 1e-5
    ws = [weight(M, K, True, seed=20 + i) for i, M in enumerate(Ms)]
    x, nw = _randn(K, dt, 3, 2.0), (1.0 + 0.1 * _randn(K, F32, 4)).to(dt)
    As = [_randn((r, K), dt, 30 + i, 0.05) for i, r in enumerate(ranks)]
    Bs = [_randn((M, r), dt, 40 + i, 0.05) for i, (M, r) in enumerate(zip(Ms, ranks))]
    scal = [torch.tensor([0.5]), torch.tensor([2.0])]
    toff = (0, ranks[0])
    c = Case().inp("x", x).inp("nw", nw).out("t", (sum(ranks),), F32)
    for i in range(2):
        ws[i].add(c, f"w{i}")
        c.inp(f"A{i}", As[i]).inp(f"lB{i}", Bs[i]).inp(f"s{i}", scal[i]).inp(f"bias{i}", _randn(Ms[i], dt, 50 + i, 0.1))
        c.out(f"y{i}", (Ms[i],), dt)
    c.out("y1s", (Ms[1],), dt)
    # without the fused norm the GEMVs take the normalised vector as their x
    xn = rms_norm(x.to(DEV).view(1, K), nw.to(DEV), eps).view(K) if norm else x.to(DEV)
    c.inp("xn", xn)

    def call(b):
        sh = (L().LoraShrinkSegment * 2)(*(L().LoraShrinkSegment(P(b[f"A{i}"]), P(b[f"s{i}"]), ranks[i], toff[i])
                                           for i in range(2)))
        rc = lib.qz_lora_shrink(2, _vp(sh), K, P(b.x), dtc, P(b.nw) if norm else 0, eps, P(b.t), S())
        w = ws[1]
        rc = rc or lib.qz_gemv_4bit_lora(Ms[1], K, P(b.xn), dtc, P(b.w1B), 1, 64, *w.scale(b, "w1"), 0, 0, P(b.bias1), 0,
                                         P(b.lB1), ranks[1], P(b.t) + 4 * toff[1], P(b.y1s), S())
        segs = _segments(b, ws, ["y0", "y1"], ["bias0", "bias1"])
        ls = (L().LoraSegment * 2)(*(L().LoraSegment(P(b[f"lB{i}"]), ranks[i], toff[i]) for i in range(2)))
        return rc or lib.qz_gemv_4bit_grouped_lora(2, _vp(segs), _vp(ls), P(b.t), K, P(b.x), dtc, 1, 64, 256, 0,
                                                   P(b.nw) if norm else 0, eps, S())

    g = c.run(call)
    xd = xn.double()
    t_ref = torch.cat([scal[i].double().to(DEV) * (As[i].double().to(DEV) @ xd) for i in range(2)])
    assert_close(g.t.double().cpu().numpy(), t_ref.cpu().numpy(), F32, "shrink")
    for i in range(2):
        yref = ws[i].wd(F32) @ xd + g[f"bias{i}"].double() + Bs[i].double().to(DEV) @ t_ref[toff[i]:toff[i] + ranks[i]]
        assert_close(g[f"y{i}"].double().cpu().numpy(), yref.cpu().numpy(), dt, f"grouped lora seg {i}")
    assert_close(g.y1s.double().cpu().numpy(), yref.cpu().numpy(), dt, "gemv lora")


# ---------------------------------------------------------------------------------------------
# GEMM routes
# ---------------------------------------------------------------------------------------------

def _gemm_4bit_case(T, M, K, dt, dq, ldy_pad, ws_bytes=0, seed=0):
    """qz_gemm_4bit with ldx = K + 8, ldy = M + ldy_pad, bias and an exact, NaN-filled workspace; returns
    the guarded buffers after every footprint check and the fp64 comparison."""
    lib, dtc = L().lib, L().dtype_code(dt)
    w = weight(M, K, dq, seed=seed)
    X, bias = _randn((T, K), dt, T + K + seed), _randn(M, dt, M, 0.1)
    c = Case()
    w.add(c, "w")
    c.inp("X", X, row_stride=K + 8).inp("bias", bias).out("Y", (T, M), dt, row_stride=M + ldy_pad)
    if ws_bytes:
        c.scratch("ws", ws_bytes // 4, F32)
    g = c.run(lambda b: lib.qz_gemm_4bit(T, M, K, P(b.X), b.X.stride(0), dtc, P(b.wB), 1, 64, *w.scale(b, "w"), P(b.bias),
                                         P(b.Y), b.Y.stride(0), P(b.ws) if ws_bytes else 0, ws_bytes, S()))
    assert g.X.stride(0) == K + 8 and g.Y.stride(0) == M + ldy_pad and c.p.Y.stride(0) == M
    yref = X.double().to(DEV) @ w.wd(dt).t() + bias.double().to(DEV)
    assert_close(g.Y.double().cpu().numpy(), yref.cpu().numpy(), dt, f"gemm_4bit T={T} M={M} K={K}")
    return g


@pytest.mark.parametrize("dq", [False, True], ids=["absmax", "dq"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
def test_gemm_4bit_multi_token_route(dt, dq):
    ws = L().lib.qz_gemm_4bit_workspace_size
    for T in (2, 3, 16):
        for M in (4, 132):
            assert ws(T, M, 256) == 0            # 2..16 tokens, K % 256 == 0: reduced in LDS
            _gemm_4bit_case(T, M, 256, dt, dq, 4)


@pytest.mark.parametrize("dq", [False, True], ids=["absmax", "dq"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
@pytest.mark.parametrize("K", [64, 320])
def test_gemm_4bit_64_and_128_tiles(dt, dq, K):
    """T <= 64 takes the 64-token tile (T = 17 because K % 256 != 0 or T > 16), above it the 128-token one;
    K / 64 < 8 steps: no split, no workspace."""
    ws = L().lib.qz_gemm_4bit_workspace_size
    for T in (1, 17, 64, 65, 129):
        for M in (4, 132):
            assert ws(T, M, K) == 0
            _gemm_4bit_case(T, M, K, dt, dq, 4)


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
def test_gemm_4bit_256_tile(dt):
    """T >= 4096 with M % 8 == 0, ldy % 8 == 0 and a 16-B-aligned Y: the 256 x 256 tile and its 16-B stores."""
    _gemm_4bit_case(4097, 264, 64, dt, True, 8)


@pytest.mark.parametrize("dq", [False, True], ids=["absmax", "dq"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
def test_gemm_4bit_split_k_exact_and_half_workspace(dt, dq):
    """K = 4096 (64 steps): T = 1, M = 4 is the smallest shape that splits.  Once with exactly
    qz_gemm_4bit_workspace_size bytes, once with half of them (the reduced split)."""
    for T, M in ((1, 4), (17, 132)):
        need = int(L().lib.qz_gemm_4bit_workspace_size(T, M, 4096))
        assert need > 0 and need % (T * M * 4) == 0 and need // (T * M * 4) >= 4
        full = _gemm_4bit_case(T, M, 4096, dt, dq, 4, ws_bytes=need)
        half = _gemm_4bit_case(T, M, 4096, dt, dq, 4, ws_bytes=need // 2)
        _gemm_4bit_case(T, M, 4096, dt, dq, 4)                                        # no workspace: no split
        assert not same_bits(full.ws, filled(need // 4, F32, "poison", DEV))          # the split ran ...
        assert not same_bits(half.ws, filled(need // 8, F32, "poison", DEV))          # ... and the reduced one


@pytest.mark.parametrize("dq", [False, True], ids=["absmax", "dq"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
@pytest.mark.parametrize("T", [2, 5, 16])
def test_gemm_4bit_grouped_and_adapter_banks(dt, dq, T):
    """Segments M = (4, 132), K = 256, ldx = K + 8.  slot has exactly ceil(T / 2) entries between
    out-of-range guards; t_stride exceeds the summed ranks and the slack keeps the sentinel."""
    lib, dtc, K = L().lib, L().dtype_code(dt), 256
    Ms, ranks, n, tps = (4, 132), (5, 16), 3, 2
    ws = [weight(M, K, dq, seed=60 + i) for i, M in enumerate(Ms)]
    X = _randn((T, K), dt, T)
    nslot = -(-T // tps)
    slot = torch.tensor([1, -1, 2, 0, 7, 1, 0, 2][:nslot], dtype=I32)
    toff, tw = (0, ranks[0]), sum(ranks)
    As = [_randn((n, r, K), dt, 70 + i, 0.05) for i, r in enumerate(ranks)]
    Bs = [_randn((n, M, r), dt, 80 + i, 0.05) for i, (M, r) in enumerate(zip(Ms, ranks))]
    scal = [torch.tensor([0.5, 1.0, 2.0]), torch.tensor([1.5, 0.25, 1.0])]
    c = Case().inp("X", X, row_stride=K + 8).inp("slot", slot, fill=n + 997).out("t", (T, tw), F32, row_stride=tw + 3)
    for i in range(2):
        ws[i].add(c, f"w{i}")
        c.inp(f"A{i}", As[i].view(n * ranks[i], K)).inp(f"lB{i}", Bs[i].view(n * Ms[i], ranks[i])).inp(f"s{i}", scal[i])
        c.inp(f"bias{i}", _randn(Ms[i], dt, 90 + i, 0.1)).out(f"y{i}", (T, Ms[i]), dt).out(f"z{i}", (T, Ms[i]), dt)

    def call(b):
        sh = (L().LoraBankShrinkSegment * 2)(*(L().LoraBankShrinkSegment(P(b[f"A{i}"]), P(b[f"s{i}"]), n, ranks[i], toff[i])
                                               for i in range(2)))
        rc = lib.qz_lora_shrink_mt(2, _vp(sh), T, K, P(b.X), b.X.stride(0), dtc, P(b.slot), tps, P(b.t), b.t.stride(0), S())
        bi = ["bias0", "bias1"]
        rc = rc or lib.qz_gemm_4bit_grouped(2, _vp(_segments(b, ws, ["y0", "y1"], bi)), T, K, P(b.X), b.X.stride(0), dtc,
                                            1, 64, ws[0].bs2, S())
        ls = (L().LoraBankSegment * 2)(*(L().LoraBankSegment(P(b[f"lB{i}"]), n, ranks[i], toff[i]) for i in range(2)))
        return rc or lib.qz_gemm_4bit_grouped_lora(2, _vp(_segments(b, ws, ["z0", "z1"], bi)), _vp(ls), P(b.t), b.t.stride(0),
                                                   P(b.slot), tps, T, K, P(b.X), b.X.stride(0), dtc, 1, 64, ws[0].bs2, S())

    g = c.run(call)
    assert g.t.stride(0) == tw + 3 and c.p.t.stride(0) == tw
    Xd = X.double().to(DEV)
    for i in range(2):
        base = Xd @ ws[i].wd(dt).t() + g[f"bias{i}"].double()
        assert_close(g[f"y{i}"].double().cpu().numpy(), base.cpu().numpy(), dt, f"grouped seg {i}")
        want = base.clone()
        for row in range(T):
            a = int(slot[row // tps])
            tr = torch.zeros(ranks[i], dtype=F64, device=DEV)
            if 0 <= a < n:
                tr = float(scal[i][a]) * (As[i][a].double().to(DEV) @ Xd[row])
                want[row] += Bs[i][a].double().to(DEV) @ tr
            assert_close(g.t[row, toff[i]:toff[i] + ranks[i]].double().cpu().numpy(), tr.cpu().numpy(), F32,
                         f"shrink_mt row {row} bank {i}")      # a row without an adapter: exactly 0
        assert_close(g[f"z{i}"].double().cpu().numpy(), want.cpu().numpy(), dt, f"bank seg {i}")


@pytest.fixture
def sched_knob():
    before = L().gemv_knobs().get("QZ_GEMM16_SCHED", 971)
    yield lambda s: L().set_gemv_knob("QZ_GEMM16_SCHED", s)
    L().set_gemv_knob("QZ_GEMM16_SCHED", before)


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
@pytest.mark.parametrize("sched", ["default", 0])
def test_gemm_16bit_strided_in_and_out(sched_knob, dt, sched):
    """ldx = K + 8 and ldy = M + 8 at the default (persistent) schedule and at schedule 0."""
    lib, dtc = L().lib, L().dtype_code(dt)
    if sched != "default":
        sched_knob(sched)
        assert L().gemv_knobs().get("QZ_GEMM16_SCHED") == sched
    for T in (1, 255, 257):
        for M in (8, 264):
            for K in (64, 192):
                W, X, bias = _randn((M, K), dt, M + K, 0.02), _randn((T, K), dt, T + K), _randn(M, dt, M, 0.1)
                c = (Case().inp("W", W).inp("X", X, row_stride=K + 8).inp("bias", bias)
                     .out("Y", (T, M), dt, row_stride=M + 8))

                def call(b):
                    assert lib.qz_gemm_16bit_ok(T, M, K, P(b.X), b.X.stride(0), P(b.W), P(b.Y), b.Y.stride(0))
                    return lib.qz_gemm_16bit(T, M, K, P(b.X), b.X.stride(0), dtc, P(b.W), P(b.bias), P(b.Y), b.Y.stride(0), S())

                g = c.run(call)
                exp = X.double() @ W.double().t() + bias.double()
                rel = ((g.Y.double().cpu() - exp).norm() / exp.norm()).item()
                assert rel <= (1e-3 if dt == F16 else 4e-3), (T, M, K, rel)      # test_gpu_gemm16_sched.py's bars


@pytest.mark.parametrize("dq", [False, True], ids=["absmax", "dq"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
def test_gemm_4bit_dgrad_strided(dt, dq):
    """ldg = M + 8, ldx = K + 4; the M = 4096 case splits the weight rows over an exact, NaN-filled
    workspace."""
    lib, dtc = L().lib, L().dtype_code(dt)
    shapes = [(T, M, K) for T in (1, 17, 129) for M in (8, 136) for K in (64, 320)] + [(17, 4096, 64)]
    for T, M, K in shapes:
        need = int(lib.qz_gemm_4bit_dgrad_workspace_size(T, M, K))
        assert (need > 0) == (M == 4096)
        w = weight(M, K, dq, seed=5)
        G = _randn((T, M), dt, T + M + K)
        c = Case()
        w.add(c, "w")
        c.inp("G", G, row_stride=M + 8).out("dX", (T, K), dt, row_stride=K + 4)
        if need:
            c.scratch("ws", need // 4, F32)
        g = c.run(lambda b: lib.qz_gemm_4bit_dgrad(T, M, K, P(b.G), b.G.stride(0), dtc, P(b.wB), 1, 64, *w.scale(b, "w"),
                                                   P(b.dX), b.dX.stride(0), P(b.ws) if need else 0, need, S()))
        if need:
            assert not same_bits(g.ws, filled(need // 4, F32, "poison", DEV))
        ref = G.double().to(DEV) @ w.wd(dt)
        assert_close(g.dX.double().cpu().numpy(), ref.cpu().numpy(), dt, f"dgrad T={T} M={M} K={K}")


# ---------------------------------------------------------------------------------------------
# layer ops
# ---------------------------------------------------------------------------------------------

def _ulp_at(y, dt):
    eps = {F16: 2.0 ** -10, BF16: 2.0 ** -7, F32: 2.0 ** -23}[dt]
    tiny = {F16: 2.0 ** -24, BF16: 2.0 ** -133, F32: 2.0 ** -149}[dt]
    return torch.clamp(y.abs().double() * eps, min=tiny)


def _rms_ref(x, w, eps):
    h = x.float()
    return w * (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps)).to(x.dtype)


@pytest.mark.parametrize("dt", [F16, BF16, F32], ids=DT_IDS)
@pytest.mark.parametrize("K", [8, 520, 4096])
def test_rmsnorm_and_add_rmsnorm_strided(dt, K):
    """rows = 3, ldx = K + 8, ldy = K + 16.  Bars: test_gpu_layer_ops.py's (2 ulp, fp32 4 ulp; the sum exact)."""
    lib, dtc, rows, eps = L().lib, L().dtype_code(dt), 3, 1e-5
    x, r, w = _randn((rows, K), dt, K, 3.0), _randn((rows, K), dt, K + 1, 3.0), (1.0 + 0.1 * _randn(K, F32, 2)).to(dt)
    c = (Case().inp("x", x, row_stride=K + 8).inp("r", r, row_stride=K + 8).inp("w", w)
         .out("y", (rows, K), dt, row_stride=K + 16).out("s", (rows, K), dt, row_stride=K + 16)
         .out("y2", (rows, K), dt, row_stride=K + 16))

    def call(b):
        rc = lib.qz_rmsnorm(P(b.x), dtc, rows, K, b.x.stride(0), P(b.w), eps, P(b.y), b.y.stride(0), S())
        return rc or lib.qz_add_rmsnorm(P(b.x), P(b.r), dtc, rows, K, b.x.stride(0), P(b.w), eps, P(b.s), P(b.y2),
                                        b.y2.stride(0), S())

    g = c.run(call)
    ulps = 4 if dt == F32 else 2
    ref = _rms_ref(x.to(DEV), w.to(DEV), eps)
    assert bool(((g.y.double() - ref.double()).abs() <= ulps * _ulp_at(ref, dt)).all())
    s = r.to(DEV) + x.to(DEV)
    assert_same_bits(g.s.contiguous(), s, "residual sum")
    ref2 = _rms_ref(s, w.to(DEV), eps)
    assert bool(((g.y2.double() - ref2.double()).abs() <= ulps * _ulp_at(ref2, dt)).all())


@pytest.mark.parametrize("dt", [F16, BF16, F32], ids=DT_IDS)
def test_silu_mul_aligned_and_offset(dt):
    lib, dtc = L().lib, L().dtype_code(dt)
    for n in (1, 7, 16385, 16384):
        for off in (0, 1):
            gate, up = _randn(n, dt, n, 4.0), _randn(n, dt, n + 1, 4.0)
            c = (Case().inp("g", gate, offset_elems=off).inp("u", up, offset_elems=off)
                 .out("y", (n,), dt, offset_elems=off))
            g = c.run(lambda b: lib.qz_silu_mul(P(b.g), P(b.u), dtc, n, P(b.y), S()))
            ref = torch.nn.functional.silu(gate.to(DEV)) * up.to(DEV)
            d = (g.y.double() - ref.double()).abs()
            assert bool((d <= 2 * _ulp_at(ref, dt) + 1e-30).all()), (n, off, float(d.max()))


def _rotate_half(x):
    x1, x2 = x[..., : x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


@pytest.mark.parametrize("dt", [F16, BF16, F32], ids=DT_IDS)
def test_rope_qk_views_of_one_fused_buffer(dt):
    """q and k are column views of one [B, S, (Hq + 2 Hkv) D] projection buffer (v's columns poisoned
    like a guard would be), the outputs [B, H, S, D] and [B, S, H, D] laid out differently, cos / sin
    broadcast over the batch with stride 0.  Bit-exact against the torch expression."""
    lib, dtc = L().lib, L().dtype_code(dt)
    B, Sq, Hq, Hk, D = 2, 3, 4, 2, 64
    width = (Hq + 2 * Hk) * D
    fused = _randn((B, Sq, width), dt, 5, 4.0)
    fused[..., (Hq + Hk) * D:] = float("nan")
    ang = torch.rand(Sq, D // 2, generator=torch.Generator().manual_seed(6)) * 50
    cos, sin = torch.cat((ang, ang), -1).cos().to(dt), torch.cat((ang, ang), -1).sin().to(dt)
    c = (Case().inp("f", fused).inp("cos", cos).inp("sin", sin)
         .out("qo", (B, Hq, Sq, D), dt).out("ko", (B, Sq, Hk, D), dt))
    ll3 = ctypes.c_longlong * 3

    def call(b):
        q_str = ll3(Sq * width, D, width)                          # (b, h, s) element strides inside the fused rows
        qo_str = ll3(Hq * Sq * D, Sq * D, D)                       # [B, H, S, D]
        ko_str = ll3(Sq * Hk * D, D, Hk * D)                       # [B, S, H, D]
        cs = (ctypes.c_longlong * 2)(0, D)
        return lib.qz_rope_qk(dtc, B, Sq, D, P(b.f), Hq, q_str, P(b.qo), qo_str, P(b.f) + Hq * D * fused.element_size(),
                              Hk, q_str, P(b.ko), ko_str, P(b.cos), P(b.sin), cs, S())

    g = c.run(call)
    fd = fused.to(DEV)
    q = fd[..., :Hq * D].view(B, Sq, Hq, D).transpose(1, 2)
    k = fd[..., Hq * D:(Hq + Hk) * D].view(B, Sq, Hk, D).transpose(1, 2)
    cd, sd = cos.to(DEV)[None, None], sin.to(DEV)[None, None]
    assert_same_bits(g.qo, ((q * cd) + (_rotate_half(q) * sd)).contiguous(), "q")
    assert_same_bits(g.ko, ((k * cd) + (_rotate_half(k) * sd)).transpose(1, 2).contiguous(), "k")


def test_decode_mask_and_rope_table_exact_size_outputs():
    lib = L().lib
    for n in (1, 7, 129):
        B = 2
        c = Case().inp("off", torch.tensor([n // 2], dtype=I64), fill=1 << 40).out("mask", (B, n), torch.bool)
        g = c.run(lambda b: lib.qz_decode_mask(P(b.off), B, n, P(b.mask), S()))
        want = (torch.arange(n) <= n // 2).expand(B, n).to(DEV)
        assert_same_bits(g.mask, want.contiguous(), "mask")
    D, T = 64, 16
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.outer(torch.arange(T).float(), inv)
    for dt in (F16, BF16, F32):
        ct, st = torch.cat((fr, fr), -1).cos().to(dt), torch.cat((fr, fr), -1).sin().to(dt)
        for Sq in (1, 7, 129):
            pos = (torch.arange(2 * Sq, dtype=I64) * 5 % T).view(2, Sq)         # inside the table: copied rows
            c = (Case().inp("pos", pos, fill=1 << 40).inp("ct", ct).inp("st", st).inp("inv", inv)
                 .out("cos", (2, Sq, D), dt).out("sin", (2, Sq, D), dt))
            g = c.run(lambda b: lib.qz_rope_table(L().dtype_code(dt), 2, Sq, D, P(b.pos), Sq, 1, P(b.ct), P(b.st), T,
                                                  P(b.inv), 1.0, P(b.cos), P(b.sin), S()))
            assert_same_bits(g.cos, ct.to(DEV)[pos.to(DEV)], "cos")
            assert_same_bits(g.sin, st.to(DEV)[pos.to(DEV)], "sin")


# ---------------------------------------------------------------------------------------------
# decode attention
# ---------------------------------------------------------------------------------------------

def _attention_operands(dt, B, Hq, Hkv, D, Lc, ps, nan_above, seed):
    g = torch.Generator().manual_seed(seed)
    width = (Hq + 2 * Hkv) * D
    f = torch.randn(B, width, generator=g).to(dt)                   # one fused q | k | v projection row per stream
    ang = torch.rand(B, D // 2, generator=g) * 6.0
    cos, sin = torch.cat((ang.cos(), ang.cos()), -1).to(dt), torch.cat((ang.sin(), ang.sin()), -1).to(dt)
    kc, vc = torch.randn(B, Hkv, Lc, D, generator=g).to(dt), torch.randn(B, Hkv, Lc, D, generator=g).to(dt)
    if nan_above:
        for b, p in enumerate(ps):
            kc[b, :, p + 1:] = float("nan")
            vc[b, :, p + 1:] = float("nan")
    return f, cos, sin, kc, vc


def _attention_ref(f, cos, sin, kc, vc, ps, Hq, Hkv, D):
    """(out [B, Hq D] float64, k cache, v cache after the call): test_gpu_decode_attention_streams.py's restatement."""
    B, Lc, dt = f.shape[0], kc.shape[2], f.dtype
    f, cos, sin, kc2, vc2 = f.to(DEV), cos.to(DEV), sin.to(DEV), kc.to(DEV).clone(), vc.to(DEV).clone()
    qh = f[:, :Hq * D].reshape(B, 1, Hq, D).transpose(1, 2)
    kh = f[:, Hq * D:(Hq + Hkv) * D].reshape(B, 1, Hkv, D).transpose(1, 2)
    v = f[:, (Hq + Hkv) * D:]
    c, s = cos.view(B, 1, 1, D), sin.view(B, 1, 1, D)
    qr, kr = (qh * c) + (_rotate_half(qh) * s), (kh * c) + (_rotate_half(kh) * s)
    for b, p in enumerate(ps):
        kc2[b, :, p] = kr[b, :, 0]
        vc2[b, :, p] = v[b].view(Hkv, D)
    pos = torch.tensor(ps, device=DEV)
    visible = torch.arange(Lc, device=DEV)[None, :] <= pos[:, None]
    G = Hq // Hkv
    kk = torch.where(visible[:, None, :, None], kc2, torch.zeros_like(kc2)).double().repeat_interleave(G, dim=1)
    vv = torch.where(visible[:, None, :, None], vc2, torch.zeros_like(vc2)).double().repeat_interleave(G, dim=1)
    sc = (qr.double() @ kk.transpose(-1, -2)) * (1.0 / math.sqrt(D))
    sc = sc.masked_fill(~visible[:, None, None, :], float("-inf"))
    out = (torch.softmax(sc, dim=-1) @ vv).transpose(1, 2).reshape(B, Hq * D)
    assert out.dtype == F64 and kc2.dtype == dt
    return out, kc2, vc2


@pytest.mark.parametrize("streams", [False, True], ids=["masked", "streams"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Lc", [8, 128, 129, 257])
def test_decode_attention_fused_rows_exact_work(dt, D, Lc, streams):
    """q, k and v are views of one fused projection row buffer; out has a row stride above Hq D; `work` is
    exactly the header's size and NaN-filled; arrive, pos and the mask lie inside guards.  In the caches
    only slot p of each (b, head) may change.  Streams: the rows above p_b are NaN; masked entry: the
    masked rows hold finite garbage."""
    lib, dtc = L().lib, L().dtype_code(dt)
    Hq, Hkv = 8, 2
    width, scale = (Hq + 2 * Hkv) * D, 1.0 / math.sqrt(D)
    nsplit = -(-Lc // 128)
    for B in (1, 3):
        ps = [Lc - 3, 0, Lc - 1][:B] if streams else [Lc - 3] * B
        f, cos, sin, kc, vc = _attention_operands(dt, B, Hq, Hkv, D, Lc, ps, streams, Lc + D + B)
        c = (Case().inp("f", f).inp("cos", cos).inp("sin", sin).inout("kc", kc).inout("vc", vc)
             .out("out", (B, Hq * D), dt, row_stride=Hq * D + 8))
        nwork = B * Hkv * nsplit * (Hq // Hkv) * (D + 2) if nsplit > 1 else 0
        if nwork:
            c.scratch("work", nwork, F32)
        if streams:
            c.inp("pos", torch.tensor(ps, dtype=I64), fill=Lc + 5)
        else:
            mask = (torch.arange(Lc) <= ps[0]).expand(B, Lc).contiguous()
            c.inp("mask", mask).inout("pos", torch.tensor([ps[0]], dtype=I64)).inout("arrive", torch.zeros(1, dtype=I32))
        es = f.element_size()

        def call(b):
            head = (dtc, B, Hq, Hkv, D, Lc, P(b.f), width, P(b.f) + Hq * D * es, width, P(b.f) + (Hq + Hkv) * D * es, width,
                    P(b.cos), P(b.sin), D if B > 1 else 0, P(b.kc), P(b.vc))
            tail = (P(b.out), b.out.stride(0), P(b.work) if nwork else 0, scale, S())
            if streams:
                return lib.qz_decode_attention_streams(*head, P(b.pos), *tail)
            return lib.qz_decode_attention(*head, P(b.mask), Lc, 1, P(b.pos), P(b.arrive), *tail)

        g = c.run(call)
        for name in ("kc", "vc"):
            ch = fp.changed_payload(g[name]).clone()
            for b, p in enumerate(ps):
                ch[b, :, p] = False
            assert not bool(ch.any()), f"{name}: a row other than slot p changed: {torch.nonzero(ch)[:4].tolist()}"
        if not streams:
            assert int(g.pos[0]) == ps[0] + 1 and int(g.arrive[0]) == 0
        ref, kc2, vc2 = _attention_ref(f, cos, sin, kc, vc, ps, Hq, Hkv, D)
        assert_same_bits(g.kc, kc2, "k cache"), assert_same_bits(g.vc, vc2, "v cache")
        tol = 2e-3 if dt == F16 else 1e-2                               # test_gpu_decode_attention.py's bars
        torch.testing.assert_close(g.out.double(), ref, atol=tol, rtol=tol)


# ---------------------------------------------------------------------------------------------
# the picks
# ---------------------------------------------------------------------------------------------

HIST_LEN, HIST_ROW, UNI_ROW = 4, 7, 9
PICK_CFG = [(1.0, 0, 1.0), (0.0, 0, 1.0), (0.7, 1, 0.9)]      # (temperature, top_k, top_p): sampled, greedy, top-1


@pytest.mark.parametrize("streams", [False, True], ids=["shared", "streams"])
@pytest.mark.parametrize("kind,dt", [("greedy", F16), ("greedy", BF16), ("greedy", F32), ("sample", F16), ("sample", BF16)],
                         ids=["greedy-fp16", "greedy-bf16", "greedy-fp32", "sample-fp16", "sample-bf16"])
def test_picks_padded_rows_exact_work(kind, dt, streams):
    """row = V + 24 with +inf in the padding of every logits row (a read of it changes the pick);
    hist_row and uniform_row above hist_len with sentinels in the slack; work exactly *_work_bytes,
    0xFF-filled.  Streams: stream 1 of 3 is dead -- its tok, pos, hist row and live word keep their bits."""
    from sampling_reference import greedy_pick, interval, pick, sample_reference

    lib, dtc = L().lib, L().dtype_code(dt)
    for V in (1, 2047, 2048, 2049, 4097):
        for B in (1, 3):
            logits = _randn((B, V), dt, V + B, 3.0)
            z = logits.float().numpy()
            ps = [2, 1, 0][:B] if streams else [2] * B
            live = [1, 0, 1][:B]
            uni = torch.rand(B, HIST_LEN, generator=torch.Generator().manual_seed(V))
            want = []
            for b in range(B):
                if kind == "greedy":
                    want.append(greedy_pick(z[b]))
                    continue
                t, k, p = PICK_CFG[b]
                ref = sample_reference(z[b], t, k, p)
                if not ref.greedy:          # u in the middle of a token's interval: no rounding moves the pick
                    lo, hi = interval(ref, pick(ref, 0.37))
                    uni[b, ps[b]] = (lo + hi) / 2
                want.append(pick(ref, float(uni[b, ps[b]])))
            hist0 = torch.arange(B * HIST_LEN, dtype=I64).view(B, HIST_LEN) - 100
            tok0 = torch.full((B,), -7, dtype=I64)
            nwork = int((lib.qz_greedy_step_work_bytes if kind == "greedy" else lib.qz_sample_step_work_bytes)(B, V))
            assert nwork > 0 and nwork % 16 == 0
            c = (Case().inp("logits", logits, row_stride=V + 24, fill=float("inf"))
                 .inout("hist", hist0, row_stride=HIST_ROW).inout("tok", tok0).scratch("work", nwork, U8))
            c.inout("pos", torch.tensor(ps if streams else ps[:1], dtype=I64))
            if kind == "sample":
                temp, topk, topp = (torch.tensor(col) for col in zip(*PICK_CFG[:B]))
                c.inp("temp", temp).inp("topk", topk.to(I32), fill=-12345).inp("topp", topp)
                c.inp("uni", uni, row_stride=UNI_ROW)
            if streams:
                c.inout("live", torch.tensor(live, dtype=I32)).inp("stop", torch.full((B,), -1, dtype=I64), fill=-2)
                c.inp("limit", torch.full((B,), 1000, dtype=I64), fill=-3)

            def call(b):
                lg = (P(b.logits), dtc, B, V, b.logits.stride(0))
                hs = (P(b.hist), b.hist.stride(0), HIST_LEN, P(b.pos))
                st = (P(b.live), P(b.stop), P(b.limit)) if streams else ()
                if kind == "greedy":
                    fn = lib.qz_greedy_step_streams if streams else lib.qz_greedy_step
                    return fn(*lg, *hs, *st, P(b.tok), P(b.work), S())
                fn = lib.qz_sample_step_streams if streams else lib.qz_sample_step
                return fn(*lg, P(b.temp), P(b.topk), P(b.topp), P(b.uni), b.uni.stride(0), *hs, *st, P(b.tok), P(b.work), S())

            g = c.run(call)
            assert g.logits.stride(0) == V + 24 and g.hist.stride(0) == HIST_ROW
            tok, hist, pos = g.tok.cpu(), g.hist.cpu(), g.pos.cpu()
            for b in range(B):
                what = f"{kind} V={V} B={B} b={b}"
                if streams and not live[b]:
                    assert int(tok[b]) == -7 and int(pos[b]) == ps[b] and torch.equal(hist[b], hist0[b]), what
                    assert int(g.live[b]) == 0, what
                    continue
                assert int(tok[b]) == want[b], (what, int(tok[b]), want[b])
                exp_row = hist0[b].clone()
                exp_row[ps[b]] = want[b]
                assert torch.equal(hist[b], exp_row), what
                if streams:
                    assert int(pos[b]) == ps[b] + 1 and int(g.live[b]) == 1, what
            if not streams:
                assert int(pos[0]) == ps[0] + 1


# ---------------------------------------------------------------------------------------------
# the public API on strided and misaligned activations
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
@pytest.mark.parametrize("T,K", [(5, 256), (17, 320)])
def test_core_gemm_4bit_strided_and_misaligned_activation(dt, T, K):
    """base[:, :K] is taken as it is (row stride K + 8), base[:, 1:K+1] is 2 B off and copied: both the
    bits of the contiguous call."""
    from quantizations_amd.core import gemm_4bit

    M = 132
    w = weight(M, K, True, seed=7)
    base = guarded(_randn((T, K + 8), dt, T).to(DEV))
    bias = _randn(M, dt, 1, 0.1).to(DEV)
    for view in (base[:, :K], base[:, 1:K + 1]):
        assert view.stride(0) == K + 8 and not view.is_contiguous()
        y = gemm_4bit(view, w.packed, w.st, bias, route="fused")
        assert_same_bits(y, gemm_4bit(view.contiguous(), w.packed, w.st, bias, route="fused"), "gemm_4bit")
    assert fp.is_aligned(base[:, :K]) and not fp.is_aligned(base[:, 1:K + 1])
    assert_unchanged(base)
    yref = base[:, :K].double() @ w.wd(dt).t() + bias.double()
    assert_close(gemm_4bit(base[:, :K], w.packed, w.st, bias, route="fused").double().cpu().numpy(), yref.cpu().numpy(), dt)


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
@pytest.mark.parametrize("T,K", [(5, 256), (17, 320)])
def test_core_gemm_4bit_dgrad_strided_and_misaligned_gradient(dt, T, K):
    from quantizations_amd.core import gemm_4bit_dgrad

    M = 136
    w = weight(M, K, True, seed=8)
    base = guarded(_randn((T, M + 8), dt, T + 1).to(DEV))
    for view in (base[:, :M], base[:, 1:M + 1]):
        assert view.stride(0) == M + 8 and not view.is_contiguous()
        dx = gemm_4bit_dgrad(view, w.packed, w.st, route="fused")
        assert_same_bits(dx, gemm_4bit_dgrad(view.contiguous(), w.packed, w.st, route="fused"), "gemm_4bit_dgrad")
    assert_unchanged(base)
    ref = base[:, :M].double() @ w.wd(dt)
    assert_close(gemm_4bit_dgrad(base[:, :M], w.packed, w.st, route="fused").double().cpu().numpy(), ref.cpu().numpy(), dt)


@pytest.mark.parametrize("T", [1, 5])
def test_linear4bit_forward_transposed_input(T):
    """A transposed, non-contiguous input (element stride != 1): the bits of the contiguous call."""
    import quantizations_amd as qa

    M, K, dt = 132, 256, F16
    W = wf.outlier(seed=9, shape=(M, K))
    m = qa.Linear4bit(K, M, bias=True, compute_dtype=None, quant_type="nf4")
    m.weight = qa.Params4bit(W.clone(), requires_grad=False, quant_type="nf4", module=m)
    with torch.no_grad():
        m.bias.copy_(_randn(M, F32, 2, 0.1))
    m = m.to(DEV)
    base = _randn((K, T + 1), dt, T).to(DEV)
    x = base.t()[:T]
    assert x.shape == (T, K) and x.stride(-1) != 1 and not x.is_contiguous()
    with torch.no_grad():
        y, yc = m(x.unsqueeze(0)), m(x.contiguous().unsqueeze(0))
    assert y.shape == (1, T, M)
    assert_same_bits(y, yc, "Linear4bit.forward")
    from quantizations_amd.core import dequantize_4bit

    Wd = dequantize_4bit(m.weight.data, m.weight.quant_state, out_dtype=dt).t().double()
    yref = x.double() @ Wd.t() + m.bias.detach().to(dt).double()
    assert_close(y.double().cpu().numpy(), yref.cpu().numpy(), dt, "Linear4bit")
