"""GPU: operands whose element and byte offsets pass 2^31 and 2^32 -- the 64-bit casts and the 32-bit
guards of the kernels, entered on a GPU instead of read.

What each test enters:
  gemv_4bit, M = 524287 (K = 8192)   the vector GEMV at the top of its 32-bit range: `row * K` and the
                                     block index as uint32 for rows >= 262144 (elements >= 2^31), the
                                     packed row base as size_t past 2^31 bytes (make_params' guard
                                     M K + 2048 < 2^32 is met with 6144 elements to spare)
  gemv_4bit, M = 524288              M K = 2^32: the guard sends it to gemv_generic_body, `(long long)row * K`
  quantize_4bit / dequantize_4bit    n = 2^31 + 2^20 + 64: `long long e` / `e0` past 2^31 elements, the
                                     16-bit operand past 4 GiB
  static cache [72, 8, 32768, 128]   attn_core.h's `(long long)` cache row (stream 32 starts at 2^31 bytes,
                                     stream 64 at 2^32 bytes = 2^31 elements), k_verify_kv_write's and
                                     k_prefill_kv_write's `slot`, prefill_core.h's kg / vg bases
  logits rows at 2^30 + 8 elements   `(size_t)r * row`: row 2 starts past 2^32 bytes (fp32: row 1 does).  The
                                     greedy pick is entered by the fp16 and the fp32 view; sample.hip, logits.hip
                                     and logprobs.hip by the fp16 view only (they have no fp32 kernels: fp32
                                     logits take torch ops there)

  gemm_4bit fused, M = 524288       gemm_mt.hip's `ebase` (T = 2, 16) and gemm_4bit.hip's 128-row tile kernel
                                     (T = 64): `(size_t)wrow * row_bytes`, `(long long)wrow * K`, `(size_t)t * ldy`
  activation stride 2^19 - 8 / 2^19  the guard T ldx 2 < 2^32 of gemm_4bit.hip (256 x 256 tile kernel below it,
                                     128-row tile kernel at it) and of qz_gemm_16bit_ok
  page pools of 16384 + 16 pages     (kv8: 32768 + 16) `crow` / `blk8`, the writers' `slot` / `blk`, prefill_core.h's
                                     `base` / `blk` past 2^31 and 2^32 bytes

  gemm_4bit fused, T = 4096,        the 256 x 256 tile kernel k_gemm_4bit_8p over rows on both sides of 2^31
  M = 262144 + 512                   elements: `(size_t)wrow * (K >> 1)`, `blk_row` / `blk_row_s`, the epilogue's
                                     `(size_t)t * ldy` (2.2 GiB of output); compared on scale_cases.boundary_rows

References.  The big weight is random bytes with random scales, built on the device
(scale_cases.big_weight); its reference dequantises 16384 rows at a time in plain torch and multiplies
in float64 on the GPU, one pass per (quant type, scale kind) shared by the tests; a one-hot's
reference is a gather.  Bars: test_gpu_parity.assert_close per chunk of 16384 rows.  Everything else
is bit equality with the same kernel on a small operand: slices of 2^24 elements (quantise /
dequantise, by block independence), a B = 1 copy of the stream or the same pages in a small pool
(attention), a contiguous copy of the rows (logits).

Memory rules.  A test allocates at most 12 GiB on the device, builds everything with torch on the
device (never more than 1 GiB on the host), touches only the bytes it needs (torch.empty for the
rest), drops its tensors and calls torch.cuda.empty_cache() when done.  A test skips only when
torch.cuda.mem_get_info() shows less than its need plus 2 GiB free, and the reason names both figures.
"""
import math

import pytest
import torch

import scale_cases as sc
from test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
GIB = 1 << 30
K = sc.BIG_K
ONE_HOT = (0, 4097, K - 1)


def _need(gib, what):
    free, _ = torch.cuda.mem_get_info()
    if free < (gib + 2) * GIB:
        pytest.skip(f"{what}: needs {gib} GiB + 2 GiB free on the device, {free / GIB:.1f} GiB are free")


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


@pytest.fixture(scope="module")
def big():
    """The 524288 x 8192 weight (2 GiB of codes, 256 MiB of scales) and the cache of its references."""
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * GIB:
        pytest.skip(f"the big weight and its reference: need 10 GiB + 2 GiB free on the device, {free / GIB:.1f} GiB are free")
    w = sc.big_weight(DEV)
    w["refs"] = {}
    yield w
    w.clear()
    torch.cuda.empty_cache()


def _xs():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(K, generator=g)
    return {F16: x.to(F16).to(DEV), BF16: x.to(BF16).to(DEV)}


def _reference(big, qt, nested):
    """One pass over the weight, 16384 rows at a time: fp64 of the dense products for the fp16 and the
    bf16 activation, and the one-hot columns (a gather of the fp32 product code x scale)."""
    key = (qt, nested)
    if key not in big["refs"]:
        from quantizations_amd.core import get_4bit_type

        code = get_4bit_type(qt, device=DEV)
        xs = _xs()
        X = torch.stack((xs[F16].double(), xs[BF16].double()), 1)             # [K, 2]
        dense = torch.empty((sc.BIG_ROWS, 2), dtype=torch.float64, device=DEV)
        cols = torch.empty((sc.BIG_ROWS, len(ONE_HOT)), dtype=torch.float64, device=DEV)
        for r0 in range(0, sc.BIG_ROWS, sc.REF_ROWS):
            Wd = sc.dequantize_rows(big, r0, r0 + sc.REF_ROWS, code, nested)
            cols[r0:r0 + sc.REF_ROWS] = Wd[:, list(ONE_HOT)].double()
            dense[r0:r0 + sc.REF_ROWS] = Wd.double() @ X
            del Wd
        big["refs"][key] = (dense, cols)
    return big["refs"][key]


def _assert_rows(y, yref, dt, what):
    """assert_close per chunk of REF_ROWS rows; prints the worst relative error of a chunk."""
    y, yref = y.double().reshape(-1).cpu().numpy(), yref.reshape(-1).cpu().numpy()
    assert y.shape == yref.shape
    worst = 0.0
    for r0 in range(0, y.shape[0], sc.REF_ROWS):
        a, b = y[r0:r0 + sc.REF_ROWS], yref[r0:r0 + sc.REF_ROWS]
        assert_close(a, b, dt, f"{what} rows {r0}..")
        worst = max(worst, float(((a - b) ** 2).sum() ** 0.5 / max((b ** 2).sum() ** 0.5, 1e-30)))
    return worst


@pytest.mark.parametrize("nested", [False, True], ids=["plain", "dq"])
@pytest.mark.parametrize("qt", ["nf4", "fp4"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("M", [524287, 524288], ids=["vector", "generic"])
def test_gemv_4bit_across_2_to_the_31_elements(big, M, dt, qt, nested):
    from quantizations_amd.core import gemv_4bit

    assert (M * K + 2048 < 1 << 32) == (M == 524287), "make_params' guard splits the two cases"
    dense, cols = _reference(big, qt, nested)
    st = sc.big_state(big, M, qt, nested, dt)
    packed = big["packed"][:M * K // 2]
    x = _xs()[dt]
    y = gemv_4bit(x.reshape(1, 1, K), packed, state=st)
    torch.cuda.synchronize()
    assert y.shape == (1, 1, M) and y.dtype == dt and bool(torch.isfinite(y).all())
    what = f"gemv_4bit M={M} {dt} {qt} {'dq' if nested else 'plain'}"
    ref = dense[:M, 0 if dt == F16 else 1]
    worst = {"dense": _assert_rows(y, ref, dt, what + " dense")}
    for i, k in enumerate(ONE_HOT):
        e = torch.zeros(K, dtype=dt, device=DEV)
        e[k] = 1
        worst[f"one-hot {k}"] = _assert_rows(gemv_4bit(e.reshape(1, 1, K), packed, state=st), cols[:M, i], dt,
                                             what + f" one-hot {k}")
    if dt == F16 and qt == "nf4" and not nested:     # the residual epilogue, once per route
        res = torch.randn(M, generator=torch.Generator().manual_seed(5)).to(dt).to(DEV)
        yr = gemv_4bit(x.reshape(1, 1, K), packed, state=st, residual=res)
        assert torch.equal(_bits(yr.reshape(-1)), _bits(res + y.reshape(-1))), "residual + y, the torch add's bits"
    print(f"{what}: worst relative error of a 16384-row chunk " + ", ".join(f"{n} {v:.2e}" for n, v in worst.items())
          + " (bar 1e-3; bf16 figures are raw, the bar applies after the output format's own rounding is removed)")


# ---------------------------------------------------------------------------
# gemm_4bit(route="fused") over the same weight: the multi-token kernel and the 128-row tile kernel
# ---------------------------------------------------------------------------

GEMM_T = {2: slice(0, 2), 16: slice(2, 18), 64: slice(18, 82)}
GEMM_COMBOS = [("nf4", True, F16), ("fp4", False, BF16)]


def _gemm_x(dt):
    return torch.randn((82, K), generator=torch.Generator().manual_seed(13)).to(dt).to(DEV)


def _gemm_reference(big, qt, nested, dt):
    """fp64 of X . W^T for the 82 token rows of GEMM_T, W = the dequantised weight rounded once to dt
    (the MFMA operand, test_gpu_weight_range.py's w-operand contract): [BIG_ROWS, 82]."""
    key = ("gemm", qt, nested, dt)
    if key not in big["refs"]:
        from quantizations_amd.core import get_4bit_type

        code = get_4bit_type(qt, device=DEV)
        Xt = _gemm_x(dt).double().t().contiguous()
        ref = torch.empty((sc.BIG_ROWS, 82), dtype=torch.float64, device=DEV)
        for r0 in range(0, sc.BIG_ROWS, sc.REF_ROWS):
            ref[r0:r0 + sc.REF_ROWS] = sc.dequantize_rows(big, r0, r0 + sc.REF_ROWS, code, nested).to(dt).double() @ Xt
        big["refs"][key] = ref
    return big["refs"][key]


@pytest.mark.parametrize("T", sorted(GEMM_T))
@pytest.mark.parametrize("qt,nested,dt", GEMM_COMBOS, ids=["nf4-dq-fp16", "fp4-plain-bf16"])
def test_gemm_4bit_fused_across_2_to_the_31_elements(big, qt, nested, dt, T):
    """M K = 2^32 codes: gemm_mt.hip's `ebase` (T = 2, 16) and gemm_4bit.hip's `(size_t)wrow * row_bytes`,
    `(long long)wrow * K` and `(size_t)t * ldy` (T = 64, the 128-row tile kernel) past 2^31."""
    from quantizations_amd.core import gemm_4bit

    M = sc.BIG_ROWS
    ref = _gemm_reference(big, qt, nested, dt)[:, GEMM_T[T]]
    st = sc.big_state(big, M, qt, nested, dt)
    Y = gemm_4bit(_gemm_x(dt)[GEMM_T[T]].contiguous(), big["packed"], st, route="fused")
    torch.cuda.synchronize()
    assert Y.shape == (T, M) and Y.dtype == dt and bool(torch.isfinite(Y).all())
    y, r = Y.t().double().cpu().numpy(), ref.cpu().numpy()
    worst = 0.0
    for r0 in range(0, M, sc.REF_ROWS):
        a, b = y[r0:r0 + sc.REF_ROWS], r[r0:r0 + sc.REF_ROWS]
        assert_close(a, b, dt, f"gemm_4bit fused T={T} {qt} {dt} rows {r0}..")
        worst = max(worst, float(((a - b) ** 2).sum() ** 0.5 / (b ** 2).sum() ** 0.5))
    print(f"gemm_4bit fused T={T} M={M} {qt} {'dq' if nested else 'plain'} {dt}: worst relative error of a 16384-row chunk "
          f"{worst:.2e} (bar 1e-3; bf16 raw, the bar applies after the output format's own rounding is removed)")


@pytest.mark.parametrize("qt,nested,dt", GEMM_COMBOS + [("nf4", True, BF16)], ids=["nf4-dq-fp16", "fp4-plain-bf16", "nf4-dq-bf16"])
def test_gemm_4bit_tile256_on_rows_around_2_to_the_31_elements(big, qt, nested, dt):
    """T = 4096 at M = 262144 + 512: the 256 x 256 tile kernel; row 262144 starts at element 2^31.  Compared
    on boundary_rows: the first and last 64 rows, the 64 around row 262144 and 4096 random ones."""
    from quantizations_amd.core import gemm_4bit, get_4bit_type

    _need(4, "gemm_4bit T = 4096: 2.2 GiB of output and its reference")
    T, M = 4096, 262144 + 512
    rows = sc.boundary_rows(M, K)
    assert set(range(262144 - 32, 262144 + 32)) <= set(rows) and rows[-1] == M - 1
    X = torch.randn((T, K), generator=torch.Generator().manual_seed(17)).to(dt).to(DEV)
    Wd = sc.dequantize_row_list(big, rows, get_4bit_type(qt, device=DEV), nested).to(dt)      # the MFMA operand
    ref = (Wd.double() @ X.double().t()).cpu().numpy()                                       # [rows, T]
    st = sc.big_state(big, M, qt, nested, dt)
    Y = gemm_4bit(X, big["packed"][:M * K // 2], st, route="fused")
    torch.cuda.synchronize()
    assert Y.shape == (T, M) and Y.dtype == dt
    y = Y[:, torch.tensor(rows, device=DEV)].t().double().cpu().numpy()
    del Y
    worst, step = 0.0, 512
    for i in range(0, len(rows), step):
        a, b = y[i:i + step], ref[i:i + step]
        assert_close(a, b, dt, f"gemm_4bit T=4096 {qt} {dt} rows {rows[i]}..{rows[min(i + step, len(rows)) - 1]}")
        worst = max(worst, float(((a - b) ** 2).sum() ** 0.5 / (b ** 2).sum() ** 0.5))
    print(f"gemm_4bit fused T={T} M={M} {qt} {'dq' if nested else 'plain'} {dt}: {len(rows)} boundary rows, worst relative "
          f"error of {step} rows {worst:.2e} (bar 1e-3; bf16 raw, the bar applies after the output format's own rounding is removed)")
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# ---------------------------------------------------------------------------
# the activation stride guard T * ldx * 2 < 2^32 of gemm_4bit.hip and gemm_16bit.hip
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("ldx", [(1 << 19) - 8, 1 << 19], ids=["below", "at"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
def test_activation_stride_guard(dt, ldx):
    """X [4096, 512] inside a 4-GiB allocation.  ldx = 2^19 - 8: T ldx 2 is 65536 below 2^32, the 256 x 256
    tile kernel's 32-bit byte offsets pass 2^31 from row 2049 on.  ldx = 2^19: the guard sends gemm_4bit
    to the 128-row tile kernel (`(size_t)t * ldx`) and makes gemm_16bit decline.  Only the K columns
    that are read are written."""
    from quantizations_amd.core import dequantize_4bit, gemm_16bit, gemm_4bit, quantize_4bit

    _need(5, "a 4-GiB activation buffer")
    T, Kx, M = 4096, 512, 512
    assert (T * ldx * 2 < 1 << 32) == (ldx < 1 << 19) and (T - 1) * ldx * 2 > 1 << 31
    g = torch.Generator(device=DEV).manual_seed(ldx)
    base = torch.empty((T - 1) * ldx + Kx, dtype=dt, device=DEV)
    X = base.as_strided((T, Kx), (ldx, 1))
    X.copy_(torch.randn((T, Kx), device=DEV, generator=g).to(dt))
    W = (torch.randn((M, Kx), device=DEV, generator=g) * 0.05).to(dt)
    packed, st = quantize_4bit(W, blocksize=64, quant_type="nf4")
    Wd = dequantize_4bit(packed, st, out_dtype=dt).t().contiguous()       # [M, K]: the operand of both kernels
    ref = (X.double() @ Wd.double().t()).cpu().numpy()
    Y = gemm_4bit(X, packed, st, route="fused")
    torch.cuda.synchronize()
    assert Y.shape == (T, M)
    assert_close(Y.double().cpu().numpy(), ref, dt, f"gemm_4bit fused ldx={ldx} {dt}")
    Y16 = gemm_16bit(X, Wd)
    torch.cuda.synchronize()
    assert Y16 is not None or ldx == 1 << 19, "below the guard qz_gemm_16bit takes the shape"
    if Y16 is not None:      # at the guard None is a pass; a wrong result is not
        assert Y16.shape == (T, M)
        assert_close(Y16.double().cpu().numpy(), ref, dt, f"gemm_16bit ldx={ldx} {dt}")
    print(f"activation stride {ldx} {dt}: gemm_4bit fused on the bar" + ("; gemm_16bit declines" if Y16 is None else "; gemm_16bit on the bar"))
    del base, X, Y, Y16
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# quantise / dequantise past 2^31 elements
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("bs", [64, 4096])
@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
def test_quantize_dequantize_past_2_to_the_31_elements(dt, bs):
    from quantizations_amd.core import QuantState, dequantize_4bit, get_4bit_type, quantize_4bit

    _need(10, "quantize / dequantize of 2^31 + 2^20 + 64 elements")
    n, step = (1 << 31) + (1 << 20) + 64, 1 << 24
    qt = "nf4" if bs == 64 else "fp4"
    g = torch.Generator(device=DEV).manual_seed(bs)
    A = torch.empty(n, dtype=dt, device=DEV)
    for s in range(0, n, 1 << 28):
        A[s:s + (1 << 28)] = (torch.randn(min(1 << 28, n - s), device=DEV, generator=g) * 0.02).to(dt)
    packed, st = quantize_4bit(A, blocksize=bs, quant_type=qt, compress_statistics=False)
    assert packed.numel() == n // 2 and st.absmax.numel() == -(-n // bs)
    for s in range(0, n, step):
        e = min(s + step, n)
        p1, s1 = quantize_4bit(A[s:e], blocksize=bs, quant_type=qt, compress_statistics=False)
        assert torch.equal(packed[s // 2:e // 2], p1), ("packed bytes", s)
        assert torch.equal(_bits(st.absmax[s // bs:-(-e // bs)]), _bits(s1.absmax)), ("absmax", s)
    del A, p1, s1
    torch.cuda.empty_cache()
    W = dequantize_4bit(packed, st, out_dtype=dt)
    assert W.shape == (n,) and W.dtype == dt
    code = get_4bit_type(qt, device=DEV)
    for s in range(0, n, step):
        e = min(s + step, n)
        st1 = QuantState(absmax=st.absmax[s // bs:-(-e // bs)], shape=torch.Size((e - s,)), dtype=dt, blocksize=bs,
                         code=code, quant_type=qt)
        w1 = dequantize_4bit(packed[s // 2:e // 2], st1, out_dtype=dt)
        assert torch.equal(_bits(W[s:e]), _bits(w1)), ("dequantised values", s)
    torch.cuda.synchronize()
    print(f"quantize / dequantize {dt} blocksize {bs}: {-(-n // step)} slices of 2^24 elements bit-equal to the call on all "
          f"{n} elements")
    del W, packed, st
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# attention over a static cache of 9 GiB
# ---------------------------------------------------------------------------

def test_attention_addresses_in_a_static_cache_past_4_gib():
    from quantizations_amd import layer_ops as lo

    _need(11, "two static caches [72, 8, 32768, 128] fp16")
    B, Hq, Hkv, L, D, dt = 72, 16, 8, 32768, 128, F16
    row_bytes = Hkv * L * D * 2
    assert 32 * row_bytes == 1 << 31 and 64 * row_bytes == 1 << 32     # streams 31 | 32 and 63 | 64 meet there
    tested = {0: 0, 31: 8192, 32: L - 1, 63: 8192 + 77, 64: L - 1, 71: 20000}
    g = torch.Generator(device=DEV).manual_seed(72)
    kc = torch.empty((B, Hkv, L, D), dtype=dt, device=DEV)
    vc = torch.empty_like(kc)
    for b, p in tested.items():                       # only the rows a tested stream can see are written
        n = min(p + 65, L)
        kc[b, :, :n] = torch.randn((Hkv, n, D), device=DEV, generator=g).to(dt)
        vc[b, :, :n] = torch.randn((Hkv, n, D), device=DEV, generator=g).to(dt)
    ps = [tested.get(b, 0) for b in range(B)]
    pos = torch.tensor(ps, dtype=torch.int64, device=DEV)
    scale = 1.0 / math.sqrt(D)
    for form, T in (("streams", 1), ("verify", 4), ("prefill", 65)):
        q = torch.randn((B, T, Hq * D), device=DEV, generator=g).to(dt)
        k = torch.randn((B, T, Hkv * D), device=DEV, generator=g).to(dt)
        v = torch.randn((B, T, Hkv * D), device=DEV, generator=g).to(dt)
        ang = torch.rand((B, T, D // 2), device=DEV, generator=g) * 6.0
        cos, sin = torch.cat((ang.cos(), ang.cos()), -1).to(dt), torch.cat((ang.sin(), ang.sin()), -1).to(dt)
        length = torch.full((B,), T, dtype=torch.int64, device=DEV)
        solo = {b: (kc[b:b + 1].clone(), vc[b:b + 1].clone()) for b in tested}

        def run(q, k, v, cos, sin, kc, vc, pos, length):
            if form == "streams":
                return lo.decode_attention_streams(q, k, v, cos, sin, kc, vc, pos, Hq, scale)
            if form == "verify":
                return lo.decode_attention_verify(q, k, v, cos, sin, kc, vc, pos, Hq, scale)
            return lo.prefill_attention(q, k, v, cos, sin, kc, vc, pos, length, Hq, scale)

        out = run(q, k, v, cos, sin, kc, vc, pos, length)
        for b, (k1, v1) in solo.items():
            s = slice(b, b + 1)
            o1 = run(q[s], k[s], v[s], cos[s], sin[s], k1, v1, pos[s], length[s])
            assert torch.equal(_bits(out[s]), _bits(o1)), (form, b, "output bits of the stream alone")
            assert torch.equal(_bits(kc[s]), _bits(k1)) and torch.equal(_bits(vc[s]), _bits(v1)), (form, b, "cache bits")
            legal = max(0, min(T, L - ps[b]))
            assert not bool(torch.isnan(out[b, :legal]).any()) and bool(torch.isnan(out[b, legal:]).all()), (form, b)
        torch.cuda.synchronize()
        print(f"static cache past 4 GiB, {form} (T = {T}): streams {sorted(tested)} bit-equal to their B = 1 calls")
        del solo, out
    del kc, vc
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# page pools past 4 GiB
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kv8", [False, True], ids=["16bit", "kv8"])
def test_attention_addresses_in_page_pools_past_4_gib(kv8):
    """Pools of 16384 + 16 pages (kv8: 32768 + 16), 256 KiB (129 KiB) a page: page 8192 (kv8: 16257) is
    the first at or past 2^31 bytes, page 16384 (32514) the first past 2^32.  The stream's table names the
    pages on both sides of each, the last page and pages 8191, 8192, 16383 and 16384; the same pages copied into a small pool under a renumbered table give the same bits --
    the addresses differ, nothing else.  attn_core.h's `crow` / `blk8`, the paged writers' `slot` / `blk`
    and prefill_core.h's `base` / `blk`."""
    from quantizations_amd import layer_ops as lo

    _need(10, "two page pools of 4.1 GiB")
    Hq, Hkv, D, dt = 16, 8, 128, F16
    P = (32768 if kv8 else 16384) + 16
    page_bytes = Hkv * 128 * (D + 1 if kv8 else 2 * D)
    b31, b32 = -(-(1 << 31) // page_bytes), -(-(1 << 32) // page_bytes)      # the first page at or past 2^31 / 2^32 bytes
    assert b32 < P and (kv8 or (b31, b32) == (8192, 16384))
    pages = list(dict.fromkeys([0, b31 - 1, b31, b32 - 1, b32, P - 1, 8191, 8192, 16383, 16384, 77, 5]))
    NP = len(pages)
    g = torch.Generator(device=DEV).manual_seed(P)
    shape = (P, Hkv, 128 * (D + 1)) if kv8 else (P, Hkv, 128, D)
    pools, small = [], []
    for _ in range(2):
        pool = torch.empty(shape, dtype=torch.uint8 if kv8 else dt, device=DEV)       # only the named pages are written
        for pg in pages:
            if kv8:     # finite codes (no 0x7F / 0xFF), scales 2^-7 .. 2^2
                codes = torch.randint(0, 0x78, (Hkv, 128 * D), device=DEV, generator=g, dtype=torch.uint8)
                codes |= torch.randint(0, 2, (Hkv, 128 * D), device=DEV, generator=g, dtype=torch.uint8) << 7
                scales = torch.randint(120, 130, (Hkv, 128), device=DEV, generator=g, dtype=torch.uint8)
                pool[pg] = torch.cat((codes, scales), -1)
            else:
                pool[pg] = torch.randn((Hkv, 128, D), device=DEV, generator=g).to(dt)
        pools.append(pool)
        small.append(pool[torch.tensor(pages, device=DEV)].clone())
    table = torch.tensor([pages], dtype=torch.int32, device=DEV)
    table_s = torch.arange(NP, dtype=torch.int32, device=DEV).view(1, NP)
    scale = 1.0 / math.sqrt(D)
    sfx = "_kv8" if kv8 else ""
    for form, T, p0 in (("decode_attention_paged", 1, 128 * NP - 1), ("decode_attention_verify_paged", 4, 126),
                        ("prefill_attention_paged", 65, 128 * 6 - 30)):
        q = torch.randn((1, T, Hq * D), device=DEV, generator=g).to(dt)
        k = torch.randn((1, T, Hkv * D), device=DEV, generator=g).to(dt)
        v = torch.randn((1, T, Hkv * D), device=DEV, generator=g).to(dt)
        ang = torch.rand((1, T, D // 2), device=DEV, generator=g) * 6.0
        cos, sin = torch.cat((ang.cos(), ang.cos()), -1).to(dt), torch.cat((ang.sin(), ang.sin()), -1).to(dt)
        pos = torch.tensor([p0], dtype=torch.int64, device=DEV)
        extra = (torch.tensor([T], dtype=torch.int64, device=DEV),) if form.startswith("prefill") else ()
        fn = getattr(lo, form + sfx)
        assert getattr(lo, form + sfx + "_supported")(q, cos, *pools, table, pos, *extra, Hq)
        out = fn(q, k, v, cos, sin, *pools, table, pos, *extra, Hq, scale)
        ref = fn(q, k, v, cos, sin, *small, table_s, pos, *extra, Hq, scale)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(out).any()), form
        assert torch.equal(_bits(out), _bits(ref)), (form, "output bits")
        for pool, sm in zip(pools, small):
            assert torch.equal(_bits(pool[torch.tensor(pages, device=DEV)]), _bits(sm)), (form, "the pages after the call")
        print(f"page pools past 4 GiB ({'kv8' if kv8 else '16-bit'}, P = {P}), {form + sfx} T = {T} at {p0}: bit-equal to the "
              f"same pages in a pool of {NP}")
    del pools, small
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# logits rows 2 GiB apart
# ---------------------------------------------------------------------------

ROW = (1 << 30) + 8


def _logit_rows(V, dt, seed):
    """(view [3, V] with a row stride of 2^30 + 8 elements, contiguous copy).  Only the 3 V elements of
    the view are ever written."""
    base = torch.empty(2 * ROW + V, dtype=dt, device=DEV)
    view = base.as_strided((3, V), (ROW, 1))
    g = torch.Generator(device=DEV).manual_seed(seed)
    view.copy_((torch.randn((3, V), device=DEV, generator=g) * 3).to(dt))
    assert view.data_ptr() % 16 == 0 and 2 * ROW * view.element_size() >= 1 << 32
    return view, view.contiguous()


def _stream_state(H=6):
    g = torch.Generator(device=DEV).manual_seed(1)
    return dict(hist=torch.randint(0, 2000, (3, H), device=DEV, generator=g), pos=torch.tensor([1, 3, 2], device=DEV),
                live=torch.ones(3, dtype=torch.int32, device=DEV), stop=torch.full((3,), -1, dtype=torch.int64, device=DEV),
                limit=torch.full((3,), H, dtype=torch.int64, device=DEV), tok=torch.zeros(3, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("V", [2056, 128256])
@pytest.mark.parametrize("dt", [F16, F32], ids=["fp16", "fp32"])
def test_logits_rows_past_2_to_the_32_bytes(dt, V):
    from quantizations_amd import layer_ops as lo

    _need(5 if dt == F16 else 9, "logits rows 2^30 + 8 elements apart")
    view, flat = _logit_rows(V, dt, seed=V)
    assert view.stride(0) == ROW and flat.stride(0) == V
    ran = []

    def same(a, b, what):
        for name in a:
            assert torch.equal(_bits(a[name]), _bits(b[name])), (what, name)
        ran.append(what)

    # the greedy pick (fp16 and fp32 kernels)
    a, b = _stream_state(), _stream_state()
    lo.greedy_step_streams(view, **a)
    lo.greedy_step_streams(flat, **b)
    same(a, b, "greedy_step_streams")
    assert a["tok"].tolist() == flat.argmax(-1).tolist()
    if dt == F16:       # the 16-bit kernels (fp32 logits take torch ops there)
        smp = dict(temperature=torch.tensor([1.0, 0.7, 1.3], device=DEV), top_k=torch.tensor([50, 0, 7], dtype=torch.int32, device=DEV),
                   top_p=torch.tensor([0.9, 1.0, 0.5], device=DEV),
                   uniform=torch.rand((3, 6), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2)))
        a, b = _stream_state(), _stream_state()
        lo.sample_step_streams(view, **a, **smp)
        lo.sample_step_streams(flat, **b, **smp)
        same(a, b, "sample_step_streams")
        for top in (0, 5):
            ids = torch.tensor([0, V - 1, V // 2], device=DEV)
            assert lo.token_logprobs_supported(view)
            ra, rb = lo.token_logprobs(view, ids, top), lo.token_logprobs(flat, ids, top)
            same(dict(zip("abc", ra)), dict(zip("abc", rb)), f"token_logprobs top={top}")
        # process_logits, in place: last, it changes the rows
        st = _stream_state()
        st["hist"] = st["hist"] % V
        pen = dict(repetition_penalty=torch.tensor([1.3, 1.0, 2.0], device=DEV), presence_penalty=torch.tensor([0.5, 0.0, 0.1], device=DEV),
                   frequency_penalty=torch.tensor([0.2, 0.0, 0.3], device=DEV),
                   no_repeat_ngram=torch.tensor([1, 0, 2], dtype=torch.int32, device=DEV))
        assert lo.process_logits_supported(view)
        before = flat.clone()
        lo.process_logits(view, st["hist"], st["pos"], **pen)
        lo.process_logits(flat, st["hist"], st["pos"], **pen)
        same(dict(rows=view), dict(rows=flat), "process_logits")
        assert not torch.equal(_bits(flat), _bits(before)), "the processors changed something"
    torch.cuda.synchronize()
    print(f"logits rows {ROW} elements apart, {dt} V={V}: bit-equal to the contiguous rows: " + ", ".join(ran))
    del view, flat
    torch.cuda.empty_cache()
