"""GPU: the kernels around the 4-bit projections on activations beyond randn -- the families of
tests/activation_families.py (tests/test_activation_families.py shows on the CPU alone that each
reaches its edge and that fp32 arithmetic stays inside half of every bar used here).

* silu_mul: every 16-bit gate (and the fp32 neighbourhoods of -88, -20, 0, 88) against the float64
  value rounded as torch rounds; bit-exact except within 4 fp32 ulps of a rounding boundary; NaN /
  inf / zero / exp-overflow gates carry torch's bits; vector and scalar kernel agree.
* rope_qk and the cache row of both attention launches: every 16-bit value against exact and
  ordinary cos / sin rows, bit-exact against apply_rotary_pos_emb.
* rms_norm / add_rms_norm on every kernel route (held and sliced, held, loop, scalar, the fp32 limit)
  with outliers, subnormals, squares that under- and overflow, sums that overflow or tie, inf / NaN.
* The fused twins (RMSNorm prologue, SiLU epilogue, residual epilogue) keep their bit-identity.
* decode_attention / decode_attention_streams: `census` counts the keys (one key missed, doubled or
  wrongly admitted moves an element by 1 / n), the other families reach the softmax's edges.
* gemv_dense and the 4-bit GEMVs on outlier / subnormal / cancelling operands: whether gfx950's
  v_dot2_f32_f16 / v_dot2_f32_bf16 keep 16-bit subnormal operands is decided by the `sub16` cases.

No number here comes from the kernels: every bar is an existing one of the suite or follows from
the formats' ulps.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import activation_families as af
import test_activation_families as taf
import weight_families as wf

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
IDS = {F16: "fp16", BF16: "bf16", F32: "fp32"}
SHAPES = taf.SHAPES
ATTN_L = [128, 130, 384, 640]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _same_by_position(a, b):
    """Bit-identical, NaN compared by position (its payload and sign are free)."""
    nan = torch.isnan(a)
    return torch.equal(nan, torch.isnan(b)) and torch.equal(_bits(a)[~nan], _bits(b)[~nan])


def _offset(t):
    """A contiguous copy of t that starts one element past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


# ---------------------------------------------------------------------------
# silu_mul
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("uval", [1.0, -3.0, 2.0 ** -14, 6e4])
@pytest.mark.parametrize("dt", [F16, BF16, F32], ids=IDS.get)
def test_silu_mul_every_gate(dt, uval):
    from quantizations_amd.layer_ops import silu_mul

    g = af.all16(IDS[dt]) if dt != F32 else taf.silu_gates32()
    g = torch.cat([g, torch.zeros(-g.numel() % 8, dtype=dt)])
    if dt == F32:
        g[-2:] = torch.tensor([float("inf"), float("nan")])
    u = torch.full_like(g, uval)
    gd, ud = g.to(DEV), u.to(DEV)
    yv = silu_mul(gd, ud)                        # 16-byte aligned: the vector kernel
    ys = silu_mul(_offset(gd), _offset(ud))      # the per-element kernel
    yt = F.silu(gd) * ud
    assert _same_by_position(yv, ys) and torch.equal(_bits(yv), _bits(ys))
    by_value = taf.silu_by_value(g)
    ok, frac = taf.silu_check(g[by_value], u[by_value], yv.cpu()[by_value])
    print(f"silu {IDS[dt]} u={uval}: {frac:.5f} of {int(by_value.sum())} gates took a neighbour of silu(g)")
    assert bool(ok.all()), (g[by_value][~ok][:8], yv.cpu()[by_value][~ok][:8])
    if dt != F32:       # an fp32 store keeps expf's own last place: 4 of the 21 gates differ in numpy's float32 too
        assert frac <= 0.01
    rest = ~by_value                             # NaN, +-inf and the gates whose exp(-x) overflows fp32
    assert int(rest.sum()) >= 2 and _same_by_position(yv.cpu()[rest], yt.cpu()[rest])
    zero = g == 0
    assert int(zero.sum()) >= 2 and torch.equal(_bits(yv.cpu()[zero]), _bits(yt.cpu()[zero]))   # the sign of zero


# ---------------------------------------------------------------------------
# rotary: rope_qk and the cache row both attention launches write
# ---------------------------------------------------------------------------


def _rope_rows(dt, n=8):
    """cos / sin [n, 64]: (1, 0), (0, 1), (-1, 0), (0, -1), then ordinary angles."""
    g = torch.Generator().manual_seed(1)
    ang = torch.rand(n, 32, generator=g) * 50
    cos, sin = torch.cat((ang.cos(), ang.cos()), -1), torch.cat((ang.sin(), ang.sin()), -1)
    for i, (c, s) in enumerate([(1, 0), (0, 1), (-1, 0), (0, -1)]):
        cos[i], sin[i] = c, s
    return cos.to(dt), sin.to(dt)


def _rope_values(dt):
    """(q, k) [1, 128, 8, 64]: every 16-bit pattern (as fp32 values for fp32) in two orders."""
    a = af.all16("bf16" if dt == BF16 else "fp16").to(dt)
    return a.view(1, 128, 8, 64), a.flip(0).roll(12345).view(1, 128, 8, 64)


@pytest.mark.parametrize("dt", [F16, BF16, F32], ids=IDS.get)
def test_rope_qk_every_value(dt):
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb

    from quantizations_amd.layer_ops import rope_qk

    fn = getattr(apply_rotary_pos_emb, "_qz_orig", apply_rotary_pos_emb)
    cos, sin = (t.view(1, 8, 64).to(DEV) for t in _rope_rows(dt))
    name = IDS[dt]
    cases = [_rope_values(dt),
             (af.sub16(name, (1, 16, 8, 64)), af.nonfinite(name, 8192)[3].view(1, 16, 8, 64)),
             (af.nonfinite(name, 8192)[:3].reshape(1, 48, 8, 64), af.sub16(name, (1, 48, 8, 64), seed=3))]
    for q, k in cases:
        q, k = q.to(DEV), k.to(DEV)
        qr, kr = fn(q, k, cos, sin)
        qo, ko = rope_qk(q, k, cos, sin)
        assert _same_by_position(qo, qr) and _same_by_position(ko, kr)


@pytest.mark.parametrize("streams", [False, True], ids=["masked", "streams"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=IDS.get)
def test_attention_cache_row_every_value(dt, streams):
    """512 sequences x 2 kv heads x 64: k runs over every 16-bit pattern, v over every pattern in
    another order; the row written is apply_rotary_pos_emb(k) by position and v's bits, the rest of
    the cache is untouched."""
    from quantizations_amd.layer_ops import decode_attention, decode_attention_streams

    B, Hq, Hkv, D, L = 512, 2, 2, 64, 128
    kv, vv = _rope_values(dt)
    k, v = kv.reshape(B, 1, Hkv * D).to(DEV), vv.reshape(B, 1, Hkv * D).to(DEV)
    q = torch.zeros(B, 1, Hq * D, dtype=dt, device=DEV)
    cos8, sin8 = _rope_rows(dt)
    idx = torch.arange(B) % 8
    cos, sin = cos8[idx].view(B, 1, D).to(DEV), sin8[idx].view(B, 1, D).to(DEV)
    kc = torch.zeros(B, Hkv, L, D, dtype=dt, device=DEV)
    vc = torch.zeros_like(kc)
    ps = [(37 * b) % L for b in range(B)] if streams else [77] * B
    if streams:
        decode_attention_streams(q, k, v, cos, sin, kc, vc, torch.tensor(ps, device=DEV), Hq, 0.125)
    else:
        mask = (torch.arange(L, device=DEV) <= 77).view(1, 1, 1, L)
        pos = torch.tensor(77, dtype=torch.int64, device=DEV)
        decode_attention(q, k, v, cos, sin, kc, vc, mask, pos, torch.zeros(1, dtype=torch.int32, device=DEV), Hq, 0.125)
        assert int(pos) == 78
    kh = k.view(B, Hkv, D)
    kr = (kh * cos) + (af._rotate_half(kh) * sin)
    rows = torch.arange(B, device=DEV)
    pt = torch.tensor(ps, device=DEV)
    assert _same_by_position(kc[rows, :, pt], kr)
    assert torch.equal(_bits(vc[rows, :, pt]), _bits(v.view(B, Hkv, D)))
    kc[rows, :, pt] = 0
    vc[rows, :, pt] = 0
    assert not bool(_bits(kc).any()) and not bool(_bits(vc).any())


# ---------------------------------------------------------------------------
# rms_norm / add_rms_norm on every route
# ---------------------------------------------------------------------------

NORM_ROUTES = {          # name -> (K, rows, aligned, dtypes)
    "held-sliced": (4096, 1, True, (F16, BF16, F32)),
    "held": (4096, 80, True, (F16, BF16, F32)),
    "loop": (16392, 2, True, (F16, BF16, F32)),
    "scalar": (1000, 2, False, (F16, BF16, F32)),
    "fp32-held-limit": (8192, 2, True, (F32,)),
    "fp32-past-limit": (8200, 2, True, (F32,)),
}
NORM_CASES = [(r, dt) for r, (_, _, _, dts) in NORM_ROUTES.items() for dt in dts]


def _rows(x, rows):
    """x's rows tiled to `rows` rows -- or, for the one-row route, each row on its own."""
    if rows == 1:
        return [x[i:i + 1] for i in range(x.shape[0])]
    return [x[torch.arange(rows) % x.shape[0]]]


def _llama_norm(x, w, eps):
    """LlamaRMSNorm.forward, torch's own ops on the GPU."""
    h = x.to(torch.float32)
    var = h.pow(2).mean(-1, keepdim=True)
    h = h * torch.rsqrt(var + eps)
    return w * h.to(x.dtype)


def _assert_norm(y, x_cpu, w_cpu, ref_gpu, what, dt, r_cpu=None):
    ulps = 4 if dt == F32 else 2
    ref64 = af.rms_norm64(x_cpu, w_cpu, 1e-5, r_cpu)
    ref64 = ref64[1] if r_cpu is not None else ref64
    for ref, who in ((ref64, "float64 restatement"), (ref_gpu.cpu(), "torch on the GPU")):
        assert taf.same_specials(y.cpu(), ref), (what, who, "positions of inf / NaN / zero")
        fin = torch.isfinite(ref)
        d = (y.cpu().double() - ref.double()).abs()[fin] / af.ulp_at(ref, dt)[fin]
        assert bool((d <= ulps).all()), (what, who, float(d.max()))


@pytest.mark.parametrize("route,dt", NORM_CASES, ids=lambda v: IDS.get(v, v))
def test_rms_norm_families_on_every_route(route, dt):
    from quantizations_amd.layer_ops import add_rms_norm, rms_norm

    K, rows, aligned, _ = NORM_ROUTES[route]
    name = IDS[dt]
    place = (lambda t: t.to(DEV)) if aligned else (lambda t: _offset(t.to(DEV)))
    for wname, w in taf.norm_weights(name, K).items():
        wd = w.to(DEV)
        for fam, xs in taf.norm_inputs(name, K).items():
            for x in _rows(xs, rows):
                xd = place(x)
                _assert_norm(rms_norm(xd, wd, 1e-5), x, w, _llama_norm(xd, wd, 1e-5), f"{route} {name} {fam} w={wname}", dt)
        for x, r in (zip(*(_rows(t, rows) for t in af.overflow_add(name, K))) if dt != F32 else ()):
            xd, rd = place(x), place(r)
            s, y = add_rms_norm(xd, rd, wd, 1e-5)
            s_ref = rd + xd
            assert torch.equal(_bits(s), _bits(s_ref)) and torch.equal(_bits(s.cpu()), _bits((r.float() + x.float()).to(dt)))
            _assert_norm(y, x, w, _llama_norm(s_ref, wd, 1e-5), f"{route} {name} overflow_add w={wname}", dt, r)
        x = _rows(af.outlier(name, (2, K)), rows)[0]      # the add form on a finite family too
        r = _rows(af.sub16(name, (2, K)), rows)[0]
        s, y = add_rms_norm(place(x), place(r), wd, 1e-5)
        assert torch.equal(_bits(s.cpu()), _bits((r.float() + x.float()).to(dt)))
        _assert_norm(y, x, w, _llama_norm(s, wd, 1e-5), f"{route} {name} outlier + sub16 w={wname}", dt, r)


@pytest.mark.parametrize("K", [4096, 16384, 16392])
@pytest.mark.parametrize("dt", [F16, BF16, F32], ids=IDS.get)
def test_rms_norm_kernels_agree_bitwise_on_exactly_summable_rows(dt, K):
    """Rows of +-{0.5, 1, 2, 4} with one 64: every square is a multiple of 0.25 and the row's sum stays
    below 2^24 * 0.25, so the fp32 sum of squares is exact in any order and the vector kernels (held
    up to 16384 elements, the loop past it; aligned) and the per-element kernel (an offset view) must
    store the same bits."""
    from quantizations_amd.layer_ops import add_rms_norm, rms_norm

    if dt == F32 and K == 16384:
        K = 8192      # the held kernel's fp32 limit
    g = torch.Generator().manual_seed(K)
    x = (2.0 ** torch.randint(-1, 3, (3, K), generator=g).double() * (torch.randint(0, 2, (3, K), generator=g) * 2 - 1)).to(dt)
    x[:, 5] = 64.0
    r = (2.0 ** torch.randint(-1, 3, (3, K), generator=g).double()).to(dt)
    w = (1 + 0.1 * torch.randn(K, generator=g)).to(dt)
    xd, rd, wd = x.to(DEV), r.to(DEV), w.to(DEV)
    a, b = rms_norm(xd, wd, 1e-5), rms_norm(_offset(xd), _offset(wd), 1e-5)
    assert torch.equal(_bits(a), _bits(b))
    (sa, ya), (sb, yb) = add_rms_norm(xd, rd, wd, 1e-5), add_rms_norm(_offset(xd), _offset(rd), _offset(wd), 1e-5)
    assert torch.equal(_bits(sa), _bits(sb)) and torch.equal(_bits(ya), _bits(yb))


# ---------------------------------------------------------------------------
# the fused twins keep their bit-identity
# ---------------------------------------------------------------------------

_cache = {}


def _quantised(family, qt, shape):
    """(oracle state, packed, QuantState on the GPU) of a weight family, double quant."""
    import oracle
    from test_gpu_weight_range import _gpu_state

    key = (family, qt, shape)
    if key not in _cache:
        W = taf.gemv_weight(family, shape)
        _cache[key] = (W, oracle.quantize_4bit(W.float().numpy(), 64, qt, double_quant=True))
    W, o = _cache[key]
    return (W, o) + tuple(_gpu_state(o))


_gemv_inputs = taf.gemv_inputs


@pytest.mark.parametrize("K", [2048, 4096])
@pytest.mark.parametrize("dt", [F16, BF16], ids=IDS.get)
def test_grouped_rmsnorm_prologue_bit_identity(orc, dt, K):
    from quantizations_amd.core import gemv_4bit_grouped
    from quantizations_amd.layer_ops import rms_norm

    items = [_quantised(f, "nf4", (M, K))[2:] + (None,) for f, M in (("randn", 512), ("outlier", 128), ("tiny", 128))]
    name = IDS[dt]
    nw = (1 + 0.1 * torch.randn(K, generator=torch.Generator().manual_seed(K))).to(dt).to(DEV)
    for fam, x in _gemv_inputs(name, K).items():
        x = x.to(DEV).reshape(1, K)
        got = gemv_4bit_grouped(x, items, norm=(nw, 1e-5))
        want = gemv_4bit_grouped(rms_norm(x, nw, 1e-5), items)
        for a, b in zip(got, want):
            assert torch.equal(_bits(a), _bits(b)) and bool(torch.isfinite(a).all()), fam


@pytest.mark.parametrize("dt", [F16, BF16], ids=IDS.get)
def test_pair_silu_epilogue_bit_identity_over_the_gate_range(orc, dt):
    """gate = outlier weights x an activation with two +-6e4 elements: it spans the format, overflows
    to +-inf in some rows (fp16) and puts silu(gate) into the subnormal range in others."""
    from quantizations_amd.core import gemv_4bit_grouped, gemv_4bit_pair_silu
    from quantizations_amd.layer_ops import silu_mul

    M, K = 512, 2048
    items = [_quantised(f, "nf4", (M, K))[2:] + (None,) for f in ("outlier", "tiny")]
    g = torch.Generator().manual_seed(7)
    x = torch.randn(K, generator=g) * 8
    Wd = torch.from_numpy(orc.dequantize(_quantised("outlier", "nf4", (M, K))[1])).abs()
    big = Wd.amax(0).topk(2).indices                 # the columns of the largest weights
    x[big] = torch.tensor([6e4, -6e4])
    x = x.to(dt).to(DEV).reshape(1, K)
    h = gemv_4bit_pair_silu(x, items)
    assert h is not None
    gate, up = gemv_4bit_grouped(x, items)
    assert torch.equal(_bits(h), _bits(silu_mul(gate, up)))
    a = F.silu(gate)
    tiny = torch.finfo(dt).tiny
    assert float(gate.float().abs().max()) > 6e4
    if dt == F16:                     # (bf16's subnormals lie below the gates whose exp(-x) overflows fp32)
        assert int(((a != 0) & (a.abs() < tiny)).sum()) >= 1
        assert int((gate == float("inf")).sum()) >= 1 and int((gate == float("-inf")).sum()) >= 1
    ref = a * up
    assert torch.equal(torch.isnan(h), torch.isnan(ref))
    fin = torch.isfinite(ref)
    d = (h.double() - ref.double()).abs()
    assert bool((d[fin] <= 2 * af.ulp_at(ref, dt)[fin]).all())           # test_silu_mul_vs_torch's bar
    assert torch.equal(h[~fin & ~torch.isnan(ref)], ref[~fin & ~torch.isnan(ref)])


@pytest.mark.parametrize("M,K", [(300, 1000), (1024, 4096)])
@pytest.mark.parametrize("dt", [F16, BF16], ids=IDS.get)
def test_residual_epilogue_bit_identity_with_overflowing_sums(dt, M, K):
    from quantizations_amd.core import gemv_4bit, quantize_4bit

    g = torch.Generator().manual_seed(M)
    W = (torch.randn(M, K, generator=g) * 0.5).to(dt)
    packed, st = quantize_4bit(W.to(DEV), quant_type="nf4")
    x = torch.randn(1, K, generator=g).to(dt).to(DEV)
    for row in (0, 1):
        r = af.overflow_add(IDS[dt], M + 2)[0][row][:M].clone()                   # +-max, even integers, N(0, 9)
        r[20::50] = torch.finfo(dt).max
        r[21::50] = -torch.finfo(dt).max
        r = r.to(DEV)
        got = gemv_4bit(x, packed, state=st, residual=r)
        y = gemv_4bit(x, packed, state=st)
        want = r + y.view(-1)
        assert torch.equal(_bits(got.view(-1)), _bits(want))
        if dt == F16 and row == 1:        # max + y overflows once |y| reaches half a spacing (16)
            assert int(torch.isinf(want).sum()) >= 1


# ---------------------------------------------------------------------------
# decode attention
# ---------------------------------------------------------------------------


def _dev(case):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in case.items()}


def _streams(case):
    """(out [B, Hq D], kc, vc after the call) of one decode_attention_streams launch."""
    from quantizations_amd.layer_ops import decode_attention_streams

    c = _dev(case)
    kc, vc = c["kc"].clone(), c["vc"].clone()
    pos = torch.tensor(c["pos"], dtype=torch.int64, device=DEV)
    out = decode_attention_streams(c["q"], c["k"], c["v"], c["cos"], c["sin"], kc, vc, pos, c["Hq"], c["scale"])
    torch.cuda.synchronize()
    assert pos.tolist() == c["pos"]
    return out.view(len(c["pos"]), -1), kc, vc


def _masked(case):
    """The same from one decode_attention launch per stream (mask = the case's visibility)."""
    from quantizations_amd.layer_ops import decode_attention

    c = _dev(case)
    outs, kcs, vcs = [], [], []
    for b, p in enumerate(c["pos"]):
        kb, vb = c["kc"][b:b + 1].clone(), c["vc"][b:b + 1].clone()
        pos = torch.tensor(p, dtype=torch.int64, device=DEV)
        arrive = torch.zeros(1, dtype=torch.int32, device=DEV)
        mask = c["visible"][b].view(1, 1, 1, -1).contiguous()
        outs.append(decode_attention(c["q"][b:b + 1], c["k"][b:b + 1], c["v"][b:b + 1], c["cos"][b:b + 1],
                                     c["sin"][b:b + 1], kb, vb, mask, pos, arrive, c["Hq"], c["scale"]))
        assert int(pos) == p + 1 and int(arrive) == 0
        kcs.append(kb), vcs.append(vb)
    return torch.cat(outs).view(len(c["pos"]), -1), torch.cat(kcs), torch.cat(vcs)


def _assert_caches(case, kc, vc):
    kc_ref, vc_ref = af.updated_caches(case)
    assert _same_by_position(kc.cpu(), kc_ref) and _same_by_position(vc.cpu(), vc_ref), "cache rows"
    for b, p in enumerate(case["pos"]):
        assert torch.equal(_bits(kc[b, :, p].cpu()), _bits(kc_ref[b, :, p])) and not bool(torch.isnan(kc[b, :, p]).any())


@pytest.mark.parametrize("dt", [F16, BF16], ids=IDS.get)
@pytest.mark.parametrize("L", ATTN_L)
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_attention_census_counts_the_keys(Hq, Hkv, D, L, dt):
    """q = 0 and one-hot v: output element d is (visible keys with j % D == d) / (visible keys), for
    every position around the chunk boundaries in ONE streams launch and, with 30 % holes, in one
    masked launch each; every cache row that is not visible holds NaN."""
    for holes, run in ((False, _streams), (False, _masked), (True, _masked)):
        case = taf.census_case(IDS[dt], Hq, Hkv, D, L, holes=holes)
        out, kc, vc = run(case)
        assert not bool(torch.isnan(out).any()), (holes, run.__name__)
        want = torch.from_numpy(case["expected"]).to(dt)
        d = (out.cpu().double() - want.double()).abs()
        bad = (d > af.ulp_at(want, dt)).nonzero()
        assert bad.shape[0] == 0, (holes, run.__name__, [(case["pos"][b], int(e) % D, float(out[b, e]), float(want[b, e]))
                                                         for b, e in bad[:6]])
        _assert_caches(case, kc, vc)


def _family_positions(L):
    return sorted({5, L // 2, L - 1} | ({129} if L > 129 else set()))


# a product of two bf16 subnormals is below fp32: sub16_q is the bf16 case of sub16
FAMILY_CASES = [(f, dt) for f in af.ATTENTION_FAMILIES if f != "census" for dt in (F16, BF16) if (f, dt) != ("sub16", BF16)]


@pytest.mark.parametrize("L", ATTN_L)
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
@pytest.mark.parametrize("family,dt", FAMILY_CASES, ids=lambda v: IDS.get(v, v))
def test_attention_families(family, dt, Hq, Hkv, D, L):
    holes = family == "dirty_mask"
    case = af.attention_case(family, IDS[dt], Hq, Hkv, D, L, _family_positions(L), holes=holes)
    ref, bound = af.attention_fp64(case)
    assert bound <= af.SCORE_BOUND
    vm = af.vmax(case)
    tol = taf.ATTN_TOL[IDS[dt]]
    out_m, kc, vc = _masked(case)
    _assert_caches(case, kc, vc)
    runs = [("masked", out_m)]
    if not holes:
        out_s, kc, vc = _streams(case)
        _assert_caches(case, kc, vc)
        assert torch.equal(_bits(out_s), _bits(out_m)), "streams launch vs the solo masked launches"
        runs.append(("streams", out_s))
    for who, out in runs:
        out = out.cpu()
        assert not bool(torch.isnan(out).any()), who
        torch.testing.assert_close(out.double() / vm, ref / vm, atol=tol, rtol=tol, msg=lambda m: f"{who}: {m}")
        if "dominant" in case:
            _, vc_ref = af.updated_caches(case)
            want = torch.stack([vc_ref[b, :, j] for b, j in enumerate(case["dominant"])]).repeat_interleave(case["G"], 1)
            want = want.reshape(out.shape)
            assert bool(((out.double() - want.double()).abs() <= af.ulp_at(want, dt)).all()), who


# ---------------------------------------------------------------------------
# gemv_dense (the lm_head)
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("K", [4096, 8192])
@pytest.mark.parametrize("dt", [F16, BF16], ids=IDS.get)
def test_gemv_dense_families(dt, K):
    from quantizations_amd.layer_ops import gemv_dense, gemv_dense_supported

    failures = []
    for what, x, W in taf.dense_cases(IDS[dt], 65, K):
        xd, Wd = x.to(DEV).view(1, 1, K), W.to(DEV)
        assert gemv_dense_supported(xd, Wd)
        y = gemv_dense(xd, Wd).view(-1).cpu()
        yl = F.linear(xd, Wd).view(-1).cpu()
        ref = W.double() @ x.double()
        mag = W.double().abs() @ x.double().abs()
        bar = taf.dense_bar(ref, mag, dt)
        d = (y.double() - ref).abs()
        dl = (yl.double() - ref).abs()
        fin = torch.isfinite(yl)
        ulp = torch.finfo(dt).eps
        vs_lib = ((y.float() - yl.float()).abs() / (2 * ulp * yl.float().abs().clamp_min(1e-3)))[fin]
        print(f"gemv_dense {IDS[dt]} K={K} {what}: worst err / bar {float((d / bar).max()):.3f} (F.linear "
              f"{float((dl / bar).max()):.3f}), worst |y - F.linear| / (2 ulp) {float(vs_lib.max()):.3f}")
        if not bool(torch.isfinite(y).all()) or not bool((d <= bar).all()):
            failures.append((what, "float64 bar", float((d / bar).max())))
        if not bool((vs_lib <= 1).all()):
            failures.append((what, "2 ulp of F.linear", float(vs_lib.max())))
    assert not failures, failures


# ---------------------------------------------------------------------------
# the 4-bit GEMVs with fp16 activations
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("K", [2048, 4096])
@pytest.mark.parametrize("qt", ["nf4", "fp4"])
@pytest.mark.parametrize("wfam", ["randn", "outlier"])
def test_gemv_4bit_fp16_activation_families(orc, wfam, qt, K):
    import quantizations_amd as qa
    from quantizations_amd.core import gemv_4bit, gemv_4bit_grouped

    M = 256
    W, o, packed, st = _quantised(wfam, qt, (M, K))
    m = qa.Linear4bit(K, M, bias=False, quant_type=qt, compute_dtype=F16)
    m.weight = qa.Params4bit(W, requires_grad=False, quant_type=qt, module=m)
    m = m.to(DEV)
    assert np.array_equal(m.weight.cpu().numpy().ravel(), o.packed)
    failures = []
    for fam, x in _gemv_inputs("fp16", K).items():
        ref = orc.gemv(x.float().numpy(), o)
        xd = x.to(DEV).reshape(1, K)
        outs = {"Linear4bit": m(xd.view(1, 1, K)).view(-1)}
        for exact in (False, True):
            outs[f"gemv exact={exact}"] = gemv_4bit(xd, packed, state=st, exact_codes=exact).view(-1)
            outs[f"grouped exact={exact}"] = gemv_4bit_grouped(xd, [(packed, st, None)], exact_codes=exact)[0].view(-1)
        # outlier weights x outlier activations leave fp16: such a row must be that inf; rows between
        # 6e4 and 7e4 may fall either side of the largest finite value
        fin, over = np.abs(ref) < 6e4, np.abs(ref) > 7e4
        assert fin.sum() >= M // 2
        for who, y in outs.items():
            y = y.double().cpu().numpy()
            assert np.array_equal(y[over], np.sign(ref[over]) * np.inf), (fam, who)
            err = np.abs(y - ref)[fin]
            bar = taf.gemv_bar(ref, "exact=True" in who)[fin]
            worst = float((err / bar).max())
            print(f"{wfam} {qt} K={K} {fam} {who}: worst err / bar {worst:.3f}")
            if not (np.isfinite(worst) and worst <= 1):
                failures.append((fam, who, worst))
    assert not failures, failures
