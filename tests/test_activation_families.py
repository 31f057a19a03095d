"""CPU only: (1) every family of tests/activation_families.py reaches the edge it is named for, with
a minimum count; (2) for every family a plain fp32 restatement of the operation (numpy float32, its
own summation order, np.exp in float32, roundings where the kernels round) stays within HALF of
the bar tests/test_gpu_activation_range.py asserts against the float64 reference -- so a bar that a
kernel misses is missed by the kernel, not by fp32 arithmetic."""
import numpy as np
import pytest
import torch

import activation_families as af
import weight_families as wf

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
f32 = np.float32
SHAPES = [(4, 2, 64), (8, 1, 128)]
CENSUS_PS = [0, 1, 31, 32, 63, 64, 126, 127, 128, 129, 255, 256, 383, 511, 512]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


# ---------------------------------------------------------------------------
# 1. each family reaches its edge
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_all16_is_every_bit_pattern(name):
    x = af.all16(name)
    assert x.dtype == af.DTYPES[name] and torch.unique(_bits(x)).numel() == 65536
    nan, inf = int(torch.isnan(x).sum()), int(torch.isinf(x).sum())
    assert inf == 2 and nan == 2 * af.SUB_MAX[name]          # the NaN payloads number the subnormals
    assert int((x == 0).sum()) == 2 and int(((x != 0) & (x.abs() < torch.finfo(x.dtype).tiny)).sum()) == 2 * af.SUB_MAX[name]


@pytest.mark.parametrize("name", ["fp16", "bf16", "fp32"])
def test_outlier_few_elements_carry_the_sum_of_squares(name):
    x = af.outlier(name, (3, 4096)).double()
    sq = x * x
    top = sq.sort(-1, descending=True).values[:, :8].sum(-1)
    assert bool((top >= 0.99 * sq.sum(-1)).all())
    assert bool(((x.abs() >= 3e4 * 0.99).sum(-1) == 4).all()) and float(x.abs().median()) < 2e-3


@pytest.mark.parametrize("name", ["fp16", "bf16", "fp32"])
def test_sub16_has_no_normal_value(name):
    x = af.sub16(name, (2, 4096))
    tiny = 2.0 ** -14 if name != "bf16" else 2.0 ** -126
    assert bool(((x != 0) & (x.double().abs() < tiny)).all())
    lo, hi = af.SUB_ULP[name], af.SUB_ULP[name] * af.SUB_MAX[name]
    for want in (lo, hi, -lo, -hi):
        assert int((x.double() == want).sum()) >= 1
    assert int((x > 0).sum()) > 1000 and int((x < 0).sum()) > 1000


@pytest.mark.parametrize("name", ["bf16", "fp32"])
def test_tiny32_squares_to_zero_and_huge32_to_inf(name):
    t, h = af.tiny32(name, 4096).float(), af.huge32(name, 4096).float()
    assert bool((t != 0).all()) and bool(((t * t) == 0).all())
    assert bool(torch.isfinite(h).all()) and bool(torch.isinf(h * h).all())
    assert int((h > 0).sum()) > 1000 and int((h < 0).sum()) > 1000


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_overflow_add_has_infs_and_exact_ties(name):
    x, r = af.overflow_add(name, 4096)
    s32 = x.float() + r.float()
    fin = torch.isfinite(s32)                      # bf16: max + max is beyond fp32 too (2 elements)
    assert int((~fin).sum()) == (0 if name == "fp16" else 2)
    exact = s32.double() == x.double() + r.double()
    assert bool(exact[:, :19][fin[:, :19]].all()) and bool(exact[:, ::3].all())   # the planted sums are exact in fp32
    s = s32.to(x.dtype)
    assert bool(torch.isfinite(s[0]).all())
    assert int((s[1] == float("inf")).sum()) >= 3 and int((s[1] == float("-inf")).sum()) >= 2
    assert int((torch.isinf(s[1]) & fin[1]).sum()) >= 3                 # finite in fp32: the overflow is the store's
    mx = torch.finfo(x.dtype).max
    assert int((s[0].abs() == mx).sum()) == 2 and int((s[1].abs() == mx).sum()) == 1   # max + just below half a spacing
    for row in (0, 1):
        half, odd = wf.tie_kind(s32[row].numpy(), name)
        assert int((half & odd).sum()) >= 600 and int((half & ~odd).sum()) >= 600
        assert int((half & (s32[row].numpy() < 0)).sum()) >= 400


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_nonfinite_rows(name):
    x = af.nonfinite(name, 4096)
    assert [int(torch.isinf(x[i]).sum()) for i in range(4)] == [1, 1, 0, 2]
    assert [int(torch.isnan(x[i]).sum()) for i in range(4)] == [0, 0, 1, 1]


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_mixed_chunks(name):
    x = af.mixed(name, 4096).double().reshape(-1, 32)
    tiny = 2.0 ** -14 if name == "fp16" else 2.0 ** -126
    sub = (x != 0) & (x.abs() < tiny)
    kind = torch.arange(x.shape[0]) % 4
    assert bool((x[kind == 3] == 0).all()) and bool(sub[kind == 1].all()) and bool(sub[kind == 2][:, 1::2].all())
    assert bool((x[kind == 0][:, 0].abs() > 1e4).all()) and bool((x[kind == 2][:, 0].abs() > 1e4).all())
    assert bool((x[kind == 2][:, 0::2].abs().median(-1).values > 100 * tiny * (name == "bf16")).all())


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_cancel_result_far_below_the_sum_of_magnitudes(name):
    x, W = af.cancel(name, 65, 4096)
    ref = W.double() @ x.double()
    mag = W.double().abs() @ x.double().abs()
    assert bool((ref.abs() <= 1e-2 * mag).all()) and float(ref.abs().median()) <= 2e-3 * float(mag.median())
    assert bool((ref != 0).all())


def census_case(name, Hq, Hkv, D, L, holes=False):
    ps = [p for p in CENSUS_PS + [L - 1] if p < L]
    return af.attention_case("census", name, Hq, Hkv, D, L, sorted(set(ps)), holes=holes)


@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_census_counts_differ_across_every_chunk_boundary(Hq, Hkv, D):
    c = census_case("fp16", Hq, Hkv, D, 640)
    exp = torch.from_numpy(c["expected"]).to(F16)             # what the test compares against, rounded
    ps = c["pos"]
    for edge in (128, 256, 512):                              # 383 / 511 / 512 / 639 straddle 384 and 512 too
        a, b = ps.index(edge - 1), ps.index(edge)
        d = edge % D
        assert exp[a, d] != exp[b, d] and int(c["visible"][b].sum()) == int(c["visible"][a].sum()) + 1
    # one key more or fewer moves an element by about 1 / n: more than an ulp of every expected value
    for b, p in enumerate(ps):
        n = p + 1
        cnt = torch.from_numpy(c["expected"][b]) * n
        admitted = (cnt + (torch.arange(Hq * D) % D == (p + 1) % D).double()) / (n + 1)       # key p + 1 let in
        assert int((admitted.to(F16) != exp[b]).sum()) >= Hq
        if n > 1:
            missed = (cnt - (torch.arange(Hq * D) % D == p % D).double()) / (n - 1)           # key p left out
            assert int((missed.to(F16) != exp[b]).sum()) >= Hq
    assert bool(torch.isnan(c["kc"][0, :, 1:]).all()) and bool(torch.isnan(c["vc"][-1, :, ps[-1]]).all())


@pytest.mark.parametrize("name", ["fp16", "bf16"])
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_sink_combine_weights_are_zero_and_gap_weights_subnormal(name, Hq, Hkv, D):
    ps = [300, 383, 639]
    for fam in ("sink", "late_peak"):
        w = []
        c = af.attention_case(fam, name, Hq, Hkv, D, 640, ps)
        af.attention_fp32(c, w)
        nz = sum(1 for x in w if x == 0.0)
        assert nz >= 2 * len(ps) * Hq and sum(1 for x in w if x == 1.0) == len(ps) * Hq   # every other chunk weighs 0
    w = []
    c = af.attention_case("gap", name, Hq, Hkv, D, 640, ps)
    af.attention_fp32(c, w)
    assert sum(1 for x in w if 0.0 < x < 2.0 ** -126) >= 2 * len(ps) * Hq and all(x > 0 for x in w)


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_dirty_mask_holes_and_dirt(name):
    c = af.attention_case("dirty_mask", name, 4, 2, 64, 640, [129, 639], holes=True)
    vis = c["visible"]
    for b, p in enumerate(c["pos"]):
        frac = 1.0 - float(vis[b, :p].float().mean())
        assert 0.2 < frac < 0.4 and bool(vis[b, p]) and not bool(vis[b, p + 1:].any())
        hidden = ~vis[b]
        hidden[p] = True
        for t in (c["kc"], c["vc"]):
            assert not bool(torch.isfinite(t[b, :, hidden]).any()) and bool(torch.isfinite(t[b, :, ~hidden]).all())
            assert int(torch.isnan(t[b, 0, hidden, 0]).sum()) > 10 and int(torch.isinf(t[b, 0, hidden, 0]).sum()) > 20


# ---------------------------------------------------------------------------
# 2. the fp32 restatement alone stays inside half of each bar
# ---------------------------------------------------------------------------

ATTN_TOL = {"fp16": 2e-3, "bf16": 1e-2}


def _attn_cases(name, Hq, Hkv, D, L):
    ps = sorted({5, L // 2, L - 1} | ({129} if L > 129 else set()))
    for fam in af.ATTENTION_FAMILIES:
        if fam == "census" or (fam == "sub16" and name == "bf16"):
            continue
        yield af.attention_case(fam, name, Hq, Hkv, D, L, ps, holes=fam == "dirty_mask")


@pytest.mark.parametrize("name", ["fp16", "bf16"])
@pytest.mark.parametrize("L", [130, 640])
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_attention_fp32_restatement_within_half_the_bar(name, Hq, Hkv, D, L):
    for c in _attn_cases(name, Hq, Hkv, D, L):
        ref, bound = af.attention_fp64(c)
        assert bound <= af.SCORE_BOUND, (c["family"], bound)
        got = af.attention_fp32(c).double()
        vm = af.vmax(c)
        assert not bool(torch.isnan(got).any()) and not bool(torch.isnan(ref).any())
        tol = ATTN_TOL[name]
        d = ((got - ref) / vm).abs()
        assert bool((d <= 0.5 * (tol + tol * (ref / vm).abs())).all()), (c["family"], float(d.max()))
        if "dominant" in c:       # the output is the dominant key's v row: <= 1 ulp asserted, 0 here
            _, vc = af.updated_caches(c)
            B = len(c["pos"])
            want = torch.stack([vc[b, :, j] for b, j in enumerate(c["dominant"])]).repeat_interleave(c["G"], 1)
            assert torch.equal(_bits(af.attention_fp32(c)), _bits(want.reshape(B, -1)))


@pytest.mark.parametrize("name", ["fp16", "bf16"])
@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("L", [128, 130, 384, 640])
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_census_fp32_restatement_is_the_rounded_count(name, Hq, Hkv, D, L, holes):
    """Asserted on the GPU within 1 ulp of count / n rounded to the dtype; fp32 count / n rounded to the
    dtype is within half of that, i.e. equal, except where the fp32 quotient sits on a double-rounding
    case -- there it is the neighbour; none may be further."""
    c = census_case(name, Hq, Hkv, D, L, holes)
    want = torch.from_numpy(c["expected"]).to(af.DTYPES[name])
    got = af.attention_fp32(c)
    d = (got.double() - want.double()).abs()
    assert bool((d <= af.ulp_at(want, want.dtype)).all())
    assert float((d == 0).double().mean()) >= 0.999


def _silu_f32(g, u):
    dt = g.dtype
    x = g.float().numpy()
    with np.errstate(over="ignore", invalid="ignore"):
        a = (x / (f32(1) + np.exp(-x, dtype=f32))).astype(f32)
    a = torch.from_numpy(a).to(dt)
    return a, (a.float() * u.float()).to(dt)


def silu_check(g, u, y):
    """The bar of the GPU test on finite gates: y must carry the bits of round(a * u) for a = the float64
    silu rounded to fp32 and to the dtype -- or, only where the float64 value lies within 4 fp32 ulps
    of a rounding boundary of the dtype, for a's neighbour on either side.  Returns (every element
    allowed, fraction that took a neighbour)."""
    dt = g.dtype
    y64 = af.silu64(g)
    a = y64.float().to(dt)
    inf = torch.full_like(a, float("inf"))
    cands = [a, torch.nextafter(a, inf), torch.nextafter(a, -inf)]
    ys = [_bits((c.float() * u.float()).to(dt)) for c in cands]
    exact = _bits(y) == ys[0]
    near = af.near_boundary(y64, dt)
    ok = exact | (near & ((_bits(y) == ys[1]) | (_bits(y) == ys[2])))
    return ok, 1.0 - float(exact.double().mean())


SILU_EXP_OVERFLOW = -88.72283905206835     # below it exp(-x) is beyond fp32: torch's fp32 silu is x / inf = -0


def silu_by_value(g):
    """The gates compared against the float64 reference: finite, and exp(-x) finite in fp32.  The others
    (NaN, +-inf, and the finite gates below SILU_EXP_OVERFLOW, where the float64 value is a tiny
    negative number but every fp32 evaluation gives -0) must carry torch's bits instead."""
    return torch.isfinite(g) & (g.double() >= SILU_EXP_OVERFLOW)


def silu_gates32():
    """fp32: -2 .. +2 ulp around -88, -20, 0 and 88, and the zeros."""
    out = []
    for c in (-88.0, -20.0, 0.0, 88.0):
        v = np.full(5, c, f32)
        for k in range(-2, 3):
            for _ in range(abs(k)):
                v[k + 2] = np.nextafter(v[k + 2], f32(np.inf if k > 0 else -np.inf), dtype=f32)
        out.append(v)
    return torch.from_numpy(np.concatenate(out + [np.array([-0.0], f32)]))


@pytest.mark.parametrize("uval", [1.0, -3.0, 2.0 ** -14, 6e4])
@pytest.mark.parametrize("name", ["fp16", "bf16", "fp32"])
def test_silu_fp32_restatement_within_half_the_cap(name, uval):
    g = af.all16(name) if name != "fp32" else silu_gates32()
    rest = g[torch.isfinite(g) & ~silu_by_value(g)]
    assert (rest.numel() > 5000) == (name != "fp32")        # the neighbourhood of -88 stays above the overflow
    assert bool((_bits(_silu_f32(rest, torch.ones_like(rest))[0]) == _bits(torch.tensor(-0.0, dtype=g.dtype))).all())
    g = g[silu_by_value(g)]
    u = torch.full_like(g, uval)
    _, y = _silu_f32(g, u)
    ok, frac = silu_check(g, u, y)
    assert bool(ok.all()), g[~ok][:8]
    if name != "fp32":
        assert frac <= 0.005, frac                # the GPU test allows 1 %
    else:       # no storage rounding absorbs exp's last place: float32 arithmetic itself takes a neighbour on
        assert frac > 0.01                        # 4 of these 21 gates, so the cap is asserted for 16-bit stores only


def rms_f32(x, w, eps, r=None):
    dt = x.dtype
    s = (r.float() + x.float()).to(dt) if r is not None else x
    sf = s.float().numpy()
    with np.errstate(over="ignore", invalid="ignore"):
        var = (sf * sf).sum(-1, keepdims=True, dtype=f32) * f32(1.0 / sf.shape[-1])
        rs = (f32(1) / np.sqrt(var + f32(eps), dtype=f32)).astype(f32)
        h = torch.from_numpy((sf * rs).astype(f32)).to(dt)
        y = torch.from_numpy((w.float().numpy() * h.float().numpy()).astype(f32)).to(dt)
    return (s, y) if r is not None else y


def norm_weights(name, K):
    """Powers of two: weight * h is exact (up to the subnormal store), so a last-place difference of h
    stays one of y -- half of the 2 ulp the existing bar grants a general weight."""
    dt = af.DTYPES[name]
    e = torch.arange(K) % 7 - 3
    return {"2^-14": torch.full((K,), 2.0 ** -14, dtype=dt), "2^15": torch.full((K,), 2.0 ** 15, dtype=dt),
            "2^(-3..3)": (2.0 ** e.double()).to(dt)}


def norm_inputs(name, K):
    """family -> x [rows, K] for rms_norm."""
    out = {"outlier": af.outlier(name, (2, K)), "sub16": af.sub16(name, (2, K)), "nonfinite": af.nonfinite(name, K)}
    if name != "fp16":
        out["tiny32"], out["huge32"] = af.tiny32(name, (2, K)), af.huge32(name, (2, K))
    return out


def same_specials(a, b):
    """inf, NaN and exact zeros in the same places (infs and zeros with their signs)."""
    return (torch.equal(torch.isnan(a), torch.isnan(b))
            and torch.equal(torch.where(torch.isinf(a), a, torch.zeros_like(a)), torch.where(torch.isinf(b), b, torch.zeros_like(b)))
            and torch.equal(a == 0, b == 0))


def within_ulps(y, ref, ulps):
    fin = torch.isfinite(ref)
    d = (y.double() - ref.double()).abs()
    return bool((d[fin] <= ulps * af.ulp_at(ref, ref.dtype)[fin]).all())


@pytest.mark.parametrize("K", [1000, 4096, 16392])
@pytest.mark.parametrize("name", ["fp16", "bf16", "fp32"])
def test_rms_norm_fp32_restatement_within_half_the_bar(name, K):
    half = 2 if name == "fp32" else 1
    for wname, w in norm_weights(name, K).items():
        for fam, x in norm_inputs(name, K).items():
            ref, got = af.rms_norm64(x, w, 1e-5), rms_f32(x, w, 1e-5)
            assert same_specials(got, ref), (fam, wname)
            assert within_ulps(got, ref, half), (fam, wname)
        if name != "fp32":
            x, r = af.overflow_add(name, K)
            (s_ref, ref), (s, got) = af.rms_norm64(x, w, 1e-5, r), rms_f32(x, w, 1e-5, r)
            assert torch.equal(_bits(s), _bits(s_ref)) and int(torch.isinf(s).sum()) >= 5
            assert same_specials(got, ref) and within_ulps(got, ref, half), wname


def dense_bar(ref, mag, dt):
    """eps * max(|ref|, tiny) + 2^-20 * sum_k |w_k x_k| (test_gpu_parity's form for fp32 partial sums)."""
    eps = {F16: 2.0 ** -10, BF16: 2.0 ** -7}[dt]
    tiny = {F16: 2.0 ** -14, BF16: 2.0 ** -126}[dt]
    return eps * ref.abs().clamp_min(tiny) + 2.0 ** -20 * mag


def dense_cases(name, M, K):
    """(what, x [K], W [M, K]) with finite products."""
    g = torch.Generator().manual_seed(K)
    dt = af.DTYPES[name]
    Wn = (torch.randn(M, K, generator=g) * 0.02).to(dt)
    xn = torch.randn(K, generator=g).to(dt)
    yield "outlier x", af.outlier(name, K), Wn
    yield "outlier W", xn, (af.outlier(name, (M, K)).double() * 1e-3).to(dt)
    yield "sub16 x", af.sub16(name, K), (Wn.double() * 50).to(dt)
    yield "sub16 W", xn, af.sub16(name, (M, K))
    if name == "fp16":        # a product of two bf16 subnormals is below fp32
        yield "sub16 both", af.sub16(name, K), af.sub16(name, (M, K), seed=9)
    yield ("cancel",) + af.cancel(name, M, K)
    if name == "bf16":
        yield "tiny32 x huge32 W", af.tiny32(name, K), (af.huge32(name, (M, K)).double() * 1e-2).to(dt)
        yield "huge32 x tiny32 W", (af.huge32(name, K).double() * 1e-2).to(dt), af.tiny32(name, (M, K))


@pytest.mark.parametrize("K", [4096, 8192])
@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_gemv_dense_fp32_restatement_within_half_the_bar(name, K):
    dt = af.DTYPES[name]
    for what, x, W in dense_cases(name, 65, K):
        ref = W.double() @ x.double()
        mag = W.double().abs() @ x.double().abs()
        assert bool(torch.isfinite(mag).all()) and bool((mag > 0).all()), what
        got = torch.from_numpy(W.float().numpy() @ x.float().numpy()).to(dt)
        assert bool(torch.isfinite(got).all()), what
        d = (got.double() - ref).abs()
        assert bool((d <= 0.5 * dense_bar(ref, mag, dt)).all()), (what, float((d / dense_bar(ref, mag, dt)).max()))
        # the other bar, 2 ulp of F.linear (another fp32 evaluation): a second fp32 order -- 64 interleaved
        # partial sums, as lanes keep them -- stays within half of it (1 ulp, with the existing 1e-3 floor)
        lanes = (W.float().numpy().reshape(65, -1, 64) * x.float().numpy().reshape(-1, 64)).sum(1, dtype=f32)
        other = torch.from_numpy(lanes.sum(-1, dtype=f32)).to(dt)
        lib_bar = torch.finfo(dt).eps * got.float().abs().clamp_min(1e-3)
        assert bool(((other.float() - got.float()).abs() <= lib_bar).all()), what


def gemv_bar(ref, exact):
    """test_gemv_exact_nf4_codes' bar (exact codes) or 1e-3 (the fp16-rounded table), both relative to
    the largest output that fp16 holds, plus one ulp of the fp16 output with its subnormal floor."""
    ref = np.abs(np.asarray(ref, np.float64))
    return 2.0 ** -10 * np.maximum(ref, 2.0 ** -14) + (1e-5 if exact else 1e-3) * ref[ref < 6e4].max()


def gemv_inputs(name, K):
    return {"outlier": af.outlier(name, K), "sub16": af.sub16(name, K), "mixed": af.mixed(name, K)}


def gemv_weight(family, shape):
    if family == "randn":
        return (torch.randn(shape, generator=torch.Generator().manual_seed(shape[0] + shape[1])) * 0.02).half()
    return wf.tiny(-14, shape=shape) if family == "tiny" else wf.outlier(shape=shape)


@pytest.mark.parametrize("K", [2048, 4096])
@pytest.mark.parametrize("qt", ["nf4", "fp4"])
@pytest.mark.parametrize("wfam", ["randn", "outlier"])
def test_gemv_4bit_fp32_restatement_within_half_the_exact_bar(orc, wfam, qt, K):
    """fp32 products of the oracle's dequantised weight summed in float32, rounded once to fp16."""
    o = orc.quantize_4bit(gemv_weight(wfam, (256, K)).float().numpy(), 64, qt, double_quant=True)
    W32 = orc.dequantize(o).astype(f32)
    for fam, x in gemv_inputs("fp16", K).items():
        ref = orc.gemv(x.float().numpy(), o)
        fin = np.abs(ref) < 6e4
        got = torch.from_numpy(W32 @ x.float().numpy()).half().double().numpy()
        assert fin.sum() >= 128 and np.all(np.abs(got - ref)[fin] <= 0.5 * gemv_bar(ref, True)[fin]), fam
