"""GPU: prefill attention of a window of T new tokens per stream against a static cache
(qz_prefill_attention, layer_ops.prefill_attention).

Shapes are in the kernel's own tile constants TQ / TK: L in {TK, TK + 2, 3 TK + 5}, T in {1, 2, TQ - 1,
TQ, TQ + 1, 2 TQ + 3}, window starts 0, TK - 1, TK, TK + 1, L - T and L - 2 (the last runs off the end)
dealt over B = 4 streams whose lengths are T, T - 1, 1 and 0, in two rotations so that every start
meets a window of T or T - 1 real rows.  Every cache row at or above pos[b]
holds NaN before the call, so one key too many shows.  Inputs come from prefill_reference.make_case
(seeded, CPU) so test_prefill_reference_cpu.py proves the bars on the same values."""
import math

import pytest
import torch
import activation_families as af
import prefill_reference as pr
from activation_families import ulp_at

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
TQ, TK = pr.TQ, pr.TK
LS = [TK, TK + 2, 3 * TK + 5]
TS = [1, 2, TQ - 1, TQ, TQ + 1, 2 * TQ + 3]
HEADS = [(4, 2), (8, 1)]
NAMES = ["fp16", "bf16"]
OPS = ("q", "k", "v", "cos", "sin", "kc", "vc")


def test_the_tile_constants_are_the_kernels():
    from quantizations_amd import layer_ops
    assert (layer_ops.PREFILL_TQ, layer_ops.PREFILL_TK) == (TQ, TK)


def _dev(case):
    d = {n: case[n].to(DEV) for n in OPS}
    d["pos"] = torch.tensor(case["pos"], dtype=torch.int64, device=DEV)
    d["len"] = torch.tensor(case["len"], dtype=torch.int64, device=DEV)
    return d


def _run(case, d=None):
    """(out, kc, vc) of one prefill_attention call on fresh device copies of the case."""
    from quantizations_amd.layer_ops import prefill_attention
    d = d or _dev(case)
    out = prefill_attention(d["q"], d["k"], d["v"], d["cos"], d["sin"], d["kc"], d["vc"], d["pos"], d["len"],
                            case["Hq"], case["scale"])
    torch.cuda.synchronize()
    assert d["pos"].tolist() == case["pos"] and d["len"].tolist() == case["len"], "pos and len are read only"
    return out, d["kc"], d["vc"]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    """Bit-identical, a NaN matching any NaN."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(_bits(a)[~na], _bits(b)[~nb])


def _rounds(L, T, B=4):
    """The six window starts dealt over B streams, twice, the second time two starts further on: with the
    lengths fixed per stream (T, T - 1, 1, 0) every start meets a window of T or T - 1 real rows."""
    s = pr.window_starts(L, T)
    out = []
    for rot in (0, 2):
        r = s[rot:] + s[:rot]
        r = r + r[:(-len(r)) % B]
        out += [r[i:i + B] for i in range(0, len(r), B)]
    return out


def _assert_fill(case, out):
    for b, row in enumerate(pr.expected_fill(case)):
        for i, what in enumerate(row):
            r = out[b, i]
            ok = {"ok": not torch.isnan(r).any(), "nan": torch.isnan(r).all(), "zero": (_bits(r) == 0).all()}[what]
            assert bool(ok), (case["pos"], case["len"], b, i, what)


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name", NAMES)
def test_caches_carry_the_bits_of_the_decode_launches(name, D, Hq, Hkv, L):
    """Stream by stream the caches equal decode_attention_verify (len >= 2) or decode_attention_streams
    (len = 1) run on that stream's real rows alone: slots pos .. pos + len - 1 written, NaN above, the
    old bits below."""
    from quantizations_amd.layer_ops import decode_attention_streams, decode_attention_verify
    for T in TS:
        for rnd, ps in enumerate(_rounds(L, T)):
            case = pr.make_case(4, T, Hq, Hkv, D, L, ps, pr.window_lengths(T), name, seed=L + D + Hq + 7 * T + rnd)
            d = _dev(case)
            kc0, vc0 = d["kc"].clone(), d["vc"].clone()
            out, kc, vc = _run(case, d)
            _assert_fill(case, out)
            for b, (p, n) in enumerate(zip(case["pos"], case["len"])):
                kr, vr = kc0[b:b + 1].clone(), vc0[b:b + 1].clone()
                if n >= 1:
                    a = [d[x][b:b + 1, :n] for x in ("q", "k", "v", "cos", "sin")]
                    fn = decode_attention_verify if n >= 2 else decode_attention_streams
                    fn(*a, kr, vr, d["pos"][b:b + 1], Hq, case["scale"])
                assert _same(kc[b:b + 1], kr) and _same(vc[b:b + 1], vr), (T, ps, b)
                w = pr.legal_rows(case, b)
                if 0 <= p < L:
                    assert not torch.isnan(kc[b, :, p:p + w]).any() and torch.isnan(kc[b, :, p + w:]).all()
                    assert torch.equal(_bits(kc[b, :, :p]), _bits(kc0[b, :, :p]))
                    assert torch.equal(_bits(vc[b, :, :p]), _bits(vc0[b, :, :p]))


@pytest.mark.parametrize("Hq,Hkv", HEADS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name", NAMES)
def test_a_window_equals_its_two_halves_bit_for_bit(name, D, Hq, Hkv):
    """Whole window == the same window as two calls split at rows 1, TQ - 1, TQ and ceil(T / 2), the
    second at pos + split: output bits and cache bits, NaN matching NaN."""
    L = 3 * TK + 5
    for T in TS[1:]:
        for rnd, ps in enumerate(_rounds(L, T)):
            case = pr.make_case(4, T, Hq, Hkv, D, L, ps, pr.window_lengths(T), name, seed=11 * T + D + rnd)
            out, kc, vc = _run(case)
            for split in pr.splits_of(T):
                first, second = pr.split_case(case, split)
                o1, kc1, vc1 = _run(first)
                d2 = _dev(second)
                d2["kc"], d2["vc"] = kc1, vc1
                o2, kc2, vc2 = _run(second, d2)
                assert _same(torch.cat((o1, o2), 1), out), (T, ps, split)
                assert _same(kc2, kc) and _same(vc2, vc), (T, ps, split)


@pytest.mark.parametrize("name,D,Hq,Hkv", [("fp16", 128, 8, 1), ("bf16", 64, 4, 2)])
def test_a_stream_alone_equals_the_stream_beside_others(name, D, Hq, Hkv):
    L, T = 3 * TK + 5, 2 * TQ + 3
    ps = [TK - 1, 0, TK + 1, 5]
    lens = [T, 3, TQ, 0]
    case = pr.make_case(4, T, Hq, Hkv, D, L, ps, lens, name, seed=5)
    out, kc, vc = _run(case)
    for b in range(3):
        for n in (lens[b], T if b else TQ + 1):          # its own length; another window width for stream 0
            solo = dict(case, B=1, T=n, pos=[ps[b]], len=[min(lens[b], n)])
            for x in OPS:
                solo[x] = case[x][b:b + 1, :n].contiguous() if x not in ("kc", "vc") else case[x][b:b + 1]
            o, kcs, vcs = _run(solo)
            m = min(lens[b], n)
            assert _same(o[0, :m], out[b, :m]), (b, n)
            if n >= lens[b]:
                assert _same(kcs[0], kc[b]) and _same(vcs[0], vc[b]), (b, n)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("D", [64, 128])
def test_census_counts_the_keys_each_window_row_sees(name, D):
    """q = 0 makes every visible key weigh the same (P is exactly 1, l an exact integer); v one-hot at
    j % D makes element d of row i the number of keys j <= pos + i with j % D == d over their number,
    to one ulp.  The starts put a key-tile edge and a query-tile edge inside every window."""
    from quantizations_amd.layer_ops import prefill_attention
    dtype = pr.DTYPES[name]
    Hq, Hkv, L, T = 4, 2, 3 * TK + 5, TQ + 5
    ps = [0, TK - 3, TK, L - T]
    B = len(ps)
    j = torch.arange(L)
    onehot = torch.zeros(L, D)
    onehot[j, j % D] = 1.0
    g = torch.Generator().manual_seed(D)
    vc = onehot.to(dtype).expand(B, Hkv, L, D).contiguous()
    kc = torch.randn(B, Hkv, L, D, generator=g).to(dtype)
    v = torch.empty(B, T, Hkv * D, dtype=dtype)
    for b, p in enumerate(ps):
        vc[b, :, p:] = float("nan")
        kc[b, :, p:] = float("nan")
        v[b] = onehot[p:p + T].to(dtype).repeat(1, Hkv)
    q = torch.zeros(B, T, Hq * D, dtype=dtype)
    k = torch.randn(B, T, Hkv * D, generator=g).to(dtype)
    cos, sin = torch.ones(B, T, D, dtype=dtype), torch.zeros(B, T, D, dtype=dtype)
    pos = torch.tensor(ps, dtype=torch.int64, device=DEV)
    length = torch.full((B,), T, dtype=torch.int64, device=DEV)
    out = prefill_attention(*(x.to(DEV) for x in (q, k, v, cos, sin, kc, vc)), pos, length, Hq, 1.0 / math.sqrt(D)).cpu()
    for b, p in enumerate(ps):
        for i in range(T):
            n = p + i + 1
            want = torch.bincount(j[:n] % D, minlength=D).double() / n
            err = (out[b, i].double().view(Hq, D) - want[None, :]).abs()
            assert bool((err <= ulp_at(want, dtype)[None, :]).all()), (b, i, p, float(err.max()))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("Hq,Hkv,D,L,T", pr.VALUE_CASES)
def test_values_against_an_fp64_restatement(name, Hq, Hkv, D, L, T):
    case = pr.value_case(name, Hq, Hkv, D, L, T)
    ref = pr.reference_fp64(case)
    kc_ref, vc_ref = pr.updated_caches(case)
    out, kc, vc = _run(case)
    _assert_fill(case, out)
    assert _same(kc.cpu(), kc_ref) and _same(vc.cpu(), vc_ref)
    tol = pr.TOL[name]
    err = (out.cpu().double() - ref).abs()
    print(name, D, L, T, "max err", float(err[~torch.isnan(ref)].max()))
    torch.testing.assert_close(out.cpu().double(), ref, atol=tol, rtol=tol, equal_nan=True)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("family,name", pr.FAMILY_CASES)
def test_activation_families(family, name, D):
    """A sink key far above the rest, v at +-6e4 and subnormal q / k / v, one token per stream (T = 1,
    len = 1), at the bars test_gpu_activation_range.py holds the decode launches to."""
    from quantizations_amd.layer_ops import prefill_attention
    case = pr.family_case(family, name, D)
    dtype = pr.DTYPES[name]
    ref, bound = af.attention_fp64(case)
    assert bound <= af.SCORE_BOUND
    vm = af.vmax(case)
    B = len(case["pos"])
    pos = torch.tensor(case["pos"], dtype=torch.int64, device=DEV)
    length = torch.ones(B, dtype=torch.int64, device=DEV)
    kc, vc = case["kc"].to(DEV), case["vc"].to(DEV)
    out = prefill_attention(*(case[x].to(DEV) for x in ("q", "k", "v", "cos", "sin")), kc, vc, pos, length,
                            case["Hq"], case["scale"]).cpu()[:, 0]
    kc_ref, vc_ref = af.updated_caches(case)
    assert _same(kc.cpu(), kc_ref) and _same(vc.cpu(), vc_ref)
    assert not bool(torch.isnan(out).any())
    tol = pr.TOL[name]
    print(family, name, D, float(((out.double() - ref) / vm).abs().max()))
    torch.testing.assert_close(out.double() / vm, ref / vm, atol=tol, rtol=tol)
    if "dominant" in case:
        want = torch.stack([vc_ref[b, :, j] for b, j in enumerate(case["dominant"])]).repeat_interleave(case["G"], 1)
        want = want.reshape(out.shape)
        assert bool(((out.double() - want.double()).abs() <= ulp_at(want, dtype)).all())


@pytest.mark.parametrize("bad", [-1, "L", "L+5"])
def test_a_bad_position_harms_its_own_stream_only(bad):
    L, T = 3 * TK + 5, TQ + 1
    good = [5, TK - 1, 0, L - T]
    case = pr.make_case(4, T, 4, 2, 64, L, good, [T, T - 1, T, 1], "fp16", seed=L)
    want, kc_w, vc_w = _run(case)
    broken = dict(case, pos=[good[0], good[1], {-1: -1, "L": L, "L+5": L + 5}[bad], good[3]])
    out, kc, vc = _run(broken)
    assert torch.isnan(out[2]).all()
    assert _same(kc[2].cpu(), case["kc"][2]) and _same(vc[2].cpu(), case["vc"][2])
    for b in (0, 1, 3):
        assert _same(out[b], want[b]) and not torch.isnan(out[b, :case["len"][b]]).any()
        assert _same(kc[b], kc_w[b]) and _same(vc[b], vc_w[b])


@pytest.mark.parametrize("name", NAMES)
def test_padding_rows_are_zero_whatever_they_hold(name):
    L, T = 3 * TK + 5, TQ + 1
    ps, lens = [0, TK - 1, TK, 7], [T - 1, 1, 0, TQ - 1]
    case = pr.make_case(4, T, 8, 1, 128, L, ps, lens, name, seed=2)
    want, kc_w, vc_w = _run(case)
    dirty = dict(case)
    junk = [float("nan"), float("inf"), float("-inf")]
    for x in ("q", "k", "v", "cos", "sin"):
        t = case[x].clone()
        for b, n in enumerate(lens):
            for i in range(n, T):
                t[b, i] = junk[(b + i) % 3]
        dirty[x] = t
    out, kc, vc = _run(dirty)
    for b, n in enumerate(lens):
        assert bool((_bits(out[b, n:]) == 0).all()) and bool((_bits(want[b, n:]) == 0).all()), b
    assert _same(out, want) and _same(kc, kc_w) and _same(vc, vc_w)


def test_one_captured_graph_follows_new_positions_and_lengths():
    from quantizations_amd.layer_ops import prefill_attention
    L, T, Hq = 3 * TK + 5, TQ + 1, 8
    first = ([3, TK, L - T, 0], [T, 5, T, 0])
    case = pr.make_case(4, T, Hq, 1, 128, L, first[0], first[1], "fp16", seed=9, nan_above=False)
    d = _dev(case)
    kc0, vc0 = d["kc"].clone(), d["vc"].clone()
    call = lambda: prefill_attention(d["q"], d["k"], d["v"], d["cos"], d["sin"], d["kc"], d["vc"], d["pos"],   # noqa: E731
                                     d["len"], Hq, case["scale"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    for ps, lens in (first, ([TK - 1, 0, 1, 100], [1, T, 0, TQ]), ([L - 2, 50, TK + 1, 9], [T, TQ - 1, 2, T])):
        d["kc"].copy_(kc0), d["vc"].copy_(vc0)
        d["pos"].copy_(torch.tensor(ps, device=DEV)), d["len"].copy_(torch.tensor(lens, device=DEV))
        g.replay()
        got, kc_g, vc_g = out.clone(), d["kc"].clone(), d["vc"].clone()
        d["kc"].copy_(kc0), d["vc"].copy_(vc0)
        eager = call()
        torch.cuda.synchronize()
        assert _same(got, eager)
        assert torch.equal(_bits(kc_g), _bits(d["kc"])) and torch.equal(_bits(vc_g), _bits(d["vc"]))
        assert not torch.equal(_bits(d["kc"]), _bits(kc0))


def test_rejects_what_it_cannot_take():
    from quantizations_amd.layer_ops import prefill_attention, prefill_attention_supported
    B, T, Hq, Hkv, D, L = 4, 4, 4, 2, 64, TK
    case = pr.make_case(B, T, Hq, Hkv, D, L, [1, 2, 3, 4], [T] * B, "fp16", seed=1, nan_above=False)
    d = _dev(case)
    q, k, v, cos, sin, kc, vc, pos, ln = (d[x] for x in OPS + ("pos", "len"))
    assert prefill_attention_supported(q, cos, kc, vc, pos, ln, Hq)
    wide = torch.zeros(B, Hkv, L, 2 * D, device=DEV, dtype=torch.float16)[..., :D]      # a strided cache
    kc96 = torch.zeros(B, Hkv, L, 96, device=DEV, dtype=torch.float16)
    for args in ((q, cos, kc, vc, pos.int(), ln, Hq), (q, cos, kc, vc, pos, ln.int(), Hq),       # wrong dtype
                 (q, cos, kc, vc, pos[:3], ln, Hq), (q, cos, kc, vc, pos, ln[:3], Hq),           # wrong length
                 (q, cos, kc, vc, pos.cpu(), ln, Hq), (q, cos, kc, vc, pos, ln.cpu(), Hq),       # wrong device
                 (q, cos, wide, wide, pos, ln, Hq),               # non-contiguous cache
                 (q, cos, kc96, kc96, pos, ln, Hq),               # D = 96
                 (q, cos, kc, vc, pos, ln, 32),                   # 16 query heads per kv head
                 (q.float(), cos, kc, vc, pos, ln, Hq)):
        assert not prefill_attention_supported(*args)
    kc0 = kc.clone()
    for bad in (dict(pos=pos.int()), dict(ln=ln[:3]), dict(pos=pos.cpu()), dict(kc=wide, vc=wide),
                dict(kc=kc96, vc=kc96), dict(Hq=32), dict(q=q.float()), dict(k=k[:, :2]), dict(sin=sin[:, :2])):
        a = dict(q=q, kc=kc, vc=vc, pos=pos, ln=ln, k=k, sin=sin, Hq=Hq)
        a.update(bad)
        with pytest.raises(ValueError):
            prefill_attention(a["q"], a["k"], v, cos, a["sin"], a["kc"], a["vc"], a["pos"], a["ln"], a["Hq"], 0.125)
    torch.cuda.synchronize()
    assert torch.equal(kc, kc0)   # nothing ran
