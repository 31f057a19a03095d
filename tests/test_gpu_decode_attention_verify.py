"""GPU: decode attention for a window of T new tokens per stream, causal among themselves
(qz_decode_attention_verify, layer_ops.decode_attention_verify).

The contract needs no tolerance: outputs and whole caches are bit-identical to T successive
decode_attention_streams calls on each stream alone at positions p_b, p_b + 1, ...  Every cache row at
or above p_b holds NaN before the call, so a key too many shows.  L covers one chunk (128), a ragged
second chunk (130) and both sides of kAttnSpecL = 512 (384, 640); every (B, T) is run over all the
window starts 0, 125, 126, 127, 128, L - T, L - 2 and L - 1, dealt over its streams round by round:
125..127 put the chunk boundary inside the window, L - 2 and L - 1 run off the end (the rows past L
are NaN and write nothing, the rows before them are intact -- in the sequential calls too).
A census (q = 0, one-hot v: tests/activation_families.py's family) counts the keys each window row
sees, which randn hides; an fp64 restatement holds the values at the bars of
test_gpu_decode_attention.py (2e-3 fp16, 1e-2 bf16)."""
import math

import pytest
import torch
from activation_families import ulp_at

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
SHAPES_BT = [(1, 2), (1, 4), (1, 8), (2, 4), (3, 4), (4, 4)]


def _starts(L, T):
    return [0, 125, 126, 127, 128, L - T, L - 2, L - 1]


def _rounds(L, B, T):
    """The eight window starts dealt over B streams: ceil(8 / B) lists of B starts."""
    s = _starts(L, T)
    s = s + s[:(-len(s)) % B]
    return [s[i:i + B] for i in range(0, len(s), B)]


def _case(B, T, Hq, Hkv, D, L, ps, dtype, seed, nan_above=True):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randn(B, T, Hq * D, device=DEV, generator=g).to(dtype)
    k = torch.randn(B, T, Hkv * D, device=DEV, generator=g).to(dtype)
    v = torch.randn(B, T, Hkv * D, device=DEV, generator=g).to(dtype)
    ang = torch.rand(B, T, D // 2, device=DEV, generator=g) * 6.0      # a rotary row per token row
    cos = torch.cat((ang.cos(), ang.cos()), -1).to(dtype)
    sin = torch.cat((ang.sin(), ang.sin()), -1).to(dtype)
    kc = torch.randn(B, Hkv, L, D, device=DEV, generator=g).to(dtype)
    vc = torch.randn(B, Hkv, L, D, device=DEV, generator=g).to(dtype)
    if nan_above:
        for b, p in enumerate(ps):
            if 0 <= p < L:
                kc[b, :, p:] = float("nan")
                vc[b, :, p:] = float("nan")
    pos = torch.tensor(ps, dtype=torch.int64, device=DEV)
    return q, k, v, cos, sin, kc, vc, pos


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    """Bit-identical, a NaN matching any NaN."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(_bits(a)[~na], _bits(b)[~nb])


def _sequential(q, k, v, cos, sin, kc, vc, ps, Hq, scale):
    """T successive decode_attention_streams calls on each stream alone; (out [B, T, Hq*D], caches)."""
    from quantizations_amd.layer_ops import decode_attention_streams

    B, T = q.shape[:2]
    kc, vc = kc.clone(), vc.clone()
    out = torch.empty_like(q)
    for b in range(B):
        for i in range(T):
            pos = torch.tensor([ps[b] + i], dtype=torch.int64, device=DEV)
            out[b, i] = decode_attention_streams(q[b:b + 1, i:i + 1], k[b:b + 1, i:i + 1], v[b:b + 1, i:i + 1],
                                                 cos[b:b + 1, i:i + 1], sin[b:b + 1, i:i + 1], kc[b:b + 1], vc[b:b + 1],
                                                 pos, Hq, scale)[0, 0]
    return out, kc, vc


@pytest.mark.parametrize("B,T", SHAPES_BT)
@pytest.mark.parametrize("L", [128, 130, 384, 640])
@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (8, 1)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_a_window_carries_the_bits_of_its_sequential_calls(dtype, D, Hq, Hkv, L, B, T):
    from quantizations_amd.layer_ops import decode_attention_verify

    scale = 1.0 / math.sqrt(D)
    for rnd, ps in enumerate(_rounds(L, B, T)):
        q, k, v, cos, sin, kc, vc, pos = _case(B, T, Hq, Hkv, D, L, ps, dtype, seed=L + D + Hq + 7 * T + rnd)
        ref, kc_ref, vc_ref = _sequential(q, k, v, cos, sin, kc, vc, ps, Hq, scale)
        out = decode_attention_verify(q, k, v, cos, sin, kc, vc, pos, Hq, scale)
        torch.cuda.synchronize()
        for b, p in enumerate(ps):
            for i in range(T):
                assert bool(torch.isnan(out[b, i]).all() if p + i >= L else not torch.isnan(out[b, i]).any()), (ps, b, i)
        assert _same(out, ref), (ps, torch.nonzero(_bits(out) != _bits(ref))[:8])
        assert _same(kc, kc_ref) and _same(vc, vc_ref), ps
        for b, p in enumerate(ps):      # the window's slots are written, the rows above stay NaN
            n = max(0, min(T, L - p))
            assert not torch.isnan(kc[b, :, p:p + n]).any() and torch.isnan(kc[b, :, p + n:]).all()
        assert pos.tolist() == ps, "pos is read only"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D,L,T", [(64, 130, 4), (128, 640, 8), (64, 384, 2)])
def test_census_counts_the_keys_each_window_row_sees(dtype, D, L, T):
    """q = 0 makes every visible key weigh the same; v one-hot at j % D makes element d of row i the
    number of keys j <= p_b + i with j % D == d over their number, to one ulp."""
    from quantizations_amd.layer_ops import decode_attention_verify

    Hq, Hkv = 4, 2
    ps = [0, 125, 126, L - T]
    B = len(ps)
    j = torch.arange(L, device=DEV)
    onehot = torch.zeros(L, D, device=DEV)
    onehot[j, j % D] = 1.0
    vc = onehot.to(dtype).expand(B, Hkv, L, D).contiguous()
    kc = torch.randn(B, Hkv, L, D, device=DEV).to(dtype)
    v = torch.empty(B, T, Hkv * D, device=DEV, dtype=dtype)
    for b, p in enumerate(ps):
        vc[b, :, p:] = float("nan")
        kc[b, :, p:] = float("nan")
        v[b] = onehot[p:p + T].to(dtype).repeat(1, Hkv)
    q = torch.zeros(B, T, Hq * D, device=DEV, dtype=dtype)
    k = torch.randn(B, T, Hkv * D, device=DEV).to(dtype)
    cos = torch.ones(B, T, D, device=DEV, dtype=dtype)
    sin = torch.zeros(B, T, D, device=DEV, dtype=dtype)
    pos = torch.tensor(ps, dtype=torch.int64, device=DEV)
    out = decode_attention_verify(q, k, v, cos, sin, kc, vc, pos, Hq, 1.0 / math.sqrt(D))
    torch.cuda.synchronize()
    for b, p in enumerate(ps):
        for i in range(T):
            n = p + i + 1
            want = torch.bincount(j[:n] % D, minlength=D).double() / n
            got = out[b, i].double().view(Hq, D)
            err = (got - want[None, :]).abs()
            print(b, i, float(err.max()))
            assert bool((err <= ulp_at(want, dtype)[None, :]).all()), (b, i, p)


def _rotate_half(x):
    x1, x2 = x[..., : x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("Hq,Hkv,D,L", [(4, 2, 64, 130), (8, 1, 128, 640)])
def test_values_against_an_fp64_restatement(dtype, Hq, Hkv, D, L):
    from quantizations_amd.layer_ops import decode_attention_verify

    B, T = 4, 4
    ps = [0, 125, 126, L - T]
    q, k, v, cos, sin, kc, vc, pos = _case(B, T, Hq, Hkv, D, L, ps, dtype, seed=3 * L + D)
    qh = q.view(B, T, Hq, D).transpose(1, 2)
    kh = k.view(B, T, Hkv, D).transpose(1, 2)
    c, s = cos.unsqueeze(1), sin.unsqueeze(1)
    qr = (qh * c) + (_rotate_half(qh) * s)            # apply_rotary_pos_emb, torch's own rounding
    kr = (kh * c) + (_rotate_half(kh) * s)
    kc2, vc2 = kc.clone(), vc.clone()
    for b, p in enumerate(ps):
        kc2[b, :, p:p + T] = kr[b]
        vc2[b, :, p:p + T] = v[b].view(T, Hkv, D).transpose(0, 1)
    rows = pos[:, None] + torch.arange(T, device=DEV)[None, :]                      # [B, T]
    visible = torch.arange(L, device=DEV)[None, None, :] <= rows[:, :, None]       # [B, T, L]
    anyrow = visible.any(1)                                                         # [B, L]: written or older
    G = Hq // Hkv
    kk = torch.where(anyrow[:, None, :, None], kc2, torch.zeros_like(kc2)).double().repeat_interleave(G, dim=1)
    vv = torch.where(anyrow[:, None, :, None], vc2, torch.zeros_like(vc2)).double().repeat_interleave(G, dim=1)
    sc = (qr.double() @ kk.transpose(-1, -2)) * (1.0 / math.sqrt(D))                # [B, Hq, T, L]
    sc = sc.masked_fill(~visible[:, None, :, :], float("-inf"))
    ref = (torch.softmax(sc, dim=-1) @ vv).transpose(1, 2).reshape(B, T, Hq * D)
    out = decode_attention_verify(q, k, v, cos, sin, kc, vc, pos, Hq, 1.0 / math.sqrt(D))
    torch.cuda.synchronize()
    assert _same(kc, kc2) and _same(vc, vc2)
    tol = 2e-3 if dtype == torch.float16 else 1e-2
    torch.testing.assert_close(out.double(), ref, atol=tol, rtol=tol)


@pytest.mark.parametrize("L", [128, 384])     # one chunk / three chunks (the combine launch)
@pytest.mark.parametrize("bad", [-1, "L", "L+5"])
def test_a_bad_position_harms_its_own_stream_only(L, bad):
    from quantizations_amd.layer_ops import decode_attention_verify

    B, T, Hq, Hkv, D, dtype = 4, 4, 4, 2, 64, torch.float16
    good = [5, 120, 0, L - T]
    q, k, v, cos, sin, kc, vc, pos = _case(B, T, Hq, Hkv, D, L, good, dtype, seed=L)
    scale = 1.0 / math.sqrt(D)
    kc0, vc0 = kc.clone(), vc.clone()
    want = decode_attention_verify(q, k, v, cos, sin, kc, vc, pos, Hq, scale)
    kc_w, vc_w = kc.clone(), vc.clone()
    kc.copy_(kc0), vc.copy_(vc0)
    pos[2] = {-1: -1, "L": L, "L+5": L + 5}[bad]
    out = decode_attention_verify(q, k, v, cos, sin, kc, vc, pos, Hq, scale)
    torch.cuda.synchronize()
    assert torch.isnan(out[2]).all()
    assert _same(kc[2], kc0[2]) and _same(vc[2], vc0[2])
    for b in (0, 1, 3):
        assert not torch.isnan(out[b]).any() and torch.equal(_bits(out[b]), _bits(want[b]))
        assert _same(kc[b], kc_w[b]) and _same(vc[b], vc_w[b])


def test_one_captured_graph_follows_new_positions():
    from quantizations_amd.layer_ops import decode_attention_verify

    B, T, Hq, Hkv, D, L, dtype = 4, 4, 8, 1, 128, 640, torch.float16
    first = [3, 200, 636, 126]
    q, k, v, cos, sin, kc, vc, pos = _case(B, T, Hq, Hkv, D, L, first, dtype, seed=9, nan_above=False)
    scale = 1.0 / math.sqrt(D)
    kc0, vc0 = kc.clone(), vc.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        decode_attention_verify(q, k, v, cos, sin, kc, vc, pos, Hq, scale)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = decode_attention_verify(q, k, v, cos, sin, kc, vc, pos, Hq, scale)
    for ps in (first, [636, 0, 127, 511], [130, 131, 132, 133]):
        kc.copy_(kc0), vc.copy_(vc0)
        pos.copy_(torch.tensor(ps, device=DEV))
        g.replay()
        got, kc_g, vc_g = out.clone(), kc.clone(), vc.clone()
        kc.copy_(kc0), vc.copy_(vc0)
        eager = decode_attention_verify(q, k, v, cos, sin, kc, vc, pos, Hq, scale)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(eager)) and not torch.isnan(got).any()
        assert torch.equal(_bits(kc_g), _bits(kc)) and torch.equal(_bits(vc_g), _bits(vc))
        assert not torch.equal(_bits(kc), _bits(kc0))


def test_rejects_what_it_cannot_take():
    from quantizations_amd.layer_ops import decode_attention_verify, decode_attention_verify_supported

    B, T, Hq, Hkv, D, L = 4, 4, 4, 2, 64, 128
    q, k, v, cos, sin, kc, vc, pos = _case(B, T, Hq, Hkv, D, L, [1, 2, 3, 4], torch.float16, seed=1, nan_above=False)
    assert decode_attention_verify_supported(q, cos, kc, vc, pos, Hq)
    wide = torch.zeros(B, Hkv, L, 2 * D, device=DEV, dtype=torch.float16)[..., :D]      # a strided cache
    kc96 = torch.zeros(B, Hkv, L, 96, device=DEV, dtype=torch.float16)
    for args in ((q, cos, kc, vc, pos.int(), Hq),                 # wrong dtype of pos
                 (q, cos, kc, vc, pos[:3], Hq),                   # wrong length
                 (q, cos, kc, vc, pos.cpu(), Hq),
                 (q[:, :1], cos[:, :1], kc, vc, pos, Hq),         # one token per stream: the streams launch
                 (q, cos[:, :1], kc, vc, pos, Hq),                # one rotary row for the window
                 (q, cos[:1], kc, vc, pos, Hq),                   # one rotary window for every stream
                 (q, cos, wide, wide, pos, Hq),                   # non-contiguous cache
                 (q, cos, kc96, kc96, pos, Hq),                   # D = 96
                 (q, cos, kc, vc, pos, 32),                       # 16 query heads per kv head
                 (q.float(), cos, kc, vc, pos, Hq)):
        assert not decode_attention_verify_supported(*args)
    kc0 = kc.clone()
    for bad in (dict(pos=pos.int()), dict(pos=pos[:3]), dict(kc=wide, vc=wide), dict(kc=kc96, vc=kc96),
                dict(k=k[:, :2]), dict(sin=sin[:, :2])):
        a = dict(kc=kc, vc=vc, pos=pos, k=k, sin=sin)
        a.update(bad)
        with pytest.raises(ValueError):
            decode_attention_verify(q, a["k"], v, cos, a["sin"], a["kc"], a["vc"], a["pos"], Hq, 0.125)
    torch.cuda.synchronize()
    assert torch.equal(kc, kc0)   # nothing ran
