"""GPU: decode attention with a position per stream (qz_decode_attention_streams,
layer_ops.decode_attention_streams).

The contract needs no tolerance: for every stream b, the output row and the cache rows written are
bit-identical to decode_attention called on that stream alone (B = 1 views, mask[j] = (j <= p_b),
*pos = p_b).  Cache rows above p_b hold NaN here: they must never reach the output.  L covers one
chunk (128), a ragged second chunk (130) and both sides of kAttnSpecL = 512 (384, 640); the
positions of the four streams are 0, 127, 128 (64 where L = 128 has no slot 128) and L - 1.
An fp64 restatement in torch (rotary, cache write, softmax) holds the values themselves at the bars
of test_gpu_decode_attention.py (2e-3 fp16, 1e-2 bf16)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
B = 4


def _positions(L):
    return [0, 127, 128 if L > 128 else 64, L - 1]


def _case(Hq, Hkv, D, L, ps, dtype, seed, nan_above=True):
    g = torch.Generator(device="cuda").manual_seed(seed)
    nb = len(ps)
    q = torch.randn(nb, 1, Hq * D, device=DEV, generator=g).to(dtype)
    k = torch.randn(nb, 1, Hkv * D, device=DEV, generator=g).to(dtype)
    v = torch.randn(nb, 1, Hkv * D, device=DEV, generator=g).to(dtype)
    ang = torch.rand(nb, 1, D // 2, device=DEV, generator=g) * 6.0      # a rotary row per stream
    cos = torch.cat((ang.cos(), ang.cos()), -1).to(dtype)
    sin = torch.cat((ang.sin(), ang.sin()), -1).to(dtype)
    kc = torch.randn(nb, Hkv, L, D, device=DEV, generator=g).to(dtype)
    vc = torch.randn(nb, Hkv, L, D, device=DEV, generator=g).to(dtype)
    if nan_above:
        for b, p in enumerate(ps):
            if 0 <= p < L:
                kc[b, :, p + 1:] = float("nan")
                vc[b, :, p + 1:] = float("nan")
    pos = torch.tensor(ps, dtype=torch.int64, device=DEV)
    return q, k, v, cos, sin, kc, vc, pos


def _bits(t):
    return t.contiguous().view(torch.int16)


def _solo(q, k, v, cos, sin, kc, vc, ps, Hq, scale):
    """decode_attention on each stream alone; returns (out [B, 1, Hq*D], caches) assembled."""
    from quantizations_amd.layer_ops import decode_attention

    L = kc.shape[2]
    outs, kcs, vcs = [], [], []
    for b, p in enumerate(ps):
        kb, vb = kc[b:b + 1].clone(), vc[b:b + 1].clone()
        mask = (torch.arange(L, device=DEV) <= p).view(1, 1, 1, L)
        pos = torch.tensor(p, dtype=torch.int64, device=DEV)
        arrive = torch.zeros(1, dtype=torch.int32, device=DEV)
        outs.append(decode_attention(q[b:b + 1], k[b:b + 1], v[b:b + 1], cos[b:b + 1], sin[b:b + 1], kb, vb, mask, pos,
                                     arrive, Hq, scale))
        kcs.append(kb), vcs.append(vb)
    return torch.cat(outs), torch.cat(kcs), torch.cat(vcs)


@pytest.mark.parametrize("L", [128, 130, 384, 640])
@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (8, 1)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_each_stream_carries_the_bits_of_its_solo_call(dtype, D, Hq, Hkv, L):
    from quantizations_amd.layer_ops import decode_attention_streams

    ps = _positions(L)
    q, k, v, cos, sin, kc, vc, pos = _case(Hq, Hkv, D, L, ps, dtype, seed=L + D + Hq)
    scale = 1.0 / math.sqrt(D)
    ref, kc_ref, vc_ref = _solo(q, k, v, cos, sin, kc, vc, ps, Hq, scale)
    out = decode_attention_streams(q, k, v, cos, sin, kc, vc, pos, Hq, scale)
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and not torch.isnan(ref).any()
    assert torch.equal(_bits(out), _bits(ref)), torch.nonzero(_bits(out) != _bits(ref))[:8]
    assert torch.equal(_bits(kc), _bits(kc_ref)) and torch.equal(_bits(vc), _bits(vc_ref))
    assert pos.tolist() == ps, "pos is read only"


def _rotate_half(x):
    x1, x2 = x[..., : x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("Hq,Hkv,D,L", [(4, 2, 64, 130), (8, 1, 128, 640)])
def test_values_against_an_fp64_restatement(dtype, Hq, Hkv, D, L):
    from quantizations_amd.layer_ops import decode_attention_streams

    ps = _positions(L)
    q, k, v, cos, sin, kc, vc, pos = _case(Hq, Hkv, D, L, ps, dtype, seed=3 * L + D)
    qh = q.view(B, 1, Hq, D).transpose(1, 2)
    kh = k.view(B, 1, Hkv, D).transpose(1, 2)
    c, s = cos.unsqueeze(1), sin.unsqueeze(1)
    qr = (qh * c) + (_rotate_half(qh) * s)            # apply_rotary_pos_emb, torch's own rounding
    kr = (kh * c) + (_rotate_half(kh) * s)
    kc2, vc2 = kc.clone(), vc.clone()
    for b, p in enumerate(ps):
        kc2[b, :, p] = kr[b, :, 0]
        vc2[b, :, p] = v[b].view(Hkv, D)
    visible = torch.arange(L, device=DEV)[None, :] <= pos[:, None]          # [B, L]
    G = Hq // Hkv
    # rows above p_b are NaN: they carry no weight, so the restatement drops them before 0 * NaN
    kk = torch.where(visible[:, None, :, None], kc2, torch.zeros_like(kc2)).double().repeat_interleave(G, dim=1)
    vv = torch.where(visible[:, None, :, None], vc2, torch.zeros_like(vc2)).double().repeat_interleave(G, dim=1)
    sc = (qr.double() @ kk.transpose(-1, -2)) * (1.0 / math.sqrt(D))
    sc = sc.masked_fill(~visible[:, None, None, :], float("-inf"))
    ref = (torch.softmax(sc, dim=-1) @ vv).transpose(1, 2).reshape(B, 1, Hq * D)
    out = decode_attention_streams(q, k, v, cos, sin, kc, vc, pos, Hq, 1.0 / math.sqrt(D))
    torch.cuda.synchronize()
    assert torch.equal(_bits(kc), _bits(kc2)) and torch.equal(_bits(vc), _bits(vc2))
    tol = 2e-3 if dtype == torch.float16 else 1e-2
    torch.testing.assert_close(out.double(), ref, atol=tol, rtol=tol)


@pytest.mark.parametrize("L", [128, 384])     # one chunk / three chunks (the combine launch)
@pytest.mark.parametrize("bad", [-1, "L"])
def test_a_position_outside_the_cache_is_loud_for_its_stream_only(L, bad):
    from quantizations_amd.layer_ops import decode_attention_streams

    Hq, Hkv, D, dtype = 4, 2, 64, torch.float16
    good = [5, 127, 0, L - 1]
    q, k, v, cos, sin, kc, vc, pos = _case(Hq, Hkv, D, L, good, dtype, seed=L)
    scale = 1.0 / math.sqrt(D)
    kc0, vc0 = kc.clone(), vc.clone()
    want = decode_attention_streams(q, k, v, cos, sin, kc, vc, pos, Hq, scale)
    kc_w, vc_w = kc.clone(), vc.clone()
    kc.copy_(kc0), vc.copy_(vc0)
    pos[2] = L if bad == "L" else bad
    out = decode_attention_streams(q, k, v, cos, sin, kc, vc, pos, Hq, scale)
    torch.cuda.synchronize()
    assert torch.isnan(out[2]).all()
    assert torch.equal(_bits(kc[2]), _bits(kc0[2])) and torch.equal(_bits(vc[2]), _bits(vc0[2]))
    for b in (0, 1, 3):
        assert torch.equal(_bits(out[b]), _bits(want[b]))
        assert torch.equal(_bits(kc[b]), _bits(kc_w[b])) and torch.equal(_bits(vc[b]), _bits(vc_w[b]))


def test_one_captured_graph_follows_new_positions():
    from quantizations_amd.layer_ops import decode_attention_streams

    Hq, Hkv, D, L, dtype = 8, 1, 128, 640, torch.float16
    first = [3, 200, 639, 128]
    q, k, v, cos, sin, kc, vc, pos = _case(Hq, Hkv, D, L, first, dtype, seed=9, nan_above=False)
    scale = 1.0 / math.sqrt(D)
    kc0, vc0 = kc.clone(), vc.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        decode_attention_streams(q, k, v, cos, sin, kc, vc, pos, Hq, scale)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = decode_attention_streams(q, k, v, cos, sin, kc, vc, pos, Hq, scale)
    for ps in (first, [639, 0, 127, 511], [130, 131, 132, 133]):
        kc.copy_(kc0), vc.copy_(vc0)
        pos.copy_(torch.tensor(ps, device=DEV))
        g.replay()
        got, kc_g, vc_g = out.clone(), kc.clone(), vc.clone()
        kc.copy_(kc0), vc.copy_(vc0)
        eager = decode_attention_streams(q, k, v, cos, sin, kc, vc, pos, Hq, scale)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(eager)) and not torch.isnan(got).any()
        assert torch.equal(_bits(kc_g), _bits(kc)) and torch.equal(_bits(vc_g), _bits(vc))
        assert not torch.equal(_bits(kc), _bits(kc0))


def test_rejects_what_it_cannot_take():
    from quantizations_amd.layer_ops import decode_attention_streams, decode_attention_streams_supported

    Hq, Hkv, D, L = 4, 2, 64, 128
    q, k, v, cos, sin, kc, vc, pos = _case(Hq, Hkv, D, L, [1, 2, 3, 4], torch.float16, seed=1, nan_above=False)
    assert decode_attention_streams_supported(q, cos, kc, vc, pos, Hq)
    wide = torch.zeros(B, Hkv, L, 2 * D, device=DEV, dtype=torch.float16)[..., :D]      # a strided cache
    kc96 = torch.zeros(B, Hkv, L, 96, device=DEV, dtype=torch.float16)
    for args in ((q, cos, kc, vc, pos.int(), Hq),                 # wrong dtype of pos
                 (q, cos, kc, vc, pos[:3], Hq),                   # wrong length
                 (q, cos, kc, vc, pos[:1], Hq),                   # the shared-position form
                 (q, cos, kc, vc, pos.cpu(), Hq),
                 (q, cos, wide, wide, pos, Hq),                   # non-contiguous cache
                 (q, cos, kc96, kc96, pos, Hq),                   # D = 96
                 (q.float(), cos, kc, vc, pos, Hq)):
        assert not decode_attention_streams_supported(*args)
    kc0 = kc.clone()
    for bad in (dict(pos=pos.int()), dict(pos=pos[:3]), dict(kc=wide, vc=wide), dict(kc=kc96, vc=kc96)):
        a = dict(kc=kc, vc=vc, pos=pos)
        a.update(bad)
        with pytest.raises(ValueError):
            decode_attention_streams(q, k, v, cos, sin, a["kc"], a["vc"], a["pos"], Hq, 0.125)
    torch.cuda.synchronize()
    assert torch.equal(kc, kc0)   # nothing ran
