"""GPU: sliding-window attention over a ring KV cache (layer_ops.decode_attention_window / prefill_attention_window).
Every stream is a fixed token sequence indexed by absolute position; the reference is fp64 softmax over positions
max(0, p - W + 1) .. p of what torch's own rotary would have written, gathered by position, never by ring slot.
Bars: test_gpu_decode_attention_streams.py's and test_gpu_prefill_attention.py's (2e-3 fp16, 1e-2 bf16)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
TOL = {torch.float16: 2e-3, torch.bfloat16: 1e-2}
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])


def _tokens(B, N, Hq, Hkv, D, dtype, seed):
    """N tokens per stream: q / k / v [B, N, *], cos / sin [B, N, D] and torch's rotated q / k [B, N, H, D]."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    q, k, v = (torch.randn(B, N, H * D, device=DEV, generator=g).to(dtype) for H in (Hq, Hkv, Hkv))
    ang = torch.rand(B, N, D // 2, device=DEV, generator=g) * 6.0
    cos, sin = (torch.cat((f(ang), f(ang)), -1).to(dtype) for f in (torch.cos, torch.sin))

    def rot(x, H):
        x = x.view(B, N, H, D)
        half = torch.cat((-x[..., D // 2:], x[..., : D // 2]), -1)
        return (x * cos.unsqueeze(2)) + (half * sin.unsqueeze(2))
    return q, k, v, cos, sin, rot(q, Hq), rot(k, Hkv)


def _ref(qr, hk, hv, p, W, scale):
    """One row at position p in fp64: qr [Hq, D]; hk / hv [P, Hkv, D] by absolute position.  -> [Hq * D]"""
    lo, G = max(0, p - W + 1), qr.shape[0] // hk.shape[1]
    kk = hk[lo:p + 1].double().transpose(0, 1).repeat_interleave(G, 0)      # [Hq, n, D]
    vv = hv[lo:p + 1].double().transpose(0, 1).repeat_interleave(G, 0)
    sc = torch.einsum("hd,hnd->hn", qr.double(), kk) * scale
    return torch.einsum("hn,hnd->hd", torch.softmax(sc, -1), vv).reshape(-1)


def _ring(B, Hkv, R, D, dtype):
    return tuple(torch.full((B, Hkv, R, D), float("nan"), device=DEV, dtype=dtype) for _ in range(2))


def _decode_run(tok, kc, vc, W, Hq, offs, steps, scale):
    """Steps 0 .. steps - 1 with stream b at position step - offs[b] (negative: an idle NaN row); every output."""
    from quantizations_amd.layer_ops import decode_attention_window

    q, k, v, cos, sin = tok[:5]
    rows = torch.arange(len(offs), device=DEV)
    outs = []
    for s in range(steps):
        pos = torch.tensor([s - o for o in offs], dtype=torch.int64, device=DEV)
        i = pos.clamp(min=0)
        outs.append(decode_attention_window(q[rows, i, None], k[rows, i, None], v[rows, i, None], cos[rows, i, None],
                                            sin[rows, i, None], kc, vc, pos, Hq, scale, W))
    return torch.cat(outs, 1)                                              # [B, steps, Hq * D]


@DTYPES
@pytest.mark.parametrize("W", [1, 96, 128, 200])
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (8, 2)])
@pytest.mark.parametrize("D", [64, 128])
def test_decode_matches_fp64_through_two_laps_of_the_ring(D, Hq, Hkv, W, dtype):
    from quantizations_amd.layer_ops import ring_size

    R, offs, scale = ring_size(W), (0, 1, 67), 1.0 / math.sqrt(D)
    steps = 2 * R + 6
    tok = _tokens(3, steps, Hq, Hkv, D, dtype, seed=W + D + Hq)
    kc, vc = _ring(3, Hkv, R, D, dtype)
    out = _decode_run(tok, kc, vc, W, Hq, offs, steps, scale)
    v, qr, kr = tok[2].view(3, steps, Hkv, D), tok[5], tok[6]
    for s in (W - 1, W, R - 1, R, R + 1, 2 * R + 5):
        for b, o in enumerate(offs):
            if s - o < 0:
                assert torch.isnan(out[b, s]).all()
                continue
            ref = _ref(qr[b, s - o], kr[b], v[b], s - o, W, scale)
            torch.testing.assert_close(out[b, s].double(), ref, atol=TOL[dtype], rtol=TOL[dtype])


@pytest.mark.parametrize("W", [1, 96, 128, 200, 600])      # 600: a ring above 512 slots reads its rows behind the mask
def test_decode_census_every_visible_key_once(W):
    """q = 0 and v = onehot(position % D): output element d is (visible keys with j % D == d) / (visible keys), at
    every step of two laps over a NaN-filled ring.  A key missed, doubled, stale or wrongly admitted moves an element
    by 1 / n >= 1 / 600 (or makes it NaN); the fp16 rounding of a quotient below 1 is under 2^-11."""
    from quantizations_amd.layer_ops import ring_size

    D, Hq, Hkv, R, offs = 64, 8, 2, ring_size(W), (0, 1, 67)
    steps = 2 * R + 6
    q, k, v, cos, sin = _tokens(3, steps, Hq, Hkv, D, torch.float16, seed=W)[:5]
    q.zero_()
    v.copy_(torch.eye(D, device=DEV, dtype=v.dtype)[torch.arange(steps, device=DEV) % D].repeat(1, Hkv)[None])
    kc, vc = _ring(3, Hkv, R, D, torch.float16)
    out = _decode_run((q, k, v, cos, sin), kc, vc, W, Hq, offs, steps, 0.125).view(3, steps, Hq, D)
    for b, o in enumerate(offs):
        for s in range(o, steps):
            p = s - o
            vis = torch.arange(max(0, p - W + 1), p + 1, device=DEV)
            want = torch.bincount(vis % D, minlength=D).double() / vis.numel()
            assert (out[b, s].double() - want).abs().max() < 1e-3, (b, p, out[b, s, 0], want)


@DTYPES
@pytest.mark.parametrize("D,Hq,Hkv", [(64, 4, 4), (128, 8, 2)])
@pytest.mark.parametrize("W,ps", [(96, (0, 50, 95)), (200, (0, 130, 199)), (600, (127, 511, 599))])
def test_decode_below_the_window_keeps_the_streams_launch_bits(W, ps, D, Hq, Hkv, dtype):
    from quantizations_amd.layer_ops import decode_attention_streams, decode_attention_window, ring_size

    R = ring_size(W)
    q, k, v, cos, sin = (t[:, :1] for t in _tokens(3, 2, Hq, Hkv, D, dtype, seed=W + D)[:5])
    g = torch.Generator(device="cuda").manual_seed(1)
    kc, vc = (torch.randn(3, Hkv, R, D, device=DEV, generator=g).to(dtype) for _ in range(2))
    for b, p in enumerate(ps):
        kc[b, :, p + 1:] = vc[b, :, p + 1:] = float("nan")
    kc2, vc2 = kc.clone(), vc.clone()
    pos = torch.tensor(ps, dtype=torch.int64, device=DEV)
    want = decode_attention_streams(q, k, v, cos, sin, kc2, vc2, pos, Hq, 0.1)
    out = decode_attention_window(q, k, v, cos, sin, kc, vc, pos, Hq, 0.1, W)
    assert not torch.isnan(out).any()
    for a, b in ((out, want), (kc, kc2), (vc, vc2)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("D,Hq,Hkv,dtype", [(64, 4, 4, torch.float16), (128, 8, 2, torch.bfloat16)])
@pytest.mark.parametrize("chunks", [(1, 17, 64, 130), (130, 130, 130)])
@pytest.mark.parametrize("W", [16, 96, 200])          # 16: rows of a 64-row query tile that see nothing in its first key tile
def test_prefill_chunks_and_a_decode_step_after_each_match_fp64(W, chunks, D, Hq, Hkv, dtype):
    from quantizations_amd.layer_ops import decode_attention_window, prefill_attention_window, ring_size

    R, scale, N = ring_size(W, max(chunks)), 1.0 / math.sqrt(D), sum(chunks) + len(chunks) + 130
    q, k, v, cos, sin, qr, kr = _tokens(2, N, Hq, Hkv, D, dtype, seed=W + D + len(chunks))
    vh = v.view(2, N, Hkv, D)
    kc, vc = _ring(2, Hkv, R, D, dtype)
    cur, rows = [0, 0], torch.arange(2, device=DEV)
    for T in chunks:
        lens = [T, max(1, T - 3)]
        pos = torch.tensor(cur, dtype=torch.int64, device=DEV)
        i = pos[:, None] + torch.arange(T, device=DEV)                     # [2, T] token rows
        out = prefill_attention_window(*(t[rows[:, None], i] for t in (q, k, v, cos, sin)), kc, vc, pos,
                                       torch.tensor(lens, dtype=torch.int64, device=DEV), Hq, scale, W)
        for b in range(2):
            ref = torch.stack([_ref(qr[b, cur[b] + j], kr[b], vh[b], cur[b] + j, W, scale) for j in range(lens[b])])
            torch.testing.assert_close(out[b, :lens[b]].double(), ref, atol=TOL[dtype], rtol=TOL[dtype])
            assert not out[b, lens[b]:].any()
            cur[b] += lens[b]
        pos = torch.tensor(cur, dtype=torch.int64, device=DEV)             # the ring holds what a decode step expects
        out = decode_attention_window(*(t[rows, pos, None] for t in (q, k, v, cos, sin)), kc, vc, pos, Hq, scale, W)
        for b in range(2):
            ref = _ref(qr[b, cur[b]], kr[b], vh[b], cur[b], W, scale)
            torch.testing.assert_close(out[b, 0].double(), ref, atol=TOL[dtype], rtol=TOL[dtype])
            cur[b] += 1


@DTYPES
def test_prefill_of_a_prompt_shorter_than_the_window_keeps_prefill_attention_bits(dtype):
    from quantizations_amd.layer_ops import prefill_attention, prefill_attention_window

    D, Hq, Hkv, W, T, R = 128, 8, 2, 96, 90, 256
    q, k, v, cos, sin = _tokens(2, T, Hq, Hkv, D, dtype, seed=5)[:5]
    pos = torch.zeros(2, dtype=torch.int64, device=DEV)
    lens = torch.tensor([90, 70], dtype=torch.int64, device=DEV)
    (kc, vc), (kc2, vc2) = _ring(2, Hkv, R, D, dtype), _ring(2, Hkv, R, D, dtype)
    want = prefill_attention(q, k, v, cos, sin, kc2, vc2, pos, lens, Hq, 0.1)
    out = prefill_attention_window(q, k, v, cos, sin, kc, vc, pos, lens, Hq, 0.1, W)
    assert not torch.isnan(out).any()
    for a, b in ((out, want), (kc, kc2), (vc, vc2)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_host_guards():
    from quantizations_amd import layer_ops as lo

    Hq, Hkv, D = 4, 2, 64
    q, k, v, cos, sin = _tokens(2, 64, Hq, Hkv, D, torch.float16, seed=0)[:5]
    kc, vc = _ring(2, Hkv, 128, D, torch.float16)
    pos, lens = torch.zeros(2, dtype=torch.int64, device=DEV), torch.full((2,), 64, dtype=torch.int64, device=DEV)
    assert lo.prefill_attention_window_supported(q, cos, kc, vc, pos, lens, Hq, 65)
    assert not lo.prefill_attention_window_supported(q, cos, kc, vc, pos, lens, Hq, 66)      # 66 + 64 - 1 > 128
    with pytest.raises(ValueError, match="ring"):
        lo.prefill_attention_window(q, k, v, cos, sin, kc, vc, pos, lens, Hq, 0.125, 66)
    one = [t[:, :1] for t in (q, k, v, cos, sin)]
    assert lo.decode_attention_window_supported(one[0], one[3], kc, vc, pos, Hq, 128)
    with pytest.raises(ValueError, match="ring"):
        lo.decode_attention_window(*one, kc, vc, pos, Hq, 0.125, 129)
    with pytest.raises(ValueError, match="ring"):                                            # not a multiple of 128
        lo.decode_attention_window(*one, kc[:, :, :100].contiguous(), vc[:, :, :100].contiguous(), pos, Hq, 0.125, 64)
    k96 = torch.zeros(2, Hkv, 128, 96, device=DEV, dtype=torch.float16)
    assert not lo.decode_attention_window_supported(one[0], one[3], k96, k96, pos, Hq, 64)                   # D = 96
    assert not lo.decode_attention_window_supported(one[0].float(), one[3].float(), kc.float(), vc.float(), pos, Hq, 64)
    assert not lo.prefill_attention_window_supported(q, cos, k96, k96, pos, lens, Hq, 16)
    torch.cuda.synchronize()
    assert torch.isnan(kc).all()   # nothing ran
