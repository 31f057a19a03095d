"""GPU: the decode attention launches leave the BITS they left before the wave-local head.

tests/golden/decode_attention_parent.npz holds, for every case of tests/golden/make_attention_golden.py,
the bytes of the output and of the cache rows the launch wrote, recorded once on an MI355X from the
commit before the head of csrc/attn_core.h was rescheduled (wave-local scores, softmax exchange and
P V; the sum of the probabilities keeps its tree).  The cases regenerate their inputs from
numpy.random.default_rng and must reproduce those bytes: fp16 / bf16, D 64 / 128, G 1 / 4 / 8, B 1 / 3,
L 1 .. 257 (one, two and three chunks), the new token at every wave seam of a chunk, masks with holes at
the seams, with one whole wave hidden and with everything hidden but the new token, and one launch of
each other form (streams, verify T = 2 and 4, paged, kv8 with a non-finite row).  Bytes, not values:
a NaN must be the same NaN.  Last, a captured graph replayed three times equals three eager calls."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_attention_golden",
                                               os.path.join(HERE, "golden", "make_attention_golden.py"))
gold = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gold)

CASES = gold.cases()


@pytest.fixture(scope="module")
def recorded():
    z = np.load(os.path.join(HERE, "golden", "decode_attention_parent.npz"))
    names, sizes, data = [str(n) for n in z["names"]], z["sizes"], z["data"]
    assert names == [n for n, _ in CASES], "the fixture was recorded from another case list"
    ends = np.cumsum(sizes)
    return {n: data[e - s: e] for n, s, e in zip(names, sizes, ends)}


@pytest.mark.parametrize("name,spec", CASES, ids=[n for n, _ in CASES])
def test_bits_equal_the_recorded_launch(recorded, name, spec):
    got = gold.run_case(name, spec)
    want = recorded[name]
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} of {got.size} bytes differ, first at {bad[:8]}"


def test_graph_replays_equal_eager_calls():
    from quantizations_amd.layer_ops import decode_attention

    dev = torch.device("cuda")
    B, Hq, Hkv, D, L, p0 = 1, 8, 2, 128, 128, 62     # three steps across the seam 63 | 64
    rng = np.random.default_rng(5)

    def t(*shape):
        return torch.from_numpy(rng.standard_normal(shape, dtype=np.float32)).to(dev).half()

    q, k, v = t(B, 1, Hq * D), t(B, 1, Hkv * D), t(B, 1, Hkv * D)
    ang = torch.from_numpy(rng.uniform(0.0, 6.0, (1, 1, D // 2)).astype(np.float32)).to(dev)
    cos, sin = torch.cat((ang.cos(), ang.cos()), -1).half(), torch.cat((ang.sin(), ang.sin()), -1).half()
    kc0, vc0 = t(B, Hkv, L, D), t(B, Hkv, L, D)
    mask = torch.ones(1, 1, 1, L, dtype=torch.bool, device=dev)   # the cache holds values everywhere
    scale = 1.0 / math.sqrt(D)

    def state():
        return (kc0.clone(), vc0.clone(), torch.tensor(p0, dtype=torch.int64, device=dev),
                torch.zeros(1, dtype=torch.int32, device=dev))

    kc, vc, pos, arrive = state()
    eager = [decode_attention(q, k, v, cos, sin, kc, vc, mask, pos, arrive, Hq, scale).clone() for _ in range(3)]
    torch.cuda.synchronize()
    kc_e, vc_e = kc.clone(), vc.clone()
    assert int(pos) == p0 + 3

    kc, vc, pos, arrive = state()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        decode_attention(q, k, v, cos, sin, kc, vc, mask, pos, arrive, Hq, scale)   # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    kc.copy_(kc0), vc.copy_(vc0), pos.fill_(p0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = decode_attention(q, k, v, cos, sin, kc, vc, mask, pos, arrive, Hq, scale)
    for i in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), eager[i].view(torch.int16)), f"replay {i}"
    assert int(pos) == p0 + 3 and int(arrive) == 0
    assert torch.equal(kc.view(torch.int16), kc_e.view(torch.int16)) and torch.equal(vc.view(torch.int16), vc_e.view(torch.int16))
