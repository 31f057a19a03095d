"""The routed one-token expert launches on the byte-table GEMV (csrc/moe_gemv.hip) against fp64 torch on the
product's own dequantize_4bit output, in the form of test_gpu_moe.py: expert e's weights carry the tag
2^((3e) % 7 - 3), so codes or scales read from a neighbouring expert are off by >= 2x, and the bar is measured --
twice the worst-row error of a plain torch twin in the activation dtype on the same inputs.  The reference weights
are dequantize_4bit's fp32 output, code x fp32 scale, which is what a byte-table kernel decodes (the dense pair's
test, test_gpu_mlp_pair.py, takes the same); the twin rounds them to the activation dtype.  Against the 16-bit
dequantisation the reference itself is off by a rounding per weight that these kernels do not make: fp16 FP4 at
(4096, 2048), one valid slot, measured 8.26e-4 against a one-row bar of 8.04e-4 there.

Shapes: (H, I) = (4096, 2048) and (2048, 6144) give K of two, one and three K-steps across the two kernels (the
straight-line form, the loop, an odd step count).  With blocksize 4096 a K-step kernel needs K % 4096 == 0, so
experts share a second-level scale block only where they have under 256 rows' worth of blocks: the pair is run at
I = 64 (two experts per absmax2 entry) and the down launch at H = 64 (four).

Measured on an MI355X (kernel vs bar): see profiles/moe_gemv_gpu_tests.txt."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_moe import down_ref, pair_ref, row_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROUTINGS = ("random", "descending", "ends", "invalid")


def experts(H, I, E, top_k, dtype, qt, dq, bs):
    """Stacked expert-tagged weights made on the device, quantised flat: (packed, state, dequantised fp64)."""
    import quantizations_amd as qa
    g = torch.Generator(device=DEV).manual_seed(H + I)
    tag = (2.0 ** ((3 * torch.arange(E, device=DEV)) % 7 - 3))[:, None, None]
    out = {}
    for name, rows, K in (("gu", 2 * I, H), ("dn", H, I)):
        w = (torch.randn(E, rows, K, generator=g, device=DEV) * 0.02 * tag).to(dtype).reshape(-1, K)
        packed, st = qa.quantize_4bit(w, blocksize=bs, quant_type=qt, compress_statistics=dq)
        out[name] = (packed, st, qa.dequantize_4bit(packed, st, out_dtype=torch.float32).t().reshape(E, rows, K).double())
    out["x"] = torch.randn(1, H, generator=g, device=DEV).to(dtype)
    out["h"] = (torch.randn(1, top_k, I, generator=g, device=DEV) * 0.5).to(dtype)
    out["res"] = torch.randn(1, H, generator=g, device=DEV).to(dtype)
    return out


def routing(pattern, E, top_k):
    g = torch.Generator().manual_seed(top_k)
    idx = torch.randperm(E, generator=g)[:top_k]
    if pattern == "descending":   # the down launch must walk these from the last slot to the first
        idx = idx.sort(descending=True).values
    elif pattern == "ends":
        idx[0], idx[1] = E - 1, 0
    elif pattern == "invalid":
        idx[1] = -1
    w = torch.rand(top_k, generator=g) + 0.1
    return idx.to(DEV, torch.int32)[None], (w / w.sum()).to(DEV)[None]


def check(H, I, E, top_k, dtype, qt, dq, bs=64, pair=True, down=True):
    from quantizations_amd.core import moe_gemv_down, moe_gemv_pair_silu
    c = experts(H, I, E, top_k, dtype, qt, dq, bs)
    for pattern in ROUTINGS:
        idx, w = routing(pattern, E, top_k)
        bad = idx < 0
        if pair:
            h = moe_gemv_pair_silu(c["x"], c["gu"][0], c["gu"][1], idx, E)
            ref = pair_ref(c["x"], c["gu"][2], idx, dtype)
            err, bar = row_err(h, ref), 2 * row_err(pair_ref(c["x"], c["gu"][2].to(dtype), idx, dtype), ref)
            print(f"H{H} I{I} E{E} k{top_k} {dtype} {qt} dq={dq} bs={bs} {pattern}: pair {err:.3e} (bar {bar:.3e})")
            assert err <= bar, (pattern, err, bar)
            # a slot without an expert: zeros, and the other slots keep the bits they have beside a real one
            other = moe_gemv_pair_silu(c["x"], c["gu"][0], c["gu"][1], idx.clamp(min=0), E)
            assert torch.all(h[bad] == 0) and torch.equal(h[~bad], other[~bad])
        if down:
            y = moe_gemv_down(c["h"], c["dn"][0], c["dn"][1], idx, w, E)
            ref = down_ref(c["h"], c["dn"][2], idx, w, dtype)
            err, bar = row_err(y, ref), 2 * row_err(down_ref(c["h"], c["dn"][2].to(dtype), idx, w, dtype), ref)
            print(f"H{H} I{I} E{E} k{top_k} {dtype} {qt} dq={dq} bs={bs} {pattern}: down {err:.3e} (bar {bar:.3e})")
            assert err <= bar, (pattern, err, bar)
            assert torch.equal(moe_gemv_down(c["h"], c["dn"][0], c["dn"][1], idx, w, E, residual=c["res"]), c["res"] + y)


@pytest.mark.parametrize("qt, dq", [("nf4", True), ("fp4", False)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("H, I, E, top_k", [(4096, 2048, 8, 2), (2048, 6144, 4, 3)])
def test_pair_and_down(H, I, E, top_k, dtype, qt, dq):
    check(H, I, E, top_k, dtype, qt, dq)


def test_experts_share_a_second_level_block():
    check(4096, 64, 8, 2, torch.float16, "nf4", True, bs=4096, down=False)
    check(64, 4096, 8, 2, torch.float16, "nf4", True, bs=4096, pair=False)


def test_declined_shapes_return_none():
    from quantizations_amd.core import moe_gemv_down, moe_gemv_pair_silu
    c = experts(256, 256, 8, 2, torch.float16, "nf4", True, 64)   # K = 256 is no whole K-step
    idx, w = routing("random", 8, 2)
    assert moe_gemv_pair_silu(c["x"], c["gu"][0], c["gu"][1], idx, 8) is None
    assert moe_gemv_down(c["h"], c["dn"][0], c["dn"][1], idx, w, 8) is None
    c = experts(2048, 2048, 8, 2, torch.float16, "nf4", True, 64)   # a shape both take, but two rows
    idx2, w2 = idx.repeat(2, 1), w.repeat(2, 1)
    assert moe_gemv_pair_silu(c["x"], c["gu"][0], c["gu"][1], idx, 8) is not None
    assert moe_gemv_pair_silu(c["x"].repeat(2, 1), c["gu"][0], c["gu"][1], idx2, 8) is None
    assert moe_gemv_down(c["h"].repeat(2, 1, 1), c["dn"][0], c["dn"][1], idx2, w2, 8) is None


@pytest.fixture(scope="module")
def block():
    from quantizations_amd.moe import SparseMoe4bit
    g = torch.Generator(device=DEV).manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)
    moe = SparseMoe4bit((r(8, 2048) / 32).half(), (r(8, 4096, 2048) * 0.02).half(), (r(8, 2048, 2048) * 0.02).half(), 2)
    xs = [r(1, 2048).half() for _ in range(3)]
    choices = [torch.topk(F.linear(x, moe.gate.weight), 2).indices.sort().values for x in xs]
    assert not torch.equal(choices[0], choices[1]) and not torch.equal(choices[0], choices[2])
    return moe, xs


@pytest.mark.parametrize("route", ["mma", "gemv"])
def test_module_route_runs_its_own_launches(block, route, monkeypatch):
    """"mma": the one-row output is what moe_pair_silu / moe_down give (the bits before this route existed); "gemv":
    what the two new launches give, residual included; any other value raises."""
    from quantizations_amd import core
    moe, xs = block
    monkeypatch.setattr(moe, "decode_route", route)
    pair, down = (core.moe_pair_silu, core.moe_down) if route == "mma" else (core.moe_gemv_pair_silu, core.moe_gemv_down)
    for x in xs:
        idx, w = core.moe_route(x, moe.gate.weight, 2)
        y = down(pair(x, moe.gate_up_proj, moe.gate_up_proj.quant_state, idx, 8), moe.down_proj,
                 moe.down_proj.quant_state, idx, w, 8)
        assert torch.equal(moe(x), y) and torch.equal(moe(x, _qz_residual=xs[0]), xs[0] + y)
    monkeypatch.setattr(moe, "decode_route", "fast")
    with pytest.raises(ValueError, match="decode_route"):
        moe(xs[0])


def test_graph_replay_follows_new_routing(block, monkeypatch):
    moe, xs = block
    monkeypatch.setattr(moe, "decode_route", "gemv")
    x = xs[0].clone()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        moe(x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = moe(x)
    for xn in xs[1:] + xs[:1] + xs[1:]:   # the replays route elsewhere than the capture did
        x.copy_(xn)
        graph.replay()
        assert torch.equal(y, moe(xn))
