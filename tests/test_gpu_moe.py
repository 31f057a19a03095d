"""Routed 4-bit mixture-of-experts decode (csrc/moe.hip, moe.SparseMoe4bit) against fp64 torch on the
product's own dequantize_4bit output.  Expert e's weights are scaled by 2^((3e) % 7 - 3): a launch
that reads a neighbouring expert's codes or scales is off by >= 2x, not by a few percent.  Error bars
are measured, not fixed: twice the worst error of a plain torch twin in the activation dtype.

Measured on an MI355X (per-row error / row max; kernel vs twin): see profiles/moe_gpu_tests.txt."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E, TOPK = 8, 2
FORMATS = [("nf4", True), ("fp4", False)]
DTYPES = [torch.float16, torch.bfloat16]


@functools.lru_cache(maxsize=None)
def experts(H, I, dtype, qt, dq, bs=64):
    """Stacked expert-tagged weights, quantised flat; the dequantised experts in fp64; 16 token rows."""
    import quantizations_amd as qa
    g = torch.Generator().manual_seed(H + I)
    tag = (2.0 ** ((3 * torch.arange(E)) % 7 - 3))[:, None, None]
    out = {}
    for name, rows, K in (("gu", 2 * I, H), ("dn", H, I)):
        w = (torch.randn(E, rows, K, generator=g) * 0.02 * tag).to(DEV, dtype).reshape(-1, K)
        packed, st = qa.quantize_4bit(w, blocksize=bs, quant_type=qt, compress_statistics=dq)
        out[name] = (packed, st, qa.dequantize_4bit(packed, st).t().reshape(E, rows, K).double())
    out["x"] = torch.randn(16, H, generator=g).to(DEV, dtype)
    out["h"] = (torch.randn(16, TOPK, I, generator=g) * 0.5).to(DEV, dtype)
    return out


def routing(pattern, T, seed=0):
    g = torch.Generator().manual_seed(seed + T)
    idx = torch.stack([torch.randperm(E, generator=g)[:TOPK] for _ in range(T)])
    if pattern == "same":
        idx[:] = torch.tensor([2, 5])
    elif pattern == "cover":
        idx = torch.stack([torch.arange(T) % E, (torch.arange(T) + 3) % E], dim=1)
    elif pattern == "ends":
        idx[:] = torch.tensor([E - 1, 0])
    elif pattern == "invalid":
        idx.view(-1)[1] = -1
        idx.view(-1)[-2] = E
    w = torch.rand(T, TOPK, generator=g) + 0.1
    return idx.to(DEV, torch.int32), (w / w.sum(-1, keepdim=True)).to(DEV)


PATTERNS = ("random", "same", "cover", "ends", "invalid")


def pair_ref(x, W, idx, dtype):
    """h [T, k, I] from weights W [E, 2I, H] in W's precision (fp64: the reference; dtype: the twin)."""
    T, I = x.shape[0], W.shape[1] // 2
    h = torch.zeros(T, idx.shape[1], I, dtype=W.dtype, device=DEV)
    for t, s in ((t, s) for t in range(T) for s in range(idx.shape[1]) if 0 <= idx[t, s] < E):
        gate, up = F.linear(x[t].to(W.dtype), W[idx[t, s]]).chunk(2)
        h[t, s] = F.silu(gate) * up
    return h


def down_ref(h, W, idx, w, dtype):
    T = h.shape[0]
    acc = torch.float64 if W.dtype == torch.float64 else torch.float32
    y = torch.zeros(T, W.shape[1], dtype=acc, device=DEV)
    for t, s in ((t, s) for t in range(T) for s in range(idx.shape[1]) if 0 <= idx[t, s] < E):
        y[t] += w[t, s].to(acc) * F.linear(h[t, s].to(W.dtype), W[idx[t, s]]).to(acc)
    return y.to(W.dtype)


def row_err(out, ref):
    """Worst row of max |out - ref| / max |ref| (rows whose reference is all zero must be zero)."""
    out, ref = out.double().flatten(0, -2), ref.flatten(0, -2)
    scale = ref.abs().amax(-1)
    assert torch.all(out[scale == 0] == 0)
    rel = (out - ref).abs().amax(-1)[scale > 0] / scale[scale > 0]
    return rel.max().item() if rel.numel() else 0.0


def check_both(H, I, T, dtype, qt, dq, bs=64):
    from quantizations_amd.core import moe_down, moe_pair_silu
    c = experts(H, I, dtype, qt, dq, bs)
    x, hin = c["x"][:T], c["h"][:T].contiguous()
    for pattern in PATTERNS:
        idx, w = routing(pattern, T)
        h = moe_pair_silu(x, c["gu"][0], c["gu"][1], idx, E)
        y = moe_down(hin, c["dn"][0], c["dn"][1], idx, w, E)
        href, yref = pair_ref(x, c["gu"][2], idx, dtype), down_ref(hin, c["dn"][2], idx, w, dtype)
        htwin = pair_ref(x, c["gu"][2].to(dtype), idx, dtype)
        ytwin = down_ref(hin, c["dn"][2].to(dtype), idx, w, dtype)
        eh, bh, ey, by = row_err(h, href), 2 * row_err(htwin, href), row_err(y, yref), 2 * row_err(ytwin, yref)
        print(f"H{H} I{I} T{T} {dtype} {qt} dq={dq} bs={bs} {pattern}: pair {eh:.3e} (bar {bh:.3e}) "
              f"down {ey:.3e} (bar {by:.3e})")
        assert eh <= bh and ey <= by, (pattern, eh, bh, ey, by)
        if pattern == "invalid":
            bad = (idx < 0) | (idx >= E)
            assert bad.sum() == 2 and torch.all(h[bad] == 0)


@pytest.mark.parametrize("qt, dq", FORMATS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [1, 2, 16])
@pytest.mark.parametrize("H, I", [(256, 256), (512, 768)])
def test_pair_and_down(H, I, T, dtype, qt, dq):
    check_both(H, I, T, dtype, qt, dq)


def test_experts_share_a_second_level_block():
    check_both(256, 256, 16, torch.float16, "nf4", True, bs=4096)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_hot_reads_an_expert_back(dtype):
    """T = 1, one-hot activations: every column of one expert through each kernel, bit for bit."""
    from quantizations_amd.core import moe_down, moe_pair_silu
    from quantizations_amd.layer_ops import silu_mul
    c = experts(256, 256, dtype, "nf4", True)
    e = 5
    idx, one = torch.tensor([[e]], dtype=torch.int32, device=DEV), torch.ones(1, 1, device=DEV)
    eye = torch.eye(256, device=DEV, dtype=dtype)
    Wgu, Wdn = c["gu"][2][e].to(dtype), c["dn"][2][e].to(dtype)
    hs = torch.stack([moe_pair_silu(eye[k:k + 1], c["gu"][0], c["gu"][1], idx, E)[0, 0] for k in range(256)], dim=1)
    assert torch.equal(hs, silu_mul(Wgu[:256].contiguous(), Wgu[256:].contiguous()))
    ys = torch.stack([moe_down(eye[k].view(1, 1, 256), c["dn"][0], c["dn"][1], idx, one, E)[0] for k in range(256)],
                     dim=1)
    assert torch.equal(ys, Wdn)


@pytest.mark.parametrize("H, I, dtype, qt, dq", [(256, 256, torch.float16, "nf4", True),
                                                  (512, 768, torch.bfloat16, "fp4", False)])
def test_batch_invariance_and_residual(H, I, dtype, qt, dq):
    from quantizations_amd.core import moe_down, moe_pair_silu
    c = experts(H, I, dtype, qt, dq)
    x, hin = c["x"], c["h"]
    res = torch.randn(16, H, device=DEV).to(dtype)
    for pattern in ("random", "same", "cover"):
        idx, w = routing(pattern, 16)
        h = moe_pair_silu(x, c["gu"][0], c["gu"][1], idx, E)
        y = moe_down(hin, c["dn"][0], c["dn"][1], idx, w, E)
        for t in range(16):
            s = slice(t, t + 1)
            assert torch.equal(h[s], moe_pair_silu(x[s], c["gu"][0], c["gu"][1], idx[s].contiguous(), E)), (pattern, t)
            assert torch.equal(y[s], moe_down(hin[s].contiguous(), c["dn"][0], c["dn"][1], idx[s].contiguous(),
                                              w[s].contiguous(), E)), (pattern, t)
        assert torch.equal(moe_down(hin, c["dn"][0], c["dn"][1], idx, w, E, residual=res), res + y)


# ---------------------------------------------------------------------------
SEED = 3   # chosen so that the gap holds for >= 90 % of the tokens of every case below (asserted)


def route_case(Er, k, T, dtype, seed):
    """x [T, 256] and a router weight scaled for logits of about 0.5: 16-bit values, the fp64 router on
    them, and the tokens whose k-th / (k+1)-th logit gap exceeds one 16-bit ulp of those logits."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, 256, generator=g).to(dtype)
    W = (torch.randn(Er, 256, generator=g) / 32).to(dtype)
    logits = x.double() @ W.double().t()
    p = torch.softmax(logits, -1)
    top_v, top_i = torch.topk(p, k, -1)
    srt = logits.sort(-1, descending=True).values
    if k == Er:
        holds = torch.ones(T, dtype=torch.bool)
    else:
        mant = 10 if dtype == torch.float16 else 7
        ulp = 2.0 ** (torch.floor(torch.log2(srt[:, k - 1:k + 1].abs().amax(-1))) - mant)
        holds = (srt[:, k - 1] - srt[:, k]) > ulp
    return x, W, top_i, top_v / top_v.sum(-1, keepdim=True), holds


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [1, 5, 16])
@pytest.mark.parametrize("Er, k", [(8, 2), (4, 1), (64, 8)])
def test_route(Er, k, T, dtype):
    from quantizations_amd.core import moe_route
    x, W, ref_i, ref_w, holds = route_case(Er, k, T, dtype, seed=SEED)
    assert holds.float().mean() >= 0.9
    idx, w, logits = moe_route(x.to(DEV), W.to(DEV), k, logits=True)
    idx, w = idx.cpu().long(), w.cpu().double()
    exact = x.double() @ W.double().t()   # the stored logits: the fp64 ones rounded once (half an ulp)
    assert torch.all((logits.cpu().double() - exact).abs() <= exact.abs() * 2.0 ** (-11 if dtype == torch.float16 else -8) + 1e-6)
    assert torch.all(w[:, :-1] >= w[:, 1:]) and torch.all((idx >= 0) & (idx < Er))
    tol = 2.0 ** (-8 if dtype == torch.float16 else -6)
    for t in torch.nonzero(holds).flatten().tolist():
        assert set(idx[t].tolist()) == set(ref_i[t].tolist()), t
        ref = dict(zip(ref_i[t].tolist(), ref_w[t].tolist()))
        for e, v in zip(idx[t].tolist(), w[t].tolist()):
            assert abs(v - ref[e]) <= tol * ref[e], (t, e, v, ref[e])



@pytest.mark.parametrize("k, want", [(1, [1]), (2, [1, 3]), (3, [1, 3, 6])])
def test_route_tie_goes_to_the_lower_index(k, want):
    from quantizations_amd.core import moe_route
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 256, generator=g).half()
    W = (torch.randn(8, 256, generator=g) / 64).half()
    W[6] = W[3] = W[1] = (x[0] / 64).half()          # three identical rows: exactly equal logits, the largest
    idx, w = moe_route(x[:1].to(DEV), W.to(DEV), k)
    assert idx[0].tolist() == want and torch.equal(w[0], w[0, :1].expand(k))


# ---------------------------------------------------------------------------
def test_graph_replay_follows_new_routing():
    from quantizations_amd.moe import SparseMoe4bit
    g = torch.Generator().manual_seed(1)
    tag = (2.0 ** ((3 * torch.arange(E)) % 7 - 3))[:, None, None]
    moe = SparseMoe4bit((torch.randn(E, 256, generator=g) / 16).half().to(DEV),
                        (torch.randn(E, 512, 256, generator=g) * 0.02 * tag).half().to(DEV),
                        (torch.randn(E, 256, 256, generator=g) * 0.02 * tag).half().to(DEV), TOPK)
    xs = [torch.randn(4, 256, generator=g).half().to(DEV) for _ in range(3)]
    choices = [torch.topk(F.linear(x, moe.gate.weight), TOPK).indices for x in xs]
    assert not torch.equal(choices[0], choices[1])   # the replays route elsewhere than the capture did
    x = xs[0].clone()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        moe(x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = moe(x)
    for xn in xs[1:] + xs[:1] + xs[1:]:
        x.copy_(xn)
        graph.replay()
        assert torch.equal(y, moe(xn))


# ---------------------------------------------------------------------------
def mixtral(seed):
    from transformers import MixtralConfig, MixtralForCausalLM
    cfg = MixtralConfig(hidden_size=256, intermediate_size=256, num_local_experts=E, num_experts_per_tok=TOPK,
                        num_attention_heads=4, num_key_value_heads=4, num_hidden_layers=2, vocab_size=512,
                        max_position_embeddings=128, attn_implementation="eager", experts_implementation="eager")
    torch.manual_seed(seed)
    return MixtralForCausalLM(cfg).half().to(DEV).eval()


def quantised(model):
    import quantizations_amd as qa
    from quantizations_amd.integration import replace_with_bnb_linear
    return qa.replace_moe_blocks(replace_with_bnb_linear(model))


def test_module_in_a_mixtral_model():
    import quantizations_amd as qa
    from quantizations_amd.moe import SparseMoe4bit
    dense = mixtral(0)
    model = quantised(copy.deepcopy(dense))
    blocks = [m for m in model.modules() if isinstance(m, SparseMoe4bit)]
    assert len(blocks) == 2 and not any(p.dim() == 3 for p in model.parameters())
    assert all(b.gate_up_proj.dtype == torch.uint8 and b.down_proj.dtype == torch.uint8 for b in blocks)
    assert copy.deepcopy(blocks[0]).gate_up_proj.quant_state is not None
    for name, m in model.named_modules():   # the dense twin carries the dequantised weights in the model dtype
        if isinstance(m, qa.Linear4bit):
            dense.get_submodule(name).weight.data.copy_(m.dequantize())
        elif isinstance(m, SparseMoe4bit):
            ex = dense.get_submodule(name).experts
            for pn in ("gate_up_proj", "down_proj"):
                p = getattr(m, pn)
                getattr(ex, pn).data.copy_(qa.dequantize_4bit(p, p.quant_state).t().reshape(getattr(ex, pn).shape))
    exact = copy.deepcopy(dense).double()
    other = quantised(mixtral(1))
    other.load_state_dict(model.state_dict())
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for L in (5, 40):   # 5 rows: the three launches; 40 rows: the composed form
            ids = torch.randint(0, 512, (1, L), generator=g).to(DEV)
            ref = exact(ids).logits
            out = model(ids).logits
            err, bar = (out.double() - ref).abs().max().item(), 2 * (dense(ids).logits.double() - ref).abs().max().item()
            print(f"L={L}: 4-bit blocks {err:.3e}, bar (2 x dense twin) {bar:.3e}")
            assert err <= bar
            assert torch.equal(other(ids).logits, out)
