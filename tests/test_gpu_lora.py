"""GPU: LoRA adapters on Linear4bit inside the fused decode launches (lora.shrink + the *_lora
GEMVs), against the fp64 reference dequantize_4bit(W) @ x' + scaling * B (A x') at the project's
GEMV bar (test_gpu_parity.assert_close).

Inputs: W = 0.02 randn (fp16, NF4 + double quant unless stated), x = randn, A = 0.02 randn,
B = randn / sqrt(r), scaling = 1: the adapter term has about the norm of the base output, and each
parity test first asserts on the reference that it is at least a quarter of it, so the tolerance
cannot hide a dropped term or rank index.

t (shrink alone): the kernel's fp32 dot of K exact 16-bit products against fp64.  An fp32 summation
tree of depth d is bounded (first order) by d * 2^-24 * sum|a_k x_k|.  The kernel's depth: each of
256 threads adds its 8 * ceil(K / 2048) products in sequence, then 6 butterfly steps, 2 adds of the
four wave partials and the scaling multiply: d = 8 * ceil(K / 2048) + 9.  Bar per rank row:
|t - t_ref| <= d * 2^-24 * scaling * sum_k |a_jk x'_k|.  (One dropped product is about 1 / K of that
sum: 40x the bar at K = 14336, more at smaller K.)
"""
import math

import pytest
import torch
from test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
_WEIGHTS = {}


def _weight(M, K, qt="nf4", dq=True):
    """(packed, state, fp64 dequantised W [M, K]) -- quantised once per shape and shared."""
    from quantizations_amd.core import dequantize_4bit, quantize_4bit

    key = (M, K, qt, dq)
    if key not in _WEIGHTS:
        g = torch.Generator().manual_seed(M * 31 + K)
        W = (torch.randn(M, K, generator=g) * 0.02).half().to(DEV)
        packed, st = quantize_4bit(W, quant_type=qt, compress_statistics=dq)
        Wd = dequantize_4bit(packed, st, out_dtype=torch.float32).t().double().contiguous()
        _WEIGHTS[key] = (packed, st, Wd)
    return _WEIGHTS[key]


def _inputs(M, K, r, dtype, seed=0):
    # (seeds whose rank-1 draws keep |t| away from zero: the precondition of _ref)
    g = torch.Generator().manual_seed(1000 * seed + M + 7 * K + 5 * r)
    x = torch.randn(1, 1, K, generator=g).to(dtype).to(DEV)
    A = (torch.randn(r, K, generator=g) * 0.02).to(dtype).to(DEV)
    B = (torch.randn(M, r, generator=g) / math.sqrt(r)).to(dtype).to(DEV)
    return x, A, B


def _adapter(A, B, scaling=1.0):
    from quantizations_amd.lora import LoraAdapter

    return LoraAdapter(A, B, scaling, A.device)


def _ref(Wd, xp, A, B, scaling=1.0, bias=None):
    """(fp64 reference, base term, adapter term) for the 16-bit x' the GEMV multiplies."""
    xd = xp.double().reshape(-1)
    base = Wd @ xd
    if bias is not None:
        base = base + bias.double()
    ad = (B.double() @ (A.double() @ xd)) * scaling
    assert ad.norm() >= 0.25 * base.norm(), (ad.norm().item(), base.norm().item())
    return base + ad, base, ad


SHAPES = [(64, 4096), (300, 1000), (1023, 4096), (4096, 4096), (8192, 8192), (4096, 14336)]


@pytest.mark.parametrize("exact", [True, None])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("r", [1, 3, 16, 64])
@pytest.mark.parametrize("M,K", SHAPES)
def test_gemv_lora_parity_and_residual(M, K, r, dtype, exact):
    from quantizations_amd import lora
    from quantizations_amd.core import gemv_4bit

    packed, st, Wd = _weight(M, K)
    x, A, B = _inputs(M, K, r, dtype)
    bias = None
    if M == 1023:
        bias = (torch.randn(M, generator=torch.Generator().manual_seed(5)) * 0.1).to(dtype).to(DEV)
    yref, _, _ = _ref(Wd, x, A, B, bias=bias)
    t, offs = lora.shrink(x, [_adapter(A, B)])
    assert offs == [0] and t.shape == (r,) and t.dtype == torch.float32
    y = gemv_4bit(x, packed, state=st, bias=bias, exact_codes=exact, lora=(B, t))
    assert y.shape == (1, 1, M) and y.dtype == dtype
    assert_close(y.double().cpu().numpy(), yref.cpu().numpy(), dtype, f"lora gemv {M}x{K} r={r}")
    # the residual epilogue keeps its form: round(residual + round(y)), the torch add of the plain output
    res = (torch.randn(1, 1, M, generator=torch.Generator().manual_seed(6)) * 4).to(dtype).to(DEV)
    yr = gemv_4bit(x, packed, state=st, bias=bias, exact_codes=exact, residual=res, lora=(B, t))
    assert torch.equal(yr, res + y)


@pytest.mark.parametrize("qt,dq", [("fp4", True), ("nf4", False)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_gemv_lora_fp4_and_plain_absmax(qt, dq, dtype):
    from quantizations_amd import lora
    from quantizations_amd.core import gemv_4bit

    M, K, r = 4096, 4096, 16
    packed, st, Wd = _weight(M, K, qt, dq)
    x, A, B = _inputs(M, K, r, dtype, seed=1)
    yref, _, _ = _ref(Wd, x, A, B)
    t, _ = lora.shrink(x, [_adapter(A, B)])
    y = gemv_4bit(x, packed, state=st, lora=(B, t))
    assert_close(y.double().cpu().numpy(), yref.cpu().numpy(), dtype, f"lora gemv {qt} dq={dq}")


# ---------------------------------------------------------------------------
# shrink alone
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("with_norm", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("ranks", [(1,), (16, 8), (64, 64, 64, 64)])      # R_total 1, 24, 256
@pytest.mark.parametrize("K", [1000, 1024, 4096, 14336])
def test_shrink_against_fp64(K, ranks, dtype, with_norm):
    """K = 1000 is served by the same kernel (16-B chunks of 8 elements: K % 8 == 0), not declined."""
    from quantizations_amd import layer_ops, lora

    g = torch.Generator().manual_seed(K + sum(ranks))
    x = torch.randn(1, 1, K, generator=g).to(dtype).to(DEV)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(dtype).to(DEV)
    ads, scal = [], []
    for i, r in enumerate(ranks):
        scal.append(0.5 + 0.75 * i)
        ads.append(_adapter((torch.randn(r, K, generator=g) * 0.02).to(dtype).to(DEV),
                            torch.zeros(8, r, dtype=dtype, device=DEV), scal[-1]))
    t, offs = lora.shrink(x, ads, norm=(nw, 1e-5) if with_norm else None)
    assert t.shape == (sum(ranks),) and offs == [sum(ranks[:i]) for i in range(len(ranks))]
    xp = layer_ops.rms_norm(x, nw, 1e-5) if with_norm else x     # the stored output of the norm launch
    xd = xp.double().reshape(-1)
    for a, s, o in zip(ads, scal, offs):
        tref = (a.A.double() @ xd) * s
        mag = (a.A.double().abs() @ xd.abs()) * s
        bound = (8 * math.ceil(K / 2048) + 9) * 2.0 ** -24 * mag
        err = (t[o:o + a.r].double() - tref).abs()
        print(f"shrink K={K} r={a.r} norm={with_norm}: max err / bound = {(err / bound).max().item():.3e}")
        assert bool((err <= bound).all()), (err / bound).max().item()


def test_shrink_declines_unaligned_k():
    from quantizations_amd import _lib, lora

    x = torch.randn(1, 1, 1004, device=DEV).half()
    ad = _adapter(torch.zeros(4, 1004, device=DEV).half(), torch.zeros(8, 4, device=DEV).half())
    assert not lora.fused_ok(ad, x)                               # K % 8 != 0: the composed path
    with pytest.raises(_lib.QuantizationsError, match="shape"):
        lora.shrink(x, [ad])


# ---------------------------------------------------------------------------
# grouped launches
# ---------------------------------------------------------------------------


def _group(rows, K, dtype, exact, norm, ranks=(8, None, 64), zero_b=False):
    """Grouped launch with adapters on some segments -> (outs with, outs without, refs or None)."""
    from quantizations_amd import layer_ops, lora
    from quantizations_amd.core import gemv_4bit_grouped

    g = torch.Generator().manual_seed(sum(rows) + K)
    x = torch.randn(1, 1, K, generator=g).to(dtype).to(DEV)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(dtype).to(DEV)
    nrm = (nw, 1e-5) if norm else None
    xp = layer_ops.rms_norm(x, nw, 1e-5) if norm else x
    items, ads, refs = [], [], []
    for i, M in enumerate(rows):
        packed, st, Wd = _weight(M, K)
        items.append((packed, st, None))
        r = ranks[-1] if i == len(rows) - 1 else ranks[i]   # the first and the last segment
        if r is None:
            ads.append(None)
            refs.append(None)
            continue
        _, A, B = _inputs(M, K, r, dtype, seed=2 + i)
        if zero_b:
            B = torch.zeros_like(B)
            refs.append(None)
        else:
            refs.append(_ref(Wd, xp, A, B)[0])
        ads.append(_adapter(A, B))
    t, offs = lora.shrink(x, ads, norm=nrm)
    lo = (t, [None if a is None else (a.B, o) for a, o in zip(ads, offs)])
    got = gemv_4bit_grouped(x, items, exact_codes=exact, norm=nrm, lora=lo)
    plain = gemv_4bit_grouped(x, items, exact_codes=exact, norm=nrm)
    return got, plain, refs


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("dtype,exact", [(torch.float16, True), (torch.float16, None), (torch.bfloat16, None)])
@pytest.mark.parametrize("rows,K", [((4096, 1024, 1024), 4096), ((2048, 2048), 4096), ((1024, 256, 256), 1024)])
def test_grouped_lora_mixed_segments(rows, K, dtype, exact, norm):
    """Adapters (ranks 8 and 64) on the first and last segment only; K = 1024 has no full K-step, so
    its norm runs as its own launch."""
    got, plain, refs = _group(rows, K, dtype, exact, norm)
    for i, (y, p, ref) in enumerate(zip(got, plain, refs)):
        if ref is None:
            assert torch.equal(y, p), f"segment {i} has no adapter: the plain launch's bits"
        else:
            assert not torch.equal(y, p)
            assert_close(y.double().cpu().numpy(), ref.cpu().numpy(), dtype, f"grouped {rows} seg {i}")


# ---------------------------------------------------------------------------
# zero adapter: every launch form returns the bits of the call without one
# ---------------------------------------------------------------------------


def _lin(M, K, dtype, bias=False, seed=0, compute_dtype=torch.float32):
    import quantizations_amd as qa

    g = torch.Generator().manual_seed(seed + M + K)
    W = (torch.randn(M, K, generator=g) * 0.02).half()
    m = qa.Linear4bit(K, M, bias=bias, quant_type="nf4", compute_dtype=compute_dtype)
    m.weight = qa.Params4bit(W, requires_grad=False, quant_type="nf4", module=m)
    if bias:
        m.bias = torch.nn.Parameter((torch.randn(M, generator=g) * 0.1).to(dtype), requires_grad=False)
    return m.to(DEV)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_zero_adapter_is_bit_identical_in_every_form(dtype):
    from quantizations_amd import layer_ops
    from quantizations_amd.integration import fuse_projection_groups
    from quantizations_amd.modules import linear4bit_silu_pair

    cd = torch.float32 if dtype == torch.float16 else None
    K, M = 4096, 2048
    x = torch.randn(1, 1, K, generator=torch.Generator().manual_seed(3)).to(dtype).to(DEV)
    res = torch.randn(1, 1, M, generator=torch.Generator().manual_seed(4)).to(dtype).to(DEV)
    lin = _lin(M, K, dtype, bias=True, compute_dtype=cd)
    y0, yr0 = lin(x), lin.forward_residual(x, res)
    lin.set_adapter(torch.randn(16, K).to(dtype), torch.zeros(M, 16, dtype=dtype), 1.0)
    assert lin.adapter.A.device == x.device
    assert torch.equal(lin(x), y0) and torch.equal(lin.forward_residual(x, res), yr0)      # single, residual
    # grouped, grouped + fused norm, and the pair route (gate/up: grouped launch + silu_mul)
    mlp = torch.nn.Module()
    mlp.gate_proj, mlp.up_proj = _lin(M, K, dtype, seed=1, compute_dtype=cd), _lin(M, K, dtype, seed=2, compute_dtype=cd)
    assert fuse_projection_groups(mlp) == 1
    grp = mlp.gate_proj.__dict__["_qz_group"]
    nw = (1 + 0.1 * torch.randn(K)).to(dtype).to(DEV)

    def forms():
        out = []
        for norm in (None, (nw, 1e-5, lambda v: layer_ops.rms_norm(v, nw, 1e-5))):
            grp.prenorm = norm
            xi = x.clone()
            g, u = mlp.gate_proj(xi), mlp.up_proj(xi)
            h = linear4bit_silu_pair(grp, xi)
            out += [g, u, h if h is not None else layer_ops.silu_mul(g, u)]
        grp.prenorm = None
        return out

    plain = forms()
    assert linear4bit_silu_pair(grp, x) is not None
    mlp.up_proj.set_adapter(torch.randn(8, K).to(dtype), torch.zeros(M, 8, dtype=dtype), 1.0)
    assert linear4bit_silu_pair(grp, x) is None          # a member with an adapter: not the pair launch
    for a, b in zip(forms(), plain):
        assert torch.equal(a, b)
    mlp.gate_proj.set_adapter(torch.randn(64, K).to(dtype), torch.zeros(M, 64, dtype=dtype), 1.0)
    for a, b in zip(forms(), plain):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# fallbacks: the composed torch form
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("case", ["3 tokens", "fp32 x", "rank 65"])
def test_fallbacks_take_the_composed_form(case):
    import torch.nn.functional as F

    from quantizations_amd import lora
    from quantizations_amd.core import dequantize_4bit

    M, K = 1024, 1024
    r = 65 if case == "rank 65" else 16
    dtype = torch.float32 if case == "fp32 x" else torch.float16
    lin = _lin(M, K, torch.float16, compute_dtype=None)
    g = torch.Generator().manual_seed(9)
    T = 3 if case == "3 tokens" else 1
    x = torch.randn(1, T, K, generator=g).to(dtype).to(DEV)
    A = (torch.randn(r, K, generator=g) * 0.02).half().to(DEV)
    B = (torch.randn(M, r, generator=g) / math.sqrt(r)).half().to(DEV)
    lin.set_adapter(A, B, 1.0)
    ad = lin.adapter
    assert not lora.fused_ok(ad, x)
    y = lin(x)
    lin.clear_adapter()
    y0 = lin(x)
    dt = torch.promote_types(dtype, torch.float16)
    term = F.linear(F.linear(x.to(dt), A.to(dt)), B.to(dt)) * ad.scaling
    assert y.dtype == dtype and torch.equal(y, y0 + term.to(dtype))          # the composed torch form
    Wd = dequantize_4bit(lin.weight, lin.weight.quant_state, out_dtype=torch.float32).t().double()
    for i in range(T):
        yref, _, _ = _ref(Wd, x[0, i], A, B)
        assert_close(y[0, i].double().cpu().numpy(), yref.cpu().numpy(), dtype, f"fallback {case} token {i}")


# ---------------------------------------------------------------------------
# whole model
# ---------------------------------------------------------------------------


def _tiny_llama(seed=4):
    from transformers import LlamaConfig, LlamaForCausalLM

    from quantizations_amd.integration import replace_with_bnb_linear

    cfg = LlamaConfig(hidden_size=1024, intermediate_size=2048, num_hidden_layers=2, num_attention_heads=8,
                      num_key_value_heads=2, vocab_size=512)
    torch.manual_seed(seed)
    model = LlamaForCausalLM(cfg).half().to(DEV).eval()
    replace_with_bnb_linear(model, quant_type="nf4", compute_dtype=torch.float32)
    return cfg, model


def _adapters_for(model, names, seed, ranks):
    import quantizations_amd as qa

    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, m in model.named_modules():
        leaf = name.split(".")[-1]
        if isinstance(m, qa.Linear4bit) and leaf in names:
            r = ranks[leaf]
            out[name] = ((torch.randn(r, m.in_features, generator=g) * 0.02).half(),
                         (torch.randn(m.out_features, r, generator=g) / math.sqrt(r)).half(), 1.0)
    return out


def _decode(model, cfg, ids, graph, between=None):
    """Logits of the prefill's last token and of four decode steps; graph: the steps after the first
    are replays of one captured step (`between` runs after the capture, before the replays)."""
    from transformers.cache_utils import StaticCache

    cache = StaticCache(config=cfg, max_cache_len=32)
    out = model(input_ids=ids, past_key_values=cache, cache_position=torch.arange(9, device=DEV))
    tok = out.logits[:, -1:].argmax(-1)
    pos = torch.tensor([9], device=DEV)
    logits = []

    def step():
        return model(input_ids=tok, past_key_values=cache, cache_position=pos, position_ids=pos.view(1, 1)).logits

    if graph:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            lo = step()
        torch.cuda.current_stream().wait_stream(s)
        logits.append(lo[:, -1].clone())
        pos.add_(1)
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph):
            lo = step()
        if between is not None:
            between()
        for _ in range(3):
            gph.replay()
            logits.append(lo[:, -1].clone())
            pos.add_(1)
    else:
        for _ in range(4):
            lo = step()
            logits.append(lo[:, -1].clone())
            pos.add_(1)
    torch.cuda.synchronize()
    return logits


ALL7 = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


@pytest.mark.parametrize("names", [ALL7, ("q_proj", "v_proj")], ids=["all7", "qv"])
def test_tiny_llama_with_adapters(names):
    import quantizations_amd as qa
    from quantizations_amd.integration import (fuse_layer_ops, fuse_prenorm, fuse_projection_groups,
                                               unfuse_layer_ops)

    cfg, model = _tiny_llama()
    ranks = {"q_proj": 16, "k_proj": 8, "v_proj": 64, "o_proj": 16, "gate_proj": 4, "up_proj": 16, "down_proj": 3}
    ad1 = _adapters_for(model, names, 11, ranks)
    ad2 = _adapters_for(model, names, 12, ranks)
    mods = dict(model.named_modules())
    ids = torch.randint(0, 512, (1, 9), device=DEV, generator=torch.Generator(device="cuda").manual_seed(1))

    def set_all(ads):
        for name, (A, B, s) in ads.items():
            mods[name].set_adapter(A, B, s)

    class DenseF32(torch.nn.Linear):
        """fp32 weight, fp32 matmul, on the model's fp16 activations"""
        def forward(self, x):
            return torch.nn.functional.linear(x.float(), self.weight).to(x.dtype)

    def dense_ref(ads):
        """the same model with every Linear4bit as a dense fp32 nn.Linear holding dequantize() + s B A"""
        import copy
        ref = copy.deepcopy(model)
        for name, m in list(ref.named_modules()):
            if isinstance(m, qa.Linear4bit):
                W = mods[name].dequantize().float()
                if name in ads:
                    A, B, s = ads[name]
                    W = W + s * (B.float().to(DEV) @ A.float().to(DEV))
                lin = DenseF32(m.in_features, m.out_features, bias=False, device=DEV, dtype=torch.float32)
                lin.weight.data.copy_(W)
                parent = ref.get_submodule(name.rsplit(".", 1)[0])
                parent._modules[name.rsplit(".", 1)[1]] = lin
        return ref

    with torch.no_grad():
        ref1 = _decode(dense_ref(ad1), cfg, ids, False)
        ref2 = _decode(dense_ref(ad2), cfg, ids, False)
        fuse_projection_groups(model)
        fuse_layer_ops(model)
        fuse_prenorm(model)
        try:
            set_all(ad1)
            assert sum(m.adapter is not None for m in mods.values() if isinstance(m, qa.Linear4bit)) == \
                len(names) * cfg.num_hidden_layers
            eager1 = _decode(model, cfg, ids, False)
            for a, b in zip(eager1, ref1):
                rel = ((a.float() - b).norm() / b.norm()).item()
                print(f"tiny llama {names[:2]}: logits rel err {rel:.3e}")
                assert rel < 2e-3, rel
            graph1 = _decode(model, cfg, ids, True)
            assert all(torch.equal(a, b) for a, b in zip(graph1, eager1))
            # captured with adapter 1, replayed with adapter 2 (same ranks: copied in place)
            swapped = _decode(model, cfg, ids, True, between=lambda: set_all(ad2))
            eager2_first = _decode(model, cfg, ids, False)       # adapter 2 from the start ...
            set_all(ad1)
            # ... but the swapped run took its prefill and first step with adapter 1: replay that eagerly
            mixed = _decode_switch(model, cfg, ids, lambda: set_all(ad2))
            assert all(torch.equal(a, b) for a, b in zip(swapped, mixed))
            for a, b in zip(eager2_first, ref2):
                assert ((a.float() - b).norm() / b.norm()).item() < 2e-3
        finally:
            unfuse_layer_ops(model)


def _decode_switch(model, cfg, ids, switch):
    """_decode(graph=False) with `switch` called where the graph run calls `between`: after the
    second decode step's inputs are fixed (the captured step's own eager-less capture computes nothing)."""
    from transformers.cache_utils import StaticCache

    cache = StaticCache(config=cfg, max_cache_len=32)
    out = model(input_ids=ids, past_key_values=cache, cache_position=torch.arange(9, device=DEV))
    tok = out.logits[:, -1:].argmax(-1)
    pos = torch.tensor([9], device=DEV)
    logits = []
    for i in range(4):
        if i == 1:
            switch()
        lo = model(input_ids=tok, past_key_values=cache, cache_position=pos, position_ids=pos.view(1, 1)).logits
        logits.append(lo[:, -1].clone())
        pos.add_(1)
    torch.cuda.synchronize()
    return logits
