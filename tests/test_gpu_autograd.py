"""GPU: backward through Linear4bit -- the fused 4-bit dgrad GEMM (csrc/gemm_dgrad.hip,
core.gemm_4bit_dgrad) and autograd.MatMul4Bit.

* The W operand of the dgrad kernel is the dequantised weight, bit for bit: one-hot gradients pick
  single rows of it out of the MFMA (every output is one product plus exact zeros).
* Random gradients against the fp64 product of the dequantised weight (bit-exact to the oracle), on
  the project's GEMM bars (assert_close: 1e-3 relative norm + the elementwise bound).
* Linear4bit: same output bits with and without autograd, input / bias gradients, no weight
  gradient; compute_dtype casts, adapters and banks; the decode fast paths step aside for an input
  that requires grad and stay in place under no_grad.
* A tiny Llama with hand-written LoRA wrappers: every LoRA gradient against two dense twins.
"""
import copy
import math

import pytest
import torch

from test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")

# (T, M, K, blocksize): the kernel's tile is BT (64 | 128) tokens x 128 columns, 64 weight rows per step
SHAPES = [
    (5, 64, 64, 64),        # one step, one partial column tile
    (16, 200, 192, 64),     # M ragged against the 64-row step; K ragged against a 128-column tile
    (65, 1032, 320, 64),    # T across a 64-token tile; 21 absmax2 groups whose boundaries fall mid-row
    (130, 4096, 256, 64),   # long contraction on a 2-column-tile grid: split-M engages; T across 128
    (300, 264, 4096, 64),   # many column tiles, short contraction, no split
    (16, 200, 256, 128),    # blocksize above 64
    (16, 4104, 256, 64),    # 65 steps over 13 splits of 5: a ragged last split (4 1/8 steps) and a partial last step
    (130, 4104, 256, 64),   # the same split under the 128-token tile, T across it
]
_ID = [f"T{t}-M{m}-K{k}-bs{b}" for t, m, k, b in SHAPES]


def _weight(M, K, quant_type, dq, blocksize, dtype, seed):
    """(packed, state, Wd [M, K] = the dequantised weight in `dtype`, on the GPU)."""
    from quantizations_amd.core import dequantize_4bit, quantize_4bit

    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(M, K, generator=g) * 0.02).to(dtype).to(DEV)
    packed, st = quantize_4bit(W, blocksize=blocksize, quant_type=quant_type, compress_statistics=dq)
    Wd = dequantize_4bit(packed, st, out_dtype=dtype).t().contiguous()
    assert Wd.shape == (M, K)
    return packed, st, Wd


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("dq", [True, False], ids=["dq", "plain"])
@pytest.mark.parametrize("quant_type", ["nf4", "fp4"])
@pytest.mark.parametrize("T,M,K,bs", SHAPES, ids=_ID)
def test_dgrad_w_operand_is_the_dequantised_weight(T, M, K, bs, quant_type, dq, dtype):
    from quantizations_amd.core import gemm_4bit_dgrad

    packed, st, Wd = _weight(M, K, quant_type, dq, bs, dtype, seed=T + M + K)
    rows = torch.tensor([(997 * t + 13) % M for t in range(T)], device=DEV)
    G = torch.zeros(T, M, dtype=dtype, device=DEV)
    G[torch.arange(T, device=DEV), rows] = 1
    dX = gemm_4bit_dgrad(G, packed, st, route="fused")
    assert dX.shape == (T, K) and dX.dtype == dtype
    want = Wd[rows]
    bad = (dX != want).nonzero()
    assert torch.equal(dX, want), f"{bad.shape[0]} of {T * K} elements differ, first at {bad[:4].tolist()}"


@pytest.fixture(scope="module")
def random_cases():
    """(G, packed, state, fp64 reference) per (shape index, dtype), built once."""
    out = {}
    for i, (T, M, K, bs) in enumerate(SHAPES):
        for dtype in (torch.float16, torch.bfloat16):
            packed, st, Wd = _weight(M, K, "nf4", True, bs, dtype, seed=31 * i + 7)
            G = torch.randn(T, M, generator=torch.Generator().manual_seed(i)).to(dtype).to(DEV)
            out[i, dtype] = (G, packed, st, (G.double() @ Wd.double()).cpu().numpy())
    return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=_ID)
def test_dgrad_random_vs_fp64(random_cases, i, dtype):
    from quantizations_amd.core import gemm_4bit_dgrad

    G, packed, st, ref = random_cases[i, dtype]
    dX = gemm_4bit_dgrad(G, packed, st, route="fused")
    assert_close(dX.float().cpu().numpy(), ref, dtype, f"fused {_ID[i]}")


def test_dgrad_random_vs_oracle_weight(orc):
    """The weight from the CPU oracle's dequantiser, as test_gpu_edges._layer takes it."""
    from test_gpu_edges import _layer

    from quantizations_amd.core import gemm_4bit_dgrad

    m, wref, _ = _layer(orc, 320, 1032, "nf4", True, seed=5)
    G = torch.randn(65, 1032, generator=torch.Generator().manual_seed(9)).half()
    dX = gemm_4bit_dgrad(G.to(DEV), m.weight, m.weight.quant_state, route="fused")
    assert_close(dX.float().cpu().numpy(), (G.double() @ wref).numpy(), torch.float16, "oracle weight")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("i", [1, 3], ids=[_ID[1], _ID[3]])
def test_dgrad_dequant_route(random_cases, i, dtype):
    from quantizations_amd.core import gemm_4bit_dgrad

    G, packed, st, ref = random_cases[i, dtype]
    dX = gemm_4bit_dgrad(G, packed, st, route="dequant")
    assert dX.dtype == dtype
    assert_close(dX.float().cpu().numpy(), ref, dtype, f"dequant {_ID[i]}")
    # leading dimensions are kept, and auto agrees with one of the two routes' bars
    dX3 = gemm_4bit_dgrad(G.reshape(1, *G.shape), packed, st)
    assert dX3.shape == (1, G.shape[0], st.shape[1])
    assert_close(dX3.float().cpu().numpy(), ref, dtype, f"auto {_ID[i]}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("T,M,K", [(130, 4096, 256), (16, 200, 192)], ids=["split", "unsplit"])
def test_dgrad_strided_gradient(T, M, K, dtype):
    """G as a column slice of a wider tensor (row stride M + 64 > M, what autograd hands the layer when
    the output was sliced): the kernel reads it in place through ldg, bit-identical to the copy's result."""
    from quantizations_amd import _lib
    from quantizations_amd.core import gemm_4bit_dgrad

    packed, st, Wd = _weight(M, K, "nf4", True, 64, dtype, seed=T + M)
    wide = torch.randn(T, M + 64, generator=torch.Generator().manual_seed(T)).to(dtype).to(DEV)
    G = wide[:, 32:32 + M]
    assert G.stride(0) == M + 64 and not G.is_contiguous() and G.data_ptr() % 16 == 0
    assert (_lib.lib.qz_gemm_4bit_dgrad_workspace_size(T, M, K) > 0) == (M == 4096)
    dX = gemm_4bit_dgrad(G, packed, st, route="fused")
    assert torch.equal(dX, gemm_4bit_dgrad(G.contiguous(), packed, st, route="fused"))
    assert_close(dX.float().cpu().numpy(), (G.double() @ Wd.double()).cpu().numpy(), dtype, f"strided T={T} M={M}")
    # the C-ABI reads the view itself: a stride below M is refused, nothing launched
    out = torch.empty(T, K, dtype=dtype, device=DEV)
    assert _lib.lib.qz_gemm_4bit_dgrad(T, M, K, G.data_ptr(), M - 8, _lib.dtype_code(dtype), packed.data_ptr(), _lib.NF4,
                                       64, *st.scale_args(), out.data_ptr(), K, 0, 0, 0) == _lib.QZ_ERR_SHAPE


def test_dgrad_routes_that_do_not_apply():
    from quantizations_amd.core import gemm_4bit_dgrad

    packed, st, Wd = _weight(64, 100, "nf4", True, 64, torch.float16, seed=1)      # K = 100
    G = torch.randn(7, 64, device=DEV).half()
    with pytest.raises(ValueError):
        gemm_4bit_dgrad(G, packed, st, route="fused")
    assert_close(gemm_4bit_dgrad(G, packed, st).float().cpu().numpy(), (G.double() @ Wd.double()).cpu().numpy(),
                 torch.float16, "K=100 auto")
    packed, st, Wd = _weight(64, 128, "nf4", True, 64, torch.float16, seed=2)
    G32 = torch.randn(7, 64, device=DEV)
    with pytest.raises(ValueError):
        gemm_4bit_dgrad(G32, packed, st, route="fused")                              # fp32 G
    dX = gemm_4bit_dgrad(G32, packed, st)
    assert dX.dtype == torch.float32
    assert_close(dX.cpu().numpy(), (G32.double() @ Wd.double()).cpu().numpy(), torch.float32, "fp32 auto")
    with pytest.raises(ValueError):
        gemm_4bit_dgrad(G32, packed, st, route="nope")


# ---------------------------------------------------------------------------
# Linear4bit
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("bias_grad", [True, False], ids=["bias-grad", "bias-frozen"])
@pytest.mark.parametrize("in_f,out_f", [(320, 1000), (100, 3), (72, 130)])
@pytest.mark.parametrize("T", [1, 5, 40, 600])
def test_linear4bit_backward(orc, T, in_f, out_f, bias_grad):
    from test_gpu_edges import _layer

    m, wref, _ = _layer(orc, in_f, out_f, "nf4", True, seed=in_f + out_f + T)
    m.bias.requires_grad_(bias_grad)
    gen = torch.Generator().manual_seed(T)
    x = torch.randn(1, T, in_f, generator=gen).half().to(DEV).requires_grad_()
    g = torch.randn(1, T, out_f, generator=gen).half().to(DEV)
    y = m(x)
    assert y.grad_fn is not None and y.requires_grad
    with torch.no_grad():
        y0 = m(x.detach())
    assert y0.grad_fn is None and torch.equal(y, y0)
    y.backward(g)
    assert x.grad is not None and x.grad.dtype == x.dtype and x.grad.shape == x.shape
    ref = g.double().cpu().reshape(T, out_f) @ wref
    assert_close(x.grad.float().cpu().reshape(T, in_f).numpy(), ref.numpy(), torch.float16, f"dX T={T}")
    if bias_grad:
        assert m.bias.grad is not None and m.bias.grad.dtype == m.bias.dtype and m.bias.grad.shape == m.bias.shape
        assert_close(m.bias.grad.float().cpu().numpy(), g.double().cpu().reshape(T, out_f).sum(0).numpy(),
                     torch.float16, f"dbias T={T}")
    else:
        assert m.bias.grad is None
    assert m.weight.grad is None


def test_matmul4bit_is_exported_and_takes_bnb_argument_order(orc):
    import quantizations_amd as qa
    from test_gpu_edges import _layer

    m, wref, b = _layer(orc, 128, 64, "nf4", True, seed=3)
    x = torch.randn(6, 128, device=DEV).half().requires_grad_()
    y = qa.MatMul4Bit.apply(x, m.weight, None, m.bias, m.weight.quant_state)
    assert torch.equal(y, qa.matmul_4bit(x.detach(), m.weight, m.weight.quant_state, bias=m.bias))
    y.sum().backward()
    ref = torch.ones(6, 64, dtype=torch.float64) @ wref
    assert_close(x.grad.float().cpu().numpy(), ref.numpy(), torch.float16, "MatMul4Bit.apply")
    assert m.weight.grad is None


def test_compute_dtype_casts_are_differentiated(orc):
    """fp16 x through a bf16-compute layer: x -> bf16 -> MatMul4Bit -> fp16.  The backward rounds g to
    bf16 and multiplies the bf16 weight, so that is the reference; the bar is the bf16 output's."""
    from test_gpu_edges import _layer

    from quantizations_amd.core import dequantize_4bit

    m, _, _ = _layer(orc, 320, 1000, "nf4", True, seed=11)
    m.compute_dtype = torch.bfloat16
    x = torch.randn(2, 20, 320, device=DEV).half().requires_grad_()
    g = torch.randn(2, 20, 1000, device=DEV).half()
    y = m(x)
    assert y.dtype == torch.float16 and y.grad_fn is not None
    with torch.no_grad():
        assert torch.equal(y, m(x.detach()))
    y.backward(g)
    assert x.grad.dtype == torch.float16 and x.grad.shape == x.shape
    Wd = dequantize_4bit(m.weight, m.weight.quant_state, out_dtype=torch.bfloat16).t().double()
    ref = g.to(torch.bfloat16).double().reshape(40, 1000) @ Wd
    assert_close(x.grad.float().cpu().reshape(40, 320).numpy(), ref.cpu().numpy(), torch.bfloat16, "bf16 compute")


def _lora_weights(in_f, out_f, r, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.randn(r, in_f, generator=g) * 0.05).half().to(DEV),
            (torch.randn(out_f, r, generator=g) / math.sqrt(r) * 0.05).half().to(DEV))


@pytest.mark.parametrize("T", [1, 9])
def test_adapter_gradient(orc, T):
    from test_gpu_edges import _layer

    m, wref, _ = _layer(orc, 320, 1000, "nf4", True, seed=21)
    A, B = _lora_weights(320, 1000, 8, seed=1)
    s = 0.5
    m.set_adapter(A, B, s)
    x = torch.randn(1, T, 320, device=DEV).half().requires_grad_()
    g = torch.randn(1, T, 1000, device=DEV).half()
    y = m(x)
    with torch.no_grad():
        y0 = m(x.detach())          # T = 1: the fused adapter launches; same numerics class, not the same bits
    assert_close(y.detach().float().cpu().numpy(), y0.float().cpu().numpy(), torch.float16, "adapter forward")
    y.backward(g)
    weff = wref + s * (B.double().cpu() @ A.double().cpu())
    assert_close(x.grad.float().cpu().reshape(T, 320).numpy(), (g.double().cpu().reshape(T, 1000) @ weff).numpy(),
                 torch.float16, f"adapter dX T={T}")


def test_bank_gradient_per_row(orc):
    from test_gpu_edges import _layer

    m, wref, _ = _layer(orc, 320, 1000, "nf4", True, seed=22)
    ads = [(*_lora_weights(320, 1000, 8, seed=2), 0.5), (*_lora_weights(320, 1000, 4, seed=3), 2.0)]
    slots = torch.tensor([1, -1, 0, 1], dtype=torch.int32, device=DEV)
    m.set_adapter_bank(ads, slots)
    x = torch.randn(4, 1, 320, device=DEV).half().requires_grad_()
    g = torch.randn(4, 1, 1000, device=DEV).half()
    m(x).backward(g)
    for row, a in enumerate(slots.tolist()):
        weff = wref if a < 0 else wref + ads[a][2] * (ads[a][1].double().cpu() @ ads[a][0].double().cpu())
        assert_close(x.grad[row, 0].float().cpu().numpy(), (g[row, 0].double().cpu() @ weff).numpy(), torch.float16,
                     f"bank row {row} (adapter {a})")


# ---------------------------------------------------------------------------
# the decode fast paths step aside
# ---------------------------------------------------------------------------


def _tiny_llama(seed=4, compute_dtype=torch.float16):
    from transformers import LlamaConfig, LlamaForCausalLM

    from quantizations_amd.integration import replace_with_bnb_linear

    cfg = LlamaConfig(hidden_size=1024, intermediate_size=2048, num_hidden_layers=2, num_attention_heads=8,
                      num_key_value_heads=2, vocab_size=512)
    torch.manual_seed(seed)
    model = LlamaForCausalLM(cfg).half().to(DEV).eval()
    replace_with_bnb_linear(model, quant_type="nf4", compute_dtype=compute_dtype)
    return cfg, model


def _dense_weight(lin):
    return lin.dequantize().double().cpu()      # [out, in]


@pytest.mark.parametrize("prenorm", [False, True], ids=["plain", "prenorm"])
def test_groups_step_aside_for_a_grad_input(prenorm):
    from quantizations_amd import core
    from quantizations_amd.integration import fuse_prenorm, fuse_projection_groups

    _, model = _tiny_llama()
    model.requires_grad_(False)
    layer = model.model.layers[0]
    att, mlp = layer.self_attn, layer.mlp
    x = torch.randn(1, 1, 1024, device=DEV).half()
    with torch.no_grad():   # the un-grouped layers on the (normalised) token
        xa, xm = (layer.input_layernorm(x), layer.post_attention_layernorm(x)) if prenorm else (x, x)
        want = {"q": att.q_proj(xa), "k": att.k_proj(xa), "v": att.v_proj(xa), "gate": mlp.gate_proj(xm),
                "up": mlp.up_proj(xm)}
    assert fuse_projection_groups(model) > 0
    if prenorm:
        assert fuse_prenorm(model) > 0
    projs = {"q": att.q_proj, "k": att.k_proj, "v": att.v_proj, "gate": mlp.gate_proj, "up": mlp.up_proj}
    norms = {"q": layer.input_layernorm, "k": layer.input_layernorm, "v": layer.input_layernorm,
             "gate": layer.post_attention_layernorm, "up": layer.post_attention_layernorm}

    with torch.no_grad():   # without autograd: the grouped launch
        core.LAST_FORM.pop("grouped", None)
        before = {n: projs[n](x) for n in ("q", "k", "v")}
        form = core.LAST_FORM["grouped"]

    core.LAST_FORM.pop("grouped", None)
    xg = x.clone().requires_grad_()
    outs = {n: p(xg) for n, p in projs.items()}
    assert "grouped" not in core.LAST_FORM          # no grouped launch on the grad route
    gen = torch.Generator().manual_seed(5)
    for n, o in outs.items():
        assert o.grad_fn is not None and torch.equal(o, want[n]), n
        g = torch.randn(o.shape, generator=gen).half()
        (dx,) = torch.autograd.grad(o, xg, g.to(DEV))
        xr = x.double().cpu().reshape(-1).requires_grad_()
        xin = xr
        if prenorm:     # LlamaRMSNorm in fp64
            w = norms[n].weight.double().cpu()
            xin = w * xr * torch.rsqrt(xr.pow(2).mean() + norms[n].variance_epsilon)
        (g.double().reshape(-1) @ (_dense_weight(projs[n]) @ xin)).backward()
        assert dx.dtype == x.dtype and dx.shape == x.shape
        assert_close(dx.float().cpu().reshape(-1).numpy(), xr.grad.numpy(), torch.float16, f"{n}_proj dX")

    # the same token without autograd still takes the grouped launch, as before
    with torch.no_grad():
        after = {n: projs[n](x) for n in ("q", "k", "v")}
    assert core.LAST_FORM["grouped"] == form
    for n in after:
        assert after[n].grad_fn is None and torch.equal(after[n], before[n]), n


def test_silu_pair_steps_aside_for_a_grad_input():
    import quantizations_amd as qa
    from quantizations_amd import core
    from quantizations_amd.modules import DecodeGroup, _linear4bit_group_compute, linear4bit_silu_pair

    def proj(seed):     # 2048 -> 3000: a shape the pair launch takes
        W = (torch.randn(3000, 2048, generator=torch.Generator().manual_seed(seed)) * 0.02).half()
        m = qa.Linear4bit(2048, 3000, bias=False, quant_type="nf4", compute_dtype=torch.float16)
        m.weight = qa.Params4bit(W, requires_grad=False, quant_type="nf4", module=m)
        return m.to(DEV)

    gate, up = proj(1), proj(2)
    grp = DecodeGroup([gate, up], _linear4bit_group_compute)   # as integration.fuse_projection_groups attaches it
    gate.__dict__["_qz_group"] = up.__dict__["_qz_group"] = grp
    x = torch.randn(1, 1, 2048, device=DEV).half()
    core.LAST_FORM.pop("pair", None)
    with torch.no_grad():
        h = linear4bit_silu_pair(grp, x)
    assert h is not None and core.LAST_FORM["pair"] == "pair"
    xg = x.clone().requires_grad_()
    assert linear4bit_silu_pair(grp, xg) is None
    hg = torch.nn.functional.silu(gate(xg)) * up(xg)
    assert hg.grad_fn is not None and torch.equal(hg, h)
    (dx,) = torch.autograd.grad(hg, xg, torch.ones_like(hg))
    assert dx.shape == x.shape and torch.isfinite(dx).all() and dx.abs().max() > 0
    with torch.no_grad():
        h2 = linear4bit_silu_pair(grp, xg)      # grad mode off: the launch again
    assert h2 is not None and torch.equal(h2, h)


def test_forward_residual_on_the_grad_route(orc):
    from test_gpu_edges import _layer

    m, wref, _ = _layer(orc, 320, 1000, "nf4", True, seed=23)
    x = torch.randn(1, 1, 320, device=DEV).half()
    res = torch.randn(1, 1, 1000, device=DEV).half()
    with torch.no_grad():
        fused = m.forward_residual(x, res)           # the epilogue add, bit-identical to the torch add
    xg, rg = x.clone().requires_grad_(), res.clone().requires_grad_()
    out = m.forward_residual(xg, rg)
    assert out.grad_fn is not None and torch.equal(out, fused)
    g = torch.randn(1, 1, 1000, device=DEV).half()
    out.backward(g)
    assert torch.equal(rg.grad, g)
    assert_close(xg.grad.float().cpu().reshape(-1).numpy(), (g.double().cpu().reshape(-1) @ wref).numpy(),
                 torch.float16, "forward_residual dX")
    # only the residual carries a gradient: still differentiable
    rg2 = res.clone().requires_grad_()
    out2 = m.forward_residual(x, rg2)
    assert out2.grad_fn is not None and torch.equal(out2, fused)


def test_layer_op_predicates_decline_grad_inputs():
    from quantizations_amd import layer_ops

    x = torch.randn(2, 64, device=DEV).half()
    w = torch.ones(64, device=DEV).half()
    xg = x.clone().requires_grad_()
    assert layer_ops.rms_norm_supported(x, w) and not layer_ops.rms_norm_supported(xg, w)
    assert layer_ops.silu_mul_supported(x, x) and not layer_ops.silu_mul_supported(xg, x)
    assert not layer_ops.silu_mul_supported(x, xg)
    assert layer_ops.add_rms_norm_supported(x, x, w) and not layer_ops.add_rms_norm_supported(x, xg, w)
    with torch.no_grad():
        assert layer_ops.rms_norm_supported(xg, w) and layer_ops.silu_mul_supported(xg, xg)


# ---------------------------------------------------------------------------
# whole model: LoRA gradients against dense twins
# ---------------------------------------------------------------------------


class _LoRA(torch.nn.Module):
    def __init__(self, base, r, seed, scale=2.0):
        super().__init__()
        self.base, self.scale = base, scale
        self.lora_A = torch.nn.Linear(base.in_features, r, bias=False)
        self.lora_B = torch.nn.Linear(r, base.out_features, bias=False)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            self.lora_A.weight.copy_(torch.randn(r, base.in_features, generator=g) * 0.02)
            self.lora_B.weight.copy_(torch.randn(base.out_features, r, generator=g) * 0.02)
        self.lora_A.to(device=DEV, dtype=torch.float16)
        self.lora_B.to(device=DEV, dtype=torch.float16)

    def forward(self, x):
        return self.base(x) + self.lora_B(self.lora_A(x)) * self.scale


def _lora_grads(model, ids):
    model.zero_grad(set_to_none=True)
    logits = model(input_ids=ids, use_cache=False).logits
    logits.float().pow(2).mean().backward()
    return {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if "lora_" in n}


def test_tiny_llama_lora_gradients():
    """Measured bar: e_dense = rel. error of the fp16 dense twin's LoRA gradients against the fp32
    twin's; ours against the fp32 twin may be at most 2 x e_dense per parameter."""
    import quantizations_amd as qa

    _, model = _tiny_llama()
    model.requires_grad_(False)
    seed = 100
    for layer in model.model.layers:
        for name in ("q_proj", "v_proj"):
            seed += 1
            setattr(layer.self_attn, name, _LoRA(getattr(layer.self_attn, name), 8, seed))

    def twin(dtype):
        t = copy.deepcopy(model)
        for parent in list(t.modules()):
            for name, child in list(parent.named_children()):
                if isinstance(child, qa.Linear4bit):
                    lin = torch.nn.Linear(child.in_features, child.out_features, bias=False, device=DEV,
                                          dtype=torch.float16)
                    lin.weight = torch.nn.Parameter(child.dequantize().contiguous(), requires_grad=False)
                    setattr(parent, name, lin)
        return t.to(dtype)

    t16, t32 = twin(torch.float16), twin(torch.float32)
    ids = torch.randint(0, 512, (1, 9), generator=torch.Generator().manual_seed(1)).to(DEV)
    ours, g16, g32 = _lora_grads(model, ids), _lora_grads(t16, ids), _lora_grads(t32, ids)
    assert len(ours) == 8 and ours.keys() == g16.keys() == g32.keys()
    worst = []
    for n in ours:
        assert torch.isfinite(ours[n]).all() and ours[n].abs().max() > 0, n
        e_dense = ((g16[n] - g32[n]).norm() / g32[n].norm()).item()
        e_ours = ((ours[n] - g32[n]).norm() / g32[n].norm()).item()
        print(f"{n}: ours {e_ours:.3e}  fp16 dense twin {e_dense:.3e}")
        if e_ours > 2 * e_dense:
            worst.append((n, e_ours, e_dense))
    assert not worst, f"LoRA gradients beyond 2 x the dense fp16 twin's error: {worst}"
