"""GPU: Mixtral in the sessions.  A two-layer MixtralForCausalLM wide enough for the one-token expert GEMVs (hidden 2048,
intermediate 2048, 8 experts, top-2, 16 heads of 128, 4 kv heads) runs in StreamSession / generate_ragged under each
SparseMoe4bit.decode_route, once with sliding_window=40 over the ring cache.  The reference is the model in fp64 on the
dequantised weights, teacher-forced over the product's sequences; the bar is twice the error of the dense fp16 twin on
the same weights (test_gpu_moe.py::test_module_in_a_mixtral_model's method)."""
import copy

import pytest
import torch

from test_gpu_generation_speculative import _unprepare
from test_gpu_product_geometry import _count_entry_points

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
NEW, LENGTHS, LAYERS = 24, (37, 5, 50), 2


@pytest.fixture(scope="module")
def trio():
    """(dense fp16 twin, its fp64 copy, the quantised model); the first two carry the dequantised weights."""
    import quantizations_amd as qa
    from quantizations_amd.integration import replace_with_bnb_linear
    from quantizations_amd.moe import SparseMoe4bit
    from transformers import MixtralConfig, MixtralForCausalLM

    cfg = MixtralConfig(hidden_size=2048, intermediate_size=2048, num_local_experts=8, num_experts_per_tok=2,
                        num_attention_heads=16, num_key_value_heads=4, head_dim=128, num_hidden_layers=LAYERS,
                        vocab_size=512, max_position_embeddings=256, sliding_window=None, eos_token_id=None,
                        bos_token_id=None, pad_token_id=None, attn_implementation="eager",
                        experts_implementation="eager")
    torch.manual_seed(0)
    dense = MixtralForCausalLM(cfg).half().to(DEV).eval()
    model = qa.replace_moe_blocks(replace_with_bnb_linear(copy.deepcopy(dense), modules_to_not_convert=["lm_head"]))
    model.config._attn_implementation = "sdpa"
    for name, m in model.named_modules():
        if isinstance(m, qa.Linear4bit):
            dense.get_submodule(name).weight.data.copy_(m.dequantize())
        elif isinstance(m, SparseMoe4bit):
            ex = dense.get_submodule(name).experts
            for pn in ("gate_up_proj", "down_proj"):
                p = getattr(m, pn)
                getattr(ex, pn).data.copy_(qa.dequantize_4bit(p, p.quant_state).t().reshape(getattr(ex, pn).shape))
    return dense, copy.deepcopy(dense).double(), model


@pytest.mark.parametrize("route, window, B", [("mma", None, 1), ("gemv", None, 1), ("mma", None, 3), ("gemv", None, 3),
                                              ("gemv", 40, 3)])
def test_streams_match_the_fp64_model(trio, monkeypatch, route, window, B):
    from quantizations_amd.generation import StreamSession, generate_ragged, prepare_for_decode
    from quantizations_amd.moe import SparseMoe4bit

    dense, exact, model = trio
    for m in trio:
        monkeypatch.setattr(m.config, "sliding_window", window)
    blocks = [m for m in model.modules() if isinstance(m, SparseMoe4bit)]
    for blk in blocks:
        monkeypatch.setattr(blk, "decode_route", route)
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, 512, (n,), generator=g).to(DEV) for n in LENGTHS][:B]
    counts = prepare_for_decode(model)
    try:
        assert len(blocks) == LAYERS and all("_qz_residual_decoder" in layer.__dict__ for layer in model.model.layers), counts
        out = generate_ragged(model, prompts, NEW, logprobs=0, prefill_chunk=16 if window else None)
        if B == 1:   # one eager step: which expert launches a one-row step takes
            with monkeypatch.context() as mp:
                sess = StreamSession(model, 1, 64, graph=False)
                sess.prefill(prompts[0][None], [LENGTHS[0]], max_new_tokens=4)
                sess.step()
                calls = _count_entry_points(mp)
                sess.step()
            took = [calls.get(f"qz_moe_{k}_4bit", 0) for k in ("gemv_pair_silu", "gemv_down", "pair_silu", "down")]
            assert took == ([LAYERS, LAYERS, 0, 0] if route == "gemv" else [0, 0, LAYERS, LAYERS]), calls
        torch.cuda.synchronize()
    finally:
        _unprepare(model)                                    # the references run transformers' own functions
    with torch.no_grad():
        for b, (seq, lp) in enumerate(zip(out.sequences, out.logprobs)):
            S = LENGTHS[b]
            assert seq.numel() == S + NEW
            r = torch.log_softmax(exact(input_ids=seq[None]).logits[0], -1)[S - 1:-1]            # the rows that picked
            t = torch.log_softmax(dense(input_ids=seq[None]).logits[0].double(), -1)[S - 1:-1]
            nxt = seq[S:, None]
            e_twin = (t.gather(1, nxt) - r.gather(1, nxt)).abs().max().item()
            e_prod = (lp[S:].double() - r.gather(1, nxt)[:, 0]).abs().max().item()
            print(f"{route} W={window} B={B} stream {b}: product {e_prod:.3e}, fp16 twin {e_twin:.3e}")
            assert e_prod <= 2 * e_twin
            top = r.topk(2, -1)
            sure = (top.values[:, 0] - top.values[:, 1]) > 2 * e_twin
            assert torch.equal(top.indices[sure, 0], seq[S:][sure])
