"""GPU: Mistral in the sessions.  A two-layer MistralForCausalLM (hidden 256, D 64): with sliding_window=40 it runs in
a StreamSession over a RingKVCache, with sliding_window=None it takes a Llama's launches.  The reference is the model's
eager fp32 forward on the dequantised weights, teacher-forced over the product's sequences; the bar is twice the error of
a plain fp16 torch twin of that reference on the same rows (test_gpu_product_geometry.py's method)."""
import pytest
import torch

from test_gpu_generation_speculative import _build as _build_llama
from test_gpu_generation_speculative import _unprepare
from test_gpu_product_geometry import _census

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
W, NEW, LENGTHS = 40, 60, (5, 37, 90)


def _build(window, dtype=torch.float16, quantised=True, attn="sdpa"):
    from transformers import MistralConfig, MistralForCausalLM

    from quantizations_amd.integration import replace_with_bnb_linear

    cfg = MistralConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                        num_key_value_heads=2, head_dim=64, vocab_size=4096, max_position_embeddings=256,
                        rope_theta=500000.0, sliding_window=window, eos_token_id=None, bos_token_id=None,
                        pad_token_id=None, attn_implementation=attn)
    torch.manual_seed(0)
    model = MistralForCausalLM(cfg).to(dtype).to(DEV).eval()
    if quantised:
        replace_with_bnb_linear(model, modules_to_not_convert=["lm_head"], quant_type="nf4", compute_dtype=torch.float32)
    return model


def _prompts():
    g = torch.Generator().manual_seed(3)
    return [torch.randint(0, 4096, (n,), generator=g).to(DEV) for n in LENGTHS]


@pytest.fixture()
def windowed():
    import quantizations_amd as qa
    from quantizations_amd.generation import prepare_for_decode

    model = _build(W)
    state = {n: p.detach().float() for n, p in model.named_parameters() if p.dtype.is_floating_point}
    for name, m in model.named_modules():
        if isinstance(m, qa.Linear4bit):                   # the reference's weights: what the 4-bit codes stand for
            state[name + ".weight"] = qa.dequantize_4bit(m.weight, m.weight.quant_state, out_dtype=torch.float32).t()
    prepare_for_decode(model)
    yield model, state
    _unprepare(model)


def test_ragged_streams_past_the_window_match_the_fp32_reference(windowed):
    from quantizations_amd.generation import generate_ragged

    model, state = windowed
    out = generate_ragged(model, _prompts(), NEW, logprobs=0, prefill_chunk=16)      # a ring of 128 slots
    torch.cuda.synchronize()
    _unprepare(model)                                        # the reference runs transformers' own functions
    ref, twin = (_build(W, dt, quantised=False, attn="eager") for dt in (torch.float32, torch.float16))
    ref.load_state_dict(state), twin.load_state_dict(state)
    with torch.no_grad():
        for b, (seq, lp) in enumerate(zip(out.sequences, out.logprobs)):
            S = LENGTHS[b]
            assert seq.numel() == S + NEW > W                # every stream passes the window; the longest laps the ring
            r = torch.log_softmax(ref(input_ids=seq[None]).logits[0].double(), -1)[S - 1:-1]     # the rows that picked
            t = torch.log_softmax(twin(input_ids=seq[None]).logits[0].double(), -1)[S - 1:-1]
            nxt = seq[S:, None]
            e_twin = (t.gather(1, nxt) - r.gather(1, nxt)).abs().max().item()
            e_prod = (lp[S:].double() - r.gather(1, nxt)[:, 0]).abs().max().item()
            print(f"stream {b}: product {e_prod:.3e}, fp16 twin {e_twin:.3e}")
            assert e_prod <= 2 * e_twin
            top = r.topk(2, -1)
            sure = (top.values[:, 0] - top.values[:, 1]) > 2 * e_twin
            assert torch.equal(top.indices[sure, 0], seq[S:][sure])


def test_mistral_without_a_window_takes_llamas_launches(monkeypatch):
    from quantizations_amd.generation import prepare_for_decode

    small = [p[:n] for p, n in zip(_prompts(), (5, 37, 80))]
    counts = []
    for model in (_build(None), _build_llama()):
        prepare_for_decode(model)
        counts.append(_census(model, monkeypatch, 1, small))
        _unprepare(model)
    assert counts[0] == counts[1] and counts[0]["qz_decode_attention"] == 2, counts


@pytest.mark.parametrize("open_it", ["decode", "speculative", "kv_pages", "fp8"])
def test_what_cannot_serve_a_window_says_so(windowed, open_it):
    from quantizations_amd.generation import DecodeSession, SpeculativeSession, StreamSession

    windowed = windowed[0]
    with pytest.raises(ValueError, match="sliding-window model.*StreamSession"):
        {"decode": lambda: DecodeSession(windowed, 1, 64),
         "speculative": lambda: SpeculativeSession(windowed, 2, 64),
         "kv_pages": lambda: StreamSession(windowed, 2, 64, prefill_chunk=64, kv_pages=4),
         "fp8": lambda: StreamSession(windowed, 2, 64, prefill_chunk=64, kv_pages=4, kv_dtype="fp8")}[open_it]()
