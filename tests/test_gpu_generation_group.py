"""GPU: a model with 16 query heads per kv head in the sessions.  A two-layer LlamaForCausalLM (hidden 256, D 64, 16
query heads on 1 kv head) has no launch among the one-head-per-workgroup attentions; its step, verify window and
prefill windows run on layer_ops.attention_group.  The reference is the model's eager fp32 forward on the dequantised
weights, teacher-forced over the product's sequences; the bar is twice the error of a plain fp16 torch twin of that
reference on the same rows (test_gpu_product_geometry.py's method).  A 4-on-2 model checks the opt-in route on the
same bar and that the default route keeps its launches."""
import pytest
import torch

from test_gpu_generation_speculative import _unprepare
from test_gpu_product_geometry import _census, _count_entry_points

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
NEW, LENGTHS = 40, (5, 37, 90)


def _build(heads, kv, dtype=torch.float16, quantised=True, attn="sdpa"):
    from transformers import LlamaConfig, LlamaForCausalLM

    from quantizations_amd.integration import replace_with_bnb_linear

    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=heads,
                      num_key_value_heads=kv, head_dim=64, vocab_size=4096, max_position_embeddings=256,
                      rope_theta=500000.0, eos_token_id=None, bos_token_id=None, pad_token_id=None,
                      attn_implementation=attn)
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).to(dtype).to(DEV).eval()
    if quantised:
        replace_with_bnb_linear(model, modules_to_not_convert=["lm_head"], quant_type="nf4", compute_dtype=torch.float32)
    return model


def _prompts():
    g = torch.Generator().manual_seed(3)
    return [torch.randint(0, 4096, (n,), generator=g).to(DEV) for n in LENGTHS]


@pytest.fixture()
def prepared(request):
    import quantizations_amd as qa
    from quantizations_amd.generation import prepare_for_decode

    heads, kv = request.param
    model = _build(heads, kv)
    state = {n: p.detach().float() for n, p in model.named_parameters() if p.dtype.is_floating_point}
    for name, m in model.named_modules():
        if isinstance(m, qa.Linear4bit):                   # the reference's weights: what the 4-bit codes stand for
            state[name + ".weight"] = qa.dequantize_4bit(m.weight, m.weight.quant_state, out_dtype=torch.float32).t()
    prepare_for_decode(model)
    yield model, state, (heads, kv)
    _unprepare(model)


def _check(out, state, heads_kv):
    ref, twin = (_build(*heads_kv, dt, quantised=False, attn="eager") for dt in (torch.float32, torch.float16))
    ref.load_state_dict(state), twin.load_state_dict(state)
    with torch.no_grad():
        for b, (seq, lp) in enumerate(zip(out.sequences, out.logprobs)):
            S = LENGTHS[b]
            assert seq.numel() == S + NEW
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


@pytest.mark.parametrize("how", [{}, {"prefill_chunk": 16}, {"prompt_lookup_num_tokens": 3},
                                 {"prompt_lookup_num_tokens": 3, "prefill_chunk": 16}],
                         ids=["whole-prompt", "chunked", "speculative", "speculative-chunked"])
@pytest.mark.parametrize("prepared", [(16, 1)], indirect=True, ids=["G16"])
def test_sixteen_heads_per_kv_head_match_the_fp32_reference(prepared, how, monkeypatch):
    from quantizations_amd.generation import generate_ragged

    model, state, heads_kv = prepared
    calls = _count_entry_points(monkeypatch)
    out = generate_ragged(model, _prompts(), NEW, logprobs=0, **how)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert calls.get("qz_attention_group", 0) > 0 and not any(k.startswith("qz_decode_attention") for k in calls), calls
    _unprepare(model)                                        # the reference runs transformers' own functions
    _check(out, state, heads_kv)


@pytest.mark.parametrize("speculative", [False, True], ids=["stream", "speculative"])
@pytest.mark.parametrize("prepared", [(4, 2)], indirect=True, ids=["G4"])
def test_the_group_route_by_request(prepared, speculative, monkeypatch):
    """attention_route="group": the 4-on-2 model's step / verify window and prefill windows leave their own launches
    for the group launch, on the same bar."""
    from quantizations_amd import generation as G

    model, state, heads_kv = prepared
    prompts = _prompts()
    ids = torch.zeros((3, max(LENGTHS)), dtype=torch.int64, device=DEV)
    for b, p in enumerate(prompts):
        ids[b, :p.numel()] = p
    kind = G.SpeculativeSession if speculative else G.StreamSession
    sess = kind(model, 3, max(LENGTHS) + NEW, logprobs=0, prefill_chunk=16, attention_route="group")
    calls = _count_entry_points(monkeypatch)
    sess.prefill(ids, list(LENGTHS), max_new_tokens=NEW)
    if speculative:
        G._run_speculative(sess, NEW)
    else:
        for _ in range(NEW - 1):
            sess.step()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert calls.get("qz_attention_group", 0) > 0, calls
    assert not any("attention" in k and k != "qz_attention_group" for k in calls), calls
    out = G._ragged_output(sess)
    _unprepare(model)
    _check(out, state, heads_kv)


def test_the_default_route_keeps_its_launches(monkeypatch):
    from quantizations_amd.generation import StreamSession, prepare_for_decode

    model = _build(4, 2)
    prepare_for_decode(model)
    small = [p[:n] for p, n in zip(_prompts(), (5, 37, 80))]
    counts = _census(model, monkeypatch, 3, small)
    assert counts["qz_decode_attention_streams"] == 2 and "qz_attention_group" not in counts, counts
    with pytest.raises(ValueError, match="attention_route"):
        StreamSession(model, 2, 64, attention_route="tiles")
    with pytest.raises(ValueError, match="flat cache"):
        StreamSession(model, 2, 64, prefill_chunk=16, kv_pages=4, attention_route="group")
    _unprepare(model)
