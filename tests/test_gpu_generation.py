"""GPU: quantizations_amd.generation -- prepare_for_decode, DecodeSession and generate() on a tiny
random-init Llama (2 layers, hidden 256, vocab 4096) with Linear4bit projections: greedy tokens
against transformers' own generate() on the unfused model and against an eager greedy_step loop;
sampled tokens of the captured step against the same step run eagerly and against a hand-written
loop around layer_ops.sample_step (same seeded uniform numbers, so this checks the capture
plumbing, not the sampler: test_gpu_sampling.py does that).

The hand-written loops follow bench.py's convention, independently of the session: `pos` is the position
of the token being fed, the pick of that step is the token at pos + 1 and is drawn with uniform[:, pos]."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
S, N = 8, 24


def _unprepare(model):
    from quantizations_amd import integration as I

    I.unfuse_lm_head(model)
    I.unfuse_decode_glue(model)
    I.unfuse_prenorm(model)
    I.unfuse_layer_ops(model)
    I.unfuse_projection_groups(model)
    model.__dict__.pop("_qz_prepared", None)


@pytest.fixture(scope="module")
def tiny():
    """(prepared model, prompts [3, S], transformers' greedy continuation of the unfused model for
    the first 1 and all 3 prompts, prepare_for_decode's counts)"""
    from transformers import LlamaConfig, LlamaForCausalLM

    from quantizations_amd.generation import prepare_for_decode
    from quantizations_amd.integration import replace_with_bnb_linear

    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=4096, max_position_embeddings=256, rope_theta=500000.0,
                      eos_token_id=None, bos_token_id=None, pad_token_id=None)   # generate() runs to the length
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).half().to(DEV).eval()
    replace_with_bnb_linear(model, modules_to_not_convert=["lm_head"], quant_type="nf4", compute_dtype=torch.float32)
    ids = torch.randint(0, 4096, (3, S), generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        hf = {B: model.generate(ids[:B], do_sample=False, max_new_tokens=N) for B in (1, 3)}
    counts = prepare_for_decode(model)
    try:
        yield model, ids, hf, counts
    finally:
        _unprepare(model)


def _hand_loop(model, ids, n, pick):
    """bench.decode_bench_graph's loop, eager: the prompt, then n - 1 steps that feed `tok` at position
    `pos`; pick(logits [B, V], picked, pos, tok) writes picked[:, pos], tok and pos += 1, so picked[:, p]
    is the token at sequence index p + 1.  Returns the sequence [B, s + n]."""
    from transformers.cache_utils import StaticCache

    B, s = ids.shape
    cache = StaticCache(config=model.config, max_cache_len=s + n + 2)
    picked = torch.zeros((B, s + n), dtype=torch.int64, device=DEV)
    pos = torch.tensor([s - 1], device=DEV)          # the last prompt token was fed at s - 1
    tok = torch.zeros((B, 1), dtype=torch.int64, device=DEV)
    pos_ids = pos.view(1, 1).expand(B, 1)
    with torch.inference_mode():
        out = model(input_ids=ids, past_key_values=cache, cache_position=torch.arange(s, device=DEV), use_cache=True)
        pick(out.logits[:, -1], picked, pos, tok)
        for _ in range(n - 1):
            assert int(pos) == s + _                  # the fed token's sequence index, as transformers positions it
            lo = model(input_ids=tok, past_key_values=cache, cache_position=pos, position_ids=pos_ids,
                       use_cache=True).logits
            pick(lo[:, -1], picked, pos, tok)
    return torch.cat([ids, picked[:, s - 1:s + n - 1]], 1)


@pytest.mark.parametrize("B", [1, 3])
def test_greedy_generate_equals_transformers_and_the_eager_loop(tiny, B):
    from quantizations_amd.generation import generate
    from quantizations_amd.layer_ops import greedy_step

    model, ids, hf, _ = tiny
    out = generate(model, ids[:B], N)
    assert out.dtype == torch.int64 and out.shape == (B, S + N)
    assert torch.equal(out, hf[B])
    assert torch.equal(out, _hand_loop(model, ids[:B], N, greedy_step))
    assert torch.equal(out, generate(model, ids[:B], N, graph=False))


def test_sampled_generate_graph_equals_eager_and_a_hand_loop(tiny):
    from quantizations_amd.generation import generate
    from quantizations_amd.layer_ops import sample_step

    model, ids, _, _ = tiny
    B = 3
    kw = dict(do_sample=True, temperature=[0.0, 0.8, 1.2], top_k=[0, 50, 0], top_p=[1.0, 0.9, 0.95], generator=1234)
    out = generate(model, ids, N, **kw)
    assert torch.equal(out, generate(model, ids, N, graph=False, **kw))
    T = torch.tensor(kw["temperature"], device=DEV)
    K = torch.tensor(kw["top_k"], dtype=torch.int32, device=DEV)
    P = torch.tensor(kw["top_p"], device=DEV)
    U = torch.rand((B, S + N), generator=torch.Generator(device=DEV).manual_seed(1234), device=DEV)
    hand = _hand_loop(model, ids, N, lambda lo, hist, pos, tok: sample_step(lo, hist, pos, tok.view(-1), T, K, P, U))
    assert torch.equal(out, hand)
    # per-stream settings: the cold stream is the greedy one, the others left it somewhere
    greedy = generate(model, ids, N)
    assert torch.equal(out[0], greedy[0])
    assert not torch.equal(out[1], greedy[1]) and not torch.equal(out[2], greedy[2])
    # another seed, other tokens
    assert not torch.equal(out, generate(model, ids, N, **{**kw, "generator": 99}))


def test_set_sampling_after_capture_changes_the_next_replay(tiny):
    from quantizations_amd.generation import DecodeSession

    model, ids, _, _ = tiny

    def run(graph, change):
        sess = DecodeSession(model, 3, S + 12, graph=graph)
        sess.set_sampling(temperature=0.9, top_k=40, top_p=0.95)
        sess.seed(7)
        sess.prefill(ids)
        for _ in range(4):
            sess.step()
        if change:
            sess.set_sampling(temperature=[0.0, 0.0, 1.5], top_k=0, top_p=[1.0, 1.0, 0.5])
        for _ in range(6):
            sess.step()
        torch.cuda.synchronize()
        assert int(sess.pos.item()) == S + 10
        return sess.hist.clone()

    a, b, c = run(True, True), run(False, True), run(True, False)
    assert torch.equal(a, b)
    assert torch.equal(a[:, :S + 5], c[:, :S + 5]) and not torch.equal(a, c)
    sess = DecodeSession(model, 3, S + 2)
    sess.prefill(ids)
    sess.step()
    with pytest.raises(ValueError):
        sess.step()                           # the history is full
    with pytest.raises(ValueError):
        sess.set_sampling(temperature=0.7)    # captured greedy-only


def test_eos_stops_and_pads(tiny):
    from quantizations_amd.generation import generate

    model, ids, _, _ = tiny
    n = 40
    free, free1 = generate(model, ids, n), generate(model, ids[:1], n)
    # one stream: it stops at the first host check after its EOS (every 16 steps) and is padded with it
    eos = int(free1[0, S + 5])
    first = int((free1[0, S:] == eos).nonzero()[0])
    out = generate(model, ids[:1], n, eos_token_id=eos)
    assert out.shape == (1, S + 16) and first <= 5
    assert torch.equal(out[0, :S + first + 1], free1[0, :S + first + 1]) and bool((out[0, S + first:] == eos).all())
    # three streams: each padded after its own first EOS; no early return while one has none
    out3 = generate(model, ids, n, eos_token_id=eos)
    hit = [(free[b, S:] == eos).nonzero() for b in range(3)]
    stop_all = max(int(h[0]) if h.numel() else n for h in hit)
    want_len = n if stop_all >= n else min(n, -(-(stop_all + 1) // 16) * 16)
    assert out3.shape == (3, S + want_len)
    for b in range(3):
        f = int(hit[b][0]) if hit[b].numel() else n
        assert torch.equal(out3[b, :S + min(f + 1, want_len)], free[b, :S + min(f + 1, want_len)])
        assert bool((out3[b, S + f:] == eos).all())


def test_padded_attention_mask_raises(tiny):
    from quantizations_amd.generation import DecodeSession, generate

    model, ids, _, _ = tiny
    mask = torch.ones_like(ids)
    assert generate(model, ids, 2, attention_mask=mask).shape == (3, S + 2)
    mask[1, 0] = 0
    with pytest.raises(ValueError):
        generate(model, ids, 2, attention_mask=mask)
    with pytest.raises(ValueError):
        DecodeSession(model, 3, S + 4).prefill(ids, attention_mask=mask)


def test_prepare_for_decode_is_idempotent(tiny):
    from quantizations_amd.generation import prepare_for_decode

    model, _, _, counts = tiny
    assert counts["groups"] == 4 and counts["layer_ops"] > 0 and counts["prenorm"] > 0 and counts["glue"] > 0
    before = {name: (m.__dict__.get("forward"), m.__dict__.get("_qz_group")) for name, m in model.named_modules()}
    assert prepare_for_decode(model) == counts
    after = {name: (m.__dict__.get("forward"), m.__dict__.get("_qz_group")) for name, m in model.named_modules()}
    assert all(after[k][0] is before[k][0] and after[k][1] is before[k][1] for k in before)


def test_exports():
    import quantizations_amd as qa
    from quantizations_amd import generation

    assert qa.generate is generation.generate and qa.DecodeSession is generation.DecodeSession
    assert qa.prepare_for_decode is generation.prepare_for_decode
