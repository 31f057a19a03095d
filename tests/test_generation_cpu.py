"""CPU: generation.generate / DecodeSession on an unquantised fp32 tiny Llama, where no fused
numerics are involved: greedy tokens equal transformers' own generate() on every seeded prompt.
initializer_range 0.1 makes the attention sharp enough that a rotary position off by one changes
tokens on every prompt (at 0.02 it does on some).  On the CPU the step runs eagerly and the pick is
sample_step's torch route."""
import pytest
import torch

S, N = 8, 16


@pytest.fixture(scope="module")
def model():
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=512, max_position_embeddings=128, rope_theta=10000.0,
                      initializer_range=0.1, eos_token_id=None, bos_token_id=None, pad_token_id=None)
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg).eval()


@pytest.mark.parametrize("seed", range(10))
def test_greedy_generate_equals_transformers(model, seed):
    from quantizations_amd.generation import generate

    B = 1 if seed % 2 else 3
    ids = torch.randint(0, 512, (B, S), generator=torch.Generator().manual_seed(seed))
    with torch.no_grad():
        want = model.generate(ids, do_sample=False, max_new_tokens=N)
    got = generate(model, ids, N)
    assert got.shape == (B, S + N) and torch.equal(got, want)
    assert torch.equal(generate(model, ids, N, do_sample=True, temperature=0.0), want)


def test_session_positions_and_uniform_columns(model):
    """hist is the sequence, pos the position of the newest token; the token at index i is drawn with
    uniform[:, i - 1]: a hand-written loop with transformers' positions gives the same tokens."""
    from transformers.cache_utils import DynamicCache

    from quantizations_amd.generation import DecodeSession
    from quantizations_amd.layer_ops import sample_step

    B = 2
    ids = torch.randint(0, 512, (B, S), generator=torch.Generator().manual_seed(77))
    sess = DecodeSession(model, B, S + N)
    sess.set_sampling(temperature=[0.9, 1.3], top_k=[20, 0], top_p=[1.0, 0.8])
    sess.seed(torch.Generator().manual_seed(5))
    sess.prefill(ids)
    assert int(sess.pos) == S
    for _ in range(N - 1):
        sess.step()
    assert int(sess.pos) == S + N - 1 and torch.equal(sess.tok[:, 0], sess.hist[:, -1])
    with pytest.raises(ValueError):
        sess.step()
    U = torch.rand((B, S + N), generator=torch.Generator().manual_seed(5))
    assert torch.equal(sess.uniform, U)
    T, K, P = sess.temperature, sess.top_k, sess.top_p
    seq = ids.clone()
    cache = DynamicCache()
    with torch.no_grad():
        logits = model(input_ids=seq, past_key_values=cache, use_cache=True).logits[:, -1]
        for i in range(S, S + N):                     # the token at index i
            h = torch.zeros((B, 1), dtype=torch.int64)
            t = torch.zeros(B, dtype=torch.int64)
            sample_step(logits, h, torch.zeros(1, dtype=torch.int64), t, T, K, P, U[:, i - 1:i].contiguous())
            seq = torch.cat([seq, t[:, None]], 1)
            logits = model(input_ids=t[:, None], past_key_values=cache, use_cache=True).logits[:, -1]   # position i
    assert torch.equal(sess.hist, seq)
