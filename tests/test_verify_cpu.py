"""CPU: the composed routes of layer_ops.verify_step_streams and layer_ops.ngram_draft against
tests/verify_reference.py's numpy restatements, the hand-made drafter cases against that restatement,
and what generate / generate_ragged refuse before anything runs."""
import numpy as np
import pytest
import torch
from streams_reference import SENTINEL
from verify_reference import DRAFT_CASES, accept_case, crafted_logits, draft_rule, verify_feedback

KEYS = ("hist", "pos", "live", "stop", "limit", "tok", "accepted")


@pytest.mark.parametrize("T", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["fp32", "fp16", "bf16"])
def test_composed_pick_against_the_numpy_restatement(dtype, T):
    from quantizations_amd.layer_ops import verify_step_streams

    V = 300
    case, picks, accepted = accept_case(T, V, seed=T)
    want = verify_feedback(picks, *(case[k].numpy() for k in KEYS[:-1]))
    assert np.array_equal(want[4], accepted), "the case is built to accept these counts"
    for kw in ({}, dict(ties=True), dict(nan_rows=(0, 1, T, 2 * T + 1))):
        logits = crafted_logits(picks, V, dtype, seed=3, **kw)
        c = {k: v.clone() for k, v in case.items()}
        verify_step_streams(logits, *(c[k] for k in KEYS))
        for name, w in zip(("hist", "pos", "live", "tok", "accepted"), want):
            assert np.array_equal(c[name].numpy(), w), (kw, name)
        dead = T + 2
        assert c["tok"][dead].tolist() == [SENTINEL] * T and c["hist"][dead].tolist() == [SENTINEL] * c["hist"].shape[1]


def test_an_emitted_row_lies_inside_the_limit():
    """Random drafts, stops and limits: the restatement and the composed route agree, and every emitted
    row i has pos + i + 1 <= limit -- with limit <= L - 1, a row past a cache of L slots is never emitted."""
    from quantizations_amd.layer_ops import verify_step_streams

    rng = np.random.default_rng(0)
    B, T, V, H = 64, 4, 6, 32          # six tokens: drafts match often
    seen = set()
    for trial in range(20):
        picks = rng.integers(0, V, (B, T)).astype(np.int64)
        tok = rng.integers(0, V, (B, T)).astype(np.int64)
        right = rng.random((B, T - 1)) < 0.7                     # most drafts are the pick of the row before
        tok[:, 1:] = np.where(right, picks[:, :-1], tok[:, 1:])
        pos = rng.integers(0, H - 1, B).astype(np.int64)
        limit = np.minimum(pos + rng.integers(1, 2 * T, B), H - 1).astype(np.int64)
        live = (rng.random(B) < 0.8).astype(np.int32)
        stop = np.where(rng.random(B) < 0.5, rng.integers(0, V, B), -1).astype(np.int64)
        hist = np.full((B, H), SENTINEL, dtype=np.int64)
        want = verify_feedback(picks, hist, pos, live, stop, limit, tok)
        t = [torch.from_numpy(a.copy()) for a in (hist, pos, live, stop, limit, tok)]
        acc = torch.zeros(B, dtype=torch.int32)
        verify_step_streams(crafted_logits(picks, V, torch.float32, seed=trial), *t, acc)
        for got, w in zip((t[0], t[1], t[2], t[5], acc), want):
            assert np.array_equal(got.numpy(), w), trial
        n = acc.numpy()
        assert bool((n[live == 0] == 0).all()) and bool((n[live != 0] >= 1).all()) and bool((n <= T).all())
        assert bool((pos + n <= np.maximum(limit, pos + 1))[live != 0].all())   # pos + 1 > limit: one token, then out
        seen |= set(n.tolist())
    assert seen == set(range(T + 1)), "the trials reach every count"


@pytest.mark.parametrize("name", list(DRAFT_CASES))
def test_composed_drafter_on_crafted_histories(name):
    from quantizations_amd.layer_ops import ngram_draft

    s, ngram_max, T, want = DRAFT_CASES[name]
    p = len(s) - 1
    assert draft_rule(s, p, s[-1], T, ngram_max) == want
    hist = torch.full((2, len(s) + 2), SENTINEL, dtype=torch.int64)
    hist[0, :len(s)] = torch.tensor(s)
    hist[1, :3] = torch.tensor([2, 2, 2])
    tok = torch.full((2, T), SENTINEL, dtype=torch.int64)
    tok[:, 0] = torch.tensor([s[-1], 2])
    pos = torch.tensor([p, 2])
    ids = torch.zeros((2, T), dtype=torch.int64)
    ngram_draft(hist, pos, tok, ids, ngram_max)
    assert tok[0].tolist() == [s[-1]] + want and tok[1].tolist() == [2] * T
    assert ids.tolist() == [[p + i for i in range(T)], [2 + i for i in range(T)]]


def test_composed_drafter_on_random_histories():
    from quantizations_amd.layer_ops import ngram_draft

    rng = np.random.default_rng(1)
    T = 5
    for ngram_max in (1, 2, 3, 4):
        hists = [rng.integers(0, 2, 60).tolist() for _ in range(12)]
        ps = [int(rng.integers(0, 60)) for _ in hists]
        hist = torch.tensor(hists)
        tok = torch.zeros((12, T), dtype=torch.int64)
        tok[:, 0] = torch.tensor([h[p] for h, p in zip(hists, ps)])
        ids = torch.zeros((12, T), dtype=torch.int64)
        ngram_draft(hist, torch.tensor(ps), tok, ids, ngram_max)
        for b, (h, p) in enumerate(zip(hists, ps)):
            assert tok[b, 1:].tolist() == draft_rule(h, p, h[p], T, ngram_max), (ngram_max, b)


def test_generate_refuses_before_anything_runs():
    from transformers import LlamaConfig, LlamaForCausalLM

    from quantizations_amd.generation import generate, generate_ragged

    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=128, max_position_embeddings=64)
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).eval()
    ids = torch.randint(0, 128, (2, 5), generator=torch.Generator().manual_seed(0))
    with pytest.raises(ValueError, match="do_sample"):
        generate(model, ids, 4, do_sample=True, prompt_lookup_num_tokens=3)
    with pytest.raises(ValueError, match="do_sample"):
        generate_ragged(model, [ids[0], ids[1, :3]], 4, do_sample=True, prompt_lookup_num_tokens=3)
    with pytest.raises(ValueError, match="max_matching_ngram_size"):
        generate(model, ids, 4, max_matching_ngram_size=2)
    with pytest.raises(ValueError, match="max_matching_ngram_size"):
        generate_ragged(model, [ids[0]], 4, max_matching_ngram_size=2)
    with pytest.raises(ValueError, match="draft_tokens"):
        generate(model, ids, 4, prompt_lookup_num_tokens=0)
    with pytest.raises(ValueError, match="rows per step"):
        generate(model, ids, 4, prompt_lookup_num_tokens=8)            # 2 streams x 9 rows
    with pytest.raises(ValueError, match="ngram"):
        generate(model, ids, 4, prompt_lookup_num_tokens=3, max_matching_ngram_size=5)
    with pytest.raises(ValueError, match="HIP decode kernels"):
        generate(model, ids, 4, prompt_lookup_num_tokens=3)            # a CPU model: no torch fall-back
    assert generate(model, ids, 0, prompt_lookup_num_tokens=3).tolist() == ids.tolist()
    assert generate(model, ids, 3).shape == (2, 8)                     # unset: the plain path, unchanged
