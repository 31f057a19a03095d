"""CPU: tests/llama_reference.py against transformers' LlamaForCausalLM in fp64, on two toy configs
(G = 1; G = 4 with D = 16, which is not hidden / heads) and ragged rows, to 1e-10 on log-probabilities.

transformers pins three of its ops to fp32 whatever the model's dtype: LlamaRotaryEmbedding (inverse
frequencies, cos / sin), LlamaRMSNorm (the variance) and the eager attention's softmax.  A .double() model
therefore sits 7e-8 from any true fp64 computation (measured here before the replacements), not 1e-10.  The
model under comparison gets fp64 modules for the first two, written here from their formulas (theta^(-2i/D)
with duplicated halves; x rsqrt(mean x^2 + eps) w) and not taken from llama_reference, and runs its sdpa
attention, whose softmax on the CPU is in the tensors' dtype.  What the 1e-10 comparison holds against
transformers is the composition: the half-split pairing (rotate_half), which kv head a query head reads
(repeat_kv), the causal mask, the residual order, the MLP, the lm_head rows.  The two replaced formulas -- the
rotary frequencies and where eps sits in the norm -- are held against transformers' own modules by a second
comparison with the unmodified .double() model (eager attention), to LOOSE = 1e-6: an order of magnitude above
the 7e-8 its fp32 islands cost, and far below what a wrong theta, a wrong pairing or a misplaced eps moves."""
import pytest
import torch

import llama_reference as LR

TOL = 1e-10
LOOSE = 1e-6        # against the unmodified model: its fp32 rotary, norm variance and softmax cost 7e-8
LENGTHS = [1, 7, 19, 12]

CONFIGS = {
    "g1": dict(hidden_size=64, intermediate_size=96, num_hidden_layers=2, num_attention_heads=4,
               num_key_value_heads=4, vocab_size=97),
    "g4_d16": dict(hidden_size=96, intermediate_size=160, num_hidden_layers=3, num_attention_heads=8,
                   num_key_value_heads=2, head_dim=16, vocab_size=131),
}


class Norm64(torch.nn.Module):
    def __init__(self, weight, eps):
        super().__init__()
        self.weight, self.eps = weight, eps

    def forward(self, x):
        return self.weight * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.eps))


class Rotary64(torch.nn.Module):
    def __init__(self, D, theta):
        super().__init__()
        self.inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float64) / D))

    def forward(self, x, position_ids):
        f = position_ids.to(torch.float64)[:, :, None] * self.inv[None, None, :]
        emb = torch.cat((f, f), -1)
        return emb.cos(), emb.sin()


@pytest.fixture(scope="module", params=list(CONFIGS))
def pair(request):
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(**CONFIGS[request.param], rope_theta=500000.0, rms_norm_eps=1e-5, max_position_embeddings=64,
                      tie_word_embeddings=False, attn_implementation="sdpa")
    torch.manual_seed(11)
    model = LlamaForCausalLM(cfg).double().eval()
    with torch.no_grad():
        for name, p in model.named_parameters():      # norms away from 1, so a dropped weight shows
            if "norm" in name:
                p.copy_(1.0 + 0.3 * torch.randn_like(p))
    g = torch.Generator().manual_seed(5)
    rows = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in LENGTHS]
    model.config._attn_implementation = "eager"       # transformers as it is: its own rotary, norms and softmax
    with torch.no_grad():
        stock = [torch.log_softmax(model(input_ids=r[None]).logits[0], -1) for r in rows]
    model.config._attn_implementation = "sdpa"
    D = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
    model.model.rotary_emb = Rotary64(D, 500000.0)
    model.model.norm = Norm64(model.model.norm.weight, cfg.rms_norm_eps)
    for layer in model.model.layers:
        layer.input_layernorm = Norm64(layer.input_layernorm.weight, cfg.rms_norm_eps)
        layer.post_attention_layernorm = Norm64(layer.post_attention_layernorm.weight, cfg.rms_norm_eps)
    with torch.no_grad():
        want = [torch.log_softmax(model(input_ids=r[None]).logits[0], -1) for r in rows]
    assert want[0].dtype == torch.float64
    return cfg, dict(model.state_dict()), rows, want, stock


def test_every_position_matches_transformers_fp64(pair):
    cfg, weights, rows, want, _ = pair
    got = LR.logprobs(weights, cfg, rows, [range(len(r)) for r in rows])
    worst = 0.0
    for g, w in zip(got, want):
        assert g.dtype == torch.float64 and g.shape == w.shape
        worst = max(worst, float((g - w).abs().max()))
    print(f"largest |log-probability difference| to transformers fp64: {worst:.3e}")
    assert worst <= TOL


def test_every_position_is_near_the_unmodified_transformers_model(pair):
    """transformers' own rotary table and RMSNorm (and eager softmax), fp32 islands included: LOOSE, not TOL."""
    cfg, weights, rows, _, stock = pair
    got = LR.logprobs(weights, cfg, rows, [range(len(r)) for r in rows])
    worst = max(float((g - w).abs().max()) for g, w in zip(got, stock))
    print(f"largest |log-probability difference| to the unmodified transformers model: {worst:.3e}")
    assert 1e-12 < worst <= LOOSE       # above 1e-12: the stock modules did run


def test_requested_positions_only_and_narrow_tables(pair):
    """A subset of positions gives those rows; fp32 embedding / lm_head tables cast on use are the tables cast first."""
    cfg, weights, rows, _, _ = pair
    at = [[0], [6, 2], [18, 0, 9], [11]]
    full = LR.logprobs(weights, cfg, rows, [range(len(r)) for r in rows])
    some = LR.logprobs(weights, cfg, rows, at)
    for f, s, a in zip(full, some, at):
        assert s.shape[0] == len(a) and float((s - f[list(a)]).abs().max()) <= 1e-13   # BLAS blocks by row count
    w32 = dict(weights)
    for name in ("model.embed_tokens.weight", "lm_head.weight"):
        w32[name] = weights[name].float()
    w64 = dict(w32)
    for name in ("model.embed_tokens.weight", "lm_head.weight"):
        w64[name] = w32[name].double()
    for a, b in zip(LR.logprobs(w32, cfg, rows, at), LR.logprobs(w64, cfg, rows, at)):
        assert torch.equal(a, b)


def test_head_row_blocks_do_not_change_the_result(pair, monkeypatch):
    cfg, weights, rows, _, _ = pair
    at = [[len(r) - 1] for r in rows]
    whole = LR.logprobs(weights, cfg, rows, at)
    monkeypatch.setattr(LR, "HEAD_ROWS", 40)          # not a divisor of either vocabulary
    for a, b in zip(LR.logprobs(weights, cfg, rows, at), whole):
        assert float((a - b).abs().max()) <= 1e-13


def test_identity_kv_round_changes_nothing(pair):
    cfg, weights, rows, _, _ = pair
    at = [range(len(r)) for r in rows]
    seen = []

    def same(k, v):
        seen.append((tuple(k.shape), tuple(v.shape)))
        return k, v

    plain = LR.logprobs(weights, cfg, rows, at)
    for a, b in zip(LR.logprobs(weights, cfg, rows, at, kv_round=same), plain):
        assert torch.equal(a, b)
    D = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
    want = [((len(r), cfg.num_key_value_heads, D),) * 2 for r in rows for _ in range(cfg.num_hidden_layers)]
    assert seen == want


def test_kv_round_reaches_the_attention(pair):
    """A hook that does change the rows changes the result (position 0 aside: one key, softmax = 1, v scaled)."""
    cfg, weights, rows, _, _ = pair
    at = [[len(r) - 1] for r in rows]
    plain = LR.logprobs(weights, cfg, rows, at)
    bent = LR.logprobs(weights, cfg, rows, at, kv_round=lambda k, v: (k * 1.01, v))
    assert torch.equal(bent[0], plain[0])            # one key: the scores do not matter
    assert all(float((a - b).abs().max()) > 1e-8 for a, b in zip(bent[1:], plain[1:]))


def test_traces_name_every_layer(pair):
    cfg, weights, rows, _, _ = pair
    traces = []
    LR.logprobs(weights, cfg, rows[:2], [[0], [3]], traces=traces)
    names = [n for n, _ in traces[1]]
    want = ["embed"] + [f"layer{i}.{s}" for i in range(cfg.num_hidden_layers) for s in ("attn", "mid", "out")] + ["norm"]
    assert names == want and all(t.shape[0] == len(rows[1]) for _, t in traces[1])
