"""A plain fp64 Llama, written from the architecture's definition: the yardstick of
test_gpu_product_geometry.py.  Nothing of quantizations_amd or transformers.models is imported; the only
arithmetic is torch's own fp64 (matmul, softmax, rsqrt, cos / sin), on whichever device the weights are on.

Weights: a dict under the checkpoint names of a Llama (`model.embed_tokens.weight`,
`model.layers.{i}.input_layernorm.weight`, `...self_attn.{q,k,v,o}_proj.weight`,
`...post_attention_layernorm.weight`, `...mlp.{gate,up,down}_proj.weight`, `model.norm.weight`,
`lm_head.weight`), fp64.  The two vocabulary-sized tables may stay in a narrower dtype: the embedding rows
that are looked up and the lm_head row blocks that are multiplied are cast to fp64 where they are used, which
is the same number as casting the whole table first (a cast to fp64 is exact).

Config: anything with the attributes hidden_size, num_attention_heads, num_key_value_heads,
num_hidden_layers, rms_norm_eps, rope_theta and, optionally, head_dim.

The ops, in order: embedding; per layer RMSNorm (x * rsqrt(mean(x^2) + eps) * w), q / k / v projections,
half-split rotary (element i pairs with i + D/2; angle = position * theta^(-2i/D), all in fp64), causal
grouped-query attention (query head h reads kv head h // G, G = heads / kv heads; scores scaled by
D^-1/2; an fp64 softmax), o projection, residual, RMSNorm, SiLU(gate) * up, down projection, residual;
the final RMSNorm; the lm_head and log_softmax, on the requested rows only."""
import math
from typing import Callable, Optional, Sequence

import torch

F64 = torch.float64
HEAD_ROWS = 16384      # lm_head rows cast and multiplied at a time


def _get(cfg, name, default=None):
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name, default)


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w.to(F64)


def rotary_angles(positions: torch.Tensor, D: int, theta: float):
    """cos, sin [S, D/2] in fp64 for integer positions [S]."""
    i = torch.arange(0, D, 2, dtype=F64, device=positions.device)
    inv = torch.exp(-(i / D) * math.log(theta))
    ang = positions.to(F64)[:, None] * inv[None, :]
    return ang.cos(), ang.sin()


def rotate(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """x [S, H, D]: the half-split rotation, (a, b) -> (a cos - b sin, b cos + a sin) with a = x[..., :D/2]."""
    h = x.shape[-1] // 2
    a, b = x[..., :h], x[..., h:]
    c, s = cos[:, None, :], sin[:, None, :]
    return torch.cat((a * c - b * s, b * c + a * s), -1)


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """q [S, Hq, D], k / v [S, Hkv, D] at positions 0..S-1 -> [S, Hq * D]; causal, query head h on kv head h // G."""
    S, Hq, D = q.shape
    G = Hq // k.shape[1]
    kk = k.repeat_interleave(G, dim=1)            # kv head j serves query heads j G .. j G + G - 1
    vv = v.repeat_interleave(G, dim=1)
    s = torch.einsum("ihd,jhd->hij", q, kk) / math.sqrt(D)
    hidden = torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1)
    p = torch.softmax(s.masked_fill(hidden, float("-inf")), -1)
    return torch.einsum("hij,jhd->ihd", p, vv).reshape(S, Hq * D)


def head_logprobs(h: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """log_softmax(h @ w.T) for h [n, H] fp64 and the lm_head w [V, H] of any dtype, in row blocks of w."""
    out = torch.empty(h.shape[0], w.shape[0], dtype=F64, device=h.device)
    for a in range(0, w.shape[0], HEAD_ROWS):
        out[:, a:a + HEAD_ROWS] = h @ w[a:a + HEAD_ROWS].to(F64).t()
    return torch.log_softmax(out, -1)


def forward(weights: dict, cfg, tokens: torch.Tensor, kv_round: Optional[Callable] = None, trace: Optional[list] = None):
    """One sequence (1-D token ids) -> the final-norm hidden states [S, H], fp64.  `trace`, a list, receives
    (name, tensor [S, .]) for the embedding, each layer's attention output (before o_proj), its hidden state
    after the attention residual and after the MLP residual, and the final norm."""
    H, Hq, Hkv = _get(cfg, "hidden_size"), _get(cfg, "num_attention_heads"), _get(cfg, "num_key_value_heads")
    D = _get(cfg, "head_dim") or H // Hq
    theta = _get(cfg, "rope_theta")
    if theta is None:                       # newer transformers configs keep it in rope_parameters
        theta = _get(cfg, "rope_parameters")["rope_theta"]
    eps, theta = float(_get(cfg, "rms_norm_eps")), float(theta)
    S = tokens.numel()
    emb = weights["model.embed_tokens.weight"]
    x = emb[tokens.to(emb.device)].to(F64)
    cos, sin = rotary_angles(torch.arange(S, device=x.device), D, theta)

    def note(name, t):
        if trace is not None:
            trace.append((name, t))

    note("embed", x)
    for i in range(_get(cfg, "num_hidden_layers")):
        p = f"model.layers.{i}."
        h = rms_norm(x, weights[p + "input_layernorm.weight"], eps)
        q = rotate((h @ weights[p + "self_attn.q_proj.weight"].t()).view(S, Hq, D), cos, sin)
        k = rotate((h @ weights[p + "self_attn.k_proj.weight"].t()).view(S, Hkv, D), cos, sin)
        v = (h @ weights[p + "self_attn.v_proj.weight"].t()).view(S, Hkv, D)
        if kv_round is not None:
            k, v = kv_round(k, v)
        a = attention(q, k, v)
        note(f"layer{i}.attn", a)
        x = x + a @ weights[p + "self_attn.o_proj.weight"].t()
        note(f"layer{i}.mid", x)
        h = rms_norm(x, weights[p + "post_attention_layernorm.weight"], eps)
        g = h @ weights[p + "mlp.gate_proj.weight"].t()
        u = h @ weights[p + "mlp.up_proj.weight"].t()
        x = x + (g * torch.sigmoid(g) * u) @ weights[p + "mlp.down_proj.weight"].t()
        note(f"layer{i}.out", x)
    x = rms_norm(x, weights["model.norm.weight"], eps)
    note("norm", x)
    return x


def logprobs(weights: dict, cfg, rows: Sequence[torch.Tensor], positions: Sequence[Sequence[int]],
             kv_round: Optional[Callable] = None, traces: Optional[list] = None) -> list:
    """rows: token sequences of any lengths (1-D int64 each).  positions[b]: the indices p of rows[b] at which
    the distribution of the NEXT token is wanted.  Returns one fp64 [len(positions[b]), V] per row:
    log_softmax of the lm_head over the final-norm hidden state at p -- the lm_head sees those rows only.
    kv_round(k, v) -> (k, v), both [S, Hkv, D] fp64 (k after the rotary), replaces every position's key and
    value rows in front of the attention (a cache format's round trip).  traces, a list, receives one
    `forward` trace per row."""
    out = []
    with torch.no_grad():
        for toks, at in zip(rows, positions):
            trace = None if traces is None else []
            h = forward(weights, cfg, toks, kv_round, trace)
            if traces is not None:
                traces.append(trace)
            idx = torch.as_tensor(list(at), dtype=torch.int64, device=h.device)
            out.append(head_logprobs(h[idx], weights["lm_head.weight"]))
    return out
