"""One-launch HIP forms of the small ops around a Llama layer's 4-bit
projections (csrc/layer_ops.hip, C-ABI include/quantizations.h):

* ``rms_norm``  -- LlamaRMSNorm.forward (transformers modeling_llama.py:62-67),
  which produces the input of q/k/v and gate/up;
* ``rope_qk``   -- apply_rotary_pos_emb (modeling_llama.py:138-160), applied to
  the outputs of q_proj/k_proj;
* ``silu_mul``  -- LlamaMLP's act_fn(gate_proj(x)) * up_proj(x)
  (modeling_llama.py:175), the input of down_proj;
* ``add_rms_norm`` -- LlamaDecoderLayer's ``residual + h`` followed by the
  post-attention RMSNorm (modeling_llama.py:317-321).

``greedy_step`` / ``sample_step`` are a decode loop's token pick with its feedback (csrc/sample.hip for the
sampled one, which alone has a composed torch route: fp32 or CPU logits).  ``decode_attention_streams``,
``greedy_step_streams`` and ``sample_step_streams`` are their forms with a position per stream
(generation.StreamSession); both streams picks have a composed torch route.  ``decode_attention_verify``,
``verify_step_streams`` and ``ngram_draft`` are the three launches of a speculative greedy step
(generation.SpeculativeSession): a window of T tokens per stream, the pick that accepts the longest
matching prefix of its drafts, and the prompt-lookup drafter; the last two have a composed / host route.
``verify_sample_step_streams`` is that pick for sampled streams: every row is drawn as
``sample_step_streams`` would draw it at its position, and a draft is accepted when it is that token.

None of them is in the reference (it leaves them to transformers).  They exist
because at batch-1 decode the eager torch forms cost ~8, ~10 and 2 dependent
launches per call, which dominate the step once the Linear4bit GEMVs are
fused.  ``integration.fuse_layer_ops`` installs them.
No CPU or torch fallback lives here: the callers decide what is supported.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib

_SUPPORTED = (torch.float16, torch.bfloat16, torch.float32)


def _needs_grad(*xs: torch.Tensor) -> bool:
    """Autograd is recording and one of the activations requires grad.  These launches write into
    fresh buffers and have no backward, so every *_supported predicate declines such an input: a
    model patched by integration.fuse_* then runs the original torch op instead of detaching."""
    return torch.is_grad_enabled() and any(x.requires_grad for x in xs)


def rms_norm_supported(x: torch.Tensor, weight: torch.Tensor) -> bool:
    return (not _needs_grad(x)
            and x.is_cuda and x.dtype in _SUPPORTED and weight.dtype == x.dtype and weight.device == x.device
            and weight.dim() == 1 and x.dim() >= 1 and x.shape[-1] == weight.shape[0] and weight.is_contiguous()
            and x.stride(-1) == 1)


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    """weight * (x.float() * rsqrt(mean(x.float()**2, -1) + eps)).to(x.dtype), one launch."""
    if not rms_norm_supported(x, weight):
        raise ValueError(f"rms_norm: unsupported input ({x.dtype} on {x.device}, weight {weight.dtype})")
    K = x.shape[-1]
    x2 = x.reshape(-1, K)  # a view for every layout HF produces (row stride may exceed K)
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib.qz_rmsnorm(x2.data_ptr(), _lib.dtype_code(x.dtype), x2.shape[0], K, x2.stride(0),
                                   weight.data_ptr(), float(eps), y.data_ptr(), K, _lib.stream_of(x)),
               "qz_rmsnorm")
    return y


def add_rms_norm_supported(x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor) -> bool:
    return (not _needs_grad(residual) and rms_norm_supported(x, weight)
            and residual.dtype == x.dtype and residual.device == x.device
            and residual.shape == x.shape and x.is_contiguous() and residual.is_contiguous())


def add_rms_norm(x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float):
    """(s, rms_norm(s)) with s = residual + x (rounded to x.dtype, bit-exact to the
    torch add), one launch."""
    if not add_rms_norm_supported(x, residual, weight):
        raise ValueError("add_rms_norm: unsupported input")
    K = x.shape[-1]
    rows = x.numel() // K if K else 0
    s = torch.empty_like(x)
    y = torch.empty_like(x)
    _lib.check(_lib.lib.qz_add_rmsnorm(x.data_ptr(), residual.data_ptr(), _lib.dtype_code(x.dtype), rows, K, K,
                                       weight.data_ptr(), float(eps), s.data_ptr(), y.data_ptr(), K,
                                       _lib.stream_of(x)), "qz_add_rmsnorm")
    return s, y


def _strides3(t: torch.Tensor):
    return (ctypes.c_longlong * 3)(t.stride(0), t.stride(1), t.stride(2))


def rope_supported(q: torch.Tensor, k: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                   unsqueeze_dim: int = 1) -> bool:
    if _needs_grad(q, k):
        return False
    if unsqueeze_dim != 1 or q.dim() != 4 or k.dim() != 4 or cos.dim() != 3 or sin.shape != cos.shape:
        return False
    if not (q.is_cuda and q.dtype in _SUPPORTED and k.dtype == q.dtype and cos.dtype == q.dtype
            and sin.dtype == q.dtype and k.device == q.device and cos.device == q.device and sin.device == q.device):
        return False
    B, _, S, D = q.shape
    if k.shape[0] != B or k.shape[2] != S or k.shape[3] != D or D % 2 or cos.shape[1] != S or cos.shape[2] != D:
        return False
    if cos.shape[0] not in (1, B) or cos.stride() != sin.stride():
        return False
    return q.stride(-1) == 1 and k.stride(-1) == 1 and cos.stride(-1) == 1


def rope_qk(q: torch.Tensor, k: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor):
    """(q*cos + rotate_half(q)*sin, k*cos + rotate_half(k)*sin) for q/k [B, H, S, D]
    and cos/sin [B or 1, S, D]; one launch, bit-identical to the torch expression."""
    if not rope_supported(q, k, cos, sin):
        raise ValueError("rope_qk: unsupported shapes/dtypes/layout")
    B, Hq, S, D = q.shape
    Hk = k.shape[1]
    qo = torch.empty_like(q)  # keeps q's (transposed) layout, as torch's elementwise ops do
    ko = torch.empty_like(k)
    if qo.stride(-1) != 1 or ko.stride(-1) != 1:
        qo = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        ko = torch.empty(k.shape, dtype=k.dtype, device=k.device)
    q3, qo3, k3, ko3 = (t[:, :, :, 0] for t in (q, qo, k, ko))
    cs = (ctypes.c_longlong * 2)(cos.stride(0) if cos.shape[0] == B else 0, cos.stride(1))
    _lib.check(_lib.lib.qz_rope_qk(_lib.dtype_code(q.dtype), B, S, D,
                                   q.data_ptr(), Hq, _strides3(q3), qo.data_ptr(), _strides3(qo3),
                                   k.data_ptr(), Hk, _strides3(k3), ko.data_ptr(), _strides3(ko3),
                                   cos.data_ptr(), sin.data_ptr(), cs, _lib.stream_of(q)),
               "qz_rope_qk")
    return qo, ko


def silu_mul_supported(g: torch.Tensor, u: torch.Tensor) -> bool:
    return (not _needs_grad(g, u)
            and g.is_cuda and g.dtype in _SUPPORTED and u.dtype == g.dtype and u.device == g.device
            and g.shape == u.shape and g.is_contiguous() and u.is_contiguous())


def silu_mul(g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """F.silu(g) * u with torch's per-op rounding, one launch."""
    if not silu_mul_supported(g, u):
        raise ValueError("silu_mul: unsupported shapes/dtypes/layout")
    y = torch.empty_like(g)
    _lib.check(_lib.lib.qz_silu_mul(g.data_ptr(), u.data_ptr(), _lib.dtype_code(g.dtype), g.numel(), y.data_ptr(),
                                    _lib.stream_of(g)), "qz_silu_mul")
    return y


ATTN_CHUNK = 128  # key positions per workgroup of qz_decode_attention (csrc/layer_ops.hip)


def _attention_operands_supported(q, cos, key_cache, value_cache, num_heads: int) -> bool:
    """What both decode attention launches ask of the activations, the caches and cos/sin."""
    if _needs_grad(q) or not (q.is_cuda and q.dtype in (torch.float16, torch.bfloat16) and q.dim() == 3
                              and q.shape[1] == 1):
        return False
    if key_cache.dim() != 4 or value_cache.shape != key_cache.shape:
        return False
    B, Hkv, L, D = key_cache.shape
    if D not in (64, 128) or num_heads % Hkv or num_heads // Hkv > 8 or q.shape[0] != B or L == 0:
        return False
    for t in (key_cache, value_cache):
        if t.dtype != q.dtype or t.device != q.device or not t.is_contiguous() or t.data_ptr() % 16:
            return False
    return (cos.dim() == 3 and cos.shape[0] in (1, B) and cos.shape[1] == 1 and cos.shape[2] == D
            and cos.dtype == q.dtype and cos.device == q.device and cos.stride(-1) == 1)


def decode_attention_supported(q: torch.Tensor, cos: torch.Tensor, key_cache: torch.Tensor,
                               value_cache: torch.Tensor, mask, pos, num_heads: int) -> bool:
    """What qz_decode_attention takes: one new token per sequence (q, or the layer input:
    [B, 1, *]), 16-bit activations, a contiguous static cache [B, Hkv, L, D] with D in {64, 128}
    and Hq/Hkv <= 8, a bool mask [B or 1, 1, 1, L], cos/sin [B or 1, 1, D] and an int64 position
    on the GPU.  Metadata only: nothing is launched or allocated."""
    if not _attention_operands_supported(q, cos, key_cache, value_cache, num_heads):
        return False
    B, L = key_cache.shape[0], key_cache.shape[2]
    if not (isinstance(mask, torch.Tensor) and mask.dtype == torch.bool and mask.device == q.device
            and mask.dim() == 4 and mask.shape[0] in (1, B) and mask.shape[1] == 1 and mask.shape[2] == 1
            and mask.shape[3] == L):
        return False
    return (isinstance(pos, torch.Tensor) and pos.dtype == torch.int64 and pos.numel() == 1 and pos.device == q.device)


def _attention_launch_operands(name, q, k, v, cos, sin, key_cache, num_heads):
    """The row views, output, chunk workspace and cos/sin row stride both decode attention launches pass."""
    B, Hkv, L, D = key_cache.shape
    G = num_heads // Hkv
    if q.shape[2] != num_heads * D:
        raise ValueError(f"{name}: q width differs from num_heads * head_dim")
    if sin.shape != cos.shape or sin.stride() != cos.stride() or sin.dtype != cos.dtype:
        raise ValueError(f"{name}: sin must match cos")
    q2, k2, v2 = (t.reshape(B, -1) for t in (q, k, v))
    k2 = k2 if k2.stride(-1) == 1 else k2.contiguous()
    q2 = q2 if q2.stride(-1) == 1 else q2.contiguous()
    if v2.stride(-1) != 1 or v2.stride(0) % 2 or v2.data_ptr() % 4:
        v2 = v2.contiguous()
    if k2.shape[1] != Hkv * D or v2.shape[1] != Hkv * D:
        raise ValueError(f"{name}: k/v width differs from the cache's heads")
    out = torch.empty((B, 1, num_heads * D), dtype=q.dtype, device=q.device)
    nsplit = -(-L // ATTN_CHUNK)
    work = torch.empty(B * Hkv * nsplit * G * (D + 2), dtype=torch.float32, device=q.device) if nsplit > 1 else None
    cs_row = cos.stride(0) if cos.shape[0] == B and B > 1 else 0
    return q2, k2, v2, out, work, cs_row


def decode_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                     key_cache: torch.Tensor, value_cache: torch.Tensor, mask: torch.Tensor, pos: torch.Tensor,
                     arrive: torch.Tensor, num_heads: int, scale: float) -> torch.Tensor:
    """LlamaAttention.forward for one new token per sequence against a static cache, up to the
    o_proj input: rotary of q/k, key_cache/value_cache[:, :, pos] = k, v, pos += 1 (all on the
    GPU, graph-capturable), masked GQA softmax(q k^T * scale) v.  q [B, 1, Hq*D], k/v
    [B, 1, Hkv*D] (the projection outputs), cos/sin [B or 1, 1, D], caches [B, Hkv, L, D],
    mask bool [B or 1, 1, 1, L], pos int64 (StaticLayer.cumulative_length), arrive a zeroed
    int32 scratch word.  Returns [B, 1, Hq*D]."""
    if not decode_attention_supported(q, cos, key_cache, value_cache, mask, pos, num_heads):
        raise ValueError("decode_attention: unsupported shapes/dtypes/layout")
    B, Hkv, L, D = key_cache.shape
    q2, k2, v2, out, work, cs_row = _attention_launch_operands("decode_attention", q, k, v, cos, sin, key_cache,
                                                               num_heads)
    mb = mask.stride(0) if mask.shape[0] == B and B > 1 else 0
    _lib.check(_lib.lib.qz_decode_attention(
        _lib.dtype_code(q.dtype), B, num_heads, Hkv, D, L, q2.data_ptr(), q2.stride(0), k2.data_ptr(), k2.stride(0),
        v2.data_ptr(), v2.stride(0), cos.data_ptr(), sin.data_ptr(), cs_row, key_cache.data_ptr(),
        value_cache.data_ptr(), mask.data_ptr(), mb, mask.stride(3), pos.data_ptr(), arrive.data_ptr(),
        out.data_ptr(), num_heads * D, work.data_ptr() if work is not None else None, float(scale),
        _lib.stream_of(q)), "qz_decode_attention")
    return out


def decode_attention_streams_supported(q: torch.Tensor, cos: torch.Tensor, key_cache: torch.Tensor,
                                       value_cache: torch.Tensor, pos, num_heads: int) -> bool:
    """What qz_decode_attention_streams takes: decode_attention_supported's activations, caches and
    cos/sin, no mask, and an int64 position per stream -- pos [B], contiguous, on the GPU.  Metadata
    only: nothing is launched or allocated."""
    if not _attention_operands_supported(q, cos, key_cache, value_cache, num_heads):
        return False
    return (isinstance(pos, torch.Tensor) and pos.dtype == torch.int64 and pos.dim() == 1
            and pos.shape[0] == key_cache.shape[0] and pos.device == q.device and pos.is_contiguous())


def decode_attention_streams(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                             key_cache: torch.Tensor, value_cache: torch.Tensor, pos: torch.Tensor, num_heads: int,
                             scale: float) -> torch.Tensor:
    """decode_attention with a position per stream (qz_decode_attention_streams): pos int64 [B];
    stream b's new k/v go to cache slot pos[b] and its keys 0..pos[b] are visible.  No mask, no
    arrival word, and pos is left as it is (greedy_step_streams / sample_step_streams advance it).
    Each stream's output and cache rows carry the bits of decode_attention on that stream alone; a
    position outside [0, L) gives that stream a NaN row and writes nothing of it.  Returns
    [B, 1, Hq*D]."""
    if not decode_attention_streams_supported(q, cos, key_cache, value_cache, pos, num_heads):
        raise ValueError("decode_attention_streams: unsupported shapes/dtypes/layout")
    B, Hkv, L, D = key_cache.shape
    q2, k2, v2, out, work, cs_row = _attention_launch_operands("decode_attention_streams", q, k, v, cos, sin,
                                                               key_cache, num_heads)
    _lib.check(_lib.lib.qz_decode_attention_streams(
        _lib.dtype_code(q.dtype), B, num_heads, Hkv, D, L, q2.data_ptr(), q2.stride(0), k2.data_ptr(), k2.stride(0),
        v2.data_ptr(), v2.stride(0), cos.data_ptr(), sin.data_ptr(), cs_row, key_cache.data_ptr(),
        value_cache.data_ptr(), pos.data_ptr(), out.data_ptr(), num_heads * D,
        work.data_ptr() if work is not None else None, float(scale), _lib.stream_of(q)),
        "qz_decode_attention_streams")
    return out


def decode_attention_verify_supported(q: torch.Tensor, cos: torch.Tensor, key_cache: torch.Tensor,
                                      value_cache: torch.Tensor, pos, num_heads: int) -> bool:
    """What qz_decode_attention_verify takes: T >= 2 new tokens per stream (q, or the layer input:
    [B, T, *]), 16-bit activations, decode_attention_streams_supported's caches and pos [B], and
    cos/sin [B, T, D] whose B T rows lie at one stride.  Metadata only: nothing is launched or
    allocated."""
    if _needs_grad(q) or not (isinstance(q, torch.Tensor) and q.is_cuda and q.dtype in (torch.float16, torch.bfloat16)
                              and q.dim() == 3 and q.shape[1] >= 2):
        return False
    if key_cache.dim() != 4 or value_cache.shape != key_cache.shape:
        return False
    B, Hkv, L, D = key_cache.shape
    T = q.shape[1]
    if (D not in (64, 128) or Hkv == 0 or num_heads % Hkv or num_heads // Hkv > 8 or q.shape[0] != B or L == 0
            or B * T > 65535):
        return False
    for t in (key_cache, value_cache):
        if t.dtype != q.dtype or t.device != q.device or not t.is_contiguous() or t.data_ptr() % 16:
            return False
    if not (cos.dim() == 3 and tuple(cos.shape) == (B, T, D) and cos.dtype == q.dtype and cos.device == q.device
            and cos.stride(-1) == 1 and (B == 1 or cos.stride(0) == T * cos.stride(1))):
        return False
    return (isinstance(pos, torch.Tensor) and pos.dtype == torch.int64 and pos.dim() == 1
            and pos.shape[0] == B and pos.device == q.device and pos.is_contiguous())


def decode_attention_verify(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                            key_cache: torch.Tensor, value_cache: torch.Tensor, pos: torch.Tensor, num_heads: int,
                            scale: float) -> torch.Tensor:
    """decode_attention_streams for a window of T tokens per stream (qz_decode_attention_verify): q
    [B, T, Hq*D], k/v [B, T, Hkv*D], cos/sin [B, T, D], pos int64 [B].  Token (b, i) sits at position
    pos[b] + i: its k/v go to that slot of cache row b and it sees keys 0..pos[b] + i, the window's
    earlier tokens included.  Outputs and caches carry the bits of T successive
    decode_attention_streams calls on stream b alone, so a token's result does not depend on its row.
    A row past the cache end is NaN and writes nothing; pos[b] < 0 makes stream b's T rows NaN; pos
    is left as it is.  Returns [B, T, Hq*D]."""
    if not decode_attention_verify_supported(q, cos, key_cache, value_cache, pos, num_heads):
        raise ValueError("decode_attention_verify: unsupported shapes/dtypes/layout")
    B, Hkv, L, D = key_cache.shape
    T, G = q.shape[1], num_heads // Hkv
    _check_window("decode_attention_verify", q, k, v, cos, sin, num_heads, D)
    q2, k2, v2 = _verify_rows("decode_attention_verify", q, k, v, Hkv * D, "cache's")
    out = torch.empty((B, T, num_heads * D), dtype=q.dtype, device=q.device)
    nsplit = -(-L // ATTN_CHUNK)
    work = (torch.empty(B * T * Hkv * nsplit * G * (D + 2), dtype=torch.float32, device=q.device) if nsplit > 1
            else None)
    _lib.check(_lib.lib.qz_decode_attention_verify(
        _lib.dtype_code(q.dtype), B, T, num_heads, Hkv, D, L, q2.data_ptr(), q2.stride(0), k2.data_ptr(), k2.stride(0),
        v2.data_ptr(), v2.stride(0), cos.data_ptr(), sin.data_ptr(), cos.stride(1), key_cache.data_ptr(),
        value_cache.data_ptr(), pos.data_ptr(), out.data_ptr(), num_heads * D,
        work.data_ptr() if work is not None else None, float(scale), _lib.stream_of(q)),
        "qz_decode_attention_verify")
    return out


PREFILL_TQ = 64  # query rows per workgroup of qz_prefill_attention (csrc/prefill_attn.hip: kPfTQ)
PREFILL_TK = 64  # keys per staged tile, from absolute position 0 (kPfTK)


def prefill_attention_supported(q: torch.Tensor, cos: torch.Tensor, key_cache: torch.Tensor,
                                value_cache: torch.Tensor, pos, length, num_heads: int) -> bool:
    """What qz_prefill_attention takes: T >= 1 new tokens per stream (q, or the layer input:
    [B, T, *]), 16-bit activations, a contiguous static cache [B, Hkv, L, D] with D in {64, 128} and
    Hq/Hkv <= 8, cos/sin [B or 1, T, D] with unit inner stride, and int64 pos / length [B],
    contiguous, on q's device.  Metadata only: nothing is launched or allocated."""
    if not (isinstance(q, torch.Tensor) and q.is_cuda and q.dtype in (torch.float16, torch.bfloat16)
            and q.dim() == 3 and q.shape[1] >= 1) or _needs_grad(q):
        return False
    if key_cache.dim() != 4 or value_cache.shape != key_cache.shape:
        return False
    B, Hkv, L, D = key_cache.shape
    T = q.shape[1]
    if (D not in (64, 128) or Hkv == 0 or num_heads % Hkv or num_heads // Hkv > 8 or q.shape[0] != B or L == 0
            or B > 65535 or num_heads > 65535):
        return False
    for t in (key_cache, value_cache):
        if t.dtype != q.dtype or t.device != q.device or not t.is_contiguous() or t.data_ptr() % 16:
            return False
    if not (isinstance(cos, torch.Tensor) and cos.dim() == 3 and cos.shape[0] in (1, B) and cos.shape[1] == T
            and cos.shape[2] == D and cos.dtype == q.dtype and cos.device == q.device and cos.stride(-1) == 1):
        return False
    for p in (pos, length):
        if not (isinstance(p, torch.Tensor) and p.dtype == torch.int64 and p.dim() == 1 and p.shape[0] == B
                and p.device == q.device and p.is_contiguous()):
            return False
    return True


def prefill_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                      key_cache: torch.Tensor, value_cache: torch.Tensor, pos: torch.Tensor, length: torch.Tensor,
                      num_heads: int, scale: float) -> torch.Tensor:
    """Causal attention of a window of T new tokens per stream against the static cache
    (qz_prefill_attention): q [B, T, Hq*D], k/v [B, T, Hkv*D], cos/sin [B or 1, T, D], pos and length
    int64 [B].  Token (b, i) with i < length[b] sits at position pos[b] + i: its rotated k and its v go
    to that slot of cache row b (the bits a decode step stores there) and it sees keys 0..pos[b] + i.
    Rows i >= length[b] write nothing and come back as zeros.  The work is O(visible keys): key tiles
    above a query tile's last position are never loaded.  A row's bits do not depend on T, on its
    index in the window or on the other streams, so a prompt run in chunks equals the prompt run
    whole.  A real row past the cache end is NaN and writes nothing; pos[b] outside [0, L) makes
    stream b's real rows NaN; pos and length are left as they are.  Returns [B, T, Hq*D]."""
    if not prefill_attention_supported(q, cos, key_cache, value_cache, pos, length, num_heads):
        raise ValueError("prefill_attention: unsupported shapes/dtypes/layout")
    B, Hkv, L, D = key_cache.shape
    T = q.shape[1]
    _check_window("prefill_attention", q, k, v, cos, sin, num_heads, D)
    if k.shape[2] != Hkv * D or v.shape[2] != Hkv * D:
        raise ValueError("prefill_attention: k/v width differs from the cache's heads")
    q2, qs, k2, ks, v2, vs, c2, s2, cs = _prefill_rows(q, k, v, cos, sin, B, T, D)
    out = torch.empty((B, T, num_heads * D), dtype=q.dtype, device=q.device)
    _lib.check(_lib.lib.qz_prefill_attention(
        _lib.dtype_code(q.dtype), B, T, num_heads, Hkv, D, L, q2.data_ptr(), qs, k2.data_ptr(), ks, v2.data_ptr(), vs,
        c2.data_ptr(), s2.data_ptr(), cs, key_cache.data_ptr(), value_cache.data_ptr(), pos.data_ptr(),
        length.data_ptr(), out.data_ptr(), num_heads * D, float(scale), _lib.stream_of(q)), "qz_prefill_attention")
    return out


KV_PAGE = 128  # positions per page of the paged cache (qz_kv_page_size(): the decode head's key chunk)


KV8_ROW_EXTRA = 1  # bytes a kv8 cache row carries beyond its D codes: the scale byte


def _pool_geometry(k_pool, v_pool, kv8: bool):
    """(P, Hkv, D) of a pair of page pools -- [P, Hkv, 128, D], or kv8: uint8 [P, Hkv, 128 (D + 1)];
    None for anything else."""
    if not (isinstance(k_pool, torch.Tensor) and isinstance(v_pool, torch.Tensor)
            and k_pool.dim() == (3 if kv8 else 4) and v_pool.shape == k_pool.shape):
        return None
    if not kv8:
        P, Hkv, page, D = k_pool.shape
        return (P, Hkv, D) if page == KV_PAGE else None
    if k_pool.dtype != torch.uint8:
        return None
    P, Hkv, W = k_pool.shape
    D = W // KV_PAGE - KV8_ROW_EXTRA
    return (P, Hkv, D) if W == KV_PAGE * (D + KV8_ROW_EXTRA) else None


def _paged_operands_supported(q, cos, k_pool, v_pool, table, pos, num_heads: int, min_t: int, cos_batches,
                              kv8: bool = False) -> bool:
    """What the three paged launches ask of the activations, the pools [P, Hkv, 128, D] (kv8: uint8
    [P, Hkv, 128 (D + 1)]), the table int32 [B, NP] with unit inner stride, pos int64 [B] and cos/sin
    [*, T, D]."""
    if not (isinstance(q, torch.Tensor) and q.is_cuda and q.dtype in (torch.float16, torch.bfloat16)
            and q.dim() == 3 and q.shape[1] >= min_t) or _needs_grad(q):
        return False
    geometry = _pool_geometry(k_pool, v_pool, kv8)
    if geometry is None:
        return False
    P, Hkv, D = geometry
    B, T = q.shape[0], q.shape[1]
    if (D not in (64, 128) or Hkv == 0 or P == 0 or num_heads % Hkv or num_heads // Hkv > 8 or B > 65535
            or num_heads > 65535):
        return False
    for t in (k_pool, v_pool):
        if (t.dtype != (torch.uint8 if kv8 else q.dtype) or t.device != q.device or not t.is_contiguous()
                or t.data_ptr() % 16):
            return False
    if not (isinstance(table, torch.Tensor) and table.dtype == torch.int32 and table.dim() == 2
            and table.shape[0] == B and table.shape[1] >= 1 and table.device == q.device
            and table.stride(1) == 1 and table.stride(0) >= table.shape[1]):
        return False
    if not (isinstance(cos, torch.Tensor) and cos.dim() == 3 and cos.shape[0] in cos_batches(B) and cos.shape[1] == T
            and cos.shape[2] == D and cos.dtype == q.dtype and cos.device == q.device and cos.stride(-1) == 1):
        return False
    return (isinstance(pos, torch.Tensor) and pos.dtype == torch.int64 and pos.dim() == 1 and pos.shape[0] == B
            and pos.device == q.device and pos.is_contiguous())


def _decode_paged_supported(q, cos, k_pool, v_pool, table, pos, num_heads: int, kv8: bool) -> bool:
    return (isinstance(q, torch.Tensor) and q.dim() == 3 and q.shape[1] == 1
            and _paged_operands_supported(q, cos, k_pool, v_pool, table, pos, num_heads, 1, lambda B: (1, B), kv8))


def _verify_paged_supported(q, cos, k_pool, v_pool, table, pos, num_heads: int, kv8: bool) -> bool:
    if not _paged_operands_supported(q, cos, k_pool, v_pool, table, pos, num_heads, 2, lambda B: (B,), kv8):
        return False
    B, T = q.shape[0], q.shape[1]
    return B * T <= 65535 and (B == 1 or cos.stride(0) == T * cos.stride(1))


def _prefill_paged_supported(q, cos, k_pool, v_pool, table, pos, length, num_heads: int, kv8: bool) -> bool:
    if not _paged_operands_supported(q, cos, k_pool, v_pool, table, pos, num_heads, 1, lambda B: (1, B), kv8):
        return False
    return (isinstance(length, torch.Tensor) and length.dtype == torch.int64 and length.dim() == 1
            and length.shape[0] == q.shape[0] and length.device == q.device and length.is_contiguous())


def _decode_paged(q, k, v, cos, sin, k_pool, v_pool, table, pos, num_heads: int, scale: float, kv8: bool):
    """decode_attention_paged and decode_attention_paged_kv8: one launch, two pool formats."""
    name = "decode_attention_paged_kv8" if kv8 else "decode_attention_paged"
    if not _decode_paged_supported(q, cos, k_pool, v_pool, table, pos, num_heads, kv8):
        raise ValueError(f"{name}: unsupported shapes/dtypes/layout")
    P, Hkv, D = _pool_geometry(k_pool, v_pool, kv8)
    B, NP = table.shape
    # _attention_launch_operands reads only the shape of its cache operand: [B, Hkv, L, D]
    shape = q.as_strided((B, Hkv, NP * KV_PAGE, D), (0, 0, 0, 0))
    q2, k2, v2, out, work, cs_row = _attention_launch_operands(name, q, k, v, cos, sin, shape, num_heads)
    launch = _lib.lib.qz_decode_attention_paged_kv8 if kv8 else _lib.lib.qz_decode_attention_paged
    _lib.check(launch(
        _lib.dtype_code(q.dtype), B, num_heads, Hkv, D, NP, P, q2.data_ptr(), q2.stride(0), k2.data_ptr(), k2.stride(0),
        v2.data_ptr(), v2.stride(0), cos.data_ptr(), sin.data_ptr(), cs_row, k_pool.data_ptr(), v_pool.data_ptr(),
        table.data_ptr(), table.stride(0), pos.data_ptr(), out.data_ptr(), num_heads * D,
        work.data_ptr() if work is not None else None, float(scale), _lib.stream_of(q)), "qz_" + name)
    return out


def _verify_paged(q, k, v, cos, sin, k_pool, v_pool, table, pos, num_heads: int, scale: float, kv8: bool):
    """decode_attention_verify_paged and decode_attention_verify_paged_kv8: one launch, two pool formats."""
    name = "decode_attention_verify_paged_kv8" if kv8 else "decode_attention_verify_paged"
    if not _verify_paged_supported(q, cos, k_pool, v_pool, table, pos, num_heads, kv8):
        raise ValueError(f"{name}: unsupported shapes/dtypes/layout")
    P, Hkv, D = _pool_geometry(k_pool, v_pool, kv8)
    B, NP = table.shape
    T, G = q.shape[1], num_heads // Hkv
    _check_window(name, q, k, v, cos, sin, num_heads, D)
    q2, k2, v2 = _verify_rows(name, q, k, v, Hkv * D, "pools'")
    out = torch.empty((B, T, num_heads * D), dtype=q.dtype, device=q.device)
    work = torch.empty(B * T * Hkv * NP * G * (D + 2), dtype=torch.float32, device=q.device) if NP > 1 else None
    launch = _lib.lib.qz_decode_attention_verify_paged_kv8 if kv8 else _lib.lib.qz_decode_attention_verify_paged
    _lib.check(launch(
        _lib.dtype_code(q.dtype), B, T, num_heads, Hkv, D, NP, P, q2.data_ptr(), q2.stride(0), k2.data_ptr(),
        k2.stride(0), v2.data_ptr(), v2.stride(0), cos.data_ptr(), sin.data_ptr(), cos.stride(1), k_pool.data_ptr(),
        v_pool.data_ptr(), table.data_ptr(), table.stride(0), pos.data_ptr(), out.data_ptr(), num_heads * D,
        work.data_ptr() if work is not None else None, float(scale), _lib.stream_of(q)), "qz_" + name)
    return out


def _prefill_paged(q, k, v, cos, sin, k_pool, v_pool, table, pos, length, num_heads: int, scale: float, kv8: bool):
    """prefill_attention_paged and prefill_attention_paged_kv8: one launch, two pool formats."""
    name = "prefill_attention_paged_kv8" if kv8 else "prefill_attention_paged"
    if not _prefill_paged_supported(q, cos, k_pool, v_pool, table, pos, length, num_heads, kv8):
        raise ValueError(f"{name}: unsupported shapes/dtypes/layout")
    P, Hkv, D = _pool_geometry(k_pool, v_pool, kv8)
    B, NP = table.shape
    T = q.shape[1]
    _check_window(name, q, k, v, cos, sin, num_heads, D)
    if k.shape[2] != Hkv * D or v.shape[2] != Hkv * D:
        raise ValueError(f"{name}: k/v width differs from the pools' heads")
    q2, qs, k2, ks, v2, vs, c2, s2, cs = _prefill_rows(q, k, v, cos, sin, B, T, D)
    out = torch.empty((B, T, num_heads * D), dtype=q.dtype, device=q.device)
    launch = _lib.lib.qz_prefill_attention_paged_kv8 if kv8 else _lib.lib.qz_prefill_attention_paged
    _lib.check(launch(
        _lib.dtype_code(q.dtype), B, T, num_heads, Hkv, D, NP, P, q2.data_ptr(), qs, k2.data_ptr(), ks, v2.data_ptr(),
        vs, c2.data_ptr(), s2.data_ptr(), cs, k_pool.data_ptr(), v_pool.data_ptr(), table.data_ptr(), table.stride(0),
        pos.data_ptr(), length.data_ptr(), out.data_ptr(), num_heads * D, float(scale), _lib.stream_of(q)),
        "qz_" + name)
    return out


def decode_attention_paged_supported(q: torch.Tensor, cos: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor,
                                     table, pos, num_heads: int) -> bool:
    """What qz_decode_attention_paged takes: one new token per stream (q [B, 1, *]), 16-bit
    activations, pools [P, Hkv, 128, D] with D in {64, 128} and Hq/Hkv <= 8, a table int32 [B, NP] with
    unit inner stride, cos/sin [B or 1, 1, D] and pos int64 [B], all on q's device.  Metadata only:
    nothing is launched or allocated."""
    return _decode_paged_supported(q, cos, k_pool, v_pool, table, pos, num_heads, False)


def decode_attention_paged(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                           k_pool: torch.Tensor, v_pool: torch.Tensor, table: torch.Tensor, pos: torch.Tensor,
                           num_heads: int, scale: float) -> torch.Tensor:
    """decode_attention_streams through a page table (qz_decode_attention_paged): pools
    [P, Hkv, 128, D], table int32 [B, NP]; key j of stream b lives in page table[b, j >> 7] at slot
    j & 127, and the logical cache length is 128 NP.  Output and the slot written carry the bits of
    decode_attention_streams on the cache the table gathers.  A table entry outside [0, P) that the
    stream needs makes its row NaN and is never dereferenced; entries above pos[b] >> 7 may hold
    anything.  Returns [B, 1, Hq*D]."""
    return _decode_paged(q, k, v, cos, sin, k_pool, v_pool, table, pos, num_heads, scale, False)


def decode_attention_verify_paged_supported(q: torch.Tensor, cos: torch.Tensor, k_pool: torch.Tensor,
                                            v_pool: torch.Tensor, table, pos, num_heads: int) -> bool:
    """What qz_decode_attention_verify_paged takes: T >= 2 new tokens per stream (q [B, T, *]),
    decode_attention_paged_supported's pools, table and pos, and cos/sin [B, T, D] whose B T rows lie
    at one stride.  Metadata only: nothing is launched or allocated."""
    return _verify_paged_supported(q, cos, k_pool, v_pool, table, pos, num_heads, False)


def decode_attention_verify_paged(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor,
                                  sin: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, table: torch.Tensor,
                                  pos: torch.Tensor, num_heads: int, scale: float) -> torch.Tensor:
    """decode_attention_verify through a page table (qz_decode_attention_verify_paged): token (b, i)
    sits at position pos[b] + i, writes through table[b, (pos[b] + i) >> 7] and sees keys
    0..pos[b] + i.  Bits are decode_attention_verify's on the gathered cache; a row that needs an
    entry outside [0, P) is NaN and a row whose write entry is invalid writes nothing.  Returns
    [B, T, Hq*D]."""
    return _verify_paged(q, k, v, cos, sin, k_pool, v_pool, table, pos, num_heads, scale, False)


def prefill_attention_paged_supported(q: torch.Tensor, cos: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor,
                                      table, pos, length, num_heads: int) -> bool:
    """What qz_prefill_attention_paged takes: T >= 1 new tokens per stream (q [B, T, *]),
    decode_attention_paged_supported's pools, table and pos, cos/sin [B or 1, T, D] with unit inner
    stride and an int64 length [B].  Metadata only: nothing is launched or allocated."""
    return _prefill_paged_supported(q, cos, k_pool, v_pool, table, pos, length, num_heads, False)


def prefill_attention_paged(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                            k_pool: torch.Tensor, v_pool: torch.Tensor, table: torch.Tensor, pos: torch.Tensor,
                            length: torch.Tensor, num_heads: int, scale: float) -> torch.Tensor:
    """prefill_attention through a page table (qz_prefill_attention_paged): token (b, i) with
    i < length[b] sits at position pos[b] + i, writes through table[b, (pos[b] + i) >> 7] and sees keys
    0..pos[b] + i; a 64-key tile's base comes from table[b, tile >> 1].  Bits are prefill_attention's
    on the gathered cache, so a window split into several calls equals the whole window.  A row that
    needs an entry outside [0, P) is NaN; a row whose write entry is invalid writes nothing.  Returns
    [B, T, Hq*D]."""
    return _prefill_paged(q, k, v, cos, sin, k_pool, v_pool, table, pos, length, num_heads, scale, False)


def decode_attention_paged_kv8_supported(q: torch.Tensor, cos: torch.Tensor, k_pool: torch.Tensor,
                                         v_pool: torch.Tensor, table, pos, num_heads: int) -> bool:
    """What qz_decode_attention_paged_kv8 takes: decode_attention_paged_supported's operands with kv8
    pools, uint8 [P, Hkv, 128 (D + 1)] with D in {64, 128}, contiguous and 16-B aligned, in place of the
    16-bit ones.  Metadata only."""
    return _decode_paged_supported(q, cos, k_pool, v_pool, table, pos, num_heads, True)


def decode_attention_paged_kv8(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor,
                               sin: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, table: torch.Tensor,
                               pos: torch.Tensor, num_heads: int, scale: float) -> torch.Tensor:
    """decode_attention_paged over kv8 pools (qz_decode_attention_paged_kv8): a cache row is D E4M3
    codes and a power-of-two scale byte.  The new token's rotated k and its v are quantised, stored,
    and scored as they will read back, so the output carries the bits of decode_attention_paged with
    identity cos/sin on the dequantised pools, the rotated q and the dequantised new rows.  Validity
    rules are decode_attention_paged's.  Returns [B, 1, Hq*D]."""
    return _decode_paged(q, k, v, cos, sin, k_pool, v_pool, table, pos, num_heads, scale, True)


def decode_attention_verify_paged_kv8_supported(q: torch.Tensor, cos: torch.Tensor, k_pool: torch.Tensor,
                                                v_pool: torch.Tensor, table, pos, num_heads: int) -> bool:
    """What qz_decode_attention_verify_paged_kv8 takes: decode_attention_verify_paged_supported's
    operands with kv8 pools.  Metadata only."""
    return _verify_paged_supported(q, cos, k_pool, v_pool, table, pos, num_heads, True)


def decode_attention_verify_paged_kv8(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor,
                                      sin: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor,
                                      table: torch.Tensor, pos: torch.Tensor, num_heads: int,
                                      scale: float) -> torch.Tensor:
    """decode_attention_verify_paged over kv8 pools (qz_decode_attention_verify_paged_kv8): the T new
    rows of every stream are rotated, quantised and stored first, then every token reads its keys,
    slot pos[b] + i included, from the pools.  One call equals T successive decode_attention_paged_kv8
    calls in outputs and pool bytes.  Returns [B, T, Hq*D]."""
    return _verify_paged(q, k, v, cos, sin, k_pool, v_pool, table, pos, num_heads, scale, True)


def prefill_attention_paged_kv8_supported(q: torch.Tensor, cos: torch.Tensor, k_pool: torch.Tensor,
                                          v_pool: torch.Tensor, table, pos, length, num_heads: int) -> bool:
    """What qz_prefill_attention_paged_kv8 takes: prefill_attention_paged_supported's operands with kv8
    pools.  Metadata only."""
    return _prefill_paged_supported(q, cos, k_pool, v_pool, table, pos, length, num_heads, True)


def prefill_attention_paged_kv8(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor,
                                sin: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, table: torch.Tensor,
                                pos: torch.Tensor, length: torch.Tensor, num_heads: int, scale: float) -> torch.Tensor:
    """prefill_attention_paged over kv8 pools (qz_prefill_attention_paged_kv8): the window's rows are
    rotated, quantised and stored, then the tile kernel converts the codes it loads to the 16-bit
    operands of its MFMAs.  A window split into several calls equals the whole window.  Returns
    [B, T, Hq*D]."""
    return _prefill_paged(q, k, v, cos, sin, k_pool, v_pool, table, pos, length, num_heads, scale, True)


def _check_window(name: str, q, k, v, cos, sin, num_heads: int, D: int) -> None:
    """What every window launch (verify, prefill; contiguous or paged) asks of q / k / v [B, T, *] and sin
    beyond its _supported predicate."""
    if q.shape[2] != num_heads * D:
        raise ValueError(f"{name}: q width differs from num_heads * head_dim")
    if sin.shape != cos.shape or sin.stride() != cos.stride() or sin.dtype != cos.dtype:
        raise ValueError(f"{name}: sin must match cos")
    if k.shape[:2] != q.shape[:2] or v.shape[:2] != q.shape[:2]:
        raise ValueError(f"{name}: k/v must hold q's [B, T] rows")


def _verify_rows(name: str, q, k, v, kv_width: int, owner: str):
    """q / k / v [B, T, *] as the B T rows the verify launches take: unit inner stride, v in 4-B words.
    `owner` names what k / v's width is checked against in the error text."""
    R = q.shape[0] * q.shape[1]
    q2, k2, v2 = (t.reshape(R, -1) for t in (q, k, v))
    k2 = k2 if k2.stride(-1) == 1 else k2.contiguous()
    q2 = q2 if q2.stride(-1) == 1 else q2.contiguous()
    if v2.stride(-1) != 1 or v2.stride(0) % 2 or v2.data_ptr() % 4:
        v2 = v2.contiguous()
    if k2.shape[1] != kv_width or v2.shape[1] != kv_width:
        raise ValueError(f"{name}: k/v width differs from the {owner} heads")
    return q2, k2, v2


def _prefill_rows(q, k, v, cos, sin, B: int, T: int, D: int):
    """The row views of the prefill launches: (q, stride, k, stride, v, stride, cos, sin, their stride)."""
    q2, qs = _token_rows(q, B, T, 16, 8)
    k2, ks = _token_rows(k, B, T, 2, 1)
    v2, vs = _token_rows(v, B, T, 4, 2)
    c2, cs = _token_rows(cos, B, T, 16, 8)
    s2, ss = _token_rows(sin, B, T, 16, 8)
    if ss != cs:
        s2, c2 = s2.contiguous(), c2.contiguous()
        cs = D
    return q2, qs, k2, ks, v2, vs, c2, s2, cs


def _token_rows(t: torch.Tensor, B: int, T: int, align: int, mult: int):
    """[B or 1, T, W] as B T rows at one stride (a multiple of `mult` elements) from an `align`-byte
    base: prefill_attention's row-view rule.  Returns (tensor, row stride)."""
    W = t.shape[2]
    if t.shape[0] != B:
        t = t.expand(B, -1, -1)
    t = t.reshape(B * T, W)   # a view where the rows lie at one stride, a copy otherwise
    if B * T == 1 and t.stride(-1) == 1 and t.data_ptr() % align == 0:
        return t, W
    if t.stride(-1) != 1 or t.stride(0) < W or t.stride(0) % mult or t.data_ptr() % align:
        t = t.contiguous()
    return t, t.stride(0)


def decode_mask(q_offset: torch.Tensor, batch: int, kv_length: int) -> torch.Tensor:
    """masking_utils.create_causal_mask's sdpa mask for one new token per sequence against a static
    cache (no padding mask, kv_offset 0): bool [batch, 1, 1, kv_length], True where kv position
    j <= q_offset (StaticLayer.cumulative_length, a device int64 read in-kernel)."""
    if not (q_offset.is_cuda and q_offset.dtype == torch.int64 and q_offset.numel() == 1):
        raise ValueError("decode_mask: q_offset must be one int64 on the GPU")
    mask = torch.empty((batch, 1, 1, kv_length), dtype=torch.bool, device=q_offset.device)
    _lib.check(_lib.lib.qz_decode_mask(q_offset.data_ptr(), batch, kv_length, mask.data_ptr(),
                                       _lib.stream_of(q_offset)), "qz_decode_mask")
    return mask


def rope_table(position_ids: torch.Tensor, cos_t: torch.Tensor, sin_t: torch.Tensor, inv_freq: torch.Tensor,
               scale: float):
    """LlamaRotaryEmbedding.forward from tables: cos/sin [B, S, D] of position_ids [B, S] (int64)
    copied from cos_t/sin_t [T, D] (what the module computed for positions 0..T-1); positions
    outside the table computed in-kernel from inv_freq (fp32) and scale."""
    if not (position_ids.is_cuda and position_ids.dtype == torch.int64 and position_ids.dim() == 2):
        raise ValueError("rope_table: position_ids must be int64 [B, S] on the GPU")
    T, D = cos_t.shape
    if sin_t.shape != cos_t.shape or sin_t.dtype != cos_t.dtype or not (cos_t.is_contiguous() and sin_t.is_contiguous()):
        raise ValueError("rope_table: cos/sin tables must be contiguous [T, D] of one dtype")
    if inv_freq.dtype != torch.float32 or inv_freq.numel() * 2 != D or not inv_freq.is_contiguous():
        raise ValueError("rope_table: inv_freq must be contiguous fp32 [D / 2]")
    B, S = position_ids.shape
    cos = torch.empty((B, S, D), dtype=cos_t.dtype, device=position_ids.device)
    sin = torch.empty_like(cos)
    _lib.check(_lib.lib.qz_rope_table(_lib.dtype_code(cos_t.dtype), B, S, D, position_ids.data_ptr(),
                                      position_ids.stride(0), position_ids.stride(1), cos_t.data_ptr(),
                                      sin_t.data_ptr(), T, inv_freq.data_ptr(), float(scale), cos.data_ptr(),
                                      sin.data_ptr(), _lib.stream_of(position_ids)), "qz_rope_table")
    return cos, sin


def greedy_step(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, tok: torch.Tensor) -> None:
    """A decode loop's greedy pick and feedback in two launches (qz_greedy_step): next = logits.argmax(-1) (torch's
    order: NaN first, then the largest, the first index among equals) for logits [B, V] (rows of
    any stride, unit element stride); hist[b, pos] = next[b]; tok[b] = next[b]; pos += 1.  hist
    [B, H] contiguous int64, pos one int64, tok B contiguous int64, all on the logits' GPU."""
    if logits.dim() != 2 or logits.stride(-1) != 1 or not logits.is_cuda:
        raise ValueError("greedy_step: logits must be [B, V] on the GPU with unit element stride")
    B, V = logits.shape
    for t in (hist, pos, tok):
        if t.dtype != torch.int64 or t.device != logits.device or not t.is_contiguous():
            raise ValueError("greedy_step: hist/pos/tok must be contiguous int64 on the logits' device")
    if hist.dim() != 2 or hist.shape[0] != B or pos.numel() != 1 or tok.numel() != B:
        raise ValueError("greedy_step: hist [B, H], pos [1], tok [B]")
    work = torch.empty(_lib.lib.qz_greedy_step_work_bytes(B, V), dtype=torch.uint8, device=logits.device)
    _lib.check(_lib.lib.qz_greedy_step(logits.data_ptr(), _lib.dtype_code(logits.dtype), B, V, logits.stride(0),
                                       hist.data_ptr(), hist.shape[1], hist.shape[1], pos.data_ptr(), tok.data_ptr(),
                                       work.data_ptr(), _lib.stream_of(logits)), "qz_greedy_step")


DENSE_K = (4096, 8192)   # the widths qz_gemv_dense takes (Llama-3 8B / 70B)


def gemv_dense_supported(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """One token through an unquantised fp16/bf16 [M, K] weight (the lm_head) with qz_gemv_dense."""
    if _needs_grad(x) or not (x.is_cuda and weight.is_cuda and x.device == weight.device and x.dtype == weight.dtype
                              and x.dtype in (torch.float16, torch.bfloat16) and weight.dim() == 2
                              and weight.is_contiguous()):
        return False
    K = weight.shape[1]
    return (K in DENSE_K and x.shape[-1] == K and x.numel() == K and x.is_contiguous()
            and x.data_ptr() % 16 == 0 and weight.data_ptr() % 16 == 0 and weight.shape[0] < 2 ** 31)


def gemv_dense(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """F.linear(x, weight) for one token ([..., K] with one row) -- fp32 accumulation, rounded once
    (the library's numerics class; the summation order differs)."""
    if not gemv_dense_supported(x, weight):
        raise ValueError("gemv_dense: unsupported shapes/dtypes/layout")
    M, K = weight.shape
    y = torch.empty((*x.shape[:-1], M), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib.qz_gemv_dense(M, K, x.data_ptr(), _lib.dtype_code(x.dtype), weight.data_ptr(), y.data_ptr(),
                                      _lib.stream_of(x)), "qz_gemv_dense")
    return y


def sample_step_supported(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, tok: torch.Tensor,
                          temperature: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
                          uniform: torch.Tensor) -> bool:
    """What qz_sample_step takes: fp16 / bf16 logits [B, V] on the GPU with unit element stride, and
    the buffers sample_step documents, contiguous on the same device.  Metadata only: nothing is
    launched or allocated."""
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype in (torch.float16, torch.bfloat16)
            and logits.dim() == 2 and logits.stride(-1) == 1 and logits.stride(0) >= logits.shape[1]):
        return False
    B = logits.shape[0]
    if B > 65535:
        return False
    for t, dt in ((hist, torch.int64), (pos, torch.int64), (tok, torch.int64), (temperature, torch.float32),
                  (top_k, torch.int32), (top_p, torch.float32), (uniform, torch.float32)):
        if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.device == logits.device and t.is_contiguous()):
            return False
    return (hist.dim() == 2 and hist.shape[0] == B and uniform.shape == hist.shape and pos.numel() == 1
            and tok.numel() == B and temperature.shape == top_k.shape == top_p.shape == (B,))


def _sample_step_composed(logits, hist, pos, tok, temperature, top_k, top_p, uniform) -> None:
    """qz_sample_step's semantics in torch ops (sort-based, fp32, no host read: capturable)."""
    B, V = logits.shape
    H = hist.shape[1]
    z = logits.float()
    ninf = torch.full((), float("-inf"), device=z.device)
    zmax = z.max(dim=1).values                                             # NaN if the row holds one
    greedy = ~(temperature > 0) | ~torch.isfinite(zmax)
    T = torch.where(temperature > 0, temperature, torch.ones_like(temperature))
    s = torch.where(torch.isneginf(z), ninf, z / T[:, None])
    vals, _ = s.sort(dim=1, descending=True)
    kon = (top_k >= 1) & (top_k < V)
    kth = vals.gather(1, (top_k.long().clamp(1, V) - 1)[:, None])
    s = torch.where(~kon[:, None] | (s >= kth), s, ninf)
    vals = torch.where(~kon[:, None] | (vals >= kth), vals, ninf)
    smax = vals[:, :1]
    ws = torch.exp(vals - smax)
    cum = ws.cumsum(1)
    Z = cum[:, -1:]
    first = torch.ones_like(vals, dtype=torch.bool)
    first[:, 1:] = vals[:, 1:] != vals[:, :-1]
    above = torch.where(first, cum - ws, torch.zeros_like(cum)).cummax(1).values   # mass strictly above
    keep_sorted = (vals > ninf) & ((top_p >= 1)[:, None] | (above < top_p[:, None] * Z) | (vals == smax))
    cut = torch.where(keep_sorted, vals, torch.full_like(vals, float("inf"))).min(dim=1, keepdim=True).values
    w = torch.where((s >= cut) & (s > ninf), torch.exp(s - smax), torch.zeros_like(s))
    cdf = w.cumsum(1)
    p = pos.reshape(1)
    col = p.clamp(0, max(H - 1, 0))              # a [1] index tensor: index_select / index_copy_ read it on the device
    u = uniform.index_select(1, col)[:, 0] if H else torch.zeros(B, device=z.device)
    hit = cdf > (u * cdf[:, -1])[:, None]
    last = (V - 1) - (w.flip(1) > 0).int().argmax(1)
    pick = torch.where(hit.any(1), hit.int().argmax(1), last)
    token = torch.where(greedy, logits.argmax(-1), pick)
    if H:
        inside = (p >= 0) & (p < H)
        hist.index_copy_(1, col, torch.where(inside, token, hist.index_select(1, col)[:, 0])[:, None])
    tok.copy_(token.view(tok.shape))
    pos.add_(1)


def sample_step(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, tok: torch.Tensor,
                temperature: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor, uniform: torch.Tensor,
                *, composed: bool = False) -> None:
    """A decode loop's sampled pick and feedback (qz_sample_step; include/quantizations.h states the
    rules): per stream b, temperature[b] <= 0 or a non-finite row maximum picks greedy_step's token;
    else scores logits / temperature, top_k[b] (ties at the threshold kept; outside [1, V): off),
    top_p[b] (tie groups whole, >= 1: off) and the inverse CDF in index order at
    uniform[b, min(pos, H - 1)].  Then hist[b, pos] = token, tok[b] = token, pos += 1.  logits [B, V]
    (unit element stride), temperature / top_p float32 [B], top_k int32 [B], uniform float32 [B, H],
    hist [B, H] / pos [1] / tok [B] contiguous int64, all on one device.  Every value is read on the
    device, so a captured call follows in-place changes.  fp32 or CPU logits (sample_step_supported
    is false), or composed=True, take the same rules in torch ops."""
    if logits.dim() != 2 or logits.stride(-1) != 1:
        raise ValueError("sample_step: logits must be [B, V] with unit element stride")
    B, V = logits.shape
    for t in (hist, pos, tok):
        if t.dtype != torch.int64 or t.device != logits.device or not t.is_contiguous():
            raise ValueError("sample_step: hist/pos/tok must be contiguous int64 on the logits' device")
    if hist.dim() != 2 or hist.shape[0] != B or pos.numel() != 1 or tok.numel() != B:
        raise ValueError("sample_step: hist [B, H], pos [1], tok [B]")
    for t, dt, name in ((temperature, torch.float32, "temperature"), (top_k, torch.int32, "top_k"),
                        (top_p, torch.float32, "top_p")):
        if t.dtype != dt or t.device != logits.device or t.shape != (B,) or not t.is_contiguous():
            raise ValueError(f"sample_step: {name} must be contiguous {dt} [B] on the logits' device")
    if (uniform.dtype != torch.float32 or uniform.device != logits.device or uniform.shape != hist.shape
            or not uniform.is_contiguous()):
        raise ValueError("sample_step: uniform must be contiguous float32 [B, H] on the logits' device")
    if composed or not sample_step_supported(logits, hist, pos, tok, temperature, top_k, top_p, uniform):
        if V:
            _sample_step_composed(logits, hist, pos, tok, temperature, top_k, top_p, uniform)
        return
    work = torch.empty(_lib.lib.qz_sample_step_work_bytes(B, V), dtype=torch.uint8, device=logits.device)
    _lib.check(_lib.lib.qz_sample_step(logits.data_ptr(), _lib.dtype_code(logits.dtype), B, V, logits.stride(0),
                                       temperature.data_ptr(), top_k.data_ptr(), top_p.data_ptr(),
                                       uniform.data_ptr(), uniform.shape[1], hist.data_ptr(), hist.shape[1],
                                       hist.shape[1], pos.data_ptr(), tok.data_ptr(), work.data_ptr(),
                                       _lib.stream_of(logits)), "qz_sample_step")


def _check_streams(name, logits, hist, pos, live, stop, limit, tok):
    if logits.dim() != 2 or logits.stride(-1) != 1:
        raise ValueError(f"{name}: logits must be [B, V] with unit element stride")
    B = logits.shape[0]
    for t, dt, what in ((hist, torch.int64, "hist"), (pos, torch.int64, "pos"), (tok, torch.int64, "tok"),
                        (live, torch.int32, "live"), (stop, torch.int64, "stop"), (limit, torch.int64, "limit")):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != logits.device or not t.is_contiguous():
            raise ValueError(f"{name}: {what} must be contiguous {dt} on the logits' device")
    if hist.dim() != 2 or hist.shape[0] != B or tok.numel() != B:
        raise ValueError(f"{name}: hist [B, H], tok [B]")
    for t, what in ((pos, "pos"), (live, "live"), (stop, "stop"), (limit, "limit")):
        if t.shape != (B,):
            raise ValueError(f"{name}: {what} must be [B]")


def _feedback_streams(token, hist, pos, live, stop, limit, tok) -> None:
    """The per-stream feedback of qz_*_step_streams in torch ops (gather / scatter over pos, no host read)."""
    B, H = hist.shape
    alive = live != 0
    p = pos.clone()
    if H:
        col = p.clamp(0, H - 1)[:, None]
        inside = alive & (p >= 0) & (p < H)
        hist.scatter_(1, col, torch.where(inside, token, hist.gather(1, col)[:, 0])[:, None])
    tok.copy_(torch.where(alive, token, tok.view(-1)).view(tok.shape))
    pos.copy_(torch.where(alive, p + 1, p))
    live.copy_(torch.where(alive & ((token == stop) | (p + 1 >= limit)), torch.zeros_like(live), live))


def _greedy_step_streams_composed(logits, hist, pos, live, stop, limit, tok) -> None:
    _feedback_streams(logits.argmax(-1), hist, pos, live, stop, limit, tok)


def _sample_step_streams_composed(logits, hist, pos, live, stop, limit, tok, temperature, top_k, top_p,
                                  uniform) -> None:
    """Each row through _sample_step_composed's rules at its own position: the uniform number is
    gathered at pos[b] into a one-column table, the pick lands in scratch, the feedback follows."""
    B, H = hist.shape
    if H:
        u = uniform.gather(1, pos.clamp(0, H - 1)[:, None])
    else:
        u = torch.zeros((B, 1), dtype=torch.float32, device=logits.device)
    token = torch.zeros(B, dtype=torch.int64, device=logits.device)
    _sample_step_composed(logits, torch.zeros((B, 1), dtype=torch.int64, device=logits.device),
                          torch.zeros(1, dtype=torch.int64, device=logits.device), token, temperature, top_k, top_p, u)
    _feedback_streams(token, hist, pos, live, stop, limit, tok)


def greedy_step_streams(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, live: torch.Tensor,
                        stop: torch.Tensor, limit: torch.Tensor, tok: torch.Tensor, *, composed: bool = False) -> None:
    """greedy_step with the feedback per stream (qz_greedy_step_streams): pos / stop / limit int64
    [B], live int32 [B].  A live stream b picks greedy_step's token for its row, writes
    hist[b, pos[b]] and tok[b], advances pos[b], then clears live[b] if the token is stop[b] (-1:
    none) or pos[b] reached limit[b]; a stream that is not live has nothing written.  CPU logits,
    or composed=True, take the same rules in torch ops."""
    _check_streams("greedy_step_streams", logits, hist, pos, live, stop, limit, tok)
    B, V = logits.shape
    if composed or not logits.is_cuda:
        if B and V:
            _greedy_step_streams_composed(logits, hist, pos, live, stop, limit, tok)
        return
    work = torch.empty(_lib.lib.qz_greedy_step_work_bytes(B, V), dtype=torch.uint8, device=logits.device)
    _lib.check(_lib.lib.qz_greedy_step_streams(
        logits.data_ptr(), _lib.dtype_code(logits.dtype), B, V, logits.stride(0), hist.data_ptr(), hist.shape[1],
        hist.shape[1], pos.data_ptr(), live.data_ptr(), stop.data_ptr(), limit.data_ptr(), tok.data_ptr(),
        work.data_ptr(), _lib.stream_of(logits)), "qz_greedy_step_streams")


def sample_step_streams(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, live: torch.Tensor,
                        stop: torch.Tensor, limit: torch.Tensor, tok: torch.Tensor, temperature: torch.Tensor,
                        top_k: torch.Tensor, top_p: torch.Tensor, uniform: torch.Tensor, *,
                        composed: bool = False) -> None:
    """sample_step with the feedback per stream (qz_sample_step_streams): a live stream b picks what
    sample_step picks for its row alone at pos = pos[b] (uniform[b, min(pos[b], H - 1)]), then the
    feedback of greedy_step_streams.  fp32 or CPU logits, or composed=True, take the same rules in
    torch ops."""
    _check_streams("sample_step_streams", logits, hist, pos, live, stop, limit, tok)
    B, V = logits.shape
    for t, dt, name in ((temperature, torch.float32, "temperature"), (top_k, torch.int32, "top_k"),
                        (top_p, torch.float32, "top_p")):
        if t.dtype != dt or t.device != logits.device or t.shape != (B,) or not t.is_contiguous():
            raise ValueError(f"sample_step_streams: {name} must be contiguous {dt} [B] on the logits' device")
    if (uniform.dtype != torch.float32 or uniform.device != logits.device or uniform.shape != hist.shape
            or not uniform.is_contiguous()):
        raise ValueError("sample_step_streams: uniform must be contiguous float32 [B, H] on the logits' device")
    if (composed or not logits.is_cuda or logits.dtype not in (torch.float16, torch.bfloat16)
            or logits.stride(0) < V or B > 65535):
        if B and V:
            _sample_step_streams_composed(logits, hist, pos, live, stop, limit, tok, temperature, top_k, top_p,
                                          uniform)
        return
    work = torch.empty(_lib.lib.qz_sample_step_work_bytes(B, V), dtype=torch.uint8, device=logits.device)
    _lib.check(_lib.lib.qz_sample_step_streams(
        logits.data_ptr(), _lib.dtype_code(logits.dtype), B, V, logits.stride(0), temperature.data_ptr(),
        top_k.data_ptr(), top_p.data_ptr(), uniform.data_ptr(), uniform.shape[1], hist.data_ptr(), hist.shape[1],
        hist.shape[1], pos.data_ptr(), live.data_ptr(), stop.data_ptr(), limit.data_ptr(), tok.data_ptr(),
        work.data_ptr(), _lib.stream_of(logits)), "qz_sample_step_streams")


VERIFY_MAX_T = 16   # kVerifyMaxT (csrc/layer_ops.hip): rows per stream of verify_step_streams / ngram_draft
NGRAM_MAX = 4       # the longest suffix ngram_draft looks up


def _check_verify(name, logits, hist, pos, live, stop, limit, tok, accepted):
    if logits.dim() != 2 or logits.stride(-1) != 1:
        raise ValueError(f"{name}: logits must be [B*T, V] with unit element stride")
    for t, dt, what in ((hist, torch.int64, "hist"), (pos, torch.int64, "pos"), (tok, torch.int64, "tok"),
                        (live, torch.int32, "live"), (stop, torch.int64, "stop"), (limit, torch.int64, "limit"),
                        (accepted, torch.int32, "accepted")):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != logits.device or not t.is_contiguous():
            raise ValueError(f"{name}: {what} must be contiguous {dt} on the logits' device")
    if tok.dim() != 2 or not 1 <= tok.shape[1] <= VERIFY_MAX_T:
        raise ValueError(f"{name}: tok must be [B, T] with T <= {VERIFY_MAX_T}")
    B, T = tok.shape
    if logits.shape[0] != B * T or hist.dim() != 2 or hist.shape[0] != B:
        raise ValueError(f"{name}: logits [B*T, V], hist [B, H]")
    for t, what in ((pos, "pos"), (live, "live"), (stop, "stop"), (limit, "limit"), (accepted, "accepted")):
        if t.shape != (B,):
            raise ValueError(f"{name}: {what} must be [B]")


def _verify_step_streams_composed(logits, hist, pos, live, stop, limit, tok, accepted) -> None:
    """qz_verify_step_streams' rules in torch ops (no host read): T masked rounds of _feedback_streams."""
    _accept_streams(logits.argmax(-1).view(tok.shape), hist, pos, live, stop, limit, tok, accepted)


def _verify_sample_step_streams_composed(logits, hist, pos, live, stop, limit, tok, accepted, temperature, top_k,
                                         top_p, uniform) -> None:
    """qz_verify_sample_step_streams' rules in torch ops (no host read): every row of the window
    through _sample_step_composed with its stream's parameters and the uniform number of position
    pos[b] + i (a one-column table, as _sample_step_streams_composed builds it), then the accept loop."""
    B, T = tok.shape
    H = hist.shape[1]
    R, dev = B * T, logits.device
    if H:
        cols = (pos[:, None] + torch.arange(T, device=dev)[None, :]).clamp(0, H - 1)
        u = uniform.gather(1, cols).reshape(R, 1)
    else:
        u = torch.zeros((R, 1), dtype=torch.float32, device=dev)
    token = torch.zeros(R, dtype=torch.int64, device=dev)
    _sample_step_composed(logits, torch.zeros((R, 1), dtype=torch.int64, device=dev),
                          torch.zeros(1, dtype=torch.int64, device=dev), token,
                          *(t[:, None].expand(B, T).reshape(R) for t in (temperature, top_k, top_p)), u)
    _accept_streams(token.view(B, T), hist, pos, live, stop, limit, tok, accepted)


def _accept_streams(g, hist, pos, live, stop, limit, tok, accepted) -> None:
    """The accept loop of the verify picks over the rows' tokens g [B, T] (no host read)."""
    B, T = tok.shape
    H = hist.shape[1]
    going = live != 0
    p, lv, last = pos.clone(), live.clone(), tok[:, 0].clone()
    n = torch.zeros_like(accepted)
    for i in range(T):
        gi = g[:, i]
        if H:
            col = p.clamp(0, H - 1)[:, None]
            inside = going & (p >= 0) & (p < H)
            hist.scatter_(1, col, torch.where(inside, gi, hist.gather(1, col)[:, 0])[:, None])
        p = torch.where(going, p + 1, p)
        n = n + going.to(n.dtype)
        last = torch.where(going, gi, last)
        ended = going & ((gi == stop) | (p >= limit))
        lv = torch.where(ended, torch.zeros_like(lv), lv)
        if i + 1 < T:
            going = going & ~ended & (tok[:, i + 1] == gi)
    pos.copy_(p)
    live.copy_(lv)
    tok[:, 0] = last
    accepted.copy_(n)


def verify_step_streams(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, live: torch.Tensor,
                        stop: torch.Tensor, limit: torch.Tensor, tok: torch.Tensor, accepted: torch.Tensor, *,
                        composed: bool = False) -> None:
    """The greedy pick that accepts drafts (qz_verify_step_streams).  tok int64 [B, T]: column 0 the
    token that was fed, columns 1.. the drafts; logits [B*T, V], row b*T + i the model's output after
    tok[b, :i + 1]; g_i its greedy_step pick.  A live stream does what successive
    greedy_step_streams calls would: for i = 0, 1, ...: hist[b, pos[b]] = g_i, pos[b] += 1; it leaves
    (live[b] = 0) and ends on its stop token or at its limit; it ends after row T - 1 or when draft
    tok[b, i + 1] is not g_i.  tok[b, 0] becomes the last token emitted and accepted[b] (int32 [B]) the
    number emitted; a stream that is not live has accepted[b] = 0 and nothing else written.  An
    emitted row i has pos[b] + i + 1 <= limit[b], so with limit[b] <= L - 1 no row past the cache of
    decode_attention_verify is ever emitted.  CPU logits, or composed=True, take the same rules in
    torch ops."""
    _check_verify("verify_step_streams", logits, hist, pos, live, stop, limit, tok, accepted)
    B, T = tok.shape
    V = logits.shape[1]
    if composed or not logits.is_cuda:
        if B and V:
            _verify_step_streams_composed(logits, hist, pos, live, stop, limit, tok, accepted)
        return
    work = torch.empty(_lib.lib.qz_greedy_step_work_bytes(B * T, V), dtype=torch.uint8, device=logits.device)
    _lib.check(_lib.lib.qz_verify_step_streams(
        logits.data_ptr(), _lib.dtype_code(logits.dtype), B, T, V, logits.stride(0), hist.data_ptr(), hist.shape[1],
        hist.shape[1], pos.data_ptr(), live.data_ptr(), stop.data_ptr(), limit.data_ptr(), tok.data_ptr(),
        accepted.data_ptr(), work.data_ptr(), _lib.stream_of(logits)), "qz_verify_step_streams")


def verify_sample_step_streams(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, live: torch.Tensor,
                               stop: torch.Tensor, limit: torch.Tensor, tok: torch.Tensor, accepted: torch.Tensor,
                               temperature: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
                               uniform: torch.Tensor, *, composed: bool = False) -> None:
    """The sampled pick that accepts drafts (qz_verify_sample_step_streams): verify_step_streams with
    g_i := s_i, the token sample_step_streams picks for row b*T + i alone with stream b's
    temperature / top_k / top_p ([B]) at position pos[b] + i, i.e. with
    uniform[b, min(max(pos[b] + i, 0), H - 1)] (pos as it is before the call).  s_i depends on the row
    and on that number alone, so the emitted tokens are those of successive sample_step_streams calls
    over the same `uniform` whatever the drafts were; a stream with temperature <= 0 gets
    verify_step_streams' result.  fp32 or CPU logits, or composed=True, take the same rules in torch
    ops."""
    name = "verify_sample_step_streams"
    _check_verify(name, logits, hist, pos, live, stop, limit, tok, accepted)
    B, T = tok.shape
    V = logits.shape[1]
    for t, dt, what in ((temperature, torch.float32, "temperature"), (top_k, torch.int32, "top_k"),
                        (top_p, torch.float32, "top_p")):
        if (not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != logits.device or t.shape != (B,)
                or not t.is_contiguous()):
            raise ValueError(f"{name}: {what} must be contiguous {dt} [B] on the logits' device")
    if (not isinstance(uniform, torch.Tensor) or uniform.dtype != torch.float32 or uniform.device != logits.device
            or uniform.shape != hist.shape or not uniform.is_contiguous()):
        raise ValueError(f"{name}: uniform must be contiguous float32 [B, H] on the logits' device")
    if (composed or not logits.is_cuda or logits.dtype not in (torch.float16, torch.bfloat16)
            or logits.stride(0) < V or B * T > 65535):
        if B and V:
            _verify_sample_step_streams_composed(logits, hist, pos, live, stop, limit, tok, accepted, temperature,
                                                 top_k, top_p, uniform)
        return
    work = torch.empty(_lib.lib.qz_verify_sample_step_work_bytes(B, T, V), dtype=torch.uint8, device=logits.device)
    _lib.check(_lib.lib.qz_verify_sample_step_streams(
        logits.data_ptr(), _lib.dtype_code(logits.dtype), B, T, V, logits.stride(0), temperature.data_ptr(),
        top_k.data_ptr(), top_p.data_ptr(), uniform.data_ptr(), uniform.shape[1], hist.data_ptr(), hist.shape[1],
        hist.shape[1], pos.data_ptr(), live.data_ptr(), stop.data_ptr(), limit.data_ptr(), tok.data_ptr(),
        accepted.data_ptr(), work.data_ptr(), _lib.stream_of(logits)), "qz_verify_sample_step_streams")


_PROCESS_PARAMS = (("repetition_penalty", torch.float32), ("presence_penalty", torch.float32),
                   ("frequency_penalty", torch.float32), ("no_repeat_ngram", torch.int32),
                   ("min_new_tokens", torch.int64), ("prompt_len", torch.int64), ("eos", torch.int64))


def process_logits_supported(logits: torch.Tensor) -> bool:
    """What qz_logits_process takes: fp16 / bf16 logits [R, V] on the GPU with unit element stride and
    a row stride of at least V, at most 65535 rows.  Metadata only."""
    return (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype in (torch.float16, torch.bfloat16)
            and logits.dim() == 2 and logits.stride(-1) == 1 and logits.stride(0) >= logits.shape[1]
            and logits.shape[0] <= 65535 and logits.shape[1] < 2 ** 31)


def _process_logits_composed(logits, hist, pos, tok, T, params) -> None:
    """qz_logits_process' rules with the bookkeeping on the host (one read of hist, pos, tok and the
    parameters) and the arithmetic in torch ops on the logits' device: the same fp32 operations,
    rounded once to the logits' dtype (for fp32 logits that rounding is the identity)."""
    B, H = hist.shape
    V = logits.shape[1]
    h_all, ps = hist.cpu().tolist(), pos.cpu().reshape(-1).tolist()
    drafts = tok.cpu().reshape(B, T).tolist() if tok is not None else None
    host = {k: (v.cpu().tolist() if v is not None else None) for k, v in params.items()}

    def val(name, b, default):
        return default if host[name] is None else host[name][b]

    dev = logits.device
    ninf = float("-inf")
    for b in range(B):
        p = ps[b if len(ps) > 1 else 0]
        if not 0 <= p < H:
            continue
        rp, pp, fp = val("repetition_penalty", b, 1.0), val("presence_penalty", b, 0.0), val("frequency_penalty", b, 0.0)
        g, pl = val("no_repeat_ngram", b, 0), val("prompt_len", b, 0)
        mn = val("min_new_tokens", b, 0) if host["eos"] is not None else 0
        pen = rp != 1.0 or pp != 0.0 or fp != 0.0
        if not pen and g <= 0 and mn <= 0:
            continue
        for i in range(T):
            h = h_all[b][:p + 1] + (drafts[b][1:i + 1] if i else [])
            n = len(h)
            row = logits[b * T + i]
            banned = set()
            if 1 <= g <= n:
                tail = h[n - g + 1:]
                banned = {h[k + g - 1] for k in range(n - g + 1) if h[k:k + g - 1] == tail}
            if mn > 0 and n - pl < mn:
                banned.add(host["eos"][b])
            banned = sorted(t for t in banned if 0 <= t < V)
            if pen:
                cnt = {}
                for k, t in enumerate(h):
                    if 0 <= t < V:
                        cnt[t] = cnt.get(t, 0) + (1 if k >= pl else 0)
                ids = torch.tensor(list(cnt.keys()), dtype=torch.int64, device=dev)
                c = torch.tensor(list(cnt.values()), dtype=torch.float32, device=dev)
                old = row[ids]
                x = old.float()
                f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)   # noqa: E731
                y = torch.where(x < 0, x * f32(rp), x / f32(rp)) if rp != 1.0 else x
                y = torch.where(c > 0, (y - f32(fp) * c) - f32(pp), y)
                out = torch.where(torch.isnan(y), torch.full_like(y, float("nan")), y).to(row.dtype)
                row[ids] = torch.where(torch.isnan(x), old, out)    # a NaN logit keeps its bits
            if banned:
                row[torch.tensor(banned, dtype=torch.int64, device=dev)] = ninf


def process_logits(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, tok: Optional[torch.Tensor] = None, *,
                   repetition_penalty: Optional[torch.Tensor] = None, presence_penalty: Optional[torch.Tensor] = None,
                   frequency_penalty: Optional[torch.Tensor] = None, no_repeat_ngram: Optional[torch.Tensor] = None,
                   min_new_tokens: Optional[torch.Tensor] = None, prompt_len: Optional[torch.Tensor] = None,
                   eos: Optional[torch.Tensor] = None, composed: bool = False) -> None:
    """The logits processors of a step, in place, in front of a pick (qz_logits_process;
    include/quantizations.h states the rules).  logits [B*T, V]; hist int64 [B, H] is the sequence
    itself (ngram_draft's operand, not the picks' shifted one); pos int64 [1] (one position for all) or
    [B]; tok int64 [B, T] (column 0 = hist[b, pos[b]], columns 1.. the drafts) -- None, or [B] / [B, 1],
    means T = 1.  Row (b, i) has the history hist[b, :pos[b] + 1] + tok[b, 1:i + 1].  Per stream, each
    None = off: repetition_penalty (transformers' rule, every distinct token of the history once),
    presence_penalty / frequency_penalty (float32 [B]; vLLM's rule over the tokens at indices >=
    prompt_len[b]), no_repeat_ngram (int32 [B]; banned tokens become -inf), min_new_tokens / prompt_len /
    eos (int64 [B]: eos[b] is -inf while fewer than min_new_tokens[b] tokens follow the prompt).
    Neutral values (1, 0, 0, 0, 0) leave every bit as it is.  Every value is read on the device, so a
    captured call follows in-place changes.  fp32 or CPU logits (process_logits_supported is false),
    or composed=True, take the same rules with the bookkeeping on the host (not capturable)."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.stride(-1) != 1:
        raise ValueError("process_logits: logits must be [B*T, V] with unit element stride")
    for t, what in ((hist, "hist"), (pos, "pos")) + (((tok, "tok"),) if tok is not None else ()):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.device != logits.device or not t.is_contiguous():
            raise ValueError(f"process_logits: {what} must be contiguous int64 on the logits' device")
    if hist.dim() != 2:
        raise ValueError("process_logits: hist must be [B, H]")
    B, H = hist.shape
    T = 1
    if tok is not None:
        if tok.dim() == 2 and tok.shape[0] == B:
            T = tok.shape[1]
        elif tok.shape != (B,):
            raise ValueError("process_logits: tok must be [B, T] (or [B])")
    if not 1 <= T <= VERIFY_MAX_T:
        raise ValueError(f"process_logits: T must be in 1..{VERIFY_MAX_T}")
    R, V = logits.shape
    if R != B * T or pos.numel() not in (1, B):
        raise ValueError("process_logits: logits [B*T, V], pos [1] or [B]")
    params = dict(repetition_penalty=repetition_penalty, presence_penalty=presence_penalty,
                  frequency_penalty=frequency_penalty, no_repeat_ngram=no_repeat_ngram, min_new_tokens=min_new_tokens,
                  prompt_len=prompt_len, eos=eos)
    for name, dt in _PROCESS_PARAMS:
        t = params[name]
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != logits.device
                              or t.shape != (B,) or not t.is_contiguous()):
            raise ValueError(f"process_logits: {name} must be contiguous {dt} [B] on the logits' device")
    if not (B and V):
        return
    if composed or not process_logits_supported(logits):
        _process_logits_composed(logits, hist, pos, tok if T > 1 else None, T, params)
        return
    work = torch.empty(_lib.lib.qz_logits_process_work_bytes(B, T, H), dtype=torch.uint8, device=logits.device)
    _lib.check(_lib.lib.qz_logits_process(
        logits.data_ptr(), _lib.dtype_code(logits.dtype), B, T, V, logits.stride(0), hist.data_ptr(), H, H,
        pos.data_ptr(), 0 if pos.numel() == 1 and B > 1 else 1, _lib.ptr(tok) if T > 1 else 0,
        *(_lib.ptr(params[name]) for name, _ in _PROCESS_PARAMS), work.data_ptr() if work.numel() else 0,
        _lib.stream_of(logits)), "qz_logits_process")


LOGPROBS_MAX_TOP = 20   # QZ_LOGPROBS_MAX_TOP


def token_logprobs_supported(logits: torch.Tensor) -> bool:
    """What qz_token_logprobs / qz_logprobs_streams take: fp16 / bf16 logits [R, V] on the GPU with unit
    element stride and a row stride of at least V, at most 65535 rows.  Metadata only."""
    return (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype in (torch.float16, torch.bfloat16)
            and logits.dim() == 2 and logits.stride(-1) == 1 and logits.stride(0) >= logits.shape[1]
            and logits.shape[0] <= 65535 and logits.shape[1] < 2 ** 31)


def _token_logprobs_composed(logits, ids, top):
    """qz_token_logprobs' rules in torch ops: fp32 log_softmax, a stable descending sort for the lists."""
    R, V = logits.shape
    dev = logits.device
    z = logits.float()
    nan = torch.full((), float("nan"), device=dev)
    bad = torch.isnan(z).any(1) | (z == float("inf")).any(1) | (z.max(1).values == float("-inf"))
    lsm = torch.where(bad[:, None], nan, torch.log_softmax(z, -1))
    inside = (ids >= 0) & (ids < V)
    lp = torch.where(inside, lsm.gather(1, ids.clamp(0, V - 1)[:, None])[:, 0], nan)
    top_id = torch.full((R, top), -1, dtype=torch.int32, device=dev)
    top_lp = torch.full((R, top), float("-inf"), dtype=torch.float32, device=dev)
    k = min(top, V)
    if k:
        order = torch.sort(z, dim=1, descending=True, stable=True).indices[:, :k]
        top_id[:, :k] = order.to(torch.int32)
        top_lp[:, :k] = lsm.gather(1, order)
    if top:
        top_id[bad] = -1
        top_lp[bad] = nan
    return lp, top_id, top_lp


def _check_logprobs_logits(name, logits, top):
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.stride(-1) != 1:
        raise ValueError(f"{name}: logits must be [R, V] with unit element stride")
    if not isinstance(top, int) or isinstance(top, bool) or not 0 <= top <= LOGPROBS_MAX_TOP:
        raise ValueError(f"{name}: top must be an integer in 0..{LOGPROBS_MAX_TOP}")


def token_logprobs(logits: torch.Tensor, ids: torch.Tensor, top: int = 0, *, composed: bool = False):
    """Log-probabilities of logits rows (qz_token_logprobs; include/quantizations.h states the rules).
    logits [R, V] (unit element stride), ids int64 [R] on the logits' device.  Returns (lp float32 [R]:
    the log-softmax of row r at ids[r], NaN for an id outside [0, V); top_id int32 [R, top] and top_lp
    float32 [R, top]: the `top` <= LOGPROBS_MAX_TOP most likely tokens of each row, value descending then
    index ascending, padded with -1 / -inf when V < top).  A row holding a NaN or +inf, or nothing but
    -inf, is NaN / -1 throughout.  fp32 or CPU logits (token_logprobs_supported is false), or
    composed=True, take the same rules in torch ops (fp32 log_softmax, a stable sort)."""
    _check_logprobs_logits("token_logprobs", logits, top)
    R, V = logits.shape
    if (not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.device != logits.device
            or ids.shape != (R,) or not ids.is_contiguous()):
        raise ValueError("token_logprobs: ids must be contiguous int64 [R] on the logits' device")
    dev = logits.device
    if not (R and V):
        return (torch.full((R,), float("nan"), dtype=torch.float32, device=dev),
                torch.full((R, top), -1, dtype=torch.int32, device=dev),
                torch.full((R, top), float("-inf"), dtype=torch.float32, device=dev))
    if composed or not token_logprobs_supported(logits):
        return _token_logprobs_composed(logits, ids, top)
    lp = torch.empty(R, dtype=torch.float32, device=dev)
    top_id = torch.empty((R, top), dtype=torch.int32, device=dev)
    top_lp = torch.empty((R, top), dtype=torch.float32, device=dev)
    work = torch.empty(_lib.lib.qz_logprobs_work_bytes(R, V, top), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib.qz_token_logprobs(
        logits.data_ptr(), _lib.dtype_code(logits.dtype), R, V, logits.stride(0), ids.data_ptr(), top, lp.data_ptr(),
        top_id.data_ptr() if top else 0, top_lp.data_ptr() if top else 0, work.data_ptr(), _lib.stream_of(logits)),
        "qz_token_logprobs")
    return lp, top_id, top_lp


def logprobs_streams(logits: torch.Tensor, seq: torch.Tensor, pos0: torch.Tensor, pos1: torch.Tensor,
                     lp_tab: torch.Tensor, top_id_tab: Optional[torch.Tensor] = None,
                     top_lp_tab: Optional[torch.Tensor] = None, T: int = 1, *, composed: bool = False) -> None:
    """The log-probabilities of the tokens a step emitted, written into a session's tables
    (qz_logprobs_streams).  logits [B*T, V]; seq int64 [B, L] (unit element stride) is the sequence
    itself; pos0 / pos1 int64 [1] (one position for all) or [B]: the streams' positions before and after
    the pick.  Row (b, i) describes column c = pos0[b] + 1 + i and is live iff 0 <= c <= pos1[b] and
    c < L: then lp_tab[b, c] (float32 [B, >= L]) is the log-probability of seq[b, c] under the row, and
    top_id_tab[b, c, :] (int32) / top_lp_tab[b, c, :] (float32), [B, as lp_tab, n] with n <=
    LOGPROBS_MAX_TOP, its n most likely tokens (both None: no lists).  Any other row writes nothing.
    Every address is computed on the device, so a captured call follows the streams.  fp32 or CPU
    logits, or composed=True, take the same rules in torch ops (not capturable)."""
    n = 0 if top_id_tab is None else int(top_id_tab.shape[-1])
    _check_logprobs_logits("logprobs_streams", logits, n)
    dev = logits.device
    if (not isinstance(seq, torch.Tensor) or seq.dtype != torch.int64 or seq.device != dev or seq.dim() != 2
            or (seq.shape[1] > 1 and seq.stride(1) != 1) or seq.stride(0) < seq.shape[1]):
        raise ValueError("logprobs_streams: seq must be int64 [B, L] with unit element stride on the logits' device")
    B, L = seq.shape
    if not 1 <= T <= VERIFY_MAX_T:
        raise ValueError(f"logprobs_streams: T must be in 1..{VERIFY_MAX_T}")
    R, V = logits.shape
    if R != B * T:
        raise ValueError("logprobs_streams: logits must be [B*T, V]")
    for t, what in ((pos0, "pos0"), (pos1, "pos1")):
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.device != dev or not t.is_contiguous()
                or t.numel() not in (1, B)):
            raise ValueError(f"logprobs_streams: {what} must be contiguous int64 [1] or [B] on the logits' device")
    if (not isinstance(lp_tab, torch.Tensor) or lp_tab.dtype != torch.float32 or lp_tab.device != dev
            or lp_tab.dim() != 2 or lp_tab.shape[0] != B or lp_tab.shape[1] < L or not lp_tab.is_contiguous()):
        raise ValueError("logprobs_streams: lp_tab must be contiguous float32 [B, >= L] on the logits' device")
    if (top_id_tab is None) != (top_lp_tab is None):
        raise ValueError("logprobs_streams: top_id_tab and top_lp_tab go together")
    for t, dt, what in ((top_id_tab, torch.int32, "top_id_tab"), (top_lp_tab, torch.float32, "top_lp_tab")):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != dev
                              or t.shape != (B, lp_tab.shape[1], n) or not t.is_contiguous()):
            raise ValueError(f"logprobs_streams: {what} must be contiguous {dt} [B, {lp_tab.shape[1]}, n]")
    if not (B and V and L):
        return
    if composed or not token_logprobs_supported(logits):
        b = torch.arange(B, device=dev).repeat_interleave(T)
        i = torch.arange(T, device=dev).repeat(B)
        p0 = (pos0.expand(B) if pos0.numel() == 1 else pos0)[b]
        p1 = (pos1.expand(B) if pos1.numel() == 1 else pos1)[b]
        c = p0 + 1 + i
        live = (c >= 0) & (c <= p1) & (c < L)
        cc = c.clamp(0, L - 1)
        lp, ti, tl = _token_logprobs_composed(logits, seq[b, cc], n)
        lp_tab[b[live], cc[live]] = lp[live]
        if n:
            top_id_tab[b[live], cc[live]] = ti[live]
            top_lp_tab[b[live], cc[live]] = tl[live]
        return
    work = torch.empty(_lib.lib.qz_logprobs_work_bytes(R, V, n), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib.qz_logprobs_streams(
        logits.data_ptr(), _lib.dtype_code(logits.dtype), B, T, V, logits.stride(0), seq.data_ptr(), seq.stride(0), L,
        pos0.data_ptr(), 0 if pos0.numel() == 1 and B > 1 else 1, pos1.data_ptr(),
        0 if pos1.numel() == 1 and B > 1 else 1, n, lp_tab.data_ptr(), _lib.ptr(top_id_tab) if n else 0,
        _lib.ptr(top_lp_tab) if n else 0, lp_tab.shape[1], work.data_ptr(), _lib.stream_of(logits)),
        "qz_logprobs_streams")


def constrain_logits_supported(logits: torch.Tensor) -> bool:
    """What qz_constrain_logits takes: fp16 / bf16 logits [R, V] on the GPU with unit element stride and
    a row stride of at least V, at most 65535 rows.  Metadata only."""
    return process_logits_supported(logits)


def _check_tables(name, tables, dev):
    if (not isinstance(tables, (tuple, list)) or len(tables) != 3
            or not all(isinstance(t, torch.Tensor) and t.device == dev and t.is_contiguous() for t in tables)):
        raise ValueError(f"{name}: automaton must be TokenAutomaton.to(device)'s (class_of, next, allow) on the "
                         "operands' device")
    class_of, nxt, allow = tables
    if (class_of.dtype != torch.int16 or class_of.dim() != 1 or nxt.dtype != torch.int32 or nxt.dim() != 2
            or allow.dtype != torch.int32 or allow.shape != (nxt.shape[0], (nxt.shape[1] + 31) // 32)
            or nxt.shape[0] < 1 or not 1 <= nxt.shape[1] <= 32767):
        raise ValueError(f"{name}: class_of int16 [V], next int32 [S, C <= 32767], allow int32 [S, ceil(C/32)]")
    return class_of, nxt, allow


def _constrain_logits_composed(logits, B, T, state, tok, tables, mask, bias_ids, bias_vals, bias_n) -> None:
    """qz_constrain_logits' rules with the bookkeeping on the host (one read of the states, the drafts,
    the tables and the lists) and the arithmetic in torch ops on the logits' device."""
    V = logits.shape[1]
    dev = logits.device
    ninf = float("-inf")
    idx = torch.arange(V, device=dev)
    if tables is not None:
        class_of, nxt = tables[0].cpu().long(), tables[1].cpu()
        S, C = nxt.shape
        states = state.cpu().tolist()
        drafts = tok.cpu().reshape(B, T).tolist() if tok is not None else None
    if bias_ids is not None:
        counts = bias_n.cpu().tolist()
    for b in range(B):
        s = -1
        if tables is not None:
            s = states[b] if 0 <= states[b] < S else -1
        for i in range(T):
            row = logits[b * T + i]
            if i and s >= 0:
                d = drafts[b][i]
                s = int(nxt[s, class_of[d]]) if 0 <= d < V else -1
                s = s if 0 <= s < S else -1
            if bias_ids is not None:
                n = min(max(counts[b], 0), bias_ids.shape[1])
                ids, vals = bias_ids[b, :n].long(), bias_vals[b, :n]
                keep = (ids >= 0) & (ids < V) & ~torch.isnan(vals)
                ids, vals = ids[keep], vals[keep]
                if len(set(ids.tolist())) != ids.numel():
                    raise ValueError("constrain_logits: the bias ids of a stream must be distinct")
                if bool((vals == float("inf")).any()):
                    raise ValueError("constrain_logits: a bias of +inf")
                old = row[ids]
                x = old.float()
                y = torch.where(vals == ninf, vals, x + vals).to(row.dtype)
                row[ids] = torch.where(torch.isnan(x), old, y)      # a NaN logit keeps its bits
            if s >= 0:
                row[(nxt[s][class_of] < 0).to(dev)] = ninf
            if mask is not None:
                words = mask[b, :(V + 31) // 32]
                row[((words[idx >> 5] >> (idx & 31)) & 1) == 0] = ninf


def constrain_logits(logits: torch.Tensor, *, state: Optional[torch.Tensor] = None,
                     tok: Optional[torch.Tensor] = None, automaton=None, mask: Optional[torch.Tensor] = None,
                     bias_ids: Optional[torch.Tensor] = None, bias_vals: Optional[torch.Tensor] = None,
                     bias_n: Optional[torch.Tensor] = None, T: int = 1, composed: bool = False) -> None:
    """Constrained decoding's masks and bias, in place, in front of a pick and behind process_logits
    (qz_constrain_logits; include/quantizations.h states the rules).  logits [B*T, V].  Three operands,
    each None = off:
    state int32 [B] with automaton = TokenAutomaton.to(device)'s (class_of, next, allow): row (b, i) is
    masked by the state reached from state[b] over the drafts tok[b, 1..i] (tok int64 [B, T], needed
    when T > 1); every token the state refuses becomes -inf; a row whose state is negative (-1:
    unconstrained; a refused draft in front of it) is left as it is.
    mask int32 [B, >= ceil(V/32)] (unit element stride; xgrammar's layout, set bit = allowed; T = 1).
    bias_ids int32 / bias_vals float32 [B, NB], bias_n int32 [B]: x' = round(float32(x) + bias) for the
    stream's first bias_n[b] entries on all its T rows; -inf bans; ids distinct within a row.
    The bias goes first, a mask's -inf wins.  Every value is read on the device, so a captured call
    follows in-place changes.  fp32 or CPU logits (constrain_logits_supported is false), or
    composed=True, take the same rules with the bookkeeping on the host (not capturable)."""
    name = "constrain_logits"
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.stride(-1) != 1:
        raise ValueError(f"{name}: logits must be [B*T, V] with unit element stride")
    dev = logits.device
    R, V = logits.shape
    if tok is not None:
        if not isinstance(tok, torch.Tensor) or tok.dtype != torch.int64 or tok.device != dev or not tok.is_contiguous():
            raise ValueError(f"{name}: tok must be contiguous int64 on the logits' device")
        if tok.dim() == 2:
            T = tok.shape[1]
    if not 1 <= T <= VERIFY_MAX_T:
        raise ValueError(f"{name}: T must be in 1..{VERIFY_MAX_T}")
    if R % T:
        raise ValueError(f"{name}: logits must be [B*T, V]")
    B = R // T
    if tok is not None and tok.numel() != B * T:
        raise ValueError(f"{name}: tok must be [B, T] (or [B] when T = 1)")
    if (state is None) != (automaton is None):
        raise ValueError(f"{name}: state and automaton go together")
    tables = None
    if state is not None:
        tables = _check_tables(name, automaton, dev)
        if (not isinstance(state, torch.Tensor) or state.dtype != torch.int32 or state.device != dev
                or state.shape != (B,) or not state.is_contiguous()):
            raise ValueError(f"{name}: state must be contiguous int32 [B] on the logits' device")
        if tables[0].shape[0] != V:
            raise ValueError(f"{name}: the automaton is over {tables[0].shape[0]} tokens, the logits over {V}")
        if T > 1 and tok is None:
            raise ValueError(f"{name}: a window (T > 1) needs tok")
    if mask is not None:
        if T != 1:
            raise ValueError(f"{name}: a host mask describes one row per stream; T must be 1")
        if (not isinstance(mask, torch.Tensor) or mask.dtype != torch.int32 or mask.device != dev or mask.dim() != 2
                or mask.shape[0] != B or mask.shape[1] < (V + 31) // 32 or (mask.shape[1] > 1 and mask.stride(1) != 1)
                or mask.stride(0) < mask.shape[1]):
            raise ValueError(f"{name}: mask must be int32 [B, >= ceil(V/32)] with unit element stride")
    given = [t is not None for t in (bias_ids, bias_vals, bias_n)]
    if any(given) and not all(given):
        raise ValueError(f"{name}: bias_ids, bias_vals and bias_n go together")
    if bias_ids is not None:
        ok = (isinstance(bias_ids, torch.Tensor) and bias_ids.dtype == torch.int32 and bias_ids.dim() == 2
              and bias_ids.shape[0] == B and isinstance(bias_vals, torch.Tensor) and bias_vals.dtype == torch.float32
              and bias_vals.shape == bias_ids.shape and isinstance(bias_n, torch.Tensor) and bias_n.dtype == torch.int32
              and bias_n.shape == (B,)
              and all(t.device == dev and t.is_contiguous() for t in (bias_ids, bias_vals, bias_n)))
        if not ok:
            raise ValueError(f"{name}: bias_ids int32 [B, NB], bias_vals float32 [B, NB], bias_n int32 [B], contiguous "
                             "on the logits' device")
    if not (B and V) or (state is None and mask is None and bias_ids is None):
        return
    if composed or not constrain_logits_supported(logits):
        _constrain_logits_composed(logits, B, T, state, tok if T > 1 else None, tables, mask, bias_ids, bias_vals,
                                   bias_n)
        return
    class_of, nxt, allow = tables if tables is not None else (None, None, None)
    _lib.check(_lib.lib.qz_constrain_logits(
        logits.data_ptr(), _lib.dtype_code(logits.dtype), B, T, V, logits.stride(0), _lib.ptr(state),
        _lib.ptr(tok) if T > 1 else 0, _lib.ptr(class_of), _lib.ptr(allow), _lib.ptr(nxt),
        nxt.shape[0] if nxt is not None else 0, nxt.shape[1] if nxt is not None else 0, _lib.ptr(mask),
        mask.stride(0) if mask is not None else 0, _lib.ptr(bias_ids), _lib.ptr(bias_vals), _lib.ptr(bias_n),
        bias_ids.shape[1] if bias_ids is not None else 0, _lib.stream_of(logits)), "qz_constrain_logits")


def constraint_advance_supported(state: torch.Tensor, seq: torch.Tensor) -> bool:
    """What qz_constraint_advance takes: state int32 [B] and seq int64 [B, L] (unit element stride) on
    the GPU, at most 65535 streams.  Metadata only."""
    return (isinstance(state, torch.Tensor) and isinstance(seq, torch.Tensor) and state.is_cuda and seq.is_cuda
            and state.dtype == torch.int32 and seq.dtype == torch.int64 and state.shape[0] <= 65535)


def constraint_advance(state: torch.Tensor, seq: torch.Tensor, pos0: torch.Tensor, pos1: torch.Tensor, automaton, *,
                       composed: bool = False) -> None:
    """Behind a pick: advance every stream's automaton state over the tokens the pick emitted
    (qz_constraint_advance).  state int32 [B]; seq int64 [B, L] (unit element stride) is the sequence
    itself; pos0 / pos1 int64 [1] (one position for all) or [B] are the streams' positions before and
    after the pick; automaton = TokenAutomaton.to(device)'s tensors.  For each column c = pos0[b] + 1 ..
    pos1[b]: state[b] = next[state[b], class_of[seq[b, c]]].  A stream that emitted nothing keeps its
    state, a negative state stays, a refused transition or a token outside the vocabulary writes -2.
    CPU operands, or composed=True, take the same rules on the host (not capturable)."""
    name = "constraint_advance"
    if not isinstance(state, torch.Tensor) or state.dtype != torch.int32 or state.dim() != 1 or not state.is_contiguous():
        raise ValueError(f"{name}: state must be contiguous int32 [B]")
    dev = state.device
    B = state.shape[0]
    if (not isinstance(seq, torch.Tensor) or seq.dtype != torch.int64 or seq.device != dev or seq.dim() != 2
            or seq.shape[0] != B or (seq.shape[1] > 1 and seq.stride(1) != 1) or seq.stride(0) < seq.shape[1]):
        raise ValueError(f"{name}: seq must be int64 [B, L] with unit element stride on the state's device")
    L = seq.shape[1]
    for t, what in ((pos0, "pos0"), (pos1, "pos1")):
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.device != dev or not t.is_contiguous()
                or t.numel() not in (1, B)):
            raise ValueError(f"{name}: {what} must be contiguous int64 [1] or [B] on the state's device")
    class_of, nxt, _ = _check_tables(name, automaton, dev)
    V, (S, C) = class_of.shape[0], nxt.shape
    if not (B and L):
        return
    if composed or not constraint_advance_supported(state, seq):
        st, rows = state.cpu().tolist(), seq.cpu().tolist()
        p0, p1 = pos0.cpu().reshape(-1).tolist(), pos1.cpu().reshape(-1).tolist()
        co, nx = class_of.cpu().tolist(), nxt.cpu()
        for b in range(B):
            lo, hi = max(p0[b if len(p0) > 1 else 0] + 1, 0), min(p1[b if len(p1) > 1 else 0], L - 1)
            s = st[b]
            if lo > hi or s < 0:
                continue
            s = s if s < S else -1
            for c in range(lo, hi + 1):
                t = rows[b][c]
                s = int(nx[s, co[t]]) if (s >= 0 and 0 <= t < V) else -1
                if not 0 <= s < S:
                    s = -1
                    break
            state[b] = s if s >= 0 else -2
        return
    _lib.check(_lib.lib.qz_constraint_advance(
        state.data_ptr(), B, seq.data_ptr(), seq.stride(0), L, pos0.data_ptr(), 0 if pos0.numel() == 1 and B > 1 else 1,
        pos1.data_ptr(), 0 if pos1.numel() == 1 and B > 1 else 1, class_of.data_ptr(), nxt.data_ptr(), V, S, C,
        _lib.stream_of(state)), "qz_constraint_advance")


def ngram_draft_reference(seq, tok0: int, p: int, T: int, ngram_max: int) -> list:
    """The drafter's rule on host integers: seq[0..p] is the stream's history (seq[p] the newest
    token), the result its T - 1 drafts."""
    if 0 <= p < len(seq):
        for n in range(min(ngram_max, p), 0, -1):
            tail = list(seq[p - n + 1:p + 1])
            for m in range(p - n, -1, -1):
                if list(seq[m:m + n]) == tail:
                    e = list(seq[:p + 1])
                    for i in range(T - 1):
                        e.append(e[m + n + i])
                    return e[p + 1:]
    return [tok0] * (T - 1)


def ngram_draft(hist: torch.Tensor, pos: torch.Tensor, tok: torch.Tensor, pos_ids: torch.Tensor,
                ngram_max: int = 3, *, composed: bool = False) -> None:
    """The prompt-lookup drafter (qz_ngram_draft), one workgroup per stream: hist int64 [B, H] is the
    sequence itself (hist[b, pos[b]] is tok[b, 0], the newest token), tok int64 [B, T], pos_ids int64
    [B, T].  For n = ngram_max .. 1 with n <= pos[b]: the latest earlier copy of the last n tokens
    (largest start m with m + n <= pos[b]); the first n that has one wins and the drafts
    tok[b, 1:] are what followed it, running on into the drafts themselves where the copy ends at the
    newest token.  No match: every draft is tok[b, 0].  Also pos_ids[b, i] = pos[b] + i.  Drafts are
    hints: no result may depend on them.  CPU tensors, or composed=True, run ngram_draft_reference on
    the host."""
    for t, what in ((hist, "hist"), (pos, "pos"), (tok, "tok"), (pos_ids, "pos_ids")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.device != hist.device or not t.is_contiguous():
            raise ValueError(f"ngram_draft: {what} must be contiguous int64 on one device")
    if tok.dim() != 2 or not 1 <= tok.shape[1] <= VERIFY_MAX_T or pos_ids.shape != tok.shape:
        raise ValueError(f"ngram_draft: tok and pos_ids must be [B, T] with T <= {VERIFY_MAX_T}")
    B, T = tok.shape
    if hist.dim() != 2 or hist.shape[0] != B or pos.shape != (B,):
        raise ValueError("ngram_draft: hist [B, H], pos [B]")
    if not 1 <= int(ngram_max) <= NGRAM_MAX:
        raise ValueError(f"ngram_draft: ngram_max must be in 1..{NGRAM_MAX}")
    if composed or not hist.is_cuda:
        h, ps, tk = hist.cpu().tolist(), pos.cpu().tolist(), tok.cpu()
        for b in range(B):
            tk[b, 1:] = torch.tensor(ngram_draft_reference(h[b], int(tk[b, 0]), ps[b], T, int(ngram_max)),
                                     dtype=torch.int64)
        tok.copy_(tk)
        pos_ids.copy_(pos[:, None] + torch.arange(T, device=pos.device)[None, :])
        return
    _lib.check(_lib.lib.qz_ngram_draft(B, T, int(ngram_max), hist.data_ptr(), hist.shape[1], hist.shape[1],
                                       pos.data_ptr(), tok.data_ptr(), pos_ids.data_ptr(), _lib.stream_of(hist)),
               "qz_ngram_draft")
