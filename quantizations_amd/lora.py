"""LoRA adapters on ``Linear4bit`` (QLoRA results: a frozen 4-bit base plus low-rank adapters,
which cannot be merged into the 4-bit codes without re-quantising the weight).

A layer with an adapter ``A [r, K]``, ``B [M, r]``, ``scaling`` computes
``base(x) + lora_B(lora_A(x)) * scaling`` (peft's form).  For one decode token of 16-bit
activations on the GPU that is two launches: ``shrink`` (``t = scaling * A x'``, fp32, for every
adapter that reads the same x, qz_lora_shrink) and the layer's usual fused GEMV launch carrying
the adapter operand (``B . t`` added to its fp32 row sums, qz_gemv_4bit_lora /
qz_gemv_4bit_grouped_lora).  Every other input takes ``composed_term`` -- the torch ops.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import check, dtype_code, lib, ptr

# measurement switch (scripts/lora_times.py): True sends every input down the composed torch path
FORCE_COMPOSED = False


class LoraAdapter:
    """One layer's adapter: A [r, K] and B [M, r] contiguous on the layer's device, scaling as a
    one-element fp32 tensor there (the shrink launch reads it from device memory, so a captured
    graph serves whatever value and weights the buffers hold at replay)."""

    __slots__ = ("A", "B", "scaling")

    def __init__(self, A: torch.Tensor, B: torch.Tensor, scaling, device):
        self.A = A.detach().to(device).contiguous().clone()
        self.B = B.detach().to(device).contiguous().clone()
        self.scaling = torch.tensor([float(scaling)], dtype=torch.float32, device=device)

    @property
    def r(self) -> int:
        return self.A.shape[0]

    def matches(self, A: torch.Tensor, B: torch.Tensor) -> bool:
        return A.shape == self.A.shape and B.shape == self.B.shape and A.dtype == self.A.dtype and \
            B.dtype == self.B.dtype

    def copy_(self, A: torch.Tensor, B: torch.Tensor, scaling) -> None:
        self.A.copy_(A.detach())
        self.B.copy_(B.detach())
        self.scaling.fill_(float(scaling))

    def to(self, device) -> None:
        self.A, self.B, self.scaling = self.A.to(device), self.B.to(device), self.scaling.to(device)


def check_shapes(A: torch.Tensor, B: torch.Tensor, out_features: int, in_features: int) -> None:
    if A.dim() != 2 or B.dim() != 2 or A.shape[0] != B.shape[1] or A.shape[0] < 1:
        raise ValueError(f"adapter: A must be [r, K] and B [M, r], got {tuple(A.shape)} and {tuple(B.shape)}")
    if A.shape[1] != in_features or B.shape[0] != out_features:
        raise ValueError(f"adapter: A [r, {in_features}] and B [{out_features}, r] expected, got "
                         f"{tuple(A.shape)} and {tuple(B.shape)}")
    if A.dtype != B.dtype or not A.dtype.is_floating_point:
        raise ValueError(f"adapter: A and B must share a floating dtype, got {A.dtype} and {B.dtype}")


def fused_ok(ad: LoraAdapter, x: torch.Tensor) -> bool:
    """The shrink + fused-launch route takes this adapter for x: one 16-bit token on the GPU,
    adapter tensors of x's dtype, rank <= 64, 16-B chunks of K."""
    return (not FORCE_COMPOSED and x.is_cuda and x.numel() == x.shape[-1]
            and x.dtype in (torch.float16, torch.bfloat16) and ad.A.dtype == x.dtype and ad.A.device == x.device
            and ad.r <= _lib.LORA_MAX_RANK and x.shape[-1] % 8 == 0 and x.shape[-1] == ad.A.shape[1]
            and ad.A.data_ptr() % 16 == 0)


def composed_term(ad: LoraAdapter, x: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """lora_B(lora_A(x)) * scaling with torch ops, in the wider of x's and the adapter's dtype."""
    dt = torch.promote_types(x.dtype, ad.A.dtype)
    a, b = ad.A.to(dt), ad.B.to(dt)
    return (F.linear(F.linear(x.to(dt), a), b) * ad.scaling.to(x.device)).to(out_dtype)


def shrink(x: torch.Tensor, adapters: Sequence[Optional[LoraAdapter]], norm=None):
    """t = scaling_i * A_i x' for the adapters (None entries skipped) that read the single token x,
    in one launch.  norm=(weight, eps): x' = layer_ops.rms_norm(x, weight, eps), formed in the
    launch's prologue with that kernel's arithmetic; else x' = x.  Returns (t fp32 [sum r],
    [t_offset_i or None])."""
    live = [a for a in adapters if a is not None]
    if not 1 <= len(live) <= _lib.GEMV_MAX_SEGMENTS:
        raise ValueError(f"shrink takes 1..{_lib.GEMV_MAX_SEGMENTS} adapters, got {len(live)}")
    K = x.shape[-1]
    if x.numel() != K:
        raise ValueError("shrink needs a single input vector")
    x = x.contiguous()
    segs = (_lib.LoraShrinkSegment * len(live))()
    offs, total, i = [], 0, 0
    for a in adapters:
        if a is None:
            offs.append(None)
            continue
        if a.A.dtype != x.dtype or a.A.shape[1] != K or not a.A.is_contiguous():
            raise ValueError(f"shrink: adapter A must be a contiguous [r, {K}] {x.dtype} tensor")
        segs[i] = _lib.LoraShrinkSegment(ptr(a.A), ptr(a.scaling), a.r, total)
        offs.append(total)
        total += a.r
        i += 1
    t = torch.empty(total, dtype=torch.float32, device=x.device)
    nw, eps = (None, 0.0) if norm is None else norm
    if nw is not None and not (nw.dtype == x.dtype and nw.is_contiguous() and nw.numel() == K):
        raise ValueError(f"shrink: the norm weight must be a contiguous {x.dtype} tensor of {K} elements")
    check(lib.qz_lora_shrink(len(live), ctypes.cast(segs, ctypes.c_void_p), K, ptr(x), dtype_code(x.dtype), ptr(nw),
                             float(eps), ptr(t), _lib.stream_of(x)), "lora.shrink")
    return t, offs
