"""LoRA adapters on ``Linear4bit`` (QLoRA results: a frozen 4-bit base plus low-rank adapters,
which cannot be merged into the 4-bit codes without re-quantising the weight).

A layer with an adapter ``A [r, K]``, ``B [M, r]``, ``scaling`` computes
``base(x) + lora_B(lora_A(x)) * scaling`` (peft's form).  For one decode token of 16-bit
activations on the GPU that is two launches: ``shrink`` (``t = scaling * A x'``, fp32, for every
adapter that reads the same x, qz_lora_shrink) and the layer's usual fused GEMV launch carrying
the adapter operand (``B . t`` added to its fp32 row sums, qz_gemv_4bit_lora /
qz_gemv_4bit_grouped_lora).  Every other input takes ``composed_term`` -- the torch ops.

``AdapterBank``: several adapters on one resident 4-bit layer, each stream of a small batch on its
own adapter or on none (``slots``, a device int32 tensor the caller owns and usually shares
between every layer of the model: stream b uses entry ``slots[b]``, any value outside
``[0, n)`` means no adapter).  2..16 rows of 16-bit activations run as ``shrink_mt``
(qz_lora_shrink_mt, one launch for every bank that reads the same x) plus the usual multi-token
launch carrying the expand in its epilogue (qz_gemm_4bit_grouped_lora); everything else -- one
token, more than 16 rows, fp32 x, K % 256 != 0, the CPU -- takes ``composed_bank_term``, torch ops
that read ``slots`` on the device only (no host read, so it can be captured in a graph).  The
single-token GEMV kernels and the gate/up pair launch do not know banks.
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


class AdapterBank:
    """n adapters of one layer, stacked: A [n, r, K], B [n, M, r] and scaling fp32 [n] on the
    layer's device, adapters of a smaller rank zero-padded to the bank's rank r (exact: the padded
    rank rows contribute 0), ``None`` entries all zero.  ``slots`` (int32, same device, or None =
    every row on entry 0) is only referenced: the caller owns it and writes the adapter index of
    each stream into it; the kernels read it at run time, so a captured graph serves whatever it
    holds at replay, and whatever ``put`` wrote into the bank."""

    __slots__ = ("A", "B", "scaling", "slots")

    def __init__(self, adapters, slots, out_features: int, in_features: int, device):
        adapters = list(adapters)
        live = [a for a in adapters if a is not None]
        if not adapters or not live:
            raise ValueError("adapter bank: at least one (A, B, scaling) entry is needed")
        if len(adapters) > _lib.LORA_MAX_ADAPTERS:
            raise ValueError(f"adapter bank: at most {_lib.LORA_MAX_ADAPTERS} entries, got {len(adapters)}")
        dtype = live[0][0].dtype
        for A, B, _ in live:
            check_shapes(A, B, out_features, in_features)
            if A.dtype != dtype:
                raise ValueError(f"adapter bank: every entry must have the dtype {dtype}, got {A.dtype}")
        r = max(A.shape[0] for A, _, _ in live)
        n = len(adapters)
        self.A = torch.zeros(n, r, in_features, dtype=dtype, device=device)
        self.B = torch.zeros(n, out_features, r, dtype=dtype, device=device)
        self.scaling = torch.zeros(n, dtype=torch.float32, device=device)
        self.slots = None
        self.set_slots(slots)
        for i, ent in enumerate(adapters):
            if ent is not None:
                self.put(i, *ent)

    @property
    def n(self) -> int:
        return self.A.shape[0]

    @property
    def r(self) -> int:
        return self.A.shape[1]

    def set_slots(self, slots) -> None:
        if slots is not None and (slots.dtype != torch.int32 or slots.dim() != 1 or slots.device != self.A.device
                                  or not slots.is_contiguous()):
            raise ValueError(f"adapter bank: slots must be a contiguous 1-D int32 tensor on {self.A.device}")
        self.slots = slots

    def put(self, i: int, A=None, B=None, scaling: float = 1.0) -> None:
        """Overwrite entry i in place (A = B = None: an all-zero entry).  A rank up to the bank's is
        accepted and zero-padded; a larger one raises ValueError."""
        if not 0 <= i < self.n:
            raise IndexError(f"adapter bank: entry {i} of {self.n}")
        if A is None or B is None:
            self.A[i].zero_()
            self.B[i].zero_()
            self.scaling[i] = 0.0
            return
        check_shapes(A, B, self.B.shape[1], self.A.shape[2])
        ra = A.shape[0]
        if ra > self.r:
            raise ValueError(f"adapter bank: rank {ra} exceeds the bank's rank {self.r}")
        if A.dtype != self.A.dtype:
            raise ValueError(f"adapter bank: entries have the dtype {self.A.dtype}, got {A.dtype}")
        self.A[i, :ra].copy_(A.detach())
        self.A[i, ra:].zero_()
        self.B[i, :, :ra].copy_(B.detach())
        self.B[i, :, ra:].zero_()
        self.scaling[i] = float(scaling)

    def to(self, device) -> None:
        """Follow the layer to `device`.  A slots tensor left on another device is copied (the copy
        is then this bank's own: hand the moved model a new shared one with set_slots)."""
        self.A, self.B, self.scaling = self.A.to(device), self.B.to(device), self.scaling.to(device)
        if self.slots is not None:
            self.slots = self.slots.to(device)


def bank_rows(bank: AdapterBank, x: torch.Tensor):
    """(T, S) of x for a bank: T rows, S consecutive rows per stream (x.shape[-2] for x of 3 or more
    dimensions -- [B, 1, K] decode and [B, S, K] prefill -- else 1).  More streams than slots holds
    raises ValueError (a shape check, no device read)."""
    K = x.shape[-1]
    T = x.numel() // K if K else 0
    S = max(int(x.shape[-2]), 1) if x.dim() >= 3 else 1
    streams = (T + S - 1) // S
    if bank.slots is not None and streams > bank.slots.numel():
        raise ValueError(f"adapter bank: {streams} streams but slots holds {bank.slots.numel()} entries")
    return T, S


def bank_fused_ok(bank: AdapterBank, x: torch.Tensor) -> bool:
    """The shrink_mt + multi-token launch route takes this bank for x (the caller also checks
    core.grouped_tokens_ok for the weights): 16-bit x on the GPU, the bank in x's dtype."""
    return (not FORCE_COMPOSED and x.is_cuda and x.dtype in (torch.float16, torch.bfloat16)
            and bank.A.dtype == x.dtype and bank.A.device == x.device and bank.r <= _lib.LORA_MAX_RANK
            and x.shape[-1] == bank.A.shape[2] and x.shape[-1] % 8 == 0
            and bank.A.data_ptr() % 16 == 0 and bank.B.data_ptr() % 16 == 0)


def composed_bank_term(bank: AdapterBank, x: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """The bank's term for every row of x with torch ops, in the wider of x's and the bank's dtype:
    t = x A^T for all n adapters at once ([T, n r]), each block of r columns masked by slot == i and
    scaled, then t B^T with B as [M, n r].  slots is compared on the device (no host read: the route
    can be captured); the only temporaries are [T, n r] and the [M, n r] view of B."""
    T, S = bank_rows(bank, x)
    n, r, K = bank.A.shape
    M = bank.B.shape[1]
    dt = torch.promote_types(x.dtype, bank.A.dtype)
    t = F.linear(x.reshape(T, K).to(dt), bank.A.reshape(n * r, K).to(dt)).float().view(T, n, r)
    if bank.slots is None:
        row_slot = torch.zeros(T, dtype=torch.int32, device=x.device)
    else:
        streams = (T + S - 1) // S
        row_slot = bank.slots[:streams].view(streams, 1).expand(streams, S).reshape(-1)[:T]
    sel = row_slot.view(T, 1) == torch.arange(n, dtype=torch.int32, device=x.device).view(1, n)
    t = t * (sel.to(torch.float32) * bank.scaling.view(1, n)).unsqueeze(-1)
    out = F.linear(t.view(T, n * r).to(dt), bank.B.permute(1, 0, 2).reshape(M, n * r).to(dt))
    return out.reshape(*x.shape[:-1], M).to(out_dtype)


def shrink_mt(x: torch.Tensor, banks: Sequence[Optional[AdapterBank]]):
    """t[c, off_i + j] = scaling_i[a] * A_i[a, j] . x_c (a = the row's slot) for the banks (None
    entries skipped; they share one slots tensor) that read the 2..16 rows of x, in one launch.
    Rows without an adapter get zeros.  Returns (t fp32 [T, sum r], [t_offset_i or None])."""
    live = [b for b in banks if b is not None]
    if not 1 <= len(live) <= _lib.GEMV_MAX_SEGMENTS:
        raise ValueError(f"shrink_mt takes 1..{_lib.GEMV_MAX_SEGMENTS} banks, got {len(live)}")
    if any(b.slots is not live[0].slots for b in live):
        raise ValueError("shrink_mt: the banks must share one slots tensor")
    K = x.shape[-1]
    T, S = bank_rows(live[0], x)
    x2 = x.reshape(T, K)
    if x2.stride(-1) != 1 or x2.stride(0) % 8 != 0 or x2.data_ptr() % 16 != 0:
        x2 = x2.contiguous()
    segs = (_lib.LoraBankShrinkSegment * len(live))()
    offs, total, i = [], 0, 0
    for b in banks:
        if b is None:
            offs.append(None)
            continue
        if b.A.dtype != x.dtype or b.A.shape[2] != K or not b.A.is_contiguous():
            raise ValueError(f"shrink_mt: bank A must be a contiguous [n, r, {K}] {x.dtype} tensor")
        segs[i] = _lib.LoraBankShrinkSegment(ptr(b.A), ptr(b.scaling), b.n, b.r, total)
        offs.append(total)
        total += b.r
        i += 1
    t = torch.empty((T, total), dtype=torch.float32, device=x.device)
    check(lib.qz_lora_shrink_mt(len(live), ctypes.cast(segs, ctypes.c_void_p), T, K, ptr(x2), x2.stride(0),
                                dtype_code(x.dtype), ptr(live[0].slots), S, ptr(t), total, _lib.stream_of(x)),
          "lora.shrink_mt")
    return t, offs
