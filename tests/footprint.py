"""Memory-footprint harness: guard bands, row tails and sentinels around the operands of a kernel.

`guarded(t, ...)` places `t`'s values inside one larger allocation, with a leading guard, a
trailing guard and (with `row_stride`) a guard tail after every row, and returns the view a kernel
is handed.  Everything a kernel may touch by mistake -- an over-fetch of a whole unclamped tile, a
ragged vector store -- therefore stays inside a live allocation: a dependence on foreign bytes or a
spill shows up BY VALUE (`assert_untouched`, or a payload that is no longer the contiguous call's
bits), never as a fault.

Guard-size rule: the leading and the trailing guard of an operand are each at least 256 of that
operand's row strides or 64 KiB, whichever is larger, rounded up to a multiple of 256 B (so the
payload keeps exactly the alignment the test asked for through `offset_elems`).

Fills:
  "poison"    inputs: floats are NaN with payload 0x5EA, uint8 is 0xFF, other integers must name an
              out-of-range value (`fill=<int>`);
  "sentinel"  outputs and scratch: floats are NaN with payload 0xA5.., everything else 0xA5 bytes,
              so "written with the right value" and "not written" cannot coincide;
  a number    that value in every guard element (an out-of-range slot id, +inf logits padding).

Plain torch; importing this module needs no GPU.
"""
from __future__ import annotations

import math

import torch

GUARD_ROWS = 256          # guards hold at least this many row strides ...
GUARD_MIN_BYTES = 65536   # ... and at least this many bytes
GUARD_ALIGN = 256

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}

# NaN bit patterns by element size (quiet NaNs, distinct payloads for inputs and outputs)
_POISON_NAN = {torch.float16: 0x7E5A, torch.bfloat16: 0x7FDA, torch.float32: 0x7FC005EA,
               torch.float64: 0x7FF80000000005EA}
_SENTINEL_NAN = {torch.float16: 0x7EA5, torch.bfloat16: 0x7FE5, torch.float32: 0x7FE5A5A5,
                 torch.float64: 0x7FFDA5A5A5A5A5A5}
_SENTINEL_INT = {1: 0xA5, 2: 0xA5A5, 4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}


def _signed(pattern: int, nbytes: int) -> int:
    bits = 8 * nbytes
    return pattern - (1 << bits) if nbytes > 1 and pattern >= 1 << (bits - 1) else pattern


def _bits(t: torch.Tensor) -> torch.Tensor:
    """t's elements as integers of the same width (no copy, any strides)."""
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    return t.view(_INT_VIEW[t.element_size()])


bits = _bits


def fill_pattern(dtype: torch.dtype, fill) -> int:
    """The integer bit pattern (signed, element width) of one guard element."""
    esize = torch.empty(0, dtype=dtype).element_size()
    if fill == "poison":
        if dtype.is_floating_point:
            return _signed(_POISON_NAN[dtype], esize)
        if dtype in (torch.uint8, torch.bool):
            return 0xFF
        raise ValueError(f"poisoned {dtype} guards need an explicit out-of-range value (fill=<int>)")
    if fill == "sentinel":
        return _signed(_SENTINEL_NAN[dtype] if dtype.is_floating_point else _SENTINEL_INT[esize], esize)
    if isinstance(fill, (int, float)):
        return int(_bits(torch.tensor([fill], dtype=dtype))[0])
    raise ValueError(f"unknown fill {fill!r}")


def filled(shape, dtype: torch.dtype, fill, device="cpu") -> torch.Tensor:
    """A tensor whose every element carries fill's bit pattern: the payload of an output or scratch buffer
    before the call ("sentinel"), or a dirty workspace ("poison": NaN / 0xFF)."""
    esize = torch.empty(0, dtype=dtype).element_size()
    idt = torch.uint8 if dtype == torch.bool else _INT_VIEW[esize]
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return torch.full(shape, fill_pattern(dtype, fill), dtype=idt, device=device).view(dtype)


class _Footprint:
    """Where a guarded view's payload lies inside its allocation (element units)."""

    def __init__(self, base, start, rows, cols, row_stride, mask, name):
        self.base = base              # the whole allocation, as integers of the element width
        self.start = start            # first payload element
        self.rows, self.cols, self.row_stride = rows, cols, row_stride
        self.mask = mask              # True on payload elements
        self.snapshot = None          # guard (and payload) bits when the view was handed out
        self.name = name

    def where(self, idx: int) -> str:
        rel = idx - self.start
        last = (self.rows - 1) * self.row_stride + self.cols
        if rel < 0:
            return f"{rel} elements before the payload"
        if rel >= last:
            return f"+{rel - last} elements past the end (row {self.rows - 1})"
        r, c = divmod(rel, self.row_stride)
        if c < self.cols:
            return f"payload element {c} of row {r}"
        return f"+{c - self.cols} elements past row {r}"


def guard_bytes(row_stride_elems: int, esize: int) -> int:
    need = max(GUARD_ROWS * row_stride_elems * esize, GUARD_MIN_BYTES)
    return (need + GUARD_ALIGN - 1) // GUARD_ALIGN * GUARD_ALIGN


def guarded(t: torch.Tensor, *, row_stride: int | None = None, offset_elems: int = 0, fill="poison",
            name: str = "") -> torch.Tensor:
    """A view holding t's values (t's shape; the last dimension contiguous, every leading index
    `row_stride` elements apart, default: packed) between guard bands.  offset_elems shifts the
    payload's first element off the 256-B boundary it would otherwise start at."""
    assert offset_elems >= 0
    shape = tuple(t.shape) if t.dim() else (1,)
    cols = shape[-1]
    rows = math.prod(shape[:-1])
    rs = cols if row_stride is None else int(row_stride)
    assert rs >= cols, "row_stride must cover the row"
    assert cols > 0 and rows > 0
    dtype = t.dtype
    esize = t.element_size()
    g = guard_bytes(rs, esize)
    span = (rows - 1) * rs + cols
    lead = g // esize + offset_elems
    total = lead + span + g // esize
    total = (total * esize + GUARD_ALIGN - 1) // GUARD_ALIGN * GUARD_ALIGN // esize
    raw = torch.empty(total * esize, dtype=torch.uint8, device=t.device)
    base = raw.view(torch.uint8 if dtype == torch.bool else _INT_VIEW[esize])
    base.fill_(fill_pattern(dtype, fill))
    typed = raw.view(dtype) if dtype != torch.bool else raw.view(torch.bool)
    lead_strides = []
    acc = rs
    for d in reversed(shape[:-1]):
        lead_strides.append(acc)
        acc *= d
    strides = tuple(reversed(lead_strides)) + (1,)
    view = torch.as_strided(typed, shape, strides, lead)
    _bits(view).copy_(_bits(t.reshape(shape)))     # by bits: NaN payloads and -0 survive
    mask = torch.zeros(total, dtype=torch.bool, device=t.device)
    torch.as_strided(mask, (rows, cols), (rs, 1), lead).fill_(True)
    fp = _Footprint(base, lead, rows, cols, rs, mask, name)
    fp.snapshot = base.clone()
    view._footprint = fp
    return view


def _report(fp: _Footprint, bad: torch.Tensor, what: str) -> str:
    idx = torch.nonzero(bad.reshape(-1))[:8].reshape(-1).tolist()
    places = "; ".join(fp.where(i) for i in idx)
    n = int(bad.sum())
    label = f" of {fp.name}" if fp.name else ""
    return f"{what}{label}: {n} element(s) changed, first at: {places}"


def assert_untouched(view: torch.Tensor, name: str = "") -> None:
    """Every guard element (leading, trailing, row tails) still holds what guarded() put there."""
    fp = view._footprint
    if name:
        fp.name = name
    bad = (fp.base != fp.snapshot) & ~fp.mask
    if bool(bad.any()):
        raise AssertionError(_report(fp, bad, "guard overwritten"))


def assert_unchanged(view: torch.Tensor, name: str = "") -> None:
    """The whole allocation, payload included, is bit-identical to when it was handed out (inputs)."""
    fp = view._footprint
    if name:
        fp.name = name
    bad = fp.base != fp.snapshot
    if bool(bad.any()):
        raise AssertionError(_report(fp, bad, "input modified"))


def changed_payload(view: torch.Tensor) -> torch.Tensor:
    """Boolean tensor of view's shape: which payload elements differ from the hand-out bits."""
    fp = view._footprint
    diff = fp.base != fp.snapshot
    return torch.as_strided(diff, tuple(view.shape), tuple(view.stride()), fp.start)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Integer-view equality: NaN payloads and signed zeros count."""
    if a.dtype != b.dtype or tuple(a.shape) != tuple(b.shape):
        return False
    return bool(torch.equal(_bits(a), _bits(b)))


def assert_same_bits(a: torch.Tensor, b: torch.Tensor, name: str = "payload") -> None:
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (name, a.dtype, b.dtype, a.shape, b.shape)
    bad = _bits(a) != _bits(b)
    if bool(bad.any()):
        idx = torch.nonzero(bad)[:4].tolist()
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ in bits, first at {idx}: "
                             f"{[a[tuple(i)].item() for i in idx]} vs {[b[tuple(i)].item() for i in idx]}")


def is_aligned(t: torch.Tensor, nbytes: int = 16) -> bool:
    return t.data_ptr() % nbytes == 0
