"""The footprint harness (tests/footprint.py) would notice: deliberately wrong "kernels" written in
torch on CPU tensors are each rejected, with a message that names the place, and their correct
versions pass.  No GPU."""
import pytest
import torch

from footprint import (GUARD_MIN_BYTES, assert_same_bits, assert_unchanged, assert_untouched, changed_payload,
                       fill_pattern, filled, guard_bytes, guarded, is_aligned, same_bits)


def _flat(view, n):
    """n elements from view's first one on, as a kernel's raw pointer sees them (may pass the view's end)."""
    return torch.as_strided(view, (n,), (1,), view.storage_offset())


def _nan_scratch(n, dtype=torch.float32):
    return guarded(torch.full((n,), float("nan"), dtype=dtype), fill="sentinel")


# ---- fake kernels -------------------------------------------------------------------------------

ROWS_PER_BLOCK = 8
VEC = 8        # 16 B of fp16


def gemv(W, x, y, M, K, ldw, *, clamp_rows=True, vector_tail=False):
    """y[m] = W[m, :K] . x[:K] in fp32, one 'block' per ROWS_PER_BLOCK rows, from raw pointers."""
    Kr = (K + VEC - 1) // VEC * VEC if vector_tail else K        # the bug: a whole 16-B vector past K
    xr = _flat(x, Kr).float()
    Wr = torch.as_strided(W, (M, Kr), (ldw, 1), W.storage_offset()).float()
    for row0 in range(0, M, ROWS_PER_BLOCK):
        n = min(ROWS_PER_BLOCK, M - row0)
        acc = Wr[row0:row0 + n] @ xr
        if clamp_rows:
            _flat(y, M)[row0:row0 + n] = acc.to(y.dtype)
        else:                                                     # the bug: stores a full block of rows
            out = torch.zeros(ROWS_PER_BLOCK)
            out[:n] = acc
            _flat(y, row0 + ROWS_PER_BLOCK)[row0:] = out.to(y.dtype)


def splitk_reduce(parts, ws, y, *, zero_first):
    """y = sum of the partial vectors, accumulated through the workspace."""
    n = parts.shape[1]
    w = _flat(ws, n)
    if zero_first:
        w.zero_()
    for p in parts:                                               # the bug (zero_first=False): += into garbage
        w += p
    _flat(y, n).copy_(w)


def dequant(codes, n, out, *, per_thread_tail):
    """out[i] = nibble i of codes, 16 codes per 'thread'."""
    nib = torch.stack([codes >> 4, codes & 15], 1).reshape(-1).float()
    if per_thread_tail:                                           # the bug: the last thread stores all 16
        m = (n + 15) // 16 * 16
        vals = torch.zeros(m)
        vals[:min(m, nib.numel())] = nib[:m]
        _flat(out, m).copy_(vals.to(out.dtype))
    else:
        _flat(out, n).copy_(nib[:n].to(out.dtype))


def _gemv_case(M=13, K=36, ldw=48, **bug):
    g = torch.Generator().manual_seed(1)
    W = torch.randn(M, K, generator=g).half()
    x = torch.randn(K, generator=g).half()
    Wg = guarded(W, row_stride=ldw, name="W")
    xg = guarded(x, name="x")
    yg = guarded(torch.zeros(M).half(), fill="sentinel", name="y")
    gemv(Wg, xg, yg, M, K, ldw, **bug)
    yc = torch.empty(M).half()
    gemv(W, x, yc, M, K, K)
    return Wg, xg, yg, yc


# ---- the correct versions pass ------------------------------------------------------------------

def test_correct_gemv_passes():
    Wg, xg, yg, yc = _gemv_case()
    for v in (Wg, xg):
        assert_unchanged(v)
    assert_untouched(yg)
    assert_same_bits(yg, yc)
    assert bool(changed_payload(yg).all())          # every output element was written (sentinel gone)


def test_correct_reduce_and_dequant_pass():
    parts = torch.randn(4, 37, generator=torch.Generator().manual_seed(2))
    ws, y = _nan_scratch(37), guarded(torch.zeros(37), fill="sentinel")
    splitk_reduce(parts, ws, y, zero_first=True)
    yc = torch.empty(37)
    splitk_reduce(parts, torch.zeros(37), yc, zero_first=True)
    assert_untouched(ws), assert_untouched(y)
    assert_same_bits(y, yc)
    codes = torch.randint(0, 256, (17,), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    out = guarded(torch.zeros(33).half(), fill="sentinel", offset_elems=1)
    dequant(codes, 33, out, per_thread_tail=False)
    assert_untouched(out)


# ---- each wrong one is rejected, and the message names the place --------------------------------

def test_gemv_storing_whole_row_blocks_is_caught():
    _, _, yg, _ = _gemv_case(clamp_rows=False)       # M = 13: the second block stores rows 13..15
    with pytest.raises(AssertionError, match=r"guard overwritten of y: 3 element\(s\).*\+0 elements past the end \(row 0\)"
                                             r"; \+1 elements past the end.*; \+2 elements"):
        assert_untouched(yg)


def test_gemv_summing_a_vector_past_k_is_caught():
    _, _, yg, yc = _gemv_case(vector_tail=True)      # K = 36: lanes 36..39 are x's guard and W's row tail
    assert_untouched(yg)                             # nothing spilled: only the values show it
    with pytest.raises(AssertionError, match=r"y: 13 of 13 elements differ in bits, first at \[\[0\]"):
        assert_same_bits(yg, yc, "y")
    assert bool(torch.isnan(yg).all())               # the poison reached every sum


def test_row_tail_read_alone_is_caught():
    """x is a multiple of the vector, W's rows are not: only the row tails (ldw > K) are foreign."""
    M, K, ldw = 5, 36, 48
    g = torch.Generator().manual_seed(4)
    W, x = torch.randn(M, K, generator=g).half(), torch.zeros(40).half()
    x[:K] = torch.randn(K, generator=g).half()
    yg = guarded(torch.zeros(M).half(), fill="sentinel")
    gemv(guarded(W, row_stride=ldw), x, yg, M, K, ldw, vector_tail=True)
    assert bool(torch.isnan(yg).all())


def test_reduce_assuming_zeroed_workspace_is_caught():
    parts = torch.randn(4, 37, generator=torch.Generator().manual_seed(2))
    ws, y = _nan_scratch(37), guarded(torch.zeros(37), fill="sentinel", name="y")
    splitk_reduce(parts, ws, y, zero_first=False)
    yc = torch.empty(37)
    splitk_reduce(parts, torch.zeros(37), yc, zero_first=False)     # passes on a zeroed workspace ...
    assert torch.equal(yc, parts[0] + parts[1] + parts[2] + parts[3])
    with pytest.raises(AssertionError, match=r"y: 37 of 37 elements differ in bits"):
        assert_same_bits(y, yc, "y")                                # ... and not on a dirty one


def test_dequantiser_storing_16_codes_per_thread_is_caught():
    codes = torch.randint(0, 256, (24,), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    out = guarded(torch.zeros(33).half(), fill="sentinel", name="out")
    dequant(codes, 33, out, per_thread_tail=True)                   # n = 33: elements 33..47 spill
    with pytest.raises(AssertionError, match=r"guard overwritten of out: 15 element\(s\) changed, first at: "
                                             r"\+0 elements past the end \(row 0\); \+1 elements"):
        assert_untouched(out)


def test_row_tail_spill_names_the_row():
    y = guarded(torch.zeros(131, 36).half(), row_stride=48, fill="sentinel", name="Y")
    torch.as_strided(y, (8,), (1,), y.storage_offset() + 129 * 48 + 36).fill_(1.0)   # a vector store past row 129
    with pytest.raises(AssertionError, match=r"\+0 elements past row 129; \+1 elements past row 129; .*\+7 elements "
                                             r"past row 129"):
        assert_untouched(y)
    y2 = guarded(torch.zeros(4, 8), fill="sentinel")
    torch.as_strided(y2, (2,), (1,), y2.storage_offset() - 2).fill_(0.0)
    with pytest.raises(AssertionError, match=r"-2 elements before the payload; -1 elements before the payload"):
        assert_untouched(y2)


def test_modified_input_is_caught():
    x = guarded(torch.ones(9), name="x")
    x[4] = 2.0
    assert_untouched(x)
    with pytest.raises(AssertionError, match=r"input modified of x: 1 element\(s\) changed, first at: payload element 4 "
                                             r"of row 0"):
        assert_unchanged(x)


# ---- the harness itself -------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.uint8,
                                torch.int32, torch.int64])
@pytest.mark.parametrize("off", [0, 1, 3])
def test_alignment_kept_or_broken_as_asked(dt, off):
    t = torch.arange(40).to(dt).reshape(5, 8)
    v = guarded(t, row_stride=16, offset_elems=off, fill="sentinel")
    assert v._footprint.base.data_ptr() % 64 == 0
    assert (v.data_ptr() - v._footprint.base.data_ptr()) % 256 == off * t.element_size() % 256
    assert is_aligned(v) == (off * t.element_size() % 16 == 0)
    assert v.stride() == (16, 1) and same_bits(v, t)
    assert_untouched(v), assert_unchanged(v)


def test_guard_size_rule():
    assert guard_bytes(8, 2) == GUARD_MIN_BYTES == 65536
    assert guard_bytes(4100, 2) == 256 * 4100 * 2                   # 256 row strides, already a multiple of 256 B
    assert guard_bytes(4101, 1) % 256 == 0 and guard_bytes(4101, 1) >= 256 * 4101
    v = guarded(torch.zeros(3, 520).half(), row_stride=528)
    fp = v._footprint
    assert fp.start * 2 >= 256 * 528 * 2
    assert (fp.base.numel() - fp.start - (2 * 528 + 520)) * 2 >= 256 * 528 * 2
    v3 = guarded(torch.zeros(2, 3, 8), row_stride=12)               # leading dims flatten to rows
    assert v3.stride() == (36, 12, 1) and v3._footprint.rows == 6


def test_fills():
    for dt in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        for fill in ("poison", "sentinel"):
            v = guarded(torch.zeros(4, dtype=dt), fill=fill)
            band = v._footprint.base[:4].view(dt)
            assert bool(torch.isnan(band).all())
        assert fill_pattern(dt, "poison") != fill_pattern(dt, "sentinel")
    assert fill_pattern(torch.uint8, "poison") == 0xFF and fill_pattern(torch.uint8, "sentinel") == 0xA5
    assert fill_pattern(torch.int64, "sentinel") & 0xFF == 0xA5
    with pytest.raises(ValueError):
        guarded(torch.zeros(4, dtype=torch.int32))                  # integers must name their out-of-range value
    s = guarded(torch.zeros(4, dtype=torch.int32), fill=77)
    assert int(s._footprint.base[0]) == 77
    lg = guarded(torch.zeros(2, 5).half(), row_stride=8, fill=float("inf"))
    assert bool(torch.isinf(torch.as_strided(lg, (2, 3), (8, 1), lg.storage_offset() + 5)).all())


def test_filled_payloads_and_changed_payload():
    out = guarded(filled((3, 5), torch.float16, "sentinel"), row_stride=8, fill="sentinel")
    assert bool(torch.isnan(out).all()) and same_bits(out, filled((3, 5), torch.float16, "sentinel"))
    assert not bool(changed_payload(out).any())
    out[1, 2:4] = 1.0
    assert torch.nonzero(changed_payload(out)).tolist() == [[1, 2], [1, 3]]
    assert_untouched(out)
    assert bool((filled(7, torch.uint8, "poison") == 0xFF).all()) and filled(7, torch.bool, "sentinel").dtype == torch.bool


def test_same_bits_counts_nan_payloads_and_signed_zeros():
    a = torch.tensor([0.0, 1.0])
    assert same_bits(a, a.clone()) and not same_bits(a, torch.tensor([-0.0, 1.0]))
    n1 = torch.tensor([0x7FC00001], dtype=torch.int32).view(torch.float32)
    n2 = torch.tensor([0x7FC00002], dtype=torch.int32).view(torch.float32)
    assert same_bits(n1, n1.clone()) and not same_bits(n1, n2)
    assert not same_bits(a, a.double()) and not same_bits(a, a[:1])
    v = guarded(n1)                                                  # the copy into the view keeps the payload
    assert same_bits(v, n1)
