"""GPU: the three paged attention launches against the contiguous launches they wrap, bit for bit.

Reference (paged_reference.py): gather the pages a table names into a contiguous [B, Hkv, 128 NP, D]
cache, call the existing launch with L = 128 NP, compare the output bits, scatter the written slots
back and compare the whole pools' bits.  No tolerance anywhere.  B = 3, NP = 3, P = 8, scrambled page
ids, streams 0 and 1 naming page 0, a NaN page behind every entry above a row's needed range,
sentinel pages no table names, pools inside guard bands of at least one page.

Positions below the first page edge go to stream 2, or to one of streams 0 / 1 while the other does not
write: two streams that wrote one slot of a shared page would race, which the host side rules out.
After every call the table, pos and len are unchanged, the pools' guards and every page outside the
written slots keep their bits -- the sentinel pages, the NaN page and, where nobody writes into it,
the shared page included."""
import math

import pytest
import torch

import footprint as fp
import paged_reference as pr
from paged_reference import B, NAN_PAGE, NP, P, PAGE

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
F16, BF16 = torch.float16, torch.bfloat16
SHAPES = [(4, 2, 64), (8, 2, 128)]
L = PAGE * NP
I64 = torch.int64


def _lo():
    from quantizations_amd import layer_ops
    return layer_ops


def _nan_rows(out):
    return torch.isnan(out.float()).all(-1)


class Run:
    """One paged call and its contiguous twin on the same operands."""

    def __init__(self, dt, Hq, Hkv, D, T, last_pos, seed, overrides=None):
        self.Hq, self.D = Hq, D
        self.scale = 1.0 / math.sqrt(D)
        self.table_cpu, self.unnamed = pr.build_table(last_pos, overrides)
        self.table = self.table_cpu.to(DEV)
        self.kp, self.vp = pr.make_pools(dt, Hkv, D, self.unnamed, seed, DEV)
        self.kp0, self.vp0 = self.kp.clone(), self.vp.clone()
        self.ops = pr.operands(dt, Hq, Hkv, D, T, seed + 7, DEV)
        self.kc, self.vc = pr.gather(self.kp0, self.table_cpu), pr.gather(self.vp0, self.table_cpu)
        self.kc0, self.vc0 = self.kc.clone(), self.vc.clone()

    def check(self, out, ref, written, pos, pos0, length=None, len0=None, skipped=None):
        """out == ref in bits; pools == scatter of the contiguous caches; nothing else moved."""
        torch.cuda.synchronize()
        fp.assert_same_bits(out, ref, "out")
        for pool, pool0, c0, c1, name in ((self.kp, self.kp0, self.kc0, self.kc, "k_pool"),
                                          (self.vp, self.vp0, self.vc0, self.vc, "v_pool")):
            fp.assert_untouched(pool, name)
            want = pr.scatter(pool0, c0, c1, self.table_cpu, written, skipped)
            fp.assert_same_bits(pool, want, name)
            for p in self.unnamed + [NAN_PAGE]:
                fp.assert_same_bits(pool[p], pool0[p], f"{name} page {p}")
            if not any((j >> 7) == 0 for b in (0, 1) for j in written.get(b, ())):
                fp.assert_same_bits(pool[0], pool0[0], f"{name} shared page")
        assert torch.equal(self.table.cpu(), self.table_cpu), "the table changed"
        assert torch.equal(pos.cpu(), pos0), "pos changed"
        if length is not None:
            assert torch.equal(length.cpu(), len0), "len changed"


# every position of {0, 1, 127, 128, 129, 255, 256, 383}; streams 0 and 1 stay out of the shared page
DECODE_ROUNDS = [(128, 255, 0), (129, 256, 1), (383, 128, 127), (255, 383, 129)]


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_decode_paged_equals_streams_on_the_gathered_cache(dt, Hq, Hkv, D):
    lo = _lo()
    for i, ps in enumerate(DECODE_ROUNDS):
        r = Run(dt, Hq, Hkv, D, 1, ps, 10 * i)
        q, k, v, cos, sin = r.ops
        pos0 = torch.tensor(ps, dtype=I64)
        pos = pos0.to(DEV)
        assert lo.decode_attention_paged_supported(q, cos, r.kp, r.vp, r.table, pos, Hq)
        out = lo.decode_attention_paged(q, k, v, cos, sin, r.kp, r.vp, r.table, pos, Hq, r.scale)
        ref = lo.decode_attention_streams(q, k, v, cos, sin, r.kc, r.vc, pos, Hq, r.scale)
        assert not torch.isnan(out.float()).any()
        r.check(out, ref, {b: [p] for b, p in enumerate(ps)}, pos, pos0)


# T = 4 at 126 (rows on both sides of a page edge), 0, 380, and 382 (the last two rows past L)
VERIFY_ROUNDS = [(380, 129, 126), (255, 380, 0), (382, 200, 50)]


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_verify_paged_equals_verify_on_the_gathered_cache(dt, Hq, Hkv, D):
    lo, T = _lo(), 4
    for i, ps in enumerate(VERIFY_ROUNDS):
        r = Run(dt, Hq, Hkv, D, T, [p + T - 1 for p in ps], 100 + 10 * i)
        q, k, v, cos, sin = r.ops
        pos0 = torch.tensor(ps, dtype=I64)
        pos = pos0.to(DEV)
        assert lo.decode_attention_verify_paged_supported(q, cos, r.kp, r.vp, r.table, pos, Hq)
        out = lo.decode_attention_verify_paged(q, k, v, cos, sin, r.kp, r.vp, r.table, pos, Hq, r.scale)
        ref = lo.decode_attention_verify(q, k, v, cos, sin, r.kc, r.vc, pos, Hq, r.scale)
        legal = torch.tensor([[p + t < L for t in range(T)] for p in ps])
        assert torch.equal(_nan_rows(out).cpu(), ~legal), "NaN for exactly the rows past L"
        assert not torch.isnan(out.float()[legal.to(DEV)]).any()
        r.check(out, ref, {b: [p + t for t in range(T) if p + t < L] for b, p in enumerate(ps)}, pos, pos0)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
@pytest.mark.parametrize("ps,ns", [((100, 100, 100), (70, 0, 33)), ((130, 40, 100), (33, 0, 70))],
                         ids=["from100", "private-writers"])
def test_prefill_paged_equals_prefill_on_the_gathered_cache(dt, Hq, Hkv, D, ps, ns):
    """T = 70 from position 100: the page edge at 128, a key-tile edge, the query-tile edge at row 64, an
    idle stream and a ragged one.  In the first case stream 0 writes slots 100..127 of page 0, which the
    idle stream 1 names too; in the second every writer owns its pages and the shared page keeps its bits."""
    lo, T = _lo(), 70
    r = Run(dt, Hq, Hkv, D, T, [p + n - 1 if n else p for p, n in zip(ps, ns)], 200)
    q, k, v, cos, sin = r.ops
    pos0, len0 = torch.tensor(ps, dtype=I64), torch.tensor(ns, dtype=I64)
    pos, length = pos0.to(DEV), len0.to(DEV)
    assert lo.prefill_attention_paged_supported(q, cos, r.kp, r.vp, r.table, pos, length, Hq)
    out = lo.prefill_attention_paged(q, k, v, cos, sin, r.kp, r.vp, r.table, pos, length, Hq, r.scale)
    ref = lo.prefill_attention(q, k, v, cos, sin, r.kc, r.vc, pos, length, Hq, r.scale)
    for b, n in enumerate(ns):
        assert not torch.isnan(out[b, :n].float()).any() and bool((out[b, n:] == 0).all())
    r.check(out, ref, {b: list(range(p, p + n)) for b, (p, n) in enumerate(zip(ps, ns))}, pos, pos0, length, len0)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_prefill_paged_in_two_halves_equals_one_call(dt, Hq, Hkv, D):
    """T = 200 from 0 split at row 128, streams 0 and 2 (stream 1 is idle: it shares stream 0's first
    page): outputs and pools carry the bits of the single call, and of the contiguous single call."""
    lo, T = _lo(), 200
    ns = (T, 0, T)
    whole = Run(dt, Hq, Hkv, D, T, [T - 1, 0, T - 1], 300)
    halves = Run(dt, Hq, Hkv, D, T, [T - 1, 0, T - 1], 300)
    q, k, v, cos, sin = whole.ops
    pos0, len0 = torch.zeros(B, dtype=I64), torch.tensor(ns, dtype=I64)
    pos, length = pos0.to(DEV), len0.to(DEV)
    out = lo.prefill_attention_paged(q, k, v, cos, sin, whole.kp, whole.vp, whole.table, pos, length, Hq, whole.scale)
    ref = lo.prefill_attention(q, k, v, cos, sin, whole.kc, whole.vc, pos, length, Hq, whole.scale)
    whole.check(out, ref, {0: list(range(T)), 2: list(range(T))}, pos, pos0, length, len0)
    parts = []
    for lo_row, hi_row in ((0, 128), (128, T)):
        n = hi_row - lo_row
        p_h = torch.full((B,), lo_row, dtype=I64, device=DEV)
        l_h = torch.tensor([n, 0, n], dtype=I64, device=DEV)
        sl = [t[:, lo_row:hi_row].contiguous() for t in (q, k, v, cos, sin)]
        parts.append(lo.prefill_attention_paged(*sl, halves.kp, halves.vp, halves.table, p_h, l_h, Hq, halves.scale))
    torch.cuda.synchronize()
    got = torch.cat(parts, 1)
    for b in (0, 2):
        fp.assert_same_bits(got[b], out[b], f"stream {b}")
    fp.assert_same_bits(halves.kp, whole.kp, "k_pool")
    fp.assert_same_bits(halves.vp, whole.vp, "v_pool")
    fp.assert_untouched(halves.kp, "k_pool")
    fp.assert_untouched(halves.vp, "v_pool")


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
@pytest.mark.parametrize("bad", [-1, P], ids=["minus1", "P"])
def test_invalid_entries_are_never_addresses(dt, Hq, Hkv, D, bad):
    """Entries -1 and P only: the page before and the page after the pool lie inside its guards, so a
    missing check shows as a wrong value or a touched guard.  NaN for exactly the rows that need the
    entry, nothing written by the rows that write through it, the other rows' bits unchanged."""
    lo = _lo()
    # decode: stream 0 (pos 200) misses entry 0 and still writes through entry 1; stream 1 (pos 130)
    # misses its write entry; stream 2 is whole.  The entries above the needed range are invalid too.
    ps = (200, 130, 127)
    r = Run(dt, Hq, Hkv, D, 1, ps, 400, {(0, 0): bad, (1, 1): bad, (0, 2): bad, (2, 1): bad, (2, 2): bad})
    q, k, v, cos, sin = r.ops
    pos0 = torch.tensor(ps, dtype=I64)
    pos = pos0.to(DEV)
    out = lo.decode_attention_paged(q, k, v, cos, sin, r.kp, r.vp, r.table, pos, Hq, r.scale)
    ref = lo.decode_attention_streams(q, k, v, cos, sin, r.kc, r.vc, pos, Hq, r.scale)
    assert _nan_rows(out)[:, 0].tolist() == [True, True, False]
    ref[:2] = out[:2]
    r.check(out, ref, {0: [200], 2: [127]}, pos, pos0, skipped={1: [130]})

    # verify, T = 4 at 126 on stream 2 with entry 1 invalid: rows 126 and 127 are whole and written, rows
    # 128 and 129 are NaN and write nothing; stream 0 (pos 300) is whole
    T, ps = 4, (300, 140, 126)
    r = Run(dt, Hq, Hkv, D, T, [p + T - 1 for p in ps], 500, {(2, 1): bad, (2, 2): bad, (1, 0): bad})
    q, k, v, cos, sin = r.ops
    pos0 = torch.tensor(ps, dtype=I64)
    pos = pos0.to(DEV)
    out = lo.decode_attention_verify_paged(q, k, v, cos, sin, r.kp, r.vp, r.table, pos, Hq, r.scale)
    ref = lo.decode_attention_verify(q, k, v, cos, sin, r.kc, r.vc, pos, Hq, r.scale)
    assert _nan_rows(out).tolist() == [[False] * 4, [True] * 4, [False, False, True, True]]
    ref[1], ref[2, 2:] = out[1], out[2, 2:]
    r.check(out, ref, {0: [300, 301, 302, 303], 1: [140, 141, 142, 143], 2: [126, 127]}, pos, pos0, skipped={2: [128, 129]})

    # prefill, T = 70 from 100 on stream 2 with entry 1 invalid: the 28 rows below the page edge are
    # whole, the rest NaN and unwritten; stream 0 (33 rows from 130) is whole; stream 1 is idle
    T, ps, ns = 70, (130, 40, 100), (33, 0, 70)
    r = Run(dt, Hq, Hkv, D, T, [162, 40, 169], 600, {(2, 1): bad, (2, 2): bad, (0, 2): bad})
    q, k, v, cos, sin = r.ops
    pos0, len0 = torch.tensor(ps, dtype=I64), torch.tensor(ns, dtype=I64)
    pos, length = pos0.to(DEV), len0.to(DEV)
    out = lo.prefill_attention_paged(q, k, v, cos, sin, r.kp, r.vp, r.table, pos, length, Hq, r.scale)
    ref = lo.prefill_attention(q, k, v, cos, sin, r.kc, r.vc, pos, length, Hq, r.scale)
    want_nan = torch.zeros(B, T, dtype=torch.bool)
    want_nan[2, 28:] = True
    assert torch.equal(_nan_rows(out).cpu(), want_nan)
    ref[2, 28:] = out[2, 28:]
    r.check(out, ref, {0: list(range(130, 163)), 2: list(range(100, 128))}, pos, pos0, length, len0,
            skipped={2: list(range(128, 170))})


def test_wrappers_reject_what_the_launch_cannot_take():
    lo = _lo()
    r = Run(F16, 4, 2, 64, 1, (128, 255, 0), 0)
    q, k, v, cos, sin = r.ops
    pos = torch.tensor((128, 255, 0), dtype=I64, device=DEV)
    assert not lo.decode_attention_paged_supported(q, cos, r.kp, r.vp, r.table.long(), pos, 4)
    assert not lo.decode_attention_paged_supported(q, cos, r.kp, r.vp, r.table.t().contiguous().t(), pos, 4)
    assert not lo.decode_attention_paged_supported(q, cos, r.kp[:, :, :64], r.vp[:, :, :64], r.table, pos, 4)
    assert not lo.decode_attention_paged_supported(q, cos, r.kp, r.vp, r.table, pos.int(), 4)
    assert not lo.decode_attention_paged_supported(q, cos, r.kp, r.vp, r.table[:2], pos, 4)
    with pytest.raises(ValueError):
        lo.decode_attention_paged(q, k, v, cos, sin, r.kp, r.vp, r.table.long(), pos, 4, 0.125)
    with pytest.raises(ValueError):
        lo.prefill_attention_paged(q, k, v, cos, sin, r.kp, r.vp, r.table, pos, pos.int(), 4, 0.125)
    with pytest.raises(ValueError):
        lo.decode_attention_verify_paged(q, k, v, cos, sin, r.kp, r.vp, r.table, pos, 4, 0.125)   # T = 1
