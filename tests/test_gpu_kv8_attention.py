"""GPU: the three kv8 attention launches, every comparison one of bits (NaN compared as NaN).

Write contract: what a kv8 launch stores is pack_pool(quantize_rows(...)) (kv8_reference.py) of the rows
its 16-bit paged twin stores on equal operands, at exactly the written slots; every other byte of the
pools and their guards keeps its value.  Read contract: the output is the 16-bit paged twin's on the
dequantised pools, with identity cos / sin, the host-rotated q (torch's per-op rounding, as
prefill_reference.py restates it) and the dequantised new rows.  Shapes, tables and positions are
test_gpu_paged_attention.py's (paged_reference.py): B = 3, NP = 3, P = 8, a scrambled table, streams 0
and 1 naming page 0, an all-NaN page (scale bytes 255) behind every entry above a row's needed range.

The every-pattern tests decide which conversion instructions may stay: all 65536 bit patterns of each
dtype go through the writer, and every code at every legal scale byte comes back through the decode
launch."""
import math

import pytest
import torch

import footprint as fp
import kv8_reference as k8
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


def _rotate(x, cos, sin, H, D):
    """apply_rotary_pos_emb on [B, T, H D] rows, torch's per-op rounding in the dtype (CPU)."""
    xh = x.cpu().view(x.shape[0], x.shape[1], H, D)
    c, s = cos.cpu().unsqueeze(2), sin.cpu().unsqueeze(2)
    half = torch.cat((-xh[..., D // 2:], xh[..., :D // 2]), -1)
    return ((xh * c) + (half * s)).reshape(x.shape)


def _requantised(x, H, D):
    """[B, T, H D] rows as they read back from a kv8 cache."""
    xh = x.cpu().view(x.shape[0], x.shape[1], H, D)
    return k8.dequantize_rows(*k8.quantize_rows(xh), x.dtype).reshape(x.shape)


def _same(a, b, name):
    """Bit equality where neither is NaN, NaN exactly where the other is."""
    a, b = a.cpu(), b.cpu()
    na, nb = torch.isnan(a.float()), torch.isnan(b.float())
    assert torch.equal(na, nb), f"{name}: NaN in different places ({int(na.sum())} vs {int(nb.sum())})"
    fp.assert_same_bits(torch.where(na, torch.zeros((), dtype=a.dtype), a), torch.where(nb, torch.zeros((), dtype=b.dtype), b), name)


def _source_pools(dt, Hkv, D, unnamed, seed):
    """Two 16-bit pools [P, Hkv, 128, D] (CPU) whose rows span many scales, with the NaN page."""
    out = []
    for s in (seed, seed + 1):
        g = torch.Generator().manual_seed(s)
        mag = torch.pow(2.0, torch.randint(-6, 7, (P, Hkv, PAGE, 1), generator=g).float())
        pool = (torch.randn((P, Hkv, PAGE, D), generator=g) * mag).to(dt)
        pool[NAN_PAGE] = float("nan")
        out.append(pool)
    return out


class Case:
    """kv8 pools (guarded) quantised from random rows, the 16-bit pools they dequantise to, one set of
    operands, and the three runs a check needs: the kv8 launch, its 16-bit twin on equal operands (what
    rows get stored) and the read-contract twin."""

    def __init__(self, dt, Hq, Hkv, D, T, last_pos, seed, overrides=None, nan_row=None, nan_token=None):
        self.dt, self.Hq, self.Hkv, self.D, self.T = dt, Hq, Hkv, D, T
        self.scale = 1.0 / math.sqrt(D)
        self.table_cpu, self.unnamed = pr.build_table(last_pos, overrides)
        self.table = self.table_cpu.to(DEV)
        src = _source_pools(dt, Hkv, D, self.unnamed, seed)
        if nan_row is not None:                         # (page, kv head, slot): a row of s = 255 in both pools
            for pool in src:
                pool[nan_row] = float("nan")
        self.pools8, self.pools16 = [], []
        for pool in src:
            p8 = k8.quantize_pool(pool)
            for pg in self.unnamed:
                p8[pg] = 0xA5
            self.pools16.append(k8.dequantize_pool(p8, D, dt).to(DEV))
            v = fp.guarded(p8.to(DEV), fill="poison", name="pool")
            assert v.is_contiguous() and v.data_ptr() % 16 == 0
            self.pools8.append(v)
        self.kp, self.vp = self.pools8
        self.before = [p.cpu().clone() for p in self.pools8]
        self.ops = pr.operands(dt, Hq, Hkv, D, T, seed + 7, DEV)
        if nan_token is not None:                       # (b, i): token i of stream b carries a NaN in k's head 0
            self.ops[1][nan_token[0], nan_token[1], 3] = float("nan")

    def launch(self, kind, pools, ops, pos, length, kv8):
        lo = _lo()
        sfx = "_kv8" if kv8 else ""
        q, k, v, cos, sin = ops
        if kind == "prefill":
            fn = getattr(lo, "prefill_attention_paged" + sfx)
            assert getattr(lo, "prefill_attention_paged" + sfx + "_supported")(q, cos, *pools, self.table, pos, length, self.Hq)
            return fn(q, k, v, cos, sin, *pools, self.table, pos, length, self.Hq, self.scale)
        name = {"decode": "decode_attention_paged", "verify": "decode_attention_verify_paged"}[kind] + sfx
        assert getattr(lo, name + "_supported")(q, cos, *pools, self.table, pos, self.Hq)
        return getattr(lo, name)(q, k, v, cos, sin, *pools, self.table, pos, self.Hq, self.scale)

    def twin_operands(self, ops=None):
        q, k, v, cos, sin = ops or self.ops
        qr = _rotate(q, cos, sin, self.Hq, self.D).to(DEV)
        kq = _requantised(_rotate(k, cos, sin, self.Hkv, self.D), self.Hkv, self.D).to(DEV)
        vq = _requantised(v, self.Hkv, self.D).to(DEV)
        return qr, kq, vq, torch.ones_like(cos), torch.zeros_like(sin)

    def run(self, kind, ps, ns=None):
        pos0 = torch.tensor(ps, dtype=I64)
        pos = pos0.to(DEV)
        len0 = None if ns is None else torch.tensor(ns, dtype=I64)
        length = None if ns is None else len0.to(DEV)
        out = self.launch(kind, self.pools8, self.ops, pos, length, True)
        self.stored = [p.clone() for p in self.pools16]             # what the 16-bit twin stores
        self.launch(kind, self.stored, self.ops, pos, length, False)
        ref = self.launch(kind, [p.clone() for p in self.pools16], self.twin_operands(), pos, length, False)
        torch.cuda.synchronize()
        assert torch.equal(self.table.cpu(), self.table_cpu) and torch.equal(pos.cpu(), pos0)
        assert ns is None or torch.equal(length.cpu(), len0)
        return out, ref

    def check_pools(self, written):
        """written {b: positions}: those slots hold the quantised rows the 16-bit launch stored, every
        other byte and the guards are as they were."""
        for pool, before, stored, name in zip(self.pools8, self.before, self.stored, ("k_pool", "v_pool")):
            fp.assert_untouched(pool, name)
            codes, scales = (t.clone() for t in k8.unpack_pool(before, self.D))
            stored = stored.cpu()
            for b, slots in written.items():
                for j in slots:
                    pg = int(self.table_cpu[b, j >> 7])
                    c, s = k8.quantize_rows(stored[pg, :, j & (PAGE - 1)])
                    codes[pg, :, j & (PAGE - 1)], scales[pg, :, j & (PAGE - 1)] = c, s
            fp.assert_same_bits(pool.cpu(), k8.pack_pool(codes, scales), name)


DECODE_ROUNDS = [(128, 255, 0), (129, 256, 1), (383, 128, 127), (255, 383, 129)]
VERIFY_ROUNDS = [(380, 129, 126), (255, 380, 0), (382, 200, 50)]
PARAMS = [pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"]), pytest.mark.parametrize("Hq,Hkv,D", SHAPES)]


def _both(f):
    for m in PARAMS:
        f = m(f)
    return f


@_both
def test_decode_kv8_write_and_read_contracts(dt, Hq, Hkv, D):
    for i, ps in enumerate(DECODE_ROUNDS):
        c = Case(dt, Hq, Hkv, D, 1, ps, 10 * i)
        out, ref = c.run("decode", ps)
        assert not torch.isnan(out.float()).any()
        _same(out, ref, f"out {ps}")
        c.check_pools({b: [p] for b, p in enumerate(ps)})


@_both
def test_verify_kv8_write_and_read_contracts(dt, Hq, Hkv, D):
    T = 4
    for i, ps in enumerate(VERIFY_ROUNDS):
        c = Case(dt, Hq, Hkv, D, T, [p + T - 1 for p in ps], 100 + 10 * i)
        out, ref = c.run("verify", ps)
        legal = torch.tensor([[p + t < L for t in range(T)] for p in ps])
        assert torch.equal(torch.isnan(out.float()).all(-1).cpu(), ~legal), "NaN for exactly the rows past L"
        _same(out, ref, f"out {ps}")
        c.check_pools({b: [p + t for t in range(T) if p + t < L] for b, p in enumerate(ps)})


@_both
@pytest.mark.parametrize("ps,ns", [((100, 100, 100), (70, 0, 33)), ((130, 40, 100), (33, 0, 70))],
                         ids=["from100", "private-writers"])
def test_prefill_kv8_write_and_read_contracts(dt, Hq, Hkv, D, ps, ns):
    T = 70
    c = Case(dt, Hq, Hkv, D, T, [p + n - 1 if n else p for p, n in zip(ps, ns)], 200)
    out, ref = c.run("prefill", ps, ns)
    for b, n in enumerate(ns):
        assert not torch.isnan(out[b, :n].float()).any() and bool((out[b, n:] == 0).all())
    _same(out, ref, "out")
    c.check_pools({b: list(range(p, p + n)) for b, (p, n) in enumerate(zip(ps, ns))})


@_both
def test_prefill_kv8_in_two_halves_equals_one_call(dt, Hq, Hkv, D):
    T, ns = 200, (200, 0, 200)
    whole = Case(dt, Hq, Hkv, D, T, [T - 1, 0, T - 1], 300)
    halves = Case(dt, Hq, Hkv, D, T, [T - 1, 0, T - 1], 300)
    out, ref = whole.run("prefill", (0, 0, 0), ns)
    _same(out, ref, "whole")
    whole.check_pools({0: list(range(T)), 2: list(range(T))})
    parts = []
    for lo_row, hi_row in ((0, 128), (128, T)):
        n = hi_row - lo_row
        p_h = torch.full((B,), lo_row, dtype=I64, device=DEV)
        l_h = torch.tensor([n, 0, n], dtype=I64, device=DEV)
        sl = [t[:, lo_row:hi_row].contiguous() for t in halves.ops]
        parts.append(halves.launch("prefill", halves.pools8, sl, p_h, l_h, True))
    torch.cuda.synchronize()
    got = torch.cat(parts, 1)
    for b in (0, 2):
        fp.assert_same_bits(got[b], out[b], f"stream {b}")
    for a, b_, name in zip(halves.pools8, whole.pools8, ("k_pool", "v_pool")):
        fp.assert_same_bits(a, b_, name)
        fp.assert_untouched(a, name)


@_both
def test_one_verify_call_equals_successive_decode_calls(dt, Hq, Hkv, D):
    """The speculative contract: T = 4 rows in one call are the four decode steps, in outputs and bytes."""
    T, ps = 4, (380, 129, 126)
    one = Case(dt, Hq, Hkv, D, T, [p + T - 1 for p in ps], 700)
    steps = Case(dt, Hq, Hkv, D, T, [p + T - 1 for p in ps], 700)
    pos = torch.tensor(ps, dtype=I64, device=DEV)
    out = one.launch("verify", one.pools8, one.ops, pos, None, True)
    got = []
    for i in range(T):
        sl = [t[:, i:i + 1].contiguous() for t in steps.ops]
        got.append(steps.launch("decode", steps.pools8, sl, pos + i, None, True))
    torch.cuda.synchronize()
    fp.assert_same_bits(torch.cat(got, 1), out, "out")
    for a, b_, name in zip(steps.pools8, one.pools8, ("k_pool", "v_pool")):
        fp.assert_same_bits(a, b_, name)
        fp.assert_untouched(a, name)
        fp.assert_untouched(b_, name)


def _pattern_rows(dt, shift):
    """All 65536 bit patterns of dt as rows of 64: 63 patterns of neighbouring magnitude and, in slot 63, a
    pivot 2^shift times the largest of them (capped at the largest finite number) -- the row's largest
    element, so the 63 are quantised `shift` binades below the top of the code range.  [1041, 64]."""
    pats = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dt)
    mag = pats.float().abs()
    order = torch.argsort(torch.where(torch.isnan(mag), torch.full((), float("inf")), mag), stable=True)
    pats = torch.cat((pats[order], pats[order][-(63 * 1041 - 65536):]))       # pad with the last (non-finite) ones
    rows = pats.reshape(1041, 63)
    top = rows.float().abs().amax(-1)
    pivot = torch.clamp(top * 2.0 ** shift, max=torch.finfo(dt).max).to(dt)
    pivot = torch.where(torch.isfinite(top), pivot, top.to(dt))
    return torch.cat((rows, pivot.unsqueeze(-1)), -1)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
def test_every_bit_pattern_through_the_writer(dt):
    """Six pivots per pattern (shifts 0, 1, 2, 4, 7, 10 binades), identity cos / sin, D = 64: the codes
    and the scale byte of every row equal the reference's.  K goes through the rotary (x 1 + rot(x) 0, the
    reference applies it too: -0 may come out +0, an inf makes its partner NaN), V is stored as given."""
    lo, D, Hkv = _lo(), 64, 8
    rows = torch.cat([_pattern_rows(dt, s) for s in (0, 1, 2, 4, 7, 10)])        # [6246, 64]
    T = -(-rows.shape[0] // Hkv)
    rows = torch.cat((rows, torch.zeros((T * Hkv - rows.shape[0], D), dtype=dt)))
    npg = -(-T // PAGE)
    kv = rows.reshape(1, T, Hkv * D)
    ones, zeros = torch.ones((1, T, D), dtype=dt), torch.zeros((1, T, D), dtype=dt)
    q = torch.zeros((1, T, Hkv * D), dtype=dt, device=DEV)
    pools = [fp.guarded(torch.zeros((npg, Hkv, PAGE * (D + 1)), dtype=torch.uint8, device=DEV), name="pool") for _ in range(2)]
    table = torch.arange(npg, dtype=torch.int32, device=DEV).flip(0).reshape(1, npg).contiguous()
    pos, length = torch.zeros(1, dtype=I64, device=DEV), torch.tensor([T], dtype=I64, device=DEV)
    lo.prefill_attention_paged_kv8(q, kv.to(DEV), kv.to(DEV), ones.to(DEV), zeros.to(DEV), *pools, table, pos, length,
                                   Hkv, 0.125)
    torch.cuda.synchronize()
    want_rows = {"k_pool": _rotate(kv, ones, zeros, Hkv, D), "v_pool": kv}
    for pool, name in zip(pools, ("k_pool", "v_pool")):
        fp.assert_untouched(pool, name)
        codes, scales = k8.unpack_pool(pool.cpu().flip(0), D)                   # pages in position order
        got_c = codes.permute(0, 2, 1, 3).reshape(npg * PAGE, Hkv, D)[:T]
        got_s = scales.permute(0, 2, 1).reshape(npg * PAGE, Hkv)[:T]
        want_c, want_s = k8.quantize_rows(want_rows[name].view(T, Hkv, D))
        bad = (got_s != want_s).nonzero()
        assert bad.numel() == 0, (name, "scale", bad[:4].tolist(), got_s[got_s != want_s][:4], want_s[got_s != want_s][:4])
        bad = (got_c != want_c).nonzero()
        assert bad.numel() == 0, (name, "codes", bad[:4].tolist(), got_c[got_c != want_c][:4], want_c[got_c != want_c][:4])


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
def test_every_code_at_every_legal_scale_reads_back_exactly(dt):
    """One (stream, kv head) per row of 64 codes at one scale byte (every s from e_min + 127 to the
    largest the rule produces, and 255).  The row is v of key 0; key 0's k is +8 and the query 8, the new
    token's k is -8 and its v zero, so the new token's weight is exp(-1024) = 0 exactly and the output is
    v of key 0: the reference's dequantised value, inf and NaN included (the sign of a zero aside)."""
    lo, D, Hkv = _lo(), 64, 8
    svals = list(range(k8.E_MIN[dt] + 127, k8.E_MAX[dt] + 127 + 1)) + [255]
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8).reshape(1, 4, D).expand(len(svals), 4, D).reshape(-1, D)
    scales = torch.tensor(svals, dtype=torch.int32).to(torch.uint8).repeat_interleave(4)
    nb = -(-codes.shape[0] // Hkv)
    pad = nb * Hkv - codes.shape[0]
    codes = torch.cat((codes, torch.zeros((pad, D), dtype=torch.uint8))).reshape(nb, Hkv, 1, D)
    scales = torch.cat((scales, torch.full((pad,), 127, dtype=torch.uint8))).reshape(nb, Hkv, 1)
    vc, vs = torch.zeros((nb, Hkv, PAGE, D), dtype=torch.uint8), torch.zeros((nb, Hkv, PAGE), dtype=torch.uint8)
    vc[:, :, :1], vs[:, :, :1] = codes, scales
    kc, ks = torch.zeros_like(vc), torch.zeros_like(vs)
    kc[:, :, 0], ks[:, :, 0] = 0x50, 127                                   # 8.0
    pools = [fp.guarded(k8.pack_pool(c, s).to(DEV), name="pool") for c, s in ((kc, ks), (vc, vs))]
    table = torch.arange(nb, dtype=torch.int32, device=DEV).reshape(nb, 1)
    pos = torch.ones(nb, dtype=I64, device=DEV)
    q = torch.full((nb, 1, Hkv * D), 8.0, dtype=dt, device=DEV)
    ones, zeros = torch.ones((nb, 1, D), dtype=dt, device=DEV), torch.zeros((nb, 1, D), dtype=dt, device=DEV)
    out = lo.decode_attention_paged_kv8(q, -q, torch.zeros_like(q), ones, zeros, *pools, table, pos, Hkv, 0.125)
    torch.cuda.synchronize()
    want = k8.dequantize_rows(codes[:, :, 0], scales[:, :, 0], dt).reshape(nb, 1, Hkv * D)
    assert bool(torch.isinf(want.float()).any()) and bool(torch.isnan(want.float()).any())   # the top scale; s = 255
    # the P V sum starts from +0, so a -0 reads back as +0: zeros compare by value
    out, want = (torch.where(t == 0, torch.zeros((), dtype=dt), t) for t in (out.cpu(), want))
    _same(out, want, "v of key 0")
    for pool in pools:
        fp.assert_untouched(pool, "pool")


@_both
@pytest.mark.parametrize("bad", [-1, P], ids=["minus1", "P"])
def test_invalid_entries_are_never_addresses(dt, Hq, Hkv, D, bad):
    """test_gpu_paged_attention.py's cases on the kv8 launches: entries -1 and P lie inside the pools'
    guards.  NaN for exactly the rows that need the entry, nothing written through it, the other rows'
    bits those of the twin."""
    ps = (200, 130, 127)
    c = Case(dt, Hq, Hkv, D, 1, ps, 400, {(0, 0): bad, (1, 1): bad, (0, 2): bad, (2, 1): bad, (2, 2): bad})
    out, ref = c.run("decode", ps)
    assert torch.isnan(out.float()).all(-1)[:, 0].tolist() == [True, True, False]
    _same(out[2], ref[2], "stream 2")
    c.check_pools({0: [200], 2: [127]})

    T, ps = 4, (300, 140, 126)
    c = Case(dt, Hq, Hkv, D, T, [p + T - 1 for p in ps], 500, {(2, 1): bad, (2, 2): bad, (1, 0): bad})
    out, ref = c.run("verify", ps)
    assert torch.isnan(out.float()).all(-1).tolist() == [[False] * 4, [True] * 4, [False, False, True, True]]
    _same(out[0], ref[0], "stream 0")
    _same(out[2, :2], ref[2, :2], "stream 2")
    c.check_pools({0: [300, 301, 302, 303], 1: [140, 141, 142, 143], 2: [126, 127]})

    T, ps, ns = 70, (130, 40, 100), (33, 0, 70)
    c = Case(dt, Hq, Hkv, D, T, [162, 40, 169], 600, {(2, 1): bad, (2, 2): bad, (0, 2): bad})
    out, ref = c.run("prefill", ps, ns)
    want_nan = torch.zeros(B, T, dtype=torch.bool)
    want_nan[2, 28:] = True
    assert torch.equal(torch.isnan(out.float()).all(-1).cpu(), want_nan)
    _same(out, ref, "out")
    c.check_pools({0: list(range(130, 163)), 2: list(range(100, 128))})


@_both
def test_a_non_finite_row_is_nan_for_exactly_the_rows_that_see_it(dt, Hq, Hkv, D):
    """A row with s = 255.  Decode: it lies in stream 1's second page, kv head 0 -- stream 1's query heads
    of that kv head are NaN, nothing else.  Verify: token 2 of stream 2 carries a NaN in k's head 0 -- the
    writer stores s = 255 and rows 2 and 3 of that kv head are NaN.  (The prefill tile multiplies a masked
    key's v by a zero weight, as its 16-bit twins do, so a NaN row inside a window also reaches the rows
    below it in its 64-key tile; its contract is the twin's bits, checked above.)"""
    G = Hq // Hkv
    ps = (128, 255, 0)
    table, _ = pr.build_table(ps)
    c = Case(dt, Hq, Hkv, D, 1, ps, 800, nan_row=(int(table[1, 1]), 0, 72))
    out, ref = c.run("decode", ps)
    nan = torch.isnan(out.float()).view(B, Hq, D)
    want = torch.zeros(B, Hq, dtype=torch.bool)
    want[1, :G] = True
    assert torch.equal(nan.all(-1).cpu(), want) and torch.equal(nan.any(-1).cpu(), want)
    _same(out, ref, "decode")

    T, ps = 4, (380, 129, 50)
    c = Case(dt, Hq, Hkv, D, T, [p + T - 1 for p in ps], 810, nan_token=(2, 2))
    out, ref = c.run("verify", ps)
    nan = torch.isnan(out.float()).view(B, T, Hq, D)
    want = torch.zeros(B, T, Hq, dtype=torch.bool)
    want[2, 2:, :G] = True
    assert torch.equal(nan.all(-1).cpu(), want) and torch.equal(nan.any(-1).cpu(), want)
    _same(out, ref, "verify")
    _, scales = k8.unpack_pool(c.kp.cpu(), D)
    assert scales[int(c.table_cpu[2, 0]), :, 50:54].tolist()[0][2] == 255


def test_wrappers_reject_what_the_launch_cannot_take():
    lo = _lo()
    c = Case(F16, 4, 2, 64, 1, (128, 255, 0), 0)
    q, k, v, cos, sin = c.ops
    pos = torch.tensor((128, 255, 0), dtype=I64, device=DEV)
    k16, v16 = c.pools16
    assert lo.decode_attention_paged_kv8_supported(q, cos, c.kp, c.vp, c.table, pos, 4)
    assert not lo.decode_attention_paged_kv8_supported(q, cos, k16, v16, c.table, pos, 4)                 # 16-bit pools
    assert not lo.decode_attention_paged_supported(q, cos, c.kp, c.vp, c.table, pos, 4)                   # and the reverse
    assert not lo.decode_attention_paged_kv8_supported(q, cos, c.kp[..., :-1], c.vp[..., :-1], c.table, pos, 4)
    wide = torch.zeros((P, 2, PAGE * 64), dtype=torch.uint8, device=DEV)                                  # no scale bytes
    assert not lo.decode_attention_paged_kv8_supported(q, cos, wide, wide, c.table, pos, 4)
    assert not lo.decode_attention_paged_kv8_supported(q, cos, c.kp.view(torch.int8), c.vp.view(torch.int8), c.table, pos, 4)
    assert not lo.decode_attention_paged_kv8_supported(q.float(), cos.float(), c.kp, c.vp, c.table, pos, 4)
    assert not lo.decode_attention_paged_kv8_supported(q.bfloat16(), cos, c.kp, c.vp, c.table, pos, 4)    # cos differs from q
    d96 = torch.zeros((P, 2, PAGE * 97), dtype=torch.uint8, device=DEV)
    assert not lo.decode_attention_paged_kv8_supported(q, cos, d96, d96, c.table, pos, 4)
    assert not lo.prefill_attention_paged_kv8_supported(q, cos, d96, d96, c.table, pos, pos, 4)
    assert not lo.decode_attention_verify_paged_kv8_supported(q, cos, c.kp, c.vp, c.table, pos, 4)        # T = 1
    with pytest.raises(ValueError):
        lo.decode_attention_paged_kv8(q, k, v, cos, sin, k16, v16, c.table, pos, 4, 0.125)
    with pytest.raises(ValueError):
        lo.prefill_attention_paged_kv8(q, k, v, cos, sin, c.kp, c.vp, c.table, pos, pos.int(), 4, 0.125)
    with pytest.raises(ValueError):
        lo.decode_attention_verify_paged_kv8(q, k, v, cos, sin, c.kp, c.vp, c.table, pos, 4, 0.125)
