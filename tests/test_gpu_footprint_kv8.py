"""GPU: the memory footprint of qz_decode_attention_paged_kv8, qz_decode_attention_verify_paged_kv8 and
qz_prefill_attention_paged_kv8 through the C ABI with the harness of test_gpu_footprint_paged.py: q, k
and v views of one fused projection buffer, cos / sin / out with row strides above their widths, the
table with table_row > NP whose tail entries and guards name the all-NaN page, pos / len inside guards
of an out-of-range value, the byte pools between guard bands, `work` of exactly the documented size and
NaN-filled, inputs bit-identical afterwards, every output the bits of the same call on plain packed
buffers, and no pool byte outside the written slots changed.  The slots a call is to write hold codes
0x7F and scale 255 before it: a finite row changes every one of those bytes."""
import math

import pytest
import torch

import footprint as fp
import kv8_reference as k8
from test_gpu_footprint import BF16, DT_IDS, F16, F32, I32, I64, Case, L, P, S, _randn

pytestmark = pytest.mark.gpu

B, NP, NPAGES, NAN_PAGE, PAGE = 3, 3, 10, 9, 128
PAGES = [[4, 0, 7], [2, 8, 5], [6, 1, 3]]          # scrambled, nothing shared: every stream writes
Hq, Hkv = 8, 2


def _case(dt, D, T, last_pos, seed, written):
    """The operands the three calls share; table entries above a stream's needed range name the NaN page,
    and the slots the call is to write ({b: positions}) are NaN before it."""
    width = (Hq + 2 * Hkv) * D
    R = B * T
    f = _randn((R, width), dt, seed)
    ang = torch.rand(R, D // 2, generator=torch.Generator().manual_seed(seed)) * 6.0
    cos, sin = torch.cat((ang.cos(), ang.cos()), -1).to(dt), torch.cat((ang.sin(), ang.sin()), -1).to(dt)
    kp, vp = _randn((NPAGES, Hkv, PAGE, D), dt, seed + 1).cpu(), _randn((NPAGES, Hkv, PAGE, D), dt, seed + 2).cpu()
    kp[NAN_PAGE] = float("nan")
    vp[NAN_PAGE] = float("nan")
    table = torch.full((B, NP), NAN_PAGE, dtype=I32)
    for b, lp in enumerate(last_pos):
        n = min(lp >> 7, NP - 1) + 1
        table[b, :n] = torch.tensor(PAGES[b][:n], dtype=I32)
    for b, slots in written.items():
        for j in slots:
            kp[int(table[b, j >> 7]), :, j & 127] = float("nan")
            vp[int(table[b, j >> 7]), :, j & 127] = float("nan")
    kp, vp = k8.quantize_pool(kp), k8.quantize_pool(vp)          # uint8 [NPAGES, Hkv, 128 (D + 1)]
    assert fp.guard_bytes(PAGE * (D + 1), 1) >= Hkv * PAGE * (D + 1)
    c = (Case().inp("f", f).inp("cos", cos, row_stride=D + 8).inp("sin", sin, row_stride=D + 8)
         .inout("kp", kp).inout("vp", vp).out("out", (R, Hq * D), dt, row_stride=Hq * D + 8)
         .inp("table", table, row_stride=NP + 5, fill=NAN_PAGE))
    return c, width, table


def _only_slots_changed(g, table, written, D):
    for name in ("kp", "vp"):
        codes, scales = (t.clone() for t in k8.unpack_pool(fp.changed_payload(g[name]).cpu(), D))
        for b, slots in written.items():
            for j in slots:
                page = int(table[b, j >> 7])
                assert bool(codes[page, :, j & 127].all()) and bool(scales[page, :, j & 127].all()), \
                    f"{name}: slot {j} of stream {b} was not written"
                codes[page, :, j & 127] = False
                scales[page, :, j & 127] = False
        assert not bool(codes.any()), f"{name}: a code outside the window changed: {torch.nonzero(codes)[:4].tolist()}"
        assert not bool(scales.any()), f"{name}: a scale outside the window changed: {torch.nonzero(scales)[:4].tolist()}"


def _work(c, rows, D):
    n = rows * Hkv * NP * (Hq // Hkv) * (D + 2)
    c.scratch("work", n, F32)


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
@pytest.mark.parametrize("D", [64, 128])
def test_decode_kv8_fused_rows_exact_work(dt, D):
    lib, dtc = L().lib, L().dtype_code(dt)
    ps = [383, 0, 128]
    written = {b: [p] for b, p in enumerate(ps)}
    c, width, table = _case(dt, D, 1, ps, 11 + D, written)
    c.inp("pos", torch.tensor(ps, dtype=I64), fill=NP * PAGE + 5)
    _work(c, B, D)
    es, scale = 2, 1.0 / math.sqrt(D)

    def call(b):
        return lib.qz_decode_attention_paged_kv8(
            dtc, B, Hq, Hkv, D, NP, NPAGES, P(b.f), width, P(b.f) + Hq * D * es, width, P(b.f) + (Hq + Hkv) * D * es, width,
            P(b.cos), P(b.sin), b.cos.stride(0), P(b.kp), P(b.vp), P(b.table), b.table.stride(0), P(b.pos), P(b.out),
            b.out.stride(0), P(b.work), scale, S())

    g = c.run(call)
    assert g.table.stride(0) == NP + 5 and g.out.stride(0) == Hq * D + 8
    assert not torch.isnan(g.out).any()
    _only_slots_changed(g, table, written, D)


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
@pytest.mark.parametrize("D", [64, 128])
def test_verify_kv8_fused_rows_exact_work(dt, D):
    lib, dtc = L().lib, L().dtype_code(dt)
    T, ps = 4, [380, 0, 126]
    written = {b: list(range(p, p + T)) for b, p in enumerate(ps)}
    c, width, table = _case(dt, D, T, [p + T - 1 for p in ps], 21 + D, written)
    c.inp("pos", torch.tensor(ps, dtype=I64), fill=NP * PAGE + 5)
    _work(c, B * T, D)
    es, scale = 2, 1.0 / math.sqrt(D)

    def call(b):
        return lib.qz_decode_attention_verify_paged_kv8(
            dtc, B, T, Hq, Hkv, D, NP, NPAGES, P(b.f), width, P(b.f) + Hq * D * es, width, P(b.f) + (Hq + Hkv) * D * es,
            width, P(b.cos), P(b.sin), b.cos.stride(0), P(b.kp), P(b.vp), P(b.table), b.table.stride(0), P(b.pos),
            P(b.out), b.out.stride(0), P(b.work), scale, S())

    g = c.run(call)
    assert g.table.stride(0) == NP + 5 and g.cos.stride(0) == D + 8
    assert not torch.isnan(g.out).any()
    _only_slots_changed(g, table, written, D)


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
@pytest.mark.parametrize("D", [64, 128])
def test_prefill_kv8_fused_rows(dt, D):
    lib, dtc = L().lib, L().dtype_code(dt)
    T, ps, ns = 70, [100, 300, 0], [70, 0, 33]
    written = {b: list(range(p, p + n)) for b, (p, n) in enumerate(zip(ps, ns))}
    c, width, table = _case(dt, D, T, [169, 300, 32], 31 + D, written)
    c.inp("pos", torch.tensor(ps, dtype=I64), fill=NP * PAGE + 5).inp("len", torch.tensor(ns, dtype=I64), fill=T + 3)
    es, scale = 2, 1.0 / math.sqrt(D)

    def call(b):
        return lib.qz_prefill_attention_paged_kv8(
            dtc, B, T, Hq, Hkv, D, NP, NPAGES, P(b.f), width, P(b.f) + Hq * D * es, width, P(b.f) + (Hq + Hkv) * D * es,
            width, P(b.cos), P(b.sin), b.cos.stride(0), P(b.kp), P(b.vp), P(b.table), b.table.stride(0), P(b.pos),
            P(b["len"]), P(b.out), b.out.stride(0), scale, S())

    g = c.run(call)
    assert g.table.stride(0) == NP + 5 and g.out.stride(0) == Hq * D + 8
    out = g.out.view(B, T, Hq * D)
    for b, n in enumerate(ns):
        assert not torch.isnan(out[b, :n]).any() and bool((out[b, n:] == 0).all())
    _only_slots_changed(g, table, written, D)
