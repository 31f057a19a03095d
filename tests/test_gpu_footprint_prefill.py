"""GPU: the memory footprint of qz_prefill_attention through tests/footprint.py, in the manner of
test_gpu_footprint_verify.py: every operand between poisoned guard bands, row strides above the row
length with poison in the tails, the output of exactly the documented size between sentinels, inputs
bit-identical afterwards, every output the bits of the same call on plain packed buffers, and no cache
byte outside slots [pos[b], pos[b] + len[b]) changed.  The launch has no workspace."""
import math

import pytest
import torch

import footprint as fp
from prefill_reference import TK, TQ
from test_gpu_footprint import BF16, DT_IDS, F16, I64, Case, L, P, S, _randn

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Lc,T", [(TK, 2), (TK + 2, TQ - 1), (3 * TK + 5, TQ + 1)])
def test_prefill_attention_fused_rows(dt, D, Lc, T):
    """q, k and v are views of one fused projection row buffer (row stride (Hq + 2 Hkv) D); cos / sin and
    out have row strides above their widths; pos and len lie inside guards of an out-of-range value.  The
    cache rows at and above pos[b] are NaN before the call; only slots pos[b] .. pos[b] + len[b] - 1 of
    each (b, head) may change, and all of them do."""
    lib, dtc = L().lib, L().dtype_code(dt)
    Hq, Hkv = 8, 2
    width, scale = (Hq + 2 * Hkv) * D, 1.0 / math.sqrt(D)
    for B in (1, 3):
        ps = [max(Lc - T, 0), 0, min(TK - 1, Lc - 1)][:B]
        ns = [min(T, Lc - ps[0]), max(T - 1, 1), 0][:B]
        R = B * T
        f = _randn((R, width), dt, Lc + D + B)
        ang = torch.rand(R, D // 2, generator=torch.Generator().manual_seed(B)) * 6.0
        cos, sin = torch.cat((ang.cos(), ang.cos()), -1).to(dt), torch.cat((ang.sin(), ang.sin()), -1).to(dt)
        kc, vc = _randn((B, Hkv, Lc, D), dt, 1), _randn((B, Hkv, Lc, D), dt, 2)
        for b, p in enumerate(ps):
            kc[b, :, p:] = float("nan")
            vc[b, :, p:] = float("nan")
        c = (Case().inp("f", f).inp("cos", cos, row_stride=D + 8).inp("sin", sin, row_stride=D + 8)
             .inout("kc", kc).inout("vc", vc).out("out", (R, Hq * D), dt, row_stride=Hq * D + 8)
             .inp("pos", torch.tensor(ps, dtype=I64), fill=Lc + 5).inp("len", torch.tensor(ns, dtype=I64), fill=T + 3))
        es = f.element_size()

        def call(b):
            return lib.qz_prefill_attention(
                dtc, B, T, Hq, Hkv, D, Lc, P(b.f), width, P(b.f) + Hq * D * es, width, P(b.f) + (Hq + Hkv) * D * es, width,
                P(b.cos), P(b.sin), b.cos.stride(0), P(b.kc), P(b.vc), P(b.pos), P(b["len"]), P(b.out), b.out.stride(0),
                scale, S())

        g = c.run(call)
        assert g.cos.stride(0) == D + 8 and g.out.stride(0) == Hq * D + 8
        out = g.out.view(B, T, Hq * D)
        for b, n in enumerate(ns):
            assert not torch.isnan(out[b, :n]).any() and bool((out[b, n:] == 0).all())
        for name in ("kc", "vc"):
            ch = fp.changed_payload(g[name]).clone()
            for b, (p, n) in enumerate(zip(ps, ns)):
                assert bool(ch[b, :, p:p + n].all()), f"{name}: a window slot kept its NaN"
                ch[b, :, p:p + n] = False
            assert not bool(ch.any()), f"{name}: a row outside the window changed: {torch.nonzero(ch)[:4].tolist()}"
