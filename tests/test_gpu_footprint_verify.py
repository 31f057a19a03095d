"""GPU: the memory footprint of qz_decode_attention_verify, qz_verify_step_streams and qz_ngram_draft
through tests/footprint.py, in the manner of test_gpu_footprint.py: every operand between guard
bands, row strides above the row length with poison in the tails, workspaces of exactly the
documented size filled with 0xFF / NaN, inputs bit-identical afterwards, and every output the bits
of the same call on plain packed buffers."""
import math

import pytest
import torch

import footprint as fp
from test_gpu_footprint import BF16, DT_IDS, F16, F32, I32, I64, U8, Case, L, P, S, _randn
from verify_reference import draft_rule, verify_feedback

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Lc", [8, 128, 129, 257])
def test_attention_verify_fused_rows_exact_work(dt, D, Lc):
    """q, k and v are views of one fused projection row buffer (row stride (Hq + 2 Hkv) D); cos / sin
    and out have row strides above their widths; `work` is exactly the header's size and NaN-filled;
    pos lies inside guards of an out-of-range position.  The cache rows at and above p_b are NaN
    before the call; only slots p_b .. p_b + T - 1 of each (b, head) may change."""
    lib, dtc = L().lib, L().dtype_code(dt)
    Hq, Hkv, T = 8, 2, 4
    width, scale = (Hq + 2 * Hkv) * D, 1.0 / math.sqrt(D)
    nsplit = -(-Lc // 128)
    for B in (1, 3):
        ps = [Lc - T, 0, max(Lc - 6, 1)][:B]
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
             .inp("pos", torch.tensor(ps, dtype=I64), fill=Lc + 5))
        nwork = R * Hkv * nsplit * (Hq // Hkv) * (D + 2) if nsplit > 1 else 0
        if nwork:
            c.scratch("work", nwork, F32)
        es = f.element_size()

        def call(b):
            return lib.qz_decode_attention_verify(
                dtc, B, T, Hq, Hkv, D, Lc, P(b.f), width, P(b.f) + Hq * D * es, width, P(b.f) + (Hq + Hkv) * D * es, width,
                P(b.cos), P(b.sin), b.cos.stride(0), P(b.kc), P(b.vc), P(b.pos), P(b.out), b.out.stride(0),
                P(b.work) if nwork else 0, scale, S())

        g = c.run(call)
        assert g.cos.stride(0) == D + 8 and g.out.stride(0) == Hq * D + 8
        assert not torch.isnan(g.out).any()
        for name in ("kc", "vc"):
            ch = fp.changed_payload(g[name]).clone()
            for b, p in enumerate(ps):
                assert bool(ch[b, :, p:p + T].all()), f"{name}: a window slot kept its NaN"
                ch[b, :, p:p + T] = False
            assert not bool(ch.any()), f"{name}: a row outside the window changed: {torch.nonzero(ch)[:4].tolist()}"


HIST_LEN, HIST_ROW = 12, 15


@pytest.mark.parametrize("dt", [F16, BF16, F32], ids=DT_IDS)
def test_verify_step_padded_rows_exact_work(dt):
    """row = V + 24 with +inf in the padding of every logits row (a read of it changes a pick);
    hist_row above hist_len with sentinels in the slack; work exactly qz_greedy_step_work_bytes(B T, V),
    0xFF-filled.  Stream 1 of 3 is dead: its tok row, pos, hist row and live word keep their bits."""
    import numpy as np

    lib, dtc = L().lib, L().dtype_code(dt)
    T = 4
    for V in (1, 2047, 2048, 2049, 4097):
        for B in (1, 3):
            R = B * T
            logits = _randn((R, V), dt, V + B, 3.0)
            picks = logits.float().argmax(-1).view(B, T).numpy().astype(np.int64)
            tok0 = torch.full((B, T), -7, dtype=I64)
            tok0[:, 1:] = torch.from_numpy(picks[:, :-1])
            if V > 1:
                tok0[0, 2] = (int(picks[0, 1]) + 1) % V            # stream 0 accepts one draft
            hist0 = torch.arange(B * HIST_LEN, dtype=I64).view(B, HIST_LEN) - 100
            ps, live = [2, 1, 0][:B], [1, 0, 1][:B]
            stop, limit = torch.full((B,), -1, dtype=I64), torch.full((B,), 1000, dtype=I64)
            nwork = int(lib.qz_greedy_step_work_bytes(R, V))
            assert nwork > 0 and nwork % 16 == 0
            c = (Case().inp("logits", logits, row_stride=V + 24, fill=float("inf"))
                 .inout("hist", hist0, row_stride=HIST_ROW).inout("tok", tok0).scratch("work", nwork, U8)
                 .inout("pos", torch.tensor(ps, dtype=I64)).inout("live", torch.tensor(live, dtype=I32))
                 .inp("stop", stop, fill=-2).inp("limit", limit, fill=-3).out("accepted", (B,), I32))

            def call(b):
                return lib.qz_verify_step_streams(P(b.logits), dtc, B, T, V, b.logits.stride(0), P(b.hist), b.hist.stride(0),
                                                  HIST_LEN, P(b.pos), P(b.live), P(b.stop), P(b.limit), P(b.tok),
                                                  P(b.accepted), P(b.work), S())

            g = c.run(call)
            assert g.logits.stride(0) == V + 24 and g.hist.stride(0) == HIST_ROW
            want = verify_feedback(picks, hist0.numpy(), np.array(ps), np.array(live, dtype=np.int32), stop.numpy(),
                                   limit.numpy(), tok0.numpy())
            for name, w in zip(("hist", "pos", "live", "tok", "accepted"), want):
                assert np.array_equal(g[name].cpu().numpy(), w), (V, B, name)
            assert int(g.accepted[0]) == (2 if V > 1 else T)


def test_ngram_draft_padded_history():
    """hist_row above hist_len with an out-of-range token in the slack and the guards; tok and pos_ids
    between sentinels; hist and pos unchanged."""
    lib = L().lib
    T, H = 5, 300
    g0 = torch.Generator().manual_seed(4)
    hists = torch.randint(0, 3, (4, H), generator=g0)
    ps = [H - 1, 0, 7, 256]
    tok0 = torch.full((4, T), -7, dtype=I64)
    tok0[:, 0] = torch.tensor([int(hists[b, p]) for b, p in enumerate(ps)])
    for ngram_max in (1, 4):
        c = (Case().inp("hist", hists, row_stride=H + 5, fill=-9).inp("pos", torch.tensor(ps, dtype=I64), fill=-1)
             .inout("tok", tok0).out("pos_ids", (4, T), I64))

        def call(b):
            return lib.qz_ngram_draft(4, T, ngram_max, P(b.hist), b.hist.stride(0), H, P(b.pos), P(b.tok), P(b.pos_ids), S())

        g = c.run(call)
        assert g.hist.stride(0) == H + 5
        for b, p in enumerate(ps):
            assert g.tok[b].tolist() == [int(hists[b, p])] + draft_rule(hists[b].tolist(), p, int(hists[b, p]), T, ngram_max)
            assert g.pos_ids[b].tolist() == [p + i for i in range(T)]
