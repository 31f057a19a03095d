"""GPU: the memory footprint of qz_verify_sample_step_streams through tests/footprint.py, as
test_gpu_footprint_verify.py pins qz_verify_step_streams': logits between guard bands with row > V
and +inf in the row tails, hist_row and uniform_row above hist_len with sentinels in the slack, a
workspace of exactly qz_verify_sample_step_work_bytes 0xFF-filled (NaN in every float view), guards
untouched, inputs bit-identical afterwards, and every output the bits of the same call on plain packed
buffers with a zeroed workspace."""
import numpy as np
import pytest
import torch

from sampling_reference import interval, pick, sample_reference
from test_gpu_footprint import BF16, DT_IDS, F16, I32, I64, U8, Case, L, P, S, _randn
from verify_sample_reference import verify_sample_feedback

pytestmark = pytest.mark.gpu

HIST_LEN, HIST_ROW, UNI_ROW = 12, 15, 17
CFG = [(1.0, 0, 1.0), (0.8, 50, 0.9), (0.0, 0, 1.0)]      # (temperature, top_k, top_p): all V, a narrow head, greedy


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
def test_verify_sample_step_padded_rows_exact_work(dt):
    """Stream 1 of 3 is dead: its tok row, pos, hist row and live word keep their bits.  Every sampled
    row's u is the midpoint of the interval of the token the reference draws at 0.37, so no rounding
    moves a pick; stream 0 accepts one draft, stream 2 (greedy) the whole window."""
    lib, dtc = L().lib, L().dtype_code(dt)
    T = 4
    for V in (1, 2047, 2048, 2049, 4097):
        for B in (1, 3):
            R = B * T
            logits = _randn((R, V), dt, V + B, 3.0)
            z = logits.double().numpy()
            ps, live = [2, 1, 0][:B], [1, 0, 1][:B]
            cfg = [CFG[b] if V > 1 else (CFG[b][0], 0, 1.0) for b in range(B)]
            uni = torch.rand(B, HIST_LEN, generator=torch.Generator().manual_seed(V))
            picks = np.zeros((B, T), dtype=np.int64)
            for b in range(B):
                for i in range(T):
                    ref = sample_reference(z[b * T + i], *cfg[b])
                    if not ref.greedy:
                        lo, hi = interval(ref, pick(ref, 0.37))
                        uni[b, ps[b] + i] = (lo + hi) / 2
                    picks[b, i] = pick(ref, float(uni[b, ps[b] + i]))
            tok0 = torch.full((B, T), -7, dtype=I64)
            tok0[:, 1:] = torch.from_numpy(picks[:, :-1])
            if V > 1:
                tok0[0, 2] = (int(picks[0, 1]) + 1) % V            # stream 0 accepts one draft
            hist0 = torch.arange(B * HIST_LEN, dtype=I64).view(B, HIST_LEN) - 100
            stop, limit = torch.full((B,), -1, dtype=I64), torch.full((B,), 1000, dtype=I64)
            temp, topk, topp = (torch.tensor(col) for col in zip(*cfg))
            nwork = int(lib.qz_verify_sample_step_work_bytes(B, T, V))
            assert nwork == int(lib.qz_sample_step_work_bytes(R, V)) and nwork % 16 == 0
            c = (Case().inp("logits", logits, row_stride=V + 24, fill=float("inf"))
                 .inout("hist", hist0, row_stride=HIST_ROW).inout("tok", tok0).scratch("work", nwork, U8)
                 .inout("pos", torch.tensor(ps, dtype=I64)).inout("live", torch.tensor(live, dtype=I32))
                 .inp("stop", stop, fill=-2).inp("limit", limit, fill=-3).out("accepted", (B,), I32)
                 .inp("temp", temp.float()).inp("topk", topk.to(I32), fill=-12345).inp("topp", topp.float())
                 .inp("uni", uni, row_stride=UNI_ROW))

            def call(b):
                return lib.qz_verify_sample_step_streams(
                    P(b.logits), dtc, B, T, V, b.logits.stride(0), P(b.temp), P(b.topk), P(b.topp), P(b.uni),
                    b.uni.stride(0), P(b.hist), b.hist.stride(0), HIST_LEN, P(b.pos), P(b.live), P(b.stop), P(b.limit),
                    P(b.tok), P(b.accepted), P(b.work), S())

            g = c.run(call)
            assert g.logits.stride(0) == V + 24 and g.hist.stride(0) == HIST_ROW and g.uni.stride(0) == UNI_ROW
            want = verify_sample_feedback(z, temp.float().numpy(), topk.numpy(), topp.float().numpy(), uni.numpy(),
                                          hist0.numpy(), np.array(ps), np.array(live, dtype=np.int32), stop.numpy(),
                                          limit.numpy(), tok0.numpy())
            for name, w in zip(("hist", "pos", "live", "tok", "accepted"), want):
                assert np.array_equal(g[name].cpu().numpy(), w), (V, B, name, g[name].cpu().tolist(), w.tolist())
            assert int(g.accepted[0]) == (2 if V > 1 else T)
            if B == 3:
                assert g.accepted.tolist()[1:] == [0, T]
