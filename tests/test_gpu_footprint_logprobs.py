"""GPU: the memory footprint of qz_token_logprobs and qz_logprobs_streams through tests/footprint.py, as
test_gpu_footprint_logits_process.py pins the processors': the logits between poisoned guard bands with
row > V, ids / seq / pos0 / pos1 between guards, outputs of exactly R (x ntop) elements and a workspace of
exactly qz_logprobs_work_bytes between sentinels, dirty with NaN / 0xFF and with 0xA5; guards untouched,
inputs bit-identical afterwards, and the outputs the bits of the same call on plain packed buffers with a
zeroed workspace -- and the values of the reference."""
import numpy as np
import pytest
import torch

import logprobs_reference as R
from test_gpu_footprint import BF16, DT_IDS, F16, F32, I32, I64, U8, Case, L, P, S

pytestmark = pytest.mark.gpu

NAME = {F16: R.F16, BF16: R.BF16}
FAR = 1 << 45     # a token id / position no buffer holds


def _logits(dt, rows, V, seed):
    bits = R.to_bits(np.random.default_rng(seed).standard_normal((rows, V)) * 3, NAME[dt])
    return bits, torch.from_numpy(bits.view(np.int16)).view(dt)


def _plain_case(dt, Rn, V, n, dirty, pad):
    lib, dtc = L().lib, L().dtype_code(dt)
    bits, logits = _logits(dt, Rn, V, V + Rn)
    ids = torch.from_numpy(np.random.default_rng(V).integers(0, V, Rn))
    nwork = int(lib.qz_logprobs_work_bytes(Rn, V, n))
    assert nwork == Rn * ((-(-V // 2048) * (8 + 4 * n) + 15) // 16 * 16)
    c = (Case().inp("logits", logits, row_stride=V + pad).inp("ids", ids, fill=FAR)
         .out("lp", (Rn,), F32).scratch("work", nwork, U8, dirty))
    if n:
        c.out("top_id", (Rn, n), I32).out("top_lp", (Rn, n), F32)

    def call(b):
        return lib.qz_token_logprobs(P(b.logits), dtc, Rn, V, b.logits.stride(0), P(b.ids), n, P(b.lp),
                                     P(b.top_id) if n else 0, P(b.top_lp) if n else 0, P(b.work), S())

    g = c.run(call)
    assert g.logits.stride(0) == V + pad
    lp, ti, tl = R.reference(bits, NAME[dt], ids.numpy(), n)
    assert R.within(g.lp.cpu().numpy(), lp)[0]
    if n:
        assert np.array_equal(g.top_id.cpu().numpy(), ti) and R.within(g.top_lp.cpu().numpy(), tl)[0]


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
@pytest.mark.parametrize("dirty", ["poison", "sentinel"])
def test_token_logprobs_padded_rows_exact_dirty_workspace(dt, dirty):
    for V, pad in ((1, 24), (2049, 24), (2048, 8), (2 * 2048 + 37, 24)):
        for Rn, n in ((1, 0), (3, 20), (16, 5)):
            _plain_case(dt, Rn, V, n, dirty, pad)


def _streams_case(dt, n, dirty, stride0):
    lib, dtc = L().lib, L().dtype_code(dt)
    B, T, Ls, V = 3, 4, 9, 2048 + 5
    bits, logits = _logits(dt, B * T, V, 17)
    seq = torch.from_numpy(np.random.default_rng(3).integers(0, V, (B, Ls)))
    if stride0:
        pos0, pos1 = torch.tensor([2], dtype=I64), torch.tensor([4], dtype=I64)
    else:
        pos0, pos1 = torch.tensor([1, 4, 6], dtype=I64), torch.tensor([5, 4, 9], dtype=I64)   # 4 tokens, none, 2 inside L
    nwork = int(lib.qz_logprobs_work_bytes(B * T, V, n))
    tab_row = Ls + 3
    c = (Case().inp("logits", logits, row_stride=V + 24).inp("seq", seq, row_stride=Ls + 2, fill=FAR)
         .inp("pos0", pos0, fill=-FAR).inp("pos1", pos1, fill=FAR)
         .inout("lp", torch.full((B, tab_row), 7.0)).scratch("work", nwork, U8, dirty))
    if n:
        c.inout("top_id", torch.full((B, tab_row, n), -7, dtype=I32)).inout("top_lp", torch.full((B, tab_row, n), 7.0))

    def call(b):
        return lib.qz_logprobs_streams(P(b.logits), dtc, B, T, V, b.logits.stride(0), P(b.seq), b.seq.stride(0), Ls,
                                       P(b.pos0), 0 if stride0 else 1, P(b.pos1), 0 if stride0 else 1, n, P(b.lp),
                                       P(b.top_id) if n else 0, P(b.top_lp) if n else 0, tab_row, P(b.work), S())

    g = c.run(call)
    assert g.seq.stride(0) == Ls + 2
    want_lp = np.full((B, tab_row), 7.0, np.float32)
    want_ti, want_tl = np.full((B, tab_row, n), -7, np.int32), np.full((B, tab_row, n), 7.0, np.float32)
    R.streams_reference(bits, NAME[dt], seq.numpy(), pos0.numpy(), pos1.numpy(), T, n, want_lp, want_ti, want_tl)
    live = want_lp != 7.0
    assert int(live.sum()) == 6
    got = g.lp.cpu().numpy()
    assert np.array_equal(got != 7.0, live) and R.within(got[live], want_lp[live])[0]
    if n:
        assert np.array_equal(g.top_id.cpu().numpy(), want_ti)
        assert R.within(g.top_lp.cpu().numpy()[live], want_tl[live])[0]


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
@pytest.mark.parametrize("dirty", ["poison", "sentinel"])
@pytest.mark.parametrize("stride0", [False, True], ids=["per_stream", "shared_pos"])
def test_logprobs_streams_padded_tables_exact_dirty_workspace(dt, dirty, stride0):
    for n in (0, 5):
        _streams_case(dt, n, dirty, stride0)
