"""GPU: the memory footprint of qz_logits_process through tests/footprint.py, as
test_gpu_footprint_verify_sample.py pins the sampled verify pick's: the logits between guard bands with
row > V (in and out: only tokens of the history may change), hist and tok between poisoned guards
(ids far outside the vocabulary) with hist_row above hist_len, every parameter array between
guards, a workspace of exactly qz_logits_process_work_bytes between sentinels, dirty with NaN and
with 0xFF; guards untouched, inputs bit-identical afterwards, and the logits the bits of the same call
on plain packed buffers with a zeroed workspace -- and of the reference."""
import numpy as np
import pytest
import torch

import logits_process_reference as R
from test_gpu_footprint import BF16, DT_IDS, F16, I32, I64, U8, Case, L, P, S, _randn

pytestmark = pytest.mark.gpu

NAME = {F16: R.F16, BF16: R.BF16}
FAR = 1 << 45     # a token id no logits row holds: whatever reads a guard as a token skips it


def _case(dt, B, T, V, H, hist_row, n, dirty):
    lib, dtc = L().lib, L().dtype_code(dt)
    rng = np.random.default_rng(V + H + B)
    logits = _randn((B * T, V), dt, V + B, 3.0)
    hist = torch.from_numpy(rng.integers(0, min(V, 50), (B, H)))
    pos = torch.full((B,), n - 1, dtype=I64)
    tok = torch.from_numpy(rng.integers(0, min(V, 50), (B, T)))
    tok[:, 0] = hist[:, n - 1]
    rp = torch.tensor([1.3, 0.5, 1.0][:B])
    pp = torch.tensor([0.5, -2.0, 0.0][:B])
    fp = torch.tensor([2.0, 0.5, 0.0][:B])
    ngram = torch.tensor([2, 3, 0][:B], dtype=I32)
    mn = torch.tensor([n, 0, 0][:B], dtype=I64)
    pl = torch.tensor([n // 2, 0, 0][:B], dtype=I64)
    eos = torch.tensor([V - 1, 3, 5][:B], dtype=I64)
    nwork = int(lib.qz_logits_process_work_bytes(B, T, H))
    c = (Case().inout("logits", logits, row_stride=V + 24, fill=float("inf"))
         .inp("hist", hist, row_stride=hist_row, fill=FAR).inp("tok", tok, fill=FAR).inp("pos", pos, fill=-7)
         .inp("rp", rp.float()).inp("pp", pp.float()).inp("fp", fp.float()).inp("ngram", ngram, fill=-12345)
         .inp("mn", mn, fill=FAR).inp("pl", pl, fill=-FAR).inp("eos", eos, fill=3))
    if nwork:
        c.scratch("work", nwork, U8, dirty)

    def call(b):
        return lib.qz_logits_process(P(b.logits), dtc, B, T, V, b.logits.stride(0), P(b.hist), b.hist.stride(0), H,
                                     P(b.pos), 1, P(b.tok), P(b.rp), P(b.pp), P(b.fp), P(b.ngram), P(b.mn), P(b.pl),
                                     P(b.eos), P(b.work) if nwork else 0, S())

    g = c.run(call)
    assert g.logits.stride(0) == V + 24 and g.hist.stride(0) == hist_row
    before = logits.view(torch.int16).numpy().view(np.uint16)
    want = R.process(before, NAME[dt], V, hist.numpy(), pos.numpy(), tok.numpy(), rp=rp.tolist(), pp=pp.tolist(),
                     fp=fp.tolist(), ngram=ngram.tolist(), min_new=mn.tolist(), prompt_len=pl.tolist(), eos=eos.tolist())
    got = g.logits.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, want)
    assert (got != before).any() and got[0, V - 1] == R.NEG_INF[NAME[dt]]
    if B == 3:
        assert np.array_equal(got[2 * T:], before[2 * T:])       # the neutral stream


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
def test_logits_process_padded_rows_table_in_lds(dt):
    for V in (1, 999, 2048):
        for B, T in ((1, 1), (3, 4)):
            _case(dt, B, T, V, H=40, hist_row=47, n=30, dirty="poison")


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
@pytest.mark.parametrize("dirty", ["poison", "sentinel"])
def test_logits_process_exact_dirty_workspace(dt, dirty):
    """hist_len 9000: 32768 slots per row in `work`, 0xFF-filled ("poison") or 0xA5-filled."""
    _case(dt, 3, 2, 4099, H=9000, hist_row=9003, n=8500, dirty=dirty)
