"""GPU: the memory footprint of qz_constrain_logits and qz_constraint_advance through
tests/footprint.py, as test_gpu_footprint_logits_process.py pins the processors': the logits between
guard bands with row > V (in and out), the host mask with a row stride above its word count, state,
tok, the automaton's three tables and the bias lists between poisoned guards; guards untouched, inputs
bit-identical afterwards, and the logits the bits of the same call on plain packed buffers -- and of
the reference.  The advance: seq with seq_row above seq_len between guards of ids far outside the
vocabulary, state in and out -- only the streams that emitted something may change."""
import numpy as np
import pytest
import torch

import constraint_reference as R
from quantizations_amd import constraints as C
from test_gpu_footprint import BF16, DT_IDS, F16, I32, I64, Case, L, P, S

pytestmark = pytest.mark.gpu

NAME = {F16: R.F16, BF16: R.BF16}
FAR = 1 << 45


def _automaton(V, states, ncols, seed):
    rng = np.random.default_rng(seed)
    ncols = min(ncols, V)
    class_of = rng.permutation(np.concatenate((np.arange(ncols), rng.integers(0, ncols, V - ncols))))
    nxt = rng.integers(0, states, (states, ncols))
    nxt[rng.random((states, ncols)) < 0.5] = -1
    return C.TokenAutomaton(class_of, nxt, starts=())


def _constrain_case(dt, B, T, V, use_mask):
    lib, dtc = L().lib, L().dtype_code(dt)
    rng = np.random.default_rng(V + B + T)
    a = _automaton(V, 5, 40, V)
    g = torch.Generator().manual_seed(V + B)
    logits = (torch.randn((B * T, V), generator=g) * 3).to(dt)
    state = torch.tensor([0, 3, -1][:B], dtype=I32)
    tok = torch.from_numpy(rng.integers(0, V, (B, T)))
    words = (V + 31) // 32
    mask = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, (B, words)).astype(np.int32))
    NB = 6
    ids = torch.from_numpy(np.stack([rng.permutation(V + 8)[:NB] for _ in range(B)]).astype(np.int32))
    vals = torch.from_numpy((rng.standard_normal((B, NB)) * 4).astype(np.float32))
    n = torch.tensor([NB, 0, 3][:B], dtype=I32)
    c = (Case().inout("logits", logits, row_stride=V + 24, fill=float("inf"))
         .inp("state", state, fill=1).inp("tok", tok, fill=FAR)
         .inp("class_of", torch.from_numpy(a.class_of), fill=-1).inp("nxt", torch.from_numpy(a.next), fill=-1)
         .inp("allow", torch.from_numpy(a.allow), fill=-1)
         .inp("ids", ids, fill=0).inp("vals", vals).inp("n", n, fill=NB))
    if use_mask:
        c.inp("mask", mask, row_stride=words + 3, fill=0)

    def call(b):
        return lib.qz_constrain_logits(P(b.logits), dtc, B, T, V, b.logits.stride(0), P(b.state), P(b.tok),
                                       P(b.class_of), P(b.allow), P(b.nxt), a.S, a.C,
                                       P(b.mask) if use_mask else 0, b.mask.stride(0) if use_mask else 0, P(b.ids),
                                       P(b.vals), P(b.n), NB, S())

    gd = c.run(call)
    assert gd.logits.stride(0) == V + 24 and (not use_mask or gd.mask.stride(0) == words + 3)
    before = logits.view(torch.int16).numpy().view(np.uint16)
    want = R.constrain(before, NAME[dt], V, T, state=state.numpy(), tok=tok.numpy(), class_of=a.class_of, nxt=a.next,
                       mask=mask.numpy() if use_mask else None, bias_ids=ids.numpy(), bias_vals=vals.numpy(),
                       bias_n=n.numpy())
    got = gd.logits.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, want)
    assert (got != before).any() or V == 1


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS)
def test_constrain_logits_padded_rows(dt):
    for V in (1, 999, 2048, 4104):
        _constrain_case(dt, 1, 1, V, use_mask=True)
        _constrain_case(dt, 3, 1, V, use_mask=True)
        _constrain_case(dt, 3, 4, V, use_mask=False)


def test_constraint_advance_writes_live_streams_only():
    lib = L().lib
    V, B, seq_len, seq_row = 50, 5, 20, 27
    a = C.TokenAutomaton.from_choices([[1, 2, 3, 4], [5]], 49, V)
    seq = torch.zeros((B, seq_len), dtype=I64)
    seq[0, 6:9] = torch.tensor([1, 2, 3])
    seq[2, 6:8] = torch.tensor([1, 7])
    seq[3, 6] = 5
    seq[4, 6] = 5
    state = torch.tensor([0, 4, 0, -1, 0], dtype=I32)
    pos0 = torch.tensor([5, 5, 5, 5, 5], dtype=I64)
    pos1 = torch.tensor([8, 5, 7, 6, 6], dtype=I64)
    c = (Case().inout("state", state, fill=3).inp("seq", seq, row_stride=seq_row, fill=FAR)
         .inp("pos0", pos0, fill=-7).inp("pos1", pos1, fill=-7)
         .inp("class_of", torch.from_numpy(a.class_of), fill=-1).inp("nxt", torch.from_numpy(a.next), fill=-1))

    def call(b):
        return lib.qz_constraint_advance(P(b.state), B, P(b.seq), b.seq.stride(0), seq_len, P(b.pos0), 1, P(b.pos1), 1,
                                         P(b.class_of), P(b.nxt), V, a.S, a.C, S())

    g = c.run(call)
    assert g.seq.stride(0) == seq_row
    want = R.advance(state.numpy(), seq.numpy(), pos0.numpy(), pos1.numpy(), a.class_of, a.next, V)
    assert want.tolist() == [3, 4, -2, -1, 5]
    assert g.state.cpu().tolist() == want.tolist()
