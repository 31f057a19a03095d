"""GPU: qz_token_logprobs / qz_logprobs_streams (csrc/logprobs.hip) through layer_ops, fp16 and bf16,
against the float64 reference of tests/logprobs_reference.py over its families: V in {1, 5 (< n), 2047,
2048, 2049, 2 * 2048 + 37} and 128256 once, R in {1, 3, 16}, n in {0, 1, 5, 20}, a row stride of V + 24
(scalar loads) and of V rounded up to 8 where V allows the 16-B loads.  Ids and order exactly; lp and
top_lp within LP_ABS + LP_REL |ref32| (twice the float32 restatement's worst error, measured in
logprobs_reference.py); non-finite results by class and position.  Then the bits: a row alone against
the same row among 15 others, the session form between guard sentinels, and T = 4 rows of a window
against four one-row calls."""
import numpy as np
import pytest
import torch

import logprobs_reference as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
NAMES = [R.F16, R.BF16]
DT = {R.F16: torch.float16, R.BF16: torch.bfloat16}


def as_logits(bits, name, pad=24):
    """The patterns as a [R, V] view with a row stride of V + pad; the padding holds +inf."""
    Rn, V = bits.shape
    inf = 0x7C00 if name == R.F16 else 0x7F80
    buf = np.full((Rn, V + pad), inf, np.uint16)
    buf[:, :V] = bits
    t = torch.from_numpy(buf.view(np.int16)).to(DEV).view(DT[name])
    return t[:, :V]


def _bits32(t):
    return t.contiguous().view(torch.int32)


def _check(name, n, src, refs, pad=24):
    from quantizations_amd.layer_ops import token_logprobs, token_logprobs_supported

    worst = 0.0
    for (label, bits, ids), ref in zip(src, refs):
        x = as_logits(bits, name, pad)
        assert token_logprobs_supported(x) and x.stride(0) == bits.shape[1] + pad
        lp, ti, tl = token_logprobs(x, torch.from_numpy(ids).to(DEV), n)
        assert ti.shape == tl.shape == (len(ids), n)
        assert np.array_equal(ti.cpu().numpy(), ref[1][:, :n]), label
        for g, r in ((lp.cpu().numpy(), ref[0]), (tl.cpu().numpy(), ref[2][:, :n])):
            ok, w = R.within(g, r)
            worst = max(worst, w)
            assert ok, (label, w)
    return worst


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n", [0, 1, 5, 20])
def test_token_logprobs_against_the_reference(name, n):
    worst = _check(name, n, R.cases(name), R.expected(name))
    print(f"{name} n={n}: largest |lp - ref32| = {worst:.3e}  (bars: abs {R.LP_ABS:.3e}, rel {R.LP_REL:.3e})")


@pytest.mark.parametrize("name", NAMES)
def test_vector_loads_give_the_same_answers(name):
    """Row strides that are multiples of 8 take the 16-B loads wherever V % 8 == 0 (V = 2048, 128256)."""
    src = [c for c in R.cases(name) if c[1].shape[1] % 8 == 0]
    refs = [r for c, r in zip(R.cases(name), R.expected(name)) if c[1].shape[1] % 8 == 0]
    assert len(src) >= 4
    _check(name, 20, src, refs, pad=8)


@pytest.mark.parametrize("name", NAMES)
def test_nonfinite_rows_by_class_and_position(name):
    _check(name, 5, R.nonfinite_cases(name), R.expected(name, True, True))
    _check(name, 0, R.nonfinite_cases(name), R.expected(name, True, True))


@pytest.mark.parametrize("name", NAMES)
def test_a_rows_bits_do_not_depend_on_the_other_rows(name):
    from quantizations_amd.layer_ops import token_logprobs

    V = 2 * R.CHUNK + 37
    rng = np.random.default_rng(5)
    bits = R.to_bits(rng.standard_normal((16, V)) * 4, name)
    ids = torch.from_numpy(rng.integers(0, V, 16)).to(DEV)
    lp, ti, tl = token_logprobs(as_logits(bits, name), ids, 20)
    for r in (0, 7, 15):
        lp1, ti1, tl1 = token_logprobs(as_logits(bits[r:r + 1], name), ids[r:r + 1], 20)
        assert torch.equal(_bits32(lp1), _bits32(lp[r:r + 1])) and torch.equal(ti1, ti[r:r + 1])
        assert torch.equal(_bits32(tl1), _bits32(tl[r:r + 1]))
    # and a shorter list is a prefix of a longer one, with the same lp
    lp5, ti5, tl5 = token_logprobs(as_logits(bits, name), ids, 5)
    assert torch.equal(_bits32(lp5), _bits32(lp)) and torch.equal(ti5, ti[:, :5]) and torch.equal(_bits32(tl5), _bits32(tl[:, :5]))


def _streams_case(name, n):
    """B = 4, T = 4, L = 9 (the tables 11 wide): stream 0 emitted 4 tokens, stream 1 one, stream 2 did not
    move, stream 3 emitted 3 of which the last lies at column L."""
    B, T, L, V = 4, 4, 9, R.CHUNK + 5
    rng = np.random.default_rng(21)
    bits = R.to_bits(rng.standard_normal((B * T, V)) * 3, name)
    seq = rng.integers(0, V, (B, L + 2)).astype(np.int64)
    pos0, pos1 = np.array([1, 4, 5, 6], np.int64), np.array([5, 5, 5, 9], np.int64)
    return B, T, L, V, bits, seq, pos0, pos1


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n", [0, 5])
def test_streams_write_between_sentinels_only_where_live(name, n):
    from quantizations_amd.layer_ops import logprobs_streams

    B, T, L, V, bits, seq, pos0, pos1 = _streams_case(name, n)
    W = L + 2
    lp_tab = torch.full((B, W), 7.0, device=DEV)
    ti_tab = torch.full((B, W, n), -7, dtype=torch.int32, device=DEV) if n else None
    tl_tab = torch.full((B, W, n), 7.0, device=DEV) if n else None
    seq_d = torch.from_numpy(seq).to(DEV)[:, :L]                       # row stride L + 2
    logprobs_streams(as_logits(bits, name), seq_d, torch.from_numpy(pos0).to(DEV), torch.from_numpy(pos1).to(DEV),
                     lp_tab, ti_tab, tl_tab, T=T)
    want_lp = np.full((B, W), 7.0, np.float32)
    want_ti, want_tl = np.full((B, W, n), -7, np.int32), np.full((B, W, n), 7.0, np.float32)
    R.streams_reference(bits, name, seq[:, :L], pos0, pos1, T, n, want_lp, want_ti, want_tl)
    live = want_lp != 7.0
    assert {(int(b), int(c)) for b, c in zip(*np.nonzero(live))} == {(0, 2), (0, 3), (0, 4), (0, 5), (1, 5), (3, 7), (3, 8)}
    got = lp_tab.cpu().numpy()
    assert np.array_equal(got != 7.0, live) and R.within(got[live], want_lp[live])[0]
    if n:
        assert np.array_equal(ti_tab.cpu().numpy(), want_ti)
        gtl = tl_tab.cpu().numpy()
        assert np.array_equal(gtl != 7.0, want_tl != 7.0) and R.within(gtl[live], want_tl[live])[0]


@pytest.mark.parametrize("name", NAMES)
def test_a_window_of_four_rows_carries_the_bits_of_four_calls(name):
    from quantizations_amd.layer_ops import logprobs_streams, token_logprobs

    B, T, L, V, bits, seq, _, _ = _streams_case(name, 20)
    n = 20
    pos0 = torch.tensor([1, 0, 3, 4], device=DEV)
    pos1 = pos0 + T
    lp_tab = torch.full((B, L), float("nan"), device=DEV)
    ti_tab = torch.full((B, L, n), -1, dtype=torch.int32, device=DEV)
    tl_tab = torch.full((B, L, n), float("nan"), device=DEV)
    x = as_logits(bits, name)
    seq_d = torch.from_numpy(seq[:, :L].copy()).to(DEV)
    logprobs_streams(x, seq_d, pos0, pos1, lp_tab, ti_tab, tl_tab, T=T)
    cols = pos0[:, None] + 1 + torch.arange(T, device=DEV)[None, :]   # all below L
    assert int(cols.max()) < L
    for i in range(T):
        rows = torch.arange(B, device=DEV) * T + i
        ids = seq_d[torch.arange(B, device=DEV), cols[:, i]].contiguous()
        lp, ti, tl = token_logprobs(x[rows], ids, n)                    # another R, other row indices, packed rows
        b = torch.arange(B, device=DEV)
        assert torch.equal(_bits32(lp), _bits32(lp_tab[b, cols[:, i]]))
        assert torch.equal(ti, ti_tab[b, cols[:, i]]) and torch.equal(_bits32(tl), _bits32(tl_tab[b, cols[:, i]]))
    # one shared position (stride 0), as DecodeSession passes it
    lp2 = torch.full((B, L), float("nan"), device=DEV)
    logprobs_streams(x[::T], seq_d, torch.tensor([3], device=DEV), torch.tensor([4], device=DEV), lp2)
    assert torch.equal(torch.isnan(lp2).cpu(), torch.arange(L)[None, :].expand(B, L) != 4)
    want = token_logprobs(x[::T], seq_d[:, 4].contiguous(), 0)[0]
    assert torch.equal(_bits32(lp2[:, 4]), _bits32(want))


def test_captured_in_a_graph_the_call_follows_the_streams():
    from quantizations_amd.layer_ops import logprobs_streams, token_logprobs

    name = R.F16
    B, T, L, V, bits, seq, _, _ = _streams_case(name, 3)
    n = 3
    x = as_logits(bits, name)[::T]
    seq_d = torch.from_numpy(seq[:, :L].copy()).to(DEV)
    pos0, pos1 = torch.zeros(B, dtype=torch.int64, device=DEV), torch.ones(B, dtype=torch.int64, device=DEV)
    lp_tab = torch.full((B, L), float("nan"), device=DEV)
    ti_tab = torch.full((B, L, n), -1, dtype=torch.int32, device=DEV)
    tl_tab = torch.full((B, L, n), float("nan"), device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        logprobs_streams(x, seq_d, pos0, pos1, lp_tab, ti_tab, tl_tab)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        logprobs_streams(x, seq_d, pos0, pos1, lp_tab, ti_tab, tl_tab)
    lp_tab.fill_(float("nan"))
    pos0.copy_(torch.tensor([2, 3, 4, 5]))
    pos1.copy_(torch.tensor([3, 4, 4, 6]))                             # stream 2 did not move
    g.replay()
    torch.cuda.synchronize()
    filled = ~torch.isnan(lp_tab).cpu()
    want = torch.zeros((B, L), dtype=torch.bool)
    want[0, 3] = want[1, 4] = want[3, 6] = True
    assert torch.equal(filled, want)
    ref = token_logprobs(x, seq_d[torch.arange(B), torch.tensor([3, 4, 5, 6])].contiguous(), 0)[0]
    assert torch.equal(_bits32(lp_tab[0, 3]), _bits32(ref[0])) and torch.equal(_bits32(lp_tab[3, 6]), _bits32(ref[3]))
