"""CPU: qa.TokenAutomaton's constructors against tests/constraint_reference.py's dense tables, the allow
bits, the rejections, and layer_ops' composed routes on CPU fp32 logits against the reference."""
import numpy as np
import pytest
import torch

import constraint_reference as R
import quantizations_amd as qa
from quantizations_amd import constraints as C
from quantizations_amd import layer_ops as ops


def dense(a):
    return R.dense_of(a.class_of, a.next)


def check_allow(a):
    S, Cn = a.next.shape
    assert a.class_of.dtype == np.int16 and a.next.dtype == np.int32 and a.allow.dtype == np.int32
    assert a.allow.shape == (S, (Cn + 31) // 32)
    words = a.allow.view(np.uint32)
    c = np.arange(Cn)
    bits = (words[:, c >> 5] >> (c & 31).astype(np.uint32)) & 1
    assert np.array_equal(bits.astype(bool), a.next >= 0)
    # nothing set above C
    pad = np.arange(Cn, a.allow.shape[1] * 32)
    assert not ((words[:, pad >> 5] >> (pad & 31).astype(np.uint32)) & 1).any()


def random_dense(S, V, ncols, seed, p_refuse=0.5):
    """[S, V] with exactly ncols distinct columns; token 0's column allows a way out of every state."""
    rng = np.random.default_rng(seed)
    out = tuple(range(S - 1, -1, -1))
    cols = {out}
    while len(cols) < ncols:
        col = rng.integers(0, S, S)
        col[rng.random(S) < p_refuse] = -1
        cols.add(tuple(col.tolist()))
    cols = np.array([out] + sorted(cols - {out})).T         # [S, ncols]
    pick = np.concatenate((np.arange(1, ncols), rng.integers(0, ncols, V - ncols)))
    return cols[:, np.concatenate(([0], rng.permutation(pick)))]


def test_exported():
    assert qa.TokenAutomaton is C.TokenAutomaton


@pytest.mark.parametrize("ncols", [1, 32, 33, 300])
def test_from_dense_reproduces_the_table_and_the_allow_bits(ncols):
    S, V = (4, 64) if ncols == 1 else (12, 700)
    full = random_dense(S, V, ncols, ncols)
    a = qa.TokenAutomaton.from_dense(full)
    assert np.array_equal(dense(a), np.where(full < 0, -1, full))
    assert a.C == ncols == len({tuple(col) for col in full.T.tolist()})
    assert (a.V, a.S) == (V, S)
    if ncols == 300:
        assert a.C > 255
    check_allow(a)
    for s in range(S):
        assert np.array_equal(a.allowed(s), full[s] >= 0)
        assert a.step(s, 5) == max(int(full[s, 5]), -1)
    assert a.step(S, 0) == -1 and a.step(0, V) == -1 and a.step(-1, 0) == -1


def test_from_edges():
    edges = [(0, 3, 1), (0, 4, 1), (1, 5, 2), (2, 0, 0), (2, 9, 2), (1, 3, 0)]
    a = qa.TokenAutomaton.from_edges(3, 10, edges)
    assert np.array_equal(dense(a), R.dense_from_edges(3, 10, edges))
    check_allow(a)
    assert a.C == 6      # 3, 4, 5, 0 and 9 each have a column of their own; the other five tokens share the refused one
    with pytest.raises(ValueError):
        qa.TokenAutomaton.from_edges(3, 10, [(0, 10, 1)])


def test_from_choices_shared_prefixes_and_a_prefix_choice():
    V, eos = 50, 49
    choices = [[5, 6, 7], [5, 6, 8], [5, 9], [5, 6], [11]]      # [5, 6] is a prefix of two others
    a = qa.TokenAutomaton.from_choices(choices, eos, V)
    assert np.array_equal(dense(a), R.dense_from_choices(choices, eos, V))
    check_allow(a)
    assert sorted(np.flatnonzero(a.allowed(0)).tolist()) == [5, 11]
    s = a.step(a.step(0, 5), 6)
    assert sorted(np.flatnonzero(a.allowed(s)).tolist()) == [7, 8, eos]
    for c in choices:
        s = 0
        for t in c:
            s = a.step(s, t)
            assert s >= 0
        term = a.step(s, eos)
        assert term == a.S - 1 and np.flatnonzero(a.allowed(term)).tolist() == [eos] and a.step(term, eos) == term
    assert a.step(a.step(0, 11), 5) == -1
    for bad in ([], [[]], [[eos]], [[V]]):
        with pytest.raises(ValueError):
            qa.TokenAutomaton.from_choices(bad, eos, V)


def digits_dfa():
    """[0-9]+ : state 0 = start, state 1 = one or more digits (accepting)."""
    trans = np.full((2, 256), -1, dtype=np.int32)
    trans[:, ord("0"):ord("9") + 1] = 1
    return trans, np.array([False, True])


def digits_vocab():
    vocab = [bytes([ord("0") + d]) for d in range(10)]                      # 0..9
    vocab += [b"12", b"007", b"3a", b"a3", b"a", b" ", b"", b"", b"99999", b"1 "]   # 10..19
    vocab += [bytes([ord("a") + k]) for k in range(19)]                     # 20..38
    vocab += [b"<eos>"]                                                     # 39
    assert len(vocab) == 40
    return vocab


def test_from_byte_dfa_digits():
    trans, acc = digits_dfa()
    vocab, eos = digits_vocab(), 39
    a = qa.TokenAutomaton.from_byte_dfa(vocab, trans, acc, eos)
    assert np.array_equal(dense(a), R.dense_from_byte_dfa(vocab, trans, acc, eos))
    check_allow(a)
    digits = list(range(10)) + [10, 11, 18]       # multi-byte tokens of digits only
    assert sorted(np.flatnonzero(a.allowed(0)).tolist()) == sorted(digits)           # no eos before a digit
    assert sorted(np.flatnonzero(a.allowed(1)).tolist()) == sorted(digits + [eos])
    # "3a" and "1 " leave the language after an accepted byte: refused; the empty entries are refused
    for t in (12, 13, 14, 15, 16, 17, 19):
        assert a.step(0, t) == -1 and a.step(1, t) == -1
    assert a.step(1, eos) == 2 and np.flatnonzero(a.allowed(2)).tolist() == [eos]
    assert a.C == 3       # digit strings, eos, everything else


def test_concat_behaves_as_each_alone():
    V, eos = 40, 39
    trans, acc = digits_dfa()
    parts = [qa.TokenAutomaton.from_choices([[1, 2], [1, 3, 4]], eos, V),
             qa.TokenAutomaton.from_byte_dfa(digits_vocab(), trans, acc, eos),
             qa.TokenAutomaton.from_choices([[7]], eos, V)]
    joint, starts = qa.TokenAutomaton.concat(parts)
    assert starts == [0, parts[0].S, parts[0].S + parts[1].S] and joint.S == sum(p.S for p in parts)
    check_allow(joint)
    d = dense(joint)
    for p, o in zip(parts, starts):
        want = dense(p)
        assert np.array_equal(d[o:o + p.S], np.where(want >= 0, want + o, -1))
    with pytest.raises(ValueError):
        qa.TokenAutomaton.concat([parts[0], qa.TokenAutomaton.from_choices([[1]], 3, 8)])


def test_rejections():
    with pytest.raises(ValueError, match="allows no token"):
        qa.TokenAutomaton.from_edges(3, 10, [(0, 1, 1), (1, 2, 2)])          # state 2 is a dead end
    qa.TokenAutomaton.from_edges(3, 10, [(0, 1, 1), (1, 2, 1)])              # state 2 unreachable: fine
    # 32768 distinct columns: the bits of the column index over 16 states (state 15 always allowed)
    v = np.arange(32768)
    full = np.where((v[None, :] >> np.arange(15)[:, None]) & 1, 0, -1)
    full = np.vstack((full, np.zeros((1, 32768), dtype=full.dtype)))
    with pytest.raises(ValueError, match="32768"):
        qa.TokenAutomaton.from_dense(full)
    qa.TokenAutomaton.from_dense(full[:, :32767], starts=(15,))
    with pytest.raises(ValueError):
        C.bias_row({3: float("inf")})
    with pytest.raises(ValueError):
        C.bias_row({3: float("nan")})
    with pytest.raises(ValueError, match="twice"):
        C.bias_row([(3, 1.0), (4, 0.5), (3, 2.0)])
    with pytest.raises(ValueError):
        C.bias_row({50: 1.0}, V=50)
    assert C.bias_row({3: float("-inf"), 7: 2}) == ([3, 7], [float("-inf"), 2.0])


def _f32_bits_case(seed=0):
    """fp32 logits whose values are fp16-representable, so the reference's fp16 rounding is the identity."""
    rng = np.random.default_rng(seed)
    B, T, V = 2, 4, 77
    x = rng.standard_normal((B * T, V)).astype(np.float16)
    x[0, 3] = np.nan
    x[1, 5] = np.inf
    x[2, 6] = -np.inf
    full = random_dense(6, V, 20, 3)
    a = qa.TokenAutomaton.from_dense(full)
    state = np.array([2, 5], dtype=np.int32)
    tok = rng.integers(0, V, (B, T))
    tok[0, 1] = 0                       # token 0 is allowed everywhere: stream 0's window walks on
    return B, T, V, x, a, state, tok


def test_composed_route_on_cpu_fp32():
    B, T, V, x, a, state, tok = _f32_bits_case()
    ids = np.array([[3, 10, 76, 200, 0], [5, 6, 7, -1, 0]], dtype=np.int32)
    vals = np.array([[0.5, -3.0, 4.0, 1.0, 9.0], [2.0, -np.inf, 0.25, 1.0, 9.0]], dtype=np.float32)
    n = np.array([4, 4], dtype=np.int32)
    want = R.constrain(x.view(np.uint16), R.F16, V, T, state=state, tok=tok, class_of=a.class_of, nxt=a.next,
                       bias_ids=ids, bias_vals=vals, bias_n=n)
    logits = torch.from_numpy(x.astype(np.float32))
    assert not ops.constrain_logits_supported(logits)
    ops.constrain_logits(logits, state=torch.from_numpy(state), tok=torch.from_numpy(tok), automaton=a.to("cpu"),
                         bias_ids=torch.from_numpy(ids), bias_vals=torch.from_numpy(vals), bias_n=torch.from_numpy(n))
    got = logits.numpy()
    ref = want.view(np.float16).astype(np.float32)
    # biased values may need more than fp16: compare those in fp32 arithmetic, everything else by value
    biased = np.zeros_like(ref, dtype=bool)
    for b in range(B):
        for k in range(n[b]):
            if 0 <= ids[b, k] < V:
                biased[b * T:(b + 1) * T, ids[b, k]] = True
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    plain = ~biased & ~np.isnan(ref)
    assert np.array_equal(got[plain], ref[plain])
    x32 = x.astype(np.float32)
    for r, t in zip(*np.nonzero(biased)):
        b = r // T
        v = vals[b, list(ids[b, :n[b]]).index(t)]
        if np.isneginf(ref[r, t]):
            assert np.isneginf(got[r, t])
        elif not np.isnan(ref[r, t]):
            assert got[r, t] == np.float32(x32[r, t] + v)
    assert np.isneginf(got).sum() > np.isneginf(x32).sum()


def test_composed_mask_and_advance_on_cpu():
    rng = np.random.default_rng(5)
    B, V = 3, 45
    x = rng.standard_normal((B, V)).astype(np.float16)
    words = rng.integers(-2 ** 31, 2 ** 31, (B, 3)).astype(np.int32)       # 2 words needed, stride 3
    want = R.constrain(x.view(np.uint16), R.F16, V, mask=words)
    logits = torch.from_numpy(x.astype(np.float32))
    ops.constrain_logits(logits, mask=torch.from_numpy(words))
    assert np.array_equal(logits.numpy(), want.view(np.float16).astype(np.float32))
    with pytest.raises(ValueError, match="T must be 1"):
        ops.constrain_logits(torch.zeros(2 * B, V), mask=torch.from_numpy(words), T=2)

    a = qa.TokenAutomaton.from_choices([[1, 2, 3], [4]], 44, V)
    seq = np.zeros((4, 12), dtype=np.int64)
    seq[0, 5:8] = [1, 2, 3]
    seq[1, 5:7] = [1, 9]            # refused
    seq[2, 5] = V                   # outside the vocabulary
    seq[3, 5] = 4
    state = np.array([0, 0, 0, -1], dtype=np.int32)
    pos0 = np.array([4, 4, 4, 4])
    pos1 = np.array([7, 6, 5, 5])
    want = R.advance(state, seq, pos0, pos1, a.class_of, a.next, V)
    assert want.tolist() == [3, -2, -2, -1]
    st = torch.from_numpy(state.copy())
    ops.constraint_advance(st, torch.from_numpy(seq), torch.from_numpy(pos0), torch.from_numpy(pos1), a.to("cpu"))
    assert st.tolist() == want.tolist()
    st = torch.from_numpy(state.copy())
    ops.constraint_advance(st, torch.from_numpy(seq), torch.tensor([4]), torch.tensor([4]), a.to("cpu"))
    assert st.tolist() == state.tolist()        # nothing emitted
