"""GPU: qz_constrain_logits and qz_constraint_advance against tests/constraint_reference.py -- bit-equal
on the whole logits buffer (the row tails hold NaN and must survive), fp16 and bf16.  The buffers hold
uniformly random 16-bit patterns (every class: +-0, subnormals, +-inf, NaNs) with a fixed list of edge
patterns planted at the row's first tokens, so allowed and refused tokens both carry all of them."""
import numpy as np
import pytest
import torch

import constraint_reference as R
from quantizations_amd import constraints as C

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
TORCH_DT = {R.F16: torch.float16, R.BF16: torch.bfloat16}
DTS = [R.F16, R.BF16]
EDGE = {R.F16: [0x0000, 0x8000, 0x0001, 0x8001, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0xFE01, 0x7D55, 0x3C00, 0xBC00],
        R.BF16: [0x0000, 0x8000, 0x0001, 0x8001, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7FA5, 0x3F80, 0xBF80]}
TAIL = {R.F16: 0x7E00, R.BF16: 0x7FC0}


def tables(V, S, ncols, seed, p_refuse=0.5):
    """A random compressed automaton (class_of, next, allow), every class used when V >= ncols; no
    reachability check: dead ends and full rows are wanted here."""
    rng = np.random.default_rng(seed)
    ncols = min(ncols, V)
    class_of = rng.permutation(np.concatenate((np.arange(ncols), rng.integers(0, ncols, V - ncols))))
    nxt = rng.integers(0, S, (S, ncols))
    nxt[rng.random((S, ncols)) < p_refuse] = -1
    a = C.TokenAutomaton(class_of, nxt, starts=())
    return a.class_of, a.next, a.allow


def _dev(a, dtype):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def run(dt, V, B, T, *, row=None, auto=None, state=None, tok=None, mask=None, bias=None, bits=None, seed=0):
    """Calls the C ABI on a [B*T, row] buffer; returns (before, after, want) as uint16, whole rows."""
    from quantizations_amd import _lib

    row = V + 24 if row is None else row
    rng = np.random.default_rng(seed)
    if bits is None:
        bits = rng.integers(0, 65536, (B * T, row)).astype(np.uint16)
        k = min(V, len(EDGE[dt]))
        for r in range(B * T):
            bits[r, :k] = np.roll(EDGE[dt], r)[:k]
    bits = np.array(bits, dtype=np.uint16)
    bits[:, V:] = TAIL[dt]
    buf = torch.from_numpy(bits.view(np.int16).copy()).to(DEV)
    d_state = _dev(state, torch.int32)
    d_tok = _dev(tok, torch.int64)
    d_auto = [None] * 3 if auto is None else [_dev(auto[0], torch.int16), _dev(auto[1], torch.int32),
                                              _dev(auto[2], torch.int32)]
    d_mask = _dev(mask, torch.int32)
    d_bias = [None] * 3 if bias is None else [_dev(bias[0], torch.int32), _dev(bias[1], torch.float32),
                                              _dev(bias[2], torch.int32)]
    S, Cn = (0, 0) if auto is None else auto[1].shape
    p = _lib.ptr
    rc = _lib.lib.qz_constrain_logits(
        buf.data_ptr(), _lib.dtype_code(TORCH_DT[dt]), B, T, V, row, p(d_state), p(d_tok), p(d_auto[0]), p(d_auto[2]),
        p(d_auto[1]), S, Cn, p(d_mask), 0 if mask is None else np.asarray(mask).shape[1], p(d_bias[0]), p(d_bias[1]),
        p(d_bias[2]), 0 if bias is None else np.asarray(bias[0]).shape[1], torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint16)
    kw = {}
    if auto is not None:
        kw.update(state=state, tok=tok, class_of=auto[0], nxt=auto[1])
    if bias is not None:
        kw.update(bias_ids=bias[0], bias_vals=bias[1], bias_n=bias[2])
    want = R.constrain(bits, dt, V, T, mask=mask, **kw)
    for t, src in ((d_state, state), (d_tok, tok), (d_mask, mask), (d_bias[0], None if bias is None else bias[0])):
        if t is not None:
            assert np.array_equal(t.cpu().numpy(), np.asarray(src)), "an input changed"
    return bits, got, want


def same(got, want, what=""):
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:6].tolist(), got[bad][:6].tolist(),
                           want[bad][:6].tolist())


def walk_drafts(auto, state, B, T, V, rng, p_follow=0.8):
    """tok [B, T]: column 0 anything, columns 1.. mostly tokens the walked state allows."""
    class_of, nxt, _ = auto
    tok = rng.integers(0, V, (B, T))
    for b in range(B):
        s = int(state[b])
        for i in range(1, T):
            if not 0 <= s < nxt.shape[0]:
                break
            ok = np.flatnonzero(nxt[s, class_of] >= 0)
            if ok.size and rng.random() < p_follow:
                tok[b, i] = rng.choice(ok)
            s = R._step(s, int(tok[b, i]), class_of, nxt, V)
    return tok


@pytest.mark.parametrize("V", [1, 7, 8, 2047, 2048, 2049, 4104])
@pytest.mark.parametrize("dt", DTS)
def test_shapes_automaton_and_bias(dt, V):
    """Row stride V + 24 (vector accesses only where it is a multiple of 8) and the next multiple of 8
    above it (vector accesses with a scalar tail where V is not)."""
    rng = np.random.default_rng(V)
    auto = tables(V, 6, 20, V)
    for B, T in ((1, 1), (3, 1), (2, 4), (1, 16)):
        state = rng.integers(0, 6, B)
        tok = walk_drafts(auto, state, B, T, V, rng)
        ids = rng.permutation(max(V, 4))[:4][None, :].repeat(B, 0).astype(np.int32)      # distinct; some >= V when V < 4
        bias = (ids, rng.standard_normal((B, 4)).astype(np.float32) * 4, np.array([4, 0, 2][:B], dtype=np.int32))
        for row in sorted({V + 24, (V + 24 + 7) // 8 * 8}):
            before, got, want = run(dt, V, B, T, row=row, auto=auto, state=state, tok=tok, bias=bias, seed=V + B + T)
            same(got, want, (B, T, row))
            assert (got[:, V:] == TAIL[dt]).all()
    assert (got != before).any() or V == 1


@pytest.mark.parametrize("ncols", [1, 32, 33, 300])
@pytest.mark.parametrize("dt", DTS)
def test_states(dt, ncols):
    V, S = 700, 5
    class_of, nxt, _ = tables(V, S, ncols, ncols)
    nxt = nxt.copy()
    nxt[1] = 2                                   # state 1 allows everything
    nxt[2] = -1
    nxt[2, class_of[13]] = 0                     # state 2 allows token 13's class only
    a = C.TokenAutomaton(class_of, nxt, starts=())
    auto = (a.class_of, a.next, a.allow)
    state = np.array([-1, -2, S - 1, S, 1, 2, 0], dtype=np.int32)
    B = len(state)
    before, got, want = run(dt, V, B, 1, auto=auto, state=state, seed=ncols)
    same(got, want)
    for b in (0, 1, 3, 4):                       # negative, beyond S, allow-everything: every bit as it was
        assert np.array_equal(got[b], before[b])
    ok = class_of == class_of[13]
    assert (got[5, :V][~ok] == R.NEG_INF[dt]).all() and np.array_equal(got[5, :V][ok], before[5, :V][ok])
    # NaN and +-inf sit on allowed and on refused tokens of the masked rows
    for b in (2, 6):
        allowed = nxt[state[b], class_of] >= 0
        x = R.to_f32(before[b, :V], dt)
        if 1 < ncols:
            assert np.isnan(x[allowed]).any() and np.isnan(x[~allowed]).any()
            assert np.isinf(x).any()
        assert np.array_equal(got[b, :V][allowed], before[b, :V][allowed])
        assert (got[b, :V][~allowed] == R.NEG_INF[dt]).all()


@pytest.mark.parametrize("dt", DTS)
def test_windows(dt):
    V, S, T = 2500, 6, 4
    rng = np.random.default_rng(11)
    auto = tables(V, S, 40, 11, p_refuse=0.3)
    class_of, nxt, _ = auto
    state = np.array([0, 1, 2, 3, 4], dtype=np.int32)
    B = len(state)
    tok = walk_drafts(auto, state, B, T, V, rng, p_follow=1.0)       # every draft allowed: four states per stream
    states = R.row_states(state, tok, class_of, nxt, V, B, T)
    assert (states >= 0).all() and len(set(states[0].tolist())) > 1
    # stream 1: the draft at i = 2 is refused; stream 2: a draft of -1 at i = 1; stream 3: a draft of V at i = 3
    refused = np.flatnonzero(nxt[states[1, 1], class_of] < 0)
    tok[1, 2] = refused[0]
    tok[2, 1] = -1
    tok[3, 3] = V
    before, got, want = run(dt, V, B, T, auto=auto, state=state, tok=tok, seed=5)
    same(got, want)
    assert np.array_equal(got[T + 2:T + 4], before[T + 2:T + 4])                    # rows 2 and 3 of stream 1
    assert (got[T:T + 2] != before[T:T + 2]).any(1).all()                           # rows 0 and 1 are masked
    assert np.array_equal(got[2 * T + 1:3 * T], before[2 * T + 1:3 * T]) and (got[2 * T] != before[2 * T]).any()
    assert np.array_equal(got[3 * T + 3], before[3 * T + 3]) and (got[3 * T + 2] != before[3 * T + 2]).any()


@pytest.mark.parametrize("dt", DTS)
def test_host_mask(dt):
    from quantizations_amd import _lib, layer_ops as ops

    rng = np.random.default_rng(3)
    for V in (77, 2049, 4096):
        B, words = 3, (V + 31) // 32
        mask = rng.integers(-2 ** 31, 2 ** 31, (B, words + 2)).astype(np.int32)    # row stride above the word count,
        mask[1, :words] = -1                                                       # garbage in the tail bits
        before, got, want = run(dt, V, B, 1, mask=mask, seed=V)
        same(got, want, V)
        assert np.array_equal(got[1], before[1]) and (got[0] != before[0]).any()
        # with an automaton and a bias in the same launch
        auto = tables(V, 4, 10, V)
        bias = (np.tile(np.array([[0, V - 1, V // 2]], dtype=np.int32), (B, 1)),
                np.tile(np.array([[1.5, -2.0, -np.inf]], dtype=np.float32), (B, 1)), np.full(B, 3, dtype=np.int32))
        before, got, want = run(dt, V, B, 1, mask=mask, auto=auto, state=np.array([0, 1, -1], dtype=np.int32), bias=bias,
                                seed=V + 1)
        same(got, want, V)
    logits = torch.zeros((4, 64), dtype=TORCH_DT[dt], device=DEV)
    m = torch.full((2, 2), -1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="T must be 1"):
        ops.constrain_logits(logits, mask=m, T=2)
    rc = _lib.lib.qz_constrain_logits(logits.data_ptr(), _lib.dtype_code(TORCH_DT[dt]), 2, 2, 64, 64, 0, 0, 0, 0, 0, 0, 0,
                                      m.data_ptr(), 2, 0, 0, 0, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == -1


@pytest.mark.parametrize("dt", DTS)
def test_bias_over_every_pattern(dt):
    """A V = 65536 row holding every 16-bit pattern, one stream per bias, every token in the list."""
    V = 65536
    biases = [0.5, -3.0, 100.0, 1e-8, -np.inf]
    B = len(biases)
    rng = np.random.default_rng(1)
    bits = np.tile(np.arange(V, dtype=np.uint16), (B, 1))
    ids = np.stack([rng.permutation(V) for _ in range(B)]).astype(np.int32)
    vals = np.repeat(np.array(biases, dtype=np.float32)[:, None], V, 1)
    before, got, want = run(dt, V, B, 1, row=V, bits=bits, bias=(ids, vals, np.full(B, V, dtype=np.int32)))
    same(got, want)
    x = R.to_f32(before[0], dt)
    assert np.array_equal(got[:, np.isnan(x)], before[:, np.isnan(x)])              # a NaN keeps its bits
    assert (got[4][~np.isnan(x)] == R.NEG_INF[dt]).all()


@pytest.mark.parametrize("dt", DTS)
def test_bias_edges(dt):
    V, B, T = 4100, 3, 2
    auto = tables(V, 4, 10, 2)
    class_of, nxt, _ = auto
    state = np.array([0, 1, 2], dtype=np.int32)
    tok = walk_drafts(auto, state, B, T, V, np.random.default_rng(2), p_follow=1.0)
    masked = int([t for t in np.flatnonzero(nxt[0, class_of] < 0) if t not in (0, 2047, 2048, 4095, 4096, V - 1)][0])
    # a chunk's last element and the next one's first, the row's last, out of range twice, a masked token
    ids = np.array([[2047, 2048, V - 1, V, -5, masked, 0, 4095, 4096]] * B, dtype=np.int32)
    vals = np.array([[0.5, -3.0, 100.0, 7.0, 7.0, 100.0, 1e-8, -np.inf, 0.0]] * B, dtype=np.float32)
    n = np.array([9, 0, 3], dtype=np.int32)                                        # stream 1: bias_n = 0
    before, got, want = run(dt, V, B, T, auto=auto, state=state, tok=tok, bias=(ids, vals, n), seed=9)
    same(got, want)
    assert got[0, masked] == R.NEG_INF[dt]
    # the bias alone (no automaton): only listed tokens change, stream 1's rows keep every bit
    before, got, want = run(dt, V, B, T, bias=(ids, vals, n), seed=10)
    same(got, want)
    assert np.array_equal(got[T:2 * T], before[T:2 * T])
    changed = np.flatnonzero((got[0] != before[0]))
    assert set(changed.tolist()) <= {2047, 2048, V - 1, masked, 0, 4095, 4096} and changed.size >= 2


def test_advance():
    from quantizations_amd import _lib

    V = 50
    a = C.TokenAutomaton.from_choices([[1, 2, 3, 4], [5]], 49, V)
    class_of, nxt, _ = [t.to(DEV) for t in a.to("cpu")]
    L, row = 20, 23
    seq = np.full((7, row), -9, dtype=np.int64)
    seq[0, 6:9] = [1, 2, 3]          # three emitted columns
    seq[1, 6] = 1                    # pos0 == pos1: nothing emitted
    seq[2, 6:8] = [1, 7]             # a refused transition
    seq[3, 6] = V                    # a token outside the vocabulary
    seq[4, 6] = 5                    # state -1 stays
    seq[5, 6:8] = [5, 49]            # through the complete choice into the terminal state
    seq[6, 6] = 5                    # a state >= S
    state = np.array([0, 0, 0, 0, -1, 0, a.S], dtype=np.int32)
    pos0 = np.array([5, 5, 5, 5, 5, 5, 5])
    pos1 = np.array([8, 5, 7, 6, 6, 7, 6])
    want = R.advance(state, seq[:, :L], pos0, pos1, a.class_of, a.next, V)
    assert want.tolist() == [3, 0, -2, -2, -1, a.S - 1, -2]
    d_seq = torch.from_numpy(seq).to(DEV)
    d_state = torch.from_numpy(state.copy()).to(DEV)
    d0, d1 = torch.from_numpy(pos0).to(DEV), torch.from_numpy(pos1).to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    rc = _lib.lib.qz_constraint_advance(d_state.data_ptr(), 7, d_seq.data_ptr(), row, L, d0.data_ptr(), 1, d1.data_ptr(),
                                        1, class_of.data_ptr(), nxt.data_ptr(), V, a.S, a.C, st)
    assert rc == 0
    assert d_state.cpu().tolist() == want.tolist()
    assert np.array_equal(d_seq.cpu().numpy(), seq)
    # the shared-position form: one pos0 and one pos1 for all
    seq2 = np.tile(np.array([[0] * 6 + [1, 2] + [0] * 12]), (3, 1)).astype(np.int64)
    seq2[2, 7] = 9
    state2 = np.array([0, -1, 0], dtype=np.int32)
    want2 = R.advance(state2, seq2, [5], [7], a.class_of, a.next, V)
    assert want2.tolist() == [2, -1, -2]
    d_state2 = torch.from_numpy(state2.copy()).to(DEV)
    one0, one1 = torch.tensor([5], device=DEV), torch.tensor([7], device=DEV)
    d_seq2 = torch.from_numpy(seq2).to(DEV)
    rc = _lib.lib.qz_constraint_advance(d_state2.data_ptr(), 3, d_seq2.data_ptr(), 20, 20,
                                        one0.data_ptr(), 0, one1.data_ptr(), 0, class_of.data_ptr(), nxt.data_ptr(), V,
                                        a.S, a.C, st)
    assert rc == 0
    assert d_state2.cpu().tolist() == want2.tolist()


def test_advance_more_than_one_wave_of_columns():
    from quantizations_amd import layer_ops as ops

    V = 30
    a = C.TokenAutomaton.from_edges(3, V, [(0, 1, 1), (1, 2, 2), (2, 3, 0), (0, 29, 0)])
    L = 150
    seq = np.tile(np.array([1, 2, 3]), 50)[None, :].repeat(2, 0).astype(np.int64)
    seq[1, 100] = 7
    state = torch.zeros(2, dtype=torch.int32, device=DEV)
    ops.constraint_advance(state, torch.from_numpy(seq).to(DEV), torch.tensor([-1, -1], device=DEV),
                           torch.tensor([139, 139], device=DEV), [t.to(DEV) for t in a.to("cpu")])
    want = R.advance([0, 0], seq, [-1, -1], [139, 139], a.class_of, a.next, V)
    assert want.tolist() == [2, -2] and state.cpu().tolist() == want.tolist()
    assert L == seq.shape[1]


def test_composed_route_on_gpu_fp32():
    from quantizations_amd import layer_ops as ops

    rng = np.random.default_rng(8)
    B, T, V = 2, 4, 333
    x = rng.standard_normal((B * T, V)).astype(np.float16)
    x[0, 3], x[1, 5], x[2, 6] = np.nan, np.inf, -np.inf
    auto = tables(V, 6, 20, 8)
    state = np.array([2, 5], dtype=np.int32)
    tok = walk_drafts(auto, state, B, T, V, rng)
    ids = np.array([[3, 10, 332, 400], [5, 6, 7, -1]], dtype=np.int32)
    vals = np.array([[-np.inf, -np.inf, -np.inf, 1.0], [-np.inf, -np.inf, -np.inf, 1.0]], dtype=np.float32)
    n = np.array([4, 3], dtype=np.int32)
    # fp16-representable values and bans only: the reference's fp16 rounding is the identity on them
    want = R.constrain(x.view(np.uint16), R.F16, V, T, state=state, tok=tok, class_of=auto[0], nxt=auto[1], bias_ids=ids,
                       bias_vals=vals, bias_n=n)
    logits = torch.from_numpy(x.astype(np.float32)).to(DEV)
    assert not ops.constrain_logits_supported(logits)
    ops.constrain_logits(logits, state=_dev(state, torch.int32), tok=_dev(tok, torch.int64),
                         automaton=(_dev(auto[0], torch.int16), _dev(auto[1], torch.int32), _dev(auto[2], torch.int32)),
                         bias_ids=_dev(ids, torch.int32), bias_vals=_dev(vals, torch.float32), bias_n=_dev(n, torch.int32))
    got = logits.cpu().numpy()
    ref = want.view(np.float16).astype(np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(got[~np.isnan(ref)], ref[~np.isnan(ref)])
    # and the 16-bit kernel through layer_ops on the same case
    h = torch.from_numpy(x).to(DEV)
    ops.constrain_logits(h, state=_dev(state, torch.int32), tok=_dev(tok, torch.int64),
                         automaton=(_dev(auto[0], torch.int16), _dev(auto[1], torch.int32), _dev(auto[2], torch.int32)),
                         bias_ids=_dev(ids, torch.int32), bias_vals=_dev(vals, torch.float32), bias_n=_dev(n, torch.int32))
    assert np.array_equal(h.cpu().numpy().view(np.uint16), want)
