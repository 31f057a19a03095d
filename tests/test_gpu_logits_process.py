"""GPU: qz_logits_process against tests/logits_process_reference.py -- bit-equal on the whole logits
buffer (row tails included: nothing outside the first V elements of a row may change), fp16 and bf16.

Every case fills the buffer with uniformly random 16-bit patterns (every class: +-0, subnormals,
+-max, +-inf, NaNs) and then plants a fixed list of edge patterns at the tokens of the history, so the
penalised positions hold all of them.  The histories cover: all tokens distinct, one token n times, a
7-token alphabet (counts around n / 7), ids congruent modulo every power of two up to the table size
(the hash is the id's low bits: one collision chain), ids outside the vocabulary.  n crosses 256, the
workgroup's 1024 threads and the 4096 history elements a workgroup loads before its first barrier;
hist_len = 4092 and 8188 fill the 64 KiB and the 128 KiB LDS table (8192 and 16384 slots), hist_len =
8189 and 20000 put the table into `work`, pre-filled with 0xFF."""
import numpy as np
import pytest
import torch

import logits_process_reference as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
TORCH_DT = {R.F16: torch.float16, R.BF16: torch.bfloat16}
EDGE = {R.F16: [0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0xFE01, 0x7D55,
                0x3C00, 0xBC00, 0x4248, 0xC248, 0x0400, 0x8400],
        R.BF16: [0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x807F, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7FA5,
                 0x3F80, 0xBF80, 0x4049, 0xC049, 0x0080, 0x8080]}
DTS = [R.F16, R.BF16]


def _dev(a, dtype):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def run(dt, V, row, hist, pos, tok=None, *, seed=0, work_fill=None, plant=True, **par):
    """Calls the C ABI on a [B*T, row] buffer of random patterns; returns (before, after, want) as uint16."""
    from quantizations_amd import _lib

    hist = np.asarray(hist, dtype=np.int64)
    B, H = hist.shape
    T = 1 if tok is None else np.asarray(tok).reshape(B, -1).shape[1]
    pos = np.asarray(pos, dtype=np.int64).reshape(-1)
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 65536, (B * T, row)).astype(np.uint16)
    if plant:
        edge = EDGE[dt]
        for b in range(B):
            ids = np.unique(hist[b][(hist[b] >= 0) & (hist[b] < V)])
            for i in range(T):
                bits[b * T + i, ids] = np.resize(np.roll(edge, b + i), ids.size)
    buf = torch.from_numpy(bits.view(np.int16).copy()).to(DEV)
    d_hist, d_pos = _dev(hist, torch.int64), _dev(pos, torch.int64)
    d_tok = _dev(np.asarray(tok).reshape(B, T), torch.int64) if tok is not None else None
    kinds = dict(rp=torch.float32, pp=torch.float32, fp=torch.float32, ngram=torch.int32, min_new=torch.int64,
                 prompt_len=torch.int64, eos=torch.int64)
    d = {k: _dev(par.get(k), kinds[k]) for k in kinds}
    nwork = int(_lib.lib.qz_logits_process_work_bytes(B, T, H))
    work = torch.full((max(nwork, 8),), 0xFF if work_fill is None else work_fill, dtype=torch.uint8, device=DEV)
    p = _lib.ptr
    rc = _lib.lib.qz_logits_process(
        buf.data_ptr(), _lib.dtype_code(TORCH_DT[dt]), B, T, V, row, d_hist.data_ptr(), H, H, d_pos.data_ptr(),
        0 if pos.size == 1 and B > 1 else 1, p(d_tok), p(d["rp"]), p(d["pp"]), p(d["fp"]), p(d["ngram"]),
        p(d["min_new"]), p(d["prompt_len"]), p(d["eos"]), work.data_ptr() if nwork else 0,
        torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint16)
    want = R.process(bits, dt, V, hist, pos, tok, **{k: par.get(k) for k in kinds})
    for name, t, src in (("hist", d_hist, hist), ("pos", d_pos, pos)):
        assert np.array_equal(t.cpu().numpy(), src), name
    return bits, got, want


def same(got, want, what=""):
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:6].tolist(), got[bad][:6].tolist(),
                           want[bad][:6].tolist())


def contents(n, V, H, seed):
    """Three streams of n tokens: all distinct, one token n times, a 7-token alphabet."""
    rng = np.random.default_rng(seed)
    hist = rng.integers(0, V, (3, H))
    hist[0, :n] = np.resize(rng.permutation(V), n)          # all distinct while n <= V
    hist[1, :n] = 17
    hist[2, :n] = rng.integers(0, 7, n) * 131 + 5
    return hist


ALL_ON = dict(rp=[1.3, 0.5, 1e4], pp=[2.0, -2.0, 0.5], fp=[0.5, 2.0, -2.0], ngram=[2, 3, 1], min_new=[5, 0, 10 ** 6],
              eos=[3, 4, 999])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 600, 1023, 1024, 1025, 4097])
def test_history_lengths_and_contents(dt, n):
    V, row, H = 1000, 1016, max(640, n + 40)
    hist = contents(n, V, H, n)
    for T in (1, 4):
        tok = None
        if T > 1:
            tok = np.random.default_rng(n + T).integers(0, 7, (3, T)) * 131 + 5
            tok[:, 0] = hist[:, n - 1]
        bits, got, want = run(dt, V, row, hist, [n - 1] * 3, tok, seed=n, prompt_len=[0, n // 2, n], **ALL_ON)
        same(got, want, (dt, n, T))
        assert (got != bits).any()
    # B = 1, and one shared position for three streams (pos_stride 0)
    one = {k: v[2:] for k, v in ALL_ON.items()}
    _, got, want = run(dt, V, row, hist[2:], [n - 1], seed=n + 1, prompt_len=[n // 3], **one)
    same(got, want, (dt, n, "B=1"))
    _, got, want = run(dt, V, row, hist, np.array([n - 1]), seed=n + 2, prompt_len=[0, n // 2, n + 5], **ALL_ON)
    same(got, want, (dt, n, "pos_stride 0"))


@pytest.mark.parametrize("dt", DTS)
def test_large_vocabulary_collision_chains_and_foreign_ids(dt):
    V = 128256
    # the table of n = 40 tokens has 512 slots; hist_len 100 gives a capacity of 512: ids congruent
    # modulo 512, 1024, ... 65536 all start at one slot and walk one chain
    chain = [5 + 65536 * k for k in range(2)] + [5 + 8192 * k for k in range(1, 8)] + [5 + 512 * k for k in range(1, 12)]
    foreign = [-1, V, 2 ** 40, -2 ** 40, V + 5]
    h = (chain + foreign + chain[:7] + [6, 7, 8] + foreign)[:45]
    H = 100
    hist = np.full((2, H), 9, dtype=np.int64)
    hist[0, :len(h)] = h
    hist[1, :len(h)] = h[::-1]
    bits, got, want = run(dt, V, V, hist, [len(h) - 1] * 2, seed=5, rp=[1.3, 0.5], pp=[0.5, 2.0], fp=[2.0, -2.0],
                          ngram=[2, 1], min_new=[100, 100], prompt_len=[20, 0], eos=[V - 1, 2 ** 40])
    same(got, want, dt)
    assert got[0, V - 1] == R.NEG_INF[dt] and (got != bits).sum() >= 10


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H, n", [(4092, 4000), (8188, 8100), (8189, 6000), (20000, 17000)],
                         ids=["lds_64k", "lds_128k", "work_small", "work_20000"])
def test_both_homes_of_the_table(dt, H, n):
    from quantizations_amd import _lib

    V, T = 50000, 4
    assert (int(_lib.lib.qz_logits_process_work_bytes(2, T, H)) == 0) == (H <= 8188)
    rng = np.random.default_rng(H)
    hist = rng.integers(0, V, (2, H))
    hist[1, :n] = rng.integers(0, 7, n) * 4096 + 1          # counts around n / 7, one collision chain
    tok = rng.integers(0, 7, (2, T)) * 4096 + 1
    tok[:, 0] = hist[:, n - 1]
    for fill in (0xFF, 0x00):
        _, got, want = run(dt, V, V + 8, hist, [n - 1, n - 1], tok, seed=H, work_fill=fill, rp=[1.3, 3.0], pp=[0.5, 0.5],
                           fp=[0.5, 0.5], ngram=[3, 2], min_new=[n, 5], prompt_len=[n // 2, 100], eos=[7, 7])
        same(got, want, (dt, H, fill))


@pytest.mark.parametrize("dt", DTS)
def test_values_prompt_lengths_and_neutral_streams(dt):
    V, row, H, n = 1000, 1016, 64, 40
    rng = np.random.default_rng(3)
    for rp in (0.5, 1.3, 1e4):
        for f in (-2.0, 0.5, 2.0):
            hist = rng.integers(0, 25, (5, H)) * 39
            bits, got, want = run(dt, V, row, hist, [n - 1] * 5, seed=int(rp * 10 + f * 7 + 20), rp=[rp, rp, rp, rp, 1.0],
                                  pp=[f, -f, f, f, 0.0], fp=[-f, f, f, f, 0.0], prompt_len=[0, n // 2, n, n + 5, 0])
            same(got, want, (dt, rp, f))
            assert np.array_equal(got[4], bits[4])                       # a neutral stream keeps every bit
            nan = np.isnan(R.to_f32(bits, dt))
            assert nan[:, :V].sum() > 5 and np.array_equal(got[nan], bits[nan])
    # every array given, every value neutral; and every array NULL
    hist = rng.integers(0, 25, (3, H)) * 39
    bits, got, _ = run(dt, V, row, hist, [n - 1] * 3, rp=[1.0] * 3, pp=[0.0] * 3, fp=[0.0, -0.0, 0.0], ngram=[0, 0, -1],
                       min_new=[0, -5, 0], prompt_len=[0, 3, 50], eos=[1, 2, 3])
    assert np.array_equal(got, bits)
    bits, got, _ = run(dt, V, row, hist, [n - 1] * 3)
    assert np.array_equal(got, bits)
    # min_new_tokens without an eos array does nothing
    bits, got, _ = run(dt, V, row, hist, [n - 1] * 3, min_new=[100] * 3)
    assert np.array_equal(got, bits)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("T", [1, 4, 16])
def test_window_rows_see_their_own_drafts_only(dt, T):
    V, row, H = 1000, 1016, 40
    p = 9
    hist = np.zeros((2, H), dtype=np.int64)
    hist[0, :p + 1] = [1, 2, 3, 4, 5, 6, 7, 8, 50, 51]
    hist[1, :p + 1] = [1, 2, 3, 1, 2, 4, 9, 9, 9, 1]            # the bigram (1, 2) straddles hist and draft 1
    tok = np.zeros((2, T), dtype=np.int64)
    tok[0] = [51] + [100 + i for i in range(1, T)]              # draft i occurs nowhere else
    tok[1] = ([1, 2, 3, 1, 2, 4] * 3)[:T]
    par = dict(rp=[1.3, 1.0], pp=[0.5, 0.0], fp=[0.5, 0.0], ngram=[0, 3], prompt_len=[p + 1, 0])
    bits, got, want = run(dt, V, row, hist, [p, p], tok if T > 1 else None, seed=T, plant=False, **par)
    same(got, want, (dt, T))
    for i in range(T):
        for j in range(1, T):
            touched = got[i, 100 + j] != bits[i, 100 + j]
            finite = bool(np.isfinite(R.to_f32(bits[i, 100 + j], dt)))
            if j <= i and finite:
                assert touched, (i, j)                           # presence 0.5 moves every finite value
            if j > i:
                assert not touched, (i, j)                       # row i never sees draft i + 1
    if T >= 4:
        # stream 1, row 1: h = ..., 1 | 2 -> the trigram (1, 2, 3) and (1, 2, 4) ban 3 and 4
        r = T + 1
        assert got[r, 3] == R.NEG_INF[dt] and got[r, 4] == R.NEG_INF[dt]


@pytest.mark.parametrize("dt", DTS)
def test_no_repeat_ngram_sizes(dt):
    V, row, H = 1000, 1016, 700
    for n in (7, 300, 600):
        period = [11, 12, 13, 14, 15]
        h = (period * (n // 5 + 1))[:n]
        hist = np.zeros((6, H), dtype=np.int64)
        hist[:, :n] = h
        gs = [1, 2, 3, n, n + 1, n + 2]
        bits, got, want = run(dt, V, row, hist, [n - 1] * 6, seed=n, rp=[1.3] * 6, pp=[0.5] * 6, fp=[0.5] * 6, ngram=gs,
                              prompt_len=[0] * 6)
        same(got, want, (dt, n))
        nxt = period[n % 5]
        assert got[1, nxt] == R.NEG_INF[dt] and got[2, nxt] == R.NEG_INF[dt]       # banned and penalised: -inf
        assert all(got[0, t] == R.NEG_INF[dt] for t in period[:min(n, 5)])         # g = 1 bans every token seen
        # g > n bans nothing; g = n has the one candidate k = 0, a match iff the history has period 1
        for b in (3, 4, 5):
            assert np.array_equal(got[b], R.process_row(bits[b], dt, V, h, rp=1.3, pp=0.5, fp=0.5)), b
    hist = np.full((1, H), 21, dtype=np.int64)
    _, got, want = run(dt, V, row, hist, [9], ngram=[10])
    same(got, want)
    assert got[0, 21] == R.NEG_INF[dt]


@pytest.mark.parametrize("dt", DTS)
def test_min_length_and_positions_out_of_range(dt):
    V, row, H, n, m = 1000, 1016, 32, 20, 6
    rng = np.random.default_rng(9)
    hist = rng.integers(0, V, (6, H))
    hist[:, :n] = np.where(hist[:, :n] == 77, 78, hist[:, :n])
    pl = [n - (m - 1), n - m, n - (m - 1), n - (m - 1), 0, 0]
    eos = [77, 77, -1, V, 77, 77]
    pos = [n - 1, n - 1, n - 1, n - 1, -1, H]
    bits, got, want = run(dt, V, row, hist, pos, seed=2, plant=False, min_new=[m] * 6, prompt_len=pl, eos=eos,
                          rp=[1.0, 1.0, 1.0, 1.0, 1.3, 1.3], ngram=[0, 0, 0, 0, 1, 1])
    same(got, want, dt)
    assert got[0, 77] == R.NEG_INF[dt]                         # m - 1 new tokens: held back
    assert np.array_equal(got[1:], bits[1:])                   # m new tokens; no eos; eos >= V; p = -1; p = hist_len
    assert np.array_equal(np.delete(got[0], 77), np.delete(bits[0], 77))


@pytest.mark.parametrize("dt", DTS)
def test_picks_never_return_a_banned_token(dt):
    from quantizations_amd import layer_ops as ops

    V, H, n, B = 1000, 32, 12, 3
    tdt = TORCH_DT[dt]
    g = torch.Generator().manual_seed(7)
    logits = torch.randn((B, V), generator=g).to(tdt).to(DEV)
    hist = torch.randint(0, V, (B, H), generator=g).to(DEV)
    hist[:, 0] = hist[:, n - 1]                                 # the bigram (h[0], h[1]) would repeat
    top = logits.argmax(-1)
    hist[:, 1] = top                                            # ... with the row's argmax
    pos = torch.full((B,), n - 1, dtype=torch.int64, device=DEV)
    ngram = torch.full((B,), 2, dtype=torch.int32, device=DEV)
    rp = torch.full((B,), 1.3, device=DEV)
    before = logits.clone()
    ops.process_logits(logits, hist, pos, repetition_penalty=rp, no_repeat_ngram=ngram)
    want = R.process(before.cpu().view(torch.int16).numpy().view(np.uint16), dt, V, hist.cpu().numpy(),
                     pos.cpu().numpy(), rp=[1.3] * B, ngram=[2] * B)
    assert np.array_equal(logits.cpu().view(torch.int16).numpy().view(np.uint16), want)
    assert bool(torch.isneginf(logits[torch.arange(B), top]).all())
    ref_pick = np.argmax(R.to_f32(want, dt), axis=1)
    live = torch.ones(B, dtype=torch.int32, device=DEV)
    stop = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    limit = torch.full((B,), H, dtype=torch.int64, device=DEV)
    for sampled in (False, True):
        h2, p2, tok = torch.zeros((B, H), dtype=torch.int64, device=DEV), pos.clone(), torch.zeros(B, dtype=torch.int64, device=DEV)
        if not sampled:
            ops.greedy_step_streams(logits, h2, p2, live.clone(), stop, limit, tok)
            assert tok.cpu().tolist() == ref_pick.tolist()
        else:
            for k, u in ((1, 0.5), (0, 0.0), (0, 0.999)):
                tok.zero_()
                ops.sample_step_streams(logits, h2, pos.clone(), live.clone(), stop, limit, tok,
                                        torch.ones(B, device=DEV), torch.full((B,), k, dtype=torch.int32, device=DEV),
                                        torch.ones(B, device=DEV), torch.full((B, H), u, device=DEV))
                banned = torch.isneginf(logits[torch.arange(B), tok])
                assert not bool(banned.any()), (k, u)
                assert bool((tok != top).all())
                if k == 1:
                    assert tok.cpu().tolist() == ref_pick.tolist()
