"""GPU: `logprobs` in DecodeSession / StreamSession / SpeculativeSession, generate() / generate_ragged()
and score(), on the tiny random-init Llama of test_gpu_generation_prefill.py (a prepared model and an
unfused twin with the same weights).

Exact checks: a session with logprobs emits the tokens, pos and live of the same session without;
graph and eager fill bit-equal tables; a greedy session's top-1 is its token with the same bits; with
penalties the tables are those of the raw rows; a speculative window fills every emitted column once;
admit() resets and fork() copies a row.  Against the unfused twin, teacher-forced with fp32
log_softmax: |logprobs - ref| <= 2 tol, tol the fixture's measured value (twice the largest logit
difference d between the decode path and the unfused model) -- a logit error d moves a
log-probability by at most 2 d, so the bar keeps a factor of two.  The tests print the largest
difference."""
import pytest
import torch

from test_gpu_generation_prefill import LENGTHS, SMAX, _build, _decode_path_logits, _prompts, _unprepare

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
S, N, NTOP, DRAFTS = 8, 12, 5, 3
L = SMAX + N + 4


@pytest.fixture(scope="module")
def tiny():
    """(prepared model, unfused twin, tol)"""
    from quantizations_amd.generation import prepare_for_decode

    ref = _build()
    model = _build()
    ids = torch.randint(0, 4096, (3, S), generator=torch.Generator().manual_seed(1)).to(DEV)
    prepare_for_decode(model)
    try:
        seq, lo = _decode_path_logits(model, ids, 24)
        with torch.inference_mode():
            want = torch.stack([ref(input_ids=seq[b:b + 1]).logits[0, S - 1:S + 23].float() for b in range(3)])
        d = float((lo - want).abs().max())
        print(f"decode path vs unfused model: largest |logit difference| d = {d:.6f}, tol = {2 * d:.6f}")
        assert 0 < d < 1.0, d    # a sanity bracket around the measurement, not the bar
        yield model, ref, 2 * d
    finally:
        _unprepare(model)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _open(model, kind, mode, logprobs, graph=True, **kw):
    from quantizations_amd.generation import DecodeSession, SpeculativeSession, StreamSession

    if kind == "decode":
        sess = DecodeSession(model, 3, S + N, graph=graph, logprobs=logprobs)
    elif kind == "stream":
        sess = StreamSession(model, 3, L, graph=graph, logprobs=logprobs, **kw)
    else:
        sess = SpeculativeSession(model, 3, L, draft_tokens=DRAFTS, graph=graph, sample=mode == "sampled",
                                  logprobs=logprobs, **kw)
    if mode == "sampled":
        sess.set_sampling(temperature=[0.8, 1.1, 0.0], top_k=[40, 0, 0], top_p=[1.0, 0.9, 1.0])
        sess.seed(7)
    if mode == "penalties":
        sess.set_penalties(repetition_penalty=1.3, frequency_penalty=0.4, no_repeat_ngram_size=2)
    return sess


def _run(model, kind, mode, logprobs, graph=True, steps=N - 1, **kw):
    sess = _open(model, kind, mode, logprobs, graph, **kw)
    if kind == "decode":
        sess.prefill(torch.randint(0, 4096, (3, S), generator=torch.Generator().manual_seed(5)))
    else:
        sess.prefill(_prompts(), LENGTHS, max_new_tokens=N)
    for _ in range(steps):
        sess.step()
    torch.cuda.synchronize()
    return sess


def _spans(sess, kind):
    """Per stream: (first generated column, one past the last)."""
    if kind == "decode":
        return [(S, int(sess.pos) + 1)] * 3
    return [(n, p + 1) for n, p in zip(LENGTHS, sess.pos.tolist())]


def _same_tables(a, b):
    return (torch.equal(_bits(a.logprobs), _bits(b.logprobs)) and torch.equal(a.top_ids, b.top_ids)
            and torch.equal(_bits(a.top_logprobs), _bits(b.top_logprobs)))


def _filled_exactly(sess, spans):
    for b, (lo, hi) in enumerate(spans):
        assert bool(torch.isnan(sess.logprobs[b, :lo]).all()) and bool(torch.isnan(sess.logprobs[b, hi:]).all())
        assert bool(torch.isfinite(sess.logprobs[b, lo:hi]).all())
        assert bool((sess.top_ids[b, :lo] == -1).all()) and bool((sess.top_ids[b, hi:] == -1).all())
        assert bool((sess.top_ids[b, lo:hi] >= 0).all()) and bool(torch.isfinite(sess.top_logprobs[b, lo:hi]).all())
        assert bool(torch.isnan(sess.top_logprobs[b, :lo]).all()) and bool(torch.isnan(sess.top_logprobs[b, hi:]).all())


def _against_twin(ref, sess, spans, tol, who):
    worst = 0.0
    with torch.inference_mode():
        for b, (lo, hi) in enumerate(spans):
            seq = sess.hist[b, :hi]
            want = torch.log_softmax(ref(input_ids=seq[None]).logits[0, lo - 1:hi - 1].float(), -1)
            got = sess.logprobs[b, lo:hi]
            worst = max(worst, float((got - want.gather(1, seq[lo:, None])[:, 0]).abs().max()))
            if sess.top_ids.shape[-1]:
                ids = sess.top_ids[b, lo:hi].long()
                worst = max(worst, float((sess.top_logprobs[b, lo:hi] - want.gather(1, ids)).abs().max()))
    print(f"{who}: largest |logprob - unfused twin| = {worst:.6f}, bar 2 tol = {2 * tol:.6f}")
    assert worst <= 2 * tol, (who, worst, 2 * tol)


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
@pytest.mark.parametrize("kind", ["decode", "stream", "speculative"])
def test_same_tokens_and_graph_equals_eager(tiny, kind, mode):
    model, ref, tol = tiny
    plain = _run(model, kind, mode, None)
    assert plain.logprobs is None and plain.top_ids is None and plain.top_logprobs is None and plain._pos0 is None
    sess = _run(model, kind, mode, NTOP)
    eager = _run(model, kind, mode, NTOP, graph=False)
    assert torch.equal(plain.hist, sess.hist) and torch.equal(plain.pos, sess.pos) and torch.equal(plain.tok, sess.tok)
    if kind != "decode":
        assert torch.equal(plain.live, sess.live)
    assert sess.logprobs.shape == sess.hist.shape and sess.top_ids.shape == sess.hist.shape + (NTOP,)
    assert _same_tables(sess, eager)
    spans = _spans(sess, kind)
    assert all(hi - lo == N for lo, hi in spans)
    _filled_exactly(sess, spans)
    if mode == "greedy":     # the pick and the top-1 read the same row and share argmax's first-index rule
        for b, (lo, hi) in enumerate(spans):
            assert torch.equal(sess.top_ids[b, lo:hi, 0].long(), sess.hist[b, lo:hi])
            assert torch.equal(_bits(sess.logprobs[b, lo:hi]), _bits(sess.top_logprobs[b, lo:hi, 0]))
    _against_twin(ref, sess, spans, tol, f"{kind} {mode}")


def test_chosen_only_has_no_lists(tiny):
    model = tiny[0]
    a, b = _run(model, "stream", "greedy", 0, steps=3), _run(model, "stream", "greedy", NTOP, steps=3)
    assert a.top_ids.shape == a.hist.shape + (0,) and torch.equal(_bits(a.logprobs), _bits(b.logprobs))


@pytest.mark.parametrize("kind", ["decode", "stream"])
def test_penalties_report_the_raw_rows(tiny, kind):
    """The processors rewrite the logits in place before the pick; the tables still describe the model's
    own rows: a hook keeps every forward's logits of an eager session before they are processed."""
    from quantizations_amd.layer_ops import token_logprobs

    model = tiny[0]
    plain = _run(model, kind, "penalties", None)
    assert plain._processing                                  # the step holds a processing launch
    sess = _run(model, kind, "penalties", NTOP)
    assert torch.equal(plain.hist, sess.hist) and torch.equal(plain.pos, sess.pos)
    kept = []
    hook = model.register_forward_hook(lambda m, a, out: kept.append(out.logits.clone()))
    try:
        eager = _run(model, kind, "penalties", NTOP, graph=False)
    finally:
        hook.remove()
    assert _same_tables(sess, eager) and len(kept) == N
    starts = [S] * 3 if kind == "decode" else LENGTHS
    for k, lo in enumerate(kept):          # forward k picked column start + k of every stream
        for b, n in enumerate(starts):
            row = lo[b, (n - 1) if k == 0 else -1][None].contiguous()
            lp, ti, tl = token_logprobs(row, eager.hist[b, n + k].reshape(1), NTOP)
            assert torch.equal(_bits(lp), _bits(eager.logprobs[b, n + k].reshape(1)))
            assert torch.equal(ti[0], eager.top_ids[b, n + k]) and torch.equal(_bits(tl[0]), _bits(eager.top_logprobs[b, n + k]))


def _drafters():
    from quantizations_amd.generation import SpeculativeSession

    class Null(SpeculativeSession):
        def _draft(self):
            super()._draft()                                     # pos_ids
            self.tok[:, 1:] = (self.tok[:, :1] + 1) % 4096

    class Replay(SpeculativeSession):
        known = None

        def _draft(self):
            ar = torch.arange(self.T, device=self.device)
            self.pos_ids.copy_(self.pos[:, None] + ar[None, :])
            nxt = (self.pos_ids[:, 1:]).clamp(max=self.known.shape[1] - 1)
            self.tok[:, 1:] = self.known.gather(1, nxt).clamp(min=0)

    return Null, Replay


@pytest.mark.parametrize("drafts", ["perfect", "useless"])
@pytest.mark.parametrize("penalties", [False, True])
def test_speculative_window_fills_every_emitted_column_once(tiny, drafts, penalties):
    model, ref, tol = tiny
    mode = "penalties" if penalties else "greedy"
    base = _run(model, "stream", mode, NTOP)
    Null, Replay = _drafters()
    cls = Replay if drafts == "perfect" else Null
    sess = cls(model, 3, L, draft_tokens=DRAFTS, logprobs=NTOP)
    sess.known = base._hist_full.clone()
    if penalties:
        sess.set_penalties(repetition_penalty=1.3, frequency_penalty=0.4, no_repeat_ngram_size=2)
    sess.prefill(_prompts(), LENGTHS, max_new_tokens=N)
    steps = 0
    while bool(sess.alive().any()):
        sess.step()
        steps += 1
        assert steps <= N
    torch.cuda.synchronize()
    if drafts == "perfect":
        assert steps == -(-(N - 1) // (DRAFTS + 1))
    assert torch.equal(sess.hist, base.hist) and torch.equal(sess.pos, base.pos)
    spans = _spans(sess, "speculative")
    _filled_exactly(sess, spans)
    filled = (~torch.isnan(sess.logprobs)).sum(1).cpu()
    assert torch.equal(filled, sess.stats()["tokens"] + 1)             # the steps' tokens and prefill's first
    # a row of the window carries the bits of the one-token step on the same logits -- where the logits
    # are the same bits: the window's GEMMs are another route, so the values are held against the twin
    # and the ids against the plain session wherever its top-two gap is clear of tol
    _against_twin(ref, sess, spans, tol, f"speculative {drafts} penalties={penalties}")
    if not penalties:
        for b, (lo, hi) in enumerate(spans):
            assert torch.equal(sess.top_ids[b, lo:hi, 0].long(), sess.hist[b, lo:hi])


def test_admit_resets_a_row_and_fork_copies_it(tiny):
    from quantizations_amd.generation import StreamSession

    model = tiny[0]
    sess = StreamSession(model, 3, L, prefill_chunk=5, kv_pages=12, logprobs=NTOP)
    sess.prefill(_prompts(), LENGTHS, max_new_tokens=N)
    for _ in range(4):
        sess.step()
    before = [t.clone() for t in (sess.logprobs, sess.top_ids, sess.top_logprobs)]
    _filled_exactly(sess, [(n, n + 5) for n in LENGTHS])
    sess.fork(0, 2)
    for t in (sess.logprobs, sess.top_ids, sess.top_logprobs):
        assert torch.equal(t[2].view(torch.int32), t[0].view(torch.int32))
    prompt = torch.randint(0, 4096, (4,), generator=torch.Generator().manual_seed(9))
    sess.admit(1, prompt, max_new_tokens=N)
    torch.cuda.synchronize()
    assert bool(torch.isnan(sess.logprobs[1, :4]).all()) and bool(torch.isnan(sess.logprobs[1, 5:]).all())
    assert bool(torch.isfinite(sess.logprobs[1, 4])) and bool((sess.top_ids[1, 5:] == -1).all())
    assert torch.equal(_bits(sess.logprobs[0]), _bits(before[0][0]))   # the other streams keep theirs
    for _ in range(3):
        sess.step()
    torch.cuda.synchronize()
    _filled_exactly(sess, [(LENGTHS[0], LENGTHS[0] + 8), (4, 8), (LENGTHS[0], LENGTHS[0] + 8)])


@pytest.mark.parametrize("kv_dtype", [None, "fp8"])
def test_paged_sessions_fill_the_tables(tiny, kv_dtype):
    model, ref, tol = tiny
    plain = _run(model, "stream", "greedy", None, prefill_chunk=5, kv_pages=12, kv_dtype=kv_dtype)
    sess = _run(model, "stream", "greedy", NTOP, prefill_chunk=5, kv_pages=12, kv_dtype=kv_dtype)
    assert torch.equal(plain.hist, sess.hist) and torch.equal(plain.pos, sess.pos)
    _filled_exactly(sess, _spans(sess, "stream"))
    if kv_dtype is None:
        _against_twin(ref, sess, _spans(sess, "stream"), tol, "paged")


def test_generate_and_generate_ragged_return_generate_output(tiny):
    import quantizations_amd as qa

    model = tiny[0]
    ids = torch.randint(0, 4096, (2, S), generator=torch.Generator().manual_seed(5)).to(DEV)
    plain = qa.generate(model, ids, 6)
    out = qa.generate(model, ids, 6, logprobs=2)
    assert isinstance(out, qa.GenerateOutput) and torch.equal(out.sequences, plain)
    assert out.logprobs.shape == (2, S + 6) and out.top_ids.shape == out.top_logprobs.shape == (2, S + 6, 2)
    assert bool(torch.isnan(out.logprobs[:, :S]).all()) and bool(torch.isfinite(out.logprobs[:, S:]).all())
    spec = qa.generate(model, ids, 6, prompt_lookup_num_tokens=2, logprobs=2)
    assert torch.equal(spec.sequences, qa.generate(model, ids, 6, prompt_lookup_num_tokens=2))
    assert bool(torch.isnan(spec.logprobs[:, :S]).all()) and bool(torch.isfinite(spec.logprobs[:, S:]).all())
    prompts = [_prompts()[b, :n] for b, n in enumerate(LENGTHS)]
    kw = dict(do_sample=True, temperature=0.9, top_k=50, generator=3, repetition_penalty=1.2, prefill_chunk=5,
              kv_pages=12, kv_dtype="fp8")
    want = qa.generate_ragged(model, prompts, 6, **kw)
    got = qa.generate_ragged(model, prompts, 6, logprobs=3, **kw)
    assert isinstance(got, qa.GenerateOutput) and all(torch.equal(a, b) for a, b in zip(got.sequences, want))
    for b, n in enumerate(LENGTHS):
        assert got.logprobs[b].shape == (n + 6,) and got.top_ids[b].shape == (n + 6, 3)
        assert bool(torch.isnan(got.logprobs[b][:n]).all()) and bool(torch.isfinite(got.logprobs[b][n:]).all())


@pytest.mark.parametrize("chunk", [11, 5, 1])
def test_score_against_the_unfused_twin(tiny, chunk):
    import quantizations_amd as qa
    from quantizations_amd.generation import StreamSession

    model, ref, tol = tiny
    prompts = [_prompts()[b, :n] for b, n in enumerate(LENGTHS)]
    got = qa.score(model, prompts, prefill_chunk=chunk)
    worst = 0.0
    with torch.inference_mode():
        for p, t in zip(prompts, got):
            assert t.shape == p.shape and t.dtype == torch.float32 and bool(torch.isnan(t[0]))
            want = torch.log_softmax(ref(input_ids=p[None]).logits[0, :-1].float(), -1).gather(1, p[1:, None])[:, 0]
            assert bool(torch.isfinite(t[1:]).all())
            if p.numel() > 1:
                worst = max(worst, float((t[1:] - want).abs().max()))
    print(f"score chunk={chunk}: largest |logprob - unfused twin| = {worst:.6f}, bar 2 tol = {2 * tol:.6f}")
    assert worst <= 2 * tol
    # a session with prompt_logprobs fills the same bits at the same chunk size, and generates behind them
    sess = StreamSession(model, 3, L, prefill_chunk=chunk, logprobs=2, prompt_logprobs=True)
    sess.prefill(_prompts(), LENGTHS, max_new_tokens=N)
    sess.step()
    torch.cuda.synchronize()
    for b, n in enumerate(LENGTHS):
        assert torch.equal(_bits(sess.logprobs[b, :n]), _bits(got[b]))
        assert bool(torch.isfinite(sess.logprobs[b, n:n + 2]).all()) and bool(torch.isnan(sess.logprobs[b, n + 2:]).all())
        assert bool((sess.top_ids[b, 1:n + 2] >= 0).all()) and bool((sess.top_ids[b, 0] == -1).all())
    with_top = qa.score(model, prompts, top_logprobs=2, prefill_chunk=chunk)
    for b, n in enumerate(LENGTHS):
        assert torch.equal(_bits(with_top[b][0]), _bits(got[b])) and torch.equal(with_top[b][1], sess.top_ids[b, :n])


def test_a_prefix_cache_hit_leaves_its_mapped_columns_nan(tiny):
    from quantizations_amd.generation import StreamSession

    model = tiny[0]
    long = torch.randint(0, 4096, (140,), generator=torch.Generator().manual_seed(4)).to(DEV)
    sess = StreamSession(model, 2, 160, prefill_chunk=64, kv_pages=8, prefix_cache=True, logprobs=0,
                         prompt_logprobs=True)
    ids = torch.zeros((2, 140), dtype=torch.int64, device=DEV)
    ids[0], ids[1, :3] = long, long[:3]
    sess.prefill(ids, [140, 3], max_new_tokens=4)
    full = sess.logprobs[0].clone()
    assert bool(torch.isnan(full[0])) and bool(torch.isfinite(full[1:141]).all())
    sess.admit(1, long, max_new_tokens=4)          # page 0 (columns 0..127) is mapped: no forward ran there
    torch.cuda.synchronize()
    got = sess.logprobs[1]
    assert bool(torch.isnan(got[:129]).all()) and bool(torch.isfinite(got[129:141]).all()) and bool(torch.isnan(got[141:]).all())


def test_refusals_name_the_argument(tiny):
    import quantizations_amd as qa

    model, ref, _ = tiny
    for cls in (qa.DecodeSession, qa.StreamSession, qa.SpeculativeSession):
        with pytest.raises(ValueError, match="logprobs"):
            cls(model, 1, 16, logprobs=21)
    with pytest.raises(ValueError, match="prompt_logprobs"):
        qa.StreamSession(model, 1, 16, logprobs=0, prompt_logprobs=True)
    with pytest.raises(ValueError, match="prompt_logprobs"):
        qa.StreamSession(model, 1, 16, prefill_chunk=4, prompt_logprobs=True)
    with pytest.raises(ValueError, match="model"):
        qa.score(ref, [torch.zeros(4, dtype=torch.int64)])
    with pytest.raises(ValueError, match="top_logprobs"):
        qa.score(model, [torch.zeros(4, dtype=torch.int64)], top_logprobs=21)
