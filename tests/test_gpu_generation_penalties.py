"""GPU: the logits processors inside the sessions' steps (set_penalties, generate's keyword arguments)
on the tiny random-init Llama of test_gpu_generation_speculative.py.  Every check is exact: a captured
step against the eager one, the sessions against a loop that replaces the processing launch by
tests/logits_process_reference.py (numpy) on the same logits and then calls the same pick, a batch with
different settings per stream against each stream's own session, SpeculativeSession against
StreamSession with all five processors on under three drafters, replays that follow set_penalties(),
and sessions without settings, which hold no processing launch at all."""
import numpy as np
import pytest
import torch

import logits_process_reference as R
from test_gpu_generation_speculative import DRAFTS, LENGTHS, N, SENT, _build, _prompts, _sessions, _unprepare

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
PEN = dict(repetition_penalty=1.2, presence_penalty=0.3, frequency_penalty=0.2, no_repeat_ngram_size=3,
           min_new_tokens=10)
MIXED = dict(repetition_penalty=[1.3, 1.0, 0.8], presence_penalty=[0.0, 0.0, 0.5], frequency_penalty=[0.4, 0.0, 0.0],
             no_repeat_ngram_size=[2, 0, 4], min_new_tokens=[0, 0, 8])     # stream 1 is neutral
SAMPLING = dict(temperature=0.8, top_k=50, top_p=0.9)
SEED = 11


@pytest.fixture(scope="module")
def model():
    from quantizations_amd.generation import prepare_for_decode

    m = _build()
    prepare_for_decode(m)
    try:
        yield m
    finally:
        _unprepare(m)


def _run(sess):
    n = 0
    while bool(sess.alive().any()):
        sess.step()
        n += 1
        assert n <= N
    torch.cuda.synchronize()
    return sess


def _open(model, cls=None, *, pen=PEN, stop=None, sampling=None, graph=True, rows=(0, 1, 2), known=None, **kw):
    """A stream session over the prompts `rows` of the three ragged ones, prefilled."""
    from quantizations_amd.generation import StreamSession

    cls = StreamSession if cls is None else cls
    lens = [LENGTHS[r] for r in rows]
    sess = cls(model, len(rows), max(LENGTHS) + N, graph=graph, **kw)
    if known is not None:
        sess.known = known
    if sampling is not None:
        sess.set_sampling(**sampling)
        sess.seed(SEED)
    if pen is not None:
        sess.set_penalties(**pen)
    sess.hist.fill_(SENT)
    sess.prefill(_prompts()[list(rows)], lens, stop=stop, max_new_tokens=N)
    return sess


@pytest.fixture(scope="module")
def stops(model):
    """A stop token per stream that the penalised greedy run picks as its fourth token: min_new_tokens
    has something to hold back."""
    free = _run(_open(model, graph=False, pen={k: v for k, v in PEN.items() if k != "min_new_tokens"}))
    return [int(free.hist[b, n + 3]) for b, n in enumerate(LENGTHS)]


def _same(a, b):
    return torch.equal(a.hist, b.hist) and torch.equal(a.pos, b.pos) and torch.equal(a.live, b.live)


def _trigrams(seq):
    return list(zip(seq[:-2], seq[1:-1], seq[2:]))


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_stream_session_graph_equals_eager(model, stops, sampled):
    sampling = SAMPLING if sampled else None
    a = _run(_open(model, stop=stops, sampling=sampling, graph=True))
    b = _run(_open(model, stop=stops, sampling=sampling, graph=False))
    assert a._graph is not None and b._graph is None and a._processing and b._processing
    assert _same(a, b)
    plain = _run(_open(model, pen=None, stop=stops, sampling=sampling, graph=False))
    assert not plain._processing and not torch.equal(plain.hist, a.hist)       # the processors do something
    for r, (seq, n) in enumerate(zip(a.sequences(), LENGTHS)):
        seq = seq.tolist()
        assert len(set(_trigrams(seq))) == len(_trigrams(seq)), r              # no_repeat_ngram_size = 3
        assert stops[r] not in seq[n:n + PEN["min_new_tokens"]], r              # held back for ten tokens
        assert a.prompt_len[r] == n


def test_decode_session_graph_equals_eager(model, stops):
    from quantizations_amd.generation import DecodeSession

    ids = _prompts()
    out = []
    for graph in (True, False):
        sess = DecodeSession(model, 3, ids.shape[1] + N, graph=graph)
        sess.set_penalties(**PEN)
        sess.stop.copy_(torch.tensor(stops))
        sess.prefill(ids)
        for _ in range(N - 1):
            sess.step()
        torch.cuda.synchronize()
        assert (sess._graph is not None) == graph and sess.prompt_len.tolist() == [ids.shape[1]] * 3
        out.append(sess.hist.clone())
    assert torch.equal(out[0], out[1])
    for r, seq in enumerate(out[0].tolist()):
        assert len(set(_trigrams(seq))) == len(_trigrams(seq)), r


def _manual_class():
    """A StreamSession whose processing launch is the numpy reference on the host."""
    from quantizations_amd.generation import StreamSession

    class Manual(StreamSession):
        def _process(self, logits, rows=slice(None), tok=None):
            assert tok is None and logits.dtype == torch.float16
            bits = logits.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
            c = lambda t: t[rows].cpu().numpy()   # noqa: E731
            want = R.process(bits, R.F16, logits.shape[1], c(self._hist_full), c(self.pos),
                             rp=c(self.repetition_penalty), pp=c(self.presence_penalty), fp=c(self.frequency_penalty),
                             ngram=c(self.no_repeat_ngram), min_new=c(self.min_new_tokens),
                             prompt_len=c(self.prompt_len), eos=c(self.stop))
            logits.copy_(torch.from_numpy(want.view(np.int16)).view(torch.float16).to(logits.device))

    return Manual


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("which", ["all_on", "mixed"])
def test_stream_session_equals_a_manual_loop(model, stops, sampled, which):
    sampling = SAMPLING if sampled else None
    pen = PEN if which == "all_on" else MIXED
    a = _run(_open(model, pen=pen, stop=stops, sampling=sampling, graph=True))
    m = _run(_open(model, _manual_class(), pen=pen, stop=stops, sampling=sampling, graph=False))
    assert _same(a, m)


def test_per_stream_settings_equal_each_streams_own_session(model, stops):
    batch = _run(_open(model, pen=MIXED, stop=stops, graph=True))
    plain = _run(_open(model, pen=None, stop=stops, graph=True))
    assert torch.equal(batch.hist[1], plain.hist[1])                  # the neutral stream among processed ones
    assert not torch.equal(batch.hist[0], plain.hist[0]) and not torch.equal(batch.hist[2], plain.hist[2])
    for r in range(3):
        own = {k: v[r] for k, v in MIXED.items()}
        alone = _run(_open(model, pen=own, stop=[stops[r]], graph=True, rows=(r,)))
        assert torch.equal(alone.hist[0], batch.hist[r]), r
        assert alone.pos[0] == batch.pos[r]


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_speculative_session_equals_stream_session(model, stops, sampled):
    Ngram, Null, Replay = _sessions()
    sampling = SAMPLING if sampled else None
    one = _run(_open(model, stop=stops, sampling=sampling, graph=True))
    kw = dict(stop=stops, sampling=sampling, draft_tokens=DRAFTS, sample=sampled)
    ngram = _run(_open(model, Ngram, graph=True, **kw))
    assert ngram._processing and ngram._graph is not None
    assert _same(ngram, one), "n-gram drafter"
    null = _run(_open(model, Null, graph=True, **kw))                  # wrong on purpose
    assert _same(null, one), "null drafter"
    replay = _run(_open(model, Replay, graph=False, known=one._hist_full.clone(), **kw))   # always right
    assert _same(replay, one), "replay drafter"
    steps = replay.stats()["steps"].tolist()
    tokens = replay.stats()["tokens"].tolist()
    assert all(s == -(-t // (DRAFTS + 1)) for s, t in zip(steps, tokens)), (steps, tokens)   # whole windows accepted
    mixed_one = _run(_open(model, pen=MIXED, stop=stops, sampling=sampling, graph=True))
    mixed = _run(_open(model, Ngram, pen=MIXED, graph=True, **kw))
    assert _same(mixed, mixed_one), "per-stream settings"


def _bigrams(seq):
    return list(zip(seq[:-1], seq[1:]))


def test_generate_no_repeat_ngram(model):
    from quantizations_amd.generation import generate, generate_ragged

    ids = _prompts()
    n_new = 40
    plain = generate(model, ids, n_new, no_repeat_ngram_size=2)
    lookup = generate(model, ids, n_new, no_repeat_ngram_size=2, prompt_lookup_num_tokens=DRAFTS)
    sampled = generate(model, ids, n_new, no_repeat_ngram_size=2, do_sample=True, generator=3, prompt_lookup_num_tokens=DRAFTS,
                       prompt_lookup_sampling=True, **SAMPLING)
    for out in (plain, lookup, sampled):
        assert out.shape == (3, ids.shape[1] + n_new) and torch.equal(out[:, :ids.shape[1]], ids)
        for row in out.tolist():
            assert len(set(_bigrams(row))) == len(_bigrams(row)), row
    prompts = [ids[b, :n] for b, n in enumerate(LENGTHS)]
    for kw in (dict(), dict(prompt_lookup_num_tokens=DRAFTS)):
        rag = generate_ragged(model, prompts, n_new, no_repeat_ngram_size=[2, 2, 2], repetition_penalty=1.1, **kw)
        for seq, n in zip(rag, LENGTHS):
            seq = seq.tolist()
            assert len(seq) == n + n_new and len(set(_bigrams(seq))) == len(_bigrams(seq))


def test_replay_follows_set_penalties(model, stops):
    later = dict(repetition_penalty=[1.0, 1.5, 1.2], presence_penalty=[0.0, 0.0, 0.3], frequency_penalty=[0.0, 0.6, 0.2],
                 no_repeat_ngram_size=[0, 2, 3], min_new_tokens=[0, 20, 10])         # stream 0 goes back to neutral
    k = 5
    out = []
    for graph in (True, False):
        sess = _open(model, stop=stops, graph=graph)
        for _ in range(k):
            sess.step()
        captured = sess._graph
        sess.set_penalties(**later)
        assert sess._processing
        _run(sess)
        assert sess._graph is captured and (captured is not None) == graph      # no recapture
        out.append(sess)
    assert _same(out[0], out[1])
    never = _run(_open(model, stop=stops, graph=True))
    assert not torch.equal(never.hist, out[0].hist)
    for r, n in enumerate(LENGTHS):                                              # the same tokens up to the switch
        assert torch.equal(never.hist[r, :n + 1 + k], out[0].hist[r, :n + 1 + k]), r


def test_enabling_a_processor_after_a_neutral_capture_raises(model):
    sess = _open(model, pen=None, graph=True)
    sess.step()
    assert sess._graph is not None and not sess._processing
    with pytest.raises(ValueError, match="without logits processing"):
        sess.set_penalties(repetition_penalty=1.2)
    with pytest.raises(ValueError, match="without logits processing"):
        sess.set_penalties(no_repeat_ngram_size=[0, 0, 2])
    sess.set_penalties(repetition_penalty=1.0, min_new_tokens=0)                 # neutral values are no change
    assert not sess._processing
    eager = _open(model, pen=None, graph=False)
    eager.step()
    eager.set_penalties(repetition_penalty=1.2)                                  # nothing captured: free to change
    assert eager._processing


def test_a_session_without_settings_launches_no_processing(model, monkeypatch):
    from quantizations_amd import layer_ops
    from quantizations_amd.generation import SpeculativeSession, generate_ragged

    def boom(*a, **k):
        raise AssertionError("process_logits was called by a session without penalties")

    monkeypatch.setattr(layer_ops, "process_logits", boom)
    prompts = [_prompts()[b, :n] for b, n in enumerate(LENGTHS)]
    want = generate_ragged(model, prompts, N)
    sess = _run(_open(model, pen=None, graph=True))
    assert not sess._processing and all(sess._neutral.values())
    for seq, w in zip(sess.sequences(), want):
        assert torch.equal(seq, w)
    spec = _run(_open(model, SpeculativeSession, pen=None, graph=True, draft_tokens=DRAFTS))
    assert not spec._processing
    for seq, w in zip(spec.sequences(), want):
        assert torch.equal(seq, w)
    neutral = _run(_open(model, pen=dict(repetition_penalty=1.0, presence_penalty=0.0, no_repeat_ngram_size=0), graph=True))
    assert not neutral._processing and _same(neutral, sess)
