"""GPU: constrained decoding inside the sessions' steps (constraint=, constraint_start=, set_logit_bias,
set_token_mask, generate's keyword arguments) on the tiny random-init Llama of
test_gpu_generation_speculative.py.  Every check is exact: the emitted tokens against the automaton, an
unconstrained stream against the session without a constraint, a captured step against the eager one,
SpeculativeSession against StreamSession, and every constrained pick against the unfused twin's strict
argmax among the allowed tokens (masked on the host with tests/constraint_reference.py), at every
position: the twin's top-two gap among the allowed tokens is asserted to be at least the fixture's tol
at each of them (most positions allow one to three tokens, so the gap is that of two or three
random-init logits; the prompt seed 3 is the speculative file's).
Measured on an MI355X: d = 0.001343, tol = 0.002686; 11 constrained positions over the three streams, 6 of
them with one allowed token, the others with gaps of 0.304, 0.440, 1.019, 0.290 and 1.467; the stream whose
forced choice stands in its prompt emitted its 7 step tokens in 2 steps."""
import numpy as np
import pytest
import torch

import constraint_reference as R
import quantizations_amd as qa
from test_gpu_generation_speculative import DRAFTS, LENGTHS, N, SENT, _prompts, tiny  # noqa: F401  (tiny: the fixture)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
V, EOS = 4096, 4095
CHOICES = [[11, 12, 13, 14], [11, 12, 20], [11, 30, 31, 32, 33, 34], [40], [11, 12]]
OTHER = [[900, 901, 902], [903]]
SAMPLING = dict(temperature=0.9, top_k=50, top_p=0.95)
SEED = 5
FORCED = [100, 101, 102, 103, 104, 105, 106]      # the single choice of the lookup case; it stands in the prompt


@pytest.fixture(scope="module")
def automata():
    """(joint automaton, [start of CHOICES, start of OTHER, start of FORCED])"""
    parts = [qa.TokenAutomaton.from_choices(c, EOS, V) for c in (CHOICES, OTHER, [FORCED])]
    return qa.TokenAutomaton.concat(parts)


def _run(sess):
    n = 0
    while bool(sess.alive().any()):
        sess.step()
        n += 1
        assert n <= N
    torch.cuda.synchronize()
    return sess


def _open(model, cls=None, *, constraint=None, start=None, sampling=None, graph=True, prompts=None, lens=LENGTHS,
          bias=None, **kw):
    from quantizations_amd.generation import StreamSession

    cls = StreamSession if cls is None else cls
    sess = cls(model, 3, max(lens) + N, graph=graph, constraint=constraint, **kw)
    if sampling is not None:
        sess.set_sampling(**sampling)
        sess.seed(SEED)
    if bias is not None:
        sess.set_logit_bias(None, bias)
    sess.hist.fill_(SENT)
    ids = _prompts() if prompts is None else prompts
    extra = {} if constraint is None else dict(constraint_start=start)
    sess.prefill(ids, lens, stop=EOS, max_new_tokens=N, **extra)
    return sess


def _same(a, b):
    ok = torch.equal(a.hist, b.hist) and torch.equal(a.pos, b.pos) and torch.equal(a.live, b.live)
    if a.constraint_state is not None and b.constraint_state is not None:
        ok = ok and torch.equal(a.constraint_state, b.constraint_state)
    return ok


def _new_tokens(sess):
    return [seq[n:].tolist() for seq, n in zip(sess.sequences(), sess.prompt_len.tolist())]


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_choices_and_an_unconstrained_stream(tiny, automata, sampled):
    model = tiny[0]
    joint, starts = automata
    sampling = SAMPLING if sampled else None
    sess = _run(_open(model, constraint=joint, start=[starts[0], -1, starts[1]], sampling=sampling))
    plain = _run(_open(model, sampling=sampling))
    new = _new_tokens(sess)
    assert new[0][-1] == EOS and new[0][:-1] in CHOICES, new[0]
    assert new[2][-1] == EOS and new[2][:-1] in OTHER, new[2]
    # the terminal states; stream 1 was never constrained and carries the bits of the session without
    S0 = qa.TokenAutomaton.from_choices(CHOICES, EOS, V).S
    assert sess.constraint_state.tolist() == [S0 - 1, -1, starts[2] - 1]
    assert torch.equal(sess.hist[1], plain.hist[1]) and sess.pos[1] == plain.pos[1]
    assert plain.constraint_state is None and len(new[1]) >= 1
    assert not torch.equal(sess.hist[0], plain.hist[0])


def test_every_constrained_pick_is_the_twins_argmax_among_the_allowed(tiny, automata):
    model, ref, _, tol = tiny
    joint, starts = automata
    start = [starts[0], starts[0], starts[1]]
    sess = _run(_open(model, constraint=joint, start=start))
    checked = 0
    for b, seq in enumerate(sess.sequences()):
        n = LENGTHS[b]
        with torch.inference_mode():
            lo = ref(input_ids=seq[None]).logits[0, n - 1:seq.numel() - 1]            # the rows that pick seq[n:]
        bits = lo.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
        s = start[b]
        for j, t in enumerate(seq[n:].tolist()):
            masked = R.constrain(bits[j:j + 1], R.F16, V, state=[s], class_of=joint.class_of, nxt=joint.next)
            x = R.to_f32(masked[0], R.F16)
            allowed = joint.allowed(s)
            assert np.array_equal(np.isneginf(x), ~allowed | np.isneginf(R.to_f32(bits[j], R.F16)))
            top = np.sort(x)[::-1][:2]
            gap = top[0] - top[1]                                                      # inf where one token is allowed
            print(b, j, "allowed", int(allowed.sum()), "gap", float(gap), "tol", tol)
            assert gap >= tol, (b, j, float(gap), tol)
            assert t == int(np.argmax(x)), (b, j)
            s = joint.step(s, t)
            assert s >= 0
            checked += 1
    assert checked >= 6


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_graph_equals_eager(tiny, automata, sampled):
    model = tiny[0]
    joint, starts = automata
    kw = dict(constraint=joint, start=[starts[0], -1, starts[1]], sampling=SAMPLING if sampled else None,
              logit_bias_slots=4, bias={11: 0.5, 7: -2.0})
    a = _run(_open(model, graph=True, **kw))
    b = _run(_open(model, graph=False, **kw))
    assert a._graph is not None and b._graph is None and a._constraining and b._constraining
    assert _same(a, b)


def test_decode_session_and_generate(tiny, automata):
    from quantizations_amd.generation import DecodeSession, generate, generate_ragged

    model = tiny[0]
    joint, starts = automata
    ids = _prompts()
    out = []
    for graph in (True, False):
        sess = DecodeSession(model, 3, ids.shape[1] + 10, graph=graph, constraint=joint)
        sess.prefill(ids, constraint_start=[starts[0], -1, starts[1]])
        for _ in range(9):
            sess.step()
        torch.cuda.synchronize()
        out.append((sess.hist.clone(), sess.constraint_state.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    S = ids.shape[1]
    gen = generate(model, ids, 10, constraint=joint, constraint_start=[starts[0], -1, starts[1]], eos_token_id=EOS)
    assert torch.equal(gen, out[0][0][:, :S + 10])
    row = gen[0, S:].tolist()
    k = row.index(EOS)
    assert row[:k] in CHOICES and set(row[k:]) == {EOS}
    for kw in (dict(), dict(prompt_lookup_num_tokens=DRAFTS)):
        rag = generate_ragged(model, [ids[b, :n] for b, n in enumerate(LENGTHS)], 10, constraint=joint,
                              constraint_start=starts[1], eos_token_id=EOS, **kw)
        for seq, n in zip(rag, LENGTHS):
            assert seq[n:].tolist()[:-1] in OTHER and int(seq[-1]) == EOS
    with pytest.raises(ValueError, match="constraint_start needs"):
        generate(model, ids, 4, constraint_start=0)


def test_admit_under_the_captured_graph_follows_another_start(tiny, automata):
    model = tiny[0]
    joint, starts = automata
    prompt = torch.randint(0, V, (4,), generator=torch.Generator().manual_seed(9))
    out = []
    for graph in (True, False):
        sess = _open(model, constraint=joint, start=starts[0], graph=graph)
        for _ in range(2):
            sess.step()
        captured = sess._graph
        sess.admit(1, prompt, stop=EOS, max_new_tokens=N, constraint_start=starts[1])
        assert int(sess.constraint_state[1]) != starts[1]                       # the first pick advanced it
        _run(sess)
        assert sess._graph is captured and (captured is not None) == graph      # no recapture
        out.append(sess)
    assert _same(out[0], out[1])
    new = out[0].sequences()[1][4:].tolist()
    assert new[-1] == EOS and new[:-1] in OTHER, new
    first = out[0].sequences()[0][LENGTHS[0]:].tolist()
    assert first[:-1] in CHOICES


def test_fork_copies_the_state(tiny, automata):
    from quantizations_amd.generation import StreamSession

    model = tiny[0]
    joint, starts = automata
    sess = StreamSession(model, 3, max(LENGTHS) + N, prefill_chunk=5, kv_pages=12, constraint=joint)
    sess.prefill(_prompts(), LENGTHS, stop=EOS, max_new_tokens=N, constraint_start=[starts[2], starts[0], -1])
    sess.step()
    sess.step()                                       # stream 0 is three tokens into the forced choice
    assert sess.hist[0, LENGTHS[0]:LENGTHS[0] + 3].tolist() == FORCED[:3]
    sess.fork(0, 2)
    assert int(sess.constraint_state[2]) == int(sess.constraint_state[0]) == starts[2] + 3
    _run(sess)
    n = LENGTHS[0]
    assert sess.hist[2, n:n + len(FORCED) + 1].tolist() == FORCED + [EOS]
    assert torch.equal(sess.hist[2], sess.hist[0]) and sess.constraint_state[2] == sess.constraint_state[0]


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_speculative_session_equals_stream_session(tiny, automata, sampled):
    from quantizations_amd.generation import SpeculativeSession

    model = tiny[0]
    joint, starts = automata
    sampling = SAMPLING if sampled else None
    # stream 0: one forced choice whose tokens also stand in its prompt, so the prompt-lookup drafts are right
    ids = _prompts().clone()
    ids[0, 1:8] = torch.tensor(FORCED, device=DEV)
    kw = dict(constraint=joint, start=[starts[2], starts[0], -1], sampling=sampling, prompts=ids)
    one = _run(_open(model, **kw))
    spec = _run(_open(model, SpeculativeSession, draft_tokens=DRAFTS, sample=sampled, **kw))
    assert spec._graph is not None and spec._constraining
    assert _same(spec, one)
    assert one.sequences()[0][LENGTHS[0]:].tolist() == FORCED + [EOS]
    st = spec.stats()
    print("steps", st["steps"].tolist(), "tokens", st["tokens"].tolist())
    assert int(st["tokens"][0]) > int(st["steps"][0])            # the window's state walk was accepted through
    eager = _run(_open(model, SpeculativeSession, draft_tokens=DRAFTS, sample=sampled, graph=False, **kw))
    assert _same(eager, one)


def test_logit_bias_and_suppress_tokens(tiny):
    from quantizations_amd.generation import generate_ragged

    model = tiny[0]
    plain = _run(_open(model, logprobs=0))
    forced = _run(_open(model, logit_bias_slots=4, bias={77: 100.0}))
    for new in _new_tokens(forced):
        assert new == [77] * N
    # bans of tokens the plain run does not pick first: the same first token, and the log-probabilities
    # are those of the model's own row, not of the banned one
    absent = [t for t in range(200, 300) if t not in set(plain.hist.flatten().tolist())][:3]
    banned = _open(model, logprobs=0, logit_bias_slots=4, bias={absent[0]: float("-inf"), absent[1]: -5.0, absent[2]: -0.5})
    assert banned._constraining
    for b, n in enumerate(LENGTHS):
        assert banned.hist[b, n] == plain.hist[b, n]
        assert torch.equal(banned.logprobs[b, n].view(torch.int32), plain.logprobs[b, n].view(torch.int32))
    prompts = [_prompts()[b, :n] for b, n in enumerate(LENGTHS)]
    kw = dict(do_sample=True, generator=SEED, **SAMPLING)
    free = generate_ragged(model, prompts, 32, **kw)
    seen = sorted({t for seq, n in zip(free, LENGTHS) for t in seq[n:].tolist()})
    held = generate_ragged(model, prompts, 32, suppress_tokens=seen, **kw)
    for seq, n in zip(held, LENGTHS):
        assert seq.numel() == n + 32 and not set(seq[n:].tolist()) & set(seen)
    with pytest.raises(ValueError):
        forced.set_logit_bias(0, {1: 1.0, 2: 1.0, 3: 1.0, 4: 1.0, 5: 1.0})      # more entries than slots
    with pytest.raises(ValueError):
        forced.set_logit_bias(0, {1: float("inf")})


def _only(token):
    words = np.zeros((3, (V + 31) // 32), dtype=np.uint32)
    words[:, token >> 5] = np.uint32(1) << np.uint32(token & 31)
    return torch.from_numpy(words.view(np.int32))


def test_replay_follows_set_token_mask(tiny):
    from quantizations_amd.generation import SpeculativeSession, StreamSession

    model = tiny[0]
    sess = StreamSession(model, 3, max(LENGTHS) + N, graph=True)
    sess.set_token_mask(torch.full((3, (V + 31) // 32), -1, dtype=torch.int32))     # everything allowed
    sess.prefill(_prompts(), LENGTHS, max_new_tokens=N)
    plain = _open(model)
    assert torch.equal(sess.tok, plain.tok) and sess._constraining      # a mask of ones changes nothing
    sess.step()
    captured = sess._graph
    assert captured is not None
    for token in (123, 3210, 4095):
        sess.set_token_mask(_only(token))
        sess.step()
        torch.cuda.synchronize()
        assert sess.tok[:, 0].tolist() == [token] * 3 and sess._graph is captured
    sess.set_token_mask(None)
    sess.step()
    assert sess._graph is captured
    spec = SpeculativeSession(model, 3, max(LENGTHS) + N, draft_tokens=DRAFTS)
    with pytest.raises(ValueError, match="SpeculativeSession"):
        spec.set_token_mask(_only(5))


def test_enabling_after_a_neutral_capture_raises(tiny, automata):
    model = tiny[0]
    sess = _open(model, logit_bias_slots=4)
    sess.step()
    assert sess._graph is not None and not sess._constraining
    with pytest.raises(ValueError, match="without constrained decoding"):
        sess.set_logit_bias(0, {5: 1.0})
    with pytest.raises(ValueError, match="without a host mask"):
        sess.set_token_mask(_only(5))
    sess.set_logit_bias(0, {})                                  # an empty list is no change
    with pytest.raises(ValueError, match="constraint_start needs"):
        sess.admit(1, torch.tensor([1, 2, 3]), constraint_start=0)
    eager = _open(model, logit_bias_slots=4, graph=False)
    eager.step()
    eager.set_logit_bias(0, {5: 1.0})                           # nothing captured: free to change
    assert eager._constraining


def test_a_session_without_options_launches_neither_call(tiny, monkeypatch):
    from quantizations_amd import layer_ops
    from quantizations_amd.generation import SpeculativeSession, generate_ragged

    model = tiny[0]
    prompts = [_prompts()[b, :n] for b, n in enumerate(LENGTHS)]
    want = generate_ragged(model, prompts, N)

    def boom(*a, **k):
        raise AssertionError("a session without constraint options called a constrained-decoding launch")

    monkeypatch.setattr(layer_ops, "constrain_logits", boom)
    monkeypatch.setattr(layer_ops, "constraint_advance", boom)
    sess = _run(_open(model))
    assert not sess._constraining and sess.constraint_state is None and sess._pos0 is None
    for seq, w in zip(sess.sequences(), want):
        assert torch.equal(seq, w)
    spec = _run(_open(model, SpeculativeSession, draft_tokens=DRAFTS))
    assert not spec._constraining
    for seq, w in zip(spec.sequences(), want):
        assert torch.equal(seq, w)
    for seq, w in zip(generate_ragged(model, prompts, N), want):
        assert torch.equal(seq, w)
