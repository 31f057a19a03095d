"""GPU: SpeculativeSession(sample=True) and generate(..., prompt_lookup_sampling=True) on the tiny
random-init Llama and the Ngram / Null / Replay sessions of test_gpu_generation_speculative.py.

Every check is exact.  A token is a function of its logits row and of the uniform number of its
position, and every launch of the step gives a row the same bits wherever it sits, so the history must
not depend on the drafts: the n-gram drafter, the null drafter (M steps) and the replay drafter
(ceil(M / T) steps) leave the same tokens; graph equals eager; the same seed gives the same tokens and
another seed others; temperature 0 gives the default session's tokens.  There is no comparison with
the one-token sampled StreamSession: its launches differ from the window's in the last logit bits, and
on this near-flat vocabulary no honest margin around the CDF boundaries would leave most draws in
(DESIGN.md); layer_ops' per-row identity (test_gpu_verify_sample_step.py) and the greedy model tests
carry that ground."""
import math

import pytest
import torch
from test_gpu_generation_speculative import DRAFTS, LENGTHS, M, N, SENT, T, _build, _prompts, _sessions, _unprepare

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
SEED = 11
ONE = dict(temperature=0.8, top_k=50, top_p=0.9)
MIX = dict(temperature=[0.8, 0.0, 1.1], top_k=[50, 0, 7], top_p=[0.9, 1.0, 1.0])      # stream 1 is greedy
SETTINGS = {"one": ONE, "mix": MIX}


@pytest.fixture(scope="module")
def model():
    from quantizations_amd.generation import prepare_for_decode

    m = _build()
    prepare_for_decode(m)
    try:
        yield m
    finally:
        _unprepare(m)


def _open(model, cls, settings=ONE, seed=SEED, graph=True, known=None, sample=True, **prefill_kw):
    prefill_kw.setdefault("max_new_tokens", N)
    sess = cls(model, 3, max(LENGTHS) + N, draft_tokens=DRAFTS, graph=graph, sample=sample)
    if known is not None:
        sess.known = known
    if settings is not None:
        sess.set_sampling(**settings)
        sess.seed(seed)
    sess.hist.fill_(SENT)
    sess.prefill(_prompts(), LENGTHS, **prefill_kw)
    return sess


def _until_done(sess):
    n = 0
    while bool(sess.alive().any()):
        sess.step()
        n += 1
        assert n <= M
    torch.cuda.synchronize()
    return n


def _same(a, b):
    return torch.equal(a.hist, b.hist) and torch.equal(a.pos, b.pos) and torch.equal(a.live, b.live)


@pytest.mark.parametrize("which", list(SETTINGS))
def test_tokens_do_not_depend_on_the_drafter(model, which):
    Ngram, Null, Replay = _sessions()
    a = _open(model, Ngram, SETTINGS[which])
    assert not a._greedy_only
    n_a = _until_done(a)
    ids = _prompts()
    for r, n in enumerate(LENGTHS):      # the prompt, N new tokens, nothing after
        assert torch.equal(a.hist[r, :n], ids[r, :n]) and bool((a.hist[r, n:n + N] != SENT).all())
        assert bool((a.hist[r, n + N:] == SENT).all())
    assert a.pos.tolist() == [n + N - 1 for n in LENGTHS]
    assert len(set(a.hist[0, LENGTHS[0]:LENGTHS[0] + N].tolist())) > 3
    null = _open(model, Null, SETTINGS[which])
    n_null = _until_done(null)
    replay = _open(model, Replay, SETTINGS[which], known=a._hist_full.clone())
    n_replay = _until_done(replay)
    assert _same(null, a), "null"
    assert _same(replay, a), "replay"
    assert n_replay == math.ceil(M / T) and n_null == M and math.ceil(M / T) <= n_a <= M, (n_replay, n_null, n_a)
    assert replay.stats()["steps"].tolist() == [math.ceil(M / T)] * 3 and replay.stats()["tokens"].tolist() == [M] * 3
    assert null.stats()["steps"].tolist() == [M] * 3 and null.stats()["tokens"].tolist() == [M] * 3
    if which == "mix":                   # the greedy stream among sampled ones: the default session's tokens
        g = _open(model, Ngram, None, sample=False)
        _until_done(g)
        assert torch.equal(g.hist[1], a.hist[1]) and not torch.equal(g.hist[0], a.hist[0])


def test_graph_equals_eager(model):
    Ngram, _, Replay = _sessions()
    a = _open(model, Ngram, graph=True)
    b = _open(model, Ngram, graph=False)
    _until_done(a), _until_done(b)
    assert a._graph is not None and b._graph is None
    assert _same(a, b)
    c = _open(model, Replay, graph=True, known=a._hist_full.clone())
    d = _open(model, Replay, graph=False, known=a._hist_full.clone())
    assert _until_done(c) == _until_done(d) == math.ceil(M / T)
    assert _same(c, a) and _same(d, a) and torch.equal(c.accepted, d.accepted)


def test_seeds(model):
    Ngram, _, _ = _sessions()
    a, b, c = _open(model, Ngram, seed=SEED), _open(model, Ngram, seed=SEED), _open(model, Ngram, seed=SEED + 1)
    for s in (a, b, c):
        _until_done(s)
    assert _same(a, b)
    assert all(not torch.equal(a.hist[r], c.hist[r]) for r in range(3))
    assert torch.equal(a.uniform, b.uniform) and not torch.equal(a.uniform, c.uniform)
    gen = torch.Generator(device=DEV).manual_seed(SEED)
    d = _open(model, Ngram, seed=gen)
    _until_done(d)
    assert _same(a, d), "an int seed is a generator on the session's device"


def test_temperature_0_gives_the_default_sessions_tokens(model):
    Ngram, _, _ = _sessions()
    plain = _open(model, Ngram, None, sample=False)
    cold = _open(model, Ngram, dict(temperature=0.0, top_k=50, top_p=0.9))
    assert cold._greedy_only
    assert _until_done(plain) == _until_done(cold)
    assert _same(plain, cold)
    assert cold._graph is not None
    with pytest.raises(ValueError, match="greedy-only"):        # the captured step holds the greedy verify launch
        cold.set_sampling(temperature=0.7)
    with pytest.raises(ValueError, match="greedy only"):        # the default session refuses as it always did
        plain.set_sampling(temperature=0.7)
    cold.set_sampling(temperature=0.0, top_k=3)


def test_a_retired_row_is_readmitted_under_the_first_graph(model):
    Ngram, _, _ = _sessions()
    undisturbed = _open(model, Ngram)
    _until_done(undisturbed)
    newcomer = torch.randint(0, 4096, (6,), generator=torch.Generator().manual_seed(8))

    def scenario(graph):
        sess = _open(model, Ngram, graph=graph, max_new_tokens=[N, 4, N])      # stream 1 retires by its limit
        for _ in range(3):
            sess.step()                                                        # at least 3 tokens each
        captured = sess._graph
        assert (captured is not None) == graph and sess.alive().tolist() == [True, False, True]
        assert sess.pos[1].item() == LENGTHS[1] + 3
        assert torch.equal(sess.hist[1, :LENGTHS[1] + 4], undisturbed.hist[1, :LENGTHS[1] + 4])
        sess.admit(1, newcomer, max_new_tokens=7)
        assert sess.alive().tolist() == [True, True, True] and sess.pos[1].item() == 6
        _until_done(sess)
        assert sess._graph is captured, "no recapture"
        return sess

    sess = scenario(True)
    for r in (0, 2):
        assert torch.equal(sess.hist[r], undisturbed.hist[r])
    assert sess.pos.tolist() == [LENGTHS[0] + N - 1, 6 + 7 - 1, LENGTHS[2] + N - 1]
    assert torch.equal(sess.hist[1, :6].cpu(), newcomer) and bool((sess.hist[1, 6:13] != SENT).all())
    assert bool((sess.hist[1, 13:] == SENT).all())
    assert torch.equal(sess.hist, scenario(False).hist)


def test_generate_with_prompt_lookup_sampling(model):
    from quantizations_amd.generation import generate, generate_ragged

    ids = _prompts()
    n_new = 40
    kw = dict(do_sample=True, generator=SEED, prompt_lookup_num_tokens=DRAFTS, prompt_lookup_sampling=True, **ONE)
    free = generate(model, ids, n_new, **kw)
    Sx = ids.shape[1]
    assert free.shape == (3, Sx + n_new) and free.dtype == torch.int64 and torch.equal(free[:, :Sx], ids)
    assert bool(((free >= 0) & (free < 4096)).all())
    assert torch.equal(free, generate(model, ids, n_new, **kw)), "reproducible from an int seed"
    assert torch.equal(free, generate(model, ids, n_new, graph=False, max_matching_ngram_size=1, **kw))
    assert not torch.equal(free, generate(model, ids, n_new, **dict(kw, generator=SEED + 1)))
    assert not torch.equal(free, generate(model, ids, n_new, prompt_lookup_num_tokens=DRAFTS)), "it samples"
    with pytest.raises(ValueError, match="do_sample.*prompt_lookup_sampling"):
        generate(model, ids, n_new, do_sample=True, prompt_lookup_num_tokens=DRAFTS)
    # the flag alone changes nothing: without do_sample the run is the greedy speculative one
    assert torch.equal(generate(model, ids, n_new, prompt_lookup_num_tokens=DRAFTS, prompt_lookup_sampling=True),
                       generate(model, ids, n_new, prompt_lookup_num_tokens=DRAFTS))
    # an EOS the streams meet at different places: the plain form's layout (n a multiple of 16, EOS fill)
    eos = int(free[0, Sx + 5])
    out = generate(model, ids, n_new, eos_token_id=eos, **kw)
    hits = [(free[b, Sx:] == eos).nonzero() for b in range(3)]
    ends = [int(h[0]) + 1 if h.numel() else None for h in hits]
    n = n_new if None in ends else min(n_new, -(-max(ends) // 16) * 16)
    assert out.shape == (3, Sx + n)
    for b, e in enumerate(ends):
        want = free[b, :Sx + n].clone()
        if e is not None:
            want[Sx + e:] = eos
        assert torch.equal(out[b], want), b
    # the ragged twin: each prompt's own length, ending on its EOS
    prompts = [ids[b, :n] for b, n in enumerate(LENGTHS)]
    rfree = generate_ragged(model, prompts, n_new, **kw)
    assert [t.numel() for t in rfree] == [n + n_new for n in LENGTHS]
    assert all(torch.equal(t[:n], p) for t, p, n in zip(rfree, prompts, LENGTHS))
    again = generate_ragged(model, prompts, n_new, **kw)
    assert all(torch.equal(x, y) for x, y in zip(rfree, again)), "reproducible from an int seed"
    eos = int(rfree[0][LENGTHS[0] + 5])
    rout = generate_ragged(model, prompts, n_new, eos_token_id=eos, **kw)
    for b, n in enumerate(LENGTHS):
        hit = (rfree[b][n:] == eos).nonzero()
        want = rfree[b][:n + int(hit[0]) + 1] if hit.numel() else rfree[b]
        assert torch.equal(rout[b], want), b
    assert rout[0].numel() <= LENGTHS[0] + 6 and rout[0][-1] == eos
    with pytest.raises(ValueError, match="do_sample.*prompt_lookup_sampling"):
        generate_ragged(model, prompts, n_new, do_sample=True, prompt_lookup_num_tokens=DRAFTS)


def test_a_two_adapter_bank_run_is_drafter_independent(model):
    import quantizations_amd as qa

    Ngram, Null, Replay = _sessions()
    g = torch.Generator().manual_seed(17)
    slots = torch.full((16,), -1, dtype=torch.int32)
    slots[:3] = torch.tensor([0, 1, -1], dtype=torch.int32)
    slots = slots.to(DEV)
    lins = [m for m in model.modules() if isinstance(m, qa.Linear4bit)]
    assert len(lins) == 14
    plain = _open(model, Ngram)
    _until_done(plain)
    try:
        for m in lins:
            ents = [((torch.randn(8, m.in_features, generator=g) * 0.02).half(),
                     (torch.randn(m.out_features, 8, generator=g) * (0.25 / math.sqrt(8))).half(), 1.0) for _ in range(2)]
            m.set_adapter_bank(ents, slots)
        a = _open(model, Ngram)
        _until_done(a)
        null = _open(model, Null)
        n_null = _until_done(null)
        replay = _open(model, Replay, known=a._hist_full.clone())
        n_replay = _until_done(replay)
        assert _same(null, a) and _same(replay, a)
        assert n_replay == math.ceil(M / T) and n_null == M
        assert not torch.equal(a.hist[0], plain.hist[0]) and not torch.equal(a.hist[1], plain.hist[1])
    finally:
        for m in lins:
            m.clear_adapter_bank()
