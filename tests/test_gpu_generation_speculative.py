"""GPU: quantizations_amd.generation.SpeculativeSession and generate(..., prompt_lookup_num_tokens=...)
on the tiny random-init Llama of test_gpu_generation_streams.py (2 layers, hidden 256, vocab 4096,
Linear4bit projections), built afresh here: a prepared model and an unfused twin with the same weights.

Exact checks.  Drafts are hints: the tokens of a run must not depend on them.  Three drafters run the
same ragged prompts -- the n-gram drafter, a null drafter (draft = newest token + 1: it matches by
chance only) and a replay drafter (a test subclass whose _draft gathers the continuation the first run
produced, so every draft is right) -- and must leave the same history.  With M = N - 1 tokens per stream
left to the steps (prefill picks the first), the replay run takes ceil(M / T) steps and the null run M,
and stats() agrees.  They rest on every launch of the step giving a token the same bits whichever
row it sits in: the multi-token 4-bit kernel (MFMA columns are independent), the attention
(test_gpu_decode_attention_verify.py) and the library GEMM behind the lm_head, which nobody had
measured; the exact checks here are that measurement.  Graph equals eager; admit() into a retired
row under the first graph; stop tokens; generate / generate_ragged; one run with a two-adapter bank.

One check cannot be exact: speculative tokens against the unfused model, held teacher-forced exactly
as test_gpu_generation_streams.py holds the ragged run.  `tol` is twice the largest absolute logit
difference between the parent's StreamSession decode path (per-stream positions, one token per stream:
code this file's subject does not change) and the unfused model, teacher-forced over the same tokens
on this same model, measured in the fixture.  The token must be the strict argmax wherever the
unfused model's top-two gap is at least tol, and at least 90 % of positions must have such a gap (the
prompt seed, 3, is the streams file's, chosen there so that the unfused model alone meets that).
Measured on an MI355X: d = 0.001343, tol = 0.002686; the unfused model has a top-two gap of at least
tol on 67 of the 72 generated positions (93 %); the largest shortfall of a picked token below its
position's maximum was 0.00098; the n-gram drafter took 8, 12 and 12 steps for the 23 tokens of the
three streams (a random-init model repeats itself a little), the replay drafter 6, the null drafter 23."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
S, N = 8, 24
M = N - 1                 # tokens per stream the steps emit: prefill picks the first
LENGTHS = [8, 3, 5]
SENT = -5
DRAFTS = 3
T = DRAFTS + 1


def _unprepare(model):
    from quantizations_amd import integration as I

    I.unfuse_lm_head(model)
    I.unfuse_decode_glue(model)
    I.unfuse_prenorm(model)
    I.unfuse_layer_ops(model)
    I.unfuse_projection_groups(model)
    model.__dict__.pop("_qz_prepared", None)


def _build():
    from transformers import LlamaConfig, LlamaForCausalLM

    from quantizations_amd.integration import replace_with_bnb_linear

    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=4096, max_position_embeddings=256, rope_theta=500000.0,
                      eos_token_id=None, bos_token_id=None, pad_token_id=None)
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).half().to(DEV).eval()
    replace_with_bnb_linear(model, modules_to_not_convert=["lm_head"], quant_type="nf4", compute_dtype=torch.float32)
    return model


def _prompts():
    return torch.randint(0, 4096, (3, max(LENGTHS)), generator=torch.Generator().manual_seed(3)).to(DEV)


def _stream_path_logits(model, ids, lengths, n):
    """The parent's per-stream decode path, greedy and eager: (sequences, the logits [B, n - 1, V] that
    picked each stream's tokens 2..n)."""
    from quantizations_amd.generation import StreamSession

    sess = StreamSession(model, len(lengths), max(lengths) + n, graph=False)
    sess.prefill(ids, lengths, max_new_tokens=n)
    logits = []
    with torch.inference_mode():
        for _ in range(n - 1):
            lo = model(input_ids=sess.tok, past_key_values=sess.cache, position_ids=sess._pos_ids,
                       attention_mask=sess._mask, use_cache=True, _qz_stream_pos=sess.pos).logits[:, -1]
            logits.append(lo.float().clone())
            sess._pick(lo)
    return sess.sequences(), torch.stack(logits, 1)


@pytest.fixture(scope="module")
def tiny():
    """(prepared model, unfused twin, prompts [3, max(LENGTHS)], tol)"""
    from quantizations_amd.generation import prepare_for_decode

    ref = _build()
    model = _build()
    ids = _prompts()
    prepare_for_decode(model)
    try:
        seqs, lo = _stream_path_logits(model, ids, LENGTHS, N)
        d = 0.0
        with torch.inference_mode():
            for b, n in enumerate(LENGTHS):
                want = ref(input_ids=seqs[b][None]).logits[0, n:n + N - 1].float()   # picks tokens n + 1 .. n + N - 1
                d = max(d, float((lo[b] - want).abs().max()))
        print(f"StreamSession decode path vs unfused model: largest |logit difference| d = {d:.6f}, tol = {2 * d:.6f}")
        assert 0 < d < 1.0, d    # a sanity bracket around the measurement, not the bar
        yield model, ref, ids, 2 * d
    finally:
        _unprepare(model)


def _sessions():
    from quantizations_amd.generation import SpeculativeSession

    class Null(SpeculativeSession):
        def _draft(self):
            super()._draft()                                     # pos_ids
            self.tok[:, 1:] = (self.tok[:, :1] + 1) % 4096

    class Replay(SpeculativeSession):
        known = None                                             # [B, width]: the sequences to come

        def _draft(self):
            ar = torch.arange(self.T, device=self.device)
            self.pos_ids.copy_(self.pos[:, None] + ar[None, :])
            nxt = (self.pos_ids[:, 1:]).clamp(max=self.known.shape[1] - 1)
            # past a stream's end `known` holds the SENT fill: a draft must still be a token id the
            # embedding can look up, whatever becomes of it
            self.tok[:, 1:] = self.known.gather(1, nxt).clamp(min=0)

    return SpeculativeSession, Null, Replay


def _run(sess, steps):
    for _ in range(steps):
        sess.step()
    torch.cuda.synchronize()


def _ragged(model, cls, graph=True, steps=M, known=None, **prefill_kw):
    prefill_kw.setdefault("max_new_tokens", N)
    ids = _prompts()
    sess = cls(model, 3, max(LENGTHS) + N, draft_tokens=DRAFTS, graph=graph)
    if known is not None:
        sess.known = known
    sess.hist.fill_(SENT)
    sess.prefill(ids, LENGTHS, **prefill_kw)
    _run(sess, steps)
    return sess, ids


def _steps_until_done(model, cls, known=None, **prefill_kw):
    """Step one at a time until no stream is live; (session, steps taken)."""
    sess, _ = _ragged(model, cls, steps=0, known=known, **prefill_kw)
    n = 0
    while bool(sess.alive().any()):
        sess.step()
        n += 1
        assert n <= M
    return sess, n


def test_tokens_do_not_depend_on_the_drafter(tiny):
    model = tiny[0]
    Ngram, Null, Replay = _sessions()
    a, ids = _ragged(model, Ngram)
    for r, n in enumerate(LENGTHS):      # the prompt, N new tokens, nothing after
        assert torch.equal(a.hist[r, :n], ids[r, :n]) and bool((a.hist[r, n:n + N] != SENT).all())
        assert bool((a.hist[r, n + N:] == SENT).all())
    assert a.pos.tolist() == [n + N - 1 for n in LENGTHS] and not bool(a.alive().any())
    assert len(set(a.hist[0, LENGTHS[0]:].tolist())) > 3      # not a constant
    known = a._hist_full.clone()
    null, n_null = _steps_until_done(model, Null)
    replay, n_replay = _steps_until_done(model, Replay, known=known)
    for other, what in ((null, "null"), (replay, "replay")):
        assert torch.equal(other.hist, a.hist), what
        assert torch.equal(other.pos, a.pos) and torch.equal(other.live, a.live), what
    assert n_replay == math.ceil(M / T) and n_null == M, (n_replay, n_null)
    st = replay.stats()
    assert st["steps"].tolist() == [math.ceil(M / T)] * 3 and st["tokens"].tolist() == [M] * 3
    st = null.stats()
    assert st["steps"].tolist() == [M] * 3 and st["tokens"].tolist() == [M] * 3
    st = a.stats()
    assert st["tokens"].tolist() == [M] * 3 and all(math.ceil(M / T) <= s <= M for s in st["steps"].tolist())
    print("n-gram drafter steps per stream", st["steps"].tolist(), "of", M)


def test_graph_equals_eager(tiny):
    model = tiny[0]
    Ngram, _, Replay = _sessions()
    a, _ = _ragged(model, Ngram, graph=True)
    b, _ = _ragged(model, Ngram, graph=False)
    assert a._graph is not None and b._graph is None
    assert torch.equal(a.hist, b.hist) and torch.equal(a.pos, b.pos) and torch.equal(a.live, b.live)
    c, _ = _ragged(model, Replay, graph=True, steps=math.ceil(M / T), known=a._hist_full.clone())
    d, _ = _ragged(model, Replay, graph=False, steps=math.ceil(M / T), known=a._hist_full.clone())
    assert torch.equal(c.hist, a.hist) and torch.equal(d.hist, a.hist)
    assert torch.equal(c.accepted, d.accepted)


def test_speculative_tokens_against_the_unfused_model(tiny):
    model, ref, _, tol = tiny
    Ngram, _, _ = _sessions()
    sess, ids = _ragged(model, Ngram)
    seqs = sess.sequences()
    assert [t.numel() for t in seqs] == [n + N for n in LENGTHS]
    clear = total = 0
    for b, seq in enumerate(seqs):
        n = LENGTHS[b]
        assert torch.equal(seq[:n], ids[b, :n])
        with torch.inference_mode():
            lo = ref(input_ids=seq[None]).logits[0, n - 1:n + N - 1].float()      # the logits that pick seq[n:]
        top2 = lo.topk(2, dim=-1).values
        picked = lo.gather(1, seq[n:, None])[:, 0]
        gap = top2[:, 0] - top2[:, 1]
        print(b, "largest shortfall", float((top2[:, 0] - picked).max()), "smallest gap", float(gap.min()), "tol", tol)
        assert bool((top2[:, 0] - picked <= tol).all()), (b, (top2[:, 0] - picked).max())
        sure = gap >= tol
        assert torch.equal(seq[n:][sure], lo.argmax(-1)[sure])
        clear += int(sure.sum())
        total += N
    print("top-two gap >= tol on", clear, "of", total, "generated positions")
    assert clear >= 0.9 * total


def test_a_retired_row_is_readmitted_under_the_first_graph(tiny):
    model = tiny[0]
    Ngram, _, _ = _sessions()
    undisturbed, ids = _ragged(model, Ngram)
    newcomer = torch.randint(0, 4096, (6,), generator=torch.Generator().manual_seed(8))

    def scenario(graph):
        sess = Ngram(model, 3, max(LENGTHS) + N, draft_tokens=DRAFTS, graph=graph)
        sess.hist.fill_(SENT)
        sess.prefill(ids, LENGTHS, max_new_tokens=[N, 4, N])       # stream 1 retires by its limit
        _run(sess, 3)                                              # at least 3 tokens each: stream 1 is done
        captured = sess._graph
        assert (captured is not None) == graph and sess.alive().tolist() == [True, False, True]
        assert sess.pos[1].item() == LENGTHS[1] + 3 and bool((sess.hist[1, LENGTHS[1] + 4:] == SENT).all())
        assert torch.equal(sess.hist[1, :LENGTHS[1] + 4], undisturbed.hist[1, :LENGTHS[1] + 4])
        sess.admit(1, newcomer, max_new_tokens=7)
        assert sess.alive().tolist() == [True, True, True] and sess.pos[1].item() == 6
        _run(sess, M)
        assert sess._graph is captured, "no recapture"
        return sess

    sess = scenario(True)
    for r in (0, 2):
        assert torch.equal(sess.hist[r], undisturbed.hist[r])
    assert sess.pos.tolist() == [LENGTHS[0] + N - 1, 6 + 7 - 1, LENGTHS[2] + N - 1]
    assert torch.equal(sess.hist[1, :6].cpu(), newcomer) and bool((sess.hist[1, 6:13] != SENT).all())
    assert bool((sess.hist[1, 13:] == SENT).all())
    assert torch.equal(sess.hist, scenario(False).hist)


def test_a_stream_stops_after_writing_its_stop_token(tiny):
    model = tiny[0]
    Ngram, _, Replay = _sessions()
    free, _ = _ragged(model, Ngram)
    n = LENGTHS[1]
    stop = int(free.hist[1, n + 5])
    first = int((free.hist[1, n:] == stop).nonzero()[0])
    # the replay drafter accepts whole windows: the stop token sits in the middle of an accepted run
    for cls in (Ngram, Replay):
        sess, _ = _ragged(model, cls, known=free._hist_full.clone(), stop=[-1, stop, -1])
        assert sess.alive().tolist() == [False, False, False]
        assert sess.pos.tolist() == [LENGTHS[0] + N - 1, n + first, LENGTHS[2] + N - 1]
        assert torch.equal(sess.hist[1, :n + first + 1], free.hist[1, :n + first + 1]) and sess.hist[1, n + first] == stop
        assert bool((sess.hist[1, n + first + 1:] == SENT).all())
        for r in (0, 2):
            assert torch.equal(sess.hist[r], free.hist[r])


def test_generate_with_prompt_lookup(tiny):
    from quantizations_amd.generation import generate, generate_ragged

    model = tiny[0]
    ids = _prompts()
    n_new = 40
    plain = generate(model, ids, n_new)
    free = generate(model, ids, n_new, prompt_lookup_num_tokens=DRAFTS)
    assert free.shape == plain.shape == (3, ids.shape[1] + n_new) and free.dtype == torch.int64
    assert torch.equal(free[:, :ids.shape[1]], ids)
    assert torch.equal(free, generate(model, ids, n_new, prompt_lookup_num_tokens=DRAFTS, max_matching_ngram_size=1,
                                      graph=False))
    # an EOS the streams meet at different places: the plain form's layout (n a multiple of 16, EOS fill)
    Sx = ids.shape[1]
    eos = int(free[0, Sx + 5])
    out = generate(model, ids, n_new, eos_token_id=eos, prompt_lookup_num_tokens=DRAFTS)
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
    rfree = generate_ragged(model, prompts, n_new, prompt_lookup_num_tokens=DRAFTS)
    assert [t.numel() for t in rfree] == [n + n_new for n in LENGTHS]
    assert all(torch.equal(t[:n], p) for t, p, n in zip(rfree, prompts, LENGTHS))
    eos = int(rfree[0][LENGTHS[0] + 5])
    rout = generate_ragged(model, prompts, n_new, eos_token_id=eos, prompt_lookup_num_tokens=DRAFTS)
    for b, n in enumerate(LENGTHS):
        hit = (rfree[b][n:] == eos).nonzero()
        want = rfree[b][:n + int(hit[0]) + 1] if hit.numel() else rfree[b]
        assert torch.equal(rout[b], want), b
    assert rout[0].numel() <= LENGTHS[0] + 6 and rout[0][-1] == eos
    assert [t.numel() for t in generate_ragged(model, prompts, n_new)] == [t.numel() for t in rfree]


def test_a_two_adapter_bank_run_is_drafter_independent(tiny):
    import quantizations_amd as qa

    model = tiny[0]
    Ngram, Null, Replay = _sessions()
    g = torch.Generator().manual_seed(17)
    slots = torch.full((16,), -1, dtype=torch.int32)
    slots[:3] = torch.tensor([0, 1, -1], dtype=torch.int32)
    slots = slots.to(DEV)
    lins = [m for m in model.modules() if isinstance(m, qa.Linear4bit)]
    assert len(lins) == 14
    try:
        for m in lins:
            ents = [((torch.randn(8, m.in_features, generator=g) * 0.02).half(),
                     (torch.randn(m.out_features, 8, generator=g) * (0.25 / math.sqrt(8))).half(), 1.0) for _ in range(2)]
            m.set_adapter_bank(ents, slots)
        a, _ = _ragged(model, Ngram)
        plain, _ = _ragged_without_bank(model, lins, Ngram)
        null, _ = _steps_until_done(model, Null)
        replay, n_replay = _steps_until_done(model, Replay, known=a._hist_full.clone())
        assert torch.equal(null.hist, a.hist) and torch.equal(replay.hist, a.hist)
        assert n_replay == math.ceil(M / T)
        assert not torch.equal(a.hist[0], plain.hist[0]) and not torch.equal(a.hist[1], plain.hist[1])
    finally:
        for m in lins:
            m.clear_adapter_bank()


def _ragged_without_bank(model, lins, cls):
    """The same run with every bank's slots at -1 (no row on an adapter)."""
    banks = [m.adapter_bank for m in lins]
    slots = banks[0].slots
    keep = slots.clone()
    slots.fill_(-1)
    try:
        return _ragged(model, cls)
    finally:
        slots.copy_(keep)


def test_what_the_session_generate_and_the_layer_refuse(tiny):
    from quantizations_amd.generation import SpeculativeSession, generate, generate_ragged

    model, ref, ids, _ = tiny
    with pytest.raises(ValueError, match="prepare_for_decode"):
        SpeculativeSession(ref, 3, 16)
    with pytest.raises(ValueError, match="rows per step"):
        SpeculativeSession(model, 5, 32, draft_tokens=3)         # 20 rows
    with pytest.raises(ValueError):
        SpeculativeSession(model, 1, 32, draft_tokens=0)
    with pytest.raises(ValueError):
        SpeculativeSession(model, 1, 32, ngram=5)
    sess = SpeculativeSession(model, 3, S + 8)
    with pytest.raises(ValueError, match="greedy only"):
        sess.set_sampling(temperature=0.7)
    sess.set_sampling(temperature=0.0)
    with pytest.raises(ValueError):
        sess.step()                                              # prefill first
    with pytest.raises(ValueError, match="do_sample"):
        generate(model, ids, 4, do_sample=True, prompt_lookup_num_tokens=3)
    with pytest.raises(ValueError, match="do_sample"):
        generate_ragged(model, [ids[0]], 4, do_sample=True, prompt_lookup_num_tokens=3)
    with pytest.raises(ValueError, match="max_matching_ngram_size"):
        generate(model, ids, 4, max_matching_ngram_size=2)
    with pytest.raises(ValueError, match="rows per step"):
        generate(model, ids, 4, prompt_lookup_num_tokens=7)      # 3 streams x 8 rows
    sess.prefill(ids, [S] * 3)
    pos = torch.tensor([3, 1, 2], device=DEV)
    with torch.inference_mode(), pytest.raises(ValueError, match="_qz_verify_pos"):
        model(input_ids=ids[:, :1], past_key_values=sess.cache, position_ids=pos.view(3, 1), use_cache=True,
              _qz_verify_pos=pos)                                # one token per stream: the streams launch's case
    with torch.inference_mode(), pytest.raises(ValueError, match="exclude"):
        model(input_ids=ids[:, :2], past_key_values=sess.cache, position_ids=pos.view(3, 1) + torch.arange(2, device=DEV),
              use_cache=True, _qz_verify_pos=pos, _qz_stream_pos=pos)
