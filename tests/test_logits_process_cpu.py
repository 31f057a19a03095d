"""CPU: the logits processors' rules.  tests/logits_process_reference.py is pinned to transformers'
RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and MinNewTokensLengthLogitsProcessor
(bit-equal after the one rounding, over all 65536 fp16 and all 65536 bf16 patterns as logits), the
presence / frequency counts to hand-written cases, layer_ops' composed route to the reference, and the
sessions' plumbing to what the options promise on the fp32 tiny Llama of test_generation_cpu.py."""
import numpy as np
import pytest
import torch

import logits_process_reference as R
from test_generation_cpu import model  # noqa: F401  (the module-scoped tiny fp32 Llama)

TORCH_DT = {R.F16: torch.float16, R.BF16: torch.bfloat16}


def _as_torch(bits, dt):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint16).view(np.int16).copy()).view(TORCH_DT[dt])


def _bits_of(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def _same(got, want, dt, what):
    """Bit equality; where both are NaN the payload is not compared (IEEE leaves it open and the
    reference keeps the logit's own)."""
    g, w = R.to_f32(got, dt), R.to_f32(want, dt)
    both_nan = np.isnan(g) & np.isnan(w)
    bad = (np.asarray(got) != np.asarray(want)) & ~both_nan
    assert not bad.any(), (what, int(bad.sum()), np.nonzero(bad)[0][:8].tolist())


@pytest.mark.parametrize("dt", [R.F16, R.BF16])
@pytest.mark.parametrize("rp", [0.5, 1.0000001, 1.3, 3.0, 1e4])
def test_repetition_rule_is_transformers_on_every_pattern(dt, rp):
    from transformers import RepetitionPenaltyLogitsProcessor

    V = 65536
    bits = np.arange(V, dtype=np.uint16)
    scores = _as_torch(bits, dt).float()[None, :]          # transformers processes fp32 scores
    ids = torch.arange(V)[None, :]
    want = RepetitionPenaltyLogitsProcessor(penalty=rp)(ids, scores.clone())[0].to(TORCH_DT[dt])
    got = R.process_row(bits, dt, V, list(range(V)), rp=rp)
    _same(got, _bits_of(want), dt, (dt, rp))
    nan = np.isnan(R.to_f32(bits, dt))
    assert np.array_equal(got[nan], bits[nan])              # a NaN logit keeps its bits
    # every other token of a history that holds half the vocabulary stays as it was
    half = R.process_row(bits, dt, V, list(range(0, V, 2)), rp=rp)
    assert np.array_equal(half[1::2], bits[1::2]) and np.array_equal(half[0::2], got[0::2])


@pytest.mark.parametrize("g", [1, 2, 3, 4, 5])
def test_no_repeat_ngram_rule_is_transformers(g):
    from transformers import NoRepeatNGramLogitsProcessor

    rng = np.random.default_rng(g)
    proc = NoRepeatNGramLogitsProcessor(g)
    V = 4
    for trial in range(200):
        n = int(rng.integers(1, 24))
        h = rng.integers(0, V, n).tolist()
        scores = torch.zeros((1, V))
        want = torch.isneginf(proc(torch.tensor([h]), scores)[0]).numpy()
        got = R.process_row(np.zeros(V, dtype=np.uint16), R.F16, V, h, ngram=g) == R.NEG_INF[R.F16]
        assert np.array_equal(got, want), (g, h, got, want)


def test_min_new_tokens_rule_is_transformers():
    from transformers import MinNewTokensLengthLogitsProcessor

    V, eos = 16, 5
    for prompt_len in (0, 3):
        for m in (0, 1, 4):
            proc = MinNewTokensLengthLogitsProcessor(prompt_len, m, eos)
            for n in range(max(prompt_len, 1), prompt_len + 7):
                h = [1] * n
                want = torch.isneginf(proc(torch.tensor([h]), torch.zeros((1, V)))[0]).numpy()
                got = R.process_row(np.zeros(V, dtype=np.uint16), R.BF16, V, h, min_new=m, prompt_len=prompt_len,
                                    eos=eos) == R.NEG_INF[R.BF16]
                assert np.array_equal(got, want), (prompt_len, m, n)
    assert (R.process_row(np.zeros(V, dtype=np.uint16), R.F16, V, [1], min_new=3, eos=-1) == 0).all()
    assert (R.process_row(np.zeros(V, dtype=np.uint16), R.F16, V, [1], min_new=3, eos=V) == 0).all()


def test_order_is_repetition_then_ngram_then_min_length():
    from transformers import (MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                              RepetitionPenaltyLogitsProcessor)

    V = 8
    h = [1, 2, 3, 1, 2]
    z = torch.tensor([[0.5, -1.25, 2.0, 3.0, -0.75, 1.5, 0.25, -2.0]], dtype=torch.float16)
    s = z.float()
    for proc in (RepetitionPenaltyLogitsProcessor(1.3), NoRepeatNGramLogitsProcessor(3),
                 MinNewTokensLengthLogitsProcessor(2, 9, 6)):
        s = proc(torch.tensor([h]), s)
    got = R.process_row(_bits_of(z[0]), R.F16, V, h, rp=1.3, ngram=3, min_new=9, prompt_len=2, eos=6)
    assert np.array_equal(got, _bits_of(s[0].half()))
    assert got[3] == R.NEG_INF[R.F16] and got[6] == R.NEG_INF[R.F16]    # 3 carries a penalty too: banned wins


def test_presence_and_frequency_count_generated_tokens_only():
    V = 8
    z = np.array([1.0, 2.0, -3.0, 4.0, 0.5, 0.0, -1.0, 8.0], dtype=np.float32)
    bits = z.astype(np.float16).view(np.uint16)
    h = [0, 1, 1, 2, 3, 3, 3, 1, 9, -1]          # the prompt is h[:4]; 9 and -1 are outside the vocabulary
    got = R.to_f32(R.process_row(bits, R.F16, V, h, pp=0.5, fp=0.25, prompt_len=4), R.F16)
    want = z.copy()
    want[3] = 4.0 - 0.25 * 3 - 0.5                # three generated occurrences
    want[1] = 2.0 - 0.25 * 1 - 0.5                # two in the prompt do not count, one generated does
    assert np.array_equal(got, want)              # tokens 0 and 2 occur in the prompt only: untouched
    # prompt_len = 0 counts everything; prompt_len >= n counts nothing
    all_ = R.to_f32(R.process_row(bits, R.F16, V, h, pp=0.5, fp=0.25, prompt_len=0), R.F16)
    assert all_[1] == 2.0 - 0.75 - 0.5 and all_[0] == 1.0 - 0.25 - 0.5 and all_[2] == -3.0 - 0.25 - 0.5
    for pl in (len(h), len(h) + 5):
        assert np.array_equal(R.process_row(bits, R.F16, V, h, pp=0.5, fp=0.25, prompt_len=pl), bits)
    # repetition applies to prompt tokens as well, once however often the token occurs, before the others
    both = R.to_f32(R.process_row(bits, R.F16, V, h, rp=2.0, pp=0.5, fp=0.25, prompt_len=4), R.F16)
    assert both[0] == 0.5 and both[2] == -6.0 and both[1] == 1.0 - 0.25 - 0.5 and both[3] == 2.0 - 0.75 - 0.5
    assert both[4] == 0.5 and both[7] == 8.0


def _window(dt, seed, B=3, T=4, V=40, H=30):
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 65536, (B * T, V + 3)).astype(np.uint16)
    hist = rng.integers(-1, 9, (B, H))
    pos = rng.integers(0, H, B)
    tok = rng.integers(0, 9, (B, T))
    tok[:, 0] = hist[np.arange(B), pos]
    par = dict(rp=[1.3, 1.0, 0.5][:B], pp=[0.5, 0.0, -2.0][:B], fp=[2.0, 0.0, 0.5][:B], ngram=[2, 0, 1][:B],
               min_new=[3, 0, 50][:B], prompt_len=[int(pos[0]), 0, 4][:B], eos=[7, 2, V + 3][:B])
    return bits, hist, pos, tok, par


@pytest.mark.parametrize("dt", [R.F16, R.BF16, "fp32"])
@pytest.mark.parametrize("T", [1, 4])
def test_composed_route_equals_reference(dt, T):
    from quantizations_amd.layer_ops import process_logits

    V = 40
    bits, hist, pos, tok, par = _window(R.F16 if dt == "fp32" else dt, 11 + T, T=T, V=V)
    if dt == "fp32":   # fp32 logits that hold fp16 values: the rounding is the identity, the rules the same
        finite = np.where(np.isnan(R.to_f32(bits, R.F16)), np.uint16(0x3C00), bits)
        logits = _as_torch(finite, R.F16).float()
        bits = finite
    else:
        logits = _as_torch(bits, dt)
    logits = logits.clone()[:, :V + 3]
    view = logits[:, :V]                                    # row stride V + 3: the tail must stay
    t = lambda v, d: torch.tensor(v, dtype=d)               # noqa: E731
    process_logits(view, torch.from_numpy(hist), torch.from_numpy(pos), torch.from_numpy(tok) if T > 1 else None,
                   repetition_penalty=t(par["rp"], torch.float32), presence_penalty=t(par["pp"], torch.float32),
                   frequency_penalty=t(par["fp"], torch.float32), no_repeat_ngram=t(par["ngram"], torch.int32),
                   min_new_tokens=t(par["min_new"], torch.int64), prompt_len=t(par["prompt_len"], torch.int64),
                   eos=t(par["eos"], torch.int64))
    if dt == "fp32":
        # the fp32 result before any 16-bit rounding: compare with the reference's own fp32 arithmetic
        for r in range(bits.shape[0]):
            b, i = divmod(r, T)
            h = hist[b, :pos[b] + 1].tolist() + (tok[b, 1:i + 1].tolist() if i else [])
            cnt = {}
            for k, tk in enumerate(h):
                if 0 <= tk < V:
                    cnt[tk] = cnt.get(tk, 0) + (k >= par["prompt_len"][b])
            x = R.to_f32(bits[r], R.F16)
            want = x.copy()
            for tk, c in cnt.items():
                y = np.float32(x[tk])
                rp = np.float32(par["rp"][b])
                if rp != 1:
                    y = np.float32(y * rp) if y < 0 else np.float32(y / rp)
                if c > 0:
                    y = np.float32(np.float32(y - np.float32(np.float32(par["fp"][b]) * np.float32(c))) - np.float32(par["pp"][b]))
                want[tk] = y
            for tk in R.banned_ngram_tokens(h, par["ngram"][b]):
                if 0 <= tk < V:
                    want[tk] = -np.inf
            if par["min_new"][b] > 0 and 0 <= par["eos"][b] < V and len(h) - par["prompt_len"][b] < par["min_new"][b]:
                want[par["eos"][b]] = -np.inf
            assert np.array_equal(logits[r, :V].numpy(), want[:V]), r
            assert np.array_equal(logits[r, V:].numpy(), x[V:])
        return
    want = R.process(bits, dt, V, hist, pos, tok if T > 1 else None, **par)
    got = _bits_of(logits)
    _same(got[:, :V], want[:, :V], dt, (dt, T))
    assert np.array_equal(got[:, V:], bits[:, V:])
    nan = np.isnan(R.to_f32(bits, dt)) & (want != R.NEG_INF[dt])     # a NaN logit keeps its bits unless banned
    assert np.array_equal(got[nan], bits[nan])


def test_neutral_values_leave_every_bit():
    from quantizations_amd.layer_ops import process_logits

    bits, hist, pos, tok, _ = _window(R.F16, 3)
    logits = _as_torch(bits, R.F16).clone()
    B = hist.shape[0]
    process_logits(logits, torch.from_numpy(hist), torch.from_numpy(pos), torch.from_numpy(tok),
                   repetition_penalty=torch.ones(B), presence_penalty=torch.zeros(B), frequency_penalty=torch.zeros(B),
                   no_repeat_ngram=torch.zeros(B, dtype=torch.int32), min_new_tokens=torch.zeros(B, dtype=torch.int64),
                   prompt_len=torch.zeros(B, dtype=torch.int64), eos=torch.full((B,), 3, dtype=torch.int64))
    assert np.array_equal(_bits_of(logits), bits)
    assert np.array_equal(R.process(bits, R.F16, 40, hist, pos, tok), bits)


def _bigrams(seq):
    return list(zip(seq[:-1], seq[1:]))


def test_session_no_repeat_bigram(model):  # noqa: F811
    from quantizations_amd.generation import DecodeSession, generate

    S, N = 8, 48
    ids = torch.randint(0, 512, (2, S), generator=torch.Generator().manual_seed(1))
    plain = generate(model, ids, N)
    assert any(len(set(_bigrams(row))) < len(_bigrams(row)) for row in plain.tolist())   # greedy loops
    out = generate(model, ids, N, no_repeat_ngram_size=2)
    for row in out.tolist():
        assert len(set(_bigrams(row))) == len(_bigrams(row)), row
    # the session itself: per-stream values, and a stream left neutral keeps the plain tokens
    sess = DecodeSession(model, 2, S + N, graph=False)
    sess.set_penalties(no_repeat_ngram_size=[2, 0])
    assert sess._processing and sess.prompt_len.tolist() == [0, 0]
    sess.prefill(ids)
    assert sess.prompt_len.tolist() == [S, S]
    for _ in range(N - 1):
        sess.step()
    assert torch.equal(sess.hist[0], out[0]) and torch.equal(sess.hist[1], plain[1])


def test_session_min_new_tokens_and_penalties(model):  # noqa: F811
    from quantizations_amd.generation import DecodeSession, generate

    S, N = 8, 24
    ids = torch.randint(0, 512, (1, S), generator=torch.Generator().manual_seed(4))
    plain = generate(model, ids, N)
    eos = int(plain[0, S + 2])                  # a token the greedy run picks third
    first = (plain[0, S:] == eos).nonzero()[0].item()
    assert first <= 2
    m = 10
    out = generate(model, ids, N, eos_token_id=eos, min_new_tokens=m)
    where = (out[0, S:] == eos).nonzero()
    assert where.numel() == 0 or where[0].item() >= m
    assert torch.equal(out[0, :S + first], plain[0, :S + first])       # the same tokens until the EOS is held back
    # without an EOS the option does nothing
    assert torch.equal(generate(model, ids, N, min_new_tokens=m), plain)
    # penalties: the session equals a manual loop that applies the reference's rules in fp32
    sess = DecodeSession(model, 1, S + N, graph=False)
    sess.set_penalties(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25)
    sess.prefill(ids)
    for _ in range(N - 1):
        sess.step()
    seq = ids[0].tolist()
    with torch.no_grad():
        for _ in range(N):
            x = model(input_ids=torch.tensor([seq])).logits[0, -1].numpy().astype(np.float32)
            for tk in set(seq):
                y = np.float32(x[tk] * np.float32(1.3)) if x[tk] < 0 else np.float32(x[tk] / np.float32(1.3))
                c = seq[S:].count(tk)
                if c:
                    y = np.float32(np.float32(y - np.float32(np.float32(0.25) * np.float32(c))) - np.float32(0.5))
                x[tk] = y
            seq.append(int(np.argmax(x)))
    assert sess.hist[0].tolist() == seq


def test_set_penalties_validates(model):  # noqa: F811
    from quantizations_amd.generation import DecodeSession

    sess = DecodeSession(model, 2, 16, graph=False)
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=[1.0, -1.0]), dict(no_repeat_ngram_size=-1),
                dict(min_new_tokens=-2), dict(presence_penalty=[0.1, 0.2, 0.3]), dict(frequency_penalty=float("nan"))):
        with pytest.raises(ValueError):
            sess.set_penalties(**bad)
    assert not sess._processing
    sess.set_penalties(frequency_penalty=[0.0, 0.5])
    assert sess._processing and sess.frequency_penalty.tolist() == [0.0, 0.5]
    sess.set_penalties(frequency_penalty=0.0)
    assert not sess._processing
