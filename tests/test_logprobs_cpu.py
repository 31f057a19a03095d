"""CPU: log-probabilities without a GPU.  (1) The float32 numpy restatement of tests/logprobs_reference.py
stays inside HALF of the bars the GPU tests assert against the float64 reference, over every family
(the rule of test_activation_families.py) -- and the bars are twice what it measures.  (2) The
composed torch route of layer_ops.token_logprobs / logprobs_streams (what CPU and fp32 logits take)
against the same reference: ids and order exactly, values inside the bars, the non-finite classes,
the V < n tail, the liveness rule on sentinel-filled tables.  (3) DecodeSession / generate() with
`logprobs` on the fp32 tiny Llama of test_generation_cpu.py: same tokens, tables aligned with hist
and equal to log_softmax of a teacher-forced forward."""
import numpy as np
import pytest
import torch

import logprobs_reference as R

NAMES = [R.F16, R.BF16]
DT = {R.F16: torch.float16, R.BF16: torch.bfloat16}


def as_logits(bits, name):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(DT[name])


# ---------------------------------------------------------------------------------------------
# 1. the bars
# ---------------------------------------------------------------------------------------------

def test_restatement32_within_half_the_bars_and_the_bars_are_twice_the_measurement():
    errs, mags = [], []
    for name in NAMES:
        for (label, bits, ids), ref in zip(R.cases(name), R.expected(name)):
            got = R.restatement32(bits, name, ids, R.MAX_TOP)
            assert np.array_equal(got[1], ref[1]), label
            for g, r in ((got[0], ref[0]), (got[2], ref[2])):
                ok, worst = R.within(g, r, scale=0.5)
                assert ok, (name, label, worst)
                e, m = R.errors(g, r)
                errs.append(e)
                mags.append(m)
    e, m = np.concatenate(errs), np.concatenate(mags)
    rel, ab = float((e[m >= 1] / m[m >= 1]).max()), float(e[m < 1].max())
    print(f"measured REL {rel:.4e} ABS {ab:.4e}; bars {R.LP_REL:.4e} {R.LP_ABS:.4e}")
    # the recorded measurement is the measurement (numpy's exp / log may move it by an ulp or two) ...
    assert 0.5 * R.MEASURED_REL <= rel <= R.MEASURED_REL and 0.5 * R.MEASURED_ABS <= ab <= R.MEASURED_ABS
    assert R.LP_REL == 2 * R.MEASURED_REL and R.LP_ABS == 2 * R.MEASURED_ABS      # ... and the bars twice it


def test_families_reach_their_edges():
    for name in NAMES:
        by = {label: (bits, ids) for label, bits, ids in R.cases(name)}
        ref = dict(zip(by, R.expected(name)))
        lp, ti, tl = ref["one hot 6e4 over -6e4"]
        assert lp[0] == 0.0 and tl[0, 0] == 0.0 and ti[0, 0] == R.CHUNK + 2 and tl[0, 1] < -1.19e5
        assert list(ti[0, 1:4]) == [0, 1, 2]                           # the cold ones tie: index order
        lp, ti, tl = ref[f"flat V={2 * R.CHUNK + 37}"]
        assert list(ti[0]) == list(range(R.MAX_TOP)) and abs(lp[0] + np.log(2 * R.CHUNK + 37)) < 1e-6
        _, ti, _ = ref["top n across a boundary / in the partial chunk"]
        assert ti[0].min() < R.CHUNK <= ti[0].max() and ti[1].min() >= 2 * R.CHUNK
        _, ti, tl = ref["n + 3 equal maxima over the chunks"]
        assert list(ti[0]) == [179 * k for k in range(R.MAX_TOP)] and len(set(tl[0])) == 1
        assert ti[0].max() > R.CHUNK
        _, ti, tl = ref["randn4 V=5 R=3"]
        assert (ti[:, 5:] == -1).all() and np.isneginf(tl[:, 5:]).all() and (ti[:, :5] >= 0).all()
        bits = by["subnormal logits and signed zeros"][0]
        assert set(bits[1, :40].tolist()) == {0, 0x8000} and float(np.abs(R.to_f64(bits, name)).max()) < 2.0 ** -14
        lp, ti, tl = ref["-inf holes"]
        assert np.isneginf(lp[0]) and np.isneginf(tl[1, 3:]).all() and list(ti[1, 3:6]) == [3, 4, 5]
        lp, ti, _ = ref["ids at 0, V - 1, outside and below the lists"]
        assert np.isnan(lp[2]) and np.isnan(lp[4]) and np.isfinite(lp[[0, 1, 3]]).all()
        assert by["ids at 0, V - 1, outside and below the lists"][1][3] not in ti[3]
        if name == R.BF16:
            lp, _, tl = ref["bf16 at 3e38"]
            assert np.isneginf(lp[0]) and -2.0 < tl[0, 0] <= 0.0       # x - m is beyond fp32: -inf, as the reference rounds
        (_, bits, _), = R.nonfinite_cases(name)
        lp, ti, tl = R.expected(name, True, True)[0]
        assert np.isnan(lp[1:5]).all() and np.isfinite(lp[[0, 5]]).all()
        assert (ti[1:5] == -1).all() and np.isnan(tl[1:5]).all() and np.isfinite(tl[[0, 5]]).all()


# ---------------------------------------------------------------------------------------------
# 2. the composed route
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n", [0, 1, 5, 20])
def test_composed_token_logprobs_against_the_reference(name, n):
    from quantizations_amd.layer_ops import token_logprobs

    worst = 0.0
    for nonfinite in (False, True):
        src = R.nonfinite_cases(name) if nonfinite else R.cases(name)
        for (label, bits, ids), ref in zip(src, R.expected(name, True, nonfinite)):
            lp, ti, tl = token_logprobs(as_logits(bits, name), torch.from_numpy(ids), n)
            assert lp.dtype == torch.float32 and ti.dtype == torch.int32 and ti.shape == tl.shape == (len(ids), n)
            assert np.array_equal(ti.numpy(), ref[1][:, :n]), label
            for g, r in ((lp.numpy(), ref[0]), (tl.numpy(), ref[2][:, :n])):
                ok, w = R.within(g, r)
                worst = max(worst, w)
                assert ok, (label, w)
    print("largest difference", worst)


def test_composed_takes_fp32_logits_and_refuses_bad_arguments():
    from quantizations_amd.layer_ops import LOGPROBS_MAX_TOP, token_logprobs, token_logprobs_supported

    assert LOGPROBS_MAX_TOP == 20
    x = torch.randn(3, 77, generator=torch.Generator().manual_seed(3))
    ids = torch.tensor([0, 76, 5])
    lp, ti, tl = token_logprobs(x, ids, 4)
    want = torch.log_softmax(x, -1)
    assert torch.equal(lp, want[torch.arange(3), ids]) and torch.equal(ti.long(), want.topk(4).indices)
    assert not token_logprobs_supported(x) and not token_logprobs_supported(x.half())
    for bad in (dict(top=21), dict(top=-1), dict(top=True)):
        with pytest.raises(ValueError, match="top"):
            token_logprobs(x, ids, **bad)
    with pytest.raises(ValueError, match="ids"):
        token_logprobs(x, ids.int())
    with pytest.raises(ValueError, match="ids"):
        token_logprobs(x, ids[:2])


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n", [0, 3])
def test_composed_streams_write_only_live_rows(name, n):
    """B = 4 streams, T = 3 rows each, L = 9 columns.  Stream 0 emitted 3 tokens, stream 1 one (rows 1 and
    2 lie above pos1), stream 2 did not move, stream 3 emitted 3 from column 7 on: column 9 = L is
    outside.  Everything else keeps the sentinel."""
    from quantizations_amd.layer_ops import logprobs_streams

    B, T, L, V = 4, 3, 9, 300
    rng = np.random.default_rng(8)
    bits = R.to_bits(rng.standard_normal((B * T, V)) * 3, name)
    seq = rng.integers(0, V, (B, L)).astype(np.int64)
    pos0, pos1 = np.array([2, 4, 5, 6], np.int64), np.array([5, 5, 5, 9], np.int64)
    live = {(0, 3), (0, 4), (0, 5), (1, 5), (3, 7), (3, 8)}
    lp_tab = torch.full((B, L), 7.0)
    ti_tab = torch.full((B, L, n), -7, dtype=torch.int32) if n else None
    tl_tab = torch.full((B, L, n), 7.0) if n else None
    logprobs_streams(as_logits(bits, name), torch.from_numpy(seq), torch.from_numpy(pos0), torch.from_numpy(pos1),
                     lp_tab, ti_tab, tl_tab, T=T)
    want_lp = np.full((B, L), 7.0, np.float32)
    want_ti, want_tl = np.full((B, L, n), -7, np.int32), np.full((B, L, n), 7.0, np.float32)
    R.streams_reference(bits, name, seq, pos0, pos1, T, n, want_lp, want_ti, want_tl)
    assert {(b, c) for b in range(B) for c in range(L) if want_lp[b, c] != 7.0} == live
    written = lp_tab.numpy() != 7.0
    assert np.array_equal(written, want_lp != 7.0)
    assert R.within(lp_tab.numpy()[written], want_lp[written])[0]
    if n:
        assert np.array_equal(ti_tab.numpy(), want_ti)
        assert np.array_equal(tl_tab.numpy() != 7.0, want_tl != 7.0)
        assert R.within(tl_tab.numpy()[written], want_tl[written])[0]
    # one shared position (DecodeSession): stride 0
    lp2 = torch.full((B, L), 7.0)
    logprobs_streams(as_logits(bits[::T].copy(), name), torch.from_numpy(seq), torch.tensor([3]), torch.tensor([4]), lp2)
    assert np.array_equal(lp2.numpy() != 7.0, np.arange(L)[None, :].repeat(B, 0) == 4)


# ---------------------------------------------------------------------------------------------
# 3. sessions on the CPU
# ---------------------------------------------------------------------------------------------

S, N = 8, 12


@pytest.fixture(scope="module")
def model():
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=512, max_position_embeddings=128, rope_theta=10000.0,
                      initializer_range=0.1, eos_token_id=None, bos_token_id=None, pad_token_id=None)
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg).eval()


def _teacher(model, seq):
    """log_softmax of the model's logits for every column >= 1 of seq, [B, L, V] (column 0: NaN)."""
    with torch.no_grad():
        lo = model(input_ids=seq).logits
    out = torch.full_like(lo, float("nan"))
    out[:, 1:] = torch.log_softmax(lo[:, :-1].float(), -1)
    return out


@pytest.mark.parametrize("mode", ["greedy", "sampled", "penalties"])
def test_decode_session_logprobs_on_cpu(model, mode):
    from quantizations_amd.generation import DecodeSession

    B, n = 2, 5
    ids = torch.randint(0, 512, (B, S), generator=torch.Generator().manual_seed(11))

    def run(logprobs):
        sess = DecodeSession(model, B, S + N, logprobs=logprobs)
        if mode == "sampled":
            sess.set_sampling(temperature=[0.8, 1.2], top_k=[30, 0], top_p=[1.0, 0.9])
            sess.seed(4)
        if mode == "penalties":
            sess.set_penalties(repetition_penalty=1.4, frequency_penalty=0.3, no_repeat_ngram_size=2)
        sess.prefill(ids)
        for _ in range(N - 1):
            sess.step()
        return sess

    plain, sess = run(None), run(n)
    assert plain.logprobs is None and plain.top_ids is None and plain._pos0 is None
    assert torch.equal(plain.hist, sess.hist) and torch.equal(plain.pos, sess.pos)
    assert sess.logprobs.shape == (B, S + N) and sess.top_ids.shape == sess.top_logprobs.shape == (B, S + N, n)
    assert bool(torch.isnan(sess.logprobs[:, :S]).all()) and bool((sess.top_ids[:, :S] == -1).all())
    assert bool(torch.isfinite(sess.logprobs[:, S:]).all())
    # the model's own distribution, whatever the processors and the sampler did with it
    want = _teacher(model, sess.hist)
    got = sess.logprobs[:, S:]
    ref = want.gather(2, sess.hist[:, :, None])[:, S:, 0]
    assert float((got - ref).abs().max()) <= 1e-4
    top = want[:, S:].topk(n, -1)
    assert torch.equal(sess.top_ids[:, S:].long(), top.indices)
    assert float((sess.top_logprobs[:, S:] - top.values).abs().max()) <= 1e-4
    if mode == "greedy":
        assert torch.equal(sess.top_ids[:, S:, 0].long(), sess.hist[:, S:])
        assert torch.equal(sess.logprobs[:, S:], sess.top_logprobs[:, S:, 0])


def test_generate_returns_generate_output_on_cpu(model):
    import quantizations_amd as qa

    ids = torch.randint(0, 512, (2, S), generator=torch.Generator().manual_seed(2))
    plain = qa.generate(model, ids, N)
    out = qa.generate(model, ids, N, logprobs=0)
    assert isinstance(out, qa.GenerateOutput) and torch.equal(out.sequences, plain)
    assert out.logprobs.shape == (2, S + N) and out.top_ids.shape == (2, S + N, 0)
    assert bool(torch.isnan(out.logprobs[:, :S]).all()) and bool(torch.isfinite(out.logprobs[:, S:]).all())
    # behind a stream's first EOS nothing was emitted: NaN / -1 there
    eos = int(plain[0, S + 3])
    cut = qa.generate(model, ids, N, eos_token_id=eos, logprobs=2)
    first = int((cut.sequences[0, S:] == eos).nonzero()[0])
    assert bool(torch.isfinite(cut.logprobs[0, S:S + first + 1]).all())
    assert bool(torch.isnan(cut.logprobs[0, S + first + 1:]).all()) and bool((cut.top_ids[0, S + first + 1:] == -1).all())
    empty = qa.generate(model, ids, 0, logprobs=3)
    assert torch.equal(empty.sequences, ids) and empty.top_ids.shape == (2, S, 3)


@pytest.mark.parametrize("bad", [21, -1, True, 2.0])
def test_sessions_refuse_a_bad_logprobs(model, bad):
    import quantizations_amd as qa

    with pytest.raises(ValueError, match="logprobs"):
        qa.DecodeSession(model, 1, 8, logprobs=bad)
    with pytest.raises(ValueError, match="logprobs"):
        qa.generate(model, torch.zeros((1, 4), dtype=torch.int64), 2, logprobs=bad)
    with pytest.raises(ValueError, match="logprobs"):
        qa.StreamSession(model, 1, 8, logprobs=bad)
    with pytest.raises(ValueError, match="logprobs"):
        qa.generate_ragged(model, [torch.zeros(4, dtype=torch.int64)], 2, logprobs=bad)


def test_prompt_logprobs_and_score_refusals(model):
    import quantizations_amd as qa

    with pytest.raises(ValueError, match="prompt_logprobs"):
        qa.StreamSession(model, 1, 8, logprobs=0, prompt_logprobs=True)
    with pytest.raises(ValueError, match="model"):
        qa.score(model, [torch.zeros(4, dtype=torch.int64)])
