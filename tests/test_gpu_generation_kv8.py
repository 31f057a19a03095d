"""GPU: StreamSession / SpeculativeSession / generate_ragged with kv_dtype="fp8" on the tiny Llama of
test_gpu_generation_paged.py (2 layers, hidden 256, 4 heads of 64 over 2 kv heads, Linear4bit projections).

An fp8 session does not give a 16-bit session's tokens: the cache is quantised.  What is exact is
everything inside the fp8 world -- the wiring (layer 0's pools are the quantised rows of the 16-bit
session's layer 0, whose k and v do not depend on attention), speculative against plain decoding, fork,
prefix sharing, a refused admit -- and the isolation of every other session from the new code.  One
loose bar ties the fp8 session to the 16-bit one: the logits that pick the first new token."""
import pytest
import torch

import kv8_reference as k8
from test_gpu_generation_paged import (CHUNK, LENGTHS, MAX_LEN, N, PAGES, _prompts, _run, _same, _session, _tokens,
                                       _unprepare)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
FP8 = dict(kv_pages=PAGES, kv_dtype="fp8")
# max |logit difference| of the first pick, fp8 session against the 16-bit paged session, measured on an
# MI355X (the 16-bit logits reach 1.386 / 1.398 in magnitude): the bar is four times that
MEASURED = {torch.float16: 0.0344238, torch.bfloat16: 0.0439453}


def _build(dtype):
    from transformers import LlamaConfig, LlamaForCausalLM

    from quantizations_amd.generation import prepare_for_decode
    from quantizations_amd.integration import replace_with_bnb_linear

    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=4096, max_position_embeddings=512, rope_theta=500000.0,
                      eos_token_id=None, bos_token_id=None, pad_token_id=None)
    torch.manual_seed(0)
    m = LlamaForCausalLM(cfg).to(dtype).to(DEV).eval()
    replace_with_bnb_linear(m, modules_to_not_convert=["lm_head"], quant_type="nf4", compute_dtype=torch.float32)
    prepare_for_decode(m)
    return m


@pytest.fixture(scope="module")
def model():
    m = _build(torch.float16)
    try:
        yield m
    finally:
        _unprepare(m)


@pytest.fixture(scope="module")
def plain8(model):
    """The undisturbed fp8 session the others are compared with (computed once)."""
    return _session(model, **FP8)


def test_fp8_session_wiring_and_page_size(model, plain8):
    from quantizations_amd.generation import PagedKVCache

    a = _session(model, steps=0, kv_pages=PAGES)
    b = _session(model, steps=0, **FP8)
    assert isinstance(b.cache, PagedKVCache) and b.cache.kv_dtype == "fp8" and a.cache.kv_dtype is None
    assert b.cache.bytes_per_page == 2 * 2 * 2 * 128 * (64 + 1) == b.page_stats()["bytes_per_page"]
    assert a.cache.bytes_per_page == 2 * 2 * 2 * 128 * 64 * 2
    l16, l8 = a.cache.layers[0], b.cache.layers[0]
    assert l8.keys.dtype == torch.uint8 and tuple(l8.keys.shape) == (PAGES, 2, 128 * 65)
    for p16, p8 in ((l16.keys, l8.keys), (l16.values, l8.values)):
        want_c, want_s = k8.quantize_rows(p16.cpu())
        got_c, got_s = k8.unpack_pool(p8.cpu(), 64)
        for r, n in enumerate(LENGTHS):
            for c, (pg16, pg8) in enumerate(zip(a.pages.pages(r), b.pages.pages(r))):
                m = max(0, min(128, n - 128 * c))
                assert torch.equal(got_c[pg8, :, :m], want_c[pg16, :, :m]) and torch.equal(got_s[pg8, :, :m], want_s[pg16, :, :m])
    # the whole run: every page the streams hold stays finite, and the graph was captured
    assert plain8._graph is not None and plain8.pos.tolist() == [n + N - 1 for n in LENGTHS]
    eager = _session(model, graph=False, **FP8)
    _same(eager, plain8)
    plain8.pages.check()


def test_fp8_speculative_session_emits_the_stream_sessions_tokens(model, plain8):
    from quantizations_amd.generation import SpeculativeSession, generate_ragged

    for graph, drafts in ((True, 3), (False, 2)):
        spec = _session(model, cls=SpeculativeSession, graph=graph, draft_tokens=drafts, **FP8)
        for a, b in zip(plain8.sequences(), spec.sequences()):
            assert torch.equal(a, b)
    ids = _prompts()
    prompts = [ids[r, :n] for r, n in enumerate(LENGTHS)]
    for kw in ({}, {"prompt_lookup_num_tokens": 3}):
        outs = generate_ragged(model, prompts, N, prefill_chunk=CHUNK, **FP8, **kw)
        for a, b in zip(plain8.sequences(), outs):
            assert torch.equal(a, b)
    sampled = _session(model, sampling=True, **FP8)
    spec = _session(model, cls=SpeculativeSession, sampling=True, sample=True, draft_tokens=3, **FP8)
    for a, b in zip(sampled.sequences(), spec.sequences()):
        assert torch.equal(a, b)
    assert not all(torch.equal(a, b) for a, b in zip(sampled.sequences(), plain8.sequences()))


def test_fp8_fork_continues_as_its_source(model, plain8):
    sess = _session(model, steps=10, **FP8)
    sess.fork(0, 1)
    assert sess.pages.pages(1)[:2] == sess.pages.pages(0)[:2] and sess.pages.pages(1)[2] != sess.pages.pages(0)[2]
    captured = sess._graph
    _run(sess, N - 1 - 10)
    assert sess._graph is captured
    assert torch.equal(sess.hist[1], sess.hist[0]) and sess.pos[1].item() == sess.pos[0].item()
    for r in (0, 2):
        assert torch.equal(sess.hist[r], plain8.hist[r])
    sess.pages.check()


def test_fp8_prefix_shared_admit_picks_the_unshared_admits_tokens(model):
    donor = _tokens(200, 30)
    newcomer = torch.cat((donor[:160], _tokens(30, 31)))
    runs = {}
    for share in (True, False):
        sess = _session(model, steps=4, prefix_cache=share, max_new_tokens=[N, 2, 2], **FP8)
        sess.admit(1, donor, max_new_tokens=8)
        sess.admit(2, newcomer, max_new_tokens=8)
        assert (sess.pages.pages(2)[0] == sess.pages.pages(1)[0]) == share
        _run(sess, 8)
        sess.pages.check()
        runs[share] = sess
    _same(runs[True], runs[False])


def test_fp8_exhaustion_leaves_the_session_as_it_was(model, plain8):
    from quantizations_amd.kv_pages import KVPagesExhausted

    sess = _session(model, steps=6, kv_pages=7, kv_dtype="fp8")
    table, stats = sess.pages.table.clone(), sess.page_stats()
    state = [t.clone() for t in (sess.hist, sess.pos, sess.live, sess.tok, sess.limit)]
    pools = [layer.keys.clone() for layer in sess.cache.layers]
    with pytest.raises(KVPagesExhausted):
        sess.admit(2, _tokens(200, 12), max_new_tokens=60)
    assert torch.equal(sess.pages.table, table) and sess.page_stats() == stats
    for t, v in zip((sess.hist, sess.pos, sess.live, sess.tok, sess.limit), state):
        assert torch.equal(t, v)
    for layer, before in zip(sess.cache.layers, pools):
        assert torch.equal(layer.keys, before)
    _run(sess, N - 1 - 6)
    _same(sess, plain8)


def test_fp8_refusals(model):
    from quantizations_amd.generation import PagedKVCache, SpeculativeSession, StreamSession, generate_ragged

    with pytest.raises(ValueError, match="kv_pages"):
        StreamSession(model, 3, MAX_LEN, prefill_chunk=CHUNK, kv_dtype="fp8")
    with pytest.raises(ValueError, match="kv_pages"):
        SpeculativeSession(model, 3, MAX_LEN, prefill_chunk=CHUNK, kv_dtype="fp8")
    with pytest.raises(ValueError, match="kv_pages"):
        generate_ragged(model, [_tokens(5, 1)], 2, prefill_chunk=CHUNK, kv_dtype="fp8")
    for bad in ("fp16", "e5m2", "FP8", ""):
        with pytest.raises(ValueError, match="kv_dtype"):
            StreamSession(model, 3, MAX_LEN, prefill_chunk=CHUNK, kv_pages=PAGES, kv_dtype=bad)
        with pytest.raises(ValueError, match="kv_dtype"):
            PagedKVCache(model.config, 4, torch.float16, DEV, kv_dtype=bad)


def test_other_sessions_call_none_of_the_kv8_wrappers(model, monkeypatch):
    from quantizations_amd import layer_ops
    from quantizations_amd.generation import SpeculativeSession

    names = ("decode_attention_paged_kv8", "decode_attention_verify_paged_kv8", "prefill_attention_paged_kv8")
    calls = []
    for name in names:
        real = getattr(layer_ops, name)
        monkeypatch.setattr(layer_ops, name, lambda *a, _r=real, _n=name, **k: (calls.append(_n), _r(*a, **k))[1])
    _session(model, steps=3, graph=False)
    _session(model, steps=3, graph=False, cls=SpeculativeSession, draft_tokens=2)
    _session(model, steps=3, graph=False, kv_pages=PAGES)
    _session(model, steps=3, graph=False, kv_pages=PAGES, cls=SpeculativeSession, draft_tokens=2)
    assert not calls
    _session(model, steps=2, graph=False, **FP8)
    _session(model, steps=2, graph=False, cls=SpeculativeSession, draft_tokens=2, **FP8)
    assert set(calls) == set(names)


def _first_logits(model, **kw):
    from quantizations_amd.generation import StreamSession

    sess = StreamSession(model, 3, MAX_LEN, graph=False, prefill_chunk=CHUNK, **kw)
    seen, pick = [], sess._pick
    sess._pick = lambda logits, *a, **k: (seen.append(logits.float().clone()), pick(logits, *a, **k))[1]
    sess.prefill(_prompts(), LENGTHS, max_new_tokens=N)
    torch.cuda.synchronize()
    return seen[0]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_first_logits_stay_near_the_16_bit_sessions(model, dtype):
    """The logits that pick the first new token (prompts of 250 / 131 / 70 tokens in windows of 64), fp8
    session against 16-bit paged session: a wrong scale that still decodes to finite numbers moves them
    by the size of the logits themselves.  Measured on an MI355X: 0.0344 at fp16 and 0.0439 at bf16,
    against logits of up to 1.39 (MEASURED); the bar is four times the measured value, because GEMM
    routes and boxes move it."""
    m = model if dtype == torch.float16 else _build(dtype)
    try:
        ref = _first_logits(m, kv_pages=PAGES)
        got = _first_logits(m, **FP8)
    finally:
        if m is not model:
            _unprepare(m)
    diff = float((got - ref).abs().max())
    print(f"first logits {dtype}: max |fp8 - 16-bit| = {diff:.6g}, max |16-bit| = {float(ref.abs().max()):.6g}")
    assert bool(torch.isfinite(got).all())
    assert diff <= 4 * MEASURED[dtype], (diff, MEASURED[dtype])
