"""GPU: StreamSession / SpeculativeSession / generate_ragged over a paged KV cache (kv_pages=...), on the
tiny random-init Llama of test_gpu_generation_prefill.py (2 layers, hidden 256, vocab 4096, Linear4bit
projections), built afresh here with max_position_embeddings 512.

Every check is exact.  The paged launches carry the bits of the contiguous launches, so a paged session
that runs the same windows as a contiguous one gives the same tokens: hist, pos and live are compared
with torch.equal, graph and eager, greedy and speculative.  admit() after the capture, release(), fork()
and a refused admit() leave the other streams on an undisturbed run's tokens and the graph object in
place.  Prefix sharing is counted (pages, refcounts, the windows the newcomer runs) and its tokens are
compared with the same admit into a session that shares nothing: the donor ran the same batch-1,
64-token windows, so the shared page holds the bits the newcomer would have computed."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
N = 24
LENGTHS = [250, 131, 70]      # stream 0 crosses the page edge at 256 while decoding
SMAX = max(LENGTHS)
MAX_LEN = SMAX + N + 12       # 286: three pages per stream
CHUNK = 64
PAGES = 12


def _unprepare(model):
    from quantizations_amd import integration as I

    I.unfuse_lm_head(model)
    I.unfuse_decode_glue(model)
    I.unfuse_prenorm(model)
    I.unfuse_layer_ops(model)
    I.unfuse_projection_groups(model)
    model.__dict__.pop("_qz_prepared", None)


@pytest.fixture(scope="module")
def model():
    from transformers import LlamaConfig, LlamaForCausalLM

    from quantizations_amd.generation import prepare_for_decode
    from quantizations_amd.integration import replace_with_bnb_linear

    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=4096, max_position_embeddings=512, rope_theta=500000.0,
                      eos_token_id=None, bos_token_id=None, pad_token_id=None)
    torch.manual_seed(0)
    m = LlamaForCausalLM(cfg).half().to(DEV).eval()
    replace_with_bnb_linear(m, modules_to_not_convert=["lm_head"], quant_type="nf4", compute_dtype=torch.float32)
    prepare_for_decode(m)
    try:
        yield m
    finally:
        _unprepare(m)


def _prompts():
    return torch.randint(0, 4096, (3, SMAX), generator=torch.Generator().manual_seed(3)).to(DEV)


def _tokens(n, seed):
    return torch.randint(0, 4096, (n,), generator=torch.Generator().manual_seed(seed))


def _run(sess, steps):
    for _ in range(steps):
        sess.step()
    torch.cuda.synchronize()


def _session(model, cls=None, graph=True, steps=N - 1, sampling=False, **kw):
    from quantizations_amd.generation import StreamSession

    prefill_kw = {"max_new_tokens": kw.pop("max_new_tokens", N)}
    sess = (cls or StreamSession)(model, 3, MAX_LEN, graph=graph, prefill_chunk=CHUNK, **kw)
    if sampling:
        sess.set_sampling(temperature=1.0, top_k=50)
        sess.seed(11)
    sess.prefill(_prompts(), LENGTHS, **prefill_kw)
    _run(sess, steps)
    return sess


def _same(a, b):
    assert torch.equal(a.hist, b.hist) and torch.equal(a.pos, b.pos) and torch.equal(a.live, b.live)


@pytest.fixture(scope="module")
def contiguous(model):
    """The contiguous session every paged run is compared with (computed once)."""
    return _session(model)


def test_paged_session_equals_the_contiguous_session(model, contiguous):
    from quantizations_amd.generation import PagedKVCache

    a = _session(model, kv_pages=PAGES)
    b = _session(model, graph=False, kv_pages=PAGES)
    assert isinstance(a.cache, PagedKVCache) and a._graph is not None and b._graph is None
    _same(a, contiguous)
    _same(b, contiguous)
    assert a.pos.tolist() == [n + N - 1 for n in LENGTHS] and not bool(a.alive().any())
    st = a.page_stats()
    assert st == {"free": PAGES - 6, "held": 6, "idle": 0, "total": PAGES, "bytes_per_page": 2 * 2 * 2 * 128 * 64 * 2}
    assert [len(a.pages.pages(r)) for r in range(3)] == [3, 2, 1]      # up to each stream's limit
    a.pages.check()
    with pytest.raises(RuntimeError):
        a.cache.update(None, None, 0)


def test_paged_speculative_session_equals_the_contiguous_one(model, contiguous):
    from quantizations_amd.generation import SpeculativeSession, generate_ragged

    plain = _session(model, cls=SpeculativeSession, draft_tokens=3)
    for graph in (True, False):
        spec = _session(model, cls=SpeculativeSession, graph=graph, draft_tokens=3, kv_pages=PAGES)
        _same(spec, plain)
        assert torch.equal(spec.accepted, plain.accepted)
    for a, b in zip(contiguous.sequences(), spec.sequences()):
        assert torch.equal(a, b)
    ids = _prompts()
    outs = generate_ragged(model, [ids[r, :n] for r, n in enumerate(LENGTHS)], N, prefill_chunk=CHUNK, kv_pages=PAGES)
    for a, b in zip(contiguous.sequences(), outs):
        assert torch.equal(a, b)


def test_kv_pages_needs_prefill_chunk_and_a_paged_session(model, contiguous):
    from quantizations_amd.generation import StreamSession

    with pytest.raises(ValueError):
        StreamSession(model, 3, MAX_LEN, kv_pages=PAGES)
    with pytest.raises(ValueError):
        StreamSession(model, 3, MAX_LEN, prefill_chunk=CHUNK, prefix_cache=True)
    with pytest.raises(ValueError):
        StreamSession(model, 3, MAX_LEN, prefill_chunk=CHUNK, kv_pages=2)      # fewer pages than rows
    for call in (lambda: contiguous.release(0), lambda: contiguous.fork(0, 1), contiguous.page_stats):
        with pytest.raises(ValueError):
            call()


def test_admit_after_capture_without_recapture(model, contiguous):
    sess = _session(model, steps=6, kv_pages=PAGES, max_new_tokens=[N, 4, N])    # stream 1 retires by its limit
    captured = sess._graph
    assert captured is not None and sess.alive().tolist() == [True, False, True]
    newcomer = _tokens(140, 8)
    sess.admit(1, newcomer, max_new_tokens=7)
    assert sess.alive().tolist() == [True, True, True] and sess.pos[1].item() == 140
    _run(sess, N - 1 - 6)
    assert sess._graph is captured, "no recapture"
    for r in (0, 2):
        assert torch.equal(sess.hist[r], contiguous.hist[r])
    seq = sess.sequences()[1]
    assert torch.equal(seq[:140].cpu(), newcomer) and seq.numel() == 147
    # the same admit into a contiguous session: the same batch-1 windows, the same tokens
    ref = _session(model, steps=6, max_new_tokens=[N, 4, N])
    ref.admit(1, newcomer, max_new_tokens=7)
    _run(ref, N - 1 - 6)
    _same(sess, ref)
    sess.pages.check()


def _count_prefill(monkeypatch):
    from quantizations_amd import layer_ops

    calls = []
    real = layer_ops.prefill_attention_paged

    def spy(q, k, v, cos, sin, kp, vp, table, pos, length, nq, scale):
        calls.append((int(pos.min()), int(length.sum())))
        return real(q, k, v, cos, sin, kp, vp, table, pos, length, nq, scale)
    monkeypatch.setattr(layer_ops, "prefill_attention_paged", spy)
    return calls


def test_prefix_sharing_runs_the_windows_behind_the_shared_page_only(model, monkeypatch):
    donor = _tokens(200, 30)
    newcomer = torch.cat((donor[:160], _tokens(30, 31)))          # equal in its first 160 tokens: one full page
    runs = {}
    for share in (True, False):
        sess = _session(model, steps=4, kv_pages=PAGES, prefix_cache=share, max_new_tokens=[N, 2, 2])
        assert sess.alive().tolist() == [True, False, False]
        sess.admit(1, donor, max_new_tokens=8)
        calls = _count_prefill(monkeypatch)
        sess.admit(2, newcomer, max_new_tokens=8)
        monkeypatch.undo()
        page = sess.pages.pages(1)[0]
        if share:
            assert sess.pages.pages(2)[0] == page and sess.pages.refcount(page) == 2
            assert sess.pages.pages(2)[1] not in sess.pages.pages(1)
            # two layers, one window of 62 rows from position 128
            assert calls == [(128, 62), (128, 62)], calls
        else:
            assert sess.pages.pages(2)[0] != page and sess.pages.refcount(page) == 1
            assert [c[0] for c in calls] == [0, 0, 64, 64, 128, 128] and sum(c[1] for c in calls) == 2 * 190
        _run(sess, 8)
        sess.pages.check()
        runs[share] = sess
    _same(runs[True], runs[False])
    assert runs[True].sequences()[2].numel() == 190 + 8
    # a different salt shares nothing
    sess = runs[True]
    sess.release(2)
    calls = _count_prefill(monkeypatch)
    sess.admit(2, newcomer, max_new_tokens=8, prefix_salt="another adapter")
    monkeypatch.undo()
    assert [c[0] for c in calls] == [0, 0, 64, 64, 128, 128]
    assert sess.pages.pages(2)[0] != sess.pages.pages(1)[0] and sess.pages.refcount(sess.pages.pages(1)[0]) == 1
    _run(sess, 8)
    assert torch.equal(sess.sequences()[2], runs[False].sequences()[2])
    sess.pages.check()


def test_release_returns_the_pages_and_the_row_steps_on(model, contiguous):
    sess = _session(model, steps=5, kv_pages=PAGES, prefix_cache=True)
    held = sess.page_stats()["held"]
    gone = sess.pages.pages(1)
    sess.release(1)
    st = sess.page_stats()
    # stream 1 held two pages: its first was a full prompt page, published, so it stays resident but idle
    assert st["held"] == held - 1 and st["idle"] == 1 and len(sess.pages.pages(1)) == 1
    assert sess.pos[1].item() == 0 and not bool(sess.alive()[1])
    captured = sess._graph
    _run(sess, 5)
    own = sess.pages.pages(1)[0]
    for layer in sess.cache.layers:
        assert bool(torch.isfinite(layer.keys[own].float()).all()) and bool(torch.isfinite(layer.values[own].float()).all())
    assert sess.pos[1].item() == 0 and torch.equal(sess.hist[1], _hist_at(model, 5)[1])
    # a later admit takes pages again (the released ones among them) while the others run on undisturbed
    newcomer = _tokens(150, 9)
    sess.admit(1, newcomer, max_new_tokens=6)
    assert set(sess.pages.pages(1)) & (set(gone) | {own})
    _run(sess, N - 1 - 10)
    assert sess._graph is captured
    for r in (0, 2):
        assert torch.equal(sess.hist[r], contiguous.hist[r])
    assert sess.sequences()[1].numel() == 156
    sess.pages.check()


_HIST = {}


def _hist_at(model, steps):
    """hist of the contiguous session after `steps` steps (computed once per step count)."""
    if steps not in _HIST:
        _HIST[steps] = _session(model, steps=steps).hist.clone()
    return _HIST[steps]


def test_eviction_under_pressure_never_takes_a_live_streams_page(model, contiguous):
    """Nine pages: streams 0 and 2 hold 3 + 1, row 1 is admitted again and again with prompts of two
    pages whose first page is published, so idle pages pile up and are evicted for the next prompt."""
    sess = _session(model, steps=2, kv_pages=9, prefix_cache=True, max_new_tokens=[N, 1, N])
    mine = set(sess.pages.pages(0)) | set(sess.pages.pages(2))
    evicted = False
    for i in range(4):
        before = set(sess.pages._key_of)
        sess.admit(1, _tokens(130, 40 + i), max_new_tokens=2)
        evicted |= bool(before - set(sess.pages._key_of))
        assert mine == set(sess.pages.pages(0)) | set(sess.pages.pages(2))
        assert not set(sess.pages.pages(1)) & mine
        sess.pages.check()
        _run(sess, 3)
    assert evicted, "the pool was large enough to keep every published page: no pressure"
    _run(sess, N - 1 - 2 - 12)
    for r in (0, 2):
        assert torch.equal(sess.hist[r], contiguous.hist[r])


def test_exhaustion_leaves_the_session_as_it_was(model, contiguous):
    from quantizations_amd.kv_pages import KVPagesExhausted

    sess = _session(model, steps=6, kv_pages=7)       # 3 + 2 + 1 pages held, one free
    table, stats = sess.pages.table.clone(), sess.page_stats()
    state = [t.clone() for t in (sess.hist, sess.pos, sess.live, sess.tok, sess.limit)]
    with pytest.raises(KVPagesExhausted):
        sess.admit(2, _tokens(200, 12), max_new_tokens=60)        # three pages: two more than row 2 can get
    assert torch.equal(sess.pages.table, table) and sess.page_stats() == stats
    for t, v in zip((sess.hist, sess.pos, sess.live, sess.tok, sess.limit), state):
        assert torch.equal(t, v)
    _run(sess, N - 1 - 6)
    _same(sess, contiguous)
    sess.pages.check()


def test_fork_continues_one_stream_in_two_rows(model, contiguous):
    sess = _session(model, steps=10, kv_pages=PAGES)
    p = int(sess.pos[0])
    assert p == 260 and p & 127
    sess.fork(0, 1)
    assert sess.pages.pages(1)[:2] == sess.pages.pages(0)[:2] and sess.pages.pages(1)[2] != sess.pages.pages(0)[2]
    assert [sess.pages.refcount(x) for x in sess.pages.pages(0)] == [2, 2, 1]
    captured = sess._graph
    _run(sess, N - 1 - 10)
    assert sess._graph is captured
    assert torch.equal(sess.hist[1], sess.hist[0]) and sess.pos[1].item() == sess.pos[0].item()
    for r in (0, 2):
        assert torch.equal(sess.hist[r], contiguous.hist[r])
    sess.pages.check()


def test_forked_samples_diverge_on_shared_pages(model):
    undisturbed = _session(model, kv_pages=PAGES, sampling=True)
    sess = _session(model, steps=10, kv_pages=PAGES, sampling=True)
    assert not torch.equal(sess.uniform[0], sess.uniform[1])
    p = int(sess.pos[0])
    sess.fork(0, 1, max_new_tokens=N - 11)
    _run(sess, N - 1 - 10)
    assert torch.equal(sess.hist[0], undisturbed.hist[0]) and torch.equal(sess.hist[2], undisturbed.hist[2])
    assert torch.equal(sess.hist[1, :p + 1], sess.hist[0, :p + 1])
    assert not torch.equal(sess.hist[1, p + 1:p + N - 11], sess.hist[0, p + 1:p + N - 11]), "the samples did not diverge"
    assert sess.pages.pages(1)[:2] == sess.pages.pages(0)[:2]
    assert sess.pos[1].item() == sess.pos[0].item()
    sess.pages.check()


def test_default_sessions_call_none_of_the_new_code(model, monkeypatch):
    from quantizations_amd import kv_pages, layer_ops
    from quantizations_amd.generation import SpeculativeSession

    calls = []
    for name in ("decode_attention_paged", "decode_attention_verify_paged", "prefill_attention_paged"):
        real = getattr(layer_ops, name)
        monkeypatch.setattr(layer_ops, name, lambda *a, _r=real, _n=name, **k: (calls.append(_n), _r(*a, **k))[1])
    monkeypatch.setattr(kv_pages, "KVPagePool", lambda *a, **k: calls.append("pool"))
    a = _session(model, steps=3)
    b = _session(model, steps=3, cls=SpeculativeSession, draft_tokens=2)
    a.admit(1, _tokens(20, 5), max_new_tokens=3)
    assert not calls and a.pages is None and b.pages is None and a._extra == {}
    monkeypatch.undo()
    calls = []
    for name in ("decode_attention_paged", "decode_attention_verify_paged", "prefill_attention_paged"):
        real = getattr(layer_ops, name)
        monkeypatch.setattr(layer_ops, name, lambda *a, _r=real, _n=name, **k: (calls.append(_n), _r(*a, **k))[1])
    _session(model, steps=2, graph=False, kv_pages=PAGES)
    _session(model, steps=2, graph=False, kv_pages=PAGES, cls=SpeculativeSession, draft_tokens=2)
    assert set(calls) == {"decode_attention_paged", "decode_attention_verify_paged", "prefill_attention_paged"}
