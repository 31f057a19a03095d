"""GPU: quantizations_amd.generation.StreamSession and generate_ragged on the tiny random-init Llama
of test_gpu_generation.py (2 layers, hidden 256, vocab 4096, Linear4bit projections), built afresh
here: a prepared model and an unfused twin with the same weights.

Exact checks (the same kernels see the same rows): equal-length streams against DecodeSession,
greedy and sampled; a ragged run with and without the graph; rows that must not notice another
row's retirement and replacement; a stop token; generate_ragged's lengths.

One check cannot be exact: ragged greedy tokens against the unfused model.  The ragged prefill runs
at another token count than a solo run, and so possibly down another GEMM route.  It is held
teacher-forced: each returned sequence is fed to the unfused model alone; every generated token's
reference logit must be within `tol` of that position's maximum, and the token must be the strict
argmax wherever the reference's top-two gap is at least `tol`.  `tol` is measured in the fixture,
not chosen: twice the largest absolute logit difference between the shared-position decode path
(DecodeSession's forward, as it was before this file existed) and the unfused model, teacher-forced
over the same tokens on this same model -- twice, because two independently rounded paths are
compared.  Measured on an MI355X: d = 0.001099, so
tol = 0.002197; with the prompt seed below (3) the unfused model alone has a top-two gap of at least
tol on 67 of the 72 generated positions (93 %; the test asserts at least 90 %), and the largest
shortfall of a picked token below its position's maximum was 0.00098."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
S, N = 8, 24
LENGTHS = [8, 3, 5]
SENT = -5


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


def _decode_path_logits(model, ids, n):
    """The shared-position decode path, greedy: (sequence [B, s + n], the logits [B, n, V] that
    picked its new tokens)."""
    from transformers.cache_utils import StaticCache

    B, s = ids.shape
    cache = StaticCache(config=model.config, max_cache_len=s + n + 2)
    pos = torch.tensor([s - 1], device=DEV)
    seq, logits = [ids], []
    with torch.inference_mode():
        lo = model(input_ids=ids, past_key_values=cache, cache_position=torch.arange(s, device=DEV),
                   use_cache=True).logits[:, -1]
        for _ in range(n):
            logits.append(lo.float().clone())
            tok = lo.argmax(-1, keepdim=True)
            seq.append(tok)
            pos += 1
            lo = model(input_ids=tok, past_key_values=cache, cache_position=pos,
                       position_ids=pos.view(1, 1).expand(B, 1), use_cache=True).logits[:, -1]
    return torch.cat(seq, 1), torch.stack(logits, 1)


@pytest.fixture(scope="module")
def tiny():
    """(prepared model, unfused twin, prompts [3, S], tol)"""
    from quantizations_amd.generation import prepare_for_decode

    ref = _build()
    model = _build()
    ids = torch.randint(0, 4096, (3, S), generator=torch.Generator().manual_seed(1)).to(DEV)
    prepare_for_decode(model)
    try:
        seq, lo = _decode_path_logits(model, ids, N)
        with torch.inference_mode():
            want = torch.stack([ref(input_ids=seq[b:b + 1]).logits[0, S - 1:S + N - 1].float() for b in range(3)])
        d = float((lo - want).abs().max())
        print(f"decode path vs unfused model: largest |logit difference| d = {d:.6f}, tol = {2 * d:.6f}")
        assert 0 < d < 1.0, d    # a sanity bracket around the measurement, not the bar
        yield model, ref, ids, 2 * d
    finally:
        _unprepare(model)


def _run(sess, steps):
    for _ in range(steps):
        sess.step()
    torch.cuda.synchronize()


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_equal_lengths_equal_decode_session(tiny, sampled):
    from quantizations_amd.generation import DecodeSession, StreamSession

    model, _, ids, _ = tiny
    out = []
    for cls in (DecodeSession, StreamSession):
        sess = cls(model, 3, S + N)
        if sampled:
            sess.set_sampling(temperature=[0.0, 0.8, 1.2], top_k=[0, 50, 0], top_p=[1.0, 0.9, 0.95])
            sess.seed(1234)
        if cls is DecodeSession:
            sess.prefill(ids)
        else:
            sess.prefill(ids, [S] * 3)
        _run(sess, N - 1)
        out.append(sess.hist.clone())
    assert torch.equal(out[0], out[1])
    assert sess.pos.tolist() == [S + N - 1] * 3 and not bool(sess.alive().any())   # every stream reached its limit
    assert len(set(out[1][:, S:].reshape(-1).tolist())) > 3      # not a constant


def _ragged(model, graph, sampled=False, steps=N - 1, **prefill_kw):
    """Three streams of LENGTHS, N new tokens each (the last step retires all of them) unless told otherwise."""
    from quantizations_amd.generation import StreamSession

    prefill_kw.setdefault("max_new_tokens", N)

    g = torch.Generator().manual_seed(3)
    Smax = max(LENGTHS)
    ids = torch.randint(0, 4096, (3, Smax), generator=g).to(DEV)
    sess = StreamSession(model, 3, Smax + N, graph=graph)
    if sampled:
        sess.set_sampling(temperature=[0.9, 0.0, 1.1], top_k=[40, 0, 0], top_p=[0.95, 1.0, 0.9])
        sess.seed(99)
    sess.hist.fill_(SENT)
    sess.prefill(ids, LENGTHS, **prefill_kw)
    _run(sess, steps)
    return sess, ids


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_ragged_graph_equals_eager(tiny, sampled):
    model = tiny[0]
    a, ids = _ragged(model, True, sampled)
    b, _ = _ragged(model, False, sampled)
    assert torch.equal(a.hist, b.hist) and torch.equal(a.pos, b.pos) and torch.equal(a.live, b.live)
    # every stream grew from its own length: the prompt, N new tokens, nothing after; pads never stored
    for r, n in enumerate(LENGTHS):
        assert torch.equal(a.hist[r, :n], ids[r, :n]) and bool((a.hist[r, n:n + N] != SENT).all())
        assert bool((a.hist[r, n + N:] == SENT).all())
    assert a.pos.tolist() == [n + N - 1 for n in LENGTHS] and not bool(a.alive().any())


def test_ragged_greedy_tokens_against_the_unfused_model(tiny):
    model, ref, _, tol = tiny
    sess, ids = _ragged(model, True)
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


def test_a_retired_row_is_readmitted_without_recapture_or_disturbing_the_others(tiny):
    from quantizations_amd.generation import StreamSession

    model = tiny[0]
    undisturbed, ids = _ragged(model, True)
    newcomer = torch.randint(0, 4096, (6,), generator=torch.Generator().manual_seed(8))

    def scenario(graph):
        sess = StreamSession(model, 3, max(LENGTHS) + N, graph=graph)
        sess.hist.fill_(SENT)
        sess.prefill(ids, LENGTHS, max_new_tokens=[N, 4, N])       # stream 1 retires by its limit
        _run(sess, 6)
        captured = sess._graph
        assert (captured is not None) == graph and sess.alive().tolist() == [True, False, True]
        assert sess.pos[1].item() == LENGTHS[1] + 3 and bool((sess.hist[1, LENGTHS[1] + 4:] == SENT).all())
        assert torch.equal(sess.hist[1, :LENGTHS[1] + 4], undisturbed.hist[1, :LENGTHS[1] + 4])
        sess.admit(1, newcomer, max_new_tokens=7)
        assert sess.alive().tolist() == [True, True, True] and sess.pos[1].item() == 6
        _run(sess, N - 1 - 6)
        assert sess._graph is captured, "no recapture"
        return sess

    sess = scenario(True)
    for r in (0, 2):
        assert torch.equal(sess.hist[r], undisturbed.hist[r])
    assert sess.pos.tolist() == [LENGTHS[0] + N - 1, 6 + 7 - 1, LENGTHS[2] + N - 1]
    assert torch.equal(sess.hist[1, :6].cpu(), newcomer) and bool((sess.hist[1, 6:13] != SENT).all())
    # the newcomer's row: the replayed steps and eager ones pick the same tokens
    assert torch.equal(sess.hist, scenario(False).hist)


def test_a_stream_stops_after_writing_its_stop_token(tiny):
    model = tiny[0]
    free, _ = _ragged(model, True)
    n = LENGTHS[1]
    stop = int(free.hist[1, n + 5])
    first = int((free.hist[1, n:] == stop).nonzero()[0])
    sess, _ = _ragged(model, True, stop=[-1, stop, -1])
    assert sess.alive().tolist() == [False, False, False]          # 0 and 2 by their limits, at the last step
    assert sess.pos.tolist() == [LENGTHS[0] + N - 1, n + first, LENGTHS[2] + N - 1]
    assert torch.equal(sess.hist[1, :n + first + 1], free.hist[1, :n + first + 1]) and sess.hist[1, n + first] == stop
    assert bool((sess.hist[1, n + first + 1:] == SENT).all())
    for r in (0, 2):
        assert torch.equal(sess.hist[r], free.hist[r])
    part, _ = _ragged(model, True, steps=first + 2, stop=[-1, stop, -1])
    assert part.alive().tolist() == [True, False, True]


def test_generate_ragged_returns_each_prompts_own_length(tiny):
    from quantizations_amd.generation import generate_ragged

    model = tiny[0]
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 4096, (3, max(LENGTHS)), generator=g)
    prompts = [ids[b, :n] for b, n in enumerate(LENGTHS)]
    n_new = 40
    free = generate_ragged(model, prompts, n_new)
    assert [t.numel() for t in free] == [n + n_new for n in LENGTHS] and all(t.dtype == torch.int64 for t in free)
    assert all(torch.equal(t[:n].cpu(), p) for t, p, n in zip(free, prompts, LENGTHS))
    assert all(torch.equal(a, b) for a, b in zip(free, generate_ragged(model, prompts, n_new, graph=False)))
    eos = int(free[0][LENGTHS[0] + 5])
    out = generate_ragged(model, prompts, n_new, eos_token_id=eos)
    for b, n in enumerate(LENGTHS):
        hit = (free[b][n:] == eos).nonzero()
        want = free[b][:n + int(hit[0]) + 1] if hit.numel() else free[b]
        assert torch.equal(out[b], want), b
    assert out[0].numel() <= LENGTHS[0] + 6 and out[0][-1] == eos
    kw = dict(do_sample=True, temperature=[0.0, 0.8, 1.2], top_k=[0, 50, 0], top_p=[1.0, 0.9, 0.95], generator=5)
    sampled = generate_ragged(model, prompts, 12, **kw)
    assert torch.equal(sampled[0], free[0][:LENGTHS[0] + 12]) and not torch.equal(sampled[1], free[1][:LENGTHS[1] + 12])
    assert all(torch.equal(a, b) for a, b in zip(sampled, generate_ragged(model, prompts, 12, graph=False, **kw)))


def test_what_the_session_and_the_layer_refuse(tiny):
    from transformers.cache_utils import StaticCache

    from quantizations_amd.generation import StreamSession

    model, ref, ids, _ = tiny
    with pytest.raises(ValueError, match="prepare_for_decode"):
        StreamSession(ref, 3, 16)
    sess = StreamSession(model, 3, S + 4)
    with pytest.raises(ValueError):
        sess.step()                                            # prefill first
    with pytest.raises(ValueError):
        sess.admit(0, ids[0])
    with pytest.raises(ValueError):
        sess.prefill(ids, [S, S, S + 1])                       # a length past Smax
    with pytest.raises(ValueError):
        sess.prefill(ids, [S, 0, S])
    with pytest.raises(ValueError):
        sess.prefill(ids, [S] * 3, max_new_tokens=5)           # no room
    sess.prefill(ids, [S] * 3)
    with pytest.raises(ValueError):
        sess.prefill(ids, [S] * 3)
    with pytest.raises(ValueError):
        sess.admit(3, ids[0])
    with pytest.raises(ValueError):
        sess.admit(0, ids[0], max_new_tokens=9)
    # the layer never falls to the shared-position path: per-stream positions against an fp32 cache raise
    cache = StaticCache(config=model.config, max_cache_len=16)
    pos = torch.tensor([3, 1, 2], device=DEV)
    with torch.inference_mode(), pytest.raises(ValueError, match="_qz_stream_pos"):
        model(input_ids=ids[:, :1], past_key_values=cache, position_ids=pos.view(3, 1), use_cache=True,
              _qz_stream_pos=pos)                              # a cache no prefill has laid out
    with torch.inference_mode(), pytest.raises(ValueError, match="_qz_stream_pos"):
        model(input_ids=ids[:, :2], past_key_values=sess.cache, position_ids=pos.view(3, 1).expand(3, 2),
              use_cache=True, _qz_stream_pos=pos)              # two tokens per stream
