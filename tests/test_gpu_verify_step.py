"""GPU: the greedy pick that accepts drafts (qz_verify_step_streams, layer_ops.verify_step_streams) and
the prompt-lookup drafter (qz_ngram_draft, layer_ops.ngram_draft).

The pick is held three ways: against tests/verify_reference.py's numpy restatement, against T
successive greedy_step_streams launches on each stream alone (the rule's own definition), and against
the composed torch route.  The crafted batch (verify_reference.accept_case) has streams with 0, 1, ...,
T - 1 matching drafts, a stop token in the middle of an accepted run, a limit reached in the middle
of a run, a dead stream among sentinels and a stream that accepts everything.  The drafter is held
against the numpy rule on crafted histories and on random ones over a two-letter alphabet."""
import numpy as np
import pytest
import torch
from streams_reference import SENTINEL
from verify_reference import DRAFT_CASES, accept_case, crafted_logits, draft_rule, verify_feedback

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
KEYS = ("hist", "pos", "live", "stop", "limit", "tok", "accepted")


def _gpu(case):
    return {k: v.clone().to(DEV) for k, v in case.items()}


def _run(logits, c, **kw):
    from quantizations_amd.layer_ops import verify_step_streams

    verify_step_streams(logits, *(c[k] for k in KEYS), **kw)
    torch.cuda.synchronize()


def _check(c, want, what):
    for name, w in zip(("hist", "pos", "live", "tok", "accepted"), want):
        got = c[name].cpu().numpy()
        assert np.array_equal(got, w), (what, name, got, w)


@pytest.mark.parametrize("V,T", [(1000, 2), (1000, 4), (4096, 4), (4096, 8), (128256, 3)])
@pytest.mark.parametrize("name", list(DTYPES))
def test_accept_rule_against_the_numpy_restatement_and_the_composed_route(name, V, T):
    case, picks, accepted = accept_case(T, V, seed=V + T)
    logits = crafted_logits(picks, V, DTYPES[name], seed=T).to(DEV)
    if V == 1000:      # a row stride above the row length
        wide = torch.full((logits.shape[0], V + 24), 99.0, dtype=logits.dtype, device=DEV)
        wide[:, :V] = logits
        logits = wide[:, :V]
    want = verify_feedback(picks, *(case[k].numpy() for k in KEYS[:-1]))
    assert np.array_equal(want[4], accepted), "the case is built to accept these counts"
    c = _gpu(case)
    _run(logits, c)
    _check(c, want, "native")
    assert int(c["tok"][T + 2, 0]) == SENTINEL and int(c["pos"][T + 2]) == int(case["pos"][T + 2])   # the dead stream
    d = _gpu(case)
    _run(logits, d, composed=True)
    _check(d, want, "composed")


@pytest.mark.parametrize("name", list(DTYPES))
def test_accept_rule_against_sequential_streams_picks(name):
    """The definition itself: greedy_step_streams on one stream and one row at a time, continued on
    the host while the stream stays live and its next draft is the token just written."""
    from quantizations_amd.layer_ops import greedy_step_streams

    T, V = 4, 4096
    case, picks, _ = accept_case(T, V, seed=5)
    logits = crafted_logits(picks, V, DTYPES[name], seed=6).to(DEV)
    c = _gpu(case)
    _run(logits, c)
    s = _gpu(case)
    B = s["tok"].shape[0]
    emitted = [0] * B
    for b in range(B):
        for i in range(T):
            if int(s["live"][b]) == 0:
                break
            one = torch.full((1,), SENTINEL, dtype=torch.int64, device=DEV)
            greedy_step_streams(logits[b * T + i:b * T + i + 1], s["hist"][b:b + 1], s["pos"][b:b + 1],
                                s["live"][b:b + 1], s["stop"][b:b + 1], s["limit"][b:b + 1], one)
            s["tok"][b, 0] = one[0]
            emitted[b] += 1
            if i + 1 < T and int(s["tok"][b, i + 1]) != int(one[0]):
                break
    torch.cuda.synchronize()
    for k in ("hist", "pos", "live", "tok"):
        assert torch.equal(c[k], s[k]), k
    assert c["accepted"].tolist() == emitted


@pytest.mark.parametrize("name", list(DTYPES))
def test_ties_take_the_first_index_and_nan_ranks_above_every_number(name):
    T, V = 4, 4096
    case, picks, _ = accept_case(T, V, seed=11)
    want = verify_feedback(picks, *(case[k].numpy() for k in KEYS[:-1]))
    for kw in (dict(ties=True), dict(nan_rows=tuple(range(0, (T + 4) * T, 3)))):
        logits = crafted_logits(picks, V, DTYPES[name], seed=12, **kw).to(DEV)
        assert torch.equal(logits.argmax(-1).cpu(), torch.from_numpy(picks.reshape(-1))), "torch.argmax agrees"
        c = _gpu(case)
        _run(logits, c)
        _check(c, want, str(kw))


def test_invariant_an_emitted_row_lies_inside_the_limit():
    """limit[b] <= L - 1 and an emitted row i has p_b + i + 1 <= limit[b]: windows that start close to
    their limit accept everything the drafts offer and still stop at the limit."""
    T, V, H = 8, 1000, 64
    rng = np.random.default_rng(3)
    B = T
    picks = np.stack([rng.permutation(V)[:T] for _ in range(B)]).astype(np.int64)
    tok = np.concatenate([rng.integers(0, V, (B, 1)), picks[:, :-1]], 1).astype(np.int64)
    limit = np.full(B, H - 1, dtype=np.int64)
    pos = (H - 1 - np.arange(1, B + 1)).astype(np.int64)          # 1 .. T tokens of room
    case = dict(hist=torch.full((B, H), SENTINEL, dtype=torch.int64), pos=torch.from_numpy(pos),
                live=torch.ones(B, dtype=torch.int32), stop=torch.full((B,), -1, dtype=torch.int64),
                limit=torch.from_numpy(limit), tok=torch.from_numpy(tok),
                accepted=torch.zeros(B, dtype=torch.int32))
    c = _gpu(case)
    _run(crafted_logits(picks, V, torch.float16, seed=1).to(DEV), c)
    acc = c["accepted"].cpu().numpy()
    assert acc.tolist() == list(range(1, B + 1))
    assert bool((pos + acc <= limit).all()) and c["live"].tolist() == [0] * B
    assert bool((c["pos"].cpu().numpy() == limit).all())


def test_a_captured_pick_and_drafter_follow_new_state():
    from quantizations_amd.layer_ops import ngram_draft, verify_step_streams

    T, V = 4, 1000
    case, picks, _ = accept_case(T, V, seed=21)
    c = _gpu(case)
    logits = crafted_logits(picks, V, torch.float16, seed=22).to(DEV)
    pos_ids = torch.zeros_like(c["tok"])

    def both():
        verify_step_streams(logits, *(c[k] for k in KEYS))
        ngram_draft(c["hist"], c["pos"], c["tok"], pos_ids, 3)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        both()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both()
    for seed in (21, 33):
        case2, picks2, _ = accept_case(T, V, seed=seed)
        for k in KEYS:
            c[k].copy_(case2[k])
        logits.copy_(crafted_logits(picks2, V, torch.float16, seed=seed + 1))
        g.replay()
        torch.cuda.synchronize()
        got = {k: v.clone() for k, v in c.items()}
        e = _gpu(case2)
        e_ids = torch.zeros_like(pos_ids)
        verify_step_streams(logits, *(e[k] for k in KEYS))
        ngram_draft(e["hist"], e["pos"], e["tok"], e_ids, 3)
        torch.cuda.synchronize()
        want = verify_feedback(picks2, *(case2[k].numpy() for k in KEYS[:-1]))
        assert np.array_equal(got["pos"].cpu().numpy(), want[1]) and np.array_equal(got["accepted"].cpu().numpy(), want[4])
        for k in KEYS:
            assert torch.equal(got[k], e[k]), k
        assert torch.equal(pos_ids, e_ids)


def _draft(hists, ps, T, ngram_max, composed=False):
    """Run the drafter on histories of different lengths (padded with sentinels above p)."""
    from quantizations_amd.layer_ops import ngram_draft

    B, H = len(hists), max(len(h) for h in hists) + 3
    hist = torch.full((B, H), SENTINEL, dtype=torch.int64)
    for b, h in enumerate(hists):
        hist[b, :len(h)] = torch.tensor(h)
    tok = torch.full((B, T), SENTINEL, dtype=torch.int64)
    tok[:, 0] = torch.tensor([h[p] for h, p in zip(hists, ps)])
    pos = torch.tensor(ps, dtype=torch.int64)
    hist, tok, pos = hist.to(DEV), tok.to(DEV), pos.to(DEV)
    pos_ids = torch.full((B, T), SENTINEL, dtype=torch.int64, device=DEV)
    hist0 = hist.clone()
    ngram_draft(hist, pos, tok, pos_ids, ngram_max, composed=composed)
    torch.cuda.synchronize()
    assert torch.equal(hist, hist0) and pos.tolist() == list(ps), "inputs unchanged"
    assert pos_ids.tolist() == [[p + i for i in range(T)] for p in ps]
    assert tok[:, 0].tolist() == [h[p] for h, p in zip(hists, ps)]
    return tok[:, 1:].tolist()


@pytest.mark.parametrize("composed", [False, True], ids=["native", "composed"])
@pytest.mark.parametrize("name", list(DRAFT_CASES))
def test_drafter_on_crafted_histories(name, composed):
    s, ngram_max, T, want = DRAFT_CASES[name]
    assert draft_rule(s, len(s) - 1, s[-1], T, ngram_max) == want, "the restatement agrees with the hand-made case"
    # the same stream beside a neighbour with another history: one workgroup per stream
    got = _draft([s, [1, 1, 2, 1, 1]], [len(s) - 1, 4], T, ngram_max, composed)
    assert got[0] == want and got[1] == draft_rule([1, 1, 2, 1, 1], 4, 1, T, ngram_max)


@pytest.mark.parametrize("ngram_max", [1, 2, 3, 4])
def test_drafter_on_random_histories(ngram_max):
    """Two letters make every kind of match common; lengths up to 700 give a thread several starts."""
    rng = np.random.default_rng(ngram_max)
    T = 6
    hists = [rng.integers(0, 2, n).tolist() for n in (1, 2, 3, 5, 17, 255, 256, 257, 300, 700)]
    hists += [rng.integers(0, 50, n).tolist() for n in (40, 300, 700)]
    ps = [len(h) - 1 for h in hists]
    got = _draft(hists, ps, T, ngram_max)
    for h, p, g in zip(hists, ps, got):
        assert g == draft_rule(h, p, h[p], T, ngram_max), (len(h), g)
    # a position below the end of what hist holds: the tokens above p are not history
    ps2 = [max(0, p // 2) for p in ps]
    got = _draft(hists, ps2, T, ngram_max)
    for h, p, g in zip(hists, ps2, got):
        assert g == draft_rule(h, p, h[p], T, ngram_max), (len(h), p, g)


def test_wrappers_reject_what_they_cannot_take():
    from quantizations_amd.layer_ops import ngram_draft, verify_step_streams

    T, V = 4, 1000
    case, picks, _ = accept_case(T, V, seed=2)
    c = _gpu(case)
    logits = crafted_logits(picks, V, torch.float16, seed=2).to(DEV)
    before = {k: v.clone() for k, v in c.items()}
    for bad in (dict(tok=c["tok"][:, 0]), dict(tok=c["tok"].int()), dict(accepted=c["accepted"].long()),
                dict(pos=c["pos"][:3]), dict(live=c["live"].cpu()), dict(hist=c["hist"][:, ::2])):
        a = dict(c)
        a.update(bad)
        with pytest.raises(ValueError):
            verify_step_streams(logits, *(a[k] for k in KEYS))
    with pytest.raises(ValueError):
        verify_step_streams(logits[:-1], *(c[k] for k in KEYS))
    ids = torch.zeros_like(c["tok"])
    for args in ((c["hist"], c["pos"], c["tok"], ids, 0), (c["hist"], c["pos"], c["tok"], ids, 5),
                 (c["hist"], c["pos"], c["tok"], ids[:, :2], 3), (c["hist"], c["pos"][:2], c["tok"], ids, 3),
                 (c["hist"].int(), c["pos"], c["tok"], ids, 3)):
        with pytest.raises(ValueError):
            ngram_draft(*args)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(c[k], before[k]), k
