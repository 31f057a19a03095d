"""GPU: the sampled pick that accepts drafts (qz_verify_sample_step_streams,
layer_ops.verify_sample_step_streams).

Held four ways.  Bit for bit against the rule's own definition, successive sample_step_streams calls on
one stream and one row at a time, for seeded random u and any drafts: both sides run the same
arithmetic on the same row, so nothing is left out.  Against tests/verify_sample_reference.py on
verify_reference.accept_case's streams with targeted u (the fp64 midpoint of a CDF interval >= 1e-4
wide).  Against verify_step_streams for a stream with temperature 0 among sampled ones.  And against
the composed torch route.  accept_case has T + 4 streams, so its T = 16 case runs 320 rows (at V =
1000); every other case keeps B T <= 48."""
import numpy as np
import pytest
import torch
from sampling_reference import sample_reference
from streams_reference import SENTINEL
from test_gpu_sampling import ALL, FAMILIES, NARROW, family_row, laid_out
from verify_reference import accept_case, crafted_logits, verify_feedback
from verify_sample_reference import SAMPLING, STATE, expected, midpoint, row_picks, wide_tokens, window_case

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
RESULT = ("hist", "pos", "live", "tok", "accepted")
LAYOUT = {1000: "odd", 2056: "strided", 32000: "plain", 128256: "strided"}
MIX = [(0.8, 50, 0.9), (0.8, 7, 1.0), (0.0, 0, 1.0), (1.3, 0, 0.95), (0.8, 0, 1.0), (0.8, 0, 0.6)]


def _gpu(case):
    return {k: v.clone().to(DEV) for k, v in case.items() if k != "logits"}


def _run(logits, c, **kw):
    from quantizations_amd.layer_ops import verify_sample_step_streams

    verify_sample_step_streams(logits, *(c[k] for k in STATE), c["accepted"], *(c[k] for k in SAMPLING), **kw)
    torch.cuda.synchronize()


def _check(c, want, what):
    for name, w in zip(RESULT, want):
        got = c[name].cpu().numpy()
        assert np.array_equal(got, w), (what, name, got, w)


def _one_row_picks(logits, c, T):
    """picks [B, T] (numpy): row b T + i through sample_step_streams at position pos[b] + i, all streams
    live, nothing stopping them -- what each row draws, whatever becomes of it."""
    from quantizations_amd.layer_ops import sample_step_streams

    B, H = c["hist"].shape
    rows = torch.as_strided(logits, (B, T, logits.shape[1]), (T * logits.stride(0), logits.stride(0), 1))
    picks = torch.zeros((B, T), dtype=torch.int64, device=DEV)
    for i in range(T):
        one = torch.zeros(B, dtype=torch.int64, device=DEV)
        sample_step_streams(rows[:, i], torch.zeros((B, H), dtype=torch.int64, device=DEV), c["pos"] + i,
                            torch.ones(B, dtype=torch.int32, device=DEV), torch.full((B,), -1, dtype=torch.int64, device=DEV),
                            torch.full((B,), 1 << 40, dtype=torch.int64, device=DEV), one, *(c[k] for k in SAMPLING))
        picks[:, i] = one
    return picks.cpu().numpy()


def _host_loop(logits, c, T):
    """The definition: sample_step_streams on one stream and one row at a time, continued on the host
    while the stream stays live and its next draft is the token just written."""
    from quantizations_amd.layer_ops import sample_step_streams

    s = {k: v.clone() for k, v in c.items()}
    B = s["tok"].shape[0]
    emitted = [0] * B
    for b in range(B):
        for i in range(T):
            if int(s["live"][b]) == 0:
                break
            one = torch.full((1,), SENTINEL, dtype=torch.int64, device=DEV)
            sample_step_streams(logits[b * T + i:b * T + i + 1], s["hist"][b:b + 1], s["pos"][b:b + 1],
                                s["live"][b:b + 1], s["stop"][b:b + 1], s["limit"][b:b + 1], one,
                                *(s[k][b:b + 1] for k in SAMPLING))
            s["tok"][b, 0] = one[0]
            emitted[b] += 1
            if i + 1 < T and int(s["tok"][b, i + 1]) != int(one[0]):
                break
    return s, emitted


@pytest.mark.parametrize("name,V,T", [(n, V, T) for n in DTYPES for V in (1000, 2056, 32000) for T in (2, 4, 16)]
                         + [("fp16", 128256, 4)])
def test_bit_identity_with_the_one_row_pick(name, V, T):
    B, H = (3 if V == 128256 else min(6, 48 // T)), 24
    g = torch.Generator().manual_seed(V + T)
    logits = laid_out(torch.stack([family_row(FAMILIES[r % 3], V, DTYPES[name], g) for r in range(B * T)]), LAYOUT[V])
    rng = np.random.default_rng(V * T)
    temp, topk, topp = zip(*MIX[:B])
    pos = rng.permutation(H - T - 1)[:B].astype(np.int64)
    pos[B - 1] = H - 2                                   # rows 1.. of this stream read column H - 1 and write no history
    c = dict(hist=torch.full((B, H), SENTINEL, dtype=torch.int64), pos=torch.from_numpy(pos),
             live=torch.ones(B, dtype=torch.int32), stop=torch.full((B,), -1, dtype=torch.int64),
             limit=torch.full((B,), H + 100, dtype=torch.int64), tok=torch.zeros((B, T), dtype=torch.int64),
             accepted=torch.full((B,), SENTINEL, dtype=torch.int32), temperature=torch.tensor(temp),
             top_k=torch.tensor(topk, dtype=torch.int32), top_p=torch.tensor(topp),
             uniform=torch.from_numpy(rng.random((B, H), dtype=np.float32)))
    c = _gpu(c)
    picks = _one_row_picks(logits, c, T)
    c["stop"][0] = int(picks[0, min(1, T - 1)])          # a stop token inside an accepted run
    c["limit"][1] = int(pos[1]) + 2                      # a limit after two tokens
    c["tok"][:, 0] = torch.from_numpy(rng.integers(0, V, B)).to(DEV)
    wrong_at = list(range(1, T)) if T <= 4 else [1, T // 2, T - 1]
    seen = set()
    for variant in ["right", "all_wrong"] + wrong_at:
        drafts = picks[:, :-1].copy()
        if variant == "all_wrong":
            drafts = (drafts + 1) % V
        elif variant != "right":
            drafts[:, variant - 1] = (drafts[:, variant - 1] + 1) % V
        d = {k: v.clone() for k, v in c.items()}
        d["tok"][:, 1:] = torch.from_numpy(drafts).to(DEV)
        want, emitted = _host_loop(logits, d, T)
        _run(logits, d)
        for k in ("hist", "pos", "live"):
            assert torch.equal(d[k], want[k]), (variant, k, d[k].tolist(), want[k].tolist())
        assert d["tok"][:, 0].tolist() == want["tok"][:, 0].tolist(), variant
        assert d["accepted"].tolist() == emitted, (variant, d["accepted"].tolist(), emitted)
        assert torch.equal(d["tok"][:, 1:].cpu(), torch.from_numpy(drafts)), "the drafts are inputs"
        seen |= set(emitted)
    assert {1, min(2, T), T} <= seen, seen


@pytest.mark.parametrize("T,V", [(2, 1000), (4, 2056), (4, 32000), (16, 1000)])
@pytest.mark.parametrize("name", list(DTYPES))
def test_targeted_u_against_the_reference_native_and_composed(name, T, V):
    case, picks, accepted = window_case(T, V, DTYPES[name], seed=3 * T + V, settings=ALL, family_row=family_row,
                                        families=FAMILIES, greedy_stream=1)
    want = expected(case)
    assert np.array_equal(want[4], accepted), "the case is built to accept these counts"
    logits = laid_out(case["logits"], LAYOUT[V])
    c = _gpu(case)
    _run(logits, c)
    _check(c, want, "native")
    dead = T + 2
    assert c["tok"][dead].tolist() == [SENTINEL] * T and int(c["pos"][dead]) == int(case["pos"][dead])
    assert c["hist"][dead].tolist() == [SENTINEL] * case["hist"].shape[1]
    for k in SAMPLING + ("stop", "limit"):
        assert torch.equal(c[k].cpu(), case[k]), f"{k} is an input"
    d = _gpu(case)
    _run(logits, d, composed=True)
    _check(d, want, "composed")
    if V <= 2056:            # fp32 logits take the composed route by themselves
        e = _gpu(case)
        _run(logits.float(), e)
        _check(e, want, "fp32 logits")


def test_the_column_of_u():
    """Every row of a stream holds the same logits; column pos[b] + i targets the i-th wide token and
    every other column another one, so each pick tells which column was read.  The last stream starts
    at H - 2: its rows 1.. read column H - 1 and write no history, pos still advances."""
    T, V, H, B = 4, 2056, 12, 3
    g = torch.Generator().manual_seed(8)
    base = torch.stack([family_row("randn", V, torch.float16, g) for _ in range(B)])
    logits = base.repeat_interleave(T, 0).to(DEV)
    pos = np.array([0, 5, H - 2], dtype=np.int64)
    U = np.zeros((B, H), dtype=np.float32)
    picks = np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        ref = sample_reference(base[b].double().numpy(), 0.8, 50, 1.0)
        k = wide_tokens(ref)
        assert k.size > T + 1
        U[b, :] = midpoint(ref, k[T])
        for i in range(T):
            col = min(pos[b] + i, H - 1)
            if pos[b] + i <= H - 1:
                U[b, col] = midpoint(ref, k[i])
            picks[b, i] = k[i] if pos[b] + i <= H - 1 else k[H - 1 - pos[b]]
    tok = np.concatenate([np.zeros((B, 1), dtype=np.int64), picks[:, :-1]], 1)
    case = dict(hist=torch.full((B, H), SENTINEL, dtype=torch.int64), pos=torch.from_numpy(pos),
                live=torch.ones(B, dtype=torch.int32), stop=torch.full((B,), -1, dtype=torch.int64),
                limit=torch.full((B,), H + 9, dtype=torch.int64), tok=torch.from_numpy(tok),
                accepted=torch.zeros(B, dtype=torch.int32), temperature=torch.full((B,), 0.8),
                top_k=torch.full((B,), 50, dtype=torch.int32), top_p=torch.ones(B), uniform=torch.from_numpy(U))
    assert np.array_equal(row_picks(logits.cpu().double().numpy(), *(case[k].numpy() for k in SAMPLING), pos, T), picks)
    want = verify_feedback(picks, *(case[k].numpy() for k in STATE))
    assert want[4].tolist() == [T] * B and want[1].tolist() == (pos + T).tolist()
    assert want[0][2, H - 2:].tolist() == [picks[2, 0], picks[2, 1]], "positions past the history write nothing"
    for kw in ({}, dict(composed=True)):
        c = _gpu(case)
        _run(logits, c, **kw)
        _check(c, want, str(kw))


@pytest.mark.parametrize("name", list(DTYPES))
def test_a_greedy_stream_among_sampled_ones_gets_the_greedy_verify_result(name):
    """Even streams have temperature 0: their hist rows, pos, live, tok and accepted are
    verify_step_streams', with plain rows, with a tie at a later index, and with NaN rows (which make
    the sampled streams' rows greedy as well)."""
    from quantizations_amd.layer_ops import verify_step_streams

    T, V = 4, 2056
    case, picks, _ = accept_case(T, V, seed=17)
    B = T + 4
    cold = [b for b in range(B) if b % 2 == 0]
    for kw in ({}, dict(ties=True), dict(nan_rows=tuple(range(0, B * T, 3)))):
        logits = crafted_logits(picks, V, DTYPES[name], seed=18, **kw).to(DEV)
        gr = {k: v.clone().to(DEV) for k, v in case.items()}
        verify_step_streams(logits, *(gr[k] for k in STATE), gr["accepted"])
        c = _gpu(case)
        c.update(temperature=torch.tensor([0.0 if b % 2 == 0 else 0.8 for b in range(B)], device=DEV),
                 top_k=torch.full((B,), 50, dtype=torch.int32, device=DEV), top_p=torch.full((B,), 0.9, device=DEV),
                 uniform=torch.rand((B, 40), generator=torch.Generator().manual_seed(1)).to(DEV))
        _run(logits, c)
        for k in ("hist", "pos", "live", "accepted"):
            assert torch.equal(c[k][cold], gr[k][cold]), (kw, k)
        assert torch.equal(c["tok"][cold, 0], gr["tok"][cold, 0]), kw
        want = verify_feedback(picks, *(case[k].numpy() for k in STATE))
        assert np.array_equal(c["accepted"].cpu().numpy()[cold], want[4][cold])


@pytest.mark.parametrize("composed", [False, True], ids=["kernel", "composed"])
def test_a_captured_call_follows_new_values(composed):
    """Captured once; logits, temperature, top_k, top_p, uniform, tok, pos (and the rest of the state)
    changed in place: the replay gives the new case's reference result."""
    T, V, dtype = 4, 1000, torch.float16
    cases = [window_case(T, V, dtype, seed=s, settings=st, family_row=family_row, families=FAMILIES, greedy_stream=gs)
             for s, st, gs in ((41, NARROW, None), (42, ALL[3:], 2), (41, NARROW, None))]
    c = _gpu(cases[0][0])
    logits = cases[0][0]["logits"].to(DEV)

    def call():
        from quantizations_amd.layer_ops import verify_sample_step_streams

        verify_sample_step_streams(logits, *(c[k] for k in STATE), c["accepted"], *(c[k] for k in SAMPLING),
                                   composed=composed)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for case, _, accepted in cases:
        for k in STATE + SAMPLING + ("accepted",):
            c[k].copy_(case[k])
        logits.copy_(case["logits"])
        graph.replay()
        torch.cuda.synchronize()
        want = expected(case)
        assert np.array_equal(want[4], accepted)
        _check(c, want, "replay")
