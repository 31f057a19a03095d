"""CPU: the composed route of layer_ops.verify_sample_step_streams against
tests/verify_sample_reference.py on targeted cases (every row's u is the fp64 midpoint of a CDF
interval >= 1e-4 wide: no random draw, nothing left out), a proof on the reference alone that the rule
emits the one-token sampler's tokens whatever the drafts were, and the wrapper's argument errors."""
import numpy as np
import pytest
import torch
from sampling_reference import pick, sample_reference
from streams_reference import SENTINEL
from test_gpu_sampling import ALL, FAMILIES, family_row
from verify_reference import verify_feedback
from verify_sample_reference import SAMPLING, STATE, expected, row_picks, window_case

RESULT = ("hist", "pos", "live", "tok", "accepted")


def run(case, logits=None, **kw):
    from quantizations_amd.layer_ops import verify_sample_step_streams

    c = {k: v.clone() for k, v in case.items()}
    verify_sample_step_streams(c["logits"] if logits is None else logits, *(c[k] for k in STATE), c["accepted"],
                               *(c[k] for k in SAMPLING), **kw)
    return c


@pytest.mark.parametrize("T,V", [(2, 1000), (4, 2056), (16, 1000), (4, 32000)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["fp32", "fp16", "bf16"])
def test_composed_route_against_the_reference(dtype, T, V):
    """fp32: the fp16 rows widened, so the reference's rows are the same numbers."""
    src = torch.float16 if dtype == torch.float32 else dtype
    case, picks, accepted = window_case(T, V, src, seed=T + V, settings=ALL, family_row=family_row, families=FAMILIES,
                                        greedy_stream=1)
    want = expected(case)
    assert np.array_equal(want[4], accepted), "the case is built to accept these counts"
    assert np.array_equal(row_picks(case["logits"].double().numpy(), *(case[k].numpy() for k in SAMPLING),
                                    case["pos"].numpy(), T), picks), "the midpoints draw the targets"
    got = run(case, case["logits"].to(dtype))
    for name, w in zip(RESULT, want):
        assert np.array_equal(got[name].numpy(), w), name
    dead = T + 2
    assert got["tok"][dead].tolist() == [SENTINEL] * T and got["hist"][dead].tolist() == [SENTINEL] * 40
    for k in SAMPLING + ("stop", "limit"):
        assert torch.equal(got[k], case[k]), f"{k} is an input"


V_TOY, N_TOY = 50, 64


def _toy_rows():
    """The toy model: a fixed table of logits rows; the row after (..., a, b) is table[hash(a, b)]."""
    table = (np.random.default_rng(5).standard_normal((N_TOY, V_TOY)) * 3).astype(np.float16).astype(np.float64)
    return [sample_reference(z, 0.8, 20, 0.9) for z in table]


def _toy_ref(refs, a, b):
    return refs[(int(a) * 31 + int(b) * 17 + 3) % N_TOY]


def _decode_one_by_one(refs, prompt, M, U):
    seq = list(prompt)
    for _ in range(M):
        seq.append(pick(_toy_ref(refs, seq[-2], seq[-1]), U[len(seq) - 1]))   # index q is drawn with U[q - 1]
    return seq


def _decode_by_windows(refs, prompt, M, U, T, drafter):
    """The verify rule on the reference alone: pos is the index of the newest token, the pick feedback
    writes the shifted history (column p is sequence index p + 1), row i is drawn with U[pos + i]."""
    H = len(prompt) + M
    nxt = np.full((1, H), SENTINEL, dtype=np.int64)
    seq = list(prompt)
    pos = np.array([len(prompt) - 1], dtype=np.int64)
    live = np.ones(1, dtype=np.int32)
    stop = np.full(1, -1, dtype=np.int64)
    limit = np.array([len(prompt) + M - 1], dtype=np.int64)
    steps = 0
    while live[0]:
        drafts = drafter(seq, T - 1)
        tok = np.array([[seq[-1]] + drafts], dtype=np.int64)
        ctx = seq + drafts
        p = int(pos[0])
        picks = np.array([[pick(_toy_ref(refs, ctx[p + i - 1], ctx[p + i]), U[min(p + i, len(U) - 1)])
                           for i in range(T)]], dtype=np.int64)
        nxt, pos, live, tok, acc = verify_feedback(picks, nxt, pos, live, stop, limit, tok)
        seq = list(prompt) + nxt[0, len(prompt) - 1:int(pos[0])].tolist()
        assert seq[-1] == tok[0, 0] and len(seq) == p + 1 + acc[0]
        steps += 1
    return seq, steps


@pytest.mark.parametrize("T", [2, 4, 5])
def test_the_rule_emits_the_one_token_samplers_tokens_whatever_the_drafts(T):
    refs = _toy_rows()
    M, prompt = 37, [3, 11]
    U = np.random.default_rng(T).random(len(prompt) + M).astype(np.float32)
    truth = _decode_one_by_one(refs, prompt, M, U)
    assert len(set(truth[2:])) > 5, "the toy model samples (it is not one token over and over)"
    rng = np.random.default_rng(9)

    def all_wrong(seq, n):
        ctx, out = list(seq), []
        for _ in range(n):        # never the token the row before will draw
            q = len(ctx) - 1
            right = pick(_toy_ref(refs, ctx[-2], ctx[-1]), U[min(q, len(U) - 1)])
            out.append((right + 1) % V_TOY)
            ctx.append(out[-1])
        return out

    def random(seq, n):
        return [int(x) for x in rng.integers(0, V_TOY, n)]

    def replay(seq, n):
        tail = truth[len(seq):len(seq) + n]
        return tail + [0] * (n - len(tail))

    seq, steps = _decode_by_windows(refs, prompt, M, U, T, all_wrong)
    assert seq == truth and steps == M
    seq, steps = _decode_by_windows(refs, prompt, M, U, T, random)
    assert seq == truth and steps <= M
    seq, steps = _decode_by_windows(refs, prompt, M, U, T, replay)
    assert seq == truth and steps == -(-M // T)


def test_argument_errors():
    from quantizations_amd.layer_ops import verify_sample_step_streams

    B, T, V, H = 2, 3, 16, 8

    def args(**kw):
        a = dict(logits=torch.zeros(B * T, V), hist=torch.zeros((B, H), dtype=torch.int64),
                 pos=torch.zeros(B, dtype=torch.int64), live=torch.ones(B, dtype=torch.int32),
                 stop=torch.full((B,), -1, dtype=torch.int64), limit=torch.full((B,), H, dtype=torch.int64),
                 tok=torch.zeros((B, T), dtype=torch.int64), accepted=torch.zeros(B, dtype=torch.int32),
                 temperature=torch.ones(B), top_k=torch.zeros(B, dtype=torch.int32), top_p=torch.ones(B),
                 uniform=torch.zeros((B, H)))
        a.update(kw)
        return [a[k] for k in ("logits",) + STATE + ("accepted",) + SAMPLING]

    verify_sample_step_streams(*args())
    bad = [
        ("logits", dict(logits=torch.zeros(B * T + 1, V))),
        ("logits", dict(logits=torch.zeros(V, B * T).t())),
        ("tok", dict(tok=torch.zeros((B, 17), dtype=torch.int64), logits=torch.zeros(B * 17, V))),
        ("tok", dict(tok=torch.zeros(B * T, dtype=torch.int64))),
        ("tok", dict(tok=torch.zeros((B, T), dtype=torch.int32))),
        ("accepted", dict(accepted=torch.zeros(B, dtype=torch.int64))),
        ("accepted", dict(accepted=torch.zeros(B + 1, dtype=torch.int32))),
        ("live", dict(live=torch.ones(B, dtype=torch.int64))),
        ("pos", dict(pos=torch.zeros(B + 1, dtype=torch.int64))),
        ("hist", dict(hist=torch.zeros((B + 1, H), dtype=torch.int64), uniform=torch.zeros((B + 1, H)))),
        ("temperature", dict(temperature=torch.ones(B * T))),
        ("temperature", dict(temperature=torch.ones(B, dtype=torch.float64))),
        ("top_k", dict(top_k=torch.zeros(B, dtype=torch.int64))),
        ("top_p", dict(top_p=torch.ones(B + 1))),
        ("top_p", dict(top_p=None)),
        ("uniform", dict(uniform=torch.zeros((B, H + 1)))),
        ("uniform", dict(uniform=torch.zeros((B, H), dtype=torch.float64))),
        ("uniform", dict(uniform=torch.zeros((H, B)).t())),
    ]
    for what, kw in bad:
        with pytest.raises(ValueError, match=f"verify_sample_step_streams.*{what}"):
            verify_sample_step_streams(*args(**kw))
    # nothing to do: no stream, or an empty vocabulary
    verify_sample_step_streams(torch.zeros(0, V), *(t[:0] for t in args()[1:]))
    a = args(logits=torch.zeros(B * T, 0))
    verify_sample_step_streams(*a)
    assert a[6].tolist() == [[0] * T] * B and a[7].tolist() == [0] * B
