"""CPU: the composed torch routes of layer_ops.greedy_step_streams / sample_step_streams against the
numpy statement of their rules (tests/streams_reference.py over tests/sampling_reference.py), with a
position, liveness, stop token and limit per stream; and what StreamSession / generate_ragged refuse
without a GPU."""
import numpy as np
import pytest
import torch
from streams_reference import SENTINEL, build_case, expected

H = 12


def _clone(case):
    return {k: v.clone() for k, v in case.items()}


def _same(c, want):
    hist, pos, live, tok = want
    assert np.array_equal(c["hist"].numpy(), hist), np.argwhere(c["hist"].numpy() != hist)[:8]
    assert np.array_equal(c["pos"].numpy(), pos) and np.array_equal(c["live"].numpy(), live)
    assert np.array_equal(c["tok"].numpy(), tok)


@pytest.mark.parametrize("V,B", [(1000, 1), (1000, 4), (2056, 6)])
def test_composed_sample_step_streams_equals_the_reference(V, B):
    from quantizations_amd.layer_ops import sample_step_streams

    case, tokens = build_case(V, B, H, torch.float32, seed=V + B)
    c = _clone(case)
    sample_step_streams(c["logits"], c["hist"], c["pos"], c["live"], c["stop"], c["limit"], c["tok"],
                        c["temperature"], c["top_k"], c["top_p"], c["uniform"])
    want = expected(case, tokens)
    _same(c, want)
    if B >= 4:
        # the stop token and the limit clear `live` after the write; the dead row kept its sentinels
        p = case["pos"].numpy()
        assert want[2][1] == 0 and want[0][1, p[1]] == tokens[1]
        assert want[2][2] == 0 and want[0][2, p[2]] == tokens[2]
        assert (want[0][3] == SENTINEL).all() and want[3][3] == SENTINEL and want[1][3] == p[3]
    # a second call moves the survivors only (their u is now outside [0, 1): the last kept index)
    before = _clone(c)
    sample_step_streams(c["logits"], c["hist"], c["pos"], c["live"], c["stop"], c["limit"], c["tok"],
                        c["temperature"], c["top_k"], c["top_p"], c["uniform"])
    dead = before["live"].numpy() == 0
    assert np.array_equal(c["hist"].numpy()[dead], before["hist"].numpy()[dead])
    assert np.array_equal(c["pos"].numpy()[dead], before["pos"].numpy()[dead])
    assert np.array_equal(c["pos"].numpy()[~dead], before["pos"].numpy()[~dead] + 1)


@pytest.mark.parametrize("V,B", [(1000, 1), (1000, 4), (2056, 6)])
def test_composed_greedy_step_streams_equals_the_reference(V, B):
    from quantizations_amd.layer_ops import greedy_step_streams

    case, tokens = build_case(V, B, H, torch.float32, seed=3 * V + B)
    if B > 1:   # row 1 stops on ITS greedy token
        case["stop"][1] = int(case["logits"][1].argmax())
    c = _clone(case)
    greedy_step_streams(c["logits"], c["hist"], c["pos"], c["live"], c["stop"], c["limit"], c["tok"])
    _same(c, expected(case, tokens, greedy=True))


def test_positions_outside_the_history_write_no_column():
    from quantizations_amd.layer_ops import greedy_step_streams

    logits = torch.randn(3, 50)
    hist = torch.full((3, 4), SENTINEL, dtype=torch.int64)
    pos = torch.tensor([-2, 4, 3])
    live = torch.ones(3, dtype=torch.int32)
    tok = torch.zeros(3, dtype=torch.int64)
    greedy_step_streams(logits, hist, pos, live, torch.full((3,), -1), torch.full((3,), 100), tok)
    assert torch.equal(tok, logits.argmax(-1)) and pos.tolist() == [-1, 5, 4]
    assert (hist[:2] == SENTINEL).all() and hist[2].tolist() == [SENTINEL] * 3 + [int(tok[2])]


def test_streams_picks_reject_wrong_operands():
    from quantizations_amd.layer_ops import greedy_step_streams, sample_step_streams

    case, _ = build_case(100, 3, H, torch.float32, seed=1)
    names = ("logits", "hist", "pos", "live", "stop", "limit", "tok")
    for bad in (dict(pos=case["pos"][:2]), dict(live=case["live"].long()), dict(stop=case["stop"].int()),
                dict(limit=case["limit"][:1]), dict(hist=case["hist"][:2]), dict(logits=case["logits"][:, ::2])):
        with pytest.raises(ValueError):
            greedy_step_streams(*({**case, **bad}[k] for k in names))
    with pytest.raises(ValueError):
        sample_step_streams(*(case[k] for k in names), case["temperature"], case["top_k"].long(), case["top_p"],
                            case["uniform"])
    with pytest.raises(ValueError):
        sample_step_streams(*(case[k] for k in names), case["temperature"], case["top_k"], case["top_p"],
                            case["uniform"][:, :4])


def test_stream_session_refuses_what_it_cannot_run():
    from transformers import LlamaConfig, LlamaForCausalLM

    import quantizations_amd as qa
    from quantizations_amd import generation

    assert qa.StreamSession is generation.StreamSession and qa.generate_ragged is generation.generate_ragged
    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2,
                      num_key_value_heads=1, vocab_size=64, max_position_embeddings=32)
    model = LlamaForCausalLM(cfg).eval()
    with pytest.raises(ValueError, match="batch"):
        qa.StreamSession(model, 0, 16)
    with pytest.raises(ValueError, match="max_len"):
        qa.StreamSession(model, 2, 1)
    with pytest.raises(ValueError, match="cpu"):          # a CPU model: no eager fallback
        qa.StreamSession(model, 2, 16)
    with pytest.raises(ValueError, match="cpu"):
        qa.generate_ragged(model, [torch.tensor([1, 2, 3]), torch.tensor([4])], 4)
    for prompts in ([], [torch.tensor([[1, 2]])], [torch.tensor([], dtype=torch.int64)], [[1, 2, 3]]):
        with pytest.raises(ValueError, match="prompts"):
            qa.generate_ragged(model, prompts, 4)
    with pytest.raises(ValueError, match="max_new_tokens"):
        qa.generate_ragged(model, [torch.tensor([1])], 0)
