"""GPU: layer_ops.greedy_step_streams / sample_step_streams (qz_*_step_streams): the picks with a
position, liveness, stop token and limit per stream.

A live row's token must be IDENTICAL to what greedy_step / sample_step pick for that row alone at
pos = p_b (the same kernels see the same row), and it is the reference's token too: every sampled
row draws a targeted u of tests/sampling_reference.py (the fp64 midpoint of a kept token's CDF
interval, >= 1e-4 wide) that sits at the row's own column of `uniform`; every other column holds a
number that would pick another token.  The feedback is held against tests/streams_reference.py."""
import numpy as np
import pytest
import torch
from streams_reference import SENTINEL, build_case, expected

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
H = 20
SHAPES = [(V, B) for V in (1000, 2056, 32000) for B in (1, 3, 16)]
LAYOUT = {(1000, 1): "plain", (1000, 3): "odd", (1000, 16): "last",
          (2056, 1): "strided", (2056, 3): "last", (2056, 16): "odd",
          (32000, 1): "odd", (32000, 3): "plain", (32000, 16): "strided"}
NAMES = ("hist", "pos", "live", "stop", "limit", "tok")
SAMPLING = ("temperature", "top_k", "top_p", "uniform")


def laid_out(logits, layout):
    nb, V = logits.shape
    if layout == "plain":
        return logits.to(DEV)
    if layout == "last":
        t = torch.zeros((nb, 1, V), dtype=logits.dtype, device=DEV)
        t[:, 0] = logits.to(DEV)
        return t[:, -1]
    pad, off = (24, 8) if layout == "strided" else (11, 3)
    wide = torch.full((nb, V + pad), 30.0, dtype=logits.dtype, device=DEV)   # the padding would win if read
    wide[:, off:off + V] = logits.to(DEV)
    return wide[:, off:off + V]


def on_gpu(case, layout):
    c = {k: v.to(DEV) for k, v in case.items() if k != "logits"}
    c["logits"] = laid_out(case["logits"], layout)
    return c


def same(c, want):
    hist, pos, live, tok = want
    got = c["hist"].cpu().numpy()
    assert np.array_equal(got, hist), np.argwhere(got != hist)[:8]
    assert np.array_equal(c["pos"].cpu().numpy(), pos) and np.array_equal(c["live"].cpu().numpy(), live)
    assert np.array_equal(c["tok"].cpu().numpy(), tok)


def check_feedback_shape(case, want, tokens):
    """the edges the case builder plants: stop and limit clear `live` AFTER the write; a dead row
    keeps every sentinel"""
    hist, pos, live, tok = want
    p = case["pos"].numpy()
    nb = len(p)
    assert live[0] == 1 and hist[0, p[0]] == tokens[0] and pos[0] == p[0] + 1
    if nb > 1:
        assert live[1] == 0 and hist[1, p[1]] == tokens[1] and tok[1] == tokens[1] and pos[1] == p[1] + 1
    if nb > 2:
        assert live[2] == 0 and hist[2, p[2]] == tokens[2] and pos[2] == p[2] + 1
    if nb > 3:
        assert (hist[3] == SENTINEL).all() and tok[3] == SENTINEL and pos[3] == p[3] and live[3] == 0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("V,B", SHAPES)
def test_sample_step_streams(V, B, dtype):
    from quantizations_amd.layer_ops import sample_step, sample_step_streams

    case, tokens = build_case(V, B, H, dtype, seed=V + B)
    c = on_gpu(case, LAYOUT[V, B])
    sample_step_streams(c["logits"], *(c[k] for k in NAMES), *(c[k] for k in SAMPLING))
    # each row alone through the shared-position entry point at pos = p_b
    solo = []
    for b in range(B):
        hist = torch.full((1, H), SENTINEL, dtype=torch.int64, device=DEV)
        pos = case["pos"][b:b + 1].to(DEV)
        tok = torch.zeros(1, dtype=torch.int64, device=DEV)
        sample_step(c["logits"][b:b + 1], hist, pos, tok, *(c[k][b:b + 1] for k in SAMPLING))
        solo.append(int(tok))
        assert int(pos) == int(case["pos"][b]) + 1 and int(hist[0, int(case["pos"][b])]) == solo[-1]
    torch.cuda.synchronize()
    assert solo == tokens.tolist(), "the targeted u returns the target through sample_step itself"
    want = expected(case, tokens)
    same(c, want)
    check_feedback_shape(case, want, tokens)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("V,B", SHAPES)
def test_greedy_step_streams(V, B, dtype):
    from quantizations_amd.layer_ops import greedy_step, greedy_step_streams

    case, _ = build_case(V, B, H, dtype, seed=5 * V + B)
    c0 = on_gpu(case, LAYOUT[V, B])
    solo = []
    for b in range(B):
        hist = torch.full((1, H), SENTINEL, dtype=torch.int64, device=DEV)
        pos = case["pos"][b:b + 1].to(DEV)
        tok = torch.zeros(1, dtype=torch.int64, device=DEV)
        greedy_step(c0["logits"][b:b + 1], hist, pos, tok)
        solo.append(int(tok))
    tokens = np.array(solo, dtype=np.int64)
    if B > 1:
        case["stop"][1] = solo[1]     # row 1 stops on ITS greedy token
    c = on_gpu(case, LAYOUT[V, B])
    greedy_step_streams(c["logits"], *(c[k] for k in NAMES))
    torch.cuda.synchronize()
    want = expected(case, tokens, greedy=True)
    assert want[3][case["live"].numpy() != 0].tolist() == tokens[case["live"].numpy() != 0].tolist()
    same(c, want)
    check_feedback_shape(case, want, tokens)


@pytest.mark.parametrize("composed", [False, True], ids=["hip", "composed"])
def test_fp32_logits_and_the_composed_route_follow_the_same_rules(composed):
    from quantizations_amd.layer_ops import greedy_step_streams, sample_step_streams

    V, B = 2056, 6
    case, tokens = build_case(V, B, H, torch.float16, seed=77)
    if not composed:
        case["logits"] = case["logits"].float()       # fp32: the sampler's composed route, the greedy kernel
    c = on_gpu(case, "plain")
    sample_step_streams(c["logits"], *(c[k] for k in NAMES), *(c[k] for k in SAMPLING), composed=composed)
    same(c, expected(case, tokens))
    c = on_gpu(case, "plain")
    greedy_step_streams(c["logits"], *(c[k] for k in NAMES), composed=composed)
    same(c, expected(case, tokens, greedy=True))


def test_a_captured_pick_follows_new_positions_liveness_and_parameters():
    from quantizations_amd.layer_ops import sample_step_streams

    V, B = 2056, 4
    case, tokens = build_case(V, B, H, torch.float16, seed=11)
    c = on_gpu(case, "plain")
    start = {k: c[k].clone() for k in NAMES}
    args = (c["logits"], *(c[k] for k in NAMES), *(c[k] for k in SAMPLING))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sample_step_streams(*args)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sample_step_streams(*args)
    # replay 1: the case as built
    for k in NAMES:
        c[k].copy_(start[k])
    g.replay()
    torch.cuda.synchronize()
    same(c, expected(case, tokens))
    # replay 2: the dead row revived and every row greedy, rows 0 and 1 at swapped positions, no stop
    case2 = {k: v.clone() for k, v in case.items()}
    case2["live"][:] = 1
    case2["stop"][:] = -1
    case2["pos"][0], case2["pos"][1] = case["pos"][1], case["pos"][0]
    case2["temperature"][:] = 0.0
    for k in NAMES + SAMPLING:
        c[k].copy_(case2[k])
    g.replay()
    torch.cuda.synchronize()
    same(c, expected(case2, tokens, greedy=True))
