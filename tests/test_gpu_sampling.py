"""GPU: layer_ops.sample_step (csrc/sample.hip, qz_sample_step) against tests/sampling_reference.py,
the fp64 statement of its rules.

Every row of a case is called once per column of `uniform` with pos advancing, so hist holds one pick
per column.  The first columns are TARGETED: u is the fp64 midpoint of the CDF interval (>= 1e-4
wide) of a chosen token of the reference's kept set and the kernel must return that token.  The next
256 columns are seeded random draws: a draw is left out only if the fp64 CDF has a boundary within
1e-4 of u, at most 2 % of a case's draws may be left out, every other draw equals the reference.

What each part can hold, worked out with the helper on the CPU before the seeds were fixed:
* the share of u within 1e-4 of a boundary is about 2e-4 per boundary that carries weight, so the
  random draws use settings with a narrow head (top-k 7 / 50, or top-p on the heavy tokens: <= 0.6 %
  measured for the reference alone at every V); rows that keep all V tokens are 11-24 % at V =
  128256 and are checked by targeted u instead;
* a flat row (all logits equal: one tie group, always kept whole) has CDF steps of 1 / V, narrower
  than 1e-4 from V = 32000 on, so no u is 1e-4 away from a boundary there.  Its weights are all
  exp(0) = 1 and every fp32 sum of them is exact, so its pick is asserted EXACTLY at every V,
  floor(fp32(u * V)) with no draw left out, and with targeted u as well where V <= 2056.
top_p is always safe_top_p's: >= 5e-4 away from every tie-group boundary, far above fp32 error."""
import numpy as np
import pytest
import torch
from sampling_reference import gap_many, interval, pick_many, safe_top_p, sample_reference

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
NT, NR = 6, 256                      # targeted and random columns
SHAPES = [(V, B) for V in (1000, 2056, 32000, 128256) for B in (1, 3, 16)]
# rows of stride > V: "strided" keeps the 16-B vector loads where V % 8 == 0, "odd" takes the scalar
# loads; "last" is the logits[:, -1] view of a [B, 1, V] tensor
LAYOUT = {(1000, 1): "plain", (1000, 3): "odd", (1000, 16): "last",
          (2056, 1): "strided", (2056, 3): "last", (2056, 16): "odd",
          (32000, 1): "odd", (32000, 3): "plain", (32000, 16): "strided",
          (128256, 1): "last", (128256, 3): "strided", (128256, 16): "odd"}
FAMILIES = ("randn", "peaked", "minus_inf")
NARROW = [(0.8, 50, 0.9), (0.8, 7, 1.0), (1.0, 50, 1.0), (0.8, 0, 0.6)]            # the random draws
ALL = NARROW + [(0.8, 0, 1.0), (1.3, 0, 0.95), (0.8, 5000, 1.0), (0.5, -3, 2.0)]   # the targeted ones


def family_row(fam, V, dtype, g):
    z = torch.randn(V, generator=g) * 4
    if fam == "peaked":
        z[int(torch.randint(V, (1,), generator=g))] = z.max() + 20
    elif fam == "minus_inf":
        z[torch.rand(V, generator=g) < 0.3] = float("-inf")
    elif fam == "flat":
        z = torch.full((V,), 1.5)
    return z.to(dtype)


def build(V, B, dtype, rot, settings, seed):
    """logits [B, V] (CPU), per-row (temperature, top_k, top_p) and references"""
    g = torch.Generator().manual_seed(seed)
    logits = torch.stack([family_row(FAMILIES[(b + rot) % 3], V, dtype, g) for b in range(B)])
    T, K, P, refs = [], [], [], []
    for b in range(B):
        t, k, want = settings[(b + rot) % len(settings)]
        z = logits[b].double().numpy()
        p = safe_top_p(z, t, k, want) if want < 1 else want
        ref = sample_reference(z, t, k, p)
        assert not ref.greedy and (p >= 1 or ref.p_margin >= 4e-4)
        T.append(t), K.append(k), P.append(p), refs.append(ref)
    return logits, T, K, P, refs


def laid_out(logits, layout):
    B, V = logits.shape
    if layout == "plain":
        return logits.to(DEV)
    if layout == "last":
        t = torch.zeros((B, 1, V), dtype=logits.dtype, device=DEV)
        t[:, 0] = logits.to(DEV)
        return t[:, -1]
    pad, off = (24, 8) if layout == "strided" else (11, 3)
    wide = torch.full((B, V + pad), 30.0, dtype=logits.dtype, device=DEV)   # the padding would win if read
    wide[:, off:off + V] = logits.to(DEV)
    return wide[:, off:off + V]


def run_columns(logits, T, K, P, U, **kw):
    """One sample_step per column of U [B, H]; returns hist [B, H] (numpy)."""
    from quantizations_amd.layer_ops import sample_step

    B, H = U.shape
    hist = torch.full((B, H), -1, dtype=torch.int64, device=DEV)
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    tok = torch.zeros(B, dtype=torch.int64, device=DEV)
    args = (torch.tensor(T, dtype=torch.float32, device=DEV), torch.tensor(K, dtype=torch.int32, device=DEV),
            torch.tensor(P, dtype=torch.float32, device=DEV), torch.tensor(U, dtype=torch.float32, device=DEV))
    for _ in range(H):
        sample_step(logits, hist, pos, tok, *args, **kw)
    torch.cuda.synchronize()
    assert int(pos.item()) == H and torch.equal(tok, hist[:, -1])
    return hist.cpu().numpy()


def targets_of(ref, rng):
    """first, last and median of the kept tokens whose CDF interval is >= 1e-4 wide, plus three seeded"""
    idx = np.nonzero(ref.kept)[0]
    width = np.diff(np.concatenate([[0.0], ref.cdf[idx]]))
    wide = idx[width >= 1e-4]
    assert wide.size, "no token with a CDF interval of 1e-4"
    picks = [wide[0], wide[-1], wide[wide.size // 2]] + list(rng.choice(wide, 3))
    return [int(t) for t in picks]


def target_columns(refs, seed):
    rng = np.random.default_rng(seed)
    toks = np.array([targets_of(r, rng) for r in refs])
    U = np.array([[np.float32(sum(interval(r, t)) / 2) for t in row] for r, row in zip(refs, toks)], dtype=np.float32)
    return toks, U


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("V,B", SHAPES)
def test_targeted_u_returns_the_target(V, B, dtype):
    for rot in range(3 if B == 1 else 1):
        logits, T, K, P, refs = build(V, B, dtype, rot, ALL, seed=V + B + rot)
        toks, U = target_columns(refs, seed=V + B)
        got = run_columns(laid_out(logits, LAYOUT[V, B]), T, K, P, U)
        print(V, B, dtype, rot, "kept", [int(r.kept.sum()) for r in refs])
        assert np.array_equal(got, toks), (rot, np.argwhere(got != toks)[:8])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("V,B", SHAPES)
def test_random_u_equals_the_reference(V, B, dtype):
    left_out = total = 0
    for rot in range(3 if B == 1 else 1):
        logits, T, K, P, refs = build(V, B, dtype, rot, NARROW, seed=7 * V + B + rot)
        U = np.random.default_rng(V + 31 * B + rot).random((B, NR), dtype=np.float32)
        got = run_columns(laid_out(logits, LAYOUT[V, B]), T, K, P, U)
        for b, ref in enumerate(refs):
            assert ref.kept[got[b]].all(), "a token outside the reference's kept set (or a -inf entry)"
            assert np.isfinite(logits[b].float().numpy()[got[b]]).all()
            near = gap_many(ref, U[b]) < 1e-4
            total += NR
            left_out += int(near.sum())
            want = pick_many(ref, U[b])
            assert np.array_equal(got[b][~near], want[~near]), (rot, b, np.argwhere((got[b] != want) & ~near)[:8])
    print(V, B, dtype, f"left out {left_out} of {total}")
    assert left_out <= 0.02 * total


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("V", [1000, 2056, 32000, 128256])
def test_flat_rows(V, dtype):
    """All logits equal: one tie group, kept whole by every top_k and top_p; all weights are 1 and
    every fp32 sum is exact, so the pick is floor(fp32(u * V)) at every V.  Where the steps are >= 1e-4
    wide (V <= 2056) the targeted u of the reference hold as well."""
    B = 4
    logits = torch.stack([family_row("flat", V, dtype, None) for _ in range(B)])
    T, K, P = [0.8, 1.3, 0.8, 1.0], [50, 0, 1, V], [0.9, 0.3, 0.0, 1.0]
    refs = [sample_reference(logits[b].double().numpy(), T[b], K[b], P[b]) for b in range(B)]
    assert all(r.kept.all() for r in refs)
    U = np.random.default_rng(V).random((B, 64), dtype=np.float32)
    U[:, 0], U[:, 1] = 0.0, np.nextafter(np.float32(1), np.float32(0))
    want = np.floor(U * np.float32(V)).astype(np.int64)          # fp32 product, as the kernel forms u * R
    want = np.minimum(want, V - 1)                               # u * R == R: the last kept index
    got = run_columns(laid_out(logits, "plain"), T, K, P, U)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    if V <= 2056:
        toks, Ut = target_columns(refs, seed=V)
        assert np.array_equal(run_columns(laid_out(logits, "odd"), T, K, P, Ut), toks)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("V", [1000, 128256])
def test_greedy_rows_equal_greedy_step(V, dtype):
    """temperature 0 and 0.8 mixed: the rows with temperature <= 0 and the NaN, +inf and all -inf rows
    give greedy_step's tok, hist and pos; the sampled rows of the same batch are not disturbed."""
    from quantizations_amd.layer_ops import greedy_step, sample_step

    g = torch.Generator().manual_seed(V)
    rows, T = [], []
    z = family_row("randn", V, dtype, g)
    rows.append(z), T.append(0.0)                      # cold
    rows.append(z), T.append(0.8)                      # sampled, same logits
    t = z.clone(); t[V // 2] = t[V - 1] = float("nan")
    rows.append(t), T.append(0.8)                      # NaN: the first one
    t = z.clone(); t[V // 3] = t[V - 2] = float("inf")
    rows.append(t), T.append(0.8)                      # +inf: the first one
    rows.append(torch.full((V,), float("-inf"), dtype=dtype)), T.append(0.8)   # all -inf: index 0
    t = z.clone(); t[V // 2] = float("nan")
    rows.append(t), T.append(-1.0)                     # NaN and cold
    t = z.clone(); t[V // 3] = t[V - 1] = 50.0
    rows.append(t), T.append(0.0)                      # a tie: the first index
    rows.append(family_row("minus_inf", V, dtype, g)), T.append(0.0)
    logits = torch.stack(rows).to(DEV)
    B, H = len(rows), 8
    greedy = [b for b in range(B) if b != 1]
    hist = torch.randint(0, 9, (B, H), device=DEV)
    pos = torch.tensor([3], device=DEV)
    tok = torch.zeros(B, dtype=torch.int64, device=DEV)
    hist_r, pos_r, tok_r = hist.clone(), pos.clone(), tok.clone()
    greedy_step(logits, hist_r, pos_r, tok_r)
    ref = sample_reference(rows[1].double().numpy(), 0.8, 50, 1.0)
    t1 = int(np.nonzero(ref.kept)[0][-1])
    U = torch.full((B, H), np.float32(sum(interval(ref, t1)) / 2), device=DEV)
    sample_step(logits, hist, pos, tok, torch.tensor(T, device=DEV), torch.full((B,), 50, dtype=torch.int32, device=DEV),
                torch.ones(B, device=DEV), U)
    torch.cuda.synchronize()
    assert torch.equal(tok[greedy], tok_r[greedy]) and torch.equal(hist[greedy], hist_r[greedy])
    assert torch.equal(pos, pos_r)
    assert int(tok[1]) == t1 == int(hist[1, 3]) and torch.equal(hist[1, :3], hist_r[1, :3])


@pytest.mark.parametrize("B", [1, 3])
def test_feedback_and_the_column_of_u(B):
    """hist[b, pos], tok and pos + 1 are written; pos >= H (or < 0) writes no history but still
    advances; u comes from column min(max(pos, 0), H - 1)."""
    from quantizations_amd.layer_ops import sample_step

    V, H = 2056, 8
    g = torch.Generator().manual_seed(B)
    logits = torch.stack([family_row("randn", V, torch.float16, g) for _ in range(B)])
    refs = [sample_reference(logits[b].double().numpy(), 0.8, 7, 1.0) for b in range(B)]
    kept = [np.nonzero(r.kept)[0] for r in refs]
    # column j targets the (j mod 7)-th kept token of the row: the pick tells which column was read
    U = torch.tensor([[np.float32(sum(interval(r, int(k[j % 7]))) / 2) for j in range(H)] for r, k in zip(refs, kept)],
                     device=DEV)
    T = torch.full((B,), 0.8, device=DEV)
    K = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    P = torch.ones(B, device=DEV)
    lg = logits.to(DEV)
    for p0, col, writes in ((0, 0, True), (5, 5, True), (H - 1, H - 1, True), (H, H - 1, False), (H + 9, H - 1, False),
                            (-2, 0, False)):
        flat = torch.full((B * H + 4,), -7, dtype=torch.int64, device=DEV)
        hist = flat[:B * H].view(B, H)
        pos = torch.tensor([p0], device=DEV)
        tok = torch.full((B,), -1, dtype=torch.int64, device=DEV)
        sample_step(lg, hist, pos, tok, T, K, P, U)
        torch.cuda.synchronize()
        want = torch.tensor([int(k[col % 7]) for k in kept], device=DEV)
        assert torch.equal(tok, want), (p0, tok, want)
        assert int(pos.item()) == p0 + 1
        expect = torch.full_like(flat, -7)
        if writes:
            expect[:B * H].view(B, H)[:, p0] = want
        assert torch.equal(flat, expect), p0


@pytest.mark.parametrize("composed", [False, True], ids=["kernel", "composed"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_captured_step_follows_new_values(dtype, composed):
    """sample_step captured once; temperature, top_k, top_p, uniform and the logits changed in place:
    the replay equals an eager call with the new values (and the targeted tokens of the reference)."""
    from functools import partial

    from quantizations_amd import layer_ops

    sample_step = partial(layer_ops.sample_step, composed=composed)   # the torch route can be captured as well
    V, B, H = 32000, 3, 4
    logits, T, K, P, refs = build(V, B, dtype, 0, NARROW, seed=5)
    lg = logits.to(DEV)
    toks, U = target_columns(refs, seed=1)
    t_T, t_K, t_P = (torch.tensor(T, device=DEV), torch.tensor(K, dtype=torch.int32, device=DEV),
                     torch.tensor(P, dtype=torch.float32, device=DEV))
    t_U = torch.tensor(U[:, :H], device=DEV)
    hist = torch.zeros((B, H), dtype=torch.int64, device=DEV)
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    tok = torch.zeros(B, dtype=torch.int64, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sample_step(lg, hist, pos, tok, t_T, t_K, t_P, t_U)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sample_step(lg, hist, pos, tok, t_T, t_K, t_P, t_U)
    pos.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert tok.tolist() == toks[:, 0].tolist()
    # other settings, another u, other logits in the same buffer (stale bins would show)
    logits2, T2, K2, P2, refs2 = build(V, B, dtype, 1, ALL[3:], seed=6)
    lg.copy_(logits2)
    toks2, U2 = target_columns(refs2, seed=2)
    t_T.copy_(torch.tensor(T2)), t_K.copy_(torch.tensor(K2, dtype=torch.int32)), t_P.copy_(torch.tensor(P2))
    t_U.copy_(torch.tensor(U2[:, 2:2 + H]))
    hist_e, pos_e, tok_e = hist.clone(), pos.clone(), tok.clone()
    sample_step(lg, hist_e, pos_e, tok_e, t_T, t_K, t_P, t_U)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(tok, tok_e) and torch.equal(hist, hist_e) and torch.equal(pos, pos_e)
    assert tok.tolist() == toks2[:, 3].tolist() and int(pos.item()) == 2


@pytest.mark.parametrize("how", ["fp32_logits", "forced_fp16", "forced_bf16"])
@pytest.mark.parametrize("V,B", [(1000, 3), (32000, 16)])
def test_composed_route_gives_the_targeted_picks(V, B, how):
    """The torch route (what fp32 logits take, and composed=True) on the targeted cases, with greedy
    rows mixed in."""
    from quantizations_amd.layer_ops import sample_step, sample_step_supported

    dtype = torch.bfloat16 if how == "forced_bf16" else torch.float16
    logits, T, K, P, refs = build(V, B, dtype, 0, ALL, seed=V + B)
    toks, U = target_columns(refs, seed=V)
    logits[B - 1, V // 2] = float("nan")
    T[0] = 0.0
    toks[0, :] = int(logits[0].argmax())
    toks[B - 1, :] = V // 2
    lg = laid_out(logits, "strided")
    kw = {"composed": True}
    if how == "fp32_logits":
        lg, kw = lg.float(), {}
        B_, H_ = U.shape
        bufs = (torch.zeros((B_, H_), dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV),
                torch.zeros(B_, dtype=torch.int64, device=DEV), torch.ones(B_, device=DEV),
                torch.zeros(B_, dtype=torch.int32, device=DEV), torch.ones(B_, device=DEV),
                torch.zeros((B_, H_), device=DEV))
        assert not sample_step_supported(lg, *bufs) and sample_step_supported(lg.half(), *bufs)
        assert not sample_step_supported(lg.half(), bufs[0].t(), *bufs[1:])      # a transposed history
        assert not sample_step_supported(lg.half().cpu(), *bufs)
    got = run_columns(lg, T, K, P, U, **kw)
    assert np.array_equal(got, toks), np.argwhere(got != toks)[:8]
