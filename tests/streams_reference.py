"""The per-stream feedback of qz_greedy_step_streams / qz_sample_step_streams (include/quantizations.h)
restated in numpy, independently of the product, and the case builder the CPU and GPU tests share:
rows from test_gpu_sampling's families with a targeted u at each row's own column."""
import numpy as np
import torch
from sampling_reference import greedy_pick, interval, safe_top_p, sample_reference

SENTINEL = -7


def feedback(tokens, hist, pos, live, stop, limit, tok):
    """Apply one pick's feedback to numpy copies; returns (hist, pos, live, tok)."""
    hist, pos, live, tok = hist.copy(), pos.copy(), live.copy(), tok.copy()
    for b, t in enumerate(tokens):
        if live[b] == 0:
            continue
        p = int(pos[b])
        if 0 <= p < hist.shape[1]:
            hist[b, p] = t
        tok[b] = t
        pos[b] = p + 1
        if t == stop[b] or p + 1 >= limit[b]:
            live[b] = 0
    return hist, pos, live, tok


def family_row(fam, V, dtype, g):
    z = torch.randn(V, generator=g) * 4
    if fam == "peaked":
        z[int(torch.randint(V, (1,), generator=g))] = z.max() + 20
    elif fam == "minus_inf":
        z[torch.rand(V, generator=g) < 0.3] = float("-inf")
    return z.to(dtype)


SETTINGS = [(0.8, 50, 0.9), (0.8, 7, 1.0), (0.0, 0, 1.0), (0.8, 0, 0.6), (1.3, 0, 0.95), (0.8, 0, 1.0)]


def build_case(V, B, H, dtype, seed):
    """A batch with mixed positions and liveness.  Returns a dict of CPU tensors (logits, hist, pos,
    live, stop, limit, tok, temperature, top_k, top_p, uniform) and `tokens`, the reference pick of
    every row (dead rows included: what a live row would have picked).  Row b's uniform number sits
    at its own column pos[b] -- the fp64 midpoint of the CDF interval (>= 1e-4 wide) of a kept token
    -- and every other column holds a number that picks another token or is far outside [0, 1).
    stop / limit: row 1 (if any) stops on its token, row 2 reaches its limit, row 3 is dead."""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    fams = ("randn", "peaked", "minus_inf")
    logits = torch.stack([family_row(fams[b % 3], V, dtype, g) for b in range(B)])
    pos = rng.permutation(H - 1)[:B] if B <= H - 1 else rng.integers(0, H - 1, B)
    pos = np.asarray(pos, dtype=np.int64)
    T, K, P, tokens = [], [], [], []
    U = np.full((B, H), 7.0, dtype=np.float32)     # u >= 1 would pick the last kept index
    for b in range(B):
        t, k, want = SETTINGS[b % len(SETTINGS)]
        z = logits[b].double().numpy()
        if t > 0:
            p = safe_top_p(z, t, k, want) if want < 1 else want
            ref = sample_reference(z, t, k, p)
            idx = np.nonzero(ref.kept)[0]
            width = np.diff(np.concatenate([[0.0], ref.cdf[idx]]))
            wide = idx[width >= 1e-4]
            target = int(wide[wide.size // 2]) if b % 2 else int(wide[0])
            U[b, pos[b]] = np.float32(sum(interval(ref, target)) / 2)
        else:
            p, target = want, greedy_pick(z)
        T.append(t), K.append(k), P.append(p), tokens.append(target)
    tokens = np.array(tokens, dtype=np.int64)
    live = np.ones(B, dtype=np.int32)
    stop = np.full(B, -1, dtype=np.int64)
    limit = np.full(B, H + 5, dtype=np.int64)
    if B > 1:
        stop[1] = tokens[1]
    if B > 2:
        limit[2] = pos[2] + 1
    if B > 3:
        live[3] = 0
    case = dict(logits=logits, hist=torch.full((B, H), SENTINEL, dtype=torch.int64), pos=torch.from_numpy(pos.copy()),
                live=torch.from_numpy(live), stop=torch.from_numpy(stop), limit=torch.from_numpy(limit),
                tok=torch.full((B,), SENTINEL, dtype=torch.int64), temperature=torch.tensor(T, dtype=torch.float32),
                top_k=torch.tensor(K, dtype=torch.int32), top_p=torch.tensor(P, dtype=torch.float32),
                uniform=torch.from_numpy(U))
    return case, tokens


def expected(case, tokens, greedy=False):
    """(hist, pos, live, tok) after one streams pick of `case` (numpy); greedy: argmax tokens."""
    if greedy:
        tokens = np.array([greedy_pick(r.double().numpy()) for r in case["logits"]], dtype=np.int64)
    return feedback(tokens, *(case[k].numpy() for k in ("hist", "pos", "live", "stop", "limit", "tok")))
