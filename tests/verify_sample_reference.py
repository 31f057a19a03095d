"""The rule of qz_verify_sample_step_streams (include/quantizations.h) in numpy, composed from
sampling_reference (the pick of one row for one uniform number) and verify_reference (the accept
loop), and the targeted cases the CPU and GPU tests share: verify_reference.accept_case's streams
over rows from test_gpu_sampling's families, every row's u the fp64 midpoint of the CDF interval
(>= 1e-4 wide) of a kept token of that row's reference."""
import numpy as np
import torch
from sampling_reference import interval, pick, sample_reference
from verify_reference import accept_case, verify_feedback

MIN_WIDTH = 1e-4


def row_picks(logits, temperature, top_k, top_p, uniform, pos, T):
    """picks [B, T]: row b T + i drawn alone with stream b's settings and uniform[b, clamp(pos[b] + i)]."""
    B, H = uniform.shape
    picks = np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        for i in range(T):
            ref = sample_reference(np.asarray(logits[b * T + i], dtype=np.float64), float(temperature[b]),
                                   int(top_k[b]), float(top_p[b]))
            u = uniform[b, min(max(int(pos[b]) + i, 0), H - 1)] if H else 0.0
            picks[b, i] = pick(ref, u)
    return picks


def verify_sample_feedback(logits, temperature, top_k, top_p, uniform, hist, pos, live, stop, limit, tok):
    """numpy copies (hist, pos, live, tok, accepted) after one sampled verify step."""
    picks = row_picks(logits, temperature, top_k, top_p, uniform, pos, tok.shape[1])
    return verify_feedback(picks, hist, pos, live, stop, limit, tok)


def wide_tokens(ref):
    """The kept tokens of a sampled row whose CDF interval is at least MIN_WIDTH wide, ascending."""
    idx = np.nonzero(ref.kept)[0]
    width = np.diff(np.concatenate([[0.0], ref.cdf[idx]]))
    return idx[width >= MIN_WIDTH]


def midpoint(ref, token):
    return np.float32(sum(interval(ref, int(token))) / 2)


def safe_top_p_rows(rows, temperature, top_k, want, margin=4e-4):
    """A top_p near `want` that lies at least `margin` from every tie-group boundary of EVERY row (a
    stream's rows share one top_p): safe_top_p's margin for one row, far above fp32 error."""
    for j in range(200):
        p = float(np.float32(want + (-1) ** j * 0.0037 * ((j + 1) // 2)))
        if 0 < p < 1 and all(sample_reference(z, temperature, top_k, p).p_margin >= margin for z in rows):
            return p
    raise AssertionError("no top_p clear of every row's tie-group boundaries")


def window_case(T, V, dtype, seed, settings, family_row, families, H=40, greedy_stream=None, other=7.0):
    """accept_case(T, V, seed, H)'s B = T + 4 streams (exactly b matching drafts for stream b < T, a
    stop token inside an accepted run, a limit after two tokens, a dead stream among sentinels, a full
    window) with SAMPLED picks: logits [B T, V] from `families`, stream b's settings
    settings[b % len] (top_p moved clear of every row's tie-group boundaries), and picks[b, i] a kept token of row
    b T + i's reference with an interval >= MIN_WIDTH, distinct inside a stream where the row has a choice, whose midpoint sits at
    uniform[b, pos[b] + i]; every other column holds `other` (>= 1: it would pick the last kept
    index).  greedy_stream: that stream gets temperature 0, its picks are its rows' argmax.  Returns
    (case dict of CPU tensors incl. logits and the sampling operands, picks [B, T], accepted [B])."""
    from sampling_reference import greedy_pick

    case, _, want = accept_case(T, V, seed, H)
    B = T + 4
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed + 1)
    logits = torch.stack([family_row(families[(r + seed) % len(families)], V, dtype, g) for r in range(B * T)])
    pos = case["pos"].numpy()
    temp, K, P = [], [], []
    picks = np.zeros((B, T), dtype=np.int64)
    U = np.full((B, H), other, dtype=np.float32)
    for b in range(B):
        t, k, p_want = settings[b % len(settings)]
        if greedy_stream == b:
            t = 0.0
        rows = [logits[b * T + i].double().numpy() for i in range(T)]
        p = safe_top_p_rows(rows, t, k, p_want) if (t > 0 and p_want < 1) else p_want
        temp.append(t), K.append(k), P.append(p)
        used = set()
        for i in range(T):
            z = logits[b * T + i].double().numpy()
            if not t > 0:
                picks[b, i] = greedy_pick(z)
                continue
            ref = sample_reference(z, t, k, p)
            assert not ref.greedy and (p >= 1 or ref.p_margin >= 1e-4), (b, i, ref.p_margin)
            wide = [int(x) for x in wide_tokens(ref)]
            assert wide, "no token with a CDF interval of 1e-4"
            wide = [x for x in wide if x not in used] or wide      # a peaked row has one such token
            target = wide[int(rng.integers(len(wide)))]
            used.add(target)
            picks[b, i] = target
            U[b, pos[b] + i] = midpoint(ref, target)
    # accept_case's drafts, stop and limit over these picks
    tok = case["tok"].numpy().copy()
    tok[:, 1:] = picks[:, :-1]
    for b in range(T):
        if b + 1 < T:
            tok[b, b + 1] = (picks[b, b] + 1) % V
    stop = case["stop"].numpy().copy()
    stop[T] = picks[T, min(1, T - 1)]
    tok[T + 2] = case["tok"].numpy()[T + 2]          # the dead stream keeps its sentinels
    case = dict(case, logits=logits, tok=torch.from_numpy(tok), stop=torch.from_numpy(stop),
                temperature=torch.tensor(temp, dtype=torch.float32), top_k=torch.tensor(K, dtype=torch.int32),
                top_p=torch.tensor(P, dtype=torch.float32), uniform=torch.from_numpy(U))
    return case, picks, want


STATE = ("hist", "pos", "live", "stop", "limit", "tok")
SAMPLING = ("temperature", "top_k", "top_p", "uniform")


def expected(case):
    """verify_sample_feedback of a window_case (numpy)."""
    return verify_sample_feedback(case["logits"].double().numpy(), *(case[k].numpy() for k in SAMPLING),
                                  *(case[k].numpy() for k in STATE))
