"""The accept rule of qz_verify_step_streams and the drafter rule of qz_ngram_draft
(include/quantizations.h) restated in numpy, independently of the product, and the crafted cases the
CPU and GPU tests share."""
import numpy as np
import torch
from streams_reference import SENTINEL, feedback


def verify_feedback(picks, hist, pos, live, stop, limit, tok):
    """picks [B, T]: the greedy token of every row.  Successive streams feedbacks on each stream alone
    for as long as it stays live and the next draft is the token just emitted.  Returns numpy copies
    (hist, pos, live, tok, accepted)."""
    hist, pos, live, tok = hist.copy(), pos.copy(), live.copy(), tok.copy()
    B, T = tok.shape
    accepted = np.zeros(B, dtype=np.int32)
    for b in range(B):
        if live[b] == 0:
            continue
        for i in range(T):
            one = np.array([SENTINEL], dtype=np.int64)
            h, p, lv, one = feedback(picks[b, i:i + 1], hist[b:b + 1], pos[b:b + 1], live[b:b + 1], stop[b:b + 1],
                                     limit[b:b + 1], one)
            hist[b], pos[b], live[b], tok[b, 0] = h[0], p[0], lv[0], one[0]
            accepted[b] += 1
            if live[b] == 0 or i == T - 1 or tok[b, i + 1] != picks[b, i]:
                break
    return hist, pos, live, tok, accepted


def draft_rule(s, p, tok0, T, ngram_max):
    """The T - 1 drafts of a stream whose history is s[0..p] (s[p] == tok0)."""
    s = [int(x) for x in s]
    if 0 <= p < len(s):
        for n in range(min(ngram_max, p), 0, -1):
            hits = [m for m in range(0, p - n + 1) if s[m:m + n] == s[p - n + 1:p + 1]]
            if hits:
                e = s[:p + 1]
                for i in range(T - 1):
                    e.append(e[hits[-1] + n + i])
                return e[p + 1:]
    return [int(tok0)] * (T - 1)


def crafted_logits(picks, V, dtype, seed, ties=False, nan_rows=()):
    """logits [B*T, V] whose row r has its strict maximum at picks.flat[r] (ties: the same value again at
    a LATER index, so the first index must win; nan_rows: a NaN at the pick and a larger number
    elsewhere, NaN ranks above every number)."""
    g = torch.Generator().manual_seed(seed)
    flat = np.asarray(picks).reshape(-1)
    z = torch.randn(len(flat), V, generator=g) * 2
    for r, t in enumerate(flat):
        z[r, t] = 30.0
        if ties and t + 1 < V:
            z[r, V - 1 if t + 1 < V - 1 else t + 1] = 30.0
        if r in nan_rows:
            z[r, t] = float("nan")
            z[r, (t + 3) % V] = 60.0
    return z.to(dtype)


def accept_case(T, V, seed, H=40):
    """B = T + 4 streams over one crafted pick table.  Stream b < T has exactly b matching drafts (so
    it emits b + 1 tokens); stream T: every draft matches but pick 1 is its stop token (written, then
    the stream leaves, the later rows are ignored); stream T + 1: every draft matches, the limit is
    reached after two tokens; stream T + 2: dead among sentinels; stream T + 3: every draft matches
    and nothing stops it (T tokens).  Returns a dict of CPU tensors and picks [B, T]."""
    rng = np.random.default_rng(seed)
    B = T + 4
    picks = rng.integers(0, V, (B, T)).astype(np.int64)
    for b in range(B):          # no accidental repeats inside a row: a wrong draft is wrong
        picks[b] = rng.permutation(V)[:T]
    tok = np.full((B, T), SENTINEL, dtype=np.int64)
    tok[:, 0] = rng.integers(0, V, B)
    tok[:, 1:] = picks[:, :-1]
    for b in range(T):
        if b + 1 < T:
            tok[b, b + 1] = (picks[b, b] + 1) % V      # draft b + 1 is wrong: rows 0..b are emitted
    pos = rng.permutation(H - T - 2)[:B].astype(np.int64)
    live = np.ones(B, dtype=np.int32)
    stop = np.full(B, -1, dtype=np.int64)
    limit = np.full(B, H + 5, dtype=np.int64)
    stop[T] = picks[T, min(1, T - 1)]
    limit[T + 1] = pos[T + 1] + 2
    live[T + 2] = 0
    tok[T + 2] = SENTINEL
    case = dict(hist=torch.full((B, H), SENTINEL, dtype=torch.int64), pos=torch.from_numpy(pos),
                live=torch.from_numpy(live), stop=torch.from_numpy(stop), limit=torch.from_numpy(limit),
                tok=torch.from_numpy(tok), accepted=torch.full((B,), SENTINEL, dtype=torch.int32))
    want = np.array([b + 1 for b in range(T)] + [min(2, T), min(2, T), 0, T], dtype=np.int32)
    return case, picks, want


DRAFT_CASES = {
    # name: (history up to p, ngram_max, T, expected drafts)
    "no_match": ([1, 2, 3, 4, 5], 3, 4, [5, 5, 5]),
    "match_only_at_n1": ([7, 1, 9, 2, 8, 1], 3, 4, [9, 2, 8]),
    "two_matches_later_wins": ([1, 2, 3, 4, 1, 2, 5, 6, 1, 2], 2, 4, [5, 6, 1]),
    "longer_n_beats_later_match": ([9, 1, 2, 7, 5, 2, 8, 8, 1, 2], 2, 3, [7, 5]),
    "period_1_runs_into_the_drafts": ([3, 4, 4], 3, 5, [4, 4, 4, 4]),
    "period_2_runs_into_the_drafts": ([5, 6, 7, 6, 7], 3, 6, [6, 7, 6, 7, 6]),
    "p_below_ngram_max": ([4, 4], 4, 3, [4, 4]),
    "p_zero": ([6], 3, 3, [6, 6]),
    "n4": ([1, 2, 3, 4, 9, 9, 1, 2, 3, 4], 4, 3, [9, 9]),
}
