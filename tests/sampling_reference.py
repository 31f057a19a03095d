"""The sampling rules of qz_sample_step (include/quantizations.h) restated in numpy, independently
of the product: scores are the fp32 quotient logit / temperature (so ties are the kernel's ties),
everything after that is fp64.  One row at a time.

    ref = sample_reference(z, temperature, top_k, top_p)
    ref.greedy          the row takes torch.argmax's pick (ref.token)
    ref.kept            bool [V], the final kept set
    ref.cdf             fp64 [V], inclusive prefix of the kept weights in index order, divided by R
    ref.p_margin        distance of top_p from the nearest tie-group boundary G(v) (inf: filter off)
    pick(ref, u)        the token for a uniform number u          (pick_many: an array of u)
    boundary_gap(ref, u)  distance of u from the nearest CDF boundary   (gap_many)
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np


def greedy_pick(z) -> int:
    """torch.argmax's order: the first NaN, else the first index of the largest value."""
    z = np.asarray(z, dtype=np.float64)
    nan = np.isnan(z)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(z))


@dataclass
class Ref:
    greedy: bool
    token: Optional[int] = None
    kept: Optional[np.ndarray] = None
    cdf: Optional[np.ndarray] = None
    p_margin: float = float("inf")
    groups: Optional[tuple] = None    # (scores descending, G of each, mass of each), after top-k


def scores(z, temperature) -> np.ndarray:
    return (np.asarray(z, dtype=np.float32) / np.float32(temperature)).astype(np.float64)


def tie_groups(z, temperature, top_k):
    """After top-k: the distinct scores in descending order, the softmax mass strictly above each
    (G) and each group's own mass."""
    z = np.asarray(z, dtype=np.float64)
    V = z.size
    s = scores(z, temperature)
    kept = z > -np.inf
    if 1 <= top_k < V:
        kth = np.sort(s)[::-1][top_k - 1]
        kept &= s >= kth
    smax = s[kept].max()
    w = np.where(kept, np.exp(np.where(kept, s, smax) - smax), 0.0)
    vals, inv = np.unique(s[kept], return_inverse=True)
    mass = np.bincount(inv, weights=w[kept], minlength=vals.size)[::-1] / w.sum()
    vals = vals[::-1]
    G = np.concatenate([[0.0], np.cumsum(mass)[:-1]])
    return s, kept, vals, G, mass


def sample_reference(z, temperature, top_k, top_p) -> Ref:
    z = np.asarray(z, dtype=np.float64)
    zmax = np.nan if np.isnan(z).any() else z.max()
    if not (temperature > 0) or not np.isfinite(zmax):
        return Ref(greedy=True, token=greedy_pick(z))
    s, kept, vals, G, mass = tie_groups(z, temperature, int(top_k))
    P = float(np.float32(top_p))
    margin = float("inf")
    if P < 1:
        stay = G < P
        stay[0] = True                       # the maximal tie group always stays
        kept &= s >= vals[stay].min()
        if vals.size > 1:
            margin = float(np.abs(G[1:] - P).min())
    smax = s[kept].max()
    w = np.where(kept, np.exp(np.where(kept, s, smax) - smax), 0.0)
    cdf = np.cumsum(w)
    return Ref(greedy=False, kept=kept, cdf=cdf / cdf[-1], p_margin=margin, groups=(vals, G, mass))


def pick(ref: Ref, u) -> int:
    if ref.greedy:
        return ref.token
    hit = np.nonzero(ref.cdf > float(u))[0]
    return int(hit[0]) if hit.size else int(np.nonzero(ref.kept)[0][-1])


def boundary_gap(ref: Ref, u) -> float:
    """Distance of u from the nearest boundary of the CDF's steps (inf for a greedy row)."""
    if ref.greedy:
        return float("inf")
    b = ref.cdf[ref.kept]
    return float(np.abs(b - float(u)).min())


def pick_many(ref: Ref, u) -> np.ndarray:
    """pick() for an array of u (sampled rows)."""
    j = np.searchsorted(ref.cdf, np.asarray(u, dtype=np.float64), side="right")   # first index with cdf > u
    return np.where(j < ref.cdf.size, j, np.nonzero(ref.kept)[0][-1])


def gap_many(ref: Ref, u) -> np.ndarray:
    """boundary_gap() for an array of u (sampled rows)."""
    u = np.asarray(u, dtype=np.float64)
    b = ref.cdf[ref.kept]                     # ascending
    j = np.searchsorted(b, u)
    below = np.where(j > 0, u - b[np.maximum(j - 1, 0)], np.inf)
    above = np.where(j < b.size, b[np.minimum(j, b.size - 1)] - u, np.inf)
    return np.minimum(below, above)


def interval(ref: Ref, token: int):
    """[lo, hi): the u for which pick() returns `token`."""
    idx = np.nonzero(ref.kept)[0]
    j = int(np.searchsorted(idx, token))
    assert idx[j] == token
    return (float(ref.cdf[idx[j - 1]]) if j else 0.0), float(ref.cdf[token])


def safe_top_p(z, temperature, top_k, want: float, min_mass: float = 1e-3) -> float:
    """A top_p near `want` that no fp32 rounding can move across a tie-group boundary: `want` itself
    if every boundary G is at least min_mass / 2 away, else the middle of the nearest tie group of
    mass >= min_mass (its two boundaries are then >= min_mass / 2 away)."""
    _, _, vals, G, mass = tie_groups(z, temperature, int(top_k))
    if vals.size < 2 or np.abs(G[1:] - want).min() >= min_mass / 2:
        return float(np.float32(want))
    ends = G + mass                          # group j spans [G[j], ends[j]) of the descending mass
    ok = np.nonzero(mass >= min_mass)[0]
    assert ok.size, "no tie group heavy enough for a safe top_p"
    mids = (G[ok] + ends[ok]) / 2
    return float(np.float32(mids[np.abs(mids - want).argmin()]))
