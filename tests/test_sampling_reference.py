"""CPU: tests/sampling_reference.py (the numpy statement of qz_sample_step's rules) against
transformers' logits warpers where the two are defined alike -- tie-free rows -- and the rules the
warpers leave open: tie groups stay or go whole, the corner values of top_k / top_p, and the rows
that fall back to torch.argmax's pick."""
import numpy as np
import pytest
import torch
from sampling_reference import greedy_pick, interval, pick, safe_top_p, sample_reference

V = 1000


def _row(seed):
    g = torch.Generator().manual_seed(seed)
    while True:
        z = torch.randn(V, generator=g) * 4
        if z.unique().numel() == V:
            return z


def _warped(z, temperature, top_k):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper

    s = TemperatureLogitsWarper(float(temperature))(None, z[None].clone())
    if top_k is not None:
        s = TopKLogitsWarper(top_k=top_k)(None, s)
    return s


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("temperature", [0.5, 0.8, 1.0, 1.7])
@pytest.mark.parametrize("top_k", [None, 1, 7, 50, 999, 1000, 5000])
def test_kept_set_equals_transformers_warpers(seed, temperature, top_k):
    from transformers.generation.logits_process import TopPLogitsWarper

    z = _row(seed)
    s = _warped(z, temperature, top_k)
    # top_p = 1 - the midpoint of two adjacent ascending cumulative sums, at tokens of probability
    # >= 1e-3: the warper's `cumsum <= 1 - top_p` then has a margin >= 5e-4
    probs, _ = s.softmax(-1)[0].double().sort()
    cum = probs.cumsum(0)
    heavy = torch.nonzero(probs >= 1e-3).flatten().tolist()
    heavy = [j for j in heavy if j > 0]
    assert heavy or top_k == 1
    tops = [1.0, 0.0]
    for j in {heavy[0], heavy[len(heavy) // 2], heavy[-1]} if heavy else ():
        tops.append(float(np.float32(1.0 - float(cum[j - 1] + cum[j]) / 2)))
    k = 0 if top_k is None else top_k
    for top_p in tops:
        want = s if top_p >= 1 else TopPLogitsWarper(top_p=max(top_p, 0.0))(None, s.clone())
        ref = sample_reference(z.numpy(), temperature, k, top_p)
        assert not ref.greedy
        assert np.array_equal(ref.kept, torch.isfinite(want[0]).numpy()), (top_p, int(ref.kept.sum()))
        if 0 < top_p < 1:
            assert ref.p_margin >= 4e-4


def test_tie_group_straddling_top_k_stays_whole():
    z = np.array([1.0, 2.0, 3.0, 2.0, 2.0, 0.5])
    assert sample_reference(z, 1.0, 2, 1.0).kept.tolist() == [False, True, True, True, True, False]
    assert sample_reference(z, 1.0, 1, 1.0).kept.tolist() == [False, False, True, False, False, False]
    assert sample_reference(z, 1.0, 5, 1.0).kept.tolist() == [True, True, True, True, True, False]


def test_tie_group_straddling_top_p_stays_or_goes_whole():
    z = np.array([0.0, 1.0, 2.0, 1.0, 1.0])
    # mass strictly above the score 1 is e^2 / (e^2 + 3 e + 1) = 0.4467; above 0 it is 0.9395
    assert sample_reference(z, 1.0, 0, 0.6).kept.tolist() == [False, True, True, True, True]
    assert sample_reference(z, 1.0, 0, 0.44).kept.tolist() == [False, False, True, False, False]
    assert sample_reference(z, 1.0, 0, 0.95).kept.tolist() == [True] * 5
    # the softmax is over the top-k survivors: with k = 4 the score 0 is gone before top-p looks
    assert sample_reference(z, 1.0, 4, 0.999).kept.tolist() == [False, True, True, True, True]


def test_corner_values():
    z = _row(5).numpy().astype(np.float64)
    z[17] = z[400] = z.max() + 1.0          # a maximal tie group of two
    z[3] = -np.inf
    finite = np.isfinite(z)
    for P in (0.0, -1.0):
        assert np.nonzero(sample_reference(z, 0.8, 0, P).kept)[0].tolist() == [17, 400]
    for k in (V, V + 1, 10 ** 6, 0, -1):
        assert np.array_equal(sample_reference(z, 0.8, k, 1.0).kept, finite)
    assert int(sample_reference(z, 0.8, V - 1, 1.0).kept.sum()) == V - 1   # fewer finite entries than k: all of them
    ref = sample_reference(z, 0.8, 0, 1.0)
    assert pick(ref, 0.0) == 0 and pick(ref, np.nextafter(1.0, 0.0)) == V - 1
    assert pick(ref, 1.0) == V - 1          # nothing above u * R: the last kept index
    lo, hi = interval(ref, 17)
    assert pick(ref, (lo + hi) / 2) == 17 and hi > lo


def test_rows_that_take_torch_argmax():
    z = _row(6)
    rows = {"cold": (z, 0.0), "negative_temperature": (z, -1.0)}
    t = z.clone(); t[500] = float("nan"); t[900] = float("nan")
    rows["nan"] = (t, 0.8)
    t = z.clone(); t[321] = float("inf"); t[700] = float("inf")
    rows["plus_inf"] = (t, 0.8)
    rows["all_minus_inf"] = (torch.full((V,), float("-inf")), 0.8)
    t = z.clone(); t[10] = t[600] = 99.0
    rows["tie_cold"] = (t, 0.0)
    for name, (row, temperature) in rows.items():
        ref = sample_reference(row.numpy(), temperature, 50, 0.9)
        assert ref.greedy, name
        assert ref.token == int(torch.argmax(row)) == greedy_pick(row.numpy()), name
        assert pick(ref, 0.37) == ref.token


def test_safe_top_p_keeps_its_margin():
    z = _row(7).numpy()
    for want in (0.5, 0.9, 0.99):
        P = safe_top_p(z, 0.8, 50, want)
        assert sample_reference(z, 0.8, 50, P).p_margin >= 4e-4
