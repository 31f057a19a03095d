"""CPU: the numpy-float32 restatement of qz_prefill_attention's order (prefill_reference.restatement_f32:
key tiles of TK from absolute 0, online softmax, P rounded to the storage dtype, one final rounding)
stays within HALF of each bar of test_gpu_prefill_attention.py against float64, on the very inputs of
its value and family checks -- the bars are not hiding the arithmetic's own error -- and is itself
bit-invariant under the window splits of the invariance check."""
import pytest
import torch
import activation_families as af
import prefill_reference as pr


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(_bits(a)[~na], _bits(b)[~nb])


@pytest.mark.parametrize("name", ["fp16", "bf16"])
@pytest.mark.parametrize("Hq,Hkv,D,L,T", pr.VALUE_CASES)
def test_restatement_within_half_the_bar_on_the_value_inputs(name, Hq, Hkv, D, L, T):
    case = pr.value_case(name, Hq, Hkv, D, L, T)
    ref = pr.reference_fp64(case)
    got, _, _ = pr.restatement_f32(case)
    got = got.double()
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    ok = ~torch.isnan(ref)
    tol = pr.TOL[name]
    d = (got - ref).abs()[ok]
    ratio = float((d / (tol + tol * ref.abs()[ok])).max())
    print(name, D, L, T, "worst share of the bar", ratio)
    assert ratio <= 0.5


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("family,name", pr.FAMILY_CASES)
def test_restatement_within_half_the_bar_on_the_families(family, name, D):
    c = pr.family_case(family, name, D)
    ref, bound = af.attention_fp64(c)
    assert bound <= af.SCORE_BOUND
    vm = af.vmax(c)
    got = pr.restatement_f32(pr.family_as_window(c))[0][:, 0].double()
    assert not bool(torch.isnan(got).any())
    tol = pr.TOL[name]
    d = ((got - ref) / vm).abs()
    ratio = float((d / (tol + tol * (ref / vm).abs())).max())
    print(family, name, D, "worst share of the bar", ratio)
    assert ratio <= 0.5


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_restatement_is_invariant_under_the_splits(name):
    L, T = 3 * pr.TK + 5, 2 * pr.TQ + 3
    case = pr.make_case(4, T, 4, 2, 64, L, pr.window_starts(L, T)[:4], pr.window_lengths(T), name, seed=T)
    out, kc, vc = pr.restatement_f32(case)
    for split in pr.splits_of(T):
        first, second = pr.split_case(case, split)
        o1, kc1, vc1 = pr.restatement_f32(first)
        second["kc"], second["vc"] = kc1, vc1
        o2, kc2, vc2 = pr.restatement_f32(second)
        assert _same(torch.cat((o1, o2), 1), out), split
        assert _same(kc2, kc) and _same(vc2, vc), split
