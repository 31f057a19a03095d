"""GPU: the group-tiled attention (qz_attention_group, layer_ops.attention_group) against prefill_reference's
fp64 reference on the bar of the MFMA prefill tile (pr.TOL: the arithmetic inside a chunk is the same class).

One call per case holds every window start of L = 320 that can go wrong -- 0, around the 64-key tile and the
128-key chunk, L - T, L - 1 (its window runs past L for T > 1) -- with ragged lengths, a stream at pos < 0
and an idle one; every cache row at or above pos[b] holds NaN before the call, so one key too many shows."""
import pytest
import torch
import prefill_reference as pr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
L = 320
OPS = ("q", "k", "v", "cos", "sin", "kc", "vc")
# (G, Hkv, T, D, dtype): G = 12, T = 6 is 72 rows (the tile boundary falls inside a token's heads); G = 16, T = 1 fills
# one wave of a tile; G = 64, T = 16 is one token per tile
SHAPES = [(1, 2, 3, 64, "fp16"), (4, 2, 16, 128, "bf16"), (12, 1, 6, 64, "bf16"), (16, 1, 1, 128, "fp16"),
          (16, 2, 3, 64, "fp16"), (64, 1, 16, 128, "fp16"), (64, 1, 1, 64, "bf16")]
CHUNKS = [64, 128, 320]


def _case(G, Hkv, T, D, name, seed=0):
    ps = [0, 62, 63, 64, 65, 127, 128, 129, L - T, L - 1, -1, 5]
    short = max(T - 1, 1)
    lens = [T, short, T, 1, T, T, short, T, T, T, T, 0]
    return pr.make_case(len(ps), T, G * Hkv, Hkv, D, L, ps, lens, name, seed=seed + 31 * G + T + D)


def _run(case, key_chunk, fn=None, **over):
    """(out, kc, vc) of one call on fresh device copies of the case."""
    from quantizations_amd.layer_ops import attention_group
    d = {n: case[n].to(DEV) for n in OPS}
    d["pos"] = torch.tensor(case["pos"], dtype=torch.int64, device=DEV)
    d["len"] = torch.tensor(case["len"], dtype=torch.int64, device=DEV)
    d.update(over)
    tail = (case["Hq"], case["scale"]) + (() if fn else (key_chunk,))
    out = (fn or attention_group)(d["q"], d["k"], d["v"], d["cos"], d["sin"], d["kc"], d["vc"], d["pos"], d["len"], *tail)
    torch.cuda.synchronize()
    return out.cpu(), d["kc"].cpu(), d["vc"].cpu()


def _same(a, b):
    """Bit-identical, a NaN matching any NaN."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a.contiguous().view(torch.int16)[~na], b.contiguous().view(torch.int16)[~nb])


@pytest.fixture(scope="module")
def references():
    """shape -> (case, fp64 reference, caches after the call): computed once, shared by the key chunks, never changed."""
    memo = {}

    def get(shape):
        if shape not in memo:
            case = _case(*shape)
            memo[shape] = (case, pr.reference_fp64(case), pr.updated_caches(case))
        return memo[shape]
    return get


@pytest.mark.parametrize("key_chunk", CHUNKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "G%d-Hkv%d-T%d-D%d-%s" % s)
def test_values_against_fp64_and_the_caches_bit_for_bit(references, shape, key_chunk):
    case, ref, (kc_ref, vc_ref) = references(shape)
    out, kc, vc = _run(case, key_chunk)
    assert _same(kc, kc_ref) and _same(vc, vc_ref)
    for b, row in enumerate(pr.expected_fill(case)):      # NaN and zero rows exactly where the rules put them
        for i, what in enumerate(row):
            r = out[b, i]
            assert bool({"ok": not r.isnan().any(), "nan": r.isnan().all(), "zero": (r.view(torch.int16) == 0).all()}[what])
    tol = pr.TOL[shape[4]]
    print(shape, key_chunk, "max err", float((out.double() - ref).abs()[~ref.isnan()].max()))
    torch.testing.assert_close(out.double(), ref, atol=tol, rtol=tol, equal_nan=True)
    if shape[0] <= 8:                                      # the bits every other launch stores
        from quantizations_amd.layer_ops import prefill_attention
        _, kc_p, vc_p = _run(case, None, fn=prefill_attention)
        assert _same(kc, kc_p) and _same(vc, vc_p)


@pytest.mark.parametrize("key_chunk", CHUNKS)
@pytest.mark.parametrize("G,Hkv,T,D,name", [(12, 1, 6, 64, "fp16"), (16, 2, 16, 128, "bf16")])
def test_a_rows_bits_do_not_depend_on_T_len_or_the_other_streams(G, Hkv, T, D, name, key_chunk):
    case = _case(G, Hkv, T, D, name, seed=5)
    # whole windows (the halves below are whole too); the pos < 0 stream idles: its second half would start at a legal position
    case["len"] = [T if n and p >= 0 else 0 for n, p in zip(case["len"], case["pos"])]
    out, kc, vc = _run(case, key_chunk)
    # the window as two calls, the second on the caches the first leaves (another T, another len, other row tiles)
    first, second = pr.split_case(case, T // 2 + 1)
    o1, k1, v1 = _run(first, key_chunk)
    second["kc"], second["vc"] = k1, v1
    o2, k2, v2 = _run(second, key_chunk)
    # a row that starts past L in the second call is a bad position there (NaN either way)
    assert _same(torch.cat((o1, o2), 1), out) and _same(k2, kc) and _same(v2, vc)
    # stream 5 (pos 127) alone: no other streams beside it
    alone = dict(case, B=1, pos=case["pos"][5:6], len=case["len"][5:6], **{n: case[n][5:6] for n in OPS})
    assert _same(_run(alone, key_chunk)[0], out[5:6])


def test_refusals_leave_the_cache_untouched():
    from quantizations_amd.layer_ops import attention_group, attention_group_supported
    for G, D, key_chunk, spoil in [(65, 64, 128, None), (4, 96, 128, None), (4, 64, 100, None), (4, 64, 128, "stride"),
                                   (4, 64, 128, "pos")]:
        case = pr.make_case(2, 2, G, 1, D, 128, [3, 9], [2, 2], "fp16", seed=G + D, nan_above=False)
        d = {n: case[n].to(DEV) for n in OPS}
        pos = torch.tensor(case["pos"], dtype=torch.int32 if spoil == "pos" else torch.int64, device=DEV)
        length = torch.tensor(case["len"], dtype=torch.int64, device=DEV)
        if spoil == "stride":
            d["kc"], d["vc"] = (torch.cat((d[n], d[n]), -1)[..., :D] for n in ("kc", "vc"))
        before = d["kc"].clone(), d["vc"].clone()
        assert not attention_group_supported(d["q"], d["cos"], d["kc"], d["vc"], pos, length, G, key_chunk)
        with pytest.raises(ValueError):
            attention_group(d["q"], d["k"], d["v"], d["cos"], d["sin"], d["kc"], d["vc"], pos, length, G, case["scale"],
                            key_chunk)
        torch.cuda.synchronize()
        assert torch.equal(d["kc"], before[0]) and torch.equal(d["vc"], before[1])


def test_a_graph_replay_of_a_g16_step_equals_the_eager_bits():
    from quantizations_amd.layer_ops import attention_group
    case = pr.make_case(3, 1, 32, 2, 128, L, [0, 129, L - 1], [1, 1, 1], "fp16", seed=11)
    eager = _run(case, 128)
    d = {n: case[n].to(DEV) for n in OPS}
    pos = torch.tensor(case["pos"], dtype=torch.int64, device=DEV)
    length = torch.ones(3, dtype=torch.int64, device=DEV)
    kc0, vc0 = d["kc"].clone(), d["vc"].clone()
    call = lambda: attention_group(d["q"], d["k"], d["v"], d["cos"], d["sin"], d["kc"], d["vc"], pos, length, 32,  # noqa: E731
                                   case["scale"], 128)
    graph = torch.cuda.CUDAGraph()                         # the eager call above has loaded the kernels
    with torch.cuda.graph(graph):
        out = call()
    for _ in range(3):                                     # every replay from the first state, the workspace reused
        d["kc"].copy_(kc0), d["vc"].copy_(vc0), out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(out.cpu(), eager[0]) and _same(d["kc"].cpu(), eager[1]) and _same(d["vc"].cpu(), eager[2])
