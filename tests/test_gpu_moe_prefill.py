"""Routed 4-bit mixture-of-experts above 16 rows (csrc/moe_prefill.hip: route_rows, plan, the two
expert-grouped tile GEMMs; moe.SparseMoe4bit's route to them) against fp64 torch on the product's own
dequantised, expert-tagged weights of test_gpu_moe.py.  Bars are measured as there: twice the error of
the plain torch twin in the activation dtype against the same fp64 reference.

Measured on an MI355X: see profiles/moe_prefill_gpu_tests.txt."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_moe import DEV, DTYPES, E, FORMATS, PATTERNS, TOPK, down_ref, experts, pair_ref, routing, row_err

pytestmark = pytest.mark.gpu
SHAPES = [(256, 256), (512, 768)]
# what each row count is for: 17 = just past the decode limit, nearly empty tiles; 80 "same" = two
# experts with 80 entries each (a full and a ragged tile), six empty; 200 = every expert, several tiles
CASES = {17: PATTERNS, 80: ("same",), 200: ("random", "cover")}


@functools.lru_cache(maxsize=None)
def rows(H, I, dtype, T=300):
    g = torch.Generator().manual_seed(7 * H + I)
    return (torch.randn(T, H, generator=g).to(DEV, dtype), (torch.randn(T, TOPK, I, generator=g) * 0.5).to(DEV, dtype))


def launch(c, x, hin, idx, w, residual=None):
    """(h, y) of the grouped launches: pair on x, down on hin."""
    from quantizations_amd.core import moe_gemm_down, moe_gemm_pair_silu, moe_plan
    plan = moe_plan(idx, E)
    return (moe_gemm_pair_silu(x, c["gu"][0], c["gu"][1], idx, plan, E),
            moe_gemm_down(hin, c["dn"][0], c["dn"][1], idx, w, plan, E, residual=residual))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("T", [17, 200])
def test_plan_is_a_stable_sort_by_expert(T, pattern):
    from quantizations_amd.core import moe_plan
    idx, _ = routing(pattern, T)
    srt, offsets = moe_plan(idx, E)
    seg = idx.flatten().long()
    seg = torch.where((seg < 0) | (seg >= E), E, seg)
    assert torch.equal(srt.long(), torch.sort(seg, stable=True).indices)
    counts = torch.bincount(seg, minlength=E + 1)
    assert torch.equal(offsets.long(), F.pad(counts.cumsum(0), (1, 0)))
    assert counts[E] == (2 if pattern == "invalid" else 0)   # invalid entries: only in the last segment


@pytest.mark.parametrize("dtype", DTYPES)
def test_route_rows_gives_route_bits(dtype):
    from quantizations_amd.core import moe_route, moe_route_rows
    g = torch.Generator().manual_seed(11)
    x, W = torch.randn(40, 256, generator=g).to(DEV, dtype), (torch.randn(E, 256, generator=g) / 32).to(DEV, dtype)
    whole = moe_route_rows(x, W, TOPK, logits=True)
    for r0 in (0, 16, 32):
        for a, b in zip(whole, moe_route(x[r0:r0 + 16], W, TOPK, logits=True)):
            assert torch.equal(a[r0:r0 + 16], b)


def check_values(H, I, T, dtype, qt, dq, bs=64, patterns=None):
    c = experts(H, I, dtype, qt, dq, bs)
    x, hin = rows(H, I, dtype)[0][:T], rows(H, I, dtype)[1][:T].contiguous()
    for pattern in patterns or CASES[T]:
        idx, w = routing(pattern, T)
        h, y = launch(c, x, hin, idx, w)
        href, yref = pair_ref(x, c["gu"][2], idx, dtype), down_ref(hin, c["dn"][2], idx, w, dtype)
        htwin = pair_ref(x, c["gu"][2].to(dtype), idx, dtype)
        ytwin = down_ref(hin, c["dn"][2].to(dtype), idx, w, dtype)
        eh, bh, ey, by = row_err(h, href), 2 * row_err(htwin, href), row_err(y, yref), 2 * row_err(ytwin, yref)
        print(f"H{H} I{I} T{T} {dtype} {qt} dq={dq} bs={bs} {pattern}: pair {eh:.3e} (bar {bh:.3e}) "
              f"down {ey:.3e} (bar {by:.3e})")
        assert eh <= bh and ey <= by, (pattern, eh, bh, ey, by)
        if pattern == "invalid":   # zero h rows; y without those entries is the fp64 reference's y (held above)
            bad = (idx < 0) | (idx >= E)
            assert bad.sum() == 2 and torch.all(h[bad] == 0)


@pytest.mark.parametrize("qt, dq", FORMATS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", sorted(CASES))
@pytest.mark.parametrize("H, I", SHAPES)
def test_pair_and_down(H, I, T, dtype, qt, dq):
    check_values(H, I, T, dtype, qt, dq)


@pytest.mark.parametrize("H, I, bs", [(256, 256, 4096),   # experts share a second-level block
                                      (512, 768, 512)])    # down rows (K = 768) start inside a scale block
def test_scale_layouts(H, I, bs):
    check_values(H, I, 200, torch.float16, "nf4", True, bs=bs, patterns=("random",))


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_reads_an_expert_back(dtype):
    """top_k = 1, the 256 rows of eye(256) on one expert: every weight of it through both tile kernels, bit for bit."""
    from quantizations_amd.core import moe_gemm_down, moe_gemm_pair_silu, moe_plan
    from quantizations_amd.layer_ops import silu_mul
    c = experts(256, 256, dtype, "nf4", True)
    e = 5
    idx = torch.full((256, 1), e, dtype=torch.int32, device=DEV)
    one = torch.ones(256, 1, device=DEV)
    eye = torch.eye(256, device=DEV, dtype=dtype)
    Wgu, Wdn = c["gu"][2][e].to(dtype), c["dn"][2][e].to(dtype)
    plan = moe_plan(idx, E)
    h = moe_gemm_pair_silu(eye, c["gu"][0], c["gu"][1], idx, plan, E)
    assert torch.equal(h[:, 0].t(), silu_mul(Wgu[:256].contiguous(), Wgu[256:].contiguous()))
    y = moe_gemm_down(eye.view(256, 1, 256), c["dn"][0], c["dn"][1], idx, one, plan, E)
    assert torch.equal(y.t(), Wdn)


@pytest.mark.parametrize("H, I, dtype, qt, dq", [(256, 256, torch.float16, "nf4", True),
                                                  (512, 768, torch.bfloat16, "fp4", False)])
def test_row_invariance_and_residual(H, I, dtype, qt, dq):
    """Rows of a 200-row launch (64-column tiles) keep their bits among 17 rows with other neighbours and
    routings, and among 300 rows (128-column tiles)."""
    c = experts(H, I, dtype, qt, dq)
    x, hin = rows(H, I, dtype)
    idx, w = routing("random", 200)
    h, y = launch(c, x[:200], hin[:200].contiguous(), idx, w)
    picked = [0, 137, 199]
    for T, places, pattern in ((17, [5, 0, 16], "cover"), (300, [299, 64, 130], "random")):
        x2, hin2 = x[:T].flip(0).contiguous(), hin[:T].flip(0).contiguous()
        idx2, w2 = routing(pattern, T, seed=1)
        for r, p in zip(picked, places):
            x2[p], hin2[p], idx2[p], w2[p] = x[r], hin[r], idx[r], w[r]
        h2, y2 = launch(c, x2, hin2, idx2, w2)
        assert torch.equal(h2[places], h[picked]) and torch.equal(y2[places], y[picked]), T
    res = torch.randn(200, H, device=DEV).to(dtype)
    assert torch.equal(launch(c, x[:200], hin[:200].contiguous(), idx, w, residual=res)[1], res + y)


def test_graph_replay_follows_new_routing():
    from quantizations_amd.core import moe_gemm_down, moe_gemm_pair_silu, moe_plan, moe_route_rows
    c = experts(256, 256, torch.float16, "nf4", True)
    g = torch.Generator().manual_seed(5)
    W = (torch.randn(E, 256, generator=g) / 16).half().to(DEV)
    xs = [torch.randn(80, 256, generator=g).half().to(DEV) for _ in range(3)]

    def chain(x):
        idx, w = moe_route_rows(x, W, TOPK)
        plan = moe_plan(idx, E)
        h = moe_gemm_pair_silu(x, c["gu"][0], c["gu"][1], idx, plan, E)
        return idx, h, moe_gemm_down(h, c["dn"][0], c["dn"][1], idx, w, plan, E)

    eager = [chain(x) for x in xs]
    assert not torch.equal(eager[0][0], eager[1][0])   # the replays route elsewhere than the capture did
    x = xs[0].clone()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        chain(x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = chain(x)
    for k in (1, 2, 0, 1):
        x.copy_(xs[k])
        graph.replay()
        assert all(torch.equal(a, b) for a, b in zip(out, eager[k])), k


GROUPED = ("qz_moe_route_rows", "qz_moe_plan", "qz_moe_gemm_pair_silu_4bit", "qz_moe_gemm_down_4bit")
DECODE = ("qz_moe_route", "qz_moe_pair_silu_4bit", "qz_moe_down_4bit")


def test_module_routes(monkeypatch):
    from quantizations_amd import _lib, dequantize_4bit
    from quantizations_amd.core import moe_route_rows
    from quantizations_amd.moe import SparseMoe4bit
    H = I = 256
    g = torch.Generator().manual_seed(1)
    tag = (2.0 ** ((3 * torch.arange(E)) % 7 - 3))[:, None, None]
    moe = SparseMoe4bit((torch.randn(E, H, generator=g) / 16).half().to(DEV),
                        (torch.randn(E, 2 * I, H, generator=g) * 0.02 * tag).half().to(DEV),
                        (torch.randn(E, H, I, generator=g) * 0.02 * tag).half().to(DEV), TOPK)
    Wgu, Wdn = (dequantize_4bit(p, p.quant_state).t().reshape(E, -1, p.quant_state.shape[1]).double()
                for p in (moe.gate_up_proj, moe.down_proj))
    calls = {}
    for name in GROUPED + DECODE:
        def counted(*a, _real=getattr(_lib.lib, name), _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*a)
        monkeypatch.setattr(_lib.lib, name, counted)

    def census(x, route):
        calls.clear()
        moe.prefill_route = route
        return moe(x), dict(calls)

    for T in (40, 300):
        x = torch.randn(1, T, H, generator=g).half().to(DEV)
        y, seen = census(x, "auto")
        assert seen == dict.fromkeys(GROUPED, 1)
        assert census(x, "composed")[1] == {}
        idx, w = moe_route_rows(x[0], moe.gate.weight, TOPK)   # the product's own choice of experts
        ref = down_ref(pair_ref(x[0], Wgu, idx, x.dtype), Wdn, idx, w, x.dtype)
        twin = down_ref(pair_ref(x[0], Wgu.half(), idx, x.dtype), Wdn.half(), idx, w, x.dtype)
        err, bar = row_err(y[0], ref), 2 * row_err(twin, ref)
        print(f"module T={T}: {err:.3e} (bar {bar:.3e})")
        assert y.shape == x.shape and err <= bar
    assert census(torch.randn(5, H, generator=g).half().to(DEV), "auto")[1] == dict.fromkeys(DECODE, 1)
