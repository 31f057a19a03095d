"""GPU: LoRA adapter banks on Linear4bit -- a different adapter (or none) per decode stream -- on the
fused route (lora.shrink_mt + the multi-token launch carrying the expand, qz_lora_shrink_mt /
qz_gemm_4bit_grouped_lora) and on the composed torch route, against the fp64 reference per row
    y_c = dequantize_4bit(W, out_dtype=x.dtype) x_c (+ bias) + s_a B_a (A_a x_c),   a = slots[c // S]
at the project's bar (test_gpu_parity.assert_close).

Inputs as in test_gpu_lora.py: W = 0.02 randn (fp16, NF4 + double quant unless stated), x = randn,
A = 0.02 randn, B = randn / sqrt(r), scaling 1, 1.5 and 2 for entries 0, 1, 2.  Every adapted row
first asserts on the reference that its adapter term is at least a quarter of its base term, so the
bar cannot hide a dropped term, a wrong slot or a wrong rank index.  The seed of every case was
picked on the CPU (scripts/dev/lora_bank_seeds.py) as the first for which that ratio on the
UNQUANTISED W is at least 0.35 for every adapted row -- rank 1 included, where a row's term is a
single |N(0, 1)| draw -- so the 4-bit quantisation error (a few percent of the base norm) cannot
take it below 1/4.

t (shrink_mt alone): k_lora_shrink_mt runs k_lora_shrink's body per (rank row, token): each of 256
threads adds its 8 * ceil(K / 2048) exact 16-bit products in sequence (fp32 FMAs), then 6 butterfly
steps, 2 adds of the four wave partials and the scaling multiply: an fp32 summation tree of depth
d = 8 * ceil(K / 2048) + 9, bounded (first order) by d * 2^-24 * scaling * sum_k |a_jk x_ck| per
element of t.  (One dropped product is about 1 / K of that sum: 40x the bar at K = 14336.)
"""
import math

import pytest
import torch
from test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
SCALINGS = (1.0, 1.5, 2.0)


# ---------------------------------------------------------------------------
# inputs (generated on the CPU from seeds; shared with scripts/dev/lora_bank_seeds.py)
# ---------------------------------------------------------------------------


def _w16(M, K):
    """The unquantised fp16 weight of a shape (one per shape, whatever the case's seed)."""
    return (torch.randn(M, K, generator=torch.Generator().manual_seed(M * 31 + K)) * 0.02).half()


def _draw(M, K, T, ranks, dtype, seed, S=1):
    """x [T // S, S, K] and the bank entries [(A, B, scaling)] of a case, on the CPU."""
    g = torch.Generator().manual_seed(100003 * seed + M + 7 * K + 13 * T + sum(ranks))
    x = torch.randn(T // S, S, K, generator=g).to(dtype)
    ents = []
    for i, r in enumerate(ranks):
        A = (torch.randn(r, K, generator=g) * 0.02).to(dtype)
        B = (torch.randn(M, r, generator=g) / math.sqrt(r)).to(dtype)
        ents.append((A, B, SCALINGS[i % 3]))
    return x, ents


def _row_terms(Wd, x, ents, slots, S, bias=None):
    """fp64 (base [T, M], adapter term [T, M], adapted [T] bool) for rows x (any device)."""
    rows = x.reshape(-1, x.shape[-1]).double()
    base = rows @ Wd.t()
    if bias is not None:
        base = base + bias.double()
    ad = torch.zeros_like(base)
    adapted = []
    for c in range(rows.shape[0]):
        a = 0 if slots is None else int(slots[c // S])
        adapted.append(0 <= a < len(ents))
        if adapted[-1]:
            A, B, s = ents[a]
            ad[c] = s * (B.double() @ (A.double() @ rows[c]))
    return base, ad, adapted


def min_ratio_unquantised(M, K, T, ranks, dtype, seed, slots, S=1):
    """The smallest |adapter term| / |base term| over the adapted rows, on the unquantised weight."""
    x, ents = _draw(M, K, T, ranks, dtype, seed, S)
    base, ad, adapted = _row_terms(_w16(M, K).double(), x, ents, slots, S)
    return min((ad[c].norm() / base[c].norm()).item() for c in range(T) if adapted[c])


# (M, K, T, ranks of the bank's entries, dtype, quant_type, double quant, bias, slots per stream, seed)
F16, BF16 = torch.float16, torch.bfloat16
CASES = [
    (20, 256, 2, (1,), F16, "nf4", True, False, [0, -1], 0),
    (20, 1024, 3, (3, 3, 3), BF16, "nf4", True, True, [2, 0, 1], 0),
    (64, 256, 4, (16, 16, 16), F16, "nf4", True, False, [1, -1, 3, 0], 0),
    (64, 1024, 5, (64, 64, 64), BF16, "nf4", True, False, [0, 99, 2, -7, 1], 0),
    (64, 4096, 8, (3, 3, 3), F16, "nf4", True, True, [0, 1, 2, -1, 2, 1, 0, 3], 0),
    (4096, 4096, 9, (16, 16, 16), F16, "nf4", True, False, [0, 1, 2, -1, 0, 1, 2, 99, 1], 0),
    (4096, 4096, 16, (16, 16, 16), BF16, "nf4", True, False, [0, 1, 2, -1] * 4, 0),
    (4096, 1024, 16, (64,), F16, "nf4", True, False, [0, -1] * 8, 0),
    (20, 4096, 5, (1, 1, 1), BF16, "nf4", True, True, [0, 1, 2, -7, 1], 1),
    (4096, 256, 2, (64, 64, 64), F16, "nf4", True, False, [2, 1], 0),
    (64, 1024, 8, (16, 3, 8), F16, "nf4", True, False, [0, 1, 2, 0, 1, 2, -1, 1], 0),      # ranks padded to 16
    (4096, 4096, 4, (16, 16, 16), F16, "fp4", True, False, [0, 1, -1, 2], 0),
    (4096, 4096, 4, (16, 16, 16), BF16, "nf4", False, False, [0, 1, -1, 2], 0),            # plain absmax
    (4096, 4096, 3, (16, 16, 16), F16, "nf4", True, True, [1, 1, -1], 0),
]
# (M, K, streams, S, ranks, dtype, slots, seed): [B, S, K] prefill rows; a bank of one without slots
STREAM_CASE = (64, 1024, 4, 3, (16, 3, 8), F16, [2, -1, 0, 1], 0)
NOSLOT_CASE = (64, 1024, 5, (16,), BF16, 0)
# composed route: (name, M, K, T, ranks, x dtype, slots, seed)
COMPOSED_CASES = [
    ("one token", 64, 1024, 1, (16, 3, 8), F16, [1], 0),
    ("17 rows", 64, 1024, 17, (16, 3, 8), F16, [0, 1, 2, -1, 99] * 3 + [2, 1], 0),
    ("fp32 x", 64, 1024, 4, (16, 3, 8), torch.float32, [2, -1, 0, 1], 0),
]
# grouped launch: segments (64, 16, 16) at K = 1024, T = 4; banks (ranks 8 and 64) on the first and last
GROUP_CASE = ((64, 16, 16), 1024, 4, ((8, 8, 8), None, (64, 64, 64)), [0, 2, -1, 1], 0)


def _group_draw(seed=None):
    """The grouped case's shared x [T, 1, K] and per-segment entries (None: no bank), on the CPU."""
    rows, K, T, ranks, _, seed0 = GROUP_CASE
    g = torch.Generator().manual_seed(7919 * (seed0 if seed is None else seed) + 5)
    x = torch.randn(T, 1, K, generator=g).half()
    ents = []
    for M, rk in zip(rows, ranks):
        ents.append(None if rk is None else [((torch.randn(r, K, generator=g) * 0.02).half(),
                                              (torch.randn(M, r, generator=g) / math.sqrt(r)).half(), SCALINGS[i])
                                             for i, r in enumerate(rk)])
    return x, ents


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------

_LINS = {}


def _lin(M, K, dtype, qt="nf4", dq=True, bias=False):
    """(Linear4bit on the GPU without a bank, the dequantised operand of `dtype` rows as fp64, the fp32
    one as fp64) per shape and format, quantised once and shared."""
    import quantizations_amd as qa
    from quantizations_amd.core import dequantize_4bit

    key = (M, K, dtype, qt, dq, bias)
    if key not in _LINS:
        cd = torch.float32 if dtype == torch.float16 else None
        m = qa.Linear4bit(K, M, bias=bias, quant_type=qt, compress_statistics=dq, compute_dtype=cd)
        m.weight = qa.Params4bit(_w16(M, K), requires_grad=False, quant_type=qt, compress_statistics=dq, module=m)
        if bias:
            g = torch.Generator().manual_seed(M + K)
            bdt = dtype if dtype != torch.float32 else torch.float16
            m.bias = torch.nn.Parameter((torch.randn(M, generator=g) * 0.1).to(bdt), requires_grad=False)
        m = m.to(DEV)
        qs = m.weight.quant_state
        od = dtype if dtype != torch.float32 else torch.float16   # fp32 rows: the dequantise route's fp16 W
        Wd = dequantize_4bit(m.weight, qs, out_dtype=od).t().double().contiguous()
        W32 = dequantize_4bit(m.weight, qs, out_dtype=torch.float32).t().double().contiguous()
        _LINS[key] = (m, Wd, W32)
    m, Wd, W32 = _LINS[key]
    m.clear_adapter_bank()
    return m, Wd, W32


def _slots(vals, n=16):
    s = torch.full((n,), -1, dtype=torch.int32)
    s[:len(vals)] = torch.tensor(vals, dtype=torch.int32)
    return s.to(DEV)


def _dev(ents):
    return [(A.to(DEV), B.to(DEV), s) for A, B, s in ents]


def _check_rows(y, y_plain, Wd, x, ents, slot_vals, S, bias, dtype, what):
    """Adapted rows against the fp64 reference (after the 1/4 precondition); the others are the
    bits of the call without a bank."""
    base, ad, adapted = _row_terms(Wd, x, ents, slot_vals, S, bias)
    y2, p2 = y.reshape(-1, y.shape[-1]), y_plain.reshape(-1, y.shape[-1])
    for c in range(y2.shape[0]):
        if not adapted[c]:
            assert torch.equal(y2[c], p2[c]), f"{what}: row {c} has no adapter: the plain call's bits"
            continue
        ratio = (ad[c].norm() / base[c].norm()).item()
        assert ratio >= 0.25, f"{what}: row {c}: adapter / base = {ratio:.3f}"
        assert not torch.equal(y2[c], p2[c])
        assert_close(y2[c].double().cpu().numpy(), (base[c] + ad[c]).cpu().numpy(), dtype, f"{what} row {c}")


def _count_fused(monkeypatch):
    from quantizations_amd import lora

    calls = []
    real = lora.shrink_mt

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(lora, "shrink_mt", counted)
    return calls


# ---------------------------------------------------------------------------
# the fused route through Linear4bit
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}-T{c[2]}-r{'.'.join(map(str, c[3]))}-"
                         f"{'f16' if c[4] == F16 else 'bf16'}-{c[5]}{'' if c[6] else '-absmax'}{'-bias' if c[7] else ''}")
def test_bank_rows_on_the_fused_route(case, monkeypatch):
    M, K, T, ranks, dtype, qt, dq, bias, slot_vals, seed = case
    lin, Wd, _ = _lin(M, K, dtype, qt, dq, bias)
    x, ents = _draw(M, K, T, ranks, dtype, seed)
    x, ents = x.to(DEV), _dev(ents)
    y_plain = lin(x)
    slots = _slots(slot_vals)
    lin.set_adapter_bank(ents, slots)
    assert lin.adapter_bank.A.device == x.device and lin.adapter_bank.r == max(ranks)
    calls = _count_fused(monkeypatch)
    y = lin(x)
    assert calls == [1], "2..16 rows of 16-bit x take shrink_mt + the multi-token launch"
    assert y.shape == (T, 1, M) and y.dtype == dtype
    b = None if lin.bias is None else lin.bias.to(dtype)
    _check_rows(y, y_plain, Wd, x, ents, slot_vals, 1, b, dtype, f"bank {M}x{K} T={T} r={ranks}")
    slots.fill_(-1)                                      # no row on an adapter: the whole plain output
    assert torch.equal(lin(x), y_plain)
    slots.fill_(len(ranks))                              # the first index past the bank, on every row
    assert torch.equal(lin(x), y_plain)
    lin.clear_adapter_bank()


def test_bank_of_one_without_slots_serves_every_row(monkeypatch):
    """slots=None is slot == NULL in the launches: adapter 0 on every row."""
    M, K, T, ranks, dtype, seed = NOSLOT_CASE
    lin, Wd, _ = _lin(M, K, dtype)
    x, ents = _draw(M, K, T, ranks, dtype, seed)
    x, ents = x.to(DEV), _dev(ents)
    y_plain = lin(x)
    lin.set_adapter_bank(ents, None)
    calls = _count_fused(monkeypatch)
    y = lin(x)
    assert calls == [1]
    _check_rows(y, y_plain, Wd, x, ents, None, 1, None, dtype, "bank of one, no slots")
    lin.clear_adapter_bank()


def test_prefill_rows_of_a_stream_share_its_slot(monkeypatch):
    """x [B = 4, S = 3, K]: the three rows of stream b use slots[b]."""
    M, K, streams, S, ranks, dtype, slot_vals, seed = STREAM_CASE
    lin, Wd, _ = _lin(M, K, dtype)
    x, ents = _draw(M, K, streams * S, ranks, dtype, seed, S)
    x, ents = x.to(DEV), _dev(ents)
    assert x.shape == (streams, S, K)
    y_plain = lin(x)
    lin.set_adapter_bank(ents, _slots(slot_vals, n=4))
    calls = _count_fused(monkeypatch)
    y = lin(x)
    assert calls == [1] and y.shape == (streams, S, M)
    _check_rows(y, y_plain, Wd, x, ents, slot_vals, S, None, dtype, "[B, S, K] rows")
    # the same rows as 2-D x are one stream each: 12 streams do not fit 4 slots
    with pytest.raises(ValueError, match="streams"):
        lin(x.reshape(streams * S, K))
    lin.clear_adapter_bank()


# ---------------------------------------------------------------------------
# shrink_mt alone
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("ranks", [(1,), (16, 8), (64, 64, 64, 64)])      # 1, 24 and 256 rank rows per token
@pytest.mark.parametrize("K,T", [(1000, 2), (1024, 5), (4096, 16), (14336, 3)])
def test_shrink_mt_against_fp64(K, T, ranks, dtype):
    """The bar of the module docstring, per element of t; rows without an adapter are exactly 0.
    K = 1000 is served (16-B chunks: K % 8 == 0), and x rows may be strided (ldx = K + 8)."""
    from quantizations_amd import lora

    g = torch.Generator().manual_seed(K + sum(ranks) + T)
    n = 3
    xs = torch.randn(T, K + 8, generator=g).to(dtype).to(DEV)
    x = xs[:, :K]                                                  # row stride K + 8
    slot_vals = [0, 2, -1, 1, 99, 1, n, 0, 2, -7, 1, 0, 2, 2, 1, 0][:T]
    slots = _slots(slot_vals)
    banks, ents_all = [], []
    for i, r in enumerate(ranks):
        ents = [((torch.randn(r, K, generator=g) * 0.02).to(dtype).to(DEV), torch.zeros(8, r, dtype=dtype, device=DEV),
                 0.5 + 0.75 * (i + a)) for a in range(n)]
        ents_all.append(ents)
        banks.append(lora.AdapterBank(ents, slots, 8, K, DEV))
    t, offs = lora.shrink_mt(x, banks)
    assert t.shape == (T, sum(ranks)) and t.dtype == torch.float32
    assert offs == [sum(ranks[:i]) for i in range(len(ranks))]
    depth = 8 * math.ceil(K / 2048) + 9
    for c in range(T):
        a = slot_vals[c]
        xd = x[c].double()
        for ents, o, r in zip(ents_all, offs, ranks):
            got = t[c, o:o + r].double()
            if not 0 <= a < n:
                assert not got.any(), f"row {c} (slot {a}): t must be exactly 0"
                continue
            A, _, s = ents[a]
            tref = (A.double() @ xd) * s
            bound = depth * 2.0 ** -24 * s * (A.double().abs() @ xd.abs())
            err = (got - tref).abs()
            assert bool((err <= bound).all()), (c, r, (err / bound).max().item())


def test_shrink_mt_declines_unaligned_k():
    from quantizations_amd import _lib, lora

    x = torch.randn(3, 1004, device=DEV).half()
    ent = (torch.zeros(4, 1004, device=DEV).half(), torch.zeros(8, 4, device=DEV).half(), 1.0)
    bank = lora.AdapterBank([ent], _slots([0, 0, 0]), 8, 1004, DEV)
    assert not lora.bank_fused_ok(bank, x)                        # K % 8 != 0: the composed route
    with pytest.raises(_lib.QuantizationsError, match="shape"):
        lora.shrink_mt(x, [bank])


# ---------------------------------------------------------------------------
# grouped launch
# ---------------------------------------------------------------------------


def test_grouped_launch_with_banks_on_the_first_and_last_segment():
    """Three segments (M = 64, 16, 16); banks of rank 8 and 64 on the first and last: the middle
    segment's output is bit-identical to the plain grouped launch's."""
    from quantizations_amd import lora
    from quantizations_amd.core import gemm_4bit_grouped

    rows, K, T, ranks, slot_vals, _ = GROUP_CASE
    dtype = F16
    slots = _slots(slot_vals)
    x, drawn = _group_draw()
    x = x.to(DEV)
    items, banks, info = [], [], []
    for M, ents in zip(rows, drawn):
        lin, Wd, _ = _lin(M, K, dtype)
        items.append((lin.weight, lin.weight.quant_state, None))
        if ents is None:
            banks.append(None)
            info.append(None)
            continue
        ents = _dev(ents)
        banks.append(lora.AdapterBank(ents, slots, M, K, DEV))
        info.append((Wd, ents))
    t, offs = lora.shrink_mt(x, banks)
    lo = (t, [None if b is None else (b.B, o) for b, o in zip(banks, offs)], slots, 1)
    got = gemm_4bit_grouped(x, items, lora=lo)
    plain = gemm_4bit_grouped(x, items)
    assert torch.equal(got[1], plain[1]), "the segment without a bank: the plain launch's bits"
    for i in (0, 2):
        Wd, ents = info[i]
        _check_rows(got[i], plain[i], Wd, x, ents, slot_vals, 1, None, dtype, f"grouped segment {i}")


def test_decode_group_with_mixed_members(monkeypatch):
    """q has a bank, k a set_adapter adapter, v nothing: one shrink_mt launch, k keeps its composed
    term; then v gets a bank on ANOTHER slots tensor and takes the composed bank route."""
    import copy

    from quantizations_amd import lora
    from quantizations_amd.integration import fuse_projection_groups

    K, T, dtype = 1024, 4, F16
    slot_vals = [0, 2, -1, 1]
    att = torch.nn.Module()
    att.q_proj, att.k_proj, att.v_proj = (copy.deepcopy(_lin(M, K, dtype)[0]) for M in (64, 16, 16))
    x, drawn = _group_draw()
    x, q_ents, v_ents = x.to(DEV), _dev(drawn[0]), _dev(drawn[2])
    slots = _slots(slot_vals)
    att.q_proj.set_adapter_bank(q_ents, slots)
    att.k_proj.set_adapter(*_dev(_draw(16, K, T, (4,), dtype, 1)[1])[0])
    want_q, want_k, want_v = att.q_proj(x), att.k_proj(x), att.v_proj(x)       # each layer on its own
    assert fuse_projection_groups(att) == 1
    calls = _count_fused(monkeypatch)
    xi = x.clone()
    q, k, v = att.q_proj(xi), att.k_proj(xi), att.v_proj(xi)
    assert calls == [1]
    assert torch.equal(q, want_q) and torch.equal(k, want_k) and torch.equal(v, want_v)
    other = _slots(slot_vals)                                                   # equal values, another tensor
    att.v_proj.set_adapter_bank(v_ents, other)
    xi = x.clone()
    q, k, v2 = att.q_proj(xi), att.k_proj(xi), att.v_proj(xi)
    assert calls == [1, 1], "only q's bank (the first bank's slots) rides the fused route"
    assert torch.equal(q, want_q) and torch.equal(k, want_k)
    assert torch.equal(v2, want_v + lora.composed_bank_term(att.v_proj.adapter_bank, x, dtype))


# ---------------------------------------------------------------------------
# the composed route
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("case", COMPOSED_CASES, ids=lambda c: c[0])
def test_composed_bank_route(case, monkeypatch):
    name, M, K, T, ranks, dtype, slot_vals, seed = case
    adt = F16 if dtype == torch.float32 else dtype
    lin, Wd, W32 = _lin(M, K, dtype)
    x, ents = _draw(M, K, T, ranks, adt, seed)
    x = x.to(dtype).to(DEV)
    ents = _dev(ents)
    # one token multiplies the fp32 operand (the decode GEMV with exact codes)
    Wref = Wd if T > 1 else W32
    y_plain = lin(x)
    slots = _slots(slot_vals, n=max(16, T))
    lin.set_adapter_bank(ents, slots)
    calls = _count_fused(monkeypatch)
    y = lin(x)
    assert calls == [] and y.dtype == dtype and y.shape == (T, 1, M)
    base, ad, adapted = _row_terms(Wref, x, ents, slot_vals, 1)
    for c in range(T):
        if not adapted[c]:
            assert torch.equal(y[c], y_plain[c])                  # + 0 of the masked term
            continue
        assert ad[c].norm() >= 0.25 * base[c].norm()
        assert_close(y[c].double().cpu().numpy(), (base[c] + ad[c]).cpu().numpy(), dtype, f"composed {name} row {c}")
    if name == "one token":
        # no host read of slots anywhere on the route: it can be captured, and the replay reads
        # whatever slots holds then
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            lin(x)
        torch.cuda.current_stream().wait_stream(s)
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph):
            yg = lin(x)
        gph.replay()
        torch.cuda.synchronize()
        assert torch.equal(yg, y)
        slots[0] = 2
        want = lin(x)
        gph.replay()
        torch.cuda.synchronize()
        assert torch.equal(yg, want) and not torch.equal(yg, y)
    lin.clear_adapter_bank()


# ---------------------------------------------------------------------------
# graph: slots and put() are read at replay
# ---------------------------------------------------------------------------


def test_captured_fused_step_follows_slots_and_put():
    M, K, T, ranks, dtype, qt, dq, bias, slot_vals, seed = CASES[2]
    lin, _, _ = _lin(M, K, dtype)
    x, ents = _draw(M, K, T, ranks, dtype, seed)
    x, ents = x.to(DEV), _dev(ents)
    slots = _slots(slot_vals)
    lin.set_adapter_bank(ents, slots)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        lin(x)
    torch.cuda.current_stream().wait_stream(s)
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph):
        yg = lin(x)
    gph.replay()
    torch.cuda.synchronize()
    y0 = lin(x)
    assert torch.equal(yg, y0)
    slots.copy_(_slots([2, 0, 1, -1]))                               # (a) new slots
    gph.replay()
    torch.cuda.synchronize()
    y1 = lin(x)
    assert torch.equal(yg, y1) and not torch.equal(y1, y0)
    A3, B3, _ = _dev(_draw(M, K, T, (3,), dtype, 5)[1])[0]           # (b) put: a smaller rank into entry 2
    lin.adapter_bank.put(2, A3, B3, 0.75)
    gph.replay()
    torch.cuda.synchronize()
    y2 = lin(x)
    assert torch.equal(yg, y2) and not torch.equal(y2, y1)
    assert torch.equal(y2[1:], y1[1:])                               # only the stream on entry 2 moved
    lin.clear_adapter_bank()


# ---------------------------------------------------------------------------
# whole model: four streams, three adapters, one stream on none
# ---------------------------------------------------------------------------


def _decode_batch(model, cfg, ids, toks=None, steps=3):
    """Logits of the prefill's last token and of `steps` decode steps for the streams of ids
    [B, 9]; toks (a list of [B, 1] tensors) forces the input tokens, else each stream's argmax."""
    from transformers.cache_utils import StaticCache

    B = ids.shape[0]
    cache = StaticCache(config=cfg, max_cache_len=32)
    out = model(input_ids=ids, past_key_values=cache, cache_position=torch.arange(9, device=DEV))
    logits, used = [out.logits[:, -1].clone()], []
    tok = out.logits[:, -1:].argmax(-1)
    pos = torch.tensor([9], device=DEV)
    for i in range(steps):
        if toks is not None:
            tok = toks[i]
        used.append(tok.clone())
        lo = model(input_ids=tok, past_key_values=cache, cache_position=pos,
                   position_ids=pos.view(1, 1).expand(B, 1)).logits
        logits.append(lo[:, -1].clone())
        tok = lo[:, -1:].argmax(-1)
        pos.add_(1)
    torch.cuda.synchronize()
    return logits, used


# B of the whole-model adapters is LLAMA_B_SCALE * randn / sqrt(r) (A = 0.02 randn as everywhere): see
# test_tiny_llama_four_streams_three_adapters
LLAMA_B_SCALE = 0.25


def _llama_adapters(model, seed, ranks):
    import quantizations_amd as qa

    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, m in model.named_modules():
        leaf = name.split(".")[-1]
        if isinstance(m, qa.Linear4bit) and leaf in ranks:
            r = ranks[leaf]
            out[name] = ((torch.randn(r, m.in_features, generator=g) * 0.02).half(),
                         (torch.randn(m.out_features, r, generator=g) * (LLAMA_B_SCALE / math.sqrt(r))).half(), 1.0)
    return out


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def test_tiny_llama_four_streams_three_adapters(monkeypatch):
    """Four streams (slots [0, 1, -1, 2]) through the tiny Llama with every fusion on, adapters on all
    seven projections: the prefill's last logits (36 rows: the composed route) and three decode steps
    (4 rows: the fused route), per stream against the dense-fp32 model with that stream's adapter
    merged, at rel < 2e-3 (the bar of test_gpu_lora.test_tiny_llama_with_adapters).

    The reference keeps fp16 activations, as the model does, so both carry the rounding noise of the
    residual stream, and the bar measures their difference.  Two preconditions on the REFERENCE keep
    that meaningful: (1) its own error -- against the same merged model run with fp32 activations --
    is at most bar / sqrt(2) for every figure (a model exactly as accurate as the reference, with
    independent roundings, then sits at the bar; above that the bar would be asking the model to be
    better than its reference), and (2) every adapter moves its stream's logits by at least 25x the
    bar, so a dropped or swapped adapter cannot pass.

    B is scaled by LLAMA_B_SCALE = 1/4 because of (1).  With B = randn / sqrt(r) the adapter term
    equals the base term in every projection, q and k among them, which doubles the attention scores
    and with them the model's sensitivity to rounding: measured on one MI355X, the reference's own
    error was then 0.97e-3 .. 1.58e-3 (over bar / sqrt(2) = 1.41e-3 in four figures; 1.03e-3 ..
    1.08e-3 for the stream without an adapter), and the model's figures 1.16e-3 .. 1.80e-3 for the
    fused decode steps and 1.93e-3, 2.11e-3 and 2.67e-3 for the three adapted streams' composed
    prefill.  A quarter is the smallest adapter-to-base ratio the layer tests above accept; the
    adapters then still move the logits by 0.6 (300x the bar), the reference's own error is 0.88e-3 ..
    1.08e-3 and the model's figures 1.1e-3 .. 1.5e-3."""
    import copy

    import quantizations_amd as qa
    from quantizations_amd.integration import (fuse_layer_ops, fuse_prenorm, fuse_projection_groups,
                                               unfuse_layer_ops, unfuse_projection_groups)
    from test_gpu_lora import _tiny_llama

    cfg, model = _tiny_llama()
    ranks = {"q_proj": 16, "k_proj": 8, "v_proj": 64, "o_proj": 16, "gate_proj": 4, "up_proj": 16, "down_proj": 3}
    ads = [_llama_adapters(model, 21 + i, ranks) for i in range(3)]
    mods = dict(model.named_modules())
    ids = torch.randint(0, 512, (4, 9), device=DEV, generator=torch.Generator(device="cuda").manual_seed(1))
    stream_slots = [0, 1, -1, 2]
    slots = _slots(stream_slots)

    class DenseF32(torch.nn.Linear):
        """fp32 weight, fp32 matmul, on the model's activations"""
        def forward(self, x):
            return torch.nn.functional.linear(x.float(), self.weight).to(x.dtype)

    def dense_ref(ad):
        """the same model with every Linear4bit as a dense fp32 nn.Linear holding dequantize() + s B A"""
        ref = copy.deepcopy(model)
        for name, m in list(ref.named_modules()):
            if isinstance(m, qa.Linear4bit):
                W = mods[name].dequantize().float()
                if name in ad:
                    A, B, s = ad[name]
                    W = W + s * (B.float().to(DEV) @ A.float().to(DEV))
                lin = DenseF32(m.in_features, m.out_features, bias=False, device=DEV, dtype=torch.float32)
                lin.weight.data.copy_(W)
                parent = ref.get_submodule(name.rsplit(".", 1)[0])
                parent._modules[name.rsplit(".", 1)[1]] = lin
        return ref

    with torch.no_grad():
        fuse_projection_groups(model)
        fuse_layer_ops(model)
        fuse_prenorm(model)
        try:
            for name in ads[0]:
                mods[name].set_adapter_bank([a[name] for a in ads], slots)
            assert sum(m.adapter_bank is not None for m in mods.values() if isinstance(m, qa.Linear4bit)) == \
                7 * cfg.num_hidden_layers
            calls = _count_fused(monkeypatch)
            got, used = _decode_batch(model, cfg, ids)
            # per decode step and layer: q/k/v, o, gate/up, down -- one shrink_mt launch each
            assert len(calls) == 3 * cfg.num_hidden_layers * 4, len(calls)
        finally:
            unfuse_layer_ops(model)
        for name in ads[0]:
            mods[name].clear_adapter_bank()
        unfuse_projection_groups(model)
        rels, own, moved = {}, {}, {}
        plain_ref = dense_ref({})
        for b, a in enumerate(stream_slots):
            toks = [t[b:b + 1] for t in used]
            ref = dense_ref(ads[a]) if a >= 0 else plain_ref
            want, _ = _decode_batch(ref, cfg, ids[b:b + 1], toks=toks)
            exact, _ = _decode_batch(copy.deepcopy(ref).float(), cfg, ids[b:b + 1], toks=toks)   # fp32 activations
            base, _ = _decode_batch(plain_ref, cfg, ids[b:b + 1], toks=toks) if a >= 0 else (None, None)
            for i, (g, w, e) in enumerate(zip(got, want, exact)):
                rels[b, i], own[b, i] = _rel(g[b], w[0]), _rel(w[0], e[0])
                if a >= 0:
                    moved[b, i] = _rel(w[0], base[i][0])
                print(f"tiny llama stream {b} (adapter {a}) step {i}: logits rel err {rels[b, i]:.3e}  "
                      f"(reference's own {own[b, i]:.3e}, adapter moves the logits by {moved.get((b, i), 0.0):.3e})")
        own_bar = 2e-3 / math.sqrt(2)
        assert all(r <= own_bar for r in own.values()), {k: f"{r:.3e}" for k, r in own.items() if r > own_bar}
        assert all(r >= 0.05 for r in moved.values()), {k: f"{r:.3e}" for k, r in moved.items() if r < 0.05}
        assert all(r < 2e-3 for r in rels.values()), {k: f"{r:.3e}" for k, r in rels.items() if r >= 2e-3}
