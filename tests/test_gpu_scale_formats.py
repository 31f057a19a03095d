"""GPU: the 4-bit kernels over the scale layout -- blocksize, the nested blocksize2, and rows that
start inside a scale block (tests/scale_formats.py has the weights and the cases;
tests/test_scale_formats.py shows on the CPU that the cases can see a wrong scale index).

* Readback, bit-exact: one-hot tokens / gradients read every weight of every straddling and
  "K divides the block" case back through each MFMA kernel; it must be the oracle's dequantised
  weight.  The weights are block-tagged, so a scale taken from another block is off by >= 2x.
* Products on the suite's existing bars (test_gpu_parity.assert_close for 16-bit outputs, 1e-5
  relative for fp32 x, 2^-8 for bf16 x) on every case, the fused decode forms on the aligned ones.
* Row shards whose scales start inside a second-level block.

Every reference is the ORACLE's dequantize / gemv of the oracle's own quantisation; the GPU
QuantState is built by hand from the oracle's arrays (so blocksize2 != 256 is expressible).
"""
import numpy as np
import pytest
import torch

import scale_formats as sf
from test_gpu_parity import assert_close
from test_gpu_weight_range import _assert_operand, _gpu_state, _one_hot

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DT_IDS = {F16: "fp16", BF16: "bf16", F32: "fp32"}

_wd = {}


def _weight(c, qt, dt, shift=0):
    """(packed, state, Wd [M, K] in dt on the GPU = the oracle's dequantised weight rounded once)."""
    import oracle

    o = sf.oracle_state(c, qt, shift)
    key = (c.name, qt, dt, shift)
    if key not in _wd:
        _wd[key] = torch.from_numpy(oracle.dequantize(o)).to(dt)
    packed, st = _gpu_state(o)
    return packed, st, _wd[key].to(DEV)


def _workspace(T, c):
    from quantizations_amd._lib import lib

    return int(lib.qz_gemm_4bit_workspace_size(T, c.M, c.K))


# ---------------------------------------------------------------------------
# readback: the W operand of each MFMA kernel, every weight
# ---------------------------------------------------------------------------

M8 = [c for c in sf.READBACK if c.M % 8 == 0]
K256 = [c for c in sf.READBACK if c.K % 256 == 0]


def test_readback_case_lists():
    assert len(M8) == len(sf.READBACK) - 1
    assert {(c.K, c.bs) for c in K256 if c.kind == "straddle"} == {(768, 512), (6144, 4096)}
    # split-K (a workgroup whose K range starts at kbeg != 0) runs in the 128-row tile readbacks
    assert any(_workspace(64, c) > 0 and _workspace(256, c) > 0 for c in sf.STRADDLING)


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS.get)
@pytest.mark.parametrize("c", sf.READBACK, ids=sf.case_id)
def test_tile128_readback(c, dt, qt):
    """gemm_4bit(route='fused') on the 128-row tile kernel at T = 64 (64-token tile) and T = 256
    (128-token tiles) per launch; every column, so every (row, K-step) pair and every split."""
    from quantizations_amd.core import gemm_4bit

    packed, st, Wd = _weight(c, qt, dt)
    if c.K in (2112, 768):
        assert _workspace(64, c) > 0 and _workspace(256, c) > 0
    for T in (64, 256):
        for c0 in range(0, c.K, T):
            cols = torch.arange(c0, c0 + T, device=DEV) % c.K
            Y = gemm_4bit(_one_hot(T, c.K, cols, dt), packed, st, route="fused")
            _assert_operand(Y, Wd[:, cols].t(), f"{c.name} {qt} {dt} T={T} columns {c0}..")


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS.get)
@pytest.mark.parametrize("c", M8, ids=sf.case_id)
def test_tile256_readback(c, dt, qt):
    """The 256 x 256 tile kernel at T = 4096, columns (37 i) % K (37 and K are coprime)."""
    from quantizations_amd.core import gemm_4bit

    packed, st, Wd = _weight(c, qt, dt)
    seen = torch.zeros(c.K, dtype=torch.bool, device=DEV)
    for j in range((c.K + 4095) // 4096):
        cols = ((torch.arange(4096, device=DEV) + 4096 * j) * 37) % c.K
        Y = gemm_4bit(_one_hot(4096, c.K, cols, dt), packed, st, route="fused")
        _assert_operand(Y, Wd[:, cols].t(), f"{c.name} {qt} {dt} launch {j}")
        seen[cols] = True
    assert seen.all()


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS.get)
@pytest.mark.parametrize("c", K256, ids=sf.case_id)
def test_multi_token_readback(c, dt, qt):
    """The multi-token kernel: T = 16 over every column, T = 2 at three column pairs."""
    from quantizations_amd.core import gemm_4bit

    packed, st, Wd = _weight(c, qt, dt)
    for c0 in range(0, c.K, 16):
        cols = torch.arange(c0, c0 + 16, device=DEV)
        Y = gemm_4bit(_one_hot(16, c.K, cols, dt), packed, st, route="fused")
        _assert_operand(Y, Wd[:, cols].t(), f"{c.name} {qt} {dt} T=16 columns {c0}..")
    for c0 in (0, 77, c.K - 2):
        cols = torch.tensor([c0, (c0 + c.K // 2 + 1) % c.K], device=DEV)
        Y = gemm_4bit(_one_hot(2, c.K, cols, dt), packed, st, route="fused")
        _assert_operand(Y, Wd[:, cols].t(), f"{c.name} {qt} {dt} T=2 columns {cols.tolist()}")


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS.get)
@pytest.mark.parametrize("c", K256, ids=sf.case_id)
def test_grouped_multi_token_readback(c, dt, qt):
    """gemm_4bit_grouped: two weights of one format whose tags are two blocks out of step."""
    from quantizations_amd.core import gemm_4bit_grouped

    ws = [_weight(c, qt, dt, shift) for shift in (0, 2)]
    assert not torch.equal(ws[0][2], ws[1][2])
    items = [(p, st, None) for p, st, _ in ws]
    for c0 in range(0, c.K, 16):
        cols = torch.arange(c0, c0 + 16, device=DEV)
        ys = gemm_4bit_grouped(_one_hot(16, c.K, cols, dt), items)
        for i, (y, (_, _, Wd)) in enumerate(zip(ys, ws)):
            _assert_operand(y, Wd[:, cols].t(), f"{c.name} weight {i} {qt} {dt} columns {c0}..")


@pytest.mark.parametrize("qt", ["fp4", "nf4"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS.get)
@pytest.mark.parametrize("c", M8, ids=sf.case_id)
def test_dgrad_readback(c, dt, qt):
    """gemm_4bit_dgrad(route='fused'): one-hot gradients pick rows; T = 130 reads every row, T = 16
    two more groups of rows."""
    from quantizations_amd.core import gemm_4bit_dgrad

    packed, st, Wd = _weight(c, qt, dt)
    for T, starts in ((130, range(0, c.M, 130)), (16, (0, max(c.M - 13, 0)))):
        for r0 in starts:
            rows = torch.arange(r0, r0 + T, device=DEV) % c.M
            dX = gemm_4bit_dgrad(_one_hot(T, c.M, rows, dt), packed, st, route="fused")
            _assert_operand(dX, Wd[rows], f"{c.name} {qt} {dt} T={T} rows {r0}..")


# ---------------------------------------------------------------------------
# products on the existing bars
# ---------------------------------------------------------------------------


def _on_bar(y, yref, dt, what):
    """The bars of test_gemv_bf16_fp32_tables_on_every_geometry (fp32 x: 1e-5, bf16 x: 2^-8,
    relative, in the norm) and assert_close; each figure is printed before it is asserted."""
    y = y.double().cpu().numpy().ravel()
    yref = np.asarray(yref, np.float64).ravel()
    assert np.isfinite(y).all(), what
    rel = float(np.linalg.norm(y - yref) / np.linalg.norm(yref))
    print(f"{what}: rel {rel:.3e}")
    if dt == F32:
        assert rel <= 1e-5, (what, rel)
    elif dt == BF16:
        assert rel <= 2.0 ** -8, (what, rel)
    assert_close(y, yref, dt, what)


def _x(n, dt, seed, rows=None):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*(() if rows is None else (rows,)), n, generator=g).to(dt)


@pytest.mark.parametrize("dt,exact", [(F16, None), (F16, True), (BF16, None), (F32, None)],
                         ids=["fp16", "fp16-exact", "bf16", "fp32"])
@pytest.mark.parametrize("c", sf.CASES, ids=sf.case_id)
def test_gemv_products(orc, c, dt, exact):
    """gemv_4bit, and gemv_4bit_grouped with a second weight of the same format, against the
    oracle's fp32 weight products summed in fp64."""
    from quantizations_amd.core import gemv_4bit, gemv_4bit_grouped

    qt = sf.quant_type_of(c)
    os_ = [sf.oracle_state(c, qt, shift) for shift in (0, 2)]
    x = _x(c.K, dt, seed=c.M + c.K)
    xd = x.to(DEV).reshape(1, c.K)
    packed, st = _gpu_state(os_[0])
    y = gemv_4bit(xd, packed, state=st, exact_codes=exact)
    assert y.dtype == dt and y.shape == (1, c.M)
    _on_bar(y, orc.gemv(x.float().numpy(), os_[0]), dt, f"gemv {c.name} {qt} {dt} exact={exact}")
    ys = gemv_4bit_grouped(xd, [(*_gpu_state(o), None) for o in os_], exact_codes=exact)
    for i, (o, yg) in enumerate(zip(os_, ys)):
        _on_bar(yg, orc.gemv(x.float().numpy(), o), dt, f"grouped {c.name} weight {i} {qt} {dt} exact={exact}")


def _linear(c, qt, dt, shift=0):
    """A Linear4bit around the oracle's quantisation (never re-quantised)."""
    import quantizations_amd as qa

    packed, st, _ = _weight(c, qt, dt, shift)
    m = qa.Linear4bit(c.K, c.M, bias=False, quant_type=qt, compute_dtype=dt, compress_statistics=c.bs2 is not None,
                      device="meta")
    m.weight = qa.Params4bit(packed, requires_grad=False, quant_state=st, blocksize=c.bs, quant_type=qt, module=m,
                             bnb_quantized=True, compress_statistics=c.bs2 is not None)
    m.quant_state = st
    return m


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS.get)
@pytest.mark.parametrize("c", sf.CASES, ids=sf.case_id)
def test_linear4bit_forward(orc, c, dt):
    """Linear4bit.forward at T = 1 (GEMV), 5 (multi-token kernel or 64-token tile), 40 (128-row tile
    kernel) and 600 (the auto route's choice, and the tile kernel's 128-token tiles by
    route='fused'), against fp64 of the oracle's weight in the dtype the route multiplies
    (decode: the fp32 products; prefill: rounded to dt)."""
    from quantizations_amd.core import gemm_4bit

    qt = sf.quant_type_of(c)
    o = sf.oracle_state(c, qt)
    m = _linear(c, qt, dt)
    _, _, Wd = _weight(c, qt, dt)
    for T in (1, 5, 40, 600):
        X = _x(c.K, dt, seed=T, rows=T)
        with torch.no_grad():
            y = m(X.to(DEV).reshape(1, T, c.K))
        assert y.shape == (1, T, c.M) and y.dtype == dt
        if T == 1:
            ref = orc.gemv(X.float().numpy().ravel(), o)
        else:
            ref = (X.to(DEV).double() @ Wd.double().t()).cpu().numpy()
        assert_close(torch.from_numpy(np.asarray(ref)).to(dt).double().numpy(), ref, dt, "the rounded reference")
        _on_bar(y.reshape(T, c.M), ref, dt, f"Linear4bit {c.name} {qt} {dt} T={T}")
        if T == 600:
            yf = gemm_4bit(X.to(DEV), m.weight, m.weight.quant_state, route="fused")
            _on_bar(yf, ref, dt, f"gemm_4bit fused {c.name} {qt} {dt} T={T}")


# ---------------------------------------------------------------------------
# the fused decode forms on the aligned cases
# ---------------------------------------------------------------------------

# (blocksize, blocksize2) -> launch form.  Every aligned case has K % 2048 == 0, K % blocksize == 0
# and blocksize2 a multiple of the 2048 / blocksize blocks of a K-step, which is all full_steps()
# asks of the format: no launch declines it, every one takes its fused form (DESIGN.md has the table).
FUSED_FORMS = {"grouped": "grouped (norm fused)", "pair": "pair", "pair+norm": "pair (norm fused)"}


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS.get)
@pytest.mark.parametrize("c", sf.ALIGNED, ids=sf.case_id)
def test_fused_decode_forms(orc, c, dt):
    """Grouped + RMSNorm, the SiLU pair with and without the norm and the residual epilogue: each
    bit-identical to its unfused composition (as at blocksize 64), on the bar, in the fused form."""
    from quantizations_amd import core
    from quantizations_amd.core import gemv_4bit, gemv_4bit_grouped, gemv_4bit_pair_silu
    from quantizations_amd.layer_ops import rms_norm, silu_mul

    qt = sf.quant_type_of(c)
    os_ = [sf.oracle_state(c, qt, shift) for shift in (0, 2)]
    items = [(*_gpu_state(o), None) for o in os_]
    # x and the norm weight at 1/4: gate and up stay near 10 and their product far below fp16's 65504
    x = (_x(c.K, dt, seed=c.K + c.bs) * 0.25).to(DEV).reshape(1, c.K)
    nw = (0.25 * (1 + 0.1 * _x(c.K, F32, seed=c.K + 1))).to(dt).to(DEV)
    xn = rms_norm(x, nw, 1e-5)

    def refs(xin):
        return [orc.gemv(xin.float().cpu().numpy().ravel(), o) for o in os_]

    def silu_ref(xin):
        g, u = (torch.from_numpy(v).to(dt).double().numpy() for v in refs(xin))   # the launch rounds gate and up
        return g / (1 + np.exp(-g)) * u

    # grouped + RMSNorm
    core.LAST_FORM.clear()
    ys = gemv_4bit_grouped(x, items, norm=(nw, 1e-5))
    assert core.LAST_FORM["grouped"] == FUSED_FORMS["grouped"], (c.name, core.LAST_FORM)
    plain = gemv_4bit_grouped(xn, items)
    for i, (a, b, r) in enumerate(zip(ys, plain, refs(xn))):
        assert torch.equal(a, b), f"grouped + norm, weight {i}"
        _on_bar(a, r, dt, f"grouped + norm {c.name} weight {i} {dt}")
    # the SiLU pair, without and with the norm
    g, u = gemv_4bit_grouped(x, items)
    h = gemv_4bit_pair_silu(x, items)
    assert h is not None and core.LAST_FORM["pair"] == FUSED_FORMS["pair"], (c.name, core.LAST_FORM)
    hn = gemv_4bit_pair_silu(x, items, norm=(nw, 1e-5))
    assert hn is not None and core.LAST_FORM["pair"] == FUSED_FORMS["pair+norm"], (c.name, core.LAST_FORM)
    assert torch.equal(hn, gemv_4bit_pair_silu(xn, items)), "pair + norm against norm, then pair"
    _on_bar(h, silu_ref(x), dt, f"pair {c.name} {dt}")
    _on_bar(hn, silu_ref(xn), dt, f"pair + norm {c.name} {dt}")
    # against the grouped launch + product: these few rows make the grouped launch split K over
    # waves while the pair keeps whole rows per wave -- another fp32 summation order, so the bar of
    # test_pair_silu_whole_rows_at_k8192 (the same bits wherever the geometries agree)
    # (fp16: its norm bar; bf16: assert_close, which takes the output format's own ulp out)
    ref = silu_mul(g, u)
    same = torch.equal(h, ref)
    rel = ((h.float() - ref.float()).norm() / ref.float().norm()).item()
    print(f"pair vs grouped + silu_mul {c.name} {dt}: rel {rel:.3e}, same bits {same}")
    if not same and dt == F16:
        assert rel < 2e-3
    elif not same:
        assert_close(h.double().cpu().numpy(), ref.double().cpu().numpy(), dt, f"pair vs grouped {c.name}")
    # the residual epilogue
    res = (_x(c.M, dt, seed=6) * 4).to(DEV).reshape(1, c.M)
    y = gemv_4bit(x, items[0][0], state=items[0][1])
    assert torch.equal(gemv_4bit(x, items[0][0], state=items[0][1], residual=res), res + y)


@pytest.mark.parametrize("dt", [F16, BF16], ids=DT_IDS.get)
@pytest.mark.parametrize("c", sf.ALIGNED, ids=sf.case_id)
def test_lora_forms(orc, c, dt):
    """One LoRA GEMV (r = 16; on the bar, its residual form the torch add of it) and the bank epilogue
    of gemm_4bit_grouped (rows and weights without an adapter: the plain launch's bits, themselves
    the multi-token kernel's; adapted rows on the bar)."""
    from quantizations_amd import lora
    from quantizations_amd.core import gemm_4bit, gemm_4bit_grouped, gemv_4bit

    qt = sf.quant_type_of(c)
    r = 16
    g = torch.Generator().manual_seed(c.M + 7 * c.K + c.bs)
    A = (torch.randn(r, c.K, generator=g) * 0.02).to(dt).to(DEV)
    B = (torch.randn(c.M, r, generator=g) * (12 / r ** 0.5)).to(dt).to(DEV)
    o = sf.oracle_state(c, qt)
    packed, st, Wd = _weight(c, qt, dt)
    x = _x(c.K, dt, seed=c.K + 3)
    xd = x.to(DEV).reshape(1, 1, c.K)
    base = orc.gemv(x.float().numpy(), o)
    ad = (B.double() @ (A.double() @ xd.double().reshape(-1))).cpu().numpy()
    assert np.linalg.norm(ad) >= 0.25 * np.linalg.norm(base)
    t, _ = lora.shrink(xd, [lora.LoraAdapter(A, B, 1.0, DEV)])
    y = gemv_4bit(xd, packed, state=st, lora=(B, t))
    _on_bar(y, base + ad, dt, f"lora gemv {c.name} {dt}")
    res = (_x(c.M, dt, seed=6) * 4).to(DEV).reshape(1, 1, c.M)
    assert torch.equal(gemv_4bit(xd, packed, state=st, residual=res, lora=(B, t)), res + y)
    # the bank epilogue: 4 rows, slots [0, -1, 1, 0]; the second weight carries no bank
    T, slot_vals = 4, [0, -1, 1, 0]
    slots = torch.tensor(slot_vals, dtype=torch.int32, device=DEV)
    ents = [(A, B, 1.0), ((A * 0.5).to(dt), B, -1.0)]
    p2, st2, Wd2 = _weight(c, qt, dt, shift=2)
    items = [(packed, st, None), (p2, st2, None)]
    banks = [lora.AdapterBank(ents, slots, c.M, c.K, DEV), None]
    X = _x(c.K, dt, seed=c.K + 4, rows=T).to(DEV)
    tt, offs = lora.shrink_mt(X, banks)
    got = gemm_4bit_grouped(X, items, lora=(tt, [(banks[0].B, offs[0]), None], slots, 1))
    plain = gemm_4bit_grouped(X, items)
    assert torch.equal(got[1], plain[1])
    for y_, (p_, s_, _), W_ in zip(plain, items, (Wd, Wd2)):
        assert torch.equal(y_, gemm_4bit(X, p_, s_, route="fused"))
        _on_bar(y_, (X.double() @ W_.double().t()).cpu().numpy(), dt, f"grouped multi-token {c.name} {dt}")
    for row, a in enumerate(slot_vals):
        if a < 0:
            assert torch.equal(got[0][row], plain[0][row])
            continue
        Ae, Be, s = ents[a]
        ref = X[row].double() @ Wd.double().t() + s * (Be.double() @ (Ae.double() @ X[row].double()))
        assert not torch.equal(got[0][row], plain[0][row])
        _on_bar(got[0][row], ref.cpu().numpy(), dt, f"bank row {row} {c.name} {dt}")


@pytest.mark.parametrize("c", sf.READBACK, ids=sf.case_id)
def test_unaligned_formats_take_the_unfused_forms(orc, c):
    """Rows that start mid-block (or K % 2048 != 0): the full-step launches decline -- the norm runs
    as its own launch, the pair returns None -- and the grouped result still meets the bar."""
    from quantizations_amd import core
    from quantizations_amd.core import gemv_4bit_grouped, gemv_4bit_pair_silu
    from quantizations_amd.layer_ops import rms_norm

    qt = sf.quant_type_of(c)
    os_ = [sf.oracle_state(c, qt, shift) for shift in (0, 2)]
    items = [(*_gpu_state(o), None) for o in os_]
    x = (_x(c.K, F16, seed=c.K) * 3).to(DEV).reshape(1, c.K)
    nw = (1 + 0.1 * _x(c.K, F32, seed=c.K + 1)).half().to(DEV)
    core.LAST_FORM.clear()
    ys = gemv_4bit_grouped(x, items, norm=(nw, 1e-5))
    assert core.LAST_FORM["grouped"] == "norm launch + grouped", (c.name, core.LAST_FORM)
    xn = rms_norm(x, nw, 1e-5)
    for i, (o, y) in enumerate(zip(os_, ys)):
        _on_bar(y, orc.gemv(xn.float().cpu().numpy().ravel(), o), F16, f"norm launch + grouped {c.name} weight {i}")
    assert gemv_4bit_pair_silu(x, items) is None and gemv_4bit_pair_silu(x, items, norm=(nw, 1e-5)) is None


# ---------------------------------------------------------------------------
# row shards
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("c", sf.SHARDS, ids=sf.case_id)
def test_row_shards(orc, c, world):
    """shard_rows of a nested format: each shard's gemv_4bit, grouped launch and
    RowShardedLinear4bit.forward (1, 5, 40 tokens) give the bits of the unsharded call's columns.
    A shard whose scales start inside a second-level block (block_base != 0) serves one token and
    the grouped multi-token launch; its module refuses prefill (the tile kernels take no
    block_base), which is asserted, not skipped."""
    from quantizations_amd.core import gemm_4bit, gemm_4bit_grouped, gemv_4bit, gemv_4bit_grouped
    from quantizations_amd.parallel import RowShardedLinear4bit, shard_rows

    qt, dt = "nf4", F16
    o = sf.oracle_state(c, qt)
    full = _linear(c, qt, dt)
    packed, st = full.weight.data, full.weight.quant_state
    xs = {T: _x(c.K, dt, seed=T, rows=T).to(DEV) for T in (1, 5, 40)}
    with torch.no_grad():
        want = {T: full(x) for T, x in xs.items()}
    _on_bar(want[1], orc.gemv(xs[1].float().cpu().numpy().ravel(), o), dt, f"unsharded gemv {c.name}")
    bases = []
    for rank in range(world):
        sh = shard_rows(packed, st, rank, world)
        bases.append(sh.block_base)
        cols = slice(sh.r0, sh.r1)
        y = gemv_4bit(xs[1], sh.packed, state=sh.state, block_base=sh.block_base)
        assert torch.equal(y, want[1][:, cols]), (c.name, world, rank, "gemv")
        (yg,) = gemv_4bit_grouped(xs[1], [(sh.packed, sh.state, None, sh.block_base)])
        assert torch.equal(yg, want[1][:, cols]), (c.name, world, rank, "grouped")
        (y5,) = gemm_4bit_grouped(xs[5], [(sh.packed, sh.state, None, sh.block_base)])
        assert torch.equal(y5, want[5][:, cols]), (c.name, world, rank, "grouped multi-token")
        mod = RowShardedLinear4bit(full, rank, world, gather=False)
        with torch.no_grad():
            assert torch.equal(mod(xs[1]), want[1][:, cols])
            for T in (5, 40):
                if sh.block_base != 0:
                    with pytest.raises(ValueError, match="block-aligned second-level"):
                        mod(xs[T])
                else:
                    assert torch.equal(mod(xs[T]), want[T][:, cols]), (c.name, world, rank, T)
    if (c.bs, world) == (4096, 4):
        assert any(b != 0 for b in bases), bases
    assert torch.equal(want[40], gemm_4bit(xs[40], packed, st, route="fused"))
