"""GPU: the wide multi-token 4-bit kernel (csrc/gemm_mt_wide.hip, 17..64 rows) and what reaches it:
core.gemm_4bit_wide / gemm_4bit_grouped_wide, the modules' decode_rows opt-in, the sessions' keyword.

Weights are tests/scale_formats.py's block-tagged ones (a scale from a wrong block is off by >= 2x),
quantised by the oracle.  Every output is held to test_gpu_scale_formats._on_bar (the multi-token
kernel's own bar) against the fp64 product of the oracle's dequantised weight, and every 16-row slice
to the bits of the existing 2..16-row kernel on those rows alone.  Shapes: K = 512 (six waves own no
chunk), 2048 (one chunk per wave), 2304 (nine chunks, and at blocksize 4096 rows that start inside a
scale block); M = 16, 20 (ragged last row block), 48; T = every NB with full and one-row last blocks."""
import pytest
import torch

import scale_formats as sf
from test_gpu_generation_speculative import _build, _unprepare
from test_gpu_scale_formats import _on_bar, _weight

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
F16, BF16 = torch.float16, torch.bfloat16
TS = (17, 31, 32, 33, 48, 49, 64)
# (K, M, blocksize, blocksize2, quant type, dtype): every (K, M), and blocksize 4096 at K = 2304
CASES = [(512, 16, 64, None, "nf4", F16), (512, 20, 64, 256, "fp4", BF16), (512, 48, 64, 256, "nf4", BF16),
         (2048, 16, 64, 256, "fp4", F16), (2048, 20, 64, None, "nf4", BF16), (2048, 48, 64, None, "fp4", F16),
         (2304, 16, 64, 256, "nf4", BF16), (2304, 20, 64, None, "fp4", F16), (2304, 48, 64, 256, "nf4", F16),
         (2304, 20, 4096, 64, "nf4", F16), (2304, 48, 4096, None, "fp4", BF16)]


def _id(c):
    return f"K{c[0]}-M{c[1]}-b{c[2]}-n{c[3]}-{c[4]}-{'fp16' if c[5] == F16 else 'bf16'}"


def _x(T, K, dt, seed=0):
    return torch.randn(T, K, generator=torch.Generator().manual_seed(seed + K)).to(dt).to(DEV)


def _slices(T):
    """(rows to launch, rows of that launch to keep) per 16-row block: a one-row block takes two rows."""
    for s in range(0, T, 16):
        e = min(s + 16, T)
        yield (slice(s - 1, e), slice(1, 2), slice(s, e)) if e - s == 1 else (slice(s, e), slice(None), slice(s, e))


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_wide_against_fp64_and_the_16_row_kernel(c):
    from quantizations_amd.core import gemm_4bit, gemm_4bit_grouped, gemm_4bit_grouped_wide, gemm_4bit_wide

    K, M, bs, bs2, qt, dt = c
    case = sf._case("wide", M, K, bs, bs2)
    ws = [_weight(case, qt, dt, shift) for shift in (0, 2)]
    items = [(p, st, None) for p, st, _ in ws]
    X = _x(64, K, dt)
    for T in TS:
        x = X[:T]
        y = gemm_4bit_wide(x, ws[0][0], ws[0][1])
        ys = gemm_4bit_grouped_wide(x, items)
        assert y.shape == (T, M) and y.dtype == dt and torch.equal(ys[0], y)
        for yi, (_, _, Wd) in zip(ys, ws):
            _on_bar(yi, (x.double() @ Wd.double().t()).cpu().numpy(), dt, f"wide {_id(c)} T={T}")
        for run, keep, rows in _slices(T):
            assert torch.equal(y[rows], gemm_4bit(x[run], ws[0][0], ws[0][1], route="fused")[keep]), (T, rows)
            for yi, yo in zip(ys, gemm_4bit_grouped(x[run], items)):
                assert torch.equal(yi[rows], yo[keep]), (T, rows)


def test_a_row_does_not_depend_on_its_index_or_its_neighbours():
    from quantizations_amd.core import gemm_4bit_wide

    K, M = 2304, 20
    p, st, _ = _weight(sf._case("wide", M, K, 4096, 64), "nf4", F16)
    X, other = _x(64, K, F16), _x(17, K, F16, seed=5)
    y64 = gemm_4bit_wide(X, p, st)
    for r, at in ((0, 16), (15, 0), (16, 3), (47, 16), (63, 9)):
        x17 = other.clone()
        x17[at] = X[r]
        assert torch.equal(gemm_4bit_wide(x17, p, st)[at], y64[r]), (r, at)


def test_bias_row_stride_and_block_base():
    from quantizations_amd.core import gemm_4bit, gemm_4bit_wide
    from quantizations_amd.parallel import shard_rows

    K, M, T, dt = 2048, 20, 33, BF16
    p, st, Wd = _weight(sf._case("wide", M, K, 64, 256), "fp4", dt)
    bias = torch.randn(M, generator=torch.Generator().manual_seed(1)).to(dt).to(DEV)
    buf = torch.zeros(T, K + 64, dtype=dt, device=DEV)
    buf[:, :K] = _x(T, K, dt)
    x = buf[:, :K]                       # ldx = K + 64
    y = gemm_4bit_wide(x, p, st, bias=bias)
    _on_bar(y, (x.double() @ Wd.double().t() + bias.double()).cpu().numpy(), dt, "wide + bias, ldx > K")
    assert torch.equal(y[16:32], gemm_4bit(x[16:32].contiguous(), p, st, bias=bias, route="fused"))
    # a row shard whose scales start inside a second-level block
    c = sf.SHARDS[0]
    p, st, _ = _weight(c, "nf4", F16)
    x = _x(20, c.K, F16)
    full = gemm_4bit_wide(x, p, st)
    shards = [shard_rows(p, st, rank, 4) for rank in range(4)]
    assert any(sh.block_base != 0 for sh in shards)
    for sh in shards:
        assert torch.equal(gemm_4bit_wide(x, sh.packed, sh.state, block_base=sh.block_base), full[:, sh.r0:sh.r1])


def test_refusals():
    import ctypes

    from quantizations_amd import _lib, core

    K, M = 512, 16
    p, st, _ = _weight(sf._case("wide", M, K, 64, None), "nf4", F16)
    for T in (16, 65):
        x = _x(T, K, F16)
        with pytest.raises(ValueError, match="17..64"):
            core.gemm_4bit_wide(x, p, st)
        with pytest.raises(ValueError, match="17..64"):
            core.gemm_4bit_grouped_wide(x, [(p, st, None)])
        # the library itself refuses, whatever the binding lets through
        y = torch.full((T, M), 7, dtype=F16, device=DEV)
        segs, _, _ = core._pack_segments([(p, st, None)], F16, lambda _m: y, "test")
        args = (T, K, x.data_ptr(), K, _lib.DT_F16, _lib.QUANT_TYPES["nf4"], 64, 0, _lib.stream_of(x))
        assert _lib.lib.qz_gemm_4bit_grouped_wide(1, ctypes.cast(segs, ctypes.c_void_p), *args) == _lib.QZ_ERR_SHAPE
        assert _lib.lib.qz_gemm_4bit_mt_wide(T, M, K, x.data_ptr(), K, _lib.DT_F16, p.data_ptr(), _lib.QUANT_TYPES["nf4"],
                                             64, *st.scale_args(), 0, 0, y.data_ptr(), M,
                                             _lib.stream_of(x)) == _lib.QZ_ERR_SHAPE
        torch.cuda.synchronize()
        assert bool((y == 7).all())
    with pytest.raises(ValueError, match="2..16"):
        core.gemm_4bit_grouped(_x(20, K, F16), [(p, st, None)])


@pytest.fixture(scope="module")
def tiny():
    from quantizations_amd.generation import prepare_for_decode

    model = _build()
    prepare_for_decode(model)
    try:
        yield model
    finally:
        _unprepare(model)


def test_a_fused_group_takes_the_wide_launch_only_after_set_decode_rows(tiny, monkeypatch):
    import quantizations_amd as qa
    from test_gpu_product_geometry import _count_entry_points

    attn = tiny.model.layers[0].self_attn
    x = _x(20, 256, F16)

    def run():
        with monkeypatch.context() as mp, torch.no_grad():
            calls = _count_entry_points(mp)
            out = [proj(x) for proj in (attn.q_proj, attn.k_proj, attn.v_proj)]
            torch.cuda.synchronize()
            return out, dict(calls)

    before, calls = run()
    assert "qz_gemm_4bit_grouped_wide" not in calls and calls["qz_gemm_4bit"] == 3, calls
    assert qa.set_decode_rows(tiny, 64) > 0
    try:
        after, calls = run()
    finally:
        qa.set_decode_rows(tiny, 16)
    assert calls["qz_gemm_4bit_grouped_wide"] == 1 and "qz_gemm_4bit" not in calls, calls
    assert not any(k.startswith("refused:") for k in calls), calls
    assert all(a.shape == b.shape for a, b in zip(after, before))
    with torch.no_grad():               # rows 0..15 and 16..19 through the group's 16-row launch: the same bits
        for rows in (slice(0, 16), slice(16, 20)):
            xs = x[rows].contiguous()
            for a, proj in zip(after, (attn.q_proj, attn.k_proj, attn.v_proj)):
                assert torch.equal(a[rows], proj(xs)), rows
    assert "qz_gemm_4bit_grouped_wide" not in run()[1]


LENGTHS = [8, 3, 5, 6, 4]
N = 24


def _speculate(model, rows, **kw):
    """(sequences, accepted per step [steps, B]) of the streams `rows` of the five prompts."""
    from quantizations_amd.generation import SpeculativeSession

    ids = torch.randint(0, 4096, (5, 8), generator=torch.Generator().manual_seed(3)).to(DEV)[rows]
    lens = [LENGTHS[b] for b in rows]
    sess = SpeculativeSession(model, len(rows), 8 + N, draft_tokens=3, **kw)
    sess.prefill(ids, lens, max_new_tokens=N)
    acc = []
    for _ in range(N - 1):
        sess.step()
        acc.append(sess.accepted.clone())
    return sess.sequences(), torch.stack(acc)


def test_a_20_row_verify_step_emits_what_12_and_8_rows_emit(tiny):
    with pytest.raises(ValueError, match="rows per step"):
        _speculate(tiny, [0, 1, 2, 3, 4])
    try:
        seqs, acc = _speculate(tiny, [0, 1, 2, 3, 4], decode_rows=64)
        for rows in ([0, 1, 2], [3, 4]):
            s, a = _speculate(tiny, rows)
            assert torch.equal(a, acc[:, rows])
            for b, t in zip(rows, s):
                assert torch.equal(t, seqs[b]), b
    finally:
        import quantizations_amd as qa
        qa.set_decode_rows(tiny, 16)


def test_generate_with_seven_drafts_over_three_prompts(tiny):
    import quantizations_amd as qa

    ids = torch.randint(0, 4096, (3, 8), generator=torch.Generator().manual_seed(3)).to(DEV)
    want = qa.generate(tiny, ids, 40, prompt_lookup_num_tokens=3)       # 12 rows per step: the 16-row kernel
    with pytest.raises(ValueError, match="rows per step"):
        qa.generate(tiny, ids, 40, prompt_lookup_num_tokens=7)
    try:
        got = qa.generate(tiny, ids, 40, prompt_lookup_num_tokens=7, decode_rows=64)    # 24 rows per step
        rag = qa.generate_ragged(tiny, list(ids), 40, prompt_lookup_num_tokens=7, decode_rows=64)
    finally:
        qa.set_decode_rows(tiny, 16)
    assert got.shape == qa.generate(tiny, ids, 40).shape
    # a token is a function of its own row's bits in every launch of the step: exact, whatever the drafts
    assert torch.equal(got, want)
    assert all(torch.equal(r, w) for r, w in zip(rag, want))
