"""CPU: the host side of the backward -- the status qz_gemm_4bit_dgrad (csrc/gemm_dgrad.hip) returns
BEFORE any HIP call over fake 16-byte-aligned pointers (in the manner of
test_gemm_prelaunch_status.py: no row reaches a launch), its workspace size, the auto route's token
table, and that the autograd entry point imports without a GPU."""
import pytest

from quantizations_amd import _lib

OK, ARG, BLOCKSIZE, SHAPE, DTYPE = 0, -1, -2, -3, -4
F16, BF16, F32 = _lib.DT_F16, _lib.DT_BF16, _lib.DT_F32
NF4 = _lib.QUANT_TYPES["nf4"]
P = 4096   # a fake, 16-B-aligned, non-null pointer

SRC = {"am": (P, 0, 0, 0, 0), "dq": (0, P, P, P, P), "both": (P, P, P, P, P), "none": (0, 0, 0, 0, 0),
       "dq_no_tables": (0, P, 0, P, P)}


def call(T=64, M=1024, K=4096, g=P, ldg=None, dtype=F16, b=P, quant_type=NF4, blocksize=64, scales="am",
         blocksize2=256, dx=P, ldx=None, ws=0, ws_bytes=0):
    am, q, am2, code2, off = SRC[scales]
    return _lib.lib.qz_gemm_4bit_dgrad(T, M, K, g, M if ldg is None else ldg, dtype, b, quant_type, blocksize, am, q,
                                       am2, code2, off, blocksize2, dx, K if ldx is None else ldx, ws, ws_bytes, 0)


ROWS = [
    # -- null operands, negative sizes --
    ("null_dy", dict(g=0), ARG),
    ("null_weight", dict(b=0), ARG),
    ("null_dx", dict(dx=0), ARG),
    ("negative_T", dict(T=-1), ARG),
    ("negative_M", dict(M=-8, ldg=8), ARG),
    ("negative_K", dict(K=-64, ldx=64), ARG),
    # -- scale sources --
    ("both_scale_sources", dict(scales="both"), ARG),
    ("no_scale_source", dict(scales="none"), ARG),
    ("double_quant_without_tables", dict(scales="dq_no_tables"), ARG),
    # -- quant type, dtype, block sizes --
    ("quant_type_7", dict(quant_type=7), DTYPE),
    ("dtype_7", dict(dtype=7), DTYPE),
    ("dtype_fp32", dict(dtype=F32), DTYPE),
    ("blocksize_48", dict(blocksize=48), BLOCKSIZE),
    ("blocksize_32", dict(blocksize=32), BLOCKSIZE),
    ("blocksize2_100", dict(blocksize2=100, scales="dq"), BLOCKSIZE),
    # -- shapes the kernel declines --
    ("K_100", dict(K=100), SHAPE),
    ("K_not_multiple_of_64", dict(K=4128), SHAPE),
    ("M_not_multiple_of_8", dict(M=1004), SHAPE),
    ("ldg_below_M", dict(ldg=1016), SHAPE),
    ("ldg_not_multiple_of_8", dict(ldg=1028), SHAPE),
    ("ldx_below_K", dict(ldx=4032), SHAPE),
    ("dy_misaligned", dict(g=P + 8), SHAPE),
    ("weight_misaligned", dict(b=P + 8), SHAPE),
    # -- the split-M workspace --
    ("negative_workspace_bytes", dict(ws_bytes=-1), ARG),
    ("workspace_bytes_without_workspace", dict(ws_bytes=1 << 20), ARG),
    # -- nothing to do --
    ("T_0", dict(T=0), OK),
    ("K_0", dict(K=0), OK),
]


@pytest.mark.parametrize("case, expected", [pytest.param(c, e, id=n) for n, c, e in ROWS])
def test_dgrad_prelaunch_status(case, expected):
    assert call(**case) == expected


def test_dgrad_workspace_size():
    size = _lib.lib.qz_gemm_4bit_dgrad_workspace_size
    # shapes the kernel does not take
    for T, M, K in ((0, 1024, 4096), (-1, 1024, 4096), (64, 0, 4096), (64, 1024, 0), (64, 1024, 4100), (64, 1004, 4096)):
        assert size(T, M, K) == 0, (T, M, K)
    # no split: the grid already has 512 workgroups, or fewer than 8 steps of 64 weight rows
    assert size(2048, 4096, 4096) == 0        # 32 column tiles x 16 token tiles
    assert size(300, 264, 4096) == 0          # 5 steps
    assert size(64, 256, 4096) == 0           # 4 steps
    assert size(5, 64, 64) == 0
    # split M: nsplit * T * K fp32 partials
    assert size(64, 4096, 4096) == 16 * 64 * 4096 * 4
    assert size(1, 4096, 4096) == 16 * 1 * 4096 * 4
    assert size(130, 4096, 256) == 16 * 130 * 256 * 4
    assert size(64, 1024, 4096) == 4 * 64 * 4096 * 4       # 16 steps: 4 splits of 4
    assert size(65, 1032, 320) == 4 * 65 * 320 * 4         # 17 steps in splits of 5: 4 partials
    assert size(256, 14336, 4096) == 8 * 256 * 4096 * 4    # 64 tiles: 8 splits reach 512 workgroups


def test_dgrad_fused_max_tokens_follows_its_table(monkeypatch):
    from quantizations_amd import core

    monkeypatch.setattr(core, "DGRAD_FUSED_MAX_TOKENS", None)
    # the four Llama-3-8B shapes of profiles/dgrad_lowT_sweep.txt
    assert core.dgrad_fused_max_tokens(4096, 4096) == 512
    assert core.dgrad_fused_max_tokens(14336, 4096) == 512
    assert core.dgrad_fused_max_tokens(1024, 4096) == 128
    assert core.dgrad_fused_max_tokens(4096, 14336) == 128
    monkeypatch.setattr(core, "DGRAD_FUSED_MAX_TOKENS", 7)
    assert core.dgrad_fused_max_tokens(4096, 4096) == 7


def test_matmul4bit_is_importable_without_a_gpu():
    import torch

    import quantizations_amd as qa
    from quantizations_amd.autograd import MatMul4Bit

    assert qa.MatMul4Bit is MatMul4Bit and issubclass(MatMul4Bit, torch.autograd.Function)
    assert callable(qa.gemm_4bit_dgrad)


def test_grad_route_costs_nothing_without_autograd():
    """The test that picks the autograd route reads two flags: no grad mode or no requires_grad, no route."""
    import torch

    from quantizations_amd.modules import DecodeGroup, grad_route

    x = torch.zeros(1, 8)
    xg = torch.zeros(1, 8, requires_grad=True)
    assert not grad_route(x) and grad_route(xg) and grad_route(x, xg)
    assert DecodeGroup.accepts(x) and not DecodeGroup.accepts(xg)
    with torch.no_grad():
        assert not grad_route(xg) and DecodeGroup.accepts(xg)
    with torch.inference_mode():
        assert not grad_route(torch.zeros(1, 8)) and DecodeGroup.accepts(torch.zeros(1, 8))
