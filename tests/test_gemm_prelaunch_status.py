"""CPU: the status every GEMM entry point (csrc/gemm_4bit.hip, gemm_16bit.hip, gemm_mt.hip) returns
BEFORE any HIP call, over a table of argument combinations it rejects (negative status), declines
(QZ_ERR_SHAPE: the caller takes another route) or has nothing to do for (QZ_OK).  Pointers are fake
16-byte-aligned non-null addresses: no row reaches a launch.  The expected values are what the single
gemm.hip returned before it was split by route.

Entry points: "gemm4" = qz_gemm_4bit, "gemm16" = qz_gemm_16bit, "grouped" = qz_gemm_4bit_grouped,
"bank" = qz_gemm_4bit_grouped_lora.  A row lists only the entry points that have the argument.  The
order of the checks shows in two places: the grouped entry points decline T = 0 (it is outside
the 2..16-token range, checked first) where the others have nothing to do, and they look at the
bank operand only after every segment passed.

qz_gemm_16bit_ok and qz_gemm_4bit_workspace_size are pure functions and are pinned next to it.
"""
import ctypes

import pytest

from quantizations_amd import _lib

OK, ARG, BLOCKSIZE, SHAPE, DTYPE = 0, -1, -2, -3, -4
F16, BF16, F32 = _lib.DT_F16, _lib.DT_BF16, _lib.DT_F32
NF4 = _lib.QUANT_TYPES["nf4"]
P = 4096   # a fake, 16-B-aligned, non-null pointer

DENSE = ("gemm4", "gemm16")
GROUPS = ("grouped", "bank")
FOUR_BIT = ("gemm4",) + GROUPS
ALL = DENSE + GROUPS

SRC = {"am": (P, 0, 0, 0, 0), "dq": (0, P, P, P, P), "both": (P, P, P, P, P), "none": (0, 0, 0, 0, 0),
       "dq_no_tables": (0, P, 0, P, P)}


def call(entry, T=None, Ms=(8, 8), K=4096, x=P, ldx=None, b=P, y=P, dtype=F16, quant_type=NF4, blocksize=64,
         blocksize2=256, scales=("am", "am"), nseg=None, segs_null=False, ws=0, ws_bytes=0, lora_null=False,
         bank_b=P, n=2, r=8, t=P, t_offset=0, t_stride=16, tokens_per_slot=1):
    """One entry point on a case.  T defaults to 64 tokens for the dense entry points and 4 for the
    grouped ones; segment i has Ms[i] rows and the scale source scales[i] (the dense entry points take
    segment 0); b / y: every segment's weight / output pointer; the rest is the bank operand."""
    L = _lib.lib
    ldx = K if ldx is None else ldx
    if entry in DENSE:
        T = 64 if T is None else T
        M = Ms[0]
        if entry == "gemm16":
            return L.qz_gemm_16bit(T, M, K, x, ldx, dtype, b, 0, y, M, 0)
        am, q, am2, code2, off = SRC[scales[0]]
        return L.qz_gemm_4bit(T, M, K, x, ldx, dtype, b, quant_type, blocksize, am, q, am2, code2, off, blocksize2,
                              0, y, M, ws, ws_bytes, 0)
    T = 4 if T is None else T
    segs = (_lib.GemvSegment * len(Ms))(*[_lib.GemvSegment(m, b, *SRC[s], 0, 0, y) for m, s in zip(Ms, scales)])
    segp = None if segs_null else ctypes.cast(segs, ctypes.c_void_p)
    ns = len(Ms) if nseg is None else nseg
    tail = (T, K, x, ldx, dtype, quant_type, blocksize, blocksize2, 0)
    if entry == "grouped":
        return L.qz_gemm_4bit_grouped(ns, segp, *tail)
    lsegs = (_lib.LoraBankSegment * len(Ms))(*[_lib.LoraBankSegment(bank_b, n, r, t_offset) for _ in Ms])
    lp = None if lora_null else ctypes.cast(lsegs, ctypes.c_void_p)
    return L.qz_gemm_4bit_grouped_lora(ns, segp, lp, t, t_stride, 0, tokens_per_slot, *tail)


def row(name, case, *expected):
    """expected: (entry points, status) pairs; an entry point that lacks the argument is left out"""
    return pytest.param(case, {e: st for es, st in expected for e in es}, id=name)


ROWS = [
    # -- null operands, negative sizes --
    row("null_x", dict(x=0), (ALL, ARG)),
    row("null_weight", dict(b=0), (ALL, ARG)),
    row("null_y", dict(y=0), (ALL, ARG)),
    row("null_segs", dict(segs_null=True), (GROUPS, ARG)),
    row("negative_T", dict(T=-1), (ALL, ARG)),
    row("negative_M", dict(Ms=(-8, -8)), (ALL, ARG)),
    row("negative_K", dict(K=-64, ldx=64), (ALL, ARG)),
    # -- scale sources --
    row("both_scale_sources", dict(scales=("both", "both")), (FOUR_BIT, ARG)),
    row("no_scale_source", dict(scales=("none", "none")), (FOUR_BIT, ARG)),
    row("double_quant_without_tables", dict(scales=("dq_no_tables", "dq_no_tables")), (FOUR_BIT, ARG)),
    row("mixed_scale_formats", dict(scales=("am", "dq")), (GROUPS, ARG)),
    # -- quant type, dtype, block sizes --
    row("quant_type_7", dict(quant_type=7), (FOUR_BIT, DTYPE)),
    row("dtype_7", dict(dtype=7), (ALL, DTYPE)),
    row("dtype_fp32", dict(dtype=F32), (ALL, DTYPE)),
    row("blocksize_48", dict(blocksize=48), (FOUR_BIT, BLOCKSIZE)),
    row("blocksize_32", dict(blocksize=32), (FOUR_BIT, BLOCKSIZE)),
    row("blocksize2_100", dict(blocksize2=100, scales=("dq", "dq")), (FOUR_BIT, BLOCKSIZE)),
    # -- shapes the kernels decline --
    row("K_not_multiple_of_64", dict(K=4100, ldx=4104), (ALL, SHAPE)),
    row("ldx_below_K", dict(ldx=4088), (ALL, SHAPE)),
    row("x_misaligned", dict(x=P + 8), (ALL, SHAPE)),
    row("weight_misaligned", dict(b=P + 8), (ALL, SHAPE)),
    row("M_not_multiple_of_4", dict(Ms=(6, 6)), (ALL, SHAPE)),
    row("M_4_dense_16bit_needs_8", dict(Ms=(4, 4)), (("gemm16",), SHAPE)),
    row("grouped_T_1", dict(T=1), (GROUPS, SHAPE)),
    row("grouped_T_17", dict(T=17), (GROUPS, SHAPE)),
    row("grouped_T_0", dict(T=0), (GROUPS, SHAPE)),
    row("grouped_K_not_multiple_of_256", dict(K=4160), (GROUPS, SHAPE)),
    row("nseg_0", dict(nseg=0), (GROUPS, ARG)),
    row("nseg_5", dict(nseg=5), (GROUPS, ARG)),
    # -- nothing to do --
    row("T_0", dict(T=0), (DENSE, OK)),
    row("M_0", dict(Ms=(0, 0)), (ALL, OK)),
    # -- the split-K workspace --
    row("negative_workspace_bytes", dict(ws_bytes=-1), (("gemm4",), ARG)),
    row("workspace_bytes_without_workspace", dict(ws_bytes=1 << 20), (("gemm4",), ARG)),
    # -- the bank operand --
    row("null_lora", dict(lora_null=True), (("bank",), ARG)),
    row("rank_0", dict(r=0), (("bank",), ARG)),
    row("rank_65", dict(r=65, t_stride=128), (("bank",), ARG)),
    row("bank_n_0", dict(n=0), (("bank",), ARG)),
    row("bank_n_257", dict(n=257), (("bank",), ARG)),
    row("t_offset_plus_r_over_t_stride", dict(t_offset=9), (("bank",), ARG)),
    row("negative_t_offset", dict(t_offset=-1), (("bank",), ARG)),
    row("null_t", dict(t=0), (("bank",), ARG)),
    row("tokens_per_slot_0", dict(tokens_per_slot=0), (("bank",), ARG)),
    row("bank_b_misaligned", dict(bank_b=P + 8), (("bank",), SHAPE)),
]


@pytest.mark.parametrize("case, expected", ROWS)
def test_prelaunch_status(case, expected):
    got = {e: call(e, **case) for e in expected}
    print(got)
    assert got == expected


def test_every_entry_point_is_in_the_table():
    seen = set()
    for p in ROWS:
        seen |= set(p.values[1])
    assert seen == set(ALL)


def test_gemm_16bit_ok_is_a_pure_function_of_its_arguments():
    ok = _lib.lib.qz_gemm_16bit_ok

    def case(T=512, M=256, K=4096, x=P, ldx=None, w=P, y=P, ldy=None):
        return ok(T, M, K, x, K if ldx is None else ldx, w, y, M if ldy is None else ldy)

    assert case() == 1
    assert case(T=1, M=8, K=64) == 1
    assert case(ldx=4104, ldy=264) == 1
    for bad in (dict(T=0), dict(M=0), dict(K=0), dict(K=4100, ldx=4104), dict(M=252), dict(ldx=4088), dict(ldx=4100),
                dict(ldy=248), dict(ldy=260), dict(x=P + 8), dict(w=P + 8), dict(y=P + 8),
                dict(T=1 << 19, K=4096),            # T * ldx * 2 bytes reach 2^32: the kernels' 32-bit offsets
                dict(M=1 << 19, K=4096)):           # M * K * 2 bytes reach 2^32
        assert case(**bad) == 0, bad
    assert case(T=(1 << 19) - 1, K=4096) == 1


def test_gemm_4bit_workspace_size():
    size = _lib.lib.qz_gemm_4bit_workspace_size
    # bad shapes
    for T, M, K in ((0, 1024, 4096), (-1, 1024, 4096), (64, 0, 4096), (64, 1024, 0), (64, 1024, 4100)):
        assert size(T, M, K) == 0, (T, M, K)
    # the multi-token range reduces in LDS
    for T in (2, 4, 16):
        assert size(T, 1024, 4096) == 0, T
    # no split: the grid already has 512 workgroups, or K has fewer than 8 steps
    assert size(2048, 4096, 4096) == 0
    assert size(64, 1024, 256) == 0
    # split K: nsplit * T * M fp32 partials
    assert size(64, 1024, 4096) == 16 * 64 * 1024 * 4
    assert size(128, 4096, 4096) == 16 * 128 * 4096 * 4
    assert size(1, 4096, 4096) == 16 * 1 * 4096 * 4
    assert size(17, 1024, 4096) == 16 * 17 * 1024 * 4
    # 2..16 tokens outside the multi-token kernel's K % 256 == 0: 65 K-steps in 13 splits of 5
    assert size(4, 1024, 4160) == 13 * 4 * 1024 * 4
    # large T (>= 4096 tokens takes the 256 x 256 tile kernel, which uses no workspace): the size is
    # still the 128-row tile kernel's plan -- 0 once the grid is large, but not for few weight rows
    assert size(8192, 1024, 4096) == 0
    assert size(4096, 256, 4096) == 8 * 4096 * 256 * 4
