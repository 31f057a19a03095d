"""CPU: the status every decode-GEMV entry point returns BEFORE any HIP call, over a table of
argument combinations it rejects (negative status), declines (QZ_ERR_SHAPE: the caller takes
another route) or has nothing to do for (QZ_OK).  Pointers are fake non-null addresses: no row
reaches a launch.

The plain and the adapter-carrying entry points share one launch path (csrc/gemv_launch.h); the
table pins what each returned when they were separate copies, and every row that has a plain and
an adapter twin also asserts that the two agree when the adapter operand is valid.  Not in the
table because it launches: K = 8192 with 10240 rows and a norm weight on qz_gemv_4bit_pair_silu
(the pair keeps whole rows per wave there, 640 workgroups, and takes the fused norm).
"""
import ctypes

import pytest

from quantizations_amd import _lib

OK, ARG, BLOCKSIZE, SHAPE, DTYPE = 0, -1, -2, -3, -4
F16, F32 = _lib.DT_F16, _lib.DT_F32
NF4 = _lib.QUANT_TYPES["nf4"]
P = 16   # a fake, 16-B-aligned, non-null pointer

SINGLE = ("gemv", "residual", "lora")
GROUPED = ("grouped", "grouped_lora")
NORMED = ("grouped_rmsnorm", "grouped_lora_norm")
ALL = SINGLE + GROUPED + NORMED + ("pair",)
# (plain, adapter) twins: the same arguments plus a valid adapter operand
TWINS = (("gemv", "lora"), ("residual", "lora"), ("grouped", "grouped_lora"), ("grouped_rmsnorm", "grouped_lora_norm"))


def call(entry, Ms=(8, 8), K=4096, x=P, dtype=F16, blocksize=64, scales=("am", "am"), nseg=None, segs_null=False,
         nw=P, r=8, t=P, t_offset=0):
    """One entry point on a case: segment i has Ms[i] rows and the scale source scales[i] ("am" =
    absmax, "dq" = double-quantised, "both", "none"); the single-GEMV entry points take segment 0.
    nw: the norm weight of the entry points that have one; r, t, t_offset: the adapter operand."""
    L = _lib.lib
    src = {"am": (P, 0, 0, 0, 0), "dq": (0, P, P, P, P), "both": (P, P, P, P, P), "none": (0, 0, 0, 0, 0)}
    if entry in SINGLE:
        head = (Ms[0], K, x, dtype, P, NF4, blocksize) + src[scales[0]] + (256, 0, 0, 0)
        if entry == "gemv":
            return L.qz_gemv_4bit(*head, P, 0)
        if entry == "residual":
            return L.qz_gemv_4bit_residual(*head, P, P, 0)
        return L.qz_gemv_4bit_lora(*head, 0, P, r, t, P, 0)
    segs = (_lib.GemvSegment * len(Ms))(*[_lib.GemvSegment(m, P, *src[s], 0, 0, P) for m, s in zip(Ms, scales)])
    segp = None if segs_null else ctypes.cast(segs, ctypes.c_void_p)
    n = len(Ms) if nseg is None else nseg
    tail = (K, x, dtype, NF4, blocksize, 256, 0)
    if entry == "pair":
        return L.qz_gemv_4bit_pair_silu(segp, *tail, nw, 1e-6, P, 0)
    if entry == "grouped":
        return L.qz_gemv_4bit_grouped(n, segp, *tail, 0)
    if entry == "grouped_rmsnorm":
        return L.qz_gemv_4bit_grouped_rmsnorm(n, segp, *tail, nw, 1e-6, 0)
    lsegs = (_lib.LoraSegment * len(Ms))(*[_lib.LoraSegment(P, r, t_offset) for _ in Ms])
    return L.qz_gemv_4bit_grouped_lora(n, segp, ctypes.cast(lsegs, ctypes.c_void_p), t, *tail,
                                       nw if entry == "grouped_lora_norm" else 0, 1e-6, 0)


def row(name, case, *expected):
    """expected: (entry points, status) pairs; an entry point that lacks the argument is left out"""
    return pytest.param(case, {e: st for es, st in expected for e in es}, id=name)


GROUPS = GROUPED + NORMED
ROWS = [
    # -- the plain entry points' rows (the adapter twins run them with a valid operand) --
    row("nseg_0", dict(nseg=0), (GROUPS, ARG)),
    row("nseg_5", dict(nseg=5), (GROUPS, ARG)),
    row("null_segs", dict(segs_null=True), (GROUPS + ("pair",), ARG)),
    row("dtype_7", dict(dtype=7), (SINGLE + GROUPS, DTYPE), (("pair",), SHAPE)),
    row("blocksize_48", dict(blocksize=48), (ALL, BLOCKSIZE)),
    row("both_scale_sources", dict(scales=("both", "both")), (ALL, ARG)),
    row("no_scale_source", dict(scales=("none", "none")), (ALL, ARG)),
    row("mixed_scale_formats", dict(scales=("am", "dq")), (GROUPS, ARG), (("pair",), SHAPE)),
    row("total_m_0", dict(Ms=(0, 0)), (GROUPS + ("pair",), OK)),
    row("M_0", dict(Ms=(0, 0)), (SINGLE, OK)),
    row("K_0_generic", dict(K=0), (ALL, SHAPE)),
    # -- with a norm weight --
    row("norm_K_not_multiple_of_8", dict(K=4100), (NORMED + ("pair",), SHAPE)),
    row("norm_K_16392", dict(K=16392), (NORMED + ("pair",), SHAPE)),
    row("norm_x_misaligned_by_8", dict(x=P + 8), (NORMED + ("pair",), SHAPE)),
    row("norm_K_1024_not_full_step", dict(K=1024), (NORMED + ("pair",), SHAPE)),
    row("norm_over_4096_workgroups", dict(Ms=(35000, 35000)), (NORMED + ("pair",), SHAPE)),
    row("norm_K_8192_split_limit", dict(K=8192, Ms=(5120, 5120)), (NORMED, SHAPE)),
    # -- the adapter operand --
    row("rank_0", dict(r=0), (("lora", "grouped_lora", "grouped_lora_norm"), ARG)),
    row("rank_65", dict(r=65), (("lora", "grouped_lora", "grouped_lora_norm"), ARG)),
    row("null_t", dict(t=0), (("lora", "grouped_lora", "grouped_lora_norm"), ARG)),
    row("negative_t_offset", dict(t_offset=-1), (("grouped_lora", "grouped_lora_norm"), ARG)),
    row("adapter_fp32", dict(dtype=F32), (("lora", "grouped_lora", "grouped_lora_norm"), DTYPE)),
    # -- the pair launch --
    row("pair_unequal_M", dict(Ms=(8, 16)), (("pair",), SHAPE)),
    row("pair_fp32", dict(dtype=F32), (("pair",), SHAPE)),
]


@pytest.mark.parametrize("case, expected", ROWS)
def test_prelaunch_status(case, expected):
    got = {e: call(e, **case) for e in expected}
    print(got)
    assert got == expected
    for plain, adapter in TWINS:
        if plain in got and adapter in got:
            assert got[plain] == got[adapter], (plain, adapter)


def test_every_entry_point_is_in_the_table():
    seen = set()
    for p in ROWS:
        seen |= set(p.values[1])
    assert seen == set(ALL)
