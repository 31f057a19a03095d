"""CPU: the cases of tests/scale_formats.py can see what tests/test_gpu_scale_formats.py looks for.

Shown on the oracle and a numpy model of the scale index alone: the block tags survive the
quantiser (and double quantisation at every blocksize2 in use), the straddling cases separate the
flat scale index from the sum-of-floors one, the other cases do not, and shard_rows refuses a shard
that would start inside a scale block.
"""
import numpy as np
import pytest
import torch

import scale_formats as sf

ALL = sf.CASES + sf.SHARDS


def _ratio(a, b):
    return np.maximum(a / b, b / a)


@pytest.mark.parametrize("qt", ["nf4", "fp4"])
@pytest.mark.parametrize("c", ALL, ids=sf.case_id)
def test_tags_survive_quantisation(orc, c, qt):
    """The decoded scales of blocks b and b + 1, and of the blocks that hold (r, k) and (r + 1, k),
    differ by a factor >= 1.5 -- with plain scales and after the 8-bit double quantisation; every
    block holds every code and both signs."""
    assert c.M * c.K <= sf.MAX_ELEMENTS and c.K % sf.STEP == 0 and c.bs >= 64
    o = sf.oracle_state(c, qt)
    assert o.double_quant == (c.bs2 is not None) and (not o.double_quant or o.blocksize2 == c.bs2)
    am = o.absmax()
    assert am.size == c.M * c.K // c.bs and (am > 0).all()
    assert _ratio(am[1:], am[:-1]).min() >= 1.5
    r = np.arange(c.M - 1)[:, None]
    k = (np.arange(c.K // sf.STEP) * sf.STEP)[None, :]
    b0, b1 = sf.flat_block(r, c.K, k, c.bs), sf.flat_block(r + 1, c.K, k, c.bs)
    apart = b0 != b1
    assert apart.any() and _ratio(am[b1], am[b0])[apart].min() >= 1.5
    # the weights stay normal in fp16 and bf16 (fp32 a fortiori), zero codes aside
    wd = np.abs(orc.dequantize(o))
    assert wd.max() < 4 and wd[wd > 0].min() >= 2.0 ** -14
    first = o.packed[:c.bs // 2]
    codes = np.unique(np.concatenate([first >> 4, first & 15]))
    assert codes.size >= (16 if qt == "nf4" else 15)       # the FP4 quantiser never emits -0 (code 8)
    W = sf.tagged_weight(c.M, c.K, c.bs)
    assert (W[0, :c.bs if c.bs <= c.K else c.K] > 0).any() and (W[0, :c.bs if c.bs <= c.K else c.K] < 0).any()


@pytest.mark.parametrize("c", sf.STRADDLING, ids=sf.case_id)
def test_straddling_cases_separate_the_indices(c):
    assert c.K % c.bs != 0 and c.K % sf.STEP == 0
    wrong = sf.wrong_pairs(c.M, c.K, c.bs)
    assert wrong.mean() >= 0.10, wrong.mean()
    # where the indices differ, the tags do: the wrong block is a neighbour (one block back)
    r, s = np.nonzero(wrong)
    d = sf.flat_block(r, c.K, s * sf.STEP, c.bs) - sf.sum_of_floors(r, c.K, s * sf.STEP, c.bs)
    assert (d == 1).all()


@pytest.mark.parametrize("c", sf.K_DIVIDES + sf.ALIGNED + sf.SHARDS, ids=sf.case_id)
def test_other_cases_do_not(c):
    assert (c.K % c.bs == 0) or (c.bs % c.K == 0)
    assert not sf.wrong_pairs(c.M, c.K, c.bs).any()
    if c.kind == "kdiv":        # rows start mid-block
        assert ((np.arange(c.M) * c.K) % c.bs != 0).any()


def test_example_of_the_wrong_index():
    """K = 192, blocksize 128, row 1, k0 = 64: element 256 sits in block 2; the sum of floors says 1."""
    assert sf.flat_block(1, 192, 64, 128) == 2 and sf.sum_of_floors(1, 192, 64, 128) == 1
    assert int(sf.wrong_pairs(8, 192, 128).sum()) == 4          # 4 of 24
    assert int(sf.wrong_pairs(8, 2112, 128).sum()) == 64        # 64 of 264
    assert not sf.wrong_pairs(64, 4096, 4096).any() and not sf.wrong_pairs(64, 2112, 64).any()


def _cpu_state(o):
    """(packed, QuantState) on the CPU from an OracleState (shard_rows is device agnostic)."""
    from quantizations_amd.core import QuantState

    packed = torch.from_numpy(o.packed).reshape(-1, 1)
    code = torch.from_numpy(o.code)
    if not o.double_quant:
        return packed, QuantState(absmax=torch.from_numpy(o.absmax_raw), shape=torch.Size(o.shape),
                                  dtype=torch.float16, blocksize=o.blocksize, code=code, quant_type=o.quant_type)
    st2 = QuantState(absmax=torch.from_numpy(o.absmax2), code=torch.from_numpy(o.code2), blocksize=o.blocksize2,
                     dtype=torch.float32)
    return packed, QuantState(absmax=torch.from_numpy(o.qabsmax), shape=torch.Size(o.shape), dtype=torch.float16,
                              blocksize=o.blocksize, code=code, quant_type=o.quant_type,
                              offset=torch.tensor(float(o.offset), dtype=torch.float32), state2=st2)


def test_shard_rows_refuses_a_shard_that_starts_mid_block(orc):
    from quantizations_amd.parallel import shard_rows

    refused = taken = 0
    for c in sf.READBACK:
        packed, st = _cpu_state(sf.oracle_state(c, "nf4"))
        for world in (2, 4, 8):
            if c.M % world:
                continue
            for rank in range(world):
                mid = (rank * (c.M // world) * c.K) % c.bs != 0
                if mid:
                    with pytest.raises(ValueError, match="scale-block boundary"):
                        shard_rows(packed, st, rank, world)
                    refused += 1
                else:
                    sh = shard_rows(packed, st, rank, world)
                    assert (sh.r0 * c.K) % c.bs == 0
                    taken += 1
    assert refused >= 10 and taken >= 10, (refused, taken)


def test_shard_cases_start_inside_a_second_level_block(orc):
    """The shard cases are block-aligned at world 2 and 4, and some rank's scales start inside a
    second-level block (block_base != 0); the sliced statistics decode to the full layer's."""
    from quantizations_amd.parallel import shard_rows

    bases = []
    for c in sf.SHARDS:
        o = sf.oracle_state(c, "nf4")
        packed, st = _cpu_state(o)
        am = o.absmax()
        for world in (2, 4):
            for rank in range(world):
                sh = shard_rows(packed, st, rank, world)
                bases.append(sh.block_base)
                nb = (sh.r1 - sh.r0) * c.K // c.bs
                q = sh.state.absmax[sh.block_base:sh.block_base + nb].numpy()
                b0 = sh.r0 * c.K // c.bs
                assert np.array_equal(q, o.qabsmax[b0:b0 + nb])
                a2 = sh.state.state2.absmax.numpy()[(sh.block_base + np.arange(nb)) // c.bs2]
                assert np.array_equal(a2, o.absmax2[(b0 + np.arange(nb)) // c.bs2])
                assert am[b0:b0 + nb].size == nb
    assert any(b != 0 for b in bases), bases
