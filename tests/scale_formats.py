"""Scale layouts of the 4-bit format beyond blocksize 64 -- helpers for tests/test_scale_formats.py
(CPU) and tests/test_gpu_scale_formats.py (GPU).  No GPU is touched here.

The layout has three parts: `blocksize`, the nested `blocksize2` of double quantisation, and where a
weight row starts relative to a scale block (a row starts mid-block whenever K % blocksize != 0; the
quantiser runs over the FLAT weight, so a block may straddle two rows).

* block-tagged weights: element e of the flat weight sits in block b = e // blocksize and holds an
  in-block pattern (both signs, every NF4 and FP4 code point) times 2 ** ((3 * b) % 7 - 3).
  Neighbouring blocks differ by a factor >= 8 and blocks d apart (d % 7 != 0) by >= 2, so a launch
  that reads another block's scale is off by at least a factor of two in every weight of that step.
* the case list (M, K, blocksize, blocksize2 | None).
* a numpy model of the scale index a kernel has to form: flat_block(), and the (row, step) pairs at
  which a wrong formula differs from it.
"""
from collections import namedtuple

import numpy as np

STEP = 64            # the K-step of the tile kernels: one scale block per (row, step) for blocksize >= 64
BASE = 2.0 ** -2     # base scale: the dequantised weights span [2^-5 * 0.0052, 2] -- normal in fp16, bf16, fp32

Case = namedtuple("Case", "name M K bs bs2 kind")


def _case(kind, M, K, bs, bs2=None):
    return Case(f"{kind}-{M}x{K}-b{bs}" + (f"-n{bs2}" if bs2 else ""), M, K, bs, bs2, kind)


# K % blocksize != 0, K % 64 == 0: blocks straddle rows
STRADDLING = [
    _case("straddle", 132, 192, 128),
    _case("straddle", 264, 320, 256, 64),
    _case("straddle", 136, 2112, 128, 256),
    _case("straddle", 128, 1088, 1024),
    _case("straddle", 64, 6144, 4096, 64),
    _case("straddle", 264, 768, 512, 256),
]
# K divides the blocksize: rows start mid-block but never cross a block boundary
K_DIVIDES = [
    _case("kdiv", 64, 1024, 4096, 64),
    _case("kdiv", 16, 2048, 4096),
]
# every row starts on a block boundary, blocksize != 64
ALIGNED = [_case("aligned", M, K, bs, bs2)
           for (M, K) in ((256, 4096), (64, 8192))
           for bs in (128, 512, 2048, 4096)
           for bs2 in (None, 256, 4096)]
CASES = STRADDLING + K_DIVIDES + ALIGNED
READBACK = STRADDLING + K_DIVIDES
# row shards (parallel.shard_rows at world 2 and 4)
SHARDS = [
    _case("shard", 512, 4096, 4096, 256),
    _case("shard", 512, 4096, 1024, 256),
    _case("shard", 256, 4096, 128, 256),
]
MAX_ELEMENTS = 2 * 1024 * 1024


def case_id(c):
    return c.name


def quant_type_of(c):
    """The quant type a case's product tests use (the readbacks run both)."""
    return "nf4" if (c.M // 8 + c.K // 64 + (c.bs2 or 0) // 64) % 2 == 0 else "fp4"


# ---------------------------------------------------------------------------
# block-tagged weights
# ---------------------------------------------------------------------------


def tag_exponent(b, shift=0):
    return (3 * (np.asarray(b, np.int64) + shift)) % 7 - 3


def _pattern(i, b):
    """In-block pattern at position i of block b, |.| <= 1 with +1 and -1 in every block: the 16 NF4
    and the 16 FP4 code points (rounded to fp16, so that every tagged weight is exact in fp16),
    visited in an order that differs from one 32-element group to the next.  The walk starts 11 b
    places in: with one start for every block, rows 7 apart would be equal (the tags repeat every 7
    blocks) and a product over such a weight would take 7 values."""
    import oracle

    vals = np.concatenate([oracle.codebook("nf4"), oracle.codebook("fp4")]).astype(np.float16).astype(np.float32)
    return vals[(7 * i + i // 32 + 11 * b) % 32]


def tagged_weight(M, K, bs, shift=0):
    """fp32 [M, K] (every value exact in fp16): pattern(e % bs, b) * BASE * 2 ** tag_exponent(b), b = e // bs."""
    assert M * K <= MAX_ELEMENTS
    e = np.arange(M * K, dtype=np.int64)
    w = _pattern(e % bs, e // bs) * np.exp2(tag_exponent(e // bs, shift)).astype(np.float32) * np.float32(BASE)
    assert np.array_equal(w.astype(np.float16).astype(np.float32), w)
    return w.reshape(M, K)


_states = {}


def oracle_state(c, qt, shift=0):
    """The oracle's quantisation of a case's tagged weight (cached; never modified)."""
    import oracle

    key = (c.M, c.K, c.bs, c.bs2, qt, shift)
    if key not in _states:
        _states[key] = oracle.quantize_4bit(tagged_weight(c.M, c.K, c.bs, shift), c.bs, qt,
                                            double_quant=c.bs2 is not None, blocksize2=c.bs2 or 256)
    return _states[key]


# ---------------------------------------------------------------------------
# numpy model of the scale index
# ---------------------------------------------------------------------------


def flat_block(r, K, k, bs):
    """The scale block of element (r, k): the quantiser's, over the flat weight."""
    return (np.asarray(r, np.int64) * K + np.asarray(k, np.int64)) // bs


def sum_of_floors(r, K, k, bs):
    """A wrong index: the row's first block plus the step's block counted from the ROW START."""
    return (np.asarray(r, np.int64) * K) // bs + np.asarray(k, np.int64) // bs


def wrong_pairs(M, K, bs, formula=sum_of_floors, step=STEP):
    """Boolean [M, K // step]: the (row, step) pairs at which `formula` differs from flat_block."""
    r = np.arange(M, dtype=np.int64)[:, None]
    k = (np.arange(K // step, dtype=np.int64) * step)[None, :]
    return formula(r, K, k, bs) != flat_block(r, K, k, bs)
