"""quantizations_amd -- MI355X (gfx950) native 4-bit Linear4bit.

Drop-in for the reference kkbwilldo/quantizations (``core``, ``modules``,
``kbkim_lib``): same classes/functions, backed by hand-written HIP kernels in
``libquantizations.so`` (C-ABI: include/quantizations.h).
"""
from ._lib import LIB_PATH, QuantizationsError  # noqa: F401  (loads the native library; fails loudly)
from .core import (  # noqa: F401
    Params4bit,
    QuantState,
    create_dynamic_map,
    dequantize_4bit,
    dequantize_blockwise,
    gemm_4bit,
    gemm_4bit_dgrad,
    gemv_4bit,
    get_4bit_type,
    get_ptr,
    quantize_4bit,
    quantize_blockwise,
)
from .autograd import MatMul4Bit  # noqa: F401
from .modules import Linear4bit, matmul_4bit  # noqa: F401
from .generation import (  # noqa: F401
    DecodeSession,
    GenerateOutput,
    SpeculativeSession,
    StreamSession,
    generate,
    generate_ragged,
    prepare_for_decode,
    score,
)
from . import constraints, kv_pages  # noqa: F401
from .constraints import TokenAutomaton  # noqa: F401
from .kv_pages import KVPagePool, KVPagesExhausted  # noqa: F401

__version__ = "0.1.0"
