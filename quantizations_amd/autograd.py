"""Autograd through the 4-bit matmul: ``MatMul4Bit`` (bitsandbytes' name and argument order).

The weight is frozen, so the backward is one product per layer, the input gradient
``grad_A = grad_out . W`` (core.gemm_4bit_dgrad: the fused 4-bit dgrad GEMM, or dequantise + the
library GEMM), plus the bias gradient.  The forward calls exactly what ``modules.matmul_4bit``
calls without autograd, so its output bits are the no-grad forward's; only the packed weight and
its QuantState are kept for the backward -- no activation.

Out of scope: gradients of the 4-bit weight, double backward, torch.compile.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .core import gemm_4bit, gemm_4bit_dgrad, gemv_4bit


class MatMul4Bit(torch.autograd.Function):
    """A . W^T (+ bias) for a 4-bit W, differentiable in A and bias.  ``B`` is the packed weight
    (only its storage is used, as in matmul_4bit), ``out`` an optional output buffer for the
    one-token GEMV, ``exact_codes`` as in core.gemv_4bit."""

    @staticmethod
    def forward(ctx, A, B, out=None, bias=None, quant_state=None, exact_codes=None):
        assert quant_state is not None
        ctx.state = quant_state
        ctx.bias_dtype = None if bias is None else bias.dtype
        ctx.a_shape = A.shape
        ctx.save_for_backward(B)
        if out is not None:
            ctx.mark_dirty(out)
        if A.numel() == A.shape[-1]:
            return gemv_4bit(A, B, out, state=quant_state, bias=bias, exact_codes=exact_codes)
        return gemm_4bit(A, B, quant_state, bias=bias)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (B,) = ctx.saved_tensors
        grad_A = grad_bias = None
        if ctx.needs_input_grad[0]:
            grad_A = gemm_4bit_dgrad(grad_out, B, ctx.state).reshape(ctx.a_shape)
        if ctx.bias_dtype is not None and ctx.needs_input_grad[3]:
            grad_bias = grad_out.reshape(-1, grad_out.shape[-1]).sum(0, dtype=ctx.bias_dtype)
        return grad_A, None, None, grad_bias, None, None
