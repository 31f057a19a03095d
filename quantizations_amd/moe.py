"""``SparseMoe4bit`` -- a 4-bit ``MixtralSparseMoeBlock`` (transformers 5.x: a top-k router over E
expert MLPs whose weights are two stacked 3-D parameters, ``gate_up_proj [E, 2I, H]`` and
``down_proj [E, H, I]``).

Each stacked parameter is quantised FLAT, as bitsandbytes treats a 3-D parameter: one ``Params4bit``
over the 2-D view ``[E * rows, K]`` with one ``QuantState``; expert e is the row range
``[e * rows, (e + 1) * rows)`` of it.

Dispatch: up to 16 rows of fp16 / bf16 on the GPU run three launches -- route, gate/up/SiLU of the
hit experts, down projection with the weighted sum (csrc/moe.hip); more rows (prompts, prefill
chunks, scoring passes, wide batches) run route, a device-side plan that sorts the routing entries by
expert, and two expert-grouped tile GEMMs (csrc/moe_prefill.hip).  Both keep the expert choice in
device memory, so the block never synchronises and can be captured in a graph.  ``decode_route = "gemv"``
(opt-in) sends a one-row input's two expert launches to the byte-table GEMV form (csrc/moe_gemv.hip) where it
takes the shape.  Anything else (fp32,
shapes off the kernels' grid, ``prefill_route = "composed"``) runs the composed form with the same
semantics: the host loop over hit experts, each dequantised on its row range and applied with
``F.linear``.  Inference only: an input that requires grad raises.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .core import (MOE_MAX_ENTRIES, MOE_MAX_ROWS, MT_MAX_TOKENS, Params4bit, QuantState, dequantize_4bit, moe_down,
                   moe_gemm_down, moe_gemm_pair_silu, moe_gemv_down, moe_gemv_pair_silu, moe_pair_silu, moe_plan,
                   moe_route, moe_route_rows)
from .modules import grad_route


class _Router(nn.Module):
    """Holds the dense router weight [E, H] under the name the replaced block uses (``gate.weight``)."""

    def __init__(self, weight: torch.Tensor):
        super().__init__()
        self.weight = nn.Parameter(weight, requires_grad=False)


def _expert_weight(p: Params4bit, e: int, rows: int, dtype: torch.dtype) -> torch.Tensor:
    """Dense [rows, K] weight of expert e from the stacked flat-quantised p, the values
    dequantize_4bit gives for the whole tensor."""
    qs = p.quant_state
    K = qs.shape[1]
    n0, n1 = e * rows * K, (e + 1) * rows * K
    bs = qs.blocksize
    if n0 % bs or n1 % bs:   # the expert's rows do not start and end on a scale block
        return dequantize_4bit(p, qs, out_dtype=dtype).t()[e * rows:(e + 1) * rows]
    b0, b1 = n0 // bs, n1 // bs
    if qs.nested:   # the fp32 scale of each block as every kernel rebuilds it: two rounded fp32 ops
        b = torch.arange(b0, b1, device=qs.absmax.device)
        absmax = qs.state2.code[qs.absmax[b0:b1].long()] * qs.state2.absmax[b // qs.state2.blocksize] + qs.offset
    else:
        absmax = qs.absmax[b0:b1]
    part = QuantState(absmax=absmax.contiguous(), shape=torch.Size((rows, K)), code=qs.code, blocksize=bs,
                      quant_type=qs.quant_type, dtype=qs.dtype)
    return dequantize_4bit(p.data.reshape(-1)[n0 // 2:n1 // 2], part, out_dtype=dtype).t()


class SparseMoe4bit(nn.Module):
    """Built from the replaced block's tensors: ``gate_weight [E, H]``, ``gate_up_proj [E, 2I, H]``,
    ``down_proj [E, H, I]``.  The expert weights are quantised when they reach a GPU (at once if
    ``device`` or the tensors' device is one)."""

    def __init__(self, gate_weight: torch.Tensor, gate_up_proj: torch.Tensor, down_proj: torch.Tensor, top_k: int,
                 quant_type: str = "nf4", compress_statistics: bool = True, blocksize: int = 64, device=None):
        super().__init__()
        E, I2, H = gate_up_proj.shape
        if gate_weight.shape != (E, H) or down_proj.shape != (E, H, I2 // 2) or I2 % 2 or not 1 <= top_k <= E:
            raise ValueError("SparseMoe4bit: expected gate_weight [E, H], gate_up_proj [E, 2I, H], down_proj [E, H, I] "
                             "and 1 <= top_k <= E")
        self.num_experts, self.top_k, self.hidden_dim, self.intermediate_dim = E, int(top_k), H, I2 // 2
        dev = torch.device(device) if device is not None else gate_up_proj.device
        self.gate = _Router(gate_weight.detach().to(dev))

        def quantised(w3):
            p = Params4bit(w3.detach().reshape(-1, w3.shape[-1]), requires_grad=False, blocksize=blocksize,
                           quant_type=quant_type, compress_statistics=compress_statistics)
            return p.to(dev)
        self.gate_up_proj = quantised(gate_up_proj)
        self.down_proj = quantised(down_proj)

    _EXPERT_PARAMS = ("gate_up_proj", "down_proj")
    # inputs of more than 16 rows: "auto" = the grouped tile GEMMs where they take the shape,
    # "composed" = always the host loop (kept reachable for timing and comparison)
    prefill_route = "auto"
    # a one-row input: "mma" = the three launches every 1..16-row input takes (a row's bits do not depend
    # on the batch), "gemv" = the expert launches on the byte-table GEMV (csrc/moe_gemv.hip: the same
    # values to fp32 summation error, other bits) where they take the shape, else "mma"'s
    decode_route = "mma"

    def forward(self, hidden_states: torch.Tensor, _qz_residual=None) -> torch.Tensor:
        """`_qz_residual` (the residual-fused decoder layer): returns residual + block output, the add
        inside the down launch where that launch takes one."""
        if grad_route(hidden_states):
            raise RuntimeError("SparseMoe4bit is inference-only: the input requires grad")
        if self.gate_up_proj.quant_state is None or self.down_proj.quant_state is None:
            raise RuntimeError("SparseMoe4bit weights are not quantised yet: move the module to a GPU first")
        x = hidden_states.reshape(-1, self.hidden_dim)
        y = None
        if self.prefill_route not in ("auto", "composed"):
            raise ValueError(f"SparseMoe4bit.prefill_route must be 'auto' or 'composed', not {self.prefill_route!r}")
        if self.decode_route not in ("mma", "gemv"):
            raise ValueError(f"SparseMoe4bit.decode_route must be 'mma' or 'gemv', not {self.decode_route!r}")
        res = None
        if _qz_residual is not None:
            res = _qz_residual.reshape(x.shape)
            res = res if res.is_contiguous() and res.dtype == x.dtype else None
        added = res is not None
        if x.is_cuda and x.shape[0] >= 1 and x.dtype in (torch.float16, torch.bfloat16):
            if x.shape[0] <= MT_MAX_TOKENS:
                y = self._routed(x, res)
            elif self.prefill_route == "auto":
                y = self._grouped(x, res)
        if y is None:
            y, added = self._composed(x), False
        y = y.reshape(hidden_states.shape)
        return y if _qz_residual is None or added else _qz_residual + y

    def _routed(self, x, residual=None):
        """The three launches; None where one of them declines the shape."""
        E = self.num_experts
        r = moe_route(x, self.gate.weight, self.top_k)
        if r is None:
            return None
        idx, w = r
        if self.decode_route == "gemv" and x.shape[0] == 1:
            h = moe_gemv_pair_silu(x, self.gate_up_proj, self.gate_up_proj.quant_state, idx, E)
            y = None if h is None else moe_gemv_down(h, self.down_proj, self.down_proj.quant_state, idx, w, E,
                                                     residual)
            if y is not None:
                return y
        h = moe_pair_silu(x, self.gate_up_proj, self.gate_up_proj.quant_state, idx, E)
        if h is None:
            return None
        return moe_down(h, self.down_proj, self.down_proj.quant_state, idx, w, E, residual)

    def _grouped(self, x, residual=None):
        """More than 16 rows: route_rows, plan and the two grouped tile GEMMs, in row chunks of what one
        plan takes (a row has the same bits in any chunk); None where a launch declines the shape."""
        E = self.num_experts
        step = min(MOE_MAX_ROWS, MOE_MAX_ENTRIES // self.top_k)
        out = []
        for xc in x.split(step):
            r = moe_route_rows(xc, self.gate.weight, self.top_k)
            if r is None:
                return None
            idx, w = r
            plan = moe_plan(idx, E)
            if plan is None:
                return None
            h = moe_gemm_pair_silu(xc, self.gate_up_proj, self.gate_up_proj.quant_state, idx, plan, E)
            if h is None:
                return None
            y = moe_gemm_down(h, self.down_proj, self.down_proj.quant_state, idx, w, plan, E)
            if y is None:
                return None
            out.append(y)
        y = out[0] if len(out) == 1 else torch.cat(out)
        return y if residual is None else residual + y

    def _composed(self, x):
        """The same semantics from torch ops: MixtralTopKRouter, then the host loop over hit experts with
        the weighted outputs summed in fp32 in ascending expert order and rounded once."""
        I = self.intermediate_dim
        logits = F.linear(x, self.gate.weight.to(x.dtype))
        top_v, top_i = torch.topk(torch.softmax(logits.float(), dim=-1), self.top_k, dim=-1)
        top_v = top_v / top_v.sum(dim=-1, keepdim=True)
        y = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
        for e in torch.unique(top_i).tolist():
            t, s = torch.where(top_i == e)
            gate, up = F.linear(x[t], _expert_weight(self.gate_up_proj, e, 2 * I, x.dtype)).chunk(2, dim=-1)
            d = F.linear(F.silu(gate) * up, _expert_weight(self.down_proj, e, self.hidden_dim, x.dtype))
            y.index_add_(0, t, top_v[t, s, None] * d.float())
        return y.to(x.dtype)

    # -- checkpoints: the stacked weights under their own names with QuantState.as_dict(packed=True)
    # beside them, as Linear4bit saves its weight --
    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        for name in self._EXPERT_PARAMS:
            qs = getattr(self, name).quant_state
            if qs is None:
                continue   # not quantised yet: the plain float weight is saved
            for k, v in qs.as_dict(packed=True).items():
                destination[f"{prefix}{name}.{k}"] = v if keep_vars else v.detach()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        rest = dict(state_dict)
        loaded = []
        for name in self._EXPERT_PARAMS:
            wkey = prefix + name
            stats = {k[len(wkey) + 1:]: v for k, v in state_dict.items() if k.startswith(wkey + ".")}
            if not stats or wkey not in state_dict:
                continue   # float checkpoint: quantised on .to(cuda)
            old = getattr(self, name)
            dev = old.device if old.device.type != "meta" else state_dict[wkey].device
            setattr(self, name, Params4bit.from_prequantized(state_dict[wkey], stats, requires_grad=False, device=dev))
            for k in [wkey] + [f"{wkey}.{s}" for s in stats]:
                rest.pop(k)
            loaded.append(wkey)
        n_missing = len(missing_keys)
        super()._load_from_state_dict(rest, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        missing_keys[n_missing:] = [k for k in missing_keys[n_missing:] if k not in loaded]
