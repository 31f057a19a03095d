"""qz_moe_*: argument and shape checks answer before any HIP call (this runs without a GPU), and
SparseMoe4bit on CPU tensors raises what Linear4bit raises there."""
import ctypes

import pytest
import torch

from quantizations_amd import _lib
from quantizations_amd.moe import SparseMoe4bit

ARG, SHAPE = -1, -3
_buf = ctypes.create_string_buffer(4096 + 16)
P = (ctypes.addressof(_buf) + 15) & ~15   # a 16-B aligned host address: never dereferenced on these paths


def route(T=4, H=256, E=8, k=2, x=P, rw=P, idx=P, w=P):
    return _lib.lib.qz_moe_route(T, H, E, k, x, H, _lib.DT_F16, rw, idx, w, None, None)


def pair(T=4, H=256, I=256, E=8, k=2, x=P, B=P, absmax=P, qabsmax=None, idx=P, h=P):
    return _lib.lib.qz_moe_pair_silu_4bit(T, H, I, E, k, x, H, _lib.DT_F16, B, _lib.NF4, 64, absmax, qabsmax, None, None,
                                          None, 0, 0, idx, h, None)


def down(T=4, H=256, I=256, E=8, k=2, h=P, B=P, absmax=P, qabsmax=None, idx=P, w=P, y=P):
    return _lib.lib.qz_moe_down_4bit(T, H, I, E, k, h, _lib.DT_F16, B, _lib.NF4, 64, absmax, qabsmax, None, None, None,
                                     0, 0, idx, w, None, y, H, None)


@pytest.mark.parametrize("fn, kw, rc", [
    (route, dict(x=None), ARG), (route, dict(rw=None), ARG), (route, dict(idx=None), ARG), (route, dict(w=None), ARG),
    (route, dict(T=0), SHAPE), (route, dict(T=17), SHAPE), (route, dict(k=9, E=8), ARG), (route, dict(H=384), SHAPE),
    (route, dict(E=65), SHAPE),
    (pair, dict(x=None), ARG), (pair, dict(B=None), ARG), (pair, dict(idx=None), ARG), (pair, dict(h=None), ARG),
    (pair, dict(T=0), SHAPE), (pair, dict(T=17), SHAPE), (pair, dict(k=5, E=4), ARG), (pair, dict(H=320), SHAPE),
    (pair, dict(I=128), SHAPE), (pair, dict(qabsmax=P), ARG), (pair, dict(absmax=None), ARG),
    (down, dict(h=None), ARG), (down, dict(B=None), ARG), (down, dict(idx=None), ARG), (down, dict(w=None), ARG),
    (down, dict(y=None), ARG), (down, dict(T=0), SHAPE), (down, dict(T=17), SHAPE), (down, dict(k=5, E=4), ARG),
    (down, dict(H=264), SHAPE), (down, dict(I=520), SHAPE), (down, dict(qabsmax=P), ARG),
])
def test_prelaunch_status(fn, kw, rc):
    assert fn(**kw) == rc


def test_cpu_module_raises_like_linear4bit():
    g = torch.Generator().manual_seed(0)
    m = SparseMoe4bit(torch.randn(4, 256, generator=g), torch.randn(4, 512, 256, generator=g),
                      torch.randn(4, 256, 256, generator=g), top_k=2)
    assert m.gate_up_proj.quant_state is None and m.gate_up_proj.shape == (4 * 512, 256)
    with pytest.raises(RuntimeError, match="not quantised yet: move the module to a GPU first"):
        m(torch.randn(1, 3, 256))
    with pytest.raises(RuntimeError, match="inference-only"):
        m(torch.randn(1, 3, 256, requires_grad=True))
