"""qz_moe_route_rows / qz_moe_plan / qz_moe_gemm_*: argument and shape checks answer before any HIP call
(this runs without a GPU), in the manner of test_moe_host.py."""
import pytest

from quantizations_amd import _lib
from test_moe_host import ARG, SHAPE, P


def route_rows(T=40, H=256, E=8, k=2, x=P, rw=P, idx=P, w=P):
    return _lib.lib.qz_moe_route_rows(T, H, E, k, x, H, _lib.DT_F16, rw, idx, w, None, None)


def plan(T=40, E=8, k=2, idx=P, srt=P, offsets=P):
    return _lib.lib.qz_moe_plan(T, E, k, idx, srt, offsets, None)


def pair(T=40, H=256, I=256, E=8, k=2, x=P, B=P, absmax=P, qabsmax=None, srt=P, offsets=P, h=P):
    return _lib.lib.qz_moe_gemm_pair_silu_4bit(T, H, I, E, k, x, H, _lib.DT_F16, B, _lib.NF4, 64, absmax, qabsmax, None,
                                               None, None, 0, 0, srt, offsets, h, None)


def down(T=40, H=256, I=256, E=8, k=2, h=P, B=P, absmax=P, qabsmax=None, idx=P, w=P, srt=P, offsets=P, d=P, y=P):
    return _lib.lib.qz_moe_gemm_down_4bit(T, H, I, E, k, h, _lib.DT_F16, B, _lib.NF4, 64, absmax, qabsmax, None, None,
                                          None, 0, 0, idx, w, srt, offsets, d, None, y, H, None)


@pytest.mark.parametrize("fn, kw, rc", [
    (route_rows, dict(x=None), ARG), (route_rows, dict(rw=None), ARG), (route_rows, dict(idx=None), ARG),
    (route_rows, dict(w=None), ARG), (route_rows, dict(T=0), SHAPE), (route_rows, dict(T=65537), SHAPE),
    (route_rows, dict(k=9, E=8), ARG), (route_rows, dict(H=384), SHAPE), (route_rows, dict(E=65), SHAPE),
    (plan, dict(idx=None), ARG), (plan, dict(srt=None), ARG), (plan, dict(offsets=None), ARG), (plan, dict(T=0), SHAPE),
    (plan, dict(T=65536, k=4), SHAPE), (plan, dict(k=5, E=4), ARG), (plan, dict(E=65), SHAPE),
    (pair, dict(x=None), ARG), (pair, dict(B=None), ARG), (pair, dict(srt=None), ARG), (pair, dict(offsets=None), ARG),
    (pair, dict(h=None), ARG), (pair, dict(T=0), SHAPE), (pair, dict(T=65536, k=4), SHAPE), (pair, dict(k=5, E=4), ARG),
    (pair, dict(H=320), SHAPE), (pair, dict(I=128), SHAPE), (pair, dict(qabsmax=P), ARG), (pair, dict(absmax=None), ARG),
    (down, dict(h=None), ARG), (down, dict(B=None), ARG), (down, dict(idx=None), ARG), (down, dict(w=None), ARG),
    (down, dict(srt=None), ARG), (down, dict(offsets=None), ARG), (down, dict(d=None), ARG), (down, dict(y=None), ARG),
    (down, dict(T=0), SHAPE), (down, dict(T=65536, k=4), SHAPE), (down, dict(k=5, E=4), ARG), (down, dict(H=264), SHAPE),
    (down, dict(I=520), SHAPE), (down, dict(qabsmax=P), ARG),
])
def test_prelaunch_status(fn, kw, rc):
    assert fn(**kw) == rc
