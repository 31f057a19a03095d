"""CPU: the status qz_decode_attention_streams, qz_greedy_step_streams and qz_sample_step_streams
return BEFORE any HIP call, over tables of argument combinations they reject (negative status) or
have nothing to do for (QZ_OK), in the manner of test_sample_prelaunch_status.py.  Pointers are fake
16-byte-aligned non-null addresses: no row reaches a launch."""
import pytest

from quantizations_amd import _lib

OK, ARG, SHAPE, DTYPE = 0, -1, -3, -4
F16, BF16, F32 = _lib.DT_F16, _lib.DT_BF16, _lib.DT_F32
P = 4096   # a fake, 16-B-aligned, non-null pointer


def attn(dtype=F16, B=2, Hq=4, Hkv=2, D=64, L=256, q=P, q_row=None, k=P, k_row=None, v=P, v_row=None, cos=P, sin=P,
         cs_row=64, kc=P, vc=P, pos=P, out=P, out_row=None, work=P):
    return _lib.lib.qz_decode_attention_streams(
        dtype, B, Hq, Hkv, D, L, q, Hq * D if q_row is None else q_row, k, Hkv * D if k_row is None else k_row, v,
        Hkv * D if v_row is None else v_row, cos, sin, cs_row, kc, vc, pos, out, Hq * D if out_row is None else out_row,
        work, 0.125, 0)


ATTN_ROWS = [
    ("null_q", dict(q=0), ARG), ("null_k", dict(k=0), ARG), ("null_v", dict(v=0), ARG),
    ("null_cos", dict(cos=0), ARG), ("null_sin", dict(sin=0), ARG),
    ("null_k_cache", dict(kc=0), ARG), ("null_v_cache", dict(vc=0), ARG),
    ("null_pos", dict(pos=0), ARG), ("null_out", dict(out=0), ARG),
    ("null_work_two_chunks", dict(work=0), ARG),
    ("negative_B", dict(B=-1), ARG), ("negative_Hq", dict(Hq=-4), ARG), ("negative_L", dict(L=-1), ARG),
    ("negative_D", dict(D=-64), ARG), ("negative_cs_row", dict(cs_row=-1), ARG),
    ("q_row_below_width", dict(q_row=255), ARG), ("k_row_below_width", dict(k_row=127), ARG),
    ("v_row_below_width", dict(v_row=126), ARG), ("out_row_below_width", dict(out_row=255), ARG),
    ("v_row_odd", dict(v_row=129), ARG), ("v_misaligned", dict(v=P + 2), ARG),
    ("k_cache_misaligned", dict(kc=P + 8), ARG),
    ("D_96", dict(D=96), SHAPE), ("L_0", dict(L=0), SHAPE), ("Hkv_0", dict(Hkv=0), SHAPE),
    ("heads_not_a_multiple", dict(Hq=5), SHAPE), ("group_of_16", dict(Hq=16, Hkv=1), SHAPE),
    ("B_65536", dict(B=65536), SHAPE),
    ("dtype_fp32", dict(dtype=F32), DTYPE), ("dtype_7", dict(dtype=7), DTYPE),
    ("B_0", dict(B=0), OK), ("Hq_0", dict(Hq=0, Hkv=0), OK), ("B_0_null_everything", dict(B=0, q=0, pos=0, out=0), OK),
]


def greedy(logits=P, dtype=F16, B=2, V=1000, row=None, hist=P, hist_row=16, hist_len=16, pos=P, live=P, stop=P,
           limit=P, tok=P, work=P):
    return _lib.lib.qz_greedy_step_streams(logits, dtype, B, V, V if row is None else row, hist, hist_row, hist_len,
                                           pos, live, stop, limit, tok, work, 0)


GREEDY_ROWS = [
    ("null_logits", dict(logits=0), ARG), ("null_hist", dict(hist=0), ARG), ("null_pos", dict(pos=0), ARG),
    ("null_live", dict(live=0), ARG), ("null_stop", dict(stop=0), ARG), ("null_limit", dict(limit=0), ARG),
    ("null_tok", dict(tok=0), ARG), ("null_work", dict(work=0), ARG),
    ("negative_B", dict(B=-1), ARG), ("negative_V", dict(V=-5, row=8), ARG), ("negative_row", dict(row=-1), ARG),
    ("negative_hist_row", dict(hist_row=-1), ARG), ("negative_hist_len", dict(hist_len=-1), ARG),
    ("row_below_V", dict(row=999), ARG), ("hist_row_below_hist_len", dict(hist_row=8), ARG),
    ("V_0", dict(V=0), ARG),   # as qz_greedy_step: an empty row has no argmax
    ("dtype_7", dict(dtype=7), DTYPE),
    ("B_65536", dict(B=65536), SHAPE),
    ("B_0", dict(B=0), OK), ("B_0_null_everything", dict(B=0, logits=0, hist=0, live=0, work=0), OK),
]


def sample(logits=P, dtype=F16, B=2, V=1000, row=None, temperature=P, top_k=P, top_p=P, uniform=P, uniform_row=16,
           hist=P, hist_row=16, hist_len=16, pos=P, live=P, stop=P, limit=P, tok=P, work=P):
    return _lib.lib.qz_sample_step_streams(logits, dtype, B, V, V if row is None else row, temperature, top_k, top_p,
                                           uniform, uniform_row, hist, hist_row, hist_len, pos, live, stop, limit,
                                           tok, work, 0)


SAMPLE_ROWS = [
    ("null_logits", dict(logits=0), ARG), ("null_temperature", dict(temperature=0), ARG),
    ("null_top_k", dict(top_k=0), ARG), ("null_top_p", dict(top_p=0), ARG), ("null_uniform", dict(uniform=0), ARG),
    ("null_hist", dict(hist=0), ARG), ("null_pos", dict(pos=0), ARG), ("null_live", dict(live=0), ARG),
    ("null_stop", dict(stop=0), ARG), ("null_limit", dict(limit=0), ARG), ("null_tok", dict(tok=0), ARG),
    ("null_work", dict(work=0), ARG),
    ("negative_B", dict(B=-1), ARG), ("negative_V", dict(V=-5, row=8), ARG), ("negative_row", dict(row=-1), ARG),
    ("negative_uniform_row", dict(uniform_row=-1), ARG), ("negative_hist_row", dict(hist_row=-1), ARG),
    ("negative_hist_len", dict(hist_len=-1), ARG),
    ("row_below_V", dict(row=999), ARG), ("hist_row_below_hist_len", dict(hist_row=8), ARG),
    ("uniform_row_below_hist_len", dict(uniform_row=8), ARG), ("work_misaligned", dict(work=P + 8), ARG),
    ("dtype_fp32", dict(dtype=F32), DTYPE), ("dtype_7", dict(dtype=7), DTYPE),
    ("B_65536", dict(B=65536), SHAPE),
    ("B_0", dict(B=0), OK), ("V_0", dict(V=0), OK),
    ("B_0_null_everything", dict(B=0, logits=0, hist=0, live=0, work=0), OK), ("V_0_bf16", dict(V=0, dtype=BF16), OK),
]


@pytest.mark.parametrize("case, expected", [pytest.param(c, e, id=n) for n, c, e in ATTN_ROWS])
def test_attention_streams_prelaunch_status(case, expected):
    got = attn(**case)
    print(got)
    assert got == expected


@pytest.mark.parametrize("case, expected", [pytest.param(c, e, id=n) for n, c, e in GREEDY_ROWS])
def test_greedy_streams_prelaunch_status(case, expected):
    got = greedy(**case)
    print(got)
    assert got == expected


@pytest.mark.parametrize("case, expected", [pytest.param(c, e, id=n) for n, c, e in SAMPLE_ROWS])
def test_sample_streams_prelaunch_status(case, expected):
    got = sample(**case)
    print(got)
    assert got == expected
