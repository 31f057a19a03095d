"""CPU: the status qz_decode_attention_verify, qz_verify_step_streams and qz_ngram_draft return BEFORE
any HIP call, over tables of argument combinations they reject (negative status) or have nothing to
do for (QZ_OK), in the manner of test_streams_prelaunch_status.py.  Pointers are fake 16-byte-aligned
non-null addresses: no row reaches a launch."""
import pytest

from quantizations_amd import _lib

OK, ARG, SHAPE, DTYPE = 0, -1, -3, -4
F16, BF16, F32 = _lib.DT_F16, _lib.DT_BF16, _lib.DT_F32
P = 4096   # a fake, 16-B-aligned, non-null pointer


def attn(dtype=F16, B=2, T=4, Hq=4, Hkv=2, D=64, L=256, q=P, q_row=None, k=P, k_row=None, v=P, v_row=None, cos=P,
         sin=P, cs_row=64, kc=P, vc=P, pos=P, out=P, out_row=None, work=P):
    return _lib.lib.qz_decode_attention_verify(
        dtype, B, T, Hq, Hkv, D, L, q, Hq * D if q_row is None else q_row, k, Hkv * D if k_row is None else k_row, v,
        Hkv * D if v_row is None else v_row, cos, sin, cs_row, kc, vc, pos, out, Hq * D if out_row is None else out_row,
        work, 0.125, 0)


ATTN_ROWS = [
    ("null_q", dict(q=0), ARG), ("null_k", dict(k=0), ARG), ("null_v", dict(v=0), ARG),
    ("null_cos", dict(cos=0), ARG), ("null_sin", dict(sin=0), ARG),
    ("null_k_cache", dict(kc=0), ARG), ("null_v_cache", dict(vc=0), ARG),
    ("null_pos", dict(pos=0), ARG), ("null_out", dict(out=0), ARG),
    ("null_work_two_chunks", dict(work=0), ARG),
    ("negative_B", dict(B=-1), ARG), ("negative_T", dict(T=-1), ARG), ("negative_Hq", dict(Hq=-4), ARG),
    ("negative_L", dict(L=-1), ARG), ("negative_D", dict(D=-64), ARG), ("negative_cs_row", dict(cs_row=-1), ARG),
    ("negative_L_with_B_0", dict(B=0, L=-1), ARG),
    ("q_row_below_width", dict(q_row=255), ARG), ("k_row_below_width", dict(k_row=127), ARG),
    ("v_row_below_width", dict(v_row=126), ARG), ("out_row_below_width", dict(out_row=255), ARG),
    ("v_row_odd", dict(v_row=129), ARG), ("v_misaligned", dict(v=P + 2), ARG),
    ("k_cache_misaligned", dict(kc=P + 8), ARG),
    ("D_96", dict(D=96), SHAPE), ("L_0", dict(L=0), SHAPE), ("Hkv_0", dict(Hkv=0), SHAPE),
    ("heads_not_a_multiple", dict(Hq=5), SHAPE), ("group_of_16", dict(Hq=16, Hkv=1), SHAPE),
    ("rows_65536", dict(B=16384, T=4), SHAPE), ("rows_overflow_int", dict(B=65536, T=65536), SHAPE),
    ("dtype_fp32", dict(dtype=F32), DTYPE), ("dtype_7", dict(dtype=7), DTYPE),
    ("B_0", dict(B=0), OK), ("T_0", dict(T=0), OK), ("Hq_0", dict(Hq=0, Hkv=0), OK),
    ("B_0_null_everything", dict(B=0, q=0, pos=0, out=0), OK),
]


def pick(logits=P, dtype=F16, B=2, T=4, V=1000, row=None, hist=P, hist_row=16, hist_len=16, pos=P, live=P, stop=P,
         limit=P, tok=P, accepted=P, work=P):
    return _lib.lib.qz_verify_step_streams(logits, dtype, B, T, V, V if row is None else row, hist, hist_row, hist_len,
                                           pos, live, stop, limit, tok, accepted, work, 0)


PICK_ROWS = [
    ("null_logits", dict(logits=0), ARG), ("null_hist", dict(hist=0), ARG), ("null_pos", dict(pos=0), ARG),
    ("null_live", dict(live=0), ARG), ("null_stop", dict(stop=0), ARG), ("null_limit", dict(limit=0), ARG),
    ("null_tok", dict(tok=0), ARG), ("null_accepted", dict(accepted=0), ARG), ("null_work", dict(work=0), ARG),
    ("negative_B", dict(B=-1), ARG), ("negative_T", dict(T=-1), ARG), ("negative_V", dict(V=-5, row=8), ARG),
    ("negative_row", dict(row=-1), ARG), ("negative_hist_row", dict(hist_row=-1), ARG),
    ("negative_hist_len", dict(hist_len=-1), ARG),
    ("row_below_V", dict(row=999), ARG), ("hist_row_below_hist_len", dict(hist_row=8), ARG),
    ("V_0", dict(V=0), ARG),   # as qz_greedy_step_streams: an empty row has no argmax
    ("dtype_7", dict(dtype=7), DTYPE),
    ("T_17", dict(T=17), SHAPE), ("rows_65536", dict(B=4096, T=16), SHAPE),
    ("B_0", dict(B=0), OK), ("T_0", dict(T=0), OK),
    ("B_0_null_everything", dict(B=0, logits=0, hist=0, live=0, accepted=0, work=0), OK),
]


def draft(B=2, T=4, ngram_max=3, hist=P, hist_row=16, hist_len=16, pos=P, tok=P, pos_ids=P):
    return _lib.lib.qz_ngram_draft(B, T, ngram_max, hist, hist_row, hist_len, pos, tok, pos_ids, 0)


DRAFT_ROWS = [
    ("null_hist", dict(hist=0), ARG), ("null_pos", dict(pos=0), ARG), ("null_tok", dict(tok=0), ARG),
    ("null_pos_ids", dict(pos_ids=0), ARG),
    ("negative_B", dict(B=-1), ARG), ("negative_T", dict(T=-1), ARG), ("negative_hist_row", dict(hist_row=-1), ARG),
    ("negative_hist_len", dict(hist_len=-1), ARG), ("hist_row_below_hist_len", dict(hist_row=8), ARG),
    ("ngram_0", dict(ngram_max=0), ARG), ("ngram_5", dict(ngram_max=5), ARG), ("ngram_negative", dict(ngram_max=-1), ARG),
    ("T_17", dict(T=17), SHAPE), ("B_65536", dict(B=65536), SHAPE),
    ("hist_len_2_pow_31", dict(hist_len=1 << 31, hist_row=1 << 31), SHAPE),
    ("B_0", dict(B=0), OK), ("T_0", dict(T=0), OK), ("B_0_null_everything", dict(B=0, hist=0, pos=0, tok=0), OK),
]


@pytest.mark.parametrize("case, expected", [pytest.param(c, e, id=n) for n, c, e in ATTN_ROWS])
def test_attention_verify_prelaunch_status(case, expected):
    got = attn(**case)
    print(got)
    assert got == expected


@pytest.mark.parametrize("case, expected", [pytest.param(c, e, id=n) for n, c, e in PICK_ROWS])
def test_verify_step_prelaunch_status(case, expected):
    got = pick(**case)
    print(got)
    assert got == expected


@pytest.mark.parametrize("case, expected", [pytest.param(c, e, id=n) for n, c, e in DRAFT_ROWS])
def test_ngram_draft_prelaunch_status(case, expected):
    got = draft(**case)
    print(got)
    assert got == expected
