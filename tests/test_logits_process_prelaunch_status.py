"""CPU: the status qz_logits_process returns BEFORE any HIP call, over a table of argument
combinations it rejects (negative status) or has nothing to do for (QZ_OK), in the manner of
test_verify_prelaunch_status.py.  Pointers are fake 16-byte-aligned non-null addresses: no row
reaches a launch."""
import pytest

from quantizations_amd import _lib

OK, ARG, SHAPE, DTYPE = 0, -1, -3, -4
F16, BF16, F32 = _lib.DT_F16, _lib.DT_BF16, _lib.DT_F32
P = 4096   # a fake, 16-B-aligned, non-null pointer


def process(logits=P, dtype=F16, B=2, T=4, V=1000, row=None, hist=P, hist_row=16, hist_len=16, pos=P, pos_stride=1,
            tok=P, rp=P, pp=P, fp=P, ngram=P, min_new=P, prompt_len=P, eos=P, work=P):
    return _lib.lib.qz_logits_process(logits, dtype, B, T, V, V if row is None else row, hist, hist_row, hist_len, pos,
                                      pos_stride, tok, rp, pp, fp, ngram, min_new, prompt_len, eos, work, 0)


ROWS = [
    ("null_logits", dict(logits=0), ARG), ("null_hist", dict(hist=0), ARG), ("null_pos", dict(pos=0), ARG),
    ("null_tok_in_a_window", dict(tok=0), ARG), ("null_tok_T_2", dict(T=2, tok=0), ARG),
    ("negative_B", dict(B=-1), ARG), ("negative_T", dict(T=-1), ARG), ("negative_V", dict(V=-5, row=8), ARG),
    ("negative_row", dict(row=-1), ARG), ("negative_hist_row", dict(hist_row=-1), ARG),
    ("negative_hist_len", dict(hist_len=-1), ARG), ("negative_hist_len_with_B_0", dict(B=0, hist_len=-1), ARG),
    ("row_below_V", dict(row=999), ARG), ("hist_row_below_hist_len", dict(hist_row=8), ARG),
    ("hist_row_below_hist_len_B_1", dict(B=1, hist_row=15), ARG),
    ("pos_stride_2", dict(pos_stride=2), ARG), ("pos_stride_negative", dict(pos_stride=-1), ARG),
    ("null_work_with_the_table_in_work", dict(hist_len=20000, hist_row=20000, work=0), ARG),
    ("dtype_fp32", dict(dtype=F32), DTYPE), ("dtype_7", dict(dtype=7), DTYPE),
    ("T_17", dict(T=17), SHAPE), ("rows_65536", dict(B=4096, T=16), SHAPE),
    ("rows_overflow_int", dict(B=1 << 30, T=16), SHAPE), ("V_2_pow_31", dict(V=1 << 31), SHAPE),
    ("hist_len_2_pow_31", dict(hist_len=1 << 31, hist_row=1 << 31), SHAPE),
    ("B_0", dict(B=0), OK), ("T_0", dict(T=0), OK), ("V_0", dict(V=0), OK),
    ("B_0_null_everything", dict(B=0, logits=0, hist=0, pos=0, tok=0, work=0), OK),
    ("V_0_null_everything", dict(V=0, logits=0, hist=0, pos=0, tok=0), OK),
]


@pytest.mark.parametrize("case, expected", [pytest.param(c, e, id=n) for n, c, e in ROWS])
def test_logits_process_prelaunch_status(case, expected):
    got = process(**case)
    print(got)
    assert got == expected


def test_work_bytes():
    wb = _lib.lib.qz_logits_process_work_bytes
    assert wb(0, 1, 100) == 0 and wb(1, 0, 100) == 0 and wb(1, 1, -1) == 0
    # the table has at least 2 (hist_len + T) slots of 8 bytes; up to 16384 slots it lives in LDS
    assert wb(3, 4, 4093) == 0 and wb(3, 4, 8188) == 0
    assert wb(3, 4, 8189) == 3 * 4 * 32768 * 8
    assert wb(1, 1, 20000) == 65536 * 8
