"""CPU: the status qz_token_logprobs and qz_logprobs_streams return BEFORE any HIP call, over a table
of argument combinations they reject (negative status) or have nothing to do for (QZ_OK), and
qz_logprobs_work_bytes, in the manner of test_logits_process_prelaunch_status.py.  Pointers are fake
16-byte-aligned non-null addresses: no row reaches a launch."""
import pytest

from quantizations_amd import _lib

OK, ARG, SHAPE, DTYPE = 0, -1, -3, -4
F16, BF16, F32 = _lib.DT_F16, _lib.DT_BF16, _lib.DT_F32
P = 4096   # a fake, 16-B-aligned, non-null pointer


def plain(logits=P, dtype=F16, R=3, V=1000, row=None, ids=P, ntop=5, lp=P, top_id=P, top_lp=P, work=P):
    return _lib.lib.qz_token_logprobs(logits, dtype, R, V, V if row is None else row, ids, ntop, lp, top_id, top_lp,
                                      work, 0)


def streams(logits=P, dtype=BF16, B=2, T=4, V=1000, row=None, seq=P, seq_row=16, seq_len=16, pos0=P, pos0_stride=1,
            pos1=P, pos1_stride=1, ntop=5, lp_tab=P, top_id_tab=P, top_lp_tab=P, tab_row=16, work=P):
    return _lib.lib.qz_logprobs_streams(logits, dtype, B, T, V, V if row is None else row, seq, seq_row, seq_len, pos0,
                                        pos0_stride, pos1, pos1_stride, ntop, lp_tab, top_id_tab, top_lp_tab, tab_row,
                                        work, 0)


PLAIN = [
    ("null_logits", dict(logits=0), ARG), ("null_ids", dict(ids=0), ARG), ("null_lp", dict(lp=0), ARG),
    ("null_work", dict(work=0), ARG), ("work_not_16B_aligned", dict(work=P + 8), ARG),
    ("null_top_id", dict(top_id=0), ARG), ("null_top_lp", dict(top_lp=0), ARG),
    ("negative_R", dict(R=-1), ARG), ("negative_V", dict(V=-5, row=8), ARG), ("negative_row", dict(row=-1), ARG),
    ("row_below_V", dict(row=999), ARG), ("ntop_minus_1", dict(ntop=-1), ARG),
    ("negative_R_with_V_0", dict(R=-1, V=0), ARG),
    ("dtype_fp32", dict(dtype=F32), DTYPE), ("dtype_7", dict(dtype=7), DTYPE),
    ("ntop_21", dict(ntop=21), SHAPE), ("rows_65536", dict(R=65536), SHAPE), ("V_2_pow_31", dict(V=1 << 31), SHAPE),
    ("R_0", dict(R=0), OK), ("V_0", dict(V=0), OK),
    ("R_0_null_everything", dict(R=0, logits=0, ids=0, lp=0, top_id=0, top_lp=0, work=0), OK),
    ("V_0_null_everything", dict(V=0, logits=0, ids=0, lp=0, top_id=0, top_lp=0, work=0), OK),
]

STREAMS = [
    ("null_logits", dict(logits=0), ARG), ("null_seq", dict(seq=0), ARG), ("null_pos0", dict(pos0=0), ARG),
    ("null_pos1", dict(pos1=0), ARG), ("null_lp_tab", dict(lp_tab=0), ARG), ("null_work", dict(work=0), ARG),
    ("null_top_id_tab", dict(top_id_tab=0), ARG), ("null_top_lp_tab", dict(top_lp_tab=0), ARG),
    ("negative_B", dict(B=-1), ARG), ("negative_T", dict(T=-1), ARG), ("negative_V", dict(V=-5, row=8), ARG),
    ("negative_row", dict(row=-1), ARG), ("negative_seq_row", dict(seq_row=-1), ARG),
    ("negative_seq_len", dict(seq_len=-1), ARG), ("negative_seq_len_with_B_0", dict(B=0, seq_len=-1), ARG),
    ("negative_tab_row", dict(tab_row=-1), ARG), ("ntop_minus_1", dict(ntop=-1), ARG),
    ("row_below_V", dict(row=999), ARG), ("seq_row_below_seq_len", dict(seq_row=15), ARG),
    ("tab_row_below_seq_len", dict(tab_row=15), ARG),
    ("pos0_stride_2", dict(pos0_stride=2), ARG), ("pos0_stride_negative", dict(pos0_stride=-1), ARG),
    ("pos1_stride_2", dict(pos1_stride=2), ARG), ("pos1_stride_negative", dict(pos1_stride=-1), ARG),
    ("dtype_fp32", dict(dtype=F32), DTYPE), ("dtype_7", dict(dtype=7), DTYPE),
    ("ntop_21", dict(ntop=21), SHAPE), ("T_17", dict(T=17), SHAPE), ("rows_65536", dict(B=4096, T=16), SHAPE),
    ("rows_overflow_int", dict(B=1 << 30, T=16), SHAPE), ("V_2_pow_31", dict(V=1 << 31), SHAPE),
    ("B_0", dict(B=0), OK), ("T_0", dict(T=0), OK), ("V_0", dict(V=0), OK),
    ("B_0_null_everything", dict(B=0, logits=0, seq=0, pos0=0, pos1=0, lp_tab=0, top_id_tab=0, top_lp_tab=0, work=0), OK),
    ("V_0_null_everything", dict(V=0, logits=0, seq=0, pos0=0, pos1=0, lp_tab=0, top_id_tab=0, top_lp_tab=0, work=0), OK),
]


@pytest.mark.parametrize("case, expected", [pytest.param(c, e, id=n) for n, c, e in PLAIN])
def test_token_logprobs_prelaunch_status(case, expected):
    got = plain(**case)
    print(got)
    assert got == expected


@pytest.mark.parametrize("case, expected", [pytest.param(c, e, id=n) for n, c, e in STREAMS])
def test_logprobs_streams_prelaunch_status(case, expected):
    got = streams(**case)
    print(got)
    assert got == expected


def test_ntop_0_needs_no_lists():
    """ntop = 0 with null lists passes every argument check: it is rejected for the next reason only."""
    assert plain(ntop=0, top_id=0, top_lp=0, dtype=F32) == DTYPE
    assert streams(ntop=0, top_id_tab=0, top_lp_tab=0, dtype=F32) == DTYPE


def test_work_bytes():
    wb = _lib.lib.qz_logprobs_work_bytes
    assert wb(0, 100, 5) == 0 and wb(1, 0, 5) == 0 and wb(-1, 100, 5) == 0
    assert wb(1, 100, -1) == 0 and wb(1, 100, 21) == 0 and wb(1, 1 << 31, 5) == 0
    # per row and chunk of 2048 logits: (m, sum) = 8 bytes and ntop candidates of 4; rows padded to 16 bytes
    assert wb(1, 1, 0) == 16 and wb(1, 2048, 0) == 16 and wb(1, 2049, 0) == 16 and wb(1, 4097, 0) == 32
    assert wb(3, 2049, 5) == 3 * 64 and wb(1, 128256, 20) == 63 * 88 + 8
    assert wb(16, 128256, 20) == 16 * (63 * 88 + 8) and wb(65535, 2048, 1) == 65535 * 16
