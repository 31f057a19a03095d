"""CPU: the status qz_verify_sample_step_streams returns BEFORE any HIP call, over a table of argument
combinations it rejects (negative status) or has nothing to do for (QZ_OK), in the manner of
test_verify_prelaunch_status.py.  Pointers are fake 16-byte-aligned non-null addresses: no row reaches
a launch."""
import pytest

from quantizations_amd import _lib

OK, ARG, SHAPE, DTYPE = 0, -1, -3, -4
F16, BF16, F32 = _lib.DT_F16, _lib.DT_BF16, _lib.DT_F32
P = 4096   # a fake, 16-B-aligned, non-null pointer


def pick(logits=P, dtype=F16, B=2, T=4, V=1000, row=None, temperature=P, top_k=P, top_p=P, uniform=P, uniform_row=16,
         hist=P, hist_row=16, hist_len=16, pos=P, live=P, stop=P, limit=P, tok=P, accepted=P, work=P):
    return _lib.lib.qz_verify_sample_step_streams(logits, dtype, B, T, V, V if row is None else row, temperature, top_k,
                                                  top_p, uniform, uniform_row, hist, hist_row, hist_len, pos, live,
                                                  stop, limit, tok, accepted, work, 0)


ROWS = [
    ("null_logits", dict(logits=0), ARG), ("null_temperature", dict(temperature=0), ARG),
    ("null_top_k", dict(top_k=0), ARG), ("null_top_p", dict(top_p=0), ARG), ("null_uniform", dict(uniform=0), ARG),
    ("null_hist", dict(hist=0), ARG), ("null_pos", dict(pos=0), ARG), ("null_live", dict(live=0), ARG),
    ("null_stop", dict(stop=0), ARG), ("null_limit", dict(limit=0), ARG), ("null_tok", dict(tok=0), ARG),
    ("null_accepted", dict(accepted=0), ARG), ("null_work", dict(work=0), ARG),
    ("negative_B", dict(B=-1), ARG), ("negative_T", dict(T=-1), ARG), ("negative_V", dict(V=-5, row=8), ARG),
    ("negative_row", dict(row=-1), ARG), ("negative_uniform_row", dict(uniform_row=-1), ARG),
    ("negative_hist_row", dict(hist_row=-1), ARG), ("negative_hist_len", dict(hist_len=-1), ARG),
    ("negative_hist_len_with_B_0", dict(B=0, hist_len=-1), ARG),
    ("row_below_V", dict(row=999), ARG), ("hist_row_below_hist_len", dict(hist_row=8), ARG),
    ("uniform_row_below_hist_len", dict(uniform_row=8), ARG),
    ("work_misaligned", dict(work=P + 8), ARG),
    ("T_17", dict(T=17), SHAPE), ("rows_65536", dict(B=4096, T=16), SHAPE),
    ("dtype_fp32", dict(dtype=F32), DTYPE), ("dtype_7", dict(dtype=7), DTYPE),
    ("B_0", dict(B=0), OK), ("T_0", dict(T=0), OK), ("V_0", dict(V=0), OK),
    ("B_0_null_everything", dict(B=0, logits=0, temperature=0, uniform=0, hist=0, live=0, accepted=0, work=0), OK),
    ("T_0_fp32", dict(T=0, dtype=F32), OK),
]


@pytest.mark.parametrize("case, expected", [pytest.param(c, e, id=n) for n, c, e in ROWS])
def test_verify_sample_step_prelaunch_status(case, expected):
    got = pick(**case)
    print(got)
    assert got == expected


def test_work_bytes():
    wb = _lib.lib.qz_verify_sample_step_work_bytes
    one = _lib.lib.qz_sample_step_work_bytes
    for V in (1, 1000, 2056, 128256):
        assert wb(1, 1, V) == one(1, V) and wb(3, 4, V) == one(12, V) == 12 * one(1, V)
    assert wb(0, 4, 1000) == wb(2, 0, 1000) == wb(2, 4, 0) == 0
