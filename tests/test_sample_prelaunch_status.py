"""CPU: the status qz_sample_step (csrc/sample.hip) returns BEFORE any HIP call, over a table of
argument combinations it rejects (negative status) or has nothing to do for (QZ_OK), in the manner
of test_gemm_prelaunch_status.py.  Pointers are fake 16-byte-aligned non-null addresses: no row
reaches a launch.  qz_sample_step_work_bytes is a pure function and is pinned next to it."""
import pytest

from quantizations_amd import _lib

OK, ARG, SHAPE, DTYPE = 0, -1, -3, -4
F16, BF16, F32 = _lib.DT_F16, _lib.DT_BF16, _lib.DT_F32
P = 4096   # a fake, 16-B-aligned, non-null pointer


def call(logits=P, dtype=F16, B=2, V=1000, row=None, temperature=P, top_k=P, top_p=P, uniform=P, uniform_row=16,
         hist=P, hist_row=16, hist_len=16, pos=P, tok=P, work=P):
    return _lib.lib.qz_sample_step(logits, dtype, B, V, V if row is None else row, temperature, top_k, top_p,
                                   uniform, uniform_row, hist, hist_row, hist_len, pos, tok, work, 0)


ROWS = [
    # -- null operands --
    ("null_logits", dict(logits=0), ARG),
    ("null_temperature", dict(temperature=0), ARG),
    ("null_top_k", dict(top_k=0), ARG),
    ("null_top_p", dict(top_p=0), ARG),
    ("null_uniform", dict(uniform=0), ARG),
    ("null_hist", dict(hist=0), ARG),
    ("null_pos", dict(pos=0), ARG),
    ("null_tok", dict(tok=0), ARG),
    ("null_work", dict(work=0), ARG),
    # -- negative sizes --
    ("negative_B", dict(B=-1), ARG),
    ("negative_V", dict(V=-5, row=8), ARG),
    ("negative_row", dict(row=-1), ARG),
    ("negative_uniform_row", dict(uniform_row=-1), ARG),
    ("negative_hist_row", dict(hist_row=-1), ARG),
    ("negative_hist_len", dict(hist_len=-1), ARG),
    # -- layouts --
    ("row_below_V", dict(row=999), ARG),
    ("hist_row_below_hist_len", dict(hist_row=8), ARG),
    ("uniform_row_below_hist_len", dict(uniform_row=8), ARG),
    ("work_misaligned", dict(work=P + 8), ARG),
    # -- dtype --
    ("dtype_fp32", dict(dtype=F32), DTYPE),
    ("dtype_7", dict(dtype=7), DTYPE),
    # -- sizes the launch declines --
    ("B_65536", dict(B=65536), SHAPE),
    # -- nothing to do (even with null pointers: nothing would be touched) --
    ("B_0", dict(B=0), OK),
    ("V_0", dict(V=0), OK),
    ("B_0_null_everything", dict(B=0, logits=0, hist=0, work=0), OK),
    ("V_0_bf16", dict(V=0, dtype=BF16), OK),
]


@pytest.mark.parametrize("case, expected", [pytest.param(c, e, id=n) for n, c, e in ROWS])
def test_prelaunch_status(case, expected):
    got = call(**case)
    print(got)
    assert got == expected


def test_sample_step_work_bytes_is_a_pure_function():
    size = _lib.lib.qz_sample_step_work_bytes
    for B, V in ((0, 1000), (-1, 1000), (4, 0), (4, -1)):
        assert size(B, V) == 0, (B, V)

    def per_stream(V):
        # 65536 count bins, a 64-byte header and, per 2048-logit chunk, a greedy partial (fp32 value
        # and int64 index) and the kept weight with the last kept index; rounded to 64 bytes
        nb = -(-V // 2048)
        return (65536 * 4 + 64 + nb * 20 + 63) // 64 * 64

    for V in (1, 1000, 2048, 2049, 2056, 32000, 128256, 1 << 31):
        assert size(1, V) == per_stream(V), V
        assert size(16, V) == 16 * per_stream(V), V
    assert size(1, 128256) == 263488          # 262144 + 64 + 63 * 20 = 263468, rounded up
    assert size(65535, 128256) == 65535 * size(1, 128256)   # no 32-bit overflow
