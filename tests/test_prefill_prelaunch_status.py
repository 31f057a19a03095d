"""CPU: the status qz_prefill_attention returns BEFORE any HIP call, over a table of argument
combinations it rejects (negative status) or has nothing to do for (QZ_OK), in the manner of
test_verify_prelaunch_status.py.  Pointers are fake 16-byte-aligned non-null addresses: no row reaches a
launch."""
import pytest

from quantizations_amd import _lib

OK, ARG, SHAPE, DTYPE = 0, -1, -3, -4
F16, BF16, F32 = _lib.DT_F16, _lib.DT_BF16, _lib.DT_F32
P = 4096   # a fake, 16-B-aligned, non-null pointer


def attn(dtype=F16, B=2, T=4, Hq=4, Hkv=2, D=64, L=256, q=P, q_row=None, k=P, k_row=None, v=P, v_row=None, cos=P,
         sin=P, cs_row=64, kc=P, vc=P, pos=P, ln=P, out=P, out_row=None):
    return _lib.lib.qz_prefill_attention(
        dtype, B, T, Hq, Hkv, D, L, q, Hq * D if q_row is None else q_row, k, Hkv * D if k_row is None else k_row, v,
        Hkv * D if v_row is None else v_row, cos, sin, cs_row, kc, vc, pos, ln, out,
        Hq * D if out_row is None else out_row, 0.125, 0)


ROWS = [
    ("null_q", dict(q=0), ARG), ("null_k", dict(k=0), ARG), ("null_v", dict(v=0), ARG),
    ("null_cos", dict(cos=0), ARG), ("null_sin", dict(sin=0), ARG),
    ("null_k_cache", dict(kc=0), ARG), ("null_v_cache", dict(vc=0), ARG),
    ("null_pos", dict(pos=0), ARG), ("null_len", dict(ln=0), ARG), ("null_out", dict(out=0), ARG),
    ("negative_B", dict(B=-1), ARG), ("negative_T", dict(T=-1), ARG), ("negative_Hq", dict(Hq=-4), ARG),
    ("negative_L", dict(L=-1), ARG), ("negative_D", dict(D=-64), ARG), ("negative_cs_row", dict(cs_row=-1), ARG),
    ("negative_L_with_B_0", dict(B=0, L=-1), ARG),
    ("q_row_below_width", dict(q_row=248), ARG), ("k_row_below_width", dict(k_row=127), ARG),
    ("v_row_below_width", dict(v_row=126), ARG), ("out_row_below_width", dict(out_row=252), ARG),
    ("cs_row_below_width", dict(cs_row=56), ARG),
    ("q_row_not_a_multiple_of_8", dict(q_row=260), ARG), ("cs_row_not_a_multiple_of_8", dict(cs_row=68), ARG),
    ("out_row_not_a_multiple_of_4", dict(out_row=258), ARG),
    ("v_row_odd", dict(v_row=129), ARG), ("v_misaligned", dict(v=P + 2), ARG),
    ("q_misaligned", dict(q=P + 8), ARG), ("cos_misaligned", dict(cos=P + 8), ARG), ("out_misaligned", dict(out=P + 4), ARG),
    ("k_cache_misaligned", dict(kc=P + 8), ARG), ("v_cache_misaligned", dict(vc=P + 8), ARG),
    ("D_96", dict(D=96), SHAPE), ("L_0", dict(L=0), SHAPE), ("Hkv_0", dict(Hkv=0), SHAPE),
    ("heads_not_a_multiple", dict(Hq=5), SHAPE), ("group_of_16", dict(Hq=16, Hkv=1), SHAPE),
    ("B_65536", dict(B=65536), SHAPE),
    ("dtype_fp32", dict(dtype=F32), DTYPE), ("dtype_7", dict(dtype=7), DTYPE),
    ("B_0", dict(B=0), OK), ("T_0", dict(T=0), OK), ("Hq_0", dict(Hq=0, Hkv=0), OK),
    ("B_0_null_everything", dict(B=0, q=0, pos=0, ln=0, out=0), OK),
]


@pytest.mark.parametrize("case, expected", [pytest.param(c, e, id=n) for n, c, e in ROWS])
def test_prefill_attention_prelaunch_status(case, expected):
    got = attn(**case)
    print(got)
    assert got == expected
