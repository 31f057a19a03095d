"""CPU: the status the three paged attention entry points return BEFORE any HIP call, over a table of
argument combinations they reject (negative status) or have nothing to do for (QZ_OK), in the manner
of test_prefill_prelaunch_status.py.  Pointers are fake 16-byte-aligned non-null addresses: no row
reaches a launch.  The rows of the contiguous twins are kept with NP, P in place of L; the paged
operands add a null table, table_row < NP, NP or P negative (ARG) or zero with work to do (SHAPE) and
misaligned pools."""
import pytest

from quantizations_amd import _lib

OK, ARG, SHAPE, DTYPE = 0, -1, -3, -4
F16, BF16, F32 = _lib.DT_F16, _lib.DT_BF16, _lib.DT_F32
P = 4096   # a fake, 16-B-aligned, non-null pointer


def _common(kw):
    d = dict(dtype=F16, B=2, T=4, Hq=4, Hkv=2, D=64, NP=2, NPG=8, q=P, q_row=None, k=P, k_row=None, v=P, v_row=None,
             cos=P, sin=P, cs_row=64, kp=P, vp=P, table=P, table_row=None, pos=P, ln=P, out=P, out_row=None, work=P)
    d.update(kw)
    for name, w in (("q_row", d["Hq"] * d["D"]), ("k_row", d["Hkv"] * d["D"]), ("v_row", d["Hkv"] * d["D"]),
                    ("out_row", d["Hq"] * d["D"]), ("table_row", d["NP"])):
        if d[name] is None:
            d[name] = w
    return d


def decode(**kw):
    d = _common(kw)
    return _lib.lib.qz_decode_attention_paged(
        d["dtype"], d["B"], d["Hq"], d["Hkv"], d["D"], d["NP"], d["NPG"], d["q"], d["q_row"], d["k"], d["k_row"], d["v"],
        d["v_row"], d["cos"], d["sin"], d["cs_row"], d["kp"], d["vp"], d["table"], d["table_row"], d["pos"], d["out"],
        d["out_row"], d["work"], 0.125, 0)


def verify(**kw):
    d = _common(kw)
    return _lib.lib.qz_decode_attention_verify_paged(
        d["dtype"], d["B"], d["T"], d["Hq"], d["Hkv"], d["D"], d["NP"], d["NPG"], d["q"], d["q_row"], d["k"], d["k_row"],
        d["v"], d["v_row"], d["cos"], d["sin"], d["cs_row"], d["kp"], d["vp"], d["table"], d["table_row"], d["pos"],
        d["out"], d["out_row"], d["work"], 0.125, 0)


def prefill(**kw):
    d = _common(kw)
    return _lib.lib.qz_prefill_attention_paged(
        d["dtype"], d["B"], d["T"], d["Hq"], d["Hkv"], d["D"], d["NP"], d["NPG"], d["q"], d["q_row"], d["k"], d["k_row"],
        d["v"], d["v_row"], d["cos"], d["sin"], d["cs_row"], d["kp"], d["vp"], d["table"], d["table_row"], d["pos"],
        d["ln"], d["out"], d["out_row"], 0.125, 0)


# rows every entry point shares
SHARED = [
    ("null_q", dict(q=0), ARG), ("null_k", dict(k=0), ARG), ("null_v", dict(v=0), ARG),
    ("null_cos", dict(cos=0), ARG), ("null_sin", dict(sin=0), ARG),
    ("null_k_pool", dict(kp=0), ARG), ("null_v_pool", dict(vp=0), ARG), ("null_table", dict(table=0), ARG),
    ("null_pos", dict(pos=0), ARG), ("null_out", dict(out=0), ARG),
    ("negative_B", dict(B=-1), ARG), ("negative_Hq", dict(Hq=-4), ARG), ("negative_D", dict(D=-64), ARG),
    ("negative_NP", dict(NP=-1), ARG), ("negative_P", dict(NPG=-1), ARG), ("negative_cs_row", dict(cs_row=-1), ARG),
    ("negative_NP_with_B_0", dict(B=0, NP=-1), ARG),
    ("q_row_below_width", dict(q_row=248), ARG), ("k_row_below_width", dict(k_row=127), ARG),
    ("v_row_below_width", dict(v_row=126), ARG), ("out_row_below_width", dict(out_row=252), ARG),
    ("table_row_below_NP", dict(table_row=1), ARG), ("table_row_0", dict(table_row=0), ARG),
    ("v_row_odd", dict(v_row=129), ARG), ("v_misaligned", dict(v=P + 2), ARG),
    ("k_pool_misaligned", dict(kp=P + 8), ARG), ("v_pool_misaligned", dict(vp=P + 8), ARG),
    ("D_96", dict(D=96), SHAPE), ("NP_0", dict(NP=0, table_row=1), SHAPE), ("P_0", dict(NPG=0), SHAPE),
    ("Hkv_0", dict(Hkv=0), SHAPE), ("heads_not_a_multiple", dict(Hq=5), SHAPE),
    ("group_of_16", dict(Hq=16, Hkv=1), SHAPE),
    ("dtype_fp32", dict(dtype=F32), DTYPE), ("dtype_7", dict(dtype=7), DTYPE),
    ("B_0", dict(B=0), OK), ("Hq_0", dict(Hq=0, Hkv=0), OK),
    ("B_0_null_everything", dict(B=0, q=0, pos=0, table=0, kp=0, out=0), OK),
    ("table_row_above_NP", dict(table_row=5, B=0), OK),
]
DECODE_ONLY = [("B_65536", dict(B=65536), SHAPE), ("null_work_two_pages", dict(work=0), ARG)]
VERIFY_ONLY = [("negative_T", dict(T=-1), ARG), ("T_0", dict(T=0), OK), ("rows_65536", dict(B=16384, T=4), SHAPE),
               ("null_work_two_pages", dict(work=0), ARG)]
PREFILL_ONLY = [
    ("negative_T", dict(T=-1), ARG), ("T_0", dict(T=0), OK), ("null_len", dict(ln=0), ARG), ("B_65536", dict(B=65536), SHAPE),
    ("cs_row_below_width", dict(cs_row=56), ARG), ("q_row_not_a_multiple_of_8", dict(q_row=260), ARG),
    ("cs_row_not_a_multiple_of_8", dict(cs_row=68), ARG), ("out_row_not_a_multiple_of_4", dict(out_row=258), ARG),
    ("q_misaligned", dict(q=P + 8), ARG), ("cos_misaligned", dict(cos=P + 8), ARG), ("out_misaligned", dict(out=P + 4), ARG),
]
CASES = ([(decode, "decode", r) for r in SHARED + DECODE_ONLY] + [(verify, "verify", r) for r in SHARED + VERIFY_ONLY]
         + [(prefill, "prefill", r) for r in SHARED + PREFILL_ONLY])


@pytest.mark.parametrize("fn, case, expected", [pytest.param(f, c, e, id=f"{w}-{n}") for f, w, (n, c, e) in CASES])
def test_paged_attention_prelaunch_status(fn, case, expected):
    got = fn(**case)
    print(got)
    assert got == expected


def test_one_page_needs_no_workspace_check():
    """NP = 1 has no combine: a null work is not an error by itself (the next check, the dtype, answers)."""
    assert decode(NP=1, work=0, dtype=F32) == DTYPE
    assert verify(NP=1, work=0, dtype=F32) == DTYPE
