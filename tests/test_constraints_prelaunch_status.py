"""CPU: the status qz_constrain_logits and qz_constraint_advance return BEFORE any HIP call, over a
table of argument combinations they reject (negative status) or have nothing to do for (QZ_OK), in the
manner of test_logprobs_prelaunch_status.py.  Pointers are fake 16-byte-aligned non-null addresses: no
row reaches a launch."""
import pytest

from quantizations_amd import _lib

OK, ARG, SHAPE, DTYPE = 0, -1, -3, -4
F16, BF16, F32 = _lib.DT_F16, _lib.DT_BF16, _lib.DT_F32
P = 4096   # a fake, 16-B-aligned, non-null pointer


def constrain(logits=P, dtype=F16, B=2, T=1, V=1000, row=None, state=P, tok=P, class_of=P, allow=P, next=P, S=5,
              C=40, mask=0, mask_row=0, bias_ids=P, bias_vals=P, bias_n=P, NB=8):
    return _lib.lib.qz_constrain_logits(logits, dtype, B, T, V, V if row is None else row, state, tok, class_of, allow,
                                        next, S, C, mask, mask_row, bias_ids, bias_vals, bias_n, NB, 0)


def advance(state=P, B=2, seq=P, seq_row=16, seq_len=16, pos0=P, pos0_stride=1, pos1=P, pos1_stride=1, class_of=P,
            next=P, V=1000, S=5, C=40):
    return _lib.lib.qz_constraint_advance(state, B, seq, seq_row, seq_len, pos0, pos0_stride, pos1, pos1_stride,
                                          class_of, next, V, S, C, 0)


OFF = dict(state=0, tok=0, class_of=0, allow=0, next=0, S=0, C=0, bias_ids=0, bias_vals=0, bias_n=0, NB=0)
MASK = dict(OFF, mask=P, mask_row=32)

# the expected status is that of the first check that fails: arguments, then the dtype, then the shape
CONSTRAIN = [
    ("null_logits", dict(logits=0), ARG), ("negative_B", dict(B=-1), ARG), ("negative_T", dict(T=-1), ARG),
    ("negative_V", dict(V=-5, row=8), ARG), ("negative_row", dict(row=-1), ARG), ("negative_S", dict(S=-1), ARG),
    ("negative_C", dict(C=-1), ARG), ("negative_NB", dict(NB=-1), ARG), ("negative_mask_row", dict(mask_row=-1), ARG),
    ("negative_B_with_V_0", dict(B=-1, V=0), ARG),
    ("row_below_V", dict(row=999), ARG),
    ("state_without_class_of", dict(class_of=0), ARG), ("state_without_allow", dict(allow=0), ARG),
    ("state_without_next", dict(next=0), ARG), ("state_with_S_0", dict(S=0), ARG), ("state_with_C_0", dict(C=0), ARG),
    ("window_without_tok", dict(T=4, tok=0), ARG),
    ("mask_with_T_2", dict(MASK, T=2), ARG), ("mask_row_too_short", dict(MASK, mask_row=31), ARG),
    ("bias_without_vals", dict(bias_vals=0), ARG), ("bias_without_n", dict(bias_n=0), ARG),
    ("dtype_fp32", dict(dtype=F32), DTYPE), ("dtype_7", dict(dtype=7), DTYPE),
    ("T_17", dict(T=17), SHAPE), ("rows_65536", dict(B=4096, T=16), SHAPE),
    ("rows_overflow_int", dict(B=1 << 30, T=16), SHAPE), ("V_2_pow_31", dict(V=1 << 31), SHAPE),
    ("S_2_pow_31", dict(S=1 << 31), SHAPE), ("C_32768", dict(C=32768), SHAPE),
    ("B_0", dict(B=0), OK), ("T_0", dict(T=0), OK), ("V_0", dict(V=0), OK),
    ("B_0_null_everything", dict(OFF, B=0, logits=0), OK), ("V_0_null_everything", dict(OFF, V=0, logits=0), OK),
    ("every_operand_off", dict(OFF), OK), ("bias_of_no_slots_alone", dict(OFF, bias_ids=P, bias_vals=P, bias_n=P), OK),
]

ADVANCE = [
    ("null_state", dict(state=0), ARG), ("null_seq", dict(seq=0), ARG), ("null_pos0", dict(pos0=0), ARG),
    ("null_pos1", dict(pos1=0), ARG), ("null_class_of", dict(class_of=0), ARG), ("null_next", dict(next=0), ARG),
    ("negative_B", dict(B=-1), ARG), ("negative_V", dict(V=-1), ARG), ("negative_S", dict(S=-1), ARG),
    ("negative_C", dict(C=-1), ARG), ("negative_seq_row", dict(seq_row=-1), ARG),
    ("negative_seq_len", dict(seq_len=-1), ARG), ("negative_seq_len_with_B_0", dict(B=0, seq_len=-1), ARG),
    ("S_0", dict(S=0), ARG), ("C_0", dict(C=0), ARG), ("seq_row_below_seq_len", dict(seq_row=15), ARG),
    ("pos0_stride_2", dict(pos0_stride=2), ARG), ("pos0_stride_negative", dict(pos0_stride=-1), ARG),
    ("pos1_stride_2", dict(pos1_stride=2), ARG), ("pos1_stride_negative", dict(pos1_stride=-1), ARG),
    ("streams_65536", dict(B=65536), SHAPE), ("V_2_pow_31", dict(V=1 << 31), SHAPE),
    ("S_2_pow_31", dict(S=1 << 31), SHAPE), ("C_32768", dict(C=32768), SHAPE),
    ("B_0", dict(B=0), OK), ("V_0", dict(V=0), OK), ("seq_len_0", dict(seq_len=0, seq_row=0), OK),
    ("B_0_null_everything", dict(B=0, state=0, seq=0, pos0=0, pos1=0, class_of=0, next=0), OK),
]


@pytest.mark.parametrize("case, expected", [pytest.param(c, e, id=n) for n, c, e in CONSTRAIN])
def test_constrain_logits_prelaunch_status(case, expected):
    kw = dict(case)
    if expected == ARG:
        kw.setdefault("dtype", F32)     # an argument error is reported in front of the dtype's
    got = constrain(**kw)
    print(got)
    assert got == expected


@pytest.mark.parametrize("case, expected", [pytest.param(c, e, id=n) for n, c, e in ADVANCE])
def test_constraint_advance_prelaunch_status(case, expected):
    got = advance(**case)
    print(got)
    assert got == expected


def test_each_operand_alone_passes_the_argument_checks():
    """The automaton, the mask and the bias alone, with the others null: rejected for the next reason only."""
    auto = dict(bias_ids=0, bias_vals=0, bias_n=0, NB=0)
    assert constrain(dtype=F32, **auto) == DTYPE
    assert constrain(dtype=F32, T=1, tok=0, **auto) == DTYPE          # T = 1 needs no tok
    assert constrain(dtype=F32, **MASK) == DTYPE
    assert constrain(dtype=F32, **dict(OFF, bias_ids=P, bias_vals=P, bias_n=P, NB=4)) == DTYPE
