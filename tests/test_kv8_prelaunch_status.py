"""CPU: the status the three kv8 attention entry points return BEFORE any HIP call: the table of
test_paged_prelaunch_status.py, row for row, on qz_decode_attention_paged_kv8,
qz_decode_attention_verify_paged_kv8 and qz_prefill_attention_paged_kv8 (they take their _paged twins'
operand lists and rules; the pools are byte pools), and the size of a (page, kv head) block."""
import pytest
from test_paged_prelaunch_status import (DECODE_ONLY, DTYPE, F32, PREFILL_ONLY, SHARED, VERIFY_ONLY, _common)

from quantizations_amd import _lib


def decode(**kw):
    d = _common(kw)
    return _lib.lib.qz_decode_attention_paged_kv8(
        d["dtype"], d["B"], d["Hq"], d["Hkv"], d["D"], d["NP"], d["NPG"], d["q"], d["q_row"], d["k"], d["k_row"], d["v"],
        d["v_row"], d["cos"], d["sin"], d["cs_row"], d["kp"], d["vp"], d["table"], d["table_row"], d["pos"], d["out"],
        d["out_row"], d["work"], 0.125, 0)


def verify(**kw):
    d = _common(kw)
    return _lib.lib.qz_decode_attention_verify_paged_kv8(
        d["dtype"], d["B"], d["T"], d["Hq"], d["Hkv"], d["D"], d["NP"], d["NPG"], d["q"], d["q_row"], d["k"], d["k_row"],
        d["v"], d["v_row"], d["cos"], d["sin"], d["cs_row"], d["kp"], d["vp"], d["table"], d["table_row"], d["pos"],
        d["out"], d["out_row"], d["work"], 0.125, 0)


def prefill(**kw):
    d = _common(kw)
    return _lib.lib.qz_prefill_attention_paged_kv8(
        d["dtype"], d["B"], d["T"], d["Hq"], d["Hkv"], d["D"], d["NP"], d["NPG"], d["q"], d["q_row"], d["k"], d["k_row"],
        d["v"], d["v_row"], d["cos"], d["sin"], d["cs_row"], d["kp"], d["vp"], d["table"], d["table_row"], d["pos"],
        d["ln"], d["out"], d["out_row"], 0.125, 0)


CASES = ([(decode, "decode", r) for r in SHARED + DECODE_ONLY] + [(verify, "verify", r) for r in SHARED + VERIFY_ONLY]
         + [(prefill, "prefill", r) for r in SHARED + PREFILL_ONLY])


@pytest.mark.parametrize("fn, case, expected", [pytest.param(f, c, e, id=f"{w}-{n}") for f, w, (n, c, e) in CASES])
def test_kv8_attention_prelaunch_status(fn, case, expected):
    got = fn(**case)
    print(got)
    assert got == expected


def test_one_page_needs_no_workspace_check():
    assert decode(NP=1, work=0, dtype=F32) == DTYPE
    assert verify(NP=1, work=0, dtype=F32) == DTYPE


def test_page_head_bytes():
    assert _lib.lib.qz_kv8_page_head_bytes(64) == 8320 and _lib.lib.qz_kv8_page_head_bytes(128) == 16512
    assert _lib.lib.qz_kv8_page_head_bytes(96) < 0
