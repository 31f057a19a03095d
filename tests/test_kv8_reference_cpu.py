"""CPU: the properties of the kv8 format that make the GPU tests exact (kv8_reference.py): every
dequantised value is a 16-bit number, the scale is the smallest that keeps the row inside E4M3, and a
dequantised row quantises to itself."""
import pytest
import torch

import kv8_reference as k8

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
ALL_CODES = torch.arange(256, dtype=torch.int32).to(torch.uint8)
FINITE = ALL_CODES[(ALL_CODES & 0x7F) != 0x7F]


def _exact_values(codes, e):
    """decode(code) 2^e in fp64 (exact)."""
    return codes.view(k8.F8).to(torch.float32).double() * 2.0 ** e


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_every_dequantised_value_is_a_storage_number(dt):
    """Every finite code at every e from e_min to E_MAX - 1: the value survives the storage dtype
    unchanged.  (At E_MAX itself -- 8 for fp16, 120 for bf16 -- 448 2^e is past the dtype's largest
    number: the next test.)"""
    for e in range(k8.E_MIN[dt], k8.E_MAX[dt]):
        got = k8.dequantize_rows(FINITE.unsqueeze(0), torch.tensor([e + 127], dtype=torch.uint8), dt)[0]
        assert torch.equal(got.double(), _exact_values(FINITE, e)), e   # no rounding happened
        assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_the_top_scale_overflows_exactly_at_magnitude_256(dt):
    """e = 8 on fp16 (and e = 120 on bf16, the same edge): 256 2^e is 2^16 (2^128), one past the largest
    finite number, so exactly the codes of magnitude >= 256 read back as inf and the rest stay exact.
    Only a row whose absmax scales to 248 or more holds such a code: fp16 elements from 63488 up, the
    seven largest bf16 numbers."""
    e = k8.E_MAX[dt]
    got = k8.dequantize_rows(FINITE.unsqueeze(0), torch.tensor([e + 127], dtype=torch.uint8), dt)[0]
    mag = FINITE.view(k8.F8).to(torch.float32).abs()
    assert torch.equal(torch.isinf(got), mag >= 256)
    keep = mag < 256
    assert torch.equal(got[keep].double(), _exact_values(FINITE, e)[keep])
    top = torch.tensor([63456.0, 63488.0] if dt == torch.float16 else [1.9296875 * 2.0 ** 127, 1.9375 * 2.0 ** 127]).to(dt)
    back = k8.dequantize_rows(*k8.quantize_rows(top.reshape(2, 1).expand(2, 64).contiguous()), dt)
    assert torch.isfinite(back[0]).all() and torch.isinf(back[1]).all()


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_the_scaled_absmax_fills_the_top_binade(dt):
    pats = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dt)
    a = pats[torch.isfinite(pats)].to(torch.float32).abs()
    e = k8.scale_exponent(a, dt)
    scaled = a.double() * torch.pow(2.0, -e.double())
    free = e > k8.E_MIN[dt]
    assert bool(((scaled[free] > 224) & (scaled[free] <= 448)).all())
    assert bool((scaled[~free] <= 448).all())
    assert int(e.max()) == k8.E_MAX[dt]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_quantising_a_dequantised_row_gives_the_row_back(dt):
    """Rows whose largest code is above 224 in magnitude: the scaled absmax of the rule lies in
    (224, 448], so at 224 or below the row's scale is not the minimal one and it requantises finer."""
    g = torch.Generator().manual_seed(5)
    tops = FINITE[FINITE.view(k8.F8).to(torch.float32).abs() > 224]
    n = 0
    for e in range(k8.E_MIN[dt], k8.E_MAX[dt]):           # not the top scale: its large codes read back as inf
        codes = FINITE[torch.randint(0, FINITE.numel(), (len(tops), 64), generator=g)]
        codes[:, 17] = tops                                   # an element of magnitude > 224 in every row
        scales = torch.full((len(tops),), e + 127, dtype=torch.uint8)
        rows = k8.dequantize_rows(codes, scales, dt)
        c2, s2 = k8.quantize_rows(rows)
        assert torch.equal(s2, scales), e
        # -0 and +0 codes: the sign survives the round trip too
        assert torch.equal(c2, codes), e
        n += len(tops)
    assert n > 0


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_a_non_finite_element_poisons_its_row_only(dt, bad):
    rows = torch.randn((3, 64), generator=torch.Generator().manual_seed(1)).to(dt)
    rows[1, 40] = bad
    codes, scales = k8.quantize_rows(rows)
    assert int(scales[1]) == 255 and bool((codes[1] == 0x7F).all())
    back = k8.dequantize_rows(codes, scales, dt)
    assert bool(torch.isnan(back[1]).all()) and bool(torch.isfinite(back[[0, 2]]).all())


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_zero_rows_and_zero_pages(dt):
    codes, scales = k8.quantize_rows(torch.zeros((2, 64), dtype=dt))
    assert bool((codes == 0).all()) and scales.tolist() == [k8.E_MIN[dt] + 127] * 2
    pool = torch.zeros((2, 2, k8.PAGE * 65), dtype=torch.uint8)
    assert bool((k8.dequantize_pool(pool, 64, dt) == 0).all())


def test_pool_layout_round_trip():
    g = torch.Generator().manual_seed(2)
    codes = torch.randint(0, 256, (3, 2, k8.PAGE, 64), generator=g).to(torch.uint8)
    scales = torch.randint(0, 256, (3, 2, k8.PAGE), generator=g).to(torch.uint8)
    pool = k8.pack_pool(codes, scales)
    assert pool.shape == (3, 2, k8.PAGE * 65)
    c2, s2 = k8.unpack_pool(pool, 64)
    assert torch.equal(c2, codes) and torch.equal(s2, scales)
    # row j of block (page, h): codes at (j & 127) D, scale at 128 D + (j & 127)
    flat = pool.reshape(-1)
    base = (2 * 2 + 1) * k8.PAGE * 65
    assert torch.equal(flat[base + 77 * 64: base + 78 * 64], codes[2, 1, 77]) and flat[base + k8.PAGE * 64 + 77] == scales[2, 1, 77]


def test_the_rounding_is_nearest_even_and_never_saturates():
    x = torch.tensor([447.0, 448.0, 2.0 ** -10, 1.5 * 2.0 ** -10, 2.5 * 2.0 ** -9, 3.5 * 2.0 ** -9])
    assert x.to(k8.F8).view(torch.uint8).tolist() == [126, 126, 0, 1, 2, 4]
