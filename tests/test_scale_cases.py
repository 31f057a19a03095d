"""CPU: the cases of tests/scale_cases.py reach the edges they claim, shown on the references alone.

* The signature case.  Its fp64 reference is count_d / (p + 1).  Dropping, duplicating or reading
  from its neighbour's place any single chunk (128 keys, decode) or tile (64 keys, prefill) changes
  the element that chunk feeds by about 1 / n of its value, n being the whole chunks that share the
  element's dimension: n = ceil(chunks / D).  "At least half its value" therefore holds only while no
  dimension collects a second chunk, and even then only nearly (duplicating 64 of 65 keys moves the
  other key's element by 0.496 of its value).  At L = 16384 + 130 a dimension collects up to 3 decode
  chunks (D = 64) or 5 prefill tiles, so the bar asserted for a whole chunk is value / (n + 2), and the
  smallest change is printed in units of value / n; a ragged last chunk of 2 keys beside a whole one
  moves its element by 1.5 %.  What the GPU test can see is one spacing of the storage
  dtype at the element (2^-8 of the value at worst, bf16): every perturbation of every chunk, ragged
  ones included, is asserted to move some element by at least 1.75 spacings in both dtypes -- the GPU
  bar is one spacing and the rounding of a wrong kernel's result can give back at most half of one, so
  anything above 1.5 is caught.  That holds for every chunk in fp16 and every whole chunk in bf16.  A
  ragged chunk of one key is below bf16's resolution where its dimension is crowded: the single key of
  decode chunk 64 at p = 8192 moves its element by 1.9 spacings beside the 128 keys of chunk 0
  (D = 128) and by 1.0 beside 256 keys (D = 64); the single key of prefill tile 258 at p = L - 2 by 1.0
  and 0.5.  fp16 sees the same keys at 15.4, 7.8, 7.8 and 3.9 spacings.  The bf16
  figures are printed, not asserted; the same kernel templates run the fp16 case.
* The random case.  k0 -- the worst error of an fp32 restatement against fp64, in spacings of the
  storage dtype at the row's largest |value| -- is printed per (dtype, D, L) and is below 1: the
  restatement's error is its final rounding.  The GPU bar is k = 2 k0 + 1 < 3 spacings.  Removing a
  whole chunk from the fp64 reference must move some element of the row by at least 4 k; the smallest
  move over every whole chunk of every row is printed and asserted.  Ragged chunks (1 key at p = 128,
  2 keys at the end) cannot meet that in any dtype -- one key of 16514 weighs 6e-5 -- and are the
  signature case's to catch.  RANDOM_L holds, per (kind, dtype, D), the longest length offered that
  meets the condition, and this module shows that it is the longest.  Measured (heads (4, 2)):
      decode  fp16 D=64/128  L=16514: k0 0.41/0.45, smallest move 40.9/41.0 spacings (4 k = 7.3/7.6)
      decode  bf16 D=64   L=16514: 4.9 < 7.7;  L=8322: 8.9 >= 7.8 (k0 0.48)
      decode  bf16 D=128  L=16514: 5.9 < 7.3;  L=8322: 7.0 < 7.8;  L=4226: 11.2 >= 7.2 (k0 0.40)
      prefill fp16 D=64/128  L=16514: k0 0.66/0.60, smallest move 20.0/23.5 (4 k = 9.3/8.8)
      prefill bf16 D=64   L=16514/8322/4226: 2.1/3.9/6.3 against 4 k = 8.9/8.9/9.3
      prefill bf16 D=128  L=16514/8322/4226: 2.4/4.0/6.9 against 4 k = 8.7/9.5/8.8
  So no length offered meets it for the bf16 prefill tile.  Those cases run at 4096 + 130, where the
  removal of a tile moves a row by more than 2 k: a kernel that drops one still leaves the bar, its own
  error of up to k counted against it.  That weaker margin is asserted here and named in the GPU module.
* chunk_slices maps row chunks to packed, block and double-quant group ranges with block indices
  above 2^31, in integer arithmetic; boundary_rows holds the rows it promises.
"""
import pytest
import torch

import activation_families as af
import prefill_reference as pfr
import scale_cases as sc

CASES = [(name, D) for name in ("fp16", "bf16") for D in (64, 128)]
_memo = {}


def _case(kind, which, name, D, L):
    """decode: T = 1 at decode_positions; prefill: T = TQ + 1 at prefill_streams.  Heads (4, 2)."""
    key = (kind, which, name, D, L)
    if key not in _memo:
        _memo.clear()        # one long case in memory at a time
        unit = sc.CHUNK if kind == "decode" else sc.TILE
        T = 1 if kind == "decode" else pfr.TQ + 1
        ps, ns = (sc.decode_positions(L), [1] * 6) if kind == "decode" else sc.prefill_streams(L, T)
        seed = sc.case_seed(kind, name, D, L, T, 4)
        if which == "signature":
            _memo[key] = sc.signature_case(T, 4, 2, D, L, ps, ns, name, unit, seed)
        else:
            _memo[key] = sc.random_case(T, 4, 2, D, L, ps, ns, name, seed)
    return _memo[key]


def _rows_of(case, b):
    n = pfr.legal_rows(case, b)
    return sorted({0, n - 1}) if n else []


@pytest.mark.parametrize("kind", ["decode", "prefill"])
@pytest.mark.parametrize("name,D", CASES)
def test_signature_reference_is_the_chunk_census(kind, name, D):
    L = sc.L_LONG
    unit = sc.CHUNK if kind == "decode" else sc.TILE
    case = _case(kind, "signature", name, D, L)
    ref = sc.reference_fp64(case).reshape(case["B"], case["T"], case["Hq"], D)
    dt = sc.DTYPES[name]
    worst_whole, worst_any = float("inf"), float("inf")
    for b in range(case["B"]):
        rows = _rows_of(case, b)
        if not rows:
            continue
        w, Vp, keys = sc.chunk_partials(case, b, rows, unit)
        out, drop, dup, moved = sc.perturbed_outputs(w, Vp)
        for r, i in enumerate(rows):
            p = case["pos"][b] + i
            # the reference is the census: count_d / (p + 1)
            count = sc.signature_rows(torch.arange(p + 1), D, unit, torch.float64).sum(0)
            assert torch.allclose(out[:, r], (count / (p + 1)).expand(case["Hq"], D), rtol=1e-12, atol=0)
            assert torch.allclose(ref[b, i], out[:, r], rtol=1e-12, atol=0)
            C = int((keys[r] > 0).sum())               # the chunks this row sees
            n_share = -(-C // D)
            for what, pert in (("drop", drop), ("duplicate", dup), ("move", moved)):
                for c in range(keys.shape[1]):
                    if keys[r, c] == 0 or C == 1:     # a row's only chunk: a mean is blind to its own multiple
                        continue
                    delta = (pert[:, r, c] - out[:, r]).abs()
                    rel = (delta / out[:, r].abs().clamp(min=1e-300)).amax(-1).min().item()
                    spacings = (delta / af.ulp_at(torch.maximum(out[:, r], pert[:, r, c]), dt)).amax(-1).min().item()
                    if keys[r, c] == unit:
                        worst_whole = min(worst_whole, rel * n_share)
                        assert rel >= 1.0 / (n_share + 2), (what, b, i, c, rel, n_share)
                    worst_any = min(worst_any, spacings)
                    if keys[r, c] == unit or name == "fp16":
                        assert spacings >= 1.75, (what, b, i, c, int(keys[r, c]), spacings)
    print(f"signature {kind} {name} D={D} L={L}: smallest change of a whole chunk = {worst_whole:.3f} x value / n; "
          f"of any chunk = {worst_any:.1f} spacings")


def _random_figures(kind, name, D, L):
    """(k0, smallest move of a whole chunk's removal in spacings, the same over ragged chunks)."""
    unit = sc.CHUNK if kind == "decode" else sc.TILE
    case = _case(kind, "random", name, D, L)
    ref = sc.reference_fp64(case)
    k0 = sc.units_of_error(sc.restatement_f32(case, unit, round_p=kind == "prefill"), ref, case).max().item()
    whole, ragged = float("inf"), float("inf")
    for b in range(case["B"]):
        rows = _rows_of(case, b)
        if not rows:
            continue
        move, keys = sc.removal_sensitivity(case, b, rows, unit)
        full = (keys == unit)[None].expand_as(move)
        part = ((keys > 0) & (keys < unit))[None].expand_as(move)
        if full.any():
            whole = min(whole, move[full].min().item())
        if part.any():
            ragged = min(ragged, move[part].min().item())
    return k0, whole, ragged


@pytest.mark.parametrize("kind", ["decode", "prefill"])
@pytest.mark.parametrize("name,D", CASES)
def test_random_case_bar_and_chunk_sensitivity(kind, name, D):
    L = sc.RANDOM_L[(kind, name, D)]
    k0, whole, ragged = _random_figures(kind, name, D, L)
    k = 2 * k0 + 1
    print(f"random {kind} {name} D={D} L={L}: k0 = {k0:.3f}, k = {k:.3f}, 4 k = {4 * k:.2f}; removing a whole chunk moves "
          f"a row by at least {whole:.2f} spacings, a ragged one by at least {ragged:.4f}")
    assert k0 < 1.0, "the fp32 restatement's error is its final rounding"
    if (kind, name, D) in sc.RANDOM_BELOW_CONDITION:
        # no length offered meets 4 k here (see the module docstring); the margin that is left is asserted
        assert 2 * k < whole < 4 * k, (whole, k)
    else:
        assert whole >= 4 * k, (whole, k)


@pytest.mark.parametrize("kind,D", [("decode", 64), ("decode", 128), ("prefill", 64), ("prefill", 128)])
def test_bf16_runs_at_the_longest_length_that_meets_the_condition(kind, D):
    """Every longer length of L_CHOICES fails the 4 k condition; where the chosen one fails it too it is
    the shortest offered."""
    chosen = sc.RANDOM_L[(kind, "bf16", D)]
    for L in sc.L_CHOICES:
        if L <= chosen and (kind, "bf16", D) not in sc.RANDOM_BELOW_CONDITION:
            break
        k0, whole, _ = _random_figures(kind, "bf16", D, L)
        print(f"random {kind} bf16 D={D} L={L}: k0 = {k0:.3f}, 4 k = {4 * (2 * k0 + 1):.2f}, removing a whole chunk moves at "
              f"least {whole:.2f} spacings")
        assert whole < 4 * (2 * k0 + 1)
    if (kind, "bf16", D) in sc.RANDOM_BELOW_CONDITION:
        assert chosen == min(sc.L_CHOICES)


def test_chunk_slices_above_2_to_the_31():
    K, bs = sc.BIG_K, 64
    # rows whose first block index is 2^31 and 2^32 - 128: a weight of 2^37 codes
    for r0 in ((1 << 31) * bs // K, ((1 << 32) - 128) * bs // K):
        y0, y1, b0, b1, g0, g1 = sc.chunk_slices(r0, r0 + sc.REF_ROWS, K, bs)
        assert b0 >= 1 << 31 and b0 == r0 * (K // bs) and b1 - b0 == sc.REF_ROWS * (K // bs)
        assert y0 == b0 * bs // 2 and y1 - y0 == sc.REF_ROWS * K // 2 and y0 >= 1 << 36
        assert g0 * 256 <= b0 < (g0 + 1) * 256 and (g1 - 1) * 256 < b1 <= g1 * 256
    # chunks tile the big weight exactly, through the 2^31-element and 2^32-element rows
    prev = (0, 0)
    for r0 in range(0, sc.BIG_ROWS, sc.REF_ROWS):
        y0, y1, b0, b1, _, _ = sc.chunk_slices(r0, r0 + sc.REF_ROWS, K, bs)
        assert (y0, b0) == prev
        prev = (y1, b1)
    assert prev == (1 << 31, (1 << 32) // bs)
    assert sc.chunk_slices(262144, 262145, K, bs)[:4] == (1 << 30, (1 << 30) + K // 2, (1 << 31) // bs, (1 << 31) // bs + K // bs)


def test_row_list_dequantiser_equals_the_row_range_one():
    """dequantize_row_list (the reference of the boundary-row GEMM test) against dequantize_rows on a
    64-row weight of the big weight's K, plain and double-quant scales; its block index is int64."""
    g = torch.Generator().manual_seed(4)
    rows_n, bs = 64, 64
    blocks = rows_n * sc.BIG_K // bs
    w = dict(packed=torch.randint(0, 256, (rows_n * sc.BIG_K // 2, 1), generator=g, dtype=torch.uint8),
             absmax=torch.rand(blocks, generator=g) + 0.5, qabsmax=torch.randint(0, 256, (blocks,), generator=g, dtype=torch.uint8),
             absmax2=torch.rand(blocks // 256, generator=g) + 0.5, offset=torch.tensor(0.75),
             code2=torch.linspace(-1, 1, 256), blocksize=bs, blocksize2=256)
    code = torch.linspace(-1, 1, 16)
    rows = [0, 1, 17, 31, 32, 63]
    for nested in (False, True):
        full = sc.dequantize_rows(w, 0, rows_n, code, nested)
        got = sc.dequantize_row_list(w, rows, code, nested)
        assert torch.equal(got, full[rows])
    r = torch.tensor([(1 << 32) * bs // sc.BIG_K - 1], dtype=torch.int64)
    assert int((r * (sc.BIG_K // bs) + sc.BIG_K // bs - 1)[0]) == (1 << 32) - 1      # no 32-bit wrap in the index


def test_boundary_rows():
    M, K = sc.BIG_ROWS, sc.BIG_K
    rows = sc.boundary_rows(M, K)
    assert rows == sorted(set(rows)) and rows[0] == 0 and rows[-1] == M - 1
    have = set(rows)
    assert set(range(64)) <= have and set(range(M - 64, M)) <= have
    r31 = (1 << 31) // K                       # elements cross 2^31 here; bytes cross 2^31 at 2 r31 = M
    assert set(range(r31 - 32, r31 + 32)) <= have
    assert len(rows) >= 4096 and rows == sc.boundary_rows(M, K)
    M2, K2 = 262144 + 512, 16384               # r K crosses 2^31 at 131072, 2^32 at 262144; bytes 2^31 at 262144
    have = set(sc.boundary_rows(M2, K2))
    for r in (131072, 262144):
        assert set(range(r - 32, r + 32)) <= have
    small = sc.boundary_rows(100, 64)
    assert small == list(range(100))
