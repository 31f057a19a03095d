"""Shared by the tests of extent (test_gpu_long_context.py, test_gpu_large_offsets.py; proved on the
CPU by test_scale_cases.py): attention cases at long context, a weight of 2^32 codes built on the
device, and the rows a 2^31 / 2^32 boundary crosses.  Plain torch; importing it needs no GPU.

Attention cases are prefill_reference.make_case dicts (q / k / v [B, T, *], cos / sin [B, T, D],
caches [B, Hkv, L, D], one position and one length per stream), generated on the CPU from a seed.
T = 1 is a decode step, T = 4 a verify window, anything else a prefill window.  The CPU proof and
the GPU tests draw from the same recipe but not the same values: the proof measures heads (4, 2) at
T = 1 / TQ + 1 and length L, the GPU tests generate at L rounded up to whole pages and also run heads
(8, 1), T = 4 and T = 1, and the seed depends on all of these.  What the proof shows (k0, the
sensitivity to a lost chunk) holds for siblings of the GPU inputs; the GPU tests therefore measure k0
again on their own inputs and take their bar from that.

  signature_case   q = 0, so every visible key weighs the same; v[j, d] = 1 where
                   d == (j // unit) % D, else 0 (unit = the decode chunk of 128 keys or the prefill
                   tile of 64); k random.  The output is count_d / (p + 1): which chunks were summed,
                   and how often, is written in the value.  0 and 1 are exact in fp16, bf16 and kv8.
  random_case      the randn recipe of prefill_reference.make_case, NaN at and above each stream's
                   position.

reference_fp64 is the plain softmax(q k^T * scale) v in float64; restatement_f32 the same attention in
fp32 chunk by chunk (online softmax, optionally P rounded to the storage dtype before P V), whose
error against fp64 -- k0, in spacings of the storage dtype at the row's largest |value| -- sets the
bar k = 2 k0 + 1 of the random case.  chunk_partials splits the fp64 reference into per-chunk sums so
a chunk can be dropped, duplicated or read from its neighbour's place.
"""
import math

import torch

import activation_families as af
import prefill_reference as pfr

CHUNK = 128                  # layer_ops.ATTN_CHUNK: keys per decode workgroup, positions per page
TILE = pfr.TK                # layer_ops.PREFILL_TK: keys per prefill tile
L_LONG = 16384 + 130         # 130 chunks / 259 tiles, both with a ragged last one
L_CHOICES = (16384 + 130, 8192 + 130, 4096 + 130)
DTYPES = pfr.DTYPES
HEADS = [(8, 1), (4, 2)]


def case_seed(kind, name, D, L, T, Hq):
    return 1000 * (("decode", "prefill").index(kind) + 1) + 100 * ("fp16", "bf16").index(name) + D + L + 7 * T + Hq


# The length of the random case per (kind, dtype, D): the longest of L_CHOICES at which removing any
# whole chunk from the fp64 reference moves some element of the row by >= 4 k spacings
# (test_scale_cases.py measures it).  fp16 holds it at L_LONG.  bf16, decode chunks: D = 64 at 8192 + 130,
# D = 128 at 4096 + 130.  bf16, prefill tiles: no length offered holds it (a tile is half a chunk and
# bf16's spacing is 8 times fp16's); those run at the shortest length, where the removal of a tile
# still moves a row by more than 2 k -- beyond the bar even with the kernel's own k against it.
RANDOM_L = {(kind, name, D): L_LONG for kind in ("decode", "prefill") for name in ("fp16", "bf16") for D in (64, 128)}
RANDOM_L[("decode", "bf16", 64)] = 8192 + 130
RANDOM_L[("decode", "bf16", 128)] = 4096 + 130
RANDOM_L[("prefill", "bf16", 64)] = RANDOM_L[("prefill", "bf16", 128)] = 4096 + 130
RANDOM_BELOW_CONDITION = {("prefill", "bf16", 64), ("prefill", "bf16", 128)}


def mid_position(L):
    """8192 at L_LONG; 4096 and 2048 at the shorter choices."""
    return (L - 130) // 2


def decode_positions(L, T=1):
    """Stream positions of the decode forms: 0, 127, 128, 8191, 8192 (L_LONG; the middle of a shorter
    cache) and the last window of the cache."""
    return [0, 127, 128, mid_position(L) - 1, mid_position(L), L - T]


def prefill_streams(L, T):
    """(positions, lengths): windows at 0, 8191, 8192, L - T - 3 and L - 2 (the last runs off the end)
    with T real rows, then the lengths T - 1, 1 and 0 at 8191 (mid_position(L) for a shorter cache)."""
    mid = mid_position(L)
    ps = [0, mid - 1, mid, L - T - 3, L - 2]
    ns = [T] * len(ps)
    for n in pfr.window_lengths(T)[1:]:
        ps.append(mid - 1)
        ns.append(n)
    return ps, ns


def signature_rows(positions, D, unit, dt):
    """v rows of the signature case for keys at `positions` (any integer tensor): [..., D]."""
    d = (positions // unit) % D
    return torch.nn.functional.one_hot(d, D).to(dt)


def signature_case(T, Hq, Hkv, D, L, ps, lens, name, unit, seed):
    """See the module docstring.  NaN at and above each stream's position in both caches, as in the
    random case: a key too many shows."""
    c = pfr.make_case(len(ps), T, Hq, Hkv, D, L, ps, lens, name, seed, nan_above=False)
    dt = DTYPES[name]
    c["q"] = torch.zeros_like(c["q"])
    c["vc"] = signature_rows(torch.arange(L), D, unit, dt).expand(len(ps), Hkv, L, D).contiguous()
    pos = torch.tensor(ps).view(-1, 1) + torch.arange(T).view(1, -1)            # [B, T]
    c["v"] = signature_rows(pos.clamp(min=0), D, unit, dt).unsqueeze(2).expand(-1, -1, Hkv, -1).reshape(len(ps), T, Hkv * D).contiguous()
    for b, p in enumerate(ps):
        if 0 <= p < L:
            c["kc"][b, :, p:] = float("nan")
            c["vc"][b, :, p:] = float("nan")
    c["unit"] = unit
    return c


def random_case(T, Hq, Hkv, D, L, ps, lens, name, seed):
    return pfr.make_case(len(ps), T, Hq, Hkv, D, L, ps, lens, name, seed, nan_above=True)


def to_device(case, device):
    out = dict(case)
    for n in ("q", "k", "v", "cos", "sin", "kc", "vc"):
        out[n] = case[n].to(device)
    return out


def written_slots(case):
    """{b: the cache positions stream b's window writes}."""
    return {b: list(range(p, p + pfr.legal_rows(case, b))) for b, p in enumerate(case["pos"])}


def _stream_operands(case, b, requant=None):
    """(q [Hq, n, D], K, V [Hq, p + n, D], row positions [n]) of stream b's computed rows; K and V are
    the caches after the window's write (requant: what a written row reads back as)."""
    G = case["Hq"] // case["Hkv"]
    n, p = pfr.legal_rows(case, b), case["pos"][b]
    qr, kr = pfr.rotated(case)
    vn = case["v"].view(case["B"], case["T"], case["Hkv"], case["D"])
    knew, vnew = kr[b, :n].transpose(0, 1), vn[b, :n].transpose(0, 1)          # [Hkv, n, D]
    if requant is not None:
        knew, vnew = requant(knew), requant(vnew)
    K = torch.cat((case["kc"][b, :, :p], knew), 1).repeat_interleave(G, 0)
    V = torch.cat((case["vc"][b, :, :p], vnew), 1).repeat_interleave(G, 0)
    rows = p + torch.arange(n, device=K.device)
    return qr[b, :n].transpose(0, 1), K, V, rows


def _fill_illegal(case, out):
    fill = pfr.expected_fill(case)
    for b in range(case["B"]):
        for i in range(case["T"]):
            if fill[b][i] == "nan":
                out[b, i] = float("nan")
    return out


def reference_fp64(case, requant=None):
    """softmax(q k^T * scale) v over keys 0 .. pos[b] + i in float64, a stream at a time:
    [B, T, Hq D]; NaN for real rows that have no slot, zeros for padding rows."""
    B, T, Hq, D = case["B"], case["T"], case["Hq"], case["D"]
    out = torch.zeros(B, T, Hq, D, dtype=torch.float64, device=case["q"].device)
    for b in range(B):
        if pfr.legal_rows(case, b) == 0:
            continue
        q, K, V, rows = _stream_operands(case, b, requant)
        sc = torch.einsum("htd,hnd->htn", q.double(), K.double()) * case["scale"]
        vis = torch.arange(K.shape[1], device=K.device)[None, None, :] <= rows[None, :, None]
        w = torch.softmax(sc.masked_fill(~vis, float("-inf")), -1)
        out[b, :rows.numel()] = torch.einsum("htn,hnd->thd", w, V.double())
    return _fill_illegal(case, out).reshape(B, T, Hq * D)


def restatement_f32(case, unit, round_p, requant=None):
    """The same attention in fp32, `unit` keys at a time with an online softmax; round_p: the
    probabilities rounded to the storage dtype as the P V operand (the prefill kernel; the decode
    head keeps them fp32).  Output rounded once to the dtype: [B, T, Hq D]."""
    B, T, Hq, D = case["B"], case["T"], case["Hq"], case["D"]
    dt = DTYPES[case["name"]]
    out = torch.zeros(B, T, Hq, D, dtype=torch.float32, device=case["q"].device)
    for b in range(B):
        if pfr.legal_rows(case, b) == 0:
            continue
        q, K, V, rows = _stream_operands(case, b, requant)
        q, K, V = q.float(), K.float(), V.float()
        n = rows.numel()
        m = torch.full((Hq, n), float("-inf"), device=q.device)
        l = torch.zeros((Hq, n), device=q.device)
        o = torch.zeros((Hq, n, D), device=q.device)
        for j0 in range(0, K.shape[1], unit):
            j1 = min(j0 + unit, K.shape[1])
            s = torch.einsum("htd,hnd->htn", q, K[:, j0:j1]) * case["scale"]
            vis = torch.arange(j0, j1, device=q.device)[None, None, :] <= rows[None, :, None]
            s = s.masked_fill(~vis, float("-inf"))
            mn = torch.maximum(m, s.amax(-1))
            alpha = torch.exp(m - mn)
            e = torch.exp(s - mn.unsqueeze(-1))
            l = l * alpha + e.sum(-1)
            if round_p:
                e = e.to(dt).float()
            o = o * alpha.unsqueeze(-1) + torch.einsum("htn,hnd->htd", e, V[:, j0:j1])
            m = mn
        out[b, :n] = (o / l.unsqueeze(-1)).transpose(0, 1)
    return _fill_illegal(case, out).reshape(B, T, Hq * D).to(dt)


def units_of_error(out, ref64, case):
    """|out - ref64| in spacings of the storage dtype at the row's largest |ref64| (a row: the D
    elements of one stream, token and head): [B, T, Hq, D], NaN rows and padding rows as 0."""
    B, T, Hq, D = case["B"], case["T"], case["Hq"], case["D"]
    dt = DTYPES[case["name"]]
    r = ref64.reshape(B, T, Hq, D)
    o = out.double().reshape(B, T, Hq, D)
    live = ~torch.isnan(r).any(-1, keepdim=True) & (r.abs().amax(-1, keepdim=True) > 0)
    unit = af.ulp_at(torch.nan_to_num(r).abs().amax(-1, keepdim=True), dt)
    return torch.where(live, (o - torch.nan_to_num(r)).abs() / unit, torch.zeros((), dtype=torch.float64, device=o.device))


def assert_fill(out, case, what):
    """Rows that are not computed: NaN where a real row has no slot, zeros where the row is padding."""
    fill = pfr.expected_fill(case)
    o = out.reshape(case["B"], case["T"], -1)
    for b in range(case["B"]):
        for i in range(case["T"]):
            if fill[b][i] == "nan":
                assert bool(torch.isnan(o[b, i]).all()), (what, b, i, "a real row without a slot is NaN")
            elif fill[b][i] == "zero":
                assert not bool(o[b, i].any()), (what, b, i, "a padding row is zero")
            else:
                assert not bool(torch.isnan(o[b, i]).any()), (what, b, i, "NaN in a computed row")


def chunk_partials(case, b, rows, unit):
    """The fp64 reference of rows `rows` (indices into stream b's computed rows) split by chunk of
    `unit` keys: (w [Hq, R, C, unit] the unnormalised weights, zero where a key is invisible,
    V [Hq, C, unit, D] zero-padded, keys [R, C] the visible keys of each chunk)."""
    q, K, V, pos_rows = _stream_operands(case, b)
    q, pos_rows = q[:, rows], pos_rows[rows]
    n = K.shape[1]
    C = -(-n // unit)
    sc = torch.einsum("htd,hnd->htn", q.double(), K.double()) * case["scale"]
    vis = torch.arange(n)[None, None, :] <= pos_rows[None, :, None]
    sc = sc.masked_fill(~vis, float("-inf"))
    w = torch.exp(sc - sc.amax(-1, keepdim=True))
    pad = C * unit - n
    w = torch.nn.functional.pad(w, (0, pad)).reshape(w.shape[0], w.shape[1], C, unit)
    Vp = torch.nn.functional.pad(V.double(), (0, 0, 0, pad)).reshape(V.shape[0], C, unit, V.shape[2])
    keys = torch.nn.functional.pad(vis[0].to(torch.int64), (0, pad)).reshape(-1, C, unit).sum(-1)
    return w, Vp, keys


def perturbed_outputs(w, Vp):
    """From chunk_partials: the reference (out [Hq, R, D]) and, for every chunk c, the output with the
    chunk dropped, summed twice, or read from chunk c + 1's place (the last from chunk c - 1's):
    each [Hq, R, C, D]."""
    l_c = w.sum(-1)                                            # [Hq, R, C]
    o_c = torch.einsum("hrcu,hcud->hrcd", w, Vp)
    Vn = torch.roll(Vp, -1, 1)
    if Vp.shape[1] > 1:
        Vn[:, -1] = Vp[:, -2]
    o_n = torch.einsum("hrcu,hcud->hrcd", w, Vn)
    Lsum, O = l_c.sum(-1)[..., None, None], o_c.sum(2, keepdim=True)
    out = (O / Lsum).squeeze(2)
    drop = (O - o_c) / (Lsum - l_c.unsqueeze(-1))
    dup = (O + o_c) / (Lsum + l_c.unsqueeze(-1))
    moved = (O - o_c + o_n) / Lsum
    return out, drop, dup, moved


def removal_sensitivity(case, b, rows, unit):
    """For the rows of stream b: by how many spacings of the storage dtype at the row's largest |value|
    the element that moves most moves when chunk c leaves the fp64 reference -- [Hq, R, C] -- and
    keys [R, C].  A row's only chunk (nothing left without it) counts as inf."""
    w, Vp, keys = chunk_partials(case, b, rows, unit)
    out, drop, _, _ = perturbed_outputs(w, Vp)
    spacing = af.ulp_at(out.abs().amax(-1), DTYPES[case["name"]])[..., None]
    move = (drop - out.unsqueeze(2)).abs().amax(-1) / spacing
    return torch.nan_to_num(move, nan=float("inf")), keys


# ---------------------------------------------------------------------------
# a weight of 2^32 codes, built on the device
# ---------------------------------------------------------------------------

BIG_ROWS, BIG_K = 524288, 8192        # 2^32 codes: 2 GiB packed
REF_ROWS = 16384                      # the reference dequantises at most this many rows at a time


def big_weight(device, blocksize=64, seed=0):
    """dict of device tensors: packed uint8 [BIG_ROWS * BIG_K / 2, 1] from randint, absmax fp32 in
    [0.5, 2) per block, and the double-quant statistics of the same blocks: qabsmax random bytes,
    absmax2 in [0.5, 2) per 256 blocks, offset in [0.5, 2), create_dynamic_map's code."""
    from quantizations_amd.core import create_dynamic_map

    g = torch.Generator(device=device).manual_seed(seed)
    nbytes = BIG_ROWS * BIG_K // 2
    packed = torch.empty((nbytes, 1), dtype=torch.uint8, device=device)
    step = 1 << 28
    for i in range(0, nbytes, step):    # randint's int64 intermediate: a quarter GiB of codes at a time
        packed[i:i + step, 0] = torch.randint(0, 256, (min(step, nbytes - i),), device=device, generator=g,
                                              dtype=torch.uint8)
    blocks = BIG_ROWS * BIG_K // blocksize
    absmax = torch.rand(blocks, device=device, generator=g) * 1.5 + 0.5
    qabsmax = torch.empty(blocks, dtype=torch.uint8, device=device)
    qabsmax[:] = torch.randint(0, 256, (blocks,), device=device, generator=g, dtype=torch.uint8)
    absmax2 = torch.rand(-(-blocks // 256), device=device, generator=g) * 1.5 + 0.5
    offset = (torch.rand((), device=device, generator=g) * 1.5 + 0.5).float()
    return dict(packed=packed, absmax=absmax, qabsmax=qabsmax, absmax2=absmax2, offset=offset,
                code2=create_dynamic_map().to(device), blocksize=blocksize, blocksize2=256)


def big_state(w, M, quant_type, nested, dtype):
    """A QuantState over the first M rows of big_weight's buffers, assembled by hand."""
    from quantizations_amd.core import QuantState, get_4bit_type

    dev = w["packed"].device
    code = get_4bit_type(quant_type, device=dev)
    blocks = M * BIG_K // w["blocksize"]
    if not nested:
        return QuantState(absmax=w["absmax"][:blocks], shape=torch.Size((M, BIG_K)), dtype=dtype,
                          blocksize=w["blocksize"], code=code, quant_type=quant_type)
    st2 = QuantState(absmax=w["absmax2"][:-(-blocks // 256)], code=w["code2"], blocksize=256, dtype=torch.float32)
    return QuantState(absmax=w["qabsmax"][:blocks], shape=torch.Size((M, BIG_K)), dtype=dtype, blocksize=w["blocksize"],
                      code=code, quant_type=quant_type, offset=w["offset"], state2=st2)


def chunk_slices(r0, r1, K, blocksize, blocksize2=256):
    """Rows [r0, r1) of a row-major 4-bit weight with K % blocksize == 0 and K even: (first packed
    byte, end byte, first block, end block, first double-quant group, end group).  Python integers
    throughout: nothing here is 32 bits wide."""
    assert K % blocksize == 0 and K % 2 == 0 and 0 <= r0 <= r1
    b0, b1 = r0 * K // blocksize, r1 * K // blocksize
    return r0 * K // 2, r1 * K // 2, b0, b1, b0 // blocksize2, -(-b1 // blocksize2)


def dequantize_rows(w, r0, r1, code, nested):
    """Rows [r0, r1) of big_weight dequantised in plain torch: codebook lookup x scale as an fp32
    product, [r1 - r0, K] fp32 (the high nibble of a byte is the even element)."""
    assert r1 - r0 <= REF_ROWS
    y0, y1, b0, b1, g0, _ = chunk_slices(r0, r1, BIG_K, w["blocksize"], w["blocksize2"])
    by = w["packed"][y0:y1, 0].long()
    idx = torch.stack((by >> 4, by & 15), -1).reshape(-1)
    if nested:
        grp = torch.arange(b0, b1, device=by.device) // w["blocksize2"]
        scale = w["code2"][w["qabsmax"][b0:b1].long()] * w["absmax2"][grp] + w["offset"]
    else:
        scale = w["absmax"][b0:b1]
    vals = code[idx].reshape(b1 - b0, w["blocksize"]) * scale.unsqueeze(-1)
    return vals.reshape(r1 - r0, BIG_K)


def dequantize_row_list(w, rows, code, nested):
    """dequantize_rows for a list of rows (boundary_rows): [len(rows), K] fp32.  Row and block indices
    are int64 tensors: a block index may pass 2^31."""
    dev = w["packed"].device
    r = torch.as_tensor(rows, dtype=torch.int64, device=dev)
    bpr = BIG_K // w["blocksize"]
    by = w["packed"].view(-1, BIG_K // 2)[r].long()
    idx = torch.stack((by >> 4, by & 15), -1).reshape(r.numel(), BIG_K)
    blk = r[:, None] * bpr + torch.arange(bpr, device=dev)[None, :]
    if nested:
        scale = w["code2"][w["qabsmax"][blk].long()] * w["absmax2"][blk // w["blocksize2"]] + w["offset"]
    else:
        scale = w["absmax"][blk]
    return (code[idx].reshape(r.numel(), bpr, w["blocksize"]) * scale.unsqueeze(-1)).reshape(r.numel(), BIG_K)


def boundary_rows(M, K, seed=0):
    """Sorted unique rows of an [M, K] 4-bit weight: the first and the last 64, the 64 around each row
    r where r * K crosses 2^31 or 2^32 (elements) or r * K / 2 does (bytes), and 4096 seeded random ones."""
    rows = set(range(min(64, M))) | set(range(max(0, M - 64), M))
    for bound in (1 << 31, 1 << 32):
        for per_row in (K, K / 2):
            r = int(bound // per_row)
            rows |= {x for x in range(r - 32, r + 32) if 0 <= x < M}
    g = torch.Generator().manual_seed(seed)
    rows |= set(torch.randint(0, M, (4096,), generator=g).tolist())
    return sorted(rows)
