"""numpy restatement of qz_token_logprobs / qz_logprobs_streams (include/quantizations.h states the
rules), on raw 16-bit patterns: `reference` in float64 (the bars are measured against it, rounded to
float32), `restatement32` in float32 with np.exp / np.log and a left-to-right sum per chunk of 2048 (the CPU
proof that the bars are not missed by fp32 arithmetic), and the logits families both are run over.

The bars.  |got - ref32| <= LP_ABS + LP_REL * |ref32| on every finite entry, ref32 = the float64
reference rounded to float32.  They are twice the worst error of restatement32 over every case of
`cases` for both dtypes, measured as: REL = the largest err / |ref32| among the entries with
|ref32| >= 1, ABS = the largest err among the entries with |ref32| < 1 (every entry meets one of the
two, hence their sum).  Measured (numpy 2.x, x86-64): REL 2.725e-06, ABS 7.794e-06 -- the rounding
of the sum of exponentials, which every entry of a row shares through log S.
tests/test_logprobs_cpu.py asserts that the restatement stays inside HALF of the bars below, so
these constants cannot sink below what fp32 arithmetic needs."""
import functools

import numpy as np

F16, BF16 = "fp16", "bf16"
MAX_TOP = 20
CHUNK = 2048

MEASURED_ABS, MEASURED_REL = 7.794e-06, 2.725e-06
LP_ABS, LP_REL = 2 * MEASURED_ABS, 2 * MEASURED_REL


def to_f64(bits, name):
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    with np.errstate(invalid="ignore"):      # signalling NaN patterns
        if name == F16:
            return bits.view(np.float16).astype(np.float64)
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def to_bits(x, name):
    """float array -> the dtype's patterns (round to nearest even; fp16 through numpy, bf16 by hand)."""
    x = np.asarray(x, dtype=np.float32)
    if name == F16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def _bad(x):
    return np.isnan(x).any(-1) | (x == np.inf).any(-1) | (x.max(-1) == -np.inf)


def _all_lp(x, dtype):
    """log-softmax of every element of the rows x (float64 values), evaluated in `dtype`."""
    x = x.astype(dtype)
    with np.errstate(all="ignore"):
        m = x.max(-1, keepdims=True)
        d = (x - m).astype(dtype)
        e = np.exp(d, dtype=dtype)
        if dtype == np.float32:      # chunks of 2048 left to right, then the chunks' sums left to right
            pad = (-e.shape[-1]) % CHUNK
            ec = np.concatenate([e, np.zeros(e.shape[:-1] + (pad,), dtype)], -1).reshape(e.shape[:-1] + (-1, CHUNK))
            s = np.cumsum(np.cumsum(ec, axis=-1, dtype=dtype)[..., -1], axis=-1, dtype=dtype)[..., -1:]
        else:
            s = e.sum(-1, keepdims=True)
        lp = (d - np.log(s, dtype=dtype)).astype(dtype)
    lp[_bad(x.astype(np.float64))] = np.nan
    return lp


def _pick(bits, name, ids, n, dtype):
    x = to_f64(bits, name)
    R, V = x.shape
    with np.errstate(over="ignore"):
        lp_all = _all_lp(x, dtype).astype(np.float32)             # float64 -> float32: beyond the range is -inf
    bad = _bad(x)
    ids = np.asarray(ids, dtype=np.int64)
    inside = (ids >= 0) & (ids < V)
    lp = np.where(inside, lp_all[np.arange(R), np.clip(ids, 0, V - 1)], np.float32(np.nan)).astype(np.float32)
    top_id = np.full((R, n), -1, np.int32)
    top_lp = np.full((R, n), -np.inf, np.float32)
    k = min(n, V)
    if k:
        order = np.argsort(-x, axis=-1, kind="stable")[:, :k]     # value descending, index ascending; -0 == +0
        top_id[:, :k] = order
        top_lp[:, :k] = np.take_along_axis(lp_all, order, -1)
    top_id[bad] = -1
    top_lp[bad] = np.nan
    return lp, top_id, top_lp


def reference(bits, name, ids, n):
    """(lp float32 [R], top_id int32 [R, n], top_lp float32 [R, n]): float64, rounded to float32."""
    return _pick(bits, name, ids, n, np.float64)


def restatement32(bits, name, ids, n):
    return _pick(bits, name, ids, n, np.float32)


def streams_reference(bits, name, seq, pos0, pos1, T, n, lp_tab, top_id_tab, top_lp_tab):
    """qz_logprobs_streams on numpy tables, in place: only live rows write."""
    B, L = seq.shape
    lp, ti, tl = reference(bits, name, np.zeros(bits.shape[0], np.int64), n)
    for b in range(B):
        p0 = int(pos0[b if len(pos0) > 1 else 0])
        p1 = int(pos1[b if len(pos1) > 1 else 0])
        for i in range(T):
            c = p0 + 1 + i
            if not (0 <= c <= p1 and c < L):
                continue
            r = b * T + i
            lp_tab[b, c] = reference(bits[r:r + 1], name, seq[b, c:c + 1], 0)[0][0]
            if n:
                top_id_tab[b, c], top_lp_tab[b, c] = ti[r], tl[r]


def errors(got, ref):
    """(err, |ref|) over the entries where both are finite; the classes must agree everywhere else."""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    fin = np.isfinite(ref)
    same_class = np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)],
                                                                                 ref[~fin & ~np.isnan(ref)])
    assert same_class and np.isfinite(got[fin]).all(), "non-finite entries differ in class or position"
    return np.abs(got[fin] - ref[fin]), np.abs(ref[fin])


def within(got, ref, scale=1.0):
    err, mag = errors(got, ref)
    return bool((err <= scale * (LP_ABS + LP_REL * mag)).all()), (float(err.max()) if err.size else 0.0)


# ---------------------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------------------

def _randn_bits(rng, name, R, V, scale=4.0):
    return to_bits(rng.standard_normal((R, V)) * scale, name)


def _ids(rng, R, V):
    ids = rng.integers(0, V, R)
    ids[0] = 0
    ids[-1] = V - 1
    return ids.astype(np.int64)


def _all16(name):
    p = np.arange(65536, dtype=np.uint16)
    return np.where(np.isfinite(to_f64(p, name)), p, np.uint16(0))[None, :]


@functools.lru_cache(maxsize=None)
def cases(name, big=True):
    """[(label, bits uint16 [R, V], ids int64 [R])]: every family of the issue at the smallest shapes
    that still cross a chunk boundary; `big` adds the V = 128256 row and the all-patterns row."""
    rng = np.random.default_rng(1234 if name == F16 else 4321)
    n = MAX_TOP
    out = []
    for V, R in ((1, 3), (5, 3), (2047, 3), (2048, 3), (2049, 16), (2 * CHUNK + 37, 1), (2 * CHUNK + 37, 3)):
        out.append((f"randn4 V={V} R={R}", _randn_bits(rng, name, R, V), _ids(rng, R, V)))
    V = 2 * CHUNK + 37
    hot = np.full((1, V), -6e4, np.float32)
    hot[0, CHUNK + 2] = 6e4
    out.append(("one hot 6e4 over -6e4", to_bits(hot, name), np.array([CHUNK + 2], np.int64)))
    out.append(("one hot, a cold token", to_bits(hot, name), np.array([7], np.int64)))
    for Vf in (CHUNK, V):
        out.append((f"flat V={Vf}", to_bits(np.full((1, Vf), 1.5, np.float32), name), np.array([Vf - 1], np.int64)))
    x = rng.standard_normal((2, V)).astype(np.float32)
    x[0, CHUNK - n // 2:CHUNK + n // 2] = 12.0 - 0.25 * ((np.arange(n) * 7) % n)       # the top n straddle 2048
    x[1, 2 * CHUNK + 5:2 * CHUNK + 5 + n] = 12.0 - 0.25 * ((np.arange(n) * 3) % n)     # all in the partial chunk
    out.append(("top n across a boundary / in the partial chunk", to_bits(x, name),
                np.array([CHUNK, 2 * CHUNK + 5], np.int64)))
    x = rng.standard_normal((1, V)).astype(np.float32)
    x[0, ::179][:n + 3] = 9.0                                                          # n + 3 equal maxima
    out.append(("n + 3 equal maxima over the chunks", to_bits(x, name), np.array([179 * (n + 2)], np.int64)))
    sub = rng.integers(1, 128 if name == BF16 else 1024, (2, CHUNK + 1)).astype(np.uint16)
    sub |= (rng.integers(0, 2, sub.shape).astype(np.uint16) << 15)
    sub[1, :40] &= 0x8000                                                              # -0 and +0 tie by index
    out.append(("subnormal logits and signed zeros", sub, np.array([0, CHUNK], np.int64)))
    holes = _randn_bits(rng, name, 3, CHUNK + 1)
    ninf = np.uint16(0xFC00 if name == F16 else 0xFF80)
    holes[0][rng.random(CHUNK + 1) < 0.3] = ninf
    holes[1, 3:] = ninf                                                                # three finite logits: the lists hold -inf
    holes[2, :CHUNK] = ninf                                                            # a chunk of nothing but -inf
    out.append(("-inf holes", holes, np.array([int(np.argmax(holes[0] == ninf)), 5, CHUNK], np.int64)))
    x = _randn_bits(rng, name, 5, CHUNK + 1)
    low = int(np.argmin(to_f64(x[3], name)))
    out.append(("ids at 0, V - 1, outside and below the lists", x,
                np.array([0, CHUNK, -1, low, 1 << 40], np.int64)))
    if name == BF16:
        x = np.clip(rng.standard_normal((2, CHUNK + 1)) * 1e38, -3e38, 3e38).astype(np.float32)
        x[0, 5], x[0, 6], x[1, CHUNK] = 3e38, -3e38, 3e38
        out.append(("bf16 at 3e38", to_bits(x, name), np.array([6, 0], np.int64)))
    if big:
        out.append(("randn4 V=128256", _randn_bits(rng, name, 1, 128256), np.array([128255], np.int64)))
        out.append(("every finite pattern once", _all16(name), np.array([0x3C00], np.int64)))
    return out


@functools.lru_cache(maxsize=None)
def nonfinite_cases(name):
    """Rows whose class is NaN throughout (a NaN, a +inf, nothing but -inf) between finite rows."""
    rng = np.random.default_rng(99)
    V = CHUNK + 1
    x = _randn_bits(rng, name, 6, V)
    nan, pinf, ninf = ((0x7E00, 0x7C00, 0xFC00) if name == F16 else (0x7FC0, 0x7F80, 0xFF80))
    x[1, CHUNK] = nan
    x[2, 17] = pinf
    x[3, :] = ninf
    x[4, 100] = nan | 0x8001          # a negative NaN with a payload
    x[4, 101] = ninf
    return [("non-finite rows", x, np.array([0, 1, 2, 3, 4, 5], np.int64))]


@functools.lru_cache(maxsize=None)
def expected(name, big=True, nonfinite=False):
    """The float64 reference of every case at n = MAX_TOP (a smaller n is a prefix of the lists)."""
    src = nonfinite_cases(name) if nonfinite else cases(name, big)
    return [reference(bits, name, ids, MAX_TOP) for _, bits, ids in src]
