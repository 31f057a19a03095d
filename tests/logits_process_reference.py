"""qz_logits_process' rules (include/quantizations.h) restated in numpy float32, on the raw 16-bit
patterns of the logits: what the kernel, layer_ops' composed route and the sessions are compared with.

A row's history h is a list of Python integers.  For every distinct token of h inside [0, V), once:
x = the stored logit as float32; rp != 1: y = x * rp if x < 0 else x / rp; a token with c_gen > 0
occurrences at indices >= prompt_len: y = y - fp * float32(c_gen), then y = y - pp; every operation
one float32 rounding; y rounded once (nearest, ties to even) to the storage format.  A NaN logit keeps
its bits; a NaN that the arithmetic makes of numbers is stored as the quiet NaN 0x7E00 / 0x7FC0.  Then
the no-repeat n-gram bans, then the minimum length's EOS ban: -inf, which wins over a penalty.
"""
import numpy as np

F16, BF16 = "fp16", "bf16"
NEG_INF = {F16: 0xFC00, BF16: 0xFF80}
QUIET_NAN = {F16: 0x7E00, BF16: 0x7FC0}


def to_f32(bits, dt):
    """uint16 patterns -> float32 (exact)."""
    bits = np.asarray(bits, dtype=np.uint16)
    if dt == F16:
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def from_f32(y, dt):
    """float32 -> uint16 patterns, one round-to-nearest-even; NaN -> the quiet NaN."""
    y = np.asarray(y, dtype=np.float32)
    nan = np.isnan(y)
    with np.errstate(over="ignore", invalid="ignore"):
        if dt == F16:
            out = np.where(nan, np.float32(0), y).astype(np.float16).view(np.uint16)
        else:
            u = np.where(nan, np.float32(0), y).view(np.uint32).astype(np.uint64)
            out = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(nan, np.uint16(QUIET_NAN[dt]), out).astype(np.uint16)


def penalise(bits, dt, c_gen, rp=1.0, pp=0.0, fp=0.0):
    """Step 1 on the patterns `bits` of tokens that occur in the history, c_gen their generated counts."""
    bits = np.asarray(bits, dtype=np.uint16)
    x = to_f32(bits, dt)
    rp, pp, fp = np.float32(rp), np.float32(pp), np.float32(fp)
    c = np.asarray(c_gen, dtype=np.int64)
    with np.errstate(all="ignore"):
        y = np.where(x < 0, x * rp, x / rp).astype(np.float32) if rp != np.float32(1) else x
        t = (fp * c.astype(np.float32)).astype(np.float32)
        y = np.where(c > 0, ((y - t).astype(np.float32) - pp).astype(np.float32), y)
    return np.where(np.isnan(x), bits, from_f32(y, dt)).astype(np.uint16)


def banned_ngram_tokens(h, g):
    """Step 2: the tokens that would complete an n-gram of size g already in h."""
    n = len(h)
    if g < 1 or g > n:
        return set()
    tail = list(h[n - g + 1:])
    return {h[k + g - 1] for k in range(n - g + 1) if list(h[k:k + g - 1]) == tail}


def process_row(bits, dt, V, h, *, rp=1.0, pp=0.0, fp=0.0, ngram=0, min_new=0, prompt_len=0, eos=-1):
    """One row: bits uint16 [>= V] (a copy is returned; elements past V are never touched)."""
    out = np.array(bits, dtype=np.uint16, copy=True)
    h = [int(t) for t in h]
    n = len(h)
    neutral_pen = np.float32(rp) == 1 and np.float32(pp) == 0 and np.float32(fp) == 0
    if not neutral_pen:
        cnt = {}
        for k, t in enumerate(h):
            if 0 <= t < V:
                cnt[t] = cnt.get(t, 0) + (1 if k >= prompt_len else 0)
        if cnt:
            ids = np.fromiter(cnt.keys(), dtype=np.int64)
            out[ids] = penalise(out[ids], dt, np.fromiter(cnt.values(), dtype=np.int64), rp, pp, fp)
    for t in banned_ngram_tokens(h, int(ngram)):
        if 0 <= t < V:
            out[t] = NEG_INF[dt]
    if min_new > 0 and 0 <= eos < V and n - prompt_len < min_new:
        out[eos] = NEG_INF[dt]
    return out


def process(bits, dt, V, hist, pos, tok=None, *, rp=None, pp=None, fp=None, ngram=None, min_new=None, prompt_len=None,
            eos=None):
    """The whole window: bits uint16 [B*T, row]; hist [B, H]; pos [1] or [B]; tok [B, T] or None (T = 1);
    per-stream sequences or None (off for everyone).  Returns the processed copy."""
    out = np.array(bits, dtype=np.uint16, copy=True)
    hist = np.asarray(hist)
    B, H = hist.shape
    T = 1 if tok is None else np.asarray(tok).reshape(B, -1).shape[1]
    tok = None if tok is None else np.asarray(tok).reshape(B, T)
    pos = np.asarray(pos).reshape(-1)
    for b in range(B):
        p = int(pos[b if len(pos) > 1 else 0])
        if not 0 <= p < H:
            continue
        for i in range(T):
            h = hist[b, :p + 1].tolist() + (tok[b, 1:i + 1].tolist() if i else [])
            out[b * T + i] = process_row(
                out[b * T + i], dt, V, h,
                rp=1.0 if rp is None else rp[b], pp=0.0 if pp is None else pp[b], fp=0.0 if fp is None else fp[b],
                ngram=0 if ngram is None else int(ngram[b]),
                min_new=0 if (min_new is None or eos is None) else int(min_new[b]),
                prompt_len=0 if prompt_len is None else int(prompt_len[b]), eos=-1 if eos is None else int(eos[b]))
    return out
