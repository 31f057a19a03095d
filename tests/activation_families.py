"""Test-only activation families that reach the edges `randn * (1..4)` never does, for the kernels
around the 4-bit projections (RMSNorm, rotary, SiLU, decode attention, the dense lm_head GEMV and
the activations of the 4-bit GEMVs).  Everything is deterministic from a seed and built with numpy /
torch on the CPU; tests/test_activation_families.py proves on the CPU alone that each family reaches
its edge and that a plain fp32 restatement stays inside half of every bar the GPU tests assert;
tests/test_gpu_activation_range.py hands the families to the HIP kernels.

Vectors (name = "fp16" | "bf16" | "fp32"; shape's last dimension is the row):
  all16(name)             every one of the 65536 bit patterns of the 16-bit format, finite and not
  outlier(name, shape)    N(0, 1e-6) with four elements per row at +-(3e4 .. 6e4)
  sub16(name, shape)      every value a subnormal of the 16-bit format (fp32: of fp16), both signs,
                          the smallest and the largest included
  tiny32 / huge32         magnitudes near 1e-30 (squares underflow to 0 in fp32) and 1e20 .. 1e30
                          (squares overflow to inf); bf16 and fp32
  mixed(name, K)          32-element chunks of outlier values, of subnormals, of both interleaved,
                          and all-zero chunks
  cancel(name, M, K)      (x, W): products in pairs of opposite sign, the result ~1e-3 of sum |w x|
  overflow_add(name, K)   (x, r) [2, K]: row 0 sums to exact halfway cases of the format (finite), row
                          1 also overflows to +-inf, at the halfway case below inf among others
  nonfinite(name, K)      [4, K]: +inf / -inf / NaN / all three planted in N(0, 9) rows

Attention cases (attention_case): dicts of q, k, v, cos, sin, the caches, one position per stream,
the visibility of every key and the softmax scale; see the builder of each family below.  Every one
keeps sum_d |q_d k_d| * scale <= 64 (SCORE_BOUND), so fp32 scores resolve the weights.
"""
from __future__ import annotations

import math

import numpy as np
import torch

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
SUB_ULP = {"fp16": 2.0 ** -24, "bf16": 2.0 ** -133, "fp32": 2.0 ** -24}   # spacing of the subnormals
SUB_MAX = {"fp16": 1023, "bf16": 127, "fp32": 1023}                       # the largest, in spacings
MANT = {"fp16": 11, "bf16": 8}                                            # significand bits
CHUNK = 128                    # key positions per attention workgroup (layer_ops.ATTN_CHUNK)
SCORE_BOUND = 64.0
ATTENTION_FAMILIES = ("census", "sink", "late_peak", "gap", "big_v", "sub16", "sub16_q", "dirty_mask")


def _to(a64, dtype: torch.dtype) -> torch.Tensor:
    """float64 -> dtype, one rounding, clamped to the dtype's finite maximum first."""
    mx = torch.finfo(dtype).max
    return torch.from_numpy(np.clip(np.asarray(a64, np.float64), -mx, mx)).to(dtype)


def _shape(shape):
    return (shape,) if isinstance(shape, int) else tuple(shape)


# ---------------------------------------------------------------------------
# vectors
# ---------------------------------------------------------------------------

def all16(name: str) -> torch.Tensor:
    bits = np.arange(1 << 16, dtype=np.uint16)
    return torch.from_numpy(bits.view(np.int16).copy()).view(DTYPES[name])


def outlier(name: str, shape, seed: int = 0, n_out: int = 4) -> torch.Tensor:
    shape = _shape(shape)
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 1e-3).reshape(-1, shape[-1])
    for row in x:
        idx = rng.choice(shape[-1], n_out, replace=False)
        row[idx] = rng.uniform(3e4, 6e4, n_out) * rng.choice([-1.0, 1.0], n_out)
    return _to(x.reshape(shape), DTYPES[name])


def sub16(name: str, shape, seed: int = 1) -> torch.Tensor:
    shape = _shape(shape)
    rng = np.random.default_rng(seed)
    k = rng.integers(1, SUB_MAX[name] + 1, shape).astype(np.float64) * rng.choice([-1.0, 1.0], shape)
    flat = k.reshape(-1)
    flat[:4] = [1, SUB_MAX[name], -1, -SUB_MAX[name]]
    return _to(k * SUB_ULP[name], DTYPES[name])


def tiny32(name: str, shape, seed: int = 2) -> torch.Tensor:
    shape = _shape(shape)
    rng = np.random.default_rng(seed)
    x = (0.5 + np.abs(rng.standard_normal(shape))) * 1e-30 * rng.choice([-1.0, 1.0], shape)
    return _to(x, DTYPES[name])


def huge32(name: str, shape, seed: int = 3) -> torch.Tensor:
    shape = _shape(shape)
    rng = np.random.default_rng(seed)
    x = 10.0 ** rng.uniform(20, 30, shape) * rng.choice([-1.0, 1.0], shape)
    return _to(x, DTYPES[name])


def mixed(name: str, K: int, seed: int = 4) -> torch.Tensor:
    """Chunks of 32 (what one lane of a 4-bit GEMV takes per step), cycling: outlier values (the first
    of every chunk at +-3e4 and above), subnormals, the two interleaved element by element, all zero."""
    assert K % 128 == 0
    big = outlier(name, K, seed).double().numpy().reshape(-1, 32)
    big[:, 0] = (3e4 + 64.0 * np.arange(K // 32)) * np.where(np.arange(K // 32) % 3 == 0, -1.0, 1.0)
    sub = sub16(name, K, seed + 1).double().numpy().reshape(-1, 32)
    both = big.copy()
    both[:, 1::2] = sub[:, 1::2]
    kind = np.arange(K // 32) % 4
    x = np.where(kind[:, None] == 0, big, np.where(kind[:, None] == 1, sub, np.where(kind[:, None] == 2, both, 0.0)))
    return _to(x.reshape(K), DTYPES[name])


def cancel(name: str, M: int, K: int, seed: int = 5):
    """(x [K], W [M, K]): 7 / 8 of the columns come in pairs (i, partner) a random distance apart with
    W[:, partner] = W[:, i] and x[partner] = -x[i] (N(0, 1 / 16) x N(0, 4e-4)), the rest is N(0, 2.5e-3) x
    N(0, 4e-4): the result is of the order of a thousandth of sum |w x|.  (Pairs any larger put the
    difference of two fp32 summation orders above one fp16 ulp of the result, and the dense GEMV is
    also held to 2 ulp of F.linear, another fp32 order: test_activation_families measures it.)"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(K)
    npair = K * 7 // 16
    a, b, rest = perm[:npair], perm[npair:2 * npair], perm[2 * npair:]
    x = rng.standard_normal(K) * 0.25
    W = rng.standard_normal((M, K)) * 0.02
    x[b] = -x[a]
    W[:, b] = W[:, a]
    x[rest] = rng.standard_normal(len(rest)) * 0.05
    return _to(x, DTYPES[name]), _to(W, DTYPES[name])


def overflow_add(name: str, K: int, seed: int = 6):
    """(x, r), each [2, K] of a 16-bit format.  Every third element of both rows: x an even integer of
    [2^p, 2^(p+1)) (p = significand bits, spacing 2) and r = 1, both with one sign -- an odd sum, the
    exact halfway case, lower neighbour even and odd in turn.  Row 0 also holds max + (just below half
    a spacing), which stays max; row 1 max + half a spacing (the halfway case below inf: rounds to inf),
    max + max and their negatives."""
    dt = DTYPES[name]
    p = MANT[name]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, K)) * 3.0
    r = rng.standard_normal((2, K)) * 3.0
    n3 = len(range(0, K, 3))
    ev = (2.0 ** p + 2.0 * (np.arange(n3) % (2 ** (p - 1)))) * np.where(np.arange(n3) % 5 < 2, -1.0, 1.0)
    x[:, ::3] = ev
    r[:, ::3] = np.sign(ev)
    mx = float(torch.finfo(dt).max)
    half = 2.0 ** (math.floor(math.log2(mx)) - p)           # half the spacing at max
    below = half * (1.0 - 2.0 ** -p)                        # the 16-bit value next below `half`
    x[0, 1], r[0, 1] = mx, below
    x[0, 4], r[0, 4] = -mx, -below
    for i, (a, b) in enumerate([(mx, half), (-mx, -half), (mx, mx), (-mx, -mx), (half, mx), (mx, below)]):
        x[1, 1 + 3 * i], r[1, 1 + 3 * i] = a, b
    x, r = _to(x, dt), _to(r, dt)
    assert float(r[0, 1]) == below and float(r[1, 1]) == half
    return x, r


def nonfinite(name: str, K: int, seed: int = 7) -> torch.Tensor:
    rng = np.random.default_rng(seed)
    x = _to(rng.standard_normal((4, K)) * 3.0, DTYPES[name])
    inf, nan = float("inf"), float("nan")
    x[0, 5] = inf
    x[1, K // 2] = -inf
    x[2, K - 1] = nan
    x[3, 1], x[3, K // 3], x[3, K - 2] = inf, -inf, nan
    return x


# ---------------------------------------------------------------------------
# attention cases
# ---------------------------------------------------------------------------

def _dirt(shape, rng):
    """NaN, +inf, -inf cycling by row."""
    n = int(np.prod(shape[:-1]))
    vals = np.array([float("nan"), float("inf"), float("-inf")])[(np.arange(n) + rng.integers(3)) % 3]
    return np.broadcast_to(vals.reshape(*shape[:-1], 1), shape).copy()


def attention_case(family: str, name: str, Hq: int, Hkv: int, D: int, L: int, ps, seed: int = 0,
                   holes: bool = False) -> dict:
    """One stream per position of `ps`.  Returns q [B, 1, Hq D], k / v [B, 1, Hkv D], cos / sin
    [B, 1, D], kc / vc [B, Hkv, L, D] (the caches BEFORE the call: slot p and every row that is not
    visible hold NaN, `dirty_mask`: NaN / +-inf), pos (list), visible bool [B, L] (j <= p, minus the
    holes; p itself always), scale, and per family: `expected` [B, Hq D] float64 (census), `dominant`
    [B] key index whose v row the output must equal (sink, late_peak).

    census     q = 0, v[j] one-hot at j % D: output element d = (visible j with j % D == d) / visible
    sink       key 3 scores +55, every other about -55 (q = a s, k = +-a s, a^2 D scale = 55)
    late_peak  the same with the new token (j == p) the one at +55
    gap        chunk c's best key scores (50, -42, -38, -45, 48)[c % 5], the others up to 8 below
    big_v      v = +-(6e4 - 32 i), sign (-1)^(j + d), scores of order one
    sub16      q, k, v subnormal (fp16 only: a product of two bf16 subnormals is below fp32), scale 2^34 / D
    sub16_q    q and v subnormal, k near +-1e4, scale the power of two that keeps the bound
    dirty_mask N(0, 1) q, k, v, ordinary angles, NaN / +-inf where not visible (use holes=True)
    """
    assert family in ATTENTION_FAMILIES
    dt = DTYPES[name]
    rng = np.random.default_rng(seed + 1000 * ATTENTION_FAMILIES.index(family))
    B = len(ps)
    G = Hq // Hkv
    scale = 1.0 / math.sqrt(D)
    j_all = np.arange(L)
    visible = j_all[None, :] <= np.asarray(ps)[:, None]
    if holes:
        visible &= rng.random((B, L)) > 0.3
        visible[np.arange(B), ps] = True
    cos, sin = np.ones((B, 1, D)), np.zeros((B, 1, D))
    q = np.zeros((B, Hq, D))
    k = rng.standard_normal((B, Hkv, D))
    v = rng.standard_normal((B, Hkv, D))
    kc = rng.standard_normal((B, Hkv, L, D))
    vc = rng.standard_normal((B, Hkv, L, D))
    extra = {}
    a = math.sqrt(55.0 / (D * scale))
    sgn = rng.choice([-1.0, 1.0], D)

    def keys_scoring(score, noise):
        """k rows with q . k * scale = score (up to the noise and the format's rounding), q = a * sgn."""
        score = np.asarray(score, np.float64)
        return (score[..., None] / 55.0) * a * sgn * (1.0 + noise * rng.standard_normal(score.shape + (D,)))

    if family == "census":
        vc = np.zeros((B, Hkv, L, D))
        vc[:, :, j_all, j_all % D] = 1.0
        v = np.zeros((B, Hkv, D))
        v[np.arange(B), :, np.asarray(ps) % D] = 1.0
        cnt = np.stack([np.bincount(j_all[visible[b]] % D, minlength=D) for b in range(B)]).astype(np.float64)
        extra["expected"] = np.tile(cnt / visible.sum(1, keepdims=True), (1, Hq))
    elif family in ("sink", "late_peak"):
        q[:] = a * sgn
        kc = keys_scoring(np.full((B, Hkv, L), -55.0), 0.05)
        k = keys_scoring(np.full((B, Hkv), -55.0), 0.05)
        if family == "sink":
            assert min(ps) > 3
            kc[:, :, 3] = a * sgn
            visible[:, 3] = True
            extra["dominant"] = [3] * B
        else:
            k[:] = a * sgn
            extra["dominant"] = list(ps)
    elif family == "gap":
        q[:] = a * sgn
        top = np.array([50.0, -42.0, -38.0, -45.0, 48.0])[(j_all // CHUNK) % 5]
        sc = np.broadcast_to(top - rng.uniform(0.5, 8.0, (B, Hkv, L)), (B, Hkv, L)).copy()
        sc[:, :, 7::CHUNK] = top[7::CHUNK]                                  # every chunk's best key
        kc = keys_scoring(sc, 0.02)
        k = keys_scoring(sc[np.arange(B), :, ps], 0.02)
    elif family == "big_v":
        q = rng.standard_normal((B, Hq, D)) * 0.5
        big = lambda shape, j: ((6e4 - 32.0 * rng.integers(0, 64, shape))                    # noqa: E731
                                * np.where((j + np.arange(D)) % 2 == 0, 1.0, -1.0))
        vc = big((B, Hkv, L, D), j_all[:, None])
        v = big((B, Hkv, D), np.asarray(ps)[:, None, None])
    elif family in ("sub16", "sub16_q"):
        ulp, smax = SUB_ULP[name], SUB_MAX[name]
        sub = lambda shape: rng.integers(1, smax + 1, shape) * rng.choice([-1.0, 1.0], shape) * ulp   # noqa: E731
        q, v, vc = sub((B, Hq, D)), sub((B, Hkv, D)), sub((B, Hkv, L, D))
        q[0, 0, :2], v[0, 0, :2] = [ulp, -smax * ulp], [smax * ulp, -ulp]
        if family == "sub16":
            assert name == "fp16"
            k, kc = sub((B, Hkv, D)), sub((B, Hkv, L, D))
            scale = 2.0 ** 34 / D            # D * 1023^2 * 2^-48 * scale < 64
        else:
            big = lambda shape: 1e4 * (1.0 + 0.1 * rng.standard_normal(shape)) * rng.choice([-1.0, 1.0], shape)   # noqa: E731
            k, kc = big((B, Hkv, D)), big((B, Hkv, L, D))
            scale = 2.0 ** math.floor(math.log2(SCORE_BOUND / (D * smax * ulp * 1.6e4)))
    elif family == "dirty_mask":
        q = rng.standard_normal((B, Hq, D))
        ang = rng.random((B, 1, D // 2)) * 6.0
        cos, sin = np.concatenate((np.cos(ang),) * 2, -1), np.concatenate((np.sin(ang),) * 2, -1)

    hidden = np.broadcast_to(~visible[:, None, :, None], kc.shape).copy()
    hidden[np.arange(B), :, ps] = True                        # slot p is written by the call
    dirt = _dirt(kc.shape, rng) if family == "dirty_mask" else np.full(kc.shape, float("nan"))
    kc, vc = np.where(hidden, dirt, kc), np.where(hidden, dirt, vc)
    t = lambda x, shape: _to(x, dt).reshape(shape)            # noqa: E731  (keeps NaN, clips inf: see below)
    case = dict(family=family, name=name, Hq=Hq, Hkv=Hkv, D=D, L=L, G=G, pos=list(ps), scale=scale,
                visible=torch.from_numpy(visible),
                q=t(q, (B, 1, Hq * D)), k=t(k, (B, 1, Hkv * D)), v=t(v, (B, 1, Hkv * D)),
                cos=t(cos, (B, 1, D)), sin=t(sin, (B, 1, D)), kc=t(kc, kc.shape), vc=t(vc, vc.shape), **extra)
    if family == "dirty_mask":                                # np.clip turned +-inf into +-max: put them back
        inf_rows = torch.from_numpy(hidden & np.isinf(dirt))
        for c in ("kc", "vc"):
            case[c] = torch.where(inf_rows, torch.from_numpy(dirt).to(dt), case[c])
    return case


def _rotate_half(x):
    x1, x2 = x[..., : x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


def rotated(case):
    """(q [B, Hq, D], k [B, Hkv, D]) after apply_rotary_pos_emb, torch's own per-op rounding in the dtype."""
    B, D = len(case["pos"]), case["D"]
    qh, kh = case["q"].view(B, case["Hq"], D), case["k"].view(B, case["Hkv"], D)
    c, s = case["cos"], case["sin"]
    return (qh * c) + (_rotate_half(qh) * s), (kh * c) + (_rotate_half(kh) * s)


def updated_caches(case):
    """The caches after the call: slot p_b of stream b holds the rotated k and the new v."""
    B, D = len(case["pos"]), case["D"]
    _, kr = rotated(case)
    kc, vc = case["kc"].clone(), case["vc"].clone()
    for b, p in enumerate(case["pos"]):
        kc[b, :, p] = kr[b]
        vc[b, :, p] = case["v"].view(B, case["Hkv"], D)[b]
    return kc, vc


def attention_fp64(case):
    """softmax(q k^T * scale) v over the visible keys in float64: (out [B, Hq D], scores, abs-score sums)."""
    B, Hq, G, D = len(case["pos"]), case["Hq"], case["G"], case["D"]
    qr, _ = rotated(case)
    kc, vc = updated_caches(case)
    out = torch.zeros(B, Hq, D, dtype=torch.float64)
    worst = 0.0
    for b in range(B):
        vis = case["visible"][b]
        for hq in range(Hq):
            kk, vv = kc[b, hq // G, vis].double(), vc[b, hq // G, vis].double()
            qd = qr[b, hq].double()
            worst = max(worst, float((kk.abs() @ qd.abs()).max() * case["scale"]))
            out[b, hq] = torch.softmax((kk @ qd) * case["scale"], 0) @ vv
    return out.reshape(B, Hq * D), worst


def attention_fp32(case, combine_weights=None):
    """The kernel's arithmetic restated in numpy float32: per 128-key chunk the maximum, exp(s - m),
    their sum and the unnormalised P V; the chunks merged with exp(m_s - M); one rounding to the
    dtype at the end.  `combine_weights`, a list, receives every merge weight."""
    f32 = np.float32
    B, Hq, G, D, L = len(case["pos"]), case["Hq"], case["G"], case["D"], case["L"]
    qr, _ = rotated(case)
    kc, vc = updated_caches(case)
    out = np.zeros((B, Hq, D), f32)
    scale = f32(case["scale"])
    for b in range(B):
        vis = case["visible"][b].numpy()
        for hq in range(Hq):
            qd = qr[b, hq].float().numpy()
            parts = []
            for j0 in range(0, L, CHUNK):
                idx = np.flatnonzero(vis[j0:j0 + CHUNK]) + j0
                if idx.size == 0:
                    continue
                kk, vv = kc[b, hq // G, idx].float().numpy(), vc[b, hq // G, idx].float().numpy()
                s = (kk @ qd).astype(f32) * scale
                m = s.max()
                e = np.exp(s - m, dtype=f32)
                parts.append((m, e.sum(dtype=f32), (e[None, :] @ vv).astype(f32)[0]))
            M = max(m for m, _, _ in parts)
            if len(parts) == 1:
                out[b, hq] = parts[0][2] / parts[0][1]
                continue
            w = [np.exp(f32(m - M), dtype=f32) for m, _, _ in parts]
            if combine_weights is not None:
                combine_weights += [float(x) for x in w]
            num = sum((wi * o for wi, (_, _, o) in zip(w, parts)), np.zeros(D, f32))
            den = sum((wi * l for wi, (_, l, _) in zip(w, parts)), f32(0))
            out[b, hq] = num / den
    return torch.from_numpy(out.reshape(B, Hq * D)).to(DTYPES[case["name"]])


def vmax(case):
    """[B, 1]: the largest visible |v| of each stream (the new token's included), float64."""
    _, vc = updated_caches(case)
    vis = case["visible"][:, None, :, None]
    return torch.where(vis, vc.double().abs(), torch.zeros((), dtype=torch.float64)).amax((1, 2, 3)).reshape(-1, 1)


# ---------------------------------------------------------------------------
# shared references and bars (float64; the GPU tests and the CPU proof use the same)
# ---------------------------------------------------------------------------

def ulp_at(y: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """One unit in the last place of `dtype` at |y| (test_gpu_layer_ops._ulp_at: eps * |y|, floored at the
    format's smallest subnormal)."""
    eps = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -23}[dtype]
    tiny = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133, torch.float32: 2.0 ** -149}[dtype]
    return torch.clamp(y.abs().double() * eps, min=tiny)


def silu64(g: torch.Tensor) -> torch.Tensor:
    """x / (1 + exp(-x)) in float64 (finite x; exp(-x) may be inf: x / inf = -0)."""
    x = g.double()
    return x / (1.0 + torch.exp(-x))


def near_boundary(y64: torch.Tensor, dtype: torch.dtype, fp32_ulps: int = 4) -> torch.Tensor:
    """True where the float64 value lies within `fp32_ulps` fp32 ulps of a rounding boundary of
    `dtype` (y - d and y + d round to different values): only there can the last place of an fp32
    intermediate decide the stored value.  Every fp32 value is its own storage: all True."""
    if dtype == torch.float32:
        return torch.ones_like(y64, dtype=torch.bool)
    d = fp32_ulps * torch.clamp(y64.abs() * 2.0 ** -23, min=2.0 ** -149)
    return (y64 - d).to(dtype) != (y64 + d).to(dtype)


def rms_norm64(x: torch.Tensor, w: torch.Tensor, eps: float, r: torch.Tensor | None = None):
    """LlamaRMSNorm.forward with torch's roundings and float64 arithmetic between them: fp32 squares
    (they overflow and underflow as fp32 does), their float64 mean rounded to fp32, + eps rounded to
    fp32, 1 / sqrt rounded to fp32, x * that rounded to fp32 and to the dtype, times the weight,
    rounded to the dtype.  With r: of s = (r + x) rounded to the dtype; returns (s, y)."""
    dt = x.dtype
    s = (r.float() + x.float()).to(dt) if r is not None else x
    sf = s.float()
    var = ((sf * sf).double().sum(-1, keepdim=True) / sf.shape[-1]).float()
    ve = (var.double() + float(np.float32(eps))).float()
    rs = (1.0 / torch.sqrt(ve.double())).float()
    h = (sf.double() * rs.double()).float().to(dt)
    y = (w.float().double() * h.float().double()).float().to(dt)
    return (s, y) if r is not None else y
