"""Shared by the prefill attention tests (GPU and CPU): seeded CPU inputs for a window of T tokens per
stream, a float64 reference, and a numpy-float32 restatement of qz_prefill_attention's order of
operations -- key tiles of TK keys from absolute position 0, online softmax (running maximum, rescale
by exp(m_old - m_new), fp32 row sum of the unrounded probabilities), P rounded to the storage dtype
as the P V operand, fp32 accumulation, one division and one rounding at the end.

Inputs are generated on the CPU so the CPU proof (test_prefill_reference_cpu.py) sees the very values
the GPU test moves to the device."""
import math

import numpy as np
import torch
import activation_families as af

TQ = 64   # layer_ops.PREFILL_TQ (asserted equal by the tests that import the package)
TK = 64   # layer_ops.PREFILL_TK
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
TOL = {"fp16": 2e-3, "bf16": 1e-2}   # test_gpu_decode_attention_verify.py's bars


def window_lengths(T):
    """Lengths 0, 1, T - 1 and T in one call (clamped to [0, T], in this order)."""
    return [T, max(T - 1, 0), min(1, T), 0]


def window_starts(L, T):
    """The issue's window starts; the last runs off the end."""
    return [0, TK - 1, TK, TK + 1, L - T, L - 2]


def make_case(B, T, Hq, Hkv, D, L, ps, lens, name, seed, nan_above=True):
    """CPU tensors: q [B, T, Hq D], k / v [B, T, Hkv D], cos / sin [B, T, D] (a rotary row per token
    row), caches [B, Hkv, L, D] with NaN at and above pos[b] (so one key too many shows)."""
    dt = DTYPES[name]
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, T, Hq * D, generator=g).to(dt)
    k = torch.randn(B, T, Hkv * D, generator=g).to(dt)
    v = torch.randn(B, T, Hkv * D, generator=g).to(dt)
    ang = torch.rand(B, T, D // 2, generator=g) * 6.0
    cos = torch.cat((ang.cos(), ang.cos()), -1).to(dt)
    sin = torch.cat((ang.sin(), ang.sin()), -1).to(dt)
    kc = torch.randn(B, Hkv, L, D, generator=g).to(dt)
    vc = torch.randn(B, Hkv, L, D, generator=g).to(dt)
    if nan_above:
        for b, p in enumerate(ps):
            if 0 <= p < L:
                kc[b, :, p:] = float("nan")
                vc[b, :, p:] = float("nan")
    return dict(B=B, T=T, Hq=Hq, Hkv=Hkv, D=D, L=L, name=name, pos=list(ps), len=list(lens),
                scale=1.0 / math.sqrt(D), q=q, k=k, v=v, cos=cos, sin=sin, kc=kc, vc=vc)


def _rotate_half(x):
    x1, x2 = x[..., : x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


def rotated(case):
    """(q [B, T, Hq, D], k [B, T, Hkv, D]) after apply_rotary_pos_emb, torch's per-op rounding in the dtype."""
    B, T, D = case["B"], case["T"], case["D"]
    qh, kh = case["q"].view(B, T, case["Hq"], D), case["k"].view(B, T, case["Hkv"], D)
    c, s = case["cos"].unsqueeze(2), case["sin"].unsqueeze(2)
    return (qh * c) + (_rotate_half(qh) * s), (kh * c) + (_rotate_half(kh) * s)


def legal_rows(case, b):
    """Number of rows of stream b that are computed: real (i < len) and inside the cache."""
    p, n, L = case["pos"][b], case["len"][b], case["L"]
    if p < 0 or p >= L:
        return 0
    return max(0, min(n, case["T"], L - p))


def updated_caches(case):
    """The caches after the call: slots pos[b] .. pos[b] + legal - 1 hold the rotated k and the new v."""
    _, kr = rotated(case)
    kc, vc = case["kc"].clone(), case["vc"].clone()
    vh = case["v"].view(case["B"], case["T"], case["Hkv"], case["D"])
    for b, p in enumerate(case["pos"]):
        n = legal_rows(case, b)
        if n:
            kc[b, :, p:p + n] = kr[b, :n].transpose(0, 1)
            vc[b, :, p:p + n] = vh[b, :n].transpose(0, 1)
    return kc, vc


def expected_fill(case):
    """[B, T] of 'ok' / 'nan' / 'zero': what each output row must be."""
    out = []
    for b in range(case["B"]):
        n = legal_rows(case, b)
        real = max(0, min(case["len"][b], case["T"]))
        out.append(["ok" if i < n else "nan" if i < real else "zero" for i in range(case["T"])])
    return out


def reference_fp64(case):
    """softmax(q k^T * scale) v over keys 0 .. pos[b] + i in float64: [B, T, Hq D]; NaN for real rows
    at a bad position, zeros for padding rows."""
    B, T, Hq, Hkv, D = case["B"], case["T"], case["Hq"], case["Hkv"], case["D"]
    G = Hq // Hkv
    qr, _ = rotated(case)
    kc, vc = updated_caches(case)
    fill = expected_fill(case)
    out = torch.zeros(B, T, Hq, D, dtype=torch.float64)
    for b in range(B):
        for i in range(T):
            if fill[b][i] != "ok":
                out[b, i] = float("nan") if fill[b][i] == "nan" else 0.0
                continue
            n = case["pos"][b] + i + 1
            kk = kc[b, :, :n].double().repeat_interleave(G, 0)       # [Hq, n, D]
            vv = vc[b, :, :n].double().repeat_interleave(G, 0)
            sc = torch.einsum("hd,hnd->hn", qr[b, i].double(), kk) * case["scale"]
            out[b, i] = torch.einsum("hn,hnd->hd", torch.softmax(sc, -1), vv)
    return out.reshape(B, T, Hq * D)


def _round(x32, dt):
    return torch.from_numpy(np.ascontiguousarray(x32)).to(dt).float().numpy()


def restatement_f32(case, tk=TK):
    """The kernel's order in numpy float32 (see the module docstring): (out [B, T, Hq D] in the dtype,
    kc, vc after the call)."""
    f32 = np.float32
    B, T, Hq, Hkv, D = case["B"], case["T"], case["Hq"], case["Hkv"], case["D"]
    G = Hq // Hkv
    dt = DTYPES[case["name"]]
    qr, _ = rotated(case)
    kc, vc = updated_caches(case)
    kn, vn = kc.float().numpy(), vc.float().numpy()
    fill = expected_fill(case)
    scale = f32(case["scale"])
    out = np.zeros((B, T, Hq, D), f32)
    for b in range(B):
        for i in range(T):
            if fill[b][i] != "ok":
                out[b, i] = f32("nan") if fill[b][i] == "nan" else f32(0)
                continue
            p = case["pos"][b] + i
            qd = qr[b, i].float().numpy()                            # [Hq, D]
            m = np.full(Hq, -np.inf, f32)
            l = np.zeros(Hq, f32)
            o = np.zeros((Hq, D), f32)
            for j0 in range(0, p + 1, tk):
                j1 = min(j0 + tk, p + 1)
                kk = np.repeat(kn[b, :, j0:j1], G, 0)                # [Hq, n, D]
                vv = np.repeat(vn[b, :, j0:j1], G, 0)
                s = np.einsum("hd,hnd->hn", qd, kk).astype(f32) * scale
                mn = np.maximum(m, s.max(1))
                alpha = np.exp(m - mn, dtype=f32)
                e = np.exp(s - mn[:, None], dtype=f32)
                l = l * alpha + e.sum(1, dtype=f32)
                o = o * alpha[:, None] + np.einsum("hn,hnd->hd", _round(e, dt), vv).astype(f32)
                m = mn
            out[b, i] = o / l[:, None]
    return torch.from_numpy(out.reshape(B, T, Hq * D)).to(dt), kc, vc


def split_case(case, split):
    """The window as two calls split at row `split`: (first, second), the second at pos + split on the
    caches the first leaves (the caller passes them on)."""
    def part(lo, hi, ps, lens):
        c = dict(case)
        c["T"] = hi - lo
        for n in ("q", "k", "v", "cos", "sin"):
            c[n] = case[n][:, lo:hi].contiguous()
        c["pos"], c["len"] = ps, lens
        return c
    T = case["T"]
    first = part(0, split, list(case["pos"]), [min(n, split) for n in case["len"]])
    second = part(split, T, [p + split for p in case["pos"]], [max(0, n - split) for n in case["len"]])
    return first, second


def splits_of(T):
    """Rows 1, TQ - 1, TQ and ceil(T / 2), those that lie inside the window."""
    return sorted({s for s in (1, TQ - 1, TQ, -(-T // 2)) if 0 < s < T})


# the inputs of the value checks: the GPU test runs the kernel on them, the CPU test the restatement
VALUE_CASES = [(4, 2, 64, TK + 2, TQ - 1), (8, 1, 128, 3 * TK + 5, TQ + 1), (4, 2, 128, 3 * TK + 5, 2 * TQ + 3)]
FAMILY_CASES = [("sink", "fp16"), ("sink", "bf16"), ("big_v", "fp16"), ("big_v", "bf16"), ("sub16", "fp16"),
                ("sub16_q", "bf16")]


def value_case(name, Hq, Hkv, D, L, T):
    ps = [0, TK - 1, TK + 1, L - T]
    return make_case(4, T, Hq, Hkv, D, L, ps, window_lengths(T), name, seed=3 * L + D + T)


def family_case(family, name, D):
    """One of activation_families' attention families, one token per stream (T = 1, len = 1)."""
    L = 3 * TK + 5
    return af.attention_case(family, name, 4, 2, D, L, [5, TK - 1, TK, L - 1])


def family_as_window(c):
    """An activation_families case as a make_case dict (T = 1, len = 1)."""
    B = len(c["pos"])
    return dict(B=B, T=1, Hq=c["Hq"], Hkv=c["Hkv"], D=c["D"], L=c["L"], name=c["name"], pos=list(c["pos"]),
                len=[1] * B, scale=c["scale"], q=c["q"], k=c["k"], v=c["v"], cos=c["cos"], sin=c["sin"],
                kc=c["kc"], vc=c["vc"])
