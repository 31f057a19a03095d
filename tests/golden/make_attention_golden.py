"""The decode attention bit fixture: tests/golden/decode_attention_parent.npz.

  python tests/golden/make_attention_golden.py --tree PATH/TO/CHECKOUT --out decode_attention_parent.npz

Run ONCE, on an MI355X, against the built library of the commit BEFORE the wave-local decode head (a
`git worktree` of it, built with the same toolchain): every case below is launched there and the bytes
of its output and of the cache rows it wrote are stored.  tests/test_gpu_attention_bits.py launches the
same cases on the working tree and compares bytes.  Inputs come from numpy.random.default_rng(seed), so
the test regenerates them; the fixture holds results only (and the ROCm version that produced them).

cases() is the list; run_case() launches one against whichever quantizations_amd is importable.
"""
import argparse
import math
import os
import sys

import numpy as np

HKV = 2
SEAMS = (0, 31, 32, 63, 64)          # the wave seams of a chunk: the owner of the new key changes here
LENGTHS = (1, 2, 31, 32, 33, 64, 127, 128, 129, 257)


def cases():
    """[(name, spec dict)] -- the order is the fixture's."""
    out = []
    n = 0
    gs, bs = (1, 4, 8), (1, 3)
    for dt in ("f16", "bf16"):
        for D in (64, 128):
            # every cache length, the new token at a seam or at the end, G and B taking turns
            for L in LENGTHS:
                ps = sorted({p for p in SEAMS if p < L} | {L - 1})
                p = ps[n % len(ps)]
                G, B = gs[n % 3], (bs[1] if n % 7 == 3 else bs[0])   # B = 3 on every seventh: the fixture stays small
                out.append((f"shared-{dt}-D{D}-G{G}-B{B}-L{L}-p{p}", dict(form="shared", dt=dt, D=D, G=G, B=B, L=L, p=p)))
                n += 1
    # every seam position in one full chunk and in the second of three chunks
    for dt, D in (("f16", 128), ("bf16", 64)):
        for L, base in ((128, 0), (257, 128)):
            for p in SEAMS + (127,):
                G = gs[n % 2]
                n += 1
                name = f"shared-{dt}-D{D}-G{G}-B1-L{L}-p{base + p}"
                if all(name != c[0] for c in out):
                    out.append((name, dict(form="shared", dt=dt, D=D, G=G, B=1, L=L, p=base + p)))
    # masks: holes at the seams, one whole wave masked, everything masked but the new token
    for dt, D in (("f16", 128), ("bf16", 64)):
        out.append((f"holes-{dt}-D{D}", dict(form="shared", dt=dt, D=D, G=4, B=1, L=128, p=127,
                                              hide=(31, 32, 63, 64, 95, 96))))
        out.append((f"wave-masked-{dt}-D{D}", dict(form="shared", dt=dt, D=D, G=4, B=1, L=128, p=127,
                                                    hide=tuple(range(32, 64)))))
        out.append((f"only-new-{dt}-D{D}", dict(form="shared", dt=dt, D=D, G=4, B=1, L=128, p=64,
                                                 hide=tuple(range(64)))))
    # the other forms
    out.append(("streams-f16-D128", dict(form="streams", dt="f16", D=128, G=4, B=3, L=129, pos=(5, 64, 128))))
    out.append(("streams-bf16-D64", dict(form="streams", dt="bf16", D=64, G=8, B=3, L=96, pos=(31, 32, 95))))
    out.append(("verify-T2-f16-D128", dict(form="verify", dt="f16", D=128, G=4, B=2, L=129, T=2, pos=(31, 127))))
    out.append(("verify-T4-bf16-D64", dict(form="verify", dt="bf16", D=64, G=1, B=2, L=100, T=4, pos=(61, 0))))
    out.append(("paged-f16-D128", dict(form="paged", dt="f16", D=128, G=4, B=2, NP=2, P=5, pos=(63, 200))))
    out.append(("kv8-f16-D128", dict(form="kv8", dt="f16", D=128, G=4, B=2, NP=2, P=5, pos=(64, 131), nonfinite=True)))
    out.append(("kv8-bf16-D64", dict(form="kv8", dt="bf16", D=64, G=8, B=1, NP=1, P=3, pos=(32,), nonfinite=False)))
    return out


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31)


def _t(rng, shape, dtype, dev):
    import torch

    return torch.from_numpy(rng.standard_normal(shape, dtype=np.float32)).to(dev).to(dtype)


def _bytes(t):
    import torch

    return t.contiguous().view(torch.uint8).cpu().numpy().ravel()


def run_case(name, s):
    """Launch the case; the bytes of the output and of the cache rows it wrote, concatenated."""
    import torch

    from quantizations_amd import layer_ops as lo

    dev = torch.device("cuda")
    dtype = torch.float16 if s["dt"] == "f16" else torch.bfloat16
    rng = np.random.default_rng(_seed(name))
    D, G, B = s["D"], s["G"], s["B"]
    Hq = G * HKV
    T = s.get("T", 1)
    scale = 1.0 / math.sqrt(D)
    q = _t(rng, (B, T, Hq * D), dtype, dev)
    k = _t(rng, (B, T, HKV * D), dtype, dev)
    v = _t(rng, (B, T, HKV * D), dtype, dev)
    ang = torch.from_numpy(rng.uniform(0.0, 6.0, (B, T, D // 2)).astype(np.float32)).to(dev)
    cos = torch.cat((ang.cos(), ang.cos()), -1).to(dtype)
    sin = torch.cat((ang.sin(), ang.sin()), -1).to(dtype)
    form = s["form"]
    if form == "shared":
        L, p = s["L"], s["p"]
        kc, vc = _t(rng, (B, HKV, L, D), dtype, dev), _t(rng, (B, HKV, L, D), dtype, dev)
        mask = torch.zeros(1, 1, 1, L, dtype=torch.bool, device=dev)
        mask[..., : p + 1] = True
        for j in s.get("hide", ()):
            mask[..., j] = False
        pos = torch.tensor(p, dtype=torch.int64, device=dev)
        arrive = torch.zeros(1, dtype=torch.int32, device=dev)
        out = lo.decode_attention(q, k, v, cos[:1], sin[:1], kc, vc, mask, pos, arrive, Hq, scale)
        torch.cuda.synchronize()
        assert int(pos) == p + 1 and int(arrive) == 0
        return np.concatenate([_bytes(out), _bytes(kc[:, :, p]), _bytes(vc[:, :, p])])
    pos = torch.tensor(s["pos"], dtype=torch.int64, device=dev)
    if form in ("streams", "verify"):
        L = s["L"]
        kc, vc = _t(rng, (B, HKV, L, D), dtype, dev), _t(rng, (B, HKV, L, D), dtype, dev)
        if form == "streams":
            out = lo.decode_attention_streams(q, k, v, cos, sin, kc, vc, pos, Hq, scale)
        else:
            out = lo.decode_attention_verify(q, k, v, cos, sin, kc, vc, pos, Hq, scale)
        torch.cuda.synchronize()
        rows = [t[b, :, s["pos"][b]: s["pos"][b] + T] for t in (kc, vc) for b in range(B)]
        return np.concatenate([_bytes(out)] + [_bytes(r) for r in rows])
    NP, P = s["NP"], s["P"]
    perm = rng.permutation(P)[: B * NP].astype(np.int32).reshape(B, NP)   # distinct pages, shuffled
    table = torch.from_numpy(perm).to(dev)
    if form == "paged":
        kp, vp = _t(rng, (P, HKV, 128, D), dtype, dev), _t(rng, (P, HKV, 128, D), dtype, dev)
        out = lo.decode_attention_paged(q, k, v, cos, sin, kp, vp, table, pos, Hq, scale)
        torch.cuda.synchronize()
        rows = [t[int(perm[b, s["pos"][b] >> 7]), :, s["pos"][b] & 127] for t in (kp, vp) for b in range(B)]
        return np.concatenate([_bytes(out)] + [_bytes(r) for r in rows])
    # kv8: D code bytes per row (no NaN codes), then the rows' scale bytes near 2^0; one visible non-finite row
    def pool():
        codes = rng.integers(0, 256, (P, HKV, 128, D), dtype=np.uint8)
        codes[(codes & 0x7F) == 0x7F] = 0x3C
        scales = rng.integers(122, 131, (P, HKV, 128), dtype=np.uint8)
        return codes, scales
    (kcodes, kscales), (vcodes, vscales) = pool(), pool()
    if s["nonfinite"]:
        kscales[int(perm[0, 0]), 0, 7] = 255     # key 7 of stream 0, kv head 0: every value NaN
    kp = torch.from_numpy(np.concatenate([kcodes.reshape(P, HKV, -1), kscales], axis=2)).to(dev)
    vp = torch.from_numpy(np.concatenate([vcodes.reshape(P, HKV, -1), vscales], axis=2)).to(dev)
    out = lo.decode_attention_paged_kv8(q, k, v, cos, sin, kp, vp, table, pos, Hq, scale)
    torch.cuda.synchronize()
    rows = []
    for t in (kp, vp):
        for b in range(B):
            blk, slot = t[int(perm[b, s["pos"][b] >> 7])], s["pos"][b] & 127
            rows += [blk[:, slot * D: (slot + 1) * D], blk[:, 128 * D + slot: 128 * D + slot + 1]]
    return np.concatenate([_bytes(out)] + [_bytes(r) for r in rows])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True, help="the checkout whose built quantizations_amd is recorded")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch

    import quantizations_amd

    assert os.path.abspath(quantizations_amd.__file__).startswith(os.path.abspath(a.tree)), quantizations_amd.__file__
    names, chunks = [], []
    for name, spec in cases():
        names.append(name)
        chunks.append(run_case(name, spec))
    sizes = np.array([c.size for c in chunks], dtype=np.int64)
    np.savez_compressed(a.out, names=np.array(names), sizes=sizes, data=np.concatenate(chunks),
                        rocm=np.array(str(torch.version.hip)), device=np.array(torch.cuda.get_device_name(0)))
    print(f"{len(names)} cases, {int(sizes.sum())} bytes of results, ROCm {torch.version.hip} -> {a.out}")


if __name__ == "__main__":
    main()
