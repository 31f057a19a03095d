#!/usr/bin/env python
"""The window attention launches over a ring beside the flat launches at the same positions.

  python scripts/window_attn_times.py            # -> profiles/window_attn_times.txt

Llama-3-8B heads (Hq 32, Hkv 8, D 128, fp16), W = 4096.  us per call: one call per cache copy captured back
to back into one graph and replayed between two events (scripts/sample_times.py's graph_time_us); the
copies rotate so that a pass reads at least 512 MiB of keys and values, past the last-level cache.  Medians
of three interleaved repeats with their min and max.
  decode   B = 1 and 8: decode_attention_window (ring for one token per launch) at positions 4 000, 32 000 and
           200 000; decode_attention_streams on a flat cache at position 4 000 (L = 4096) and 32 000 (L = 32 768)
  prefill  B = 1, a 128-token chunk at positions 0 / 8 192 / 32 000: prefill_attention_window (ring for 128
           tokens per launch) beside prefill_attention on a flat cache of 32 768 + 128 positions
The caches hold random finite data: a launch's time does not depend on what the visible rows contain.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from sample_times import graph_time_us  # noqa: E402  (scripts/ is sys.path[0])

HQ, HKV, D, W = 32, 8, 128, 4096
DEV = torch.device("cuda")


def _stats(xs):
    s = sorted(xs)
    return f"{s[len(s) // 2]:9.2f} us  (min {s[0]:.2f}, max {s[-1]:.2f})"


def _caches(B, L, copies, g):
    return [tuple(torch.randn(B, HKV, L, D, device=DEV, generator=g).half() for _ in range(2)) for _ in range(copies)]


def _inputs(B, T, g):
    q = torch.randn(B, T, HQ * D, device=DEV, generator=g).half()
    k, v = (torch.randn(B, T, HKV * D, device=DEV, generator=g).half() for _ in range(2))
    ang = torch.rand(B, T, D // 2, device=DEV, generator=g) * 6.0
    return q, k, v, torch.cat((ang.cos(), ang.cos()), -1).half(), torch.cat((ang.sin(), ang.sin()), -1).half()


@torch.inference_mode()
def main():
    from quantizations_amd import layer_ops as lo

    g = torch.Generator(device="cuda").manual_seed(0)
    cases = {}   # label -> list of closures, one per cache copy
    for B in (1, 8):
        x = _inputs(B, 1, g)
        for label, L, positions, win in (("window", lo.ring_size(W), (4000, 32000, 200000), True),
                                         ("streams L=4096", 4096, (4000,), False),
                                         ("streams L=32768", 32768, (32000,), False)):
            copies = max(2, -(-(512 << 20) // (2 * B * HKV * min(L, W) * D * 2)))
            caches = _caches(B, L, copies, g)
            for p in positions:
                pos = torch.full((B,), p, dtype=torch.int64, device=DEV)
                if win:
                    fns = [lambda kc=kc, vc=vc, pos=pos, x=x: lo.decode_attention_window(*x, kc, vc, pos, HQ, 0.088, W)
                           for kc, vc in caches]
                else:
                    fns = [lambda kc=kc, vc=vc, pos=pos, x=x: lo.decode_attention_streams(*x, kc, vc, pos, HQ, 0.088)
                           for kc, vc in caches]
                cases[f"decode  B={B} {label:16s} pos {p:6d}"] = fns
    x = _inputs(1, 128, g)
    n = torch.full((1,), 128, dtype=torch.int64, device=DEV)
    for label, L, win in (("window", lo.ring_size(W, 128), True), ("flat L=32896", 32768 + 128, False)):
        caches = _caches(1, L, 8, g)
        for p in (0, 8192, 32000):
            pos = torch.full((1,), p, dtype=torch.int64, device=DEV)
            if win:
                fns = [lambda kc=kc, vc=vc, pos=pos, x=x: lo.prefill_attention_window(*x, kc, vc, pos, n, HQ, 0.088, W)
                       for kc, vc in caches]
            else:
                fns = [lambda kc=kc, vc=vc, pos=pos, x=x: lo.prefill_attention(*x, kc, vc, pos, n, HQ, 0.088)
                       for kc, vc in caches]
            cases[f"prefill B=1 {label:16s} pos {p:6d}"] = fns
    times = {k: [] for k in cases}
    for _ in range(3):                       # interleaved repeats
        for k, fns in cases.items():
            times[k].append(graph_time_us(fns))
    lines = [__doc__.strip().splitlines()[0], ""] + [f"{k}: {_stats(v)}" for k, v in times.items()]
    out = os.path.join(REPO, "profiles", "window_attn_times.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
