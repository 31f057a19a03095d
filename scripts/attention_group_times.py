#!/usr/bin/env python
"""Group-tiled attention (layer_ops.attention_group) beside the one-head-per-workgroup launches.

  python scripts/attention_group_times.py            # written to profiles/attention_group_times.txt

Per-call times (us) by scripts/verify_times.py's method: COPIES calls over rotating caches are captured back
to back into one graph, which is replayed between two events; three repeats, interleaved; every list is the
three repeats (median and min-max are read off it).  Llama-3-8B heads (Hq 32, Hkv 8, D 128, fp16), the window
starting at L - 64:
  verify   attention_group (key chunk 128) beside decode_attention_verify, L in {512, 4096}, T in {2, 4, 8}, B in {1, 4}
  step     attention_group (T = 1) beside decode_attention_streams
  prefill  attention_group (one pass) beside prefill_attention, a 128-token chunk at positions 0 and 8192 (L = 8320)
  g16      Hq 128 on Hkv 8 (no other launch takes it), L = 4096, T in {1, 4}: the time and the fraction of the HBM
           peak (--peak-tbs, 8.0 TB/s) that reading the visible K and V rows once in that time amounts to
"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from sample_times import graph_time_us  # noqa: E402  (scripts/ is sys.path[0])

COPIES = 16
D = 128


def _inputs(B, T, Hq, Hkv, L, g, dev):
    q = torch.randn(B, T, Hq * D, device=dev, generator=g).half()
    k = torch.randn(B, T, Hkv * D, device=dev, generator=g).half()
    v = torch.randn(B, T, Hkv * D, device=dev, generator=g).half()
    ang = torch.rand(B, T, D // 2, device=dev, generator=g) * 6.0
    cos = torch.cat((ang.cos(), ang.cos()), -1).half()
    sin = torch.cat((ang.sin(), ang.sin()), -1).half()
    caches = [(torch.randn(B, Hkv, L, D, device=dev, generator=g).half(),
               torch.randn(B, Hkv, L, D, device=dev, generator=g).half()) for _ in range(COPIES)]
    return (q, k, v, cos, sin), caches


@torch.inference_mode()
def main():
    from quantizations_amd import layer_ops as ops

    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "attention_group_times.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    scale = 1.0 / math.sqrt(D)
    lines = []

    def emit(row):
        row = {k: [round(x, 2) for x in v] if k.endswith("_us") else v for k, v in row.items()}
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    def timed(row, calls):
        """calls: name -> f(kc, vc); the repeats interleaved."""
        for name in calls:
            row[name + "_us"] = []
        for _ in range(args.repeat):
            for name, f in calls.items():
                row[name + "_us"].append(graph_time_us([lambda kc=kc, vc=vc: f(kc, vc) for kc, vc in row["_caches"]]))
        torch.cuda.synchronize()
        del row["_caches"]
        return {n: sorted(row[n + "_us"])[len(row[n + "_us"]) // 2] for n in calls}

    for L in (512, 4096):
        for B in (1, 4):
            for T in (1, 2, 4, 8):
                a, caches = _inputs(B, T, 32, 8, L, g, dev)
                pos = torch.full((B,), L - 64, dtype=torch.int64, device=dev)
                length = torch.full((B,), T, dtype=torch.int64, device=dev)
                old = ((lambda kc, vc: ops.decode_attention_streams(*a, kc, vc, pos, 32, scale)) if T == 1 else
                       (lambda kc, vc: ops.decode_attention_verify(*a, kc, vc, pos, 32, scale)))
                row = {"case": "step" if T == 1 else "verify", "B": B, "T": T, "L": L, "p": L - 64, "_caches": caches}
                med = timed(row, {"group": lambda kc, vc: ops.attention_group(*a, kc, vc, pos, length, 32, scale, 128),
                                  "rows": old})
                row["group_over_rows"] = round(med["group"] / med["rows"], 3)
                emit(row)
                del caches
    L, T = 8320, 128
    for p0 in (0, 8192):
        a, caches = _inputs(1, T, 32, 8, L, g, dev)
        pos = torch.tensor([p0], dtype=torch.int64, device=dev)
        length = torch.tensor([T], dtype=torch.int64, device=dev)
        row = {"case": "prefill", "B": 1, "T": T, "L": L, "p": p0, "_caches": caches}
        med = timed(row, {"group": lambda kc, vc: ops.attention_group(*a, kc, vc, pos, length, 32, scale, L),
                          "rows": lambda kc, vc: ops.prefill_attention(*a, kc, vc, pos, length, 32, scale)})
        row["group_over_rows"] = round(med["group"] / med["rows"], 3)
        emit(row)
        del caches
    L = 4096
    for T in (1, 4):
        a, caches = _inputs(1, T, 128, 8, L, g, dev)
        pos = torch.tensor([L - 64], dtype=torch.int64, device=dev)
        length = torch.tensor([T], dtype=torch.int64, device=dev)
        row = {"case": "g16", "B": 1, "T": T, "L": L, "p": L - 64, "Hq": 128, "Hkv": 8, "_caches": caches}
        med = timed(row, {"group": lambda kc, vc: ops.attention_group(*a, kc, vc, pos, length, 128, scale, 128)})
        row["cache_bytes"] = 2 * 8 * (L - 64 + T) * D * 2
        row["fraction_of_hbm_peak"] = round(row["cache_bytes"] / (med["group"] * 1e-6) / (args.peak_tbs * 1e12), 4)
        emit(row)
        del caches
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
