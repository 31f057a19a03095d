#!/usr/bin/env python
"""The routed mixture-of-experts launches at Mixtral-8x7B geometry: what each costs, beside one dense
gate/up pair launch and beside the composed fallback.

  python scripts/moe_times.py                       # -> profiles/moe_times.txt
  python scripts/moe_times.py --bench --parent DIR  # bench.py's line, parent and this tree in turn

H 4096, I 14336, E 8, top-k 2, NF4 + double quant, fp16; T = 1, 4, 16 rows.  The routing of each T is
drawn once from a fixed seed (distinct experts per row); `hit` is how many distinct experts it names.
us per call: COPIES calls over rotating weight / activation buffers captured back to back into one
graph and replayed between two events (scripts/sample_times.py's graph_time_us); medians of three
interleaved repeats with their min and max.  The weight copies rotate so that no call finds its
experts in the last-level cache: one copy of the hit experts at T = 1 alone is 176 MB.
  route / pair / down   qz_moe_route, qz_moe_pair_silu_4bit, qz_moe_down_4bit
  frac_hbm              bytes of the hit experts' codes and scales over the time, over HBM_PEAK_GBS
  dense_pair            qz_gemv_4bit_pair_silu on ONE dense 14336 x 4096 gate/up pair, one token: the
                        yardstick for "time per hit expert" (pair_over_dense_per_hit = pair / (hit * dense))
  composed              SparseMoe4bit's fallback on the same rows (host loop over hit experts: it
                        synchronises, so it is timed on the host clock around synchronised calls)
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from sample_times import graph_time_us  # noqa: E402  (scripts/ is sys.path[0])
from streams_times import bench_cases  # noqa: E402

H, I, E, TOPK = 4096, 14336, 8, 2
COPIES = 4
HBM_PEAK_GBS = 8000.0   # bench.py's figure for the MI355X


def _stats(xs):
    s = sorted(xs)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2)}


@torch.inference_mode()
def moe_cases(emit, repeat):
    import quantizations_amd as qa
    from quantizations_amd.core import gemv_4bit_pair_silu, moe_down, moe_pair_silu, moe_route
    from quantizations_amd.moe import SparseMoe4bit

    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    moe = SparseMoe4bit((torch.randn(E, H, device=dev, generator=g) / 64).half(),
                        (torch.randn(E, 2 * I, H, device=dev, generator=g) * 0.02).half(),
                        (torch.randn(E, H, I, device=dev, generator=g) * 0.02).half(), TOPK)
    gu_state, dn_state = moe.gate_up_proj.quant_state, moe.down_proj.quant_state
    gus = [moe.gate_up_proj.data.clone() for _ in range(COPIES)]
    dns = [moe.down_proj.data.clone() for _ in range(COPIES)]
    dense = [qa.quantize_4bit((torch.randn(I, H, device=dev, generator=g) * 0.02).half(), quant_type="nf4")
             for _ in range(2 * COPIES)]
    scale_bytes = 1.0 / 64 + 4.0 / (64 * 256)          # per weight element: one u8 per 64, one fp32 per 64 * 256
    cpu = torch.Generator().manual_seed(1234)
    for T in (1, 4, 16):
        idx = torch.stack([torch.randperm(E, generator=cpu)[:TOPK] for _ in range(T)]).to(dev, torch.int32)
        w = torch.rand(T, TOPK, generator=cpu).to(dev) + 0.1
        w = (w / w.sum(-1, keepdim=True)).contiguous()
        hit = int(idx.unique().numel())
        xs = [torch.randn(T, H, device=dev, generator=g).half() for _ in range(COPIES)]
        hs = [moe_pair_silu(xs[i], gus[i], gu_state, idx, E) for i in range(COPIES)]
        calls = {
            "route": [lambda i=i: moe_route(xs[i], moe.gate.weight, TOPK) for i in range(COPIES)],
            "pair": [lambda i=i: moe_pair_silu(xs[i], gus[i], gu_state, idx, E) for i in range(COPIES)],
            "down": [lambda i=i: moe_down(hs[i], dns[i], dn_state, idx, w, E) for i in range(COPIES)],
            "dense_pair": [lambda i=i: gemv_4bit_pair_silu(xs[i][:1], [(dense[2 * i][0], dense[2 * i][1], None),
                                                                       (dense[2 * i + 1][0], dense[2 * i + 1][1], None)])
                           for i in range(COPIES)],
        }
        assert all(f() is not None for fs in calls.values() for f in fs)
        us = {k: [] for k in calls}
        composed = []
        for _ in range(repeat):
            for k, fs in calls.items():
                us[k].append(graph_time_us(fs, reps=10))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = moe._composed(xs[0])
            torch.cuda.synchronize()
            composed.append(1e6 * (time.perf_counter() - t0))
        # the three launches against the composed form on the same rows (it routes by its own top-k)
        fast = moe._routed(xs[0])
        row = {"case": "moe", "H": H, "I": I, "E": E, "top_k": TOPK, "T": T, "hit": hit, "format": "nf4+dq", "dtype": "fp16",
               "copies": COPIES, "max_abs_fast_minus_composed": round((fast.float() - ref.float()).abs().max().item(), 5)}
        for k, v in us.items():
            row[k + "_us"] = _stats(v)
        row["composed_us_host_clock"] = _stats(composed)
        med = {k: row[k + "_us"]["median"] for k in us}
        pair_bytes = hit * 2 * I * H * (0.5 + scale_bytes)
        down_bytes = hit * H * I * (0.5 + scale_bytes)
        row["pair_frac_hbm"] = round(pair_bytes / (med["pair"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
        row["down_frac_hbm"] = round(down_bytes / (med["down"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
        row["dense_pair_frac_hbm"] = round(2 * I * H * (0.5 + scale_bytes) / (med["dense_pair"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
        row["pair_over_dense_per_hit"] = round(med["pair"] / (hit * med["dense_pair"]), 2)
        row["three_launches_us"] = round(med["route"] + med["pair"] + med["down"], 2)
        row["composed_over_three_launches"] = round(row["composed_us_host_clock"]["median"] / row["three_launches_us"], 1)
        emit(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench", action="store_true", help="only bench.py's line (with --parent: against that tree)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "moe_times.txt"))
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.bench else "w") as f:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if args.bench:
            bench_cases(emit, args)
        else:
            moe_cases(emit, args.repeat)


if __name__ == "__main__":
    main()
